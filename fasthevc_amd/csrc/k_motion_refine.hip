// k_motion_refine.hip -- source-only quarter-sample refinement of the motion search per CU node (config 4: P slices), gfx950 only.
//
// Twin of TEncSearch::xPatternSearchFracDIF + xPatternRefinement (TEncSearch.cpp:4370-4406, :823-877; candidate tables :51-75): around the
// integer vector of every CU node (85 per CTU, as k_motion.hip writes them) a half-sample and then a quarter-sample stage of nine candidates
// each, strict "<" in the order of s_acMvRefineH / s_acMvRefineQ, cost = Hadamard distortion (TComRdCost::xGetHADs: the node's 8x8 tile
// Hadamards, (sum + 2) >> 2 each, the node's sum >> (bit depth - 8) once) + getCostOfVectorWithPredictor (zero predictor; bits of the vector in
// QUARTER units in both stages: cost scale 1 on half units, 0 on quarter units), on HEVC's 8-tap luma interpolation of the PREVIOUS ORIGINAL
// picture with coordinates clamped to the picture (TComPicYuv::extendPicBorder).
//
// Interpolation (TComInterpolationFilter::filter, xExtDIFUpSamplingH / Q): ONE form serves the four cases.  With c_0 = {0,0,0,64,0,0,0,0}
//   t = (sum c_fx s >> (bd - 8)) - 8192 over rows y-3 .. y+4,  sample = clip((sum c_fy t + (1 << (19 - bd)) + (8192 << 6)) >> (20 - bd))
// is what the reference computes when both fractions are non-zero, and for fy = 0 it collapses to ((sum c_fx s >> (bd - 8)) + (1 << (13 - bd)))
// >> (14 - bd) = (sum c_fx s + 32) >> 6 (nested floors of integers), for fx = 0 to the reference's own vertical pass behind its 14-bit copy,
// for fx = fy = 0 to the sample itself.  So the fractions are DATA (two packed coefficient vectors per lane), not control flow: the
// quarter stage starts from each node's own half-sample winner, and the lanes of a wave need not agree on a phase.
//
// Mapping: workgroup (4 waves) = one CTU at a time, grid-stride; wave = level (64x64, 32x32, 16x16, 8x8), lane = one 8x8 tile: every level
// covers the same 64 tiles, so the waves are balanced.  A lane keeps its 64 original samples as 32 packed pairs, reads the window of ITS node's
// candidate from LDS (the reference window of (64 + 2 MR + 8)^2 samples, border replicated, staged once per CTU; aligned dword reads +
// v_alignbit, as k_motion.hip), filters it with v_dot2_i32_i16 (two taps per instruction: horizontally on pairs of neighbouring samples,
// vertically on pairs of rows of the 16-bit intermediates), runs the Hadamard of k_had8x8.h, and the tiles of a node meet through lane
// shuffles.  The candidate loop is wave-uniform; a wave whose lanes all have a zero fraction in one direction skips that filter's arithmetic.
// No scratch, no HBM state between calls: the vector costs travel by value (cost by number of bits, 40 entries).
#include "fhevc_internal.h"
#include "k_had8x8.h"
#include "k_refine_tile.h"

namespace {

// T = int16_t (HM Pel planes) or uint8_t; PACKED = bit depth <= 10 (the packed Hadamard); MR = 8 or 64: the largest integer vector the window is laid out for
// CENTRED (fhevc_motion_refine_pu_centred; MR = 8): the window of every CTU is staged around that CTU's centre P (k_search_tile.h: SearchCentre) and the kernel
// works on vectors RELATIVE to P -- an input vector is valid iff |mv - P| <= max_range, the cost of a candidate q is that of q - 4 P, which is
// getCostOfVectorWithPredictor with the predictor 4 P -- and adds 4 P to the winner.  The samples a candidate reads are those of the absolute vector
template <typename T, bool PACKED, int MR, bool CENTRED = false>
__global__ __launch_bounds__(256) void fhevc_motion_refine_kernel(FhevcFrames F, int max_range, FhevcMvBitCost cost, const FhevcMotionNode* __restrict__ nodes,
                                                                  FhevcMotionQpelNode* __restrict__ out, SearchCentres<CENTRED> centres)
{
  constexpr int RP = RefineGeom<MR>::RP;
  constexpr bool BIG = MR > FHEVC_MOTION_MAX_RANGE;
  extern __shared__ __attribute__((aligned(16))) short s_dyn[];
  __shared__ __attribute__((aligned(16))) short s_small[BIG ? 8 : RefineGeom<MR>::SAMPLES];
  short* const s_ref = BIG ? s_dyn : s_small;
  __shared__ unsigned s_cost[FHEVC_MV_BIT_COSTS], s_taps[16];
  const int tid = threadIdx.x, lane = tid & 63, lvl = tid >> 6;
  const int tx = lane & 7, ty = lane >> 3;
  const int total = SearchWork::total(F);  // frame f >= 1 is refined in frame f - 1
  const int shift = F.bit_depth - 8;
  const RefineArith arith(F.bit_depth);
  const T* plane = reinterpret_cast<const T*>(F.luma);
  if (tid < FHEVC_MV_BIT_COSTS) s_cost[tid] = cost.c[tid];
  if (tid < 16) s_taps[tid] = kLumaTaps[tid];
  const RefineNode N(lvl, tx, ty);  // this lane's node: level lvl, (nbx, nby) in the CTU

  for (int work = blockIdx.x; work < total; work += gridDim.x) {
    const SearchWork W(F, work);
    const int cy = W.cy, cx = W.cx;
    const long long oc = W.oc(F);
    SearchCentre P;
    if constexpr (CENTRED) {
      P = SearchCentre(centres, oc);
      if (!P.in_range()) {  // uniform: every node of this CTU gets the marker, nothing is read for it
        if (N.writer) out[oc * FHEVC_NODES + N.nidx] = refine_record(false, 0, 0, 0, 0, 0);
        continue;
      }
    }
    // ---- stage the reference window: rows cy*64 - MR - 4 .., columns cx*64 - MR - 4 .., coordinates clamped to the picture ----
    __syncthreads();  // the previous CTU's readers are done
    if constexpr (CENTRED) refine_stage_window<T, MR>(s_ref, plane, W.ref_base, F, cx, cy, tid, P.x, P.y);
    else refine_stage_window<T, MR>(s_ref, plane, W.ref_base, F, cx, cy, tid);
    // ---- this lane's original 8x8 tile (all four waves hold the same 64 tiles) ----
    const int px = cx * 64 + tx * 8, py = cy * 64 + ty * 8;
    const bool inside = (px + 8 <= F.width) && (py + 8 <= F.height);
    unsigned O[32];
    load_tile8x8(plane, W.cur_base, F, px, py, inside, O);
    // ---- its node's integer vector: only mvx / mvy of the input are read, validity comes from the geometry and from max_range ----
    int mx = 0, my = 0;
    bool valid = false;
    if (search_node_inside(F, cx, cy, N.nbx, N.nby, 64 >> lvl)) {
      const unsigned w = reinterpret_cast<const unsigned*>(nodes)[(oc * FHEVC_NODES + N.nidx) * 4 + 3];
      mx = vec_x(w); my = vec_y(w);
      if constexpr (CENTRED) { mx -= P.x; my -= P.y; }
      valid = abs(mx) <= max_range && abs(my) <= max_range;
      if (!valid) { mx = 0; my = 0; }  // the arithmetic below stays inside the window; its result is dropped
    }
    __syncthreads();

    int base_x = 4 * mx, base_y = 4 * my;      // quarter units
    int best_x = base_x, best_y = base_y;
    unsigned best_c = 0xFFFFFFFFu, best_s = 0, satd_int = 0;
#pragma unroll 1
    for (int i = 0; i < 18; ++i) {
      if (i == 9) { base_x = best_x; base_y = best_y; best_c = 0xFFFFFFFFu; }  // the quarter stage starts from the half stage's winner
      const int step = i < 9 ? 2 : 1;
      const int qx = base_x + step * (int)kRefineX[i], qy = base_y + step * (int)kRefineY[i];
      // ---- the tile's prediction at the candidate, its difference to the original, Hadamard (k_refine_tile.h); the node's sum ----
      unsigned t8;
      {
        unsigned D[32];
        int v[64];
        refine_tile_at<PACKED, RP>(s_ref, s_taps, arith, tx, ty, qx, qy, O, D, v);
        t8 = refine_had8x8<PACKED>(D, v, inside);
      }
      const unsigned sd = refine_node_sum(t8, lvl) >> shift;  // DISTORTION_PRECISION_ADJUSTMENT on the block's sum (TComRdCost.cpp:1823)
      const unsigned c = sd + s_cost[eg_bits(qx) + eg_bits(qy)];
      if (i == 0) satd_int = sd;
      if (c < best_c) { best_c = c; best_s = sd; best_x = qx; best_y = qy; }
    }
    if (N.writer) {
      if constexpr (CENTRED) { best_x += 4 * P.x; best_y += 4 * P.y; }
      out[oc * FHEVC_NODES + N.nidx] = refine_record(valid, satd_int, best_s, best_c, best_x, best_y);
    }
  }
}

}  // namespace

// the MR = 8 layout around one centre per CTU (behind fhevc_motion_refine_pu_centred): max_range 1 .. FHEVC_MOTION_MAX_RANGE
hipError_t fhevc_launch_motion_refine_centred(const FhevcFrames& fr, int max_range, const FhevcMvBitCost& cost, const FhevcMotionNode* d_centres, const FhevcMotionNode* d_nodes,
                                              FhevcMotionQpelNode* d_out, int num_cus, hipStream_t stream)
{
  return refine_launch<FHEVC_MOTION_MAX_RANGE>(fr, d_centres != nullptr, max_range, num_cus, {4, false}, {}, stream, [&](auto t, auto packed, auto mr, const RefineLaunch& L) {
    return refine_launch_kernel<&fhevc_motion_refine_kernel<decltype(t), decltype(packed)::value, decltype(mr)::value, true>>(L, fr, max_range, cost, d_nodes, d_out, d_centres);
  });
}

// four workgroups per CU at MR = 8; at MR = 64 the window of 80 016 B leaves one workgroup per CU beside another kernel's, two alone
hipError_t fhevc_launch_motion_refine(const FhevcFrames& fr, int max_range, const FhevcMvBitCost& cost, const FhevcMotionNode* d_nodes, FhevcMotionQpelNode* d_out,
                                      int num_cus, hipStream_t stream)
{
  return refine_launch<FHEVC_MOTION_WIDE_MAX_RANGE>(fr, true, max_range, num_cus, {4, false}, {2, false}, stream, [&](auto t, auto packed, auto mr, const RefineLaunch& L) {
    return refine_launch_kernel<&fhevc_motion_refine_kernel<decltype(t), decltype(packed)::value, decltype(mr)::value>>(L, fr, max_range, cost, d_nodes, d_out, SearchNoCentres{});
  });
}
