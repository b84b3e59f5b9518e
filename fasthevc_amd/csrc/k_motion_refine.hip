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
  const int band_rows = F.row_end - F.row_begin;
  const int per_frame = band_rows * F.ctus_x;
  const int total = per_frame * (F.num_frames - 1);  // frame f >= 1 is refined in frame f - 1
  const int bd = F.bit_depth;
  const int shift = bd - 8;
  const RefineArith arith(bd);
  const T* plane = reinterpret_cast<const T*>(F.luma);
  if (tid < FHEVC_MV_BIT_COSTS) s_cost[tid] = cost.c[tid];
  if (tid < 16) s_taps[tid] = kLumaTaps[tid];
  // this lane's node: level lvl, (nbx, nby) in the CTU
  const int nsize = 64 >> lvl, ncnt = 1 << lvl;
  const int nbx = tx >> (3 - lvl), nby = ty >> (3 - lvl);
  const int nidx = ((1 << (2 * lvl)) - 1) / 3 + nby * ncnt + nbx;
  const bool writer = (tx & ((8 >> lvl) - 1)) == 0 && (ty & ((8 >> lvl) - 1)) == 0;

  for (int work = blockIdx.x; work < total; work += gridDim.x) {
    const int f = 1 + work / per_frame;
    const int rem = work % per_frame;
    const int cy = F.row_begin + rem / F.ctus_x, cx = rem % F.ctus_x;
    const long long cur_base = (long long)f * F.frame_stride, ref_base = (long long)(f - 1) * F.frame_stride;
    const long long oc = (long long)((f - 1) * band_rows + (cy - F.row_begin)) * F.ctus_x + cx;
    SearchCentre P;
    if constexpr (CENTRED) {
      P = SearchCentre(centres, oc);
      if (!P.in_range()) {  // uniform: every node of this CTU gets the marker, nothing is read for it
        if (writer) { FhevcMotionQpelNode o; o.satd_int = o.satd_best = o.cost_best = 0xFFFFFFFFu; o.mvx = 0; o.mvy = 0; out[oc * FHEVC_NODES + nidx] = o; }
        continue;
      }
    }
    // ---- stage the reference window: rows cy*64 - MR - 4 .., columns cx*64 - MR - 4 .., coordinates clamped to the picture ----
    __syncthreads();  // the previous CTU's readers are done
    if constexpr (CENTRED) refine_stage_window<T, MR>(s_ref, plane, ref_base, F, cx, cy, tid, P.x, P.y);
    else refine_stage_window<T, MR>(s_ref, plane, ref_base, F, cx, cy, tid);
    // ---- this lane's original 8x8 tile (all four waves hold the same 64 tiles) ----
    const int px = cx * 64 + tx * 8, py = cy * 64 + ty * 8;
    const bool inside = (px + 8 <= F.width) && (py + 8 <= F.height);
    unsigned O[32];
    load_tile8x8(plane, cur_base, F, px, py, inside, O);
    // ---- its node's integer vector: only mvx / mvy of the input are read, validity comes from the geometry and from max_range ----
    const bool node_in = cx * 64 + nbx * nsize + nsize <= F.width && cy * 64 + nby * nsize + nsize <= F.height;
    int mx = 0, my = 0;
    bool valid = false;
    if (node_in) {
      const unsigned w = reinterpret_cast<const unsigned*>(nodes)[(oc * FHEVC_NODES + nidx) * 4 + 3];
      mx = (int)(short)(w & 0xFFFFu); my = (int)(short)(w >> 16);
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
      const int fx = qx & 3, fy = qy & 3;
      const int col = tx * 8 + MR + 4 + (qx >> 2) - 3, row0 = ty * 8 + MR + 4 + (qy >> 2) - 3;  // first tap of sample (0, 0)
      // ---- the tile's prediction at the candidate, its difference to the original (k_refine_tile.h), Hadamard ----
      unsigned t8;
      {
        unsigned D[32];
        int v[64];
        refine_tile_diff<PACKED, RP>(s_ref, s_taps, arith, col, row0, fx, fy, O, D, v);
        if constexpr (PACKED) t8 = had8x8_packed(D);
        else t8 = had8x8_wide(v);
      }
      t8 = inside ? ((t8 + 2) >> 2) : 0u;  // xCalcHADs8x8: (sum + 2) >> 2 (TComRdCost.cpp:1747)
      // the node's sum: 16x16 = tiles (tx ^ 1, ty ^ 1), 32x32 = + bits 1, 64x64 = + bits 2 (wave-uniform depth)
      unsigned s = t8;
      for (int k = 0; k < 3 - lvl; ++k) {
        s += __shfl_xor(s, 1 << k);
        s += __shfl_xor(s, 8 << k);
      }
      const unsigned sd = s >> shift;  // DISTORTION_PRECISION_ADJUSTMENT on the block's sum (TComRdCost.cpp:1823)
      const unsigned c = sd + s_cost[eg_bits(qx) + eg_bits(qy)];
      if (i == 0) satd_int = sd;
      if (c < best_c) { best_c = c; best_s = sd; best_x = qx; best_y = qy; }
    }
    if (writer) {
      FhevcMotionQpelNode o;
      if constexpr (CENTRED) { best_x += 4 * P.x; best_y += 4 * P.y; }
      if (valid) { o.satd_int = satd_int; o.satd_best = best_s; o.cost_best = best_c; o.mvx = (short)best_x; o.mvy = (short)best_y; }
      else { o.satd_int = o.satd_best = o.cost_best = 0xFFFFFFFFu; o.mvx = 0; o.mvy = 0; }
      out[oc * FHEVC_NODES + nidx] = o;
    }
  }
}

template <typename T, bool PACKED>
hipError_t launch_refine(const FhevcFrames& fr, int max_range, const FhevcMvBitCost& cost, const FhevcMotionNode* d_nodes, FhevcMotionQpelNode* d_out, int num_cus,
                         long long total, hipStream_t stream)
{
  if (max_range <= FHEVC_MOTION_MAX_RANGE) {
    const int grid = (int)(total < 4LL * num_cus ? total : 4LL * num_cus);
    hipLaunchKernelGGL((fhevc_motion_refine_kernel<T, PACKED, FHEVC_MOTION_MAX_RANGE>), dim3(grid), dim3(256), 0, stream, fr, max_range, cost, d_nodes, d_out, SearchNoCentres{});
  } else {
    constexpr int MRB = FHEVC_MOTION_WIDE_MAX_RANGE;
    const size_t lds = (size_t)RefineGeom<MRB>::SAMPLES * sizeof(short);  // 80 016 B: one workgroup per CU beside another kernel's, two alone
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&fhevc_motion_refine_kernel<T, PACKED, MRB>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    const int grid = (int)(total < 2LL * num_cus ? total : 2LL * num_cus);
    hipLaunchKernelGGL((fhevc_motion_refine_kernel<T, PACKED, MRB>), dim3(grid), dim3(256), lds, stream, fr, max_range, cost, d_nodes, d_out, SearchNoCentres{});
  }
  return hipGetLastError();
}

template <typename T, bool PACKED>
hipError_t launch_refine_centred(const FhevcFrames& fr, int max_range, const FhevcMvBitCost& cost, const FhevcMotionNode* d_centres, const FhevcMotionNode* d_nodes,
                                 FhevcMotionQpelNode* d_out, int num_cus, long long total, hipStream_t stream)
{
  const int grid = (int)(total < 4LL * num_cus ? total : 4LL * num_cus);
  hipLaunchKernelGGL((fhevc_motion_refine_kernel<T, PACKED, FHEVC_MOTION_MAX_RANGE, true>), dim3(grid), dim3(256), 0, stream, fr, max_range, cost, d_nodes, d_out, d_centres);
  return hipGetLastError();
}

}  // namespace

// the MR = 8 layout around one centre per CTU (behind fhevc_motion_refine_pu_centred): max_range 1 .. FHEVC_MOTION_MAX_RANGE
hipError_t fhevc_launch_motion_refine_centred(const FhevcFrames& fr, int max_range, const FhevcMvBitCost& cost, const FhevcMotionNode* d_centres, const FhevcMotionNode* d_nodes,
                                              FhevcMotionQpelNode* d_out, int num_cus, hipStream_t stream)
{
  const long long total = (long long)(fr.row_end - fr.row_begin) * fr.ctus_x * (fr.num_frames - 1);
  if (total <= 0) return hipSuccess;
  if (max_range < 1 || max_range > FHEVC_MOTION_MAX_RANGE || !d_centres) return hipErrorInvalidValue;
  if (fr.sample_bytes == 2 && fr.bit_depth <= 10) return launch_refine_centred<int16_t, true>(fr, max_range, cost, d_centres, d_nodes, d_out, num_cus, total, stream);
  if (fr.sample_bytes == 2) return launch_refine_centred<int16_t, false>(fr, max_range, cost, d_centres, d_nodes, d_out, num_cus, total, stream);
  return launch_refine_centred<uint8_t, true>(fr, max_range, cost, d_centres, d_nodes, d_out, num_cus, total, stream);
}

hipError_t fhevc_launch_motion_refine(const FhevcFrames& fr, int max_range, const FhevcMvBitCost& cost, const FhevcMotionNode* d_nodes, FhevcMotionQpelNode* d_out,
                                      int num_cus, hipStream_t stream)
{
  const long long total = (long long)(fr.row_end - fr.row_begin) * fr.ctus_x * (fr.num_frames - 1);
  if (total <= 0) return hipSuccess;
  if (max_range < 1 || max_range > FHEVC_MOTION_WIDE_MAX_RANGE) return hipErrorInvalidValue;
  if (fr.sample_bytes == 2 && fr.bit_depth <= 10) return launch_refine<int16_t, true>(fr, max_range, cost, d_nodes, d_out, num_cus, total, stream);
  if (fr.sample_bytes == 2) return launch_refine<int16_t, false>(fr, max_range, cost, d_nodes, d_out, num_cus, total, stream);
  return launch_refine<uint8_t, true>(fr, max_range, cost, d_nodes, d_out, num_cus, total, stream);
}