// k_motion_refine_pu.hip -- source-only quarter-sample refinement of the motion search per PREDICTION UNIT (config 4: P slices), gfx950 only.
//
// What k_motion_refine.hip does for the 85 square CU nodes, for the 508 PUs of HM's partitioned CUs: the 124 whose sides are multiples of 8
// (k_motion_pu.hip, layout fhevc_motion_pu_index) and the 384 with a 4-sample side (k_motion_pu_small.hip, layout fhevc_motion_pu_small_index).
// HM runs xPatternSearchFracDIF behind the integer search of EVERY PU (TEncSearch::xMotionEstimation), so xCheckRDCostInter compares partition
// shapes on each PU's Hadamard cost at its quarter-sample vector.  Per PU: the half-sample stage of s_acMvRefineH, the quarter-sample stage of
// s_acMvRefineQ around its winner, strict "<", cost = TComRdCost::xGetHADs of the whole w x h PU on the 8-tap interpolation of the previous
// original picture + getCostOfVectorWithPredictor in quarter units (zero predictor).  xGetHADs has two branches (TComRdCost.cpp:1771-1823):
//   both sides multiples of 8 (all 124):   the sum over the PU's 8x8 tiles of (sum |H8 d H8| + 2) >> 2
//   otherwise (all 384, 16x12 included):   the sum over ALL (w/4)(h/4) 4x4 tiles of (sum |H4 d H4| + 1) >> 1
// and the PU's sum is shifted ONCE by bit_depth - 8.  A 16x12 part is twelve 4x4 Hadamards, not "the node minus the quarter".
//
// Mapping as k_motion_refine.hip: workgroup (4 waves) = one CTU at a time, grid-stride; the reference window staged once per CTU in LDS; lane =
// one 8x8 tile (lane = ty * 8 + tx) with its 64 original samples as packed pairs; the fractions are per-lane data, so the 18-candidate loop is
// wave-uniform; tile prediction, window and tables are k_refine_tile.h's.  Where that kernel's wave takes one LEVEL, a wave here takes a list of
// PASSES, each a covering of the CTU by one (CU size, shape) pair (RefinePuPass and refine_pu_had there: k_motion_merge_pu.hip walks the same passes):
//   passes 0..13   the 124: shapes 0..5 of the 64x64 CU, shapes 0..5 of the 32x32 CUs, shapes 0..1 of the 16x16 CUs.  Every tile lies in exactly one
//                  PU; a lane predicts its tile at ITS PU's candidate and the PU's sum is a reduction over lanes: a butterfly across the CU in the
//                  direction of the cut, a butterfly over the lane's own half (2NxN, Nx2N) or quarter, and for AMP one lane read of the CU's first
//                  or last quarter strip -- the three-quarter part is the CU's sum of 8x8 tiles minus that strip (the lanes k_motion_pu.hip pairs)
//   passes 14..25  the 384: for each of the shapes 2..5 of the 16x16 CUs and 0..1 of the 8x8 CUs one pass PER PART.  A tile can straddle two PUs with
//                  different vectors: in the pass of part p every lane predicts its tile at part p's candidate, takes the four quadrant Hadamards
//                  (had4x4_* of k_had8x8.h) and sums only the quadrants that belong to part p; the 16x16 CU's four tiles meet over lane bits 0 and 3
// Wave w takes passes w, w + 4, .. of the families asked for: 7 + 7 + 6 + 6 of the 26, so the waves finish within one pass of each other.
// No scratch, no HBM state between calls: the vector costs travel by value.
//
// Two layouts, as k_motion_refine.hip: MR = 8 (max_range 1..8; the static window of 15 504 B + tables, the square refinement's) and MR = 64 (max_range
// 9..64, behind fhevc_motion_refine_pu_wide: the window of (64 + 2 * 64 + 8)^2 samples = 80 016 B as dynamic LDS, + 224 B of tables).  Passes, pu_sum, the
// quadrant path, the validity rule and the cost table are one code for both; only RP, the window's origin (MR + 4) and where the window lives differ.
// Residency at MR = 64: the VGPRs allow two workgroups per CU and so does the LDS, just: 2 * (80 016 + 224) = 160 480 of 163 840 B.  The launcher asks
// hipOccupancyMaxActiveBlocksPerMultiprocessor and sizes the persistent grid by its answer.  The MR = 64 layout stages only the part of the window that
// max_range can reach (refine_stage_window_reach: rows and columns within max_range + 4 of the CTU, columns widened to the 4-sample chunks): at
// max_range 64 that is the whole window, at 9 a quarter of it.  The addressing is that of the whole window and the results are bit-identical;
// FHEVC_REFINE_PU_STAGE=full in the environment of fhevc_create stages the whole window whatever max_range is (tests, A/B timing).
#include "fhevc_internal.h"
#include "k_had8x8.h"
#include "k_refine_tile.h"

namespace {

// more than 128 VGPRs in every instance: two waves per SIMD, and the persistent grid is sized to that residency; at MR = 64 to what is actually resident,
// at most what the VGPRs allow
constexpr int WG_PER_CU = 2;
constexpr RefineResidency kSmall = {WG_PER_CU, false}, kBig = {WG_PER_CU, true};

// T = int16_t (HM Pel planes) or uint8_t; PACKED = bit depth <= 10 (the packed Hadamards); MR = 8 or 64: the largest integer vector the window is laid
// out for; stage_full (MR = 64 only): stage the whole window, not only what max_range reaches
// CENTRED (fhevc_motion_refine_pu_centred; MR = 8): as fhevc_motion_refine_kernel's -- the window staged around the CTU's centre P, vectors relative to P inside,
// 4 P added to the winner
template <typename T, bool PACKED, int MR, bool CENTRED = false>
__global__ __launch_bounds__(256) void fhevc_motion_refine_pu_kernel(FhevcFrames F, int max_range, FhevcMvBitCost cost, const FhevcMotionNode* __restrict__ pus,
                                                                     FhevcMotionQpelNode* __restrict__ out_pus, const FhevcMotionNode* __restrict__ pus_small,
                                                                     FhevcMotionQpelNode* __restrict__ out_small, bool stage_full, SearchCentres<CENTRED> centres)
{
  constexpr int RP = RefineGeom<MR>::RP;
  constexpr bool BIG = MR > FHEVC_MOTION_MAX_RANGE;
  extern __shared__ __attribute__((aligned(16))) short s_dyn[];
  __shared__ __attribute__((aligned(16))) short s_small[BIG ? 8 : RefineGeom<MR>::SAMPLES];
  short* const s_ref = BIG ? s_dyn : s_small;
  __shared__ unsigned s_cost[FHEVC_MV_BIT_COSTS], s_taps[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tx = lane & 7, ty = lane >> 3;
  const int total = SearchWork::total(F);  // frame f >= 1 is refined in frame f - 1
  const int shift = F.bit_depth - 8;
  const RefineArith arith(F.bit_depth);
  const T* plane = reinterpret_cast<const T*>(F.luma);
  const int pass_begin = pus ? 0 : PASSES_PU, pass_end = pus_small ? PASSES : PASSES_PU;
  if (tid < FHEVC_MV_BIT_COSTS) s_cost[tid] = cost.c[tid];
  if (tid < 16) s_taps[tid] = kLumaTaps[tid];

  for (int work = blockIdx.x; work < total; work += gridDim.x) {
    const SearchWork W(F, work);
    const int cy = W.cy, cx = W.cx;
    const long long oc = W.oc(F);
    SearchCentre P;
    if constexpr (CENTRED) {
      P = SearchCentre(centres, oc);
      if (!P.in_range()) {  // uniform: every entry of this CTU gets the marker, nothing is read for it
        const FhevcMotionQpelNode o = refine_record(false, 0, 0, 0, 0, 0);
        if (pus && tid < FHEVC_PUS) out_pus[oc * FHEVC_PUS + tid] = o;
        if (pus_small)
          for (int e = tid; e < FHEVC_PUS_SMALL; e += 256) out_small[oc * FHEVC_PUS_SMALL + e] = o;
        continue;
      }
    }
    __syncthreads();  // the previous CTU's readers are done
    if constexpr (CENTRED) refine_stage_window<T, MR>(s_ref, plane, W.ref_base, F, cx, cy, tid, P.x, P.y);
    else if (BIG && !stage_full) refine_stage_window_reach<T, MR>(s_ref, plane, W.ref_base, F, cx, cy, tid, max_range);
    else refine_stage_window<T, MR>(s_ref, plane, W.ref_base, F, cx, cy, tid);
    // ---- this lane's original 8x8 tile (all four waves hold the same 64 tiles) ----
    const int px = cx * 64 + tx * 8, py = cy * 64 + ty * 8;
    const bool inside = (px + 8 <= F.width) && (py + 8 <= F.height);
    unsigned O[32];
    load_tile8x8(plane, W.cur_base, F, px, py, inside, O);
    __syncthreads();

#pragma unroll 1
    for (int pass = pass_begin + wave; pass < pass_end; pass += 4) {
      const RefinePuPass U(pass, tx, ty);  // the pass's covering and this lane's PU in it (pass is wave-uniform)
      // ---- its integer vector: only mvx / mvy of the input are read, validity comes from the geometry and from max_range ----
      const long long e = U.record(oc);
      int mx = 0, my = 0;
      bool valid = false;
      if (search_node_inside(F, cx, cy, U.nbx, U.nby, U.nsize())) {
        const unsigned w = reinterpret_cast<const unsigned*>(U.small ? pus_small : pus)[e * 4 + 3];
        mx = vec_x(w); my = vec_y(w);
        if constexpr (CENTRED) { mx -= P.x; my -= P.y; }
        valid = abs(mx) <= max_range && abs(my) <= max_range;
        if (!valid) { mx = 0; my = 0; }  // the arithmetic below stays inside the window; its result is dropped
      }

      int base_x = 4 * mx, base_y = 4 * my;      // quarter units
      int best_x = base_x, best_y = base_y;
      unsigned best_c = 0xFFFFFFFFu, best_s = 0, satd_int = 0;
#pragma unroll 1
      for (int i = 0; i < 18; ++i) {
        if (i == 9) { base_x = best_x; base_y = best_y; best_c = 0xFFFFFFFFu; }  // the quarter stage starts from the half stage's winner
        const int step = i < 9 ? 2 : 1;
        const int qx = base_x + step * (int)kRefineX[i], qy = base_y + step * (int)kRefineY[i];
        const unsigned sum = refine_pu_had<PACKED, RP>(s_ref, s_taps, arith, lane, tx, ty, U, qx, qy, O, inside);
        const unsigned sd = sum >> shift;  // DISTORTION_PRECISION_ADJUSTMENT on the block's sum (TComRdCost.cpp:1823)
        const unsigned c = sd + s_cost[eg_bits(qx) + eg_bits(qy)];
        if (i == 0) satd_int = sd;
        if (c < best_c) { best_c = c; best_s = sd; best_x = qx; best_y = qy; }
      }
      if (U.rep) {
        if constexpr (CENTRED) { best_x += 4 * P.x; best_y += 4 * P.y; }
        (U.small ? out_small : out_pus)[e] = refine_record(valid, satd_int, best_s, best_c, best_x, best_y);
      }
    }
  }
}

}  // namespace

hipError_t fhevc_launch_motion_refine_pu(const FhevcFrames& fr, int max_range, const FhevcMvBitCost& cost, const FhevcMotionNode* d_pus, FhevcMotionQpelNode* d_out_pus,
                                         const FhevcMotionNode* d_pus_small, FhevcMotionQpelNode* d_out_small, int num_cus, bool stage_full, hipStream_t stream)
{
  const bool args_ok = (d_pus || d_pus_small) && !d_pus == !d_out_pus && !d_pus_small == !d_out_small;
  return refine_launch<FHEVC_MOTION_WIDE_MAX_RANGE>(fr, args_ok, max_range, num_cus, kSmall, kBig, stream, [&](auto t, auto packed, auto mr, const RefineLaunch& L) {
    return refine_launch_kernel<&fhevc_motion_refine_pu_kernel<decltype(t), decltype(packed)::value, decltype(mr)::value>>(L, fr, max_range, cost, d_pus, d_out_pus, d_pus_small,
                                                                                                                           d_out_small, stage_full, SearchNoCentres{});
  });
}

// the MR = 8 layout around one centre per CTU (behind fhevc_motion_refine_pu_centred): max_range 1 .. FHEVC_MOTION_MAX_RANGE, the same residency
hipError_t fhevc_launch_motion_refine_pu_centred(const FhevcFrames& fr, int max_range, const FhevcMvBitCost& cost, const FhevcMotionNode* d_centres, const FhevcMotionNode* d_pus,
                                                 FhevcMotionQpelNode* d_out_pus, const FhevcMotionNode* d_pus_small, FhevcMotionQpelNode* d_out_small, int num_cus, hipStream_t stream)
{
  const bool args_ok = d_centres && (d_pus || d_pus_small) && !d_pus == !d_out_pus && !d_pus_small == !d_out_small;
  return refine_launch<FHEVC_MOTION_MAX_RANGE>(fr, args_ok, max_range, num_cus, kSmall, {}, stream, [&](auto t, auto packed, auto mr, const RefineLaunch& L) {
    return refine_launch_kernel<&fhevc_motion_refine_pu_kernel<decltype(t), decltype(packed)::value, decltype(mr)::value, true>>(L, fr, max_range, cost, d_pus, d_out_pus,
                                                                                                                                 d_pus_small, d_out_small, false, d_centres);
  });
}

// workgroups of the MR = 64 instance that the device keeps on one CU, for the form that planes of sample_bytes at bit_depth take (measurement tools)
hipError_t fhevc_motion_refine_pu_big_residency(int sample_bytes, int bit_depth, int* per_cu)
{
  constexpr int MRB = FHEVC_MOTION_WIDE_MAX_RANGE;
  constexpr size_t LDS = (size_t)RefineGeom<MRB>::SAMPLES * sizeof(short);  // 80 016 B
  if (sample_bytes == 2 && bit_depth <= 10) return refine_resident<&fhevc_motion_refine_pu_kernel<int16_t, true, MRB>>(LDS, per_cu);
  if (sample_bytes == 2) return refine_resident<&fhevc_motion_refine_pu_kernel<int16_t, false, MRB>>(LDS, per_cu);
  return refine_resident<&fhevc_motion_refine_pu_kernel<uint8_t, true, MRB>>(LDS, per_cu);
}
