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
// PASSES, each a covering of the CTU by one (CU size, shape) pair:
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

#include <atomic>

namespace {

constexpr int PASSES_PU = 14, PASSES = 26;
constexpr int WG_PER_CU = 2;   // 210 (packed) / 238 (32-bit) VGPRs at MR = 8, 218 / 246 at MR = 64: two waves per SIMD, and the persistent grid is sized to that residency

// the sum over the tiles of this lane's PU of shape s (0 2NxN, 1 Nx2N, 2 2NxnU, 3 2NxnD, 4 nLx2N, 5 nRx2N) of a CU of 2^n x 2^n tiles; n and s are
// wave-uniform.  horiz: the CU is cut by a horizontal line; along: the tile's row (column) inside the CU; part: the part that holds the tile
__device__ __forceinline__ unsigned pu_sum(unsigned t8, int lane, int n, int s, bool horiz, int along, int part)
{
  const int ob = horiz ? 1 : 8, ab = horiz ? 8 : 1;   // lane bits across the cut's direction / along it
  unsigned strip = t8;
  for (int k = 0; k < n; ++k) strip += __shfl_xor(strip, ob << k);       // the CU's whole width (height) at this tile row (column)
  const int own = s < 2 ? n - 1 : n - 2;                                 // ... summed over the lane's own half, or its own quarter
  for (int k = 0; k < own; ++k) strip += __shfl_xor(strip, ab << k);
  if (s < 2) return strip;
  unsigned cu = strip;
  for (int k = own; k < n; ++k) cu += __shfl_xor(cu, ab << k);
  const int qpart = s & 1;                                               // 2NxnU, nLx2N: the quarter comes first; 2NxnD, nRx2N: last
  const unsigned quarter = __shfl(strip, lane + ((qpart ? (1 << n) - 1 : 0) - along) * ab);
  return part == qpart ? quarter : cu - quarter;
}

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
  const int band_rows = F.row_end - F.row_begin;
  const int per_frame = band_rows * F.ctus_x;
  const int total = per_frame * (F.num_frames - 1);  // frame f >= 1 is refined in frame f - 1
  const int bd = F.bit_depth;
  const int shift = bd - 8;
  const RefineArith arith(bd);
  const T* plane = reinterpret_cast<const T*>(F.luma);
  const int pass_begin = pus ? 0 : PASSES_PU, pass_end = pus_small ? PASSES : PASSES_PU;
  if (tid < FHEVC_MV_BIT_COSTS) s_cost[tid] = cost.c[tid];
  if (tid < 16) s_taps[tid] = kLumaTaps[tid];

  for (int work = blockIdx.x; work < total; work += gridDim.x) {
    const int f = 1 + work / per_frame;
    const int rem = work % per_frame;
    const int cy = F.row_begin + rem / F.ctus_x, cx = rem % F.ctus_x;
    const long long cur_base = (long long)f * F.frame_stride, ref_base = (long long)(f - 1) * F.frame_stride;
    const long long oc = (long long)((f - 1) * band_rows + (cy - F.row_begin)) * F.ctus_x + cx;
    SearchCentre P;
    if constexpr (CENTRED) {
      P = SearchCentre(centres, oc);
      if (!P.in_range()) {  // uniform: every entry of this CTU gets the marker, nothing is read for it
        FhevcMotionQpelNode o;
        o.satd_int = o.satd_best = o.cost_best = 0xFFFFFFFFu; o.mvx = 0; o.mvy = 0;
        if (pus && tid < FHEVC_PUS) out_pus[oc * FHEVC_PUS + tid] = o;
        if (pus_small)
          for (int e = tid; e < FHEVC_PUS_SMALL; e += 256) out_small[oc * FHEVC_PUS_SMALL + e] = o;
        continue;
      }
    }
    __syncthreads();  // the previous CTU's readers are done
    if constexpr (CENTRED) refine_stage_window<T, MR>(s_ref, plane, ref_base, F, cx, cy, tid, P.x, P.y);
    else if (BIG && !stage_full) refine_stage_window_reach<T, MR>(s_ref, plane, ref_base, F, cx, cy, tid, max_range);
    else refine_stage_window<T, MR>(s_ref, plane, ref_base, F, cx, cy, tid);
    // ---- this lane's original 8x8 tile (all four waves hold the same 64 tiles) ----
    const int px = cx * 64 + tx * 8, py = cy * 64 + ty * 8;
    const bool inside = (px + 8 <= F.width) && (py + 8 <= F.height);
    unsigned O[32];
    load_tile8x8(plane, cur_base, F, px, py, inside, O);
    __syncthreads();

#pragma unroll 1
    for (int pass = pass_begin + wave; pass < pass_end; pass += 4) {
      // ---- the pass's covering and this lane's PU in it (pass is wave-uniform) ----
      const bool small = pass >= PASSES_PU;
      int n, s, want = 0;   // CU of 2^n x 2^n tiles (small: n = 1: 16x16, 0: 8x8), shape, the part a small pass sums
      if (!small) { n = pass < 6 ? 3 : pass < 12 ? 2 : 1; s = pass - (pass < 6 ? 0 : pass < 12 ? 6 : 12); }
      else { const int c = (pass - PASSES_PU) >> 1; want = (pass - PASSES_PU) & 1; n = c < 4 ? 1 : 0; s = c < 4 ? 2 + c : c - 4; }
      const int tn = 1 << n, nsize = 8 << n;
      const int lx = tx & (tn - 1), ly = ty & (tn - 1);
      const bool horiz = s == 0 || s == 2 || s == 3;                 // cut by a horizontal line: part 0 on top
      const int ni = (ty >> n) * (8 >> n) + (tx >> n);               // the CU among those of its size, raster
      int entry, part;
      unsigned qmask = 0;                                            // small: the quadrants q00 q01 / q10 q11 of the tile that lie in part `want`
      bool rep;                                                      // this lane writes the PU
      if (!small) {
        const int sp = s < 2 ? tn / 2 : (s & 1) ? 3 * tn / 4 : tn / 4;   // where the CU is cut, in tiles
        const int along = horiz ? ly : lx, other = horiz ? lx : ly;
        part = along >= sp ? 1 : 0;
        rep = other == 0 && along == part * sp;
        entry = (n == 3 ? 0 : n == 2 ? (1 + ni) * 12 : 60 + ni * 4) + s * 2 + part;
      } else {
        part = want;
        const int cut = n == 0 ? 1 : (s & 1) ? 3 : 1;                // in 4-sample units from the CU's top (left) edge
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int pos = horiz ? ly * 2 + (k >> 1) : lx * 2 + (k & 1);
          if ((pos >= cut ? 1 : 0) == want) qmask |= 1u << k;
        }
        rep = lx == 0 && ly == 0;
        entry = n == 1 ? ni * 8 + (s - 2) * 2 + part : 128 + ni * 4 + s * 2 + part;
      }
      // ---- its integer vector: only mvx / mvy of the input are read, validity comes from the geometry and from max_range ----
      const bool node_in = cx * 64 + (tx >> n) * nsize + nsize <= F.width && cy * 64 + (ty >> n) * nsize + nsize <= F.height;
      const long long e = small ? oc * FHEVC_PUS_SMALL + entry : oc * FHEVC_PUS + entry;
      int mx = 0, my = 0;
      bool valid = false;
      if (node_in) {
        const unsigned w = reinterpret_cast<const unsigned*>(small ? pus_small : pus)[e * 4 + 3];
        mx = (int)(short)(w & 0xFFFFu); my = (int)(short)(w >> 16);
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
        const int col = tx * 8 + MR + 4 + (qx >> 2) - 3, row0 = ty * 8 + MR + 4 + (qy >> 2) - 3;  // first tap of sample (0, 0)
        unsigned sum;
        {
          unsigned D[32];
          int v[64];
          refine_tile_diff<PACKED, RP>(s_ref, s_taps, arith, col, row0, qx & 3, qy & 3, O, D, v);
          if (small) {  // xCalcHADs4x4 per quadrant, (sum + 1) >> 1 each (TComRdCost.cpp:1771-1803); only the quadrants of this pass's part
            sum = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              unsigned q;
              if constexpr (PACKED) q = had4x4_packed(D, (k >> 1) * 4, (k & 1) * 2);
              else q = had4x4_wide(v, (k >> 1) * 4, (k & 1) * 4);
              sum += ((qmask >> k) & 1u) ? q : 0u;
            }
            sum = inside ? sum : 0u;
            if (n == 1) { sum += __shfl_xor(sum, 1); sum += __shfl_xor(sum, 8); }  // the four tiles of the 16x16 CU
          } else {
            unsigned t8;
            if constexpr (PACKED) t8 = had8x8_packed(D);
            else t8 = had8x8_wide(v);
            t8 = inside ? ((t8 + 2) >> 2) : 0u;  // xCalcHADs8x8: (sum + 2) >> 2 (TComRdCost.cpp:1747)
            sum = pu_sum(t8, lane, n, s, horiz, horiz ? ly : lx, part);
          }
        }
        const unsigned sd = sum >> shift;  // DISTORTION_PRECISION_ADJUSTMENT on the block's sum (TComRdCost.cpp:1823)
        const unsigned c = sd + s_cost[eg_bits(qx) + eg_bits(qy)];
        if (i == 0) satd_int = sd;
        if (c < best_c) { best_c = c; best_s = sd; best_x = qx; best_y = qy; }
      }
      if (rep) {
        FhevcMotionQpelNode o;
        if constexpr (CENTRED) { best_x += 4 * P.x; best_y += 4 * P.y; }
        if (valid) { o.satd_int = satd_int; o.satd_best = best_s; o.cost_best = best_c; o.mvx = (short)best_x; o.mvy = (short)best_y; }
        else { o.satd_int = o.satd_best = o.cost_best = 0xFFFFFFFFu; o.mvx = 0; o.mvy = 0; }
        (small ? out_small : out_pus)[e] = o;
      }
    }
  }
}

// the MR = 64 instance of one (T, PACKED) form: its dynamic LDS, and how many of its workgroups the device keeps on one CU (asked once per instance)
template <typename T, bool PACKED> struct RefinePuBig {
  static constexpr int MRB = FHEVC_MOTION_WIDE_MAX_RANGE;
  static constexpr size_t LDS = (size_t)RefineGeom<MRB>::SAMPLES * sizeof(short);  // 80 016 B
  static const void* kernel() { return reinterpret_cast<const void*>(&fhevc_motion_refine_pu_kernel<T, PACKED, MRB>); }
  static hipError_t resident(int* per_cu)
  {
    const hipError_t e = hipFuncSetAttribute(kernel(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS);
    if (e != hipSuccess) return e;
    static std::atomic<int> asked{0};   // every device of a context is a gfx950: one answer per instance
    int n = asked.load(std::memory_order_relaxed);
    if (n == 0) {
      const hipError_t q = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fhevc_motion_refine_pu_kernel<T, PACKED, MRB>, 256, LDS);
      if (q != hipSuccess) return q;
      asked.store(n, std::memory_order_relaxed);
    }
    *per_cu = n;
    return hipSuccess;
  }
};

template <typename T, bool PACKED>
hipError_t launch_refine_pu(const FhevcFrames& fr, int max_range, const FhevcMvBitCost& cost, const FhevcMotionNode* d_pus, FhevcMotionQpelNode* d_out_pus,
                            const FhevcMotionNode* d_pus_small, FhevcMotionQpelNode* d_out_small, int num_cus, bool stage_full, long long total, hipStream_t stream)
{
  if (max_range <= FHEVC_MOTION_MAX_RANGE) {
    const long long resident = (long long)WG_PER_CU * num_cus;
    const int grid = (int)(total < resident ? total : resident);
    hipLaunchKernelGGL((fhevc_motion_refine_pu_kernel<T, PACKED, FHEVC_MOTION_MAX_RANGE>), dim3(grid), dim3(256), 0, stream, fr, max_range, cost, d_pus, d_out_pus,
                       d_pus_small, d_out_small, false, SearchNoCentres{});
  } else {
    using Big = RefinePuBig<T, PACKED>;
    int per_cu = 0;
    const hipError_t e = Big::resident(&per_cu);
    if (e != hipSuccess) return e;
    if (per_cu < 1) return hipErrorLaunchOutOfResources;
    const long long resident = (long long)(per_cu < WG_PER_CU ? per_cu : WG_PER_CU) * num_cus;   // what is actually resident, at most what the VGPRs allow
    const int grid = (int)(total < resident ? total : resident);
    hipLaunchKernelGGL((fhevc_motion_refine_pu_kernel<T, PACKED, Big::MRB>), dim3(grid), dim3(256), Big::LDS, stream, fr, max_range, cost, d_pus, d_out_pus,
                       d_pus_small, d_out_small, stage_full, SearchNoCentres{});
  }
  return hipGetLastError();
}

}  // namespace

hipError_t fhevc_launch_motion_refine_pu(const FhevcFrames& fr, int max_range, const FhevcMvBitCost& cost, const FhevcMotionNode* d_pus, FhevcMotionQpelNode* d_out_pus,
                                         const FhevcMotionNode* d_pus_small, FhevcMotionQpelNode* d_out_small, int num_cus, bool stage_full, hipStream_t stream)
{
  const long long total = (long long)(fr.row_end - fr.row_begin) * fr.ctus_x * (fr.num_frames - 1);
  if (total <= 0) return hipSuccess;
  if (max_range < 1 || max_range > FHEVC_MOTION_WIDE_MAX_RANGE || (!d_pus && !d_pus_small) || !d_pus != !d_out_pus || !d_pus_small != !d_out_small) return hipErrorInvalidValue;
#define FHEVC_REFINE_PU(T, P) return launch_refine_pu<T, P>(fr, max_range, cost, d_pus, d_out_pus, d_pus_small, d_out_small, num_cus, stage_full, total, stream)
  if (fr.sample_bytes == 2 && fr.bit_depth <= 10) FHEVC_REFINE_PU(int16_t, true);
  else if (fr.sample_bytes == 2) FHEVC_REFINE_PU(int16_t, false);
  else FHEVC_REFINE_PU(uint8_t, true);
#undef FHEVC_REFINE_PU
}

// the MR = 8 layout around one centre per CTU (behind fhevc_motion_refine_pu_centred): max_range 1 .. FHEVC_MOTION_MAX_RANGE, the same residency
hipError_t fhevc_launch_motion_refine_pu_centred(const FhevcFrames& fr, int max_range, const FhevcMvBitCost& cost, const FhevcMotionNode* d_centres, const FhevcMotionNode* d_pus,
                                                 FhevcMotionQpelNode* d_out_pus, const FhevcMotionNode* d_pus_small, FhevcMotionQpelNode* d_out_small, int num_cus, hipStream_t stream)
{
  const long long total = (long long)(fr.row_end - fr.row_begin) * fr.ctus_x * (fr.num_frames - 1);
  if (total <= 0) return hipSuccess;
  if (max_range < 1 || max_range > FHEVC_MOTION_MAX_RANGE || !d_centres || (!d_pus && !d_pus_small) || !d_pus != !d_out_pus || !d_pus_small != !d_out_small) return hipErrorInvalidValue;
  const long long resident = (long long)WG_PER_CU * num_cus;
  const int grid = (int)(total < resident ? total : resident);
#define FHEVC_REFINE_PU_CENTRED(T, P)                                                                                                                              \
  hipLaunchKernelGGL((fhevc_motion_refine_pu_kernel<T, P, FHEVC_MOTION_MAX_RANGE, true>), dim3(grid), dim3(256), 0, stream, fr, max_range, cost, d_pus, d_out_pus, \
                     d_pus_small, d_out_small, false, d_centres)
  if (fr.sample_bytes == 2 && fr.bit_depth <= 10) FHEVC_REFINE_PU_CENTRED(int16_t, true);
  else if (fr.sample_bytes == 2) FHEVC_REFINE_PU_CENTRED(int16_t, false);
  else FHEVC_REFINE_PU_CENTRED(uint8_t, true);
#undef FHEVC_REFINE_PU_CENTRED
  return hipGetLastError();
}

// workgroups of the MR = 64 instance that the device keeps on one CU, for the form that planes of sample_bytes at bit_depth take (measurement tools)
hipError_t fhevc_motion_refine_pu_big_residency(int sample_bytes, int bit_depth, int* per_cu)
{
  if (sample_bytes == 2 && bit_depth <= 10) return RefinePuBig<int16_t, true>::resident(per_cu);
  if (sample_bytes == 2) return RefinePuBig<int16_t, false>::resident(per_cu);
  return RefinePuBig<uint8_t, true>::resident(per_cu);
}
