// k_motion_merge_pu.hip -- source-only merge-candidate costs per PREDICTION UNIT (config 4: P slices), gfx950 only.
//
// TEncSearch::xMergeEstimation (TEncSearch.cpp:2831-2884) where HM runs it: for every PU of a CU whose partition size is not 2Nx2N (:3336, :3371), on the
// candidate list of TComDataCU::getInterMergeCandidates (TComDataCU.cpp:2142-2320); spec in include/fasthevc.h.  What k_motion_merge.hip prices for the 85
// square nodes, for the 508 PUs of k_motion_refine_pu.hip: the five samples L, A, AR, BL, AL around the PU's OWN rectangle, each mapped to the node of the
// CU's level that holds it, that node's refined square vector as the candidate; HM's order and pruning pairs, AL only below four entries, one zero vector
// below five; each entry priced as xGetHADs of the whole w x h PU at that quarter-sample vector + getCost(bits of the merge index): 1, 2, 3, 4, 4.
//
// A composition of two kernels, no new arithmetic:
//   * of k_motion_refine_pu.hip the mapping: workgroup (4 waves) = one CTU at a time over a persistent grid; the window of k_refine_tile.h staged once per
//     CTU (refine_stage_window_reach in both layouts; MR = 8: static LDS, MR = 64: dynamic); lane = one 8x8 tile; the 26 passes dealt to the four waves;
//     pu_sum for the 14 tile-aligned passes, the quadrant mask and one pass per part for the 12 others;
//   * of k_motion_merge.hip the list: five "taken" flags in registers, the unrolled pick with no dynamic indexing, the wave-uniform loop to the wave's longest
//     list by four ballots, a lane with a shorter list evaluating the zero vector and dropping the result.  The candidate loop of a pass is at most 5 long.
// Where the list comes from is new: the lane's PU changes per pass, and so do its five neighbour nodes.  The nodes that can be a neighbour of any PU of the
// CTU are parked in LDS once per CTU, before the passes: the CTU's own 85 nodes, the right column of the left CTU and the bottom row of the upper CTU (15
// each), the corner nodes of the two upper diagonal CTUs (4 each) -- 123 dwords.  A parked dword is the node's vector if the node is on the grid, INSIDE, in
// a CTU row of the band, no marker and within the reach 4 max_range + 3; otherwise mvx = -32768, which no reach admits.  (CTUs to the right and below
// follow in coding order: none of their nodes is ever available.)  What a pass adds per lane is the coding-order test inside the own CTU -- the z-index of
// the neighbour strictly below that of the PU's own CU, which also excludes the own CU, HM's two second-PU rules -- and five LDS reads whose addresses depend
// on the geometry alone.  LDS on top of the window: 492 B parked + 96 B tables (MR = 64: two workgroups per CU leave 1 680 B each).
// No scratch, no HBM state between calls: the bit costs travel by value.
#include "fhevc_internal.h"
#include "k_had8x8.h"
#include "k_refine_tile.h"

#include <atomic>

namespace {

constexpr int PASSES_PU = 14, PASSES = 26;
constexpr unsigned kMergeMark = 0xFFFFFFFFu;
constexpr unsigned kNoVector = 0x00008000u;   // mvx = -32768, mvy = 0: beyond any reach
constexpr int kParked = 123;                  // 85 own + 15 left + 15 upper + 4 upper-left + 4 upper-right
constexpr int kLeft = 85, kUpper = 100, kUpLeft = 115, kUpRight = 119;

// z-scan index of (x, y) in a level's grid of up to 8 x 8 nodes: the bit interleave, x in the even bits
__device__ __forceinline__ unsigned merge_pu_z(unsigned x, unsigned y)
{
  const unsigned sx = (x & 1u) | ((x & 2u) << 1) | ((x & 4u) << 2), sy = (y & 1u) | ((y & 2u) << 1) | ((y & 4u) << 2);
  return sx | (sy << 1);
}

// k_motion_refine_pu.hip's: the sum over the tiles of this lane's PU of shape s of a CU of 2^n x 2^n tiles; n and s are wave-uniform
__device__ __forceinline__ unsigned merge_pu_sum(unsigned t8, int lane, int n, int s, bool horiz, int along, int part)
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

// where the same-level node at (rx, ry) relative to the CTU's grid of 2^lvl x 2^lvl nodes is parked; -1: a CTU that follows in coding order
__device__ __forceinline__ int parked_slot(int lvl, int rx, int ry)
{
  const int ncnt = 1 << lvl, first = ((1 << (2 * lvl)) - 1) / 3;
  if (ry >= ncnt || (rx >= ncnt && ry >= 0)) return -1;
  if (ry < 0) return rx < 0 ? kUpLeft + lvl : (rx >= ncnt ? kUpRight + lvl : kUpper + ncnt - 1 + rx);
  return rx < 0 ? kLeft + ncnt - 1 + ry : first + ry * ncnt + rx;
}

// T = int16_t or uint8_t planes; PACKED = bit depth <= 10; MR = 8 or 64: the largest max_range the window is laid out for
template <typename T, bool PACKED, int MR>
__global__ __launch_bounds__(256) void fhevc_motion_merge_pu_kernel(FhevcFrames F, int max_range, FhevcMvBitCost cost, const unsigned* __restrict__ refined,
                                                                    FhevcMotionMergeNode* __restrict__ out_pus, FhevcMotionMergeNode* __restrict__ out_small)
{
  constexpr int RP = RefineGeom<MR>::RP;
  constexpr bool BIG = MR > FHEVC_MOTION_MAX_RANGE;
  extern __shared__ __attribute__((aligned(16))) short s_dyn[];
  __shared__ __attribute__((aligned(16))) short s_small[BIG ? 8 : RefineGeom<MR>::SAMPLES];
  short* const s_ref = BIG ? s_dyn : s_small;
  __shared__ unsigned s_cost[8], s_taps[16], s_nb[kParked];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tx = lane & 7, ty = lane >> 3;
  const int band_rows = F.row_end - F.row_begin;
  const int per_frame = band_rows * F.ctus_x;
  const int total = per_frame * (F.num_frames - 1);  // frame f >= 1 is predicted from frame f - 1
  const int shift = F.bit_depth - 8;
  const RefineArith arith(F.bit_depth);
  const T* plane = reinterpret_cast<const T*>(F.luma);
  const int pass_begin = out_pus ? 0 : PASSES_PU, pass_end = out_small ? PASSES : PASSES_PU;
  const int reach = 4 * max_range + 3;
  if (tid < 8) s_cost[tid] = cost.c[tid];
  if (tid < 16) s_taps[tid] = kLumaTaps[tid];
  // the node this thread parks (tid < 123): the CTU it lies in relative to the own one, its level and place there
  int p_dcx = 0, p_dcy = 0, p_lvl = 0, p_bx = 0, p_by = 0;
  if (tid < kLeft) {
    p_lvl = tid < 1 ? 0 : (tid < 5 ? 1 : (tid < 21 ? 2 : 3));
    const int i = tid - ((1 << (2 * p_lvl)) - 1) / 3;
    p_bx = i & ((1 << p_lvl) - 1); p_by = i >> p_lvl;
  } else if (tid < kUpLeft) {
    const int i = (tid - kLeft) % 15;          // 0 | 1 2 | 3..6 | 7..14
    p_lvl = i < 1 ? 0 : (i < 3 ? 1 : (i < 7 ? 2 : 3));
    const int along = i - ((1 << p_lvl) - 1), last = (1 << p_lvl) - 1;
    if (tid < kUpper) { p_dcx = -1; p_bx = last; p_by = along; }
    else { p_dcy = -1; p_bx = along; p_by = last; }
  } else if (tid < kParked) {
    p_lvl = (tid - kUpLeft) & 3; p_dcy = -1;
    const int last = (1 << p_lvl) - 1;
    if (tid < kUpRight) { p_dcx = -1; p_bx = last; p_by = last; }
    else { p_dcx = 1; p_bx = 0; p_by = last; }
  }

  for (int work = blockIdx.x; work < total; work += gridDim.x) {
    const int f = 1 + work / per_frame;
    const int rem = work % per_frame;
    const int cy = F.row_begin + rem / F.ctus_x, cx = rem % F.ctus_x;
    const long long cur_base = (long long)f * F.frame_stride, ref_base = (long long)(f - 1) * F.frame_stride;
    const long long oc = (long long)((f - 1) * band_rows + (cy - F.row_begin)) * F.ctus_x + cx;
    // ---- the node to park: its address from geometry and band alone, the load issued before the staging ----
    unsigned pcost = kMergeMark, pvec = 0;
    if (tid < kParked) {
      const int ncx = cx + p_dcx, ncy = cy + p_dcy;
      const int gx = ncx * (1 << p_lvl) + p_bx, gy = ncy * (1 << p_lvl) + p_by;
      const bool ok = ncx >= 0 && ncx < F.ctus_x && ncy >= F.row_begin && gx < (F.width >> (6 - p_lvl)) && gy < (F.height >> (6 - p_lvl));
      if (ok) {
        const long long rec = ((oc + p_dcy * F.ctus_x + p_dcx) * FHEVC_NODES + ((1 << (2 * p_lvl)) - 1) / 3 + p_by * (1 << p_lvl) + p_bx) * 4;
        pcost = refined[rec + 2]; pvec = refined[rec + 3];
      }
    }
    __syncthreads();  // the previous CTU's readers are done
    refine_stage_window_reach<T, MR>(s_ref, plane, ref_base, F, cx, cy, tid, max_range);
    if (tid < kParked) {
      const int vx = (int)(short)(pvec & 0xFFFFu), vy = (int)(short)(pvec >> 16);
      s_nb[tid] = pcost != kMergeMark && abs(vx) <= reach && abs(vy) <= reach ? pvec : kNoVector;
    }
    // ---- this lane's original 8x8 tile (all four waves hold the same 64 tiles) ----
    const int px = cx * 64 + tx * 8, py = cy * 64 + ty * 8;
    const bool inside = (px + 8 <= F.width) && (py + 8 <= F.height);
    unsigned O[32];
    load_tile8x8(plane, cur_base, F, px, py, inside, O);
    __syncthreads();

#pragma unroll 1
    for (int pass = pass_begin + wave; pass < pass_end; pass += 4) {
      // ---- the pass's covering and this lane's PU in it (pass is wave-uniform): k_motion_refine_pu.hip's ----
      const bool small = pass >= PASSES_PU;
      int n, s, want = 0;   // CU of 2^n x 2^n tiles (small: n = 1: 16x16, 0: 8x8), shape, the part a small pass sums
      if (!small) { n = pass < 6 ? 3 : pass < 12 ? 2 : 1; s = pass - (pass < 6 ? 0 : pass < 12 ? 6 : 12); }
      else { const int c = (pass - PASSES_PU) >> 1; want = (pass - PASSES_PU) & 1; n = c < 4 ? 1 : 0; s = c < 4 ? 2 + c : c - 4; }
      const int tn = 1 << n, nsize = 8 << n, lvl = 3 - n;
      const int lx = tx & (tn - 1), ly = ty & (tn - 1);
      const bool horiz = s == 0 || s == 2 || s == 3;                 // cut by a horizontal line: part 0 on top
      const int nbx = tx >> n, nby = ty >> n;                        // the CU on its level's grid inside the CTU
      const int ni = nby * (8 >> n) + nbx;
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
      const bool node_in = cx * 64 + nbx * nsize + nsize <= F.width && cy * 64 + nby * nsize + nsize <= F.height;
      // ---- the PU's rectangle inside the CTU (getPartIndexAndSize), its five samples, their nodes, the list ----
      const int cut_s = s < 2 ? nsize / 2 : (s & 1) ? 3 * nsize / 4 : nsize / 4;
      const int far = part ? cut_s : 0, len = part ? nsize - cut_s : cut_s;      // along the cut's normal: where the part begins, how long it is
      const int x0 = nbx * nsize + (horiz ? 0 : far), y0 = nby * nsize + (horiz ? far : 0);
      const int w = horiz ? nsize : len, h = horiz ? len : nsize;
      const unsigned zme = merge_pu_z((unsigned)nbx, (unsigned)nby);
      unsigned nvec[5];
      bool av[5];
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const int sx = j == 1 ? x0 + w - 1 : (j == 2 ? x0 + w : x0 - 1);                      // L, A, AR, BL, AL
        const int sy = j == 0 ? y0 + h - 1 : (j == 3 ? y0 + h : y0 - 1);
        const int rx = sx >> (6 - lvl), ry = sy >> (6 - lvl);                                 // arithmetic: -1 stays -1
        const int slot = parked_slot(lvl, rx, ry);
        const bool own = rx >= 0 && ry >= 0 && slot >= 0;                                     // inside the own CTU: coding order by z-index
        const bool ok = node_in && slot >= 0 && (!own || merge_pu_z((unsigned)rx, (unsigned)ry) < zme);
        nvec[j] = s_nb[slot < 0 ? 0 : slot];
        av[j] = ok && nvec[j] != kNoVector;
      }
      bool take[5];
      take[0] = av[0];
      take[1] = av[1] && !(av[0] && nvec[1] == nvec[0]);
      take[2] = av[2] && !(av[1] && nvec[2] == nvec[1]);
      take[3] = av[3] && !(av[0] && nvec[3] == nvec[0]);
      const int n4 = (int)take[0] + (int)take[1] + (int)take[2] + (int)take[3];
      take[4] = n4 < 4 && av[4] && !(av[0] && nvec[4] == nvec[0]) && !(av[1] && nvec[4] == nvec[1]);
      const int n5 = n4 + (int)take[4];
      const int num = node_in ? n5 + (n5 < 5 ? 1 : 0) : 0;   // the zero vector closes a list of fewer than five
      int longest = 1;
#pragma unroll
      for (int m = 2; m <= 5; ++m)
        if (__builtin_amdgcn_ballot_w64(num >= m) != 0) longest = m;   // wave-uniform

      unsigned best_c = kMergeMark, best_s = kMergeMark, best_v = 0;
      int best_i = 255, best_src = 255;
#pragma unroll 1
      for (int i = 0; i < longest; ++i) {
        unsigned qv = 0;   // a lane whose list has ended, or holds the zero vector here
        int src = 5, pos = 0;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
          if (take[j] && pos == i) { qv = nvec[j]; src = j; }
          pos += (int)take[j];
        }
        const int qx = (int)(short)(qv & 0xFFFFu), qy = (int)(short)(qv >> 16);
        const int col = tx * 8 + MR + 4 + (qx >> 2) - 3, row0 = ty * 8 + MR + 4 + (qy >> 2) - 3;  // first tap of sample (0, 0)
        unsigned sum;
        {
          unsigned D[32];
          int v[64];
          refine_tile_diff<PACKED, RP>(s_ref, s_taps, arith, col, row0, qx & 3, qy & 3, O, D, v);
          if (small) {  // xCalcHADs4x4 per quadrant, (sum + 1) >> 1 each; only the quadrants of this pass's part
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
            t8 = inside ? ((t8 + 2) >> 2) : 0u;  // xCalcHADs8x8: (sum + 2) >> 2
            sum = merge_pu_sum(t8, lane, n, s, horiz, horiz ? ly : lx, part);
          }
        }
        const unsigned sd = sum >> shift;  // the PU's sum, shifted once
        const unsigned c = sd + s_cost[i == 4 ? 4 : i + 1];   // MaxNumMergeCand 5: the last index saves its terminating bit
        if (i < num && c < best_c) { best_c = c; best_s = sd; best_v = qv; best_i = i; best_src = src; }
      }
      if (rep) {
        FhevcMotionMergeNode o;
        o.satd_best = best_s; o.cost_best = best_c;
        o.mvx = (short)(best_v & 0xFFFFu); o.mvy = (short)(best_v >> 16);
        o.idx = (uint8_t)best_i; o.num = (uint8_t)num; o.src = (uint8_t)best_src; o.pad = 0;
        if (small) out_small[oc * FHEVC_PUS_SMALL + entry] = o;
        else out_pus[oc * FHEVC_PUS + entry] = o;
      }
    }
  }
}

// one (T, PACKED, MR) instance: its dynamic LDS, and how many of its workgroups the device keeps on one CU (asked once per instance)
template <typename T, bool PACKED, int MR> struct MergePuInstance {
  static constexpr size_t LDS = MR > FHEVC_MOTION_MAX_RANGE ? (size_t)RefineGeom<MR>::SAMPLES * sizeof(short) : 0;   // MR = 64: 80 016 B
  static hipError_t resident(int* per_cu)
  {
    if (LDS) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&fhevc_motion_merge_pu_kernel<T, PACKED, MR>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS);
      if (e != hipSuccess) return e;
    }
    static std::atomic<int> asked{0};   // every device of a context is a gfx950: one answer per instance
    int n = asked.load(std::memory_order_relaxed);
    if (n == 0) {
      const hipError_t q = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fhevc_motion_merge_pu_kernel<T, PACKED, MR>, 256, LDS);
      if (q != hipSuccess) return q;
      asked.store(n, std::memory_order_relaxed);
    }
    *per_cu = n;
    return hipSuccess;
  }
};

template <typename T, bool PACKED, int MR>
hipError_t launch_merge_pu_at(const FhevcFrames& fr, int max_range, const FhevcMvBitCost& cost, const unsigned* refined, FhevcMotionMergeNode* d_out_pus,
                              FhevcMotionMergeNode* d_out_small, int num_cus, long long total, hipStream_t stream)
{
  using Inst = MergePuInstance<T, PACKED, MR>;
  int per_cu = 0;
  const hipError_t e = Inst::resident(&per_cu);
  if (e != hipSuccess) return e;
  if (per_cu < 1) return hipErrorLaunchOutOfResources;
  const long long resident = (long long)per_cu * num_cus;   // the persistent grid: what the device keeps resident
  const int grid = (int)(total < resident ? total : resident);
  hipLaunchKernelGGL((fhevc_motion_merge_pu_kernel<T, PACKED, MR>), dim3(grid), dim3(256), Inst::LDS, stream, fr, max_range, cost, refined, d_out_pus, d_out_small);
  return hipGetLastError();
}

template <typename T, bool PACKED>
hipError_t launch_merge_pu(const FhevcFrames& fr, int max_range, const FhevcMvBitCost& cost, const unsigned* refined, FhevcMotionMergeNode* d_out_pus,
                           FhevcMotionMergeNode* d_out_small, int num_cus, long long total, hipStream_t stream)
{
  if (max_range <= FHEVC_MOTION_MAX_RANGE)
    return launch_merge_pu_at<T, PACKED, FHEVC_MOTION_MAX_RANGE>(fr, max_range, cost, refined, d_out_pus, d_out_small, num_cus, total, stream);
  return launch_merge_pu_at<T, PACKED, FHEVC_MOTION_WIDE_MAX_RANGE>(fr, max_range, cost, refined, d_out_pus, d_out_small, num_cus, total, stream);
}

}  // namespace

hipError_t fhevc_launch_motion_merge_pu(const FhevcFrames& fr, int max_range, const FhevcMvBitCost& cost, const FhevcMotionQpelNode* d_refined,
                                        FhevcMotionMergeNode* d_out_pus, FhevcMotionMergeNode* d_out_small, int num_cus, hipStream_t stream)
{
  static_assert(sizeof(FhevcMotionQpelNode) == 16 && sizeof(FhevcMotionMergeNode) == 16, "record layouts");
  const long long total = (long long)(fr.row_end - fr.row_begin) * fr.ctus_x * (fr.num_frames - 1);
  if (total <= 0) return hipSuccess;
  if (max_range < 1 || max_range > FHEVC_MOTION_WIDE_MAX_RANGE || total > 0x7FFFFFFF || !d_refined || (!d_out_pus && !d_out_small)) return hipErrorInvalidValue;
  const unsigned* refined = reinterpret_cast<const unsigned*>(d_refined);
  if (fr.sample_bytes == 2 && fr.bit_depth <= 10) return launch_merge_pu<int16_t, true>(fr, max_range, cost, refined, d_out_pus, d_out_small, num_cus, total, stream);
  if (fr.sample_bytes == 2) return launch_merge_pu<int16_t, false>(fr, max_range, cost, refined, d_out_pus, d_out_small, num_cus, total, stream);
  return launch_merge_pu<uint8_t, true>(fr, max_range, cost, refined, d_out_pus, d_out_small, num_cus, total, stream);
}
