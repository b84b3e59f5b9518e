// k_motion_merge_pu.hip -- source-only merge-candidate costs per PREDICTION UNIT (config 4: P slices), gfx950 only.
//
// TEncSearch::xMergeEstimation (TEncSearch.cpp:2831-2884) where HM runs it: for every PU of a CU whose partition size is not 2Nx2N (:3336, :3371), on the
// candidate list of TComDataCU::getInterMergeCandidates (TComDataCU.cpp:2142-2320); spec in include/fasthevc.h.  What k_motion_merge.hip prices for the 85
// square nodes, for the 508 PUs of k_motion_refine_pu.hip: the five samples L, A, AR, BL, AL around the PU's OWN rectangle, each mapped to the node of the
// CU's level that holds it, that node's refined square vector as the candidate; HM's order and pruning pairs, AL only below four entries, one zero vector
// below five; each entry priced as xGetHADs of the whole w x h PU at that quarter-sample vector + getCost(bits of the merge index): 1, 2, 3, 4, 4.
//
// Mapping and arithmetic are k_refine_tile.h's: workgroup (4 waves) = one CTU at a time over a persistent grid; the window staged once per CTU
// (refine_stage_window_reach in both layouts; MR = 8: static LDS, MR = 64: dynamic); lane = one 8x8 tile; the 26 passes of RefinePuPass dealt to the four
// waves and a PU's sum by refine_pu_had, as in k_motion_refine_pu.hip; the list by MergeList, as in k_motion_merge.hip.  The candidate loop of a pass is at
// most 5 long.  Where the list comes from is this kernel's own: the lane's PU changes per pass, and so do its five neighbour nodes.  The nodes that can be a
// neighbour of any PU of the CTU are parked in LDS once per CTU, before the passes: the CTU's own 85 nodes, the right column of the left CTU and the bottom
// row of the upper CTU (15 each), the corner nodes of the two upper diagonal CTUs (4 each) -- 123 dwords.  A parked dword is the node's vector if the node is on the grid, INSIDE, in
// a CTU row of the band, no marker and within the reach 4 max_range + 3; otherwise mvx = -32768, which no reach admits.  (CTUs to the right and below
// follow in coding order: none of their nodes is ever available.)  What a pass adds per lane is the coding-order test inside the own CTU -- the z-index of
// the neighbour strictly below that of the PU's own CU, which also excludes the own CU, HM's two second-PU rules -- and five LDS reads whose addresses depend
// on the geometry alone.  LDS on top of the window: 492 B parked + 96 B tables (MR = 64: two workgroups per CU leave 1 680 B each).
// No scratch, no HBM state between calls: the bit costs travel by value.
#include "fhevc_internal.h"
#include "k_had8x8.h"
#include "k_refine_tile.h"

namespace {

constexpr unsigned kNoVector = 0x00008000u;   // mvx = -32768, mvy = 0: beyond any reach
constexpr int kParked = 123;                  // 85 own + 15 left + 15 upper + 4 upper-left + 4 upper-right
constexpr int kLeft = 85, kUpper = 100, kUpLeft = 115, kUpRight = 119;

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
  const int total = SearchWork::total(F);  // frame f >= 1 is predicted from frame f - 1
  const int shift = F.bit_depth - 8;
  const RefineArith arith(F.bit_depth);
  const T* plane = reinterpret_cast<const T*>(F.luma);
  const int pass_begin = out_pus ? 0 : PASSES_PU, pass_end = out_small ? PASSES : PASSES_PU;
  const int reach = vec_reach(max_range);
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
    const SearchWork W(F, work);
    const int cy = W.cy, cx = W.cx;
    const long long oc = W.oc(F);
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
    refine_stage_window_reach<T, MR>(s_ref, plane, W.ref_base, F, cx, cy, tid, max_range);
    if (tid < kParked) s_nb[tid] = pcost != kMergeMark && vec_in_reach(pvec, reach) ? pvec : kNoVector;
    // ---- this lane's original 8x8 tile (all four waves hold the same 64 tiles) ----
    const int px = cx * 64 + tx * 8, py = cy * 64 + ty * 8;
    const bool inside = (px + 8 <= F.width) && (py + 8 <= F.height);
    unsigned O[32];
    load_tile8x8(plane, W.cur_base, F, px, py, inside, O);
    __syncthreads();

#pragma unroll 1
    for (int pass = pass_begin + wave; pass < pass_end; pass += 4) {
      const RefinePuPass U(pass, tx, ty);  // the pass's covering and this lane's PU in it (pass is wave-uniform)
      const int nsize = U.nsize(), lvl = 3 - U.n, s = U.s;
      const bool horiz = U.horiz, node_in = search_node_inside(F, cx, cy, U.nbx, U.nby, nsize);
      // ---- the PU's rectangle inside the CTU (getPartIndexAndSize), its five samples, their nodes, the list ----
      const int cut_s = s < 2 ? nsize / 2 : (s & 1) ? 3 * nsize / 4 : nsize / 4;
      const int far = U.part ? cut_s : 0, len = U.part ? nsize - cut_s : cut_s;  // along the cut's normal: where the part begins, how long it is
      const int x0 = U.nbx * nsize + (horiz ? 0 : far), y0 = U.nby * nsize + (horiz ? far : 0);
      const int w = horiz ? nsize : len, h = horiz ? len : nsize;
      const unsigned zme = merge_z((unsigned)U.nbx, (unsigned)U.nby);
      unsigned nvec[5];
      bool av[5];
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const int sx = j == 1 ? x0 + w - 1 : (j == 2 ? x0 + w : x0 - 1);                      // L, A, AR, BL, AL
        const int sy = j == 0 ? y0 + h - 1 : (j == 3 ? y0 + h : y0 - 1);
        const int rx = sx >> (6 - lvl), ry = sy >> (6 - lvl);                                 // arithmetic: -1 stays -1
        const int slot = parked_slot(lvl, rx, ry);
        const bool own = rx >= 0 && ry >= 0 && slot >= 0;                                     // inside the own CTU: coding order by z-index
        const bool ok = node_in && slot >= 0 && (!own || merge_z((unsigned)rx, (unsigned)ry) < zme);
        nvec[j] = s_nb[slot < 0 ? 0 : slot];
        av[j] = ok && nvec[j] != kNoVector;
      }
      const MergeList list(av, nvec, node_in);
      const int longest = list.longest();

      MergeBest best;
#pragma unroll 1
      for (int i = 0; i < longest; ++i) {
        unsigned qv;
        int src;
        list.pick(i, qv, src);
        const unsigned sd = refine_pu_had<PACKED, RP>(s_ref, s_taps, arith, lane, tx, ty, U, vec_x(qv), vec_y(qv), O, inside) >> shift;  // the PU's sum, shifted once
        best.offer(i, list.num, sd + merge_index_cost(s_cost, i), sd, qv, src);
      }
      if (U.rep) (U.small ? out_small : out_pus)[U.record(oc)] = best.record(list.num);
    }
  }
}

}  // namespace

// the persistent grid of either layout: what the device keeps resident
hipError_t fhevc_launch_motion_merge_pu(const FhevcFrames& fr, int max_range, const FhevcMvBitCost& cost, const FhevcMotionQpelNode* d_refined,
                                        FhevcMotionMergeNode* d_out_pus, FhevcMotionMergeNode* d_out_small, int num_cus, hipStream_t stream)
{
  static_assert(sizeof(FhevcMotionQpelNode) == 16 && sizeof(FhevcMotionMergeNode) == 16, "record layouts");
  const unsigned* refined = reinterpret_cast<const unsigned*>(d_refined);
  return refine_launch<FHEVC_MOTION_WIDE_MAX_RANGE>(fr, d_refined && (d_out_pus || d_out_small), max_range, num_cus, {0, true}, {0, true}, stream,
                                                    [&](auto t, auto packed, auto mr, const RefineLaunch& L) {
    return refine_launch_kernel<&fhevc_motion_merge_pu_kernel<decltype(t), decltype(packed)::value, decltype(mr)::value>>(L, fr, max_range, cost, refined, d_out_pus, d_out_small);
  });
}
