// k_motion_amvp.hip -- refined motion costs re-priced against neighbour predictors (config 4: P slices), gfx950 only.
//
// HM prices an explicit vector against an AMVP predictor, not against zero: predInterSearch calls xEstimateMvPredAMVP (TEncSearch.cpp:3028), xMotionEstimation
// and xPatternSearchFracDIF run under setPredictor(mvp), and xCheckBestMVP (:3566-3615) keeps the predictor of fewest bits; the list is
// TComDataCU::fillMvpCand (TComDataCU.cpp:2578-2716).  Spec in include/fasthevc.h (fhevc_motion_amvp*).  This stage reads NO samples: per entry -- one of the
// 85 nodes, 124 PUs, 384 small PUs of a CTU -- the refined record, the refined square vectors of the same-level nodes at the five positions L, A, AR, BL, AL
// around the entry's rectangle, and for part 1 of a PU the refined vector of part 0 of the same partition size; out goes the record with cost_best =
// satd_best + getCost(bits of q - p) for the cheaper of the two predictors.
//
// A memory-bound pass: 9 488 B of records read and as many written per CTU, 4 744 B of predictor records where asked for, a few dozen integer operations
// per entry.  Workgroup (4 waves) = one CTU at a time, grid-stride over the band's CTUs of all picture pairs:
//   * the 123 nodes that can be a neighbour of any entry of the CTU are parked in LDS once per CTU, laid out as k_motion_merge_pu.hip parks them (the own 85,
//     the right column of the left CTU, the bottom row of the upper CTU, the corner nodes of the two upper diagonal CTUs) but without a reach test: a parked
//     slot is (vector, available), available iff the node is on the grid, INSIDE, in a CTU row of the band and no marker.  Which record a thread parks
//     depends on geometry and band alone;
//   * the 593 entries in three rounds of one record per lane: round A waves 0..1 the nodes, waves 2..3 the PUs, rounds B and C the small PUs.  All of a
//     thread's record loads are issued before the barrier behind the parking.  A record comes and goes as one 16-byte access where every record pointer
//     is 16-byte aligned and every predictor pointer 8-byte aligned (WIDE); as dwords otherwise -- pointers 4 bytes off are as good;
//   * where an entry's five candidates are parked, which of them coding order admits and which is part 0 of the own CU depends on the entry alone: a
//     thread works that out once for its three entries, before the CTU loop, and keeps it packed in six registers -- per CTU and entry there remain five
//     LDS reads, the list and the price;
//   * part 0 of a PU sits in the lane before part 1's (both PU orders keep part 1 behind part 0 and start on an even entry): one cross-lane read, no LDS;
//   * the list and the choice are fhevc_mvp_choose (fhevc_internal.h), the code the host twin runs.
// A round past a family's end re-reads the family's last entry (in bounds) and stores nothing.  No scratch, no HBM state between calls: the 67 bit costs and
// the geometry travel by value.
#include "fhevc_internal.h"

namespace {

constexpr uint32_t kMark = 0xFFFFFFFFu;
constexpr int kParked = 123;                  // 85 own + 15 left + 15 upper + 4 upper-left + 4 upper-right
constexpr int kLeft = 85, kUpper = 100, kUpLeft = 115, kUpRight = 119;

struct AmvpGeom {
  int width, height, ctus_x;   // the whole picture
  int row_begin, band_ctus;    // the band: first CTU row, CTUs per picture pair in it
  int total;                   // picture pairs * band_ctus
};

// where the same-level node at (rx, ry) relative to the CTU's grid of 2^lvl x 2^lvl nodes is parked; -1: a CTU that follows in coding order
__device__ __forceinline__ int parked_slot(int lvl, int rx, int ry)
{
  const int ncnt = 1 << lvl, first = ((1 << (2 * lvl)) - 1) / 3;
  if (ry >= ncnt || (rx >= ncnt && ry >= 0)) return -1;
  if (ry < 0) return rx < 0 ? kUpLeft + lvl : (rx >= ncnt ? kUpRight + lvl : kUpper + ncnt - 1 + rx);
  return rx < 0 ? kLeft + ncnt - 1 + ry : first + ry * ncnt + rx;
}

// the bit interleave of a node's place in its CTU, x in the even bits
__device__ __forceinline__ unsigned z_index(unsigned x, unsigned y)
{
  const unsigned sx = (x & 1u) | ((x & 2u) << 1) | ((x & 4u) << 2), sy = (y & 1u) | ((y & 2u) << 1) | ((y & 4u) << 2);
  return sx | (sy << 1);
}

template <bool WIDE> __device__ __forceinline__ uint4 load_record(const uint32_t* p)
{
  if (WIDE) return *reinterpret_cast<const uint4*>(p);
  return make_uint4(p[0], p[1], p[2], p[3]);
}

// family: 0 the nodes, 1 the PUs (fhevc_motion_pu_index), 2 the small PUs (fhevc_motion_pu_small_index); wave-uniform
struct AmvpEntry {
  int lvl, bx, by;        // the entry's CU node: level, place on the CTU's grid of that level
  int x0, y0, w, h;       // the entry's rectangle inside the CTU
  bool part1;             // part 1 of a PU
  __device__ __forceinline__ AmvpEntry(int family, int e)
  {
    int k, s = -1;
    if (family == 0) k = e;
    else if (family == 1) { k = e < 60 ? e / 12 : 5 + (e - 60) / 4; s = e < 60 ? (e % 12) >> 1 : ((e - 60) & 3) >> 1; }
    else { k = e < 128 ? 5 + e / 8 : 21 + (e - 128) / 4; s = e < 128 ? 2 + ((e & 7) >> 1) : ((e - 128) & 3) >> 1; }
    part1 = family != 0 && (e & 1);
    lvl = k < 1 ? 0 : (k < 5 ? 1 : (k < 21 ? 2 : 3));
    const int i = k - ((1 << (2 * lvl)) - 1) / 3, size = 64 >> lvl;
    bx = i & ((1 << lvl) - 1); by = i >> lvl;
    x0 = bx * size; y0 = by * size; w = size; h = size;
    if (s >= 0) {
      // getPartIndexAndSize: shapes 0 2NxN, 1 Nx2N, 2 2NxnU, 3 2NxnD, 4 nLx2N, 5 nRx2N
      const bool horiz = s == 0 || s == 2 || s == 3;
      const int cut = s < 2 ? size / 2 : ((s & 1) ? 3 * size / 4 : size / 4);
      const int far = part1 ? cut : 0, len = part1 ? size - cut : cut;
      if (horiz) { y0 += far; h = len; } else { x0 += far; w = len; }
    }
  }
};

template <bool WIDE>
__global__ __launch_bounds__(256) void fhevc_motion_amvp_kernel(AmvpGeom G, FhevcMvpBitCost cost, const uint32_t* __restrict__ nodes, const uint32_t* __restrict__ pus,
                                                                const uint32_t* __restrict__ small, uint32_t* __restrict__ out_nodes, uint32_t* __restrict__ out_pus,
                                                                uint32_t* __restrict__ out_small, uint32_t* __restrict__ mvp_nodes, uint32_t* __restrict__ mvp_pus,
                                                                uint32_t* __restrict__ mvp_small)
{
  __shared__ uint2 s_nb[kParked];              // x: the node's vector, y: available
  __shared__ uint32_t s_cost[FHEVC_MVP_BIT_COSTS];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (tid < FHEVC_MVP_BIT_COSTS) s_cost[tid] = cost.c[tid];
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
  // the three rounds of this thread: (family, entry), wave-uniform family; an entry past the family's end is clamped for the load and stores nothing
  const int fam_a = wave < 2 ? 0 : 1, e_a = wave < 2 ? tid : tid - 128, cnt_a = wave < 2 ? FHEVC_NODES : FHEVC_PUS;
  const uint32_t* const in_a = wave < 2 ? nodes : pus;
  uint32_t* const out_a = wave < 2 ? out_nodes : out_pus;
  uint32_t* const mvp_a = wave < 2 ? mvp_nodes : mvp_pus;
  const bool do_a = in_a && (out_a || mvp_a), do_s = small && (out_small || mvp_small);
  // What of an entry's five candidates depends on the entry alone, worked out once per thread and round, before the CTU loop:
  //   geo_slots  a byte per position L, A, AR, BL: where its node is parked
  //   geo_rest   bits 0..7 the slot of AL; 8..12 per position: on this side of the coding order (a CTU that follows: not; inside the own CTU: by z-index);
  //              13..17 per position: inside the entry's own CU (only L or A of a part 1); 18..24 and 25..31: the right and the lower edge of the CU in the CTU
  uint32_t geo_slots[3], geo_rest[3];
#pragma unroll
  for (int round = 0; round < 3; ++round) {
    const int family = round == 0 ? fam_a : 2, cnt = round == 0 ? cnt_a : FHEVC_PUS_SMALL;
    const AmvpEntry E(family, min(round == 0 ? e_a : tid + 256 * (round - 1), cnt - 1));
    const int size = 64 >> E.lvl, cu_x = E.bx * size, cu_y = E.by * size;
    const unsigned zme = z_index((unsigned)E.bx, (unsigned)E.by);
    uint32_t slots = 0, rest = (uint32_t)(cu_x + size) << 18 | (uint32_t)(cu_y + size) << 25;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int sx = j == 1 ? E.x0 + E.w - 1 : (j == 2 ? E.x0 + E.w : E.x0 - 1);                      // L, A, AR, BL, AL
      const int sy = j == 0 ? E.y0 + E.h - 1 : (j == 3 ? E.y0 + E.h : E.y0 - 1);
      const bool own_cu = sx >= cu_x && sx < cu_x + size && sy >= cu_y && sy < cu_y + size;
      const int rx = sx >> (6 - E.lvl), ry = sy >> (6 - E.lvl);                                     // arithmetic: -1 stays -1
      const int slot = parked_slot(E.lvl, rx, ry);
      const bool own_ctu = rx >= 0 && ry >= 0 && slot >= 0;
      const bool admitted = slot >= 0 && (!own_ctu || z_index((unsigned)rx, (unsigned)ry) < zme);
      const uint32_t where = (uint32_t)min(max(slot, 0), kParked - 1);
      if (j < 4) slots |= where << (8 * j);
      else rest |= where;
      rest |= (admitted ? 1u : 0u) << (8 + j) | (own_cu ? 1u : 0u) << (13 + j);
    }
    geo_slots[round] = slots; geo_rest[round] = rest;
  }

  for (int g = blockIdx.x; g < G.total; g += gridDim.x) {
    const int in_band = g % G.band_ctus, ctu = G.row_begin * G.ctus_x + in_band;
    const int cx = ctu % G.ctus_x, cy = ctu / G.ctus_x;
    // ---- the node to park: its address from geometry and band alone ----
    uint32_t pcost = kMark, pvec = 0;
    if (tid < kParked) {
      const int ncx = cx + p_dcx, ncy = cy + p_dcy;
      const int gx = ncx * (1 << p_lvl) + p_bx, gy = ncy * (1 << p_lvl) + p_by;
      const bool ok = ncx >= 0 && ncx < G.ctus_x && ncy >= G.row_begin && gx < (G.width >> (6 - p_lvl)) && gy < (G.height >> (6 - p_lvl));
      if (ok) {
        const size_t rec = ((size_t)(g + p_dcy * G.ctus_x + p_dcx) * FHEVC_NODES + ((1 << (2 * p_lvl)) - 1) / 3 + p_by * (1 << p_lvl) + p_bx) * 4;
        pcost = nodes[rec + 2]; pvec = nodes[rec + 3];
      }
    }
    // ---- this thread's records, all loads in flight before the barrier ----
    uint4 r[3];
    r[0] = r[1] = r[2] = make_uint4(0, 0, kMark, 0);
    if (do_a) r[0] = load_record<WIDE>(in_a + ((size_t)g * cnt_a + min(e_a, cnt_a - 1)) * 4);
    if (do_s) {
      r[1] = load_record<WIDE>(small + ((size_t)g * FHEVC_PUS_SMALL + tid) * 4);
      r[2] = load_record<WIDE>(small + ((size_t)g * FHEVC_PUS_SMALL + min(tid + 256, FHEVC_PUS_SMALL - 1)) * 4);
    }
    __syncthreads();  // the previous CTU's readers are done
    if (tid < kParked) s_nb[tid] = make_uint2(pvec, pcost != kMark ? 1u : 0u);
    __syncthreads();

#pragma unroll
    for (int round = 0; round < 3; ++round) {
      const int e = round == 0 ? e_a : tid + 256 * (round - 1), cnt = round == 0 ? cnt_a : FHEVC_PUS_SMALL;
      if (!(round == 0 ? do_a : do_s)) continue;
      if (round == 2 && wave >= 2) continue;   // entries 256..383: waves 0 and 1
      const uint4 rec = r[round];
      // part 0 of this lane's PU: the lane before (an odd lane's; for the nodes it is not looked at)
      const uint32_t part0_cost = __shfl_xor(rec.z, 1), part0_vec = __shfl_xor(rec.w, 1);
      if (e >= cnt) continue;
      const uint32_t gs = geo_slots[round], gr = geo_rest[round];
      const bool inside = cx * 64 + (int)((gr >> 18) & 127u) <= G.width && cy * 64 + (int)(gr >> 25) <= G.height;
      bool av_l, av_a, av_ar, av_bl, av_al;
      uint32_t v_l, v_a, v_ar, v_bl, v_al;
      // position j, a constant at each of the five calls below
      auto candidate = [&](int j, bool& avail, uint32_t& v) {
        const uint2 nb = s_nb[j < 4 ? (gs >> (8 * j)) & 255u : gr & 255u];
        const bool own_cu = (gr >> (13 + j)) & 1u;
        avail = own_cu ? part0_cost != kMark : ((gr >> (8 + j)) & 1u) != 0 && nb.y != 0;
        v = own_cu ? part0_vec : nb.x;
      };
      candidate(0, av_l, v_l); candidate(1, av_a, v_a); candidate(2, av_ar, v_ar); candidate(3, av_bl, v_bl); candidate(4, av_al, v_al);
      const FhevcMvpChoice c = fhevc_mvp_choose(av_l, av_a, av_ar, av_bl, av_al, v_l, v_a, v_ar, v_bl, v_al, rec.w);
      const bool priced = inside && rec.z != kMark;
      uint4 o = rec;                                                                                  // an input marker record is copied as it is
      if (priced) {
        const uint64_t sum = (uint64_t)rec.y + s_cost[c.bits];
        o.z = sum > 0xFFFFFFFEull ? 0xFFFFFFFEu : (uint32_t)sum;
      }
      if (!inside) o = make_uint4(kMark, kMark, kMark, 0);
      uint32_t* const out = round == 0 ? out_a : out_small;
      uint32_t* const mvp = round == 0 ? mvp_a : mvp_small;
      if (out) {
        uint32_t* dst = out + ((size_t)g * cnt + e) * 4;
        if (WIDE) *reinterpret_cast<uint4*>(dst) = o;
        else { dst[0] = o.x; dst[1] = o.y; dst[2] = o.z; dst[3] = o.w; }
      }
      if (mvp) {
        const uint2 m = priced ? make_uint2(c.pred, (uint32_t)c.idx | (uint32_t)c.num_spatial << 8 | (uint32_t)c.src << 16 | (uint32_t)c.bits << 24) : make_uint2(0u, 0x00FF00FFu);
        uint32_t* dst = mvp + ((size_t)g * cnt + e) * 2;
        if (WIDE) *reinterpret_cast<uint2*>(dst) = m;
        else { dst[0] = m.x; dst[1] = m.y; }
      }
    }
  }
}

}  // namespace

hipError_t fhevc_launch_motion_amvp(const FhevcFrames& fr, const FhevcMvpBitCost& cost, const FhevcMotionQpelNode* d_nodes, const FhevcMotionQpelNode* d_pus,
                                    const FhevcMotionQpelNode* d_pus_small, FhevcMotionQpelNode* d_out_nodes, FhevcMotionQpelNode* d_out_pus,
                                    FhevcMotionQpelNode* d_out_small, FhevcMotionMvp* d_mvp_nodes, FhevcMotionMvp* d_mvp_pus, FhevcMotionMvp* d_mvp_small, int num_cus,
                                    hipStream_t stream)
{
  static_assert(sizeof(FhevcMotionQpelNode) == 16, "record layout");
  if (!d_nodes || (!d_pus && (d_out_pus || d_mvp_pus)) || (!d_pus_small && (d_out_small || d_mvp_small))) return hipErrorInvalidValue;
  if (!d_out_nodes && !d_out_pus && !d_out_small && !d_mvp_nodes && !d_mvp_pus && !d_mvp_small) return hipErrorInvalidValue;
  AmvpGeom G;
  G.width = fr.width; G.height = fr.height; G.ctus_x = fr.ctus_x;
  G.row_begin = fr.row_begin; G.band_ctus = (fr.row_end - fr.row_begin) * fr.ctus_x;
  const long long total = (long long)G.band_ctus * fr.num_frames;
  if (total <= 0) return hipSuccess;
  if (total > 0x7FFFFFFF) return hipErrorInvalidValue;
  G.total = (int)total;
  const long long cap = (long long)num_cus * 8;
  const unsigned grid = (unsigned)(total < cap ? total : cap);
  // 16-byte accesses need every record pointer 16-byte and every predictor pointer 8-byte aligned (a CTU's share is a multiple of both); dwords otherwise
  const uintptr_t recs = (uintptr_t)d_nodes | (uintptr_t)d_pus | (uintptr_t)d_pus_small | (uintptr_t)d_out_nodes | (uintptr_t)d_out_pus | (uintptr_t)d_out_small;
  const uintptr_t preds = (uintptr_t)d_mvp_nodes | (uintptr_t)d_mvp_pus | (uintptr_t)d_mvp_small;
  auto u = [](const void* p) { return reinterpret_cast<const uint32_t*>(p); };
  auto v = [](void* p) { return reinterpret_cast<uint32_t*>(p); };
  if ((recs & 15) == 0 && (preds & 7) == 0)
    hipLaunchKernelGGL((fhevc_motion_amvp_kernel<true>), dim3(grid), dim3(256), 0, stream, G, cost, u(d_nodes), u(d_pus), u(d_pus_small), v(d_out_nodes), v(d_out_pus),
                       v(d_out_small), v(d_mvp_nodes), v(d_mvp_pus), v(d_mvp_small));
  else
    hipLaunchKernelGGL((fhevc_motion_amvp_kernel<false>), dim3(grid), dim3(256), 0, stream, G, cost, u(d_nodes), u(d_pus), u(d_pus_small), v(d_out_nodes), v(d_out_pus),
                       v(d_out_small), v(d_mvp_nodes), v(d_mvp_pus), v(d_mvp_small));
  return hipGetLastError();
}
