// k_pu_shape.hip -- partition sizes per CU from the refined PU costs, on the device (config 4), gfx950 only.
//
// The device form of fhevc_pu_shape_select (fhevc_host.hip; spec in include/fasthevc.h): per CTU the 85 refined nodes, the 124 refined PUs and the 384
// refined small PUs, added up per partition size, then best / second in HM's checking order and the mask of the sizes within the margin.  Integer
// arithmetic throughout, the same bits as the host code for any content of the entries.
//
// A memory-bound pass: 9 488 B read per CTU, 1 360 B of records and (optionally) 2 720 B of costs written.  One wave per CTU, four per workgroup, grid-stride;
// no workgroup barriers: waves are independent.
//   * entries: one entry per lane in ten rounds (2 of nodes, 2 of PUs, 6 of small PUs); only the cost_best dword of each is read and parked in the wave's
//     LDS image: 593 dwords, nodes at 0, PUs at 85, small PUs at 209.  Without d_pus_small that part of the image holds the marker.  (A 16-byte load per
//     entry, as k_p_rule.hip issues where it needs whole nodes, is narrowed by the compiler to this dword: see park_costs);
//   * lanes 0..63, then 0..20, own nodes 0..63 and 64..84: a lane reads its node's cost and the (at most) twelve parts from LDS as dwords.  Which dwords
//     depends on the node number alone -- never on what the entries hold --, so every LDS read stays inside the image for any input;
//   * a record leaves as one 16-byte store, the eight costs as two, where both output pointers are 16-byte aligned; as dwords otherwise.
// The rule (36 bytes) and the geometry are kernel arguments: two launches with different rules never share state (no per-context table).
//
// The merge form (fhevc_pu_shape_select_merge_device): two further instantiations that also get the PUs' merge records (k_motion_merge_pu.hip) and park, per
// PU entry, the SMALLER of the refined cost_best and the merge cost_best (dword 1 of a merge record) -- HM's uiMRGCost < uiMECost -- and one flag byte that says
// which it was: 8 128 B more read per CTU, 2 048 B more LDS, and optionally 170 B of "merged" bits written.  Everything behind the image is the same code.
#include "../../include/fasthevc.h"   // FHEVC_PART_*
#include "fhevc_internal.h"

namespace {

constexpr int kImage = FHEVC_NODES + FHEVC_PUS + FHEVC_PUS_SMALL;   // 593 cost_best dwords per CTU
constexpr uint32_t kNone = 0xFFFFFFFFu;

struct PuShapeGeom {
  int width, height, ctus_x;   // the whole picture
  int row_begin, band_ctus;    // the band: first CTU row, CTUs per picture in it
  int total;                   // num_pictures * band_ctus
};

// cost_best (dword 2) of COUNT 16-byte entries, one entry per lane and round, all rounds' loads issued before the first is waited for.  A round past the end
// re-reads the last entry (in bounds) and parks nothing.  hipcc narrows a 16-byte load of which only .z is used to this dword load anyway -- the other twelve
// bytes are dead, and the same cache lines come from HBM either way --, so both instantiations of the kernel read entries alike; they differ in the stores
template <int COUNT>
__device__ __forceinline__ void park_costs(uint32_t* dst, const uint32_t* __restrict__ src, int lane)
{
  constexpr int ROUNDS = (COUNT + 63) / 64;
  uint32_t v[ROUNDS];
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) v[r] = src[4 * min(lane + 64 * r, COUNT - 1) + 2];
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r)
    if (lane + 64 * r < COUNT) dst[lane + 64 * r] = v[r];
}

// the merge variant's: per entry the smaller of the refined entry's cost_best (dword 2; src null: the marker) and of its merge record's (dword 1; merge null:
// the marker) into dst, and into flg whether the merge cost is strictly the smaller one
template <int COUNT>
__device__ __forceinline__ void park_min_costs(uint32_t* dst, uint8_t* flg, const uint32_t* __restrict__ src, const uint32_t* __restrict__ merge, int lane)
{
  constexpr int ROUNDS = (COUNT + 63) / 64;
  uint32_t a[ROUNDS], m[ROUNDS];
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const int e = min(lane + 64 * r, COUNT - 1);
    a[r] = src ? src[4 * e + 2] : kNone;
    m[r] = merge ? merge[4 * e + 1] : kNone;
  }
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r)
    if (lane + 64 * r < COUNT) { dst[lane + 64 * r] = min(a[r], m[r]); flg[lane + 64 * r] = m[r] < a[r] ? 1 : 0; }
}

// the sum of a shape's two parts: unavailable if either is, otherwise saturated below the marker
__device__ __forceinline__ uint32_t pair_cost(const uint32_t* img, int e0)
{
  const uint32_t a = img[e0], b = img[e0 + 1];
  const uint64_t s = (uint64_t)a + b;
  return a == kNone || b == kNone ? kNone : (s > 0xFFFFFFFEull ? 0xFFFFFFFEu : (uint32_t)s);
}

// what the merge variant gets beside the plain form's arguments: the merge records of the 124 and of the 384 PUs (small may be null), and where the
// "merged" bits go (may be null)
struct PuShapeMerge { const uint32_t *pus, *small; uint16_t* merged; };

// WIDE: both output pointers are 16-byte aligned (16-byte stores; otherwise dwords)
// M... (fhevc_pu_shape_select_merge_device): empty, or ONE PuShapeMerge -- a part then costs the smaller of its refined cost and its merge cost (HM's uiMRGCost <
// uiMECost, TEncSearch.cpp:3373).  A pack keeps the plain instantiations' argument list, and so their code, what it was
template <bool WIDE, class... M>
__global__ __launch_bounds__(256) void fhevc_pu_shape_kernel(PuShapeGeom G, FhevcPuShapeRule R, const uint32_t* __restrict__ nodes, const uint32_t* __restrict__ pus,
                                                             const uint32_t* __restrict__ pus_small, uint32_t* __restrict__ shapes, uint32_t* __restrict__ costs,
                                                             M... merge_arg)
{
  constexpr bool MERGE = sizeof...(M) != 0;
  __shared__ uint32_t cost_image[4][kImage + 3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t* img = cost_image[wave];
  uint8_t* flg = nullptr;   // the merge variant: per PU entry of the image, whether its merge cost was the smaller one
  if constexpr (MERGE) {
    __shared__ uint8_t merged_image[4][FHEVC_PUS + FHEVC_PUS_SMALL + 4];
    flg = merged_image[wave];
  }

  for (int g = blockIdx.x * 4 + wave; g < G.total; g += gridDim.x * 4) {
    const int in_band = g % G.band_ctus;
    const int ctu = G.row_begin * G.ctus_x + in_band;
    const int x0 = (ctu % G.ctus_x) * 64, y0 = (ctu / G.ctus_x) * 64;
    const int valid_w = min(64, G.width - x0), valid_h = min(64, G.height - y0);
    park_costs<FHEVC_NODES>(img, nodes + (size_t)g * (FHEVC_NODES * 4), lane);
    if constexpr (MERGE) {
      const PuShapeMerge mg = (merge_arg, ...);
      park_min_costs<FHEVC_PUS>(img + FHEVC_NODES, flg, pus + (size_t)g * (FHEVC_PUS * 4), mg.pus + (size_t)g * (FHEVC_PUS * 4), lane);
      park_min_costs<FHEVC_PUS_SMALL>(img + FHEVC_NODES + FHEVC_PUS, flg + FHEVC_PUS, pus_small ? pus_small + (size_t)g * (FHEVC_PUS_SMALL * 4) : nullptr,
                                      mg.small ? mg.small + (size_t)g * (FHEVC_PUS_SMALL * 4) : nullptr, lane);
    } else {
      park_costs<FHEVC_PUS>(img + FHEVC_NODES, pus + (size_t)g * (FHEVC_PUS * 4), lane);
      if (pus_small) park_costs<FHEVC_PUS_SMALL>(img + FHEVC_NODES + FHEVC_PUS, pus_small + (size_t)g * (FHEVC_PUS_SMALL * 4), lane);
      else
        for (int e = lane; e < FHEVC_PUS_SMALL; e += 64) img[FHEVC_NODES + FHEVC_PUS + e] = kNone;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

#pragma unroll
    for (int round = 0; round < 2; ++round) {
      const int k = lane + 64 * round;
      if (k >= FHEVC_NODES) break;
      const int lvl = k < 1 ? 0 : (k < 5 ? 1 : (k < 21 ? 2 : 3));
      const int first = lvl == 0 ? 0 : (lvl == 1 ? 1 : (lvl == 2 ? 5 : 21));
      const int size = 64 >> lvl, nx = (k - first) & ((1 << lvl) - 1), ny = (k - first) >> lvl;
      const bool valid = nx * size + size <= valid_w && ny * size + size <= valid_h;
      // where part 0 of the two symmetric shapes (p = 1, 2) and of the four AMP shapes (p = 4..7) sits in the image: fhevc_motion_pu_index behind the nodes,
      // fhevc_motion_pu_small_index behind the PUs; part 1 follows part 0.  -1: not covered (AMP of the 8x8 nodes)
      const int sym = lvl < 2 ? FHEVC_NODES + k * 12 : (lvl == 2 ? FHEVC_NODES + 60 + (k - 5) * 4 : FHEVC_NODES + FHEVC_PUS + 128 + (k - 21) * 4);
      const int amp = lvl < 2 ? FHEVC_NODES + k * 12 + 4 : (lvl == 2 ? FHEVC_NODES + FHEVC_PUS + (k - 5) * 8 : -1);
      uint32_t c[8];
#pragma unroll
      for (int p = 0; p < 8; ++p) c[p] = kNone;
      if (valid) {
        c[0] = img[k];
        c[1] = pair_cost(img, sym);
        c[2] = pair_cost(img, sym + 2);
        if (amp >= 0) {
#pragma unroll
          for (int p = 4; p < 8; ++p) c[p] = pair_cost(img, amp + (p - 4) * 2);
        }
      }
      // best and second in HM's checking order 0, 2, 1, 4, 5, 6, 7, strict "<" (a marker is never smaller than the initial marker)
      constexpr int order[7] = { FHEVC_PART_2Nx2N, FHEVC_PART_Nx2N, FHEVC_PART_2NxN, FHEVC_PART_2NxnU, FHEVC_PART_2NxnD, FHEVC_PART_nLx2N, FHEVC_PART_nRx2N };
      uint32_t c_best = kNone, c_second = kNone, best = 255, second = 255, avail = 0;
#pragma unroll
      for (int i = 0; i < 7; ++i) {
        const int p = order[i];
        avail |= c[p] != kNone ? 1u << p : 0u;
        if (c[p] < c_best) { c_best = c[p]; best = p; }
      }
#pragma unroll
      for (int i = 0; i < 7; ++i) {
        const int p = order[i];
        if ((uint32_t)p != best && c[p] < c_second) { c_second = c[p]; second = p; }
      }
      const int32_t m_q8 = lvl == 0 ? R.margin_q8[0] : (lvl == 1 ? R.margin_q8[1] : (lvl == 2 ? R.margin_q8[2] : R.margin_q8[3]));
      const int32_t m_abs = lvl == 0 ? R.margin_abs[0] : (lvl == 1 ? R.margin_abs[1] : (lvl == 2 ? R.margin_abs[2] : R.margin_abs[3]));
      const uint64_t limit = (uint64_t)c_best + (uint64_t)m_abs + (((uint64_t)c_best * (uint64_t)m_q8) >> 8);
      uint32_t mask = 1;   // HM always checks 2Nx2N
      if (best != 255) {
#pragma unroll
        for (int p = 0; p < 8; ++p) mask |= c[p] != kNone && c[p] <= limit ? 1u << p : 0u;
      }
      if (R.amp_mode == 1) {
        // TEncCu::deriveTestModeAMP without its merge / skip conditions (not visible to a source-only pass)
        uint32_t c3 = kNone;
        int b3 = -1;
#pragma unroll
        for (int i = 0; i < 3; ++i)
          if (c[order[i]] < c3) { c3 = c[order[i]]; b3 = order[i]; }
        if (!(b3 == FHEVC_PART_2Nx2N || b3 == FHEVC_PART_2NxN)) mask &= ~0x30u;
        if (!(b3 == FHEVC_PART_2Nx2N || b3 == FHEVC_PART_Nx2N)) mask &= ~0xC0u;
      }
      if (!valid) mask = 0;
      const uint4 rec = make_uint4(c[0], c_best, c_second, best | second << 8 | mask << 16 | avail << 24);
      uint32_t* dst = shapes + ((size_t)g * FHEVC_NODES + k) * 4;
      if (WIDE) *reinterpret_cast<uint4*>(dst) = rec;
      else { dst[0] = rec.x; dst[1] = rec.y; dst[2] = rec.z; dst[3] = rec.w; }
      if (costs) {
        uint32_t* cd = costs + ((size_t)g * FHEVC_NODES + k) * 8;
        if (WIDE) {
          reinterpret_cast<uint4*>(cd)[0] = make_uint4(c[0], c[1], c[2], c[3]);
          reinterpret_cast<uint4*>(cd)[1] = make_uint4(c[4], c[5], c[6], c[7]);
        } else {
#pragma unroll
          for (int p = 0; p < 8; ++p) cd[p] = c[p];
        }
      }
      if constexpr (MERGE) {
        const PuShapeMerge mg = (merge_arg, ...);
        if (mg.merged) {
          // bit 2 p + part: that part's merge cost is strictly smaller than its refined cost; p = 0 stays the explicit cost, an invalid node has none
          uint32_t bits = 0;
          if (valid) {
            const uint8_t* fs = flg + (sym - FHEVC_NODES);
            bits = (uint32_t)fs[0] << 2 | (uint32_t)fs[1] << 3 | (uint32_t)fs[2] << 4 | (uint32_t)fs[3] << 5;
            if (amp >= 0) {
              const uint8_t* fa = flg + (amp - FHEVC_NODES);
#pragma unroll
              for (int e = 0; e < 8; ++e) bits |= (uint32_t)fa[e] << (8 + e);
            }
          }
          mg.merged[(size_t)g * FHEVC_NODES + k] = (uint16_t)bits;
        }
      }
    }
    __builtin_amdgcn_wave_barrier();  // the next CTU of this wave overwrites the image
  }
}

}  // namespace

// d_merge_pus: null for the plain form
static hipError_t launch_pu_shape(const FhevcFrames& fr, const FhevcPuShapeRule& rule, const FhevcMotionQpelNode* d_nodes, const FhevcMotionQpelNode* d_pus,
                                  const FhevcMotionQpelNode* d_pus_small, const FhevcMotionMergeNode* d_merge_pus, const FhevcMotionMergeNode* d_merge_small,
                                  FhevcPuShapeNode* d_shapes, uint32_t* d_costs, uint16_t* d_merged, int num_cus, hipStream_t stream)
{
  static_assert(sizeof(FhevcMotionQpelNode) == 16 && sizeof(FhevcPuShapeNode) == 16 && sizeof(FhevcMotionMergeNode) == 16, "entry layout");
  PuShapeGeom G;
  G.width = fr.width; G.height = fr.height; G.ctus_x = fr.ctus_x;
  G.row_begin = fr.row_begin; G.band_ctus = (fr.row_end - fr.row_begin) * fr.ctus_x;
  const long long total = (long long)G.band_ctus * fr.num_frames;
  if (total <= 0) return hipSuccess;
  if (total > 0x7FFFFFFF) return hipErrorInvalidValue;
  G.total = (int)total;
  long long grid = (total + 3) / 4;
  const long long cap = (long long)num_cus * 8;
  if (grid > cap) grid = cap;
  // 16-byte stores need both outputs aligned (records and costs are 4-byte aligned by type); the entries are read as dwords whatever their alignment
  const uintptr_t all = (uintptr_t)d_shapes | (uintptr_t)d_costs;
  const uint32_t* nodes = reinterpret_cast<const uint32_t*>(d_nodes);
  const uint32_t* pus = reinterpret_cast<const uint32_t*>(d_pus);
  const uint32_t* small = reinterpret_cast<const uint32_t*>(d_pus_small);
  uint32_t* shapes = reinterpret_cast<uint32_t*>(d_shapes);
  if (d_merge_pus) {
    // cost_best is dword 1 of a merge record; the records are read as dwords whatever their alignment, the "merged" bits leave as 2-byte stores
    const PuShapeMerge mg = { reinterpret_cast<const uint32_t*>(d_merge_pus), reinterpret_cast<const uint32_t*>(d_merge_small), d_merged };
    if ((all & 15) == 0) hipLaunchKernelGGL((fhevc_pu_shape_kernel<true, PuShapeMerge>), dim3((unsigned)grid), dim3(256), 0, stream, G, rule, nodes, pus, small, shapes, d_costs, mg);
    else hipLaunchKernelGGL((fhevc_pu_shape_kernel<false, PuShapeMerge>), dim3((unsigned)grid), dim3(256), 0, stream, G, rule, nodes, pus, small, shapes, d_costs, mg);
    return hipGetLastError();
  }
  if ((all & 15) == 0) hipLaunchKernelGGL((fhevc_pu_shape_kernel<true>), dim3((unsigned)grid), dim3(256), 0, stream, G, rule, nodes, pus, small, shapes, d_costs);
  else hipLaunchKernelGGL((fhevc_pu_shape_kernel<false>), dim3((unsigned)grid), dim3(256), 0, stream, G, rule, nodes, pus, small, shapes, d_costs);
  return hipGetLastError();
}

hipError_t fhevc_launch_pu_shape(const FhevcFrames& fr, const FhevcPuShapeRule& rule, const FhevcMotionQpelNode* d_nodes, const FhevcMotionQpelNode* d_pus,
                                 const FhevcMotionQpelNode* d_pus_small, FhevcPuShapeNode* d_shapes, uint32_t* d_costs, int num_cus, hipStream_t stream)
{
  return launch_pu_shape(fr, rule, d_nodes, d_pus, d_pus_small, nullptr, nullptr, d_shapes, d_costs, nullptr, num_cus, stream);
}

hipError_t fhevc_launch_pu_shape_merge(const FhevcFrames& fr, const FhevcPuShapeRule& rule, const FhevcMotionQpelNode* d_nodes, const FhevcMotionQpelNode* d_pus,
                                       const FhevcMotionQpelNode* d_pus_small, const FhevcMotionMergeNode* d_merge_pus, const FhevcMotionMergeNode* d_merge_small,
                                       FhevcPuShapeNode* d_shapes, uint32_t* d_costs, uint16_t* d_merged, int num_cus, hipStream_t stream)
{
  if (!d_merge_pus) return hipErrorInvalidValue;
  return launch_pu_shape(fr, rule, d_nodes, d_pus, d_pus_small, d_merge_pus, d_merge_small, d_shapes, d_costs, d_merged, num_cus, stream);
}
