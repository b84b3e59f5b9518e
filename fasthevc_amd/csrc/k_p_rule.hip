// k_p_rule.hip -- P-picture depth ranges on the device (config 4), gfx950 only.
//
// The device form of the host rule in fhevc_host.hip (fhevc_p_depth_range): per CTU the 85 motion nodes that fhevc_motion_search_device
// wrote, the reference picture's depths obtained in one of three ways (co-located; exactly fhevc_p_motion_compensated_depth; exactly
// fhevc_p_node_depth), then exactly fhevc_p_depth_range.  Integer arithmetic throughout, the same bits as the host code for any 32-bit field
// values and any int16 vectors -- including where the host code wraps ((uint32_t)gain + 1u and (uint32_t)child_satd + 1u truncate 64-bit sums).
// The host code evaluates the 21 split decisions lazily; here all 21 are evaluated, which gives the same maps because a node's decision is
// only consumed under open parents.
//
// A memory-bound pass of about 2.1 KB per CTU (1 360 B of nodes, 256 B of depths, 512 B written).  One wave per CTU, four per workgroup,
// grid-stride; no workgroup barriers: waves are independent.
//   * nodes: 16-byte loads, one node per lane in two rounds, parked in the wave's LDS image (every LDS read is a dword or wider);
//   * the reference depths never touch LDS: lane l owns the four horizontally adjacent 4x4 units of dword l of the CTU's 256-byte map
//     (row l / 4, units 4 (l % 4) .. + 3), which all lie in ONE 16x16 block, so the largest / smallest depth inside a 16x16, 32x32 and 64x64
//     node meet through lane shuffles (lane = 16 * block_row + 4 * unit_row + block_col);
//   * 21 lanes that end up holding a node's extremes compute its split score (64-bit, Q18); the decisions travel as two ballots;
//   * every lane writes one dword to each map: a wave writes each 256-byte map as one coalesced row.
// The rule (148 bytes) is a kernel argument: two launches with different rules never share state (no per-context table).
#include "../../include/fasthevc.h"   // FHEVC_P_PREV_*
#include "fhevc_internal.h"

namespace {

__device__ __forceinline__ int32_t ilog2_q8(uint32_t x)  // floor(256 log2 x) by integer squaring (x = 0 as x = 1)
{
  const int msb = 31 - __builtin_clz(x | 1u);
  uint64_t y = ((uint64_t)x << 31) >> msb;
  int32_t r = msb << 8;
#pragma unroll
  for (int b = 7; b >= 0; --b) {
    y = (y * y) >> 31;
    if (y >> 32) { r |= 1 << b; y >>= 1; }
  }
  return r;
}

__device__ __forceinline__ int max4(uint32_t v) { return max(max((int)(v & 255), (int)((v >> 8) & 255)), max((int)((v >> 16) & 255), (int)(v >> 24))); }
__device__ __forceinline__ int min4(uint32_t v) { return min(min((int)(v & 255), (int)((v >> 8) & 255)), min((int)((v >> 16) & 255), (int)(v >> 24))); }

// the vector of a node, or `parent` when the node crosses the picture edge (cost_best 0xFFFFFFFF); node: (satd_zero, satd_best, cost_best, mvx | mvy << 16)
__device__ __forceinline__ int2 vector_of(const uint4& node, int2 parent)
{
  return node.z != 0xFFFFFFFFu ? make_int2((int)(int16_t)(node.w & 0xFFFFu), (int)(int16_t)(node.w >> 16)) : parent;
}

struct PRuleGeom {
  int width, height, ctus_x, num_ctus;   // the whole picture
  int row_begin, band_ctus;              // the band: first CTU row, CTUs per picture in it
  int total;                             // num_pictures * band_ctus
};

// depth of the reference picture at sample (x, y), clamped to the picture (the host code's ref_depth)
__device__ __forceinline__ uint32_t ref_depth(const uint8_t* __restrict__ map, const PRuleGeom& G, int x, int y)
{
  x = min(max(x, 0), G.width - 1); y = min(max(y, 0), G.height - 1);
  return map[(size_t)((y >> 6) * G.ctus_x + (x >> 6)) * 256 + ((y & 63) >> 2) * 16 + ((x & 63) >> 2)];
}

// MODE: FHEVC_P_PREV_*; WIDE: every pointer is aligned for 16-byte node loads and dword map accesses (otherwise dword node loads, byte map accesses)
template <int MODE, bool WIDE>
__global__ __launch_bounds__(256) void fhevc_p_rule_kernel(PRuleGeom G, int qp, FhevcPRule R, const uint32_t* __restrict__ nodes,
                                                           const uint8_t* __restrict__ prev_maps, uint8_t* __restrict__ depth_min,
                                                           uint8_t* __restrict__ depth_max)
{
  __shared__ uint4 node_image[4][88];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint4* nd = node_image[wave];
  // lane = 16 * by + 4 * r + bx: 16x16 block (bx, by) of the CTU, unit row r of it; the lane's four units are that block's row
  const int bx = lane & 3, r = (lane >> 2) & 3, by = lane >> 4;
  // the node this lane scores, if any: the lanes with r == 0 the 16x16 node of their block, four lanes with r == 1 the 32x32 node of
  // their quadrant, one lane with r == 2 the CTU -- each of them holds that node's depth extremes after the shuffles below
  const int lvl = r == 0 ? 2 : (r == 1 ? 1 : 0);
  const bool scores = r == 0 || (r == 1 && !(by & 1) && !(bx & 1)) || (r == 2 && by == 0 && bx == 0);
  const int nx = bx >> (2 - lvl), ny = by >> (2 - lvl);
  const int first = lvl == 0 ? 0 : (lvl == 1 ? 1 : 5), first_child = lvl == 0 ? 1 : (lvl == 1 ? 5 : 21);
  const int node_id = first + ny * (1 << lvl) + nx;
  const int child_id = first_child + 2 * ny * (2 << lvl) + 2 * nx;
  // the rule's row of this lane's level: constant indices only (a lane-indexed kernel argument would live in scratch)
  int32_t w[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) w[i] = lvl == 0 ? R.w[0][i] : (lvl == 1 ? R.w[1][i] : R.w[2][i]);
  const int64_t t_split = lvl == 0 ? R.t_split[0] : (lvl == 1 ? R.t_split[1] : R.t_split[2]);
  const int64_t t_stop = lvl == 0 ? R.t_stop[0] : (lvl == 1 ? R.t_stop[1] : R.t_stop[2]);
  const int norm = 512 * (6 - lvl) + (qp * 256) / 6;
  // where the three ancestors' decisions of this lane's units sit in the ballots
  const int bit64 = 8, bit32 = 32 * (by >> 1) + 2 * (bx >> 1) + 4, bit16 = 16 * by + bx;

  for (int g = blockIdx.x * 4 + wave; g < G.total; g += gridDim.x * 4) {
    const int p = g / G.band_ctus, in_band = g - p * G.band_ctus;
    const int ctu = G.row_begin * G.ctus_x + in_band;
    const int x0 = (ctu % G.ctus_x) * 64, y0 = (ctu / G.ctus_x) * 64;
    const int valid_w = min(64, G.width - x0), valid_h = min(64, G.height - y0);
    const uint32_t* src = nodes + (size_t)g * (FHEVC_NODES * 4);
    if (WIDE) {
      nd[lane] = reinterpret_cast<const uint4*>(src)[lane];
      if (lane < FHEVC_NODES - 64) nd[64 + lane] = reinterpret_cast<const uint4*>(src)[64 + lane];
    } else {
      nd[lane] = make_uint4(src[4 * lane], src[4 * lane + 1], src[4 * lane + 2], src[4 * lane + 3]);
      if (lane < FHEVC_NODES - 64) nd[64 + lane] = make_uint4(src[256 + 4 * lane], src[257 + 4 * lane], src[258 + 4 * lane], src[259 + 4 * lane]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    // ---- the reference picture's depths of this lane's four units, one byte each ----
    const uint8_t* map = prev_maps + (size_t)p * G.num_ctus * 256;
    uint32_t prev;
    if (MODE == FHEVC_P_PREV_COLOCATED) {
      const uint8_t* own = map + (size_t)ctu * 256 + 4 * lane;
      prev = WIDE ? *reinterpret_cast<const uint32_t*>(own) : (uint32_t)own[0] | (uint32_t)own[1] << 8 | (uint32_t)own[2] << 16 | (uint32_t)own[3] << 24;
    } else {
      // the vectors of the enclosing nodes, top-down; all three positions depend on the nodes only, so the loads are independent
      const uint4 n64 = nd[0], n32 = nd[1 + (by >> 1) * 2 + (bx >> 1)], n16 = nd[5 + by * 4 + bx];
      if (MODE == FHEVC_P_PREV_UNIT) {
        // fhevc_p_motion_compensated_depth: the vector of the smallest valid node around the block (16x16, 32x32, the CTU, else zero)
        const int2 v = vector_of(n16, vector_of(n32, vector_of(n64, make_int2(0, 0))));
        const int py = y0 + by * 16 + r * 4 + 2 + v.y;
        prev = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) prev |= ref_depth(map, G, x0 + bx * 16 + k * 4 + 2 + v.x, py) << (8 * k);
      } else {
        // fhevc_p_node_depth: the depth at each node's displaced centre; a node not deeper than its level becomes one CU
        const int2 v0 = vector_of(n64, make_int2(0, 0)), v1 = vector_of(n32, v0), v2 = vector_of(n16, v1);
        const uint32_t d0 = ref_depth(map, G, x0 + 32 + v0.x, y0 + 32 + v0.y);
        const uint32_t d1 = ref_depth(map, G, x0 + (bx >> 1) * 32 + 16 + v1.x, y0 + (by >> 1) * 32 + 16 + v1.y);
        const uint32_t d2 = ref_depth(map, G, x0 + bx * 16 + 8 + v2.x, y0 + by * 16 + 8 + v2.y);
        prev = (d0 == 0 ? 0u : (d1 <= 1 ? 1u : (d2 <= 2 ? 2u : 3u))) * 0x01010101u;
      }
    }

    // ---- largest / smallest reference depth inside the 16x16, 32x32 and 64x64 node around this lane ----
    int deep16 = max4(prev), shallow16 = min4(prev);
    deep16 = max(deep16, __shfl_xor(deep16, 4)); shallow16 = min(shallow16, __shfl_xor(shallow16, 4));
    deep16 = max(deep16, __shfl_xor(deep16, 8)); shallow16 = min(shallow16, __shfl_xor(shallow16, 8));
    int deep32 = max(deep16, __shfl_xor(deep16, 1)), shallow32 = min(shallow16, __shfl_xor(shallow16, 1));
    deep32 = max(deep32, __shfl_xor(deep32, 16)); shallow32 = min(shallow32, __shfl_xor(shallow32, 16));
    int deep64 = max(deep32, __shfl_xor(deep32, 2)), shallow64 = min(shallow32, __shfl_xor(shallow32, 2));
    deep64 = max(deep64, __shfl_xor(deep64, 32)); shallow64 = min(shallow64, __shfl_xor(shallow64, 32));

    // ---- split decisions: score > t_split ("sure"), score >= -t_stop ("maybe"); nodes crossing the picture edge split in both ----
    bool sure = false, maybe = false;
    if (scores) {
      const int size = 64 >> lvl;
      if (nx * size + size > valid_w || ny * size + size > valid_h) sure = maybe = true;
      else {
        const uint4 n = nd[node_id];
        uint64_t child_cost = 0, child_satd = 0;
        int moved = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint4 c = nd[child_id + (k >> 1) * (2 << lvl) + (k & 1)];
          child_cost += c.z; child_satd += c.y;
          moved += c.w != n.w;   // (mvx, mvy) as one word
        }
        const int deepest = lvl == 0 ? deep64 : (lvl == 1 ? deep32 : deep16), shallowest = min(3, lvl == 0 ? shallow64 : (lvl == 1 ? shallow32 : shallow16));
        const int64_t gain = max((int64_t)0, (int64_t)n.z - (int64_t)child_cost);
        const int32_t l_best = ilog2_q8(n.y + 1u);
        const int32_t f[9] = { l_best - norm, ilog2_q8((uint32_t)gain + 1u) - norm, ilog2_q8((uint32_t)child_satd + 1u) - norm, ilog2_q8(n.x + 1u) - l_best,
                               deepest > lvl ? 256 : 0, shallowest > lvl ? 256 : 0, deepest > lvl + 1 ? 256 : 0, 64 * moved, 8 * qp };
        int64_t s = w[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) s += (int64_t)w[i] * (int64_t)f[i];
        sure = s > t_split;
        maybe = s >= -t_stop;
      }
    }
    const unsigned long long sure_mask = __ballot(sure), maybe_mask = __ballot(maybe);

    // ---- the lane's units: depths the decisions open top-down (the same for all four), the window clip per unit, 0 outside the picture ----
    const bool lo64 = (sure_mask >> bit64) & 1, lo32 = lo64 && ((sure_mask >> bit32) & 1), lo16 = lo32 && ((sure_mask >> bit16) & 1);
    const bool hi64 = (maybe_mask >> bit64) & 1, hi32 = hi64 && ((maybe_mask >> bit32) & 1), hi16 = hi32 && ((maybe_mask >> bit16) & 1);
    const int lo_tree = (int)lo64 + (int)lo32 + (int)lo16, hi_tree = (int)hi64 + (int)hi32 + (int)hi16;
    uint32_t out_lo = 0, out_hi = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int lo = lo_tree, hi = hi_tree;
      if (R.window < 4) {
        const int pd = (int)((prev >> (8 * k)) & 255);
        lo = min(3, max(0, max(lo, pd - R.window)));
        hi = min(3, max(0, min(hi, pd + R.window)));
        if (lo > hi) lo = hi;
      }
      const bool inside = (bx * 4 + k) * 4 < valid_w && (by * 4 + r) * 4 < valid_h;
      out_lo |= (inside ? (uint32_t)lo : 0u) << (8 * k);
      out_hi |= (inside ? (uint32_t)hi : 0u) << (8 * k);
    }
    uint8_t* dst_lo = depth_min + (size_t)g * 256 + 4 * lane;
    if (WIDE) *reinterpret_cast<uint32_t*>(dst_lo) = out_lo;
    else { dst_lo[0] = (uint8_t)out_lo; dst_lo[1] = (uint8_t)(out_lo >> 8); dst_lo[2] = (uint8_t)(out_lo >> 16); dst_lo[3] = (uint8_t)(out_lo >> 24); }
    if (depth_max) {
      uint8_t* dst_hi = depth_max + (size_t)g * 256 + 4 * lane;
      if (WIDE) *reinterpret_cast<uint32_t*>(dst_hi) = out_hi;
      else { dst_hi[0] = (uint8_t)out_hi; dst_hi[1] = (uint8_t)(out_hi >> 8); dst_hi[2] = (uint8_t)(out_hi >> 16); dst_hi[3] = (uint8_t)(out_hi >> 24); }
    }
    __builtin_amdgcn_wave_barrier();  // the next CTU of this wave overwrites the node image
  }
}

template <int MODE>
void launch_mode(bool wide, unsigned grid, hipStream_t stream, const PRuleGeom& G, int qp, const FhevcPRule& rule, const uint32_t* nodes,
                 const uint8_t* prev_maps, uint8_t* depth_min, uint8_t* depth_max)
{
  if (wide) hipLaunchKernelGGL((fhevc_p_rule_kernel<MODE, true>), dim3(grid), dim3(256), 0, stream, G, qp, rule, nodes, prev_maps, depth_min, depth_max);
  else hipLaunchKernelGGL((fhevc_p_rule_kernel<MODE, false>), dim3(grid), dim3(256), 0, stream, G, qp, rule, nodes, prev_maps, depth_min, depth_max);
}

}  // namespace

hipError_t fhevc_launch_p_rule(const FhevcFrames& fr, int prev_mode, const FhevcPRule& rule, const FhevcMotionNode* d_nodes, const uint8_t* d_prev_maps,
                               uint8_t* d_depth_min, uint8_t* d_depth_max, int num_cus, hipStream_t stream)
{
  PRuleGeom G;
  G.width = fr.width; G.height = fr.height; G.ctus_x = fr.ctus_x; G.num_ctus = fr.ctus_x * fr.ctus_y;
  G.row_begin = fr.row_begin; G.band_ctus = (fr.row_end - fr.row_begin) * fr.ctus_x;
  const long long total = (long long)G.band_ctus * fr.num_frames;
  if (total <= 0) return hipSuccess;
  if (total > 0x7FFFFFFF) return hipErrorInvalidValue;
  G.total = (int)total;
  long long grid = (total + 3) / 4;
  const long long cap = (long long)num_cus * 8;
  if (grid > cap) grid = cap;
  const uintptr_t all = (uintptr_t)d_prev_maps | (uintptr_t)d_depth_min | (uintptr_t)d_depth_max;
  const bool wide = ((uintptr_t)d_nodes & 15) == 0 && (all & 3) == 0;
  const uint32_t* nodes = reinterpret_cast<const uint32_t*>(d_nodes);
  switch (prev_mode) {
    case FHEVC_P_PREV_COLOCATED: launch_mode<FHEVC_P_PREV_COLOCATED>(wide, (unsigned)grid, stream, G, fr.qp, rule, nodes, d_prev_maps, d_depth_min, d_depth_max); break;
    case FHEVC_P_PREV_UNIT: launch_mode<FHEVC_P_PREV_UNIT>(wide, (unsigned)grid, stream, G, fr.qp, rule, nodes, d_prev_maps, d_depth_min, d_depth_max); break;
    case FHEVC_P_PREV_NODE: launch_mode<FHEVC_P_PREV_NODE>(wide, (unsigned)grid, stream, G, fr.qp, rule, nodes, d_prev_maps, d_depth_min, d_depth_max); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
