// k_p_tree.hip -- P-picture depth ranges from the selection's records, decided bottom-up over the quad-tree, on the device (config 4), gfx950 only.
//
// The device form of fhevc_p_tree_select (fhevc_host.hip; spec in include/fasthevc.h): per CTU the 85 records of fhevc_pu_shape_select_device, of which only
// cost_best is read; the best tree of every node against its own cost, the two decisions per node of levels 0..2, and the depth_min / depth_max maps as
// k_p_rule.hip writes them.  Integer arithmetic throughout, the same bits as the host code for any content of the records.
//
// A memory-bound pass: 1 360 B of records read per CTU (dword 1 of each is used), 512 B of maps and (optionally) 1 360 B of tree records written.  One wave per
// CTU, four per workgroup, grid-stride; no LDS, no workgroup barriers: waves are independent.
//   * lane i loads cost_best of node 21 + i, so a lane is an 8x8 node in raster position (x = i & 7, y = i >> 3); lanes 0..20 load nodes 0..20 in a second
//     load (the other lanes re-read node 20, in bounds); both loads are issued before the first is waited for;
//   * the three sums of four children are lane exchanges: xor 1 and xor 8, then xor 2 and xor 16, then xor 4 and xor 32.  What a node hands its parent
//     travels as one 64-bit value: its tree cost, 2^40 where that is the marker, 0 where no CU is coded; four of them never carry into each other, so the
//     high bits of a sum say whether a child was marked and the low 40 bits hold the 64-bit sum.  After each exchange all lanes of a node hold that node,
//     and every lane decides its three ancestors redundantly;
//   * a map leaves as one dword per lane (row lane >> 2, units 4 (lane & 3) .. + 3, all in ONE 16x16 node): the depths its three ancestors open come from
//     the lane at that 16x16 node's corner in one shuffle;
//   * the records of nodes 21 + lane are the lane's own; those of nodes 0..20 come to lanes 0..20 from one lane inside each node, chosen so that no lane
//     serves two nodes (16x16: its corner, even x and y; 32x32: x % 4 == 1, y % 4 == 0; the CTU: lane 8).
// Which lane and which address is read depends on lane and node numbers alone -- never on what the records hold.
// Two further families of instantiations take more records beside the selection's (the parameter pack of the kernel): the merge stage's (own = the smaller
// cost, bit 6) and, behind those, the skip stage's (fhevc_p_tree_select_skip_device: a merged node of level 0..2 with a masked zero bit is not descended).
// A fourth family takes the intra stage's records behind all of these (fhevc_p_tree_select_intra_device: a node of any level that is not such a calm one
// takes its intra cost where that is strictly smaller, bit 16 of the record's last dword).
// The rule (60 bytes) and the geometry are kernel arguments: two launches with different rules never share state (no per-context table).
#include "../../include/fasthevc.h"
#include "fhevc_internal.h"
#include <cstddef>

namespace {

constexpr uint32_t kMark = 0xFFFFFFFFu, kSat = 0xFFFFFFFEu;
constexpr uint64_t kMarked = 1ull << 40;

struct PTreeGeom {
  int width, height, ctus_x;   // the whole picture
  int row_begin, band_ctus;    // the band: first CTU row, CTUs per picture in it
  int total;                   // num_pictures * band_ctus
};

// flags: bit 0 split_sure, 1 stop_sure, 2 CROSSING, 3 ABSENT, 4 own available, 5 kids available; sure / maybe: whether depth_min / depth_max descend through the node
struct TreeNode { uint32_t own, kids, tree, flags; bool sure, maybe; };

// what a node hands its parent
__device__ __forceinline__ uint64_t share(uint32_t tree, bool absent) { return absent ? 0ull : (tree == kMark ? kMarked : (uint64_t)tree); }

__device__ __forceinline__ uint64_t sum4(uint64_t v, int a, int b)
{
  v += __shfl_xor(v, a);
  v += __shfl_xor(v, b);
  return v;
}

// the node of level L (0..2) at sample (x, y) of the CTU: cost_best of its record, the sum of what its four children hand it
// merged (the merge variants only): the record's merge cost is the smaller one -- bit 6 of an INSIDE node's flags
// skipped (the skip variant only): the node's skip record carries a masked bit; with merged, on an INSIDE node: HM's EarlyCU -- not descended, bit 7
// intra (the intra variant only): cost_best is the node's intra cost, taken by the lane that loaded it -- bit 16 of an INSIDE node's flags (byte 14 of the record)
template <int L>
__device__ __forceinline__ TreeNode decide(const FhevcPTreeRule& R, uint32_t cost_best, uint64_t sum, int x, int y, int valid_w, int valid_h, bool merged, bool skipped,
                                           bool intra = false)
{
  constexpr int S = 64 >> L;
  const bool inside = x + S <= valid_w && y + S <= valid_h, outside = x >= valid_w || y >= valid_h;
  TreeNode n;
  n.own = inside ? cost_best : kMark;
  const uint64_t total = (sum & (kMarked - 1)) + (inside ? (uint64_t)R.split_cost[L] : 0ull);
  n.kids = sum >= kMarked ? kMark : (total > kSat ? kSat : (uint32_t)total);
  n.tree = !inside ? n.kids : (n.kids == kMark ? n.own : (n.own == kMark ? n.kids : (n.kids < n.own ? n.kids : n.own)));
  bool split = false, stop = false;
  if (inside && n.own != kMark && n.kids != kMark) {
    split = (uint64_t)n.kids + (uint64_t)R.split_abs[L] + (((uint64_t)n.kids * (uint64_t)R.split_q8[L]) >> 8) < (uint64_t)n.own;
    stop = (uint64_t)n.own + (uint64_t)R.stop_abs[L] + (((uint64_t)n.own * (uint64_t)R.stop_q8[L]) >> 8) <= (uint64_t)n.kids;
  }
  const bool early = skipped && merged && inside;   // merged: own is a cost, not the marker
  if (early) { n.tree = n.own; split = false; stop = true; }
  n.sure = !inside || split;
  n.maybe = !inside || !stop;
  n.flags = (split ? 1u : 0u) | (stop ? 2u : 0u) | (!inside ? 4u : 0u) | (n.own != kMark ? 16u : 0u) | (n.kids != kMark ? 32u : 0u);
  if (merged && inside) n.flags |= 64u;
  if (early) n.flags |= 128u;
  if (intra && inside) n.flags |= 1u << 16;
  if (outside) { n.own = n.kids = n.tree = kMark; n.flags = 8u; }
  return n;
}

__device__ __forceinline__ void store_map(uint8_t* dst, uint32_t v, bool wide)
{
  if (wide) *reinterpret_cast<uint32_t*>(dst) = v;
  else { dst[0] = (uint8_t)v; dst[1] = (uint8_t)(v >> 8); dst[2] = (uint8_t)(v >> 16); dst[3] = (uint8_t)(v >> 24); }
}

__device__ __forceinline__ void store_record(uint32_t* dst, uint32_t own, uint32_t kids, uint32_t tree, uint32_t flags_level, bool wide)
{
  if (wide) *reinterpret_cast<uint4*>(dst) = make_uint4(own, kids, tree, flags_level);
  else { dst[0] = own; dst[1] = kids; dst[2] = tree; dst[3] = flags_level; }
}

// WIDE_MAPS: both map pointers are 4-byte aligned (dword stores; otherwise bytes); WIDE_TREE: tree is 16-byte aligned (16-byte stores; otherwise dwords)
// M... (fhevc_p_tree_select_merge_device): empty, or ONE const uint32_t* -- the records of k_motion_merge.hip beside the selection's, of which cost_best
// (dword 1) is read by the same lanes in the same two loads; a node's cost is the smaller of the two (the marker is the largest value, so it loses to any
// cost), bit 6 of its flags says that the merge cost is strictly smaller.  A pack keeps the plain instantiation's argument list, and so its code, what it was
// ... or THREE (fhevc_p_tree_select_skip_device): behind the merge records the records of k_motion_skip.hip as bytes and the mask on their flags (byte 10),
// read by lanes 0..20 in one byte load; the answer travels to the node's lanes in a shuffle of its own
// ... or FOUR (fhevc_p_tree_select_intra_device): behind those the records of k_intra_p.hip, of which cost_best (dword 1) is read by the same lanes in the
// same two loads, and one more byte load for the leaves' skip flags; whether the intra cost was taken travels like the merged bit
__device__ __forceinline__ const uint32_t* merge_of() { return nullptr; }
__device__ __forceinline__ const uint32_t* merge_of(const uint32_t* m) { return m; }
__device__ __forceinline__ const uint32_t* merge_of(const uint32_t* m, const uint8_t*, int) { return m; }
__device__ __forceinline__ const uint8_t* skip_of() { return nullptr; }
__device__ __forceinline__ const uint8_t* skip_of(const uint32_t*) { return nullptr; }
__device__ __forceinline__ const uint8_t* skip_of(const uint32_t*, const uint8_t* s, int) { return s; }
__device__ __forceinline__ int mask_of() { return 0; }
__device__ __forceinline__ int mask_of(const uint32_t*) { return 0; }
__device__ __forceinline__ int mask_of(const uint32_t*, const uint8_t*, int mask) { return mask; }
__device__ __forceinline__ const uint32_t* merge_of(const uint32_t* m, const uint8_t*, int, const uint32_t*) { return m; }
__device__ __forceinline__ const uint8_t* skip_of(const uint32_t*, const uint8_t* s, int, const uint32_t*) { return s; }
__device__ __forceinline__ int mask_of(const uint32_t*, const uint8_t*, int mask, const uint32_t*) { return mask; }
template <class... M> __device__ __forceinline__ const uint32_t* intra_of(M...) { return nullptr; }
__device__ __forceinline__ const uint32_t* intra_of(const uint32_t*, const uint8_t*, int, const uint32_t* i) { return i; }
template <bool WIDE_MAPS, bool WIDE_TREE, class... M>
__global__ __launch_bounds__(256) void fhevc_p_tree_kernel(PTreeGeom G, FhevcPTreeRule R, const uint32_t* __restrict__ shapes, uint8_t* __restrict__ depth_min,
                                                           uint8_t* __restrict__ depth_max, uint32_t* __restrict__ tree, M... merge_arg)
{
  constexpr bool MERGE = sizeof...(M) != 0, SKIP = sizeof...(M) >= 3, INTRA = sizeof...(M) == 4;
  const uint32_t* __restrict__ merge = merge_of(merge_arg...);
  const uint8_t* __restrict__ skip = skip_of(merge_arg...);
  const int skip_mask = mask_of(merge_arg...);
  const uint32_t* __restrict__ intra = intra_of(merge_arg...);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = (lane & 7) * 8, y = (lane >> 3) * 8;   // this lane's 8x8 node
  // where this lane's ancestors sit among lanes 0..20 of the second load
  const int k16 = 5 + (y >> 4) * 4 + (x >> 4), k32 = 1 + (y >> 5) * 2 + (x >> 5);
  // the map dword of this lane: its 16x16 node's corner lane
  const int map_src = (lane >> 4) * 16 + (lane & 3) * 2;
  // the record of node `lane` (lanes 0..20) comes from one lane inside that node
  const int rec_level = lane < 1 ? 0 : (lane < 5 ? 1 : 2);
  const int rec_src = lane < 1 ? 8 : (lane < 5 ? ((lane - 1) >> 1) * 32 + ((lane - 1) & 1) * 4 + 1 : (lane < 21 ? ((lane - 5) >> 2) * 16 + ((lane - 5) & 3) * 2 : 0));
  // ... and which of its ancestors this lane serves
  const int serves = (x & 8) == 0 && (y & 8) == 0 ? 2 : ((x & 24) == 8 && (y & 24) == 0 ? 1 : 0);

  for (int g = blockIdx.x * 4 + wave; g < G.total; g += gridDim.x * 4) {
    const int in_band = g % G.band_ctus;
    const int ctu = G.row_begin * G.ctus_x + in_band;
    const int x0 = (ctu % G.ctus_x) * 64, y0 = (ctu / G.ctus_x) * 64;
    const int valid_w = min(64, G.width - x0), valid_h = min(64, G.height - y0);
    const uint32_t* src = shapes + (size_t)g * (FHEVC_NODES * 4);
    uint32_t leaf = src[4 * (21 + lane) + 1], upper = src[4 * min(lane, 20) + 1];
    bool leaf_merged = false, upper_merged = false;
    if constexpr (MERGE) {
      const uint32_t* msrc = merge + (size_t)g * (FHEVC_NODES * 4);
      const uint32_t mleaf = msrc[4 * (21 + lane) + 1], mupper = msrc[4 * min(lane, 20) + 1];
      leaf_merged = mleaf < leaf; upper_merged = mupper < upper;
      leaf = leaf_merged ? mleaf : leaf; upper = upper_merged ? mupper : upper;
    }
    uint32_t us = 0u;
    if constexpr (SKIP) us = ((uint32_t)skip[(size_t)g * (FHEVC_NODES * 16) + 16 * min(lane, 20) + 10] & (uint32_t)skip_mask) != 0u ? 1u : 0u;
    // the intra cost where the node is not calm (merged, with a masked zero bit) and it is strictly smaller: a marker, the largest value, never is
    bool leaf_intra = false;
    uint32_t ui = 0u;
    if constexpr (INTRA) {
      const uint32_t* isrc = intra + (size_t)g * (FHEVC_NODES * 4);
      const uint32_t ileaf = isrc[4 * (21 + lane) + 1], iupper = isrc[4 * min(lane, 20) + 1];
      const bool leaf_zero = ((uint32_t)skip[(size_t)g * (FHEVC_NODES * 16) + 16 * (21 + lane) + 10] & (uint32_t)skip_mask) != 0u;
      leaf_intra = !(leaf_merged && leaf_zero) && ileaf < leaf;
      const bool upper_intra = !(upper_merged && us != 0u) && iupper < upper;
      leaf = leaf_intra ? ileaf : leaf; upper = upper_intra ? iupper : upper;
      ui = (uint32_t)upper_intra;
    }

    // ---- level 3: a leaf is coded iff it lies wholly inside ----
    const bool inside8 = x + 8 <= valid_w && y + 8 <= valid_h;
    const uint32_t own8 = inside8 ? leaf : kMark;
    // ---- levels 2, 1, 0: every lane decides the node around it ----
    // (the merge variant hands the "merged" bit along in bit 0 of a second shuffle; the plain one passes a constant)
    const uint32_t um = MERGE ? (uint32_t)upper_merged : 0u;
    const TreeNode n16 = decide<2>(R, __shfl(upper, k16), sum4(share(own8, !inside8), 1, 8), x & 48, y & 48, valid_w, valid_h, MERGE && __shfl(um, k16) != 0u,
                                    SKIP && __shfl(us, k16) != 0u, INTRA && __shfl(ui, k16) != 0u);
    const TreeNode n32 = decide<1>(R, __shfl(upper, k32), sum4(share(n16.tree, n16.flags == 8u), 2, 16), x & 32, y & 32, valid_w, valid_h, MERGE && __shfl(um, k32) != 0u,
                                    SKIP && __shfl(us, k32) != 0u, INTRA && __shfl(ui, k32) != 0u);
    const TreeNode n64 = decide<0>(R, __shfl(upper, 0), sum4(share(n32.tree, n32.flags == 8u), 4, 32), 0, 0, valid_w, valid_h, MERGE && __shfl(um, 0) != 0u,
                                    SKIP && __shfl(us, 0) != 0u, INTRA && __shfl(ui, 0) != 0u);

    // ---- the maps: the depths the decisions open top-down, 0 outside the picture ----
    if (depth_min || depth_max) {
      const bool lo64 = n64.sure, lo32 = lo64 && n32.sure, lo16 = lo32 && n16.sure;
      const bool hi64 = n64.maybe, hi32 = hi64 && n32.maybe, hi16 = hi32 && n16.maybe;
      const uint32_t opened = __shfl(((uint32_t)lo64 + (uint32_t)lo32 + (uint32_t)lo16) | ((uint32_t)hi64 + (uint32_t)hi32 + (uint32_t)hi16) << 8, map_src);
      const uint32_t lo = opened & 255u, hi = opened >> 8;
      uint32_t out_lo = 0, out_hi = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool inside = ((lane & 3) * 4 + k) * 4 < valid_w && (lane >> 2) * 4 < valid_h;
        out_lo |= (inside ? lo : 0u) << (8 * k);
        out_hi |= (inside ? hi : 0u) << (8 * k);
      }
      if (depth_min) store_map(depth_min + (size_t)g * 256 + 4 * lane, out_lo, WIDE_MAPS);
      if (depth_max) store_map(depth_max + (size_t)g * 256 + 4 * lane, out_hi, WIDE_MAPS);
    }

    // ---- the records: node 21 + lane from every lane, node `lane` from lanes 0..20 ----
    if (tree) {
      uint32_t* dst = tree + (size_t)g * (FHEVC_NODES * 4);
      store_record(dst + 4 * (21 + lane), own8, kMark, own8, (inside8 ? (own8 != kMark ? 16u : 0u) | (MERGE && leaf_merged ? 64u : 0u) | (INTRA && leaf_intra ? 1u << 16 : 0u) : 8u) | 3u << 8, WIDE_TREE);
      const TreeNode& mine = serves == 2 ? n16 : (serves == 1 ? n32 : n64);
      const uint32_t own = __shfl(mine.own, rec_src), kids = __shfl(mine.kids, rec_src), best = __shfl(mine.tree, rec_src), flags = __shfl(mine.flags, rec_src);
      if (lane < 21) store_record(dst + 4 * lane, own, kids, best, flags | (uint32_t)rec_level << 8, WIDE_TREE);
    }
  }
}

}  // namespace

static hipError_t launch_p_tree(const FhevcFrames& fr, const FhevcPTreeRule& rule, const FhevcPuShapeNode* d_shapes, const FhevcMotionMergeNode* d_merge, uint8_t* d_depth_min,
                                uint8_t* d_depth_max, FhevcPTreeNode* d_tree, int num_cus, hipStream_t stream, const FhevcMotionSkipNode* d_skip = nullptr, int skip_mask = 0,
                                const FhevcIntraPNode* d_intra = nullptr)
{
  static_assert(offsetof(FhevcIntraPNode, cost_best) == 4 && offsetof(FhevcPTreeNode, pad) == 14, "intra record layout, the tree record's byte 14");
  static_assert(sizeof(FhevcMotionSkipNode) == 16 && offsetof(FhevcMotionSkipNode, flags) == 10, "skip record layout");
  static_assert(sizeof(FhevcPuShapeNode) == 16 && sizeof(FhevcPTreeNode) == 16 && sizeof(FhevcPTreeRule) == 60 && sizeof(FhevcMotionMergeNode) == 16, "record layouts");
  PTreeGeom G;
  G.width = fr.width; G.height = fr.height; G.ctus_x = fr.ctus_x;
  G.row_begin = fr.row_begin; G.band_ctus = (fr.row_end - fr.row_begin) * fr.ctus_x;
  const long long total = (long long)G.band_ctus * fr.num_frames;
  if (total <= 0) return hipSuccess;
  if (total > 0x7FFFFFFF) return hipErrorInvalidValue;
  G.total = (int)total;
  long long grid = (total + 3) / 4;
  const long long cap = (long long)num_cus * 8;
  if (grid > cap) grid = cap;
  // the records are read as dwords whatever their alignment (4 bytes by type)
  const bool wide_maps = (((uintptr_t)d_depth_min | (uintptr_t)d_depth_max) & 3) == 0, wide_tree = ((uintptr_t)d_tree & 15) == 0;
  const uint32_t* shapes = reinterpret_cast<const uint32_t*>(d_shapes);
  const uint32_t* merge = reinterpret_cast<const uint32_t*>(d_merge);   // cost_best is dword 1 of a merge record too
  uint32_t* tree = reinterpret_cast<uint32_t*>(d_tree);
  const dim3 blocks((unsigned)grid), threads(256);
  if (d_intra) {
    const uint8_t* skip = reinterpret_cast<const uint8_t*>(d_skip);
    const uint32_t* intra = reinterpret_cast<const uint32_t*>(d_intra);   // cost_best is dword 1 of an intra record too
    if (wide_maps && wide_tree) hipLaunchKernelGGL((fhevc_p_tree_kernel<true, true, const uint32_t*, const uint8_t*, int, const uint32_t*>), blocks, threads, 0, stream, G, rule, shapes, d_depth_min, d_depth_max, tree, merge, skip, skip_mask, intra);
    else if (wide_maps) hipLaunchKernelGGL((fhevc_p_tree_kernel<true, false, const uint32_t*, const uint8_t*, int, const uint32_t*>), blocks, threads, 0, stream, G, rule, shapes, d_depth_min, d_depth_max, tree, merge, skip, skip_mask, intra);
    else if (wide_tree) hipLaunchKernelGGL((fhevc_p_tree_kernel<false, true, const uint32_t*, const uint8_t*, int, const uint32_t*>), blocks, threads, 0, stream, G, rule, shapes, d_depth_min, d_depth_max, tree, merge, skip, skip_mask, intra);
    else hipLaunchKernelGGL((fhevc_p_tree_kernel<false, false, const uint32_t*, const uint8_t*, int, const uint32_t*>), blocks, threads, 0, stream, G, rule, shapes, d_depth_min, d_depth_max, tree, merge, skip, skip_mask, intra);
  }
  else if (d_skip) {
    const uint8_t* skip = reinterpret_cast<const uint8_t*>(d_skip);
    if (wide_maps && wide_tree) hipLaunchKernelGGL((fhevc_p_tree_kernel<true, true, const uint32_t*, const uint8_t*, int>), blocks, threads, 0, stream, G, rule, shapes, d_depth_min, d_depth_max, tree, merge, skip, skip_mask);
    else if (wide_maps) hipLaunchKernelGGL((fhevc_p_tree_kernel<true, false, const uint32_t*, const uint8_t*, int>), blocks, threads, 0, stream, G, rule, shapes, d_depth_min, d_depth_max, tree, merge, skip, skip_mask);
    else if (wide_tree) hipLaunchKernelGGL((fhevc_p_tree_kernel<false, true, const uint32_t*, const uint8_t*, int>), blocks, threads, 0, stream, G, rule, shapes, d_depth_min, d_depth_max, tree, merge, skip, skip_mask);
    else hipLaunchKernelGGL((fhevc_p_tree_kernel<false, false, const uint32_t*, const uint8_t*, int>), blocks, threads, 0, stream, G, rule, shapes, d_depth_min, d_depth_max, tree, merge, skip, skip_mask);
  }
  else if (merge) {
    if (wide_maps && wide_tree) hipLaunchKernelGGL((fhevc_p_tree_kernel<true, true, const uint32_t*>), blocks, threads, 0, stream, G, rule, shapes, d_depth_min, d_depth_max, tree, merge);
    else if (wide_maps) hipLaunchKernelGGL((fhevc_p_tree_kernel<true, false, const uint32_t*>), blocks, threads, 0, stream, G, rule, shapes, d_depth_min, d_depth_max, tree, merge);
    else if (wide_tree) hipLaunchKernelGGL((fhevc_p_tree_kernel<false, true, const uint32_t*>), blocks, threads, 0, stream, G, rule, shapes, d_depth_min, d_depth_max, tree, merge);
    else hipLaunchKernelGGL((fhevc_p_tree_kernel<false, false, const uint32_t*>), blocks, threads, 0, stream, G, rule, shapes, d_depth_min, d_depth_max, tree, merge);
  }
  else if (wide_maps && wide_tree) hipLaunchKernelGGL((fhevc_p_tree_kernel<true, true>), blocks, threads, 0, stream, G, rule, shapes, d_depth_min, d_depth_max, tree);
  else if (wide_maps) hipLaunchKernelGGL((fhevc_p_tree_kernel<true, false>), blocks, threads, 0, stream, G, rule, shapes, d_depth_min, d_depth_max, tree);
  else if (wide_tree) hipLaunchKernelGGL((fhevc_p_tree_kernel<false, true>), blocks, threads, 0, stream, G, rule, shapes, d_depth_min, d_depth_max, tree);
  else hipLaunchKernelGGL((fhevc_p_tree_kernel<false, false>), blocks, threads, 0, stream, G, rule, shapes, d_depth_min, d_depth_max, tree);
  return hipGetLastError();
}

hipError_t fhevc_launch_p_tree(const FhevcFrames& fr, const FhevcPTreeRule& rule, const FhevcPuShapeNode* d_shapes, uint8_t* d_depth_min, uint8_t* d_depth_max,
                               FhevcPTreeNode* d_tree, int num_cus, hipStream_t stream)
{
  return launch_p_tree(fr, rule, d_shapes, nullptr, d_depth_min, d_depth_max, d_tree, num_cus, stream);
}

hipError_t fhevc_launch_p_tree_merge(const FhevcFrames& fr, const FhevcPTreeRule& rule, const FhevcPuShapeNode* d_shapes, const FhevcMotionMergeNode* d_merge,
                                     uint8_t* d_depth_min, uint8_t* d_depth_max, FhevcPTreeNode* d_tree, int num_cus, hipStream_t stream)
{
  if (!d_merge) return hipErrorInvalidValue;
  return launch_p_tree(fr, rule, d_shapes, d_merge, d_depth_min, d_depth_max, d_tree, num_cus, stream);
}

hipError_t fhevc_launch_p_tree_skip(const FhevcFrames& fr, const FhevcPTreeRule& rule, const FhevcPuShapeNode* d_shapes, const FhevcMotionMergeNode* d_merge,
                                    const FhevcMotionSkipNode* d_skip, int skip_mask, uint8_t* d_depth_min, uint8_t* d_depth_max, FhevcPTreeNode* d_tree, int num_cus,
                                    hipStream_t stream)
{
  if (!d_merge || !d_skip || skip_mask < 0 || skip_mask > 3) return hipErrorInvalidValue;
  return launch_p_tree(fr, rule, d_shapes, d_merge, d_depth_min, d_depth_max, d_tree, num_cus, stream, d_skip, skip_mask);
}

hipError_t fhevc_launch_p_tree_intra(const FhevcFrames& fr, const FhevcPTreeRule& rule, const FhevcPuShapeNode* d_shapes, const FhevcMotionMergeNode* d_merge,
                                     const FhevcMotionSkipNode* d_skip, int skip_mask, const FhevcIntraPNode* d_intra, uint8_t* d_depth_min, uint8_t* d_depth_max,
                                     FhevcPTreeNode* d_tree, int num_cus, hipStream_t stream)
{
  if (!d_merge || !d_skip || !d_intra || skip_mask < 0 || skip_mask > 3) return hipErrorInvalidValue;
  return launch_p_tree(fr, rule, d_shapes, d_merge, d_depth_min, d_depth_max, d_tree, num_cus, stream, d_skip, skip_mask, d_intra);
}
