// k_intra_p.hip -- intra candidate costs per CU node for P pictures, from the records of the two intra first passes, on the device (config 4), gfx950 only.
//
// The device form of fhevc_intra_p_picture (fhevc_host.hip; spec in include/fasthevc.h): per CTU the 85 records of k_firstpass.hip and (optionally) the 256
// records of k_firstpass4.hip, of which satd and mode (dwords 0 and 1) are read -- never the double --; per node the integer price satd + getCost(bits(mode)) of
// the first pass's winner, and for an 8x8 node the better of 2Nx2N and NxN (the four 4x4 PUs), in the record form the tree of k_p_tree.hip reads (cost_best
// is dword 1).  Integer arithmetic throughout, the same bits as the host code for any content of the input bytes.
//
// A pass over records that reads no samples: 5 456 B in, 1 360 B out per CTU.  The mapping is k_p_tree.hip's: one wave per CTU, four per workgroup,
// grid-stride; no LDS, no barrier, no lane exchange -- every record is computed by the lane that loads its inputs.
//   * lane i is 8x8 node 21 + i at (x = i & 7, y = i >> 3): it loads that node's record and the records of its four PUs (2x, 2y), (2x + 1, 2y), (2x, 2y + 1),
//     (2x + 1, 2y + 1) of the 16x16 raster -- two runs of two adjacent records, so a wave's loads cover the CTU's 4 KB of PU records exactly once;
//   * lanes 0..20 load nodes 0..20 in one more load (the other lanes re-read node 20, in bounds, and store nothing for it);
//   * all loads of a round are issued before the first is waited for; a record leaves as one 16-byte store where the output is 16-byte aligned, as four
//     dwords otherwise; inputs are read as 8-byte pairs where both arrays are 8-byte aligned, as dwords otherwise.
// Which lane and which address is read depends on lane and node numbers alone -- never on what the records hold.  The three bit costs and the geometry are
// kernel arguments: two launches with different QPs never share state.
#include "../../include/fasthevc.h"
#include "fhevc_internal.h"
#include <cstddef>

namespace {

constexpr uint32_t kMark = 0xFFFFFFFFu, kSat = 0xFFFFFFFEu;

struct IntraPGeom {
  int width, height, ctus_x;   // the whole picture
  int row_begin, band_ctus;    // the band: first CTU row, CTUs per picture in it
  int total;                   // num_pictures * band_ctus
};

// satd and mode of a first-pass record
template <bool WIDE> __device__ __forceinline__ uint2 load_pair(const uint32_t* rec)
{
  if (WIDE) return *reinterpret_cast<const uint2*>(rec);
  return make_uint2(rec[0], rec[1]);
}

template <bool WIDE> __device__ __forceinline__ void store_node(uint32_t* dst, uint32_t satd, uint32_t cost, uint32_t modes, uint32_t part)
{
  if (WIDE) *reinterpret_cast<uint4*>(dst) = make_uint4(satd, cost, modes, part);
  else { dst[0] = satd; dst[1] = cost; dst[2] = modes; dst[3] = part; }
}

__device__ __forceinline__ uint32_t saturated(uint64_t v) { return v > kSat ? kSat : (uint32_t)v; }

// WIDE_IN: both input arrays are 8-byte aligned; WIDE_OUT: the output is 16-byte aligned; NXN: the 4x4 records are given
template <bool WIDE_IN, bool WIDE_OUT, bool NXN>
__global__ __launch_bounds__(256) void fhevc_intra_p_kernel(IntraPGeom G, FhevcIntraBitCost C, const uint32_t* __restrict__ first, const uint32_t* __restrict__ first4,
                                                            uint32_t* __restrict__ out)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = (lane & 7) * 8, y = (lane >> 3) * 8;   // this lane's 8x8 node
  // the node `lane` of levels 0..2 (lanes 0..20): its corner and size
  const int up_level = lane < 1 ? 0 : (lane < 5 ? 1 : 2), up_size = 64 >> up_level;
  const int up_idx = lane < 1 ? 0 : (lane < 5 ? lane - 1 : min(lane, 20) - 5);
  const int up_x = (up_idx & ((1 << up_level) - 1)) * up_size, up_y = (up_idx >> up_level) * up_size;
  // the first of this lane's four PUs in the 16x16 raster
  const int pu0 = (lane >> 3) * 32 + (lane & 7) * 2;

  for (int g = blockIdx.x * 4 + wave; g < G.total; g += gridDim.x * 4) {
    const int in_band = g % G.band_ctus;
    const int ctu = G.row_begin * G.ctus_x + in_band;
    const int x0 = (ctu % G.ctus_x) * 64, y0 = (ctu / G.ctus_x) * 64;
    const int valid_w = min(64, G.width - x0), valid_h = min(64, G.height - y0);
    const uint32_t* src = first + (size_t)g * (FHEVC_NODES * 4);
    const uint2 leaf = load_pair<WIDE_IN>(src + 4 * (21 + lane)), upper = load_pair<WIDE_IN>(src + 4 * min(lane, 20));
    uint2 p0 = make_uint2(kMark, 0u), p1 = p0, p2 = p0, p3 = p0;
    if constexpr (NXN) {
      const uint32_t* src4 = first4 + (size_t)g * (FHEVC_PUS4_PER_CTU * 4) + 4 * pu0;
      p0 = load_pair<WIDE_IN>(src4); p1 = load_pair<WIDE_IN>(src4 + 4);
      p2 = load_pair<WIDE_IN>(src4 + 64); p3 = load_pair<WIDE_IN>(src4 + 68);
    }
    uint32_t* dst = out + (size_t)g * (FHEVC_NODES * 4);

    // ---- the 8x8 node: 2Nx2N, then NxN where it is strictly cheaper or the only one ----
    const bool inside8 = x + 8 <= valid_w && y + 8 <= valid_h;
    const uint32_t m = leaf.y & 255u;
    bool have = inside8 && leaf.x != kMark;
    uint32_t satd = leaf.x, cost = fhevc_intra_p_price(leaf.x, m, C), modes = m * 0x01010101u, part = 0u;
    if constexpr (NXN) {
      const uint32_t m0 = p0.y & 255u, m1 = p1.y & 255u, m2 = p2.y & 255u, m3 = p3.y & 255u;
      const bool have4 = inside8 && p0.x != kMark && p1.x != kMark && p2.x != kMark && p3.x != kMark;
      const uint32_t cost4 = saturated((uint64_t)fhevc_intra_p_price(p0.x, m0, C) + fhevc_intra_p_price(p1.x, m1, C) + fhevc_intra_p_price(p2.x, m2, C) +
                                       fhevc_intra_p_price(p3.x, m3, C));
      if (have4 && (!have || cost4 < cost)) {
        have = true; part = 1u; cost = cost4;
        satd = saturated((uint64_t)p0.x + p1.x + p2.x + p3.x);
        modes = m0 | m1 << 8 | m2 << 16 | m3 << 24;
      }
    }
    if (!have) { satd = cost = modes = kMark; part = 0u; }
    store_node<WIDE_OUT>(dst + 4 * (21 + lane), satd, cost, modes, part);

    // ---- node `lane` of levels 0..2 ----
    if (lane < 21) {
      const bool inside = up_x + up_size <= valid_w && up_y + up_size <= valid_h;
      const uint32_t um = upper.y & 255u;
      if (inside && upper.x != kMark) store_node<WIDE_OUT>(dst + 4 * lane, upper.x, fhevc_intra_p_price(upper.x, um, C), um * 0x01010101u, 0u);
      else store_node<WIDE_OUT>(dst + 4 * lane, kMark, kMark, kMark, 0u);
    }
  }
}

template <bool WIDE_IN, bool WIDE_OUT>
void launch(bool nxn, dim3 blocks, hipStream_t stream, const IntraPGeom& G, const FhevcIntraBitCost& cost, const uint32_t* first, const uint32_t* first4, uint32_t* out)
{
  if (nxn) hipLaunchKernelGGL((fhevc_intra_p_kernel<WIDE_IN, WIDE_OUT, true>), blocks, dim3(256), 0, stream, G, cost, first, first4, out);
  else hipLaunchKernelGGL((fhevc_intra_p_kernel<WIDE_IN, WIDE_OUT, false>), blocks, dim3(256), 0, stream, G, cost, first, first4, out);
}

}  // namespace

hipError_t fhevc_launch_intra_p(const FhevcFrames& fr, const FhevcIntraBitCost& cost, const uint32_t* d_first, const uint32_t* d_first4, FhevcIntraPNode* d_out,
                                int num_cus, hipStream_t stream)
{
  static_assert(sizeof(FhevcNodeCost) == 16 && offsetof(FhevcNodeCost, satd) == 0 && offsetof(FhevcNodeCost, mode) == 4, "first-pass record layout");
  static_assert(offsetof(FhevcIntraPNode, satd_best) == 0 && offsetof(FhevcIntraPNode, cost_best) == 4 && offsetof(FhevcIntraPNode, modes) == 8 &&
                offsetof(FhevcIntraPNode, part) == 12 && offsetof(FhevcIntraPNode, pad) == 13, "intra record layout");
  if (!d_first || !d_out) return hipErrorInvalidValue;
  IntraPGeom G;
  G.width = fr.width; G.height = fr.height; G.ctus_x = fr.ctus_x;
  G.row_begin = fr.row_begin; G.band_ctus = (fr.row_end - fr.row_begin) * fr.ctus_x;
  const long long total = (long long)G.band_ctus * fr.num_frames;
  if (total <= 0) return hipSuccess;
  if (total > 0x7FFFFFFF) return hipErrorInvalidValue;
  G.total = (int)total;
  long long grid = (total + 3) / 4;
  const long long cap = (long long)num_cus * 8;
  if (grid > cap) grid = cap;
  const bool wide_in = (((uintptr_t)d_first | (uintptr_t)d_first4) & 7) == 0, wide_out = ((uintptr_t)d_out & 15) == 0;
  uint32_t* out = reinterpret_cast<uint32_t*>(d_out);
  const dim3 blocks((unsigned)grid);
  if (wide_in && wide_out) launch<true, true>(d_first4 != nullptr, blocks, stream, G, cost, d_first, d_first4, out);
  else if (wide_in) launch<true, false>(d_first4 != nullptr, blocks, stream, G, cost, d_first, d_first4, out);
  else if (wide_out) launch<false, true>(d_first4 != nullptr, blocks, stream, G, cost, d_first, d_first4, out);
  else launch<false, false>(d_first4 != nullptr, blocks, stream, G, cost, d_first, d_first4, out);
  return hipGetLastError();
}
