// k_motion_merge.hip -- source-only merge-candidate costs per CU node (config 4: P slices), gfx950 only.
//
// Twin of TEncSearch::xMergeEstimation (TEncSearch.cpp:2831-2884) on the candidate list of TComDataCU::getInterMergeCandidates (TComDataCU.cpp:2142-2320),
// spec in include/fasthevc.h: for every CU node (85 per CTU) the vectors its five spatial neighbours of the SAME level were refined to -- L, A, AR, BL, AL
// in HM's order with HM's four pruning pairs, AL only below four entries, then one zero vector --, each priced as the Hadamard distortion of the whole node at
// that quarter-sample vector (TComRdCost::xGetHADs: the node's 8x8 tile Hadamards, (sum + 2) >> 2 each, the node's sum >> (bit depth - 8) once) plus
// getCost(bits of the merge index): 1, 2, 3, 4, 4.  Strict "<", the first entry of equal cost wins.  The prediction is k_motion_refine.hip's: HEVC's 8-tap
// interpolation of the PREVIOUS ORIGINAL picture in the one arithmetic form, coordinates clamped to the picture.
//
// Mapping: that of k_motion_refine.hip -- workgroup (4 waves) = one CTU at a time, grid-stride; wave = level, lane = one 8x8 tile; the reference window of
// k_refine_tile.h in LDS (MR = 8 layout: static; MR = 64 layout: dynamic), of which only the part max_range reaches is staged; refine_tile_diff, the Hadamard
// of k_had8x8.h, the node's sum by lane butterflies.  Where that kernel walks 18 table candidates this one walks the node's list: at most five entries, the
// loop is wave-uniform and stops at the wave's longest list; a lane whose list is shorter evaluates the zero vector and drops the result.
// Every lane builds ITS node's list from ten dword loads (cost_best and the vector dword of the five neighbours' refined records); which of them are issued
// and where they point depends on geometry and band alone, never on a record's content, and they are issued before the window staging is waited for.  A
// neighbour's vector is used only if both components lie within 4 max_range + 3 quarter samples -- the reach of a refined vector -- so no input byte can
// send a read outside the staged window.  Neighbour CTUs are oc - 1 and oc - ctus_x + {-1, 0, 1} of the same picture and band.
// No scratch, no HBM state between calls: the bit costs travel by value.
#include "fhevc_internal.h"
#include "k_had8x8.h"
#include "k_refine_tile.h"
#include <atomic>

namespace {

constexpr unsigned kMergeMark = 0xFFFFFFFFu;

// z-scan index of (x, y) in a level's grid of up to 8 x 8 nodes: the bit interleave, x in the even bits
__device__ __forceinline__ unsigned merge_z(unsigned x, unsigned y)
{
  const unsigned sx = (x & 1u) | ((x & 2u) << 1) | ((x & 4u) << 2), sy = (y & 1u) | ((y & 2u) << 1) | ((y & 4u) << 2);
  return sx | (sy << 1);
}

// T = int16_t or uint8_t planes; PACKED = bit depth <= 10; MR = 8 or 64: the largest max_range the window is laid out for
template <typename T, bool PACKED, int MR>
__global__ __launch_bounds__(256) void fhevc_motion_merge_kernel(FhevcFrames F, int max_range, FhevcMvBitCost cost, const unsigned* __restrict__ refined,
                                                                 FhevcMotionMergeNode* __restrict__ out)
{
  constexpr int RP = RefineGeom<MR>::RP;
  constexpr bool BIG = MR > FHEVC_MOTION_MAX_RANGE;
  extern __shared__ __attribute__((aligned(16))) short s_dyn[];
  __shared__ __attribute__((aligned(16))) short s_small[BIG ? 8 : RefineGeom<MR>::SAMPLES];
  short* const s_ref = BIG ? s_dyn : s_small;
  __shared__ unsigned s_cost[8], s_taps[16];
  const int tid = threadIdx.x, lane = tid & 63, lvl = tid >> 6;
  const int tx = lane & 7, ty = lane >> 3;
  const int band_rows = F.row_end - F.row_begin;
  const int per_frame = band_rows * F.ctus_x;
  const int total = per_frame * (F.num_frames - 1);  // frame f >= 1 is predicted from frame f - 1
  const int shift = F.bit_depth - 8;
  const RefineArith arith(F.bit_depth);
  const T* plane = reinterpret_cast<const T*>(F.luma);
  if (tid < 8) s_cost[tid] = cost.c[tid];
  if (tid < 16) s_taps[tid] = kLumaTaps[tid];
  // this lane's node: level lvl, (nbx, nby) in the CTU
  const int ncnt = 1 << lvl;
  const int nbx = tx >> (3 - lvl), nby = ty >> (3 - lvl);
  const int first = ((1 << (2 * lvl)) - 1) / 3;
  const int nidx = first + nby * ncnt + nbx;
  const bool writer = (tx & ((8 >> lvl) - 1)) == 0 && (ty & ((8 >> lvl) - 1)) == 0;
  const unsigned zme = merge_z((unsigned)nbx, (unsigned)nby);
  const int gw = F.width >> (6 - lvl), gh = F.height >> (6 - lvl);   // the level's nodes that lie wholly inside the picture: gx < gw && gy < gh
  const int reach = 4 * max_range + 3;

  for (int work = blockIdx.x; work < total; work += gridDim.x) {
    const int f = 1 + work / per_frame;
    const int rem = work % per_frame;
    const int cy = F.row_begin + rem / F.ctus_x, cx = rem % F.ctus_x;
    const long long cur_base = (long long)f * F.frame_stride, ref_base = (long long)(f - 1) * F.frame_stride;
    const long long oc = (long long)((f - 1) * band_rows + (cy - F.row_begin)) * F.ctus_x + cx;
    // ---- the five neighbours' records: L, A, AR, BL, AL -- addresses from geometry and band alone, loads issued before the staging ----
    const int gx = cx * ncnt + nbx, gy = cy * ncnt + nby;
    const bool node_in = gx < gw && gy < gh;
    const unsigned key = ((unsigned)(cy * F.ctus_x + cx) << 6) | zme;
    unsigned ncost[5], nvec[5];
    bool av[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int dx = j == 1 ? 0 : (j == 2 ? 1 : -1), dy = j == 0 ? 0 : (j == 3 ? 1 : -1);
      const int ngx = gx + dx, ngy = gy + dy;
      const int ncx = ngx >> lvl, ncy = ngy >> lvl, obx = ngx & (ncnt - 1), oby = ngy & (ncnt - 1);
      bool ok = node_in && ngx >= 0 && ngy >= 0 && ngx < gw && ngy < gh && ncy >= F.row_begin && ncy < F.row_end;
      ok = ok && ((((unsigned)(ncy * F.ctus_x + ncx) << 6) | merge_z((unsigned)obx, (unsigned)oby)) < key);   // coding order
      ncost[j] = kMergeMark; nvec[j] = 0;
      if (ok) {
        const long long rec = (((long long)((f - 1) * band_rows + (ncy - F.row_begin)) * F.ctus_x + ncx) * FHEVC_NODES + first + oby * ncnt + obx) * 4;
        ncost[j] = refined[rec + 2]; nvec[j] = refined[rec + 3];
      }
      av[j] = ok;
    }
    // ---- stage the part of the reference window that max_range reaches ----
    __syncthreads();  // the previous CTU's readers are done
    refine_stage_window_reach<T, MR>(s_ref, plane, ref_base, F, cx, cy, tid, max_range);
    // ---- this lane's original 8x8 tile (all four waves hold the same 64 tiles) ----
    const int px = cx * 64 + tx * 8, py = cy * 64 + ty * 8;
    const bool inside = (px + 8 <= F.width) && (py + 8 <= F.height);
    unsigned O[32];
    load_tile8x8(plane, cur_base, F, px, py, inside, O);
    // ---- the node's list: availability, HM's pruning pairs, positions ----
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int vx = (int)(short)(nvec[j] & 0xFFFFu), vy = (int)(short)(nvec[j] >> 16);
      av[j] = av[j] && ncost[j] != kMergeMark && abs(vx) <= reach && abs(vy) <= reach;
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
    for (int n = 2; n <= 5; ++n)
      if (__builtin_amdgcn_ballot_w64(num >= n) != 0) longest = n;   // wave-uniform
    __syncthreads();

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
      const int fx = qx & 3, fy = qy & 3;
      const int col = tx * 8 + MR + 4 + (qx >> 2) - 3, row0 = ty * 8 + MR + 4 + (qy >> 2) - 3;  // first tap of sample (0, 0)
      unsigned t8;
      {
        unsigned D[32];
        int v[64];
        refine_tile_diff<PACKED, RP>(s_ref, s_taps, arith, col, row0, fx, fy, O, D, v);
        if constexpr (PACKED) t8 = had8x8_packed(D);
        else t8 = had8x8_wide(v);
      }
      t8 = inside ? ((t8 + 2) >> 2) : 0u;  // xCalcHADs8x8: (sum + 2) >> 2
      unsigned s = t8;
      for (int k = 0; k < 3 - lvl; ++k) {
        s += __shfl_xor(s, 1 << k);
        s += __shfl_xor(s, 8 << k);
      }
      const unsigned sd = s >> shift;
      const unsigned c = sd + s_cost[i == 4 ? 4 : i + 1];   // MaxNumMergeCand 5: the last index saves its terminating bit
      if (i < num && c < best_c) { best_c = c; best_s = sd; best_v = qv; best_i = i; best_src = src; }
    }
    if (writer) {
      FhevcMotionMergeNode o;
      o.satd_best = best_s; o.cost_best = best_c;
      o.mvx = (short)(best_v & 0xFFFFu); o.mvy = (short)(best_v >> 16);
      o.idx = (uint8_t)best_i; o.num = (uint8_t)num; o.src = (uint8_t)best_src; o.pad = 0;
      out[oc * FHEVC_NODES + nidx] = o;
    }
  }
}

// the MR = 64 instance of one (T, PACKED) form: its dynamic LDS, and how many of its workgroups the device keeps on one CU (asked once per instance)
template <typename T, bool PACKED> struct MergeBig {
  static constexpr int MRB = FHEVC_MOTION_WIDE_MAX_RANGE;
  static constexpr size_t LDS = (size_t)RefineGeom<MRB>::SAMPLES * sizeof(short);  // 80 016 B
  static hipError_t resident(int* per_cu)
  {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&fhevc_motion_merge_kernel<T, PACKED, MRB>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS);
    if (e != hipSuccess) return e;
    static std::atomic<int> asked{0};   // every device of a context is a gfx950: one answer per instance
    int n = asked.load(std::memory_order_relaxed);
    if (n == 0) {
      const hipError_t q = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fhevc_motion_merge_kernel<T, PACKED, MRB>, 256, LDS);
      if (q != hipSuccess) return q;
      asked.store(n, std::memory_order_relaxed);
    }
    *per_cu = n;
    return hipSuccess;
  }
};

template <typename T, bool PACKED>
hipError_t launch_merge(const FhevcFrames& fr, int max_range, const FhevcMvBitCost& cost, const unsigned* refined, FhevcMotionMergeNode* d_out, int num_cus, long long total,
                        hipStream_t stream)
{
  if (max_range <= FHEVC_MOTION_MAX_RANGE) {
    const int grid = (int)(total < 4LL * num_cus ? total : 4LL * num_cus);   // as the square refinement's MR = 8 instance
    hipLaunchKernelGGL((fhevc_motion_merge_kernel<T, PACKED, FHEVC_MOTION_MAX_RANGE>), dim3(grid), dim3(256), 0, stream, fr, max_range, cost, refined, d_out);
  } else {
    using Big = MergeBig<T, PACKED>;
    int per_cu = 0;
    const hipError_t e = Big::resident(&per_cu);
    if (e != hipSuccess) return e;
    if (per_cu < 1) return hipErrorLaunchOutOfResources;
    const long long resident = (long long)(per_cu < 2 ? per_cu : 2) * num_cus;   // the LDS holds two windows per CU at most
    const int grid = (int)(total < resident ? total : resident);
    hipLaunchKernelGGL((fhevc_motion_merge_kernel<T, PACKED, Big::MRB>), dim3(grid), dim3(256), Big::LDS, stream, fr, max_range, cost, refined, d_out);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t fhevc_launch_motion_merge(const FhevcFrames& fr, int max_range, const FhevcMvBitCost& cost, const FhevcMotionQpelNode* d_refined, FhevcMotionMergeNode* d_out,
                                     int num_cus, hipStream_t stream)
{
  static_assert(sizeof(FhevcMotionQpelNode) == 16 && sizeof(FhevcMotionMergeNode) == 16, "record layouts");
  const long long total = (long long)(fr.row_end - fr.row_begin) * fr.ctus_x * (fr.num_frames - 1);
  if (total <= 0) return hipSuccess;
  if (max_range < 1 || max_range > FHEVC_MOTION_WIDE_MAX_RANGE || total > 0x7FFFFFFF) return hipErrorInvalidValue;
  const unsigned* refined = reinterpret_cast<const unsigned*>(d_refined);
  if (fr.sample_bytes == 2 && fr.bit_depth <= 10) return launch_merge<int16_t, true>(fr, max_range, cost, refined, d_out, num_cus, total, stream);
  if (fr.sample_bytes == 2) return launch_merge<int16_t, false>(fr, max_range, cost, refined, d_out, num_cus, total, stream);
  return launch_merge<uint8_t, true>(fr, max_range, cost, refined, d_out, num_cus, total, stream);
}
