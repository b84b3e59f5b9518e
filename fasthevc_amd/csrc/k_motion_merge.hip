// k_motion_merge.hip -- source-only merge-candidate costs per CU node (config 4: P slices), gfx950 only.
//
// Twin of TEncSearch::xMergeEstimation (TEncSearch.cpp:2831-2884) on the candidate list of TComDataCU::getInterMergeCandidates (TComDataCU.cpp:2142-2320),
// spec in include/fasthevc.h: for every CU node (85 per CTU) the vectors its five spatial neighbours of the SAME level were refined to -- L, A, AR, BL, AL
// in HM's order with HM's four pruning pairs, AL only below four entries, then one zero vector --, each priced as the Hadamard distortion of the whole node at
// that quarter-sample vector (TComRdCost::xGetHADs: the node's 8x8 tile Hadamards, (sum + 2) >> 2 each, the node's sum >> (bit depth - 8) once) plus
// getCost(bits of the merge index): 1, 2, 3, 4, 4.  Strict "<", the first entry of equal cost wins.  The prediction is k_motion_refine.hip's: HEVC's 8-tap
// interpolation of the PREVIOUS ORIGINAL picture in the one arithmetic form, coordinates clamped to the picture.
//
// Mapping: k_refine_tile.h's, as in k_motion_refine.hip -- workgroup (4 waves) = one CTU at a time, grid-stride; wave = level, lane = one 8x8 tile
// (RefineNode); the reference window in LDS (MR = 8 layout: static; MR = 64 layout: dynamic), of which only the part max_range reaches is staged;
// refine_tile_at, the node's sum by lane butterflies (refine_node_sum).  Where that kernel walks 18 table candidates this one walks the node's list
// (MergeList): at most five entries, the loop is wave-uniform and stops at the wave's longest list; a lane whose list is shorter evaluates the zero vector
// and drops the result.
// Every lane builds ITS node's list from ten dword loads (cost_best and the vector dword of the five neighbours' refined records); which of them are issued
// and where they point depends on geometry and band alone, never on a record's content, and they are issued before the window staging is waited for.  A
// neighbour's vector is used only if both components lie within 4 max_range + 3 quarter samples -- the reach of a refined vector -- so no input byte can
// send a read outside the staged window.  Neighbour CTUs are oc - 1 and oc - ctus_x + {-1, 0, 1} of the same picture and band.
// No scratch, no HBM state between calls: the bit costs travel by value.
#include "fhevc_internal.h"
#include "k_had8x8.h"
#include "k_refine_tile.h"

namespace {

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
  const int total = SearchWork::total(F);  // frame f >= 1 is predicted from frame f - 1
  const int shift = F.bit_depth - 8;
  const RefineArith arith(F.bit_depth);
  const T* plane = reinterpret_cast<const T*>(F.luma);
  if (tid < 8) s_cost[tid] = cost.c[tid];
  if (tid < 16) s_taps[tid] = kLumaTaps[tid];
  const RefineNode N(lvl, tx, ty);  // this lane's node: level lvl, (nbx, nby) in the CTU
  const int ncnt = N.ncnt;
  const unsigned zme = merge_z((unsigned)N.nbx, (unsigned)N.nby);
  const int gw = F.width >> (6 - lvl), gh = F.height >> (6 - lvl);   // the level's nodes that lie wholly inside the picture: gx < gw && gy < gh
  const int reach = vec_reach(max_range);

  for (int work = blockIdx.x; work < total; work += gridDim.x) {
    const SearchWork W(F, work);
    const int f = W.f, cy = W.cy, cx = W.cx;
    const long long oc = W.oc(F);
    // ---- the five neighbours' records: L, A, AR, BL, AL -- addresses from geometry and band alone, loads issued before the staging ----
    const int gx = cx * ncnt + N.nbx, gy = cy * ncnt + N.nby;
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
        const long long rec = (((long long)((f - 1) * band_rows + (ncy - F.row_begin)) * F.ctus_x + ncx) * FHEVC_NODES + N.first + oby * ncnt + obx) * 4;
        ncost[j] = refined[rec + 2]; nvec[j] = refined[rec + 3];
      }
      av[j] = ok;
    }
    // ---- stage the part of the reference window that max_range reaches ----
    __syncthreads();  // the previous CTU's readers are done
    refine_stage_window_reach<T, MR>(s_ref, plane, W.ref_base, F, cx, cy, tid, max_range);
    // ---- this lane's original 8x8 tile (all four waves hold the same 64 tiles) ----
    const int px = cx * 64 + tx * 8, py = cy * 64 + ty * 8;
    const bool inside = (px + 8 <= F.width) && (py + 8 <= F.height);
    unsigned O[32];
    load_tile8x8(plane, W.cur_base, F, px, py, inside, O);
    // ---- the node's list: a neighbour counts if it was refined and its vector is within reach ----
#pragma unroll
    for (int j = 0; j < 5; ++j) av[j] = av[j] && ncost[j] != kMergeMark && vec_in_reach(nvec[j], reach);
    const MergeList list(av, nvec, node_in);
    const int longest = list.longest();
    __syncthreads();

    MergeBest best;
#pragma unroll 1
    for (int i = 0; i < longest; ++i) {
      unsigned qv;
      int src;
      list.pick(i, qv, src);
      unsigned t8;
      {
        unsigned D[32];
        int v[64];
        refine_tile_at<PACKED, RP>(s_ref, s_taps, arith, tx, ty, vec_x(qv), vec_y(qv), O, D, v);
        t8 = refine_had8x8<PACKED>(D, v, inside);
      }
      const unsigned sd = refine_node_sum(t8, lvl) >> shift;
      best.offer(i, list.num, sd + merge_index_cost(s_cost, i), sd, qv, src);
    }
    if (N.writer) out[oc * FHEVC_NODES + N.nidx] = best.record(list.num);
  }
}

}  // namespace

// four workgroups per CU at MR = 8, as the square refinement's instance; at MR = 64 the LDS holds two windows per CU at most
hipError_t fhevc_launch_motion_merge(const FhevcFrames& fr, int max_range, const FhevcMvBitCost& cost, const FhevcMotionQpelNode* d_refined, FhevcMotionMergeNode* d_out,
                                     int num_cus, hipStream_t stream)
{
  static_assert(sizeof(FhevcMotionQpelNode) == 16 && sizeof(FhevcMotionMergeNode) == 16, "record layouts");
  const unsigned* refined = reinterpret_cast<const unsigned*>(d_refined);
  return refine_launch<FHEVC_MOTION_WIDE_MAX_RANGE>(fr, true, max_range, num_cus, {4, false}, {2, true}, stream, [&](auto t, auto packed, auto mr, const RefineLaunch& L) {
    return refine_launch_kernel<&fhevc_motion_merge_kernel<decltype(t), decltype(packed)::value, decltype(mr)::value>>(L, fr, max_range, cost, refined, d_out);
  });
}
