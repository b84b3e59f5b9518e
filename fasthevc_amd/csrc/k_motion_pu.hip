// k_motion_pu.hip -- source-only integer motion search of the rectangular PUs (2NxN, Nx2N and the four AMP shapes), gfx950 only.
//
// What k_motion.hip delivers for the 85 square CU nodes of a CTU, for the 124 PUs of HM's partitioned CUs whose sides are multiples of 8
// (TComDataCU::getPartIndexAndSize; layout: fhevc_motion_pu_index of fasthevc.h): full search over [-R, R]^2 in the PREVIOUS ORIGINAL picture,
// raster order and strict "<" (TEncSearch::xPatternSearch), SAD or Hadamard SATD, the vector cost of getCostOfVectorWithPredictor with a zero
// predictor, reference samples outside the picture replicated from the border.  TComRdCost::xGetHADs tiles any block whose sides are multiples
// of 8 into 8x8 Hadamards and SAD is additive, so the per-vector 8x8 tile distortions of k_motion.hip give every such rectangle exactly: the
// sum of its tiles, shifted ONCE by bit_depth - 8.
//
// Mapping: k_search_tile.h, at MR = 8 (lane = ty * 8 + tx).  Own to this kernel is the reduction.  The butterfly to 16x16 / 32x32 / 64x64 already
// passes through the symmetric halves:
//   t8 + xor 1 = 16x8     t8 + xor 8 = 8x16     s16 + xor 2 = 32x16     s16 + xor 16 = 16x32     s32 + xor 4 = 64x32     s32 + xor 32 = 32x64
// the AMP quarter strips are one more step on those (16x8 + xor 2 = 32x8, 8x16 + xor 16 = 8x32, 32x16 + xor 4 = 64x16, 16x32 + xor 32 = 16x64),
// fetched from the node's first / last strip by a lane broadcast (32x32 nodes: ds_swizzle; the 64x64 node: v_readlane), and the three-quarter
// part is the node's sum minus the quarter.  Every lane keeps the running best (cost, vector index) of the PU that CONTAINS ITS TILE, for each
// of its 14 shapes, next to the four squares; the distortion at the best vector is cost - vector cost, so it has no register of its own.
// When d_nodes is given the 85 square nodes are written too, byte for byte what fhevc_motion_kernel writes.
//
// MR = 64 (fhevc_launch_motion_pu_big; SAD only, behind fhevc_motion_search_pu_wide): the same kernel laid out for HM's own SearchRange, as
// fhevc_motion_kernel<.., 64> of k_motion.hip is -- the window in 76.8 KB of dynamic LDS, and no table of (2 R + 1)^2 vector costs anywhere: the cost of
// a vector comes from the bits of its components (search_vector_bits) and the 40 bit costs that travel with the launch, so nothing is kept between
// calls.  Which of the two families (the 85 nodes, the 124 PUs) a launch delivers is a template argument there (FAM): the slots of a family that is
// not asked for do not exist.
#include "fhevc_internal.h"
#include "k_search_tile.h"

namespace {

constexpr int SLOTS = 18;                      // per lane: 4 squares, 6 shapes of the 64x64 node, 6 of its 32x32 node, 2 of its 16x16 node
constexpr int ENTRIES = FHEVC_NODES + FHEVC_PUS;  // per CTU in the merge arrays: the nodes, then the PUs in output order

// lane j = ((i & AND) | OR) ^ XOR inside each half of the wave (ds_swizzle, bit-mask mode): no address register, no LDS traffic
template <int AND, int OR, int XOR>
__device__ __forceinline__ unsigned swz(unsigned v) { return (unsigned)__builtin_amdgcn_ds_swizzle((int)v, AND | (OR << 5) | (XOR << 10)); }
template <int M> __device__ __forceinline__ unsigned sx(unsigned v) { return swz<0x1F, 0, M>(v); }

// node of the 85 at level l (0: 64x64 .. 3: 8x8) that holds tile (tx, ty)
__device__ __forceinline__ int node_of(int l, int tx, int ty)
{
  return l == 0 ? 0 : l == 1 ? 1 + (ty >> 2) * 2 + (tx >> 2) : l == 2 ? 5 + (ty >> 1) * 4 + (tx >> 1) : 21 + ty * 8 + tx;
}
// the entry of the merge arrays that slot `slot` of the lane at tile (tx, ty) belongs to; rep: this lane is the PU's (node's) first tile
__device__ __forceinline__ int slot_entry(int slot, int tx, int ty, bool& rep)
{
  if (slot < 4) {
    const int tn = 8 >> slot;
    rep = ((tx | ty) & (tn - 1)) == 0;
    return node_of(slot, tx, ty);
  }
  const int L = slot < 10 ? 0 : slot < 16 ? 1 : 2, s = slot - (slot < 10 ? 4 : slot < 16 ? 10 : 16);
  const int tn = 8 >> L, lx = tx & (tn - 1), ly = ty & (tn - 1);
  const int sp = s < 2 ? tn / 2 : (s & 1) ? 3 * tn / 4 : tn / 4;  // where the CU is cut, in tiles
  const bool horiz = s == 0 || s == 2 || s == 3;                  // cut by a horizontal line: part 0 on top
  const int along = horiz ? ly : lx, other = horiz ? lx : ly;
  const int part = along >= sp ? 1 : 0;
  rep = other == 0 && along == part * sp;
  const int k = node_of(L, tx, ty);
  return FHEVC_NODES + (L < 2 ? k * 12 : 60 + (k - 5) * 4) + s * 2 + part;
}

// the vector costs of a launch: the window's own table at MR = 8, the cost of every number of bits at MR = 64 (by value either way)
template <int MR> using SearchCosts = typename std::conditional<(MR > FHEVC_MOTION_MAX_RANGE), FhevcMvBitCost, FhevcMvCost>::type;

// T = int16_t (HM Pel planes) or uint8_t; PACKED = bit depth <= 10; SAD: as fhevc_motion_kernel; MR: the largest range the layout holds (8 or 64);
// FAM: 0 = the 124 PUs, and the 85 nodes where out_nodes is given (MR = 8); otherwise the families of this instantiation, 1 = nodes | 2 = PUs
// CENTRED (fhevc_motion_search_pu_centred; MR = 8, SAD): the window of every CTU lies around that CTU's entry of `centres` (k_search_tile.h: SearchCentre)
template <typename T, bool PACKED, bool SAD, int MR = FHEVC_MOTION_MAX_RANGE, int FAM = 0, bool CENTRED = false>
__global__ __launch_bounds__(256, (MR > FHEVC_MOTION_MAX_RANGE ? 1 : PACKED ? 3 : 2)) void fhevc_motion_pu_kernel(FhevcFrames F, int range, SearchCosts<MR> mvc,
                                                             FhevcMotionNode* __restrict__ out_nodes, FhevcMotionNode* __restrict__ out_pus,
                                                             SearchCentres<CENTRED> centres)
{
  using Geom = SearchGeom<MR>;
  constexpr int RP = Geom::RP;
  constexpr bool BIG = MR > FHEVC_MOTION_MAX_RANGE;
  extern __shared__ __attribute__((aligned(16))) short s_dyn[];
  __shared__ __attribute__((aligned(16))) short s_small[BIG ? 8 : Geom::REF_SAMPLES];
  short* const s_ref = BIG ? s_dyn : s_small;
  __shared__ unsigned s_cost[4][ENTRIES], s_idx[4][ENTRIES], s_zero[ENTRIES], s_vc[BIG ? FHEVC_MV_BIT_COSTS : Geom::NMV_MAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx = lane & 7, ty = lane >> 3;
  SearchRange R(range);
  const int total = SearchWork::total(F), nmv = R.nmv, centre = R.centre;
  const int shift = F.bit_depth - 8;
  const bool want_nodes = FAM ? (FAM & 1) != 0 : out_nodes != nullptr;
  constexpr bool want_pus = FAM == 0 || (FAM & 2) != 0;
  const T* plane = reinterpret_cast<const T*>(F.luma);
  if constexpr (BIG) {
    if (tid < FHEVC_MV_BIT_COSTS) s_vc[tid] = mvc.c[tid];  // visible behind the first barrier of the CTU loop
  }

  for (int work = blockIdx.x; work < total; work += gridDim.x) {
    const SearchWork W(F, work);
    const int cx = W.cx, cy = W.cy;
    SearchCentre P;
    if constexpr (CENTRED) {
      P = SearchCentre(centres, W.oc(F));
      if (!P.in_range()) {  // uniform: every entry of this CTU gets the marker, nothing is read for it
        if (tid < ENTRIES && (tid < FHEVC_NODES ? want_nodes : want_pus))
          *reinterpret_cast<uint4*>(tid < FHEVC_NODES ? out_nodes + W.oc(F) * FHEVC_NODES + tid : out_pus + W.oc(F) * FHEVC_PUS + (tid - FHEVC_NODES)) = search_record_outside();
        continue;
      }
      R.centre_on(P.x);
    }
    __syncthreads();  // the previous CTU's readers are done
    if constexpr (CENTRED) search_stage_window<T, RP>(s_ref, plane, W.ref_base, F, cx, cy, R, tid, P.x, P.y);
    else search_stage_window<T, RP>(s_ref, plane, W.ref_base, F, cx, cy, R, tid);
    // ---- this lane's original 8x8 tile (all four waves hold the same 64 tiles) ----
    const int px = cx * 64 + tx * 8, py = cy * 64 + ty * 8;
    const bool inside = (px + 8 <= F.width) && (py + 8 <= F.height);
    unsigned O[32];
    load_tile8x8(plane, W.cur_base, F, px, py, inside, O);
    __syncthreads();

    unsigned bc[SLOTS], bi[SLOTS];
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) { bc[k] = 0xFFFFFFFFu; bi[k] = 0; }
    for (int m = wave; m < nmv; m += 4) {  // raster order inside a wave; the waves interleave and are merged by (cost, index)
      int col, row0;
      R.at(m, tx, ty, col, row0);
      const unsigned t8 = search_tile8x8<PACKED, SAD, RP>(s_ref, row0, col, O, inside);

      // ---- the sums of every square and rectangle that holds this lane's tile (tx = lane bits 0..2, ty = bits 3..5) ----
      unsigned d[SLOTS];
      const unsigned h16x8 = t8 + sx<1>(t8), v8x16 = t8 + sx<8>(t8);
      const unsigned s16 = h16x8 + sx<8>(h16x8);
      const unsigned h32x16 = s16 + sx<2>(s16), v16x32 = s16 + sx<16>(s16);
      const unsigned s32 = h32x16 + sx<16>(h32x16);
      const unsigned h64x32 = s32 + sx<4>(s32), v32x64 = s32 + __shfl_xor(s32, 32);
      const unsigned s64 = h64x32 + __shfl_xor(h64x32, 32);
      const unsigned h32x8 = h16x8 + sx<2>(h16x8), v8x32 = v8x16 + sx<16>(v8x16);         // quarter strips of the 32x32 node, per tile row / column
      const unsigned h64x16 = h32x16 + sx<4>(h32x16), v16x64 = v16x32 + __shfl_xor(v16x32, 32);  // ... of the 64x64 node, per pair of rows / columns
      d[0] = s64; d[1] = s32; d[2] = s16; d[3] = t8;
      {  // the 64x64 node: its first and last strips are wave-uniform
        const unsigned top = __builtin_amdgcn_readlane(h64x16, 0), bottom = __builtin_amdgcn_readlane(h64x16, 63);
        const unsigned left = __builtin_amdgcn_readlane(v16x64, 0), right = __builtin_amdgcn_readlane(v16x64, 63);
        d[4] = h64x32; d[5] = v32x64;
        d[6] = ty < 2 ? top : s64 - top;      d[7] = ty >= 6 ? bottom : s64 - bottom;
        d[8] = tx < 2 ? left : s64 - left;    d[9] = tx >= 6 ? right : s64 - right;
      }
      {  // the lane's 32x32 node: row 0 / row 3 (ty bits 0, 1 cleared / set), column 0 / column 3 (tx bits 0, 1)
        const unsigned top = swz<0x07, 0, 0>(h32x8), bottom = swz<0x1F, 0x18, 0>(h32x8);
        const unsigned left = swz<0x1C, 0, 0>(v8x32), right = swz<0x1F, 0x03, 0>(v8x32);
        d[10] = h32x16; d[11] = v16x32;
        d[12] = (ty & 3) == 0 ? top : s32 - top;     d[13] = (ty & 3) == 3 ? bottom : s32 - bottom;
        d[14] = (tx & 3) == 0 ? left : s32 - left;   d[15] = (tx & 3) == 3 ? right : s32 - right;
      }
      d[16] = h16x8; d[17] = v8x16;
      unsigned vc;
      if constexpr (BIG) vc = s_vc[search_vector_bits(m, R)];
      else {
        vc = mvc.c[m];
        if (lane == 0) s_vc[m] = vc;  // the merge looks the winner's vector cost up by a per-thread index (every m is one wave's)
      }
#pragma unroll
      for (int k = 0; k < SLOTS; ++k) {
        if (k < 4 ? !want_nodes : !want_pus) continue;
        const unsigned c = (d[k] >> shift) + vc;  // DISTORTION_PRECISION_ADJUSTMENT on the block's sum, once (TComRdCost.cpp:1823)
        if (c < bc[k]) { bc[k] = c; bi[k] = (unsigned)m; }
      }
      if (m == centre) {  // uniform: one wave, once per CTU
        int txo = tx, tyo = ty;
        asm volatile("" : "+v"(txo), "+v"(tyo));  // the 18 entries are worked out HERE, not hoisted out of the loops into 36 registers
#pragma unroll
        for (int k = 0; k < SLOTS; ++k) {
          bool rep;
          const int e = slot_entry(k, txo, tyo, rep);
          if (FAM && (k < 4 ? !want_nodes : !want_pus)) continue;
          if (rep) s_zero[e] = d[k] >> shift;
        }
      }
    }
    int txo = tx, tyo = ty;
    asm volatile("" : "+v"(txo), "+v"(tyo));  // as above
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) {
      bool rep;
      const int e = slot_entry(k, txo, tyo, rep);
      if (FAM && (k < 4 ? !want_nodes : !want_pus)) continue;
      if (rep) { s_cost[wave][e] = bc[k]; s_idx[wave][e] = bi[k]; }
    }
    __syncthreads();
    if (tid < ENTRIES && (tid < FHEVC_NODES ? want_nodes : want_pus)) {
      // the CU node this entry belongs to: a PU is valid iff its node lies wholly inside the picture
      const int p = tid - FHEVC_NODES;
      const int node = p < 0 ? tid : p < 60 ? p / 12 : 5 + (p - 60) / 4;
      int l, ni;
      search_node_level(node, l, ni);
      const int n = 64 >> l, cnt = 1 << l;
      uint4 o = search_record_outside();
      if (search_node_inside(F, cx, cy, ni % cnt, ni / cnt, n)) {
        unsigned c, ix;
        search_merge(&s_cost[0][0], &s_idx[0][0], ENTRIES, tid, c, ix);
        o = search_record(s_zero[tid], c, s_vc[BIG ? search_vector_bits((int)ix, R) : (int)ix], ix, R);
        if constexpr (CENTRED) o = P.absolute(o);
      }
      FhevcMotionNode* dst = p < 0 ? out_nodes + W.oc(F) * FHEVC_NODES + tid : out_pus + W.oc(F) * FHEVC_PUS + p;
      *reinterpret_cast<uint4*>(dst) = o;  // one 16-byte store per entry
    }
  }
}

}  // namespace

// Resources (hipcc -Rpass-analysis=kernel-resource-usage): 22 788 B of LDS per workgroup (window 14 096 B, merge 7 524 B, vector costs
// 1 156 B), no scratch; the packed forms are held to 168 VGPRs (three waves per SIMD: three workgroups per CU, 68 KB of its LDS), the 32-bit forms
// to 256 (two workgroups per CU).  The persistent grid is sized to exactly that residency
hipError_t fhevc_launch_motion_pu(const FhevcFrames& fr, int range, const FhevcMvCost& mvc, FhevcMotionNode* d_nodes, FhevcMotionNode* d_pus, int num_cus, bool sad,
                                  hipStream_t stream)
{
  return search_launch(fr, range >= 1 && range <= FHEVC_MOTION_MAX_RANGE && d_pus, num_cus, 3, 2, sad, [&](auto t, auto packed, auto sad_c, int grid) {
    hipLaunchKernelGGL((fhevc_motion_pu_kernel<decltype(t), decltype(packed)::value, decltype(sad_c)::value>), dim3(grid), dim3(256), 0, stream, fr, range, mvc, d_nodes, d_pus, SearchNoCentres{});
    return hipSuccess;
  });
}

// the same layout and residency around one centre per CTU (SAD; the window's table prices d, the vector relative to the centre): the families asked for are
// instantiated (FAM), so a call for the nodes alone runs this kernel too -- its nodes are byte for byte fhevc_motion_kernel's
hipError_t fhevc_launch_motion_pu_centred(const FhevcFrames& fr, int range, const FhevcMvCost& mvc, const FhevcMotionNode* d_centres, FhevcMotionNode* d_nodes,
                                          FhevcMotionNode* d_pus, int num_cus, hipStream_t stream)
{
  return search_launch(fr, range >= 1 && range <= FHEVC_MOTION_MAX_RANGE && d_centres && (d_nodes || d_pus), num_cus, 3, 2, true, [&](auto t, auto packed, auto sad_c, int grid) {
    if constexpr (decltype(sad_c)::value) {
      using T = decltype(t);
      constexpr bool P = decltype(packed)::value;
      if (d_nodes && d_pus) hipLaunchKernelGGL((fhevc_motion_pu_kernel<T, P, true, FHEVC_MOTION_MAX_RANGE, 3, true>), dim3(grid), dim3(256), 0, stream, fr, range, mvc, d_nodes, d_pus, d_centres);
      else if (d_pus) hipLaunchKernelGGL((fhevc_motion_pu_kernel<T, P, true, FHEVC_MOTION_MAX_RANGE, 2, true>), dim3(grid), dim3(256), 0, stream, fr, range, mvc, d_nodes, d_pus, d_centres);
      else hipLaunchKernelGGL((fhevc_motion_pu_kernel<T, P, true, FHEVC_MOTION_MAX_RANGE, 1, true>), dim3(grid), dim3(256), 0, stream, fr, range, mvc, d_nodes, d_pus, d_centres);
      return hipSuccess;
    } else return hipErrorInvalidValue;
  });
}

// search ranges up to 64 in the SAD mode (HM's integer-search distortion), any bit depth: the MR = 64 layout.  The window (76 816 B) and the merge
// arrays are more than half of a CU's 160 KB of LDS: one workgroup per CU.  Either output may be null, not both
hipError_t fhevc_launch_motion_pu_big(const FhevcFrames& fr, int range, const FhevcMvBitCost& cost, FhevcMotionNode* d_nodes, FhevcMotionNode* d_pus, int num_cus,
                                      hipStream_t stream)
{
  constexpr int MRB = FHEVC_MOTION_WIDE_MAX_RANGE;
  const size_t lds = (size_t)SearchGeom<MRB>::REF_SAMPLES * sizeof(short);
  return search_launch(fr, range >= 1 && range <= MRB && (d_nodes || d_pus), num_cus, 1, 1, true, [&](auto t, auto packed, auto sad_c, int grid) {
    if constexpr (decltype(sad_c)::value) {
      auto go = [&](auto kernel) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds, stream, fr, range, cost, d_nodes, d_pus, SearchNoCentres{});
        return hipSuccess;
      };
      using T = decltype(t);
      constexpr bool P = decltype(packed)::value;
      if (d_nodes && d_pus) return go(&fhevc_motion_pu_kernel<T, P, true, MRB, 3>);
      return d_pus ? go(&fhevc_motion_pu_kernel<T, P, true, MRB, 2>) : go(&fhevc_motion_pu_kernel<T, P, true, MRB, 1>);
    } else return hipErrorInvalidValue;
  });
}
