// k_motion.hip -- source-only integer motion search per CU node (config 4: P slices), gfx950 only.
//
// Bit-exact twin of oracle/fhevc_oracle.c: fho_motion_ctu_dist.  For every CU node (64x64, 32x32, 16x16, 8x8: 85 per CTU) of a
// picture: full search over [-R, R]^2 integer vectors in the PREVIOUS ORIGINAL picture, cost = distortion + vector cost, raster
// order over the window and strict "<" as TEncSearch::xPatternSearch (TEncSearch.cpp:3786-3848), vector cost as
// TComRdCost::getCostOfVectorWithPredictor (TComRdCost.h:166-174; the host tabulates it with HM's double arithmetic),
// reference samples outside the picture replicated from the border (TComPicYuv::extendPicBorder, TComPicYuv.cpp:229-270).
// Two distortions (template argument SAD):
//   SAD  -- what HM's integer search uses: xPatternSearch's setDistParam selects DF_SAD (TComRdCost.cpp:205-236, xGetSAD* :518-..).
//           In this mode the kernel reproduces the reference's own xPatternSearch bit for bit (vector, SAD, cost): the oracle is pinned
//           to tests/golden/ref_pattern_search.npz, the kernel to the oracle.  One v_sad_u16 per pair of samples.
//   SATD -- TComRdCost::xGetHADs (TComRdCost.cpp:1753-1824) at integer positions.  HM applies Hadamard to the FRACTIONAL refinement
//           only (HadamardME, TEncSearch.cpp:836; cfg/encoder_lowdelay_P_main.cfg:37): at integer positions it is this build's own
//           choice (the P-picture rule's features are fitted on it), the default of fhevc_motion_search.
// Either distortion of a node is the sum of its 8x8 tiles' (both shift the block's sum once), so ONE pass over the 64 tiles of a
// CTU per vector serves all four levels.
//
// Mapping: k_search_tile.h (workgroup = CTU, lane = 8x8 tile, the window in LDS, the waves split the vectors).  Own to this kernel: per vector the
// tile distortions meet through lane shuffles, a butterfly to the four levels (packed-16 Hadamard: k_had8x8.h), and the MR = 64 layout below.
#include "fhevc_internal.h"
#include "k_search_tile.h"

namespace {

// MR = the largest search range an instantiation is laid out for: FHEVC_MOTION_MAX_RANGE (8: the window in 15 KB of static LDS, the vector costs in the
// kernel arguments) or FHEVC_MOTION_WIDE_MAX_RANGE (64, round 4: HM's own SearchRange for content ABOVE 8 bit, where k_motion_wide.hip's byte SADs do
// not apply -- the window in 76.8 KB of dynamic LDS, the (2 R + 1)^2 vector costs in HBM).  Same code, same raster order, same first-found minimum.
// T = int16_t (HM Pel planes) or uint8_t; PACKED = bit depth <= 10; SAD: see the header
template <typename T, bool PACKED, bool SAD, int MR>
__global__ __launch_bounds__(256) void fhevc_motion_kernel(FhevcFrames F, int range, FhevcMvCost mvc, const uint32_t* __restrict__ mvtab, FhevcMotionNode* __restrict__ out)
{
  constexpr int RP = SearchGeom<MR>::RP;
  constexpr bool BIG = MR > FHEVC_MOTION_MAX_RANGE;
  extern __shared__ __attribute__((aligned(16))) short s_dyn[];
  __shared__ __attribute__((aligned(16))) short s_small[BIG ? 8 : SearchGeom<MR>::REF_SAMPLES];
  short* const s_ref = BIG ? s_dyn : s_small;
  __shared__ unsigned s_cost[4][4][64], s_satd[4][4][64], s_idx[4][4][64], s_zero[4][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx = lane & 7, ty = lane >> 3;
  const SearchRange R(range);
  const int total = SearchWork::total(F), nmv = R.nmv, centre = R.centre;
  const int shift = F.bit_depth - 8;
  const T* plane = reinterpret_cast<const T*>(F.luma);

  for (int work = blockIdx.x; work < total; work += gridDim.x) {
    const SearchWork W(F, work);
    const int cx = W.cx, cy = W.cy;
    __syncthreads();  // the previous CTU's readers are done
    search_stage_window<T, RP>(s_ref, plane, W.ref_base, F, cx, cy, R, tid);
    // ---- this lane's original 8x8 tile (all four waves hold the same 64 tiles) ----
    const int px = cx * 64 + tx * 8, py = cy * 64 + ty * 8;
    const bool inside = (px + 8 <= F.width) && (py + 8 <= F.height);
    unsigned O[32];
    load_tile8x8(plane, W.cur_base, F, px, py, inside, O);
    __syncthreads();

    unsigned bc[4], bs[4], bi[4];
#pragma unroll
    for (int l = 0; l < 4; ++l) { bc[l] = 0xFFFFFFFFu; bs[l] = 0; bi[l] = 0; }
    unsigned z[4] = { 0, 0, 0, 0 };
    for (int m = wave; m < nmv; m += 4) {  // raster order inside a wave; the waves interleave and are merged by (cost, index)
      int col, row0;
      R.at(m, tx, ty, col, row0);
      const unsigned t8 = search_tile8x8<PACKED, SAD, RP>(s_ref, row0, col, O, inside);
      // node sums: 16x16 = tiles (tx ^ 1, ty ^ 1), 32x32 = + bits 1, 64x64 = + bits 2
      unsigned s[4];
      s[3] = t8;
      unsigned a = t8 + __shfl_xor(t8, 1);
      s[2] = a + __shfl_xor(a, 8);
      a = s[2] + __shfl_xor(s[2], 2);
      s[1] = a + __shfl_xor(a, 16);
      a = s[1] + __shfl_xor(s[1], 4);
      s[0] = a + __shfl_xor(a, 32);
      const unsigned vc = BIG ? mvtab[m] : mvc.c[m];
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        const unsigned sd = s[l] >> shift;  // DISTORTION_PRECISION_ADJUSTMENT on the block's sum (TComRdCost.cpp:1823)
        const unsigned c = sd + vc;
        if (m == centre) z[l] = sd;
        if (c < bc[l]) { bc[l] = c; bs[l] = sd; bi[l] = (unsigned)m; }
      }
    }
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      s_cost[wave][l][lane] = bc[l]; s_satd[wave][l][lane] = bs[l]; s_idx[wave][l][lane] = bi[l];
      if ((centre & 3) == wave) s_zero[l][lane] = z[l];
    }
    __syncthreads();
    if (tid < FHEVC_NODES) {
      int l, ni;
      search_node_level(tid, l, ni);
      const int n = 64 >> l, cnt = 1 << l, tn = n >> 3;
      const int bx = ni % cnt, by = ni / cnt;
      const int rep = (by * tn) * 8 + bx * tn;  // a lane of the node (all of them hold the node's sums)
      FhevcMotionNode o;
      if (!search_node_inside(F, cx, cy, bx, by, n)) {
        o.satd_zero = o.satd_best = o.cost_best = 0xFFFFFFFFu; o.mvx = 0; o.mvy = 0;
      } else {
        unsigned c, ix;
        const int w = search_merge(&s_cost[0][0][0], &s_idx[0][0][0], 4 * 64, l * 64 + rep, c, ix);
        o.satd_zero = s_zero[l][rep]; o.satd_best = s_satd[w][l][rep]; o.cost_best = c;
        o.mvx = (short)((int)(ix % R.side) - range); o.mvy = (short)((int)(ix / R.side) - range);
      }
      out[W.oc(F) * FHEVC_NODES + tid] = o;
    }
  }
}

}  // namespace

hipError_t fhevc_launch_motion(const FhevcFrames& fr, int range, const FhevcMvCost& mvc, FhevcMotionNode* d_out, int num_cus, bool sad, hipStream_t stream)
{
  return search_launch(fr, true, num_cus, 4, 4, sad, [&](auto t, auto packed, auto sad_c, int grid) {
    hipLaunchKernelGGL((fhevc_motion_kernel<decltype(t), decltype(packed)::value, decltype(sad_c)::value, FHEVC_MOTION_MAX_RANGE>), dim3(grid), dim3(256), 0, stream, fr, range, mvc, nullptr, d_out);
    return hipSuccess;
  });
}

// ranges 9 .. 64 on 16-bit planes above 8 bit (SAD, HM's integer-search distortion): the same kernel laid out for a window of up to 192 x 192 samples
hipError_t fhevc_launch_motion_big(const FhevcFrames& fr, int range, const uint32_t* d_mvtab, FhevcMotionNode* d_out, int num_cus, hipStream_t stream)
{
  constexpr int MRB = FHEVC_MOTION_WIDE_MAX_RANGE;
  const size_t lds = (size_t)SearchGeom<MRB>::REF_SAMPLES * sizeof(short);   // 76 816 B: two workgroups per CU
  return search_launch(fr, fr.sample_bytes == 2 && range <= MRB, num_cus, 2, 2, true, [&](auto t, auto packed, auto sad_c, int grid) {
    if constexpr (sizeof(t) == 2 && decltype(sad_c)::value) {
      const auto kernel = &fhevc_motion_kernel<int16_t, decltype(packed)::value, true, MRB>;
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds, stream, fr, range, FhevcMvCost{}, d_mvtab, d_out);
      return hipSuccess;
    } else return hipErrorInvalidValue;
  });
}
