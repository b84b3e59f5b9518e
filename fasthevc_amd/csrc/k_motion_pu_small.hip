// k_motion_pu_small.hip -- source-only integer motion search of the PUs with a 4-sample side: the AMP shapes of the 16x16 CUs (16x4, 16x12, 4x16,
// 12x16) and the 2NxN / Nx2N PUs of the 8x8 CUs (8x4, 4x8), gfx950 only.
//
// What k_motion_pu.hip delivers for the 124 PUs whose sides are multiples of 8, for the 384 that are left (layout: fhevc_motion_pu_small_index of
// fasthevc.h): full search over [-R, R]^2 in the PREVIOUS ORIGINAL picture, raster order and strict "<", SAD or Hadamard SATD, the vector cost of
// getCostOfVectorWithPredictor with a zero predictor, reference samples outside the picture replicated from the border.  TComRdCost::xGetHADs
// tiles a block by 8x8 only if BOTH sides are multiples of 8; every other block goes WHOLLY through xCalcHADs4x4 (TComRdCost.cpp:1771-1803).  So
// these PUs are not sums of the 8x8 tile distortions of the other two kernels: a 16x12 PU is twelve 4x4 Hadamards, each with its own
// (sum + 1) >> 1, and the block's sum is shifted ONCE by bit_depth - 8.  SAD is additive and shifted once as well.
//
// Mapping: k_search_tile.h, at MR = 8.  Own to this kernel: per tile and vector the lane computes the four QUADRANT distortions q00 q01 / q10 q11
// (4x4 SAD or 4x4 Hadamard) on that header's displaced rows and packed differences, and the lanes are
// numbered so that the four tiles of a 16x16 node sit on one lane quad (lane = node * 4 + ty1 * 2 + tx1), which makes the node's reduction three
// DPP quad permutes and no LDS:
//   the tile's own PUs      8x4 top = q00 + q01    8x4 bottom = q10 + q11    4x8 left = q00 + q10    4x8 right = q01 + q11
//   the node's AMP PUs      quarter strip = the two tiles' halves on that side; three-quarter part = the node's sixteen quadrants minus the strip
// Lane p of the quad keeps one AMP shape of its node, the one whose quarter strip passes through its tile and its neighbour's in ONE permute:
//   p = 0: 2NxnU (top strip, + lane 1's top)      p = 1: nRx2N (right strip, + lane 3's right)
//   p = 2: nLx2N (left strip, + lane 0's left)    p = 3: 2NxnD (bottom strip, + lane 2's bottom)
// so every lane keeps six running (cost, vector index) pairs, all of entries it alone owns; the distortion at the best vector is cost - vector cost.
//
// MR = 64 (fhevc_launch_motion_pu_small_big; SAD only, behind fhevc_motion_search_pu_wide): the same kernel laid out for HM's own SearchRange, as
// k_motion_pu.hip's -- the window in dynamic LDS, the vector cost from the bits of the components and the 40 bit costs of the launch.
#include "fhevc_internal.h"
#include "k_search_tile.h"

namespace {

constexpr int SLOTS = 6;                       // per lane: 8x4 top, 8x4 bottom, 4x8 left, 4x8 right of its tile; part 0 and part 1 of its AMP shape
constexpr int ENTRIES = FHEVC_PUS_SMALL;
constexpr int AMP_ENTRIES = 128;               // 16 nodes x 4 shapes x 2 parts, then 64 tiles x 2 shapes x 2 parts

// lane (i & ~3) | P_(i & 3) of the same quad (DPP quad_perm: a VALU operand modifier, no LDS); every lane of the wave is active where this is used
template <int P0, int P1, int P2, int P3>
__device__ __forceinline__ unsigned quad(unsigned v)
{
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, P0 | (P1 << 2) | (P2 << 4) | (P3 << 6), 0xF, 0xF, false);
}

// the vector costs of a launch: the window's own table at MR = 8, the cost of every number of bits at MR = 64 (by value either way)
template <int MR> using SearchCosts = typename std::conditional<(MR > FHEVC_MOTION_MAX_RANGE), FhevcMvBitCost, FhevcMvCost>::type;

// T = int16_t (HM Pel planes) or uint8_t; PACKED = bit depth <= 10; SAD: as fhevc_motion_kernel; MR: the largest range the layout holds (8 or 64)
// CENTRED (fhevc_motion_search_pu_centred; MR = 8, SAD): the window of every CTU lies around that CTU's entry of `centres` (k_search_tile.h: SearchCentre)
template <typename T, bool PACKED, bool SAD, int MR = FHEVC_MOTION_MAX_RANGE, bool CENTRED = false>
__global__ __launch_bounds__(256, (MR > FHEVC_MOTION_MAX_RANGE ? 1 : PACKED ? 4 : 3)) void fhevc_motion_pu_small_kernel(FhevcFrames F, int range, SearchCosts<MR> mvc,
                                                                                                         FhevcMotionNode* __restrict__ out_pus, SearchCentres<CENTRED> centres)
{
  using Geom = SearchGeom<MR>;
  constexpr int RP = Geom::RP;
  constexpr bool BIG = MR > FHEVC_MOTION_MAX_RANGE;
  extern __shared__ __attribute__((aligned(16))) short s_dyn[];
  __shared__ __attribute__((aligned(16))) short s_small[BIG ? 8 : Geom::REF_SAMPLES];
  short* const s_ref = BIG ? s_dyn : s_small;
  __shared__ unsigned s_cost[4][ENTRIES], s_idx[4][ENTRIES], s_zero[ENTRIES], s_vc[BIG ? FHEVC_MV_BIT_COSTS : Geom::NMV_MAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int quad_pos = lane & 3, node16 = lane >> 2;  // the tile's place in its 16x16 node (bit 0: right, bit 1: lower), the node (raster 4x4)
  const int tx = (node16 & 3) * 2 + (quad_pos & 1), ty = (node16 >> 2) * 2 + (quad_pos >> 1);
  // this lane's six entries: four of its tile (8x8 node 21 + ty * 8 + tx), two of its node's AMP shape (0: 2NxnU, 1: 2NxnD, 2: nLx2N, 3: nRx2N)
  const int amp_shape = quad_pos == 0 ? 0 : quad_pos == 1 ? 3 : quad_pos == 2 ? 2 : 1;
  const int e_tile = AMP_ENTRIES + (ty * 8 + tx) * 4, e_amp = node16 * 8 + amp_shape * 2;
  const bool strip_is_part0 = (quad_pos & 1) == 0;  // 2NxnU and nLx2N: the quarter strip comes first
  SearchRange R(range);
  const int total = SearchWork::total(F), nmv = R.nmv, centre = R.centre;
  const int shift = F.bit_depth - 8;
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
        for (int e = tid; e < ENTRIES; e += 256) *reinterpret_cast<uint4*>(out_pus + W.oc(F) * ENTRIES + e) = search_record_outside();
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
      unsigned q[4] = { 0, 0, 0, 0 };  // q00 q01 / q10 q11
      if (PACKED && SAD) {  // sum |org - ref| on pairs of unsigned 16-bit samples: v_sad_u16
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const SearchRefRow w = search_ref_row<RP>(s_ref, row0 + j, col);
#pragma unroll
          for (int k = 0; k < 4; ++k) q[(j >> 2) * 2 + (k >> 1)] = __builtin_amdgcn_sad_u16(O[4 * j + k], w.pair(k), q[(j >> 2) * 2 + (k >> 1)]);
        }
      } else if (PACKED) {
        unsigned D[32];
        search_tile_diff<RP>(s_ref, row0, col, O, D);
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = had4x4_packed(D, (k >> 1) * 4, (k & 1) * 2);
      } else {
        int v[64];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const SearchRefRow w = search_ref_row<RP>(s_ref, row0 + j, col);  // whole dwords from LDS, as the packed forms read them
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const unsigned p = w.pair(k);
            v[8 * j + 2 * k] = (int)(short)(O[4 * j + k] & 0xFFFFu) - (int)(short)(p & 0xFFFFu);
            v[8 * j + 2 * k + 1] = (int)(short)(O[4 * j + k] >> 16) - (int)(short)(p >> 16);
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (SAD) {
#pragma unroll
            for (int y = 0; y < 4; ++y)
#pragma unroll
              for (int x = 0; x < 4; ++x) q[k] += (unsigned)abs(v[8 * ((k >> 1) * 4 + y) + (k & 1) * 4 + x]);
          } else q[k] = had4x4_wide(v, (k >> 1) * 4, (k & 1) * 4);
        }
      }
      // ---- the tile's four PUs, then the node's AMP shape this lane keeps (quad_pos = lane bits 0..1) ----
      unsigned d[SLOTS];
      const unsigned top = inside ? q[0] + q[1] : 0u, bottom = inside ? q[2] + q[3] : 0u;
      const unsigned left = inside ? q[0] + q[2] : 0u, right = inside ? q[1] + q[3] : 0u;
      d[0] = top; d[1] = bottom; d[2] = left; d[3] = right;
      const unsigned t8 = top + bottom;
      const unsigned h = t8 + quad<1, 0, 3, 2>(t8);
      const unsigned s16 = h + quad<2, 3, 0, 1>(h);  // the node's sixteen quadrants
      // each lane hands the half its partner's strip needs: 0 <- 1: top, 1 <- 3: right, 2 <- 0: left, 3 <- 2: bottom
      const unsigned give = quad_pos == 1 ? top : quad_pos == 3 ? right : quad_pos == 0 ? left : bottom;
      const unsigned own = quad_pos == 0 ? top : quad_pos == 1 ? right : quad_pos == 2 ? left : bottom;
      const unsigned strip = own + quad<1, 3, 0, 2>(give);
      d[4] = strip_is_part0 ? strip : s16 - strip;
      d[5] = s16 - d[4];
      unsigned vc;
      if constexpr (BIG) vc = s_vc[search_vector_bits(m, R)];
      else {
        vc = mvc.c[m];
        if (lane == 0) s_vc[m] = vc;  // the merge looks the winner's vector cost up by a per-thread index (every m is one wave's)
      }
#pragma unroll
      for (int k = 0; k < SLOTS; ++k) {
        const unsigned c = (d[k] >> shift) + vc;  // DISTORTION_PRECISION_ADJUSTMENT on the block's sum, once (TComRdCost.cpp:1823)
        if (c < bc[k]) { bc[k] = c; bi[k] = (unsigned)m; }
      }
      if (m == centre) {  // uniform: one wave, once per CTU
#pragma unroll
        for (int k = 0; k < SLOTS; ++k) s_zero[k < 4 ? e_tile + k : e_amp + k - 4] = d[k] >> shift;
      }
    }
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) {
      const int e = k < 4 ? e_tile + k : e_amp + k - 4;
      s_cost[wave][e] = bc[k]; s_idx[wave][e] = bi[k];
    }
    __syncthreads();
    for (int e = tid; e < ENTRIES; e += 256) {
      // the CU node this entry belongs to: a PU is valid iff its node lies wholly inside the picture
      const int n = e < AMP_ENTRIES ? 16 : 8, cnt = 64 / n;
      const int ni = e < AMP_ENTRIES ? e >> 3 : (e - AMP_ENTRIES) >> 2;
      uint4 o = search_record_outside();
      if (search_node_inside(F, cx, cy, ni % cnt, ni / cnt, n)) {
        unsigned c, ix;
        search_merge(&s_cost[0][0], &s_idx[0][0], ENTRIES, e, c, ix);
        o = search_record(s_zero[e], c, s_vc[BIG ? search_vector_bits((int)ix, R) : (int)ix], ix, R);
        if constexpr (CENTRED) o = P.absolute(o);
      }
      *reinterpret_cast<uint4*>(out_pus + W.oc(F) * ENTRIES + e) = o;  // one 16-byte store per entry
    }
  }
}

}  // namespace

// Resources (hipcc -Rpass-analysis=kernel-resource-usage): 29 076 B of LDS per workgroup (window 14 096 B, merge 13 824 B, vector costs
// 1 156 B), no scratch; the packed forms take 95 (SAD) and 117 (SATD) VGPRs and are held to four waves per SIMD (four workgroups per CU, 116 KB of
// its LDS), the 32-bit forms 150 and 130 (three workgroups per CU).  The persistent grid is sized to exactly that residency
hipError_t fhevc_launch_motion_pu_small(const FhevcFrames& fr, int range, const FhevcMvCost& mvc, FhevcMotionNode* d_pus, int num_cus, bool sad, hipStream_t stream)
{
  return search_launch(fr, range >= 1 && range <= FHEVC_MOTION_MAX_RANGE && d_pus, num_cus, 4, 3, sad, [&](auto t, auto packed, auto sad_c, int grid) {
    hipLaunchKernelGGL((fhevc_motion_pu_small_kernel<decltype(t), decltype(packed)::value, decltype(sad_c)::value>), dim3(grid), dim3(256), 0, stream, fr, range, mvc, d_pus, SearchNoCentres{});
    return hipSuccess;
  });
}

// the same layout and residency around one centre per CTU (SAD; the window's table prices d, the vector relative to the centre)
hipError_t fhevc_launch_motion_pu_small_centred(const FhevcFrames& fr, int range, const FhevcMvCost& mvc, const FhevcMotionNode* d_centres, FhevcMotionNode* d_pus, int num_cus,
                                                hipStream_t stream)
{
  return search_launch(fr, range >= 1 && range <= FHEVC_MOTION_MAX_RANGE && d_centres && d_pus, num_cus, 4, 3, true, [&](auto t, auto packed, auto sad_c, int grid) {
    if constexpr (decltype(sad_c)::value) {
      hipLaunchKernelGGL((fhevc_motion_pu_small_kernel<decltype(t), decltype(packed)::value, true, FHEVC_MOTION_MAX_RANGE, true>), dim3(grid), dim3(256), 0, stream, fr, range, mvc, d_pus,
                         d_centres);
      return hipSuccess;
    } else return hipErrorInvalidValue;
  });
}

// search ranges up to 64 in the SAD mode, any bit depth: the MR = 64 layout (window 76 816 B + merge 13 824 B of LDS: one workgroup per CU)
hipError_t fhevc_launch_motion_pu_small_big(const FhevcFrames& fr, int range, const FhevcMvBitCost& cost, FhevcMotionNode* d_pus, int num_cus, hipStream_t stream)
{
  constexpr int MRB = FHEVC_MOTION_WIDE_MAX_RANGE;
  const size_t lds = (size_t)SearchGeom<MRB>::REF_SAMPLES * sizeof(short);
  return search_launch(fr, range >= 1 && range <= MRB && d_pus, num_cus, 1, 1, true, [&](auto t, auto packed, auto sad_c, int grid) {
    if constexpr (decltype(sad_c)::value) {
      const auto kernel = &fhevc_motion_pu_small_kernel<decltype(t), decltype(packed)::value, true, MRB>;
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds, stream, fr, range, cost, d_pus, SearchNoCentres{});
      return hipSuccess;
    } else return hipErrorInvalidValue;
  });
}
