// k_motion_skip.hip -- the zero-residual (skip) test per CU node (config 4: P slices), gfx950 only.
//
// Spec in include/fasthevc.h: for every CU node (85 per CTU) the residual of the prediction at the vector its merge record holds -- k_motion_refine.hip's
// prediction: HEVC's 8-tap interpolation of the PREVIOUS ORIGINAL picture in the one arithmetic form, coordinates clamped --, HM's forward DCT of it
// (xTrMxN, TComTrQuant.cpp:860-915: TUs of min(node, 32) samples, shifts log2 N + bit depth - 9 and log2 N + 6 with partialButterfly's rounding) and HM's
// scalar quantiser without scaling lists (TComTrQuant.cpp:1186-1232) under the two offsets: the P-slice dead zone and RDOQ's starting levels.
//
// Mapping: k_refine_tile.h's -- workgroup (4 waves) = one CTU at a time over a persistent grid; the reference window in LDS (MR = 8 layout: static;
// MR = 64 layout: dynamic), of which only the part max_range reaches is staged; wave = level and lane = one 8x8 tile (RefineNode) for the prediction: ONE
// refine_tile_diff per lane, at its node's vector.  The residual fits 16 bits at every bit depth (|r| <= 4095), so the packed form of
// refine_tile_diff serves 12 bit too: there is no PACKED parameter.
// The transform goes through LDS.  Once all four waves hold their residual tiles the window is dead: behind a barrier four buffers of 64 rows x 72 shorts
// (one per level; 9 216 B each, a pitch of 36 dwords so that a wave's 64 rows start in different banks) lie OVER it.  Both passes are the same loop: a
// thread holds one row segment of N shorts as N / 2 packed pairs and makes v_dot2_i32_i16 products with rows of the matrix, which lies behind the buffers
// (2 048 B, copied there with the residuals: the window covers that place while it lives) and is read at wave-uniform addresses -- LDS broadcasts.
// All four waves share every level: lane = row; 32-point levels: wave = (segment, half of the outputs), 16 outputs of 16 products each; 16-point: wave =
// segment, 16 x 8; 8-point: wave = segments w and w + 4, 2 x 8 x 4 -- 704 products per thread and pass.  The first pass writes its outputs TRANSPOSED inside the TU, as partialButterfly does, in place: every thread has read before a barrier and
// writes behind it, so the second pass reads rows again.  16-bit intermediates are exact: the largest absolute row sum of the matrices is 64 N, so no
// first-stage or second-stage value exceeds 32 760 (tests/test_motion_skip_ref.py computes the bound from the recorded matrices).
// The second pass quantises in registers: max |c|, the sum of levels and the number of non-zero levels per thread, eight lanes (the rows of one 8-point
// TU, a part of every larger one) combined by lane exchanges, then LDS atomics per node.  level = (|c| scale + add) >> qbits fits 32 bits: |c| <= 32 768,
// scale < 2^15, add < 2^26.  The quantiser's numbers per TU size travel by value.  No scratch, no HBM state between calls.
#include "fhevc_internal.h"
#include "k_had8x8.h"
#include "k_refine_tile.h"

namespace {

constexpr unsigned kSkipMark = 0xFFFFFFFFu;
constexpr int kPitch = 72;                       // shorts per row of a transform buffer
constexpr int kLevelBuf = 64 * kPitch;           // shorts per level
constexpr int kTransformShorts = 4 * kLevelBuf;  // 36 864 B
constexpr int kMatrixShorts = 32 * 32;           // the 32-point matrix behind them: 2 048 B
constexpr int kRowsInFlight = 2;                 // matrix rows the scheduler may fetch ahead of their products

// the 32-point matrix of the standard (H.265 8.6.4.2) as packed pairs [k][x / 2], low half = the even column; the 16- and the 8-point matrices are its
// rows 2 k and 4 k, first 16 and 8 columns.  Entry m of kCos is the scaled cos(m pi / 64), entry 0 the DC row's 64
struct DctTable { unsigned p[32][16]; };
constexpr int kCos[32] = { 64, 90, 90, 90, 89, 88, 87, 85, 83, 82, 80, 78, 75, 73, 70, 67, 64, 61, 57, 54, 50, 46, 43, 38, 36, 31, 25, 22, 18, 13, 9, 4 };
constexpr int dct_entry(int k, int x)
{
  int a = ((2 * x + 1) * k) % 128;   // the angle in units of pi / 64
  if (a > 64) a = 128 - a;
  return a > 32 ? -kCos[64 - a] : kCos[a];
}
constexpr DctTable make_dct()
{
  DctTable t{};
  for (int k = 0; k < 32; ++k)
    for (int j = 0; j < 16; ++j) t.p[k][j] = ((unsigned)dct_entry(k, 2 * j) & 0xFFFFu) | ((unsigned)dct_entry(k, 2 * j + 1) << 16);
  return t;
}
__constant__ DctTable kDct = make_dct();

// the row segment of N shorts at buf[row][x0 ..] as N / 2 packed pairs: 16-byte reads (x0 is a multiple of 8, the pitch of 8 too)
template <int N>
__device__ __forceinline__ void load_segment(const short* buf, int row, int x0, unsigned (&x)[N / 2])
{
  const uint4* p = reinterpret_cast<const uint4*>(buf + row * kPitch + x0);
#pragma unroll
  for (int i = 0; i < N / 8; ++i) {
    const uint4 q = p[i];
    x[4 * i] = q.x; x[4 * i + 1] = q.y; x[4 * i + 2] = q.z; x[4 * i + 3] = q.w;
  }
}

// output k (wave-uniform) of the N-point transform of a segment, rounded and shifted as partialButterfly does; mat: the matrix in LDS
template <int N>
__device__ __forceinline__ int dct_output(const short* mat, const unsigned (&x)[N / 2], int k, int shift)
{
  const uint4* m = reinterpret_cast<const uint4*>(mat + k * (32 / N) * 32);
  int a = 1 << (shift - 1);
#pragma unroll
  for (int i = 0; i < N / 8; ++i) {
    const uint4 q = m[i];
    a = dot2(x[4 * i], q.x, a); a = dot2(x[4 * i + 1], q.y, a); a = dot2(x[4 * i + 2], q.z, a); a = dot2(x[4 * i + 3], q.w, a);
  }
  return a >> shift;
}

// first pass: outputs k0 .. k0 + NK - 1 of segment seg of this lane's row
template <int N, int NK>
__device__ __forceinline__ void rows_pass(const short* mat, const short* buf, int row, int seg, int k0, int shift, unsigned (&t)[NK / 2])
{
  unsigned x[N / 2];
  load_segment<N>(buf, row, seg * N, x);
#pragma unroll
  for (int i = 0; i < NK; ++i) {
    const unsigned v = (unsigned)dct_output<N>(mat, x, k0 + i, shift);
    if (i & 1) t[i >> 1] |= v << 16;
    else t[i >> 1] = v & 0xFFFFu;
    if ((i & (kRowsInFlight - 1)) == kRowsInFlight - 1) __builtin_amdgcn_sched_barrier(0);   // or every matrix row of the pass is fetched ahead, into registers
  }
}
// ... written transposed inside the TU: tmp[k][j] of input row j
template <int N, int NK>
__device__ __forceinline__ void rows_store(short* buf, int row, int seg, int k0, const unsigned (&t)[NK / 2])
{
  short* dst = buf + ((row & ~(N - 1)) + k0) * kPitch + seg * N + (row & (N - 1));
#pragma unroll
  for (int i = 0; i < NK; ++i) dst[i * kPitch] = (short)(i & 1 ? t[i >> 1] >> 16 : t[i >> 1] & 0xFFFFu);
}

struct SkipSums { unsigned top, sum, nonzero; };

// second pass: the same outputs of the transposed buffer are the coefficients; quantised under add_plain
template <int N, int NK>
__device__ __forceinline__ void cols_pass(const short* mat, const short* buf, int row, int seg, int k0, int shift, unsigned scale, unsigned qbits, unsigned add, SkipSums& s)
{
  unsigned x[N / 2];
  load_segment<N>(buf, row, seg * N, x);
#pragma unroll
  for (int i = 0; i < NK; ++i) {
    const unsigned a = (unsigned)abs(dct_output<N>(mat, x, k0 + i, shift));
    const unsigned lv = (a * scale + add) >> qbits;
    s.top = max(s.top, a); s.sum += lv; s.nonzero += lv != 0u ? 1u : 0u;
    if ((i & (kRowsInFlight - 1)) == kRowsInFlight - 1) __builtin_amdgcn_sched_barrier(0);
  }
}

// eight neighbouring lanes (rows of one TU) into one, then that lane into the node's sums
__device__ __forceinline__ void skip_commit(unsigned* acc, int node, int lane, SkipSums s)
{
#pragma unroll
  for (int d = 1; d < 8; d <<= 1) {
    s.top = max(s.top, (unsigned)__shfl_xor((int)s.top, d));
    s.sum += (unsigned)__shfl_xor((int)s.sum, d);
    s.nonzero += (unsigned)__shfl_xor((int)s.nonzero, d);
  }
  if ((lane & 7) == 0) {
    atomicMax(&acc[3 * node], s.top);
    atomicAdd(&acc[3 * node + 1], s.sum);
    atomicAdd(&acc[3 * node + 2], s.nonzero);
  }
}

// T = int16_t or uint8_t planes; MR = 8 or 64: the largest max_range the window is laid out for
template <typename T, int MR>
__global__ __launch_bounds__(256) void fhevc_motion_skip_kernel(FhevcFrames F, int max_range, FhevcSkipQuant Q, const unsigned* __restrict__ merge,
                                                                FhevcMotionSkipNode* __restrict__ out)
{
  constexpr int RP = RefineGeom<MR>::RP;
  constexpr bool BIG = MR > FHEVC_MOTION_MAX_RANGE;
  constexpr int OVER = kTransformShorts + kMatrixShorts;                                    // what lies over the dead window
  constexpr int SMALL = RefineGeom<MR>::SAMPLES > OVER ? RefineGeom<MR>::SAMPLES : OVER;   // the larger of the two uses
  static_assert(!BIG || RefineGeom<MR>::SAMPLES >= OVER, "the dynamic window holds the transform buffers and the matrix");
  extern __shared__ __attribute__((aligned(16))) short s_dyn[];
  __shared__ __attribute__((aligned(16))) short s_small[BIG ? 8 : SMALL];
  short* const s_ref = BIG ? s_dyn : s_small;
  __shared__ unsigned s_taps[16], s_acc[3 * FHEVC_NODES];
  const int tid = threadIdx.x, lane = tid & 63, lvl = tid >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(lvl);   // the transform's matrix rows are read at wave-uniform addresses
  const int tx = lane & 7, ty = lane >> 3;
  const int total = SearchWork::total(F);  // frame f >= 1 is predicted from frame f - 1
  const RefineArith arith(F.bit_depth);
  const T* plane = reinterpret_cast<const T*>(F.luma);
  if (tid < 16) s_taps[tid] = kLumaTaps[tid];
  const RefineNode N(lvl, tx, ty);  // this lane's node: level lvl, (nbx, nby) in the CTU
  const int nidx = N.nidx;
  const int gw = F.width >> (6 - lvl), gh = F.height >> (6 - lvl);   // the level's nodes that lie wholly inside the picture
  const int reach = vec_reach(max_range);
  const int s1_8 = F.bit_depth - 6, s1_16 = F.bit_depth - 5, s1_32 = F.bit_depth - 4;   // shift_1st = log2 N + bit depth - 9
  // the transform's work of this thread: its row is its lane
  const int seg32 = wave & 1, k32 = (wave >> 1) * 16;

  for (int work = blockIdx.x; work < total; work += gridDim.x) {
    const SearchWork W(F, work);
    const int cy = W.cy, cx = W.cx;
    const long long oc = W.oc(F);
    // ---- the node's merge record: cost_best (the marker test) and the vector dword; the address depends on geometry alone ----
    const bool node_in = cx * N.ncnt + N.nbx < gw && cy * N.ncnt + N.nby < gh;
    const unsigned mcost = merge[(oc * FHEVC_NODES + nidx) * 4 + 1], mvec = merge[(oc * FHEVC_NODES + nidx) * 4 + 2];
    // ---- stage the part of the reference window that max_range reaches ----
    __syncthreads();  // the previous CTU's readers of the buffers and of the sums are done
    refine_stage_window_reach<T, MR>(s_ref, plane, W.ref_base, F, cx, cy, tid, max_range);
    for (int i = tid; i < 3 * FHEVC_NODES; i += 256) s_acc[i] = 0;
    const int px = cx * 64 + tx * 8, py = cy * 64 + ty * 8;
    const bool inside = (px + 8 <= F.width) && (py + 8 <= F.height);
    unsigned O[32];
    load_tile8x8(plane, W.cur_base, F, px, py, inside, O);
    const int vx = vec_x(mvec), vy = vec_y(mvec);
    const bool valid = node_in && mcost != kSkipMark && vec_in_reach(mvec, reach);
    const int qx = valid ? vx : 0, qy = valid ? vy : 0;   // an invalid node predicts at the zero vector and drops the result: no read outside the window
    __syncthreads();
    // ---- the residual of this lane's tile at its node's vector ----
    unsigned D[32];
    {
      int v[64];
      refine_tile_at<true, RP>(s_ref, s_taps, arith, tx, ty, qx, qy, O, D, v);
    }
    __syncthreads();  // the window is dead: the transform buffers lie over it
    {
      short* dst = s_ref + lvl * kLevelBuf + (ty * 8) * kPitch + tx * 8;
#pragma unroll
      for (int y = 0; y < 8; ++y) *reinterpret_cast<uint4*>(dst + y * kPitch) = make_uint4(D[4 * y], D[4 * y + 1], D[4 * y + 2], D[4 * y + 3]);
      unsigned* mdst = reinterpret_cast<unsigned*>(s_ref + kTransformShorts);
      mdst[tid] = kDct.p[tid >> 4][tid & 15]; mdst[tid + 256] = kDct.p[(tid >> 4) + 16][tid & 15];
    }
    __syncthreads();
    // ---- rows: every thread reads, a barrier, every thread writes ----
    const short* const mat = s_ref + kTransformShorts;
    short *const b0 = s_ref, *const b1 = s_ref + kLevelBuf, *const b2 = s_ref + 2 * kLevelBuf, *const b3 = s_ref + 3 * kLevelBuf;
    {
      // the outputs are kept packed, two to a register, until the barrier
      unsigned t0[8], t1[8], t2[8], t3a[4], t3b[4];
      rows_pass<32, 16>(mat, b0, lane, seg32, k32, s1_32, t0);
      rows_pass<32, 16>(mat, b1, lane, seg32, k32, s1_32, t1);
      rows_pass<16, 16>(mat, b2, lane, wave, 0, s1_16, t2);
      rows_pass<8, 8>(mat, b3, lane, wave, 0, s1_8, t3a);
      rows_pass<8, 8>(mat, b3, lane, wave + 4, 0, s1_8, t3b);
      __syncthreads();
      rows_store<32, 16>(b0, lane, seg32, k32, t0);
      rows_store<32, 16>(b1, lane, seg32, k32, t1);
      rows_store<16, 16>(b2, lane, wave, 0, t2);
      rows_store<8, 8>(b3, lane, wave, 0, t3a);
      rows_store<8, 8>(b3, lane, wave + 4, 0, t3b);
    }
    __syncthreads();
    // ---- columns, quantiser, the nodes' sums ----
    {
      SkipSums s = { 0, 0, 0 };
      cols_pass<32, 16>(mat, b0, lane, seg32, k32, 11, Q.scale, Q.qbits[2], Q.add_plain[2], s);
      skip_commit(s_acc, 0, lane, s);
      s = { 0, 0, 0 };
      cols_pass<32, 16>(mat, b1, lane, seg32, k32, 11, Q.scale, Q.qbits[2], Q.add_plain[2], s);
      skip_commit(s_acc, 1 + (lane >> 5) * 2 + seg32, lane, s);
      s = { 0, 0, 0 };
      cols_pass<16, 16>(mat, b2, lane, wave, 0, 10, Q.scale, Q.qbits[1], Q.add_plain[1], s);
      skip_commit(s_acc, 5 + (lane >> 4) * 4 + wave, lane, s);
      s = { 0, 0, 0 };
      cols_pass<8, 8>(mat, b3, lane, wave, 0, 9, Q.scale, Q.qbits[0], Q.add_plain[0], s);
      skip_commit(s_acc, 21 + (lane >> 3) * 8 + wave, lane, s);
      s = { 0, 0, 0 };
      cols_pass<8, 8>(mat, b3, lane, wave + 4, 0, 9, Q.scale, Q.qbits[0], Q.add_plain[0], s);
      skip_commit(s_acc, 21 + (lane >> 3) * 8 + wave + 4, lane, s);
    }
    __syncthreads();
    if (N.writer) {
      FhevcMotionSkipNode o;
      o.coef_max = o.level_sum = kSkipMark; o.nonzero = 0xFFFFu; o.flags = 0; o.pad = 0; o.mvx = o.mvy = 0;
      if (valid) {
        const int li = lvl == 3 ? 0 : (lvl == 2 ? 1 : 2);
        o.coef_max = s_acc[3 * nidx]; o.level_sum = s_acc[3 * nidx + 1]; o.nonzero = (uint16_t)s_acc[3 * nidx + 2];
        // both levels grow with |c|: the node is zero under an offset iff its largest coefficient is
        const bool zero_plain = ((o.coef_max * Q.scale + Q.add_plain[li]) >> Q.qbits[li]) == 0u, zero_half = ((o.coef_max * Q.scale + Q.add_half[li]) >> Q.qbits[li]) == 0u;
        o.flags = (uint8_t)((zero_plain ? 1 : 0) | (zero_half ? 2 : 0));
        o.mvx = (short)vx; o.mvy = (short)vy;
      }
      out[oc * FHEVC_NODES + nidx] = o;
    }
  }
}

}  // namespace

// what the device keeps resident, at most four workgroups per CU at MR = 8 (38 912 B of static LDS for the transform buffers and the matrix) and two at
// MR = 64: the LDS holds two windows per CU at most
hipError_t fhevc_launch_motion_skip(const FhevcFrames& fr, int max_range, const FhevcSkipQuant& q, const FhevcMotionMergeNode* d_merge, FhevcMotionSkipNode* d_out,
                                    int num_cus, hipStream_t stream)
{
  static_assert(sizeof(FhevcMotionMergeNode) == 16 && sizeof(FhevcMotionSkipNode) == 16, "record layouts");
  const unsigned* merge = reinterpret_cast<const unsigned*>(d_merge);
  return refine_launch<FHEVC_MOTION_WIDE_MAX_RANGE>(fr, true, max_range, num_cus, {4, true}, {2, true}, stream, [&](auto t, auto, auto mr, const RefineLaunch& L) {
    return refine_launch_kernel<&fhevc_motion_skip_kernel<decltype(t), decltype(mr)::value>>(L, fr, max_range, q, merge, d_out);
  });
}
