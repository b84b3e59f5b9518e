// k_motion_rd.hip -- the RD estimate per CU node at a vector (config 4: P slices), gfx950 only.
//
// Spec in include/fasthevc.h: k_motion_skip.hip's pass carried through to the end.  The residual of fhevc_motion_refine's prediction at the vector a merge
// record or a refined node holds goes through HM's forward DCT (xTrMxN), its plain quantiser, its dequantiser (xDeQuant) and its inverse DCT (xITrMxN); the
// rebuilt block gives xGetSSE's distortion, the levels the library's own bit estimate; all of it at two TU sizes, N0 = min(node, 32) and N0 / 2, and per
// depth-0 TU the cheaper of the two under J = 256 D + lam_q8 bits (TEncSearch.cpp:5117).
//
// Mapping: k_motion_skip.hip's.  Workgroup (4 waves) = one CTU at a time over a persistent grid, the window of the refinement in LDS in both layouts, wave =
// level and lane = one 8x8 tile for the prediction; the lane keeps its tile's residual packed in registers to the end and loads the original again for the squared error (the prediction is their
// difference).  Once the window is dead, four buffers of 64 rows x 72 shorts (one per level) lie over it, behind them the 32-point matrix (2 048 B: the
// forward passes read its rows 32 / N k, first N columns) and the four TRANSPOSED matrices (32-, 16-, 8-, 4-point: 2 720 B; a smaller transpose is no
// sub-block of a larger one), all read at wave-uniform addresses.  One depth = four passes, each "every thread reads its row segment, makes dot products
// with matrix rows, a barrier, every thread writes": forward rows (written transposed inside the TU, as partialButterfly does), forward columns (quantised,
// priced, dequantised in registers and written back IN PLACE: the thread of row k then holds horizontal frequency k over the vertical frequencies, which is
// what partialButterflyInverse's first stage reads), inverse first stage on the transposed matrix (shift 7, clipped, written transposed), inverse second
// stage (shift 20 - bit depth, clipped, in place).  Then the lane that holds the tile reads its 8x8 of the rebuilt residual and takes the squared error.
// The residual is rewritten from registers and the same four passes run at N / 2.  Thread mapping per buffer: lane = row; N = 32: wave = (segment, half of
// the outputs); N = 16: wave = segment; N = 8: segments w and w + 4; N = 4: segments w, w + 4, w + 8, w + 12 -- 16 outputs per thread, buffer and pass.
// Sums per depth-0 TU (88 per CTU): bits and max |c| through eight-lane exchanges and LDS atomics, the distortion through lane exchanges over the TU's
// tiles and ONE plain store.  The writer lane of each node makes the choice.  16-bit intermediates are exact: forward as in k_motion_skip.hip, now also at
// N = 4; the inverse clips to 16 bits by definition, and its accumulations stay below 32 * 32 768 * 90 < 2^31.  The quantiser's and dequantiser's numbers
// per TU size travel by value.  No scratch, no HBM state between calls.
//
// The PU instances (fhevc_motion_rd_pu_device; PU = true): the same kernel with the prediction COMPOSED from the vectors of the two parts of one of HM's
// partition sizes.  Per lane the node's size p (forced, or one dword of its selection record), the two parts' records at addresses that depend on lane,
// node and p alone, the merged decision and the side bits -- computed by every lane of the node, as the node's record is --, and per 4x4 quadrant of the
// lane's tile the part that holds it (RefinePuPass::qmask's arithmetic).  One prediction at the vector of the part that holds quadrant 0; only in a wave
// where some tile straddles the cut (AMP of the 16x16 nodes, everything of the 8x8 nodes) a second one at the other part's vector, and the residual
// registers are taken per quadrant: D[4 y + k] holds columns 2 k, 2 k + 1 of row y, so a quadrant is whole registers.  Everything behind the residual is
// the code above, untouched; the writer lane folds its record into an earlier launch's where one is given.  The PU = false instances keep their argument
// list (the PU arguments are a pack that is empty there) and their code.
//
// The intra instances (fhevc_intra_rd_device; fhevc_intra_rd_kernel further below): the same passes behind another prediction -- the first pass's ONE mode per
// node, predicted per TU from the first pass's own reference lines, separately for the two TU depths.  No window: the lines and the staged CTU take its place.
#include "fhevc_internal.h"
#include "k_had8x8.h"
#include "k_refine_tile.h"
#include "k_firstpass_common.h"
#include <type_traits>

namespace {

constexpr unsigned kRdMark = 0xFFFFFFFFu;
constexpr int kPitch = 72;                       // shorts per row of a transform buffer
constexpr int kLevelBuf = 64 * kPitch;           // shorts per level
constexpr int kTransformShorts = 4 * kLevelBuf;  // 36 864 B
constexpr int kFwdShorts = 32 * 32;              // the 32-point matrix behind them
constexpr int kInvShorts = 32 * 32 + 16 * 16 + 8 * 8 + 4 * 4;   // ... and the four transposes behind it
constexpr int kRowsInFlight = 2;                 // matrix rows the scheduler may fetch ahead of their products
constexpr int kTus = 88, kAccWords = 5;          // per depth-0 TU: D0, bits0 - 1, sum D1, sum bits1 - 4, max |c| at depth 0
constexpr int kFineTus = 16 + 64, kFineWords = 4;   // three TU depths: per depth-1 TU of levels 1 and 2: D1, bits1 - 1, sum D2, sum bits2 - 4
constexpr int kFineShorts = kFineTus * kFineWords * 2;   // ... as shorts: 1 280 B behind the matrices
constexpr int kDstAt = kFwdShorts + kInvShorts + kFineShorts, kDstShorts = 32;   // the intra instances of three TU depths: the DST-VII of the 4x4 luma TUs, [k][x] then [x][k], behind those sums
enum { ROWS = 0, COLS = 1, INV1 = 2, INV2 = 3 };

constexpr int ilog2(int n) { return n <= 1 ? 0 : 1 + ilog2(n >> 1); }
constexpr int inv_at(int n) { return n == 32 ? 0 : n == 16 ? 1024 : n == 8 ? 1280 : 1344; }   // where the N-point transpose begins, in shorts

// the 32-point matrix of the standard (H.265 8.6.4.2) as packed pairs [k][x / 2], low half = the even column, and the transposes [x][k / 2] of the N-point
// matrices (its rows 32 / N k, first N columns) at a pitch of N.  Entry m of kCos is the scaled cos(m pi / 64), entry 0 the DC row's 64
struct RdTables { unsigned fwd[kFwdShorts / 2], inv[kInvShorts / 2]; };
constexpr int kCos[32] = { 64, 90, 90, 90, 89, 88, 87, 85, 83, 82, 80, 78, 75, 73, 70, 67, 64, 61, 57, 54, 50, 46, 43, 38, 36, 31, 25, 22, 18, 13, 9, 4 };
constexpr int dct_entry(int k, int x)
{
  int a = ((2 * x + 1) * k) % 128;   // the angle in units of pi / 64
  if (a > 64) a = 128 - a;
  return a > 32 ? -kCos[64 - a] : kCos[a];
}
constexpr unsigned pack2(int lo, int hi) { return ((unsigned)lo & 0xFFFFu) | ((unsigned)hi << 16); }
constexpr RdTables make_tables()
{
  RdTables t{};
  for (int k = 0; k < 32; ++k)
    for (int j = 0; j < 16; ++j) t.fwd[k * 16 + j] = pack2(dct_entry(k, 2 * j), dct_entry(k, 2 * j + 1));
  for (int n = 4; n <= 32; n *= 2)
    for (int x = 0; x < n; ++x)
      for (int j = 0; j < n / 2; ++j) t.inv[(inv_at(n) + x * n) / 2 + j] = pack2(dct_entry(2 * j * (32 / n), x), dct_entry((2 * j + 1) * (32 / n), x));
  return t;
}
__constant__ RdTables kRdTables = make_tables();

// HM's DST-VII of the intra 4x4 luma TUs (g_as_DST_MAT_4, TComRom.cpp:513-517) in the same two forms: the matrix [k][x / 2] and its transpose [x][k / 2].
// fastForwardDst / fastInverseDst (TComTrQuant.cpp:412-466) are plain products with it, in the index order of the 4-point DCT's passes
struct DstTables { unsigned fwd[8], inv[8]; };
constexpr int kDst[4][4] = { { 29, 55, 74, 84 }, { 74, 74, 0, -74 }, { 84, -29, -74, 55 }, { 55, -84, 74, -29 } };
constexpr DstTables make_dst_tables()
{
  DstTables t{};
  for (int a = 0; a < 4; ++a)
    for (int j = 0; j < 2; ++j) {
      t.fwd[a * 2 + j] = pack2(kDst[a][2 * j], kDst[a][2 * j + 1]);
      t.inv[a * 2 + j] = pack2(kDst[2 * j][a], kDst[2 * j + 1][a]);
    }
  return t;
}
__constant__ DstTables kDstTables = make_dst_tables();

// which units of an N-point pass over one buffer a thread has: UNITS segments of its row, NK outputs of each from k0 on -- 16 outputs in all
template <int N> struct TuMap {
  static constexpr int NK = N < 16 ? N : 16, UNITS = 16 / NK;
  __device__ __forceinline__ static int seg(int wave, int u) { return N == 32 ? (wave & 1) : wave + 4 * u; }
  __device__ __forceinline__ static int k0(int wave) { return N == 32 ? (wave >> 1) * 16 : 0; }
};

// the row segment of N shorts at buf[row][x0 ..] as N / 2 packed pairs: 16-byte reads (N = 4: one of 8 bytes); x0 is a multiple of N, the pitch of 8
template <int N>
__device__ __forceinline__ void load_segment(const short* buf, int row, int x0, unsigned (&x)[N / 2])
{
  if constexpr (N == 4) {
    const uint2 q = *reinterpret_cast<const uint2*>(buf + row * kPitch + x0);
    x[0] = q.x; x[1] = q.y;
  } else {
    const uint4* p = reinterpret_cast<const uint4*>(buf + row * kPitch + x0);
#pragma unroll
    for (int i = 0; i < N / 8; ++i) {
      const uint4 q = p[i];
      x[4 * i] = q.x; x[4 * i + 1] = q.y; x[4 * i + 2] = q.z; x[4 * i + 3] = q.w;
    }
  }
}

// a + the product of a segment with the matrix row at m (wave-uniform; LDS)
template <int N>
__device__ __forceinline__ int dot_row(const short* m, const unsigned (&x)[N / 2], int a)
{
  if constexpr (N == 4) {
    const uint2 q = *reinterpret_cast<const uint2*>(m);
    a = dot2(x[0], q.x, a); a = dot2(x[1], q.y, a);
  } else {
    const uint4* p = reinterpret_cast<const uint4*>(m);
#pragma unroll
    for (int i = 0; i < N / 8; ++i) {
      const uint4 q = p[i];
      a = dot2(x[4 * i], q.x, a); a = dot2(x[4 * i + 1], q.y, a); a = dot2(x[4 * i + 2], q.z, a); a = dot2(x[4 * i + 3], q.w, a);
    }
  }
  return a;
}

__device__ __forceinline__ int clip16(int v) { return min(max(v, -32768), 32767); }

// eight neighbouring lanes (rows that share every depth-0 TU) into one, then that lane into the TU's sums
// FINE: tu counts depth-1 TUs (eight rows share those too: two 4x4 TUs of one 8x8 parent at the least) and acc holds their four words
template <int DEPTH, bool FINE = false>
__device__ __forceinline__ void rd_commit(unsigned* acc, int tu, int lane, unsigned bits, unsigned top)
{
  if constexpr (FINE) {
    static_assert(DEPTH >= 1, "a depth-1 TU has no depth 0");
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) bits += (unsigned)__shfl_xor((int)bits, d);
    if ((lane & 7) == 0) atomicAdd(&acc[kFineWords * tu + 2 * DEPTH - 1], bits);
    return;
  }
#pragma unroll
  for (int d = 1; d < 8; d <<= 1) {
    bits += (unsigned)__shfl_xor((int)bits, d);
    if (DEPTH == 0) top = max(top, (unsigned)__shfl_xor((int)top, d));
  }
  if ((lane & 7) == 0) {
    atomicAdd(&acc[kAccWords * tu + 1 + 2 * DEPTH], bits);
    if (DEPTH == 0) atomicMax(&acc[kAccWords * tu + 4], top);
  }
}

// the NxN candidate of the 8x8 nodes (fhevc_intra_rd_nxn*): three words per 8x8 node behind the sums per depth-0 TU -- the distortion, the level bits of
// its four 4x4 TUs (low half; bit 16 + i: TU i has a level), max |c|
constexpr int kNxnWords = 3;
// one unit of a 4-point COLS pass is one row of ONE 4x4 TU: four neighbouring lanes into one, then that lane into the words of the 8x8 node that holds the TU
__device__ __forceinline__ void rd_commit_nxn(unsigned* nx, int lane, int seg, unsigned bits, unsigned top)
{
#pragma unroll
  for (int d = 1; d < 4; d <<= 1) {
    bits += (unsigned)__shfl_xor((int)bits, d);
    top = max(top, (unsigned)__shfl_xor((int)top, d));
  }
  if ((lane & 3) == 0) {
    unsigned* const w = nx + kNxnWords * ((lane >> 3) * 8 + (seg >> 1));
    const int i = ((lane >> 2) & 1) * 2 + (seg & 1);   // fhevc_intra_p's order of the four PUs
    atomicAdd(&w[1], bits | (bits != 0u ? 0x10000u << i : 0u));   // 64 levels of 31 bits at the most: the low half never carries
    atomicMax(&w[2], top);
  }
}

// the candidate search (fhevc_intra_rd_search*): the 4x4 PUs are priced one by one, so the sums of a 4-point COLS pass over the level-3 buffer stay per PU --
// two words (level bits, max |c|) per unit of the CTU's 16x16 raster.  A 4x4 TU is one segment of four neighbouring rows: one lane holds it all, plain stores
constexpr int kPuWords = 2;
__device__ __forceinline__ void rd_commit_pu(unsigned* pw, int lane, int seg, unsigned bits, unsigned top)
{
#pragma unroll
  for (int d = 1; d < 4; d <<= 1) {
    bits += (unsigned)__shfl_xor((int)bits, d);
    top = max(top, (unsigned)__shfl_xor((int)top, d));
  }
  if ((lane & 3) == 0) {
    unsigned* const w = pw + kPuWords * ((lane >> 2) * 16 + seg);
    w[0] = bits; w[1] = top;
  }
}

// one pass over one buffer at TU size N: the thread's 16 outputs, packed two to a register until the barrier.  COLS quantises, prices and dequantises them
// and commits the sums of every unit to its depth-0 TU: tu0 = the buffer's first, l0 = log2 of the buffer's depth-0 TU size (FINE: of its depth-1 TUs)
// DST (the intra instances of three TU depths): a pass at N = 4 takes the DST matrix instead; the shifts and clips are the 4-point DCT's (xTrMxN, xITrMxN)
// NXN: the pass over the level-3 buffer at N = 4 behind the NxN prediction; acc is the NxN words then (PERPU: the candidate search's words per 4x4 PU)
template <int N, int STAGE, int DEPTH, bool FINE = false, bool DST = false, bool NXN = false, bool PERPU = false>
__device__ __forceinline__ void tu_pass(const short* tables, const short* buf, int lane, int wave, int bd, const FhevcRdQuant& Q, unsigned* acc, int tu0, int l0,
                                        unsigned (&t)[8])
{
  using M = TuMap<N>;
  constexpr int LN = ilog2(N), QI = LN - 2;
  constexpr bool D4 = DST && N == 4;
  const short* mat = D4 ? tables + kDstAt + (STAGE <= COLS ? 0 : 16) : STAGE <= COLS ? tables : tables + kFwdShorts + inv_at(N);
  constexpr int pitch = D4 ? 4 : STAGE <= COLS ? (32 / N) * 32 : N;
  const int shift = STAGE == ROWS ? LN + bd - 9 : STAGE == COLS ? LN + 6 : STAGE == INV1 ? 7 : 20 - bd;
  const int k0 = M::k0(wave);
#pragma unroll
  for (int u = 0; u < M::UNITS; ++u) {
    const int seg = M::seg(wave, u);
    unsigned x[N / 2];
    load_segment<N>(buf, lane, seg * N, x);
    unsigned bits = 0, top = 0;
#pragma unroll
    for (int i = 0; i < M::NK; ++i) {
      int a = dot_row<N>(mat + (k0 + i) * pitch, x, 1 << (shift - 1)) >> shift;
      if (STAGE == COLS) {
        const unsigned mag = (unsigned)abs(a);
        const unsigned lv = min((mag * Q.scale + Q.add_plain[QI]) >> Q.qbits[QI], 32767u);
        bits += lv != 0u ? 3u + 2u * (31u - (unsigned)__builtin_clz(lv)) : 0u;
        top = max(top, mag);
        const int sl = a < 0 ? -(int)lv : (int)lv;
        a = clip16((sl * (int)Q.inv_scale[QI] + (int)Q.inv_add[QI]) >> Q.inv_shift[QI]);
      }
      if (STAGE >= INV1) a = clip16(a);
      const int o = u * M::NK + i;
      if (o & 1) t[o >> 1] |= (unsigned)a << 16;
      else t[o >> 1] = (unsigned)a & 0xFFFFu;
      if ((i & (kRowsInFlight - 1)) == kRowsInFlight - 1) __builtin_amdgcn_sched_barrier(0);   // or every matrix row of the pass is fetched ahead, into registers
    }
    if constexpr (NXN) {
      static_assert(N == 4 && !FINE, "the NxN candidate is four 4x4 TUs");
      if constexpr (PERPU) { if (STAGE == COLS) rd_commit_pu(acc, lane, seg, bits, top); } else
      if (STAGE == COLS) rd_commit_nxn(acc, lane, seg, bits, top);
    } else
    if (STAGE == COLS) {
      int ln = lane;   // FINE: opaque, so that the depth-1 TU's index is worked out here and not kept through the CTU loop beside the depth-0 TU's
      if constexpr (FINE) asm volatile("" : "+v"(ln));
      rd_commit<DEPTH, FINE>(acc, tu0 + ((ln >> l0) << (6 - l0)) + ((seg * N) >> l0), ln, bits, top);
    }
  }
}

// ... written behind the barrier: ROWS and INV1 transposed inside the TU (output k of input row j at [k][j]), COLS and INV2 into the row they were read from
template <int N, int STAGE>
__device__ __forceinline__ void tu_store(short* buf, int lane, int wave, const unsigned (&t)[8])
{
  using M = TuMap<N>;
  const int k0 = M::k0(wave);
#pragma unroll
  for (int u = 0; u < M::UNITS; ++u) {
    const int seg = M::seg(wave, u);
    if (STAGE == ROWS || STAGE == INV1) {
      short* dst = buf + ((lane & ~(N - 1)) + k0) * kPitch + seg * N + (lane & (N - 1));
#pragma unroll
      for (int i = 0; i < M::NK; ++i) {
        const int o = u * M::NK + i;
        dst[i * kPitch] = (short)(o & 1 ? t[o >> 1] >> 16 : t[o >> 1] & 0xFFFFu);
      }
    } else {
      short* dst = buf + lane * kPitch + seg * N + k0;   // a multiple of NK shorts
      constexpr int R = M::NK / 2;                       // registers of this unit
      if constexpr (M::NK == 4) *reinterpret_cast<uint2*>(dst) = make_uint2(t[u * R], t[u * R + 1]);
      else {
#pragma unroll
        for (int i = 0; i < R / 4; ++i) reinterpret_cast<uint4*>(dst)[i] = make_uint4(t[u * R + 4 * i], t[u * R + 4 * i + 1], t[u * R + 4 * i + 2], t[u * R + 4 * i + 3]);
      }
    }
  }
}

// one pass over the four buffers: levels 0 and 1 at 32 >> DEPTH, level 2 at 16 >> DEPTH, level 3 at 8 >> DEPTH
// QT (three TU depths): the sums of depths 1 and 2 of the level-1 and level-2 buffers go per depth-1 TU into the words behind the matrices; DEPTH 2 is a
// pass over those two buffers alone, at 8 and 4, by all four waves
// NXN (fhevc_intra_rd_nxn*): the DEPTH 2 pass takes the level-3 buffer along, at 4: the NxN candidate's four TUs per 8x8 node, their sums behind acc's
template <int STAGE, int DEPTH, bool QT = false, bool DST = false, bool NXN = false>
__device__ __forceinline__ void rd_stage(short* s, int lane, int wave, int bd, const FhevcRdQuant& Q, unsigned* acc)
{
  static_assert(DEPTH < 2 || QT, "the third depth goes with QT");
  const short* tables = s + kTransformShorts;
  short *const b0 = s, *const b1 = s + kLevelBuf, *const b2 = s + 2 * kLevelBuf, *const b3 = s + 3 * kLevelBuf;
  if constexpr (DEPTH == 2) {
    unsigned* const fine = reinterpret_cast<unsigned*>(s + kTransformShorts + kFwdShorts + kInvShorts);
    unsigned t1[8], t2[8];
    tu_pass<8, STAGE, 2, true>(tables, b1, lane, wave, bd, Q, fine, 0, 4, t1);
    tu_pass<4, STAGE, 2, true, DST>(tables, b2, lane, wave, bd, Q, fine, 16, 3, t2);
    if constexpr (NXN) {
      unsigned t3[8];
      tu_pass<4, STAGE, 2, false, true, true>(tables, b3, lane, wave, bd, Q, acc + kAccWords * kTus, 0, 0, t3);
      __syncthreads();   // every thread has read
      tu_store<8, STAGE>(b1, lane, wave, t1);
      tu_store<4, STAGE>(b2, lane, wave, t2);
      tu_store<4, STAGE>(b3, lane, wave, t3);
      __syncthreads();
      return;
    }
    __syncthreads();   // every thread has read
    tu_store<8, STAGE>(b1, lane, wave, t1);
    tu_store<4, STAGE>(b2, lane, wave, t2);
    __syncthreads();
  } else {
    constexpr int NA = 32 >> DEPTH, NB = 16 >> DEPTH, NC = 8 >> DEPTH;
    unsigned t0[8], t1[8], t2[8], t3[8];
    tu_pass<NA, STAGE, DEPTH>(tables, b0, lane, wave, bd, Q, acc, 0, 5, t0);
    if constexpr (QT && DEPTH == 1) {
      unsigned* const fine = reinterpret_cast<unsigned*>(s + kTransformShorts + kFwdShorts + kInvShorts);
      tu_pass<NA, STAGE, DEPTH, true>(tables, b1, lane, wave, bd, Q, fine, 0, 4, t1);
      tu_pass<NB, STAGE, DEPTH, true>(tables, b2, lane, wave, bd, Q, fine, 16, 3, t2);
    } else {
      tu_pass<NA, STAGE, DEPTH>(tables, b1, lane, wave, bd, Q, acc, 4, 5, t1);
      tu_pass<NB, STAGE, DEPTH>(tables, b2, lane, wave, bd, Q, acc, 8, 4, t2);
    }
    tu_pass<NC, STAGE, DEPTH, false, DST>(tables, b3, lane, wave, bd, Q, acc, 24, 3, t3);
    __syncthreads();   // every thread has read
    tu_store<NA, STAGE>(b0, lane, wave, t0);
    tu_store<NA, STAGE>(b1, lane, wave, t1);
    tu_store<NB, STAGE>(b2, lane, wave, t2);
    tu_store<NC, STAGE>(b3, lane, wave, t3);
    __syncthreads();
  }
}

// one depth of the TU tree: the residual tiles into the buffers, the four passes, xGetSSE of this lane's tile of the rebuilt block (the per-sample shift
// of TComRdCost.cpp:1190-1199) summed over the tiles of its depth-0 TU
// The original tile is loaded a second time here (from the cache): kept in registers across the passes it cost the kernel its second wave per SIMD
// QT (three TU depths): at depths 1 and 2 the level-1 and level-2 waves sum over the tiles of their depth-1 TU (2 x 2 tiles, the lane's own) and store per
// depth-1 TU; at depth 2 only they rewrite their tiles and take the squared error -- the other two buffers have no third depth
// NXN (fhevc_intra_rd_nxn*): at depth 2 the level-3 wave writes its tile too -- the NxN prediction's residual -- and stores its squared error per 8x8 node
template <int DEPTH, typename T, bool QT = false, bool DST = false, bool NXN = false>
__device__ __forceinline__ void rd_depth(short* s, int lane, int lvl, int wave, int tx, int ty, const FhevcRdQuant& Q, unsigned* acc, const T* plane, long long cur_base,
                                         const FhevcFrames& F, int px, int py, bool inside, const unsigned (&D)[32])
{
  const int bd = F.bit_depth;
  short* const tile = s + lvl * kLevelBuf + (ty * 8) * kPitch + tx * 8;
  const bool fine = QT && DEPTH >= 1 && (wave == 1 || wave == 2);   // wave-uniform
  if (DEPTH < 2 || fine) {
#pragma unroll
    for (int y = 0; y < 8; ++y) *reinterpret_cast<uint4*>(tile + y * kPitch) = make_uint4(D[4 * y], D[4 * y + 1], D[4 * y + 2], D[4 * y + 3]);
  }
  if constexpr (NXN && DEPTH == 2) {
    if (wave == 3) {   // wave-uniform
#pragma unroll
      for (int y = 0; y < 8; ++y) *reinterpret_cast<uint4*>(tile + y * kPitch) = make_uint4(D[4 * y], D[4 * y + 1], D[4 * y + 2], D[4 * y + 3]);
    }
  }
  __syncthreads();
  rd_stage<ROWS, DEPTH, QT, DST, NXN>(s, lane, wave, bd, Q, acc);
  rd_stage<COLS, DEPTH, QT, DST, NXN>(s, lane, wave, bd, Q, acc);
  rd_stage<INV1, DEPTH, QT, DST, NXN>(s, lane, wave, bd, Q, acc);
  rd_stage<INV2, DEPTH, QT, DST, NXN>(s, lane, wave, bd, Q, acc);
  if constexpr (NXN) {
    if (DEPTH == 2 && !fine && wave != 3) { __syncthreads(); return; }
  } else
  if (DEPTH == 2 && !fine) { __syncthreads(); return; }
  const int top = (1 << bd) - 1, sh = 2 * (bd - 8);
  unsigned O[32];
  load_tile8x8(plane, cur_base, F, px, py, inside, O);
  unsigned sum = 0;
#pragma unroll
  for (int y = 0; y < 8; ++y) {
    const uint4 q = *reinterpret_cast<const uint4*>(tile + y * kPitch);
    const unsigned r[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned o = O[4 * y + k], p = pk_sub(o, D[4 * y + k]);   // the prediction: original minus residual
      const int e0 = (int)(o & 0xFFFFu) - min(max((int)(p & 0xFFFFu) + (int)(short)(r[k] & 0xFFFFu), 0), top);
      const int e1 = (int)(o >> 16) - min(max((int)(p >> 16) + (int)(short)(r[k] >> 16), 0), top);
      sum += ((unsigned)(e0 * e0) >> sh) + ((unsigned)(e1 * e1) >> sh);
    }
  }
  if constexpr (NXN && DEPTH == 2) {
    if (wave == 3) {
      acc[kAccWords * kTus + kNxnWords * lane] = sum;   // the lane's tile is its 8x8 node
      __syncthreads();
      return;
    }
  }
  if (fine) {
    const int lt = 2 - wave;                 // log2 of the depth-1 TU's side in tiles: 16 of 2 x 2 tiles at level 1, 64 of one tile at level 2
    for (int k = 0; k < lt; ++k) {
      sum += __shfl_xor(sum, 1 << k);
      sum += __shfl_xor(sum, 8 << k);
    }
    unsigned* const words = reinterpret_cast<unsigned*>(s + kTransformShorts + kFwdShorts + kInvShorts);
    int ln = lane;   // opaque: where the sum goes is worked out here, not kept through the CTU loop
    asm volatile("" : "+v"(ln));
    const int ux = ln & 7, uy = ln >> 3;
    const int m = (1 << lt) - 1, e = (wave == 1 ? 0 : 16) + (uy >> lt) * (8 >> lt) + (ux >> lt);
    if ((ux & m) == 0 && (uy & m) == 0) words[kFineWords * e + 2 * DEPTH - 2] = sum;
    __syncthreads();
    return;
  }
  const int lt = wave <= 1 ? 2 : 3 - wave;   // log2 of the depth-0 TU's side in tiles
  for (int k = 0; k < lt; ++k) {
    sum += __shfl_xor(sum, 1 << k);
    sum += __shfl_xor(sum, 8 << k);
  }
  const int m = (1 << lt) - 1, tu0 = wave == 0 ? 0 : wave == 1 ? 4 : wave == 2 ? 8 : 24;
  if ((tx & m) == 0 && (ty & m) == 0) acc[kAccWords * (tu0 + (ty >> lt) * (8 >> lt) + (tx >> lt)) + 2 * DEPTH] = sum;
  __syncthreads();   // the tiles are read: the next depth rewrites them; the sums are in
}

// the candidate search (fhevc_intra_rd_search*): ONE position of the 4x4 PUs' lists -- the level-3 wave's tiles (four PUs each, every one predicted at its own
// candidate: D is that residual) into the level-3 buffer, the four passes over that buffer ALONE at N = 4 with the DST by all four waves, the sums per PU in pw;
// the lanes of the level-3 wave come back with the squared error of their tile's four PUs (fhevc_intra_p's order), the others with nothing
template <int STAGE>
__device__ __forceinline__ void rd_pu_stage(short* s, int lane, int wave, int bd, const FhevcRdQuant& Q, unsigned* pw)
{
  unsigned t3[8];
  tu_pass<4, STAGE, 2, false, true, true, true>(s + kTransformShorts, s + 3 * kLevelBuf, lane, wave, bd, Q, pw, 0, 0, t3);
  __syncthreads();   // every thread has read
  tu_store<4, STAGE>(s + 3 * kLevelBuf, lane, wave, t3);
  __syncthreads();
}
template <typename T>
__device__ __forceinline__ void rd_pu_pass(short* s, int lane, int wave, int tx, int ty, const FhevcRdQuant& Q, unsigned* pw, const T* plane, long long cur_base,
                                           const FhevcFrames& F, int px, int py, bool inside, const unsigned (&D)[32], unsigned (&sse)[4])
{
  const int bd = F.bit_depth;
  short* const tile = s + 3 * kLevelBuf + (ty * 8) * kPitch + tx * 8;
  if (wave == 3) {   // wave-uniform
#pragma unroll
    for (int y = 0; y < 8; ++y) *reinterpret_cast<uint4*>(tile + y * kPitch) = make_uint4(D[4 * y], D[4 * y + 1], D[4 * y + 2], D[4 * y + 3]);
  }
  __syncthreads();
  rd_pu_stage<ROWS>(s, lane, wave, bd, Q, pw);
  rd_pu_stage<COLS>(s, lane, wave, bd, Q, pw);
  rd_pu_stage<INV1>(s, lane, wave, bd, Q, pw);
  rd_pu_stage<INV2>(s, lane, wave, bd, Q, pw);
  sse[0] = sse[1] = sse[2] = sse[3] = 0u;
  if (wave != 3) return;   // the tiles are the level-3 wave's own, read and rewritten by the lane that holds them: no barrier behind this
  const int top = (1 << bd) - 1, sh = 2 * (bd - 8);
  unsigned O[32];
  load_tile8x8(plane, cur_base, F, px, py, inside, O);
#pragma unroll
  for (int y = 0; y < 8; ++y) {
    const uint4 q = *reinterpret_cast<const uint4*>(tile + y * kPitch);
    const unsigned r[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned o = O[4 * y + k], p = pk_sub(o, D[4 * y + k]);   // the prediction: original minus residual
      const int e0 = (int)(o & 0xFFFFu) - min(max((int)(p & 0xFFFFu) + (int)(short)(r[k] & 0xFFFFu), 0), top);
      const int e1 = (int)(o >> 16) - min(max((int)(p >> 16) + (int)(short)(r[k] >> 16), 0), top);
      sse[(y >> 2) * 2 + (k >> 1)] += ((unsigned)(e0 * e0) >> sh) + ((unsigned)(e1 * e1) >> sh);
    }
  }
}

// bits(m) of fhevc_intra_p: planar 2, DC and vertical 3, every other mode 6 (the search instances' code; the instances there were keep their own expression)
__device__ __forceinline__ unsigned intra_mode_bits(unsigned m) { return m == 0u ? 2u : (m == 1u || m == 26u) ? 3u : 6u; }

// the candidate at position pos of the list whose entry begins at e: the byte there while pos < count (255 where it is above 34: skipped); at pos == count the
// appended planar -- iff append, the first count bytes hold a valid mode and none of them is 0 --; 255 behind that.  count <= the entry's stride, and no byte
// reaches an address or a loop bound
__device__ __forceinline__ unsigned search_cand(const unsigned char* __restrict__ e, int count, int append, int pos)
{
  if (pos < count) { const unsigned b = e[pos]; return b <= 34u ? b : 255u; }
  if (pos > count || !append) return 255u;
  bool any = false, zero = false;
  for (int i = 0; i < count; ++i) { const unsigned b = e[i]; any = any || b <= 34u; zero = zero || b == 0u; }
  return any && !zero ? 0u : 255u;
}

// ---- the PU instances: what one lane knows of its node's partition size ----
struct RdPuArgs {
  const unsigned *pus, *small;               // the refined (or re-priced) entries of the 124 and of the 384 PUs; small may be null
  const unsigned *merge_pus, *merge_small;   // their merge records, or null
  const unsigned *mvp_pus, *mvp_small;       // their predictor records, or null
  const unsigned *shapes, *fold;             // the selection's records (part_mode 8, 9), an earlier launch's output; or null
  int part_mode;
};
struct RdPuLane {
  unsigned first = 0, other = 0;   // the vector dwords of the part that holds quadrant 0 of the lane's tile, and of the other part
  unsigned info = 255u << 18;      // everything else in one register, which is all that lives through the transform: bits 0..11 the parts' side bits (at most
                                   // 2 x 256), 12..13 merged, 14..17 bit k: quadrant k of the tile lies in the other part, 18..25 p, 26 both parts usable
                                   // (before the INSIDE test), 27 this lane's tile needs the second prediction
  __device__ __forceinline__ unsigned side() const { return info & 0xFFFu; }
  __device__ __forceinline__ unsigned merged() const { return (info >> 12) & 3u; }
  __device__ __forceinline__ unsigned flips() const { return (info >> 14) & 15u; }
  __device__ __forceinline__ unsigned p() const { return (info >> 18) & 0xFFu; }
  __device__ __forceinline__ bool ok() const { return (info >> 26) & 1u; }
  __device__ __forceinline__ bool two() const { return (info >> 27) & 1u; }
};
// one part: the refined entry e of its family against its merge record (HM's uiMRGCost < uiMECost, strictly), the vector taken and its side bits.  Without
// branches: an array that is not there is read in the refined entries instead (in bounds: the same entry, or half-way to it) and what was read is dropped
__device__ __forceinline__ bool rd_pu_part(const unsigned* ref, const unsigned* mrg, const unsigned* mvp, long long e, int reach, unsigned& vec, unsigned& side, bool& merged)
{
  const unsigned* const m = mrg ? mrg : ref;
  const unsigned* const pv = mvp ? mvp : ref;
  const unsigned rc = ref[e * 4 + 2], rv = ref[e * 4 + 3], mc = mrg ? m[e * 4 + 1] : kRdMark, mv = m[e * 4 + 2], mi = m[e * 4 + 3] & 0xFFu;
  const unsigned w = pv[e * 2 + 1];         // idx in the low byte (255: a marker), bits in the high one
  merged = mc < rc;                         // a marker loses to anything
  vec = merged ? mv : rv;
  const bool ok = merged || (rc != kRdMark && !(mvp && (w & 0xFFu) == 255u));   // both markers: nothing to take
  side = merged ? (mi == 4u ? 4u : mi + 1u) : mvp ? w >> 24 : (unsigned)(eg_bits(vec_x(rv)) + eg_bits(vec_y(rv)));
  return ok && vec_in_reach(vec, reach);
}
// the lane's node k of level lvl in the CTU with output index oc; own_ok / own_vec / own_side: what the node's own record gives (p = 0).  No input byte
// reaches an address: p is used only once it is one of the six two-part sizes that level has, and then selects among entries of this node
__device__ __forceinline__ RdPuLane rd_pu_lane(const RdPuArgs& A, long long oc, int k, int lvl, int tx, int ty, int reach, bool own_ok, unsigned own_vec, unsigned own_side)
{
  RdPuLane L;
  int p = A.part_mode;
  if (p >= 8) p = (int)((A.shapes[(oc * FHEVC_NODES + k) * 4 + 3] >> (p == 8 ? 0 : 8)) & 0xFFu);   // best: byte 12, second: byte 13
  L.info = (unsigned)p << 18;
  if (p == 0) { L.first = L.other = own_vec; L.info = own_side | (own_ok ? 1u << 26 : 0u); return L; }
  const bool two_part = p == 1 || p == 2 || (p >= 4 && p <= 7);
  const bool amp = p >= 4;
  const bool in_small = lvl == 3 || (lvl == 2 && amp);
  const unsigned* ref = in_small ? A.small : A.pus;
  if (!two_part || (lvl == 3 && amp) || !ref) return L;   // AMP of the 8x8 nodes, a family that is not there, 3 and 255: the marker
  const int shape = amp ? p - 2 : p - 1;
  const int e0 = lvl < 2 ? k * 12 + shape * 2 : lvl == 2 ? (amp ? (k - 5) * 8 + (shape - 2) * 2 : 60 + (k - 5) * 4 + shape * 2) : 128 + (k - 21) * 4 + shape * 2;
  const long long e = oc * (in_small ? FHEVC_PUS_SMALL : FHEVC_PUS) + e0;
  const unsigned* mrg = in_small ? A.merge_small : A.merge_pus;
  const unsigned* mvp = in_small ? A.mvp_small : A.mvp_pus;
  unsigned v0, v1, s0, s1;
  bool m0, m1;
  const bool ok0 = rd_pu_part(ref, mrg, mvp, e, reach, v0, s0, m0), ok1 = rd_pu_part(ref, mrg, mvp, e + 1, reach, v1, s1, m1);
  L.info |= (s0 + s1) | (m0 ? 1u << 12 : 0u) | (m1 ? 2u << 12 : 0u) | (ok0 && ok1 ? 1u << 26 : 0u);
  // which part holds each quadrant: positions in 4-sample units from the node's top (left) edge against the cut (getPartIndexAndSize)
  const int tn = 8 >> lvl, s4 = 16 >> lvl;
  const bool horiz = p == 1 || p == 4 || p == 5;
  const int cut = !amp ? s4 / 2 : (p & 1) ? 3 * s4 / 4 : s4 / 4;
  const int at = horiz ? (ty & (tn - 1)) * 2 : (tx & (tn - 1)) * 2;
  unsigned parts = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) parts |= (at + (horiz ? q >> 1 : q & 1) >= cut ? 1u : 0u) << q;
  const bool swap = (parts & 1u) != 0u;
  L.first = swap ? v1 : v0; L.other = swap ? v0 : v1;
  const unsigned flips = swap ? parts ^ 15u : parts;
  L.info |= flips << 14 | (flips != 0u && v0 != v1 ? 1u << 27 : 0u);
  return L;
}

struct RdThreeDepths {};   // a tag in the kernel's argument pack: it carries nothing
struct RdNxN { const unsigned* first4; unsigned* nxn; };   // the second tag of the intra instances: the 4x4 first pass's records as dwords, the plain NxN records (or null)
// the third tag (fhevc_intra_rd_search*), behind RdThreeDepths in RdNxN's place: the node lists (85 entries of stride bytes per CTU), the 4x4 PUs' lists (256 of
// stride4; or null), the plain NxN records (or null) and the rule: count[l] in byte l of counts
struct RdSearch { const unsigned char *modes, *modes4; unsigned* nxn; int stride, stride4; unsigned counts; int count4, append; };
// where the tag stands in front of the PU arguments, the comma fold that picks the pack's last argument drops it: that is what it is for
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-value"

// T = int16_t or uint8_t planes; MR = 8 or 64: the largest max_range the window is laid out for
// PU (fhevc_motion_rd_pu_device): the prediction is composed from the two parts of a partition size; A...: ONE RdPuArgs then, empty otherwise -- a pack keeps
// the plain instances' argument list, and so their code, what it was.  in / mvp are the nodes' own records there (source 1)
// Three TU depths (fhevc_motion_rd_qt* at tu_depths 3): RdThreeDepths IN FRONT of the pack -- the 32x32 and 16x16 nodes get their third TU size, with sums per
// depth-1 TU behind the matrices.  Without it the instances are the ones there always were, by name and by code
template <typename T, int MR, bool PU, class... A>
__global__ __launch_bounds__(256) void fhevc_motion_rd_kernel(FhevcFrames F, int max_range, FhevcRdQuant Q, int source, const unsigned* __restrict__ in,
                                                              const unsigned* __restrict__ mvp, FhevcMotionRdNode* __restrict__ out, A... pu_args)
{
  constexpr bool QT = (std::is_same_v<A, RdThreeDepths> || ...);
  static_assert(sizeof...(A) == (PU ? 1 : 0) + (QT ? 1 : 0), "the PU arguments go with the PU instances, the tag with those of three TU depths");
  constexpr int RP = RefineGeom<MR>::RP;
  constexpr bool BIG = MR > FHEVC_MOTION_MAX_RANGE;
  constexpr int OVER = kTransformShorts + kFwdShorts + kInvShorts + (QT ? kFineShorts : 0);   // what lies over the dead window: 41 632 B (QT: 42 912 B)
  constexpr int SMALL = RefineGeom<MR>::SAMPLES > OVER ? RefineGeom<MR>::SAMPLES : OVER;   // the larger of the two uses
  static_assert(!BIG || RefineGeom<MR>::SAMPLES >= OVER, "the dynamic window holds the transform buffers and the matrices");
  static_assert(sizeof(RdTables) == (kFwdShorts + kInvShorts) * 2 && sizeof(RdTables) / 4 <= 5 * 256, "the tables: five dwords per thread at most");
  extern __shared__ __attribute__((aligned(16))) short s_dyn[];
  __shared__ __attribute__((aligned(16))) short s_small[BIG ? 8 : SMALL];
  short* const s_ref = BIG ? s_dyn : s_small;
  __shared__ unsigned s_taps[16], s_acc[kAccWords * kTus];
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
  const int cost_at = source ? 2 : 1;   // the marker test's dword; the vector is the next one

  for (int work = blockIdx.x; work < total; work += gridDim.x) {
    const SearchWork W(F, work);
    const int cy = W.cy, cx = W.cx;
    const long long oc = W.oc(F);
    // ---- the node's input record: the marker test, the vector, the side bits; the addresses depend on geometry alone ----
    const bool node_in = cx * N.ncnt + N.nbx < gw && cy * N.ncnt + N.nby < gh;
    const long long rec = oc * FHEVC_NODES + nidx;
    const unsigned rcost = in[rec * 4 + cost_at], rvec = in[rec * 4 + cost_at + 1];
    const int vx = vec_x(rvec), vy = vec_y(rvec);
    unsigned side;
    bool marked = rcost == kRdMark;
    if (source == 0) {
      const unsigned idx = in[rec * 4 + 3] & 0xFFu;   // the merge stage's own pricing of the index
      side = idx == 4u ? 4u : idx + 1u;
    } else if (mvp) {
      const unsigned w = mvp[rec * 2 + 1];            // idx in the low byte (255: a marker), bits in the high one
      marked = marked || (w & 0xFFu) == 255u;
      side = w >> 24;
    } else side = (unsigned)(eg_bits(vx) + eg_bits(vy));
    RdPuLane L;
    if constexpr (PU) {
      const RdPuArgs pa = (pu_args, ...);   // the pack's last argument
      // the lane number and the level made opaque once per CTU: what the part addresses derive from it is then computed here, inside the loop.  Hoisted out of it, those
      // values lived through the whole loop in nine registers more than the 256 there are.  (One is still missing: DESIGN 4.12)
      int ln = lane, wv = wave;   // the level as the scalar it is
      asm volatile("" : "+v"(ln), "+s"(wv));
      const RefineNode M(wv, ln & 7, ln >> 3);
      L = rd_pu_lane(pa, oc, M.nidx, wv, ln & 7, ln >> 3, reach, !marked && vec_in_reach(rvec, reach), rvec, side);
      side = L.side();
    }
    // ---- stage the part of the reference window that max_range reaches ----
    __syncthreads();  // the previous CTU's readers of the buffers and of the sums are done
    refine_stage_window_reach<T, MR>(s_ref, plane, W.ref_base, F, cx, cy, tid, max_range);
    for (int i = tid; i < kAccWords * kTus; i += 256) s_acc[i] = 0;
    const int px = cx * 64 + tx * 8, py = cy * 64 + ty * 8;
    const bool inside = (px + 8 <= F.width) && (py + 8 <= F.height);
    unsigned O[32];
    if constexpr (!PU) load_tile8x8(plane, W.cur_base, F, px, py, inside, O);
    const bool valid = PU ? node_in && L.ok() : node_in && !marked && vec_in_reach(rvec, reach);
    const int qx = valid ? (PU ? vec_x(L.first) : vx) : 0, qy = valid ? (PU ? vec_y(L.first) : vy) : 0;   // an invalid node predicts at the zero vector and drops the result: no read outside the window
    __syncthreads();
    // ---- the residual of this lane's tile at its node's vector ----
    unsigned D[32];
    {
      int v[64];
      if constexpr (!PU) refine_tile_at<true, RP>(s_ref, s_taps, arith, tx, ty, qx, qy, O, D, v);
      else {
        // the predictions are taken against a zero tile and the original is added behind them: the original live across a second prediction cost
        // 26 registers more (packed 16-bit arithmetic wraps, so o + (0 - p) is o - p)
        unsigned Z[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) Z[i] = 0u;
        refine_tile_at<true, RP>(s_ref, s_taps, arith, tx, ty, qx, qy, Z, D, v);
        // ---- ... and, where some tile of the wave straddles the cut, at the other part's vector: the quadrants of that part come from there ----
        const bool two = valid && L.two();
        if (__builtin_amdgcn_ballot_w64(two) != 0) {
          unsigned E[32];
          refine_tile_at<true, RP>(s_ref, s_taps, arith, tx, ty, two ? vec_x(L.other) : qx, two ? vec_y(L.other) : qy, Z, E, v);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const bool flip = two && ((L.flips() >> q) & 1u) != 0u;
#pragma unroll
            for (int y = 0; y < 4; ++y) {
              const int r = 4 * ((q >> 1) * 4 + y) + (q & 1) * 2;
              D[r] = flip ? E[r] : D[r]; D[r + 1] = flip ? E[r + 1] : D[r + 1];
            }
          }
        }
        unsigned P[32];
        load_tile8x8(plane, W.cur_base, F, px, py, inside, P);
#pragma unroll
        for (int i = 0; i < 32; ++i) D[i] = pk_add(P[i], D[i]);
      }
    }
    __syncthreads();  // the window is dead: the transform buffers and the matrices lie over it
    {
      unsigned* mdst = reinterpret_cast<unsigned*>(s_ref + kTransformShorts);
      const unsigned* msrc = reinterpret_cast<const unsigned*>(&kRdTables);
      for (int i = tid; i < (kFwdShorts + kInvShorts) / 2; i += 256) mdst[i] = msrc[i];
      // the sums per depth-1 TU lie behind the matrices, in what was window: zeroed here, not with s_acc during staging
      if constexpr (QT)
        for (int i = tid; i < kFineTus * kFineWords; i += 256) mdst[(kFwdShorts + kInvShorts) / 2 + i] = 0u;
    }
    rd_depth<0, T, QT>(s_ref, lane, lvl, wave, tx, ty, Q, s_acc, plane, W.cur_base, F, px, py, inside, D);
    rd_depth<1, T, QT>(s_ref, lane, lvl, wave, tx, ty, Q, s_acc, plane, W.cur_base, F, px, py, inside, D);
    if constexpr (QT) rd_depth<2, T, QT>(s_ref, lane, lvl, wave, tx, ty, Q, s_acc, plane, W.cur_base, F, px, py, inside, D);
    if (N.writer) {
      FhevcMotionRdNode o;
      o.dist = o.cost_rd = kRdMark; o.bits = 0xFFFFu; o.flags = 0; o.tu_split = 0; o.mvx = o.mvy = 0;
      if (valid) {
        const int qi = lvl == 3 ? 1 : (lvl == 2 ? 2 : 3);                // the depth-0 TU size's numbers
        const int tu0 = lvl == 0 ? 0 : (lvl == 1 ? 4 : lvl == 2 ? 8 : 24) + (nidx - N.first), ntu = lvl == 0 ? 4 : 1;   // a 64x64 node: four TUs
        unsigned long long j = (unsigned long long)Q.lam_q8 * side, bits = side;
        unsigned dist = 0, top = 0, any0 = 0, split = 0;
        if (QT && (lvl == 1 || lvl == 2)) {
          // HM's recursion over three depths (TEncSearch.cpp:5020-5134), bottom-up: per depth-1 TU its own cost with its split flag against its four
          // children, then the depth-0 TU against the four results.  A split depth-1 TU counts as coded one level up (:5093-5101)
          const unsigned lam = Q.lam_q8;
          const unsigned* const fine = reinterpret_cast<const unsigned*>(s_ref + kTransformShorts + kFwdShorts + kInvShorts);
          const unsigned* a = &s_acc[kAccWords * tu0];
          // the lane number and the level made opaque, here and where the sums are committed and stored: what the depth-1 TU's place derives from them is then
          // computed on the spot.  Hoisted out of the CTU loop those values cost the plain instances their second wave per SIMD
          int ln = lane, wv = wave;
          asm volatile("" : "+v"(ln), "+s"(wv));
          const RefineNode M(wv, ln & 7, ln >> 3);
          const int e0 = wv == 1 ? (2 * M.nby) * 4 + 2 * M.nbx : 16 + (2 * M.nby) * 8 + 2 * M.nbx, row = wv == 1 ? 4 : 8;   // the node's first depth-1 TU
          const unsigned d0 = a[0], r0 = 1u + a[1];
          const unsigned long long j0 = 256ull * d0 + (unsigned long long)lam * (1u + r0);
          unsigned long long j1 = lam;
          unsigned dsub = 0, rsub = 0, s1 = 0;
          bool coded = false;
          for (int i = 0; i < 4; ++i) {
            const unsigned* b = &fine[kFineWords * (e0 + (i >> 1) * row + (i & 1))];
            const unsigned d1 = b[0], r1 = 1u + b[1], d2 = b[2], r2 = 4u + b[3];
            const unsigned long long k1 = 256ull * d1 + (unsigned long long)lam * (1u + r1), k2 = 256ull * d2 + (unsigned long long)lam * (1u + r2);
            const bool take1 = b[3] != 0u && k2 < k1;
            j1 += take1 ? k2 : k1; dsub += take1 ? d2 : d1; rsub += 1u + (take1 ? r2 : r1);
            s1 |= take1 ? 16u << i : 0u; coded = coded || take1 || b[1] != 0u;
          }
          const bool take = coded && j1 < j0;
          j += take ? j1 : j0; dist = take ? dsub : d0; bits += 1u + (take ? rsub : r0);
          split = take ? 1u | s1 : 0u; any0 = a[1]; top = a[4];
        } else
        for (int i = 0; i < ntu; ++i) {
          const unsigned* a = &s_acc[kAccWords * (tu0 + i)];
          const unsigned d0 = a[0], r0 = 1u + a[1], d1 = a[2], r1 = 4u + a[3];
          const unsigned long long j0 = 256ull * d0 + (unsigned long long)Q.lam_q8 * (1u + r0), j1 = 256ull * d1 + (unsigned long long)Q.lam_q8 * (1u + r1);
          const bool take = a[3] != 0u && j1 < j0;                        // uiCbfAny && dSubdivCost < dSingleCost
          j += take ? j1 : j0; dist += take ? d1 : d0; bits += 1u + (take ? r1 : r0);
          split |= take ? 1u << i : 0u; any0 |= a[1]; top = max(top, a[4]);
        }
        // both levels grow with |c|: the node is zero under an offset iff its largest coefficient is
        const bool zero_half = ((top * Q.scale + Q.add_half[qi]) >> Q.qbits[qi]) == 0u;
        j >>= 8;
        o.dist = dist; o.cost_rd = j < 0xFFFFFFFEull ? (unsigned)j : 0xFFFFFFFEu;
        o.bits = (uint16_t)(bits < 65535ull ? bits : 65535ull);
        o.flags = (uint8_t)((any0 == 0u ? 1 : 0) | (zero_half ? 2 : 0) | (split ? 4 : 0)); o.tu_split = (uint8_t)split;
        o.mvx = (short)vx; o.mvy = (short)vy;
      }
      if constexpr (PU) {
        const RdPuArgs pa = (pu_args, ...);   // the pack's last argument
        FhevcMotionRdPuNode u;
        u.dist = o.dist; u.cost_rd = o.cost_rd; u.bits = o.bits; u.flags = o.flags; u.tu_split = o.tu_split;
        u.part = (uint8_t)(valid ? L.p() : 255u); u.merged = (uint8_t)(valid ? L.merged() : 0u); u.pad[0] = u.pad[1] = 0;
        FhevcMotionRdPuNode* const dst = reinterpret_cast<FhevcMotionRdPuNode*>(out);
        if (pa.fold) {
          // the earlier record stays unless this one is valid and strictly cheaper (a marker's cost_rd is the largest number).  In place the earlier
          // record is read through the output pointer: this lane reads it, then writes it
          const FhevcMotionRdPuNode* const src = reinterpret_cast<const void*>(pa.fold) == reinterpret_cast<const void*>(out) ? dst : reinterpret_cast<const FhevcMotionRdPuNode*>(pa.fold);
          const FhevcMotionRdPuNode f = src[rec];
          if (!(valid && u.cost_rd < f.cost_rd)) u = f;
        }
        dst[rec] = u;
      } else out[rec] = o;
    }
  }
}

// ---- the intra candidate on RD costs (fhevc_intra_rd_device): the first pass's lines, ONE mode per node, the transform passes above ----
//
// Per CTU: the CTU with its row above and column left staged over the (still dead) transform buffers, the 85 reference lines and their smoothed twins
// built exactly as k_firstpass.hip builds them (units, HM's substitution walk, smoothing, DC values; the lines keep their own LDS, the staged CTU is dead
// once the units are copied).  Then per TU depth: every lane predicts its tile at ITS node's mode from the line of the TU of that depth that holds the tile
// (the mode differs per lane, so nothing is wave-uniform but the TU size: negative angles project per sample, no extended reference is built), the residual
// against the original goes through rd_depth<DEPTH> unchanged.  The level-3 wave has no depth 1 (4x4 TUs are left out): it runs its depth-0 residual
// through the depth-1 passes and the writer drops the sums.  The writer lane makes HM's intra choice (dSplitCost < dSingleCost alone), applies the calm
// gate and the fold.  The matrices lie behind the transform buffers for the whole launch: nothing ever lies over them here.
namespace ird {
constexpr int kLineTotal = 257 + 4 * 129 + 16 * 65 + 64 * 33;  // 3 925 samples: all 85 lines of 4 n + 1
constexpr int kLinePad = 8;                                    // the unconditional second tap may touch one sample past a line
constexpr int kUnits = 65 + 4 * 33 + 16 * 17 + 64 * 9;         // 1 045 four-sample units (n + 1 per node: the corner is a unit)
// three TU depths: behind the matrices the sums per depth-1 TU and the DST (where rd_stage looks for them), then the unfiltered lines of the CTU's 256 4x4
// blocks (17 samples each, the corner at 8; a 4x4 block never takes the smoothed line) and their DC values -- which also take the second tap's one sample
// past the last line
constexpr int kLine4 = 17, kLines4At = kTransformShorts + kDstAt + kDstShorts, kDc4At = kLines4At + 256 * kLine4;
constexpr int kQtShorts = kFineShorts + kDstShorts + 256 * kLine4 + 256;   // 10 560 B
__device__ __forceinline__ int line_off(int level) { return level == 0 ? 0 : (level == 1 ? 257 : (level == 2 ? 773 : 1813)); }
__device__ __forceinline__ int node_off(int level) { return level == 0 ? 0 : (level == 1 ? 1 : (level == 2 ? 5 : 21)); }
__device__ __forceinline__ int unit_off(int level) { return level == 0 ? 0 : (level == 1 ? 65 : (level == 2 ? 197 : 469)); }
__device__ __forceinline__ int level_of_node(int k) { return k < 1 ? 0 : (k < 5 ? 1 : (k < 21 ? 2 : 3)); }
// unit u of a node at (x0, y0) of size n in HM's walk order: bottom-left first, up the left column, the corner, the row above left to right
__device__ __forceinline__ void unit_pos(int u, int n, int x0, int y0, int& ux, int& uy)
{
  const int L = n >> 1;
  if (u < L) { ux = x0 - 4; uy = y0 + 4 * (L - 1 - u); }
  else if (u == L) { ux = x0 - 4; uy = y0 - 4; }
  else { ux = x0 + 4 * (u - L - 1); uy = y0 - 4; }
}
// sample i of HM's refMain (TComPrediction.cpp:278-300) without the copy: i >= 0 lies on the main side, i < 0 is the side reference at the inverse angle
__device__ __forceinline__ int main_ref(const short* ref, int sgn, int inv_angle, int i)
{
  return ref[i >= 0 ? sgn * i : -sgn * ((128 - i * inv_angle) >> 8)];
}
// the tile at (bx, by) of the n x n TU (n = 1 << lg <= 32) whose line has its corner at ref[0] (above at +i, left at -i), predicted at mode 0..34 with the
// edge filters of n <= 16; tab: the angle and inverse-angle tables.  One sample at a time: the mode is this lane's own
// W, OX, OY (three TU depths, n = 4): the W x W samples go to (OX, OY) of the lane's tile -- one of the four 4x4 TUs it holds, each from its own line
template <int W = 8, int OX = 0, int OY = 0>
__device__ __forceinline__ void predict_tile(const short* ref, const short* tab, int n, int lg, int bx, int by, int mode, int dc, int maxval, unsigned (&P)[32])
{
  if (mode == 0) {
    const int topRight = ref[n + 1], bottomLeft = ref[-(n + 1)];
#pragma unroll
    for (int y = 0; y < W; ++y) {
      const int left = ref[-(by + y + 1)];
#pragma unroll
      for (int x = 0; x < W; ++x) {
        const int top = ref[bx + x + 1];
        const int hor = (left << lg) + n + (bx + x + 1) * (topRight - left);
        const int ver = (top << lg) + (by + y + 1) * (bottomLeft - top);
        const unsigned v = (unsigned)((hor + ver) >> (lg + 1)) & 0xFFFFu;
        if (x & 1) P[4 * (OY + y) + ((OX + x) >> 1)] |= v << 16; else P[4 * (OY + y) + ((OX + x) >> 1)] = v;
      }
    }
  } else if (mode == 1) {
    const bool edge = n <= 16;
#pragma unroll
    for (int y = 0; y < W; ++y)
#pragma unroll
      for (int x = 0; x < W; ++x) {
        const int X = bx + x, Y = by + y;
        int v = dc;
        if (edge && Y == 0) v = (ref[X + 1] + 3 * dc + 2) >> 2;
        if (edge && X == 0) v = (ref[-(Y + 1)] + 3 * dc + 2) >> 2;
        if (edge && X == 0 && Y == 0) v = (ref[1] + ref[-1] + 2 * dc + 2) >> 2;
        const unsigned w = (unsigned)v & 0xFFFFu;
        if (x & 1) P[4 * (OY + y) + ((OX + x) >> 1)] |= w << 16; else P[4 * (OY + y) + ((OX + x) >> 1)] = w;
      }
  } else {
    const bool is_ver = mode >= 18;
    const int ang_mode = is_ver ? mode - 26 : 10 - mode;
    const int abs_mode = abs(ang_mode);                      // 0..8: mode is 2..34
    const int angle = ang_mode < 0 ? -(int)tab[abs_mode] : (int)tab[abs_mode];
    const int inv_angle = tab[9 + abs_mode];
    const int sgn = is_ver ? 1 : -1;                         // main(i) = ref[sgn i], side(i) = ref[-sgn i]
    const bool edge = angle == 0 && n <= 16;                 // the pure vertical / horizontal modes: the first column (row) leans on the side reference
    const int tl = ref[0];
#pragma unroll
    for (int y = 0; y < W; ++y)
#pragma unroll
      for (int x = 0; x < W; ++x) {
        const int X = bx + x, Y = by + y;
        const int xx = is_ver ? X : Y, yy = is_ver ? Y : X;   // horizontal modes are the vertical ones of the transposed block
        const int delta = (yy + 1) * angle, di = delta >> 5, df = delta & 31;
        const int i = xx + di + 1;
        int v = ((32 - df) * main_ref(ref, sgn, inv_angle, i) + df * main_ref(ref, sgn, inv_angle, i + 1) + 16) >> 5;
        if (edge && xx == 0) v = min(maxval, max(0, v + ((ref[-sgn * (yy + 1)] - tl) >> 1)));
        const unsigned w = (unsigned)v & 0xFFFFu;
        if (x & 1) P[4 * (OY + y) + ((OX + x) >> 1)] |= w << 16; else P[4 * (OY + y) + ((OX + x) >> 1)] = w;
      }
  }
}
}  // namespace ird

// the NxN candidate's four PUs of the 8x8 node at (tx, ty) of CTU ctu: units (2 tx + (i & 1), 2 ty + (i >> 1)) of the 16x16 raster of the 4x4 first pass's
// records (satd, mode, ...).  Byte i is PU i's mode; where the node lies outside or a PU has the marker or a mode byte above 34 the candidate is invalid:
// all four 0 and bit 31 set.  No byte of the records reaches an address
__device__ __forceinline__ unsigned nxn_modes(const unsigned* __restrict__ first4, long long ctu, int tx, int ty, bool node_in)
{
  const unsigned* r4 = first4 + (ctu * 256 + (2 * ty) * 16 + 2 * tx) * 4;
  bool ok = node_in;
  unsigned m = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned* r = r4 + ((i >> 1) * 16 + (i & 1)) * 4;
    const unsigned sa = r[0], mo = r[1] & 0xFFu;
    ok = ok && sa != kRdMark && mo <= 34u;
    m |= mo << (8 * i);
  }
  return ok ? m : 0x80000000u;
}

// the candidate search: the record of a valid node at mode m from the sums as they stand -- what the writer lane of the instances of three TU depths makes of
// them, word for word (s_t: the transform buffers with the sums per depth-1 TU behind the matrices; nfirst, nbx, nby: the node's level's first node and its
// place in the level's raster); the answer is the unshifted J
__device__ __forceinline__ unsigned long long intra_search_record(const short* s_t, const unsigned* s_acc, const FhevcRdQuant& Q, int lvl, int nidx, int nfirst, int nbx, int nby, int m,
                                                                   FhevcMotionRdPuNode& u)
{
    const int qi = lvl == 3 ? 1 : (lvl == 2 ? 2 : 3);                // the depth-0 TU size's numbers
    const int tu0 = lvl == 0 ? 0 : (lvl == 1 ? 4 : lvl == 2 ? 8 : 24) + (nidx - nfirst), ntu = lvl == 0 ? 4 : 1;   // a 64x64 node: four TUs
    const unsigned side = intra_mode_bits((unsigned)m);
    unsigned long long j = (unsigned long long)Q.lam_q8 * side, bits = side;
    unsigned dist = 0, top = 0, any0 = 0, split = 0;
    if (lvl == 1 || lvl == 2) {
      // HM's intra recursion over three depths (TEncSearch.cpp:1610-1661), bottom-up: per depth-1 TU its own cost with its split flag against its four
      // children, then the depth-0 TU against the four results; dSplitCost < dSingleCost alone at both depths
      const unsigned lam = Q.lam_q8;
      const unsigned* const fine = reinterpret_cast<const unsigned*>(s_t + kTransformShorts + kFwdShorts + kInvShorts);
      const unsigned* a = &s_acc[kAccWords * tu0];
      const int e0 = lvl == 1 ? (2 * nby) * 4 + 2 * nbx : 16 + (2 * nby) * 8 + 2 * nbx, row = lvl == 1 ? 4 : 8;   // the node's first depth-1 TU
      const unsigned d0 = a[0], r0 = 1u + a[1];
      const unsigned long long j0 = 256ull * d0 + (unsigned long long)lam * (1u + r0);
      unsigned long long j1 = lam;
      unsigned dsub = 0, rsub = 0, s1 = 0;
      for (int i = 0; i < 4; ++i) {
        const unsigned* b = &fine[kFineWords * (e0 + (i >> 1) * row + (i & 1))];
        const unsigned d1 = b[0], r1 = 1u + b[1], d2 = b[2], r2 = 4u + b[3];
        const unsigned long long k1 = 256ull * d1 + (unsigned long long)lam * (1u + r1), k2 = 256ull * d2 + (unsigned long long)lam * (1u + r2);
        const bool take1 = k2 < k1;
        j1 += take1 ? k2 : k1; dsub += take1 ? d2 : d1; rsub += 1u + (take1 ? r2 : r1);
        s1 |= take1 ? 16u << i : 0u;
      }
      const bool take = j1 < j0;
      j += take ? j1 : j0; dist = take ? dsub : d0; bits += 1u + (take ? rsub : r0);
      split = take ? 1u | s1 : 0u; any0 = a[1]; top = a[4];
    } else
    for (int i = 0; i < ntu; ++i) {
      const unsigned* a = &s_acc[kAccWords * (tu0 + i)];
      const unsigned d0 = a[0], r0 = 1u + a[1], d1 = a[2], r1 = 4u + a[3];
      const unsigned long long j0 = 256ull * d0 + (unsigned long long)Q.lam_q8 * (1u + r0), j1 = 256ull * d1 + (unsigned long long)Q.lam_q8 * (1u + r1);
      const bool take = j1 < j0;                  // dSplitCost < dSingleCost alone (TEncSearch.cpp:1661)
      j += take ? j1 : j0; dist += take ? d1 : d0; bits += 1u + (take ? r1 : r0);
      split |= take ? 1u << i : 0u; any0 |= a[1]; top = max(top, a[4]);
    }
    const bool zero_half = ((top * Q.scale + Q.add_half[qi]) >> Q.qbits[qi]) == 0u;
    const unsigned long long unshifted = j;
    j >>= 8;
    u.dist = dist; u.cost_rd = j < 0xFFFFFFFEull ? (unsigned)j : 0xFFFFFFFEu;
    u.bits = (uint16_t)(bits < 65535ull ? bits : 65535ull);
    u.flags = (uint8_t)((any0 == 0u ? 1 : 0) | (zero_half ? 2 : 0) | (split ? 4 : 0)); u.tu_split = (uint8_t)split;
    u.part = kRdPartIntra; u.pad[0] = (uint8_t)m;
    return unshifted;
}

// T = int16_t or uint8_t planes.  first: the first pass's records as dwords (satd, mode, the cost's two); fold / rd_merge: RD records as dwords, or null;
// fold may be out (the writer lane reads its record, then writes it)
// Three TU depths (fhevc_intra_rd_qt* at tu_depths 3): RdThreeDepths as the pack -- the 32x32 and 16x16 nodes get their third TU size, the 8x8 nodes their
// depth 1, every 4x4 TU the DST.  With the empty pack the instances are the ones there always were, by code
// The NxN candidate (fhevc_intra_rd_nxn*): RdNxN BEHIND RdThreeDepths -- in the third pass, where the level-3 buffer is idle, the level-3 wave predicts the
// four 4x4 blocks of its tile each at ITS mode of the 4x4 first pass; the pass over that buffer at 4 with the DST gives the candidate's sums per 8x8 node,
// and the writer lane of an 8x8 node takes NxN where it is strictly cheaper than its 2Nx2N record (or that one is invalid), before the gate and the fold
template <typename T, class... A>
__global__ __launch_bounds__(256) void fhevc_intra_rd_kernel(FhevcFrames F, FhevcRdQuant Q, const unsigned* __restrict__ first, const unsigned* fold,
                                                             const unsigned* __restrict__ rd_merge, int skip_mask, FhevcMotionRdPuNode* out, A... tag)
{
  using namespace ird;
  constexpr bool QT = (std::is_same_v<A, RdThreeDepths> || ...);
  constexpr bool NXN = (std::is_same_v<A, RdNxN> || ...);
  constexpr bool SEARCH = (std::is_same_v<A, RdSearch> || ...);
  static_assert(sizeof...(A) == (QT ? 1 : 0) + (NXN ? 1 : 0) + (SEARCH ? 1 : 0) && (QT || !(NXN || SEARCH)) && !(NXN && SEARCH),
                "the pack is empty, the tag of three TU depths, or that tag and the NxN arguments or the search's behind it");
  // SEARCH: behind the sums the words of the search -- per 4x4 PU the sums of the position in hand (kPuWords) and its best so far (D, r | mode << 16, max |c|);
  // per node best and second of step A (the two A in 64 bits; mode and position of each in one word, mode 255: none) and F(best) with its unshifted J
  constexpr int kPuAt = kAccWords * kTus, kPuBestAt = kPuAt + kPuWords * 256, kNodeAt = kPuBestAt + 3 * 256, kRecAt = kNodeAt + 5 * FHEVC_NODES;
  constexpr int kSearchWords = kPuWords * 256 + 3 * 256 + 5 * FHEVC_NODES + 6 * FHEVC_NODES;   // 8 860 B: 80 532 B of static LDS in all
  // the transform buffers (under them, first, the staged CTU) and the matrices; QT: behind them the sums per depth-1 TU, the DST, the 4x4 lines and their DC values
  __shared__ __attribute__((aligned(16))) short s_t[kTransformShorts + kFwdShorts + kInvShorts + (QT ? kQtShorts : 0)];
  __shared__ short s_refbuf[kLinePad + kLineTotal + kLinePad + 1];   // unfiltered lines: line[2 n] the corner, + i above, - j left
  __shared__ short s_fltbuf[kLinePad + kLineTotal + kLinePad + 1];   // smoothed lines
  __shared__ short s_above[132], s_left[64], s_tab[18];
  __shared__ int s_dc[FHEVC_NODES];
  __shared__ unsigned char s_av[kUnits + 3], s_valid[FHEVC_NODES];
  __shared__ unsigned s_acc[kAccWords * kTus + (NXN ? kNxnWords * 64 : 0) + (SEARCH ? kSearchWords : 0)];   // NXN: behind the sums, the candidate's three words per 8x8 node
  static_assert(kTransformShorts >= 64 * 64, "the staged CTU lies under the transform buffers");
  short* const s_org = s_t;
  short* const s_ref = s_refbuf + kLinePad;
  short* const s_flt = s_fltbuf + kLinePad;
  const int tid = threadIdx.x, lane = tid & 63, lvl = tid >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(lvl);
  const int tx = lane & 7, ty = lane >> 3;
  const int bd = F.bit_depth, maxval = (1 << bd) - 1;
  const int band_rows = F.row_end - F.row_begin, per_frame = band_rows * F.ctus_x, total = per_frame * F.num_frames;
  const T* plane = reinterpret_cast<const T*>(F.luma);
  const RefineNode N(lvl, tx, ty);
  const int nidx = N.nidx;
  const int gw = F.width >> (6 - lvl), gh = F.height >> (6 - lvl);   // the level's nodes that lie wholly inside the picture
  {
    unsigned* mdst = reinterpret_cast<unsigned*>(s_t + kTransformShorts);
    const unsigned* msrc = reinterpret_cast<const unsigned*>(&kRdTables);
    for (int i = tid; i < (kFwdShorts + kInvShorts) / 2; i += 256) mdst[i] = msrc[i];
    if (tid < 9) {
      const int ang[9] = { 0, 2, 5, 9, 13, 17, 21, 26, 32 }, inv[9] = { 0, 4096, 1638, 910, 630, 482, 390, 315, 256 };
      int a = 0, b = 0;
#pragma unroll
      for (int k = 0; k < 9; ++k) { a = tid == k ? ang[k] : a; b = tid == k ? inv[k] : b; }
      s_tab[tid] = (short)a; s_tab[9 + tid] = (short)b;
    }
    if constexpr (QT)
      if (tid < kDstShorts / 2) mdst[kDstAt / 2 + tid] = reinterpret_cast<const unsigned*>(&kDstTables)[tid];
  }

  for (int work = blockIdx.x; work < total; work += gridDim.x) {
    const int f = work / per_frame, rem = work - f * per_frame;
    const int cy = F.row_begin + rem / F.ctus_x, cx = rem % F.ctus_x;
    const long long base = (long long)f * F.frame_stride;
    const T* frame = plane + base;
    const int ox = cx * 64, oy = cy * 64;
    const long long rec = ((long long)(f * band_rows + (cy - F.row_begin)) * F.ctus_x + cx) * FHEVC_NODES + nidx;
    // ---- the node's input record: satd and the low byte of mode; nothing of it reaches an address ----
    const bool node_in = cx * N.ncnt + N.nbx < gw && cy * N.ncnt + N.nby < gh;
    unsigned rsatd = kRdMark, rmode = 0;   // SEARCH: there are no records -- the modes come from the lists, position by position, and validity with them
    if constexpr (!SEARCH) { rsatd = first[rec * 4]; rmode = first[rec * 4 + 1] & 0xFFu; }
    const bool valid = node_in && rsatd != kRdMark && rmode <= 34u;
    const int mode = valid ? (int)rmode : 0;   // an invalid node predicts with mode 0 and drops the result
    __syncthreads();   // the previous CTU's readers of the buffers and of the sums are done
    // ---- the CTU, the row above it and the column left of it; which of the 85 nodes lie inside ----
    fhevc_fp::stage_ctu<T>(frame, F, ox, oy, tid, s_org, s_above, s_left);
    if (tid < FHEVC_NODES) {
      const int level = level_of_node(tid), n = 64 >> level, cnt = 1 << level, ni = tid - node_off(level);
      s_valid[tid] = ((ox + (ni % cnt) * n + n <= F.width) && (oy + (ni / cnt) * n + n <= F.height)) ? 1 : 0;
    }
    for (int i = tid; i < kAccWords * kTus; i += 256) s_acc[i] = 0;
    if constexpr (NXN)
      if (tid < kNxnWords * 64) s_acc[kAccWords * kTus + tid] = 0;
    if constexpr (SEARCH) {
      s_acc[kPuBestAt + 3 * tid] = 0u; s_acc[kPuBestAt + 3 * tid + 1] = 255u << 16; s_acc[kPuBestAt + 3 * tid + 2] = 0u;   // no PU has a mode yet
      if (tid < FHEVC_NODES) s_acc[kNodeAt + 5 * tid + 4] = 0x00FF00FFu;                                                  // ... and no node a best or a second
    }
    if constexpr (QT)
      for (int i = tid; i < kFineTus * kFineWords; i += 256) reinterpret_cast<unsigned*>(s_t + kTransformShorts + kFwdShorts + kInvShorts)[i] = 0u;
    __syncthreads();
    if constexpr (QT) {
      // ---- one thread per 4x4 block of the CTU: its five units in HM's walk order (below left, left, the corner, above, above right) with z-order
      // availability in 4-sample units, the substitution walk and the DC value -- what fhevc_intra_first_pass_4x4 evaluates for the block
      const int x0 = ox + (tid & 15) * 4, y0 = oy + (tid >> 4) * 4;
      if (x0 + 4 <= F.width && y0 + 4 <= F.height) {
        short* line = s_t + kLines4At + tid * kLine4;
        bool av[5];
        int first_av = -1;
#pragma unroll
        for (int u = 4; u >= 0; --u) {
          int ux, uy;
          unit_pos(u, 4, x0, y0, ux, uy);
          av[u] = fhevc_fp::unit_available(ux, uy, x0, y0, F.width, F.height, F.ctus_x);
          if (av[u]) {
            first_av = u;
            if (u == 2) line[8] = fhevc_fp::staged(s_org, s_above, s_left, x0 - 1, y0 - 1, ox, oy);
            else {
#pragma unroll
              for (int i = 0; i < 4; ++i)
                line[u < 2 ? 4 * u + i : 4 * u - 3 + i] = u < 2 ? fhevc_fp::staged(s_org, s_above, s_left, x0 - 1, y0 + 7 - (4 * u + i), ox, oy)
                                                                : fhevc_fp::staged(s_org, s_above, s_left, x0 + 4 * (u - 3) + i, y0 - 1, ox, oy);
            }
          }
        }
        if (first_av < 0) {
#pragma unroll
          for (int i = 0; i < kLine4; ++i) line[i] = (short)(1 << (bd - 1));
        } else {
          short prev = line[first_av <= 2 ? 4 * first_av : 4 * first_av - 3];
#pragma unroll
          for (int u = 0; u < 5; ++u) {
            const int s = u <= 2 ? 4 * u : 4 * u - 3, c = u == 2 ? 1 : 4;
            if (av[u]) prev = line[s + c - 1];
            else for (int i = 0; i < c; ++i) line[s + i] = prev;
          }
        }
        int sum = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) sum += line[9 + i] + line[7 - i];
        s_t[kDc4At + tid] = (short)((sum + 4) >> 3);
      }
    }
    // ---- one thread per 4-sample unit: availability in coding order and, where available, its samples ----
    for (int ug = 65 + tid; ug < kUnits; ug += 256) {   // from the first unit of level 1 on: a 64x64 block is no TU
      const int level = ug < 197 ? 1 : (ug < 469 ? 2 : 3);
      const int n = 64 >> level, cnt = 1 << level, upn = n + 1;
      const int ni = (ug - unit_off(level)) / upn, u = (ug - unit_off(level)) - ni * upn;
      const int x0 = ox + (ni % cnt) * n, y0 = oy + (ni / cnt) * n;
      int ux, uy;
      unit_pos(u, n, x0, y0, ux, uy);
      const bool av = s_valid[node_off(level) + ni] && fhevc_fp::unit_available(ux, uy, x0, y0, F.width, F.height, F.ctus_x);
      s_av[ug] = av ? 1 : 0;
      if (av) {
        short* line = s_ref + line_off(level) + ni * (4 * n + 1);
        const int L = n >> 1;
        if (u < L) {
#pragma unroll
          for (int i = 0; i < 4; ++i) line[4 * u + i] = fhevc_fp::staged(s_org, s_above, s_left, x0 - 1, y0 + 2 * n - 1 - (4 * u + i), ox, oy);
        } else if (u == L) {
          line[2 * n] = fhevc_fp::staged(s_org, s_above, s_left, x0 - 1, y0 - 1, ox, oy);
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) line[4 * u - 3 + i] = fhevc_fp::staged(s_org, s_above, s_left, x0 + 4 * (u - L - 1) + i, y0 - 1, ox, oy);
        }
      }
    }
    __syncthreads();
    // ---- HM's substitution walk (TComPattern.cpp:461-524), one thread per node ----
    if (tid >= 1 && tid < FHEVC_NODES && s_valid[tid]) {
      const int level = level_of_node(tid), n = 64 >> level, ni = tid - node_off(level), upn = n + 1, L = n >> 1;
      short* line = s_ref + line_off(level) + ni * (4 * n + 1);
      const unsigned char* av = s_av + unit_off(level) + ni * upn;
      int first_av = -1;
      for (int u = 0; u < upn && first_av < 0; ++u) if (av[u]) first_av = u;
      if (first_av < 0) {
        for (int i = 0; i < 4 * n + 1; ++i) line[i] = (short)(1 << (bd - 1));
      } else {
        short prev = line[first_av <= L ? 4 * first_av : 4 * first_av - 3];
        for (int u = 0; u < upn; ++u) {
          const int s = u <= L ? 4 * u : 4 * u - 3, c = (u == L) ? 1 : 4;
          if (av[u]) prev = line[s + c - 1];
          else for (int i = 0; i < c; ++i) line[s + i] = prev;
        }
      }
    }
    __syncthreads();
    // ---- the smoothed lines (one thread per sample; level 0 is no TU size and is left out) and the DC values ----
#pragma unroll
    for (int level = 1; level < 4; ++level) {
      const int n = 64 >> level, len = 4 * n + 1, cnt = (1 << (2 * level)) * len;
      for (int i = tid; i < cnt; i += 256) {
        const int ni = i / len, k = i - ni * len;
        if (!s_valid[node_off(level) + ni]) continue;
        const short* ref = s_ref + line_off(level) + ni * len;
        int v;
        if (k == 0 || k == 4 * n) v = ref[k];
        else {
          bool strong = false;
          if (n >= 32) {
            const int thr = 1 << (bd - 5);
            const int bl = ref[0], tl = ref[2 * n], tr = ref[4 * n];
            strong = (abs(bl + tl - 2 * ref[n]) < thr) && (abs(tl + tr - 2 * ref[3 * n]) < thr);
            if (strong) {
              if (k < 2 * n) v = ((2 * n - k) * bl + k * tl + n) >> 6;
              else if (k == 2 * n) v = tl;
              else v = ((2 * n - (k - 2 * n)) * tl + (k - 2 * n) * tr + n) >> 6;
            }
          }
          if (!strong) v = (ref[k - 1] + 2 * ref[k] + ref[k + 1] + 2) >> 2;
        }
        s_flt[line_off(level) + i] = (short)v;
      }
    }
    if (tid >= 1 && tid < FHEVC_NODES && s_valid[tid]) {
      const int level = level_of_node(tid), n = 64 >> level, ni = tid - node_off(level);
      const short* ref = s_ref + line_off(level) + ni * (4 * n + 1);   // DC never uses the smoothed line
      int sum = 0;
      for (int i = 0; i < n; ++i) sum += ref[2 * n + 1 + i] + ref[2 * n - 1 - i];
      s_dc[tid] = (sum + n) >> (7 - level);                            // / (2 n)
    }
    const int px = ox + tx * 8, py = oy + ty * 8;
    const bool inside = (px + 8 <= F.width) && (py + 8 <= F.height);
    __syncthreads();   // the lines stand; the staged CTU is dead: the transform buffers lie over it
    // ---- per TU depth: this lane's tile predicted at its node's mode from the line of the TU that holds it, the residual through the passes ----
    // ---- SEARCH: what the rule gives this launch (uniform) and this wave; the positions of the 4x4 PUs' lists, in passes of their own over the level-3 buffer ----
    int npos = 0, runs = 1, my_count = 0;
    if constexpr (SEARCH) {
      const RdSearch S = (tag, ...);   // the pack's last argument
      const int c0 = S.counts & 0xFF, c1 = (S.counts >> 8) & 0xFF, c2 = (S.counts >> 16) & 0xFF, c3 = S.counts >> 24;
      npos = max(max(c0, c1), max(c2, c3)) + S.append;   // 9 at the most
      runs = npos > 1 ? 2 : 1;                           // one position: nothing can be second
      my_count = wave == 0 ? c0 : wave == 1 ? c1 : wave == 2 ? c2 : c3;
      const int n4 = S.modes4 ? S.count4 + S.append : 0;
      const long long ctu = (long long)(f * band_rows + (cy - F.row_begin)) * F.ctus_x + cx;   // compact over the band
#pragma unroll 1
      for (int pos = 0; pos < n4; ++pos) {
        unsigned D[32], m4 = 0;
#pragma unroll
        for (int i = 0; i < 32; ++i) D[i] = 0u;
        if (wave == 3) {
          const unsigned char* const e4 = S.modes4 + (ctu * 256 + (2 * ty) * 16 + 2 * tx) * S.stride4;
#pragma unroll
          for (int i = 0; i < 4; ++i) m4 |= search_cand(e4 + ((i >> 1) * 16 + (i & 1)) * S.stride4, S.count4, S.append, pos) << (8 * i);
          const short* l4 = s_t + kLines4At + ((2 * ty) * 16 + 2 * tx) * kLine4 + 8;
          const short* d4 = s_t + kDc4At + (2 * ty) * 16 + 2 * tx;
          const auto pm = [&](int i) { const unsigned m = (m4 >> (8 * i)) & 0xFFu; return m <= 34u ? (int)m : 0; };   // a PU without a candidate here predicts with mode 0
          predict_tile<4, 0, 0>(l4, s_tab, 4, 2, 0, 0, pm(0), d4[0], maxval, D);
          predict_tile<4, 4, 0>(l4 + kLine4, s_tab, 4, 2, 0, 0, pm(1), d4[1], maxval, D);
          predict_tile<4, 0, 4>(l4 + 16 * kLine4, s_tab, 4, 2, 0, 0, pm(2), d4[16], maxval, D);
          predict_tile<4, 4, 4>(l4 + 17 * kLine4, s_tab, 4, 2, 0, 0, pm(3), d4[17], maxval, D);
          unsigned O[32];
          load_tile8x8(plane, base, F, px, py, inside, O);
#pragma unroll
          for (int i = 0; i < 32; ++i) D[i] = pk_sub(O[i], D[i]);
        }
        unsigned sse[4];
        rd_pu_pass(s_t, lane, wave, tx, ty, Q, &s_acc[kPuAt], plane, base, F, px, py, inside, D, sse);
        if (wave == 3) {
          // per PU: 256 D + lam (r + bits(m)) against its best so far, strictly below in list order; r = 1 + the level bits
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int unit = (2 * ty + (i >> 1)) * 16 + 2 * tx + (i & 1);
            const unsigned m = (m4 >> (8 * i)) & 0xFFu, lv = s_acc[kPuAt + kPuWords * unit], top = s_acc[kPuAt + kPuWords * unit + 1];
            unsigned* const pb = &s_acc[kPuBestAt + 3 * unit];
            const unsigned bm = (pb[1] >> 16) & 0xFFu, blv = pb[1] & 0xFFFFu;
            const unsigned side = intra_mode_bits(m), bside = intra_mode_bits(bm);
            const unsigned long long j = 256ull * sse[i] + (unsigned long long)Q.lam_q8 * (1u + lv + side), jb = 256ull * pb[0] + (unsigned long long)Q.lam_q8 * (1u + blv + bside);
            if (node_in && m <= 34u && (bm == 255u || j < jb)) { pb[0] = sse[i]; pb[1] = lv | m << 16; pb[2] = top; }
          }
        }
      }
    }
#pragma unroll 1
    for (int ph = 0; ph < (SEARCH ? npos + 3 * runs : QT ? 3 : 2); ++ph) {
      int depth = ph, md = mode;
      [[maybe_unused]] int run = 0, pos = 0;        // SEARCH: the phases are the positions of step A (depth 0 alone), then the three depths at the best and at the second mode
      [[maybe_unused]] unsigned cand = 255u;
      if constexpr (SEARCH) {
        const RdSearch S = (tag, ...);
        const bool step_a = ph < npos;
        run = step_a ? 0 : (ph - npos >= 3 ? 1 : 0);
        depth = step_a ? 0 : ph - npos - 3 * run;
        pos = step_a ? ph : -1;
        if (step_a) {
          const long long ctu = (long long)(f * band_rows + (cy - F.row_begin)) * F.ctus_x + cx;
          cand = search_cand(S.modes + (ctu * FHEVC_NODES + nidx) * S.stride, my_count, S.append, ph);
          md = cand <= 34u ? (int)cand : 0;   // a node without a candidate here predicts with mode 0 and drops the result
        } else {
          if (depth == 0) {
            __syncthreads();   // the writer lanes' words of step A (of the first run) stand; the sums are read
            if (run == 1) {
              for (int i = tid; i < kAccWords * kTus; i += 256) s_acc[i] = 0;
              for (int i = tid; i < kFineTus * kFineWords; i += 256) reinterpret_cast<unsigned*>(s_t + kTransformShorts + kFwdShorts + kInvShorts)[i] = 0u;
              __syncthreads();
            }
          }
          const unsigned m = (s_acc[kNodeAt + 5 * nidx + 4] >> (16 * run)) & 0xFFu;
          md = m <= 34u ? (int)m : 0;
        }
      }
      const int L = min(max(wave, 1) + depth, 3);        // the TU's level (wave 3 has no depth 1: its depth-0 TU again, dropped by the writer)
      const bool four = QT && max(wave, 1) + depth == 4;  // three depths: the 4x4 TUs, four to a tile, each with its own line -- L is not used then
      const int n = 64 >> L, lg = 6 - L;
      const int ni = ((ty >> (3 - L)) << L) + (tx >> (3 - L));
      const int bx = (tx * 8) & (n - 1), by = (ty * 8) & (n - 1);
      const int thr = L == 1 ? 0 : (L == 2 ? 1 : 7);     // m_aucIntraFilter of 32, 16, 8
      const bool use_flt = md != 1 && min(abs(md - 10), abs(md - 26)) > thr;
      const short* ref = (use_flt ? s_flt : s_ref) + line_off(L) + ni * (4 * n + 1) + 2 * n;
      unsigned D[32];
      if (QT && depth == 2 && wave != 1 && wave != 2) {
        // the 64x64 and the 8x8 nodes have no third depth: rd_depth<2> keeps their waves at the barriers and reads no residual
#pragma unroll
        for (int i = 0; i < 32; ++i) D[i] = 0u;
      } else if (four) {
        const short* l4 = s_t + kLines4At + ((2 * ty) * 16 + 2 * tx) * kLine4 + 8;   // the tile's first 4x4 block: its line's corner
        const short* d4 = s_t + kDc4At + (2 * ty) * 16 + 2 * tx;
        predict_tile<4, 0, 0>(l4, s_tab, 4, 2, 0, 0, md, d4[0], maxval, D);
        predict_tile<4, 4, 0>(l4 + kLine4, s_tab, 4, 2, 0, 0, md, d4[1], maxval, D);
        predict_tile<4, 0, 4>(l4 + 16 * kLine4, s_tab, 4, 2, 0, 0, md, d4[16], maxval, D);
        predict_tile<4, 4, 4>(l4 + 17 * kLine4, s_tab, 4, 2, 0, 0, md, d4[17], maxval, D);
      } else
      predict_tile(ref, s_tab, n, lg, bx, by, md, s_dc[node_off(L) + ni], maxval, D);
      if (!(QT && depth == 2 && wave != 1 && wave != 2)) {
        unsigned O[32];
        load_tile8x8(plane, base, F, px, py, inside, O);
#pragma unroll
        for (int i = 0; i < 32; ++i) D[i] = pk_sub(O[i], D[i]);
      }
      if constexpr (NXN) {
        if (depth == 2 && wave == 3) {
          // the level-3 buffer is idle in the third pass: the NxN candidate runs there -- the four 4x4 blocks of the lane's tile, each at ITS mode of the
          // 4x4 first pass from its own line, as the `four` branch predicts them at the node's one mode
          const unsigned m4 = nxn_modes((tag, ...).first4, ((long long)(f * band_rows + (cy - F.row_begin)) * F.ctus_x + cx), tx, ty, node_in);
          const short* l4 = s_t + kLines4At + ((2 * ty) * 16 + 2 * tx) * kLine4 + 8;
          const short* d4 = s_t + kDc4At + (2 * ty) * 16 + 2 * tx;
          predict_tile<4, 0, 0>(l4, s_tab, 4, 2, 0, 0, (int)(m4 & 0x7Fu), d4[0], maxval, D);
          predict_tile<4, 4, 0>(l4 + kLine4, s_tab, 4, 2, 0, 0, (int)((m4 >> 8) & 0xFFu), d4[1], maxval, D);
          predict_tile<4, 0, 4>(l4 + 16 * kLine4, s_tab, 4, 2, 0, 0, (int)((m4 >> 16) & 0xFFu), d4[16], maxval, D);
          predict_tile<4, 4, 4>(l4 + 17 * kLine4, s_tab, 4, 2, 0, 0, (int)((m4 >> 24) & 0x7Fu), d4[17], maxval, D);
          unsigned O[32];
          load_tile8x8(plane, base, F, px, py, inside, O);
#pragma unroll
          for (int i = 0; i < 32; ++i) D[i] = pk_sub(O[i], D[i]);
        }
      }
      if (depth == 0) rd_depth<0, T, QT, QT>(s_t, lane, lvl, wave, tx, ty, Q, s_acc, plane, base, F, px, py, inside, D);
      else if (!QT || depth == 1) rd_depth<1, T, QT, QT>(s_t, lane, lvl, wave, tx, ty, Q, s_acc, plane, base, F, px, py, inside, D);
      else if constexpr (QT) rd_depth<2, T, QT, QT, NXN>(s_t, lane, lvl, wave, tx, ty, Q, s_acc, plane, base, F, px, py, inside, D);
      if constexpr (SEARCH) {
        if (N.writer) {
          unsigned* const nw = &s_acc[kNodeAt + 5 * nidx];
          unsigned* const rw = &s_acc[kRecAt + 6 * nidx];
          if (pos >= 0) {
            // step A (bCheckFirst): A_c = the depth-0 TUs' J0 + lam bits(m_c); best and second as HM keeps them.  The sums that the next position adds
            // to are cleared here, by the lane that read them (the distortion is a plain store)
            const int tu0 = lvl == 0 ? 0 : (lvl == 1 ? 4 : lvl == 2 ? 8 : 24) + (nidx - N.first), ntu = lvl == 0 ? 4 : 1;
            unsigned long long a_c = (unsigned long long)Q.lam_q8 * intra_mode_bits((unsigned)md);
            for (int i = 0; i < ntu; ++i) {
              unsigned* const a = &s_acc[kAccWords * (tu0 + i)];
              a_c += 256ull * a[0] + (unsigned long long)Q.lam_q8 * (2u + a[1]);
              a[1] = 0u; a[4] = 0u;
            }
            if (node_in && cand <= 34u) {
              const unsigned info = nw[4];
              const unsigned long long best = (unsigned long long)nw[1] << 32 | nw[0], second = (unsigned long long)nw[3] << 32 | nw[2];
              const unsigned me = cand | (unsigned)pos << 8;
              if ((info & 0xFFu) == 255u || a_c < best) {   // strictly below the best: it becomes the best and the old best the second
                nw[2] = nw[0]; nw[3] = nw[1]; nw[0] = (unsigned)a_c; nw[1] = (unsigned)(a_c >> 32); nw[4] = me | info << 16;
              } else if (((info >> 16) & 0xFFu) == 255u || a_c < second) {   // otherwise strictly below the second: it becomes the second
                nw[2] = (unsigned)a_c; nw[3] = (unsigned)(a_c >> 32); nw[4] = (info & 0xFFFFu) | me << 16;
              }
            }
          } else if (depth == 2) {
            // step B: F(best) is kept with its unshifted J; F(second) takes its place iff there is a second and its J is strictly smaller
            const unsigned who = (nw[4] >> (16 * run)) & 0xFFFFu;
            FhevcMotionRdPuNode r;
            r.dist = r.cost_rd = kRdMark; r.bits = 0xFFFFu; r.flags = 0; r.tu_split = 0; r.part = 255; r.merged = 0; r.pad[0] = r.pad[1] = 0;
            unsigned long long j = ~0ull;
            if (node_in && (who & 0xFFu) <= 34u) { j = intra_search_record(s_t, s_acc, Q, lvl, nidx, N.first, N.nbx, N.nby, (int)(who & 0xFFu), r); r.pad[1] = (uint8_t)(who >> 8); }
            const unsigned long long kept = (unsigned long long)rw[5] << 32 | rw[4];
            if (run == 0 || j < kept) {   // a node without a second has all ones there: below nothing
              unsigned w[4];
              __builtin_memcpy(w, &r, 16);
              rw[0] = w[0]; rw[1] = w[1]; rw[2] = w[2]; rw[3] = w[3]; rw[4] = (unsigned)j; rw[5] = (unsigned)(j >> 32);
            }
          }
        }
      }
    }
    if (N.writer) {
      FhevcMotionRdPuNode u;
      u.dist = u.cost_rd = kRdMark; u.bits = 0xFFFFu; u.flags = 0; u.tu_split = 0; u.part = 255; u.merged = 0; u.pad[0] = u.pad[1] = 0;
      const FhevcMotionRdPuNode none = u;
      if constexpr (SEARCH) {
        unsigned w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = s_acc[kRecAt + 6 * nidx + i];
        __builtin_memcpy(&u, w, 16);   // the marker where the node lies outside or its list is empty
      } else
      // (intra_search_record above is this block at three depths, word for word, for the search instances: a change here is a change there)
      if (valid) {
        const int qi = lvl == 3 ? 1 : (lvl == 2 ? 2 : 3);                // the depth-0 TU size's numbers
        const int tu0 = lvl == 0 ? 0 : (lvl == 1 ? 4 : lvl == 2 ? 8 : 24) + (nidx - N.first), ntu = lvl == 0 ? 4 : 1;   // a 64x64 node: four TUs
        const unsigned side = mode == 0 ? 2u : (mode == 1 || mode == 26) ? 3u : 6u;   // bits(m) of fhevc_intra_p
        unsigned long long j = (unsigned long long)Q.lam_q8 * side, bits = side;
        unsigned dist = 0, top = 0, any0 = 0, split = 0;
        if (QT && (lvl == 1 || lvl == 2)) {
          // HM's intra recursion over three depths (TEncSearch.cpp:1610-1661), bottom-up: per depth-1 TU its own cost with its split flag against its four
          // children, then the depth-0 TU against the four results; dSplitCost < dSingleCost alone at both depths
          const unsigned lam = Q.lam_q8;
          const unsigned* const fine = reinterpret_cast<const unsigned*>(s_t + kTransformShorts + kFwdShorts + kInvShorts);
          const unsigned* a = &s_acc[kAccWords * tu0];
          const int e0 = lvl == 1 ? (2 * N.nby) * 4 + 2 * N.nbx : 16 + (2 * N.nby) * 8 + 2 * N.nbx, row = lvl == 1 ? 4 : 8;   // the node's first depth-1 TU
          const unsigned d0 = a[0], r0 = 1u + a[1];
          const unsigned long long j0 = 256ull * d0 + (unsigned long long)lam * (1u + r0);
          unsigned long long j1 = lam;
          unsigned dsub = 0, rsub = 0, s1 = 0;
          for (int i = 0; i < 4; ++i) {
            const unsigned* b = &fine[kFineWords * (e0 + (i >> 1) * row + (i & 1))];
            const unsigned d1 = b[0], r1 = 1u + b[1], d2 = b[2], r2 = 4u + b[3];
            const unsigned long long k1 = 256ull * d1 + (unsigned long long)lam * (1u + r1), k2 = 256ull * d2 + (unsigned long long)lam * (1u + r2);
            const bool take1 = k2 < k1;
            j1 += take1 ? k2 : k1; dsub += take1 ? d2 : d1; rsub += 1u + (take1 ? r2 : r1);
            s1 |= take1 ? 16u << i : 0u;
          }
          const bool take = j1 < j0;
          j += take ? j1 : j0; dist = take ? dsub : d0; bits += 1u + (take ? rsub : r0);
          split = take ? 1u | s1 : 0u; any0 = a[1]; top = a[4];
        } else
        for (int i = 0; i < ntu; ++i) {
          const unsigned* a = &s_acc[kAccWords * (tu0 + i)];
          const unsigned d0 = a[0], r0 = 1u + a[1], d1 = a[2], r1 = 4u + a[3];
          const unsigned long long j0 = 256ull * d0 + (unsigned long long)Q.lam_q8 * (1u + r0), j1 = 256ull * d1 + (unsigned long long)Q.lam_q8 * (1u + r1);
          const bool take = (QT || lvl != 3) && j1 < j0;                  // dSplitCost < dSingleCost alone (TEncSearch.cpp:1661); at two depths an 8x8 node has one depth
          j += take ? j1 : j0; dist += take ? d1 : d0; bits += 1u + (take ? r1 : r0);
          split |= take ? 1u << i : 0u; any0 |= a[1]; top = max(top, a[4]);
        }
        const bool zero_half = ((top * Q.scale + Q.add_half[qi]) >> Q.qbits[qi]) == 0u;
        j >>= 8;
        u.dist = dist; u.cost_rd = j < 0xFFFFFFFEull ? (unsigned)j : 0xFFFFFFFEu;
        u.bits = (uint16_t)(bits < 65535ull ? bits : 65535ull);
        u.flags = (uint8_t)((any0 == 0u ? 1 : 0) | (zero_half ? 2 : 0) | (split ? 4 : 0)); u.tu_split = (uint8_t)split;
        u.part = kRdPartIntra; u.pad[0] = (uint8_t)mode;
      }
      if constexpr (NXN) {
        if (lvl == 3) {
          // the NxN candidate: four 4x4 TUs, each with its cbf bit and its mode's bits, no split flag (HM infers it); its own record whatever becomes of it,
          // and the node's record where it is strictly cheaper than 2Nx2N (a marker there loses to anything)
          const RdNxN X = (tag, ...);   // the pack's last argument
          const long long ctu = (long long)(f * band_rows + (cy - F.row_begin)) * F.ctus_x + cx;   // compact over the band
          const unsigned modes4 = nxn_modes(X.first4, ctu, tx, ty, node_in);   // read a second time (from the cache): nothing of it is kept through the passes
          const bool nv = (modes4 >> 31) == 0u;
          const unsigned* const w = &s_acc[kAccWords * kTus + kNxnWords * (nidx - N.first)];
          unsigned side4 = 0;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const unsigned m = (modes4 >> (8 * i)) & 0xFFu;
            side4 += m == 0u ? 2u : (m == 1u || m == 26u) ? 3u : 6u;
          }
          const unsigned nd = w[0], lv = w[1] & 0xFFFFu, cbf = w[1] >> 16, nb = 4u + lv + side4;
          unsigned long long nj = (256ull * nd + (unsigned long long)Q.lam_q8 * nb) >> 8;
          const unsigned nc = nj < 0xFFFFFFFEull ? (unsigned)nj : 0xFFFFFFFEu;
          const unsigned nf = (lv == 0u ? 1u : 0u) | (((w[2] * Q.scale + Q.add_half[0]) >> Q.qbits[0]) == 0u ? 2u : 0u) | 4u;
          if (X.nxn) {
            unsigned* const o = X.nxn + (ctu * 64 + (nidx - N.first)) * 4;
            o[0] = nv ? nd : kRdMark; o[1] = nv ? nc : kRdMark;
            o[2] = nv ? (nb < 65535u ? nb : 65535u) | nf << 16 | cbf << 24 : 0xFFFFu;
            o[3] = nv ? modes4 : 0xFFFFFFFFu;
          }
          if (nv && nc < u.cost_rd) {
            u.dist = nd; u.cost_rd = nc; u.bits = (uint16_t)(nb < 65535u ? nb : 65535u); u.flags = (uint8_t)nf; u.tu_split = 1;
            u.part = kRdPartIntraNxN; u.merged = 0; u.pad[0] = u.pad[1] = 0;
          }
        }
      }
      if constexpr (SEARCH) {
        const RdSearch S = (tag, ...);
        if (lvl == 3 && S.modes4) {
          // the NxN candidate over the four PUs' chosen modes: the record of the NxN instances, from the words per PU (a PU priced alone is the PU priced with
          // its three neighbours: every line is the original's); valid iff the node lies inside and every PU has a mode
          const long long ctu = (long long)(f * band_rows + (cy - F.row_begin)) * F.ctus_x + cx;   // compact over the band
          unsigned nd = 0, lv = 0, cbf = 0, top = 0, side4 = 0, modes4 = 0;
          bool nv = node_in;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const unsigned* const pb = &s_acc[kPuBestAt + 3 * ((2 * ty + (i >> 1)) * 16 + 2 * tx + (i & 1))];
            const unsigned m = (pb[1] >> 16) & 0xFFu, l = pb[1] & 0xFFFFu;
            nv = nv && m <= 34u;
            nd += pb[0]; lv += l; cbf |= l != 0u ? 1u << i : 0u; top = max(top, pb[2]); modes4 |= m << (8 * i);
            side4 += intra_mode_bits(m);
          }
          const unsigned nb = 4u + lv + side4;
          unsigned long long nj = (256ull * nd + (unsigned long long)Q.lam_q8 * nb) >> 8;
          const unsigned nc = nj < 0xFFFFFFFEull ? (unsigned)nj : 0xFFFFFFFEu;
          const unsigned nf = (lv == 0u ? 1u : 0u) | (((top * Q.scale + Q.add_half[0]) >> Q.qbits[0]) == 0u ? 2u : 0u) | 4u;
          if (S.nxn) {
            unsigned* const o = S.nxn + (ctu * 64 + (nidx - N.first)) * 4;
            o[0] = nv ? nd : kRdMark; o[1] = nv ? nc : kRdMark;
            o[2] = nv ? (nb < 65535u ? nb : 65535u) | nf << 16 | cbf << 24 : 0xFFFFu;
            o[3] = nv ? modes4 : 0xFFFFFFFFu;
          }
          if (nv && nc < u.cost_rd) {
            u.dist = nd; u.cost_rd = nc; u.bits = (uint16_t)(nb < 65535u ? nb : 65535u); u.flags = (uint8_t)nf; u.tu_split = 1;
            u.part = kRdPartIntraNxN; u.merged = 0; u.pad[0] = u.pad[1] = 0;
          }
        }
      }
      // the earlier record (a marker where there is none), read through the output pointer where the fold is in place
      const FhevcMotionRdPuNode* const src = reinterpret_cast<const void*>(fold) == reinterpret_cast<const void*>(out) ? out : reinterpret_cast<const FhevcMotionRdPuNode*>(fold);
      const FhevcMotionRdPuNode fr = fold ? src[rec] : none;
      // calm: the merge candidate is strictly the cheapest so far and has a masked zero bit -- HM does not try intra there (TEncCu.cpp:799-804)
      bool calm = false;
      if (rd_merge) calm = rd_merge[rec * 4 + 1] < fr.cost_rd && (((rd_merge[rec * 4 + 2] >> 16) & 0xFFu) & (unsigned)skip_mask) != 0u;
      if constexpr (NXN || SEARCH) {
        if (calm || (fold && !(u.cost_rd < fr.cost_rd))) u = fr;   // a marker's cost is below nothing: the test of validity is in the comparison
      } else
      if (calm || (fold && !(valid && u.cost_rd < fr.cost_rd))) u = fr;
      out[rec] = u;
    }
  }
}

}  // namespace

// the instances of three TU depths are launched -- and so instantiated -- at the end of this file, behind every instance there was: the ten keep their code AND
// their order in the code object
static hipError_t rd_launch_three_depths(const FhevcFrames& fr, int max_range, const FhevcRdQuant& q, int source, const unsigned* in, const unsigned* mvp, FhevcMotionRdNode* d_out,
                                         const RdPuArgs* pa, int num_cus, hipStream_t stream);
static hipError_t intra_rd_launch_three_depths(const RefineLaunch& L, const FhevcFrames& fr, const FhevcRdQuant& q, const unsigned* first, const unsigned* fold,
                                               const unsigned* rd_merge, int skip_mask, FhevcMotionRdPuNode* d_out);

// what the device keeps resident is the occupancy query's answer in both layouts: two workgroups per CU by the registers (256 VGPRs), which is also what the
// LDS allows at MR = 64 (1 824 B static + 80 016 B dynamic); the caps are the skip stage's
hipError_t fhevc_launch_motion_rd(const FhevcFrames& fr, int max_range, const FhevcRdQuant& q, int source, const void* d_in, const FhevcMotionMvp* d_mvp,
                                  FhevcMotionRdNode* d_out, int num_cus, hipStream_t stream, int tu_depths)
{
  static_assert(sizeof(FhevcMotionMergeNode) == 16 && sizeof(FhevcMotionQpelNode) == 16 && sizeof(FhevcMotionMvp) == 8 && sizeof(FhevcMotionRdNode) == 16, "record layouts");
  const unsigned* in = reinterpret_cast<const unsigned*>(d_in);
  const unsigned* mvp = reinterpret_cast<const unsigned*>(d_mvp);
  if (tu_depths == 3) return rd_launch_three_depths(fr, max_range, q, source, in, mvp, d_out, nullptr, num_cus, stream);
  return refine_launch<FHEVC_MOTION_WIDE_MAX_RANGE>(fr, (source == 0 || source == 1) && tu_depths == 2, max_range, num_cus, {4, true}, {2, true}, stream, [&](auto t, auto, auto mr, const RefineLaunch& L) {
    return refine_launch_kernel<&fhevc_motion_rd_kernel<decltype(t), decltype(mr)::value, false>>(L, fr, max_range, q, source, in, mvp, d_out);
  });
}

// the PU instances: ONE workgroup per CU by their registers (256 VGPRs + 1 AGPR: the resource table in DESIGN 4.12), which the occupancy query
// answers; the caps stay.  Every record array as dwords
hipError_t fhevc_launch_motion_rd_pu(const FhevcFrames& fr, int max_range, const FhevcRdQuant& q, int part_mode, const FhevcMotionRdPuInputs& I, FhevcMotionRdPuNode* d_out,
                                     int num_cus, hipStream_t stream, int tu_depths)
{
  static_assert(sizeof(FhevcMotionRdPuNode) == 16 && sizeof(FhevcPuShapeNode) == 16, "record layouts");
  const auto dw = [](const void* p) { return reinterpret_cast<const unsigned*>(p); };
  const RdPuArgs pa = { dw(I.pus), dw(I.pus_small), dw(I.merge_pus), dw(I.merge_pus_small), dw(I.mvp_pus), dw(I.mvp_pus_small), dw(I.shapes), dw(I.fold), part_mode };
  const bool mode_ok = part_mode >= 0 && part_mode <= 9 && part_mode != 3 && (part_mode == 0 || I.pus) && (part_mode < 8 || I.shapes) && (tu_depths == 2 || tu_depths == 3);
  if (tu_depths == 3 && I.nodes && d_out && mode_ok)
    return rd_launch_three_depths(fr, max_range, q, 1, dw(I.nodes), dw(I.mvp_nodes), reinterpret_cast<FhevcMotionRdNode*>(d_out), &pa, num_cus, stream);
  return refine_launch<FHEVC_MOTION_WIDE_MAX_RANGE>(fr, I.nodes && d_out && mode_ok, max_range, num_cus, {4, true}, {2, true}, stream, [&](auto t, auto, auto mr, const RefineLaunch& L) {
    return refine_launch_kernel<&fhevc_motion_rd_kernel<decltype(t), decltype(mr)::value, true, RdPuArgs>>(L, fr, max_range, q, 1, dw(I.nodes), dw(I.mvp_nodes),
                                                                                                         reinterpret_cast<FhevcMotionRdNode*>(d_out), pa);
  });
}

// the intra instances: no window, so the LDS (61 KB static) leaves room for two workgroups per CU; what is resident is the occupancy query's answer
hipError_t fhevc_launch_intra_rd(const FhevcFrames& fr, const FhevcRdQuant& q, const FhevcNodeCost* d_first, const FhevcMotionRdPuNode* d_fold,
                                 const FhevcMotionRdNode* d_rd_merge, int skip_mask, FhevcMotionRdPuNode* d_out, int num_cus, hipStream_t stream, int tu_depths)
{
  static_assert(sizeof(FhevcNodeCost) == 16 && offsetof(FhevcNodeCost, satd) == 0 && offsetof(FhevcNodeCost, mode) == 4, "first-pass record layout");
  const long long total = (long long)(fr.row_end - fr.row_begin) * fr.ctus_x * fr.num_frames;
  if (total <= 0) return hipSuccess;
  if (!d_first || !d_out || skip_mask < 0 || skip_mask > 3 || total > 0x7FFFFFFF || (tu_depths != 2 && tu_depths != 3)) return hipErrorInvalidValue;
  const auto dw = [](const void* p) { return reinterpret_cast<const unsigned*>(p); };
  const RefineLaunch L = { 0, { 4, true }, num_cus, total, stream };
  if (tu_depths == 3) return intra_rd_launch_three_depths(L, fr, q, dw(d_first), dw(d_fold), dw(d_rd_merge), skip_mask, d_out);
  if (fr.sample_bytes == 2) return refine_launch_kernel<&fhevc_intra_rd_kernel<int16_t>>(L, fr, q, dw(d_first), dw(d_fold), dw(d_rd_merge), skip_mask, d_out);
  return refine_launch_kernel<&fhevc_intra_rd_kernel<uint8_t>>(L, fr, q, dw(d_first), dw(d_fold), dw(d_rd_merge), skip_mask, d_out);
}

// ---- the instances of three TU depths (fhevc_motion_rd_qt*, fhevc_motion_rd_pu_qt* at tu_depths 3): the plain ones where pa is null ----
static hipError_t rd_launch_three_depths(const FhevcFrames& fr, int max_range, const FhevcRdQuant& q, int source, const unsigned* in, const unsigned* mvp, FhevcMotionRdNode* d_out,
                                         const RdPuArgs* pa, int num_cus, hipStream_t stream)
{
  return refine_launch<FHEVC_MOTION_WIDE_MAX_RANGE>(fr, source == 0 || source == 1, max_range, num_cus, {4, true}, {2, true}, stream, [&](auto t, auto, auto mr, const RefineLaunch& L) {
    if (pa)
      return refine_launch_kernel<&fhevc_motion_rd_kernel<decltype(t), decltype(mr)::value, true, RdThreeDepths, RdPuArgs>>(L, fr, max_range, q, source, in, mvp, d_out, RdThreeDepths{}, *pa);
    return refine_launch_kernel<&fhevc_motion_rd_kernel<decltype(t), decltype(mr)::value, false, RdThreeDepths>>(L, fr, max_range, q, source, in, mvp, d_out, RdThreeDepths{});
  });
}

// ---- ... and of the intra candidate (fhevc_intra_rd_qt* at tu_depths 3): 71 668 B of static LDS, which still leaves room for two workgroups per CU ----
static hipError_t intra_rd_launch_three_depths(const RefineLaunch& L, const FhevcFrames& fr, const FhevcRdQuant& q, const unsigned* first, const unsigned* fold,
                                               const unsigned* rd_merge, int skip_mask, FhevcMotionRdPuNode* d_out)
{
  if (fr.sample_bytes == 2) return refine_launch_kernel<&fhevc_intra_rd_kernel<int16_t, RdThreeDepths>>(L, fr, q, first, fold, rd_merge, skip_mask, d_out, RdThreeDepths{});
  return refine_launch_kernel<&fhevc_intra_rd_kernel<uint8_t, RdThreeDepths>>(L, fr, q, first, fold, rd_merge, skip_mask, d_out, RdThreeDepths{});
}

// workgroups of an MR = 64 instance that the device keeps on one CU (measurement tools): planes of sample_bytes, plain or PU, two or three TU depths
hipError_t fhevc_motion_rd_big_residency(int sample_bytes, bool pu, int tu_depths, int* per_cu)
{
  constexpr int MRB = FHEVC_MOTION_WIDE_MAX_RANGE;
  constexpr size_t LDS = (size_t)RefineGeom<MRB>::SAMPLES * sizeof(short);  // 80 016 B
  const auto pick = [&](auto t) -> hipError_t {
    using T = decltype(t);
    if (tu_depths == 3) return pu ? refine_resident<&fhevc_motion_rd_kernel<T, MRB, true, RdThreeDepths, RdPuArgs>>(LDS, per_cu)
                                  : refine_resident<&fhevc_motion_rd_kernel<T, MRB, false, RdThreeDepths>>(LDS, per_cu);
    return pu ? refine_resident<&fhevc_motion_rd_kernel<T, MRB, true, RdPuArgs>>(LDS, per_cu) : refine_resident<&fhevc_motion_rd_kernel<T, MRB, false>>(LDS, per_cu);
  };
  return sample_bytes == 2 ? pick(int16_t()) : pick(uint8_t());
}

// ---- the intra candidate with the NxN candidate of the 8x8 nodes (fhevc_intra_rd_nxn*): the instances of three TU depths with the second tag, behind every
// instance there was; 72 436 B of static LDS.  Without the 4x4 records it is fhevc_launch_intra_rd's launch at three depths ----
hipError_t fhevc_launch_intra_rd_nxn(const FhevcFrames& fr, const FhevcRdQuant& q, const FhevcNodeCost* d_first, const FhevcNodeCost* d_first4, const FhevcMotionRdPuNode* d_fold,
                                     const FhevcMotionRdNode* d_rd_merge, int skip_mask, FhevcMotionRdPuNode* d_out, FhevcIntraRdNxN* d_nxn, int num_cus, hipStream_t stream)
{
  static_assert(sizeof(FhevcIntraRdNxN) == 16, "record layout");
  if (!d_first4) return d_nxn ? hipErrorInvalidValue : fhevc_launch_intra_rd(fr, q, d_first, d_fold, d_rd_merge, skip_mask, d_out, num_cus, stream, 3);
  const long long total = (long long)(fr.row_end - fr.row_begin) * fr.ctus_x * fr.num_frames;
  if (total <= 0) return hipSuccess;
  if (!d_first || !d_out || skip_mask < 0 || skip_mask > 3 || total > 0x7FFFFFFF) return hipErrorInvalidValue;
  const auto dw = [](const void* p) { return reinterpret_cast<const unsigned*>(p); };
  const RefineLaunch L = { 0, { 4, true }, num_cus, total, stream };
  const RdNxN x = { dw(d_first4), reinterpret_cast<unsigned*>(d_nxn) };
  if (fr.sample_bytes == 2)
    return refine_launch_kernel<&fhevc_intra_rd_kernel<int16_t, RdThreeDepths, RdNxN>>(L, fr, q, dw(d_first), dw(d_fold), dw(d_rd_merge), skip_mask, d_out, RdThreeDepths{}, x);
  return refine_launch_kernel<&fhevc_intra_rd_kernel<uint8_t, RdThreeDepths, RdNxN>>(L, fr, q, dw(d_first), dw(d_fold), dw(d_rd_merge), skip_mask, d_out, RdThreeDepths{}, x);
}

// ---- the intra candidate searched over the first pass's lists (fhevc_intra_rd_search*): the instances of three TU depths with the third tag, behind every
// instance there was; 80 532 B of static LDS, which still leaves room for two workgroups per CU.  ONE launch: step A's positions, the 4x4 PUs' positions
// (passes of their own over the level-3 buffer) and the two runs of step B are phases of the one kernel ----
hipError_t fhevc_launch_intra_rd_search(const FhevcFrames& fr, const FhevcRdQuant& q, const uint8_t* d_modes, int list_stride, const uint8_t* d_modes4, int list_stride4,
                                        const FhevcIntraSearchRule& rule, const FhevcMotionRdPuNode* d_fold, const FhevcMotionRdNode* d_rd_merge, int skip_mask,
                                        FhevcMotionRdPuNode* d_out, FhevcIntraRdNxN* d_nxn, int num_cus, hipStream_t stream)
{
  const long long total = (long long)(fr.row_end - fr.row_begin) * fr.ctus_x * fr.num_frames;
  if (total <= 0) return hipSuccess;
  bool ok = d_modes && d_out && skip_mask >= 0 && skip_mask <= 3 && total <= 0x7FFFFFFF && list_stride >= 1 && list_stride <= 8 && rule.append_planar <= 1 && (d_modes4 || !d_nxn);
  for (int l = 0; l < 4; ++l) ok = ok && rule.count[l] >= 1 && rule.count[l] <= list_stride;
  if (d_modes4) ok = ok && list_stride4 >= 1 && list_stride4 <= 8 && rule.count4 >= 1 && rule.count4 <= list_stride4;
  if (!ok) return hipErrorInvalidValue;   // a count above its stride would read the neighbouring entry
  const auto dw = [](const void* p) { return reinterpret_cast<const unsigned*>(p); };
  const RefineLaunch L = { 0, { 4, true }, num_cus, total, stream };
  const RdSearch x = { d_modes, d_modes4, reinterpret_cast<unsigned*>(d_nxn), list_stride, d_modes4 ? list_stride4 : 1,
                       (unsigned)rule.count[0] | (unsigned)rule.count[1] << 8 | (unsigned)rule.count[2] << 16 | (unsigned)rule.count[3] << 24, d_modes4 ? rule.count4 : 1,
                       rule.append_planar };
  if (fr.sample_bytes == 2)
    return refine_launch_kernel<&fhevc_intra_rd_kernel<int16_t, RdThreeDepths, RdSearch>>(L, fr, q, dw(nullptr), dw(d_fold), dw(d_rd_merge), skip_mask, d_out, RdThreeDepths{}, x);
  return refine_launch_kernel<&fhevc_intra_rd_kernel<uint8_t, RdThreeDepths, RdSearch>>(L, fr, q, dw(nullptr), dw(d_fold), dw(d_rd_merge), skip_mask, d_out, RdThreeDepths{}, x);
}

#pragma clang diagnostic pop
