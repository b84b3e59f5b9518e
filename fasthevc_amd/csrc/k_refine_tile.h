// k_refine_tile.h -- what the five quarter-sample window kernels share (k_motion_refine.hip: the 85 square CU nodes refined; k_motion_refine_pu.hip: the
// 508 PUs refined; k_motion_merge.hip and k_motion_merge_pu.hip: the merge candidates of the nodes and of the PUs; k_motion_skip.hip: the zero-residual test
// per node).  All five run one mapping: workgroup (4 waves) = one CTU at a time, grid-stride (k_search_tile.h's SearchWork); the reference window in LDS
// (MR = 8 layout: static, MR = 64 layout: dynamic); lane = one 8x8 tile, predicted at a quarter-sample candidate as a block of differences to the
// original.  Here, once: the window and its staging, the candidate tables, the tile prediction, a lane's square node and its sum, the PU passes and a PU's
// sum, the merge list, the output records, and the launch.  Each kernel keeps its body.  The interpolation form is the one k_motion_refine.hip's header
// comment derives: the fractions are DATA (two packed coefficient vectors per lane), so the lanes of a wave need not agree on a phase.
#pragma once
#include <atomic>
#include "fhevc_internal.h"
#include "k_had8x8.h"
#include "k_search_tile.h"  // sample_of, load_tile8x8: one definition for the searches and the refinements

namespace {

template <int MR> struct RefineGeom {
  static constexpr int RP = 64 + 2 * MR + 8;    // LDS row pitch in samples: the CTU, the range, and 4 samples each side for the taps (x-3 .. x+4 around x-1 .. x)
  static constexpr int ROWS = 64 + 2 * MR + 8;
  static constexpr int SAMPLES = ROWS * RP + 8; // a lane's ninth dword of a row may lie behind the window's last sample: never used for its value
};

// c_f as four packed pairs (low half = the tap of the lower coordinate)
#define FHEVC_PK(a, b) (((unsigned)(a) & 0xFFFFu) | ((unsigned)(b) << 16))
__constant__ unsigned kLumaTaps[16] = {
  FHEVC_PK(0, 0), FHEVC_PK(0, 64), FHEVC_PK(0, 0), FHEVC_PK(0, 0),
  FHEVC_PK(-1, 4), FHEVC_PK(-10, 58), FHEVC_PK(17, -5), FHEVC_PK(1, 0),
  FHEVC_PK(-1, 4), FHEVC_PK(-11, 40), FHEVC_PK(40, -11), FHEVC_PK(4, -1),
  FHEVC_PK(0, 1), FHEVC_PK(-5, 17), FHEVC_PK(58, -10), FHEVC_PK(4, -1) };
#undef FHEVC_PK
// s_acMvRefineH, then s_acMvRefineQ (TEncSearch.cpp:51-75): (x, y) as two signed nibbles
__constant__ signed char kRefineX[18] = { 0, 0, 0, -1, 1, -1, 1, -1, 1,   0, 0, 0, -1, 1, -1, 1, -1, 1 };
__constant__ signed char kRefineY[18] = { 0, -1, 1, 0, 0, -1, -1, 1, 1,   0, -1, 1, -1, -1, 0, 0, 1, 1 };

__device__ __forceinline__ int dot2(unsigned a, unsigned b, int c)
{
  return __builtin_amdgcn_sdot2(__builtin_bit_cast(i16x2, a), __builtin_bit_cast(i16x2, b), c, false);
}
__device__ __forceinline__ int eg_bits(int v)  // xGetExpGolombNumberOfBits (TComRdCost.h:177-190)
{
  const unsigned u = (v <= 0) ? (((unsigned)(-v)) << 1) + 1u : ((unsigned)v) << 1;
  return 1 + 2 * (31 - __builtin_clz(u));
}

// the constants of the interpolation at one bit depth
struct RefineArith {
  int bd, shift, v_off, v_shift, top;
  __device__ __forceinline__ explicit RefineArith(int bit_depth)
    : bd(bit_depth), shift(bit_depth - 8), v_off((1 << (19 - bit_depth)) + (8192 << 6)), v_shift(20 - bit_depth), top((1 << bit_depth) - 1) {}
};

// ---- one chunk of 4 samples of the reference window of CTU (cx, cy): window row wr, columns wc .. wc + 3 = picture row cy*64 - MR - 4 + wr, columns
// cx*64 - MR - 4 + wc .., coordinates clamped to the picture.  The window's first column is a multiple of 4, so a chunk inside the picture is ONE 8-byte
// (uint8 planes: 4-byte) load where the plane allows it, and one 8-byte LDS store.  The centred refinements move the window by their centre (ox, oy): the
// coarse centres are multiples of 4, so their chunks keep the one-load form; any other centre goes through the per-sample form ----
template <typename T, int MR>
__device__ __forceinline__ void refine_stage_chunk(short* s_ref, const T* plane, long long ref_base, const FhevcFrames& F, int cx, int cy, int wr, int wc,
                                                   int ox = 0, int oy = 0)
{
  constexpr int RP = RefineGeom<MR>::RP;
  const int py = min(max(cy * 64 - MR - 4 + oy + wr, 0), F.height - 1);
  const int px0 = cx * 64 - MR - 4 + ox + wc;
  const long long row = ref_base + (long long)py * F.stride;
  const T* src = plane + row + px0;
  uint2 q;
  if (px0 >= 0 && px0 + 4 <= F.width && (reinterpret_cast<uintptr_t>(src) & (4 * sizeof(T) - 1)) == 0) {
    if (sizeof(T) == 2) q = *reinterpret_cast<const uint2*>(src);
    else {
      const unsigned b = *reinterpret_cast<const unsigned*>(src);
      q.x = (b & 0xFFu) | ((b & 0xFF00u) << 8); q.y = ((b >> 16) & 0xFFu) | ((b >> 24) << 16);
    }
  } else {
    int v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = sample_of(plane, row + min(max(px0 + k, 0), F.width - 1));
    q.x = ((unsigned)v[0] & 0xFFFFu) | ((unsigned)v[1] << 16); q.y = ((unsigned)v[2] & 0xFFFFu) | ((unsigned)v[3] << 16);
  }
  *reinterpret_cast<uint2*>(s_ref + wr * RP + wc) = q;
}

// ---- stage the whole reference window of CTU (cx, cy): rows cy*64 - MR - 4 .., columns cx*64 - MR - 4 .. ----
template <typename T, int MR>
__device__ __forceinline__ void refine_stage_window(short* s_ref, const T* plane, long long ref_base, const FhevcFrames& F, int cx, int cy, int tid,
                                                    int ox = 0, int oy = 0)
{
  constexpr int CH = RefineGeom<MR>::RP / 4;
  for (int it = tid; it < RefineGeom<MR>::ROWS * CH; it += 256) {
    const int wr = it / CH, wc = (it - wr * CH) * 4;
    refine_stage_chunk<T, MR>(s_ref, plane, ref_base, F, cx, cy, wr, wc, ox, oy);
  }
}

// ---- ... or only the part of it that vectors of up to max_range can reach: a candidate's first tap lies (qx >> 2) - 3 >= -max_range - 4 samples before
// the tile and its last one (qx >> 2) + 4 <= max_range + 4 behind it, so window rows and columns MR - max_range .. RP - 1 - (MR - max_range) hold every
// sample that is read for its value; the columns are widened to whole chunks.  Same addresses, same values: the rest of the window is never staged and
// never used ----
template <typename T, int MR>
__device__ __forceinline__ void refine_stage_window_reach(short* s_ref, const T* plane, long long ref_base, const FhevcFrames& F, int cx, int cy, int tid, int max_range)
{
  constexpr int CH = RefineGeom<MR>::RP / 4;
  const int skip = MR - max_range, c0 = skip >> 2;       // rows skipped at either end; chunks skipped at either end (RP is a multiple of 4)
  const int rows = RefineGeom<MR>::ROWS - 2 * skip, ch = CH - 2 * c0;
  for (int it = tid; it < rows * ch; it += 256) {
    const int r = it / ch;
    refine_stage_chunk<T, MR>(s_ref, plane, ref_base, F, cx, cy, skip + r, (c0 + it - r * ch) * 4);
  }
}

// ---- original minus prediction of the 8x8 tile whose sample (0, 0) has its first tap at window column `col`, row `row0`, at fraction (fx, fy): as 8 rows
// x 4 packed pairs in D (PACKED: bit depth <= 10) or 64 integers in v.  Two taps per v_dot2_i32_i16: horizontally on pairs of neighbouring samples
// (aligned dword reads + v_alignbit), vertically on pairs of rows of the 16-bit intermediates.  A wave whose lanes all have a zero fraction in one
// direction skips that filter's arithmetic ----
template <bool PACKED, int RP>
__device__ __forceinline__ void refine_tile_diff(const short* s_ref, const unsigned* s_taps, const RefineArith& A, int col, int row0, int fx, int fy,
                                                 const unsigned (&O)[32], unsigned (&D)[32], int (&v)[64])
{
  const int bd = A.bd, shift = A.shift, v_off = A.v_off, v_shift = A.v_shift, top = A.top;
  const unsigned sh = (unsigned)(col & 1) * 16u;
  const bool hor = __builtin_amdgcn_ballot_w64(fx != 0) != 0, ver = __builtin_amdgcn_ballot_w64(fy != 0) != 0;  // wave-uniform
  unsigned cxp[4], cyp[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { cxp[j] = s_taps[4 * fx + j]; cyp[j] = s_taps[4 * fy + j]; }
  // ---- horizontal: rows row0 .. + 14, 8 intermediates each, kept as pairs of rows: Pe[r / 2][x] = (t[r][x], t[r + 1][x]) ----
  unsigned Pe[8][8];
  if (ver) {
#pragma unroll
    for (int r = 0; r < 15; ++r) {
      const unsigned* q = reinterpret_cast<const unsigned*>(s_ref) + (((row0 + r) * RP + col) >> 1);
      int t[8];
      if (hor) {
        unsigned d[9], N[8], M[7];
#pragma unroll
        for (int k = 0; k < 9; ++k) d[k] = q[k];
#pragma unroll
        for (int k = 0; k < 8; ++k) N[k] = __builtin_amdgcn_alignbit(d[k + 1], d[k], sh);    // pairs starting at col, col + 2, ..
#pragma unroll
        for (int k = 0; k < 7; ++k) M[k] = __builtin_amdgcn_alignbit(N[k + 1], N[k], 16u);   // pairs starting at col + 1, col + 3, ..
#pragma unroll
        for (int x = 0; x < 8; ++x) {
          int a = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) a = dot2((x & 1) ? M[(x >> 1) + j] : N[(x >> 1) + j], cxp[j], a);
          t[x] = (a >> shift) - 8192;
        }
      } else {  // fx = 0 in every lane: (64 s >> (bd - 8)) - 8192 of samples col + 3 .. col + 10
        unsigned d[7], N[6];
#pragma unroll
        for (int k = 1; k < 7; ++k) d[k] = q[k];
#pragma unroll
        for (int k = 1; k < 6; ++k) N[k] = __builtin_amdgcn_alignbit(d[k + 1], d[k], sh);     // pairs starting at col + 2 k
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const unsigned pr = __builtin_amdgcn_alignbit(N[k + 2], N[k + 1], 16u);              // samples col + 3 + 2 k, + 1
          t[2 * k] = (int)((pr & 0xFFFFu) << (14 - bd)) - 8192; t[2 * k + 1] = (int)((pr >> 16) << (14 - bd)) - 8192;
        }
      }
#pragma unroll
      for (int x = 0; x < 8; ++x) {
        if (r & 1) Pe[r >> 1][x] = (Pe[r >> 1][x] & 0xFFFFu) | ((unsigned)t[x] << 16);
        else Pe[r >> 1][x] = (unsigned)t[x] & 0xFFFFu;
      }
    }
  }
  // ---- vertical, difference to the original ----
#pragma unroll
  for (int y = 0; y < 8; ++y) {
    int p[8];
    if (ver) {
#pragma unroll
      for (int x = 0; x < 8; ++x) {
        int a = v_off;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int m = (y >> 1) + j;
          a = dot2((y & 1) ? __builtin_amdgcn_alignbit(Pe[m + 1][x], Pe[m][x], 16u) : Pe[m][x], cyp[j], a);
        }
        p[x] = min(max(a >> v_shift, 0), top);
      }
    } else {  // fy = 0 in every lane: row row0 + 3 + y, filtered horizontally to the final sample
      const unsigned* q = reinterpret_cast<const unsigned*>(s_ref) + (((row0 + 3 + y) * RP + col) >> 1);
      unsigned d[9], N[8], M[7];
#pragma unroll
      for (int k = 0; k < 9; ++k) d[k] = q[k];
#pragma unroll
      for (int k = 0; k < 8; ++k) N[k] = __builtin_amdgcn_alignbit(d[k + 1], d[k], sh);
#pragma unroll
      for (int k = 0; k < 7; ++k) M[k] = __builtin_amdgcn_alignbit(N[k + 1], N[k], 16u);
#pragma unroll
      for (int x = 0; x < 8; ++x) {
        int a = 32;
#pragma unroll
        for (int j = 0; j < 4; ++j) a = dot2((x & 1) ? M[(x >> 1) + j] : N[(x >> 1) + j], cxp[j], a);
        p[x] = min(max(a >> 6, 0), top);
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned o = O[4 * y + k];
      if constexpr (PACKED) D[4 * y + k] = pk_sub(o, ((unsigned)p[2 * k] & 0xFFFFu) | ((unsigned)p[2 * k + 1] << 16));
      else { v[8 * y + 2 * k] = (int)(o & 0xFFFFu) - p[2 * k]; v[8 * y + 2 * k + 1] = (int)(o >> 16) - p[2 * k + 1]; }
    }
  }
}

// ... of the lane's tile (tx, ty) of the CTU at the quarter-sample vector (qx, qy); the CTU begins (RP - 64) / 2 = MR + 4 samples into the window
template <bool PACKED, int RP>
__device__ __forceinline__ void refine_tile_at(const short* s_ref, const unsigned* s_taps, const RefineArith& A, int tx, int ty, int qx, int qy,
                                               const unsigned (&O)[32], unsigned (&D)[32], int (&v)[64])
{
  constexpr int ORG = (RP - 64) / 2;
  const int col = tx * 8 + ORG + (qx >> 2) - 3, row0 = ty * 8 + ORG + (qy >> 2) - 3;  // first tap of sample (0, 0)
  refine_tile_diff<PACKED, RP>(s_ref, s_taps, A, col, row0, qx & 3, qy & 3, O, D, v);
}
// the tile's Hadamard of that difference; 0 where the tile is not inside the picture.  The caller declares D and v inside its candidate loop: with the two
// arrays in a helper of their own the compiler allocated the registers of that loop differently from how it does for the loop written out
template <bool PACKED>
__device__ __forceinline__ unsigned refine_had8x8(unsigned (&D)[32], int (&v)[64], bool inside)
{
  unsigned t8;
  if constexpr (PACKED) t8 = had8x8_packed(D);
  else t8 = had8x8_wide(v);
  return inside ? ((t8 + 2) >> 2) : 0u;  // xCalcHADs8x8: (sum + 2) >> 2 (TComRdCost.cpp:1747)
}

// ---- a vector dword of a record: mvx in the low half, mvy in the high one.  A vector is used only if both components lie within the reach of a refined
// vector, 4 max_range + 3 quarter samples, so no input byte can send a read outside the staged window ----
__device__ __forceinline__ int vec_x(unsigned w) { return (int)(short)(w & 0xFFFFu); }
__device__ __forceinline__ int vec_y(unsigned w) { return (int)(short)(w >> 16); }
__device__ __forceinline__ int vec_reach(int max_range) { return 4 * max_range + 3; }
__device__ __forceinline__ bool vec_in_reach(unsigned w, int reach) { return abs(vec_x(w)) <= reach && abs(vec_y(w)) <= reach; }

// ---- the square node of tile (tx, ty) where wave = level (0: 64x64 .. 3: 8x8): ncnt x ncnt nodes in the CTU, this one at (nbx, nby); first: the level's
// first node among the CTU's 85, nidx: this one; writer: the lane of the node's first tile ----
struct RefineNode {
  int ncnt, nbx, nby, first, nidx;
  bool writer;
  __device__ __forceinline__ RefineNode(int lvl, int tx, int ty)
    : ncnt(1 << lvl), nbx(tx >> (3 - lvl)), nby(ty >> (3 - lvl)), first(((1 << (2 * lvl)) - 1) / 3), nidx(first + nby * ncnt + nbx),
      writer((tx & ((8 >> lvl) - 1)) == 0 && (ty & ((8 >> lvl) - 1)) == 0) {}
};
// the node's sum: 16x16 = tiles (tx ^ 1, ty ^ 1), 32x32 = + bits 1, 64x64 = + bits 2 (wave-uniform depth)
__device__ __forceinline__ unsigned refine_node_sum(unsigned t8, int lvl)
{
  unsigned s = t8;
  for (int k = 0; k < 3 - lvl; ++k) {
    s += __shfl_xor(s, 1 << k);
    s += __shfl_xor(s, 8 << k);
  }
  return s;
}

// ---- the 26 PU passes (k_motion_refine_pu.hip's header comment), each a covering of the CTU by one (CU size, shape) pair: what pass `pass` (wave-uniform)
// makes of tile (tx, ty) ----
constexpr int PASSES_PU = 14, PASSES = 26;
struct RefinePuPass {
  bool small, horiz, rep;   // one of the 12 passes of the 384; the CU is cut by a horizontal line: part 0 on top; this lane writes the PU
  int n, s;                 // CU of 2^n x 2^n tiles (small: n = 1: 16x16, 0: 8x8), shape (0 2NxN, 1 Nx2N, 2 2NxnU, 3 2NxnD, 4 nLx2N, 5 nRx2N)
  int nbx, nby, lx, ly;     // the CU on its level's grid inside the CTU, the tile inside the CU
  int part, entry;          // the part that holds the tile (small: the part the pass sums), its index in the family's layout
  unsigned qmask;           // small: the quadrants q00 q01 / q10 q11 of the tile that lie in the pass's part
  __device__ __forceinline__ RefinePuPass(int pass, int tx, int ty)
  {
    small = pass >= PASSES_PU;
    int want = 0;
    if (!small) { n = pass < 6 ? 3 : pass < 12 ? 2 : 1; s = pass - (pass < 6 ? 0 : pass < 12 ? 6 : 12); }
    else { const int c = (pass - PASSES_PU) >> 1; want = (pass - PASSES_PU) & 1; n = c < 4 ? 1 : 0; s = c < 4 ? 2 + c : c - 4; }
    const int tn = 1 << n;
    lx = tx & (tn - 1); ly = ty & (tn - 1);
    horiz = s == 0 || s == 2 || s == 3;
    nbx = tx >> n; nby = ty >> n;
    const int ni = nby * (8 >> n) + nbx;                             // the CU among those of its size, raster
    qmask = 0;
    if (!small) {
      const int sp = s < 2 ? tn / 2 : (s & 1) ? 3 * tn / 4 : tn / 4;   // where the CU is cut, in tiles
      const int other = horiz ? lx : ly;
      part = along() >= sp ? 1 : 0;
      rep = other == 0 && along() == part * sp;
      entry = (n == 3 ? 0 : n == 2 ? (1 + ni) * 12 : 60 + ni * 4) + s * 2 + part;
    } else {
      part = want;
      const int cut = n == 0 ? 1 : (s & 1) ? 3 : 1;                // in 4-sample units from the CU's top (left) edge
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int pos = horiz ? ly * 2 + (k >> 1) : lx * 2 + (k & 1);
        if ((pos >= cut ? 1 : 0) == want) qmask |= 1u << k;
      }
      rep = lx == 0 && ly == 0;
      entry = n == 1 ? ni * 8 + (s - 2) * 2 + part : 128 + ni * 4 + s * 2 + part;
    }
  }
  __device__ __forceinline__ int along() const { return horiz ? ly : lx; }   // the tile's row (column) inside the CU
  __device__ __forceinline__ int nsize() const { return 8 << n; }            // the CU's side in samples
  // the PU's record among those of its family (pus / pus_small) of the CTU with output index oc
  __device__ __forceinline__ long long record(long long oc) const { return small ? oc * FHEVC_PUS_SMALL + entry : oc * FHEVC_PUS + entry; }
};

// the sum over the tiles of this lane's PU of a tile-aligned pass: n and s are wave-uniform
__device__ __forceinline__ unsigned pu_sum(unsigned t8, int lane, const RefinePuPass& U)
{
  const int n = U.n, s = U.s, along = U.along();
  const int ob = U.horiz ? 1 : 8, ab = U.horiz ? 8 : 1;   // lane bits across the cut's direction / along it
  unsigned strip = t8;
  for (int k = 0; k < n; ++k) strip += __shfl_xor(strip, ob << k);       // the CU's whole width (height) at this tile row (column)
  const int own = s < 2 ? n - 1 : n - 2;                                 // ... summed over the lane's own half, or its own quarter
  for (int k = 0; k < own; ++k) strip += __shfl_xor(strip, ab << k);
  if (s < 2) return strip;
  unsigned cu = strip;
  for (int k = own; k < n; ++k) cu += __shfl_xor(cu, ab << k);
  const int qpart = s & 1;                                               // 2NxnU, nLx2N: the quarter comes first; 2NxnD, nRx2N: last
  const unsigned quarter = __shfl(strip, lane + ((qpart ? (1 << n) - 1 : 0) - along) * ab);
  return U.part == qpart ? quarter : cu - quarter;
}

// xGetHADs of this lane's PU of pass U at the quarter-sample vector (qx, qy), before the shift by bit depth - 8: every lane predicts its tile there
template <bool PACKED, int RP>
__device__ __forceinline__ unsigned refine_pu_had(const short* s_ref, const unsigned* s_taps, const RefineArith& A, int lane, int tx, int ty, const RefinePuPass& U,
                                                  int qx, int qy, const unsigned (&O)[32], bool inside)
{
  unsigned D[32];
  int v[64];
  refine_tile_at<PACKED, RP>(s_ref, s_taps, A, tx, ty, qx, qy, O, D, v);
  if (U.small) {  // xCalcHADs4x4 per quadrant, (sum + 1) >> 1 each (TComRdCost.cpp:1771-1803); only the quadrants of this pass's part
    unsigned sum = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      unsigned q;
      if constexpr (PACKED) q = had4x4_packed(D, (k >> 1) * 4, (k & 1) * 2);
      else q = had4x4_wide(v, (k >> 1) * 4, (k & 1) * 4);
      sum += ((U.qmask >> k) & 1u) ? q : 0u;
    }
    sum = inside ? sum : 0u;
    if (U.n == 1) { sum += __shfl_xor(sum, 1); sum += __shfl_xor(sum, 8); }  // the four tiles of the 16x16 CU
    return sum;
  }
  return pu_sum(refine_had8x8<PACKED>(D, v, inside), lane, U);
}

// ---- the refinements' output record; the marker where nothing was refined ----
__device__ __forceinline__ FhevcMotionQpelNode refine_record(bool valid, unsigned satd_int, unsigned satd_best, unsigned cost_best, int mvx, int mvy)
{
  FhevcMotionQpelNode o;
  if (valid) { o.satd_int = satd_int; o.satd_best = satd_best; o.cost_best = cost_best; o.mvx = (short)mvx; o.mvy = (short)mvy; }
  else { o.satd_int = o.satd_best = o.cost_best = 0xFFFFFFFFu; o.mvx = 0; o.mvy = 0; }
  return o;
}

// ---- the merge list of TComDataCU::getInterMergeCandidates (TComDataCU.cpp:2142-2320) from the vectors nvec of the five neighbours L, A, AR, BL, AL of
// which av says whether they can be used: HM's order with HM's four pruning pairs, AL only below four entries, then one zero vector.  Five "taken" flags in
// registers; a lane whose list is shorter than its wave's longest picks the zero vector there and drops the result ----
constexpr unsigned kMergeMark = 0xFFFFFFFFu;
struct MergeList {
  bool take[5];
  unsigned nvec[5];
  int num;
  __device__ __forceinline__ MergeList(const bool (&av)[5], const unsigned (&vec)[5], bool node_in)
  {
#pragma unroll
    for (int j = 0; j < 5; ++j) nvec[j] = vec[j];
    take[0] = av[0];
    take[1] = av[1] && !(av[0] && nvec[1] == nvec[0]);
    take[2] = av[2] && !(av[1] && nvec[2] == nvec[1]);
    take[3] = av[3] && !(av[0] && nvec[3] == nvec[0]);
    const int n4 = (int)take[0] + (int)take[1] + (int)take[2] + (int)take[3];
    take[4] = n4 < 4 && av[4] && !(av[0] && nvec[4] == nvec[0]) && !(av[1] && nvec[4] == nvec[1]);
    const int n5 = n4 + (int)take[4];
    num = node_in ? n5 + (n5 < 5 ? 1 : 0) : 0;   // the zero vector closes a list of fewer than five
  }
  // the longest list of the wave: the candidate loop's wave-uniform length
  __device__ __forceinline__ int longest() const
  {
    int l = 1;
#pragma unroll
    for (int n = 2; n <= 5; ++n)
      if (__builtin_amdgcn_ballot_w64(num >= n) != 0) l = n;
    return l;
  }
  // entry i: its vector dword and which neighbour it came from (5: the zero vector, or the list has ended); unrolled, no dynamic indexing
  __device__ __forceinline__ void pick(int i, unsigned& qv, int& src) const
  {
    qv = 0; src = 5;
    int pos = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      if (take[j] && pos == i) { qv = nvec[j]; src = j; }
      pos += (int)take[j];
    }
  }
};
// z-scan index of (x, y) in a level's grid of up to 8 x 8 nodes: the bit interleave, x in the even bits
__device__ __forceinline__ unsigned merge_z(unsigned x, unsigned y)
{
  const unsigned sx = (x & 1u) | ((x & 2u) << 1) | ((x & 4u) << 2), sy = (y & 1u) | ((y & 2u) << 1) | ((y & 4u) << 2);
  return sx | (sy << 1);
}
// getCost(bits of merge index i) from the launch's table by number of bits: 1, 2, 3, 4, 4 -- MaxNumMergeCand 5: the last index saves its terminating bit
__device__ __forceinline__ unsigned merge_index_cost(const unsigned* s_cost, int i) { return s_cost[i == 4 ? 4 : i + 1]; }
// the best entry so far (strict "<": the first entry of equal cost wins) and the record it ends as
struct MergeBest {
  unsigned c = kMergeMark, s = kMergeMark, v = 0;
  int i = 255, src = 255;
  __device__ __forceinline__ void offer(int idx, int num, unsigned cost, unsigned satd, unsigned qv, int from)
  {
    if (idx < num && cost < c) { c = cost; s = satd; v = qv; i = idx; src = from; }
  }
  __device__ __forceinline__ FhevcMotionMergeNode record(int num) const
  {
    FhevcMotionMergeNode o;
    o.satd_best = s; o.cost_best = c;
    o.mvx = (short)(v & 0xFFFFu); o.mvy = (short)(v >> 16);
    o.idx = (uint8_t)i; o.num = (uint8_t)num; o.src = (uint8_t)src; o.pad = 0;
    return o;
  }
};

// ---- launch.  Per layout the persistent grid has at most `cap` workgroups per CU (0: no cap) and, where `ask` is set, no more than the device says it
// keeps resident (hipErrorLaunchOutOfResources where that is none); no more workgroups than there are CTUs ----
struct RefineResidency { int cap; bool ask; };
struct RefineLaunch {
  size_t lds;   // dynamic LDS: the MR = 64 window (80 016 B), 0 at MR = 8
  RefineResidency res;
  int num_cus;
  long long total;
  hipStream_t stream;
};

// one kernel instance: its dynamic LDS allowed, and how many of its workgroups the device keeps on one CU (asked once per instance)
template <auto Kernel>
hipError_t refine_resident(size_t lds, int* per_cu)
{
  if (lds) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  if (!per_cu) return hipSuccess;
  static std::atomic<int> asked{0};   // every device of a context is a gfx950: one answer per instance
  int n = asked.load(std::memory_order_relaxed);
  if (n == 0) {
    const hipError_t q = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, Kernel, 256, lds);
    if (q != hipSuccess) return q;
    asked.store(n, std::memory_order_relaxed);
  }
  *per_cu = n;
  return hipSuccess;
}

template <auto Kernel, typename... Args>
hipError_t refine_launch_kernel(const RefineLaunch& L, Args... args)
{
  int asked = 0, per_cu = L.res.cap;
  const hipError_t e = refine_resident<Kernel>(L.lds, L.res.ask ? &asked : nullptr);
  if (e != hipSuccess) return e;
  if (L.res.ask) {
    if (asked < 1) return hipErrorLaunchOutOfResources;
    if (per_cu == 0 || asked < per_cu) per_cu = asked;
  }
  const long long resident = (long long)per_cu * L.num_cus;
  const int grid = (int)(L.total < resident ? L.total : resident);
  hipLaunchKernelGGL(Kernel, dim3(grid), dim3(256), L.lds, L.stream, args...);
  return hipGetLastError();
}

// what the launch functions of the five kernels share: nothing to do for an empty band; max_range 1 .. RANGE_MAX and a CTU count the kernels' int holds;
// the layout from max_range (the MR = 64 one only where RANGE_MAX reaches it); launch(T(), packed, mr, L) with T = int16_t (HM Pel planes) or uint8_t,
// packed (bit depth <= 10) as std::true_type / std::false_type, mr as std::integral_constant, and L for refine_launch_kernel
template <int RANGE_MAX, typename Launch>
hipError_t refine_launch(const FhevcFrames& fr, bool args_ok, int max_range, int num_cus, RefineResidency small, RefineResidency big, hipStream_t stream, Launch&& launch)
{
  const long long total = (long long)(fr.row_end - fr.row_begin) * fr.ctus_x * (fr.num_frames - 1);
  if (total <= 0) return hipSuccess;
  if (!args_ok || max_range < 1 || max_range > RANGE_MAX || total > 0x7FFFFFFF) return hipErrorInvalidValue;
  const auto dispatch = [&](auto mr, RefineResidency res) -> hipError_t {
    constexpr int MR = decltype(mr)::value;
    const RefineLaunch L = { MR > FHEVC_MOTION_MAX_RANGE ? (size_t)RefineGeom<MR>::SAMPLES * sizeof(short) : 0, res, num_cus, total, stream };
    const std::true_type yes; const std::false_type no;
    if (fr.sample_bytes == 2 && fr.bit_depth <= 10) return launch(int16_t(), yes, mr, L);
    if (fr.sample_bytes == 2) return launch(int16_t(), no, mr, L);
    return launch(uint8_t(), yes, mr, L);
  };
  if constexpr (RANGE_MAX > FHEVC_MOTION_MAX_RANGE)
    if (max_range > FHEVC_MOTION_MAX_RANGE) return dispatch(std::integral_constant<int, FHEVC_MOTION_WIDE_MAX_RANGE>(), big);
  return dispatch(std::integral_constant<int, FHEVC_MOTION_MAX_RANGE>(), small);
}

}  // namespace
