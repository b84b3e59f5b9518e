// k_refine_tile.h -- what the two quarter-sample refinement kernels share (k_motion_refine.hip: the 85 square CU nodes; k_motion_refine_pu.hip: the
// 508 PUs): the reference window in LDS, the candidate tables, and the prediction of one 8x8 tile at one quarter-sample
// candidate as a block of differences to the original.  The interpolation form is the one k_motion_refine.hip's header comment derives: the
// fractions are DATA (two packed coefficient vectors per lane), so the lanes of a wave need not agree on a phase.
#pragma once
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

}  // namespace
