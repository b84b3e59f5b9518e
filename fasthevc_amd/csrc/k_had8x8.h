// k_had8x8.h -- the 8x8 Hadamard of a block held in one lane's registers, shared by the motion kernels (k_motion.hip: the integer search,
// k_motion_refine.hip: the quarter-sample refinement), and the 4x4 Hadamard of one quadrant of such a block (k_motion_pu_small.hip,
// k_motion_refine_pu.hip: the PUs with a 4-sample side).  Packed-16 form of k_hadamard.hip (|coefficients| stay below 2^15 through five stages
// up to 10 bit; the sixth, inside a packed pair, is folded into the absolute sum: |a+b| + |a-b| = 2 max(|a|,|b|)) and its 32-bit twin.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

typedef __attribute__((ext_vector_type(2))) short i16x2;
__device__ __forceinline__ unsigned pk_add(unsigned a, unsigned b)
{
  return __builtin_bit_cast(unsigned, (i16x2)(__builtin_bit_cast(i16x2, a) + __builtin_bit_cast(i16x2, b)));
}
__device__ __forceinline__ unsigned pk_sub(unsigned a, unsigned b)
{
  return __builtin_bit_cast(unsigned, (i16x2)(__builtin_bit_cast(i16x2, a) - __builtin_bit_cast(i16x2, b)));
}
__device__ __forceinline__ unsigned pk_abs(unsigned a)
{
  const i16x2 v = __builtin_bit_cast(i16x2, a);
  return __builtin_bit_cast(unsigned, __builtin_elementwise_max(v, (i16x2)(-v)));
}
// sum of |WHT8x8(d)| of a block held as 8 rows x 4 packed pairs (low half = even column), |samples| < 2^10
__device__ __forceinline__ unsigned had8x8_packed(unsigned (&d)[32])
{
#pragma unroll
  for (int hs = 1; hs < 8; hs <<= 1)  // vertical: rows y, y + hs
#pragma unroll
    for (int i = 0; i < 8; i += hs << 1)
#pragma unroll
      for (int y = i; y < i + hs; ++y)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const unsigned a = d[y * 4 + j], b = d[(y + hs) * 4 + j];
          d[y * 4 + j] = pk_add(a, b); d[(y + hs) * 4 + j] = pk_sub(a, b);
        }
#pragma unroll
  for (int hs = 1; hs < 4; hs <<= 1)  // horizontal distance 2 and 4: pairs j, j + hs
#pragma unroll
    for (int y = 0; y < 8; ++y)
#pragma unroll
      for (int i = 0; i < 4; i += hs << 1)
#pragma unroll
        for (int j = i; j < i + hs; ++j) {
          const unsigned a = d[y * 4 + j], b = d[y * 4 + j + hs];
          d[y * 4 + j] = pk_add(a, b); d[y * 4 + j + hs] = pk_sub(a, b);
        }
  unsigned acc = 0;
#pragma unroll
  for (int i = 0; i < 32; ++i) {  // horizontal distance 1, inside a pair: |a + b| + |a - b| = 2 max(|a|, |b|)
    const unsigned a = pk_abs(d[i]);
    acc += max(a & 0xFFFFu, a >> 16);
  }
  return 2 * acc;
}
// 32-bit twin (12-bit content): d[64] row-major
__device__ __forceinline__ unsigned had8x8_wide(int (&v)[64])
{
#pragma unroll
  for (int y = 0; y < 8; ++y)
#pragma unroll
    for (int hs = 1; hs < 8; hs <<= 1)
#pragma unroll
      for (int i = 0; i < 8; i += hs << 1)
#pragma unroll
        for (int j = i; j < i + hs; ++j) {
          const int a = v[8 * y + j], b = v[8 * y + j + hs];
          v[8 * y + j] = a + b; v[8 * y + j + hs] = a - b;
        }
#pragma unroll
  for (int x = 0; x < 8; ++x)
#pragma unroll
    for (int hs = 1; hs < 8; hs <<= 1)
#pragma unroll
      for (int i = 0; i < 8; i += hs << 1)
#pragma unroll
        for (int j = i; j < i + hs; ++j) {
          const int a = v[8 * j + x], b = v[8 * (j + hs) + x];
          v[8 * j + x] = a + b; v[8 * (j + hs) + x] = a - b;
        }
  unsigned s = 0;
#pragma unroll
  for (int i = 0; i < 64; ++i) s += (unsigned)abs(v[i]);
  return s;
}

// xCalcHADs4x4 of the quadrant at rows r0 .., packed pairs j0, j0 + 1 of a block of differences held as 8 rows x 4 packed pairs: (sum |H4 d H4| + 1) >> 1.
// |coefficients| stay below 2^15 through three stages up to 10 bit (8 * 1023); the fourth, inside a packed pair, is folded into the absolute sum:
// |a + b| + |a - b| = 2 max(|a|, |b|), so the sum is even and the rounding shift is exact
__device__ __forceinline__ unsigned had4x4_packed(const unsigned (&d)[32], int r0, int j0)
{
  unsigned a[4][2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {  // vertical
    const unsigned s0 = pk_add(d[(r0 + 0) * 4 + j0 + j], d[(r0 + 1) * 4 + j0 + j]), d0 = pk_sub(d[(r0 + 0) * 4 + j0 + j], d[(r0 + 1) * 4 + j0 + j]);
    const unsigned s1 = pk_add(d[(r0 + 2) * 4 + j0 + j], d[(r0 + 3) * 4 + j0 + j]), d1 = pk_sub(d[(r0 + 2) * 4 + j0 + j], d[(r0 + 3) * 4 + j0 + j]);
    a[0][j] = pk_add(s0, s1); a[1][j] = pk_sub(s0, s1); a[2][j] = pk_add(d0, d1); a[3][j] = pk_sub(d0, d1);
  }
  unsigned acc = 0;
#pragma unroll
  for (int y = 0; y < 4; ++y) {  // horizontal distance 2: pair 0 +- pair 1; distance 1: inside the pair
    const unsigned p = pk_abs(pk_add(a[y][0], a[y][1])), q = pk_abs(pk_sub(a[y][0], a[y][1]));
    acc += max(p & 0xFFFFu, p >> 16) + max(q & 0xFFFFu, q >> 16);
  }
  return (2 * acc + 1) >> 1;
}
// 32-bit twin (12-bit content): v[64] row-major, the quadrant at (r0, c0)
__device__ __forceinline__ unsigned had4x4_wide(const int (&v)[64], int r0, int c0)
{
  int a[16];
#pragma unroll
  for (int y = 0; y < 4; ++y) {
    const int x0 = v[8 * (r0 + y) + c0], x1 = v[8 * (r0 + y) + c0 + 1], x2 = v[8 * (r0 + y) + c0 + 2], x3 = v[8 * (r0 + y) + c0 + 3];
    const int s0 = x0 + x1, d0 = x0 - x1, s1 = x2 + x3, d1 = x2 - x3;
    a[4 * y + 0] = s0 + s1; a[4 * y + 1] = s0 - s1; a[4 * y + 2] = d0 + d1; a[4 * y + 3] = d0 - d1;
  }
  unsigned s = 0;
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    const int s0 = a[x] + a[4 + x], d0 = a[x] - a[4 + x], s1 = a[8 + x] + a[12 + x], d1 = a[8 + x] - a[12 + x];
    s += (unsigned)abs(s0 + s1) + (unsigned)abs(s0 - s1) + (unsigned)abs(d0 + d1) + (unsigned)abs(d0 - d1);
  }
  return (s + 1) >> 1;
}

}  // namespace
