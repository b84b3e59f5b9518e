// k_firstpass_common.h -- what the two first-pass kernels (k_firstpass.hip: the 85 nodes, k_firstpass4.hip: the 256 4x4 PUs) share:
// HM's coding-order availability rule and the staging of a CTU with the row above it and the column left of it in LDS.
#pragma once
#include "fhevc_internal.h"

namespace fhevc_fp {

// raster 16x16 -> z-order (Morton) of the 4x4 units of a CTU (TComRom.cpp:290-323)
__device__ __forceinline__ int zorder_of(int ux, int uy)
{
  int z = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) z |= (((ux >> b) & 1) << (2 * b)) | (((uy >> b) & 1) << (2 * b + 1));
  return z;
}

__device__ __forceinline__ bool unit_available(int ux, int uy, int x0, int y0, int width, int height, int ctus_x)
{
  if (ux < 0 || uy < 0 || ux >= width || uy >= height) return false;
  const int ca = (uy >> 6) * ctus_x + (ux >> 6), cb = (y0 >> 6) * ctus_x + (x0 >> 6);
  if (ca != cb) return ca < cb;
  return zorder_of((ux & 63) >> 2, (uy & 63) >> 2) < zorder_of((x0 & 63) >> 2, (y0 & 63) >> 2);
}

// a sample that an AVAILABLE unit covers: inside this CTU, in the row above it, or in the column left of it
__device__ __forceinline__ short staged(const short* s_org, const short* s_above, const short* s_left, int px, int py, int ox, int oy)
{
  if (py >= oy && px >= ox) return s_org[(py - oy) * 64 + (px - ox)];
  if (py < oy) return s_above[px - ox + 1];
  return s_left[py - oy];
}

// 256 threads stage the CTU at (ox, oy) (16 samples per thread), the row above it (129 samples from x = ox - 1) and the column left of it (64).
// Three load paths: 16-byte aligned int16, 16-byte aligned uint8, and the per-sample fallback; samples outside the picture are 0.
template <typename T>
__device__ __forceinline__ void stage_ctu(const T* frame, const FhevcFrames& F, int ox, int oy, int tid, short* s_org, short* s_above, short* s_left)
{
  const int row = tid >> 2, seg = (tid & 3) * 16;
  const int y = oy + row;
  const T* src = frame + (long long)y * F.stride + ox + seg;
  short* dst = &s_org[row * 64 + seg];
  const bool whole = y < F.height && ox + seg + 16 <= F.width;
  if (whole && sizeof(T) == 2 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
    reinterpret_cast<uint4*>(dst)[0] = reinterpret_cast<const uint4*>(src)[0];
    reinterpret_cast<uint4*>(dst)[1] = reinterpret_cast<const uint4*>(src)[1];
  } else if (whole && sizeof(T) == 1 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
    const uint4 q = *reinterpret_cast<const uint4*>(src);
    const unsigned w[4] = { q.x, q.y, q.z, q.w };
    unsigned o8[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) o8[k] = ((w[k >> 1] >> (16 * (k & 1))) & 0xFF) | (((w[k >> 1] >> (16 * (k & 1) + 8)) & 0xFF) << 16);
    reinterpret_cast<uint4*>(dst)[0] = make_uint4(o8[0], o8[1], o8[2], o8[3]);
    reinterpret_cast<uint4*>(dst)[1] = make_uint4(o8[4], o8[5], o8[6], o8[7]);
  } else {
#pragma unroll 4
    for (int k = 0; k < 16; ++k) dst[k] = (y < F.height && ox + seg + k < F.width) ? (short)src[k] : (short)0;
  }
  if (tid < 129) {
    const int x = ox - 1 + tid;
    s_above[tid] = (oy > 0 && x >= 0 && x < F.width) ? (short)frame[(long long)(oy - 1) * F.stride + x] : (short)0;
  } else if (tid >= 192) {
    const int yl = oy + tid - 192;
    s_left[tid - 192] = (ox > 0 && yl < F.height) ? (short)frame[(long long)yl * F.stride + ox - 1] : (short)0;
  }
}

// candidate list of one block: the eight modes of smallest cost seen so far, best first.  A new mode goes behind every entry of smaller or EQUAL
// cost, so of two modes of equal cost the earlier one keeps its place (TEncSearch::xUpdateCandList, TEncSearch.cpp:5385-5408)
__device__ __forceinline__ void cand_init(double (&cost)[8], uint8_t (&mode)[8])
{
#pragma unroll
  for (int i = 0; i < 8; ++i) { cost[i] = 1e300; mode[i] = 255; }
}
__device__ __forceinline__ void cand_insert(double (&cost)[8], uint8_t (&mode)[8], double c, int m)
{
  int pos = 8;
#pragma unroll
  for (int i = 7; i >= 0; --i) if (c < cost[i]) pos = i;
#pragma unroll
  for (int i = 7; i > 0; --i) if (i > pos) { cost[i] = cost[i - 1]; mode[i] = mode[i - 1]; }
#pragma unroll
  for (int i = 0; i < 8; ++i) if (i == pos) { cost[i] = c; mode[i] = (uint8_t)m; }
}

}  // namespace fhevc_fp
