// k_wide_tile.h -- what the two byte-SAD searches at HM's own SearchRange share (k_motion_wide.hip: the 85 square CU nodes; k_motion_pu_wide.hip: the
// 124 PUs and the 384 small PUs with them): the window's geometry in LDS, v_qsad_pk_u16_u8 with its early-clobber constraint, the key-building
// multiply-adds, the wave minimum, and the staging of the window and of the CTU's own bytes.  8-bit content only.
#pragma once
#include "fhevc_internal.h"

namespace {

constexpr int WR = FHEVC_MOTION_WIDE_MAX_RANGE;   // 64
constexpr int WP = 64 + 2 * WR + 4;               // window pitch in bytes: 196 = 49 dwords (odd: rows 8 apart land 8 banks apart)
constexpr int WROWS = 64 + 2 * WR;

typedef unsigned long long u64;

// (the destination registers must not overlap ANY source, the accumulator included: the hardware writes the low dword before it has read the
//  sources for the high one -- with an overlapping allocation results 2 and 3 come out wrong, tools/probes/probe_qsad.hip; hence "=&v")
__device__ __forceinline__ u64 qsad(u64 ref8, unsigned cur4, u64 acc)
{
  u64 d;
  asm("v_qsad_pk_u16_u8 %0, %1, %2, %3" : "=&v"(d) : "v"(ref8), "s"(cur4), "v"(acc));
  return d;
}
// (lo / hi half of a) * m + c
__device__ __forceinline__ unsigned mad_lo16(unsigned a, unsigned m, unsigned c)
{
  unsigned d;
  asm("v_mad_u32_u16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(m), "v"(c));
  return d;
}
__device__ __forceinline__ unsigned mad_hi16(unsigned a, unsigned m, unsigned c)
{
  unsigned d;
  asm("v_mad_u32_u16 %0, %1, %2, %3 op_sel:[1,0,0,0]" : "=v"(d) : "v"(a), "v"(m), "v"(c));
  return d;
}
// minimum over the wave (every lane of the wave ends with it; uniform)
__device__ __forceinline__ unsigned wave_min_u32(unsigned v)
{
  v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
  v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
  v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x141, 0xF, 0xF, false));  // row_half_mirror
  v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x140, 0xF, 0xF, false));  // row_mirror
  const unsigned a = (unsigned)__builtin_amdgcn_readlane((int)v, 0), b = (unsigned)__builtin_amdgcn_readlane((int)v, 16);
  const unsigned c = (unsigned)__builtin_amdgcn_readlane((int)v, 32), d = (unsigned)__builtin_amdgcn_readlane((int)v, 48);
  return min(min(a, b), min(c, d));
}

// ---- stage: the reference window of CTU (cx, cy) (coordinates clamped to the picture = replicated border) and the CTU's own samples, as bytes.
// T = int16_t (HM Pel planes holding 8-bit content) or uint8_t ----
template <typename T>
__device__ __forceinline__ void wide_stage(unsigned char* s_ref, unsigned char* s_cur, const T* plane, const FhevcFrames& F, int cx, int cy, int range,
                                           int win_rows, int win_cols, long long cur_base, long long ref_base, int tid)
{
  // chunks of 8 columns starting at a multiple of 8 picture columns (delta = what the window's first column lacks to one): a chunk inside
  // the picture is one 16-byte (uint8 planes: 8-byte) load; its bytes land at window columns wc - delta .. (two dword LDS stores when
  // delta is a multiple of 4, bytes otherwise)
  const int delta = (8 - (range & 7)) & 7;
  const int chunks = (win_cols + delta + 7) >> 3;
  for (int it = tid; it < win_rows * chunks; it += 256) {
    const int wr = it / chunks, wc = (it - wr * chunks) * 8 - delta;   // window column of the chunk's first sample (may be < 0)
    const int py = min(max(cy * 64 - range + wr, 0), F.height - 1);
    const long long row = ref_base + (long long)py * F.stride;
    const int px0 = cx * 64 - range + wc;
    unsigned lo = 0, hi = 0;
    const T* src = plane + row + px0;
    if (px0 >= 0 && px0 + 8 <= F.width && (reinterpret_cast<uintptr_t>(src) & (8 * sizeof(T) - 1)) == 0) {
      if (sizeof(T) == 2) {
        const uint4 q = *reinterpret_cast<const uint4*>(src);
        lo = __builtin_amdgcn_perm(q.y, q.x, 0x06040200u); hi = __builtin_amdgcn_perm(q.w, q.z, 0x06040200u);   // low bytes of the 16-bit samples
      } else {
        const uint2 q = *reinterpret_cast<const uint2*>(src);
        lo = q.x; hi = q.y;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        lo |= ((unsigned)plane[row + min(max(px0 + k, 0), F.width - 1)] & 0xFFu) << (8 * k);
        hi |= ((unsigned)plane[row + min(max(px0 + 4 + k, 0), F.width - 1)] & 0xFFu) << (8 * k);
      }
    }
    unsigned char* dst = s_ref + wr * WP + wc;
    if ((delta & 3) == 0) {
      if (wc >= 0 && wc + 4 <= WP) *reinterpret_cast<unsigned*>(dst) = lo;
      if (wc + 4 >= 0 && wc + 8 <= WP) *reinterpret_cast<unsigned*>(dst + 4) = hi;
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (wc + k >= 0 && wc + k < WP) dst[k] = (unsigned char)(((k < 4 ? lo : hi) >> (8 * (k & 3))) & 0xFFu);
    }
  }
  for (int it = tid; it < 64 * 16; it += 256) {
    const int y = it >> 4, x = (it & 15) * 4;
    const int py = min(cy * 64 + y, F.height - 1);
    const long long row = cur_base + (long long)py * F.stride;
    unsigned v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) v |= ((unsigned)plane[row + min(cx * 64 + x + k, F.width - 1)] & 0xFFu) << (8 * k);
    *reinterpret_cast<unsigned*>(s_cur + y * 64 + x) = v;
  }
}

}  // namespace
