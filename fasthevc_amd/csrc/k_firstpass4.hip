// k_firstpass4.hip -- 35-mode intra first pass for the 256 4x4 PUs of a CTU, with the candidate lists selected on chip.  gfx950 only.
//
// Source-only twin of the first loop of TEncSearch::estIntraPredLumaQT as xCheckRDCostIntra(SIZE_NxN) runs it: four 4x4 PUs per 8x8 CU, each
// over all 35 modes with xCalcHADs4x4, the numModesForFullRD cheapest kept (TEncSearch.cpp:2233-2320).  Semantics are those of
// k_firstpass.hip at n = 4: reference samples from the ORIGINAL plane, 17 per PU, availability per 4-sample unit by coding order (CTU raster,
// z-order inside the CTU), HM's substitution walk, no smoothed line (c_filterThr[4x4] = 10 is never exceeded), the DC edge filter and the
// edge filter of modes 10 / 26, SATD = (sum|WHT4x4| + 1) >> 1 >> (bit_depth - 8), cost = satd + modeBits * sqrt(lambda) with strict '<'.
// Bit-exact against oracle/fhevc_oracle.c: fho_first_pass_node(n = 4).  A PU is valid iff its 8x8 CU lies wholly inside the picture.
//
// One workgroup (256 threads) per CTU, persistent over CTUs:
//   * the CTU, the row above it and the column left of it are staged in LDS exactly as the 85-node kernel stages them (stage_ctu);
//   * lane = one PU for the whole CTU: its 16 original samples and its 17 reference samples live in registers; the reference line
//     also goes to LDS (18 shorts = 9 dwords per PU: an odd dword pitch, so the 64 lanes of a wave, which always read the SAME offset
//     of their own line, hit 64 different banks);
//   * the mode loop is wave-uniform (planar, DC, the 16 horizontal, the 17 vertical modes in mode order): every index into the line is
//     scalar arithmetic, only availability and validity diverge.  Horizontal modes are evaluated in the transposed frame
//     (sum|WHT(X^T)| = sum|WHT(X)|): transposing the PU in registers is a renaming, nothing moves;
//   * the candidate list (k <= 8, best first, the earlier mode ahead of a later one of equal cost) is kept in registers while the modes
//     go by; per PU 16 bytes (best) and k bytes (list) reach HBM.  The (PU, mode) table is written only for the parity entry point.
// 32-bit integer VALU throughout: at 4x4 the Hadamard is 64 add/sub per mode, a third of the work per mode next to prediction, residual
// and the list, so one form serves 8 to 12 bit.
#include "fhevc_internal.h"
#include "k_firstpass_common.h"

namespace {

using fhevc_fp::cand_init;
using fhevc_fp::cand_insert;
using fhevc_fp::stage_ctu;
using fhevc_fp::staged;
using fhevc_fp::unit_available;

constexpr int kPitch = 18;  // shorts per PU line: 17 samples + one zero that a tap of weight 0 may touch (angle 32, last row)

__constant__ int c_angTable4[9] = { 0, 2, 5, 9, 13, 17, 21, 26, 32 };
__constant__ int c_invAngTable4[9] = { 0, 4096, 1638, 910, 630, 482, 390, 315, 256 };

// sum|WHT4x4(d)|, rows then columns
__device__ __forceinline__ unsigned had4x4(int (&d)[16])
{
#pragma unroll
  for (int y = 0; y < 4; ++y) {
    const int a = d[4 * y] + d[4 * y + 1], b = d[4 * y] - d[4 * y + 1], c = d[4 * y + 2] + d[4 * y + 3], e = d[4 * y + 2] - d[4 * y + 3];
    d[4 * y] = a + c; d[4 * y + 1] = b + e; d[4 * y + 2] = a - c; d[4 * y + 3] = b - e;
  }
  unsigned s = 0;
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    const int a = d[x] + d[4 + x], b = d[x] - d[4 + x], c = d[8 + x] + d[12 + x], e = d[8 + x] - d[12 + x];
    s += (unsigned)(abs(a + c) + abs(b + e) + abs(a - c) + abs(b - e));
  }
  return s;
}

// what every mode ends in: SATD against the prediction P (FRAME_T: P is in the transposed frame), cost, best / list / parity output
struct Pick {
  double cost[8];
  uint8_t mode[8];
  unsigned satd0;  // SATD of the entry at the head of the list
};

template <bool FRAME_T>
__device__ __forceinline__ void finish_mode(const int (&O)[16], const int (&P)[16], int m, int shift, double mode_cost, Pick& pk, FhevcNodeCost* all)
{
  int d[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) d[i] = (FRAME_T ? O[(i & 3) * 4 + (i >> 2)] : O[i]) - P[i];
  const unsigned sd = ((had4x4(d) + 1) >> 1) >> shift;
  const double c = __dadd_rn((double)sd, mode_cost);
  if (c < pk.cost[0]) pk.satd0 = sd;
  cand_insert(pk.cost, pk.mode, c, m);
  if (all != nullptr) { FhevcNodeCost r; r.satd = sd; r.mode = (unsigned)m; r.cost = c; all[m] = r; }
}

// an angular mode in its own frame (VER: rows are picture rows; otherwise rows are picture columns): main(i) = r[SGN * i], side(i) = r[-SGN * i]
template <bool VER>
__device__ __forceinline__ void angular4(const short* r, int m, int maxval, int (&P)[16])
{
  constexpr int SGN = VER ? 1 : -1;
  const int ang_mode = VER ? m - 26 : 10 - m;
  const int abs_mode = abs(ang_mode);
  const int angle = ang_mode < 0 ? -c_angTable4[abs_mode] : c_angTable4[abs_mode];
  const int inv_angle = c_invAngTable4[abs_mode];
#pragma unroll
  for (int yy = 0; yy < 4; ++yy) {
    const int delta = (yy + 1) * angle;
    const int di = delta >> 5, df = delta & 31;
    int mv[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int i = di + 1 + k;  // HM's refMain with its projected extension (TComPrediction.cpp:278-300) for i < 0
      mv[k] = r[i >= 0 ? SGN * i : -SGN * ((128 - i * inv_angle) >> 8)];
    }
#pragma unroll
    for (int xx = 0; xx < 4; ++xx) P[4 * yy + xx] = ((32 - df) * mv[xx] + df * mv[xx + 1] + 16) >> 5;
  }
  if (angle == 0) {  // edge filter of the pure vertical / horizontal mode (first column of its frame)
    const int tl = r[0];
#pragma unroll
    for (int yy = 0; yy < 4; ++yy) P[4 * yy] = min(maxval, max(0, P[4 * yy] + ((r[-SGN * (yy + 1)] - tl) >> 1)));
  }
}

template <typename T>
__global__ __launch_bounds__(256) void fhevc_first_pass4_kernel(FhevcFrames F, double sqrt_lambda, int num_modes, FhevcNodeCost* __restrict__ out,
                                                                uint8_t* __restrict__ out_modes, FhevcNodeCost* __restrict__ out_all)
{
  __shared__ __attribute__((aligned(16))) short s_org[64 * 64];
  __shared__ short s_above[132], s_left[64];
  __shared__ short s_linebuf[2 + 256 * kPitch];  // line of PU t at 2 + t * kPitch: [0..7] left column bottom to top, [8] TL, [9..16] row above, [17] = 0

  const int tid = threadIdx.x;
  const int band_rows = F.row_end - F.row_begin;
  const int per_frame = band_rows * F.ctus_x;
  const int total = per_frame * F.num_frames;
  const int bd = F.bit_depth;
  const int ux = tid & 15, uy = tid >> 4;  // raster 16x16 of 4x4 units: the depth map's unit order
  short* const line = s_linebuf + 2 + tid * kPitch;
  if (tid == 0) { s_linebuf[0] = 0; s_linebuf[1] = 0; }  // what PU 0's horizontal modes touch with weight 0
  line[17] = 0;
  // mode bits 2 / 3 / 6 (planar; DC and vertical; the rest) times sqrt(lambda), in the oracle's own operation order
  const double cost2 = __dmul_rn(2.0, sqrt_lambda), cost3 = __dmul_rn(3.0, sqrt_lambda), cost6 = __dmul_rn(6.0, sqrt_lambda);

  for (int work = blockIdx.x; work < total; work += gridDim.x) {
    const int f = work / per_frame;
    const int rem = work - f * per_frame;
    const int cy = F.row_begin + rem / F.ctus_x, cx = rem % F.ctus_x;
    const T* frame = reinterpret_cast<const T*>(F.luma) + (long long)f * F.frame_stride;
    const int ox = cx * 64, oy = cy * 64;
    stage_ctu<T>(frame, F, ox, oy, tid, s_org, s_above, s_left);
    __syncthreads();

    const int x0 = ox + 4 * ux, y0 = oy + 4 * uy;
    // HM codes NxN only in whole 8x8 CUs
    const bool valid = (ox + (ux >> 1) * 8 + 8 <= F.width) && (oy + (uy >> 1) * 8 + 8 <= F.height);
    const long long pu = ((long long)(f * band_rows + (cy - F.row_begin)) * F.ctus_x + cx) * 256 + tid;
    FhevcNodeCost* const all = out_all != nullptr ? out_all + pu * 35 : nullptr;
    Pick pk;
    cand_init(pk.cost, pk.mode);
    pk.satd0 = 0xFFFFFFFFu;

    if (valid) {
      // ---- reference samples: five units in HM's walk order (below-left, left, the top-left corner, above, above-right) ----
      const bool av[5] = { unit_available(x0 - 4, y0 + 4, x0, y0, F.width, F.height, F.ctus_x), unit_available(x0 - 4, y0, x0, y0, F.width, F.height, F.ctus_x),
                           unit_available(x0 - 4, y0 - 4, x0, y0, F.width, F.height, F.ctus_x), unit_available(x0, y0 - 4, x0, y0, F.width, F.height, F.ctus_x),
                           unit_available(x0 + 4, y0 - 4, x0, y0, F.width, F.height, F.ctus_x) };
      int ref[17];
#pragma unroll
      for (int i = 0; i < 8; ++i) ref[i] = av[i >> 2] ? staged(s_org, s_above, s_left, x0 - 1, y0 + 7 - i, ox, oy) : 0;
      ref[8] = av[2] ? staged(s_org, s_above, s_left, x0 - 1, y0 - 1, ox, oy) : 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) ref[9 + i] = av[3 + (i >> 2)] ? staged(s_org, s_above, s_left, x0 + i, y0 - 1, ox, oy) : 0;
      // HM's substitution walk (TComPattern.cpp:461-524): unavailable units copy the last sample before them, leading unavailable units the
      // first available sample; nothing available -> 1 << (bd - 1)
      if (!(av[0] || av[1] || av[2] || av[3] || av[4])) {
#pragma unroll
        for (int i = 0; i < 17; ++i) ref[i] = 1 << (bd - 1);
      } else {
        int prev = av[0] ? ref[0] : (av[1] ? ref[4] : (av[2] ? ref[8] : (av[3] ? ref[9] : ref[13])));
#pragma unroll
        for (int u = 0; u < 5; ++u) {
          const int s = u <= 2 ? 4 * u : 4 * u - 3, c = (u == 2) ? 1 : 4;
          if (av[u]) prev = ref[s + c - 1];
          else {
#pragma unroll
            for (int i = 0; i < c; ++i) ref[s + i] = prev;
          }
        }
      }
#pragma unroll
      for (int i = 0; i < 17; ++i) line[i] = (short)ref[i];
      int O[16];
#pragma unroll
      for (int y = 0; y < 4; ++y) {
        const uint2 q = *reinterpret_cast<const uint2*>(&s_org[(4 * uy + y) * 64 + 4 * ux]);
        O[4 * y] = (int)(short)(q.x & 0xFFFF); O[4 * y + 1] = (int)(short)(q.x >> 16);
        O[4 * y + 2] = (int)(short)(q.y & 0xFFFF); O[4 * y + 3] = (int)(short)(q.y >> 16);
      }
      const int shift = bd - 8, maxval = (1 << bd) - 1;
      int P[16];

      // ---- mode 0, planar (TComPrediction.cpp:731-792), n = 4: top[x] = ref[9 + x], left[y] = ref[7 - y] ----
      {
        const int topRight = ref[13], bottomLeft = ref[3];
#pragma unroll
        for (int y = 0; y < 4; ++y)
#pragma unroll
          for (int x = 0; x < 4; ++x) {
            const int left = ref[7 - y], top = ref[9 + x];
            const int hor = (left << 2) + 4 + (x + 1) * (topRight - left);
            const int ver = (top << 2) + (y + 1) * (bottomLeft - top);
            P[4 * y + x] = (hor + ver) >> 3;
          }
        finish_mode<false>(O, P, 0, shift, cost2, pk, all);
      }
      // ---- mode 1, DC with its edge filter (n <= 16) ----
      {
        int sum = 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) sum += ref[9 + i] + ref[7 - i];
        const int dc = sum >> 3;
#pragma unroll
        for (int i = 0; i < 16; ++i) P[i] = dc;
        P[0] = (ref[9] + ref[7] + 2 * dc + 2) >> 2;
#pragma unroll
        for (int x = 1; x < 4; ++x) P[x] = (ref[9 + x] + 3 * dc + 2) >> 2;
#pragma unroll
        for (int y = 1; y < 4; ++y) P[4 * y] = (ref[7 - y] + 3 * dc + 2) >> 2;
        finish_mode<false>(O, P, 1, shift, cost3, pk, all);
      }
      // ---- modes 2..17 horizontal (transposed frame), 18..34 vertical; the loop counter is wave-uniform ----
      const short* const r = line + 8;  // r[0] = TL, r[+i] above, r[-j] left
#pragma unroll 1
      for (int m = 2; m < 18; ++m) {
        angular4<false>(r, m, maxval, P);
        finish_mode<true>(O, P, m, shift, cost6, pk, all);
      }
#pragma unroll 1
      for (int m = 18; m < 35; ++m) {
        angular4<true>(r, m, maxval, P);
        finish_mode<false>(O, P, m, shift, m == 26 ? cost3 : cost6, pk, all);
      }
    } else if (all != nullptr) {
      FhevcNodeCost e; e.satd = 0xFFFFFFFFu; e.mode = 255; e.cost = -1.0;
      for (int m = 0; m < 35; ++m) all[m] = e;
    }

    if (out != nullptr) {
      FhevcNodeCost b;
      b.satd = pk.satd0; b.mode = pk.mode[0]; b.cost = valid ? pk.cost[0] : -1.0;
      out[pu] = b;
    }
    if (out_modes != nullptr) {
#pragma unroll
      for (int i = 0; i < 8; ++i) if (i < num_modes) out_modes[pu * num_modes + i] = pk.mode[i];
    }
    __syncthreads();  // the next CTU is staged over s_org
  }
}

}  // namespace

hipError_t fhevc_launch_first_pass4(const FhevcFrames& fr, double sqrt_lambda, int num_modes, FhevcNodeCost* d_best, uint8_t* d_modes, FhevcNodeCost* d_all,
                                    hipStream_t stream)
{
  const long long total = (long long)(fr.row_end - fr.row_begin) * fr.ctus_x * fr.num_frames;
  if (total <= 0) return hipSuccess;
  const int grid = (int)(total < 2048 ? total : 2048);
  if (fr.sample_bytes == 2) hipLaunchKernelGGL((fhevc_first_pass4_kernel<int16_t>), dim3(grid), dim3(256), 0, stream, fr, sqrt_lambda, num_modes, d_best, d_modes, d_all);
  else hipLaunchKernelGGL((fhevc_first_pass4_kernel<uint8_t>), dim3(grid), dim3(256), 0, stream, fr, sqrt_lambda, num_modes, d_best, d_modes, d_all);
  return hipGetLastError();
}
