// k_motion_coarse.hip -- one coarse motion centre per CTU from a 4:1 decimated picture pair (config 4: P slices), gfx950 only.
//
// What fhevc_motion_centres defines (include/fasthevc.h); HM has no counterpart: its predictor comes from the neighbouring PUs' coded vectors, which a
// source-only pass does not have.  Per CTU of frame f >= 1, searched in frame f - 1:
//   D_p(X, Y) = (sum of the 4x4 samples at (4X.., 4Y..) + 8) >> 4 over the floor(width / 4) x floor(height / 4) cells wholly inside the picture, a cell
//   coordinate outside that grid clamped to it; the CTU owns cells (16 cx + i, 16 cy + j), i, j < 16, of which those inside the grid count;
//   candidates d in [-Rc, Rc]^2 in raster order, strict "<":  sad(d) = (16 * sum |D_cur(X, Y) - D_ref(X + dx, Y + dy)|) >> (bit_depth - 8),
//   cost(d) = sad(d) + c[bits(4 dx) + bits(4 dy)] with the launch's FhevcMvBitCost and fhevc_mv_component_bits: the whole-sample vector 4 d against a
//   zero predictor.  Record: satd_zero = sad(0), satd_best, cost_best, (mvx, mvy) = 4 d.
//
// Mapping: workgroup (4 waves) = one CTU at a time, grid-stride.
//   * the decimated reference window ((16 + 2 Rc)^2 <= 44 x 44 cells) and the CTU's 16 x 16 current cells are built in LDS, one dword per cell.  A work item
//     is two horizontally adjacent cells: four rows of eight samples, each ONE 16-byte (uint8 planes: 8-byte) load where the plane's alignment allows it
//     -- a pair starts at a sample column that is a multiple of 8 --, scalar loads otherwise and for the pairs the grid's edge cuts (clamped cells);
//   * thread t takes candidates t, t + 256, ... (at most four of the <= 841) and walks the current cells once for all of them: the current cell is a
//     broadcast read, the four reference cells are at consecutive addresses across consecutive lanes;
//   * (cost, raster index) as one 64-bit key: the minimum over the wave by lane shuffles, over the four waves through LDS -- the smaller cost, at equal
//     cost the earlier candidate, which is what one thread walking the whole window with strict "<" finds (the merge of k_search_tile.h).
// Every global read is of a cell inside the grid, so of samples inside the picture; every LDS index depends on (Rc, t) alone.  The bit costs travel by value:
// no per-context state, nothing allocated, two launches with different QPs and ranges may be in flight on two streams.
#include "fhevc_internal.h"
#include "k_search_tile.h"   // SearchWork, sample_of

namespace {

constexpr int kSide = 16 + 2 * FHEVC_MOTION_COARSE_MAX_RANGE;   // 44 cells
constexpr int kPitch = kSide + 1;                               // odd: rows of the window start on different banks
constexpr int kPerThread = 4;                                   // (2 * 14 + 1)^2 = 841 candidates over 256 threads

// the sum of the 4x4 samples of cell (X, Y), which lies inside the grid
template <typename T>
__device__ __forceinline__ int coarse_cell(const T* plane, long long base, int stride, int X, int Y)
{
  int s = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long long row = base + (long long)(4 * Y + j) * stride + 4 * X;
#pragma unroll
    for (int k = 0; k < 4; ++k) s += sample_of(plane, row + k);
  }
  return s;
}

// ... of cells (X, Y) and (X + 1, Y), both inside the grid, X even: rows of eight samples from a column that is a multiple of 8
template <typename T>
__device__ __forceinline__ void coarse_cell_pair(const T* plane, long long base, int stride, int X, int Y, int& s0, int& s1)
{
  s0 = 0; s1 = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long long row = base + (long long)(4 * Y + j) * stride + 4 * X;
    const T* src = plane + row;
    if ((reinterpret_cast<uintptr_t>(src) & (8 * sizeof(T) - 1)) == 0) {
      if (sizeof(T) == 2) {
        const uint4 q = *reinterpret_cast<const uint4*>(src);
        s0 += (int)(short)q.x + ((int)q.x >> 16) + (int)(short)q.y + ((int)q.y >> 16);
        s1 += (int)(short)q.z + ((int)q.z >> 16) + (int)(short)q.w + ((int)q.w >> 16);
      } else {
        const uint2 q = *reinterpret_cast<const uint2*>(src);
        s0 += (int)__builtin_amdgcn_sad_u8(q.x, 0u, 0u);   // the sum of four bytes
        s1 += (int)__builtin_amdgcn_sad_u8(q.y, 0u, 0u);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) { s0 += sample_of(plane, row + k); s1 += sample_of(plane, row + 4 + k); }
    }
  }
}

// decimated cells Xa = 2 * pair and Xa + 1 of cell row Y (inside the grid) of one plane, cell columns clamped to the grid
template <typename T>
__device__ __forceinline__ void coarse_pair_clamped(const T* plane, long long base, int stride, int gw, int Xa, int Y, int& d0, int& d1)
{
  int s0, s1;
  if (Xa >= 0 && Xa + 1 < gw) coarse_cell_pair(plane, base, stride, Xa, Y, s0, s1);
  else {
    s0 = coarse_cell(plane, base, stride, min(max(Xa, 0), gw - 1), Y);
    s1 = coarse_cell(plane, base, stride, min(max(Xa + 1, 0), gw - 1), Y);
  }
  d0 = (s0 + 8) >> 4; d1 = (s1 + 8) >> 4;
}

template <typename T>
__global__ __launch_bounds__(256) void fhevc_motion_coarse_kernel(FhevcFrames F, int rc, FhevcMvBitCost cost, FhevcMotionNode* __restrict__ out)
{
  __shared__ int s_ref[kSide * kPitch];
  __shared__ int s_cur[16 * 16];
  __shared__ unsigned long long s_key[4];
  __shared__ unsigned s_zero;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int side = 2 * rc + 1, nmv = side * side, centre = (nmv - 1) >> 1, win = 16 + 2 * rc;
  const int gw = F.width >> 2, gh = F.height >> 2;
  const int shift = F.bit_depth - 8;
  const int total = SearchWork::total(F);
  const T* plane = reinterpret_cast<const T*>(F.luma);

  // this thread's candidates: where candidate m's cell (0, 0) sits in the window.  A slot past the last candidate reads the window's corner and is dropped
  int woff[kPerThread];
  unsigned vcost[kPerThread];
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int m = tid + 256 * k;
    const int my = m < nmv ? m / side : 0, mx = m < nmv ? m % side : 0;
    woff[k] = my * kPitch + mx;
    vcost[k] = cost.c[fhevc_mv_component_bits(4 * (mx - rc)) + fhevc_mv_component_bits(4 * (my - rc))];
  }

  for (int work = blockIdx.x; work < total; work += gridDim.x) {
    const SearchWork W(F, work);
    const int cx = W.cx, cy = W.cy;
    FhevcMotionNode* dst = out + W.oc(F);
    const int vw = min(16, gw - 16 * cx), vh = min(16, gh - 16 * cy);   // the CTU's cells inside the grid
    if (vw <= 0 || vh <= 0) {   // a picture whose last CTU column or row is narrower than one cell: nothing to compare
      if (tid == 0) { FhevcMotionNode o; o.satd_zero = o.satd_best = o.cost_best = 0xFFFFFFFFu; o.mvx = 0; o.mvy = 0; *dst = o; }
      continue;
    }
    __syncthreads();  // the previous CTU's readers are done
    // ---- the decimated reference window: cell rows 16 cy - rc .. + win, cell columns 16 cx - rc .. + win, clamped to the grid ----
    const int X0 = 16 * cx - rc, Y0 = 16 * cy - rc;
    const int p0 = X0 >> 1, pairs = ((X0 + win - 1) >> 1) - p0 + 1;
    for (int it = tid; it < win * pairs; it += 256) {
      const int wr = it / pairs, Xa = 2 * (p0 + it % pairs);
      int d0, d1;
      coarse_pair_clamped(plane, W.ref_base, F.stride, gw, Xa, min(max(Y0 + wr, 0), gh - 1), d0, d1);
      if (Xa >= X0) s_ref[wr * kPitch + Xa - X0] = d0;
      if (Xa + 1 < X0 + win) s_ref[wr * kPitch + Xa + 1 - X0] = d1;
    }
    // ---- the current cells: row j = tid >> 3, cells 2 (tid & 7) and the next; cells outside the grid are never read ----
    if (tid < 128 && (tid >> 3) < vh) {
      const int j = tid >> 3, i = 2 * (tid & 7);
      if (i + 1 < vw) {
        int d0, d1;
        coarse_pair_clamped(plane, W.cur_base, F.stride, gw, 16 * cx + i, 16 * cy + j, d0, d1);
        s_cur[j * 16 + i] = d0; s_cur[j * 16 + i + 1] = d1;
      } else if (i < vw) s_cur[j * 16 + i] = (coarse_cell(plane, W.cur_base, F.stride, 16 * cx + i, 16 * cy + j) + 8) >> 4;
    }
    __syncthreads();

    unsigned acc[kPerThread];
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) acc[k] = 0;
    for (int j = 0; j < vh; ++j)
      for (int i = 0; i < vw; ++i) {
        const int c = s_cur[j * 16 + i];
        const int* r = s_ref + j * kPitch + i;
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) acc[k] += (unsigned)abs(c - r[woff[k]]);
      }
    // this thread's candidates in raster order, strict "<"; an empty slot never wins
    unsigned long long key = ~0ull;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
      const int m = tid + 256 * k;
      const unsigned sad = (acc[k] << 4) >> shift;
      if (m == centre) s_zero = sad;
      const unsigned long long cand = ((unsigned long long)(sad + vcost[k]) << 32) | (unsigned)m;
      if (m < nmv && cand < key) key = cand;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const unsigned long long other = __shfl_xor(key, d);
      key = other < key ? other : key;
    }
    if (lane == 0) s_key[wave] = key;
    __syncthreads();
    if (tid == 0) {
      unsigned long long best = s_key[0];
#pragma unroll
      for (int w = 1; w < 4; ++w) best = s_key[w] < best ? s_key[w] : best;
      const unsigned c = (unsigned)(best >> 32), m = (unsigned)best;
      const int dx = (int)(m % (unsigned)side) - rc, dy = (int)(m / (unsigned)side) - rc;
      FhevcMotionNode o;
      o.satd_zero = s_zero;
      o.satd_best = c - cost.c[fhevc_mv_component_bits(4 * dx) + fhevc_mv_component_bits(4 * dy)];
      o.cost_best = c;
      o.mvx = (short)(4 * dx); o.mvy = (short)(4 * dy);
      *dst = o;
    }
  }
}

}  // namespace

hipError_t fhevc_launch_motion_coarse(const FhevcFrames& fr, int coarse_range, const FhevcMvBitCost& cost, FhevcMotionNode* d_centres, int num_cus, hipStream_t stream)
{
  static_assert((2 * FHEVC_MOTION_COARSE_MAX_RANGE + 1) * (2 * FHEVC_MOTION_COARSE_MAX_RANGE + 1) <= 256 * kPerThread, "candidates per thread");
  const long long total = (long long)(fr.row_end - fr.row_begin) * fr.ctus_x * (fr.num_frames - 1);
  if (total <= 0) return hipSuccess;
  if (coarse_range < 1 || coarse_range > FHEVC_MOTION_COARSE_MAX_RANGE || total > 0x7FFFFFFF) return hipErrorInvalidValue;
  const long long resident = 8ll * num_cus;   // 9 KB of LDS per workgroup
  const int grid = (int)(total < resident ? total : resident);
  if (fr.sample_bytes == 2) hipLaunchKernelGGL((fhevc_motion_coarse_kernel<int16_t>), dim3(grid), dim3(256), 0, stream, fr, coarse_range, cost, d_centres);
  else hipLaunchKernelGGL((fhevc_motion_coarse_kernel<uint8_t>), dim3(grid), dim3(256), 0, stream, fr, coarse_range, cost, d_centres);
  return hipGetLastError();
}
