// k_search_tile.h -- what the three integer motion-search kernels share (k_motion.hip: the 85 square CU nodes; k_motion_pu.hip: the 124 PUs whose
// sides are multiples of 8; k_motion_pu_small.hip: the 384 PUs with a 4-sample side).  All three run one mapping: workgroup (4 waves) = one CTU at
// a time, grid-stride; lane = one 8x8 tile whose 64 original samples stay in registers as 32 packed pairs; the reference window ((64 + 2R)^2
// samples, border replicated) staged in LDS once per CTU; the four waves split the vectors of the window in raster order and are merged by
// (cost, raster index).  Here, once: the geometry, the work decomposition, the staging loop, the tile load (k_refine_tile.h's too), a lane's
// displaced 8x8 block and its distortion, the merge, the output record, and the launch.  Each kernel keeps its reduction.
#pragma once
#include <type_traits>
#include "fhevc_internal.h"
#include "k_had8x8.h"

namespace {

// MR = the largest search range an instantiation is laid out for
template <int MR> struct SearchGeom {
  static constexpr int RP = 64 + 2 * MR + 8;  // LDS row pitch of the reference window in samples (multiple of 8: 16-byte row starts)
  static constexpr int WIN_ROWS = 64 + 2 * MR;
  static constexpr int REF_SAMPLES = WIN_ROWS * RP + 8;
  static constexpr int NMV_MAX = (2 * MR + 1) * (2 * MR + 1);
};

template <typename T>
__device__ __forceinline__ int sample_of(const T* plane, long long off) { return (int)plane[off]; }

// the window of one launch: (2 range + 1)^2 vectors in raster order, the zero vector in the middle -- or, in the centred searches, the CTU's centre:
// every vector of the window is then relative to the centre, and the kernel calls centre_on() per CTU
struct SearchRange {
  int range, side, nmv, centre, win, delta;
  __device__ __forceinline__ explicit SearchRange(int r)
    : range(r), side(2 * r + 1), nmv(side * side), centre((nmv - 1) >> 1), win(64 + 2 * r),
      delta((8 - (r & 7)) & 7) {}  // the window starts at column 64 cx - range: delta samples after a multiple of 8
  // ... at column 64 cx - range + px where the window lies around a centre whose horizontal component is px (px = 0: the value above)
  __device__ __forceinline__ void centre_on(int px) { delta = (px - range) & 7; }
  // vector m seen from tile (tx, ty): window column and row of the displaced block's first sample
  __device__ __forceinline__ void at(int m, int tx, int ty, int& col, int& row0) const
  {
    const int dy = m / side - range, dx = m % side - range;
    col = tx * 8 + range + dx + delta; row0 = ty * 8 + range + dy;
  }
};

// ---- the vector cost without a table per window (the MR = 64 layouts: (2 * 64 + 1)^2 entries would be 66 KB): the bits of vector m of the window in
// raster order, the index into the launch's FhevcMvBitCost (fhevc_mv_component_bits) ----
__device__ __forceinline__ int search_vector_bits(int m, const SearchRange& R)
{
  return fhevc_mv_component_bits(m % R.side - R.range) + fhevc_mv_component_bits(m / R.side - R.range);
}

// work item = one CTU of frame f >= 1 of the band, searched in frame f - 1; oc(): its index in the outputs
struct SearchWork {
  int f, cy, cx;
  long long cur_base, ref_base;
  __device__ __forceinline__ static int total(const FhevcFrames& F) { return (F.row_end - F.row_begin) * F.ctus_x * (F.num_frames - 1); }
  __device__ __forceinline__ SearchWork(const FhevcFrames& F, int work)
  {
    const int band_rows = F.row_end - F.row_begin, per_frame = band_rows * F.ctus_x;
    const int rem = work % per_frame;
    f = 1 + work / per_frame; cy = F.row_begin + rem / F.ctus_x; cx = rem % F.ctus_x;
    cur_base = (long long)f * F.frame_stride; ref_base = (long long)(f - 1) * F.frame_stride;
  }
  __device__ __forceinline__ long long oc(const FhevcFrames& F) const { return (long long)((f - 1) * (F.row_end - F.row_begin) + (cy - F.row_begin)) * F.ctus_x + cx; }
};

// ---- stage the reference window of CTU (cx, cy): rows cy*64 - R .. + win, columns cx*64 - R .. + win, coordinates clamped to the picture; the centred
// searches move the window by their centre (ox, oy), after R.centre_on(ox) ----
template <typename T, int RP>
__device__ __forceinline__ void search_stage_window(short* s_ref, const T* plane, long long ref_base, const FhevcFrames& F, int cx, int cy, const SearchRange& R, int tid,
                                                    int ox = 0, int oy = 0)
{
  // chunks of 8 samples starting at a column that is a multiple of 8 (delta = what the window's first column lacks to one): a chunk
  // inside the picture is ONE 16-byte (uint8 planes: 8-byte) load where the plane allows it, and one 16-byte LDS store
  const int chunks = (R.win + R.delta + 7) >> 3;
  for (int it = tid; it < R.win * chunks; it += 256) {
    const int wr = it / chunks, wc = (it - wr * chunks) * 8;
    const int py = min(max(cy * 64 - R.range + oy + wr, 0), F.height - 1);
    const int px0 = cx * 64 - R.range + ox - R.delta + wc;
    short v[8];
    const long long row = ref_base + (long long)py * F.stride;
    const T* src = plane + row + px0;
    if (px0 >= 0 && px0 + 8 <= F.width && (reinterpret_cast<uintptr_t>(src) & (8 * sizeof(T) - 1)) == 0) {
      if (sizeof(T) == 2) {
        const uint4 q = *reinterpret_cast<const uint4*>(src);
        *reinterpret_cast<uint4*>(s_ref + wr * RP + wc) = q;
        continue;
      } else {
        const uint2 q = *reinterpret_cast<const uint2*>(src);
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[k] = (short)((q.x >> (8 * k)) & 0xFF); v[4 + k] = (short)((q.y >> (8 * k)) & 0xFF); }
      }
    } else if (px0 >= 0 && px0 + 8 <= F.width) {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = (short)sample_of(plane, row + px0 + k);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = (short)sample_of(plane, row + min(max(px0 + k, 0), F.width - 1));
    }
    // one 16-byte store of whole dwords (no sub-dword LDS access): wc is a multiple of 8, the row pitch too
    uint4 q;
    q.x = ((unsigned)v[0] & 0xFFFFu) | ((unsigned)v[1] << 16); q.y = ((unsigned)v[2] & 0xFFFFu) | ((unsigned)v[3] << 16);
    q.z = ((unsigned)v[4] & 0xFFFFu) | ((unsigned)v[5] << 16); q.w = ((unsigned)v[6] & 0xFFFFu) | ((unsigned)v[7] << 16);
    *reinterpret_cast<uint4*>(s_ref + wr * RP + wc) = q;
  }
}

// ---- a lane's original 8x8 tile at (px, py) as 32 packed pairs (zeros where the tile is not wholly inside the picture) ----
template <typename T>
__device__ __forceinline__ void load_tile8x8(const T* plane, long long cur_base, const FhevcFrames& F, int px, int py, bool inside, unsigned (&O)[32])
{
  if (inside) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const long long row = cur_base + (long long)(py + j) * F.stride + px;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        O[4 * j + k] = ((unsigned)sample_of(plane, row + 2 * k) & 0xFFFFu) | ((unsigned)sample_of(plane, row + 2 * k + 1) << 16);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 32; ++i) O[i] = 0;
  }
}

// ---- the eight samples of window row r from column col on: five dword reads, and v_alignbit for odd columns makes pair k of the four ----
struct SearchRefRow {
  unsigned d[5], sh;
  __device__ __forceinline__ unsigned pair(int k) const { return __builtin_amdgcn_alignbit(d[k + 1], d[k], sh); }
};
template <int RP>
__device__ __forceinline__ SearchRefRow search_ref_row(const short* s_ref, int r, int col)
{
  SearchRefRow w;
  const unsigned* q = reinterpret_cast<const unsigned*>(s_ref) + ((r * RP + col) >> 1);
#pragma unroll
  for (int k = 0; k < 5; ++k) w.d[k] = q[k];
  w.sh = (unsigned)(col & 1) * 16u;  // uniform: R + dx
  return w;
}

// original minus the displaced block at (row0, col), as 8 rows x 4 packed pairs (bit depth <= 10)
template <int RP>
__device__ __forceinline__ void search_tile_diff(const short* s_ref, int row0, int col, const unsigned (&O)[32], unsigned (&D)[32])
{
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const SearchRefRow w = search_ref_row<RP>(s_ref, row0 + j, col);
#pragma unroll
    for (int k = 0; k < 4; ++k) D[4 * j + k] = pk_sub(O[4 * j + k], w.pair(k));
  }
}

// ---- the distortion of the lane's 8x8 tile against the displaced block at (row0, col); 0 where the tile is not inside the picture.
// PACKED = bit depth <= 10; SAD, else Hadamard SATD with xCalcHADs8x8's (sum + 2) >> 2 (TComRdCost.cpp:1747) ----
template <bool PACKED, bool SAD, int RP>
__device__ __forceinline__ unsigned search_tile8x8(const short* s_ref, int row0, int col, const unsigned (&O)[32], bool inside)
{
  unsigned t8;
  if (PACKED && SAD) {  // sum |org - ref| on pairs of unsigned 16-bit samples: v_sad_u16
    t8 = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const SearchRefRow w = search_ref_row<RP>(s_ref, row0 + j, col);
#pragma unroll
      for (int k = 0; k < 4; ++k) t8 = __builtin_amdgcn_sad_u16(O[4 * j + k], w.pair(k), t8);
    }
  } else if (PACKED) {
    unsigned D[32];
    search_tile_diff<RP>(s_ref, row0, col, O, D);
    t8 = had8x8_packed(D);
  } else {  // 32-bit (12-bit content): per-sample LDS reads
    int v[64];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const unsigned o = O[4 * j + (k >> 1)];
        const int os = (k & 1) ? (int)(short)(o >> 16) : (int)(short)(o & 0xFFFFu);
        v[8 * j + k] = os - (int)s_ref[(row0 + j) * RP + col + k];
      }
    if (SAD) {
      t8 = 0;
#pragma unroll
      for (int i = 0; i < 64; ++i) t8 += (unsigned)abs(v[i]);
    } else t8 = had8x8_wide(v);
  }
  if (SAD) return inside ? t8 : 0u;
  return inside ? ((t8 + 2) >> 2) : 0u;
}

// ---- the best (cost, vector index) of entry e over the four waves' arrays ([wave][entries of one wave = stride]): the smaller cost, at equal
// cost the earlier vector in raster order, which is what one wave walking the whole window with strict "<" finds.  Returns the winning wave ----
__device__ __forceinline__ int search_merge(const unsigned* s_cost, const unsigned* s_idx, int stride, int e, unsigned& c, unsigned& ix)
{
  int best = 0;
  c = s_cost[e]; ix = s_idx[e];
#pragma unroll
  for (int w = 1; w < 4; ++w) {
    const unsigned c2 = s_cost[w * stride + e], i2 = s_idx[w * stride + e];
    if (c2 < c || (c2 == c && i2 < ix)) { c = c2; ix = i2; best = w; }
  }
  return best;
}

// level (0: 64x64 .. 3: 8x8) and raster index inside the level of node 0 .. 84
__device__ __forceinline__ void search_node_level(int node, int& l, int& ni)
{
  if (node == 0) { l = 0; ni = 0; } else if (node < 5) { l = 1; ni = node - 1; } else if (node < 21) { l = 2; ni = node - 5; } else { l = 3; ni = node - 21; }
}
// a node (and every PU of it) is searched iff it lies wholly inside the picture: node (bx, by) of size n in CTU (cx, cy)
__device__ __forceinline__ bool search_node_inside(const FhevcFrames& F, int cx, int cy, int bx, int by, int n)
{
  return cx * 64 + bx * n + n <= F.width && cy * 64 + by * n + n <= F.height;
}
// the 16-byte output record (FhevcMotionNode) of a searched entry: the distortion at the best vector is its cost minus its vector cost
__device__ __forceinline__ uint4 search_record(unsigned zero, unsigned c, unsigned vc, unsigned ix, const SearchRange& R)
{
  const int mvx = (int)(ix % R.side) - R.range, mvy = (int)(ix / R.side) - R.range;
  return make_uint4(zero, c - vc, c, ((unsigned)mvx & 0xFFFFu) | ((unsigned)mvy << 16));
}
__device__ __forceinline__ uint4 search_record_outside() { return make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u); }

// ---- the centred searches (fhevc_motion_search_pu_centred): the CTU's centre P, of which only mvx / mvy are read (one dword: an entry is 4-byte aligned by its
// type, whatever else the caller's pointer is).  Candidates are P + d, d in [-R, R]^2; the vector cost is that of d (the predictor is P), so the window's table of
// the zero-centred search serves; a centre with a component outside +-FHEVC_MOTION_CENTRE_MAX marks every entry of its CTU and nothing is read for it ----
struct SearchNoCentres {};
template <bool CENTRED> using SearchCentres = typename std::conditional<CENTRED, const FhevcMotionNode*, SearchNoCentres>::type;
struct SearchCentre {
  int x, y;
  __device__ __forceinline__ SearchCentre() : x(0), y(0) {}
  __device__ __forceinline__ SearchCentre(const FhevcMotionNode* centres, long long oc)
  {
    const unsigned v = reinterpret_cast<const unsigned*>(centres + oc)[3];
    x = (int)(short)(v & 0xFFFFu); y = (int)(short)(v >> 16);
  }
  __device__ __forceinline__ bool in_range() const { return abs(x) <= FHEVC_MOTION_CENTRE_MAX && abs(y) <= FHEVC_MOTION_CENTRE_MAX; }
  // the record of a searched entry with its vector made absolute
  __device__ __forceinline__ uint4 absolute(uint4 rec) const
  {
    const int mvx = (int)(short)(rec.w & 0xFFFFu) + x, mvy = (int)(short)(rec.w >> 16) + y;
    rec.w = ((unsigned)mvx & 0xFFFFu) | ((unsigned)mvy << 16);
    return rec;
  }
};

// ---- launch: a persistent grid of k workgroups per CU (k_packed: the forms up to 10 bit, k_wide: the 32-bit form), no more than there are CTUs;
// launch(T(), packed, sad, grid) with T = int16_t (HM Pel planes) or uint8_t and the two switches as std::true_type / std::false_type ----
template <typename Launch>
hipError_t search_launch(const FhevcFrames& fr, bool args_ok, int num_cus, int k_packed, int k_wide, bool sad, Launch&& launch)
{
  const long long total = (long long)(fr.row_end - fr.row_begin) * fr.ctus_x * (fr.num_frames - 1);
  if (total <= 0) return hipSuccess;
  if (!args_ok) return hipErrorInvalidValue;
  const bool wide = fr.sample_bytes == 2 && fr.bit_depth > 10;
  const long long resident = (long long)(wide ? k_wide : k_packed) * num_cus;
  const int grid = (int)(total < resident ? total : resident);
  const std::true_type yes; const std::false_type no;
  hipError_t e;
  if (wide) e = sad ? launch(int16_t(), no, yes, grid) : launch(int16_t(), no, no, grid);
  else if (fr.sample_bytes == 2) e = sad ? launch(int16_t(), yes, yes, grid) : launch(int16_t(), yes, no, grid);
  else e = sad ? launch(uint8_t(), yes, yes, grid) : launch(uint8_t(), yes, no, grid);
  return e != hipSuccess ? e : hipGetLastError();
}

}  // namespace
