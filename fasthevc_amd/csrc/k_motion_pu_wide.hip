// k_motion_pu_wide.hip -- the integer full search of config 4 at HM's own SearchRange (up to +-64) for ALL 593 entries of a CTU: the 85 square CU
// nodes, the 124 PUs whose sides are multiples of 8 and the 384 PUs with a 4-sample side; SAD distortion, 8-bit content; gfx950 only.
//
// Same definition as k_motion_pu.hip / k_motion_pu_small.hip in their SAD mode (the twin of TEncSearch::xPatternSearch on a w x h pattern: raster
// order, strict "<", cost = SAD + getCostOfVectorWithPredictor with a zero predictor, border replicated), in k_motion_wide.hip's layout
// (k_wide_tile.h): a lane is a block of DB dy x 4 dx VECTORS, the original bytes sit in SGPRs, the window is staged as bytes, and
// v_qsad_pk_u16_u8 adds four SADs of a 4-byte group to four packed 16-bit accumulators.  What is new is where the rectangles come from:
//
//  * qsad(w01, clo[r]) and qsad(w12, chi[r]) are the SADs of the LEFT and RIGHT 4-sample halves of tile row r.  Accumulated separately for rows 0-3
//    and rows 4-7 they are the tile's four 4x4 QUADRANT SADs (each <= 4 080, packed): q00 q01 / q10 q11.  From them the tile's 8x4 / 4x8 PUs and
//    the tile itself; over the four tiles of a 16x16 block its 2NxN / Nx2N parts and the quarter strips of its four AMP shapes (16x4, 4x16); SAD is
//    additive and the shift is 0 at 8 bit, so every three-quarter part is the node's sum minus the quarter's.
//  * the 32- and 64-level PUs are running sums over the z-order walk: per 32x32 quadrant the node, its top half, its left half and the four quarter
//    strips (sums of the 16x16 blocks' halves); per CTU the same seven, built from the 32-level ones as each quadrant completes.
//  * minima: everything up to 16x16 keeps keys (cost << 15 | raster index) in 32 bits (cost < 2^17), reduced by a wave minimum and ONE LDS atomic per
//    wave and entry; every entry of the 32x32 and 64x64 nodes takes 64-bit keys (cost << 32 | raster index), first-found inside the lane, one LDS
//    atomic per lane.  The smallest key IS HM's first-found minimum in raster order.
//  * the vector cost comes from the exp-Golomb bits of the two components and the 40 bit costs that travel with the launch (FhevcMvBitCost): no
//    table in HBM, no state between calls.
//  * the SAD at the zero vector: the 256 4x4 blocks of the CTU, one thread each, summed per entry's rectangle when the entry is written.
//
// The register file is what sizes the instantiations: FAM (1 = nodes | 2 = PUs | 4 = small PUs) removes the sums and keys of a family that is not
// asked for, and DB is chosen per FAM so that nothing spills: seven running sums per upper level times 4 DB vectors per lane is what
// the PUs cost, four accumulators per dy instead of one what the small PUs cost.
//
// Workgroup (4 waves) = one CTU at a time, grid-stride; two workgroups per CU.
#include "fhevc_internal.h"
#include "k_wide_tile.h"

namespace {

constexpr int E_PU = FHEVC_NODES, E_SMALL = FHEVC_NODES + FHEVC_PUS, ENTRIES = FHEVC_NODES + FHEVC_PUS + FHEVC_PUS_SMALL;   // 85, 209, 593
constexpr int KEYS64 = 5 + 60;   // the nodes 0..4, then their 12 PUs each, in output order

// entry e of the 593 -> its rectangle inside the CTU in units of 4 samples, and its CU node's (TComDataCU::getPartIndexAndSize)
__device__ __forceinline__ void wide_entry_rect(int e, int& x, int& y, int& w, int& h, int& nx, int& ny, int& n)
{
  int node, shape = -1, part = 0;
  if (e < E_PU) node = e;
  else if (e < E_SMALL) {
    const int p = e - E_PU;
    if (p < 60) { node = p / 12; shape = (p % 12) >> 1; } else { node = 5 + ((p - 60) >> 2); shape = ((p - 60) & 3) >> 1; }
    part = p & 1;
  } else {
    const int q = e - E_SMALL;
    if (q < 128) { node = 5 + (q >> 3); shape = 2 + ((q & 7) >> 1); } else { node = 21 + ((q - 128) >> 2); shape = ((q - 128) & 3) >> 1; }
    part = q & 1;
  }
  const int l = node == 0 ? 0 : node < 5 ? 1 : node < 21 ? 2 : 3;
  const int ni = node - (l == 0 ? 0 : l == 1 ? 1 : l == 2 ? 5 : 21), cnt = 1 << l;
  n = 16 >> l; nx = (ni % cnt) * n; ny = (ni / cnt) * n;
  x = nx; y = ny; w = n; h = n;
  if (shape < 0) return;
  const int cut = shape < 2 ? n / 2 : (shape == 2 || shape == 4) ? n / 4 : 3 * n / 4;
  if (shape == 0 || shape == 2 || shape == 3) { h = part ? n - cut : cut; y += part ? cut : 0; }
  else { w = part ? n - cut : cut; x += part ? cut : 0; }
}

// T = int16_t (HM Pel planes holding 8-bit content) or uint8_t; FAM: the families of this instantiation; DB: dy per block of vectors
template <typename T, int FAM, int DB>
__global__ __launch_bounds__(256, 2) void fhevc_motion_pu_wide_kernel(FhevcFrames F, int range, FhevcMvBitCost bitc, FhevcMotionNode* __restrict__ out_nodes,
                                                                    FhevcMotionNode* __restrict__ out_pus, FhevcMotionNode* __restrict__ out_small)
{
  constexpr bool N = (FAM & 1) != 0, P = (FAM & 2) != 0, S = (FAM & 4) != 0;
  constexpr int NV = 4 * DB;       // vectors per lane and round
  constexpr int NA = S ? 4 : 1;    // accumulators per dy: the tile's quadrants, or the tile
  __shared__ __attribute__((aligned(16))) unsigned char s_ref[(WROWS + 1) * WP];
  __shared__ __attribute__((aligned(16))) unsigned char s_cur[64 * 64];
  __shared__ unsigned s_key32[ENTRIES], s_zq[256], s_bitc[FHEVC_MV_BIT_COSTS];
  __shared__ u64 s_key64[KEYS64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int band_rows = F.row_end - F.row_begin;
  const int per_frame = band_rows * F.ctus_x;
  const int total = per_frame * (F.num_frames - 1);
  const int side = 2 * range + 1;
  const int win_rows = 64 + 2 * range, win_cols = 64 + 2 * range + 3;   // + the columns the last dx group reads past +R
  const int ng = (side + 3) >> 2, ndb = (side + DB - 1) / DB, items = ng * ndb;
  const int rounds = (items + 255) >> 8;
  const T* plane = reinterpret_cast<const T*>(F.luma);
  if (tid < FHEVC_MV_BIT_COSTS) s_bitc[tid] = bitc.c[tid];   // visible behind the first barrier of the CTU loop

  for (int work = blockIdx.x; work < total; work += gridDim.x) {
    const int f = 1 + work / per_frame;
    const int rem = work % per_frame;
    const int cy = F.row_begin + rem / F.ctus_x, cx = rem % F.ctus_x;
    const long long cur_base = (long long)f * F.frame_stride, ref_base = (long long)(f - 1) * F.frame_stride;
    __syncthreads();  // the previous CTU's readers are done
    wide_stage(s_ref, s_cur, plane, F, cx, cy, range, win_rows, win_cols, cur_base, ref_base, tid);
    for (int e = tid; e < ENTRIES; e += 256) s_key32[e] = 0xFFFFFFFFu;
    if (tid < KEYS64) s_key64[tid] = ~0ull;
    __syncthreads();
    // ---- the SAD at vector (0, 0) of every 4x4 block of the CTU (0 where its tile is not inside the picture, as in the search) ----
    {
      const int qx = tid & 15, qy = tid >> 4;
      const bool inside = (cx * 64 + (qx >> 1) * 8 + 8 <= F.width) && (cy * 64 + (qy >> 1) * 8 + 8 <= F.height);
      unsigned z = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned char* c = s_cur + (qy * 4 + j) * 64 + qx * 4;
        const unsigned char* r = s_ref + (qy * 4 + j + range) * WP + qx * 4 + range;
#pragma unroll
        for (int i = 0; i < 4; ++i) z += (unsigned)abs((int)c[i] - (int)r[i]);
      }
      s_zq[tid] = inside ? z : 0u;
    }
    // ---- the search ----
    for (int round = 0; round < rounds; ++round) {
      const int item = min(tid + 256 * round, items - 1);   // spare lanes of the last round repeat the last item
      const int db = item / ng, gx = item - db * ng;
      const int dyb = min(-range + DB * db, range - (DB - 1)), dx0 = -range + 4 * gx;
      // per vector (d, k): addend = cost << 15 | raster index; multiplier per k: 32768, or 0 past +R (then the addend is all ones)
      unsigned addend[NV], mul[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) mul[k] = (dx0 + k <= range) ? 32768u : 0u;
#pragma unroll
      for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int dx = min(dx0 + k, range), dy = dyb + d;   // (the launcher keeps 2 range + 1 >= DB: dyb >= -range)
          const unsigned ras = (unsigned)((dy + range) * side + dx + range);
          const unsigned vc = s_bitc[fhevc_mv_component_bits(dx) + fhevc_mv_component_bits(dy)];
          addend[4 * d + k] = (dx0 + k <= range) ? ((vc << 15) | ras) : 0xFFFFFFFFu;
        }
      // 32-bit keys of DB x 4 packed sums (pk[2 d]: dx 0, 1; pk[2 d + 1]: dx 2, 3): lane minimum, wave minimum, one atomic per wave
      auto emit32 = [&](int e, const unsigned (&pk)[2 * DB]) {
        unsigned m = 0xFFFFFFFFu;
#pragma unroll
        for (int d = 0; d < DB; ++d) {
          const unsigned lo = pk[2 * d], hi = pk[2 * d + 1];
          const unsigned k0 = mad_lo16(lo, mul[0], addend[4 * d + 0]), k1 = mad_hi16(lo, mul[1], addend[4 * d + 1]);
          const unsigned k2 = mad_lo16(hi, mul[2], addend[4 * d + 2]), k3 = mad_hi16(hi, mul[3], addend[4 * d + 3]);
          m = min(min(m, k0), min(min(k1, k2), k3));
        }
        m = wave_min_u32(m);
        if (lane == 0) atomicMin(&s_key32[e], m);
      };
      // 64-bit keys of NV 32-bit sums: first-found inside the lane (its vectors are in raster order), one atomic per lane
      auto emit64 = [&](int slot, const unsigned (&v32)[NV]) {
        unsigned bh = 0xFFFFFFFFu, bl = 0;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          const unsigned h = (addend[v] != 0xFFFFFFFFu) ? v32[v] + (addend[v] >> 15) : 0xFFFFFFFFu;
          if (h < bh) { bh = h; bl = addend[v] & 0x7FFFu; }
        }
        atomicMin(&s_key64[slot], ((u64)bh << 32) | bl);
      };
      auto unpack = [&](const unsigned (&pk)[2 * DB], unsigned (&v32)[NV]) {
#pragma unroll
        for (int d = 0; d < DB; ++d) {
          v32[4 * d + 0] = pk[2 * d] & 0xFFFFu; v32[4 * d + 1] = pk[2 * d] >> 16;
          v32[4 * d + 2] = pk[2 * d + 1] & 0xFFFFu; v32[4 * d + 3] = pk[2 * d + 1] >> 16;
        }
      };
      // the two parts of a shape of an upper-level node from the node's sum and one part's: slots base, base + 1
      auto emit64_parts = [&](int base, const unsigned (&node)[NV], const unsigned (&part)[NV], bool part_is_first) {
        unsigned rest[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) rest[v] = node[v] - part[v];
        emit64(base + (part_is_first ? 0 : 1), part);
        emit64(base + (part_is_first ? 1 : 0), rest);
      };

      const unsigned char* lane_ref = s_ref + (dyb + range) * WP + 4 * gx;
      // running sums of the 32x32 quadrant and of the CTU: node, top half, left half (32-bit), the quarter strips U D L R (32-level: packed)
      unsigned n32[NV], t32[P ? NV : 1], l32[P ? NV : 1], u32p[P ? 2 * DB : 1], d32p[P ? 2 * DB : 1], a32p[P ? 2 * DB : 1], r32p[P ? 2 * DB : 1];
      unsigned n64[NV], t64[P ? NV : 1], l64[P ? NV : 1], u64s[P ? NV : 1], d64s[P ? NV : 1], a64s[P ? NV : 1], r64s[P ? NV : 1];
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        n32[i] = 0; n64[i] = 0;
        if constexpr (P) { t32[i] = 0; l32[i] = 0; t64[i] = 0; l64[i] = 0; u64s[i] = 0; d64s[i] = 0; a64s[i] = 0; r64s[i] = 0; }
      }
      if constexpr (P) {
#pragma unroll
        for (int i = 0; i < 2 * DB; ++i) { u32p[i] = 0; d32p[i] = 0; a32p[i] = 0; r32p[i] = 0; }
      }
      for (int b = 0; b < 16; ++b) {   // 16x16 blocks in z-order
        const int q = b >> 2, s = b & 3;
        const int by = 2 * (q >> 1) + (s >> 1), bx = 2 * (q & 1) + (s & 1);
        const unsigned char* blk_ref = lane_ref + (by * 16) * WP + bx * 16;
        // sums of the 16x16 block: node, top half, left half, the quarter strips U D L R (all packed, <= 65 280)
        unsigned s16[2 * DB], t16[P ? 2 * DB : 1], l16[P ? 2 * DB : 1], u16[S ? 2 * DB : 1], d16[S ? 2 * DB : 1], a16[S ? 2 * DB : 1], r16[S ? 2 * DB : 1];
#pragma unroll
        for (int i = 0; i < 2 * DB; ++i) {
          s16[i] = 0;
          if constexpr (P) { t16[i] = 0; l16[i] = 0; }
          if constexpr (S) { u16[i] = 0; d16[i] = 0; a16[i] = 0; r16[i] = 0; }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {   // its four 8x8 tiles
          const int ty = 2 * by + (t >> 1), tx = 2 * bx + (t & 1);
          if ((cx * 64 + tx * 8 + 8 > F.width) || (cy * 64 + ty * 8 + 8 > F.height)) continue;   // uniform: tile outside the picture adds 0
          // the tile's original bytes -> SGPRs
          unsigned clo[8], chi[8];
#pragma unroll
          for (int r = 0; r < 8; ++r) {
            const uint2 c = *reinterpret_cast<const uint2*>(s_cur + (ty * 8 + r) * 64 + tx * 8);
            clo[r] = (unsigned)__builtin_amdgcn_readfirstlane((int)c.x);
            chi[r] = (unsigned)__builtin_amdgcn_readfirstlane((int)c.y);
          }
          const unsigned char* tr = blk_ref + ((t >> 1) * 8) * WP + (t & 1) * 8;
          u64 acc[NA][DB];   // S: q00 q01 / q10 q11 per dy; else the tile per dy
#pragma unroll
          for (int a = 0; a < NA; ++a)
#pragma unroll
            for (int d = 0; d < DB; ++d) acc[a][d] = 0;
#pragma unroll
          for (int j = 0; j < DB + 7; ++j) {   // reference row j of the block of DB dy: tile row r = j - d for vector row d
            const unsigned* p = reinterpret_cast<const unsigned*>(tr + j * WP);
            const unsigned d0 = p[0], d1 = p[1], d2 = p[2];
            const u64 w01 = ((u64)d1 << 32) | d0, w12 = ((u64)d2 << 32) | d1;
#pragma unroll
            for (int d = 0; d < DB; ++d) {
              const int r = j - d;
              if (r >= 0 && r < 8) {
                const int a0 = S ? (r >> 2) * 2 : 0, a1 = S ? a0 + 1 : 0;
                acc[a0][d] = qsad(w01, clo[r], acc[a0][d]);
                acc[a1][d] = qsad(w12, chi[r], acc[a1][d]);
              }
            }
          }
          unsigned t8[2 * DB];
          if constexpr (S) {
            unsigned top[2 * DB], bot[2 * DB], lef[2 * DB], rig[2 * DB];
#pragma unroll
            for (int d = 0; d < DB; ++d)
#pragma unroll
              for (int w = 0; w < 2; ++w) {   // packed halves <= 2 * 4 080: no carry between them
                const unsigned q00 = (unsigned)(acc[0][d] >> (32 * w)), q01 = (unsigned)(acc[1][d] >> (32 * w));
                const unsigned q10 = (unsigned)(acc[2][d] >> (32 * w)), q11 = (unsigned)(acc[3][d] >> (32 * w));
                top[2 * d + w] = q00 + q01; bot[2 * d + w] = q10 + q11; lef[2 * d + w] = q00 + q10; rig[2 * d + w] = q01 + q11;
                t8[2 * d + w] = top[2 * d + w] + bot[2 * d + w];
              }
            const int e = E_SMALL + 128 + (ty * 8 + tx) * 4;   // the 8x8 node's 2NxN (8x4) and Nx2N (4x8) PUs
            emit32(e + 0, top); emit32(e + 1, bot); emit32(e + 2, lef); emit32(e + 3, rig);
#pragma unroll
            for (int i = 0; i < 2 * DB; ++i) {   // the block's quarter strips: 2NxnU / 2NxnD / nLx2N / nRx2N
              if (t < 2) u16[i] += top[i]; else d16[i] += bot[i];
              if ((t & 1) == 0) a16[i] += lef[i]; else r16[i] += rig[i];
            }
          } else {
#pragma unroll
            for (int d = 0; d < DB; ++d) { t8[2 * d] = (unsigned)acc[0][d]; t8[2 * d + 1] = (unsigned)(acc[0][d] >> 32); }
          }
          if (N) emit32(21 + ty * 8 + tx, t8);
#pragma unroll
          for (int i = 0; i < 2 * DB; ++i) {   // packed halves <= 4 * 16 320: no carry between them
            s16[i] += t8[i];
            if constexpr (P) { if (t < 2) t16[i] += t8[i]; if ((t & 1) == 0) l16[i] += t8[i]; }
          }
        }
        const int i16 = by * 4 + bx;
        if (N) emit32(5 + i16, s16);
        unsigned b16[P ? 2 * DB : 1], g16[P ? 2 * DB : 1];   // bottom and right halves
        if constexpr (P) {
#pragma unroll
          for (int i = 0; i < 2 * DB; ++i) { b16[i] = s16[i] - t16[i]; g16[i] = s16[i] - l16[i]; }   // per half: part <= whole, no borrow
          const int e = E_PU + 60 + i16 * 4;
          emit32(e + 0, t16); emit32(e + 1, b16); emit32(e + 2, l16); emit32(e + 3, g16);
        }
        if constexpr (S) {
          unsigned rest[2 * DB];
          const int e = E_SMALL + i16 * 8;
          emit32(e + 0, u16);
#pragma unroll
          for (int i = 0; i < 2 * DB; ++i) rest[i] = s16[i] - u16[i];
          emit32(e + 1, rest);
#pragma unroll
          for (int i = 0; i < 2 * DB; ++i) rest[i] = s16[i] - d16[i];
          emit32(e + 2, rest);
          emit32(e + 3, d16);
          emit32(e + 4, a16);
#pragma unroll
          for (int i = 0; i < 2 * DB; ++i) rest[i] = s16[i] - a16[i];
          emit32(e + 5, rest);
#pragma unroll
          for (int i = 0; i < 2 * DB; ++i) rest[i] = s16[i] - r16[i];
          emit32(e + 6, rest);
          emit32(e + 7, r16);
        }
        if constexpr (N || P) {
          // ---- the block joins its 32x32 quadrant (s: bit 1 = lower, bit 0 = right) ----
          unsigned v16[NV];
          unpack(s16, v16);
#pragma unroll
          for (int v = 0; v < NV; ++v) {
            n32[v] += v16[v];
            if constexpr (P) { if (s < 2) t32[v] += v16[v]; if ((s & 1) == 0) l32[v] += v16[v]; }
          }
          if constexpr (P) {
#pragma unroll
            for (int i = 0; i < 2 * DB; ++i) {   // 32x8 / 8x32 strips <= 65 280: packed
              if (s < 2) u32p[i] += t16[i]; else d32p[i] += b16[i];
              if ((s & 1) == 0) a32p[i] += l16[i]; else r32p[i] += g16[i];
            }
          }
          if (s == 3) {   // the quadrant is complete: node 1 + q and its twelve PUs, then it joins the CTU (q: bit 1 = lower, bit 0 = right)
            if (N) emit64(1 + q, n32);
            if constexpr (P) {
              const int base = 5 + (1 + q) * 12;
              unsigned strip[NV];
              emit64_parts(base + 0, n32, t32, true);
              emit64_parts(base + 2, n32, l32, true);
              unpack(u32p, strip); emit64_parts(base + 4, n32, strip, true);
              unpack(d32p, strip); emit64_parts(base + 6, n32, strip, false);
              unpack(a32p, strip); emit64_parts(base + 8, n32, strip, true);
              unpack(r32p, strip); emit64_parts(base + 10, n32, strip, false);
            }
#pragma unroll
            for (int v = 0; v < NV; ++v) {
              n64[v] += n32[v];
              if constexpr (P) {
                if (q < 2) { t64[v] += n32[v]; u64s[v] += t32[v]; } else d64s[v] += n32[v] - t32[v];
                if ((q & 1) == 0) { l64[v] += n32[v]; a64s[v] += l32[v]; } else r64s[v] += n32[v] - l32[v];
                t32[v] = 0; l32[v] = 0;
              }
              n32[v] = 0;
            }
            if constexpr (P) {
#pragma unroll
              for (int i = 0; i < 2 * DB; ++i) { u32p[i] = 0; d32p[i] = 0; a32p[i] = 0; r32p[i] = 0; }
            }
          }
        }
      }
      if (N) emit64(0, n64);
      if constexpr (P) {
        emit64_parts(5 + 0, n64, t64, true);
        emit64_parts(5 + 2, n64, l64, true);
        emit64_parts(5 + 4, n64, u64s, true);
        emit64_parts(5 + 6, n64, d64s, false);
        emit64_parts(5 + 8, n64, a64s, true);
        emit64_parts(5 + 10, n64, r64s, false);
      }
    }
    __syncthreads();
    const long long oc = (long long)((f - 1) * band_rows + (cy - F.row_begin)) * F.ctus_x + cx;
    for (int e = tid; e < ENTRIES; e += 256) {
      if (e < E_PU ? !N : e < E_SMALL ? !P : !S) continue;
      int x, y, w, h, nx, ny, n;
      wide_entry_rect(e, x, y, w, h, nx, ny, n);
      uint4 o = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u);   // the CU node crosses the picture's edge
      if (cx * 64 + (nx + n) * 4 <= F.width && cy * 64 + (ny + n) * 4 <= F.height) {
        unsigned zero = 0;
        for (int j = y; j < y + h; ++j)
          for (int i = x; i < x + w; ++i) zero += s_zq[j * 16 + i];
        unsigned cost, ras;
        const int slot = e < 5 ? e : (e >= E_PU && e < E_PU + 60) ? 5 + (e - E_PU) : -1;
        if (slot >= 0) { const u64 k = s_key64[slot]; cost = (unsigned)(k >> 32); ras = (unsigned)k; }
        else { const unsigned k = s_key32[e]; cost = k >> 15; ras = k & 0x7FFFu; }
        const int mvx = (int)(ras % side) - range, mvy = (int)(ras / side) - range;
        const unsigned vc = s_bitc[fhevc_mv_component_bits(mvx) + fhevc_mv_component_bits(mvy)];
        o = make_uint4(zero, cost - vc, cost, ((unsigned)mvx & 0xFFFFu) | ((unsigned)mvy << 16));
      }
      FhevcMotionNode* dst = e < E_PU ? out_nodes + oc * FHEVC_NODES + e : e < E_SMALL ? out_pus + oc * FHEVC_PUS + (e - E_PU) : out_small + oc * FHEVC_PUS_SMALL + (e - E_SMALL);
      *reinterpret_cast<uint4*>(dst) = o;   // one 16-byte store per entry
    }
  }
}

template <typename T, int FAM, int DB>
void wide_launch(const FhevcFrames& fr, int range, const FhevcMvBitCost& cost, FhevcMotionNode* d_nodes, FhevcMotionNode* d_pus, FhevcMotionNode* d_small, int grid,
                 hipStream_t stream)
{
  hipLaunchKernelGGL((fhevc_motion_pu_wide_kernel<T, FAM, DB>), dim3(grid), dim3(256), 0, stream, fr, range, cost, d_nodes, d_pus, d_small);
}
// DB per family set (the largest that leaves the vector loop without scratch)
template <typename T>
void wide_dispatch(const FhevcFrames& fr, int range, const FhevcMvBitCost& cost, FhevcMotionNode* d_nodes, FhevcMotionNode* d_pus, FhevcMotionNode* d_small, int grid,
                   hipStream_t stream)
{
  const int fam = (d_nodes ? 1 : 0) | (d_pus ? 2 : 0) | (d_small ? 4 : 0);
  switch (fam) {
    case 1: return wide_launch<T, 1, 6>(fr, range, cost, d_nodes, d_pus, d_small, grid, stream);
    case 2: return wide_launch<T, 2, 2>(fr, range, cost, d_nodes, d_pus, d_small, grid, stream);
    case 3: return wide_launch<T, 3, 2>(fr, range, cost, d_nodes, d_pus, d_small, grid, stream);
    case 4: return wide_launch<T, 4, 4>(fr, range, cost, d_nodes, d_pus, d_small, grid, stream);
    case 5: return wide_launch<T, 5, 4>(fr, range, cost, d_nodes, d_pus, d_small, grid, stream);
    case 6: return wide_launch<T, 6, 2>(fr, range, cost, d_nodes, d_pus, d_small, grid, stream);
    default: return wide_launch<T, 7, 2>(fr, range, cost, d_nodes, d_pus, d_small, grid, stream);
  }
}

}  // namespace

// 8-bit content, search ranges 3 .. 64 (2 range + 1 >= the largest DB; the entry point sends ranges up to 8 to the MR = 8 kernels); at least one output
hipError_t fhevc_launch_motion_pu_wide(const FhevcFrames& fr, int range, const FhevcMvBitCost& cost, FhevcMotionNode* d_nodes, FhevcMotionNode* d_pus, FhevcMotionNode* d_small,
                                       int num_cus, hipStream_t stream)
{
  const long long total = (long long)(fr.row_end - fr.row_begin) * fr.ctus_x * (fr.num_frames - 1);
  if (total <= 0) return hipSuccess;
  if (fr.bit_depth != 8 || range < 3 || range > FHEVC_MOTION_WIDE_MAX_RANGE || (!d_nodes && !d_pus && !d_small)) return hipErrorInvalidValue;
  const int grid = (int)(total < 2LL * num_cus ? total : 2LL * num_cus);
  if (fr.sample_bytes == 2) wide_dispatch<int16_t>(fr, range, cost, d_nodes, d_pus, d_small, grid, stream);
  else wide_dispatch<uint8_t>(fr, range, cost, d_nodes, d_pus, d_small, grid, stream);
  return hipGetLastError();
}
