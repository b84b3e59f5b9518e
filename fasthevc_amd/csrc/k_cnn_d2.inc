// k_cnn_d2.inc -- included by k_cnn.hip (inside its anonymous namespace, behind k_cnn_layers.inc whose epilogue and weight images it shares): the members of
// the reference's Bayesian-optimisation network family with TWO convolutions per block (NetworkDepth 2: 23 / 46 / 92 filters,
// matlab/dataExtraction/OptimizeDeepNeuralNetworksUsingBayesianOptimizationExample.m:103-106, 233-259, 367-373) as ONE kernel.  Round 3 ran them layer by
// layer through HBM (k_cnn_layers.inc: 0.59 MB of activations written and read back per CTU, ~70 x the algorithmic bytes); here a CTU's activations never
// leave LDS: one 512-thread workgroup per CU takes a CTU from its samples to its depth map.
//
//   tile    66 x 66 centred samples (bytes, 0 outside the picture: oracle fho_load_ctu), row pitch 96, sample x at byte 16 + x
//   block 1 in two strips of 32 rows: conv1a (1 -> C1, K = the nine taps, one MFMA per 32 positions) writes 34 rows x 66 positions x 32 B into S; conv1b
//           (C1 -> C1) + 2x2 max-pool reads S (four accumulators (dy, dx) per pooled position, 4 x 4 window of B fragments) and writes 16 rows of A1
//   block 2 conv2a (C1 -> C2) A1 -> A2a [34][34][64 B]; conv2b (C2 -> C2) + pool A2a -> A2 [18][18][64 B]
//   block 3 conv3a (C2 -> C3) A2 -> A3a [18][18][96 B]; conv3b (C3 -> C3) A3a -> A3 [256 positions][96 B]
//   heads   thread = position, v_dot4_i32_i8 against its rows of the three FC weights (L2), DPP / readlane sums, depth_map_of_ctu
// Two LDS regions carry the six maps: R_big = S | A2a | A3a, R_a = A1 | A2 | A3 (each map is dead before its region's next tenant is written); every image
// is [row][position][Cpad bytes] with the halo part of it ("activation 0" = 0x80), the row pitch padded and the 16-byte slots XOR-ed exactly as the layer
// path's staged images (fhevc_layer_lds_image: conflict-free B-fragment reads for 64-channel inputs).  All arithmetic is the layer path's: v_mfma_i32_32x32x32_i8,
// A = the layer's weight fragments (fhevc_weights.hip: build_layers_image -- rows permuted so that a lane's 16 accumulators are 16 consecutive channels), B = 16 bytes
// per lane from the image, requant4_i8, activations a - 128.  Bit-exact with oracle/fhevc_oracle.c: fho_cnn_ctu_family (tests/test_gpu_family.py).
//
// Work split (8 waves): a wave keeps ONE M tile (32 output channels) per layer, its A fragments in registers for the layer (9 x Cin / 32 fragments, from L2);
// the N tiles (32 positions; pooled layers: 32 pooled positions) of that M tile are dealt over the waves that share it.  Blocks 1, 2: 8 / MT waves per M tile;
// block 3 (three M tiles): waves 0-5, two per M tile.
#ifndef FHEVC_D2_RING
#define FHEVC_D2_RING 6
#endif
constexpr int D2_RING = FHEVC_D2_RING;
constexpr int D2_TILE_PITCH = 96, D2_TILE_X0 = 16;   // sample x of tile row r (halo coordinates 0 .. 65) at byte r * 96 + 16 + x, x = -1 .. 64

struct D2Img { int off, px, pitch, mask; };   // LDS byte offset, bytes per position, row pitch, XOR mask of the 16-byte slots (0: plain)
__host__ __device__ constexpr int d2_pad(int kc, bool pool, int H, bool want_mask)
{
  // the table of fhevc_layer_lds_image (k_cnn.hip; tools/lds_swizzle_search.py) as a constant expression: (pad bytes, mask) that make the B-fragment reads of a
  // (kc, pool, H) layer free of bank conflicts.  Unlike the layer path, EVERY image uses its entry: here all of a CTU's traffic is LDS traffic, and the plain
  // 32- and 96-channel images (two and four ways conflicted) made 35 % of the LDS-active cycles conflict cycles (profiles/r04_pmc_d2_kernel.json)
  const int hi = H == 16 ? 0 : (H == 32 ? 1 : 2);
  constexpr int T[4][2][3][2] = {
    { { { 16, 0 }, { 0, 1 }, { 0, 1 } }, { { 192, 3 }, { 16, 1 }, { 0, 3 } } },
    { { { 32, 1 }, { 0, 3 }, { 0, 3 } }, { { 16, 1 }, { 32, 3 }, { 0, 7 } } },
    { { { 16, 0 }, { 0, 1 }, { 0, 1 } }, { { 64, 3 }, { 16, 1 }, { 0, 3 } } },
    { { { 64, 3 }, { 0, 7 }, { 0, 7 } }, { { 32, 3 }, { 64, 7 }, { 0, 15 } } } };
  return T[kc - 1][pool ? 1 : 0][hi][want_mask ? 1 : 0];
}
__host__ __device__ constexpr int d2_round256(int v) { return (v + 255) & ~255; }

template <int KC1, int KC2, int KC3>
struct LdsD2 {
  static constexpr int PX1 = 32 * KC1, PX2 = 32 * KC2, PX3 = 32 * KC3;
  // (consumer's kc, pool, H) decide an image's padding and mask
  static constexpr int S_PITCH = 66 * PX1 + d2_pad(KC1, true, 64, false), S_MASK = d2_pad(KC1, true, 64, true);
  static constexpr int A1_PITCH = 34 * PX1 + d2_pad(KC1, false, 32, false), A1_MASK = d2_pad(KC1, false, 32, true);
  static constexpr int A2A_PITCH = 34 * PX2 + d2_pad(KC2, true, 32, false), A2A_MASK = d2_pad(KC2, true, 32, true);
  static constexpr int A2_PITCH = 18 * PX2 + d2_pad(KC2, false, 16, false), A2_MASK = d2_pad(KC2, false, 16, true);
  static constexpr int A3A_PITCH = 18 * PX3 + d2_pad(KC3, false, 16, false), A3A_MASK = d2_pad(KC3, false, 16, true);
  static constexpr int S_BYTES = d2_round256(34 * S_PITCH), A1_BYTES = d2_round256(34 * A1_PITCH), A2A_BYTES = d2_round256(34 * A2A_PITCH);
  static constexpr int A2_BYTES = d2_round256(18 * A2_PITCH), A3A_BYTES = d2_round256(18 * A3A_PITCH), A3_BYTES = 256 * PX3;
  static constexpr int BIG_BYTES = S_BYTES > A2A_BYTES ? (S_BYTES > A3A_BYTES ? S_BYTES : A3A_BYTES) : (A2A_BYTES > A3A_BYTES ? A2A_BYTES : A3A_BYTES);
  static constexpr int RA_BYTES = A1_BYTES > A2_BYTES ? (A1_BYTES > A3_BYTES ? A1_BYTES : A3_BYTES) : (A2_BYTES > A3_BYTES ? A2_BYTES : A3_BYTES);
  static constexpr int BIG_OFF = 0, RA_OFF = BIG_BYTES, TILE_OFF = RA_OFF + RA_BYTES;
  static constexpr int TILE_BYTES = d2_round256(66 * D2_TILE_PITCH);
  static constexpr int LOGIT_OFF = TILE_OFF + TILE_BYTES;    // 64 ints as Lds::LOGIT_OFF
  static constexpr int PARK_OFF = LOGIT_OFF + 256;           // the next CTU's raw samples, parked by global_load_lds_dwordx4: [wave 4..7][2][64 lanes][16 B]
  static constexpr int LDS_BYTES = PARK_OFF + 4 * 2048;
  static_assert(LDS_BYTES <= 160 * 1024, "one workgroup per CU");
};

// (Measured and dropped: the requant form chosen per layer from its weights -- shift <= 7: 28 instead of 36 instructions per 16 values, shift 8 with every
// accumulator inside 24 bits: 20, as the tuned kernel's; every layer of the shipped blob qualifies for a short form.  Bit-exact, and 5 % SLOWER (4.27-4.33 against
// 4.04-4.14 ms, profiles/r04_d2_ab_experiments.log), as the same change was in the layer path: the uniform three-way branch at every store site costs more than
// the shorter forms save.)
__device__ __forceinline__ unsigned d2_swz(unsigned a, int mask) { return mask ? a ^ (((a >> 8) & (unsigned)mask) << 4) : a; }

// the halo of an [N + 2][N + 2] image: "activation 0" in every 16-byte slot of the border cells
template <int N, int PX, int PITCH, int MASK>
__device__ __forceinline__ void d2_fill_halo(unsigned char* img, int tid)
{
  constexpr int CELLS = 4 * (N + 1), SLOTS = PX / 16;
  const uint4 z = make_uint4(0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u);
  { unsigned t_ = (unsigned)tid; asm volatile("" : "+v"(t_)); tid = (int)t_; }   // (not hoisted out of the CTU loop: see d2_conv)
  for (int e = tid; e < CELLS * SLOTS; e += 512) {
    const int c = e / SLOTS, s = e - c * SLOTS;
    int y, x;
    if (c < N + 2) { y = 0; x = c; }
    else if (c < 2 * (N + 2)) { y = N + 1; x = c - (N + 2); }
    else { const int k = c - 2 * (N + 2); y = 1 + (k >> 1); x = (k & 1) ? N + 1 : 0; }
    *reinterpret_cast<uint4*>(img + d2_swz((unsigned)(y * PITCH + x * PX + 16 * s), MASK)) = z;
  }
}

// A layer's weights for this wave: the A fragments of its M tile (9 x KC) and the bias tile, from L2 into registers.  Called one phase EARLY -- from the previous
// layer's hook, behind its last MFMA chain and in front of its last epilogue and the barrier -- so that the loads travel while the waves finish and meet
// instead of at the head of the layer (7 phases x ~600 cycles per CTU with every wave of the CU waiting).
// which M tile a wave starts a layer with: MT = 1, 2, 4: wave mod MT for the whole layer; MT = 3 (block 3: 24 (M tile, N tile) items, three per wave,
// M-tile-major): the M tile of the wave's first item -- waves 2 and 5 cross into the next M tile at their third / second item and reload there
template <int MT> __device__ __forceinline__ int d2_first_mt(int wave) { return MT == 3 ? (3 * wave) >> 3 : wave % MT; }

template <int KC, int MT>
__device__ __forceinline__ void d2_weights(const uint4* __restrict__ frag, const int32_t* __restrict__ bias, bf16x8 (&wA)[KC * 9], i32x16& binit, int mt_override = -1)
{
  constexpr int NF = KC * 9;
  // thread coordinates re-derived from an opaque copy of threadIdx: everything computed from them is loop-invariant over the CTUs, and hipcc would otherwise
  // hoist it (and the loads: 344 registers spilled in the first build) out of the CTU loop for all phases at once
  unsigned t_ = threadIdx.x;
  asm volatile("" : "+v"(t_));
  const int lane = (int)(t_ & 63u), wave = __builtin_amdgcn_readfirstlane((int)(t_ >> 6));
  const int mt = mt_override >= 0 ? mt_override : d2_first_mt<MT>(wave), h = lane >> 5;
  const unsigned char* fb = reinterpret_cast<const unsigned char*>(frag) + ((unsigned)mt * NF * 64 + (unsigned)lane) * 16u;
#pragma unroll
  for (int s = 0; s < NF; ++s) wA[s] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(fb + s * 64 * 16));
  const unsigned char* bb = reinterpret_cast<const unsigned char*>(bias) + (unsigned)(mt * 32 + 16 * h) * 4u;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int4 v = *reinterpret_cast<const int4*>(bb + 16 * g);
    binit[4 * g + 0] = v.x; binit[4 * g + 1] = v.y; binit[4 * g + 2] = v.z; binit[4 * g + 3] = v.w;
  }
}

// One convolution from an LDS image to an LDS image.  KC = Cin_pad / 32; MT = Cout_pad / 32; POOL: 2x2 max-pool behind it; H: input size; rows [y0, y0 + ROWS) of
// the (pre-pool) output are computed, the input image pointer addresses row 0 of the WHOLE input map (halo coordinates) minus in_row0 rows (the strip form
// of block 1: S holds rows in_row0 .. of the map).  OUT_HALO: the output image has a halo (position (y, x) at row y + 1, cell x + 1).
// wA / binit: d2_weights of this layer.  hook(): called once per wave behind the LAST tile's MFMA chain, in front of its epilogue (the next layer's d2_weights).
// The ring of B fragments runs ACROSS the wave's tiles: the first D2_RING reads of tile i + 1 are issued in front of tile i's epilogue (pool, requant, store:
// ~100 vector instructions), so only the first tile of a phase exposes the LDS latency.
// Block 3 (three M tiles x eight N tiles of the 16 x 16 map = 24 items): ALL eight waves, three single-tile items each in M-tile-major order (round 4's first
// build ran two-tile steps on six waves: 72 / 108 MFMAs on the critical path of conv3a / conv3b instead of 54 / 81).  One accumulator per item -- a chain of
// dependent 32x32 MFMAs issues back to back (MI355X_MICROARCH.md) -- the B ring runs across the items; a wave whose items straddle two M tiles reloads its
// weights in between.  frag / bias: this layer's images (for that reload); wA / binit arrive loaded for the wave's FIRST item (d2_weights).
template <int KC, bool POOLX, int H, int IN_PITCH_B, int IN_MASK, int OUT_PX, int OUT_PITCH_B, int OUT_MASK, bool OUT_HALO, int RQ, typename Hook>
__device__ __forceinline__ void d2_conv_m3(const unsigned char* in, unsigned char* out, const uint4* __restrict__ frag, const int32_t* __restrict__ bias, bf16x8 (&wA)[KC * 9],
                                           i32x16& binit, int shift, Hook&& hook)
{
  static_assert(!POOLX && H == 16, "block 3: 16 x 16 maps, no pool");
  constexpr int PX = KC * 32, NS = KC * 9, TILES = 8;
  unsigned t_ = threadIdx.x;
  asm volatile("" : "+v"(t_));   // (see d2_weights)
  const int lane = (int)(t_ & 63u), wave = __builtin_amdgcn_readfirstlane((int)(t_ >> 6));
  const int n = lane & 31, h = lane >> 5;
  int mt = d2_first_mt<3>(wave);
  int oy = 0, ox = 0, q = 0;
  auto base_of = [&](int item) { const int p = (item % TILES) * 32 + n; oy = p >> 4; ox = p & 15; q = oy * IN_PITCH_B + ox * PX + 16 * h; };
  auto frag_b = [&](int i) {
    const int tap = i % 9;
    const int o = q + (tap / 3) * IN_PITCH_B + (tap % 3) * PX + (i / 9) * 32;
    return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(in + d2_swz((unsigned)o, IN_MASK)));
  };
  bf16x8 ring[D2_RING];
  // chain of item k into `acc`; the epilogue of item k - 1 (`prev`) runs behind it, as in blocks 1 and 2.  (Dealing that epilogue over the chain's
  // first four MFMA steps with sched_group_barrier measured no gain: 4.00-4.13 ms against 4.02, profiles/r04_d2_ab_experiments.log.)
  auto chain = [&](i32x16& acc, const i32x16* prev, int po) {
    acc = binit;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const bf16x8 b = ring[i % D2_RING];
      if (i + D2_RING < NS) ring[i % D2_RING] = frag_b(i + D2_RING);
      acc = mfma_i8(wA[i], b, acc);
    }
    if (prev != nullptr) layer_store16<RQ>(*prev, out + d2_swz((unsigned)po, OUT_MASK), shift);
  };
  auto out_off = [&](int m) { return OUT_HALO ? (oy + 1) * OUT_PITCH_B + (ox + 1) * OUT_PX + m * 32 + 16 * h : (oy * 16 + ox) * OUT_PX + m * 32 + 16 * h; };
  base_of(3 * wave);
#pragma unroll
  for (int i = 0; i < D2_RING && i < NS; ++i) ring[i] = frag_b(i);
  i32x16 a0, a1, a2;
  // item 0
  chain(a0, nullptr, 0);
  const int o0 = out_off(mt);
  {
    const int nmt = (3 * wave + 1) >> 3;
    base_of(3 * wave + 1);
#pragma unroll
    for (int i = 0; i < D2_RING && i < NS; ++i) ring[i] = frag_b(i);
    if (nmt != mt) { mt = nmt; asm volatile("" : "+v"(a0)); d2_weights<KC, 3>(frag, bias, wA, binit, mt); }   // (behind the chain that used the old ones)
  }
  // item 1 (then the epilogue of item 0)
  chain(a1, &a0, o0);
  const int o1 = out_off(mt);
  {
    const int nmt = (3 * wave + 2) >> 3;
    base_of(3 * wave + 2);
#pragma unroll
    for (int i = 0; i < D2_RING && i < NS; ++i) ring[i] = frag_b(i);
    if (nmt != mt) { mt = nmt; asm volatile("" : "+v"(a1)); d2_weights<KC, 3>(frag, bias, wA, binit, mt); }
  }
  // item 2 (then the epilogue of item 1)
  chain(a2, &a1, o1);
  const int o2 = out_off(mt);
  asm volatile("" : "+v"(a2));   // the hook's loads stay BEHIND the chain
  hook();
  layer_store16<RQ>(a2, out + d2_swz((unsigned)o2, OUT_MASK), shift);
}

template <int KC, int MT, bool POOL, int H, int ROWS, int IN_PITCH_B, int IN_MASK, int OUT_PX, int OUT_PITCH_B, int OUT_MASK, bool OUT_HALO, int RQ, typename Hook>
__device__ __forceinline__ void d2_conv(const unsigned char* in, int in_row0, unsigned char* out, int y0, const bf16x8 (&wA)[KC * 9], const i32x16& binit, int shift, Hook&& hook,
                                        const int32_t* __restrict__ bias = nullptr)
{
  // LATE_BIAS (the pooled 64-channel layer, conv2b: 72 weight + 64 accumulator + 24 ring registers): the accumulators start from zero and the bias tile joins
  // BEHIND the max-pool (max commutes with a per-channel constant; exact in 32 bits), re-requested from L2 there -- 16 registers fewer across the chains, which
  // is what hipcc was parking in scratch around them (198 MB of scratch writes reaching HBM per launch)
  constexpr bool LATE_BIAS = POOL && KC == 2;
  constexpr int PX = KC * 32;
  constexpr int Ho = POOL ? H / 2 : H, RO = POOL ? ROWS / 2 : ROWS;   // output geometry
  constexpr int TILES = RO * Ho / 32;                                   // N tiles of this call
  constexpr int WPM = MT == 3 ? 2 : 8 / MT;                             // waves per M tile
  constexpr int TS = POOL ? 1 : 2;                                      // N tiles per step (two accumulators) / pooled: one tile, four accumulators
  static_assert(TILES % (WPM * TS) == 0, "the N tiles divide over the waves of an M tile");
  unsigned t_ = threadIdx.x;
  asm volatile("" : "+v"(t_));   // (see d2_weights)
  const int lane = (int)(t_ & 63u), wave = __builtin_amdgcn_readfirstlane((int)(t_ >> 6));
  if (wave >= MT * WPM) { hook(); return; }
  const int n = lane & 31, h = lane >> 5;
  const int mt = wave % MT, sub = wave / MT;
  constexpr int LG = Ho == 64 ? 6 : (Ho == 32 ? 5 : 4);
  const int t0 = (POOL ? y0 / 2 : y0) * Ho / 32;   // first N tile of this call in the whole output map
  bf16x8 ring[D2_RING];
  if constexpr (POOL) {
    constexpr int NS = KC * 16;
    // the 4 x 4 input positions around a pooled position: position (iy, ix) is tap (iy - dy, ix - dx) of the pre-pool output (dy, dx)
    auto base_of = [&](int t, int& oy, int& ox) { const int p = (t0 + t) * 32 + n; oy = p >> LG; ox = p & (Ho - 1); return (oy * 2 - in_row0) * IN_PITCH_B + (ox * 2) * PX + 16 * h; };
    auto frag_b = [&](int q, int i) {
      const int o = q + ((i & 15) >> 2) * IN_PITCH_B + (i & 3) * PX + (i >> 4) * 32;
      return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(in + d2_swz((unsigned)o, IN_MASK)));
    };
    int oy, ox;
    int q = base_of(sub * TS, oy, ox);
#pragma unroll
    for (int i = 0; i < D2_RING && i < NS; ++i) ring[i] = frag_b(q, i);
    i32x16 acc[4];
    auto chain = [&]() {
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        if (LATE_BIAS) {
#pragma unroll
          for (int k = 0; k < 16; ++k) acc[a][k] = 0;
        } else acc[a] = binit;
      }
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        const bf16x8 b = ring[i % D2_RING];
        if (i + D2_RING < NS) ring[i % D2_RING] = frag_b(q, i + D2_RING);
        const int kc = i >> 4, iy = (i & 15) >> 2, ix = i & 3;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const int ky = iy - (a >> 1), kx = ix - (a & 1);
          if (ky >= 0 && ky < 3 && kx >= 0 && kx < 3) acc[a] = mfma_i8(wA[kc * 9 + ky * 3 + kx], b, acc[a]);
        }
      }
    };
    auto epilogue = [&](int o) {
      int4 bv[4];
      if (LATE_BIAS) {
        unsigned bo = (unsigned)(mt * 32 + 16 * h) * 4u;
        asm volatile("" : "+v"(bo));   // (a fresh address per tile: the loads are neither hoisted nor merged with d2_weights')
        const unsigned char* bb = reinterpret_cast<const unsigned char*>(bias) + bo;
#pragma unroll
        for (int g = 0; g < 4; ++g) bv[g] = *reinterpret_cast<const int4*>(bb + 16 * g);
      }
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[0][k] = max(max(acc[0][k], acc[1][k]), max(acc[2][k], acc[3][k]));
      if (LATE_BIAS) {
#pragma unroll
        for (int g = 0; g < 4; ++g) { acc[0][4 * g] += bv[g].x; acc[0][4 * g + 1] += bv[g].y; acc[0][4 * g + 2] += bv[g].z; acc[0][4 * g + 3] += bv[g].w; }
      }
      layer_store16<RQ>(acc[0], out + d2_swz((unsigned)o, OUT_MASK), shift);
    };
    auto out_off = [&]() { return (oy + (OUT_HALO ? 1 : 0)) * OUT_PITCH_B + (ox + (OUT_HALO ? 1 : 0)) * OUT_PX + mt * 32 + 16 * h; };
    // every tile but the wave's last: chain, the next tile's first fragments requested, epilogue
#pragma unroll 1
    for (int t = sub * TS; t + WPM * TS < TILES; t += WPM * TS) {
      chain();
      const int o = out_off();
      q = base_of(t + WPM * TS, oy, ox);
#pragma unroll
      for (int i = 0; i < D2_RING && i < NS; ++i) ring[i] = frag_b(q, i);
      epilogue(o);
    }
    // the last tile OUTSIDE the loop, so that what the hook loads (the next layer's weights) is not a loop-carried value that shares the loop with this layer's
    chain();
    asm volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]));   // the hook's loads stay BEHIND the chain: this layer's weights are dead when the next layer's arrive
    hook();
    epilogue(out_off());
  } else {
    constexpr int NS = KC * 18;   // (K chunk, tap, N tile of the pair)
    int oy[2], ox[2], q[2];
    auto base_of = [&](int t) {
#pragma unroll
      for (int u = 0; u < 2; ++u) { const int p = (t0 + t + u) * 32 + n; oy[u] = p >> LG; ox[u] = p & (Ho - 1); q[u] = (oy[u] - in_row0) * IN_PITCH_B + ox[u] * PX + 16 * h; }
    };
    auto frag_b = [&](int i) {
      const int tap = (i >> 1) % 9;
      const int o = q[i & 1] + (tap / 3) * IN_PITCH_B + (tap % 3) * PX + (i / 18) * 32;
      return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(in + d2_swz((unsigned)o, IN_MASK)));
    };
    base_of(sub * TS);
#pragma unroll
    for (int i = 0; i < D2_RING && i < NS; ++i) ring[i] = frag_b(i);
    i32x16 acc[2];
    auto chain = [&]() {
      acc[0] = binit; acc[1] = binit;
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        const bf16x8 b = ring[i % D2_RING];
        if (i + D2_RING < NS) ring[i % D2_RING] = frag_b(i + D2_RING);
        acc[i & 1] = mfma_i8(wA[(i / 18) * 9 + (i >> 1) % 9], b, acc[i & 1]);
      }
    };
    int o[2];
    auto out_off = [&]() {
#pragma unroll
      for (int u = 0; u < 2; ++u) o[u] = OUT_HALO ? (oy[u] + 1) * OUT_PITCH_B + (ox[u] + 1) * OUT_PX + mt * 32 + 16 * h : (oy[u] * Ho + ox[u]) * OUT_PX + mt * 32 + 16 * h;
    };
    auto epilogue = [&]() {
#pragma unroll
      for (int u = 0; u < 2; ++u) layer_store16<RQ>(acc[u], out + d2_swz((unsigned)o[u], OUT_MASK), shift);
    };
#pragma unroll 1
    for (int t = sub * TS; t + WPM * TS < TILES; t += WPM * TS) {
      chain();
      out_off();
      base_of(t + WPM * TS);
#pragma unroll
      for (int i = 0; i < D2_RING && i < NS; ++i) ring[i] = frag_b(i);
      epilogue();
    }
    chain();
    out_off();
    asm volatile("" : "+v"(acc[0]), "+v"(acc[1]));   // (as above)
    hook();
    epilogue();
  }
}

// SHORT: every layer runs its short requant form (conv1a: form 1, the other five: form 2) -- the host found the blob qualified (FhevcLayersWeights::d2_short);
// a compile-time choice for the whole kernel: the same choice as a uniform branch at every store site measured 5 % slower than no choice at all
template <int KC1, int KC2, int KC3, bool SHORT>
__global__ __launch_bounds__(512, 2) void fhevc_cnn_d2_kernel(FhevcFrames F, FhevcLayersWeights W, uint8_t* __restrict__ d_depth, int32_t* __restrict__ d_logits,
                                                              uint32_t* __restrict__ d_flags, uint8_t* __restrict__ d_depth_max, int margin_split, int margin_stop)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  using P = LdsD2<KC1, KC2, KC3>;
  constexpr int RQA = SHORT ? 1 : 0, RQB = SHORT ? 2 : 0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hb64a = W.bhead[0], hb64b = W.bhead[1] + W.bhead[6 + 0 * 52 + F.qp];
  const int hb32a = W.bhead[2], hb32b = W.bhead[3] + W.bhead[6 + 1 * 52 + F.qp];
  const int hb16a = W.bhead[4], hb16b = W.bhead[5] + W.bhead[6 + 2 * 52 + F.qp];
  // (Measured and dropped: one static s_setprio level for waves 4-7.  Stamped, waves 0-3 leave every convolution ~30 % ahead of their SIMD partners 4-7 -- the
  // arbiter serves the older wave first -- and wait at the barrier; raising the younger half changed nothing, 4.63 against 4.64 ms.)
  int* logitL = reinterpret_cast<int*>(lds + P::LOGIT_OFF);
  unsigned char* const big = lds + P::BIG_OFF;
  unsigned char* const ra = lds + P::RA_OFF;
  unsigned char* const tile = lds + P::TILE_OFF;

  const int band_rows = F.row_end - F.row_begin;
  const int per_frame = band_rows * F.ctus_x;
  const int total = per_frame * F.num_frames;
  const int shift_in = F.bit_depth - 8;
  const int grid = (int)gridDim.x;
  const int vblock = (grid & 7) ? (int)blockIdx.x : (int)((blockIdx.x & 7) * (grid >> 3) + (blockIdx.x >> 3));   // XCD-aware walk (speed only), as the other kernels
  CtuPos pos, step;
  {
    const int vb = min(vblock, total - 1);
    pos.f = vb / per_frame; pos.ry = (vb - pos.f * per_frame) / F.ctus_x; pos.cx = (vb - pos.f * per_frame) - pos.ry * F.ctus_x;
    step.f = grid / per_frame; step.ry = (grid - step.f * per_frame) / F.ctus_x; step.cx = (grid - step.f * per_frame) - step.ry * F.ctus_x;
  }
  // the tile's halo (row 0, row 65, columns -1 and 64) and its unused margins are written once: staging only rewrites the 64 x 64 interior
  for (int i = tid; i < P::TILE_BYTES / 16; i += 512) *reinterpret_cast<uint4*>(tile + 16 * i) = make_uint4(0, 0, 0, 0);
  __syncthreads();

  // staging of a CTU: threads 256 .. 511 (waves 4-7) hold 16 samples of one picture row each (prefetch_ctu), convert them to centred bytes (rounded to 8 bits
  // above 8 bit, 0 outside the picture: fho_load_ctu) and store one aligned 16-byte slot of the tile
  auto stage = [&](const Prefetched& pre, const CtuPos& c, int ld_row, int ld_seg) {
    unsigned char* dst = tile + (ld_row + 1) * D2_TILE_PITCH + D2_TILE_X0 + 16 * ld_seg;
    unsigned v[16];
    if (pre.fast) {
      if (F.sample_bytes == 2) {
        const unsigned wds[8] = { pre.a.x, pre.a.y, pre.a.z, pre.a.w, pre.b.x, pre.b.y, pre.b.z, pre.b.w };
        const unsigned rnd2 = shift_in > 0 ? (0x00010001u << (shift_in - 1)) : 0u;
#pragma unroll
        for (int j = 0; j < 8; ++j) { const unsigned t = sample8_pair(wds[j], shift_in, rnd2); v[2 * j] = t & 0xFF; v[2 * j + 1] = (t >> 16) & 0xFF; }
      } else {
        const unsigned wds[4] = { pre.a.x, pre.a.y, pre.a.z, pre.a.w };
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = (wds[j >> 2] >> (8 * (j & 3))) & 0xFF;
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] ^= 0x80;   // sample - 128 as a byte
    } else {  // picture edge or unaligned plane: guarded scalar loads
      const int py = (F.row_begin + c.ry) * 64 + ld_row, px0 = c.cx * 64 + ld_seg * 16;
      const long long base = (long long)c.f * F.frame_stride + (long long)py * F.stride + px0;
      const bool row_ok = py < F.height;
#pragma unroll 4
      for (int j = 0; j < 16; ++j) {
        unsigned s = 0;
        if (row_ok && px0 + j < F.width) {
          const int smp = F.sample_bytes == 2 ? load_sample8(reinterpret_cast<const int16_t*>(F.luma) + base + j, shift_in) : (int)reinterpret_cast<const uint8_t*>(F.luma)[base + j];
          s = (unsigned)(smp ^ 0x80) & 0xFF;
        }
        v[j] = s;
      }
    }
    uint4 o;
    o.x = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
    o.y = v[4] | (v[5] << 8) | (v[6] << 16) | (v[7] << 24);
    o.z = v[8] | (v[9] << 8) | (v[10] << 16) | (v[11] << 24);
    o.w = v[12] | (v[13] << 8) | (v[14] << 16) | (v[15] << 24);
    *reinterpret_cast<uint4*>(dst) = o;
  };
  // a CTU is staged by threads 256 .. 511 (waves 4-7): its samples are requested at the head of block 3 of the CTU before it and stored during that CTU's heads
  // (waves 4-7 idle there).  (Measured and dropped: the whole fetch + store by the two waves that have no M tile in block 3, inside one phase so that no
  // prefetch register lives across a convolution -- the exposed HBM latency of 128 threads cost more, 4.50 -> 4.75 ms, than the registers' spills.)
  const int st_row = (tid & 255) >> 2, st_seg = tid & 3;
  // the aligned fast path of prefetch_ctu: the thread's 16 samples lie inside the picture and their address is 16-byte aligned (recomputed where needed, not kept)
  auto park_fast = [&](const CtuPos& c, int ld_row, int ld_seg) {
    const int py = (F.row_begin + c.ry) * 64 + ld_row, px0 = c.cx * 64 + ld_seg * 16;
    if (py >= F.height || px0 + 16 > F.width) return 0;
    const long long base = (long long)c.f * F.frame_stride + (long long)py * F.stride + px0;
    const uintptr_t a = reinterpret_cast<uintptr_t>(F.luma) + (uintptr_t)base * (uintptr_t)F.sample_bytes;
    return (a & 15) ? 0 : 1;
  };
  if (tid >= 256 && vblock < total) {   // the workgroup's first CTU: through registers, nothing else is in flight yet
    const Prefetched pre = prefetch_ctu<false>(F, true, pos, st_row, st_seg);
    stage(pre, pos, st_row, st_seg);
  }
  __syncthreads();

  const FhevcLayer& L1a = W.l[0]; const FhevcLayer& L1b = W.l[1]; const FhevcLayer& L2a = W.l[2];
  const FhevcLayer& L2b = W.l[3]; const FhevcLayer& L3a = W.l[4]; const FhevcLayer& L3b = W.l[5];
  // the weights of a layer that follows an un-pooled one are requested one phase early (d2_weights from the hook of d2_conv)

#if defined(FHEVC_D2_STAMPS)   // (diagnostic variant, WRONG output: cycle sums per phase of wave FHEVC_D2_STAMPS - 1 overwrite the first bytes of the workgroup's first depth map)
  unsigned long long tsum[12] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 }, tprev = stamp();
#define D2_STAMP(k) { const unsigned long long tn = stamp(); tsum[k] += tn - tprev; tprev = tn; }
#else
#define D2_STAMP(k)
#endif
  for (int work = vblock; work < total; work += grid) {
    const CtuPos next = advance(pos, step, band_rows, F.ctus_x);
    bf16x8 w1b[KC1 * 9], w2a[KC1 * 9], w2b[KC2 * 9], w3a[KC2 * 9], w3b[KC3 * 9];
    i32x16 b1b, b2a, b2b, b3a, b3b;
    // ================= block 1, two strips of 32 rows: conv1a -> S, then conv1b + pool -> A1 =================
    d2_fill_halo<32, P::PX1, P::A1_PITCH, P::A1_MASK>(ra, tid);   // (R_a held the previous CTU's last map until its heads were done: one barrier back)
    d2_weights<KC1, KC1>(L1b.frag, L1b.bias, w1b, b1b);           // the second convolution's weights travel under the first convolution's first strip
#pragma unroll 1
    for (int s = 0; s < 2; ++s) {
      {
        // rows y0 .. y0 + 33 (halo coordinates) of the first convolution's output into S.  The cells outside the map -- row 0 (first strip) or 65 (second strip)
        // and the two halo columns of every row -- are "activation 0", written by the first threads of the workgroup; the 33 rows inside the map are one MFMA
        // per 32 positions (K = the nine taps), requant, one 16-byte store per lane.  The tile loop is free of branches: the wave index is made scalar
        // (readfirstlane), and every lane reads its window -- lanes 32-63 the same bytes as lanes 0-31: their K slots 16 .. 31, like the slots 9 .. 15, meet zero
        // weights (build_layers_image), so what the B operand holds there is irrelevant.  (First build: exec-masked reads and three per-tile branches, ~120
        // instructions per tile, 27 % of the kernel.)
        const int y0 = 32 * s;
        unsigned t_ = threadIdx.x;
        asm volatile("" : "+v"(t_));
        const int lane = (int)(t_ & 63u), wave = __builtin_amdgcn_readfirstlane((int)(t_ >> 6));   // (shadow the kernel's: see d2_conv)
        const int n = lane & 31, h = lane >> 5;
        const uint4 zero = make_uint4(0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u);
        {
          constexpr int SL = KC1 * 2;                       // 16-byte slots per position
          const int e = (int)t_;
          if (e < 34 * 2 * SL) {                            // halo columns: (row, left / right, slot)
            const int rw = e / (2 * SL), rem = e - rw * (2 * SL), side = rem / SL, sl = rem - side * SL;
            *reinterpret_cast<uint4*>(big + d2_swz((unsigned)(rw * P::S_PITCH + (side ? 65 * P::PX1 : 0) + 16 * sl), P::S_MASK)) = zero;
          } else if (e < 34 * 2 * SL + 64 * SL) {           // the row outside the map: local row 0 of the first strip, 33 of the second
            const int k = e - 34 * 2 * SL, x = k / SL, sl = k - x * SL;
            *reinterpret_cast<uint4*>(big + d2_swz((unsigned)((s == 0 ? 0 : 33) * P::S_PITCH + (x + 1) * P::PX1 + 16 * sl), P::S_MASK)) = zero;
          }
        }
        bf16x8 f0[KC1];
        i32x16 b0[KC1];
        unsigned foff = (unsigned)lane * 16u, boff = (unsigned)(16 * h) * 4u;
        asm volatile("" : "+v"(foff), "+v"(boff));   // (as d2_conv: the loads stay inside the loop)
#pragma unroll
        for (int m0 = 0; m0 < KC1; ++m0) {
          f0[m0] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned char*>(L1a.frag) + foff + m0 * 64 * 16));
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int4 v = *reinterpret_cast<const int4*>(reinterpret_cast<const unsigned char*>(L1a.bias) + boff + (m0 * 32 + 4 * g) * 4);
            b0[m0][4 * g + 0] = v.x; b0[m0][4 * g + 1] = v.y; b0[m0][4 * g + 2] = v.z; b0[m0][4 * g + 3] = v.w;
          }
        }
        // tile tt = (row lr, half) of the strip's 33 rows inside the map: local rows 1 .. 33 of the first strip, 0 .. 32 of the second
        const int lr0 = s == 0 ? 1 : 0;
#pragma unroll 1
        for (int tt = wave; tt < 33 * 2; tt += 8) {
          const int lr = lr0 + (tt >> 1), xs = (tt & 1) * 32;         // local row of S; first image column of the tile
          const int r = y0 + lr;                                       // the same row in halo coordinates (image row r - 1)
          // the window: rows r - 1 .. r + 1 (halo coordinates), columns x - 1 .. x + 1 = three bytes from byte a = X0 - 1 + x of three tile rows.  Read as the two
          // ALIGNED dwords around a per row + v_alignbyte (sub-dword LDS reads, ds_read_u8 / _u16, cost this phase ~750 cycles per tile: 22 k of its 23 k cycles
          // per CTU went away with them in a sensitivity build), then two v_perm put the nine taps into K slots 0 .. 8; what lands in slots 9 .. 15 meets zero weights
          const unsigned a = (unsigned)((r - 1) * D2_TILE_PITCH + D2_TILE_X0 - 1 + xs + n);
          const unsigned* qd = reinterpret_cast<const unsigned*>(tile + (a & ~3u));
          unsigned rw[3];
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const unsigned lo = qd[k * (D2_TILE_PITCH / 4)], hi = qd[k * (D2_TILE_PITCH / 4) + 1];
            rw[k] = __builtin_amdgcn_alignbyte(hi, lo, a & 3u);
          }
          uint4 bq;
          bq.x = __builtin_amdgcn_perm(rw[1], rw[0], 0x04020100u);   // taps (0,0) (0,1) (0,2) (1,0)
          bq.y = __builtin_amdgcn_perm(rw[2], rw[1], 0x05040201u);   // taps (1,1) (1,2) (2,0) (2,1)
          bq.z = rw[2] >> 16;                                        // tap (2,2) (+ a byte on a zero weight)
          bq.w = 0;
          const unsigned row = (unsigned)lr * (unsigned)P::S_PITCH;
#pragma unroll
          for (int m0 = 0; m0 < KC1; ++m0) {
            const i32x16 a0 = mfma_i8(f0[m0], __builtin_bit_cast(bf16x8, bq), b0[m0]);
            layer_store16<RQA>(a0, big + d2_swz(row + (unsigned)(xs + n + 1) * P::PX1 + m0 * 32 + 16 * h, P::S_MASK), L1a.shift);
          }
        }
      }
      D2_STAMP(0)   // conv1a
      __syncthreads();
      D2_STAMP(1)   // barrier wait
      d2_conv<KC1, KC1, true, 64, 32, P::S_PITCH, P::S_MASK, P::PX1, P::A1_PITCH, P::A1_MASK, true, RQB>(big, 32 * s, ra, 32 * s, w1b, b1b, L1b.shift, []() {});
      D2_STAMP(2)   // conv1b
      __syncthreads();
      D2_STAMP(1)
    }
    // ================= block 2 =================
    // (the pooled layers carry no hook: in block 2 four accumulators + 18 fragments + the next layer's 18 in flight exceed the 256 registers -- 388 spilled, in
    // the chains; in block 1 the hook fits only with the strip loop unrolled, and that build measured 3 % slower)
    d2_weights<KC1, KC2>(L2a.frag, L2a.bias, w2a, b2a);
    d2_fill_halo<32, P::PX2, P::A2A_PITCH, P::A2A_MASK>(big, tid);
    d2_conv<KC1, KC2, false, 32, 32, P::A1_PITCH, P::A1_MASK, P::PX2, P::A2A_PITCH, P::A2A_MASK, true, RQB>(ra, 0, big, 0, w2a, b2a, L2a.shift,
                                                                                                        [&]() { d2_weights<KC2, KC2>(L2b.frag, L2b.bias, w2b, b2b); });
    D2_STAMP(3)   // conv2a
    __syncthreads();
    D2_STAMP(1)
    d2_fill_halo<16, P::PX2, P::A2_PITCH, P::A2_MASK>(ra, tid);
    d2_conv<KC2, KC2, true, 32, 32, P::A2A_PITCH, P::A2A_MASK, P::PX2, P::A2_PITCH, P::A2_MASK, true, RQB>(big, 0, ra, 0, w2b, b2b, L2b.shift, []() {}, L2b.bias);
    D2_STAMP(4)   // conv2b
    __syncthreads();
    D2_STAMP(1)
    // ================= block 3 =================
    d2_weights<KC2, KC3>(L3a.frag, L3a.bias, w3a, b3a);
    // the next CTU's samples travel under block 3 -- global memory -> LDS directly (global_load_lds_dwordx4: lane i's 16 bytes land at M0 base + 16 i,
    // tools/probes/probe_lds_dma.hip), no register holds them across the two convolutions.  (Through registers they crossed conv3b, whose 108 weight
    // registers pushed them into scratch: 8 KB of scratch written per CTU = 228 MB of HBM writes per launch against 8 MB of depth maps.)
    if (tid >= 256 && work + grid < total && park_fast(next, st_row, st_seg)) {
      unsigned char* pw = lds + P::PARK_OFF + __builtin_amdgcn_readfirstlane((tid - 256) >> 6) * 2048;   // this wave's 2 x 1 KB
      const long long base = (long long)next.f * F.frame_stride + (long long)((F.row_begin + next.ry) * 64 + st_row) * F.stride + next.cx * 64 + st_seg * 16;
      if (F.sample_bytes == 2) {
        const int16_t* src = reinterpret_cast<const int16_t*>(F.luma) + base;
        __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)src, (void __attribute__((address_space(3)))*)pw, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)(src + 8), (void __attribute__((address_space(3)))*)(pw + 1024), 16, 0, 0);
      } else {
        const uint8_t* src = reinterpret_cast<const uint8_t*>(F.luma) + base;
        __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)src, (void __attribute__((address_space(3)))*)pw, 16, 0, 0);
      }
    }
    d2_fill_halo<16, P::PX3, P::A3A_PITCH, P::A3A_MASK>(big, tid);
    d2_conv_m3<KC2, false, 16, P::A2_PITCH, P::A2_MASK, P::PX3, P::A3A_PITCH, P::A3A_MASK, true, RQB>(ra, big, L3a.frag, L3a.bias, w3a, b3a, L3a.shift,
                                                                                                   [&]() { d2_weights<KC3, KC3>(L3b.frag, L3b.bias, w3b, b3b); });
    D2_STAMP(5)   // conv3a
    __syncthreads();
    D2_STAMP(1)
    d2_conv_m3<KC3, false, 16, P::A3A_PITCH, P::A3A_MASK, P::PX3, P::PX3, 0, false, RQB>(big, ra, L3b.frag, L3b.bias, w3b, b3b, L3b.shift, []() {});
    D2_STAMP(6)   // conv3b
    __syncthreads();
    D2_STAMP(1)
    // ================= heads (waves 0-3: thread = position of the 16 x 16 map, DPP row = 16x16 block, wave = quadrant) | next CTU staged (waves 4-7) =================
    if (tid < 256) {
      unsigned t_ = threadIdx.x;
      asm volatile("" : "+v"(t_));
      const int lane = (int)(t_ & 63u), wave = (int)(t_ >> 6);
      const int qy = wave >> 1, qx = wave & 1, sblk = (lane >> 4) & 3, p = lane & 15;
      const int by = qy * 2 + (sblk >> 1), bx = qx * 2 + (sblk & 1);
      const int y = by * 4 + (p >> 2), x = bx * 4 + (p & 3);
      const int cp = W.c3_pad;
      unsigned o64 = (unsigned)(((y >> 1) * 8 + (x >> 1)) * cp), o32 = (unsigned)((2 * 64 + (y & 7) * 8 + (x & 7)) * cp), o16 = (unsigned)((4 * 64 + (y & 3) * 4 + (x & 3)) * cp);
      asm volatile("" : "+v"(o64), "+v"(o32), "+v"(o16));   // (the thread's weight rows are loop-invariant too: 144 registers if hoisted)
      const uint8_t* w64 = W.whead + o64;
      const uint8_t* w32 = W.whead + o32;
      const uint8_t* w16 = W.whead + o16;
      const unsigned char* a = ra + (y * 16 + x) * P::PX3;
      int s64a = 0, s64b = 0, s32a = 0, s32b = 0, s16a = 0, s16b = 0;
      auto dot16 = [](const uint4& v, const uint4& q, int acc) { return sdot4(v.w, q.w, sdot4(v.z, q.z, sdot4(v.y, q.y, sdot4(v.x, q.x, acc)))); };
#pragma unroll
      for (int j = 0; j < KC3 * 2; ++j) {
        const uint4 v = *reinterpret_cast<const uint4*>(a + 16 * j);
        s64a = dot16(v, *reinterpret_cast<const uint4*>(w64 + 16 * j), s64a); s64b = dot16(v, *reinterpret_cast<const uint4*>(w64 + (size_t)64 * cp + 16 * j), s64b);
        s32a = dot16(v, *reinterpret_cast<const uint4*>(w32 + 16 * j), s32a); s32b = dot16(v, *reinterpret_cast<const uint4*>(w32 + (size_t)64 * cp + 16 * j), s32b);
        s16a = dot16(v, *reinterpret_cast<const uint4*>(w16 + 16 * j), s16a); s16b = dot16(v, *reinterpret_cast<const uint4*>(w16 + (size_t)16 * cp + 16 * j), s16b);
      }
      const int r16a = dpp_row_sum(s16a), r16b = dpp_row_sum(s16b);
      const int r32a = dpp_row_sum(s32a), r32b = dpp_row_sum(s32b);
      const int r64a = dpp_row_sum(s64a), r64b = dpp_row_sum(s64b);
      const int q32a = __builtin_amdgcn_readlane(r32a, 0) + __builtin_amdgcn_readlane(r32a, 16) + __builtin_amdgcn_readlane(r32a, 32) + __builtin_amdgcn_readlane(r32a, 48);
      const int q32b = __builtin_amdgcn_readlane(r32b, 0) + __builtin_amdgcn_readlane(r32b, 16) + __builtin_amdgcn_readlane(r32b, 32) + __builtin_amdgcn_readlane(r32b, 48);
      const int q64a = __builtin_amdgcn_readlane(r64a, 0) + __builtin_amdgcn_readlane(r64a, 16) + __builtin_amdgcn_readlane(r64a, 32) + __builtin_amdgcn_readlane(r64a, 48);
      const int q64b = __builtin_amdgcn_readlane(r64b, 0) + __builtin_amdgcn_readlane(r64b, 16) + __builtin_amdgcn_readlane(r64b, 32) + __builtin_amdgcn_readlane(r64b, 48);
      if (p == 0) *reinterpret_cast<int2*>(logitL + 2 * (5 + by * 4 + bx)) = make_int2(hb16a + r16a, hb16b + r16b);
      if (lane == 0) {
        *reinterpret_cast<int2*>(logitL + 2 * (1 + qy * 2 + qx)) = make_int2(hb32a + q32a, hb32b + q32b);
        *reinterpret_cast<int2*>(logitL + 44 + 2 * wave) = make_int2(q64a, q64b);
      }
    } else if (tid >= 256 && work + grid < total) {
      // the tile's last readers were block 1's first convolutions; the samples have been parked in LDS since the head of block 3
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      Prefetched pk;
      pk.fast = park_fast(next, st_row, st_seg);
      pk.a = *reinterpret_cast<const uint4*>(lds + P::PARK_OFF + ((tid - 256) >> 6) * 2048 + ((tid - 256) & 63) * 16);
      pk.b = *reinterpret_cast<const uint4*>(lds + P::PARK_OFF + ((tid - 256) >> 6) * 2048 + 1024 + ((tid - 256) & 63) * 16);
      stage(pk, next, st_row, st_seg);
    }
    D2_STAMP(7)   // heads | staging
    __syncthreads();
    D2_STAMP(1)
    if (tid < 256)
      depth_map_of_ctu(F, logitL, nullptr, tid, lane, wave, pos.f, F.row_begin + pos.ry, pos.cx, band_rows, hb64a, hb64b, margin_split, margin_stop,
                       d_depth, d_depth_max, d_logits, d_flags, nullptr, false);
    D2_STAMP(8)   // depth map
#if defined(FHEVC_D2_STAMPS)
    tsum[9] += 1;
#endif
    pos = next;
    // no barrier here: the next block 1 writes R_a's halo and S (both dead), reads the tile (staged before the barrier above); the logits are rewritten only
    // behind the six barriers of the next CTU's convolutions
  }
#if defined(FHEVC_D2_STAMPS)
  if (tid == 64 * (FHEVC_D2_STAMPS - 1) && vblock < per_frame)
    for (int k = 0; k < 12; ++k) reinterpret_cast<unsigned long long*>(d_depth + (size_t)vblock * 256)[k] = tsum[k];
#endif
#undef D2_STAMP
}
