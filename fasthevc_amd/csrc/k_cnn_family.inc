// k_cnn_family.inc -- included by k_cnn.hip (inside its anonymous namespace; shares its helpers): the depth classifier for members of the
// REFERENCE'S BAYESIAN-OPTIMISATION NETWORK FAMILY (matlab/dataExtraction/OptimizeDeepNeuralNetworksUsingBayesianOptimizationExample.m
// :103-106 NetworkDepth in [1, 3]; :233-259 convBlock(3, F, depth) x 3 with F = round(32 / sqrt(depth)), 2F, 4F filters; :367-373).
// This file implements the members with ONE convolution per block (NetworkDepth 1: 32 / 64 / 128 filters -- and, as a cross-check of the
// code path, 16 / 32 / 64, which is the network of the tuned kernels above): bit-exact twin of oracle/fhevc_oracle.c: fho_cnn_ctu_family.
//
// Same fixed-point arithmetic and the same building blocks as the i8 form above, generalised over the channel widths:
//   * one 64x64 CTU per workgroup iteration (256 threads), persistent grid, 2 workgroups per CU;
//   * conv1 (1 -> C1) on the bf16 MFMA with the 2x2 max-pool folded into M, once per group of 16 filters;
//   * conv2 (C1 -> C2) and conv3 (C2 -> C3) on v_mfma_i32_32x32x32_i8: a K step = one tap x 32 input channels (lane half h = the
//     16-channel activation plane 2 k + h), M tiles of 32 output channels; conv2 keeps the in-lane 2x2 pool (four accumulators (dy, dx)
//     per pooled position), conv3 two output rows 8 apart per MFMA; weights come from L2 into registers at the head of each phase;
//   * activations between the layers travel as a - 128 in 16-channel planes in LDS; the conv3 map [256 positions][C3] with 16-byte
//     chunks XOR-swizzled by position;
//   * heads: thread = position, v_dot4_i32_i8 against per-position weights read from L2, quad / row reductions, LDS atomics for the
//     32- and 64-level sums; the depth map, soft ranges, logits and split-flag words by the same depth_map_of_ctu as above.
// The source Hadamard is not fused here (the stand-alone kernel runs).  Not tuned: round 3 adds the family to the kernel; its roofline
// line is reported by bench.py --family.
template <int C1, int C2, int C3>
struct LdsFam {
  static constexpr int G1 = C1 / 16;                           // conv1 filter groups = A1 planes
  static constexpr int K1 = (C1 + 31) / 32;                    // conv2 K chunks of 32 input channels (C1 = 16: the second plane holds "activation 0" under zero weights)
  static constexpr int P1 = 2 * K1;                            // A1 planes allocated
  static constexpr int M2 = C2 / 32, K2 = C2 / 32, M3 = C3 / 32;
  static constexpr int A1_PLANE_B = 35 * A1_ROW;               // 20160
  static constexpr int A1_OFF = 0;
  static constexpr int A3_OFF = 0;                             // conv3's map reuses A1's region (dead after conv2)
  static constexpr int R1_BYTES = (P1 * A1_PLANE_B > 256 * C3) ? P1 * A1_PLANE_B : 256 * C3;
  static constexpr int A2_OFF = R1_BYTES;
  static constexpr int A2_BYTES = (C2 / 16) * A2_PLANE;
  static constexpr int T_OFF = A2_OFF + A2_BYTES;
  static constexpr int T_BYTES = 37 * IN_PITCH * 4;
  static constexpr int BIAS_OFF = T_OFF + T_BYTES;             // int32 bias2[C2], bias3[C3]
  static constexpr int LOGIT_OFF = BIAS_OFF + (C2 + C3) * 4;   // 64 ints as Lds::LOGIT_OFF
  static constexpr int LDS_BYTES = LOGIT_OFF + 64 * 4;
  static_assert(C1 % 16 == 0 && C2 % 32 == 0 && (C3 == 64 || C3 == 128), "supported widths");
  static_assert(2 * LDS_BYTES <= 160 * 1024, "two workgroups per CU");
};

template <int C1, int C2, int C3>
__global__ __launch_bounds__(256, 2) void fhevc_cnn_family_kernel(FhevcFrames F, FhevcFamilyWeights W, uint8_t* __restrict__ d_depth, int32_t* __restrict__ d_logits,
                                                                   uint32_t* __restrict__ d_flags, uint8_t* __restrict__ d_depth_max, int margin_split, int margin_stop)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __builtin_amdgcn_s_setreg((1 << 11) | 1, 2);  // fp32 rounding toward -inf: v_cvt_pk_u8_f32 = floor + clamp (conv1's requant)
  using P = LdsFam<C1, C2, C3>;
  constexpr int G1 = P::G1, K1 = P::K1, M2 = P::M2, K2 = P::K2, M3 = P::M3, NC3 = C3 / 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int hb64a = W.bhead[0], hb64b = W.bhead[1] + W.bhead[6 + 0 * 52 + F.qp];
  const int hb32a = W.bhead[2], hb32b = W.bhead[3] + W.bhead[6 + 1 * 52 + F.qp];
  const int hb16a = W.bhead[4], hb16b = W.bhead[5] + W.bhead[6 + 2 * 52 + F.qp];
  int* biasL = reinterpret_cast<int*>(lds + P::BIAS_OFF);
  int* logitL = reinterpret_cast<int*>(lds + P::LOGIT_OFF);
  for (int i = tid; i < C2 + C3; i += 256) biasL[i] = W.bias_i8[i];
  // "activation 0" everywhere in A1 and A2 (halos; the second plane of a 16-channel A1), bf16(128) everywhere in the tile
  for (int i = tid; i < (P::P1 * P::A1_PLANE_B) / 16; i += 256) *reinterpret_cast<uint4*>(lds + P::A1_OFF + i * 16) = make_uint4(0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u);
  for (int i = tid; i < P::A2_BYTES / 16; i += 256) *reinterpret_cast<uint4*>(lds + P::A2_OFF + i * 16) = make_uint4(0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u);
  for (int i = tid; i < P::T_BYTES / 16; i += 256) *reinterpret_cast<uint4*>(lds + P::T_OFF + i * 16) = make_uint4(0x43004300u, 0x43004300u, 0x43004300u, 0x43004300u);
  if (tid < 64) logitL[tid] = 0;
  __syncthreads();

  const int band_rows = F.row_end - F.row_begin;
  const int per_frame = band_rows * F.ctus_x;
  const int total = per_frame * F.num_frames;
  const int shift_in = F.bit_depth - 8;
  const int shift2 = W.shift[1], shift3 = W.shift[2];
  const int ld_row = tid >> 2, ld_seg = tid & 3;
  const int grid = (int)gridDim.x;
  const int vblock = (grid & 7) ? (int)blockIdx.x : (int)((blockIdx.x & 7) * (grid >> 3) + (blockIdx.x >> 3));
  CtuPos pos, step;
  {
    const int vb = min(vblock, total - 1);
    pos.f = vb / per_frame; pos.ry = (vb - pos.f * per_frame) / F.ctus_x; pos.cx = (vb - pos.f * per_frame) - pos.ry * F.ctus_x;
    step.f = grid / per_frame; step.ry = (grid - step.f * per_frame) / F.ctus_x; step.cx = (grid - step.f * per_frame) - step.ry * F.ctus_x;
  }
  auto frag1 = [](const unsigned char* p) {
    const uint2 lo = *reinterpret_cast<const uint2*>(p);
    const uint2 hi = *reinterpret_cast<const uint2*>(p + IN_PITCH * 4);
    return __builtin_bit_cast(bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
  };
  // halo cells of A1 this thread re-fills after conv3's map has used the region: 132 positions x G1 planes (the rest is rewritten by conv1)
  auto refill_a1_halo = [&]() {
    for (int e = tid; e < 132 * G1; e += 256) {
      const int pl = e / 132, k0 = e - pl * 132;
      int y, x;
      if (k0 < 34) { y = 0; x = k0; }
      else if (k0 < 68) { y = 33; x = k0 - 34; }
      else { const int k = k0 - 68; y = 1 + (k >> 1); x = (k & 1) ? 33 : 0; }
      *reinterpret_cast<uint4*>(lds + P::A1_OFF + pl * P::A1_PLANE_B + y * A1_ROW + ((x & 1) ? 0 : A1_EVEN) + (x >> 1) * 16) =
          make_uint4(0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u);
    }
  };

  Prefetched pre = prefetch_ctu<false>(F, vblock < total, pos, ld_row, ld_seg);
  if (vblock < total) stage_ctu<false>(lds, P::T_OFF, pre, F, pos, tid, ld_row, ld_seg, shift_in, 0u);
  __syncthreads();

  for (int work = vblock; work < total; work += grid) {
    const CtuPos next = advance(pos, step, band_rows, F.ctus_x);
    // ================= conv1 (1 -> C1): per group of 16 filters two MFMAs per pooled row, fused max-pool + requant =================
    {
      const unsigned char* c1_in = lds + P::T_OFF + (2 * r + 2 * h) * 4 + wave * (IN_PITCH * 4);
      unsigned char* c1_out = lds + P::A1_OFF + 8 * h + (wave + 1) * A1_ROW + (((r + 1) & 1) ? 0 : A1_EVEN) + ((r + 1) >> 1) * 16;
      bf16x8 wa[G1], wb[G1];
      f32x16 bias1[G1];
#pragma unroll
      for (int g = 0; g < G1; ++g) {
        wa[g] = __builtin_bit_cast(bf16x8, W.frag1[(2 * g + 0) * 64 + lane]);
        wb[g] = __builtin_bit_cast(bf16x8, W.frag1[(2 * g + 1) * 64 + lane]);
        const float4 b0 = *reinterpret_cast<const float4*>(W.bias1 + 16 * g + 8 * h), b1 = *reinterpret_cast<const float4*>(W.bias1 + 16 * g + 8 * h + 4);
        bias1[g][0] = b0.x; bias1[g][1] = b0.y; bias1[g][2] = b0.z; bias1[g][3] = b0.w; bias1[g][4] = b1.x; bias1[g][5] = b1.y; bias1[g][6] = b1.z; bias1[g][7] = b1.w;
#pragma unroll
        for (int i = 0; i < 8; ++i) bias1[g][8 + i] = bias1[g][i];
      }
#pragma unroll 2
      for (int i = 0; i < 8; ++i) {
        const bf16x8 bq = frag1(c1_in + i * (4 * IN_PITCH * 4));   // one fragment per pooled row, all filter groups
#pragma unroll
        for (int g = 0; g < G1; ++g) {
          const f32x16 acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa[g], bq, bias1[g], 0, 0, 0);
          const f32x16 acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wb[g], bq, bias1[g], 0, 0, 0);
          conv1_store_i8(acc0, acc1, c1_out + g * P::A1_PLANE_B + i * (4 * A1_ROW));
        }
      }
      // the 32- and 16-level logits start from their head biases (their last readers are two barriers back)
      if (tid < 40) logitL[2 + tid] = tid < 8 ? ((tid & 1) ? hb32b : hb32a) : ((tid & 1) ? hb16b : hb16a);
    }
    // conv2's first M tile of weights travels from L2 while the waves meet at the barrier
    bf16x8 w2[K1 * 9];
#pragma unroll
    for (int s = 0; s < K1 * 9; ++s) w2[s] = __builtin_bit_cast(bf16x8, W.frag2[s * 64 + lane]);
    __syncthreads();
    // ================= conv2 (C1 -> C2): K step = tap x 32 channels; lane = pooled position, four accumulators (dy, dx) =================
    {
      // wave priority 1 in the two MFMA phases (round 4), 0 elsewhere.  Measured: none (round 3) 1.2468 ms, level 1 for both workgroups 1.2372 (-0.8 %),
      // 1 + the workgroup's slot on its CU (the depth kernel's scheme) 1.2587 (+1.0 %): profiles/r04_ab_family_priority.log
      __builtin_amdgcn_s_setprio(1);
      const int q = r >> 2;
      const int pr = (q ^ (q >> 1) ^ (q >> 2)) & 1, pc = ((r >> 3) << 2) | (r & 3);
      const unsigned char* a1p = lds + P::A1_OFF + h * P::A1_PLANE_B + (2 * pr) * A1_ROW + pc * 16;
      unsigned char* a2dst = lds + P::A2_OFF + ((pr + 1) * A2_PITCH + pc + 1) * 16 + 4 * h;
#pragma unroll
      for (int mt = 0; mt < M2; ++mt) {   // one M tile's weights in registers at a time (K1 x 9 fragments)
        if (mt > 0) {
#pragma unroll
          for (int s = 0; s < K1 * 9; ++s) w2[s] = __builtin_bit_cast(bf16x8, W.frag2[(mt * K1 * 9 + s) * 64 + lane]);
        }
        const i32x16 binit = bias_tile_i8(biasL + 32 * mt, h);
        // one half-chain = the pre-pool outputs (dy, dx = 0) and (dy, dx = 1) of 32 pooled positions: K1 x 12 fragments, K1 x 18 MFMAs
        auto half = [&](const unsigned char* ub, int dy, i32x16& acc0, i32x16& acc1) {
          acc0 = binit; acc1 = binit;
#pragma unroll
          for (int k = 0; k < K1; ++k)
#pragma unroll
            for (int f = 0; f < 12; ++f) {
              const int ky = f / 4, c = f % 4;
              const bf16x8 b = lds_frag(ub + 2 * k * P::A1_PLANE_B + (dy + ky) * A1_ROW + ((c & 1) ? 0 : A1_EVEN) + (c >> 1) * 16);
              if (c < 3) acc0 = mfma_i8(w2[k * 9 + ky * 3 + c], b, acc0);
              if (c > 0) acc1 = mfma_i8(w2[k * 9 + ky * 3 + c - 1], b, acc1);
            }
        };
        // the two units of this wave, their pools and requants written where the NEXT half-chain can cover them (as conv2 of the tuned kernel)
        const unsigned char* u0b = a1p + (4 * wave) * A1_ROW;
        const unsigned char* u1b = a1p + (4 * (wave + 4)) * A1_ROW;
        unsigned char* d0 = a2dst + (2 * wave) * A2_PITCH * 16 + 2 * mt * A2_PLANE;
        unsigned char* d1 = a2dst + (2 * (wave + 4)) * A2_PITCH * 16 + 2 * mt * A2_PLANE;
        i32x16 t0, t1, a0, a1;
        half(u0b, 0, t0, t1);
        half(u0b, 1, a0, a1);
        pool_h_i8(t0, t1);
        pool_v_i8(t0, a0, a1);
        half(u1b, 0, t1, a0);
        conv2_requant_store_i8m<0>(t0, d0, shift2);
        half(u1b, 1, a1, t0);
        pool_h_i8(t1, a0);
        pool_v_i8(t1, a1, t0);
        conv2_requant_store_i8m<0>(t1, d1, shift2);
      }
      __builtin_amdgcn_s_setprio(0);
    }
    // conv3's weights (this wave's M tile) travel from L2 while the waves meet at the barrier
    constexpr int PER_WAVE = M3 * 8 / 4;              // (M tile, row pair) items per wave, M-tile-major: one M tile per wave
    const int mt3 = (wave * PER_WAVE) / 8, nt0 = (wave * PER_WAVE) % 8;
    bf16x8 w3[K2 * 9];
#pragma unroll
    for (int s = 0; s < K2 * 9; ++s) w3[s] = __builtin_bit_cast(bf16x8, W.frag3[(mt3 * K2 * 9 + s) * 64 + lane]);
    __syncthreads();
    // ================= conv3 (C2 -> C3): K step = tap x 32 channels; an MFMA = 32 output channels x two output rows 8 apart =================
    pre = prefetch_ctu<false>(F, work + grid < total, next, ld_row, ld_seg);
    {
      __builtin_amdgcn_s_setprio(1);
      const int x = lane & 15, rs = (lane >> 4) & 1;
      const int psw = (x / (16 / NC3)) % NC3;           // chunk swizzle of the map's rows: the heads' 16-lane reads hit 16 distinct slots
      const i32x16 binit = bias_tile_i8(biasL + C2 + 32 * mt3, h);
      constexpr int STEPS = K2 * 9, RING = 4;           // fragment ring: reads run RING (pair, step) slots ahead of their MFMAs
      auto frag_off = [](int st) { return 2 * (st / 9) * A2_PLANE + (((st % 9) / 3) * A2_PITCH + (st % 9) % 3) * 16; };
#pragma unroll
      for (int it = 0; it < PER_WAVE; it += 2) {
        const int ya = nt0 + it, yb = nt0 + it + 1;     // row pairs (ya, ya + 8) and (yb, yb + 8)
        const unsigned char* pa = lds + P::A2_OFF + h * A2_PLANE + ((ya + 8 * rs) * A2_PITCH + x) * 16;
        const unsigned char* pb = lds + P::A2_OFF + h * A2_PLANE + ((yb + 8 * rs) * A2_PITCH + x) * 16;
        i32x16 acca = binit, accb = binit;
        bf16x8 ring[RING];
#pragma unroll
        for (int g = 0; g < RING; ++g) ring[g] = lds_frag(((g & 1) ? pb : pa) + frag_off(g >> 1));
#pragma unroll
        for (int g = 0; g < 2 * STEPS; ++g) {           // slot g = 2 step + pair
          if (g & 1) accb = mfma_i8(w3[g >> 1], ring[g % RING], accb);
          else acca = mfma_i8(w3[g >> 1], ring[g % RING], acca);
          if (g + RING < 2 * STEPS) ring[g % RING] = lds_frag((((g + RING) & 1) ? pb : pa) + frag_off((g + RING) >> 1));
        }
        unsigned char* da = lds + P::A3_OFF + ((ya + 8 * rs) * 16 + x) * C3 + 4 * h;
        unsigned char* db = lds + P::A3_OFF + ((yb + 8 * rs) * 16 + x) * C3 + 4 * h;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          *reinterpret_cast<unsigned*>(da + (((2 * mt3 + (g >> 1)) ^ psw) << 4) + 8 * (g & 1)) = requant4_i8(acca[4 * g], acca[4 * g + 1], acca[4 * g + 2], acca[4 * g + 3], shift3, 0);
          *reinterpret_cast<unsigned*>(db + (((2 * mt3 + (g >> 1)) ^ psw) << 4) + 8 * (g & 1)) = requant4_i8(accb[4 * g], accb[4 * g + 1], accb[4 * g + 2], accb[4 * g + 3], shift3, 0);
        }
      }
      __builtin_amdgcn_s_setprio(0);
    }
    __syncthreads();
    // ================= heads: thread = position (y = tid >> 4, x = tid & 15), v_dot4 against its rows of the three FC weights =================
    {
      // 16- and 32-level heads as ONE GEMM on v_mfma_i32_16x16x64_i8 (as P4 of the tuned kernel): rows = the 16 blocks of the CTU, a K step =
      // one position (py = wave, px) of a block x 64 channels (C3 / 64 chunks), columns = the weight variants: 0, 1 the 16-level classes,
      // 2 + 2 sub + class the 32-level weights of a block at sub-position sub of its quadrant.  The B operands come from L2 (W.headm:
      // [position 16][chunk][column 16][64 B]); lane (m = lane & 15 -> block (by, bx), kg = lane >> 4) reads the A operand from the map
      constexpr int KC = C3 / 64;
      const int m = lane & 15, kg = lane >> 4, by = m >> 2, bx = m & 3;
      i32x4 hacc = { 0, 0, 0, 0 };
#pragma unroll
      for (int px = 0; px < 4; ++px) {
        const int xx = 4 * bx + px;
        const unsigned char* arow = lds + P::A3_OFF + ((4 * by + wave) * 16 + xx) * C3;
        const int psw = (xx / (16 / NC3)) % NC3;
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) {
          const i32x4 av = *reinterpret_cast<const i32x4*>(arow + (((4 * kc + kg) ^ psw) << 4));
          const i32x4 bv = *reinterpret_cast<const i32x4*>(W.headm + ((size_t)(((4 * wave + px) * KC + kc) * 16 + m) * 64 + 16 * kg));
          hacc = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, bv, hacc, 0, 0, 0);
        }
      }
      // 64-level head on v_dot4_i32_i8: lane = one position of quadrant `wave` (a 16-lane row = one 16x16 block of it)
      int s64a = 0, s64b = 0;
      {
        const int q = wave, blk = lane >> 4;
        const int y = (q >> 1) * 8 + (blk >> 1) * 4 + ((lane >> 2) & 3), x = (q & 1) * 8 + (blk & 1) * 4 + (lane & 3);
        const int psw = (x / (16 / NC3)) % NC3;
        const unsigned char* arow = lds + P::A3_OFF + (y * 16 + x) * C3;
        const unsigned char* w64p = W.whead + (size_t)((y >> 1) * 8 + (x >> 1)) * C3;
#pragma unroll
        for (int c = 0; c < NC3; ++c) {
          const uint4 a = *reinterpret_cast<const uint4*>(arow + ((c ^ psw) << 4));
          const uint4 d0 = *reinterpret_cast<const uint4*>(w64p + 16 * c), d1 = *reinterpret_cast<const uint4*>(w64p + 64 * C3 + 16 * c);
          s64a = sdot4(a.x, d0.x, s64a); s64a = sdot4(a.y, d0.y, s64a); s64a = sdot4(a.z, d0.z, s64a); s64a = sdot4(a.w, d0.w, s64a);
          s64b = sdot4(a.x, d1.x, s64b); s64b = sdot4(a.y, d1.y, s64b); s64b = sdot4(a.z, d1.z, s64b); s64b = sdot4(a.w, d1.w, s64b);
        }
      }
      {
        const int n = lane & 15, rg = lane >> 4, subn = (n - 2) >> 1;
        const bool is16 = n < 2, is32 = n >= 2 && n < 10 && ((rg & 1) == (subn >> 1));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool act = is16 || (is32 && ((i & 1) == (subn & 1)));
          const int idx = is16 ? 2 * (5 + 4 * rg + i) + n : 2 * (1 + (rg >> 1) * 2 + (i >> 1)) + (n & 1);
          if (act) atomicAdd(logitL + idx, hacc[i]);
        }
      }
      const int r64a = dpp_row_sum(s64a), r64b = dpp_row_sum(s64b);
      const int q64a = __builtin_amdgcn_readlane(r64a, 0) + __builtin_amdgcn_readlane(r64a, 16) + __builtin_amdgcn_readlane(r64a, 32) + __builtin_amdgcn_readlane(r64a, 48);
      const int q64b = __builtin_amdgcn_readlane(r64b, 0) + __builtin_amdgcn_readlane(r64b, 16) + __builtin_amdgcn_readlane(r64b, 32) + __builtin_amdgcn_readlane(r64b, 48);
      if (lane == 0) *reinterpret_cast<int2*>(logitL + 44 + 2 * wave) = make_int2(q64a, q64b);
      if (work + grid < total) stage_ctu<false>(lds, P::T_OFF, pre, F, next, tid, ld_row, ld_seg, shift_in, 0u);
    }
    __syncthreads();
    // ================= depth map (and the optional outputs), A1's halo for the next CTU =================
    depth_map_of_ctu(F, logitL, logitL + 56, tid, lane, wave, pos.f, F.row_begin + pos.ry, pos.cx, band_rows, hb64a, hb64b, margin_split, margin_stop,
                     d_depth, d_depth_max, d_logits, d_flags, nullptr, false);
    refill_a1_halo();
    __syncthreads();
    pos = next;
  }
}
