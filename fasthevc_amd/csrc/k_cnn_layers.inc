// k_cnn_layers.inc -- the GENERIC path of the reference's Bayesian-optimisation network family (Optimize...Example.m:103-106, 233-259): any member
// (NetworkDepth 1..3 convolutions per block, widths up to 128) layer by layer through HBM.  Included by k_cnn.hip (shares its epilogues).
//
// The two fused kernels (k_cnn.hip: 16/32/64, k_cnn_family.inc: 32/64/128) keep a CTU's activations in LDS from the samples to the depth map;
// the deeper members do not fit there (23/46/92 x 2: the second convolution of block 1 alone reads 66 x 66 x 32 B = 139 KB per CTU), so their
// activations travel through HBM -- [CTU][H + 2] rows of [H + 2][C padded to 32] signed bytes a - 128 (+ the row padding of the consumer's LDS image), the halo ("activation 0" = -128, written once when
// the buffer is allocated) part of the tensor so that a convolution needs no edge logic -- one launch per convolution over a chunk of CTUs:
//   fhevc_layers_stage_kernel   picture -> [CTU][66][66] centred samples (halo and samples outside the picture: 0, as the oracle's fho_load_ctu)
//   fhevc_layer_conv_kernel     conv3x3 (+ 2x2 max-pool) + requant on v_mfma_i32_32x32x32_i8: a WAVE owns one M tile (32 output channels) of one
//                               CTU at a time, its A fragments (9 taps x Cin / 32 chunks) resident in registers for the whole launch; N tile = 32
//                               output positions, B operand = 16 bytes per lane from the input map (or a strip of its rows) staged in LDS by the
//                               workgroup -- two buffers, the next item streamed in by LDS-direct loads behind the current one's MFMAs, the image
//                               padded / XOR-ed so that the reads are conflict-free -- or, for the first layer, straight from HBM; pooled layers
//                               keep four accumulators (dy, dx) per pooled position and take their maximum in the lane; rows of the A fragments
//                               permuted so that a lane's 16 results are 16 consecutive channels = one 16-byte store.
//   fhevc_layers_heads_kernel   the three FC heads on v_dot4_i32_i8 (thread = position of the 16 x 16 map, DPP row = 16x16 block, wave = quadrant;
//                               the CTU's last map staged in LDS by one coalesced copy, the thread's six weight rows resident in registers),
//                               QP prior, depth map / ranges / logits / flag word through depth_map_of_ctu.
// Bit-exact with oracle/fhevc_oracle.c: fho_cnn_ctu_family (tests/test_gpu_family.py).

// (inside k_cnn.hip's anonymous namespace; the launcher is at the end of k_cnn.hip)

// the lane's 16 accumulators = 16 consecutive channels (rows of the A fragments permuted on the host): requant, one 16-byte store
// RQ: the requant form (requant4_i8): 0 general (36 instructions per 16 values), 1 for shifts up to 7 (28), 2 for shift 8 with every accumulator inside 24 bits (20);
// the host says which a layer qualifies for (FhevcLayer::rq)
template <int RQ = 0>
__device__ __forceinline__ void layer_store16(const i32x16& acc, unsigned char* dst, int shift)
{
  uint4 v;
  v.x = requant4_i8(acc[0], acc[1], acc[2], acc[3], shift, RQ);
  v.y = requant4_i8(acc[4], acc[5], acc[6], acc[7], shift, RQ);
  v.z = requant4_i8(acc[8], acc[9], acc[10], acc[11], shift, RQ);
  v.w = requant4_i8(acc[12], acc[13], acc[14], acc[15], shift, RQ);
  *reinterpret_cast<uint4*>(dst) = v;
}

template <typename T>
__global__ __launch_bounds__(256) void fhevc_layers_stage_kernel(FhevcFrames F, int first, int count, int8_t* __restrict__ in0)
{
  const int band_rows = F.row_end - F.row_begin, per_frame = band_rows * F.ctus_x;
  const T* plane = reinterpret_cast<const T*>(F.luma);
  const int sh = F.bit_depth - 8;
  for (int k = blockIdx.x; k < count; k += gridDim.x) {
    const int g = first + k, f = g / per_frame, rem = g - f * per_frame;
    const int cy = F.row_begin + rem / F.ctus_x, cx = rem % F.ctus_x;
    int8_t* dst = in0 + (size_t)k * 66 * 66;
    for (int i = threadIdx.x; i < 66 * 66; i += 256) {
      const int y = i / 66 - 1, x = i % 66 - 1;
      const int px = cx * 64 + x, py = cy * 64 + y;
      int v = 0;
      if (x >= 0 && x < 64 && y >= 0 && y < 64 && px < F.width && py < F.height) {
        int p = (int)plane[(long long)f * F.frame_stride + (long long)py * F.stride + px];
        if (sh > 0) p = min(255, (p + (1 << (sh - 1))) >> sh);
        v = min(max(p, 0), 255) - 128;
      }
      dst[i] = (int8_t)v;
    }
  }
}

// KC = Cin_pad / 32 (0: the first layer); POOL: 2x2 max-pool behind the convolution; LDS: the workgroup stages a CTU's whole input map (halo
// included: one contiguous copy) in LDS and its waves -- M tile = wave % MT, the N tiles dealt over the waves of an M tile -- read their B operands
// from there (the maps of 32 x 32 and 16 x 16 positions fit: at most 34 x 34 x 64 B = 74 KB); otherwise every wave reads HBM / L2 directly
// FUSE0 (LDS form of the SECOND convolution of a member with two or three convolutions per block): the strip of the first convolution's output is
// not copied from HBM but computed into LDS from the CTU's sample tile (first.in0: [CTU][66][66] bytes) -- one MFMA per 32 positions and M tile --
// so that the first convolution's launch, its 139 KB per CTU of output and their re-read disappear
#ifndef FHEVC_LAYER_RING
#define FHEVC_LAYER_RING 6   // B fragments in flight ahead of their MFMAs
#endif
constexpr int RINGL = FHEVC_LAYER_RING;
struct FhevcFirstConv { const int8_t* in0; const uint4* frag; const int32_t* bias; int shift; };
// one LDS-direct load: every lane's 16 bytes at gsrc land at LDS byte address lds_dst (wave-uniform) + 16 x lane, no register in between.  hipcc does
// not count it: the issuer waits vmcnt(0) itself before the barrier that publishes the buffer
__device__ __forceinline__ void layer_glds16(const void* gsrc, unsigned lds_dst)
{
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0" : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
template <int KC, bool POOL, bool LDS, bool FUSE0 = false>
__global__ __launch_bounds__(256, 2) void fhevc_layer_conv_kernel(const int8_t* __restrict__ in, int8_t* __restrict__ out, const uint4* __restrict__ frag,
                                                               const int32_t* __restrict__ bias, int shift, int H, int cout_pad, int ctus, int strip_rows,
                                                               FhevcFirstConv first, int dbuf, int in_pad, int out_pad, int swz)
{
  // in_pad / out_pad: bytes added to the row pitch of the input / output tensor; swz: the LDS image keeps byte a of the staged map at
  // a ^ (((a >> 8) & swz) << 4).  Together they make every B-fragment read (ds_read_b128) free of bank conflicts (tools/lds_swizzle_search.py; plain
  // images cost 2 .. 8 LDS cycles per cycle of data and bound the kernel)
  // strip_rows (LDS form only): pre-pool output rows per workgroup item; H: the whole map.  A 64 x 64 map is staged in two strips of 32 rows
  // (34 input rows x 66 x 32 B = 71.8 KB)
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_map[];
  constexpr int NF = KC == 0 ? 1 : KC * 9;     // A fragments of an M tile
  constexpr int NA = POOL ? 4 : 2;             // accumulators in flight: the four pre-pool outputs of a pooled position / two N tiles
  const int lane = threadIdx.x & 63, n = lane & 31, h = lane >> 5;
  const int MT = cout_pad >> 5;
  const int gw = LDS ? (int)(threadIdx.x >> 6) : blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nw = gridDim.x * 4;   // (not LDS) a multiple of 12: every wave keeps its M tile
  const int mt = gw % MT;
  const int nsub = LDS ? (MT >= 3 ? 1 : 4 / MT) : 1, sub = LDS ? gw / MT : 0;   // LDS: waves per M tile, this wave's share of the N tiles
  const bool active = !LDS || gw < MT * nsub;                                    // (96 channels: three M tiles, the fourth wave only helps staging)
  const int Ho = POOL ? H >> 1 : H, lg = Ho == 64 ? 6 : (Ho == 32 ? 5 : 4);
  constexpr int S = POOL ? 2 : 1;
  const int px_bytes = KC == 0 ? 1 : KC * 32;            // bytes per input position
  const int in_pitch = (H + 2) * px_bytes + in_pad;
  const size_t in_ctu = (size_t)(H + 2) * in_pitch;
  const int out_pitch = (Ho + 2) * cout_pad + out_pad;
  const size_t out_ctu = (size_t)(Ho + 2) * out_pitch;
  bf16x8 wA[NF];
#pragma unroll
  for (int s = 0; s < NF; ++s) wA[s] = __builtin_bit_cast(bf16x8, frag[((size_t)mt * NF + s) * 64 + lane]);
  i32x16 binit;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int4 v = *reinterpret_cast<const int4*>(bias + mt * 32 + 16 * h + 4 * g);
    binit[4 * g + 0] = v.x; binit[4 * g + 1] = v.y; binit[4 * g + 2] = v.z; binit[4 * g + 3] = v.w;
  }
  // the weights are in their registers before the item loop: left alone, hipcc waits for them at their first use INSIDE the loop with vmcnt(0), which
  // also drains the LDS-direct loads of the next item that are meant to stay in flight behind the MFMAs
#pragma unroll
  for (int s = 0; s < NF; ++s) asm volatile("" :: "v"(wA[s]));
  asm volatile("" :: "v"(binit));
  // FUSE0: the first convolution's fragments and bias as well (hoisted out of the loop by hipcc, but waited for inside it: vmcnt(0) in front of every
  // staging MFMA, i.e. behind the previous strip's stores)
  constexpr int KF = FUSE0 ? KC : 1;
  bf16x8 f0[KF];
  i32x16 b0[KF];
  if constexpr (FUSE0) {
#pragma unroll
    for (int m0 = 0; m0 < KF; ++m0) {
      f0[m0] = __builtin_bit_cast(bf16x8, first.frag[(size_t)m0 * 64 + lane]);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int4 v = *reinterpret_cast<const int4*>(first.bias + m0 * 32 + 16 * h + 4 * g);
        b0[m0][4 * g + 0] = v.x; b0[m0][4 * g + 1] = v.y; b0[m0][4 * g + 2] = v.z; b0[m0][4 * g + 3] = v.w;
      }
#if defined(__HIP_DEVICE_COMPILE__)   // (the host pass drops the whole instantiation, silently, if it sees these two)
      asm volatile("" :: "v"(f0[m0]));
      asm volatile("" :: "v"(b0[m0]));
#endif
    }
  }
  const int tiles = (Ho * Ho) >> 5;
  constexpr int TS = POOL ? 1 : 2;
  const int nstrips = LDS ? H / strip_rows : 1;
  const int strip_tiles = tiles / nstrips;   // N tiles of a strip
  const int items = LDS ? ctus * nstrips : ctus;
  // dbuf (LDS form, maps that come from HBM): two map buffers; item k + 1 streams into the other one by LDS-direct loads while item k's MFMAs run
  // (single-buffered, a workgroup's staging and compute add up: tools/experiments/README.md), one barrier per item
  const int n16 = ((strip_rows + 2) * in_pitch) >> 4, n16r = (n16 + 15) & ~15;   // 16-byte pieces of a staged strip; rounded to whole 256-byte rows
  const bool two = LDS && !FUSE0 && dbuf != 0;
  // (only where the plain image is four or more ways conflicted: at two ways the address arithmetic costs what the conflicts did)
  constexpr bool SWZ = KC == 2 || KC == 4 || (KC == 3 && POOL);
  auto swz_off = [&](unsigned a) { return SWZ ? a ^ (((a >> 8) & (unsigned)swz) << 4) : a; };
  auto prefetch = [&](int it, int buf) {
    const int c = it / nstrips, s = it - c * nstrips;
    const uint4* src = reinterpret_cast<const uint4*>(in + (size_t)c * in_ctu + (size_t)(s * strip_rows) * in_pitch);
    const unsigned dst = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lds_map + (unsigned)buf * ((unsigned)n16r << 4);
    for (int j = 0; j < n16r; j += 256) {
      const int i = j + (int)threadIdx.x, si = SWZ ? i ^ ((i >> 4) & swz) : i;   // the LDS side of an LDS-direct load is lane-linear: the image's XOR goes on the source
      if (si < n16) layer_glds16(src + si, __builtin_amdgcn_readfirstlane(dst + (unsigned)((j + (int)(threadIdx.x & ~63u)) << 4)));
    }
  };
  int parity = 0;
  if (two && (int)blockIdx.x < items) prefetch((int)blockIdx.x, 0);
  for (int item = LDS ? (int)blockIdx.x : gw / MT; item < items; item += LDS ? (int)gridDim.x : nw / MT) {
    const int ctu = LDS ? item / nstrips : item, sidx = LDS ? item - ctu * nstrips : 0;
    const int8_t* ip = nullptr;
    const unsigned char* lb = lds_map;                              // LDS form: the staged strip, and the byte offset of its first row in the whole map
    const int ybias = LDS ? sidx * strip_rows * in_pitch : 0;
    if (two) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's share of the item has landed (and its stores of the previous one have left)
      __syncthreads();                                    // ... everyone's; the other buffer's readers are done
      if (item + (int)gridDim.x < items) prefetch(item + (int)gridDim.x, parity ^ 1);
      lb = lds_map + (size_t)parity * ((size_t)n16r << 4);
      parity ^= 1;
    } else if constexpr (LDS) {
      __syncthreads();   // the previous item's readers are done
      const int y0 = sidx * strip_rows;   // the strip's first input row (halo coordinates): rows y0 .. y0 + strip_rows + 1 are one contiguous run
      if constexpr (FUSE0) {
        // rows y0 .. y0 + strip_rows + 1 (halo coordinates) of the first convolution's output, 64 positions + two halo columns each, KC x 32 channels:
        // halo rows / columns = "activation 0"; the rest one MFMA per 32 positions and M tile (K = the nine taps), requant, 16-byte LDS stores
        const int wave = threadIdx.x >> 6;
        // the sample rows this strip's first convolution reads, copied to LDS behind the map first (one coalesced pass: nine dependent byte loads
        // per lane and tile straight from HBM made this staging the longest part of the kernel)
        const int rlo = max(y0 - 1, 0), rhi = min(y0 + strip_rows + 2, 65);
        unsigned char* tile = lds_map + ((size_t)n16r << 4);
        {
          const unsigned short* src = reinterpret_cast<const unsigned short*>(first.in0 + (size_t)ctu * 66 * 66 + rlo * 66);
          for (int i = threadIdx.x; i < (rhi - rlo + 1) * 33; i += 256) reinterpret_cast<unsigned short*>(tile)[i] = src[i];
        }
        __syncthreads();
        const unsigned char* t0 = tile - rlo * 66;   // addressed as the whole 66 x 66 tile
        const uint4 zero = make_uint4(0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u);
        for (int tt = wave; tt < (strip_rows + 2) * 2; tt += 4) {
          const int r = y0 + (tt >> 1), xs = (tt & 1) * 32;          // row in halo coordinates (image row r - 1), first image column of the tile
          const unsigned row = (unsigned)(tt >> 1) * (unsigned)in_pitch;   // byte offset in the strip's image
          if (n == 0 && (tt & 1) == 0) {                              // the two halo columns of this row
#pragma unroll
            for (int c = 0; c < KC * 2; ++c) *reinterpret_cast<uint4*>(lds_map + swz_off(row + (h == 0 ? 0u : (unsigned)(H + 1) * px_bytes) + 16u * c)) = zero;
          }
          if (r == 0 || r == H + 1) {
#pragma unroll
            for (int c = 0; c < KC; ++c) *reinterpret_cast<uint4*>(lds_map + swz_off(row + (unsigned)(xs + n + 1) * px_bytes + c * 32 + 16 * h)) = zero;
            continue;
          }
          // the 3 x 3 window as the two ALIGNED dwords around each of its three rows + v_alignbyte, packed by two v_perm (round 4: sub-dword LDS reads --
          // the nine ds_read_u8 this replaces -- cost the fused two-convolution kernel ~750 cycles per tile, k_cnn_d2.inc).  Every lane reads: lanes 32-63 the
          // same bytes as lanes 0-31; their K slots, like slots 9 .. 15, meet zero weights (fhevc_weights.hip: build_layers_image)
          uint4 bq;
          {
            const unsigned char* q = t0 + (r - 1) * 66 + xs + n;
            unsigned rw[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              const unsigned a = (unsigned)(size_t)(__attribute__((address_space(3))) const unsigned char*)(q + k * 66);
              const unsigned* qd = reinterpret_cast<const unsigned*>(q + k * 66 - (a & 3u));
              rw[k] = __builtin_amdgcn_alignbyte(qd[1], qd[0], a & 3u);
            }
            bq.x = __builtin_amdgcn_perm(rw[1], rw[0], 0x04020100u);
            bq.y = __builtin_amdgcn_perm(rw[2], rw[1], 0x05040201u);
            bq.z = rw[2] >> 16;
            bq.w = 0;
          }
#pragma unroll
          for (int m0 = 0; m0 < KC; ++m0) {
            const i32x16 a0 = mfma_i8(f0[m0], __builtin_bit_cast(bf16x8, bq), b0[m0]);
            layer_store16(a0, lds_map + swz_off(row + (unsigned)(xs + n + 1) * px_bytes + m0 * 32 + 16 * h), first.shift);
          }
        }
      } else {
        const uint4* src = reinterpret_cast<const uint4*>(in + (size_t)ctu * in_ctu + (size_t)y0 * in_pitch);
        for (int i = threadIdx.x; i < n16; i += 256) reinterpret_cast<uint4*>(lds_map)[SWZ ? i ^ ((i >> 4) & swz) : i] = src[i];
      }
      __syncthreads();
    } else {
      ip = in + (size_t)ctu * in_ctu;
    }
    int8_t* op = out + (size_t)ctu * out_ctu;
    for (int t = sidx * strip_tiles + sub * TS; active && t < (sidx + 1) * strip_tiles; t += nsub * TS) {
      i32x16 acc[NA];
#pragma unroll
      for (int a = 0; a < NA; ++a) acc[a] = binit;
      int oy[2], ox[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) { const int p = (t + u) * 32 + n; oy[u] = p >> lg; ox[u] = p & (Ho - 1); }
      if constexpr (KC == 0) {
        // first layer: K = the nine taps; lane half 0 carries them in bytes 0..8, lane half 1 zeros
        if constexpr (POOL) {
          unsigned win[4][4];
          const int8_t* q = ip + (oy[0] * 2) * in_pitch + ox[0] * 2;
#pragma unroll
          for (int iy = 0; iy < 4; ++iy)
#pragma unroll
            for (int ix = 0; ix < 4; ++ix) win[iy][ix] = (unsigned)(unsigned char)q[iy * in_pitch + ix];
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            const int dy = a >> 1, dx = a & 1;
            uint4 b = make_uint4(0, 0, 0, 0);
            if (h == 0) {
              b.x = win[dy][dx] | (win[dy][dx + 1] << 8) | (win[dy][dx + 2] << 16) | (win[dy + 1][dx] << 24);
              b.y = win[dy + 1][dx + 1] | (win[dy + 1][dx + 2] << 8) | (win[dy + 2][dx] << 16) | (win[dy + 2][dx + 1] << 24);
              b.z = win[dy + 2][dx + 2];
            }
            acc[a] = mfma_i8(wA[0], __builtin_bit_cast(bf16x8, b), acc[a]);
          }
        } else {
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const int8_t* q = ip + oy[u] * in_pitch + ox[u];
            uint4 b = make_uint4(0, 0, 0, 0);
            if (h == 0) {
              unsigned w9[9];
#pragma unroll
              for (int k = 0; k < 9; ++k) w9[k] = (unsigned)(unsigned char)q[(k / 3) * in_pitch + k % 3];
              b.x = w9[0] | (w9[1] << 8) | (w9[2] << 16) | (w9[3] << 24);
              b.y = w9[4] | (w9[5] << 8) | (w9[6] << 16) | (w9[7] << 24);
              b.z = w9[8];
            }
            acc[u] = mfma_i8(wA[0], __builtin_bit_cast(bf16x8, b), acc[u]);
          }
        }
      } else if constexpr (POOL) {
        // the 4 x 4 input positions around a pooled position: position (iy, ix) is tap (iy - dy, ix - dx) of the pre-pool output (dy, dx).
        // The B fragments run RINGL reads ahead of their MFMAs (left to itself hipcc reads each one right in front of its MFMA and waits for it:
        // the LDS latency 16 / 27 times per tile -- the ISA showed w M r w M r ... and the MFMA pipe a quarter busy)
        const int q = (oy[0] * 2) * in_pitch + (ox[0] * 2) * px_bytes + 16 * h - ybias;
        constexpr int NS = (KC == 0 ? 1 : KC) * 16;
        auto frag_b = [&](int i) {
          const int o = q + ((i & 15) >> 2) * in_pitch + (i & 3) * px_bytes + (i >> 4) * 32;
          if constexpr (LDS) return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(lb + swz_off((unsigned)o)));
          else return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(ip + o));
        };
        bf16x8 ring[RINGL];
#pragma unroll
        for (int i = 0; i < RINGL && i < NS; ++i) ring[i] = frag_b(i);
#pragma unroll
        for (int i = 0; i < NS; ++i) {
          const bf16x8 b = ring[i % RINGL];
          if (i + RINGL < NS) ring[i % RINGL] = frag_b(i + RINGL);
          const int kc = i >> 4, iy = (i & 15) >> 2, ix = i & 3;
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            const int ky = iy - (a >> 1), kx = ix - (a & 1);
            if (ky >= 0 && ky < 3 && kx >= 0 && kx < 3) acc[a] = mfma_i8(wA[kc * 9 + ky * 3 + kx], b, acc[a]);
          }
        }
      } else {
        constexpr int NS = (KC == 0 ? 1 : KC) * 18;   // (K chunk, tap, N tile of the pair)
        const int q0 = oy[0] * in_pitch + ox[0] * px_bytes + 16 * h - ybias;
        const int q1 = oy[1] * in_pitch + ox[1] * px_bytes + 16 * h - ybias;
        auto frag_b = [&](int i) {
          const int tap = (i >> 1) % 9;
          const int o = ((i & 1) ? q1 : q0) + (tap / 3) * in_pitch + (tap % 3) * px_bytes + (i / 18) * 32;
          if constexpr (LDS) return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(lb + swz_off((unsigned)o)));
          else return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(ip + o));
        };
        bf16x8 ring[RINGL];
#pragma unroll
        for (int i = 0; i < RINGL && i < NS; ++i) ring[i] = frag_b(i);
#pragma unroll
        for (int i = 0; i < NS; ++i) {
          const bf16x8 b = ring[i % RINGL];
          if (i + RINGL < NS) ring[i % RINGL] = frag_b(i + RINGL);
          acc[i & 1] = mfma_i8(wA[(i / 18) * 9 + (i >> 1) % 9], b, acc[i & 1]);
        }
      }
      if constexpr (POOL) {
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[0][k] = max(max(acc[0][k], acc[1][k]), max(acc[2][k], acc[3][k]));
        layer_store16(acc[0], reinterpret_cast<unsigned char*>(op) + (size_t)(oy[0] + 1) * out_pitch + (ox[0] + 1) * cout_pad + mt * 32 + 16 * h, shift);
      } else {
#pragma unroll
        for (int u = 0; u < 2; ++u)
          layer_store16(acc[u], reinterpret_cast<unsigned char*>(op) + (size_t)(oy[u] + 1) * out_pitch + (ox[u] + 1) * cout_pad + mt * 32 + 16 * h, shift);
      }
    }
  }
}

// CP = c3_pad / 32: a thread's position is the same for every CTU, so its six weight rows (two classes x three heads, CP x 32 bytes each) stay in
// registers for the whole launch (read per CTU from L1 they were six 16-byte loads per step on a kernel that is bound by its load instructions)
template <int CP>
__global__ __launch_bounds__(256, 2) void fhevc_layers_heads_kernel(FhevcFrames F, const int8_t* __restrict__ a3, int c3, int c3_pad, const uint8_t* __restrict__ whead,
                                                                 const int32_t* __restrict__ bhead, int first, int count, uint8_t* __restrict__ d_depth,
                                                                 int32_t* __restrict__ d_logits, uint32_t* __restrict__ d_flags, uint8_t* __restrict__ d_depth_max,
                                                                 int margin_split, int margin_stop)
{
  __shared__ __attribute__((aligned(16))) int logitL[64];
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_map[];   // the CTU's last map, halo included: 18 x 18 x c3_pad bytes
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int band_rows = F.row_end - F.row_begin, per_frame = band_rows * F.ctus_x;
  const int hb64a = bhead[0], hb64b = bhead[1] + bhead[6 + 0 * 52 + F.qp];
  const int hb32a = bhead[2], hb32b = bhead[3] + bhead[6 + 1 * 52 + F.qp];
  const int hb16a = bhead[4], hb16b = bhead[5] + bhead[6 + 2 * 52 + F.qp];
  // wave = quadrant (z-order), 16-lane row = 16x16 block of it, lane in the row = position of the block's 4 x 4
  const int qy = wave >> 1, qx = wave & 1, s = (lane >> 4) & 3, p = lane & 15;
  const int by = qy * 2 + (s >> 1), bx = qx * 2 + (s & 1);
  const int y = by * 4 + (p >> 2), x = bx * 4 + (p & 3);
  const uint8_t* w64 = whead + ((size_t)(y >> 1) * 8 + (x >> 1)) * c3_pad;
  const uint8_t* w32 = whead + (size_t)2 * 64 * c3_pad + ((size_t)(y & 7) * 8 + (x & 7)) * c3_pad;
  const uint8_t* w16 = whead + (size_t)4 * 64 * c3_pad + ((size_t)(y & 3) * 4 + (x & 3)) * c3_pad;
  uint4 wr[6][CP * 2];
#pragma unroll
  for (int j = 0; j < CP * 2; ++j) {
    wr[0][j] = *reinterpret_cast<const uint4*>(w64 + 16 * j); wr[1][j] = *reinterpret_cast<const uint4*>(w64 + (size_t)64 * c3_pad + 16 * j);
    wr[2][j] = *reinterpret_cast<const uint4*>(w32 + 16 * j); wr[3][j] = *reinterpret_cast<const uint4*>(w32 + (size_t)64 * c3_pad + 16 * j);
    wr[4][j] = *reinterpret_cast<const uint4*>(w16 + 16 * j); wr[5][j] = *reinterpret_cast<const uint4*>(w16 + (size_t)16 * c3_pad + 16 * j);
  }
  for (int k = blockIdx.x; k < count; k += gridDim.x) {
    // the map comes in as ONE contiguous, fully coalesced copy (a thread reading its own position straight from HBM touches 64 different lines per
    // wave-instruction: 2 TB/s); several workgroups per CU hide the copy of one behind the dot products of the others
    __syncthreads();   // the previous CTU's readers of the map are done
    {
      const uint4* src = reinterpret_cast<const uint4*>(a3 + (size_t)k * 18 * 18 * c3_pad);
      for (int i = tid; i < (18 * 18 * c3_pad) >> 4; i += 256) reinterpret_cast<uint4*>(lds_map)[i] = src[i];
    }
    __syncthreads();
    const unsigned char* a = lds_map + ((size_t)(y + 1) * 18 + x + 1) * c3_pad;
    int s64a = 0, s64b = 0, s32a = 0, s32b = 0, s16a = 0, s16b = 0;
    // 16 channels per step (the weights' rows are padded to c3_pad with zeros; the map's padded channels are "activation 0")
    auto dot16 = [](const uint4& v, const uint4& q, int acc) { return sdot4(v.w, q.w, sdot4(v.z, q.z, sdot4(v.y, q.y, sdot4(v.x, q.x, acc)))); };
#pragma unroll
    for (int j = 0; j < CP * 2; ++j) {
      const uint4 v = *reinterpret_cast<const uint4*>(a + 16 * j);
      s64a = dot16(v, wr[0][j], s64a); s64b = dot16(v, wr[1][j], s64b);
      s32a = dot16(v, wr[2][j], s32a); s32b = dot16(v, wr[3][j], s32b);
      s16a = dot16(v, wr[4][j], s16a); s16b = dot16(v, wr[5][j], s16b);
    }
    const int r16a = dpp_row_sum(s16a), r16b = dpp_row_sum(s16b);
    const int r32a = dpp_row_sum(s32a), r32b = dpp_row_sum(s32b);
    const int r64a = dpp_row_sum(s64a), r64b = dpp_row_sum(s64b);
    const int q32a = __builtin_amdgcn_readlane(r32a, 0) + __builtin_amdgcn_readlane(r32a, 16) + __builtin_amdgcn_readlane(r32a, 32) + __builtin_amdgcn_readlane(r32a, 48);
    const int q32b = __builtin_amdgcn_readlane(r32b, 0) + __builtin_amdgcn_readlane(r32b, 16) + __builtin_amdgcn_readlane(r32b, 32) + __builtin_amdgcn_readlane(r32b, 48);
    const int q64a = __builtin_amdgcn_readlane(r64a, 0) + __builtin_amdgcn_readlane(r64a, 16) + __builtin_amdgcn_readlane(r64a, 32) + __builtin_amdgcn_readlane(r64a, 48);
    const int q64b = __builtin_amdgcn_readlane(r64b, 0) + __builtin_amdgcn_readlane(r64b, 16) + __builtin_amdgcn_readlane(r64b, 32) + __builtin_amdgcn_readlane(r64b, 48);
    __syncthreads();   // the previous CTU's readers of logitL are done
    if (p == 0) *reinterpret_cast<int2*>(logitL + 2 * (5 + by * 4 + bx)) = make_int2(hb16a + r16a, hb16b + r16b);
    if (lane == 0) {
      *reinterpret_cast<int2*>(logitL + 2 * (1 + qy * 2 + qx)) = make_int2(hb32a + q32a, hb32b + q32b);
      *reinterpret_cast<int2*>(logitL + 44 + 2 * wave) = make_int2(q64a, q64b);
    }
    __syncthreads();
    const int g = first + k, f = g / per_frame, rem = g - f * per_frame;
    depth_map_of_ctu(F, logitL, nullptr, tid, lane, wave, f, F.row_begin + rem / F.ctus_x, rem % F.ctus_x, band_rows, hb64a, hb64b, margin_split, margin_stop,
                     d_depth, d_depth_max, d_logits, d_flags, nullptr, false);
  }
}

