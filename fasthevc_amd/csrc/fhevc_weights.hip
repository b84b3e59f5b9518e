// fhevc_weights.hip -- fhevc_set_weights: the FHW1 / FHW3 blobs of fasthevc_amd/weights.py turned into the device weight images of the depth kernels
// (k_cnn.hip and its .inc forms).  Host-side C++ only.
#include "fhevc_ctx.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace {

// FHW1 blob layout (fasthevc_amd/weights.py)
struct BlobView {
  const int32_t* shift;
  const int8_t* w1; const int32_t* b1;
  const int8_t* w2; const int32_t* b2;
  const int8_t* w3; const int32_t* b3;
  const int8_t* wh64; const int32_t* bh64;
  const int8_t* wh32; const int32_t* bh32;
  const int8_t* wh16; const int32_t* bh16;
  const int32_t* qp_bias;
};
constexpr size_t kBlobBytes = 8 + 12 + 144 + 64 + 4608 + 128 + 18432 + 256 + 8192 + 8 + 8192 + 8 + 2048 + 8 + 3 * 52 * 4;

bool parse_blob(const uint8_t* p, size_t n, BlobView& v, std::vector<uint8_t>& aligned)
{
  if (n != kBlobBytes || std::memcmp(p, "FHW1", 4) != 0) return false;
  uint32_t ver;
  std::memcpy(&ver, p + 4, 4);
  if (ver != 2) return false;
  // copy the int32 sections out to aligned storage: the blob packs int8 and int32 arrays back to back
  aligned.assign(p, p + n);
  size_t off = 8;
  auto take = [&](size_t bytes) { const uint8_t* q = aligned.data() + off; off += bytes; return q; };
  v.shift = reinterpret_cast<const int32_t*>(take(12));
  v.w1 = reinterpret_cast<const int8_t*>(take(144));   v.b1 = reinterpret_cast<const int32_t*>(take(64));
  v.w2 = reinterpret_cast<const int8_t*>(take(4608));  v.b2 = reinterpret_cast<const int32_t*>(take(128));
  v.w3 = reinterpret_cast<const int8_t*>(take(18432)); v.b3 = reinterpret_cast<const int32_t*>(take(256));
  v.wh64 = reinterpret_cast<const int8_t*>(take(8192)); v.bh64 = reinterpret_cast<const int32_t*>(take(8));
  v.wh32 = reinterpret_cast<const int8_t*>(take(8192)); v.bh32 = reinterpret_cast<const int32_t*>(take(8));
  v.wh16 = reinterpret_cast<const int8_t*>(take(2048)); v.bh16 = reinterpret_cast<const int32_t*>(take(8));
  v.qp_bias = reinterpret_cast<const int32_t*>(take(3 * 52 * 4));
  return off == n;
}

inline int32_t rd32(const void* p, int i)  // unaligned-safe read
{
  int32_t v;
  std::memcpy(&v, static_cast<const uint8_t*>(p) + 4 * (size_t)i, 4);
  return v;
}

// FHW3 blob layout (fasthevc_amd/weights.py: family_fields): a member of the reference's Bayesian-optimisation network family.  Pointers into the caller's
// blob; its int32 sections are not aligned (rd32)
struct FamilyView {
  int C[3], depth, convs;                                 // widths of the three blocks, convolutions per block, 3 * depth
  int32_t shift[9];                                       // [block][convolution]
  struct Conv { const int8_t* w; const void* b; int cout, cin; } conv[9];
  const int8_t* wh[3]; const void* bh[3]; int head_rows[3];   // the 64 / 32 / 16 heads: [2 classes][rows][C3]
  const void* qp_bias;
};

int parse_family(fhevc_ctx* c, const uint8_t* blob, size_t bytes, FamilyView& v)
{
  if (bytes < 24) return fail(c, FHEVC_E_WEIGHTS, "FHW3 blob too short");
  if (rd32(blob, 1) != 1) return fail(c, FHEVC_E_WEIGHTS, "unsupported FHW3 version");
  for (int b = 0; b < 3; ++b) if ((v.C[b] = rd32(blob, 2 + b)) < 1 || v.C[b] > 128) return fail(c, FHEVC_E_WEIGHTS, "family widths must be 1..128");
  v.depth = rd32(blob, 5);
  if (v.depth < 1 || v.depth > 3 || (v.C[2] & 3)) return fail(c, FHEVC_E_WEIGHTS, "family members: 1..3 convolutions per block, last width a multiple of 4");
  const size_t C3 = (size_t)v.C[2];
  size_t need = 24 + 36, ci = 1;
  for (int b = 0; b < 3; ++b) for (int j = 0; j < v.depth; ++j) { need += (size_t)v.C[b] * ci * 9 + 4 * (size_t)v.C[b]; ci = (size_t)v.C[b]; }
  need += (size_t)(2 * 64 + 2 * 64 + 2 * 16) * C3 + 24 + 3 * 52 * 4;
  if (bytes != need) return fail(c, FHEVC_E_WEIGHTS, "FHW3 blob has the wrong size");
  size_t off = 24;
  auto take = [&](size_t n) { const uint8_t* q = blob + off; off += n; return q; };
  std::memcpy(v.shift, take(36), 36);
  v.convs = 0;
  int cin = 1;
  for (int b = 0; b < 3; ++b)
    for (int j = 0; j < v.depth; ++j) {
      FamilyView::Conv& k = v.conv[v.convs++];
      k.cout = v.C[b]; k.cin = cin;
      k.w = reinterpret_cast<const int8_t*>(take((size_t)k.cout * cin * 9));
      k.b = take(4 * (size_t)k.cout);
      cin = k.cout;
    }
  for (int hd = 0; hd < 3; ++hd) {
    v.head_rows[hd] = hd < 2 ? 64 : 16;
    v.wh[hd] = reinterpret_cast<const int8_t*>(take(2 * (size_t)v.head_rows[hd] * C3));
    v.bh[hd] = take(8);
  }
  v.qp_bias = take(3 * 52 * 4);
  return FHEVC_OK;
}

// conv1's two bf16 fragments (jm = pre-pool column px) of the group g of 16 filters, [jm][64 lanes][8], weights scaled by 2^-shift: w * 2^-s is still exact in
// bf16 (a power-of-two scaling of an 8-bit integer).  Row m = r + 32*jm: channel = 16 g + m[1:0] + 4*m[3] + 8*m[2], pre-pool row py = m[4].  K slot k = 8h + j
// addresses the 4x4 input window: column wc = 2h + ((j >> 1) & 1), row wr = 2*(j >> 2) + (j & 1) (two row-pair dwords per column).  Tap (ky, kx) = (wr - py, wc - px).
void conv1_fragments(const int8_t* w1, int g, int shift, uint16_t* frag)
{
  for (int lane = 0; lane < 64; ++lane) {
    const int r = lane & 31, h = lane >> 5;
    for (int j = 0; j < 8; ++j)
      for (int jm = 0; jm < 2; ++jm) {
        const int ch = 16 * g + (r & 3) + 4 * ((r >> 3) & 1) + 8 * ((r >> 2) & 1), py = (r >> 4) & 1, px = jm;
        const int wc = 2 * h + ((j >> 1) & 1), wr = 2 * (j >> 2) + (j & 1);
        const int ky = wr - py, kx = wc - px;
        if (ky < 0 || ky > 2 || kx < 0 || kx > 2) continue;
        const float f = std::ldexp((float)w1[ch * 9 + ky * 3 + kx], -shift);
        uint32_t u;
        std::memcpy(&u, &f, 4);
        frag[((size_t)jm * 64 + lane) * 8 + j] = (uint16_t)(u >> 16);
      }
  }
}

// conv1 is fed the samples x, not x - 128: sum w (x - 128) + b = sum w x + (b - 128 sum w).  |b| <= 2^22 keeps |.| < 2^22 + 128 * 9 * 127 < 2^23: exact in
// fp32, and conv1's sums stay below 2^24
bool conv1_bias(const int8_t* w9, int32_t b, int32_t* out)
{
  int sw = 0;
  for (int t = 0; t < 9; ++t) sw += w9[t];
  *out = b - 128 * sw;
  return std::abs(b) <= 4194304;
}

// the bias of a filter whose input travels as a - 128: sum w a = sum w (a - 128) + 128 sum w (over ALL taps: the halo holds a - 128 = -128, "activation 0",
// and meets the same correction).  centred: the input IS centred samples, no correction.  bound (optional) collects the largest |accumulator| any input can
// produce over the filters it is handed: |b'| + 128 * sum |w| (|input| <= 128)
int32_t folded_bias(const int8_t* w, size_t n, int32_t b, long long* bound = nullptr, bool centred = false)
{
  int sw = 0, sa = 0;
  for (size_t i = 0; i < n; ++i) { sw += w[i]; sa += std::abs((int)w[i]); }
  const int32_t folded = b + (centred ? 0 : 128 * sw);
  if (bound) *bound = std::max(*bound, std::llabs((long long)folded) + 128LL * sa);
  return folded;
}

// FC heads on v_dot4_i32_i8: the last map is kept as a - 128 (signed bytes), so sum w a = sum w (a - 128) + 128 sum w and the second term moves into the
// head biases (the 64-level weights act on the 2x2 sum pool: four positions each).  bh64[2], bh32[2], bh16[2], then qp_bias[3][52]
using HeadBiases = std::array<int32_t, 6 + 3 * 52>;
HeadBiases head_biases(const int8_t* wh64, const int8_t* wh32, const int8_t* wh16, int C3, const void* bh64, const void* bh32, const void* bh16, const void* qp_bias)
{
  HeadBiases bhead = { rd32(bh64, 0), rd32(bh64, 1), rd32(bh32, 0), rd32(bh32, 1), rd32(bh16, 0), rd32(bh16, 1) };
  for (int cls = 0; cls < 2; ++cls) {
    int s64 = 0, s32 = 0, s16 = 0;
    for (int i = 0; i < 64 * C3; ++i) { s64 += wh64[(size_t)cls * 64 * C3 + i]; s32 += wh32[(size_t)cls * 64 * C3 + i]; }
    for (int i = 0; i < 16 * C3; ++i) s16 += wh16[(size_t)cls * 16 * C3 + i];
    bhead[0 + cls] += 128 * 4 * s64;
    bhead[2 + cls] += 128 * s32;
    bhead[4 + cls] += 128 * s16;
  }
  for (int i = 0; i < 3 * 52; ++i) bhead[6 + i] = rd32(qp_bias, i);
  return bhead;
}

// host array -> device buffer, allocated on first use
template <class T, class V> hipError_t upload(T*& d, const V& host)
{
  const size_t bytes = host.size() * sizeof(host[0]);
  if (!d) { const hipError_t e = hipMalloc(&d, bytes); if (e != hipSuccess) return e; }
  return hipMemcpy(d, host.data(), bytes, hipMemcpyHostToDevice);
}
template <class T> void release(T*& d) { (void)hipFree(d); d = nullptr; }

// Build the device weight image: MFMA A-operand fragments in lane order (k_cnn.hip header comment).
int build_weight_image(fhevc_ctx* c, const BlobView& b)
{
  int new_shift[3], new_mode[3] = { 0, 0, 0 };
  for (int l = 0; l < 3; ++l) {
    const int s = rd32(b.shift, l);
    if (s < 0 || s > 14) return fail(c, FHEVC_E_WEIGHTS, "shift out of range (0..14)");
    new_shift[l] = s;
  }
  std::vector<uint16_t> frag((size_t)FHEVC_FRAG_TOTAL * 8, 0);
  // all conv weights carry their layer's 2^-shift: w * 2^-s is still exact in bf16 (a power-of-two scaling of an 8-bit integer)
  // and every partial sum is a multiple of 2^-s below 2^24 * 2^-s, so the fp32 accumulation stays exact and the MFMA
  // delivers (acc + b) * 2^-s directly: one multiply per output less in the epilogue
  // conv1 takes bf16 operands (its input tile is bf16), conv2 and conv3 f16 ones (their inputs are written as f16 by the
  // epilogues before them): |w| * 2^-s >= 2^-14 is a normal f16 number and 7 significant bits fit its 11
  auto put_f16 = [&](int layer, int frag_idx, int lane, int j, int v) {
    const _Float16 h = (_Float16)std::ldexp((float)v, -new_shift[layer]);
    std::memcpy(&frag[((size_t)frag_idx + lane) * 8 + j], &h, 2);
  };
  conv1_fragments(b.w1, 0, new_shift[0], &frag[(size_t)FHEVC_FRAG_CONV1 * 8]);
  for (int lane = 0; lane < 64; ++lane) {
    const int r = lane & 31, h = lane >> 5;
    for (int j = 0; j < 8; ++j)   // conv2: K-step s = tap, k = 8h + j = input channel
      for (int s = 0; s < 9; ++s) put_f16(1, FHEVC_FRAG_CONV2 + s * 64, lane, j, b.w2[((r * 16 + 8 * h + j) * 9) + s]);
  }
  // conv3 runs on v_mfma_f32_16x16x32_bf16: lane (m = lane & 15, kg = lane >> 4) holds A[m][8 kg + j]; tile t = the wave's 32
  // output channels, fragment s = 9 mt + tap: M tile mt (16 channels), K = the tap's 32 input channels
  for (int lane = 0; lane < 64; ++lane) {
    const int m = lane & 15, kg = lane >> 4;
    for (int j = 0; j < 8; ++j)
      for (int t = 0; t < 2; ++t)
        for (int s = 0; s < 18; ++s) {
#if FHEVC_F16_CONV3_32
          // v_mfma_f32_32x32x16_f16: lane (row = lane & 31, h = lane >> 5) holds A[row][8 h + j]; fragment s = 2 tap + c2: K = the tap's
          // channels 16 c2 .. 16 c2 + 15, rows = the tile's 32 output channels
          (void)m; (void)kg;
          const int oc = 32 * t + (lane & 31), ic = 16 * (s & 1) + 8 * (lane >> 5) + j, tap = s >> 1;
#else
          const int oc = 32 * t + 16 * (s / 9) + m, ic = 8 * kg + j, tap = s % 9;
#endif
          put_f16(2, FHEVC_FRAG_CONV3 + (t * 18 + s) * 64, lane, j, b.w3[(oc * 32 + ic) * 9 + tap]);
        }
  }
  // the source Hadamard's constant A operands (k_cnn.hip, HAD == 2; v_mfma_f32_32x32x16_bf16): row m of M tile mt = coefficient
  // c = 32 mt + m = (u = c >> 3, v = c & 7) of the 2-D Walsh-Hadamard transform of an 8x8 block, K slot 8 h + j of step st = the sample
  // at column 4 h + (j >> 1), row 2 st - 1 + (j & 1) of the block (the staged tile keeps picture rows 2P - 1 and 2P in one dword):
  // +-1 by the parity of popcount(u & row) + popcount(v & column); rows -1 and 8 belong to the neighbouring blocks and the DC
  // coefficient is not part of the sum (TEncCu.cpp:1319): zero
  for (int mt = 0; mt < 2; ++mt)
    for (int st = 0; st < 5; ++st)
      for (int lane = 0; lane < 64; ++lane) {
        const int c = 32 * mt + (lane & 31), u = c >> 3, v = c & 7, h = lane >> 5;
        for (int j = 0; j < 8; ++j) {
          const int col = 4 * h + (j >> 1), row = 2 * st - 1 + (j & 1);
          uint16_t bits = 0;
          if (c != 0 && row >= 0 && row <= 7) bits = ((__builtin_popcount(u & row) + __builtin_popcount(v & col)) & 1) ? 0xBF80 : 0x3F80;
          frag[((size_t)FHEVC_FRAG_HAD + (mt * 5 + st) * 64 + lane) * 8 + j] = bits;
        }
      }
  // the i8 variant (v_mfma_i32_32x32x32_i8: a lane holds 16 signed bytes of K; lanes 0-31 K 0-15, lanes 32-63 K 16-31):
  //   conv2 fragments (k_cnn.hip, conv2_half_i8): row = output channel lane & 31, K byte j of lane half h = input channel j at tap
  //                           0-2: (ky = h, kx = 0..2); 3: (2, kx = 2 h); 4: (2, 1) for h = 0, zero for h = 1; 5: zero | (2, 1);
  //   conv3 fragment (tile, tap): row = output channel 32 tile + (lane & 31), K byte j of lane half h = input channel 16 h + j
  std::vector<int8_t> frag8((size_t)FHEVC_FRAGI8_TOTAL * 16, 0);
  for (int lane = 0; lane < 64; ++lane) {
    const int r = lane & 31, h = lane >> 5;
    for (int j = 0; j < 16; ++j) {
      auto w2 = [&](int ky, int kx) { return b.w2[(r * 16 + j) * 9 + ky * 3 + kx]; };
      int8_t* f2 = &frag8[((size_t)FHEVC_FRAGI8_CONV2 + lane) * 16 + j];   // fragment s at f2[s * 64 * 16]
      for (int kx = 0; kx < 3; ++kx) f2[(size_t)kx * 1024] = w2(h, kx);
      f2[3 * 1024] = w2(2, 2 * h);              // [(2, 0) | (2, 2)]
      f2[4 * 1024] = h == 0 ? w2(2, 1) : 0;     // [(2, 1) | 0]
      f2[5 * 1024] = h == 1 ? w2(2, 1) : 0;     // [0 | (2, 1)]
      for (int t = 0; t < 2; ++t)
        for (int tap = 0; tap < 9; ++tap)
          frag8[((size_t)FHEVC_FRAGI8_CONV3 + (t * 9 + tap) * 64 + lane) * 16 + j] = b.w3[((32 * t + r) * 32 + 16 * h + j) * 9 + tap];
    }
  }
  // its biases (laid out like the f16 form's: entries 16.. are used) and the largest |accumulator| per layer
  std::vector<int32_t> bias8(112, 0);
  long long bound[3] = { 0, 0, 0 };
  for (int oc = 0; oc < 32; ++oc) bias8[16 + oc] = folded_bias(b.w2 + oc * 144, 144, rd32(b.b2, oc), &bound[1]);
  for (int oc = 0; oc < 64; ++oc) bias8[48 + oc] = folded_bias(b.w3 + oc * 288, 288, rd32(b.b3, oc), &bound[2]);
  // the requant's form per layer (k_cnn.hip: requant4_i8); FHEVC_CNN_REQUANT=general keeps the general one (A/B, tests)
  for (int l = 1; l < 3; ++l)
    new_mode[l] = c->knobs.requant_general ? 0 : (new_shift[l] == 8 && bound[l] < (1LL << 23)) ? 2 : (new_shift[l] <= 7 ? 1 : 0);
  // the high-byte forms (k_cnn.hip: requant4_i8_hi; mode 3): conv2 at shift 7 (one saturating doubling), conv3 at shift 8, their biases with - (128 << shift) folded
  // in -- valid while the folded accumulator cannot wrap int32.  The depth kernel has ONE instantiation for them, so both layers take mode 3 or neither does;
  // FHEVC_CNN_REQUANT=short and the TRIO form (built on the short forms) keep modes 1 / 2 and their biases
  auto high_byte_ok = [&](int l, int want_shift) { return new_shift[l] == want_shift && bound[l] + (128LL << new_shift[l]) < (1LL << 31); };
  if (!c->knobs.requant_general && !c->knobs.requant_short && !c->knobs.trio && high_byte_ok(1, 7) && high_byte_ok(2, 8)) {
    new_mode[1] = new_mode[2] = 3;
    for (int oc = 0; oc < 32; ++oc) bias8[16 + oc] -= 128 << new_shift[1];
    for (int oc = 0; oc < 64; ++oc) bias8[48 + oc] -= 128 << new_shift[2];
  }
  std::vector<float> bias(112);
  for (int i = 0; i < 16; ++i) {
    int32_t b1;
    if (!conv1_bias(b.w1 + i * 9, rd32(b.b1, i), &b1)) return fail(c, FHEVC_E_WEIGHTS, "|bias| > 2^22");
    bias[i] = (float)b1;
  }
  for (int i = 0; i < 32; ++i) bias[16 + i] = (float)rd32(b.b2, i);
  for (int i = 0; i < 64; ++i) bias[48 + i] = (float)rd32(b.b3, i);
  for (int i = 16; i < 112; ++i) if (std::fabs(bias[i]) > 4194304.0f) return fail(c, FHEVC_E_WEIGHTS, "|bias| > 2^22");
  std::vector<uint8_t> whead(4 * 4096 + 2 * 1024);
  std::memcpy(whead.data(), b.wh64, 8192);
  std::memcpy(whead.data() + 8192, b.wh32, 8192);
  std::memcpy(whead.data() + 16384, b.wh16, 2048);
  const HeadBiases bhead = head_biases(b.wh64, b.wh32, b.wh16, 64, b.bh64, b.bh32, b.bh16, b.qp_bias);

  // everything above validated the blob without touching the context.  From here the base image is overwritten in place: if it is the one in
  // use, a HIP failure below leaves the context WITHOUT weights (predict then fails with FHEVC_E_STATE) rather than with a torn image; if a family
  // member is in use it stays in use until the last copy has succeeded
  if (c->have_weights && !c->family) c->have_weights = false;
  HIP_TRY(c, upload(c->d_frag_i8, frag8));
  HIP_TRY(c, upload(c->d_bias_i8, bias8));
  HIP_TRY(c, upload(c->d_frag, frag));
  HIP_TRY(c, upload(c->d_bias, bias));
  HIP_TRY(c, upload(c->d_whead, whead));
  HIP_TRY(c, upload(c->d_bhead, bhead));
  for (int l = 0; l < 3; ++l) { c->shift[l] = new_shift[l]; c->scale[l] = std::ldexp(1.0f, -new_shift[l]); c->requant_mode[l] = new_mode[l]; }
  c->family = false; c->fam_layers = false;   // the dispatch flips only now, with the image complete
  c->have_weights = true;
  return FHEVC_OK;
}

// FHW3 member without a fused kernel: one image per convolution for k_cnn_layers.inc + the activation tensors of a chunk of CTUs in HBM
int build_layers_image(fhevc_ctx* c, const FamilyView& v)
{
  const int C3 = v.C[2], depth = v.depth;
  // validate the whole blob before the image in use is touched: a rejected blob leaves the context exactly as it was
  for (int li = 0; li < v.convs; ++li) {
    const FamilyView::Conv& k = v.conv[li];
    for (size_t i = 0; i < (size_t)k.cout * k.cin * 9; ++i) if (k.w[i] == -128) return fail(c, FHEVC_E_WEIGHTS, "weight -128 not allowed");
    const int sh = v.shift[(li / depth) * 3 + li % depth];
    if (sh < 0 || sh > 14) return fail(c, FHEVC_E_WEIGHTS, "shift out of range (0..14)");
  }
  for (int hd = 0; hd < 3; ++hd)
    for (size_t i = 0; i < 2 * (size_t)v.head_rows[hd] * C3; ++i) if (v.wh[hd][i] == -128) return fail(c, FHEVC_E_WEIGHTS, "weight -128 not allowed");
  for (void* q : c->lw_bufs) (void)hipFree(q);
  c->lw_bufs.clear();
  if (c->family && c->fam_layers) c->have_weights = false;   // the layered image in use is gone: a HIP failure below leaves NO weights (never a torn image)
  FhevcLayersWeights lw = {};
  // a chunk of CTUs whose activations live in HBM at once: up to 16 pictures of 1080p (3.2 GB for 23/46/92 x 2), at least one picture row
  lw.chunk = std::min(c->num_ctus * std::max(1, c->cfg.max_frames), 8192);
  if (lw.chunk < 64) lw.chunk = 64;
  auto dev = [&](size_t n, int fill) -> void* { void* q = nullptr; if (hipMalloc(&q, n) != hipSuccess) return nullptr; c->lw_bufs.push_back(q); (void)hipMemset(q, fill, n); return q; };
  // a host array in a buffer of its own (null: the allocation or the copy failed)
  auto dev_copy = [&](const void* host, size_t n) -> void* { void* q = dev(n, 0); return q && hipMemcpy(q, host, n, hipMemcpyHostToDevice) == hipSuccess ? q : nullptr; };
  // two convolutions per block at padded widths 32 / 64 / 96 (the reference's 23 / 46 / 92 x 2): k_cnn_d2.inc keeps a CTU's activations in LDS -- the same weight
  // images, no activation tensors in HBM (FHEVC_FUSED_D2=0 / FHEVC_FAMILY_LAYERS keep the layer-by-layer path: tests, A/B)
  auto pad32 = [](int x) { return 32 * ((x + 31) / 32); };
  const bool d2 = depth == 2 && pad32(v.C[0]) == 32 && pad32(v.C[1]) == 64 && pad32(C3) == 96 && c->knobs.fused_d2 && !c->knobs.family_layers;
  if (!d2 && !(lw.in0 = static_cast<int8_t*>(dev((size_t)lw.chunk * 66 * 66, 0)))) return fail(c, FHEVC_E_HIP, "layer buffers");
  int H = 64;
  for (int li = 0; li < v.convs; ++li) {
    const FamilyView::Conv& k = v.conv[li];
    const int b = li / depth, j = li % depth, co = k.cout, cin = k.cin, first = li == 0;
    const int kc = first ? 0 : (cin + 31) / 32, cout_pad = pad32(co), MT = cout_pad / 32, NF = first ? 1 : kc * 9;
    // A fragments: lane (m, h) of (M tile, fragment): row m carries channel 32 mt + 16 m[2] + 4 m[4:3] + m[1:0] (so that a lane's 16 accumulators are 16
    // consecutive channels); byte jj of lane half h = input channel 32 kc + 16 h + jj at the fragment's tap (first layer: tap jj of the one channel, h = 0)
    std::vector<int8_t> frag((size_t)MT * NF * 64 * 16, 0);
    for (int mt = 0; mt < MT; ++mt)
      for (int f = 0; f < NF; ++f)
        for (int lane = 0; lane < 64; ++lane) {
          const int m = lane & 31, h = lane >> 5;
          const int oc = 32 * mt + 16 * ((m >> 2) & 1) + 4 * (m >> 3) + (m & 3);
          if (oc >= co) continue;
          for (int jj = 0; jj < 16; ++jj) {
            int8_t w = 0;
            if (first) { if (h == 0 && jj < 9) w = k.w[(size_t)oc * 9 + jj]; }
            else { const int ic = 32 * (f / 9) + 16 * h + jj; if (ic < cin) w = k.w[((size_t)oc * cin + ic) * 9 + f % 9]; }
            frag[(((size_t)mt * NF + f) * 64 + lane) * 16 + jj] = w;
          }
        }
    std::vector<int32_t> bias((size_t)cout_pad, 0);
    long long bound = 0;
    for (int oc = 0; oc < co; ++oc) bias[(size_t)oc] = folded_bias(k.w + (size_t)oc * cin * 9, (size_t)cin * 9, rd32(k.b, oc), &bound, first);
    const int pool = (j == depth - 1) && b < 2, Ho = pool ? H / 2 : H;
    FhevcLayer& L = lw.l[li];
    void* dfrag = dev_copy(frag.data(), frag.size()); void* dbias = dev_copy(bias.data(), bias.size() * 4);
    // the tensor's row pitch carries the padding its consumer's LDS image wants (the last map goes to the heads kernel: none)
    const int ni = li + 1, nb = ni / depth, nj = ni % depth;
    int in_pad = 0, swz = 0, out_pad = 0, unused = 0;
    if (!first) fhevc_layer_lds_image(kc, pool, H, &in_pad, &swz);
    if (ni < v.convs) fhevc_layer_lds_image(cout_pad / 32, (nj == depth - 1) && nb < 2, Ho, &out_pad, &unused);
    L.in_pad = in_pad; L.out_pad = out_pad; L.swz = swz;
    L.out = d2 ? nullptr : static_cast<int8_t*>(dev((size_t)lw.chunk * (Ho + 2) * ((size_t)(Ho + 2) * cout_pad + out_pad), 0x80));   // halo = "activation 0", written here once
    if (!dfrag || !dbias || (!d2 && !L.out)) return fail(c, FHEVC_E_HIP, "layer buffers");
    L.frag = static_cast<const uint4*>(dfrag); L.bias = static_cast<const int32_t*>(dbias);
    const int sh = v.shift[b * 3 + j];
    L.shift = sh; L.kc = kc; L.cout_pad = cout_pad; L.H = H; L.pool = pool;
    // requant4_i8's short forms: 1 packs to i16 with saturation BEFORE the shift (exact for shifts up to 7: a saturated value still clamps to 255 / 0 behind
    // it); 2 takes bytes 1-2 of the accumulator (shift 8, exact while the accumulator fits 24 bits)
    L.rq = sh <= 7 ? 1 : (sh == 8 && bound < (1LL << 23)) ? 2 : 0;
    H = Ho;
  }
  lw.num_layers = v.convs; lw.c3 = C3; lw.c3_pad = pad32(C3);
  // rows of c3_pad bytes (zeros behind the C3 weights): the heads kernel reads activations and weights 16 bytes at a time
  const size_t cp = lw.c3_pad;
  std::vector<uint8_t> whead((size_t)(2 * 64 + 2 * 64 + 2 * 16) * cp, 0);
  for (int hd = 0, row = 0; hd < 3; ++hd)
    for (int r = 0; r < 2 * v.head_rows[hd]; ++r, ++row) std::memcpy(whead.data() + (size_t)row * cp, v.wh[hd] + (size_t)r * C3, (size_t)C3);
  const HeadBiases bhead = head_biases(v.wh[0], v.wh[1], v.wh[2], C3, v.bh[0], v.bh[1], v.bh[2], v.qp_bias);
  lw.whead = static_cast<const uint8_t*>(dev_copy(whead.data(), whead.size()));
  lw.bhead = static_cast<const int32_t*>(dev_copy(bhead.data(), sizeof bhead));
  if (!lw.whead || !lw.bhead) return fail(c, FHEVC_E_HIP, "layer buffers");
  if (d2 && !fhevc_cnn_d2_supported(lw)) return fail(c, FHEVC_E_STATE, "layer images do not match the fused two-convolution kernel");
  lw.d2_short = d2 && !c->knobs.d2_requant_general && lw.l[0].rq == 1;
  for (int i = 1; i < 6 && lw.d2_short; ++i) lw.d2_short = lw.l[i].rq == 2;
  c->lw = lw;
  for (int b = 0; b < 3; ++b) c->fam_c[b] = v.C[b];
  c->family = true; c->fam_layers = true; c->fam_d2 = d2; c->have_weights = true;
  return FHEVC_OK;
}

// FHW3: the kernel of k_cnn_family.inc runs the members with one convolution per block whose widths it is instantiated for (fhevc_cnn_family_supported);
// every other member goes layer by layer
int build_family_image(fhevc_ctx* c, const uint8_t* blob, size_t bytes)
{
  FamilyView v;
  const int rc = parse_family(c, blob, bytes, v);
  if (rc != FHEVC_OK) return rc;
  const int C1 = v.C[0], C2 = v.C[1], C3 = v.C[2];
  if (v.depth != 1 || !fhevc_cnn_family_supported(C1, C2, C3) || c->knobs.family_layers)   // (the knob: the generic path for a fused member too)
    return build_layers_image(c, v);
  const int sh[3] = { v.shift[0], v.shift[3], v.shift[6] };
  for (int l = 0; l < 3; ++l) if (sh[l] < 0 || sh[l] > 14) return fail(c, FHEVC_E_WEIGHTS, "shift out of range (0..14)");
  const int8_t* w1 = v.conv[0].w; const int8_t* w2 = v.conv[1].w; const int8_t* w3 = v.conv[2].w;
  const int G1 = C1 / 16, K1 = (C1 + 31) / 32, M2 = C2 / 32, K2 = C2 / 32, M3 = C3 / 32;
  // conv1: per group of 16 filters the two fragments of the base network (rows = filter x 2x2 pre-pool position, K = 4x4 window)
  for (int i = 0; i < C1 * 9; ++i) if (w1[i] == -128) return fail(c, FHEVC_E_WEIGHTS, "weight -128 not allowed");
  std::vector<uint16_t> frag1((size_t)G1 * 2 * 64 * 8, 0);
  std::vector<float> bias1((size_t)C1);
  for (int g = 0; g < G1; ++g) conv1_fragments(w1, g, sh[0], &frag1[(size_t)g * 2 * 64 * 8]);
  for (int i = 0; i < C1; ++i) {
    int32_t b1;
    if (!conv1_bias(w1 + i * 9, rd32(v.conv[0].b, i), &b1)) return fail(c, FHEVC_E_WEIGHTS, "|bias| > 2^22");
    bias1[(size_t)i] = std::ldexp((float)b1, -sh[0]);
  }
  // conv2 / conv3: fragment (M tile, K chunk, tap): row = output channel 32 mt + (lane & 31), byte j of lane half h = input channel 32 k + 16 h + j
  auto build = [&](const int8_t* w, int CI, int M, int K, std::vector<int8_t>& frag) {
    frag.assign((size_t)M * K * 9 * 64 * 16, 0);
    for (int mt = 0; mt < M; ++mt)
      for (int k = 0; k < K; ++k)
        for (int tap = 0; tap < 9; ++tap)
          for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 16; ++j) {
              const int oc = 32 * mt + (lane & 31), ic = 32 * k + 16 * (lane >> 5) + j;
              if (ic < CI) frag[((((size_t)mt * K + k) * 9 + tap) * 64 + lane) * 16 + j] = w[((size_t)oc * CI + ic) * 9 + tap];
            }
  };
  std::vector<int8_t> frag2, frag3;
  build(w2, C1, M2, K1, frag2);
  build(w3, C2, M3, K2, frag3);
  std::vector<int32_t> bias8((size_t)C2 + C3);
  for (int oc = 0; oc < C2; ++oc) bias8[(size_t)oc] = folded_bias(w2 + (size_t)oc * C1 * 9, (size_t)C1 * 9, rd32(v.conv[1].b, oc));
  for (int oc = 0; oc < C3; ++oc) bias8[(size_t)C2 + oc] = folded_bias(w3 + (size_t)oc * C2 * 9, (size_t)C2 * 9, rd32(v.conv[2].b, oc));
  const int8_t* wh64 = v.wh[0]; const int8_t* wh32 = v.wh[1]; const int8_t* wh16 = v.wh[2];
  std::vector<uint8_t> whead((size_t)(2 * 64 + 2 * 64 + 2 * 16) * C3);
  std::memcpy(whead.data(), wh64, (size_t)2 * 64 * C3);
  std::memcpy(whead.data() + (size_t)2 * 64 * C3, wh32, (size_t)2 * 64 * C3);
  std::memcpy(whead.data() + (size_t)4 * 64 * C3, wh16, (size_t)2 * 16 * C3);
  // the MFMA image of the two smaller heads: [position j = (py, px) of a 16x16 block][chunk of 64 channels][column][64 B]
  const int KC = C3 / 64;
  std::vector<uint8_t> headm((size_t)16 * KC * 16 * 64, 0);
  for (int j = 0; j < 16; ++j)
    for (int kc = 0; kc < KC; ++kc)
      for (int n = 0; n < 10; ++n) {
        const int8_t* src;
        if (n < 2) src = wh16 + ((size_t)n * 16 + j) * C3 + 64 * kc;
        else {
          const int sub = (n - 2) >> 1, cls = n & 1, py = j >> 2, px = j & 3;
          src = wh32 + ((size_t)cls * 64 + ((sub >> 1) * 4 + py) * 8 + (sub & 1) * 4 + px) * C3 + 64 * kc;
        }
        std::memcpy(headm.data() + (((size_t)j * KC + kc) * 16 + n) * 64, src, 64);
      }
  const HeadBiases bhead = head_biases(wh64, wh32, wh16, C3, v.bh[0], v.bh[1], v.bh[2], v.qp_bias);
  // validated; the fused member's image is replaced now: if it is the one in use, a HIP failure below leaves NO weights
  if (c->family && !c->fam_layers) c->have_weights = false;
  release(c->f_frag1); release(c->f_bias1); release(c->f_frag2); release(c->f_frag3);
  release(c->f_bias_i8); release(c->f_whead); release(c->f_headm); release(c->f_bhead);
  HIP_TRY(c, upload(c->f_frag1, frag1));
  HIP_TRY(c, upload(c->f_bias1, bias1));
  HIP_TRY(c, upload(c->f_frag2, frag2));
  HIP_TRY(c, upload(c->f_frag3, frag3));
  HIP_TRY(c, upload(c->f_bias_i8, bias8));
  HIP_TRY(c, upload(c->f_whead, whead));
  HIP_TRY(c, upload(c->f_headm, headm));
  HIP_TRY(c, upload(c->f_bhead, bhead));
  c->fam_c[0] = C1; c->fam_c[1] = C2; c->fam_c[2] = C3;
  c->shift[0] = sh[0]; c->shift[1] = sh[1]; c->shift[2] = sh[2];
  c->family = true; c->fam_layers = false;
  c->have_weights = true;
  return FHEVC_OK;
}

}  // namespace

FhevcFamilyWeights family_weights(const fhevc_ctx* c)
{
  FhevcFamilyWeights w;
  w.c[0] = c->fam_c[0]; w.c[1] = c->fam_c[1]; w.c[2] = c->fam_c[2];
  w.frag1 = c->f_frag1; w.bias1 = c->f_bias1; w.frag2 = c->f_frag2; w.frag3 = c->f_frag3; w.bias_i8 = c->f_bias_i8; w.whead = c->f_whead; w.headm = c->f_headm; w.bhead = c->f_bhead;
  w.shift[0] = c->shift[0]; w.shift[1] = c->shift[1]; w.shift[2] = c->shift[2];
  return w;
}

FhevcCnnWeights cnn_weights(const fhevc_ctx* c)
{
  FhevcCnnWeights w;
  w.frag = c->d_frag; w.bias = c->d_bias; w.whead = c->d_whead; w.bhead = c->d_bhead;
  w.scale[0] = c->scale[0]; w.scale[1] = c->scale[1]; w.scale[2] = c->scale[2];
  w.frag_i8 = c->d_frag_i8; w.bias_i8 = c->d_bias_i8;
  w.shift[0] = c->shift[0]; w.shift[1] = c->shift[1]; w.shift[2] = c->shift[2];
  w.requant_mode[0] = 0; w.requant_mode[1] = c->requant_mode[1]; w.requant_mode[2] = c->requant_mode[2];
  w.i8 = c->cnn_i8 ? 1 : 0;
  w.had_valu = c->had_valu ? 1 : 0;
  return w;
}

extern "C" int fhevc_set_weights(fhevc_ctx* c, const void* blob, size_t bytes)
{
  if (!c || !blob) return FHEVC_E_INVALID;
  // The primary validates and builds first (a rejected blob changes nothing anywhere); only then do the peers get the blob.  A peer that fails after
  // the primary succeeded would leave devices with different weights: the whole context then reports "weights not set" until a blob is accepted by all
  auto push_to_peers = [&]() {
    for (fhevc_ctx* peer : c->peers) {
      const int rc = fhevc_set_weights(peer, blob, bytes);
      if (rc != FHEVC_OK) {
        c->have_weights = false;
        for (fhevc_ctx* p2 : c->peers) p2->have_weights = false;
        return fail(c, rc, "weights rejected by a peer device");
      }
    }
    (void)hipSetDevice(c->device);
    return (int)FHEVC_OK;
  };
  (void)hipSetDevice(c->device);
  // The images below are overwritten in place or freed.  Launches issued earlier, on ANY stream (a caller's non-blocking stream is not
  // ordered with the synchronous copies), still read them: wait for the device first, so that they see the old weights to the end
  HIP_TRY(c, hipDeviceSynchronize());
  if (bytes >= 4 && std::memcmp(blob, "FHW3", 4) == 0) {  // a member of the reference's Bayesian-optimisation network family
    const int rc = build_family_image(c, static_cast<const uint8_t*>(blob), bytes);
    return rc != FHEVC_OK ? rc : push_to_peers();
  }
  BlobView v;
  std::vector<uint8_t> copy;
  if (!parse_blob(static_cast<const uint8_t*>(blob), bytes, v, copy)) return fail(c, FHEVC_E_WEIGHTS, "not an FHW1 blob");
  const struct { const int8_t* p; size_t n; } i8s[6] = { { v.w1, 144 }, { v.w2, 4608 }, { v.w3, 18432 }, { v.wh64, 8192 }, { v.wh32, 8192 }, { v.wh16, 2048 } };
  for (const auto& a : i8s)
    for (size_t i = 0; i < a.n; ++i) if (a.p[i] == -128) return fail(c, FHEVC_E_WEIGHTS, "weight -128 not allowed");
  const int rc = build_weight_image(c, v);
  return rc != FHEVC_OK ? rc : push_to_peers();
}
