// motion_amvp_host_check.cpp -- the host twin of the re-pricing against neighbour predictors (fhevc_motion_amvp_picture, fasthevc_amd/csrc/fhevc_host.hip) run
// from a stand-alone program, so that the CPU sanitizers see it without Python in the process.  CPU only: never built into the library, never run on a
// GPU machine.  Build and run (no device code is linked or called):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/motion_amvp_host_check.cpp fasthevc_amd/csrc/fhevc_host.hip -o build/motion_amvp_host_check -fsanitize=address,undefined && build/motion_amvp_host_check
//
// Every input and output is a heap block of exactly its size, so a read or a write one byte outside is reported; records are also handed over 4 bytes
// off their natural alignment (any 4-byte alignment is allowed).  Vectors come from a small pool that holds the int16 extremes, so differences reach 33
// bits per component and sums saturate.  Prints one line and returns 0 when every call returned what it must.
#include "../include/fasthevc.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>

namespace {

std::mt19937 rng(2578);

// n records in a heap block of exactly n * sizeof(T) (+ shift) bytes, starting `shift` bytes into it
template <class T> struct Block {
  std::unique_ptr<unsigned char[]> raw;
  T* p;
  Block(size_t n, int shift, bool random) : raw(new unsigned char[n * sizeof(T) + shift]), p(reinterpret_cast<T*>(raw.get() + shift))
  {
    for (size_t i = 0; i < n * sizeof(T); ++i) raw[shift + i] = random ? (unsigned char)rng() : 0xA5;
  }
};

void fill(fhevc_motion_qpel_node* r, size_t n)
{
  static const int16_t pool[8][2] = { { 0, 0 }, { 2, 2 }, { 4, 4 }, { -5, 2 }, { 3, 3 }, { 32767, -32768 }, { -32768, 32767 }, { 32767, 32767 } };
  for (size_t i = 0; i < n; ++i) {
    const int16_t* v = pool[rng() % 8];
    r[i].mvx = v[0]; r[i].mvy = v[1];
    r[i].cost_best = rng() % 10 == 0 ? 0xFFFFFFFFu : rng() % 100000;
    r[i].satd_best = rng() % 10 == 0 ? 0xFFFFFFF0u + rng() % 15 : rng() % 50000;
  }
}

}  // namespace

int main()
{
  static_assert(sizeof(fhevc_motion_qpel_node) == 16 && sizeof(fhevc_motion_mvp) == 8, "records");
  const int sizes[][2] = { { 168, 152 }, { 200, 136 }, { 64, 64 }, { 8, 8 }, { 72, 200 } };
  long calls = 0, priced = 0, saturated = 0, wide = 0;
  for (int it = 0; it < 600; ++it) {
    const int W = sizes[it % 5][0], H = sizes[it % 5][1], cw = (W + 63) / 64, ch = (H + 63) / 64;
    const int rb = (int)(rng() % (unsigned)ch), re = rb + 1 + (int)(rng() % (unsigned)(ch - rb));
    const size_t n = (size_t)(re - rb) * cw;
    const int shift = (it & 1) ? 4 : 0, qp = (int)(rng() % 52), bd = 8 + (int)(rng() % 5);
    Block<fhevc_motion_qpel_node> nodes(n * 85, shift, true), pus(n * 124, shift, true), small(n * 384, shift, true);
    fill(nodes.p, n * 85); fill(pus.p, n * 124); fill(small.p, n * 384);
    const unsigned want = 1 + rng() % 63;   // which of the six outputs
    Block<fhevc_motion_qpel_node> o0(n * 85, shift, false), o1(n * 124, shift, false), o2(n * 384, shift, false);
    Block<fhevc_motion_mvp> m0(n * 85, shift, false), m1(n * 124, shift, false), m2(n * 384, shift, false);
    const bool need1 = want & (2 | 16), need2 = want & (4 | 32);
    if (fhevc_motion_amvp_picture(W, H, bd, rb, re, qp, nodes.p, need1 || (it & 2) ? pus.p : nullptr, need2 || (it & 4) ? small.p : nullptr, (want & 1) ? o0.p : nullptr,
                                  (want & 2) ? o1.p : nullptr, (want & 4) ? o2.p : nullptr, (want & 8) ? m0.p : nullptr, (want & 16) ? m1.p : nullptr,
                                  (want & 32) ? m2.p : nullptr) != FHEVC_OK)
      return 1;
    ++calls;
    // what must hold for any input: vectors and distortions copied, a price only where the input has one, a predictor record that matches the price
    if ((want & 5) == 5 && (want & 32))
      for (size_t i = 0; i < n * 384; ++i) {
        const fhevc_motion_qpel_node &a = small.p[i], &b = o2.p[i];
        const fhevc_motion_mvp& m = m2.p[i];
        if (b.cost_best == 0xFFFFFFFFu) {
          if (m.idx != 255 || m.src != 255 || m.px || m.py || m.bits || m.num_spatial) return 2;
          continue;
        }
        if (a.cost_best == 0xFFFFFFFFu || b.mvx != a.mvx || b.mvy != a.mvy || b.satd_best != a.satd_best || b.satd_int != a.satd_int) return 3;
        if (m.idx > 1 || m.num_spatial > 2 || m.src > 5 || m.bits < 2 || m.bits > 66 || b.cost_best < a.satd_best) return 4;
        ++priced; saturated += b.cost_best == 0xFFFFFFFEu; wide += m.bits >= 62;
      }
    // rejected calls write nothing and read nothing they should not
    if (fhevc_motion_amvp_picture(W, H, bd, rb, re, qp, nullptr, pus.p, small.p, o0.p, o1.p, o2.p, m0.p, m1.p, m2.p) != FHEVC_E_INVALID) return 5;
    if (fhevc_motion_amvp_picture(W, H, bd, rb, re, qp, nodes.p, nullptr, small.p, o0.p, o1.p, o2.p, m0.p, m1.p, m2.p) != FHEVC_E_INVALID) return 6;
    if (fhevc_motion_amvp_picture(W, H, bd, rb, re, qp, nodes.p, pus.p, small.p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != FHEVC_E_INVALID) return 7;
    if (fhevc_motion_amvp_picture(W, H, bd, rb, ch + 1, qp, nodes.p, pus.p, small.p, o0.p, o1.p, o2.p, m0.p, m1.p, m2.p) != FHEVC_E_INVALID) return 8;
    if (fhevc_motion_amvp_picture(W, H, bd, rb, re, 52, nodes.p, pus.p, small.p, o0.p, o1.p, o2.p, m0.p, m1.p, m2.p) != FHEVC_E_INVALID) return 9;
    if (fhevc_motion_amvp_picture(7, H, bd, rb, re, qp, nodes.p, pus.p, small.p, o0.p, o1.p, o2.p, m0.p, m1.p, m2.p) != FHEVC_E_INVALID) return 10;
    // an empty band is accepted and touches nothing: blocks of zero records
    Block<fhevc_motion_qpel_node> none(0, shift, false);
    if (fhevc_motion_amvp_picture(W, H, bd, rb, rb, qp, none.p, nullptr, nullptr, none.p, nullptr, nullptr, nullptr, nullptr, nullptr) != FHEVC_OK) return 11;
  }
  std::printf("motion_amvp_host_check: %ld calls, %ld priced small PUs checked (%ld saturated, %ld of 62 bits and more), no finding\n", calls, priced, saturated, wide);
  return priced > 0 && saturated > 0 && wide > 0 ? 0 : 12;
}
