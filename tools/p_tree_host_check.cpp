// p_tree_host_check.cpp -- the host twins of the tree decision (fhevc_p_tree_select, fhevc_p_tree_select_merge, fhevc_p_tree_select_skip: one shared body in
// fasthevc_amd/csrc/fhevc_host.hip) run from a stand-alone program, so that the CPU sanitizers see them without Python in the process.  CPU only: never
// built into the library, never run on a GPU machine.  Build and run (no device code is linked or called):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/p_tree_host_check.cpp fasthevc_amd/csrc/fhevc_host.hip -o build/p_tree_host_check -fsanitize=address,undefined && build/p_tree_host_check
//
// Every input and output is a heap block of exactly its size, so a read or a write one byte outside is reported; records are also handed over 4 bytes
// off their natural alignment (any 4-byte alignment is allowed).  Prints one line and returns 0 when every call returned what it must.
#include "../include/fasthevc.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>

namespace {

std::mt19937 rng(2264);

// n records of 16 random bytes in a heap block of exactly n * 16 (+ shift) bytes, starting `shift` bytes into it
template <class T> struct Block {
  std::unique_ptr<unsigned char[]> raw;
  T* p;
  Block(int n, int shift) : raw(new unsigned char[(size_t)n * sizeof(T) + shift]), p(reinterpret_cast<T*>(raw.get() + shift))
  {
    for (size_t i = 0; i < (size_t)n * sizeof(T); ++i) raw[shift + i] = (unsigned char)rng();
  }
};

uint32_t cost()
{
  switch (rng() % 6) {
    case 0: return 0xFFFFFFFFu;
    case 1: return 0xFFFFFFF0u + rng() % 15;
    default: return 100 + rng() % 400;
  }
}

}  // namespace

int main()
{
  static_assert(sizeof(fhevc_pu_shape_node) == 16 && sizeof(fhevc_motion_merge_node) == 16 && sizeof(fhevc_motion_skip_node) == 16 && sizeof(fhevc_p_tree_node) == 16, "records");
  const int sizes[] = { 8, 12, 36, 40, 63, 64 };
  long calls = 0, skipped = 0;
  for (int it = 0; it < 4000; ++it) {
    const int shift = (it & 1) ? 4 : 0;
    Block<fhevc_pu_shape_node> shapes(85, shift);
    Block<fhevc_motion_merge_node> merge(85, shift);
    Block<fhevc_motion_skip_node> skip(85, shift);
    for (int k = 0; k < 85; ++k) {
      shapes.p[k].cost_best = cost();
      merge.p[k].cost_best = cost();
      skip.p[k].flags = (uint8_t)(rng() & ((it & 2) ? 0xFF : 3));
    }
    fhevc_p_tree_rule rule;
    fhevc_p_tree_rule_default(&rule);
    if (it % 3) {
      for (int l = 0; l < 3; ++l) {
        rule.split_q8[l] = (int32_t)(rng() % 65536); rule.stop_q8[l] = (int32_t)(rng() % 65536);
        rule.split_abs[l] = (int32_t)(rng() & 0x7FFFFFFF); rule.stop_abs[l] = (int32_t)(rng() % 200); rule.split_cost[l] = (int32_t)(rng() % 50);
      }
    }
    const int vw = sizes[rng() % 6], vh = sizes[rng() % 6];
    const int want = 1 + (int)(rng() % 7);
    std::unique_ptr<uint8_t[]> dmin((want & 1) ? new uint8_t[256] : nullptr), dmax((want & 2) ? new uint8_t[256] : nullptr);
    std::unique_ptr<fhevc_p_tree_node[]> tree((want & 4) ? new fhevc_p_tree_node[85] : nullptr), base((want & 4) ? new fhevc_p_tree_node[85] : nullptr);
    const int mask = (int)(rng() % 4);
    if (fhevc_p_tree_select(shapes.p, vw, vh, &rule, dmin.get(), dmax.get(), tree.get()) != FHEVC_OK) return 1;
    if (fhevc_p_tree_select_merge(shapes.p, merge.p, vw, vh, &rule, dmin.get(), dmax.get(), base.get()) != FHEVC_OK) return 2;
    if (fhevc_p_tree_select_skip(shapes.p, merge.p, skip.p, mask, vw, vh, &rule, dmin.get(), dmax.get(), tree.get()) != FHEVC_OK) return 3;
    calls += 3;
    if (tree) {
      bool any = false;
      for (int k = 0; k < 85; ++k) {
        if (tree[k].flags & 128) {
          any = true;
          if (!(tree[k].flags & 64) || tree[k].level > 2 || tree[k].cost_tree != tree[k].cost_own || (tree[k].flags & 3) != 2) return 4;
        }
        if (tree[k].cost_own != base[k].cost_own) return 5;
      }
      skipped += any;
      if (!any && std::memcmp(tree.get(), base.get(), 85 * sizeof(fhevc_p_tree_node)) != 0) return 6;   // no record carries a masked bit: the merge tree's bytes
    }
    // rejected calls write nothing and read nothing they should not
    if (fhevc_p_tree_select_skip(shapes.p, merge.p, nullptr, mask, vw, vh, &rule, dmin.get(), dmax.get(), tree.get()) != FHEVC_E_INVALID) return 7;
    if (fhevc_p_tree_select_skip(shapes.p, merge.p, skip.p, 4, vw, vh, &rule, dmin.get(), dmax.get(), tree.get()) != FHEVC_E_INVALID) return 8;
    if (fhevc_p_tree_select_skip(shapes.p, merge.p, skip.p, -1, vw, vh, &rule, dmin.get(), dmax.get(), tree.get()) != FHEVC_E_INVALID) return 9;
    if (fhevc_p_tree_select_skip(shapes.p, merge.p, skip.p, mask, 7, vh, &rule, dmin.get(), dmax.get(), tree.get()) != FHEVC_E_INVALID) return 10;
  }
  std::printf("p_tree_host_check: %ld calls, %ld CTUs with a skipped node, no finding\n", calls, skipped);
  return skipped > 0 ? 0 : 11;
}
