// intra_p_host_check.cpp -- a stand-alone program (its own main) that drives the two host twins of the intra stage, fhevc_intra_p_picture and
// fhevc_p_tree_select_intra, on exact-size heap blocks: random bytes, random geometries and bands, arrays 4 bytes off their natural alignment, and rejected
// calls.  Every block is allocated at exactly the size the call may touch, so that a sanitizer sees any access beyond it.  Meant for a CPU build with
// -fsanitize=address,undefined of this file and fasthevc_amd/csrc/fhevc_host.hip (host code only; see DESIGN 4.10 for the command line); it needs no
// device, is never loaded into Python and never run on a GPU machine.  Exit status 0 and "no finding" on success.
#include "../include/fasthevc.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

namespace {

std::mt19937_64 rng(20240607);

// `bytes` bytes of the heap, the payload starting `off` bytes (a multiple of 4) behind malloc's alignment and ending at the block's last byte
struct Block {
  unsigned char* base;
  unsigned char* p;
  size_t n;
  Block(size_t bytes, size_t off, bool random) : base((unsigned char*)std::malloc(bytes + off)), p(base + off), n(bytes)
  {
    if (!base) std::abort();
    for (size_t i = 0; i < bytes; ++i) p[i] = random ? (unsigned char)rng() : 0xA5;
  }
  ~Block() { std::free(base); }
  bool untouched() const
  {
    for (size_t i = 0; i < n; ++i)
      if (p[i] != 0xA5) return false;
    return true;
  }
};

int fails = 0;
void expect(bool ok, const char* what)
{
  if (!ok) { std::printf("FINDING: %s\n", what); ++fails; }
}

int pick(int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); }

void stage_round()
{
  const int width = pick(8, 300), height = pick(8, 200), qp = pick(0, 51);
  const int cw = (width + 63) / 64, ch = (height + 63) / 64;
  const int rb = pick(0, ch), re = pick(rb, ch);
  const size_t ctus = (size_t)(re - rb) * cw;
  const size_t off_in = 4 * (size_t)pick(0, 3), off_in4 = 4 * (size_t)pick(0, 3), off_out = 4 * (size_t)pick(0, 3);
  const bool with4 = pick(0, 2) != 0;
  Block first(ctus * 85 * 16, off_in, true), first4(ctus * 256 * 16, off_in4, true), out(ctus * 85 * 16, off_out, false);
  // a share of markers and of the three cheap modes, so that every branch is walked
  for (size_t i = 0; i < ctus * 85; ++i) {
    if (pick(0, 7) == 0) std::memset(first.p + 16 * i, 0xFF, 4);
    if (pick(0, 3) == 0) first.p[16 * i + 4] = (unsigned char)(pick(0, 2) == 0 ? 0 : (pick(0, 1) ? 1 : 26));
  }
  for (size_t i = 0; i < ctus * 256; ++i)
    if (pick(0, 15) == 0) std::memset(first4.p + 16 * i, 0xFF, 4);
  const int rc = fhevc_intra_p_picture(width, height, rb, re, qp, (const fhevc_node_cost*)first.p, with4 ? (const fhevc_node_cost*)first4.p : nullptr,
                                       (fhevc_intra_p_node*)out.p);
  expect(rc == FHEVC_OK, "fhevc_intra_p_picture rejected a legal call");
  // every record is a marker or a record with a zero pad
  for (size_t i = 0; i < ctus * 85; ++i) {
    const unsigned char* r = out.p + 16 * i;
    expect(r[13] == 0 && r[14] == 0 && r[15] == 0 && r[12] <= 1, "a record's part or pad");
  }
  // rejected: nothing written
  Block clean(ctus * 85 * 16, off_out, false);
  const fhevc_node_cost* f = (const fhevc_node_cost*)first.p;
  fhevc_intra_p_node* o = (fhevc_intra_p_node*)clean.p;
  expect(fhevc_intra_p_picture(7, height, rb, re, qp, f, nullptr, o) == FHEVC_E_INVALID, "width 7");
  expect(fhevc_intra_p_picture(width, 7, 0, 0, qp, f, nullptr, o) == FHEVC_E_INVALID, "height 7");
  expect(fhevc_intra_p_picture(width, height, rb, re, 52, f, nullptr, o) == FHEVC_E_INVALID, "qp 52");
  expect(fhevc_intra_p_picture(width, height, rb, re, -1, f, nullptr, o) == FHEVC_E_INVALID, "qp -1");
  expect(fhevc_intra_p_picture(width, height, -1, re, qp, f, nullptr, o) == FHEVC_E_INVALID, "band begins below 0");
  expect(fhevc_intra_p_picture(width, height, rb, ch + 1, qp, f, nullptr, o) == FHEVC_E_INVALID, "band ends beyond the picture");
  expect(fhevc_intra_p_picture(width, height, re + 1, re, qp, f, nullptr, o) == FHEVC_E_INVALID, "band reversed");
  expect(fhevc_intra_p_picture(width, height, rb, re, qp, nullptr, nullptr, o) == FHEVC_E_INVALID, "null input");
  expect(fhevc_intra_p_picture(width, height, rb, re, qp, f, nullptr, nullptr) == FHEVC_E_INVALID, "null output");
  expect(fhevc_intra_p_picture(width, height, rb, re, qp, (const fhevc_node_cost*)(first.p + 2), nullptr, o) == FHEVC_E_INVALID, "misaligned input");
  expect(fhevc_intra_p_picture(width, height, rb, re, qp, f, nullptr, (fhevc_intra_p_node*)(clean.p + 1)) == FHEVC_E_INVALID, "misaligned output");
  expect(clean.untouched(), "a rejected call of fhevc_intra_p_picture wrote");
}

void tree_round()
{
  const int valid_w = pick(0, 3) ? 4 * pick(2, 16) : 64, valid_h = pick(0, 3) ? 4 * pick(2, 16) : 64, mask = pick(0, 3);
  const size_t off = 4 * (size_t)pick(0, 3);
  Block shapes(85 * 16, off, true), merge(85 * 16, 4 * (size_t)pick(0, 3), true), skip(85 * 16, 4 * (size_t)pick(0, 3), true), intra(85 * 16, 4 * (size_t)pick(0, 3), true);
  // costs close to each other, so that every comparison falls both ways; a share of markers
  for (int k = 0; k < 85; ++k) {
    const uint32_t base = (uint32_t)pick(90, 110) << (2 * (k < 1 ? 3 : (k < 5 ? 2 : (k < 21 ? 1 : 0))));
    uint32_t v[3] = { base + (uint32_t)pick(0, 2), base + (uint32_t)pick(0, 2), base + (uint32_t)pick(0, 2) };
    for (int j = 0; j < 3; ++j)
      if (pick(0, 9) == 0) v[j] = 0xFFFFFFFFu;
    std::memcpy(shapes.p + 16 * k + 4, &v[0], 4);
    std::memcpy(merge.p + 16 * k + 4, &v[1], 4);
    std::memcpy(intra.p + 16 * k + 4, &v[2], 4);
  }
  fhevc_p_tree_rule rule;
  fhevc_p_tree_rule_default(&rule);
  if (pick(0, 1))
    for (int l = 0; l < 3; ++l) { rule.split_q8[l] = pick(0, 65535); rule.stop_q8[l] = pick(0, 65535); rule.split_abs[l] = pick(0, 1000); rule.stop_abs[l] = pick(0, 1000); rule.split_cost[l] = pick(0, 50); }
  const int want = pick(1, 7);
  Block dmin(256, 0, false), dmax(256, 0, false), tree(85 * 16, 4 * (size_t)pick(0, 3), false);
  const fhevc_pu_shape_node* s = (const fhevc_pu_shape_node*)shapes.p;
  const fhevc_motion_merge_node* m = (const fhevc_motion_merge_node*)merge.p;
  const fhevc_motion_skip_node* z = (const fhevc_motion_skip_node*)skip.p;
  const fhevc_intra_p_node* i = (const fhevc_intra_p_node*)intra.p;
  const int rc = fhevc_p_tree_select_intra(s, m, z, mask, i, valid_w, valid_h, &rule, (want & 1) ? dmin.p : nullptr, (want & 2) ? dmax.p : nullptr,
                                           (want & 4) ? (fhevc_p_tree_node*)tree.p : nullptr);
  expect(rc == FHEVC_OK, "fhevc_p_tree_select_intra rejected a legal call");
  expect(((want & 1) || dmin.untouched()) && ((want & 2) || dmax.untouched()) && ((want & 4) || tree.untouched()), "an output that was not asked for was written");
  if (want & 4)
    for (int k = 0; k < 85; ++k) expect(tree.p[16 * k + 14] <= 1 && tree.p[16 * k + 15] == 0, "bytes 14 and 15 of a tree record");
  Block c1(256, 0, false), c2(85 * 16, 0, false);
  fhevc_p_tree_node* t = (fhevc_p_tree_node*)c2.p;
  expect(fhevc_p_tree_select_intra(s, m, z, mask, nullptr, valid_w, valid_h, &rule, c1.p, c1.p, t) == FHEVC_E_INVALID, "null intra");
  expect(fhevc_p_tree_select_intra(s, m, nullptr, mask, i, valid_w, valid_h, &rule, c1.p, c1.p, t) == FHEVC_E_INVALID, "null skip");
  expect(fhevc_p_tree_select_intra(s, nullptr, z, mask, i, valid_w, valid_h, &rule, c1.p, c1.p, t) == FHEVC_E_INVALID, "null merge");
  expect(fhevc_p_tree_select_intra(nullptr, m, z, mask, i, valid_w, valid_h, &rule, c1.p, c1.p, t) == FHEVC_E_INVALID, "null shapes");
  expect(fhevc_p_tree_select_intra(s, m, z, 4, i, valid_w, valid_h, &rule, c1.p, c1.p, t) == FHEVC_E_INVALID, "skip_mask 4");
  expect(fhevc_p_tree_select_intra(s, m, z, -1, i, valid_w, valid_h, &rule, c1.p, c1.p, t) == FHEVC_E_INVALID, "skip_mask -1");
  expect(fhevc_p_tree_select_intra(s, m, z, mask, i, 7, valid_h, &rule, c1.p, c1.p, t) == FHEVC_E_INVALID, "valid_w 7");
  expect(fhevc_p_tree_select_intra(s, m, z, mask, i, valid_w, 65, &rule, c1.p, c1.p, t) == FHEVC_E_INVALID, "valid_h 65");
  expect(fhevc_p_tree_select_intra(s, m, z, mask, i, valid_w, valid_h, nullptr, c1.p, c1.p, t) == FHEVC_E_INVALID, "null rule");
  expect(fhevc_p_tree_select_intra(s, m, z, mask, i, valid_w, valid_h, &rule, nullptr, nullptr, nullptr) == FHEVC_E_INVALID, "no output");
  expect(c1.untouched() && c2.untouched(), "a rejected call of fhevc_p_tree_select_intra wrote");
}

}  // namespace

int main()
{
  for (int r = 0; r < 400; ++r) stage_round();
  for (int r = 0; r < 4000; ++r) tree_round();
  std::printf(fails ? "%d finding(s)\n" : "no finding (%d)\n", fails);
  return fails ? 1 : 0;
}
