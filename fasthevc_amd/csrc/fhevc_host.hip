// fhevc_host.hip -- the functions of include/fasthevc.h that take no context and never touch the device: the band split, the YUV reader, the AQ
// partition / QP arithmetic, the host form of the P-picture rule, the two motion-compensated depth maps and the host form of the
// partition-size selection, of the tree decision and of the re-pricing against neighbour predictors.  Plain C++.
#include "../../include/fasthevc.h"
#include "fhevc_ctx.h"   // sqrt_lambda_intra
#include "fhevc_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

// ---- P-picture depth range from motion nodes + co-located depths (host-side integer rule; spec in include/fasthevc.h) ----
namespace {
inline int32_t ilog2_q8(uint32_t x)  // floor(256 log2 x) by integer squaring
{
  const int msb = 31 - __builtin_clz(x | 1u);
  uint64_t y = ((uint64_t)x << 31) >> msb;
  int32_t r = msb << 8;
  for (int b = 7; b >= 0; --b) {
    y = (y * y) >> 31;
    if (y >> 32) { r |= 1 << b; y >>= 1; }
  }
  return r;
}
struct PNodeRef { int first, per_row; };
constexpr PNodeRef kLevel[4] = { { 0, 1 }, { 1, 2 }, { 5, 4 }, { 21, 8 } };
int64_t p_split_score(const fhevc_motion_node* nodes, const uint8_t* prev, int lvl, int nx, int ny, int qp, const fhevc_p_rule& r)
{
  const fhevc_motion_node& n = nodes[kLevel[lvl].first + ny * kLevel[lvl].per_row + nx];
  int64_t child_cost = 0, child_satd = 0;
  int moved = 0;
  for (int k = 0; k < 4; ++k) {
    const fhevc_motion_node& c = nodes[kLevel[lvl + 1].first + (2 * ny + (k >> 1)) * kLevel[lvl + 1].per_row + 2 * nx + (k & 1)];
    child_cost += c.cost_best; child_satd += c.satd_best;
    moved += (c.mvx != n.mvx) || (c.mvy != n.mvy);
  }
  const int units = 16 >> lvl;
  int deepest = 0, shallowest = 3;
  for (int y = 0; y < units; ++y)
    for (int x = 0; x < units; ++x) {
      const int d = prev[(ny * units + y) * 16 + nx * units + x];
      deepest = std::max(deepest, d); shallowest = std::min(shallowest, d);
    }
  const int64_t gain = std::max<int64_t>(0, (int64_t)n.cost_best - child_cost);
  const int norm = 512 * (6 - lvl) + (qp * 256) / 6;
  const int64_t f[9] = { ilog2_q8(n.satd_best + 1u) - norm, ilog2_q8((uint32_t)gain + 1u) - norm, ilog2_q8((uint32_t)child_satd + 1u) - norm,
                         ilog2_q8(n.satd_zero + 1u) - ilog2_q8(n.satd_best + 1u), deepest > lvl ? 256 : 0, shallowest > lvl ? 256 : 0,
                         deepest > lvl + 1 ? 256 : 0, 64 * moved, 8 * qp };
  int64_t s = r.w[lvl][9];
  for (int i = 0; i < 9; ++i) s += (int64_t)r.w[lvl][i] * f[i];
  return s;
}
}  // namespace

extern "C" {

const char* fhevc_version(void) { return "fasthevc_amd 0.1.0 (gfx950)"; }

int fhevc_band(int ctu_rows, int rank, int world, int* begin, int* end)
{
  if (ctu_rows < 0 || world <= 0 || rank < 0 || rank >= world || !begin || !end) return FHEVC_E_INVALID;
  *begin = (int)(((long long)rank * ctu_rows) / world);
  *end = (int)(((long long)(rank + 1) * ctu_rows) / world);
  return FHEVC_OK;
}

int fhevc_read_yuv_luma(const char* path, int file_width, int file_height, int file_bit_depth, int chroma_format, long long first_frame,
                        int num_frames, int dst_width, int dst_height, int internal_bit_depth, int dst_sample_bytes, void* dst,
                        long long dst_stride_samples, long long dst_frame_stride_samples)
{
  if (!path || !dst || file_width < 1 || file_height < 1 || num_frames < 0 || first_frame < 0) return FHEVC_E_INVALID;
  if (file_bit_depth < 8 || file_bit_depth > 16 || internal_bit_depth < file_bit_depth || internal_bit_depth > 12) return FHEVC_E_INVALID;
  if (dst_width < file_width || dst_height < file_height || dst_stride_samples < dst_width) return FHEVC_E_INVALID;
  if (dst_sample_bytes != 1 && dst_sample_bytes != 2) return FHEVC_E_INVALID;
  if (dst_sample_bytes == 1 && (file_bit_depth != 8 || internal_bit_depth != 8)) return FHEVC_E_INVALID;
  if (num_frames > 1 && dst_frame_stride_samples < dst_stride_samples * (dst_height - 1) + dst_width) return FHEVC_E_INVALID;
  const long long bps = file_bit_depth > 8 ? 2 : 1;
  long long chroma_samples;  // both chroma planes of the FILE's format
  const long long cw = (file_width + 1) / 2, chh = (file_height + 1) / 2;
  switch (chroma_format) {
    case 400: chroma_samples = 0; break;
    case 420: chroma_samples = 2 * cw * chh; break;
    case 422: chroma_samples = 2 * cw * file_height; break;
    case 444: chroma_samples = 2LL * file_width * file_height; break;
    default: return FHEVC_E_INVALID;
  }
  const long long luma_bytes = (long long)file_width * file_height * bps, frame_bytes = luma_bytes + chroma_samples * bps;
  FILE* fp = std::fopen(path, "rb");
  if (!fp) return FHEVC_E_STATE;
  const int shift = internal_bit_depth - file_bit_depth;
  std::vector<uint8_t> row8;
  int done = 0;
  for (; done < num_frames; ++done) {
    if (fseeko(fp, (off_t)((first_frame + done) * frame_bytes), SEEK_SET) != 0) break;
    bool ok = true;
    if (dst_sample_bytes == 1) {
      uint8_t* plane = static_cast<uint8_t*>(dst) + (size_t)done * (size_t)dst_frame_stride_samples;
      if (dst_width == file_width && dst_stride_samples == file_width) ok = std::fread(plane, 1, (size_t)luma_bytes, fp) == (size_t)luma_bytes;  // one read, file -> destination
      else
        for (int y = 0; y < file_height && ok; ++y) ok = std::fread(plane + (size_t)y * dst_stride_samples, 1, (size_t)file_width, fp) == (size_t)file_width;
      if (!ok) break;
      for (int y = 0; y < file_height; ++y) {
        uint8_t* r = plane + (size_t)y * dst_stride_samples;
        for (int x = file_width; x < dst_width; ++x) r[x] = r[file_width - 1];
      }
      for (int y = file_height; y < dst_height; ++y) std::memcpy(plane + (size_t)y * dst_stride_samples, plane + (size_t)(file_height - 1) * dst_stride_samples, (size_t)dst_width);
    } else {
      int16_t* plane = static_cast<int16_t*>(dst) + (size_t)done * (size_t)dst_frame_stride_samples;
      if (bps == 1) row8.resize((size_t)file_width);
      for (int y = 0; y < file_height && ok; ++y) {
        int16_t* r = plane + (size_t)y * dst_stride_samples;
        if (bps == 2) {  // two little-endian bytes per sample: the host is little-endian (x86-64), read them in place
          ok = std::fread(r, 2, (size_t)file_width, fp) == (size_t)file_width;
          if (shift) for (int x = 0; x < file_width; ++x) r[x] = (int16_t)(r[x] << shift);
        } else {
          ok = std::fread(row8.data(), 1, (size_t)file_width, fp) == (size_t)file_width;
          for (int x = 0; x < file_width; ++x) r[x] = (int16_t)((int)row8[(size_t)x] << shift);
        }
        for (int x = file_width; x < dst_width; ++x) r[x] = r[file_width - 1];
      }
      if (!ok) break;
      for (int y = file_height; y < dst_height; ++y) std::memcpy(plane + (size_t)y * dst_stride_samples, plane + (size_t)(file_height - 1) * dst_stride_samples, (size_t)dst_width * 2);
    }
  }
  std::fclose(fp);
  if (done == 0 && num_frames > 0) return FHEVC_E_STATE;
  return done;
}

int fhevc_aq_parts(int width, int height, int max_aq_depth, long long* layer_offsets)
{
  if (width <= 0 || height <= 0 || max_aq_depth < 1 || max_aq_depth > 4) return FHEVC_E_INVALID;
  long long off = 0;
  for (int d = 0; d < max_aq_depth; ++d) {
    if (layer_offsets) layer_offsets[d] = off;
    const int p = 64 >> d;
    off += (long long)((width + p - 1) / p) * ((height + p - 1) / p);
  }
  if (layer_offsets) layer_offsets[max_aq_depth] = off;
  return (int)off;
}

int fhevc_aq_qp(const double* activity, const double* avg_activity, int width, int height, int max_aq_depth,
                int qp_adaptation_range, int base_qp, int qp_bd_offset, int8_t* qp)
{
  long long off[5];
  if (!activity || !avg_activity || !qp || fhevc_aq_parts(width, height, max_aq_depth, off) < 0) return FHEVC_E_INVALID;
  if (base_qp < -qp_bd_offset || base_qp > 51 || qp_bd_offset < 0 || qp_bd_offset > 48) return FHEVC_E_INVALID;
  const double max_q_scale = std::pow(2.0, qp_adaptation_range / 6.0);
  for (int d = 0; d < max_aq_depth; ++d) {
    const double avg = avg_activity[d];
    for (long long i = off[d]; i < off[d + 1]; ++i) {
      const double act = activity[i];
      const double norm = (max_q_scale * act + avg) / (act + max_q_scale * avg);
      const double qoff = std::log(norm) / std::log(2.0) * 6.0;
      const int v = base_qp + (int)std::floor(qoff + 0.49999);
      qp[i] = (int8_t)std::min(51, std::max(-qp_bd_offset, v));
    }
  }
  return FHEVC_OK;
}

// the entry of a CTU's FHEVC_PUS_PER_CTU that holds part `part` of shape `shape` of CU node `node`: the 64x64 and 32x32 nodes carry all six shapes, the 16x16
// nodes the two symmetric ones (their AMP parts are 4 samples wide, below the 8x8 tiles)
int fhevc_motion_pu_index(int node, int shape, int part)
{
  if (node < 0 || shape < 0 || part < 0 || part > 1) return -1;
  if (node < 5) return shape < 6 ? node * 12 + shape * 2 + part : -1;
  if (node < 21) return shape < 2 ? 60 + (node - 5) * 4 + shape * 2 + part : -1;
  return -1;
}

// the entry of a CTU's FHEVC_PUS_SMALL_PER_CTU: the four AMP shapes of the 16x16 nodes first, then the two symmetric shapes of the 8x8 nodes
int fhevc_motion_pu_small_index(int node, int shape, int part)
{
  if (part < 0 || part > 1) return -1;
  if (node >= 5 && node < 21) return shape >= 2 && shape < 6 ? (node - 5) * 8 + (shape - 2) * 2 + part : -1;
  if (node >= 21 && node < 85) return shape >= 0 && shape < 2 ? 128 + (node - 21) * 4 + shape * 2 + part : -1;
  return -1;
}

void fhevc_p_rule_default(fhevc_p_rule* rule)
{
  if (!rule) return;
  // logistic fit of HM-16.14's own P-picture split decisions (vanilla decision path, tests/quality/make_labels_p.py +
  // p_features.py + fit_p_rule.py) on seeded pan clips of all synthetic families; weights Q10, bias and thresholds Q18
  static const int32_t w[3][10] = FHEVC_P_RULE_WEIGHTS;
  std::memcpy(rule->w, w, sizeof w);
  const int32_t ts[3] = FHEVC_P_RULE_T_SPLIT, tp[3] = FHEVC_P_RULE_T_STOP;
  std::memcpy(rule->t_split, ts, sizeof ts);
  std::memcpy(rule->t_stop, tp, sizeof tp);
  rule->window = FHEVC_P_RULE_WINDOW;
}

void fhevc_p_rule_default_wide(fhevc_p_rule* rule)
{
  if (!rule) return;
  fhevc_p_rule_default(rule);   // thresholds and window as the default rule: same score semantics (a logit)
  static const int32_t w[3][10] = FHEVC_P_RULE_WIDE_WEIGHTS;
  std::memcpy(rule->w, w, sizeof w);
}

int fhevc_p_depth_range(const fhevc_motion_node* nodes, const uint8_t* prev_depth, int valid_w, int valid_h, int qp, const fhevc_p_rule* rule,
                        uint8_t* depth_min, uint8_t* depth_max)
{
  if (!nodes || !prev_depth || !rule || !depth_min || !depth_max || valid_w < 8 || valid_w > 64 || valid_h < 8 || valid_h > 64 || qp < 0 || qp > 51)
    return FHEVC_E_INVALID;
  std::memset(depth_min, 0, 256);
  std::memset(depth_max, 0, 256);
  // split decisions of the 21 nodes, both thresholds, evaluated lazily top-down; -1 = not evaluated
  int8_t sure[21], maybe[21];
  std::memset(sure, -1, sizeof sure);
  std::memset(maybe, -1, sizeof maybe);
  auto decide = [&](int lvl, int nx, int ny) {
    const int id = kLevel[lvl].first + ny * kLevel[lvl].per_row + nx, n = 64 >> lvl;
    if (sure[id] >= 0) return id;
    if (nx * n + n > valid_w || ny * n + n > valid_h) { sure[id] = maybe[id] = 1; return id; }  // crosses the picture edge
    const int64_t s = p_split_score(nodes, prev_depth, lvl, nx, ny, qp, *rule);
    sure[id] = s > rule->t_split[lvl];
    maybe[id] = s >= -(int64_t)rule->t_stop[lvl];
    return id;
  };
  for (int uy = 0; uy * 4 < valid_h; ++uy)
    for (int ux = 0; ux * 4 < valid_w; ++ux) {
      int lo = 0, hi = 0;
      bool lo_open = true, hi_open = true;
      for (int lvl = 0; lvl < 3 && (lo_open || hi_open); ++lvl) {
        const int id = decide(lvl, ux >> (4 - lvl), uy >> (4 - lvl));
        lo_open = lo_open && sure[id];
        hi_open = hi_open && maybe[id];
        if (lo_open) lo = lvl + 1;
        if (hi_open) hi = lvl + 1;
      }
      if (rule->window < 4) {
        const int p = prev_depth[uy * 16 + ux];
        lo = std::min(3, std::max(0, std::max(lo, p - rule->window)));
        hi = std::min(3, std::max(0, std::min(hi, p + rule->window)));
        if (lo > hi) lo = hi;
      }
      depth_min[uy * 16 + ux] = (uint8_t)lo;
      depth_max[uy * 16 + ux] = (uint8_t)hi;
    }
  return FHEVC_OK;
}

// ---- partition sizes per CU from the refined PU costs (spec in include/fasthevc.h; the device form is k_pu_shape.hip) ----

void fhevc_pu_shape_rule_default(fhevc_pu_shape_rule* rule)
{
  if (!rule) return;
  std::memset(rule, 0, sizeof *rule);   // the unfitted hard decision: no margins
  rule->amp_mode = 1;
}

// merge_pus: null for fhevc_pu_shape_select; otherwise the merge records of the 124 PUs and (or null: all markers) of the 384, of which cost_best is read: a part
// costs the smaller of its refined and its merge cost (a null pus_small: all markers too), and merged (or null) says per node for which parts that is the merge cost
static int pu_shape_select(const fhevc_motion_qpel_node* nodes, const fhevc_motion_qpel_node* pus, const fhevc_motion_qpel_node* pus_small,
                           const fhevc_motion_merge_node* merge_pus, const fhevc_motion_merge_node* merge_small, int valid_w, int valid_h, const fhevc_pu_shape_rule* rule,
                           fhevc_pu_shape_node* out, uint32_t* costs, uint16_t* merged)
{
  if (!nodes || !pus || !rule || !out || valid_w < 8 || valid_w > 64 || valid_h < 8 || valid_h > 64 || fhevc_pu_shape_rule_error(*rule)) return FHEVC_E_INVALID;
  const uint32_t none = 0xFFFFFFFFu;
  static const int order[7] = { FHEVC_PART_2Nx2N, FHEVC_PART_Nx2N, FHEVC_PART_2NxN, FHEVC_PART_2NxnU, FHEVC_PART_2NxnD, FHEVC_PART_nLx2N, FHEVC_PART_nRx2N };
  for (int k = 0; k < FHEVC_NODES; ++k) {
    const int lvl = k < 1 ? 0 : (k < 5 ? 1 : (k < 21 ? 2 : 3));
    const int size = 64 >> lvl, idx = k - kLevel[lvl].first, nx = idx % kLevel[lvl].per_row, ny = idx / kLevel[lvl].per_row;
    const bool valid = nx * size + size <= valid_w && ny * size + size <= valid_h;
    uint32_t cost[8];
    for (int p = 0; p < 8; ++p) cost[p] = none;
    unsigned bits = 0;
    if (valid) {
      cost[0] = nodes[k].cost_best;
      for (int p = 1; p < 8; ++p) {
        if (p == 3) continue;
        const int shape = p < 3 ? p - 1 : p - 2;
        // the two parts: in pus where fhevc_motion_pu_index covers the combination, otherwise in pus_small where fhevc_motion_pu_small_index does
        const fhevc_motion_qpel_node* src = pus;
        const fhevc_motion_merge_node* msrc = merge_pus;
        int e0 = fhevc_motion_pu_index(k, shape, 0);
        if (e0 < 0) { src = pus_small; msrc = merge_small; e0 = fhevc_motion_pu_small_index(k, shape, 0); }
        if (e0 < 0 || (!src && !msrc)) continue;
        uint32_t a = src ? src[e0].cost_best : none, b = src ? src[e0 + 1].cost_best : none;   // part 1 follows part 0 in both orders
        if (msrc) {   // uiMRGCost < uiMECost (TEncSearch.cpp:3373): the marker is the largest value, so it never wins
          if (msrc[e0].cost_best < a) { a = msrc[e0].cost_best; bits |= 1u << (2 * p); }
          if (msrc[e0 + 1].cost_best < b) { b = msrc[e0 + 1].cost_best; bits |= 2u << (2 * p); }
        }
        if (a == none || b == none) continue;
        cost[p] = (uint32_t)std::min<uint64_t>((uint64_t)a + b, 0xFFFFFFFEu);
      }
    }
    if (costs) std::memcpy(costs + k * 8, cost, sizeof cost);
    if (merged) merged[k] = (uint16_t)bits;
    fhevc_pu_shape_node& o = out[k];
    o.cost_2Nx2N = cost[0]; o.cost_best = o.cost_second = none;
    o.best = o.second = 255; o.mask = o.avail = 0;
    if (!valid) continue;
    for (int i = 0; i < 7; ++i) {
      const int p = order[i];
      if (cost[p] == none) continue;
      o.avail |= (uint8_t)(1 << p);
      if (cost[p] < o.cost_best) { o.cost_best = cost[p]; o.best = (uint8_t)p; }
    }
    for (int i = 0; i < 7; ++i) {
      const int p = order[i];
      if (cost[p] == none || p == o.best) continue;
      if (cost[p] < o.cost_second) { o.cost_second = cost[p]; o.second = (uint8_t)p; }
    }
    unsigned mask = 1;   // HM always checks 2Nx2N
    if (o.best != 255) {
      const uint64_t limit = (uint64_t)o.cost_best + (uint64_t)rule->margin_abs[lvl] + (((uint64_t)o.cost_best * (uint64_t)rule->margin_q8[lvl]) >> 8);
      for (int p = 0; p < 8; ++p)
        if (cost[p] != none && cost[p] <= limit) mask |= 1u << p;
    }
    if (rule->amp_mode == 1) {
      // TEncCu::deriveTestModeAMP without the merge / skip conditions (not visible to a source-only pass): the best of 2Nx2N, Nx2N, 2NxN decides which AMP pair stays
      int b3 = -1;
      uint32_t c3 = none;
      for (int i = 0; i < 3; ++i)
        if (cost[order[i]] < c3) { c3 = cost[order[i]]; b3 = order[i]; }
      if (!(b3 == FHEVC_PART_2Nx2N || b3 == FHEVC_PART_2NxN)) mask &= ~0x30u;
      if (!(b3 == FHEVC_PART_2Nx2N || b3 == FHEVC_PART_Nx2N)) mask &= ~0xC0u;
    }
    o.mask = (uint8_t)mask;
  }
  return FHEVC_OK;
}

int fhevc_pu_shape_select(const fhevc_motion_qpel_node* nodes, const fhevc_motion_qpel_node* pus, const fhevc_motion_qpel_node* pus_small, int valid_w,
                          int valid_h, const fhevc_pu_shape_rule* rule, fhevc_pu_shape_node* out, uint32_t* costs)
{
  return pu_shape_select(nodes, pus, pus_small, nullptr, nullptr, valid_w, valid_h, rule, out, costs, nullptr);
}

int fhevc_pu_shape_select_merge(const fhevc_motion_qpel_node* nodes, const fhevc_motion_qpel_node* pus, const fhevc_motion_qpel_node* pus_small,
                                const fhevc_motion_merge_node* merge_pus, const fhevc_motion_merge_node* merge_pus_small, int valid_w, int valid_h,
                                const fhevc_pu_shape_rule* rule, fhevc_pu_shape_node* out, uint32_t* costs, uint16_t* merged)
{
  if (!merge_pus) return FHEVC_E_INVALID;
  return pu_shape_select(nodes, pus, pus_small, merge_pus, merge_pus_small, valid_w, valid_h, rule, out, costs, merged);
}

// ---- P-picture depth ranges from the selection's records, bottom-up over the quad-tree (spec in include/fasthevc.h; the device form is k_p_tree.hip) ----

void fhevc_p_tree_rule_default(fhevc_p_tree_rule* rule)
{
  if (!rule) return;
  std::memset(rule, 0, sizeof *rule);   // the unfitted hard decision: no margins, no split cost
}

}  // extern "C"

// merge: null for fhevc_p_tree_select; otherwise the CTU's 85 merge records, of which cost_best is read
// skip: null but for fhevc_p_tree_select_skip and _intra; otherwise the CTU's 85 skip records, of which flags is read under skip_mask (HM's EarlyCU, TEncCu.cpp:892)
// intra: null but for fhevc_p_tree_select_intra; otherwise the CTU's 85 intra records, of which cost_best is read (HM's intra check, TEncCu.cpp:797-816)
static int p_tree_select(const fhevc_pu_shape_node* shapes, const fhevc_motion_merge_node* merge, int valid_w, int valid_h, const fhevc_p_tree_rule* rule, uint8_t* depth_min,
                         uint8_t* depth_max, fhevc_p_tree_node* tree, const fhevc_motion_skip_node* skip = nullptr, int skip_mask = 0,
                         const fhevc_intra_p_node* intra = nullptr)
{
  if (!shapes || !rule || (!depth_min && !depth_max && !tree) || valid_w < 8 || valid_w > 64 || valid_h < 8 || valid_h > 64 || fhevc_p_tree_rule_error(*rule))
    return FHEVC_E_INVALID;
  const uint32_t mark = 0xFFFFFFFFu, sat = 0xFFFFFFFEu;
  fhevc_p_tree_node t[FHEVC_NODES];
  bool sure[21], maybe[21];
  // bottom-up: the children of a node carry larger numbers, so node numbers descending
  for (int k = FHEVC_NODES - 1; k >= 0; --k) {
    const int lvl = k < 1 ? 0 : (k < 5 ? 1 : (k < 21 ? 2 : 3));
    const int size = 64 >> lvl, idx = k - kLevel[lvl].first, nx = idx % kLevel[lvl].per_row, ny = idx / kLevel[lvl].per_row;
    const bool inside = nx * size + size <= valid_w && ny * size + size <= valid_h, outside = nx * size >= valid_w || ny * size >= valid_h;
    fhevc_p_tree_node& n = t[k];
    n.cost_own = n.cost_kids = n.cost_tree = mark;
    n.flags = 0; n.level = (uint8_t)lvl; n.pad[0] = n.pad[1] = 0;
    if (lvl < 3) { sure[k] = false; maybe[k] = true; }
    if (outside || (lvl == 3 && !inside)) { n.flags = 8; continue; }   // no CU is coded there
    if (inside) n.cost_own = shapes[k].cost_best;
    // the merge cost is taken where it is strictly smaller: the marker is the largest value, so an unavailable one never is, and any cost beats a marker
    const bool merged = inside && merge && merge[k].cost_best < n.cost_own;
    if (merged) n.cost_own = merge[k].cost_best;
    // a calm node (merged, with a masked zero bit) is HM's "best mode has no coded residual": intra is not tried there; elsewhere it wins where strictly cheaper
    const bool calm = merged && skip && (skip[k].flags & skip_mask) != 0;
    if (inside && intra && !calm && intra[k].cost_best < n.cost_own) { n.cost_own = intra[k].cost_best; n.pad[0] = 1; }
    if (lvl == 3) { n.cost_tree = n.cost_own; n.flags = (uint8_t)((n.cost_own != mark ? 16 : 0) | (merged ? 64 : 0)); continue; }
    uint64_t sum = inside ? (uint64_t)rule->split_cost[lvl] : 0;
    bool marked = false;
    for (int c = 0; c < 4; ++c) {
      const fhevc_p_tree_node& ch = t[kLevel[lvl + 1].first + (2 * ny + (c >> 1)) * kLevel[lvl + 1].per_row + 2 * nx + (c & 1)];
      if (ch.flags & 8) continue;
      if (ch.cost_tree == mark) marked = true;
      else sum += ch.cost_tree;
    }
    if (!marked) n.cost_kids = (uint32_t)std::min<uint64_t>(sum, sat);
    const uint64_t own = n.cost_own, kids = n.cost_kids;
    bool split = false, stop = false;
    if (!inside) n.cost_tree = n.cost_kids;
    else if (kids == mark) n.cost_tree = n.cost_own;
    else if (own == mark) n.cost_tree = n.cost_kids;
    else {
      n.cost_tree = kids < own ? n.cost_kids : n.cost_own;   // strict "<": xCheckBestMode
      split = kids + (uint64_t)rule->split_abs[lvl] + ((kids * (uint64_t)rule->split_q8[lvl]) >> 8) < own;
      stop = own + (uint64_t)rule->stop_abs[lvl] + ((own * (uint64_t)rule->stop_q8[lvl]) >> 8) <= kids;
    }
    // a merged node with an all-zero residual is a skip: its children are never visited, whatever they would cost
    const bool early = calm;
    if (early) { n.cost_tree = n.cost_own; split = false; stop = true; }
    n.flags = (uint8_t)((split ? 1 : 0) | (stop ? 2 : 0) | (!inside ? 4 : 0) | (own != mark ? 16 : 0) | (kids != mark ? 32 : 0) | (merged ? 64 : 0) | (early ? 128 : 0));
    sure[k] = !inside || split;
    maybe[k] = !inside || !stop;
  }
  if (tree) std::memcpy(tree, t, sizeof t);
  if (depth_min) std::memset(depth_min, 0, 256);
  if (depth_max) std::memset(depth_max, 0, 256);
  // the per-unit walk of fhevc_p_depth_range, without its window
  for (int uy = 0; uy * 4 < valid_h; ++uy)
    for (int ux = 0; ux * 4 < valid_w; ++ux) {
      int lo = 0, hi = 0;
      bool lo_open = true, hi_open = true;
      for (int lvl = 0; lvl < 3 && (lo_open || hi_open); ++lvl) {
        const int id = kLevel[lvl].first + (uy >> (4 - lvl)) * kLevel[lvl].per_row + (ux >> (4 - lvl));
        lo_open = lo_open && sure[id];
        hi_open = hi_open && maybe[id];
        if (lo_open) lo = lvl + 1;
        if (hi_open) hi = lvl + 1;
      }
      if (depth_min) depth_min[uy * 16 + ux] = (uint8_t)lo;
      if (depth_max) depth_max[uy * 16 + ux] = (uint8_t)hi;
    }
  return FHEVC_OK;
}

extern "C" {

int fhevc_p_tree_select(const fhevc_pu_shape_node* shapes, int valid_w, int valid_h, const fhevc_p_tree_rule* rule, uint8_t* depth_min, uint8_t* depth_max,
                        fhevc_p_tree_node* tree)
{
  return p_tree_select(shapes, nullptr, valid_w, valid_h, rule, depth_min, depth_max, tree);
}

int fhevc_p_tree_select_merge(const fhevc_pu_shape_node* shapes, const fhevc_motion_merge_node* merge, int valid_w, int valid_h, const fhevc_p_tree_rule* rule,
                              uint8_t* depth_min, uint8_t* depth_max, fhevc_p_tree_node* tree)
{
  if (!merge) return FHEVC_E_INVALID;
  return p_tree_select(shapes, merge, valid_w, valid_h, rule, depth_min, depth_max, tree);
}

int fhevc_p_tree_select_skip(const fhevc_pu_shape_node* shapes, const fhevc_motion_merge_node* merge, const fhevc_motion_skip_node* skip, int skip_mask, int valid_w,
                             int valid_h, const fhevc_p_tree_rule* rule, uint8_t* depth_min, uint8_t* depth_max, fhevc_p_tree_node* tree)
{
  if (!merge || !skip || skip_mask < 0 || skip_mask > 3) return FHEVC_E_INVALID;
  return p_tree_select(shapes, merge, valid_w, valid_h, rule, depth_min, depth_max, tree, skip, skip_mask);
}

// ... on RD records, which carry cost_rd where the selection and the merge records keep cost_best and flags where the skip record keeps flags
int fhevc_p_tree_select_rd(const fhevc_motion_rd_node* rd_explicit, const fhevc_motion_rd_node* rd_merge, int skip_mask, int valid_w, int valid_h,
                           const fhevc_p_tree_rule* rule, uint8_t* depth_min, uint8_t* depth_max, fhevc_p_tree_node* tree)
{
  static_assert(sizeof(fhevc_motion_rd_node) == 16 && offsetof(fhevc_motion_rd_node, cost_rd) == offsetof(fhevc_pu_shape_node, cost_best) &&
                offsetof(fhevc_motion_rd_node, cost_rd) == offsetof(fhevc_motion_merge_node, cost_best) &&
                offsetof(fhevc_motion_rd_node, flags) == offsetof(fhevc_motion_skip_node, flags), "RD record layout");
  return fhevc_p_tree_select_skip(reinterpret_cast<const fhevc_pu_shape_node*>(rd_explicit), reinterpret_cast<const fhevc_motion_merge_node*>(rd_merge),
                                  reinterpret_cast<const fhevc_motion_skip_node*>(rd_merge), skip_mask, valid_w, valid_h, rule, depth_min, depth_max, tree);
}

// ... and on the folded records of fhevc_motion_rd_pu*: the same twelve bytes in front
int fhevc_p_tree_select_rd_pu(const fhevc_motion_rd_pu_node* rd_pu, const fhevc_motion_rd_node* rd_merge, int skip_mask, int valid_w, int valid_h,
                              const fhevc_p_tree_rule* rule, uint8_t* depth_min, uint8_t* depth_max, fhevc_p_tree_node* tree)
{
  static_assert(sizeof(fhevc_motion_rd_pu_node) == 16 && offsetof(fhevc_motion_rd_pu_node, cost_rd) == offsetof(fhevc_motion_rd_node, cost_rd) &&
                offsetof(fhevc_motion_rd_pu_node, flags) == offsetof(fhevc_motion_rd_node, flags) && offsetof(fhevc_motion_rd_pu_node, part) == 12,
                "RD record layout of a partition size");
  return fhevc_p_tree_select_rd(reinterpret_cast<const fhevc_motion_rd_node*>(rd_pu), rd_merge, skip_mask, valid_w, valid_h, rule, depth_min, depth_max, tree);
}

int fhevc_p_tree_select_intra(const fhevc_pu_shape_node* shapes, const fhevc_motion_merge_node* merge, const fhevc_motion_skip_node* skip, int skip_mask,
                              const fhevc_intra_p_node* intra, int valid_w, int valid_h, const fhevc_p_tree_rule* rule, uint8_t* depth_min, uint8_t* depth_max,
                              fhevc_p_tree_node* tree)
{
  if (!merge || !skip || !intra || skip_mask < 0 || skip_mask > 3) return FHEVC_E_INVALID;
  return p_tree_select(shapes, merge, valid_w, valid_h, rule, depth_min, depth_max, tree, skip, skip_mask, intra);
}

// ---- intra candidate costs per CU node for P pictures (spec in include/fasthevc.h; the device form is k_intra_p.hip) ----

int fhevc_intra_p_picture(int width, int height, int ctu_row_begin, int ctu_row_end, int qp, const fhevc_node_cost* first, const fhevc_node_cost* first4,
                          fhevc_intra_p_node* out)
{
  if (width < 8 || height < 8 || qp < 0 || qp > 51 || !first || !out) return FHEVC_E_INVALID;
  const int cw = (width + 63) / 64, ch = (height + 63) / 64;
  if (ctu_row_begin < 0 || ctu_row_end > ch || ctu_row_begin > ctu_row_end) return FHEVC_E_INVALID;
  if ((((uintptr_t)first | (uintptr_t)first4 | (uintptr_t)out) & 3) != 0) return FHEVC_E_INVALID;
  const uint32_t mark = 0xFFFFFFFFu, sat = 0xFFFFFFFEu;
  const FhevcIntraBitCost cost = fhevc_intra_bit_cost(65536.0 * sqrt_lambda_intra(qp));
  // satd and mode of record `index` as two dwords, addressed in bytes: the arrays may sit on any 4-byte alignment (a fhevc_node_cost wants 8), and the double
  // is never read
  auto dwords = [](const fhevc_node_cost* records, size_t index, uint32_t* satd, uint32_t* mode) {
    uint32_t v[2];
    std::memcpy(v, reinterpret_cast<const unsigned char*>(records) + 16 * index, sizeof v);
    *satd = v[0]; *mode = v[1] & 255u;
  };
  auto put = [](fhevc_intra_p_node* dst, uint32_t satd, uint32_t price, const uint32_t* modes, int part) {
    const uint8_t rec[16] = { (uint8_t)satd, (uint8_t)(satd >> 8), (uint8_t)(satd >> 16), (uint8_t)(satd >> 24), (uint8_t)price, (uint8_t)(price >> 8), (uint8_t)(price >> 16),
                              (uint8_t)(price >> 24), (uint8_t)modes[0], (uint8_t)modes[1], (uint8_t)modes[2], (uint8_t)modes[3], (uint8_t)part, 0, 0, 0 };
    std::memcpy(dst, rec, sizeof rec);
  };
  const uint32_t no_modes[4] = { 255, 255, 255, 255 };
  for (int i = 0; i < (ctu_row_end - ctu_row_begin) * cw; ++i) {
    const int ctu = ctu_row_begin * cw + i;
    const int valid_w = std::min(64, width - (ctu % cw) * 64), valid_h = std::min(64, height - (ctu / cw) * 64);
    for (int k = 0; k < FHEVC_NODES; ++k) {
      const int lvl = k < 1 ? 0 : (k < 5 ? 1 : (k < 21 ? 2 : 3));
      const int size = 64 >> lvl, idx = k - kLevel[lvl].first, nx = idx % kLevel[lvl].per_row, ny = idx / kLevel[lvl].per_row;
      const bool inside = nx * size + size <= valid_w && ny * size + size <= valid_h;
      fhevc_intra_p_node* dst = out + (size_t)i * FHEVC_NODES + k;
      uint32_t satd, mode;
      dwords(first, (size_t)i * FHEVC_NODES + k, &satd, &mode);
      bool have = inside && satd != mark;
      uint32_t price = fhevc_intra_p_price(satd, mode, cost), modes[4] = { mode, mode, mode, mode };
      int part = 0;
      if (lvl == 3 && first4 && inside) {
        uint64_t sum_price = 0, sum_satd = 0;
        uint32_t m4[4];
        bool have4 = true;
        for (int j = 0; j < 4; ++j) {
          uint32_t s4;
          dwords(first4, (size_t)i * FHEVC_PUS4_PER_CTU + (2 * ny + (j >> 1)) * 16 + 2 * nx + (j & 1), &s4, &m4[j]);
          have4 = have4 && s4 != mark;
          sum_price += fhevc_intra_p_price(s4, m4[j], cost); sum_satd += s4;
        }
        const uint32_t price4 = (uint32_t)std::min<uint64_t>(sum_price, sat);
        if (have4 && (!have || price4 < price)) {   // strict "<": HM tries 2Nx2N first, and xCheckBestMode keeps the earlier mode on a tie
          have = true; part = 1; price = price4; satd = (uint32_t)std::min<uint64_t>(sum_satd, sat);
          std::memcpy(modes, m4, sizeof modes);
        }
      }
      if (have) put(dst, satd, price, modes, part);
      else put(dst, mark, mark, no_modes, 0);
    }
  }
  return FHEVC_OK;
}

}  // extern "C"

// ---- refined costs re-priced against neighbour predictors (spec in include/fasthevc.h; the device form is k_motion_amvp.hip) ----
// One family of one picture: entries[band CTUs][per] in the order `index` gives for (node, shape, part) -- shape -1: the square node itself.  The candidates are
// looked up in `nodes` by picture position, the own-CU candidate in `entries`; list and choice are fhevc_mvp_choose
namespace {
struct AmvpPicture { int width, height, cw, row_begin, row_end; };

inline unsigned amvp_z(int x, int y)
{
  unsigned z = 0;
  for (int b = 0; b < 3; ++b) z |= (unsigned)((x >> b) & 1) << (2 * b) | (unsigned)((y >> b) & 1) << (2 * b + 1);
  return z;
}

void amvp_entry(const AmvpPicture& P, const FhevcMvpBitCost& cost, const fhevc_motion_qpel_node* nodes, const fhevc_motion_qpel_node* entries, int per, int i, int k, int shape,
                int part, int e, fhevc_motion_qpel_node* out, fhevc_motion_mvp* mvp)
{
  const uint32_t mark = 0xFFFFFFFFu;
  const int ctu = P.row_begin * P.cw + i, cx = ctu % P.cw, cy = ctu / P.cw;
  const int lvl = k < 1 ? 0 : (k < 5 ? 1 : (k < 21 ? 2 : 3)), n = 1 << lvl, s = 64 >> lvl;
  const int bx = (k - kLevel[lvl].first) % n, by = (k - kLevel[lvl].first) / n;
  const int cu_x = cx * 64 + bx * s, cu_y = cy * 64 + by * s;          // the CU in picture samples
  int x = cu_x, y = cu_y, w = s, h = s;
  if (shape >= 0) {                                                    // getPartIndexAndSize
    const int cut = shape < 2 ? s / 2 : ((shape & 1) ? 3 * s / 4 : s / 4);
    if (shape == 0 || shape == 2 || shape == 3) { y += part ? cut : 0; h = part ? s - cut : cut; }
    else { x += part ? cut : 0; w = part ? s - cut : cut; }
  }
  const fhevc_motion_qpel_node& in = entries[(size_t)i * per + e];
  const bool inside = cu_x + s <= P.width && cu_y + s <= P.height;
  auto packed = [](const fhevc_motion_qpel_node& r) { return (uint32_t)(uint16_t)r.mvx | (uint32_t)(uint16_t)r.mvy << 16; };
  bool av[5];
  uint32_t vec[5];
  const int sxs[5] = { x - 1, x + w - 1, x + w, x - 1, x - 1 }, sys[5] = { y + h - 1, y - 1, y - 1, y + h, y - 1 };   // L, A, AR, BL, AL
  for (int j = 0; j < 5; ++j) {
    const int sx = sxs[j], sy = sys[j];
    av[j] = false; vec[j] = 0;
    if (sx >= cu_x && sx < cu_x + s && sy >= cu_y && sy < cu_y + s) {
      // inside the entry's own CU: part 0 of the same partition size, the entry before this one
      if (part == 1) {
        const fhevc_motion_qpel_node& p0 = entries[(size_t)i * per + e - 1];
        av[j] = p0.cost_best != mark; vec[j] = packed(p0);
      }
      continue;
    }
    if (sx < 0 || sy < 0) continue;
    const int gx = sx / s, gy = sy / s;                                // the same-level node that holds the sample
    if ((gx + 1) * s > P.width || (gy + 1) * s > P.height) continue;   // not on the grid or not INSIDE
    const int ncx = gx >> lvl, ncy = gy >> lvl, nctu = ncy * P.cw + ncx;
    if (ncy < P.row_begin || ncy >= P.row_end) continue;
    const unsigned zn = amvp_z(gx & (n - 1), gy & (n - 1)), zme = amvp_z(bx, by);
    if (!(nctu < ctu || (nctu == ctu && zn < zme))) continue;          // the coding-order key, strictly smaller
    const fhevc_motion_qpel_node& r = nodes[(size_t)(nctu - P.row_begin * P.cw) * FHEVC_NODES + kLevel[lvl].first + (gy & (n - 1)) * n + (gx & (n - 1))];
    av[j] = r.cost_best != mark; vec[j] = packed(r);
  }
  const FhevcMvpChoice c = fhevc_mvp_choose(av[0], av[1], av[2], av[3], av[4], vec[0], vec[1], vec[2], vec[3], vec[4], packed(in));
  const bool priced = inside && in.cost_best != mark;
  if (out) {
    fhevc_motion_qpel_node o = in;                                     // an input marker record is copied as it is
    if (priced) o.cost_best = (uint32_t)std::min<uint64_t>((uint64_t)in.satd_best + cost.c[c.bits], 0xFFFFFFFEu);
    if (!inside) { o.satd_int = o.satd_best = o.cost_best = mark; o.mvx = o.mvy = 0; }
    out[(size_t)i * per + e] = o;
  }
  if (mvp) {
    fhevc_motion_mvp m = { 0, 0, 255, 0, 255, 0 };
    if (priced) m = { (int16_t)(c.pred & 0xFFFFu), (int16_t)(c.pred >> 16), (uint8_t)c.idx, (uint8_t)c.num_spatial, (uint8_t)c.src, (uint8_t)c.bits };
    mvp[(size_t)i * per + e] = m;
  }
}
}  // namespace

extern "C" {

int fhevc_motion_amvp_picture(int width, int height, int bit_depth, int ctu_row_begin, int ctu_row_end, int qp, const fhevc_motion_qpel_node* nodes,
                              const fhevc_motion_qpel_node* pus, const fhevc_motion_qpel_node* pus_small, fhevc_motion_qpel_node* out_nodes,
                              fhevc_motion_qpel_node* out_pus, fhevc_motion_qpel_node* out_pus_small, fhevc_motion_mvp* mvp_nodes, fhevc_motion_mvp* mvp_pus,
                              fhevc_motion_mvp* mvp_pus_small)
{
  if (width < 8 || height < 8 || bit_depth < 8 || bit_depth > 12 || qp < 0 || qp > 51) return FHEVC_E_INVALID;
  const int cw = (width + 63) / 64, ch = (height + 63) / 64;
  if (ctu_row_begin < 0 || ctu_row_end > ch || ctu_row_begin > ctu_row_end) return FHEVC_E_INVALID;
  if (!nodes || (!out_nodes && !out_pus && !out_pus_small && !mvp_nodes && !mvp_pus && !mvp_pus_small)) return FHEVC_E_INVALID;
  if ((!pus && (out_pus || mvp_pus)) || (!pus_small && (out_pus_small || mvp_pus_small))) return FHEVC_E_INVALID;
  // getCost(b) at the slice QP's motion lambda (the lambda does not depend on the bit depth), as the device form's launch gets it
  const FhevcMvpBitCost cost = fhevc_mvp_bit_cost_table(65536.0 * sqrt_lambda_intra(qp));
  const AmvpPicture P = { width, height, cw, ctu_row_begin, ctu_row_end };
  for (int i = 0; i < (ctu_row_end - ctu_row_begin) * cw; ++i) {
    if (out_nodes || mvp_nodes)
      for (int k = 0; k < FHEVC_NODES; ++k) amvp_entry(P, cost, nodes, nodes, FHEVC_NODES, i, k, -1, 0, k, out_nodes, mvp_nodes);
    for (int k = 0; k < FHEVC_NODES; ++k)
      for (int shape = 0; shape < 6; ++shape)
        for (int part = 0; part < 2; ++part) {
          const int e = fhevc_motion_pu_index(k, shape, part), es = fhevc_motion_pu_small_index(k, shape, part);
          if (e >= 0 && (out_pus || mvp_pus)) amvp_entry(P, cost, nodes, pus, FHEVC_PUS, i, k, shape, part, e, out_pus, mvp_pus);
          if (es >= 0 && (out_pus_small || mvp_pus_small)) amvp_entry(P, cost, nodes, pus_small, FHEVC_PUS_SMALL, i, k, shape, part, es, out_pus_small, mvp_pus_small);
        }
  }
  return FHEVC_OK;
}

int fhevc_p_motion_compensated_depth(const fhevc_motion_node* nodes, const uint8_t* prev_map, int width, int height, int ctu, uint8_t* out)
{
  if (!nodes || !prev_map || !out || width < 8 || height < 8 || ctu < 0) return FHEVC_E_INVALID;
  const int cw = (width + 63) / 64, chh = (height + 63) / 64;
  if (ctu >= cw * chh) return FHEVC_E_INVALID;
  const int x0 = (ctu % cw) * 64, y0 = (ctu / cw) * 64;
  for (int by = 0; by < 4; ++by)
    for (int bx = 0; bx < 4; ++bx) {
      // the vector of the smallest valid node around the block: 16x16, 32x32, the CTU
      const fhevc_motion_node* cand[3] = { &nodes[5 + by * 4 + bx], &nodes[1 + (by >> 1) * 2 + (bx >> 1)], &nodes[0] };
      int mvx = 0, mvy = 0;
      for (int k = 0; k < 3; ++k)
        if (cand[k]->cost_best != 0xFFFFFFFFu) { mvx = cand[k]->mvx; mvy = cand[k]->mvy; break; }
      for (int uy = 0; uy < 4; ++uy)
        for (int ux = 0; ux < 4; ++ux) {
          const int px = std::min(std::max(x0 + bx * 16 + ux * 4 + 2 + mvx, 0), width - 1);
          const int py = std::min(std::max(y0 + by * 16 + uy * 4 + 2 + mvy, 0), height - 1);
          const int sc = (py >> 6) * cw + (px >> 6);
          out[(by * 4 + uy) * 16 + bx * 4 + ux] = prev_map[(size_t)sc * 256 + ((py & 63) >> 2) * 16 + ((px & 63) >> 2)];
        }
    }
  return FHEVC_OK;
}

int fhevc_p_node_depth(const fhevc_motion_node* nodes, const uint8_t* prev_map, int width, int height, int ctu, uint8_t* out)
{
  if (!nodes || !prev_map || !out || width < 8 || height < 8 || ctu < 0) return FHEVC_E_INVALID;
  const int cw = (width + 63) / 64, chh = (height + 63) / 64;
  if (ctu >= cw * chh) return FHEVC_E_INVALID;
  const int x0 = (ctu % cw) * 64, y0 = (ctu / cw) * 64;
  auto ref_depth = [&](int x, int y) {
    x = std::min(std::max(x, 0), width - 1); y = std::min(std::max(y, 0), height - 1);
    return (int)prev_map[(size_t)((y >> 6) * cw + (x >> 6)) * 256 + ((y & 63) >> 2) * 16 + ((x & 63) >> 2)];
  };
  auto fill = [&](int ux, int uy, int units, int depth) {
    for (int y = uy; y < uy + units; ++y) std::memset(out + y * 16 + ux, depth, (size_t)units);
  };
  struct Mv { int x, y; };
  auto vector_of = [](const fhevc_motion_node& n, Mv parent) { return n.cost_best != 0xFFFFFFFFu ? Mv{ n.mvx, n.mvy } : parent; };
  const Mv v0 = vector_of(nodes[0], Mv{ 0, 0 });
  if (ref_depth(x0 + 32 + v0.x, y0 + 32 + v0.y) == 0) { fill(0, 0, 16, 0); return FHEVC_OK; }
  for (int q = 0; q < 4; ++q) {
    const int qx = q & 1, qy = q >> 1;
    const Mv v1 = vector_of(nodes[1 + q], v0);
    if (ref_depth(x0 + qx * 32 + 16 + v1.x, y0 + qy * 32 + 16 + v1.y) <= 1) { fill(qx * 8, qy * 8, 8, 1); continue; }
    for (int b = 0; b < 4; ++b) {
      const int bx = 2 * qx + (b & 1), by = 2 * qy + (b >> 1);
      const Mv v2 = vector_of(nodes[5 + by * 4 + bx], v1);
      fill(bx * 4, by * 4, 4, ref_depth(x0 + bx * 16 + 8 + v2.x, y0 + by * 16 + 8 + v2.y) <= 2 ? 2 : 3);
    }
  }
  return FHEVC_OK;
}

}  // extern "C"
