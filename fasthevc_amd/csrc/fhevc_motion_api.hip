// fhevc_motion_api.hip -- the C ABI of config 4 (P pictures): the device forms of the motion stages over a device-resident batch, and the host forms
// that stage one picture pair, run device forms on the context's own stream and bring the results back.  Host-side C++ only, as fhevc_api.hip.
#include "fhevc_ctx.h"

#include <cstddef>
#include <cstring>

namespace {

// ---- the vector costs, with HM's own arithmetic (TComRdCost.h:166-174, TComRdCost.cpp:109-114, 177-190): getCost(bits) of the exp-Golomb lengths ----

double motion_lambda(int qp) { return 65536.0 * sqrt_lambda_intra(qp); }
uint32_t mv_bits_cost(double motion_lambda, unsigned bits) { return (uint32_t)((motion_lambda * bits) / 65536.0); }
unsigned exp_golomb_bits(int v)
{
  unsigned len = 1, u = (v <= 0) ? (((unsigned)(-v)) << 1) + 1 : ((unsigned)v) << 1;
  while (u != 1) { u >>= 1; len += 2; }
  return len;
}
// ... of the window of +-range whole samples in raster order, (2 range + 1)^2 entries
void mv_window_costs(int qp, int range, uint32_t* out)
{
  const double ml = motion_lambda(qp);
  const int side = 2 * range + 1;
  for (int m = 0; m < side * side; ++m) out[m] = mv_bits_cost(ml, exp_golomb_bits(((m % side) - range) << 2) + exp_golomb_bits(((m / side) - range) << 2));
}
FhevcMvCost mv_cost_table(int qp, int range)
{
  FhevcMvCost t;
  mv_window_costs(qp, range, t.c);
  return t;
}
// ... of every number of bits a quarter-sample vector can take (k_motion_refine.hip)
FhevcMvBitCost mv_bit_cost_table(int qp)
{
  FhevcMvBitCost t;
  const double ml = motion_lambda(qp);
  for (int b = 0; b < FHEVC_MV_BIT_COSTS; ++b) t.c[b] = mv_bits_cost(ml, (unsigned)b);
  return t;
}

// ---- the records of fasthevc.h as the kernels' own types (the same 16 bytes) ----

template <class P> struct Kernel;
template <> struct Kernel<fhevc_motion_node> { using T = FhevcMotionNode; };
template <> struct Kernel<fhevc_motion_qpel_node> { using T = FhevcMotionQpelNode; };
template <> struct Kernel<fhevc_motion_merge_node> { using T = FhevcMotionMergeNode; };
template <> struct Kernel<fhevc_motion_skip_node> { using T = FhevcMotionSkipNode; };
template <> struct Kernel<fhevc_pu_shape_node> { using T = FhevcPuShapeNode; };
template <> struct Kernel<fhevc_p_tree_node> { using T = FhevcPTreeNode; };
template <> struct Kernel<fhevc_motion_mvp> { using T = FhevcMotionMvp; };
template <> struct Kernel<fhevc_intra_p_node> { using T = FhevcIntraPNode; };
template <> struct Kernel<fhevc_motion_rd_node> { using T = FhevcMotionRdNode; };
template <> struct Kernel<fhevc_motion_rd_pu_node> { using T = FhevcMotionRdPuNode; };
template <> struct Kernel<fhevc_node_cost> { using T = FhevcNodeCost; };
template <class P> typename Kernel<P>::T* kn(P* p) { return reinterpret_cast<typename Kernel<P>::T*>(p); }
template <class P> const typename Kernel<P>::T* kn(const P* p) { return reinterpret_cast<const typename Kernel<P>::T*>(p); }
static_assert(sizeof(fhevc_motion_node) == 16 && sizeof(FhevcMotionNode) == 16 && sizeof(fhevc_motion_qpel_node) == 16 && sizeof(FhevcMotionQpelNode) == 16, "node layouts");
static_assert(sizeof(fhevc_motion_merge_node) == 16 && sizeof(FhevcMotionMergeNode) == 16 && sizeof(fhevc_pu_shape_node) == 16 && sizeof(FhevcPuShapeNode) == 16, "record layouts");
static_assert(sizeof(fhevc_motion_skip_node) == 16 && offsetof(fhevc_motion_skip_node, nonzero) == 8 && offsetof(fhevc_motion_skip_node, flags) == 10 &&
              offsetof(fhevc_motion_skip_node, mvx) == 12 && offsetof(FhevcMotionSkipNode, flags) == 10 && offsetof(FhevcMotionSkipNode, mvx) == 12, "skip record layout");
static_assert(sizeof(fhevc_intra_p_node) == 16 && offsetof(fhevc_intra_p_node, satd_best) == 0 && offsetof(fhevc_intra_p_node, cost_best) == 4 &&
              offsetof(fhevc_intra_p_node, modes) == 8 && offsetof(fhevc_intra_p_node, part) == 12 && offsetof(fhevc_intra_p_node, pad) == 13 &&
              sizeof(FhevcIntraPNode) == 16 && offsetof(FhevcIntraPNode, cost_best) == 4 && offsetof(FhevcIntraPNode, part) == 12, "intra record layout");
// the RD record is read by the tree kernels as a selection record, a merge record and a skip record: cost_rd where they keep cost_best, flags where flags is
static_assert(sizeof(fhevc_motion_rd_node) == 16 && offsetof(fhevc_motion_rd_node, cost_rd) == 4 && offsetof(fhevc_motion_rd_node, flags) == 10 &&
              offsetof(fhevc_motion_rd_node, mvx) == 12 && offsetof(FhevcMotionRdNode, cost_rd) == 4 && offsetof(FhevcMotionRdNode, flags) == 10 &&
              offsetof(fhevc_pu_shape_node, cost_best) == 4 && offsetof(fhevc_motion_merge_node, cost_best) == 4, "RD record layout");
// ... and so is the RD record of a partition size; byte 12 is where the size priced lies
static_assert(sizeof(fhevc_motion_rd_pu_node) == 16 && offsetof(fhevc_motion_rd_pu_node, cost_rd) == 4 && offsetof(fhevc_motion_rd_pu_node, flags) == 10 &&
              offsetof(fhevc_motion_rd_pu_node, part) == 12 && offsetof(fhevc_motion_rd_pu_node, merged) == 13 && offsetof(fhevc_motion_rd_pu_node, bits) == 8 &&
              offsetof(fhevc_motion_rd_pu_node, tu_split) == offsetof(fhevc_motion_rd_node, tu_split) && sizeof(FhevcMotionRdPuNode) == 16 &&
              offsetof(fhevc_pu_shape_node, best) == 12 && offsetof(fhevc_pu_shape_node, second) == 13, "RD record of a partition size");
static_assert(sizeof(fhevc_node_cost) == 16 && offsetof(fhevc_node_cost, satd) == 0 && offsetof(fhevc_node_cost, mode) == 4, "first-pass record layout");
// the intra candidate's RD record is the partition-size one: the mode lies in pad[0], byte 14, and part holds a number no PartSize has
static_assert(FHEVC_RD_PART_INTRA == kRdPartIntra && FHEVC_RD_PART_INTRA > 9 && FHEVC_RD_PART_INTRA != 255 && offsetof(fhevc_motion_rd_pu_node, pad) == 14 &&
              offsetof(FhevcMotionRdPuNode, pad) == 14 && sizeof(FhevcNodeCost) == sizeof(fhevc_node_cost), "RD record of the intra candidate");
// ... and the NxN candidate's own record: the costs where every RD record has them, the four modes in its last dword
template <> struct Kernel<fhevc_intra_rd_nxn_node> { using T = FhevcIntraRdNxN; };
static_assert(FHEVC_RD_PART_INTRA_NXN == kRdPartIntraNxN && FHEVC_RD_PART_INTRA_NXN == FHEVC_RD_PART_INTRA + 1 && sizeof(fhevc_intra_rd_nxn_node) == 16 &&
              sizeof(FhevcIntraRdNxN) == 16 && offsetof(fhevc_intra_rd_nxn_node, cost_rd) == 4 && offsetof(fhevc_intra_rd_nxn_node, bits) == 8 &&
              offsetof(fhevc_intra_rd_nxn_node, flags) == 10 && offsetof(fhevc_intra_rd_nxn_node, cbf) == 11 && offsetof(fhevc_intra_rd_nxn_node, modes) == 12 &&
              offsetof(FhevcIntraRdNxN, cbf) == 11 && offsetof(FhevcIntraRdNxN, modes) == 12, "record of the NxN candidate");
static_assert(FHEVC_PUS_PER_CTU == FHEVC_PUS && FHEVC_PUS_SMALL_PER_CTU == FHEVC_PUS_SMALL, "PU counts");
static_assert(sizeof(fhevc_motion_mvp) == 8 && offsetof(fhevc_motion_mvp, idx) == 4 && offsetof(fhevc_motion_mvp, bits) == 7 && offsetof(FhevcMotionMvp, bits) == 7,
              "predictor record layout");

// ---- how every device form over a batch of picture pairs opens ----

const int GO = 1;   // beside FHEVC_OK (nothing to do) and the error codes (rejected)
struct Batch { const void* luma; int sample_bytes, stride; long long frame_stride; int num_frames, row_begin, row_end, qp; };
inline const char* nothing_more() { return nullptr; }

// args_ok: the entry point's pointers (bad_args: its message; null: none is set); then the batch's layout, the range against 1..limit (bad_range), whatever
// more() finds (a message, or null) and the empty band, which launches nothing and writes nothing.  GO: *fr describes the batch
template <class More = const char* (*)()>
int open_device_form(fhevc_ctx* c, bool args_ok, const char* bad_args, const Batch& b, int range, int limit, const char* bad_range, FhevcFrames* fr, More&& more = nothing_more)
{
  if (!c) return FHEVC_E_INVALID;
  if (!args_ok) return bad_args ? fail(c, FHEVC_E_INVALID, bad_args) : FHEVC_E_INVALID;
  if (const char* bad = batch_error(c, b.sample_bytes, b.stride, b.frame_stride, b.num_frames, 2, b.row_begin, b.row_end, b.qp, true)) return fail(c, FHEVC_E_INVALID, bad);
  if (range < 1 || range > limit) return fail(c, FHEVC_E_INVALID, bad_range);
  if (const char* bad = more()) return fail(c, FHEVC_E_INVALID, bad);
  if (b.row_begin == b.row_end) return FHEVC_OK;
  *fr = frames_of(c, b.luma, b.sample_bytes, b.stride, b.frame_stride, b.num_frames, b.row_begin, b.row_end, b.qp);
  return GO;
}

// ... and the device forms of one launch: launch(frames, stream), timed and counted under `slot`
template <class L, class More = const char* (*)()>
int device_form(fhevc_ctx* c, bool args_ok, const char* bad_args, const Batch& b, int range, int limit, const char* bad_range, void* stream, int slot, const char* what,
                L&& launch, More&& more = nothing_more)
{
  FhevcFrames fr;
  const int rc = open_device_form(c, args_ok, bad_args, b, range, limit, bad_range, &fr, more);
  return rc != GO ? rc : launch_on(c, stream, slot, what, [&](hipStream_t s) { return launch(fr, s); });
}

// ---- how every host form stages its picture pair and its arrays ----
//
// The context's staging buffers, each allocated by the first call that needs it.  An entry of every family is 16 bytes, whichever record it holds:
//
//   buffer                   entries per CTU   what the host forms keep in it
//   d_pair                   --                the reference and the current picture, two planes of pair_plane() samples: a batch of two frames
//   d_motion                 85  (nodes)       the integer nodes; once the refinement has read them, the partition-size records of the frame chains;
//                                              the merge records of fhevc_motion_merge, and those fhevc_motion_skip reads; in its head, the one centre per
//                                              CTU of fhevc_motion_centres
//   d_qpel                   85                the refined nodes (the input of fhevc_motion_merge); the skip records of fhevc_motion_skip, which has no
//                                              refined nodes: the buffer is dead there
//   d_motion_pu, d_qpel_pu   124 (PUs)         the integer and the refined PUs; once the refinement has read the integer PUs, the merge records
//                                              of fhevc_p_tree_merge_frame in the head of d_motion_pu (85 of the 124 entries per CTU)
//   d_motion_pu_small,       384 (small PUs)   the integer and the refined small PUs
//   d_qpel_pu_small
//   d_centres                1                 the centres that the centred searches and refinements read
//   d_merge_pu               508 (all PUs)     the PUs' merge records: the 124 in fhevc_motion_pu_index order, behind them the 384 (fhevc_motion_merge_pu,
//                                              fhevc_p_tree_merge_pu_frame) -- 8 128 B per CTU; no dead buffer of the chain holds that much
//   d_amvp, d_amvp_mvp       593 (everything)  the re-priced entries and their predictor records (8 bytes each): the 85, behind them the 124, behind them the
//                                              384 (fhevc_motion_amvp, fhevc_p_tree_amvp_frame)
//   d_p_maps                 3 x 256 bytes     the reference picture's depth map, depth_min, depth_max (fhevc_p_predict_frame; the tree chains use the last two)
//   (fhevc_motion_rd_pu)                       its inputs: the three families of entries in d_amvp, their predictor records in d_amvp_mvp, the PUs' merge
//                                              records in d_merge_pu, the selection's records in d_motion; the folded records in d_qpel, in and out
//   (fhevc_p_tree_rd_frame)                    fhevc_p_tree_amvp_frame's buffers, with d_amvp_mvp; the merge records' RD records in d_qpel and the folded RD
//                                              records in the head of d_qpel_pu: the re-pricing has read the refined nodes and PUs by then
//   (fhevc_intra_rd)                            the picture in the second plane of d_pair, the first-pass records in the head of d_first_p, the merge records' RD
//                                              records in d_qpel, the folded records in the head of d_qpel_pu, in and out
//   (fhevc_p_tree_rd_intra_frame)              fhevc_p_tree_rd_frame's buffers and the first-pass records of the current picture in the head of d_first_p
//   (fhevc_intra_rd_nxn,                       fhevc_intra_rd's buffers, the 4x4 PUs' records behind the nodes' in d_first_p and the NxN records (64 per CTU) in the
//    fhevc_p_tree_rd_intra_nxn_frame)          head of d_intra_p, which those chains do not use
//   (fhevc_intra_rd_search,                    the same with the lists in the records' place: the nodes' in the head of d_first_p, the 4x4 PUs' where the 4x4
//    fhevc_p_tree_rd_intra_search_frame)       records begin (the frame chain, which keeps the nodes' records: both lists there)
//   d_first_p                341 (85 + 256)    the first-pass records of the nodes, behind them those of the 4x4 PUs (fhevc_intra_p, fhevc_p_tree_intra_frame)
//   d_intra_p                85                the intra records made from them
// fhevc_p_tree_intra_frame keeps its skip records in d_qpel: the re-pricing has read the refined nodes by then, and every later stage reads d_amvp
//
// The timing slots (fhevc_kernel_timing) of the launches below: 4 fhevc_motion_search, 5 the P rule, 7 fhevc_motion_refine, 8 / 9 the searches of the PUs / the
// small PUs, 10 fhevc_motion_refine_pu, 11 / 12 the wide search / refinement, 13 the partition sizes, 15 the centres and everything centred, 17 the tree, 19 the merge stage,
// 21 the merge stage per PU, 23 the zero-residual test, 25 the re-pricing against neighbour predictors, 27 the intra stage, 29 the RD estimate, 31 the RD estimate under a partition size,
// 33 the RD estimate of the intra candidate, 37 the RD estimate of the intra candidate at three TU depths (fhevc_intra_rd_qt* with tu_depths 3; at 2 it is slot 33's launch),
// 39 the same with the NxN candidate of the 8x8 nodes (fhevc_intra_rd_nxn* with d_first4; without it, it is slot 37's launch),
// 41 the same with the mode searched over the first pass's candidate lists (fhevc_intra_rd_search*),
// 35 the RD estimates at three TU depths (fhevc_motion_rd_qt*, fhevc_motion_rd_pu_qt* with tu_depths 3; at 2 they are
// the launches of slots 29 and 31)
struct Family { int per_ctu; FhevcMotionNode* fhevc_ctx::*found; FhevcMotionQpelNode* fhevc_ctx::*refined; };
constexpr Family kNodes = { FHEVC_NODES, &fhevc_ctx::d_motion, &fhevc_ctx::d_qpel }, kPus = { FHEVC_PUS, &fhevc_ctx::d_motion_pu, &fhevc_ctx::d_qpel_pu },
                 kSmall = { FHEVC_PUS_SMALL, &fhevc_ctx::d_motion_pu_small, &fhevc_ctx::d_qpel_pu_small }, kCentres = { 1, &fhevc_ctx::d_centres, nullptr };

// fn, a device form, over the staged pair: a batch of two frames, the whole picture
template <class Fn, class... A> int on_pair(fhevc_ctx* c, Fn fn, int qp, A... rest)
{
  return fn(c, c->d_pair, 2, c->dev_stride, (long long)pair_plane(c), 2, 0, c->ctus_y, qp, rest...);
}

int upload_pair(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples)
{
  HIP_TRY(c, ensure(c->d_pair, 2 * pair_plane(c) * sizeof(int16_t)));
  HIP_TRY(c, ensure(c->d_motion, (size_t)c->num_ctus * FHEVC_NODES * sizeof(FhevcMotionNode)));
  const int16_t* src[2] = { ref_luma, cur_luma };   // a form of one picture (fhevc_intra_rd) has no reference: its plane stays as it is
  for (int i = 0; i < 2; ++i) {
    if (!src[i]) continue;
    HIP_TRY(c, hipMemcpy2DAsync(c->d_pair + i * pair_plane(c), (size_t)c->dev_stride * 2, src[i], (size_t)stride_samples * 2, (size_t)c->cfg.width * 2,
                                (size_t)c->cfg.height, hipMemcpyHostToDevice, c->stream));
    c->stats.bytes_h2d += (uint64_t)c->cfg.width * c->cfg.height * 2;
  }
  return FHEVC_OK;
}

// One call of a host form.  First name what it moves: in() and out() take a staging buffer with its full size, the caller's array, the bytes to copy and
// where in the buffer they lie, and answer the device address the device form gets -- null for an array the caller left out, which moves nothing; dev()
// only claims the buffer.  Then run(): the pair and the inputs up, queue() -- the device form or chain, on the context's stream --, the outputs down,
// one synchronisation, the counters
class HostForm {
 public:
  explicit HostForm(fhevc_ctx* ctx) : c(ctx) { (void)hipSetDevice(c->device); }
  size_t bytes(const Family& f) const { return (size_t)c->num_ctus * f.per_ctu * sizeof(FhevcMotionNode); }

  template <class H, class D> H* dev(D*& buf, size_t size, size_t at = 0)
  {
    if (e == hipSuccess) e = ensure(buf, size);
    return reinterpret_cast<H*>(reinterpret_cast<char*>(buf) + at);
  }
  template <class H, class D> const H* in(D*& buf, size_t size, const H* host, size_t n, size_t at = 0) { return host ? copy(ins[n_in++], dev<H>(buf, size, at), const_cast<H*>(host), n) : nullptr; }
  template <class H, class D> H* out(D*& buf, size_t size, H* host, size_t n, size_t at = 0) { return host ? copy(outs[n_out++], dev<H>(buf, size, at), host, n) : nullptr; }
  // ... a family's integer entries in, its integer or refined entries out, or on the device only
  template <class H> const H* found_in(const Family& f, const H* host) { return in(c->*f.found, bytes(f), host, bytes(f)); }
  template <class H> H* found_out(const Family& f, H* host) { return out(c->*f.found, bytes(f), host, bytes(f)); }
  template <class H> H* refined_out(const Family& f, H* host) { return out(c->*f.refined, bytes(f), host, bytes(f)); }
  fhevc_motion_node* found(const Family& f) { return dev<fhevc_motion_node>(c->*f.found, bytes(f)); }
  fhevc_motion_qpel_node* refined(const Family& f) { return dev<fhevc_motion_qpel_node>(c->*f.refined, bytes(f)); }

  template <class Q> int run(const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, Q&& queue)
  {
    const int rc = e != hipSuccess ? fail(c, FHEVC_E_HIP, "staging buffer", e) : staged(cur_luma, ref_luma, stride_samples, queue);
    if (rc != FHEVC_OK) (void)hipStreamSynchronize(c->stream);   // the uploads read the caller's buffers, the downloads write them: through before a failed call returns
    return rc;
  }
  // ... of a form that reads no samples: only its arrays move
  template <class Q> int run(Q&& queue) { return run(nullptr, nullptr, 0, queue); }

 private:
  struct Copy { void* dev; void* host; size_t n; };
  template <class H> static H* copy(Copy& slot, H* dev, H* host, size_t n) { slot = { dev, host, n }; return dev; }

  template <class Q> int staged(const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, Q& queue)
  {
    int rc = cur_luma ? upload_pair(c, cur_luma, ref_luma, stride_samples) : FHEVC_OK;
    if (rc != FHEVC_OK) return rc;
    for (int i = 0; i < n_in; ++i) {
      HIP_TRY(c, hipMemcpyAsync(ins[i].dev, ins[i].host, ins[i].n, hipMemcpyHostToDevice, c->stream));
      c->stats.bytes_h2d += ins[i].n;
    }
    rc = queue();
    if (rc != FHEVC_OK) return rc;
    uint64_t down = 0;
    for (int i = 0; i < n_out; ++i) {
      HIP_TRY(c, hipMemcpyAsync(outs[i].host, outs[i].dev, outs[i].n, hipMemcpyDeviceToHost, c->stream));
      down += outs[i].n;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->stats.bytes_d2h += down;
    return FHEVC_OK;
  }

  fhevc_ctx* c;
  hipError_t e = hipSuccess;
  Copy ins[10], outs[8];   // at most: the ten arrays of fhevc_motion_rd_pu in; three families of records and of predictor records out (the RD chain: six too, seven with the intra candidate, eight with its NxN records)
  int n_in = 0, n_out = 0;
};

// what the host forms check before they touch the device: the context, the entry point's pointers, the stride, qp 0..51 and the range 1..limit -> GO or the error
int open_host_form(fhevc_ctx* c, bool args_ok, int stride_samples, int qp, int range, int limit, const char* bad)
{
  if (!c) return FHEVC_E_INVALID;
  if (!args_ok || stride_samples < c->cfg.width || qp < 0 || qp > 51 || range < 1 || range > limit) return fail(c, FHEVC_E_INVALID, bad);
  return GO;
}

// The frame chains: all three families through a search and its refinement on the context's stream -- coarse_range 0: the wide pair; otherwise the centres
// and the centred pair around them -- into the refined staging buffers
struct Chain {
  fhevc_motion_node *nodes, *pus, *small, *centres;
  fhevc_motion_qpel_node *q_nodes, *q_pus, *q_small;
  fhevc_motion_qpel_node *q_nodes_out = nullptr, *q_pus_out = nullptr, *q_small_out = nullptr;   // fhevc_p_tree_amvp_frame: where the re-priced records go
};
Chain claim_chain(HostForm& h, bool centred)
{
  return { h.found(kNodes), h.found(kPus), h.found(kSmall), centred ? h.found(kCentres) : nullptr, h.refined(kNodes), h.refined(kPus), h.refined(kSmall) };
}
int queue_chain(fhevc_ctx* c, int qp, int search_range, int coarse_range, const Chain& k)
{
  int rc;
  if (!coarse_range) {
    rc = on_pair(c, fhevc_motion_search_pu_wide_device, qp, search_range, k.nodes, k.pus, k.small, c->stream);
    return rc != FHEVC_OK ? rc : on_pair(c, fhevc_motion_refine_pu_wide_device, qp, search_range, k.nodes, k.q_nodes, k.pus, k.q_pus, k.small, k.q_small, c->stream);
  }
  rc = on_pair(c, fhevc_motion_centres_device, qp, coarse_range, k.centres, c->stream);
  if (rc == FHEVC_OK) rc = on_pair(c, fhevc_motion_search_pu_centred_device, qp, search_range, k.centres, k.nodes, k.pus, k.small, c->stream);
  return rc != FHEVC_OK ? rc : on_pair(c, fhevc_motion_refine_pu_centred_device, qp, search_range, k.centres, k.nodes, k.q_nodes, k.pus, k.q_pus, k.small, k.q_small, c->stream);
}

// what a part mode asks of the inputs of fhevc_motion_rd_pu*, the same for pointers of either kind -> a message, or null
constexpr const char* kBadTuDepths = "bad RD-stage arguments (tu_depths 2 or 3)";
const char* rd_pu_mode_error(int part_mode, const fhevc_motion_rd_pu_inputs& in)
{
  if (part_mode < 0 || part_mode > 9 || part_mode == 3) return "bad partition-size RD-stage arguments (part_mode 0, 1, 2, 4..9)";
  if (part_mode != 0 && !in.pus) return "bad partition-size RD-stage arguments (a two-part size needs the PUs' entries)";
  if (part_mode >= 8 && !in.shapes) return "bad partition-size RD-stage arguments (part_mode 8 and 9 need the selection's records)";
  if ((!in.pus && (in.merge_pus || in.mvp_pus)) || (!in.pus_small && (in.merge_pus_small || in.mvp_pus_small)))
    return "bad partition-size RD-stage arguments (a family's merge and predictor records need that family's entries)";
  return nullptr;
}

}  // namespace

extern "C" {

// ---- source-only motion search per CU node (k_motion.hip, k_motion_wide.hip) ----

int fhevc_motion_search_device(fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                               int num_frames, int ctu_row_begin, int ctu_row_end, int qp, int search_range, fhevc_motion_node* d_out, void* stream)
{
  const bool wide = search_range > FHEVC_MOTION_MAX_RANGE;
  const Batch b{ d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, ctu_row_begin, ctu_row_end, qp };
  FhevcFrames fr;
  const int rc = open_device_form(c, d_luma && d_out, nullptr, b, search_range, FHEVC_MOTION_WIDE_MAX_RANGE, "bad motion-search arguments", &fr, [&]() -> const char* {
    if (wide && !c->motion_sad) return "search ranges above 8 need the SAD distortion (fhevc_set_motion_distortion)";
    return wide && c->cfg.bit_depth > 8 && sample_bytes != 2 ? "bad motion-search arguments" : nullptr;
  });
  if (rc != GO) return rc;
  const bool big = wide && c->cfg.bit_depth > 8;   // above 8 bit: the generic kernel laid out for the wide window (round 4); 8 bit: the byte-SAD kernel
  if (wide && (c->mvtab_qp != qp || c->mvtab_range != search_range)) {
    // the wide kernels read the window's vector costs from HBM
    (void)hipSetDevice(c->device);
    HIP_TRY(c, ensure(c->d_mvtab, sizeof(uint32_t) * (2 * FHEVC_MOTION_WIDE_MAX_RANGE + 1) * (2 * FHEVC_MOTION_WIDE_MAX_RANGE + 1)));
    // EVERY launch that reads the old table has to be through, on whatever streams the callers passed (an event behind the latest launch would
    // cover that one stream only).  A rebuild happens only when (qp, range) changes: off the hot path
    HIP_TRY(c, hipDeviceSynchronize());
    c->mvtab_host.resize((size_t)(2 * search_range + 1) * (2 * search_range + 1));
    mv_window_costs(qp, search_range, c->mvtab_host.data());
    HIP_TRY(c, hipMemcpy(c->d_mvtab, c->mvtab_host.data(), c->mvtab_host.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    c->mvtab_qp = qp; c->mvtab_range = search_range;
  }
  return launch_on(c, stream, 4, "motion search", [&](hipStream_t s) {
    if (big) return fhevc_launch_motion_big(fr, search_range, c->d_mvtab, kn(d_out), c->num_cus, s);
    if (wide) return fhevc_launch_motion_wide(fr, search_range, c->d_mvtab, kn(d_out), c->num_cus, s);
    return fhevc_launch_motion(fr, search_range, mv_cost_table(qp, search_range), kn(d_out), c->num_cus, c->motion_sad, s);
  });
}

int fhevc_motion_search(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range,
                        fhevc_motion_node* out)
{
  if (!c) return FHEVC_E_INVALID;
  if (!cur_luma || !ref_luma || !out || stride_samples < c->cfg.width) return fail(c, FHEVC_E_INVALID, "bad motion-search arguments");
  // what the device form says to these two, said before the pair is staged; which distortion a range needs stays the device form's to say
  if (qp < 0 || qp > 51) return fail(c, FHEVC_E_INVALID, "qp out of range (0..51)");
  if (search_range < 1 || search_range > FHEVC_MOTION_WIDE_MAX_RANGE) return fail(c, FHEVC_E_INVALID, "bad motion-search arguments");
  HostForm h(c);
  fhevc_motion_node* d_out = h.found_out(kNodes, out);
  return h.run(cur_luma, ref_luma, stride_samples, [&] { return on_pair(c, fhevc_motion_search_device, qp, search_range, d_out, c->stream); });
}

// ---- the search of the rectangular PUs (k_motion_pu.hip) ----

int fhevc_motion_search_pu_device(fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                                  int num_frames, int ctu_row_begin, int ctu_row_end, int qp, int search_range,
                                  fhevc_motion_node* d_nodes, fhevc_motion_node* d_pus, void* stream)
{
  const Batch b{ d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, ctu_row_begin, ctu_row_end, qp };
  return device_form(c, d_luma && d_pus, "bad PU motion-search arguments", b, search_range, FHEVC_MOTION_MAX_RANGE, "the PU motion search covers search ranges 1..8",
                     stream, 8, "fhevc_launch_motion_pu", [&](const FhevcFrames& fr, hipStream_t s) {
    return fhevc_launch_motion_pu(fr, search_range, mv_cost_table(qp, search_range), kn(d_nodes), kn(d_pus), c->num_cus, c->motion_sad, s);
  });
}

int fhevc_motion_search_pu(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range,
                           fhevc_motion_node* nodes, fhevc_motion_node* pus)
{
  const int rc = open_host_form(c, cur_luma && ref_luma && pus, stride_samples, qp, search_range, FHEVC_MOTION_MAX_RANGE, "bad PU motion-search arguments");
  if (rc != GO) return rc;
  HostForm h(c);
  fhevc_motion_node *d_nodes = h.found_out(kNodes, nodes), *d_pus = h.found_out(kPus, pus);
  return h.run(cur_luma, ref_luma, stride_samples, [&] { return on_pair(c, fhevc_motion_search_pu_device, qp, search_range, d_nodes, d_pus, c->stream); });
}

// ---- the search of the PUs with a 4-sample side (k_motion_pu_small.hip) ----

int fhevc_motion_search_pu_small_device(fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                                        int num_frames, int ctu_row_begin, int ctu_row_end, int qp, int search_range,
                                        fhevc_motion_node* d_pus, void* stream)
{
  const Batch b{ d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, ctu_row_begin, ctu_row_end, qp };
  return device_form(c, d_luma && d_pus, "bad small-PU motion-search arguments", b, search_range, FHEVC_MOTION_MAX_RANGE, "the small-PU motion search covers search ranges 1..8",
                     stream, 9, "fhevc_launch_motion_pu_small", [&](const FhevcFrames& fr, hipStream_t s) {
    return fhevc_launch_motion_pu_small(fr, search_range, mv_cost_table(qp, search_range), kn(d_pus), c->num_cus, c->motion_sad, s);
  });
}

int fhevc_motion_search_pu_small(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range,
                                 fhevc_motion_node* pus)
{
  const int rc = open_host_form(c, cur_luma && ref_luma && pus, stride_samples, qp, search_range, FHEVC_MOTION_MAX_RANGE, "bad small-PU motion-search arguments");
  if (rc != GO) return rc;
  HostForm h(c);
  fhevc_motion_node* d_pus = h.found_out(kSmall, pus);
  return h.run(cur_luma, ref_luma, stride_samples, [&] { return on_pair(c, fhevc_motion_search_pu_small_device, qp, search_range, d_pus, c->stream); });
}

// ---- the three searches at HM's own SearchRange, SAD (the MR = 64 layouts of k_motion_pu.hip and k_motion_pu_small.hip) ----

int fhevc_motion_search_pu_wide_device(fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                                       int num_frames, int ctu_row_begin, int ctu_row_end, int qp, int search_range,
                                       fhevc_motion_node* d_nodes, fhevc_motion_node* d_pus, fhevc_motion_node* d_pus_small, void* stream)
{
  FhevcFrames fr;
  const Batch b{ d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, ctu_row_begin, ctu_row_end, qp };
  const int open = open_device_form(c, d_luma && (d_nodes || d_pus || d_pus_small), "bad wide PU motion-search arguments", b, search_range, FHEVC_MOTION_WIDE_MAX_RANGE,
                                    "the wide PU motion search covers search ranges 1..64", &fr);
  if (open != GO) return open;
  FhevcMotionNode *nodes = kn(d_nodes), *pus = kn(d_pus), *small = kn(d_pus_small);
  // Always SAD, and every vector cost travels with its launch: the window's table up to +-8 (the MR = 8 layouts, several workgroups per CU), the 40 bit
  // costs above.  Nothing of the context is read or written by the launches: calls on different streams may be in flight together.  Above +-8: 8-bit
  // contexts take the byte-SAD kernel (k_motion_pu_wide.hip: one launch for whatever is asked for), contexts above 8 bit -- and 8-bit int16 planes under
  // FHEVC_PU_WIDE=generic -- the MR = 64 layouts of the generic kernels (one launch for nodes and PUs, one for the small PUs).  Timed under slot 11
  const bool big = search_range > FHEVC_MOTION_MAX_RANGE;
  if (big && c->cfg.bit_depth == 8 && !(c->knobs.pu_wide_generic && sample_bytes == 2))
    return launch_on(c, stream, 11, "fhevc_launch_motion_pu_wide", [&](hipStream_t s) {
      return fhevc_launch_motion_pu_wide(fr, search_range, mv_bit_cost_table(qp), nodes, pus, small, c->num_cus, s);
    });
  if (nodes || pus) {
    const int rc = launch_on(c, stream, 11, "fhevc_motion_search_pu_wide (nodes, PUs)", [&](hipStream_t s) {
      if (big) return fhevc_launch_motion_pu_big(fr, search_range, mv_bit_cost_table(qp), nodes, pus, c->num_cus, s);
      if (!pus) return fhevc_launch_motion(fr, search_range, mv_cost_table(qp, search_range), nodes, c->num_cus, true, s);
      return fhevc_launch_motion_pu(fr, search_range, mv_cost_table(qp, search_range), nodes, pus, c->num_cus, true, s);
    });
    if (rc != FHEVC_OK) return rc;
  }
  if (!small) return FHEVC_OK;
  return launch_on(c, stream, 11, "fhevc_motion_search_pu_wide (small PUs)", [&](hipStream_t s) {
    if (big) return fhevc_launch_motion_pu_small_big(fr, search_range, mv_bit_cost_table(qp), small, c->num_cus, s);
    return fhevc_launch_motion_pu_small(fr, search_range, mv_cost_table(qp, search_range), small, c->num_cus, true, s);
  });
}

int fhevc_motion_search_pu_wide(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range,
                                fhevc_motion_node* nodes, fhevc_motion_node* pus, fhevc_motion_node* pus_small)
{
  const int rc = open_host_form(c, cur_luma && ref_luma && (nodes || pus || pus_small), stride_samples, qp, search_range, FHEVC_MOTION_WIDE_MAX_RANGE,
                                "bad wide PU motion-search arguments");
  if (rc != GO) return rc;
  HostForm h(c);
  fhevc_motion_node *d_nodes = h.found_out(kNodes, nodes), *d_pus = h.found_out(kPus, pus), *d_small = h.found_out(kSmall, pus_small);
  return h.run(cur_luma, ref_luma, stride_samples, [&] { return on_pair(c, fhevc_motion_search_pu_wide_device, qp, search_range, d_nodes, d_pus, d_small, c->stream); });
}

// ---- one coarse motion centre per CTU from the 4:1 decimated picture pair (k_motion_coarse.hip) ----

int fhevc_motion_centres_device(fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                                int num_frames, int ctu_row_begin, int ctu_row_end, int qp, int coarse_range, fhevc_motion_node* d_centres, void* stream)
{
  const Batch b{ d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, ctu_row_begin, ctu_row_end, qp };
  // the bit costs travel with the launch: nothing of the context is read or written by it.  Timed under slot 15
  return device_form(c, d_luma && d_centres, "bad motion-centre arguments", b, coarse_range, FHEVC_MOTION_COARSE_MAX_RANGE, "the motion centres cover coarse ranges 1..14",
                     stream, 15, "fhevc_launch_motion_coarse", [&](const FhevcFrames& fr, hipStream_t s) {
    return fhevc_launch_motion_coarse(fr, coarse_range, mv_bit_cost_table(qp), kn(d_centres), c->num_cus, s);
  });
}

int fhevc_motion_centres(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int coarse_range, fhevc_motion_node* centres)
{
  const int rc = open_host_form(c, cur_luma && ref_luma && centres, stride_samples, qp, coarse_range, FHEVC_MOTION_COARSE_MAX_RANGE, "bad motion-centre arguments");
  if (rc != GO) return rc;
  HostForm h(c);
  fhevc_motion_node* d_centres = h.out(c->d_motion, h.bytes(kNodes), centres, h.bytes(kCentres));
  return h.run(cur_luma, ref_luma, stride_samples, [&] { return on_pair(c, fhevc_motion_centres_device, qp, coarse_range, d_centres, c->stream); });
}

// ---- the three integer searches around one centre per CTU (the MR = 8 layouts of k_motion_pu.hip and k_motion_pu_small.hip, centred) ----

int fhevc_motion_search_pu_centred_device(fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                                          int num_frames, int ctu_row_begin, int ctu_row_end, int qp, int search_range, const fhevc_motion_node* d_centres,
                                          fhevc_motion_node* d_nodes, fhevc_motion_node* d_pus, fhevc_motion_node* d_pus_small, void* stream)
{
  FhevcFrames fr;
  const Batch b{ d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, ctu_row_begin, ctu_row_end, qp };
  const int open = open_device_form(c, d_luma && d_centres && (d_nodes || d_pus || d_pus_small), "bad centred PU motion-search arguments", b, search_range,
                                    FHEVC_MOTION_MAX_RANGE, "the centred PU motion search covers search ranges 1..8", &fr);
  if (open != GO) return open;
  // Always SAD.  The window's table of vector costs travels with the launch and prices d = v - P, the vector relative to the centre: exactly
  // getCostOfVectorWithPredictor with the predictor 4 P.  Whether a centre is in range is the kernel's to decide (the host cannot see device centres).  Nothing of the
  // context is read or written by the launches.  One launch for nodes and PUs, one for the small PUs, each timed and counted under slot 15
  if (d_nodes || d_pus) {
    const int rc = launch_on(c, stream, 15, "fhevc_motion_search_pu_centred (nodes, PUs)", [&](hipStream_t s) {
      return fhevc_launch_motion_pu_centred(fr, search_range, mv_cost_table(qp, search_range), kn(d_centres), kn(d_nodes), kn(d_pus), c->num_cus, s);
    });
    if (rc != FHEVC_OK) return rc;
  }
  if (!d_pus_small) return FHEVC_OK;
  return launch_on(c, stream, 15, "fhevc_motion_search_pu_centred (small PUs)", [&](hipStream_t s) {
    return fhevc_launch_motion_pu_small_centred(fr, search_range, mv_cost_table(qp, search_range), kn(d_centres), kn(d_pus_small), c->num_cus, s);
  });
}

int fhevc_motion_search_pu_centred(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range,
                                   const fhevc_motion_node* centres, fhevc_motion_node* nodes, fhevc_motion_node* pus, fhevc_motion_node* pus_small)
{
  const int rc = open_host_form(c, cur_luma && ref_luma && centres && (nodes || pus || pus_small), stride_samples, qp, search_range, FHEVC_MOTION_MAX_RANGE,
                                "bad centred PU motion-search arguments");
  if (rc != GO) return rc;
  HostForm h(c);
  const fhevc_motion_node* d_centres = h.found_in(kCentres, centres);
  fhevc_motion_node *d_nodes = h.found_out(kNodes, nodes), *d_pus = h.found_out(kPus, pus), *d_small = h.found_out(kSmall, pus_small);
  return h.run(cur_luma, ref_luma, stride_samples,
               [&] { return on_pair(c, fhevc_motion_search_pu_centred_device, qp, search_range, d_centres, d_nodes, d_pus, d_small, c->stream); });
}

// ---- quarter-sample refinement of the search's vectors (k_motion_refine.hip) ----

int fhevc_motion_refine_device(fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                               int num_frames, int ctu_row_begin, int ctu_row_end, int qp, int max_range, const fhevc_motion_node* d_nodes,
                               fhevc_motion_qpel_node* d_out, void* stream)
{
  const Batch b{ d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, ctu_row_begin, ctu_row_end, qp };
  return device_form(c, d_luma && d_nodes && d_out, "bad motion-refinement arguments", b, max_range, FHEVC_MOTION_WIDE_MAX_RANGE, "bad motion-refinement arguments",
                     stream, 7, "fhevc_launch_motion_refine", [&](const FhevcFrames& fr, hipStream_t s) {
    return fhevc_launch_motion_refine(fr, max_range, mv_bit_cost_table(qp), kn(d_nodes), kn(d_out), c->num_cus, s);
  });
}

int fhevc_motion_refine(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int max_range,
                        const fhevc_motion_node* nodes, fhevc_motion_qpel_node* out)
{
  const int rc = open_host_form(c, cur_luma && ref_luma && nodes && out, stride_samples, qp, max_range, FHEVC_MOTION_WIDE_MAX_RANGE, "bad motion-refinement arguments");
  if (rc != GO) return rc;
  HostForm h(c);
  const fhevc_motion_node* d_nodes = h.found_in(kNodes, nodes);
  fhevc_motion_qpel_node* d_out = h.refined_out(kNodes, out);
  return h.run(cur_luma, ref_luma, stride_samples, [&] { return on_pair(c, fhevc_motion_refine_device, qp, max_range, d_nodes, d_out, c->stream); });
}

// ---- merge-candidate costs per CU node from the refined nodes (k_motion_merge.hip) ----

int fhevc_motion_merge_device(fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                              int num_frames, int ctu_row_begin, int ctu_row_end, int qp, int max_range, const fhevc_motion_qpel_node* d_refined,
                              fhevc_motion_merge_node* d_out, void* stream)
{
  const Batch b{ d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, ctu_row_begin, ctu_row_end, qp };
  return device_form(c, d_luma && d_refined && d_out, "bad merge-stage arguments", b, max_range, FHEVC_MOTION_WIDE_MAX_RANGE, "bad merge-stage arguments (max_range 1..64)",
                     stream, 19, "fhevc_launch_motion_merge", [&](const FhevcFrames& fr, hipStream_t s) {
    return fhevc_launch_motion_merge(fr, max_range, mv_bit_cost_table(qp), kn(d_refined), kn(d_out), c->num_cus, s);
  }, [&]() -> const char* {
    return (long long)(num_frames - 1) * (ctu_row_end - ctu_row_begin) * c->ctus_x > 0x7FFFFFFFLL ? "more than 2^31 - 1 CTUs" : nullptr;
  });
}

int fhevc_motion_merge(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int max_range,
                       const fhevc_motion_qpel_node* refined, fhevc_motion_merge_node* out)
{
  const int rc = open_host_form(c, cur_luma && ref_luma && refined && out, stride_samples, qp, max_range, FHEVC_MOTION_WIDE_MAX_RANGE, "bad merge-stage arguments");
  if (rc != GO) return rc;
  HostForm h(c);
  const fhevc_motion_qpel_node* d_refined = h.in(c->d_qpel, h.bytes(kNodes), refined, h.bytes(kNodes));
  fhevc_motion_merge_node* d_out = h.out(c->d_motion, h.bytes(kNodes), out, h.bytes(kNodes));
  return h.run(cur_luma, ref_luma, stride_samples, [&] { return on_pair(c, fhevc_motion_merge_device, qp, max_range, d_refined, d_out, c->stream); });
}

// ---- the zero-residual (skip) test per CU node at its merge vector (k_motion_skip.hip) ----

int fhevc_motion_skip_device(fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                             int num_frames, int ctu_row_begin, int ctu_row_end, int qp, int max_range, const fhevc_motion_merge_node* d_merge,
                             fhevc_motion_skip_node* d_out, void* stream)
{
  const Batch b{ d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, ctu_row_begin, ctu_row_end, qp };
  // the quantiser's numbers per TU size travel with the launch: nothing of the context is read or written by it
  return device_form(c, d_luma && d_merge && d_out, "bad skip-stage arguments", b, max_range, FHEVC_MOTION_WIDE_MAX_RANGE, "bad skip-stage arguments (max_range 1..64)",
                     stream, 23, "fhevc_launch_motion_skip", [&](const FhevcFrames& fr, hipStream_t s) {
    return fhevc_launch_motion_skip(fr, max_range, fhevc_skip_quant(qp, c->cfg.bit_depth), kn(d_merge), kn(d_out), c->num_cus, s);
  }, [&]() -> const char* {
    return (long long)(num_frames - 1) * (ctu_row_end - ctu_row_begin) * c->ctus_x > 0x7FFFFFFFLL ? "more than 2^31 - 1 CTUs" : nullptr;
  });
}

int fhevc_motion_skip(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int max_range,
                      const fhevc_motion_merge_node* merge, fhevc_motion_skip_node* out)
{
  const int rc = open_host_form(c, cur_luma && ref_luma && merge && out, stride_samples, qp, max_range, FHEVC_MOTION_WIDE_MAX_RANGE, "bad skip-stage arguments");
  if (rc != GO) return rc;
  HostForm h(c);
  const fhevc_motion_merge_node* d_merge = h.in(c->d_motion, h.bytes(kNodes), merge, h.bytes(kNodes));
  fhevc_motion_skip_node* d_out = h.out(c->d_qpel, h.bytes(kNodes), out, h.bytes(kNodes));   // no refined nodes in this call: their buffer is dead
  return h.run(cur_luma, ref_luma, stride_samples, [&] { return on_pair(c, fhevc_motion_skip_device, qp, max_range, d_merge, d_out, c->stream); });
}

// ---- the RD estimate per CU node at its merge or its explicit vector (k_motion_rd.hip) ----

int fhevc_motion_rd_qt_device(fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                              int num_frames, int ctu_row_begin, int ctu_row_end, int qp, int max_range, int source, const void* d_in,
                              const fhevc_motion_mvp* d_mvp, int tu_depths, fhevc_motion_rd_node* d_out, void* stream)
{
  const Batch b{ d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, ctu_row_begin, ctu_row_end, qp };
  // the quantiser's, the dequantiser's and lambda's numbers travel with the launch: nothing of the context is read or written by it
  return device_form(c, d_luma && d_in && d_out, "bad RD-stage arguments", b, max_range, FHEVC_MOTION_WIDE_MAX_RANGE, "bad RD-stage arguments (max_range 1..64)",
                     stream, tu_depths == 3 ? 35 : 29, "fhevc_launch_motion_rd", [&](const FhevcFrames& fr, hipStream_t s) {
    return fhevc_launch_motion_rd(fr, max_range, fhevc_rd_quant(qp, c->cfg.bit_depth), source, d_in, kn(d_mvp), kn(d_out), c->num_cus, s, tu_depths);
  }, [&]() -> const char* {
    if (tu_depths != 2 && tu_depths != 3) return kBadTuDepths;
    if (source != FHEVC_RD_SOURCE_MERGE && source != FHEVC_RD_SOURCE_EXPLICIT) return "bad RD-stage arguments (source 0..1)";
    if (d_mvp && source == FHEVC_RD_SOURCE_MERGE) return "bad RD-stage arguments (predictor records go with the explicit source)";
    if (((uintptr_t)d_in | (uintptr_t)d_mvp | (uintptr_t)d_out) & 3) return "bad RD-stage arguments (records are 4-byte aligned)";
    return (long long)(num_frames - 1) * (ctu_row_end - ctu_row_begin) * c->ctus_x > 0x7FFFFFFFLL ? "more than 2^31 - 1 CTUs" : nullptr;
  });
}

// the entry point of two TU depths: the same launch of the same instances
int fhevc_motion_rd_device(fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                           int num_frames, int ctu_row_begin, int ctu_row_end, int qp, int max_range, int source, const void* d_in,
                           const fhevc_motion_mvp* d_mvp, fhevc_motion_rd_node* d_out, void* stream)
{
  return fhevc_motion_rd_qt_device(c, d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, ctu_row_begin, ctu_row_end, qp, max_range, source, d_in, d_mvp, 2,
                                   d_out, stream);
}

int fhevc_motion_rd_qt(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int max_range, int source, const void* in,
                       const fhevc_motion_mvp* mvp, int tu_depths, fhevc_motion_rd_node* out)
{
  const bool source_ok = source == FHEVC_RD_SOURCE_EXPLICIT || (source == FHEVC_RD_SOURCE_MERGE && !mvp);
  const int rc = open_host_form(c, cur_luma && ref_luma && in && out && source_ok, stride_samples, qp, max_range, FHEVC_MOTION_WIDE_MAX_RANGE, "bad RD-stage arguments");
  if (rc != GO) return rc;
  if (tu_depths != 2 && tu_depths != 3) return fail(c, FHEVC_E_INVALID, kBadTuDepths);   // said before anything is staged
  HostForm h(c);
  const size_t bn = h.bytes(kNodes), all = bn + h.bytes(kPus) + h.bytes(kSmall);
  const void* d_in = h.in(c->d_motion, bn, static_cast<const fhevc_motion_node*>(in), bn);   // 16-byte records of either kind
  const fhevc_motion_mvp* d_mvp = h.in(c->d_amvp_mvp, all / 2, mvp, bn / 2);                  // the head of the re-pricing's predictor records
  fhevc_motion_rd_node* d_out = h.out(c->d_qpel, bn, out, bn);                                // no refined nodes in this call: their buffer is dead
  return h.run(cur_luma, ref_luma, stride_samples, [&] { return on_pair(c, fhevc_motion_rd_qt_device, qp, max_range, source, d_in, d_mvp, tu_depths, d_out, c->stream); });
}

int fhevc_motion_rd(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int max_range, int source, const void* in,
                    const fhevc_motion_mvp* mvp, fhevc_motion_rd_node* out)
{
  return fhevc_motion_rd_qt(c, cur_luma, ref_luma, stride_samples, qp, max_range, source, in, mvp, 2, out);
}

uint32_t fhevc_motion_rd_lambda_q8(int qp) { return fhevc_rd_lambda_q8(qp < 0 ? 0 : (qp > 51 ? 51 : qp)); }

// ---- the RD estimate of a CU node under a partition size, folded over several launches (the PU instances of k_motion_rd.hip) ----

int fhevc_motion_rd_pu_qt_device(fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples, int num_frames,
                                 int ctu_row_begin, int ctu_row_end, int qp, int max_range, int part_mode, const fhevc_motion_rd_pu_inputs* inputs, int tu_depths,
                                 fhevc_motion_rd_pu_node* d_out, void* stream)
{
  const Batch b{ d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, ctu_row_begin, ctu_row_end, qp };
  fhevc_motion_rd_pu_inputs in{};   // read here, handed to the kernel by value: the caller's struct is free again when this call returns
  if (inputs) in = *inputs;
  // as for the RD stage, everything the kernel needs travels with the launch: nothing of the context is read or written by it
  return device_form(c, d_luma && inputs && in.nodes && d_out, "bad partition-size RD-stage arguments", b, max_range, FHEVC_MOTION_WIDE_MAX_RANGE,
                     "bad partition-size RD-stage arguments (max_range 1..64)", stream, tu_depths == 3 ? 35 : 31, "fhevc_launch_motion_rd_pu", [&](const FhevcFrames& fr, hipStream_t s) {
    const FhevcMotionRdPuInputs k = { kn(in.nodes), kn(in.pus), kn(in.pus_small), kn(in.merge_pus), kn(in.merge_pus_small), kn(in.mvp_nodes), kn(in.mvp_pus),
                                      kn(in.mvp_pus_small), kn(in.shapes), kn(in.fold) };
    return fhevc_launch_motion_rd_pu(fr, max_range, fhevc_rd_quant(qp, c->cfg.bit_depth), part_mode, k, kn(d_out), c->num_cus, s, tu_depths);
  }, [&]() -> const char* {
    if (tu_depths != 2 && tu_depths != 3) return kBadTuDepths;
    if (const char* bad = rd_pu_mode_error(part_mode, in)) return bad;
    const uintptr_t all = (uintptr_t)in.nodes | (uintptr_t)in.pus | (uintptr_t)in.pus_small | (uintptr_t)in.merge_pus | (uintptr_t)in.merge_pus_small |
                          (uintptr_t)in.mvp_nodes | (uintptr_t)in.mvp_pus | (uintptr_t)in.mvp_pus_small | (uintptr_t)in.shapes | (uintptr_t)in.fold | (uintptr_t)d_out;
    if (all & 3) return "bad partition-size RD-stage arguments (records are 4-byte aligned)";
    const long long ctus = (long long)(num_frames - 1) * (ctu_row_end - ctu_row_begin) * c->ctus_x;
    if (ctus > 0x7FFFFFFFLL) return "more than 2^31 - 1 CTUs";
    // folding in place is one lane reading and writing one record; any other overlap of the two extents is a race between lanes
    const uintptr_t extent = (uintptr_t)ctus * FHEVC_NODES * sizeof(fhevc_motion_rd_pu_node), f = (uintptr_t)in.fold, o = (uintptr_t)d_out;
    if (in.fold && f != o && f < o + extent && o < f + extent) return "bad partition-size RD-stage arguments (fold overlaps the output without being it)";
    return nullptr;
  });
}

int fhevc_motion_rd_pu_device(fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples, int num_frames,
                              int ctu_row_begin, int ctu_row_end, int qp, int max_range, int part_mode, const fhevc_motion_rd_pu_inputs* inputs,
                              fhevc_motion_rd_pu_node* d_out, void* stream)
{
  return fhevc_motion_rd_pu_qt_device(c, d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, ctu_row_begin, ctu_row_end, qp, max_range, part_mode, inputs, 2,
                                      d_out, stream);
}

int fhevc_motion_rd_pu_qt(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int max_range, int part_mode,
                          const fhevc_motion_rd_pu_inputs* inputs, int tu_depths, fhevc_motion_rd_pu_node* out)
{
  const int rc = open_host_form(c, cur_luma && ref_luma && inputs && inputs->nodes && out, stride_samples, qp, max_range, FHEVC_MOTION_WIDE_MAX_RANGE,
                                "bad partition-size RD-stage arguments");
  if (rc != GO) return rc;
  const fhevc_motion_rd_pu_inputs& in = *inputs;
  if (tu_depths != 2 && tu_depths != 3) return fail(c, FHEVC_E_INVALID, kBadTuDepths);
  if (const char* bad = rd_pu_mode_error(part_mode, in)) return fail(c, FHEVC_E_INVALID, bad);   // said before anything is staged
  HostForm h(c);
  const size_t bn = h.bytes(kNodes), bp = h.bytes(kPus), bs = h.bytes(kSmall), all = bn + bp + bs;
  fhevc_motion_rd_pu_inputs d{};
  d.nodes = h.in(c->d_amvp, all, in.nodes, bn); d.pus = h.in(c->d_amvp, all, in.pus, bp, bn); d.pus_small = h.in(c->d_amvp, all, in.pus_small, bs, bn + bp);
  d.mvp_nodes = h.in(c->d_amvp_mvp, all / 2, in.mvp_nodes, bn / 2); d.mvp_pus = h.in(c->d_amvp_mvp, all / 2, in.mvp_pus, bp / 2, bn / 2);
  d.mvp_pus_small = h.in(c->d_amvp_mvp, all / 2, in.mvp_pus_small, bs / 2, (bn + bp) / 2);
  d.merge_pus = h.in(c->d_merge_pu, bp + bs, in.merge_pus, bp); d.merge_pus_small = h.in(c->d_merge_pu, bp + bs, in.merge_pus_small, bs, bp);
  d.shapes = h.in(c->d_motion, bn, in.shapes, bn);
  d.fold = h.in(c->d_qpel, bn, in.fold, bn);                       // folded in place on the device: the earlier records go up to where the new ones come from
  fhevc_motion_rd_pu_node* d_out = h.out(c->d_qpel, bn, out, bn);
  return h.run(cur_luma, ref_luma, stride_samples, [&] { return on_pair(c, fhevc_motion_rd_pu_qt_device, qp, max_range, part_mode, &d, tu_depths, d_out, c->stream); });
}

int fhevc_motion_rd_pu(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int max_range, int part_mode,
                       const fhevc_motion_rd_pu_inputs* inputs, fhevc_motion_rd_pu_node* out)
{
  return fhevc_motion_rd_pu_qt(c, cur_luma, ref_luma, stride_samples, qp, max_range, part_mode, inputs, 2, out);
}

// ---- the RD estimate of the intra candidate per CU node, gated and folded (the intra instances of k_motion_rd.hip) ----

static bool intra_tu_depths_ok(int tu_depths) { return tu_depths == 2 || tu_depths == 3; }

int fhevc_intra_rd_qt_device(fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples, int num_frames,
                             int ctu_row_begin, int ctu_row_end, int qp, const fhevc_node_cost* d_first, const fhevc_motion_rd_pu_node* d_fold,
                             const fhevc_motion_rd_node* d_rd_merge, int skip_mask, int tu_depths, fhevc_motion_rd_pu_node* d_out, void* stream)
{
  if (!c) return FHEVC_E_INVALID;
  if (!intra_tu_depths_ok(tu_depths)) return fail(c, FHEVC_E_INVALID, kBadTuDepths);
  if (!d_luma || !d_first || !d_out) return fail(c, FHEVC_E_INVALID, "bad intra RD-stage arguments (the planes, the first-pass records, the output)");
  // pictures, not pairs: the layout is checked as fhevc_intra_first_pass_device checks it
  if (const char* bad = batch_error(c, sample_bytes, stride_samples, frame_stride_samples, num_frames, 1, ctu_row_begin, ctu_row_end, qp, false)) return fail(c, FHEVC_E_INVALID, bad);
  if (skip_mask < 0 || skip_mask > 3) return fail(c, FHEVC_E_INVALID, "bad intra RD-stage arguments (skip_mask 0..3)");
  if (((uintptr_t)d_first | (uintptr_t)d_fold | (uintptr_t)d_rd_merge | (uintptr_t)d_out) & 3) return fail(c, FHEVC_E_INVALID, "bad intra RD-stage arguments (records are 4-byte aligned)");
  const long long ctus = (long long)num_frames * (ctu_row_end - ctu_row_begin) * c->ctus_x;
  if (ctus > 0x7FFFFFFFLL) return fail(c, FHEVC_E_INVALID, "more than 2^31 - 1 CTUs");
  // folding in place is one lane reading and writing one record; any other overlap of the two extents is a race between lanes
  const uintptr_t extent = (uintptr_t)ctus * FHEVC_NODES * sizeof(fhevc_motion_rd_pu_node), f = (uintptr_t)d_fold, o = (uintptr_t)d_out;
  if (d_fold && f != o && f < o + extent && o < f + extent) return fail(c, FHEVC_E_INVALID, "bad intra RD-stage arguments (fold overlaps the output without being it)");
  if (ctu_row_begin == ctu_row_end) return FHEVC_OK;   // an empty band: nothing to launch, nothing written
  // everything the kernel needs travels with the launch: nothing of the context is read or written by it
  const FhevcFrames fr = frames_of(c, d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, ctu_row_begin, ctu_row_end, qp);
  return launch_on(c, stream, tu_depths == 3 ? 37 : 33, "fhevc_launch_intra_rd", [&](hipStream_t s) {
    return fhevc_launch_intra_rd(fr, fhevc_rd_quant(qp, c->cfg.bit_depth), kn(d_first), kn(d_fold), kn(d_rd_merge), skip_mask, kn(d_out), c->num_cus, s, tu_depths);
  });
}

// the entry point of two TU depths: the same launch of the same instances
int fhevc_intra_rd_device(fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples, int num_frames,
                          int ctu_row_begin, int ctu_row_end, int qp, const fhevc_node_cost* d_first, const fhevc_motion_rd_pu_node* d_fold,
                          const fhevc_motion_rd_node* d_rd_merge, int skip_mask, fhevc_motion_rd_pu_node* d_out, void* stream)
{
  return fhevc_intra_rd_qt_device(c, d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, ctu_row_begin, ctu_row_end, qp, d_first, d_fold, d_rd_merge, skip_mask,
                                  2, d_out, stream);
}

int fhevc_intra_rd_qt(fhevc_ctx* c, const int16_t* luma, int stride_samples, int qp, const fhevc_node_cost* first, const fhevc_motion_rd_pu_node* fold,
                      const fhevc_motion_rd_node* rd_merge, int skip_mask, int tu_depths, fhevc_motion_rd_pu_node* out)
{
  const int rc = open_host_form(c, luma && first && out && skip_mask >= 0 && skip_mask <= 3, stride_samples, qp, 1, 1, "bad intra RD-stage arguments");
  if (rc != GO) return rc;
  if (!intra_tu_depths_ok(tu_depths)) return fail(c, FHEVC_E_INVALID, kBadTuDepths);   // said before anything is staged
  HostForm h(c);
  const size_t bn = h.bytes(kNodes), b4 = (size_t)c->num_ctus * FHEVC_PUS4_PER_CTU * sizeof(fhevc_node_cost);
  const fhevc_node_cost* d_first = h.in(c->d_first_p, bn + b4, first, bn);
  const fhevc_motion_rd_node* d_rd_merge = h.in(c->d_qpel, bn, rd_merge, bn);
  const fhevc_motion_rd_pu_node* d_fold = h.in(c->d_qpel_pu, h.bytes(kPus), fold, bn);   // folded in place on the device, as fhevc_motion_rd_pu does
  fhevc_motion_rd_pu_node* d_out = h.out(c->d_qpel_pu, h.bytes(kPus), out, bn);
  return h.run(luma, nullptr, stride_samples, [&] {   // the picture alone: the current plane of the staged pair, as a batch of one frame
    return fhevc_intra_rd_qt_device(c, c->d_pair + pair_plane(c), 2, c->dev_stride, 0, 1, 0, c->ctus_y, qp, d_first, d_fold, d_rd_merge, skip_mask, tu_depths, d_out, c->stream);
  });
}

int fhevc_intra_rd(fhevc_ctx* c, const int16_t* luma, int stride_samples, int qp, const fhevc_node_cost* first, const fhevc_motion_rd_pu_node* fold,
                   const fhevc_motion_rd_node* rd_merge, int skip_mask, fhevc_motion_rd_pu_node* out)
{
  return fhevc_intra_rd_qt(c, luma, stride_samples, qp, first, fold, rd_merge, skip_mask, 2, out);
}

// ---- ... on HM's full TU tree with the NxN candidate of the 8x8 nodes (the NxN instances of k_motion_rd.hip) ----

int fhevc_intra_rd_nxn_device(fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples, int num_frames,
                              int ctu_row_begin, int ctu_row_end, int qp, const fhevc_node_cost* d_first, const fhevc_node_cost* d_first4,
                              const fhevc_motion_rd_pu_node* d_fold, const fhevc_motion_rd_node* d_rd_merge, int skip_mask, fhevc_motion_rd_pu_node* d_out,
                              fhevc_intra_rd_nxn_node* d_nxn, void* stream)
{
  if (!c) return FHEVC_E_INVALID;
  if (!d_first4) {   // without the 4x4 records there is no candidate: the mirrored call, byte for byte and launch for launch
    if (d_nxn) return fail(c, FHEVC_E_INVALID, "bad intra NxN RD-stage arguments (the NxN records need the 4x4 first pass's records)");
    return fhevc_intra_rd_qt_device(c, d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, ctu_row_begin, ctu_row_end, qp, d_first, d_fold, d_rd_merge,
                                    skip_mask, 3, d_out, stream);
  }
  if (!d_luma || !d_first || !d_out) return fail(c, FHEVC_E_INVALID, "bad intra RD-stage arguments (the planes, the first-pass records, the output)");
  if (const char* bad = batch_error(c, sample_bytes, stride_samples, frame_stride_samples, num_frames, 1, ctu_row_begin, ctu_row_end, qp, false)) return fail(c, FHEVC_E_INVALID, bad);
  if (skip_mask < 0 || skip_mask > 3) return fail(c, FHEVC_E_INVALID, "bad intra RD-stage arguments (skip_mask 0..3)");
  if (((uintptr_t)d_first | (uintptr_t)d_first4 | (uintptr_t)d_fold | (uintptr_t)d_rd_merge | (uintptr_t)d_out | (uintptr_t)d_nxn) & 3)
    return fail(c, FHEVC_E_INVALID, "bad intra RD-stage arguments (records are 4-byte aligned)");
  const long long ctus = (long long)num_frames * (ctu_row_end - ctu_row_begin) * c->ctus_x;
  if (ctus > 0x7FFFFFFFLL) return fail(c, FHEVC_E_INVALID, "more than 2^31 - 1 CTUs");
  const uintptr_t extent = (uintptr_t)ctus * FHEVC_NODES * sizeof(fhevc_motion_rd_pu_node), f = (uintptr_t)d_fold, o = (uintptr_t)d_out;
  if (d_fold && f != o && f < o + extent && o < f + extent) return fail(c, FHEVC_E_INVALID, "bad intra RD-stage arguments (fold overlaps the output without being it)");
  if (d_nxn) {
    // the NxN records are written by other lanes than anything else is read or written by: no extent may touch theirs
    const uintptr_t n = (uintptr_t)d_nxn, nn = (uintptr_t)ctus * 64 * sizeof(fhevc_intra_rd_nxn_node), e4 = (uintptr_t)ctus * FHEVC_PUS4_PER_CTU * sizeof(fhevc_node_cost);
    const uintptr_t planes = (uintptr_t)(((long long)(num_frames - 1) * frame_stride_samples + (long long)(c->cfg.height - 1) * stride_samples + c->cfg.width) * sample_bytes);
    const uintptr_t at[6] = { o, f, (uintptr_t)d_first, (uintptr_t)d_first4, (uintptr_t)d_rd_merge, (uintptr_t)d_luma }, len[6] = { extent, extent, extent, e4, extent, planes };
    for (int i = 0; i < 6; ++i)
      if (at[i] && at[i] < n + nn && n < at[i] + len[i]) return fail(c, FHEVC_E_INVALID, "bad intra NxN RD-stage arguments (the NxN records overlap another array)");
  }
  if (ctu_row_begin == ctu_row_end) return FHEVC_OK;   // an empty band: nothing to launch, nothing written
  const FhevcFrames fr = frames_of(c, d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, ctu_row_begin, ctu_row_end, qp);
  return launch_on(c, stream, 39, "fhevc_launch_intra_rd_nxn", [&](hipStream_t s) {
    return fhevc_launch_intra_rd_nxn(fr, fhevc_rd_quant(qp, c->cfg.bit_depth), kn(d_first), kn(d_first4), kn(d_fold), kn(d_rd_merge), skip_mask, kn(d_out), kn(d_nxn), c->num_cus, s);
  });
}

int fhevc_intra_rd_nxn(fhevc_ctx* c, const int16_t* luma, int stride_samples, int qp, const fhevc_node_cost* first, const fhevc_node_cost* first4,
                       const fhevc_motion_rd_pu_node* fold, const fhevc_motion_rd_node* rd_merge, int skip_mask, fhevc_motion_rd_pu_node* out, fhevc_intra_rd_nxn_node* nxn)
{
  const int rc = open_host_form(c, luma && first && out && skip_mask >= 0 && skip_mask <= 3, stride_samples, qp, 1, 1, "bad intra RD-stage arguments");
  if (rc != GO) return rc;
  if (nxn && !first4) return fail(c, FHEVC_E_INVALID, "bad intra NxN RD-stage arguments (the NxN records need the 4x4 first pass's records)");   // said before anything is staged
  HostForm h(c);
  const size_t bn = h.bytes(kNodes), b4 = (size_t)c->num_ctus * FHEVC_PUS4_PER_CTU * sizeof(fhevc_node_cost), bx = (size_t)c->num_ctus * 64 * sizeof(fhevc_intra_rd_nxn_node);
  const fhevc_node_cost *d_first = h.in(c->d_first_p, bn + b4, first, bn), *d_first4 = h.in(c->d_first_p, bn + b4, first4, b4, bn);
  const fhevc_motion_rd_node* d_rd_merge = h.in(c->d_qpel, bn, rd_merge, bn);
  const fhevc_motion_rd_pu_node* d_fold = h.in(c->d_qpel_pu, h.bytes(kPus), fold, bn);   // folded in place on the device, as fhevc_intra_rd_qt does
  fhevc_motion_rd_pu_node* d_out = h.out(c->d_qpel_pu, h.bytes(kPus), out, bn);
  fhevc_intra_rd_nxn_node* d_nxn = h.out(c->d_intra_p, bn, nxn, bx);                     // 64 records of 16 bytes per CTU: the head of the intra records' buffer
  return h.run(luma, nullptr, stride_samples, [&] {
    return fhevc_intra_rd_nxn_device(c, c->d_pair + pair_plane(c), 2, c->dev_stride, 0, 1, 0, c->ctus_y, qp, d_first, d_first4, d_fold, d_rd_merge, skip_mask, d_out, d_nxn, c->stream);
  });
}

// ---- ... with the mode searched over the first pass's candidate lists (the search instances of k_motion_rd.hip) ----

void fhevc_intra_search_rule_default(fhevc_intra_search_rule* rule)
{
  if (!rule) return;
  // HM: 3 modes for PUs of 16 and above, 8 for 8x8 and 4x4 PUs (g_aucIntraModeNumFast_UseMPM), one MPM appended
  *rule = fhevc_intra_search_rule{ { 3, 3, 3, 8 }, 8, 1, { 0, 0 } };
}

// what is wrong with a rule under the two strides (with4: the 4x4 lists are there), or null
static const char* intra_search_rule_error(const fhevc_intra_search_rule& r, int list_stride, bool with4, int list_stride4)
{
  if (list_stride < 1 || list_stride > 8 || (with4 && (list_stride4 < 1 || list_stride4 > 8))) return "bad intra search arguments (list strides 1..8)";
  for (int l = 0; l < 4; ++l)
    if (r.count[l] < 1 || r.count[l] > list_stride) return "bad intra search rule (counts 1..list_stride)";
  if (with4 && (r.count4 < 1 || r.count4 > list_stride4)) return "bad intra search rule (count4 1..list_stride4)";
  if (r.append_planar > 1 || r.pad[0] || r.pad[1]) return "bad intra search rule (append_planar 0 / 1, pad 0)";
  return nullptr;
}

int fhevc_intra_rd_search_device(fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples, int num_frames,
                                 int ctu_row_begin, int ctu_row_end, int qp, const uint8_t* d_modes, int list_stride, const uint8_t* d_modes4, int list_stride4,
                                 const fhevc_intra_search_rule* rule, const fhevc_motion_rd_pu_node* d_fold, const fhevc_motion_rd_node* d_rd_merge, int skip_mask,
                                 fhevc_motion_rd_pu_node* d_out, fhevc_intra_rd_nxn_node* d_nxn, void* stream)
{
  if (!c) return FHEVC_E_INVALID;
  if (!d_luma || !d_modes || !rule || !d_out) return fail(c, FHEVC_E_INVALID, "bad intra search arguments (the planes, the lists, the rule, the output)");
  if (d_nxn && !d_modes4) return fail(c, FHEVC_E_INVALID, "bad intra search arguments (the NxN records need the 4x4 PUs' lists)");
  if (const char* bad = batch_error(c, sample_bytes, stride_samples, frame_stride_samples, num_frames, 1, ctu_row_begin, ctu_row_end, qp, false)) return fail(c, FHEVC_E_INVALID, bad);
  if (skip_mask < 0 || skip_mask > 3) return fail(c, FHEVC_E_INVALID, "bad intra RD-stage arguments (skip_mask 0..3)");
  if (const char* bad = intra_search_rule_error(*rule, list_stride, d_modes4 != nullptr, list_stride4)) return fail(c, FHEVC_E_INVALID, bad);
  if (((uintptr_t)d_fold | (uintptr_t)d_rd_merge | (uintptr_t)d_out | (uintptr_t)d_nxn) & 3) return fail(c, FHEVC_E_INVALID, "bad intra RD-stage arguments (records are 4-byte aligned)");
  const long long ctus = (long long)num_frames * (ctu_row_end - ctu_row_begin) * c->ctus_x;
  if (ctus > 0x7FFFFFFFLL) return fail(c, FHEVC_E_INVALID, "more than 2^31 - 1 CTUs");
  const uintptr_t extent = (uintptr_t)ctus * FHEVC_NODES * sizeof(fhevc_motion_rd_pu_node), f = (uintptr_t)d_fold, o = (uintptr_t)d_out;
  if (d_fold && f != o && f < o + extent && o < f + extent) return fail(c, FHEVC_E_INVALID, "bad intra RD-stage arguments (fold overlaps the output without being it)");
  const uintptr_t n = (uintptr_t)d_nxn, nn = (uintptr_t)ctus * 64 * sizeof(fhevc_intra_rd_nxn_node);
  if (d_nxn) {
    // the NxN records are written by other lanes than anything else is read or written by: no extent may touch theirs
    const uintptr_t planes = (uintptr_t)(((long long)(num_frames - 1) * frame_stride_samples + (long long)(c->cfg.height - 1) * stride_samples + c->cfg.width) * sample_bytes);
    const uintptr_t at[4] = { o, f, (uintptr_t)d_rd_merge, (uintptr_t)d_luma }, len[4] = { extent, extent, extent, planes };
    for (int i = 0; i < 4; ++i)
      if (at[i] && at[i] < n + nn && n < at[i] + len[i]) return fail(c, FHEVC_E_INVALID, "bad intra NxN RD-stage arguments (the NxN records overlap another array)");
  }
  // a list is read by every lane of its node through all the positions, an output record is written at the CTU's end: no list may touch an output
  const uintptr_t lists[2] = { (uintptr_t)d_modes, (uintptr_t)d_modes4 };
  const uintptr_t list_len[2] = { (uintptr_t)ctus * FHEVC_NODES * (uintptr_t)list_stride, d_modes4 ? (uintptr_t)ctus * FHEVC_PUS4_PER_CTU * (uintptr_t)list_stride4 : 0 };
  for (int i = 0; i < 2; ++i) {
    if (!lists[i]) continue;
    if ((lists[i] < o + extent && o < lists[i] + list_len[i]) || (d_nxn && lists[i] < n + nn && n < lists[i] + list_len[i]))
      return fail(c, FHEVC_E_INVALID, "bad intra search arguments (a list overlaps an output)");
  }
  if (ctu_row_begin == ctu_row_end) return FHEVC_OK;   // an empty band: nothing to launch, nothing written
  const FhevcFrames fr = frames_of(c, d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, ctu_row_begin, ctu_row_end, qp);
  FhevcIntraSearchRule r;
  static_assert(sizeof(fhevc_intra_search_rule) == 8 && sizeof(FhevcIntraSearchRule) == 8 && offsetof(fhevc_intra_search_rule, count4) == 4 &&
                offsetof(fhevc_intra_search_rule, append_planar) == 5 && offsetof(FhevcIntraSearchRule, append_planar) == 5, "the search rule");
  memcpy(&r, rule, sizeof r);   // by value with the launch: the caller's rule may change once the call has returned
  return launch_on(c, stream, 41, "fhevc_launch_intra_rd_search", [&](hipStream_t s) {
    return fhevc_launch_intra_rd_search(fr, fhevc_rd_quant(qp, c->cfg.bit_depth), d_modes, list_stride, d_modes4, list_stride4, r, kn(d_fold), kn(d_rd_merge), skip_mask, kn(d_out),
                                        kn(d_nxn), c->num_cus, s);
  });
}

int fhevc_intra_rd_search(fhevc_ctx* c, const int16_t* luma, int stride_samples, int qp, const uint8_t* modes, int list_stride, const uint8_t* modes4, int list_stride4,
                          const fhevc_intra_search_rule* rule, const fhevc_motion_rd_pu_node* fold, const fhevc_motion_rd_node* rd_merge, int skip_mask,
                          fhevc_motion_rd_pu_node* out, fhevc_intra_rd_nxn_node* nxn)
{
  const int rc = open_host_form(c, luma && modes && rule && out && skip_mask >= 0 && skip_mask <= 3, stride_samples, qp, 1, 1, "bad intra search arguments");
  if (rc != GO) return rc;
  if (nxn && !modes4) return fail(c, FHEVC_E_INVALID, "bad intra search arguments (the NxN records need the 4x4 PUs' lists)");   // said before anything is staged
  if (const char* bad = intra_search_rule_error(*rule, list_stride, modes4 != nullptr, list_stride4)) return fail(c, FHEVC_E_INVALID, bad);
  HostForm h(c);
  const size_t bn = h.bytes(kNodes), b4 = (size_t)c->num_ctus * FHEVC_PUS4_PER_CTU * sizeof(fhevc_node_cost), bx = (size_t)c->num_ctus * 64 * sizeof(fhevc_intra_rd_nxn_node);
  // the lists lie where fhevc_intra_rd_nxn keeps the first-pass records they stand for: the nodes' in the head of d_first_p, the 4x4 PUs' behind them (8 of the 16 bytes of an entry at the most)
  const size_t ln = (size_t)c->num_ctus * FHEVC_NODES * list_stride, l4 = modes4 ? (size_t)c->num_ctus * FHEVC_PUS4_PER_CTU * list_stride4 : 0;
  const uint8_t *d_modes = h.in(c->d_first_p, bn + b4, modes, ln), *d_modes4 = h.in(c->d_first_p, bn + b4, modes4, l4, bn);
  const fhevc_motion_rd_node* d_rd_merge = h.in(c->d_qpel, bn, rd_merge, bn);
  const fhevc_motion_rd_pu_node* d_fold = h.in(c->d_qpel_pu, h.bytes(kPus), fold, bn);   // folded in place on the device, as fhevc_intra_rd_qt does
  fhevc_motion_rd_pu_node* d_out = h.out(c->d_qpel_pu, h.bytes(kPus), out, bn);
  fhevc_intra_rd_nxn_node* d_nxn = h.out(c->d_intra_p, bn, nxn, bx);                     // 64 records of 16 bytes per CTU: the head of the intra records' buffer
  return h.run(luma, nullptr, stride_samples, [&] {
    return fhevc_intra_rd_search_device(c, c->d_pair + pair_plane(c), 2, c->dev_stride, 0, 1, 0, c->ctus_y, qp, d_modes, list_stride, d_modes4, list_stride4, rule, d_fold, d_rd_merge,
                                        skip_mask, d_out, d_nxn, c->stream);
  });
}

// ---- merge-candidate costs per PU from the refined nodes (k_motion_merge_pu.hip) ----

int fhevc_motion_merge_pu_device(fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                                 int num_frames, int ctu_row_begin, int ctu_row_end, int qp, int max_range, const fhevc_motion_qpel_node* d_refined,
                                 fhevc_motion_merge_node* d_out_pus, fhevc_motion_merge_node* d_out_pus_small, void* stream)
{
  const Batch b{ d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, ctu_row_begin, ctu_row_end, qp };
  // either family may be null, not both
  return device_form(c, d_luma && d_refined && (d_out_pus || d_out_pus_small), "bad PU merge-stage arguments", b, max_range, FHEVC_MOTION_WIDE_MAX_RANGE,
                     "bad PU merge-stage arguments (max_range 1..64)", stream, 21, "fhevc_launch_motion_merge_pu", [&](const FhevcFrames& fr, hipStream_t s) {
    return fhevc_launch_motion_merge_pu(fr, max_range, mv_bit_cost_table(qp), kn(d_refined), kn(d_out_pus), kn(d_out_pus_small), c->num_cus, s);
  }, [&]() -> const char* {
    return (long long)(num_frames - 1) * (ctu_row_end - ctu_row_begin) * c->ctus_x > 0x7FFFFFFFLL ? "more than 2^31 - 1 CTUs" : nullptr;
  });
}

int fhevc_motion_merge_pu(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int max_range,
                          const fhevc_motion_qpel_node* refined, fhevc_motion_merge_node* out_pus, fhevc_motion_merge_node* out_pus_small)
{
  const int rc = open_host_form(c, cur_luma && ref_luma && refined && (out_pus || out_pus_small), stride_samples, qp, max_range, FHEVC_MOTION_WIDE_MAX_RANGE,
                                "bad PU merge-stage arguments");
  if (rc != GO) return rc;
  HostForm h(c);
  const size_t all = h.bytes(kPus) + h.bytes(kSmall);
  const fhevc_motion_qpel_node* d_refined = h.in(c->d_qpel, h.bytes(kNodes), refined, h.bytes(kNodes));
  fhevc_motion_merge_node *d_pus = h.out(c->d_merge_pu, all, out_pus, h.bytes(kPus)), *d_small = h.out(c->d_merge_pu, all, out_pus_small, h.bytes(kSmall), h.bytes(kPus));
  return h.run(cur_luma, ref_luma, stride_samples, [&] { return on_pair(c, fhevc_motion_merge_pu_device, qp, max_range, d_refined, d_pus, d_small, c->stream); });
}

// ---- refined costs re-priced against neighbour predictors (k_motion_amvp.hip) ----

int fhevc_motion_amvp_device(fhevc_ctx* c, int num_frames, int ctu_row_begin, int ctu_row_end, int qp, const fhevc_motion_qpel_node* d_nodes,
                             const fhevc_motion_qpel_node* d_pus, const fhevc_motion_qpel_node* d_pus_small, fhevc_motion_qpel_node* d_out_nodes,
                             fhevc_motion_qpel_node* d_out_pus, fhevc_motion_qpel_node* d_out_pus_small, fhevc_motion_mvp* d_mvp_nodes, fhevc_motion_mvp* d_mvp_pus,
                             fhevc_motion_mvp* d_mvp_pus_small, void* stream)
{
  if (!c) return FHEVC_E_INVALID;
  if (!d_nodes || (!d_out_nodes && !d_out_pus && !d_out_pus_small && !d_mvp_nodes && !d_mvp_pus && !d_mvp_pus_small))
    return fail(c, FHEVC_E_INVALID, "bad re-pricing arguments (the refined nodes and at least one output)");
  if ((!d_pus && (d_out_pus || d_mvp_pus)) || (!d_pus_small && (d_out_pus_small || d_mvp_pus_small)))
    return fail(c, FHEVC_E_INVALID, "bad re-pricing arguments (a family's outputs need that family's input)");
  const uintptr_t all = (uintptr_t)d_nodes | (uintptr_t)d_pus | (uintptr_t)d_pus_small | (uintptr_t)d_out_nodes | (uintptr_t)d_out_pus | (uintptr_t)d_out_pus_small |
                        (uintptr_t)d_mvp_nodes | (uintptr_t)d_mvp_pus | (uintptr_t)d_mvp_pus_small;
  if (all & 3) return fail(c, FHEVC_E_INVALID, "bad re-pricing arguments (records are 4-byte aligned)");
  // (records have no sample layout: the checks of the frames' number, the band and the qp)
  if (const char* bad = batch_error(c, 2, c->cfg.width, 0, num_frames, 2, ctu_row_begin, ctu_row_end, qp, false)) return fail(c, FHEVC_E_INVALID, bad);
  if ((long long)(num_frames - 1) * (ctu_row_end - ctu_row_begin) * c->ctus_x > 0x7FFFFFFFLL) return fail(c, FHEVC_E_INVALID, "more than 2^31 - 1 CTUs");
  if (ctu_row_begin == ctu_row_end) return FHEVC_OK;  // an empty band: nothing to launch, nothing written
  // the 67 bit costs travel with the launch: nothing of the context is read or written by it
  const FhevcFrames fr = frames_of(c, nullptr, 2, c->cfg.width, 0, num_frames - 1, ctu_row_begin, ctu_row_end, qp);
  return launch_on(c, stream, 25, "fhevc_launch_motion_amvp", [&](hipStream_t s) {
    return fhevc_launch_motion_amvp(fr, fhevc_mvp_bit_cost_table(motion_lambda(qp)), kn(d_nodes), kn(d_pus), kn(d_pus_small), kn(d_out_nodes), kn(d_out_pus),
                                    kn(d_out_pus_small), kn(d_mvp_nodes), kn(d_mvp_pus), kn(d_mvp_pus_small), c->num_cus, s);
  });
}

int fhevc_motion_amvp(fhevc_ctx* c, int qp, const fhevc_motion_qpel_node* nodes, const fhevc_motion_qpel_node* pus, const fhevc_motion_qpel_node* pus_small,
                      fhevc_motion_qpel_node* out_nodes, fhevc_motion_qpel_node* out_pus, fhevc_motion_qpel_node* out_pus_small, fhevc_motion_mvp* mvp_nodes,
                      fhevc_motion_mvp* mvp_pus, fhevc_motion_mvp* mvp_pus_small)
{
  if (!c) return FHEVC_E_INVALID;
  if (!nodes || (!out_nodes && !out_pus && !out_pus_small && !mvp_nodes && !mvp_pus && !mvp_pus_small) || qp < 0 || qp > 51)
    return fail(c, FHEVC_E_INVALID, "bad re-pricing arguments (the refined nodes, at least one output, qp 0..51)");
  if ((!pus && (out_pus || mvp_pus)) || (!pus_small && (out_pus_small || mvp_pus_small)))
    return fail(c, FHEVC_E_INVALID, "bad re-pricing arguments (a family's outputs need that family's input)");
  HostForm h(c);
  const size_t bn = h.bytes(kNodes), bp = h.bytes(kPus), bs = h.bytes(kSmall), all = bn + bp + bs;
  const fhevc_motion_qpel_node *d_nodes = h.in(c->d_qpel, bn, nodes, bn), *d_pus = h.in(c->d_qpel_pu, bp, pus, bp), *d_small = h.in(c->d_qpel_pu_small, bs, pus_small, bs);
  fhevc_motion_qpel_node *o_nodes = h.out(c->d_amvp, all, out_nodes, bn), *o_pus = h.out(c->d_amvp, all, out_pus, bp, bn), *o_small = h.out(c->d_amvp, all, out_pus_small, bs, bn + bp);
  fhevc_motion_mvp *m_nodes = h.out(c->d_amvp_mvp, all / 2, mvp_nodes, bn / 2), *m_pus = h.out(c->d_amvp_mvp, all / 2, mvp_pus, bp / 2, bn / 2),
                   *m_small = h.out(c->d_amvp_mvp, all / 2, mvp_pus_small, bs / 2, (bn + bp) / 2);
  return h.run([&] { return fhevc_motion_amvp_device(c, 2, 0, c->ctus_y, qp, d_nodes, d_pus, d_small, o_nodes, o_pus, o_small, m_nodes, m_pus, m_small, c->stream); });
}

// ---- quarter-sample refinement of the PUs' vectors (k_motion_refine_pu.hip) ----

int fhevc_motion_refine_pu_device(fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                                  int num_frames, int ctu_row_begin, int ctu_row_end, int qp, int max_range,
                                  const fhevc_motion_node* d_pus, fhevc_motion_qpel_node* d_out_pus,
                                  const fhevc_motion_node* d_pus_small, fhevc_motion_qpel_node* d_out_pus_small, void* stream)
{
  const Batch b{ d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, ctu_row_begin, ctu_row_end, qp };
  // either family's pair may be null together, not both pairs and not half a pair
  return device_form(c, d_luma && (d_pus || d_pus_small) && !d_pus == !d_out_pus && !d_pus_small == !d_out_pus_small, "bad PU motion-refinement arguments", b, max_range,
                     FHEVC_MOTION_MAX_RANGE, "the PU motion refinement covers vectors of the search ranges 1..8", stream, 10, "fhevc_launch_motion_refine_pu",
                     [&](const FhevcFrames& fr, hipStream_t s) {
    return fhevc_launch_motion_refine_pu(fr, max_range, mv_bit_cost_table(qp), kn(d_pus), kn(d_out_pus), kn(d_pus_small), kn(d_out_pus_small), c->num_cus, false, s);
  });
}

int fhevc_motion_refine_pu(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int max_range,
                           const fhevc_motion_node* pus, fhevc_motion_qpel_node* out_pus, const fhevc_motion_node* pus_small, fhevc_motion_qpel_node* out_pus_small)
{
  const int rc = open_host_form(c, cur_luma && ref_luma && (pus || pus_small) && !pus == !out_pus && !pus_small == !out_pus_small, stride_samples, qp, max_range,
                                FHEVC_MOTION_MAX_RANGE, "bad PU motion-refinement arguments");
  if (rc != GO) return rc;
  HostForm h(c);
  const fhevc_motion_node *d_pus = h.found_in(kPus, pus), *d_small = h.found_in(kSmall, pus_small);
  fhevc_motion_qpel_node *q_pus = h.refined_out(kPus, out_pus), *q_small = h.refined_out(kSmall, out_pus_small);
  return h.run(cur_luma, ref_luma, stride_samples, [&] { return on_pair(c, fhevc_motion_refine_pu_device, qp, max_range, d_pus, q_pus, d_small, q_small, c->stream); });
}

// ---- the two refinements at HM's own SearchRange: what fhevc_motion_search_pu_wide writes feeds straight in (k_motion_refine.hip, k_motion_refine_pu.hip) ----

int fhevc_motion_refine_pu_wide_device(fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                                       int num_frames, int ctu_row_begin, int ctu_row_end, int qp, int max_range,
                                       const fhevc_motion_node* d_nodes, fhevc_motion_qpel_node* d_out_nodes,
                                       const fhevc_motion_node* d_pus, fhevc_motion_qpel_node* d_out_pus,
                                       const fhevc_motion_node* d_pus_small, fhevc_motion_qpel_node* d_out_pus_small, void* stream)
{
  FhevcFrames fr;
  const Batch b{ d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, ctu_row_begin, ctu_row_end, qp };
  // each family's pair may be null together, not all three pairs and not half a pair
  const bool args_ok = d_luma && (d_nodes || d_pus || d_pus_small) && !d_nodes == !d_out_nodes && !d_pus == !d_out_pus && !d_pus_small == !d_out_pus_small;
  const int open = open_device_form(c, args_ok, "bad wide PU motion-refinement arguments", b, max_range, FHEVC_MOTION_WIDE_MAX_RANGE,
                                    "the wide PU motion refinement covers vectors of the search ranges 1..64", &fr);
  if (open != GO) return open;
  // Nothing of the context is read or written by the launches (the 40 bit costs travel by value): calls on different streams may be in flight together.
  // The nodes: the square kernel, the launch of fhevc_motion_refine_device; the PUs: one launch for both families, the MR = 8 layout up to +-8 (the launch
  // of fhevc_motion_refine_pu_device), the MR = 64 layout above.  Each launch is timed and counted under slot 12
  if (d_nodes) {
    const int rc = launch_on(c, stream, 12, "fhevc_motion_refine_pu_wide (nodes)", [&](hipStream_t s) {
      return fhevc_launch_motion_refine(fr, max_range, mv_bit_cost_table(qp), kn(d_nodes), kn(d_out_nodes), c->num_cus, s);
    });
    if (rc != FHEVC_OK) return rc;
  }
  if (!d_pus && !d_pus_small) return FHEVC_OK;
  return launch_on(c, stream, 12, "fhevc_motion_refine_pu_wide (PUs)", [&](hipStream_t s) {
    return fhevc_launch_motion_refine_pu(fr, max_range, mv_bit_cost_table(qp), kn(d_pus), kn(d_out_pus), kn(d_pus_small), kn(d_out_pus_small), c->num_cus,
                                         c->knobs.refine_pu_stage_full, s);
  });
}

int fhevc_motion_refine_pu_wide(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int max_range,
                                const fhevc_motion_node* nodes, fhevc_motion_qpel_node* out_nodes,
                                const fhevc_motion_node* pus, fhevc_motion_qpel_node* out_pus,
                                const fhevc_motion_node* pus_small, fhevc_motion_qpel_node* out_pus_small)
{
  const bool args_ok = cur_luma && ref_luma && (nodes || pus || pus_small) && !nodes == !out_nodes && !pus == !out_pus && !pus_small == !out_pus_small;
  const int rc = open_host_form(c, args_ok, stride_samples, qp, max_range, FHEVC_MOTION_WIDE_MAX_RANGE, "bad wide PU motion-refinement arguments");
  if (rc != GO) return rc;
  HostForm h(c);
  const fhevc_motion_node *d_nodes = h.found_in(kNodes, nodes), *d_pus = h.found_in(kPus, pus), *d_small = h.found_in(kSmall, pus_small);
  fhevc_motion_qpel_node *q_nodes = h.refined_out(kNodes, out_nodes), *q_pus = h.refined_out(kPus, out_pus), *q_small = h.refined_out(kSmall, out_pus_small);
  return h.run(cur_luma, ref_luma, stride_samples,
               [&] { return on_pair(c, fhevc_motion_refine_pu_wide_device, qp, max_range, d_nodes, q_nodes, d_pus, q_pus, d_small, q_small, c->stream); });
}

// ---- the two refinements around one centre per CTU: what fhevc_motion_search_pu_centred writes feeds straight in (k_motion_refine.hip, k_motion_refine_pu.hip, centred) ----

int fhevc_motion_refine_pu_centred_device(fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                                          int num_frames, int ctu_row_begin, int ctu_row_end, int qp, int max_range, const fhevc_motion_node* d_centres,
                                          const fhevc_motion_node* d_nodes, fhevc_motion_qpel_node* d_out_nodes,
                                          const fhevc_motion_node* d_pus, fhevc_motion_qpel_node* d_out_pus,
                                          const fhevc_motion_node* d_pus_small, fhevc_motion_qpel_node* d_out_pus_small, void* stream)
{
  FhevcFrames fr;
  const Batch b{ d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, ctu_row_begin, ctu_row_end, qp };
  const bool args_ok = d_luma && d_centres && (d_nodes || d_pus || d_pus_small) && !d_nodes == !d_out_nodes && !d_pus == !d_out_pus && !d_pus_small == !d_out_pus_small;
  const int open = open_device_form(c, args_ok, "bad centred PU motion-refinement arguments", b, max_range, FHEVC_MOTION_MAX_RANGE,
                                    "the centred PU motion refinement covers max_range 1..8", &fr);
  if (open != GO) return open;
  // the MR = 8 layouts with the window staged around each CTU's centre; one launch for the nodes, one for both PU families, each timed and counted under slot 15
  if (d_nodes) {
    const int rc = launch_on(c, stream, 15, "fhevc_motion_refine_pu_centred (nodes)", [&](hipStream_t s) {
      return fhevc_launch_motion_refine_centred(fr, max_range, mv_bit_cost_table(qp), kn(d_centres), kn(d_nodes), kn(d_out_nodes), c->num_cus, s);
    });
    if (rc != FHEVC_OK) return rc;
  }
  if (!d_pus && !d_pus_small) return FHEVC_OK;
  return launch_on(c, stream, 15, "fhevc_motion_refine_pu_centred (PUs)", [&](hipStream_t s) {
    return fhevc_launch_motion_refine_pu_centred(fr, max_range, mv_bit_cost_table(qp), kn(d_centres), kn(d_pus), kn(d_out_pus), kn(d_pus_small), kn(d_out_pus_small), c->num_cus, s);
  });
}

int fhevc_motion_refine_pu_centred(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int max_range,
                                   const fhevc_motion_node* centres, const fhevc_motion_node* nodes, fhevc_motion_qpel_node* out_nodes,
                                   const fhevc_motion_node* pus, fhevc_motion_qpel_node* out_pus,
                                   const fhevc_motion_node* pus_small, fhevc_motion_qpel_node* out_pus_small)
{
  const bool args_ok = cur_luma && ref_luma && centres && (nodes || pus || pus_small) && !nodes == !out_nodes && !pus == !out_pus && !pus_small == !out_pus_small;
  const int rc = open_host_form(c, args_ok, stride_samples, qp, max_range, FHEVC_MOTION_MAX_RANGE, "bad centred PU motion-refinement arguments");
  if (rc != GO) return rc;
  HostForm h(c);
  const fhevc_motion_node *d_centres = h.found_in(kCentres, centres), *d_nodes = h.found_in(kNodes, nodes), *d_pus = h.found_in(kPus, pus), *d_small = h.found_in(kSmall, pus_small);
  fhevc_motion_qpel_node *q_nodes = h.refined_out(kNodes, out_nodes), *q_pus = h.refined_out(kPus, out_pus), *q_small = h.refined_out(kSmall, out_pus_small);
  return h.run(cur_luma, ref_luma, stride_samples,
               [&] { return on_pair(c, fhevc_motion_refine_pu_centred_device, qp, max_range, d_centres, d_nodes, q_nodes, d_pus, q_pus, d_small, q_small, c->stream); });
}

// measurement tools only (tools/motion_refine_pu_wide_bench.py; not in fasthevc.h): what hipOccupancyMaxActiveBlocksPerMultiprocessor answers for the MR = 64
// instance of k_motion_refine_pu.hip that planes of sample_bytes take on this context, and the cap of its persistent grid
int fhevc_debug_refine_pu_wide_residency(fhevc_ctx* c, int sample_bytes, int* blocks_per_cu, int* grid_cap)
{
  if (!c || !blocks_per_cu || !grid_cap || (sample_bytes != 1 && sample_bytes != 2)) return FHEVC_E_INVALID;
  (void)hipSetDevice(c->device);
  HIP_TRY(c, fhevc_motion_refine_pu_big_residency(sample_bytes, c->cfg.bit_depth, blocks_per_cu));
  *grid_cap = (*blocks_per_cu < 2 ? *blocks_per_cu : 2) * c->num_cus;
  return FHEVC_OK;
}

// measurement tools only (tools/motion_rd_qt_bench.py; not in fasthevc.h): the same answer for an MR = 64 instance of k_motion_rd.hip
int fhevc_debug_motion_rd_wide_residency(fhevc_ctx* c, int sample_bytes, int pu, int tu_depths, int* blocks_per_cu)
{
  if (!c || !blocks_per_cu || (sample_bytes != 1 && sample_bytes != 2) || (tu_depths != 2 && tu_depths != 3)) return FHEVC_E_INVALID;
  (void)hipSetDevice(c->device);
  HIP_TRY(c, fhevc_motion_rd_big_residency(sample_bytes, pu != 0, tu_depths, blocks_per_cu));
  return FHEVC_OK;
}

// ---- P-picture depth ranges over a device-resident batch (k_p_rule.hip; the host form of the rule: fhevc_host.hip) ----
int fhevc_p_depth_range_device(fhevc_ctx* c, const fhevc_motion_node* d_nodes, const uint8_t* d_prev_maps, int num_pictures, int ctu_row_begin,
                               int ctu_row_end, int qp, int prev_mode, const fhevc_p_rule* rule, uint8_t* d_depth_min, uint8_t* d_depth_max, void* stream)
{
  if (!c || !d_nodes || !d_prev_maps || !d_depth_min) return FHEVC_E_INVALID;
  // (nodes and maps have no sample layout: the checks of the pictures' number, the band and the qp)
  if (const char* bad = batch_error(c, 2, c->cfg.width, 0, num_pictures, 1, ctu_row_begin, ctu_row_end, qp, false)) return fail(c, FHEVC_E_INVALID, bad);
  if (prev_mode != FHEVC_P_PREV_COLOCATED && prev_mode != FHEVC_P_PREV_UNIT && prev_mode != FHEVC_P_PREV_NODE)
    return fail(c, FHEVC_E_INVALID, "prev_mode: FHEVC_P_PREV_COLOCATED, FHEVC_P_PREV_UNIT or FHEVC_P_PREV_NODE");
  if ((long long)num_pictures * (ctu_row_end - ctu_row_begin) * c->ctus_x > 0x7FFFFFFFLL) return fail(c, FHEVC_E_INVALID, "bad P-rule arguments");
  if (ctu_row_begin == ctu_row_end) return FHEVC_OK;
  static_assert(sizeof(fhevc_p_rule) == sizeof(FhevcPRule), "P rule layout");
  FhevcPRule r;   // read here, handed to the kernel by value: the caller's struct is free again when this call returns
  if (rule) std::memcpy(&r, rule, sizeof r);
  else { fhevc_p_rule d; fhevc_p_rule_default(&d); std::memcpy(&r, &d, sizeof r); }
  const FhevcFrames fr = frames_of(c, nullptr, 1, c->cfg.width, 0, num_pictures, ctu_row_begin, ctu_row_end, qp);
  return launch_on(c, stream, 5, "fhevc_launch_p_rule", [&](hipStream_t s) {
    return fhevc_launch_p_rule(fr, prev_mode, r, kn(d_nodes), d_prev_maps, d_depth_min, d_depth_max, c->num_cus, s);
  });
}

int fhevc_p_predict_frame(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range,
                          const uint8_t* prev_map, int prev_mode, const fhevc_p_rule* rule, uint8_t* depth_min, uint8_t* depth_max)
{
  if (!c || !cur_luma || !ref_luma || !prev_map || !depth_min || !depth_max || stride_samples < c->cfg.width) return FHEVC_E_INVALID;
  if (prev_mode != FHEVC_P_PREV_COLOCATED && prev_mode != FHEVC_P_PREV_UNIT && prev_mode != FHEVC_P_PREV_NODE)
    return fail(c, FHEVC_E_INVALID, "prev_mode: FHEVC_P_PREV_COLOCATED, FHEVC_P_PREV_UNIT or FHEVC_P_PREV_NODE");
  HostForm h(c);
  const size_t map = (size_t)c->num_ctus * 256;
  const uint8_t* d_prev = h.in(c->d_p_maps, 3 * map, prev_map, map);
  uint8_t *d_min = h.out(c->d_p_maps, 3 * map, depth_min, map, map), *d_max = h.out(c->d_p_maps, 3 * map, depth_max, map, 2 * map);
  fhevc_motion_node* d_nodes = h.found(kNodes);
  return h.run(cur_luma, ref_luma, stride_samples, [&] {
    const int rc = on_pair(c, fhevc_motion_search_device, qp, search_range, d_nodes, c->stream);
    return rc != FHEVC_OK ? rc : fhevc_p_depth_range_device(c, d_nodes, d_prev, 1, 0, c->ctus_y, qp, prev_mode, rule, d_min, d_max, c->stream);
  });
}

// ---- partition sizes per CU from the refined PU costs over a device-resident batch (k_pu_shape.hip; the host form: fhevc_host.hip) ----
// d_merge_pus: null for fhevc_pu_shape_select_device; with_merge says which of the two entry points is asking
static int pu_shape_select_on(fhevc_ctx* c, const fhevc_motion_qpel_node* d_nodes, const fhevc_motion_qpel_node* d_pus, const fhevc_motion_qpel_node* d_pus_small,
                              const fhevc_motion_merge_node* d_merge_pus, const fhevc_motion_merge_node* d_merge_pus_small, bool with_merge, int num_pictures,
                              int ctu_row_begin, int ctu_row_end, const fhevc_pu_shape_rule* rule, fhevc_pu_shape_node* d_shapes, uint32_t* d_costs, uint16_t* d_merged,
                              void* stream)
{
  if (!c) return FHEVC_E_INVALID;
  if (!d_nodes || !d_pus || !d_shapes || (with_merge && !d_merge_pus)) return fail(c, FHEVC_E_INVALID, "bad partition-size selection arguments");
  // (refined entries have no sample layout: the checks of the pictures' number and the band)
  if (const char* bad = batch_error(c, 2, c->cfg.width, 0, num_pictures, 1, ctu_row_begin, ctu_row_end, 0, false)) return fail(c, FHEVC_E_INVALID, bad);
  static_assert(sizeof(fhevc_pu_shape_rule) == sizeof(FhevcPuShapeRule), "partition-size rule layout");
  FhevcPuShapeRule r;   // read here, handed to the kernel by value: the caller's struct is free again when this call returns
  if (rule) std::memcpy(&r, rule, sizeof r);
  else { fhevc_pu_shape_rule d; fhevc_pu_shape_rule_default(&d); std::memcpy(&r, &d, sizeof r); }
  if (const char* bad = fhevc_pu_shape_rule_error(r)) return fail(c, FHEVC_E_INVALID, bad);
  if ((long long)num_pictures * (ctu_row_end - ctu_row_begin) * c->ctus_x > 0x7FFFFFFFLL) return fail(c, FHEVC_E_INVALID, "more than 2^31 - 1 CTUs");
  if (ctu_row_begin == ctu_row_end) return FHEVC_OK;  // an empty band: nothing to launch, nothing written
  const FhevcFrames fr = frames_of(c, nullptr, 1, c->cfg.width, 0, num_pictures, ctu_row_begin, ctu_row_end);
  if (with_merge)
    return launch_on(c, stream, 13, "fhevc_launch_pu_shape_merge", [&](hipStream_t s) {
      return fhevc_launch_pu_shape_merge(fr, r, kn(d_nodes), kn(d_pus), kn(d_pus_small), kn(d_merge_pus), kn(d_merge_pus_small), kn(d_shapes), d_costs, d_merged, c->num_cus, s);
    });
  return launch_on(c, stream, 13, "fhevc_launch_pu_shape", [&](hipStream_t s) {
    return fhevc_launch_pu_shape(fr, r, kn(d_nodes), kn(d_pus), kn(d_pus_small), kn(d_shapes), d_costs, c->num_cus, s);
  });
}

int fhevc_pu_shape_select_device(fhevc_ctx* c, const fhevc_motion_qpel_node* d_nodes, const fhevc_motion_qpel_node* d_pus, const fhevc_motion_qpel_node* d_pus_small,
                                 int num_pictures, int ctu_row_begin, int ctu_row_end, const fhevc_pu_shape_rule* rule, fhevc_pu_shape_node* d_shapes,
                                 uint32_t* d_costs, void* stream)
{
  return pu_shape_select_on(c, d_nodes, d_pus, d_pus_small, nullptr, nullptr, false, num_pictures, ctu_row_begin, ctu_row_end, rule, d_shapes, d_costs, nullptr, stream);
}

int fhevc_pu_shape_select_merge_device(fhevc_ctx* c, const fhevc_motion_qpel_node* d_nodes, const fhevc_motion_qpel_node* d_pus, const fhevc_motion_qpel_node* d_pus_small,
                                       const fhevc_motion_merge_node* d_merge_pus, const fhevc_motion_merge_node* d_merge_pus_small, int num_pictures, int ctu_row_begin,
                                       int ctu_row_end, const fhevc_pu_shape_rule* rule, fhevc_pu_shape_node* d_shapes, uint32_t* d_costs, uint16_t* d_merged, void* stream)
{
  return pu_shape_select_on(c, d_nodes, d_pus, d_pus_small, d_merge_pus, d_merge_pus_small, true, num_pictures, ctu_row_begin, ctu_row_end, rule, d_shapes, d_costs, d_merged,
                            stream);
}

int fhevc_p_shape_frame(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range,
                        const fhevc_pu_shape_rule* rule, fhevc_pu_shape_node* shapes)
{
  const int open = open_host_form(c, cur_luma && ref_luma && shapes, stride_samples, qp, search_range, FHEVC_MOTION_WIDE_MAX_RANGE, "bad partition-size frame arguments");
  if (open != GO) return open;
  if (rule)
    if (const char* bad = fhevc_pu_shape_rule_error(*rule)) return fail(c, FHEVC_E_INVALID, bad);
  HostForm h(c);
  const Chain k = claim_chain(h, false);
  fhevc_pu_shape_node* d_shapes = h.out(c->d_motion, h.bytes(kNodes), shapes, h.bytes(kNodes));
  return h.run(cur_luma, ref_luma, stride_samples, [&] {
    const int rc = queue_chain(c, qp, search_range, 0, k);
    return rc != FHEVC_OK ? rc : fhevc_pu_shape_select_device(c, k.q_nodes, k.q_pus, k.q_small, 1, 0, c->ctus_y, rule, d_shapes, nullptr, c->stream);
  });
}

// ---- P-picture depth ranges from the selection's records over a device-resident batch (k_p_tree.hip; the host form: fhevc_host.hip) ----
// d_merge: null for fhevc_p_tree_select_device; with_merge / with_skip say which of the three entry points is asking (the skip variant takes the merge records too)
static int p_tree_select_on(fhevc_ctx* c, const fhevc_pu_shape_node* d_shapes, const fhevc_motion_merge_node* d_merge, bool with_merge, int num_pictures, int ctu_row_begin,
                            int ctu_row_end, const fhevc_p_tree_rule* rule, uint8_t* d_depth_min, uint8_t* d_depth_max, fhevc_p_tree_node* d_tree, void* stream,
                            bool with_skip = false, const fhevc_motion_skip_node* d_skip = nullptr, int skip_mask = 0, bool with_intra = false,
                            const fhevc_intra_p_node* d_intra = nullptr)
{
  if (!c) return FHEVC_E_INVALID;
  if (!d_shapes || (with_merge && !d_merge) || (!d_depth_min && !d_depth_max && !d_tree)) return fail(c, FHEVC_E_INVALID, "bad tree-decision arguments");
  if (with_skip && (!d_skip || skip_mask < 0 || skip_mask > 3)) return fail(c, FHEVC_E_INVALID, "bad tree-decision arguments (skip records, skip_mask 0..3)");
  if (with_intra && !d_intra) return fail(c, FHEVC_E_INVALID, "bad tree-decision arguments (intra records)");
  // (the older entry points read their records as dwords without asking; this one says what it wants)
  if (with_intra && (((uintptr_t)d_shapes | (uintptr_t)d_merge | (uintptr_t)d_skip | (uintptr_t)d_intra | (uintptr_t)d_tree) & 3))
    return fail(c, FHEVC_E_INVALID, "bad tree-decision arguments (records are 4-byte aligned)");
  // (records have no sample layout: the checks of the pictures' number and the band)
  if (const char* bad = batch_error(c, 2, c->cfg.width, 0, num_pictures, 1, ctu_row_begin, ctu_row_end, 0, false)) return fail(c, FHEVC_E_INVALID, bad);
  static_assert(sizeof(fhevc_p_tree_rule) == sizeof(FhevcPTreeRule) && sizeof(fhevc_p_tree_node) == sizeof(FhevcPTreeNode), "tree-decision layouts");
  FhevcPTreeRule r;   // read here, handed to the kernel by value: the caller's struct is free again when this call returns
  if (rule) std::memcpy(&r, rule, sizeof r);
  else std::memset(&r, 0, sizeof r);   // fhevc_p_tree_rule_default
  if (const char* bad = fhevc_p_tree_rule_error(r)) return fail(c, FHEVC_E_INVALID, bad);
  if ((long long)num_pictures * (ctu_row_end - ctu_row_begin) * c->ctus_x > 0x7FFFFFFFLL) return fail(c, FHEVC_E_INVALID, "more than 2^31 - 1 CTUs");
  if (ctu_row_begin == ctu_row_end) return FHEVC_OK;  // an empty band: nothing to launch, nothing written
  const FhevcFrames fr = frames_of(c, nullptr, 1, c->cfg.width, 0, num_pictures, ctu_row_begin, ctu_row_end);
  if (with_intra)
    return launch_on(c, stream, 17, "fhevc_launch_p_tree_intra", [&](hipStream_t s) {
      return fhevc_launch_p_tree_intra(fr, r, kn(d_shapes), kn(d_merge), kn(d_skip), skip_mask, kn(d_intra), d_depth_min, d_depth_max, kn(d_tree), c->num_cus, s);
    });
  if (with_skip)
    return launch_on(c, stream, 17, "fhevc_launch_p_tree_skip", [&](hipStream_t s) {
      return fhevc_launch_p_tree_skip(fr, r, kn(d_shapes), kn(d_merge), kn(d_skip), skip_mask, d_depth_min, d_depth_max, kn(d_tree), c->num_cus, s);
    });
  if (with_merge)
    return launch_on(c, stream, 17, "fhevc_launch_p_tree_merge", [&](hipStream_t s) {
      return fhevc_launch_p_tree_merge(fr, r, kn(d_shapes), kn(d_merge), d_depth_min, d_depth_max, kn(d_tree), c->num_cus, s);
    });
  return launch_on(c, stream, 17, "fhevc_launch_p_tree", [&](hipStream_t s) {
    return fhevc_launch_p_tree(fr, r, kn(d_shapes), d_depth_min, d_depth_max, kn(d_tree), c->num_cus, s);
  });
}

int fhevc_p_tree_select_device(fhevc_ctx* c, const fhevc_pu_shape_node* d_shapes, int num_pictures, int ctu_row_begin, int ctu_row_end, const fhevc_p_tree_rule* rule,
                               uint8_t* d_depth_min, uint8_t* d_depth_max, fhevc_p_tree_node* d_tree, void* stream)
{
  return p_tree_select_on(c, d_shapes, nullptr, false, num_pictures, ctu_row_begin, ctu_row_end, rule, d_depth_min, d_depth_max, d_tree, stream);
}

int fhevc_p_tree_select_merge_device(fhevc_ctx* c, const fhevc_pu_shape_node* d_shapes, const fhevc_motion_merge_node* d_merge, int num_pictures, int ctu_row_begin,
                                     int ctu_row_end, const fhevc_p_tree_rule* rule, uint8_t* d_depth_min, uint8_t* d_depth_max, fhevc_p_tree_node* d_tree, void* stream)
{
  return p_tree_select_on(c, d_shapes, d_merge, true, num_pictures, ctu_row_begin, ctu_row_end, rule, d_depth_min, d_depth_max, d_tree, stream);
}

int fhevc_p_tree_select_skip_device(fhevc_ctx* c, const fhevc_pu_shape_node* d_shapes, const fhevc_motion_merge_node* d_merge, const fhevc_motion_skip_node* d_skip,
                                    int skip_mask, int num_pictures, int ctu_row_begin, int ctu_row_end, const fhevc_p_tree_rule* rule, uint8_t* d_depth_min,
                                    uint8_t* d_depth_max, fhevc_p_tree_node* d_tree, void* stream)
{
  return p_tree_select_on(c, d_shapes, d_merge, true, num_pictures, ctu_row_begin, ctu_row_end, rule, d_depth_min, d_depth_max, d_tree, stream, true, d_skip, skip_mask);
}

// the skip tree on RD records: cost_rd lies where the selection and the merge records keep cost_best, flags where the skip record keeps flags
int fhevc_p_tree_select_rd_device(fhevc_ctx* c, const fhevc_motion_rd_node* d_rd_explicit, const fhevc_motion_rd_node* d_rd_merge, int skip_mask, int num_pictures,
                                  int ctu_row_begin, int ctu_row_end, const fhevc_p_tree_rule* rule, uint8_t* d_depth_min, uint8_t* d_depth_max, fhevc_p_tree_node* d_tree,
                                  void* stream)
{
  return fhevc_p_tree_select_skip_device(c, reinterpret_cast<const fhevc_pu_shape_node*>(d_rd_explicit), reinterpret_cast<const fhevc_motion_merge_node*>(d_rd_merge),
                                         reinterpret_cast<const fhevc_motion_skip_node*>(d_rd_merge), skip_mask, num_pictures, ctu_row_begin, ctu_row_end, rule,
                                         d_depth_min, d_depth_max, d_tree, stream);
}

// ... and on folded records of fhevc_motion_rd_pu*: bytes 0..11 are the RD record's
int fhevc_p_tree_select_rd_pu_device(fhevc_ctx* c, const fhevc_motion_rd_pu_node* d_rd_pu, const fhevc_motion_rd_node* d_rd_merge, int skip_mask, int num_pictures,
                                     int ctu_row_begin, int ctu_row_end, const fhevc_p_tree_rule* rule, uint8_t* d_depth_min, uint8_t* d_depth_max, fhevc_p_tree_node* d_tree,
                                     void* stream)
{
  return fhevc_p_tree_select_rd_device(c, reinterpret_cast<const fhevc_motion_rd_node*>(d_rd_pu), d_rd_merge, skip_mask, num_pictures, ctu_row_begin, ctu_row_end, rule,
                                       d_depth_min, d_depth_max, d_tree, stream);
}

int fhevc_p_tree_select_intra_device(fhevc_ctx* c, const fhevc_pu_shape_node* d_shapes, const fhevc_motion_merge_node* d_merge, const fhevc_motion_skip_node* d_skip,
                                     int skip_mask, const fhevc_intra_p_node* d_intra, int num_pictures, int ctu_row_begin, int ctu_row_end, const fhevc_p_tree_rule* rule,
                                     uint8_t* d_depth_min, uint8_t* d_depth_max, fhevc_p_tree_node* d_tree, void* stream)
{
  return p_tree_select_on(c, d_shapes, d_merge, true, num_pictures, ctu_row_begin, ctu_row_end, rule, d_depth_min, d_depth_max, d_tree, stream, true, d_skip, skip_mask, true,
                          d_intra);
}

// ---- intra candidate costs per CU node for P pictures, from the first passes' records (k_intra_p.hip; the host twin: fhevc_host.hip) ----

int fhevc_intra_p_device(fhevc_ctx* c, int num_pictures, int ctu_row_begin, int ctu_row_end, int qp, const fhevc_node_cost* d_first, const fhevc_node_cost* d_first4,
                         fhevc_intra_p_node* d_out, void* stream)
{
  if (!c) return FHEVC_E_INVALID;
  if (!d_first || !d_out) return fail(c, FHEVC_E_INVALID, "bad intra-stage arguments (the first-pass records and the output)");
  if (((uintptr_t)d_first | (uintptr_t)d_first4 | (uintptr_t)d_out) & 3) return fail(c, FHEVC_E_INVALID, "bad intra-stage arguments (records are 4-byte aligned)");
  // (records have no sample layout: the checks of the pictures' number, the band and the qp)
  if (const char* bad = batch_error(c, 2, c->cfg.width, 0, num_pictures, 1, ctu_row_begin, ctu_row_end, qp, false)) return fail(c, FHEVC_E_INVALID, bad);
  if ((long long)num_pictures * (ctu_row_end - ctu_row_begin) * c->ctus_x > 0x7FFFFFFFLL) return fail(c, FHEVC_E_INVALID, "more than 2^31 - 1 CTUs");
  if (ctu_row_begin == ctu_row_end) return FHEVC_OK;  // an empty band: nothing to launch, nothing written
  // the three bit costs travel with the launch: nothing of the context is read or written by it
  const FhevcFrames fr = frames_of(c, nullptr, 2, c->cfg.width, 0, num_pictures, ctu_row_begin, ctu_row_end, qp);
  return launch_on(c, stream, 27, "fhevc_launch_intra_p", [&](hipStream_t s) {
    return fhevc_launch_intra_p(fr, fhevc_intra_bit_cost(motion_lambda(qp)), reinterpret_cast<const uint32_t*>(d_first), reinterpret_cast<const uint32_t*>(d_first4),
                                kn(d_out), c->num_cus, s);
  });
}

int fhevc_intra_p(fhevc_ctx* c, int qp, const fhevc_node_cost* first, const fhevc_node_cost* first4, fhevc_intra_p_node* out)
{
  if (!c) return FHEVC_E_INVALID;
  if (!first || !out || qp < 0 || qp > 51) return fail(c, FHEVC_E_INVALID, "bad intra-stage arguments (the first-pass records, the output, qp 0..51)");
  HostForm h(c);
  const size_t bn = h.bytes(kNodes), b4 = (size_t)c->num_ctus * FHEVC_PUS4_PER_CTU * sizeof(fhevc_node_cost);
  const fhevc_node_cost *d_first = h.in(c->d_first_p, bn + b4, first, bn), *d_first4 = h.in(c->d_first_p, bn + b4, first4, b4, bn);
  fhevc_intra_p_node* d_out = h.out(c->d_intra_p, bn, out, bn);
  return h.run([&] { return fhevc_intra_p_device(c, 1, 0, c->ctus_y, qp, d_first, d_first4, d_out, c->stream); });
}

// with_merge: fhevc_p_tree_merge_frame -- the merge stage between refinement and tree; with_merge_pu: fhevc_p_tree_merge_pu_frame -- behind it the merge stage
// per PU, and the selection that takes its costs; with_amvp: fhevc_p_tree_amvp_frame -- the re-pricing behind the refinements, and every later stage on its records;
// with_intra: fhevc_p_tree_intra_frame -- behind the selection the zero-residual stage, the two first passes of the current picture and the intra stage, and the
// tree that takes all of it; with_rd: fhevc_p_tree_rd_frame -- the re-pricing keeps its predictor records, and behind the selection come the RD estimate of the
// nodes' merge records, the RD estimates of 2Nx2N and of the selection's best and second size folded into one record per node, and the RD tree
// (fhevc_p_tree_rd_intra_frame: intra -- behind the folded inter records the first pass of the current picture and the RD estimate of its winners, gated and
// folded in place)
// (fhevc_p_tree_rd_intra_nxn_frame: nxn -- behind the first pass the 4x4 first pass of the current picture, best records only, and the intra stage with the NxN candidate
// of the 8x8 nodes in the intra stage's place; nxn_out: where its NxN records go, or null)
// (fhevc_p_tree_rd_intra_search_frame: search, with nxn -- both first passes give their lists at 8 candidates, into the dead 4x4 records' place behind the nodes'
// records, and the search stage under that rule stands in the NxN stage's place)
struct RdFrameOut { fhevc_motion_rd_node* rd_merge; fhevc_motion_rd_pu_node* rd_pu; bool intra; fhevc_node_cost* first; int tu_depths = 2; bool nxn = false;
                    fhevc_intra_rd_nxn_node* nxn_out = nullptr; const fhevc_intra_search_rule* search = nullptr; };
static int p_tree_frame_on(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range, int coarse_range,
                           const fhevc_pu_shape_rule* shape_rule, const fhevc_p_tree_rule* tree_rule, uint8_t* depth_min, uint8_t* depth_max, fhevc_pu_shape_node* shapes,
                           bool with_merge, fhevc_motion_merge_node* merge, bool with_merge_pu = false, bool with_amvp = false, bool with_intra = false, int skip_mask = 0,
                           fhevc_intra_p_node* intra = nullptr, const RdFrameOut* with_rd = nullptr)
{
  if (!c) return FHEVC_E_INVALID;
  if (!cur_luma || !ref_luma || !depth_min || !depth_max || stride_samples < c->cfg.width) return fail(c, FHEVC_E_INVALID, "bad tree-decision frame arguments");
  if (qp < 0 || qp > 51 || coarse_range < 0 || coarse_range > FHEVC_MOTION_COARSE_MAX_RANGE || search_range < 1 ||
      search_range > (coarse_range ? FHEVC_MOTION_MAX_RANGE : FHEVC_MOTION_WIDE_MAX_RANGE))
    return fail(c, FHEVC_E_INVALID, "bad tree-decision frame arguments (around a centre the search covers ranges 1..8, coarse ranges 1..14)");
  if (shape_rule)
    if (const char* bad = fhevc_pu_shape_rule_error(*shape_rule)) return fail(c, FHEVC_E_INVALID, bad);
  if (tree_rule)
    if (const char* bad = fhevc_p_tree_rule_error(*tree_rule)) return fail(c, FHEVC_E_INVALID, bad);
  if ((with_intra || with_rd) && (skip_mask < 0 || skip_mask > 3)) return fail(c, FHEVC_E_INVALID, "bad tree-decision frame arguments (skip_mask 0..3)");
  if (with_rd && with_rd->tu_depths != 2 && with_rd->tu_depths != 3) return fail(c, FHEVC_E_INVALID, kBadTuDepths);
  if (with_rd && with_rd->search)
    if (const char* bad = intra_search_rule_error(*with_rd->search, 8, true, 8)) return fail(c, FHEVC_E_INVALID, bad);
  HostForm h(c);
  const size_t map = (size_t)c->num_ctus * 256, records = h.bytes(kNodes);
  Chain k = claim_chain(h, coarse_range != 0);
  uint8_t *d_min = h.out(c->d_p_maps, 3 * map, depth_min, map, map), *d_max = h.out(c->d_p_maps, 3 * map, depth_max, map, 2 * map);
  fhevc_pu_shape_node* d_shapes = h.dev<fhevc_pu_shape_node>(c->d_motion, records);
  fhevc_motion_merge_node* d_merge = h.dev<fhevc_motion_merge_node>(c->d_motion_pu, h.bytes(kPus));
  h.out(c->d_motion, records, shapes, records);
  if (with_merge) h.out(c->d_motion_pu, h.bytes(kPus), merge, records);
  fhevc_motion_merge_node *d_merge_pus = nullptr, *d_merge_small = nullptr;
  if (with_merge_pu) {
    d_merge_pus = h.dev<fhevc_motion_merge_node>(c->d_merge_pu, h.bytes(kPus) + h.bytes(kSmall));
    d_merge_small = h.dev<fhevc_motion_merge_node>(c->d_merge_pu, h.bytes(kPus) + h.bytes(kSmall), h.bytes(kPus));
  }
  if (with_amvp) {
    const size_t all = h.bytes(kNodes) + h.bytes(kPus) + h.bytes(kSmall);
    fhevc_motion_qpel_node* const d_priced = h.dev<fhevc_motion_qpel_node>(c->d_amvp, all);
    k.q_nodes_out = d_priced; k.q_pus_out = d_priced + (size_t)c->num_ctus * FHEVC_NODES; k.q_small_out = k.q_pus_out + (size_t)c->num_ctus * FHEVC_PUS;
  }
  fhevc_motion_mvp *d_mvp_nodes = nullptr, *d_mvp_pus = nullptr, *d_mvp_small = nullptr;
  fhevc_motion_rd_node* d_rd_merge = nullptr;
  fhevc_motion_rd_pu_node* d_rd_pu = nullptr;
  if (with_rd) {
    const size_t all = h.bytes(kNodes) + h.bytes(kPus) + h.bytes(kSmall);
    d_mvp_nodes = h.dev<fhevc_motion_mvp>(c->d_amvp_mvp, all / 2);
    d_mvp_pus = d_mvp_nodes + (size_t)c->num_ctus * FHEVC_NODES; d_mvp_small = d_mvp_pus + (size_t)c->num_ctus * FHEVC_PUS;
    d_rd_merge = h.dev<fhevc_motion_rd_node>(c->d_qpel, records);              // the refined nodes and PUs are dead once the re-pricing has read them
    d_rd_pu = h.dev<fhevc_motion_rd_pu_node>(c->d_qpel_pu, h.bytes(kPus));
    h.out(c->d_qpel, records, with_rd->rd_merge, records);
    h.out(c->d_qpel_pu, h.bytes(kPus), with_rd->rd_pu, records);
  }
  fhevc_node_cost* d_first_rd = nullptr;
  if (with_rd && with_rd->intra) {
    const size_t b4 = (size_t)c->num_ctus * FHEVC_PUS4_PER_CTU * sizeof(fhevc_node_cost);
    d_first_rd = h.dev<fhevc_node_cost>(c->d_first_p, records + b4);
    h.out(c->d_first_p, records + b4, with_rd->first, records);
  }
  fhevc_node_cost* d_first4_rd = nullptr;
  fhevc_intra_rd_nxn_node* d_nxn = nullptr;
  if (with_rd && with_rd->intra && with_rd->nxn) {
    const size_t b4 = (size_t)c->num_ctus * FHEVC_PUS4_PER_CTU * sizeof(fhevc_node_cost);
    d_first4_rd = h.dev<fhevc_node_cost>(c->d_first_p, records + b4, records);   // the 4x4 records behind the nodes', where fhevc_p_tree_intra_frame keeps them
    d_nxn = h.out(c->d_intra_p, records, with_rd->nxn_out, (size_t)c->num_ctus * 64 * sizeof(fhevc_intra_rd_nxn_node));   // the head of the intra records' buffer, unused in this chain
  }
  fhevc_motion_skip_node* d_skip = nullptr;
  fhevc_node_cost *d_first = nullptr, *d_first4 = nullptr;
  fhevc_intra_p_node* d_intra = nullptr;
  if (with_intra) {
    const size_t b4 = (size_t)c->num_ctus * FHEVC_PUS4_PER_CTU * sizeof(fhevc_node_cost);
    d_skip = h.dev<fhevc_motion_skip_node>(c->d_qpel, records);   // the refined nodes are dead once the re-pricing has read them
    d_first = h.dev<fhevc_node_cost>(c->d_first_p, records + b4);
    d_first4 = h.dev<fhevc_node_cost>(c->d_first_p, records + b4, records);
    d_intra = h.dev<fhevc_intra_p_node>(c->d_intra_p, records);
    h.out(c->d_intra_p, records, intra, records);
  }
  return h.run(cur_luma, ref_luma, stride_samples, [&] {
    int rc = queue_chain(c, qp, search_range, coarse_range, k);
    if (rc == FHEVC_OK && with_amvp) {
      rc = fhevc_motion_amvp_device(c, 2, 0, c->ctus_y, qp, k.q_nodes, k.q_pus, k.q_small, k.q_nodes_out, k.q_pus_out, k.q_small_out, d_mvp_nodes, d_mvp_pus, d_mvp_small, c->stream);
      k.q_nodes = k.q_nodes_out; k.q_pus = k.q_pus_out; k.q_small = k.q_small_out;   // what every later stage reads
    }
    // absolute vectors of the centred chain reach +-64 and neighbouring CTUs have different centres: the merge stages look around zero at the full range there
    const int merge_range = coarse_range ? FHEVC_MOTION_WIDE_MAX_RANGE : search_range;
    if (rc == FHEVC_OK && with_merge) rc = on_pair(c, fhevc_motion_merge_device, qp, merge_range, k.q_nodes, d_merge, c->stream);
    if (rc == FHEVC_OK && with_merge_pu) rc = on_pair(c, fhevc_motion_merge_pu_device, qp, merge_range, k.q_nodes, d_merge_pus, d_merge_small, c->stream);
    if (rc == FHEVC_OK && with_merge_pu)
      rc = fhevc_pu_shape_select_merge_device(c, k.q_nodes, k.q_pus, k.q_small, d_merge_pus, d_merge_small, 1, 0, c->ctus_y, shape_rule, d_shapes, nullptr, nullptr, c->stream);
    else if (rc == FHEVC_OK) rc = fhevc_pu_shape_select_device(c, k.q_nodes, k.q_pus, k.q_small, 1, 0, c->ctus_y, shape_rule, d_shapes, nullptr, c->stream);
    if (rc == FHEVC_OK && with_rd) {
      const int tud = with_rd->tu_depths;   // all four RD launches at one depth count: both sides of every comparison of the tree on one footing
      rc = on_pair(c, fhevc_motion_rd_qt_device, qp, merge_range, FHEVC_RD_SOURCE_MERGE, static_cast<const void*>(d_merge), static_cast<const fhevc_motion_mvp*>(nullptr), tud,
                   d_rd_merge, c->stream);
      // 2Nx2N first, then the selection's best and its second size: the earlier record stays on a tie, as xCheckBestMode keeps the earlier mode
      fhevc_motion_rd_pu_inputs in = { k.q_nodes, k.q_pus, k.q_small, d_merge_pus, d_merge_small, d_mvp_nodes, d_mvp_pus, d_mvp_small, d_shapes, nullptr };
      if (rc == FHEVC_OK) rc = on_pair(c, fhevc_motion_rd_pu_qt_device, qp, merge_range, 0, &in, tud, d_rd_pu, c->stream);
      in.fold = d_rd_pu;
      if (rc == FHEVC_OK) rc = on_pair(c, fhevc_motion_rd_pu_qt_device, qp, merge_range, 8, &in, tud, d_rd_pu, c->stream);
      if (rc == FHEVC_OK) rc = on_pair(c, fhevc_motion_rd_pu_qt_device, qp, merge_range, 9, &in, tud, d_rd_pu, c->stream);
      if (rc == FHEVC_OK && with_rd->intra) {
        const int16_t* d_cur = c->d_pair + pair_plane(c);   // the current picture of the staged pair, as a batch of one frame
        rc = fhevc_intra_first_pass_device(c, d_cur, 2, c->dev_stride, 0, 1, 0, c->ctus_y, qp, d_first_rd, c->stream);
        // intra last, as HM tries it after the inter sizes: the earlier record stays on a tie
        if (rc == FHEVC_OK && with_rd->search) {
          // the lists lie in the 4x4 records' place, which this chain leaves dead: the nodes' (680 B per CTU) and behind them the 4x4 PUs' (2 048 of the 4 096)
          uint8_t* const d_lists = reinterpret_cast<uint8_t*>(d_first4_rd);
          uint8_t* const d_lists4 = d_lists + (size_t)c->num_ctus * FHEVC_NODES * 8;
          rc = fhevc_intra_first_pass_candidates_device(c, d_cur, 2, c->dev_stride, 0, 1, 0, c->ctus_y, qp, 8, d_lists, c->stream);
          if (rc == FHEVC_OK) rc = fhevc_intra_first_pass_4x4_device(c, d_cur, 2, c->dev_stride, 0, 1, 0, c->ctus_y, qp, 8, nullptr, d_lists4, c->stream);
          if (rc == FHEVC_OK) rc = fhevc_intra_rd_search_device(c, d_cur, 2, c->dev_stride, 0, 1, 0, c->ctus_y, qp, d_lists, 8, d_lists4, 8, with_rd->search, d_rd_pu, d_rd_merge, skip_mask, d_rd_pu, d_nxn, c->stream);
        } else
        if (rc == FHEVC_OK && with_rd->nxn) {
          rc = fhevc_intra_first_pass_4x4_device(c, d_cur, 2, c->dev_stride, 0, 1, 0, c->ctus_y, qp, 0, d_first4_rd, nullptr, c->stream);
          if (rc == FHEVC_OK) rc = fhevc_intra_rd_nxn_device(c, d_cur, 2, c->dev_stride, 0, 1, 0, c->ctus_y, qp, d_first_rd, d_first4_rd, d_rd_pu, d_rd_merge, skip_mask, d_rd_pu, d_nxn, c->stream);
        } else
        if (rc == FHEVC_OK) rc = fhevc_intra_rd_qt_device(c, d_cur, 2, c->dev_stride, 0, 1, 0, c->ctus_y, qp, d_first_rd, d_rd_pu, d_rd_merge, skip_mask, tud, d_rd_pu, c->stream);
      }
      return rc != FHEVC_OK ? rc : fhevc_p_tree_select_rd_pu_device(c, d_rd_pu, d_rd_merge, skip_mask, 1, 0, c->ctus_y, tree_rule, d_min, d_max, nullptr, c->stream);
    }
    if (rc == FHEVC_OK && with_intra) {
      const int16_t* d_cur = c->d_pair + pair_plane(c);   // the current picture of the staged pair, as a batch of one frame
      rc = on_pair(c, fhevc_motion_skip_device, qp, merge_range, d_merge, d_skip, c->stream);
      if (rc == FHEVC_OK) rc = fhevc_intra_first_pass_device(c, d_cur, 2, c->dev_stride, 0, 1, 0, c->ctus_y, qp, d_first, c->stream);
      if (rc == FHEVC_OK) rc = fhevc_intra_first_pass_4x4_device(c, d_cur, 2, c->dev_stride, 0, 1, 0, c->ctus_y, qp, 0, d_first4, nullptr, c->stream);
      if (rc == FHEVC_OK) rc = fhevc_intra_p_device(c, 1, 0, c->ctus_y, qp, d_first, d_first4, d_intra, c->stream);
      return rc != FHEVC_OK ? rc : p_tree_select_on(c, d_shapes, d_merge, true, 1, 0, c->ctus_y, tree_rule, d_min, d_max, nullptr, c->stream, true, d_skip, skip_mask, true, d_intra);
    }
    return rc != FHEVC_OK ? rc : p_tree_select_on(c, d_shapes, d_merge, with_merge, 1, 0, c->ctus_y, tree_rule, d_min, d_max, nullptr, c->stream);
  });
}

int fhevc_p_tree_frame(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range, int coarse_range,
                       const fhevc_pu_shape_rule* shape_rule, const fhevc_p_tree_rule* tree_rule, uint8_t* depth_min, uint8_t* depth_max, fhevc_pu_shape_node* shapes)
{
  return p_tree_frame_on(c, cur_luma, ref_luma, stride_samples, qp, search_range, coarse_range, shape_rule, tree_rule, depth_min, depth_max, shapes, false, nullptr);
}

int fhevc_p_tree_merge_frame(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range, int coarse_range,
                             const fhevc_pu_shape_rule* shape_rule, const fhevc_p_tree_rule* tree_rule, uint8_t* depth_min, uint8_t* depth_max, fhevc_pu_shape_node* shapes,
                             fhevc_motion_merge_node* merge)
{
  return p_tree_frame_on(c, cur_luma, ref_luma, stride_samples, qp, search_range, coarse_range, shape_rule, tree_rule, depth_min, depth_max, shapes, true, merge);
}

int fhevc_p_tree_merge_pu_frame(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range, int coarse_range,
                                const fhevc_pu_shape_rule* shape_rule, const fhevc_p_tree_rule* tree_rule, uint8_t* depth_min, uint8_t* depth_max, fhevc_pu_shape_node* shapes,
                                fhevc_motion_merge_node* merge)
{
  return p_tree_frame_on(c, cur_luma, ref_luma, stride_samples, qp, search_range, coarse_range, shape_rule, tree_rule, depth_min, depth_max, shapes, true, merge, true);
}

int fhevc_p_tree_amvp_frame(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range, int coarse_range,
                            const fhevc_pu_shape_rule* shape_rule, const fhevc_p_tree_rule* tree_rule, uint8_t* depth_min, uint8_t* depth_max, fhevc_pu_shape_node* shapes,
                            fhevc_motion_merge_node* merge)
{
  return p_tree_frame_on(c, cur_luma, ref_luma, stride_samples, qp, search_range, coarse_range, shape_rule, tree_rule, depth_min, depth_max, shapes, true, merge, true, true);
}

int fhevc_p_tree_intra_frame(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range, int coarse_range,
                             const fhevc_pu_shape_rule* shape_rule, const fhevc_p_tree_rule* tree_rule, int skip_mask, uint8_t* depth_min, uint8_t* depth_max,
                             fhevc_pu_shape_node* shapes, fhevc_motion_merge_node* merge, fhevc_intra_p_node* intra)
{
  return p_tree_frame_on(c, cur_luma, ref_luma, stride_samples, qp, search_range, coarse_range, shape_rule, tree_rule, depth_min, depth_max, shapes, true, merge, true, true,
                         true, skip_mask, intra);
}

int fhevc_p_tree_rd_frame(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range, int coarse_range,
                          const fhevc_pu_shape_rule* shape_rule, const fhevc_p_tree_rule* tree_rule, int skip_mask, uint8_t* depth_min, uint8_t* depth_max,
                          fhevc_pu_shape_node* shapes, fhevc_motion_merge_node* merge, fhevc_motion_rd_node* rd_merge, fhevc_motion_rd_pu_node* rd_pu)
{
  const RdFrameOut rd = { rd_merge, rd_pu, false, nullptr };
  return p_tree_frame_on(c, cur_luma, ref_luma, stride_samples, qp, search_range, coarse_range, shape_rule, tree_rule, depth_min, depth_max, shapes, true, merge, true, true,
                         false, skip_mask, nullptr, &rd);
}

int fhevc_p_tree_rd_qt_frame(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range, int coarse_range,
                             const fhevc_pu_shape_rule* shape_rule, const fhevc_p_tree_rule* tree_rule, int skip_mask, int tu_depths, uint8_t* depth_min, uint8_t* depth_max,
                             fhevc_pu_shape_node* shapes, fhevc_motion_merge_node* merge, fhevc_motion_rd_node* rd_merge, fhevc_motion_rd_pu_node* rd_pu)
{
  const RdFrameOut rd = { rd_merge, rd_pu, false, nullptr, tu_depths };
  return p_tree_frame_on(c, cur_luma, ref_luma, stride_samples, qp, search_range, coarse_range, shape_rule, tree_rule, depth_min, depth_max, shapes, true, merge, true, true,
                         false, skip_mask, nullptr, &rd);
}

int fhevc_p_tree_rd_intra_frame(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range, int coarse_range,
                                const fhevc_pu_shape_rule* shape_rule, const fhevc_p_tree_rule* tree_rule, int skip_mask, uint8_t* depth_min, uint8_t* depth_max,
                                fhevc_pu_shape_node* shapes, fhevc_motion_merge_node* merge, fhevc_motion_rd_node* rd_merge, fhevc_motion_rd_pu_node* rd_pu,
                                fhevc_node_cost* first)
{
  const RdFrameOut rd = { rd_merge, rd_pu, true, first };
  return p_tree_frame_on(c, cur_luma, ref_luma, stride_samples, qp, search_range, coarse_range, shape_rule, tree_rule, depth_min, depth_max, shapes, true, merge, true, true,
                         false, skip_mask, nullptr, &rd);
}

int fhevc_p_tree_rd_intra_qt_frame(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range, int coarse_range,
                                   const fhevc_pu_shape_rule* shape_rule, const fhevc_p_tree_rule* tree_rule, int skip_mask, int tu_depths, uint8_t* depth_min,
                                   uint8_t* depth_max, fhevc_pu_shape_node* shapes, fhevc_motion_merge_node* merge, fhevc_motion_rd_node* rd_merge,
                                   fhevc_motion_rd_pu_node* rd_pu, fhevc_node_cost* first)
{
  const RdFrameOut rd = { rd_merge, rd_pu, true, first, tu_depths };
  return p_tree_frame_on(c, cur_luma, ref_luma, stride_samples, qp, search_range, coarse_range, shape_rule, tree_rule, depth_min, depth_max, shapes, true, merge, true, true,
                         false, skip_mask, nullptr, &rd);
}

int fhevc_p_tree_rd_intra_nxn_frame(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range, int coarse_range,
                                    const fhevc_pu_shape_rule* shape_rule, const fhevc_p_tree_rule* tree_rule, int skip_mask, uint8_t* depth_min, uint8_t* depth_max,
                                    fhevc_pu_shape_node* shapes, fhevc_motion_merge_node* merge, fhevc_motion_rd_node* rd_merge, fhevc_motion_rd_pu_node* rd_pu,
                                    fhevc_node_cost* first, fhevc_intra_rd_nxn_node* nxn)
{
  const RdFrameOut rd = { rd_merge, rd_pu, true, first, 3, true, nxn };
  return p_tree_frame_on(c, cur_luma, ref_luma, stride_samples, qp, search_range, coarse_range, shape_rule, tree_rule, depth_min, depth_max, shapes, true, merge, true, true,
                         false, skip_mask, nullptr, &rd);
}

int fhevc_p_tree_rd_intra_search_frame(fhevc_ctx* c, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range, int coarse_range,
                                       const fhevc_pu_shape_rule* shape_rule, const fhevc_p_tree_rule* tree_rule, const fhevc_intra_search_rule* rule, int skip_mask,
                                       uint8_t* depth_min, uint8_t* depth_max, fhevc_pu_shape_node* shapes, fhevc_motion_merge_node* merge, fhevc_motion_rd_node* rd_merge,
                                       fhevc_motion_rd_pu_node* rd_pu, fhevc_node_cost* first, fhevc_intra_rd_nxn_node* nxn)
{
  fhevc_intra_search_rule hm;
  fhevc_intra_search_rule_default(&hm);
  const RdFrameOut rd = { rd_merge, rd_pu, true, first, 3, true, nxn, rule ? rule : &hm };
  return p_tree_frame_on(c, cur_luma, ref_luma, stride_samples, qp, search_range, coarse_range, shape_rule, tree_rule, depth_min, depth_max, shapes, true, merge, true, true,
                         false, skip_mask, nullptr, &rd);
}

}  // extern "C"
