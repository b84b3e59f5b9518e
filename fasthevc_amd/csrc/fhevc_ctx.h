// fhevc_ctx.h -- private to the C-ABI layer (fhevc_api.hip, fhevc_motion_api.hip, fhevc_weights.hip): the context behind the opaque fhevc_ctx of
// include/fasthevc.h, its error helpers, and the few functions that cross those files.  (fhevc_host.hip, which never touches a context, takes
// sqrt_lambda_intra from here: the host twin of the re-pricing builds the table of bit costs the device form builds.)
#pragma once
#include "../../include/fasthevc.h"
#include "fhevc_internal.h"

#include <cmath>
#include <string>
#include <utility>
#include <vector>

struct TimedLaunch { hipEvent_t start, stop; int which; };

struct fhevc_ctx {
  fhevc_cfg cfg{};
  int device = 0, num_cus = 256;
  hipStream_t stream = nullptr;
  int ctus_x = 0, ctus_y = 0, num_ctus = 0;
  int dev_stride = 0;  // samples, staging plane
  // weight image
  bool have_weights = false;
  uint4* d_frag = nullptr; float* d_bias = nullptr; uint8_t* d_whead = nullptr; int32_t* d_bhead = nullptr;
  uint4* d_frag_i8 = nullptr; int32_t* d_bias_i8 = nullptr;  // the i8 variant of conv2 / conv3 (k_cnn.hip)
  // a member of the reference's Bayesian-optimisation network family (FHW3 blob; k_cnn_family.inc): set instead of the arrays above
  bool family = false;
  bool fam_layers = false;            // ... run layer by layer through HBM (k_cnn_layers.inc): every member the fused kernels do not cover
  bool fam_d2 = false;                // ... of those, the members k_cnn_d2.inc runs as one LDS-resident kernel (the layer images are the same; no HBM scratch)
  FhevcLayersWeights lw = {};
  std::vector<void*> lw_bufs;         // everything lw points to (freed with the context / the next blob)
  // the layer path's activation tensors are ONE set per context: a launch on another stream than the previous one waits for that one's last kernel
  // (the host batch alternates two streams; callers may pass any stream per call)
  hipEvent_t lw_done = nullptr; hipStream_t lw_last_stream = nullptr; bool lw_in_flight = false;
  int fam_c[3] = { 0, 0, 0 };
  uint4* f_frag1 = nullptr; float* f_bias1 = nullptr; uint4* f_frag2 = nullptr; uint4* f_frag3 = nullptr; int32_t* f_bias_i8 = nullptr;
  uint8_t* f_whead = nullptr; uint8_t* f_headm = nullptr; int32_t* f_bhead = nullptr;
  int shift[3] = { 0, 0, 0 };
  int requant_mode[3] = { 0, 0, 0 };
  bool cnn_i8 = true;                                         // fhevc_set_cnn_arith / FHEVC_CNN_ARITH at fhevc_create
  float scale[3] = { 1, 1, 1 };
  // staging for the host-buffer entry points
  int16_t* d_luma = nullptr; uint8_t* d_depth = nullptr; int32_t* d_had = nullptr; FhevcNodeCost* d_nodes = nullptr;
  int16_t* d_satd = nullptr; uint32_t* d_satd_out = nullptr;
  hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr };
  // kernel timing
  bool fuse_hadamard = true;  // FHEVC_FUSE_HADAMARD=0 keeps the stand-alone Hadamard launch (A/B measurements)
  bool motion_sad = false;    // fhevc_set_motion_distortion: SAD (HM's integer-search distortion) instead of Hadamard SATD
  bool had_valu = true;       // FHEVC_HADAMARD_FORM=mfma: the fused Hadamard of 8-bit content on the bf16 MFMA from the staged tile instead of packed
                              // 16-bit VALU (parity-green, and measured 7 % SLOWER in round 3: profiles/r03_ab_hadamard_forms.log) -- kept for A/B and tests
  FhevcKnobs knobs;           // the environment's tuning / test switches, read once in fhevc_create
  bool timing = false;
  std::vector<TimedLaunch> pending;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
  // per timing slot (14, 16, 18, 20, 22, 24, 26, 28, 30, 32 and 34 are not in use); config 4's slots and its staging buffers d_pair .. d_intra_p: the tables in fhevc_motion_api.hip
  double sum_ms[34] = {};
  uint64_t launches[34] = {};
  double sum_ms_35 = 0;        // slot 35 (the RD estimates at three TU depths) beside the table: 34 is no slot
  uint64_t launches_35 = 0;
  double sum_ms_37 = 0;        // slot 37 (the RD estimate of the intra candidate at three TU depths), beside the table as well: 36 is no slot
  uint64_t launches_37 = 0;
  double sum_ms_39 = 0;        // slot 39 (... with the NxN candidate of the 8x8 nodes), beside the table as well: 38 is no slot
  uint64_t launches_39 = 0;
  double sum_ms_41 = 0;        // slot 41 (... searched over the first pass's candidate lists), beside the table as well: 40 is no slot
  uint64_t launches_41 = 0;
  double& slot_ms(int which) { return which == 41 ? sum_ms_41 : which == 39 ? sum_ms_39 : which == 37 ? sum_ms_37 : which == 35 ? sum_ms_35 : sum_ms[which]; }
  uint64_t& slot_launches(int which) { return which == 41 ? launches_41 : which == 39 ? launches_39 : which == 37 ? launches_37 : which == 35 ? launches_35 : launches[which]; }
  double* d_act = nullptr;
  int16_t* d_pair = nullptr;
  FhevcMotionNode *d_motion = nullptr, *d_motion_pu = nullptr, *d_motion_pu_small = nullptr, *d_centres = nullptr;
  FhevcMotionQpelNode *d_qpel = nullptr, *d_qpel_pu = nullptr, *d_qpel_pu_small = nullptr;
  FhevcMotionMergeNode* d_merge_pu = nullptr;
  FhevcMotionQpelNode* d_amvp = nullptr;     // the 593 re-priced entries per CTU of fhevc_motion_amvp and of fhevc_p_tree_amvp_frame
  FhevcMotionMvp* d_amvp_mvp = nullptr;      // ... and their predictor records
  uint8_t* d_p_maps = nullptr;
  FhevcNodeCost* d_first_p = nullptr;        // the 85 + 256 first-pass records per CTU of fhevc_intra_p and of fhevc_p_tree_intra_frame
  FhevcIntraPNode* d_intra_p = nullptr;      // ... and their 85 intra records
  FhevcNodeCost* d_cand_all = nullptr; uint8_t* d_cand = nullptr;   // fhevc_intra_first_pass_candidates: every (node, mode) cost, the lists
  FhevcNodeCost* d_best4 = nullptr; uint8_t* d_modes4 = nullptr;    // fhevc_intra_first_pass_4x4: the best mode and the list of every 4x4 PU
  uint32_t* d_mvtab = nullptr;        // vector costs of the wide search (k_motion_wide.hip), rebuilt when (qp, range) changes
  int mvtab_qp = -1, mvtab_range = -1;
  std::vector<uint32_t> mvtab_host;
  // host-batch ring (fhevc_predict_frames): two slots, each with its own stream, device buffers and pinned staging
  struct Slot {
    hipStream_t st = nullptr;
    uint8_t* d_in = nullptr; uint8_t* d_depth = nullptr; int32_t* d_had = nullptr;
    uint8_t* h_in = nullptr; uint8_t* h_depth = nullptr; int32_t* h_had = nullptr;  // pinned staging (pageable callers)
    size_t in_cap = 0, frames_cap = 0, h_in_cap = 0;
    // what is in flight on this slot: where its outputs go once the stream has drained
    int frames = 0; uint8_t* out_depth = nullptr; int32_t* out_had = nullptr; bool staged_out = false;
  } slot[2];
  uint8_t* d_depth_max = nullptr;
  fhevc_stats stats{};
  std::string err;
  // cfg.num_devices > 1: this context is the PRIMARY (device_ids[0]); the other devices are full single-device contexts of their own.
  // The host-buffer entry points shard over them (CTU-row bands of a picture, runs of pictures of a batch); a device that fails is
  // dropped for the rest of the context's life and its share is redone on a device that works (devices_failed counts them)
  std::vector<fhevc_ctx*> peers;
  int fail_peer_for_test = -1;   // FHEVC_TEST_FAIL_DEVICE=<index >= 1>: that device reports a failure on its next share (tests)
};

static inline int fail(fhevc_ctx* c, int code, const char* what, hipError_t e = hipSuccess)
{
  if (c) {
    c->err = what;
    if (e != hipSuccess) { c->err += ": "; c->err += hipGetErrorString(e); }
  }
  return code;
}

#define HIP_TRY(c, call)                                                   \
  do {                                                                     \
    hipError_t e_ = (call);                                                \
    if (e_ != hipSuccess) return fail((c), FHEVC_E_HIP, #call, e_);        \
  } while (0)

// ---- what the entry points of fhevc_api.hip and fhevc_motion_api.hip share ----

inline void time_begin(fhevc_ctx* c, hipStream_t s, int which)
{
  if (!c->timing) return;
  TimedLaunch t;
  if (!c->pool.empty()) { t.start = c->pool.back().first; t.stop = c->pool.back().second; c->pool.pop_back(); }
  else { (void)hipEventCreate(&t.start); (void)hipEventCreate(&t.stop); }
  t.which = which;
  (void)hipEventRecord(t.start, s);
  c->pending.push_back(t);
}
inline void time_end(fhevc_ctx* c, hipStream_t s)
{
  if (!c->timing) return;
  (void)hipEventRecord(c->pending.back().stop, s);
}

// One launch of an entry point: on the context's device, on the caller's stream (null: the context's own), between the timing events of slot `which`, counted.
// launch(stream) returns the launcher's hipError_t
template <class F> int launch_on(fhevc_ctx* c, void* stream, int which, const char* what, F&& launch)
{
  (void)hipSetDevice(c->device);
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
  time_begin(c, s, which);
  const hipError_t e = launch(s);
  if (e != hipSuccess) return fail(c, FHEVC_E_HIP, what, e);
  time_end(c, s);
  c->stats.kernels_launched++;
  return FHEVC_OK;
}

// a buffer of the context that is allocated by the first call that needs it
template <class T> hipError_t ensure(T*& p, size_t bytes) { return p ? hipSuccess : hipMalloc(&p, bytes); }

inline FhevcFrames frames_of(const fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride, long long frame_stride,
                      int num_frames, int row_begin, int row_end, int qp = 32)
{
  FhevcFrames f;
  f.luma = d_luma; f.sample_bytes = sample_bytes; f.stride = stride; f.frame_stride = frame_stride;
  f.width = c->cfg.width; f.height = c->cfg.height; f.bit_depth = c->cfg.bit_depth;
  f.ctus_x = c->ctus_x; f.ctus_y = c->ctus_y; f.num_frames = num_frames; f.row_begin = row_begin; f.row_end = row_end;
  f.qp = qp < 0 ? 0 : (qp > 51 ? 51 : qp);
  return f;
}

// What the entry points over a device-resident batch check of its layout, each condition in one spelling; null: nothing wrong.  min_frames: 2 where a picture
// is searched in the one before it.  qp: 0..51 (an entry point that clamps it, or has none, passes 0).  overlap: the frames of a batch must not overlap (asked
// by the entry points whose launch covers the whole batch at once and by the motion entry points)
inline const char* batch_error(const fhevc_ctx* c, int sample_bytes, int stride_samples, long long frame_stride_samples, int num_frames, int min_frames,
                        int ctu_row_begin, int ctu_row_end, int qp, bool overlap)
{
  if ((sample_bytes != 1 && sample_bytes != 2) || stride_samples < c->cfg.width || num_frames < min_frames) return "bad frame layout";
  if (ctu_row_begin < 0 || ctu_row_end > c->ctus_y || ctu_row_begin > ctu_row_end) return "bad CTU-row band";
  if (qp < 0 || qp > 51) return "qp out of range (0..51)";
  if (sample_bytes == 1 && c->cfg.bit_depth != 8) return "uint8 samples need bit_depth 8";
  if (overlap && num_frames > 1 && frame_stride_samples < (long long)stride_samples * (c->cfg.height - 1) + c->cfg.width) return "frames overlap";
  return nullptr;
}

// lambda = 0.57 * 2^((qp-12)/3): TEncSlice::calculateLambda, all-intra path (TEncSlice.cpp:433-527).  The first-pass cost is compared bit-for-bit with the
// oracle's doubles: this expression stays as it is
inline double sqrt_lambda_intra(int qp) { return std::sqrt(0.57 * std::pow(2.0, ((double)qp - 12.0) / 3.0)); }

// one of the context's two staging planes of a picture pair, in samples (fhevc_motion_api.hip); the single staging plane d_luma is as large
inline size_t pair_plane(const fhevc_ctx* c) { return (size_t)c->dev_stride * c->ctus_y * 64; }

// the kernel-argument views of the weight image in use (fhevc_weights.hip)
FhevcCnnWeights cnn_weights(const fhevc_ctx* c);
FhevcFamilyWeights family_weights(const fhevc_ctx* c);
