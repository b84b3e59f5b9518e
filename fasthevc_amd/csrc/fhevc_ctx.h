// fhevc_ctx.h -- private to the C-ABI layer (fhevc_api.hip, fhevc_weights.hip): the context behind the opaque fhevc_ctx of include/fasthevc.h,
// its error helpers, and the few functions that cross those two files.
#pragma once
#include "../../include/fasthevc.h"
#include "fhevc_internal.h"

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
  double sum_ms[20] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };     // slots 14, 16 and 18 are not in use (fhevc_kernel_timing rejects them)
  uint64_t launches[20] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
  double* d_act = nullptr;
  int16_t* d_pair = nullptr;          // two staging planes (reference, current) of fhevc_motion_search
  FhevcMotionNode* d_motion = nullptr;     // ... and, once the refinement has read them, the records of fhevc_p_shape_frame (an entry is as large)
  FhevcMotionQpelNode* d_qpel = nullptr;   // the output of fhevc_motion_refine and the nodes' output of fhevc_motion_refine_pu_wide (host forms); the input nodes go through d_motion
  FhevcMotionNode* d_motion_pu = nullptr;  // the output of fhevc_motion_search_pu (host form); its optional nodes go through d_motion
  FhevcMotionNode* d_motion_pu_small = nullptr;  // the output of fhevc_motion_search_pu_small (host form)
  FhevcMotionNode* d_centres = nullptr;    // the centres of fhevc_motion_search_pu_centred (host form): one entry per CTU
  FhevcMotionQpelNode* d_qpel_pu = nullptr;        // the outputs of fhevc_motion_refine_pu (host form); its input PUs go through d_motion_pu /
  FhevcMotionQpelNode* d_qpel_pu_small = nullptr;  // d_motion_pu_small
  uint8_t* d_p_maps = nullptr;       // fhevc_p_predict_frame: the reference picture's map, depth_min, depth_max (numCtus * 256 each)
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

// the kernel-argument views of the weight image in use (fhevc_weights.hip)
FhevcCnnWeights cnn_weights(const fhevc_ctx* c);
FhevcFamilyWeights family_weights(const fhevc_ctx* c);
