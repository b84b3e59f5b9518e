// fhevc_api.hip -- the C ABI of include/fasthevc.h but for config 4 (fhevc_motion_api.hip): context, staging buffers, launches, multi-device sharding, the host-batch ring.
// Host-side C++ only; all device work is in the k_*.hip files, the weight images in fhevc_weights.hip, the context-free functions in fhevc_host.hip.
#include "fhevc_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <new>
#include <thread>

namespace {

void time_resolve(fhevc_ctx* c)
{
  for (auto& t : c->pending) {
    float ms = 0;
    if (hipEventSynchronize(t.stop) == hipSuccess && hipEventElapsedTime(&ms, t.start, t.stop) == hipSuccess) {
      c->slot_ms(t.which) += ms;
      c->slot_launches(t.which) += 1;
      if (t.which == 0) c->stats.last_cnn_ms = ms;
      if (t.which == 1) c->stats.last_hadamard_ms = ms;
      if (t.which == 2) c->stats.last_first_pass_ms = ms;
    }
    c->pool.emplace_back(t.start, t.stop);
  }
  c->pending.clear();
}

// the one picture in the context's staging plane (the host-buffer entry points)
FhevcFrames staged_frame(const fhevc_ctx* c) { return frames_of(c, c->d_luma, 2, c->dev_stride, 0, 1, 0, c->ctus_y); }

// upload rows [y0, y1) of one host picture (Pel plane with stride) into the context's staging plane, between the events that time the upload
int upload_rows(fhevc_ctx* c, const int16_t* luma, int stride_samples, int y0, int y1)
{
  HIP_TRY(c, hipEventRecord(c->ev[0], c->stream));
  HIP_TRY(c, hipMemcpy2DAsync(c->d_luma + (size_t)y0 * c->dev_stride, (size_t)c->dev_stride * 2, luma + (size_t)y0 * stride_samples, (size_t)stride_samples * 2,
                              (size_t)c->cfg.width * 2, (size_t)(y1 - y0), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipEventRecord(c->ev[1], c->stream));
  c->stats.bytes_h2d += (uint64_t)c->cfg.width * (y1 - y0) * 2;
  return FHEVC_OK;
}
int upload_frame(fhevc_ctx* c, const int16_t* luma, int stride_samples) { return upload_rows(c, luma, stride_samples, 0, c->cfg.height); }

// The parity entry points that bring back the cost of every (unit, mode) pair: a table allocated per call, one picture up, launch(frame, sqrt_lambda, table),
// the table (and, where asked, the 85-node best costs) back, the table freed
template <class F> int first_pass_all_modes(fhevc_ctx* c, const int16_t* luma, int stride_samples, int qp, size_t units_per_ctu, fhevc_node_cost* all,
                                            fhevc_node_cost* best, const char* what, F&& launch)
{
  if (!c || !luma || !all || stride_samples < c->cfg.width || qp < 0 || qp > 51) return FHEVC_E_INVALID;
  (void)hipSetDevice(c->device);
  const size_t n_all = (size_t)c->num_ctus * units_per_ctu * 35;
  FhevcNodeCost* d_all = nullptr;
  HIP_TRY(c, hipMalloc(&d_all, n_all * sizeof(FhevcNodeCost)));
  int rc = upload_frame(c, luma, stride_samples);
  if (rc == FHEVC_OK) {
    hipError_t e = launch(staged_frame(c), sqrt_lambda_intra(qp), d_all);
    if (e == hipSuccess) e = hipMemcpyAsync(all, d_all, n_all * sizeof(FhevcNodeCost), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && best) e = hipMemcpyAsync(best, c->d_nodes, (size_t)c->num_ctus * FHEVC_NODES_PER_CTU * sizeof(FhevcNodeCost), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) rc = fail(c, FHEVC_E_HIP, what, e);
  }
  (void)hipFree(d_all);
  c->stats.kernels_launched++;
  return rc;
}

}  // namespace

extern "C" {

const char* fhevc_last_error(fhevc_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int fhevc_create(fhevc_ctx** out, const fhevc_cfg* cfg)
{
  if (!out || !cfg) return FHEVC_E_INVALID;
  *out = nullptr;
  if (cfg->width <= 0 || cfg->height <= 0 || cfg->width > 16384 || cfg->height > 16384) return FHEVC_E_INVALID;
  if (cfg->ctu_size != FHEVC_CTU || cfg->max_depth != 3) return FHEVC_E_INVALID;
  if (cfg->bit_depth < 8 || cfg->bit_depth > 12) return FHEVC_E_INVALID;
  if (cfg->backend != FHEVC_BACKEND_HIP) return FHEVC_E_INVALID;  // there is no CPU backend
  if (cfg->num_devices > 16 || (cfg->num_devices > 1 && !cfg->device_ids)) return FHEVC_E_INVALID;
  fhevc_ctx* c = new (std::nothrow) fhevc_ctx();
  if (!c) return FHEVC_E_NOMEM;
  c->cfg = *cfg;
  c->cfg.weights_path = nullptr;
  c->cfg.device_ids = nullptr;
  if (c->cfg.max_frames < 1) c->cfg.max_frames = 1;
  c->device = (cfg->device_ids && cfg->num_devices >= 1) ? cfg->device_ids[0] : 0;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || c->device >= ndev) { delete c; return FHEVC_E_NO_DEVICE; }
  hipDeviceProp_t prop;
  if (hipSetDevice(c->device) != hipSuccess || hipGetDeviceProperties(&prop, c->device) != hipSuccess) { delete c; return FHEVC_E_NO_DEVICE; }
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) { delete c; return FHEVC_E_NO_DEVICE; }  // code object is gfx950-only
  c->num_cus = prop.multiProcessorCount;
  c->knobs = fhevc_read_knobs();   // every environment switch of the library is read here, once per context
  if (const char* fz = std::getenv("FHEVC_FUSE_HADAMARD")) c->fuse_hadamard = fz[0] != '0';
  if (const char* hf = std::getenv("FHEVC_HADAMARD_FORM")) c->had_valu = std::strcmp(hf, "mfma") != 0;
  // arithmetic of conv2 / conv3 in the depth kernel: "f16" (16-bit MFMAs) or "i8" (v_mfma_i32_32x32x32_i8); both are exact
  if (const char* ar = std::getenv("FHEVC_CNN_ARITH")) c->cnn_i8 = std::strcmp(ar, "f16") != 0;
  c->ctus_x = (cfg->width + 63) / 64;
  c->ctus_y = (cfg->height + 63) / 64;
  c->num_ctus = c->ctus_x * c->ctus_y;
  c->dev_stride = c->ctus_x * 64;
  // A BLOCKING stream (hipStreamDefault): it is ordered after everything issued earlier on the legacy default stream and before
  // everything issued later on it, so a caller that works on the default stream (stream 0, torch's default) and passes
  // stream = NULL needs no extra synchronisation; callers on their own non-blocking streams pass that stream explicitly
  if (hipStreamCreateWithFlags(&c->stream, hipStreamDefault) != hipSuccess) { delete c; return FHEVC_E_NO_DEVICE; }
  if (fhevc_cnn_prepare_device() != hipSuccess) { (void)hipStreamDestroy(c->stream); delete c; return FHEVC_E_NO_DEVICE; }  // per device, not per process
  bool ok = true;
  ok &= hipMalloc(&c->d_luma, pair_plane(c) * sizeof(int16_t)) == hipSuccess;
  ok &= hipMalloc(&c->d_depth, (size_t)c->num_ctus * 256) == hipSuccess;
  ok &= hipMalloc(&c->d_had, (size_t)c->num_ctus * 4) == hipSuccess;
  ok &= hipMalloc(&c->d_nodes, (size_t)c->num_ctus * FHEVC_NODES_PER_CTU * sizeof(FhevcNodeCost)) == hipSuccess;
  ok &= hipMalloc(&c->d_satd, 2 * 64 * 64 * sizeof(int16_t)) == hipSuccess;
  ok &= hipMalloc(&c->d_satd_out, 4) == hipSuccess;
  for (auto& e : c->ev) ok &= hipEventCreate(&e) == hipSuccess;
  if (!ok) { fhevc_destroy(c); return FHEVC_E_NOMEM; }
  if (hipMemset(c->d_luma, 0, pair_plane(c) * sizeof(int16_t)) != hipSuccess) { fhevc_destroy(c); return FHEVC_E_HIP; }
  if (cfg->weights_path) {
    FILE* fp = std::fopen(cfg->weights_path, "rb");
    if (!fp) { fhevc_destroy(c); return FHEVC_E_WEIGHTS; }
    std::vector<uint8_t> buf((size_t)4 << 20);   // FHW1 is 42 KB, the largest family member this build runs (FHW3, 32 / 64 / 128) 133 KB
    const size_t n = std::fread(buf.data(), 1, buf.size(), fp);
    std::fclose(fp);
    const int rc = fhevc_set_weights(c, buf.data(), n);
    if (rc != FHEVC_OK) { fhevc_destroy(c); return rc; }
  }
  // the other devices of a multi-device context: one single-device context each (the same picture geometry and weights).  A device
  // that cannot be brought up is left out -- the context works with the ones that can -- and counted in stats.devices_failed
  c->stats.devices = 1;
  for (int d = 1; d < cfg->num_devices; ++d) {
    fhevc_cfg sub = *cfg;
    int id = cfg->device_ids[d];
    sub.num_devices = 1;
    sub.device_ids = &id;
    fhevc_ctx* peer = nullptr;
    if (fhevc_create(&peer, &sub) == FHEVC_OK) { c->peers.push_back(peer); c->stats.devices++; }
    else c->stats.devices_failed++;
  }
  if (const char* ft = std::getenv("FHEVC_TEST_FAIL_DEVICE")) c->fail_peer_for_test = std::atoi(ft);
  (void)hipSetDevice(c->device);
  *out = c;
  return FHEVC_OK;
}

void fhevc_destroy(fhevc_ctx* c)
{
  if (!c) return;
  for (fhevc_ctx* peer : c->peers) fhevc_destroy(peer);
  c->peers.clear();
  (void)hipSetDevice(c->device);
  // launches of the *_device entry points may still be queued on the callers' own streams: nothing below may be freed under them
  (void)hipDeviceSynchronize();
  time_resolve(c);
  for (auto& p : c->pool) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
  for (auto& e : c->ev) if (e) (void)hipEventDestroy(e);
  if (c->lw_done) (void)hipEventDestroy(c->lw_done);
  void* const bufs[] = { c->d_frag, c->d_bias, c->d_whead, c->d_bhead, c->d_frag_i8, c->d_bias_i8,                                  // the base image
                         c->f_frag1, c->f_bias1, c->f_frag2, c->f_frag3, c->f_bias_i8, c->f_whead, c->f_headm, c->f_bhead,          // a fused family member's
                         c->d_luma, c->d_depth, c->d_had, c->d_nodes, c->d_satd, c->d_satd_out, c->d_act, c->d_depth_max, c->d_pair, c->d_motion, c->d_qpel, c->d_motion_pu, c->d_motion_pu_small, c->d_centres, c->d_qpel_pu, c->d_qpel_pu_small, c->d_merge_pu, c->d_amvp, c->d_amvp_mvp,
                         c->d_p_maps, c->d_first_p, c->d_intra_p, c->d_mvtab, c->d_cand_all, c->d_cand, c->d_best4, c->d_modes4 };
  for (void* q : bufs) (void)hipFree(q);
  for (void* q : c->lw_bufs) (void)hipFree(q);
  for (auto& sl : c->slot) {  // the host-batch ring of fhevc_predict_frames: stream, device buffers, pinned staging
    if (sl.st) { (void)hipStreamSynchronize(sl.st); (void)hipStreamDestroy(sl.st); }
    (void)hipFree(sl.d_in); (void)hipFree(sl.d_depth); (void)hipFree(sl.d_had);
    if (sl.h_in) (void)hipHostFree(sl.h_in);
    if (sl.h_depth) (void)hipHostFree(sl.h_depth);
    if (sl.h_had) (void)hipHostFree(sl.h_had);
  }
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int fhevc_enable_kernel_timing(fhevc_ctx* c, int on)
{
  if (!c) return FHEVC_E_INVALID;
  if (!on) time_resolve(c);
  c->timing = on != 0;
  return FHEVC_OK;
}

int fhevc_kernel_timing(fhevc_ctx* c, int which, int reset, double* avg_ms, uint64_t* launches)
{
  // 14, 16, 18, 20, 22, 24 and 26 stay rejected: callers probe them as the first numbers behind the slots of the partition-size selection, of the centred chain,
  // of the tree, of the two merge stages, of the zero-residual test, of the re-pricing and of the intra stage (28; 29 is the RD estimate); 30 likewise, 31 is the RD estimate under a partition size; 32 likewise, 33 is the RD
  // estimate of the intra candidate; 34 likewise, 35 is the RD estimates at three TU depths: the first slot beside the table; 36 likewise, 37 is the RD estimate
  // of the intra candidate at three TU depths, beside the table too
  if (which != 41)   // ... and 41 the same searched over the first pass's candidate lists; 40 and 42 likewise rejected
  if (which != 39)   // ... and 39 the RD estimate of the intra candidate with the NxN candidate; 38 and 40 likewise rejected
  if (which != 37)
  if (which != 35)
  if (!c || which < 0 || which > 33 || which == 32 || which == 30 || which == 28 || which == 14 || which == 16 || which == 18 || which == 20 || which == 22 || which == 24 || which == 26) return FHEVC_E_INVALID;
  if (!c) return FHEVC_E_INVALID;
  time_resolve(c);
  if (avg_ms) *avg_ms = c->slot_launches(which) ? c->slot_ms(which) / (double)c->slot_launches(which) : 0.0;
  if (launches) *launches = c->slot_launches(which);
  if (reset) { c->slot_ms(which) = 0; c->slot_launches(which) = 0; }
  return FHEVC_OK;
}

int fhevc_predict_frames_device(fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride_samples,
                                long long frame_stride_samples, int num_frames, int ctu_row_begin, int ctu_row_end, int qp,
                                uint8_t* d_depth_map, int32_t* d_hadamard, int32_t* d_logits, uint32_t* d_flags, void* stream)
{
  return fhevc_predict_frames_device_range(c, d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, ctu_row_begin,
                                           ctu_row_end, qp, 0, 0, d_depth_map, nullptr, d_hadamard, d_logits, d_flags, stream);
}

int fhevc_predict_frames_device_range(fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride_samples,
                                      long long frame_stride_samples, int num_frames, int ctu_row_begin, int ctu_row_end, int qp,
                                      int margin_split, int margin_stop, uint8_t* d_depth_map, uint8_t* d_depth_max, int32_t* d_hadamard, int32_t* d_logits,
                                      uint32_t* d_flags, void* stream)
{
  if (!c || !d_luma || !d_depth_map) return FHEVC_E_INVALID;
  if (!c->have_weights) return fail(c, FHEVC_E_STATE, "weights not set");
  if (const char* bad = batch_error(c, sample_bytes, stride_samples, frame_stride_samples, num_frames, 1, ctu_row_begin, ctu_row_end, 0, true))   // qp is clamped
    return fail(c, FHEVC_E_INVALID, bad);
  if (margin_split < 0 || margin_split > (1 << 30) || margin_stop < 0 || margin_stop > (1 << 30)) return fail(c, FHEVC_E_INVALID, "bad decision margin");
  if (ctu_row_begin == ctu_row_end) return FHEVC_OK;
  const FhevcFrames fr = frames_of(c, d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, ctu_row_begin, ctu_row_end, qp);
  // the source Hadamard rides on the depth kernel's own pass over the frame wherever the layout allows the fused form
  // (aligned planes, widths that are multiples of 16, up to 10 bit); otherwise it is its own HBM-bound launch
  const bool fuse = d_hadamard && c->fuse_hadamard && !c->family && fhevc_cnn_can_fuse_hadamard(fr);
  if (d_hadamard && !fuse) {
    const int rc = launch_on(c, stream, 1, "fhevc_launch_src_hadamard", [&](hipStream_t s) { return fhevc_launch_src_hadamard(fr, d_hadamard, s); });
    if (rc != FHEVC_OK) return rc;
  }
  const int rc = launch_on(c, stream, 0, "depth kernel", [&](hipStream_t s) {
    if (!c->family) return fhevc_launch_cnn(fr, cnn_weights(c), d_depth_map, fuse ? d_hadamard : nullptr, d_logits, d_flags, d_depth_max, margin_split, margin_stop, c->num_cus, c->knobs, s);
    if (!c->fam_layers) return fhevc_launch_cnn_family(fr, family_weights(c), d_depth_map, d_logits, d_flags, d_depth_max, margin_split, margin_stop, c->num_cus, s);
    if (c->fam_d2) return fhevc_launch_cnn_d2(fr, c->lw, d_depth_map, d_logits, d_flags, d_depth_max, margin_split, margin_stop, c->num_cus, s);
    hipError_t e = c->lw_done ? hipSuccess : hipEventCreateWithFlags(&c->lw_done, hipEventDisableTiming);
    if (e == hipSuccess && c->lw_in_flight && c->lw_last_stream != s) e = hipStreamWaitEvent(s, c->lw_done, 0);   // the scratch tensors are still being read there
    if (e != hipSuccess) return e;
    e = fhevc_launch_cnn_layers(fr, c->lw, d_depth_map, d_logits, d_flags, d_depth_max, margin_split, margin_stop, c->num_cus, c->knobs, s);
    (void)hipEventRecord(c->lw_done, s);   // also after a failed launch: whatever did get queued on s still owns the scratch
    c->lw_last_stream = s; c->lw_in_flight = true;
    return e;
  });
  if (rc != FHEVC_OK) return rc;
  c->stats.frames += (uint64_t)num_frames;
  c->stats.ctus += (uint64_t)num_frames * (uint64_t)(ctu_row_end - ctu_row_begin) * (uint64_t)c->ctus_x;
  return FHEVC_OK;
}

int fhevc_expand_depth_flags_device(fhevc_ctx* c, const uint32_t* d_flags, int num_frames, uint8_t* d_depth_map, void* stream)
{
  if (!c || !d_flags || !d_depth_map || num_frames < 1) return FHEVC_E_INVALID;
  (void)hipSetDevice(c->device);
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
  const FhevcFrames fr = frames_of(c, nullptr, 1, c->cfg.width, 0, num_frames, 0, c->ctus_y);
  HIP_TRY(c, fhevc_launch_expand_flags(fr, d_flags, d_depth_map, s));
  c->stats.kernels_launched++;
  return FHEVC_OK;
}

// One picture's CTU rows [rb, re) on ONE device: upload those rows, run the depth kernel over the band, bring the band's maps back
// into the caller's whole-picture buffers at the band's place.  depth_max (with its margins) is optional.  Synchronous.
static int predict_band_host(fhevc_ctx* c, const int16_t* luma, int stride_samples, int qp, int rb, int re, int margin_split, int margin_stop,
                             uint8_t* depth_min, uint8_t* depth_max, int32_t* ctu_src_hadamard)
{
  if (rb >= re) return FHEVC_OK;
  if (!c->have_weights) return fail(c, FHEVC_E_STATE, "weights not set");
  (void)hipSetDevice(c->device);
  if (depth_max) HIP_TRY(c, ensure(c->d_depth_max, (size_t)c->num_ctus * 256));
  const size_t band_ctus = (size_t)(re - rb) * c->ctus_x, first = (size_t)rb * c->ctus_x;
  int rc = upload_rows(c, luma, stride_samples, rb * 64, std::min(c->cfg.height, re * 64));
  if (rc != FHEVC_OK) return rc;
  // the kernel writes a band's results compactly from the start of its output buffers
  rc = fhevc_predict_frames_device_range(c, c->d_luma, 2, c->dev_stride, 0, 1, rb, re, qp, margin_split, margin_stop, c->d_depth, depth_max ? c->d_depth_max : nullptr,
                                         ctu_src_hadamard ? c->d_had : nullptr, nullptr, nullptr, c->stream);
  if (rc != FHEVC_OK) return rc;
  HIP_TRY(c, hipEventRecord(c->ev[2], c->stream));
  HIP_TRY(c, hipMemcpyAsync(depth_min + first * 256, c->d_depth, band_ctus * 256, hipMemcpyDeviceToHost, c->stream));
  if (depth_max) HIP_TRY(c, hipMemcpyAsync(depth_max + first * 256, c->d_depth_max, band_ctus * 256, hipMemcpyDeviceToHost, c->stream));
  if (ctu_src_hadamard) HIP_TRY(c, hipMemcpyAsync(ctu_src_hadamard + first, c->d_had, band_ctus * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipEventRecord(c->ev[3], c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  float ms = 0;
  if (hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) c->stats.ms_h2d += ms;
  if (hipEventElapsedTime(&ms, c->ev[1], c->ev[2]) == hipSuccess) c->stats.ms_kernels += ms;
  if (hipEventElapsedTime(&ms, c->ev[2], c->ev[3]) == hipSuccess) c->stats.ms_d2h += ms;
  c->stats.bytes_d2h += (uint64_t)band_ctus * ((depth_max ? 512 : 256) + (ctu_src_hadamard ? 4 : 0));
  return FHEVC_OK;
}

// The devices of a context that still work: the primary first.  (A failed peer is destroyed and forgotten: drop_peer.)
static std::vector<fhevc_ctx*> live_devices(fhevc_ctx* c)
{
  std::vector<fhevc_ctx*> v{ c };
  v.insert(v.end(), c->peers.begin(), c->peers.end());
  return v;
}
static void drop_peer(fhevc_ctx* c, fhevc_ctx* peer, const char* what)
{
  for (size_t i = 0; i < c->peers.size(); ++i)
    if (c->peers[i] == peer) {
      c->err = std::string("device ") + std::to_string(peer->device) + " dropped (" + what + "): " + peer->err;
      fhevc_destroy(peer);
      c->peers.erase(c->peers.begin() + (long)i);
      c->stats.devices_failed++;
      c->stats.devices = 1 + c->peers.size();
      return;
    }
}
// run share(i, device_i) for every live device concurrently (one host thread per device beyond the caller's own); a share that fails
// on a PEER is redone on the primary and the peer is dropped: the call fails only if the primary itself fails
static int run_sharded(fhevc_ctx* c, const std::function<int(int, int, fhevc_ctx*)>& share)
{
  const std::vector<fhevc_ctx*> dev = live_devices(c);
  const int n = (int)dev.size();
  std::vector<int> rc((size_t)n, FHEVC_OK);
  std::vector<std::thread> th;
  for (int i = 1; i < n; ++i)
    th.emplace_back([&, i] {
      rc[(size_t)i] = (c->fail_peer_for_test == i) ? fail(dev[(size_t)i], FHEVC_E_HIP, "failure injected by FHEVC_TEST_FAIL_DEVICE") : share(i, n, dev[(size_t)i]);
    });
  rc[0] = share(0, n, c);
  for (auto& t : th) t.join();
  if (c->fail_peer_for_test >= 1) c->fail_peer_for_test = -1;  // once
  (void)hipSetDevice(c->device);
  if (rc[0] != FHEVC_OK) return rc[0];
  for (int i = 1; i < n; ++i) {
    // statistics of a multi-device context are the sums over its devices
    c->stats.frames += dev[(size_t)i]->stats.frames; c->stats.ctus += dev[(size_t)i]->stats.ctus;
    c->stats.bytes_h2d += dev[(size_t)i]->stats.bytes_h2d; c->stats.bytes_d2h += dev[(size_t)i]->stats.bytes_d2h;
    c->stats.kernels_launched += dev[(size_t)i]->stats.kernels_launched;
    dev[(size_t)i]->stats = fhevc_stats{};
    if (rc[(size_t)i] != FHEVC_OK) {
      const int redo = share(i, n, c);   // the failed device's share, on the primary
      drop_peer(c, dev[(size_t)i], "its share was redone on the primary device");
      if (redo != FHEVC_OK) return redo;
    }
  }
  return FHEVC_OK;
}

// one host picture through the classifier: the plain map (depth_max null, margins 0) or the range
static int predict_frame_host(fhevc_ctx* c, const int16_t* luma, int stride_samples, int qp, int margin_split, int margin_stop,
                              uint8_t* depth_min, uint8_t* depth_max, int32_t* ctu_src_hadamard)
{
  if (!c || !luma || !depth_min || stride_samples < c->cfg.width) return FHEVC_E_INVALID;
  if (!c->have_weights) return fail(c, FHEVC_E_STATE, "weights not set");
  if (c->peers.empty()) return predict_band_host(c, luma, stride_samples, qp, 0, c->ctus_y, margin_split, margin_stop, depth_min, depth_max, ctu_src_hadamard);
  // CTU-row bands over the devices (fhevc_band): rows [i * rows / n, (i + 1) * rows / n) on device i
  const uint64_t frames0 = c->stats.frames;
  const int rc = run_sharded(c, [&](int i, int n, fhevc_ctx* d) {
    int rb = 0, re = 0;
    (void)fhevc_band(c->ctus_y, i, n, &rb, &re);
    return predict_band_host(d, luma, stride_samples, qp, rb, re, margin_split, margin_stop, depth_min, depth_max, ctu_src_hadamard);
  });
  c->stats.frames = frames0 + 1;   // one picture = one frame in the statistics whatever the number of bands
  return rc;
}

int fhevc_predict_frame(fhevc_ctx* c, const int16_t* luma, int stride_samples, int qp, int slice_type,
                        uint8_t* depth_map, int32_t* ctu_src_hadamard)
{
  (void)slice_type;
  return predict_frame_host(c, luma, stride_samples, qp, 0, 0, depth_map, nullptr, ctu_src_hadamard);
}

int fhevc_predict_frame_range(fhevc_ctx* c, const int16_t* luma, int stride_samples, int qp, int slice_type, int margin_split, int margin_stop,
                              uint8_t* depth_min, uint8_t* depth_max, int32_t* ctu_src_hadamard)
{
  (void)slice_type;
  if (!depth_max) return FHEVC_E_INVALID;
  return predict_frame_host(c, luma, stride_samples, qp, margin_split, margin_stop, depth_min, depth_max, ctu_src_hadamard);
}

void* fhevc_alloc_host(fhevc_ctx* c, size_t bytes)
{
  if (!c || bytes == 0) return nullptr;
  (void)hipSetDevice(c->device);
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
  return p;
}

void fhevc_free_host(fhevc_ctx* c, void* p)
{
  if (!c || !p) return;
  (void)hipSetDevice(c->device);
  (void)hipHostFree(p);
}

static bool is_pinned(const void* p)
{
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }  // pageable memory: "invalid value"
  return a.type == hipMemoryTypeHost;
}

// wait for the slot's stream and hand its outputs to the caller (pageable destinations were staged in pinned memory)
static int drain_slot(fhevc_ctx* c, fhevc_ctx::Slot& sl)
{
  if (sl.frames == 0) return FHEVC_OK;
  HIP_TRY(c, hipStreamSynchronize(sl.st));
  if (sl.staged_out) {
    std::memcpy(sl.out_depth, sl.h_depth, (size_t)sl.frames * c->num_ctus * 256);
    if (sl.out_had) std::memcpy(sl.out_had, sl.h_had, (size_t)sl.frames * c->num_ctus * 4);
  }
  sl.frames = 0;
  return FHEVC_OK;
}

static int predict_frames_one_device(fhevc_ctx* c, const void* luma, int sample_bytes, int stride_samples, long long frame_stride_samples, int num_frames,
                                     int qp, uint8_t* depth_map, int32_t* ctu_src_hadamard);

int fhevc_predict_frames(fhevc_ctx* c, const void* luma, int sample_bytes, int stride_samples, long long frame_stride_samples, int num_frames,
                         int qp, uint8_t* depth_map, int32_t* ctu_src_hadamard)
{
  if (!c || !luma || !depth_map) return FHEVC_E_INVALID;
  if (c->peers.empty() || num_frames < 2) return predict_frames_one_device(c, luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, qp, depth_map, ctu_src_hadamard);
  // a batch over several devices: contiguous runs of pictures, frames [i * F / n, (i + 1) * F / n) on device i ("frames can
  // instead be dealt round-robin -- strictly simpler"); every device runs its own two-stream host batch, all at the same time
  return run_sharded(c, [&](int i, int n, fhevc_ctx* d) {
    int fb = 0, fe = 0;
    (void)fhevc_band(num_frames, i, n, &fb, &fe);
    if (fb >= fe) return (int)FHEVC_OK;
    return predict_frames_one_device(d, static_cast<const uint8_t*>(luma) + (size_t)fb * (size_t)frame_stride_samples * sample_bytes, sample_bytes, stride_samples,
                                     frame_stride_samples, fe - fb, qp, depth_map + (size_t)fb * c->num_ctus * 256,
                                     ctu_src_hadamard ? ctu_src_hadamard + (size_t)fb * c->num_ctus : nullptr);
  });
}

static int predict_frames_one_device(fhevc_ctx* c, const void* luma, int sample_bytes, int stride_samples, long long frame_stride_samples, int num_frames,
                                     int qp, uint8_t* depth_map, int32_t* ctu_src_hadamard)
{
  if (!c || !luma || !depth_map) return FHEVC_E_INVALID;
  if (!c->have_weights) return fail(c, FHEVC_E_STATE, "weights not set");
  if (const char* bad = batch_error(c, sample_bytes, stride_samples, frame_stride_samples, num_frames, 1, 0, c->ctus_y, 0, true)) return fail(c, FHEVC_E_INVALID, bad);
  const long long frame_extent = (long long)stride_samples * (c->cfg.height - 1) + c->cfg.width;  // samples of one frame, first to last
  (void)hipSetDevice(c->device);
  const int chunk = c->cfg.max_frames;
  const size_t fs_bytes = (size_t)(num_frames > 1 ? frame_stride_samples : frame_extent) * sample_bytes;
  const size_t chunk_in = (size_t)(chunk - 1) * fs_bytes + (size_t)frame_extent * sample_bytes;  // bytes from the first sample of a chunk to its last
  const bool in_pinned = is_pinned(luma), out_pinned = is_pinned(depth_map) && (!ctu_src_hadamard || is_pinned(ctu_src_hadamard));
  for (auto& sl : c->slot) {
    if (!sl.st) HIP_TRY(c, hipStreamCreateWithFlags(&sl.st, hipStreamNonBlocking));
    if (sl.in_cap < chunk_in) {
      (void)hipFree(sl.d_in);
      sl.d_in = nullptr; sl.in_cap = 0;
      HIP_TRY(c, hipMalloc(&sl.d_in, chunk_in + 64));
      sl.in_cap = chunk_in;
    }
    if (sl.frames_cap < (size_t)chunk) {
      (void)hipFree(sl.d_depth); (void)hipFree(sl.d_had);
      if (sl.h_depth) (void)hipHostFree(sl.h_depth);
      if (sl.h_had) (void)hipHostFree(sl.h_had);
      sl.d_depth = nullptr; sl.d_had = nullptr; sl.h_depth = nullptr; sl.h_had = nullptr; sl.frames_cap = 0;
      HIP_TRY(c, hipMalloc(&sl.d_depth, (size_t)chunk * c->num_ctus * 256));
      HIP_TRY(c, hipMalloc(&sl.d_had, (size_t)chunk * c->num_ctus * 4));
      HIP_TRY(c, hipHostMalloc(&sl.h_depth, (size_t)chunk * c->num_ctus * 256, hipHostMallocDefault));
      HIP_TRY(c, hipHostMalloc(&sl.h_had, (size_t)chunk * c->num_ctus * 4, hipHostMallocDefault));
      sl.frames_cap = (size_t)chunk;
    }
    if (!in_pinned && sl.h_in_cap < chunk_in) {
      if (sl.h_in) (void)hipHostFree(sl.h_in);
      sl.h_in = nullptr; sl.h_in_cap = 0;
      HIP_TRY(c, hipHostMalloc(&sl.h_in, chunk_in, hipHostMallocDefault));
      sl.h_in_cap = chunk_in;
    }
  }
  int rc = FHEVC_OK;
  auto hip_rc = [&](hipError_t e, const char* what) { return e == hipSuccess ? FHEVC_OK : fail(c, FHEVC_E_HIP, what, e); };
  for (int f0 = 0, k = 0; f0 < num_frames && rc == FHEVC_OK; f0 += chunk, ++k) {
    fhevc_ctx::Slot& sl = c->slot[k & 1];
    rc = drain_slot(c, sl);  // chunk k-2: its maps reach the caller while chunk k-1 computes
    if (rc != FHEVC_OK) break;
    const int nf = std::min(chunk, num_frames - f0);
    const uint8_t* src = static_cast<const uint8_t*>(luma) + (size_t)f0 * fs_bytes;
    const size_t bytes = (size_t)(nf - 1) * fs_bytes + (size_t)frame_extent * sample_bytes;
    if (!in_pinned) { std::memcpy(sl.h_in, src, bytes); src = sl.h_in; }
    rc = hip_rc(hipMemcpyAsync(sl.d_in, src, bytes, hipMemcpyHostToDevice, sl.st), "upload of a chunk");
    if (rc != FHEVC_OK) break;
    rc = fhevc_predict_frames_device(c, sl.d_in, sample_bytes, stride_samples, (long long)(fs_bytes / sample_bytes), nf, 0, c->ctus_y, qp, sl.d_depth,
                                     ctu_src_hadamard ? sl.d_had : nullptr, nullptr, nullptr, sl.st);
    if (rc != FHEVC_OK) break;
    rc = hip_rc(hipMemcpyAsync(out_pinned ? depth_map + (size_t)f0 * c->num_ctus * 256 : sl.h_depth, sl.d_depth, (size_t)nf * c->num_ctus * 256,
                               hipMemcpyDeviceToHost, sl.st), "download of a chunk's maps");
    if (rc == FHEVC_OK && ctu_src_hadamard)
      rc = hip_rc(hipMemcpyAsync(out_pinned ? (void*)(ctu_src_hadamard + (size_t)f0 * c->num_ctus) : (void*)sl.h_had, sl.d_had, (size_t)nf * c->num_ctus * 4,
                                 hipMemcpyDeviceToHost, sl.st), "download of a chunk's Hadamard sums");
    if (rc != FHEVC_OK) break;
    // only now is the slot "in flight": a failure above leaves nothing for a later drain to copy into this caller's buffers
    sl.frames = nf;
    sl.out_depth = depth_map + (size_t)f0 * c->num_ctus * 256;
    sl.out_had = ctu_src_hadamard ? ctu_src_hadamard + (size_t)f0 * c->num_ctus : nullptr;
    sl.staged_out = !out_pinned;
    c->stats.bytes_h2d += bytes;
    c->stats.bytes_d2h += (uint64_t)nf * c->num_ctus * (256 + (ctu_src_hadamard ? 4 : 0));
  }
  if (rc != FHEVC_OK) {
    // error path: let both streams finish whatever they hold, hand nothing more to the caller, and forget the slots' destinations
    // (the caller's buffers may be gone by the next call)
    for (auto& sl : c->slot) {
      if (sl.st) (void)hipStreamSynchronize(sl.st);
      sl.frames = 0; sl.out_depth = nullptr; sl.out_had = nullptr;
    }
    return rc;
  }
  for (auto& sl : c->slot) {
    const int r2 = drain_slot(c, sl);
    if (rc == FHEVC_OK) rc = r2;
  }
  if (rc != FHEVC_OK)
    for (auto& sl : c->slot) { sl.frames = 0; sl.out_depth = nullptr; sl.out_had = nullptr; }
  return rc;
}

int fhevc_satd(fhevc_ctx* c, const int16_t* org, int org_stride, const int16_t* cur, int cur_stride,
               int w, int h, int bit_depth, uint32_t* out)
{
  if (!c || !org || !cur || !out) return FHEVC_E_INVALID;
  if (w < 2 || h < 2 || w > 64 || h > 64 || (w & 1) || (h & 1) || bit_depth < 8 || bit_depth > 12) return fail(c, FHEVC_E_INVALID, "bad SATD block");
  if (org_stride < w || cur_stride < w) return fail(c, FHEVC_E_INVALID, "bad SATD stride");
  (void)hipSetDevice(c->device);
  HIP_TRY(c, hipMemcpy2DAsync(c->d_satd, 64 * 2, org, (size_t)org_stride * 2, (size_t)w * 2, (size_t)h, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpy2DAsync(c->d_satd + 64 * 64, 64 * 2, cur, (size_t)cur_stride * 2, (size_t)w * 2, (size_t)h, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, fhevc_launch_satd(c->d_satd, 64, c->d_satd + 64 * 64, 64, w, h, bit_depth, c->d_satd_out, c->stream));
  HIP_TRY(c, hipMemcpyAsync(out, c->d_satd_out, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->stats.kernels_launched++;
  return FHEVC_OK;
}

// ---- 35-mode first pass of the 85 nodes (k_firstpass.hip) ----

int fhevc_intra_first_pass(fhevc_ctx* c, const int16_t* luma, int stride_samples, int qp, fhevc_node_cost* out)
{
  if (!c || !luma || !out || stride_samples < c->cfg.width || qp < 0 || qp > 51) return FHEVC_E_INVALID;
  (void)hipSetDevice(c->device);
  int rc = upload_frame(c, luma, stride_samples);
  if (rc != FHEVC_OK) return rc;
  rc = launch_on(c, nullptr, 2, "fhevc_launch_first_pass", [&](hipStream_t s) { return fhevc_launch_first_pass(staged_frame(c), sqrt_lambda_intra(qp), c->d_nodes, nullptr, s); });
  if (rc != FHEVC_OK) return rc;
  static_assert(sizeof(fhevc_node_cost) == sizeof(FhevcNodeCost), "node cost layout");
  HIP_TRY(c, hipMemcpyAsync(out, c->d_nodes, (size_t)c->num_ctus * FHEVC_NODES_PER_CTU * sizeof(FhevcNodeCost), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FHEVC_OK;
}

int fhevc_intra_first_pass_all(fhevc_ctx* c, const int16_t* luma, int stride_samples, int qp, fhevc_node_cost* best, fhevc_node_cost* all)
{
  return first_pass_all_modes(c, luma, stride_samples, qp, FHEVC_NODES_PER_CTU, all, best, "first pass (all modes)",
                              [&](const FhevcFrames& fr, double sqrt_lambda, FhevcNodeCost* d_all) { return fhevc_launch_first_pass(fr, sqrt_lambda, c->d_nodes, d_all, c->stream); });
}

// The consumer of the first pass: HM prunes the 35 modes of a PU to numModesForFullRD candidates with exactly these costs
// (TEncSearch::estIntraPredLumaQT, TEncSearch.cpp:2271-2320, xUpdateCandList :5385-5408: the N smallest costs, an earlier mode ahead of a later
// one of the same cost).  modes: numCtus * 85 * num_candidates, best first; 255 in every slot of a node that crosses the picture edge.
int fhevc_intra_first_pass_candidates(fhevc_ctx* c, const int16_t* luma, int stride_samples, int qp, int num_candidates, uint8_t* modes)
{
  if (!c || !luma || !modes || num_candidates < 1 || num_candidates > 8 || stride_samples < c->cfg.width || qp < 0 || qp > 51) return FHEVC_E_INVALID;
  (void)hipSetDevice(c->device);
  const size_t nodes = (size_t)c->num_ctus * FHEVC_NODES_PER_CTU;
  HIP_TRY(c, ensure(c->d_cand_all, nodes * 35 * sizeof(FhevcNodeCost)));
  HIP_TRY(c, ensure(c->d_cand, nodes * 8));
  int rc = upload_frame(c, luma, stride_samples);
  if (rc != FHEVC_OK) return rc;
  rc = launch_on(c, nullptr, 2, "first-pass candidates", [&](hipStream_t s) { return fhevc_launch_first_pass(staged_frame(c), sqrt_lambda_intra(qp), c->d_nodes, c->d_cand_all, s); });
  if (rc != FHEVC_OK) return rc;
  // the sort runs on the device: 85 x K bytes per CTU come back instead of 85 x 35 x 16
  hipError_t e = fhevc_launch_first_pass_topk(c->d_cand_all, (long long)nodes, num_candidates, c->d_cand, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(modes, c->d_cand, nodes * num_candidates, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(c, FHEVC_E_HIP, "first-pass candidates", e);
  c->stats.kernels_launched++;
  c->stats.bytes_d2h += nodes * num_candidates;
  return FHEVC_OK;
}

int fhevc_intra_first_pass_device(fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride_samples,
                                  long long frame_stride_samples, int num_frames, int ctu_row_begin, int ctu_row_end,
                                  int qp, fhevc_node_cost* d_out, void* stream)
{
  if (!c || !d_luma || !d_out) return FHEVC_E_INVALID;
  if (const char* bad = batch_error(c, sample_bytes, stride_samples, frame_stride_samples, num_frames, 1, ctu_row_begin, ctu_row_end, qp, false)) return fail(c, FHEVC_E_INVALID, bad);
  // (no early return on an empty band: the launcher has nothing to do, and the launch is counted)
  const FhevcFrames fr = frames_of(c, d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, ctu_row_begin, ctu_row_end);
  return launch_on(c, stream, 2, "fhevc_launch_first_pass",
                   [&](hipStream_t s) { return fhevc_launch_first_pass(fr, sqrt_lambda_intra(qp), reinterpret_cast<FhevcNodeCost*>(d_out), nullptr, s); });
}

// the lists of the 85 nodes over a device-resident batch: selected inside the 85-node kernel, so no (node, mode) table and nothing that two
// streams could share
int fhevc_intra_first_pass_candidates_device(fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                                             int num_frames, int ctu_row_begin, int ctu_row_end, int qp, int num_candidates, uint8_t* d_modes, void* stream)
{
  if (!c || !d_luma || !d_modes) return FHEVC_E_INVALID;
  if (const char* bad = batch_error(c, sample_bytes, stride_samples, frame_stride_samples, num_frames, 1, ctu_row_begin, ctu_row_end, qp, false)) return fail(c, FHEVC_E_INVALID, bad);
  if (num_candidates < 1 || num_candidates > 8) return fail(c, FHEVC_E_INVALID, "num_candidates: 1..8");
  if (ctu_row_begin == ctu_row_end) return FHEVC_OK;  // an empty band: nothing to launch, nothing written
  const FhevcFrames fr = frames_of(c, d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, ctu_row_begin, ctu_row_end);
  return launch_on(c, stream, 2, "fhevc_launch_first_pass",
                   [&](hipStream_t s) { return fhevc_launch_first_pass(fr, sqrt_lambda_intra(qp), nullptr, nullptr, s, d_modes, num_candidates); });
}

// ---- first pass of the 4x4 PUs of NxN CUs (k_firstpass4.hip) ----

int fhevc_intra_first_pass_4x4_device(fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                                      int num_frames, int ctu_row_begin, int ctu_row_end, int qp, int num_candidates, fhevc_node_cost* d_best,
                                      uint8_t* d_modes, void* stream)
{
  if (!c || !d_luma || (!d_best && !d_modes)) return FHEVC_E_INVALID;
  if (const char* bad = batch_error(c, sample_bytes, stride_samples, frame_stride_samples, num_frames, 1, ctu_row_begin, ctu_row_end, qp, false)) return fail(c, FHEVC_E_INVALID, bad);
  if (d_modes && (num_candidates < 1 || num_candidates > 8)) return fail(c, FHEVC_E_INVALID, "num_candidates: 1..8");
  if (ctu_row_begin == ctu_row_end) return FHEVC_OK;  // an empty band: nothing to launch, nothing written
  const FhevcFrames fr = frames_of(c, d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, ctu_row_begin, ctu_row_end);
  return launch_on(c, stream, 6, "fhevc_launch_first_pass4", [&](hipStream_t s) {
    return fhevc_launch_first_pass4(fr, sqrt_lambda_intra(qp), d_modes ? num_candidates : 0, reinterpret_cast<FhevcNodeCost*>(d_best), d_modes, nullptr, s);
  });
}

int fhevc_intra_first_pass_4x4(fhevc_ctx* c, const int16_t* luma, int stride_samples, int qp, int num_candidates, fhevc_node_cost* best, uint8_t* modes)
{
  if (!c || !luma || (!best && !modes) || stride_samples < c->cfg.width || qp < 0 || qp > 51 || (modes && (num_candidates < 1 || num_candidates > 8)))
    return FHEVC_E_INVALID;
  (void)hipSetDevice(c->device);
  const size_t pus = (size_t)c->num_ctus * FHEVC_PUS4_PER_CTU;
  HIP_TRY(c, ensure(c->d_best4, pus * sizeof(FhevcNodeCost)));
  HIP_TRY(c, ensure(c->d_modes4, pus * 8));
  int rc = upload_frame(c, luma, stride_samples);
  if (rc != FHEVC_OK) return rc;
  rc = fhevc_intra_first_pass_4x4_device(c, c->d_luma, 2, c->dev_stride, 0, 1, 0, c->ctus_y, qp, num_candidates, best ? reinterpret_cast<fhevc_node_cost*>(c->d_best4) : nullptr,
                                         modes ? c->d_modes4 : nullptr, c->stream);
  if (rc != FHEVC_OK) return rc;
  if (best) HIP_TRY(c, hipMemcpyAsync(best, c->d_best4, pus * sizeof(FhevcNodeCost), hipMemcpyDeviceToHost, c->stream));
  if (modes) HIP_TRY(c, hipMemcpyAsync(modes, c->d_modes4, pus * num_candidates, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->stats.bytes_d2h += (best ? pus * sizeof(FhevcNodeCost) : 0) + (modes ? pus * num_candidates : 0);
  return FHEVC_OK;
}

int fhevc_intra_first_pass_4x4_all(fhevc_ctx* c, const int16_t* luma, int stride_samples, int qp, fhevc_node_cost* all)
{
  return first_pass_all_modes(c, luma, stride_samples, qp, FHEVC_PUS4_PER_CTU, all, nullptr, "4x4 first pass (all modes)",
                              [&](const FhevcFrames& fr, double sqrt_lambda, FhevcNodeCost* d_all) { return fhevc_launch_first_pass4(fr, sqrt_lambda, 0, nullptr, nullptr, d_all, c->stream); });
}

// ---- adaptive-QP pre-analysis (k_preanalyze.hip) ----

int fhevc_preanalyze_frames_device(fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride_samples,
                                   long long frame_stride_samples, int num_frames, int ctu_row_begin, int ctu_row_end,
                                   int max_aq_depth, double* d_activity, void* stream)
{
  if (!c || !d_luma || !d_activity) return FHEVC_E_INVALID;
  if (const char* bad = batch_error(c, sample_bytes, stride_samples, frame_stride_samples, num_frames, 1, ctu_row_begin, ctu_row_end, 0, false)) return fail(c, FHEVC_E_INVALID, bad);
  if (max_aq_depth < 1 || max_aq_depth > 4) return fail(c, FHEVC_E_INVALID, "bad max_aq_depth");
  if ((c->cfg.width & 7) || (c->cfg.height & 7)) return fail(c, FHEVC_E_INVALID, "pre-analysis needs picture sizes that are multiples of 8");
  // (no early return on an empty band: the launcher has nothing to do, and the launch is counted)
  const FhevcFrames fr = frames_of(c, d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, ctu_row_begin, ctu_row_end);
  const long long per_frame = fhevc_aq_parts(c->cfg.width, c->cfg.height, max_aq_depth, nullptr);
  return launch_on(c, stream, 3, "fhevc_launch_preanalyze", [&](hipStream_t s) { return fhevc_launch_preanalyze(fr, max_aq_depth, per_frame, d_activity, c->num_cus, s); });
}

int fhevc_preanalyze(fhevc_ctx* c, const int16_t* luma, int stride_samples, int max_aq_depth, double* activity, double* avg_activity)
{
  if (!c || !luma || !activity || !avg_activity || stride_samples < c->cfg.width) return FHEVC_E_INVALID;
  long long off[5];
  const int total = fhevc_aq_parts(c->cfg.width, c->cfg.height, max_aq_depth, off);
  if (total < 0) return fail(c, FHEVC_E_INVALID, "bad max_aq_depth");
  (void)hipSetDevice(c->device);
  HIP_TRY(c, ensure(c->d_act, (size_t)fhevc_aq_parts(c->cfg.width, c->cfg.height, 4, nullptr) * sizeof(double)));
  int rc = upload_frame(c, luma, stride_samples);
  if (rc != FHEVC_OK) return rc;
  rc = fhevc_preanalyze_frames_device(c, c->d_luma, 2, c->dev_stride, 0, 1, 0, c->ctus_y, max_aq_depth, c->d_act, c->stream);
  if (rc != FHEVC_OK) return rc;
  HIP_TRY(c, hipMemcpyAsync(activity, c->d_act, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  // TEncPreanalyzer.cpp:147-150: dSumAct accumulates part by part in raster order; keep that order
  for (int d = 0; d < max_aq_depth; ++d) {
    double sum = 0.0;
    for (long long i = off[d]; i < off[d + 1]; ++i) sum += activity[i];
    avg_activity[d] = sum / (double)(off[d + 1] - off[d]);
  }
  c->stats.bytes_d2h += (uint64_t)total * sizeof(double);
  return FHEVC_OK;
}

// Diagnostic (not part of include/fasthevc.h): run the stamped instantiation of the depth kernel over a
// device-resident batch and return per-phase cycle sums averaged over workgroups (slots 0..7: prologue, conv1, conv2, conv3,
// barrier wait after staging, depth, heads, staging), CTUs per workgroup (8), the grid (9), and the in-kernel clock in MHz
// (10: median over the workgroups, 11: the slowest; s_memtime span / s_memrealtime span of the whole CTU loop).
int fhevc_debug_cnn_phase_cycles(fhevc_ctx* c, const void* d_luma, int sample_bytes, int stride_samples,
                                 long long frame_stride_samples, int num_frames, uint8_t* d_depth_map, double* out12)
{
  if (!c || !d_luma || !d_depth_map || !out12 || !c->have_weights) return FHEVC_E_INVALID;
  (void)hipSetDevice(c->device);
  const FhevcFrames fr = frames_of(c, d_luma, sample_bytes, stride_samples, frame_stride_samples, num_frames, 0, c->ctus_y);
  unsigned long long* d_st = nullptr;
  const int max_grid = 4 * c->num_cus;  // fhevc_launch_cnn_stamped runs at most four workgroups per CU
  const size_t slots = (size_t)max_grid * FHEVC_STAMP_SLOTS;
  HIP_TRY(c, hipMalloc(&d_st, slots * sizeof(unsigned long long)));
  HIP_TRY(c, hipMemset(d_st, 0, slots * sizeof(unsigned long long)));
  int grid = 0;
  int32_t* d_had = nullptr;  // the fused source Hadamard's output, as in the timed launch (FHEVC_DEBUG_STAMPS_NO_HADAMARD=1: without it)
  if (!std::getenv("FHEVC_DEBUG_STAMPS_NO_HADAMARD")) HIP_TRY(c, hipMalloc(&d_had, (size_t)num_frames * c->num_ctus * sizeof(int32_t)));
  HIP_TRY(c, fhevc_launch_cnn_stamped(fr, cnn_weights(c), d_depth_map, d_had, c->num_cus, c->knobs, d_st, &grid, c->stream));
  std::vector<unsigned long long> h(slots);
  HIP_TRY(c, hipMemcpyAsync(h.data(), d_st, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  (void)hipFree(d_st);
  if (d_had) (void)hipFree(d_had);
  for (int k = 0; k < 12; ++k) out12[k] = 0;
  for (int b = 0; b < grid; ++b) for (int k = 0; k < 8; ++k) out12[k] += (double)h[(size_t)b * FHEVC_STAMP_SLOTS + k] / grid;
  out12[8] = (double)num_frames * c->num_ctus / grid;
  out12[9] = grid;
  // the in-kernel clock: shader cycles per 100 MHz tick over each workgroup's whole CTU loop, median over the workgroups (MHz)
  std::vector<double> mhz;
  for (int b = 0; b < grid; ++b)
    if (h[(size_t)b * FHEVC_STAMP_SLOTS + 9]) mhz.push_back(100.0 * (double)h[(size_t)b * FHEVC_STAMP_SLOTS + 8] / (double)h[(size_t)b * FHEVC_STAMP_SLOTS + 9]);
  std::sort(mhz.begin(), mhz.end());
  out12[10] = mhz.empty() ? 0.0 : mhz[mhz.size() / 2];
  out12[11] = mhz.empty() ? 0.0 : mhz.front();
  // [12 + 9 * slot + k]: the same eight phase sums averaged over the workgroups of CU slot 0 / 1 / 2 (k = 8: how many workgroups that is) -- the caller's
  // array holds 39 doubles (FHEVC_DEBUG_STAMPS_BY_SLOT=1; the i8 form's conv-phase priority differs by slot, k_cnn.hip FHEVC_PRIO_ON)
  if (std::getenv("FHEVC_DEBUG_STAMPS_BY_SLOT")) {
    for (int k = 12; k < 39; ++k) out12[k] = 0;
    for (int b = 0; b < grid; ++b) {
      const int sl = (int)std::min<unsigned long long>(h[(size_t)b * FHEVC_STAMP_SLOTS + 10], 2);
      for (int k = 0; k < 8; ++k) out12[12 + 9 * sl + k] += (double)h[(size_t)b * FHEVC_STAMP_SLOTS + k];
      out12[12 + 9 * sl + 8] += 1;
    }
    for (int sl = 0; sl < 3; ++sl)
      for (int k = 0; k < 8; ++k) if (out12[12 + 9 * sl + 8] > 0) out12[12 + 9 * sl + k] /= out12[12 + 9 * sl + 8];
  }
  return FHEVC_OK;
}

int fhevc_set_cnn_arith(fhevc_ctx* c, int arith)
{
  if (!c) return FHEVC_E_INVALID;
  if (arith != FHEVC_CNN_ARITH_I8 && arith != FHEVC_CNN_ARITH_F16) return fail(c, FHEVC_E_INVALID, "arith: FHEVC_CNN_ARITH_I8 or FHEVC_CNN_ARITH_F16");
  c->cnn_i8 = arith == FHEVC_CNN_ARITH_I8;
  for (fhevc_ctx* peer : c->peers) peer->cnn_i8 = c->cnn_i8;
  return FHEVC_OK;
}

int fhevc_set_motion_distortion(fhevc_ctx* c, int mode)
{
  if (!c) return FHEVC_E_INVALID;
  if (mode != FHEVC_MOTION_SATD && mode != FHEVC_MOTION_SAD) return fail(c, FHEVC_E_INVALID, "mode: FHEVC_MOTION_SATD or FHEVC_MOTION_SAD");
  c->motion_sad = mode == FHEVC_MOTION_SAD;
  return FHEVC_OK;
}

int fhevc_get_cnn_arith(const fhevc_ctx* c)
{
  if (!c) return FHEVC_E_INVALID;
  return c->cnn_i8 ? FHEVC_CNN_ARITH_I8 : FHEVC_CNN_ARITH_F16;
}

int fhevc_get_stats(fhevc_ctx* c, void* out, size_t size)
{
  if (!c || !out) return FHEVC_E_INVALID;
  time_resolve(c);
  std::memcpy(out, &c->stats, size < sizeof(fhevc_stats) ? size : sizeof(fhevc_stats));
  return FHEVC_OK;
}

}  // extern "C"
