/*
 * fasthevc.h -- C ABI of the MI355X-native CU-partition fast-decision path.
 *
 * This is the drop-in boundary for HM's source/Lib/TLibEncoder (reference: omricarmi/FastHEVC, an HM-16.14
 * fork).  The reference has no plugin/FFI layer: the boundary the path sits behind is HM's own C++ class
 * surface, TEncSlice::compressSlice -> TEncCu::compressCtu -> TEncCu::xCompressCU (TEncSlice.cpp:698-983,
 * TEncCu.cpp:252-288, 496-1058).  A patched TEncSlice/TEncCu (hm_patch/) calls these entry
 * points from three places; everything else in HM stays untouched.  Plain pointers and sizes only.
 *
 * Conventions:
 *   - return 0 on success, a negative FHEVC_E_* code on failure; the caller falls back to stock full RDO for
 *     that picture -- the library never aborts the encode.  (HM itself reports errors by assert/exit:
 *     TEncCu.cpp:1055-1057.)
 *   - all buffers are caller-owned; calls are synchronous from the single encoder thread unless the entry
 *     point takes a stream; a context is not thread-safe (HM is not re-entrant either: TEncCu.cpp:50,126-131).
 *   - there is NO CPU backend: fhevc_create fails with FHEVC_E_NO_DEVICE when no gfx950 device is usable.
 *
 * Depth-map convention: per CTU 256 bytes, raster 16x16 of 4x4 luma units, value = CU depth 0..3
 * (0 = 64x64 ... 3 = 8x8); equals TComDataCU::getDepth(g_auiRasterToZscan[r]) (TComDataCU.h:86,207-211,
 * TComRom.cpp:284-287).  Units outside the picture carry 0; CUs that cross the picture edge are marked split,
 * as HM forces them to be (TEncCu.cpp:574, 894, 915).
 */
#ifndef FASTHEVC_H
#define FASTHEVC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FHEVC_OK               0
#define FHEVC_E_INVALID       -1   /* bad argument / unsupported geometry */
#define FHEVC_E_NO_DEVICE     -2   /* no usable gfx950 device, or HIP runtime error at create */
#define FHEVC_E_HIP           -3   /* HIP runtime error during a call (fhevc_last_error has the text) */
#define FHEVC_E_WEIGHTS       -4   /* weight blob missing / malformed */
#define FHEVC_E_NOMEM         -5
#define FHEVC_E_STATE         -6   /* call not valid in this state (e.g. predict before weights are set) */

#define FHEVC_BACKEND_HIP      1

#define FHEVC_NODES_PER_CTU   85   /* 1 + 4 + 16 + 64 CU nodes of sizes 64, 32, 16, 8 */
#define FHEVC_LOGITS_PER_CTU  42   /* 21 split decisions x 2 classes */

typedef struct fhevc_ctx fhevc_ctx; /* opaque: device buffers, streams, weights, timing events */

typedef struct {
  int width, height;        /* luma picture size (TComPicYuv::getWidth/getHeight(COMPONENT_Y)) */
  int bit_depth;            /* sps.getBitDepth(CHANNEL_TYPE_LUMA): 8..12 */
  int ctu_size;             /* 64 (the reference's dumper hard-codes it: HARP_Defines.h:28-29) */
  int max_depth;            /* 3: 8x8 leaves (MaxPartitionDepth 4) */
  int num_devices;          /* devices of THIS process (<= 16): > 1 makes the host-buffer entry points (fhevc_predict_frame[_range], fhevc_predict_frames)
                               shard CTU-row bands / runs of pictures over them (fhevc_band) and gather the maps into the caller's buffer;
                               a device that fails is dropped and its share redone on another (fhevc_stats.devices_failed), never an abort.
                               Entry points that take DEVICE pointers, and the parity / feature entry points, run on device_ids[0] */
  const int* device_ids;    /* HIP device ordinals, NULL = {0}; an ordinal may repeat (two queues on one device: tests) */
  const char* weights_path; /* FHW1 blob (fasthevc_amd/weights.py), or NULL and call fhevc_set_weights */
  int backend;              /* FHEVC_BACKEND_HIP */
  int max_frames;           /* frames per batched call the context sizes its staging buffers for (>= 1) */
} fhevc_cfg;

/* per-node result of the 35-mode first pass (twin of TEncSearch::estIntraPredLumaQT's first pass,
 * TEncSearch.cpp:2271-2295, with reference samples taken from the ORIGINAL plane) */
typedef struct {
  uint32_t satd;            /* SATD of the cheapest mode (TComRdCost::xGetHADs) */
  uint32_t mode;            /* its intra mode 0..34; 255 when the node crosses the picture edge */
  double   cost;            /* satd + modeBits * sqrt(lambda); -1 for skipped nodes */
} fhevc_node_cost;

typedef struct {
  uint64_t frames;          /* frames processed since create */
  uint64_t ctus;            /* CTU depth decisions delivered */
  uint64_t bytes_h2d, bytes_d2h;
  uint64_t kernels_launched;
  double   ms_h2d, ms_kernels, ms_d2h;   /* accumulated, HIP-event timed (host-buffer entry points only) */
  double   last_cnn_ms, last_hadamard_ms, last_first_pass_ms; /* last launch of each kernel */
  uint64_t devices;         /* devices this context works with right now (cfg.num_devices minus the failed ones) */
  uint64_t devices_failed;  /* devices that could not be brought up at fhevc_create or were dropped after a failed call */
} fhevc_stats;

int  fhevc_create(fhevc_ctx** out, const fhevc_cfg* cfg);
/* waits for the device first: launches of the *_device entry points still queued on any stream finish before anything is freed */
void fhevc_destroy(fhevc_ctx* ctx);
/* weights from memory instead of cfg.weights_path (same FHW1 bytes, or an FHW3 family member).  Ordering against the *_device entry points, on any
 * stream (the context's own, the default stream, a caller's non-blocking stream): launches issued BEFORE this call use the old weights, launches
 * issued after it the new ones.  The call waits for the device before the first byte of a weight image is overwritten or freed, so it blocks the
 * host until the work queued so far has finished: not for the hot path. */
int  fhevc_set_weights(fhevc_ctx* ctx, const void* blob, size_t bytes);

/* One picture, host buffers, synchronous.  Called once per picture before the CTU loop of
 * TEncSlice::compressSlice (TEncSlice.cpp:792) with pcPic->getPicYuvOrg()->getAddr(COMPONENT_Y) / getStride
 * (TComPicYuv.h:121-147).  depth_map: numCtus*256 bytes.  ctu_src_hadamard: optional, numCtus values equal to
 * TEncCu::updateCtuDataISlice(ctu, w, h) (TEncCu.cpp:1324-1343) -- what TEncSlice::calCostSliceI sums
 * (TEncSlice.cpp:663-695).  qp is the slice QP: it selects a per-QP prior on the split decisions (the reference
 * stores QP in its labels, CShow_PredResiReco.h:93, but its MATLAB pipeline never reads it); slice_type is
 * reserved (I slices only this round).
 * Plane contract of every entry point that takes luma / d_luma with stride_samples (tests/test_gpu_layouts.py): the pointer may have any
 * alignment (the sample's own included: an int16 plane may start on an odd byte pair, a uint8 plane on any byte), stride_samples any value
 * >= width, frame_stride_samples any value that keeps frames from overlapping; aligned layouts (16-byte aligned rows) are merely faster.
 * Nothing outside the picture rectangle is read FOR ITS VALUE: margins, stride padding, rows below a ragged picture and the gap between
 * frames may hold anything (HM's uninitialised or border-extended margins), results do not depend on them, and samples outside the
 * picture are taken as 0 (classifier, first pass) or as the replicated border (motion search).  Outputs are written over exactly the
 * extent stated per entry point; a band with ctu_row_begin == ctu_row_end writes nothing. */
int  fhevc_predict_frame(fhevc_ctx* ctx, const int16_t* luma, int stride_samples, int qp, int slice_type,
                         uint8_t* depth_map, int32_t* ctu_src_hadamard);

/* Host batch ("one CTU's depth map delivered to host memory"): num_frames pictures in host memory ->
 * depth maps (and, optionally, per-CTU source Hadamards) in host memory.  luma: sample_bytes = 2 (int16 Pel planes as HM lays
 * them out) or 1 (uint8 planes of 8-bit content, e.g. straight from an 8-bit .yuv file: TVideoIOYuv.cpp:249-330 reads the
 * same bytes and widens them); frame f starts at luma + f * frame_stride_samples.  The pictures travel in chunks of
 * cfg.max_frames through two streams, so that the upload of chunk k+1 and the download of chunk k-1 overlap the kernels of
 * chunk k.  Buffers from fhevc_alloc_host (or otherwise pinned) are read / written by DMA directly; pageable buffers go
 * through the context's pinned staging ring (one extra host copy per chunk).  Synchronous. */
int  fhevc_predict_frames(fhevc_ctx* ctx, const void* luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                          int num_frames, int qp, uint8_t* depth_map /* num_frames * numCtus * 256 */,
                          int32_t* ctu_src_hadamard /* num_frames * numCtus, or NULL */);
/* Library-side luma reader, host code only -- no device work, callable without a context: the luma planes of
 * `num_frames` pictures of a planar YUV file, from picture `first_frame` on, straight into `dst` (fhevc_alloc_host memory: no intermediate
 * copy between the file and the DMA source of fhevc_predict_frames).  What TVideoIOYuv::read does for COMPONENT_Y (TVideoIOYuv.cpp:249-330,
 * 675-760): one byte per sample for file_bit_depth 8, two little-endian bytes above; chroma (chroma_format 400 / 420 / 422 / 444) is skipped
 * with a seek, never read; the plane is padded on the right and at the bottom by edge replication from file_width x file_height to
 * dst_width x dst_height (the conformance size: ConformanceWindowMode 1 pads to a multiple of the minimum CU size 8, TAppEncCfg.cpp:1310-1370),
 * and left-shifted from the file's to the internal bit depth (scalePlane, TVideoIOYuv.cpp:70-84, :730; internal < file is not supported).
 * dst_sample_bytes 2: int16 Pel samples; 1: uint8 samples (8-bit file at 8-bit internal depth only).  Returns the number of pictures read
 * (fewer than asked for at the end of the file), or FHEVC_E_INVALID / FHEVC_E_STATE (file cannot be opened / is shorter than one picture). */
int  fhevc_read_yuv_luma(const char* path, int file_width, int file_height, int file_bit_depth, int chroma_format, long long first_frame,
                         int num_frames, int dst_width, int dst_height, int internal_bit_depth, int dst_sample_bytes, void* dst,
                         long long dst_stride_samples, long long dst_frame_stride_samples);
/* pinned host memory for the batch entry point (a .yuv reader can read luma planes straight into it) */
void* fhevc_alloc_host(fhevc_ctx* ctx, size_t bytes);
void  fhevc_free_host(fhevc_ctx* ctx, void* p);

/* Soft decisions for the xCompressCU hook (hm_patch/): depth_min holds only the splits whose logit difference exceeds
 * +margin_split, depth_max every split not rejected by more than -margin_stop (both >= 0, logit units; 0, 0: both maps
 * equal the map of fhevc_predict_frame).  The hook forces a split while depth < depth_min, forbids one at
 * depth >= depth_max and leaves the depths in between to HM's own RD search (TEncCu.cpp:576-849, 892).  margin_split
 * costs almost no time (the parent CU is evaluated as well), margin_stop costs the recursion it allows. */
int  fhevc_predict_frame_range(fhevc_ctx* ctx, const int16_t* luma, int stride_samples, int qp, int slice_type,
                               int margin_split, int margin_stop, uint8_t* depth_min, uint8_t* depth_max,
                               int32_t* ctu_src_hadamard);

/* == TComRdCost::calcHAD(bitDepth, org, strideOrg, cur, strideCur, w, h) (TComRdCost.cpp:297-334) and
 * xGetHADs (:1753-1824); host buffers, w,h <= 64.  Parity entry point. */
int  fhevc_satd(fhevc_ctx* ctx, const int16_t* org, int org_stride, const int16_t* cur, int cur_stride,
                int w, int h, int bit_depth, uint32_t* out);

/* 35-mode first pass for every CU node of every CTU of one picture (host buffers).  out: numCtus * 85 entries,
 * node order 64x64, 32x32 (raster), 16x16 (raster), 8x8 (raster).  lambda as TEncSlice::calculateLambda
 * (TEncSlice.cpp:433-527) would give it for qp; pass qp. */
int  fhevc_intra_first_pass(fhevc_ctx* ctx, const int16_t* luma, int stride_samples, int qp, fhevc_node_cost* out);

/* Parity entry point: the same pass, returning EVERY (node, mode) pair -- all: numCtus * 85 * 35 entries, [CTU][node][mode]
 * with satd = xGetHADs of that mode's prediction, mode = the mode, cost = satd + modeBits * sqrt(lambda) (nodes crossing the
 * picture edge: satd 0xFFFFFFFF, mode 255, cost -1); best (optional) as fhevc_intra_first_pass.  Lets a test see the
 * predictors and SATDs of modes that never win. */
int  fhevc_intra_first_pass_all(fhevc_ctx* ctx, const int16_t* luma, int stride_samples, int qp, fhevc_node_cost* best,
                                fhevc_node_cost* all);

/* What HM's own first pass is for: the candidate list of estIntraPredLumaQT (TEncSearch.cpp:2271-2320).  Per node the num_candidates (1..8; HM: 8 for
 * 8x8 PUs, 3 above) modes of smallest cost, best first, an earlier mode ahead of a later one of equal cost (xUpdateCandList,
 * TEncSearch.cpp:5385-5408); modes: numCtus * 85 * num_candidates bytes, 255 for nodes crossing the picture edge.  The costs come from ORIGINAL
 * neighbours (HM's own pass sees reconstructed ones inside its serial loop) and the mode-bit model of fhevc_intra_first_pass; HM still appends its
 * most-probable modes itself.  The selection runs on the device (85 x num_candidates bytes per CTU come back).  hm_patch: FHEVC_FIRST_PASS=1. */
int  fhevc_intra_first_pass_candidates(fhevc_ctx* ctx, const int16_t* luma, int stride_samples, int qp, int num_candidates, uint8_t* modes);

/* first pass over a device-resident batch (layout and band arguments as fhevc_predict_frames_device below);
 * d_out: (num_frames * band CTUs) * 85 entries in HBM.  Asynchronous with respect to the host. */
int  fhevc_intra_first_pass_device(fhevc_ctx* ctx, const void* d_luma, int sample_bytes, int stride_samples,
                                   long long frame_stride_samples, int num_frames, int ctu_row_begin, int ctu_row_end,
                                   int qp, fhevc_node_cost* d_out, void* stream);

/* The same first pass one level down: the four 4x4 PUs of every 8x8 CU, what HM's xCheckRDCostIntra(SIZE_NxN) runs through estIntraPredLumaQT
 * (35 modes per PU with xCalcHADs4x4, eight candidates kept: TEncSearch.cpp:2271-2320).  Per CTU 256 PUs in the depth map's unit order: PU
 * (ux, uy), raster 16x16, is the 4x4 block at (64 cx + 4 ux, 64 cy + 4 uy).  A PU is valid iff the 8x8 CU that holds it lies wholly inside the
 * picture (HM codes NxN only in whole 8x8 CUs); the others carry satd 0xFFFFFFFF, mode 255, cost -1 and 255 in every list slot.  Reference
 * samples (17 per PU) from the ORIGINAL plane with coding-order availability per 4-sample unit -- so inside one 8x8 CU PU 1 has no below-left,
 * PU 3 no above-right, and PU 2's above-right is PU 1 --; no smoothed line at this size; SATD, cost, mode-bit model and tie rule as above.
 * The lists are selected inside the kernel: per CTU 4 KB (best) and 256 * num_candidates bytes (lists) reach HBM.  The xCompressCU hook of
 * hm_patch/ does not consume these lists yet. */
#define FHEVC_PUS4_PER_CTU 256   /* raster 16x16 of 4x4 units: the depth map's unit order */

/* one picture, host buffers, synchronous.  best: numCtus * 256, or NULL; modes: numCtus * 256 * num_candidates
 * bytes, or NULL (then num_candidates is ignored); both NULL: FHEVC_E_INVALID */
int  fhevc_intra_first_pass_4x4(fhevc_ctx* ctx, const int16_t* luma, int stride_samples, int qp, int num_candidates,
                                fhevc_node_cost* best, uint8_t* modes);
/* parity entry point: all = numCtus * 256 * 35 entries [CTU][PU][mode], as fhevc_intra_first_pass_all */
int  fhevc_intra_first_pass_4x4_all(fhevc_ctx* ctx, const int16_t* luma, int stride_samples, int qp, fhevc_node_cost* all);
/* device-resident batch, layout / band / stream arguments as fhevc_intra_first_pass_device; outputs compact over
 * the band: d_best (num_frames * band CTUs) * 256 entries, d_modes (num_frames * band CTUs) * 256 * num_candidates bytes, written over exactly
 * that extent; d_best or d_modes may be NULL, not both; asynchronous with respect to the host, no allocation.  FHEVC_E_INVALID (nothing is
 * launched or written): a null plane, both outputs NULL, num_candidates outside 1..8 when d_modes is given, qp outside 0..51,
 * stride_samples < width, num_frames < 1, a bad band, uint8 planes on a context above 8 bit */
int  fhevc_intra_first_pass_4x4_device(fhevc_ctx* ctx, const void* d_luma, int sample_bytes, int stride_samples,
                                       long long frame_stride_samples, int num_frames, int ctu_row_begin, int ctu_row_end,
                                       int qp, int num_candidates, fhevc_node_cost* d_best, uint8_t* d_modes, void* stream);
/* the lists of the 85 nodes for a device-resident batch (the device form of fhevc_intra_first_pass_candidates, same bytes picture by
 * picture): d_modes = num_frames * band CTUs * 85 * num_candidates bytes, compact over the band.  Selected inside the first-pass kernel: no
 * scratch in HBM, so calls on different streams may be in flight together.  Arguments, errors and stream semantics as above */
int  fhevc_intra_first_pass_candidates_device(fhevc_ctx* ctx, const void* d_luma, int sample_bytes, int stride_samples,
                                              long long frame_stride_samples, int num_frames, int ctu_row_begin, int ctu_row_end,
                                              int qp, int num_candidates, uint8_t* d_modes, void* stream);

/* Device-resident batch: num_frames pictures already in HBM, CTU rows [ctu_row_begin, ctu_row_end) of each.
 * d_luma: sample_bytes = 2 -> int16 Pel plane(s) as HM lays them out, 1 -> uint8 (8-bit content);
 * frame f starts at d_luma + f * frame_stride_samples.  Outputs are device pointers, compact over the band:
 * entry ((f * band_rows + (row - ctu_row_begin)) * ctus_per_row + col).  d_hadamard / d_logits / d_flags may be NULL.
 * stream: hipStream_t.  NULL = the context's own stream, a BLOCKING stream: work on it is ordered after everything issued
 * earlier on the legacy default stream (stream 0) and before everything issued later on it, so a caller that lives on the
 * default stream needs no extra synchronisation; a caller on its own non-blocking stream passes that stream.
 * Asynchronous with respect to the host. */
int  fhevc_predict_frames_device(fhevc_ctx* ctx, const void* d_luma, int sample_bytes, int stride_samples,
                                 long long frame_stride_samples, int num_frames, int ctu_row_begin, int ctu_row_end,
                                 int qp, uint8_t* d_depth_map, int32_t* d_hadamard, int32_t* d_logits, uint32_t* d_flags,
                                 void* stream);

/* the same with soft decisions (see fhevc_predict_frame_range); d_depth_max may be NULL; d_flags follow d_depth_map */
int  fhevc_predict_frames_device_range(fhevc_ctx* ctx, const void* d_luma, int sample_bytes, int stride_samples,
                                       long long frame_stride_samples, int num_frames, int ctu_row_begin, int ctu_row_end,
                                       int qp, int margin_split, int margin_stop, uint8_t* d_depth_map, uint8_t* d_depth_max, int32_t* d_hadamard,
                                       int32_t* d_logits, uint32_t* d_flags, void* stream);

/* The 21 split decisions of a CTU as one word (bit 0 = 64x64, bits 1..4 = 32x32 quadrants, bits 5..20 = 16x16
 * blocks; set only under split parents, forced splits at the picture edge included): the optional d_flags output
 * above, 4 bytes per CTU instead of 256 -- what the ranks of a node all-gather.  This call expands gathered words
 * back into depth maps on the device: num_frames * numCtus words, whole pictures in CTU raster order. */
int  fhevc_expand_depth_flags_device(fhevc_ctx* ctx, const uint32_t* d_flags, int num_frames, uint8_t* d_depth_map, void* stream);

/* Adaptive-QP pre-analysis == TEncPreanalyzer::xPreanalyze (TEncPreanalyzer.cpp:64-152), called by TEncGOP before
 * compressSlice when --AdaptiveQP is on (TEncGOP.cpp: m_pcPreanalyzer->xPreanalyze(pcPic)).  max_aq_depth =
 * TEncPic's uiMaxAdaptiveQPDepth (1..4): layer d has parts of 64 >> d samples, ceil(height/P) x ceil(width/P) of
 * them, raster order.  activity: all layers concatenated (fhevc_aq_parts gives the offsets) = what
 * TEncQPAdaptationUnit::getActivity returns; avg_activity: max_aq_depth values = TEncPicQPAdaptationLayer::
 * getAvgActivity.  Doubles are bit-identical to HM's.  Picture width/height must be multiples of 8. */
int  fhevc_aq_parts(int width, int height, int max_aq_depth, long long* layer_offsets /* max_aq_depth + 1, may be NULL */);
int  fhevc_preanalyze(fhevc_ctx* ctx, const int16_t* luma, int stride_samples, int max_aq_depth,
                      double* activity, double* avg_activity);
/* == TEncCu::xComputeQP (TEncCu.cpp:1093-1117) for every AQ part: qp[i] = Clip3(-qp_bd_offset, 51, base_qp +
 * floor(6*log2(normalised activity) + 0.49999)); activity/avg_activity/qp in fhevc_preanalyze's layout.  Runs on
 * the host with the same libm calls HM makes (pow, log, floor), so the integers are HM's. */
int  fhevc_aq_qp(const double* activity, const double* avg_activity, int width, int height, int max_aq_depth,
                 int qp_adaptation_range, int base_qp, int qp_bd_offset, int8_t* qp);
/* device-resident batch; d_activity holds num_frames * fhevc_aq_parts() doubles in whole-picture layout, of which
 * this call writes the parts inside CTU rows [ctu_row_begin, ctu_row_end) */
int  fhevc_preanalyze_frames_device(fhevc_ctx* ctx, const void* d_luma, int sample_bytes, int stride_samples,
                                    long long frame_stride_samples, int num_frames, int ctu_row_begin, int ctu_row_end,
                                    int max_aq_depth, double* d_activity, void* stream);

/* ---- config 4 (P slices): source-only motion search per CU node ----------------------------------------------------
 * For every CU node of every CTU (node order as fhevc_node_cost): integer full search over [-search_range, search_range]^2
 * in the PREVIOUS ORIGINAL picture, raster order and strict "<" as TEncSearch::xPatternSearch (TEncSearch.cpp:3786-3848),
 * cost = distortion + TComRdCost::getCostOfVectorWithPredictor (TComRdCost.h:166-174; zero predictor, iCostScale 2, lambda of
 * slice QP qp), samples outside the picture replicated from the border (TComPicYuv::extendPicBorder).  Distortion
 * (fhevc_set_motion_distortion):
 *   FHEVC_MOTION_SAD   what HM's integer search uses (xPatternSearch's setDistParam selects DF_SAD, TComRdCost.cpp:205-236): in this
 *                      mode vector, distortion and cost equal what the reference's own xPatternSearch returns on the same planes;
 *   FHEVC_MOTION_SATD  (default) Hadamard SATD (TComRdCost::xGetHADs) at integer positions.  HM applies Hadamard to the fractional
 *                      refinement only (HadamardME, TEncSearch.cpp:836): this is the library's own choice, the one the P-picture
 *                      rule of fhevc_p_depth_range was fitted on.
 * HM's own search runs on reconstructed references inside its serial CTU loop; this is its source-only twin, available for
 * the whole picture before that loop starts.  search_range 1..8 in either mode; 9..64 (HM's cfg: SearchRange 64; xPatternSearch,
 * TEncSearch.cpp:3786-3848, is bit-depth agnostic) in the SAD mode: the same full search, same result as xPatternSearch over that
 * window -- 8-bit content on a kernel laid out for 16 641 vectors per node around v_qsad_pk_u16_u8 (k_motion_wide.hip), content above
 * 8 bit (16-bit planes; cfg/encoder_lowdelay_P_main10.cfg) on the 16-bit SAD kernel laid out for the wide window (k_motion.hip, round 4;
 * ~20 x slower than the byte kernel, still ~100 x HM's own search per core); 9..64 in the SATD mode: FHEVC_E_INVALID.
 * The vector costs of a wide search live in one table per context, rebuilt when (qp, search_range) differs from the previous wide call's: that call
 * waits for the device first (every earlier wide search, on any stream, still reads the old table), so it blocks the host; calls that repeat the
 * previous (qp, search_range) stay asynchronous.
 * (HM's P configuration itself runs the TZ search, cfg/encoder_lowdelay_P_main.cfg:34 FastSearch 1 -> xPatternSearchFast,
 * TEncSearch.cpp:3850: the exhaustive twin is a superset of what TZ visits and serves as a source-only feature.) */
#define FHEVC_MOTION_SATD 0
#define FHEVC_MOTION_SAD  1
int  fhevc_set_motion_distortion(fhevc_ctx* ctx, int mode);
#define FHEVC_MOTION_MAX_RANGE 8        /* SATD mode */
#define FHEVC_MOTION_SAD_MAX_RANGE 64   /* SAD mode, any bit depth */
typedef struct {
  uint32_t satd_zero;       /* distortion (SATD or SAD) at vector (0, 0) */
  uint32_t satd_best;       /* distortion at the cheapest vector */
  uint32_t cost_best;       /* its distortion + vector cost; 0xFFFFFFFF in all three for nodes crossing the picture edge */
  int16_t  mvx, mvy;        /* the cheapest vector, integer samples */
} fhevc_motion_node;
/* one picture pair, host buffers (both planes with the same stride), synchronous; out: numCtus * 85 */
int  fhevc_motion_search(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp,
                         int search_range, fhevc_motion_node* out);
/* device-resident batch (layout as fhevc_predict_frames_device): frame f = 1 .. num_frames-1 is searched in frame f-1;
 * d_out: (num_frames - 1) * band CTUs * 85 nodes in HBM */
int  fhevc_motion_search_device(fhevc_ctx* ctx, const void* d_luma, int sample_bytes, int stride_samples,
                                long long frame_stride_samples, int num_frames, int ctu_row_begin, int ctu_row_end,
                                int qp, int search_range, fhevc_motion_node* d_out, void* stream);

/* Quarter-sample refinement of the search's vectors (k_motion_refine.hip): the source-only twin of what HM's xMotionEstimation always runs behind
 * its integer search, TEncSearch::xPatternSearchFracDIF + xPatternRefinement (TEncSearch.cpp:4370-4406, :823-877).  Per CU node, around the node's
 * integer vector (mvx, mvy): the nine half-sample candidates of s_acMvRefineH (centre first, TEncSearch.cpp:51-62), then the nine quarter-sample
 * candidates of s_acMvRefineQ (in ITS order, :64-75) around the half stage's winner, strict "<" in both.  A candidate costs its Hadamard distortion
 * (TComRdCost::xGetHADs, HadamardME: ALWAYS SATD here, whatever fhevc_set_motion_distortion says) on HEVC's 8-tap luma interpolation
 * (TComInterpolationFilter; 14-bit intermediates when both fractions are non-zero) of the PREVIOUS ORIGINAL picture with coordinates clamped to the
 * picture, plus getCostOfVectorWithPredictor of the candidate in quarter units (zero predictor, lambda of slice QP qp as the search).
 * nodes: what fhevc_motion_search[_device] wrote for the same pictures and band, in either distortion mode, any search range up to 64; only mvx and
 * mvy are read.  Validity comes from the context's geometry: a node crossing the picture edge gets 0xFFFFFFFF in the three distortion fields and a
 * zero vector, and so does a node whose |mvx| or |mvy| exceeds max_range (1..64; pass the search's range), so no content of `nodes` can send a read
 * outside the staged window.  max_range <= 8 runs on a 15.5 KB window per CTU, above on an 80 KB one. */
typedef struct {
  uint32_t satd_int;        /* SATD at the integer vector (candidate 0 of the half stage) */
  uint32_t satd_best;       /* SATD at the final vector */
  uint32_t cost_best;       /* its SATD + vector cost: what xPatternSearchFracDIF returns in ruiCost; 0xFFFFFFFF in all three: see above */
  int16_t  mvx, mvy;        /* the final vector in QUARTER samples: 4 * integer + 2 * half + quarter */
} fhevc_motion_qpel_node;
/* one picture pair, host buffers (both planes with the same stride), synchronous; nodes, out: numCtus * 85 */
int  fhevc_motion_refine(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int max_range,
                         const fhevc_motion_node* nodes, fhevc_motion_qpel_node* out);
/* device-resident batch: layout, band and stream arguments as fhevc_motion_search_device; frame f = 1 .. num_frames-1 is refined in frame f-1;
 * d_nodes, d_out: (num_frames - 1) * band CTUs * 85 entries in HBM, compact over the band; d_out is written over exactly that extent, an empty band
 * writes nothing.  Asynchronous with respect to the host, allocates nothing, keeps no state in HBM between calls: calls on different streams may be
 * in flight together, and a search and its refinement may follow each other on one stream without a synchronisation.  FHEVC_E_INVALID (nothing is
 * launched or written): a null pointer, num_frames < 2, qp outside 0..51, max_range outside 1..64, stride_samples < width, a bad band, uint8 planes
 * on a context above 8 bit. */
int  fhevc_motion_refine_device(fhevc_ctx* ctx, const void* d_luma, int sample_bytes, int stride_samples,
                                long long frame_stride_samples, int num_frames, int ctu_row_begin, int ctu_row_end,
                                int qp, int max_range, const fhevc_motion_node* d_nodes, fhevc_motion_qpel_node* d_out, void* stream);

/* The same integer search for the rectangular prediction units (k_motion_pu.hip): what HM's P configuration (AMP : 1) checks per CU after 2Nx2N,
 * xCheckRDCostInter for SIZE_2NxN, SIZE_Nx2N and the four AMP shapes, each a predInterSearch with one xMotionEstimation per PU.  Per PU exactly the
 * search fhevc_motion_search defines per node: full search over [-search_range, search_range]^2 in the previous original picture, raster order,
 * strict "<", SAD or SATD as fhevc_set_motion_distortion says -- summed over the PU's 8x8 tiles and shifted ONCE by bit_depth - 8, as
 * TComRdCost::xGetHADs does for any block whose sides are multiples of 8 --, getCostOfVectorWithPredictor with a zero predictor, border replicated.
 * PU geometry as TComDataCU::getPartIndexAndSize, for a CU of size S:
 *   shape 0  SIZE_2NxN   S x S/2 top,    S x S/2 bottom        shape 3  SIZE_2NxnD  S x 3S/4 top,   S x S/4 bottom
 *   shape 1  SIZE_Nx2N   S/2 x S left,   S/2 x S right         shape 4  SIZE_nLx2N  S/4 x S left,   3S/4 x S right
 *   shape 2  SIZE_2NxnU  S x S/4 top,    S x 3S/4 bottom       shape 5  SIZE_nRx2N  3S/4 x S left,  S/4 x S right
 * Covered are the PUs whose sides are multiples of 8: shapes 0 and 1 of the 64x64, 32x32 and 16x16 nodes (nodes 0..20 of the 85), shapes 2..5 of
 * the 64x64 and 32x32 nodes (nodes 0..4): FHEVC_PUS_PER_CTU entries per CTU,
 *   nodes k = 0..4:   entry k * 12 + shape * 2 + part             nodes k = 5..20:  entry 60 + (k - 5) * 4 + shape * 2 + part
 * which is what fhevc_motion_pu_index returns (-1 for a combination that is not covered; it needs no context).
 * NOT covered by this entry point: AMP of 16x16 CUs (16x4 PUs need 4x4 Hadamards) and the 8x4 and 4x8 PUs of 8x8 CUs -- those are
 * fhevc_motion_search_pu_small's, below.  NOT covered by either: search ranges above 8 -- those are fhevc_motion_search_pu_wide's, further below
 * (SAD only, up to HM's own SearchRange 64); a
 * predictor other than zero (HM's second PU sees the first PU's vector as a candidate, this source-only twin does not).  The SEARCH stays so; its
 * refined costs are priced against such predictors afterwards by fhevc_motion_amvp*, further below.
 * An entry is a fhevc_motion_node.  A PU is valid iff its CU NODE lies wholly inside the picture (HM never codes a partitioned CU that crosses the
 * edge); otherwise the three distortion fields hold 0xFFFFFFFF and the vector is zero, as for nodes.  The encoder hook does not consume this
 * output yet: a rule that turns it into a shape mask has to be fitted on the reference's own decisions first. */
#define FHEVC_PUS_PER_CTU 124
int  fhevc_motion_pu_index(int node, int shape, int part);
/* device-resident batch; layout, band and stream arguments as fhevc_motion_search_device; frame f >= 1 searched in f-1.
 * d_pus: (num_frames-1) * band CTUs * FHEVC_PUS_PER_CTU entries, compact over the band, written over exactly that extent.
 * d_nodes: optional, (num_frames-1) * band CTUs * 85, the bytes fhevc_motion_search_device writes for the same arguments: a caller that wants both
 * pays for the tile distortions once.  Asynchronous with respect to the host, allocates nothing, keeps no state in HBM between calls (the vector
 * costs travel by value): calls on different streams may be in flight together.  An empty band writes nothing.  FHEVC_E_INVALID (nothing is
 * launched or written): a null d_luma, d_pus or context, num_frames < 2, qp outside 0..51, search_range outside 1..8, stride_samples < width, a bad
 * band, uint8 planes on a context above 8 bit. */
int  fhevc_motion_search_pu_device(fhevc_ctx* ctx, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                                   int num_frames, int ctu_row_begin, int ctu_row_end, int qp, int search_range,
                                   fhevc_motion_node* d_nodes, fhevc_motion_node* d_pus, void* stream);
/* one picture pair, host buffers, synchronous; nodes may be NULL */
int  fhevc_motion_search_pu(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range,
                            fhevc_motion_node* nodes, fhevc_motion_node* pus);

/* ... and for the PUs with a side of 4 or 12 samples (k_motion_pu_small.hip), the shapes HM's P configuration checks at the deepest levels of the
 * quad-tree: AMP of the 16x16 CUs (TEncCu.cpp:685 opens AMP for the 64x64, 32x32 AND 16x16 CUs: PUs of 16x4, 16x12, 4x16, 12x16) and the 2NxN /
 * Nx2N PUs of the 8x8 CUs (8x4, 4x8: the smallest inter PUs of HEVC).  Per PU exactly the search fhevc_motion_search defines per node: full search
 * over [-search_range, search_range]^2 (search_range 1..8) in the previous ORIGINAL picture, border replicated, raster order, strict "<", cost =
 * distortion + getCostOfVectorWithPredictor with a zero predictor and the lambda of slice QP qp, SAD or SATD as fhevc_set_motion_distortion says.
 * The distortion of a w x h PU with a side that is not a multiple of 8:
 *   SAD   the plain sum of absolute differences over the block, >> (bit_depth - 8) once;
 *   SATD  TComRdCost::xGetHADs tiles a block by 8x8 only if BOTH sides are multiples of 8; otherwise the WHOLE block goes through xCalcHADs4x4:
 *         the sum over ALL (w/4) (h/4) 4x4 tiles of the PU of (sum |H4 d H4| + 1) >> 1, shifted ONCE by bit_depth - 8.  A 16x12 PU is twelve 4x4
 *         Hadamards, not one row of 8x8 plus one of 4x4.  Consequence: the three-quarter part of an AMP shape is NOT "the node's SATD minus the
 *         quarter" -- the node's SATD (fhevc_motion_search) is built from 8x8 Hadamards; the three-quarter part is the sum of the node's sixteen
 *         4x4 Hadamards minus the quarter's four.  (In SAD mode at 8 bit the two parts of a shape do sum to the node's SAD.)
 * PU geometry and shape numbers as above (TComDataCU::getPartIndexAndSize).  FHEVC_PUS_SMALL_PER_CTU entries per CTU, each a fhevc_motion_node:
 *   nodes k = 5..20 (16x16), shapes 2..5:  entry (k - 5) * 8 + (shape - 2) * 2 + part            0..127
 *   nodes k = 21..84 (8x8),  shapes 0..1:  entry 128 + (k - 21) * 4 + shape * 2 + part           128..383
 * which is what fhevc_motion_pu_small_index returns (-1 for anything else; it needs no context).  A PU is valid iff its CU NODE lies wholly inside
 * the picture; otherwise the three distortion fields hold 0xFFFFFFFF and the vector is zero, as for nodes and for the 124 PUs.  Still left out, on
 * purpose: search ranges above 8, predictors other than zero.  (The ranges above 8 are fhevc_motion_search_pu_wide's, below, in SAD mode.)  The
 * encoder hook does not consume this output. */
#define FHEVC_PUS_SMALL_PER_CTU 384
int  fhevc_motion_pu_small_index(int node, int shape, int part);
/* device-resident batch; layout, band and stream arguments as fhevc_motion_search_pu_device; frame f >= 1 searched in f-1.
 * d_pus: (num_frames-1) * band CTUs * FHEVC_PUS_SMALL_PER_CTU entries, compact over the band, written over exactly that extent.  Asynchronous with
 * respect to the host, allocates nothing, keeps no state in HBM between calls (the vector costs travel by value): calls on different streams may
 * be in flight together.  An empty band writes nothing.  FHEVC_E_INVALID (nothing is launched or written): a null d_luma, d_pus or context,
 * num_frames < 2, qp outside 0..51, search_range outside 1..8, stride_samples < width, a bad band, uint8 planes on a context above 8 bit. */
int  fhevc_motion_search_pu_small_device(fhevc_ctx* ctx, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                                         int num_frames, int ctu_row_begin, int ctu_row_end, int qp, int search_range,
                                         fhevc_motion_node* d_pus, void* stream);
/* one picture pair, host buffers, synchronous */
int  fhevc_motion_search_pu_small(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range,
                                  fhevc_motion_node* pus);

/* The three integer searches at HM's own SearchRange: the 85 nodes, the 124 PUs and the 384 small PUs of every CTU from ONE entry point, for
 * search_range 1..64.  Per entry exactly the search fhevc_motion_search defines in its SAD mode: full search over [-search_range, search_range]^2 in
 * the previous ORIGINAL picture, border replicated, raster order, strict "<", zero predictor (iCostScale 2, the lambda of slice QP qp), distortion =
 * the SAD of the whole w x h block shifted ONCE by bit_depth - 8.  The distortion is ALWAYS SAD, whatever fhevc_set_motion_distortion says: that
 * is HM's integer-search distortion (xPatternSearch's setDistParam selects DF_SAD), the only one the reference pins, and what the square search
 * requires above +-8 too.  Each of the three outputs may be NULL, at least one must be given; a family that is not asked for is not computed:
 *   d_nodes      85 per CTU, byte for byte what fhevc_motion_search_device writes in SAD mode for the same arguments
 *   d_pus        FHEVC_PUS_PER_CTU per CTU in fhevc_motion_pu_index order, what fhevc_motion_search_pu_device writes in SAD mode up to range 8
 *   d_pus_small  FHEVC_PUS_SMALL_PER_CTU per CTU in fhevc_motion_pu_small_index order, likewise
 * Validity, markers, the compact-over-band layout and the exact write extent are those of the PU searches above.  Ranges up to 8 run the kernels of
 * those entry points.  Above, 8-bit contexts (int16 or uint8 planes) run k_motion_pu_wide.hip, the byte-SAD layout of the square wide search
 * (v_qsad_pk_u16_u8; quadrant SADs per tile, running sums per level), in one launch instantiated for the families asked for; contexts above 8 bit
 * run the kernels of the PU searches laid out for a window of up to 192 x 192 samples in LDS (k_motion_pu.hip, k_motion_pu_small.hip at MR = 64),
 * one launch for nodes and PUs and one for the small PUs; FHEVC_PU_WIDE=generic in the environment of fhevc_create sends 8-bit int16 planes down
 * that path too (tests, A/B timing; the bytes are the same).  NO state is kept between
 * calls and nothing is synchronised: the vector cost depends only on the exp-Golomb bits of the two components, 2 floor(log2 t) + 1 with
 * t = v <= 0 ? (-v << 3) + 1 : v << 3, and the cost of every number of bits travels by value with the launch -- unlike fhevc_motion_search_device
 * above +-8, whose per-context table of vector costs blocks the host when (qp, search_range) changes.  Two calls with different QPs and ranges may be
 * in flight on two streams.  Asynchronous with respect to the host, allocates nothing.  An empty band writes nothing.  FHEVC_E_INVALID with a
 * fhevc_last_error text (nothing is launched or written): a null context or d_luma, all three outputs null, num_frames < 2, qp outside 0..51,
 * search_range outside 1..64, stride_samples < width, a bad band, uint8 planes on a context above 8 bit.  Not covered: the quarter-sample refinement
 * of PU vectors beyond +-8 (fhevc_motion_refine_pu marks them), SATD at integer positions above +-8, predictors other than zero.  The encoder hook
 * does not consume this output.  (Since then: fhevc_motion_refine_pu_wide, below, refines the vectors of all three outputs at max_range 1..64.) */
int  fhevc_motion_search_pu_wide_device(fhevc_ctx* ctx, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                                        int num_frames, int ctu_row_begin, int ctu_row_end, int qp, int search_range,
                                        fhevc_motion_node* d_nodes, fhevc_motion_node* d_pus, fhevc_motion_node* d_pus_small, void* stream);
/* one picture pair, host buffers, synchronous; each output may be NULL, not all three */
int  fhevc_motion_search_pu_wide(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range,
                                 fhevc_motion_node* nodes, fhevc_motion_node* pus, fhevc_motion_node* pus_small);

/* Quarter-sample refinement of the PUs' vectors (k_motion_refine_pu.hip): HM never compares partition shapes at integer positions -- every
 * xMotionEstimation runs TEncSearch::xPatternSearchFracDIF behind the integer search, for every PU, 8x4 and 4x8 included, and xCheckRDCostInter sees each
 * PU's Hadamard cost at its quarter-sample vector.  This is the definition of fhevc_motion_refine per PU instead of per node, for all 508 PUs of a CTU:
 * around the PU's integer vector (mvx, mvy) the nine half-sample candidates of s_acMvRefineH (centre first), then the nine quarter-sample candidates
 * of s_acMvRefineQ (in ITS order) around the half stage's winner, strict "<" in both; prediction by HEVC's 8-tap luma interpolation of the PREVIOUS
 * ORIGINAL picture with coordinates clamped to the picture (14-bit intermediates when both fractions are non-zero); vector cost
 * getCostOfVectorWithPredictor of the candidate in quarter units (zero predictor, lambda of slice QP qp).  Distortion: ALWAYS TComRdCost::xGetHADs on the
 * whole w x h PU, whatever fhevc_set_motion_distortion says, through the branch xGetHADs itself takes:
 *   both sides multiples of 8 (all 124 PUs of fhevc_motion_pu_index):  the sum over the PU's 8x8 tiles of (sum |H8 d H8| + 2) >> 2;
 *   otherwise (all 384 PUs of fhevc_motion_pu_small_index, the 16x12 and 12x16 parts included):  the sum over ALL (w/4) (h/4) 4x4 tiles of
 *   (sum |H4 d H4| + 1) >> 1 -- a 16x12 part is twelve 4x4 Hadamards, not the node minus the quarter;
 * in both cases the PU's sum is shifted ONCE by bit_depth - 8.  PU geometry and entry order are exactly those of fhevc_motion_pu_index (pus, out_pus:
 * FHEVC_PUS_PER_CTU entries per CTU) and fhevc_motion_pu_small_index (pus_small, out_pus_small: FHEVC_PUS_SMALL_PER_CTU).  Input entries are what the
 * two PU searches wrote for the same pictures and band, in either distortion mode; only mvx and mvy are read.  A PU is valid iff its CU node lies
 * wholly inside the picture and |mvx|, |mvy| <= max_range (1..8: no PU search writes longer vectors, so the 15.5 KB window serves); an invalid PU gets
 * 0xFFFFFFFF in the three distortion fields and a zero vector, so no content of the input can send a read outside the staged window.  Output entries
 * are fhevc_motion_qpel_node.  Either family's in / out pair may be NULL together: that family's work is then not done at all.  Vectors of the search
 * ranges above 8 (fhevc_motion_search_pu_wide) are fhevc_motion_refine_pu_wide's, below.
 * One picture pair, host buffers (both planes with the same stride), synchronous: */
int  fhevc_motion_refine_pu(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int max_range,
                            const fhevc_motion_node* pus, fhevc_motion_qpel_node* out_pus,
                            const fhevc_motion_node* pus_small, fhevc_motion_qpel_node* out_pus_small);
/* device-resident batch: layout, band and stream arguments as fhevc_motion_refine_device and fhevc_motion_search_pu_device; frame f = 1 .. num_frames-1
 * is refined in frame f-1; d_pus, d_out_pus: (num_frames - 1) * band CTUs * 124 entries, d_pus_small, d_out_pus_small: ... * 384, compact over the band;
 * the outputs are written over exactly that extent, an empty band writes nothing.  Asynchronous with respect to the host, allocates nothing, keeps no
 * state in HBM between calls (the vector costs travel by value): calls on different streams may be in flight together, and a PU search and its
 * refinement may follow each other on one stream without a host synchronisation.  FHEVC_E_INVALID (nothing is launched or written): a null context or
 * d_luma, both pairs null, a pair with exactly one null member, num_frames < 2, qp outside 0..51, max_range outside 1..8, stride_samples < width, a bad
 * band, uint8 planes on a context above 8 bit. */
int  fhevc_motion_refine_pu_device(fhevc_ctx* ctx, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                                   int num_frames, int ctu_row_begin, int ctu_row_end, int qp, int max_range,
                                   const fhevc_motion_node* d_pus, fhevc_motion_qpel_node* d_out_pus,
                                   const fhevc_motion_node* d_pus_small, fhevc_motion_qpel_node* d_out_pus_small, void* stream);

/* The quarter-sample refinements at HM's own SearchRange: the counterpart of fhevc_motion_search_pu_wide, whose three outputs feed straight in.  max_range 1..64.
 * Per entry the definition is exactly that of fhevc_motion_refine for the 85 nodes and of fhevc_motion_refine_pu for the 124 PUs and the 384 small PUs: the
 * half-sample stage of s_acMvRefineH, then the quarter-sample stage of s_acMvRefineQ around its winner, strict "<" in both; TComRdCost::xGetHADs on the whole
 * block through the branch xGetHADs itself takes (8x8 tiles where both sides are multiples of 8, otherwise 4x4 tiles), shifted ONCE by bit_depth - 8; ALWAYS
 * SATD, whatever fhevc_set_motion_distortion says; zero predictor, the lambda of slice QP qp; coordinates clamped to the picture.  An entry is valid iff its
 * CU node lies wholly inside the picture and |mvx|, |mvy| <= max_range; an invalid one gets 0xFFFFFFFF in the three distortion fields and a zero vector, so no
 * content of the input can send a read outside the staged window.  Only mvx and mvy of the input entries are read.
 *   d_nodes, d_out_nodes          85 per CTU: a second launch on the same stream of the kernel behind fhevc_motion_refine_device; the result is byte for byte
 *                                 what that entry point writes for the same arguments
 *   d_pus, d_out_pus              FHEVC_PUS_PER_CTU per CTU in fhevc_motion_pu_index order
 *   d_pus_small, d_out_pus_small  FHEVC_PUS_SMALL_PER_CTU per CTU in fhevc_motion_pu_small_index order; both PU families in one launch.  At max_range <= 8
 *                                 the PU outputs are byte for byte what fhevc_motion_refine_pu_device writes; above, k_motion_refine_pu.hip runs laid out for
 *                                 vectors up to +-64 (a window of 200 x 200 samples, 80 016 B of LDS, of which the part max_range reaches is staged)
 * Each in / out pair may be NULL together: a family that is not asked for is neither computed nor written.  All three pairs NULL, or a pair with exactly
 * one NULL member, is FHEVC_E_INVALID.  Entry order, the compact-over-band layout ((num_frames - 1) * band CTUs * 85 / 124 / 384 entries; frame
 * f = 1 .. num_frames-1 is refined in frame f-1), the exact write extent and the empty band that writes nothing are those of the existing refinements.
 * Asynchronous with respect to the host, allocates nothing, keeps NO state in HBM between calls (the vector costs travel by value) and synchronises nothing:
 * calls with different QPs and ranges may be in flight on two streams, and a wide search and its refinement may follow each other on one stream without a host
 * synchronisation.  FHEVC_E_INVALID with a fhevc_last_error text (nothing is launched or written): a null context or d_luma, all three pairs null, a pair
 * with exactly one null member, num_frames < 2, qp outside 0..51, max_range outside 1..64, stride_samples < width, a bad band, uint8 planes on a context above
 * 8 bit.  Timed under slot 12 of fhevc_kernel_timing, each launch counted.  The encoder hook does not consume this output.  (Since then:
 * fhevc_pu_shape_select_device, further below, adds these costs up per partition size and turns them into a mask, on the device.) */
int  fhevc_motion_refine_pu_wide_device(fhevc_ctx* ctx, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                                        int num_frames, int ctu_row_begin, int ctu_row_end, int qp, int max_range,
                                        const fhevc_motion_node* d_nodes, fhevc_motion_qpel_node* d_out_nodes,
                                        const fhevc_motion_node* d_pus, fhevc_motion_qpel_node* d_out_pus,
                                        const fhevc_motion_node* d_pus_small, fhevc_motion_qpel_node* d_out_pus_small, void* stream);
/* one picture pair, host buffers (both planes with the same stride), synchronous; each in / out pair may be NULL together, not all three */
int  fhevc_motion_refine_pu_wide(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int max_range,
                                 const fhevc_motion_node* nodes, fhevc_motion_qpel_node* out_nodes,
                                 const fhevc_motion_node* pus, fhevc_motion_qpel_node* out_pus,
                                 const fhevc_motion_node* pus_small, fhevc_motion_qpel_node* out_pus_small);

/* One coarse motion centre per CTU (k_motion_coarse.hip): where a search around a predictor would start.  Every search and refinement above looks around
 * the ZERO vector and prices vectors against a zero predictor, so real motion is reachable only by widening the window (the +-64 search costs about twenty
 * times the +-8 one).  HM centres its window on the motion-vector predictor (xSetSearchRange, TComRdCost::setPredictor), which comes from the neighbouring
 * PUs' CODED vectors; a source-only pass has none.  This definition therefore has NO HM counterpart and is pinned to no reference: it is this library's
 * own, restated in tests/motion_centred_ref.py.  Per CTU (cx, cy) of the current picture p, searched in the previous ORIGINAL picture:
 *   decimated picture  D_p(X, Y) = (sum of the 4x4 samples at (4X.., 4Y..) + 8) >> 4 for the floor(width / 4) x floor(height / 4) cells that lie wholly
 *                      inside the picture; a cell coordinate outside that grid is clamped to it (border replication on the decimated grid)
 *   current cells      the CTU owns cells (16 cx + i, 16 cy + j), i, j < 16; only those inside the grid count (a ragged CTU has fewer)
 *   candidates         d in [-coarse_range, coarse_range]^2 in raster order (dy outer, dx inner), strict "<":
 *                        sad(d)  = (16 * sum over the counted cells of |D_cur(X, Y) - D_ref(X + dx, Y + dy)|) >> (bit_depth - 8)
 *                        cost(d) = sad(d) + c[bits(4 dx) + bits(4 dy)]
 *                      with c[b] = getCost(b) at the lambda of slice QP qp and bits(v) = 2 floor(log2 t) + 1, t = v <= 0 ? (-v << 3) + 1 : v << 3: the
 *                      whole-sample vector 4 d against a zero predictor at iCostScale 2, as fhevc_motion_search_pu_wide prices it.  Flat content lands on zero
 *   record             satd_zero = sad(0), satd_best = sad at the winner, cost_best, (mvx, mvy) = 4 d in whole samples: multiples of 4 within +-56
 * coarse_range is 1..14, in cells.  A CTU that owns no cell (picture width or height of 1..3 modulo 64) has nothing to compare: it gets 0xFFFFFFFF in the
 * three distortion fields and a zero vector.  int16 or uint8 planes, 8 to 12 bit.
 * Device form: layout, band and stream arguments as fhevc_motion_search_pu_wide_device; frame f >= 1 is searched in frame f-1.  d_centres:
 * (num_frames-1) * band CTUs entries (ONE per CTU), compact over the band, written over exactly that extent; an empty band writes nothing.  Asynchronous with
 * respect to the host, allocates nothing, keeps NO state between calls (the bit costs travel by value): calls with different QPs and ranges may be in flight on
 * two streams.  FHEVC_E_INVALID with a fhevc_last_error text (nothing is launched or written): a null context, d_luma or d_centres, num_frames < 2, qp
 * outside 0..51, coarse_range outside 1..14, stride_samples < width, a bad band, uint8 planes on a context above 8 bit.  Timed under slot 15 of
 * fhevc_kernel_timing.
 * NOT covered: per-32x32 centres; anything but fhevc_motion_search_pu_centred and fhevc_motion_refine_pu_centred, below, consuming them (the encoder hook,
 * the P rule -- fitted on zero-predictor features --, fhevc_p_shape_frame keep the zero predictor). */
int  fhevc_motion_centres_device(fhevc_ctx* ctx, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                                 int num_frames, int ctu_row_begin, int ctu_row_end, int qp, int coarse_range, fhevc_motion_node* d_centres, void* stream);
/* one picture pair, host buffers (both planes with the same stride), synchronous; centres: numCtus entries */
int  fhevc_motion_centres(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int coarse_range,
                          fhevc_motion_node* centres);

/* The three integer searches AROUND A CENTRE per CTU: what fhevc_motion_search_pu_wide does around the zero vector, in a window of +-search_range (1..8) around
 * the CTU's entry of d_centres -- fhevc_motion_centres' output, or any vectors of the caller's.  This is HM's arrangement: xMotionEstimation centres its
 * window on the predictor (xSetSearchRange) and prices vectors against it (TComRdCost::setPredictor); here the predictor of every entry of a CTU is the CTU's
 * centre P.  Arguments, optional outputs (each may be NULL, not all three), entry order, layouts, validity, markers and the exact write extent are those of
 * fhevc_motion_search_pu_wide_device.  Per entry:
 *   candidates    v = P + d for d in [-search_range, search_range]^2, in raster order over d, strict "<"
 *   distortion    ALWAYS the SAD of the whole w x h block at v, reference coordinates clamped to the picture, the sum shifted ONCE by bit_depth - 8
 *   cost          SAD + c[bits(dx) + bits(dy)]: exactly getCostOfVectorWithPredictor with the predictor 4 P in quarter units at iCostScale 2 (the lambda of
 *                 slice QP qp)
 *   record        mvx, mvy = v, ABSOLUTE; satd_best, cost_best; satd_zero = the SAD AT THE CENTRE (d = 0), not at the zero vector -- with a zero centre
 *                 the two are the same, and the whole output is byte for byte fhevc_motion_search_pu_wide_device's for the same search_range
 * d_centres: (num_frames-1) * band CTUs entries, compact over the band, never NULL, 4-byte aligned; only mvx / mvy are read.  If a component of a CTU's
 * centre lies outside [-56, 56], all 593 entries of that CTU get the marker (0xFFFFFFFF three times, a zero vector) and nothing is read for it: 56 + 8 stays
 * within HM's SearchRange 64, which is what the refinement's layouts hold.  The kernels decide this, the host never sees device centres.  The marker record
 * fhevc_motion_centres writes for a CTU that owns no cell carries a zero vector, and only the vector is read: such a CTU is searched around (0, 0).
 * The MR = 8 layouts of k_motion_pu.hip and k_motion_pu_small.hip with the window's origin and its 8-sample phase taken per CTU; one launch for nodes and
 * PUs, one for the small PUs.  Asynchronous with respect to the host, allocates nothing, keeps NO state between calls (the window's vector costs travel by
 * value): calls with different QPs, ranges and centres may be in flight on two streams, and fhevc_motion_centres_device and this search may follow each other
 * on one stream without a host synchronisation.  An empty band writes nothing.  FHEVC_E_INVALID with a fhevc_last_error text (nothing is launched or
 * written): what fhevc_motion_search_pu_wide_device rejects, a null d_centres, search_range outside 1..8.  Timed under slot 15 of fhevc_kernel_timing, each
 * launch counted.
 * NOT covered: search ranges above 8 around a centre; a centred fhevc_p_shape_frame; the encoder hook; the P rule.  (The refinement priced against 4 P is
 * fhevc_motion_refine_pu_centred, below.)  (Since then: fhevc_p_tree_frame, further below, runs the centred chain end to end from host buffers.) */
int  fhevc_motion_search_pu_centred_device(fhevc_ctx* ctx, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                                           int num_frames, int ctu_row_begin, int ctu_row_end, int qp, int search_range, const fhevc_motion_node* d_centres,
                                           fhevc_motion_node* d_nodes, fhevc_motion_node* d_pus, fhevc_motion_node* d_pus_small, void* stream);
/* one picture pair, host buffers, synchronous; centres: numCtus entries; each output may be NULL, not all three */
int  fhevc_motion_search_pu_centred(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range,
                                    const fhevc_motion_node* centres, fhevc_motion_node* nodes, fhevc_motion_node* pus, fhevc_motion_node* pus_small);

/* The quarter-sample refinements AROUND A CENTRE per CTU: the counterpart of fhevc_motion_search_pu_centred, whose three outputs feed straight in.  The contract is
 * that of fhevc_motion_refine_pu_wide_device -- the half-sample stage of s_acMvRefineH, then the quarter-sample stage of s_acMvRefineQ around its winner, strict
 * "<" in both; TComRdCost::xGetHADs on the whole block through the branch xGetHADs itself takes, shifted ONCE by bit_depth - 8; ALWAYS SATD; HEVC's 8-tap
 * interpolation of the previous ORIGINAL picture with coordinates clamped to the picture; the three in / out pairs, each NULL together, not all three; entry
 * order, layouts, the exact write extent -- with max_range 1..8 and three differences, P being the CTU's entry of d_centres:
 *   validity     an entry is valid iff its CU node lies wholly inside the picture, both components of P lie in [-56, 56], and |mvx - Px|, |mvy - Py| <=
 *                max_range; any other entry gets 0xFFFFFFFF in the three distortion fields and a zero vector (an out-of-range centre: all 593 entries of its
 *                CTU, and nothing is read for it)
 *   vector cost  of a candidate q in quarter units: c[bits_q(qx - 4 Px) + bits_q(qy - 4 Py)], bits_q the exp-Golomb bits fhevc_motion_refine counts:
 *                getCostOfVectorWithPredictor with the predictor 4 P
 *   vectors      input and output vectors are ABSOLUTE (the output in quarter units), as fhevc_motion_search_pu_centred writes them
 * With zero centres the output is byte for byte fhevc_motion_refine_pu_wide_device's for the same max_range, so fhevc_pu_shape_select_device consumes it
 * unchanged.  The MR = 8 layouts of k_motion_refine.hip and k_motion_refine_pu.hip with the window staged around P and vectors relative to P inside the kernel
 * (DESIGN.md says why not the MR = 64 layouts on absolute vectors); one launch for the nodes, one for both PU families.  d_centres as for the centred search (never
 * NULL, 4-byte aligned, only mvx / mvy read).  Asynchronous with respect to the host, allocates nothing, keeps NO state between calls: calls with different QPs, ranges
 * and centres may be in flight on two streams; centres, centred search, this refinement and fhevc_pu_shape_select_device may follow each other on one stream
 * without a host synchronisation.  FHEVC_E_INVALID with a fhevc_last_error text (nothing is launched or written): what fhevc_motion_refine_pu_wide_device
 * rejects, a null d_centres, max_range outside 1..8.  Timed under slot 15 of fhevc_kernel_timing, each launch counted.
 * NOT covered: max_range above 8 around a centre; a centred fhevc_p_shape_frame; the encoder hook; the P rule.  (Since then: fhevc_p_tree_frame, further below, runs
 * centres, centred search, this refinement, the selection and the tree decision as one call from host buffers.) */
int  fhevc_motion_refine_pu_centred_device(fhevc_ctx* ctx, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                                           int num_frames, int ctu_row_begin, int ctu_row_end, int qp, int max_range, const fhevc_motion_node* d_centres,
                                           const fhevc_motion_node* d_nodes, fhevc_motion_qpel_node* d_out_nodes,
                                           const fhevc_motion_node* d_pus, fhevc_motion_qpel_node* d_out_pus,
                                           const fhevc_motion_node* d_pus_small, fhevc_motion_qpel_node* d_out_pus_small, void* stream);
/* one picture pair, host buffers (both planes with the same stride), synchronous; centres: numCtus entries; each in / out pair may be NULL together, not all three */
int  fhevc_motion_refine_pu_centred(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int max_range,
                                    const fhevc_motion_node* centres, const fhevc_motion_node* nodes, fhevc_motion_qpel_node* out_nodes,
                                    const fhevc_motion_node* pus, fhevc_motion_qpel_node* out_pus,
                                    const fhevc_motion_node* pus_small, fhevc_motion_qpel_node* out_pus_small);

/* Depth range of every 4x4 unit of a P picture's CTU from its motion nodes and the co-located depths of its reference picture
 * ("inter-CU depth reuse", BASELINE config 4).  Host-side integer arithmetic, no device work.  Per split decision (64->32,
 * 32->16, 16->8) a linear score over nine features of the node, all in 1/256 units (L(x) = floor(256 log2 x) by integer
 * squaring, lgN = 2 * 256 * log2(node size), qn = 256 * qp / 6):
 *   f0 = L(satd_best + 1) - lgN - qn          residual per sample against the quantiser step
 *   f1 = L(cost_best - sum of the four children's cost_best (clamped at 0) + 1) - lgN - qn     what splitting the search gains
 *   f2 = L(sum of the children's satd_best + 1) - lgN - qn
 *   f3 = L(satd_zero + 1) - L(satd_best + 1)  how much motion compensation helps at all
 *   f4, f5 = 256 if the largest / smallest co-located depth of the reference picture inside the node is deeper than the node
 *   f6 = 256 if the largest co-located depth is at least two levels deeper
 *   f7 = 64 * number of children whose cheapest vector differs from the node's
 *   f8 = 8 * qp
 * score = sum w[level][i] * f_i + w[level][9]   (Q18).  depth_min follows the splits with score > t_split[level] top-down,
 * depth_max those with score >= -t_stop[level]; CUs crossing the picture edge are split in both, units outside get 0; then
 * both are clipped to the co-located depth +- window when window < 4.  The xCompressCU hook forces a split while depth <
 * depth_min and forbids one at depth >= depth_max (as for I pictures).  Device form: fhevc_p_depth_range_device. */
typedef struct {
  int32_t w[3][10];
  int32_t t_split[3], t_stop[3];
  int32_t window;
} fhevc_p_rule;
void fhevc_p_rule_default(fhevc_p_rule* rule);   /* the shipped rule (fitted on the reference's own P-picture decisions) */
/* the same rule fitted on SAD-mode features of the +-64 search with the reference picture's depths taken at the motion-compensated position
 * (fhevc_p_motion_compensated_depth): what goes with search ranges above 8 */
void fhevc_p_rule_default_wide(fhevc_p_rule* rule);
int  fhevc_p_depth_range(const fhevc_motion_node* nodes /* 85 */, const uint8_t* prev_depth /* 256, raster */, int valid_w,
                         int valid_h, int qp, const fhevc_p_rule* rule, uint8_t* depth_min /* 256 */, uint8_t* depth_max /* 256 */);

/* "Inter-CU depth reuse" for content that moves: the reference picture's depths seen THROUGH the motion.  For every 4x4 unit of CTU `ctu`
 * (raster CTU index) the depth the reference picture's map holds where the unit's centre lands when displaced by the cheapest vector
 * of the 16x16 node the unit lies in (a node crossing the picture edge: the vector of its 32x32 node, then of the CTU, then zero),
 * positions clamped to the picture.  prev_map: numCtus * 256 depths of the reference picture (raster per CTU, as fhevc_predict_frame writes
 * them and TComDataCU::getDepth holds them); out: 256, the prev_depth argument of fhevc_p_depth_range.  With zero vectors this is the
 * co-located map.  Host-side integer logic, no device work, no context.  Device form: fhevc_p_depth_range_device with FHEVC_P_PREV_UNIT. */
int  fhevc_p_motion_compensated_depth(const fhevc_motion_node* nodes /* 85 */, const uint8_t* prev_map, int width, int height, int ctu,
                                      uint8_t* out /* 256 */);

/* The same through the CU NODES of the current picture (round 4): a displaced depth map is not aligned to the current picture's CU grid -- a 64x64 CU of the
 * reference picture lands on two half CTUs here -- and forcing such a map costs more than the co-located one (HISTORY.md section 4b).  This form asks, top-down
 * per node of CTU `ctu`, for the reference picture's depth at the node's CENTRE displaced by the node's cheapest vector (a node crossing the picture edge: its
 * parent's vector; the CTU node: zero): a node whose answer is not deeper than its own level becomes one CU of that depth, otherwise its four children are
 * asked (16x16 nodes: depth 2, or 3 when the answer is 3).  out is a quadtree-consistent partition on the CURRENT grid.  With zero vectors and a prev_map
 * that is itself a partition this is the co-located map.  Measured (profiles/r04_p_slice_node_*.json): one global pan of 32 samples per picture
 * -0.26 % BD-rate with the +-1 window where the per-unit form costs +1.76 % and the co-located map -0.10 %; elsewhere equal to the co-located map.
 * Device form: fhevc_p_depth_range_device with FHEVC_P_PREV_NODE. */
int  fhevc_p_node_depth(const fhevc_motion_node* nodes /* 85 */, const uint8_t* prev_map, int width, int height, int ctu, uint8_t* out /* 256 */);

/* The P-picture decision over a device-resident batch (k_p_rule.hip): one launch turns the motion nodes of num_pictures P pictures into their depth
 * ranges, without the host in between.  Per CTU the same bits as the host functions above: the reference picture's depths as prev_mode says,
 *   FHEVC_P_PREV_COLOCATED  the CTU's own 256 bytes of the reference map,
 *   FHEVC_P_PREV_UNIT       fhevc_p_motion_compensated_depth,
 *   FHEVC_P_PREV_NODE       fhevc_p_node_depth,
 * then fhevc_p_depth_range with the valid width / height the context's geometry gives the CTU.
 * d_nodes: num_pictures * band CTUs * 85 nodes, compact over the band: what fhevc_motion_search_device writes for the same (ctu_row_begin, ctu_row_end);
 * its output for num_frames frames is the input for num_pictures = num_frames - 1.  d_prev_maps: WHOLE pictures, num_pictures * numCtus * 256 bytes
 * (values 0..3), picture p of the batch is decided against map p; the two displaced modes read outside the band.  It must not overlap the outputs: a
 * caller that chains picture by picture issues one call per picture on one stream.  d_depth_min / d_depth_max (may be NULL): compact over the band,
 * entry ((p * band_rows + row - ctu_row_begin) * ctus_per_row + col) * 256, written over exactly that extent; an empty band writes nothing.
 * rule: HOST memory, read during the call (it travels to the kernel by value, so calls with different rules may follow each other on any streams
 * without synchronisation); NULL = fhevc_p_rule_default.  Stream semantics as fhevc_predict_frames_device (NULL = the context's blocking stream);
 * asynchronous with respect to the host; runs on device_ids[0].  FHEVC_E_INVALID (nothing is launched or written): a null pointer other than rule
 * and d_depth_max, num_pictures < 1, qp outside 0..51, an unknown prev_mode, a bad band. */
#define FHEVC_P_PREV_COLOCATED 0
#define FHEVC_P_PREV_UNIT      1
#define FHEVC_P_PREV_NODE      2
int  fhevc_p_depth_range_device(fhevc_ctx* ctx, const fhevc_motion_node* d_nodes, const uint8_t* d_prev_maps, int num_pictures,
                                int ctu_row_begin, int ctu_row_end, int qp, int prev_mode, const fhevc_p_rule* rule,
                                uint8_t* d_depth_min, uint8_t* d_depth_max, void* stream);
/* One picture pair, host buffers, synchronous: uploads both planes (same stride) and prev_map (numCtus * 256, the reference picture's depths),
 * searches (search_range and distortion as fhevc_motion_search), decides on the device and downloads only the two maps (numCtus * 256 each):
 * 512 bytes per CTU come back instead of the 1 360 bytes of nodes. */
int  fhevc_p_predict_frame(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range,
                           const uint8_t* prev_map, int prev_mode, const fhevc_p_rule* rule, uint8_t* depth_min, uint8_t* depth_max);

/* ---- config 4 (P slices): partition sizes per CU from the refined PU costs (k_pu_shape.hip) ---------------------------------------
 * HM's xCompressCU runs one xCheckRDCostInter, with a motion estimation per PU, for up to seven partition sizes per CU.  What this library offers per
 * partition size is the sum of its PUs' refined costs; this entry point adds the parts up per partition size on the device and decides which sizes HM
 * should check.  Partition sizes carry HM's PartSize numbers (TypeDef.h), so a hook can use the mask as it is; 3 (SIZE_NxN) is never produced.  The
 * library's shape number of fhevc_motion_pu_index is p - 1 for p = 1, 2 and p - 2 for p = 4..7. */
#define FHEVC_PART_2Nx2N 0
#define FHEVC_PART_2NxN  1
#define FHEVC_PART_Nx2N  2
#define FHEVC_PART_2NxnU 4
#define FHEVC_PART_2NxnD 5
#define FHEVC_PART_nLx2N 6
#define FHEVC_PART_nRx2N 7
/* Cost table: cost[k][p] per CU node k (0..84, node order as everywhere) and partition size p (0..7), u32, 0xFFFFFFFF = unavailable.
 *   p = 0             cost_best of refined node k (nodes[k])
 *   p = 1, 2, 4..7    cost_best(part 0) + cost_best(part 1) of that shape's two PUs: unavailable if either part carries the 0xFFFFFFFF marker, otherwise
 *                     the 64-bit sum saturated at 0xFFFFFFFE (so a sum is never mistaken for the marker).  The parts, by the formulas of
 *                     fhevc_motion_pu_index (pus) and fhevc_motion_pu_small_index (pus_small), shape = p - 1 (p <= 2) or p - 2:
 *                       k = 0..4     pus[k * 12 + shape * 2 + part]
 *                       k = 5..20    p = 1, 2: pus[60 + (k - 5) * 4 + shape * 2 + part];  p = 4..7: pus_small[(k - 5) * 8 + (shape - 2) * 2 + part]
 *                       k = 21..84   p = 1, 2: pus_small[128 + (k - 21) * 4 + shape * 2 + part];  p = 4..7 unavailable (HM opens AMP only above the
 *                                    smallest CU)
 *   p = 3             always unavailable
 * With pus_small == NULL everything taken from it is unavailable.  Level l = 0, 1, 2, 3 for k = 0, 1..4, 5..20, 21..84.
 * A node is valid iff it lies wholly inside the picture, as for every motion entry point; an invalid node gets all eight costs 0xFFFFFFFF,
 * best = second = 255, mask = avail = 0 and 0xFFFFFFFF in the three cost fields of its record.
 * best / second are selected in HM's checking order 0, 2, 1, 4, 5, 6, 7 with strict "<": the order of the inter checks in TEncCu::xCompressCU as
 * hm_patch/restore_inter.py puts them back (Nx2N before 2NxN, then the AMP pairs), and xCheckBestMode replaces only on a strictly smaller cost.
 * second runs the same scan with best removed. */
typedef struct {
  uint32_t cost_2Nx2N;      /* cost[k][0] */
  uint32_t cost_best;       /* smallest available cost */
  uint32_t cost_second;     /* smallest available cost among the other sizes, 0xFFFFFFFF if none */
  uint8_t  best, second;    /* their PartSize numbers, 255 if none */
  uint8_t  mask;            /* bit p: HM should check PartSize p */
  uint8_t  avail;           /* bit p: cost[k][p] is available */
} fhevc_pu_shape_node;      /* 16 bytes */
/* Mask of a valid node: bit 0 is always set (HM always checks 2Nx2N, even when cost[k][0] is the marker); bit p of an available p is set iff
 *   cost[k][p] <= cost_best + margin_abs[l] + ((cost_best * margin_q8[l]) >> 8)        evaluated in 64 bits.
 * With amp_mode == 1 the gate of TEncCu::deriveTestModeAMP (TEncCu.cpp:426-438) is applied afterwards: let b3 be the argmin over p in {0, 2, 1}, in that
 * order, strict "<", available ones only; bits 4 and 5 are cleared unless b3 is 0 or 1, bits 6 and 7 unless b3 is 0 or 2; none of the three available:
 * all four AMP bits are cleared.  HM's extra conditions on the merge and skip flags of the best mode are not visible to a source-only pass and are
 * not modelled. */
typedef struct {
  int32_t margin_q8[4];     /* per level, 0..65535: relative margin in 1/256 of cost_best */
  int32_t margin_abs[4];    /* per level, cost units, >= 0 */
  int32_t amp_mode;         /* 0 or 1 */
} fhevc_pu_shape_rule;
/* margins 0, amp_mode 1: the UNFITTED hard decision (only the sizes that tie with the cheapest one, behind HM's AMP gate) -- not a tuned default; margins
 * have to be fitted on the reference's own partition choices first */
void fhevc_pu_shape_rule_default(fhevc_pu_shape_rule* rule);
/* One CTU, host-side integer logic, no context, no device work (the twin of the kernel, as fhevc_p_depth_range is of k_p_rule.hip).  nodes / pus / pus_small:
 * the refined entries of the CTU (fhevc_motion_refine*, fhevc_motion_refine_pu*); only cost_best is read.  valid_w / valid_h: the CTU's samples inside the
 * picture (8..64).  out: 85 records; costs: the 85 x 8 table, or NULL.  FHEVC_E_INVALID: a null nodes, pus, rule or out, valid_w / valid_h outside 8..64, a
 * margin outside its range, amp_mode outside 0..1. */
int  fhevc_pu_shape_select(const fhevc_motion_qpel_node* nodes /* 85 */, const fhevc_motion_qpel_node* pus /* 124 */,
                           const fhevc_motion_qpel_node* pus_small /* 384 or NULL */, int valid_w, int valid_h, const fhevc_pu_shape_rule* rule,
                           fhevc_pu_shape_node* out /* 85 */, uint32_t* costs /* 85 * 8 or NULL */);
/* Device form (k_pu_shape.hip): the same bits per CTU with the valid width / height the context's geometry gives it.  d_nodes / d_pus / d_pus_small (may be
 * NULL): num_pictures * band CTUs * 85 / 124 / 384 entries, compact over the band: exactly what fhevc_motion_refine_pu_wide_device writes for
 * num_frames = num_pictures + 1 (or the MR = 8 refinements plus fhevc_motion_refine_device).  d_shapes: num_pictures * band CTUs * 85 records; d_costs (may be
 * NULL): ... * 85 * 8 dwords; both written over exactly that extent, an empty band writes nothing.  rule: HOST memory, read during the call (it travels to the
 * kernel by value); NULL = fhevc_pu_shape_rule_default.  Asynchronous with respect to the host, allocates nothing, keeps no state: calls with different rules
 * may be in flight on two streams.  Stream semantics as fhevc_p_depth_range_device (NULL = the context's blocking stream), so a wide search, its refinement
 * and the selection may follow each other on one stream without a host synchronisation.  The entries may have any alignment their type allows (4 bytes);
 * where d_shapes and d_costs are 16-byte aligned the outputs leave as 16-byte stores, as dwords otherwise; the bytes written are the same.  Timed under slot 13 of
 * fhevc_kernel_timing.  FHEVC_E_INVALID with a fhevc_last_error text (nothing is launched or written): a null context, d_nodes, d_pus or d_shapes,
 * num_pictures < 1, a bad band, a margin outside its range, amp_mode outside 0..1, more than 2^31 - 1 CTUs.  The encoder hook does not consume the mask yet
 * (INTEGRATION.md). */
int  fhevc_pu_shape_select_device(fhevc_ctx* ctx, const fhevc_motion_qpel_node* d_nodes, const fhevc_motion_qpel_node* d_pus,
                                  const fhevc_motion_qpel_node* d_pus_small, int num_pictures, int ctu_row_begin, int ctu_row_end,
                                  const fhevc_pu_shape_rule* rule, fhevc_pu_shape_node* d_shapes, uint32_t* d_costs, void* stream);
/* One picture pair, host buffers (both planes with the same stride), synchronous: uploads the pair and runs, on the context's stream,
 * fhevc_motion_search_pu_wide_device for all three families (search_range 1..64, SAD), fhevc_motion_refine_pu_wide_device with max_range = search_range and the
 * selection; downloads only the shapes (numCtus * 85 records): 1 360 bytes per CTU come back instead of the 9 488 bytes of refined entries. */
int  fhevc_p_shape_frame(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range,
                         const fhevc_pu_shape_rule* rule, fhevc_pu_shape_node* shapes /* numCtus * 85 */);

/* ---- config 4 (P slices): depth ranges from the refined inter costs, decided bottom-up over the quad-tree (k_p_tree.hip) -------------------------
 * HM decides the quad-tree bottom-up: the best cost of a CU over its partition sizes against the sum of the best trees of its four children
 * (TEncCu::xCompressCU, xCheckBestMode).  The records of fhevc_pu_shape_select[_device] hold "best cost over partition sizes" per node, on quarter-sample
 * Hadamard costs; this entry point makes the comparison and writes its outcome in the form the encoder hook already takes: a depth_min / depth_max map per
 * CTU, as fhevc_p_depth_range writes them.
 * Input per CTU: the 85 fhevc_pu_shape_node records; only cost_best is read.  Node order, levels l = 0, 1, 2, 3 for k = 0, 1..4, 5..20, 21..84 and raster
 * order inside a level as everywhere else.  MARK = 0xFFFFFFFF, SAT = 0xFFFFFFFE, s = 64 >> l, node (nx, ny) of level l, valid_w / valid_h the CTU's samples
 * inside the picture.
 * Geometry classes (the geometry alone decides them, no input byte does):
 *   INSIDE    iff nx * s + s <= valid_w && ny * s + s <= valid_h
 *   OUTSIDE   iff nx * s >= valid_w || ny * s >= valid_h
 *   CROSSING  otherwise
 *   ABSENT    iff OUTSIDE, or l == 3 and not INSIDE: no CU is coded there
 * Bottom-up costs:
 *   own[k]    cost_best of record k if INSIDE, else MARK
 *   kids[k]   level 3: MARK.  Other levels, not ABSENT: MARK if any non-ABSENT child has tree == MARK; otherwise the 64-bit sum of tree[child] over the
 *             non-ABSENT children, plus split_cost[l] only when k is INSIDE, saturated at SAT
 *   tree[k]   level 3: own[k].  CROSSING: kids[k].  INSIDE: own if kids == MARK; kids if own == MARK (both MARK gives MARK); otherwise
 *             kids < own ? kids : own -- strict "<": xCheckBestMode replaces only on a strictly smaller cost
 * Margins never enter tree.
 * Decisions exist for an INSIDE node of level 0..2 with own != MARK && kids != MARK, evaluated in 64 bits:
 *   split_sure = kids + split_abs[l] + ((kids * split_q8[l]) >> 8) < own
 *   stop_sure  = own + stop_abs[l] + ((own * stop_q8[l]) >> 8) <= kids
 * otherwise neither holds.  With all margins 0 exactly one of the two holds; with non-negative margins never both.
 * Maps: assembled exactly as fhevc_p_depth_range assembles its maps (the per-unit walk over levels 0..2) with
 *   sure  = CROSSING || split_sure          (depth_min follows the sure splits top-down)
 *   maybe = CROSSING || !stop_sure          (depth_max follows the maybe splits top-down)
 * There is no window and no prev_depth.  Units with 4 * ux >= valid_w or 4 * uy >= valid_h get 0.  depth_min <= depth_max per unit follows from the
 * definition. */
typedef struct {
  uint32_t cost_own;        /* own[k] */
  uint32_t cost_kids;       /* kids[k] */
  uint32_t cost_tree;       /* tree[k] */
  uint8_t  flags;           /* bit 0 split_sure, bit 1 stop_sure, bit 2 CROSSING, bit 3 ABSENT, bit 4 own available (!= MARK), bit 5 kids available;
                             * bit 6 (fhevc_p_tree_select_merge* and fhevc_p_tree_select_skip* only): own is the merge cost;
                             * bit 7 (fhevc_p_tree_select_skip* only): a skip, not descended */
  uint8_t  level;           /* l */
  uint8_t  pad[2];          /* written 0 */
} fhevc_p_tree_node;        /* 16 bytes; an ABSENT node gets three MARKs and bit 3 only */
typedef struct {
  int32_t split_q8[3];      /* per level 0..2, 0..65535: relative margin in 1/256 of kids */
  int32_t split_abs[3];     /* per level, cost units, >= 0 */
  int32_t stop_q8[3];       /* per level, 0..65535: relative margin in 1/256 of own */
  int32_t stop_abs[3];      /* per level, cost units, >= 0 */
  int32_t split_cost[3];    /* per level, cost units, >= 0: added to the children's sum of an INSIDE node (what signalling the split costs) */
} fhevc_p_tree_rule;        /* 60 bytes */
/* all zero: the UNFITTED hard decision (depth_min == depth_max wherever no MARK is involved) -- not a tuned default; margins have to be fitted on the
 * reference's own depths first */
void fhevc_p_tree_rule_default(fhevc_p_tree_rule* rule);
/* One CTU, host-side integer logic, no context, no device work (the twin of the kernel).  shapes: the CTU's 85 records; valid_w / valid_h: 8..64.
 * depth_min / depth_max: 256 bytes each, raster 16 x 16; tree: 85 records.  Each of the three outputs may be NULL, not all three.  FHEVC_E_INVALID (nothing
 * is written): a null shapes or rule, all three outputs null, valid_w / valid_h outside 8..64, a q8 outside 0..65535, a negative abs or split_cost. */
int  fhevc_p_tree_select(const fhevc_pu_shape_node* shapes /* 85 */, int valid_w, int valid_h, const fhevc_p_tree_rule* rule,
                         uint8_t* depth_min /* 256 or NULL */, uint8_t* depth_max /* 256 or NULL */, fhevc_p_tree_node* tree /* 85 or NULL */);
/* Device form (k_p_tree.hip): the same bits per CTU with the valid width / height the context's geometry gives it (any 1..64).  d_shapes: num_pictures *
 * band CTUs * 85 records, compact over the band: exactly what fhevc_pu_shape_select_device writes for the same arguments.  d_depth_min / d_depth_max:
 * compact over the band, entry ((p * band_rows + row - ctu_row_begin) * ctus_per_row + col) * 256; d_tree: num_pictures * band CTUs * 85 records.  Each of
 * the three outputs may be NULL, not all three; each is written over exactly its extent, an empty band writes nothing.  rule: HOST memory, read during the
 * call (it travels to the kernel by value); NULL = fhevc_p_tree_rule_default.  Asynchronous with respect to the host, allocates nothing, keeps no state:
 * calls with different rules may be in flight on two streams.  Stream semantics as fhevc_pu_shape_select_device (NULL = the context's blocking stream), so
 * the selection and the tree may follow each other on one stream without a host synchronisation.  d_shapes and d_tree may have any alignment their type
 * allows (4 bytes), the maps any byte alignment: where the maps are 4-byte aligned they leave as dwords, as bytes otherwise; where d_tree is 16-byte aligned
 * its records leave as 16-byte stores, as dwords otherwise; the bytes written are the same.  Timed under slot 17 of fhevc_kernel_timing.  FHEVC_E_INVALID
 * with a fhevc_last_error text (nothing is launched or written): a null context or d_shapes, all three outputs null, num_pictures < 1, a bad band, a rule
 * field outside its range, more than 2^31 - 1 CTUs.  The maps reach the encoder as fhevc_p_depth_range's do (TEncFastDepth::setExternalRange,
 * INTEGRATION.md); the margins are unfitted. */
int  fhevc_p_tree_select_device(fhevc_ctx* ctx, const fhevc_pu_shape_node* d_shapes, int num_pictures, int ctu_row_begin, int ctu_row_end,
                                const fhevc_p_tree_rule* rule, uint8_t* d_depth_min, uint8_t* d_depth_max, fhevc_p_tree_node* d_tree, void* stream);
/* One picture pair, host buffers (both planes with the same stride), synchronous, on the context's stream: uploads the pair and runs
 *   coarse_range == 0      the chain of fhevc_p_shape_frame (fhevc_motion_search_pu_wide_device for all three families, search_range 1..64;
 *                          fhevc_motion_refine_pu_wide_device with max_range = search_range; the selection), then the tree;
 *   coarse_range 1..14     fhevc_motion_centres_device, fhevc_motion_search_pu_centred_device (search_range 1..8, all three families),
 *                          fhevc_motion_refine_pu_centred_device (max_range = search_range), the selection, the tree: the centred chain end to end.
 * shape_rule / tree_rule: NULL = the defaults.  Downloads the two maps (numCtus * 256 bytes each, both required) and, where shapes is not NULL, the
 * selection's records.  FHEVC_E_INVALID (nothing is launched or written): a null context, plane or map, stride_samples < width, qp outside 0..51,
 * coarse_range outside 0..14, search_range outside 1..64 (coarse_range 0) or 1..8 (coarse_range > 0), a rule field outside its range. */
int  fhevc_p_tree_frame(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range, int coarse_range,
                        const fhevc_pu_shape_rule* shape_rule, const fhevc_p_tree_rule* tree_rule, uint8_t* depth_min /* numCtus * 256 */,
                        uint8_t* depth_max /* numCtus * 256 */, fhevc_pu_shape_node* shapes /* numCtus * 85 or NULL */);

/* ---- config 4 (P slices): merge-candidate costs per CU node (k_motion_merge.hip) -------------------------------------------------------------
 * Every inter cost above is the cost of an explicitly coded vector: a Hadamard distortion plus the exp-Golomb bits of the vector.  HM checks something else
 * first at every CU of a P picture (TEncCu::xCheckRDCostMerge2Nx2N, a full RD check of every merge candidate of the 2Nx2N CU), and for every PU of the OTHER
 * partition sizes predInterSearch runs TEncSearch::xMergeEstimation (TEncSearch.cpp:2831-2884, called at :3371 under `getPartitionSize != SIZE_2Nx2N`, :3336):
 * the same Hadamard distortion at a vector INHERITED from a spatial neighbour, priced at one to four bits of merge index and no vector bits at all.  HM does
 * not run xMergeEstimation for a 2Nx2N CU; this entry point APPLIES its pricing to the square CU node -- a source-only estimate of what the 2Nx2N merge check
 * finds -- on what a source-only pass has: the vectors the neighbouring nodes of the SAME level were refined to.
 * Input: the 85 refined square nodes per CTU, fhevc_motion_qpel_node records, (num_frames - 1) * band CTUs * 85, compact over the band -- what
 * fhevc_motion_refine_device, the d_out_nodes of fhevc_motion_refine_pu_wide_device or of fhevc_motion_refine_pu_centred_device wrote for the same pictures
 * and band.  Only cost_best (for the marker test), mvx and mvy (quarter samples) are read.  qp 0..51, max_range 1..64.
 * Geometry: node k of level l (s = 64 >> l, N = 1 << l) at (bx, by) in CTU (cx, cy) has the grid position (gx, gy) = (cx N + bx, cy N + by) in the picture; it
 * is valid iff it lies wholly inside the picture (INSIDE as for fhevc_p_tree_select); its coding-order key is (CTU raster index, z-index of (bx, by) at level
 * l), the z-index being the bit interleave with x in the even bits.
 * Candidate positions: HM's five spatial positions (TComDataCU::getInterMergeCandidates, TComDataCU.cpp:2142-2320) mapped to the same-level node that holds
 * HM's sample:
 *   j = 0  L   (A1)  node (gx - 1, gy)          j = 1  A   (B1)  node (gx, gy - 1)          j = 2  AR  (B0)  node (gx + 1, gy - 1)
 *   j = 3  BL  (A0)  node (gx - 1, gy + 1)      j = 4  AL  (B2)  node (gx - 1, gy - 1)
 * avail[j] iff ALL of: the neighbour lies on the level's grid and is INSIDE; its CTU row lies in [ctu_row_begin, ctu_row_end) -- a band behaves as a slice,
 * candidates never cross it, as in HM --; its key is smaller than the node's own (always so for L, A and AL; for AR and BL this decides exactly what
 * getPUAboveRight and getPUBelowLeft decide for CUs of equal size); its record's cost_best != 0xFFFFFFFF; |mvx| <= 4 max_range + 3 and |mvy| <= 4 max_range + 3,
 * the reach of a refined vector, so that no input byte can send a read outside the staged window.
 * List, in HM's order with HM's pruning pairs (vectors compared as (mvx, mvy)):
 *   1. L   if avail[L]                                              2. A   if avail[A] and not (avail[L] and v_A = v_L)
 *   3. AR  if avail[AR] and not (avail[A] and v_AR = v_A)           4. BL  if avail[BL] and not (avail[L] and v_BL = v_L)
 *   5. AL  only if the list holds fewer than 4 entries, avail[AL], and its vector equals neither an available L's nor an available A's
 *   6. the zero vector if the list holds fewer than 5 entries; it is not pruned
 * so the list is never empty.  Two parts of HM's list are left out: HM fills the rest of its list with zero candidates (of which only the first can win
 * under strict "<", so one is enough), and the temporal candidate needs a coded co-located picture.
 * Cost of list entry i with vector q: sd(q) + c[bits], bits = i + 1 except bits = 4 for i = 4 (MaxNumMergeCand 5, TEncSearch.cpp:2869-2874).  sd(q) is
 * TComRdCost::xGetHADs of the whole node -- the sum over its 8x8 tiles of (sum |H8 d H8| + 2) >> 2, the node's sum shifted ONCE by bit_depth - 8 -- on
 * fhevc_motion_refine's prediction: HEVC's 8-tap interpolation of the PREVIOUS ORIGINAL picture in that entry point's one arithmetic form, coordinates
 * clamped to the picture.  c[b] = getCost(b) at the lambda of slice QP qp, the table the refinements pass by value: predInterSearch calls
 * m_pcRdCost->selectMotionLambda(true, 0, ..) at TEncSearch.cpp:3345, before the xMergeEstimation of :3371, and xMotionEstimation selects the same lambda
 * again (:3717), so the getCost of :2874 runs under the motion estimation's lambda; getCost(bits) does not involve the cost scale.  The winner takes strict
 * "<": the first entry of equal cost wins. */
typedef struct {
  uint32_t satd_best;       /* sd at the winner */
  uint32_t cost_best;       /* its cost */
  int16_t  mvx, mvy;        /* the winner's vector, quarter samples */
  uint8_t  idx;             /* the winner's position in the list */
  uint8_t  num;             /* the list's length, 1..5 */
  uint8_t  src;             /* where the winner came from: 0..4 = L, A, AR, BL, AL; 5 = the zero vector */
  uint8_t  pad;             /* written 0 */
} fhevc_motion_merge_node;  /* 16 bytes; a node that is not INSIDE gets 0xFFFFFFFF twice, a zero vector, idx = src = 255, num = 0, pad = 0 */
/* Device form: planes, band and stream arguments as fhevc_motion_refine_device; frame f = 1 .. num_frames-1 is predicted from frame f-1.  d_refined, d_out:
 * (num_frames - 1) * band CTUs * 85 records, compact over the band; the output is written over exactly that extent, an empty band writes nothing.  The
 * kernel has the square refinement's mapping (a workgroup of four waves per CTU over a persistent grid, wave = level, lane = 8x8 tile, the window of that
 * kernel in LDS: the MR = 8 layout up to max_range 8, the MR = 64 layout above, of which the part max_range reaches is staged) and walks the node's list of
 * at most five entries where that kernel walks 18 candidates.  Asynchronous with respect to the host, allocates nothing, keeps NO state in HBM between calls
 * (the bit costs travel by value): calls with different QPs and ranges may be in flight on two streams, and a refinement and the merge stage may follow each
 * other on one stream without a host synchronisation.  FHEVC_E_INVALID with a fhevc_last_error text (nothing is launched or written): a null context, d_luma,
 * d_refined or d_out, num_frames < 2, qp outside 0..51, max_range outside 1..64, stride_samples < width, a bad band, overlapping frames, uint8 planes on a
 * context above 8 bit -- whatever fhevc_motion_refine_device rejects.  Timed under slot 19 of fhevc_kernel_timing.
 * NOT covered: the temporal candidate, candidates from neighbours of a finer level than the node's own, a window staged around per-CTU centres.  (Skip
 * detection: fhevc_motion_skip*, further below.)  (The rectangular PUs, with HM's second-PU rules: fhevc_motion_merge_pu*, further below.)  The encoder hook does not consume this output. */
int  fhevc_motion_merge_device(fhevc_ctx* ctx, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                               int num_frames, int ctu_row_begin, int ctu_row_end, int qp, int max_range, const fhevc_motion_qpel_node* d_refined,
                               fhevc_motion_merge_node* d_out, void* stream);
/* one picture pair, host buffers (both planes with the same stride), synchronous, as fhevc_motion_refine; refined, out: numCtus * 85 */
int  fhevc_motion_merge(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int max_range,
                        const fhevc_motion_qpel_node* refined, fhevc_motion_merge_node* out);

/* The tree decision WITH the merge costs: fhevc_p_tree_select[_device] with one more input, the CTU's 85 fhevc_motion_merge_node records (never NULL; on the
 * device compact over the band like d_shapes; only cost_best is read).  The one change to the definition above is the own cost: for an INSIDE node
 *   own[k] = the smaller of shapes[k].cost_best and merge[k].cost_best, MARK counting as unavailable (both MARK: own[k] = MARK)
 * and bit 6 of the record's flags is set iff the node is INSIDE and the merge cost is available and strictly smaller than shapes[k].cost_best, or that is
 * MARK -- which, MARK being the largest value, is merge[k].cost_best < shapes[k].cost_best.  Everything else -- kids, tree, margins, maps, CROSSING / ABSENT,
 * NULL outputs, alignments, the rule by value, the rejected calls -- is the existing definition; with all merge costs MARK the output is byte for byte
 * fhevc_p_tree_select[_device]'s.  The device form is a further instantiation of k_p_tree.hip (one more dword load per lane and round), timed under slot 17;
 * d_merge may have any alignment its type allows (4 bytes).  The host form needs no context. */
int  fhevc_p_tree_select_merge(const fhevc_pu_shape_node* shapes /* 85 */, const fhevc_motion_merge_node* merge /* 85 */, int valid_w, int valid_h,
                               const fhevc_p_tree_rule* rule, uint8_t* depth_min /* 256 or NULL */, uint8_t* depth_max /* 256 or NULL */,
                               fhevc_p_tree_node* tree /* 85 or NULL */);
int  fhevc_p_tree_select_merge_device(fhevc_ctx* ctx, const fhevc_pu_shape_node* d_shapes, const fhevc_motion_merge_node* d_merge, int num_pictures,
                                      int ctu_row_begin, int ctu_row_end, const fhevc_p_tree_rule* rule, uint8_t* d_depth_min, uint8_t* d_depth_max,
                                      fhevc_p_tree_node* d_tree, void* stream);
/* fhevc_p_tree_frame with the merge stage between refinement and tree: the same arguments, checks and chains, then fhevc_motion_merge_device on the refined
 * nodes -- with max_range = search_range on the zero-centred chain (coarse_range 0), with max_range 64 on the centred chain, where absolute vectors reach
 * +-64 and neighbouring CTUs have different centres --, the selection, and fhevc_p_tree_select_merge_device.  merge: numCtus * 85 records, or NULL. */
int  fhevc_p_tree_merge_frame(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range, int coarse_range,
                              const fhevc_pu_shape_rule* shape_rule, const fhevc_p_tree_rule* tree_rule, uint8_t* depth_min /* numCtus * 256 */,
                              uint8_t* depth_max /* numCtus * 256 */, fhevc_pu_shape_node* shapes /* numCtus * 85 or NULL */,
                              fhevc_motion_merge_node* merge /* numCtus * 85 or NULL */);

/* ---- config 4 (P slices): merge-candidate costs per PU (k_motion_merge_pu.hip) -----------------------------------------------------------------
 * TEncSearch::xMergeEstimation (TEncSearch.cpp:2831-2884) where HM itself runs it: for every PU of a CU whose partition size is not 2Nx2N (:3336, :3371);
 * predInterSearch then keeps the merge cost instead of the motion-estimation cost when uiMRGCost < uiMECost (:3373).  The 124 + 384 PUs are those of
 * fhevc_motion_refine_pu*.
 *   Input: the refined square nodes (85 per CTU; cost_best, mvx, mvy are read) -- exactly what fhevc_motion_merge_device takes.  No PU entry is read.
 *   Output: one fhevc_motion_merge_node per PU: d_out_pus 124 per CTU in fhevc_motion_pu_index order, d_out_pus_small 384 per CTU in
 * fhevc_motion_pu_small_index order; either may be NULL, not both.
 *   Geometry: a PU belongs to CU node k of level l (s = 64 >> l); its rectangle (xP, yP, w, h) in picture samples is getPartIndexAndSize's, the one the PU
 * searches use.  It is valid iff its CU node is INSIDE; an invalid PU gets the record of an invalid node (0xFFFFFFFF twice, a zero vector, idx = src = 255,
 * num = 0, pad = 0).
 *   Candidate positions (TComDataCU.cpp:2142-2320): L (xP - 1, yP + h - 1), A (xP + w - 1, yP - 1), AR (xP + w, yP - 1), BL (xP - 1, yP + h),
 * AL (xP - 1, yP - 1).  Each maps to the node of the CU's OWN level l that holds the sample: grid position (sx >> log2 s, sy >> log2 s), a negative
 * coordinate is off the grid; its vector is that node's refined square vector.
 *   A candidate is available iff it is on the grid and INSIDE, its CTU row lies in the band, its coding-order key (CTU raster index, z-index of the node
 * in its CTU) is strictly smaller than the key of the PU's own CU, its record is no marker, and |mvx| and |mvy| are both <= 4 max_range + 3.  The key
 * rule reproduces HM's two second-PU exclusions (:2170, :2202): part 1 of Nx2N / nLx2N / nRx2N has its L sample, part 1 of 2NxN / 2NxnU / 2NxnD its A sample
 * inside part 0 of its own CU, whose key is equal, not smaller; no other candidate of any of the 508 PUs falls inside its own CU.
 *   Parallel merge level: modelled at HM's default Log2ParMrgLevel 2, where isDiffMER is true for every position outside the PU and the shared list of
 * 8x8 CUs (TEncSearch.cpp:2841) does not apply.
 *   List, cost and choice as fhevc_motion_merge*: HM's order and pruning pairs on vectors (two positions in one node prune each other), AL only below four
 * entries, one zero vector below five; entry i costs sd(q) + c[bits], bits = i + 1, 4 for i = 4, c at the slice QP's motion lambda; sd(q) = xGetHADs of the
 * whole w x h PU through the branch xGetHADs takes -- 8x8 Hadamards (sum + 2) >> 2 for the 124, 4x4 Hadamards (sum + 1) >> 1 over all (w/4)(h/4) tiles for the
 * 384 --, the PU's sum shifted once by bit_depth - 8, on fhevc_motion_refine's prediction; strict "<", the first entry of equal cost wins.
 *   Device form: planes, band, qp 0..51, max_range 1..64 and stream as fhevc_motion_merge_device, and whatever that rejects is rejected here with
 * FHEVC_E_INVALID and a fhevc_last_error text, nothing launched, nothing written.  Outputs compact over the band, written over exactly their extent; an
 * empty band writes nothing.  Asynchronous, allocates nothing, keeps no state in HBM (the bit costs travel by value).  The kernel has
 * fhevc_motion_refine_pu's mapping (workgroup = CTU over a persistent grid, 26 passes dealt to four waves, lane = 8x8 tile) and the merge stage's list in
 * registers; the 123 nodes that can be a neighbour are parked in LDS once per CTU.  Timed under slot 21 of fhevc_kernel_timing.
 * NOT covered: the temporal candidate, candidates from finer-level neighbours, Log2ParMrgLevel above 2, per-PU skip tests (the CU nodes' own:
 * fhevc_motion_skip*, further below), a window around per-CTU centres.
 * The encoder hook does not consume this output. */
int  fhevc_motion_merge_pu_device(fhevc_ctx* ctx, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                                  int num_frames, int ctu_row_begin, int ctu_row_end, int qp, int max_range, const fhevc_motion_qpel_node* d_refined,
                                  fhevc_motion_merge_node* d_out_pus, fhevc_motion_merge_node* d_out_pus_small, void* stream);
/* one picture pair, host buffers (both planes with the same stride), synchronous, as fhevc_motion_merge; refined: numCtus * 85; out_pus: numCtus * 124 or
 * NULL; out_pus_small: numCtus * 384 or NULL (not both NULL) */
int  fhevc_motion_merge_pu(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int max_range,
                           const fhevc_motion_qpel_node* refined, fhevc_motion_merge_node* out_pus, fhevc_motion_merge_node* out_pus_small);

/* The partition-size selection WITH the PUs' merge costs: fhevc_pu_shape_select[_device] with two more inputs, the merge records of the 124 and of the 384
 * PUs (merge_pus never NULL; merge_pus_small may be NULL, which means all markers -- as a NULL pus_small means for the refined small PUs), and ONE changed
 * rule, HM's :3373: the cost of a part is min(refined cost_best, merge cost_best).  The marker is the largest value, so it loses to any cost and two markers
 * stay one; a pair's sum, saturation and unavailability are as before.  p = 0 stays the explicit 2Nx2N cost: the node's own merge cost enters at the tree
 * (fhevc_p_tree_select_merge*).  One more optional output, merged: a uint16_t per node, bit 2 p + part set iff that part's merge cost is strictly smaller
 * than its refined cost; 0 for an invalid node, and never set for a part whose two costs are both markers or for a size the node does not have.  With every
 * merge cost MARK, records and cost table are byte for byte fhevc_pu_shape_select[_device]'s.  The host form needs no context; the device form is a
 * further instantiation of k_pu_shape.hip (of a merge record cost_best is dword 1), timed under slot 13; d_merged is written as 2-byte stores over
 * num_pictures * band CTUs * 85 values.  Everything else -- rule, bands, alignments, rejected calls -- is the existing definition. */
int  fhevc_pu_shape_select_merge(const fhevc_motion_qpel_node* nodes /* 85 */, const fhevc_motion_qpel_node* pus /* 124 */,
                                 const fhevc_motion_qpel_node* pus_small /* 384 or NULL */, const fhevc_motion_merge_node* merge_pus /* 124 */,
                                 const fhevc_motion_merge_node* merge_pus_small /* 384 or NULL */, int valid_w, int valid_h, const fhevc_pu_shape_rule* rule,
                                 fhevc_pu_shape_node* out /* 85 */, uint32_t* costs /* 85 * 8 or NULL */, uint16_t* merged /* 85 or NULL */);
int  fhevc_pu_shape_select_merge_device(fhevc_ctx* ctx, const fhevc_motion_qpel_node* d_nodes, const fhevc_motion_qpel_node* d_pus,
                                        const fhevc_motion_qpel_node* d_pus_small, const fhevc_motion_merge_node* d_merge_pus,
                                        const fhevc_motion_merge_node* d_merge_pus_small, int num_pictures, int ctu_row_begin, int ctu_row_end,
                                        const fhevc_pu_shape_rule* rule, fhevc_pu_shape_node* d_shapes, uint32_t* d_costs, uint16_t* d_merged, void* stream);
/* fhevc_p_tree_merge_frame on merge-aware selection costs: the same arguments, checks and chains; behind fhevc_motion_merge_device comes
 * fhevc_motion_merge_pu_device for all 508 PUs with the same max_range (search_range, or 64 on the centred chain), and the selection is
 * fhevc_pu_shape_select_merge_device.  Downloads what fhevc_p_tree_merge_frame downloads. */
int  fhevc_p_tree_merge_pu_frame(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range, int coarse_range,
                                 const fhevc_pu_shape_rule* shape_rule, const fhevc_p_tree_rule* tree_rule, uint8_t* depth_min /* numCtus * 256 */,
                                 uint8_t* depth_max /* numCtus * 256 */, fhevc_pu_shape_node* shapes /* numCtus * 85 or NULL */,
                                 fhevc_motion_merge_node* merge /* numCtus * 85 or NULL */);

/* ---- config 4 (P slices): refined costs re-priced against neighbour predictors (k_motion_amvp.hip) ---------------------------------------------
 * Every explicit cost above is satd + getCost(bits(q - p)) with p the zero vector (the centred chain: one coarse centre per CTU).  HM does not price an
 * explicit vector against zero: predInterSearch calls xEstimateMvPredAMVP (TEncSearch.cpp:3028), xMotionEstimation and xPatternSearchFracDIF run under
 * setPredictor(mvp) (:3065), and xCheckBestMVP then keeps the predictor of fewest bits (:3566-3615).  The list is TComDataCU::fillMvpCand
 * (TComDataCU.cpp:2578-2716).  This stage re-prices the refined records on what a source-only pass has -- the refined vectors of the same-level neighbours
 * -- and reads NO samples: the vector stays the one the chain found, only its price changes.  It writes the record type it reads, so the selection, the
 * merge stages, the skip stage and the tree consume its output unchanged.
 *   Inputs per CTU: the 85 refined nodes (always: neighbour vectors come from them), optionally the 124 refined PUs and the 384 refined small PUs; all
 * fhevc_motion_qpel_node, compact over the band, as fhevc_motion_refine_pu_wide_device (or _centred_device) writes them.  Of a record satd_int, satd_best,
 * cost_best (for the marker test only: 0xFFFFFFFF), mvx and mvy are read.  Any int16 vector is legal: there is no reach condition, nothing is read from a plane.
 *   Entry E: a node, or a PU with getPartIndexAndSize's rectangle: (xP, yP, w, h) in picture samples, in CU node k of level l (s = 64 >> l).
 *   Positions, the five of fillMvpCand, which are the merge stage's: L (xP - 1, yP + h - 1), A (xP + w - 1, yP - 1), AR (xP + w, yP - 1), BL (xP - 1, yP + h),
 * AL (xP - 1, yP - 1).
 *   Candidate at a position.  (1) The sample lies inside E's own CU -- only for part 1: L of Nx2N / nLx2N / nRx2N, A of 2NxN / 2NxnU / 2NxnD --: the
 * candidate is part 0 of the same partition size in the same input family, its vector that PU's refined vector, available iff that record is no marker.
 * This is where AMVP departs from merge: fillMvpCand has no second-PU exclusion, and HM has set PU 0's motion by the time it searches PU 1.  (2) Any other
 * sample maps to the same-level node that holds it, exactly as for fhevc_motion_merge_pu*: available iff the node is on the grid and INSIDE, its CTU row lies
 * in the band, its coding-order key is strictly smaller than that of E's own CU, and its record is no marker; its vector is that node's refined square vector.
 *   List (single reference picture, TMVP off, as oracle/ref_rdo_harness.cpp runs the reference): a = the first available of (BL, L) (:2603-2619),
 * b = the first available of (AR, A, AL) (:2621-2632); the list is [a] then [b]; if both exist and are equal the second is dropped (the iN == 2 pruning,
 * :2647-2653); (0, 0) is appended until the list holds two entries (:2710-2714).  With one reference picture every inter neighbour refers to the target picture,
 * so xAddMVPCandUnscaled finds whatever xAddMVPCandWithScaling would: the scaled left passes (:2612-2615) never run, and the scaled above passes (:2634-2645),
 * which run only when neither BL nor L is inter, can only add the vector the unscaled above pass has added already -- which the iN == 2 pruning removes.
 *   Choice: bits_i = eg(mvx - p_i.x) + eg(mvy - p_i.y), eg = xGetExpGolombNumberOfBits at cost scale 0 (TComRdCost.h:166-174): 2 floor(log2 t) + 1 with
 * t = v <= 0 ? (-v << 1) + 1 : v << 1.  The index costs one bit for either index (xGetMvpIdxBits(., 2)), so it cancels and is left out, like the reference-index
 * and mode bits of every other stage.  idx = the first i of least bits.  DEPARTURE: where the bits tie, HM keeps the index its template match
 * (xEstimateMvPredAMVP) chose; this library takes the lower index.
 *   Output: per entry one fhevc_motion_qpel_node: satd_int, satd_best, mvx, mvy copied; cost_best = min(satd_best + c[bits_idx], 0xFFFFFFFE), the sum in 64
 * bits; c[b] = getCost(b) at the slice QP's motion lambda, the arithmetic of every other stage's table, in a table of its own with 67 entries (two int16
 * differences take at most 2 * 33 bits) that travels by value.  An input marker record is copied as it is.  An entry whose CU node is not INSIDE gets the
 * refinement's marker record (0xFFFFFFFF three times, a zero vector), whatever the input holds.
 *   Optional second output per family, one 8-byte record per entry: */
typedef struct {
  int16_t  px, py;          /* the chosen predictor, quarter samples */
  uint8_t  idx;             /* its index in the list, 0 or 1 */
  uint8_t  num_spatial;     /* entries of the list before the zero fill (after the pruning), 0..2 */
  uint8_t  src;             /* where it came from: 0..4 = L, A, AR, BL, AL; 5 = a filled zero */
  uint8_t  bits;            /* bits_idx, 2..66 */
} fhevc_motion_mvp;         /* 8 bytes; a marker entry and an entry that is not INSIDE get zeros with idx = src = 255 */
/* Device form: num_frames - 1 picture pairs (as the motion entry points count them: num_frames >= 2), the band, qp 0..51; d_nodes never NULL; d_pus /
 * d_pus_small may be NULL; a family's outputs (d_out_*, d_mvp_*) need that family's input; at least one of the six outputs must be non-NULL.  All arrays
 * compact over the band: (num_frames - 1) * band CTUs * 85 / 124 / 384 entries, outputs written over exactly that extent; an empty band writes nothing.
 * Every array may sit on any 4-byte alignment (16-byte accesses where all are 16-byte -- the predictor records 8-byte -- aligned, dwords otherwise); input
 * and output arrays must not overlap.  One launch for all 593 entries of every CTU: a workgroup per CTU, the 123 nodes that can be a neighbour parked in LDS
 * once per CTU, part 0 of a PU read from the lane before.  Asynchronous, allocates nothing, keeps NO state in HBM (the bit costs travel by value): calls with
 * different QPs may be in flight on two streams, and refinement, this stage and the merge stages may follow each other on one stream without a host
 * synchronisation.  FHEVC_E_INVALID with a fhevc_last_error text (nothing launched, nothing written): a null context (no text), a null d_nodes, no output, an
 * output without its input, a pointer that is not 4-byte aligned, num_frames < 2, a bad band, qp outside 0..51.  Timed under slot 25 of fhevc_kernel_timing.
 * NOT covered: a search or refinement that moves its window to the predictor or picks its winner under it, the temporal candidate, predictors from
 * finer-level neighbours.  Table entries 39..66 rest on the formula, and the formula on the reference's own getCost(0..66) at every QP: recorded, with
 * fillMvpCand's lists on hand-set motion fields, in tests/golden/ref_motion_candidates.npz.  Not held to the reference: the band rule, INSIDE, the tie
 * departure above.  The encoder hook does not consume this output. */
int  fhevc_motion_amvp_device(fhevc_ctx* ctx, int num_frames, int ctu_row_begin, int ctu_row_end, int qp, const fhevc_motion_qpel_node* d_nodes,
                              const fhevc_motion_qpel_node* d_pus, const fhevc_motion_qpel_node* d_pus_small, fhevc_motion_qpel_node* d_out_nodes,
                              fhevc_motion_qpel_node* d_out_pus, fhevc_motion_qpel_node* d_out_pus_small, fhevc_motion_mvp* d_mvp_nodes,
                              fhevc_motion_mvp* d_mvp_pus, fhevc_motion_mvp* d_mvp_pus_small, void* stream);
/* one picture, host arrays over the whole picture (numCtus * 85 / 124 / 384), synchronous; NULL rules as the device form */
int  fhevc_motion_amvp(fhevc_ctx* ctx, int qp, const fhevc_motion_qpel_node* nodes, const fhevc_motion_qpel_node* pus, const fhevc_motion_qpel_node* pus_small,
                       fhevc_motion_qpel_node* out_nodes, fhevc_motion_qpel_node* out_pus, fhevc_motion_qpel_node* out_pus_small, fhevc_motion_mvp* mvp_nodes,
                       fhevc_motion_mvp* mvp_pus, fhevc_motion_mvp* mvp_pus_small);
/* The host twin: the same definition in plain C++ for one picture of width x height and the band [ctu_row_begin, ctu_row_end); arrays compact over the
 * band.  Needs no context and no device.  bit_depth 8..12 (the motion lambda does not depend on it).  FHEVC_E_INVALID (nothing written): what the device
 * form rejects, width or height below 8. */
int  fhevc_motion_amvp_picture(int width, int height, int bit_depth, int ctu_row_begin, int ctu_row_end, int qp, const fhevc_motion_qpel_node* nodes,
                               const fhevc_motion_qpel_node* pus, const fhevc_motion_qpel_node* pus_small, fhevc_motion_qpel_node* out_nodes,
                               fhevc_motion_qpel_node* out_pus, fhevc_motion_qpel_node* out_pus_small, fhevc_motion_mvp* mvp_nodes, fhevc_motion_mvp* mvp_pus,
                               fhevc_motion_mvp* mvp_pus_small);
/* fhevc_p_tree_merge_pu_frame with this stage between the refinements and the merge stages: the same arguments, checks and both chains; the merge stages,
 * the selection and the tree then read the re-priced records.  On the centred chain the stage replaces the per-CTU-centre pricing. */
int  fhevc_p_tree_amvp_frame(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range, int coarse_range,
                             const fhevc_pu_shape_rule* shape_rule, const fhevc_p_tree_rule* tree_rule, uint8_t* depth_min /* numCtus * 256 */,
                             uint8_t* depth_max /* numCtus * 256 */, fhevc_pu_shape_node* shapes /* numCtus * 85 or NULL */,
                             fhevc_motion_merge_node* merge /* numCtus * 85 or NULL */);

/* ---- config 4 (P slices): the zero-residual (skip) test per CU node (k_motion_skip.hip) -----------------------------------------------------------
 * In HM a CU whose best mode is merge with an all-zero residual is a skip: TEncCu.cpp:892 (EarlyCU) does not descend below it, and :610-637 with
 * :1444-1468 (EarlySkipDetection) do not try its other partition sizes.  Whether a residual quantises to zero is an exact integer question: HM's forward
 * transform and its dead-zone quantiser are closed-form integer arithmetic.  This entry point answers it for the vector a node's merge record holds.
 *   Input per CTU: the 85 fhevc_motion_merge_node records that fhevc_motion_merge_device wrote for the same pictures and band; only cost_best (the marker
 * test), mvx and mvy are read.  qp 0..51, max_range 1..64.  Planes, band, stream, frame pairing (frame f is predicted from frame f - 1), the
 * compact-over-the-band record layout and the rejected calls are exactly fhevc_motion_merge_device's.
 *   A node k of level l (s = 64 >> l) is valid iff it is INSIDE, its merge record is no marker (cost_best != 0xFFFFFFFF), and |mvx| and |mvy| are both
 * <= 4 max_range + 3, so that no input byte can send a read outside the staged window.
 *   Step 1, the residual: r = original - fhevc_motion_refine's prediction at (mvx, mvy): the previous ORIGINAL picture through HEVC's 8-tap interpolation
 * in the one arithmetic form, coordinates clamped to the picture.
 *   Step 2, the transform: HM's forward transform xTrMxN (TComTrQuant.cpp:860-915).  TU size N = min(s, 32): a 64x64 node is four 32x32 TUs
 * (QuadtreeTULog2MaxSize 5, cfg/encoder_lowdelay_P_main.cfg:12), every other node is one TU; the TU tree is not searched.  The DCT, never the DST;
 * maxLog2TrDynamicRange 15, so shift_1st = log2 N + bit_depth - 9 over the rows and shift_2nd = log2 N + 6 over the columns; the matrices are the
 * reference's g_aiT8 / g_aiT16 / g_aiT32; rounding as partialButterfly8 / 16 / 32: add 1 << (shift - 1), then an arithmetic shift right.
 *   Step 3, the quantiser: HM's scalar quantiser without scaling lists (TComTrQuant.cpp:1186-1232).  QP' = qp + 6 (bit_depth - 8), per = QP' / 6,
 * rem = QP' % 6, scale = g_quantScales[rem] = {26214, 23302, 20560, 18396, 16384, 14564}, qbits = 14 + per + (15 - bit_depth - log2 N),
 * level(c) = (|c| * scale + add) >> qbits evaluated in 64 bits, under two offsets: add_plain = 85 << (qbits - 9), the P-slice dead zone (:1215), and
 * add_half = 1 << (qbits - 1), the rounding from which RDOQ takes its starting levels (uiMaxAbsLevel, :2257).  If every starting level is 0, RDOQ never
 * finds a last position (:2264) and the block is zero: the second test is a SUFFICIENT condition for cbf = 0 under the reference's RDOQ : 1.
 *   Field order (pinned: 16 bytes without padding): */
typedef struct {
  uint32_t coef_max;        /* max |c| over the node's TU or TUs; depends on no QP */
  uint32_t level_sum;       /* sum of level(c) under add_plain: uiAbsSum of xQuant */
  uint16_t nonzero;         /* number of coefficients with level != 0 under add_plain, 0..4096 */
  uint8_t  flags;           /* bit 0: zero under add_plain (nonzero == 0); bit 1: zero under add_half.  Bit 1 implies bit 0 */
  uint8_t  pad;             /* written 0 */
  int16_t  mvx, mvy;        /* the vector tested, copied from the merge record */
} fhevc_motion_skip_node;   /* 16 bytes; an invalid node gets coef_max = level_sum = 0xFFFFFFFF, nonzero = 0xFFFF, flags = 0, pad = 0 and a zero vector */
/* Device form: d_merge, d_out: (num_frames - 1) * band CTUs * 85 records, compact over the band; the output is written over exactly that extent, an empty
 * band writes nothing.  The kernel keeps the merge kernel's outer mapping (a workgroup of four waves per CTU over a persistent grid sized by the
 * device's own occupancy answer, the window of the refinement in LDS in both layouts, lane = one 8x8 tile, one prediction per node) and runs both passes of
 * the transform through LDS buffers laid over the dead window, as 16-bit dot products -- exact: no intermediate exceeds 32 760.  The quantiser's numbers
 * are computed on the host and travel by value.  Asynchronous with respect to the host, allocates nothing, keeps NO state in HBM between calls: calls with
 * different QPs and ranges may be in flight on two streams, and the merge stage and this one may follow each other on one stream without a host
 * synchronisation.  FHEVC_E_INVALID with a fhevc_last_error text (nothing is launched or written): a null context, d_luma, d_merge or d_out, and whatever
 * fhevc_motion_merge_device rejects.  Timed under slot 23 of fhevc_kernel_timing.
 * NOT covered: per-PU skip tests, the TU quad-tree, transform skip, sign hiding, chroma.  The encoder hook does not consume this output. */
int  fhevc_motion_skip_device(fhevc_ctx* ctx, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples,
                              int num_frames, int ctu_row_begin, int ctu_row_end, int qp, int max_range, const fhevc_motion_merge_node* d_merge,
                              fhevc_motion_skip_node* d_out, void* stream);
/* one picture pair, host buffers (both planes with the same stride), synchronous, as fhevc_motion_merge; merge, out: numCtus * 85 */
int  fhevc_motion_skip(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int max_range,
                       const fhevc_motion_merge_node* merge, fhevc_motion_skip_node* out);

/* The tree decision that STOPS at a skip: fhevc_p_tree_select_merge[_device] with two more arguments, the CTU's 85 fhevc_motion_skip_node records (never
 * NULL; on the device compact over the band like d_shapes; any 4-byte alignment; only flags is read) and skip_mask (0..3: which of the two zero tests
 * count).  ONE changed rule, HM's EarlyCU (TEncCu.cpp:892): for an INSIDE node of level 0..2 whose own cost is the merge cost (bit 6 of the tree flags as
 * defined above) and whose skip.flags & skip_mask != 0
 *   tree[k] = own[k] whatever kids is -- HM never visits the children --, stop_sure = 1, split_sure = 0, and bit 7 of the record's flags is set;
 * kids[k] is still recorded.  Everything else is the existing definition; with skip_mask 0, or with no record carrying a masked bit, the output is byte for
 * byte fhevc_p_tree_select_merge[_device]'s.  The device form is a further instantiation of k_p_tree.hip (one more byte load per lane and round), timed
 * under slot 17.  The host form needs no context.  FHEVC_E_INVALID: what fhevc_p_tree_select_merge[_device] rejects, a null skip pointer, skip_mask
 * outside 0..3. */
int  fhevc_p_tree_select_skip(const fhevc_pu_shape_node* shapes /* 85 */, const fhevc_motion_merge_node* merge /* 85 */,
                              const fhevc_motion_skip_node* skip /* 85 */, int skip_mask, int valid_w, int valid_h, const fhevc_p_tree_rule* rule,
                              uint8_t* depth_min /* 256 or NULL */, uint8_t* depth_max /* 256 or NULL */, fhevc_p_tree_node* tree /* 85 or NULL */);
int  fhevc_p_tree_select_skip_device(fhevc_ctx* ctx, const fhevc_pu_shape_node* d_shapes, const fhevc_motion_merge_node* d_merge,
                                     const fhevc_motion_skip_node* d_skip, int skip_mask, int num_pictures, int ctu_row_begin, int ctu_row_end,
                                     const fhevc_p_tree_rule* rule, uint8_t* d_depth_min, uint8_t* d_depth_max, fhevc_p_tree_node* d_tree, void* stream);

/* ---- config 4 (P slices): the RD estimate per CU node: transform, quantise, rebuild, one TU split (k_motion_rd.hip) -----------------------------------
 * Every decision above compares Hadamard distortion + sqrt(lambda) * bits.  HM compares something else at every CU: xCheckRDCostMerge2Nx2N and
 * xCheckRDCostInter end in encodeResAndCalcRdInterCU (TEncSearch.cpp), where the residual goes through the forward transform, the quantiser, the
 * dequantiser and the inverse transform, and what xCheckBestMode compares is the SSE of the rebuilt block + lambda * bits over a residual quad-tree
 * (xEstimateInterResidualQT).  This entry point carries the skip stage's pass through to that quantity, for the vector a record holds.
 *   Input per CTU: 85 records that carry a vector, of the kind `source` names.
 *   FHEVC_RD_SOURCE_MERGE (0): fhevc_motion_merge_node records; the marker test is cost_best (dword 1), the vector dword 2, and
 * side_bits = idx + 1, but 4 for idx == 4: the merge stage's own pricing of the index.  d_mvp must be NULL.
 *   FHEVC_RD_SOURCE_EXPLICIT (1): fhevc_motion_qpel_node records (refined or re-priced); the marker test is cost_best (dword 2), the vector dword 3.  With
 * the re-pricing's fhevc_motion_mvp records in d_mvp, side_bits = bits of that record, and a marker predictor record (idx == 255) makes the node invalid;
 * with d_mvp NULL, side_bits = eg(mvx) + eg(mvy) against the zero predictor at cost scale 0, eg exactly as fhevc_motion_amvp* defines it.
 *   Planes (int16 or uint8), band, stream, frame pairing (frame f is predicted from frame f - 1), the compact-over-the-band record layout, qp 0..51,
 * max_range 1..64 and the rejected calls are exactly fhevc_motion_skip_device's.  A node is valid iff it is INSIDE, its record is no marker, and |mvx| and
 * |mvy| are both <= 4 max_range + 3.
 *   Step 1, the residual: r = original - fhevc_motion_refine's prediction at the vector, as in the skip stage.
 *   Step 2, the TUs: the depth-0 TU size is N0 = min(s, 32) (a 64x64 node is four 32x32 TUs), the depth-1 size N1 = N0 / 2: 64 -> 32 and 16, 32 -> 32 and
 * 16, 16 -> 16 and 8, 8 -> 8 and 4.  Under HM's limits (QuadtreeTUMaxDepthInter 3, getQuadtreeTULog2MinSizeInCU = log2 CU - 2 clipped to 2..5 for 2Nx2N)
 * these two sizes are HM's COMPLETE TU tree for 64x64 and 8x8 CUs; for 32x32 and 16x16 CUs HM has a third depth, which is left out.
 *   Step 3, per TU of either size, all in integers:
 *   forward transform: xTrMxN (TComTrQuant.cpp:860-915) as in the skip stage, now also at N = 4 -- the DCT: inter 4x4 never takes the DST --,
 * shift_1st = log2 N + bit_depth - 9, shift_2nd = log2 N + 6;
 *   quantiser: level = sign(c) * ((|c| * scale + add_plain) >> qbits), qbits = 21 + QP' / 6 - (bit_depth - 8) - log2 N: the skip stage's formula, with
 * log2 N = 2 added (TComTrQuant.cpp:1186-1232).  add_half serves flag bit 1 only.  RDOQ is NOT modelled;
 *   dequantiser: xDeQuant without scaling lists (TComTrQuant.cpp:1387-1422): rightShift = 6 - (15 - bit_depth - log2 N + per) = log2 N - 1 - qp / 6, which
 * does not depend on the bit depth; the level clipped to int16 (targetInputBitDepth is 16 for every legal argument; no level exceeds 13 108);
 * rightShift > 0: c^ = (level * g_invQuantScales[rem] + (1 << (rightShift - 1))) >> rightShift, otherwise c^ = (level * scale) << -rightShift; c^ clipped
 * to [-32768, 32767]; g_invQuantScales = {40, 45, 51, 57, 64, 72};
 *   inverse transform: xITrMxN (TComTrQuant.cpp:927-990): the first stage over the vertical frequencies, shift 7, clipped to [-32768, 32767]; the second
 * stage, shift 20 - bit_depth, clipped to the Pel range (the same interval): r^.  Every accumulation stays below 32 * 32768 * 90 < 2^31;
 *   distortion: xGetSSE with its PER-SAMPLE shift (TComRdCost.cpp:1190-1199): D = sum ((org - Clip(pred + r^, 0, 2^bit_depth - 1))^2 >> 2 (bit_depth - 8));
 * D < 2^32 at every bit depth;
 *   bits: the library's OWN estimate, unfitted: r(TU) = 1 + sum over the non-zero levels of (3 + 2 floor(log2 |level|)) -- 1 for the cbf; a level of 1
 * costs 3 (significance, greater-1, sign), larger levels grow like an exp-Golomb code.  Not counted: the significance flags of zero levels, the last
 * position, any context effect.
 *   Step 4, the choice per depth-0 TU, in 64 bits: lam_q8 = floor(lambda * 256 + 0.5) with lambda = 0.57 * 2^((qp - 12) / 3), computed on the host
 * (fhevc_motion_rd_lambda_q8) and handed to the kernel by value; J0 = 256 D0 + lam_q8 (1 + r0); J1 = 256 sum D1 + lam_q8 (1 + sum r1) over the four
 * children; the split is taken iff some child holds a non-zero level AND J1 < J0, strictly (TEncSearch.cpp:5117: uiCbfAny && dSubdivCost < dSingleCost).
 * Node: cost_rd = min((sum of the chosen J + lam_q8 * side_bits) >> 8, 0xFFFFFFFE).
 *   Field order (pinned: 16 bytes without padding; dword 1 and byte 10 are where the existing tree kernels read): */
#define FHEVC_RD_SOURCE_MERGE    0
#define FHEVC_RD_SOURCE_EXPLICIT 1
typedef struct {
  uint32_t dist;            /* D summed over the chosen TUs */
  uint32_t cost_rd;         /* dword 1: where merge and selection records keep cost_best */
  uint16_t bits;            /* everything lam_q8 multiplies: sum over the depth-0 TUs of 1 + the chosen r, + side_bits; saturated at 65535 */
  uint8_t  flags;           /* byte 10: where fhevc_motion_skip_node keeps flags.  bit 0: every depth-0 level zero under add_plain; bit 1: zero under
                               add_half -- the skip stage's two bits, by the same arithmetic; bit 2: some TU split */
  uint8_t  tu_split;        /* bit i: depth-0 TU i (raster in the node) is split; only the 64x64 node uses bits 1..3 */
  int16_t  mvx, mvy;        /* the vector, copied from the input record */
} fhevc_motion_rd_node;     /* 16 bytes; an invalid node gets dist = cost_rd = 0xFFFFFFFF, bits = 0xFFFF, flags = tu_split = 0 and a zero vector */
/* Device form: d_in, d_out: (num_frames - 1) * band CTUs * 85 records of 16 bytes, d_mvp as many of 8, compact over the band; the output is written over
 * exactly that extent, an empty band writes nothing.  The kernel keeps the skip kernel's mapping and buffers and runs four passes per TU depth through
 * them -- forward rows, forward columns with quantiser, pricing and dequantiser in registers, and the two inverse stages on transposed matrices --, then
 * takes the squared error of the rebuilt tile; by a count of its code about three times the skip stage's dot products (an expectation, not a
 * measurement).  Asynchronous with respect to the host, allocates nothing, keeps NO state in HBM between calls: calls with different QPs, ranges and
 * sources may be in flight on two streams.  FHEVC_E_INVALID with a fhevc_last_error text (nothing is launched or written): what
 * fhevc_motion_skip_device rejects, source outside 0..1, d_mvp together with source 0, a pointer that is not 4-byte aligned.  Timed under slot 29 of
 * fhevc_kernel_timing (28 stays rejected).
 * NOT covered: RDOQ, the third TU depth of 32x32 and 16x16 CUs, the partition sizes other than 2Nx2N (their prediction is composed from two vectors),
 * transform skip, sign hiding, chroma, CABAC's contexts.  The encoder hook does not consume this output. */
int  fhevc_motion_rd_device(fhevc_ctx* ctx, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples, int num_frames,
                            int ctu_row_begin, int ctu_row_end, int qp, int max_range, int source, const void* d_in, const fhevc_motion_mvp* d_mvp /* or NULL */,
                            fhevc_motion_rd_node* d_out, void* stream);
/* one picture pair, host buffers (both planes with the same stride), synchronous, as fhevc_motion_skip; in, out: numCtus * 85; mvp: numCtus * 85 or NULL */
int  fhevc_motion_rd(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int max_range, int source, const void* in,
                     const fhevc_motion_mvp* mvp /* or NULL */, fhevc_motion_rd_node* out);
/* lam_q8 of a QP (clamped to 0..51); needs no context */
uint32_t fhevc_motion_rd_lambda_q8(int qp);

/* The tree on RD costs: fhevc_p_tree_select_skip[_device], byte for byte, with three substitutions: rd_explicit[k].cost_rd stands where
 * shapes[k].cost_best is read, rd_merge[k].cost_rd where merge[k].cost_best is read, rd_merge[k].flags where skip[k].flags is read.  The record layout
 * makes these the same byte offsets, so both forms forward to the existing implementation; the device form is timed under slot 17.  This is HM with 2Nx2N
 * and merge as its ONLY inter candidates, decided on RD costs: a statement about two of the seven partition sizes.  FHEVC_E_INVALID: what the skip tree
 * rejects. */
int  fhevc_p_tree_select_rd(const fhevc_motion_rd_node* rd_explicit /* 85 */, const fhevc_motion_rd_node* rd_merge /* 85 */, int skip_mask, int valid_w,
                            int valid_h, const fhevc_p_tree_rule* rule, uint8_t* depth_min /* 256 or NULL */, uint8_t* depth_max /* 256 or NULL */,
                            fhevc_p_tree_node* tree /* 85 or NULL */);
int  fhevc_p_tree_select_rd_device(fhevc_ctx* ctx, const fhevc_motion_rd_node* d_rd_explicit, const fhevc_motion_rd_node* d_rd_merge, int skip_mask,
                                   int num_pictures, int ctu_row_begin, int ctu_row_end, const fhevc_p_tree_rule* rule, uint8_t* d_depth_min,
                                   uint8_t* d_depth_max, fhevc_p_tree_node* d_tree, void* stream);

/* ---- config 4 (P slices): the RD estimate of a CU node under any of HM's seven inter partition sizes (the PU instances of k_motion_rd.hip) ---------
 * fhevc_motion_rd prices one vector per node, so the RD tree above speaks of 2Nx2N and merge alone, while the selection (fhevc_pu_shape_select*) picks a
 * partition size on Hadamard costs.  This entry point closes that gap: the CU's prediction is composed from its two PUs' vectors -- what
 * TComPrediction::motionCompensation does per PU -- before the residual goes through transform, quantiser and rebuild; several launches fold into one record
 * per node, and the RD tree reads the folded records.
 *   The record (pinned: 16 bytes without padding; cost_rd stays in dword 1 and flags in byte 10, where the tree kernels read): */
typedef struct {
  uint32_t dist;  uint32_t cost_rd;  uint16_t bits;  uint8_t flags;  uint8_t tu_split;   /* bytes 0..11: fhevc_motion_rd_node's, same meaning */
  uint8_t  part;            /* the PartSize priced, 255 in a marker record */
  uint8_t  merged;          /* bit i: part i took its merge vector */
  uint8_t  pad[2];          /* written 0 */
} fhevc_motion_rd_pu_node;  /* 16 bytes; marker: dist = cost_rd = 0xFFFFFFFF, bits = 0xFFFF, flags = tu_split = merged = 0, part = 255 */
/*   Inputs travel in one struct: device pointers for the device form, host pointers for the host form.  Counts per CTU: 85 / 124 / 384. */
typedef struct {
  const fhevc_motion_qpel_node  *nodes, *pus, *pus_small;       /* refined or re-priced; 85 / 124 / 384 per CTU */
  const fhevc_motion_merge_node *merge_pus, *merge_pus_small;   /* fhevc_motion_merge_pu*'s records, or NULL */
  const fhevc_motion_mvp        *mvp_nodes, *mvp_pus, *mvp_pus_small;   /* the re-pricing's predictor records, or NULL */
  const fhevc_pu_shape_node     *shapes;                        /* needed by part_mode 8 and 9 only */
  const fhevc_motion_rd_pu_node *fold;                          /* an earlier launch's output, or NULL */
} fhevc_motion_rd_pu_inputs;
/*   part_mode 0, 1, 2, 4, 5, 6, 7: that HM PartSize (FHEVC_PART_*) for every node; 8: the node's shapes[k].best; 9: the node's shapes[k].second.
 *   Per node k of level l (s = 64 >> l), with p the size chosen for it; the node is INSIDE as everywhere else.
 *   p = 0: one vector, the node's own record in nodes.  Validity and side bits are exactly fhevc_motion_rd_device's with FHEVC_RD_SOURCE_EXPLICIT, with
 * mvp_nodes given or not.  The node's own merge candidate keeps entering at the tree, as before.
 *   p in {1, 2, 4..7}: the two parts are the entries the cost table of fhevc_pu_shape_select names (the formulas there: pus / pus_small by k and shape).
 * The size is unavailable for that node, and the record is a marker, in three cases: AMP at level 3, a NULL family, and p = 3 / 255 (or any other number a
 * selection record may hold that is no PartSize).
 *   Per part the selection's own rule applies (fhevc_pu_shape_select_merge, HM's uiMRGCost < uiMECost): if the family's merge array is given and the merge
 * record's cost_best is strictly smaller than the refined record's, the part takes the merge record's vector; its side bits are then idx + 1, or 4 for
 * idx == 4.  Otherwise it takes the refined vector; its side bits are then bits of its predictor record where that family's mvp_* is given (idx == 255
 * makes the part invalid), else eg(mvx) + eg(mvy).  A marker loses to anything; both markers make the part invalid; a part whose chosen vector is beyond
 * 4 max_range + 3 in either component is invalid.
 *   The node is valid iff it is INSIDE and both parts are valid.
 *   The prediction is fhevc_motion_refine's prediction per sample at the vector of the part whose getPartIndexAndSize rectangle holds the sample.
 *   Residual, TU sizes, transform, quantiser, dequantiser, inverse transform, SSE, bit estimate, TU choice and cost_rd are word for word those of
 * fhevc_motion_rd; side_bits is the sum over the parts.
 *   The TU tree does not depend on the partition size: under this configuration the interSplitFlag of TComDataCU::getQuadtreeTULog2MinSizeInCU
 * (TComDataCU.cpp:1478-1503) needs QuadtreeTUMaxDepthInter == 1, and the cfg has 3, so a two-part CU gets the TU sizes of a 2Nx2N CU.
 *   The bits of the part mode and of the merge flags are left out, as every other stage leaves them out.
 *   Fold: with fold given, the record written is the new one iff it is valid and (the fold record is a marker, i.e. its cost_rd is 0xFFFFFFFF, or the new
 * cost_rd < the fold record's cost_rd), strictly; otherwise the fold record's 16 bytes are written unchanged.  HM's xCheckBestMode keeps the earlier mode
 * on a tie, so a caller gets HM's order by launching in HM's order.  fold == d_out is allowed: each record is read and written by the same lane.  An
 * overlap of the two extents that is not equality is rejected.
 *   Device form: planes, band, frame pairing, the compact-over-the-band layout, qp 0..51, max_range 1..64, the stream contract and asynchrony are
 * fhevc_motion_rd_device's.  The output is written over exactly its extent ((num_frames - 1) * band CTUs * 85 records); an empty band writes nothing.  No
 * per-context or HBM state: launches with different QPs, ranges and part modes may be in flight on two streams.  FHEVC_E_INVALID with a fhevc_last_error
 * text (nothing is launched or written): what fhevc_motion_rd_device rejects; a null struct, nodes or d_out; part_mode outside {0, 1, 2, 4..9}; a non-zero
 * part_mode without pus; 8 / 9 without shapes; a merge or predictor array whose family's records are NULL; any pointer that is not 4-byte aligned; the
 * partial overlap above.  Timed under slot 31 of fhevc_kernel_timing (30 stays rejected).
 *   The kernel is a further instantiation of the RD kernel: the same mapping and buffers; per lane the node's p, its two parts' records, the merged decision
 * and the side bits; one prediction at the vector of the part that holds the first 4x4 quadrant of the lane's tile, and only where a tile straddles the cut
 * (AMP of the 16x16 nodes, both sizes of the 8x8 nodes) a second one at the other part's vector.
 * NOT covered: what fhevc_motion_rd does not cover (RDOQ, the third TU depth of 32x32 and 16x16 CUs, chroma, CABAC's contexts), the bits of the part mode and
 * of the merge flag, a skip test per PU, the temporal merge candidate, several sizes in one launch.  The encoder hook does not consume this output. */
int  fhevc_motion_rd_pu_device(fhevc_ctx* ctx, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples, int num_frames,
                               int ctu_row_begin, int ctu_row_end, int qp, int max_range, int part_mode, const fhevc_motion_rd_pu_inputs* inputs,
                               fhevc_motion_rd_pu_node* d_out, void* stream);
/* one picture pair, host buffers (both planes with the same stride), synchronous, as fhevc_motion_rd; every array of inputs is a host array of numCtus * 85 /
 * 124 / 384 entries or NULL; out: numCtus * 85 (out == inputs->fold is allowed) */
int  fhevc_motion_rd_pu(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int max_range, int part_mode,
                        const fhevc_motion_rd_pu_inputs* inputs, fhevc_motion_rd_pu_node* out);

/* The RD tree on folded records: typed forwarders to fhevc_p_tree_select_rd[_device] -- folded fhevc_motion_rd_pu_node records stand where rd_explicit
 * stands (bytes 0..11 are the same fields); no new tree kernel, the device form is timed under slot 17.  With the records of part_mode 0, 8 and 9 folded
 * this is HM with 2Nx2N, the selection's two sizes and merge as its inter candidates.  FHEVC_E_INVALID: what fhevc_p_tree_select_rd rejects. */
int  fhevc_p_tree_select_rd_pu(const fhevc_motion_rd_pu_node* rd_pu /* 85 */, const fhevc_motion_rd_node* rd_merge /* 85 */, int skip_mask, int valid_w,
                               int valid_h, const fhevc_p_tree_rule* rule, uint8_t* depth_min /* 256 or NULL */, uint8_t* depth_max /* 256 or NULL */,
                               fhevc_p_tree_node* tree /* 85 or NULL */);
int  fhevc_p_tree_select_rd_pu_device(fhevc_ctx* ctx, const fhevc_motion_rd_pu_node* d_rd_pu, const fhevc_motion_rd_node* d_rd_merge, int skip_mask,
                                      int num_pictures, int ctu_row_begin, int ctu_row_end, const fhevc_p_tree_rule* rule, uint8_t* d_depth_min,
                                      uint8_t* d_depth_max, fhevc_p_tree_node* d_tree, void* stream);
/* One picture pair, host buffers, synchronous -- the first frame call that reaches the RD stage.  On the context's stream, in order: the chain of
 * fhevc_p_tree_amvp_frame up to and including fhevc_pu_shape_select_merge_device, this time keeping the re-pricing's predictor records;
 * fhevc_motion_rd_device on the nodes' merge records; fhevc_motion_rd_pu_device with part_mode 0, then 8 and then 9 folded in place;
 * fhevc_p_tree_select_rd_pu_device with skip_mask.  The RD launches run at the range of the chain's merge stages (search_range, or 64 around centres).
 * Downloads the two maps and, where asked (non-NULL), the shapes, the nodes' merge records, their RD records and the folded RD records, numCtus * 85 each.
 * coarse_range 0 and 1..14 as for the other frame calls. */
int  fhevc_p_tree_rd_frame(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range, int coarse_range,
                           const fhevc_pu_shape_rule* shape_rule, const fhevc_p_tree_rule* tree_rule, int skip_mask, uint8_t* depth_min, uint8_t* depth_max,
                           fhevc_pu_shape_node* shapes, fhevc_motion_merge_node* merge, fhevc_motion_rd_node* rd_merge, fhevc_motion_rd_pu_node* rd_pu);

/* ---- config 4 (P slices): the RD estimates with HM's full residual quad-tree: the third TU depth (further instances of k_motion_rd.hip) -----------
 * fhevc_motion_rd* and fhevc_motion_rd_pu* price two TU sizes per node.  That is HM's complete residual quad-tree for 64x64 and 8x8 CUs and one depth
 * short for 32x32 and 16x16 CUs: a 32x32 node can use TUs of 32 and 16 while its four 16x16 children can use 16 and 8, so wherever the smallest transform
 * pays, the RD tree books that gain as a gain of the CU split.  HM sees the same TU sizes on both sides (xEstimateInterResidualQT,
 * TEncSearch.cpp:4556-5160).  The entry points below take the depth count as an argument, tu_depths, placed before the output pointer.
 *   tu_depths 2: every byte is what the entry point without _qt writes; the launch IS that entry point's launch (the same kernel instances, the same timing
 * slot 29 or 31).
 *   tu_depths 3: nodes of 64x64 and 8x8 are priced exactly as before -- their bytes equal the tu_depths 2 bytes.  A node of side s = 32 or 16 gets N0 = s,
 * N1 = s / 2, N2 = s / 4: 32 -> 32, 16, 8 and 16 -> 16, 8, 4.  Per TU of any size, step 3 of fhevc_motion_rd applies word for word, on the same residual:
 * it yields D, r = 1 + sum (3 + 2 floor(log2 |level|)) and cbf (some level non-zero).  Inter 4x4 takes the DCT.
 *   The choice is HM's recursion (TEncSearch.cpp:5020-5134), bottom-up, in 64 bits, with lam = lam_q8.
 *   Per depth-1 TU i, in raster order inside the node (i = 2 * (row half) + (column half)):
 *     K1_i = 256 D1_i + lam (1 + r1_i) -- the 1 is this TU's own split flag, which exists now that it can split;
 *     K2_i = 256 sum D2 + lam (1 + sum r2) over its four children;
 *     take1_i = (some child has a non-zero level) AND K2_i < K1_i, strictly;
 *     C_i = take1_i ? K2_i : K1_i;
 *     coded_i = take1_i OR cbf1_i -- HM's uiCbfAny one level up: HM ORs the cbf of a split child into the parent's depth (:5093-5101), so a depth-0 TU
 *   whose only coded descendants sit at depth 2 counts as coded.
 *   Per depth-0 TU: J0 = 256 D0 + lam (1 + r0), unchanged; J1 = sum C_i + lam; take0 = (some coded_i) AND J1 < J0, strictly.
 *   Per node: cost_rd = min((chosen J + lam * side_bits) >> 8, 0xFFFFFFFE); dist is D summed over the chosen TUs; bits is everything lam multiplies in the
 * chosen J, + side_bits, saturated at 65535.
 *   With no third depth K1_i carries no flag and never splits: that is J1 of fhevc_motion_rd.  So tu_depths 2 is the special case of this definition, not a
 * second one.  A node that splits at depth 0 and nowhere at depth 1 therefore costs four flag bits MORE at tu_depths 3 than at 2.
 *   Record types are unchanged (fhevc_motion_rd_node, fhevc_motion_rd_pu_node: 16 bytes, dword 1 and byte 10 where the tree reads them).  flags keeps its
 * meaning: bits 0 and 1 are depth-0 properties, bit 2 means depth 0 split.  tu_split gains bits 4..7: bit 4 + i is set when depth-1 TU i of a 32x32 or
 * 16x16 node is split; these bits are zero unless bit 0 is set.  Bits 1..3 stay the 64x64 node's.  The existing tree kernels and forwarders
 * (fhevc_p_tree_select_rd*, fhevc_p_tree_select_rd_pu*) read these records as they are; there is no new tree kernel.
 *   Everything else -- inputs, validity, side bits, the composed prediction, the fold (which works across launches of either depth count, in place where
 * wanted), planes, band, stream, asynchrony -- is the mirrored entry point's.  FHEVC_E_INVALID with a fhevc_last_error text (nothing is launched or
 * written): what the mirrored call rejects, and tu_depths outside {2, 3}.  No per-context or HBM state: calls with different tu_depths, QPs and ranges
 * may be in flight on two streams.  Timed under slot 35 of fhevc_kernel_timing at tu_depths 3 (34 stays rejected); at tu_depths 2 under the mirrored
 * call's slot.
 *   The kernel: eight further instances of the RD kernel.  A third pass group runs over the level-1 buffer at N = 8 and the level-2 buffer at N = 4 alone,
 * by all 256 threads; the sums are kept per depth-1 TU (16 + 64 of them, four words each) in the dead window behind the matrices, and the writer lane makes
 * the nested choice.  By a count of the code about a quarter more transform work than two depths (an expectation, not a measurement).
 * NOT covered: the third depth of the intra candidate (fhevc_intra_rd* stays two depths deep; it takes records folded at either depth count as d_fold
 * unchanged), RDOQ, a fitted bit model, HM's per-TU zero-cost comparison, chroma.  The encoder hook does not consume this output. */
int  fhevc_motion_rd_qt_device(fhevc_ctx* ctx, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples, int num_frames,
                               int ctu_row_begin, int ctu_row_end, int qp, int max_range, int source, const void* d_in, const fhevc_motion_mvp* d_mvp /* or NULL */,
                               int tu_depths, fhevc_motion_rd_node* d_out, void* stream);
int  fhevc_motion_rd_qt(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int max_range, int source, const void* in,
                        const fhevc_motion_mvp* mvp /* or NULL */, int tu_depths, fhevc_motion_rd_node* out);
int  fhevc_motion_rd_pu_qt_device(fhevc_ctx* ctx, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples, int num_frames,
                                  int ctu_row_begin, int ctu_row_end, int qp, int max_range, int part_mode, const fhevc_motion_rd_pu_inputs* inputs,
                                  int tu_depths, fhevc_motion_rd_pu_node* d_out, void* stream);
int  fhevc_motion_rd_pu_qt(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int max_range, int part_mode,
                           const fhevc_motion_rd_pu_inputs* inputs, int tu_depths, fhevc_motion_rd_pu_node* out);
/* fhevc_p_tree_rd_frame's chain with all four RD launches (the merge records, part_mode 0 / 8 / 9 folded) at tu_depths: the two sides of every comparison of
 * the RD tree then stand on one footing.  At tu_depths 2 every byte is fhevc_p_tree_rd_frame's.  Rejects what that call rejects, and tu_depths outside
 * {2, 3}. */
int  fhevc_p_tree_rd_qt_frame(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range, int coarse_range,
                              const fhevc_pu_shape_rule* shape_rule, const fhevc_p_tree_rule* tree_rule, int skip_mask, int tu_depths, uint8_t* depth_min,
                              uint8_t* depth_max, fhevc_pu_shape_node* shapes, fhevc_motion_merge_node* merge, fhevc_motion_rd_node* rd_merge,
                              fhevc_motion_rd_pu_node* rd_pu);

/* ---- config 4 (P slices): the RD estimate of the intra candidate per CU node, folded per CU (the intra instances of k_motion_rd.hip) --------------
 * The tree that takes the intra candidate (fhevc_p_tree_select_intra*, further below) compares Hadamard costs; the RD tree above compares SSE + lambda
 * bits and has no intra candidate, so a node whose content is not in the reference picture can only split there.  This stage prices ONE intra mode per
 * node -- the first pass's winner -- in the RD stage's unit and folds it into the records the RD tree already reads.
 *   Input per CTU: the 85 fhevc_node_cost records of fhevc_intra_first_pass_device for the same picture, compact over the band, and the luma planes in the
 * layout, band and stream arguments of fhevc_intra_first_pass_device.  There is no frame pairing: num_frames pictures give num_frames * band CTUs * 85
 * records; a caller that folds into the records of picture pairs passes plane and record pointers offset by one picture.
 *   Of a first-pass record only satd (dword 0) and the low byte of mode (dword 1) are read; any byte content is legal.  A node is valid iff it is INSIDE,
 * satd != 0xFFFFFFFF and that byte is <= 34.  No input byte reaches an address or a loop bound: an invalid node predicts with mode 0 and its result is
 * dropped.
 *   Prediction: for a TU that is node t of size n in {32, 16, 8} and mode m, exactly what the first pass evaluates for (t, m): the reference line from the
 * ORIGINAL plane with coding-order availability and HM's substitution walk, the smoothing as the first pass applies it, the filter decision by (m, n), the
 * predictor with its edge filters (the oracle's fho_fill_ref, fho_filter_ref, fho_use_filtered_ref, fho_pred_intra).  The z-order availability of a TU
 * inside a CU is that of the node of that size at that place, so every line is one of the 85 the first pass builds.
 *   TUs of a node of level l (s = 64 >> l): the depth-0 TUs are the nodes of level max(l, 1) inside it (N0 = min(s, 32); a 64x64 node has four), the
 * depth-1 TUs the nodes one level further down (N1 = N0 / 2).  Both depths use the node's one mode; an intra TU is predicted from its own neighbours, so
 * the two depths have different residuals.  An 8x8 node has depth 0 only (tu_split 0).
 *   Per TU everything is word for word step 3 of fhevc_motion_rd on r = original - prediction: xTrMxN, the plain quantiser, xDeQuant, xITrMxN, xGetSSE
 * with its per-sample shift, r(TU) = 1 + sum (3 + 2 floor(log2 |level|)), lam_q8 = fhevc_motion_rd_lambda_q8(qp).
 *   Per depth-0 TU, in 64 bits: J0 = 256 D0 + lam_q8 (1 + r0), J1 = 256 sum D1 + lam_q8 (1 + sum r1); the split is taken iff J1 < J0, strictly.  This
 * differs from the inter rule of fhevc_motion_rd, which also asks that some child is coded: HM's intra recursion compares dSplitCost < dSingleCost alone
 * (TEncSearch.cpp:1661 against :5117).
 *   Node result: side_bits = bits(m) of fhevc_intra_p (2 / 3 / 6); cost_rd = min((sum J + lam_q8 side_bits) >> 8, 0xFFFFFFFE); bits and dist as in the RD
 * record; flags bit 0: every depth-0 level is zero under add_plain, bit 1: under add_half, bit 2: some TU split.  The record is a
 * fhevc_motion_rd_pu_node with part = FHEVC_RD_PART_INTRA, merged = 0, pad[0] = the mode, pad[1] = 0; the marker is that record's marker (part 255).
 *   Calm gate (fhevc_p_tree_select_intra's rule 1 on RD records): with d_rd_merge given, a node is CALM iff its merge RD record's cost_rd is strictly
 * smaller than the fold record's (an absent fold or a marker counts as the largest number; a marker merge record is never smaller) and
 * rd_merge.flags & skip_mask != 0.  HM does not try intra where the best mode so far has no coded residual (TEncCu.cpp:799-804).  A calm node keeps the
 * fold record's 16 bytes, the marker where there is no fold.
 *   Fold (fhevc_motion_rd_pu's rule): with d_fold given, the intra record is written iff it is valid and strictly cheaper than the fold record, else the
 * fold record unchanged: HM tries intra after the inter sizes and keeps the earlier mode on a tie.  d_fold == d_out is allowed: each record is read and
 * written by the same lane.  Any other overlap of the two extents is rejected.  With d_fold and d_rd_merge NULL and skip_mask 0 the output is the plain
 * intra RD record of every valid node.
 *   Asynchronous on `stream` (NULL: the context's), allocates nothing, keeps no HBM state between calls: calls with different QPs may be in flight on two
 * streams.  The output is written over exactly its extent; an empty band writes nothing.  FHEVC_E_INVALID with a fhevc_last_error text (nothing is launched
 * or written): what fhevc_intra_first_pass_device rejects; a null d_first or d_out; skip_mask outside 0..3; a pointer that is not 4-byte aligned; the
 * partial overlap above.  Timed under slot 33 of fhevc_kernel_timing (32 stays rejected).
 * NOT covered: 4x4 TUs, and with them the DST, NxN and the depth-1 split of 8x8 CUs; the third TU depth, RDOQ, transform skip, chroma and reconstructed
 * neighbours; HM's RD search over the candidate list and MPMs (the stage takes one mode per node); the mode-flag bits; the margin fit and any hook
 * consumer.  Nothing here can be pinned to HM's own intra coding, which predicts from reconstructed neighbours. */
#define FHEVC_RD_PART_INTRA 16
int  fhevc_intra_rd_device(fhevc_ctx* ctx, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples, int num_frames,
                           int ctu_row_begin, int ctu_row_end, int qp, const fhevc_node_cost* d_first, const fhevc_motion_rd_pu_node* d_fold,
                           const fhevc_motion_rd_node* d_rd_merge, int skip_mask, fhevc_motion_rd_pu_node* d_out, void* stream);
/* one picture, host buffers, synchronous: first, fold (or NULL), rd_merge (or NULL) and out are host arrays of numCtus * 85 records (out == fold is allowed) */
int  fhevc_intra_rd(fhevc_ctx* ctx, const int16_t* luma, int stride_samples, int qp, const fhevc_node_cost* first, const fhevc_motion_rd_pu_node* fold,
                    const fhevc_motion_rd_node* rd_merge, int skip_mask, fhevc_motion_rd_pu_node* out);
/* fhevc_p_tree_rd_frame with the intra candidate.  On the context's stream, in order: the whole chain of fhevc_p_tree_rd_frame up to the folded inter
 * records; fhevc_intra_first_pass_device on the CURRENT picture; fhevc_intra_rd_device with the folded records as d_fold (in place), the merge RD records
 * as d_rd_merge, and skip_mask; fhevc_p_tree_select_rd_pu_device.  There is no new tree kernel: the tree reads dword 1 and byte 10 as before.  Downloads
 * what fhevc_p_tree_rd_frame downloads (rd_pu: the records folded with the intra candidate) and, where asked, the first-pass records, numCtus * 85.  A
 * rejected call moves nothing. */
int  fhevc_p_tree_rd_intra_frame(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range,
                                 int coarse_range, const fhevc_pu_shape_rule* shape_rule, const fhevc_p_tree_rule* tree_rule, int skip_mask, uint8_t* depth_min,
                                 uint8_t* depth_max, fhevc_pu_shape_node* shapes, fhevc_motion_merge_node* merge, fhevc_motion_rd_node* rd_merge,
                                 fhevc_motion_rd_pu_node* rd_pu, fhevc_node_cost* first);

/* ---- config 4 (P slices): the intra candidate on HM's full TU tree: the third depth, 4x4 TUs, the DST (two further intra instances of k_motion_rd.hip) ----
 * fhevc_intra_rd* above prices two TU sizes per node and no 4x4 TU, while the inter candidates it is folded with are priced on HM's complete residual
 * quad-tree at tu_depths 3 (fhevc_motion_rd_qt*).  These entry points take the depth count, as those do: tu_depths stands before the output pointer.
 *   tu_depths 2: every byte is what the entry point without _qt writes, the launch is that entry point's launch (the same two kernel instances, slot 33);
 * the entry points without _qt are forwarders with tu_depths 2.
 *   tu_depths 3 (HM: QuadtreeTUMaxDepthIntra 3, minimum TU 4).  TU sizes: a node of side s has N0 = min(s, 32);
 *     64x64: 32, 16 -- unchanged, its bytes equal the tu_depths 2 bytes;   32x32: 32, 16, 8;   16x16: 16, 8, 4;   8x8: 8, 4 -- the depth-1 split it never had.
 *   Prediction: the node's ONE mode at every depth; per TU of size n at (x0, y0) what the oracle composes for that block: fho_fill_ref(x0, y0, n) ->
 * fho_filter_ref -> fho_use_filtered_ref(m, n) -> fho_pred_intra, n = 4 included.  For n >= 8 the line is one of the 85 the first pass builds, as above.  A
 * 4x4 TU takes the line of the 4x4 block at that place: 17 samples of the ORIGINAL plane, z-order availability in 4-sample units (what
 * fhevc_intra_first_pass_4x4 evaluates for the block), HM's substitution walk, the edge filters of n <= 16.  The filter decision at n = 4 never selects the
 * smoothed line (its threshold is 10 and no mode is further than 8 from modes 10 and 26), so no smoothed 4x4 line is built.
 *   Transform: per TU step 3 of fhevc_motion_rd word for word, on r = original - prediction of that depth -- except that an intra 4x4 luma TU takes HM's
 * DST-VII: g_as_DST_MAT_4 = { 29, 55, 74, 84 / 74, 74, 0, -74 / 84, -29, -74, 55 / 55, -84, 74, -29 } (TComRom.cpp:513-517) through fastForwardDst /
 * fastInverseDst (TComTrQuant.cpp:412-466), selected in xTrMxN / xITrMxN (:876, :898, :945, :969); the shifts and clips are those of the 4-point DCT.
 * Inter 4x4 TUs (fhevc_motion_rd_qt*) keep the DCT.
 *   Choice: HM's intra recursion (TEncSearch.cpp:1610-1661), bottom-up, in 64 bits, with lam = lam_q8.  The test is dSplitCost < dSingleCost ALONE at every
 * depth; the coded-child condition of fhevc_motion_rd_qt is the inter rule's and does not apply.
 *   Per depth-1 TU i of a 32x32 or 16x16 node, in raster order (i = 2 * (row half) + (column half)):
 *     K1_i = 256 D1_i + lam (1 + r1_i);   K2_i = 256 sum D2 + lam (1 + sum r2) over its four children;   take1_i = K2_i < K1_i, strictly;
 *     C_i = take1_i ? K2_i : K1_i.
 *   Per depth-0 TU: J0 = 256 D0 + lam (1 + r0), unchanged; J1 = sum C_i + lam; take0 = J1 < J0, strictly.
 *   The depth-1 TUs of an 8x8 node are leaves: J1 = 256 sum D1 + lam (1 + sum r1), the two-depth formula on the residuals of the four 4x4 DST TUs.
 *   Two depths are the special case in which K1 carries no flag and never splits: this is not a second definition.
 *   Record: cost_rd = min((sum of the chosen J + lam * bits(m)) >> 8, 0xFFFFFFFE); dist and bits are taken over the chosen TUs; flags bits 0 and 1 stay
 * depth-0 properties; flags bit 2 and tu_split bit 0 mean depth 0 split; tu_split bits 4..7 mean depth-1 TU i split -- zero unless bit 0 is set, and zero
 * for 8x8 and 64x64 nodes (bits 1..3 stay the 64x64 node's); part = FHEVC_RD_PART_INTRA, the mode in pad[0], 16 bytes.  The tree kernels read the records
 * as they are: there is no new tree kernel.
 *   Everything else is the mirrored entry point's: inputs, validity, bits(m), the calm gate, the fold (in place where wanted; it works across depth
 * counts), planes, band, stream, asynchrony.  FHEVC_E_INVALID with a fhevc_last_error text (nothing is launched or written): what the mirrored call
 * rejects, and tu_depths outside {2, 3}.  No per-context or HBM state: calls with different QPs and depth counts may be in flight on two streams.  Timed
 * under slot 37 of fhevc_kernel_timing at tu_depths 3 (36 stays rejected); at tu_depths 2 under slot 33.
 *   The kernel: the lines of the CTU's 256 4x4 blocks with their DC values are built from the staged CTU, one thread per block; a third prediction pass
 * runs at the level below (a lane's 8x8 tile then holds four 4x4 TUs with four lines); the transform passes are those of fhevc_motion_rd_qt's third depth
 * (N = 8 on the level-1 buffer, N = 4 on the level-2 buffer), the level-3 buffer's depth 1 runs at N = 4 for real, and every 4-point pass takes the DST
 * matrix.  Sums are kept per depth-1 TU; the writer lane makes the nested choice.
 * NOT covered: NxN with its four modes, HM's RD search over the candidate list, the mode-flag bits, reconstructed neighbours, transform skip, RDOQ,
 * chroma; the margin fit and any hook consumer. */
int  fhevc_intra_rd_qt_device(fhevc_ctx* ctx, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples, int num_frames,
                              int ctu_row_begin, int ctu_row_end, int qp, const fhevc_node_cost* d_first, const fhevc_motion_rd_pu_node* d_fold,
                              const fhevc_motion_rd_node* d_rd_merge, int skip_mask, int tu_depths, fhevc_motion_rd_pu_node* d_out, void* stream);
int  fhevc_intra_rd_qt(fhevc_ctx* ctx, const int16_t* luma, int stride_samples, int qp, const fhevc_node_cost* first, const fhevc_motion_rd_pu_node* fold,
                       const fhevc_motion_rd_node* rd_merge, int skip_mask, int tu_depths, fhevc_motion_rd_pu_node* out);
/* fhevc_p_tree_rd_intra_frame with the depth count.  In order: fhevc_p_tree_rd_qt_frame's chain at tu_depths; the first pass of the current picture;
 * fhevc_intra_rd_qt_device at tu_depths, folding in place under skip_mask; the RD tree.  At tu_depths 2 every byte is fhevc_p_tree_rd_intra_frame's.
 * Rejects what that call rejects, and tu_depths outside {2, 3}. */
int  fhevc_p_tree_rd_intra_qt_frame(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range,
                                    int coarse_range, const fhevc_pu_shape_rule* shape_rule, const fhevc_p_tree_rule* tree_rule, int skip_mask, int tu_depths,
                                    uint8_t* depth_min, uint8_t* depth_max, fhevc_pu_shape_node* shapes, fhevc_motion_merge_node* merge,
                                    fhevc_motion_rd_node* rd_merge, fhevc_motion_rd_pu_node* rd_pu, fhevc_node_cost* first);

/* ---- config 4 (P slices): the intra candidate with the NxN candidate of the 8x8 CUs, four modes (two further intra instances of k_motion_rd.hip) ----------
 * At the smallest CU HM checks xCheckRDCostIntra(SIZE_NxN) right behind SIZE_2Nx2N (TEncCu.cpp:806-815).  fhevc_intra_rd_qt* prices an 8x8 node with ONE
 * mode only: what the section above lists as not covered is covered by the entry points of this section.  The stage is fhevc_intra_rd_qt* at tu_depths 3 plus that
 * candidate; there is no tu_depths argument.  The NxN candidate exists only for 8x8 nodes (nodes 21..84).
 *   Input: beside everything fhevc_intra_rd_qt_device takes, d_first4: the 256 fhevc_node_cost records per CTU of fhevc_intra_first_pass_4x4_device for the
 * same pictures, in 16x16 raster of 4x4 units, compact over the band.  Of a record only satd (dword 0) and the low byte of mode (dword 1) are read; any byte
 * content is legal and none of it reaches an address or a loop bound.  The four PUs of 8x8 node (x, y) of the 8x8 raster are units (2x, 2y), (2x+1, 2y),
 * (2x, 2y+1), (2x+1, 2y+1): fhevc_intra_p's order.
 *   Validity: NxN is valid iff the node is INSIDE and each of the four records has satd != 0xFFFFFFFF and a mode byte <= 34.  An invalid candidate predicts
 * with mode 0 and is dropped.
 *   Prediction and transform: PU i is one 4x4 TU (uiInitTrDepth = 1, TEncSearch.cpp:2187-2188; 4 is the minimum TU, nothing splits further), predicted at
 * ITS mode m_i from the line of the 4x4 block at its place -- the line the section above builds: 17 original samples, z-order availability in 4-sample units, the
 * substitution walk, never smoothed, the edge filters of n <= 16; in oracle terms fho_fill_ref(x, y, 4) -> fho_pred_intra.  Then step 3 of fhevc_motion_rd
 * with the DST-VII, word for word as the 4x4 intra TUs above.
 *   Cost, in 64 bits: J = 256 * sum D_i + lam_q8 * (sum r_i + sum bits(m_i)); cost_rd = min(J >> 8, 0xFFFFFFFE); dist = sum D_i;
 * bits = min(sum r_i + sum bits(m_i), 65535); r_i = 1 + the level bits of TU i; bits(m) is fhevc_intra_p's (2 / 3 / 6).  NO split-flag bit is counted: HM
 * infers the split of an intra NxN CU at its own depth (TEncEntropy.cpp:241-244).  The part-mode bin is left out as everywhere else: at the smallest CU
 * both sizes cost one bin.
 *   Flags bits 0 and 1 are properties of the four TUs priced: every level is zero under add_plain, respectively under add_half, with the 4-point
 * quantiser's numbers.
 *   Choice: HM tries 2Nx2N first and xCheckBestMode keeps the earlier mode on a tie.  The stage's intra record is the NxN record iff NxN is valid and either
 * its cost_rd is STRICTLY smaller than the 2Nx2N record's or 2Nx2N is invalid; otherwise it is the bytes fhevc_intra_rd_qt_device writes at 3.  The calm
 * gate and the fold then act on that record unchanged; folding in place is allowed.
 *   The NxN record in the output: a fhevc_motion_rd_pu_node with part = FHEVC_RD_PART_INTRA_NXN (17), tu_split = 1, flags bit 2 set, merged = 0,
 * pad = {0, 0}.  The four modes are the caller's own d_first4 bytes.  The tree kernels read dword 1 and byte 10 as before: no tree kernel is added.
 *   d_nxn (or NULL): the plain NxN candidate of every 8x8 node, 64 fhevc_intra_rd_nxn_node per CTU in node order 21..84, compact over the band,
 * independent of the choice, the gate and the fold; cbf bit i: TU i has a non-zero level.  The marker: dist = cost_rd = 0xFFFFFFFF, bits = 0xFFFF,
 * flags = cbf = 0, modes 255 four times.  It is written over exactly its extent.
 *   d_first4 == NULL: every byte and the launch itself are fhevc_intra_rd_qt_device's at 3 (slot 37); d_nxn must then be NULL too, else FHEVC_E_INVALID.
 *   FHEVC_E_INVALID with nothing launched or written: what the mirrored call rejects, a d_first4 or d_nxn that is not 4-byte aligned, and any overlap of
 * d_nxn with another array of the call (the planes included).  No per-context or HBM state: calls with different QPs may be in flight on two streams.
 * Timed under slot 39 of fhevc_kernel_timing (38 stays rejected).
 *   The kernel: in the third pass the level-3 wave, whose buffer is idle there, predicts the four 4x4 blocks of each lane's tile at their four modes; the
 * pass takes the level-3 buffer along at N = 4 with the DST; three words per 8x8 node (D, level bits with the four cbf bits, max |c|) lie behind the sums
 * per depth-0 TU; the writer lane of the node forms J, compares and writes both records.  ONE launch per call.
 * NOT covered (stated departures): HM predicts PU i+1 from PU i's reconstruction -- here every line is from the original picture, as in every other
 * stage; HM searches eight candidates plus MPMs per PU -- here there is one mode per PU; transform skip (which HM tries only for NxN,
 * TEncSearch.cpp:1479), RDOQ, chroma's four PUs and the mode-flag bits; the margin fit and any hook consumer. */
#define FHEVC_RD_PART_INTRA_NXN 17
typedef struct fhevc_intra_rd_nxn_node {
  uint32_t dist;       /* sum D_i of the four 4x4 TUs */
  uint32_t cost_rd;    /* min(J >> 8, 0xFFFFFFFE) */
  uint16_t bits;
  uint8_t  flags;      /* bits 0, 1 as above; bit 2 set */
  uint8_t  cbf;        /* bit i: TU i has a non-zero level */
  uint8_t  modes[4];   /* the four modes priced, in fhevc_intra_p's order */
} fhevc_intra_rd_nxn_node;  /* 16 bytes */
int  fhevc_intra_rd_nxn_device(fhevc_ctx* ctx, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples, int num_frames,
                               int ctu_row_begin, int ctu_row_end, int qp, const fhevc_node_cost* d_first, const fhevc_node_cost* d_first4,
                               const fhevc_motion_rd_pu_node* d_fold, const fhevc_motion_rd_node* d_rd_merge, int skip_mask, fhevc_motion_rd_pu_node* d_out,
                               fhevc_intra_rd_nxn_node* d_nxn, void* stream);
/* the host form: one picture, first4 its 256 records per CTU (or NULL), nxn the 64 NxN records per CTU (or NULL; needs first4) */
int  fhevc_intra_rd_nxn(fhevc_ctx* ctx, const int16_t* luma, int stride_samples, int qp, const fhevc_node_cost* first, const fhevc_node_cost* first4,
                        const fhevc_motion_rd_pu_node* fold, const fhevc_motion_rd_node* rd_merge, int skip_mask, fhevc_motion_rd_pu_node* out,
                        fhevc_intra_rd_nxn_node* nxn);
/* fhevc_p_tree_rd_intra_qt_frame's chain at tu_depths 3 with the NxN candidate.  In order: fhevc_p_tree_rd_qt_frame's chain at 3; the first pass of the
 * current picture and fhevc_intra_first_pass_4x4_device on it (best records only); fhevc_intra_rd_nxn_device, folding in place under skip_mask; the RD
 * tree.  nxn (or NULL): the NxN records of the picture.  Rejects what fhevc_p_tree_rd_intra_qt_frame rejects. */
int  fhevc_p_tree_rd_intra_nxn_frame(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range,
                                     int coarse_range, const fhevc_pu_shape_rule* shape_rule, const fhevc_p_tree_rule* tree_rule, int skip_mask,
                                     uint8_t* depth_min, uint8_t* depth_max, fhevc_pu_shape_node* shapes, fhevc_motion_merge_node* merge,
                                     fhevc_motion_rd_node* rd_merge, fhevc_motion_rd_pu_node* rd_pu, fhevc_node_cost* first, fhevc_intra_rd_nxn_node* nxn);

/* ---- config 4 (P slices): the intra candidate searched over the first pass's candidate lists (two further intra instances of k_motion_rd.hip) ----------
 * fhevc_intra_rd_nxn* prices ONE mode per node and per 4x4 PU: the winner of the Hadamard pass.  HM keeps a list from that pass -- 3 modes for PUs of 16 and
 * above, 8 for 8x8 and 4x4 PUs (TEncSearch.cpp:2244, g_aucIntraModeNumFast_UseMPM) --, appends most-probable modes (:2297-2320) and decides among them on
 * RD cost in two steps (:2349-2480).  The stage of this section is fhevc_intra_rd_nxn* (three TU depths, DST, NxN) with the mode taken from a list.
 * Everything not named below is that stage's: planes, band, prediction per TU, transform, quantiser, bit estimate, lam, calm gate, fold (in place allowed),
 * record types, markers, asynchrony, no per-context or HBM state.
 *   Inputs.  d_modes is what fhevc_intra_first_pass_candidates_device writes with num_candidates = list_stride (1..8): 85 * list_stride bytes per CTU, best
 * first, compact over the band.  d_modes4 (or NULL) is the d_modes of fhevc_intra_first_pass_4x4_device with list_stride4: 256 * list_stride4 bytes per CTU.
 * Any byte content is legal.  No byte reaches an address or a loop bound.  The lists are byte arrays: no alignment is asked of them.
 *   The rule travels by value with the launch: count[l] for the nodes of level l (0: 64x64 .. 3: 8x8), count4 for the 4x4 PUs, append_planar 0 / 1, pad 0.
 *   The list of a node of level l is the first count[l] bytes of its entry; the list of a 4x4 PU is the first count4 bytes of its entry.  Bytes > 34 are
 * skipped.  With append_planar, mode 0 is appended behind the list iff the list has at least one valid entry and none of them is 0: what
 * getIntraDirPredictor gives when neither neighbour is intra-coded -- both directions DC, *piMode 1, one MPM appended, PLANAR (TComDataCU.cpp:1403-1421) --,
 * the common case in a P picture and the neighbourhood that bits(m) = 2 / 3 / 6 already assumes.  MPMs from coded intra neighbours stay a stated departure.
 * A node is valid iff it is INSIDE and its list is not empty.
 *   Step A (bCheckFirst): for every list entry c, in order,
 *     A_c = sum over the node's depth-0 TUs of J0 (the fhevc_intra_rd_qt J0, predicted at m_c) + lam * bits(m_c), in 64 bits.
 * Best and second are kept as HM keeps them: a candidate strictly below the best becomes the best, and the old best becomes the second; otherwise a
 * candidate strictly below the second becomes the second.  (The first valid entry is the best; with no second yet, any further entry is below it.)
 *   Step B: F(m) is the record fhevc_intra_rd_qt_device writes at tu_depths 3 for a node whose mode is m.  The node's record is F(best); it is F(second)
 * instead iff a second exists and its cost_rd is STRICTLY smaller, compared on the unshifted 64-bit J.  The record has part 16 and pad[0] = the mode;
 * pad[1] = the winner's position in the list (0 = the first pass's own winner; the appended planar counts as the position behind the last list byte
 * used, count[l]).
 *   NxN of the 8x8 nodes (only with d_modes4): a 4x4 PU has no split, so HM's two steps coincide.  Per PU i the candidate with the smallest
 * 256 D + lam (r + bits(m)) wins, strict < in list order.  The NxN record and the optional d_nxn record are the section above's over the four chosen modes
 * (NxN is valid iff the node is INSIDE and each of the four lists is not empty).  The choice against 2Nx2N, the gate and the fold are unchanged.  With
 * d_modes4 NULL there is no NxN candidate, and d_nxn must be NULL.
 *   FHEVC_E_INVALID with nothing launched or written: what fhevc_intra_rd_nxn_device rejects; a null d_modes or rule; strides outside 1..8; a count of 0,
 * or a count above its stride; append_planar above 1, or a non-zero pad; d_nxn without d_modes4; any overlap of an input list with an output.
 * (list_stride4 and count4 are not looked at where d_modes4 is NULL.)
 *   Timed under slot 41 of fhevc_kernel_timing (40 and 42 stay rejected).
 *   Identities: (i) with all counts 1 and append_planar 0 every byte of d_out and d_nxn equals fhevc_intra_rd_nxn_device fed records whose modes are the
 * lists' first bytes, with or without the 4x4 input, through gate and fold; (ii) the output record of any node equals fhevc_intra_rd_qt_device's record at 3
 * for a `first` array holding the winning mode, in all bytes but pad[1]; (iii) F(m).J <= A(m), so the result never costs more
 * than step A's cost of the list's first valid entry (not: than F of that entry -- the two steps rank on A, and a mode ranked third there is never tried on the
 * full tree).
 *   The kernel: ONE launch per call.  Per CTU, behind the lines: the positions of the 4x4 PUs' lists in passes of their own over the level-3 buffer (N = 4,
 * DST, all four waves; sums and best per PU in LDS); then one loop of phases -- the positions of step A run the prediction and the depth-0 pass alone,
 * the writer lane of each node keeps best and second in LDS and clears the sums; then the three depths at the best mode and again at the second (a wave
 * whose list is exhausted keeps the barriers and its result is dropped).  80 532 B of static LDS, no scratch.
 * NOT covered (stated departures): MPMs from coded intra neighbours, reconstructed neighbours, transform skip, RDOQ, chroma, the mode-flag bits; the margin
 * fit and any hook consumer. */
typedef struct fhevc_intra_search_rule {
  uint8_t count[4];        /* list entries read per node of level 0..3 */
  uint8_t count4;          /* ... per 4x4 PU */
  uint8_t append_planar;   /* 0 / 1 */
  uint8_t pad[2];          /* 0 */
} fhevc_intra_search_rule;  /* 8 bytes */
/* HM: count {3, 3, 3, 8}, count4 8, append_planar 1 */
void fhevc_intra_search_rule_default(fhevc_intra_search_rule* rule);
int  fhevc_intra_rd_search_device(fhevc_ctx* ctx, const void* d_luma, int sample_bytes, int stride_samples, long long frame_stride_samples, int num_frames,
                                  int ctu_row_begin, int ctu_row_end, int qp, const uint8_t* d_modes, int list_stride, const uint8_t* d_modes4, int list_stride4,
                                  const fhevc_intra_search_rule* rule, const fhevc_motion_rd_pu_node* d_fold, const fhevc_motion_rd_node* d_rd_merge,
                                  int skip_mask, fhevc_motion_rd_pu_node* d_out, fhevc_intra_rd_nxn_node* d_nxn, void* stream);
/* the host form: one picture, host buffers, synchronous; modes its 85 * list_stride bytes per CTU, modes4 its 256 * list_stride4 (or NULL) */
int  fhevc_intra_rd_search(fhevc_ctx* ctx, const int16_t* luma, int stride_samples, int qp, const uint8_t* modes, int list_stride, const uint8_t* modes4,
                           int list_stride4, const fhevc_intra_search_rule* rule, const fhevc_motion_rd_pu_node* fold, const fhevc_motion_rd_node* rd_merge,
                           int skip_mask, fhevc_motion_rd_pu_node* out, fhevc_intra_rd_nxn_node* nxn);
/* fhevc_p_tree_rd_intra_nxn_frame's chain with this stage in the NxN stage's place.  In order: fhevc_p_tree_rd_qt_frame's chain at 3; the first pass of the
 * current picture; its lists through fhevc_intra_first_pass_candidates_device and those of fhevc_intra_first_pass_4x4_device, both at 8 candidates;
 * fhevc_intra_rd_search_device under rule (NULL: the default), folding in place under skip_mask; the RD tree.  It downloads what the NxN frame call
 * downloads.  Rejects what that call rejects, and a bad rule. */
int  fhevc_p_tree_rd_intra_search_frame(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range,
                                        int coarse_range, const fhevc_pu_shape_rule* shape_rule, const fhevc_p_tree_rule* tree_rule,
                                        const fhevc_intra_search_rule* rule, int skip_mask, uint8_t* depth_min, uint8_t* depth_max, fhevc_pu_shape_node* shapes,
                                        fhevc_motion_merge_node* merge, fhevc_motion_rd_node* rd_merge, fhevc_motion_rd_pu_node* rd_pu, fhevc_node_cost* first,
                                        fhevc_intra_rd_nxn_node* nxn);

/* ---- config 4 (P slices): intra candidate costs per CU node (k_intra_p.hip) -----------------------------------------------------------------------
 * HM checks intra at every CU of a P slice (TEncCu.cpp:797-816): xCheckRDCostIntra(SIZE_2Nx2N) at every depth, SIZE_NxN at the 8x8 level, both only while
 * the best mode so far has a non-zero CBF.  Without that candidate a node whose content is not in the reference picture -- uncovered background, the second
 * of two transparent motions, a new object -- has only a huge inter cost, and the tree can only split.  The expensive half exists: the two first passes
 * deliver the best of the 35 modes per node and per 4x4 PU under sqrt(lambda), the square-root lambda every motion stage prices its bits with, so intra
 * first-pass cost and refined inter cost stand on one footing, SATD + sqrt(lambda) * bits.  This stage turns those records into the integer record form the
 * tree reads.
 *   Input per CTU: the 85 fhevc_node_cost records of fhevc_intra_first_pass_device and, optionally, the 256 of fhevc_intra_first_pass_4x4_device (NULL: no
 * NxN candidate), for the pictures that are P pictures, compact over the band; num_pictures counts as in fhevc_pu_shape_select_device.  Of a record only
 * satd and the low byte of mode are read -- the double `cost` never --, and any content of the input bytes is legal.
 *   MARK = 0xFFFFFFFF, SAT = 0xFFFFFFFE.  bits(m) = 2 for mode 0, 3 for modes 1 and 26, 6 for every other byte value: the first pass's own model.
 * c[b] = (uint32_t)((motion_lambda * b) / 65536.0) for b in {2, 3, 6} with motion_lambda = 65536 sqrt(lambda(qp)): getCost(b) in the arithmetic of the
 * motion stages, computed on the host, by value with the launch.  A first-pass record is PRICED iff satd != MARK; its price is min(satd + c[bits(mode)], SAT),
 * the sum in 64 bits.
 *   Node k of level 0..2: a marker record unless the node is INSIDE (the tree's geometry class) and its record is priced; otherwise satd_best = satd,
 * cost_best = the price, part = 0, modes[0..3] = mode.
 *   Node of level 3 (a marker unless INSIDE): the 2Nx2N candidate as above.  The NxN candidate exists iff the 4x4 array is given and all four PUs of the
 * 8x8 CU at (x, y) are priced: (2x, 2y), (2x + 1, 2y), (2x, 2y + 1), (2x + 1, 2y + 1) of the 16x16 unit raster.  Its cost is the 64-bit sum of the four
 * prices saturated at SAT, its satd the saturated sum of the four satds.  NxN replaces 2Nx2N iff its cost is STRICTLY smaller (HM tries 2Nx2N first and
 * xCheckBestMode keeps the earlier mode on a tie) or 2Nx2N is unavailable; then part = 1 and modes[i] = the four PU modes in that order.
 *   Stated departures: the bits of the skip flag, the pred-mode flag and the part mode are left out, as every other stage leaves out its mode bits.  The
 * price is the INTEGER price of the first pass's winner; the first pass chose that winner under its double cost, so a mode whose integer price is smaller by
 * the truncation of c[] can exist and is not looked for.
 *   Field order (pinned: 16 bytes without padding; cost_best is dword 1, as in every record the tree reads): */
typedef struct {
  uint32_t satd_best;       /* the SATD of the candidate taken (NxN: the saturated sum of four) */
  uint32_t cost_best;       /* its price */
  uint8_t  modes[4];        /* part 0: the node's mode four times; part 1: the modes of the four PUs */
  uint8_t  part;            /* 0 = 2Nx2N, 1 = NxN */
  uint8_t  pad[3];          /* written 0 */
} fhevc_intra_p_node;       /* 16 bytes; a marker record: satd_best = cost_best = 0xFFFFFFFF, modes = 255 four times, part = 0, pad = 0 */
/* Device form: d_first: num_pictures * band CTUs * 85 records, d_first4: ... * 256 or NULL, d_out: ... * 85 records, all compact over the band.  The output
 * is written over exactly its extent, an empty band writes nothing.  One wave per CTU, four per workgroup, grid-stride, no LDS: lane i is 8x8 node 21 + i
 * and loads its record and its four PU records, lanes 0..20 load the upper nodes; which address a lane reads depends on lane and node numbers only.  All
 * arrays may sit on any 4-byte alignment: inputs are read as 8-byte pairs where both are 8-byte aligned, records leave as 16-byte stores where d_out is
 * 16-byte aligned, as dwords otherwise; the bytes are the same.  Asynchronous with respect to the host, allocates nothing, keeps NO state in HBM between
 * calls: calls with different QPs may be in flight on two streams, and the first passes and this stage may follow each other on one stream without a host
 * synchronisation.  FHEVC_E_INVALID with a fhevc_last_error text (nothing is launched or written): a null context, d_first or d_out, a pointer that is not
 * 4-byte aligned, num_pictures < 1, a bad band, qp outside 0..51.  Timed under slot 27 of fhevc_kernel_timing.
 * NOT covered: reconstructed neighbours (the first passes predict from the source picture), the RD search behind HM's candidate list (one winner per
 * block, no residual coding), chroma, PCM.  The encoder hook does not consume this output. */
int  fhevc_intra_p_device(fhevc_ctx* ctx, int num_pictures, int ctu_row_begin, int ctu_row_end, int qp, const fhevc_node_cost* d_first,
                          const fhevc_node_cost* d_first4 /* or NULL */, fhevc_intra_p_node* d_out, void* stream);
/* one picture, host arrays over the whole picture (numCtus * 85 / 256 / 85), synchronous */
int  fhevc_intra_p(fhevc_ctx* ctx, int qp, const fhevc_node_cost* first, const fhevc_node_cost* first4 /* or NULL */, fhevc_intra_p_node* out);
/* The host twin: the same definition in plain C++ for one picture of width x height and the band [ctu_row_begin, ctu_row_end); arrays compact over the band.
 * Needs no context and no device.  FHEVC_E_INVALID (nothing written): what the device form rejects, width or height below 8. */
int  fhevc_intra_p_picture(int width, int height, int ctu_row_begin, int ctu_row_end, int qp, const fhevc_node_cost* first,
                           const fhevc_node_cost* first4 /* or NULL */, fhevc_intra_p_node* out);

/* The tree decision that takes the intra candidate: fhevc_p_tree_select_skip[_device] with one more argument, the CTU's 85 fhevc_intra_p_node records (never
 * NULL; on the device compact over the band like d_shapes; any 4-byte alignment; only cost_best is read).  TWO changed rules.
 *   Rule 1, the calm gate: for an INSIDE node of ANY level 0..3 let inter = the smaller of selection and merge cost, as before.  The node is CALM iff the
 * merge cost is strictly smaller (bit 6) and skip.flags & skip_mask != 0: HM's "best mode has no coded residual", under which intra is not tried
 * (TEncCu.cpp:799-804).  On levels 0..2 calm is exactly the EarlyCU condition above and behaves as there.
 *   Rule 2, intra as own cost: if the node is not calm and intra.cost_best < inter (strict; a marker never wins), own[k] = intra.cost_best and bit 0 of
 * byte 14 of the tree record (pad[0], a zero byte in every other tree) is set; byte 15 stays 0.  Bit 6 keeps its meaning.
 *   Everything else is the existing definition: kids, tree, the margins, the maps, CROSSING and ABSENT.  With every intra cost 0xFFFFFFFF the output is byte
 * for byte fhevc_p_tree_select_skip[_device]'s.  The device form is a further instantiation of k_p_tree.hip (one more dword load per lane and round for the
 * intra cost, one more byte load for the leaves' skip flags), timed under slot 17.  The host form needs no context.  FHEVC_E_INVALID: what
 * fhevc_p_tree_select_skip[_device] rejects, a null intra pointer; the device form also rejects a record pointer (d_shapes, d_merge, d_skip, d_intra, d_tree)
 * that is not 4-byte aligned. */
int  fhevc_p_tree_select_intra(const fhevc_pu_shape_node* shapes /* 85 */, const fhevc_motion_merge_node* merge /* 85 */,
                               const fhevc_motion_skip_node* skip /* 85 */, int skip_mask, const fhevc_intra_p_node* intra /* 85 */, int valid_w, int valid_h,
                               const fhevc_p_tree_rule* rule, uint8_t* depth_min /* 256 or NULL */, uint8_t* depth_max /* 256 or NULL */,
                               fhevc_p_tree_node* tree /* 85 or NULL */);
int  fhevc_p_tree_select_intra_device(fhevc_ctx* ctx, const fhevc_pu_shape_node* d_shapes, const fhevc_motion_merge_node* d_merge,
                                      const fhevc_motion_skip_node* d_skip, int skip_mask, const fhevc_intra_p_node* d_intra, int num_pictures,
                                      int ctu_row_begin, int ctu_row_end, const fhevc_p_tree_rule* rule, uint8_t* d_depth_min, uint8_t* d_depth_max,
                                      fhevc_p_tree_node* d_tree, void* stream);
/* The frame chain with everything: fhevc_p_tree_amvp_frame's arguments, checks and both chains (zero-centred; coarse_range 1..14), plus skip_mask (0..3) and
 * an optional download of the intra records.  One pair from host buffers on the context's stream: search, refinement, re-pricing, merge per node and per PU,
 * merge-aware selection, the zero-residual stage on the node merge records, the two intra first passes of the CURRENT picture, the intra stage, and
 * fhevc_p_tree_select_intra_device.  Every buffer is one of the context's staging buffers, allocated by the first call that needs it.  A rejected call
 * moves nothing. */
int  fhevc_p_tree_intra_frame(fhevc_ctx* ctx, const int16_t* cur_luma, const int16_t* ref_luma, int stride_samples, int qp, int search_range, int coarse_range,
                              const fhevc_pu_shape_rule* shape_rule, const fhevc_p_tree_rule* tree_rule, int skip_mask, uint8_t* depth_min /* numCtus * 256 */,
                              uint8_t* depth_max /* numCtus * 256 */, fhevc_pu_shape_node* shapes /* numCtus * 85 or NULL */,
                              fhevc_motion_merge_node* merge /* numCtus * 85 or NULL */, fhevc_intra_p_node* intra /* numCtus * 85 or NULL */);

/* CTU-row band of rank `rank` out of `world`: rows [begin, end) */
int  fhevc_band(int ctu_rows, int rank, int world, int* begin, int* end);

/* average duration in ms of the dominant kernels over launches since the last reset, measured with HIP
 * events on the launch stream; which: 0 = depth CNN, 1 = source Hadamard, 2 = first pass, 3 = pre-analysis, 4 = motion search,
 * 5 = P-picture depth ranges (fhevc_p_depth_range_device), 6 = first pass of the 4x4 PUs (fhevc_intra_first_pass_4x4*),
 * 7 = quarter-sample motion refinement (fhevc_motion_refine*), 8 = motion search of the rectangular PUs (fhevc_motion_search_pu*),
 * 9 = motion search of the PUs with a 4-sample side (fhevc_motion_search_pu_small*), 10 = quarter-sample refinement of the PUs
 * (fhevc_motion_refine_pu*), 11 = the searches at HM's SearchRange (fhevc_motion_search_pu_wide*: one launch for nodes and PUs, one for the
 * small PUs, each counted), 12 = the refinements at HM's SearchRange (fhevc_motion_refine_pu_wide*: one launch for the nodes, one for the PUs,
 * each counted), 13 = the partition-size selection (fhevc_pu_shape_select_device), 15 = the coarse motion centres (fhevc_motion_centres*), the searches around them
 * (fhevc_motion_search_pu_centred*) and their refinements (fhevc_motion_refine_pu_centred*), each launch counted; 14 is not a slot and is rejected like any number above 15
 * -- except 17 = the P-picture tree decision (fhevc_p_tree_select_device, fhevc_p_tree_select_merge_device), added later.  16 is not a slot either: it stays rejected
 * -- and 19 = the merge-candidate costs (fhevc_motion_merge*), added later still.  18 is not a slot: it stays rejected -- and 21 = the merge-candidate
 * costs per PU (fhevc_motion_merge_pu*).  20 is not a slot: it stays rejected -- and 23 = the zero-residual test (fhevc_motion_skip*).  22 is not a slot: it stays
 * rejected -- and 25 = the re-pricing against neighbour predictors (fhevc_motion_amvp*).  24 is not a slot: it stays rejected, as does any number above 25
 * -- except 27 = the intra candidate costs of P pictures (fhevc_intra_p*).  26 is not a slot: it stays rejected, as does any number above 27
 * -- except 29 = the RD estimate (fhevc_motion_rd*).  28 is not a slot: it stays rejected, as does any number above 29.
 * -- except 31 = the RD estimate under a partition size (fhevc_motion_rd_pu*).  30 is not a slot: it stays rejected, as does any number above 31.
 * -- except 33 = the RD estimate of the intra candidate (fhevc_intra_rd*).  32 is not a slot: it stays rejected, as does any number above 33.
 * -- except 35 = the RD estimates at three TU depths (fhevc_motion_rd_qt*, fhevc_motion_rd_pu_qt* with tu_depths 3).  34 is not a slot: it stays rejected,
 * as does any number above 35
 * -- except 37 = the RD estimate of the intra candidate at three TU depths (fhevc_intra_rd_qt* with tu_depths 3).  36 is not a slot: it stays rejected,
 * as does any number above 37
 * -- except 39 = the RD estimate of the intra candidate with the NxN candidate (fhevc_intra_rd_nxn* with d_first4; without it the launch is slot 37's).
 * 38 is not a slot: it stays rejected, as does any number above 39.
 * -- except 41 = the RD estimate of the intra candidate searched over the first pass's candidate lists (fhevc_intra_rd_search*).
 * 40 is not a slot: it stays rejected, as does any number above 41.
 * The tree that stops at a skip (fhevc_p_tree_select_skip_device), the tree that takes the intra candidate (fhevc_p_tree_select_intra_device) and the tree
 * on RD costs (fhevc_p_tree_select_rd_device) are timed under 17 */
int  fhevc_kernel_timing(fhevc_ctx* ctx, int which, int reset, double* avg_ms, uint64_t* launches);
int  fhevc_enable_kernel_timing(fhevc_ctx* ctx, int on);

/* Arithmetic of the depth classifier's conv2 / conv3 (both forms deliver the same integers, bit for bit):
 *   FHEVC_CNN_ARITH_I8  (default): v_mfma_i32_32x32x32_i8 on activations kept as signed bytes, three workgroups per CU;
 *   FHEVC_CNN_ARITH_F16          : 16-bit MFMAs (f16 activations), two workgroups per CU.
 * The environment variable FHEVC_CNN_ARITH=i8|f16 sets the initial value at fhevc_create; a change takes effect at the next launch. */
#define FHEVC_CNN_ARITH_I8   8
#define FHEVC_CNN_ARITH_F16 16
int  fhevc_set_cnn_arith(fhevc_ctx* ctx, int arith);
int  fhevc_get_cnn_arith(const fhevc_ctx* ctx);   /* FHEVC_CNN_ARITH_*, or a negative status */

int  fhevc_get_stats(fhevc_ctx* ctx, void* out, size_t size); /* copies min(size, sizeof(fhevc_stats)) */
const char* fhevc_last_error(fhevc_ctx* ctx);
const char* fhevc_version(void);

#ifdef __cplusplus
}
#endif
#endif
