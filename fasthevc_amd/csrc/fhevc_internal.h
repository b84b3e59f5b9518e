// fhevc_internal.h -- shared declarations between the C-ABI layer (fhevc_api.hip, fhevc_weights.hip, fhevc_host.hip) and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include <cstddef>

#define FHEVC_CTU 64

// ---- depth CNN (k_cnn.hip) -------------------------------------------------------------------------------
// Packed weight image in HBM, built once by fhevc_set_weights (fhevc_weights.hip: build_weight_image):
//   frag  : MFMA A-operand fragments, one uint4 (8 bf16) per lane: conv1 [2][64], conv2 [9][64], conv3 [2][18][64], all scaled
//           by their layer's 2^-shift
//   bias  : float b1[16], b2[32], b3[64]
//   whead : int8: wh64[2][4096], wh32[2][4096], wh16[2][1024]
//   bhead : int32 bh64[2], bh32[2], bh16[2], qp_bias[3][52]
#define FHEVC_FRAG_CONV1 0
#define FHEVC_FRAG_CONV2 128
#define FHEVC_FRAG_CONV3 (128 + 9 * 64)
#define FHEVC_FRAG_HAD (128 + 9 * 64 + 2 * 18 * 64)  // the source Hadamard's constant A operands (k_cnn.hip, HAD == 2): [M tile 2][K step 5][64]
#define FHEVC_FRAG_TOTAL (FHEVC_FRAG_HAD + 2 * 5 * 64)
// conv3 of the 16-bit form: 0 = v_mfma_f32_16x16x32_f16 (M tiles of 16 channels, one output row per chain), 1 = v_mfma_f32_32x32x16_f16
// (the wave's 32 channels x two output rows 8 apart per MFMA, K step = one tap x 16 channels).  The fragment image differs:
// kernel and build_weight_image read this switch
#ifndef FHEVC_F16_CONV3_32
#define FHEVC_F16_CONV3_32 0  // measured equal (0.5624 against 0.5659 ms on one box, parity green): the 16x16x32 form stays
#endif
// the i8 variant's fragments (one uint4 = 16 signed bytes per lane): conv2 [2 row pairs][3 columns of taps][64], conv3 [2 tiles][9 taps][64]
#define FHEVC_STAMP_SLOTS 11   // per workgroup of the stamped diagnostic kernel: 8 phase sums, the CTU loop's s_memtime and s_memrealtime spans, the workgroup's slot on its CU
#define FHEVC_FRAGI8_CONV2 0
#define FHEVC_FRAGI8_CONV3 (6 * 64)
#define FHEVC_FRAGI8_TOTAL (6 * 64 + 2 * 9 * 64)

// Tuning / test switches read from the environment ONCE, at fhevc_create (fhevc_read_knobs), and kept in the context: nothing on a launch path
// calls getenv.  None of them changes results; FHEVC_CNN_ARITH / FHEVC_CNN_REQUANT / FHEVC_HADAMARD_FORM / FHEVC_FUSE_HADAMARD
// select between forms that the parity suite runs side by side.
struct FhevcKnobs {
  int wg_per_cu = 0;            // FHEVC_CNN_WG_PER_CU=1..4: workgroups per CU of the depth kernel's persistent grid (0: the form's own)
  int debug_wg_per_cu = 0;      // FHEVC_DEBUG_WG_PER_CU=1..4: the same for the stamped diagnostic build only
  bool requant_general = false; // FHEVC_CNN_REQUANT=general: the i8 form's general requant instead of the short forms
  bool requant_short = false;   // FHEVC_CNN_REQUANT=short: the short forms 1 / 2 also where the blob qualifies for the high-byte forms (tests, A/B)
  bool family_layers = false;   // FHEVC_FAMILY_LAYERS: a member with a fused kernel runs layer by layer all the same (tests)
  bool trio = false;            // FHEVC_CNN_TRIO=1: the i8 depth kernel as ONE 768-thread workgroup per CU, three groups one barrier interval apart (k_cnn.hip, TRIO)
  bool d2_requant_general = false; // FHEVC_D2_REQUANT=general: the fused two-convolution kernel's general requant instantiation whatever the blob allows (tests, A/B)
  bool fused_d2 = true;         // FHEVC_FUSED_D2=0: the two-convolutions-per-block members run layer by layer instead of through k_cnn_d2.inc (tests, A/B)
  bool layers_no_fuse = false;  // FHEVC_LAYERS_NO_FUSE: the layer path without the first convolution fused into the second (tests)
  bool layers_no_dbuf = false;  // FHEVC_LAYERS_NO_DBUF: the layer path's single-buffered staging (tests)
  size_t layers_lds_limit = 80 * 1024;  // FHEVC_LAYERS_LDS_KB (experiments)
  int layers_grid = 2048;       // FHEVC_LAYERS_GRID (experiments)
  bool refine_pu_stage_full = false; // FHEVC_REFINE_PU_STAGE=full: the MR = 64 layout of k_motion_refine_pu.hip stages its whole window whatever max_range is (tests, A/B)
  bool pu_wide_generic = false; // FHEVC_PU_WIDE=generic: fhevc_motion_search_pu_wide sends 8-bit int16 planes down the generic MR = 64 kernels instead of k_motion_pu_wide.hip (tests, A/B)
};
FhevcKnobs fhevc_read_knobs();

struct FhevcFrames {
  const void* luma;          // device pointer to sample (0,0) of frame 0
  int sample_bytes;          // 1 or 2
  int stride;                // samples
  long long frame_stride;    // samples
  int width, height, bit_depth;
  int ctus_x, ctus_y;
  int num_frames;
  int row_begin, row_end;    // CTU-row band processed by this launch
  int qp;                    // slice QP (0..51): selects the per-QP prior of the classifier heads
};

struct FhevcCnnWeights {
  const uint4* frag;
  const float* bias;
  const uint8_t* whead;
  const int32_t* bhead;      // bh64[2], bh32[2], bh16[2], then qp_bias[3][52]
  float scale[3];            // 2^-shift per conv layer (folded into the fragments; the kernel pre-scales the biases with it)
  // the i8 variant of conv2 / conv3 (v_mfma_i32_32x32x32_i8 on activations a - 128): unscaled int8 fragments, int32 biases
  // (+ 128 * the sum of the filter's weights; entries 16.. of bias_i8, laid out like bias) and the requant shifts
  const uint4* frag_i8;
  const int32_t* bias_i8;
  int shift[3];
  int requant_mode[3];       // per layer: 0 general, 1 shift <= 7 (packed 16-bit shift), 2 shift == 8 and |accumulator| < 2^23 (byte gather),
                             // 3 high byte of the saturated 16-bit value (conv2 at shift 7, conv3 at shift 8; bias_i8 then carries - (128 << shift) as well)
  int i8;                    // 1: run that variant
  int had_valu;              // 1: the fused source Hadamard on packed 16-bit VALU also for 8-bit content (default; FHEVC_HADAMARD_FORM=mfma: 0)
};

// a member of the reference's Bayesian-optimisation network family with one convolution per block (k_cnn_family.inc; FHW3 blob)
struct FhevcFamilyWeights {
  int c[3];                  // channel widths (multiples of 16 / 32 / 32)
  const uint4* frag1;        // conv1: [C1 / 16 groups][2 (pre-pool column)][64 lanes], bf16, scaled by 2^-shift1
  const float* bias1;        // conv1 biases, pre-scaled, - 128 * sum of weights
  const uint4* frag2;        // conv2: [M tile][K chunk][tap][64 lanes], 16 signed bytes per lane
  const uint4* frag3;        // conv3: likewise
  const int32_t* bias_i8;    // bias2[C2], bias3[C3], + 128 * sum of weights
  const uint8_t* whead;      // wh64[2][8][8][C3], wh32[2][8][8][C3], wh16[2][4][4][C3]
  const uint8_t* headm;      // MFMA image of wh32 / wh16: [position 16][chunk C3 / 64][column 16][64 B] (columns 0, 1: 16-level; 2 + 2 sub + class: 32-level)
  const int32_t* bhead;      // as FhevcCnnWeights::bhead
  int shift[3];
};
hipError_t fhevc_launch_cnn_family(const FhevcFrames& fr, const FhevcFamilyWeights& w, uint8_t* d_depth, int32_t* d_logits, uint32_t* d_flags,
                                   uint8_t* d_depth_max, int margin_split, int margin_stop, int num_cus, hipStream_t stream);
bool fhevc_cnn_family_supported(int c1, int c2, int c3);

// any member of the family, layer by layer through HBM (k_cnn_layers.inc)
struct FhevcLayer {
  const uint4* frag;     // [M tile][K chunk][tap 9][64 lanes] (first layer: [M tile][64]: K = the nine taps of the one input channel)
  const int32_t* bias;   // [cout_pad], + 128 * sum of the filter's weights (not for the first layer: its input is centred samples)
  int8_t* out;           // [chunk CTUs][Ho + 2] rows of ([Ho + 2][cout_pad] + out_pad bytes)
  int shift, kc, cout_pad, H, pool;   // kc = Cin_pad / 32 (0: first layer); H = input size (64 / 32 / 16)
  int rq;                             // the shortest requant form the layer's weights allow (k_cnn_layers.inc: layer_store16): 1 = shift <= 7, 2 = shift 8 and |accumulator| < 2^23, else 0
  int in_pad, out_pad, swz;           // bytes added to the row pitch of the input / output tensor; XOR mask of the LDS image (fhevc_layer_lds_image)
};
// the row-pitch padding and XOR mask that make the layer kernel's LDS reads conflict-free for an input of kc x 32 channels at H x H (tools/lds_swizzle_search.py)
void fhevc_layer_lds_image(int kc, int pool, int H, int* pad, int* mask);
struct FhevcLayersWeights {
  int num_layers, chunk, c3, c3_pad;
  int d2_short;            // the fused two-convolution kernel may run its short-requant instantiation (l[0].rq == 1, l[1..5].rq == 2; FHEVC_D2_REQUANT=general: never)
  FhevcLayer l[9];
  int8_t* in0;             // [chunk CTUs][66][66]
  const uint8_t* whead;    // wh64[2][8][8][c3_pad], wh32[2][8][8][c3_pad], wh16[2][4][4][c3_pad] (zeros behind the c3 weights)
  const int32_t* bhead;    // as FhevcCnnWeights::bhead
};

hipError_t fhevc_launch_cnn_layers(const FhevcFrames& fr, const FhevcLayersWeights& w, uint8_t* d_depth, int32_t* d_logits, uint32_t* d_flags,
                                   uint8_t* d_depth_max, int margin_split, int margin_stop, int num_cus, const FhevcKnobs& knobs, hipStream_t stream);

// the same members with two convolutions per block and padded widths 32 / 64 / 96 (23 / 46 / 92 x 2) as one LDS-resident kernel (k_cnn_d2.inc)
bool fhevc_cnn_d2_supported(const FhevcLayersWeights& w);
hipError_t fhevc_launch_cnn_d2(const FhevcFrames& fr, const FhevcLayersWeights& w, uint8_t* d_depth, int32_t* d_logits, uint32_t* d_flags,
                               uint8_t* d_depth_max, int margin_split, int margin_stop, int num_cus, hipStream_t stream);

hipError_t fhevc_cnn_prepare_device();  // LDS opt-in of the depth kernel on the current device (once per context)
// d_depth_max / margins: soft decisions (nullptr / 0, 0 = the plain map only)
// d_had != nullptr: the per-CTU source Hadamard is computed inside the depth kernel from the samples it loads anyway (one
// pass over the frame); allowed only where fhevc_cnn_can_fuse_hadamard(fr), otherwise use fhevc_launch_src_hadamard
bool fhevc_cnn_can_fuse_hadamard(const FhevcFrames& fr);
hipError_t fhevc_launch_cnn(const FhevcFrames& fr, const FhevcCnnWeights& w, uint8_t* d_depth, int32_t* d_had, int32_t* d_logits,
                            uint32_t* d_flags, uint8_t* d_depth_max, int margin_split, int margin_stop, int num_cus, const FhevcKnobs& knobs, hipStream_t stream);
hipError_t fhevc_launch_expand_flags(const FhevcFrames& fr, const uint32_t* d_flags, uint8_t* d_depth, hipStream_t stream);

hipError_t fhevc_launch_cnn_stamped(const FhevcFrames& fr, const FhevcCnnWeights& w, uint8_t* d_depth, int32_t* d_had /* null: without the fused Hadamard */, int num_cus, const FhevcKnobs& knobs,
                                    unsigned long long* d_stamps, int* grid_out, hipStream_t stream);

// ---- source Hadamard + SATD (k_hadamard.hip) ---------------------------------------------------------------
hipError_t fhevc_launch_src_hadamard(const FhevcFrames& fr, int32_t* d_out, hipStream_t stream);
hipError_t fhevc_launch_satd(const int16_t* d_org, int org_stride, const int16_t* d_cur, int cur_stride,
                             int w, int h, int bit_depth, uint32_t* d_out, hipStream_t stream);

// ---- 35-mode first pass (k_firstpass.hip) ------------------------------------------------------------------
struct FhevcNodeCost { uint32_t satd; uint32_t mode; double cost; };
// d_all (optional): every (node, mode) pair, [CTU][85][35] -- the parity output behind fhevc_intra_first_pass_all
// d_modes (optional): the candidate lists, [CTU][85][num_modes], selected inside the kernel (no table in HBM); d_out may then be null
hipError_t fhevc_launch_first_pass(const FhevcFrames& fr, double sqrt_lambda, FhevcNodeCost* d_out, FhevcNodeCost* d_all, hipStream_t stream,
                                   uint8_t* d_modes = nullptr, int num_modes = 0);

// the K (<= 8) cheapest modes per node out of d_all, best first (candidate lists of fhevc_intra_first_pass_candidates)
hipError_t fhevc_launch_first_pass_topk(const FhevcNodeCost* d_all, long long nodes, int k, uint8_t* d_modes, hipStream_t stream);

// ---- 35-mode first pass of the 256 4x4 PUs of a CTU (k_firstpass4.hip) ---------------------------------------
// d_best [CTU][256], d_modes [CTU][256][num_modes] (1..8), d_all [CTU][256][35]: each may be null; PUs in raster 16x16 order
hipError_t fhevc_launch_first_pass4(const FhevcFrames& fr, double sqrt_lambda, int num_modes, FhevcNodeCost* d_best, uint8_t* d_modes, FhevcNodeCost* d_all,
                                    hipStream_t stream);

// ---- source-only motion search per CU node (k_motion.hip; config 4) -----------------------------------------
#define FHEVC_NODES 85
#define FHEVC_MOTION_MAX_RANGE 8
struct FhevcMotionNode { uint32_t satd_zero, satd_best, cost_best; int16_t mvx, mvy; };
struct FhevcMvCost { uint32_t c[(2 * FHEVC_MOTION_MAX_RANGE + 1) * (2 * FHEVC_MOTION_MAX_RANGE + 1)]; };  // [dy + R][dx + R] of the window in use
// frames 1 .. num_frames-1 of fr, each searched in the frame before it; d_out: (num_frames - 1) * band CTUs * 85 nodes
// sad: SAD (HM's integer-search distortion, pinned to the reference's xPatternSearch) instead of Hadamard SATD
hipError_t fhevc_launch_motion(const FhevcFrames& fr, int range, const FhevcMvCost& mvc, FhevcMotionNode* d_out, int num_cus, bool sad, hipStream_t stream);

// the same search in its SAD mode over a window of up to +-64 (HM's SearchRange), 8-bit content (k_motion_wide.hip); d_mvtab: (2 range + 1)^2
// vector costs in raster order, in HBM
#define FHEVC_MOTION_WIDE_MAX_RANGE 64
hipError_t fhevc_launch_motion_wide(const FhevcFrames& fr, int range, const uint32_t* d_mvtab, FhevcMotionNode* d_out, int num_cus, hipStream_t stream);
// ... and for content ABOVE 8 bit (16-bit planes; round 4): fhevc_motion_kernel itself laid out for the +-64 window (k_motion.hip), the same d_mvtab
hipError_t fhevc_launch_motion_big(const FhevcFrames& fr, int range, const uint32_t* d_mvtab, FhevcMotionNode* d_out, int num_cus, hipStream_t stream);

// ---- the same search for the rectangular PUs of the 64x64, 32x32 and 16x16 nodes (k_motion_pu.hip; config 4) ------
#define FHEVC_PUS 124   // FHEVC_PUS_PER_CTU of fasthevc.h: 5 nodes x 6 shapes x 2 parts + 16 nodes x 2 shapes x 2 parts
// fr, range (1 .. FHEVC_MOTION_MAX_RANGE), mvc, sad as fhevc_launch_motion; d_pus: (num_frames - 1) * band CTUs * 124 entries in the order of
// fhevc_motion_pu_index; d_nodes (may be null): the 85 nodes of fhevc_launch_motion for the same arguments, byte for byte
hipError_t fhevc_launch_motion_pu(const FhevcFrames& fr, int range, const FhevcMvCost& mvc, FhevcMotionNode* d_nodes, FhevcMotionNode* d_pus, int num_cus, bool sad,
                                  hipStream_t stream);

// ---- ... and for the PUs with a 4-sample side: AMP of the 16x16 nodes, 8x4 / 4x8 of the 8x8 nodes (k_motion_pu_small.hip; config 4) ------
#define FHEVC_PUS_SMALL 384   // FHEVC_PUS_SMALL_PER_CTU of fasthevc.h: 16 nodes x 4 shapes x 2 parts + 64 nodes x 2 shapes x 2 parts
// fr, range (1 .. FHEVC_MOTION_MAX_RANGE), mvc, sad as fhevc_launch_motion; d_pus: (num_frames - 1) * band CTUs * 384 entries in the order of
// fhevc_motion_pu_small_index
hipError_t fhevc_launch_motion_pu_small(const FhevcFrames& fr, int range, const FhevcMvCost& mvc, FhevcMotionNode* d_pus, int num_cus, bool sad, hipStream_t stream);

// getCost(bits) for every number of bits two exp-Golomb components of a quarter-sample vector up to +-(4 * 64 + 3) can take (at most 38), tabulated by
// the host with HM's doubles; travels by value as a kernel argument, so every launch has its own lambda
#define FHEVC_MV_BIT_COSTS 40
struct FhevcMvBitCost { uint32_t c[FHEVC_MV_BIT_COSTS]; };
// the exp-Golomb bits of a WHOLE-sample vector component v at iCostScale 2 (TComRdCost.h:166-174, xGetComponentBits of v << 2): 2 floor(log2 t) + 1 with
// t = v <= 0 ? (-v << 3) + 1 : v << 3; at most 19 for +-64.  The cost of a whole-sample vector with a zero predictor is c[bits(dx) + bits(dy)]: the searches
// at HM's SearchRange need no table of (2 R + 1)^2 vector costs
__host__ __device__ inline int fhevc_mv_component_bits(int v)
{
  const unsigned t = v <= 0 ? ((unsigned)(-v) << 3) + 1u : (unsigned)v << 3;
  return 2 * (31 - __builtin_clz(t)) + 1;
}

// ---- the three searches at HM's own SearchRange, SAD, any bit depth (the MR = 64 layouts of k_motion_pu.hip and k_motion_pu_small.hip; behind
// fhevc_motion_search_pu_wide).  range 1 .. FHEVC_MOTION_WIDE_MAX_RANGE; cost: the bit costs of the launch's QP, by value -- no table in HBM, nothing kept
// between calls.  d_nodes / d_pus: as fhevc_launch_motion_pu, either may be null (not both); d_pus of the small form as fhevc_launch_motion_pu_small ----
hipError_t fhevc_launch_motion_pu_big(const FhevcFrames& fr, int range, const FhevcMvBitCost& cost, FhevcMotionNode* d_nodes, FhevcMotionNode* d_pus, int num_cus,
                                      hipStream_t stream);
hipError_t fhevc_launch_motion_pu_small_big(const FhevcFrames& fr, int range, const FhevcMvBitCost& cost, FhevcMotionNode* d_pus, int num_cus, hipStream_t stream);
// ... and for 8-bit content on byte SADs (k_motion_pu_wide.hip, the layout of k_motion_wide.hip): range 3 .. 64; any of the three outputs may be null (not all);
// one launch, instantiated for the families asked for
hipError_t fhevc_launch_motion_pu_wide(const FhevcFrames& fr, int range, const FhevcMvBitCost& cost, FhevcMotionNode* d_nodes, FhevcMotionNode* d_pus, FhevcMotionNode* d_pus_small,
                                       int num_cus, hipStream_t stream);

// ---- one coarse motion centre per CTU from the 4:1 decimated picture pair (k_motion_coarse.hip; config 4) --------------------------
// fr as fhevc_launch_motion; coarse_range 1 .. FHEVC_MOTION_COARSE_MAX_RANGE in decimated cells (vector components of up to +-56 samples); cost: the bit
// costs of the launch's QP, by value; d_centres: (num_frames - 1) * band CTUs entries, compact over the band
#define FHEVC_MOTION_COARSE_MAX_RANGE 14
#define FHEVC_MOTION_CENTRE_MAX 56   // the largest centre component the centred search and refinement take: 56 + 8 stays within HM's SearchRange 64
hipError_t fhevc_launch_motion_coarse(const FhevcFrames& fr, int coarse_range, const FhevcMvBitCost& cost, FhevcMotionNode* d_centres, int num_cus, hipStream_t stream);

// ---- the integer searches around one centre per CTU (the MR = 8 layouts of k_motion_pu.hip and k_motion_pu_small.hip with a per-CTU window origin; behind
// fhevc_motion_search_pu_centred).  SAD; range 1 .. FHEVC_MOTION_MAX_RANGE; mvc: the window's table, which prices the vector RELATIVE to the centre;
// d_centres: (num_frames - 1) * band CTUs entries of which mvx / mvy are read (4-byte aligned); a component outside +-FHEVC_MOTION_CENTRE_MAX marks the CTU's entries.
// d_nodes / d_pus: either may be null (not both); records hold absolute vectors and, as satd_zero, the SAD at the centre ----
hipError_t fhevc_launch_motion_pu_centred(const FhevcFrames& fr, int range, const FhevcMvCost& mvc, const FhevcMotionNode* d_centres, FhevcMotionNode* d_nodes,
                                          FhevcMotionNode* d_pus, int num_cus, hipStream_t stream);
hipError_t fhevc_launch_motion_pu_small_centred(const FhevcFrames& fr, int range, const FhevcMvCost& mvc, const FhevcMotionNode* d_centres, FhevcMotionNode* d_pus, int num_cus,
                                                hipStream_t stream);

// ---- quarter-sample refinement of the search's vectors (k_motion_refine.hip; config 4) --------------------------
struct FhevcMotionQpelNode { uint32_t satd_int, satd_best, cost_best; int16_t mvx, mvy; };
// fr as fhevc_launch_motion; d_nodes: what it wrote for the same frames and band (only mvx / mvy are read; |component| > max_range: the marker);
// d_out: (num_frames - 1) * band CTUs * 85
hipError_t fhevc_launch_motion_refine(const FhevcFrames& fr, int max_range, const FhevcMvBitCost& cost, const FhevcMotionNode* d_nodes, FhevcMotionQpelNode* d_out,
                                      int num_cus, hipStream_t stream);

// ---- merge-candidate costs per CU node from the refined nodes of the same level (k_motion_merge.hip; config 4) --------------------------
struct FhevcMotionMergeNode { uint32_t satd_best, cost_best; int16_t mvx, mvy; uint8_t idx, num, src, pad; };
// fr, max_range (1 .. FHEVC_MOTION_WIDE_MAX_RANGE), cost as fhevc_launch_motion_refine; d_refined: (num_frames - 1) * band CTUs * 85 refined nodes of which
// cost_best, mvx and mvy are read; d_out: as many records
hipError_t fhevc_launch_motion_merge(const FhevcFrames& fr, int max_range, const FhevcMvBitCost& cost, const FhevcMotionQpelNode* d_refined, FhevcMotionMergeNode* d_out,
                                     int num_cus, hipStream_t stream);

// ... per PU (k_motion_merge_pu.hip): the same input; d_out_pus: ... * 124 records in the order of fhevc_motion_pu_index, d_out_small: ... * 384 in the order of
// fhevc_motion_pu_small_index; either may be null, not both
hipError_t fhevc_launch_motion_merge_pu(const FhevcFrames& fr, int max_range, const FhevcMvBitCost& cost, const FhevcMotionQpelNode* d_refined,
                                        FhevcMotionMergeNode* d_out_pus, FhevcMotionMergeNode* d_out_small, int num_cus, hipStream_t stream);

// ---- refined costs re-priced against neighbour predictors (k_motion_amvp.hip; config 4) --------------------------
// getCost(bits) for every number of bits two exp-Golomb components of a DIFFERENCE of two int16 vectors can take: at most 2 * 33; travels by value
#define FHEVC_MVP_BIT_COSTS 67
struct FhevcMvpBitCost { uint32_t c[FHEVC_MVP_BIT_COSTS]; };
// motion_lambda: 65536 * sqrt(lambda) of the slice QP, the number mv_bit_cost_table (fhevc_motion_api.hip) builds FhevcMvBitCost from
inline FhevcMvpBitCost fhevc_mvp_bit_cost_table(double motion_lambda)
{
  FhevcMvpBitCost t;
  for (int b = 0; b < FHEVC_MVP_BIT_COSTS; ++b) t.c[b] = (uint32_t)((motion_lambda * (unsigned)b) / 65536.0);
  return t;
}
struct FhevcMotionMvp { int16_t px, py; uint8_t idx, num_spatial, src, bits; };
static_assert(sizeof(FhevcMotionMvp) == 8, "predictor record: 8 bytes without padding");
// xGetExpGolombNumberOfBits at cost scale 0 of a vector difference v (|v| <= 65535): 2 floor(log2 t) + 1, t = v <= 0 ? (-v << 1) + 1 : v << 1; at most 33
__host__ __device__ inline int fhevc_mvd_bits(int v)
{
  const unsigned t = v <= 0 ? ((unsigned)(-v) << 1) + 1u : (unsigned)v << 1;
  return 2 * (31 - __builtin_clz(t)) + 1;
}
// List and choice of fhevc_motion_amvp* (include/fasthevc.h), shared by the kernel and the host twin.  The candidates at L, A, AR, BL, AL: whether each is
// available, and its vector (as dword 3 of a record: mvx in the low half); q: the entry's own vector, packed alike.  a = the first available of (BL, L),
// b = of (AR, A, AL); b is dropped if it equals a; (0, 0) fills the list up to two; the first index of least bits wins.  Ten scalars, no arrays: a select
// between two elements of an array handed over by address becomes an indexed load, and the array then leaves the registers
struct FhevcMvpChoice { uint32_t pred; int idx, num_spatial, src, bits; };
__host__ __device__ inline FhevcMvpChoice fhevc_mvp_choose(bool av_l, bool av_a, bool av_ar, bool av_bl, bool av_al, uint32_t v_l, uint32_t v_a, uint32_t v_ar, uint32_t v_bl,
                                                           uint32_t v_al, uint32_t q)
{
  const bool has_a = av_bl || av_l;
  bool has_b = av_ar || av_a || av_al;
  const uint32_t va = av_bl ? v_bl : v_l, vb = av_ar ? v_ar : (av_a ? v_a : v_al);
  const int sa = av_bl ? 3 : 0, sb = av_ar ? 2 : (av_a ? 1 : 4);
  if (has_a && has_b && va == vb) has_b = false;
  const uint32_t p0 = has_a ? va : (has_b ? vb : 0u), p1 = has_a && has_b ? vb : 0u;
  const int s0 = has_a ? sa : (has_b ? sb : 5), s1 = has_a && has_b ? sb : 5;
  const int qx = (int16_t)(q & 0xFFFFu), qy = (int16_t)(q >> 16);
  const int b0 = fhevc_mvd_bits(qx - (int16_t)(p0 & 0xFFFFu)) + fhevc_mvd_bits(qy - (int16_t)(p0 >> 16));
  const int b1 = fhevc_mvd_bits(qx - (int16_t)(p1 & 0xFFFFu)) + fhevc_mvd_bits(qy - (int16_t)(p1 >> 16));
  FhevcMvpChoice c;
  c.idx = b1 < b0 ? 1 : 0;
  c.pred = c.idx ? p1 : p0; c.src = c.idx ? s1 : s0; c.bits = c.idx ? b1 : b0;
  c.num_spatial = (has_a ? 1 : 0) + (has_b ? 1 : 0);
  return c;
}
// fr: geometry, band, num_frames = the picture pairs of the batch (luma is not read).  d_nodes (never null) / d_pus / d_pus_small: num_frames * band CTUs * 85 /
// 124 / 384 refined entries; d_out_*: as many records, d_mvp_*: as many predictor records; each output may be null (not all six), all compact over the band
hipError_t fhevc_launch_motion_amvp(const FhevcFrames& fr, const FhevcMvpBitCost& cost, const FhevcMotionQpelNode* d_nodes, const FhevcMotionQpelNode* d_pus,
                                    const FhevcMotionQpelNode* d_pus_small, FhevcMotionQpelNode* d_out_nodes, FhevcMotionQpelNode* d_out_pus,
                                    FhevcMotionQpelNode* d_out_small, FhevcMotionMvp* d_mvp_nodes, FhevcMotionMvp* d_mvp_pus, FhevcMotionMvp* d_mvp_small, int num_cus,
                                    hipStream_t stream);

// ---- the zero-residual (skip) test per CU node at its merge vector (k_motion_skip.hip; config 4) --------------------------
struct FhevcMotionSkipNode { uint32_t coef_max, level_sum; uint16_t nonzero; uint8_t flags, pad; int16_t mvx, mvy; };
static_assert(sizeof(FhevcMotionSkipNode) == 16, "skip record: 16 bytes without padding");
// HM's scalar quantiser per TU size 8, 16, 32 (index log2 N - 3), computed on the host: level = (|c| * scale + add) >> qbits
struct FhevcSkipQuant { uint32_t scale, qbits[3], add_plain[3], add_half[3]; };
inline FhevcSkipQuant fhevc_skip_quant(int qp, int bit_depth)
{
  static const uint32_t scales[6] = { 26214, 23302, 20560, 18396, 16384, 14564 };   // g_quantScales
  const int qpp = qp + 6 * (bit_depth - 8);
  FhevcSkipQuant q;
  q.scale = scales[qpp % 6];
  for (int i = 0; i < 3; ++i) {
    q.qbits[i] = (uint32_t)(14 + qpp / 6 + (15 - bit_depth - (i + 3)));   // 16 .. 26
    q.add_plain[i] = 85u << (q.qbits[i] - 9);                              // the P-slice dead zone
    q.add_half[i] = 1u << (q.qbits[i] - 1);                                // the rounding RDOQ starts from
  }
  return q;
}
// fr, max_range as fhevc_launch_motion_merge; d_merge: (num_frames - 1) * band CTUs * 85 merge records of which cost_best, mvx and mvy are read; d_out: as many
hipError_t fhevc_launch_motion_skip(const FhevcFrames& fr, int max_range, const FhevcSkipQuant& q, const FhevcMotionMergeNode* d_merge, FhevcMotionSkipNode* d_out,
                                    int num_cus, hipStream_t stream);

// ---- the RD estimate per CU node at a vector: transform, quantiser, rebuilt block, one TU split (k_motion_rd.hip; config 4) --------------------------
// dist / cost_rd / flags lie where the merge and selection records keep cost_best (dword 1) and the skip record keeps flags (byte 10)
struct FhevcMotionRdNode { uint32_t dist, cost_rd; uint16_t bits; uint8_t flags, tu_split; int16_t mvx, mvy; };
static_assert(sizeof(FhevcMotionRdNode) == 16, "RD record: 16 bytes without padding");
// lam_q8 = floor(lambda * 256 + 0.5), lambda = 0.57 * 2^((qp - 12) / 3)
inline uint32_t fhevc_rd_lambda_q8(int qp) { return (uint32_t)std::floor(0.57 * std::pow(2.0, (qp - 12) / 3.0) * 256.0 + 0.5); }
// HM's quantiser and dequantiser without scaling lists per TU size 4, 8, 16, 32 (index log2 N - 2), computed on the host:
// level = (|c| * scale + add) >> qbits; c^ = (level * inv_scale + inv_add) >> inv_shift, where inv_scale holds the left shift of a negative rightShift
struct FhevcRdQuant { uint32_t scale, lam_q8, qbits[4], add_plain[4], add_half[4], inv_scale[4], inv_add[4], inv_shift[4]; };
inline FhevcRdQuant fhevc_rd_quant(int qp, int bit_depth)
{
  static const uint32_t scales[6] = { 26214, 23302, 20560, 18396, 16384, 14564 };   // g_quantScales
  static const uint32_t inv_scales[6] = { 40, 45, 51, 57, 64, 72 };                 // g_invQuantScales
  const int qpp = qp + 6 * (bit_depth - 8);
  FhevcRdQuant q;
  q.scale = scales[qpp % 6];
  q.lam_q8 = fhevc_rd_lambda_q8(qp);
  for (int i = 0; i < 4; ++i) {
    q.qbits[i] = (uint32_t)(14 + qpp / 6 + (15 - bit_depth - (i + 2)));     // 16 .. 27
    q.add_plain[i] = 85u << (q.qbits[i] - 9);
    q.add_half[i] = 1u << (q.qbits[i] - 1);
    const int right = 6 - (15 - bit_depth - (i + 2) + qpp / 6);              // xDeQuant's rightShift = log2 N - 1 - qp / 6: -7 .. 4
    q.inv_scale[i] = inv_scales[qpp % 6] << (right < 0 ? -right : 0);
    q.inv_add[i] = right > 0 ? 1u << (right - 1) : 0u;
    q.inv_shift[i] = (uint32_t)(right > 0 ? right : 0);
  }
  return q;
}
// fr, max_range as fhevc_launch_motion_skip; source 0: d_in are merge records, 1: refined (or re-priced) nodes, d_mvp (may be null) their predictor records;
// d_in, d_out: (num_frames - 1) * band CTUs * 85 records
hipError_t fhevc_launch_motion_rd(const FhevcFrames& fr, int max_range, const FhevcRdQuant& q, int source, const void* d_in, const FhevcMotionMvp* d_mvp,
                                  FhevcMotionRdNode* d_out, int num_cus, hipStream_t stream, int tu_depths = 2);

// ... of a node under any of HM's seven inter partition sizes, the prediction composed from its two parts' vectors (the PU instances of k_motion_rd.hip):
// bytes 0..11 as FhevcMotionRdNode, so the tree kernels read cost_rd and flags where they always do
struct FhevcMotionRdPuNode { uint32_t dist, cost_rd; uint16_t bits; uint8_t flags, tu_split; uint8_t part, merged, pad[2]; };
static_assert(sizeof(FhevcMotionRdPuNode) == 16 && offsetof(FhevcMotionRdPuNode, cost_rd) == 4 && offsetof(FhevcMotionRdPuNode, flags) == 10 &&
              offsetof(FhevcMotionRdPuNode, part) == 12, "RD record of a partition size: 16 bytes, dword 1 and byte 10 where the tree kernels read");
// the kernels' view of fhevc_motion_rd_pu_inputs (the same ten pointers)
struct FhevcPuShapeNode;
struct FhevcMotionRdPuInputs {
  const FhevcMotionQpelNode *nodes, *pus, *pus_small;
  const FhevcMotionMergeNode *merge_pus, *merge_pus_small;
  const FhevcMotionMvp *mvp_nodes, *mvp_pus, *mvp_pus_small;
  const FhevcPuShapeNode* shapes;
  const FhevcMotionRdPuNode* fold;
};
// part_mode 0, 1, 2, 4..7: that PartSize for every node; 8 / 9: the selection's best / second; I.fold == d_out is allowed
// tu_depths (both launchers): 2 -- the instances there always were; 3 -- the instances with HM's third TU size for the 32x32 and 16x16 nodes (tu_split bits 4..7)
hipError_t fhevc_launch_motion_rd_pu(const FhevcFrames& fr, int max_range, const FhevcRdQuant& q, int part_mode, const FhevcMotionRdPuInputs& I, FhevcMotionRdPuNode* d_out,
                                     int num_cus, hipStream_t stream, int tu_depths = 2);

// workgroups of an MR = 64 instance of the RD kernel that the device keeps on one CU (hipOccupancyMaxActiveBlocksPerMultiprocessor; measurement tools)
hipError_t fhevc_motion_rd_big_residency(int sample_bytes, bool pu, int tu_depths, int* per_cu);

// ... and of the intra candidate (the intra instances of k_motion_rd.hip): ONE mode per node, the first pass's, predicted per TU from the first pass's own
// lines; the record is a FhevcMotionRdPuNode with part kRdPartIntra and the mode in pad[0].  fr: num_frames pictures, no pairing; d_first: num_frames * band
// CTUs * 85 first-pass records of which satd and the low byte of mode are read; d_fold (an earlier launch's records; d_fold == d_out is allowed) and
// d_rd_merge (the merge records' RD records, for the calm gate under skip_mask 0..3) may be null
// tu_depths: 2 -- the instances there always were; 3 -- the instances with HM's full intra TU tree: the third TU size of the 32x32 and 16x16 nodes, the
// depth 1 of the 8x8 nodes, the DST of every 4x4 TU (tu_split bits 4..7)
constexpr int kRdPartIntra = 16;   // FHEVC_RD_PART_INTRA
hipError_t fhevc_launch_intra_rd(const FhevcFrames& fr, const FhevcRdQuant& q, const FhevcNodeCost* d_first, const FhevcMotionRdPuNode* d_fold,
                                 const FhevcMotionRdNode* d_rd_merge, int skip_mask, FhevcMotionRdPuNode* d_out, int num_cus, hipStream_t stream, int tu_depths = 2);
// ... at three depths with the NxN candidate of the 8x8 nodes (two further intra instances): d_first4 the 256 records per CTU of the 4x4 first pass, of which
// satd and the low byte of mode are read; the node's record is the NxN record (part kRdPartIntraNxN) where that is valid and strictly cheaper than 2Nx2N or
// that one is invalid.  d_nxn (may be null): the plain candidate of every 8x8 node, 64 records per CTU.  d_first4 null: fhevc_launch_intra_rd's launch at 3
constexpr int kRdPartIntraNxN = 17;   // FHEVC_RD_PART_INTRA_NXN
struct FhevcIntraRdNxN { uint32_t dist, cost_rd; uint16_t bits; uint8_t flags, cbf; uint8_t modes[4]; };
hipError_t fhevc_launch_intra_rd_nxn(const FhevcFrames& fr, const FhevcRdQuant& q, const FhevcNodeCost* d_first, const FhevcNodeCost* d_first4, const FhevcMotionRdPuNode* d_fold,
                                     const FhevcMotionRdNode* d_rd_merge, int skip_mask, FhevcMotionRdPuNode* d_out, FhevcIntraRdNxN* d_nxn, int num_cus, hipStream_t stream);
// ... with the mode searched over the first pass's lists (two further intra instances): d_modes the 85 entries of list_stride bytes per CTU, d_modes4 (may be
// null: no NxN candidate, and d_nxn null) the 256 entries of list_stride4; the rule travels by value.  Step A over a node's list, best and second on the full
// TU tree, the 4x4 PUs each on its own list.  ONE launch; counts within 1..stride or nothing is launched
struct FhevcIntraSearchRule { uint8_t count[4], count4, append_planar, pad[2]; };
hipError_t fhevc_launch_intra_rd_search(const FhevcFrames& fr, const FhevcRdQuant& q, const uint8_t* d_modes, int list_stride, const uint8_t* d_modes4, int list_stride4,
                                        const FhevcIntraSearchRule& rule, const FhevcMotionRdPuNode* d_fold, const FhevcMotionRdNode* d_rd_merge, int skip_mask,
                                        FhevcMotionRdPuNode* d_out, FhevcIntraRdNxN* d_nxn, int num_cus, hipStream_t stream);

// ---- ... and of the PUs' vectors (k_motion_refine_pu.hip; config 4) --------------------------------------------------
// fr, max_range (1 .. FHEVC_MOTION_WIDE_MAX_RANGE: up to FHEVC_MOTION_MAX_RANGE the MR = 8 layout, above it the MR = 64 layout with its window in dynamic LDS),
// cost as fhevc_launch_motion_refine; d_pus / d_out_pus: (num_frames - 1) * band CTUs * 124 entries in the order of fhevc_motion_pu_index, d_pus_small /
// d_out_small: ... * 384 in the order of fhevc_motion_pu_small_index; either pair may be null together.  stage_full: the MR = 64 layout stages its whole
// window instead of the part max_range reaches (FhevcKnobs::refine_pu_stage_full; the bytes are the same)
hipError_t fhevc_launch_motion_refine_pu(const FhevcFrames& fr, int max_range, const FhevcMvBitCost& cost, const FhevcMotionNode* d_pus, FhevcMotionQpelNode* d_out_pus,
                                         const FhevcMotionNode* d_pus_small, FhevcMotionQpelNode* d_out_small, int num_cus, bool stage_full, hipStream_t stream);
// workgroups of its MR = 64 instance that the device keeps on one CU (hipOccupancyMaxActiveBlocksPerMultiprocessor), for the form that planes of
// sample_bytes at bit_depth take: the launcher sizes the persistent grid by it, at most two
hipError_t fhevc_motion_refine_pu_big_residency(int sample_bytes, int bit_depth, int* per_cu);

// ---- the two refinements around one centre per CTU (the MR = 8 layouts with the window staged around the centre; behind fhevc_motion_refine_pu_centred).
// max_range 1 .. FHEVC_MOTION_MAX_RANGE; d_centres as fhevc_launch_motion_pu_centred; an entry is valid iff its node is inside, the centre in range and
// |mv - centre| <= max_range; the vector cost of a candidate q is that of q - 4 centre ----
hipError_t fhevc_launch_motion_refine_centred(const FhevcFrames& fr, int max_range, const FhevcMvBitCost& cost, const FhevcMotionNode* d_centres, const FhevcMotionNode* d_nodes,
                                              FhevcMotionQpelNode* d_out, int num_cus, hipStream_t stream);
hipError_t fhevc_launch_motion_refine_pu_centred(const FhevcFrames& fr, int max_range, const FhevcMvBitCost& cost, const FhevcMotionNode* d_centres, const FhevcMotionNode* d_pus,
                                                 FhevcMotionQpelNode* d_out_pus, const FhevcMotionNode* d_pus_small, FhevcMotionQpelNode* d_out_small, int num_cus, hipStream_t stream);

// the shipped P-picture rule (fhevc_p_rule_default): see fasthevc.h; regenerate with tests/quality/fit_p_rule.py
#define FHEVC_P_RULE_WEIGHTS { { 3101, 188, -94, 80, 1149, 1149, 3174, -138, 15748, -351620 }, \
                               { 594, 101, 375, -8, 1078, 1078, -197, 436, 3462, 256745 },      \
                               { 317, -3, 366, -216, 745, 745, 0, 1344, 2780, -18423 } }
// thresholds (Q18) picked on the 1080p pan clip (tests/quality/eval_p.py, profiles/r02_p_slice_motion_rule.json): no split is
// ever FORCED (a wrongly forced split costs several percent of rate on P pictures), splits are FORBIDDEN below scores of
// -3 / -1 / -0.5, and the range stays within +-1 of the co-located depth
#define FHEVC_P_RULE_T_SPLIT { 25952256, 25952256, 25952256 }
#define FHEVC_P_RULE_T_STOP  { 786432, 262144, 131072 }
#define FHEVC_P_RULE_WINDOW  1

// the rule for the wide search (fhevc_p_rule_default_wide): fitted on SAD-mode features of the +-64 search with the reference picture's depths taken
// at the motion-compensated position (tests/quality/p_features_gpu.py on the MI355X, fit_p_rule.py; 176 clips with motion of 0 .. 48 samples per picture)
#define FHEVC_P_RULE_WIDE_WEIGHTS { { 6048, -127, -5256, 95, 876, 1134, 2120, 630, 1548, -447236 }, \
                                    { 1152, -30, -842, -103, 866, 1285, 415, -455, -48, 19539 },     \
                                    { 255, 36, -3, 16, 643, 1206, 0, -243, -177, 342124 } }

// ---- P-picture depth ranges on the device (k_p_rule.hip; config 4) --------------------------------------------
// fhevc_p_rule of fasthevc.h; travels by value as a kernel argument, so every launch has its own rule
struct FhevcPRule { int32_t w[3][10]; int32_t t_split[3], t_stop[3]; int32_t window; };
// fr: geometry, band, num_frames = the P pictures of the batch, qp (luma is not read).  d_nodes: num_frames * band CTUs * 85 as fhevc_launch_motion* writes
// them; d_prev_maps: num_frames whole-picture depth maps; prev_mode: FHEVC_P_PREV_*; d_depth_min / d_depth_max (may be null): compact over the band
hipError_t fhevc_launch_p_rule(const FhevcFrames& fr, int prev_mode, const FhevcPRule& rule, const FhevcMotionNode* d_nodes, const uint8_t* d_prev_maps,
                               uint8_t* d_depth_min, uint8_t* d_depth_max, int num_cus, hipStream_t stream);

// ---- partition sizes per CU from the refined PU costs (k_pu_shape.hip; config 4) ------------------------------------
// fhevc_pu_shape_rule of fasthevc.h; travels by value as a kernel argument, so every launch has its own rule
struct FhevcPuShapeRule { int32_t margin_q8[4]; int32_t margin_abs[4]; int32_t amp_mode; };
// what is wrong with a rule (host form and device form reject the same rules); null: nothing
template <class R> inline const char* fhevc_pu_shape_rule_error(const R& r)
{
  for (int l = 0; l < 4; ++l) {
    if (r.margin_q8[l] < 0 || r.margin_q8[l] > 65535) return "margin_q8 out of range (0..65535)";
    if (r.margin_abs[l] < 0) return "margin_abs out of range (>= 0)";
  }
  return r.amp_mode < 0 || r.amp_mode > 1 ? "amp_mode out of range (0..1)" : nullptr;
}
struct FhevcPuShapeNode { uint32_t cost_2Nx2N, cost_best, cost_second; uint8_t best, second, mask, avail; };
// fr: geometry, band, num_frames = the P pictures of the batch (luma is not read).  d_nodes / d_pus / d_pus_small (may be null): num_frames * band CTUs * 85 / 124 /
// 384 refined entries; d_shapes: num_frames * band CTUs * 85; d_costs (may be null): ... * 85 * 8 dwords; all compact over the band
hipError_t fhevc_launch_pu_shape(const FhevcFrames& fr, const FhevcPuShapeRule& rule, const FhevcMotionQpelNode* d_nodes, const FhevcMotionQpelNode* d_pus,
                                 const FhevcMotionQpelNode* d_pus_small, FhevcPuShapeNode* d_shapes, uint32_t* d_costs, int num_cus, hipStream_t stream);
// ... with the merge records of fhevc_launch_motion_merge_pu beside the refined PUs (d_merge_pus never null; d_merge_small may be null: all markers): a part
// costs the smaller of the two; d_merged (may be null): ... * 85 uint16_t, bit 2p + part set iff that part's merge cost is strictly the smaller one
hipError_t fhevc_launch_pu_shape_merge(const FhevcFrames& fr, const FhevcPuShapeRule& rule, const FhevcMotionQpelNode* d_nodes, const FhevcMotionQpelNode* d_pus,
                                       const FhevcMotionQpelNode* d_pus_small, const FhevcMotionMergeNode* d_merge_pus, const FhevcMotionMergeNode* d_merge_small,
                                       FhevcPuShapeNode* d_shapes, uint32_t* d_costs, uint16_t* d_merged, int num_cus, hipStream_t stream);

// ---- P-picture depth ranges from the selection's records, bottom-up over the quad-tree (k_p_tree.hip; config 4) ------------------------------------
// fhevc_p_tree_rule of fasthevc.h; travels by value as a kernel argument, so every launch has its own rule
struct FhevcPTreeRule { int32_t split_q8[3], split_abs[3], stop_q8[3], stop_abs[3], split_cost[3]; };
// what is wrong with a rule (host form and device form reject the same rules); null: nothing
template <class R> inline const char* fhevc_p_tree_rule_error(const R& r)
{
  for (int l = 0; l < 3; ++l) {
    if (r.split_q8[l] < 0 || r.split_q8[l] > 65535) return "split_q8 out of range (0..65535)";
    if (r.stop_q8[l] < 0 || r.stop_q8[l] > 65535) return "stop_q8 out of range (0..65535)";
    if (r.split_abs[l] < 0) return "split_abs out of range (>= 0)";
    if (r.stop_abs[l] < 0) return "stop_abs out of range (>= 0)";
    if (r.split_cost[l] < 0) return "split_cost out of range (>= 0)";
  }
  return nullptr;
}
struct FhevcPTreeNode { uint32_t cost_own, cost_kids, cost_tree; uint8_t flags, level, pad[2]; };
// fr: geometry, band, num_frames = the P pictures of the batch (luma is not read).  d_shapes: num_frames * band CTUs * 85 records as fhevc_launch_pu_shape writes
// them; d_depth_min / d_depth_max: ... * 256 bytes; d_tree: ... * 85 records; each output may be null (not all three); all compact over the band
hipError_t fhevc_launch_p_tree(const FhevcFrames& fr, const FhevcPTreeRule& rule, const FhevcPuShapeNode* d_shapes, uint8_t* d_depth_min, uint8_t* d_depth_max,
                               FhevcPTreeNode* d_tree, int num_cus, hipStream_t stream);
// ... with the merge records of fhevc_launch_motion_merge beside the selection's (never null): a node's own cost is the smaller of the two, and bit 6 of the
// record's flags says that the merge cost is the one taken
hipError_t fhevc_launch_p_tree_merge(const FhevcFrames& fr, const FhevcPTreeRule& rule, const FhevcPuShapeNode* d_shapes, const FhevcMotionMergeNode* d_merge,
                                     uint8_t* d_depth_min, uint8_t* d_depth_max, FhevcPTreeNode* d_tree, int num_cus, hipStream_t stream);
// ... and with the skip records of fhevc_launch_motion_skip (never null; only flags, byte 10, is read): an INSIDE node of level 0..2 whose own cost is the
// merge cost and whose flags carry a bit of skip_mask (0..3) is not descended -- tree = own, stop_sure, bit 7
hipError_t fhevc_launch_p_tree_skip(const FhevcFrames& fr, const FhevcPTreeRule& rule, const FhevcPuShapeNode* d_shapes, const FhevcMotionMergeNode* d_merge,
                                    const FhevcMotionSkipNode* d_skip, int skip_mask, uint8_t* d_depth_min, uint8_t* d_depth_max, FhevcPTreeNode* d_tree, int num_cus,
                                    hipStream_t stream);

// ---- intra candidate costs per CU node for P pictures, from the first passes' records (k_intra_p.hip; config 4) ------------------------------------
struct FhevcIntraPNode { uint32_t satd_best, cost_best; uint8_t modes[4]; uint8_t part; uint8_t pad[3]; };
static_assert(sizeof(FhevcIntraPNode) == 16, "intra record: 16 bytes without padding");
// getCost(b) of the first pass's three mode-bit counts (k_firstpass.hip: 2 for planar, 3 for DC and vertical, 6 otherwise) at the slice QP's motion lambda,
// computed on the host with the arithmetic of mv_bits_cost; travels by value
struct FhevcIntraBitCost { uint32_t c2, c3, c6; };
inline FhevcIntraBitCost fhevc_intra_bit_cost(double motion_lambda)
{
  return { (uint32_t)((motion_lambda * 2u) / 65536.0), (uint32_t)((motion_lambda * 3u) / 65536.0), (uint32_t)((motion_lambda * 6u) / 65536.0) };
}
// The price of a first-pass record, shared by the kernel and the host twin: mode = the low byte of the record's mode dword; the caller has tested
// satd != 0xFFFFFFFF.  64-bit sum, saturated at 0xFFFFFFFE
__host__ __device__ inline uint32_t fhevc_intra_p_price(uint32_t satd, uint32_t mode, const FhevcIntraBitCost& c)
{
  const uint64_t p = (uint64_t)satd + (mode == 0u ? c.c2 : (mode == 1u || mode == 26u ? c.c3 : c.c6));
  return p > 0xFFFFFFFEull ? 0xFFFFFFFEu : (uint32_t)p;
}
// fr: geometry, band, num_frames = the P pictures of the batch (luma is not read).  d_first: num_frames * band CTUs * 85 first-pass records as dwords (4 per
// record; dwords 0 and 1 are read); d_first4 (may be null: no NxN candidate): ... * 256 records alike; d_out: ... * 85 records; all compact over the band
hipError_t fhevc_launch_intra_p(const FhevcFrames& fr, const FhevcIntraBitCost& cost, const uint32_t* d_first, const uint32_t* d_first4, FhevcIntraPNode* d_out,
                                int num_cus, hipStream_t stream);
// ... and the tree that takes them (k_p_tree.hip): fhevc_launch_p_tree_skip with the intra records (never null; only cost_best, dword 1, is read).  A node that
// is not calm (merged with a masked zero bit) and whose intra cost is strictly below its inter cost takes the intra cost as its own: bit 0 of byte 14
hipError_t fhevc_launch_p_tree_intra(const FhevcFrames& fr, const FhevcPTreeRule& rule, const FhevcPuShapeNode* d_shapes, const FhevcMotionMergeNode* d_merge,
                                     const FhevcMotionSkipNode* d_skip, int skip_mask, const FhevcIntraPNode* d_intra, uint8_t* d_depth_min, uint8_t* d_depth_max,
                                     FhevcPTreeNode* d_tree, int num_cus, hipStream_t stream);

// ---- adaptive-QP pre-analysis (k_preanalyze.hip) -----------------------------------------------------------
// d_activity: per frame parts_per_frame doubles, layers concatenated (layer d: ceil(H/P) x ceil(W/P), P = 64 >> d)
hipError_t fhevc_launch_preanalyze(const FhevcFrames& fr, int layers, long long parts_per_frame, double* d_activity,
                                   int num_cus, hipStream_t stream);
