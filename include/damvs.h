/* damvs.h — C ABI of the MI355X cascade-MVS cost-volume engine (libdamvs.so).
 *
 * Drop-in boundary for the per-stage hot path of wsmtht520/DAMVSNet. The reference has no
 * native/FFI layer; its boundary is the Python module API, which the
 * package damvsnet_amd mirrors on top of this ABI. Each entry point names the reference
 * interface it replaces (paths relative to the reference repo).
 *
 * Conventions
 *   - Plain C types only. Tensor arguments are DEVICE pointers owned by the caller; parameter
 *     structs passed to damvs_stage_create are HOST pointers (copied, BN-folded, packed).
 *   - No allocation, no host synchronisation inside the *_forward / kernel entry points: work is
 *     enqueued on `stream` (a hipStream_t, NULL = default stream) and is graph-capturable.
 *   - Return 0 (DAMVS_OK) or a negative DAMVS_E_* code; damvs_last_error_string() gives the
 *     message of the last failure on the calling thread.
 *   - A damvs_stage is immutable after create and may be used concurrently from several threads
 *     on different streams (workspaces must differ).
 *   - Layouts: features NHWC [B][h][w][C]; cost volume NDHWC [B][D][h][w][C]; hypotheses,
 *     logits and probabilities [B][D][h][w] float; projections [B][N][2][4][4] float with
 *     [..,0,:,:] the world->camera extrinsic and [..,1,:3,:3] the stage intrinsics
 *     (datasets/general_eval.py:158-175).
 */
#ifndef DAMVS_H
#define DAMVS_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DAMVS_ABI_VERSION 1

enum {
  DAMVS_OK = 0,
  DAMVS_E_ARG = -1,       /* null pointer / bad enum */
  DAMVS_E_SHAPE = -2,     /* unsupported or inconsistent shape */
  DAMVS_E_DTYPE = -3,     /* unsupported storage type */
  DAMVS_E_HIP = -4,       /* HIP runtime error */
  DAMVS_E_NOMEM = -5,     /* device allocation failed (create only) */
  DAMVS_E_WORKSPACE = -6, /* workspace too small; a full voxel table (damvs_cloud_thin_status) */
  DAMVS_E_RANGE = -7      /* non-finite depth / confidence / variance (damvs_stage_status); a point outside the voxel
                             grid (damvs_cloud_thin_status) */
};

enum { DAMVS_F32 = 0, DAMVS_BF16 = 1 };                       /* storage of features / volumes */
enum { DAMVS_AGG_ADAPTIVE = 0, DAMVS_AGG_VARIANCE = 1 };      /* models/cas_mvsnet.py:11-16 */

/* BatchNorm in eval form: y = (x - running_mean) / sqrt(running_var + eps) * weight + bias. */
typedef struct {
  const float* weight;
  const float* bias;
  const float* running_mean;
  const float* running_var;
  float eps;
} damvs_bn;

/* CostRegNet (models/module.py:510-541). conv_weight[i] for i = 0..9 is
 * conv0..conv6 (Conv3d, [Cout][Cin][3][3][3]) then conv7, conv9, conv11
 * (ConvTranspose3d, [Cin][Cout][3][3][3]); bn[i] the matching BatchNorm3d;
 * prob_weight is prob.weight [1][base][3][3][3] (no bias, no BN). */
typedef struct {
  int in_channels;
  int base_channels;
  const float* conv_weight[10];
  damvs_bn bn[10];
  const float* prob_weight;
} damvs_costreg_params;

/* AggWeightNetVolume (models/module.py:544-563): w_net.0 = Conv3d(C,1,1)+BN+ReLU (w1 is [C]),
 * w_net.1 = Conv3d(1,1,1)+BN+ReLU (w2 is [1]). conv0 is unused by the reference forward. */
typedef struct {
  int in_channels;
  const float* w1;
  damvs_bn bn1;
  const float* w2;
  damvs_bn bn2;
} damvs_aggweight_params;

typedef struct damvs_stage damvs_stage;

int damvs_abi_version(void);
const char* damvs_last_error_string(void);
/* Provenance: sha256 (hex, first 16 digits) of the sources, headers and compiler flags this library was built
 * from (damvsnet_amd/build.py), "unstamped" for builds outside build.py. The Python binding compares it with the
 * sources next to it and refuses a stale library. */
const char* damvs_build_id(void);

/* One cascade stage's weights (replaces DepthNet.weight_net[s] + cost_regularization[s],
 * models/cas_mvsnet.py:16,180-182). `aggw` may be NULL for DAMVS_AGG_VARIANCE. Uses the
 * current HIP device. */
int damvs_stage_create(const damvs_costreg_params* costreg, const damvs_aggweight_params* aggw, int agg_mode,
                       int dtype, damvs_stage** out);
int damvs_stage_destroy(damvs_stage* st);

/* Bytes of device workspace damvs_stage_forward needs for this problem size. */
int damvs_stage_workspace_size(const damvs_stage* st, int B, int N, int D, int h, int w, size_t* bytes);

/* DepthNet.forward (models/cas_mvsnet.py:18-134) for one stage: warp + aggregation,
 * CostRegNet, softmax regression, confidence, exp-variance.
 *   feats[N]  : N device pointers (host array), view 0 = reference, each [B][h][w][C] of dtype
 *   proj      : [B][N][2][4][4]      hyps: [B][D][h][w]      prob_init: NULL or [B][D][h][w]
 *   depth, conf, var : [B][h][w]     prob: NULL or [B][D][h][w] (prob_volume output)
 * D, h, w must be multiples of 8 (three stride-2 levels, models/module.py:515-528). */
int damvs_stage_forward(const damvs_stage* st, void* stream, int B, int N, int D, int h, int w,
                        const void* const* feats, const float* proj, const float* hyps, const float* prob_init,
                        void* workspace, size_t workspace_bytes, float* depth, float* conf, float* var,
                        float* prob);

/* Range status of the damvs_stage_forward calls that used `workspace` since the previous damvs_stage_status on it
 * (synchronises `stream`, the stream they ran on, then clears the status): DAMVS_OK, or DAMVS_E_RANGE when any depth,
 * confidence or variance value one of them wrote is non-finite. The status is the workspace's first 4 bytes: zero them
 * when the workspace is allocated (hipMemset), or call damvs_stage_status once before the first forward and ignore the
 * result. Why it exists: the fp32 path computes every conv product on split-f16 MFMAs (x = f16 hi + f16 lo), so an
 * activation of magnitude >= 65520 (beyond the f16 range) turns into NaN there; ReLU keeps NaN as torch.relu does, and
 * the stage's outputs carry it. The forward itself never synchronises (its last kernel checks the three output maps
 * and sets the status); damvsnet_amd asks once per CascadeMVSNet.forward. The reference's fp32 convolutions have no
 * such limit (the volume of models/cas_mvsnet.py:64-76 is the first tensor that can reach it). */
int damvs_stage_status(const damvs_stage* st, void* stream, const void* workspace, size_t workspace_bytes);

/* damvs_stage_forward with in-pipeline timing probes: events (NULL, or 4 hipEvent_t, any may be NULL) are
 * recorded on `stream` before the warp + aggregation launch, after it, after the U-Net and after the
 * regression -- the per-kernel-group durations of the stage as the product runs it (bench.py roofline). */
int damvs_stage_forward_probed(const damvs_stage* st, void* stream, int B, int N, int D, int h, int w,
                               const void* const* feats, const float* proj, const float* hyps, const float* prob_init,
                               void* workspace, size_t workspace_bytes, float* depth, float* conf, float* var,
                               float* prob, void* const* events);

/* ---- split entry points (used by the parity tests and by sharded execution) ---- */

/* Per (b, src view): 3x4 [R|t] of P_src * inv(P_ref) with P = [K E[:3,:4]; E[3]]
 * (models/cas_mvsnet.py:44-47, models/module.py:308-310). rt: [B][N-1][12]. */
int damvs_proj_prepare(void* stream, int B, int N, const float* proj, float* rt);

/* homo_warping(src_fea, src_proj, ref_proj, depth_values) (models/module.py:297-332) for one source
 * view: src [B][h][w][C], rt [B][12] (from damvs_proj_prepare with N = 2), hyps [B][D][h][w],
 * out [B][D][h][w][C]. C in {8, 16, 32}. */
int damvs_homo_warp(void* stream, int dtype, int B, int C, int D, int h, int w, const void* src, const float* rt,
                    const float* hyps, void* out);

/* Feature layouts accepted by damvs_warp_aggregate. */
enum { DAMVS_LAYOUT_NHWC = 0, DAMVS_LAYOUT_CBLOCK = 1 /* [B][C/E][h][w][E], E = 16 bytes of channels */ };

/* Aggregated cost volume (models/cas_mvsnet.py:26-87): volume [B][D][h][w][C]. `layout` gives the
 * feature layout (damvs_stage_forward repacks NHWC to DAMVS_LAYOUT_CBLOCK internally when C spans
 * several 16-byte chunks: each gather instruction then touches half the cache lines). */
int damvs_warp_aggregate(const damvs_stage* st, void* stream, int B, int N, int D, int h, int w,
                         const void* const* feats, int layout, const float* rt, const float* hyps, void* volume);

/* NHWC [B][h][w][C] -> DAMVS_LAYOUT_CBLOCK for N maps (src[v] -> dst[v], device buffers). */
/* 1 if the stage forward gathers C-channel maps of this dtype at N views from channel-blocked copies
 * (damvs_block_channels: pixels wider than 32 bytes that the channel-split warp does not take -- it takes 32 / 64 /
 * 128-byte pixels at odd N >= 3), 0 if it gathers the NHWC maps in place, negative on a bad argument. The split entry
 * point damvs_warp_aggregate takes either layout; callers that mirror damvs_stage_forward ask here.
 * damvs_warp_feat_blocked(dtype, C) is the N = 5 answer (the round-4 entry point, kept for existing callers). */
int damvs_warp_feat_blocked_n(int dtype, int C, int N);
int damvs_warp_feat_blocked(int dtype, int C);
int damvs_block_channels(void* stream, int dtype, int N, int B, int h, int w, int C, const void* const* src,
                         void* const* dst);

/* CostRegNet forward incl. the final prob conv (models/module.py:532-541): logits [B][D][h][w]. */
int damvs_costreg_logits(const damvs_stage* st, void* stream, int B, int D, int h, int w, const void* volume,
                         void* workspace, size_t workspace_bytes, float* logits);

/* ---- pieces of one stage for sharded execution (damvsnet_amd/sharded.py: one depth map over P GPUs) ---- */

/* The aggregated volume of reference rows [y0, y0 + rows) only (models/cas_mvsnet.py:26-87 restricted to
 * those rows; the feature maps stay whole: [B][h][w][C] or channel-blocked per `layout`), read from / written
 * to rows [out_y, out_y + rows) of planes of out_rows rows: hyps [B][D][out_rows][w], volume
 * [B][D][out_rows][w][C] (a haloed H-slab; other rows untouched). Voxels are bitwise those of
 * damvs_warp_aggregate. */
int damvs_warp_aggregate_rows(const damvs_stage* st, void* stream, int B, int N, int D, int h, int w, int y0, int rows,
                              int out_rows, int out_y, const void* const* feats, int layout, const float* rt,
                              const float* hyps, void* volume);

/* One CostRegNet layer (models/module.py:532-540; Conv3d / Deconv3d wrappers :117-202): layer 0..9 =
 * conv0..conv6, conv7, conv9, conv11. D, h, w are the level-0 volume dims (multiples of 8); level l has
 * D>>l, h>>l, w>>l. in: the layer input at its level ([B][Dl][hl][wl][cin]); out: its output. For
 * conv7 / conv9 / conv11, `out` holds the skip tensor (conv4 / conv2 / conv0 output) on entry and
 * relu(deconv(in)) + skip on exit (models/module.py:537-539). Zero padding at every tensor edge. */
int damvs_costreg_layer(const damvs_stage* st, void* stream, int layer, int B, int D, int h, int w, const void* in,
                        void* out);

/* Magnitude slots (fp32 stages). The fp32 path splits each activation x into f16 pieces x * 2^k = hi + lo with k
 * chosen per tensor and batch element from its largest magnitude, so large activations do not overflow the f16 range
 * and small ones keep their lo piece normal (the reference's fp32 convolutions have no range limit:
 * models/cas_mvsnet.py:64-76, models/module.py:510-541), and a sample's result does not depend on the rest of its
 * batch. damvs_stage_forward keeps the slots of its tensors in its workspace. A caller running the U-Net layer by layer
 * (sharded execution) owns them: per tensor B slots of DAMVS_AMAX_SLOT_BYTES of device memory (slot b for batch
 * element b, consecutive), zeroed before use; producers fold max |value| into them (atomically; bit patterns of
 * non-negative floats compare as unsigned integers), consumers read them. Any replica word of a slot may hold the
 * maximum: to set a slot by hand, zero it and write the float's bits (as uint32) into its first word. */
#define DAMVS_AMAX_SLOT_BYTES 4096

/* damvs_costreg_layer with magnitude slots (fp32; bf16 stages ignore them): in_slot = the input tensor's B slots
 * (NULL: unscaled split, exact only while the activations stay inside [2^-3, 65504)), out_slot = the B slots this
 * layer's stored outputs are folded into (NULL: not recorded). damvs_costreg_layer = both NULL. */
int damvs_costreg_layer_scaled(const damvs_stage* st, void* stream, int layer, int B, int D, int h, int w,
                               const void* in, void* out, const void* in_slot, void* out_slot);

/* Fold max |x[i]| of n floats (device) into one magnitude slot (stream-ordered; the slot is not cleared): call it
 * per batch element with that element's slot. */
int damvs_tensor_amax(void* stream, const float* x, long long n, void* slot);

/* The tail of damvs_stage_forward: prob conv (models/module.py:541) + softmax regression, confidence and
 * exp-variance (models/cas_mvsnet.py:105-124) on the U-Net output c0 [B][D][h][w][base].
 * scratch: [B][D][h][w] float (used only when the fused kernels cannot hold a pixel's logits). */
int damvs_stage_regress(const damvs_stage* st, void* stream, int B, int D, int h, int w, const void* c0,
                        const float* hyps, const float* prob_init, float* scratch, float* depth, float* conf, float* var,
                        float* prob);

/* Softmax regression on logits (models/cas_mvsnet.py:105-124). prob_init / prob may be NULL. */
int damvs_regress(void* stream, int B, int D, int h, int w, const float* logits, const float* hyps,
                  const float* prob_init, float* depth, float* conf, float* var, float* prob);

/* Stage hypotheses at stage resolution h = H/scale, w = W/scale (models/cas_mvsnet.py:238-296 with
 * uncertainty_aware_samples, models/module.py:999-1038):
 *   prev_depth == NULL : stage 1, linspace(depth_values[b,0], depth_values[b,Dv-1], D)
 *   otherwise          : uncertainty-aware samples around prev_depth / prev_var ([B][hp][wp]),
 *                        bilinearly upsampled to H x W, then trilinearly resampled to h x w.
 * hyps: [B][D][h][w]. scale must be 1, 2 (refinement) or any value for stage 1. */
int damvs_hypotheses(void* stream, int B, int D, int H, int W, int scale, const float* depth_values, int Dv,
                     const float* prev_depth, const float* prev_var, int hp, int wp, float* hyps);

/* GeoFeatureFusion's sparse depth pyramid (models/geometry.py:90-96, 117-121; SparseDownSampleClose,
 * models/geometry.py:443-455): d0 = (depth - depth_values[b][0]) / (depth_values[b][Dv-1] - depth_values[b][0]),
 * valid mask = mask ? mask : (d0 > 0) ('basic'), then three 2x2 stride-2 closest-valid poolings.
 * depth / mask: [B][h][w] fp32, h, w >= 8; d_l: [B][h >> l][w >> l] (floor sizes, as max_pool2d); scratch: at least
 * B*(h/2)*(w/2) + B*(h/4)*(w/4) floats (the level-1/2 masks). Bitwise equal to the reference's torch ops. */
int damvs_sparse_depth_pyramid(void* stream, int B, int h, int w, const float* depth, const float* depth_values, int Dv,
                               const float* mask, float* d0, float* d1, float* d2, float* d3, float* scratch);

/* ---- 2D front-end convolutions (FeatureNet models/module.py:355-462,
 * GeoFeatureFusion models/geometry.py:14-277). One layer = Conv2d or ConvTranspose2d with BN already
 * folded into weight/bias by the caller, optional ReLU, fused concat of up to two NHWC tensors and up
 * to four fp32 planar inputs (the reference's torch.cat of feature maps and depth planes), and fused
 * residual adds before / after the ReLU. */
typedef struct {
  int transposed;        /* 0: Conv2d weight [cout][cin][k][k]; 1: ConvTranspose2d weight [cin][cout][k][k] */
  int kernel, stride, padding, output_padding;
  int cin, cout;         /* channels of the weight */
  int c0, c0_at;         /* NHWC tensor input 0: channel count, first weight input channel it feeds */
  int c1, c1_at;         /* NHWC tensor input 1 (c1 = 0: none) */
  int ngeo;              /* fp32 planar inputs, each one weight input channel: <= 4 when c0 = c1 = 0
                            (then cout <= 16), else <= 1 (BasicBlockGeo's depth plane) */
  int geo_at[4];
  int relu;
} damvs_conv2d_desc;

typedef struct damvs_conv2d damvs_conv2d;

/* weight / bias: host fp32 (bias may be NULL). c0, c1 must be multiples of 8 (bf16) / 4 (f32);
 * the output is stored with cout rounded up to a multiple of 4 (extra channels are 0 + ReLU).
 * Every operand of a forward call must be smaller than 2 GiB (32-bit device offsets). */
int damvs_conv2d_create(const damvs_conv2d_desc* desc, const float* weight, const float* bias, int dtype,
                        damvs_conv2d** out);
int damvs_conv2d_destroy(damvs_conv2d* layer);
/* Output spatial size for an Hi x Wi input. */
int damvs_conv2d_out_size(const damvs_conv2d* layer, int Hi, int Wi, int* Ho, int* Wo, int* cout_stored);
/* in0/in1: [B][Hi][Wi][c0/c1]; geo[g]: fp32 [Hi][Wi] planes, batch b at geo[g] + b*geo_batch_stride[g];
 * res_pre / res_post: [B][Ho][Wo][cout_stored] (res_post at (Ho/post_up, Wo/post_up), nearest);
 * out: [B][Ho][Wo][cout_stored]. */
int damvs_conv2d_forward(const damvs_conv2d* layer, void* stream, int B, int Hi, int Wi, const void* in0,
                         const void* in1, const float* const* geo, const long long* geo_batch_stride, const void* res_pre,
                         const void* res_post, int post_up, void* out);

/* ---- introspection ---- */
/* The kernel damvs_conv2d_forward would launch for this layer at this size under the current
 * switch settings, as the demangled kernel name without namespace and argument list, e.g.
 * "conv2d_mfma_kernel<float, 4, true, false, true>", followed by " grid=(x,y)". No device work.
 * The answer is the forward's for 16-byte aligned planes one image (Hi * Wi floats) apart, as the front-end passes
 * them: the plane-only layers' vector kernels ask for aligned planes and fall back to the one-column kernel otherwise.
 * DAMVS_E_ARG: null layer or buffer, or a buffer too small for the answer; DAMVS_E_SHAPE: no kernel takes the layer at
 * this size (the forward fails too). */
int damvs_conv2d_route(const damvs_conv2d* layer, int B, int Hi, int Wi, char* buf, size_t n);

/* Border fix-up for a 3x3 padding-1 conv whose bias held the full 9-tap sum of a per-tap constant
 * (a bias that reached the 3x3 conv through a 1x1 conv, FeatureNet's inner2 -> out3,
 * models/module.py:455-459): at every border pixel of out [B][H][W][cout_stored] subtract
 * corr[t * cout + c] (host fp32, t = ky*3 + kx, cout <= 16) for the taps t outside the image. */
int damvs_conv2d_border_bias(void* stream, int dtype, int B, int H, int W, int cout_stored, int cout, const float* corr,
                             void* out);

/* FeatureNet's FPN top level (models/module.py:455-459, out3(up2(f) + inner2(c0))) in one launch, bf16:
 * out = conv3x3_p1(c0) + ConvTranspose2d_k4s2p1(f) + bias — the two layers of the re-association in
 * damvsnet_amd/frontend_hip.py:fpn_top_layers, fused. c0 [B][H][W][8], f [B][H/2][W/2][32], out [B][H][W][8]
 * (bf16); apack: 15 MFMA A chunks x 64 lanes x 8 bf16 (frontend_hip.pack_fpn_top: chunks 0-2 the 3x3 conv's
 * kernel rows as x-pair taps, 3-14 the transposed conv's (row parity, input row, x offset) taps); bias: device
 * fp32 [8]. H, W even. The border fix-up (damvs_conv2d_border_bias) follows as a separate call. */
int damvs_fpn_top_forward(void* stream, int B, int H, int W, const void* c0, const void* f, const void* apack,
                          const float* bias, void* out);

/* The same in fp32 storage (the fp32 parity path): c0, f, out fp32; the products as split-f16 MFMAs. apack: the
 * 15 A chunks scaled by 2^k (max |A| in (2^13, 2^14]) as f16 halves, [chunk][hi: 64 lanes x 8][lo: 64 lanes x 8]
 * (frontend_hip.pack_fpn_top_split); wscale = 2^-k. */
int damvs_fpn_top_forward_f32(void* stream, int B, int H, int W, const void* c0, const void* f, const void* apack,
                              float wscale, const float* bias, void* out);

/* ------------------------------------------------------------------ depth fusion (f4)
 * One reference view of the reference's dynamic-consistency fusion (filter/dypcd.py:98-297,
 * filter_depth per ref view): all maps [H][W] fp32 device buffers of one resolution. Camera
 * products are float32, formed on the host exactly as numpy forms them for float32 matrices. */
#define DAMVS_FUSION_MAX_SRC 10
typedef struct {
  float kinv_ref[9], k_ref[9], einv_ref[16];            /* inv(K_ref), K_ref, inv(E_ref) */
  float t_sr[DAMVS_FUSION_MAX_SRC][16];                  /* E_src . inv(E_ref) */
  float k_src[DAMVS_FUSION_MAX_SRC][9];
  float kinv_src[DAMVS_FUSION_MAX_SRC][9];
  float t_rs[DAMVS_FUSION_MAX_SRC][16];                  /* E_ref . inv(E_src) */
} damvs_fusion_cams;

/* conf: 3 maps (final-stage, stage-2, stage-1 confidence at the final resolution) or NULL (photo
 * test off); conf_thr: args.conf[0..2] (stage-1, stage-2, stage-3). Outputs: depth_avg (averaged
 * depth), mask (bit 0 photo, bit 1 geometric, bit 2 final), xyz [H][W][3] world points of final
 * pixels (0 elsewhere; NULL: not written). 1 <= nsrc <= DAMVS_FUSION_MAX_SRC. */
int damvs_fusion_view(void* stream, int H, int W, int nsrc, const float* depth_ref, const float* const* depth_src,
                      const float* const* conf, const float* conf_thr, const damvs_fusion_cams* cams, double dist_base,
                      double rel_diff_base, float* depth_avg, unsigned char* mask, float* xyz);

/* The same view under the reference's static rule (filter/pcd.py:58-113, 142-170, 190-208, the CasMVSNet filter):
 * a source agrees when its reprojection error is < dist_thr pixels (float64) and its relative depth difference is
 * < (float)rel_thr (float32); the reference's constants are dist_thr = 1, rel_thr = 0.01. The geometric mask is
 * "at least thres_view sources agree" (args.thres_view); the agreeing reprojected depths are averaged with the
 * reference depth. Unlike dypcd.py, pcd.py divides by the reprojected z unguarded: a zero depth gives inf / NaN and
 * fails both tests. Maps, conf, conf_thr, cams and the outputs are those of damvs_fusion_view.
 * 1 <= nsrc <= DAMVS_FUSION_MAX_SRC (DAMVS_E_SHAPE otherwise); thres_view >= 1 (DAMVS_E_ARG otherwise); a thres_view
 * above nsrc is legal and gives an empty geometric mask, as in the reference. */
int damvs_fusion_view_static(void* stream, int H, int W, int nsrc, const float* depth_ref,
                             const float* const* depth_src, const float* const* conf, const float* conf_thr,
                             const damvs_fusion_cams* cams, double dist_thr, double rel_thr, int thres_view,
                             float* depth_avg, unsigned char* mask, float* xyz);

/* The point cloud of one fused view (filter/dypcd.py:275-301, xyz[final] / color[final]): the view's final pixels
 * (mask bit value 4; bits 1 and 2 are ignored), in row-major pixel order, as PLY vertex records of 15 bytes: x, y, z
 * little-endian float32 from xyz [H][W][3], then red, green, blue from rgb [H][W][3] (the image bytes as decoded: the
 * reference's (float32(u) / 255 * 255).astype(uint8) is u for all 256 values), packed without padding. Record i of the
 * view is written at byte (base + i) * 15 of `records`, base = *cursor before the call, if and only if
 * base + i < capacity; *cursor becomes base + the view's count either way, so a cursor above the capacity says how
 * many records were needed. capacity 0 only counts (records may then be NULL); records needs no alignment.
 * Three launches on `stream` (count per tile, one-block scan, scatter), no atomics and no waiting between blocks: the
 * order is exact and the bytes are reproducible. The cursor is read and written by plain device loads and stores, so
 * all calls that share a cursor must be enqueued on one stream. scratch: damvs_fusion_cloud_scratch(H, W) unsigned
 * ints of device memory, free for reuse by the next call on the stream.
 * Errors (before any device work): a null pointer, scratch_elems too small or capacity < 0 -> DAMVS_E_ARG;
 * H < 1, W < 1 or H * W >= 2^31 -> DAMVS_E_SHAPE. */
int damvs_fusion_cloud_scratch(int H, int W);
int damvs_fusion_cloud(void* stream, int H, int W, const unsigned char* mask, const float* xyz, const unsigned char* rgb,
                       unsigned int* scratch, long long scratch_elems, unsigned char* records, long long capacity,
                       unsigned long long* cursor);

/* ------------------------------------------------------------------ oriented cloud: per-point normals (f4)
 * The normal of every final pixel of a fused view, from the view's averaged depth map and its camera: each point is a
 * pixel of an organised map, so the normal is a cross product of two finite differences and its orientation towards the
 * camera is known. fusion.normals_statement (Python) is the same rule in numpy; the kernels equal it bit for bit.
 * Inputs: depth_avg [H][W] and mask [H][W] as damvs_fusion_view wrote them (only bit value 4, final, is read); of cams
 * only kinv_ref (Kinv) and the rotation rows of einv_ref (Rinv) are read; jump, a relative depth step.
 * All arithmetic is IEEE double on the float32 inputs, one rounding per operation, sums left to right, no fused
 * multiply-add. For a final pixel c = (x, y), d = depth_avg:
 *   P(q) = Kinv (x_q d_q, y_q d_q, d_q), the camera-frame point of pixel q;
 *   a 4-neighbour q is usable when it lies inside the image, is final and |d_q - d_c| <= jump * d_c (NaN: not usable);
 *   tx = P(E) - P(W) when east (x + 1) and west are usable, P(E) - P(c) or P(c) - P(W) when one is, else missing;
 *   ty the same with south (y + 1) and north (y - 1);
 *   n = ty x tx, negated when n . P(c) > 0 (it faces the camera), n_cam = n / sqrt(n . n);
 *   when a tangent is missing or n . n is 0 or not finite: n_cam = -P(c) / sqrt(P(c) . P(c)), the direction to the camera;
 *   normal = (float) Rinv n_cam, not renormalised; (0, 0, 0) when a component is not finite.
 * damvs_fusion_normals writes normals [H][W][3] float32, (0, 0, 0) for pixels that are not final: one launch.
 * damvs_fusion_cloud_oriented is damvs_fusion_cloud with records of 27 bytes: x, y, z, nx, ny, nz little-endian float32,
 * then red, green, blue, packed without padding. `select` [H][W] picks the pixels (bit value 4): the fusion's mask, or
 * damvs_cloud_thin's keep; `mask` is the fusion's mask, by which the neighbours are judged (a selected pixel that is not
 * final there gets the normal (0, 0, 0)). The normal is computed in the scatter; no normal map is written. Order, cursor
 * and capacity are damvs_fusion_cloud's: record i of the view goes to byte (base + i) * 27 if and only if
 * base + i < capacity, *cursor advances by the view's count either way, capacity 0 only counts (records may be NULL).
 * Four launches on `stream` (damvs_fusion_cloud's three at capacity 0, then the oriented scatter, which reads their
 * scan from `scratch`), no atomics, nothing synchronised; calls that share a cursor must be enqueued on one stream.
 * scratch: damvs_fusion_cloud_scratch(H, W) unsigned ints.
 * Errors (before any device work): a null pointer, a jump that is negative, infinite or NaN, scratch_elems too small or
 * capacity < 0 -> DAMVS_E_ARG; H < 1, W < 1 or H * W >= 2^31 -> DAMVS_E_SHAPE. */
int damvs_fusion_normals(void* stream, int H, int W, const float* depth_avg, const unsigned char* mask,
                         const damvs_fusion_cams* cams, double jump, float* normals);
int damvs_fusion_cloud_oriented(void* stream, int H, int W, const unsigned char* select, const unsigned char* mask,
                                const float* depth_avg, const damvs_fusion_cams* cams, double jump, const float* xyz,
                                const unsigned char* rgb, unsigned int* scratch, long long scratch_elems,
                                unsigned char* records, long long capacity, unsigned long long* cursor);

/* ------------------------------------------------------------------ consensus fusion (f4)
 * The fusibile family's fusion over a whole scene: a depth sample that was merged into a point is consumed and is not
 * emitted again from its own view; the point written is the average of the agreeing views' 3D points and its colour
 * the average of their colours. fusion.consensus_statement (Python) is the same rule in numpy; the kernel equals it bit
 * for bit. The rule is this project's statement of the published algorithm with the thresholds the reference passes to
 * the external binary; parity with that binary is unverified.
 * The scene table holds, per view v of 0..V-1, its cameras and the device pointers of depth [H][W] float32, conf [H][W]
 * float32 (the final-stage confidence), rgb [H][W][3] uint8 and used [H][W] uint8 (all zero before the first view).
 * damvs_consensus_table_bytes gives its size; damvs_consensus_table fills `table` (device memory of that size) from the
 * host arrays: one copy on `stream`, synchronised before it returns, so the host arrays may be freed at once.
 * damvs_consensus_view runs one reference view, one thread per pixel, one launch:
 *   valid(v, q): depth finite, depth > 0 and not (conf < prob_thr) (a NaN confidence stays).
 *   A pixel p = (x, y) is skipped unless valid(ref, p) and used[ref][p] == 0. Then, in IEEE double on the float32 inputs,
 *   one rounding per operation, sums left to right, no fused multiply-add:
 *   X = Einv_ref (Kinv_ref (x d, y d, d)); for each source s = src[i] in list order: q = E_s X, skipped unless q.z > 0;
 *   u = K_s q, px = floor(u.x / u.z + 0.5), py likewise, skipped unless both are finite and inside the image;
 *   skipped unless valid(s, (px, py)), ds its depth; skipped unless |fb[i] / q.z - fb[i] / ds| < disp_thr (fb[i]: focal
 *   length times baseline of the pair, formed by the caller). Otherwise X_s = Einv_s (Kinv_s (px ds, py ds, ds)) is
 *   added to the position sum, rgb[s][py][px] to the channel sums, used[s][py][px] = 1 and n counts the source.
 *   When n >= num_consistent: xyz = (float)((X + X_s1 + ...) / (n + 1)), rgb_avg = (2 sum + (n + 1)) / (2 (n + 1)) in
 *   integers per channel; otherwise xyz and rgb_avg are 0.
 *   mask: 1 valid | 2 n >= num_consistent | 4 emitted | 8 used[ref][p] was set on entry: the mask damvs_fusion_cloud takes.
 * A launch writes `used` of its sources only and reads `used` of its reference view only, so its result does not depend
 * on the order of its threads; the views of a scene must run one after another on one stream.
 * Errors (before any device work): a null pointer, ref among the sources, a repeated source, num_consistent < 1, a
 * threshold that is infinite or NaN -> DAMVS_E_ARG; H < 1, W < 1, H * W >= 2^31, V outside 1..DAMVS_CONSENSUS_MAX_VIEWS,
 * nsrc outside 1..DAMVS_CONSENSUS_MAX_VIEWS - 1, ref or a source outside 0..V-1 -> DAMVS_E_SHAPE. */
#define DAMVS_CONSENSUS_MAX_VIEWS 64
typedef struct damvs_consensus_cam {
  float k[9], kinv[9]; /* K and inv(K), row-major */
  float e[16], einv[16]; /* E and inv(E), row-major */
} damvs_consensus_cam;
int damvs_consensus_table_bytes(int V, size_t* bytes);
int damvs_consensus_table(void* stream, int H, int W, int V, const damvs_consensus_cam* cams, const float* const* depth,
                          const float* const* conf, const unsigned char* const* rgb, unsigned char* const* used,
                          void* table);
int damvs_consensus_view(void* stream, int H, int W, int V, const void* table, int ref, int nsrc, const int* src,
                         const double* fb, float prob_thr, double disp_thr, int num_consistent, unsigned char* mask,
                         float* xyz, unsigned char* rgb_avg);

/* ------------------------------------------------------------------ voxel-thinned cloud (f4)
 * At most one point per cell of an axis-aligned grid, chosen on the device between the fusion kernel and
 * damvs_fusion_cloud: of a scene's selected pixels (mask bit value 4), the first one in cloud order of every cell is
 * kept. Cloud order is the PLY's: the views in the order of the calls, row-major pixels inside a view; pixel p of a call
 * has the ordinal base + p, base = the sum of n over the calls before it on this table (a host number).
 * The rule, per selected pixel with point (x, y, z) of xyz [n][3]:
 *   q = floor(x * inv_voxel) per axis (one float32 multiply, floor, integer), inv_voxel = float32(1) / float32(edge)
 *   formed by the caller; the pixel is in range when -2^20 <= q < 2^20 on all three axes (NaN and infinities are not);
 *   cell key = (qx + 2^20) | (qy + 2^20) << 21 | (qz + 2^20) << 42, 63 bits; all ones marks an empty slot.
 *   keep[p] = 4 if and only if no selected in-range pixel of a lower ordinal has the same key; else 0 (unselected and
 *   out-of-range pixels too). keep [n] is a mask in the form damvs_fusion_cloud takes.
 * The table is one open-addressing hash table per scene: `slots` 64-bit keys, `slots` 64-bit owners (the lowest ordinal
 * that claimed the key), then a status word: *bytes of damvs_cloud_thin_table_bytes (16 * slots + 8; the size passes
 * 2^31 from 2^27 slots on, hence the out-parameter, as damvs_stage_workspace_size has) of device memory, 8-byte aligned,
 * slots a power of two in [64, 2^32]. damvs_cloud_thin_clear empties it (one hipMemsetAsync of the slots to all ones,
 * one of the status) and must run, on the same stream, before the scene's first damvs_cloud_thin.
 * damvs_cloud_thin is two launches on `stream`: claim (per selected pixel, linear probing from a hash of the key; per
 * slot a 64-bit compare-and-swap empty -> key and, when it returned empty or the key, a 64-bit unsigned atomic min of
 * the ordinal into the owner; every decision rests on an atomic's returned value; a counted loop of at most `slots`
 * trips, no thread waits for another) and resolve (plain loads: keep[p] = 4 where the owner is p's ordinal). The kept
 * set depends on neither the hash, the table size nor the order in which threads arrive, and is bit for bit
 * reproducible. The call allocates nothing and does not synchronise, so it can be captured into a graph; calls that
 * share a table must be enqueued on one stream (or otherwise ordered).
 * A selected pixel out of range, or one that found no slot in a full table, sets a bit of the status word and claims
 * nothing; keep is then not the rule's. damvs_cloud_thin_status synchronises `stream`, returns DAMVS_OK,
 * DAMVS_E_RANGE (a selected point out of range) or DAMVS_E_WORKSPACE (the table was full: use more slots), with a
 * message that names which, and clears the status.
 * damvs_cloud_thin_hash: *slot = the slot a key's probe starts from in a table of `slots` slots (a host function; for
 * tests that place probe chains).
 * Errors (before any device work): a null pointer, a table that is not 8-byte aligned, slots not a power of two in
 * [64, 2^32], inv_voxel not finite or not positive, base outside [0, 2^62] -> DAMVS_E_ARG; n < 1 or n >= 2^31 ->
 * DAMVS_E_SHAPE. */
int damvs_cloud_thin_table_bytes(long long slots, size_t* bytes);
int damvs_cloud_thin_hash(unsigned long long key, long long slots, long long* slot);
int damvs_cloud_thin_clear(void* stream, void* table, long long slots);
int damvs_cloud_thin(void* stream, long long n, const unsigned char* mask, const float* xyz, float inv_voxel,
                     long long base, void* table, long long slots, unsigned char* keep);
int damvs_cloud_thin_status(void* stream, void* table, long long slots);

/* ------------------------------------------------------------------ scene ingest (f4)
 * The outputs of one forward over B reference views, written into scene-resident stores that the fusion entry points
 * above read in place. It replaces the host path of test_uni.py:246-287 (maps to the host, cv2.INTER_NEAREST resize of
 * the stage-1 / stage-2 confidences, PFM files, the reference image as (img * 255).astype(uint8)) and the reader side
 * filter/dypcd.py:198-209 (the files read back and uploaded). Inputs, device fp32, contiguous: depth and conf3
 * [B][H][W] (final stage), conf2 [B][H/2][W/2], conf1 [B][H/4][W/4]; img: sample b's reference image at
 * img + b * img_batch_stride floats, three planes (red, green, blue) of H * W floats, so view 0 of a (B, N, 3, H, W)
 * batch is read in place with img_batch_stride = N * 3 * H * W; NULL: rgb_store is not written (and may be NULL).
 * Stores, device, V views of one size; sample b goes to slot s = slots[b]:
 *   depth_store [V][H][W] fp32            depth_store[s] = depth[b]
 *   conf_store  [V][3][H][W] fp32         the order damvs_fusion_view takes: [s][0] = conf3[b],
 *                                         [s][1][y][x] = conf2[b][y >> 1][x >> 1], [s][2][y][x] = conf1[b][y >> 2][x >> 2]
 *                                         (INTER_NEAREST at exactly x2 and x4)
 *   rgb_store   [V][H][W][3] uint8        [s][y][x][c] = uint8(trunc(clip(img[b][c][y][x] * 255.0f, 0, 255))): one fp32
 *                                         multiply rounded to nearest, clamp, truncation, as numpy computes it in float32
 * slots is a HOST array of B distinct entries in [0, V); it is copied into the kernel arguments, so the call needs no
 * device memory of its own, does not synchronise, and can be captured into a graph. One launch on `stream`; slots not
 * named are not touched.
 * Errors (before any device work): a null pointer other than img (rgb_store may be null only when img is), a slot
 * outside [0, V) or repeated, a full-size map or store not 16-byte aligned (conf2: 8, rgb_store: 4), img_batch_stride
 * not a multiple of 4 -> DAMVS_E_ARG; B outside 1..DAMVS_SCENE_MAX_BATCH, H or W not a positive multiple of 4, V < 1,
 * H * W * 12 >= 2^31 -> DAMVS_E_SHAPE. */
#define DAMVS_SCENE_MAX_BATCH 64
int damvs_scene_ingest(void* stream, int B, int H, int W, int V, const float* depth, const float* conf3,
                       const float* conf2, const float* conf1, const float* img, long long img_batch_stride,
                       const int* slots, float* depth_store, float* conf_store, unsigned char* rgb_store);

/* ------------------------------------------------------------------ scene inputs (f3)
 * The forward's `imgs` tensor for a batch, written from the scene's decoded images, which stay on the device as the
 * bytes they were decoded to. It replaces the host path of datasets/general_eval.py:83-108 (np.array(img, float32) /
 * 255, the resize to the working size) and the upload of B * N float32 images per batch.
 *   rgb_store [V][H0][W0][3] uint8, device: V decoded views of one size
 *   out       [n_images][3][H][W] fp32, device: out[i] is view slots[i] as float32 in [0, 1], resized to H x W, planar;
 *             with n_images = B * N and i = b * N + n it is the contiguous (B, N, 3, H, W) tensor of the forward
 * Arithmetic, all float32, every operation rounded to nearest on its own: p = float(byte) / 255; per axis with n_in
 * source and n_out output samples scale = float(n_in) / float(n_out), src = max(fma(scale, float(d) + 0.5f, -0.5f), 0)
 * (one rounding for the multiply-add), i0 = min(int(src), n_in - 1), i1 = min(i0 + 1, n_in - 1), l1 = src - float(i0),
 * l0 = 1 - l1; out = a0 * (b0 * p00 + b1 * p01) + a1 * (b0 * p10 + b1 * p11) with a the row and b the column weights:
 * bilinear interpolation with half-pixel centres and clamped borders (torch's F.interpolate, align_corners=False, as
 * its CPU kernel computes it; tests/inputs_statement.py states it in numpy). At H == H0 and W == W0 the output is
 * float(byte) / 255 exactly.
 * slots is a HOST array of n_images entries in [0, V), which may repeat; it is copied into the kernel arguments, so the
 * call needs no device memory of its own, does not synchronise, and can be captured into a graph. One launch on
 * `stream`.
 * Errors (before any device work), all DAMVS_E_ARG with a message that names the argument: a null pointer, n_images
 * outside 1..DAMVS_INPUTS_MAX_IMAGES, a size below 1, W not a multiple of 4, out not 16-byte aligned, a slot outside
 * [0, V), 3 * H0 * W0 or 3 * H * W >= 2^31. */
#define DAMVS_INPUTS_MAX_IMAGES 128
int damvs_scene_inputs(void* stream, int n_images, int H0, int W0, int H, int W, int V,
                       const unsigned char* rgb_store, const int* slots, float* out);

/* ------------------------------------------------------------------ scene features (f1)
 * A batch's FeatureNet outputs, gathered from scene stores in which every view's features were written once (FeatureNet's
 * output depends on the image alone; scene.SceneFeatures). For pair i < n_pairs (a sample's view) and tensor k < K:
 *   outs[k] + i * view_bytes[k]  <-  stores[k] + slots[i] * view_bytes[k]        view_bytes[k] bytes
 * stores[k] holds V blocks of view_bytes[k] bytes, outs[k] n_pairs of them. The call moves bytes and knows nothing of
 * dtype or shape, so one launch serves the three stages' tensors, whose sizes differ, in either storage type.
 * stores, view_bytes, slots and outs are HOST arrays (K, K, n_pairs and K entries); slots may repeat. They are copied
 * into the kernel arguments, so the call needs no device memory of its own, does not synchronise, and can be captured
 * into a graph. One launch on `stream`: blockIdx.z the pair, blockIdx.y the tensor, blockIdx.x striding over the view's
 * 16-byte vectors with min(blocks the largest tensor needs, 2048 / (n_pairs * K)) blocks of 256 threads.
 * Errors (before any device work), with a message that names the argument:
 *   DAMVS_E_ARG    a null pointer (an array or one of its K entries), a store or out that is not 16-byte aligned;
 *   DAMVS_E_SHAPE  n_pairs outside 1..DAMVS_FEATURES_MAX_PAIRS, K outside 1..DAMVS_FEATURES_MAX_TENSORS, V < 1, a slot
 *                  outside [0, V), a view_bytes[k] that is 0, not a multiple of 16, or >= 2^31. */
#define DAMVS_FEATURES_MAX_PAIRS 128
#define DAMVS_FEATURES_MAX_TENSORS 4
int damvs_feature_gather(void* stream, int n_pairs, int K, int V, const void* const* stores,
                         const unsigned long long* view_bytes, const int* slots, void* const* outs);

#ifdef __cplusplus
}
#endif

#endif /* DAMVS_H */
