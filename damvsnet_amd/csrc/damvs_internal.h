// Internal declarations shared by the HIP kernels and the C-ABI layer (not installed).
//
// Layouts (all device, row-major, innermost last):
//   features  [B][h][w][C]            (NHWC, T = float | bf16)
//   volume    [B][D][h][w][C]         (NDHWC, T)
//   hyps      [B][D][h][w]            float
//   rt        [B][N-1][12]            float: R row-major (9) then t (3) of P_src * inv(P_ref)
//   logits    [B][D][h][w]            float
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "conv_phases.h"
#include "switches.h"
#include "warp_tiles.h"

namespace damvs {

typedef uint16_t bf16_t;  // bf16 storage (upper half of an IEEE f32)

enum StoreType { ST_F32 = 0, ST_BF16 = 1 };
enum AggMode { AGG_ADAPTIVE = 0, AGG_VARIANCE = 1, AGG_WARP_ONLY = 2 };

constexpr int kMaxViews = 16;
// magnitude slots of the fp32 prescale (damvs_device.h prescale_of; include/damvs.h DAMVS_AMAX_SLOT_BYTES)
constexpr int kAmaxReps = 32;    // replicas per slot (one 128-byte line each): atomics spread over 32 addresses
constexpr int kAmaxStride = 32;  // words between replicas
constexpr int kAmaxSlotWords = kAmaxReps * kAmaxStride;

// ---------------------------------------------------------------- warp + aggregation
struct WarpArgs {
  const void* feats[kMaxViews];  // N views, view 0 = reference
  const float* rt;               // [B][N-1][12]
  const float* hyps;             // [B][D][out_rows][w]
  void* out;                     // [B][D][out_rows][w][C]
  int B, N, C, D, h, w;          // h x w: the feature maps (and the full reference image grid)
  int y0, rows;                  // computed: reference rows [y0, y0 + rows) (0, h: the whole image) ...
  int out_rows, out_y;           // ... at rows [out_y, out_y + rows) of the hyps / out planes
  // adaptive weight net, BN folded: a = relu(sum_c k1[c] x_c * s1 + t1); wt = relu(a * s2 + t2)
  float k1[32];
  float s1, t1, s2, t2;
  // pixel-block shape (set by the warp launcher): tiles across the width (warp_tiles.h)
  int tiles_x;
  unsigned* out_amax;  // fp32: magnitude slots of the written volume, one per batch element (prescale_of), or nullptr
};

// n / d for 0 <= n < 2^31 without a hardware divide: q = (umulhi(n, mul) + n) >> shift.
struct FastDiv {
  uint32_t mul, shift;
  int d;
};
inline FastDiv make_fastdiv(int d) {
  FastDiv f;
  f.d = d;
  uint32_t sh = 0;
  while (sh < 31 && (1u << sh) < (uint32_t)d) ++sh;
  f.shift = sh;
  f.mul = (uint32_t)((((uint64_t)1 << 32) * (((uint64_t)1 << sh) - (uint64_t)d)) / (uint64_t)d + 1);
  return f;
}
#ifdef __HIPCC__
__device__ __forceinline__ int fdiv(const FastDiv& f, int n) {
  return (int)((__umulhi((uint32_t)n, f.mul) + (uint32_t)n) >> f.shift);
}
#endif

// ---------------------------------------------------------------- MFMA implicit-GEMM conv3d
// phases: ConvPhase, conv_phases.h
struct ConvArgs {
  const void* in;
  void* out;
  const void* resid;   // added after ReLU (may alias out); nullptr if none
  const void* wpack;   // packed A fragments, see pack_conv_weights()
  const void* wpack_pair;  // row-pair packing (stride-1, Cout <= 8), nullptr if none
  const void* wpack32;     // fp32: the z-streamed kernel's packing of this layer, 32 K per chunk, split-f16
  const void* wgat32;      // fp32: the gather kernel's packing at 32 K per chunk (split-f16; phases of build_phases(., 32))
                           // [chunk][hi: 64 lanes][lo: 64 lanes] (x-pair for conv11, row pairs for conv0), or nullptr
  const float* bias;   // [Cout] (folded BN shift)
  int B, Cin, Cout, MT;
  int Di, Hi, Wi;
  int Dq, Hq, Wq;
  int Do, Ho, Wo;
  int in_stride, out_stride;
  int relu;
  int nphase;
  int xpair;  // deconv phases are (pz, py) with both x parities in the MFMA rows (Cout <= 8)
  float wscale;  // accumulator scale of the epilogue: 2^-k of the split-f16 fp32 weights (damvs_device.h), 1 for bf16
  FastDiv div_wq, div_hq, div_dq;  // set by launch_conv3d
  ConvPhase ph[kMaxPhases];
  // fp32: the phases of wgat32 (build_phases(., 32) at layer creation): K chunks and weight offsets at 32 K per chunk
  // (the taps are those of ph)
  int k32_chunks[kMaxPhases], k32_off[kMaxPhases];
  // fp32 activation prescale (damvs_device.h prescale_of): the input tensor's magnitude slots (nullptr: unscaled) and
  // the slots this layer's stored outputs are recorded into (nullptr: not recorded), one slot (kAmaxSlotWords words)
  // per batch element: a sample's scales do not depend on the rest of its batch; bf16 ignores both
  const unsigned* in_amax;
  unsigned* out_amax;
};

// ---------------------------------------------------------------- 2D front-end convolutions
// phases: Conv2dPhase, conv_phases.h
struct Conv2dArgs {
  const void* in0;
  const void* in1;
  int c0, c1;
  const float* geo[4];      // planar fp32 [B][Hi][Wi] planes at the input resolution
  long long geo_bstride[4]; // elements between batches of each geo plane
  int ngeo;
  const void* wpack;
  const float* wgeo;
  const float* bias;        // [cout_pad]
  const void* res_pre;      // added before ReLU, [B][Ho][Wo][cout]
  const void* res_post;     // added after ReLU, [B][Ho/up][Wo/up][cout]
  int post_up;
  void* out;                // [B][Ho][Wo][cout]
  int cout, cout_pad, MTtot;
  int B, Hi, Wi, Hq, Wq, Ho, Wo, in_stride, out_stride, relu, nphase;
  FastDiv div_wq, div_hq;   // output-grid decomposition q -> (b, qy, qx)
  int xpair;                // transposed stride 2, cout 8: both x parities in one phase's 16 MFMA rows
  float wscale;             // accumulator scale of the epilogue (see ConvArgs)
  int wide32;               // fp32: ph / wpack are the 32-K split packing of conv2d_wide_kernel<float>
  Conv2dPhase ph[4];
};

// ---------------------------------------------------------------- launchers (return hipError_t)
hipError_t launch_proj_prepare(hipStream_t s, int B, int N, const float* proj, float* rt);
// status[0] = 1 when any of the n floats of a, b or c is non-finite (sticky: damvs_stage_status clears it)
hipError_t launch_finite_check(hipStream_t s, const float* a, const float* b, const float* c, long long n, int* status);
// fold max |x| of n floats into a magnitude slot (damvs_device.h prescale_of)
hipError_t launch_amax(hipStream_t s, const float* x, long long n, unsigned* slot);
hipError_t launch_hyp_linear(hipStream_t s, int B, int D, int h, int w, const float* dv, int Dv, float* out);
hipError_t launch_hyp_refine(hipStream_t s, int B, int D, int H, int W, int scale, const float* pd,
                             const float* pv, int hp, int wp, float* out);
hipError_t launch_sparse_pyramid(hipStream_t s, int B, int h, int w, const float* depth, const float* dv, int Dv,
                                 const float* mask, float* d0, float* d1, float* d2, float* d3, float* m1, float* m2);
struct FeatPtrs {
  const void* p[kMaxViews];
};
// blocked = features in channel-blocked layout [B][C/E][h][w][E] (E = 16 bytes of channels)
hipError_t launch_warp_aggregate(hipStream_t s, int store, int mode, const WarpArgs& a, bool blocked);
bool warp_split_for(int bytes, int N);  // the channel-split warp serves NHWC maps of these pixels at N views
hipError_t launch_block_channels(hipStream_t s, int store, const FeatPtrs& src, const FeatPtrs& dst, int N, int B,
                                 int hw, int C);
hipError_t launch_conv3d(hipStream_t s, int store, const ConvArgs& a);
// a: the layer on its 16-K packing (bf16: its only one); a32: the same fp32 layer on its 32-K split packing (a32->wide32
// set), or nullptr when it has none. conv2d_route (k_conv2d.hip) picks the kernel and the packing.
// rep: instead of launching, the launcher that would launch writes "<kernel><template arguments> grid=(x,y)" into
// rep->buf (damvs_conv2d_route; report_kernel, conv2d_common.h). No HIP call is made then.
struct Conv2dReport {
  char* buf;
  size_t n;    // bytes of buf
  size_t len;  // characters of the whole report (>= n: it did not fit); 0 when no launcher was reached
};
hipError_t launch_conv2d(hipStream_t s, int store, const Conv2dArgs& a, const Conv2dArgs* a32, Conv2dReport* rep = nullptr);
// layers whose only inputs are fp32 planes (c0 = c1 = 0), on the VALU (k_planes.hip)
hipError_t launch_conv2d_planes(hipStream_t s, int store, const Conv2dArgs& a, Conv2dReport* rep = nullptr);
struct BorderArgs {
  float corr[9 * 16];  // [tap][channel] of a 3x3 conv, channels < 16
};
hipError_t launch_fpn_top(hipStream_t s, int store, int B, int H, int W, const void* c0, const void* f,
                          const void* apack, float wscale, const float* bias, void* out);
hipError_t launch_border_bias(hipStream_t s, int store, const BorderArgs& a, int B, int H, int W, int cstored, int cout,
                              void* out);
// ---------------------------------------------------------------- depth fusion (filter/dypcd.py)
constexpr int kFusionMaxSrc = 10;  // the reference's masks run to i = 10 (dypcd.py:152)
struct FusionCam {
  float t_sr[16], k_src[9], kinv_src[9], t_rs[16];  // E_src inv(E_ref), K_src, inv(K_src), E_ref inv(E_src)
};
struct FusionArgs {
  int H, W, nsrc;
  const float* depth_ref;
  const float* depth_src[kFusionMaxSrc];
  const float* conf[3];  // final, stage-2, stage-1 confidences (nullptr: photometric test off)
  float conf_thr[3];     // args.conf: stage-1, stage-2, stage-3 thresholds
  float kinv_ref[9], k_ref[9], einv_ref[16];
  FusionCam src[kFusionMaxSrc];
  double dist_thr[9];    // i * dist_base, i = 2..10
  float rel_thr[9];      // float32(i * rel_diff_base)
  float* depth_avg;
  unsigned char* mask;   // bit 0 photo, bit 1 geo, bit 2 final
  float* xyz;            // world points of final pixels (0 elsewhere), or nullptr
};
hipError_t launch_fusion_view(hipStream_t s, const FusionArgs& a);
// The static rule (filter/pcd.py): dist_thr[0] / rel_thr[0] carry its two fixed thresholds (the other slots are not
// read), a pixel is geometrically consistent when at least thres_view sources agree.
hipError_t launch_fusion_view_static(hipStream_t s, const FusionArgs& a, int thres_view);
// the source stamp (DAMVS_BUILD_ID) of the library that holds the static-rule kernel (k_fusion_static.hip)
const char* fusion_static_build_id();

// ---------------------------------------------------------------- fused point cloud (k_cloud.hip, libdamvs_cloud.so)
constexpr int kCloudTile = 256;  // consecutive pixels per block of the count and scatter launches
struct CloudArgs {
  long long n;                // H * W
  unsigned ntiles;            // fusion_cloud_tiles(n)
  const unsigned char* mask;  // [n] as the fusion kernels write it; bit value 4 (final) selects
  const float* xyz;           // [n][3]
  const unsigned char* rgb;   // [n][3]
  unsigned* scratch;          // [ntiles + 2]: tile counts / offsets, then the cursor before the call (low, high)
  unsigned char* records;     // 15-byte records
  long long capacity;         // records that fit; the ones past it are counted, not written
  unsigned long long* cursor; // records written so far by the calls on this stream
};
int fusion_cloud_tiles(long long n);
// count, scan, scatter on s; calls that share a cursor must be on one stream
hipError_t launch_fusion_cloud(hipStream_t s, const CloudArgs& a);
const char* fusion_cloud_build_id();

// ---------------------------------------------------------------- scene ingest (k_scene.hip, libdamvs_scene.so)
constexpr int kSceneMaxBatch = 64;                  // DAMVS_SCENE_MAX_BATCH: the slot table lives in the kernel arguments
constexpr int kSceneBlockX = 64, kSceneBlockY = 4;  // threads: 64 groups of 4 pixels across, 4 rows
struct SceneArgs {
  int H, W;                   // multiples of 4, H * W * 12 < 2^31
  const float* depth;         // [B][H][W]
  const float* conf3;         // [B][H][W]
  const float* conf2;         // [B][H/2][W/2]
  const float* conf1;         // [B][H/4][W/4]
  const float* img;           // sample b: img + b * img_bstride, three planes [H][W]; nullptr: rgb not written
  long long img_bstride;      // floats
  float* depth_store;         // [V][H][W]
  float* conf_store;          // [V][3][H][W]: final, stage 2, stage 1
  unsigned char* rgb_store;   // [V][H][W][3]
  int slots[kSceneMaxBatch];  // sample b -> slot
};
hipError_t launch_scene_ingest(hipStream_t s, int B, const SceneArgs& a);
const char* scene_build_id();

// ---------------------------------------------------------------- scene inputs (k_inputs.hip, libdamvs_inputs.so)
constexpr int kInputsMaxImages = 128;                 // DAMVS_INPUTS_MAX_IMAGES: the slot table lives in the kernel arguments
constexpr int kInputsBlockX = 64, kInputsBlockY = 4;  // threads: 64 groups of 4 output pixels across, 4 rows
struct InputsArgs {
  int H0, W0;                       // size of the stored images, 3 * H0 * W0 < 2^31
  int H, W;                         // size of the output images, W a multiple of 4, 3 * H * W < 2^31
  const unsigned char* rgb_store;   // [V][H0][W0][3]
  float* out;                       // [n_images][3][H][W], 16-byte aligned
  int slots[kInputsMaxImages];      // image i -> slot
};
hipError_t launch_scene_inputs(hipStream_t s, int n_images, const InputsArgs& a);
const char* inputs_build_id();

// ---------------------------------------------------------------- scene features (k_features.hip, libdamvs_features.so)
constexpr int kFeaturesMaxPairs = 128;      // DAMVS_FEATURES_MAX_PAIRS: the slot table lives in the kernel arguments
constexpr int kFeaturesMaxTensors = 4;      // DAMVS_FEATURES_MAX_TENSORS
constexpr int kFeaturesBlock = 256;         // threads, one 16-byte vector each per grid pass
constexpr int kFeaturesGridBlocks = 2048;   // the launch's blocks over all pairs and tensors (256 CUs x 8), about
struct FeaturesArgs {
  const unsigned char* store[kFeaturesMaxTensors];  // [V][view_bytes[k]], 16-byte aligned
  unsigned char* out[kFeaturesMaxTensors];          // [n_pairs][view_bytes[k]], 16-byte aligned
  unsigned nvec[kFeaturesMaxTensors];               // view_bytes[k] / 16, in [1, 2^27)
  int slots[kFeaturesMaxPairs];                     // pair i -> slot
};
// blocks along x: those the largest tensor needs, at most kFeaturesGridBlocks / (n_pairs * K) (at least 1)
unsigned feature_gather_grid_x(int n_pairs, int K, unsigned max_nvec);
hipError_t launch_feature_gather(hipStream_t s, int n_pairs, int K, const FeaturesArgs& a);
const char* features_build_id();

// ---------------------------------------------------------------- voxel thinning (k_thin.hip, libdamvs_thin.so)
constexpr int kThinBlock = 256;                    // threads, one pixel each
constexpr unsigned long long kThinEmpty = ~0ull;   // an unclaimed slot's key and owner; no cell key (63 bits) equals it
constexpr unsigned kThinFull = 1u, kThinRange = 2u;  // bits of the status word
constexpr long long kThinMinSlots = 64, kThinMaxSlots = 1LL << 32;
// The slot a key's probe starts from (slots a power of two): MurmurHash3's 64-bit finalizer, so that the keys of
// neighbouring cells, which differ in a few low bits of three 21-bit fields, start from unrelated slots.
// The kept points never depend on it (they are the first of their cell in cloud order); damvs_cloud_thin_hash hands it
// to the tests that place probe chains.
__host__ __device__ inline unsigned long long thin_hash(unsigned long long key, unsigned long long slots) {
  key ^= key >> 33;
  key *= 0xff51afd7ed558ccdull;
  key ^= key >> 33;
  key *= 0xc4ceb9fe1a85ec53ull;
  key ^= key >> 33;
  return key & (slots - 1ull);
}
struct ThinArgs {
  long long n;                // H * W, in [1, 2^31)
  const unsigned char* mask;  // [n] as the fusion kernels write it; bit value 4 (final) selects
  const float* xyz;           // [n][3]
  float inv_voxel;            // float32(1) / float32(voxel), formed by the caller
  unsigned long long base;    // ordinal of the view's pixel 0: the sum of n over the views claimed before
  unsigned long long* keys;   // [slots]
  unsigned long long* owners; // [slots] the lowest ordinal that claimed the slot's key
  unsigned* status;           // kThinFull | kThinRange, set by atomic OR
  unsigned long long slots;   // a power of two in [kThinMinSlots, kThinMaxSlots]
  unsigned char* keep;        // [n] 4 where the pixel owns its cell, else 0
};
// claim, then resolve, on s
hipError_t launch_cloud_thin(hipStream_t s, const ThinArgs& a);
const char* thin_build_id();

// ---------------------------------------------------------------- point normals (k_normals.hip, libdamvs_normals.so)
struct NormalArgs {
  int H, W;
  long long n;                  // H * W
  unsigned ntiles;              // fusion_cloud_tiles(n)
  const float* depth;           // [n] the fusion's depth_avg
  const unsigned char* mask;    // [n] the fusion's mask: bit value 4 (final) says which neighbours count
  float kinv[9], rinv[9];       // inv(K_ref) and the rotation rows of inv(E_ref), as damvs_fusion_cams holds them
  double jump;                  // relative depth step above which a neighbour is not used
  float* normals;               // map form: [n][3]
  // scatter form (after launch_fusion_cloud at capacity 0 with `select` as its mask, same stream and scratch)
  const unsigned char* select;  // [n] bit value 4 selects the pixel
  const float* xyz;             // [n][3]
  const unsigned char* rgb;     // [n][3]
  const unsigned* scratch;      // [ntiles + 2] as cloud_scan_kernel left it
  unsigned char* records;       // 27-byte records
  long long capacity;
};
hipError_t launch_normal_map(hipStream_t s, const NormalArgs& a);
hipError_t launch_cloud_oriented(hipStream_t s, const NormalArgs& a);
const char* normals_build_id();

// ---------------------------------------------------------------- consensus fusion (k_consensus.hip, libdamvs_consensus.so)
constexpr int kConsensusBlock = 256;     // reference pixels per block
constexpr int kConsensusMaxViews = 64;   // DAMVS_CONSENSUS_MAX_VIEWS: a launch takes at most 63 sources
// One view of the scene table in device memory (damvs_consensus_table writes it, 232 bytes a view).
struct ConsensusEntry {
  float k[9], kinv[9], e[16], einv[16];  // K, inv(K), E, inv(E) as float32, row-major
  const float* depth;                    // [H][W]
  const float* conf;                     // [H][W] final-stage confidence
  const unsigned char* rgb;              // [H][W][3]
  unsigned char* used;                   // [H][W] 1: the sample was merged into a point of an earlier view
};
struct ConsensusArgs {
  int H, W;
  long long n;                  // H * W
  const ConsensusEntry* table;  // [V]
  int ref, nsrc, num_consistent;
  float prob_thr;
  double disp_thr;
  unsigned char* mask;          // [n] 1 valid | 2 geo | 4 emitted | 8 consumed on entry
  float* xyz;                   // [n][3]
  unsigned char* rgb_avg;       // [n][3]
  int src[kConsensusMaxViews - 1];
  double fb[kConsensusMaxViews - 1];  // focal length times baseline per source
};
hipError_t launch_consensus_view(hipStream_t s, const ConsensusArgs& a);
const char* consensus_build_id();

// ---------------------------------------------------------------- stage tail (k_regress.hip)
// prob_mfma_kernel's A operand (pack_prob_rows, capi.cpp): 18 voxel slots x 8 channels in 5 K chunks; bf16 terms per
// fp32 prob-conv weight (hi + lo)
constexpr int kProbRowChunks = 5, kProbRowTerms = 2;
// The prob conv alone (first pass of the two-pass tail; damvs_costreg_logits): logits (+ prob_init) to HBM.
// hipErrorInvalidValue for a base other than 8 or 16.
hipError_t launch_prob_conv(hipStream_t s, int store, int B, int Cb, int D, int h, int w, const void* feat,
                            const float* wprob, const float* prob_init, float* logits);
// The regression alone, from logits in HBM (second pass of the two-pass tail; damvs_regress).
hipError_t launch_regress(hipStream_t s, int B, int D, int h, int w, const float* logits, const float* hyps,
                          float* depth, float* conf, float* var, float* prob);
// A stage's prob conv + regression on the form tail_route picks. apack: the stage's MFMA packing for its storage type
// (bf16: prob_pack; fp32: prob_split with pscale its 2^-k), or nullptr; logits: scratch of the two-pass form.
// Returns the first failing launch's error with *what its hip_check label. A two-pass route without logits launches
// nothing and returns an error with *what = nullptr (the caller's DAMVS_E_WORKSPACE).
struct TailArgs {
  int B, Cb, D, h, w;
  const void* feat;     // [B][D][h][w][Cb], storage type
  const float* wprob;   // [kd][kh][kw][Cb]
  const void* apack;
  float pscale;
  const float* prob_init;
  const float* hyps;
  float* logits;
  float *depth, *conf, *var, *prob;  // prob may be nullptr
};
hipError_t launch_tail(hipStream_t s, int store, const TailArgs& a, const char** what);

#ifdef __HIPCC__
// Launch a kernel whose dynamic LDS may exceed the 64 KB a kernel gets without asking: above that, raise the kernel's
// limit first. Returns the attribute call's error, else the launch's.
template <typename... P, typename... A>
hipError_t launch_big_lds(void (*k)(P...), dim3 grid, dim3 block, size_t smem, hipStream_t s, const A&... args) {
  if (smem > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)smem);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k, grid, block, smem, s, args...);
  return hipGetLastError();
}
#endif

}  // namespace damvs
