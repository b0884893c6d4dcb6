// C ABI of libdamvs.so (include/damvs.h): parameter folding/packing at create time and
// stream-ordered orchestration of the per-stage kernels.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "damvs.h"
#include "damvs_internal.h"
#include "weight_pack.h"

using namespace damvs;

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

int hip_check(hipError_t e, const char* what) {
  if (e == hipSuccess) return DAMVS_OK;
  return fail(DAMVS_E_HIP, "%s: %s", what, hipGetErrorString(e));
}

#define DAMVS_TRY(expr)            \
  do {                             \
    int _rc = (expr);              \
    if (_rc != DAMVS_OK) return _rc; \
  } while (0)

struct LayerPlan {
  int kind = 0, cin = 0, cout = 0, mt = 0, nphase = 0;
  ConvPhase ph[kMaxPhases];
  void* wpack = nullptr;
  void* wpack_pair = nullptr;  // Cout <= 8: row-pair packing (stride 1, conv3d_lds_pair_kernel) or
                               // x-parity-pair phases (deconv, conv3d_mfma_kernel<.., XP>)
  int nphase_pair = 0;
  ConvPhase ph_pair[4];
  float* bias = nullptr;
  float wscale = 1.f;  // fp32: 2^-k of the split-f16 weights (split_weights)
  void* wpack32 = nullptr;  // fp32: the z-streamed kernel's 32-K split packing (ConvArgs::wpack32)
  void* wgat32 = nullptr;   // fp32: the gather kernel's 32-K split packing (ConvArgs::wgat32; may alias wpack32)
  int k32_chunks[kMaxPhases] = {0}, k32_off[kMaxPhases] = {0};  // its phases' K chunks / weight offsets (build_phases 32)
};

size_t align_up(size_t x) { return (x + 255) & ~size_t(255); }

}  // namespace

struct damvs_stage {
  int C = 0, base = 0, mode = 0, dtype = 0, device = 0;
  LayerPlan L[10];
  float* prob_w = nullptr;  // device [kd][kh][kw][c]
  void* prob_pack = nullptr;  // bf16, base 8: prob_mfma_kernel's A operand (weight_pack.h pack_prob_rows)
  void* prob_split = nullptr;  // fp32, base 8: the same rows as split-f16 pairs (prob_mfma_kernel<float>)
  float prob_scale = 1.f;      // 2^-k of prob_split
  float k1[32] = {0};
  float s1 = 0, t1 = 0, s2 = 0, t2 = 0;
};

namespace {

// Weight packing is host arithmetic in weight_pack.h; this unit validates, uploads what it returns and launches.
int fold_bn(const damvs_bn& bn, int c, std::vector<float>& scale, std::vector<float>& shift) {
  if (!bn.weight || !bn.bias || !bn.running_mean || !bn.running_var) return fail(DAMVS_E_ARG, "null BatchNorm tensor");
  bn_affine(bn, c, scale, shift);
  return DAMVS_OK;
}

int upload(const void* host, size_t bytes, void** dev) {
  if (hipMalloc(dev, bytes) != hipSuccess) return fail(DAMVS_E_NOMEM, "hipMalloc(%zu) failed", bytes);
  return hip_check(hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice), "hipMemcpy H2D");
}
// a packing of weight_pack.h, when the layer has it (*dev stays null otherwise)
template <typename T, typename D>
int upload(const std::vector<T>& v, D** dev) {
  return v.empty() ? DAMVS_OK : upload(v.data(), v.size() * sizeof(T), reinterpret_cast<void**>(dev));
}

struct Shapes {
  int D[4], H[4], W[4];  // level 0 (full), 1 (/2), 2 (/4), 3 (/8)
};

Shapes level_shapes(int D, int h, int w) {
  Shapes s;
  for (int l = 0; l < 4; ++l) {
    s.D[l] = D >> l;
    s.H[l] = h >> l;
    s.W[l] = w >> l;
  }
  return s;
}

struct Workspace {
  size_t status, amax, rt, feat, vol, c[7], logits, total;
};

// Magnitude slots of the fp32 stage's activation tensors (damvs_device.h prescale_of): the volume, conv0..conv6
// outputs, conv7 / conv9 outputs after their in-place skip adds (c4', c2'). conv11's output feeds the exact-fp32 VALU
// prob conv and needs none. Per tensor B slots of kAmaxSlotBytes (one per batch element), zeroed at the start of every
// stage forward.
enum { AM_VOL = 0, AM_C0 = 1, AM_C4S = 8, AM_C2S = 9, AM_SLOTS = 10 };
constexpr size_t kAmaxSlotBytes = (size_t)kAmaxSlotWords * 4;
static_assert(kAmaxSlotBytes == DAMVS_AMAX_SLOT_BYTES, "damvs.h slot size");

// c[i] holds conv_i's output for i = 0..6 (conv7/9/11 accumulate in place into c4/c2/c0).
// Channel-blocked copies of the feature maps ([B][C/E][h][w][E], one 16-byte chunk per plane) for the one-lane warp
// kernel's gathers when a pixel is wider than 32 bytes. 32-, 64- and 128-byte pixels (bf16 C 16 / 32, fp32 C 8 / 16 /
// 32) go to the channel-split warp when the view pipeline takes the view count (odd N >= 3): S = 2 / 4 / 8 lanes read a
// corner's whole pixel record in one instruction from the NHWC maps in place, no repack launch. Where the one-lane
// kernel gathers them instead (even N, DAMVS_WARP_SPLIT=0) pixels wider than 32 bytes are blocked as well: stage 1 at
// N = 6, cfgC B = 4, unblocked against blocked, fp32 (128-byte pixels) 8.44 against 3.62 ms, bf16 (64-byte) 2.04
// against 1.58 ms; at N = 5 the split kernel on NHWC maps wins, fp32 2.05 against 2.38 ms (bf16 1.40 against 1.34 ms
// before the 0.17 ms repack launch it saves; profiles/r05/ab_warp_layout_r05p.txt). damvs_warp_feat_blocked_n exports
// the decision (engine.warp_blocked asks it, so Python and the stage forward always agree).
bool feat_blocked(int dtype, int C, int N) {
  const int bytes = C * (dtype == DAMVS_BF16 ? 2 : 4);
  return bytes > 32 && !warp_split_for(bytes, N);
}
bool feat_needs_blocking(const damvs_stage* st, int N) { return feat_blocked(st->dtype, st->C, N); }

Workspace plan_ws(const damvs_stage* st, int B, int N, int D, int h, int w) {
  const size_t es = st->dtype == DAMVS_BF16 ? 2 : 4;
  const size_t V = (size_t)B * D * h * w;
  const int b = st->base;
  const size_t sz[7] = {V * b, V / 8 * 2 * b, V / 8 * 2 * b, V / 64 * 4 * b, V / 64 * 4 * b, V / 512 * 8 * b,
                        V / 512 * 8 * b};
  Workspace ws;
  size_t o = 0;
  ws.status = o;  // the range status word at offset 0 (damvs_stage_status needs no shape)
  o += align_up(4);
  ws.amax = o;  // fp32: the magnitude slots of the stage's activation tensors
  if (st->dtype == DAMVS_F32) o += align_up(AM_SLOTS * (size_t)B * kAmaxSlotBytes);
  ws.rt = o;
  o += align_up((size_t)B * (N > 1 ? N - 1 : 1) * 12 * 4);
  ws.feat = o;  // channel-blocked copies of the N feature maps (only when C spans several 16-B chunks)
  if (feat_needs_blocking(st, N)) o += (size_t)N * align_up((size_t)B * h * w * st->C * es);
  ws.vol = o;
  o += align_up(V * st->C * es);
  for (int i = 0; i < 7; ++i) {
    ws.c[i] = o;
    o += align_up(sz[i] * es);
  }
  ws.logits = o;
  o += align_up(V * 4);
  ws.total = o;
  return ws;
}

int check_stage_shape(const damvs_stage* st, int B, int N, int D, int h, int w) {
  if (B < 1 || N < 2 || N > kMaxViews) return fail(DAMVS_E_SHAPE, "need B >= 1 and 2 <= N <= %d (got B=%d N=%d)", kMaxViews, B, N);
  if (D < 8 || h < 8 || w < 8 || D % 8 || h % 8 || w % 8)
    return fail(DAMVS_E_SHAPE, "D, h, w must be positive multiples of 8 (got D=%d h=%d w=%d)", D, h, w);
  (void)st;
  return DAMVS_OK;
}

ConvArgs conv_args(const damvs_stage* st, int li, int B, const Shapes& S, int lin, int lout, const void* in, void* out,
                   const void* resid) {
  const LayerPlan& P = st->L[li];
  ConvArgs a;
  std::memset(&a, 0, sizeof(a));
  a.in = in;
  a.out = out;
  a.resid = resid;
  a.wpack = P.wpack;
  a.wpack_pair = P.wpack_pair;
  a.wpack32 = P.wpack32;
  a.wgat32 = P.wgat32;
  std::memcpy(a.k32_chunks, P.k32_chunks, sizeof(a.k32_chunks));
  std::memcpy(a.k32_off, P.k32_off, sizeof(a.k32_off));
  a.bias = P.bias;
  a.B = B;
  a.Cin = P.cin;
  a.Cout = P.cout;
  a.MT = P.mt;
  a.Di = S.D[lin]; a.Hi = S.H[lin]; a.Wi = S.W[lin];
  a.Do = S.D[lout]; a.Ho = S.H[lout]; a.Wo = S.W[lout];
  if (P.kind == DECONV_S2) {  // iterate over the input grid, one phase per output parity
    a.Dq = a.Di; a.Hq = a.Hi; a.Wq = a.Wi;
    a.in_stride = 1;
    a.out_stride = 2;
  } else {
    a.Dq = a.Do; a.Hq = a.Ho; a.Wq = a.Wo;
    a.in_stride = P.kind == CONV_S2 ? 2 : 1;
    a.out_stride = 1;
  }
  a.relu = 1;
  a.wscale = P.wscale;
  a.nphase = P.nphase;
  std::memcpy(a.ph, P.ph, sizeof(a.ph));
  if (P.kind == DECONV_S2 && P.wpack_pair && P.cout == 8) {
    a.xpair = 1;
    a.wpack = P.wpack_pair;
    a.nphase = P.nphase_pair;
    std::memset(a.ph, 0, sizeof(a.ph));
    std::memcpy(a.ph, P.ph_pair, sizeof(P.ph_pair));
  }
  return a;
}

// layer i's input / output magnitude slots (-1: none): conv0 reads the volume's, convN writes c_N's, conv7 / conv9 write
// the skip sums c4' / c2' that conv9 / conv11 read
constexpr int kLayerSlots[10][2] = {{AM_VOL, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 5}, {5, 6}, {6, 7}, {7, AM_C4S},
                                    {AM_C4S, AM_C2S}, {AM_C2S, -1}};
void set_slots(ConvArgs& a, const damvs_stage* st, char* amax, int layer, int B) {
  if (st->dtype != DAMVS_F32 || !amax) return;
  const size_t per = (size_t)B * kAmaxSlotBytes;  // a tensor's B slots
  a.in_amax = reinterpret_cast<const unsigned*>(amax + kLayerSlots[layer][0] * per);
  a.out_amax = kLayerSlots[layer][1] < 0 ? nullptr : reinterpret_cast<unsigned*>(amax + kLayerSlots[layer][1] * per);
}

// U-Net through conv11 (+conv0 skip): the prob conv input ends in c[0]. fp32: the slots at ws + W.amax must hold the
// volume's magnitude (and zeros for the rest) on entry.
int run_unet(const damvs_stage* st, hipStream_t s, int B, int D, int h, int w, const void* vol, char* ws,
             const Workspace& W, int nlayers = 10) {
  const Shapes S = level_shapes(D, h, w);
  void* c[7];
  for (int i = 0; i < 7; ++i) c[i] = ws + W.c[i];
  // (layer, in level, out level, input, output, skip)
  struct Step { int li, lin, lout; const void* in; void* out; const void* res; };
  const Step steps[10] = {
      {0, 0, 0, vol, c[0], nullptr},  {1, 0, 1, c[0], c[1], nullptr}, {2, 1, 1, c[1], c[2], nullptr},
      {3, 1, 2, c[2], c[3], nullptr}, {4, 2, 2, c[3], c[4], nullptr}, {5, 2, 3, c[4], c[5], nullptr},
      {6, 3, 3, c[5], c[6], nullptr}, {7, 3, 2, c[6], c[4], c[4]},    {8, 2, 1, c[4], c[2], c[2]},
      {9, 1, 0, c[2], c[0], c[0]}};
  for (int i = 0; i < nlayers; ++i) {
    const Step& k = steps[i];
    ConvArgs a = conv_args(st, k.li, B, S, k.lin, k.lout, k.in, k.out, k.res);
    set_slots(a, st, ws + W.amax, k.li, B);
    DAMVS_TRY(hip_check(launch_conv3d(s, st->dtype, a), "conv3d launch"));
  }
  return DAMVS_OK;
}

WarpArgs warp_args(const damvs_stage* st, int B, int N, int C, int D, int h, int w, const void* const* feats,
                   const float* rt, const float* hyps, void* out) {
  WarpArgs a;
  std::memset(&a, 0, sizeof(a));
  for (int v = 0; v < N; ++v) a.feats[v] = feats[v];
  a.rt = rt;
  a.hyps = hyps;
  a.out = out;
  a.B = B; a.N = N; a.C = C; a.D = D; a.h = h; a.w = w;
  a.y0 = 0;
  a.rows = h;
  a.out_rows = h;
  a.out_y = 0;
  if (st) {
    std::memcpy(a.k1, st->k1, sizeof(a.k1));
    a.s1 = st->s1; a.t1 = st->t1; a.s2 = st->s2; a.t2 = st->t2;
  }
  return a;
}

// Prob conv (models/module.py:541) + softmax regression, confidence and exp-variance
// (models/cas_mvsnet.py:105-124) on the U-Net output c0 [B][D][h][w][base].
int regress_tail(const damvs_stage* st, hipStream_t s, int B, int D, int h, int w, const void* feat, const float* hyps,
                 const float* prob_init, float* logits, float* depth, float* conf, float* var, float* prob) {
  // base 8: the stage's MFMA packing for its storage type (fp32: split-f16 rows and their 2^-k); k_regress.hip routes
  const bool bf16 = st->dtype == DAMVS_BF16;
  const TailArgs a = {B, st->base, D, h, w, feat, st->prob_w, bf16 ? st->prob_pack : st->prob_split,
                      bf16 ? 1.f : st->prob_scale, prob_init, hyps, logits, depth, conf, var, prob};
  const char* what = nullptr;
  const hipError_t e = launch_tail(s, st->dtype, a, &what);
  if (e != hipSuccess && !what) return fail(DAMVS_E_WORKSPACE, "this D needs the logits scratch buffer");
  return hip_check(e, what);
}

// U-Net layer i (conv0..conv6, conv7, conv9, conv11): (input level, output level)
constexpr int kLayerLevels[10][2] = {{0, 0}, {0, 1}, {1, 1}, {1, 2}, {2, 2}, {2, 3}, {3, 3}, {3, 2}, {2, 1}, {1, 0}};

}  // namespace

extern "C" {

int damvs_abi_version(void) { return DAMVS_ABI_VERSION; }

#ifndef DAMVS_BUILD_ID
#define DAMVS_BUILD_ID "unstamped"
#endif
// The stamp of this library when the libraries loaded beside it (libdamvs_fusion.so, libdamvs_cloud.so, libdamvs_scene.so,
// libdamvs_inputs.so, libdamvs_features.so, libdamvs_thin.so, libdamvs_normals.so, libdamvs_consensus.so) carry the same one; otherwise theirs too, so that a loader comparing the id with the hash of the sources refuses a stale or foreign set.
const char* damvs_build_id(void) {
  static const std::string id = [] {
    std::string s(DAMVS_BUILD_ID);
    const std::pair<const char*, const char*> side[] = {{"libdamvs_fusion.so", fusion_static_build_id()},
                                                        {"libdamvs_cloud.so", fusion_cloud_build_id()},
                                                        {"libdamvs_scene.so", scene_build_id()},
                                                        {"libdamvs_inputs.so", inputs_build_id()},
                                                        {"libdamvs_features.so", features_build_id()},
                                                        {"libdamvs_thin.so", thin_build_id()},
                                                        {"libdamvs_normals.so", normals_build_id()},
                                                        {"libdamvs_consensus.so", consensus_build_id()}};
    for (const auto& l : side)
      if (std::strcmp(l.second, DAMVS_BUILD_ID) != 0) s += std::string(" (") + l.first + ": " + l.second + ")";
    return s;
  }();
  return id.c_str();
}

const char* damvs_last_error_string(void) { return g_err.c_str(); }

int damvs_stage_create(const damvs_costreg_params* cr, const damvs_aggweight_params* aw, int agg_mode, int dtype,
                       damvs_stage** out) {
  if (!cr || !out) return fail(DAMVS_E_ARG, "null argument");
  if (dtype != DAMVS_F32 && dtype != DAMVS_BF16) return fail(DAMVS_E_DTYPE, "dtype %d unsupported", dtype);
  if (agg_mode != DAMVS_AGG_ADAPTIVE && agg_mode != DAMVS_AGG_VARIANCE) return fail(DAMVS_E_ARG, "agg_mode %d", agg_mode);
  if (agg_mode == DAMVS_AGG_ADAPTIVE && !aw) return fail(DAMVS_E_ARG, "adaptive aggregation needs weight-net params");
  const int C = cr->in_channels, b = cr->base_channels;
  if (C != 8 && C != 16 && C != 32) return fail(DAMVS_E_SHAPE, "in_channels %d not in {8,16,32}", C);
  if (b != 8 && b != 16) return fail(DAMVS_E_SHAPE, "base_channels %d not in {8,16}", b);
  if (aw && aw->in_channels != C) return fail(DAMVS_E_SHAPE, "weight-net channels %d != %d", aw->in_channels, C);
  for (int i = 0; i < 10; ++i)
    if (!cr->conv_weight[i]) return fail(DAMVS_E_ARG, "null conv weight %d", i);
  if (!cr->prob_weight) return fail(DAMVS_E_ARG, "null prob weight");

  damvs_stage* st = new damvs_stage();
  st->C = C;
  st->base = b;
  st->mode = agg_mode;
  st->dtype = dtype;
  (void)hipGetDevice(&st->device);
  // (cin, cout, kind) of conv0..conv6, conv7, conv9, conv11
  const int spec[10][3] = {{C, b, CONV_S1},         {b, 2 * b, CONV_S2},     {2 * b, 2 * b, CONV_S1},
                           {2 * b, 4 * b, CONV_S2}, {4 * b, 4 * b, CONV_S1}, {4 * b, 8 * b, CONV_S2},
                           {8 * b, 8 * b, CONV_S1}, {8 * b, 4 * b, DECONV_S2}, {4 * b, 2 * b, DECONV_S2},
                           {2 * b, b, DECONV_S2}};
  int rc = DAMVS_OK;
  for (int li = 0; li < 10 && rc == DAMVS_OK; ++li) {
    LayerPlan& P = st->L[li];
    P.cin = spec[li][0];
    P.cout = spec[li][1];
    P.kind = spec[li][2];
    std::vector<float> scale, shift;
    rc = fold_bn(cr->bn[li], P.cout, scale, shift);
    if (rc != DAMVS_OK) break;
    // normalise to wf[co][ci][27] with BN scale folded in
    std::vector<float> wf((size_t)P.cout * P.cin * 27);
    const float* W = cr->conv_weight[li];
    for (int co = 0; co < P.cout; ++co)
      for (int ci = 0; ci < P.cin; ++ci)
        for (int t = 0; t < 27; ++t) {
          const float v = P.kind == DECONV_S2 ? W[((size_t)ci * P.cout + co) * 27 + t] : W[((size_t)co * P.cin + ci) * 27 + t];
          wf[((size_t)co * P.cin + ci) * 27 + t] = v * scale[co];
        }
    const CostregPack k = pack_costreg_layer(P.cin, P.cout, P.kind, dtype, wf);
    P.mt = k.mt; P.wscale = k.wscale; P.nphase = k.ph.n; P.nphase_pair = k.ph_pair.n;
    std::memcpy(P.ph, k.ph.ph, sizeof(P.ph));
    std::memcpy(P.ph_pair, k.ph_pair.ph, sizeof(P.ph_pair));
    std::memcpy(P.k32_chunks, k.k32_chunks, sizeof(P.k32_chunks));
    std::memcpy(P.k32_off, k.k32_off, sizeof(P.k32_off));
    rc = upload(k.wpack, &P.wpack);
    if (rc == DAMVS_OK) rc = upload(k.wpack_pair, &P.wpack_pair);
    if (rc == DAMVS_OK) rc = upload(k.wpack32, &P.wpack32);
    if (rc == DAMVS_OK) rc = upload(k.wgat32, &P.wgat32);
    if (rc == DAMVS_OK && k.wgat32_is_wpack32) P.wgat32 = P.wpack32;
    if (rc == DAMVS_OK) rc = upload(shift, &P.bias);
  }
  if (rc == DAMVS_OK) {
    std::vector<float> pw((size_t)27 * b);  // [kd][kh][kw][c] from [1][c][kd][kh][kw]
    for (int c = 0; c < b; ++c)
      for (int t = 0; t < 27; ++t) pw[(size_t)t * b + c] = cr->prob_weight[(size_t)c * 27 + t];
    rc = upload(pw, &st->prob_w);
  }
  if (rc == DAMVS_OK && b == 8) {  // prob_mfma_kernel's A operand in the stage's storage type
    const ProbRows pr = pack_prob_rows(cr->prob_weight, dtype, kProbRowChunks, kProbRowTerms);
    st->prob_scale = pr.scale;
    rc = upload(pr.rows, dtype == DAMVS_BF16 ? &st->prob_pack : &st->prob_split);
  }
  if (rc == DAMVS_OK && agg_mode == DAMVS_AGG_ADAPTIVE) {
    std::vector<float> sc1, sh1, sc2, sh2;
    rc = fold_bn(aw->bn1, 1, sc1, sh1);
    if (rc == DAMVS_OK) rc = fold_bn(aw->bn2, 1, sc2, sh2);
    if (rc == DAMVS_OK) {
      if (!aw->w1 || !aw->w2) {
        rc = fail(DAMVS_E_ARG, "null weight-net conv");
      } else {
        for (int c = 0; c < C; ++c) st->k1[c] = aw->w1[c];
        st->s1 = sc1[0];
        st->t1 = sh1[0];
        st->s2 = aw->w2[0] * sc2[0];
        st->t2 = sh2[0];
      }
    }
  }
  if (rc != DAMVS_OK) {
    damvs_stage_destroy(st);
    return rc;
  }
  *out = st;
  return DAMVS_OK;
}

int damvs_stage_destroy(damvs_stage* st) {
  if (!st) return DAMVS_OK;
  for (auto& P : st->L) {
    if (P.wpack) (void)hipFree(P.wpack);
    if (P.wpack_pair) (void)hipFree(P.wpack_pair);
    if (P.wgat32 && P.wgat32 != P.wpack32) (void)hipFree(P.wgat32);
    if (P.wpack32) (void)hipFree(P.wpack32);
    if (P.bias) (void)hipFree(P.bias);
  }
  if (st->prob_w) (void)hipFree(st->prob_w);
  if (st->prob_pack) (void)hipFree(st->prob_pack);
  if (st->prob_split) (void)hipFree(st->prob_split);
  delete st;
  return DAMVS_OK;
}

int damvs_stage_workspace_size(const damvs_stage* st, int B, int N, int D, int h, int w, size_t* bytes) {
  if (!st || !bytes) return fail(DAMVS_E_ARG, "null argument");
  DAMVS_TRY(check_stage_shape(st, B, N, D, h, w));
  *bytes = plan_ws(st, B, N, D, h, w).total;
  return DAMVS_OK;
}

int damvs_stage_forward(const damvs_stage* st, void* stream, int B, int N, int D, int h, int w,
                        const void* const* feats, const float* proj, const float* hyps, const float* prob_init,
                        void* workspace, size_t workspace_bytes, float* depth, float* conf, float* var,
                        float* prob) {
  return damvs_stage_forward_probed(st, stream, B, N, D, h, w, feats, proj, hyps, prob_init, workspace, workspace_bytes,
                                    depth, conf, var, prob, nullptr);
}

int damvs_stage_forward_probed(const damvs_stage* st, void* stream, int B, int N, int D, int h, int w,
                               const void* const* feats, const float* proj, const float* hyps, const float* prob_init,
                               void* workspace, size_t workspace_bytes, float* depth, float* conf, float* var,
                               float* prob, void* const* events) {
  if (!st || !feats || !proj || !hyps || !workspace || !depth || !conf || !var) return fail(DAMVS_E_ARG, "null argument");
  DAMVS_TRY(check_stage_shape(st, B, N, D, h, w));
  for (int v = 0; v < N; ++v)
    if (!feats[v]) return fail(DAMVS_E_ARG, "null feature pointer for view %d", v);
  const Workspace W = plan_ws(st, B, N, D, h, w);
  if (workspace_bytes < W.total) return fail(DAMVS_E_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, W.total);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  float* rt = reinterpret_cast<float*>(ws + W.rt);
  int* status = reinterpret_cast<int*>(ws + W.status);
  DAMVS_TRY(hip_check(launch_proj_prepare(s, B, N, proj, rt), "proj_prepare launch"));
  const bool blk = feat_needs_blocking(st, N);
  const void* fv[kMaxViews];
  for (int v = 0; v < N; ++v) fv[v] = feats[v];
  if (blk) {  // repack to [B][C/E][h][w][E]: halves the cache lines each gather instruction touches
    FeatPtrs src, dst;
    const size_t per = align_up((size_t)B * h * w * st->C * (st->dtype == DAMVS_BF16 ? 2 : 4));
    for (int v = 0; v < N; ++v) {
      src.p[v] = feats[v];
      dst.p[v] = ws + W.feat + v * per;
      fv[v] = dst.p[v];
    }
    DAMVS_TRY(hip_check(launch_block_channels(s, st->dtype, src, dst, N, B, h * w, st->C), "block_channels launch"));
  }
  auto mark = [&](int i) {
    return events && events[i] ? hip_check(hipEventRecord(reinterpret_cast<hipEvent_t>(events[i]), s), "hipEventRecord")
                               : DAMVS_OK;
  };
  WarpArgs wa = warp_args(st, B, N, st->C, D, h, w, fv, rt, hyps, ws + W.vol);
  if (st->dtype == DAMVS_F32) {  // fresh magnitude slots; the warp records the volume's
    DAMVS_TRY(hip_check(hipMemsetAsync(ws + W.amax, 0, AM_SLOTS * (size_t)B * kAmaxSlotBytes, s), "slot clear"));
    wa.out_amax = reinterpret_cast<unsigned*>(ws + W.amax + AM_VOL * (size_t)B * kAmaxSlotBytes);
  }
  DAMVS_TRY(mark(0));
  DAMVS_TRY(hip_check(launch_warp_aggregate(s, st->dtype, st->mode, wa, blk), "warp_aggregate launch"));
  DAMVS_TRY(mark(1));
  DAMVS_TRY(run_unet(st, s, B, D, h, w, ws + W.vol, ws, W));
  DAMVS_TRY(mark(2));
  DAMVS_TRY(regress_tail(st, s, B, D, h, w, ws + W.c[0], hyps, prob_init, reinterpret_cast<float*>(ws + W.logits), depth,
                         conf, var, prob));
  DAMVS_TRY(mark(3));
  // range check of the outputs (sticky status word, damvs_stage_status), after the last probe: not in the regression's time
  return hip_check(launch_finite_check(s, depth, conf, var, (long long)B * h * w, status), "finite check launch");
}

int damvs_stage_status(const damvs_stage* st, void* stream, const void* workspace, size_t workspace_bytes) {
  if (!st || !workspace) return fail(DAMVS_E_ARG, "null argument");
  if (workspace_bytes < 4) return fail(DAMVS_E_WORKSPACE, "workspace %zu bytes", workspace_bytes);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int v = 0;
  DAMVS_TRY(hip_check(hipMemcpyAsync(&v, workspace, 4, hipMemcpyDeviceToHost, s), "status copy"));
  DAMVS_TRY(hip_check(hipMemsetAsync(const_cast<void*>(workspace), 0, 4, s), "status clear"));
  DAMVS_TRY(hip_check(hipStreamSynchronize(s), "hipStreamSynchronize"));
  if (v != 0)
    return fail(DAMVS_E_RANGE,
                "non-finite depth / confidence / variance in the stage output: an activation beyond the f16 range of "
                "the fp32 path's split-f16 products (|x| >= 65520) or non-finite inputs");
  return DAMVS_OK;
}

int damvs_proj_prepare(void* stream, int B, int N, const float* proj, float* rt) {
  if (!proj || !rt) return fail(DAMVS_E_ARG, "null argument");
  if (B < 1 || N < 2) return fail(DAMVS_E_SHAPE, "need B >= 1, N >= 2");
  return hip_check(launch_proj_prepare(reinterpret_cast<hipStream_t>(stream), B, N, proj, rt), "proj_prepare launch");
}

int damvs_homo_warp(void* stream, int dtype, int B, int C, int D, int h, int w, const void* src, const float* rt,
                    const float* hyps, void* out) {
  if (!src || !rt || !hyps || !out) return fail(DAMVS_E_ARG, "null argument");
  if (dtype != DAMVS_F32 && dtype != DAMVS_BF16) return fail(DAMVS_E_DTYPE, "dtype %d unsupported", dtype);
  if (C != 8 && C != 16 && C != 32) return fail(DAMVS_E_SHAPE, "C %d not in {8,16,32}", C);
  if (B < 1 || D < 1 || h < 2 || w < 2) return fail(DAMVS_E_SHAPE, "bad shape");
  const void* feats[2] = {src, src};
  WarpArgs a = warp_args(nullptr, B, 2, C, D, h, w, feats, rt, hyps, out);
  return hip_check(launch_warp_aggregate(reinterpret_cast<hipStream_t>(stream), dtype, AGG_WARP_ONLY, a, false),
                   "homo_warp launch");
}

int damvs_warp_aggregate(const damvs_stage* st, void* stream, int B, int N, int D, int h, int w,
                         const void* const* feats, int layout, const float* rt, const float* hyps, void* volume) {
  if (!st || !feats || !rt || !hyps || !volume) return fail(DAMVS_E_ARG, "null argument");
  if (B < 1 || N < 2 || N > kMaxViews || D < 1 || h < 2 || w < 2) return fail(DAMVS_E_SHAPE, "bad shape");
  if (layout != DAMVS_LAYOUT_NHWC && layout != DAMVS_LAYOUT_CBLOCK) return fail(DAMVS_E_ARG, "layout %d", layout);
  WarpArgs a = warp_args(st, B, N, st->C, D, h, w, feats, rt, hyps, volume);
  return hip_check(launch_warp_aggregate(reinterpret_cast<hipStream_t>(stream), st->dtype, st->mode, a,
                                         layout == DAMVS_LAYOUT_CBLOCK),
                   "warp_aggregate launch");
}

int damvs_warp_feat_blocked_n(int dtype, int C, int N) {
  if (dtype != DAMVS_F32 && dtype != DAMVS_BF16) return fail(DAMVS_E_DTYPE, "dtype %d unsupported", dtype);
  if (C < 1) return fail(DAMVS_E_SHAPE, "C %d", C);
  if (N < 2 || N > kMaxViews) return fail(DAMVS_E_SHAPE, "N %d", N);
  return feat_blocked(dtype, C, N) ? 1 : 0;
}

int damvs_warp_feat_blocked(int dtype, int C) { return damvs_warp_feat_blocked_n(dtype, C, 5); }

int damvs_block_channels(void* stream, int dtype, int N, int B, int h, int w, int C, const void* const* src,
                         void* const* dst) {
  if (!src || !dst) return fail(DAMVS_E_ARG, "null argument");
  if (dtype != DAMVS_F32 && dtype != DAMVS_BF16) return fail(DAMVS_E_DTYPE, "dtype %d unsupported", dtype);
  const int E = dtype == DAMVS_BF16 ? 8 : 4;
  if (N < 1 || N > kMaxViews || B < 1 || h < 1 || w < 1 || C < E || C % E)
    return fail(DAMVS_E_SHAPE, "bad shape (C must be a multiple of %d)", E);
  FeatPtrs s, d;
  for (int v = 0; v < N; ++v) {
    if (!src[v] || !dst[v]) return fail(DAMVS_E_ARG, "null feature pointer for map %d", v);
    s.p[v] = src[v];
    d.p[v] = dst[v];
  }
  return hip_check(launch_block_channels(reinterpret_cast<hipStream_t>(stream), dtype, s, d, N, B, h * w, C),
                   "block_channels launch");
}

int damvs_costreg_logits(const damvs_stage* st, void* stream, int B, int D, int h, int w, const void* volume,
                         void* workspace, size_t workspace_bytes, float* logits) {
  if (!st || !volume || !workspace || !logits) return fail(DAMVS_E_ARG, "null argument");
  DAMVS_TRY(check_stage_shape(st, B, 2, D, h, w));
  const Workspace W = plan_ws(st, B, 2, D, h, w);
  if (workspace_bytes < W.total) return fail(DAMVS_E_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, W.total);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  if (st->dtype == DAMVS_F32) {  // the handed-in volume's magnitude per batch element, measured once
    DAMVS_TRY(hip_check(hipMemsetAsync(ws + W.amax, 0, AM_SLOTS * (size_t)B * kAmaxSlotBytes, s), "slot clear"));
    const long long n = (long long)D * h * w * st->C;
    for (int b = 0; b < B; ++b)
      DAMVS_TRY(hip_check(launch_amax(s, static_cast<const float*>(volume) + b * n, n,
                                      reinterpret_cast<unsigned*>(ws + W.amax + (AM_VOL * (size_t)B + b) * kAmaxSlotBytes)),
                          "amax launch"));
  }
  DAMVS_TRY(run_unet(st, s, B, D, h, w, volume, ws, W));
  return hip_check(launch_prob_conv(s, st->dtype, B, st->base, D, h, w, ws + W.c[0], st->prob_w, nullptr, logits),
                   "prob conv launch");
}

int damvs_costreg_layer(const damvs_stage* st, void* stream, int layer, int B, int D, int h, int w, const void* in,
                        void* out) {
  return damvs_costreg_layer_scaled(st, stream, layer, B, D, h, w, in, out, nullptr, nullptr);
}

int damvs_costreg_layer_scaled(const damvs_stage* st, void* stream, int layer, int B, int D, int h, int w,
                               const void* in, void* out, const void* in_slot, void* out_slot) {
  if (!st || !in || !out) return fail(DAMVS_E_ARG, "null argument");
  if (layer < 0 || layer > 9) return fail(DAMVS_E_ARG, "layer %d not in 0..9", layer);
  DAMVS_TRY(check_stage_shape(st, B, 2, D, h, w));
  const Shapes S = level_shapes(D, h, w);
  const bool deconv = layer >= 7;  // conv7 / conv9 / conv11: relu(deconv) + skip, in place on `out`
  ConvArgs a = conv_args(st, layer, B, S, kLayerLevels[layer][0], kLayerLevels[layer][1], in, out, deconv ? out : nullptr);
  if (st->dtype == DAMVS_F32) {
    a.in_amax = static_cast<const unsigned*>(in_slot);
    a.out_amax = static_cast<unsigned*>(out_slot);
  }
  return hip_check(launch_conv3d(reinterpret_cast<hipStream_t>(stream), st->dtype, a), "conv3d launch");
}

int damvs_tensor_amax(void* stream, const float* x, long long n, void* slot) {
  if (!x || !slot) return fail(DAMVS_E_ARG, "null argument");
  if (n < 0) return fail(DAMVS_E_SHAPE, "n %lld", n);
  return hip_check(launch_amax(reinterpret_cast<hipStream_t>(stream), x, n, static_cast<unsigned*>(slot)), "amax launch");
}

int damvs_stage_regress(const damvs_stage* st, void* stream, int B, int D, int h, int w, const void* c0,
                        const float* hyps, const float* prob_init, float* scratch, float* depth, float* conf, float* var,
                        float* prob) {
  if (!st || !c0 || !hyps || !depth || !conf || !var) return fail(DAMVS_E_ARG, "null argument");
  DAMVS_TRY(check_stage_shape(st, B, 2, D, h, w));
  return regress_tail(st, reinterpret_cast<hipStream_t>(stream), B, D, h, w, c0, hyps, prob_init, scratch, depth, conf,
                      var, prob);
}

int damvs_warp_aggregate_rows(const damvs_stage* st, void* stream, int B, int N, int D, int h, int w, int y0, int rows,
                              int out_rows, int out_y, const void* const* feats, int layout, const float* rt,
                              const float* hyps, void* volume) {
  if (!st || !feats || !rt || !hyps || !volume) return fail(DAMVS_E_ARG, "null argument");
  if (B < 1 || N < 2 || N > kMaxViews || D < 1 || h < 2 || w < 2) return fail(DAMVS_E_SHAPE, "bad shape");
  if (y0 < 0 || rows < 1 || y0 + rows > h) return fail(DAMVS_E_SHAPE, "rows [%d, %d) outside 0..%d", y0, y0 + rows, h);
  if (out_y < 0 || out_y + rows > out_rows)
    return fail(DAMVS_E_SHAPE, "rows [%d, %d) outside the %d-row output planes", out_y, out_y + rows, out_rows);
  if (layout != DAMVS_LAYOUT_NHWC && layout != DAMVS_LAYOUT_CBLOCK) return fail(DAMVS_E_ARG, "layout %d", layout);
  WarpArgs a = warp_args(st, B, N, st->C, D, h, w, feats, rt, hyps, volume);
  a.y0 = y0;
  a.rows = rows;
  a.out_rows = out_rows;
  a.out_y = out_y;
  return hip_check(launch_warp_aggregate(reinterpret_cast<hipStream_t>(stream), st->dtype, st->mode, a,
                                         layout == DAMVS_LAYOUT_CBLOCK),
                   "warp_aggregate launch");
}

int damvs_regress(void* stream, int B, int D, int h, int w, const float* logits, const float* hyps,
                  const float* prob_init, float* depth, float* conf, float* var, float* prob) {
  if (!logits || !hyps || !depth || !conf || !var) return fail(DAMVS_E_ARG, "null argument");
  if (prob_init) return fail(DAMVS_E_ARG, "prob_init is applied by damvs_stage_forward; add it to the logits");
  if (B < 1 || D < 1 || h < 1 || w < 1) return fail(DAMVS_E_SHAPE, "bad shape");
  return hip_check(launch_regress(reinterpret_cast<hipStream_t>(stream), B, D, h, w, logits, hyps, depth, conf, var,
                                  prob),
                   "regress launch");
}

int damvs_hypotheses(void* stream, int B, int D, int H, int W, int scale, const float* depth_values, int Dv,
                     const float* prev_depth, const float* prev_var, int hp, int wp, float* hyps) {
  if (!hyps) return fail(DAMVS_E_ARG, "null argument");
  if (B < 1 || D < 2 || H < 1 || W < 1 || scale < 1 || H % scale || W % scale) return fail(DAMVS_E_SHAPE, "bad shape");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (!prev_depth) {
    if (!depth_values || Dv < 2) return fail(DAMVS_E_ARG, "stage 1 needs depth_values with Dv >= 2");
    return hip_check(launch_hyp_linear(s, B, D, H / scale, W / scale, depth_values, Dv, hyps), "hyp_linear launch");
  }
  if (!prev_var) return fail(DAMVS_E_ARG, "refinement needs prev_var");
  if (scale != 1 && scale != 2) return fail(DAMVS_E_SHAPE, "refinement scale must be 1 or 2 (got %d)", scale);
  if (hp < 1 || wp < 1) return fail(DAMVS_E_SHAPE, "bad previous-stage shape");
  return hip_check(launch_hyp_refine(s, B, D, H, W, scale, prev_depth, prev_var, hp, wp, hyps), "hyp_refine launch");
}

int damvs_sparse_depth_pyramid(void* stream, int B, int h, int w, const float* depth, const float* depth_values, int Dv,
                               const float* mask, float* d0, float* d1, float* d2, float* d3, float* scratch) {
  if (!depth || !depth_values || !d0 || !d1 || !d2 || !d3 || !scratch) return fail(DAMVS_E_ARG, "null argument");
  if (B < 1 || h < 8 || w < 8 || Dv < 1) return fail(DAMVS_E_SHAPE, "bad shape (h, w >= 8)");
  if ((long long)B * h * w >= (1ll << 31)) return fail(DAMVS_E_SHAPE, "depth map too large");
  float* m1 = scratch;
  float* m2 = scratch + (size_t)B * (h / 2) * (w / 2);
  return hip_check(launch_sparse_pyramid(reinterpret_cast<hipStream_t>(stream), B, h, w, depth, depth_values, Dv, mask,
                                         d0, d1, d2, d3, m1, m2),
                   "sparse_pool launch");
}

}  // extern "C"

// ============================================================================ 2D convolutions
struct damvs_conv2d {
  damvs_conv2d_desc d;
  int dtype = 0, cout_pad = 0, cout_store = 0, MTtot = 0, nphase = 0, kchunk_k = 0;
  int xpair = 0;  // x-parity-pair phases (weight_pack.h build_phases_2d / XPair2dElem)
  float wscale = 1.f;  // fp32: 2^-k of the split-f16 weights (split_weights)
  Conv2dPhase ph[4];
  void* wpack = nullptr;
  Conv2dPhase ph32[4];      // fp32 layers the wide kernel may take: phases and [hi8 | lo8] weights at 32 K per chunk
  void* wpack32 = nullptr;
  float* wgeo = nullptr;
  float* bias = nullptr;
};

namespace {

void conv2d_out(const damvs_conv2d* L, int Hi, int Wi, int* Ho, int* Wo) {
  const damvs_conv2d_desc& d = L->d;
  if (d.transposed) {
    *Ho = (Hi - 1) * d.stride - 2 * d.padding + d.kernel + d.output_padding;
    *Wo = (Wi - 1) * d.stride - 2 * d.padding + d.kernel + d.output_padding;
  } else {
    *Ho = (Hi + 2 * d.padding - d.kernel) / d.stride + 1;
    *Wo = (Wi + 2 * d.padding - d.kernel) / d.stride + 1;
  }
}

}  // namespace

extern "C" {

int damvs_conv2d_create(const damvs_conv2d_desc* desc, const float* weight, const float* bias, int dtype,
                        damvs_conv2d** out) {
  if (!desc || !weight || !out) return fail(DAMVS_E_ARG, "null argument");
  if (dtype != DAMVS_F32 && dtype != DAMVS_BF16) return fail(DAMVS_E_DTYPE, "dtype %d unsupported", dtype);
  const damvs_conv2d_desc& d = *desc;
  const int E = dtype == DAMVS_BF16 ? 8 : 4;
  if (d.kernel < 1 || d.kernel > 5 || d.stride < 1 || d.stride > 2 || d.cout < 1 || d.cin < 1)
    return fail(DAMVS_E_SHAPE, "kernel %d stride %d cout %d cin %d unsupported", d.kernel, d.stride, d.cout, d.cin);
  if (d.c0 % E || d.c1 % E || d.c0 < 0 || d.c1 < 0 || (d.c0 == 0 && d.c1 > 0))
    return fail(DAMVS_E_SHAPE, "tensor input channels must be multiples of %d", E);
  if (d.ngeo < 0 || d.ngeo > 4 || d.c0 + d.c1 + d.ngeo != d.cin)
    return fail(DAMVS_E_SHAPE, "c0 + c1 + ngeo (%d) != cin (%d)", d.c0 + d.c1 + d.ngeo, d.cin);
  if (d.c0 + d.c1 > 0 && d.ngeo > 1)
    return fail(DAMVS_E_SHAPE, "at most one fp32 plane next to tensor inputs (got %d)", d.ngeo);
  if (d.c0 + d.c1 == 0 && d.cout > 16)
    return fail(DAMVS_E_SHAPE, "plane-only layers support cout <= 16 (got %d)", d.cout);
  const Conv2dPack k = pack_conv2d(d, weight, dtype);
  if (!k.err.empty()) return fail(DAMVS_E_SHAPE, "%s", k.err.c_str());
  damvs_conv2d* L = new damvs_conv2d();
  L->d = d;
  L->dtype = dtype;
  L->kchunk_k = 4 * E;
  L->MTtot = k.MTtot; L->cout_pad = k.cout_pad; L->cout_store = k.cout_store;
  L->xpair = k.xpair; L->nphase = k.nphase; L->wscale = k.wscale;
  std::memcpy(L->ph, k.ph, sizeof(L->ph));
  std::memcpy(L->ph32, k.ph32, sizeof(L->ph32));
  int rc = upload(k.wpack, &L->wpack);
  if (rc == DAMVS_OK) rc = upload(k.wpack32, &L->wpack32);
  if (rc == DAMVS_OK) rc = upload(k.wgeo, &L->wgeo);
  if (rc == DAMVS_OK) {
    std::vector<float> b(L->cout_pad, 0.f);
    if (bias)
      for (int i = 0; i < d.cout; ++i) b[i] = bias[i];
    rc = upload(b, &L->bias);
  }
  if (rc != DAMVS_OK) {
    damvs_conv2d_destroy(L);
    return rc;
  }
  *out = L;
  return DAMVS_OK;
}

int damvs_fpn_top_forward(void* stream, int B, int H, int W, const void* c0, const void* f, const void* apack,
                          const float* bias, void* out) {
  if (!c0 || !f || !apack || !bias || !out) return fail(DAMVS_E_ARG, "null argument");
  if (B < 1 || H < 2 || W < 2 || H % 2 || W % 2) return fail(DAMVS_E_SHAPE, "B %d H %d W %d (H, W even)", B, H, W);
  if ((long long)B * H * W * 16 >= (1ll << 31)) return fail(DAMVS_E_SHAPE, "operands must be smaller than 2 GiB");
  return hip_check(launch_fpn_top(static_cast<hipStream_t>(stream), ST_BF16, B, H, W, c0, f, apack, 1.f, bias, out),
                   "fpn_top launch");
}

int damvs_fpn_top_forward_f32(void* stream, int B, int H, int W, const void* c0, const void* f, const void* apack,
                              float wscale, const float* bias, void* out) {
  if (!c0 || !f || !apack || !bias || !out) return fail(DAMVS_E_ARG, "null argument");
  if (B < 1 || H < 2 || W < 2 || H % 2 || W % 2) return fail(DAMVS_E_SHAPE, "B %d H %d W %d (H, W even)", B, H, W);
  if ((long long)B * H * W * 32 >= (1ll << 31)) return fail(DAMVS_E_SHAPE, "operands must be smaller than 2 GiB");
  if (!(wscale > 0.f)) return fail(DAMVS_E_ARG, "wscale %g", (double)wscale);
  return hip_check(launch_fpn_top(static_cast<hipStream_t>(stream), ST_F32, B, H, W, c0, f, apack, wscale, bias, out),
                   "fpn_top launch");
}

int damvs_conv2d_border_bias(void* stream, int dtype, int B, int H, int W, int cout_stored, int cout, const float* corr,
                             void* out) {
  if (!corr || !out) return fail(DAMVS_E_ARG, "null argument");
  if (dtype != DAMVS_F32 && dtype != DAMVS_BF16) return fail(DAMVS_E_DTYPE, "dtype %d unsupported", dtype);
  if (B < 1 || H < 2 || W < 2 || cout < 1 || cout > 16 || cout_stored < cout)
    return fail(DAMVS_E_SHAPE, "B %d H %d W %d cout %d stored %d unsupported", B, H, W, cout, cout_stored);
  BorderArgs a;
  std::memset(&a, 0, sizeof(a));
  for (int t = 0; t < 9; ++t)
    for (int c = 0; c < cout; ++c) a.corr[t * 16 + c] = corr[t * cout + c];
  return hip_check(launch_border_bias(static_cast<hipStream_t>(stream), dtype == DAMVS_BF16 ? ST_BF16 : ST_F32, a, B, H,
                                      W, cout_stored, cout, out),
                   "border_bias launch");
}

int damvs_conv2d_destroy(damvs_conv2d* L) {
  if (!L) return DAMVS_OK;
  if (L->wpack) (void)hipFree(L->wpack);
  if (L->wpack32) (void)hipFree(L->wpack32);
  if (L->wgeo) (void)hipFree(L->wgeo);
  if (L->bias) (void)hipFree(L->bias);
  delete L;
  return DAMVS_OK;
}

int damvs_conv2d_out_size(const damvs_conv2d* L, int Hi, int Wi, int* Ho, int* Wo, int* cout_stored) {
  if (!L || !Ho || !Wo) return fail(DAMVS_E_ARG, "null argument");
  conv2d_out(L, Hi, Wi, Ho, Wo);
  if (cout_stored) *cout_stored = L->cout_store;
  return DAMVS_OK;
}

// The layer's launch arguments at one size: everything conv2d_route reads (shapes, phases, packings, weights), on top
// of the operand pointers the caller has put into the zeroed `a`. a32: the fp32 layer's 32-K split packing, when it
// has one (L->wpack32). Shared by the forward and the route query, so both route on the same Conv2dArgs.
static int conv2d_args(const damvs_conv2d* L, int B, int Hi, int Wi, Conv2dArgs& a, Conv2dArgs& a32) {
  const damvs_conv2d_desc& d = L->d;
  if (B < 1 || Hi < 1 || Wi < 1) return fail(DAMVS_E_SHAPE, "bad shape");
  a.c0 = d.c0;
  a.c1 = d.c1;
  a.ngeo = d.ngeo;
  a.wpack = L->wpack;
  a.wgeo = L->wgeo;
  a.bias = L->bias;
  if (!a.res_post) a.post_up = 1;
  a.cout = L->cout_store;
  a.cout_pad = L->cout_pad;
  a.MTtot = L->MTtot;
  a.B = B;
  a.Hi = Hi;
  a.Wi = Wi;
  conv2d_out(L, Hi, Wi, &a.Ho, &a.Wo);
  if (a.Ho < 1 || a.Wo < 1) return fail(DAMVS_E_SHAPE, "empty output");
  if (d.transposed) {
    if (a.Ho != d.stride * Hi || a.Wo != d.stride * Wi)
      return fail(DAMVS_E_SHAPE, "transposed conv must produce stride x input size");
    a.Hq = Hi;
    a.Wq = Wi;
    a.in_stride = 1;
    a.out_stride = d.stride;
  } else {
    a.Hq = a.Ho;
    a.Wq = a.Wo;
    a.in_stride = d.stride;
    a.out_stride = 1;
  }
  if (a.res_post && (a.Ho % a.post_up || a.Wo % a.post_up)) return fail(DAMVS_E_SHAPE, "bad upsample shape");
  a.relu = d.relu;
  a.wscale = L->wscale;
  a.nphase = L->nphase;
  a.xpair = L->xpair;
  a.div_wq = make_fastdiv(a.Wq);
  a.div_hq = make_fastdiv(a.Hq);
  std::memcpy(a.ph, L->ph, sizeof(a.ph));
  a32 = a;
  if (L->wpack32) {  // fp32: the same layer on its 32-K split packing (same taps, K chunks of 32)
    std::memcpy(a32.ph, L->ph32, sizeof(a32.ph));
    a32.wpack = L->wpack32;
    a32.wide32 = 1;
  }
  return DAMVS_OK;
}

int damvs_conv2d_forward(const damvs_conv2d* L, void* stream, int B, int Hi, int Wi, const void* in0,
                         const void* in1, const float* const* geo, const long long* geo_batch_stride, const void* res_pre,
                         const void* res_post, int post_up, void* out) {
  if (!L || !out) return fail(DAMVS_E_ARG, "null argument");
  const damvs_conv2d_desc& d = L->d;
  if ((d.c0 > 0 && !in0) || (d.c1 > 0 && !in1)) return fail(DAMVS_E_ARG, "missing tensor input");
  if (d.ngeo > 0 && (!geo || !geo_batch_stride)) return fail(DAMVS_E_ARG, "missing geometry planes");
  if (B < 1 || Hi < 1 || Wi < 1) return fail(DAMVS_E_SHAPE, "bad shape");
  if (res_post && post_up != 1 && post_up != 2) return fail(DAMVS_E_ARG, "post_up must be 1 or 2");
  Conv2dArgs a, a32;
  std::memset(&a, 0, sizeof(a));
  a.in0 = in0;
  a.in1 = in1;
  for (int g = 0; g < d.ngeo; ++g) {
    if (!geo[g]) return fail(DAMVS_E_ARG, "null geometry plane %d", g);
    a.geo[g] = geo[g];
    a.geo_bstride[g] = geo_batch_stride[g];
  }
  a.res_pre = res_pre;
  a.res_post = res_post;
  a.post_up = post_up;
  a.out = out;
  DAMVS_TRY(conv2d_args(L, B, Hi, Wi, a, a32));
  return hip_check(launch_conv2d(reinterpret_cast<hipStream_t>(stream), L->dtype, a, L->wpack32 ? &a32 : nullptr),
                   "conv2d launch");
}

int damvs_conv2d_route(const damvs_conv2d* L, int B, int Hi, int Wi, char* buf, size_t n) {
  if (!L || !buf || n == 0) return fail(DAMVS_E_ARG, "null argument");
  buf[0] = 0;
  Conv2dArgs a, a32;
  std::memset(&a, 0, sizeof(a));
  // the forward's arguments but for the operand pointers, which no router reads; the planes as the front-end passes
  // them: 16-byte aligned, one image apart (the plane-only kernels' vector forms ask for that)
  for (int g = 0; g < L->d.ngeo; ++g) a.geo_bstride[g] = (long long)Hi * Wi;
  DAMVS_TRY(conv2d_args(L, B, Hi, Wi, a, a32));
  Conv2dReport rep = {buf, n, 0};
  if (launch_conv2d(nullptr, L->dtype, a, L->wpack32 ? &a32 : nullptr, &rep) != hipSuccess || rep.len == 0) {
    buf[0] = 0;
    return fail(DAMVS_E_SHAPE, "no conv2d kernel takes this layer at B %d, %d x %d", B, Hi, Wi);
  }
  if (rep.len >= n) return fail(DAMVS_E_ARG, "route buffer of %zu bytes too small for %zu characters", n, rep.len);
  return DAMVS_OK;
}

// ============================================================================ depth fusion
// Validation and camera / pointer packing shared by the two fusion entry points (the thresholds are theirs).
static int fusion_pack(int H, int W, int nsrc, const float* depth_ref, const float* const* depth_src,
                       const float* const* conf, const float* conf_thr, const damvs_fusion_cams* cams, float* depth_avg,
                       unsigned char* mask, float* xyz, FusionArgs& a) {
  if (!depth_ref || !depth_src || !cams || !depth_avg || !mask) return fail(DAMVS_E_ARG, "null argument");
  if (H < 1 || W < 1 || (long long)H * W >= (1LL << 31)) return fail(DAMVS_E_SHAPE, "bad shape %d x %d", H, W);
  if (nsrc < 1 || nsrc > kFusionMaxSrc) return fail(DAMVS_E_SHAPE, "nsrc %d not in [1, %d]", nsrc, kFusionMaxSrc);
  if (conf && (!conf[0] || !conf[1] || !conf[2] || !conf_thr)) return fail(DAMVS_E_ARG, "incomplete confidence maps");
  std::memset(&a, 0, sizeof(a));
  a.H = H;
  a.W = W;
  a.nsrc = nsrc;
  a.depth_ref = depth_ref;
  for (int v = 0; v < nsrc; ++v) {
    if (!depth_src[v]) return fail(DAMVS_E_ARG, "null source depth %d", v);
    a.depth_src[v] = depth_src[v];
    std::memcpy(a.src[v].t_sr, cams->t_sr[v], sizeof(a.src[v].t_sr));
    std::memcpy(a.src[v].k_src, cams->k_src[v], sizeof(a.src[v].k_src));
    std::memcpy(a.src[v].kinv_src, cams->kinv_src[v], sizeof(a.src[v].kinv_src));
    std::memcpy(a.src[v].t_rs, cams->t_rs[v], sizeof(a.src[v].t_rs));
  }
  if (conf)
    for (int i = 0; i < 3; ++i) {
      a.conf[i] = conf[i];
      a.conf_thr[i] = conf_thr[i];
    }
  std::memcpy(a.kinv_ref, cams->kinv_ref, sizeof(a.kinv_ref));
  std::memcpy(a.k_ref, cams->k_ref, sizeof(a.k_ref));
  std::memcpy(a.einv_ref, cams->einv_ref, sizeof(a.einv_ref));
  a.depth_avg = depth_avg;
  a.mask = mask;
  a.xyz = xyz;
  return DAMVS_OK;
}

int damvs_fusion_view(void* stream, int H, int W, int nsrc, const float* depth_ref, const float* const* depth_src,
                      const float* const* conf, const float* conf_thr, const damvs_fusion_cams* cams, double dist_base,
                      double rel_diff_base, float* depth_avg, unsigned char* mask, float* xyz) {
  FusionArgs a;
  DAMVS_TRY(fusion_pack(H, W, nsrc, depth_ref, depth_src, conf, conf_thr, cams, depth_avg, mask, xyz, a));
  for (int i = 2; i <= 10; ++i) {
    a.dist_thr[i - 2] = i * dist_base;
    a.rel_thr[i - 2] = (float)(i * rel_diff_base);
  }
  return hip_check(launch_fusion_view(static_cast<hipStream_t>(stream), a), "fusion_view launch");
}

int damvs_fusion_view_static(void* stream, int H, int W, int nsrc, const float* depth_ref,
                             const float* const* depth_src, const float* const* conf, const float* conf_thr,
                             const damvs_fusion_cams* cams, double dist_thr, double rel_thr, int thres_view,
                             float* depth_avg, unsigned char* mask, float* xyz) {
  FusionArgs a;
  DAMVS_TRY(fusion_pack(H, W, nsrc, depth_ref, depth_src, conf, conf_thr, cams, depth_avg, mask, xyz, a));
  if (thres_view < 1) return fail(DAMVS_E_ARG, "thres_view %d < 1", thres_view);
  // the kernel's 32-bit pixel index must not wrap in the last block of 256
  if ((long long)H * W > (1LL << 31) - 256) return fail(DAMVS_E_SHAPE, "bad shape %d x %d", H, W);
  a.dist_thr[0] = dist_thr;
  a.rel_thr[0] = (float)rel_thr;  // numpy compares the float32 relative difference with the constant in float32
  return hip_check(launch_fusion_view_static(static_cast<hipStream_t>(stream), a, thres_view),
                   "fusion_view_static launch");
}

int damvs_fusion_cloud_scratch(int H, int W) {
  if (H < 1 || W < 1 || (long long)H * W >= (1LL << 31)) return fail(DAMVS_E_SHAPE, "bad shape %d x %d", H, W);
  return fusion_cloud_tiles((long long)H * W) + 2;
}

int damvs_fusion_cloud(void* stream, int H, int W, const unsigned char* mask, const float* xyz, const unsigned char* rgb,
                       unsigned int* scratch, long long scratch_elems, unsigned char* records, long long capacity,
                       unsigned long long* cursor) {
  // records may be null when nothing can be written to it (capacity 0: the call only counts)
  if (!mask || !xyz || !rgb || !scratch || !cursor || (!records && capacity != 0)) return fail(DAMVS_E_ARG, "null argument");
  const int need = damvs_fusion_cloud_scratch(H, W);
  if (need < 0) return need;
  if (scratch_elems < need) return fail(DAMVS_E_ARG, "scratch of %lld elements, %d x %d needs %d", scratch_elems, H, W, need);
  if (capacity < 0) return fail(DAMVS_E_ARG, "capacity %lld < 0", capacity);
  CloudArgs a;
  a.n = (long long)H * W;
  a.ntiles = (unsigned)(need - 2);
  a.mask = mask;
  a.xyz = xyz;
  a.rgb = rgb;
  a.scratch = scratch;
  a.records = records;
  a.capacity = capacity;
  a.cursor = cursor;
  return hip_check(launch_fusion_cloud(static_cast<hipStream_t>(stream), a), "fusion_cloud launch");
}

// ============================================================================ point normals
// Validation and packing shared by the map and the scatter form.
static int normals_pack(int H, int W, const float* depth_avg, const unsigned char* mask, const damvs_fusion_cams* cams,
                        double jump, NormalArgs& a) {
  if (!depth_avg || !mask || !cams) return fail(DAMVS_E_ARG, "null argument");
  // NaN fails the first comparison, +inf the second
  if (!(jump >= 0.0 && jump <= 1.7976931348623157e308)) return fail(DAMVS_E_ARG, "jump %g is not a finite number >= 0", jump);
  if (H < 1 || W < 1 || (long long)H * W >= (1LL << 31)) return fail(DAMVS_E_SHAPE, "bad shape %d x %d", H, W);
  std::memset(&a, 0, sizeof(a));
  a.H = H;
  a.W = W;
  a.n = (long long)H * W;
  a.ntiles = (unsigned)fusion_cloud_tiles(a.n);
  a.depth = depth_avg;
  a.mask = mask;
  std::memcpy(a.kinv, cams->kinv_ref, sizeof(a.kinv));
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) a.rinv[3 * i + j] = cams->einv_ref[4 * i + j];
  a.jump = jump;
  return DAMVS_OK;
}

int damvs_fusion_normals(void* stream, int H, int W, const float* depth_avg, const unsigned char* mask,
                         const damvs_fusion_cams* cams, double jump, float* normals) {
  if (!normals) return fail(DAMVS_E_ARG, "null argument");
  NormalArgs a;
  DAMVS_TRY(normals_pack(H, W, depth_avg, mask, cams, jump, a));
  a.normals = normals;
  return hip_check(launch_normal_map(static_cast<hipStream_t>(stream), a), "fusion_normals launch");
}

int damvs_fusion_cloud_oriented(void* stream, int H, int W, const unsigned char* select, const unsigned char* mask,
                                const float* depth_avg, const damvs_fusion_cams* cams, double jump, const float* xyz,
                                const unsigned char* rgb, unsigned int* scratch, long long scratch_elems,
                                unsigned char* records, long long capacity, unsigned long long* cursor) {
  if (!select || !xyz || !rgb || !scratch || !cursor || (!records && capacity != 0)) return fail(DAMVS_E_ARG, "null argument");
  NormalArgs a;
  DAMVS_TRY(normals_pack(H, W, depth_avg, mask, cams, jump, a));
  if (capacity < 0) return fail(DAMVS_E_ARG, "capacity %lld < 0", capacity);
  // count and scan of damvs_fusion_cloud over `select` (its scatter returns at once at capacity 0): the tile offsets
  // and the cursor's base are then in scratch, and the cursor has advanced
  DAMVS_TRY(damvs_fusion_cloud(stream, H, W, select, xyz, rgb, scratch, scratch_elems, nullptr, 0, cursor));
  a.select = select;
  a.xyz = xyz;
  a.rgb = rgb;
  a.scratch = scratch;
  a.records = records;
  a.capacity = capacity;
  return hip_check(launch_cloud_oriented(static_cast<hipStream_t>(stream), a), "fusion_cloud_oriented launch");
}

// ============================================================================ consensus fusion
static int consensus_shape(int H, int W, int V) {
  if (H < 1 || W < 1 || (long long)H * W >= (1LL << 31)) return fail(DAMVS_E_SHAPE, "bad shape %d x %d", H, W);
  if (V < 1 || V > kConsensusMaxViews) return fail(DAMVS_E_SHAPE, "V %d not in [1, %d]", V, kConsensusMaxViews);
  return DAMVS_OK;
}

int damvs_consensus_table_bytes(int V, size_t* bytes) {
  if (!bytes) return fail(DAMVS_E_ARG, "null argument");
  if (V < 1 || V > kConsensusMaxViews) return fail(DAMVS_E_SHAPE, "V %d not in [1, %d]", V, kConsensusMaxViews);
  *bytes = (size_t)V * sizeof(ConsensusEntry);
  return DAMVS_OK;
}

int damvs_consensus_table(void* stream, int H, int W, int V, const damvs_consensus_cam* cams, const float* const* depth,
                          const float* const* conf, const unsigned char* const* rgb, unsigned char* const* used,
                          void* table) {
  if (!cams || !depth || !conf || !rgb || !used || !table) return fail(DAMVS_E_ARG, "null argument");
  DAMVS_TRY(consensus_shape(H, W, V));
  std::vector<ConsensusEntry> host(V);
  for (int v = 0; v < V; ++v) {
    if (!depth[v] || !conf[v] || !rgb[v] || !used[v]) return fail(DAMVS_E_ARG, "null map of view %d", v);
    for (int w = 0; w < v; ++w)
      if (used[w] == used[v]) return fail(DAMVS_E_ARG, "views %d and %d share a used map", w, v);
    ConsensusEntry& e = host[v];
    std::memcpy(e.k, cams[v].k, sizeof(e.k));
    std::memcpy(e.kinv, cams[v].kinv, sizeof(e.kinv));
    std::memcpy(e.e, cams[v].e, sizeof(e.e));
    std::memcpy(e.einv, cams[v].einv, sizeof(e.einv));
    e.depth = depth[v];
    e.conf = conf[v];
    e.rgb = rgb[v];
    e.used = used[v];
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  DAMVS_TRY(hip_check(hipMemcpyAsync(table, host.data(), host.size() * sizeof(ConsensusEntry), hipMemcpyHostToDevice, s),
                      "consensus table upload"));
  return hip_check(hipStreamSynchronize(s), "consensus table upload");
}

int damvs_consensus_view(void* stream, int H, int W, int V, const void* table, int ref, int nsrc, const int* src,
                         const double* fb, float prob_thr, double disp_thr, int num_consistent, unsigned char* mask,
                         float* xyz, unsigned char* rgb_avg) {
  if (!table || !src || !fb || !mask || !xyz || !rgb_avg) return fail(DAMVS_E_ARG, "null argument");
  DAMVS_TRY(consensus_shape(H, W, V));
  if (nsrc < 1 || nsrc > kConsensusMaxViews - 1)
    return fail(DAMVS_E_SHAPE, "nsrc %d not in [1, %d]", nsrc, kConsensusMaxViews - 1);
  if (ref < 0 || ref >= V) return fail(DAMVS_E_SHAPE, "ref %d not in [0, %d)", ref, V);
  for (int i = 0; i < nsrc; ++i) {
    if (src[i] < 0 || src[i] >= V) return fail(DAMVS_E_SHAPE, "source %d not in [0, %d)", src[i], V);
    if (src[i] == ref) return fail(DAMVS_E_ARG, "ref %d is among the sources", ref);
    for (int j = 0; j < i; ++j)
      if (src[j] == src[i]) return fail(DAMVS_E_ARG, "source %d is listed twice", src[i]);
  }
  if (num_consistent < 1) return fail(DAMVS_E_ARG, "num_consistent %d < 1", num_consistent);
  // NaN fails the first comparison, an infinity one of the two
  if (!(prob_thr >= -3.4028234663852886e38f && prob_thr <= 3.4028234663852886e38f))
    return fail(DAMVS_E_ARG, "prob_thr %g is not finite", (double)prob_thr);
  if (!(disp_thr >= -1.7976931348623157e308 && disp_thr <= 1.7976931348623157e308))
    return fail(DAMVS_E_ARG, "disp_thr %g is not finite", disp_thr);
  ConsensusArgs a;
  std::memset(&a, 0, sizeof(a));
  a.H = H;
  a.W = W;
  a.n = (long long)H * W;
  a.table = static_cast<const ConsensusEntry*>(table);
  a.ref = ref;
  a.nsrc = nsrc;
  a.num_consistent = num_consistent;
  a.prob_thr = prob_thr;
  a.disp_thr = disp_thr;
  a.mask = mask;
  a.xyz = xyz;
  a.rgb_avg = rgb_avg;
  for (int i = 0; i < nsrc; ++i) {
    if (!(fb[i] >= -1.7976931348623157e308 && fb[i] <= 1.7976931348623157e308))
      return fail(DAMVS_E_ARG, "fb[%d] %g is not finite", i, fb[i]);
    a.src[i] = src[i];
    a.fb[i] = fb[i];
  }
  return hip_check(launch_consensus_view(static_cast<hipStream_t>(stream), a), "consensus_view launch");
}

// ============================================================================ scene ingest
int damvs_scene_ingest(void* stream, int B, int H, int W, int V, const float* depth, const float* conf3,
                       const float* conf2, const float* conf1, const float* img, long long img_batch_stride,
                       const int* slots, float* depth_store, float* conf_store, unsigned char* rgb_store) {
  if (!depth || !conf3 || !conf2 || !conf1 || !slots || !depth_store || !conf_store)
    return fail(DAMVS_E_ARG, "null argument");
  if (img && !rgb_store) return fail(DAMVS_E_ARG, "null rgb_store with an image to convert");
  if (B < 1 || B > kSceneMaxBatch) return fail(DAMVS_E_SHAPE, "B %d not in [1, %d]", B, kSceneMaxBatch);
  if (H < 4 || W < 4 || H % 4 || W % 4)
    return fail(DAMVS_E_SHAPE, "H and W must be positive multiples of 4 (got %d x %d)", H, W);
  if (V < 1) return fail(DAMVS_E_SHAPE, "V %d < 1", V);
  if ((long long)H * W * 12 >= (1LL << 31))
    return fail(DAMVS_E_SHAPE, "%d x %d: a view's confidence and colour planes must be smaller than 2 GiB", H, W);
  SceneArgs a;
  for (int b = 0; b < B; ++b) {
    if (slots[b] < 0 || slots[b] >= V) return fail(DAMVS_E_ARG, "slot %d of sample %d outside [0, %d)", slots[b], b, V);
    for (int c = 0; c < b; ++c)
      if (slots[c] == slots[b]) return fail(DAMVS_E_ARG, "slot %d repeated (samples %d and %d)", slots[b], c, b);
    a.slots[b] = slots[b];
  }
  for (int b = B; b < kSceneMaxBatch; ++b) a.slots[b] = 0;
  // the kernel moves 4 pixels per 16-byte access (the stage-2 pair per 8-byte load)
  auto misaligned = [](const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) != 0; };
  if (misaligned(depth, 16) || misaligned(conf3, 16) || misaligned(conf2, 8) || misaligned(conf1, 4) ||
      misaligned(depth_store, 16) || misaligned(conf_store, 16) || misaligned(rgb_store, 4))
    return fail(DAMVS_E_ARG, "misaligned map (16 bytes for the full-size maps and stores, 8 for conf2, 4 for rgb_store)");
  if (img && (misaligned(img, 16) || img_batch_stride % 4))
    return fail(DAMVS_E_ARG, "img must be 16-byte aligned with a batch stride that is a multiple of 4 floats");
  a.H = H;
  a.W = W;
  a.depth = depth;
  a.conf3 = conf3;
  a.conf2 = conf2;
  a.conf1 = conf1;
  a.img = img;
  a.img_bstride = img_batch_stride;
  a.depth_store = depth_store;
  a.conf_store = conf_store;
  a.rgb_store = img ? rgb_store : nullptr;
  return hip_check(launch_scene_ingest(static_cast<hipStream_t>(stream), B, a), "scene_ingest launch");
}

// ============================================================================ scene inputs
int damvs_scene_inputs(void* stream, int n_images, int H0, int W0, int H, int W, int V, const unsigned char* rgb_store,
                       const int* slots, float* out) {
  if (!rgb_store) return fail(DAMVS_E_ARG, "null rgb_store");
  if (!slots) return fail(DAMVS_E_ARG, "null slots");
  if (!out) return fail(DAMVS_E_ARG, "null out");
  if (n_images < 1 || n_images > kInputsMaxImages)
    return fail(DAMVS_E_ARG, "n_images %d not in [1, %d]", n_images, kInputsMaxImages);
  if (H0 < 1 || W0 < 1) return fail(DAMVS_E_ARG, "H0 x W0 = %d x %d: a size below 1", H0, W0);
  if (H < 1 || W < 1) return fail(DAMVS_E_ARG, "H x W = %d x %d: a size below 1", H, W);
  if (V < 1) return fail(DAMVS_E_ARG, "V %d < 1", V);
  if (W % 4) return fail(DAMVS_E_ARG, "W %d is not a multiple of 4", W);
  // the offsets within an image are 32-bit
  if (3LL * H0 * W0 >= (1LL << 31)) return fail(DAMVS_E_ARG, "H0 x W0 = %d x %d: 3 * H0 * W0 >= 2^31", H0, W0);
  if (3LL * H * W >= (1LL << 31)) return fail(DAMVS_E_ARG, "H x W = %d x %d: 3 * H * W >= 2^31", H, W);
  if (reinterpret_cast<uintptr_t>(out) & 15) return fail(DAMVS_E_ARG, "out is not 16-byte aligned");
  InputsArgs a;
  for (int i = 0; i < n_images; ++i) {
    if (slots[i] < 0 || slots[i] >= V) return fail(DAMVS_E_ARG, "slot %d of image %d outside [0, %d)", slots[i], i, V);
    a.slots[i] = slots[i];
  }
  for (int i = n_images; i < kInputsMaxImages; ++i) a.slots[i] = 0;
  a.H0 = H0;
  a.W0 = W0;
  a.H = H;
  a.W = W;
  a.rgb_store = rgb_store;
  a.out = out;
  return hip_check(launch_scene_inputs(static_cast<hipStream_t>(stream), n_images, a), "scene_inputs launch");
}

// ============================================================================ scene features
int damvs_feature_gather(void* stream, int n_pairs, int K, int V, const void* const* stores,
                         const unsigned long long* view_bytes, const int* slots, void* const* outs) {
  if (!stores) return fail(DAMVS_E_ARG, "null stores");
  if (!view_bytes) return fail(DAMVS_E_ARG, "null view_bytes");
  if (!slots) return fail(DAMVS_E_ARG, "null slots");
  if (!outs) return fail(DAMVS_E_ARG, "null outs");
  if (n_pairs < 1 || n_pairs > kFeaturesMaxPairs)
    return fail(DAMVS_E_SHAPE, "n_pairs %d not in [1, %d]", n_pairs, kFeaturesMaxPairs);
  if (K < 1 || K > kFeaturesMaxTensors) return fail(DAMVS_E_SHAPE, "K %d not in [1, %d]", K, kFeaturesMaxTensors);
  if (V < 1) return fail(DAMVS_E_SHAPE, "V %d < 1", V);
  FeaturesArgs a;
  for (int k = 0; k < kFeaturesMaxTensors; ++k) {
    a.store[k] = nullptr;
    a.out[k] = nullptr;
    a.nvec[k] = 0;
  }
  for (int k = 0; k < K; ++k) {
    if (!stores[k]) return fail(DAMVS_E_ARG, "null stores[%d]", k);
    if (!outs[k]) return fail(DAMVS_E_ARG, "null outs[%d]", k);
    // the kernel moves 16-byte vectors
    if (reinterpret_cast<uintptr_t>(stores[k]) & 15) return fail(DAMVS_E_ARG, "stores[%d] is not 16-byte aligned", k);
    if (reinterpret_cast<uintptr_t>(outs[k]) & 15) return fail(DAMVS_E_ARG, "outs[%d] is not 16-byte aligned", k);
    const unsigned long long vb = view_bytes[k];
    if (vb == 0) return fail(DAMVS_E_SHAPE, "view_bytes[%d] is 0", k);
    if (vb % 16) return fail(DAMVS_E_SHAPE, "view_bytes[%d] %llu is not a multiple of 16", k, vb);
    // the offsets within a view are 32-bit
    if (vb >= (1ull << 31)) return fail(DAMVS_E_SHAPE, "view_bytes[%d] %llu >= 2^31", k, vb);
    a.store[k] = static_cast<const unsigned char*>(stores[k]);
    a.out[k] = static_cast<unsigned char*>(outs[k]);
    a.nvec[k] = (unsigned)(vb / 16);
  }
  for (int i = 0; i < n_pairs; ++i) {
    if (slots[i] < 0 || slots[i] >= V) return fail(DAMVS_E_SHAPE, "slot %d of pair %d outside [0, %d)", slots[i], i, V);
    a.slots[i] = slots[i];
  }
  for (int i = n_pairs; i < kFeaturesMaxPairs; ++i) a.slots[i] = 0;
  return hip_check(launch_feature_gather(static_cast<hipStream_t>(stream), n_pairs, K, a), "feature_gather launch");
}

// ============================================================================ voxel thinning
namespace {

// keys[slots], owners[slots], then the status word (8 bytes keep the size a multiple of 8)
int thin_slots_ok(long long slots) {
  if (slots < kThinMinSlots || slots > kThinMaxSlots || (slots & (slots - 1)) != 0)
    return fail(DAMVS_E_ARG, "slots %lld is not a power of two in [%lld, 2^32]", slots, kThinMinSlots);
  return DAMVS_OK;
}

unsigned* thin_status_word(void* table, long long slots) {
  return reinterpret_cast<unsigned*>(static_cast<unsigned char*>(table) + (size_t)slots * 16);
}

}  // namespace

int damvs_cloud_thin_table_bytes(long long slots, size_t* bytes) {
  if (!bytes) return fail(DAMVS_E_ARG, "null bytes");
  DAMVS_TRY(thin_slots_ok(slots));
  *bytes = (size_t)slots * 16 + 8;
  return DAMVS_OK;
}

int damvs_cloud_thin_hash(unsigned long long key, long long slots, long long* slot) {
  if (!slot) return fail(DAMVS_E_ARG, "null slot");
  DAMVS_TRY(thin_slots_ok(slots));
  *slot = (long long)thin_hash(key, (unsigned long long)slots);
  return DAMVS_OK;
}

int damvs_cloud_thin_clear(void* stream, void* table, long long slots) {
  if (!table) return fail(DAMVS_E_ARG, "null table");
  DAMVS_TRY(thin_slots_ok(slots));
  if (reinterpret_cast<uintptr_t>(table) & 7) return fail(DAMVS_E_ARG, "table is not 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  DAMVS_TRY(hip_check(hipMemsetAsync(table, 0xFF, (size_t)slots * 16, s), "table clear"));
  return hip_check(hipMemsetAsync(thin_status_word(table, slots), 0, 8, s), "status clear");
}

int damvs_cloud_thin(void* stream, long long n, const unsigned char* mask, const float* xyz, float inv_voxel,
                     long long base, void* table, long long slots, unsigned char* keep) {
  if (!mask) return fail(DAMVS_E_ARG, "null mask");
  if (!xyz) return fail(DAMVS_E_ARG, "null xyz");
  if (!table) return fail(DAMVS_E_ARG, "null table");
  if (!keep) return fail(DAMVS_E_ARG, "null keep");
  if (n < 1 || n >= (1LL << 31)) return fail(DAMVS_E_SHAPE, "n %lld not in [1, 2^31)", n);
  DAMVS_TRY(thin_slots_ok(slots));
  if (!(inv_voxel > 0.f) || !(inv_voxel <= 3.402823466e38f))
    return fail(DAMVS_E_ARG, "inv_voxel %g is not finite and positive", (double)inv_voxel);
  if (base < 0 || base > (1LL << 62)) return fail(DAMVS_E_ARG, "base %lld not in [0, 2^62]", base);
  if (reinterpret_cast<uintptr_t>(table) & 7) return fail(DAMVS_E_ARG, "table is not 8-byte aligned");
  ThinArgs a;
  a.n = n;
  a.mask = mask;
  a.xyz = xyz;
  a.inv_voxel = inv_voxel;
  a.base = (unsigned long long)base;
  a.keys = static_cast<unsigned long long*>(table);
  a.owners = a.keys + slots;
  a.status = thin_status_word(table, slots);
  a.slots = (unsigned long long)slots;
  a.keep = keep;
  return hip_check(launch_cloud_thin(static_cast<hipStream_t>(stream), a), "cloud_thin launch");
}

int damvs_cloud_thin_status(void* stream, void* table, long long slots) {
  if (!table) return fail(DAMVS_E_ARG, "null table");
  DAMVS_TRY(thin_slots_ok(slots));
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned* word = thin_status_word(table, slots);
  unsigned v = 0;
  DAMVS_TRY(hip_check(hipMemcpyAsync(&v, word, 4, hipMemcpyDeviceToHost, s), "status copy"));
  DAMVS_TRY(hip_check(hipMemsetAsync(word, 0, 4, s), "status clear"));
  DAMVS_TRY(hip_check(hipStreamSynchronize(s), "hipStreamSynchronize"));
  if (v & kThinRange)
    return fail(DAMVS_E_RANGE, "voxel thinning: a selected point is not finite or its cell index lies outside "
                               "[-2^20, 2^20) (out of range%s)", (v & kThinFull) ? "; the table was full as well" : "");
  if (v & kThinFull)
    return fail(DAMVS_E_WORKSPACE, "voxel thinning: the table of %lld slots is full (table full)", slots);
  return DAMVS_OK;
}

}  // extern "C"
