// Host weight packing: BN folding, phase tables, the MFMA A-fragment packer and its storage forms, and the two entry
// points that decide which packings a layer gets. Pure host arithmetic on std::vector; plain C++17 without HIP, so
// tests/test_weight_pack.py compiles this header alone and pins every byte to the packers it replaced. capi.cpp uploads
// what these functions return.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "conv_phases.h"
#include "damvs.h"

namespace damvs {

enum LayerKind { CONV_S1 = 0, CONV_S2 = 1, DECONV_S2 = 2 };

inline uint16_t to_bf16(float f) {  // round to nearest even; NaN stays NaN
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

// BatchNorm in eval form as y = x * scale + shift
inline void bn_affine(const damvs_bn& bn, int c, std::vector<float>& scale, std::vector<float>& shift) {
  scale.resize(c);
  shift.resize(c);
  for (int i = 0; i < c; ++i) {
    const double inv = 1.0 / std::sqrt((double)bn.running_var[i] + (double)bn.eps);
    scale[i] = (float)(inv * bn.weight[i]);
    shift[i] = (float)(bn.bias[i] - bn.running_mean[i] * inv * bn.weight[i]);
  }
}

// ---------------------------------------------------------------- storage forms
// fp32 layers compute on split-f16 MFMAs (damvs_device.h, mma_split16): the per-layer exponent k that puts the largest
// |w| * 2^k in (2^13, 2^14], so every lo piece that matters is a normal f16 (0 for an all-zero layer).
inline int split_exponent(const std::vector<float>& w) {
  float mx = 0.f;
  for (float v : w) mx = std::max(mx, std::fabs(v));
  if (!(mx > 0.f) || !std::isfinite(mx)) return 0;
  int e;
  std::frexp(mx, &e);  // mx = f * 2^e, f in [0.5, 1)
  return 14 - e;
}
// Fragments packed as fp32 -> per block of B values [hi x B | lo x B] f16 of w * 2^k. B = 4: a lane's values of a 16-K
// chunk. B = 512 ("blocked"): the 64 lanes x 8 values of a 32-K (chunk, cout tile) (conv2d_wide_kernel<float>,
// WideForm<float>).
inline std::vector<uint16_t> split_weights(const std::vector<float>& pk, int k, size_t B) {
  std::vector<uint16_t> out(pk.size() * 2);
  for (size_t i = 0; i < pk.size() / B * B; ++i) {
    const float v = std::ldexp(pk[i], k);
    const _Float16 hi = (_Float16)v;
    const _Float16 lo = (_Float16)(v - (float)hi);
    std::memcpy(&out[i / B * 2 * B + i % B], &hi, 2);
    std::memcpy(&out[i / B * 2 * B + B + i % B], &lo, 2);
  }
  return out;
}
// The device form of packed fragments, as 16-bit words: bf16 per value, or for fp32 the split-f16 pairs of w * 2^kexp,
// [hi4 | lo4] per lane (16-K chunks) or blocked per (chunk, tile) (32-K chunks).
inline std::vector<uint16_t> store_form(const std::vector<float>& pk, int dtype, int kexp, bool blocked) {
  if (dtype != DAMVS_BF16) return split_weights(pk, kexp, blocked ? 512 : 4);
  std::vector<uint16_t> out(pk.size());
  std::transform(pk.begin(), pk.end(), out.begin(), to_bf16);
  return out;
}

// ---------------------------------------------------------------- the fragment packer
// Appends nchunks x ntiles A fragments of E values per lane (K per chunk KC = 4 E):
//   element ((s * ntiles + m) * 64 + lane) * E + e  =  elem(tile m, row = lane & 15, k = s*KC + (lane >> 4)*E + e)
template <typename Elem>
void pack_fragments(std::vector<float>& out, int nchunks, int ntiles, int E, const Elem& elem) {
  out.reserve(out.size() + (size_t)nchunks * ntiles * 64 * E);
  for (int s = 0; s < nchunks; ++s)
    for (int m = 0; m < ntiles; ++m)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < E; ++e) out.push_back(elem(m, lane & 15, s * 4 * E + (lane >> 4) * E + e));
}

// ---------------------------------------------------------------- conv3d (CostRegNet)
struct ConvPhases {
  int n = 0;
  ConvPhase ph[kMaxPhases];
  ConvPhases() { std::memset(ph, 0, sizeof(ph)); }
};

// ConvTranspose k3 s2 p1 op1 per dim (o = 2i - 1 + k), output parity p: kDeconvCnt[p] taps, kernel index
// kDeconvK[p][j] at input offset kDeconvOff[p][j]:  p = 0 -> {k=1 at input q},  p = 1 -> {k=0 at q+1, k=2 at q}
constexpr int kDeconvCnt[2] = {1, 2}, kDeconvK[2][2] = {{1, -1}, {0, 2}}, kDeconvOff[2][2] = {{0, 0}, {1, 0}};

// Weight tap lists at kchunk_k K per chunk (w_off stays 0 until pack_phases numbers the fragments it packs).
// Conv: t = kd*9 + kh*3 + kw at input offset k-1 (input = q*stride + k - 1), one phase.
// ConvTranspose: one phase per output parity (pd, ph, pw), 8 in all.
// xpair: ConvTranspose (Cout <= 8) as 4 phases (pz, py) whose 16 MFMA rows are the two x parities
// x 8 channels: x-parity 0 takes kx = 1 at input offset 0, parity 1 takes kx = 2 at offset 0 and
// kx = 0 at offset +1, so both share the input x-offsets {0, +1} (tap[t][2] = dx, tap[t][3] = the
// (kz, ky) part of the weight tap). K per phase = nz * ny * 2 * cin; over the 4 phases 18 * cin
// instead of 27 * cin for the 8 single-parity phases, and no M row is padding.
inline ConvPhases build_phases(int kind, int cin, int kchunk_k, bool xpair) {
  ConvPhases r;
  if (kind != DECONV_S2) {
    r.n = 1;
    ConvPhase& ph = r.ph[0];
    ph.ntaps = 27;
    for (int t = 0; t < 27; ++t) {
      ph.tap[t][0] = (signed char)(t / 9 - 1);
      ph.tap[t][1] = (signed char)((t / 3) % 3 - 1);
      ph.tap[t][2] = (signed char)(t % 3 - 1);
      ph.tap[t][3] = (signed char)t;  // weight tap index
    }
    ph.kchunks = (27 * cin + kchunk_k - 1) / kchunk_k;
    return r;
  }
  r.n = xpair ? 4 : 8;
  const int pair_off[2] = {0, 1}, pair_k[2] = {0, 0};  // xpair's x taps: both offsets, kx left to XPairElem
  for (int p = 0; p < r.n; ++p) {
    ConvPhase& ph = r.ph[p];
    const int q = xpair ? p * 2 : p;
    ph.pd = (q >> 2) & 1;
    ph.ph = (q >> 1) & 1;
    ph.pw = q & 1;
    const int nx = xpair ? 2 : kDeconvCnt[ph.pw];
    const int *xoff = xpair ? pair_off : kDeconvOff[ph.pw], *xk = xpair ? pair_k : kDeconvK[ph.pw];
    int t = 0;
    for (int a = 0; a < kDeconvCnt[ph.pd]; ++a)
      for (int b = 0; b < kDeconvCnt[ph.ph]; ++b)
        for (int c = 0; c < nx; ++c) {
          ph.tap[t][0] = (signed char)kDeconvOff[ph.pd][a];
          ph.tap[t][1] = (signed char)kDeconvOff[ph.ph][b];
          ph.tap[t][2] = (signed char)xoff[c];
          ph.tap[t][3] = (signed char)(kDeconvK[ph.pd][a] * 9 + kDeconvK[ph.ph][b] * 3 + xk[c]);
          ++t;
        }
    ph.ntaps = t;
    ph.kchunks = (t * cin + kchunk_k - 1) / kchunk_k;
  }
  return r;
}

// BN-folded weights wf[co][ci][27] in A-fragment order: W[co = m*16 + row][k], k -> (tap t = k / cin, ci = k % cin),
// zero beyond ntaps / cout.
struct LayerElem {
  const std::vector<float>& wf;
  const ConvPhase& ph;
  int cin, cout;
  float operator()(int m, int row, int k) const {
    const int co = m * 16 + row, t = k / cin, ci = k % cin;
    if (co >= cout || t >= ph.ntaps) return 0.f;
    return wf[((size_t)co * cin + ci) * 27 + (unsigned char)ph.tap[t][3]];
  }
};
// Row-pair packing for a stride-1 layer with cout <= 8: the 16 MFMA rows are (r, co) = output rows
// y + r (r = 0, 1) x 8 channels; K runs over 36 taps (dz, dy' = 0..3, dx) x cin, where dy' is the
// input row relative to y - 1, so row r sees kernel row ky = dy' - r (zero outside 0..2).
struct RowPairElem {
  const std::vector<float>& wf;
  int cin, cout;
  float operator()(int, int row, int k) const {
    const int r = row >> 3, co = row & 7, t2 = k / cin, ci = k % cin;
    const int dz = t2 / 12, dy = (t2 / 3) % 4, dx = t2 % 3, ky = dy - r;
    if (t2 >= 36 || co >= cout || ky < 0 || ky > 2) return 0.f;
    return wf[((size_t)co * cin + ci) * 27 + (dz * 3 + ky) * 3 + dx];
  }
};
// The x-pair phases' rows (x parity px = row >> 3, channel co = row & 7): kx by (px, dx), none for (0, +1).
struct XPairElem {
  const std::vector<float>& wf;
  const ConvPhase& ph;
  int cin, cout;
  float operator()(int, int row, int k) const {
    const int px = row >> 3, co = row & 7, t = k / cin, ci = k % cin;
    if (co >= cout || t >= ph.ntaps) return 0.f;
    for (int j = 0; j < kDeconvCnt[px]; ++j)
      if (kDeconvOff[px][j] == ph.tap[t][2])
        return wf[((size_t)co * cin + ci) * 27 + (unsigned char)ph.tap[t][3] + kDeconvK[px][j]];
    return 0.f;
  }
};

// A table's phases one after the other (LayerElem on ntiles cout tiles, or XPairElem on one); sets each phase's w_off
template <typename Elem>
std::vector<float> pack_phases(ConvPhases& P, const std::vector<float>& wf, int cin, int cout, int ntiles, int E) {
  std::vector<float> pk;
  for (int p = 0; p < P.n; ++p) {
    P.ph[p].w_off = (int)(pk.size() / (64 * E));
    pack_fragments(pk, P.ph[p].kchunks, ntiles, E, Elem{wf, P.ph[p], cin, cout});
  }
  return pk;
}
inline std::vector<float> pack_layer_pair(const std::vector<float>& wf, int cin, int cout, int E) {
  std::vector<float> pk;
  pack_fragments(pk, (36 * cin + 4 * E - 1) / (4 * E), 1, E, RowPairElem{wf, cin, cout});
  return pk;
}

// Every packing of one CostRegNet layer (LayerPlan, capi.cpp), as the 16-bit words to upload; empty = none.
struct CostregPack {
  int mt = 0;
  float wscale = 1.f;           // fp32: 2^-k of the split-f16 weights
  ConvPhases ph, ph_pair;       // of wpack / wpack_pair (ph_pair.n = 0 unless x-pair)
  std::vector<uint16_t> wpack;  // the gather kernel's 16-K fragments
  std::vector<uint16_t> wpack_pair;  // Cout <= 8: row pairs (stride 1) or x-pair phases (deconv)
  std::vector<uint16_t> wpack32;     // fp32: the z-streamed kernel's 32-K blocked form
  std::vector<uint16_t> wgat32;      // fp32: the gather kernel's 32-K blocked form, unless ...
  bool wgat32_is_wpack32 = false;    // ... the z-streamed kernel's plain packing serves both
  int k32_chunks[kMaxPhases] = {0}, k32_off[kMaxPhases] = {0};  // the plain 32-K form's K chunks / weight offsets
};

// wf: BN-folded [cout][cin][27]
inline CostregPack pack_costreg_layer(int cin, int cout, int kind, int dtype, const std::vector<float>& wf) {
  CostregPack r;
  const bool f32 = dtype != DAMVS_BF16;
  const int E = f32 ? 4 : 8;
  r.mt = (cout + 15) / 16;
  if (r.mt == 3) r.mt = 4;
  const int kexp = f32 ? split_exponent(wf) : 0;
  r.wscale = std::ldexp(1.f, -kexp);
  auto form = [&](const std::vector<float>& pk, bool blocked) { return store_form(pk, dtype, kexp, blocked); };
  r.ph = build_phases(kind, cin, 4 * E, false);
  // conv11 (deconv, cout 8) runs on its x-pair packing alone: its 8-phase table stays without fragments or offsets
  if (!(kind == DECONV_S2 && cout == 8)) r.wpack = form(pack_phases<LayerElem>(r.ph, wf, cin, cout, r.mt, E), false);
  if (f32 && cout > 8) {
    // the plain packing at 32 K per chunk: the gather kernel's 32-K form (conv3d_mfma_kernel<float, MT, false, true>:
    // 16x16x32 f16 split products, twice the 16-K form's MFMA rate; conv3, conv5, conv6, conv7 and the tile kernels'
    // fallbacks), which for conv2, conv9 and conv1 is also their z-streamed kernels' operand
    ConvPhases p32 = build_phases(kind, cin, 32, false);
    r.wgat32_is_wpack32 = cout == 16 && ((kind == CONV_S1 && cin == 16) || (kind == DECONV_S2 && cin == 32) ||
                                         (kind == CONV_S2 && cin == 8));
    (r.wgat32_is_wpack32 ? r.wpack32 : r.wgat32) = form(pack_phases<LayerElem>(p32, wf, cin, cout, r.mt, 8), true);
    for (int p = 0; p < p32.n; ++p) r.k32_chunks[p] = p32.ph[p].kchunks, r.k32_off[p] = p32.ph[p].w_off;
  }
  if (kind == DECONV_S2 && cout <= 8) {
    r.ph_pair = build_phases(kind, cin, 4 * E, true);
    r.wpack_pair = form(pack_phases<XPairElem>(r.ph_pair, wf, cin, cout, 1, E), false);
    if (f32 && cin == 16 && cout == 8) {  // conv11's z-streamed kernel (deconv_xpair_zslide<float>)
      ConvPhases x32 = build_phases(kind, cin, 32, true);
      r.wpack32 = form(pack_phases<XPairElem>(x32, wf, cin, cout, 1, 8), true);
    }
  }
  if (kind == CONV_S1 && cout <= 8) {
    r.wpack_pair = form(pack_layer_pair(wf, cin, cout, E), false);
    if (f32) r.wpack32 = form(pack_layer_pair(wf, cin, cout, 8), true);  // conv0's z-streamed kernel (conv3d_zslide_pair)
  }
  return r;
}

// The prob conv (Conv3d(8, 1, k3), models/module.py:530) as prob_mfma_kernel's A operand (k_regress.hip): rows
// m = 4 j + dz (output pixel row j of four, kernel depth dz), K = (voxel slot sl = 3 r + kx of input row r = 0..5,
// channel), entry W[c][dz][ky = r - j][kx] when dz < 3, sl < 18 and 0 <= ky <= 2, else 0.
struct ProbRowElem {
  const float* w;  // [1][8][3][3][3]
  float operator()(int, int row, int k) const {
    const int j = row >> 2, dz = row & 3, sl = k / 8, c = k % 8, r = sl / 3, kx = sl % 3, ky = r - j;
    return dz < 3 && sl < 18 && ky >= 0 && ky <= 2 ? w[(size_t)c * 27 + dz * 9 + ky * 3 + kx] : 0.f;
  }
};
struct ProbRows {
  std::vector<uint16_t> rows;
  float scale = 1.f;  // fp32: 2^-k of the split
};
// bf16: [chunk][term][lane][8], the fp32 weight as `terms` bf16 terms (hi + lo); fp32: split-f16 at 32 K per chunk
// (prob_mfma_kernel<float>) with the exponent of the whole weight tensor
inline ProbRows pack_prob_rows(const float* prob_weight, int dtype, int chunks, int terms) {
  ProbRows r;
  std::vector<float> pf;
  pack_fragments(pf, chunks, 1, 8, ProbRowElem{prob_weight});
  if (dtype != DAMVS_BF16) {
    const int kp = split_exponent(std::vector<float>(prob_weight, prob_weight + 27 * 8));
    r.scale = std::ldexp(1.f, -kp);
    r.rows = store_form(pf, dtype, kp, true);
    return r;
  }
  r.rows.resize(pf.size() * terms);
  const size_t per = 64 * 8;  // values per chunk
  for (size_t i = 0; i < pf.size(); ++i) {
    float v = pf[i];
    for (int t = 0; t < terms; ++t) {
      const uint16_t q = to_bf16(v);
      r.rows[(i / per * terms + t) * per + i % per] = q;
      float qf;
      const uint32_t qb = (uint32_t)q << 16;
      std::memcpy(&qf, &qb, 4);
      v -= qf;  // exact: the remainder of a round-to-nearest bf16 term
    }
  }
  return r;
}

// ---------------------------------------------------------------- conv2d (front end)
// Kernel taps of one dim that reach output parity r of a stride-s transposed conv, k counting up or down:
// those with (r + p - k) % s == 0, at input offset (r + p - k) / s.
inline void deconv_taps(int K, int s, int p, int r, bool k_down, std::vector<int>& off, std::vector<int>& ks) {
  for (int i = 0; i < K; ++i) {
    const int k = k_down ? K - 1 - i : i;
    if (((r + p - k) % s + s) % s == 0) { off.push_back((r + p - k) / s); ks.push_back(k); }
  }
}

// Tap lists into ph[4]; returns the phase count, or 0 with *err set for an unsupported shape.
// Conv: input = q*s + (k - p), one phase. Transposed conv of stride s: one phase per output parity (ry, rx).
// xpair: ConvTranspose2d stride 2 with cout = 8 as 2 phases (output row parity ry): the 16 MFMA rows are
// (output x parity px, channel), and the taps are (input row offsets of ry) x (the union of the input
// x offsets of both parities). A row whose parity does not use an x offset gets zero weights. Per
// output pixel pair this is |offs[ry]| * |union| taps instead of |offs[ry]| * (|offs[0]| + |offs[1]|)
// over two phases with half the MFMA rows empty, and the 16 channels of an x pair are one 32-byte
// store. wtap keeps the ky * K part; XPair2dElem resolves kx per row parity.
inline int build_phases_2d(const damvs_conv2d_desc& d, int kchunk_k, bool xpair, Conv2dPhase* ph, std::string* err) {
  const int K = d.kernel, s = d.stride, p = d.padding, ctot = d.c0 + d.c1;
  std::memset(ph, 0, 4 * sizeof(Conv2dPhase));
  std::vector<int> offs[2], ks[2], xo;  // per parity r; xpair: the union of x offsets over both parities, ascending
  if (!d.transposed) {
    for (int k = 0; k < K; ++k) { offs[0].push_back(k - p); ks[0].push_back(k); }
  } else {
    if (s != 1 && s != 2) return *err = "transposed stride " + std::to_string(s) + " unsupported", 0;
    // taps in ascending input offset: a stride-1 transposed conv then has exactly the tap list of a plain conv
    // (offsets -p .. K-1-p, row-major), so the LDS-tiled 3x3 kernel (lds3_ok) takes the full-resolution decoder
    // layers instead of the gather kernel. The x-pair rows keep ascending k.
    for (int r = 0; r < s; ++r) deconv_taps(K, s, p, r, !xpair, offs[r], ks[r]);
  }
  for (int r = 0; r < 2 && xpair; ++r)
    for (int o : offs[r])
      if (std::find(xo.begin(), xo.end(), o) == xo.end()) xo.push_back(o);
  std::sort(xo.begin(), xo.end());
  const std::vector<int> no_k(xo.size(), 0);  // xpair: wtap keeps ky * K alone
  const int n = xpair ? 2 : d.transposed ? s * s : 1;
  int w_off = 0, g_off = 0;
  for (int i = 0; i < n; ++i) {
    Conv2dPhase& P = ph[i];
    P.py = xpair ? i : d.transposed ? i / s : 0;
    P.px = xpair || !d.transposed ? 0 : i % s;
    const std::vector<int>& xoff = xpair ? xo : offs[P.px], &xk = xpair ? no_k : ks[P.px];
    int t = 0;
    for (size_t a = 0; a < offs[P.py].size(); ++a)
      for (size_t b = 0; b < xoff.size(); ++b) {
        if (t >= 25) return *err = "more than 25 taps per phase", 0;
        P.tap[t][0] = (signed char)offs[P.py][a];
        P.tap[t][1] = (signed char)xoff[b];
        P.wtap[t] = (signed char)(ks[P.py][a] * K + xk[b]);
        ++t;
      }
    P.ntaps = t;
    P.kchunks = ctot > 0 ? (t * ctot + kchunk_k - 1) / kchunk_k : 0;
    P.gchunks = d.ngeo > 0 ? (t * d.ngeo + kchunk_k - 1) / kchunk_k : 0;
    P.w_off = w_off;
    P.g_off = g_off;
    w_off += P.kchunks + P.gchunks;
    g_off += t * d.ngeo;
  }
  return n;
}

inline float wget(const damvs_conv2d_desc& d, const float* W, int co, int wc, int wt) {
  const int KK = d.kernel * d.kernel;
  return d.transposed ? W[((size_t)wc * d.cout + co) * KK + wt] : W[((size_t)co * d.cin + wc) * KK + wt];
}
// the weight input channel of concatenated tensor channel ci
inline int tensor_channel(const damvs_conv2d_desc& d, int ci) {
  return ci < d.c0 ? d.c0_at + ci : d.c1_at + (ci - d.c0);
}

// A phase's tensor-input chunks (K = tap x concatenated channel) or its plane chunks (K = tap x plane)
struct Conv2dElem {
  const damvs_conv2d_desc& d;
  const float* W;
  const Conv2dPhase& P;
  bool plane;
  float operator()(int m, int row, int k) const {
    const int co = m * 16 + row, per = plane ? d.ngeo : d.c0 + d.c1, t = k / per, ci = k % per;
    if (co >= d.cout || t >= P.ntaps) return 0.f;
    return wget(d, W, co, plane ? d.geo_at[ci] : tensor_channel(d, ci), (unsigned char)P.wtap[t]);
  }
};
// A rows = (x parity px = row >> 3, channel co = row & 7); kx from the parity's tap list.
struct XPair2dElem {
  const damvs_conv2d_desc& d;
  const float* W;
  const Conv2dPhase& P;
  std::vector<int> off[2], ks[2];
  XPair2dElem(const damvs_conv2d_desc& d_, const float* W_, const Conv2dPhase& P_) : d(d_), W(W_), P(P_) {
    for (int r = 0; r < 2; ++r) deconv_taps(d.kernel, 2, d.padding, r, false, off[r], ks[r]);
  }
  float operator()(int, int row, int k) const {
    const int px = row >> 3, co = row & 7, ctot = d.c0 + d.c1, t = k / ctot, ci = k % ctot;
    if (co >= d.cout || t >= P.ntaps) return 0.f;
    const auto it = std::find(off[px].begin(), off[px].end(), (int)P.tap[t][1]);
    if (it == off[px].end()) return 0.f;
    return wget(d, W, co, tensor_channel(d, ci), (unsigned char)P.wtap[t] + ks[px][it - off[px].begin()]);
  }
};

inline std::vector<float> pack_2d(const damvs_conv2d_desc& d, const float* W, const Conv2dPhase* ph, int nphase,
                                  int kchunk_k, int ntiles, bool xpair) {
  std::vector<float> pk;
  for (int i = 0; i < nphase; ++i) {
    const Conv2dPhase& P = ph[i];
    if (xpair) pack_fragments(pk, P.kchunks, 1, kchunk_k / 4, XPair2dElem(d, W, P));
    else pack_fragments(pk, P.kchunks, ntiles, kchunk_k / 4, Conv2dElem{d, W, P, false});
    pack_fragments(pk, P.gchunks, ntiles, kchunk_k / 4, Conv2dElem{d, W, P, true});  // none for x-pair
  }
  return pk;
}

// Every packing of one 2D layer (damvs_conv2d, capi.cpp); err non-empty for a shape the phase builder rejects.
struct Conv2dPack {
  std::string err;
  int xpair = 0, MTtot = 0, cout_pad = 0, cout_store = 0, nphase = 0;
  float wscale = 1.f;  // fp32: 2^-k of the split-f16 weights
  Conv2dPhase ph[4], ph32[4];
  std::vector<uint16_t> wpack;
  std::vector<uint16_t> wpack32;  // fp32 layers the 32-K kernels may take: [hi8 | lo8] blocked, phases ph32
  std::vector<float> wgeo;        // plane weights [phase][tap][g][cout_pad]
  Conv2dPack() { std::memset(ph, 0, sizeof(ph)), std::memset(ph32, 0, sizeof(ph32)); }
};

inline Conv2dPack pack_conv2d(const damvs_conv2d_desc& d, const float* weight, int dtype) {
  Conv2dPack r;
  const bool f32 = dtype != DAMVS_BF16;
  const int kc = f32 ? 16 : 32, ctot = d.c0 + d.c1;
  r.MTtot = (d.cout + 15) / 16;
  r.cout_pad = r.MTtot * 16;
  r.cout_store = (d.cout + 3) / 4 * 4;
  r.xpair = d.transposed && d.stride == 2 && d.cout == 8 && d.ngeo == 0 && ctot > 0;
  r.nphase = build_phases_2d(d, kc, r.xpair, r.ph, &r.err);
  if (!r.err.empty()) return r;
  if (ctot + d.ngeo > 0) {
    const std::vector<float> pk = pack_2d(d, weight, r.ph, r.nphase, kc, r.MTtot, r.xpair);
    const int kexp = f32 ? split_exponent(pk) : 0;
    r.wscale = std::ldexp(1.f, -kexp);
    r.wpack = store_form(pk, dtype, kexp, false);
    // the 32-K split form of the wide kernel (conv2d_wide_kernel<float>), of the narrow halo kernel
    // (conv2d_halo_kernel<float, ..., W32>) and of the gather kernel (conv2d_mfma_kernel<float, ..., K32>: channel
    // counts in multiples of 8): phases and weights at 32 K per chunk
    if (f32 && !r.xpair && d.c0 % 8 == 0 && d.c1 % 8 == 0 && ctot >= 8 && d.ngeo <= 1) {
      const int n32 = build_phases_2d(d, 32, false, r.ph32, &r.err);
      if (!r.err.empty()) return r;
      r.wpack32 = store_form(pack_2d(d, weight, r.ph32, n32, 32, r.MTtot, false), dtype, kexp, true);
    }
  }
  for (int i = 0; i < r.nphase && d.ngeo > 0; ++i)
    for (int t = 0; t < r.ph[i].ntaps; ++t)
      for (int g = 0; g < d.ngeo; ++g)
        for (int co = 0; co < r.cout_pad; ++co)
          r.wgeo.push_back(co < d.cout ? wget(d, weight, co, d.geo_at[g], (unsigned char)r.ph[i].wtap[t]) : 0.f);
  return r;
}

}  // namespace damvs
