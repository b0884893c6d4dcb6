"""CPU: the host weight packing (damvsnet_amd/csrc/weight_pack.h: the phase builders, pack_fragments and its element
functors, store_form, pack_costreg_layer, pack_conv2d, pack_prob_rows, bn_affine) produces, bit for bit, what the
packers it replaced produced.

A stand-alone program (its own main, the header alone, no device code) is compiled with the compiler the library is
built with. Namespace `parent` holds the packing code of capi.cpp as it stood before weight_pack.h existed, written out
verbatim (build_phases .. pack_2d_xpair, the split functions, the two prob-row loops, fold_bn's arithmetic), and around
it the selection logic of the two create functions with `upload` keeping the bytes on the host. For every case the
program compares every buffer, every phase table (whole structs), the 32-K chunk tables, the scales' bits and the alias
flag, prints one line per case and stops at the first difference, naming case, buffer and byte offset.

Weights are distinct per element and have full 24-bit significands over four binades, so a permutation cannot cancel,
bf16 rounding is exercised and every f16 lo piece of a weight is non-zero."""
import os
import re
import subprocess

import pytest

from damvsnet_amd import build

PROGRAM = r"""
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include "weight_pack.h"

using damvs::ConvPhase;
using damvs::Conv2dPhase;
using damvs::kMaxPhases;
using damvs::CONV_S1;
using damvs::CONV_S2;
using damvs::DECONV_S2;

typedef std::vector<unsigned char> Bytes;
static std::vector<Bytes*> g_uploads;

// ====================================================================== the parent commit's packing, verbatim
namespace parent {

constexpr int kProbRowChunks = PROB_ROW_CHUNKS, kProbRowTerms = PROB_ROW_TERMS;  // damvs_internal.h
std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

// upload: the bytes stay on the host
int upload(const void* host, size_t bytes, void** dev) {
  const unsigned char* p = static_cast<const unsigned char*>(host);
  g_uploads.push_back(new Bytes(p, p + bytes));
  *dev = g_uploads.back();
  return DAMVS_OK;
}

uint16_t to_bf16(float f) {  // round to nearest even; NaN stays NaN
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

struct LayerPlan {
  int kind = 0, cin = 0, cout = 0, mt = 0, nphase = 0;
  ConvPhase ph[kMaxPhases];
  void* wpack = nullptr;
  void* wpack_pair = nullptr;
  int nphase_pair = 0;
  ConvPhase ph_pair[4];
  float wscale = 1.f;
  void* wpack32 = nullptr;
  void* wgat32 = nullptr;
  int k32_chunks[kMaxPhases] = {0}, k32_off[kMaxPhases] = {0};
};

void build_phases(LayerPlan& P, int kchunk_k) {
  auto kch = [&](int ntaps) { return (ntaps * P.cin + kchunk_k - 1) / kchunk_k; };
  std::memset(P.ph, 0, sizeof(P.ph));
  if (P.kind != DECONV_S2) {
    P.nphase = 1;
    ConvPhase& ph = P.ph[0];
    ph.ntaps = 27;
    for (int t = 0; t < 27; ++t) {
      ph.tap[t][0] = (signed char)(t / 9 - 1);
      ph.tap[t][1] = (signed char)((t / 3) % 3 - 1);
      ph.tap[t][2] = (signed char)(t % 3 - 1);
      ph.tap[t][3] = (signed char)t;  // weight tap index
    }
    ph.kchunks = kch(27);
    return;
  }
  P.nphase = 8;
  const int ks[2][2] = {{1, -1}, {0, 2}};
  const int off[2][2] = {{0, 0}, {1, 0}};
  const int cnt[2] = {1, 2};
  for (int p = 0; p < 8; ++p) {
    ConvPhase& ph = P.ph[p];
    ph.pd = (p >> 2) & 1;
    ph.ph = (p >> 1) & 1;
    ph.pw = p & 1;
    int t = 0;
    for (int a = 0; a < cnt[ph.pd]; ++a)
      for (int b = 0; b < cnt[ph.ph]; ++b)
        for (int c = 0; c < cnt[ph.pw]; ++c) {
          ph.tap[t][0] = (signed char)off[ph.pd][a];
          ph.tap[t][1] = (signed char)off[ph.ph][b];
          ph.tap[t][2] = (signed char)off[ph.pw][c];
          ph.tap[t][3] = (signed char)(ks[ph.pd][a] * 9 + ks[ph.ph][b] * 3 + ks[ph.pw][c]);
          ++t;
        }
    ph.ntaps = t;
    ph.kchunks = kch(t);
  }
}

template <typename S>
void pack_layer(LayerPlan& P, const std::vector<float>& wf, int E, std::vector<S>& out, S (*cvt)(float)) {
  const int KC = 4 * E;
  int w_off = 0;
  for (int p = 0; p < P.nphase; ++p) {
    ConvPhase& ph = P.ph[p];
    ph.w_off = w_off;
    for (int s = 0; s < ph.kchunks; ++s)
      for (int m = 0; m < P.mt; ++m)
        for (int lane = 0; lane < 64; ++lane)
          for (int e = 0; e < E; ++e) {
            const int co = m * 16 + (lane & 15);
            const int k = s * KC + (lane >> 4) * E + e;
            const int t = k / P.cin, ci = k % P.cin;
            float v = 0.f;
            if (co < P.cout && t < ph.ntaps) v = wf[((size_t)co * P.cin + ci) * 27 + (unsigned char)ph.tap[t][3]];
            out.push_back(cvt(v));
          }
    w_off += ph.kchunks * P.mt;
  }
}

template <typename S>
void pack_layer_pair(const LayerPlan& P, const std::vector<float>& wf, int E, std::vector<S>& out, S (*cvt)(float)) {
  const int KC = 4 * E;
  const int nch = (36 * P.cin + KC - 1) / KC;
  for (int s = 0; s < nch; ++s)
    for (int lane = 0; lane < 64; ++lane)
      for (int e = 0; e < E; ++e) {
        const int row = lane & 15, r = row >> 3, co = row & 7;
        const int k = s * KC + (lane >> 4) * E + e;
        const int t2 = k / P.cin, ci = k % P.cin;
        const int dz = t2 / 12, dy = (t2 / 3) % 4, dx = t2 % 3, ky = dy - r;
        float v = 0.f;
        if (t2 < 36 && co < P.cout && ky >= 0 && ky <= 2) v = wf[((size_t)co * P.cin + ci) * 27 + (dz * 3 + ky) * 3 + dx];
        out.push_back(cvt(v));
      }
}

void build_phases_xpair(LayerPlan& P, int kchunk_k) {
  const int ks[2][2] = {{1, -1}, {0, 2}};
  const int off[2][2] = {{0, 0}, {1, 0}};
  const int cnt[2] = {1, 2};
  std::memset(P.ph_pair, 0, sizeof(P.ph_pair));
  P.nphase_pair = 4;
  for (int p = 0; p < 4; ++p) {
    ConvPhase& ph = P.ph_pair[p];
    ph.pd = (p >> 1) & 1;
    ph.ph = p & 1;
    ph.pw = 0;
    int t = 0;
    for (int a = 0; a < cnt[ph.pd]; ++a)
      for (int b = 0; b < cnt[ph.ph]; ++b)
        for (int dx = 0; dx < 2; ++dx) {
          ph.tap[t][0] = (signed char)off[ph.pd][a];
          ph.tap[t][1] = (signed char)off[ph.ph][b];
          ph.tap[t][2] = (signed char)dx;
          ph.tap[t][3] = (signed char)(ks[ph.pd][a] * 9 + ks[ph.ph][b] * 3);  // + kx by (row parity, dx)
          ++t;
        }
    ph.ntaps = t;
    ph.kchunks = (t * P.cin + kchunk_k - 1) / kchunk_k;
  }
}

template <typename S>
void pack_layer_xpair(LayerPlan& P, const std::vector<float>& wf, int E, std::vector<S>& out, S (*cvt)(float)) {
  const int KC = 4 * E;
  const int kx_of[2][2] = {{1, -1}, {2, 0}};  // [x parity][dx]
  int w_off = 0;
  for (int p = 0; p < P.nphase_pair; ++p) {
    ConvPhase& ph = P.ph_pair[p];
    ph.w_off = w_off;
    for (int s = 0; s < ph.kchunks; ++s)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < E; ++e) {
          const int row = lane & 15, px = row >> 3, co = row & 7;
          const int k = s * KC + (lane >> 4) * E + e;
          const int t = k / P.cin, ci = k % P.cin;
          float v = 0.f;
          if (co < P.cout && t < ph.ntaps) {
            const int kx = kx_of[px][(int)ph.tap[t][2]];
            if (kx >= 0) v = wf[((size_t)co * P.cin + ci) * 27 + (unsigned char)ph.tap[t][3] + kx];
          }
          out.push_back(cvt(v));
        }
    w_off += ph.kchunks;
  }
}

float cvt_f32(float v) { return v; }
uint16_t cvt_bf16(float v) { return to_bf16(v); }

int split_exponent(const std::vector<float>& w) {
  float mx = 0.f;
  for (float v : w) mx = std::max(mx, std::fabs(v));
  if (!(mx > 0.f) || !std::isfinite(mx)) return 0;
  int e;
  std::frexp(mx, &e);  // mx = f * 2^e, f in [0.5, 1)
  return 14 - e;
}
std::vector<uint16_t> split_weights(const std::vector<float>& pk, int k) {
  std::vector<uint16_t> out(pk.size() * 2);
  for (size_t q = 0; q < pk.size() / 4; ++q)
    for (int e = 0; e < 4; ++e) {
      const float v = std::ldexp(pk[q * 4 + e], k);
      const _Float16 hi = (_Float16)v;
      const _Float16 lo = (_Float16)(v - (float)hi);
      std::memcpy(&out[q * 8 + e], &hi, 2);
      std::memcpy(&out[q * 8 + 4 + e], &lo, 2);
    }
  return out;
}
std::vector<uint16_t> split_weights_blocked(const std::vector<float>& pk, int k) {
  std::vector<uint16_t> out(pk.size() * 2);
  for (size_t blk = 0; blk < pk.size() / 512; ++blk)
    for (int lane = 0; lane < 64; ++lane)
      for (int e = 0; e < 8; ++e) {
        const float v = std::ldexp(pk[blk * 512 + lane * 8 + e], k);
        const _Float16 hi = (_Float16)v;
        const _Float16 lo = (_Float16)(v - (float)hi);
        std::memcpy(&out[blk * 1024 + lane * 8 + e], &hi, 2);
        std::memcpy(&out[blk * 1024 + 512 + lane * 8 + e], &lo, 2);
      }
  return out;
}
int upload_split(const std::vector<float>& pk, int k, void** dev) {
  const std::vector<uint16_t> h = split_weights(pk, k);
  return upload(h.data(), h.size() * 2, dev);
}

void fold_bn(const damvs_bn& bn, int c, std::vector<float>& scale, std::vector<float>& shift) {
  scale.resize(c);
  shift.resize(c);
  for (int i = 0; i < c; ++i) {
    const double inv = 1.0 / std::sqrt((double)bn.running_var[i] + (double)bn.eps);
    scale[i] = (float)(inv * bn.weight[i]);
    shift[i] = (float)(bn.bias[i] - bn.running_mean[i] * inv * bn.weight[i]);
  }
}

// damvs_stage_create's per-layer body from P.mt on (P.cin, P.cout, P.kind set; wf the BN-folded weights)
int stage_layer(LayerPlan& P, int dtype, const std::vector<float>& wf) {
  const int E = dtype == DAMVS_BF16 ? 8 : 4;
  int rc = DAMVS_OK;
  {
    P.mt = (P.cout + 15) / 16;
    if (P.mt == 3) P.mt = 4;
    build_phases(P, 4 * E);
    const int kexp = dtype == DAMVS_BF16 ? 0 : split_exponent(wf);
    P.wscale = std::ldexp(1.f, -kexp);
    if (P.kind == DECONV_S2 && P.cout == 8) {
      // conv11 runs on its x-pair packing alone (wpack_pair below; conv_args): no 8-phase packing
    } else if (dtype == DAMVS_BF16) {
      std::vector<uint16_t> pk;
      pack_layer<uint16_t>(P, wf, E, pk, cvt_bf16);
      rc = upload(pk.data(), pk.size() * 2, &P.wpack);
    } else {
      std::vector<float> pk;
      pack_layer<float>(P, wf, E, pk, cvt_f32);
      rc = upload_split(pk, kexp, &P.wpack);
    }
    if (rc == DAMVS_OK && dtype != DAMVS_BF16 &&
        ((P.kind == CONV_S1 && P.cin == 16 && P.cout == 16) || (P.kind == DECONV_S2 && P.cin == 32 && P.cout == 16) ||
         (P.kind == CONV_S2 && P.cin == 8 && P.cout == 16))) {
      LayerPlan P32 = P;
      build_phases(P32, 32);
      std::vector<float> p32;
      pack_layer<float>(P32, wf, 8, p32, cvt_f32);
      const std::vector<uint16_t> h = split_weights_blocked(p32, kexp);
      rc = upload(h.data(), h.size() * 2, &P.wpack32);
      P.wgat32 = P.wpack32;  // the same plain 32-K packing serves the gather kernel
      for (int p = 0; p < P32.nphase; ++p) P.k32_chunks[p] = P32.ph[p].kchunks, P.k32_off[p] = P32.ph[p].w_off;
    } else if (rc == DAMVS_OK && dtype != DAMVS_BF16 && P.cout > 8) {
      LayerPlan P32 = P;
      build_phases(P32, 32);
      std::vector<float> p32;
      pack_layer<float>(P32, wf, 8, p32, cvt_f32);
      const std::vector<uint16_t> h = split_weights_blocked(p32, kexp);
      rc = upload(h.data(), h.size() * 2, &P.wgat32);
      for (int p = 0; p < P32.nphase; ++p) P.k32_chunks[p] = P32.ph[p].kchunks, P.k32_off[p] = P32.ph[p].w_off;
    }
    if (rc == DAMVS_OK && P.kind == DECONV_S2 && P.cout <= 8) {
      build_phases_xpair(P, 4 * E);
      if (dtype == DAMVS_BF16) {
        std::vector<uint16_t> pk;
        pack_layer_xpair<uint16_t>(P, wf, E, pk, cvt_bf16);
        rc = upload(pk.data(), pk.size() * 2, &P.wpack_pair);
      } else {
        std::vector<float> pk;
        pack_layer_xpair<float>(P, wf, E, pk, cvt_f32);
        rc = upload_split(pk, kexp, &P.wpack_pair);
        if (rc == DAMVS_OK && P.cin == 16 && P.cout == 8) {  // conv11's z-streamed kernel (deconv_xpair_zslide<float>)
          LayerPlan P32 = P;
          build_phases_xpair(P32, 32);
          std::vector<float> p32;
          pack_layer_xpair<float>(P32, wf, 8, p32, cvt_f32);
          const std::vector<uint16_t> h = split_weights_blocked(p32, kexp);
          rc = upload(h.data(), h.size() * 2, &P.wpack32);
        }
      }
    }
    if (rc == DAMVS_OK && P.kind == CONV_S1 && P.cout <= 8) {
      if (dtype == DAMVS_BF16) {
        std::vector<uint16_t> pk;
        pack_layer_pair<uint16_t>(P, wf, E, pk, cvt_bf16);
        rc = upload(pk.data(), pk.size() * 2, &P.wpack_pair);
      } else {
        std::vector<float> pk;
        pack_layer_pair<float>(P, wf, E, pk, cvt_f32);
        rc = upload_split(pk, kexp, &P.wpack_pair);
        if (rc == DAMVS_OK) {  // conv0's z-streamed kernel (conv3d_zslide_pair<float>, CIN 8 / 16 / 32)
          std::vector<float> p32;
          pack_layer_pair<float>(P, wf, 8, p32, cvt_f32);
          const std::vector<uint16_t> h = split_weights_blocked(p32, kexp);
          rc = upload(h.data(), h.size() * 2, &P.wpack32);
        }
      }
    }
  }
  return rc;
}

// damvs_stage_create's two prob-row blocks (base 8)
struct Stage {
  void* prob_pack = nullptr;
  void* prob_split = nullptr;
  float prob_scale = 1.f;
};
int stage_prob_rows(Stage* st, int dtype, const float* prob_weight) {
  struct { const float* prob_weight; } crv = {prob_weight}, *cr = &crv;
  const int b = 8;
  int rc = DAMVS_OK;
  if (rc == DAMVS_OK && dtype == DAMVS_BF16 && b == 8) {
    std::vector<uint16_t> pk((size_t)kProbRowChunks * kProbRowTerms * 64 * 8, 0);
    for (int k = 0; k < kProbRowChunks; ++k)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 8; ++e) {
          const int m = lane & 15, j = m >> 2, dz = m & 3, sl = 4 * k + (lane >> 4), r = sl / 3, kx = sl % 3;
          const int ky = r - j;
          float v = 0.f;
          if (dz < 3 && sl < 18 && ky >= 0 && ky <= 2) v = cr->prob_weight[(size_t)e * 27 + dz * 9 + ky * 3 + kx];
          for (int t = 0; t < kProbRowTerms; ++t) {
            const uint16_t q = to_bf16(v);
            pk[(((size_t)k * kProbRowTerms + t) * 64 + lane) * 8 + e] = q;
            float qf;
            const uint32_t qb = (uint32_t)q << 16;
            std::memcpy(&qf, &qb, 4);
            v -= qf;  // exact: the remainder of a round-to-nearest bf16 term
          }
        }
    rc = upload(pk.data(), pk.size() * 2, &st->prob_pack);
  }
  if (rc == DAMVS_OK && dtype == DAMVS_F32 && b == 8) {
    std::vector<float> pf((size_t)kProbRowChunks * 64 * 8, 0.f), all(cr->prob_weight, cr->prob_weight + 27 * 8);
    for (int k = 0; k < kProbRowChunks; ++k)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 8; ++e) {
          const int m = lane & 15, j = m >> 2, dz = m & 3, sl = 4 * k + (lane >> 4), r = sl / 3, kx = sl % 3;
          const int ky = r - j;
          if (dz < 3 && sl < 18 && ky >= 0 && ky <= 2)
            pf[((size_t)k * 64 + lane) * 8 + e] = cr->prob_weight[(size_t)e * 27 + dz * 9 + ky * 3 + kx];
        }
    const int kp = split_exponent(all);
    st->prob_scale = std::ldexp(1.f, -kp);
    const std::vector<uint16_t> hsp = split_weights_blocked(pf, kp);
    rc = upload(hsp.data(), hsp.size() * 2, &st->prob_split);
  }
  return rc;
}

struct damvs_conv2d {
  damvs_conv2d_desc d;
  int dtype = 0, cout_pad = 0, cout_store = 0, MTtot = 0, nphase = 0, kchunk_k = 0;
  int xpair = 0;
  float wscale = 1.f;
  Conv2dPhase ph[4];
  void* wpack = nullptr;
  Conv2dPhase ph32[4];
  void* wpack32 = nullptr;
  float* wgeo = nullptr;
};

int build_phases_2d(damvs_conv2d* L) {
  const damvs_conv2d_desc& d = L->d;
  const int K = d.kernel, s = d.stride, p = d.padding;
  const int ctot = d.c0 + d.c1;
  std::memset(L->ph, 0, sizeof(L->ph));
  std::vector<int> offs[2], ks[2];  // per parity r
  if (!d.transposed) {
    L->nphase = 1;
    for (int k = 0; k < K; ++k) { offs[0].push_back(k - p); ks[0].push_back(k); }
  } else {
    if (s != 1 && s != 2) return fail(DAMVS_E_SHAPE, "transposed stride %d unsupported", s);
    L->nphase = s * s;
    for (int r = 0; r < s; ++r)
      for (int k = K - 1; k >= 0; --k)
        if (((r + p - k) % s + s) % s == 0) { offs[r].push_back((r + p - k) / s); ks[r].push_back(k); }
  }
  int w_off = 0, g_off = 0;
  for (int ph = 0; ph < L->nphase; ++ph) {
    Conv2dPhase& P = L->ph[ph];
    const int ry = d.transposed ? ph / s : 0, rx = d.transposed ? ph % s : 0;
    P.py = ry;
    P.px = rx;
    int t = 0;
    for (size_t a = 0; a < offs[ry].size(); ++a)
      for (size_t b = 0; b < offs[rx].size(); ++b) {
        if (t >= 25) return fail(DAMVS_E_SHAPE, "more than 25 taps per phase");
        P.tap[t][0] = (signed char)offs[ry][a];
        P.tap[t][1] = (signed char)offs[rx][b];
        P.wtap[t] = (signed char)(ks[ry][a] * K + ks[rx][b]);
        ++t;
      }
    P.ntaps = t;
    P.kchunks = ctot > 0 ? (t * ctot + L->kchunk_k - 1) / L->kchunk_k : 0;
    P.gchunks = d.ngeo > 0 ? (t * d.ngeo + L->kchunk_k - 1) / L->kchunk_k : 0;
    P.w_off = w_off;
    P.g_off = g_off;
    w_off += P.kchunks + P.gchunks;
    g_off += t * d.ngeo;
  }
  return DAMVS_OK;
}

int build_phases_2d_xpair(damvs_conv2d* L) {
  const damvs_conv2d_desc& d = L->d;
  const int K = d.kernel, p = d.padding;
  std::memset(L->ph, 0, sizeof(L->ph));
  std::vector<int> offs[2], ks[2];
  for (int r = 0; r < 2; ++r)
    for (int k = 0; k < K; ++k)
      if (((r + p - k) % 2 + 2) % 2 == 0) { offs[r].push_back((r + p - k) / 2); ks[r].push_back(k); }
  std::vector<int> xo;  // union of x offsets over both parities, ascending
  for (int r = 0; r < 2; ++r)
    for (int o : offs[r])
      if (std::find(xo.begin(), xo.end(), o) == xo.end()) xo.push_back(o);
  std::sort(xo.begin(), xo.end());
  L->nphase = 2;
  int w_off = 0;
  for (int ry = 0; ry < 2; ++ry) {
    Conv2dPhase& P = L->ph[ry];
    P.py = ry;
    P.px = 0;
    int t = 0;
    for (size_t a = 0; a < offs[ry].size(); ++a)
      for (int dx : xo) {
        if (t >= 25) return fail(DAMVS_E_SHAPE, "more than 25 taps per phase");
        P.tap[t][0] = (signed char)offs[ry][a];
        P.tap[t][1] = (signed char)dx;
        P.wtap[t] = (signed char)(ks[ry][a] * K);
        ++t;
      }
    P.ntaps = t;
    P.kchunks = (t * (d.c0 + d.c1) + L->kchunk_k - 1) / L->kchunk_k;
    P.gchunks = 0;
    P.w_off = w_off;
    w_off += P.kchunks;
  }
  return DAMVS_OK;
}

float wget(const damvs_conv2d_desc& d, const float* W, int co, int wc, int wt) {
  const int KK = d.kernel * d.kernel;
  return d.transposed ? W[((size_t)wc * d.cout + co) * KK + wt] : W[((size_t)co * d.cin + wc) * KK + wt];
}

template <typename S>
void pack_2d(const damvs_conv2d* L, const float* W, std::vector<S>& out, S (*cvt)(float)) {
  const damvs_conv2d_desc& d = L->d;
  const int E = L->kchunk_k / 4, ctot = d.c0 + d.c1;
  for (int ph = 0; ph < L->nphase; ++ph) {
    const Conv2dPhase& P = L->ph[ph];
    // tensor-input chunks (K = tap x concatenated channel), then plane chunks (K = tap x plane)
    for (int s = 0; s < P.kchunks + P.gchunks; ++s)
      for (int m = 0; m < L->MTtot; ++m)
        for (int lane = 0; lane < 64; ++lane)
          for (int e = 0; e < E; ++e) {
            const int co = m * 16 + (lane & 15);
            const bool plane = s >= P.kchunks;
            const int k = (plane ? s - P.kchunks : s) * L->kchunk_k + (lane >> 4) * E + e;
            const int per = plane ? d.ngeo : ctot;
            const int t = k / per, ci = k % per;
            float v = 0.f;
            if (co < d.cout && t < P.ntaps) {
              const int wc = plane ? d.geo_at[ci] : ci < d.c0 ? d.c0_at + ci : d.c1_at + (ci - d.c0);
              v = wget(d, W, co, wc, (unsigned char)P.wtap[t]);
            }
            out.push_back(cvt(v));
          }
  }
}

template <typename S>
void pack_2d_xpair(const damvs_conv2d* L, const float* W, std::vector<S>& out, S (*cvt)(float)) {
  const damvs_conv2d_desc& d = L->d;
  const int E = L->kchunk_k / 4, ctot = d.c0 + d.c1, K = d.kernel, p = d.padding;
  auto kx_of = [&](int px, int dx) {
    for (int k = 0; k < K; ++k)
      if (((px + p - k) % 2 + 2) % 2 == 0 && (px + p - k) / 2 == dx) return k;
    return -1;
  };
  for (int ph = 0; ph < L->nphase; ++ph) {
    const Conv2dPhase& P = L->ph[ph];
    for (int s = 0; s < P.kchunks; ++s)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < E; ++e) {
          const int row = lane & 15, px = row >> 3, co = row & 7;
          const int k = s * L->kchunk_k + (lane >> 4) * E + e;
          const int t = k / ctot, ci = k % ctot;
          float v = 0.f;
          if (co < d.cout && t < P.ntaps) {
            const int kx = kx_of(px, P.tap[t][1]);
            const int wc = ci < d.c0 ? d.c0_at + ci : d.c1_at + (ci - d.c0);
            if (kx >= 0) v = wget(d, W, co, wc, (unsigned char)P.wtap[t] + kx);
          }
          out.push_back(cvt(v));
        }
  }
}

// damvs_conv2d_create from `new damvs_conv2d()` to the plane weights (no validation, no bias)
int conv2d_create(const damvs_conv2d_desc* desc, const float* weight, int dtype, damvs_conv2d** out) {
  const damvs_conv2d_desc& d = *desc;
  const int E = dtype == DAMVS_BF16 ? 8 : 4;
  damvs_conv2d* L = new damvs_conv2d();
  *out = L;
  L->d = d;
  L->dtype = dtype;
  L->kchunk_k = 4 * E;
  L->MTtot = (d.cout + 15) / 16;
  L->cout_pad = L->MTtot * 16;
  L->cout_store = (d.cout + 3) / 4 * 4;
  L->xpair = d.transposed && d.stride == 2 && d.cout == 8 && d.ngeo == 0 && d.c0 + d.c1 > 0;
  int rc = L->xpair ? build_phases_2d_xpair(L) : build_phases_2d(L);
  if (rc == DAMVS_OK && d.c0 + d.c1 + d.ngeo > 0) {
    if (dtype == DAMVS_BF16) {
      std::vector<uint16_t> pk;
      if (L->xpair) pack_2d_xpair<uint16_t>(L, weight, pk, cvt_bf16);
      else pack_2d<uint16_t>(L, weight, pk, cvt_bf16);
      rc = upload(pk.data(), pk.size() * 2, &L->wpack);
    } else {
      std::vector<float> pk;
      if (L->xpair) pack_2d_xpair<float>(L, weight, pk, cvt_f32);
      else pack_2d<float>(L, weight, pk, cvt_f32);
      const int kexp = split_exponent(pk);
      L->wscale = std::ldexp(1.f, -kexp);
      rc = upload_split(pk, kexp, &L->wpack);
      const int ctot = d.c0 + d.c1;
      if (rc == DAMVS_OK && !L->xpair && d.c0 % 8 == 0 && d.c1 % 8 == 0 && ctot >= 8 && d.ngeo <= 1) {
        damvs_conv2d T32 = *L;
        T32.wpack = nullptr;
        T32.kchunk_k = 32;
        rc = build_phases_2d(&T32);
        if (rc == DAMVS_OK) {
          std::vector<float> p32;
          pack_2d<float>(&T32, weight, p32, cvt_f32);
          const std::vector<uint16_t> h = split_weights_blocked(p32, kexp);
          rc = upload(h.data(), h.size() * 2, &L->wpack32);
          std::memcpy(L->ph32, T32.ph, sizeof(L->ph32));
        }
      }
    }
  }
  if (rc == DAMVS_OK && d.ngeo > 0) {
    std::vector<float> wg;
    for (int ph = 0; ph < L->nphase; ++ph)
      for (int t = 0; t < L->ph[ph].ntaps; ++t)
        for (int g = 0; g < d.ngeo; ++g)
          for (int co = 0; co < L->cout_pad; ++co)
            wg.push_back(co < d.cout ? wget(d, weight, co, d.geo_at[g], (unsigned char)L->ph[ph].wtap[t]) : 0.f);
    rc = upload(wg.data(), wg.size() * 4, reinterpret_cast<void**>(&L->wgeo));
  }
  return rc;
}

}  // namespace parent

// ====================================================================== the comparison
// Element i of a tensor: distinct significands (i * odd mod 2^22, then an always-set last bit: all 24 bits in use),
// sign and one of four binades from an integer hash.
static float weight_value(uint32_t i, uint32_t salt) {
  uint32_t h = (i ^ (salt * 0x9e3779b9u)) * 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  const uint32_t mant = (((i * 2654435761u) & 0x3fffffu) << 1) | 1u;
  const uint32_t bits = (h & 0x80000000u) | ((124u + ((h >> 20) & 3u)) << 23) | mant;
  float f;
  std::memcpy(&f, &bits, 4);
  return f;
}
static std::vector<float> weights(size_t n, uint32_t salt) {
  std::vector<float> w(n);
  for (size_t i = 0; i < n; ++i) w[i] = weight_value((uint32_t)i, salt);
  return w;
}

static std::string g_case;
[[noreturn]] static void differ(const char* what, long at) {
  std::printf("DIFF case [%s] buffer %s byte offset %ld\n", g_case.c_str(), what, at);
  std::exit(1);
}
static void same(const char* what, const void* a, size_t na, const void* b, size_t nb) {
  if (na != nb) differ((std::string(what) + " (size " + std::to_string(na) + " != " + std::to_string(nb) + ")").c_str(), -1);
  const unsigned char *x = static_cast<const unsigned char*>(a), *y = static_cast<const unsigned char*>(b);
  for (size_t i = 0; i < na; ++i)
    if (x[i] != y[i]) differ(what, (long)i);
}
template <typename T>
static size_t same_buf(const char* what, const void* parent_dev, const std::vector<T>& v) {
  const Bytes none, *p = parent_dev ? static_cast<const Bytes*>(parent_dev) : &none;
  same(what, p->data(), p->size(), v.data(), v.size() * sizeof(T));
  return p->size();
}
static void same_int(const char* what, int a, int b) { same(what, &a, sizeof(a), &b, sizeof(b)); }
static void release() {
  for (Bytes* b : g_uploads) delete b;
  g_uploads.clear();
}
typedef std::chrono::steady_clock Clock;
static double ms(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

static void cases_3d() {
  double t_parent = 0, t_new = 0;
  for (int C : {8, 16, 32})
    for (int b : {8, 16}) {
      const int spec[10][3] = {{C, b, CONV_S1},         {b, 2 * b, CONV_S2},     {2 * b, 2 * b, CONV_S1},
                               {2 * b, 4 * b, CONV_S2}, {4 * b, 4 * b, CONV_S1}, {4 * b, 8 * b, CONV_S2},
                               {8 * b, 8 * b, CONV_S1}, {8 * b, 4 * b, DECONV_S2}, {4 * b, 2 * b, DECONV_S2},
                               {2 * b, b, DECONV_S2}};
      for (int li = 0; li < 10; ++li)
        for (int dtype : {DAMVS_F32, DAMVS_BF16}) {
          g_case = "3d " + std::to_string(C) + " " + std::to_string(b) + " " + std::to_string(li) + " " + std::to_string(dtype);
          const int cin = spec[li][0], cout = spec[li][1], kind = spec[li][2];
          const std::vector<float> wf = weights((size_t)cout * cin * 27, (uint32_t)(li + 1));
          parent::LayerPlan P;
          std::memset(P.ph_pair, 0, sizeof(P.ph_pair));  // `new damvs_stage()` zeroes the plan
          std::memset(P.ph, 0, sizeof(P.ph));
          P.cin = cin, P.cout = cout, P.kind = kind;
          const Clock::time_point t0 = Clock::now();
          if (parent::stage_layer(P, dtype, wf) != DAMVS_OK) differ("parent rc", -1);
          const Clock::time_point t1 = Clock::now();
          const damvs::CostregPack k = damvs::pack_costreg_layer(cin, cout, kind, dtype, wf);
          const Clock::time_point t2 = Clock::now();
          t_parent += ms(t0, t1), t_new += ms(t1, t2);
          size_t n = same_buf("wpack", P.wpack, k.wpack) + same_buf("wpack_pair", P.wpack_pair, k.wpack_pair) +
                     same_buf("wpack32", P.wpack32, k.wpack32);
          const bool alias = P.wgat32 && P.wgat32 == P.wpack32;
          same_int("wgat32 aliases wpack32", alias, k.wgat32_is_wpack32);
          n += same_buf("wgat32", alias ? nullptr : P.wgat32, k.wgat32);
          same_int("nphase", P.nphase, k.ph.n);
          same_int("nphase_pair", P.nphase_pair, k.ph_pair.n);
          same("ph", P.ph, sizeof(P.ph), k.ph.ph, sizeof(k.ph.ph));
          same("ph_pair", P.ph_pair, sizeof(P.ph_pair), k.ph_pair.ph, 4 * sizeof(ConvPhase));
          same("k32_chunks", P.k32_chunks, sizeof(P.k32_chunks), k.k32_chunks, sizeof(k.k32_chunks));
          same("k32_off", P.k32_off, sizeof(P.k32_off), k.k32_off, sizeof(k.k32_off));
          same_int("mt", P.mt, k.mt);
          same("wscale", &P.wscale, 4, &k.wscale, 4);
          std::printf("%s %zu\n", g_case.c_str(), n);
          release();
        }
    }
  std::printf("time3d %.1f %.1f\n", t_parent, t_new);
}

static void cases_prob() {
  const std::vector<float> w = weights(27 * 8, 77);
  for (int dtype : {DAMVS_F32, DAMVS_BF16}) {
    g_case = "prob " + std::to_string(dtype);
    parent::Stage st;
    if (parent::stage_prob_rows(&st, dtype, w.data()) != DAMVS_OK) differ("parent rc", -1);
    const damvs::ProbRows r = damvs::pack_prob_rows(w.data(), dtype, parent::kProbRowChunks, parent::kProbRowTerms);
    const size_t n = same_buf("rows", dtype == DAMVS_BF16 ? st.prob_pack : st.prob_split, r.rows);
    if (dtype == DAMVS_BF16 ? st.prob_split != nullptr : st.prob_pack != nullptr) differ("other form", -1);
    same("prob_scale", &st.prob_scale, 4, &r.scale, 4);
    std::printf("%s %zu\n", g_case.c_str(), n);
    release();
  }
}

// channel counts in units of E (4 fp32, 8 bf16) when negative, else as given; c1_at = kAfterC0: c0_at + c0
constexpr int kAfterC0 = 1000;
struct Case2d {
  const char* name;
  int transposed, kernel, stride, padding, output_padding, cout, c0, c0_at, c1, c1_at, ngeo, geo_at[4];
};
static const Case2d kCases2d[] = {
    {"k1s1", 0, 1, 1, 0, 0, 4, -1, 0, 0, 0, 0, {0, 0, 0, 0}},
    {"k1s2", 0, 1, 2, 0, 0, 8, -1, 0, 0, 0, 0, {0, 0, 0, 0}},
    {"k3s1", 0, 3, 1, 1, 0, 16, -1, 0, 0, 0, 0, {0, 0, 0, 0}},
    {"k3s2", 0, 3, 2, 1, 0, 24, -2, 0, 0, 0, 0, {0, 0, 0, 0}},
    {"k5s1", 0, 5, 1, 2, 0, 40, -1, 0, 0, 0, 0, {0, 0, 0, 0}},
    {"k5s2", 0, 5, 2, 2, 0, 8, -2, 0, 0, 0, 0, {0, 0, 0, 0}},
    {"k3c24", 0, 3, 1, 1, 0, 24, 24, 0, 0, 0, 0, {0, 0, 0, 0}},
    {"k3c32", 0, 3, 1, 1, 0, 16, 32, 0, 0, 0, 0, {0, 0, 0, 0}},
    {"concat", 0, 3, 1, 1, 0, 16, -1, -1, -1, 0, 0, {0, 0, 0, 0}},
    {"concat2", 0, 3, 1, 1, 0, 40, -2, -2, -2, 0, 0, {0, 0, 0, 0}},
    {"concat-inorder", 0, 3, 1, 1, 0, 16, -1, 0, -1, kAfterC0, 0, {0, 0, 0, 0}},
    {"concat-plane-first", 0, 3, 1, 1, 0, 24, -2, 1, -2, kAfterC0, 1, {0, 0, 0, 0}},
    {"plane+tensor", 0, 3, 1, 1, 0, 16, -2, 1, 0, 0, 1, {0, 0, 0, 0}},
    {"planes2", 0, 3, 1, 1, 0, 16, 0, 0, 0, 0, 2, {1, 0, 0, 0}},
    {"planes3", 0, 3, 2, 1, 0, 8, 0, 0, 0, 0, 3, {2, 0, 1, 0}},
    {"tk3s1", 1, 3, 1, 1, 0, 16, -2, 0, 0, 0, 0, {0, 0, 0, 0}},
    {"tk3s2", 1, 3, 2, 1, 1, 16, -2, 0, 0, 0, 0, {0, 0, 0, 0}},
    {"tk4s2", 1, 4, 2, 1, 0, 24, -1, 0, 0, 0, 0, {0, 0, 0, 0}},
    {"xpair-k3", 1, 3, 2, 1, 1, 8, -2, 0, 0, 0, 0, {0, 0, 0, 0}},
    {"xpair-k4", 1, 4, 2, 1, 0, 8, -1, 0, -1, kAfterC0, 0, {0, 0, 0, 0}},
    {"reject-stride3", 1, 3, 3, 1, 0, 16, -1, 0, 0, 0, 0, {0, 0, 0, 0}},
    {"reject-taps", 0, 6, 1, 2, 0, 16, -1, 0, 0, 0, 0, {0, 0, 0, 0}},
};

static void cases_2d() {
  uint32_t salt = 100;
  for (const Case2d& c : kCases2d)
    for (int dtype : {DAMVS_F32, DAMVS_BF16}) {
      g_case = std::string("2d ") + c.name + " " + std::to_string(dtype);
      const int E = dtype == DAMVS_BF16 ? 8 : 4;
      auto ch = [&](int v) { return v < 0 ? -v * E : v; };
      damvs_conv2d_desc d;
      std::memset(&d, 0, sizeof(d));
      d.transposed = c.transposed, d.kernel = c.kernel, d.stride = c.stride, d.padding = c.padding;
      d.output_padding = c.output_padding, d.cout = c.cout, d.relu = 1;
      d.c0 = ch(c.c0), d.c0_at = ch(c.c0_at), d.c1 = ch(c.c1), d.ngeo = c.ngeo;
      d.c1_at = c.c1_at == kAfterC0 ? d.c0_at + d.c0 : ch(c.c1_at);
      for (int g = 0; g < 4; ++g) d.geo_at[g] = c.geo_at[g];
      d.cin = d.c0 + d.c1 + d.ngeo;
      const std::vector<float> w = weights((size_t)d.cout * d.cin * d.kernel * d.kernel, ++salt);
      parent::damvs_conv2d* L = nullptr;
      parent::g_err.clear();
      const int rc = parent::conv2d_create(&d, w.data(), dtype, &L);
      const damvs::Conv2dPack k = damvs::pack_conv2d(d, w.data(), dtype);
      same("error", parent::g_err.data(), parent::g_err.size(), k.err.data(), k.err.size());
      same_int("rejected", rc != DAMVS_OK, !k.err.empty());
      size_t n = 0;
      if (rc == DAMVS_OK) {
        n = same_buf("wpack", L->wpack, k.wpack) + same_buf("wpack32", L->wpack32, k.wpack32) +
            same_buf("wgeo", L->wgeo ? reinterpret_cast<void*>(L->wgeo) : nullptr, k.wgeo);
        same("ph", L->ph, sizeof(L->ph), k.ph, sizeof(k.ph));
        same("ph32", L->ph32, sizeof(L->ph32), k.ph32, sizeof(k.ph32));
        same_int("nphase", L->nphase, k.nphase);
        same_int("xpair", L->xpair, k.xpair);
        same_int("MTtot", L->MTtot, k.MTtot);
        same_int("cout_pad", L->cout_pad, k.cout_pad);
        same_int("cout_store", L->cout_store, k.cout_store);
        same("wscale", &L->wscale, 4, &k.wscale, 4);
      } else if (rc != DAMVS_E_SHAPE) {
        differ("parent rc", -1);
      }
      std::printf("%s %zu %s\n", g_case.c_str(), n, rc == DAMVS_OK ? (k.xpair ? "xpair" : k.wpack32.empty() ? "ok" : "ok32") : "rejected");
      delete L;
      release();
    }
}

static void cases_bn() {
  g_case = "bn";
  const float var[] = {0.f, 1.f, 0.37f, 1e-7f, 123.5f, 3e-3f}, eps[] = {1e-5f, 1e-5f, 1e-3f, 0.f, 1e-5f, 1e-12f};
  const std::vector<float> w = weights(6, 1), m = weights(6, 2), bias = weights(6, 3);
  std::vector<float> e(6);
  int n = 0;
  for (int i = 0; i < 6; ++i) {  // eps is one value per BatchNorm: one tuple (and var = 0 with every eps) per call
    const damvs_bn bn = {w.data(), bias.data(), m.data(), var, eps[i]};
    std::vector<float> s0, t0, s1, t1;
    parent::fold_bn(bn, 6, s0, t0);
    damvs::bn_affine(bn, 6, s1, t1);
    same("scale", s0.data(), 24, s1.data(), s1.size() * 4);
    same("shift", t0.data(), 24, t1.data(), t1.size() * 4);
    n += 6;
  }
  std::printf("bn %d\n", n);
}

int main() {
  cases_3d();
  cases_prob();
  cases_2d();
  cases_bn();
  return 0;
}
"""

CASES_2D = ("k1s1", "k1s2", "k3s1", "k3s2", "k5s1", "k5s2", "k3c24", "k3c32", "concat", "concat2", "concat-inorder",
            "concat-plane-first", "plane+tensor", "planes2", "planes3", "tk3s1", "tk3s2", "tk4s2", "xpair-k3", "xpair-k4",
            "reject-stride3", "reject-taps")
F32, BF16 = 0, 1  # include/damvs.h


def expected_cases():
    out = [("3d", str(C), str(b), str(li), str(dt)) for C in (8, 16, 32) for b in (8, 16) for li in range(10)
           for dt in (F32, BF16)]
    out.append(("time3d",))
    out += [("prob", str(dt)) for dt in (F32, BF16)]
    out += [("2d", name, str(dt)) for name in CASES_2D for dt in (F32, BF16)]
    out.append(("bn",))
    return out


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("weight_pack")
    src, exe = str(d / "weight_pack_main.cpp"), str(d / "weight_pack_main")
    with open(src, "w") as f:
        f.write(PROGRAM)
    with open(os.path.join(build.CSRC, "damvs_internal.h")) as f:
        chunks, terms = re.search(r"kProbRowChunks = (\d+), kProbRowTerms = (\d+);", f.read()).groups()
    r = subprocess.run([build.HIPCC, "-x", "c++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + build.CSRC,
                        "-I" + build.INCLUDE, "-DPROB_ROW_CHUNKS=" + chunks, "-DPROB_ROW_TERMS=" + terms, src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-400:])
    print(r.stdout)
    return [line.split() for line in r.stdout.splitlines()]


def test_every_case_ran(lines):
    exp = expected_cases()
    assert [tuple(l[:len(e)]) for l, e in zip(lines, exp)] == exp
    assert len(lines) == len(exp)


def test_every_packing_form_was_compared(lines):
    """The program has compared every byte; here that the cases reached every form: each 3D layer packed something,
    the 2D cases took the 16-K form alone, the 32-K form, the x-pair form and both rejections."""
    assert all(int(l[5]) > 0 for l in lines if l[0] == "3d")
    assert all(int(l[2]) > 0 for l in lines if l[0] == "prob")
    kinds = {(l[1], int(l[2])): l[4] for l in lines if l[0] == "2d"}
    assert {n for (n, dt), k in kinds.items() if k == "rejected"} == {"reject-stride3", "reject-taps"}
    assert {n for (n, dt), k in kinds.items() if k == "xpair"} == {"xpair-k3", "xpair-k4"}
    assert {n for (n, dt), k in kinds.items() if k == "ok32"} == {"k3s2", "k5s2", "k3c24", "k3c32", "concat2",
                                                                  "concat-plane-first", "plane+tensor", "tk3s1",
                                                                  "tk3s2"}
    assert all(dt == F32 for (n, dt), k in kinds.items() if k == "ok32")
    assert all(int(l[3]) > 0 for l in lines if l[0] == "2d" and l[4] != "rejected")
    assert [l[1] for l in lines if l[0] == "bn"] == ["36"]
