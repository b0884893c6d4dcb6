// Consensus depth fusion: every surface point once, averaged over the views that agree
// on it. fusion.consensus_statement is the rule in numpy; include/damvs.h (damvs_consensus_view) states it in words.
// Every operation below is one IEEE double operation in the statement's order: this unit is built with
// -ffp-contract=off (build.FILE_FLAGS), so no multiply-add is contracted, and double division is correctly rounded.
// The device therefore equals the statement bit for bit.
//
// One thread per pixel p = (x, y) of the reference view, 256 per block. The scene table (one ConsensusEntry per view:
// cameras and the pointers of its depth, confidence, colour and `used` maps) lies in device memory and is indexed by
// kernel arguments only, so every read of it is wave-uniform; the source list and the fb values are kernel arguments.
//   valid(v, q): depth finite, depth > 0, not (conf < thr).
//   The pixel is skipped unless valid(ref, p) and used[ref][p] == 0 (bit values 1 and 8 of the mask tell).
//   X = Einv_ref (Kinv_ref (x d, y d, d)); per source s in list order: q = E_s X, q.z > 0; u = K_s q,
//   (px, py) = floor(u.xy / u.z + 0.5) inside the image; valid(s, (px, py)), ds its depth; |fb / q.z - fb / ds| < disp;
//   then X_s = Einv_s (Kinv_s (px ds, py ds, ds)) joins the position sum, the source's colour the channel sums,
//   used[s][py][px] = 1 (a plain byte store) and n counts it. n >= num_consistent emits (X + sum X_s) / (n + 1) and the
//   rounded mean colour.
// The loop over the sources is the outer order of the memory accesses: at any moment a wave reads one source's maps at
// the pixels its 64 neighbouring reference pixels project to, which are neighbours again wherever the surface is
// smooth, so the gathers of depth (4 bytes), confidence (4) and colour (3) mostly share cache lines.
// A launch writes `used` of its sources and reads `used` of its reference view only, and the reference view is never
// among the sources (capi.cpp refuses it): no thread reads a byte another thread of the launch writes, all marks store
// the same value 1, so the result does not depend on the order of the threads. No atomics, no LDS, no MFMA.
//
// This unit is linked into its own library, libdamvs_consensus.so, which libdamvs.so depends on: its kernel is pinned by
// tests/isa_pins_consensus.json (tests/test_consensus_codeobj.py).
#include "damvs_internal.h"

namespace damvs {

namespace {

// The table is written before the launch and never during it, and its addresses come from kernel arguments alone: read
// through the constant address space, every entry is fetched once per wave by scalar loads. The maps an entry points
// to are global memory.
#define DAMVS_CONSTANT __attribute__((address_space(4)))
#define DAMVS_GLOBAL __attribute__((address_space(1)))
typedef const DAMVS_CONSTANT ConsensusEntry* TablePtr;

__device__ __forceinline__ bool sample_valid(float d, float c, float thr) {
  return fabsf(d) < __builtin_inff() && d > 0.f && !(c < thr);
}

// 3x3 and 3x4 products of fusion_device.h (mv3, mv34) on a matrix of the table
__device__ __forceinline__ void tmv3(const DAMVS_CONSTANT float* m, const double* v, double* o) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
    o[i] = (double)m[3 * i] * v[0] + (double)m[3 * i + 1] * v[1] + (double)m[3 * i + 2] * v[2];
}
__device__ __forceinline__ void tmv34(const DAMVS_CONSTANT float* m, const double* v, double* o) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
    o[i] = (double)m[4 * i] * v[0] + (double)m[4 * i + 1] * v[1] + (double)m[4 * i + 2] * v[2] + (double)m[4 * i + 3];
}

// Einv (Kinv (x d, y d, d)) of the table entry e
__device__ __forceinline__ void world_point(TablePtr e, int x, int y, double d, double* X) {
  const double a[3] = {(double)x * d, (double)y * d, d};
  double c[3];
  tmv3(e->kinv, a, c);
  tmv34(e->einv, c, X);
}

__global__ __launch_bounds__(kConsensusBlock) void consensus_view_kernel(const ConsensusArgs a) {
  const long long p = (long long)blockIdx.x * kConsensusBlock + threadIdx.x;
  if (p >= a.n) return;
  const TablePtr table = (TablePtr)(uintptr_t)a.table;
  const TablePtr r = table + a.ref;
  const float d32 = ((const DAMVS_GLOBAL float*)r->depth)[p];
  const bool valid = sample_valid(d32, ((const DAMVS_GLOBAL float*)r->conf)[p], a.prob_thr);
  const bool consumed = ((const DAMVS_GLOBAL unsigned char*)r->used)[p] != 0;
  unsigned char m = (valid ? 1 : 0) | (consumed ? 8 : 0);
  float o[3] = {0.f, 0.f, 0.f};
  unsigned char oc[3] = {0, 0, 0};
  if (valid && !consumed) {
    const int y = (int)(p / a.W), x = (int)(p - (long long)y * a.W);
    double X[3];
    world_point(r, x, y, (double)d32, X);
    double s0 = X[0], s1 = X[1], s2 = X[2];
    const DAMVS_GLOBAL unsigned char* rc = (const DAMVS_GLOBAL unsigned char*)r->rgb + 3 * (size_t)p;
    unsigned c0 = rc[0], c1 = rc[1], c2 = rc[2];
    unsigned n = 0;
    for (int i = 0; i < a.nsrc; ++i) {
      const TablePtr e = table + a.src[i];
      double q[3], u[3];
      tmv34(e->e, X, q);
      if (!(q[2] > 0.0)) continue;
      tmv3(e->k, q, u);
      const double fx = floor(u[0] / u[2] + 0.5), fy = floor(u[1] / u[2] + 0.5);
      // NaN fails every comparison, an infinity one of them
      if (!(fx >= 0.0 && fx < (double)a.W && fy >= 0.0 && fy < (double)a.H)) continue;
      const int px = (int)fx, py = (int)fy;
      const size_t g = (size_t)py * a.W + px;
      const float ds32 = ((const DAMVS_GLOBAL float*)e->depth)[g];
      if (!sample_valid(ds32, ((const DAMVS_GLOBAL float*)e->conf)[g], a.prob_thr)) continue;
      const double ds = (double)ds32, fb = a.fb[i];
      if (!(fabs(fb / q[2] - fb / ds) < a.disp_thr)) continue;
      double Xs[3];
      world_point(e, px, py, ds, Xs);
      s0 = s0 + Xs[0];
      s1 = s1 + Xs[1];
      s2 = s2 + Xs[2];
      const DAMVS_GLOBAL unsigned char* sc = (const DAMVS_GLOBAL unsigned char*)e->rgb + 3 * g;
      c0 += sc[0];
      c1 += sc[1];
      c2 += sc[2];
      ((DAMVS_GLOBAL unsigned char*)e->used)[g] = 1;
      ++n;
    }
    if (n >= (unsigned)a.num_consistent) {
      m |= 2 | 4;
      const double k = (double)(n + 1);
      o[0] = (float)(s0 / k);
      o[1] = (float)(s1 / k);
      o[2] = (float)(s2 / k);
      const unsigned den = 2 * (n + 1);
      oc[0] = (unsigned char)((2 * c0 + (n + 1)) / den);
      oc[1] = (unsigned char)((2 * c1 + (n + 1)) / den);
      oc[2] = (unsigned char)((2 * c2 + (n + 1)) / den);
    }
  }
  a.mask[p] = m;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a.xyz[3 * (size_t)p + k] = o[k];
    a.rgb_avg[3 * (size_t)p + k] = oc[k];
  }
}

}  // namespace

hipError_t launch_consensus_view(hipStream_t s, const ConsensusArgs& a) {
  const unsigned blocks = (unsigned)((a.n + kConsensusBlock - 1) / kConsensusBlock);
  hipLaunchKernelGGL(consensus_view_kernel, dim3(blocks), dim3(kConsensusBlock), 0, s, a);
  return hipGetLastError();
}

#ifndef DAMVS_BUILD_ID
#define DAMVS_BUILD_ID "unstamped"
#endif
const char* consensus_build_id() { return DAMVS_BUILD_ID; }

}  // namespace damvs
