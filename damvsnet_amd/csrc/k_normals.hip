// Oriented point cloud: the normal of every fused point, from the averaged depth map it
// is a pixel of. fusion.normals_statement is the rule in numpy; include/damvs.h (damvs_fusion_normals) states it in
// words. Every operation below is one IEEE double operation in the statement's order: this unit is built with
// -ffp-contract=off (build.FILE_FLAGS), so no multiply-add is contracted, and double division and square root are
// correctly rounded. The device therefore equals the statement bit for bit.
//
// Per pixel c = (x, y) with the fusion's final bit (mask bit value 4):
//   P(q) = Kinv (x_q d_q, y_q d_q, d_q), d = depth_avg as double;
//   a 4-neighbour q is usable when it is inside the image, final, and |d_q - d_c| <= jump * d_c (NaN compares false);
//   tx = (east usable ? P(E) : P(c)) - (west usable ? P(W) : P(c)), present when either is usable; ty the same with
//   south (y + 1) and north (y - 1);
//   n = ty x tx, negated when n . P(c) > 0, divided by sqrt(n . n); when a tangent is missing or n . n is 0 or not finite,
//   -P(c) / sqrt(P(c) . P(c)) instead; the world normal is Rinv times that, cast to float32, not renormalised; (0, 0, 0)
//   when a component is not finite, and for pixels without the final bit.
//
// Two kernels share pixel_normal:
//   normal_map_kernel               one thread per pixel -> normals [H][W][3] float32 (0 off-mask)
//   cloud_scatter_oriented_kernel   the tiling, ranks and LDS staging of cloud_scatter_kernel (k_cloud.hip) with 27-byte
//                                   records: x, y, z, nx, ny, nz little-endian float32, red, green, blue. It reads the
//                                   tile offsets and the cursor's base that cloud_count_kernel / cloud_scan_kernel left
//                                   in `scratch` (layout: k_cloud.hip), so it runs after damvs_fusion_cloud's three
//                                   launches at capacity 0 on the same stream. `select` picks the pixels (the fusion
//                                   mask, or the thinning's keep), `mask` is the fusion mask the neighbours are judged by.
// No atomics, no block waits for another one.
//
// This unit is linked into its own library, libdamvs_normals.so, which libdamvs.so depends on: its kernels are pinned by
// tests/isa_pins_normals.json (tests/test_normals_codeobj.py).
#include "damvs_internal.h"

namespace damvs {

namespace {

constexpr int kRec = 27;  // bytes per oriented record
constexpr int kWaves = kCloudTile / 64;

struct P3 {
  double x, y, z;
};

// Kinv (x d, y d, d): the sums left to right, as the statement spells them
__device__ __forceinline__ P3 cam_point(const float* __restrict__ k, int x, int y, double d) {
  const double a0 = (double)x * d, a1 = (double)y * d;
  P3 p;
  p.x = (double)k[0] * a0 + (double)k[1] * a1 + (double)k[2] * d;
  p.y = (double)k[3] * a0 + (double)k[4] * a1 + (double)k[5] * d;
  p.z = (double)k[6] * a0 + (double)k[7] * a1 + (double)k[8] * d;
  return p;
}

// The neighbour at (x, y) when it is usable for the centre of depth dc (lim = jump * dc), else the centre's point.
__device__ __forceinline__ bool neighbour(const NormalArgs& a, int x, int y, double dc, double lim, P3& p) {
  if (x < 0 || x >= a.W || y < 0 || y >= a.H) return false;
  const size_t q = (size_t)y * a.W + x;
  if ((a.mask[q] & 4) == 0) return false;
  const double dq = (double)a.depth[q];
  if (!(fabs(dq - dc) <= lim)) return false;
  p = cam_point(a.kinv, x, y, dq);
  return true;
}

// The rule for the pixel (x, y), which has the final bit.
__device__ __forceinline__ void pixel_normal(const NormalArgs& a, int x, int y, float* o) {
  const double dc = (double)a.depth[(size_t)y * a.W + x];
  const double lim = a.jump * dc;
  const P3 c = cam_point(a.kinv, x, y, dc);
  P3 e = c, w = c, s = c, n = c;
  const bool ue = neighbour(a, x + 1, y, dc, lim, e), uw = neighbour(a, x - 1, y, dc, lim, w);
  const bool us = neighbour(a, x, y + 1, dc, lim, s), un = neighbour(a, x, y - 1, dc, lim, n);
  const double tx0 = e.x - w.x, tx1 = e.y - w.y, tx2 = e.z - w.z;
  const double ty0 = s.x - n.x, ty1 = s.y - n.y, ty2 = s.z - n.z;
  double n0 = ty1 * tx2 - ty2 * tx1;
  double n1 = ty2 * tx0 - ty0 * tx2;
  double n2 = ty0 * tx1 - ty1 * tx0;
  const double dot = n0 * c.x + n1 * c.y + n2 * c.z;
  if (dot > 0.0) {
    n0 = -n0;
    n1 = -n1;
    n2 = -n2;
  }
  const double nn = n0 * n0 + n1 * n1 + n2 * n2;
  double c0, c1, c2;
  if ((ue || uw) && (us || un) && nn > 0.0 && nn < __builtin_inf()) {
    const double l = sqrt(nn);
    c0 = n0 / l;
    c1 = n1 / l;
    c2 = n2 / l;
  } else {
    const double l = sqrt(c.x * c.x + c.y * c.y + c.z * c.z);
    c0 = -c.x / l;
    c1 = -c.y / l;
    c2 = -c.z / l;
  }
  const float* r = a.rinv;
  const float w0 = (float)((double)r[0] * c0 + (double)r[1] * c1 + (double)r[2] * c2);
  const float w1 = (float)((double)r[3] * c0 + (double)r[4] * c1 + (double)r[5] * c2);
  const float w2 = (float)((double)r[6] * c0 + (double)r[7] * c1 + (double)r[8] * c2);
  const bool fin = fabsf(w0) < __builtin_inff() && fabsf(w1) < __builtin_inff() && fabsf(w2) < __builtin_inff();
  o[0] = fin ? w0 : 0.f;
  o[1] = fin ? w1 : 0.f;
  o[2] = fin ? w2 : 0.f;
}

__global__ __launch_bounds__(kCloudTile) void normal_map_kernel(const NormalArgs a) {
  const long long p = (long long)blockIdx.x * kCloudTile + threadIdx.x;
  if (p >= a.n) return;
  float o[3] = {0.f, 0.f, 0.f};
  if ((a.mask[p] & 4) != 0) {
    const int y = (int)(p / a.W);
    pixel_normal(a, (int)(p - (long long)y * a.W), y, o);
  }
  a.normals[3 * (size_t)p] = o[0];
  a.normals[3 * (size_t)p + 1] = o[1];
  a.normals[3 * (size_t)p + 2] = o[2];
}

// tile_rank of k_cloud.hip: the rank of this thread among the block's selected threads and the block's total
__device__ __forceinline__ unsigned tile_rank(bool sel, unsigned* wtot, unsigned& total) {
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long b = __ballot(sel);
  if (lane == 0) wtot[wave] = (unsigned)__popcll(b);
  __syncthreads();
  unsigned before = 0;
  total = 0;
#pragma unroll
  for (unsigned w = 0; w < (unsigned)kWaves; ++w) {
    const unsigned t = wtot[w];
    if (w < wave) before += t;
    total += t;
  }
  return before + (unsigned)__popcll(b & ((1ull << lane) - 1ull));
}

__device__ __forceinline__ void put32(unsigned char* d, float f) {
  const unsigned u = __float_as_uint(f);
  d[0] = (unsigned char)u;
  d[1] = (unsigned char)(u >> 8);
  d[2] = (unsigned char)(u >> 16);
  d[3] = (unsigned char)(u >> 24);
}

// cloud_scatter_kernel's staging: the tile's records are contiguous in the output, staged in LDS at the byte phase of
// their global address, then stored as aligned dwords with byte stores at the two ragged ends. Two tiles may share a
// dword at their seam; each writes its own bytes of it only.
__global__ __launch_bounds__(kCloudTile) void cloud_scatter_oriented_kernel(const NormalArgs a) {
  __shared__ unsigned wtot[kWaves];
  __shared__ unsigned stage32[(kCloudTile * kRec + 3) / 4 + 1];
  unsigned char* stage = reinterpret_cast<unsigned char*>(stage32);
  const long long p = (long long)blockIdx.x * kCloudTile + threadIdx.x;
  const bool sel = p < a.n && (a.select[p] & 4) != 0;
  unsigned n;
  const unsigned r = tile_rank(sel, wtot, n);
  if (n == 0) return;
  const unsigned long long base = (unsigned long long)a.scratch[a.ntiles] | ((unsigned long long)a.scratch[a.ntiles + 1] << 32);
  const unsigned long long first = base + a.scratch[blockIdx.x];  // record index of the tile's first point
  const unsigned long long cap = (unsigned long long)a.capacity;
  if (first >= cap) return;
  const unsigned nw = cap - first < (unsigned long long)n ? (unsigned)(cap - first) : n;  // records that fit
  const unsigned long long g0 = (unsigned long long)reinterpret_cast<uintptr_t>(a.records) + first * (unsigned long long)kRec;
  const unsigned shift = (unsigned)(g0 & 3ull);
  if (sel && r < nw) {
    unsigned char* d = stage + shift + r * kRec;
    const float* s = a.xyz + 3 * (size_t)p;
    float o[3] = {0.f, 0.f, 0.f};
    if ((a.mask[p] & 4) != 0) {
      const int y = (int)(p / a.W);
      pixel_normal(a, (int)(p - (long long)y * a.W), y, o);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      put32(d + 4 * k, s[k]);
      put32(d + 12 + 4 * k, o[k]);
    }
    const unsigned char* c = a.rgb + 3 * (size_t)p;
    d[24] = c[0];
    d[25] = c[1];
    d[26] = c[2];
  }
  __syncthreads();
  unsigned char* g = reinterpret_cast<unsigned char*>(static_cast<uintptr_t>(g0 - shift));
  const unsigned end = shift + nw * kRec;                // stage[shift .. end) holds the tile's bytes; end >= 27
  const unsigned lo = shift ? 4u : 0u, hi = end & ~3u;  // aligned body stage[lo .. hi), lo <= hi
  if (threadIdx.x >= shift && threadIdx.x < lo) g[threadIdx.x] = stage[threadIdx.x];
  unsigned* g32 = reinterpret_cast<unsigned*>(g);
  for (unsigned i = lo / 4 + threadIdx.x; i < hi / 4; i += kCloudTile) g32[i] = stage32[i];
  if (threadIdx.x < end - hi) g[hi + threadIdx.x] = stage[hi + threadIdx.x];
}

}  // namespace

hipError_t launch_normal_map(hipStream_t s, const NormalArgs& a) {
  hipLaunchKernelGGL(normal_map_kernel, dim3(a.ntiles), dim3(kCloudTile), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_cloud_oriented(hipStream_t s, const NormalArgs& a) {
  hipLaunchKernelGGL(cloud_scatter_oriented_kernel, dim3(a.ntiles), dim3(kCloudTile), 0, s, a);
  return hipGetLastError();
}

#ifndef DAMVS_BUILD_ID
#define DAMVS_BUILD_ID "unstamped"
#endif
const char* normals_build_id() { return DAMVS_BUILD_ID; }

}  // namespace damvs
