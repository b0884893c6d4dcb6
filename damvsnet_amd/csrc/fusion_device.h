// Device helpers shared by the two depth-fusion kernels (k_fusion.hip, k_fusion_static.hip): the cv2.remap
// INTER_LINEAR lookup and the float32-matrix times float64-vector products of the reference's numpy code.
#pragma once
#include "damvs_device.h"

namespace damvs {

namespace {

__device__ __forceinline__ float remap_linear(const float* __restrict__ src, int H, int W, float mx, float my) {
  // cv2: X = cvRound(mx * 32), sx = X >> 5, fx = (X & 31) / 32 (INTER_BITS = 5)
  const float X = rintf(__fmul_rn(mx, 32.f)), Y = rintf(__fmul_rn(my, 32.f));
  if (!(X > -2147483648.f && X < 2147483520.f && Y > -2147483648.f && Y < 2147483520.f)) return 0.f;
  const int xi = (int)X, yi = (int)Y;
  const int sx = min(max(xi >> 5, -32768), 32767), sy = min(max(yi >> 5, -32768), 32767);
  if (sx >= W || sx + 1 < 0 || sy >= H || sy + 1 < 0) return 0.f;
  const float fx = __fmul_rn((float)(xi & 31), 0.03125f), fy = __fmul_rn((float)(yi & 31), 0.03125f);
  const float cx0 = __fsub_rn(1.f, fx), cy0 = __fsub_rn(1.f, fy);
  const float w[4] = {__fmul_rn(cy0, cx0), __fmul_rn(cy0, fx), __fmul_rn(fy, cx0), __fmul_rn(fy, fx)};
  float v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int xx = sx + (k & 1), yy = sy + (k >> 1);
    v[k] = (xx >= 0 && xx < W && yy >= 0 && yy < H) ? src[(size_t)yy * W + xx] : 0.f;
  }
  return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(v[0], w[0]), __fmul_rn(v[1], w[1])), __fmul_rn(v[2], w[2])),
                   __fmul_rn(v[3], w[3]));
}

// 3x3 (row-major, float32 -> double) times a double 3-vector
__device__ __forceinline__ void mv3(const float* m, const double* v, double* o) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
    o[i] = (double)m[3 * i] * v[0] + (double)m[3 * i + 1] * v[1] + (double)m[3 * i + 2] * v[2];
}
// rows 0-2 of a 4x4 (float32 -> double) times (v, 1)
__device__ __forceinline__ void mv34(const float* m, const double* v, double* o) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
    o[i] = (double)m[4 * i] * v[0] + (double)m[4 * i + 1] * v[1] + (double)m[4 * i + 2] * v[2] + (double)m[4 * i + 3];
}

}  // namespace

}  // namespace damvs
