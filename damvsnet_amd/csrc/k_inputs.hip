// Scene inputs: one launch writes the forward's `imgs` tensor for a batch from the
// scene's decoded images, resident on the device as uint8 HWC. It replaces the host path of
// datasets/general_eval.py:83-108 (np.array(img, float32) / 255, cv2.resize to the working size) and the np.stack and
// pageable upload of B * N float32 images per batch: a view crosses PCIe once, as the bytes it was decoded to.
//
// Image i of the launch, slot s = slots[i] (include/damvs.h, damvs_scene_inputs), channel c, output pixel (y, x):
//   p(v, u)      = float(rgb_store[s][v][u][c]) / 255.0f                                  correctly rounded
//   per axis     scale = float(n_in) / float(n_out);  src = max(fma(scale, float(d) + 0.5f, -0.5f), 0)
//                i0 = min(int(src), n_in - 1);  i1 = min(i0 + 1, n_in - 1);  l1 = src - float(i0);  l0 = 1 - l1
//   out[i][c][y][x] = a0 * (b0 * p(y0, x0) + b1 * p(y0, x1)) + a1 * (b0 * p(y1, x0) + b1 * p(y1, x1))
// with a the row weights and b the column weights, every product, sum and difference rounded on its own and the
// coordinate's multiply-add rounded once: F.interpolate(bilinear, align_corners=False) as torch's CPU kernel computes
// it, stated in numpy by tests/inputs_statement.py, which the kernel equals bit for bit. At n_in == n_out the
// coordinate is d exactly, l1 = 0 and the output is the byte's quotient: no second path for the identity size.
//
// The contraction that hipcc applies by default would fuse the combine's products into the sums, and the rounded
// intrinsics (__fmul_rn, __fadd_rn, ...) are plain operators in this compiler's headers, which inherit it. So the
// operators below are compiled with contraction off and the one fused operation is spelt as a builtin.
//
// VALU only, memory bound on its stores: a thread owns 4 consecutive output pixels of a row and stores three 16-byte
// vectors, one per colour plane (a wave: 1 KiB of a row per plane). The taps are byte loads: the four pixels' sources
// are 2 x 2 pixels of 3 bytes each, 6 contiguous bytes per row unless the column clamps, at any scale, and they come
// from L2 (a source row is read by the two or three output rows around it). No LDS, no atomics, no scratch, no
// dependency between blocks. The slot table travels in the kernel arguments (no device memory of the call's own: it
// can be captured into a graph); the image index is blockIdx.z, so the slot and the bases are wave-uniform 64-bit
// scalars and the offsets within an image 32-bit (3 * H0 * W0 and 3 * H * W < 2^31, checked by the C ABI). W is a
// multiple of 4 and `out` 16-byte aligned (checked there too).
//
// This unit is linked into its own library, libdamvs_inputs.so, which libdamvs.so depends on: its kernel is pinned by
// tests/isa_pins_inputs.json (tests/test_inputs_codeobj.py).
#pragma clang fp contract(off)
#include "damvs_internal.h"

namespace damvs {

namespace {

// one rounding each (contraction is off in this unit)
__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }
__device__ __forceinline__ float div_rn(float a, float b) { return a / b; }

struct Tap {
  unsigned i0, i1;  // source indices, both in [0, n_in)
  float l0, l1;     // their weights
};

__device__ __forceinline__ Tap tap(float scale, unsigned d, int n_in) {
  const float src = fmaxf(__builtin_fmaf(scale, add_rn((float)d, 0.5f), -0.5f), 0.0f);
  const int i0 = min((int)src, n_in - 1);
  const int i1 = min(i0 + 1, n_in - 1);
  const float l1 = sub_rn(src, (float)i0);
  return {(unsigned)i0, (unsigned)i1, sub_rn(1.0f, l1), l1};
}

__device__ __forceinline__ float unit(const unsigned char* __restrict__ p, unsigned off) {
  return div_rn((float)p[off], 255.0f);
}

__global__ __launch_bounds__(kInputsBlockX* kInputsBlockY) void scene_inputs_kernel(const InputsArgs a) {
  const unsigned x4 = blockIdx.x * kInputsBlockX + threadIdx.x;  // group of 4 pixels in the row
  if (x4 >= (unsigned)a.W >> 2) return;
  const unsigned i = blockIdx.z;
  const unsigned hw = (unsigned)a.H * (unsigned)a.W;
  const unsigned char* __restrict__ src = a.rgb_store + (size_t)a.slots[i] * 3 * (unsigned)a.H0 * (unsigned)a.W0;
  float* __restrict__ dst = a.out + (size_t)i * 3 * hw;
  const float sy = div_rn((float)a.H0, (float)a.H), sx = div_rn((float)a.W0, (float)a.W);
  Tap col[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) col[k] = tap(sx, 4 * x4 + k, a.W0);
  // rows: blockIdx.y strides when H / kInputsBlockY exceeds the grid's y limit (one trip at every real size)
  for (unsigned y = blockIdx.y * kInputsBlockY + threadIdx.y; y < (unsigned)a.H; y += gridDim.y * kInputsBlockY) {
    const Tap row = tap(sy, y, a.H0);
    const unsigned r0 = row.i0 * 3 * (unsigned)a.W0, r1 = row.i1 * 3 * (unsigned)a.W0;  // byte offsets < 3 * H0 * W0
    float v[3][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned c0 = 3 * col[k].i0, c1 = 3 * col[k].i1;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float top = add_rn(mul_rn(col[k].l0, unit(src, r0 + c0 + c)), mul_rn(col[k].l1, unit(src, r0 + c1 + c)));
        const float bot = add_rn(mul_rn(col[k].l0, unit(src, r1 + c0 + c)), mul_rn(col[k].l1, unit(src, r1 + c1 + c)));
        v[c][k] = add_rn(mul_rn(row.l0, top), mul_rn(row.l1, bot));
      }
    }
    const unsigned off = y * (unsigned)a.W + 4 * x4;  // first of the 4 pixels, < H * W
#pragma unroll
    for (int c = 0; c < 3; ++c)
      *reinterpret_cast<float4*>(dst + c * hw + off) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
  }
}

}  // namespace

hipError_t launch_scene_inputs(hipStream_t s, int n_images, const InputsArgs& a) {
  const unsigned gx = ((unsigned)a.W / 4 + kInputsBlockX - 1) / kInputsBlockX;
  const unsigned rows = ((unsigned)a.H + kInputsBlockY - 1) / kInputsBlockY;
  const dim3 grid(gx, rows < 32768u ? rows : 32768u, (unsigned)n_images);
  hipLaunchKernelGGL(scene_inputs_kernel, grid, dim3(kInputsBlockX, kInputsBlockY), 0, s, a);
  return hipGetLastError();
}

#ifndef DAMVS_BUILD_ID
#define DAMVS_BUILD_ID "unstamped"
#endif
const char* inputs_build_id() { return DAMVS_BUILD_ID; }

}  // namespace damvs
