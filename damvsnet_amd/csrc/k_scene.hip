// Scene ingest: one launch takes the outputs of a forward over B reference views and
// writes each sample into its slot of three scene-resident stores, the inputs of depth fusion (k_fusion.hip,
// k_fusion_static.hip, k_cloud.hip). It replaces the host path of test_uni.py:246-287 (six maps per view to the host,
// cv2.resize of the stage-1 / stage-2 confidences, PFM and image files) and its reader filter/dypcd.py:198-209.
//
// Per sample b with slot s = slots[b] (include/damvs.h, damvs_scene_ingest):
//   depth_store[s]        = depth[b]
//   conf_store[s][0]      = conf3[b]
//   conf_store[s][1][y][x] = conf2[b][y >> 1][x >> 1]      cv2.INTER_NEAREST at exactly x2 (mvsio.resize_nearest)
//   conf_store[s][2][y][x] = conf1[b][y >> 2][x >> 2]      exactly x4
//   rgb_store[s][y][x][c] = uint8(trunc(clip(img[b][c][y][x] * 255.0f, 0, 255)))   CHW f32 -> HWC u8
//
// VALU only, memory bound: a thread owns 4 consecutive pixels of a row, so every f32 map moves as one 16-byte access
// per thread (a wave: 1 KiB of a row), the 4 pixels' stage-2 sources are one 8-byte load, their stage-1 source one
// dword, and their 12 colour bytes three dwords (which the compiler may join into one 12-byte store). No LDS, no
// atomics, no dependency between blocks. The slot table travels in the kernel arguments (no device memory of the
// call's own: it can be captured into a graph); the slot is wave-uniform, so the per-slot bases are 64-bit scalars and
// the offsets within a view 32-bit (H * W * 12 < 2^31, checked by the C ABI). W is a multiple of 4 and the bases are
// 16-byte aligned (checked there too).
//
// This unit is linked into its own library, libdamvs_scene.so, which libdamvs.so depends on: its kernel is pinned by
// tests/isa_pins_scene.json (tests/test_scene_codeobj.py).
#include "damvs_internal.h"

namespace damvs {

namespace {

// fp32 multiply rounded to nearest, clamp, truncate: numpy's np.clip(v * 255, 0, 255).astype(uint8) in float32
__device__ __forceinline__ unsigned colour_byte(float v) {
  const float t = fminf(fmaxf(v * 255.0f, 0.0f), 255.0f);
  return (unsigned)t;
}

__global__ __launch_bounds__(kSceneBlockX* kSceneBlockY) void scene_ingest_kernel(const SceneArgs a) {
  const unsigned x4 = blockIdx.x * kSceneBlockX + threadIdx.x;  // group of 4 pixels in the row
  if (x4 >= (unsigned)a.W >> 2) return;
  const unsigned b = blockIdx.z;
  const unsigned hw = (unsigned)a.H * (unsigned)a.W;
  const size_t slot = (size_t)a.slots[b];
  const float* __restrict__ depth = a.depth + (size_t)b * hw;
  const float* __restrict__ conf3 = a.conf3 + (size_t)b * hw;
  const float* __restrict__ conf2 = a.conf2 + (size_t)b * (hw >> 2);
  const float* __restrict__ conf1 = a.conf1 + (size_t)b * (hw >> 4);
  const float* __restrict__ img = a.img ? a.img + (long long)b * a.img_bstride : nullptr;
  float* __restrict__ dst_depth = a.depth_store + slot * hw;
  float* __restrict__ dst_conf = a.conf_store + slot * 3 * hw;
  unsigned* __restrict__ dst_rgb = a.rgb_store ? reinterpret_cast<unsigned*>(a.rgb_store + slot * 3 * hw) : nullptr;
  const unsigned w2 = (unsigned)a.W >> 1, w4 = (unsigned)a.W >> 2;
  // rows: blockIdx.y strides when H / kSceneBlockY exceeds the grid's y limit (one trip at every real size)
  for (unsigned y = blockIdx.y * kSceneBlockY + threadIdx.y; y < (unsigned)a.H; y += gridDim.y * kSceneBlockY) {
    const unsigned off = y * (unsigned)a.W + 4 * x4;  // first of the 4 pixels, < H * W
    const float4 d = *reinterpret_cast<const float4*>(depth + off);
    const float4 c3 = *reinterpret_cast<const float4*>(conf3 + off);
    const float2 c2 = *reinterpret_cast<const float2*>(conf2 + (y >> 1) * w2 + 2 * x4);
    const float c1 = conf1[(y >> 2) * w4 + x4];
    *reinterpret_cast<float4*>(dst_depth + off) = d;
    *reinterpret_cast<float4*>(dst_conf + off) = c3;
    *reinterpret_cast<float4*>(dst_conf + hw + off) = make_float4(c2.x, c2.x, c2.y, c2.y);
    *reinterpret_cast<float4*>(dst_conf + 2 * hw + off) = make_float4(c1, c1, c1, c1);
    if (img) {
      const float4 r = *reinterpret_cast<const float4*>(img + off);
      const float4 g = *reinterpret_cast<const float4*>(img + hw + off);
      const float4 bl = *reinterpret_cast<const float4*>(img + 2 * hw + off);
      // bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3, little endian
      const unsigned q0 = colour_byte(r.x) | colour_byte(g.x) << 8 | colour_byte(bl.x) << 16 | colour_byte(r.y) << 24;
      const unsigned q1 = colour_byte(g.y) | colour_byte(bl.y) << 8 | colour_byte(r.z) << 16 | colour_byte(g.z) << 24;
      const unsigned q2 = colour_byte(bl.z) | colour_byte(r.w) << 8 | colour_byte(g.w) << 16 | colour_byte(bl.w) << 24;
      unsigned* o = dst_rgb + 3 * (off >> 2);  // byte 3 * off of the slot: dword aligned, 3 * off < 2^31
      o[0] = q0;
      o[1] = q1;
      o[2] = q2;
    }
  }
}

}  // namespace

hipError_t launch_scene_ingest(hipStream_t s, int B, const SceneArgs& a) {
  const unsigned gx = ((unsigned)a.W / 4 + kSceneBlockX - 1) / kSceneBlockX;
  const unsigned rows = ((unsigned)a.H + kSceneBlockY - 1) / kSceneBlockY;
  const dim3 grid(gx, rows < 32768u ? rows : 32768u, (unsigned)B);
  hipLaunchKernelGGL(scene_ingest_kernel, grid, dim3(kSceneBlockX, kSceneBlockY), 0, s, a);
  return hipGetLastError();
}

#ifndef DAMVS_BUILD_ID
#define DAMVS_BUILD_ID "unstamped"
#endif
const char* scene_build_id() { return DAMVS_BUILD_ID; }

}  // namespace damvs
