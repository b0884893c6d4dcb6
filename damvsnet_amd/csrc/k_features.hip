// Scene features: one launch gathers a batch's FeatureNet outputs from the scene's
// stores. FeatureNet's output depends on the image alone, so a scan's views go through it once each
// (scene.SceneFeatures) and every batch that lists a view copies that view's block instead of computing it again.
//
// Pair i of the launch (a sample's view; include/damvs.h, damvs_feature_gather), tensor k:
//   out[k] + i * view_bytes[k]  <-  store[k] + slots[i] * view_bytes[k]        view_bytes[k] bytes
// The kernel moves bytes: it knows nothing of dtype, h, w or C, so one launch serves the three stages' tensors (of
// different sizes) in either storage type and either FeatureNet architecture.
//
// Memory bound, 16-byte loads and stores only (view_bytes a multiple of 16 and every base 16-byte aligned, checked by
// the C ABI). The pair is blockIdx.z and the tensor blockIdx.y, so the slot, the view's size and both bases are
// wave-uniform: the slot's base is formed in 64 bits (a 49-view fp32 stage-3 store at 1184 x 1600 is 2.97 GB) and the
// offsets inside a view are 32-bit (view_bytes < 2^31). blockIdx.x strides over the view's vectors with a capped grid
// (feature_gather_grid_x): four independent vectors per thread and trip while four grid passes fit, then one per trip;
// a block whose first vector lies past a smaller tensor's end leaves at once. No LDS, no atomics, no scratch, no
// dependency between blocks. The slot table travels in the kernel arguments (no device memory of the call's own: the
// launch can be captured into a graph).
//
// This unit is linked into its own library, libdamvs_features.so, which libdamvs.so depends on: its kernel is pinned
// by tests/isa_pins_features.json (tests/test_features_codeobj.py).
#include "damvs_internal.h"

namespace damvs {

namespace {

__global__ __launch_bounds__(kFeaturesBlock) void feature_gather_kernel(const FeaturesArgs a) {
  const unsigned k = blockIdx.y, i = blockIdx.z;
  const unsigned nvec = a.nvec[k];  // < 2^27
  unsigned v = blockIdx.x * kFeaturesBlock + threadIdx.x;
  if (v >= nvec) return;
  const unsigned long long view_bytes = (unsigned long long)nvec * 16ull;
  const uint4* __restrict__ src =
      reinterpret_cast<const uint4*>(a.store[k] + (unsigned long long)(unsigned)a.slots[i] * view_bytes);
  uint4* __restrict__ dst = reinterpret_cast<uint4*>(a.out[k] + (unsigned long long)i * view_bytes);
  const unsigned pass = gridDim.x * kFeaturesBlock;  // <= 2^19: v + 3 * pass cannot wrap
  for (; v + 3 * pass < nvec; v += 4 * pass) {
    const uint4 r0 = src[v], r1 = src[v + pass], r2 = src[v + 2 * pass], r3 = src[v + 3 * pass];
    dst[v] = r0;
    dst[v + pass] = r1;
    dst[v + 2 * pass] = r2;
    dst[v + 3 * pass] = r3;
  }
  for (; v < nvec; v += pass) dst[v] = src[v];
}

}  // namespace

unsigned feature_gather_grid_x(int n_pairs, int K, unsigned max_nvec) {
  const unsigned need = (max_nvec + kFeaturesBlock - 1) / kFeaturesBlock;
  const unsigned cap = (unsigned)kFeaturesGridBlocks / (unsigned)(n_pairs * K);  // n_pairs * K <= 512
  return need < cap ? need : cap;
}

hipError_t launch_feature_gather(hipStream_t s, int n_pairs, int K, const FeaturesArgs& a) {
  unsigned max_nvec = 0;
  for (int k = 0; k < K; ++k) max_nvec = a.nvec[k] > max_nvec ? a.nvec[k] : max_nvec;
  const dim3 grid(feature_gather_grid_x(n_pairs, K, max_nvec), (unsigned)K, (unsigned)n_pairs);
  hipLaunchKernelGGL(feature_gather_kernel, grid, dim3(kFeaturesBlock), 0, s, a);
  return hipGetLastError();
}

#ifndef DAMVS_BUILD_ID
#define DAMVS_BUILD_ID "unstamped"
#endif
const char* features_build_id() { return DAMVS_BUILD_ID; }

}  // namespace damvs
