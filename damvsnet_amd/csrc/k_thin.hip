// Voxel thinning of the fused point cloud: of the selected pixels of a scene's
// reference views, keep the first one, in cloud order, of every cell of an axis-aligned grid. Cloud order is the order
// of the PLY: reference views as pair.txt lists them, row-major pixels inside a view; a pixel's ordinal is
// base + pixel index, base = the pixels of the views before it (a host number).
//
// The rule (include/damvs.h, damvs_cloud_thin; fusion.voxel_first is its numpy statement):
//   q = floor(x * inv_voxel) per axis: one float32 multiply, floor, integer; in range when -2^20 <= q < 2^20 on every
//   axis (a NaN or an infinity fails the comparison); key = (qx + 2^20) | (qy + 2^20) << 21 | (qz + 2^20) << 42.
//
// One open-addressing table per scene: keys[slots] and owners[slots], 64 bits each, both all ones when empty; linear
// probing from thin_hash(key). Two launches per view on the caller's stream, one thread per pixel:
//   claim    a selected pixel walks its probe sequence; at each slot one 64-bit compare-and-swap of empty -> key; when
//            the value that comes back is empty (the slot is now this key's) or the key itself, one 64-bit unsigned
//            atomic min of the pixel's ordinal into owners[slot], and the pixel is done. Every decision rests on the
//            value a device-scope atomic returned: a slot's key never changes once it is set, so a returned key is
//            final, and no plain load of the table is made in this launch (the XCDs' L2s are not coherent for those).
//            The walk is a counted loop of at most `slots` trips: a pixel that finds no slot sets kThinFull and gives
//            up. A selected pixel out of range sets kThinRange and claims nothing. No thread waits for another.
//   resolve  a separate launch, so claim's atomics have landed: a selected pixel in range finds its key with plain
//            loads and writes keep[p] = 4 when the slot's owner is its ordinal, else 0; every other pixel writes 0.
//            keep is a mask in the form compact_cloud takes.
// A later view's ordinals are larger than an earlier view's, so a cell stays with the first view that reached it, and
// the min makes the first pixel inside a view win whatever order the threads arrive in: the result depends on neither
// the hash, the table size nor the schedule, and nothing is averaged.
//
// Contention: every pixel of a cell hits one key word and one owner word. Letting only the lowest lane of a wave with
// a given key issue the atomics would cut that; it is not done here (profiles/r19/cloud_thin.md has the cost as is).
//
// This unit is linked into its own library, libdamvs_thin.so, which libdamvs.so depends on: its kernels are pinned by
// tests/isa_pins_thin.json (tests/test_thin_codeobj.py).
#include "damvs_internal.h"

namespace damvs {

namespace {

constexpr float kLim = 1048576.f;  // 2^20

// The cell key of a point, or kThinEmpty when the point is out of range.
__device__ __forceinline__ unsigned long long cell_key(const float* __restrict__ p, const float inv) {
  const float qx = floorf(p[0] * inv), qy = floorf(p[1] * inv), qz = floorf(p[2] * inv);
  const bool ok = qx >= -kLim && qx < kLim && qy >= -kLim && qy < kLim && qz >= -kLim && qz < kLim;
  if (!ok) return kThinEmpty;
  const unsigned long long ux = (unsigned long long)((int)qx + (1 << 20));
  const unsigned long long uy = (unsigned long long)((int)qy + (1 << 20));
  const unsigned long long uz = (unsigned long long)((int)qz + (1 << 20));
  return ux | (uy << 21) | (uz << 42);
}

__global__ __launch_bounds__(kThinBlock) void thin_claim_kernel(const ThinArgs a) {
  const long long p = (long long)blockIdx.x * kThinBlock + threadIdx.x;
  if (p >= a.n || (a.mask[p] & 4) == 0) return;
  const unsigned long long key = cell_key(a.xyz + 3 * p, a.inv_voxel);
  if (key == kThinEmpty) {
    atomicOr(a.status, kThinRange);
    return;
  }
  const unsigned long long ord = a.base + (unsigned long long)p;
  unsigned long long slot = thin_hash(key, a.slots);
  for (unsigned long long trip = 0; trip < a.slots; ++trip) {
    const unsigned long long was = atomicCAS(a.keys + slot, kThinEmpty, key);
    if (was == kThinEmpty || was == key) {
      atomicMin(a.owners + slot, ord);
      return;
    }
    slot = (slot + 1ull) & (a.slots - 1ull);
  }
  atomicOr(a.status, kThinFull);
}

__global__ __launch_bounds__(kThinBlock) void thin_resolve_kernel(const ThinArgs a) {
  const long long p = (long long)blockIdx.x * kThinBlock + threadIdx.x;
  if (p >= a.n) return;
  unsigned char k = 0;
  if ((a.mask[p] & 4) != 0) {
    const unsigned long long key = cell_key(a.xyz + 3 * p, a.inv_voxel);
    if (key != kThinEmpty) {
      unsigned long long slot = thin_hash(key, a.slots);
      for (unsigned long long trip = 0; trip < a.slots; ++trip) {
        const unsigned long long at = a.keys[slot];
        if (at == key) {
          k = a.owners[slot] == a.base + (unsigned long long)p ? 4 : 0;
          break;
        }
        if (at == kThinEmpty) break;  // the table was full when this pixel claimed: kThinFull is set
        slot = (slot + 1ull) & (a.slots - 1ull);
      }
    }
  }
  a.keep[p] = k;
}

}  // namespace

hipError_t launch_cloud_thin(hipStream_t s, const ThinArgs& a) {
  const dim3 grid((unsigned)((a.n + kThinBlock - 1) / kThinBlock));  // n < 2^31: at most 2^23 blocks
  hipLaunchKernelGGL(thin_claim_kernel, grid, dim3(kThinBlock), 0, s, a);
  hipLaunchKernelGGL(thin_resolve_kernel, grid, dim3(kThinBlock), 0, s, a);
  return hipGetLastError();
}

#ifndef DAMVS_BUILD_ID
#define DAMVS_BUILD_ID "unstamped"
#endif
const char* thin_build_id() { return DAMVS_BUILD_ID; }

}  // namespace damvs
