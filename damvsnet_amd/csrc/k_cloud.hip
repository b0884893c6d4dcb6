// Ordered stream compaction of one reference view's `final` pixels into PLY vertex records (SURVEY.md section 8(f)
// row f4; filter/dypcd.py:275-301, numpy's xyz[final] / color[final] in row-major pixel order): 15 bytes per point,
// x, y, z as little-endian float32 then red, green, blue, packed without padding (mvsio.write_ply's element).
// Record i of the view lands at byte (base + i) * 15 of the record buffer, base = the device cursor before the call.
//
// Three launches on the caller's stream; no block ever waits for another one:
//   count    one block per tile of kCloudTile consecutive pixels -> scratch[tile] = selected pixels of the tile
//   scan     one block: exclusive scan of scratch[0 .. ntiles) in place, in chunks of kScan; base = *cursor is kept in
//            scratch[ntiles], scratch[ntiles + 1] (low, high word) and *cursor becomes base + the view's total
//   scatter  the tiling of count: the rank inside the tile from the 64-bit wave ballot, a popcount of the lower lanes
//            and the per-wave totals through LDS; a record is written if and only if base + rank_in_view < capacity
// Order comes from the tiling and the scan alone, never from atomics. The cursor is read and written by plain loads
// and stores of the scan block, so calls that share a cursor must be enqueued on one stream (or otherwise ordered).
//
// This unit is linked into its own library, libdamvs_cloud.so, which libdamvs.so depends on: its kernels are pinned by
// tests/isa_pins_cloud.json (tests/test_cloud_codeobj.py).
#include "damvs_internal.h"

namespace damvs {

namespace {

constexpr int kRec = 15;      // bytes per record
constexpr int kScan = 1024;   // tile counts per chunk of the scan block (one per thread)
constexpr int kWaves = kCloudTile / 64;

// Rank of this thread among the block's selected threads (meaningful where sel) and the block's total.
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

__device__ __forceinline__ bool selected(const CloudArgs& a, long long p) { return p < a.n && (a.mask[p] & 4) != 0; }

__global__ __launch_bounds__(kCloudTile) void cloud_count_kernel(const CloudArgs a) {
  __shared__ unsigned wtot[kWaves];
  const long long p = (long long)blockIdx.x * kCloudTile + threadIdx.x;
  unsigned total;
  tile_rank(selected(a, p), wtot, total);
  if (threadIdx.x == 0) a.scratch[blockIdx.x] = total;
}

__global__ __launch_bounds__(kScan) void cloud_scan_kernel(unsigned* __restrict__ scratch, const unsigned ntiles,
                                                           unsigned long long* __restrict__ cursor) {
  __shared__ unsigned wsum[kScan / 64];
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned carry = 0;  // selected pixels of the chunks before this one (the same in every thread)
  for (unsigned c0 = 0; c0 < ntiles; c0 += kScan) {
    const unsigned i = c0 + threadIdx.x;
    const unsigned v = i < ntiles ? scratch[i] : 0u;
    unsigned inc = v;  // inclusive scan inside the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned t = __shfl_up(inc, d);
      if (lane >= (unsigned)d) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned before = 0, total = 0;
#pragma unroll
    for (unsigned w = 0; w < (unsigned)(kScan / 64); ++w) {
      const unsigned t = wsum[w];
      if (w < wave) before += t;
      total += t;
    }
    if (i < ntiles) scratch[i] = carry + before + inc - v;
    carry += total;
    __syncthreads();  // wsum is rewritten by the next chunk
  }
  if (threadIdx.x == 0) {
    const unsigned long long base = *cursor;
    scratch[ntiles] = (unsigned)base;
    scratch[ntiles + 1] = (unsigned)(base >> 32);
    *cursor = base + carry;
  }
}

// The tile's records are contiguous in the output: they are staged in LDS at the byte phase of their global address
// (stage[i] <-> g[i], g dword-aligned), then stored as aligned dwords with byte stores at the two ragged ends. Two
// tiles may share a dword at their seam; each writes its own bytes of it only.
__global__ __launch_bounds__(kCloudTile) void cloud_scatter_kernel(const CloudArgs a) {
  __shared__ unsigned wtot[kWaves];
  __shared__ unsigned stage32[(kCloudTile * kRec + 3) / 4 + 1];
  unsigned char* stage = reinterpret_cast<unsigned char*>(stage32);
  const long long p = (long long)blockIdx.x * kCloudTile + threadIdx.x;
  const bool sel = selected(a, p);
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
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const unsigned u = __float_as_uint(s[k]);
      d[4 * k] = (unsigned char)u;
      d[4 * k + 1] = (unsigned char)(u >> 8);
      d[4 * k + 2] = (unsigned char)(u >> 16);
      d[4 * k + 3] = (unsigned char)(u >> 24);
    }
    const unsigned char* c = a.rgb + 3 * (size_t)p;
    d[12] = c[0];
    d[13] = c[1];
    d[14] = c[2];
  }
  __syncthreads();
  unsigned char* g = reinterpret_cast<unsigned char*>(static_cast<uintptr_t>(g0 - shift));
  const unsigned end = shift + nw * kRec;                // stage[shift .. end) holds the tile's bytes; end >= 15
  const unsigned lo = shift ? 4u : 0u, hi = end & ~3u;  // aligned body stage[lo .. hi), lo <= hi
  if (threadIdx.x >= shift && threadIdx.x < lo) g[threadIdx.x] = stage[threadIdx.x];
  unsigned* g32 = reinterpret_cast<unsigned*>(g);
  for (unsigned i = lo / 4 + threadIdx.x; i < hi / 4; i += kCloudTile) g32[i] = stage32[i];
  if (threadIdx.x < end - hi) g[hi + threadIdx.x] = stage[hi + threadIdx.x];
}

}  // namespace

int fusion_cloud_tiles(long long n) { return (int)((n + kCloudTile - 1) / kCloudTile); }

hipError_t launch_fusion_cloud(hipStream_t s, const CloudArgs& a) {
  hipLaunchKernelGGL(cloud_count_kernel, dim3(a.ntiles), dim3(kCloudTile), 0, s, a);
  hipLaunchKernelGGL(cloud_scan_kernel, dim3(1), dim3(kScan), 0, s, a.scratch, a.ntiles, a.cursor);
  hipLaunchKernelGGL(cloud_scatter_kernel, dim3(a.ntiles), dim3(kCloudTile), 0, s, a);
  return hipGetLastError();
}

#ifndef DAMVS_BUILD_ID
#define DAMVS_BUILD_ID "unstamped"
#endif
const char* fusion_cloud_build_id() { return DAMVS_BUILD_ID; }

}  // namespace damvs
