// Fused homography warp + cross-view cost aggregation (one pass, one write of the volume).
//
// Replaces, per stage, the reference's per-source-view chain (models/cas_mvsnet.py:30-87):
//   ref_volume repeat (:30) -> homo_warping grid build + F.grid_sample (models/module.py:297-332)
//   -> (ref - warped)^2 (:66) -> AggWeightNetVolume (module.py:544-563) -> acc += (w+1) x (:73-76)
//   -> / (N-1) (:87)                                   [adaptive, the default agg_mode]
//   or  sum, sum^2 -> sq/N - (sum/N)^2 (:35-36,62-63,85) [variance]
// None of the (B,3,D,h*w) grids, (B,C,D,h,w) warped volumes or the repeated reference volume
// are materialised: one thread owns one voxel (b, d, y, x), keeps the reference C-vector and
// the running aggregate in registers, and writes the C-vector of the aggregated volume once
// (NDHWC, 16-byte stores, consecutive threads -> consecutive voxels).
//
// Warp arithmetic follows models/module.py:318-329: q = (R [x y 1]^T) d + t, u = q_x / q_z,
// g = u / ((W-1)/2) - 1 (align-corners style normalisation), then grid_sample's
// align_corners=False unnormalisation ix = ((g + 1) W - 1) / 2, bilinear, zero padding; the
// normalise/unnormalise pair is folded algebraically (ix = u W/(W-1) - 1/2).
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "damvs_device.h"

namespace damvs {

namespace {

constexpr int kWarpBlock = 256;  // threads per warp block

// One 16-byte storage record -> E floats.
template <typename T> struct Rec16;
template <> struct Rec16<float> {
  __device__ __forceinline__ static void unpack(const uint4& q, float* v) {
    v[0] = __uint_as_float(q.x); v[1] = __uint_as_float(q.y); v[2] = __uint_as_float(q.z); v[3] = __uint_as_float(q.w);
  }
};
template <> struct Rec16<bf16_t> {
  __device__ __forceinline__ static void unpack(const uint4& q, float* v) {
    const uint32_t u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = __uint_as_float(u[i] << 16);
      v[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u);
    }
  }
};

// Bilinear footprint of one sample at (ix, iy): byte offsets of the nw, ne, sw, se pixel records inside one
// batch element's map (rec bytes per record) and their weights. A corner outside the map gets the offset
// kOOB, so its buffer load returns 0: grid_sample's zero padding without a weight select. Samples far
// outside (or NaN) are moved to (-4, -4), where all four corners are outside.
struct Taps {
  uint32_t off[4];
  float wt[4];
};
__device__ __forceinline__ Taps bilinear_taps(int h, int w, uint32_t rec, float ix, float iy) {
  const bool inside = ix > -2.f && ix < (float)w + 1.f && iy > -2.f && iy < (float)h + 1.f;  // false for NaN
  const float cx = inside ? ix : -4.f, cy = inside ? iy : -4.f;
  const float x0f = floorf(cx), y0f = floorf(cy);
  const int x0 = (int)x0f, y0 = (int)y0f;
  const float wx1 = cx - x0f, wx0 = (x0f + 1.f) - cx;
  const float wy1 = cy - y0f, wy0 = (y0f + 1.f) - cy;
  Taps t;
  t.wt[0] = wx0 * wy0;
  t.wt[1] = wx1 * wy0;
  t.wt[2] = wx0 * wy1;
  t.wt[3] = wx1 * wy1;
  const bool vx0 = (unsigned)x0 < (unsigned)w, vx1 = (unsigned)(x0 + 1) < (unsigned)w;
  const bool vy0 = (unsigned)y0 < (unsigned)h, vy1 = (unsigned)(y0 + 1) < (unsigned)h;
  const uint32_t o = (uint32_t)(y0 * w + x0) * rec, ow = (uint32_t)w * rec;  // wraps for x0 / y0 = -1: fine
  t.off[0] = vx0 && vy0 ? o : kOOB;
  t.off[1] = vx1 && vy0 ? o + rec : kOOB;
  t.off[2] = vx0 && vy1 ? o + ow : kOOB;
  t.off[3] = vx1 && vy1 ? o + ow + rec : kOOB;
  return t;
}

// Linear work index of block i of n: blocks are dealt round-robin to the 8 XCDs, so XCD x gets the contiguous range
// of work that starts after the ranges of XCDs 0 .. x - 1 (bijective for any n).
__device__ __forceinline__ int xcd_remap(int i, int n) {
  const int q8 = n / 8, r8 = n % 8, x = i % 8;
  return (x < r8 ? x * (q8 + 1) : r8 * (q8 + 1) + (x - r8) * q8) + i / 8;
}

// Sum across the S lanes of a voxel: DPP quad permutes and a swizzle (VALU only, no LDS memory).
__device__ __forceinline__ float dpp_xor1(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));  // quad_perm 1,0,3,2
}
__device__ __forceinline__ float dpp_xor2(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false));  // quad_perm 2,3,0,1
}
__device__ __forceinline__ float swz_xor4(float v) {
  return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x101F));  // and 0x1F, xor 4 (no LDS memory)
}

// The one body of both kernels (k_warp_body.h, included in each): S consecutive lanes share one voxel and each owns
// NQ = C/E/S of its 16-byte channel chunks (lane q: channels q * NQ * E onwards).
//   S = 1 (warp_aggregate_kernel): one lane per voxel, all C/E chunks; NHWC or channel-blocked maps.
//   S = C/E = 2, 4 or 8 (warp_split_kernel; 8: the fp32 path's 32-channel stage-1 maps, 128-byte pixels): one chunk
//     per lane, NHWC maps. Per (voxel, view) sample each lane issues 4 loads (its chunk of the 4 bilinear corners)
//     instead of 4 S, and the S lanes of a voxel read one contiguous 16 S-byte pixel record per corner in the SAME
//     instruction: one L1 tag lookup per corner per voxel where the one-lane form needs S (the TA, not HBM, bounds the
//     gather: DESIGN.md section 6). The sample coordinates are computed redundantly by the S lanes; the adaptive weight
//     net's channel dot product is summed across them.
//
// Work decomposition (locality): a block owns kWarpBlock / S pixels of one image row band (warp_pixel) and a
// chunk of `dchunk` consecutive depth planes, and each thread walks its pixel through those planes.
// Consecutive hypotheses of one pixel sample along one epipolar segment, so a block's gathers stay
// inside a narrow band of each source image; blocks are dealt so that each XCD gets a contiguous
// range of (pixel-chunk, depth-chunk) work and its L2 holds that band (the naive (pixels, D) grid
// spreads every depth slice over all 8 XCDs and serves the gathers from the Infinity Cache).
//
// Per thread the depth-independent part of each view's homography (the ray R [x y 1]^T) is computed
// once; the cameras' translations are block-uniform (SGPRs). Gathers are buffer loads with 32-bit offsets (the
// batch element in the scalar offset; the channel chunk in the scalar offset at S = 1 and in the vector offset at
// S > 1), so a tap costs one select instead of 64-bit address arithmetic and a weight select. With NVC != 0
// the (depth, view) sequence is software-pipelined one view deep: the 4 NQ records of the next view
// (across the depth boundary too, from a hypothesis loaded a plane ahead) are in flight while the
// current view is reduced, and the loads are unconditional (the last plane re-reads its own last
// view) so the vmcnt waits count exactly. NVC > 0: the source-view count is a compile-time constant and the rays are
// hoisted out of the depth loop; NVC < 0: any even number of source views (a.N - 1, checked by the launcher), the view
// loop not unrolled and each view's ray recomputed from the SGPR camera (the same expression, so the same
// coordinates), so registers do not grow with N; NVC = 0: any view count, the plain loop (rays as for NVC < 0).

// One lane per voxel, NHWC (BLK = false) or channel-blocked (BLK = true) maps.
template <typename T, int C, int MODE, bool BLK, int NVC>
__global__ __attribute__((amdgpu_flat_work_group_size(1, kWarpBlock))) DAMVS_WAVES((sizeof(T) == 2 && C == 32 && NVC == 0 && MODE == AGG_ADAPTIVE ? 3 : 1)) void warp_aggregate_kernel(const WarpArgs a, const float* __restrict__ cams,
                                                             int npix_blocks, int dchunk, int ndchunks) {
  constexpr int S = 1;
#include "k_warp_body.h"
}

// Channel-split form: one lane per 16-byte chunk of an NHWC pixel.
template <typename T, int C, int MODE, int NVC>
__global__ __attribute__((amdgpu_flat_work_group_size(1, kWarpBlock))) void warp_split_kernel(const WarpArgs a, const float* __restrict__ cams,
                                                                int npix_blocks, int dchunk, int ndchunks) {
  constexpr bool BLK = false;
  constexpr int S = C / Stor<T>::E;
#include "k_warp_body.h"
}

// Geometry and kernel choice of one (storage type, C, mode, layout).
template <typename T, int C, int MODE, bool BLK>
hipError_t launch_k(hipStream_t s, const WarpArgs& a0) {
  constexpr int S = C * (int)sizeof(T) / 16;  // 16-byte chunks per pixel
  // 16-byte pixels: the blocked layout is the NHWC layout, one kernel serves both
  if constexpr (BLK && S == 1) return launch_k<T, C, MODE, false>(s, a0);
  else {
    WarpArgs a = a0;
    // 32-bit buffer offsets: each view's feature tensor must stay below 2 GiB
    if ((long long)a.B * a.h * a.w * C * (long long)sizeof(T) >= (1LL << 31)) return hipErrorInvalidValue;
    // Lanes per voxel: the channel-split kernel for NHWC maps of 2, 4 or 8 16-byte chunks per pixel when the view
    // pipeline takes the view count (odd N >= 3), else the one-lane kernel. DAMVS_WARP_SPLIT=0: one lane everywhere.
    const bool split = !BLK && warp_split_for(C * (int)sizeof(T), a.N);
    const int ppb = kWarpBlock / (split ? S : 1);  // pixels per block
    // Pixel blocks as tiles of kWarpTileRows = 8 rows (8 divides ppb) dealt across the full width, top to bottom
    // (warp_pixel, warp_tiles.h). The
    // 8-row tiles keep vertically adjacent pixels, whose bilinear footprints share source rows, on one CU: stage-2
    // L1 -> L2 requests -19 % and L2 hit 0.62 -> 0.71 already at 4 rows (profiles/r03/pmc_l2_tile.json); in the
    // pipeline (B=4) stage 3 1.48 -> 1.24 ms, stage 2 2.00 -> 1.82 ms, stage 1 1.40 -> 1.31 ms; 16 / 32 / 64 rows
    // slower again (profiles/r03/ab_warp_tile.jsonl).
    static_assert(kWarpBlock / 8 % kWarpTileRows == 0, "every lane count (1, 2, 4, 8) leaves whole tiles");
    a.tiles_x = warp_tiles_x(a.w, ppb);
    const int npb = warp_pixel_blocks(a.rows, a.tiles_x);
    // depth chunk: as long as possible (locality) while keeping >= ~4 blocks per CU in flight
    // (in 256-thread blocks: 512 - 32768 measured flat within 3 %, 16384+ slower in the pipeline)
    int dchunk = a.D;
    while (dchunk > 2 && (long long)npb * a.B * ((a.D + dchunk - 1) / dchunk) < 2048) dchunk = (dchunk + 1) / 2;
    const int ndc = (a.D + dchunk - 1) / dchunk;
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)(npb * ndc * a.B)), dim3(kWarpBlock), 0, s, a, a.rt, npb, dchunk, ndc);
      return hipGetLastError();
    };
    const bool runtime_views = switch_on(SW_WARP_RUNTIME_VIEWS);  // 1: the runtime view loop for N = 5 / 7 too
    if constexpr (!BLK && (S == 2 || S == 4 || S == 8)) {
      if (split) {
        // N = 5: the unrolled view loop at both storage types. Its fp32 form computed wrong voxels in lanes 48-63 beside
        // another stream's U-Net kernels while the warp unit was built with packed-FP32 VALU ops; built without them
        // (build.py FILE_FLAGS) it passes every stream case and runs 2 % faster than the runtime loop (stages 1-3: 0.520 /
        // 0.749 / 0.535 against 0.532 / 0.766 / 0.548 ms, profiles/r05/diag_streams/r05y; DESIGN.md section 4
        // "Concurrent streams")
        if (a.N == 5 && !runtime_views) return launch(warp_split_kernel<T, C, MODE, 4>);
        // N = 7 (cfgD) unrolled too, except the fp32 8-channel maps: cfgD B=4 stages 1 / 2 bf16 2.392 / 2.462 -> 2.293 /
        // 2.393 ms, fp32 3.525 / 4.240 -> 3.438 / 4.041 ms; fp32 stage 3 3.174 -> 3.233 ms stays on the runtime loop
        // (profiles/r05/ab_warp_n7)
        constexpr bool n7 = !(sizeof(T) == 4 && C == 8);
        if (a.N == 7 && !runtime_views && n7) return launch(warp_split_kernel<T, C, MODE, n7 ? 6 : 4>);
        return launch(warp_split_kernel<T, C, MODE, -1>);
      }
    }
    // One lane per voxel. View pipeline: unrolled for N = 5 (the DTU default) at 16 channels (stage 2; A/B: 2.29
    // against 2.37 ms, while stage 3 runs 1.47 against 1.50 ms on the runtime loop), a runtime view loop for any other
    // odd N (7, 11: the cfgD / cfgE benchmark configs; 3) and for 32 channels (the unrolled form needs 360 registers);
    // the plain loop for even N
    const bool pipe = a.N >= 3 && (a.N - 1) % 2 == 0;
    if constexpr (C == 16) {
      if (pipe && a.N == 5 && !runtime_views) return launch(warp_aggregate_kernel<T, C, MODE, BLK, 4>);
    }
    if (pipe) return launch(warp_aggregate_kernel<T, C, MODE, BLK, -1>);
    return launch(warp_aggregate_kernel<T, C, MODE, BLK, 0>);
  }
}

template <typename T, int MODE, bool BLK>
hipError_t launch_c(hipStream_t s, const WarpArgs& a) {
  switch (a.C) {
    case 8: return launch_k<T, 8, MODE, BLK>(s, a);
    case 16: return launch_k<T, 16, MODE, BLK>(s, a);
    case 32: return launch_k<T, 32, MODE, BLK>(s, a);
  }
  return hipErrorInvalidValue;
}


template <typename T, bool BLK>
hipError_t launch_t(hipStream_t s, int mode, const WarpArgs& a) {
  switch (mode) {
    case AGG_ADAPTIVE: return launch_c<T, AGG_ADAPTIVE, BLK>(s, a);
    case AGG_VARIANCE: return launch_c<T, AGG_VARIANCE, BLK>(s, a);
    case AGG_WARP_ONLY: return launch_c<T, AGG_WARP_ONLY, BLK>(s, a);
  }
  return hipErrorInvalidValue;
}

// [N views][B][h][w][C] -> [B][C/E][h][w][E] per view. One thread per pixel: it reads the pixel's NQ
// consecutive 16-byte chunks (one contiguous C-vector) and writes chunk q to plane q, so both the reads and
// each plane's writes are contiguous across the wave; blockIdx.y = view * B + batch element (no division).
template <int NQ>
__global__ __launch_bounds__(256) void block_channels_kernel(const FeatPtrs src, FeatPtrs dst, int B, int hw) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= hw) return;
  const int v = blockIdx.y / B, b = blockIdx.y - v * B;
  // the view's pointers by a select chain (indexing the by-value pointer arrays with v would copy them to scratch)
  const void* sv = src.p[0];
  const void* dv = dst.p[0];
#pragma unroll
  for (int i = 1; i < kMaxViews; ++i) {
    sv = v == i ? src.p[i] : sv;
    dv = v == i ? dst.p[i] : dv;
  }
  const uint4* sp = reinterpret_cast<const uint4*>(sv) + ((size_t)b * hw + p) * NQ;
  uint4* dp = const_cast<uint4*>(reinterpret_cast<const uint4*>(dv)) + (size_t)b * NQ * hw + p;
  // groups of at most 4 chunks: a register array of 6-8 uint4 was kept in scratch by hipcc
#pragma unroll
  for (int q0 = 0; q0 < NQ; q0 += 4) {
    constexpr int G = NQ < 4 ? NQ : 4;
    uint4 r[G];
#pragma unroll
    for (int q = 0; q < G; ++q)
      if (q0 + q < NQ) r[q] = sp[q0 + q];
#pragma unroll
    for (int q = 0; q < G; ++q)
      if (q0 + q < NQ) dp[(size_t)(q0 + q) * hw] = r[q];
  }
}

}  // namespace

// Whether launch_warp_aggregate runs the channel-split kernel for NHWC maps of `bytes`-byte pixels at N views (the
// predicate launch_k applies per launch; capi's feature-layout choice asks it before the maps are laid out).
bool warp_split_for(int bytes, int N) {
  return switch_on(SW_WARP_SPLIT) && (bytes == 32 || bytes == 64 || bytes == 128) && N >= 3 && (N - 1) % 2 == 0;
}

hipError_t launch_warp_aggregate(hipStream_t s, int store, int mode, const WarpArgs& a, bool blocked) {
  if (blocked) return store == ST_BF16 ? launch_t<bf16_t, true>(s, mode, a) : launch_t<float, true>(s, mode, a);
  return store == ST_BF16 ? launch_t<bf16_t, false>(s, mode, a) : launch_t<float, false>(s, mode, a);
}

hipError_t launch_block_channels(hipStream_t s, int store, const FeatPtrs& src, const FeatPtrs& dst, int N, int B,
                                 int hw, int C) {
  const int nq = C / (store == ST_BF16 ? 8 : 4);
  dim3 grid((unsigned)((hw + 255) / 256), (unsigned)(N * B));
  switch (nq) {
    case 1: hipLaunchKernelGGL(block_channels_kernel<1>, grid, dim3(256), 0, s, src, dst, B, hw); break;
    case 2: hipLaunchKernelGGL(block_channels_kernel<2>, grid, dim3(256), 0, s, src, dst, B, hw); break;
    case 3: hipLaunchKernelGGL(block_channels_kernel<3>, grid, dim3(256), 0, s, src, dst, B, hw); break;
    case 4: hipLaunchKernelGGL(block_channels_kernel<4>, grid, dim3(256), 0, s, src, dst, B, hw); break;
    case 5: hipLaunchKernelGGL(block_channels_kernel<5>, grid, dim3(256), 0, s, src, dst, B, hw); break;
    case 6: hipLaunchKernelGGL(block_channels_kernel<6>, grid, dim3(256), 0, s, src, dst, B, hw); break;
    case 7: hipLaunchKernelGGL(block_channels_kernel<7>, grid, dim3(256), 0, s, src, dst, B, hw); break;
    case 8: hipLaunchKernelGGL(block_channels_kernel<8>, grid, dim3(256), 0, s, src, dst, B, hw); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace damvs
