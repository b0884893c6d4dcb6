// The body of warp_aggregate_kernel and warp_split_kernel (k_warp.hip, which describes it): a fragment, included
// inside each kernel's braces and nowhere else. It expects in scope the template parameters T, C, MODE, NVC, the
// constants BLK and S (lanes per voxel), and the kernel arguments a, cams, npix_blocks, dchunk, ndchunks.
//
// It is a fragment and not a __device__ function because the compiler does not treat the two alike: the parent's
// one-lane body moved unchanged into a __forceinline__ function of the same arguments changed all its 84 instruction
// streams (GVN then merges the view-0 camera loads of the prologue and the depth loop and keeps that ray live), which
// took the bf16 8-channel runtime-loop kernel from 95 to 100 VGPRs, i.e. from 5 to 4 waves per SIMD, and a cap back
// to 5 waves put 24 bytes per lane in scratch. Included in the kernel, 27 kernels keep their streams and none changes
// occupancy or gains scratch.
  constexpr int E = Stor<T>::E;     // channels per 16-byte chunk
  constexpr int NQ = C / E / S;     // chunks per lane
  constexpr int CL = NQ * E;        // channels per lane
  static_assert(S == 1 || (!BLK && NQ == 1 && NVC != 0 && (S == 2 || S == 4 || S == 8)),
                "channel-split form: 2, 4 or 8 lanes of one chunk each, NHWC maps, pipelined views");
  static_assert(NVC % 2 == 0 || NVC < 0, "the view pipeline alternates two register sets");
  const int hw = a.h * a.w;  // feature-map plane (computed rows: y0 .. y0 + rows - 1)
  int L = xcd_remap(blockIdx.x, npix_blocks * ndchunks * a.B);
  const int dc = L % ndchunks; L /= ndchunks;
  const int pb = L % npix_blocks;
  const int b = L / npix_blocks;
  // this batch element's [N-1][12] source cameras: block-uniform reads through a read-only, non-aliased
  // kernel argument, i.e. scalar loads into SGPRs. (Staged in LDS and read back by the compiler's wide broadcast
  // ds_read_b128 / ds_read2_b64, lanes 48-63 of some waves got wrong cameras beside U-Net kernels on another
  // stream, while ds_read_b32 reads of the same copy were always right: DESIGN.md section 4, "Concurrent streams".)
  const float* __restrict__ cam = cams + (size_t)b * (a.N - 1) * 12;
  const int q = S > 1 ? (int)(threadIdx.x & (S - 1)) : 0;  // this lane's channel chunk (S > 1)
  const int p0 = warp_pixel(a.rows, a.w, a.tiles_x, pb, (int)(threadIdx.x / S), kWarpBlock / S);  // the S lanes of a pixel are consecutive: they exit together
  // fp32: lanes past the image walk pixel 0 with their stores dropped, so every lane reaches the wave's magnitude
  // reduction at the end (the volume's prescale slot, damvs_device.h prescale_of); bf16 records no magnitude
  const bool pv = p0 >= 0;
  if (sizeof(T) == 2 && !pv) return;
  const int p = pv ? p0 : 0;
  unsigned am = 0u;
  const int yl = p / a.w, x = p - yl * a.w;
  const int y = a.y0 + yl, pg = y * a.w + x;  // reference-image row and pixel
  const float fx = (float)x, fy = (float)y;
  const float kx = (float)a.w / (float)(a.w - 1), ky = (float)a.h / (float)(a.h - 1);

  // byte geometry of a feature map: record = one pixel (NHWC) or one pixel's chunk (blocked)
  constexpr uint32_t rec = BLK ? 16u : (uint32_t)(C * sizeof(T));
  const uint32_t bbytes = (uint32_t)hw * (uint32_t)(C * sizeof(T));
  const uint32_t qstep = BLK ? (uint32_t)hw * 16u : 16u;  // bytes between a record's channel chunks
  const uint32_t sb = (uint32_t)b * bbytes;
  const uint32_t qoff = (uint32_t)q * 16u;
  const long long fbytes = (long long)a.B * bbytes;
  // chunk qq of this lane's share of the record at byte offset `off`
  auto load = [&](__amdgpu_buffer_rsrc_t r, uint32_t off, int qq) {
    return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(r, S > 1 ? off + qoff : off, sb + qq * qstep, 0));
  };

  float ref[CL];
  if (MODE != AGG_WARP_ONLY) {
    const __amdgpu_buffer_rsrc_t r0 = make_rsrc(a.feats[0], fbytes);
#pragma unroll
    for (int qq = 0; qq < NQ; ++qq) Rec16<T>::unpack(load(r0, (uint32_t)pg * rec, qq), ref + qq * E);
  }
  // this lane's channels of the weight net's first 1x1 conv: kernel-argument reads at S = 1, selects at S > 1 (no
  // dynamic kernarg indexing)
  float kq[CL];
  if constexpr (S > 1) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      float k = a.k1[e];
#pragma unroll
      for (int j = 1; j < S; ++j) k = q == j ? a.k1[j * E + e] : k;
      kq[e] = k;
    }
  }
  auto k1 = [&](int c) { if constexpr (S > 1) return kq[c]; else return a.k1[c]; };
  const float inv_n = 1.f / (float)a.N, inv_n1 = 1.f / (float)(a.N - 1);  // exact for N = 5 (the default)
  const int d0 = dc * dchunk, d1 = min(a.D, d0 + dchunk);
  auto vox_of = [&](int d) { return (((size_t)b * a.D + d) * a.out_rows + a.out_y) * a.w + p; };

  // per-channel reduction of one view's sample into the running aggregate
  auto reduce = [&](const uint4* rv, const float* wt, float* acc, float* sq) {
#pragma unroll
    for (int qq = 0; qq < NQ; ++qq) {
      float v[4][E];
#pragma unroll
      for (int k = 0; k < 4; ++k) Rec16<T>::unpack(rv[qq * 4 + k], v[k]);
      float s[E];
#pragma unroll
      for (int e = 0; e < E; ++e) s[e] = ((v[0][e] * wt[0] + v[1][e] * wt[1]) + v[2][e] * wt[2]) + v[3][e] * wt[3];
      if (MODE == AGG_WARP_ONLY) {
#pragma unroll
        for (int e = 0; e < E; ++e) acc[qq * E + e] = s[e];
      } else if (MODE == AGG_VARIANCE) {
#pragma unroll
        for (int e = 0; e < E; ++e) { acc[qq * E + e] += s[e]; sq[qq * E + e] += s[e] * s[e]; }
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const float df = ref[qq * E + e] - s[e];
          sq[qq * E + e] = df * df;  // adaptive: the squared difference, weighted below
        }
      }
    }
    if (MODE == AGG_ADAPTIVE) {
      float dot = 0.f;  // over the lane's own channels in order, then across the voxel's lanes
#pragma unroll
      for (int c = 0; c < CL; ++c) dot += k1(c) * sq[c];
      if (S >= 2) dot += dpp_xor1(dot);
      if (S >= 4) dot += dpp_xor2(dot);
      if (S == 8) dot += swz_xor4(dot);
      const float a1 = fmaxf(dot * a.s1 + a.t1, 0.f);
      const float wv = fmaxf(a1 * a.s2 + a.t2, 0.f) + 1.f;
#pragma unroll
      for (int c = 0; c < CL; ++c) acc[c] += wv * sq[c];
    }
  };
  auto finish = [&](int d, float* acc, float* sq) {
    float o[CL];
#pragma unroll
    for (int c = 0; c < CL; ++c) {
      if (MODE == AGG_VARIANCE) {
        const float mean = acc[c] * inv_n;
        o[c] = sq[c] * inv_n - mean * mean;
      } else if (MODE == AGG_ADAPTIVE) {
        o[c] = acc[c] * inv_n1;
      } else {
        o[c] = acc[c];
      }
    }
    T* dst = reinterpret_cast<T*>(a.out) + vox_of(d) * C + q * CL;
    if constexpr (sizeof(T) == 4) {
      unsigned m = am;
#pragma unroll
      for (int c = 0; c < CL; ++c) m = amax_fold(m, o[c]);
      am = pv ? m : am;
      if (pv) store_vec<T, CL>(dst, o);
    } else {
      store_vec<T, CL>(dst, o);
    }
  };
  auto init = [&](float* acc, float* sq) {
#pragma unroll
    for (int c = 0; c < CL; ++c) {
      acc[c] = (MODE == AGG_VARIANCE) ? ref[c] : 0.f;
      sq[c] = (MODE == AGG_VARIANCE) ? ref[c] * ref[c] : 0.f;
    }
  };

  // source view j = 1 + v: ray (per lane), translation (block-uniform) and descriptor, hoisted for NVC > 0
  constexpr int NH = NVC > 0 ? NVC : 1;
  const int nv = NVC > 0 ? NVC : a.N - 1;
  float rx[NH], ry[NH], rz[NH], tx[NH], ty[NH], tz[NH];
  __amdgpu_buffer_rsrc_t rs[NH];
  if constexpr (NVC > 0) {
#pragma unroll
    for (int v = 0; v < NVC; ++v) {
      const float* m = cam + v * 12;
      rx[v] = m[0] * fx + m[1] * fy + m[2];
      ry[v] = m[3] * fx + m[4] * fy + m[5];
      rz[v] = m[6] * fx + m[7] * fy + m[8];
      tx[v] = m[9];
      ty[v] = m[10];
      tz[v] = m[11];
      rs[v] = make_rsrc(a.feats[v + 1], fbytes);
    }
  }
  auto taps = [&](int v, float hyp) {
    float qx, qy, qz;
    if constexpr (NVC > 0) {
      qx = rx[v] * hyp + tx[v], qy = ry[v] * hyp + ty[v], qz = rz[v] * hyp + tz[v];
    } else {
      const float* m = cam + v * 12;
      const float vx = m[0] * fx + m[1] * fy + m[2];
      const float vy = m[3] * fx + m[4] * fy + m[5];
      const float vz = m[6] * fx + m[7] * fy + m[8];
      qx = vx * hyp + m[9], qy = vy * hyp + m[10], qz = vz * hyp + m[11];
    }
    // g = (q/qz) / ((W-1)/2) - 1 and ix = ((g + 1) W - 1) / 2 fold to ix = (q/qz) W/(W-1) - 1/2:
    // one reciprocal instead of four IEEE divisions (coordinates agree to ~1 ulp)
    const float iz = __builtin_amdgcn_rcpf(qz);
    return bilinear_taps(a.h, a.w, rec, qx * iz * kx - 0.5f, qy * iz * ky - 0.5f);
  };
  auto issue = [&](int v, const Taps& t, uint4* rv, float* wt) {
    __amdgpu_buffer_rsrc_t r;
    if constexpr (NVC > 0) r = rs[v];
    else r = make_rsrc(a.feats[v + 1], fbytes);
#pragma unroll
    for (int qq = 0; qq < NQ; ++qq)
#pragma unroll
      for (int k = 0; k < 4; ++k) rv[qq * 4 + k] = load(r, t.off[k], qq);
#pragma unroll
    for (int k = 0; k < 4; ++k) wt[k] = t.wt[k];
  };

  uint4 ra[4 * NQ], rb[4 * NQ];
  float wa[4], wb[4];
  if constexpr (NVC != 0) {
    float hyp = a.hyps[vox_of(d0)];
    float hyp_n = a.hyps[vox_of(min(d0 + 1, d1 - 1))];
    issue(0, taps(0, hyp), ra, wa);
    for (int d = d0; d < d1; ++d) {
      const float hyp_nn = a.hyps[vox_of(min(d + 2, d1 - 1))];  // two planes ahead, first in the plane's loads
      float acc[CL], sq[CL];
      init(acc, sq);
      // view v's records are in (cur, wcur); the next (view, plane)'s go to (nxt, wnxt) before v is reduced
      auto step = [&](int v, const uint4* cur, const float* wcur, uint4* nxt, float* wnxt) {
        if (v + 1 < nv) issue(v + 1, taps(v + 1, hyp), nxt, wnxt);
        else issue(0, taps(0, hyp_n), nxt, wnxt);  // next plane's first view (the last plane: a re-read)
        reduce(cur, wcur, acc, sq);
      };
      if constexpr (NVC > 0) {
#pragma unroll
        for (int v = 0; v < NVC; v += 2) {
          step(v, ra, wa, rb, wb);
          step(v + 1, rb, wb, ra, wa);
        }
      } else {
#pragma unroll 1
        for (int v = 0; v < nv; v += 2) {
          step(v, ra, wa, rb, wb);
          step(v + 1, rb, wb, ra, wa);
        }
      }
      hyp = hyp_n;
      hyp_n = hyp_nn;
      finish(d, acc, sq);
    }
  } else {
    for (int d = d0; d < d1; ++d) {
      const float hyp = a.hyps[vox_of(d)];
      float acc[CL], sq[CL];
      init(acc, sq);
      for (int v = 0; v < nv; ++v) {
        issue(v, taps(v, hyp), ra, wa);
        reduce(ra, wa, acc, sq);
      }
      finish(d, acc, sq);
    }
  }
  if constexpr (sizeof(T) == 4) amax_flush(am, a.out_amax ? a.out_amax + (size_t)b * kAmaxSlotWords : nullptr, blockIdx.x * (kWarpBlock / 64) + (int)(threadIdx.x >> 6));
