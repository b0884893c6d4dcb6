// Static-threshold depth fusion for one reference view (filter/pcd.py, the reference's
// --filter_method pcd): the reprojection, arithmetic and outputs of fusion_view_kernel (k_fusion.hip) with one fixed
// pair of thresholds per source and a fixed count of agreeing views.
//
// This unit is linked into its own library, libdamvs_fusion.so, which libdamvs.so depends on: its kernel is pinned by
// tests/isa_pins_fusion.json (tests/test_fusion_static_codeobj.py), the kernels of libdamvs.so by tests/isa_pins.json.
#include "fusion_device.h"

namespace damvs {

namespace {

// The static rule (filter/pcd.py:58-113, 142-170, 190-208; the CasMVSNet filter): the same reprojection per source
// view, one fixed mask per source (dist < dist_thr[0] in float64, relative depth difference < rel_thr[0] in float32),
// geo = at least thres_view agreeing sources. pcd.py:90-91 divides by the reprojected z as it is (no zero guard): a
// zero gives inf / NaN and every comparison with NaN is false.
__global__ __launch_bounds__(256) void fusion_view_static_kernel(const FusionArgs a, const int thres_view) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.H * a.W) return;
  const int y = p / a.W, x = p - y * a.W;
  const float dref = a.depth_ref[p];
  const double v0[3] = {(double)x * (double)dref, (double)y * (double)dref, (double)dref};
  double xyz_ref[3];
  mv3(a.kinv_ref, v0, xyz_ref);
  float sum_rep = 0.f;
  int geo_sum = 0;
  for (int v = 0; v < a.nsrc; ++v) {
    const FusionCam& c = a.src[v];
    double xs[3], kxs[3];
    mv34(c.t_sr, xyz_ref, xs);
    mv3(c.k_src, xs, kxs);
    const double xsd = kxs[0] / kxs[2], ysd = kxs[1] / kxs[2];
    const float sampled = remap_linear(a.depth_src[v], a.H, a.W, (float)xsd, (float)ysd);
    const double v1[3] = {xsd * (double)sampled, ysd * (double)sampled, (double)sampled};
    double xs2[3], xr[3], kxr[3];
    mv3(c.kinv_src, v1, xs2);
    mv34(c.t_rs, xs2, xr);
    const float depth_rep = (float)xr[2];
    mv3(a.k_ref, xr, kxr);
    const float xrep = (float)(kxr[0] / kxr[2]), yrep = (float)(kxr[1] / kxr[2]);
    const double dx = (double)xrep - (double)x, dy = (double)yrep - (double)y;
    const double dist = sqrt(dx * dx + dy * dy);
    const float rel = __fdiv_rn(fabsf(__fsub_rn(depth_rep, dref)), dref);
    if (dist < a.dist_thr[0] && rel < a.rel_thr[0]) {
      ++geo_sum;
      sum_rep = __fadd_rn(sum_rep, depth_rep);
    }
  }
  // (sum of agreeing reprojected depths + ref) / (count + 1): float32 sum, float64 division (pcd.py:167)
  const double davg = (double)__fadd_rn(sum_rep, dref) / (double)(geo_sum + 1);
  const bool geo = geo_sum >= thres_view;
  bool photo = true;
  if (a.conf[0]) photo = a.conf[0][p] > a.conf_thr[2] && a.conf[1][p] > a.conf_thr[1] && a.conf[2][p] > a.conf_thr[0];
  const bool fin = photo && geo;
  a.depth_avg[p] = (float)davg;
  a.mask[p] = (unsigned char)((photo ? 1 : 0) | (geo ? 2 : 0) | (fin ? 4 : 0));
  if (a.xyz) {
    float o[3] = {0.f, 0.f, 0.f};
    if (fin) {
      const double v2[3] = {(double)x * davg, (double)y * davg, davg};
      double cam[3], w[3];
      mv3(a.kinv_ref, v2, cam);
      mv34(a.einv_ref, cam, w);
      o[0] = (float)w[0]; o[1] = (float)w[1]; o[2] = (float)w[2];
    }
    a.xyz[3 * (size_t)p] = o[0];
    a.xyz[3 * (size_t)p + 1] = o[1];
    a.xyz[3 * (size_t)p + 2] = o[2];
  }
}

}  // namespace

hipError_t launch_fusion_view_static(hipStream_t s, const FusionArgs& a, int thres_view) {
  const long long n = (long long)a.H * a.W;
  hipLaunchKernelGGL(fusion_view_static_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, thres_view);
  return hipGetLastError();
}

#ifndef DAMVS_BUILD_ID
#define DAMVS_BUILD_ID "unstamped"
#endif
const char* fusion_static_build_id() { return DAMVS_BUILD_ID; }

}  // namespace damvs
