// Phase tables of the implicit-GEMM convolutions: kernel arguments (ConvArgs / Conv2dArgs, damvs_internal.h) that the
// host packing (weight_pack.h) fills. Plain C++ without HIP types, so a host-only program can include it.
#pragma once

namespace damvs {

constexpr int kMaxPhases = 8;

// ---------------------------------------------------------------- MFMA implicit-GEMM conv3d
// A "phase" is one regular sub-convolution: for an iteration-grid point q,
//   input  coord = q * in_stride + tap_offset        (zero outside the input)
//   output coord = q * out_stride + (pd, ph, pw)
// Conv3d k3 s1/s2 has one phase with 27 taps; ConvTranspose3d k3 s2 p1 op1 is 8 phases of
// 1..8 taps each (sub-pixel decomposition), so no MFMA work is spent on structural zeros.
struct ConvPhase {
  int ntaps, kchunks, w_off, pd, ph, pw;
  signed char tap[27][4];  // dz, dy, dx, (pad)
};

// ---------------------------------------------------------------- 2D front-end convolutions
// One phase of a 2D conv / transposed conv: input = q * in_stride + tap offset, output =
// q * out_stride + (py, px). Weights for the tensor inputs are packed like the 3D kernel's
// (A-fragment order, K = taps x (c0 + c1)); geometry-plane weights are fp32 [tap][g][cout_pad].
struct Conv2dPhase {
  int ntaps, kchunks, gchunks, w_off, g_off, py, px;  // kchunks: tensor-input K chunks; gchunks: plane K chunks
  signed char tap[25][2];  // dy, dx (up to 5 x 5)
  signed char wtap[25];    // weight tap index ky*k + kx
  signed char pad_[3];
};

}  // namespace damvs
