// The runtime kernel-selection switches of libdamvs: one row per environment variable, and the only getenv in csrc/.
// Each one selects a kernel that a GPU test uses as a bitwise or rounding reference for the default path. Plain C++17,
// no HIP: tests/test_switches.py compiles this header alone. DESIGN.md section 4 repeats the table; this one is
// authoritative.
#pragma once

#include <atomic>
#include <cstdlib>

namespace damvs {

enum SwitchKind {
  DEFAULT_ON,   // switch_on() is false only when the value starts with '0'
  DEFAULT_OFF,  // switch_on() is true only when the value starts with '1'
  VALUE,        // switch_value(): the raw string (nullptr when unset); the caller parses it
};
enum SwitchRead {
  ONCE,  // read at first use and kept for the process (tests flip these in child processes)
  LIVE,  // read at every call (tests flip these with setenv between launches)
};

enum Switch {
  SW_PLANES4,
  SW_PLANES_MFMA,
  SW_WARP_SPLIT,
  SW_WARP_RUNTIME_VIEWS,
  SW_HALO_RS,
  SW_WIDE_RS,
  SW_WIDE_S2R1,
  SW_CONV2D_XPAIR_LDS,
  SW_CONV2D_LDS_PLANE,
  SW_CONV2D_G32,
  SW_CONV0_DZ,
  SW_CONV0_REUSE,
  SW_CONV_NO_ZSLIDE,
  SW_DECONV_NO_ZSLIDE,
  SW_CONV3D_K16,
  SW_PROB_VEC,
  SW_PROB_MFMA,
  SW_COUNT
};

struct SwitchRow {
  Switch id;
  const char* env;
  SwitchKind kind;
  SwitchRead read;
  const char* effect;
};

inline constexpr SwitchRow kSwitches[SW_COUNT] = {
    {SW_PLANES4, "DAMVS_PLANES4", DEFAULT_ON, LIVE, "0: plane-input conv2d on the one-column kernel, not the 4-column one"},
    {SW_PLANES_MFMA, "DAMVS_PLANES_MFMA", DEFAULT_ON, LIVE, "0: plane-input conv2d on the VALU kernels, not the MFMA one"},
    {SW_WARP_SPLIT, "DAMVS_WARP_SPLIT", DEFAULT_ON, ONCE, "0: one lane per voxel in every warp launch (no channel split)"},
    {SW_WARP_RUNTIME_VIEWS, "DAMVS_WARP_RUNTIME_VIEWS", DEFAULT_OFF, ONCE, "1: the runtime view loop at N = 5 / 7 too"},
    {SW_HALO_RS, "DAMVS_HALO_RS", DEFAULT_ON, LIVE, "0: fp32 32-K halo kernel without the rolling tap loop"},
    {SW_WIDE_RS, "DAMVS_WIDE_RS", DEFAULT_ON, LIVE, "0: fp32 stride-1 128-channel wide block on the AG loop, not the rolling one"},
    {SW_WIDE_S2R1, "DAMVS_WIDE_S2R1", DEFAULT_ON, LIVE, "0: fp32 stride-2 128-channel wide block on 2-row tiles, not 1-row"},
    {SW_CONV2D_XPAIR_LDS, "DAMVS_CONV2D_XPAIR_LDS", DEFAULT_ON, LIVE, "0: x-pair transposed conv2d on the gather kernel, not the LDS one"},
    {SW_CONV2D_LDS_PLANE, "DAMVS_CONV2D_LDS_PLANE", DEFAULT_ON, LIVE, "0: 3x3 layers with a plane stay on the gather kernel"},
    {SW_CONV2D_G32, "DAMVS_CONV2D_G32", DEFAULT_ON, LIVE, "0: fp32 gather layers on the 16-K form, not the 32-K one"},
    {SW_CONV0_DZ, "DAMVS_CONV0_DZ", VALUE, LIVE, "fp32 conv0 dz kernel: 0 never, 1 at every CIN, \"rp,txg\" its tile; default CIN 32"},
    {SW_CONV0_REUSE, "DAMVS_CONV0_REUSE", VALUE, LIVE, "conv0 input-plane walk: 1 at every CIN, anything else never; default by CIN"},
    {SW_CONV_NO_ZSLIDE, "DAMVS_CONV_NO_ZSLIDE", DEFAULT_OFF, LIVE, "1: conv3d layers off the z-streamed kernels"},
    {SW_DECONV_NO_ZSLIDE, "DAMVS_DECONV_NO_ZSLIDE", DEFAULT_OFF, LIVE, "1: transposed conv3d layers off the z-streamed kernels"},
    {SW_CONV3D_K16, "DAMVS_CONV3D_K16", DEFAULT_OFF, LIVE, "1: fp32 conv3d gather layers on the 16-K form, not the 32-K one"},
    {SW_PROB_VEC, "DAMVS_PROB_VEC", DEFAULT_ON, LIVE, "0: prob_mfma stores probabilities 4 bytes at a time, not 16"},
    {SW_PROB_MFMA, "DAMVS_PROB_MFMA", VALUE, LIVE, "0: VALU prob conv + regression at bf16 too; 1: the MFMA kernel at fp32 too"},
};

// The raw value of a switch (nullptr when unset). Read at every call: no VALUE switch is ONCE.
inline const char* switch_value(Switch s) { return std::getenv(kSwitches[s].env); }

// Whether a DEFAULT_ON / DEFAULT_OFF switch is on. Unset and empty values give the default.
inline bool switch_on(Switch s) {
  static std::atomic<signed char> memo[SW_COUNT];  // ONCE rows: 0 unread, 1 off, 2 on
  const SwitchRow& r = kSwitches[s];
  if (r.read == ONCE && memo[s].load(std::memory_order_relaxed)) return memo[s].load(std::memory_order_relaxed) == 2;
  const char* v = std::getenv(r.env);
  const bool on = r.kind == DEFAULT_ON ? !(v && v[0] == '0') : (v && v[0] == '1');
  if (r.read == ONCE) memo[s].store(on ? 2 : 1, std::memory_order_relaxed);
  return on;
}

}  // namespace damvs
