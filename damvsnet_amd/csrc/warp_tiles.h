// Pixel tiles of the warp kernels (k_warp.hip): the block -> pixel map that the launcher sizes the grid by and the
// kernels decode. Plain integer functions without HIP types, so tests/test_warp_tiles.py compiles this header alone.
//
// A pixel block is a tile of kWarpTileRows rows x ppb / kWarpTileRows columns of the computed rows (ppb = pixels per
// block, a multiple of kWarpTileRows); the tiles are dealt across the full width, top to bottom, so the blocks in
// flight on one XCD cover a compact 2D region of the reference image.
#pragma once

#ifdef __HIPCC__
#define DAMVS_HD __host__ __device__
#else
#define DAMVS_HD
#endif

namespace damvs {

constexpr int kWarpTileRows = 8;

// tiles across a w-pixel row (WarpArgs::tiles_x)
DAMVS_HD inline int warp_tiles_x(int w, int ppb) {
  const int tc = ppb / kWarpTileRows;
  return (w + tc - 1) / tc;
}
// pixel blocks of rows x w pixels
DAMVS_HD inline int warp_pixel_blocks(int rows, int tiles_x) {
  return tiles_x * ((rows + kWarpTileRows - 1) / kWarpTileRows);
}
// Pixel (index into the rows x w computed rows) of thread slot i (0 .. ppb - 1) of pixel block pb, -1 outside them.
DAMVS_HD inline int warp_pixel(int rows, int w, int tiles_x, int pb, int i, int ppb) {
  const int tc = ppb / kWarpTileRows;
  const int ty = pb / tiles_x, tx = pb - ty * tiles_x;
  const int tr = i / tc;
  const int x = tx * tc + (i - tr * tc), yl = ty * kWarpTileRows + tr;
  return (x < w && yl < rows) ? yl * w + x : -1;
}

}  // namespace damvs
