"""CPU: the warp kernels' block -> pixel map (damvsnet_amd/csrc/warp_tiles.h: warp_tiles_x, warp_pixel_blocks,
warp_pixel, the functions both the launcher and the kernels of k_warp.hip call) covers every pixel of the computed rows
exactly once, gives -1 in every other slot, and is the map of the parent commit, whose decode carried a tile height and
a strip width in WarpArgs that the launcher always set to 8 rows and one strip of the full width.

A stand-alone program (its own main, the header alone, no device code) is compiled with the compiler the library is
built with. For every pixels-per-block count of the four lane counts (256 / 1, 2, 4, 8) and every (rows, w) it walks
all (pixel block, slot) pairs and prints one line per case."""
import subprocess

import pytest

from damvsnet_amd import build

PPB = (256, 128, 64, 32)
SHAPES = ((20, 42), (8, 32), (9, 33), (7, 5), (1, 2))

PROGRAM = r"""
#include <algorithm>
#include <cstdio>
#include <vector>
#include "warp_tiles.h"
using namespace damvs;

// The parent commit's decode, written out: WarpArgs carried tile_r, tile_sw and tiles_x.
static int parent_pixel(int rows, int w, int tile_r, int tile_sw, int tiles_x, int pb, int i, int ppb) {
  if (tile_r == 0) {
    const int p = pb * ppb + i;
    return p < rows * w ? p : -1;
  }
  const int tc = ppb / tile_r;
  const int tiles_y = (rows + tile_r - 1) / tile_r;
  const int per_strip = tile_sw * tiles_y;
  const int strip = pb / per_strip, r = pb - strip * per_strip;
  const int sw = std::min(tile_sw, tiles_x - strip * tile_sw);
  const int ty = r / sw, tx = strip * tile_sw + (r - ty * sw);
  const int tr = i / tc;
  const int x = tx * tc + (i - tr * tc), yl = ty * tile_r + tr;
  return (x < w && yl < rows) ? yl * w + x : -1;
}

int main() {
  const int ppbs[] = {%(ppbs)s};
  const int shapes[][2] = {%(shapes)s};
  for (int ppb : ppbs)
    for (const auto& sh : shapes) {
      const int rows = sh[0], w = sh[1];
      // the parent launcher's geometry: R = 8, tc = ppb / R, tiles_x = ceil(w / tc), npb = tiles_x * ceil(rows / R)
      const int tc = ppb / 8, ptx = (w + tc - 1) / tc, pnpb = ptx * ((rows + 7) / 8);
      const int tiles_x = warp_tiles_x(w, ppb);
      const int npb = warp_pixel_blocks(rows, tiles_x);
      if (tiles_x != ptx || npb != pnpb) return std::printf("geometry %%d %%d %%d\n", ppb, rows, w), 1;
      std::vector<int> seen(rows * w, 0);
      long outside = 0;
      for (int pb = 0; pb < npb; ++pb)
        for (int i = 0; i < ppb; ++i) {
          const int p = warp_pixel(rows, w, tiles_x, pb, i, ppb);
          if (p != parent_pixel(rows, w, 8, ptx, ptx, pb, i, ppb)) return std::printf("parent %%d %%d %%d: %%d %%d\n", ppb, rows, w, pb, i), 1;
          if (p < -1 || p >= rows * w) return std::printf("range %%d %%d %%d: %%d %%d -> %%d\n", ppb, rows, w, pb, i, p), 1;
          if (p < 0) ++outside;
          else ++seen[p];
        }
      for (int p = 0; p < rows * w; ++p)
        if (seen[p] != 1) return std::printf("pixel %%d of %%d %%d %%d produced %%d times\n", p, ppb, rows, w, seen[p]), 1;
      std::printf("%%d %%d %%d %%d %%ld\n", ppb, rows, w, npb, outside);
    }
  return 0;
}
"""


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("warp_tiles")
    src, exe = str(d / "warp_tiles_main.cpp"), str(d / "warp_tiles_main")
    with open(src, "w") as f:
        f.write(PROGRAM % {"ppbs": ", ".join(map(str, PPB)),
                           "shapes": ", ".join("{%d, %d}" % s for s in SHAPES)})
    r = subprocess.run([build.HIPCC, "-x", "c++", "-std=c++17", "-Wall", "-Werror", "-I" + build.CSRC, src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-400:])
    return [tuple(map(int, line.split())) for line in r.stdout.splitlines()]


def test_every_case_ran(lines):
    assert [l[:3] for l in lines] == [(ppb, rows, w) for ppb in PPB for rows, w in SHAPES]


@pytest.mark.parametrize("ppb", PPB)
def test_each_pixel_once_and_every_other_slot_outside(lines, ppb):
    """The program has checked that every pixel is produced exactly once, every slot is a pixel or -1, and every slot
    equals the parent's decode; here the counts: the slots that are no pixel are all the others."""
    for p, rows, w, npb, outside in lines:
        if p == ppb:
            assert npb == -(-w // (ppb // 8)) * -(-rows // 8), (ppb, rows, w)
            assert outside == npb * ppb - rows * w, (ppb, rows, w)
