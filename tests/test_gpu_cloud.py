"""GPU: the ordered, GPU-compacted point cloud (k_cloud.hip: fusion.compact_cloud, fusion.fuse_scene).

Every comparison is exact (bytes): the kernels copy float and colour bytes and the order is that of numpy's a[final].
  1. fuse_scene over the fixture trees (tests/fusion_fixture.py) writes the PLY the reference's own filter wrote
     (tests/golden/fusion_ref.npz, through write_ply) and its mask PNGs; on the perturbed tree the files filter_depth
     writes. The fixtures hold views without a kept point (edge view 1; two of the three edge views under the static
     rule) and one empty cloud (pert, dynamic rule).
  2. compact_cloud against numpy at sizes around the tile of 256 pixels, the 64-lane wave and the scan's chunk of 1024
     tile counts (520 x 520 = 1057 tiles: two chunks), from a cursor of 7 (an odd byte offset), with poisoned borders.
  3. three views chained on one cursor without host synchronisation, also inside a side stream.
  4. overflow: records past the capacity are counted, not written; fuse_scene raises and writes no PLY.
  5. fuse_scene reads every depth PFM once.
A few seconds in total.
"""
import os

import numpy as np
import pytest
import torch

import fusion_fixture as FF
from conftest import golden

pytestmark = pytest.mark.gpu
METHODS = ("pcd", "dypcd")
REC = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
POISON = 0xA5
BASE = 7
GUARD = 64
# 1057 tiles at 520 x 520: more than one scan chunk (1024 counts); 33 x 1031 = 133 tiles, the last one ragged
SIZES = [(1, 1), (1, 63), (1, 64), (1, 65), (3, 85), (16, 16), (1, 257), (24, 40), (33, 1031), (520, 520)]
MASKS = ["zero", "all", "first", "last", "half", "sparse"]


@pytest.fixture(scope="module")
def ref():
    return golden("fusion_ref")


@pytest.fixture(scope="module")
def cases():
    return FF.cases()


@pytest.fixture(scope="module")
def fusion():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from damvsnet_amd import build, _capi, fusion
    build.build()
    _capi.load_library()
    return fusion


def make_view(H, W, kind, seed):
    """mask with byte values 0..7 (bits 1 and 2 occur without bit 4), xyz of arbitrary bit patterns, random colours."""
    rng = np.random.default_rng(seed)
    low = rng.integers(0, 4, size=(H, W), dtype=np.uint8)  # bits 1 and 2 at random everywhere
    sel = np.zeros((H, W), bool)
    if kind == "all":
        sel[:] = True
    elif kind == "first":
        sel.flat[0] = True
    elif kind == "last":
        sel.flat[-1] = True
    elif kind == "half":
        sel = rng.random((H, W)) < 0.5
    elif kind == "sparse":
        sel = rng.random((H, W)) < 0.01
    mask = (low | (sel.astype(np.uint8) << 2)).astype(np.uint8)
    xyz = rng.integers(0, 2 ** 32, size=(H, W, 3), dtype=np.uint32).view(np.float32)
    rgb = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    return mask, xyz, rgb


def expected(mask, xyz, rgb):
    m = (mask & 4) != 0
    v = np.empty(int(m.sum()), dtype=REC)
    p, c = xyz[m], rgb[m]
    v["x"], v["y"], v["z"] = p[:, 0], p[:, 1], p[:, 2]
    v["red"], v["green"], v["blue"] = c[:, 0], c[:, 1], c[:, 2]
    return v.tobytes()


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def poisoned(nbytes):
    return torch.full((nbytes,), POISON, dtype=torch.uint8, device="cuda")


# ------------------------------------------------------------------------------------------ 1. reference scenes
def run_scene(fusion, root, views, pairs, tv, method, **kw):
    FF.write_tree(root, views, pairs)
    ply = os.path.join(root, "scene.ply")
    n = fusion.fuse_scene(root, root, root, ply, conf=FF.CONF_THR, dist_base=FF.DIST_BASE,
                          rel_diff_base=FF.REL_DIFF_BASE, method=method, thres_view=tv, **kw)
    return n, ply


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("case", ["scene", "edge"])
def test_fuse_scene_equals_reference(fusion, ref, cases, case, method, tmp_path):
    from PIL import Image
    from damvsnet_amd import mvsio
    views, pairs, tv = cases[case]
    root = str(tmp_path / "tree")
    n, ply = run_scene(fusion, root, views, pairs, tv, method)
    key = "%s_%s_" % (case, method)
    want = str(tmp_path / "want.ply")
    mvsio.write_ply(want, ref[key + "xyz"], ref[key + "rgb"])
    assert open(ply, "rb").read() == open(want, "rb").read()
    assert n == len(ref[key + "xyz"])
    for i, (rv, _) in enumerate(pairs):
        for kind in ("photo", "geo", "final"):
            png = np.array(Image.open(os.path.join(root, "mask", "%08d_%s.png" % (rv, kind))))
            assert png.dtype == np.uint8 and np.array_equal(png, ref[key + kind][i].astype(np.uint8) * 255), (rv, kind)
    # the fixtures cover views whose cursor must not move
    kept = [int(ref[key + "final"][i].sum()) for i in range(len(pairs))]
    if case == "edge":
        assert kept[1] == 0 and (method != "pcd" or kept.count(0) == 2)


@pytest.mark.parametrize("method", METHODS)
def test_fuse_scene_equals_filter_depth_on_perturbed_tree(fusion, ref, cases, method, tmp_path):
    views, pairs, tv = cases["pert"]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    n, ply = run_scene(fusion, a, views, pairs, tv, method)
    FF.write_tree(b, views, pairs)
    ply_b = os.path.join(b, "scene.ply")
    n_b = fusion.filter_depth(b, b, b, ply_b, conf=FF.CONF_THR, dist_base=FF.DIST_BASE, rel_diff_base=FF.REL_DIFF_BASE,
                              method=method, thres_view=tv)
    assert n == n_b == len(ref["pert_%s_xyz" % method])
    assert open(ply, "rb").read() == open(ply_b, "rb").read()
    for rv, _ in pairs:
        for kind in ("photo", "geo", "final"):
            name = os.path.join("mask", "%08d_%s.png" % (rv, kind))
            assert open(os.path.join(a, name), "rb").read() == open(os.path.join(b, name), "rb").read(), name
    if method == "dypcd":  # an empty cloud: the header alone
        assert n == 0 and open(ply, "rb").read().endswith(b"end_header\n")


def test_fuse_scene_without_masks_writes_none(fusion, ref, cases, tmp_path):
    views, pairs, tv = cases["edge"]
    root = str(tmp_path)
    n, ply = run_scene(fusion, root, views, pairs, tv, "dypcd", save_masks=False)
    assert n == len(ref["edge_dypcd_xyz"]) and os.path.exists(ply) and not os.path.exists(os.path.join(root, "mask"))


# ------------------------------------------------------------------------------------ 2. the primitive vs numpy
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_compact_cloud_equals_numpy(fusion, size, kind):
    H, W = size
    mask, xyz, rgb = make_view(H, W, kind, seed=H * 7919 + W)
    want = expected(mask, xyz, rgb)
    count = len(want) // 15
    assert count == {"zero": 0, "all": H * W, "first": 1, "last": 1}.get(kind, count)
    records = poisoned((BASE + count) * 15 + GUARD)
    cursor = torch.tensor([BASE], dtype=torch.int64, device="cuda")
    fusion.compact_cloud(cu(mask), cu(xyz), cu(rgb), records, cursor)
    got = records.cpu().numpy().tobytes()
    assert int(cursor.item()) == BASE + count
    assert got[:BASE * 15] == bytes([POISON]) * (BASE * 15)
    assert got[BASE * 15:(BASE + count) * 15] == want
    assert got[(BASE + count) * 15:] == bytes([POISON]) * GUARD


def test_compact_cloud_at_any_byte_alignment_and_with_given_scratch(fusion):
    """records may start at any byte (a slice of a larger buffer); a scratch tensor handed in is reused as is."""
    H, W = 33, 1031
    mask, xyz, rgb = make_view(H, W, "half", seed=5)
    want = expected(mask, xyz, rgb)
    count = len(want) // 15
    m, x, c = cu(mask), cu(xyz), cu(rgb)
    scratch = None
    for off in (1, 2, 3):
        for base in (0, 1, 2, 3):
            buf = poisoned(off + (base + count) * 15 + GUARD)
            cursor = torch.tensor([base], dtype=torch.int64, device="cuda")
            scratch = fusion.compact_cloud(m, x, c, buf[off:], cursor, scratch)
            got = buf.cpu().numpy().tobytes()
            lo, hi = off + base * 15, off + (base + count) * 15
            assert int(cursor.item()) == base + count
            assert got[:lo] == bytes([POISON]) * lo and got[lo:hi] == want and got[hi:] == bytes([POISON]) * GUARD
    with pytest.raises(ValueError, match="scratch"):
        fusion.compact_cloud(m, x, c, buf, cursor, scratch[:3])


# ----------------------------------------------------------------------------------------------- 3. chaining
def chain_views():
    return [make_view(24, 40, "half", 11), make_view(1, 65, "zero", 12), make_view(33, 1031, "sparse", 13),
            make_view(16, 16, "all", 14)]


@pytest.mark.parametrize("side_stream", [False, True], ids=["default_stream", "side_stream"])
def test_views_chain_on_one_cursor_without_synchronisation(fusion, side_stream):
    views = chain_views()
    want = b"".join(expected(*v) for v in views)
    count = len(want) // 15
    dev = [tuple(cu(a) for a in v) for v in views]
    records = poisoned((BASE + count) * 15 + GUARD)
    cursor = torch.tensor([BASE], dtype=torch.int64, device="cuda")

    def enqueue():
        for m, x, c in dev:  # no host synchronisation in between
            fusion.compact_cloud(m, x, c, records, cursor)

    if side_stream:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            enqueue()
        torch.cuda.current_stream().wait_stream(s)
    else:
        enqueue()
    got = records.cpu().numpy().tobytes()
    assert int(cursor.item()) == BASE + count
    assert got[:BASE * 15] == bytes([POISON]) * (BASE * 15)
    assert got[BASE * 15:(BASE + count) * 15] == want
    assert got[(BASE + count) * 15:] == bytes([POISON]) * GUARD


# ----------------------------------------------------------------------------------------------- 4. overflow
def test_records_past_the_capacity_are_counted_not_written(fusion):
    H, W = 33, 1031
    mask, xyz, rgb = make_view(H, W, "half", seed=21)
    want = expected(mask, xyz, rgb)
    count = len(want) // 15
    m, x, c = cu(mask), cu(xyz), cu(rgb)
    capacity = BASE + count - 3
    buf = poisoned(capacity * 15 + GUARD)
    cursor = torch.tensor([BASE], dtype=torch.int64, device="cuda")
    fusion.compact_cloud(m, x, c, buf[:capacity * 15 + 14], cursor)  # len // 15 == capacity
    got = buf.cpu().numpy().tobytes()
    assert int(cursor.item()) == BASE + count
    assert got[:BASE * 15] == bytes([POISON]) * (BASE * 15)
    assert got[BASE * 15:capacity * 15] == want[:(capacity - BASE) * 15]
    assert got[capacity * 15:] == bytes([POISON]) * GUARD
    # a cursor already past the capacity: nothing is written, the count goes on
    fusion.compact_cloud(m, x, c, buf[:capacity * 15 + 14], cursor)
    assert int(cursor.item()) == BASE + 2 * count and buf.cpu().numpy().tobytes() == got


@pytest.mark.parametrize("nbytes", [0, 14])
def test_capacity_zero_only_counts(fusion, nbytes):
    mask, xyz, rgb = make_view(24, 40, "half", seed=22)
    count = len(expected(mask, xyz, rgb)) // 15
    buf = poisoned(nbytes + GUARD)
    cursor = torch.tensor([BASE], dtype=torch.int64, device="cuda")
    fusion.compact_cloud(cu(mask), cu(xyz), cu(rgb), buf[:nbytes], cursor)
    assert int(cursor.item()) == BASE + count
    assert buf.cpu().numpy().tobytes() == bytes([POISON]) * (nbytes + GUARD)


def test_fuse_scene_overflow_raises_and_writes_no_ply(fusion, ref, cases, tmp_path):
    views, pairs, tv = cases["scene"]
    count = len(ref["scene_dypcd_xyz"])
    assert count > 1
    root = str(tmp_path / "over")
    with pytest.raises(ValueError, match=r"\b%d\b" % count):
        run_scene(fusion, root, views, pairs, tv, "dypcd", max_points=count - 1)
    assert not os.path.exists(os.path.join(root, "scene.ply"))
    root = str(tmp_path / "fits")  # exactly enough room
    n, ply = run_scene(fusion, root, views, pairs, tv, "dypcd", max_points=count)
    from damvsnet_amd import mvsio
    want = str(tmp_path / "want.ply")
    mvsio.write_ply(want, ref["scene_dypcd_xyz"], ref["scene_dypcd_rgb"])
    assert n == count and open(ply, "rb").read() == open(want, "rb").read()


# ---------------------------------------------------------------------------------------------- 5. residency
def test_fuse_scene_reads_every_depth_map_once(fusion, cases, tmp_path, monkeypatch):
    from damvsnet_amd import mvsio
    views, pairs, tv = cases["scene"]
    reads = {}
    real = mvsio.read_pfm

    def counting(filename):
        reads[filename] = reads.get(filename, 0) + 1
        return real(filename)

    monkeypatch.setattr(mvsio, "read_pfm", counting)
    root = str(tmp_path)
    run_scene(fusion, root, views, pairs, tv, "dypcd")
    depth = {os.path.basename(f): n for f, n in reads.items() if os.path.basename(os.path.dirname(f)) == "depth_est"}
    used = sorted({v for r, s in pairs for v in [r] + s})
    assert sorted(depth) == ["%08d.pfm" % v for v in used]
    assert set(depth.values()) == {1}, depth
    assert set(reads.values()) == {1}, reads  # the confidences too
