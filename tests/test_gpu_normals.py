"""GPU: per-point normals computed on the device (k_normals.hip: fusion.normal_map, fusion.compact_cloud's oriented form,
the drivers' normals= option).

Every comparison with fusion.normals_statement is bit equality of float32 bytes: the kernels do the statement's IEEE
double operations in its order, without contraction.
  1. normal_map_kernel against the statement at sizes around the wave, the tile of 256 pixels and a ragged last tile,
     under zero / all / sparse / half masks, on fronto-parallel integer levels, tilted planes under general cameras and
     maps with NaN, zero, infinite and negative depths, at jump 0, 0.01 and 0.5; the bytes around the output stay.
  2. the oriented compaction against numpy (xyz[sel], normals[sel], rgb[sel] at 27 bytes) at the sizes of
     tests/test_gpu_cloud.py, at every byte phase of the destination, from a non-zero cursor, chained on one cursor
     without synchronisation (default and side stream), past the capacity, at capacity 0, and with a selecting mask
     that differs from the fusion mask.
  3. the drivers on the fixture trees (tests/fusion_fixture.py) under both methods.
  4. one oriented scatter on a side stream beside a bf16 forward.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import fusion_fixture as FF
import normals_fixture as NF
from conftest import golden

pytestmark = pytest.mark.gpu
METHODS = ("pcd", "dypcd")
REC = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                ("red", "u1"), ("green", "u1"), ("blue", "u1")])
PLAIN = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
POISON = 0xA5
BASE = 7
GUARD = 64
JUMPS = (0.0, 0.01, 0.5)
MAP_SIZES = [(1, 1), (1, 63), (1, 65), (64, 1), (3, 85), (24, 40), (33, 1031)]
MAP_MASKS = ["zero", "all", "sparse", "half"]
# tests/test_gpu_cloud.py's: 1057 tiles at 520 x 520, more than one scan chunk (1024 counts)
SIZES = [(1, 1), (1, 63), (1, 64), (1, 65), (3, 85), (16, 16), (1, 257), (24, 40), (33, 1031), (520, 520)]
MASKS = ["zero", "all", "first", "last", "half", "sparse"]
HEADER_END = b"end_header\n"


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


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def poisoned(nbytes):
    return torch.full((nbytes,), POISON, dtype=torch.uint8, device="cuda")


# ------------------------------------------------------------------------------------------------ inputs
def make_mask(H, W, kind, seed):
    """Mask bytes 0..7: bits 1 and 2 at random everywhere, bit value 4 by `kind`."""
    rng = np.random.default_rng(seed)
    low = rng.integers(0, 4, size=(H, W), dtype=np.uint8)
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
    return (low | (sel.astype(np.uint8) << 2)).astype(np.uint8)


def general_camera(H, W, f, rng):
    K = np.array([[f, 0, W / 2 - 0.3], [0, f * 1.01, H / 2 + 0.2], [0, 0, 1]], np.float32)
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    Q *= np.sign(np.linalg.det(Q))
    E = np.eye(4, dtype=np.float32)
    E[:3, :3] = Q
    E[:3, 3] = rng.normal(size=3) * 100
    return K, E


def make_depth(H, W, kind, seed):
    """-> (depth (H, W) float32, K, E).
    levels: the fixture's camera and its four depth levels in blocks of 3 x 5 pixels;
    tilted: a plane tilted up to 40 degrees under a general camera (f 300 or 2900; rays may graze the plane at the wide
            sizes, the depth is then whatever the division gives);
    holes:  tilted with NaN, zero, infinite and negative entries."""
    rng = np.random.default_rng(seed)
    if kind == "levels":
        blocks = rng.choice(np.array([16, 32, 64, 128], np.float32), size=((H + 2) // 3, (W + 4) // 5))
        d = np.repeat(np.repeat(blocks, 3, 0), 5, 1)[:H, :W]
        return np.ascontiguousarray(d), FF.K.copy(), FF.extrinsic((2, -4))
    K, E = general_camera(H, W, (300.0, 2900.0)[seed % 2], rng)
    th, ph = rng.uniform(0, np.radians(40)), rng.uniform(0, 2 * np.pi)
    m = np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), -np.cos(th)])
    Kinv = np.linalg.inv(K).astype(np.float64)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    rm = sum((Kinv[i, 0] * x + Kinv[i, 1] * y + Kinv[i, 2]) * m[i] for i in range(3))
    with np.errstate(all="ignore"):
        d = (-rng.uniform(400, 900) / rm).astype(np.float32)
    if kind == "holes":
        u = rng.random((H, W))
        d[u < 0.05] = np.nan
        d[(u >= 0.05) & (u < 0.10)] = 0
        d[(u >= 0.10) & (u < 0.12)] = np.inf
        d[(u >= 0.12) & (u < 0.14)] *= -1
    return d, K, E


DEPTHS = ("levels", "tilted", "holes")


def device_map(fusion, depth, mask, K, E, jump):
    """damvs_fusion_normals into the middle of a poisoned buffer -> (normals (H, W, 3), guards untouched)."""
    from damvsnet_amd import _capi
    H, W = mask.shape
    buf = poisoned(GUARD + H * W * 12 + GUARD)
    cams = fusion.fusion_cams(K, E, [])
    _capi.check(_capi.load_library().damvs_fusion_normals(_capi.stream_ptr(buf.device), H, W, depth.data_ptr(),
                                                          mask.data_ptr(), ctypes.byref(cams), jump,
                                                          buf.data_ptr() + GUARD))
    raw = buf.cpu().numpy()
    ok = (raw[:GUARD] == POISON).all() and (raw[-GUARD:] == POISON).all()
    return raw[GUARD:-GUARD].view(np.float32).reshape(H, W, 3), ok


def first_difference(got, want):
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).reshape(-1, 3).any(1))
    return None if not len(bad) else (int(bad[0]), got.reshape(-1, 3)[bad[0]], want.reshape(-1, 3)[bad[0]], len(bad))


# ------------------------------------------------------------------------------------- 1. the map vs the statement
@pytest.mark.parametrize("kind", MAP_MASKS)
@pytest.mark.parametrize("size", MAP_SIZES, ids=lambda s: "%dx%d" % s)
def test_normal_map_equals_statement(fusion, size, kind):
    H, W = size
    mask = make_mask(H, W, kind, seed=H * 7919 + W)
    m = cu(mask)
    for i, dk in enumerate(DEPTHS):
        depth, K, E = make_depth(H, W, dk, seed=H * 31 + W + i)
        d = cu(depth)
        for jump in JUMPS:
            want = fusion.normals_statement(depth, (mask & 4) != 0, K, E, jump)
            got, guards = device_map(fusion, d, m, K, E, jump)
            assert guards, (dk, jump)
            assert first_difference(got, want) is None, (dk, jump, first_difference(got, want))
            if kind == "zero":
                assert not got.any()
            if kind == "all" and dk == "tilted" and H > 1 and W > 1:
                assert np.abs(got).max() > 0.1  # not an agreement of zeros


@pytest.mark.parametrize("f", NF.FOCALS)
def test_normal_map_equals_statement_on_the_tilted_planes(fusion, f):
    """Three of the CPU test's planes per focal length, and fusion.normal_map, the public form."""
    planes = [p for p in NF.tilted_planes() if p["f"] == f][:3]
    assert len(planes) == 3
    for p in planes:
        mask = (p["final"].astype(np.uint8) << 2) | 3
        got = fusion.normal_map(cu(p["depth"]), cu(mask), p["K"], p["E"], NF.TILT_JUMP).cpu().numpy()
        want = fusion.normals_statement(p["depth"], p["final"], p["K"], p["E"], NF.TILT_JUMP)
        assert first_difference(got, want) is None, first_difference(got, want)
        sel = NF.both_tangents(p["depth"], p["final"], NF.TILT_JUMP)
        assert NF.angle_to(got[sel], p["normal_world"]).max() <= 8 * f * 2.0 ** -24


# ------------------------------------------------------------------------------------- 2. the oriented compaction
def make_view(H, W, kind, seed, depth_kind="holes"):
    """-> dict: mask, xyz (arbitrary bit patterns), rgb, depth, K, E."""
    rng = np.random.default_rng(seed + 1000)
    depth, K, E = make_depth(H, W, depth_kind, seed)
    return {"mask": make_mask(H, W, kind, seed), "depth": depth, "K": K, "E": E,
            "xyz": rng.integers(0, 2 ** 32, size=(H, W, 3), dtype=np.uint32).view(np.float32),
            "rgb": rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)}


def expected(fusion, v, jump, select=None):
    """Records of the pixels of `select` (default: the fusion mask), their normals from the fusion mask."""
    nrm = fusion.normals_statement(v["depth"], (v["mask"] & 4) != 0, v["K"], v["E"], jump)
    m = ((v["mask"] if select is None else select) & 4) != 0
    r = np.empty(int(m.sum()), dtype=REC)
    p, n, c = v["xyz"][m], nrm[m], v["rgb"][m]
    for k, name in enumerate(("x", "y", "z")):
        r[name], r["n" + name] = p[:, k], n[:, k]
    r["red"], r["green"], r["blue"] = c[:, 0], c[:, 1], c[:, 2]
    return r.tobytes()


def on_device(v, select=None):
    d = {k: cu(v[k]) for k in ("mask", "xyz", "rgb", "depth")}
    d["select"] = d["mask"] if select is None else cu(select)
    d["cam"] = (v["K"], v["E"])
    return d


def compact(fusion, d, records, cursor, jump, scratch=None):
    return fusion.compact_cloud(d["select"], d["xyz"], d["rgb"], records, cursor, scratch, depth_avg=d["depth"],
                                cam=d["cam"], fusion_mask=d["mask"], normal_jump=jump)


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_oriented_compaction_equals_numpy(fusion, size, kind):
    H, W = size
    v = make_view(H, W, kind, seed=H * 7919 + W, depth_kind="holes" if (H + W) % 2 else "tilted")
    want = expected(fusion, v, 0.01)
    count = len(want) // 27
    assert count == {"zero": 0, "all": H * W, "first": 1, "last": 1}.get(kind, count)
    records = poisoned((BASE + count) * 27 + GUARD)
    cursor = torch.tensor([BASE], dtype=torch.int64, device="cuda")
    compact(fusion, on_device(v), records, cursor, 0.01)
    got = records.cpu().numpy().tobytes()
    assert int(cursor.item()) == BASE + count
    assert got[:BASE * 27] == bytes([POISON]) * (BASE * 27)
    assert got[BASE * 27:(BASE + count) * 27] == want
    assert got[(BASE + count) * 27:] == bytes([POISON]) * GUARD


def test_oriented_compaction_at_every_byte_phase_and_with_given_scratch(fusion):
    """records may start at any byte; 27 is odd, so the four cursors put the first record at every phase again."""
    H, W = 33, 1031
    v = make_view(H, W, "half", seed=5, depth_kind="tilted")
    want = expected(fusion, v, 0.5)
    count = len(want) // 27
    d = on_device(v)
    scratch = None
    phases = set()
    for off in (0, 1, 2, 3):
        for base in (0, 1, 2, 3):
            buf = poisoned(off + (base + count) * 27 + GUARD)
            cursor = torch.tensor([base], dtype=torch.int64, device="cuda")
            scratch = compact(fusion, d, buf[off:], cursor, 0.5, scratch)
            got = buf.cpu().numpy().tobytes()
            lo, hi = off + base * 27, off + (base + count) * 27
            phases.add((buf.data_ptr() + lo) % 4)
            assert int(cursor.item()) == base + count
            assert got[:lo] == bytes([POISON]) * lo and got[lo:hi] == want and got[hi:] == bytes([POISON]) * GUARD
    assert phases == {0, 1, 2, 3}
    with pytest.raises(ValueError, match="scratch"):
        compact(fusion, d, buf, cursor, 0.5, scratch[:3])


def chain_views():
    return [make_view(24, 40, "half", 11, "levels"), make_view(1, 65, "zero", 12), make_view(33, 1031, "sparse", 13),
            make_view(16, 16, "all", 14, "tilted")]


@pytest.mark.parametrize("side_stream", [False, True], ids=["default_stream", "side_stream"])
def test_views_chain_on_one_cursor_without_synchronisation(fusion, side_stream):
    views = chain_views()
    want = b"".join(expected(fusion, v, 0.01) for v in views)
    count = len(want) // 27
    dev = [on_device(v) for v in views]
    records = poisoned((BASE + count) * 27 + GUARD)
    cursor = torch.tensor([BASE], dtype=torch.int64, device="cuda")

    def enqueue():
        for d in dev:  # no host synchronisation in between
            compact(fusion, d, records, cursor, 0.01)

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
    assert got[:BASE * 27] == bytes([POISON]) * (BASE * 27)
    assert got[BASE * 27:(BASE + count) * 27] == want
    assert got[(BASE + count) * 27:] == bytes([POISON]) * GUARD


def test_records_past_the_capacity_are_counted_not_written(fusion):
    H, W = 33, 1031
    v = make_view(H, W, "half", seed=21)
    want = expected(fusion, v, 0.01)
    count = len(want) // 27
    d = on_device(v)
    capacity = BASE + count - 3
    buf = poisoned(capacity * 27 + GUARD)
    cursor = torch.tensor([BASE], dtype=torch.int64, device="cuda")
    compact(fusion, d, buf[:capacity * 27 + 26], cursor, 0.01)  # len // 27 == capacity
    got = buf.cpu().numpy().tobytes()
    assert int(cursor.item()) == BASE + count
    assert got[:BASE * 27] == bytes([POISON]) * (BASE * 27)
    assert got[BASE * 27:capacity * 27] == want[:(capacity - BASE) * 27]
    assert got[capacity * 27:] == bytes([POISON]) * GUARD
    # a cursor already past the capacity: nothing is written, the count goes on
    compact(fusion, d, buf[:capacity * 27 + 26], cursor, 0.01)
    assert int(cursor.item()) == BASE + 2 * count and buf.cpu().numpy().tobytes() == got


@pytest.mark.parametrize("nbytes", [0, 26])
def test_capacity_zero_only_counts(fusion, nbytes):
    v = make_view(24, 40, "half", seed=22)
    count = len(expected(fusion, v, 0.01)) // 27
    buf = poisoned(nbytes + GUARD)
    cursor = torch.tensor([BASE], dtype=torch.int64, device="cuda")
    compact(fusion, on_device(v), buf[:nbytes], cursor, 0.01)
    assert int(cursor.item()) == BASE + count
    assert buf.cpu().numpy().tobytes() == bytes([POISON]) * (nbytes + GUARD)


@pytest.mark.parametrize("size", [(24, 40), (33, 1031)], ids=lambda s: "%dx%d" % s)
def test_selection_by_keep_normals_by_the_fusion_mask(fusion, size):
    """keep is a subset of the fusion mask (bit value 4 only, as VoxelGrid.claim writes it): the selected pixels carry the
    normals the whole fusion mask gives them, which differ from the ones the thinned mask would give."""
    H, W = size
    v = make_view(H, W, "all", seed=31, depth_kind="tilted")
    rng = np.random.default_rng(32)
    keep = ((rng.random((H, W)) < 0.3).astype(np.uint8) << 2) & v["mask"]
    want = expected(fusion, v, 0.5, select=keep)
    thinned = dict(v, mask=keep)
    assert expected(fusion, thinned, 0.5) != want
    count = len(want) // 27
    assert 0 < count < H * W
    records = poisoned(count * 27 + GUARD)
    cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
    compact(fusion, on_device(v, select=keep), records, cursor, 0.5)
    got = records.cpu().numpy().tobytes()
    assert int(cursor.item()) == count and got[:count * 27] == want and got[count * 27:] == bytes([POISON]) * GUARD


def test_oriented_form_checks_its_arguments(fusion):
    v = make_view(24, 40, "half", seed=41)
    d = on_device(v)
    records, cursor = poisoned(27 * 10), torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="normal_jump"):
        compact(fusion, d, records, cursor, -1.0)
    with pytest.raises(ValueError, match="cam"):
        fusion.compact_cloud(d["mask"], d["xyz"], d["rgb"], records, cursor, depth_avg=d["depth"])
    with pytest.raises(ValueError, match="depth_avg"):
        fusion.compact_cloud(d["mask"], d["xyz"], d["rgb"], records, cursor, cam=d["cam"])
    with pytest.raises(ValueError, match="depth_avg"):
        fusion.compact_cloud(d["mask"], d["xyz"], d["rgb"], records, cursor, depth_avg=d["depth"][:3], cam=d["cam"])
    assert int(cursor.item()) == 0 and (records.cpu().numpy() == POISON).all()


# ------------------------------------------------------------------------------------------------ 3. the drivers
def split_ply(path, rec):
    data = open(path, "rb").read()
    end = data.index(HEADER_END) + len(HEADER_END)
    return data[:end], np.frombuffer(data[end:], dtype=rec)


def run_scene(fusion, root, views, pairs, tv, method, name="scene.ply", **kw):
    if not os.path.exists(os.path.join(root, "pair.txt")):
        FF.write_tree(root, views, pairs)
    ply = os.path.join(root, name)
    n = fusion.fuse_scene(root, root, root, ply, conf=FF.CONF_THR, dist_base=FF.DIST_BASE,
                          rel_diff_base=FF.REL_DIFF_BASE, method=method, thres_view=tv, **kw)
    return n, ply


def statement_normals(fusion, views, pairs, tv, method, jump):
    """normals_statement per reference view on fuse_view's depth_avg and final, the final pixels' rows concatenated."""
    out = []
    for rv, src in pairs:
        srcs = [(cu(views[s]["depth"]), views[s]["K"], views[s]["E"]) for s in src]
        r = fusion.fuse_view(cu(views[rv]["depth"]), views[rv]["K"], views[rv]["E"], srcs,
                             [cu(c) for c in views[rv]["confs"]], FF.CONF_THR, FF.DIST_BASE, FF.REL_DIFF_BASE,
                             method=method, thres_view=tv, want_normals=True, normal_jump=jump)
        fin = r["final"].cpu().numpy()
        want = fusion.normals_statement(r["depth_avg"].cpu().numpy(), fin, views[rv]["K"], views[rv]["E"], jump)
        assert first_difference(r["normal"].cpu().numpy(), want) is None  # fuse_view's 'normal' entry
        out.append(want[fin])
    return np.concatenate(out) if out else np.zeros((0, 3), np.float32)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("case", ["scene", "edge"])
def test_oriented_ply_is_the_default_ply_with_the_statements_normals(fusion, ref, cases, case, method, tmp_path):
    from damvsnet_amd import mvsio
    views, pairs, tv = cases[case]
    root = str(tmp_path / "tree")
    n0, plain = run_scene(fusion, root, views, pairs, tv, method)
    # normals=False (the default) writes the parent's bytes: the reference's own cloud
    key = "%s_%s_" % (case, method)
    want_plain = str(tmp_path / "want.ply")
    mvsio.write_ply(want_plain, ref[key + "xyz"], ref[key + "rgb"])
    assert open(plain, "rb").read() == open(want_plain, "rb").read()
    n0b, plain_b = run_scene(fusion, root, views, pairs, tv, method, name="explicit.ply", normals=False, normal_jump=0.5)
    assert n0b == n0 and open(plain_b, "rb").read() == open(plain, "rb").read()
    for jump in (0.01, 0.5):
        n1, oriented = run_scene(fusion, root, views, pairs, tv, method, name="oriented_%g.ply" % jump, normals=True,
                                 normal_jump=jump)
        head, rec = split_ply(oriented, REC)
        _, rec0 = split_ply(plain, PLAIN)
        assert n1 == n0 == len(rec) == len(rec0) and n0 > 0
        assert head == mvsio._ply_oriented_header(n0)
        for name in PLAIN.names:  # positions and colours: the default PLY's, byte for byte
            assert rec[name].tobytes() == rec0[name].tobytes(), name
        got = np.stack([rec["nx"], rec["ny"], rec["nz"]], 1)
        want = statement_normals(fusion, views, pairs, tv, method, jump)
        assert first_difference(got, want) is None, first_difference(got, want)
        # fronto-parallel scene, identity rotation: every normal has a negative z; at jump 0.01 (no tangent crosses a
        # level step) the pixels with both tangents, more than half of the masks' pixels, give exactly (0, 0, -1)
        assert (got[:, 2] < 0).all()
        assert jump != 0.01 or (got == np.array([0, 0, -1], np.float32)).all(1).mean() > 0.3
        xyz, nrm, rgb = mvsio.read_ply_oriented(oriented)
        assert xyz.tobytes() == ref[key + "xyz"].astype("<f4").tobytes() and nrm.tobytes() == got.tobytes()
        # the per-view host path writes the same file
        ply_f = os.path.join(root, "filter_%g.ply" % jump)
        n2 = fusion.filter_depth(root, root, root, ply_f, conf=FF.CONF_THR, dist_base=FF.DIST_BASE,
                                 rel_diff_base=FF.REL_DIFF_BASE, method=method, thres_view=tv, normals=True,
                                 normal_jump=jump)
        assert n2 == n1 and open(ply_f, "rb").read() == open(oriented, "rb").read()


@pytest.mark.parametrize("case,method,voxel", [("scene", "dypcd", 0.5), ("scene", "pcd", 2.0), ("edge", "dypcd", 2.0),
                                               ("edge", "pcd", 1.0)])
def test_voxel_thins_the_oriented_ply_to_voxel_firsts_indices(fusion, cases, case, method, voxel, tmp_path):
    from damvsnet_amd import mvsio
    views, pairs, tv = cases[case]
    root = str(tmp_path / "tree")
    n_full, full = run_scene(fusion, root, views, pairs, tv, method, name="full.ply", normals=True)
    _, rec = split_ply(full, REC)
    keep = fusion.voxel_first(np.stack([rec["x"], rec["y"], rec["z"]], 1), voxel)
    assert 0 < len(keep) < n_full
    n_thin, thin = run_scene(fusion, root, views, pairs, tv, method, name="thin.ply", normals=True, voxel=voxel,
                             voxel_slots=1 << 12)
    assert n_thin == len(keep)
    assert open(thin, "rb").read() == mvsio._ply_oriented_header(len(keep)) + rec[keep].tobytes()


def test_max_points_overflow_raises_and_writes_no_oriented_ply(fusion, ref, cases, tmp_path):
    views, pairs, tv = cases["scene"]
    count = len(ref["scene_dypcd_xyz"])
    root = str(tmp_path / "tree")
    with pytest.raises(ValueError, match=r"\b%d\b" % count):
        run_scene(fusion, root, views, pairs, tv, "dypcd", name="over.ply", normals=True, max_points=count - 1)
    assert not os.path.exists(os.path.join(root, "over.ply"))
    n, ply = run_scene(fusion, root, views, pairs, tv, "dypcd", name="fits.ply", normals=True, max_points=count)
    n_all, ply_all = run_scene(fusion, root, views, pairs, tv, "dypcd", name="all.ply", normals=True)
    assert n == n_all == count and open(ply, "rb").read() == open(ply_all, "rb").read()


@pytest.mark.parametrize("method", ["dypcd", "pcd"])
def test_scene_maps_fuse_normals_equals_fuse_scene_and_filter_depth(fusion, method, tmp_path):
    """The tilted-plane scene of tests/test_gpu_scene.py: the stores' path against the two paths over the saved files."""
    from test_gpu_scene import plane_maps, write_plane_tree, fuse_kw
    from test_scene import plane_case
    c = plane_case()
    maps = plane_maps()
    ply_a, ply_b, ply_c, ply_0 = (str(tmp_path / n) for n in ("a.ply", "b.ply", "c.ply", "plain.ply"))
    n_a = maps.fuse(c["pairs"], ply_a, normals=True, normal_jump=0.02, **fuse_kw(method))
    n_0 = maps.fuse(c["pairs"], ply_0, **fuse_kw(method))
    scan = write_plane_tree(str(tmp_path / "tree"))
    n_b = fusion.fuse_scene(scan, scan, scan, ply_b, normals=True, normal_jump=0.02, **fuse_kw(method))
    n_c = fusion.filter_depth(scan, scan, scan, ply_c, normals=True, normal_jump=0.02, **fuse_kw(method))
    assert n_a == n_b == n_c == n_0 > 100
    assert open(ply_a, "rb").read() == open(ply_b, "rb").read() == open(ply_c, "rb").read()
    _, rec = split_ply(ply_a, REC)
    _, rec0 = split_ply(ply_0, PLAIN)
    for name in PLAIN.names:
        assert rec[name].tobytes() == rec0[name].tobytes(), name
    nrm = np.stack([rec["nx"], rec["ny"], rec["nz"]], 1).astype(np.float64)
    length = np.sqrt((nrm ** 2).sum(1))
    assert np.abs(length - 1).max() < 1e-5  # every point got a normal, of unit length up to the float32 rotation


# ------------------------------------------------------------------------------------- 4. beside a forward
def test_oriented_scatter_on_a_side_stream_beside_a_bf16_forward(fusion):
    """One oriented compaction on a side stream while a bf16 CascadeMVSNet.forward runs on the main stream, once: the
    records equal the statement (the kernels are VALU only and carry no packed-FP32 ops,
    tests/test_normals_codeobj.py)."""
    from common import model_state, forward_inputs
    from damvsnet_amd.cascade import CascadeMVSNet
    v = make_view(33, 1031, "half", seed=80, depth_kind="tilted")
    want = expected(fusion, v, 0.01)
    count = len(want) // 27
    net = CascadeMVSNet(ndepths=[8, 8, 8], compute_dtype=torch.bfloat16, frontend_dtype=torch.bfloat16)
    net.load_state_dict(model_state("forward_160x128_48_32_8"), strict=True)
    net = net.cuda().eval()
    imgs, proj, dv, _ = forward_inputs(1, 3, 32, 64)
    imgs, dv, proj = imgs.cuda(), dv.cuda(), {k: t.cuda() for k, t in proj.items()}
    side = torch.cuda.Stream()
    d = on_device(v)
    records = poisoned((BASE + count) * 27 + GUARD)
    cursor = torch.tensor([BASE], dtype=torch.int64, device="cuda")
    scratch = torch.empty(fusion._capi.load_library().damvs_fusion_cloud_scratch(33, 1031), device="cuda",
                          dtype=torch.int32)
    torch.cuda.synchronize()  # the side stream has nothing to wait for
    with torch.no_grad():
        out = net(imgs, proj, dv, check_range=False)  # enqueued on the main stream, not waited for
    with torch.cuda.stream(side):
        compact(fusion, d, records, cursor, 0.01, scratch)
    torch.cuda.synchronize()
    net.DepthNet.check_range()
    assert out["depth"].shape == (1, 32, 64)
    got = records.cpu().numpy().tobytes()
    assert int(cursor.item()) == BASE + count
    assert got[:BASE * 27] == bytes([POISON]) * (BASE * 27)
    assert got[BASE * 27:(BASE + count) * 27] == want
    assert got[(BASE + count) * 27:] == bytes([POISON]) * GUARD
