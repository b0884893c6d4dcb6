"""CPU: the oriented point cloud (fusion.normals_statement, the oriented PLY, damvs_fusion_normals /
damvs_fusion_cloud_oriented, the drivers' normals= option) without a GPU.

  * normals_statement, the numpy statement the kernels of k_normals.hip are compared against bit for bit
    (tests/test_gpu_normals.py): hand values on the integer scene of tests/fusion_fixture.py, tilted planes against the
    analytic normal, degenerate inputs;
  * the oriented PLY of mvsio, byte for byte;
  * the drivers refuse a bad normal_jump before they read, launch or write anything;
  * the library exports the entry points, and they refuse bad arguments with their codes before any device work.

The tilted-plane bound, 8 f 2^-24 rad: a float32 depth d is off by at most d 2^-24, which moves the point by that much
along its ray; a one-sided tangent joins two points about d / f apart, so one displaced end turns it by at most
(d 2^-24) / (d / f) = f 2^-24, both ends by 2 f 2^-24; the normal turns by at most the sum over its two tangents,
4 f 2^-24, when they are orthogonal, and a factor 2 covers tangents that are not (pixel axes seen on a plane tilted up to
70 degrees). The float64 arithmetic of the statement adds nothing visible at that scale.
"""
import ctypes
import os

import numpy as np
import pytest

import fusion_fixture as FF
import normals_fixture as NF

E_ARG, E_SHAPE = -1, -2
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORIENTED = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                     ("red", "u1"), ("green", "u1"), ("blue", "u1")])
HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
          "property float z\nproperty float nx\nproperty float ny\nproperty float nz\nproperty uchar red\n"
          "property uchar green\nproperty uchar blue\nend_header\n")


@pytest.fixture(scope="module")
def fusion():
    from damvsnet_amd import fusion
    return fusion


# ------------------------------------------------------------------------------------------------ hand values
def to_camera(x, y, d):
    """-P / |P| for the integer scene's K (its inverse is exact: P = ((x - 16) d / 64, (y - 8) d / 64, d))."""
    p0, p1, p2 = (x - 16.0) * d / 64.0, (y - 8.0) * d / 64.0, float(d)
    ln = np.sqrt(np.float64(p0 * p0 + p1 * p1 + p2 * p2))
    return np.array([-p0 / ln, -p1 / ln, -p2 / ln]).astype(np.float32)


@pytest.mark.parametrize("view", [0, 3, 7])
def test_fronto_parallel_levels_give_hand_values(fusion, view):
    v = FF.integer_views()[view]
    d = v["depth"]
    assert set(np.unique(d)) <= {16.0, 32.0, 64.0, 128.0} and len(np.unique(d)) >= 3
    rng = np.random.default_rng(view)
    final = rng.random(d.shape) < 0.6
    final[10:13, 20:23] = False
    final[11, 21] = True  # an isolated pixel
    final[0, 0], final[0, 1], final[1, 0] = True, False, False  # and one in the corner
    got = fusion.normals_statement(d, final, v["K"], v["E"], 0.01)
    assert got.dtype == np.float32 and got.shape == d.shape + (3,)
    seen = {"both": 0, "fallback": 0}
    for y in range(FF.H):
        for x in range(FF.W):
            if not final[y, x]:
                assert not got[y, x].any()
                continue
            # at jump 0.01 a neighbour counts only on the same level: the levels are a factor 2 apart
            ok = lambda yy, xx: 0 <= yy < FF.H and 0 <= xx < FF.W and final[yy, xx] and d[yy, xx] == d[y, x]
            both = (ok(y, x + 1) or ok(y, x - 1)) and (ok(y + 1, x) or ok(y - 1, x))
            want = np.array([0, 0, -1], np.float32) if both else to_camera(x, y, d[y, x])
            assert np.array_equal(got[y, x], want), (y, x, got[y, x], want)
            seen["both" if both else "fallback"] += 1
    assert seen["both"] > 100 and seen["fallback"] > 20
    assert np.array_equal(got[11, 21], to_camera(21, 11, d[11, 21])) and np.array_equal(got[0, 0], to_camera(0, 0, d[0, 0]))


def test_a_tangent_never_crosses_a_depth_step(fusion):
    """Two fronto-parallel levels side by side: with the step ignored (jump 1) the pixels beside it would tilt."""
    d = np.full((6, 8), 64, np.float32)
    d[:, 4:] = 32
    final = np.ones(d.shape, bool)
    flat = fusion.normals_statement(d, final, FF.K, FF.extrinsic((0, 0)), 0.01)
    assert np.array_equal(flat, np.broadcast_to(np.array([0, 0, -1], np.float32), flat.shape))
    crossed = fusion.normals_statement(d, final, FF.K, FF.extrinsic((0, 0)), 1.0)
    assert (crossed[:, 3:5, 0] != 0).all() and np.array_equal(crossed[:, :3], flat[:, :3])
    # the test is relative to the centre's depth: from 64 the step of 32 passes at jump 0.5, from 32 it does not
    half = fusion.normals_statement(d, final, FF.K, FF.extrinsic((0, 0)), 0.5)
    assert (half[:, 3, 0] != 0).all() and np.array_equal(half[:, 4], flat[:, 4])


# ------------------------------------------------------------------------------------------------ tilted planes
def test_tilted_planes_against_the_analytic_normal(fusion):
    planes = NF.tilted_planes()
    assert len(planes) == 60 and sorted({p["f"] for p in planes}) == [32.0, 300.0, 2900.0]
    worst = {}
    for p in planes:
        got = fusion.normals_statement(p["depth"], p["final"], p["K"], p["E"], NF.TILT_JUMP)
        sel = NF.both_tangents(p["depth"], p["final"], NF.TILT_JUMP)
        assert sel.sum() > 300
        n = got[sel]
        assert (n.astype(np.float64) @ p["normal_world"] > 0.99).all()  # the side of the camera
        assert np.abs(np.sqrt((n.astype(np.float64) ** 2).sum(1)) - 1).max() < 1e-6
        ratio = NF.angle_to(n, p["normal_world"]).max() / (p["f"] * 2.0 ** -24)
        worst[p["f"]] = max(worst.get(p["f"], 0), ratio)
        assert ratio <= 8, (p["f"], ratio)
        # the others look at the camera, which is in front of the plane too
        rest = got[p["final"] & ~sel]
        assert (rest.astype(np.float64) @ p["normal_world"] > 0).all()
        assert not got[~p["final"]].any()
    print("worst angle / (f 2^-24) per focal length:", worst)


# ------------------------------------------------------------------------------------------------ degenerate inputs
def test_degenerate_images_and_depths(fusion):
    K, E = FF.K, FF.extrinsic((2, 0))
    st = lambda d, f, jump=0.01: fusion.normals_statement(np.asarray(d, np.float32), np.asarray(f, bool), K, E, jump)
    one = st([[64]], [[True]])
    assert one.shape == (1, 1, 3) and np.array_equal(one[0, 0], to_camera(0, 0, 64))
    assert not st([[64]], [[False]]).any()
    row = st(np.full((1, 9), 64), np.ones((1, 9), bool))  # no tangent along y anywhere: all fallbacks
    col = st(np.full((7, 1), 64), np.ones((7, 1), bool))
    for x in range(9):
        assert np.array_equal(row[0, x], to_camera(x, 0, 64))
    for y in range(7):
        assert np.array_equal(col[y, 0], to_camera(0, y, 64))
    d = np.full((5, 5), 64, np.float32)
    f = np.ones((5, 5), bool)
    for bad in (np.nan, 0.0):
        dd = d.copy()
        dd[2, 2] = bad
        got = st(dd, f)
        assert not got[2, 2].any()  # NaN, and 0 / 0 in the fallback: (0, 0, 0)
        assert np.isfinite(got).all()
        # its four neighbours lose one side and keep the other: still the plane's normal
        for y, x in ((1, 2), (3, 2), (2, 1), (2, 3), (0, 0), (4, 4)):
            assert np.array_equal(got[y, x], np.array([0, 0, -1], np.float32)), (bad, y, x)
    dd = d.copy()
    dd[2, 1], dd[2, 3] = np.nan, np.nan  # the centre of the row loses both sides along x
    got = st(dd, f)
    assert np.array_equal(got[2, 2], to_camera(2, 2, 64))
    neg = st(np.full((3, 3), -64.0), np.ones((3, 3), bool))  # jump * d < 0: no neighbour is usable
    assert np.array_equal(neg[1, 1], to_camera(1, 1, -64)) and neg[1, 1, 2] > 0
    with pytest.raises(ValueError):
        st(np.zeros((3, 3)), np.ones((3, 4), bool))


@pytest.mark.parametrize("jump", [-0.01, float("nan"), float("inf"), -float("inf"), None, "0.01", True])
def test_statement_refuses_a_bad_jump(fusion, jump):
    with pytest.raises(ValueError, match="normal_jump"):
        fusion.normals_statement(np.ones((2, 2), np.float32), np.ones((2, 2), bool), FF.K, np.eye(4), jump)


# ------------------------------------------------------------------------------------------------ the PLY
def cloud(n, seed=3):
    rng = np.random.default_rng(seed)
    bits = lambda: rng.integers(0, 2 ** 32, size=(n, 3), dtype=np.uint32).view(np.float32)
    return bits(), bits(), rng.integers(0, 256, size=(n, 3), dtype=np.uint8)


@pytest.mark.parametrize("n", [0, 1, 257])
def test_oriented_ply_round_trips_byte_for_byte(n, tmp_path):
    from damvsnet_amd import mvsio
    assert mvsio.PLY_ORIENTED_RECORD_BYTES == 27 == ORIENTED.itemsize and mvsio.PLY_RECORD_BYTES == 15
    xyz, nrm, rgb = cloud(n)
    v = np.empty(n, ORIENTED)
    for k, name in enumerate(("x", "y", "z")):
        v[name], v["n" + name] = xyz[:, k], nrm[:, k]
    v["red"], v["green"], v["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    want = (HEADER % n).encode("ascii") + v.tobytes()
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    mvsio.write_ply(a, xyz, rgb, normals=nrm)
    mvsio.write_ply_records(b, v.tobytes(), normals=True)
    assert open(a, "rb").read() == want == open(b, "rb").read()
    x2, n2, c2 = mvsio.read_ply_oriented(a)
    same = lambda p, q: p.shape == q.shape and p.tobytes() == q.tobytes()  # NaN bit patterns too
    assert same(x2, xyz) and same(n2, nrm) and same(c2, rgb)
    plain = str(tmp_path / "plain.ply")
    mvsio.write_ply(plain, xyz, rgb)
    with pytest.raises(ValueError, match="oriented"):
        mvsio.read_ply_oriented(plain)


def test_oriented_records_must_be_whole_and_sizes_must_agree(tmp_path):
    from damvsnet_amd import mvsio
    ply = str(tmp_path / "no.ply")
    for nbytes in (1, 15, 26, 28, 30):
        with pytest.raises(ValueError, match="27-byte"):
            mvsio.write_ply_records(ply, bytes(nbytes), normals=True)
    with pytest.raises(ValueError, match="15-byte"):
        mvsio.write_ply_records(ply, bytes(27))
    xyz, nrm, rgb = cloud(4)
    with pytest.raises(ValueError, match="normals"):
        mvsio.write_ply(ply, xyz, rgb, normals=nrm[:3])
    assert not os.path.exists(ply)


def test_default_calls_write_the_plain_ply(tmp_path):
    from damvsnet_amd import mvsio
    xyz, _, rgb = cloud(33)
    v = np.empty(33, np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")]))
    v["x"], v["y"], v["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    v["red"], v["green"], v["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    want = (b"ply\nformat binary_little_endian 1.0\nelement vertex 33\nproperty float x\nproperty float y\n"
            b"property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n") + v.tobytes()
    names = [str(tmp_path / ("%d.ply" % i)) for i in range(4)]
    mvsio.write_ply(names[0], xyz, rgb)
    mvsio.write_ply(names[1], xyz, rgb, None)
    mvsio.write_ply_records(names[2], v.tobytes())
    mvsio.write_ply_records(names[3], v.tobytes(), False)
    for name in names:
        assert open(name, "rb").read() == want
    x2, c2 = mvsio.read_ply(names[0])  # still a 2-tuple
    assert x2.tobytes() == xyz.tobytes() and c2.tobytes() == rgb.tobytes()


# ------------------------------------------------------------------------------------------------ the drivers
BAD_JUMPS = [-1e-9, -1, float("nan"), float("inf"), "0.01", None]


@pytest.mark.parametrize("jump", BAD_JUMPS, ids=repr)
@pytest.mark.parametrize("normals", [True, False])
def test_drivers_refuse_a_bad_normal_jump_before_anything_else(jump, normals, tmp_path):
    """Nothing exists at the paths and the maps are empty: a driver that went on past the check would fail otherwise."""
    from damvsnet_amd import fusion
    from damvsnet_amd.scene import SceneMaps, reconstruct_scene
    ply, nowhere = str(tmp_path / "never.ply"), str(tmp_path / "nowhere")
    kw = dict(normals=normals, normal_jump=jump)
    with pytest.raises(ValueError, match="normal_jump"):
        fusion.fuse_scene(nowhere, nowhere, nowhere, ply, **kw)
    with pytest.raises(ValueError, match="normal_jump"):
        fusion.filter_depth(nowhere, nowhere, nowhere, ply, **kw)
    with pytest.raises(ValueError, match="normal_jump"):
        fusion.fuse_resident([(0, [1])], {}, {}, {}, {}, ply, **kw)
    with pytest.raises(ValueError, match="normal_jump"):
        SceneMaps([0, 1], 8, 8, "cpu").fuse([(0, [1])], ply, **kw)
    with pytest.raises(ValueError, match="normal_jump"):
        reconstruct_scene(None, nowhere, "scan1", ply, **kw)  # before the datapath is touched
    assert not os.path.exists(ply) and not os.path.exists(nowhere)


def test_check_normal_jump_takes_numbers(fusion):
    assert fusion.check_normal_jump(0) == 0.0 and fusion.check_normal_jump(np.float32(0.5)) == 0.5
    assert fusion.check_normal_jump(0.01) == 0.01 and isinstance(fusion.check_normal_jump(np.int64(2)), float)


# ------------------------------------------------------------------------------------------------ the library
@pytest.fixture(scope="module")
def lib():
    from damvsnet_amd import _capi, build
    build.build()
    return _capi.load_library()


def test_binding_and_header():
    from damvsnet_amd import _capi, build
    names = [s[0] for s in _capi.SIGNATURES]
    header = open(os.path.join(REPO, "include", "damvs.h")).read()
    for name in ("damvs_fusion_normals", "damvs_fusion_cloud_oriented"):
        assert name in names and name + "(" in header
    assert os.path.basename(build.NORMALS_LIB) == "libdamvs_normals.so" and build.NORMALS_UNITS == ("k_normals.hip",)


def test_library_exports_and_validates_before_device_work(lib):
    from damvsnet_amd import _capi
    assert hasattr(lib, "damvs_fusion_normals") and hasattr(lib, "damvs_fusion_cloud_oriented")
    P = 256  # never dereferenced: every call below fails validation
    err = lambda: lib.damvs_last_error_string()
    cams = _capi.DamvsFusionCams()
    C = ctypes.byref(cams)

    def normals(H=24, W=40, depth=P, mask=P, cams=C, jump=0.01, out=P):
        return lib.damvs_fusion_normals(None, H, W, depth, mask, cams, jump, out)

    def oriented(H=24, W=40, select=P, mask=P, depth=P, cams=C, jump=0.01, xyz=P, rgb=P, scratch=P, elems=6, records=P,
                 capacity=10, cursor=P):
        return lib.damvs_fusion_cloud_oriented(None, H, W, select, mask, depth, cams, jump, xyz, rgb, scratch, elems,
                                               records, capacity, cursor)

    for name in ("depth", "mask", "cams", "out"):
        assert normals(**{name: None}) == E_ARG and b"null" in err(), name
    for name in ("select", "mask", "depth", "cams", "xyz", "rgb", "scratch", "records", "cursor"):
        assert oriented(**{name: None}) == E_ARG and b"null" in err(), name
    for jump in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert normals(jump=jump) == E_ARG and b"jump" in err()
        assert oriented(jump=jump) == E_ARG and b"jump" in err()
    for H, W in ((0, 40), (24, 0), (-1, 5), (65536, 32768)):
        assert normals(H=H, W=W) == E_SHAPE and b"bad shape" in err()
        assert oriented(H=H, W=W) == E_SHAPE and b"bad shape" in err()
    assert oriented(elems=5) == E_ARG and b"scratch" in err()  # 24 x 40: 4 tiles + 2
    assert oriented(capacity=-1) == E_ARG and b"capacity" in err()
