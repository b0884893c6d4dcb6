"""CPU: the voxel-thinned point cloud (fusion.voxel_first, damvs_cloud_thin, the drivers' voxel= option) without a GPU.

  * voxel_first, the numpy statement of the rule the kernels of k_thin.hip are compared against
    (tests/test_gpu_thin.py): a subsequence, idempotent, one index per occupied cell, the first point of each cell; on
    the reference's own clouds (tests/golden/fusion_ref.npz) it keeps exactly the counts worked out for them; a point
    that is not finite or out of range is an error;
  * the C entry points refuse every bad argument with its code before any device work;
  * the binding and the header;
  * the drivers refuse a bad voxel or voxel_slots before they read, launch or write anything.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import golden

E_ARG, E_SHAPE = -1, -2
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# kept points at voxel 0.5, 1.0, 2.0
COUNTS = {"scene_dypcd": (2487, 919, 816, 224), "scene_pcd": (2018, 803, 705, 202),
          "edge_dypcd": (961, 724, 658, 223), "edge_pcd": (479, 479, 450, 194)}


@pytest.fixture(scope="module")
def lib():
    from damvsnet_amd import _capi, build
    build.build()
    return _capi.load_library()


@pytest.fixture(scope="module")
def ref():
    return golden("fusion_ref")


def lattice_cloud(n, seed, pitch=0.4, span=3, jitter=0.2):
    """n points on a coarse lattice of (2 * span + 1)^3 nodes plus jitter, both signs: cells hold several points."""
    rng = np.random.default_rng(seed)
    base = rng.integers(-span, span + 1, size=(n, 3)).astype(np.float32) * np.float32(pitch)
    return (base + rng.uniform(-jitter, jitter, size=(n, 3)).astype(np.float32)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ voxel_first
@pytest.mark.parametrize("voxel", [0.5, 0.3, 2.0])
def test_voxel_first_is_the_first_point_of_every_cell(voxel):
    from damvsnet_amd import fusion
    xyz = lattice_cloud(960, 3)
    kept = fusion.voxel_first(xyz, voxel)
    assert kept.dtype == np.int64 and np.all(np.diff(kept) > 0) and kept[0] == 0 and kept[-1] < len(xyz)  # subsequence
    cells = np.floor(xyz * (np.float32(1) / np.float32(voxel))).astype(np.int64)
    seen, want = set(), []
    for i, c in enumerate(map(tuple, cells)):  # the rule, one point at a time
        if c not in seen:
            seen.add(c)
            want.append(i)
    assert kept.tolist() == want and len(kept) == len(seen) < len(xyz)  # one index per occupied cell
    again = fusion.voxel_first(xyz[kept], voxel)
    assert again.tolist() == list(range(len(kept)))  # idempotent
    keys, ok = fusion.voxel_keys(xyz, voxel)
    assert ok.all() and len(np.unique(keys)) == len(kept) and len(np.unique(keys[kept])) == len(kept)


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_voxel_first_counts_on_the_reference_clouds(ref, name):
    from damvsnet_amd import fusion
    xyz = ref[name + "_xyz"]
    n, *want = COUNTS[name]
    assert len(xyz) == n
    got = [len(fusion.voxel_first(xyz, v)) for v in (0.5, 1.0, 2.0)]
    assert got == list(want)
    # at voxel 0.5 the views' points coincide exactly on this scene: the kept points are the distinct ones
    assert len(np.unique(xyz, axis=0)) == want[0]


def test_voxel_keys_faces_signs_and_limits():
    from damvsnet_amd import fusion
    f = np.float32
    top = np.nextafter(f(524288), f(0))  # the largest float32 below 2^19: q = 2^20 - 1 at voxel 0.5
    pts = np.array([[0, 0, 0], [-0.0, 0.25, 0.49], [0.5, 0, 0], [-0.5, 0, 0], [np.nextafter(f(-0.5), f(-1)), 0, 0],
                    [top, 0, 0], [-524288, 0, 0], [0, top, -524288]], dtype=np.float32)
    keys, ok = fusion.voxel_keys(pts, 0.5)
    assert ok.all()
    q = lambda k: [int((int(k) >> s) & 0x1FFFFF) - (1 << 20) for s in (0, 21, 42)]
    assert [q(k) for k in keys] == [[0, 0, 0], [0, 0, 0], [1, 0, 0], [-1, 0, 0], [-2, 0, 0], [(1 << 20) - 1, 0, 0],
                                    [-(1 << 20), 0, 0], [0, (1 << 20) - 1, -(1 << 20)]]
    assert fusion.voxel_first(pts, 0.5).tolist() == [0, 2, 3, 4, 5, 6, 7]  # -0.0 shares the cell of 0.0
    assert all(int(k) != 0xFFFFFFFFFFFFFFFF for k in keys)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 524288.0, -524288.5, 3e38])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_voxel_first_reports_points_out_of_range(bad, axis):
    from damvsnet_amd import fusion
    xyz = lattice_cloud(65, 4)
    xyz[41, axis] = bad
    keys, ok = fusion.voxel_keys(xyz, 0.5)
    assert ok.sum() == 64 and not ok[41] and int(keys[41]) == 0xFFFFFFFFFFFFFFFF
    with pytest.raises(ValueError, match=r"point 41 .*out of range"):
        fusion.voxel_first(xyz, 0.5)


@pytest.mark.parametrize("voxel", [0, -1, float("nan"), float("inf"), 1e-46, 1e39, "x", None])
def test_voxel_first_refuses_a_bad_voxel(voxel):
    from damvsnet_amd import fusion
    with pytest.raises(ValueError, match="voxel must be a positive finite number"):
        fusion.voxel_first(np.zeros((3, 3), np.float32), voxel)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_cloud_thin_validates_before_device_work(lib):
    P = 256  # never dereferenced: every call below fails validation
    err = lambda: lib.damvs_last_error_string()
    nbytes, home = ctypes.c_size_t(), ctypes.c_longlong()

    def call(n=960, mask=P, xyz=P, inv=2.0, base=0, table=P, slots=64, keep=P):
        return lib.damvs_cloud_thin(None, n, mask, xyz, inv, base, table, slots, keep)

    for name in ("mask", "xyz", "table", "keep"):
        assert call(**{name: None}) == E_ARG and b"null " + name.encode() in err()
    for n in (0, -1, 2 ** 31, 2 ** 40):
        assert call(n=n) == E_SHAPE and b"n %d" % n in err() and b"2^31" in err()
    for slots in (0, -64, 1, 32, 63, 65, 100, 96, 2 ** 32 + 64, 2 ** 33):
        assert call(slots=slots) == E_ARG and b"slots %d" % slots in err() and b"power of two" in err()
        assert lib.damvs_cloud_thin_table_bytes(slots, ctypes.byref(nbytes)) == E_ARG and b"slots %d" % slots in err()
        assert lib.damvs_cloud_thin_status(None, P, slots) == E_ARG and b"slots %d" % slots in err()
        assert lib.damvs_cloud_thin_clear(None, P, slots) == E_ARG and b"slots %d" % slots in err()
        assert lib.damvs_cloud_thin_hash(5, slots, ctypes.byref(home)) == E_ARG
    for inv in (0.0, -2.0, float("nan"), float("inf"), -float("inf")):
        assert call(inv=inv) == E_ARG and b"inv_voxel" in err() and b"finite and positive" in err()
    assert call(base=-1) == E_ARG and b"base -1" in err()
    assert call(table=P + 4) == E_ARG and b"8-byte aligned" in err()
    assert lib.damvs_cloud_thin_status(None, None, 64) == E_ARG and b"null table" in err()
    assert lib.damvs_cloud_thin_clear(None, None, 64) == E_ARG and b"null table" in err()
    # 16 bytes per slot and the status word
    assert lib.damvs_cloud_thin_table_bytes(64, None) == E_ARG and b"null bytes" in err()
    assert lib.damvs_cloud_thin_hash(5, 64, None) == E_ARG and b"null slot" in err()
    for slots, want in ((64, 1032), (128, 2056), (2 ** 28, 2 ** 32 + 8), (2 ** 32, 2 ** 36 + 8)):
        assert lib.damvs_cloud_thin_table_bytes(slots, ctypes.byref(nbytes)) == 0 and nbytes.value == want


def test_hash_is_a_slot_and_spreads(lib):
    from damvsnet_amd import fusion
    keys, _ = fusion.voxel_keys(lattice_cloud(960, 5), 0.3)
    cells = np.unique(keys)
    assert len(cells) > 500
    for slots in (64, 1 << 16):
        h = [fusion.voxel_home_slot(k, slots) for k in cells]
        assert min(h) >= 0 and max(h) < slots
        # neighbouring cells do not pile up: every slot of the small table is some cell's home, and in the large one
        # (load factor below 2 %) at least nine cells in ten start from a slot of their own
        assert len(set(h)) == 64 if slots == 64 else len(set(h)) > 0.9 * len(cells)
    assert fusion.voxel_home_slot(0, 64) == 0


def test_binding_and_header():
    from damvsnet_amd import _capi, fusion
    names = [s[0] for s in _capi.SIGNATURES]
    for name in ("damvs_cloud_thin", "damvs_cloud_thin_table_bytes", "damvs_cloud_thin_status", "damvs_cloud_thin_clear",
                 "damvs_cloud_thin_hash"):
        assert name in names
        assert name + "(" in open(os.path.join(REPO, "include", "damvs.h")).read()
    assert callable(fusion.voxel_first) and callable(fusion.VoxelGrid) and fusion.VOXEL_Q == 1 << 20


# ------------------------------------------------------------------------------------------------ the drivers
BAD = [dict(voxel=0), dict(voxel=-1), dict(voxel=float("nan")), dict(voxel=float("inf")),
       dict(voxel=0.5, voxel_slots=100), dict(voxel=0.5, voxel_slots=32), dict(voxel=0.5, voxel_slots=64.0),
       dict(voxel_slots=128)]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
def test_drivers_refuse_bad_voxel_arguments_before_anything_else(kw, tmp_path):
    """Nothing exists at the paths and the maps are empty: a driver that went on past the check would fail otherwise."""
    from damvsnet_amd import fusion
    from damvsnet_amd.scene import SceneMaps, reconstruct_scene
    ply, nowhere = str(tmp_path / "never.ply"), str(tmp_path / "nowhere")
    match = "voxel_slots" if "voxel_slots" in kw else "voxel must be"
    with pytest.raises(ValueError, match=match):
        fusion.fuse_scene(nowhere, nowhere, nowhere, ply, **kw)
    with pytest.raises(ValueError, match=match):
        fusion.fuse_resident([(0, [1])], {}, {}, {}, {}, ply, **kw)
    with pytest.raises(ValueError, match=match):
        SceneMaps([0, 1], 8, 8, "cpu").fuse([(0, [1])], ply, **kw)
    with pytest.raises(ValueError, match=match):
        reconstruct_scene(None, nowhere, "scan1", ply, **kw)
    if "voxel" in kw:
        with pytest.raises(ValueError, match=match):
            fusion.VoxelGrid(kw["voxel"], kw.get("voxel_slots", 64), "cpu")
    assert not os.path.exists(ply) and not os.path.exists(nowhere)


def test_default_slots_are_the_power_of_two_at_or_above_twice_the_pixels():
    from damvsnet_amd import fusion
    assert [fusion._voxel_slots(None, n) for n in (1, 31, 32, 33, 960, 5760, 2 ** 20, 2 ** 20 + 1)] == \
        [64, 64, 64, 128, 2048, 16384, 2 ** 21, 2 ** 22]
    assert fusion._voxel_slots(None, 49 * 1184 * 1600) == 2 ** 28  # the docstring's 4.3 GB
