"""GPU: the voxel-thinned point cloud (k_thin.hip: fusion.VoxelGrid, the voxel= option of the scene-level drivers).

Every comparison is exact (bytes): the kernels decide which pixels are kept and copy nothing; the statement is
fusion.voxel_first (tests/test_thin.py), applied to the selected pixels in order.
  1. VoxelGrid.claim against voxel_first at 1 to 960 points (one thread, the 64-lane wave, the block of 256 and more than
     one block) on a coarse lattice plus jitter, so that most cells hold several points; masks all / none / random /
     random bytes (only bit value 4 selects); voxels 0.5 and 0.3; negative coordinates, points on cell faces, -0.0 and
     the first and last cell index; keep poisoned beforehand, guard bands around keep and around the table.
  2. probing in a table of 64 slots: 48 cells of which several start from the last two slots (chains and the wrap past
     the last slot must occur, whatever the order of arrival), exactly 64 cells, and 65 cells: the table-full error.
  3. contention: 10 240 selected points in 7 cells, three runs, the same bytes.
  4. two and three views chained on one table without synchronisation, on the default and on a side stream.
  5. a selected point that is NaN, infinite or one cell past the range raises the range error; unselected it is ignored.
  6. the drivers on the fixture trees (tests/fusion_fixture.py): the thinned PLY is the voxel=None PLY's records at
     voxel_first's indices, the mask PNGs are unchanged; SceneMaps.fuse against fuse_scene; reconstruct_scene against
     thinning its own default PLY; max_points bounds the thinned count.
  7. one claim on a side stream beside a bf16 forward.
A few seconds in total.
"""
import os

import numpy as np
import pytest
import torch

import fusion_fixture as FF
from conftest import golden
from test_thin import COUNTS, lattice_cloud

pytestmark = pytest.mark.gpu
POISON = 0xA5
GUARD = 64
SIZES = [1, 63, 64, 65, 257, 960]
MASKS = ["all", "none", "random", "bytes"]
HEADER_END = b"end_header\n"


@pytest.fixture(scope="module")
def fusion():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from damvsnet_amd import build, _capi, fusion
    build.build()
    _capi.load_library()
    return fusion


@pytest.fixture(scope="module")
def ref():
    return golden("fusion_ref")


@pytest.fixture(scope="module")
def cases():
    return FF.cases()


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_mask(n, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "bytes":  # every bit at random: only bit value 4 selects
        return rng.integers(0, 256, size=n, dtype=np.uint8)
    low = rng.integers(0, 4, size=n, dtype=np.uint8)  # bits 1 and 2 at random, as the fusion kernels write them
    sel = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "random": rng.random(n) < 0.6}[kind]
    if kind == "none":
        low |= rng.integers(0, 2, size=n, dtype=np.uint8) * np.uint8(0xF8)  # the other bits select nothing
    return (low | (sel.astype(np.uint8) << 2)).astype(np.uint8)


def special_points(voxel):
    """Points on cell faces, -0.0, and two points in the first and in the last cell of the x axis with one in the cell
    beside each (the numpy side asserts the indices)."""
    f = np.float32
    inv = f(1) / f(voxel)
    hi, lo = (1 << 20) - 1, -((1 << 20) - 1)
    edge = lambda q, t: f((q + t) / float(inv))
    pts = [[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [0.5, -0.5, 1.0], [0.5, -0.5, 1.25], [-1.5, 2.0, -2.5],
           [edge(hi, 0.5), 0.1, 0.1], [edge(hi, 0.25), 0.1, 0.1], [edge(hi - 1, 0.5), 0.1, 0.1],
           [edge(lo, 0.5), 0.1, 0.1], [edge(lo, 0.25), 0.1, 0.1], [edge(lo + 1, 0.5), 0.1, 0.1],
           [0.1, edge(hi, 0.5), edge(lo, 0.5)]]
    pts = np.array(pts, dtype=np.float32)
    q = np.floor(pts * inv).astype(np.int64)
    assert q[5, 0] == q[6, 0] == hi and q[7, 0] == hi - 1 and q[8, 0] == q[9, 0] == lo and q[10, 0] == lo + 1
    assert q[11, 1] == hi and q[11, 2] == lo
    return pts


def make_cloud(n, voxel, seed):
    # 125 nodes 0.4 apart, jitter of 0.05: a node's points share a cell of either grid unless the node sits on a face
    xyz = lattice_cloud(n, seed, span=2, jitter=0.05)
    sp = special_points(voxel)
    if n >= 63:
        at = np.random.default_rng(seed + 1).permutation(n)[:len(sp)]
        xyz[np.sort(at)] = sp
    prod = np.abs(xyz * (np.float32(1) / np.float32(voxel)))
    assert ((prod == 0) | (prod >= np.finfo(np.float32).tiny)).all()  # no denormal product: not pinned
    assert (xyz < 0).any() or n == 1
    return xyz


def expected_keep(fusion, mask, xyz, voxel):
    sel = np.flatnonzero((mask.reshape(-1) & 4) != 0)
    keep = np.zeros(mask.size, np.uint8)
    if len(sel):
        keep[sel[fusion.voxel_first(xyz.reshape(-1, 3)[sel], voxel)]] = 4
    return keep.reshape(mask.shape)


def guarded_grid(fusion, voxel, slots):
    """A VoxelGrid whose table lies between two poisoned guard bands -> (grid, the whole buffer)."""
    grid = fusion.VoxelGrid(voxel, slots, "cuda")
    words = grid.nbytes // 8
    flat = torch.full((GUARD // 8 + words + GUARD // 8,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda")
    assert flat.view(torch.uint8)[0].item() == POISON
    grid.table = flat[GUARD // 8:GUARD // 8 + words]
    grid.clear()
    return grid, flat


def guarded_keep(shape):
    n = int(np.prod(shape))
    flat = torch.full((GUARD + n + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    return flat, flat[GUARD:GUARD + n].view(shape)


def assert_guards(flat_keep, flat_table):
    k = flat_keep.cpu().numpy()
    assert set(k[:GUARD]) == {POISON} and set(k[-GUARD:]) == {POISON}, "guard band of keep"
    t = flat_table.view(torch.uint8).cpu().numpy()
    assert set(t[:GUARD]) == {POISON} and set(t[-GUARD:]) == {POISON}, "guard band of the table"


def claim_once(fusion, mask, xyz, voxel, slots):
    """One claim into poisoned, guarded buffers -> (keep as numpy, the grid); check() has passed or raised."""
    grid, flat_table = guarded_grid(fusion, voxel, slots)
    flat_keep, keep = guarded_keep(mask.shape)
    out = grid.claim(cu(mask), cu(xyz), 0, keep)
    assert out is keep
    got = keep.cpu().numpy()
    assert_guards(flat_keep, flat_table)
    grid.check()
    return got, grid


# ------------------------------------------------------------------------------------------ 1. claim vs numpy
@pytest.mark.parametrize("voxel", [0.5, 0.3])
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("n", SIZES)
def test_claim_equals_voxel_first(fusion, n, kind, voxel):
    xyz = make_cloud(n, voxel, seed=n * 31 + MASKS.index(kind))
    mask = make_mask(n, kind, seed=n * 17 + 3)
    want = expected_keep(fusion, mask, xyz, voxel)
    got, grid = claim_once(fusion, mask, xyz, voxel, 4096)
    assert got.tobytes() == want.tobytes()
    nsel, nkept = int(((mask & 4) != 0).sum()), int((want == 4).sum())
    assert grid.occupied() == nkept
    if kind == "none":
        assert nkept == 0
    elif n >= 257 and kind == "all":
        assert nkept < 0.8 * nsel  # most cells hold several points


def test_claim_takes_two_dimensional_views_and_allocates_keep(fusion):
    H, W = 24, 40
    xyz = make_cloud(H * W, 0.5, seed=9).reshape(H, W, 3)
    mask = make_mask(H * W, "random", seed=10).reshape(H, W)
    grid = fusion.VoxelGrid(0.5, 2048, "cuda")
    assert grid.nbytes == 2048 * 16 + 8 and grid.slots == 2048
    keep = grid.claim(cu(mask), cu(xyz), 0)
    grid.check()
    assert keep.shape == (H, W) and keep.dtype == torch.uint8
    assert keep.cpu().numpy().tobytes() == expected_keep(fusion, mask, xyz, 0.5).tobytes()
    with pytest.raises(ValueError, match="claim takes"):
        grid.claim(cu(mask), cu(xyz).reshape(-1, 3), 0)
    with pytest.raises(ValueError, match="keep must be"):
        grid.claim(cu(mask), cu(xyz), 0, keep.reshape(-1))


# ------------------------------------------------------------------------------------------------ 2. probing
def cells_by_home(fusion, slots=64, span=12):
    """Integer cells of [-span, span)^3 at voxel 1 -> (cell coordinates (m, 3), their home slots)."""
    g = np.arange(-span, span)
    cells = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    keys, ok = fusion.voxel_keys(cells.astype(np.float32) + np.float32(0.5), 1.0)
    assert ok.all()
    return cells, np.array([fusion.voxel_home_slot(k, slots) for k in keys])


def points_in_cells(cells, per_cell, seed):
    rng = np.random.default_rng(seed)
    pts = np.repeat(cells.astype(np.float32), per_cell, axis=0) + \
        rng.uniform(0.05, 0.95, size=(len(cells) * per_cell, 3)).astype(np.float32)
    return pts[rng.permutation(len(pts))].astype(np.float32)


@pytest.mark.parametrize("ncells", [48, 64])
def test_probe_chains_and_wrap_around(fusion, ncells):
    cells, home = cells_by_home(fusion)
    rng = np.random.default_rng(ncells)
    last = rng.permutation(np.flatnonzero(home >= 62))[:6]  # six cells that start from the last two slots
    rest = rng.permutation(np.flatnonzero(home < 62))[:ncells - 6]
    pick = np.concatenate([last, rest])
    # two slots cannot hold six keys: at least four walk past slot 63 to slot 0, in whatever order the threads arrive;
    # and with fewer distinct homes than cells, some cell does not sit in its home slot
    assert (home[pick] >= 62).sum() == 6 and len(set(home[pick].tolist())) < ncells == len(pick)
    xyz = points_in_cells(cells[pick], 5, seed=ncells + 1)
    mask = np.full(len(xyz), 4, np.uint8)
    want = expected_keep(fusion, mask, xyz, 1.0)
    assert int((want == 4).sum()) == ncells
    got, grid = claim_once(fusion, mask, xyz, 1.0, 64)
    assert got.tobytes() == want.tobytes() and grid.occupied() == ncells
    keys = set(grid.table[:64].cpu().numpy().view(np.uint64).tolist()) - {0xFFFFFFFFFFFFFFFF}
    assert keys == set(fusion.voxel_keys(xyz, 1.0)[0].tolist())


def test_a_full_table_is_reported(fusion):
    """65 cells for 64 slots: the pixels of the cell that finds no slot end their counted walk after 64 trips and set
    the status; the call returns, check() raises, and the status is clear afterwards."""
    cells, _ = cells_by_home(fusion)
    pick = np.random.default_rng(65).permutation(len(cells))[:65]
    xyz = points_in_cells(cells[pick], 2, seed=66)
    mask = np.full(len(xyz), 4, np.uint8)
    with pytest.raises(ValueError, match=r"DAMVS_E_WORKSPACE.*64 slots is full.*raise voxel_slots"):
        claim_once(fusion, mask, xyz, 1.0, 64)
    grid = fusion.VoxelGrid(1.0, 64, "cuda")
    grid.claim(cu(mask), cu(xyz), 0)
    with pytest.raises(ValueError, match="table full"):
        grid.check()
    grid.check()  # cleared by the check that reported it
    assert grid.occupied() == 64


# --------------------------------------------------------------------------------------------- 3. contention
def test_many_points_in_few_cells_three_times(fusion):
    cells = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, -1, 0], [0, 0, 1], [-1, -1, -1], [3, -2, 1]])
    xyz = points_in_cells(cells, 10240 // 7 + 1, seed=7)[:10240]
    mask = np.full(10240, 4, np.uint8)
    want = expected_keep(fusion, mask, xyz, 1.0)
    assert int((want == 4).sum()) == 7
    runs = [claim_once(fusion, mask, xyz, 1.0, 64)[0].tobytes() for _ in range(3)]
    assert runs[0] == runs[1] == runs[2] == want.tobytes()


# ----------------------------------------------------------------------------------------------- 4. chaining
@pytest.mark.parametrize("side_stream", [False, True], ids=["default_stream", "side_stream"])
@pytest.mark.parametrize("nviews", [2, 3])
def test_views_chain_on_one_table_without_synchronisation(fusion, nviews, side_stream):
    H, W = 24, 40
    # 13^3 nodes with a wide jitter: about 1300 cells, so every view finds cells taken and cells free
    views = [(make_mask(H * W, "random", seed=40 + v).reshape(H, W),
              lattice_cloud(H * W, 50 + v, span=6).reshape(H, W, 3)) for v in range(nviews)]
    want = expected_keep(fusion, np.concatenate([m.reshape(-1) for m, _ in views]),
                         np.concatenate([x.reshape(-1, 3) for _, x in views]), 0.5).reshape(nviews, H, W)
    assert all((want[v] == 4).any() for v in range(nviews)) and (want[1] == 4).sum() < (want[0] == 4).sum()
    dev = [(cu(m), cu(x)) for m, x in views]
    grid, flat_table = guarded_grid(fusion, 0.5, 4096)
    keeps = [guarded_keep((H, W)) for _ in range(nviews)]
    torch.cuda.synchronize()

    def enqueue():
        for v, (m, x) in enumerate(dev):  # no host synchronisation in between
            grid.claim(m, x, v * H * W, keeps[v][1])

    if side_stream:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            enqueue()
            grid.check()
        torch.cuda.current_stream().wait_stream(s)
    else:
        enqueue()
        grid.check()
    for v in range(nviews):
        assert keeps[v][1].cpu().numpy().tobytes() == want[v].tobytes(), v
        assert_guards(keeps[v][0], flat_table)
    assert grid.occupied() == int((want == 4).sum())


# -------------------------------------------------------------------------------------------------- 5. range
BAD_POINTS = {"nan": np.nan, "inf": np.inf, "-inf": -np.inf, "q=2^20": 524288.0, "q=-2^20-1": -524288.25}


@pytest.mark.parametrize("axis", [0, 2])
@pytest.mark.parametrize("bad", sorted(BAD_POINTS))
def test_a_selected_point_out_of_range_is_an_error(fusion, bad, axis):
    n = 257
    xyz = make_cloud(n, 0.5, seed=70)
    mask = make_mask(n, "random", seed=71)
    at = 200
    xyz[at, axis] = BAD_POINTS[bad]
    mask[at] &= 0xFB  # unselected: ignored
    want = expected_keep(fusion, mask, xyz, 0.5)
    got, grid = claim_once(fusion, mask, xyz, 0.5, 1024)
    assert got.tobytes() == want.tobytes() and got[at] == 0
    mask[at] |= 4
    with pytest.raises(ValueError, match="out of range"):
        fusion.voxel_first(xyz[(mask & 4) != 0], 0.5)
    grid.clear()
    keep = grid.claim(cu(mask), cu(xyz), 0)
    with pytest.raises(ValueError, match=r"DAMVS_E_RANGE.*out of range"):
        grid.check()
    assert keep[at].item() == 0  # it claimed nothing
    grid.check()  # the status is clear afterwards


# ------------------------------------------------------------------------------------------------ 6. drivers
def split_ply(path):
    raw = open(path, "rb").read()
    cut = raw.index(HEADER_END) + len(HEADER_END)
    header, body = raw[:cut], raw[cut:]
    assert len(body) % 15 == 0 and b"element vertex %d\n" % (len(body) // 15) in header
    return header, np.frombuffer(body, np.uint8).reshape(-1, 15)


def thinned_ply_bytes(fusion, path, voxel):
    """The PLY at `path` thinned by the statement: its records at voxel_first's indices, the header's count renewed."""
    header, rec = split_ply(path)
    xyz = np.ascontiguousarray(rec[:, :12]).view("<f4").reshape(-1, 3)
    idx = fusion.voxel_first(xyz, voxel)
    header = header.replace(b"element vertex %d\n" % len(rec), b"element vertex %d\n" % len(idx))
    return header + rec[idx].tobytes(), len(rec), len(idx)


def run_scene(fusion, root, views, pairs, tv, method, **kw):
    FF.write_tree(root, views, pairs)
    ply = os.path.join(root, "scene.ply")
    n = fusion.fuse_scene(root, root, root, ply, conf=FF.CONF_THR, dist_base=FF.DIST_BASE,
                          rel_diff_base=FF.REL_DIFF_BASE, method=method, thres_view=tv, **kw)
    return n, ply


DRIVER_CASES = [("scene", "dypcd", 0.5), ("scene", "dypcd", 2.0), ("scene", "pcd", 0.5), ("scene", "pcd", 2.0),
                ("edge", "dypcd", 2.0), ("edge", "pcd", 2.0)]


@pytest.mark.parametrize("case,method,voxel", DRIVER_CASES)
def test_fuse_scene_voxel_is_the_thinned_default_ply(fusion, ref, cases, case, method, voxel, tmp_path):
    from damvsnet_amd import mvsio
    views, pairs, tv = cases[case]
    a, b = str(tmp_path / "full"), str(tmp_path / "thin")
    n_full, ply_full = run_scene(fusion, a, views, pairs, tv, method)
    n_thin, ply_thin = run_scene(fusion, b, views, pairs, tv, method, voxel=voxel)
    key = "%s_%s_" % (case, method)
    ref_ply = str(tmp_path / "ref.ply")
    mvsio.write_ply(ref_ply, ref[key + "xyz"], ref[key + "rgb"])
    assert open(ply_full, "rb").read() == open(ref_ply, "rb").read()  # the voxel=None PLY is the reference's cloud
    want, full, kept = thinned_ply_bytes(fusion, ply_full, voxel)
    print(case, method, voxel, "points", full, "kept", kept)
    assert full == n_full == COUNTS[case + "_" + method][0]
    assert kept == COUNTS[case + "_" + method][1 + (0.5, 1.0, 2.0).index(voxel)]
    assert 0.05 * full <= kept <= 0.95 * full  # the comparison cannot pass empty or untouched
    assert n_thin == kept and open(ply_thin, "rb").read() == want
    for rv, _ in pairs:  # the masks remain the fusion's
        for kind in ("photo", "geo", "final"):
            name = os.path.join("mask", "%08d_%s.png" % (rv, kind))
            assert open(os.path.join(a, name), "rb").read() == open(os.path.join(b, name), "rb").read(), name


def test_voxel_slots_given_and_too_few(fusion, cases, tmp_path):
    views, pairs, tv = cases["scene"]
    n_full, ply_full = run_scene(fusion, str(tmp_path / "full"), views, pairs, tv, "dypcd")
    want, _, kept = thinned_ply_bytes(fusion, ply_full, 0.5)
    n, ply = run_scene(fusion, str(tmp_path / "fits"), views, pairs, tv, "dypcd", voxel=0.5, voxel_slots=1024)
    assert kept == 919 and n == kept and open(ply, "rb").read() == want  # 919 cells in 1024 slots
    root = str(tmp_path / "full_table")
    with pytest.raises(ValueError, match="raise voxel_slots"):
        run_scene(fusion, root, views, pairs, tv, "dypcd", voxel=0.5, voxel_slots=512)
    assert not os.path.exists(os.path.join(root, "scene.ply"))


def test_max_points_bounds_the_thinned_count(fusion, cases, tmp_path):
    views, pairs, tv = cases["scene"]
    full, kept = COUNTS["scene_dypcd"][0], COUNTS["scene_dypcd"][1]
    root = str(tmp_path / "over")
    with pytest.raises(ValueError, match=r"\b%d\b" % kept):
        run_scene(fusion, root, views, pairs, tv, "dypcd", voxel=0.5, max_points=kept - 1)
    assert not os.path.exists(os.path.join(root, "scene.ply"))
    assert kept < 1000 < full
    n, ply = run_scene(fusion, str(tmp_path / "fits"), views, pairs, tv, "dypcd", voxel=0.5, max_points=1000)
    n_full, ply_full = run_scene(fusion, str(tmp_path / "full"), views, pairs, tv, "dypcd")
    assert n == kept and n_full == full and open(ply, "rb").read() == thinned_ply_bytes(fusion, ply_full, 0.5)[0]
    n, _ = run_scene(fusion, str(tmp_path / "exact"), views, pairs, tv, "dypcd", voxel=0.5, max_points=kept)
    assert n == kept


def test_a_kept_point_out_of_range_raises_and_writes_no_ply(fusion, cases, tmp_path):
    """The scene's points lie within a few units of the origin: at voxel 2^-20 their cell indices leave the range."""
    views, pairs, tv = cases["scene"]
    root = str(tmp_path / "range")
    with pytest.raises(ValueError, match="DAMVS_E_RANGE"):
        run_scene(fusion, root, views, pairs, tv, "dypcd", voxel=2.0 ** -20)
    assert not os.path.exists(os.path.join(root, "scene.ply"))


@pytest.mark.parametrize("method", ["dypcd", "pcd"])
def test_scene_maps_fuse_voxel_equals_fuse_scene_voxel(fusion, method, tmp_path):
    from test_gpu_scene import plane_maps, write_plane_tree, fuse_kw, read_masks
    from test_scene import plane_case
    c = plane_case()
    maps = plane_maps()
    ply_full = str(tmp_path / "full.ply")
    n_full = maps.fuse(c["pairs"], ply_full, **fuse_kw(method))
    _, rec = split_ply(ply_full)
    xyz = np.ascontiguousarray(rec[:, :12]).view("<f4").reshape(-1, 3)
    # 1 / 64 of the cloud's largest extent: the scene is a plane seen by five views, so its tens of thousands of
    # points fall into a few thousand of the 64^3 cells (a plane crosses a few times 64^2 of them)
    voxel = float(np.float32((xyz.max(0) - xyz.min(0)).max() / 64))
    want, full, kept = thinned_ply_bytes(fusion, ply_full, voxel)
    print(method, "voxel", voxel, "points", full, "kept", kept)
    assert full == n_full and 0.05 * full <= kept <= 0.95 * full
    ply_a, ply_b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    n_a = maps.fuse(c["pairs"], ply_a, mask_dir=str(tmp_path / "mask_a"), voxel=voxel, **fuse_kw(method))
    scan = write_plane_tree(str(tmp_path / "tree"))
    n_b = fusion.fuse_scene(scan, scan, scan, ply_b, voxel=voxel, **fuse_kw(method))
    assert n_a == n_b == kept
    assert open(ply_a, "rb").read() == open(ply_b, "rb").read() == want
    views = range(c["N"])
    m_a, m_b = read_masks(str(tmp_path / "mask_a"), views), read_masks(os.path.join(scan, "mask"), views)
    assert all(np.array_equal(m_a[k], m_b[k]) for k in m_b)
    assert n_full == sum(int((m_a[(v, "final")] > 0).sum()) for v in views)  # the fusion's masks, not the thinned ones


def test_reconstruct_scene_voxel_thins_its_own_default_ply(fusion, tmp_path, monkeypatch):
    """tests/scene_fixture.py's scan (32 x 64, 5 views) through a synthetic-weight fp32 model, as in
    tests/test_gpu_scene.py: the wiring of voxel= through reconstruct_scene's fuse_kwargs. With random weights the
    cloud is whatever it is (it may be empty), so the arguments that reach fuse_resident are asserted too; the content
    is tested on the fixture trees above."""
    import scene_fixture as SF
    from common import model_state
    from damvsnet_amd import scene
    from damvsnet_amd.cascade import CascadeMVSNet
    data = str(tmp_path / "data")
    SF.make_scene(data)
    with open(os.path.join(data, "scan1", "pair.txt"), "w") as f:
        f.write("%d\n" % len(SF.PAIRS))
        for r, src in SF.PAIRS:
            src = src or [(3, 99.5), (4, 50.25)]
            f.write("%d\n%d %s\n" % (r, len(src), " ".join("%d %g" % p for p in src)))
    net = CascadeMVSNet(ndepths=[8, 8, 8])
    net.load_state_dict(model_state("forward_160x128_48_32_8"), strict=True)
    net = net.cuda().eval()
    kw = dict(nviews=SF.NV, ndepths=8, interval_scale=1.06, max_h=1184, max_w=1600, batch=2,
              conf=(0.0, 0.0, 0.0), thres_view=2, method="pcd")
    ply_full, ply_thin = str(tmp_path / "full.ply"), str(tmp_path / "thin.ply")
    n_full = scene.reconstruct_scene(net, data, "scan1", ply_full, **kw)
    _, rec = split_ply(ply_full)
    xyz = np.ascontiguousarray(rec[:, :12]).view("<f4").reshape(-1, 3)
    voxel = float(np.float32((xyz.max(0) - xyz.min(0)).max() / 8)) if len(rec) > 1 else 1.0
    want, full, kept = thinned_ply_bytes(fusion, ply_full, voxel)
    seen, real = [], fusion.fuse_resident

    def recording(*args, **kwargs):
        seen.append(args[-2:])
        return real(*args, **kwargs)

    monkeypatch.setattr(fusion, "fuse_resident", recording)
    n_thin = scene.reconstruct_scene(net, data, "scan1", ply_thin, voxel=voxel, voxel_slots=1 << 15, **kw)
    assert seen == [(voxel, 1 << 15)]  # SceneMaps.fuse hands them on as the last two arguments
    print("reconstruct_scene voxel", voxel, "points", full, "kept", kept)
    assert n_full == full and n_thin == kept and open(ply_thin, "rb").read() == want


# ------------------------------------------------------------------------------------- 7. beside a forward
def test_claim_on_a_side_stream_beside_a_bf16_forward(fusion):
    """One claim on a side stream while a bf16 CascadeMVSNet.forward runs on the main stream, once: keep equals the
    statement (the kernels are VALU only and carry no packed-FP32 ops, tests/test_thin_codeobj.py)."""
    from common import model_state, forward_inputs
    from damvsnet_amd.cascade import CascadeMVSNet
    n = 960
    xyz = make_cloud(n, 0.3, seed=80)
    mask = make_mask(n, "bytes", seed=81)
    want = expected_keep(fusion, mask, xyz, 0.3)
    net = CascadeMVSNet(ndepths=[8, 8, 8], compute_dtype=torch.bfloat16, frontend_dtype=torch.bfloat16)
    net.load_state_dict(model_state("forward_160x128_48_32_8"), strict=True)
    net = net.cuda().eval()
    imgs, proj, dv, _ = forward_inputs(1, 3, 32, 64)
    imgs, dv, proj = imgs.cuda(), dv.cuda(), {k: v.cuda() for k, v in proj.items()}
    side = torch.cuda.Stream()
    grid, flat_table = guarded_grid(fusion, 0.3, 4096)
    flat_keep, keep = guarded_keep((n,))
    m, x = cu(mask), cu(xyz)
    torch.cuda.synchronize()  # the side stream has nothing to wait for
    with torch.no_grad():
        out = net(imgs, proj, dv, check_range=False)  # enqueued on the main stream, not waited for
    with torch.cuda.stream(side):
        grid.claim(m, x, 0, keep)
    torch.cuda.synchronize()
    net.DepthNet.check_range()
    grid.check()
    assert out["depth"].shape == (1, 32, 64)
    assert keep.cpu().numpy().tobytes() == want.tobytes()
    assert_guards(flat_keep, flat_table)
