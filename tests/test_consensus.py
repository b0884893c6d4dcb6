"""CPU: consensus depth fusion (fusion.consensus_statement, damvs_consensus_table / damvs_consensus_view, the drivers)
without a GPU.

  * properties of the rule on the integer scene of tests/fusion_fixture.py (views 0-5, 24 x 40);
  * the hand-computed 4 x 4 two-view case: exact positions, colour rounding and flags;
  * the drivers and the C entry points refuse bad arguments before they read, launch or write anything;
  * the older entry points still refuse method="gipuma".
"""
import ctypes
import os

import numpy as np
import pytest

import consensus_fixture as CF
import fusion_fixture as FF
from conftest import golden

E_ARG, E_SHAPE = -1, -2
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fusion():
    from damvsnet_amd import fusion
    return fusion


def run(fusion, s, order=None, sources="all", thr=0.1, disp=0.15, num=3, **kw):
    order = fusion.consensus_order(s["pairs"], sources) if order is None else order
    return fusion.consensus_statement(s["depth"], s["conf"], s["rgb"], s["cams"], order, thr, disp, num, **kw)


def emitted(step):
    return (step["mask"] & 4) != 0


def total(steps):
    return sum(int(emitted(st).sum()) for st in steps)


@pytest.fixture(scope="module")
def integer():
    return CF.integer_scene()


# ------------------------------------------------------------------------------------------------ rule properties
@pytest.mark.parametrize("sources", ["all", "pairs"])
@pytest.mark.parametrize("num", [1, 2, 3])
def test_flags_counts_and_outputs_are_consistent(fusion, integer, sources, num):
    steps = run(fusion, integer, sources=sources, thr=CF.INTEGER_THR, num=num)
    assert [st["ref"] for st in steps] == [r for r, _ in integer["pairs"]] and total(steps) > 100
    for st in steps:
        m, n = st["mask"], st["count"]
        e = emitted(st)
        assert (n[e] >= num).all() and (n[~e & ((m & 8) == 0)] < num).all()  # every emitted point's n >= num_consistent
        assert set(np.unique(m)) <= {0, 1, 7, 9}  # consumed implies valid: only valid samples are ever marked
        assert not st["xyz"][~e].any() and not st["rgb"][~e].any()
        assert np.isfinite(st["xyz"]).all() and st["xyz"].dtype == np.float32 and st["rgb"].dtype == np.uint8
        assert (n[(m & 8) != 0] == 0).all()


def test_low_confidence_is_neither_emitted_nor_counted(fusion, integer):
    thr = np.float32(CF.INTEGER_THR)
    low = [c < thr for c in integer["conf"]]
    assert all(0.2 < l.mean() < 0.8 for l in low)
    steps = run(fusion, integer, thr=CF.INTEGER_THR, num=1)
    for st in steps:
        assert not (st["mask"][low[st["ref"]]]).any()  # not even valid
        for v, u in st["used"].items():
            assert not u[low[v]].any()  # never merged, so never counted
    # with the low samples' depth made invalid instead, nothing changes: they took no part
    cut = dict(integer, depth=[np.where(l, np.float32(0), d) for d, l in zip(integer["depth"], low)])
    again = run(fusion, cut, thr=CF.INTEGER_THR, num=1)
    for a, b in zip(steps, again):
        assert all(np.array_equal(a[k], b[k]) for k in ("mask", "xyz", "rgb", "count"))


def test_a_nan_confidence_stays_valid(fusion):
    s = CF.tiny_case()
    s["conf"][0][0, 1] = np.nan
    st = run(fusion, s, order=[(0, [1])], num=1)[0]
    assert st["mask"][0, 1] == 7


def test_used_only_grows_and_a_consumed_sample_is_not_emitted_again(fusion, integer):
    steps = run(fusion, integer, num=2)
    before = {v: np.zeros((FF.H, FF.W), np.uint8) for v in range(6)}
    consumed_total = 0
    for st, (ref, srcs) in zip(steps, fusion.consensus_order(integer["pairs"], "all")):
        assert np.array_equal(st["used"][ref], before[ref])  # a view's own pass never writes its own state
        assert np.array_equal((st["mask"] & 8) != 0, before[ref] != 0)
        assert not (emitted(st) & (before[ref] != 0)).any()
        for v in range(6):
            assert (st["used"][v] >= before[v]).all() and set(np.unique(st["used"][v])) <= {0, 1}
        consumed_total += int((before[ref] != 0).sum())
        before = st["used"]
    assert consumed_total > 1000
    # a view whose every sample was consumed emits nothing
    full = {v: np.ones((FF.H, FF.W), np.uint8) for v in range(6)}
    st = run(fusion, integer, order=[(3, [0, 1, 2])], num=1, used=full)[0]
    assert not emitted(st).any() and ((st["mask"] & 8) != 0).all()
    assert (run(fusion, integer, order=[(3, [0, 1, 2])], num=1)[0]["mask"] & 4).any()


def test_another_order_gives_another_self_consistent_result(fusion, integer):
    fwd = fusion.consensus_order(integer["pairs"], "all")
    a, b = run(fusion, integer, order=fwd, num=2), run(fusion, integer, order=fwd[::-1], num=2)
    first = lambda steps: {st["ref"]: st for st in steps}
    per_view = lambda steps: [int(emitted(first(steps)[v]).sum()) for v in range(6)]
    print(per_view(a), per_view(b))
    assert not np.array_equal(first(a)[0]["mask"], first(b)[0]["mask"]) and per_view(a) != per_view(b)
    assert int(emitted(b[0]).sum()) > int(emitted(first(a)[5]).sum())  # whoever goes first emits the most
    for steps in (a, b):
        for st in steps:
            assert (st["count"][emitted(st)] >= 2).all()
    # the statement itself is a function of its inputs
    again = run(fusion, integer, order=fwd, num=2)
    assert all(np.array_equal(x["xyz"], y["xyz"]) and np.array_equal(x["mask"], y["mask"]) for x, y in zip(a, again))


@pytest.mark.parametrize("sources", ["all", "pairs"])
def test_fewer_points_than_the_dynamic_filter(fusion, integer, sources):
    """dypcd writes one point per kept pixel per view (2487 on this scene, tests/golden/fusion_ref.npz); consensus writes
    a surface point once. Holds for the rule alone at the reference's defaults and at the thresholds the tests use."""
    dypcd = len(golden("fusion_ref")["scene_dypcd_xyz"])
    assert dypcd == 2487
    for thr, num in ((0.1, 3), (CF.INTEGER_THR, 2), (CF.INTEGER_THR, 1)):
        n = total(run(fusion, integer, sources=sources, thr=thr, num=num))
        print(sources, thr, num, n)
        assert 0 < n < dypcd


def test_every_outcome_occurs_on_the_rotated_scene(fusion):
    t = {}
    s = CF.rotated_scene()
    steps = run(fusion, s, sources="pairs", num=2, tally=t)
    print(t)
    assert min(t[k] for k in ("behind", "outside", "invalid", "far", "agree", "up", "down")) > 100
    assert total(steps) > 100


# ------------------------------------------------------------------------------------------------ the hand case
def test_hand_computed_two_view_case(fusion):
    """K = diag(4, 4, 1), view 1 one unit along x, depth 4: the reference pixel (x, y) is the world point (x, y, 4) and
    falls on (x - 1, y) of view 1; fb = 4."""
    s = CF.tiny_case()
    cams = [fusion.consensus_cam(K, E) for K, E in s["cams"]]
    assert fusion.consensus_fb(cams[0], cams[1]) == 4.0 == fusion.consensus_fb(cams[1], cams[0])
    a, b = run(fusion, s, order=s["pairs"], num=1)
    # column 0 leaves the frame, (3, 3) is below the threshold, (2, 3) meets depth 5 (|4/4 - 4/5| = 0.2), (3, 2) meets a
    # sample below the threshold
    assert a["mask"].tolist() == [[1, 7, 7, 7], [1, 7, 7, 7], [1, 7, 7, 1], [1, 7, 1, 0]]
    assert a["count"].tolist() == [[0, 1, 1, 1], [0, 1, 1, 1], [0, 1, 1, 0], [0, 1, 0, 0]]
    for y in range(4):
        for x in range(4):
            if a["mask"][y, x] == 7 and (y, x) != (1, 2):
                assert a["xyz"][y, x].tolist() == [x, y, 4] and a["rgb"][y, x].tolist() == [11, 11, 11]  # 10.5 -> 11
            elif a["mask"][y, x] != 7:
                assert a["xyz"][y, x].tolist() == [0, 0, 0] and a["rgb"][y, x].tolist() == [0, 0, 0]
    # (1, 2) meets depth 4.5 (|1 - 4/4.5| = 0.11): X_s = (1 * 4.5 / 4 + 1, 1 * 4.5 / 4, 4.5), averaged with (2, 1, 4)
    assert a["xyz"][1, 2].tolist() == [2.0625, 1.0625, 4.25]
    assert a["rgb"][1, 2].tolist() == [11, 255, 1]  # (10 + 12) / 2, (255 + 255) / 2, (1 + 0) / 2 = 0.5 -> 1
    want_used = [[1, 1, 1, 0], [1, 1, 1, 0], [1, 1, 0, 0], [1, 0, 0, 0]]
    assert a["used"][1].tolist() == want_used and not a["used"][0].any()
    # view 1: the consumed samples are skipped; column 3 and (3, 2) find nothing valid in view 0, (2, 2) is too far
    assert b["mask"].tolist() == [[9, 9, 9, 1], [9, 9, 9, 1], [9, 9, 1, 1], [9, 0, 1, 1]]
    assert not b["xyz"].any() and not b["rgb"].any() and not b["count"].any()
    assert b["used"][1].tolist() == want_used and not b["used"][0].any()
    # two sources required: nothing is emitted, but the marks are made all the same (fusibile marks inside the loop)
    a2 = run(fusion, s, order=[(0, [1])], num=2)[0]
    assert not (a2["mask"] & 6).any() and a2["used"][1].tolist() == want_used


def test_orders(fusion):
    pairs = [(3, [1, 1, 7, 1]), (1, [3]), (7, [1, 3, 3])]
    assert fusion.consensus_order(pairs, "all") == [(3, [1, 7]), (1, [3, 7]), (7, [1, 3])]
    assert fusion.consensus_order(pairs, "pairs") == [(3, [1, 7]), (1, [3]), (7, [1, 3])]
    assert fusion.consensus_order(pairs) == fusion.consensus_order(pairs, "all")
    for bad, match in (([(0, [1]), (0, [2])], "twice"), ([(0, [0, 1])], "own sources"), ([(0, [])], "no source"),
                       ([(0, list(range(1, 65)))], "at most 64")):
        with pytest.raises(ValueError, match=match):
            fusion.consensus_order(bad, "pairs")
    with pytest.raises(ValueError, match="sources"):
        fusion.consensus_order(pairs, "every")
    assert len(fusion.consensus_order([(0, list(range(1, 64)))], "pairs")[0][1]) == 63


# ------------------------------------------------------------------------------------------------ the drivers
BAD = [dict(prob_threshold=float("nan")), dict(prob_threshold=float("inf")), dict(prob_threshold="0.1"),
       dict(prob_threshold=1e39), dict(disp_threshold=float("nan")), dict(disp_threshold=-float("inf")),
       dict(disp_threshold=None), dict(num_consistent=0), dict(num_consistent=-3), dict(num_consistent=2.0),
       dict(num_consistent=True), dict(sources="every"), dict(voxel=-1.0), dict(voxel_slots=100),
       dict(normal_jump=float("nan"))]


@pytest.mark.parametrize("kw", BAD, ids=repr)
def test_drivers_refuse_bad_arguments_before_anything_else(kw, tmp_path):
    """Nothing exists at the paths and the maps are empty: a driver that went on past the check would fail otherwise."""
    from damvsnet_amd import fusion
    from damvsnet_amd.scene import SceneMaps, reconstruct_scene
    ply, nowhere = str(tmp_path / "never.ply"), str(tmp_path / "nowhere")
    with pytest.raises(ValueError):
        fusion.fuse_consensus_scene(nowhere, nowhere, nowhere, ply, **kw)
    with pytest.raises(ValueError):
        fusion.fuse_consensus_resident([(0, [1])], {}, {}, {}, {}, ply, **kw)
    with pytest.raises(ValueError):
        SceneMaps([0, 1], 8, 8, "cpu").fuse_consensus([(0, [1])], ply, **kw)
    with pytest.raises(ValueError):
        reconstruct_scene(None, nowhere, "scan1", ply, fusion="consensus", **kw)
    if set(kw) <= {"prob_threshold", "disp_threshold", "num_consistent"}:
        with pytest.raises(ValueError, match=next(iter(kw))):
            fusion.check_consensus(**kw)
    assert not os.path.exists(ply) and not os.path.exists(nowhere)


def test_reconstruct_scene_refuses_an_unknown_fusion_before_reading(tmp_path):
    from damvsnet_amd.scene import reconstruct_scene
    ply, nowhere = str(tmp_path / "never.ply"), str(tmp_path / "nowhere")
    for bad in ("nope", "gipuma", None, True):
        with pytest.raises(ValueError, match="fusion must be"):
            reconstruct_scene(None, nowhere, "scan1", ply, fusion=bad)
    with pytest.raises(ValueError, match="conf"):  # the pair filters' arguments do not belong to the consensus rule
        reconstruct_scene(None, nowhere, "scan1", ply, fusion="consensus", conf=(0.1, 0.15, 0.9))
    assert not os.path.exists(ply) and not os.path.exists(nowhere)


def test_resident_driver_refuses_bad_scenes_before_any_launch(fusion, tmp_path):
    """Host tensors: whatever passes the scene checks is refused at the latest for not being on a device."""
    import torch
    ply = str(tmp_path / "never.ply")
    d = lambda h=8, w=8: torch.zeros(h, w)
    c = lambda h=8, w=8: torch.zeros(h, w, 3, dtype=torch.uint8)
    cam = (np.eye(3, dtype=np.float32), np.eye(4, dtype=np.float32))
    full = lambda n: ({v: cam for v in range(n)}, {v: d() for v in range(n)}, {v: d() for v in range(n)},
                      {v: c() for v in range(n)})
    cams, depths, confs, rgbs = full(3)
    pairs = [(0, [1, 2]), (1, [0])]
    run = lambda *a, **k: fusion.fuse_consensus_resident(*a, ply, **k)
    with pytest.raises(ValueError, match="twice"):
        run([(0, [1]), (0, [2])], cams, depths, confs, rgbs)
    with pytest.raises(ValueError, match="at most 64"):
        run([(0, list(range(1, 65)))], *full(65))
    with pytest.raises(ValueError, match="view 2 is missing its conf"):
        run(pairs, cams, depths, {0: d(), 1: d()}, rgbs)
    with pytest.raises(ValueError, match="view 2 is missing its colour"):
        run(pairs, cams, depths, confs, {0: c(), 1: c()})
    with pytest.raises(ValueError, match="view 2 is missing its cams"):
        run(pairs, {0: cam, 1: cam}, depths, confs, rgbs)
    with pytest.raises(ValueError, match="one size"):
        run(pairs, cams, {**depths, 2: d(8, 12)}, confs, rgbs)
    with pytest.raises(ValueError, match="one size"):
        run(pairs, cams, depths, confs, {**rgbs, 1: c(4, 8)})
    with pytest.raises(ValueError, match="CUDA"):
        run(pairs, cams, depths, confs, rgbs)
    assert not os.path.exists(ply)


def test_scene_maps_needs_every_used_view(tmp_path):
    from damvsnet_amd.scene import SceneMaps
    ply = str(tmp_path / "never.ply")
    with pytest.raises(ValueError, match="view 0 .* never added"):
        SceneMaps([0, 1], 8, 8, "cpu").fuse_consensus([(0, [1])], ply)
    with pytest.raises(ValueError, match="twice"):
        SceneMaps([0, 1], 8, 8, "cpu").fuse_consensus([(0, [1]), (0, [1])], ply)
    assert not os.path.exists(ply)


@pytest.mark.parametrize("method", ["gipuma", "consensus"])
def test_the_pair_filters_keep_their_methods(fusion, method, tmp_path):
    import torch
    assert fusion.METHODS == ("dypcd", "pcd")
    ply, nowhere = str(tmp_path / "never.ply"), str(tmp_path / "nowhere")
    with pytest.raises(ValueError, match="fusion method"):
        fusion.fuse_scene(nowhere, nowhere, nowhere, ply, method=method)
    with pytest.raises(ValueError, match="fusion method"):
        fusion.filter_depth(nowhere, nowhere, nowhere, ply, method=method)
    with pytest.raises(ValueError, match="fusion method"):
        fusion.fuse_view(torch.zeros(4, 4), np.eye(3), np.eye(4), [], method=method)
    with pytest.raises(ValueError, match="fusion method"):
        fusion.fuse_resident([(0, [1])], {}, {}, {}, {}, ply, method=method)
    assert not os.path.exists(ply)


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
    for name in ("damvs_consensus_table_bytes", "damvs_consensus_table", "damvs_consensus_view"):
        assert name in names and name + "(" in header
    assert "#define DAMVS_CONSENSUS_MAX_VIEWS 64" in header and _capi.CONSENSUS_MAX_VIEWS == 64
    assert ctypes.sizeof(_capi.DamvsConsensusCam) == 200
    assert os.path.basename(build.CONSENSUS_LIB) == "libdamvs_consensus.so"
    assert build.CONSENSUS_UNITS == ("k_consensus.hip",)


def test_library_validates_before_device_work(lib):
    from damvsnet_amd import _capi
    P = 256  # never dereferenced: every call below fails validation
    err = lambda: lib.damvs_last_error_string()
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    dbl = lambda *v: (ctypes.c_double * len(v))(*v)

    def view(H=24, W=40, V=6, table=P, ref=0, src=(1, 2, 3), fb=None, prob=0.1, disp=0.15, num=3, mask=P, xyz=P, rgb=P,
             nsrc=None, null_src=False, null_fb=False):
        n = len(src) if nsrc is None else nsrc
        fbs = dbl(*(fb if fb is not None else [1.0] * max(len(src), 1)))
        return lib.damvs_consensus_view(None, H, W, V, table, ref, n, None if null_src else ints(*src),
                                        None if null_fb else fbs, prob, disp, num, mask, xyz, rgb)

    for name in ("table", "mask", "xyz", "rgb"):
        assert view(**{name: None}) == E_ARG and b"null" in err(), name
    assert view(null_src=True) == E_ARG and b"null" in err()
    assert view(null_fb=True) == E_ARG and b"null" in err()
    for H, W in ((0, 40), (24, 0), (-1, 5), (65536, 32768)):
        assert view(H=H, W=W) == E_SHAPE and b"bad shape" in err()
    for V in (0, -1, 65):
        assert view(V=V) == E_SHAPE and b"V " in err()
    for ref in (-1, 6, 64):
        assert view(ref=ref) == E_SHAPE and b"ref" in err()
    for src in ((1, 6), (-1, 2), (1, 64)):
        assert view(src=src) == E_SHAPE and b"source" in err()
    assert view(src=(1, 0, 2)) == E_ARG and b"among the sources" in err()
    assert view(src=(1, 2, 1)) == E_ARG and b"twice" in err()
    assert view(nsrc=0) == E_SHAPE and b"nsrc" in err()
    assert view(nsrc=-1) == E_SHAPE and b"nsrc" in err()
    assert view(V=64, src=tuple(range(1, 64)) + (1,), nsrc=64) == E_SHAPE and b"nsrc" in err()
    for num in (0, -1):
        assert view(num=num) == E_ARG and b"num_consistent" in err()
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert view(prob=bad) == E_ARG and b"prob_thr" in err()
        assert view(disp=bad) == E_ARG and b"disp_thr" in err()
        assert view(fb=[1.0, bad, 1.0]) == E_ARG and b"fb[1]" in err()

    nbytes = ctypes.c_size_t()
    assert lib.damvs_consensus_table_bytes(6, ctypes.byref(nbytes)) == 0 and nbytes.value == 6 * 232
    assert lib.damvs_consensus_table_bytes(64, ctypes.byref(nbytes)) == 0 and nbytes.value == 64 * 232
    assert lib.damvs_consensus_table_bytes(6, None) == E_ARG
    for V in (0, 65):
        assert lib.damvs_consensus_table_bytes(V, ctypes.byref(nbytes)) == E_SHAPE

    cams = (_capi.DamvsConsensusCam * 3)()
    ptrs = lambda *v: (ctypes.c_void_p * len(v))(*v)

    def table(H=8, W=8, V=3, cams=cams, depth=ptrs(P, P, P), conf=ptrs(P, P, P), rgb=ptrs(P, P, P),
              used=ptrs(256, 512, 768), out=P):
        return lib.damvs_consensus_table(None, H, W, V, cams, depth, conf, rgb, used, out)

    for name in ("cams", "depth", "conf", "rgb", "used", "out"):
        assert table(**{name: None}) == E_ARG and b"null" in err(), name
    for name in ("depth", "conf", "rgb", "used"):
        assert table(**{name: ptrs(P, None, 512)}) == E_ARG and b"view 1" in err(), name
    assert table(used=ptrs(256, 512, 256)) == E_ARG and b"share" in err()
    assert table(H=0) == E_SHAPE and table(W=-2) == E_SHAPE and table(V=0) == E_SHAPE and table(V=65) == E_SHAPE
