"""GPU: consensus depth fusion on the device (k_consensus.hip: fusion.consensus_view, the consensus drivers).

Every comparison with fusion.consensus_statement is bit equality: the kernel does the statement's IEEE double operations
in its order, without contraction, and integer colour sums.
  1. consensus_view against the statement, step by step over a scene: mask, xyz, rgb_avg and every view's `used` after
     every step, the outputs written into poisoned buffers between guard bands. Scenes (tests/consensus_fixture.py): the
     integer scene (960 pixels: three blocks and a tail), the hand-computed 4 x 4 case, the rotated scene (every outcome
     of the rule occurs, asserted on the statement alone), 63 sources on 4 x 8 maps, sources with NaN, zero, infinite and
     negative depths and NaN confidences.
  2. the three drivers (fuse_consensus_resident, fuse_consensus_scene over the saved tree, SceneMaps.fuse_consensus) write
     identical PLY bytes, the statement's points in order; voxel=, normals=True and max_points compose.
  3. one launch on a side stream beside a bf16 forward.
  4. reconstruct_scene(fusion="consensus") against fuse_consensus_scene over the tree its maps save.
"""
import os

import numpy as np
import pytest
import torch

import consensus_fixture as CF

pytestmark = pytest.mark.gpu
POISON = 0xA5
GUARD = 64
PLAIN = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
REC = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                ("red", "u1"), ("green", "u1"), ("blue", "u1")])
HEADER_END = b"end_header\n"


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


def on_device(s):
    n = len(s["depth"])
    return ({v: s["cams"][v] for v in range(n)}, {v: cu(s["depth"][v]) for v in range(n)},
            {v: cu(s["conf"][v]) for v in range(n)}, {v: cu(s["rgb"][v]) for v in range(n)})


def statement(fusion, s, order, thr, disp, num, **kw):
    return fusion.consensus_statement(s["depth"], s["conf"], s["rgb"], s["cams"], order, thr, disp, num, **kw)


def guarded(H, W):
    """(mask, xyz, rgb_avg) as views into poisoned buffers with a guard band on either side, and the buffers."""
    bufs = [torch.full((GUARD + H * W * k + GUARD,), POISON, dtype=torch.uint8, device="cuda") for k in (1, 12, 3)]
    mid = [b[GUARD:b.numel() - GUARD] for b in bufs]
    return (mid[0].view(H, W), mid[1].view(torch.float32).view(H, W, 3), mid[2].view(H, W, 3)), bufs


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def compare_steps(fusion, s, order, thr, disp, num):
    """Every step of the statement against consensus_view on one table -> the statement's steps."""
    want = statement(fusion, s, order, thr, disp, num)
    cams, depths, confs, rgbs = on_device(s)
    views = sorted({v for r, src in order for v in [r] + src})
    table = fusion.ConsensusTable(views, cams, depths, confs, rgbs)
    H, W = table.H, table.W
    for (ref, srcs), st in zip(order, want):
        out, bufs = guarded(H, W)
        got = fusion.consensus_view(table, ref, srcs, thr, disp, num, out=out)
        torch.cuda.synchronize()
        assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
        mask, xyz, rgb = (t.cpu().numpy() for t in got)
        assert same(mask, st["mask"]), (ref, np.argwhere(mask != st["mask"])[:5])
        assert same(xyz, st["xyz"]), (ref, np.argwhere(xyz.view(np.uint32) != st["xyz"].view(np.uint32))[:5])
        assert same(rgb, st["rgb"]), (ref, np.argwhere(rgb != st["rgb"])[:5])
        for b in bufs:
            edge = b.cpu().numpy()
            assert (edge[:GUARD] == POISON).all() and (edge[-GUARD:] == POISON).all()
        for v in views:
            assert same(table.used_of(v).cpu().numpy(), st["used"][v]), (ref, v)
    return want


def emitted_total(steps):
    return sum(int(((st["mask"] & 4) != 0).sum()) for st in steps)


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("sources", ["all", "pairs"])
@pytest.mark.parametrize("thr,num", [(CF.INTEGER_THR, 2), (0.1, 3), (CF.INTEGER_THR, 1)])
def test_integer_scene(fusion, sources, thr, num):
    s = CF.integer_scene()
    assert s["depth"][0].size == 960 == 3 * 256 + 192
    steps = compare_steps(fusion, s, fusion.consensus_order(s["pairs"], sources), thr, 0.15, num)
    assert emitted_total(steps) > 300 and sum(int(((st["mask"] & 8) != 0).sum()) for st in steps) > 1000


@pytest.mark.parametrize("num", [1, 2])
def test_hand_computed_case(fusion, num):
    s = CF.tiny_case()
    steps = compare_steps(fusion, s, s["pairs"], 0.1, 0.15, num)
    assert emitted_total(steps) == (9 if num == 1 else 0)
    if num == 1:
        assert steps[0]["xyz"][1, 2].tolist() == [2.0625, 1.0625, 4.25] and steps[0]["rgb"][1, 2].tolist() == [11, 255, 1]


@pytest.mark.parametrize("sources", ["all", "pairs"])
@pytest.mark.parametrize("disp,num", [(0.15, 2), (0.05, 1)])
def test_rotated_scene(fusion, sources, disp, num):
    s = CF.rotated_scene()
    order = fusion.consensus_order(s["pairs"], sources)
    tally = {}
    statement(fusion, s, order, 0.1, disp, num, tally=tally)
    # under the statement alone: the rounding goes up and down, pixels leave the frame, points lie behind a camera,
    # samples are invalid, and the disparity test passes and fails
    print(sources, disp, num, tally)
    assert min(tally[k] for k in ("up", "down", "outside", "behind", "invalid", "far", "agree")) > 100
    steps = compare_steps(fusion, s, order, 0.1, disp, num)
    assert emitted_total(steps) > 100


def test_63_sources(fusion):
    s = CF.many_sources()
    order = fusion.consensus_order(s["pairs"], "pairs")
    assert len(order[0][1]) == 63
    steps = compare_steps(fusion, s, order, 0.1, 0.15, 3)
    assert steps[0]["count"].max() > 40 and emitted_total(steps) > 20
    assert ((steps[1]["mask"] & 8) != 0).any()


@pytest.mark.parametrize("sources", ["all", "pairs"])
def test_sources_with_nan_zero_infinite_and_negative_depths(fusion, sources):
    s = CF.holes_scene()
    assert np.isnan(s["depth"][1]).sum() > 50 and (s["depth"][1] == 0).sum() > 50 and np.isinf(s["depth"][2]).sum() > 50
    assert (s["depth"][2] < 0).sum() > 50 and np.isnan(s["conf"][1]).sum() > 50
    steps = compare_steps(fusion, s, fusion.consensus_order(s["pairs"], sources), CF.INTEGER_THR, 0.15, 2)
    assert emitted_total(steps) > 300
    for st in steps:
        assert np.isfinite(st["xyz"]).all()
        bad = ~(np.isfinite(s["depth"][st["ref"]]) & (s["depth"][st["ref"]] > 0))
        assert not st["mask"][bad].any()
        for v, u in st["used"].items():
            assert not u[~(np.isfinite(s["depth"][v]) & (s["depth"][v] > 0))].any()


def test_primitive_checks_its_arguments(fusion):
    s = CF.tiny_case()
    cams, depths, confs, rgbs = on_device(s)
    table = fusion.ConsensusTable([0, 1], cams, depths, confs, rgbs)
    for ref, srcs in ((0, [0]), (0, [1, 1]), (0, []), (2, [0]), (0, [5])):
        with pytest.raises(ValueError):
            fusion.consensus_view(table, ref, srcs)
    with pytest.raises(ValueError, match="num_consistent"):
        fusion.consensus_view(table, 0, [1], num_consistent=0)
    with pytest.raises(ValueError, match="out"):
        fusion.consensus_view(table, 0, [1], out=(torch.empty(4, 4, device="cuda", dtype=torch.uint8),) * 3)
    torch.cuda.synchronize()
    assert not table.used.any()


# ------------------------------------------------------------------------------------------------ 2. the drivers
def split_ply(path, rec=PLAIN):
    data = open(path, "rb").read()
    end = data.index(HEADER_END) + len(HEADER_END)
    return data[:end], np.frombuffer(data[end:], dtype=rec)


def statement_ply(steps, path):
    from damvsnet_amd import mvsio
    sel = [(st["mask"] & 4) != 0 for st in steps]
    mvsio.write_ply(path, np.concatenate([st["xyz"][m] for st, m in zip(steps, sel)]),
                    np.concatenate([st["rgb"][m] for st, m in zip(steps, sel)]))
    return open(path, "rb").read()


def scene_maps(s):
    """The scene in a SceneMaps, added as a forward's outputs in two batches."""
    from damvsnet_amd.scene import SceneMaps
    n = len(s["depth"])
    H, W = s["depth"][0].shape
    rng = np.random.default_rng(3)
    maps = SceneMaps(range(n), H, W, "cuda")
    cams = np.zeros((n, 2, 4, 4), np.float32)
    for v, (K, E) in enumerate(s["cams"]):
        cams[v, 0], cams[v, 1, :3, :3], cams[v, 1, 3, :2] = E, K, (425.0, 2.5)
    for lo, hi in ((0, n // 2), (n // 2, n)):
        f = lambda h, w: cu(rng.random((hi - lo, h, w), dtype=np.float32))
        out = {"depth": cu(np.stack(s["depth"][lo:hi])), "photometric_confidence": cu(np.stack(s["conf"][lo:hi])),
               "stage2": {"photometric_confidence": f(H // 2, W // 2)},
               "stage1": {"photometric_confidence": f(H // 4, W // 4)}}
        maps.add(list(range(lo, hi)), out, rgb=cu(np.stack(s["rgb"][lo:hi])), cams=cams[lo:hi])
    return maps


def write_pairs(path, pairs):
    with open(path, "w") as f:
        f.write("%d\n" % len(pairs))
        for r, src in pairs:
            f.write("%d\n%d %s\n" % (r, len(src), " ".join("%d 1.0" % v for v in src)))


def saved_tree(maps, s, root):
    maps.save(root, "scan", lossless=True)
    scan = os.path.join(root, "scan")
    write_pairs(os.path.join(scan, "pair.txt"), s["pairs"])
    return scan


def read_masks(folder, views):
    from PIL import Image
    return {(v, k): np.array(Image.open(os.path.join(folder, "%08d_%s.png" % (v, k))))
            for v in views for k in ("valid", "geo", "final", "consumed")}


SCENES = {"integer": (CF.integer_scene, dict(prob_threshold=CF.INTEGER_THR, num_consistent=2)),
          "rotated": (CF.rotated_scene, dict(num_consistent=2))}


@pytest.mark.parametrize("sources", ["all", "pairs"])
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_the_three_drivers_write_the_statements_points_in_order(fusion, scene, sources, tmp_path):
    make, kw = SCENES[scene]
    s = make()
    order = fusion.consensus_order(s["pairs"], sources)
    steps = statement(fusion, s, order, kw.get("prob_threshold", 0.1), 0.15, kw["num_consistent"])
    want = statement_ply(steps, str(tmp_path / "want.ply"))
    n_want = emitted_total(steps)
    assert n_want > 100
    ply = {k: str(tmp_path / (k + ".ply")) for k in ("resident", "scene", "maps")}
    n_r = fusion.fuse_consensus_resident(s["pairs"], *on_device(s), ply["resident"], sources=sources,
                                         mask_dir=str(tmp_path / "mask_r"), **kw)
    maps = scene_maps(s)
    n_m = maps.fuse_consensus(s["pairs"], ply["maps"], sources=sources, mask_dir=str(tmp_path / "mask_m"), **kw)
    scan = saved_tree(maps, s, str(tmp_path / "tree"))
    n_s = fusion.fuse_consensus_scene(scan, scan, scan, ply["scene"], sources=sources, **kw)
    assert n_r == n_m == n_s == n_want
    for k in ply:
        assert open(ply[k], "rb").read() == want, k
    views = [r for r, _ in order]
    masks = [read_masks(d, views) for d in (str(tmp_path / "mask_r"), str(tmp_path / "mask_m"), os.path.join(scan, "mask"))]
    for st in steps:
        for bit, kind in ((1, "valid"), (2, "geo"), (4, "final"), (8, "consumed")):
            for m in masks:
                assert np.array_equal(m[(st["ref"], kind)] > 0, (st["mask"] & bit) != 0), (st["ref"], kind)
    # the defaults are sources="all" and the reference's thresholds
    if sources == "all" and scene == "rotated":
        n_d = fusion.fuse_consensus_resident(s["pairs"], *on_device(s), str(tmp_path / "default.ply"))
        assert n_d == emitted_total(statement(fusion, s, order, 0.1, 0.15, 3))


@pytest.mark.parametrize("scene,voxel", [("integer", 2.0), ("rotated", 4.0)])
def test_voxel_thins_to_voxel_firsts_subsequence(fusion, scene, voxel, tmp_path):
    """The integer scene's pixels are 1 world unit apart at depth 64 and 0.5 at depth 32, and consensus writes a surface
    point once: only a voxel above that spacing thins (2.0: blocks of 2 x 2 pixels and more)."""
    from damvsnet_amd import mvsio
    make, kw = SCENES[scene]
    s = make()
    full, thin = str(tmp_path / "full.ply"), str(tmp_path / "thin.ply")
    n_full = fusion.fuse_consensus_resident(s["pairs"], *on_device(s), full, **kw)
    head, rec = split_ply(full)
    keep = fusion.voxel_first(np.stack([rec["x"], rec["y"], rec["z"]], 1), voxel)
    print(scene, "voxel", voxel, "points", n_full, "kept", len(keep))
    assert 0 < len(keep) < n_full == len(rec)
    n_thin = fusion.fuse_consensus_resident(s["pairs"], *on_device(s), thin, voxel=voxel, voxel_slots=1 << 12,
                                            mask_dir=str(tmp_path / "mask"), **kw)
    assert n_thin == len(keep)
    assert open(thin, "rb").read() == mvsio._ply_header(len(keep)) + rec[keep].tobytes()
    # the PNGs are the fusion's masks, not the thinned ones
    m = read_masks(str(tmp_path / "mask"), [r for r, _ in s["pairs"]])
    assert sum(int((m[(r, "final")] > 0).sum()) for r, _ in s["pairs"]) == n_full


@pytest.mark.parametrize("scene", sorted(SCENES))
@pytest.mark.parametrize("voxel", [None, 2.0])
def test_normals_keep_the_points_and_equal_the_normal_statement(fusion, scene, voxel, tmp_path):
    from damvsnet_amd import mvsio
    make, kw = SCENES[scene]
    s = make()
    jump = 0.02
    plain, oriented = str(tmp_path / "plain.ply"), str(tmp_path / "oriented.ply")
    vkw = dict(voxel=voxel, voxel_slots=1 << 12) if voxel else {}
    n0 = fusion.fuse_consensus_resident(s["pairs"], *on_device(s), plain, **kw, **vkw)
    n1 = fusion.fuse_consensus_resident(s["pairs"], *on_device(s), oriented, normals=True, normal_jump=jump, **kw, **vkw)
    head, rec = split_ply(oriented, REC)
    _, rec0 = split_ply(plain)
    assert n1 == n0 == len(rec) == len(rec0) > 50 and head == mvsio._ply_oriented_header(n0)
    for name in PLAIN.names:
        assert rec[name].tobytes() == rec0[name].tobytes(), name
    # the rule's inputs are the passed maps: the view's own depth map and the consensus mask's emitted bit
    order = fusion.consensus_order(s["pairs"], "all")
    steps = statement(fusion, s, order, kw.get("prob_threshold", 0.1), 0.15, kw["num_consistent"])
    nrm = [fusion.normals_statement(s["depth"][st["ref"]], (st["mask"] & 4) != 0, *s["cams"][st["ref"]], jump)
           [(st["mask"] & 4) != 0] for st in steps]
    nrm = np.concatenate(nrm)
    if voxel:
        xyz = np.concatenate([st["xyz"][(st["mask"] & 4) != 0] for st in steps])
        nrm = nrm[fusion.voxel_first(xyz, voxel)]
    got = np.stack([rec["nx"], rec["ny"], rec["nz"]], 1)
    assert same(got, nrm)


def test_max_points_overflow_raises_and_writes_nothing(fusion, tmp_path):
    make, kw = SCENES["integer"]
    s = make()
    n = fusion.fuse_consensus_resident(s["pairs"], *on_device(s), str(tmp_path / "all.ply"), **kw)
    over = str(tmp_path / "over.ply")
    with pytest.raises(ValueError, match=r"\b%d\b" % n):
        fusion.fuse_consensus_resident(s["pairs"], *on_device(s), over, max_points=n - 1, **kw)
    with pytest.raises(ValueError, match=r"\b%d\b" % n):
        fusion.fuse_consensus_resident(s["pairs"], *on_device(s), over, max_points=n - 1, normals=True, **kw)
    assert not os.path.exists(over)
    fits = str(tmp_path / "fits.ply")
    assert fusion.fuse_consensus_resident(s["pairs"], *on_device(s), fits, max_points=n, **kw) == n
    assert open(fits, "rb").read() == open(str(tmp_path / "all.ply"), "rb").read()


def test_drivers_refuse_bad_scenes_before_any_launch(fusion, tmp_path):
    s = CF.integer_scene()
    cams, depths, confs, rgbs = on_device(s)
    ply = str(tmp_path / "never.ply")
    with pytest.raises(ValueError, match="missing its conf"):
        fusion.fuse_consensus_resident(s["pairs"], cams, depths, {v: confs[v] for v in range(5)}, rgbs, ply)
    with pytest.raises(ValueError, match="one size"):
        fusion.fuse_consensus_resident(s["pairs"], cams, {**depths, 3: depths[3][:, :36].contiguous()}, confs, rgbs, ply)
    with pytest.raises(ValueError, match="twice"):
        fusion.fuse_consensus_resident(s["pairs"] + [s["pairs"][0]], cams, depths, confs, rgbs, ply)
    maps = scene_maps(s)
    maps._coloured.discard(4)
    with pytest.raises(ValueError, match="view 4 was added without"):
        maps.fuse_consensus(s["pairs"], ply)
    assert not os.path.exists(ply)


# ------------------------------------------------------------------------------------- 3. beside a forward
def test_a_launch_on_a_side_stream_beside_a_bf16_forward(fusion):
    """One consensus_view on a side stream while a bf16 CascadeMVSNet.forward runs on the main stream, once: the outputs
    equal the statement (the kernel is VALU only and carries no packed-FP32 ops, tests/test_consensus_codeobj.py)."""
    from common import model_state, forward_inputs
    from damvsnet_amd.cascade import CascadeMVSNet
    s = CF.rotated_scene()
    order = fusion.consensus_order(s["pairs"], "all")[:1]
    want, = statement(fusion, s, order, 0.1, 0.15, 2)
    net = CascadeMVSNet(ndepths=[8, 8, 8], compute_dtype=torch.bfloat16, frontend_dtype=torch.bfloat16)
    net.load_state_dict(model_state("forward_160x128_48_32_8"), strict=True)
    net = net.cuda().eval()
    imgs, proj, dv, _ = forward_inputs(1, 3, 32, 64)
    imgs, dv, proj = imgs.cuda(), dv.cuda(), {k: t.cuda() for k, t in proj.items()}
    side = torch.cuda.Stream()
    table = fusion.ConsensusTable(list(range(6)), *on_device(s))
    out, _ = guarded(table.H, table.W)
    torch.cuda.synchronize()  # the side stream has nothing to wait for
    with torch.no_grad():
        res = net(imgs, proj, dv, check_range=False)  # enqueued on the main stream, not waited for
    with torch.cuda.stream(side):
        fusion.consensus_view(table, order[0][0], order[0][1], 0.1, 0.15, 2, out=out)
    torch.cuda.synchronize()
    net.DepthNet.check_range()
    assert res["depth"].shape == (1, 32, 64)
    assert same(out[0].cpu().numpy(), want["mask"]) and same(out[1].cpu().numpy(), want["xyz"])
    assert same(out[2].cpu().numpy(), want["rgb"])
    for v in range(6):
        assert same(table.used_of(v).cpu().numpy(), want["used"][v])


# ------------------------------------------------------------------------------------- 4. reconstruct_scene
def test_reconstruct_scene_consensus_equals_the_saved_trees_fusion(fusion, tmp_path, monkeypatch):
    """tests/scene_fixture.py's scan (32 x 64, 5 views) through a synthetic-weight fp32 model, as in
    tests/test_gpu_scene.py (view 2 gets two sources there, for the same reason). With random weights the cloud is
    whatever it is, so the thresholds are wide; the content is tested on the fixture scenes above."""
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
    kw = dict(nviews=SF.NV, ndepths=8, interval_scale=1.06, max_h=1184, max_w=1600, batch=2)
    fkw = dict(prob_threshold=0.0, disp_threshold=50.0, num_consistent=1)
    kept, real, pair_path = [], scene.SceneMaps.fuse_consensus, scene.SceneMaps.fuse

    def recording(self, *a, **k):
        kept.append((self, a, k))
        return real(self, *a, **k)

    monkeypatch.setattr(scene.SceneMaps, "fuse_consensus", recording)
    monkeypatch.setattr(scene.SceneMaps, "fuse", None)  # the pair filters are not on this path
    results = {}
    for sources in ("all", "pairs"):
        ply_a, ply_b = str(tmp_path / ("a_%s.ply" % sources)), str(tmp_path / ("b_%s.ply" % sources))
        n_a = scene.reconstruct_scene(net, data, "scan1", ply_a, fusion="consensus", sources=sources, **kw, **fkw)
        maps, args, kwargs = kept[-1]
        assert kwargs == dict(sources=sources, **fkw) and args[1] == ply_a
        maps.save(str(tmp_path / ("out_" + sources)), "scan1", lossless=True)
        saved = os.path.join(str(tmp_path / ("out_" + sources)), "scan1")
        n_b = fusion.fuse_consensus_scene(os.path.join(data, "scan1"), saved, saved, ply_b, sources=sources,
                                          save_masks=False, **fkw)
        n_c = real(maps, os.path.join(data, "scan1", "pair.txt"), str(tmp_path / "c.ply"), sources=sources, **fkw)
        print("reconstruct_scene consensus", sources, "points", n_a)
        assert n_a == n_b == n_c
        assert open(ply_a, "rb").read() == open(ply_b, "rb").read() == open(str(tmp_path / "c.ply"), "rb").read()
        results[sources] = n_a
    # the default stays the pair filters' path
    monkeypatch.setattr(scene.SceneMaps, "fuse", pair_path)
    n_p = scene.reconstruct_scene(net, data, "scan1", str(tmp_path / "p.ply"), conf=(0.0, 0.0, 0.0), thres_view=2,
                                  method="pcd", **kw)
    n_q = scene.reconstruct_scene(net, data, "scan1", str(tmp_path / "q.ply"), fusion="pairs", conf=(0.0, 0.0, 0.0),
                                  thres_view=2, method="pcd", **kw)
    assert n_p == n_q and open(str(tmp_path / "p.ply"), "rb").read() == open(str(tmp_path / "q.ply"), "rb").read()
    assert len(kept) == 2
