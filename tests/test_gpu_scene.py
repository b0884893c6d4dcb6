"""GPU: scene ingest and the in-memory path from a forward's outputs to a fused PLY (k_scene.hip, damvsnet_amd/scene.py).

Every comparison is exact (bytes or torch.equal): the kernel copies floats, indexes by shifts and converts colours by
one float32 multiply, a clamp and a truncation, which numpy does bit for bit (tests/test_scene.py ingest_statement).
  1. damvs_scene_ingest against the statement: sizes from one thread's 4 pixels (4 x 4) to a width that is no multiple
     of the block's 256 pixels with two blocks per row (36 x 260), batches of 1 and 3 into slots 5, 0, 2 of 6, the
     other slots and 64-byte guard bands around every store pre-filled with a byte pattern; reference images read in
     place as view 0 of 3 through the batch stride; without an image the colour store stays untouched.
  2. SceneMaps.add: the same through the Python layer, with imgs and with rgb (bytes copied).
  3. one ingest on a side stream beside a bf16 CascadeMVSNet.forward on the main stream equals the solo result.
  4. SceneMaps.fuse writes the PLY (and masks) fusion.fuse_scene writes over the files of the same maps, for both
     filter rules, on a scene where every view keeps and drops points (tests/test_scene.py plane_case).
  5. SceneMaps.save writes save_stage_outputs' PFMs and write_cam's files, and fuse_scene over that tree gives fuse's PLY.
  6. reconstruct_scene over tests/scene_fixture.py's tree equals the file path driven by the same forwards; every image
     file is opened once.
  7. errors raise ValueError and write no PLY.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import scene_fixture as SF
from test_scene import (ingest_statement, plane_case, kept_fractions_ok, PLANE_CONF, PLANE_PCD_THRES_VIEW)

pytestmark = pytest.mark.gpu
POISON, GUARD = 0xA5, 64
V, SLOTS = 6, [5, 0, 2]
SIZES = [(4, 4), (8, 12), (32, 64), (36, 260)]
NVIEWS = 3  # views per sample of the image batch: the batch stride is three images


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from damvsnet_amd import build, _capi
    build.build()
    return _capi.load_library()


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def raw(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()


def special_colours():
    one = np.float32(1)
    extra = np.array([0, 1, np.nextafter(one, np.float32(2)), -0.25, 254.999 / 255, 0.5 / 255], dtype=np.float32)
    return np.concatenate([extra, np.arange(256, dtype=np.float32) / np.float32(255)])


@functools.lru_cache(maxsize=None)
def ingest_case(H, W, B):
    """Inputs of one launch and, per sample, what the statement says its slot holds."""
    rng = np.random.default_rng(H * 1009 + W * 7 + B)
    bits = lambda *s: rng.integers(0, 2 ** 32, size=s, dtype=np.uint32).view(np.float32)  # any bit pattern is copied
    depth, conf3 = bits(B, H, W), bits(B, H, W)
    # a distinct value per source pixel: a wrong shift or a transposed index shows
    conf2 = (np.arange(B * H * W // 4, dtype=np.float32) + np.float32(0.5)).reshape(B, H // 2, W // 2)
    conf1 = (np.arange(B * H * W // 16, dtype=np.float32) + np.float32(0.25)).reshape(B, H // 4, W // 4)
    imgs = rng.random((B, NVIEWS, 3, H, W), dtype=np.float32)
    sp = special_colours()
    for b in range(B):  # view 0 carries the special values, rotated per sample so that small images see all kinds
        imgs[b, 0] = np.resize(np.roll(sp, -37 * b), 3 * H * W).reshape(3, H, W)
    want = [ingest_statement(depth[b], conf3[b], conf2[b], conf1[b], imgs[b, 0]) for b in range(B)]
    return {"depth": depth, "conf3": conf3, "conf2": conf2, "conf1": conf1, "imgs": imgs, "want": want}


def guarded(nbytes):
    """A poisoned buffer with `nbytes` of payload between two guard bands -> (whole buffer, payload view)."""
    flat = torch.full((GUARD + nbytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    return flat, flat[GUARD:GUARD + nbytes]


def prepare(c, H, W, B):
    """The device inputs of one launch and guarded, poisoned stores, all resident before anything is launched."""
    dev = {k: cu(c[k]) for k in ("depth", "conf3", "conf2", "conf1", "imgs")}
    stores = [guarded(V * H * W * 4), guarded(V * 3 * H * W * 4), guarded(V * H * W * 3)]
    torch.cuda.synchronize()
    return stores, dev


def launch(lib, stores, dev, H, W, B, with_img=True, stream=None):
    from damvsnet_amd import _capi
    slots = (ctypes.c_int * B)(*SLOTS[:B])
    img = dev["imgs"].data_ptr() if with_img else None
    s = _capi.stream_ptr() if stream is None else stream.cuda_stream
    _capi.check(lib.damvs_scene_ingest(s, B, H, W, V, dev["depth"].data_ptr(), dev["conf3"].data_ptr(),
                                       dev["conf2"].data_ptr(), dev["conf1"].data_ptr(), img, NVIEWS * 3 * H * W, slots,
                                       stores[0][1].data_ptr(), stores[1][1].data_ptr(), stores[2][1].data_ptr()))


def run_ingest(lib, c, H, W, B, with_img=True):
    """damvs_scene_ingest into guarded, poisoned stores -> the three whole buffers."""
    stores, dev = prepare(c, H, W, B)
    launch(lib, stores, dev, H, W, B, with_img)
    torch.cuda.synchronize()
    return stores


def check_stores(stores, c, H, W, B, with_img=True):
    poison = lambda n: bytes([POISON]) * n
    per_slot = (H * W * 4, 3 * H * W * 4, H * W * 3)
    for kind, ((flat, _), n) in enumerate(zip(stores, per_slot)):
        got = raw(flat)
        assert got[:GUARD] == poison(GUARD) and got[-GUARD:] == poison(GUARD), "guard band of store %d" % kind
        for slot in range(V):
            have = got[GUARD + slot * n:GUARD + (slot + 1) * n]
            if slot in SLOTS[:B] and (kind < 2 or with_img):
                want = c["want"][SLOTS.index(slot)][kind]
                assert have == np.ascontiguousarray(want).tobytes(), "store %d slot %d" % (kind, slot)
            else:
                assert have == poison(n), "store %d slot %d was touched" % (kind, slot)


# ------------------------------------------------------------------------------------- 1. the entry point
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_ingest_equals_numpy_statement(lib, size, B):
    H, W = size
    c = ingest_case(H, W, B)
    stores = run_ingest(lib, c, H, W, B)
    check_stores(stores, c, H, W, B)
    if (H, W) == (36, 260):  # every kind of colour value went through the kernel
        assert set(np.unique(c["want"][0][2])) == set(range(256))


@pytest.mark.parametrize("size", [(4, 4), (36, 260)], ids=lambda s: "%dx%d" % s)
def test_ingest_without_image_leaves_the_colour_store(lib, size):
    H, W = size
    c = ingest_case(H, W, 3)
    stores = run_ingest(lib, c, H, W, 3, with_img=False)
    check_stores(stores, c, H, W, 3, with_img=False)


# ------------------------------------------------------------------------------------- 2. SceneMaps.add
def forward_shaped(c):
    return {"depth": cu(c["depth"]), "photometric_confidence": cu(c["conf3"]),
            "stage2": {"photometric_confidence": cu(c["conf2"])}, "stage1": {"photometric_confidence": cu(c["conf1"])}}


def poisoned_maps(view_ids, H, W):
    from damvsnet_amd.scene import SceneMaps
    maps = SceneMaps(view_ids, H, W, "cuda")
    for t in (maps.depth, maps.conf, maps.rgb):
        t.view(torch.uint8).fill_(POISON)
    return maps


@pytest.mark.parametrize("colour", ["imgs", "rgb"])
def test_scene_maps_add(lib, colour):
    H, W, B = 36, 260, 3
    c = ingest_case(H, W, B)
    ids = [10, 11, 12, 13, 14, 15]  # slot = position: views 15, 10, 12 land in slots 5, 0, 2
    maps = poisoned_maps(ids, H, W)
    rgb = np.random.default_rng(2).integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
    cams = np.arange(B * 32, dtype=np.float32).reshape(B, 2, 4, 4)
    if colour == "imgs":
        maps.add([15, 10, 12], forward_shaped(c), imgs=cu(c["imgs"]), cams=cams)
    else:
        maps.add([15, 10, 12], forward_shaped(c), rgb=cu(rgb), cams=cams)
    for b, slot in enumerate(SLOTS):
        depth, conf, col = c["want"][b]
        assert raw(maps.depth[slot]) == depth.tobytes() and raw(maps.conf[slot]) == conf.tobytes()
        assert raw(maps.rgb[slot]) == (col if colour == "imgs" else rgb[b]).tobytes()
        K, E = maps.cams[ids[slot]]
        assert np.array_equal(E, cams[b, 0]) and np.array_equal(K, cams[b, 1, :3, :3])
    for slot in (1, 3, 4):
        for t in (maps.depth, maps.conf, maps.rgb):
            assert set(raw(t[slot])) == {POISON}


# ------------------------------------------------------------------------------------- 3. beside a forward
def test_ingest_on_a_side_stream_beside_a_bf16_forward(lib):
    """One ingest launch on a side stream while a bf16 CascadeMVSNet.forward runs on the main stream, once: the stores
    equal the solo result (the kernel is VALU only and carries no packed-FP32 ops, tests/test_scene_codeobj.py)."""
    from common import model_state, forward_inputs
    from damvsnet_amd.cascade import CascadeMVSNet
    H, W, B = 36, 260, 3
    c = ingest_case(H, W, B)
    solo = run_ingest(lib, c, H, W, B)
    check_stores(solo, c, H, W, B)
    net = CascadeMVSNet(ndepths=[8, 8, 8], compute_dtype=torch.bfloat16, frontend_dtype=torch.bfloat16)
    net.load_state_dict(model_state("forward_160x128_48_32_8"), strict=True)
    net = net.cuda().eval()
    imgs, proj, dv, _ = forward_inputs(1, 3, 32, 64)
    imgs, dv, proj = imgs.cuda(), dv.cuda(), {k: v.cuda() for k, v in proj.items()}
    side = torch.cuda.Stream()
    beside, dev = prepare(c, H, W, B)  # synchronises: the side stream has nothing to wait for
    with torch.no_grad():
        out = net(imgs, proj, dv, check_range=False)  # enqueued on the main stream, not waited for
    launch(lib, beside, dev, H, W, B, stream=side)
    torch.cuda.synchronize()
    net.DepthNet.check_range()
    assert out["depth"].shape == (1, 32, 64)
    for (a, _), (b, _) in zip(solo, beside):
        assert torch.equal(a, b)
    check_stores(beside, c, H, W, B)


# ------------------------------------------------------------------------------------- 4. fuse vs the file path
def write_pairs(path, pairs):
    with open(path, "w") as f:
        f.write("%d\n" % len(pairs))
        for ref, src in pairs:
            f.write("%d\n%d %s\n" % (ref, len(src), " ".join("%d 1.0" % s for s in src)))


def part(o, lo, hi):
    return {k: part(v, lo, hi) if isinstance(v, dict) else cu(v[lo:hi]) for k, v in o.items()}


def plane_maps():
    """Path A's stores: the plane case added in two batches (3 views, then 2)."""
    from damvsnet_amd.scene import SceneMaps
    c = plane_case()
    maps = SceneMaps(range(c["N"]), c["H"], c["W"], "cuda")
    for lo, hi in ((0, 3), (3, 5)):
        maps.add(list(range(lo, hi)), part(c["outputs"], lo, hi), rgb=cu(c["rgb"][lo:hi]), cams=c["cams"][lo:hi])
    return maps


def write_plane_tree(root):
    """Path B's files: save_stage_outputs per view, write_cam, lossless images, pair.txt -> the scan folder."""
    from PIL import Image
    from damvsnet_amd import mvsio
    c = plane_case()
    scan = os.path.join(root, "scan")
    for d in ("cams", "images"):
        os.makedirs(os.path.join(scan, d), exist_ok=True)
    for v in range(c["N"]):
        mvsio.save_stage_outputs(root, "scan/{}/%08d{}" % v, c["outputs"], v)
        mvsio.write_cam(os.path.join(scan, "cams", "%08d_cam.txt" % v), c["cams"][v])
        Image.fromarray(c["rgb"][v]).save(os.path.join(scan, "images", "%08d.jpg" % v), format="PNG")
    write_pairs(os.path.join(scan, "pair.txt"), c["pairs"])
    return scan


def read_masks(folder, views):
    from PIL import Image
    return {(v, k): np.array(Image.open(os.path.join(folder, "%08d_%s.png" % (v, k))))
            for v in views for k in ("photo", "geo", "final")}


def fuse_kw(method):
    return dict(conf=PLANE_CONF, method=method, thres_view=PLANE_PCD_THRES_VIEW if method == "pcd" else 5)


@pytest.mark.parametrize("method", ["dypcd", "pcd"])
def test_fuse_writes_the_file_paths_ply(lib, method, tmp_path):
    from damvsnet_amd import fusion
    c = plane_case()
    ply_a, ply_b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    n_a = plane_maps().fuse(c["pairs"], ply_a, mask_dir=str(tmp_path / "mask_a"), **fuse_kw(method))
    scan = write_plane_tree(str(tmp_path / "tree"))
    n_b = fusion.fuse_scene(scan, scan, scan, ply_b, **fuse_kw(method))
    assert n_a == n_b and open(ply_a, "rb").read() == open(ply_b, "rb").read()
    views = range(c["N"])
    m_a, m_b = read_masks(str(tmp_path / "mask_a"), views), read_masks(os.path.join(scan, "mask"), views)
    assert all(np.array_equal(m_a[k], m_b[k]) for k in m_b)
    kept = [float((m_a[(v, "final")] > 0).mean()) for v in views]
    print(method, "kept fractions", ["%.3f" % f for f in kept], "points", n_a)
    assert kept_fractions_ok(kept, n_a), (kept, n_a)  # an empty cloud must not pass for agreement
    assert n_a == sum(int((m_a[(v, "final")] > 0).sum()) for v in views)


# ------------------------------------------------------------------------------------- 5. save
def test_save_round_trip(lib, tmp_path):
    from damvsnet_amd import fusion
    c = plane_case()
    maps = plane_maps()
    ply = str(tmp_path / "fuse.ply")
    n = maps.fuse(c["pairs"], ply, **fuse_kw("dypcd"))
    maps.save(str(tmp_path / "saved"), "scan", lossless=True)
    saved = str(tmp_path / "saved" / "scan")
    write_pairs(os.path.join(saved, "pair.txt"), c["pairs"])
    ply_s = str(tmp_path / "saved.ply")
    assert fusion.fuse_scene(saved, saved, saved, ply_s, save_masks=False, **fuse_kw("dypcd")) == n
    assert open(ply_s, "rb").read() == open(ply, "rb").read() and n >= 1000
    tree = write_plane_tree(str(tmp_path / "tree"))
    names = ["cams/%08d_cam.txt" % v for v in range(c["N"])] + ["depth_est/%08d.pfm" % v for v in range(c["N"])] + \
        ["confidence/%08d%s.pfm" % (v, s) for v in range(c["N"]) for s in ("", "_stage2", "_stage1")]
    for name in names:
        assert open(os.path.join(saved, name), "rb").read() == open(os.path.join(tree, name), "rb").read(), name
    # the stage-1 / stage-2 depth maps are not kept, so not written
    assert sorted(os.listdir(os.path.join(saved, "depth_est"))) == ["%08d.pfm" % v for v in range(c["N"])]


# ------------------------------------------------------------------------------------- 6. reconstruct_scene
def test_reconstruct_scene_equals_the_file_path(lib, tmp_path, monkeypatch):
    """tests/scene_fixture.py's tree (32 x 64, 5 views) through a synthetic-weight fp32 model in batches of 2. The
    fixture's pair list drops view 2 as a reference and names it as a source, which neither path can fuse (there is no
    depth map of it), so view 2 gets two sources here; the rest of the tree is the fixture's. With random weights the
    cloud may be empty: this case tests the wiring, the plane case the content."""
    from PIL import Image
    from common import model_state
    from damvsnet_amd import fusion, mvsio, scene
    from damvsnet_amd.cascade import CascadeMVSNet
    data = str(tmp_path / "data")
    imgs_u8 = SF.make_scene(data)["imgs"]
    with open(os.path.join(data, "scan1", "pair.txt"), "w") as f:
        f.write("%d\n" % len(SF.PAIRS))
        for ref, src in SF.PAIRS:
            src = src or [(3, 99.5), (4, 50.25)]
            f.write("%d\n%d %s\n" % (ref, len(src), " ".join("%d %g" % p for p in src)))
    net = CascadeMVSNet(ndepths=[8, 8, 8])
    net.load_state_dict(model_state("forward_160x128_48_32_8"), strict=True)
    net = net.cuda().eval()
    kw = dict(nviews=SF.NV, ndepths=8, interval_scale=1.06, max_h=1184, max_w=1600)
    fkw = dict(conf=(0.0, 0.0, 0.0), thres_view=2, method="pcd")

    # the file path, driven by the same forwards (the same batches)
    ds = mvsio.EvalScenes(data, ["scan1"], kw["nviews"], ndepths=8, interval_scale=1.06, max_h=1184, max_w=1600)
    out_dir, forwards = str(tmp_path / "out"), {}
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    with torch.no_grad():
        for i0 in range(0, len(ds), 2):
            items = [ds[i] for i in range(i0, min(i0 + 2, len(ds)))]
            imgs = np.stack([it["imgs"] for it in items])
            proj = {k: np.stack([it["proj_matrices"][k] for it in items]) for k in ("stage1", "stage2", "stage3")}
            out = net(up(imgs), {k: up(v) for k, v in proj.items()}, up(np.stack([it["depth_values"] for it in items])))
            for b, it in enumerate(items):
                mvsio.save_stage_outputs(out_dir, it["filename"], out, b)
                ref = int(it["filename"].format("", "").split("/")[-1])
                forwards[ref] = (out["depth"][b].clone(), out["photometric_confidence"][b].clone())
                for d in ("cams", "images"):
                    os.makedirs(os.path.join(out_dir, "scan1", d), exist_ok=True)
                mvsio.write_cam(os.path.join(out_dir, it["filename"].format("cams", "_cam.txt")), proj["stage3"][b, 0])
                img = np.clip(np.transpose(imgs[b, 0], (1, 2, 0)) * 255, 0, 255).astype(np.uint8)
                Image.fromarray(img).save(os.path.join(out_dir, it["filename"].format("images", ".jpg")), format="PNG")
    scan_out = os.path.join(out_dir, "scan1")
    ply_b = str(tmp_path / "b.ply")
    n_b = fusion.fuse_scene(os.path.join(data, "scan1"), scan_out, scan_out, ply_b, save_masks=False, **fkw)

    opened, kept, real_img, real_fuse = {}, [], mvsio.read_img, scene.SceneMaps.fuse

    def counting(filename):
        opened[filename] = opened.get(filename, 0) + 1
        return real_img(filename)

    def fuse(self, *a, **k):
        kept.append(self)
        return real_fuse(self, *a, **k)

    monkeypatch.setattr(mvsio, "read_img", counting)
    monkeypatch.setattr(scene.SceneMaps, "fuse", fuse)
    ply_a = str(tmp_path / "a.ply")
    n_a = scene.reconstruct_scene(net, data, "scan1", ply_a, batch=2, **kw, **fkw)
    print("reconstruct_scene points", n_a)
    assert n_a == n_b and open(ply_a, "rb").read() == open(ply_b, "rb").read()
    assert len(opened) == SF.NV and set(opened.values()) == {1}, opened
    maps, = kept
    assert sorted(maps.view_ids) == sorted(forwards) == list(range(SF.NV))
    for v, (depth, conf) in forwards.items():
        s = maps.slot[v]
        assert torch.equal(maps.depth[s], depth) and torch.equal(maps.conf[s, 0], conf), v
    for v in range(SF.NV):  # k / 255 * 255 truncates back to k for all 256 values
        assert np.array_equal(maps.rgb[maps.slot[v]].cpu().numpy(), imgs_u8[v]), v


# ------------------------------------------------------------------------------------- 7. errors
def test_errors_raise_value_error_and_write_no_ply(lib, tmp_path):
    c = plane_case()
    H, W = c["H"], c["W"]
    from damvsnet_amd.scene import SceneMaps
    maps = SceneMaps(range(5), H, W, "cuda")
    maps.add([0, 1, 2], part(c["outputs"], 0, 3), rgb=cu(c["rgb"][0:3]), cams=c["cams"][0:3])
    ply = str(tmp_path / "never.ply")
    with pytest.raises(ValueError, match="view 3 .*never added"):
        maps.fuse(c["pairs"], ply, **fuse_kw("dypcd"))
    with pytest.raises(ValueError, match="view 4 .*never added"):
        maps.fuse([(0, [1, 4])], ply, **fuse_kw("dypcd"))
    with pytest.raises(ValueError, match="view 1 added twice"):
        maps.add([3, 1], part(c["outputs"], 3, 5), rgb=cu(c["rgb"][3:5]), cams=c["cams"][3:5])
    with pytest.raises(ValueError, match="view 7 is not one of"):
        maps.add([3, 7], part(c["outputs"], 3, 5))
    bad = part(c["outputs"], 3, 5)
    bad["stage2"]["photometric_confidence"] = bad["stage2"]["photometric_confidence"][:, :, :-1].contiguous()
    with pytest.raises(ValueError, match=r"stage2 photometric_confidence of views \[3, 4\] has shape"):
        maps.add([3, 4], bad)
    bad = part(c["outputs"], 3, 5)
    bad["depth"] = bad["depth"].transpose(1, 2).contiguous().transpose(1, 2)
    with pytest.raises(ValueError, match=r"depth of views \[3, 4\] must be contiguous"):
        maps.add([3, 4], bad)
    cpu = {k: ({kk: vv.cpu() for kk, vv in v.items()} if isinstance(v, dict) else v.cpu())
           for k, v in part(c["outputs"], 3, 5).items()}
    with pytest.raises(ValueError, match=r"views \[3, 4\] must be a CUDA tensor"):
        maps.add([3, 4], cpu)
    assert not os.path.exists(ply)
    # none of the refused calls left a trace: views 3 and 4 can still be added and the scene fuses
    maps.add([3, 4], part(c["outputs"], 3, 5), rgb=cu(c["rgb"][3:5]), cams=c["cams"][3:5])
    assert maps.fuse(c["pairs"], ply, **fuse_kw("dypcd")) >= 1000 and os.path.exists(ply)
