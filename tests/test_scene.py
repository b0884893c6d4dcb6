"""CPU: scene ingest (damvs_scene_ingest, damvsnet_amd/scene.py) without a GPU.

  * the C entry point's validation: every error of include/damvs.h comes back as DAMVS_E_ARG / DAMVS_E_SHAPE before
    any device work, with a message that names the problem;
  * the package exports SceneMaps and reconstruct_scene;
  * `ingest_statement`: the numpy statement of what one ingest writes, built from mvsio.resize_nearest and the float32
    np.clip(img * 255, 0, 255).astype(np.uint8) (test_uni.py:257-259, 285). tests/test_gpu_scene.py compares the
    kernel against it, exactly; here it is pinned to mvsio.save_stage_outputs (the confidence PFMs read back equal it)
    and, at the ratios the kernel serves, to the shifts y >> 1, x >> 1 and y >> 2, x >> 2;
  * `plane_case`: the forward-shaped outputs of the byte-identical-PLY test, with the condition that makes agreement
    mean something (per view a kept fraction in [0.05, 0.95], at least 1000 points in all) checked here on the CPU
    restatements of both filters alone;
  * EvalScenes' view cache returns the samples of the uncached dataset and opens every file once.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

from damvsnet_amd import mvsio

E_ARG, E_SHAPE = -1, -2
# the thresholds of the plane case (args.conf: stage 1, stage 2, stage 3): uniform confidences pass the photometric
# test with probability 0.9 * 0.85 * 0.5 = 0.38, so with the geometric masks of the noisy plane both outcomes occur in
# every view under both rules (checked below); the reference's own 0.9 for the last stage would keep 7.6 % times the
# geometric fraction, at the 0.05 bound
PLANE_CONF = (0.1, 0.15, 0.5)
PLANE_PCD_THRES_VIEW = 2
KEPT_MIN, KEPT_MAX, POINTS_MIN = 0.05, 0.95, 1000


def ingest_statement(depth, conf3, conf2, conf1, img):
    """One sample: depth, conf3 (H, W), conf2 (H/2, W/2), conf1 (H/4, W/4) float32, img (3, H, W) float32 or None ->
    (depth_store[s] (H, W), conf_store[s] (3, H, W), rgb_store[s] (H, W, 3) uint8 or None)."""
    H, W = depth.shape
    conf = np.stack([conf3, mvsio.resize_nearest(conf2, W, H), mvsio.resize_nearest(conf1, W, H)])
    rgb = None
    if img is not None:
        assert img.dtype == np.float32
        rgb = np.clip(np.transpose(img, (1, 2, 0)) * 255, 0, 255).astype(np.uint8)
    return depth, conf, rgb


# ----------------------------------------------------------------------------------------------- C entry point
@pytest.fixture(scope="module")
def lib():
    from damvsnet_amd import _capi, build
    build.build()
    return _capi.load_library()


def test_scene_ingest_validates_before_device_work(lib):
    P = 256  # never dereferenced: every call below fails validation
    ints = lambda *v: (ctypes.c_int * len(v))(*v)

    def call(B=3, H=8, W=12, V=6, depth=P, conf3=P, conf2=P, conf1=P, img=P, stride=3 * 3 * 96, slots=None,
             dstore=P, cstore=P, rstore=P):
        slots = ints(5, 0, 2) if slots is None else slots
        return lib.damvs_scene_ingest(None, B, H, W, V, depth, conf3, conf2, conf1, img, stride, slots, dstore, cstore,
                                      rstore)

    err = lambda: lib.damvs_last_error_string()
    for name in ("depth", "conf3", "conf2", "conf1", "dstore", "cstore"):
        assert call(**{name: None}) == E_ARG and b"null" in err(), name
    assert lib.damvs_scene_ingest(None, 3, 8, 12, 6, P, P, P, P, P, 0, None, P, P, P) == E_ARG and b"null" in err()
    assert call(rstore=None) == E_ARG and b"rgb_store" in err()  # an image to convert and nowhere to put it
    assert call(slots=ints(5, 6, 2)) == E_ARG and b"slot 6" in err()
    assert call(slots=ints(5, -1, 2)) == E_ARG and b"slot -1" in err()
    assert call(slots=ints(5, 0, 5)) == E_ARG and b"repeated" in err() and b"slot 5" in err()
    assert call(B=0) == E_SHAPE and b"B 0" in err()
    assert call(B=65, slots=ints(*range(65)), V=65) == E_SHAPE and b"B 65" in err()
    assert call(B=-1) == E_SHAPE
    for H, W in ((0, 12), (8, 0), (-4, 12), (8, -4), (6, 12), (8, 10), (7, 13)):
        assert call(H=H, W=W) == E_SHAPE and b"multiples of 4" in err(), (H, W)
    assert call(V=0) == E_SHAPE and b"V 0" in err()
    assert call(V=2) == E_ARG  # slots 5 and 2 are outside [0, 2)
    # H * W * 12 < 2^31: the first multiple-of-4 height past it at W = 13376 is refused
    assert 13376 * 13376 * 12 < 2 ** 31 <= 13380 * 13376 * 12
    assert call(H=13380, W=13376) == E_SHAPE and b"2 GiB" in err()
    assert call(H=4, W=2 ** 30) == E_SHAPE
    # the 16-byte accesses of the kernel
    assert call(depth=260) == E_ARG and b"aligned" in err()
    assert call(conf2=260) == E_ARG and call(rstore=258) == E_ARG and call(stride=3 * 3 * 96 + 2) == E_ARG


def test_binding_and_exports():
    import damvsnet_amd
    from damvsnet_amd import _capi, scene
    assert damvsnet_amd.SceneMaps is scene.SceneMaps and damvsnet_amd.reconstruct_scene is scene.reconstruct_scene
    assert {"SceneMaps", "reconstruct_scene"} <= set(damvsnet_amd.__all__)
    assert "damvs_scene_ingest" in [s[0] for s in _capi.SIGNATURES] and _capi.SCENE_MAX_BATCH == 64
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "damvs.h")).read()
    assert "#define DAMVS_SCENE_MAX_BATCH 64" in header
    assert "test_uni.py:246-287" in header and "filter/dypcd.py:198-209" in header


def test_scene_maps_refuses_bad_sizes_without_a_device():
    from damvsnet_amd.scene import SceneMaps
    for H, W in ((6, 8), (8, 10), (0, 8)):
        with pytest.raises(ValueError, match="multiples of 4"):
            SceneMaps([0, 1], H, W, "cpu")
    with pytest.raises(ValueError, match="distinct"):
        SceneMaps([0, 1, 0], 8, 8, "cpu")


# --------------------------------------------------------------------------------------- the numpy statement
def test_statement_upsampling_is_the_shift():
    rng = np.random.default_rng(0)
    for H, W in ((4, 4), (8, 12), (36, 260)):
        c2 = np.arange(H * W // 4, dtype=np.float32).reshape(H // 2, W // 2)
        c1 = np.arange(H * W // 16, dtype=np.float32).reshape(H // 4, W // 4)
        d = rng.random((H, W), dtype=np.float32)
        _, conf, _ = ingest_statement(d, d, c2, c1, None)
        y, x = np.mgrid[:H, :W]
        assert np.array_equal(conf[1], c2[y >> 1, x >> 1]) and np.array_equal(conf[2], c1[y >> 2, x >> 2])


def test_statement_colour_is_clip_then_truncate():
    v = np.array([0, 1, np.nextafter(np.float32(1), np.float32(2)), -0.25, 254.999 / 255, 0.5 / 255, 128 / 255],
                 dtype=np.float32)
    img = np.broadcast_to(v.reshape(1, 1, -1), (3, 1, 7)).copy()
    z = np.zeros((1, 7), np.float32)
    _, _, rgb = ingest_statement(z, z, z, z, img)
    assert rgb[0, :, 0].tolist() == [0, 255, 255, 0, 254, 0, 128]
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    assert np.array_equal(np.clip(k * 255, 0, 255).astype(np.uint8), np.arange(256))


def test_statement_equals_save_stage_outputs(tmp_path):
    """The confidence PFMs mvsio.save_stage_outputs writes (test_uni.py:257-282) read back equal the statement, the
    depth PFM too."""
    rng = np.random.default_rng(3)
    B, H, W = 2, 36, 260
    f = lambda *s: rng.random(s, dtype=np.float32)
    out = {"depth": f(B, H, W) * 500 + 400, "photometric_confidence": f(B, H, W),
           "stage2": {"depth": f(B, H // 2, W // 2), "photometric_confidence": f(B, H // 2, W // 2)},
           "stage1": {"depth": f(B, H // 4, W // 4), "photometric_confidence": f(B, H // 4, W // 4)}}
    for b in range(B):
        mvsio.save_stage_outputs(str(tmp_path), "scan/{}/%08d{}" % b, out, b)
        depth, conf, _ = ingest_statement(out["depth"][b], out["photometric_confidence"][b],
                                          out["stage2"]["photometric_confidence"][b],
                                          out["stage1"]["photometric_confidence"][b], None)
        rd = lambda kind, sfx: mvsio.read_pfm(str(tmp_path / "scan" / kind / ("%08d%s.pfm" % (b, sfx))))[0]
        assert np.array_equal(rd("depth_est", ""), depth)
        for k, sfx in enumerate(("", "_stage2", "_stage1")):
            assert np.array_equal(rd("confidence", sfx), conf[k]), (b, sfx)


# ------------------------------------------------------------------------------------------- the plane case
@functools.lru_cache(maxsize=None)
def plane_case():
    """5 views of tests/test_fusion.plane_scene at 96 x 128 as a forward would hand them over: `outputs` (numpy, batch
    of 5: final depth and confidence, stage-2 / stage-1 confidences at half / quarter size, stage depths that only
    save_stage_outputs reads), `rgb` (5, 96, 128, 3) uint8, `cams` (5, 2, 4, 4) as proj_matrices["stage3"][:, 0] and
    the pair list (every view against the four others)."""
    from test_fusion import plane_scene
    N, H, W = 5, 96, 128
    depths, K, E, _, _ = plane_scene(N, H=H, W=W)
    rng = np.random.default_rng(16)
    f = lambda *s: rng.random(s, dtype=np.float32)
    outputs = {"depth": np.stack(depths).astype(np.float32), "photometric_confidence": f(N, H, W),
               "stage2": {"depth": f(N, H // 2, W // 2) + 500, "photometric_confidence": f(N, H // 2, W // 2)},
               "stage1": {"depth": f(N, H // 4, W // 4) + 500, "photometric_confidence": f(N, H // 4, W // 4)}}
    rgb = rng.integers(0, 256, size=(N, H, W, 3), dtype=np.uint8)
    cams = np.zeros((N, 2, 4, 4), np.float32)
    cams[:, 0] = E
    cams[:, 1, :3, :3] = K
    cams[:, 1, 3, :2] = 425.0, 2.5
    pairs = [(r, [s for s in range(N) if s != r]) for r in range(N)]
    return {"outputs": outputs, "rgb": rgb, "cams": cams, "pairs": pairs, "H": H, "W": W, "N": N}


def kept_fractions_ok(fractions, total):
    return all(KEPT_MIN <= f <= KEPT_MAX for f in fractions) and total >= POINTS_MIN


@pytest.mark.parametrize("method", ["dypcd", "pcd"])
def test_plane_case_keeps_and_drops_points_in_every_view(method):
    """oracle.fusion_oracle.fuse_view (dypcd) and the static rule's restatement (tests/test_fusion_static.py) alone, on
    the statement's maps: per view the kept fraction lies in [0.05, 0.95] and the cloud has at least 1000 points."""
    from oracle import fusion_oracle as FO
    from test_fusion_static import pcd_fuse_view
    c = plane_case()
    o, cams = c["outputs"], c["cams"]
    maps = [ingest_statement(o["depth"][v], o["photometric_confidence"][v], o["stage2"]["photometric_confidence"][v],
                             o["stage1"]["photometric_confidence"][v], None) for v in range(c["N"])]
    K, E = cams[:, 1, :3, :3], cams[:, 0]
    fractions = []
    for r, src in c["pairs"]:
        srcs = [(maps[s][0], K[s], E[s]) for s in src]
        if method == "dypcd":
            got = FO.fuse_view(maps[r][0], K[r], E[r], srcs, list(maps[r][1]), PLANE_CONF)
        else:
            got = pcd_fuse_view(maps[r][0], K[r], E[r], srcs, list(maps[r][1]), PLANE_CONF, PLANE_PCD_THRES_VIEW)
        fractions.append(float(got["final"].mean()))
    total = sum(f * c["H"] * c["W"] for f in fractions)
    print(method, "kept fractions", ["%.3f" % f for f in fractions], "total", int(round(total)))
    assert kept_fractions_ok(fractions, total), (fractions, total)


# ----------------------------------------------------------------------------------------- the view cache
def test_eval_scenes_view_cache_gives_the_same_samples_and_reads_once(tmp_path, monkeypatch):
    import scene_fixture as SF
    SF.make_scene(str(tmp_path))
    kw = dict(ndepths=8, interval_scale=1.06, max_h=1184, max_w=1600)
    plain = mvsio.EvalScenes(str(tmp_path), ["scan1"], SF.NV, **kw)
    cached = mvsio.EvalScenes(str(tmp_path), ["scan1"], SF.NV, cache_views=True, **kw)
    want = [plain[i] for i in range(len(plain))]
    opened = {}
    real = mvsio.read_img

    def counting(filename):
        opened[filename] = opened.get(filename, 0) + 1
        return real(filename)

    monkeypatch.setattr(mvsio, "read_img", counting)
    for _ in range(2):  # the second pass is served from the cache alone
        for i, w in enumerate(want):
            got = cached[i]
            assert np.array_equal(got["imgs"], w["imgs"]) and np.array_equal(got["depth_values"], w["depth_values"])
            for s in ("stage1", "stage2", "stage3"):
                assert np.array_equal(got["proj_matrices"][s], w["proj_matrices"][s]), (i, s)
                assert np.array_equal(got["intrinsics_matrices"][s], w["intrinsics_matrices"][s]), (i, s)
            assert got["filename"] == w["filename"]
    assert len(opened) == SF.NV and set(opened.values()) == {1}, opened
    opened.clear()
    for i in range(len(plain)):  # the default stays the reference's: every listing of a view is a read
        plain[i]
    assert sum(opened.values()) == len(plain) * SF.NV
