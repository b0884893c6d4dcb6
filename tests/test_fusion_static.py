"""CPU: depth fusion pinned to the reference's own filters.

tests/golden/fusion_ref.npz holds what filter/dypcd.py and filter/pcd.py themselves computed on the scenes of
tests/fusion_fixture.py (tests/golden/make_fusion.py; every remap coordinate integral, so the cv2.remap stand-in is
exact). Here, without a GPU:
  * oracle/fusion_oracle.py (the checker of tests/test_fusion.py) equals the dypcd fixtures exactly: masks, averaged
    depth (float64, bit for bit), reprojected depth, world points and colours;
  * `pcd_fuse_view` below, a numpy restatement of filter/pcd.py built from the oracle's remap_linear (the checker of
    the static rule's bilinear path in tests/test_gpu_fusion_static.py), equals the pcd fixtures exactly;
  * damvs_fusion_view_static validates its arguments before any device work; fuse_view rejects an unknown method.
"""
import ctypes
import os

import numpy as np
import pytest

import fusion_fixture as FF
from conftest import golden
from oracle import fusion_oracle as FO


@pytest.fixture(scope="module")
def ref():
    return golden("fusion_ref")


@pytest.fixture(scope="module")
def cases():
    return FF.cases()


# ---------------------------------------------------------------- numpy restatement of filter/pcd.py
def pcd_reproject(depth_ref, K_ref, E_ref, depth_src, K_src, E_src):
    """filter/pcd.py:58-95: dypcd's reprojection without the `== 0 -> += 1e-5` guard on the reprojected z."""
    height, width = depth_ref.shape
    x_ref, y_ref = np.meshgrid(np.arange(0, width), np.arange(0, height))
    x_ref, y_ref = x_ref.reshape([-1]), y_ref.reshape([-1])
    xyz_ref = np.matmul(np.linalg.inv(K_ref), np.vstack((x_ref, y_ref, np.ones_like(x_ref))) * depth_ref.reshape([-1]))
    xyz_src = np.matmul(np.matmul(E_src, np.linalg.inv(E_ref)), np.vstack((xyz_ref, np.ones_like(x_ref))))[:3]
    K_xyz_src = np.matmul(K_src, xyz_src)
    xy_src = K_xyz_src[:2] / K_xyz_src[2:3]
    x_src = xy_src[0].reshape([height, width]).astype(np.float32)
    y_src = xy_src[1].reshape([height, width]).astype(np.float32)
    sampled = FO.remap_linear(depth_src, x_src, y_src)
    xyz_src = np.matmul(np.linalg.inv(K_src), np.vstack((xy_src, np.ones_like(x_ref))) * sampled.reshape([-1]))
    xyz_rep = np.matmul(np.matmul(E_ref, np.linalg.inv(E_src)), np.vstack((xyz_src, np.ones_like(x_ref))))[:3]
    depth_rep = xyz_rep[2].reshape([height, width]).astype(np.float32)
    K_xyz_rep = np.matmul(K_ref, xyz_rep)
    xy_rep = K_xyz_rep[:2] / K_xyz_rep[2:3]
    return (depth_rep, xy_rep[0].reshape([height, width]).astype(np.float32),
            xy_rep[1].reshape([height, width]).astype(np.float32))


def pcd_check(depth_ref, K_ref, E_ref, depth_src, K_src, E_src, dist_thr=1, rel_thr=0.01):
    """filter/pcd.py:98-113 -> (mask, reprojected depth zeroed off the mask)."""
    height, width = depth_ref.shape
    x_ref, y_ref = np.meshgrid(np.arange(0, width), np.arange(0, height))
    depth_rep, x_rep, y_rep = pcd_reproject(depth_ref, K_ref, E_ref, depth_src, K_src, E_src)
    dist = np.sqrt((x_rep - x_ref) ** 2 + (y_rep - y_ref) ** 2)
    rel = np.abs(depth_rep - depth_ref) / depth_ref
    mask = np.logical_and(dist < dist_thr, rel < rel_thr)
    depth_rep[~mask] = 0
    return mask, depth_rep


def pcd_fuse_view(depth_ref, K_ref, E_ref, srcs, confs, conf_thr, thres_view, img=None):
    """One reference view of filter/pcd.py:142-170, 190-210 -> the dict of fusion_oracle.fuse_view."""
    with np.errstate(all="ignore"):
        photo = np.ones(depth_ref.shape, bool) if confs is None else np.logical_and(
            np.logical_and(confs[0] > conf_thr[2], confs[1] > conf_thr[1]), confs[2] > conf_thr[0])
        geo_sum, reps = 0, []
        for depth_src, K_src, E_src in srcs:
            mask, depth_rep = pcd_check(depth_ref, K_ref, E_ref, depth_src, K_src, E_src)
            geo_sum = geo_sum + mask.astype(np.int32)
            reps.append(depth_rep)
        depth_avg = (sum(reps) + depth_ref) / (geo_sum + 1)
        geo = geo_sum >= thres_view
        final = np.logical_and(photo, geo)
        height, width = depth_avg.shape[:2]
        x, y = np.meshgrid(np.arange(0, width), np.arange(0, height))
        x, y, depth = x[final], y[final], depth_avg[final]
        xyz_ref = np.matmul(np.linalg.inv(K_ref), np.vstack((x, y, np.ones_like(x))) * depth)
        xyz_world = np.matmul(np.linalg.inv(E_ref), np.vstack((xyz_ref, np.ones_like(x))))[:3].T
    rgb = (img[final] * 255).astype(np.uint8) if img is not None else None
    return {"photo": photo, "geo": geo, "final": final, "depth_avg": depth_avg, "xyz": xyz_world, "rgb": rgb}


# ---------------------------------------------------------------- helpers shared with the GPU tests
def view_inputs(views, ref_view, src_views):
    v = views[ref_view]
    srcs = [(views[s]["depth"], views[s]["K"], views[s]["E"]) for s in src_views]
    img = v["img"].astype(np.float32) / 255.0  # mvsio.read_img / the reference's read_img
    return v["depth"], v["K"], v["E"], srcs, v["confs"], img


def same(a, b):
    """Bit-for-bit equality of float arrays, NaNs at the same places."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def run_case(fn, ref, case, name, views, pairs):
    """fn(view inputs...) per reference view against the fixtures of filter_depth for (case, rule name)."""
    xyz, rgb = [], []
    for i, (rv, sv) in enumerate(pairs):
        r = fn(*view_inputs(views, rv, sv))
        for kind in ("photo", "geo", "final"):
            assert np.array_equal(r[kind], ref["%s_%s_%s" % (case, name, kind)][i]), (case, name, kind, rv)
        assert same(r["depth_avg"], ref["%s_%s_depth_avg" % (case, name)][i]), (case, name, rv)
        xyz.append(r["xyz"].astype(np.float32))
        rgb.append(r["rgb"])
    assert same(np.concatenate(xyz), ref["%s_%s_xyz" % (case, name)])
    assert np.array_equal(np.concatenate(rgb), ref["%s_%s_rgb" % (case, name)])


# ---------------------------------------------------------------- tests
@pytest.mark.parametrize("case", ["scene", "edge", "pert"])
def test_oracle_equals_reference_dypcd(ref, cases, case):
    views, pairs, _ = cases[case]

    def fn(d, K, E, srcs, confs, img):
        with np.errstate(all="ignore"):
            return FO.fuse_view(d, K, E, srcs, confs, FF.CONF_THR, FF.DIST_BASE, FF.REL_DIFF_BASE, img=img)
    run_case(fn, ref, case, "dypcd", views, pairs)


@pytest.mark.parametrize("case", ["scene", "edge", "pert"])
def test_pcd_restatement_equals_reference_pcd(ref, cases, case):
    views, pairs, tv = cases[case]
    assert int(ref["%s_thres_view" % case][0]) == tv
    run_case(lambda d, K, E, srcs, confs, img: pcd_fuse_view(d, K, E, srcs, confs, FF.CONF_THR, tv, img=img),
             ref, case, "pcd", views, pairs)


@pytest.mark.parametrize("case", ["scene", "pert"])
def test_check_geometric_consistency_equals_reference(ref, cases, case):
    views, pairs, _ = cases[case]
    rv, sv = pairs[0]
    V = views
    with np.errstate(all="ignore"):
        for j, s in enumerate(sv):
            masks, mask, rep = FO.check_geometric_consistency(V[rv]["depth"].copy(), V[rv]["K"], V[rv]["E"], V[s]["depth"],
                                                              V[s]["K"], V[s]["E"], FF.DIST_BASE, FF.REL_DIFF_BASE)
            assert np.array_equal(np.stack(masks), ref["%s_cgc_dypcd_masks" % case][j])
            assert np.array_equal(mask, ref["%s_cgc_dypcd_mask" % case][j])
            assert same(rep, ref["%s_cgc_dypcd_rep" % case][j])
            mask, rep = pcd_check(V[rv]["depth"].copy(), V[rv]["K"], V[rv]["E"], V[s]["depth"], V[s]["K"], V[s]["E"])
            assert np.array_equal(mask, ref["%s_cgc_pcd_mask" % case][j])
            assert same(rep, ref["%s_cgc_pcd_rep" % case][j])


def test_fixture_covers_what_the_tests_rely_on(ref):
    """Both outcomes of every mask, the two rules apart, the edge views as designed (the generator asserts the same)."""
    for name in ("dypcd", "pcd"):
        for g in ref["scene_%s_geo" % name]:
            assert 0.05 <= g.mean() <= 0.95
        assert all(f.any() for f in ref["scene_%s_final" % name]) and len(ref["scene_%s_xyz" % name]) >= 100
        assert not ref["edge_%s_geo" % name][1].any() and ref["edge_%s_geo" % name][0].any()  # nsrc = 1, nsrc = 10
    assert (ref["scene_dypcd_geo"] != ref["scene_pcd_geo"]).mean() >= 0.05
    assert not ref["edge_pcd_geo"][2].any() and ref["edge_dypcd_geo"][2].any()  # thres_view 5 > nsrc 4
    assert [len(s) for _, s in FF.EDGE_PAIRS] == [10, 1, 4] and FF.EDGE_THRES_VIEW == 5


def test_static_entry_validates_before_device_work():
    """damvs_fusion_view_static: null / bad arguments come back as DAMVS_E_ARG / DAMVS_E_SHAPE with no GPU present."""
    from damvsnet_amd import _capi, build
    build.build()
    lib = _capi.load_library()
    E_ARG, E_SHAPE = -1, -2
    cams = _capi.DamvsFusionCams()
    p = ctypes.c_void_p(256)  # never dereferenced: every call below fails validation
    src = lambda n, null_at=None: (ctypes.c_void_p * max(n, 1))(*[None if i == null_at else 256 for i in range(max(n, 1))])
    conf3 = (ctypes.c_void_p * 3)(256, 256, 256)
    thr = (ctypes.c_float * 3)(0.1, 0.15, 0.9)

    def call(H=24, W=40, nsrc=2, dref=p, dsrc=None, conf=None, cthr=None, cm=ctypes.byref(cams), tv=1, davg=p, mask=p):
        return lib.damvs_fusion_view_static(None, H, W, nsrc, dref, dsrc if dsrc is not None else src(nsrc), conf, cthr,
                                            cm, 1.0, 0.01, tv, davg, mask, None)
    assert call(dref=None) == E_ARG and b"null" in lib.damvs_last_error_string()
    assert call(davg=None) == E_ARG and call(mask=None) == E_ARG and call(cm=None) == E_ARG
    assert lib.damvs_fusion_view_static(None, 24, 40, 2, p, None, None, None, ctypes.byref(cams), 1.0, 0.01, 1, p, p,
                                        None) == E_ARG
    assert call(H=0) == E_SHAPE and call(W=-3) == E_SHAPE and call(H=65536, W=32768) == E_SHAPE
    assert call(nsrc=0) == E_SHAPE
    assert call(nsrc=11, dsrc=src(11)) == E_SHAPE and b"nsrc 11" in lib.damvs_last_error_string()
    assert call(dsrc=src(2, null_at=1)) == E_ARG
    assert call(conf=(ctypes.c_void_p * 3)(256, None, 256), cthr=thr) == E_ARG
    assert call(conf=conf3, cthr=None) == E_ARG
    assert call(tv=0) == E_ARG and b"thres_view" in lib.damvs_last_error_string()
    assert call(tv=-2) == E_ARG
    # the kernel's 32-bit pixel index: H * W may not come within a block (256) of 2^31
    assert call(H=1, W=2 ** 31 - 255) == E_SHAPE and call(H=2, W=2 ** 30 - 100) == E_SHAPE
    # the dynamic entry's validation is unchanged by the shared packing
    assert lib.damvs_fusion_view(None, 24, 40, 11, p, src(11), None, None, ctypes.byref(cams), 0.25, 1 / 1300, p, p,
                                 None) == E_SHAPE
    assert lib.damvs_fusion_view(None, 24, 40, 2, None, src(2), None, None, ctypes.byref(cams), 0.25, 1 / 1300, p, p,
                                 None) == E_ARG


def test_foreign_fusion_library_is_refused(tmp_path):
    """libdamvs.so's build id vouches for the pair: beside a libdamvs_fusion.so stamped from other sources it reports
    both stamps, which the loader's comparison with the source hash refuses (no compute call is made)."""
    import shutil
    import subprocess
    import sys
    from damvsnet_amd import build
    build.build()
    shutil.copy(build.LIB, str(tmp_path / "libdamvs.so"))
    src = os.path.join(build.CSRC, "k_fusion_static.hip")
    subprocess.run([build.HIPCC] + build.CFLAGS + build.FILE_FLAGS["k_fusion_static.hip"] +
                   ['-DDAMVS_BUILD_ID="foreign"', "-x", "hip", "-shared", src, "-o", str(tmp_path / "libdamvs_fusion.so")],
                   check=True, capture_output=True)
    code = ("import torch, ctypes; L = ctypes.CDLL(%r); L.damvs_build_id.restype = ctypes.c_char_p; "
            "print(L.damvs_build_id().decode())" % str(tmp_path / "libdamvs.so"))
    got = subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True).stdout.strip()
    want = build.source_hash()
    assert got != want and got.startswith(want) and "libdamvs_fusion.so: foreign" in got, got


def test_fuse_view_rejects_unknown_method():
    from damvsnet_amd.fusion import fuse_view, filter_depth
    with pytest.raises(ValueError):
        fuse_view(None, None, None, [], method="nope")
    with pytest.raises(ValueError):
        filter_depth("x", "x", "x", "x.ply", method="gipuma")
