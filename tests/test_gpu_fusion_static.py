"""GPU: both fusion rules (fuse_view / filter_depth, method "pcd" and "dypcd") against what the reference's own
filter/pcd.py and filter/dypcd.py computed (tests/golden/fusion_ref.npz; scenes of tests/fusion_fixture.py).

Integer scene: every camera product has at most one non-zero term per sum and every remap coordinate is integral, so the
kernels must reproduce the reference bit for bit: masks on every pixel, depth_avg == float32(reference), world points
== the reference's f4 PLY vertices. Perturbed scene: the per-source masks exactly, depths within 1 float32 ulp (a
differing float64 contraction can move the float32 rounding by at most one ulp). The static rule's bilinear path
(non-integral coordinates, which the cv2.remap stand-in of the fixtures cannot cover) is checked on
test_fusion.plane_scene against the numpy restatement of filter/pcd.py in tests/test_fusion_static.py, which the CPU
tests pin to the pcd fixtures; gate as in tests/test_fusion.py.
All at 24 x 40 (96 x 128 for the plane scenes): a few seconds in total.
"""
import os

import numpy as np
import pytest
import torch

import fusion_fixture as FF
from conftest import golden
from test_fusion import plane_scene
from test_fusion_static import pcd_fuse_view, view_inputs, same

pytestmark = pytest.mark.gpu
METHODS = ("pcd", "dypcd")


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


def gpu_view(fusion, views, rv, sv, method, thres_view=5, confs=True):
    d, K, E, srcs, cf, _ = view_inputs(views, rv, sv)
    r = fusion.fuse_view(cu(d), K, E, [(cu(sd), sk, se) for sd, sk, se in srcs], [cu(c) for c in cf] if confs else None,
                         FF.CONF_THR, FF.DIST_BASE, FF.REL_DIFF_BASE, method=method, thres_view=thres_view)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def ulps(a, b):
    """|a - b| in float32 ulps of b (both finite)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b)).astype(np.float64)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("case", ["scene", "edge"])
def test_integer_scene_equals_reference(fusion, ref, cases, case, method):
    views, pairs, tv = cases[case]
    key = "%s_%s_" % (case, method)
    at = 0
    for i, (rv, sv) in enumerate(pairs):
        got = gpu_view(fusion, views, rv, sv, method, tv)
        for kind in ("photo", "geo", "final"):
            diff = int((got[kind] != ref[key + kind][i]).sum())
            assert diff == 0, (case, method, kind, rv, diff)
        assert same(got["depth_avg"], ref[key + "depth_avg"][i].astype(np.float32)), (case, method, rv)
        fin = ref[key + "final"][i]
        n = int(fin.sum())
        assert same(got["xyz"][fin], ref[key + "xyz"][at:at + n]), (case, method, rv)
        assert not got["xyz"][~fin].any()
        at += n
    assert at == len(ref[key + "xyz"])


@pytest.mark.parametrize("method", METHODS)
def test_edge_views(fusion, ref, cases, method):
    """nsrc = 10, nsrc = 1, the static count above nsrc, and confs=None (photo all true)."""
    views, pairs, tv = cases["edge"]
    assert [len(s) for _, s in pairs] == [10, 1, 4] and tv == 5
    g10, g1, g4 = (gpu_view(fusion, views, rv, sv, method, tv) for rv, sv in pairs)
    assert g10["geo"].any() and not g10["geo"].all() and np.array_equal(g10["geo"], ref["edge_%s_geo" % method][0])
    assert not g1["geo"].any() and not g1["final"].any() and not g1["xyz"].any()
    assert g1["photo"].any() and same(g1["depth_avg"], ref["edge_%s_depth_avg" % method][1].astype(np.float32))
    if method == "pcd":  # thres_view 5 > nsrc 4: an empty geometric mask, the average unaffected
        assert not g4["geo"].any() and not g4["final"].any()
        assert same(g4["depth_avg"], ref["edge_pcd_depth_avg"][2].astype(np.float32))
        over = gpu_view(fusion, views, pairs[0][0], pairs[0][1], "pcd", 11)
        assert not over["geo"].any() and same(over["depth_avg"], g10["depth_avg"])
    for (rv, sv), with_conf in zip(pairs, (g10, g1, g4)):
        got = gpu_view(fusion, views, rv, sv, method, tv, confs=False)
        assert got["photo"].all()
        assert np.array_equal(got["geo"], with_conf["geo"]) and np.array_equal(got["final"], got["geo"])
        assert same(got["depth_avg"], with_conf["depth_avg"])


def test_perturbed_masks_and_depth(fusion, ref, cases):
    views, pairs, tv = cases["pert"]
    rv, sv = pairs[0]
    dref = views[rv]["depth"]
    worst = 0.0
    for j, s in enumerate(sv):
        # static mask of source j: one source, count 1
        got = gpu_view(fusion, views, rv, [s], "pcd", 1)
        mask, rep = ref["pert_cgc_pcd_mask"][j], ref["pert_cgc_pcd_rep"][j]
        assert np.array_equal(got["geo"], mask), ("pcd", j)
        want = ((rep + dref) / (mask.astype(np.int32) + 1)).astype(np.float32)  # pcd.py:167 for one source
        u = ulps(got["depth_avg"], want).max()
        worst = max(worst, u)
        assert u <= 1, ("pcd depth", j, u)
        # dynamic mask i of source j: the source handed in i times reaches count i at level i or not at all
        # (the masks are nested), and never the count i + 1 of the last clause
        for i in range(2, 11):
            got = gpu_view(fusion, views, rv, [s] * i, "dypcd")
            assert np.array_equal(got["geo"], ref["pert_cgc_dypcd_masks"][j, i - 2]), ("dypcd", j, i)
            if i == 10:
                assert np.array_equal(ref["pert_cgc_dypcd_mask"][j], ref["pert_cgc_dypcd_masks"][j, 8])
    assert (ref["pert_cgc_pcd_mask"][:4].mean((1, 2)) > 0.3).all() and ref["pert_cgc_pcd_mask"][4].mean() < 0.05
    for method in METHODS:  # the whole view, five sources
        got = gpu_view(fusion, views, rv, sv, method, tv)
        for kind in ("photo", "geo", "final"):
            assert np.array_equal(got[kind], ref["pert_%s_%s" % (method, kind)][0]), (method, kind)
        u = ulps(got["depth_avg"], ref["pert_%s_depth_avg" % method][0].astype(np.float32)).max()
        worst = max(worst, u)
        assert u <= 1, (method, u)
    print("perturbed case: worst depth difference %.2f float32 ulp" % worst)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("case", ["scene", "edge"])
def test_filter_depth_equals_reference(fusion, ref, cases, case, method, tmp_path):
    """filter_depth over the scene tree: the mask PNGs and the PLY (vertices and colours, in order, bit for bit)."""
    from PIL import Image
    from damvsnet_amd import mvsio
    views, pairs, tv = cases[case]
    root = str(tmp_path)
    FF.write_tree(root, views, pairs)
    ply = os.path.join(root, "scene.ply")
    n = fusion.filter_depth(root, root, root, ply, conf=FF.CONF_THR, dist_base=FF.DIST_BASE,
                            rel_diff_base=FF.REL_DIFF_BASE, method=method, thres_view=tv)
    key = "%s_%s_" % (case, method)
    for i, (rv, _) in enumerate(pairs):
        for kind in ("photo", "geo", "final"):
            png = np.array(Image.open(os.path.join(root, "mask", "%08d_%s.png" % (rv, kind))))
            assert png.dtype == np.uint8 and np.array_equal(png, ref[key + kind][i].astype(np.uint8) * 255), (rv, kind)
    xyz, rgb = mvsio.read_ply(ply)
    assert n == len(xyz) == len(ref[key + "xyz"])
    assert same(xyz, ref[key + "xyz"]) and np.array_equal(rgb, ref[key + "rgb"])


@pytest.mark.parametrize("nviews,seed,thres_view", [(4, 0, 2), (11, 2, 5)])
def test_static_rule_bilinear_path(fusion, nviews, seed, thres_view):
    """Non-integral coordinates: the kernel against the numpy restatement of filter/pcd.py, gate of tests/test_fusion.py
    (masks agree on >= 99.9 % of pixels, depth_avg within rtol 1e-6 where both final masks agree)."""
    depths, K, E, confs, img = plane_scene(nviews, seed=seed)
    srcs = [(depths[i], K[i], E[i]) for i in range(1, nviews)]
    want = pcd_fuse_view(depths[0], K[0], E[0], srcs, confs, FF.CONF_THR, thres_view, img=img)
    r = fusion.fuse_view(cu(depths[0]), K[0], E[0], [(cu(d), k, e) for d, k, e in srcs], [cu(c) for c in confs],
                         FF.CONF_THR, method="pcd", thres_view=thres_view)
    got = {k: v.cpu().numpy() for k, v in r.items()}
    for k in ("photo", "geo", "final"):
        agree = (got[k] == want[k]).mean()
        assert agree >= 0.999, (k, agree)
    assert want["geo"].mean() > 0.3 and (~want["geo"]).mean() > 0.01  # both outcomes exercised
    both = got["final"] & want["final"]
    assert both.any() and np.allclose(got["depth_avg"][both], want["depth_avg"][both], rtol=1e-6)
    ref_xyz = np.zeros_like(got["xyz"])
    ref_xyz[want["final"]] = want["xyz"]
    assert np.abs(got["xyz"][both] - ref_xyz[both]).max() <= 1e-6 * np.abs(ref_xyz).max()
    assert not got["xyz"][~got["final"]].any()
