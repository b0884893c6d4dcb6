"""Depth-fusion scenes written from seeds (no reference code): the input of the f4 fusion fixtures.

tests/golden/make_fusion.py runs the reference's own filter/dypcd.py and filter/pcd.py over these trees (build container
only, with a cv2.remap stand-in that accepts integer coordinates only) and records their outputs in
tests/golden/fusion_ref.npz; tests/test_fusion_static.py and tests/test_gpu_fusion_static.py rebuild the same trees and
run the oracle / the HIP kernels on them, so both sides see byte-identical files.

Integer scene: every remap coordinate is exactly integral, so OpenCV's INTER_LINEAR (coordinates quantised to 1/32
pixel) is an exact pixel lookup and every float64 camera product has at most one non-zero term per sum.
  * H x W = 24 x 40, K = [[64, 0, 16], [0, 64, 8], [0, 0, 1]] (its float32 inverse is exact), rotation = identity,
    camera centres with even integer x and y, z = 0;
  * depth maps: the plane z = 64 with a rectangle at z = 32 in front of it, rendered per camera, and per view three
    5 x 6 patches overwritten with 16 or 128. A pixel at depth z moves by 64 * dC / z pixels between cameras dC apart:
    integers for z in {16, 32, 64, 128} and even dC;
  * confidences k / 64, images lossless PNG bytes under .jpg names (PIL reads by content).
Perturbed scene: one reference view on the exact levels and five sources whose rendered depths are scaled by 1 + eps,
eps = 1/2048, 1/512, 1/256, 1/160, 1/64: step 1 of the reprojection (reference depth -> source pixel) stays integral,
the relative depth difference is ~eps, which switches the dynamic masks on at i = 2, 3, 6, 9 and never, and passes
the static 0.01 test for the first four only.
"""
from __future__ import annotations

import os

import numpy as np

H, W = 24, 40
K = np.array([[64, 0, 16], [0, 64, 8], [0, 0, 1]], dtype=np.float32)
# 11 distinct even-integer centres that keep the near rectangle in frame (views 0-5 form the scene)
CENTRES = [(0, 0), (2, 0), (-2, 0), (0, 2), (4, -2), (-4, 2), (2, 2), (-2, -2), (4, 0), (-4, 0), (2, -2)]
NEAR = (-4.0, 4.0, -2.0, 2.0)  # world x0, x1, y0, y1 of the rectangle at z = 32
CONF_THR = (0.1, 0.15, 0.9)
DIST_BASE, REL_DIFF_BASE = 0.25, 1 / 1300
THRES_VIEW = 3  # the static rule's count for the scene run

# scene run: ref view -> sources (5, 4, 3, 5, 3, 5 of them). Every view needs at least THRES_VIEW sources, or its static
# geometric mask is empty and the generator's "both outcomes in every view under both rules" cannot hold: a pair list
# with a 2-source view (5, 4, 3, 5, 2, 5) at thres_view 4 fails that condition, hence 3 sources for view 4 and count 3.
SCENE_PAIRS = [(0, [1, 2, 3, 4, 5]), (1, [0, 2, 3, 4]), (2, [0, 1, 5]), (3, [0, 1, 2, 4, 5]), (4, [0, 1, 3]),
               (5, [0, 1, 2, 3, 4])]
# edge run: 10 sources, 1 source, and (static rule at EDGE_THRES_VIEW = 5) a view with fewer sources than the count
EDGE_PAIRS = [(0, [1, 2, 3, 4, 5, 6, 7, 8, 9, 10]), (1, [0]), (2, [0, 1, 3, 5])]
EDGE_THRES_VIEW = 5

EPS = (1 / 2048, 1 / 512, 1 / 256, 1 / 160, 1 / 64)
PERT_PAIRS = [(0, [1, 2, 3, 4, 5])]
PERT_SWITCH = (2, 3, 6, 9, None)  # first i whose dynamic mask passes


def extrinsic(c):
    E = np.eye(4, dtype=np.float32)
    E[0, 3], E[1, 3] = -c[0], -c[1]
    return E


def render(c):
    """Depth of the plane z = 64 and the rectangle NEAR at z = 32 from the camera at centre c (rotation identity)."""
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    X = (u - K[0, 2]) * 32.0 / K[0, 0] + c[0]
    Y = (v - K[1, 2]) * 32.0 / K[1, 1] + c[1]
    near = (X >= NEAR[0]) & (X <= NEAR[1]) & (Y >= NEAR[2]) & (Y <= NEAR[3])
    return np.where(near, np.float32(32), np.float32(64)).astype(np.float32)


def _confs_img(rng):
    # final-stage confidence around the 0.9 threshold, the two others far above theirs except a few zeros
    c3 = rng.integers(54, 65, size=(H, W)).astype(np.float32) / np.float32(64)
    c2 = rng.integers(0, 65, size=(H, W)).astype(np.float32) / np.float32(64)
    c1 = rng.integers(0, 65, size=(H, W)).astype(np.float32) / np.float32(64)
    c2[c2 < 0.05], c1[c1 < 0.05] = 0, 0
    c2[c2 > 0], c1[c1 > 0] = np.maximum(c2[c2 > 0], np.float32(0.25)), np.maximum(c1[c1 > 0], np.float32(0.25))
    return [c3, c2, c1], rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)


def integer_views(seed=0):
    """11 views: {'depth', 'confs' (final, stage 2, stage 1), 'img' uint8, 'K', 'E'} each."""
    rng = np.random.default_rng(seed)
    views = []
    for c in CENTRES:
        d = render(c)
        for _ in range(3):  # inconsistent patches
            y0, x0 = int(rng.integers(0, H - 5)), int(rng.integers(0, W - 6))
            d[y0:y0 + 5, x0:x0 + 6] = np.float32(16 if rng.integers(0, 2) else 128)
        confs, img = _confs_img(rng)
        views.append({"depth": d, "confs": confs, "img": img, "K": K.copy(), "E": extrinsic(c)})
    return views


def perturbed_views(seed=1):
    """View 0 on exact levels, views 1-5 = rendered depth * (1 + EPS[i])."""
    rng = np.random.default_rng(seed)
    views = []
    for i, c in enumerate(CENTRES[:6]):
        d = render(c)
        if i:
            d = d * np.float32(1 + EPS[i - 1])  # exact: 32 and 64 times (1 + a short binary fraction or 1/160 rounded)
        confs, img = _confs_img(rng)
        views.append({"depth": d.astype(np.float32), "confs": confs, "img": img, "K": K.copy(), "E": extrinsic(c)})
    return views


def _save_pfm(path, a):
    a = np.ascontiguousarray(np.flipud(a), dtype="<f4")
    with open(path, "wb") as f:
        f.write(b"Pf\n%d %d\n-1.000000\n" % (a.shape[1], a.shape[0]))
        f.write(a.tobytes())


def write_tree(root, views, pairs):
    """The tree the reference's filter_depth reads (pair_folder = scan_folder = out_folder = root): pair.txt,
    cams/%08d_cam.txt, images/%08d.jpg, depth_est/%08d.pfm, confidence/%08d{,_stage2,_stage1}.pfm."""
    from PIL import Image
    for d in ("cams", "images", "depth_est", "confidence"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    for v, view in enumerate(views):
        rows = lambda m: [" ".join("%.1f" % x for x in r) for r in m]
        with open(os.path.join(root, "cams", "%08d_cam.txt" % v), "w") as f:
            f.write("\n".join(["extrinsic"] + rows(view["E"]) + ["", "intrinsic"] + rows(view["K"]) + ["", "16.0 1.0"])
                    + "\n")
        Image.fromarray(view["img"]).save(os.path.join(root, "images", "%08d.jpg" % v), format="PNG")
        _save_pfm(os.path.join(root, "depth_est", "%08d.pfm" % v), view["depth"])
        for c, sfx in zip(view["confs"], ("", "_stage2", "_stage1")):
            _save_pfm(os.path.join(root, "confidence", "%08d%s.pfm" % (v, sfx)), c)
    with open(os.path.join(root, "pair.txt"), "w") as f:
        f.write("%d\n" % len(pairs))
        for ref, src in pairs:
            f.write("%d\n%d %s\n" % (ref, len(src), " ".join("%d 1.0" % s for s in src)))


# the three recorded runs: name -> (views, pair list, static-rule count)
def cases():
    iv, pv = integer_views(), perturbed_views()
    return {"scene": (iv, SCENE_PAIRS, THRES_VIEW), "edge": (iv, EDGE_PAIRS, EDGE_THRES_VIEW),
            "pert": (pv, PERT_PAIRS, THRES_VIEW)}
