"""Scenes for the consensus fusion tests (fusion.consensus_statement, k_consensus.hip), written from seeds.

Every scene is a dict: 'depth', 'conf', 'rgb', 'cams' (lists indexed by view id: (H, W) float32, (H, W) float32,
(H, W, 3) uint8, (K, E) float32) and 'pairs', a pair list [(ref, [sources])].
  integer_scene   views 0-5 of tests/fusion_fixture.py's integer scene (24 x 40 = 960 pixels: three blocks of 256 and a
                  tail) with its final-stage confidence, which lies around 0.9: the tests run it at prob_threshold 0.9.
  tiny_case       4 x 4, two views, K = diag(4, 4, 1), the second camera one unit along x: the hand-computed case.
  rotated_scene   24 x 40, six rotated cameras (one of them looking away) over a tilted plane, depths off the plane by up
                  to 1.5 %: the rounding of the source pixel, the frame test, the sign of q[2] and the disparity test all
                  go both ways.
  many_sources    64 views of 4 x 8, so that a view has 63 sources.
  holes_scene     integer_scene with NaN, zero, infinite and negative depths and NaN confidences in views 1 and 2.
"""
from __future__ import annotations

import numpy as np

import fusion_fixture as FF

INTEGER_THR = 0.9


def _scene(views, pairs):
    return {"depth": [v["depth"] for v in views], "conf": [v["confs"][0] for v in views],
            "rgb": [v["img"] for v in views], "cams": [(v["K"], v["E"]) for v in views], "pairs": pairs}


def integer_scene():
    return _scene(FF.integer_views()[:6], [(r, list(s)) for r, s in FF.SCENE_PAIRS])


def holes_scene():
    s = integer_scene()
    rng = np.random.default_rng(11)
    for v, bad in ((1, (np.nan, 0.0)), (2, (np.inf, -32.0))):
        d, c = s["depth"][v].copy(), s["conf"][v].copy()
        u = rng.random(d.shape)
        d[u < 0.15] = bad[0]
        d[(u >= 0.15) & (u < 0.3)] = bad[1]
        c[(u >= 0.3) & (u < 0.4)] = np.nan
        s["depth"][v], s["conf"][v] = d, c
    return s


TINY_K = np.array([[4, 0, 0], [0, 4, 0], [0, 0, 1]], np.float32)


def tiny_case():
    E0, E1 = np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
    E1[0, 3] = -1  # centre (1, 0, 0)
    d0, d1 = np.full((4, 4), 4, np.float32), np.full((4, 4), 4, np.float32)
    c0, c1 = np.ones((4, 4), np.float32), np.ones((4, 4), np.float32)
    d1[1, 1], d1[2, 2] = 4.5, 5
    c0[3, 3], c1[3, 1] = 0.05, 0.0
    r0, r1 = np.full((4, 4, 3), 10, np.uint8), np.full((4, 4, 3), 11, np.uint8)
    r0[1, 2], r1[1, 1] = (10, 255, 1), (12, 255, 0)
    return {"depth": [d0, d1], "conf": [c0, c1], "rgb": [r0, r1], "cams": [(TINY_K, E0), (TINY_K, E1)],
            "pairs": [(0, [1]), (1, [0])]}


def _rot(yaw, pitch):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    return np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])


def rotated_scene(seed=5):
    H, W = 24, 40
    rng = np.random.default_rng(seed)
    K = np.array([[300.0, 0, 19.7], [0, 303.0, 12.2], [0, 0, 1]], np.float32)
    normal, offset = np.array([0.15, -0.1, 1.0]), 600.0  # the plane normal . X = offset
    depth, conf, rgb, cams = [], [], [], []
    for i in range(6):
        centre = np.array([20.0 * i - 50.0, 4.0 * i - 10.0, 3.0 * i])
        aim = np.arctan2(-centre[0], 600.0)  # towards the point of the plane in front of the origin
        R = _rot(aim + rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02)) if i != 4 else _rot(np.pi, 0.0)
        E = np.eye(4)
        E[:3, :3], E[:3, 3] = R.T, -R.T @ centre
        E = E.astype(np.float32)
        Kinv = np.linalg.inv(K.astype(np.float64))
        y, x = np.mgrid[0:H, 0:W].astype(np.float64)
        ray = np.stack([Kinv[j, 0] * x + Kinv[j, 1] * y + Kinv[j, 2] for j in range(3)], -1) @ R.T  # world directions
        with np.errstate(all="ignore"):
            d = (offset - normal @ centre) / (ray @ normal)
        d = np.where(np.isfinite(d) & (d > 0), d, 550.0) * (1 + rng.uniform(-0.015, 0.015, size=(H, W)))
        depth.append(d.astype(np.float32))
        conf.append(rng.uniform(0.0, 1.0, size=(H, W)).astype(np.float32))
        rgb.append(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8))
        cams.append((K.copy(), E))
    pairs = [(0, [1, 2, 3]), (1, [0, 2, 4]), (2, [1, 3, 5, 0]), (3, [2, 4, 5]), (4, [3, 5]), (5, [4, 3, 2, 1])]
    return {"depth": depth, "conf": conf, "rgb": rgb, "cams": cams, "pairs": pairs}


def many_sources(seed=6):
    H, W, V = 4, 8, 64
    rng = np.random.default_rng(seed)
    depth, conf, rgb, cams = [], [], [], []
    for v in range(V):
        E = np.eye(4, dtype=np.float32)
        E[0, 3] = -0.125 * v  # disparities in eighths of a pixel at depth 4
        d = np.full((H, W), 4, np.float32)
        d[rng.random((H, W)) < 0.2] = 4.25
        c = np.ones((H, W), np.float32)
        c[rng.random((H, W)) < 0.1] = 0
        depth.append(d)
        conf.append(c)
        rgb.append(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8))
        cams.append((TINY_K.copy(), E))
    return {"depth": depth, "conf": conf, "rgb": rgb, "cams": cams, "pairs": [(0, list(range(1, V))), (8, [0, 1, 2])]}
