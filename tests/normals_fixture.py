"""Inputs of the point-normal tests (tests/test_normals.py, tests/test_gpu_normals.py), written from seeds.

Tilted planes: a camera with a general K (focal length f, 1 % aspect, an off-centre principal point), a random rotation
and a translation, looking at the plane m . P = c of the camera frame, m up to 70 degrees away from the optical axis; a
plane is kept only when every pixel's ray meets it well in front of the camera. The depth map is the float32 rounding
of the exact depth, the mask 80 % random. 20 planes per focal length, 60 in all, at 24 x 40.
"""
from __future__ import annotations

import numpy as np

FOCALS = (32.0, 300.0, 2900.0)
PLANES_PER_FOCAL = 20
H, W = 24, 40
TILT_JUMP = 0.5


def tilted_planes(h=H, w=W, seed=0):
    """[{'f', 'K', 'E', 'depth' (h, w) float32, 'final' (h, w) bool, 'normal_cam' (3,) float64 facing the camera,
    'normal_world' (3,) float64}]; the same planes for every (h, w) of one seed only in distribution."""
    rng = np.random.default_rng(seed)
    out = []
    for f in FOCALS:
        made = 0
        while made < PLANES_PER_FOCAL:
            K = np.array([[f, 0, w / 2 - 0.3], [0, f * 1.01, h / 2 + 0.2], [0, 0, 1]], np.float32)
            Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            Q *= np.sign(np.linalg.det(Q))
            E = np.eye(4, dtype=np.float32)
            E[:3, :3] = Q
            E[:3, 3] = rng.normal(size=3) * 100
            th, ph = rng.uniform(0, np.radians(70)), rng.uniform(0, 2 * np.pi)
            m = np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), -np.cos(th)])
            c = -rng.uniform(400, 900)
            final = rng.random((h, w)) < 0.8
            Kinv = np.linalg.inv(K).astype(np.float64)
            y, x = np.mgrid[0:h, 0:w].astype(np.float64)
            rays = np.stack([Kinv[i, 0] * x + Kinv[i, 1] * y + Kinv[i, 2] for i in range(3)], -1)
            rm = rays @ m
            if not (rm < -0.2).all():
                continue  # a ray nearly parallel to the plane, or meeting it behind the camera
            made += 1
            out.append({"f": f, "K": K, "E": E, "depth": (c / rm).astype(np.float32), "final": final, "normal_cam": m,
                        "normal_world": np.linalg.inv(E)[:3, :3].astype(np.float64) @ m})
    return out


def neighbour(a, dy, dx, fill):
    hh, ww = a.shape
    b = np.full_like(a, fill)
    b[max(0, -dy):hh - max(0, dy), max(0, -dx):ww - max(0, dx)] = a[max(0, dy):hh - max(0, -dy), max(0, dx):ww - max(0, -dx)]
    return b


def both_tangents(depth, final, jump):
    """Pixels of `final` that have a usable neighbour along x and one along y (the rule's words, written again here)."""
    d = depth.astype(np.float64)
    with np.errstate(all="ignore"):
        use = lambda dy, dx: neighbour(final, dy, dx, False) & (np.abs(neighbour(d, dy, dx, np.nan) - d) <= jump * d)
        return final & (use(0, 1) | use(0, -1)) & (use(1, 0) | use(-1, 0))


def angle_to(normals, want):
    """Angle in radians (its sine, exact enough below 1e-2) between unit float32 normals (n, 3) and the unit vector want."""
    v = normals.astype(np.float64)
    cx = v[:, 1] * want[2] - v[:, 2] * want[1]
    cy = v[:, 2] * want[0] - v[:, 0] * want[2]
    cz = v[:, 0] * want[1] - v[:, 1] * want[0]
    return np.sqrt(cx * cx + cy * cy + cz * cz)
