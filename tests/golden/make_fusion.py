"""Depth-fusion fixtures from the reference's own filters (build container only).

Run from the repo root:  ``PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_fusion.py``  -> tests/golden/fusion_ref.npz

filter/dypcd.py and filter/pcd.py are numpy / PIL plus one cv2.remap, a plyfile writer and a yacs config, none of
which is installed here. Stand-ins are put in sys.modules before the import (as make_f3.py does), so the reference's
own reproject_with_depth / check_geometric_consistency / filter_depth run:
  * cv2.remap: X = rint(float32(mapx) * 32), Y likewise; raises unless every X and Y is a multiple of 32, otherwise
    returns the exact pixel lookup with a zero border: what OpenCV's INTER_LINEAR returns for such maps (its
    coordinates are quantised to 1/32 pixel, the weights of an integral coordinate are 1, 0, 0, 0);
  * plyfile: PlyData(...).write captures the vertex array it is handed;
  * yacs: an attribute bag.
The scenes of tests/fusion_fixture.py keep every remap coordinate integral. filter_depth's averaged depth is a local
of its per-view loop: it is read from the frame that calls the module's save_mask for the final mask, so the value
recorded is the one the reference computed, not a restatement. Only recorded outputs are stored.

Recorded per case (scene, edge, pert) and module (dypcd, pcd): photo / geo / final masks read back from the PNGs
filter_depth wrote, depth_est_averaged (float64), the captured PLY vertices and colours; for the pert case and the
scene's first view the masks / mask / depth_reprojected of each module's check_geometric_consistency per source.
The generator asserts the coverage the tests rely on (both mask outcomes in every scene view under both rules, the
rules differing, final non-empty, the perturbed masks switching on where expected) and fails otherwise. The file is
written with fixed zip timestamps: regenerating it gives the same bytes.
"""
from __future__ import annotations

import argparse
import io
import os
import sys
import tempfile
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
import fusion_fixture as FF  # noqa: E402

REF = "/root/reference"
CAPTURED_PLY = []


def stub_modules():
    cv2 = types.ModuleType("cv2")

    def remap(src, mapx, mapy, interpolation=None, **k):
        X = np.rint(np.asarray(mapx, np.float32) * np.float32(32))
        Y = np.rint(np.asarray(mapy, np.float32) * np.float32(32))
        if not (np.isfinite(X).all() and np.isfinite(Y).all() and (np.mod(X, 32) == 0).all()
                and (np.mod(Y, 32) == 0).all()):
            raise RuntimeError("stub cv2.remap: only integral coordinates are exact without OpenCV")
        xi, yi = (X / 32).astype(np.int64), (Y / 32).astype(np.int64)
        h, w = src.shape
        ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
        return np.where(ok, src[np.clip(yi, 0, h - 1), np.clip(xi, 0, w - 1)], src.dtype.type(0)).astype(src.dtype)

    cv2.remap = remap
    cv2.INTER_LINEAR, cv2.INTER_NEAREST = 1, 0
    ply = types.ModuleType("plyfile")

    class PlyElement:
        def __init__(self, data, name):
            self.data, self.name = data, name

        @staticmethod
        def describe(data, name):
            return PlyElement(data, name)

    class PlyData:
        def __init__(self, elements):
            self.elements = elements

        def write(self, filename):
            CAPTURED_PLY.append(np.array(self.elements[0].data))

    ply.PlyData, ply.PlyElement = PlyData, PlyElement
    yacs = types.ModuleType("yacs")
    yc = types.ModuleType("yacs.config")
    yc.CfgNode = type("CfgNode", (), {})
    yacs.config = yc
    for name, m in (("cv2", cv2), ("plyfile", ply), ("yacs", yacs), ("yacs.config", yc)):
        sys.modules.setdefault(name, m)
    sys.path.insert(0, REF)


def run_filter(mod, args, root, nviews):
    """The module's filter_depth over the tree at root -> masks (from its PNGs), its averaged depths, its PLY."""
    from PIL import Image
    davg = []
    orig = mod.save_mask

    def save_mask(filename, mask):
        if filename.endswith("_final.png"):
            davg.append(np.array(sys._getframe(1).f_locals["depth_est_averaged"], dtype=np.float64))
        return orig(filename, mask)

    mod.save_mask = save_mask
    del CAPTURED_PLY[:]
    try:
        with np.errstate(all="ignore"):
            mod.filter_depth(args, root, root, root, os.path.join(root, "out.ply"))
    finally:
        mod.save_mask = orig
    assert len(CAPTURED_PLY) == 1 and len(davg) == nviews
    v = CAPTURED_PLY[0]
    out = {"depth_avg": np.stack(davg), "xyz": np.stack([v["x"], v["y"], v["z"]], 1).astype(np.float32),
           "rgb": np.stack([v["red"], v["green"], v["blue"]], 1).astype(np.uint8)}
    assert v["x"].dtype == np.float32
    return out, lambda ref, kind: np.array(Image.open(os.path.join(root, "mask", "%08d_%s.png" % (ref, kind)))) > 0


def write_npz(path, arrays):
    """np.load-compatible archive with fixed member timestamps (np.savez stamps the current time)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), version=(1, 0), allow_pickle=False)
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "fusion_ref.npz"))
    a = ap.parse_args()
    stub_modules()
    import filter.dypcd as dy
    import filter.pcd as pc
    out = {}
    share = lambda m: float(np.mean(m))
    for case, (views, pairs, tv) in FF.cases().items():
        args = argparse.Namespace(ndepths=[48, 32, 8], conf=list(FF.CONF_THR), dist_base=FF.DIST_BASE,
                                  rel_diff_base=FF.REL_DIFF_BASE, thres_view=tv, display=False)
        res = {}
        for name, mod in (("dypcd", dy), ("pcd", pc)):
            with tempfile.TemporaryDirectory() as tmp:
                FF.write_tree(tmp, views, pairs)
                r, png = run_filter(mod, args, tmp, len(pairs))
                for kind in ("photo", "geo", "final"):
                    r[kind] = np.stack([png(ref, kind) for ref, _ in pairs])
            res[name] = r
            for k, v in r.items():
                out["%s_%s_%s" % (case, name, k)] = v
            assert r["final"].sum() == len(r["xyz"]) == len(r["rgb"])
        out["%s_thres_view" % case] = np.int64(tv)
        if case == "scene":
            for name in ("dypcd", "pcd"):
                for i in range(len(pairs)):
                    g = share(res[name]["geo"][i])
                    assert 0.05 <= g <= 0.95, (name, i, g)
                    assert res[name]["final"][i].any(), (name, i)
                assert len(res[name]["xyz"]) >= 100, (name, len(res[name]["xyz"]))
                print(case, name, "geo share per view", [round(share(g), 3) for g in res[name]["geo"]], "points",
                      len(res[name]["xyz"]))
            d = share(res["dypcd"]["geo"] != res["pcd"]["geo"])
            print("static vs dynamic geo masks differ on %.3f of the scene's pixels" % d)
            assert d >= 0.05, d
        if case == "edge":
            assert not res["dypcd"]["geo"][1].any() and not res["pcd"]["geo"][1].any()  # nsrc = 1
            assert res["dypcd"]["geo"][0].any() and res["pcd"]["geo"][0].any()          # nsrc = 10
            assert not res["pcd"]["geo"][2].any() and res["dypcd"]["geo"][2].any()      # thres_view 5 > nsrc 4
        # per-source outputs of check_geometric_consistency, first reference view
        if case in ("scene", "pert"):
            ref, srcs = pairs[0]
            V = views
            m9, m10, rep, ms, reps = [], [], [], [], []
            with np.errstate(all="ignore"):
                for s in srcs:
                    masks, mask, drep, _, _ = dy.check_geometric_consistency(
                        args, V[ref]["depth"].copy(), V[ref]["K"], V[ref]["E"], V[s]["depth"].copy(), V[s]["K"], V[s]["E"])
                    m9.append(np.stack(masks)), m10.append(mask), rep.append(drep)
                    mask, drep, _, _ = pc.check_geometric_consistency(
                        V[ref]["depth"].copy(), V[ref]["K"], V[ref]["E"], V[s]["depth"].copy(), V[s]["K"], V[s]["E"])
                    ms.append(mask), reps.append(drep)
            out["%s_cgc_dypcd_masks" % case], out["%s_cgc_dypcd_mask" % case] = np.stack(m9), np.stack(m10)
            out["%s_cgc_dypcd_rep" % case] = np.stack(rep)
            out["%s_cgc_pcd_mask" % case], out["%s_cgc_pcd_rep" % case] = np.stack(ms), np.stack(reps)
            assert out["%s_cgc_dypcd_rep" % case].dtype == np.float32
        if case == "pert":
            # the dynamic masks switch on at the expected i on the pixels every source sees consistently, the static
            # mask passes the first four sources; every relative difference is far from every threshold
            m9 = out["pert_cgc_dypcd_masks"]
            core = m9[:4, -1].all(0) & out["pert_cgc_pcd_mask"][:4].all(0)
            assert share(core) > 0.3, share(core)
            for s, first in enumerate(FF.PERT_SWITCH):
                on = [i for i in range(2, 11) if m9[s, i - 2][core].all()]
                anyon = [i for i in range(2, 11) if m9[s, i - 2][core].any()]
                assert (on[0] if on else None) == first and (anyon[0] if anyon else None) == first, (s, on, anyon)
                assert out["pert_cgc_pcd_mask"][s][core].all() == (s < 4)
                assert out["pert_cgc_pcd_mask"][s][core].any() == (s < 4)
            V = views
            d0 = V[0]["depth"]
            thr = np.array([i * FF.REL_DIFF_BASE for i in range(2, 11)] + [0.01])
            with np.errstate(all="ignore"):
                for s in range(1, 6):
                    drep = pc.reproject_with_depth(d0, V[0]["K"], V[0]["E"], V[s]["depth"], V[s]["K"], V[s]["E"])[0]
                    rel = (np.abs(drep - d0) / d0).astype(np.float64).ravel()
                    rel = rel[np.isfinite(rel)]
                    gap = np.abs(rel[:, None] - thr[None]) / thr[None]
                    assert gap.min() > 0.01, (s, gap.min())  # 1 %: ~1e5 float32 ulps
    write_npz(a.out, out)
    print("wrote", a.out, "%.1f KB" % (os.path.getsize(a.out) / 1024), len(out), "arrays")


if __name__ == "__main__":
    main()
