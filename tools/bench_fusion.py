"""Depth-fusion throughput: reference views fused per second at DTU's final
resolution (1184 x 1600 depth maps, 10 source views as in DTU's pair.txt), GPU kernel
(damvs_fusion_view, HIP events on its stream) vs the oracle's numpy restatement of filter/dypcd.py on
the host (one reference view, single process as the reference's per-scene worker).

  python tools/bench_fusion.py [--H 1184 --W 1600 --nsrc 10 --iters 20 --no-cpu --method dypcd|pcd --repeats 1]

--method pcd times the static rule (damvs_fusion_view_static, filter/pcd.py) on the same maps; the CPU baseline is the
dynamic rule's restatement and is skipped for it. --repeats N times N back-to-back groups of --iters calls and reports
each (ms_per_view_repeats) with their spread; the headline is their median. --kernel-ab compares the two kernels
themselves (see kernel_ab).

  python tools/bench_fusion.py --scene [--H 1184 --W 1600 --nsrc 10 --repeats 5 --iters 20 --method dypcd|pcd --out F]

--scene times the scene drivers end to end, files in, PLY out, on one synthetic tree of nsrc + 1 views that each list
all the others as sources (see scene_bench): filter_depth (per view through the host) against fuse_scene (resident
maps, GPU-compacted cloud), and the three cloud launches of one view by HIP events. One JSON line each, appended to
--out when given.

Algorithmic bytes per reference view: 4 B x H x W x (1 ref depth + 3 confidences + nsrc source depths
(each read once; the 4-tap lookups hit L2) + 4 depth_avg + 1 mask + 12 xyz).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def kernel_ab(args, depths, K, E, confs):
    """Both rules' C entry points launched back to back with cameras packed once (fuse_view packs them with numpy on
    every call, which takes longer than the kernel), blocks of --iters launches alternated (dynamic first in even
    repeats, static first in odd ones), HIP events around each block -> ms per launch of each block."""
    import ctypes
    from damvsnet_amd import _capi, fusion
    lib = _capi.load_library()
    H, W, n = args.H, args.W, args.nsrc
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d, cf = [cu(x) for x in depths], [cu(c) for c in confs]
    cams = fusion.fusion_cams(K[0], E[0], [(K[i], E[i]) for i in range(1, n + 1)])
    dsrc = (ctypes.c_void_p * n)(*[x.data_ptr() for x in d[1:]])
    cptr = (ctypes.c_void_p * 3)(*[c.data_ptr() for c in cf])
    thr = (ctypes.c_float * 3)(0.1, 0.15, 0.9)
    davg = torch.empty(H, W, device="cuda")
    mask = torch.empty(H, W, device="cuda", dtype=torch.uint8)
    xyz = torch.empty(H, W, 3, device="cuda")
    head = (_capi.stream_ptr(d[0].device), H, W, n, d[0].data_ptr(), dsrc, cptr, thr, ctypes.byref(cams))
    outs = (davg.data_ptr(), mask.data_ptr(), xyz.data_ptr())
    run = {"dypcd": lambda: _capi.check(lib.damvs_fusion_view(*head, 0.25, 1 / 1300, *outs)),
           "pcd": lambda: _capi.check(lib.damvs_fusion_view_static(*head, 1.0, 0.01, args.thres_view, *outs))}
    for f in run.values():
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    res = {"dypcd": [], "pcd": []}
    for r in range(max(1, args.repeats)):
        for name in (("dypcd", "pcd") if r % 2 == 0 else ("pcd", "dypcd")):  # the order swaps with every repeat
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                run[name]()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(round(e0.elapsed_time(e1) / args.iters, 4))
    print(json.dumps({"metric": "ms per launch, C entry points back to back", "shape": [H, W], "nsrc": n,
                      "launches_per_block": args.iters, "ms_per_launch": res}), flush=True)


def write_scene_tree(root, H, W, nviews, seed=0):
    """A filter_depth tree of nviews views of test_fusion.plane_scene, each with all the others as sources: pair.txt,
    cams/, images/ (lossless PNG bytes under .jpg names; PIL reads by content), depth_est/ and confidence/ PFMs."""
    from PIL import Image
    from test_fusion import plane_scene
    from damvsnet_amd import mvsio
    depths, K, E, confs, _ = plane_scene(nviews, H=H, W=W, seed=seed)
    rng = np.random.default_rng(seed + 1)
    for d in ("cams", "images", "depth_est", "confidence"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    for v in range(nviews):
        cam = np.zeros((2, 4, 4), np.float32)
        cam[0], cam[1, :3, :3] = E[v], K[v]
        mvsio.write_cam(os.path.join(root, "cams", "%08d_cam.txt" % v), cam)
        img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        Image.fromarray(img).save(os.path.join(root, "images", "%08d.jpg" % v), format="PNG", compress_level=1)
        mvsio.save_pfm(os.path.join(root, "depth_est", "%08d.pfm" % v), depths[v])
        for c, sfx in zip(confs, ("", "_stage2", "_stage1")):
            mvsio.save_pfm(os.path.join(root, "confidence", "%08d%s.pfm" % (v, sfx)), np.roll(c, 97 * v, axis=1))
    with open(os.path.join(root, "pair.txt"), "w") as f:
        f.write("%d\n" % nviews)
        for v in range(nviews):
            src = [s for s in range(nviews) if s != v]
            f.write("%d\n%d %s\n" % (v, len(src), " ".join("%d 1.0" % s for s in src)))
    return depths, K, E, confs


def scene_bench(args):
    """Wall clock of filter_depth and fuse_scene on one tree (median of --repeats runs after one warm-up each, same
    process, runs interleaved), the PLYs asserted byte-identical; then the cloud launches of one view (count, scan,
    scatter) timed by HIP events over --iters back-to-back calls. The final-stage confidence threshold is 0.5 instead
    of the reference's 0.9 so that the uniform random confidences keep about 4 in 10 pixels of the plane."""
    import tempfile
    from damvsnet_amd import fusion
    H, W, nviews = args.H, args.W, args.nsrc + 1
    conf = (0.1, 0.15, 0.5)
    lines = []
    with tempfile.TemporaryDirectory() as root:
        depths, K, E, confs = write_scene_tree(root, H, W, nviews)
        ply = {"filter_depth": os.path.join(root, "filter_depth.ply"), "fuse_scene": os.path.join(root, "fuse_scene.ply"),
               "fuse_scene_no_masks": os.path.join(root, "fuse_scene_no_masks.ply")}
        kw = dict(conf=conf, method=args.method, thres_view=args.thres_view)
        run = {"filter_depth": lambda: fusion.filter_depth(root, root, root, ply["filter_depth"], **kw),
               "fuse_scene": lambda: fusion.fuse_scene(root, root, root, ply["fuse_scene"], **kw),
               "fuse_scene_no_masks": lambda: fusion.fuse_scene(root, root, root, ply["fuse_scene_no_masks"],
                                                                save_masks=False, **kw)}
        times, count = {k: [] for k in run}, {}
        for r in range(max(5, args.repeats) + 1):  # run 0 is the warm-up
            for name, f in run.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                count[name] = f()
                torch.cuda.synchronize()
                if r:
                    times[name].append(time.perf_counter() - t0)
        blobs = {k: open(p, "rb").read() for k, p in ply.items()}
        assert blobs["filter_depth"] == blobs["fuse_scene"] == blobs["fuse_scene_no_masks"], "the PLY files differ"
        assert len(set(count.values())) == 1
        med = {k: float(np.median(v)) for k, v in times.items()}
        for name in run:
            lines.append({"metric": "scene wall clock, files in, PLY out", "driver": name, "seconds": round(med[name], 4),
                          "runs": [round(t, 4) for t in times[name]], "views": nviews, "sources_per_view": args.nsrc,
                          "shape": [H, W], "method": args.method, "conf": list(conf), "points": count[name],
                          "ply_bytes": len(blobs[name]), "ply_identical_to_filter_depth": True,
                          "speedup_vs_filter_depth": round(med["filter_depth"] / med[name], 3)})
    # the cloud launches of one view, maps resident
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = [cu(x) for x in depths]
    _, mask, xyz = fusion._fuse_view_raw(d[0], K[0], E[0], [(d[i], K[i], E[i]) for i in range(1, nviews)],
                                         [cu(c) for c in confs], conf, 0.25, 1 / 1300, True, args.method,
                                         args.thres_view, 1.0, 0.01)
    rgb = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda")
    n = int(((mask & 4) != 0).sum().item())
    records = torch.empty(n * 15, dtype=torch.uint8, device="cuda")
    cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
    scratch = fusion.compact_cloud(mask, xyz, rgb, records, cursor)
    reps = []
    for _ in range(max(5, args.repeats)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            cursor.zero_()
            fusion.compact_cloud(mask, xyz, rgb, records, cursor, scratch)
        e1.record()
        torch.cuda.synchronize()
        reps.append(e0.elapsed_time(e1) / args.iters)
    ms = float(np.median(reps))
    moved = 2 * H * W + n * (12 + 3) + n * 15 + 3 * 4 * scratch.numel()  # mask twice, kept points in, records out
    lines.append({"metric": "cloud launches per view (count + scan + scatter, incl. the cursor reset), HIP events",
                  "ms_per_view": round(ms, 4), "ms_per_view_repeats": [round(r, 4) for r in reps], "shape": [H, W],
                  "points": n, "kept_fraction": round(n / (H * W), 4), "bytes_moved": moved,
                  "achieved_GBps": round(moved / ms / 1e6, 1)})
    for line in lines:
        print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=1184)
    ap.add_argument("--W", type=int, default=1600)
    ap.add_argument("--nsrc", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--method", default="dypcd", choices=("dypcd", "pcd"))
    ap.add_argument("--thres-view", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--kernel-ab", action="store_true")
    ap.add_argument("--scene", action="store_true")
    ap.add_argument("--out", default=None, help="--scene: append the JSON lines to this file")
    args = ap.parse_args()
    if args.scene:
        return scene_bench(args)
    from test_fusion import plane_scene
    from damvsnet_amd.fusion import fuse_view
    depths, K, E, confs, img = plane_scene(args.nsrc + 1, H=args.H, W=args.W, seed=0)
    if args.kernel_ab:
        return kernel_ab(args, depths, K, E, confs)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    srcs = [(cu(depths[i]), K[i], E[i]) for i in range(1, args.nsrc + 1)]
    ref, cf = cu(depths[0]), [cu(c) for c in confs]
    run = lambda: fuse_view(ref, K[0], E[0], srcs, cf, method=args.method, thres_view=args.thres_view)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    reps = []
    for _ in range(max(1, args.repeats)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            run()
        e1.record()
        torch.cuda.synchronize()
        reps.append(e0.elapsed_time(e1) / args.iters)
    ms = float(np.median(reps))
    px = args.H * args.W
    alg = 4 * px * (1 + 3 + args.nsrc + 1) + px + 12 * px
    out = {"metric": "fused reference views/s", "value": round(1e3 / ms, 2), "ms_per_view": round(ms, 4),
           "shape": [args.H, args.W], "nsrc": args.nsrc, "achieved_GBps": round(alg / ms / 1e6, 1),
           "algorithmic_bytes": alg, "method": args.method}
    if args.repeats > 1:
        out["ms_per_view_repeats"] = [round(r, 4) for r in reps]
        out["spread_ms"] = round(max(reps) - min(reps), 4)
    if not args.no_cpu and args.method == "dypcd":
        from oracle import fusion_oracle as FO
        t0 = time.perf_counter()
        FO.fuse_view(depths[0], K[0], E[0], [(depths[i], K[i], E[i]) for i in range(1, args.nsrc + 1)], confs,
                     (0.1, 0.15, 0.9), img=img)
        cpu = time.perf_counter() - t0
        out["cpu_baseline"] = {"value": round(1.0 / cpu, 4), "unit": "views/s", "cores": 1, "kind": "port",
                               "sample": "1 reference view, numpy restatement of filter/dypcd.py"}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
