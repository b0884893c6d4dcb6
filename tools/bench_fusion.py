"""Depth-fusion throughput: reference views fused per second at DTU's final
resolution (1184 x 1600 depth maps, 10 source views as in DTU's pair.txt), GPU kernel
(damvs_fusion_view, HIP events on its stream) vs the oracle's numpy restatement of filter/dypcd.py on
the host (one reference view, single process as the reference's per-scene worker).

  python tools/bench_fusion.py [--H 1184 --W 1600 --nsrc 10 --iters 20 --no-cpu --method dypcd|pcd --repeats 1]

--method pcd times the static rule (damvs_fusion_view_static, filter/pcd.py) on the same maps; the CPU baseline is the
dynamic rule's restatement and is skipped for it. --repeats N times N back-to-back groups of --iters calls and reports
each (ms_per_view_repeats) with their spread; the headline is their median. --kernel-ab compares the two kernels
themselves (see kernel_ab).

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
    args = ap.parse_args()
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
