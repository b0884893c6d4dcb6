"""Consensus depth fusion against the dynamic pair filter on one synthetic scene (fusion.fuse_consensus_resident,
k_consensus.hip; fusion.fuse_resident(method="dypcd")).

  python tools/bench_consensus.py [--views 49 --H 1184 --W 1600 --nsrc 10 --repeats 3 --out F]

The scene: --views views of tests/test_fusion.plane_scene (a tilted plane under synth.cameras, with inconsistent patches
and 2e-4 depth noise) with uniform random confidences and colours, resident on the device. The pair list gives every
view its --nsrc nearest views by index (DTU's pair.txt lists 10). Per driver, after one warm-up run, --repeats runs
interleaved:
  consensus, sources="all"    every other view is a source (views - 1 per launch);
  consensus, sources="pairs"  the pair list's sources;
  dypcd                       fuse_resident(method="dypcd") over the same pair list, the three confidence maps all set
                              to the final-stage map and the three thresholds to 0.1, so that both rules judge the
                              confidence alike.
Wall clock is from the call to the PLY on disk (table upload, launches, one device-to-host copy, the file). Device
time is two HIP events around the views' fusion launches alone, enqueued back to back on an existing table or camera
pack (consensus: `used` cleared before the first event), divided by the number of views. The consensus launches are
far from equal: the first view finds nothing consumed and merges most of what it sees, the later ones skip what was
consumed, so the first launch is also timed alone (`device_ms_first_view`). One JSON line per driver.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--H", type=int, default=1184)
    ap.add_argument("--W", type=int, default=1600)
    ap.add_argument("--nsrc", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from test_fusion import plane_scene
    from damvsnet_amd import fusion
    V, H, W = args.views, args.H, args.W
    t0 = time.perf_counter()
    depths_h, K, E, _, _ = plane_scene(V, H=H, W=W)
    gen = torch.Generator(device="cuda").manual_seed(0)
    cams = {v: (K[v], E[v]) for v in range(V)}
    depths = {v: torch.from_numpy(depths_h[v]).cuda() for v in range(V)}
    confs = {v: torch.rand(H, W, device="cuda", generator=gen) for v in range(V)}
    rgbs = {v: torch.randint(0, 256, (H, W, 3), device="cuda", dtype=torch.uint8, generator=gen) for v in range(V)}
    confs3 = {v: (confs[v],) * 3 for v in range(V)}
    near = lambda v: sorted(range(V), key=lambda s: (abs(s - v), s))[1:args.nsrc + 1]
    pairs = [(v, near(v)) for v in range(V)]
    print("scene of %d views at %d x %d ready in %.1f s" % (V, H, W, time.perf_counter() - t0), flush=True)

    with tempfile.TemporaryDirectory() as root:
        ply = os.path.join(root, "cloud.ply")
        run = {"consensus_all": lambda: fusion.fuse_consensus_resident(pairs, cams, depths, confs, rgbs, ply,
                                                                       sources="all"),
               "consensus_pairs": lambda: fusion.fuse_consensus_resident(pairs, cams, depths, confs, rgbs, ply,
                                                                         sources="pairs"),
               "dypcd": lambda: fusion.fuse_resident(pairs, cams, depths, confs3, rgbs, ply, conf=(0.1, 0.1, 0.1),
                                                     method="dypcd")}
        wall, points = {k: [] for k in run}, {}
        for r in range(args.repeats + 1):  # run 0 is the warm-up
            for name, f in run.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                points[name] = f()
                torch.cuda.synchronize()
                if r:
                    wall[name].append(time.perf_counter() - t0)

    def events(enqueue, before=None):
        reps = []
        for _ in range(args.repeats + 1):
            if before:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            enqueue()
            e1.record()
            torch.cuda.synchronize()
            reps.append(e0.elapsed_time(e1) / V)
        return reps[1:]

    device, first = {}, {}
    table = fusion.ConsensusTable(list(range(V)), cams, depths, confs, rgbs)
    out = None
    for name, sources in (("consensus_all", "all"), ("consensus_pairs", "pairs")):
        order = fusion.consensus_order(pairs, sources)
        out = fusion.consensus_view(table, *order[0])

        def enqueue(order=order):
            for ref, srcs in order:
                fusion.consensus_view(table, ref, srcs, out=out)
        device[name] = events(enqueue, before=lambda: table.used.zero_())
        first[name] = [t * V for t in events(lambda order=order: fusion.consensus_view(table, *order[0], out=out),
                                             before=lambda: table.used.zero_())]

    def enqueue_dypcd():
        for ref, srcs in pairs:
            fusion._fuse_view_raw(depths[ref], K[ref], E[ref], [(depths[s], K[s], E[s]) for s in srcs], confs3[ref],
                                  (0.1, 0.1, 0.1), 0.25, 1 / 1300, True, "dypcd", 5, 1.0, 0.01)
    device["dypcd"] = events(enqueue_dypcd)

    for name in run:
        line = {"metric": "scene fusion, resident maps to PLY", "driver": name, "views": V, "shape": [H, W],
                "sources_per_view": V - 1 if name == "consensus_all" else args.nsrc, "points": points[name],
                "wall_s": round(float(np.median(wall[name])), 4), "wall_s_runs": [round(t, 4) for t in wall[name]],
                "wall_ms_per_view": round(float(np.median(wall[name])) / V * 1e3, 3),
                "device_ms_per_view": round(float(np.median(device[name])), 4),
                "device_ms_per_view_runs": [round(t, 4) for t in device[name]]}
        if name in first:
            line["device_ms_first_view"] = round(float(np.median(first[name])), 4)
            line["device_ms_first_view_runs"] = [round(t, 4) for t in first[name]]
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
