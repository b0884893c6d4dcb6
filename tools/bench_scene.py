"""Scene reconstruction, scene directory to PLY: the file path against the in-memory path (damvsnet_amd/scene.py).

  python tools/bench_scene.py [--views 11 --H 1184 --W 1600 --nviews 5 --batch 4 --repeats 5 --out F]

One process, one bf16 model with synthetic weights (bench.py's build_model), one scene written by the tool: --views
views at H x W with lossless images (PNG data under .jpg names) of uniform noise, DTU-like cameras (synth.cameras) and a
pair.txt in which every view lists all the others. Wall clock from the loaded model to the PLY on disk, for
  (a) files   EvalScenes -> forward -> mvsio.save_stage_outputs, write_cam and the image per view ->
              fusion.fuse_scene(save_masks=False): the reference's directory contract (test_uni.py:229-287, then the
              filter), with the fusion already on the device;
  (b) memory  scene.reconstruct_scene.
One warm-up of each, then --repeats runs of each, interleaved; the median and the spread of each and the ratio (b) / (a)
of the medians. The two PLYs are asserted byte-identical (the images are lossless). With synthetic weights the depth
maps are noise and the cloud is small or empty: the tool measures the plumbing around the forward, which is the same
work for any weights, and not the fusion kernels (tools/bench_fusion.py does).

Then the ingest launch alone (damvs_scene_ingest at B = 4 into a store of --views slots): 20 back-to-back calls per
block between two HIP events, median of 5 blocks, with the bytes it moves (reads: depth, three confidences at full,
half and quarter size and three image planes; writes: depth, three confidences, 3 colour bytes per pixel) and GB/s.
One JSON line, appended to --out when given.
"""
import argparse
import ctypes
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def write_scene(root, scan, H, W, views, seed=0):
    from PIL import Image
    from damvsnet_amd import mvsio, synth
    proj, _, dv = synth.cameras(1, views, H, W)
    cams = proj["stage3"][0].copy()  # the files hold the full-resolution K
    cams[:, 1, 3, 0], cams[:, 1, 3, 1] = dv[0, 0], dv[0, 1] - dv[0, 0]
    d = os.path.join(root, scan)
    for sub in ("cams", "images"):
        os.makedirs(os.path.join(d, sub), exist_ok=True)
    rng = np.random.default_rng(seed)
    for v in range(views):
        cam = os.path.join(d, "cams", "%08d_cam.txt" % v)
        mvsio.write_cam(cam, cams[v])
        lines = open(cam).read().rstrip().split("\n")
        open(cam, "w").write("\n".join(lines[:-1] + ["%s %s" % (cams[v, 1, 3, 0], cams[v, 1, 3, 1])]) + "\n")
        img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        Image.fromarray(img).save(os.path.join(d, "images", "%08d.jpg" % v), format="PNG", compress_level=1)
    with open(os.path.join(d, "pair.txt"), "w") as f:
        f.write("%d\n" % views)
        for v in range(views):
            src = sorted((s for s in range(views) if s != v), key=lambda s: (abs(s - v), s))
            f.write("%d\n%d %s\n" % (v, len(src), " ".join("%d 1.0" % s for s in src)))


def file_path(net, data, scan, out_dir, ply, a):
    """(a): the reference's directory contract between the forward and the fusion."""
    from PIL import Image
    from damvsnet_amd import fusion, mvsio
    ds = mvsio.EvalScenes(data, [scan], a.nviews, max_h=a.H, max_w=a.W)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    with torch.no_grad():
        for i0 in range(0, len(ds), a.batch):
            items = [ds[i] for i in range(i0, min(i0 + a.batch, len(ds)))]
            imgs = np.stack([it["imgs"] for it in items])
            proj = {k: np.stack([it["proj_matrices"][k] for it in items]) for k in items[0]["proj_matrices"]}
            ins = {k: up(np.stack([it["intrinsics_matrices"][k] for it in items]))
                   for k in items[0]["intrinsics_matrices"]}
            out = net(up(imgs), {k: up(v) for k, v in proj.items()}, up(np.stack([it["depth_values"] for it in items])),
                      ins, check_range=False)
            for b, it in enumerate(items):
                mvsio.save_stage_outputs(out_dir, it["filename"], out, b)
                for kind in ("cams", "images"):
                    os.makedirs(os.path.dirname(os.path.join(out_dir, it["filename"].format(kind, ""))), exist_ok=True)
                mvsio.write_cam(os.path.join(out_dir, it["filename"].format("cams", "_cam.txt")), proj["stage3"][b, 0])
                img = np.clip(np.transpose(imgs[b, 0], (1, 2, 0)) * 255, 0, 255).astype(np.uint8)
                Image.fromarray(img).save(os.path.join(out_dir, it["filename"].format("images", ".jpg")), format="PNG",
                                          compress_level=1)
    net.DepthNet.check_range()
    scan_out = os.path.join(out_dir, scan)
    return fusion.fuse_scene(os.path.join(data, scan), scan_out, scan_out, ply, save_masks=False)


def memory_path(net, data, scan, ply, a):
    from damvsnet_amd import scene
    return scene.reconstruct_scene(net, data, scan, ply, nviews=a.nviews, max_h=a.H, max_w=a.W, batch=a.batch)


def ingest_bench(a, calls=20, blocks=5):
    from damvsnet_amd import _capi
    lib = _capi.load_library()
    B, H, W, V = 4, a.H, a.W, a.views
    g = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.rand(*s, device="cuda", generator=g)
    depth, c3, c2, c1 = r(B, H, W), r(B, H, W), r(B, H // 2, W // 2), r(B, H // 4, W // 4)
    imgs = r(B, a.nviews, 3, H, W)
    ds, cs = torch.empty(V, H, W, device="cuda"), torch.empty(V, 3, H, W, device="cuda")
    rs = torch.empty(V, H, W, 3, device="cuda", dtype=torch.uint8)
    slots = (ctypes.c_int * B)(*[(3 * b + 1) % V for b in range(B)])
    call = lambda: _capi.check(lib.damvs_scene_ingest(
        _capi.stream_ptr(), B, H, W, V, depth.data_ptr(), c3.data_ptr(), c2.data_ptr(), c1.data_ptr(), imgs.data_ptr(),
        imgs.stride(0), slots, ds.data_ptr(), cs.data_ptr(), rs.data_ptr()))
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    px = B * H * W
    nbytes = px * 4 * (1 + 1 + 0.25 + 0.0625 + 3) + px * (4 + 12 + 3)
    med = float(np.median(ms))
    return {"B": B, "calls_per_block": calls, "ms_per_call_blocks": [round(m, 4) for m in ms],
            "ms_per_call": round(med, 4), "bytes_per_call": int(nbytes), "GBps": round(nbytes / med / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=11)
    ap.add_argument("--H", type=int, default=1184)
    ap.add_argument("--W", type=int, default=1600)
    ap.add_argument("--nviews", type=int, default=5, help="views per forward (reference + sources)")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tmp", default=None, help="where the scene and the outputs are written (default: a temp folder)")
    ap.add_argument("--out")
    a = ap.parse_args()
    from bench import build_model
    from damvsnet_amd import build
    build.build()
    net, _ = build_model((48, 32, 8), torch.bfloat16, torch.device("cuda"))
    root = tempfile.mkdtemp(prefix="bench_scene_", dir=a.tmp)
    try:
        data, scan = os.path.join(root, "data"), "scan1"
        write_scene(data, scan, a.H, a.W, a.views)
        print("scene written: %d views at %d x %d" % (a.views, a.H, a.W), flush=True)
        times, counts = {"files": [], "memory": []}, {}
        for rep in range(a.repeats + 1):  # run 0 is the warm-up of each
            for name in (("files", "memory") if rep % 2 == 0 else ("memory", "files")):
                out_dir, ply = os.path.join(root, "out_" + name), os.path.join(root, name + ".ply")
                shutil.rmtree(out_dir, ignore_errors=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = file_path(net, data, scan, out_dir, ply, a) if name == "files" else memory_path(net, data, scan, ply, a)
                dt = time.perf_counter() - t0
                counts[name] = n
                if rep:
                    times[name].append(round(dt, 3))
                print("run %d %-6s %.3f s, %d points%s" % (rep, name, dt, n, "" if rep else " (warm-up)"), flush=True)
            same = open(os.path.join(root, "files.ply"), "rb").read() == open(os.path.join(root, "memory.ply"), "rb").read()
            assert same and counts["files"] == counts["memory"], "the two paths wrote different clouds"
        med = {k: float(np.median(v)) for k, v in times.items()}
        res = {"metric": "seconds, loaded model to PLY on disk", "views": a.views, "shape": [a.H, a.W],
               "nviews": a.nviews, "batch": a.batch, "dtype": "bf16", "ndepths": [48, 32, 8], "points": counts["memory"],
               "ply_identical": True, "files_s": times["files"], "memory_s": times["memory"],
               "files_median_s": round(med["files"], 3), "memory_median_s": round(med["memory"], 3),
               "files_spread_s": [min(times["files"]), max(times["files"])],
               "memory_spread_s": [min(times["memory"]), max(times["memory"])],
               "ratio_memory_over_files": round(med["memory"] / med["files"], 4), "ingest": ingest_bench(a)}
    finally:
        shutil.rmtree(root, ignore_errors=True)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
