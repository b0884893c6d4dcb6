"""Scene reconstruction, scene directory to PLY: the file path against the in-memory path (damvsnet_amd/scene.py).

  python tools/bench_scene.py [--views 11 --H 1184 --W 1600 --H0 H --W0 W --nviews 5 --batch 4 --repeats 5 --out F]

One process, one bf16 model with synthetic weights (bench.py's build_model), one scene written by the tool: --views
views at H x W with lossless images (PNG data under .jpg names) of uniform noise, DTU-like cameras (synth.cameras) and a
pair.txt in which every view lists all the others. Wall clock from the loaded model to the PLY on disk, for
  (a) files   EvalScenes -> forward -> mvsio.save_stage_outputs, write_cam and the image per view ->
              fusion.fuse_scene(save_masks=False): the reference's directory contract (test_uni.py:229-287, then the
              filter), with the fusion already on the device;
  (b) memory  scene.reconstruct_scene;
  (c) device  scene.reconstruct_scene(inputs="device"): the views decoded to uint8 in threads, uploaded once each,
              converted, resized and batched by damvs_scene_inputs.
  (d) cached  scene.reconstruct_scene(inputs="device", features="scene"): as (c), and every view through FeatureNet
              once into a scene.SceneFeatures, each batch's features gathered by damvs_feature_gather.
One warm-up of each, then --repeats runs of each, interleaved; the median and the spread of each and the ratios (b) / (a),
(c) / (b) and (d) / (c) of the medians. The PLYs of (c) and (d) are asserted byte-identical at any size (they share
their images). The PLYs of (a) and (b) are asserted byte-identical (the images are lossless), and (c)'s
too when the scene needs no resize (--H0 x --W0, the size of the image files, equal to the working size, the default);
otherwise the `imgs` of (c)'s and (b)'s first batch are asserted to agree within 2^-21 (tests/test_inputs.py). With synthetic weights the depth
maps are noise and the cloud is small or empty: the tool measures the plumbing around the forward, which is the same
work for any weights, and not the fusion kernels (tools/bench_fusion.py does).

Then the ingest launch alone (damvs_scene_ingest at B = 4 into a store of --views slots): 20 back-to-back calls per
block between two HIP events, median of 5 blocks, with the bytes it moves (reads: depth, three confidences at full,
half and quarter size and three image planes; writes: depth, three confidences, 3 colour bytes per pixel) and GB/s.
Then the inputs launch alone (damvs_scene_inputs, B * N = 20 images of 1200 x 1600 to 1184 x 1568, what
scale_mvs_input gives DTU, from a store of --views slots), timed the same way, and a one-off breakdown of (b)'s wall
clock (`breakdown`): the same steps as reconstruct_scene's host path, one run, with a device synchronisation after
every device step so that each step's time is its own; the sum is therefore a little above an unsynchronised run.
The same for (c) and (d) (`device_breakdown`: decode and upload, the FeatureNet fill pass, the inputs launches, the
gathers, the forwards, the ingests, the fusion), with the cache's size, and the gather launch alone
(damvs_feature_gather, B * N = 20 pairs of the working size's three stage tensors in bf16 from a store of --views
slots), timed as the other launches, with the bytes it moves.
One JSON line, appended to --out when given.

--thin runs the voxel-thinning record instead (fusion's voxel= option, k_thin.hip) and prints its own JSON line:
  * `reconstruct_scene(inputs="device", features="scene")` with voxel=None against --voxels (two edges in world units),
    interleaved after one warm-up of each, with the point counts and PLY bytes (synthetic weights: the cloud is what the
    noise gives);
  * the launches of one reference view of the same scene's cameras, each timed alone (20 back-to-back calls per block
    between two HIP events, median of 5 blocks): the fusion kernel over fronto-parallel depth maps with 10 sources, then,
    on the points it wrote, with the mask forced to every pixel and to a random 30 %, compact_cloud and the claim +
    resolve pair, for an edge of 2 and of 8 pixel footprints (about 4 and 64 pixels per cell and view): view 0 into an
    empty table (every cell inserted) and the later views of the scan (most cells already taken), with the table's bytes
    and the load factor after all views.

--normals runs the oriented-cloud record instead (fusion's normals= option, k_normals.hip) and prints its own JSON line:
`reconstruct_scene(inputs="device", features="scene")` with and without normals=True, interleaved after one warm-up of
each, and per view of 1184 x 1600, with the mask forced to every pixel and to a random 30 %, compact_cloud, its oriented
form and the normal map launch, each timed alone with a record buffer that holds every call's records.
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


def memory_path(net, data, scan, ply, a, inputs="host", features="batch"):
    from damvsnet_amd import scene
    kw = {"features": features} if features != "batch" else {}
    return scene.reconstruct_scene(net, data, scan, ply, nviews=a.nviews, max_h=a.H, max_w=a.W, batch=a.batch,
                                   inputs=inputs, **kw)


def device_breakdown(net, data, scan, ply, a, features):
    """(c)'s (features="batch") or (d)'s ("scene") steps, one run, each timed on its own: what
    reconstruct_scene(inputs="device") does, with a device synchronisation after every device step."""
    from damvsnet_amd import mvsio, scene
    t = {k: 0.0 for k in ("cameras", "decode_upload", "fill", "inputs", "gather", "forward", "ingest", "fuse")}

    def timed(name, fn):
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        t[name] += time.perf_counter() - t0
        return r

    torch.cuda.synchronize()
    start = time.perf_counter()
    ds = mvsio.EvalScenes(data, [scan], a.nviews, max_h=a.H, max_w=a.W, cache_views=True)
    refs = [ref for _, ref, _ in ds.metas]
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    samples = timed("cameras", lambda: [ds.cameras(i) for i in range(len(ds))])
    (H0, W0), (H, W) = samples[0]["original_size"], samples[0]["size"]
    store = scene.SceneInputs(sorted({v for s in samples for v in s["view_ids"]}), H0, W0, H, W, "cuda")
    timed("decode_upload", lambda: [store.put(v, mvsio.read_img_bytes(ds._img_path(scan, v))) for v in store.view_ids])
    feats, maps, reused, nbytes = None, None, None, 0
    with torch.no_grad():
        if features == "scene":
            feats = scene.SceneFeatures(net, store.view_ids, H, W, "cuda")
            nbytes = feats.nbytes
            for i0 in range(0, len(store.view_ids), a.batch * a.nviews):
                group = store.view_ids[i0:i0 + a.batch * a.nviews]
                imgs = timed("inputs", lambda: store.batch([[v] for v in group], out=reused))
                reused = imgs if reused is None else reused
                timed("fill", lambda: feats.put(group, imgs[:, 0]))
            fbufs = feats.buffers(min(a.batch, len(samples)) * a.nviews)
        for i0 in range(0, len(samples), a.batch):
            items = samples[i0:i0 + a.batch]
            lists = [it["view_ids"][:1] if feats is not None else it["view_ids"] for it in items]
            imgs = timed("inputs", lambda: store.batch(lists, out=reused))
            reused = imgs if reused is None else reused
            proj_host = {k: np.stack([it["proj_matrices"][k] for it in items]) for k in items[0]["proj_matrices"]}
            proj = {k: up(v) for k, v in proj_host.items()}
            ins = {k: up(np.stack([it["intrinsics_matrices"][k] for it in items]))
                   for k in items[0]["intrinsics_matrices"]}
            dv = up(np.stack([it["depth_values"] for it in items]))
            if feats is not None:
                f = timed("gather", lambda: feats.batch([it["view_ids"] for it in items], out=fbufs))
                out = timed("forward", lambda: net(imgs, proj, dv, ins, check_range=False, features=f))
            else:
                out = timed("forward", lambda: net(imgs, proj, dv, ins, check_range=False))
            if maps is None:
                maps = scene.SceneMaps(refs, H, W, "cuda")
            timed("ingest", lambda: maps.add(refs[i0:i0 + len(items)], out, imgs=imgs, cams=proj_host["stage3"][:, 0]))
    net.DepthNet.check_range()
    n = timed("fuse", lambda: maps.fuse(os.path.join(data, scan, "pair.txt"), ply))
    total = time.perf_counter() - start
    res = {k: round(v, 4) for k, v in t.items()}
    res.update(total_s=round(total, 4), other_s=round(total - sum(t.values()), 4), points=n,
               forward_share=round(t["forward"] / total, 4), cache_MB=round(nbytes / 1e6, 1))
    return res


def features_bench(a, H, W, calls=20, blocks=5):
    """damvs_feature_gather alone: B * N = 20 pairs of the three stage tensors of an H x W image in bf16."""
    from damvsnet_amd import _capi
    lib = _capi.load_library()
    n, V, es = 20, a.views, 2
    view_bytes = [H // 4 * (W // 4) * 32 * es, H // 2 * (W // 2) * 16 * es, H * W * 8 * es]
    g = torch.Generator(device="cuda").manual_seed(0)
    stores = [torch.randint(0, 256, (V, vb), device="cuda", dtype=torch.uint8, generator=g) for vb in view_bytes]
    outs = [torch.empty(n, vb, device="cuda", dtype=torch.uint8) for vb in view_bytes]
    args = ((ctypes.c_void_p * 3)(*[t.data_ptr() for t in stores]), (ctypes.c_ulonglong * 3)(*view_bytes),
            (ctypes.c_int * n)(*[(3 * i + 1) % V for i in range(n)]), (ctypes.c_void_p * 3)(*[t.data_ptr() for t in outs]))
    call = lambda: _capi.check(lib.damvs_feature_gather(_capi.stream_ptr(), n, 3, V, *args))
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
    moved = n * sum(view_bytes)
    med = float(np.median(ms))
    return {"pairs": n, "shape": [H, W], "dtype": "bf16", "calls_per_block": calls,
            "ms_per_call_blocks": [round(m, 4) for m in ms], "ms_per_call": round(med, 4), "bytes_read": moved,
            "bytes_written": moved, "GBps": round(2 * moved / med / 1e6, 1)}


def breakdown(net, data, scan, ply, a):
    """(b)'s steps, one run, each timed on its own: what reconstruct_scene(inputs="host") does through
    mvsio.EvalScenes(cache_views=True), restated step by step (every view of the scene has one size here, so the
    dataset's second resize never happens). read_img decodes straight into float32; here the decode to uint8 and the
    conversion are separate steps, which costs one more pass over the bytes."""
    from PIL import Image
    from damvsnet_amd import mvsio
    from damvsnet_amd.scene import SceneMaps
    t = {k: 0.0 for k in ("decode", "convert", "resize", "cameras", "stack", "upload", "forward", "ingest", "fuse")}

    def timed(name, fn, sync=False):
        t0 = time.perf_counter()
        r = fn()
        if sync:
            torch.cuda.synchronize()
        t[name] += time.perf_counter() - t0
        return r

    torch.cuda.synchronize()
    start = time.perf_counter()
    ds = mvsio.EvalScenes(data, [scan], a.nviews, max_h=a.H, max_w=a.W)
    refs = [ref for _, ref, _ in ds.metas]
    views, maps, largest = {}, None, 0
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    with torch.no_grad():
        for i0 in range(0, len(ds), a.batch):
            imgs_b, proj_b, dv_b, ins_b = [], [], [], []
            for _, ref, src in ds.metas[i0:i0 + a.batch]:
                ids = [ref] + src[:a.nviews - 1]
                for v in ids:
                    if v not in views:
                        raw = timed("decode", lambda: np.array(Image.open(ds._img_path(scan, v))))
                        img = timed("convert", lambda: raw.astype(np.float32) / 255.0)
                        cam = timed("cameras", lambda: mvsio.read_cam_file(
                            os.path.join(data, scan, "cams", "%08d_cam.txt" % v), ds.ndepths, ds.interval_scale[scan]))
                        img, K = timed("resize", lambda: mvsio.scale_mvs_input(img, cam[0], a.W, a.H))
                        views[v] = (img, K) + cam[1:]
                pm = np.zeros((len(ids), 2, 4, 4), np.float32)
                for n, v in enumerate(ids):
                    pm[n, 0], pm[n, 1, :3, :3] = views[v][2], views[v][1]
                imgs_b.append(timed("stack", lambda: np.stack([views[v][0] for v in ids]).transpose(0, 3, 1, 2)))
                proj_b.append(mvsio.stage_projections(pm))
                _, K, _, dmin, dint = views[ids[-1]][:2] + views[ids[0]][2:]
                dv_b.append(np.arange(dmin, dint * (ds.ndepths - 0.5) + dmin, dint, dtype=np.float32))
                ins_b.append({"stage%d" % (k + 1): np.concatenate([K[:2] * 2.0 ** k, K[2:]]) for k in range(3)})
            stacked = timed("stack", lambda: np.ascontiguousarray(np.stack(imgs_b)))
            imgs = timed("upload", lambda: torch.from_numpy(stacked).cuda(), sync=True)
            largest = max(largest, stacked.nbytes)
            proj_host = {k: np.stack([p[k] for p in proj_b]) for k in proj_b[0]}
            proj = {k: up(v) for k, v in proj_host.items()}
            ins = {k: up(np.stack([i[k] for i in ins_b])) for k in ins_b[0]}
            dv = up(np.stack(dv_b))
            out = timed("forward", lambda: net(imgs, proj, dv, ins, check_range=False), sync=True)
            if maps is None:
                maps = SceneMaps(refs, imgs.shape[3], imgs.shape[4], "cuda")
            timed("ingest", lambda: maps.add(refs[i0:i0 + len(imgs_b)], out, imgs=imgs, cams=proj_host["stage3"][:, 0]),
                  sync=True)
    net.DepthNet.check_range()
    n = timed("fuse", lambda: maps.fuse(os.path.join(data, scan, "pair.txt"), ply), sync=True)
    total = time.perf_counter() - start
    res = {k: round(v, 4) for k, v in t.items()}
    res.update(total_s=round(total, 4), other_s=round(total - sum(t.values()), 4), points=n,
               largest_batch_MB=round(largest / 1e6, 1))
    return res


def inputs_bench(a, calls=20, blocks=5):
    """damvs_scene_inputs alone at DTU's sizes: B * N = 20 images per call."""
    from damvsnet_amd import _capi
    lib = _capi.load_library()
    n, H0, W0, H, W, V = 20, 1200, 1600, 1184, 1568, a.views
    g = torch.Generator(device="cuda").manual_seed(0)
    store = torch.randint(0, 256, (V, H0, W0, 3), device="cuda", dtype=torch.uint8, generator=g)
    out = torch.empty(n, 3, H, W, device="cuda")
    slots = (ctypes.c_int * n)(*[(3 * i + 1) % V for i in range(n)])
    call = lambda: _capi.check(lib.damvs_scene_inputs(_capi.stream_ptr(), n, H0, W0, H, W, V, store.data_ptr(), slots,
                                                      out.data_ptr()))
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
    read, written = n * 3 * H0 * W0, n * 3 * H * W * 4  # every source byte once per image that lists it; the output
    med = float(np.median(ms))
    return {"images": n, "from": [H0, W0], "to": [H, W], "calls_per_block": calls,
            "ms_per_call_blocks": [round(m, 4) for m in ms], "ms_per_call": round(med, 4), "bytes_read": read,
            "bytes_written": written, "GBps": round((read + written) / med / 1e6, 1)}


def first_batch_imgs_diff(data, scan, a):
    """max |imgs of (c) - imgs of (b)| over the first batch, when the scene needs a resize."""
    from damvsnet_amd import mvsio
    from damvsnet_amd.scene import SceneInputs
    ds = mvsio.EvalScenes(data, [scan], a.nviews, max_h=a.H, max_w=a.W, cache_views=True)
    n = min(a.batch, len(ds))
    want = torch.from_numpy(np.stack([ds[i]["imgs"] for i in range(n)]))
    cams = [ds.cameras(i) for i in range(n)]
    ids = sorted({v for c in cams for v in c["view_ids"]})
    si = SceneInputs(ids, *cams[0]["original_size"], *cams[0]["size"], "cuda")
    for v in ids:
        si.put(v, mvsio.read_img_bytes(ds._img_path(scan, v)))
    return float((si.batch([c["view_ids"] for c in cams]).cpu() - want).abs().max())


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


def _event_ms(call, calls=20, blocks=5, before=None):
    """Median over `blocks` of the mean time of `calls` back-to-back calls between two HIP events; `before` runs
    (untimed, synchronised) ahead of every block."""
    ms = []
    for _ in range(blocks + 1):  # block 0 warms up
        if before is not None:
            before()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    return round(float(np.median(ms[1:])), 4)


def thin_launches(a, H, W):
    """The launches of one reference view, each alone: fusion, compact_cloud, claim + resolve (the module docstring)."""
    from damvsnet_amd import fusion, synth
    V = a.views
    proj, _, dv = synth.cameras(1, V, H, W)
    cams = [(proj["stage3"][0, v, 1, :3, :3].copy(), proj["stage3"][0, v, 0].copy()) for v in range(V)]
    depth_mid = float(dv[0, 0] + dv[0, -1]) / 2
    depths = [torch.full((H, W), depth_mid, device="cuda") for _ in range(V)]
    confs = tuple(torch.ones(H, W, device="cuda") for _ in range(3))
    nsrc = min(10, V - 1)
    fuse = lambda v: fusion._fuse_view_raw(depths[v], cams[v][0], cams[v][1],
                                           [(depths[s],) + cams[s] for s in range(V) if s != v][:nsrc], confs,
                                           (0.1, 0.15, 0.9), 0.25, 1 / 1300, True, "dypcd", 5, 1.0, 0.01)
    res = {"shape": [H, W], "sources": nsrc, "fusion_ms": _event_ms(lambda: fuse(0))}
    xyzs = []
    for v in range(V):  # the world points of every pixel of every view, whatever the filter kept
        u, w = torch.meshgrid(torch.arange(W, device="cuda", dtype=torch.float32),
                              torch.arange(H, device="cuda", dtype=torch.float32), indexing="xy")
        K, E = (torch.from_numpy(np.asarray(m, np.float32)).cuda() for m in cams[v])
        cam = torch.linalg.inv(K) @ torch.stack([u, w, torch.ones_like(u)], -1).reshape(-1, 3).T * depth_mid
        world = torch.linalg.inv(E) @ torch.cat([cam, torch.ones_like(cam[:1])])
        xyzs.append(world[:3].T.reshape(H, W, 3).contiguous())
    res["fusion_kept_fraction_view0"] = round(float(((fuse(0)[1] & 4) != 0).float().mean()), 4)
    pixel = depth_mid / float(cams[0][0][0, 0])
    res["pixel_footprint"] = round(pixel, 4)
    rgb = torch.zeros(H, W, 3, device="cuda", dtype=torch.uint8)
    g = torch.Generator(device="cuda").manual_seed(0)
    masks = {"all": [torch.full((H, W), 4, device="cuda", dtype=torch.uint8) for _ in range(V)],
             "30%": [((torch.rand(H, W, device="cuda", generator=g) < 0.3).to(torch.uint8) * 4) for _ in range(V)]}
    records = torch.empty(H * W * fusion.RECORD_BYTES, device="cuda", dtype=torch.uint8)
    cursor = torch.zeros(1, device="cuda", dtype=torch.int64)
    scratch = fusion.compact_cloud(masks["all"][0], xyzs[0], rgb, records, cursor)
    for sel, ms in masks.items():
        row = {"selected_per_view": int((ms[0] != 0).sum()),
               "compact_ms": _event_ms(lambda: fusion.compact_cloud(ms[0], xyzs[0], rgb, records, cursor, scratch),
                                       before=cursor.zero_)}
        for px in (2, 8):
            voxel = px * pixel
            slots = fusion._voxel_slots(None, V * H * W)
            grid = fusion.VoxelGrid(voxel, slots, "cuda")
            keep = torch.empty(H, W, device="cuda", dtype=torch.uint8)
            # view 0 into an empty table: the clear is part of what is timed here (one memset of the table per call)
            first = _event_ms(lambda: (grid.clear(), grid.claim(ms[0], xyzs[0], 0, keep)), calls=5)
            clear = _event_ms(grid.clear, calls=5)
            grid.clear()
            kept = []
            for v in range(V):
                grid.claim(ms[v], xyzs[v], v * H * W, keep)
                kept.append(int((keep != 0).sum()))
            grid.check()
            occupied = grid.occupied()
            # a later view again: its cells are all taken, as most are for the later views of a scan
            later = _event_ms(lambda: grid.claim(ms[V - 1], xyzs[V - 1], (V - 1) * H * W, keep))
            grid.check()
            kept_mask = keep.clone()
            row["voxel_%dpx" % px] = {
                "voxel": round(voxel, 4), "slots": slots, "table_MB": round(grid.nbytes / 1e6, 1),
                "claim_resolve_first_view_ms": round(first - clear, 4), "table_clear_ms": clear,
                "claim_resolve_later_view_ms": later, "kept_per_view": kept, "occupied": occupied,
                "load_factor": round(occupied / slots, 4),
                "compact_kept_ms": _event_ms(lambda: fusion.compact_cloud(kept_mask, xyzs[0], rgb, records, cursor, scratch),
                                             before=cursor.zero_)}
            del grid
        res[sel] = row
    return res


def thin_main(a, net, root, data, scan):
    voxels = [None] + [float(v) for v in a.voxels.split(",")]
    names = ["none"] + ["voxel_%g" % v for v in voxels[1:]]
    times, counts, sizes = {k: [] for k in names}, {}, {}
    from damvsnet_amd import scene
    for rep in range(a.repeats + 1):  # run 0 is the warm-up of each
        order = list(range(len(names)))
        for i in order[rep % len(names):] + order[:rep % len(names)]:
            ply = os.path.join(root, names[i] + ".ply")
            kw = {} if voxels[i] is None else {"voxel": voxels[i]}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = scene.reconstruct_scene(net, data, scan, ply, nviews=a.nviews, max_h=a.H, max_w=a.W, batch=a.batch,
                                        inputs="device", features="scene", **kw)
            dt = time.perf_counter() - t0
            counts[names[i]], sizes[names[i]] = n, os.path.getsize(ply)
            if rep:
                times[names[i]].append(round(dt, 4))
            print("run %d %-10s %.4f s, %d points%s" % (rep, names[i], dt, n, "" if rep else " (warm-up)"), flush=True)
    res = {"metric": "seconds, loaded model to PLY on disk, reconstruct_scene(inputs=device, features=scene)",
           "views": a.views, "shape": [a.H, a.W], "points": counts, "ply_bytes": sizes}
    for k in names:
        res[k + "_s"], res[k + "_median_s"] = times[k], round(float(np.median(times[k])), 4)
    res["launches"] = thin_launches(a, a.H, a.W)
    return res


def normal_launches(a, H, W, calls=20):
    """Per reference view, each alone: compact_cloud's three launches (15-byte records), its oriented form (the same
    three at capacity 0, then the oriented scatter: 27-byte records with the normal computed per selected pixel) and the
    normal map launch. The record buffer holds `calls` views, so every timed call scatters all its records."""
    from damvsnet_amd import fusion, synth
    proj, _, dv = synth.cameras(1, a.views, H, W)
    K, E = proj["stage3"][0, 0, 1, :3, :3].copy(), proj["stage3"][0, 0, 0].copy()
    depth_mid = float(dv[0, 0] + dv[0, -1]) / 2
    g = torch.Generator(device="cuda").manual_seed(0)
    # a smooth surface with relief of a few per cent: most neighbours pass the 0.01 step test, some do not
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32),
                            torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    depth = (depth_mid * (1 + 0.05 * torch.sin(xx / 40) * torch.cos(yy / 55))).contiguous()
    xyz = torch.rand(H, W, 3, device="cuda", generator=g)
    rgb = torch.zeros(H, W, 3, device="cuda", dtype=torch.uint8)
    masks = {"all": torch.full((H, W), 4, device="cuda", dtype=torch.uint8),
             "30%": (torch.rand(H, W, device="cuda", generator=g) < 0.3).to(torch.uint8) * 4}
    cams = fusion.fusion_cams(K, E, [])
    cursor = torch.zeros(1, device="cuda", dtype=torch.int64)
    res = {"shape": [H, W], "calls_per_block": calls}
    for sel, m in masks.items():
        n = int((m != 0).sum())
        plain = torch.empty(calls * n * fusion.RECORD_BYTES, device="cuda", dtype=torch.uint8)
        oriented = torch.empty(calls * n * fusion.ORIENTED_RECORD_BYTES, device="cuda", dtype=torch.uint8)
        scratch = fusion.compact_cloud(m, xyz, rgb, plain, cursor)
        row = {"selected_per_view": n,
               "compact_ms": _event_ms(lambda: fusion.compact_cloud(m, xyz, rgb, plain, cursor, scratch), calls=calls,
                                       before=cursor.zero_),
               "compact_oriented_ms": _event_ms(lambda: fusion.compact_cloud(
                   m, xyz, rgb, oriented, cursor, scratch, depth_avg=depth, cam=cams, normal_jump=0.01), calls=calls,
                   before=cursor.zero_),
               "normal_map_ms": _event_ms(lambda: fusion.normal_map(depth, m, K, E, 0.01), calls=calls)}
        row["record_MB"] = {"plain": round(n * fusion.RECORD_BYTES / 1e6, 1),
                            "oriented": round(n * fusion.ORIENTED_RECORD_BYTES / 1e6, 1)}
        res[sel] = row
        del plain, oriented
    return res


def normals_main(a, net, root, data, scan):
    from damvsnet_amd import scene
    names = ["plain", "normals"]
    times, counts, sizes = {k: [] for k in names}, {}, {}
    for rep in range(a.repeats + 1):  # run 0 is the warm-up of each
        for name in names[rep % 2:] + names[:rep % 2]:
            ply = os.path.join(root, name + ".ply")
            kw = {"normals": True} if name == "normals" else {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = scene.reconstruct_scene(net, data, scan, ply, nviews=a.nviews, max_h=a.H, max_w=a.W, batch=a.batch,
                                        inputs="device", features="scene", **kw)
            dt = time.perf_counter() - t0
            counts[name], sizes[name] = n, os.path.getsize(ply)
            if rep:
                times[name].append(round(dt, 4))
            print("run %d %-8s %.4f s, %d points%s" % (rep, name, dt, n, "" if rep else " (warm-up)"), flush=True)
    res = {"metric": "seconds, loaded model to PLY on disk, reconstruct_scene(inputs=device, features=scene)",
           "views": a.views, "shape": [a.H, a.W], "points": counts, "ply_bytes": sizes}
    for k in names:
        res[k + "_s"], res[k + "_median_s"] = times[k], round(float(np.median(times[k])), 4)
    res["launches"] = normal_launches(a, a.H, a.W)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--normals", action="store_true",
                    help="the oriented-cloud record instead: reconstruct_scene with and without normals=True, and the "
                         "oriented compaction beside the 15-byte one per view")
    ap.add_argument("--thin", action="store_true", help="the voxel-thinning record instead (the module docstring)")
    ap.add_argument("--voxels", default="2,8", help="--thin: two voxel edges in world units")
    ap.add_argument("--views", type=int, default=11)
    ap.add_argument("--H", type=int, default=1184)
    ap.add_argument("--W", type=int, default=1600)
    ap.add_argument("--H0", type=int, default=None, help="height of the image files (default: --H, no resize)")
    ap.add_argument("--W0", type=int, default=None, help="width of the image files (default: --W)")
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
        H0, W0 = a.H0 or a.H, a.W0 or a.W
        write_scene(data, scan, H0, W0, a.views)
        from damvsnet_amd import mvsio
        new_w, new_h, _ = mvsio.scale_mvs_camera(H0, W0, np.eye(3, dtype=np.float32), a.W, a.H)
        resized = (new_h, new_w) != (H0, W0)
        print("scene written: %d views at %d x %d, working size %d x %d" % (a.views, H0, W0, new_h, new_w), flush=True)
        if a.thin or a.normals:
            line = json.dumps((normals_main if a.normals else thin_main)(a, net, root, data, scan))
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            return
        names = ("files", "memory", "device", "cached")
        times, counts = {k: [] for k in names}, {}
        read = lambda name: open(os.path.join(root, name + ".ply"), "rb").read()
        for rep in range(a.repeats + 1):  # run 0 is the warm-up of each
            for name in names[rep % 4:] + names[:rep % 4]:
                out_dir, ply = os.path.join(root, "out_" + name), os.path.join(root, name + ".ply")
                shutil.rmtree(out_dir, ignore_errors=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if name == "files":
                    n = file_path(net, data, scan, out_dir, ply, a)
                elif name == "cached":
                    n = memory_path(net, data, scan, ply, a, "device", "scene")
                else:
                    n = memory_path(net, data, scan, ply, a, "host" if name == "memory" else "device")
                dt = time.perf_counter() - t0
                counts[name] = n
                if rep:
                    times[name].append(round(dt, 3))
                print("run %d %-6s %.3f s, %d points%s" % (rep, name, dt, n, "" if rep else " (warm-up)"), flush=True)
            assert read("files") == read("memory") and counts["files"] == counts["memory"], \
                "the file path and the memory path wrote different clouds"
            assert resized or (read("device") == read("memory") and counts["device"] == counts["memory"]), \
                "the device inputs and the host inputs wrote different clouds"
            assert read("cached") == read("device") and counts["cached"] == counts["device"], \
                "the cached features and the per-batch features wrote different clouds"
        imgs_diff = first_batch_imgs_diff(data, scan, a) if resized else 0.0
        assert imgs_diff <= 2.0 ** -21, "imgs of the device inputs differ from the host's by %.3e" % imgs_diff
        med = {k: float(np.median(v)) for k, v in times.items()}
        res = {"metric": "seconds, loaded model to PLY on disk", "views": a.views, "image_files": [H0, W0],
               "shape": [new_h, new_w], "nviews": a.nviews, "batch": a.batch, "dtype": "bf16", "ndepths": [48, 32, 8],
               "points": counts, "ply_identical": {"files_memory": True, "device_memory": not resized, "cached_device": True},
               "imgs_max_diff_device_host": imgs_diff}
        for k in names:
            res[k + "_s"], res[k + "_median_s"] = times[k], round(med[k], 3)
            res[k + "_spread_s"] = [min(times[k]), max(times[k])]
        res["ratio_memory_over_files"] = round(med["memory"] / med["files"], 4)
        res["ratio_device_over_memory"] = round(med["device"] / med["memory"], 4)
        res["ratio_cached_over_device"] = round(med["cached"] / med["device"], 4)
        res["device_breakdown_s"] = device_breakdown(net, data, scan, os.path.join(root, "breakdown_c.ply"), a, "batch")
        res["cached_breakdown_s"] = device_breakdown(net, data, scan, os.path.join(root, "breakdown_d.ply"), a, "scene")
        res["features"] = features_bench(a, new_h, new_w)
        res["memory_breakdown_s"] = breakdown(net, data, scan, os.path.join(root, "breakdown.ply"), a)
        res["ingest"] = ingest_bench(argparse.Namespace(**dict(vars(a), H=new_h, W=new_w)))
        res["inputs"] = inputs_bench(a)
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
