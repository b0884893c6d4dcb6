"""GPU: the scene-level FeatureNet cache (k_features.hip, scene.SceneFeatures, CascadeMVSNet.forward(features=),
reconstruct_scene(features="scene")).

Every comparison is bitwise: the gather moves bytes, and FeatureNet's result for an image does not depend on the rest of
its batch (tests/test_gpu_streams.py: sub-batches are bitwise the full batch). Outputs are poisoned buffers with a guard
band on either side.
  1. damvs_feature_gather against numpy indexing on random bytes: K = 1 and K = 3 tensors of 16 bytes (one vector), 48
     bytes and a size that is no multiple of a block's 4096 bytes and takes the four-vector loop once and the
     one-vector loop after it (five grid passes and 2064 bytes; the grid is min(blocks needed, 2048 / (n * K)) blocks,
     include/damvs.h); n = 1 and n = 128 pairs; repeated slots, slots 0 and V - 1; the three stage shapes of a 64 x 96
     image at fp32 and bf16 element sizes as B = 2, N = 5.
  2. a store whose last slot begins beyond 4 GiB (32 769 slots of 128 KiB): slot 0 and the last slot gathered.
  3. SceneFeatures.batch against model.extract_features on the written scene (64 x 96, 5 views), fp32 and bf16 front
     ends, views put one by one and in a non-consecutive group, and all five in one group on a second instance.
  4. model(..., features=f) against model(...) on every tensor of the output: full imgs, reference-only imgs,
     streams=2, fp32 and bf16.
  5. reconstruct_scene(features="scene") against "batch": maps and PLY, host and device inputs; exactly 5 images pass
     through FeatureNet, against B * N per batch.
  6. one gather on a side stream beside a bf16 forward on the main stream equals the solo result.
  7. the ValueErrors, each naming its views, with nothing written.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import scene_fixture as SF
from test_inputs import write_scene, KW

pytestmark = pytest.mark.gpu
POISON, GUARD = 0xA5, 64
BLOCK_BYTES, GRID_BLOCKS = 256 * 16, 2048
H, W = 64, 96
STAGE_ELEMS = (H // 4 * (W // 4) * 32, H // 2 * (W // 2) * 16, H * W * 8)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from damvsnet_amd import build, _capi
    build.build()
    return _capi.load_library()


def grid_pass_bytes(n, K, largest):
    """Bytes of a view that one pass of the launch's grid covers (include/damvs.h)."""
    return min(-(-largest // BLOCK_BYTES), GRID_BLOCKS // (n * K)) * BLOCK_BYTES


def big(n, K):
    """A view that takes the four-vector loop once and then the one-vector loop, ending inside a block."""
    size = 5 * (GRID_BLOCKS // (n * K)) * BLOCK_BYTES + 2064
    assert size % 16 == 0 and size % BLOCK_BYTES and 5 * grid_pass_bytes(n, K, size) < size < 6 * grid_pass_bytes(n, K, size)
    return size


def guarded(nbytes):
    flat = torch.full((GUARD + nbytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    return flat, flat[GUARD:GUARD + nbytes]


def gather(lib, stores, view_bytes, slots, outs, V, stream=None):
    from damvsnet_amd import _capi
    K, n = len(stores), len(slots)
    s = _capi.stream_ptr() if stream is None else stream.cuda_stream
    _capi.check(lib.damvs_feature_gather(s, n, K, V, (ctypes.c_void_p * K)(*[t.data_ptr() for t in stores]),
                                         (ctypes.c_ulonglong * K)(*view_bytes), (ctypes.c_int * n)(*slots),
                                         (ctypes.c_void_p * K)(*[t.data_ptr() for t in outs])))


def check_guarded(flat, want, what):
    got = flat.cpu().numpy()
    assert (got[:GUARD] == POISON).all() and (got[-GUARD:] == POISON).all(), "guard band of %s" % (what,)
    body = got[GUARD:-GUARD].reshape(want.shape)
    if not np.array_equal(body, want):
        bad = np.argwhere(body != want)
        raise AssertionError("%s: %d of %d bytes differ, first at pair %d byte %d" % (
            what, len(bad), want.size, bad[0][0], bad[0][1]))


def run(lib, V, view_bytes, slots, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed + 17 * len(slots) + len(view_bytes))
    stores = [torch.randint(0, 256, (V, vb), device="cuda", dtype=torch.uint8, generator=g) for vb in view_bytes]
    outs = [guarded(len(slots) * vb) for vb in view_bytes]
    torch.cuda.synchronize()
    gather(lib, stores, view_bytes, slots, [o for _, o in outs], V)
    torch.cuda.synchronize()
    for k, (store, (flat, _)) in enumerate(zip(stores, outs)):
        check_guarded(flat, store.cpu().numpy()[np.asarray(slots)], "tensor %d of %s" % (k, list(view_bytes)))
    return stores, [flat for flat, _ in outs]


# ------------------------------------------------------------------------------------- 1. the entry point
def slots_for(n, V):
    """n slots of a V-slot store: 0 and V - 1 first (as far as n allows), then a non-monotone walk with repeats."""
    return ([V - 1, 0] + [(5 * i + 3) % V for i in range(n)])[:n]


@pytest.mark.parametrize("n", [1, 128])
@pytest.mark.parametrize("K", [1, 3])
def test_gather_equals_numpy_indexing(lib, K, n):
    from damvsnet_amd import _capi
    assert _capi.FEATURES_MAX_PAIRS == 128
    V = 3 if n == 1 else 7
    if K == 1:
        for vb in (16, 48, big(n, 1)):
            run(lib, V, (vb,), slots_for(n, V))
            if n == 1:  # the one pair from slot 0 as well
                run(lib, V, (vb,), [0], seed=1)
    else:
        # three tensors of different sizes in one launch, the large one first, last and in the middle
        sizes = (16, 48, big(n, 3))
        for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
            run(lib, V, tuple(sizes[i] for i in order), slots_for(n, V))


@pytest.mark.parametrize("es", [4, 2], ids=["fp32", "bf16"])
def test_gather_of_the_stage_shapes(lib, es):
    """B = 2, N = 5 from a store of 5 views, pairs view-major; every sample lists view 3, sample 1 lists view 0 twice."""
    views = [[3, 0, 4, 1, 2], [0, 3, 0, 2, 4]]
    slots = [views[b][n] for n in range(5) for b in range(2)]
    run(lib, 5, tuple(e * es for e in STAGE_ELEMS), slots)


# ------------------------------------------------------------------------------------- 2. 64-bit slot base
def test_slot_base_beyond_4_gib(lib):
    vb, V = 128 << 10, 32769
    assert (V - 1) * vb == 1 << 32
    if torch.cuda.mem_get_info()[0] < 8 << 30:
        pytest.skip("less than 8 GiB of device memory free")
    store = torch.empty(V, vb, dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(3)
    first = torch.randint(0, 256, (vb,), device="cuda", dtype=torch.uint8, generator=g)
    last = torch.randint(0, 256, (vb,), device="cuda", dtype=torch.uint8, generator=g)
    store[0], store[V - 1] = first, last
    assert not torch.equal(first, last)
    flat, out = guarded(3 * vb)
    torch.cuda.synchronize()
    gather(lib, [store], (vb,), [V - 1, 0, V - 1], [out], V)
    torch.cuda.synchronize()
    check_guarded(flat, torch.stack([last, first, last]).cpu().numpy(), "slots V - 1, 0, V - 1")
    del store


# ------------------------------------------------------------------------------------- 3. SceneFeatures
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


@functools.lru_cache(maxsize=None)
def model(dtype):
    from common import model_state
    from damvsnet_amd.cascade import CascadeMVSNet
    kw = {} if dtype == "fp32" else dict(compute_dtype=torch.bfloat16, frontend_dtype=torch.bfloat16)
    net = CascadeMVSNet(ndepths=[8, 8, 8], **kw)
    net.load_state_dict(model_state("forward_160x128_48_32_8"), strict=True)
    return net.cuda().eval()


def guarded_buffers(sf, n):
    """{stage: (flat, buffer)} for SceneFeatures.batch(out=): the stores' dtype, n views, a guard band either side."""
    bufs = {}
    for k, t in sf.stores.items():
        flat, body = guarded(n * t[0].numel() * t.element_size())
        bufs[k] = (flat, body.view(t.dtype).view((n,) + tuple(t.shape[1:])))
    return bufs


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_scene_features_batch_equals_extract_features(lib, tmp_path, dtype):
    from damvsnet_amd import mvsio
    from damvsnet_amd.scene import SceneFeatures
    net = model(dtype)
    write_scene(str(tmp_path), H, W)
    ds = mvsio.EvalScenes(str(tmp_path), ["scan1"], SF.NV, **KW)
    picked = (1, 4)
    imgs = torch.from_numpy(np.stack([np.ascontiguousarray(ds[i]["imgs"]) for i in picked])).cuda()
    views = [ds.cameras(i)["view_ids"] for i in picked]
    view_img = {v: imgs[b, n] for b, sample in enumerate(views) for n, v in enumerate(sample)}
    assert imgs.shape == (2, SF.NV, 3, H, W) and sorted(view_img) == list(range(SF.NV)), views
    with torch.no_grad():
        want = net.extract_features(imgs)
    one_by_one = SceneFeatures(net, range(SF.NV), H, W)
    assert one_by_one.nbytes == SF.NV * 14 * H * W * DTYPES[dtype].itemsize
    assert {k: tuple(t.shape) for k, t in one_by_one.stores.items()} == {
        "stage1": (SF.NV, H // 4, W // 4, 32), "stage2": (SF.NV, H // 2, W // 2, 16), "stage3": (SF.NV, H, W, 8)}
    one_by_one.put([3, 0], torch.stack([view_img[3], view_img[0]]))  # slots 3, 0: computed aside, then copied in
    for v in (4, 2, 1):
        one_by_one.put([v], view_img[v][None])
    grouped = SceneFeatures(net, range(SF.NV), H, W)
    grouped.put(range(SF.NV), torch.stack([view_img[v] for v in range(SF.NV)]))  # consecutive slots: written in place
    for k in grouped.stores:
        assert grouped.stores[k].dtype == DTYPES[dtype] and torch.equal(grouped.stores[k], one_by_one.stores[k]), k
    for sf in (one_by_one, grouped):
        bufs = guarded_buffers(sf, 2 * SF.NV)
        got = sf.batch(views, out={k: b for k, (_, b) in bufs.items()})
        torch.cuda.synchronize()
        assert len(got) == len(want) == SF.NV
        for n in range(SF.NV):
            assert set(got[n]) == set(want[n]) == {"stage1", "stage2", "stage3"}
            for k in want[n]:
                assert got[n][k].shape == want[n][k].shape and got[n][k].dtype == want[n][k].dtype
                assert got[n][k].is_contiguous() and got[n][k].data_ptr() == bufs[k][1][2 * n:].data_ptr()
                assert torch.equal(got[n][k], want[n][k]), (n, k)
        for k, (flat, _) in bufs.items():
            assert bool((flat[:GUARD] == POISON).all()) and bool((flat[-GUARD:] == POISON).all()), k
    # out is reused when it fits (a smaller batch takes its leading part) and replaced when it does not
    sf = grouped
    bufs = sf.buffers(2 * SF.NV)
    full = sf.batch(views, out=bufs)
    again = sf.batch(views[:1], out=bufs)
    for k in bufs:
        assert full[0][k].data_ptr() == again[0][k].data_ptr() == bufs[k].data_ptr()
        assert again[0][k].shape[0] == 1 and again[SF.NV - 1][k].data_ptr() == bufs[k][SF.NV - 1:].data_ptr()
        for n in range(SF.NV):
            assert torch.equal(again[n][k], want[n][k][:1]), (n, k)
    small = {k: torch.empty(3, device="cuda", dtype=DTYPES[dtype]) for k in bufs}
    fresh = sf.batch(views, out=small)
    assert all(fresh[0][k].data_ptr() != small[k].data_ptr() and torch.equal(fresh[1][k], want[1][k]) for k in small)


# ------------------------------------------------------------------------------------- 4. forward
@functools.lru_cache(maxsize=None)
def forward_case(dtype):
    """B = 2, N = 3 at 64 x 96: the inputs on the device, the plain forward's outputs, and the same views' features
    from a SceneFeatures in which sample b's view n is view 3 * b + n."""
    from common import forward_inputs
    from damvsnet_amd.scene import SceneFeatures
    net = model(dtype)
    imgs, proj, dv, ins = forward_inputs(2, 3, H, W)
    imgs, dv = imgs.cuda(), dv.cuda()
    proj, ins = {k: v.cuda() for k, v in proj.items()}, {k: v.cuda() for k, v in ins.items()}
    with torch.no_grad():
        want = net(imgs, proj, dv, ins)
    sf = SceneFeatures(net, range(6), H, W)
    sf.put(range(6), imgs.reshape(6, 3, H, W))
    return imgs, proj, dv, ins, want, sf


def assert_same(got, want, path="out"):
    if isinstance(want, dict):
        assert set(got) == set(want), path
        for k in want:
            assert_same(got[k], want[k], "%s[%r]" % (path, k))
    elif torch.is_tensor(want):
        assert got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want), path
    else:
        assert got == want, path


@pytest.mark.parametrize("how", ["full", "reference-only", "streams2"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_forward_with_given_features_equals_the_forward(lib, dtype, how):
    imgs, proj, dv, ins, want, sf = forward_case(dtype)
    net = model(dtype)
    calls = []
    f = sf.batch([[0, 1, 2], [3, 4, 5]])
    with torch.no_grad():
        got = net(imgs[:, :1] if how == "reference-only" else imgs, proj, dv, ins, features=f,
                  streams=2 if how == "streams2" else 1, stage_hook=None if how == "streams2" else calls.append)
    torch.cuda.synchronize()
    assert how == "streams2" or calls[0] == "features"  # the hook still fires
    assert_same(got, want)


# ------------------------------------------------------------------------------------- 5. reconstruct_scene
def test_reconstruct_scene_scene_features_equal_batch_features(lib, tmp_path, monkeypatch):
    from damvsnet_amd import scene
    from damvsnet_amd.frontend_hip import HipFeatureNet
    data = str(tmp_path / "data")
    write_scene(data, H, W)
    net = model("fp32")
    kw = dict(nviews=SF.NV, batch=2, conf=(0.0, 0.0, 0.0), thres_view=2, method="pcd", **KW)
    kept, real_fuse = [], scene.SceneMaps.fuse

    def fuse(self, *a, **k):
        kept.append(self)
        return real_fuse(self, *a, **k)

    monkeypatch.setattr(scene.SceneMaps, "fuse", fuse)
    images, real_call = [0], HipFeatureNet.__call__

    def counting(self, x, out=None):
        images[0] += x.shape[0] * (x.shape[1] if x.dim() == 5 else 1)
        return real_call(self, x, out=out)

    monkeypatch.setattr(HipFeatureNet, "__call__", counting)
    counts, points, ply = {}, {}, {}
    for inputs in ("host", "device"):
        for features in ("batch", "scene"):
            name = inputs + "-" + features
            ply[name] = str(tmp_path / (name + ".ply"))
            images[0] = 0
            points[name] = scene.reconstruct_scene(net, data, "scan1", ply[name], inputs=inputs, features=features, **kw)
            counts[name] = images[0]
    print("reconstruct_scene points %s, images through FeatureNet %s" % (points, counts))
    # 5 samples in batches of 2, 2 and 1, each of 5 views, against the scene's 5 views once
    assert counts == {"host-batch": 25, "host-scene": 5, "device-batch": 25, "device-scene": 5}
    assert len(set(points.values())) == 1
    want = open(ply["host-batch"], "rb").read()
    assert all(open(p, "rb").read() == want for p in ply.values())
    base = kept[0]
    for other in kept[1:]:
        assert other.view_ids == base.view_ids == list(range(SF.NV))
        assert torch.equal(other.depth, base.depth) and torch.equal(other.conf, base.conf)
        assert torch.equal(other.rgb, base.rgb)


# ------------------------------------------------------------------------------------- 6. beside a forward
def test_gather_on_a_side_stream_beside_a_bf16_forward(lib):
    """One launch on a side stream while a bf16 CascadeMVSNet.forward runs on the main stream, once: the output equals
    the solo result (the kernel carries no packed-FP32 ops, tests/test_features_codeobj.py)."""
    from common import forward_inputs
    view_bytes = tuple(2 * e for e in STAGE_ELEMS)
    slots = [3, 0, 4, 1, 3, 2, 0, 3, 0, 2]
    stores, solo = run(lib, 5, view_bytes, slots)
    net = model("bf16")
    imgs, proj, dv, _ = forward_inputs(1, 3, 32, 64)
    imgs, dv, proj = imgs.cuda(), dv.cuda(), {k: v.cuda() for k, v in proj.items()}
    side = torch.cuda.Stream()
    outs = [guarded(len(slots) * vb) for vb in view_bytes]
    torch.cuda.synchronize()  # the side stream has nothing to wait for
    with torch.no_grad():
        res = net(imgs, proj, dv, check_range=False)  # enqueued on the main stream, not waited for
    gather(lib, stores, view_bytes, slots, [o for _, o in outs], 5, stream=side)
    torch.cuda.synchronize()
    net.DepthNet.check_range()
    assert res["depth"].shape == (1, 32, 64)
    for (flat, _), alone in zip(outs, solo):
        assert torch.equal(flat, alone)


# ------------------------------------------------------------------------------------- 7. errors
def test_errors_name_their_views_and_write_nothing(lib):
    from common import model_state
    from damvsnet_amd.cascade import CascadeMVSNet
    from damvsnet_amd.scene import SceneFeatures
    imgs, proj, dv, ins, want, filled = forward_case("fp32")
    net = CascadeMVSNet(ndepths=[8, 8, 8])  # a model of this test's own: its weights are reloaded below
    net.load_state_dict(model_state("forward_160x128_48_32_8"), strict=True)
    net = net.cuda().eval()
    sf = SceneFeatures(net, [7, 3, 5], H, W)
    for t in sf.stores.values():
        t.view(torch.uint8).fill_(POISON)
    untouched = lambda: all(bool((t.view(torch.uint8) == POISON).all()) for t in sf.stores.values())
    x = imgs.reshape(6, 3, H, W)
    with pytest.raises(ValueError, match="view 4 is not one of"):
        sf.put([3, 4], x[:2])
    with pytest.raises(ValueError, match="view 3 put twice"):
        sf.put([3, 5, 3], x[:3])
    for bad in (x[:1], x[:3], x[:2, :, :32], x[:2, :2], x[:2].double(), x[:2].cpu(), x[:2].cpu().numpy()):
        with pytest.raises(ValueError, match=r"imgs of views \[7, 3\]"):
            sf.put([7, 3], bad)
    with pytest.raises(ValueError, match="view 7 was never put"):
        sf.batch([[7]])
    assert untouched() and not sf._put
    sf.put([3], x[:1])
    with pytest.raises(ValueError, match="view 3 put twice"):
        sf.put([3], x[:1])
    with pytest.raises(ValueError, match="view 5 was never put"):
        sf.batch([[3, 5]])
    with pytest.raises(ValueError, match=r"ragged view lists \[\[3, 3\], \[3\]\]"):
        sf.batch([[3, 3], [3]])
    with pytest.raises(ValueError, match=r"1..128 \(sample, view\) pairs"):
        sf.batch([[3] * 43] * 3)
    with pytest.raises(ValueError, match=r"1..128 \(sample, view\) pairs"):
        sf.batch([])
    before = {k: t.clone() for k, t in sf.stores.items()}
    # the weights are reloaded: the features of view 3 no longer belong to the model
    net.load_state_dict(model_state("forward_160x128_48_32_8"), strict=True)
    with pytest.raises(ValueError, match=r"weights changed after views \[3\] were put"):
        sf.put([5], x[:1])
    with pytest.raises(ValueError, match=r"weights changed after views \[3\] were put"):
        sf.batch([[3]])
    assert all(torch.equal(before[k], sf.stores[k]) for k in before)
    # forward(features=)
    net = model("fp32")
    f = filled.batch([[0, 1, 2], [3, 4, 5]])
    with torch.no_grad():
        with pytest.raises(ValueError, match="features of 2 views"):
            net(imgs, proj, dv, ins, features=f[:2])
        with pytest.raises(ValueError, match=r"features\[0\]\[\"stage1\"\]"):
            net(imgs[:1], {k: v[:1] for k, v in proj.items()}, dv[:1], ins, features=f)  # B = 1 against B = 2
        with pytest.raises(ValueError, match=r"features\[0\]\[\"stage1\"\]"):
            net(imgs[..., :32, :], proj, dv, ins, features=f)  # another image size
        with pytest.raises(ValueError, match=r"features\[1\]\[\"stage2\"\]"):
            net(imgs, proj, dv, ins, features=[f[0], dict(f[1], stage2=f[1]["stage2"].bfloat16()), f[2]])
        with pytest.raises(ValueError, match=r"features\[2\]\[\"stage3\"\]"):
            net(imgs, proj, dv, ins, features=[f[0], f[1], {k: v for k, v in f[2].items() if k != "stage3"}])
