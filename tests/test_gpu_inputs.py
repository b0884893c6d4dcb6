"""GPU: scene inputs, from the scene's decoded bytes on the device to the forward's `imgs` (k_inputs.hip,
scene.SceneInputs, reconstruct_scene(inputs="device")).

Every comparison of the kernel is bitwise against tests/inputs_statement.py: the kernel makes the statement's float32
operations one by one (a correctly rounded quotient, one fused multiply-add for the coordinate, separately rounded
products and sums), which numpy does bit for bit. `out` is a poisoned buffer with a guard band on either side.
  1. damvs_scene_inputs against the statement: the identity size with all 256 byte values in each channel; the four
     resizes of tests/test_inputs.py; one thread's 4 pixels (W = 4); a row one 4-pixel group wider than a block's 256
     pixels (W = 260); H = 1; 6 images as B = 2, N = 3 from a store of 5 with non-monotone slots and a view listed by
     both samples; 1 image and DAMVS_INPUTS_MAX_IMAGES images at 8 x 8; one image at 1200 x 1600 -> 1184 x 1568 (what
     scale_mvs_input gives DTU), from slot 1 of 2: byte offsets up to 5.76e6 and a grid of 7 x 296 blocks.
  2. one launch on a side stream beside a bf16 CascadeMVSNet.forward on the main stream equals the solo result.
  3. SceneInputs.batch against torch.stack of the host items' imgs on two written scenes: at the working size
     torch.equal, with 75 x 100 originals at most 2^-21 apart (tests/test_inputs.py has the bound's reasoning).
  4. reconstruct_scene(inputs="device") fills the SceneMaps and writes the PLY of inputs="host" bit for bit on the scene
     at the working size, with 1 and with 4 decode workers.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import scene_fixture as SF
from inputs_statement import inputs_statement, noise, RESIZE_CASES
from test_inputs import write_scene, BOUND, KW

pytestmark = pytest.mark.gpu
POISON, GUARD = 0xA5, 64


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from damvsnet_amd import build, _capi
    build.build()
    return _capi.load_library()


@functools.lru_cache(maxsize=None)
def case(V, H0, W0, H, W, slots):
    """A store of V noise images and, per image of the launch, the statement's output."""
    store = np.stack([noise(H0, W0, 100 * V + 7 * H0 + W0 + v) for v in range(V)])
    per_slot = {s: inputs_statement(store[s], H, W) for s in set(slots)}
    return store, [per_slot[s] for s in slots]


def guarded_out(n_floats):
    flat = torch.full((GUARD + 4 * n_floats + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    return flat, flat[GUARD:GUARD + 4 * n_floats]


def launch(lib, store_dev, slots, H, W, out, stream=None):
    from damvsnet_amd import _capi
    V, H0, W0, _ = store_dev.shape
    s = _capi.stream_ptr() if stream is None else stream.cuda_stream
    _capi.check(lib.damvs_scene_inputs(s, len(slots), H0, W0, H, W, V, store_dev.data_ptr(),
                                       (ctypes.c_int * len(slots))(*slots), out.data_ptr()))


def check_out(flat, want, H, W):
    got = flat.cpu().numpy().tobytes()
    poison = bytes([POISON]) * GUARD
    assert got[:GUARD] == poison and got[-GUARD:] == poison, "guard band"
    n = 3 * H * W * 4
    for i, w in enumerate(want):
        have = got[GUARD + i * n:GUARD + (i + 1) * n]
        if have != w.tobytes():
            h = np.frombuffer(have, np.float32).reshape(3, H, W)
            bad = np.argwhere(h.view(np.uint32) != w.view(np.uint32))
            raise AssertionError("image %d: %d of %d values differ, first at %s: got %r, statement %r, max diff %.3e" % (
                i, len(bad), h.size, bad[0], h[tuple(bad[0])], w[tuple(bad[0])], np.abs(h - w).max()))


def run(lib, V, H0, W0, H, W, slots, store=None, want=None):
    if store is None:
        store, want = case(V, H0, W0, H, W, tuple(slots))
    store_dev = torch.from_numpy(store).cuda()
    flat, out = guarded_out(len(slots) * 3 * H * W)
    torch.cuda.synchronize()
    launch(lib, store_dev, slots, H, W, out)
    torch.cuda.synchronize()
    check_out(flat, want, H, W)
    return flat


# ------------------------------------------------------------------------------------- 1. the entry point
def test_identity_size_gives_the_byte_table(lib):
    rgb = np.empty((16, 16, 3), np.uint8)
    for c in range(3):  # every byte value in every channel, at other places
        rgb[:, :, c] = np.roll(np.arange(256, dtype=np.uint8), 85 * c).reshape(16, 16)
    want = inputs_statement(rgb, 16, 16)
    table = np.arange(256, dtype=np.float32) / np.float32(255)
    assert all(np.array_equal(want[c], table[rgb[:, :, c]]) for c in range(3))
    run(lib, 1, 16, 16, 16, 16, [0], store=rgb[None], want=[want])


SHAPES = RESIZE_CASES + [(5, 7, 3, 4),        # W = 4: one thread per row
                         (10, 270, 6, 260),   # W = 260: the second block of a row has one thread
                         (3, 20, 1, 16),      # H = 1
                         (64, 96, 64, 96)]    # the working size of the written scene, no resize


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_inputs_equal_numpy_statement(lib, shape):
    H0, W0, H, W = shape
    run(lib, 3, H0, W0, H, W, [2, 0])


def test_batch_of_two_samples_from_five_views(lib):
    """i = b * N + n: the buffer is the contiguous (B, N, 3, H, W) tensor; view 3 is listed by both samples."""
    run(lib, 5, 20, 24, 16, 20, [3, 0, 4, 1, 3, 2])


@pytest.mark.parametrize("n", [1, 128])
def test_fewest_and_most_images(lib, n):
    from damvsnet_amd import _capi
    assert _capi.INPUTS_MAX_IMAGES == 128
    run(lib, 7, 9, 11, 8, 8, [(5 * i + 3) % 7 for i in range(n)])


def test_full_size_image(lib):
    H0, W0, H, W = 1200, 1600, 1184, 1568
    assert mvs_size(H0, W0) == (H, W)
    flat = run(lib, 2, H0, W0, H, W, [1])
    assert flat.numel() == 2 * GUARD + 3 * H * W * 4


def mvs_size(H0, W0):
    from damvsnet_amd import mvsio
    new_w, new_h, _ = mvsio.scale_mvs_camera(H0, W0, np.eye(3, dtype=np.float32), 1600, 1184)
    return new_h, new_w


# ------------------------------------------------------------------------------------- 2. beside a forward
def test_inputs_on_a_side_stream_beside_a_bf16_forward(lib):
    """One launch on a side stream while a bf16 CascadeMVSNet.forward runs on the main stream, once: the output equals
    the solo result (the kernel is VALU only and carries no packed-FP32 ops, tests/test_inputs_codeobj.py)."""
    from common import model_state, forward_inputs
    from damvsnet_amd.cascade import CascadeMVSNet
    V, H0, W0, H, W, slots = 5, 75, 100, 64, 96, (3, 0, 4, 1, 3, 2)
    store, want = case(V, H0, W0, H, W, slots)
    solo = run(lib, V, H0, W0, H, W, list(slots))
    net = CascadeMVSNet(ndepths=[8, 8, 8], compute_dtype=torch.bfloat16, frontend_dtype=torch.bfloat16)
    net.load_state_dict(model_state("forward_160x128_48_32_8"), strict=True)
    net = net.cuda().eval()
    imgs, proj, dv, _ = forward_inputs(1, 3, 32, 64)
    imgs, dv, proj = imgs.cuda(), dv.cuda(), {k: v.cuda() for k, v in proj.items()}
    side = torch.cuda.Stream()
    store_dev = torch.from_numpy(store).cuda()
    flat, out = guarded_out(len(slots) * 3 * H * W)
    torch.cuda.synchronize()  # the side stream has nothing to wait for
    with torch.no_grad():
        res = net(imgs, proj, dv, check_range=False)  # enqueued on the main stream, not waited for
    launch(lib, store_dev, list(slots), H, W, out, stream=side)
    torch.cuda.synchronize()
    net.DepthNet.check_range()
    assert res["depth"].shape == (1, 32, 64)
    assert torch.equal(flat, solo)
    check_out(flat, want, H, W)


# ------------------------------------------------------------------------------------- 3. SceneInputs
def filled_inputs(ds, imgs_u8, size):
    from damvsnet_amd.scene import SceneInputs
    cam = ds.cameras(0)
    assert cam["original_size"] == size
    si = SceneInputs(range(SF.NV), *size, *cam["size"], "cuda")
    assert si.mirror.is_pinned() and si.store.is_cuda
    for v in (3, 0, 4, 2, 1):
        si.put(v, imgs_u8[v])
    return si


@pytest.mark.parametrize("size", [(64, 96), (75, 100)], ids=lambda s: "%dx%d" % s)
def test_scene_inputs_batch_against_the_host_items(lib, tmp_path, size):
    from damvsnet_amd import mvsio
    imgs_u8 = write_scene(str(tmp_path), *size)
    ds = mvsio.EvalScenes(str(tmp_path), ["scan1"], SF.NV, **KW)
    si = filled_inputs(ds, imgs_u8, size)
    assert torch.equal(si.store.cpu(), torch.from_numpy(imgs_u8))
    items = [ds[i] for i in (1, 4)]
    want = torch.stack([torch.from_numpy(np.ascontiguousarray(it["imgs"])) for it in items])
    views = [ds.cameras(i)["view_ids"] for i in (1, 4)]
    got = si.batch(views)
    assert got.shape == want.shape == (2, SF.NV, 3, 64, 96) and got.dtype == torch.float32 and got.is_contiguous()
    diff = float((got.cpu() - want).abs().max())
    print("%d x %d originals: max |device - host| = %.3e" % (size[0], size[1], diff))
    if size == (64, 96):
        assert torch.equal(got.cpu(), want)
    else:
        assert diff <= BOUND
        for b, sample in enumerate(views):  # and the statement, exactly
            for n, v in enumerate(sample):
                assert np.array_equal(got[b, n].cpu().numpy(), inputs_statement(imgs_u8[v], 64, 96)), (b, n, v)
    # out is reused when it fits (a smaller batch takes its leading part) and replaced when it does not
    again = si.batch(views[:1], out=got)
    assert again.data_ptr() == got.data_ptr() and again.shape == (1, SF.NV, 3, 64, 96)
    assert torch.equal(again.cpu(), got[:1].cpu())
    small = torch.empty(3, device="cuda")
    assert si.batch(views, out=small).data_ptr() != small.data_ptr()


# ------------------------------------------------------------------------------------- 4. reconstruct_scene
def test_reconstruct_scene_device_inputs_equal_host_inputs(lib, tmp_path, monkeypatch):
    """The scene at the working size (64 x 96, 5 views, every view a reference view) through a synthetic-weight fp32
    model in batches of 2: the device path's images are the host's bit for bit, so the maps and the PLY are too.
    tests/test_gpu_scene.py's plane case tests the fusion's content."""
    from common import model_state
    from damvsnet_amd import mvsio, scene
    from damvsnet_amd.cascade import CascadeMVSNet
    data = str(tmp_path / "data")
    imgs_u8 = write_scene(data, 64, 96)
    net = CascadeMVSNet(ndepths=[8, 8, 8])
    net.load_state_dict(model_state("forward_160x128_48_32_8"), strict=True)
    net = net.cuda().eval()
    kw = dict(nviews=SF.NV, batch=2, conf=(0.0, 0.0, 0.0), thres_view=2, method="pcd", **KW)
    ply = {k: str(tmp_path / (k + ".ply")) for k in ("host", "device1", "device4")}
    kept, real_fuse = [], scene.SceneMaps.fuse

    def fuse(self, *a, **k):
        kept.append(self)
        return real_fuse(self, *a, **k)

    monkeypatch.setattr(scene.SceneMaps, "fuse", fuse)
    n_host = scene.reconstruct_scene(net, data, "scan1", ply["host"], **kw)
    opened, real = {}, mvsio.read_img_bytes

    def counting(filename):
        opened[filename] = opened.get(filename, 0) + 1
        return real(filename)

    monkeypatch.setattr(mvsio, "read_img_bytes", counting)
    monkeypatch.setattr(mvsio, "read_img", None)  # the device path converts nothing on the host
    n_1 = scene.reconstruct_scene(net, data, "scan1", ply["device1"], inputs="device", decode_workers=1, **kw)
    assert len(opened) == SF.NV and set(opened.values()) == {1}, opened
    n_4 = scene.reconstruct_scene(net, data, "scan1", ply["device4"], inputs="device", decode_workers=4, **kw)
    print("reconstruct_scene points: host %d, device %d / %d" % (n_host, n_1, n_4))
    assert n_host == n_1 == n_4
    want = open(ply["host"], "rb").read()
    assert open(ply["device1"], "rb").read() == want and open(ply["device4"], "rb").read() == want
    # the cloud of random weights may be empty, so the maps the fusion read are compared too: every depth map,
    # confidence and colour of the device path is the host path's
    host, dev1, dev4 = kept
    for other in (dev1, dev4):
        assert other.view_ids == host.view_ids == list(range(SF.NV))
        assert torch.equal(other.depth, host.depth) and torch.equal(other.conf, host.conf)
        assert torch.equal(other.rgb, host.rgb)
    assert torch.equal(host.rgb.cpu(), torch.from_numpy(imgs_u8))
