"""CPU: scene inputs (damvs_scene_inputs, scene.SceneInputs, EvalScenes.cameras, reconstruct_scene(inputs="device"))
without a GPU.

  * tests/inputs_statement.py, the numpy statement of the kernel's arithmetic, against mvsio.resize_bilinear of the
    read_img-style float image (what the host path feeds the forward): at most 2^-21 apart. Both evaluations make at
    most 7 roundings of quantities <= 1 (the quotient, the coordinate, a weight, two products and a sum per row pair,
    the same again across rows), 2^-25 each; measured 1.8e-7;
  * at the identity size the statement is the byte's quotient, bit for bit, for every byte value;
  * EvalScenes.cameras(i) equals ds[i] without the pixels, bit for bit, on a scene at the working size and on one that
    needs the resize; scenes whose files differ in size are refused;
  * the C entry point's validation: every error comes back as DAMVS_E_ARG before any device work, with a message that
    names the argument;
  * the ValueErrors of SceneInputs and reconstruct_scene that need no device.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import scene_fixture as SF
from damvsnet_amd import mvsio
from inputs_statement import inputs_statement, noise, RESIZE_CASES

E_ARG = -1
BOUND = 2.0 ** -21
KW = dict(ndepths=8, interval_scale=1.06, max_h=1184, max_w=1600)


def write_scene(root, H0, W0, seed=5):
    """tests/scene_fixture.py's tree with images of H0 x W0 (lossless) and a pair list in which view 2 has sources
    too, so that every view is a reference view (the fixture's own drops it) -> the images (NV, H0, W0, 3) uint8."""
    from PIL import Image
    SF.make_scene(root)
    scan = os.path.join(root, "scan1")
    imgs = np.stack([noise(H0, W0, seed + v) for v in range(SF.NV)])
    for v in range(SF.NV):
        sub = "images_post" if v == 3 else "images"
        Image.fromarray(imgs[v]).save(os.path.join(scan, sub, "%08d.jpg" % v), format="PNG")
    with open(os.path.join(scan, "pair.txt"), "w") as f:
        f.write("%d\n" % len(SF.PAIRS))
        for ref, src in SF.PAIRS:
            src = src or [(3, 99.5), (4, 50.25)]
            f.write("%d\n%d %s\n" % (ref, len(src), " ".join("%d %g" % p for p in src)))
    return imgs


# --------------------------------------------------------------------------------------- the numpy statement
@pytest.mark.parametrize("case", RESIZE_CASES, ids=lambda c: "%dx%d-%dx%d" % c)
def test_statement_against_resize_bilinear(case):
    if torch.backends.cpu.get_cpu_capability() == "DEFAULT":
        pytest.skip("torch dispatches no FMA kernels on this CPU: its source coordinate is an unfused multiply and "
                    "subtract, and the difference to the statement becomes the coordinate's ulp times the gradient")
    H0, W0, H, W = case
    rgb = noise(H0, W0, H0 * 1000 + W0)
    want = mvsio.resize_bilinear(rgb.astype(np.float32) / 255.0, W, H).transpose(2, 0, 1)
    got = inputs_statement(rgb, H, W)
    diff = float(np.abs(got - want).max())
    print("%dx%d -> %dx%d: max |statement - resize_bilinear| = %.3e (bound %.3e)" % (H0, W0, H, W, diff, BOUND))
    assert got.shape == want.shape == (3, H, W) and diff <= BOUND


def test_statement_at_the_identity_size_is_the_byte_table():
    rgb = np.broadcast_to(np.arange(256, dtype=np.uint8).reshape(16, 16, 1), (16, 16, 3)).copy()
    table = np.arange(256, dtype=np.float32) / np.float32(255)
    got = inputs_statement(rgb, 16, 16)
    for c in range(3):
        assert got[c].tobytes() == table.tobytes()
    assert np.array_equal(got, (rgb.astype(np.float32) / 255.0).transpose(2, 0, 1))  # read_img's conversion


# --------------------------------------------------------------------------------------- EvalScenes.cameras
@pytest.mark.parametrize("size", [(SF.H, SF.W), (75, 100)], ids=lambda s: "%dx%d" % s)
def test_cameras_equal_the_items_without_pixels(tmp_path, size, monkeypatch):
    write_scene(str(tmp_path), *size)
    ds = mvsio.EvalScenes(str(tmp_path), ["scan1"], SF.NV, **KW)
    want = [ds[i] for i in range(len(ds))]
    monkeypatch.setattr(mvsio, "read_img", None)  # cameras decodes no image
    assert len(ds) == SF.NV
    for i, w in enumerate(want):
        got = ds.cameras(i)
        assert set(got) == (set(w) - {"imgs"}) | {"view_ids", "size", "original_size"}
        for s in ("stage1", "stage2", "stage3"):
            assert got["proj_matrices"][s].tobytes() == w["proj_matrices"][s].tobytes(), (i, s)
            assert got["proj_matrices"][s].dtype == w["proj_matrices"][s].dtype
            assert got["intrinsics_matrices"][s].tobytes() == w["intrinsics_matrices"][s].tobytes(), (i, s)
            assert got["intrinsics_matrices"][s].dtype == w["intrinsics_matrices"][s].dtype
        assert got["depth_values"].tobytes() == w["depth_values"].tobytes()
        assert got["depth_values"].dtype == w["depth_values"].dtype and got["filename"] == w["filename"]
        scan, ref, src = ds.metas[i]
        assert got["view_ids"] == [ref] + src[:SF.NV - 1]
        assert got["size"] == w["imgs"].shape[2:] and got["original_size"] == size
    if size == (75, 100):
        assert ds.cameras(0)["size"] == (64, 96)


def test_cameras_refuse_a_scene_of_two_sizes(tmp_path):
    from PIL import Image
    write_scene(str(tmp_path), 64, 96)
    Image.fromarray(noise(75, 100, 1)).save(str(tmp_path / "scan1" / "images" / ("%08d.jpg" % 1)), format="PNG")
    ds = mvsio.EvalScenes(str(tmp_path), ["scan1"], SF.NV, **KW)
    assert ds[0]["imgs"].shape == (SF.NV, 3, 64, 96)  # the host path serves it, each view resized from its own size
    with pytest.raises(ValueError, match="view 1 of scan1 is 75 x 100"):
        ds.cameras(0)
    with pytest.raises(ValueError, match="fix_res"):
        mvsio.EvalScenes(str(tmp_path), ["scan1"], SF.NV, fix_res=True, **KW).cameras(0)


# ----------------------------------------------------------------------------------------------- C entry point
@pytest.fixture(scope="module")
def lib():
    from damvsnet_amd import _capi, build
    build.build()
    return _capi.load_library()


def test_scene_inputs_validates_before_device_work(lib):
    P = 256  # never dereferenced: every call below fails validation
    ints = lambda *v: (ctypes.c_int * len(v))(*v)

    def call(n=3, H0=9, W0=10, H=8, W=12, V=6, store=P, slots=None, out=P):
        slots = ints(5, 0, 5) if slots is None else slots
        return lib.damvs_scene_inputs(None, n, H0, W0, H, W, V, store, slots, out)

    err = lambda: lib.damvs_last_error_string()
    assert call(store=None) == E_ARG and b"null rgb_store" in err()
    assert call(out=None) == E_ARG and b"null out" in err()
    assert lib.damvs_scene_inputs(None, 3, 9, 10, 8, 12, 6, P, None, P) == E_ARG and b"null slots" in err()
    assert call(n=0) == E_ARG and b"n_images 0" in err()
    assert call(n=-1) == E_ARG and b"n_images -1" in err()
    assert call(n=129, slots=ints(*([0] * 129))) == E_ARG and b"n_images 129" in err()
    for name in ("H0", "W0", "H", "W", "V"):
        for bad in (0, -4):
            assert call(**{name: bad}) == E_ARG and name.encode() in err() and b"1" in err(), (name, bad)
    for W in (10, 13, 2):
        assert call(W=W) == E_ARG and b"W %d" % W in err() and b"multiple of 4" in err()
    assert call(out=264) == E_ARG and b"out" in err() and b"aligned" in err()
    assert call(slots=ints(5, 6, 2)) == E_ARG and b"slot 6" in err()
    assert call(slots=ints(5, -1, 2)) == E_ARG and b"slot -1" in err()
    assert call(V=2) == E_ARG and b"slot 5" in err()
    # 3 * H * W < 2^31: the first sizes past it are refused, on either side
    assert 3 * 26752 * 26752 < 2 ** 31 <= 3 * 26756 * 26756
    assert call(H=26756, W=26756) == E_ARG and b"3 * H * W" in err()
    assert call(H0=26756, W0=26756) == E_ARG and b"3 * H0 * W0" in err()
    assert call(H0=1, W0=2 ** 30) == E_ARG and call(H=1, W=2 ** 30) == E_ARG


def test_binding_and_exports():
    import damvsnet_amd
    from damvsnet_amd import _capi, scene
    assert damvsnet_amd.SceneInputs is scene.SceneInputs and "SceneInputs" in damvsnet_amd.__all__
    assert "damvs_scene_inputs" in [s[0] for s in _capi.SIGNATURES] and _capi.INPUTS_MAX_IMAGES == 128
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "damvs.h")).read()
    assert "#define DAMVS_INPUTS_MAX_IMAGES 128" in header


# --------------------------------------------------------------------------------- the Python layer's errors
def test_scene_inputs_errors_without_a_device():
    from damvsnet_amd.scene import SceneInputs
    with pytest.raises(ValueError, match="distinct"):
        SceneInputs([0, 1, 0], 8, 8, 8, 8, "cpu")
    with pytest.raises(ValueError, match="distinct"):
        SceneInputs([], 8, 8, 8, 8, "cpu")
    for sizes in ((8, 8, 8, 10), (0, 8, 8, 8), (8, 8, 0, 8)):
        with pytest.raises(ValueError, match="multiple of 4"):
            SceneInputs([0, 1], *sizes, "cpu")
    si = SceneInputs([7, 3, 5], 6, 10, 4, 8, "cpu")
    assert tuple(si.store.shape) == tuple(si.mirror.shape) == (3, 6, 10, 3) and si.store.dtype == torch.uint8
    rgb = noise(6, 10, 0)
    si.put(3, rgb)
    assert np.array_equal(si.store[1].numpy(), rgb) and np.array_equal(si.mirror[1].numpy(), rgb)
    with pytest.raises(ValueError, match="view 3 put twice"):
        si.put(3, rgb)
    with pytest.raises(ValueError, match="view 4 is not one of"):
        si.put(4, rgb)
    for bad in (rgb[:, :, 0], np.dstack([rgb, rgb[:, :, :1]]), rgb.astype(np.float32), rgb[:5], noise(10, 6, 0)):
        with pytest.raises(ValueError, match="view 7 must be a uint8 image"):  # grey, RGBA, float, other sizes
            si.put(7, bad)
    with pytest.raises(ValueError, match="view 7 was never put"):
        si.batch([[3, 7]])
    with pytest.raises(ValueError, match="ragged"):
        si.batch([[3, 3], [3]])
    with pytest.raises(ValueError, match="1..128 images"):
        si.batch([[3] * 43] * 3)
    with pytest.raises(ValueError, match="1..128 images"):
        si.batch([])


def test_reconstruct_scene_refuses_bad_keywords_without_a_device(tmp_path):
    from damvsnet_amd.scene import reconstruct_scene
    ply = str(tmp_path / "never.ply")
    with pytest.raises(ValueError, match="inputs must be"):
        reconstruct_scene(None, str(tmp_path), "scan1", ply, inputs="gpu")
    for bad in (0, -1, 2.5, None):
        with pytest.raises(ValueError, match="decode_workers"):
            reconstruct_scene(None, str(tmp_path), "scan1", ply, inputs="device", decode_workers=bad)
    assert not os.path.exists(ply)
