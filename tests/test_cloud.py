"""CPU: the host side of the GPU-compacted point cloud (damvs_fusion_cloud, fusion.compact_cloud / fuse_scene).

  * mvsio.write_ply_records(records) writes the file write_ply(xyz, rgb) writes;
  * the reference's colour, (float32(u) / 255 * 255).astype(uint8) (filter/dypcd.py:275-301 over an image read as
    float32 / 255), is u for every byte value: the kernel copies the image byte;
  * damvs_fusion_cloud_scratch / damvs_fusion_cloud validate before any device work (no GPU here).
The kernels themselves: tests/test_gpu_cloud.py; their code object: tests/test_cloud_codeobj.py.
"""
import ctypes

import numpy as np
import pytest

E_ARG, E_SHAPE = -1, -2
REC = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])


def test_record_layout_is_15_packed_bytes():
    from damvsnet_amd import mvsio
    assert REC.itemsize == mvsio.PLY_RECORD_BYTES == 15


@pytest.mark.parametrize("n", [0, 1, 7, 1000])
def test_write_ply_records_equals_write_ply(tmp_path, n):
    from damvsnet_amd import mvsio
    rng = np.random.default_rng(n)
    xyz = rng.standard_normal((n, 3)).astype(np.float32)
    xyz.view(np.uint32)[rng.random((n, 3)) < 0.1] = 0x7FC00001  # some NaN payloads: the bytes must pass untouched
    rgb = rng.integers(0, 256, size=(n, 3), dtype=np.uint8)
    v = np.empty(n, dtype=REC)
    v["x"], v["y"], v["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    v["red"], v["green"], v["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    mvsio.write_ply(a, xyz, rgb)
    for data in (v.tobytes(), bytearray(v.tobytes()), np.frombuffer(v.tobytes(), np.uint8)):
        mvsio.write_ply_records(b, data)
        assert open(a, "rb").read() == open(b, "rb").read()
    got_xyz, got_rgb = mvsio.read_ply(b)
    assert got_xyz.tobytes() == xyz.tobytes() and np.array_equal(got_rgb, rgb)


def test_write_ply_records_rejects_partial_records(tmp_path):
    from damvsnet_amd import mvsio
    with pytest.raises(ValueError):
        mvsio.write_ply_records(str(tmp_path / "x.ply"), bytes(16))


def test_reference_colour_is_the_image_byte():
    """The reference reads the image as float32(u) / 255 and stores (that * 255).astype(uint8): the identity on all 256
    byte values, so the kernel's byte copy is the reference's colour."""
    u = np.arange(256, dtype=np.uint8)
    assert np.array_equal((u.astype(np.float32) / 255 * 255).astype(np.uint8), u)
    # and in the spelling of mvsio.read_img / filter_depth (float32 array divided by a Python float)
    assert np.array_equal(((np.array(u, dtype=np.float32) / 255.0) * 255).astype(np.uint8), u)


def test_cloud_arg_errors_without_gpu():
    """Validation happens before any device work and reports through the error string."""
    from damvsnet_amd import _capi
    lib = _capi.load_library()
    assert lib.damvs_fusion_cloud_scratch(24, 40) == (24 * 40 + 255) // 256 + 2
    assert lib.damvs_fusion_cloud_scratch(1, 1) == 3
    for H, W in ((0, 40), (24, 0), (-1, 4), (2, 2 ** 30), (65536, 32768)):
        assert lib.damvs_fusion_cloud_scratch(H, W) == E_SHAPE, (H, W)
        assert b"shape" in lib.damvs_last_error_string()
    assert lib.damvs_fusion_cloud_scratch(1, 2 ** 31 - 1) == (2 ** 31 - 1 + 255) // 256 + 2

    p = ctypes.c_void_p(256)  # never dereferenced: every call below fails validation
    need = lib.damvs_fusion_cloud_scratch(24, 40)

    def call(H=24, W=40, mask=p, xyz=p, rgb=p, scratch=p, elems=need, records=p, capacity=10, cursor=p):
        return lib.damvs_fusion_cloud(None, H, W, mask, xyz, rgb, scratch, elems, records, capacity, cursor)

    for name in ("mask", "xyz", "rgb", "scratch", "records", "cursor"):
        assert call(**{name: None}) == E_ARG, name
        assert b"null" in lib.damvs_last_error_string()
    assert call(H=0) == E_SHAPE and call(W=0) == E_SHAPE and call(H=-3) == E_SHAPE
    assert call(H=65536, W=32768) == E_SHAPE and b"shape" in lib.damvs_last_error_string()
    assert call(elems=need - 1) == E_ARG and b"scratch" in lib.damvs_last_error_string()
    assert call(elems=0) == E_ARG
    assert call(capacity=-1) == E_ARG and b"capacity" in lib.damvs_last_error_string()
    # nulls are reported before shapes are looked at
    assert call(H=0, mask=None) == E_ARG


def test_python_entry_points_validate_without_gpu():
    import torch
    from damvsnet_amd import fusion
    with pytest.raises(ValueError):
        fusion.fuse_scene("x", "x", "x", "x.ply", method="gipuma")
    m = torch.zeros(4, 5, dtype=torch.uint8)
    with pytest.raises(ValueError, match="CUDA"):
        fusion.compact_cloud(m, torch.zeros(4, 5, 3), torch.zeros(4, 5, 3, dtype=torch.uint8),
                             torch.zeros(150, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64))
