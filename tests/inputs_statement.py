"""The numpy float32 statement of what damvs_scene_inputs writes (include/damvs.h, k_inputs.hip), shared by
tests/test_inputs.py (CPU: the statement against mvsio.resize_bilinear) and tests/test_gpu_inputs.py (GPU: the kernel
against the statement, bit for bit).

Every operation is one float32 operation rounded to nearest; the coordinate's multiply-add is rounded once (the product
and the difference are formed in float64, where both are exact for the sizes in use, and rounded to float32).
"""
import numpy as np

f32 = np.float32


def axis(n_in, n_out):
    """-> (i0, i1 int64, l0, l1 float32), each of length n_out: the two source samples of an output sample and their
    weights."""
    scale = f32(n_in) / f32(n_out)
    d = np.arange(n_out, dtype=f32) + f32(0.5)
    src = (np.float64(scale) * d.astype(np.float64) - 0.5).astype(f32)  # fma(scale, d + 0.5f, -0.5f)
    src = np.maximum(src, f32(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = src - i0.astype(f32)
    l0 = f32(1) - l1
    assert l0.dtype == l1.dtype == f32
    return i0, i1, l0, l1


def inputs_statement(rgb, H, W):
    """rgb (H0, W0, 3) uint8 -> (3, H, W) float32: the image as float32 in [0, 1], resized to H x W, planar."""
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    H0, W0 = rgb.shape[:2]
    p = np.transpose(rgb, (2, 0, 1)).astype(f32) / f32(255)
    y0, y1, a0, a1 = axis(H0, H)
    x0, x1, b0, b1 = axis(W0, W)
    a0, a1 = a0[:, None], a1[:, None]
    top = b0 * p[:, y0][:, :, x0] + b1 * p[:, y0][:, :, x1]
    bot = b0 * p[:, y1][:, :, x0] + b1 * p[:, y1][:, :, x1]
    out = a0 * top + a1 * bot
    assert out.dtype == f32
    return out


def noise(H0, W0, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(H0, W0, 3), dtype=np.uint8)


# (H0, W0, H, W): both axes shrink, both shrink by other ratios, one axis only, enlarging (both clamps are used)
RESIZE_CASES = [(75, 100, 64, 96), (70, 90, 64, 64), (40, 96, 32, 96), (30, 28, 32, 32)]
