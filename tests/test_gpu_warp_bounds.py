"""Per-voxel bounded tests for the fused homography warp + cost aggregation (csrc/k_warp.hip: warp_aggregate_kernel and
warp_split_kernel, which are one body, csrc/k_warp_body.h, at 1 and at 2 / 4 / 8 lanes per voxel, and the rows launch_k
picks among them) and for damvs_proj_prepare.

Every compared voxel must satisfy |got - ref| <= bound, where ref is a float64 numpy evaluation of the operation on
the float32 operands the kernel receives (rt itself, the hypotheses, the features after their storage rounding, the
folded weight net) and bound is a first-order rounding model of a float32 evaluation, per voxel and per channel:

  coordinates  r_i = m[3i] x + m[3i+1] y + m[3i+2], q_i = r_i hyp + m[9+i], ix = (q_x / q_z) w/(w-1) - 1/2
               E_r = 4u (|m0 x| + |m1 y| + |m2|), E_q = E_r |hyp| + 2u (|r hyp| + |t|),          u = 2^-24
               dx = kx (E_qx + |q_x/q_z| E_qz) / |q_z| + 8u (|q_x/q_z| kx + 1), dy likewise
  sample       ds_c = dx Gx_c + dy Gy_c + 6u sum_k |w_k v_k|; Gx / Gy: the largest |horizontal / vertical neighbour
               difference| of the zero-padded map over rows y0-1 .. y0+2 and columns x0-1 .. x0+2 (the interpolant is
               continuous, so this covers a sample that lands in the neighbouring cell)
  warp-only    ds
  variance     dsum = sum ds_v + (N+1)u (|ref| + sum |s_v|), dsq = sum (2|s_v| ds_v + ds_v^2),
               dout = dsq/N + 2|mean| dsum/N + (dsum/N)^2 + 6u (sq/N + mean^2)
  adaptive     per view: dx_c = 2|df| ds + ds^2 + 4u x_c, ddot = sum |k1_c| dx_c + (C+2)u sum |k1_c x_c|,
               da1 = |s1| ddot + 3u (|dot s1| + |t1|), dwv = |s2| da1 + 3u (|a1 s2| + |t2| + 1),
               dacc += dwv x + wv dx + 3u wv x;  dout = dacc/(N-1) + (N+2)u acc/(N-1)
  bf16         + 2^-8 (|ref| + bound) for the single round-to-nearest store

The file brings its own inputs, because the shared ones leave the kernels' arguments unused: cameras and hypotheses
distinct per batch element, and a weight net per C whose two ReLUs are live and dead on real shares of the voxels
(with the seed-0 synthetic weights the 16-channel weight net is 0 on every voxel:
test_old_metric_misses_the_dead_weight_net).

CPU part (not marked gpu): the liveness conditions of every case, a float32 restatement of the oracle's gather warp
staying inside the bound on every element (the gate is not too tight), four simulated defects each putting >= 25 % of
the voxels outside it (the gate is not too loose), and the launcher's depth-chunk rule restated for the large cases.

Depth chunks (launch_k: dchunk = D, halved (rounding up) while dchunk > 2 and pixel blocks x B x chunks < 2048 blocks
of 256 threads). The small shape B = 3, D = 5, h = 20, w = 42 gives chunks of 2, 2, 1 planes at every lane count; the
large cases give

  bf16 C = 8  N = 3 adaptive       (one lane, runtime loop)   64 x 160, B = 4, D = 40: dchunk 3, last chunk 1 plane
  bf16 C = 16 N = 5 adaptive       (2 lanes, NVC = 4)         64 x 80,  B = 4, D = 40: dchunk 3, last chunk 1 plane
  fp32 C = 16 N = 7 variance       (4 lanes, NVC = 6)         64 x 80,  B = 2, D = 40: dchunk 3, last chunk 1 plane
  fp32 C = 32 N = 3 adaptive       (8 lanes, runtime loop)    64 x 80,  B = 2, D = 40: dchunk 5, last chunk 5 planes
  fp32 C = 16 N = 5 adaptive CBLOCK (one lane, NVC = 4)       64 x 160, B = 4, D = 40: dchunk 3, last chunk 1 plane

(test_large_cases_depth_chunks asserts this table from a restatement of the rule).

Measured on an MI355X, largest |got - ref| / bound per kernel family over the matrix, the warp-only and the large
cases (no constant of the model was raised; no kernel defect was found):

  lanes per voxel          fp32 adaptive   fp32 variance   bf16 adaptive   bf16 variance
  1 (warp_aggregate)           0.141           0.166           0.987           0.989
  2 (warp_split)               0.108           0.235           0.970           0.985
  4 (warp_split)               0.100           0.244           0.974           0.984
  8 (warp_split)               0.125           0.266             -               -
  warp-only (one lane)     fp32 0.171                      bf16 0.988

The bf16 figures sit just under 1 by construction: bf16 keeps 8 significand bits, so 2^-8 |ref| is exactly the
half-ulp of the round-to-nearest store and a correctly rounded voxel can use all of it; a truncating store would need
twice that. What remains of the bound is the fp32 model, of which the kernels use a quarter at most.
"""
import functools
import types

import numpy as np
import pytest
import torch

from conftest import rel_max
from common import model_state
from damvsnet_amd import synth
from oracle import mvs_oracle as O

DEV = "cuda"
U = 2.0 ** -24
BF16, F32 = torch.bfloat16, torch.float32
DT_IDS = {BF16: "bf16", F32: "f32"}
NMAX = 16                              # kMaxViews
SMALL = (3, 5, 20, 42)                 # B, D, h, w: w ragged for 32 / 16 / 8 / 4-column tiles, h for the 8-row tiles
MATRIX_N = (2, 3, 5, 7, 11, 15, 16)
CBLOCK_N = (4, 5)
PAD = 8                                # zero border of the reference's maps (samples are clamped to [-4, size + 3])

# Source view v of the synthetic rig sits at position VIEW_T[v] along synth.view_extrinsic's path (yaw 0.08 t rad,
# translation (-40, 5, 2) t mm; integer t is synth's view t). synth's own views 11 .. 15 keep less than half of their
# samples inside a 20 x 42 map, so the 15 source views are spread over |t| <= 4, where each of them keeps most samples
# inside the map and still sends real shares outside and across the border (test_liveness asserts the shares per view).
VIEW_T = (0.0, 1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 1.5, -1.5, 2.5, -2.5, 3.5, -3.5, 0.5, -0.5, 4.0)

@pytest.fixture(scope="module")
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from damvsnet_amd import build, _capi
    build.build()
    _capi.load_library()


# ---------------------------------------------------------------------------------------------- inputs

def _yaw(a):
    return np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])


def source_extrinsic(v, b):
    """World->camera 4x4 (float64) of source view v >= 1 of batch element b: synth.view_extrinsic at VIEW_T[v], then
    the per-sample change of test_gpu_parity._distinct_samples (extra yaw 0.01 b, translation x (1 + 0.15 b))."""
    t = VIEW_T[v]
    E = np.eye(4)
    E[:3, :3] = _yaw(0.01 * b) @ _yaw(0.08 * t)
    E[:3, 3] = np.array([-40.0 * t, 5.0 * t, 2.0 * t]) * (1.0 + 0.15 * b)
    return E


def map_intrinsics(h, w):
    """K of an h x w feature map: the DTU intrinsics rescaled, as synth.cameras gives a stage of that size."""
    return synth.stage1_intrinsics(4 * h, 4 * w)


def camera_pairs(B, N, h, w):
    """float32 (B, N, 2, 4, 4) projection pairs as the cascade hands them to damvs_proj_prepare."""
    P = np.zeros((B, N, 2, 4, 4))
    for b in range(B):
        for v in range(N):
            P[b, v, 0] = np.eye(4) if v == 0 else source_extrinsic(v, b)
            P[b, v, 1, :3, :3] = map_intrinsics(h, w)
    return P.astype(np.float32)


def compose_rt(B, N, h, w):
    """rt [B][N-1][12] = [R row-major | t] of P_src inv(P_ref), composed in float64 and rounded once to float32."""
    K = np.eye(4)
    K[:3, :3] = map_intrinsics(h, w)
    rt = np.zeros((B, N - 1, 12))
    for b in range(B):
        for v in range(1, N):
            M = K @ source_extrinsic(v, b) @ np.linalg.inv(K)   # the reference camera is the identity
            rt[b, v - 1, :9] = M[:3, :3].reshape(9)
            rt[b, v - 1, 9:] = M[:3, 3]
    return rt.astype(np.float32)


def fold_bn(weight, bias, mean, var, eps):
    """weight_pack.h bn_affine, operation for operation (double arithmetic, one rounding to float32 per value)."""
    inv = 1.0 / np.sqrt(np.float64(np.float32(var)) + np.float64(np.float32(eps)))
    w, b, m = (np.float64(np.float32(t)) for t in (weight, bias, mean))
    return np.float32(inv * w), np.float32(b - m * inv * w)


# weight net per C: (sum of k1, BatchNorm 1 scale, shift, BatchNorm 2 scale, shift). k1 ~ U(-1, 1) with both signs,
# scales > 0, shifts < 0 (the issue's probe values). x_c = (ref_c - s_c)^2 >= 0, so the sum of k1 decides where the
# dot product sits against the first ReLU: the seeded draw is recentred to a fixed sum, which keeps both ReLUs live and
# dead on 20 .. 80 % of the (voxel, view) pairs at every C (test_liveness) without a shift tuned to one draw.
WEIGHT_NET = {C: (0.5, 0.35, -0.1, 0.8, -0.2) for C in (8, 16, 32)}


@functools.lru_cache(maxsize=None)
def weight_net(C):
    """(AggWeightNetVolume with the test's parameters, the folded float32 operands k1, s1, t1, s2, t2 of the kernel)."""
    from damvsnet_amd.layers import AggWeightNetVolume
    ksum, g1, b1, g2, b2 = WEIGHT_NET[C]
    k1 = synth._rng(7, C).uniform(-1.0, 1.0, C)
    k1 = (0.8 * (k1 - k1.mean()) + ksum / C).astype(np.float32)   # x_c >= 0: sum k1 places the dot product's centre
    assert (k1 > 0).any() and (k1 < 0).any() and np.abs(k1).max() <= 1.0
    net = AggWeightNetVolume(C)
    with torch.no_grad():
        for m, k, g, b in ((net.w_net[0], torch.from_numpy(k1), g1, b1), (net.w_net[1], torch.ones(1), g2, b2)):
            m.conv.weight.copy_(k.reshape(m.conv.weight.shape))
            m.bn.weight.fill_(g)
            m.bn.bias.fill_(b)
            m.bn.running_mean.zero_()
            m.bn.running_var.fill_(1.0)
    bn1, bn2 = net.w_net[0].bn, net.w_net[1].bn
    s1, t1 = fold_bn(bn1.weight.item(), bn1.bias.item(), 0.0, 1.0, bn1.eps)
    sc2, t2 = fold_bn(bn2.weight.item(), bn2.bias.item(), 0.0, 1.0, bn2.eps)
    s2 = np.float32(np.float32(1.0) * sc2)
    assert s1 > 0 and s2 > 0 and t1 < 0 and t2 < 0
    return net.eval(), types.SimpleNamespace(k1=k1, s1=s1, t1=t1, s2=s2, t2=t2)


def model_weight_net(C, sd, stage):
    """Folded operands of the weight net of a reference-keyed state_dict (the suite's shared synthetic weights)."""
    p = "DepthNet.weight_net.%d.w_net." % stage
    f = lambda i: fold_bn(*(float(sd[p + "%d.bn.%s" % (i, n)]) for n in ("weight", "bias", "running_mean",  # noqa: E731
                                                                      "running_var")), O.BN_EPS)
    s1, t1 = f(0)
    sc2, t2 = f(1)
    k1 = sd[p + "0.conv.weight"].reshape(C).numpy().astype(np.float32)
    return types.SimpleNamespace(k1=k1, s1=s1, t1=t1, s2=np.float32(np.float32(float(sd[p + "1.conv.weight"])) * sc2),
                                 t2=t2)


@functools.lru_cache(maxsize=None)
def fixture(C, bf16, shape=SMALL, nviews=NMAX):
    """Inputs of one (C, storage type, shape): nviews seeded N(0, 1) maps [B][h][w][C] rounded to the storage type, rt
    for nviews views and the hypotheses, all distinct per batch element. A case at N views uses the first N maps and
    the first N - 1 cameras."""
    B, D, h, w = shape
    f = synth._rng(11, C, h, w).standard_normal((nviews, B, h, w, C), dtype=np.float32)
    ft = torch.from_numpy(f)
    if bf16:
        ft = ft.to(BF16).float()
    scale = 1.0 + 0.02 * np.arange(B, dtype=np.float64).reshape(B, 1, 1, 1)
    hyps = (synth.stage_hypotheses(B, D, h, w, seed=3).astype(np.float64) * scale).astype(np.float32)
    fx = types.SimpleNamespace(C=C, bf16=bf16, B=B, D=D, h=h, w=w, nviews=nviews, feats=ft.numpy(), hyps=hyps,
                               rt=compose_rt(B, nviews, h, w), cache={}, maps={})
    return fx


# ---------------------------------------------------------------------------------------------- float64 reference

def _padded(fx, v, b):
    """Zero-padded float64 map of view v, batch element b, flattened to [(h + 2 PAD)(w + 2 PAD)][C], with the window
    maxima of its neighbour differences: gx[y0, x0] = max |f[r, j+1] - f[r, j]| over rows y0-1 .. y0+2 and columns
    j = x0-1 .. x0+1 (all horizontal differences inside columns x0-1 .. x0+2); gy the transpose of that."""
    key = (v, b)
    if key not in fx.maps:
        f = np.pad(fx.feats[v, b].astype(np.float64), ((PAD, PAD), (PAD, PAD), (0, 0)))
        H, W, C = f.shape
        dh = np.zeros_like(f)
        dh[:, :-1] = np.abs(f[:, 1:] - f[:, :-1])      # dh[r, j]: difference between columns j and j + 1
        dv = np.zeros_like(f)
        dv[:-1] = np.abs(f[1:] - f[:-1])
        sh = lambda a, dy, dx: np.roll(a, (-dy, -dx), (0, 1))  # noqa: E731  a[y + dy, x + dx]; the border is zero
        gx = functools.reduce(np.maximum, [sh(dh, dy, dx) for dy in (-1, 0, 1, 2) for dx in (-1, 0, 1)])
        gy = functools.reduce(np.maximum, [sh(dv, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1, 2)])
        if len(fx.maps) >= 24:
            fx.maps.clear()
        fx.maps[key] = tuple(a.reshape(H * W, C) for a in (f, gx, gy))
    return fx.maps[key]


def sample_view(fx, v, b, ys, xs, hyp, cam_b=None):
    """Source view v >= 1 sampled for the reference pixels (ys, xs) of batch element b at hypotheses hyp [D][P], with
    the camera of batch element cam_b (default b). Returns (s, ds, corners): the float64 samples [D][P][C], their
    uncertainty, and the number of bilinear corners inside the map [D][P]."""
    h, w = fx.h, fx.w
    m = fx.rt[b if cam_b is None else cam_b, v - 1].astype(np.float64)
    x, y = xs.astype(np.float64), ys.astype(np.float64)
    hyp = hyp.astype(np.float64)
    q, Eq = [], []
    for i in range(3):
        r = m[3 * i] * x + m[3 * i + 1] * y + m[3 * i + 2]
        Er = 4 * U * (np.abs(m[3 * i] * x) + np.abs(m[3 * i + 1] * y) + abs(m[3 * i + 2]))
        q.append(r[None] * hyp + m[9 + i])
        Eq.append(Er[None] * np.abs(hyp) + 2 * U * (np.abs(r[None] * hyp) + abs(m[9 + i])))
    assert (q[2] > 0).all()   # every hypothesis lies in front of every source camera
    kx, ky = w / (w - 1.0), h / (h - 1.0)
    px, py = q[0] / q[2], q[1] / q[2]
    ix, iy = px * kx - 0.5, py * ky - 0.5
    dx = kx * (Eq[0] + np.abs(px) * Eq[2]) / np.abs(q[2]) + 8 * U * (np.abs(px) * kx + 1)
    dy = ky * (Eq[1] + np.abs(py) * Eq[2]) / np.abs(q[2]) + 8 * U * (np.abs(py) * ky + 1)
    inside = (ix > -2) & (ix < w + 1) & (iy > -2) & (iy < h + 1)   # outside: 0, which is plain zero padding
    cx, cy = np.where(inside, ix, -4.0), np.where(inside, iy, -4.0)
    x0f, y0f = np.floor(cx), np.floor(cy)
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    wx1, wy1 = cx - x0f, cy - y0f
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1
    f, gx, gy = _padded(fx, v, b)
    Wp = w + 2 * PAD
    base = (y0 + PAD) * Wp + (x0 + PAD)
    s = absum = 0.0
    corners = np.zeros(ix.shape, np.int64)
    for dyk, dxk, wk in ((0, 0, wx0 * wy0), (0, 1, wx1 * wy0), (1, 0, wx0 * wy1), (1, 1, wx1 * wy1)):
        t = wk[..., None] * np.take(f, base + dyk * Wp + dxk, axis=0)
        s = s + t
        absum = absum + np.abs(t)
        corners += ((x0 + dxk >= 0) & (x0 + dxk < w) & (y0 + dyk >= 0) & (y0 + dyk < h))
    ds = dx[..., None] * np.take(gx, base, axis=0) + dy[..., None] * np.take(gy, base, axis=0) + 6 * U * absum
    return s, ds, corners


def _pixels(fx, pixels):
    if pixels is None:
        ys, xs = np.divmod(np.arange(fx.h * fx.w), fx.w)
        return [(ys, xs)] * fx.B
    return pixels


def _view(fx, v, b, ys, xs, full, hyp_shift=0, cam_b=None):
    """sample_view at the fixture's own hypotheses (plane d reads plane min(d + hyp_shift, D - 1)); the defect-free
    full-map result is kept, since every N and mode of the small matrix reuses it."""
    key = (v, b)
    plain = full and hyp_shift == 0 and cam_b is None
    if plain and key in fx.cache:
        return fx.cache[key]
    hyp = fx.hyps[b][:, ys, xs]
    if hyp_shift:
        hyp = hyp[np.minimum(np.arange(fx.D) + hyp_shift, fx.D - 1)]
    out = sample_view(fx, v, b, ys, xs, hyp, cam_b)
    if plain:
        fx.cache[key] = out
    return out


def reference(fx, N, mode, net=None, pixels=None, defect=None):
    """float64 reference and per-element bound of the N-view aggregation of fixture fx.

    mode: "adaptive" (net: the folded weight net), "variance" or "warp" (N = 2: the sample of view 1 itself).
    pixels: None (the whole map: ref, bound are [B][D][h][w][C]) or one (ys, xs) per batch element (lists of
    [D][P][C] arrays: all D planes of each listed pixel). defect: None, or one of the simulated kernel defects
    "next_plane_hyp" (the last view reads the next plane's hypothesis), "next_batch_cam" (the first source view uses
    the next batch element's camera), "half_channels" (the weight net sees only the first C/2 channels),
    "divisor_n" (adaptive: / N instead of / (N-1)), "no_weight" (wv = 1).
    Returns (ref, bound, stats); stats holds the liveness counts."""
    C, D = fx.C, fx.D
    full = pixels is None
    refs, bounds = [], []
    st = types.SimpleNamespace(a1_live=0, wv_live=0, pairs=0, corners=np.zeros((N, 3)))   # per view: none / some / all 4
    for b, (ys, xs) in enumerate(_pixels(fx, pixels)):
        r = fx.feats[0, b][ys, xs].astype(np.float64)[None]    # [1][P][C]
        views = []
        for v in range(1, N):
            s, ds, corners = _view(fx, v, b, ys, xs, full,
                                   hyp_shift=1 if defect == "next_plane_hyp" and v == N - 1 else 0,
                                   cam_b=(b + 1) % fx.B if defect == "next_batch_cam" and v == 1 else None)
            views.append((s, ds))
            st.corners[v] += ((corners == 0).sum(), ((corners > 0) & (corners < 4)).sum(), (corners == 4).sum())
        if mode == "warp":
            (out, dout), = views
        elif mode == "variance":
            tot = r + sum(s for s, _ in views)
            sq = r * r + sum(s * s for s, _ in views)
            dsum = sum(ds for _, ds in views) + (N + 1) * U * (np.abs(r) + sum(np.abs(s) for s, _ in views))
            dsq = sum(2 * np.abs(s) * ds + ds * ds for s, ds in views)
            mean = tot / N
            out = sq / N - mean * mean
            dout = dsq / N + 2 * np.abs(mean) * dsum / N + (dsum / N) ** 2 + 6 * U * (sq / N + mean * mean)
        else:
            k1 = net.k1.astype(np.float64).copy()
            if defect == "half_channels":
                k1[C // 2:] = 0.0
            s1, t1, s2, t2 = (float(t) for t in (net.s1, net.t1, net.s2, net.t2))
            acc = dacc = 0.0
            for s, ds in views:
                df = r - s
                x = df * df
                dxc = 2 * np.abs(df) * ds + ds * ds + 4 * U * x
                dot = (k1 * x).sum(-1, keepdims=True)
                ddot = (np.abs(k1) * dxc).sum(-1, keepdims=True) + (C + 2) * U * np.abs(k1 * x).sum(-1, keepdims=True)
                a1 = np.maximum(dot * s1 + t1, 0.0)
                da1 = abs(s1) * ddot + 3 * U * (np.abs(dot * s1) + abs(t1))
                wv = np.maximum(a1 * s2 + t2, 0.0) + 1.0
                dwv = abs(s2) * da1 + 3 * U * (np.abs(a1 * s2) + abs(t2) + 1)
                st.a1_live += int((a1 > 0).sum())
                st.wv_live += int((wv > 1).sum())
                st.pairs += a1.size
                if defect == "no_weight":
                    wv = np.ones_like(wv)
                acc = acc + wv * x
                dacc = dacc + dwv * x + wv * dxc + 3 * U * wv * x
            div = N if defect == "divisor_n" else N - 1
            out = acc / div
            dout = dacc / (N - 1) + (N + 2) * U * acc / (N - 1)
        if fx.bf16:
            dout = dout + 2.0 ** -8 * (np.abs(out) + dout)
        refs.append(out)
        bounds.append(dout)
    if full:
        shape = (fx.B, D, fx.h, fx.w, C)
        return np.stack(refs).reshape(shape), np.stack(bounds).reshape(shape), st
    return refs, bounds, st


def bound_ratio(got, ref, bound):
    """max |got - ref| / bound (float64); got in the storage type's values."""
    return float(ratios(got, ref, bound).max())


def ratios(got, ref, bound):
    """|got - ref| / bound per element; where the bound is 0 (every corner of every view outside the map: the exact
    result is 0 in any arithmetic) 0 for an equal element and inf for any other, so "<= 1" is "|got - ref| <= bound"."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))


# ---------------------------------------------------------------------------------------------- float32 restatement

def restate_f32(fx, N, mode, net=None):
    """The oracle's arithmetic (mvs_oracle.homo_warping impl="gather", aggregate) in float32 torch ops on the same rt:
    an independent float32 evaluation that the bound has to admit. Returns [B][D][h][w][C] in the storage type."""
    B, D, h, w, C = fx.B, fx.D, fx.h, fx.w, fx.C
    key = "f32"
    if key not in fx.cache:
        y, x = torch.meshgrid(torch.arange(h, dtype=F32), torch.arange(w, dtype=F32), indexing="ij")
        xyz = torch.stack((x.reshape(-1), y.reshape(-1), torch.ones(h * w)))
        warped = {}
        for v in range(1, fx.nviews):
            rt = torch.from_numpy(fx.rt[:, v - 1])
            rot_xyz = torch.matmul(rt[:, :9].reshape(B, 3, 3), xyz)                           # [B][3][hw]
            p = rot_xyz.unsqueeze(2) * torch.from_numpy(fx.hyps).reshape(B, 1, D, -1) + rt[:, 9:].reshape(B, 3, 1, 1)
            gx = p[:, 0] / p[:, 2] / ((w - 1) / 2) - 1
            gy = p[:, 1] / p[:, 2] / ((h - 1) / 2) - 1
            ix, iy = ((gx + 1) * w - 1) / 2, ((gy + 1) * h - 1) / 2
            src = torch.from_numpy(fx.feats[v]).permute(0, 3, 1, 2)
            warped[v] = O.bilinear_zeros(src, ix.reshape(B, -1), iy.reshape(B, -1)).reshape(B, C, D, h, w)
        fx.cache[key] = warped
    warped = fx.cache[key]
    ref = torch.from_numpy(fx.feats[0]).permute(0, 3, 1, 2).unsqueeze(2)                        # [B][C][1][h][w]
    if mode == "warp":
        out = warped[1]
    elif mode == "variance":
        vsum, vsq = ref.expand(B, C, D, h, w), ref ** 2
        for v in range(1, N):
            vsum = vsum + warped[v]
            vsq = vsq + warped[v] ** 2
        out = vsq / N - (vsum / N) ** 2
    else:
        k1 = torch.from_numpy(net.k1).reshape(1, C, 1, 1, 1)
        acc = None
        for v in range(1, N):
            xx = (ref - warped[v]) ** 2
            a1 = torch.relu((xx * k1).sum(1, keepdim=True) * float(net.s1) + float(net.t1))
            wgt = torch.relu(a1 * float(net.s2) + float(net.t2))
            acc = (wgt + 1) * xx if acc is None else acc + (wgt + 1) * xx
        out = acc / (N - 1)
    out = out.permute(0, 2, 3, 4, 1).contiguous()
    return out.to(BF16) if fx.bf16 else out


# ---------------------------------------------------------------------------------------------- cases

def lanes_per_voxel(C, bf16, N, blocked=False):
    """k_warp.hip launch_k's lane count: the channel-split kernel for NHWC maps of 2 / 4 / 8 16-byte chunks per pixel at odd
    N >= 3, else one lane per voxel."""
    S = C * (2 if bf16 else 4) // 16
    return S if (not blocked and S in (2, 4, 8) and N >= 3 and N % 2 == 1) else 1


def depth_chunks(B, D, h, w, lanes, rows=None):
    """k_warp.hip launch_k restated (tiles: warp_tiles.h): (dchunk, planes of the last chunk)."""
    rows = h if rows is None else rows
    tc = 256 // lanes // 8
    npb = -(-w // tc) * -(-rows // 8)
    dchunk = D
    while dchunk > 2 and npb * B * -(-D // dchunk) < 2048:
        dchunk = (dchunk + 1) // 2
    return dchunk, D - (-(-D // dchunk) - 1) * dchunk


# (C, bf16, mode, N, blocked) of the small matrix, grouped by (C, bf16) so that one fixture's samples serve its cases
MATRIX = [(C, bf16, mode, N, blocked)
          for bf16 in (False, True) for C in (8, 16, 32) for mode in ("adaptive", "variance")
          for N, blocked in [(n, False) for n in MATRIX_N] + [(n, True) for n in CBLOCK_N]]
WARP_ONLY = [(C, bf16) for bf16 in (False, True) for C in (8, 16, 32)]


def case_id(c):
    C, bf16, mode, N, blocked = c
    return "%s-C%d-%s-N%d%s" % ("bf16" if bf16 else "f32", C, mode, N, "-cblock" if blocked else "")


# (C, bf16, mode, N, blocked, (B, D, h, w), lanes, dchunk, last chunk): the depth pipeline beyond two planes
LARGE = [(8, True, "adaptive", 3, False, (4, 40, 64, 160), 1, 3, 1),
         (16, True, "adaptive", 5, False, (4, 40, 64, 80), 2, 3, 1),
         (16, False, "variance", 7, False, (2, 40, 64, 80), 4, 3, 1),
         (32, False, "adaptive", 3, False, (2, 40, 64, 80), 8, 5, 5),
         (16, False, "adaptive", 5, True, (4, 40, 64, 160), 1, 3, 1)]


def large_pixels(shape, seed):
    """Per batch element a seeded pixel subset, at least 8192 (b, y, x) in all: the four corners, the last row and
    the last column, and random pixels."""
    B, D, h, w = shape
    rng = synth._rng(seed, h, w)
    out = []
    for b in range(B):
        edge = np.concatenate([(h - 1) * w + np.arange(w), np.arange(h) * w + (w - 1), [0, w - 1]])
        p = np.union1d(edge, rng.choice(h * w, size=-(-8192 // B), replace=False))
        out.append(tuple(np.divmod(p, w)))
    assert sum(len(ys) for ys, _ in out) >= 8192
    return out


# ---------------------------------------------------------------------------------------------- CPU tests

def test_source_views_follow_synth():
    """VIEW_T at an integer t is synth's view t, and rt is the composition of the same float64 cameras."""
    for v, t in enumerate(VIEW_T):
        if v and t == int(t) and t > 0:
            assert np.allclose(source_extrinsic(v, 0), synth.view_extrinsic(int(t)), rtol=0, atol=1e-12)
    assert len(set(VIEW_T)) == NMAX and VIEW_T[0] == 0.0
    rt = compose_rt(3, NMAX, 20, 42)
    assert rt.dtype == np.float32 and rt.shape == (3, NMAX - 1, 12)
    assert len({rt[b, v].tobytes() for b in range(3) for v in range(NMAX - 1)}) == 3 * (NMAX - 1)   # all distinct


@pytest.mark.parametrize("C,bf16", WARP_ONLY, ids=["%s-C%d" % ("bf16" if b else "f32", C) for C, b in WARP_ONLY])
def test_liveness(C, bf16):
    """Conditions on the inputs of every small case (conditions, not measurements): both ReLUs of the weight net live
    on 20 .. 80 % of the (voxel, view) pairs; per source view >= 2 % of the samples with all four corners outside
    the map, >= 2 % with one to three corners inside, >= 50 % fully inside."""
    fx = fixture(C, bf16)
    for N in MATRIX_N + CBLOCK_N:
        _, _, st = reference(fx, N, "adaptive", weight_net(C)[1])
        a1, wv = st.a1_live / st.pairs, st.wv_live / st.pairs
        assert 0.2 <= a1 <= 0.8 and 0.2 <= wv <= 0.8, (C, N, a1, wv)
        share = st.corners[1:] / st.corners[1:].sum(1, keepdims=True)
        assert (share[:, 0] >= 0.02).all() and (share[:, 1] >= 0.02).all() and (share[:, 2] >= 0.5).all(), (N, share)
    # the large cases run the same weight nets and views on other maps
    for c in LARGE:
        if (c[0], c[1]) == (C, bf16) and c[2] == "adaptive":
            lf = fixture(C, bf16, c[5], c[3])
            px = [(ys[::16], xs[::16]) for ys, xs in large_pixels(c[5], 1)]
            _, _, st = reference(lf, c[3], "adaptive", weight_net(C)[1], pixels=px)
            assert 0.2 <= st.a1_live / st.pairs <= 0.8 and 0.2 <= st.wv_live / st.pairs <= 0.8


@pytest.mark.parametrize("C,bf16", WARP_ONLY, ids=["%s-C%d" % ("bf16" if b else "f32", C) for C, b in WARP_ONLY])
def test_float32_restatement_within_bound(C, bf16):
    """The gate is not too tight: an independent float32 evaluation (the oracle's gather warp and aggregation in
    float32 torch ops on the same rt) stays inside the bound on every element of every small case."""
    fx = fixture(C, bf16)
    net = weight_net(C)[1]
    worst = 0.0
    for mode, N in [("warp", 2)] + [(m, n) for m in ("adaptive", "variance") for n in sorted(MATRIX_N + CBLOCK_N)]:
        ref, bound, _ = reference(fx, N, mode, net)
        r = bound_ratio(restate_f32(fx, N, mode, net).float().numpy(), ref, bound)
        worst = max(worst, r)
        assert r <= 1.0, (C, bf16, mode, N, r)
    print("float32 restatement C=%d %s: max |got - ref| / bound %.3f" % (C, "bf16" if bf16 else "f32", worst))


@pytest.mark.parametrize("C,bf16,N", [(8, True, 3), (16, True, 5), (16, False, 7), (32, False, 3), (32, True, 16)])
def test_simulated_defects_are_caught(C, bf16, N):
    """The gate is not too loose: each defect, applied to the float64 reference, puts >= 25 % of the voxels (a voxel
    counts when any of its channels does) beyond the bound."""
    fx = fixture(C, bf16)
    net = weight_net(C)[1]
    ref, bound, _ = reference(fx, N, "adaptive", net)
    for defect in ("next_plane_hyp", "next_batch_cam", "half_channels", "divisor_n", "no_weight"):
        bad, _, _ = reference(fx, N, "adaptive", net, defect=defect)
        planes = slice(0, fx.D - 1) if defect == "next_plane_hyp" else slice(None)   # the last plane has no next one
        share = float((np.abs(bad - ref) > bound).any(-1)[:, planes].mean())
        assert share >= 0.25, (defect, share)
    rv, bv, _ = reference(fx, N, "variance")
    for defect in ("next_plane_hyp", "next_batch_cam"):
        bad, _, _ = reference(fx, N, "variance", defect=defect)
        planes = slice(0, fx.D - 1) if defect == "next_plane_hyp" else slice(None)
        share = float((np.abs(bad - rv) > bv).any(-1)[:, planes].mean())
        assert share >= 0.25, ("variance", defect, share)


def test_old_metric_misses_the_dead_weight_net():
    """Why the file brings its own weight net: with the suite's shared synthetic weights the 16-channel (stage-2)
    weight net is 0 on every voxel, so a kernel without it (wv = 1) has rel_max exactly 0 against the reference; with
    this file's weight net the same defect leaves the bound."""
    fx = fixture(16, False)
    old = model_weight_net(16, model_state("depthnet_cfgA_adaptive"), 1)
    for N in (3, 5):
        ref, _, st = reference(fx, N, "adaptive", old)
        bad, _, _ = reference(fx, N, "adaptive", old, defect="no_weight")
        assert st.wv_live == 0 and rel_max(bad, ref) == 0.0
        ref, bound, _ = reference(fx, N, "adaptive", weight_net(16)[1])
        bad, _, _ = reference(fx, N, "adaptive", weight_net(16)[1], defect="no_weight")
        assert float((np.abs(bad - ref) > bound).any(-1).mean()) >= 0.25


def test_large_cases_depth_chunks():
    """The large cases reach the depth chunks the docstring states, under the launcher's rule as it stands; the small
    shape gives chunks of 2, 2 and 1 planes at every lane count."""
    for C, bf16, mode, N, blocked, shape, lanes, dchunk, last in LARGE:
        assert lanes_per_voxel(C, bf16, N, blocked) == lanes
        assert depth_chunks(*shape, lanes) == (dchunk, last), (C, bf16, N, depth_chunks(*shape, lanes))
        assert dchunk > 2
    for lanes in (1, 2, 4, 8):
        assert depth_chunks(*SMALL, lanes) == (2, 1)
    assert {lanes_per_voxel(C, bf16, N, blocked) for C, bf16, _, N, blocked in MATRIX} == {1, 2, 4, 8}


# ---------------------------------------------------------------------------------------------- GPU tests

@functools.lru_cache(maxsize=None)
def engine(C, mode, dtype):
    from damvsnet_amd.engine import StageEngine
    from damvsnet_amd.layers import CostRegNet
    torch.manual_seed(C)
    return StageEngine(CostRegNet(C, 8), weight_net(C)[0] if mode == "adaptive" else None, mode, dtype,
                       torch.device(DEV))


def device_inputs(fx, N, blocked=False):
    from damvsnet_amd.engine import block_channels
    dt = BF16 if fx.bf16 else F32
    feats = [torch.from_numpy(fx.feats[v]).to(DEV, dt).contiguous() for v in range(N)]
    if blocked:
        feats = block_channels(feats)
    rt = torch.from_numpy(np.ascontiguousarray(fx.rt[:, :N - 1])).to(DEV)
    return feats, rt, torch.from_numpy(fx.hyps).to(DEV)


def run_aggregate(fx, N, mode, blocked=False):
    from damvsnet_amd import _capi
    feats, rt, hyps = device_inputs(fx, N, blocked)
    eng = engine(fx.C, mode, BF16 if fx.bf16 else F32)
    layout = _capi.DAMVS_LAYOUT_CBLOCK if blocked else _capi.DAMVS_LAYOUT_NHWC
    return eng.warp_aggregate(feats, None, hyps, rt=rt, layout=layout)


def family(C, bf16, mode, N, blocked=False):
    return "%d-lane %s %s" % (lanes_per_voxel(C, bf16, N, blocked), "bf16" if bf16 else "fp32", mode)


def assert_within_bound(got, ref, bound, what, fam):
    """|got - ref| <= bound on every element; prints the largest ratio (the per-family figure of the docstring)."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    ratio = ratios(got, ref, bound)
    worst = float(ratio.max())
    print("warp bound [%s] %s: max |got - ref| / bound = %.4f" % (fam, what, worst))
    if not worst <= 1.0:   # also catches NaN
        bad = np.argwhere(~(ratio <= 1.0))
        lines = ["%s: %d of %d elements beyond the bound (largest ratio %.3f)" % (what, len(bad), ratio.size, worst)]
        for idx in bad[:8]:
            i = tuple(idx)
            lines.append("  %s: got %r ref %r bound %.3e" % (i, float(got[i]), float(ref[i]), float(bound[i])))
        pytest.fail("\n".join(lines))


@pytest.mark.gpu
@pytest.mark.parametrize("case", MATRIX, ids=[case_id(c) for c in MATRIX])
def test_warp_aggregate_within_bound(case, _lib):
    """Every dispatch row of launch_k at the small shape, NHWC at N = 2 .. 16 and channel-blocked maps at N = 4, 5,
    against the float64 reference: each element within its bound."""
    C, bf16, mode, N, blocked = case
    fx = fixture(C, bf16)
    ref, bound, _ = reference(fx, N, mode, weight_net(C)[1])
    got = run_aggregate(fx, N, mode, blocked).float().cpu().numpy()
    assert_within_bound(got, ref, bound, case_id(case), family(C, bf16, mode, N, blocked))


@pytest.mark.gpu
@pytest.mark.parametrize("C,bf16", WARP_ONLY, ids=["%s-C%d" % ("bf16" if b else "f32", C) for C, b in WARP_ONLY])
def test_homo_warp_within_bound(C, bf16, _lib):
    """damvs_homo_warp (the warp-only mode of the one-lane kernel) on view 1's map: each element within the sample
    bound."""
    from damvsnet_amd import _capi
    from damvsnet_amd._capi import check, ptr
    from damvsnet_amd.engine import DTYPES
    fx = fixture(C, bf16)
    dt = BF16 if bf16 else F32
    feats, rt, hyps = device_inputs(fx, 2)
    out = torch.empty(fx.B, fx.D, fx.h, fx.w, C, device=DEV, dtype=dt)
    lib = _capi.load_library()
    check(lib.damvs_homo_warp(_capi.stream_ptr(torch.device(DEV)), DTYPES[dt], fx.B, C, fx.D, fx.h, fx.w, ptr(feats[1]),
                              ptr(rt), ptr(hyps), ptr(out)))
    ref, bound, _ = reference(fx, 2, "warp")
    assert_within_bound(out.float().cpu().numpy(), ref, bound, "homo_warp C=%d %s" % (C, DT_IDS[dt]),
                        "1-lane %s warp-only" % ("bf16" if bf16 else "fp32"))


@pytest.mark.gpu
@pytest.mark.parametrize("case", LARGE, ids=[case_id(c[:5]) for c in LARGE])
def test_depth_pipeline_beyond_two_planes(case, _lib):
    """Depth chunks of 3 and 5 planes (the two-planes-ahead hypothesis pipeline without its clamp, and a one-plane
    last chunk): all D planes of a seeded pixel subset (corners, last row, last column included), indexed on the
    device, each element within its bound."""
    C, bf16, mode, N, blocked, shape, lanes, dchunk, last = case
    fx = fixture(C, bf16, shape, N)
    px = large_pixels(shape, C + N)
    vol = run_aggregate(fx, N, mode, blocked)
    got = [vol[b][:, torch.from_numpy(ys).to(DEV), torch.from_numpy(xs).to(DEV)].float().cpu().numpy()
           for b, (ys, xs) in enumerate(px)]
    ref, bound, _ = reference(fx, N, mode, weight_net(C)[1], pixels=px)
    assert_within_bound(np.concatenate(got, 1), np.concatenate(ref, 1), np.concatenate(bound, 1),
                        "large " + case_id(case[:5]), family(C, bf16, mode, N, blocked))


@pytest.mark.gpu
@pytest.mark.parametrize("C,bf16,N", [(16, False, 5), (8, True, 3)], ids=["f32-split4", "bf16-one-lane"])
def test_row_slab_is_bitwise_the_full_call(C, bf16, N, _lib):
    """warp_aggregate_rows on rows 5 .. 11 of 20, written to rows 2 .. 8 of an 11-row buffer: bitwise the full call's
    rows, and every other row of the buffer untouched."""
    fx = fixture(C, bf16)
    dt = BF16 if bf16 else F32
    B, D, h, w = SMALL
    y0, rows, out_rows, out_y = 5, 7, 11, 2
    feats, rt, hyps = device_inputs(fx, N)
    full = run_aggregate(fx, N, "adaptive")
    sentinel = -12345.0   # a bf16 value no voxel takes
    out = torch.full((B, D, out_rows, w, C), sentinel, device=DEV, dtype=dt)
    slab_hyps = torch.full((B, D, out_rows, w), float("nan"), device=DEV)
    slab_hyps[:, :, out_y:out_y + rows] = hyps[:, :, y0:y0 + rows]
    engine(C, "adaptive", dt).warp_aggregate_rows(feats, rt, slab_hyps, h, y0, rows, out_y, out)
    assert torch.equal(out[:, :, out_y:out_y + rows], full[:, :, y0:y0 + rows])
    assert bool((out[:, :, :out_y] == sentinel).all()) and bool((out[:, :, out_y + rows:] == sentinel).all())
    assert not bool((full == sentinel).any())


def ulp32(x):
    """Spacing of float32 at |x| (float64 array), the smallest normal's spacing below it."""
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -126)))
    return 2.0 ** (e - 23)


def proj_prepare_reference(P):
    """float64 P_src inv(P_ref) of float32 pairs (B, N, 2, 4, 4), with P = [K E[:3, :4]; E[3]] rounded to float32 as
    the reference composes it (models/cas_mvsnet.py:44-47) and as proj_prepare_kernel does. Returns [B][N-1][12]."""
    B, N = P.shape[:2]
    P = P.astype(np.float64)
    comp = P[:, :, 0].copy()
    comp[:, :, :3, :4] = (P[:, :, 1, :3, :3] @ P[:, :, 0, :3, :4]).astype(np.float32)
    out = np.zeros((B, N - 1, 12))
    for b in range(B):
        inv = np.linalg.inv(comp[b, 0])
        for v in range(1, N):
            M = comp[b, v] @ inv
            out[b, v - 1, :9] = M[:3, :3].reshape(9)
            out[b, v - 1, 9:] = M[:3, 3]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("N", [2, 5, 16])
def test_proj_prepare_within_two_ulps(N, _lib):
    """damvs_proj_prepare (double arithmetic, one rounding) on distinct per-batch cameras: each of the 12 entries
    within 2 float32 ulps of the float64 numpy value."""
    from damvsnet_amd.engine import proj_prepare
    P = camera_pairs(3, N, 20, 42)
    want = proj_prepare_reference(P)
    got = proj_prepare(torch.from_numpy(P).to(DEV)).cpu().numpy().astype(np.float64)
    err = np.abs(got - want) / ulp32(want)
    print("proj_prepare N=%d: max error %.3f ulp" % (N, err.max()))
    assert got.shape == want.shape and (err <= 2.0).all(), np.argwhere(err > 2.0)[:8]
