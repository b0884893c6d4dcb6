"""Exact-arithmetic per-layer tests: the bf16 and fp32 convolution kernels against float64 references on inputs
on which nothing rounds, so the gate is equality per element.

Every product kernel accumulates in fp32 (bf16 MFMA, split-f16 MFMA, VALU FMAs). With activations in {0, +-1, +-2}
and weights in {0, +-0.5, +-1} every product and every partial sum, in any order, is exact in fp32; the bf16
conversions of inputs and weights are the identity; the fp32 path's f16 split has lo = 0; the power-of-two weight
scale and activation prescale are exact. Where the exact output is itself bf16-representable the store is the
identity too, so a kernel must equal the float64 reference bit for bit, and a dropped or misplaced tap moves an
element by at least 0.5 (test_one_dropped_tap_passes_rel_max_but_not_equality shows the old global-norm gate
missing exactly that).

CPU part (not marked gpu): test_lattice_fixtures_are_exact proves, for every case the GPU tests use, the
conditions that make "equal" the right gate; the GPU tests then run the same cached fixtures.
"""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import route_cases
from conftest import rel_max
from test_gpu_frontend import CASES as CONV2D_CASES

DEV = "cuda"
ACT = (-2.0, -1.0, 1.0, 2.0)     # activations, planes, residuals, skips
WGT = (-1.0, -0.5, 0.5, 1.0)     # conv weights, biases
BF16, F32 = torch.bfloat16, torch.float32
B = 2


@pytest.fixture(scope="module")
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from damvsnet_amd import build, _capi
    build.build()
    _capi.load_library()


# ---------------------------------------------------------------------------------------------- fixture helpers

def lattice(shape, values, density, gen):
    """float64 tensor of `shape`: each element is 0 with probability 1 - density, else a uniform draw from `values`."""
    v = torch.tensor(values, dtype=torch.float64)
    t = v[torch.randint(len(values), tuple(shape), generator=gen)]
    return t * (torch.rand(tuple(shape), generator=gen) < density)


def upsample(t, u):
    """nearest-neighbour x u over the two last dims (exact in any dtype)."""
    return t if u <= 1 else t.repeat_interleave(u, -2).repeat_interleave(u, -1)


def layer_reference(acc, scale=None, shift=None, res_pre=None, relu=True, res_post=None, post_up=1):
    """float64 reference of one fused layer from its convolution sum `acc` [B][C][...]: per-channel scale and shift
    (folded BatchNorm or bias), residual before the ReLU, ReLU, residual after it (nearest-upsampled by post_up).
    Returns (output, pre-activation)."""
    assert acc.dtype == torch.float64
    cshape = (1, -1) + (1,) * (acc.dim() - 2)
    pre = acc
    if scale is not None:
        pre = pre * scale.double().reshape(cshape)
    if shift is not None:
        pre = pre + shift.double().reshape(cshape)
    if res_pre is not None:
        pre = pre + res_pre
    y = F.relu(pre) if relu else pre
    if res_post is not None:
        y = y + upsample(res_post, post_up)
    return y, pre


def check_fixture(what, ref, pre, bound, unit, relu):
    """The three conditions on a fixture (conditions, not measurements):
    1. partial sums exact: the sum of absolute terms, in lattice units, stays below 2^24;
    2. the exact output is storable in bf16;
    3. at least 25 % of the outputs are non-zero, and at least 25 % are zeroed by the ReLU where there is one."""
    assert float(bound.max()) / unit < 2 ** 24, (what, float(bound.max()), unit)
    assert torch.equal((ref / unit).round() * unit, ref), (what, "off the lattice")
    assert torch.equal(ref.to(BF16).double(), ref), (what, "not bf16-storable", float(ref.abs().max()))
    check_occupancy(what, ref, pre, relu)


def check_occupancy(what, ref, pre, relu):
    """Condition 3 of check_fixture."""
    nz = float((ref != 0).double().mean())
    assert nz >= 0.25, (what, "non-zero fraction", nz)
    if relu:
        zeroed = float((pre < 0).double().mean())
        assert zeroed >= 0.25, (what, "fraction zeroed by the ReLU", zeroed)


def assert_lattice_equal(got, want, what, tiles=(8, 16, 32)):
    """torch.equal on channels-last tensors [B][spatial...][C]; on a mismatch, the count, the first coordinates with
    got / expected, and whether they lie on a tensor edge, a tile edge or a channel tail."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    shape = tuple(got.shape)
    C = shape[-1]
    lines = ["%s: %d of %d elements differ (shape %s)" % (what, len(bad), got.numel(), shape)]
    n_edge = n_tile = n_tail = 0
    for n, idx in enumerate(bad.tolist()):
        sp, c = idx[1:-1], idx[-1]
        edge = any(v == 0 or v == s - 1 for v, s in zip(sp, shape[1:-1]))
        tile = any(v % t in (0, t - 1) for v in sp for t in tiles)
        tail = c >= C // 8 * 8 if C % 8 else C > 16 and C % 16 != 0 and c >= C // 16 * 16  # last partial 8 / 16 group
        n_edge, n_tile, n_tail = n_edge + edge, n_tile + tile, n_tail + tail
        if n < 8:
            lines.append("  %s: got %r expected %r%s%s%s" % (tuple(idx), float(got[tuple(idx)]), float(want[tuple(idx)]),
                                                             " [tensor edge]" if edge else "",
                                                             " [tile edge]" if tile else "",
                                                             " [channel tail]" if tail else ""))
    lines.append("  on a tensor edge: %d, on a tile edge (multiples of %s): %d, in a channel tail: %d"
                 % (n_edge, "/".join(map(str, tiles)), n_tile, n_tail))
    pytest.fail("\n".join(lines))


def channels_last(t):
    return t.permute(0, *range(2, t.dim()), 1).contiguous()


# ---------------------------------------------------------------------------------------------- 2D front-end layers

def _conv2d_weight_density(fan):
    # small fan-ins keep every output channel busy; wide ones stay at the density the issue checked (max |y| < 128)
    return 1.0 if fan <= 64 else 0.5 if fan <= 256 else 0.25


@functools.lru_cache(maxsize=2)
def conv2d_fixture(i):
    return conv2d_build(i)


def conv2d_build(i, tweak=None, seed=None, act_density=0.5):
    """Lattice weights, bias, tensor inputs, planar inputs, res_pre and res_post of row i of test_gpu_frontend.CASES,
    with the float64 reference on the explicitly concatenated input. tweak(w, full, transposed) -> (w, full) replaces
    the weights and the concatenated input before the reference is taken (test_gpu_split.py); seed / act_density override
    the generator's seed and the density of the tensor and planar inputs."""
    case = CONV2D_CASES[i]
    tr, k, s, p, op, c0, c1, geo, cout, relu, pre, post_up = case[:12]
    H, W = case[12] if len(case) > 12 else (20, 24)
    g = torch.Generator().manual_seed(1000 + i if seed is None else seed)
    cin = c0 + c1 + len(geo)
    fan = cin * k * k // (s * s if tr else 1)
    w = lattice((cin, cout, k, k) if tr else (cout, cin, k, k), WGT, _conv2d_weight_density(fan), g)
    bias = lattice((cout,), WGT, 1.0, g)
    a = lattice((B, c0, H, W), ACT, act_density, g) if c0 else None
    b = lattice((B, c1, H, W), ACT, act_density, g) if c1 else None
    gp = lattice((B, len(geo), H, W), ACT, act_density, g) if geo else None
    full = torch.zeros(B, cin, H, W, dtype=torch.float64)  # the reference input in weight-channel order
    tensor_at = [c for c in range(cin) if c not in geo]
    if c0:
        full[:, tensor_at[:c0]] = a
    if c1:
        full[:, tensor_at[c0:]] = b
    for j, gc in enumerate(geo):
        full[:, gc] = gp[:, j]
    if tweak is not None:
        w, full = tweak(w, full, tr)
        a = full[:, tensor_at[:c0]] if c0 else None
        b = full[:, tensor_at[c0:]] if c1 else None
        gp = full[:, list(geo)] if geo else None
    if tr:
        conv = lambda x, w_: F.conv_transpose2d(x, w_, None, stride=s, padding=p, output_padding=op)  # noqa: E731
    else:
        conv = lambda x, w_: F.conv2d(x, w_, None, stride=s, padding=p)  # noqa: E731
    acc = conv(full, w)
    Ho, Wo = acc.shape[2:]
    res_pre = lattice(acc.shape, ACT, 0.5, g) if pre else None
    post = lattice((B, cout, Ho // post_up, Wo // post_up), ACT, 0.5, g) if post_up else None
    ref, preact = layer_reference(acc, None, bias, res_pre, relu, post, post_up)
    bound = layer_reference(conv(full.abs(), w.abs()), None, bias.abs(), res_pre.abs() if pre else None, False,
                            post.abs() if post_up else None, post_up)[0]
    return types.SimpleNamespace(case=case, H=H, W=W, cin=cin, tensor_at=tensor_at, w=w, bias=bias, a=a, b=b, gp=gp,
                                 full=full, conv=conv, acc=acc, res_pre=res_pre, post=post, ref=ref, preact=preact,
                                 bound=bound, unit=0.5, tr=tr, relu=relu)


# ---------------------------------------------------------------------------------------------- fused FPN top

FPN_SHAPES = ((2, 12, 20), (3, 18, 134))
_FPN_S = ((2,), (1, 2), (0, 1), (0,))  # 3x3 taps merged into each transposed k4 s2 tap by the nearest upsampling


@functools.lru_cache(maxsize=2)
def fpn_fixture(Bn, H, W):
    return fpn_build(Bn, H, W)


def fpn_build(Bn, H, W, tweak=None):
    """Lattice inner2 (1x1, 8 -> 32, bias) / out3 (3x3, 32 -> 8) and inputs; the unfused float64 reference
    out3(up2(f) + inner2(c0)); and the re-associated weights (frontend_hip.fpn_top_layers) restated in float64.
    tweak(c0, f) -> (c0, f) replaces the two inputs before the reference is taken (test_gpu_split.py)."""
    g = torch.Generator().manual_seed(H * W)
    W1 = lattice((32, 8), WGT, 0.25, g)
    b1 = lattice((32,), WGT, 1.0, g)
    W3 = lattice((8, 32, 3, 3), WGT, 0.125, g)
    c0 = lattice((Bn, 8, H, W), ACT, 0.5, g)
    f = lattice((Bn, 32, H // 2, W // 2), ACT, 0.5, g)
    if tweak is not None:
        c0, f = tweak(c0, f)
    inner = lambda x, w_, b_: F.conv2d(x, w_[:, :, None, None], b_)  # noqa: E731
    ref = F.conv2d(upsample(f, 2) + inner(c0, W1, b1), W3, padding=1)
    bound = F.conv2d(upsample(f.abs(), 2) + inner(c0.abs(), W1.abs(), b1.abs()), W3.abs(), padding=1)
    wt = torch.zeros(32, 8, 4, 4, dtype=torch.float64)
    for a in range(4):
        for b in range(4):
            wt[:, :, a, b] = sum(W3[:, :, ky, kx] for ky in _FPN_S[a] for kx in _FPN_S[b]).t()
    wc = torch.einsum("omyx,mi->oiyx", W3, W1)
    corr = torch.einsum("omyx,m->yxo", W3, b1)
    bc = corr.sum((0, 1))
    # what the fused launch stores before damvs_conv2d_border_bias: the full 9-tap bias at every pixel
    inside = F.conv2d(b1.reshape(1, 32, 1, 1).expand(1, 32, H, W), W3, padding=1)
    prefix = ref - inside + bc.reshape(1, 8, 1, 1)
    return types.SimpleNamespace(W1=W1, b1=b1, W3=W3, c0=c0, f=f, ref=ref, bound=bound, wt=wt, wc=wc, corr=corr, bc=bc,
                                 prefix=prefix, unit=0.25)


# ---------------------------------------------------------------------------------------------- 3D U-Net layers

UNET_C = (32, 16, 8)
UNET_SHAPES = ((8, 24, 40), (24, 40, 72), (40, 24, 104))
SWITCH_SHAPE = (24, 40, 72)
SWITCHES = ("DAMVS_CONV_NO_ZSLIDE", "DAMVS_DECONV_NO_ZSLIDE")
BN_EPS = 1e-5
# (BatchNorm weight, running_var + eps): scale = weight / sqrt(var + eps) is exactly 0.5, 1 or 2 in float32
BN_COMBOS = ((0.5, 1.0), (1.0, 1.0), (2.0, 1.0), (0.5, 0.25), (1.0, 0.25), (1.0, 4.0), (2.0, 4.0))


def fold_bn_numpy(weight, bias, mean, var, eps):
    """weight_pack.h bn_affine restated: float32 tensors and a float32 eps in, double arithmetic, float32 scale / shift out."""
    weight, bias, mean, var = (np.asarray(t, np.float32).astype(np.float64) for t in (weight, bias, mean, var))
    inv = 1.0 / np.sqrt(var + np.float64(np.float32(eps)))
    return (inv * weight).astype(np.float32), (bias - mean * inv * weight).astype(np.float32)


@functools.lru_cache(maxsize=None)
def unet_net(C, zero_shift=False):
    """CostRegNet(C, 8) with lattice conv weights and BatchNorms that fold to exact lattice values: per-channel scale in
    {0.5, 1, 2} (from every (weight, variance) pair of BN_COMBOS), running_mean 0, and a half-integer bias =
    scale * b with b in {+-0.5, +-1} (+-1, +-2 where the scale is 0.5): a channel is then a power-of-two multiple of
    the lattice tensor conv + b, and whether it is storable does not depend on its scale. zero_shift: the same net
    (same draws) with every BatchNorm bias 0, so that each layer is homogeneous in its input. Returns (net, {layer
    name: (intended scale, intended shift)})."""
    from damvsnet_amd.layers import CostRegNet
    g = torch.Generator().manual_seed(77 + C)
    net = CostRegNet(C, 8)
    want = {}
    with torch.no_grad():
        for name in CostRegNet.ENCODER + CostRegNet.DECODER:
            m = getattr(net, name)
            m.conv.weight.copy_(lattice(m.conv.weight.shape, WGT, 0.25, g))
            co = m.out_channels
            combo = torch.randint(len(BN_COMBOS), (co,), generator=g)
            combo[:min(co, len(BN_COMBOS))] = torch.arange(len(BN_COMBOS))[:co]  # every pair at least once
            bw = torch.tensor([BN_COMBOS[j][0] for j in combo], dtype=torch.float32)
            vb = torch.tensor([BN_COMBOS[j][1] for j in combo], dtype=torch.float32)
            scale = bw / vb.sqrt()
            half = lattice((co,), WGT, 1.0, g).float()
            shift = scale * torch.where(scale == 0.5, 2 * half, half)  # a half-integer in {+-0.5, +-1, +-2}
            if zero_shift:
                shift = torch.zeros_like(shift)
            assert m.bn.eps == BN_EPS
            m.bn.weight.copy_(bw)
            m.bn.bias.copy_(shift)
            m.bn.running_mean.zero_()
            m.bn.running_var.copy_(vb - torch.tensor(BN_EPS, dtype=torch.float32))  # float32(v) - float32(eps)
            want[name] = (scale, shift)
        net.prob.weight.copy_(lattice(net.prob.weight.shape, WGT, 0.25, g))
    return net.eval(), want


@functools.lru_cache(maxsize=3)
def unet_fixture(C, shape, layer):
    return unet_build(unet_net(C), C, shape, layer)


def unet_build(net_want, C, shape, layer, tweak=None):
    """Layer `layer` (0..9) of the net (unet_net's return value) on its own lattice input of its level's shape, a
    lattice skip tensor for the deconvs, and the float64 reference relu(conv * scale + shift) (+ skip). tweak(x) -> x
    replaces the input before the reference is taken (test_gpu_split.py)."""
    from damvsnet_amd.costmodel import unet_layers
    name, cin, cout, li, lo, tr, skip = unet_layers(C, 8)[layer]
    D, h, w = shape
    net, want = net_want
    g = torch.Generator().manual_seed(C * 1000 + layer * 10 + UNET_SHAPES.index(shape))
    x = lattice((B, cin, D >> li, h >> li, w >> li), ACT, 0.5, g)
    if tweak is not None:
        x = tweak(x)
    wgt = getattr(net, name).conv.weight.detach().double()
    scale, shift = want[name]
    if tr:
        conv = lambda x_, w_: F.conv_transpose3d(x_, w_, None, stride=2, padding=1, output_padding=1)  # noqa: E731
    else:
        conv = lambda x_, w_: F.conv3d(x_, w_, None, stride=1 if li == lo else 2, padding=1)  # noqa: E731
    acc = conv(x, wgt)
    assert acc.shape == (B, cout, D >> lo, h >> lo, w >> lo)
    sk = lattice(acc.shape, ACT, 0.5, g) if skip else None
    ref, preact = layer_reference(acc, scale, shift, None, True, sk)
    bound = layer_reference(conv(x.abs(), wgt.abs()), scale, shift.abs(), None, False, sk.abs() if skip else None)[0]
    return types.SimpleNamespace(name=name, x=x, skip=sk, ref=ref, preact=preact, bound=bound, unit=0.25, w=wgt,
                                 scale=scale.double(), shift=shift.double(), conv=conv, acc=acc, tr=bool(tr))


# ---------------------------------------------------------------------------------------------- the CPU tests

FIXTURE_GROUPS = (["conv2d", "fpn_top", "bn_fold"] +
                  ["unet_C%d_%dx%dx%d" % ((C,) + s) for C in UNET_C for s in UNET_SHAPES])


@pytest.mark.parametrize("group", FIXTURE_GROUPS)
def test_lattice_fixtures_are_exact(group):
    """Every case of the GPU tests below meets the three conditions of check_fixture; the BatchNorm fold gives exactly
    the intended lattice scale and shift; the FPN top's composed and packed weights are exact bf16 values and exact
    f16 pairs (lo = 0)."""
    if group == "conv2d":
        for i in range(len(CONV2D_CASES)):
            fx = conv2d_fixture(i)
            check_fixture("conv2d case %d" % i, fx.ref, fx.preact, fx.bound, fx.unit, fx.case[9])
    elif group == "fpn_top":
        from damvsnet_amd.frontend_hip import _fpn_top_A, pack_fpn_top, pack_fpn_top_split
        for shp in FPN_SHAPES:
            fx = fpn_fixture(*shp)
            check_fixture("fpn top %s" % (shp,), fx.ref, None, fx.bound, fx.unit, False)
            # the fused launch's own store (full bias everywhere) is exact too, before the border fix-up
            assert torch.equal(fx.prefix.to(BF16).double(), fx.prefix)
            for t in (fx.wt, fx.wc, fx.bc, fx.corr):
                assert torch.equal(t.float().double(), t)
            A = _fpn_top_A(fx.wt.float(), fx.wc.float())
            assert torch.equal(pack_fpn_top(fx.wt.float(), fx.wc.float()).float(), A)
            halves, ws = pack_fpn_top_split(fx.wt.float(), fx.wc.float())
            halves = halves.view(torch.float16)
            assert not bool(halves[:, 1].any())                      # lo = 0
            assert torch.equal(halves[:, 0].float() * ws, A)          # hi * 2^-k is the weight
    elif group == "bn_fold":
        from damvsnet_amd.layers import CostRegNet
        for C in UNET_C:
            net, want = unet_net(C)
            for name in CostRegNet.ENCODER + CostRegNet.DECODER:
                bn = getattr(net, name).bn
                scale, shift = fold_bn_numpy(bn.weight.detach().numpy(), bn.bias.detach().numpy(),
                                             bn.running_mean.numpy(), bn.running_var.numpy(), bn.eps)
                assert np.array_equal(scale, want[name][0].numpy()), (C, name)
                assert np.array_equal(shift, want[name][1].numpy()), (C, name)
                assert set(np.unique(scale)) <= {0.5, 1.0, 2.0} and len(np.unique(scale)) == 3
                assert set(np.unique(np.abs(shift))) <= {0.5, 1.0, 2.0}  # half-integers, never 0
    else:
        C, shape = [(C, s) for C in UNET_C for s in UNET_SHAPES][FIXTURE_GROUPS.index(group) - 3]
        for layer in range(10):
            fx = unet_fixture(C, shape, layer)
            check_fixture("%s %s" % (group, fx.name), fx.ref, fx.preact, fx.bound, fx.unit, True)


def test_one_dropped_tap_passes_rel_max_but_not_equality():
    """Why this file exists: zero one non-zero weight tap of the 256 -> 256 3x3 layer. The lattice comparison
    (equality of the bf16 stores) fails, while rel_max on the same pair stays under the 2e-2 gate that
    test_conv2d_layer_vs_torch allows for bf16."""
    i = next(n for n, c in enumerate(CONV2D_CASES) if c[:12] == (False, 3, 1, 1, 0, 256, 0, (), 256, True, False, 0))
    fx = conv2d_fixture(i)
    w = fx.w.clone()
    co, ci, ky, kx = (w.abs() == 0.5).nonzero()[0].tolist()
    w[co, ci, ky, kx] = 0.0
    wrong = layer_reference(fx.conv(fx.full, w), None, fx.bias, fx.res_pre, True, fx.post, 1)[0]
    a, b = wrong.to(BF16), fx.ref.to(BF16)
    assert not torch.equal(a, b)
    assert float((a.double() - b.double()).abs().max()) >= 0.5
    assert rel_max(a.float().numpy(), b.float().numpy()) < 2e-2


def test_shifted_cout_block_fails_equality():
    """What the wide-cout-tile rows are for: block row blockIdx.y of the gather kernel stores cout tiles mt0 + m, mt0 = MT
    * blockIdx.y. Take the 64+g -> 256 row's reference (bf16: MT 8, two block rows, the second owns channels 128..255)
    with the second block row's tiles shifted by one 16-channel tile, as an mt0 slip would store them (the last tile
    then holds what lies past cout: nothing). It differs from the true reference by at least 0.5 on more than 25 % of
    all elements, so the equality gate sees it."""
    i = next(n for n, c in enumerate(CONV2D_CASES)
             if c[:12] == (False, 1, 2, 0, 0, 32, 32, (64,), 256, True, False, 0) and c[12] == (200, 288))
    fx = conv2d_fixture(i)
    wrong = fx.ref.clone()
    wrong[:, 128:240] = fx.ref[:, 144:256]
    wrong[:, 240:] = 0
    assert not torch.equal(wrong.to(BF16), fx.ref.to(BF16))
    off = float(((wrong - fx.ref).abs() >= 0.5).double().mean())
    assert off > 0.25, off


# ---------------------------------------------------------------------------------------------- the GPU tests

DT_IDS = {BF16: "bf16", F32: "f32"}


@pytest.mark.gpu
@pytest.mark.parametrize("i,dtype", [(i, dt) for i in range(len(CONV2D_CASES)) for dt in (F32, BF16)],
                         ids=["%d-%s" % (i, DT_IDS[dt]) for i in range(len(CONV2D_CASES)) for dt in (F32, BF16)])
def test_conv2d_layer_exact(i, dtype, _lib):
    """Every form of test_gpu_frontend.CASES on lattice data: equal to the float64 reference on the first cout channels,
    exactly 0 on the padded channels up to cout_store."""
    run_conv2d_layer(conv2d_fixture(i), dtype, "conv2d case %d %s" % (i, DT_IDS[dtype]))


# The rows that a switch routes to another kernel, with that switch off: every "cases" entry of tests/conv2d_routes.json
# beyond the defaults (tests/route_cases.py). The kernels behind the A/B switches (the VALU plane kernels in bf16, the
# 16-K gather form, the wide and halo kernels' plain loops, the x-pair gather form) meet the reference themselves here.
SWITCHED_RUNS = route_cases.exact_runs(switched_only=True)


@pytest.mark.gpu
@pytest.mark.parametrize("i,dt,off", SWITCHED_RUNS, ids=[route_cases.case_key(*r) for r in SWITCHED_RUNS])
def test_conv2d_layer_exact_switched(i, dt, off, _lib, monkeypatch):
    for sw in off:
        monkeypatch.setenv(sw, "0")
    key = route_cases.case_key(i, dt, off)
    assert route_cases.case_route(i, dt) == route_cases.load()["cases"][key], key   # the switched kernel, not the default once more
    run_conv2d_layer(conv2d_fixture(i), route_cases.DTYPES[dt], "conv2d case %s" % key)


def run_conv2d_layer(fx, dtype, what, equal=assert_lattice_equal):
    """The body of test_conv2d_layer_exact on fixture fx (test_gpu_split.py runs it on its own fixtures)."""
    from damvsnet_amd.frontend_hip import HipConv2d, planes
    tr, k, s, p, op, c0, c1, geo, cout, relu, pre, post_up = fx.case[:12]
    H, W = fx.H, fx.W
    conv = (nn.ConvTranspose2d(fx.cin, cout, k, stride=s, padding=p, output_padding=op) if tr
            else nn.Conv2d(fx.cin, cout, k, stride=s, padding=p))
    with torch.no_grad():
        conv.weight.copy_(fx.w)
        conv.bias.copy_(fx.bias)
    at = dict(c0=c0, c1=c1, c1_at=0)
    if c0 and c1:
        at = dict(c0=c0, c0_at=fx.tensor_at[0], c1=c1, c1_at=fx.tensor_at[c0])
    elif c0:
        at = dict(c0=c0, c0_at=fx.tensor_at[0])
    L = HipConv2d(conv, dtype, relu, geo_at=geo, **at)
    cs = L.cout_store
    padc = lambda t: F.pad(t, (0, 0, 0, 0, 0, cs - cout)) if cs != cout else t  # noqa: E731
    dev = lambda t: channels_last(t).to(DEV, dtype)  # noqa: E731
    out = L(B, H, W, dev(fx.a) if c0 else None, dev(fx.b) if c1 else None,
            geo=planes(fx.gp.float().to(DEV)) if geo else (),
            res_pre=dev(padc(fx.res_pre)) if pre else None,
            res_post=dev(padc(fx.post)) if post_up else None, post_up=max(post_up, 1))
    got = out.cpu()
    assert got.shape == (B,) + tuple(fx.ref.shape[2:]) + (cs,)
    equal(got[..., :cout].contiguous(), channels_last(fx.ref).to(dtype), what)
    assert not bool(got[..., cout:].any()), "padded channels %d..%d are not zero" % (cout, cs)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("Bn,H,W", FPN_SHAPES)
def test_fpn_top_fused_exact(Bn, H, W, dt, _lib):
    """damvs_fpn_top_forward / damvs_fpn_top_forward_f32 + damvs_conv2d_border_bias, and the two-launch path, against
    the unfused out3(up2(f) + inner2(c0)) in float64: equal at every pixel, the border ring and corners included. The
    composed weights are multiples of 0.25 below 64, so they are exact bf16 values, and scaled by a power of two they
    are exact f16 values with a zero lo half (asserted on the CPU from the packed values): both dtypes are exact."""
    run_fpn_top(fpn_fixture(Bn, H, W), Bn, H, W, dt)


def run_fpn_top(fx, Bn, H, W, dt, equal=assert_lattice_equal):
    """The body of test_fpn_top_fused_exact on fixture fx (test_gpu_split.py runs it on its own fixtures)."""
    from damvsnet_amd import _capi
    from damvsnet_amd.engine import DTYPES
    from damvsnet_amd.frontend_hip import fpn_top_layers, pack_fpn_top, pack_fpn_top_split
    inner2, out3 = nn.Conv2d(8, 32, 1, bias=True), nn.Conv2d(32, 8, 3, padding=1, bias=False)
    with torch.no_grad():
        inner2.weight.copy_(fx.W1[:, :, None, None])
        inner2.bias.copy_(fx.b1)
        out3.weight.copy_(fx.W3)
    up, conv, corr, (wt, wc, bc) = fpn_top_layers(inner2, out3, dt)
    assert torch.equal(wt.double(), fx.wt) and torch.equal(wc.double(), fx.wc) and torch.equal(bc.double(), fx.bc)
    assert torch.equal(corr.double(), fx.corr.reshape(-1))
    lib = _capi.load_library()
    c0d, fd = channels_last(fx.c0).to(DEV, dt), channels_last(fx.f).to(DEV, dt)
    o = torch.empty(Bn, H, W, 8, device=DEV, dtype=dt)
    bd = bc.float().to(DEV)
    if dt == BF16:
        ap = pack_fpn_top(wt, wc).to(DEV)  # held until the launch has run
        _capi.check(lib.damvs_fpn_top_forward(_capi.stream_ptr(o.device), Bn, H, W, c0d.data_ptr(), fd.data_ptr(),
                                              ap.data_ptr(), bd.data_ptr(), o.data_ptr()))
    else:
        ap, ws = pack_fpn_top_split(wt, wc)
        ap = ap.to(DEV)
        _capi.check(lib.damvs_fpn_top_forward_f32(_capi.stream_ptr(o.device), Bn, H, W, c0d.data_ptr(), fd.data_ptr(),
                                                  ap.data_ptr(), ws, bd.data_ptr(), o.data_ptr()))
    o2 = conv(Bn, H, W, c0d, res_pre=up(Bn, H // 2, W // 2, fd))
    want_prefix = channels_last(fx.prefix).to(dt)
    equal(o.cpu(), want_prefix, "fpn top fused %s, before the border fix-up" % DT_IDS[dt])
    for t in (o, o2):
        _capi.check(lib.damvs_conv2d_border_bias(_capi.stream_ptr(t.device), DTYPES[dt], Bn, H, W, 8, 8,
                                                 _capi.float_ptr(corr), t.data_ptr()))
    want = channels_last(fx.ref).to(dt)
    equal(o.cpu(), want, "fpn top fused %s" % DT_IDS[dt])
    equal(o2.cpu(), want, "fpn top in two launches %s" % DT_IDS[dt])


_ENGINES = {}


def _engine(C, dtype):
    from damvsnet_amd.engine import StageEngine
    if (C, dtype) not in _ENGINES:
        _ENGINES[C, dtype] = StageEngine(unet_net(C)[0], None, "variance", dtype, torch.device(DEV))
    return _ENGINES[C, dtype]


UNET_MODES = ("bf16", "f32", "f32-slots")
# ordered so that the runs sharing a float64 reference follow each other (unet_fixture keeps the last few)
UNET_RUNS = [(C, shape, layer, mode, sw)
             for C in UNET_C for shape in UNET_SHAPES for layer in range(10)
             for sw in (None,) + (SWITCHES if shape == SWITCH_SHAPE else ())
             for mode in UNET_MODES]


@pytest.mark.gpu
@pytest.mark.parametrize("C,shape,layer,mode,switch", UNET_RUNS,
                         ids=["C%d-%dx%dx%d-L%d-%s%s" % ((C,) + s + (l, m, "-" + sw[6:] if sw else ""))
                              for C, s, l, m, sw in UNET_RUNS])
def test_unet_layer_exact(C, shape, layer, mode, switch, _lib, monkeypatch):
    """damvs_costreg_layer_scaled, one layer at a time on its own lattice input (chained activations would leave the
    lattice), against relu(conv3d * scale + shift) / relu(conv_transpose3d * scale + shift) + skip in float64: equal.
    fp32 with magnitude slots: as the stage forward runs it (the input's slot filled by damvs_tensor_amax, conv11
    without an output slot); the recorded output maximum equals max |ref| of each batch element exactly, read over
    every replica word of the slot. With DAMVS_CONV_NO_ZSLIDE / DAMVS_DECONV_NO_ZSLIDE the tile and gather kernels
    that other shapes fall back to meet the reference themselves, not only their z-streamed siblings."""
    dtype = BF16 if mode == "bf16" else F32
    fx = unet_fixture(C, shape, layer)
    if switch:
        monkeypatch.setenv(switch, "1")
    run_unet_layer(_engine(C, dtype), fx.x, fx.skip, fx.ref, layer, shape, mode,
                   "C %d %s %s %s %s" % (C, shape, fx.name, mode, switch or ""))


def run_unet_layer(eng, x64, skip64, ref64, layer, shape, mode, what, equal=assert_lattice_equal):
    """The body of test_unet_layer_exact: layer `layer` of engine eng on the float64 input x64 (and skip64 for the
    deconvs) against ref64 (test_gpu_split.py runs it on its own fixtures)."""
    from damvsnet_amd.sharded import _SLOTS
    dtype = BF16 if mode == "bf16" else F32
    D, h, w = shape
    x = channels_last(x64).to(DEV, dtype)
    want = channels_last(ref64).to(dtype)
    if skip64 is not None:
        out = channels_last(skip64).to(DEV, dtype)
    else:  # a conv must overwrite whatever its output held
        out = torch.full(want.shape, 3.0, device=DEV, dtype=dtype)
    if mode != "f32-slots":
        eng.unet_layer(layer, D, h, w, x, out)
    else:
        slots = eng.new_slots(B)
        sin, sout = _SLOTS[layer]
        eng.tensor_amax(x, slots[sin])
        eng.unet_layer(layer, D, h, w, x, out, in_slot=slots[sin], out_slot=None if sout is None else slots[sout])
        torch.cuda.synchronize()
        if sout is not None:
            rec = slots[sout].cpu().amax(1).view(torch.float32)  # non-negative floats order as their bit patterns
            exp = ref64.abs().reshape(B, -1).amax(1).float()
            assert torch.equal(rec, exp), (what, "recorded max", rec.tolist(), "max |ref|", exp.tolist())
            untouched = [t for t in range(slots.shape[0]) if t not in (sin, sout)]
            assert not bool(slots[untouched].any()), (what, "another tensor's slot was written")
    equal(out.cpu(), want, what)
