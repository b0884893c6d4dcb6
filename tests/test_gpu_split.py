"""Exact per-layer tests of the fp32 path's split-f16 cross terms: every conv2d form, the FPN top and every U-Net layer
against float64 references on inputs whose f16 lo pieces are not zero, so the gate is still equality per element.

The fp32 path computes w * x as wl*xh + wh*xl + wh*xh on f16 MFMAs (damvs_device.h mma_split16 / mma_split32), weights
split on the host (weight_pack.h split_weights), activations in the kernels after the power-of-two prescale. On the fixtures
of test_gpu_lattice.py every lo piece is 0, so the two cross terms never count there. The "two-piece" fixtures here add
+-2^-12 (random sign) to the non-zero lattice values of

  the activations on the odd input channels,     (their lo piece meets wh: the wh*xl term)
  the weights on the even input channels,        (their lo piece meets xh: the wl*xh term)

input channel meaning the position in the layer's concatenated weight-channel order. Then every perturbed value is the
exact sum of its two f16 pieces (1 + 2^-12 -> 1 and 2^-12; only +-(0.5 - 2^-12), an 11-bit value, has lo = 0); a
perturbed weight never meets a perturbed activation, so wl*xl is 0 and the three-term sum is the float64 convolution of
the same inputs; with folded BatchNorm scales in {0.5, 1, 2} every term is a multiple of 2^-14 and, the sum of absolute
terms staying below 2^24 such units, every partial sum in any order is exact in fp32. A kernel that drops a cross term,
pairs xl with the wrong K slot, stages a lo half at the wrong swizzle or reads a mispacked [hi | lo] fragment moves an
element by at least one unit; test_one_dropped_lo_tap_passes_rel_max_but_not_equality shows the 2e-5 global-norm gate
of the off-lattice fp32 tests missing exactly that.

CPU part (not marked gpu): test_two_piece_fixtures_are_exact proves the conditions above for every case the GPU tests
use, from the f16 pieces taken as the code takes them. The GPU tests are fp32 only (bf16 storage rounds the perturbation
away). test_unet_layer_prescale_exact_across_scales runs the same layers with one batch element scaled by 2^-40 and the
other by 2^+20 in one launch: unscaled, or with the other sample's magnitude slot, one of the two leaves the f16 range.
"""
import copy
import functools
import math
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import route_cases
import test_gpu_lattice as L
from conftest import rel_max
from test_gpu_lattice import (B, CONV2D_CASES, FPN_SHAPES, SWITCH_SHAPE, UNET_C, UNET_SHAPES, _lib,  # noqa: F401
                              assert_lattice_equal, channels_last, layer_reference, unet_net)

F32 = torch.float32
EPS = 2.0 ** -12          # the perturbation
UNIT = 2.0 ** -14         # every term of every fixture is a multiple of it (EPS * weight 0.5 * BatchNorm scale 0.5)


# ---------------------------------------------------------------------------------------------- fixture helpers

def two_piece(t, dim, parity, gen):
    """t with +-EPS (random sign) added to its non-zero elements whose index along `dim` has the given parity."""
    sign = torch.randint(2, tuple(t.shape), generator=gen).double() * 2 - 1
    sel = torch.zeros(t.shape[dim], dtype=torch.float64)
    sel[parity::2] = 1
    shape = [1] * t.dim()
    shape[dim] = -1
    return t + EPS * sign * (t != 0) * sel.reshape(shape)


def split_exponent(v):
    """weight_pack.h split_exponent and damvs_device.h prescale_from_max alike: the k that puts max |v| * 2^k in [2^13, 2^14)."""
    mx = float(v.abs().max())
    return 0 if mx == 0.0 else max(-100, min(100, 14 - math.frexp(mx)[1]))


def f16_pieces(v):
    """hi = f16(v), lo = f16(v - hi) of fp32 values, as split_weights / split_f16 / split8 take them; float64 out."""
    v32 = v.float()
    assert torch.equal(v32.double(), v), "not an fp32 value"
    hi = v32.half()
    lo = (v32 - hi.float()).half()
    return hi.double(), lo.double()


def per_sample(v, like):
    return v.reshape((-1,) + (1,) * (like.dim() - 1))


def split_terms(fx):
    """The CPU model of a layer's split products. Weights: w * scale (the folded BatchNorm scale) * 2^k with k from the
    layer's largest folded weight; activations: x * 2^ka with ka from each batch element's maximum where the layer
    prescales (the U-Net layers; the conv2d kernels split x as it is, the plane kernel's block-wise prescale is one
    more power of two). Returns the pieces, the four piece convolutions scaled back, and the scaled-back sum of the
    absolute terms. (In a layer with tensor inputs and a planar input the plane's products are plain fp32 FMAs; its
    three terms here sum to the same exact product.)"""
    ws = fx.w if fx.scale is None else fx.w * fx.scale.reshape((1, -1) + (1,) * (fx.w.dim() - 2) if fx.tr
                                                                 else (-1,) + (1,) * (fx.w.dim() - 1))
    k = split_exponent(ws)
    wv = ws * 2.0 ** k
    wh, wl = f16_pieces(wv)
    if fx.prescale:
        ka = torch.tensor([split_exponent(fx.x[b]) for b in range(fx.x.shape[0])], dtype=torch.float64)
    else:
        ka = torch.zeros(fx.x.shape[0], dtype=torch.float64)
    xv = fx.x * per_sample(2.0 ** ka, fx.x)
    xh, xl = f16_pieces(xv)
    hh, lh, hl, ll = fx.conv(xh, wh), fx.conv(xl, wh), fx.conv(xh, wl), fx.conv(xl, wl)
    back = per_sample(2.0 ** (-k - ka), hh)
    sum_abs = (fx.conv(xh.abs(), wh.abs()) + fx.conv(xl.abs(), wh.abs()) + fx.conv(xh.abs(), wl.abs())) * back
    return types.SimpleNamespace(wv=wv, wh=wh, wl=wl, xv=xv, xh=xh, xl=xl, hh=hh * back, lh=lh * back, hl=hl * back,
                                 ll=ll * back, sum_abs=sum_abs, back=back)


def check_two_piece(what, fx, weights=True):
    """The conditions that make torch.equal the right gate on fixture fx (conditions, not measurements). fx: x, w,
    scale, tr, conv, prescale, epi (layer_reference's arguments after the folded scale), ref, preact, pw (the power of
    two each batch element is scaled by). weights=False: the layer's weights carry no perturbation (the FPN top)."""
    t = split_terms(fx)
    epi = fx.epi
    # every value is the exact sum of its two f16 pieces
    assert torch.equal(t.wh + t.wl, t.wv), (what, "a weight is not hi + lo")
    assert torch.equal(t.xh + t.xl, t.xv), (what, "an activation is not hi + lo")
    # the three-term sum, scaled back and through the epilogue, is the float64 reference; the dropped term is zero
    model = layer_reference(t.hh + t.lh + t.hl, None, **epi)[0]
    assert torch.equal(model, fx.ref), (what, "three-term sum != float64 reference")
    assert not bool(t.ll.any()), (what, "wl * xl is not zero")
    # every partial sum in any order is exact in fp32, and the result is fp32-storable
    absepi = {n: (v.abs() if torch.is_tensor(v) else v) for n, v in epi.items()}
    absepi["relu"] = False
    bound = layer_reference(t.sum_abs, None, **absepi)[0]
    units = float((bound / per_sample(UNIT * 2.0 ** fx.pw, bound)).max())
    assert units < 2 ** 24, (what, "sum |terms| / unit = 2^%.2f" % math.log2(units))
    assert torch.equal(fx.ref.float().double(), fx.ref), (what, "not fp32-storable")
    # both cross terms are busy
    xlo = float((t.xl != 0).double().mean())
    assert xlo >= 0.20, (what, "activation elements with a non-zero lo", xlo)
    if weights:
        wlo = float((t.wl != 0).double().mean())
        assert wlo >= 0.05, (what, "weight elements with a non-zero lo", wlo)
        taps = (t.wl != 0).reshape(t.wl.shape[0], t.wl.shape[1], -1).any(0).any(0)
        assert bool(taps.all()), (what, "kernel taps without a non-zero lo weight", (~taps).nonzero().flatten().tolist())
    else:
        assert not bool(t.wl.any()), (what, "unperturbed weights with a non-zero lo")
    L.check_occupancy(what, fx.ref, fx.preact, epi["relu"])
    return t


def cross_terms(fx):
    """(wh * xl term, wl * xh term) of fixture fx as [B][C][...] float64, before the epilogue: the contributions of the
    odd input channels' lo activations and of the even input channels' lo weights."""
    t = split_terms(fx)
    return t.lh, t.hl


def split_equal(fx):
    """assert_lattice_equal, with one more line on a mismatch: which cross term the failing elements carry. Odd input
    channels hold the two-piece activations (the wh * xl term), even ones the two-piece weights (wl * xh)."""
    def equal(got, want, what, **kw):
        try:
            assert_lattice_equal(got, want, what, **kw)
            return
        except pytest.fail.Exception as e:
            report = str(e)
        odd, even = cross_terms(fx)
        C = got.shape[-1]
        odd, even = (channels_last(v)[..., :C] for v in (odd, even))
        bad = got != want
        err = (got.double() - want.double())[bad]
        o, ev = odd[bad], even[bad]
        n_odd, n_even = int(((err == -o) & (o != 0)).sum()), int(((err == -ev) & (ev != 0)).sum())
        pytest.fail("%s\n  of the %d failing elements: %d carry a wh*xl term (odd input channels, lo activations), %d a "
                    "wl*xh term (even input channels, lo weights)\n  error == -(wh*xl term) at %d, == -(wl*xh term) at %d, "
                    "== -(both) at %d: %s"
                    % (report, len(err), int((o != 0).sum()), int((ev != 0).sum()), n_odd, n_even,
                       int(((err == -(o + ev)) & (o != 0) & (ev != 0)).sum()),
                       "the odd input channels fail (wh*xl is wrong)" if n_odd > 2 * n_even else
                       "the even input channels fail (wl*xh is wrong)" if n_even > 2 * n_odd else
                       "neither cross term alone explains the errors"))
    return equal


# ---------------------------------------------------------------------------------------------- 2D front-end layers

# Cases whose default draw misses a condition of check_two_piece get another activation density or seed here (never another
# condition). Three planes have one odd channel: at activation density 0.5 only 1/6 of the elements would carry a lo
# piece. Two planes and two output channels leave two two-piece weights per tap: the seed is one whose draw covers all.
CONV2D_DRAWS = {6: dict(act_density=0.75), 25: dict(act_density=0.75), 7: dict(seed=7003), 64: dict(act_density=0.75),
                70: dict(act_density=0.75)}


@functools.lru_cache(maxsize=2)
def conv2d_split_fixture(i):
    """Row i of test_gpu_frontend.CASES on two-piece data: the lattice fixture's draw, the weights perturbed on the even
    input channels (dim 0 of a transposed conv's weight), the concatenated input (planes included) on the odd ones;
    bias and residuals stay on the plain lattice."""
    g = torch.Generator().manual_seed(5000 + i)
    fx = L.conv2d_build(i, lambda w, full, tr: (two_piece(w, 0 if tr else 1, 0, g), two_piece(full, 1, 1, g)),
                        **CONV2D_DRAWS.get(i, {}))
    post_up = fx.case[11]
    fx.x, fx.scale, fx.prescale, fx.pw = fx.full, None, False, torch.zeros(B, dtype=torch.float64)
    fx.epi = dict(shift=fx.bias, res_pre=fx.res_pre, relu=fx.relu, res_post=fx.post, post_up=post_up)
    return fx


def is_xpair(case):
    tr, k, s, p, op, c0, c1, geo, cout = case[:9]
    return tr and s == 2 and cout == 8 and not geo          # weight_pack.h pack_conv2d


# A layer with one input channel (the one-plane rows) has no odd channel to carry a two-piece activation: those rows run
# on the lattice alone (test_gpu_lattice.py).
SPLIT_ROWS = [i for i, c in enumerate(CONV2D_CASES) if c[5] + c[6] + len(c[7]) >= 2]
# The switched runs are the fp32 entries of tests/conv2d_routes.json beyond the defaults: the rows a switch routes to
# another kernel, with that switch off (the 16-K gather form, the VALU plane kernels, the wide and halo kernels' plain
# loops, the x-pair gather form). The test asserts the recorded kernel before it runs. Rows 0-40 also keep the runs they
# had before the table existed, picked by the packing's condition alone (G32_ROWS) or for being plane-only (PLANE_ROWS):
# where the table has no entry for such a run the switch leaves the row on its usual kernel, which the test asserts too.
G32_ROWS = [i for i, c in enumerate(CONV2D_CASES[:41])
            if not is_xpair(c) and c[5] % 8 == 0 and c[6] % 8 == 0 and c[5] + c[6] >= 8 and len(c[7]) <= 1]
PLANE_ROWS = [i for i, c in enumerate(CONV2D_CASES[:41]) if c[5] + c[6] == 0]
ROUTES = route_cases.load()["cases"]
CONV2D_RUNS = ([(i, ()) for i in SPLIT_ROWS] +
               sorted({(i, off) for i, _, off in route_cases.exact_runs(("f32",), switched_only=True) if i in SPLIT_ROWS} |
                      {(i, ("DAMVS_CONV2D_G32",)) for i in G32_ROWS} | {(i, ("DAMVS_PLANES_MFMA",)) for i in PLANE_ROWS}))


# ---------------------------------------------------------------------------------------------- fused FPN top

@functools.lru_cache(maxsize=2)
def fpn_split_fixture(Bn, H, W):
    """The lattice FPN top with two-piece activations (c0 and f on their odd channels) and its own weights: the composed
    W3 * W1 of a two-piece W1 or W3 would need three pieces."""
    g = torch.Generator().manual_seed(6000 + H * W)
    fx = L.fpn_build(Bn, H, W, lambda c0, f: (two_piece(c0, 1, 1, g), two_piece(f, 1, 1, g)))
    # as one layer for check_two_piece: input cat(c0, up2(f)) [B][8 + 32], weight cat(W3 * W1, W3), bias W3 * b1 through
    # the zero-padded 3x3 conv (ref - conv of the inputs)
    fx.x = torch.cat([fx.c0, L.upsample(fx.f, 2)], 1)
    fx.w = torch.cat([fx.wc, fx.W3], 1)
    fx.conv = lambda x, w_: F.conv2d(x, w_, None, padding=1)  # noqa: E731
    fx.scale, fx.tr, fx.prescale, fx.pw = None, False, False, torch.zeros(Bn, dtype=torch.float64)
    fx.epi = dict(shift=None, res_pre=fx.ref - fx.conv(fx.x, fx.w), relu=False, res_post=None, post_up=1)
    fx.preact = None
    return fx


# ---------------------------------------------------------------------------------------------- 3D U-Net layers

@functools.lru_cache(maxsize=None)
def split_net(C, zero_shift=False):
    """unet_net(C, zero_shift) with every conv weight perturbed on its even input channels."""
    from damvsnet_amd.layers import CostRegNet
    net, want = unet_net(C, zero_shift)
    net = copy.deepcopy(net)
    g = torch.Generator().manual_seed(9000 + C)
    with torch.no_grad():
        for name in CostRegNet.ENCODER + CostRegNet.DECODER:
            conv = getattr(net, name).conv
            w = two_piece(conv.weight.double(), 0 if isinstance(conv, nn.ConvTranspose3d) else 1, 0, g)
            assert torch.equal(w.float().double(), w)
            conv.weight.copy_(w)
    return net, want


PRESCALE_POWS = (-40, 20)      # batch element 0 * 2^-40, batch element 1 * 2^+20


@functools.lru_cache(maxsize=3)
def unet_split_fixture(C, shape, layer, scaled=False):
    """Layer `layer` of split_net(C) on two-piece input (odd channels) and a lattice skip. scaled: the zero-shift net,
    batch element b's input and skip times 2^PRESCALE_POWS[b]; the layer is homogeneous, so the reference is the
    unscaled float64 reference times the same power."""
    g = torch.Generator().manual_seed(7000 + C * 1000 + layer * 10 + UNET_SHAPES.index(shape))
    fx = L.unet_build(split_net(C, scaled), C, shape, layer, lambda x: two_piece(x, 1, 1, g))
    fx.pw = torch.tensor(PRESCALE_POWS if scaled else (0,) * B, dtype=torch.float64)
    if scaled:
        assert not bool(fx.shift.any())
        for n in ("x", "skip", "ref", "preact", "acc"):
            v = getattr(fx, n)
            if v is not None:
                setattr(fx, n, v * per_sample(2.0 ** fx.pw, v))
    fx.prescale = True
    # the shift belongs to the unscaled layer (scale folded into the weights by split_terms)
    fx.epi = dict(shift=fx.shift, res_pre=None, relu=True, res_post=fx.skip, post_up=1)
    return fx


# ---------------------------------------------------------------------------------------------- the CPU tests

UNET_GROUPS = [(C, s) for C in UNET_C for s in UNET_SHAPES]
FIXTURE_GROUPS = (["conv2d", "fpn_top", "bn_fold"] + ["unet_C%d_%dx%dx%d" % ((C,) + s) for C, s in UNET_GROUPS] +
                  ["prescale_C%d" % C for C in UNET_C])


@pytest.mark.parametrize("group", FIXTURE_GROUPS)
def test_two_piece_fixtures_are_exact(group):
    """Every case of the GPU tests below meets the conditions of check_two_piece, with the f16 pieces taken as the code
    takes them (hi = f16(v), lo = f16(v - hi); weights times the folded scale and the layer's 2^k of weight_pack.h
    split_exponent; U-Net activations times each batch element's prescale). The FPN top's packed weight halves are
    those of the lattice fixture (lo = 0). The zero-shift net folds to the lattice scales and a shift of exactly 0."""
    if group == "conv2d":
        for i in SPLIT_ROWS:
            check_two_piece("conv2d case %d" % i, conv2d_split_fixture(i))
    elif group == "fpn_top":
        from damvsnet_amd.frontend_hip import _fpn_top_A, pack_fpn_top_split
        for shp in FPN_SHAPES:
            fx, base = fpn_split_fixture(*shp), L.fpn_fixture(*shp)
            check_two_piece("fpn top %s" % (shp,), fx, weights=False)
            assert torch.equal(fx.prefix.float().double(), fx.prefix)   # the fused launch's store before the fix-up
            for n in ("wt", "wc", "bc", "corr"):
                assert torch.equal(getattr(fx, n), getattr(base, n)), n
            halves, ws = pack_fpn_top_split(fx.wt.float(), fx.wc.float())
            halves0, ws0 = pack_fpn_top_split(base.wt.float(), base.wc.float())
            assert torch.equal(halves, halves0) and ws == ws0
            halves = halves.view(torch.float16)
            assert not bool(halves[:, 1].any())
            assert torch.equal(halves[:, 0].float() * ws, _fpn_top_A(fx.wt.float(), fx.wc.float()))
    elif group == "bn_fold":
        import numpy as np
        from damvsnet_amd.layers import CostRegNet
        for C in UNET_C:
            for zero_shift in (False, True):
                net, want = split_net(C, zero_shift)
                for name in CostRegNet.ENCODER + CostRegNet.DECODER:
                    bn = getattr(net, name).bn
                    scale, shift = L.fold_bn_numpy(bn.weight.detach().numpy(), bn.bias.detach().numpy(),
                                                   bn.running_mean.numpy(), bn.running_var.numpy(), bn.eps)
                    assert np.array_equal(scale, want[name][0].numpy()), (C, name)
                    assert np.array_equal(shift, want[name][1].numpy()), (C, name)
                    assert set(np.unique(scale)) <= {0.5, 1.0, 2.0} and len(np.unique(scale)) == 3
                    if zero_shift:
                        assert not shift.any(), (C, name)
                    # the perturbation stays off the lattice net: same scales, weights differ by at most EPS
                    w0 = getattr(unet_net(C, zero_shift)[0], name).conv.weight.detach()
                    d = (getattr(net, name).conv.weight.detach().double() - w0.double()).abs()
                    assert set(d.unique().tolist()) == {0.0, EPS}, (C, name)
    elif group.startswith("unet"):
        C, shape = UNET_GROUPS[FIXTURE_GROUPS.index(group) - 3]
        for layer in range(10):
            fx = unet_split_fixture(C, shape, layer)
            check_two_piece("%s %s" % (group, fx.name), fx)
    else:
        C = int(group[len("prescale_C"):])
        for layer in range(10):
            fx = unet_split_fixture(C, SWITCH_SHAPE, layer, True)
            t = check_two_piece("%s %s" % (group, fx.name), fx)
            # what the test is about: unscaled, one sample's pieces leave the f16 range; with its own prescale the
            # pieces are those of the unscaled tensor
            assert float(fx.x[1].abs().max()) > 65504 and 0 < float(fx.x[0].abs().max()) < 2.0 ** -25
            assert all(2 ** 13 <= float(t.xv[b].abs().max()) < 2 ** 14 for b in range(B))


def test_one_dropped_lo_tap_passes_rel_max_but_not_equality():
    """Why this file exists: in the CPU three-term model of the 256 -> 256 3x3 layer, zero the lo piece of one weight
    tap. Equality with the float64 reference fails by at least one unit, while rel_max on the same pair stays under the
    2e-5 gate of test_conv2d_layer_vs_torch and test_costregnet_golden."""
    i = next(n for n, c in enumerate(CONV2D_CASES) if c[:12] == (False, 3, 1, 1, 0, 256, 0, (), 256, True, False, 0))
    fx = conv2d_split_fixture(i)
    t = split_terms(fx)
    wl = t.wl.clone()
    co, ci, ky, kx = (wl != 0).nonzero()[0].tolist()
    wl[co, ci, ky, kx] = 0.0
    wrong = layer_reference(t.hh + t.lh + fx.conv(t.xh, wl) * t.back, None, **fx.epi)[0]
    right = layer_reference(t.hh + t.lh + t.hl, None, **fx.epi)[0]
    assert torch.equal(right.float(), fx.ref.float())
    a, b = wrong.float(), fx.ref.float()
    assert not torch.equal(a, b)
    assert float((a.double() - b.double()).abs().max()) >= UNIT
    assert rel_max(a.numpy(), b.numpy()) < 2e-5


# ---------------------------------------------------------------------------------------------- the GPU tests

@pytest.mark.gpu
@pytest.mark.parametrize("i,off", CONV2D_RUNS,
                         ids=["%d%s" % (i, "".join("-%s=0" % sw[6:] for sw in off)) for i, off in CONV2D_RUNS])
def test_conv2d_layer_split_exact(i, off, _lib, monkeypatch):  # noqa: F811
    """Every form of test_gpu_frontend.CASES in fp32 on two-piece data, driven as test_conv2d_layer_exact drives it:
    equal to the float64 reference on the first cout channels, exactly 0 on the padded ones. Case 0 (16 -> 32, 3x3) is
    the smallest and runs first: it is also the check that the matrix core keeps an exact fp32 sum over the 23 bits
    these fixtures span. With DAMVS_CONV2D_G32=0 / DAMVS_PLANES_MFMA=0 the 16-K gather form and the VALU plane
    kernels meet the reference themselves (their sibling tests are tolerance tests)."""
    fx = conv2d_split_fixture(i)
    for sw in off:
        monkeypatch.setenv(sw, "0")
    default, key = ROUTES[route_cases.case_key(i, "f32")], route_cases.case_key(i, "f32", off)
    want = ROUTES.get(key, default)   # no entry: the switch does not reroute this row
    assert route_cases.case_route(i, "f32") == want, key
    assert key not in ROUTES or not off or want != default, key
    L.run_conv2d_layer(fx, F32, "conv2d case %s two-piece" % key, split_equal(fx))


@pytest.mark.gpu
@pytest.mark.parametrize("Bn,H,W", FPN_SHAPES)
def test_fpn_top_f32_split_exact(Bn, H, W, _lib):  # noqa: F811
    """damvs_fpn_top_forward_f32 + damvs_conv2d_border_bias, and the two-launch path, on two-piece activations against
    the unfused out3(up2(f) + inner2(c0)) in float64: equal at every pixel, the border ring and corners included."""
    fx = fpn_split_fixture(Bn, H, W)
    L.run_fpn_top(fx, Bn, H, W, F32, split_equal(fx))


_ENGINES = {}


def _engine(C, zero_shift=False):
    from damvsnet_amd.engine import StageEngine
    if (C, zero_shift) not in _ENGINES:
        _ENGINES[C, zero_shift] = StageEngine(split_net(C, zero_shift)[0], None, "variance", F32, torch.device(L.DEV))
    return _ENGINES[C, zero_shift]


# the fp32 forms that other shapes or configurations fall back to; the conv0 switches only move layer 0 (conv3d_route)
UNET_SWITCHES = (("DAMVS_CONV_NO_ZSLIDE", "1", range(10)), ("DAMVS_DECONV_NO_ZSLIDE", "1", range(10)),
                 ("DAMVS_CONV3D_K16", "1", range(10)), ("DAMVS_CONV0_DZ", "0", (0,)), ("DAMVS_CONV0_REUSE", "1", (0,)))
UNET_MODES = ("f32", "f32-slots")
# ordered so that the runs sharing a float64 reference follow each other (unet_split_fixture keeps the last few)
UNET_RUNS = [(C, shape, layer, mode, sw)
             for C in UNET_C for shape in UNET_SHAPES for layer in range(10)
             for sw in [None] + [s[:2] for s in UNET_SWITCHES if shape == SWITCH_SHAPE and layer in s[2]]
             for mode in UNET_MODES]


@pytest.mark.gpu
@pytest.mark.parametrize("C,shape,layer,mode,switch", UNET_RUNS,
                         ids=["C%d-%dx%dx%d-L%d-%s%s" % ((C,) + s + (l, m, "-%s=%s" % (sw[0][6:], sw[1]) if sw else ""))
                              for C, s, l, m, sw in UNET_RUNS])
def test_unet_layer_split_exact(C, shape, layer, mode, switch, _lib, monkeypatch):  # noqa: F811
    """damvs_costreg_layer_scaled in fp32, one layer at a time on its own two-piece input, against
    relu(conv3d * scale + shift) / relu(conv_transpose3d * scale + shift) + skip in float64: equal. With magnitude
    slots as test_unet_layer_exact runs them: the recorded output maximum equals max |ref| of each batch element, no
    other slot is written. Under the switches the tile, gather, 16-K and conv0 walk forms meet the reference
    themselves."""
    fx = unet_split_fixture(C, shape, layer)
    if switch:
        monkeypatch.setenv(*switch)
    L.run_unet_layer(_engine(C), fx.x, fx.skip, fx.ref, layer, shape, mode,
                     "C %d %s %s %s two-piece %s" % (C, shape, fx.name, mode, "=".join(switch) if switch else ""),
                     split_equal(fx))


@pytest.mark.gpu
@pytest.mark.parametrize("layer", range(10))
@pytest.mark.parametrize("C", UNET_C)
def test_unet_layer_prescale_exact_across_scales(C, layer, _lib):  # noqa: F811
    """The prescale's claim per layer and per sample: the zero-shift net's layers are homogeneous, so with batch element
    0's input (and skip) times 2^-40 and batch element 1's times 2^+20 in one launch, out[b] is ref * 2^p[b] bit for bit
    and the recorded maxima are exact. Unscaled, 2^21 overflows f16 and 2^-52 lies below its subnormal floor; with the
    other sample's slot one of the two happens."""
    fx = unet_split_fixture(C, SWITCH_SHAPE, layer, True)
    L.run_unet_layer(_engine(C, True), fx.x, fx.skip, fx.ref, layer, SWITCH_SHAPE, "f32-slots",
                     "C %d %s %s two-piece, batch elements * 2^%d / 2^%d" % ((C, SWITCH_SHAPE, fx.name) + PRESCALE_POWS),
                     split_equal(fx))
