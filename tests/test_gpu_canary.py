"""GPU: no kernel writes outside the tensors it is given.

Every output (U-Net level tensors, the warp's volume, the stage workspace and the stage's depth / confidence /
variance / probability outputs) is placed inside a larger buffer whose head and tail hold a byte pattern; after the
launch both guard bands must be intact. A write past a tensor's end lands in whatever the caching allocator put
next to it -- in the concurrent-stream forward that can be another sub-batch's live tensor -- and the parity tests,
which compare only the tensors themselves, cannot see it.
"""
import ctypes

import pytest
import torch

from common import model_state

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 1 << 16  # bytes before and after each output
PATTERN = 0x5A


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from damvsnet_amd import _capi
    _capi.load_library()


class Guarded:
    """A tensor of `shape` / `dtype` inside a guard-banded byte buffer."""

    def __init__(self, shape, dtype, init=None):
        n = torch.empty((), dtype=dtype).element_size()
        for d in shape:
            n *= d
        self.n = n
        self.buf = torch.full((GUARD + n + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
        self.t = self.buf[GUARD:GUARD + n].view(dtype).view(*shape)
        if init is not None:
            self.t.copy_(init)

    def check(self, what):
        torch.cuda.synchronize()
        head = self.buf[:GUARD] != PATTERN
        tail = self.buf[GUARD + self.n:] != PATTERN
        assert not bool(head.any()), "%s: %d bytes written before the tensor (nearest at -%d)" % (
            what, int(head.sum()), GUARD - int(head.nonzero().max()))
        assert not bool(tail.any()), "%s: %d bytes written past the end (first at +%d)" % (
            what, int(tail.sum()), int(tail.nonzero().min()))


# (stage index, C, D, h, w): the three stages at cfgC's channel widths and depths, at sizes that are multiples of 8
# but not of the kernels' tile sizes, and at
# stage 2's full cfgC size (the layer shapes of the concurrent-stream test)
CASES = [(0, 32, 48, 40, 72), (1, 16, 32, 56, 88), (2, 8, 8, 24, 104), (1, 16, 32, 592, 800)]
SRC = (None, 0, 1, 2, 3, 4, 5, 6, 4, 2)
DST = (0, 1, 2, 3, 4, 5, 6, 4, 2, 0)


def _net(dtype):
    from damvsnet_amd.cascade import CascadeMVSNet
    net = CascadeMVSNet(ndepths=[48, 32, 8], compute_dtype=dtype)
    net.load_state_dict(model_state("depthnet_cfgA_adaptive"), strict=True)
    return net.to(DEV).eval()


def _inputs(s, C, D, h, w, B, N, dtype):
    from damvsnet_amd import synth
    from damvsnet_amd.engine import hypotheses
    H, W = h * (4 >> s), w * (4 >> s)
    proj, _, dv = synth.cameras(B, N, H, W)
    P = torch.from_numpy(proj["stage%d" % (s + 1)]).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(s)
    if s == 0:
        hyps = hypotheses(torch.from_numpy(dv).to(DEV), D, H, W, 4)
    else:
        pd = 600 + 100 * torch.rand(B, H // 4, W // 4, device=DEV, generator=g)
        pv = 5 + 20 * torch.rand(B, H // 4, W // 4, device=DEV, generator=g)
        hyps = hypotheses(torch.from_numpy(dv).to(DEV), D, H, W, 4 >> s, pd, pv)
    feats = [torch.randn(B, h, w, C, generator=g, device=DEV).to(dtype) for _ in range(N)]
    return P, hyps, feats


@pytest.mark.timeout(240)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "s%d_%dx%d" % (c[0], c[3], c[4]))
def test_unet_layers_and_warp_write_inside_their_outputs(case, dtype):
    s, C, D, h, w = case
    B, N = 2, 5
    net = _net(dtype)
    eng = net.DepthNet.engine(s, net.cost_regularization[s], torch.device(DEV))
    P, hyps, feats = _inputs(s, C, D, h, w, B, N, dtype)
    with torch.no_grad():
        vol = Guarded((B, D, h, w, C), dtype)
        eng.warp_aggregate(feats, P, hyps, out=vol.t)
        vol.check("warp_aggregate NHWC")
        from damvsnet_amd import _capi
        from damvsnet_amd.engine import block_channels
        volb = Guarded((B, D, h, w, C), dtype)
        eng.warp_aggregate(block_channels(feats), P, hyps, layout=_capi.DAMVS_LAYOUT_CBLOCK, out=volb.t)
        volb.check("warp_aggregate channel-blocked")
        bufs = eng.unet_buffers(B, D, h, w)
        g = torch.Generator(device=DEV).manual_seed(1)
        for b in bufs:  # the deconvs add into their outputs: start from finite values
            b.copy_(torch.randn(b.shape, generator=g, device=DEV).to(dtype))
        for layer in range(10):
            src = vol.t if layer == 0 else bufs[SRC[layer]]
            dst = Guarded(bufs[DST[layer]].shape, dtype, init=bufs[DST[layer]])
            eng.unet_layer(layer, D, h, w, src, dst.t)
            dst.check("U-Net layer %d" % layer)
            bufs[DST[layer]] = dst.t


@pytest.mark.timeout(240)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("case", CASES[:3], ids=lambda c: "s%d_%dx%d" % (c[0], c[3], c[4]))
def test_stage_forward_writes_inside_workspace_and_outputs(case, dtype):
    from damvsnet_amd import _capi
    s, C, D, h, w = case
    B, N = 2, 5
    net = _net(dtype)
    eng = net.DepthNet.engine(s, net.cost_regularization[s], torch.device(DEV))
    P, hyps, feats = _inputs(s, C, D, h, w, B, N, dtype)
    lib = _capi.load_library()
    n = ctypes.c_size_t()
    assert lib.damvs_stage_workspace_size(eng.handle, B, N, D, h, w, ctypes.byref(n)) == 0
    ws = Guarded((n.value,), torch.uint8)
    outs = {k: Guarded((B, h, w), torch.float32) for k in ("depth", "conf", "var")}
    prob = Guarded((B, D, h, w), torch.float32)
    fptrs = (ctypes.c_void_p * N)(*[f.data_ptr() for f in feats])
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    with torch.no_grad():
        for prob_init in (None, torch.rand(B, D, h, w, device=DEV)):
            rc = lib.damvs_stage_forward(eng.handle, _capi.stream_ptr(torch.device(DEV)), B, N, D, h, w, fptrs, p(P),
                                         p(hyps), p(prob_init) if prob_init is not None else None, p(ws.t), ws.n,
                                         p(outs["depth"].t), p(outs["conf"].t), p(outs["var"].t), p(prob.t))
            _capi.check(rc)
            ws.check("stage workspace")
            for k, o in outs.items():
                o.check(k)
            prob.check("prob_volume")


# ---------------------------------------------------------------------------------------------- 2D front-end
import route_cases  # noqa: E402
import test_gpu_frontend as FE  # noqa: E402
from test_gpu_lattice import FPN_SHAPES  # noqa: E402

DT_IDS = {torch.bfloat16: "bf16", torch.float32: "f32"}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("i", range(len(FE.CASES)))
def test_conv2d_layers_write_inside_their_outputs(i, dtype):
    """Every row of test_gpu_frontend.CASES (each 2D kernel family, ragged tiles, channel tails, cout padded to 4) with
    its output inside guard bands; inputs and residuals are ordinary tensors."""
    from damvsnet_amd.frontend_hip import planes
    case = FE.CASES[i]
    c0, c1, geo, pre, post_up = case[5], case[6], case[7], case[10], case[11]
    H, W = route_cases.case_size(case)
    B = route_cases.B
    L = route_cases.case_layer(case, dtype)
    shape = L.out_shape(B, H, W)
    g = torch.Generator(device=DEV).manual_seed(i)
    rnd = lambda *s: torch.randn(*s, generator=g, device=DEV).to(dtype)  # noqa: E731
    out = Guarded(shape, dtype)
    L(B, H, W, rnd(B, H, W, c0) if c0 else None, rnd(B, H, W, c1) if c1 else None,
      geo=planes(torch.randn(B, len(geo), H, W, generator=g, device=DEV)) if geo else (),
      res_pre=rnd(*shape) if pre else None,
      res_post=rnd(B, shape[1] // post_up, shape[2] // post_up, shape[3]) if post_up else None,
      post_up=max(post_up, 1), out=out.t)
    out.check("conv2d case %d %s (%s)" % (i, DT_IDS[dtype], L.route(B, H, W)))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("Bn,H,W", FPN_SHAPES)
def test_fpn_top_writes_inside_its_output(Bn, H, W, dtype):
    """damvs_fpn_top_forward / damvs_fpn_top_forward_f32, then damvs_conv2d_border_bias on the same guarded output."""
    import torch.nn as nn
    from damvsnet_amd import _capi
    from damvsnet_amd.engine import DTYPES
    from damvsnet_amd.frontend_hip import fpn_top_layers, pack_fpn_top, pack_fpn_top_split
    g = torch.Generator().manual_seed(H * W)
    inner2, out3 = nn.Conv2d(8, 32, 1, bias=True), nn.Conv2d(32, 8, 3, padding=1, bias=False)
    with torch.no_grad():
        for m in (inner2, out3):
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) * 0.2)
    _, _, corr, (wt, wc, bc) = fpn_top_layers(inner2, out3, dtype)
    c0 = torch.randn(Bn, H, W, 8, generator=g).to(DEV, dtype)
    f = torch.randn(Bn, H // 2, W // 2, 32, generator=g).to(DEV, dtype)
    bd = bc.float().to(DEV)
    lib = _capi.load_library()
    o = Guarded((Bn, H, W, 8), dtype)
    st = _capi.stream_ptr(torch.device(DEV))
    if dtype == torch.bfloat16:
        ap = pack_fpn_top(wt, wc).to(DEV)
        _capi.check(lib.damvs_fpn_top_forward(st, Bn, H, W, c0.data_ptr(), f.data_ptr(), ap.data_ptr(), bd.data_ptr(),
                                              o.t.data_ptr()))
    else:
        ap, ws = pack_fpn_top_split(wt, wc)
        ap = ap.to(DEV)
        _capi.check(lib.damvs_fpn_top_forward_f32(st, Bn, H, W, c0.data_ptr(), f.data_ptr(), ap.data_ptr(), ws,
                                                  bd.data_ptr(), o.t.data_ptr()))
    o.check("fpn top %s" % DT_IDS[dtype])
    _capi.check(lib.damvs_conv2d_border_bias(st, DTYPES[dtype], Bn, H, W, 8, 8, _capi.float_ptr(corr), o.t.data_ptr()))
    o.check("fpn top border fix-up %s" % DT_IDS[dtype])


@pytest.mark.parametrize("hw", [(37, 51), (8, 9)])
@pytest.mark.parametrize("masked", [False, True], ids=["basic", "mean"])
def test_sparse_depth_pyramid_writes_inside_its_outputs(hw, masked):
    """damvs_sparse_depth_pyramid at odd sizes and at the smallest one: the four levels and the scratch, at exactly the
    size include/damvs.h asks for, each inside guard bands."""
    from damvsnet_amd import _capi
    h, w = hw
    Bn = 3
    g = torch.Generator(device=DEV).manual_seed(h * w)
    depth = 425 + 500 * torch.rand(Bn, h, w, generator=g, device=DEV)
    depth[:, : h // 3] = 300.0
    dv = torch.stack([torch.linspace(425, 935, 48), torch.linspace(400, 900, 48), torch.linspace(500, 1000, 48)]).to(DEV)
    mask = (torch.rand(Bn, h, w, generator=g, device=DEV) > 0.5).float() if masked else None
    outs = [Guarded((Bn, h >> l, w >> l), torch.float32) for l in range(4)]
    scratch = Guarded((Bn * (h // 2) * (w // 2) + Bn * (h // 4) * (w // 4),), torch.float32)
    lib = _capi.load_library()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    _capi.check(lib.damvs_sparse_depth_pyramid(_capi.stream_ptr(torch.device(DEV)), Bn, h, w, p(depth), p(dv), 48,
                                               p(mask) if masked else None, *[p(o.t) for o in outs], p(scratch.t)))
    for l, o in enumerate(outs):
        o.check("sparse pyramid level %d" % l)
    scratch.check("sparse pyramid scratch")
