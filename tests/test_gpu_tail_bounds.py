"""Per-pixel bounded tests for the tail of a stage (csrc/k_regress.hip: the prob conv in its four product forms, the
softmax, depth, confidence and exp-variance) and for the hypothesis generators that consume its outputs
(csrc/k_geometry.hip: hyp_linear_kernel, hyp_refine_kernel).

Tail. The fixtures make the conv exact: on c0 and prob.weight below every product and every partial sum, in any order,
is exact in fp32, and so are the bf16 hi + lo split of the weights and the f16 hi + lo splits of weights and
activations; prob_init holds multiples of 1/4. The logits a kernel holds then equal the float64 conv bit for bit, and
every pixel must satisfy |got - ref| <= bound for prob (per plane), depth, confidence and variance, where ref is a
float64 numpy evaluation of models/cas_mvsnet.py:105-124 (oracle.regression) on those logits and the float32
hypotheses, and bound is a first-order model of a float32 evaluation, u = 2^-24:

  e_d = expf(l_d - mx)    the argument is exact; relative error c_exp u
  S = sum e_d             positive terms: c_exp u + (D-1) u
  p_d = e_d / S           eps_p = 2 c_exp u + (D+1) u            (+ 2^-126 absolute: results below the normal range)
  depth, idx              sum |p_d h_d| (eps_p + (D+1) u), and the same with d in place of h_d (delta, below)
  variance                d_df = d_depth + u |df| for df = h_d - depth, d_vs = sum p_d (2 |df| d_df + d_df^2)
                          + vs (eps_p + (D+2) u), d_var = min(3 d_vs / (2 sqrt(vs)), 3 sqrt(d_vs)) + 2u var
  confidence              (eps_p + 3u) conf

c_exp: the ROCm installation carries no document that states the accuracy of expf, so the fallback of 2 ulp is
used: c_exp u = 2 ulp = 4u (C_EXP_ULP below). No constant of the model was raised after the first GPU run.

Window rule, from the reference alone: where the float64 idx lies within delta of an integer r the confidence may
match the window of i* = r - 1 or of i* = r; elsewhere it must match the window of trunc(idx). At most 1 % of the
pixels of any case are ambiguous (asserted on the CPU; the largest share is 0.94 %, at base 16 and D = 120, where the
sharper logits of 16 channels put more idx next to an integer; 0.5 % and less at base 8 and D = 144). An exactly one-hot
pixel is not ambiguous: its idx is the integer itself in float32 too.

Fixtures (B = 2, everything distinct per batch element and per pixel):
  wide-weights  c0 in +-{1, 1.5, 2} at density 0.5, weights +-{2^-3, 2^-2} (1 + 2^-12) at density 0.5: every non-zero
                weight needs both bf16 terms and both f16 halves (bf16 and fp32 storage)
  wide-acts     c0 in +-({1, 2} + 2^-10), weights +-{2^-3, 2^-2} (fp32 storage: prob_mfma_kernel<float> drops lo x lo
                by design). 1 + 2^-10 is itself an f16 value, so it is the activations of magnitude 2 + 2^-10, half of
                the non-zero ones, whose f16 split has lo = 2^-10 (a normal f16); the CPU test asserts that share.
  prob_init     -0.75 min(|d - t|, 32) for a per-pixel target plane t, forced to 0, D-2 and D-1 on 15 % of the pixels
                each; three one-hot pixels per batch element (-2^13 off one plane, plane D-1 among them). For the
                float32 round trip of logits + init to be the identity there too, c0 is zero in the 3 x 3
                neighbourhood of a one-hot pixel (its conv logits are exactly 0).

Routes (regress_tail, restated in route() and asserted by test_route_table):

  storage, base   switch               fused up to   kernel                         first two-pass D
  bf16, 8         default              D = 144       prob_mfma<bf16>                152
  bf16, 8         DAMVS_PROB_MFMA=0    136           prob_regress<bf16,8,false>     144
  fp32, 8         default              136           prob_regress<float,8,false>    144
  fp32, 8         DAMVS_PROB_MFMA=1    136           prob_mfma<float>               144
  bf16 / fp32, 16 -                    112           prob_regress<T,16,false>       120

each at (D, h, w) = (8, 8, 8), (16, 16, 40), (48, 24, 72), (largest fused D, 8, 40) and (first two-pass D, 8, 40: the
same conv with TWO = true, then regress_kernel), with and without prob_init, fp32 rows on both fixtures; damvs_regress
alone on lattice logits at (5, 3, 7), (32, 24, 40), (1, 3, 7), (2, 3, 7) and (9, 8, 40).

Hypotheses. ref is oracle.stage_hypotheses on float64 tensors; the bound is a first-order float32 model of
hyp_refine_kernel per full-resolution point (hyp_reference): the bilinear taps of the previous depth and variance
(4u sum |w_k m_k| each), low, step = (var - low) / (D - 1), the softmax logits x_i = 3 (low + step i) / (var + eps),
__expf as exp2(y log2 e) (relative error d_y + (2 |y| + 2) u: it grows with |y|), the softmax offset times step, the
adds of cur + low + step i + eps at their magnitudes, and the 2 x 2 average at scale 2 (+ 2u |out|). The previous
variance comes in four regimes, in column bands: 0 exactly, 1e-6, var > depth (low = -cur) and var < depth.
hyp_linear_kernel is held to 3u d itv + u |out|.

CPU part (not marked gpu): the fixture conditions, the ambiguity cap, the route table, float32 restatements staying
inside the bounds (the gates are not too tight), every simulated defect falling outside them (not too loose), and
test_zeroed_tap_against_the_old_gate.

Measured on an MI355X (profiles/r09/pytest_gpu_tail_bounds.txt), largest |got - ref| / bound per route over its cases,
against the float64 reference; no constant of either model was raised and no kernel defect was found. A kernel trace
per row (profiles/r09/tail_route_kernels.txt) shows each row launching the kernel the table names.

  route                              prob    depth   conf    var      r10: prob    depth   conf    var
  prob_mfma<bf16>                    0.340   0.201   0.226   0.021         0.340   0.201   0.226   0.021
  prob_regress<bf16,8,false>         0.340   0.201   0.226   0.021         0.340   0.201   0.226   0.021
  prob_regress<float,8,false>        0.340   0.201   0.302   0.021         0.340   0.201   0.302   0.021
  prob_mfma<float>                   0.340   0.201   0.302   0.021         0.340   0.201   0.302   0.021
  prob_regress<bf16,16,false>        0.263   0.167   0.200   0.017         0.263   0.167   0.200   0.017
  prob_regress<float,16,false>       0.300   0.224   0.236   0.017         0.300   0.224   0.235   0.017
  two-pass bf16 / fp32, base 8       0.102   0.063   0.089   0.005         0.102   0.063   0.088   0.005
  two-pass bf16 / fp32, base 16      0.104   0.062   0.085   0.004         0.104   0.062   0.085   0.004
  regress_kernel alone               0.190   0.118   0.172   0.021         0.269   0.221   0.204   0.025

  r10 (profiles/r10/pytest_gpu_tail_bounds.txt): the three kernels on one regression body (regress_column). Every
  output of every case above is bitwise the r09 build's (profiles/r10/tail_share_gpu.md; the last digits that differ
  are the rounding of a maximum over lines printed to four places); regress_kernel alone moves with its three added
  shapes, (9, 8, 40) giving its largest prob, depth and conf ratios and (2, 3, 7) its largest var ratio.

  (equal figures across rows are expected: the logits are exact, so the rows differ only where their regression
  code or their cases do)

  hyp_refine_kernel   var < depth 0.436   var > depth 0.215   var = 0 0.246   var = 1e-6 0.248   mixed 0.225
  hyp_linear_kernel   D = 8 0.351         D = 48 0.779

Base 16: damvs_stage_create accepts CostRegNet(8, 16), and prob_regress<T,16,false> and the base-16 two-pass form meet
the same bounds in both storage types; it is not refused.
"""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_max, pixel_rel
from common import model_state
from oracle import mvs_oracle as O
from test_gpu_lattice import lattice

DEV = "cuda"
U = 2.0 ** -24
BF16, F32 = torch.bfloat16, torch.float32
B = 2
SEED = 5                   # of the tail fixtures (changed until every case meets test_fixture_conditions)
C_EXP_ULP = 2.0            # accuracy assumed for expf, in ulp (the fallback: no installed ROCm document states it)
C_EXP = 2.0 * C_EXP_ULP    # the same in units of u = ulp / 2
TINY = 2.0 ** -126         # smallest normal float32: a result below it may be flushed
LDS_LIMIT = 163840         # bytes of LDS a block may ask for (regress_tail: 160 * 1024)
E_SHAPE, E_WORKSPACE = -2, -6

ACT_WIDE_W = (-2.0, -1.5, -1.0, 1.0, 1.5, 2.0)
ACT_WIDE_A = (-2.0, -1.0, 1.0, 2.0)      # + sign * 2^-10
WGT = (-0.25, -0.125, 0.125, 0.25)       # x (1 + 2^-12) on the wide-weights fixture
UNIT = {"weights": 2.0 ** -16, "acts": 2.0 ** -13}   # lattice unit of the products


@pytest.fixture(scope="module")
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from damvsnet_amd import build, _capi
    build.build()
    _capi.load_library()


# ---------------------------------------------------------------------------------------------- tail fixtures

@functools.lru_cache(maxsize=None)
def prob_weight(kind, base):
    """float64 prob.weight [1][base][3][3][3] of a fixture kind (one per (kind, base): a stage holds its weights)."""
    g = torch.Generator().manual_seed(500 + base + (1000 if kind == "acts" else 0))
    w = lattice((1, base, 3, 3, 3), WGT, 0.5, g)
    return w * (1.0 + 2.0 ** -12) if kind == "weights" else w


def one_hot_pixels(D, h, w):
    """(b, y, x, plane) of the exact one-hot pixels: two corners and the centre, plane D-1 in both batch elements."""
    return [(0, 0, 0, D - 1), (0, h - 1, w - 1, 0), (0, h // 2, w // 2, D - 1),
            (1, 0, 0, D - 2), (1, h - 1, w - 1, D - 1), (1, h // 2, w // 2, 1)]


def target_init(D, h, w, g):
    """(t, init): the per-pixel target plane and init[d] = -0.75 min(|d - t|, 32) (multiples of 1/4)."""
    r = torch.rand((B, h, w), generator=g)
    t = torch.randint(D, (B, h, w), generator=g)
    t[r < 0.15] = 0
    t[(r >= 0.15) & (r < 0.30)] = D - 2
    t[(r >= 0.30) & (r < 0.45)] = D - 1
    d = torch.arange(D).view(1, D, 1, 1)
    init = -0.75 * (d - t.unsqueeze(1)).abs().clamp(max=32).double()
    return t, init


def sorted_hyps(D, h, w, g):
    return torch.sort(450.0 + 300.0 * torch.rand((B, D, h, w), generator=g), dim=1).values.float()


def prob_conv(c0, wt):
    """float64 Conv3d(base, 1, k3, p1) of c0 [B][D][h][w][base] -> [B][D][h][w]."""
    return F.conv3d(c0.permute(0, 4, 1, 2, 3), wt, padding=1)[:, 0]


@functools.lru_cache(maxsize=None)
def tail_fixture(kind, base, D, h, w):
    g = torch.Generator().manual_seed(SEED + 100003 * D + 1009 * h + 13 * w + base + (5 if kind == "acts" else 0))
    if kind == "weights":
        c0 = lattice((B, D, h, w, base), ACT_WIDE_W, 0.5, g)
    else:
        c0 = lattice((B, D, h, w, base), ACT_WIDE_A, 0.5, g)
        c0 = c0 + torch.sign(c0) * 2.0 ** -10
    hot = one_hot_pixels(D, h, w)
    for b, y, x, _ in hot:
        c0[b, :, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = 0.0
    wt = prob_weight(kind, base)
    t, init = target_init(D, h, w, g)
    for b, y, x, plane in hot:
        init[b, :, y, x] = -2.0 ** 13
        init[b, plane, y, x] = 0.0
    return types.SimpleNamespace(kind=kind, base=base, D=D, h=h, w=w, c0=c0, wt=wt, logits=prob_conv(c0, wt),
                                 absum=prob_conv(c0.abs(), wt.abs()), t=t, init=init, hot=hot,
                                 hyps=sorted_hyps(D, h, w, g), unit=UNIT[kind])


@functools.lru_cache(maxsize=None)
def logits_fixture(D, h, w):
    """Lattice logits for damvs_regress alone: multiples of 1/4 around the same target planes (no conv)."""
    g = torch.Generator().manual_seed(31 + 1000 * D + w)
    t, init = target_init(D, h, w, g)
    noise = (torch.randn((B, D, h, w), generator=g, dtype=torch.float64) * 2.2 * 4).round() / 4
    return types.SimpleNamespace(D=D, h=h, w=w, t=t, logits=noise + init, hyps=sorted_hyps(D, h, w, g), hot=[])


def exact_logits(fx, with_init, defect=None):
    """float64 logits (+ prob_init) of a tail fixture, numpy [B][D][h][w]; defect: None or a simulated conv defect."""
    wt, init = fx.wt, fx.init
    if defect == "zero_tap":       # the first non-zero tap dropped
        wt = wt.clone()
        wt.view(-1)[int(wt.view(-1).nonzero()[0])] = 0.0
    elif defect == "drop_lo":      # the second bf16 term of the weights dropped
        wt = wt.float().to(BF16).double()
    lg = fx.logits if wt is fx.wt else prob_conv(fx.c0, wt)
    if with_init:
        if defect == "init_shift":   # prob_init of plane d added to plane d - 1
            init = torch.cat([init[:, 1:], torch.zeros_like(init[:, :1])], 1)
        lg = lg + init
    return lg.numpy()


# ---------------------------------------------------------------------------------------------- tail reference + gate

def _window(p, ii, D, mode=None):
    """sum of p over [ii - 1, ii + 2] clipped to the volume; mode "short": [ii - 1, ii + 1]; "clamp": the four indices
    clamped into the volume instead (a border plane counted more than once)."""
    if mode == "clamp":
        return sum(np.take_along_axis(p, np.clip(ii + k, 0, D - 1)[:, None], 1)[:, 0] for k in (-1, 0, 1, 2))
    d = np.arange(D).reshape((1, D) + (1,) * (p.ndim - 2))
    hi = ii + (1 if mode == "short" else 2)
    return (p * ((d >= (ii - 1)[:, None]) & (d <= hi[:, None]))).sum(1)


def regress_reference(lg, hyps, defect=None):
    """float64 models/cas_mvsnet.py:105-124 on logits lg [B][D][...] and hypotheses, with the per-element bounds of the
    module docstring. defect: None or "window_short", "window_clamp", "round_idx", "max_skip_last", "batch_hyps"."""
    lg = np.asarray(lg, np.float64)
    hy = np.asarray(hyps, np.float64)
    D = lg.shape[1]
    dd = np.arange(D, dtype=np.float64).reshape((1, D) + (1,) * (lg.ndim - 2))
    if defect == "batch_hyps":
        hy = hy.copy()
        hy[1] = hy[0]
    mx = (lg[:, :D - 1] if defect == "max_skip_last" else lg).max(1, keepdims=True)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(lg - mx)
        p = e / e.sum(1, keepdims=True)
        eps_p = (2 * C_EXP + D + 1) * U
        eps_s = eps_p + (D + 1) * U
        depth = (p * hy).sum(1)
        idx = (p * dd).sum(1)
        clip = lambda a: np.clip(np.nan_to_num(a), 0, D - 1).astype(np.int64)  # noqa: E731
        ii = clip(np.floor(idx + 0.5) if defect == "round_idx" else np.floor(idx))
        mode = {"window_short": "short", "window_clamp": "clamp"}.get(defect)
        conf = _window(p, ii, D, mode)
        df = hy - depth[:, None]
        vs = (df * df * p).sum(1)
        var = 3.0 * np.sqrt(vs)
        b_depth = np.abs(p * hy).sum(1) * eps_s
        delta = idx * eps_s
        d_df = b_depth[:, None] + U * np.abs(df)
        d_vs = (p * (2 * np.abs(df) * d_df + d_df ** 2)).sum(1) + vs * (eps_p + (D + 2) * U)
        first = np.where(vs > 0, 3 * d_vs / (2 * np.sqrt(np.where(vs > 0, vs, 1.0))), np.inf)
        b_var = np.minimum(first, 3 * np.sqrt(d_vs)) + 2 * U * var
        r = np.floor(idx + 0.5)
        amb = (np.abs(idx - r) <= delta) & (p.max(1) < 1.0)   # an exactly one-hot pixel: idx is exact in float32 too
        conf_alt = (_window(p, clip(r - 1), D), _window(p, clip(r), D))
    return types.SimpleNamespace(D=D, prob=p, depth=depth, conf=conf, var=var, idx=idx, ii=ii, b_prob=eps_p * p + TINY,
                                 b_depth=b_depth, b_var=b_var, conf_rel=eps_p + 3 * U, amb=amb, conf_alt=conf_alt,
                                 delta=delta)


def _ratio(got, ref, bound):
    """|got - ref| / bound; NaN or inf in got gives inf."""
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(np.asarray(got, np.float64) - ref) / bound
    return np.where(np.isfinite(r), r, np.inf)


def tail_ratios(got, R):
    """Per-pixel |got - ref| / bound of each output present in got (prob: the largest over the planes). The
    confidence of an ambiguous pixel takes the better of its two admissible windows."""
    out = {}
    if got.get("prob") is not None:
        out["prob"] = _ratio(got["prob"], R.prob, R.b_prob).max(1)
    out["depth"] = _ratio(got["depth"], R.depth, R.b_depth)
    out["var"] = _ratio(got["var"], R.var, R.b_var)
    c = _ratio(got["conf"], R.conf, R.conf_rel * R.conf)
    alt = np.minimum(*(_ratio(got["conf"], a, R.conf_rel * a) for a in R.conf_alt))
    out["conf"] = np.where(R.amb, np.minimum(c, alt), c)
    return out


def failing_pixels(got, R):
    """bool [B][...]: pixels with any output beyond its bound."""
    return functools.reduce(np.logical_or, [~(r <= 1.0) for r in tail_ratios(got, R).values()])


def as_got(R):
    return {"prob": R.prob, "depth": R.depth, "conf": R.conf, "var": R.var}


def regress_f32(lg, hyps):
    """The regression restated in float32 numpy, sequential sums in plane order (what regress_kernel does)."""
    f = np.float32
    lg, hy = np.asarray(lg).astype(f), np.asarray(hyps).astype(f)
    D = lg.shape[1]
    mx = lg.max(1)
    e = np.exp((lg - mx[:, None]).astype(f)).astype(f)
    s = np.zeros_like(mx)
    for d in range(D):
        s = (s + e[:, d]).astype(f)
    p = (e / s[:, None]).astype(f)
    dep, idx = np.zeros_like(mx), np.zeros_like(mx)
    for d in range(D):
        dep = (dep + (p[:, d] * hy[:, d]).astype(f)).astype(f)
        idx = (idx + (p[:, d] * f(d)).astype(f)).astype(f)
    ii = np.clip(idx.astype(np.int64), 0, D - 1)
    c, vs = np.zeros_like(mx), np.zeros_like(mx)
    for d in range(D):
        df = (hy[:, d] - dep).astype(f)
        vs = (vs + ((df * df).astype(f) * p[:, d]).astype(f)).astype(f)
        c = np.where((d >= ii - 1) & (d <= ii + 2), (c + p[:, d]).astype(f), c)
    return {"prob": p, "depth": dep, "conf": c, "var": (f(3.0) * np.sqrt(vs)).astype(f)}


@functools.lru_cache(maxsize=None)
def tail_reference(kind, base, D, h, w, with_init):
    fx = tail_fixture(kind, base, D, h, w)
    return regress_reference(exact_logits(fx, with_init), fx.hyps.numpy())


# ---------------------------------------------------------------------------------------------- routes and cases

def prob_mfma_smem(bf16, D):
    return 2 * 340 * 16 * (1 if bf16 else 2) + D * 256 * 4


def prob_regress_smem(base, D):
    return 2 * 340 * base * 4 + (D - 1) * 256 * 4


def prob_mfma_enabled(bf16, switch):
    if switch is not None and switch[:1] == "0":
        return False
    return bf16 or (switch is not None and switch[:1] == "1")


def route(bf16, base, D, switch=None):
    """capi.cpp regress_tail restated: the kernel a stage of this storage type and base runs at D planes."""
    T = "bf16" if bf16 else "float"
    if base == 8 and prob_mfma_smem(bf16, D) <= LDS_LIMIT and prob_mfma_enabled(bf16, switch):
        return "prob_mfma<%s>" % T
    if prob_regress_smem(base, D) <= LDS_LIMIT:
        return "prob_regress<%s,%d,false>" % (T, base)
    return "two-pass"


Row = types.SimpleNamespace
ROWS = [Row(id="bf16-8-mfma", bf16=True, base=8, switch=None, kernel="prob_mfma<bf16>", fused=144, two=152),
        Row(id="bf16-8-valu", bf16=True, base=8, switch="0", kernel="prob_regress<bf16,8,false>", fused=136, two=144),
        Row(id="f32-8-valu", bf16=False, base=8, switch=None, kernel="prob_regress<float,8,false>", fused=136, two=144),
        Row(id="f32-8-mfma", bf16=False, base=8, switch="1", kernel="prob_mfma<float>", fused=136, two=144),
        Row(id="bf16-16", bf16=True, base=16, switch=None, kernel="prob_regress<bf16,16,false>", fused=112, two=120),
        Row(id="f32-16", bf16=False, base=16, switch=None, kernel="prob_regress<float,16,false>", fused=112, two=120)]
BITWISE_SHAPE = (16, 16, 40)
# (1, 3, 7): the window clipped on both sides, only the last plane; (2, 3, 7): the smallest D with two planes;
# (9, 8, 40): one full group of 8 hypothesis loads plus one (the fused routes only ever see D % 8 == 0)
REGRESS_ONLY = ((5, 3, 7), (32, 24, 40), (1, 3, 7), (2, 3, 7), (9, 8, 40))


def row_shapes(row):
    return [(8, 8, 8), (16, 16, 40), (48, 24, 72), (row.fused, 8, 40), (row.two, 8, 40)]


def row_kinds(row):
    return ("weights",) if row.bf16 else ("weights", "acts")


CASES = [(row, kind, shape, with_init) for row in ROWS for kind in row_kinds(row) for shape in row_shapes(row)
         for with_init in (False, True)]
FIXTURES = sorted({(kind, row.base) + shape for row, kind, shape, _ in CASES})


def case_id(c):
    row, kind, (D, h, w), with_init = c
    return "%s-%s-D%d-%dx%d%s" % (row.id, kind, D, h, w, "-init" if with_init else "")


# ---------------------------------------------------------------------------------------------- CPU tests: tail

def f16_split(x):
    """(hi, lo) of the f16 split of float32 values (damvs_device.h split8), as float64."""
    x = np.asarray(x, np.float32)
    hi = x.astype(np.float16)
    return hi.astype(np.float64), (x - hi.astype(np.float32)).astype(np.float16).astype(np.float64)


def edge_shares(R, hot):
    n = R.ii.size
    on_last = sum(1 for b, y, x, plane in hot if plane == R.D - 1 and R.ii[b, y, x] == R.D - 1)
    return float((R.ii == 0).sum()) / n, float((R.ii >= R.D - 2).sum()) / n, on_last


@pytest.mark.parametrize("fixt", FIXTURES, ids=["%s-b%d-D%d-%dx%d" % f for f in FIXTURES])
def test_fixture_conditions(fixt):
    """The conditions that make the logits exact and the cases live (conditions, not measurements)."""
    kind, base, D, h, w = fixt
    fx = tail_fixture(*fixt)
    # 1. every partial sum is exact: the sum of |terms| stays below 2^24 lattice units, the logits lie on the lattice
    assert float(fx.absum.max()) / fx.unit < 2 ** 24, float(fx.absum.max()) / fx.unit
    assert torch.equal((fx.logits / fx.unit).round() * fx.unit, fx.logits)
    # 2. logits (+ init) survive float32; c0 survives its storage type
    for with_init in (False, True):
        lg = exact_logits(fx, with_init)
        assert np.array_equal(lg.astype(np.float32).astype(np.float64), lg)
    assert torch.equal(fx.c0.float().double(), fx.c0) and torch.equal(fx.hyps.double().float(), fx.hyps)
    if kind == "weights":
        assert torch.equal(fx.c0.to(BF16).double(), fx.c0)
    # 3. the splits: both bf16 terms / both f16 halves of every non-zero weight are live and exact
    wt = fx.wt.reshape(-1)
    wt = wt[wt != 0]
    w32 = wt.float()
    assert torch.equal(w32.double(), wt) and len(wt) >= 27 * base // 4
    ahi, alo = f16_split(fx.c0.numpy())
    assert np.array_equal(ahi + alo, fx.c0.numpy())
    if kind == "weights":
        hi = w32.to(BF16).float()
        lo = (w32 - hi).to(BF16).float()
        assert bool((lo != 0).all()) and torch.equal(hi + lo, w32)
        # damvs_stage_create's prob_split: w 2^k with the largest |w| 2^k in (2^13, 2^14], as f16 hi + lo
        k = 14 - int(np.frexp(float(w32.abs().max()))[1])
        shi, slo = f16_split(np.ldexp(w32.numpy(), k))
        assert (slo != 0).all() and np.array_equal((shi + slo) * 2.0 ** -k, wt.numpy())
        assert (np.abs(slo) >= 2.0 ** -14).all() and (alo == 0).all()   # lo x lo, which the fp32 MFMA form drops, is 0
    else:
        k = 14 - int(np.frexp(float(w32.abs().max()))[1])
        shi, slo = f16_split(np.ldexp(w32.numpy(), k))
        assert (slo == 0).all() and np.array_equal(shi * 2.0 ** -k, wt.numpy())
        big = np.abs(fx.c0.numpy()) > 2
        assert (alo[big] != 0).all() and (np.abs(alo[big]) >= 2.0 ** -14).all()     # a normal f16
        assert big.sum() >= 0.4 * (fx.c0.numpy() != 0).sum() and (alo[~big] == 0).all()   # 1 + 2^-10 is an f16 value
    # 4. the logits spread over several planes
    spread = float(fx.logits.std(1, unbiased=False).mean())
    assert 1.0 <= spread <= 4.0, spread
    # 5. both ends of the confidence window and the one-hot pixels are reached (with prob_init)
    R = tail_reference(kind, base, D, h, w, True)
    first, last, on_last = edge_shares(R, fx.hot)
    assert first >= 0.03 and last >= 0.03 and on_last >= 1, (first, last, on_last)
    for b, y, x, plane in fx.hot:
        assert R.prob[b, plane, y, x] == 1.0 and R.prob[b, :, y, x].sum() == 1.0
    # 6. at most 1 % of the pixels may take either window
    for with_init in (False, True):
        amb = float(tail_reference(kind, base, D, h, w, with_init).amb.mean())
        assert amb <= 0.01, (with_init, amb)


@pytest.mark.parametrize("shape", REGRESS_ONLY, ids=["D%d-%dx%d" % s for s in REGRESS_ONLY])
def test_logits_fixture_conditions(shape):
    fx = logits_fixture(*shape)
    lg = fx.logits.numpy()
    assert np.array_equal(lg.astype(np.float32).astype(np.float64), lg) and np.array_equal(np.round(lg * 4), lg * 4)
    R = regress_reference(lg, fx.hyps.numpy())
    first, last, _ = edge_shares(R, [])
    assert first >= 0.03 and last >= 0.03 and float(R.amb.mean()) <= 0.01, (first, last, float(R.amb.mean()))


def test_model_delta_is_below_the_crude_one():
    """delta, the model's bound on idx, lies below the crude D^2 2^-21 at D = 144: 3.9 times at the largest idx
    (c_exp of 2 ulp included), and the ambiguous share stays below 0.5 % where the crude one gave 2.7 %."""
    R = tail_reference("weights", 8, 144, 8, 40, True)
    assert float(R.delta.max()) * 3.5 <= 144 ** 2 * 2.0 ** -21 and float(R.amb.mean()) <= 0.005


def test_route_table():
    """The docstring's route table, from regress_tail's rule as it stands: every GPU case lands where it says."""
    for row in ROWS:
        assert route(row.bf16, row.base, row.fused, row.switch) == row.kernel, row.id
        assert route(row.bf16, row.base, row.two, row.switch) == "two-pass", row.id
        assert row.two == row.fused + 8    # stage shapes are multiples of 8: no fused D lies between
        for D, _, _ in row_shapes(row)[:3]:
            assert route(row.bf16, row.base, D, row.switch) == row.kernel
    # bf16 base 8 at D = 144 is fused only on the MFMA form, whose column leaves the last plane's 1 KB out of LDS
    assert route(True, 8, 144, "0") == "two-pass" and route(True, 8, 152) == "two-pass"
    assert prob_mfma_smem(True, 144) == 158336 and prob_regress_smem(16, 112) == 157184   # ~155 KB of LDS


@pytest.mark.parametrize("fixt", FIXTURES, ids=["%s-b%d-D%d-%dx%d" % f for f in FIXTURES])
def test_float32_regression_within_bound(fixt):
    """The gate is not too tight: a float32 restatement with sequential sums stays inside it on every element."""
    fx = tail_fixture(*fixt)
    for with_init in (False, True):
        R = tail_reference(*fixt, with_init)
        ratios = tail_ratios(regress_f32(exact_logits(fx, with_init), fx.hyps.numpy()), R)
        worst = {k: float(v.max()) for k, v in ratios.items()}
        print("float32 restatement %s init=%d: %s" % (fixt, with_init, worst))
        assert max(worst.values()) <= 1.0, (fixt, with_init, worst)
    for shape in REGRESS_ONLY:
        lf = logits_fixture(*shape)
        R = regress_reference(lf.logits.numpy(), lf.hyps.numpy())
        assert not failing_pixels(regress_f32(lf.logits.numpy(), lf.hyps.numpy()), R).any()


DEFECT_FIXTURES = [("weights", 8, 16, 16, 40), ("weights", 8, 144, 8, 40), ("weights", 16, 48, 24, 72),
                   ("acts", 8, 8, 8, 8), ("acts", 16, 120, 8, 40)]


@pytest.mark.parametrize("fixt", DEFECT_FIXTURES, ids=["%s-b%d-D%d-%dx%d" % f for f in DEFECT_FIXTURES])
def test_simulated_defects_are_caught(fixt):
    """The gate is not too loose: each defect, applied to the reference computation (with prob_init), puts the stated
    share of the pixels beyond a bound."""
    kind, base, D, h, w = fixt
    fx = tail_fixture(*fixt)
    R = tail_reference(*fixt, True)
    hy = fx.hyps.numpy()
    assert not failing_pixels(as_got(R), R).any()

    def bad(conv_defect=None, reg_defect=None):
        return failing_pixels(as_got(regress_reference(exact_logits(fx, True, conv_defect), hy, reg_defect)), R)

    assert bad("zero_tap").sum() >= 1
    if kind == "weights":
        assert bad("drop_lo").mean() >= 0.25, bad("drop_lo").mean()
    assert bad(None, "window_short").mean() >= 0.25
    assert bad(None, "round_idx").mean() >= 0.25
    assert bad("init_shift").mean() >= 0.25
    edge = (R.ii == 0) | (R.ii >= D - 2)
    assert bad(None, "window_clamp")[edge].mean() > 0.5, bad(None, "window_clamp")[edge].mean()
    assert not bad(None, "window_clamp")[(R.ii >= 1) & (R.ii < D - 2) & ~R.amb].any()
    skip = bad(None, "max_skip_last")
    last = [(b, y, x) for b, y, x, plane in fx.hot if plane == D - 1]
    assert last and all(skip[i] for i in last)
    assert bad(None, "batch_hyps")[1].mean() >= 0.25


def test_zeroed_tap_against_the_old_gate():
    """Why the file exists, as far as it holds. On test_prob_mfma_vs_oracle's own data (its D = 64 case: rand * 2
    activations, the shared synthetic prob weights) a prob conv that drops one non-zero tap (the smallest of these
    weights, 2.8e-4) stays inside that test's prob (1e-4 abs), variance (1e-4) and confidence (1e-4) tolerances; only
    its depth tolerance sees it, by a factor below 2 (measured 1.3e-5 against 1e-5; the issue expected the defect to
    pass the old gate outright, which it does not). Against the per-pixel bounds the same defect is beyond the bound
    on more than half of the pixels, by a factor of 50 and more."""
    D, h, w = 64, 16, 40
    wt = model_state("depthnet_cfgA_adaptive")["cost_regularization.1.prob.weight"].float()
    g = torch.Generator().manual_seed(D + w)
    c0 = (torch.rand(B, D, h, w, 8, generator=g) * 2).to(BF16)
    hyps = torch.sort(torch.rand(B, D, h, w, generator=g) * 300 + 450, dim=1).values
    flat = wt.reshape(-1).abs()
    tap = int(torch.where(flat > 0, flat, torch.full_like(flat, np.inf)).argmin())
    wbad = wt.clone()
    wbad.view(-1)[tap] = 0.0
    assert float(flat[tap]) > 0
    vol = c0.float().permute(0, 4, 1, 2, 3)
    ref = O.regression(F.conv3d(vol, wt, padding=1)[:, 0], hyps)
    bad = O.regression(F.conv3d(vol, wbad, padding=1)[:, 0], hyps)
    n = lambda t: t.numpy().astype(np.float64)  # noqa: E731
    # the old gate, as test_prob_mfma_vs_oracle states it
    from test_gpu_parity import conf_mask_pair
    assert np.abs(n(bad["prob_volume"]) - n(ref["prob_volume"])).max() < 1e-4
    assert rel_max(n(bad["variance"]), n(ref["variance"])) < 1e-4
    m = conf_mask_pair(n(bad["prob_volume"]), n(ref["prob_volume"]))
    assert np.abs(n(bad["photometric_confidence"]) - n(ref["photometric_confidence"]))[m].max() < 1e-4
    assert 1e-5 <= pixel_rel(n(bad["depth"]), n(ref["depth"])).max() < 2e-5
    # the same defect against the per-pixel bounds (float64 on the same operands)
    R = regress_reference(prob_conv(c0.double(), wt.double()).numpy(), hyps.numpy())
    Rb = regress_reference(prob_conv(c0.double(), wbad.double()).numpy(), hyps.numpy())
    worst = max(float(v.max()) for v in tail_ratios(as_got(Rb), R).values())
    share = float(failing_pixels(as_got(Rb), R).mean())
    print("zeroed tap: %.1f %% of the pixels beyond a bound, largest ratio %.0f" % (100 * share, worst))
    assert share >= 0.5 and worst >= 50


# ---------------------------------------------------------------------------------------------- hypotheses: reference

def _src_index(scale, n_out, n_in, clamp=True):
    """k_geometry.hip src_index (aten's area_pixel_compute_source_index); exact for the power-of-two scales here."""
    s = np.maximum(scale * (np.arange(n_out) + 0.5) - 0.5, 0.0)
    i0 = np.floor(s).astype(np.int64)
    i1 = i0 + ((i0 < n_in - 1) if clamp else 1)
    l1 = s - i0
    return i0, i1, 1.0 - l1, l1


def hyp_reference(pd, pv, D, H, W, scale, defect=None):
    """float64 restatement of oracle.stage_hypotheses for stages 2 / 3 on float32 maps pd, pv [B][hp][wp], with the
    first-order float32 bound of hyp_refine_kernel per element. defect: None, "no_offset", "low_var" (low = -var
    always) or "unclamped" (i1 = i0 + 1 at the last row and column: reads the next row / the next map).
    Returns (ref, bound [B][D][H/scale][W/scale], cur, var [B][H][W])."""
    pd, pv = np.asarray(pd, np.float64), np.asarray(pv, np.float64)
    Bn, hp, wp = pd.shape
    y0, y1, ly0, ly1 = _src_index(hp / H, H, hp, defect != "unclamped")
    x0, x1, lx0, lx1 = _src_index(wp / W, W, wp, defect != "unclamped")
    base = (np.arange(Bn) * hp * wp).reshape(Bn, 1, 1)

    def bilerp(m):
        flat = np.concatenate([m.reshape(-1), np.zeros(wp + 2)])
        tap = lambda y, x: flat[base + y.reshape(1, H, 1) * wp + x.reshape(1, 1, W)]  # noqa: E731
        wy0, wy1, wx0, wx1 = ly0.reshape(1, H, 1), ly1.reshape(1, H, 1), lx0.reshape(1, 1, W), lx1.reshape(1, 1, W)
        terms = [wy0 * wx0 * tap(y0, x0), wy0 * wx1 * tap(y0, x1), wy1 * wx0 * tap(y1, x0), wy1 * wx1 * tap(y1, x1)]
        return sum(terms), 4 * U * sum(np.abs(t) for t in terms)

    cur, dcur = bilerp(pd)
    var, dvar = bilerp(pv)
    eps = O.EPS
    sure = np.abs(cur - var) > dcur + dvar          # which of the two the min picks is certain
    low = -np.minimum(cur, var)
    dlow = np.where(sure, np.where(cur < var, dcur, dvar), np.maximum(dcur, dvar))
    if defect == "low_var":
        low = -var
    rden = D - 1.0
    step = (var - low) / rden
    dstep = (dvar + dlow + U * np.abs(var - low)) / rden + U * np.abs(step)
    k3 = 3.0 / (var + eps)
    rk3 = dvar / (var + eps) + 2 * U
    i = np.arange(D, dtype=np.float64).reshape(1, D, 1, 1)
    e4 = lambda a: a[:, None]  # noqa: E731
    lin = e4(low) + e4(step) * i
    dlin = e4(dlow) + i * e4(dstep) + U * np.abs(e4(step) * i) + U * np.abs(lin)
    x = lin * e4(k3)
    dx = np.abs(x) * (e4(rk3) + U) + e4(k3) * dlin
    mx = np.maximum(x[:, :1], x[:, -1:])
    dmx = np.maximum(dx[:, :1], dx[:, -1:])
    y = x - mx
    dy = dx + dmx + U * np.abs(y)
    e = np.exp(y)
    re = dy + (2 * np.abs(y) + 2) * U
    s = e.sum(1, keepdims=True)
    rs = re.max(1, keepdims=True) + (D + 1) * U
    off = e / s
    roff = re + rs + 3 * U
    t1 = e4(cur + low)
    t2 = t1 + e4(step) * i
    t3 = t2 + eps
    corr = off * e4(step)
    v = t3 + (0.0 if defect == "no_offset" else corr)
    dv = (e4(dcur + dlow) + i * e4(dstep) + U * np.abs(e4(step) * i) + U * (np.abs(t1) + np.abs(t2) + np.abs(t3))
          + off * e4(dstep) + np.abs(corr) * (roff + U) + U * np.abs(v))
    if scale == 2:
        pool = lambda a: a.reshape(Bn, D, H // 2, 2, W // 2, 2).mean((3, 5))  # noqa: E731
        v, dv = pool(v), pool(dv)
        dv = dv + 2 * U * np.abs(v)
    return v, dv, cur, var


# (scale, D, stage resolution h x w): H x W = scale (h x w); the previous map is H / 4 x W / 4 in the stage-2 form
# (scale 2) and H / 2 x W / 2 in the stage-3 form (scale 1)
HYP_CASES = [(scale, D, hw) for scale in (2, 1) for D in (8, 32) for hw in ((8, 24), (24, 40))]


def hyp_case_id(c):
    return "scale%d-D%d-%dx%d" % (c[0], c[1], c[2][0], c[2][1])


@functools.lru_cache(maxsize=None)
def hyp_fixture(scale, D, hw):
    """Previous depth in [600, 700] and previous variance in four regimes by column band of the previous map:
    0, 1e-6, 1.2 .. 2.2 x depth, [1, 41]; distinct per batch element."""
    h, w = hw
    H, W = h * scale, w * scale
    hp, wp = (H // 4, W // 4) if scale == 2 else (H // 2, W // 2)
    g = torch.Generator().manual_seed(900 + 10 * D + h + scale)
    pd = (600 + 100 * torch.rand(B, hp, wp, generator=g)).float()
    pv = (1 + 40 * torch.rand(B, hp, wp, generator=g)).float()
    big = (pd * (1.2 + torch.rand(B, hp, wp, generator=g))).float()
    col = torch.arange(wp).view(1, 1, wp).expand(B, hp, wp) / float(wp)
    pv = torch.where(col < 1 / 6, torch.zeros_like(pv), pv)
    pv = torch.where((col >= 1 / 6) & (col < 1 / 3), torch.full_like(pv, 1e-6), pv)
    pv = torch.where((col >= 1 / 3) & (col < 5 / 6), big, pv)
    dv = torch.tensor([[425.0, 935.0], [500.5, 1011.25]])
    return types.SimpleNamespace(scale=scale, D=D, h=h, w=w, H=H, W=W, pd=pd, pv=pv, dv=dv)


def hyp_regimes(fx, cur, var):
    """bool [B][h][w] per regime: every full-resolution point of the output pixel lies in it."""
    s = fx.scale
    every = lambda m: m.reshape(B, fx.h, s, fx.w, s).all((2, 4))  # noqa: E731
    return {"var<depth": every((var >= 1.0) & (var < cur)), "var>depth": every(var > cur), "var=0": every(var == 0.0),
            "var=1e-6": every(np.abs(var - 1e-6) < 1e-12)}


REGIME_SHARE = {"var<depth": 0.05, "var>depth": 0.25, "var=0": 0.05, "var=1e-6": 0.05}


def hyp_oracle(fx, dtype):
    return O.stage_hypotheses(1, fx.dv.to(dtype), fx.pd.to(dtype), fx.pv.to(dtype), fx.D, fx.H, fx.W, fx.scale)


def linear_reference(dv, D):
    """float64 stage-1 samples dmin + d itv and the ulp-level bound of hyp_linear_kernel, [B][D]."""
    dv = np.asarray(dv, np.float64)
    itv = (dv[:, -1:] - dv[:, :1]) / (D - 1)
    d = np.arange(D, dtype=np.float64).reshape(1, D)
    ref = dv[:, :1] + d * itv
    return ref, 3 * U * d * np.abs(itv) + U * np.abs(ref)


# ---------------------------------------------------------------------------------------------- CPU tests: hypotheses

@pytest.mark.parametrize("case", HYP_CASES, ids=[hyp_case_id(c) for c in HYP_CASES])
def test_hyp_reference_and_regimes(case):
    """The numpy restatement is the oracle (float64 against float64), the regimes cover their shares, and the
    oracle's float32 evaluation stays inside the bound on every element (the gate is not too tight)."""
    fx = hyp_fixture(*case)
    ref, bound, cur, var = hyp_reference(fx.pd.numpy(), fx.pv.numpy(), fx.D, fx.H, fx.W, fx.scale)
    want = hyp_oracle(fx, torch.float64).numpy()
    assert ref.shape == want.shape == (B, fx.D, fx.h, fx.w)
    assert np.abs(ref - want).max() <= 1e-12 * np.abs(want).max()
    assert fx.h * fx.w % 256 != 0 and not torch.equal(fx.pd[0], fx.pd[1])
    for name, m in hyp_regimes(fx, cur, var).items():
        assert m.mean() >= REGIME_SHARE[name], (name, float(m.mean()))
    r = _ratio(hyp_oracle(fx, torch.float32).numpy(), want, bound)
    print("float32 oracle %s: max |got - ref| / bound %.3f" % (hyp_case_id(case), r.max()))
    assert r.max() <= 1.0


@pytest.mark.parametrize("case", HYP_CASES, ids=[hyp_case_id(c) for c in HYP_CASES])
def test_hyp_simulated_defects_are_caught(case):
    """The gate is not too loose. The offset term missing: every pixel with var >= 1 throughout; low = -var always:
    every pixel of the var > depth regime; i1 unclamped: the last row and the last column."""
    fx = hyp_fixture(*case)
    ref, bound, cur, var = hyp_reference(fx.pd.numpy(), fx.pv.numpy(), fx.D, fx.H, fx.W, fx.scale)
    reg = hyp_regimes(fx, cur, var)
    args = (fx.pd.numpy(), fx.pv.numpy(), fx.D, fx.H, fx.W, fx.scale)
    bad = lambda d: (~(_ratio(hyp_reference(*args, d)[0], ref, bound) <= 1.0)).any(1)  # noqa: E731
    off = bad("no_offset")
    assert off.mean() >= 0.25 and off[reg["var<depth"] | reg["var>depth"]].all()
    low = bad("low_var")
    assert low.mean() >= 0.25 and low[reg["var>depth"]].all() and not low[reg["var<depth"]].any()
    edge = bad("unclamped")
    assert edge[:, -1, :].mean() >= 0.9 and edge[:, :, -1].mean() >= 0.9 and not edge[:, :-1, :-1].any()


def test_linear_reference_is_the_oracle():
    dv = torch.tensor([[425.0, 600.0, 935.0], [500.5, 700.0, 1011.25]])
    for D in (8, 48):
        ref, bound = linear_reference(dv.numpy(), D)
        want = O.stage_hypotheses(0, dv.double(), None, None, D, 32, 48, 4).numpy()
        assert want.shape == (B, D, 8, 12) and np.abs(want - ref[:, :, None, None]).max() <= 1e-12 * 1011.25
        f32 = O.stage_hypotheses(0, dv, None, None, D, 32, 48, 4).numpy()
        assert (_ratio(f32, ref[:, :, None, None], bound[:, :, None, None]) <= 1.0).all()


# ---------------------------------------------------------------------------------------------- GPU tests

@functools.lru_cache(maxsize=None)
def engine(kind, base, bf16):
    """The stage of CostRegNet(8, base) with the fixture's prob.weight, or None where damvs_stage_create refuses the
    base with DAMVS_E_SHAPE (any other failure is an error)."""
    from damvsnet_amd import _capi
    from damvsnet_amd.engine import StageEngine
    from damvsnet_amd.layers import CostRegNet
    torch.manual_seed(base)
    net = CostRegNet(8, base)
    with torch.no_grad():
        net.prob.weight.copy_(prob_weight(kind, base))
    try:
        return StageEngine(net.eval(), None, "variance", BF16 if bf16 else F32, torch.device(DEV))
    except _capi.DamvsError as e:
        assert base == 16 and e.rc == E_SHAPE, e
        print("base %d refused by damvs_stage_create: %s" % (base, e))
        return None


def set_switch(monkeypatch, row, vec=None):
    for name, value in (("DAMVS_PROB_MFMA", row.switch), ("DAMVS_PROB_VEC", vec)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)


def run_tail(eng, fx, with_init, bf16, want_prob=True):
    c0 = fx.c0.to(BF16 if bf16 else F32).to(DEV).contiguous()
    init = fx.init.float().to(DEV).contiguous() if with_init else None
    depth, conf, var, prob = eng.regress_c0(c0, fx.hyps.to(DEV).contiguous(), prob_init=init, want_prob=want_prob)
    torch.cuda.synchronize()
    return {"depth": depth, "conf": conf, "var": var, "prob": prob}


def to_numpy(out):
    return {k: None if v is None else v.cpu().numpy().astype(np.float64) for k, v in out.items()}


def assert_tail(got, R, what, fam):
    """Every pixel within its bounds; prints the largest ratio per output (the docstring's per-route figures)."""
    ratios = tail_ratios(got, R)
    worst = {k: float(v.max()) for k, v in ratios.items()}
    print("tail bound [%s] %s: %s" % (fam, what, " ".join("%s %.4f" % (k, worst[k]) for k in sorted(worst))))
    if not max(worst.values()) <= 1.0:
        lines = []
        for k, v in ratios.items():
            idx = np.argwhere(~(v <= 1.0))
            if len(idx):
                lines.append("%s %s: %d of %d pixels beyond the bound (largest ratio %.3f)"
                             % (what, k, len(idx), v.size, worst[k]))
                for i in idx[:6]:
                    i = tuple(i)
                    lines.append("  (b, y, x) = %s: ratio %.3f, idx %.6f, i* %d, got %s" % (
                        i, v[i], R.idx[i], R.ii[i], "-" if k == "prob" else repr(float(got[k][i]))))
        pytest.fail("\n".join(lines))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_tail_within_bound(case, _lib, monkeypatch):
    """Every row of the route table at every shape, with and without prob_init, against the float64 reference."""
    row, kind, shape, with_init = case
    set_switch(monkeypatch, row)
    eng = engine(kind, row.base, row.bf16)
    if eng is None:
        return   # base 16 refused with DAMVS_E_SHAPE: the acceptable other outcome (asserted in engine())
    fx = tail_fixture(kind, row.base, *shape)
    fam = row.kernel if shape[0] <= row.fused else "two-pass %s base %d" % ("bf16" if row.bf16 else "fp32", row.base)
    assert_tail(to_numpy(run_tail(eng, fx, with_init, row.bf16)), tail_reference(kind, row.base, *shape, with_init),
                case_id(case), fam)


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_tail_without_prob_and_without_vector_stores(row, _lib, monkeypatch):
    """want_prob=False gives depth, confidence and variance bitwise equal to the want_prob=True run; for the two
    prob_mfma rows DAMVS_PROB_VEC=0 (4-byte probability stores) gives every output bitwise equal to the default."""
    eng = engine("weights", row.base, row.bf16)
    if eng is None:
        return
    fx = tail_fixture("weights", row.base, *BITWISE_SHAPE)
    set_switch(monkeypatch, row)
    full = run_tail(eng, fx, True, row.bf16)
    bare = run_tail(eng, fx, True, row.bf16, want_prob=False)
    assert bare["prob"] is None
    for k in ("depth", "conf", "var"):
        assert torch.equal(full[k], bare[k]), k
    if row.kernel.startswith("prob_mfma"):
        set_switch(monkeypatch, row, vec="0")
        scalar = run_tail(eng, fx, True, row.bf16)
        for k in ("depth", "conf", "var", "prob"):
            assert torch.equal(full[k], scalar[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_two_pass_needs_the_logits_scratch(row, _lib, monkeypatch):
    """At the first two-pass D, scratch = NULL is refused with DAMVS_E_WORKSPACE and nothing is launched."""
    from damvsnet_amd import _capi
    from damvsnet_amd._capi import ptr
    eng = engine("weights", row.base, row.bf16)
    if eng is None:
        return
    set_switch(monkeypatch, row)
    fx = tail_fixture("weights", row.base, row.two, 8, 40)
    c0 = fx.c0.to(BF16 if row.bf16 else F32).to(DEV).contiguous()
    hyps = fx.hyps.to(DEV).contiguous()
    out = [torch.full((B, 8, 40), -1.0, device=DEV) for _ in range(3)]
    rc = eng._lib.damvs_stage_regress(eng.handle, _capi.stream_ptr(eng.device), B, row.two, 8, 40, ptr(c0), ptr(hyps),
                                      None, None, ptr(out[0]), ptr(out[1]), ptr(out[2]), None)
    torch.cuda.synchronize()
    assert rc == E_WORKSPACE, rc
    assert all(bool((o == -1.0).all()) for o in out)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", REGRESS_ONLY, ids=["D%d-%dx%d" % s for s in REGRESS_ONLY])
def test_regress_alone_within_bound(shape, _lib):
    """damvs_regress (regress_kernel) on exact lattice logits at shapes no stage allows."""
    from damvsnet_amd.engine import regress
    fx = logits_fixture(*shape)
    depth, conf, var, prob = regress(fx.logits.float().to(DEV), fx.hyps.to(DEV))
    got = to_numpy({"depth": depth, "conf": conf, "var": var, "prob": prob})
    R = regress_reference(fx.logits.numpy(), fx.hyps.numpy())
    assert_tail(got, R, "regress-D%d-%dx%d" % shape, "regress_kernel")
    d2, c2, v2, p2 = regress(fx.logits.float().to(DEV), fx.hyps.to(DEV), want_prob=False)
    assert p2 is None and torch.equal(d2, depth) and torch.equal(c2, conf) and torch.equal(v2, var)


@pytest.mark.gpu
@pytest.mark.parametrize("case", HYP_CASES, ids=[hyp_case_id(c) for c in HYP_CASES])
def test_hyp_refine_within_bound(case, _lib):
    """hyp_refine_kernel per element against the float64 oracle, in every regime of the previous variance."""
    from damvsnet_amd.engine import hypotheses
    fx = hyp_fixture(*case)
    ref, bound, cur, var = hyp_reference(fx.pd.numpy(), fx.pv.numpy(), fx.D, fx.H, fx.W, fx.scale)
    got = hypotheses(fx.dv.to(DEV), fx.D, fx.H, fx.W, fx.scale, fx.pd.to(DEV), fx.pv.to(DEV)).cpu().numpy()
    assert got.shape == ref.shape
    r = _ratio(got, ref, bound).max(1)
    reg = hyp_regimes(fx, cur, var)
    mixed = ~functools.reduce(np.logical_or, reg.values())
    worst = " ".join("%s %.4f" % (k, r[m].max()) for k, m in reg.items())
    print("hyp bound %s: %s mixed %.4f" % (hyp_case_id(case), worst, r[mixed].max()))
    if not r.max() <= 1.0:
        idx = np.argwhere(~(r <= 1.0))
        pytest.fail("%s: %d of %d pixels beyond the bound (largest ratio %.3f), first (b, y, x) %s"
                    % (hyp_case_id(case), len(idx), r.size, r.max(), [tuple(i) for i in idx[:6]]))


@pytest.mark.gpu
@pytest.mark.parametrize("D", [8, 48])
def test_hyp_linear_within_bound(D, _lib):
    """hyp_linear_kernel (stage 1) per element at its ulp bound."""
    from damvsnet_amd.engine import hypotheses
    dv = torch.tensor([[425.0, 600.0, 935.0], [500.5, 700.0, 1011.25]])
    ref, bound = linear_reference(dv.numpy(), D)
    got = hypotheses(dv.to(DEV), D, 32, 48, 4).cpu().numpy()
    assert got.shape == (B, D, 8, 12)
    r = _ratio(got, ref[:, :, None, None], bound[:, :, None, None])
    print("hyp_linear D=%d: max |got - ref| / bound %.4f" % (D, r.max()))
    assert r.max() <= 1.0
