"""Which kernel each 2D front-end test case runs.

HipConv2d.route (damvs_conv2d_route) names the kernel a layer launches at a size under the current switches, spelled as
the keys of tests/isa_pins.json without namespace and parameter list. tests/conv2d_routes.json records that name

  "cases":        for every row of test_gpu_frontend.CASES x {f32, bf16} at the default switches ("12-bf16"), and at
                  every setting of EXACT_SETTINGS that routes the row elsewhere ("12-f32-DAMVS_WIDE_RS=0"). These are
                  the runs of the exact tests: test_gpu_lattice.py runs every entry, test_gpu_split.py the fp32 ones.
  "switch_tests": for every row of the A/B case lists x both states of the list's switch ("RS_CASES-0-f32-on").

test_conv2d_routes.py checks the table against the library on the GPU and its coverage of the pinned kernels on the
CPU; tools/conv2d_routes.py rewrites it. This module holds what the three share (no test lives here).
"""
import contextlib
import json
import os
import re

import torch
import torch.nn as nn

import test_gpu_frontend as FE

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "conv2d_routes.json")
PINS = os.path.join(HERE, "isa_pins.json")
B = 2
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}

# the switches conv2d_route and k_planes.hip read (switches.h; all on by default, "0" turns one off)
SWITCHES = ("DAMVS_PLANES4", "DAMVS_PLANES_MFMA", "DAMVS_HALO_RS", "DAMVS_WIDE_RS", "DAMVS_WIDE_S2R1",
            "DAMVS_CONV2D_XPAIR_LDS", "DAMVS_CONV2D_LDS_PLANE", "DAMVS_CONV2D_G32")
# what the exact tests turn off: nothing, each switch alone, and both plane switches (the 5x5 one-column kernel hides
# behind the MFMA form and the 4-column form)
EXACT_SETTINGS = ((),) + tuple((s,) for s in SWITCHES) + (("DAMVS_PLANES_MFMA", "DAMVS_PLANES4"),)


def pinned_conv2d_names():
    """The conv2d_* kernels of the built library as isa_pins.json pins them, spelled as HipConv2d.route spells them."""
    with open(PINS) as f:
        keys = json.load(f)["kernels"]
    pre = "void damvs::(anonymous namespace)::"
    return sorted(k[len(pre):k.index(">(") + 1] for k in keys if k.startswith(pre + "conv2d_"))


def load():
    with open(TABLE) as f:
        return json.load(f)


@contextlib.contextmanager
def switched(env):
    """os.environ with the 2D switches unset but for env's ({name: value}); restored on exit (the library reads its
    switches at every call)."""
    saved = {s: os.environ.pop(s, None) for s in SWITCHES}
    os.environ.update(env)
    try:
        yield
    finally:
        for s in SWITCHES:
            os.environ.pop(s, None)
            if saved[s] is not None:
                os.environ[s] = saved[s]


def case_size(case):
    return case[12] if len(case) > 12 else (20, 24)


def case_layer(case, dtype):
    """The layer of a CASES-style row (zero weights: the route depends on shapes alone)."""
    from damvsnet_amd.frontend_hip import HipConv2d
    tr, k, s, p, op, c0, c1, geo, cout, relu = case[:10]
    cin = c0 + c1 + len(geo)
    conv = (nn.ConvTranspose2d(cin, cout, k, stride=s, padding=p, output_padding=op) if tr
            else nn.Conv2d(cin, cout, k, stride=s, padding=p))
    with torch.no_grad():
        conv.weight.zero_()
        conv.bias.zero_()
    tensor_at = [c for c in range(cin) if c not in geo]
    at = dict(c0=c0, c1=c1, c1_at=0)
    if c0 and c1:
        at = dict(c0=c0, c0_at=tensor_at[0], c1=c1, c1_at=tensor_at[c0])
    elif c0:
        at = dict(c0=c0, c0_at=tensor_at[0])
    return HipConv2d(conv, dtype, relu, geo_at=geo, **at)


def case_route(i, dt):
    """The kernel row i of CASES runs in dtype dt ("f32" / "bf16") under the current switches."""
    case = FE.CASES[i]
    return case_layer(case, DTYPES[dt]).route(B, *case_size(case))


def case_key(i, dt, off=()):
    return "%d-%s" % (i, dt) + "".join("-%s=0" % s for s in off)


def parse_case_key(key):
    """(row, dtype name, switches off) of a "cases" key."""
    parts = key.split("-")
    return int(parts[0]), parts[1], tuple(p[:-2] for p in parts[2:])


def exact_runs(dts=("f32", "bf16"), switched_only=False):
    """The (row, dtype name, switches off) of the table's "cases" entries, in row order."""
    runs = [parse_case_key(k) for k in load()["cases"]]
    runs = [r for r in runs if r[1] in dts and (r[2] or not switched_only)]
    return sorted(runs, key=lambda r: (r[0], r[1] != "f32", r[2]))


# The A/B case lists of test_gpu_frontend.py: list name -> (switch, what else the test sets, dtypes, row -> CASES-style row).
_T, _F = True, False
SWITCH_TESTS = {
    "PLANES4_CASES": ("DAMVS_PLANES4", {"DAMVS_PLANES_MFMA": "0"}, ("bf16",),
                      lambda r: (_F, r[0], 1, r[0] // 2, 0, 0, 0, tuple(range(r[1])), 8, r[2], r[3], 0, (21, 36))),
    "LDS_PLANE_CASES": ("DAMVS_CONV2D_LDS_PLANE", {}, ("bf16",),
                        lambda r: (_F, 3, 1, 1, 0, r[0], 0, r[1], r[2], r[3], r[4], r[5], r[6])),
    "XPAIR_LDS_CASES": ("DAMVS_CONV2D_XPAIR_LDS", {}, ("bf16", "f32"),
                        lambda r: (_T, r[0], 2, r[1], r[2], 16, 0, (), 8, r[3], r[4], r[5], r[6])),
    "PLANES_MFMA_CASES": ("DAMVS_PLANES_MFMA", {}, ("f32", "bf16"),
                          lambda r: (_F, r[0], 1, r[0] // 2, 0, 0, 0, tuple(range(r[1])), r[2], r[3], r[4], r[5], r[6])),
    "RS_CASES": ("DAMVS_WIDE_RS", {}, ("f32",), lambda r: r),
    "S2R1_CASES": ("DAMVS_WIDE_S2R1", {}, ("f32",), lambda r: r),
    "G32_CASES": ("DAMVS_CONV2D_G32", {}, ("f32",), lambda r: r),
    "HALO_RS_CASES": ("DAMVS_HALO_RS", {}, ("f32",), lambda r: r),
}


def switch_test_rows():
    """(key, CASES-style row, dtype name, environment) for every A/B row, dtype and switch state."""
    for name, (switch, base, dts, to_case) in SWITCH_TESTS.items():
        for i, row in enumerate(getattr(FE, name)):
            for dt in dts:
                for state, env in (("on", dict(base)), ("off", dict(base, **{switch: "0"}))):
                    yield "%s-%d-%s-%s" % (name, i, dt, state), to_case(row), dt, env


def current_routes():
    """The table as the loaded library answers now (needs a device: creating a layer uploads its weights)."""
    cases, tests = {}, {}
    for i, case in enumerate(FE.CASES):
        H, W = case_size(case)
        for dt, dtype in DTYPES.items():
            L = case_layer(case, dtype)
            seen = set()
            for off in EXACT_SETTINGS:
                with switched({s: "0" for s in off}):
                    name = L.route(B, H, W)
                if not off or name not in seen:   # a setting that reaches a kernel no earlier setting reached
                    cases[case_key(i, dt, off)] = name
                seen.add(name)
    for key, case, dt, env in switch_test_rows():
        with switched(env):
            tests[key] = case_layer(case, DTYPES[dt]).route(B, *case_size(case))
    return {"cases": cases, "switch_tests": tests}


def flips(L, Bn, H, W, monkeypatch, switch, on, off):
    """What an A/B test asserts before it compares two runs: layer L routes to two different kernels with `switch` at its
    default and at 0, and they are the pair the test is about (on / off: regular expressions for the whole name).
    Leaves the switch unset."""
    monkeypatch.delenv(switch, raising=False)
    a = L.route(Bn, H, W)
    monkeypatch.setenv(switch, "0")
    b = L.route(Bn, H, W)
    monkeypatch.delenv(switch)
    assert a != b, "%s=0 does not reroute this layer: %s both times" % (switch, a)
    assert re.fullmatch(on, a), (switch, "default", a, on)
    assert re.fullmatch(off, b), (switch, "0", b, off)
    return a, b
