"""The 2D front-end router, seen through HipConv2d.route (damvs_conv2d_route).

tests/conv2d_routes.json records which kernel every row of the per-layer tests runs (tests/route_cases.py). Here:
  * CPU: the table is complete for the case lists as they stand, every A/B row names two different kernels, and every
    conv2d_* kernel that tests/isa_pins.json pins is either run by an exact test (it is the value of a "cases" entry:
    test_gpu_lattice.py runs each of them against float64 with equality as the gate) or listed in UNREACHABLE with the
    router line that keeps every argument away from it;
  * GPU: the library answers what the table records, and a sweep over the router's inputs never meets an UNREACHABLE
    kernel nor a name the pins do not know. Neither launches anything.
"""
import itertools

import pytest
import torch

import route_cases as R
import test_gpu_frontend as FE

# Instantiations no argument reaches, each with the line of k_conv2d.hip that excludes it. They stay compiled (and
# pinned) until a pull request of its own deletes them; a router change that brings one to life fails the sweep below
# and then owes it a row in test_gpu_frontend.CASES.
_HALO = "halo_route: `constexpr int max_mt = 2; if (a.MTtot > max_mt || ...) return false;` leaves r.mt <= 2, r.wm = 1"
_G8 = "gather_mt: `if (bf16 && a.MTtot % 8 == 0 && tiles * (a.MTtot / 8) >= want) return 8;` is the only 8"
_W21 = "wide_route: `if (r.wm == 1 && f32 && a.in_stride == 2) return false;` (the 32-K gather kernel is faster)"
UNREACHABLE = dict(
    [("conv2d_halo_kernel<%s, %s, %s, false, false>" % (t, mw, two), _HALO)
     for t in ("float", "unsigned short") for mw in ("4, 1", "4, 2", "8, 1") for two in ("false", "true")] +
    [("conv2d_mfma_kernel<float, 8, %s, false, false>" % two, _G8) for two in ("false", "true")] +
    [("conv2d_wide_kernel<float, %s, 2, 1, false, false>" % two, _W21) for two in ("false", "true")])


def test_route_table_is_complete():
    """Every CASES row x dtype has its default entry, every switched entry parses to a known setting and differs from
    the row's default, and every A/B row x dtype has both states, naming two different kernels."""
    t = R.load()
    keys = set(t["cases"])
    for i in range(len(FE.CASES)):
        for dt in R.DTYPES:
            assert R.case_key(i, dt) in keys, (i, dt)
    for k in keys:
        i, dt, off = R.parse_case_key(k)
        assert i < len(FE.CASES) and dt in R.DTYPES and off in R.EXACT_SETTINGS and R.case_key(i, dt, off) == k, k
        assert not off or t["cases"][k] != t["cases"][R.case_key(i, dt)], k
    want = [key for key, _, _, _ in R.switch_test_rows()]
    assert sorted(want) == sorted(t["switch_tests"])
    for key in want:
        if key.endswith("-on"):
            assert t["switch_tests"][key] != t["switch_tests"][key[:-2] + "off"], key


def test_every_conv2d_kernel_has_an_exact_test_or_is_unreachable():
    pinned = set(R.pinned_conv2d_names())
    t = R.load()
    exact = set(t["cases"].values())
    assert exact | set(t["switch_tests"].values()) <= pinned, "the table names kernels that isa_pins.json does not pin"
    assert set(UNREACHABLE) <= pinned, sorted(set(UNREACHABLE) - pinned)
    assert not exact & set(UNREACHABLE), sorted(exact & set(UNREACHABLE))
    missing = sorted(pinned - exact - set(UNREACHABLE))
    assert not missing, "conv2d kernels that no exact test runs (add a row to test_gpu_frontend.CASES):\n  " + \
        "\n  ".join(missing)


@pytest.fixture(scope="module")
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from damvsnet_amd import build, _capi
    build.build()
    _capi.load_library()


@pytest.mark.gpu
def test_routes_match_the_table(_lib):
    """tools/conv2d_routes.py rewrites the table after a deliberate router change."""
    got, want = R.current_routes(), R.load()
    for part in want:
        diff = {k: (got[part].get(k), want[part].get(k)) for k in set(got[part]) | set(want[part])
                if got[part].get(k) != want[part].get(k)}
        assert not diff, (part, "key: (library, table)", diff)


# The router's inputs: every (transposed, k, s, p, op) of CASES; one tensor input, two, each with and without a plane.
SWEEP_COUT = (8, 16, 24, 32, 48, 64, 128, 256)
SWEEP_C0 = (8, 16, 32, 64, 128)
SWEEP_SIZES = ((8, 9), (20, 24), (37, 151), (64, 130), (120, 240), (200, 288), (241, 477))
SWEEP_FORMS = sorted({c[:5] for c in FE.CASES})


@pytest.mark.gpu
@pytest.mark.parametrize("plane", (False, True), ids=("", "plane"))
@pytest.mark.parametrize("two", (False, True), ids=("one", "two"))
@pytest.mark.parametrize("dt", list(R.DTYPES))
def test_no_argument_reaches_a_dead_form(dt, two, plane, _lib):
    """Create and query only. Every answer is a pinned kernel and none is UNREACHABLE, at every setting of the 2D
    switches the exact tests use; layers the library refuses (create or query) are not counted as answers."""
    from damvsnet_amd._capi import DamvsError
    pinned = set(R.pinned_conv2d_names())
    seen, refused = set(), 0
    for form, c0, cout in itertools.product(SWEEP_FORMS, SWEEP_C0, SWEEP_COUT):
        case = form + (c0, c0 if two else 0, (c0 * (2 if two else 1),) if plane else (), cout, True)
        try:
            L = R.case_layer(case, R.DTYPES[dt])
        except DamvsError:
            refused += 1
            continue
        for off in R.EXACT_SETTINGS:
            with R.switched({s: "0" for s in off}):
                for H, W in SWEEP_SIZES:
                    try:
                        seen.add(L.route(R.B, H, W))
                    except DamvsError:
                        refused += 1
    print("%s: %d kernels reported, %d refusals: %s" % (dt, len(seen), refused, sorted(seen)))
    assert seen <= pinned, sorted(seen - pinned)
    assert not seen & set(UNREACHABLE), sorted(seen & set(UNREACHABLE))
    assert len(seen) >= 8  # the sweep did reach the router


@pytest.mark.gpu
def test_route_errors(_lib):
    """A buffer too small for the answer and a null buffer are argument errors; a size no kernel takes (an operand of
    2 GiB) is a shape error, as the forward's."""
    import ctypes
    from damvsnet_amd import _capi
    lib = _capi.load_library()
    L = R.case_layer(FE.CASES[0], torch.float32)
    small = ctypes.create_string_buffer(8)
    assert lib.damvs_conv2d_route(L.handle, 2, 20, 24, small, len(small)) == -1
    assert b"too small" in lib.damvs_last_error_string()
    assert lib.damvs_conv2d_route(L.handle, 2, 20, 24, None, 64) == -1
    buf = ctypes.create_string_buffer(128)
    assert lib.damvs_conv2d_route(L.handle, 4096, 512, 512, buf, len(buf)) == -2 and buf.value == b""
    name, grid = L.route(2, 20, 24, grid=True)
    assert name == R.load()["cases"]["0-f32"] and grid == (6, 1)   # 20 x 24: 3 x 1 tiles of 8 x 64, B = 2
