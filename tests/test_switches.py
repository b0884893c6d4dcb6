"""CPU: the runtime kernel-selection switches (damvsnet_amd/csrc/switches.h) parse every value as the hand-written
getenv sites they replaced did, the table names exactly the switches the GPU tests use as references, ONCE switches are
memoised and LIVE ones are not, and nothing else in csrc/ reads the environment.

A stand-alone program (its own main, the header alone, no HIP) is compiled with the compiler the library is built with
and run once per environment; it prints, per table row, the accessor's answer, then sets the variable to another value
and prints the answer again."""
import glob
import os
import subprocess

import pytest

from damvsnet_amd import build

CSRC = build.CSRC

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "switches.h"
using namespace damvs;
static void show(const SwitchRow& r) {
  if (r.kind == VALUE) {
    const char* v = switch_value(r.id);
    if (v) std::printf(" [%s]", v);
    else std::printf(" -");
  } else {
    std::printf(" %d", switch_on(r.id) ? 1 : 0);
  }
}
int main() {
  for (int i = 0; i < SW_COUNT; ++i) {
    const SwitchRow& r = kSwitches[i];
    if (r.id != i) return 2;
    std::printf("%s %s %s", r.env, r.kind == DEFAULT_ON ? "DEFAULT_ON" : r.kind == DEFAULT_OFF ? "DEFAULT_OFF" : "VALUE",
                r.read == ONCE ? "ONCE" : "LIVE");
    show(r);
    const char* v = std::getenv(r.env);
    setenv(r.env, v && v[0] == '0' ? "1" : "0", 1);  // a value of the other first character
    show(r);
    std::printf("\n");
  }
  return 0;
}
"""

# The parse of each switch at the parent commit, written out from its getenv site:
#   off0: `v && v[0] == '0'` turned the default path off (default on)
#   on1:  `v && v[0] == '1'` turned the alternative on (default off)
#   raw:  the caller parses the string itself (DAMVS_CONV0_DZ, DAMVS_CONV0_REUSE: conv3d_route; DAMVS_PROB_MFMA: tail_route)
# and whether the site kept its first answer (a function-local static) or read the environment at every call.
PARENT = {
    "DAMVS_PLANES4": ("off0", "LIVE"),
    "DAMVS_PLANES_MFMA": ("off0", "LIVE"),
    "DAMVS_WARP_SPLIT": ("off0", "ONCE"),
    "DAMVS_WARP_RUNTIME_VIEWS": ("on1", "ONCE"),
    "DAMVS_HALO_RS": ("off0", "LIVE"),
    "DAMVS_WIDE_RS": ("off0", "LIVE"),
    "DAMVS_WIDE_S2R1": ("off0", "LIVE"),
    "DAMVS_CONV2D_XPAIR_LDS": ("off0", "LIVE"),
    "DAMVS_CONV2D_LDS_PLANE": ("off0", "LIVE"),
    "DAMVS_CONV2D_G32": ("off0", "LIVE"),
    "DAMVS_CONV0_DZ": ("raw", "LIVE"),
    "DAMVS_CONV0_REUSE": ("raw", "LIVE"),
    "DAMVS_CONV_NO_ZSLIDE": ("on1", "LIVE"),
    "DAMVS_DECONV_NO_ZSLIDE": ("on1", "LIVE"),
    "DAMVS_CONV3D_K16": ("on1", "LIVE"),
    "DAMVS_PROB_VEC": ("off0", "LIVE"),
    "DAMVS_PROB_MFMA": ("raw", "LIVE"),
}
KIND = {"off0": "DEFAULT_ON", "on1": "DEFAULT_OFF", "raw": "VALUE"}
VALUES = [None, "", "0", "1", "2"]


def _expected(parse, v):
    """What the accessor prints for environment value v (None: unset)."""
    if parse == "off0":  # switch_on() == the default path is on == !(v && v[0] == '0')
        return "0" if v is not None and v[:1] == "0" else "1"
    if parse == "on1":  # switch_on() == v && v[0] == '1'
        return "1" if v is not None and v[:1] == "1" else "0"
    return "-" if v is None else "[%s]" % v


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("switches")
    src, exe = str(d / "switches_main.cpp"), str(d / "switches_main")
    with open(src, "w") as f:
        f.write(PROGRAM)
    r = subprocess.run([build.HIPCC, "-x", "c++", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run(exe, value):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DAMVS_")}
    if value is not None:
        env.update({name: value for name in PARENT})
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    return [line.split(" ") for line in r.stdout.splitlines()]


def test_table_names_exactly_the_remaining_switches(program):
    rows = _run(program, None)
    assert sorted(r[0] for r in rows) == sorted(PARENT)
    assert len(rows) == 17
    for name, kind, read, _, _ in rows:
        assert (kind, read) == (KIND[PARENT[name][0]], PARENT[name][1]), name


@pytest.mark.parametrize("value", VALUES, ids=["unset", "empty", "0", "1", "2"])
def test_accessor_parses_as_the_parent_did(program, value):
    flipped = "1" if value is not None and value[:1] == "0" else "0"  # what the program sets before its second read
    for name, _, read, first, second in _run(program, value):
        parse = PARENT[name][0]
        assert first == _expected(parse, value), (name, value)
        # ONCE: the first answer stays; LIVE: the new value is seen
        assert second == (first if read == "ONCE" else _expected(parse, flipped)), (name, value, read)


def test_getenv_only_in_switches_h():
    files = [p for p in glob.glob(os.path.join(CSRC, "*")) if os.path.isfile(p)]
    assert os.path.join(CSRC, "switches.h") in files
    hits = []
    for p in files:
        with open(p, errors="replace") as f:
            if "getenv" in f.read() and os.path.basename(p) != "switches.h":
                hits.append(os.path.basename(p))
    assert not hits, "getenv outside switches.h: %s" % hits
