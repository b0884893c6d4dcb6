"""CPU: the static-rule fusion kernel's code object (damvsnet_amd/libdamvs_fusion.so, built from k_fusion_static.hip).

tests/isa_pins.json, tests/test_isa_pins.py and tests/test_codeobj.py guard the kernels of libdamvs.so; the static-rule
kernel is linked into a library of its own beside it (build.py SIDE_UNITS), and this file applies the same three rules
to that library:
  * its instruction stream equals the one the GPU stream tests last ran beside (tests/isa_pins_fusion.json; renew with
    `python tools/isa.py --lib damvsnet_amd/libdamvs_fusion.so --pins tests/isa_pins_fusion.json --update-pins
    --validated-by <committed log of tests/test_gpu_streams.py on that build>`);
  * no packed-FP32 VALU ops (built without the SLP and loop vectorizers, as every kernel without MFMA instructions);
  * no scratch, no spills, no LDS.
libdamvs.so itself must hold no kernel that tests/isa_pins.json does not know: the two pin files together cover every
kernel the package launches.
"""
import json
import os
import re
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
PINS = os.path.join(REPO, "tests", "isa_pins_fusion.json")

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no llvm-objdump")


@pytest.fixture(scope="module")
def side_lib():
    from damvsnet_amd import build
    build.build()
    assert os.path.exists(build.SIDE_LIB)
    return build.SIDE_LIB


def test_static_kernel_instruction_stream_is_the_validated_one(side_lib):
    import isa
    with open(PINS) as f:
        pins = json.load(f)
    assert os.path.exists(os.path.join(REPO, pins["validated_by"])), pins["validated_by"]
    if pins["compiler"] != isa.compiler():
        pytest.skip("different compiler (%s): instruction streams are not comparable" % isa.compiler())
    got = isa.hashes(side_lib)
    assert got == pins["kernels"], (got, pins["kernels"])
    assert list(got) == ["damvs::(anonymous namespace)::fusion_view_static_kernel(damvs::FusionArgs, int)"]
    with open(isa.PINS) as f:  # and libdamvs.so holds nothing beyond its own pin file
        main = json.load(f)["kernels"]
    assert not [k for k in isa.hashes() if k not in main]


def test_static_kernel_carries_no_packed_fp32_ops(side_lib):
    import isa
    from damvsnet_amd import build
    assert build.FILE_FLAGS.get("k_fusion_static.hip") == ["-fno-slp-vectorize", "-fno-vectorize"]
    ks = isa.disassemble(side_lib)
    assert len(ks) == 1
    pk = re.compile(r"v_pk_(fma|mul|add|mov)_f32\b")
    for name, body in ks.items():
        assert not any(t.startswith("v_mfma") for t in body)
        assert not [t for t in body if pk.match(t)], name


def test_static_kernel_uses_no_scratch_spills_or_lds(side_lib):
    import codeobj_check as C
    ks = C.kernels(side_lib)
    assert len(ks) == 1
    for name, k in ks.items():
        assert not (k["priv"] or k["spill"] or k["sspill"] or k["lds"]), (name, k)
