"""CPU: the code object of the scene inputs kernel (damvsnet_amd/libdamvs_inputs.so, built from k_inputs.hip).

The rules tests/test_scene_codeobj.py applies to libdamvs_scene.so, for the fifth library (build.py BUILD_SIDE_LIBS):
  * its kernel set and instruction stream equal the ones the GPU run ran: tests/isa_pins_inputs.json, whose
    `validated_by` is the committed log of tests/test_gpu_inputs.py on that build, the launch beside a bf16 forward on
    another stream included (renew with `python tools/isa.py --lib damvsnet_amd/libdamvs_inputs.so --pins
    tests/isa_pins_inputs.json --update-pins --validated-by <that log>`);
  * no packed-FP32 VALU ops of any kind (built without the SLP and loop vectorizers, as every kernel without MFMA
    instructions: it can share a CU with another stream's MFMA kernels);
  * no scratch, no spills, no LDS;
  * the kernel lives in that library only, and the tuples the older code-object tests assert keep their values.
"""
import json
import os
import re
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
PINS = os.path.join(REPO, "tests", "isa_pins_inputs.json")
KERNEL = "damvs::(anonymous namespace)::scene_inputs_kernel(damvs::InputsArgs)"

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no llvm-objdump")


@pytest.fixture(scope="module")
def inputs_lib():
    from damvsnet_amd import build
    build.build()
    assert os.path.exists(build.INPUTS_LIB)
    return build.INPUTS_LIB


def test_build_flags_and_library_tuples():
    from damvsnet_amd import build
    assert build.FILE_FLAGS.get("k_inputs.hip") == ["-fno-slp-vectorize", "-fno-vectorize"]
    assert os.path.basename(build.INPUTS_LIB) == "libdamvs_inputs.so" and build.INPUTS_UNITS == ("k_inputs.hip",)
    assert build.BUILD_SIDE_LIBS == build.ALL_SIDE_LIBS + ((build.INPUTS_LIB, build.INPUTS_UNITS),)
    # the older tuples keep their values (tests/test_cloud_codeobj.py, tests/test_scene_codeobj.py)
    assert build.SIDE_LIBS == ((build.SIDE_LIB, build.SIDE_UNITS), (build.CLOUD_LIB, build.CLOUD_UNITS))
    assert build.ALL_SIDE_LIBS == build.SIDE_LIBS + ((build.SCENE_LIB, build.SCENE_UNITS),)
    with open(os.path.join(REPO, ".gitignore")) as f:
        assert "*.so" in f.read().split()  # built libraries stay out of git


def test_inputs_kernel_instruction_stream_is_the_validated_one(inputs_lib):
    import isa
    with open(PINS) as f:
        pins = json.load(f)
    assert os.path.exists(os.path.join(REPO, pins["validated_by"])), pins["validated_by"]
    assert pins["validated_by"].startswith("profiles/r17/")
    assert list(pins["kernels"]) == [KERNEL]
    if pins["compiler"] != isa.compiler():
        pytest.skip("different compiler (%s): instruction streams are not comparable" % isa.compiler())
    got = isa.hashes(inputs_lib)
    assert got == pins["kernels"], (got, pins["kernels"])
    from damvsnet_amd import build
    for other in (build.LIB,) + tuple(lib for lib, _ in build.ALL_SIDE_LIBS):
        assert not [k for k in isa.hashes(other) if "inputs" in k], other


def test_inputs_kernel_carries_no_packed_fp32_ops(inputs_lib):
    import isa
    ks = isa.disassemble(inputs_lib)
    assert len(ks) == 1
    for name, body in ks.items():
        assert not any(t.startswith("v_mfma") for t in body)
        assert not [t for t in body if re.match(r"v_pk_\w+_f32\b", t)], name
        # one 16-byte store per colour plane; the taps are byte loads
        assert sum(t.startswith("global_store_dwordx4") for t in body) == 3
        assert sum(t.startswith("global_store") for t in body) == 3
        assert sum(t.startswith("global_load_ubyte") for t in body) == 48
        # the combine is not contracted: 6 products and 3 sums per value, 12 values, each an instruction of its own
        # (the quotients' expansions bring further v_mul_f32, the coordinates further v_add_f32, never fewer)
        assert sum(t.startswith("v_mul_f32") for t in body) >= 72 and sum(t.startswith("v_add_f32") for t in body) >= 36


def test_inputs_kernel_uses_no_scratch_spills_or_lds(inputs_lib):
    import codeobj_check as C
    ks = C.kernels(inputs_lib)
    assert len(ks) == 1
    for name, k in ks.items():
        assert not (k["priv"] or k["spill"] or k["sspill"] or k["lds"]), (name, k)
