"""CPU: the code object of the scene ingest kernel (damvsnet_amd/libdamvs_scene.so, built from k_scene.hip).

The rules tests/test_cloud_codeobj.py applies to libdamvs_cloud.so, for the fourth library (build.py ALL_SIDE_LIBS):
  * its kernel set and instruction stream equal the ones the GPU run ran: tests/isa_pins_scene.json, whose
    `validated_by` is the committed log of tests/test_gpu_scene.py on that build, the ingest beside a bf16 forward on
    another stream included (renew with `python tools/isa.py --lib damvsnet_amd/libdamvs_scene.so --pins
    tests/isa_pins_scene.json --update-pins --validated-by <that log>`);
  * no packed-FP32 VALU ops of any kind (built without the SLP and loop vectorizers, as every kernel without MFMA
    instructions: it can share a CU with another stream's MFMA kernels);
  * no scratch, no spills, no LDS;
  * and the kernel lives in that library only: tests/isa_pins.json stays the inventory of libdamvs.so.
"""
import json
import os
import re
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
PINS = os.path.join(REPO, "tests", "isa_pins_scene.json")
KERNEL = "damvs::(anonymous namespace)::scene_ingest_kernel(damvs::SceneArgs)"

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no llvm-objdump")


@pytest.fixture(scope="module")
def scene_lib():
    from damvsnet_amd import build
    build.build()
    assert os.path.exists(build.SCENE_LIB)
    return build.SCENE_LIB


def test_build_flags_of_the_scene_unit():
    from damvsnet_amd import build
    assert build.FILE_FLAGS.get("k_scene.hip") == ["-fno-slp-vectorize", "-fno-vectorize"]
    assert os.path.basename(build.SCENE_LIB) == "libdamvs_scene.so" and build.SCENE_UNITS == ("k_scene.hip",)
    assert build.ALL_SIDE_LIBS == build.SIDE_LIBS + ((build.SCENE_LIB, build.SCENE_UNITS),)


def test_scene_kernel_instruction_stream_is_the_validated_one(scene_lib):
    import isa
    with open(PINS) as f:
        pins = json.load(f)
    assert os.path.exists(os.path.join(REPO, pins["validated_by"])), pins["validated_by"]
    assert pins["validated_by"].startswith("profiles/r16/")
    assert list(pins["kernels"]) == [KERNEL]
    if pins["compiler"] != isa.compiler():
        pytest.skip("different compiler (%s): instruction streams are not comparable" % isa.compiler())
    got = isa.hashes(scene_lib)
    assert got == pins["kernels"], (got, pins["kernels"])
    from damvsnet_amd import build
    for other in (build.LIB,) + tuple(lib for lib, _ in build.SIDE_LIBS):
        assert not [k for k in isa.hashes(other) if "scene_" in k], other


def test_scene_kernel_carries_no_packed_fp32_ops(scene_lib):
    import isa
    ks = isa.disassemble(scene_lib)
    assert len(ks) == 1
    for name, body in ks.items():
        assert not any(t.startswith("v_mfma") for t in body)
        assert not [t for t in body if re.match(r"v_pk_\w+_f32\b", t)], name
        # 16-byte accesses for the f32 maps
        assert sum(t.startswith("global_load_dwordx4") for t in body) == 5
        assert sum(t.startswith("global_store_dwordx4") for t in body) == 4


def test_scene_kernel_uses_no_scratch_spills_or_lds(scene_lib):
    import codeobj_check as C
    ks = C.kernels(scene_lib)
    assert len(ks) == 1
    for name, k in ks.items():
        assert not (k["priv"] or k["spill"] or k["sspill"] or k["lds"]), (name, k)
