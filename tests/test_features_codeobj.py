"""CPU: the code object of the scene features gather kernel (damvsnet_amd/libdamvs_features.so, built from
k_features.hip).

The rules tests/test_inputs_codeobj.py applies to libdamvs_inputs.so, for the sixth library (build.py LINKED_SIDE_LIBS):
  * its kernel set and instruction stream equal the ones the GPU run ran: tests/isa_pins_features.json, whose
    `validated_by` is the committed log of tests/test_gpu_features.py on that build, the launch beside a bf16 forward on
    another stream included (renew with `python tools/isa.py --lib damvsnet_amd/libdamvs_features.so --pins
    tests/isa_pins_features.json --update-pins --validated-by <that log>`);
  * no MFMA and no packed-FP32 VALU ops of any kind (built without the SLP and loop vectorizers, as every kernel without
    MFMA instructions: it can share a CU with another stream's MFMA kernels);
  * no scratch, no spills, no LDS;
  * every global load and store is the 16-byte form;
  * the kernel lives in that library only, and the tuples the older code-object tests assert keep their values.
"""
import json
import os
import re
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
PINS = os.path.join(REPO, "tests", "isa_pins_features.json")
KERNEL = "damvs::(anonymous namespace)::feature_gather_kernel(damvs::FeaturesArgs)"

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no llvm-objdump")


@pytest.fixture(scope="module")
def features_lib():
    from damvsnet_amd import build
    build.build()
    assert os.path.exists(build.FEATURES_LIB)
    return build.FEATURES_LIB


def test_build_flags_and_library_tuples():
    from damvsnet_amd import build
    assert build.FILE_FLAGS.get("k_features.hip") == ["-fno-slp-vectorize", "-fno-vectorize"]
    assert os.path.basename(build.FEATURES_LIB) == "libdamvs_features.so"
    assert build.FEATURES_UNITS == ("k_features.hip",)
    assert build.LINKED_SIDE_LIBS == build.BUILD_SIDE_LIBS + ((build.FEATURES_LIB, build.FEATURES_UNITS),)
    # the older tuples keep their values (tests/test_cloud_codeobj.py, test_scene_codeobj.py, test_inputs_codeobj.py)
    assert build.SIDE_LIBS == ((build.SIDE_LIB, build.SIDE_UNITS), (build.CLOUD_LIB, build.CLOUD_UNITS))
    assert build.ALL_SIDE_LIBS == build.SIDE_LIBS + ((build.SCENE_LIB, build.SCENE_UNITS),)
    assert build.BUILD_SIDE_LIBS == build.ALL_SIDE_LIBS + ((build.INPUTS_LIB, build.INPUTS_UNITS),)
    with open(os.path.join(REPO, ".gitignore")) as f:
        assert "*.so" in f.read().split()  # built libraries stay out of git


def test_every_side_library_is_built_and_linked(features_lib):
    from damvsnet_amd import build
    for lib, units in build.LINKED_SIDE_LIBS:
        assert os.path.exists(lib), lib
        for u in units:
            assert os.path.exists(os.path.join(build.CSRC, u)), u
    import subprocess
    needed = subprocess.run(["readelf", "-d", build.LIB], capture_output=True, text=True, check=True).stdout
    assert "libdamvs_features.so" in needed


def test_gather_kernel_instruction_stream_is_the_validated_one(features_lib):
    import isa
    with open(PINS) as f:
        pins = json.load(f)
    assert os.path.exists(os.path.join(REPO, pins["validated_by"])), pins["validated_by"]
    assert pins["validated_by"].startswith("profiles/r18/")
    assert list(pins["kernels"]) == [KERNEL]
    if pins["compiler"] != isa.compiler():
        pytest.skip("different compiler (%s): instruction streams are not comparable" % isa.compiler())
    got = isa.hashes(features_lib)
    assert got == pins["kernels"], (got, pins["kernels"])
    from damvsnet_amd import build
    for other in (build.LIB,) + tuple(lib for lib, _ in build.BUILD_SIDE_LIBS):
        assert not [k for k in isa.hashes(other) if "feature_gather" in k], other


def test_gather_kernel_moves_16_byte_vectors_only(features_lib):
    import isa
    ks = isa.disassemble(features_lib)
    assert len(ks) == 1
    for name, body in ks.items():
        assert not any(t.startswith("v_mfma") for t in body)
        assert not [t for t in body if re.match(r"v_pk_\w+_f32\b", t)], name
        mem = [t.split()[0] for t in body if t.startswith(("global_", "buffer_", "flat_", "scratch_", "ds_"))]
        loads = [m for m in mem if "load" in m]
        stores = [m for m in mem if "store" in m]
        assert set(loads) == {"global_load_dwordx4"} and set(stores) == {"global_store_dwordx4"}, mem
        assert len(loads) + len(stores) == len(mem), mem  # nothing else touches memory: no atomics, no LDS
        # four independent vectors per trip of the main loop, one per trip of the tail
        assert len(loads) == len(stores) == 5


def test_gather_kernel_uses_no_scratch_spills_or_lds(features_lib):
    import codeobj_check as C
    ks = C.kernels(features_lib)
    assert len(ks) == 1
    for name, k in ks.items():
        assert not (k["priv"] or k["spill"] or k["sspill"] or k["lds"]), (name, k)
