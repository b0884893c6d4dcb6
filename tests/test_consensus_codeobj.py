"""CPU: the code object of the consensus fusion kernel (damvsnet_amd/libdamvs_consensus.so, built from k_consensus.hip).

The rules tests/test_normals_codeobj.py applies to libdamvs_normals.so, for the ninth library (build.py
SIDE_LIBS_WITH_CONSENSUS):
  * its kernel set and instruction stream equal the ones the GPU run ran: tests/isa_pins_consensus.json, whose
    `validated_by` is the committed log of tests/test_gpu_consensus.py on that build, the launch beside a bf16 forward on
    another stream included (renew with `python tools/isa.py --lib damvsnet_amd/libdamvs_consensus.so --pins
    tests/isa_pins_consensus.json --update-pins --validated-by <that log>`);
  * no MFMA and no packed-FP32 VALU ops of any kind (built without the SLP and loop vectorizers, as every kernel without
    MFMA instructions: it can share a CU with another stream's MFMA kernels);
  * no private segment, no spills, no AGPRs, no LDS; no atomics; the scene table is read by scalar loads;
  * the kernel lives in that library only, and the tuples the older code-object tests assert keep their values.
"""
import json
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
PINS = os.path.join(REPO, "tests", "isa_pins_consensus.json")
KERNEL = "damvs::(anonymous namespace)::consensus_view_kernel(damvs::ConsensusArgs)"
SHORT = "consensus_view_kernel"
OLD_PINS = ("isa_pins.json", "isa_pins_fusion.json", "isa_pins_cloud.json", "isa_pins_scene.json",
            "isa_pins_inputs.json", "isa_pins_features.json", "isa_pins_thin.json", "isa_pins_normals.json")

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no llvm-objdump")


@pytest.fixture(scope="module")
def consensus_lib():
    from damvsnet_amd import build
    build.build()
    assert os.path.exists(build.CONSENSUS_LIB)
    return build.CONSENSUS_LIB


def test_build_flags_and_library_tuples():
    from damvsnet_amd import build
    assert build.FILE_FLAGS.get("k_consensus.hip") == ["-fno-slp-vectorize", "-fno-vectorize", "-ffp-contract=off"]
    assert build.FILE_FLAGS.get("k_consensus.hip") == build.FILE_FLAGS.get("k_normals.hip")
    assert os.path.basename(build.CONSENSUS_LIB) == "libdamvs_consensus.so"
    assert build.CONSENSUS_UNITS == ("k_consensus.hip",)
    assert build.SIDE_LIBS_WITH_CONSENSUS == build.SIDE_LIBS_WITH_NORMALS + ((build.CONSENSUS_LIB, build.CONSENSUS_UNITS),)
    # the older tuples keep their values (tests/test_cloud_codeobj.py ... tests/test_normals_codeobj.py)
    assert build.SIDE_LIBS == ((build.SIDE_LIB, build.SIDE_UNITS), (build.CLOUD_LIB, build.CLOUD_UNITS))
    assert build.ALL_SIDE_LIBS == build.SIDE_LIBS + ((build.SCENE_LIB, build.SCENE_UNITS),)
    assert build.BUILD_SIDE_LIBS == build.ALL_SIDE_LIBS + ((build.INPUTS_LIB, build.INPUTS_UNITS),)
    assert build.LINKED_SIDE_LIBS == build.BUILD_SIDE_LIBS + ((build.FEATURES_LIB, build.FEATURES_UNITS),)
    assert build.EVERY_SIDE_LIB == build.LINKED_SIDE_LIBS + ((build.THIN_LIB, build.THIN_UNITS),)
    assert build.SIDE_LIBS_WITH_NORMALS == build.EVERY_SIDE_LIB + ((build.NORMALS_LIB, build.NORMALS_UNITS),)
    assert len(build.SIDE_LIBS_WITH_CONSENSUS) == 8 and len({lib for lib, _ in build.SIDE_LIBS_WITH_CONSENSUS}) == 8
    with open(os.path.join(REPO, ".gitignore")) as f:
        assert "*.so" in f.read().split()  # built libraries stay out of git


def test_every_side_library_is_built_and_linked(consensus_lib):
    from damvsnet_amd import build
    for lib, units in build.SIDE_LIBS_WITH_CONSENSUS:
        assert os.path.exists(lib), lib
        for u in units:
            assert os.path.exists(os.path.join(build.CSRC, u)), u
    needed = subprocess.run(["readelf", "-d", build.LIB], capture_output=True, text=True, check=True).stdout
    for lib, _ in build.SIDE_LIBS_WITH_CONSENSUS:
        assert os.path.basename(lib) in needed, lib
    soname = subprocess.run(["readelf", "-d", consensus_lib], capture_output=True, text=True, check=True).stdout
    assert "soname: [libdamvs_consensus.so]" in soname


def test_consensus_kernel_instruction_stream_is_the_validated_one(consensus_lib):
    import isa
    with open(PINS) as f:
        pins = json.load(f)
    assert os.path.exists(os.path.join(REPO, pins["validated_by"])), pins["validated_by"]
    assert pins["validated_by"] == "profiles/r21/pytest_gpu_consensus.txt"
    assert sorted(pins["kernels"]) == [KERNEL]
    if pins["compiler"] != isa.compiler():
        pytest.skip("different compiler (%s): instruction streams are not comparable" % isa.compiler())
    got = isa.hashes(consensus_lib)
    assert got == pins["kernels"], (got, pins["kernels"])
    from damvsnet_amd import build
    for other in (build.LIB,) + tuple(lib for lib, _ in build.SIDE_LIBS_WITH_NORMALS):
        assert not [k for k in isa.hashes(other) if SHORT in k], other
    for name in OLD_PINS:  # and no older pin file lists it
        with open(os.path.join(REPO, "tests", name)) as f:
            assert not [k for k in json.load(f)["kernels"] if SHORT in k], name


def test_consensus_kernel_instructions(consensus_lib):
    import isa
    ks = isa.disassemble(consensus_lib)
    assert len(ks) == 1
    for name, body in ks.items():
        assert SHORT in name
        assert not any(t.startswith("v_mfma") for t in body)
        assert not [t for t in body if re.match(r"v_pk_\w+_f32\b", t)]
        assert not [t for t in body if t.startswith("scratch_")]
        assert not [t for t in body if t.startswith("ds_")]
        assert not [t for t in body if "atomic" in t]
        # the marks are byte stores from vector lanes, the maps are read as global memory, the table by scalar loads
        assert [t for t in body if t.startswith("global_store_byte")]
        assert not [t for t in body if t.startswith("flat_")]
        assert len([t for t in body if t.startswith("s_load_dwordx8") or t.startswith("s_load_dwordx16")]) >= 4
        # double arithmetic, one operation at a time: the only fused multiply-adds are the division's own refinement
        # steps (5 per v_div_scale pair)
        divisions = len([t for t in body if t.startswith("v_div_fixup_f64")])
        fused = len([t for t in body if re.match(r"v_fma(c|_)?_?f64", t) or t.startswith("v_fmac_f64")])
        assert divisions == 7 and fused == 5 * divisions, (divisions, fused)


def test_consensus_kernel_uses_no_scratch_spills_agprs_or_lds(consensus_lib):
    import codeobj_check as C
    ks = C.kernels(consensus_lib)
    assert len(ks) == 1
    for name, k in ks.items():
        assert not (k["priv"] or k["spill"] or k["sspill"] or k["agpr"] or k["lds"]), (name, k)
