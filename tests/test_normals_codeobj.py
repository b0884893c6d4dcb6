"""CPU: the code object of the point-normal kernels (damvsnet_amd/libdamvs_normals.so, built from k_normals.hip).

The rules tests/test_thin_codeobj.py applies to libdamvs_thin.so, for the eighth library (build.py
SIDE_LIBS_WITH_NORMALS):
  * its kernel set and instruction streams equal the ones the GPU run ran: tests/isa_pins_normals.json, whose
    `validated_by` is the committed log of tests/test_gpu_normals.py on that build, the launch beside a bf16 forward on
    another stream included (renew with `python tools/isa.py --lib damvsnet_amd/libdamvs_normals.so --pins
    tests/isa_pins_normals.json --update-pins --validated-by <that log>`);
  * no MFMA and no packed-FP32 VALU ops of any kind (built without the SLP and loop vectorizers, as every kernel without
    MFMA instructions: it can share a CU with another stream's MFMA kernels);
  * no scratch and no spills; LDS in the scatter only;
  * the kernels live in that library only, and the tuples the older code-object tests assert keep their values.
"""
import json
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
PINS = os.path.join(REPO, "tests", "isa_pins_normals.json")
MAP = "damvs::(anonymous namespace)::normal_map_kernel(damvs::NormalArgs)"
SCATTER = "damvs::(anonymous namespace)::cloud_scatter_oriented_kernel(damvs::NormalArgs)"
SHORT = ("normal_map_kernel", "cloud_scatter_oriented_kernel")
OLD_PINS = ("isa_pins.json", "isa_pins_fusion.json", "isa_pins_cloud.json", "isa_pins_scene.json",
            "isa_pins_inputs.json", "isa_pins_features.json", "isa_pins_thin.json")

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no llvm-objdump")


@pytest.fixture(scope="module")
def normals_lib():
    from damvsnet_amd import build
    build.build()
    assert os.path.exists(build.NORMALS_LIB)
    return build.NORMALS_LIB


def test_build_flags_and_library_tuples():
    from damvsnet_amd import build
    assert build.FILE_FLAGS.get("k_normals.hip") == ["-fno-slp-vectorize", "-fno-vectorize", "-ffp-contract=off"]
    assert os.path.basename(build.NORMALS_LIB) == "libdamvs_normals.so"
    assert build.NORMALS_UNITS == ("k_normals.hip",)
    assert build.SIDE_LIBS_WITH_NORMALS == build.EVERY_SIDE_LIB + ((build.NORMALS_LIB, build.NORMALS_UNITS),)
    # the older tuples keep their values (tests/test_cloud_codeobj.py, test_scene_codeobj.py, test_inputs_codeobj.py,
    # test_features_codeobj.py, test_thin_codeobj.py)
    assert build.SIDE_LIBS == ((build.SIDE_LIB, build.SIDE_UNITS), (build.CLOUD_LIB, build.CLOUD_UNITS))
    assert build.ALL_SIDE_LIBS == build.SIDE_LIBS + ((build.SCENE_LIB, build.SCENE_UNITS),)
    assert build.BUILD_SIDE_LIBS == build.ALL_SIDE_LIBS + ((build.INPUTS_LIB, build.INPUTS_UNITS),)
    assert build.LINKED_SIDE_LIBS == build.BUILD_SIDE_LIBS + ((build.FEATURES_LIB, build.FEATURES_UNITS),)
    assert build.EVERY_SIDE_LIB == build.LINKED_SIDE_LIBS + ((build.THIN_LIB, build.THIN_UNITS),)
    assert len(build.SIDE_LIBS_WITH_NORMALS) == 7 and len({lib for lib, _ in build.SIDE_LIBS_WITH_NORMALS}) == 7
    with open(os.path.join(REPO, ".gitignore")) as f:
        assert "*.so" in f.read().split()  # built libraries stay out of git


def test_every_side_library_is_built_and_linked(normals_lib):
    from damvsnet_amd import build
    for lib, units in build.SIDE_LIBS_WITH_NORMALS:
        assert os.path.exists(lib), lib
        for u in units:
            assert os.path.exists(os.path.join(build.CSRC, u)), u
    needed = subprocess.run(["readelf", "-d", build.LIB], capture_output=True, text=True, check=True).stdout
    for lib, _ in build.SIDE_LIBS_WITH_NORMALS:
        assert os.path.basename(lib) in needed, lib
    soname = subprocess.run(["readelf", "-d", normals_lib], capture_output=True, text=True, check=True).stdout
    assert "soname: [libdamvs_normals.so]" in soname


def test_normal_kernels_instruction_streams_are_the_validated_ones(normals_lib):
    import isa
    with open(PINS) as f:
        pins = json.load(f)
    assert os.path.exists(os.path.join(REPO, pins["validated_by"])), pins["validated_by"]
    assert pins["validated_by"] == "profiles/r20/pytest_gpu_normals.txt"
    assert sorted(pins["kernels"]) == sorted([MAP, SCATTER])
    if pins["compiler"] != isa.compiler():
        pytest.skip("different compiler (%s): instruction streams are not comparable" % isa.compiler())
    got = isa.hashes(normals_lib)
    assert got == pins["kernels"], (got, pins["kernels"])
    from damvsnet_amd import build
    for other in (build.LIB,) + tuple(lib for lib, _ in build.EVERY_SIDE_LIB):
        assert not [k for k in isa.hashes(other) if any(s in k for s in SHORT)], other
    # and no older pin file lists them
    for name in OLD_PINS:
        with open(os.path.join(REPO, "tests", name)) as f:
            assert not [k for k in json.load(f)["kernels"] if any(s in k for s in SHORT)], name


def test_normal_kernels_carry_no_mfma_and_no_packed_fp32(normals_lib):
    import isa
    ks = isa.disassemble(normals_lib)
    assert len(ks) == 2
    for name, body in ks.items():
        assert any(s in name for s in SHORT), name
        assert not any(t.startswith("v_mfma") for t in body), name
        assert not [t for t in body if re.match(r"v_pk_\w+_f32\b", t)], name
        assert not [t for t in body if t.startswith("scratch_")], name
        lds = [t for t in body if t.startswith("ds_")]
        assert bool(lds) == ("cloud_scatter_oriented_kernel" in name), (name, lds[:4])


def test_normal_kernels_use_no_scratch_or_spills_and_lds_in_the_scatter_only(normals_lib):
    import codeobj_check as C
    ks = C.kernels(normals_lib)
    assert len(ks) == 2
    for name, k in ks.items():
        assert not (k["priv"] or k["spill"] or k["sspill"] or k["agpr"]), (name, k)
        assert bool(k["lds"]) == ("cloud_scatter_oriented_kernel" in name), (name, k)
