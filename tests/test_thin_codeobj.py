"""CPU: the code object of the voxel thinning kernels (damvsnet_amd/libdamvs_thin.so, built from k_thin.hip).

The rules tests/test_features_codeobj.py applies to libdamvs_features.so, for the seventh library (build.py
EVERY_SIDE_LIB):
  * its kernel set and instruction streams equal the ones the GPU run ran: tests/isa_pins_thin.json, whose
    `validated_by` is the committed log of tests/test_gpu_thin.py on that build, the launch beside a bf16 forward on
    another stream included (renew with `python tools/isa.py --lib damvsnet_amd/libdamvs_thin.so --pins
    tests/isa_pins_thin.json --update-pins --validated-by <that log>`);
  * no MFMA and no packed-FP32 VALU ops of any kind (built without the SLP and loop vectorizers, as every kernel without
    MFMA instructions: it can share a CU with another stream's MFMA kernels);
  * no scratch, no spills, no LDS;
  * claim touches the table through returning 64-bit compare-and-swaps and 64-bit unsigned minima only and loads
    nothing from it; resolve stores one byte per pixel and issues no atomic;
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
PINS = os.path.join(REPO, "tests", "isa_pins_thin.json")
CLAIM = "damvs::(anonymous namespace)::thin_claim_kernel(damvs::ThinArgs)"
RESOLVE = "damvs::(anonymous namespace)::thin_resolve_kernel(damvs::ThinArgs)"
OLD_PINS = ("isa_pins.json", "isa_pins_fusion.json", "isa_pins_cloud.json", "isa_pins_scene.json",
            "isa_pins_inputs.json", "isa_pins_features.json")

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no llvm-objdump")


@pytest.fixture(scope="module")
def thin_lib():
    from damvsnet_amd import build
    build.build()
    assert os.path.exists(build.THIN_LIB)
    return build.THIN_LIB


def test_build_flags_and_library_tuples():
    from damvsnet_amd import build
    assert build.FILE_FLAGS.get("k_thin.hip") == ["-fno-slp-vectorize", "-fno-vectorize"]
    assert os.path.basename(build.THIN_LIB) == "libdamvs_thin.so"
    assert build.THIN_UNITS == ("k_thin.hip",)
    assert build.EVERY_SIDE_LIB == build.LINKED_SIDE_LIBS + ((build.THIN_LIB, build.THIN_UNITS),)
    # the older tuples keep their values (tests/test_cloud_codeobj.py, test_scene_codeobj.py, test_inputs_codeobj.py,
    # test_features_codeobj.py)
    assert build.SIDE_LIBS == ((build.SIDE_LIB, build.SIDE_UNITS), (build.CLOUD_LIB, build.CLOUD_UNITS))
    assert build.ALL_SIDE_LIBS == build.SIDE_LIBS + ((build.SCENE_LIB, build.SCENE_UNITS),)
    assert build.BUILD_SIDE_LIBS == build.ALL_SIDE_LIBS + ((build.INPUTS_LIB, build.INPUTS_UNITS),)
    assert build.LINKED_SIDE_LIBS == build.BUILD_SIDE_LIBS + ((build.FEATURES_LIB, build.FEATURES_UNITS),)
    assert len(build.EVERY_SIDE_LIB) == 6 and len({lib for lib, _ in build.EVERY_SIDE_LIB}) == 6
    with open(os.path.join(REPO, ".gitignore")) as f:
        assert "*.so" in f.read().split()  # built libraries stay out of git


def test_every_side_library_is_built_and_linked(thin_lib):
    from damvsnet_amd import build
    for lib, units in build.EVERY_SIDE_LIB:
        assert os.path.exists(lib), lib
        for u in units:
            assert os.path.exists(os.path.join(build.CSRC, u)), u
    needed = subprocess.run(["readelf", "-d", build.LIB], capture_output=True, text=True, check=True).stdout
    for lib, _ in build.EVERY_SIDE_LIB:
        assert os.path.basename(lib) in needed, lib
    soname = subprocess.run(["readelf", "-d", thin_lib], capture_output=True, text=True, check=True).stdout
    assert "soname: [libdamvs_thin.so]" in soname


def test_thin_kernels_instruction_streams_are_the_validated_ones(thin_lib):
    import isa
    with open(PINS) as f:
        pins = json.load(f)
    assert os.path.exists(os.path.join(REPO, pins["validated_by"])), pins["validated_by"]
    assert pins["validated_by"].startswith("profiles/r19/")
    assert sorted(pins["kernels"]) == sorted([CLAIM, RESOLVE])
    if pins["compiler"] != isa.compiler():
        pytest.skip("different compiler (%s): instruction streams are not comparable" % isa.compiler())
    got = isa.hashes(thin_lib)
    assert got == pins["kernels"], (got, pins["kernels"])
    from damvsnet_amd import build
    for other in (build.LIB,) + tuple(lib for lib, _ in build.LINKED_SIDE_LIBS):
        assert not [k for k in isa.hashes(other) if "thin_" in k], other
    # and no older pin file lists them
    for name in OLD_PINS:
        with open(os.path.join(REPO, "tests", name)) as f:
            assert not [k for k in json.load(f)["kernels"] if "thin_" in k], name


def test_thin_kernels_memory_operations(thin_lib):
    import isa
    ks = isa.disassemble(thin_lib)
    assert len(ks) == 2
    mem = {}
    for name, body in ks.items():
        name, = [k for short, k in (("thin_claim_kernel", CLAIM), ("thin_resolve_kernel", RESOLVE)) if short in name]
        assert not any(t.startswith("v_mfma") for t in body), name
        assert not [t for t in body if re.match(r"v_pk_\w+_f32\b", t)], name
        ops = [t for t in body if t.startswith(("global_", "buffer_", "flat_", "scratch_", "ds_"))]
        assert all(t.startswith("global_") for t in ops), (name, ops)  # no LDS, no scratch, no flat addressing
        mem[name] = ops
    op = lambda t: t.split()[0]
    claim = [op(t) for t in mem[CLAIM]]
    # the mask byte and the point are the only loads: nothing of the table is read by a plain load
    assert sorted(o for o in claim if "load" in o) == ["global_load_dwordx3", "global_load_ubyte"]
    assert not [o for o in claim if "store" in o]
    atomics = [t for t in mem[CLAIM] if "atomic" in t]
    assert sorted(set(op(t) for t in atomics)) == ["global_atomic_cmpswap_x2", "global_atomic_or",
                                                    "global_atomic_umin_x2"]
    cas, = [t for t in atomics if op(t) == "global_atomic_cmpswap_x2"]
    assert cas.split()[-1] == "sc0"  # the returning form: the probe decides on the value that comes back
    assert len(claim) == len(atomics) + 2
    resolve = [op(t) for t in mem[RESOLVE]]
    assert not [o for o in resolve if "atomic" in o]
    assert [o for o in resolve if "store" in o] == ["global_store_byte"]
    assert set(o for o in resolve if "load" in o) == {"global_load_ubyte", "global_load_dwordx3", "global_load_dwordx2"}


def test_thin_kernels_use_no_scratch_spills_or_lds(thin_lib):
    import codeobj_check as C
    ks = C.kernels(thin_lib)
    assert len(ks) == 2
    for name, k in ks.items():
        assert not (k["priv"] or k["spill"] or k["sspill"] or k["lds"] or k["agpr"]), (name, k)
