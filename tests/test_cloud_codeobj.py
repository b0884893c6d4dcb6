"""CPU: the code object of the point-cloud compaction kernels (damvsnet_amd/libdamvs_cloud.so, built from k_cloud.hip).

The rules tests/test_fusion_static_codeobj.py applies to libdamvs_fusion.so, for the third library (build.py SIDE_LIBS):
  * its kernel set and instruction streams equal the ones the GPU stream tests last ran beside
    (tests/isa_pins_cloud.json; renew with `python tools/isa.py --lib damvsnet_amd/libdamvs_cloud.so --pins
    tests/isa_pins_cloud.json --update-pins --validated-by <committed log of tests/test_gpu_streams.py on that build>`);
  * no packed-FP32 VALU ops (built without the SLP and loop vectorizers, as every kernel without MFMA instructions);
  * no scratch, no spills. LDS is used: the per-wave totals of the rank and the scatter's staged records.
The three pin files together cover every kernel the package launches: libdamvs.so holds nothing that
tests/isa_pins.json does not know, and the cloud kernels are in no other library.
"""
import json
import os
import re
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
PINS = os.path.join(REPO, "tests", "isa_pins_cloud.json")
KERNELS = ["damvs::(anonymous namespace)::cloud_count_kernel(damvs::CloudArgs)",
           "damvs::(anonymous namespace)::cloud_scan_kernel(unsigned int*, unsigned int, unsigned long long*)",
           "damvs::(anonymous namespace)::cloud_scatter_kernel(damvs::CloudArgs)"]

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="no llvm-objdump")


@pytest.fixture(scope="module")
def cloud_lib():
    from damvsnet_amd import build
    build.build()
    assert os.path.exists(build.CLOUD_LIB)
    return build.CLOUD_LIB


def test_build_lists_the_cloud_library():
    from damvsnet_amd import build
    assert os.path.basename(build.CLOUD_LIB) == "libdamvs_cloud.so" and build.CLOUD_UNITS == ("k_cloud.hip",)
    assert build.SIDE_LIBS == ((build.SIDE_LIB, build.SIDE_UNITS), (build.CLOUD_LIB, build.CLOUD_UNITS))
    assert os.path.basename(build.SIDE_LIB) == "libdamvs_fusion.so" and build.SIDE_UNITS == ("k_fusion_static.hip",)


def test_cloud_kernel_instruction_streams_are_the_validated_ones(cloud_lib):
    import isa
    with open(PINS) as f:
        pins = json.load(f)
    assert os.path.exists(os.path.join(REPO, pins["validated_by"])), pins["validated_by"]
    assert pins["validated_by"].startswith("profiles/r13/")
    if pins["compiler"] != isa.compiler():
        pytest.skip("different compiler (%s): instruction streams are not comparable" % isa.compiler())
    got = isa.hashes(cloud_lib)
    assert got == pins["kernels"], (got, pins["kernels"])
    assert sorted(got) == KERNELS
    from damvsnet_amd import build
    for other in (build.LIB, build.SIDE_LIB):  # and the kernels live in this library only
        assert not [k for k in isa.hashes(other) if "cloud_" in k], other


def test_cloud_kernels_carry_no_packed_fp32_ops(cloud_lib):
    import isa
    from damvsnet_amd import build
    assert build.FILE_FLAGS.get("k_cloud.hip") == ["-fno-slp-vectorize", "-fno-vectorize"]
    ks = isa.disassemble(cloud_lib)
    assert len(ks) == 3
    pk = re.compile(r"v_pk_(fma|mul|add|mov)_f32\b")
    for name, body in ks.items():
        assert not any(t.startswith("v_mfma") for t in body)
        assert not [t for t in body if pk.match(t)], name


def test_cloud_kernels_use_no_scratch_or_spills(cloud_lib):
    import codeobj_check as C
    ks = C.kernels(cloud_lib)
    assert len(ks) == 3
    for name, k in ks.items():
        assert not (k["priv"] or k["spill"] or k["sspill"]), (name, k)
    lds = {n: k["lds"] for n, k in ks.items()}
    assert all(0 < v <= 4096 for v in lds.values()), lds  # wave totals; the scatter's 256 staged records
