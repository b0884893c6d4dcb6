"""Build libdamvs.so in-tree with hipcc for gfx950 (no CMake, no JIT cache).

``python -m damvsnet_amd.build`` or ``damvsnet_amd.build.build()``. Objects are compiled in
parallel and linked into ``damvsnet_amd/libdamvs.so`` (and ``libdamvs_fusion.so``, ``libdamvs_cloud.so``,
``libdamvs_scene.so``, ``libdamvs_inputs.so``, ``libdamvs_features.so``, ``libdamvs_thin.so``, ``libdamvs_normals.so``,
``libdamvs_consensus.so`` beside it, SIDE_LIBS_WITH_CONSENSUS). The library carries the sha256 of the sources,
headers and compiler flags it was built from (``damvs_build_id()``, passed as -DDAMVS_BUILD_ID); a rebuild
is skipped only when that stamp (kept beside the library in ``libdamvs.so.build_id``) equals the hash of the
tree, and ``_capi.load_library`` refuses an in-tree library whose embedded stamp differs from the sources
beside it. So the library that runs is provably the build of the sources that travel with it (file times
play no part: a snapshot copied to another machine keeps the check meaningful).
"""
from __future__ import annotations

import concurrent.futures as cf
import glob
import hashlib
import os
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
INCLUDE = os.path.join(REPO, "include")
LIB = os.path.join(PKG, "libdamvs.so")
# Units linked into a library of their own that libdamvs.so depends on (found beside it through an $ORIGIN runpath).
# The static-rule fusion kernel lives there: tests/isa_pins.json pins the kernels of libdamvs.so,
# tests/isa_pins_fusion.json the kernels of this one.
SIDE_LIB = os.path.join(PKG, "libdamvs_fusion.so")
SIDE_UNITS = ("k_fusion_static.hip",)
# The point-cloud compaction kernels (count, scan, scatter), pinned by tests/isa_pins_cloud.json.
CLOUD_LIB = os.path.join(PKG, "libdamvs_cloud.so")
CLOUD_UNITS = ("k_cloud.hip",)
# every side library with its units, in link order (all before libdamvs.so)
SIDE_LIBS = ((SIDE_LIB, SIDE_UNITS), (CLOUD_LIB, CLOUD_UNITS))
# The scene ingest kernel, pinned by tests/isa_pins_scene.json. tests/isa_pins.json is the inventory of libdamvs.so
# (tests/test_isa_pins.py and tests/test_fusion_static_codeobj.py take a kernel there that it does not list for a changed
# one), so a new kernel gets a library and a pin file of its own, as the two above did. SIDE_LIBS stays the fusion pair
# that tests/test_cloud_codeobj.py describes.
SCENE_LIB = os.path.join(PKG, "libdamvs_scene.so")
SCENE_UNITS = ("k_scene.hip",)
ALL_SIDE_LIBS = SIDE_LIBS + ((SCENE_LIB, SCENE_UNITS),)
# The scene inputs kernel, pinned by tests/isa_pins_inputs.json. ALL_SIDE_LIBS stays the three libraries that
# tests/test_scene_codeobj.py describes; BUILD_SIDE_LIBS is what the build links and checks.
INPUTS_LIB = os.path.join(PKG, "libdamvs_inputs.so")
INPUTS_UNITS = ("k_inputs.hip",)
BUILD_SIDE_LIBS = ALL_SIDE_LIBS + ((INPUTS_LIB, INPUTS_UNITS),)
# The scene features gather kernel, pinned by tests/isa_pins_features.json. BUILD_SIDE_LIBS stays the four libraries
# that tests/test_inputs_codeobj.py describes; LINKED_SIDE_LIBS is what the build links and checks.
FEATURES_LIB = os.path.join(PKG, "libdamvs_features.so")
FEATURES_UNITS = ("k_features.hip",)
LINKED_SIDE_LIBS = BUILD_SIDE_LIBS + ((FEATURES_LIB, FEATURES_UNITS),)
# The voxel thinning kernels (claim, resolve), pinned by tests/isa_pins_thin.json. LINKED_SIDE_LIBS stays the five
# libraries that tests/test_features_codeobj.py describes; EVERY_SIDE_LIB is what the build links and checks.
THIN_LIB = os.path.join(PKG, "libdamvs_thin.so")
THIN_UNITS = ("k_thin.hip",)
EVERY_SIDE_LIB = LINKED_SIDE_LIBS + ((THIN_LIB, THIN_UNITS),)
# The point-normal kernels (map, oriented scatter), pinned by tests/isa_pins_normals.json. EVERY_SIDE_LIB stays the six
# libraries that tests/test_thin_codeobj.py describes.
NORMALS_LIB = os.path.join(PKG, "libdamvs_normals.so")
NORMALS_UNITS = ("k_normals.hip",)
SIDE_LIBS_WITH_NORMALS = EVERY_SIDE_LIB + ((NORMALS_LIB, NORMALS_UNITS),)
# The consensus fusion kernel, pinned by tests/isa_pins_consensus.json. SIDE_LIBS_WITH_NORMALS stays the seven libraries
# that tests/test_normals_codeobj.py describes; SIDE_LIBS_WITH_CONSENSUS is what the build links and checks.
CONSENSUS_LIB = os.path.join(PKG, "libdamvs_consensus.so")
CONSENSUS_UNITS = ("k_consensus.hip",)
SIDE_LIBS_WITH_CONSENSUS = SIDE_LIBS_WITH_NORMALS + ((CONSENSUS_LIB, CONSENSUS_UNITS),)
STAMP = LIB + ".build_id"
OBJ = os.path.join(PKG, "build_obj")
ARCH = os.environ.get("DAMVS_ARCH", "gfx950")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

CFLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=" + ARCH, "-I" + INCLUDE, "-I" + CSRC,
          "-Wall", "-Wno-unused-function", "-Wno-unused-variable"]

# Per-file extra flags. k_warp.hip is built without the SLP vectorizer so that its kernels carry no packed-FP32 VALU
# ops (v_pk_fma/mul/add_f32): with those, the warp kernels' lanes 48-63 computed wrong tap coordinates while MFMA
# kernels of another stream shared the CU (DESIGN.md §4 "Concurrent streams"; profiles/r05/diag_streams/r05w).
FILE_FLAGS = {"k_warp.hip": ["-fno-slp-vectorize"]}
# Round 6 widened the rule to every kernel without MFMA instructions that can share a CU with another stream's MFMA
# kernels (tests/test_isa_pins.py test_valu_kernels_carry_no_packed_fp32_ops): the plane-input conv2d layers
# (k_planes.hip), the hypotheses / GeoFF depth pyramid / camera algebra (k_geometry.hip), the VALU prob conv,
# regression, range check and magnitude kernels (k_regress.hip) and depth fusion (k_fusion.hip).
# Both vectorizers are off there: the loop vectorizer, too, emits packed-FP32 ops (grid-stride loops by two).
for _f in ("k_planes.hip", "k_geometry.hip", "k_regress.hip", "k_fusion.hip", "k_fusion_static.hip", "k_cloud.hip",
           "k_scene.hip", "k_inputs.hip", "k_features.hip", "k_thin.hip"):
    FILE_FLAGS[_f] = ["-fno-slp-vectorize", "-fno-vectorize"]
# k_normals.hip must equal fusion.normals_statement bit for bit: no multiply-add may be contracted there either.
FILE_FLAGS["k_normals.hip"] = ["-fno-slp-vectorize", "-fno-vectorize", "-ffp-contract=off"]
# k_consensus.hip must equal fusion.consensus_statement bit for bit in the same way.
FILE_FLAGS["k_consensus.hip"] = ["-fno-slp-vectorize", "-fno-vectorize", "-ffp-contract=off"]


def sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.cpp")))


def _inputs():
    return sources() + sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(INCLUDE, "*.h")))


def source_hash(arch: str | None = None) -> str:
    """First 16 hex digits of sha256 over (path relative to the repo, contents) of every source and header, plus
    the compiler flags that do not depend on where the repo lives (``arch``: the offload arch to hash the flags for,
    default DAMVS_ARCH / gfx950)."""
    h = hashlib.sha256()
    for p in _inputs():
        h.update(os.path.relpath(p, REPO).encode() + b"\0")
        with open(p, "rb") as f:
            h.update(f.read())
        h.update(b"\0")
    flags = [f for f in CFLAGS if not f.startswith("-I")]
    if arch is not None:
        flags = ["--offload-arch=" + arch if f.startswith("--offload-arch=") else f for f in flags]
    h.update(" ".join(flags).encode())
    for name in sorted(FILE_FLAGS):
        h.update(("\0%s:%s" % (name, " ".join(FILE_FLAGS[name]))).encode())
    return h.hexdigest()[:16]


def stamp() -> str | None:
    try:
        with open(STAMP) as f:
            return f.read().strip()
    except OSError:
        return None


def _stale(want: str) -> bool:
    return not all(os.path.exists(p) for p in (LIB,) + tuple(lib for lib, _ in SIDE_LIBS_WITH_CONSENSUS)) or stamp() != want


def _compile(src, build_id):
    obj = os.path.join(OBJ, os.path.basename(src) + ".o")
    cmd = [HIPCC] + CFLAGS + FILE_FLAGS.get(os.path.basename(src), []) + \
        ['-DDAMVS_BUILD_ID="%s"' % build_id, "-x", "hip", "-c", src, "-o", obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s\n%s" % (src, " ".join(cmd), r.stderr))
    return obj, r.stderr


def build(force: bool = False, verbose: bool = False) -> str:
    want = source_hash()
    if not force and not _stale(want):
        if verbose:
            print("libdamvs.so up to date: build id %s == sources %s" % (stamp(), want), file=sys.stderr)
        return LIB
    os.makedirs(OBJ, exist_ok=True)
    srcs = sources()
    with cf.ThreadPoolExecutor(max_workers=min(8, len(srcs))) as ex:
        results = list(ex.map(lambda s: _compile(s, want), srcs))
    objs = [o for o, _ in results]
    if verbose:
        for (_, err), s in zip(results, srcs):
            if err.strip():
                print("[%s]\n%s" % (os.path.basename(s), err), file=sys.stderr)
    unit = lambda o: os.path.basename(o)[:-2]
    side_units = [u for _, units in SIDE_LIBS_WITH_CONSENSUS for u in units]
    # libdamvs.so finds the side libraries beside itself ($ORIGIN); the package directory it was built in follows, so
    # that a copy of libdamvs.so placed beside a replacement of one of them (tests/test_fusion_static.py
    # test_foreign_fusion_library_is_refused) still loads the others from here
    links = [(lib, [o for o in objs if unit(o) in units], ["-Wl,-soname," + os.path.basename(lib)])
             for lib, units in SIDE_LIBS_WITH_CONSENSUS]
    links.append((LIB, [o for o in objs if unit(o) not in side_units],
                  [lib for lib, _ in SIDE_LIBS_WITH_CONSENSUS] + ["-Wl,-rpath,$ORIGIN:" + PKG]))
    for lib, members, extra in links:
        tmp = lib + ".tmp"
        cmd = [HIPCC, "-shared", "-fPIC", "--offload-arch=" + ARCH, "-o", tmp] + members + extra
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("link failed:\n%s\n%s" % (" ".join(cmd), r.stderr))
        os.replace(tmp, lib)
    with open(STAMP, "w") as f:
        f.write(want + "\n")
    if verbose:
        print("libdamvs.so built from sources %s" % want, file=sys.stderr)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
