"""Depth-map fusion on the GPU: the reference's two runnable filters
(test_uni.py --filter_method) with the per-pixel reprojection checks in one HIP kernel per reference view
(k_fusion.hip):
  method="dypcd"  the dynamic-consistency filter (filter/dypcd.py, `dypcd_filter` / `filter_depth`): masks at
                  i * dist_base pixels and i * rel_diff_base relative depth, i = 2..10, a pixel kept when i views
                  agree at some i (damvs_fusion_view);
  method="pcd"    the static CasMVSNet filter (filter/pcd.py): one mask per source at dist_thr pixels and rel_thr
                  relative depth (the reference's constants 1 and 0.01), a pixel kept when at least thres_view
                  sources agree (damvs_fusion_view_static).
The third method, gipuma, hands the maps to the external fusibile binary, which the reference does not ship; METHODS
stays these two and method="gipuma" raises. The fusibile family has its own entry points here, below.

`fuse_view` is the per-view primitive (device tensors in, averaged depth / masks / world points
out); `filter_depth` mirrors filter/dypcd.py:179-326 / filter/pcd.py:116-233 over a scene directory written by
the test path (cams/, images/, depth_est/, confidence/ PFMs; see mvsio.save_stage_outputs) and writes the
masks and the PLY point cloud. The reference's defaults (test_uni.py:104-109): conf (0.1, 0.15, 0.9),
dist_base 1/4, rel_diff_base 1/1300, thres_view 5.

`fuse_scene` is filter_depth with the scene kept on the device: every map uploaded once, and the coloured points of
each view appended in pixel order to one device buffer by `compact_cloud` (k_cloud.hip, damvs_fusion_cloud), so that
one copy of count * 15 bytes is the PLY's body. Same files in, same files out.

`voxel=` on the scene-level drivers (fuse_scene, fuse_resident, scene.SceneMaps.fuse, scene.reconstruct_scene) thins
the cloud on the device, between the fusion kernel and compact_cloud: at most one point per cell of an axis-aligned
grid of that edge, the first one in PLY order (VoxelGrid, k_thin.hip; `voxel_first` is the rule in numpy). The records
are unchanged, so the thinned PLY is a subsequence of the unthinned one. voxel=None, the default, is the path above.

`normals=True` on the same drivers and on filter_depth writes an oriented cloud, 27 bytes a point (x, y, z, nx, ny, nz,
red, green, blue): each point's normal from its pixel's neighbours in the view's averaged depth map, facing the view's
camera (`normals_statement` is the rule in numpy; k_normals.hip computes it inside compact_cloud's scatter, bit for
bit). normals=False, the default, is the path above.

Consensus fusion (`fuse_consensus_scene`, `fuse_consensus_resident`, `consensus_view`; scene.SceneMaps.fuse_consensus,
scene.reconstruct_scene(fusion="consensus")) is the fusibile family's rule over all views of a scene: a depth sample
merged into a point is consumed and is not emitted again from its own view, the point written is the average of the
agreeing views' 3D points and its colour the average of their colours. `consensus_statement` is the rule in numpy, with
the thresholds the reference passes to the binary (test_uni.py:114-116, gipuma.py:170-187); k_consensus.hip, one launch
per reference view over a scene table in device memory (damvs_consensus_view), equals it bit for bit. It is this
project's statement of the published algorithm; the stated difference (the disparity test compares the depth of the
point in the source camera, not the reference pixel's own depth, with the source's depth) is in the statement's
docstring, and parity with the binary, which is not available, is unverified. Its
per-view outputs are the maps compact_cloud and VoxelGrid.claim take, so voxel=, max_points and normals=True compose.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

from . import _capi, mvsio
from ._capi import check


def fusion_cams(K_ref, E_ref, srcs):
    """Camera products as the reference forms them: float32 numpy inverses and float32 4x4 products
    (filter/dypcd.py:104-123), packed into damvs_fusion_cams."""
    c = _capi.DamvsFusionCams()
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    K_ref, E_ref = f32(K_ref), f32(E_ref)
    put = lambda dst, a: ctypes.memmove(dst, np.ascontiguousarray(f32(a)).ctypes.data, f32(a).size * 4)
    put(c.kinv_ref, np.linalg.inv(K_ref))
    put(c.k_ref, K_ref)
    put(c.einv_ref, np.linalg.inv(E_ref))
    if len(srcs) > _capi.FUSION_MAX_SRC:
        raise ValueError("at most %d source views (the reference's masks run to i = 10)" % _capi.FUSION_MAX_SRC)
    for v, (K_src, E_src) in enumerate(srcs):
        K_src, E_src = f32(K_src), f32(E_src)
        put(c.t_sr[v], np.matmul(E_src, np.linalg.inv(E_ref)))
        put(c.k_src[v], K_src)
        put(c.kinv_src[v], np.linalg.inv(K_src))
        put(c.t_rs[v], np.matmul(E_ref, np.linalg.inv(E_src)))
    return c


METHODS = ("dypcd", "pcd")


def _fuse_view_raw(depth_ref, K_ref, E_ref, srcs, confs, conf_thr, dist_base, rel_diff_base, want_xyz, method,
                   thres_view, dist_thr, rel_thr):
    """fuse_view's launch -> (depth_avg, mask uint8 (bit 0 photo, bit 1 geometric, bit 2 final), xyz or None)."""
    if method not in METHODS:
        raise ValueError("fusion method %r not in %s" % (method, METHODS))
    for t in [depth_ref] + [s[0] for s in srcs] + list(confs or []):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == depth_ref.shape):
            raise ValueError("fusion maps must be contiguous (H, W) float32 CUDA tensors of one size")
    lib = _capi.load_library()
    H, W = depth_ref.shape
    dev = depth_ref.device
    cams = fusion_cams(K_ref, E_ref, [(K, E) for _, K, E in srcs])
    n = len(srcs)
    dsrc = (ctypes.c_void_p * n)(*[s[0].data_ptr() for s in srcs])
    cptr = (ctypes.c_void_p * 3)(*[c.data_ptr() for c in confs]) if confs is not None else None
    thr = (ctypes.c_float * 3)(*conf_thr)
    depth_avg = torch.empty(H, W, device=dev, dtype=torch.float32)
    mask = torch.empty(H, W, device=dev, dtype=torch.uint8)
    xyz = torch.empty(H, W, 3, device=dev, dtype=torch.float32) if want_xyz else None
    head = (_capi.stream_ptr(dev), H, W, n, depth_ref.data_ptr(), dsrc, cptr, thr, ctypes.byref(cams))
    outs = (depth_avg.data_ptr(), mask.data_ptr(), xyz.data_ptr() if xyz is not None else None)
    if method == "pcd":
        check(lib.damvs_fusion_view_static(*head, dist_thr, rel_thr, int(thres_view), *outs))
    else:
        check(lib.damvs_fusion_view(*head, dist_base, rel_diff_base, *outs))
    return depth_avg, mask, xyz


def fuse_view(depth_ref, K_ref, E_ref, srcs, confs=None, conf_thr=(0.1, 0.15, 0.9), dist_base=0.25,
              rel_diff_base=1 / 1300, want_xyz=True, method="dypcd", thres_view=5, dist_thr=1.0, rel_thr=0.01,
              want_normals=False, normal_jump=0.01):
    """One reference view. depth_ref (H, W) fp32 CUDA tensor; srcs [(depth (H, W) CUDA, K, E)];
    confs: (final, stage-2, stage-1) confidence maps at (H, W) or None.
    method "dypcd" reads dist_base / rel_diff_base, method "pcd" reads thres_view / dist_thr / rel_thr.
    -> {'depth_avg', 'photo', 'geo', 'final' (bool), 'xyz' (H, W, 3) world points (0 off-mask)}, and with want_normals
    'normal' (H, W, 3): the world normals of the final pixels at normal_jump (normal_map; 0 off-mask)."""
    if want_normals:
        check_normal_jump(normal_jump)
    depth_avg, mask, xyz = _fuse_view_raw(depth_ref, K_ref, E_ref, srcs, confs, conf_thr, dist_base, rel_diff_base,
                                          want_xyz, method, thres_view, dist_thr, rel_thr)
    r = {"depth_avg": depth_avg, "photo": (mask & 1).bool(), "geo": (mask & 2).bool(), "final": (mask & 4).bool(),
         "xyz": xyz}
    if want_normals:
        r["normal"] = normal_map(depth_avg, mask, K_ref, E_ref, normal_jump)
    return r


# ------------------------------------------------------------------------------------------------ point normals
def check_normal_jump(normal_jump):
    """normal_jump as a Python float; ValueError unless it is a finite number >= 0."""
    ok = isinstance(normal_jump, (int, float, np.integer, np.floating)) and not isinstance(normal_jump, (bool, np.bool_))
    if not (ok and np.isfinite(normal_jump) and normal_jump >= 0):
        raise ValueError("normal_jump must be a finite number >= 0 (got %r)" % (normal_jump,))
    return float(normal_jump)


def _neighbour(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx] where that pixel exists, else fill."""
    H, W = a.shape
    b = np.full_like(a, fill)
    b[max(0, -dy):H - max(0, dy), max(0, -dx):W - max(0, dx)] = a[max(0, dy):H - max(0, -dy), max(0, dx):W - max(0, -dx)]
    return b


def normals_statement(depth_avg, final, K, E, jump):
    """The normal rule in numpy, the specification of damvs_fusion_normals and damvs_fusion_cloud_oriented (k_normals.hip
    equals it bit for bit): depth_avg (H, W) float32 and final (H, W) bool as the fusion kernels write them for a
    reference view with intrinsics K and extrinsics E -> (H, W, 3) float32 world normals, (0, 0, 0) where final is unset.
    Kinv = float32(inv(K)) and Rinv = float32(inv(E))[:3, :3] as fusion_cams forms them; everything else is float64, one
    operation at a time, every sum written out left to right (nothing a library may fuse or reorder). For a final pixel c:
      P(q) = Kinv (x_q d_q, y_q d_q, d_q); a 4-neighbour q is usable when it is inside the image, final, and
      |d_q - d_c| <= jump * d_c (NaN compares false);
      tx = P(E) - P(W) with an unusable side replaced by P(c), missing when neither is usable; ty the same with south
      (y + 1) and north (y - 1);
      n = ty x tx, negated when n . P(c) > 0 so that it faces the camera, n_cam = n / sqrt(n . n);
      a missing tangent, or n . n zero or not finite: n_cam = -P(c) / sqrt(P(c) . P(c)), the direction to the camera;
      the result is float32(Rinv n_cam), not renormalised, and (0, 0, 0) when a component is not finite."""
    jump = check_normal_jump(jump)
    d = np.asarray(depth_avg, dtype=np.float32).astype(np.float64)
    fin = np.asarray(final).astype(bool)
    if d.ndim != 2 or fin.shape != d.shape:
        raise ValueError("depth_avg and final must be (H, W) maps of one size")
    H, W = d.shape
    Kinv = np.linalg.inv(np.asarray(K, dtype=np.float32)).astype(np.float32).astype(np.float64)
    Rinv = np.linalg.inv(np.asarray(E, dtype=np.float32)).astype(np.float32)[:3, :3].astype(np.float64)
    yi, xi = np.mgrid[0:H, 0:W]
    x, y = xi.astype(np.float64), yi.astype(np.float64)
    with np.errstate(all="ignore"):
        a0, a1 = x * d, y * d
        P = [Kinv[i, 0] * a0 + Kinv[i, 1] * a1 + Kinv[i, 2] * d for i in range(3)]
        lim = jump * d

        def side(dy, dx):
            use = _neighbour(fin, dy, dx, False) & (np.abs(_neighbour(d, dy, dx, np.nan) - d) <= lim)
            return use, [np.where(use, _neighbour(P[i], dy, dx, 0.0), P[i]) for i in range(3)]

        ue, pe = side(0, 1)
        uw, pw = side(0, -1)
        us, ps = side(1, 0)
        un, pn = side(-1, 0)
        tx = [pe[i] - pw[i] for i in range(3)]
        ty = [ps[i] - pn[i] for i in range(3)]
        n0 = ty[1] * tx[2] - ty[2] * tx[1]
        n1 = ty[2] * tx[0] - ty[0] * tx[2]
        n2 = ty[0] * tx[1] - ty[1] * tx[0]
        flip = n0 * P[0] + n1 * P[1] + n2 * P[2] > 0
        n0, n1, n2 = np.where(flip, -n0, n0), np.where(flip, -n1, n1), np.where(flip, -n2, n2)
        nn = n0 * n0 + n1 * n1 + n2 * n2
        good = (ue | uw) & (us | un) & np.isfinite(nn) & (nn > 0)
        ln = np.sqrt(nn)
        lp = np.sqrt(P[0] * P[0] + P[1] * P[1] + P[2] * P[2])
        c0 = np.where(good, n0 / ln, -P[0] / lp)
        c1 = np.where(good, n1 / ln, -P[1] / lp)
        c2 = np.where(good, n2 / ln, -P[2] / lp)
        out = np.stack([(Rinv[i, 0] * c0 + Rinv[i, 1] * c1 + Rinv[i, 2] * c2).astype(np.float32) for i in range(3)], -1)
    keep = fin & np.isfinite(out[..., 0]) & np.isfinite(out[..., 1]) & np.isfinite(out[..., 2])
    return np.where(keep[..., None], out, np.float32(0))


def _view_cams(K, E):
    return fusion_cams(K, E, [])


def normal_map(depth_avg, mask, K, E, normal_jump=0.01):
    """normals_statement on the device (damvs_fusion_normals, k_normals.hip), bit for bit: depth_avg (H, W) float32 and
    mask (H, W) uint8 as the fusion kernels write them (bit value 4 is `final`), CUDA tensors -> (H, W, 3) float32."""
    jump = check_normal_jump(normal_jump)
    dev = mask.device
    ok = lambda t, dt: t.is_cuda and t.device == dev and t.dtype == dt and t.is_contiguous() and t.dim() == 2
    if not (ok(mask, torch.uint8) and ok(depth_avg, torch.float32) and depth_avg.shape == mask.shape):
        raise ValueError("normal_map takes contiguous CUDA tensors of one device: depth_avg (H, W) float32, mask (H, W) "
                         "uint8")
    H, W = mask.shape
    cams = _view_cams(K, E)
    out = torch.empty(H, W, 3, device=dev, dtype=torch.float32)
    check(_capi.load_library().damvs_fusion_normals(_capi.stream_ptr(dev), H, W, depth_avg.data_ptr(), mask.data_ptr(),
                                                    ctypes.byref(cams), jump, out.data_ptr()))
    return out


RECORD_BYTES = mvsio.PLY_RECORD_BYTES
ORIENTED_RECORD_BYTES = mvsio.PLY_ORIENTED_RECORD_BYTES


def compact_cloud(mask, xyz, rgb, records, cursor, scratch=None, depth_avg=None, cam=None, fusion_mask=None,
                  normal_jump=0.01):
    """The coloured points of one fused view, appended in row-major pixel order to a record buffer on the device
    (damvs_fusion_cloud, k_cloud.hip). mask (H, W) uint8 as the fusion kernels write it (bit value 4 selects), xyz
    (H, W, 3) float32, rgb (H, W, 3) uint8; records: 1-D uint8 CUDA tensor of capacity len // 15 records (x, y, z
    float32, red, green, blue: mvsio.write_ply's element); cursor: 1-element int64 CUDA tensor, the number of records
    so far. Record i of the view goes to records[(cursor + i) * 15:] when cursor + i < capacity; cursor advances by
    the view's count either way (a cursor above the capacity tells how many were needed). Nothing is synchronised;
    calls that share a cursor must run on one stream. scratch: int32 CUDA tensor of at least
    damvs_fusion_cloud_scratch(H, W) elements to reuse, or None to allocate. -> the scratch tensor.
    The oriented form (damvs_fusion_cloud_oriented, k_normals.hip), when depth_avg is given: records of 27 bytes, x, y,
    z, nx, ny, nz float32 then red, green, blue (mvsio.write_ply's element with normals), capacity len // 27, the same
    order and cursor. depth_avg (H, W) float32: the fusion's averaged depth; cam: the view's (K, E); fusion_mask (H, W)
    uint8: the fusion's mask, by which the normal rule judges neighbours (None: `mask`; pass it when `mask` is a
    VoxelGrid.claim keep mask); normal_jump: the rule's relative depth step. The normal of each selected pixel is
    normals_statement's, computed in the scatter."""
    H, W = mask.shape if mask.dim() == 2 else (0, 0)
    dev = mask.device
    ok = lambda t, dt, shape: t.is_cuda and t.device == dev and t.dtype == dt and t.is_contiguous() and \
        (shape is None or tuple(t.shape) == shape)
    if not (ok(mask, torch.uint8, (H, W)) and ok(xyz, torch.float32, (H, W, 3)) and ok(rgb, torch.uint8, (H, W, 3))):
        raise ValueError("compact_cloud takes contiguous CUDA tensors of one device: mask (H, W) uint8, xyz (H, W, 3) "
                         "float32, rgb (H, W, 3) uint8")
    if not (ok(records, torch.uint8, None) and records.dim() == 1):
        raise ValueError("records must be a contiguous 1-D uint8 CUDA tensor")
    if not (ok(cursor, torch.int64, None) and cursor.numel() == 1):
        raise ValueError("cursor must be a 1-element int64 CUDA tensor")
    oriented = depth_avg is not None
    if oriented:
        jump = check_normal_jump(normal_jump)
        if cam is None:
            raise ValueError("the oriented form needs cam=(K, E) of the view")
        if fusion_mask is None:
            fusion_mask = mask
        if not (ok(depth_avg, torch.float32, (H, W)) and ok(fusion_mask, torch.uint8, (H, W))):
            raise ValueError("the oriented form takes contiguous CUDA tensors of mask's device: depth_avg (H, W) float32, "
                             "fusion_mask (H, W) uint8")
    elif cam is not None or fusion_mask is not None:
        raise ValueError("cam and fusion_mask belong to the oriented form: pass depth_avg too")
    lib = _capi.load_library()
    need = lib.damvs_fusion_cloud_scratch(H, W)
    if need < 0:
        check(need)
    if scratch is None:
        scratch = torch.empty(need, device=dev, dtype=torch.int32)
    elif not (ok(scratch, torch.int32, None) and scratch.numel() >= need):
        raise ValueError("scratch must be a contiguous int32 CUDA tensor of at least %d elements" % need)
    if oriented:
        capacity = records.numel() // ORIENTED_RECORD_BYTES
        cams = cam if isinstance(cam, _capi.DamvsFusionCams) else _view_cams(*cam)
        check(lib.damvs_fusion_cloud_oriented(_capi.stream_ptr(dev), H, W, mask.data_ptr(), fusion_mask.data_ptr(),
                                              depth_avg.data_ptr(), ctypes.byref(cams), jump, xyz.data_ptr(),
                                              rgb.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                              records.data_ptr() if capacity else None, capacity, cursor.data_ptr()))
        return scratch
    capacity = records.numel() // RECORD_BYTES
    check(lib.damvs_fusion_cloud(_capi.stream_ptr(dev), H, W, mask.data_ptr(), xyz.data_ptr(), rgb.data_ptr(),
                                 scratch.data_ptr(), scratch.numel(), records.data_ptr() if capacity else None, capacity,
                                 cursor.data_ptr()))
    return scratch


# ------------------------------------------------------------------------------------------------ voxel thinning
VOXEL_Q = 1 << 20  # cell indices lie in [-2^20, 2^20) per axis
_EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def _inv_voxel(voxel):
    """float32(1) / float32(voxel) as a Python float; ValueError unless voxel and the quotient are finite and > 0."""
    try:
        with np.errstate(all="ignore"):
            v = np.float32(voxel)
            inv = np.float32(1) / v
    except (TypeError, ValueError):
        raise ValueError("voxel must be a positive finite number (got %r)" % (voxel,)) from None
    if not (np.isfinite(v) and v > 0 and np.isfinite(inv) and inv > 0):
        raise ValueError("voxel must be a positive finite number whose float32 reciprocal is one too (got %r)" % (voxel,))
    return float(inv)


def _voxel_slots(voxel_slots, pixels=None):
    """The table's slot count: voxel_slots checked (a power of two in [64, 2^32]), or, for None, the power of two at or
    above twice `pixels`."""
    if voxel_slots is None:
        return max(64, 1 << (2 * int(pixels) - 1).bit_length())
    ok = isinstance(voxel_slots, (int, np.integer)) and not isinstance(voxel_slots, bool) and \
        64 <= voxel_slots <= 1 << 32 and voxel_slots & (voxel_slots - 1) == 0
    if not ok:
        raise ValueError("voxel_slots must be a power of two in [64, 2^32] (got %r)" % (voxel_slots,))
    return int(voxel_slots)


def check_voxel(voxel, voxel_slots):
    """The drivers' argument check, before anything is launched or written: ValueError for a voxel that is not a
    positive finite number, a voxel_slots that is not a power of two in [64, 2^32], or voxel_slots without voxel."""
    if voxel is None:
        if voxel_slots is not None:
            raise ValueError("voxel_slots=%r without voxel" % (voxel_slots,))
        return
    _inv_voxel(voxel)
    if voxel_slots is not None:
        _voxel_slots(voxel_slots)


def voxel_keys(xyz, voxel):
    """The thinning rule's cell keys on the CPU: xyz (n, 3) -> (keys uint64 (n,), in_range bool (n,)).
    inv = float32(1) / float32(voxel); q = floor(float32(x) * inv) per axis (one float32 multiply, floor, integer); a
    point is in range when every q lies in [-2^20, 2^20) (NaN and infinities do not); key = (qx + 2^20) |
    (qy + 2^20) << 21 | (qz + 2^20) << 42, all ones where out of range."""
    inv = np.float32(_inv_voxel(voxel))
    p = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        q = np.floor(p * inv)
        ok = ((q >= -VOXEL_Q) & (q < VOXEL_Q)).all(axis=1)
    u = (np.where(ok[:, None], q, 0).astype(np.int64) + VOXEL_Q).astype(np.uint64)
    keys = u[:, 0] | (u[:, 1] << np.uint64(21)) | (u[:, 2] << np.uint64(42))
    return np.where(ok, keys, _EMPTY), ok


def voxel_first(xyz, voxel):
    """The thinning rule in numpy: the indices, ascending, of the points of xyz (n, 3) that are the first, in order,
    of their cell of the grid of edge `voxel` (voxel_keys). ValueError when a point is not finite or out of range."""
    keys, ok = voxel_keys(xyz, voxel)
    if not ok.all():
        bad = int(np.flatnonzero(~ok)[0])
        raise ValueError("point %d %s is not finite or its cell index lies outside [-2^20, 2^20) at voxel %r (out of "
                         "range)" % (bad, np.asarray(xyz, dtype=np.float32).reshape(-1, 3)[bad].tolist(), voxel))
    _, first = np.unique(keys, return_index=True)
    return np.sort(first).astype(np.int64)


def voxel_home_slot(key, slots):
    """The slot a cell key's probe starts from in a table of `slots` slots (damvs_cloud_thin_hash, the device's
    function run on the host): for tests that place probe chains; the kept points never depend on it."""
    out = ctypes.c_longlong()
    check(_capi.load_library().damvs_cloud_thin_hash(int(key), int(slots), ctypes.byref(out)))
    return int(out.value)


class VoxelGrid:
    """One scene's voxel table on the device (damvs_cloud_thin, k_thin.hip): `slots` 64-bit keys and owners and a
    status word, `nbytes` = 16 * slots + 8 bytes. voxel: the cell's edge in world units; slots: a power of two in
    [64, 2^32], at least the number of occupied cells (twice that keeps the probe chains short).
    claim(mask, xyz, base) per reference view in PLY order, on one stream; check() once at the end."""

    def __init__(self, voxel, slots, device="cuda"):
        self.inv_voxel = _inv_voxel(voxel)
        self.slots = _voxel_slots(slots) if slots is not None else _voxel_slots(None, 32)
        self.voxel = float(voxel)
        self._lib = _capi.load_library()
        nbytes = ctypes.c_size_t()
        check(self._lib.damvs_cloud_thin_table_bytes(self.slots, ctypes.byref(nbytes)))
        self.nbytes = int(nbytes.value)
        self.table = torch.empty(self.nbytes // 8, device=device, dtype=torch.int64)
        self.clear()

    def clear(self):
        """Empty the table and the status (two memsets on the current stream)."""
        check(self._lib.damvs_cloud_thin_clear(_capi.stream_ptr(self.table.device), self.table.data_ptr(), self.slots))

    def claim(self, mask, xyz, base, keep=None):
        """One view: mask (H, W) or (n,) uint8 (bit value 4 selects), xyz (..., 3) float32 of the same pixels, base:
        the number of pixels of the views claimed before (pixel p's ordinal is base + p). -> keep, uint8 of mask's
        shape (given, or allocated): 4 where the pixel is the first of its cell so far, else 0: the mask compact_cloud
        takes. Two launches on the current stream, nothing synchronised; a later view never takes a cell from an
        earlier one."""
        dev = self.table.device
        ok = lambda t, dt: t.is_cuda and t.device == dev and t.dtype == dt and t.is_contiguous()
        if not (ok(mask, torch.uint8) and ok(xyz, torch.float32) and tuple(xyz.shape) == tuple(mask.shape) + (3,)
                and mask.numel() >= 1):
            raise ValueError("claim takes contiguous CUDA tensors of the table's device: mask (...) uint8, xyz (..., 3) "
                             "float32")
        if keep is None:
            keep = torch.empty_like(mask)
        elif not (ok(keep, torch.uint8) and keep.shape == mask.shape):
            raise ValueError("keep must be a contiguous uint8 CUDA tensor of mask's shape")
        check(self._lib.damvs_cloud_thin(_capi.stream_ptr(dev), mask.numel(), mask.data_ptr(), xyz.data_ptr(),
                                         self.inv_voxel, int(base), self.table.data_ptr(), self.slots, keep.data_ptr()))
        return keep

    def check(self):
        """Synchronises the current stream. ValueError with the library's message when, since the last check or clear,
        a selected point was out of range or the table was full; the status is clear afterwards."""
        rc = self._lib.damvs_cloud_thin_status(_capi.stream_ptr(self.table.device), self.table.data_ptr(), self.slots)
        if rc != 0:
            msg = self._lib.damvs_last_error_string().decode(errors="replace")
            if rc == -6:
                msg += ": raise voxel_slots"
            raise ValueError("%s (%d): %s" % (_capi.ERRORS.get(rc, "DAMVS_E_?"), rc, msg))

    def occupied(self):
        """Slots that hold a key (synchronises): the table's load factor is occupied() / slots."""
        return int((self.table[:self.slots] != -1).sum().item())


def _save_mask(path, m):
    from PIL import Image
    Image.fromarray(m.astype(np.uint8) * 255).save(path)


def filter_depth(pair_folder, scan_folder, out_folder, plyfilename, conf=(0.1, 0.15, 0.9), dist_base=0.25,
                 rel_diff_base=1 / 1300, device="cuda", method="dypcd", thres_view=5, normals=False, normal_jump=0.01):
    """filter/dypcd.py:179-326 (method "dypcd") or filter/pcd.py:116-233 (method "pcd", args.thres_view) for one
    scene: per reference view of pair.txt, load its cams, image, depth and three confidences (and the sources'
    depths), run the fusion kernel, save the photo / geo / final masks, collect coloured world points; write the
    PLY. Returns the point count. normals=True: the oriented PLY (mvsio.write_ply with normals), each point's normal
    from normal_map at normal_jump."""
    if method not in METHODS:
        raise ValueError("fusion method %r not in %s" % (method, METHODS))
    check_normal_jump(normal_jump)
    pairs = mvsio.read_pair_file(os.path.join(pair_folder, "pair.txt"))
    cam = lambda v: mvsio.read_camera_parameters(os.path.join(scan_folder, "cams", "%08d_cam.txt" % v))
    pfm = lambda kind, v, sfx="": torch.from_numpy(np.ascontiguousarray(
        mvsio.read_pfm(os.path.join(out_folder, kind, "%08d%s.pfm" % (v, sfx)))[0])).to(device)
    os.makedirs(os.path.join(out_folder, "mask"), exist_ok=True)
    verts, cols, nrms = [], [], []
    for ref_view, src_views in pairs:
        K_ref, E_ref = cam(ref_view)
        img = mvsio.read_img(os.path.join(scan_folder, "images", "%08d.jpg" % ref_view))
        confs = (pfm("confidence", ref_view), pfm("confidence", ref_view, "_stage2"),
                 pfm("confidence", ref_view, "_stage1"))
        srcs = [(pfm("depth_est", v),) + cam(v) for v in src_views]
        r = fuse_view(pfm("depth_est", ref_view), K_ref, E_ref, srcs, confs, conf, dist_base, rel_diff_base,
                      method=method, thres_view=thres_view, want_normals=bool(normals), normal_jump=normal_jump)
        fin = r["final"].cpu().numpy()
        for kind in ("photo", "geo", "final"):
            _save_mask(os.path.join(out_folder, "mask", "%08d_%s.png" % (ref_view, kind)), r[kind].cpu().numpy())
        verts.append(r["xyz"][r["final"]].cpu().numpy())
        cols.append((img[fin] * 255).astype(np.uint8))
        if normals:
            nrms.append(r["normal"][r["final"]].cpu().numpy())
    xyz = np.concatenate(verts) if verts else np.zeros((0, 3), np.float32)
    rgb = np.concatenate(cols) if cols else np.zeros((0, 3), np.uint8)
    if normals:
        mvsio.write_ply(plyfilename, xyz, rgb, np.concatenate(nrms) if nrms else np.zeros((0, 3), np.float32))
    else:
        mvsio.write_ply(plyfilename, xyz, rgb)
    return len(xyz)


def fuse_scene(pair_folder, scan_folder, out_folder, plyfilename, conf=(0.1, 0.15, 0.9), dist_base=0.25,
               rel_diff_base=1 / 1300, device="cuda", method="dypcd", thres_view=5, save_masks=True, max_points=None,
               voxel=None, voxel_slots=None, normals=False, normal_jump=0.01):
    """filter_depth's files in, filter_depth's files out, with the scene kept on the device: every view's depth map,
    camera and (for reference views) three confidences and image are read and uploaded once; each reference view
    runs the fusion kernel and compact_cloud appends its coloured points to one record buffer behind one device
    cursor, with no host synchronisation between views; the masks come back only for the PNGs (save_masks) and the
    cloud in one copy of count * 15 bytes, written by mvsio.write_ply_records.
    The buffer holds the sum of H * W over the reference views (an exact upper bound) or max_points if that is less;
    a scene that needs more raises ValueError with the count needed and writes no PLY. Returns the point count.
    voxel, voxel_slots: thin the cloud to one point per cell (fuse_resident's docstring).
    normals, normal_jump: write the oriented PLY, 27 bytes a point (fuse_resident's docstring)."""
    from PIL import Image
    if method not in METHODS:
        raise ValueError("fusion method %r not in %s" % (method, METHODS))
    check_voxel(voxel, voxel_slots)
    check_normal_jump(normal_jump)
    pairs = mvsio.read_pair_file(os.path.join(pair_folder, "pair.txt"))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    pfm = lambda kind, v, sfx="": up(mvsio.read_pfm(os.path.join(out_folder, kind, "%08d%s.pfm" % (v, sfx)))[0])
    cams, depths, confs, rgbs = {}, {}, {}, {}
    for ref_view, src_views in pairs:
        for v in [ref_view] + src_views:
            if v not in depths:
                cams[v] = mvsio.read_camera_parameters(os.path.join(scan_folder, "cams", "%08d_cam.txt" % v))
                depths[v] = pfm("depth_est", v)
        if ref_view not in confs:
            confs[ref_view] = (pfm("confidence", ref_view), pfm("confidence", ref_view, "_stage2"),
                               pfm("confidence", ref_view, "_stage1"))
            img = np.array(Image.open(os.path.join(scan_folder, "images", "%08d.jpg" % ref_view)))
            if img.dtype != np.uint8 or img.shape != tuple(depths[ref_view].shape) + (3,):
                raise ValueError("image of view %d: %s %s, expected uint8 %s" % (
                    ref_view, img.dtype, img.shape, tuple(depths[ref_view].shape) + (3,)))
            rgbs[ref_view] = up(img)
    return fuse_resident(pairs, cams, depths, confs, rgbs, plyfilename, conf, dist_base, rel_diff_base, method,
                         thres_view, os.path.join(out_folder, "mask") if save_masks else None, max_points, device,
                         voxel, voxel_slots, normals, normal_jump)


def fuse_resident(pairs, cams, depths, confs, rgbs, plyfilename, conf=(0.1, 0.15, 0.9), dist_base=0.25,
                  rel_diff_base=1 / 1300, method="dypcd", thres_view=5, mask_dir=None, max_points=None, device="cuda",
                  voxel=None, voxel_slots=None, normals=False, normal_jump=0.01):
    """The per-pair loop of fuse_scene and scene.SceneMaps.fuse over maps already on the device: dicts by view id of
    cams (K, E) host arrays, depths (H, W) float32, and for the reference views confs (final, stage 2, stage 1) and rgbs
    (H, W, 3) uint8. Per pair the fusion kernel and compact_cloud on one cursor, no host synchronisation between views;
    then the mask PNGs (mask_dir, None: not written), one copy of count * 15 bytes and mvsio.write_ply_records.
    Raises ValueError, writing no PLY, when the cloud does not fit max_points. Returns the point count.
    voxel: None, or the edge in world units of an axis-aligned grid: the PLY then holds at most one point per cell, the
    first one in PLY order (reference views in pair order, pixels row-major) with its record unchanged, so it is a
    subsequence of the voxel=None PLY (voxel_first over that PLY's points gives the indices). Between the fusion kernel
    and compact_cloud a VoxelGrid.claim (two launches) turns the view's mask into the mask of the pixels that are the
    first of their cell; still no host synchronisation between views. The mask PNGs remain the fusion's masks and
    max_points bounds the thinned count. voxel_slots: the table's slots, a power of two in [64, 2^32]; None: the power of
    two at or above twice the sum of H * W over the reference views, which cannot fill. The table takes 16 bytes per
    slot: 2^28 slots, 4.3 GB, for 49 views at 1184 x 1600 (93 M pixels) on a 288 GB device; a scene whose occupied cells
    are known to be fewer can pass less. A table that fills, or a kept point that is not finite or whose cell index
    leaves [-2^20, 2^20), raises ValueError and writes no PLY. A bad voxel (not a positive finite number) or voxel_slots
    raises ValueError before anything is launched.
    normals=True: the oriented PLY, x y z nx ny nz red green blue at 27 bytes a point (mvsio.write_ply_records with
    normals). Positions, colours, order and count are those of normals=False; each point's normal is normals_statement's
    for its pixel, from the view's averaged depth, the fusion's final mask (never the thinned one, so with voxel the
    oriented PLY is still a subsequence of the unthinned oriented PLY) and normal_jump, the relative depth step above
    which a neighbour is not differenced (0.01: the static filter's relative-depth threshold). It faces the view's camera
    and is computed inside compact_cloud's scatter: no normal map is stored. A normal_jump that is not a finite number
    >= 0 raises ValueError before anything is launched."""
    if method not in METHODS:
        raise ValueError("fusion method %r not in %s" % (method, METHODS))
    check_voxel(voxel, voxel_slots)
    jump = check_normal_jump(normal_jump)
    rec_bytes = ORIENTED_RECORD_BYTES if normals else RECORD_BYTES
    save_masks = mask_dir is not None
    capacity = sum(depths[r].numel() for r, _ in pairs)
    grid = None if voxel is None else VoxelGrid(voxel, _voxel_slots(voxel_slots, max(capacity, 1)), device)
    base, keeps = 0, {}
    if max_points is not None:
        capacity = max(0, min(capacity, int(max_points)))
    records = torch.empty(capacity * rec_bytes, device=device, dtype=torch.uint8)
    cursor = torch.zeros(1, device=device, dtype=torch.int64)
    scratch, masks = {}, []
    for ref_view, src_views in pairs:
        K_ref, E_ref = cams[ref_view]
        srcs = [(depths[v],) + cams[v] for v in src_views]
        depth_avg, mask, xyz = _fuse_view_raw(depths[ref_view], K_ref, E_ref, srcs, confs[ref_view], conf, dist_base,
                                              rel_diff_base, True, method, thres_view, 1.0, 0.01)
        shape = tuple(mask.shape)
        chosen = mask
        if grid is not None:
            chosen = keeps[shape] = grid.claim(mask, xyz, base, keeps.get(shape))
            base += mask.numel()
        if normals:
            scratch[shape] = compact_cloud(chosen, xyz, rgbs[ref_view], records, cursor, scratch.get(shape),
                                           depth_avg=depth_avg, cam=(K_ref, E_ref), fusion_mask=mask, normal_jump=jump)
        else:
            scratch[shape] = compact_cloud(chosen, xyz, rgbs[ref_view], records, cursor, scratch.get(shape))
        if save_masks:
            masks.append((ref_view, mask))
    if save_masks:
        os.makedirs(mask_dir, exist_ok=True)
        for ref_view, mask in masks:
            m = mask.cpu().numpy()
            for bit, kind in ((1, "photo"), (2, "geo"), (4, "final")):
                _save_mask(os.path.join(mask_dir, "%08d_%s.png" % (ref_view, kind)), (m & bit) != 0)
    if grid is not None:
        grid.check()
    count = int(cursor.item())
    if count > capacity:
        raise ValueError("the scene's point cloud needs %d points, the record buffer holds %d" % (count, capacity))
    mvsio.write_ply_records(plyfilename, records[:count * rec_bytes].cpu().numpy(), normals=bool(normals))
    return count


# ------------------------------------------------------------------------------------------------ consensus fusion
CONSENSUS_MAX_VIEWS = _capi.CONSENSUS_MAX_VIEWS
CONSENSUS_SOURCES = ("all", "pairs")
CONSENSUS_MASKS = ((1, "valid"), (2, "geo"), (4, "final"), (8, "consumed"))


def check_consensus(prob_threshold=0.1, disp_threshold=0.15, num_consistent=3):
    """The consensus rule's parameters -> (prob_threshold rounded to float32, disp_threshold, num_consistent) as Python
    numbers; ValueError unless the thresholds are finite numbers and num_consistent is an integer >= 1."""
    num = lambda v: isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))
    with np.errstate(over="ignore"):
        finite32 = num(prob_threshold) and bool(np.isfinite(np.float32(prob_threshold)))
    if not (finite32 and np.isfinite(prob_threshold)):
        raise ValueError("prob_threshold must be a finite number (got %r)" % (prob_threshold,))
    if not (num(disp_threshold) and np.isfinite(disp_threshold)):
        raise ValueError("disp_threshold must be a finite number (got %r)" % (disp_threshold,))
    if not (isinstance(num_consistent, (int, np.integer)) and not isinstance(num_consistent, (bool, np.bool_))
            and num_consistent >= 1):
        raise ValueError("num_consistent must be an integer >= 1 (got %r)" % (num_consistent,))
    return float(np.float32(prob_threshold)), float(disp_threshold), int(num_consistent)


def consensus_order(pairs, sources="all"):
    """The processing order of a scene: pairs [(ref view, [source views])] -> [(ref, [sources])], reference views in
    pair order. sources="all" (fusibile's form): every other view that the pair list names, as a reference or as a
    source, in ascending id; "pairs": the pair's own sources with repeats dropped, the first occurrence kept.
    ValueError: an unknown `sources`, a reference view listed twice or among its own sources, a view without any source,
    more than CONSENSUS_MAX_VIEWS views."""
    if sources not in CONSENSUS_SOURCES:
        raise ValueError("sources must be one of %s (got %r)" % (CONSENSUS_SOURCES, sources))
    pairs = [(int(r), [int(s) for s in src]) for r, src in pairs]
    refs = [r for r, _ in pairs]
    for r in refs:
        if refs.count(r) > 1:
            raise ValueError("reference view %d is listed twice" % r)
    views = sorted({v for r, src in pairs for v in [r] + src})
    if len(views) > CONSENSUS_MAX_VIEWS:
        raise ValueError("%d views: consensus fusion takes at most %d" % (len(views), CONSENSUS_MAX_VIEWS))
    order = []
    for r, src in pairs:
        if sources == "all":
            src = [v for v in views if v != r]
        else:
            if r in src:
                raise ValueError("reference view %d is among its own sources" % r)
            src = list(dict.fromkeys(src))
        if not src:
            raise ValueError("reference view %d has no source view" % r)
        order.append((r, src))
    return order


def consensus_cam(K, E):
    """(K, inv(K), E, inv(E)) as float32: the inverses are np.linalg.inv on float32, as fusion_cams forms them."""
    K, E = np.asarray(K, dtype=np.float32), np.asarray(E, dtype=np.float32)
    if K.shape != (3, 3) or E.shape != (4, 4):
        raise ValueError("a camera is K (3, 3) and E (4, 4), got %s and %s" % (K.shape, E.shape))
    return K, np.linalg.inv(K).astype(np.float32), E, np.linalg.inv(E).astype(np.float32)


def consensus_fb(cam_ref, cam_src):
    """Focal length times baseline of a (reference, source) pair, a Python float: f = K_ref[0, 0]; the camera centres
    are the translation columns of the float32 inverses, inv(E)[:3, 3]; their distance is formed in float64,
    sqrt(dx * dx + dy * dy + dz * dz). cam_ref, cam_src: consensus_cam's tuples."""
    cr, cs = cam_ref[3][:3, 3].astype(np.float64), cam_src[3][:3, 3].astype(np.float64)
    dx, dy, dz = cr[0] - cs[0], cr[1] - cs[1], cr[2] - cs[2]
    return float(np.float64(cam_ref[0][0, 0]) * np.sqrt(dx * dx + dy * dy + dz * dz))


def _by_view(maps):
    return dict(maps) if isinstance(maps, dict) else dict(enumerate(maps))


def consensus_statement(depths, confs, rgbs, cams, order, prob_threshold=0.1, disp_threshold=0.15, num_consistent=3,
                        used=None, tally=None):
    """The consensus fusion rule in numpy, the specification of damvs_consensus_view (k_consensus.hip equals it bit for
    bit). It is this project's statement of the published fusibile algorithm with the thresholds the reference passes
    to that binary (test_uni.py:114-116, gipuma.py:170-187); parity with the binary itself is unverified.
    depths, confs (the final-stage confidence), rgbs, cams: per view id (dicts, or sequences indexed by view), maps of
    one size H x W: float32, float32, uint8 (H, W, 3), (K (3, 3), E (4, 4)). order: [(ref, [sources])], the processing
    order (consensus_order). used: per view (H, W) uint8 state to start from (None: all zero); it is not modified.
    tally: a dict that receives, summed over the processed (pixel, source) pairs, how many ended as 'behind'
    (q[2] <= 0), 'outside' the image, 'invalid' source sample, 'far' (disparity test failed) or 'agree', and of those
    that reached the rounding how many rounded x 'up' (fraction >= 0.5) and 'down'.
    -> one dict per entry of `order`: 'ref', 'mask' (H, W) uint8 (1 valid | 2 geo | 4 emitted | 8 consumed on entry),
    'xyz' (H, W, 3) float32 and 'rgb' (H, W, 3) uint8 (0 where nothing is emitted), 'count' (H, W) the number n of
    agreeing sources, and 'used': a copy of every view's state after the step.
    A sample (v, x, y) is valid when depth is finite, depth > 0 and not (conf < float32(prob_threshold)): the
    reference's depth_map[prob_map < prob_threshold] = 0, under which a NaN confidence stays.
    Per reference view, per pixel (x, y) whose sample is valid and whose used[ref][y, x] is 0, d its depth:
      X = Einv_ref (Kinv_ref (x d, y d, d));
      for each source s in list order: q = E_s X, skipped unless q[2] > 0; u = K_s q, px = floor(u[0] / u[2] + 0.5), py
      likewise, skipped unless both are finite and inside the image; skipped unless the sample (s, px, py) is valid, ds
      its depth; skipped unless |fb / q[2] - fb / ds| < disp_threshold, fb = consensus_fb (focal length times baseline);
      otherwise X_s = Einv_s (Kinv_s (px ds, py ds, ds)) is added to the position sum, rgb[s][py, px] to three integer
      channel sums, used[s][py, px] is set to 1 (here, before the count is known, as fusibile does) and n counts it;
      when n >= num_consistent the pixel emits (X + X_s1 + X_s2 + ...) / (n + 1), summed in list order, divided in
      float64 and cast to float32, and per channel (2 (c_ref + sum c_s) + (n + 1)) // (2 (n + 1)).
    fusibile compares the reference pixel's own depth with ds; the disparity test here compares the depth of X in the
    source camera, q[2], with ds, which is the same for fronto-parallel rectified cameras and also right for rotated
    ones.
    Arithmetic: the fusion kernels' convention. Matrices are float32 (inverses by np.linalg.inv on float32) widened to
    float64, every product and sum one float64 operation, the sums written out term by term in mv3 / mv34 order
    (fusion_device.h): nothing a library may fuse or reorder.
    Why the result does not depend on the order of the pixels: a view's pass sets bytes of other views' `used` to 1 and
    reads `used` of its own view only, which earlier views wrote and its own pass never does (a reference view is not
    among its sources); two pixels that agree with the same source sample both count it. The views run in list order."""
    thr, disp, num = check_consensus(prob_threshold, disp_threshold, num_consistent)
    thr = np.float32(thr)
    depths, confs, rgbs, cams = _by_view(depths), _by_view(confs), _by_view(rgbs), _by_view(cams)
    order = [(int(r), [int(s) for s in src]) for r, src in order]
    views = sorted({v for r, src in order for v in [r] + src})
    for r, src in order:
        if r in src or len(set(src)) != len(src) or not src:
            raise ValueError("view %d: the sources %s must be distinct, non-empty and without the reference view" % (r, src))
    D = {v: np.asarray(depths[v], dtype=np.float32) for v in views}
    C = {v: np.asarray(confs[v], dtype=np.float32) for v in views}
    RGB = {v: np.asarray(rgbs[v], dtype=np.uint8) for v in views}
    H, W = D[views[0]].shape
    for v in views:
        if D[v].shape != (H, W) or C[v].shape != (H, W) or RGB[v].shape != (H, W, 3):
            raise ValueError("view %d: the maps of a scene must be of one size" % v)
    cam = {v: consensus_cam(*cams[v]) for v in views}
    m64 = {v: [m.astype(np.float64) for m in cam[v]] for v in views}
    state = {v: (np.zeros((H, W), np.uint8) if used is None else np.array(_by_view(used)[v], dtype=np.uint8))
             for v in views}
    with np.errstate(all="ignore"):
        valid = {v: np.isfinite(D[v]) & (D[v] > 0) & ~(C[v] < thr) for v in views}
    yi, xi = np.mgrid[0:H, 0:W]

    def world(v, x, y, d):
        _, Kinv, _, Einv = m64[v]
        a0, a1 = x * d, y * d
        c = [Kinv[i, 0] * a0 + Kinv[i, 1] * a1 + Kinv[i, 2] * d for i in range(3)]
        return [Einv[i, 0] * c[0] + Einv[i, 1] * c[1] + Einv[i, 2] * c[2] + Einv[i, 3] for i in range(3)]

    steps = []
    for ref, srcs in order:
        consumed = state[ref] != 0
        act = valid[ref] & ~consumed
        with np.errstate(all="ignore"):
            X = world(ref, xi.astype(np.float64), yi.astype(np.float64), D[ref].astype(np.float64))
            S = [X[0].copy(), X[1].copy(), X[2].copy()]
            csum = RGB[ref].astype(np.int64)
            n = np.zeros((H, W), np.int64)
            for s in srcs:
                K, _, E, _ = m64[s]
                q = [E[i, 0] * X[0] + E[i, 1] * X[1] + E[i, 2] * X[2] + E[i, 3] for i in range(3)]
                ok = act & (q[2] > 0)
                ends = [("behind", int((act & ~ok).sum()))]
                u = [K[i, 0] * q[0] + K[i, 1] * q[1] + K[i, 2] * q[2] for i in range(3)]
                fx, fy = np.floor(u[0] / u[2] + 0.5), np.floor(u[1] / u[2] + 0.5)
                frac = u[0] / u[2] - np.floor(u[0] / u[2])
                ends += [("up", int((ok & (frac >= 0.5)).sum())), ("down", int((ok & (frac < 0.5)).sum())),
                         ("outside", int(ok.sum()))]
                ok &= (fx >= 0) & (fx < W) & (fy >= 0) & (fy < H)
                ends += [("outside", -int(ok.sum())), ("invalid", int(ok.sum()))]
                px, py = np.where(ok, fx, 0).astype(np.int64), np.where(ok, fy, 0).astype(np.int64)
                ok &= valid[s][py, px]
                ends += [("invalid", -int(ok.sum())), ("far", int(ok.sum()))]
                ds = D[s][py, px].astype(np.float64)
                fb = consensus_fb(cam[ref], cam[s])
                ok &= np.abs(fb / q[2] - fb / ds) < disp
                ends += [("far", -int(ok.sum())), ("agree", int(ok.sum()))]
                if tally is not None:
                    for name, k in ends:
                        tally[name] = tally.get(name, 0) + k
                Xs = world(s, px.astype(np.float64), py.astype(np.float64), ds)
                S = [np.where(ok, S[i] + Xs[i], S[i]) for i in range(3)]
                csum = csum + np.where(ok[..., None], RGB[s][py, px].astype(np.int64), 0)
                state[s][py[ok], px[ok]] = 1
                n = n + ok
            geo = act & (n >= num)
            k = n + 1
            xyz = np.stack([np.where(geo, (S[i] / k.astype(np.float64)).astype(np.float32), np.float32(0))
                            for i in range(3)], -1).astype(np.float32)
            rgb = np.where(geo[..., None], (2 * csum + k[..., None]) // (2 * k[..., None]), 0).astype(np.uint8)
        mask = (valid[ref] * 1 + geo * 6 + consumed * 8).astype(np.uint8)
        steps.append({"ref": ref, "mask": mask, "xyz": xyz, "rgb": rgb, "count": np.where(act, n, 0),
                      "used": {v: state[v].copy() for v in views}})
    return steps


class ConsensusTable:
    """One scene's table on the device (damvs_consensus_table): per view its cameras and the pointers of its depth,
    confidence, colour and `used` maps, uploaded once. views: the view ids, slot i holding views[i]; cams: view ->
    (K, E) host arrays; depths, confs (a tensor, or fuse_resident's tuple whose first element is the final-stage
    confidence), rgbs: view -> CUDA tensors (H, W) float32, (H, W) float32, (H, W, 3) uint8 of one size and device.
    `used` (V, H, W) uint8 starts at zero. ValueError, before anything is launched: no view or more than
    CONSENSUS_MAX_VIEWS, a view listed twice, a view missing its cams, depth, conf or colour, maps of different sizes,
    tensors that are not contiguous CUDA tensors of one device."""

    def __init__(self, views, cams, depths, confs, rgbs):
        views = [int(v) for v in views]
        if not 1 <= len(views) <= CONSENSUS_MAX_VIEWS:
            raise ValueError("%d views: consensus fusion takes 1 to %d" % (len(views), CONSENSUS_MAX_VIEWS))
        if len(set(views)) != len(views):
            raise ValueError("a view is listed twice in %s" % views)
        for name, maps in (("cams", cams), ("depth", depths), ("conf", confs), ("colour", rgbs)):
            for v in views:
                if v not in maps or maps[v] is None:
                    raise ValueError("view %d is missing its %s" % (v, name))
        final = lambda c: c[0] if isinstance(c, (tuple, list)) else c
        self.views, self.slot = views, {v: i for i, v in enumerate(views)}
        self.cams = {v: consensus_cam(*cams[v]) for v in views}
        self.depth = [depths[v] for v in views]
        self.conf = [final(confs[v]) for v in views]
        self.rgb = [rgbs[v] for v in views]
        shape = tuple(self.depth[0].shape)
        for v, d, c, r in zip(views, self.depth, self.conf, self.rgb):
            if len(shape) != 2 or tuple(d.shape) != shape or tuple(c.shape) != shape or tuple(r.shape) != shape + (3,):
                raise ValueError("view %d: depth %s, conf %s, colour %s; the maps of a scene must be of one size %s" % (
                    v, tuple(d.shape), tuple(c.shape), tuple(r.shape), shape))
        dev = self.depth[0].device
        ok = lambda t, dt: torch.is_tensor(t) and t.is_cuda and t.device == dev and t.dtype == dt and t.is_contiguous()
        for v, d, c, r in zip(views, self.depth, self.conf, self.rgb):
            if not (ok(d, torch.float32) and ok(c, torch.float32) and ok(r, torch.uint8)):
                raise ValueError("view %d: consensus fusion takes contiguous CUDA tensors of one device: depth and conf "
                                 "float32, colour uint8" % v)
        self.H, self.W = shape
        self.device = dev
        V = len(views)
        lib = _capi.load_library()
        nbytes = ctypes.c_size_t()
        check(lib.damvs_consensus_table_bytes(V, ctypes.byref(nbytes)))
        self.used = torch.zeros(V, self.H, self.W, device=dev, dtype=torch.uint8)
        self.table = torch.empty(int(nbytes.value) // 8, device=dev, dtype=torch.int64)
        cam_arr = (_capi.DamvsConsensusCam * V)()
        for i, v in enumerate(views):
            for name, m in zip(("k", "kinv", "e", "einv"), self.cams[v]):
                m = np.ascontiguousarray(m, dtype=np.float32)
                ctypes.memmove(getattr(cam_arr[i], name), m.ctypes.data, m.size * 4)
        ptrs = lambda ts: (ctypes.c_void_p * V)(*[t.data_ptr() for t in ts])
        check(lib.damvs_consensus_table(_capi.stream_ptr(dev), self.H, self.W, V, cam_arr, ptrs(self.depth),
                                        ptrs(self.conf), ptrs(self.rgb), ptrs(list(self.used)),
                                        self.table.data_ptr()))

    def used_of(self, view):
        """The (H, W) uint8 `used` map of a view (a slice of the table's state)."""
        return self.used[self.slot[int(view)]]


def consensus_view(table, ref, srcs, prob_threshold=0.1, disp_threshold=0.15, num_consistent=3, out=None):
    """One reference view of consensus_statement on the device (damvs_consensus_view, k_consensus.hip), bit for bit:
    table: the scene's ConsensusTable; ref, srcs: view ids, 1 to 63 distinct sources without the reference view.
    -> (mask (H, W) uint8, xyz (H, W, 3) float32, rgb_avg (H, W, 3) uint8), the shapes compact_cloud takes (out: such a
    triple to write into). One launch on the current stream, nothing synchronised: it marks `table.used` of the sources
    and reads that of the reference view, so the views of a scene must be enqueued in order on one stream."""
    thr, disp, num = check_consensus(prob_threshold, disp_threshold, num_consistent)
    ref, srcs = int(ref), [int(s) for s in srcs]
    for v in [ref] + srcs:
        if v not in table.slot:
            raise ValueError("view %d is not one of the table's views %s" % (v, table.views))
    if ref in srcs or len(set(srcs)) != len(srcs) or not 1 <= len(srcs) <= CONSENSUS_MAX_VIEWS - 1:
        raise ValueError("view %d: 1 to %d distinct sources without the reference view (got %s)" % (
            ref, CONSENSUS_MAX_VIEWS - 1, srcs))
    H, W, dev, n = table.H, table.W, table.device, len(srcs)
    if out is None:
        out = (torch.empty(H, W, device=dev, dtype=torch.uint8), torch.empty(H, W, 3, device=dev, dtype=torch.float32),
               torch.empty(H, W, 3, device=dev, dtype=torch.uint8))
    mask, xyz, rgb_avg = out
    ok = lambda t, dt, shape: t.is_cuda and t.device == dev and t.dtype == dt and t.is_contiguous() and \
        tuple(t.shape) == shape
    if not (ok(mask, torch.uint8, (H, W)) and ok(xyz, torch.float32, (H, W, 3)) and ok(rgb_avg, torch.uint8, (H, W, 3))):
        raise ValueError("out must be contiguous CUDA tensors of the table's device: mask (H, W) uint8, xyz (H, W, 3) "
                         "float32, rgb_avg (H, W, 3) uint8")
    src = (ctypes.c_int * n)(*[table.slot[s] for s in srcs])
    fb = (ctypes.c_double * n)(*[consensus_fb(table.cams[ref], table.cams[s]) for s in srcs])
    check(_capi.load_library().damvs_consensus_view(_capi.stream_ptr(dev), H, W, len(table.views), table.table.data_ptr(),
                                                    table.slot[ref], n, src, fb, thr, disp, num, mask.data_ptr(),
                                                    xyz.data_ptr(), rgb_avg.data_ptr()))
    return mask, xyz, rgb_avg


def _check_consensus_driver(prob_threshold, disp_threshold, num_consistent, sources, voxel, voxel_slots, normal_jump):
    """The consensus drivers' argument check, before anything is read, launched or written."""
    check_consensus(prob_threshold, disp_threshold, num_consistent)
    if sources not in CONSENSUS_SOURCES:
        raise ValueError("sources must be one of %s (got %r)" % (CONSENSUS_SOURCES, sources))
    check_voxel(voxel, voxel_slots)
    check_normal_jump(normal_jump)


def fuse_consensus_resident(pairs, cams, depths, confs, rgbs, plyfilename, prob_threshold=0.1, disp_threshold=0.15,
                            num_consistent=3, sources="all", mask_dir=None, max_points=None, device="cuda", voxel=None,
                            voxel_slots=None, normals=False, normal_jump=0.01):
    """Consensus fusion of a scene whose maps are on the device (consensus_statement is the rule, its docstring states
    the differences from fusibile; parity with that binary is unverified): a surface seen by several views is written
    once, at the average of the agreeing views' points and colours, and the samples merged into a point are not
    emitted again from their own views. pairs: [(ref view, [source views])]; dicts by view id of cams (K, E) host arrays,
    depths (H, W) float32, confs (the final-stage confidence, or fuse_resident's tuple starting with it) and rgbs
    (H, W, 3) uint8, for every view used, sources too. sources="all", fusibile's form: every other view the pair list
    names, ascending, reference views in pair order; "pairs": the pair's own sources, repeats dropped
    (consensus_order). prob_threshold, disp_threshold, num_consistent: test_uni.py's defaults for the binary.
    One table upload, then per reference view consensus_view and compact_cloud on one cursor, no host synchronisation
    between views; then the valid / geo / final / consumed PNGs (mask_dir, None: not written), one copy of the records and
    mvsio.write_ply_records. voxel, voxel_slots, max_points, normals, normal_jump: as fuse_resident; the oriented form
    takes the view's own depth map and the consensus mask. Returns the point count.
    ValueError before anything is launched, and no PLY: a reference view listed twice, more than 64 views, a view
    missing its conf or colour, bad thresholds, maps of different sizes; a cloud that does not fit max_points raises
    after the launches and writes no PLY either."""
    _check_consensus_driver(prob_threshold, disp_threshold, num_consistent, sources, voxel, voxel_slots, normal_jump)
    jump = float(normal_jump)
    order = consensus_order(pairs, sources)
    views = sorted({v for r, src in order for v in [r] + src})
    table = ConsensusTable(views, cams, depths, confs, rgbs)
    rec_bytes = ORIENTED_RECORD_BYTES if normals else RECORD_BYTES
    save_masks = mask_dir is not None
    capacity = table.H * table.W * len(order)
    grid = None if voxel is None else VoxelGrid(voxel, _voxel_slots(voxel_slots, max(capacity, 1)), table.device)
    base, keep = 0, None
    if max_points is not None:
        capacity = max(0, min(capacity, int(max_points)))
    records = torch.empty(capacity * rec_bytes, device=table.device, dtype=torch.uint8)
    cursor = torch.zeros(1, device=table.device, dtype=torch.int64)
    scratch, masks = None, []
    for ref, srcs in order:
        mask, xyz, rgb_avg = consensus_view(table, ref, srcs, prob_threshold, disp_threshold, num_consistent)
        chosen = mask
        if grid is not None:
            chosen = keep = grid.claim(mask, xyz, base, keep)
            base += mask.numel()
        if normals:
            scratch = compact_cloud(chosen, xyz, rgb_avg, records, cursor, scratch, depth_avg=depths[ref],
                                    cam=cams[ref], fusion_mask=mask, normal_jump=jump)
        else:
            scratch = compact_cloud(chosen, xyz, rgb_avg, records, cursor, scratch)
        if save_masks:
            masks.append((ref, mask))
    if save_masks:
        os.makedirs(mask_dir, exist_ok=True)
        for ref, mask in masks:
            m = mask.cpu().numpy()
            for bit, kind in CONSENSUS_MASKS:
                _save_mask(os.path.join(mask_dir, "%08d_%s.png" % (ref, kind)), (m & bit) != 0)
    if grid is not None:
        grid.check()
    count = int(cursor.item())
    if count > capacity:
        raise ValueError("the scene's point cloud needs %d points, the record buffer holds %d" % (count, capacity))
    mvsio.write_ply_records(plyfilename, records[:count * rec_bytes].cpu().numpy(), normals=bool(normals))
    return count


def fuse_consensus_scene(pair_folder, scan_folder, out_folder, plyfilename, prob_threshold=0.1, disp_threshold=0.15,
                         num_consistent=3, sources="all", device="cuda", save_masks=True, max_points=None, voxel=None,
                         voxel_slots=None, normals=False, normal_jump=0.01):
    """fuse_scene's files in, the same kinds of files out, fused by consensus (fuse_consensus_resident): pair.txt, and for
    every view used, sources too, cams/%08d_cam.txt, depth_est/%08d.pfm, confidence/%08d.pfm (the final stage) and
    images/%08d.jpg, each read and uploaded once; <out_folder>/mask/%08d_{valid,geo,final,consumed}.png (save_masks)
    and the PLY. Returns the point count."""
    from PIL import Image
    _check_consensus_driver(prob_threshold, disp_threshold, num_consistent, sources, voxel, voxel_slots, normal_jump)
    pairs = mvsio.read_pair_file(os.path.join(pair_folder, "pair.txt"))
    order = consensus_order(pairs, sources)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    pfm = lambda kind, v: up(mvsio.read_pfm(os.path.join(out_folder, kind, "%08d.pfm" % v))[0])
    cams, depths, confs, rgbs = {}, {}, {}, {}
    for v in sorted({v for r, src in order for v in [r] + src}):
        cams[v] = mvsio.read_camera_parameters(os.path.join(scan_folder, "cams", "%08d_cam.txt" % v))
        depths[v] = pfm("depth_est", v)
        confs[v] = pfm("confidence", v)
        img = np.array(Image.open(os.path.join(scan_folder, "images", "%08d.jpg" % v)))
        if img.dtype != np.uint8 or img.shape != tuple(depths[v].shape) + (3,):
            raise ValueError("image of view %d: %s %s, expected uint8 %s" % (
                v, img.dtype, img.shape, tuple(depths[v].shape) + (3,)))
        rgbs[v] = up(img)
    return fuse_consensus_resident(pairs, cams, depths, confs, rgbs, plyfilename, prob_threshold, disp_threshold,
                                   num_consistent, sources, os.path.join(out_folder, "mask") if save_masks else None,
                                   max_points, device, voxel, voxel_slots, normals, normal_jump)
