"""Depth-map fusion on the GPU: the reference's two runnable filters
(test_uni.py --filter_method) with the per-pixel reprojection checks in one HIP kernel per reference view
(k_fusion.hip):
  method="dypcd"  the dynamic-consistency filter (filter/dypcd.py, `dypcd_filter` / `filter_depth`): masks at
                  i * dist_base pixels and i * rel_diff_base relative depth, i = 2..10, a pixel kept when i views
                  agree at some i (damvs_fusion_view);
  method="pcd"    the static CasMVSNet filter (filter/pcd.py): one mask per source at dist_thr pixels and rel_thr
                  relative depth (the reference's constants 1 and 0.01), a pixel kept when at least thres_view
                  sources agree (damvs_fusion_view_static).
The third method, gipuma, needs an external CUDA binary and is out of scope.

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
