"""Scene reconstruction in memory: a forward's outputs go to depth fusion while they
are still on the device, and one call leads from a scene directory to a PLY.

The reference's test path (test_uni.py:246-287) copies six maps per reference view to the host, writes them as PFMs with
the camera and the image, and its filter (filter/dypcd.py:198-209) reads four of them back per view. Here
`SceneMaps.add` hands a batch of `CascadeMVSNet.forward` outputs to one HIP launch (k_scene.hip, damvs_scene_ingest)
that writes each sample into its slot of three scene-resident stores: the final depth, the three confidences at the
final resolution (stage 1 and 2 upsampled by nearest neighbour, mvsio.resize_nearest at exactly x4 / x2) and the
reference image as uint8 HWC. `SceneMaps.fuse` runs fusion.fuse_scene's per-pair loop over those stores
(fusion.fuse_resident), `SceneMaps.save` writes the reference's tree for tools that want the files, and
`reconstruct_scene` drives the whole path for one scan.

The other end of the forward (row f3): `SceneInputs` keeps the scan's decoded images on the device as uint8, each view
uploaded once, and writes the forward's `imgs` for a batch by one HIP launch (k_inputs.hip, damvs_scene_inputs) in
place of the host's float conversion, resize, stack and per-batch float32 upload (`reconstruct_scene(inputs="device")`).

Between the two (row f1): FeatureNet's output depends on the image alone, and a scan lists each view in about `nviews`
samples. `SceneFeatures` runs FeatureNet once per view into scene-resident stores and hands a batch the list
`CascadeMVSNet.extract_features` would compute, by one HIP launch that gathers the views' blocks (k_features.hip,
damvs_feature_gather); `CascadeMVSNet.forward(features=...)` takes it (`reconstruct_scene(features="scene")`).

A stated difference: the reference re-encodes the reference image as JPEG (test_uni.py:286-287) and the fusion reads
that file back, so its colours carry JPEG loss. The in-memory path takes the colour before the JPEG. Positions, masks
and point order are those of the file path bit for bit; colours are equal whenever the file path's images are lossless.
"""
from __future__ import annotations

import concurrent.futures as cf
import ctypes
import os

import numpy as np
import torch

from . import _capi, fusion, mvsio
from ._capi import check

_fusion = fusion  # reconstruct_scene has a parameter of the module's name


class SceneMaps:
    """The scene-resident inputs of depth fusion for the listed views, all of one size (H, W multiples of 4):
    `depth` (V, H, W) float32, `conf` (V, 3, H, W) float32 in the order the fusion kernels take them (final, stage 2,
    stage 1) and `rgb` (V, H, W, 3) uint8 on `device`, view i of `view_ids` in slot i, and on the host `cams`, a dict
    view id -> (K (3, 3), E (4, 4)) float32. A slot holds nothing until its view is added."""

    def __init__(self, view_ids, H, W, device="cuda"):
        view_ids = [int(v) for v in view_ids]
        if len(set(view_ids)) != len(view_ids) or not view_ids:
            raise ValueError("view_ids must be a non-empty list of distinct view ids")
        if H < 4 or W < 4 or H % 4 or W % 4:
            raise ValueError("H and W must be positive multiples of 4 (got %d x %d)" % (H, W))
        self.view_ids, self.H, self.W, self.device = view_ids, int(H), int(W), torch.device(device)
        self.slot = {v: i for i, v in enumerate(view_ids)}
        V = len(view_ids)
        self.depth = torch.empty(V, H, W, device=self.device, dtype=torch.float32)
        self.conf = torch.empty(V, 3, H, W, device=self.device, dtype=torch.float32)
        self.rgb = torch.empty(V, H, W, 3, device=self.device, dtype=torch.uint8)
        self.cams = {}
        self._cam_files = {}  # view id -> the (2, 4, 4) array mvsio.write_cam takes
        self._added, self._coloured = set(), set()

    # ------------------------------------------------------------------------------------------------- add
    def _check_map(self, t, name, shape, views):
        if not torch.is_tensor(t) or not t.is_cuda or t.device != self.depth.device:
            raise ValueError("%s of views %s must be a CUDA tensor on %s" % (name, views, self.depth.device))
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("%s of views %s must be contiguous float32 (got %s%s)" % (
                name, views, t.dtype, "" if t.is_contiguous() else ", non-contiguous"))
        if tuple(t.shape) != shape:
            raise ValueError("%s of views %s has shape %s, the scene needs %s" % (name, views, tuple(t.shape), shape))
        return t.detach()

    def add(self, view_ids, outputs, imgs=None, cams=None, rgb=None):
        """A forward's batch into the stores: one ingest launch on the current stream, no host synchronisation.
        view_ids: the batch's reference views; outputs: the dictionary CascadeMVSNet.forward returns ("depth" and
        "photometric_confidence" at (B, H, W), "stage2" / "stage1" confidences at (B, H/2, W/2) / (B, H/4, W/4));
        imgs: the forward's (B, N, 3, H, W) float32 input, view 0 read in place through the batch stride and stored as
        uint8(clip(img * 255, 0, 255)) (test_uni.py:285); rgb: instead of imgs, (B, H, W, 3) uint8 decoded images,
        copied as they are; cams: proj_matrices["stage3"][:, 0] as a host array (B, 2, 4, 4): E = [0], K = [1, :3, :3],
        what mvsio.write_cam writes and read_camera_parameters reads back (shortest-repr float32 text round-trips
        exactly). A view without cams cannot be fused, a reference view without colour neither.
        Raises ValueError, naming the views, before anything is written: map shapes other than (H, W), (H/2, W/2),
        (H/4, W/4), non-CUDA or non-contiguous tensors, unknown view ids, a view added twice."""
        view_ids = [int(v) for v in view_ids]
        B, H, W = len(view_ids), self.H, self.W
        if not 1 <= B <= _capi.SCENE_MAX_BATCH:
            raise ValueError("a batch of 1..%d views per call (got %d)" % (_capi.SCENE_MAX_BATCH, B))
        for v in view_ids:
            if v not in self.slot:
                raise ValueError("view %d is not one of the scene's views %s" % (v, self.view_ids))
            if v in self._added or view_ids.count(v) > 1:
                raise ValueError("view %d added twice" % v)
        depth = self._check_map(outputs["depth"], "depth", (B, H, W), view_ids)
        conf3 = self._check_map(outputs["photometric_confidence"], "photometric_confidence", (B, H, W), view_ids)
        conf2 = self._check_map(outputs["stage2"]["photometric_confidence"], "stage2 photometric_confidence",
                                (B, H // 2, W // 2), view_ids)
        conf1 = self._check_map(outputs["stage1"]["photometric_confidence"], "stage1 photometric_confidence",
                                (B, H // 4, W // 4), view_ids)
        if imgs is not None and rgb is not None:
            raise ValueError("views %s: give imgs or rgb, not both" % view_ids)
        img_ptr, img_stride = None, 0
        if imgs is not None:
            ok = torch.is_tensor(imgs) and imgs.is_cuda and imgs.device == self.depth.device and \
                imgs.dtype == torch.float32 and imgs.dim() == 5 and tuple(imgs.shape[2:]) == (3, H, W) and \
                imgs.shape[0] == B and tuple(imgs.stride()[2:]) == (H * W, W, 1)
            if not ok:
                raise ValueError("imgs of views %s must be a float32 CUDA tensor (%d, N, 3, %d, %d) with contiguous "
                                 "images" % (view_ids, B, H, W))
            img_ptr, img_stride = imgs.data_ptr(), imgs.stride(0) if B > 1 else 0
        if rgb is not None:
            rgb = torch.as_tensor(rgb)
            if rgb.dtype != torch.uint8 or tuple(rgb.shape) != (B, H, W, 3):
                raise ValueError("rgb of views %s must be uint8 (%d, %d, %d, 3), got %s %s" % (
                    view_ids, B, H, W, rgb.dtype, tuple(rgb.shape)))
        if cams is not None:
            cams = np.array(cams.cpu() if torch.is_tensor(cams) else cams, dtype=np.float32)
            if cams.shape != (B, 2, 4, 4):
                raise ValueError("cams of views %s must be (%d, 2, 4, 4), got %s" % (view_ids, B, cams.shape))
        slots = (ctypes.c_int * B)(*[self.slot[v] for v in view_ids])
        lib = _capi.load_library()
        check(lib.damvs_scene_ingest(_capi.stream_ptr(self.depth.device), B, H, W, len(self.view_ids),
                                     depth.data_ptr(), conf3.data_ptr(), conf2.data_ptr(), conf1.data_ptr(), img_ptr,
                                     img_stride, slots, self.depth.data_ptr(), self.conf.data_ptr(),
                                     self.rgb.data_ptr()))
        if rgb is not None:
            index = torch.tensor([self.slot[v] for v in view_ids], dtype=torch.int64).to(self.depth.device,
                                                                                       non_blocking=True)
            self.rgb.index_copy_(0, index, rgb.to(self.depth.device, non_blocking=True))
        for b, v in enumerate(view_ids):
            self._added.add(v)
            if imgs is not None or rgb is not None:
                self._coloured.add(v)
            if cams is not None:
                self.cams[v] = (cams[b, 1, :3, :3].copy(), cams[b, 0].copy())
                self._cam_files[v] = cams[b].copy()

    # ------------------------------------------------------------------------------------------------ fuse
    def _require(self, views, what):
        for v in views:
            if v not in self._added:
                raise ValueError("view %d %s but was never added" % (v, what))
            if v not in self.cams:
                raise ValueError("view %d %s but was added without cams" % (v, what))

    def fuse(self, pairs, plyfilename, conf=(0.1, 0.15, 0.9), dist_base=0.25, rel_diff_base=1 / 1300, method="dypcd",
             thres_view=5, mask_dir=None, max_points=None, voxel=None, voxel_slots=None, normals=False,
             normal_jump=0.01):
        """fusion.fuse_scene's per-pair loop over the stores (fusion.fuse_resident): per pair the fusion kernel and
        compact_cloud on one cursor, one copy of count * 15 bytes, mvsio.write_ply_records. pairs: [(ref view,
        [source views])] or the path of a pair.txt (read as filter/dypcd.py:84-95 reads it); mask_dir: where the photo /
        geo / final PNGs go (None: not written). Positions, masks and point order are those of fuse_scene over the
        files `save` writes, bit for bit; colours too when those images are lossless (the module docstring).
        voxel, voxel_slots: thin the cloud on the device to one point per cell of a grid of that edge
        (fusion.fuse_resident's docstring). normals, normal_jump: the oriented PLY, 27 bytes a point, each normal
        computed on the device from the view's averaged depth (fusion.fuse_resident's docstring).
        A pair that names a view never added raises ValueError and writes no PLY. Returns the point count."""
        fusion.check_voxel(voxel, voxel_slots)
        fusion.check_normal_jump(normal_jump)
        if isinstance(pairs, (str, os.PathLike)):
            pairs = mvsio.read_pair_file(pairs)
        pairs = [(int(r), [int(s) for s in src]) for r, src in pairs]
        for r, src in pairs:
            self._require([r], "is a reference view of the pair list")
            self._require(src, "is a source of view %d" % r)
            if r not in self._coloured:
                raise ValueError("reference view %d was added without imgs or rgb" % r)
        used = {v for r, src in pairs for v in [r] + src}
        refs = {r for r, _ in pairs}
        depths = {v: self.depth[self.slot[v]] for v in used}
        confs = {v: tuple(self.conf[self.slot[v], k] for k in range(3)) for v in refs}
        rgbs = {v: self.rgb[self.slot[v]] for v in refs}
        return fusion.fuse_resident(pairs, self.cams, depths, confs, rgbs, plyfilename, conf, dist_base, rel_diff_base,
                                    method, thres_view, mask_dir, max_points, self.depth.device, voxel, voxel_slots,
                                    normals=normals, normal_jump=normal_jump)

    def fuse_consensus(self, pairs, plyfilename, prob_threshold=0.1, disp_threshold=0.15, num_consistent=3,
                       sources="all", mask_dir=None, max_points=None, voxel=None, voxel_slots=None, normals=False,
                       normal_jump=0.01):
        """Consensus fusion over the stores (fusion.fuse_consensus_resident; fusion.consensus_statement is the rule): every
        surface point once, at the average of the agreeing views' points and colours. pairs: [(ref view, [source
        views])] or the path of a pair.txt; sources "all": every other view the pair list names, "pairs": the pair's
        own sources. Every view used, sources too, must have been added with cams and with colour (imgs or rgb).
        mask_dir: where the valid / geo / final / consumed PNGs go (None: not written); the other arguments as `fuse`.
        The PLY is that of fusion.fuse_consensus_scene over the files `save` writes, bit for bit when those images are
        lossless. A bad argument, or a view that is missing, raises ValueError before anything is launched and writes no
        PLY. Returns the point count."""
        fusion._check_consensus_driver(prob_threshold, disp_threshold, num_consistent, sources, voxel, voxel_slots,
                                       normal_jump)
        if isinstance(pairs, (str, os.PathLike)):
            pairs = mvsio.read_pair_file(pairs)
        pairs = [(int(r), [int(s) for s in src]) for r, src in pairs]
        order = fusion.consensus_order(pairs, sources)
        for r, src in order:
            self._require([r], "is a reference view of the pair list")
            self._require(src, "is a source of view %d" % r)
        used = sorted({v for r, src in order for v in [r] + src})
        for v in used:
            if v not in self._coloured:
                raise ValueError("view %d was added without imgs or rgb: consensus fusion averages the colours of "
                                 "every view it uses" % v)
        depths = {v: self.depth[self.slot[v]] for v in used}
        confs = {v: self.conf[self.slot[v], 0] for v in used}
        rgbs = {v: self.rgb[self.slot[v]] for v in used}
        return fusion.fuse_consensus_resident(pairs, self.cams, depths, confs, rgbs, plyfilename, prob_threshold,
                                              disp_threshold, num_consistent, sources, mask_dir, max_points,
                                              self.depth.device, voxel, voxel_slots, normals, normal_jump)

    # ------------------------------------------------------------------------------------------------ save
    def save(self, outdir, scan, lossless=False):
        """The reference's tree for the views added so far (test_uni.py:265-287), for tools that read it:
        <outdir>/<scan>/depth_est/%08d.pfm, confidence/%08d{,_stage2,_stage1}.pfm (the bytes mvsio.save_stage_outputs
        writes), cams/%08d_cam.txt (mvsio.write_cam) and images/%08d.jpg; fusion.fuse_scene(<pair folder>,
        <outdir>/<scan>, <outdir>/<scan>, ...) reads it back. lossless: PNG data under the .jpg name (readers decode by
        content), so the colours survive the round trip; otherwise JPEG, as the reference.
        The stage-1 and stage-2 depth maps (depth_est/%08d_stage{1,2}.pfm in the reference) are not kept in the stores
        and are not written: nothing downstream reads them."""
        from PIL import Image
        root = os.path.join(outdir, scan)
        for d in ("depth_est", "confidence", "cams", "images"):
            os.makedirs(os.path.join(root, d), exist_ok=True)
        for v in self.view_ids:
            if v not in self._added:
                continue
            s = self.slot[v]
            mvsio.save_pfm(os.path.join(root, "depth_est", "%08d.pfm" % v), self.depth[s].cpu().numpy())
            c = self.conf[s].cpu().numpy()
            for k, sfx in enumerate(("", "_stage2", "_stage1")):
                mvsio.save_pfm(os.path.join(root, "confidence", "%08d%s.pfm" % (v, sfx)), c[k])
            if v in self._cam_files:
                mvsio.write_cam(os.path.join(root, "cams", "%08d_cam.txt" % v), self._cam_files[v])
            if v in self._coloured:
                Image.fromarray(self.rgb[s].cpu().numpy()).save(os.path.join(root, "images", "%08d.jpg" % v),
                                                                format="PNG" if lossless else "JPEG")


class SceneInputs:
    """The decoded images of a scene's views, resident on the device as the bytes they were decoded to, and the
    forward's `imgs` tensor from them: `store` (V, H0, W0, 3) uint8 on `device`, view i of `view_ids` in slot i, and
    `mirror`, a host array of the same shape (pinned when the device is a GPU: the whole mirror, so no staging buffer
    is ever reused under an upload that is still in flight). `put` uploads a view once; `batch` is one launch of
    damvs_scene_inputs (k_inputs.hip), which converts to float32 in [0, 1], resizes to the working size H x W and
    writes planar images (include/damvs.h states the arithmetic)."""

    def __init__(self, view_ids, H0, W0, H, W, device="cuda"):
        view_ids = [int(v) for v in view_ids]
        if len(set(view_ids)) != len(view_ids) or not view_ids:
            raise ValueError("view_ids must be a non-empty list of distinct view ids")
        if min(H0, W0, H, W) < 1 or W % 4:
            raise ValueError("sizes of at least 1 and W a multiple of 4 (got %d x %d -> %d x %d)" % (H0, W0, H, W))
        self.view_ids, self.device = view_ids, torch.device(device)
        self.H0, self.W0, self.H, self.W = int(H0), int(W0), int(H), int(W)
        self.slot = {v: i for i, v in enumerate(view_ids)}
        shape = (len(view_ids), self.H0, self.W0, 3)
        self.store = torch.empty(shape, device=self.device, dtype=torch.uint8)
        self.mirror = torch.empty(shape, dtype=torch.uint8, pin_memory=self.device.type == "cuda")
        self._put = set()

    def put(self, view_id, rgb):
        """A decoded view, (H0, W0, 3) uint8, into its slot: copied into the mirror, then one non-blocking upload of
        that slice on the current stream. ValueError, naming the view: an unknown view, a view put twice, another
        shape or dtype (grey and RGBA images are refused, not converted)."""
        view_id = int(view_id)
        if view_id not in self.slot:
            raise ValueError("view %d is not one of the scene's views %s" % (view_id, self.view_ids))
        if view_id in self._put:
            raise ValueError("view %d put twice" % view_id)
        rgb = np.asarray(rgb)
        if rgb.dtype != np.uint8 or rgb.shape != (self.H0, self.W0, 3):
            raise ValueError("view %d must be a uint8 image (%d, %d, 3), got %s %s" % (
                view_id, self.H0, self.W0, rgb.dtype, rgb.shape))
        s = self.slot[view_id]
        self.mirror[s].numpy()[...] = rgb
        self.store[s].copy_(self.mirror[s], non_blocking=True)
        self._put.add(view_id)

    def batch(self, views, out=None):
        """views: B lists of N view ids, the reference view first -> the forward's (B, N, 3, H, W) float32 `imgs`, by
        one damvs_scene_inputs launch on the current stream (no allocation when `out` is given and fits: a contiguous
        float32 tensor on the device with at least B * N * 3 * H * W elements, whose leading part is returned in that
        shape). ValueError: a view that was never put, lists of different lengths, B * N outside
        1..DAMVS_INPUTS_MAX_IMAGES."""
        views = [[int(v) for v in sample] for sample in views]
        B, N = len(views), len(views[0]) if views else 0
        if any(len(sample) != N for sample in views):
            raise ValueError("ragged view lists %s: every sample needs the same number of views" % views)
        n = B * N
        if not 1 <= n <= _capi.INPUTS_MAX_IMAGES:
            raise ValueError("a batch of 1..%d images per call (got %d x %d)" % (_capi.INPUTS_MAX_IMAGES, B, N))
        for v in (v for sample in views for v in sample):
            if v not in self._put:
                raise ValueError("view %d was never put" % v)
        need = n * 3 * self.H * self.W
        fits = torch.is_tensor(out) and out.dtype == torch.float32 and out.device == self.store.device and \
            out.is_contiguous() and out.numel() >= need
        imgs = out.view(-1)[:need].view(B, N, 3, self.H, self.W) if fits else \
            torch.empty(B, N, 3, self.H, self.W, device=self.device, dtype=torch.float32)
        slots = (ctypes.c_int * n)(*[self.slot[v] for sample in views for v in sample])
        lib = _capi.load_library()
        check(lib.damvs_scene_inputs(_capi.stream_ptr(self.store.device), n, self.H0, self.W0, self.H, self.W,
                                     len(self.view_ids), self.store.data_ptr(), slots, imgs.data_ptr()))
        return imgs


class SceneFeatures:
    """FeatureNet's outputs for a scene's views, each computed once: `stores["stage1" | "stage2" | "stage3"]`, one
    tensor (V, h_s, w_s, C_s) per FeatureNet output at (H/4, W/4, 32), (H/2, W/2, 16), (H, W, 8) in the HIP front
    end's storage dtype (`model.frontend_dtype` or float32), NHWC, exactly what `model.extract_features` returns; view
    i of `view_ids` in slot i. `put` runs FeatureNet over a group of images into their slots; `batch` is one launch of
    damvs_feature_gather (k_features.hip) that copies the listed views' blocks into the per-view tensors a stage takes.
    The stores hold 14 * H * W elements per view: about 53 MB per view at 1184 x 1600 in bf16 and 106 MB in fp32
    (`nbytes` reports the total; 49 views: 2.6 GB / 5.2 GB). The caller decides whether a scan fits.
    HIP front end only. The features belong to the weights they were computed with: after the model's weights changed
    (or the model moved), the next `put` or `batch` raises ValueError."""

    STAGES = ("stage1", "stage2", "stage3")

    def __init__(self, model, view_ids, H, W, device="cuda"):
        view_ids = [int(v) for v in view_ids]
        if len(set(view_ids)) != len(view_ids) or not view_ids:
            raise ValueError("view_ids must be a non-empty list of distinct view ids")
        if getattr(model, "frontend_impl", None) != "hip":
            raise ValueError("SceneFeatures keeps the HIP front end's NHWC features (frontend_impl=\"hip\")")
        if H < 4 or W < 4 or H % 4 or W % 4:
            raise ValueError("H and W must be positive multiples of 4 (got %d x %d)" % (H, W))
        self.model, self.view_ids, self.H, self.W, self.device = model, view_ids, int(H), int(W), torch.device(device)
        self.slot = {v: i for i, v in enumerate(view_ids)}
        self.dtype = model.frontend_dtype or torch.float32
        self.stores = {}
        for name, scale, C in zip(self.STAGES, (4, 2, 1), model.feature.out_channels):
            self.stores[name] = torch.empty(len(view_ids), self.H // scale, self.W // scale, (C + 3) // 4 * 4,
                                            device=self.device, dtype=self.dtype)
        self.nbytes = sum(t.numel() * t.element_size() for t in self.stores.values())
        self._put, self._key = set(), None

    def _featurenet(self):
        """The model's HipFeatureNet; ValueError if views were put under other weights (CascadeMVSNet._folded_key)."""
        feat, _ = self.model._frontend()
        key = self.model._folded_key
        if self._put and key != self._key:
            raise ValueError("the model's weights changed after views %s were put: their features are stale" %
                             sorted(self._put))
        self._key = key
        return feat

    def put(self, view_ids, imgs):
        """view_ids: G views; imgs: their (G, 3, H, W) float32 planar images on the device, what the forward takes.
        One batched FeatureNet call on the current stream, no host synchronisation (groups that would pass
        HipFeatureNet.MAX_ACT_BYTES are split). The last layer of each output writes into the stores when the group's
        slots are consecutive; otherwise the outputs are copied into their slots (index_copy_).
        ValueError, naming the views, before anything is written: an unknown view, a view put twice, imgs of another
        shape, dtype or device."""
        view_ids = [int(v) for v in view_ids]
        for v in view_ids:
            if v not in self.slot:
                raise ValueError("view %d is not one of the scene's views %s" % (v, self.view_ids))
            if v in self._put or view_ids.count(v) > 1:
                raise ValueError("view %d put twice" % v)
        G, want = len(view_ids), (len(view_ids), 3, self.H, self.W)
        store = self.stores["stage3"]
        if not torch.is_tensor(imgs) or imgs.dtype != torch.float32 or tuple(imgs.shape) != want or \
                imgs.device != store.device:
            raise ValueError("imgs of views %s must be a float32 tensor %s on %s (got %s)" % (
                view_ids, want, store.device,
                "%s %s on %s" % (imgs.dtype, tuple(imgs.shape), imgs.device) if torch.is_tensor(imgs)
                else type(imgs).__name__))
        if not G:
            return
        feat = self._featurenet()
        per_image = self.H * self.W * 8 * store.element_size()  # FeatureNet's widest activation
        g = max(1, feat.MAX_ACT_BYTES // per_image)
        slots = [self.slot[v] for v in view_ids]
        with torch.no_grad():
            for i0 in range(0, G, g):
                sl, x = slots[i0:i0 + g], imgs[i0:i0 + g]
                if sl == list(range(sl[0], sl[0] + len(sl))):
                    feat(x, out={k: t[sl[0]:sl[0] + len(sl)] for k, t in self.stores.items()})
                else:
                    f = feat(x)
                    index = torch.tensor(sl, dtype=torch.int64).to(store.device, non_blocking=True)
                    for k, t in self.stores.items():
                        t.index_copy_(0, index, f[k])
        self._put.update(view_ids)

    def buffers(self, n_pairs):
        """{stage: (n_pairs, h_s, w_s, C_s)} uninitialised, for `batch(out=)`."""
        return {k: torch.empty((n_pairs,) + tuple(t.shape[1:]), device=t.device, dtype=t.dtype)
                for k, t in self.stores.items()}

    def batch(self, views, out=None):
        """views: B lists of N view ids, the reference view first (a view may repeat inside a sample: pair.txt's fill
        rule) -> the list `extract_features` returns for those images: N dicts {stage: (B, h_s, w_s, C_s)}, view n's
        tensors contiguous slices (rows n * B .. (n + 1) * B) of one buffer per stage, written by one
        damvs_feature_gather launch on the current stream, pairs ordered view-major. No allocation when `out` fits:
        {stage: buffer} as `buffers` returns (contiguous, the stores' dtype and device, at least B * N views' elements),
        whose leading parts are used; otherwise new buffers. ValueError, naming the views: a view that was never put,
        lists of different lengths, B * N outside 1..DAMVS_FEATURES_MAX_PAIRS."""
        views = [[int(v) for v in sample] for sample in views]
        B, N = len(views), len(views[0]) if views else 0
        if any(len(sample) != N for sample in views):
            raise ValueError("ragged view lists %s: every sample needs the same number of views" % views)
        n = B * N
        if not 1 <= n <= _capi.FEATURES_MAX_PAIRS:
            raise ValueError("a batch of 1..%d (sample, view) pairs per call (got %d x %d, views %s)" % (
                _capi.FEATURES_MAX_PAIRS, B, N, views))
        for v in (v for sample in views for v in sample):
            if v not in self._put:
                raise ValueError("view %d was never put" % v)
        self._featurenet()
        bufs = {}
        for k, t in self.stores.items():
            shape, o = (n,) + tuple(t.shape[1:]), out.get(k) if isinstance(out, dict) else None
            need = n * t[0].numel()
            fits = torch.is_tensor(o) and o.dtype == t.dtype and o.device == t.device and o.is_contiguous() and \
                o.numel() >= need
            bufs[k] = o.view(-1)[:need].view(shape) if fits else torch.empty(shape, device=t.device, dtype=t.dtype)
        K = len(self.STAGES)
        stores = (ctypes.c_void_p * K)(*[self.stores[k].data_ptr() for k in self.STAGES])
        outs = (ctypes.c_void_p * K)(*[bufs[k].data_ptr() for k in self.STAGES])
        view_bytes = (ctypes.c_ulonglong * K)(*[self.stores[k][0].numel() * self.stores[k].element_size()
                                                 for k in self.STAGES])
        slots = (ctypes.c_int * n)(*[self.slot[views[b][v]] for v in range(N) for b in range(B)])
        lib = _capi.load_library()
        check(lib.damvs_feature_gather(_capi.stream_ptr(self.stores["stage3"].device), n, K, len(self.view_ids), stores,
                                       view_bytes, slots, outs))
        return [{k: bufs[k][v * B:(v + 1) * B] for k in self.STAGES} for v in range(N)]


def _device_store(ds, scan, device, decode_workers):
    """reconstruct_scene's inputs="device": the samples without pixels and a SceneInputs with every view of the scan,
    decoded in `decode_workers` threads and put as soon as it is ready."""
    samples = [ds.cameras(i) for i in range(len(ds))]
    sizes = sorted({s["original_size"] for s in samples})
    if len(sizes) != 1:
        raise ValueError("the images of %s have sizes %s: one scene, one size" % (scan, sizes))
    (H0, W0), (H, W) = sizes[0], samples[0]["size"]
    store = SceneInputs(sorted({v for s in samples for v in s["view_ids"]}), H0, W0, H, W, device)
    with cf.ThreadPoolExecutor(decode_workers) as pool:
        decoding = {pool.submit(mvsio.read_img_bytes, ds._img_path(scan, v)): v for v in store.view_ids}
        for done in cf.as_completed(decoding):
            store.put(decoding[done], done.result())
    return samples, store


def _device_batches(samples, store, batch, reference_only=False, reused=None):
    """Per batch of `batch` samples (the samples, `imgs` in one reused buffer); reference_only: `imgs` holds view 0 of
    each sample alone, (B, 1, 3, H, W)."""
    for i0 in range(0, len(samples), batch):
        items = samples[i0:i0 + batch]
        imgs = store.batch([it["view_ids"][:1] if reference_only else it["view_ids"] for it in items], out=reused)
        reused = imgs if reused is None else reused  # the first batch is the largest
        yield items, imgs


def _groups(views, n):
    return [views[i:i + n] for i in range(0, len(views), n)]


CONSENSUS_KWARGS = ("prob_threshold", "disp_threshold", "num_consistent", "sources", "mask_dir", "max_points", "voxel",
                    "voxel_slots", "normals", "normal_jump")


def reconstruct_scene(model, datapath, scan, plyfilename, nviews=5, ndepths=192, interval_scale=1.06, max_h=1184,
                      max_w=1600, batch=4, streams=1, inputs="host", decode_workers=4, features="batch", fusion="pairs",
                      **fuse_kwargs):
    """One scan from its directory (<datapath>/<scan>/{pair.txt, cams/, images/}) to a fused PLY without the disk in
    between: mvsio.EvalScenes samples in batches of `batch` reference views through `model` (a CascadeMVSNet on a HIP
    device; `streams` as in its forward) with check_range=False, each batch into a SceneMaps, one
    model.DepthNet.check_range() after the last batch, then SceneMaps.fuse over the scan's pair.txt with
    `fuse_kwargs` (conf, dist_base, rel_diff_base, method, thres_view, mask_dir, max_points, voxel, voxel_slots, normals,
    normal_jump; voxel and voxel_slots thin the cloud to one point per voxel, normals=True writes the oriented PLY with a
    normal per point, fusion.fuse_resident's docstring, and a bad value of these raises ValueError before the scan is
    read). fusion: "pairs", the default, is that path. "consensus" calls SceneMaps.fuse_consensus instead (every surface
    point once, averaged over the agreeing views: fusion.consensus_statement); `fuse_kwargs` are then its arguments
    (prob_threshold, disp_threshold, num_consistent, sources, mask_dir, max_points, voxel, voxel_slots, normals,
    normal_jump), checked before the scan is read as well. Every image of the scan is
    decoded and scaled once (EvalScenes' cache_views). All views must come out at one size. Returns the point count.
    Colours are taken before the reference's JPEG re-encoding (the module docstring).
    inputs: "host" converts, resizes and stacks the images with numpy and torch on the CPU and uploads every batch as
    float32. "device" decodes the views to uint8 in `decode_workers` threads, uploads each once into a SceneInputs as
    soon as it is decoded and lets one launch per batch write `imgs` into one reused buffer; the cameras come from
    EvalScenes.cameras. The two agree bit for bit when the images need no resize; a resized image differs from the
    host's in its last bits (at most 2^-21: tests/test_inputs.py), so the depth maps may too. The device path needs
    image files of one size and raises ValueError otherwise.
    features: "batch" runs FeatureNet on the B * nviews images of every batch. "scene" first puts every view that a
    sample lists through FeatureNet once, in groups of at most batch * nviews images, into a SceneFeatures (its
    docstring states the memory: 14 * H * W elements per view); each batch then uploads or writes its reference views'
    images alone, gathers its features by one launch and calls model(..., features=...). The maps and the PLY are those
    of "batch" bit for bit (FeatureNet's result for an image does not depend on the rest of its batch)."""
    if inputs not in ("host", "device"):
        raise ValueError("inputs must be \"host\" or \"device\" (got %r)" % (inputs,))
    if features not in ("batch", "scene"):
        raise ValueError("features must be \"batch\" or \"scene\" (got %r)" % (features,))
    if not isinstance(decode_workers, int) or decode_workers < 1:
        raise ValueError("decode_workers must be a positive integer (got %r)" % (decode_workers,))
    if fusion not in ("pairs", "consensus"):
        raise ValueError("fusion must be \"pairs\" or \"consensus\" (got %r)" % (fusion,))
    consensus = fusion == "consensus"
    if consensus:
        unknown = sorted(set(fuse_kwargs) - set(CONSENSUS_KWARGS))
        if unknown:
            raise ValueError("fusion=\"consensus\" takes %s, not %s" % (", ".join(CONSENSUS_KWARGS), ", ".join(unknown)))
        _fusion._check_consensus_driver(
            fuse_kwargs.get("prob_threshold", 0.1), fuse_kwargs.get("disp_threshold", 0.15),
            fuse_kwargs.get("num_consistent", 3), fuse_kwargs.get("sources", "all"), fuse_kwargs.get("voxel"),
            fuse_kwargs.get("voxel_slots"), fuse_kwargs.get("normal_jump", 0.01))
    _fusion.check_voxel(fuse_kwargs.get("voxel"), fuse_kwargs.get("voxel_slots"))
    _fusion.check_normal_jump(fuse_kwargs.get("normal_jump", 0.01))
    ds = mvsio.EvalScenes(datapath, [scan], nviews, ndepths=ndepths, interval_scale=interval_scale, max_h=max_h,
                          max_w=max_w, cache_views=True)
    device = next(model.parameters()).device
    refs = [ref for _, ref, _ in ds.metas]
    maps = feats = fbufs = None
    device_batches = None
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    sample_views = lambda i: [ds.metas[i][1]] + ds.metas[i][2][:nviews - 1]
    with torch.no_grad():
        if inputs == "device":
            samples, store = _device_store(ds, scan, device, decode_workers)
            reused = None
            if features == "scene":
                feats = SceneFeatures(model, store.view_ids, store.H, store.W, device)
                for group in _groups(store.view_ids, batch * nviews):
                    imgs = store.batch([[v] for v in group], out=reused)
                    reused = imgs if reused is None else reused  # the first group is the largest
                    feats.put(group, imgs[:, 0])
            device_batches = _device_batches(samples, store, batch, features == "scene", reused)
        elif features == "scene":
            used = sorted({v for i in range(len(ds)) for v in sample_views(i)})
            found = {}  # view -> its scaled host image, until its group is put
            for i in range(len(ds)):
                it = ds[i]
                if feats is None:
                    feats = SceneFeatures(model, used, it["imgs"].shape[2], it["imgs"].shape[3], device)
                if it["imgs"].shape[2:] != (feats.H, feats.W):
                    raise ValueError("view %d of %s comes out at %s, the scene at %s: one scene, one size" % (
                        refs[i], scan, it["imgs"].shape[2:], (feats.H, feats.W)))
                for n, v in enumerate(sample_views(i)):
                    if v not in found and v not in feats._put:
                        found[v] = it["imgs"][n]
                if len(found) >= batch * nviews or i == len(ds) - 1:
                    for group in _groups(sorted(found), batch * nviews):
                        feats.put(group, up(np.stack([found[v] for v in group])))
                    found = {}
        if feats is not None:
            fbufs = feats.buffers(min(batch, len(ds)) * nviews)
        for i0 in range(0, len(ds), batch):
            if device_batches is not None:
                items, imgs = next(device_batches)
            else:
                items = [ds[i] for i in range(i0, min(i0 + batch, len(ds)))]
                shapes = {it["imgs"].shape for it in items}
                if len(shapes) != 1 or (maps is not None and next(iter(shapes))[2:] != (maps.H, maps.W)):
                    raise ValueError("views %s of %s come out at sizes %s: one scene, one size" % (
                        refs[i0:i0 + len(items)], scan, sorted(shapes)))
                imgs = up(np.stack([it["imgs"][:1] if feats is not None else it["imgs"] for it in items]))
            proj_host = {k: np.stack([it["proj_matrices"][k] for it in items]) for k in items[0]["proj_matrices"]}
            proj = {k: up(v) for k, v in proj_host.items()}
            depth_values = up(np.stack([it["depth_values"] for it in items]))
            ins = {k: up(np.stack([it["intrinsics_matrices"][k] for it in items]))
                   for k in items[0]["intrinsics_matrices"]}
            if maps is None:
                maps = SceneMaps(refs, imgs.shape[3], imgs.shape[4], device)
            if feats is not None:
                f = feats.batch([sample_views(i) for i in range(i0, i0 + len(items))], out=fbufs)
                out = model(imgs, proj, depth_values, ins, streams=streams, check_range=False, features=f)
            else:
                out = model(imgs, proj, depth_values, ins, streams=streams, check_range=False)
            maps.add(refs[i0:i0 + len(items)], out, imgs=imgs, cams=proj_host["stage3"][:, 0])
    model.DepthNet.check_range()
    pair_file = os.path.join(datapath, scan, "pair.txt")
    if consensus:
        return maps.fuse_consensus(pair_file, plyfilename, **fuse_kwargs)
    return maps.fuse(pair_file, plyfilename, **fuse_kwargs)
