"""The initial neural point cloud from posed depth frames, on the device (csrc/cloud_init.hip).

Mirror of the reference's `load_points=2` start of a scene (run/train_ft.py:687-770): data/scannet_ft_dataset.py:616-647
`load_init_depth_points` (back-projection + per-frame `construct_vox_points_xyz`), the range crop, `construct_vox_points_closest`, `nearest_view`
(train_ft.py:48-57), the regrouping by view and `MvsPointsModel.query_embedding` (homo_warp_nongrid + extract_from_2d_grid + the `dir` branch).
The reference's FeatureNet and premlp run on the device too (mvs_init.MvsInit, csrc/featnet.hip): pass one as `init_net` and the embedding is the
checkpoint's; without it the caller may still hand in `feature_maps` of their own.

The MVS start (`load_points=0`, run/train_ft.py:104-190) is `init_cloud_from_mvs_depth`; for the synthetic scenes it also runs the visual-hull masking
of `mvs_utils.alpha_masking` (`alpha_masking`, `AlphaMasks`, `visual_hull_select`) and the occlusion test of `homo_warp_nongrid_occ`
(`point_occlusion`), both in csrc/hull.hip.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import HnrError

OVERFLOW = 1          # HNR_CLOUD_OVERFLOW


def _host_f32(a, shape, name):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    if a.size != int(np.prod(shape)):
        raise HnrError("%s must hold %s values, got shape %s" % (name, "x".join(str(s) for s in shape), a.shape))
    return a.reshape(shape)


def _cf(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


class DepthFusion:
    """Fuses depth frames into one cloud [n,3] without a host read per frame.

    `intrinsic` is the fp32 depth intrinsic [3,3] (or the [4,4] file of a ScanNet export); its inverse is taken on the CPU in fp32, as the
    reference does (scannet_ft_dataset.py:624).  `.add(depth, c2w)` queues one frame: depth [H,W] uint16 (raw, divided by `depth_div`) or float32
    (metres) -- a host array is uploaded, a GPU tensor is used in place.  torch has no uint16 arithmetic, so raw depth travels as torch.int16 with
    the uint16 bit pattern: EVERY int16 tensor is read as uint16 (a negative value v means 65536 + v); genuinely signed data must be converted to
    float32 metres by the caller.  `.points()` does the one host read.

    Deliberately different from the reference: a frame without a valid depth pixel appends nothing (the reference raises: torch.min of an empty
    tensor at mvs_utils.py:507)."""

    def __init__(self, capacity, device, intrinsic, frame_vox_res=100, depth_div=1000., depth_min=0.3, depth_max=8.0):
        if int(capacity) < 1:
            raise HnrError("DepthFusion: capacity must be at least 1")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise HnrError("DepthFusion: device must be a GPU (the HIP path has no CPU fallback)")
        K = _host_f32(np.asarray(intrinsic, dtype=np.float32)[:3, :3], (3, 3), "intrinsic")
        self.Ki = np.ascontiguousarray(torch.inverse(torch.from_numpy(K)).numpy())
        self.capacity, self.frame_vox_res = int(capacity), int(frame_vox_res)
        self.depth_div, self.depth_min, self.depth_max = float(depth_div), float(depth_min), float(depth_max)
        self.cloud = torch.empty((self.capacity, 3), dtype=torch.float32, device=self.device)
        self.count = torch.zeros((1,), dtype=torch.int64, device=self.device)
        self.status = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self._scratch, self._shape = None, None
        self.frames = 0

    def add(self, depth, c2w):
        if not isinstance(depth, torch.Tensor):
            d = np.asarray(depth)
            if d.dtype == np.uint16:                       # torch has no uint16 arithmetic: the bytes travel as int16, the kernel reads uint16
                depth = torch.from_numpy(np.ascontiguousarray(d).view(np.int16))
            else:
                depth = torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32))
        if depth.dim() != 2:
            raise HnrError("DepthFusion.add: depth must be [H,W]")
        if depth.dtype in (torch.int16, getattr(torch, "uint16", torch.int16)):
            u16 = 1
        elif depth.dtype == torch.float32:
            u16 = 0
        else:
            raise HnrError("DepthFusion.add: depth must be uint16 (raw) or float32 (metres), got %s" % depth.dtype)
        depth = depth.to(self.device).contiguous()
        H, W = int(depth.shape[0]), int(depth.shape[1])
        if self._shape != (H, W):
            self._scratch = _lib.scratch("hnr_depth_fuse_scratch_bytes", H, W, device=self.device, what="DepthFusion.add: unsupported frame size %dx%d" % (H, W))
            self._shape = (H, W)
        M = _host_f32(c2w, (4, 4), "c2w")
        _lib.call("hnr_depth_fuse_frame", depth, u16, H, W, _cf(self.Ki), _cf(M), self.depth_div, self.depth_min, self.depth_max, self.frame_vox_res,
                  self.cloud, self.capacity, self.count, self.status, self._scratch, int(self._scratch.numel()), _lib.STREAM)
        self.frames += 1
        return self

    def points(self):
        n, st = int(self.count.item()), int(self.status.item())
        if (st & OVERFLOW) or n > self.capacity:
            raise HnrError("DepthFusion: the fused cloud needs capacity %d, the buffer holds %d" % (n, self.capacity))
        return self.cloud[:n]


def range_crop(xyz, ranges, count=None):
    """xyz [n,3] -> (buffer [n,3], device count [1] int64): the points with ranges[:3] <= p <= ranges[3:], in order (train_ft.py:713-716).
    `count` (device int64 [1]) limits the input to xyz[:count] without a host read.  ranges[0] <= -99 keeps everything."""
    xyz = _lib.require_gpu(xyz, "xyz", torch.float32)
    n, dev = int(xyz.shape[0]), xyz.device
    out = torch.empty_like(xyz)
    n_out = torch.zeros((1,), dtype=torch.int64, device=dev)
    if n == 0:
        return out, n_out
    if count is None:
        count = torch.full((1,), n, dtype=torch.int64, device=dev)
    r = _host_f32(ranges, (6,), "ranges")
    scratch = _lib.scratch("hnr_range_crop_scratch_bytes", n, device=dev, what="range_crop: too many points (%d)" % n)
    _lib.call("hnr_range_crop", xyz, count, n, _cf(r), out, n_out, scratch, scratch.numel(), _lib.STREAM)
    return out, n_out


def nearest_view_ids(campos, raydir, xyz):
    """int32 [N]: the camera of every point (hnr_nearest_view)."""
    xyz = _lib.require_gpu(xyz, "xyz", torch.float32).reshape(-1, 3)
    campos = _lib.require_gpu(campos, "campos", torch.float32).reshape(-1, 3)
    raydir = _lib.require_gpu(raydir, "raydir", torch.float32).reshape(-1, 3)
    if campos.shape != raydir.shape or campos.shape[0] == 0:
        raise HnrError("nearest_view: campos and raydir must both be [M,3], M > 0")
    out = torch.empty((xyz.shape[0],), dtype=torch.int32, device=xyz.device)
    if xyz.shape[0] > 0:
        _lib.call("hnr_nearest_view", xyz, int(xyz.shape[0]), campos, raydir, int(campos.shape[0]), out, _lib.STREAM)
    return out


def nearest_view(campos, raydir, xyz, id_list=None):
    """The reference's signature (train_ft.py:48): [N,1] int64 camera index per point; `id_list` is unused there too."""
    return nearest_view_ids(campos, raydir, xyz).long().view(-1, 1)


def cam_pos_cam(c2w, w2c):
    """(c2w[:,3] @ w2c.T)[:3] in fp32 on the CPU, as mvs_points_model.py:242-244 forms it: nearly, not exactly, zero."""
    c2w, w2c = torch.from_numpy(_host_f32(c2w, (4, 4), "c2w")), torch.from_numpy(_host_f32(w2c, (4, 4), "w2c"))
    return np.ascontiguousarray((c2w[:, 3][None] @ w2c.t())[0, :3].numpy())


def point_view_attrs(xyz, w2c, c2w, cpc, intrinsic, H, W, feat=None, want_dir=True, want_mask=True, visible=None):
    """hnr_point_view_attrs: (features [n,C] or None, dir [n,3] or None, mask [n] uint8 or None) of world points seen from one view.
    visible [n] uint8 (point_occlusion's flags, hnr_point_view_attrs_vis): where it is 0 the point counts as outside the frame."""
    xyz = _lib.require_gpu(xyz, "xyz", torch.float32).reshape(-1, 3)
    n, dev = int(xyz.shape[0]), xyz.device
    C = Hl = Wl = 0
    out_f = None
    if feat is not None:
        feat = _lib.require_gpu(feat, "feature map", torch.float32)
        if feat.dim() != 3:
            raise HnrError("a feature map must be [C,Hl,Wl]")
        C, Hl, Wl = (int(s) for s in feat.shape)
        out_f = torch.empty((n, C), dtype=torch.float32, device=dev)
    out_d = torch.empty((n, 3), dtype=torch.float32, device=dev) if want_dir else None
    out_m = torch.empty((n,), dtype=torch.uint8, device=dev) if want_mask else None
    if visible is not None:
        visible = _lib.require_gpu(visible, "visible", torch.uint8).reshape(-1)
        if visible.shape[0] != n or visible.device != dev:
            raise HnrError("point_view_attrs: visible must hold one flag per point, on xyz's device")
    if n > 0:
        a = [_host_f32(w2c, (4, 4), "w2c"), _host_f32(c2w, (4, 4), "c2w"), _host_f32(cpc, (3,), "cam_pos_cam"), _host_f32(intrinsic, (3, 3), "intrinsic")]
        head = (xyz, n, _cf(a[0]), _cf(a[1]), _cf(a[2]), _cf(a[3]), int(H), int(W), feat, C, Hl, Wl)
        if visible is not None:
            _lib.call("hnr_point_view_attrs_vis", *head, visible, out_f, out_d, out_m, _lib.STREAM)
        else:
            _lib.call("hnr_point_view_attrs", *head, out_f, out_d, out_m, _lib.STREAM)
    return out_f, out_d, out_m


def query_point_attributes(xyz, image_chw, c2w, w2c, intrinsic, feature_maps=None, default_conf=-1, conf=None, occlusion=None):
    """World points [n,3] seen from one posed frame -> (features [1,n,sum C] or None, color [1,n,3], dir [1,n,3], conf [1,n,1]): what
    `query_embedding` returns at train_ft.py:760 before premlp.  image_chw [3,H,W] (or [1,3,H,W]); feature_maps: list of [C,Hl,Wl].
    conf [n]: the points' photometric confidence (the MVS start, train_ft.py:176-180), returned as [1,n,1] in place of the ones.
    occlusion: a tolerance (the reference's 0.1) runs point_occlusion over these points first -- `depth_occ = 1`, homo_warp_nongrid_occ -- and the
    hidden ones get zero colour and features; None: no test."""
    img = _lib.require_gpu(image_chw, "image_chw", torch.float32)
    img = img.reshape(img.shape[-3:]).contiguous()
    if img.shape[0] != 3:
        raise HnrError("image_chw must be [3,H,W]")
    H, W = int(img.shape[1]), int(img.shape[2])
    w2c = torch.inverse(torch.from_numpy(_host_f32(c2w, (4, 4), "c2w"))).numpy() if w2c is None else w2c
    cpc = cam_pos_cam(c2w, w2c)
    K = _host_f32(intrinsic, (3, 3), "intrinsic")
    vis = None
    if occlusion is not None and occlusion is not False and int(np.prod(xyz.shape[:-1])) > 0:
        vis = point_occlusion(xyz, w2c, K, H, W, float(occlusion))
    color, pdir, _ = point_view_attrs(xyz, w2c, c2w, cpc, K, H, W, feat=img, want_mask=False, visible=vis)
    feats = None
    if feature_maps:
        feats = torch.cat([point_view_attrs(xyz, w2c, c2w, cpc, K, H, W, feat=f.reshape(f.shape[-3:]), want_dir=False, want_mask=False, visible=vis)[0]
                           for f in feature_maps], dim=-1)[None]
    if conf is not None:
        conf = _lib.require_gpu(conf, "conf", torch.float32).reshape(-1)
        if conf.shape[0] != color.shape[0]:
            raise HnrError("query_point_attributes: conf must hold one value per point")
        return feats, color[None], pdir[None], conf.reshape(1, -1, 1).clone()
    return feats, color[None], pdir[None], point_conf(color.shape[0], default_conf, color.device)


def point_occlusion(xyz, w2c, intrinsic, H, W, tolerate=0.1):
    """hnr_point_occlusion: uint8 [n], 1 where a world point is inside the H x W frame of the view (w2c, intrinsic) and at most `tolerate` behind the
    nearest point of its pixel cell -- the mask `homo_warp_nongrid_occ` returns (mvs_utils.py:333-369) for the points of one view."""
    xyz = _lib.require_gpu(xyz, "xyz", torch.float32).reshape(-1, 3)
    n, dev = int(xyz.shape[0]), xyz.device
    vis = torch.empty((n,), dtype=torch.uint8, device=dev)
    if n == 0:
        return vis
    H, W = int(H), int(W)
    scratch = _lib.scratch("hnr_point_occlusion_scratch_bytes", H, W, device=dev,
                           what="point_occlusion: unsupported frame %dx%d (2 <= H, W <= 32768, H*W <= 2^24)" % (H, W))
    if not float(tolerate) >= 0.0:
        raise HnrError("point_occlusion: tolerate must not be negative")
    E, K = _host_f32(w2c, (4, 4), "w2c"), _host_f32(intrinsic, (3, 3), "intrinsic")
    _lib.call("hnr_point_occlusion", xyz, n, _cf(E), _cf(K), H, W, float(tolerate), vis, scratch, scratch.numel(), _lib.STREAM)
    return vis


def alpha_pack(alphas):
    """hnr_alpha_pack: alphas [M,H,W] fp32 on the GPU -> int32 [M,H,(W+31)//32], one bit per pixel (alpha > 0.1), as uint32 bit patterns."""
    alphas = _lib.require_gpu(alphas, "alphas", torch.float32)
    if alphas.dim() != 3 or alphas.numel() == 0:
        raise HnrError("alpha_pack: alphas must be [M,H,W], got %s" % (tuple(alphas.shape),))
    M, H, W = (int(v) for v in alphas.shape)
    if M > 65535 or H > 32768 or W > 32768:
        raise HnrError("alpha_pack: alphas %s outside M <= 65535, H, W <= 32768" % (tuple(alphas.shape),))
    bits = torch.empty((M, H, (W + 31) // 32), dtype=torch.int32, device=alphas.device)
    _lib.call("hnr_alpha_pack", alphas, M, H, W, bits, _lib.STREAM)
    return bits


def _check_alphas(alphas, intrinsics, w2cs):
    """Host-side validation of a scene's silhouettes: (alphas [M,H,W] -- one tensor or array --, K [M,3,3], E [M,4,4]).  Every message names `alphas`."""
    from .geo_filter import _host_mats
    if isinstance(alphas, (list, tuple)):
        if not alphas or not all(isinstance(a, (torch.Tensor, np.ndarray)) for a in alphas):
            raise HnrError("alphas must be a list of [1,H,W] maps or one [M,H,W] tensor or array")
        if any(a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[0] != 1) for a in alphas) or len({tuple(a.shape[-2:]) for a in alphas}) != 1:
            raise HnrError("alphas: every map must be [1,H,W] (or [H,W]) of one size, got %s" % sorted({tuple(a.shape) for a in alphas}))
        if all(isinstance(a, torch.Tensor) for a in alphas) and len({a.device for a in alphas}) == 1:
            alphas = torch.stack([a.detach().reshape(a.shape[-2:]) for a in alphas])
        else:
            alphas = np.stack([np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).reshape(a.shape[-2:]) for a in alphas])
    if not isinstance(alphas, (torch.Tensor, np.ndarray)) or alphas.ndim != 3 or 0 in alphas.shape:
        raise HnrError("alphas must be a list of [1,H,W] maps or one [M,H,W] tensor or array, got %s"
                       % (tuple(alphas.shape) if hasattr(alphas, "shape") else type(alphas).__name__,))
    try:
        K, E = _host_mats(intrinsics, 3, "alphas: intrinsics"), _host_mats(w2cs, 4, "alphas: w2cs")
    except (TypeError, ValueError, AttributeError) as e:
        raise HnrError("alphas: intrinsics must be M [3,3] and w2cs M [4,4] matrices (%s)" % e)
    if K.shape[0] != alphas.shape[0] or E.shape[0] != alphas.shape[0]:
        raise HnrError("alphas: %d maps but %d intrinsics and %d w2cs" % (alphas.shape[0], K.shape[0], E.shape[0]))
    return alphas, K, E


def _pack_on(alphas, device):
    """validated alphas [M,H,W] (host or device) -> the packed bits on `device`: one copy, one launch"""
    if isinstance(alphas, np.ndarray):
        alphas = torch.from_numpy(np.ascontiguousarray(alphas, dtype=np.float32))
    return alpha_pack(alphas.detach().to(device=device, dtype=torch.float32).contiguous())


class AlphaMasks:
    """The silhouettes of a synthetic scene for visual_hull_select / alpha_masking, kept for reuse: `.bits` [M,H,Wp] (hnr_alpha_pack) and `.cams`
    [M,21] (rows 0..2 of w2c, then K) on the device.  alphas: a list of [1,H,W] (dataset.alphas) or one [M,H,W], tensors or arrays, values >= -0.9
    (dataset alphas are in [0, 1]); intrinsics: M x [3,3]; w2cs: M x [4,4].  Host alphas cross to the device once, as one copy."""

    def __init__(self, alphas, intrinsics, w2cs, device):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise HnrError("AlphaMasks: alphas go to a GPU (the HIP path has no CPU fallback), got device=%s" % dev)
        alphas, K, E = _check_alphas(alphas, intrinsics, w2cs)
        self.M, self.H, self.W = (int(v) for v in alphas.shape)
        self.device = dev
        self.bits = _pack_on(alphas, dev)
        self.cams = torch.from_numpy(np.ascontiguousarray(np.concatenate([E[:, :3, :].reshape(self.M, 12), K.reshape(self.M, 9)], axis=1))).to(dev)


def _near_far_pair(near_far, what):
    """(near - 1, far) as the reference compares them: the difference formed in double, both rounded to fp32."""
    if near_far is None:
        return None
    a = np.asarray(near_far.detach().cpu().numpy() if isinstance(near_far, torch.Tensor) else near_far, dtype=np.float64).reshape(-1)
    if a.size != 2:
        raise HnrError("%s: near_far must be a pair (near, far), got %d values" % (what, a.size))
    return np.ascontiguousarray(np.array([a[0] - 1.0, a[1]], dtype=np.float32))


def _range_mask_of(opt):
    return opt is not None and (getattr(opt, "alpha_range", 0) > 0 or getattr(opt, "inall_img", 1) == 0)


def visual_hull_select(xyz, masks, near_far=None, range_mask=False, conf=None, view=None, capacity=None, want_mask=True, compact=True):
    """hnr_visual_hull_select.  xyz [n,3] (n > 0) on the GPU, masks: an AlphaMasks there; near_far: (near, far) or None; conf [n] fp32 / view [n] int32:
    carried along.  Returns dict(mask [n] uint8 or None, xyz [cap,3], conf [cap] or None, view [cap] or None, count [1] int64, status [1] int32 -- all on
    the device -- and capacity).  Nothing is read back.  capacity None: n rows, which cannot overflow; compact=False: the mask alone."""
    xyz = _lib.require_gpu(xyz, "xyz", torch.float32).reshape(-1, 3)
    n, dev = int(xyz.shape[0]), xyz.device
    if not isinstance(masks, AlphaMasks) or masks.device != dev:
        raise HnrError("visual_hull_select: masks must be an AlphaMasks on xyz's device")
    if n == 0:
        raise HnrError("visual_hull_select: no point")
    nf = _near_far_pair(near_far, "visual_hull_select")
    cap = n if capacity is None else int(capacity)
    if cap < 0:
        raise HnrError("visual_hull_select: capacity must not be negative")
    for a, name, dt in ((conf, "conf", torch.float32), (view, "view", torch.int32)):
        if a is not None and (not isinstance(a, torch.Tensor) or not a.is_cuda or a.dtype != dt or a.numel() != n or a.device != dev):
            raise HnrError("visual_hull_select: %s must be [n] %s on xyz's device" % (name, dt))
    conf = None if conf is None else conf.reshape(-1).contiguous()
    view = None if view is None else view.reshape(-1).contiguous()
    rows = max(cap, 1)
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    out = dict(mask=e((n,), torch.uint8) if want_mask else None, xyz=e((rows, 3), torch.float32) if compact else None,
               conf=e((rows,), torch.float32) if compact and conf is not None else None, view=e((rows,), torch.int32) if compact and view is not None else None,
               count=torch.zeros((1,), dtype=torch.int64, device=dev), status=torch.zeros((1,), dtype=torch.int32, device=dev), capacity=cap)
    scratch = _lib.scratch("hnr_visual_hull_select_scratch_bytes", n, device=dev, what="visual_hull_select: too many points (%d)" % n)
    _lib.call("hnr_visual_hull_select", xyz, conf, view, n, masks.bits, masks.cams, masks.M, masks.H, masks.W, None if nf is None else _cf(nf),
              1 if range_mask else 0, out["mask"], out["xyz"], out["conf"], out["view"], cap, out["count"], out["status"], scratch, scratch.numel(),
              _lib.STREAM)
    return out


def alpha_masking(points, alphas, intrinsics, c2ws, w2cs, near_far, opt=None):
    """The reference's signature (mvs_utils.py:573) and result: bool [N], true where a point projects into every silhouette (and lies inside
    near - 1 .. far when near_far is given).  points [N,3+] on the GPU; alphas: a list of [1,H,W] or one [M,H,W] (tensors or arrays; they cross to the
    device once) or an AlphaMasks built earlier (intrinsics and w2cs are then unused); c2ws is accepted and unused, as in the reference.
    opt.alpha_range > 0 or opt.inall_img == 0 turns on the range mask: a point outside a frame passes that view."""
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise HnrError("alpha_masking: points must be a tensor on the GPU (the HIP path has no CPU fallback)")
    if points.dim() != 2 or points.shape[1] < 3 or points.dtype != torch.float32:
        raise HnrError("alpha_masking: points must be float32 [N,3], got %s %s" % (points.dtype, tuple(points.shape)))
    nf = _near_far_pair(near_far, "alpha_masking")
    masks = alphas if isinstance(alphas, AlphaMasks) else AlphaMasks(alphas, intrinsics, w2cs, points.device)
    if points.shape[0] == 0:
        return torch.zeros((0,), dtype=torch.bool, device=points.device)
    out = visual_hull_select(points[:, :3].contiguous(), masks, near_far=None if nf is None else near_far, range_mask=_range_mask_of(opt), compact=False)
    return out["mask"].bool()


def point_conf(n, default_conf, device):
    """[1,n,1]: ones (query_embedding's `point_conf` branch without a photometric confidence), times default_conf when 0 < default_conf < 1
    (train_ft.py:761)."""
    conf = torch.ones((1, n, 1), dtype=torch.float32, device=device)
    return conf * default_conf if 0 < default_conf < 1.0 else conf


def group_by_view(view_ids):
    """Stable grouping (hnr_sort_rows_by_key): (perm [N] int64, sorted ids [N] int32) -- ascending view id, the original order inside a view
    (train_ft.py:741-743: one boolean-mask pass per used view)."""
    keys = _lib.require_gpu(view_ids, "view_ids", torch.int32).reshape(-1)
    n, dev = int(keys.shape[0]), keys.device
    ks, perm = torch.empty_like(keys), torch.empty_like(keys)
    if n > 0:
        scratch = _lib.scratch("hnr_sort_rows_scratch_bytes", n, device=dev)
        _lib.call("hnr_sort_rows_by_key", keys, n, ks, perm, scratch, scratch.numel(), _lib.STREAM)
    return perm.long(), ks


def view_segments(sorted_ids):
    """[(view id, start, end)] of a sorted id array (host)."""
    ids = np.asarray(sorted_ids)
    if ids.size == 0:
        return []
    cut = np.flatnonzero(np.diff(ids)) + 1
    starts, ends = np.concatenate([[0], cut]), np.concatenate([cut, [ids.size]])
    return [(int(ids[s]), int(s), int(e)) for s, e in zip(starts, ends)]


def init_cloud_from_depth(frames, opt, campos, camdir, view_frame, capacity=None, frame_vox_res=100, device=None, init_net=None):
    """run/train_ft.py:687-770 for `load_points=2`.

    frames: iterable of (depth [H,W], c2w [4,4]) -- every depth frame of the scan; opt.depth_intrinsic is their intrinsic.  campos / camdir [M,3]: the
    training cameras (`get_campos_ray`).  view_frame(view_id) -> dict(image [3,H,W], c2w, intrinsic[, feature_maps]) for a used training view.
    Returns dict(xyz [N,3], embedding [1,N,C], color [1,N,3], dir [1,N,3], conf [1,N,1], view_of_point [N] int64): the arguments of
    NeuralPoints.set_points, points grouped by view in ascending view id.  Without feature maps the embedding is
    cloud_io.init_point_features(opt.feature_init_method).

    init_net: an mvs_init.MvsInit holding the init checkpoint.  view_frame then needs to return only image, c2w and intrinsic: the image pyramid of
    each used view is computed once and the embedding is init_net.embed_points' (train_ft.py:759-760); xyz, color, dir, conf and view_of_point are what
    the call without init_net returns.

    capacity: points the fused cloud may hold (12 bytes each), allocated up front.  The default is the frames' upper bound
    len(frames) * min(H*W, (frame_vox_res + 1)^3), CAPPED at 2^24 points (192 MiB).  A long scan can need more: the overflow is only known once every
    frame has been fused, and the HnrError raised then names the capacity to pass on the next call."""
    from . import cloud_io, voxel
    if getattr(opt, "resample_pnts", 0) > 0:
        raise HnrError("init_cloud_from_depth: opt.resample_pnts > 0 is not implemented")
    campos = _lib.require_gpu(campos, "campos", torch.float32)
    dev = campos.device if device is None else torch.device(device)
    frames = list(frames)
    if not frames:
        raise HnrError("init_cloud_from_depth: no depth frame")
    if capacity is None:
        h, w = np.shape(frames[0][0])[-2:]
        per = h * w if frame_vox_res <= 0 else min(h * w, (frame_vox_res + 1) ** 3)
        capacity = min(len(frames) * per, 1 << 24)
    fus = DepthFusion(capacity, dev, getattr(opt, "depth_intrinsic"), frame_vox_res=frame_vox_res)
    for depth, c2w in frames:
        fus.add(depth, c2w)
    pts = fus.points()                                                      # the one host read of the fusion; raises on overflow before anything else is allocated
    ranges = [float(r) for r in getattr(opt, "ranges", [-100.0] * 6)]
    if ranges[0] > -99.0 and pts.shape[0] > 0:
        buf, cnt = range_crop(pts, ranges)                                  # sized by the fused count, not by the capacity
        pts = buf[:int(cnt.item())]
    if pts.shape[0] == 0:
        raise HnrError("init_cloud_from_depth: no point survives the depth range and opt.ranges")
    if getattr(opt, "vox_res", 0) > 0:
        _, _, min_idx = voxel.construct_vox_points_closest(pts.contiguous(), opt.vox_res)
        pts = pts[min_idx]
    cam_ind = nearest_view_ids(campos, camdir, pts)
    perm, sorted_ids = group_by_view(cam_ind)
    xyz = pts[perm].contiguous()
    segs = view_segments(sorted_ids.cpu().numpy())
    colors, dirs, confs, feats = [], [], [], []
    for vid, s, e in segs:
        fr = view_frame(vid)
        if init_net is not None:
            f, c, d, cf = init_net.embed_points(xyz[s:e], fr["image"], fr["c2w"], fr.get("w2c"), fr["intrinsic"], getattr(opt, "default_conf", -1))
            colors.append(c); dirs.append(d); confs.append(cf); feats.append(f)
            continue
        f, c, d, cf = query_point_attributes(xyz[s:e], fr["image"], fr["c2w"], fr.get("w2c"), fr["intrinsic"], fr.get("feature_maps"),
                                             getattr(opt, "default_conf", -1))
        colors.append(c); dirs.append(d); confs.append(cf); feats.append(f)
    if any(f is None for f in feats):
        if not all(f is None for f in feats):
            raise HnrError("init_cloud_from_depth: view_frame must return feature_maps for every view or for none")
        emb, _ = cloud_io.init_point_features(xyz, opt.point_features_dim, opt.feature_init_method, xyz.device, opt.point_features_dim)
    else:
        emb = torch.cat(feats, dim=1)
    return dict(xyz=xyz, embedding=emb, color=torch.cat(colors, dim=1), dir=torch.cat(dirs, dim=1), conf=torch.cat(confs, dim=1),
                view_of_point=sorted_ids.long())


def _alpha_masks_of(alphas, alpha_cameras, what):
    """Validation of the `alphas` / `alpha_cameras` pair on the host, before anything else: an AlphaMasks, or the checked (alphas, K, E)."""
    if isinstance(alphas, AlphaMasks):
        return alphas
    if isinstance(alpha_cameras, dict):
        alpha_cameras = (alpha_cameras.get("intrinsics"), alpha_cameras.get("w2cs"))
    if not isinstance(alphas, (list, tuple, torch.Tensor, np.ndarray)):
        raise HnrError("%s: alphas must be a list of [1,H,W] maps, one [M,H,W] tensor or array, or a cloud_init.AlphaMasks" % what)
    if not isinstance(alpha_cameras, (list, tuple)) or len(alpha_cameras) != 2 or alpha_cameras[0] is None or alpha_cameras[1] is None:
        _check_alphas(alphas, [np.eye(3)] * len(alphas), [np.eye(4)] * len(alphas))           # a malformed `alphas` is the first complaint
        raise HnrError("%s: alphas need alpha_cameras=(intrinsics, w2cs) of the views the alphas belong to (dataset.intrinsics, dataset.world2cams)" % what)
    return _check_alphas(alphas, alpha_cameras[0], alpha_cameras[1])


def init_cloud_from_mvs_depth(views, opt, init_net=None, spacemin=None, spacemax=None, alphas=None, capacity=None, alpha_cameras=None, near_far=None,
                              occlusion=None):
    """`gen_points_filter_embeddings` after `gen_points` (run/train_ft.py:104-190) for `load_points=0`, `manual_depth_view=1`: the initial cloud from
    per-view depth and confidence maps -- the pretrained MVSNet's (mvs_depth.depth_views returns exactly these `views`), or any other estimator's.

    views: list of dict(cam_xyz [H,W,3] -- the camera-space point of every pixel, z = depth -- or depth [H,W] (cam_xyz is then K^-1 (x d, y d, d),
    what gen_points hands over), confidence [H,W], points_mask [H,W] bool (optional: all true), intrinsic [3,3], w2c [4,4], c2w [4,4] (optional: the
    fp32 inverse of w2c), image [3,H,W][, feature_maps]); the maps on the GPU.  opt: depth_conf_thresh, geo_cnsst_num, ranges, default_conf, vox_res
    (and the options of init_cloud_from_depth's last stage).  spacemin / spacemax [3]: the dataset's crop (train_ft.py:144-149).
    Stages: geo_filter.filter_views (ONE host read), the crop (folded into the filter's range mask: both are per-point comparisons), then
    voxel.construct_vox_points_closest -- the cloud's points are the voxel CENTROIDS, view and confidence those of the voxel's picked point, as at
    train_ft.py:164-166 -- the regrouping by source view (`points_vid`, not the nearest camera) and, per view, init_net.embed_points or
    query_point_attributes with the filtered confidence.
    Returns the dict init_cloud_from_depth returns; conf [1,N,1] is the filtered photometric confidence.

    The synthetic scenes (dev_scripts/w_n360): alphas -- dataset.alphas, a list of [1,H,W] or one [M,H,W], or an AlphaMasks -- with
    alpha_cameras=(dataset.intrinsics, dataset.world2cams) turns on the visual-hull masking of train_ft.py:152-158 after the filter and the crop
    (hnr_visual_hull_select on xyz, confidence and view; one more host read, the survivor count); near_far = dataset.near_far is used as the
    reference uses it, only when opt.ranges[0] < -90 and there is no spacemin.  opt.depth_occ > 0 needs occlusion=True (or a tolerance; True: the
    reference's 0.1): every view's points go through point_occlusion before they are embedded."""
    from . import cloud_io, geo_filter as gf, mvs_init, voxel
    hull = None if alphas is None else _alpha_masks_of(alphas, alpha_cameras, "init_cloud_from_mvs_depth")
    if alphas is not None:
        _near_far_pair(near_far, "init_cloud_from_mvs_depth: alphas")
    tolerate = mvs_init.occlusion_tolerance(opt, occlusion, "init_cloud_from_mvs_depth")
    gf.check_options(opt, "init_cloud_from_mvs_depth")
    views = list(views)
    if not views:
        raise HnrError("init_cloud_from_mvs_depth: no view")
    cams, confs, masks = [], [], []
    for v in views:
        c = v.get("cam_xyz")
        if c is None:
            d = _lib.require_gpu(v["depth"], "depth", torch.float32)
            Ki = torch.inverse(torch.from_numpy(_host_f32(v["intrinsic"], (3, 3), "intrinsic"))).to(d.device)
            py, px = torch.meshgrid(torch.arange(d.shape[0], device=d.device), torch.arange(d.shape[1], device=d.device), indexing="ij")
            c = (Ki @ (torch.stack([px.reshape(-1), py.reshape(-1), torch.ones_like(px.reshape(-1))], dim=0) * d.reshape(-1))).t().reshape(d.shape + (3,))
        c = _lib.require_gpu(c, "cam_xyz", torch.float32)
        c = c.reshape(c.shape[-3:])
        cams.append(c)
        confs.append(_lib.require_gpu(v["confidence"], "confidence", torch.float32).reshape(c.shape[:2]))
        m = v.get("points_mask")
        masks.append(torch.ones(c.shape[:2], dtype=torch.bool, device=c.device) if m is None else m.reshape(c.shape[:2]))
    dev = cams[0].device
    ranges = [float(r) for r in getattr(opt, "ranges", [-100.0] * 6)]
    if (spacemin is None) != (spacemax is None):
        raise HnrError("init_cloud_from_mvs_depth: spacemin and spacemax come together")
    if spacemin is not None:
        lo, hi = _host_f32(spacemin, (3,), "spacemin"), _host_f32(spacemax, (3,), "spacemax")
        if ranges[0] > -99.0:                                              # x >= a and x >= b  <=>  x >= max(a, b): exact
            lo, hi = np.maximum(lo, np.asarray(ranges[:3], np.float32)), np.minimum(hi, np.asarray(ranges[3:], np.float32))
        if lo[0] <= -99.0:
            raise HnrError("init_cloud_from_mvs_depth: spacemin[0] <= -99 collides with the `keep everything` value of opt.ranges")
        ranges = [float(r) for r in np.concatenate([lo, hi])]
    tab = gf.CameraTables([v["intrinsic"] for v in views], [v["w2c"] for v in views], dev)
    flt = gf.filter_views(torch.stack(cams), torch.stack(confs), torch.stack(masks), tab, opt, ranges=ranges, capacity=capacity)
    pts, conf, vid = flt["world"], flt["conf"], flt["view"]
    if pts.shape[0] == 0:
        raise HnrError("init_cloud_from_mvs_depth: no point survives the filter")
    if hull is not None:
        if not isinstance(hull, AlphaMasks):
            hull = AlphaMasks(hull[0], hull[1], hull[2], dev)
        use_nf = near_far is not None and float(getattr(opt, "ranges", [-100.0])[0]) < -90.0 and spacemin is None             # train_ft.py:155
        sel = visual_hull_select(pts.contiguous(), hull, near_far=near_far if use_nf else None, range_mask=_range_mask_of(opt), conf=conf.contiguous(),
                                 view=vid.contiguous(), want_mask=False)
        n = int(sel["count"].item())                                       # the one further host read
        if n == 0:
            raise HnrError("init_cloud_from_mvs_depth: no point survives the alphas (visual-hull masking)")
        pts, conf, vid = sel["xyz"][:n], sel["conf"][:n], sel["view"][:n]
    if getattr(opt, "vox_res", 0) > 0:
        pts, _, min_idx = voxel.construct_vox_points_closest(pts.contiguous(), opt.vox_res)
        conf, vid = conf[min_idx], vid[min_idx]
    perm, sorted_ids = group_by_view(vid.contiguous())
    xyz, conf = pts[perm].contiguous(), conf[perm].contiguous()
    colors, dirs, feats = [], [], []
    for v, s, e in view_segments(sorted_ids.cpu().numpy()):
        fr = views[v]
        w2c = tab.host["E"][v]
        c2w = fr.get("c2w")
        c2w = tab.host["Einv"][v] if c2w is None else c2w
        if init_net is not None:
            f, c, d, _ = init_net.embed_points(xyz[s:e], fr["image"], c2w, w2c, fr["intrinsic"], conf=conf[s:e],
                                               occlusion=False if tolerate is None else tolerate)
        else:
            f, c, d, _ = query_point_attributes(xyz[s:e], fr["image"], c2w, w2c, fr["intrinsic"], fr.get("feature_maps"), conf=conf[s:e], occlusion=tolerate)
        colors.append(c); dirs.append(d); feats.append(f)
    if any(f is None for f in feats):
        if not all(f is None for f in feats):
            raise HnrError("init_cloud_from_mvs_depth: every view must come with feature_maps, or none")
        emb, _ = cloud_io.init_point_features(xyz, opt.point_features_dim, opt.feature_init_method, xyz.device, opt.point_features_dim)
    else:
        emb = torch.cat(feats, dim=1)
    return dict(xyz=xyz, embedding=emb, color=torch.cat(colors, dim=1), dir=torch.cat(dirs, dim=1), conf=conf.reshape(1, -1, 1),
                view_of_point=sorted_ids.long())
