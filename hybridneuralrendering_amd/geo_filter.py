"""The geometric-consistency filter of MVS depth maps, on the device (csrc/geo_filter.hip).

Mirror of the reference's `load_points=0`, `manual_depth_view=1` start of a scene between MVSNet's depth maps and the point embeddings:
models/mvs/filter_utils.py:157-297 (`filter_by_masks_gpu` with `check_geometric_consistency_gpu`, `reproject_with_depth_gpu`, `range_mask_torch`
and `reassign_conf`), called from run/train_ft.py:105-114.  The reference's Python double loop over the views becomes one launch
(hnr_geo_consistency) and one ordered compaction over all views (hnr_geo_filter_select); the depth maps never leave the device.
cloud_init.init_cloud_from_mvs_depth builds the initial cloud on top of it.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import HnrError

OVERFLOW = 1          # HNR_CLOUD_OVERFLOW


def _host_mats(items, k, name):
    """A list (or array) of V matrices [k,k] (or [1,k,k]) -> float32 [V,k,k] on the host.  Tensors on the GPU are stacked there and cross in one copy."""
    if isinstance(items, torch.Tensor):
        items = [items] if items.dim() == 2 else list(items)
    if isinstance(items, np.ndarray):
        items = [items] if items.ndim == 2 else list(items)
    items = list(items)
    if not items:
        raise HnrError("%s: no view" % name)
    if all(isinstance(m, torch.Tensor) for m in items):
        if len({(m.numel(), m.device) for m in items}) != 1:
            raise HnrError("%s: the views' matrices differ in size or device" % name)
        a = torch.stack([m.detach().reshape(-1) for m in items]).to(torch.float32).cpu().numpy()
    else:
        a = np.stack([np.asarray(m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else m, dtype=np.float32).reshape(-1) for m in items])
    if a.shape[1] != k * k:
        raise HnrError("%s must hold %dx%d matrices, got %d values per view" % (name, k, k, a.shape[1]))
    return np.ascontiguousarray(a.reshape(-1, k, k), dtype=np.float32)


class CameraTables:
    """K, K^-1 [V,3,3] and E (world to camera), E^-1 [V,4,4] on the device.  The inverses are taken in fp32 with torch on the CPU, one matrix at a
    time, as the reference forms them (torch.linalg.inv / torch.inverse of fp32 matrices, filter_utils.py:165-190, :282)."""

    def __init__(self, intrinsics, extrinsics, device):
        K, E = _host_mats(intrinsics, 3, "intrinsics"), _host_mats(extrinsics, 4, "extrinsics")
        if K.shape[0] != E.shape[0]:
            raise HnrError("intrinsics and extrinsics must describe the same views (%d and %d)" % (K.shape[0], E.shape[0]))
        inv = lambda a: np.stack([torch.inverse(torch.from_numpy(m)).numpy() for m in a])
        self.V = int(K.shape[0])
        self.host = dict(K=K, Kinv=inv(K), E=E, Einv=inv(E))
        self.K, self.Kinv, self.E, self.Einv = (torch.from_numpy(np.ascontiguousarray(self.host[n])).to(device) for n in ("K", "Kinv", "E", "Einv"))


def _tables(intrinsics, extrinsics, device):
    return intrinsics if isinstance(intrinsics, CameraTables) else CameraTables(intrinsics, extrinsics, device)


def geometric_consistency(depth, intrinsics, extrinsics=None):
    """depth [V,H,W] fp32 on the GPU; intrinsics [V,3,3] and extrinsics [V,4,4] (world to camera; host arrays or tensors), or a CameraTables.
    Returns (count [V,H,W] int32: the source views consistent with each pixel, depth_averaged [V,H,W]) -- hnr_geo_consistency."""
    depth = _lib.require_gpu(depth, "depth", torch.float32)
    if depth.dim() != 3:
        raise HnrError("geometric_consistency: depth must be [V,H,W]")
    V, H, W = (int(s) for s in depth.shape)
    tab = _tables(intrinsics, extrinsics, depth.device)
    if tab.V != V or tab.K.device != depth.device:
        raise HnrError("geometric_consistency: %d depth maps but %d cameras (or cameras on another device)" % (V, tab.V))
    count = torch.empty((V, H, W), dtype=torch.int32, device=depth.device)
    avg = torch.empty_like(depth)
    _lib.call("hnr_geo_consistency", depth, V, H, W, tab.K, tab.Kinv, tab.E, tab.Einv, count, avg, _lib.STREAM)
    return count, avg


def conf_table():
    """The ten factors of `reassign_conf` (filter_utils.py:294-297), k = 1..10, by the reference's own torch expression on the host."""
    return np.ascontiguousarray((1 - 1.0 / torch.pow(1.14869, torch.arange(1, 11, dtype=torch.int32))).numpy(), dtype=np.float32)


def select_points(cam_xyz, conf, points_mask, count, depth_avg, tables, conf_thresh, geo_cnsst_num, ranges, reassign=False, capacity=None):
    """hnr_geo_filter_select.  cam_xyz [V,H,W,3], conf [V,H,W] fp32, points_mask [V,H,W] uint8, count / depth_avg from geometric_consistency.
    Returns dict(world [cap,3], cam [cap,3], conf [cap], view [cap] int32, meta [V+1] int64 on the device: per-view counts, then the total,
    status [1] int32, capacity).  Nothing is read back here.  capacity None: V*H*W rows (32 bytes each), which cannot overflow."""
    cam_xyz = _lib.require_gpu(cam_xyz, "cam_xyz", torch.float32)
    dev = cam_xyz.device
    if cam_xyz.dim() != 4 or cam_xyz.shape[3] != 3:
        raise HnrError("select_points: cam_xyz must be [V,H,W,3]")
    V, H, W = (int(s) for s in cam_xyz.shape[:3])
    conf, avg = _lib.require_gpu(conf, "conf", torch.float32), _lib.require_gpu(depth_avg, "depth_avg", torch.float32)
    pm, count = _lib.require_gpu(points_mask, "points_mask", torch.uint8), _lib.require_gpu(count, "count", torch.int32)
    for a, name in ((conf, "conf"), (avg, "depth_avg"), (pm, "points_mask"), (count, "count")):
        if tuple(a.shape) != (V, H, W) or a.device != dev:
            raise HnrError("select_points: %s must be [%d,%d,%d] on cam_xyz's device" % (name, V, H, W))
    if tables.V != V or tables.Einv.device != dev:
        raise HnrError("select_points: the camera tables describe %d views on %s" % (tables.V, tables.Einv.device))
    cap = V * H * W if capacity is None else int(capacity)
    if cap < 0:
        raise HnrError("select_points: capacity must not be negative")
    r = np.ascontiguousarray(np.asarray(ranges, dtype=np.float32).reshape(-1))
    if r.size != 6:
        raise HnrError("select_points: ranges must hold 6 values")
    table = conf_table() if reassign else None
    rows = max(cap, 1)
    out = dict(world=torch.empty((rows, 3), dtype=torch.float32, device=dev), cam=torch.empty((rows, 3), dtype=torch.float32, device=dev),
               conf=torch.empty((rows,), dtype=torch.float32, device=dev), view=torch.empty((rows,), dtype=torch.int32, device=dev),
               meta=torch.zeros((V + 1,), dtype=torch.int64, device=dev), status=torch.zeros((1,), dtype=torch.int32, device=dev), capacity=cap)
    scratch = _lib.scratch("hnr_geo_filter_select_scratch_bytes", V, H, W, device=dev, what="select_points: unsupported shape V=%d, %dx%d" % (V, H, W))
    fp = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    _lib.call("hnr_geo_filter_select", cam_xyz, conf, pm, count, avg, V, H, W, tables.Einv, float(conf_thresh), int(geo_cnsst_num), fp(r), fp(table),
              out["world"], out["cam"], out["conf"], out["view"], cap, out["meta"], out["meta"][V:], out["status"], scratch, scratch.numel(), _lib.STREAM)
    return out


def check_options(opt, what="filter_by_masks_gpu"):
    """Raises HnrError for what is not built: manual_depth_view > 1, far_plane_shift."""
    if int(getattr(opt, "manual_depth_view", 1)) > 1:
        raise HnrError("%s: manual_depth_view > 1 (per-depth-hypothesis points without the geometric mask) is not implemented" % what)
    if getattr(opt, "far_plane_shift", None) is not None:
        raise HnrError("%s: far_plane_shift (background points on the far plane) is not implemented" % what)


def filter_views(cam_xyz, conf, points_mask, tables, opt, ranges=None, capacity=None):
    """The filter on stacked device tensors: cam_xyz [V,H,W,3], conf [V,H,W], points_mask [V,H,W] (bool or uint8).  Returns
    dict(world [n,3], cam [n,3], conf [n], view [n] int32, view_counts: list of V ints), views ascending, row-major pixels inside a view.
    ONE host read (the counts).  ranges: overrides opt.ranges."""
    check_options(opt, "filter_views")
    cam_xyz = _lib.require_gpu(cam_xyz, "cam_xyz", torch.float32)
    conf = _lib.require_gpu(conf, "confidence", torch.float32)
    if not isinstance(points_mask, torch.Tensor) or not points_mask.is_cuda:
        raise HnrError("points_mask must be a tensor on the GPU (the HIP path has no CPU fallback)")
    pm = points_mask.to(torch.uint8).contiguous()
    depth = cam_xyz[..., 2].contiguous()                                    # the one extraction of the depth planes
    count, avg = geometric_consistency(depth, tables)
    if ranges is None:
        ranges = [float(r) for r in getattr(opt, "ranges", [-100.0] * 6)]
    out = select_points(cam_xyz, conf, pm, count, avg, tables, float(opt.depth_conf_thresh), int(opt.geo_cnsst_num), ranges,
                        reassign=float(getattr(opt, "default_conf", -1)) > 1.0, capacity=capacity)
    meta = out["meta"].cpu().numpy()                                        # the one host read
    n = int(meta[-1])
    if n > out["capacity"]:
        raise HnrError("filter_views: the filtered cloud needs capacity %d, the buffers hold %d" % (n, out["capacity"]))
    return dict(world=out["world"][:n], cam=out["cam"][:n], conf=out["conf"][:n], view=out["view"][:n], view_counts=[int(c) for c in meta[:-1]],
                count=count, depth_avg=avg)


def filter_by_masks_gpu(cam_xyz_all, intrinsics_all, extrinsics_all, confidence_all, points_mask_all, opt, vis=False, return_w=False, cpu2gpu=False,
                        near_fars_all=None, capacity=None):
    """The reference's signature (filter_utils.py:222) and its three returned lists (xyz_cam_lst, xyz_world_lst, confidence_filtered_lst), one entry
    per view.  cam_xyz_all[v] [1,1,1,H,W,3], intrinsics_all[v] [1,3,3], extrinsics_all[v] [1,4,4], confidence_all[v] [1,1,H,W],
    points_mask_all[v] [1,1,H,W] bool; the maps on the GPU, the camera matrices anywhere (on the host they cost no transfer).  `vis`, `return_w` and
    `near_fars_all` are accepted and unused, as without far_plane_shift in the reference.  Raises HnrError for manual_depth_view > 1, far_plane_shift,
    num_each_depth != 1 and CPU tensors (cpu2gpu, the reference's host staging of long scans, included)."""
    check_options(opt)
    if cpu2gpu:
        raise HnrError("filter_by_masks_gpu: cpu2gpu (maps staged on the host) is not implemented: the maps stay on the device")
    if len(cam_xyz_all) == 0:
        raise HnrError("filter_by_masks_gpu: no view")
    shp = tuple(cam_xyz_all[0].shape)
    if len(shp) != 6 or shp[5] != 3 or shp[0] != 1 or shp[1] != 1:
        raise HnrError("filter_by_masks_gpu: cam_xyz must be [1,1,C,H,W,3], got %s" % (shp,))
    if shp[2] != 1:
        raise HnrError("filter_by_masks_gpu: num_each_depth != 1 (C = %d depth hypotheses per pixel) is not implemented" % shp[2])
    for name, lst in (("cam_xyz_all", cam_xyz_all), ("confidence_all", confidence_all), ("points_mask_all", points_mask_all)):
        for a in lst:
            if not isinstance(a, torch.Tensor) or not a.is_cuda:
                raise HnrError("filter_by_masks_gpu: %s must hold tensors on the GPU (the HIP path has no CPU fallback)" % name)
    H, W = shp[3], shp[4]
    V = len(cam_xyz_all)
    if not (len(intrinsics_all) == len(extrinsics_all) == len(confidence_all) == len(points_mask_all) == V):
        raise HnrError("filter_by_masks_gpu: every list must have one entry per view")
    dev = cam_xyz_all[0].device
    cam = torch.stack([c.to(torch.float32).reshape(H, W, 3) for c in cam_xyz_all])
    conf = torch.stack([c.to(torch.float32).reshape(H, W) for c in confidence_all])
    pm = torch.stack([m.reshape(H, W) for m in points_mask_all])
    out = filter_views(cam, conf, pm, CameraTables(intrinsics_all, extrinsics_all, dev), opt, capacity=capacity)
    cuts = np.concatenate([[0], np.cumsum(out["view_counts"])]).astype(np.int64)
    sl = [slice(int(cuts[v]), int(cuts[v + 1])) for v in range(V)]
    return [out["cam"][s] for s in sl], [out["world"][s] for s in sl], [out["conf"][s] for s in sl]
