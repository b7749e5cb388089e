"""The host-side blocks of one ray-batch call, built once: normalised inputs, the shared fields of hnr_render_params / hnr_train_params, the
thirteen outputs of hnr_render_outputs, the aligned workspace.  render.py (hnr_render_forward), train.py (hnr_render_train_forward / _backward) and
torch_ops.py (the same ABI behind TORCH_LIBRARY, and its fake shape functions) all call in here; hnr_train_weights' table stands next to its struct in
_lib.py.  What a route does differently -- which outputs it asks for, what it pre-fills, its memory threshold -- stays at the route."""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._lib import HnrError

_f32, _i32 = torch.float32, torch.int32
# hnr_render_outputs in struct order: (key of the result dict, struct field, shape in R / SR / K, dtype)
RAY_OUTPUTS = (("coarse_raycolor", "d_raycolor", ("R", 3), _f32), ("coarse_point_opacity", "d_opacity", ("R", "SR"), _f32),
               ("coarse_is_background", "d_is_background", ("R",), _f32), ("blend_weight", "d_blend_weight", ("R", "SR"), _f32),
               ("ray_mask", "d_ray_mask", ("R",), torch.int8), ("decoded", "d_decoded", ("R", "SR", 4), _f32),
               ("sample_pidx", "d_sample_pidx", ("R", "SR", "K"), _i32), ("sample_loc_w", "d_sample_loc_w", ("R", "SR", 3), _f32),
               ("ray_nsamp", "d_ray_nsamp", ("R",), _i32), ("counts", "d_counts", (_lib.NCOUNTS,), torch.int64), ("status", "d_status", (2,), _i32),
               ("weight", "d_weight", ("R", "SR", "K"), _f32), ("conf_coefficient", "d_conf_coefficient", ("R", "SR", "K"), _f32))
TRAIN_OUTPUTS = tuple(o[0] for o in RAY_OUTPUTS)
OPTIONAL_OUTPUTS = ("blend_weight", "weight", "conf_coefficient")         # a render passes NULL for those it does not want
FORWARD_OUTPUTS = tuple(k for k in TRAIN_OUTPUTS if k not in OPTIONAL_OUTPUTS)


class RayOutputs:
    """The output tensors of one call: `t` maps every key of RAY_OUTPUTS, in order, to its tensor or to None (an output the call does not want)."""

    def __init__(self, tensors):
        self.t, self._c = dict(zip(TRAIN_OUTPUTS, tensors)), None

    @classmethod
    def alloc(cls, R, SR, K, dev, blend=True, weights=True, empty=torch.empty):
        """Uninitialised tensors of the table's shapes; `empty`: the allocator (a fake shape function passes a fake tensor's new_empty)."""
        dims = dict(R=R, SR=SR, K=K)
        skip = (() if blend else OPTIONAL_OUTPUTS[:1]) + (() if weights else OPTIONAL_OUTPUTS[1:])
        return cls(None if key in skip else empty(tuple(dims.get(s, s) for s in shape), dtype=dt, device=dev) for key, _field, shape, dt in RAY_OUTPUTS)

    def struct(self, stage_events=None):
        """hnr_render_outputs over the tensors (built once per object: its tensors do not change after the first call)."""
        if self._c is None:
            self._c = _lib.RenderOutputs(*[_lib.ptr(t) for t in self.t.values()], None)
        self._c.stage_events = stage_events
        return self._c

    def as_dict(self):
        return dict(self.t)


def empty_slot_conf(cloud, R, SR, K):
    """conf_coefficient before the gather writes the filled slots: empty slots read point 0 in the reference (index clamp, neural_points.py:711)."""
    return cloud.conf[0].clamp(0.0001, 1.0).expand(R, SR, K).contiguous()


def fill_params(prm, R, SR, K, tmid, kernel_size, radius2, vsize_z, raydist_mode_unit, V, cap_samples, knn_order):
    """The fields hnr_render_params and hnr_train_params share; tmid [D] (one table for all rays) or [R, D]; cap_samples 0 / None: R * SR, the worst case."""
    prm.R, prm.SR, prm.K, prm.D = int(R), int(SR), int(K), int(tmid.shape[-1])
    prm.tmid_stride = 0 if tmid.dim() == 1 else int(tmid.shape[1])
    for i in range(3):
        prm.kernel_size[i] = int(kernel_size[i])
    prm.radius2, prm.vsize_z, prm.raydist_mode_unit = float(radius2), float(vsize_z), int(raydist_mode_unit)
    prm.V, prm.cap_samples, prm.knn_order = int(V), int(cap_samples) if cap_samples else prm.R * prm.SR, int(knn_order)
    return prm


def opt_scalars(opt, radius2):
    """(radius2, vsize_z, raydist_mode_unit) as every route hands them to the library: fp32-rounded floats and a 0 / 1 flag."""
    return float(np.float32(radius2)), float(np.float32(opt.vsize[2])), int(getattr(opt, "raydist_mode_unit", 0) > 0)


def fill_params_opt(prm, opt, R, K, tmid, radius2, V, cap_samples, knn_order):
    return fill_params(prm, R, opt.SR, K, tmid, opt.kernel_size, *opt_scalars(opt, radius2), V, cap_samples, knn_order)


WS_ALIGN = 256           # the library wants its workspace 256-byte aligned: every workspace tensor is this much longer than the bytes asked for


def train_workspace_bytes(prm):
    nbytes = int(_lib.lib().hnr_render_train_workspace_bytes(ctypes.byref(prm)))
    if nbytes < 0:
        raise HnrError("hnr_render_train_workspace_bytes: %s" % _lib.lib().hnr_last_error().decode("utf-8", "replace"))
    return nbytes


def workspace(nbytes, dev, reuse=None):
    """(uint8 tensor, aligned void* into it with `nbytes` behind it); `reuse`: a caller's tensor, taken when it is long enough."""
    ws = reuse if (reuse is not None and reuse.numel() >= nbytes + WS_ALIGN) else torch.empty((nbytes + WS_ALIGN,), dtype=torch.uint8, device=dev)
    return ws, ctypes.c_void_p(ws.data_ptr() + (-ws.data_ptr()) % 256)


def available_bytes(dev, capturing=False):
    """What an allocation can get: free device memory (not asked for under stream capture) + what torch's allocator holds unused."""
    free = (1 << 62) if capturing else torch.cuda.mem_get_info(dev)[0]
    return free + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)


class RayInputs(namedtuple("RayInputs", "raydir campos camrot bg_color c2w campos_nearest intrinsic images w2c frame_w")):
    """The camera group and the reference-view group (all None when the route leaves the views alone) as contiguous fp32 GPU tensors."""

    def camera(self, tmid):
        p = _lib.ptr
        return _lib.RenderCamera(p(self.campos), p(self.camrot), p(self.raydir), p(tmid), p(self.bg_color))


def ray_inputs(raydir, campos, camrot, bg_color, c2w_nearest=None, campos_nearest=None, intrinsic_nearest=None, images_nearest=None, w2c_nearest=None,
               frame_weight=None, fw_name="frame_weight", views=True, invert=True):
    """views=False: the view tensors (not the frame weights) are left alone.  images_nearest [V,H,W,3] or with a leading 1 (None: the route reads the views' feature map).
    w2c_nearest None: inverse(c2w_nearest), a 4x4 plumbing op (neural_points_volumetric_model.py:250) -- unless invert=False (no view is read)."""
    g = lambda t, name, *shape: _lib.require_gpu(t, name, torch.float32).reshape(*shape)
    cam = (g(raydir, "raydir", -1, 3), g(campos, "campos", 3), g(camrot, "camrotc2w", 3, 3), g(bg_color, "bg_color", 3))
    fw = None if frame_weight is None else g(frame_weight, fw_name, -1)
    if not views:
        return RayInputs(*cam, None, None, None, None, None, fw)
    c2w, camn, intr = g(c2w_nearest, "c2w_nearest", -1, 4, 4), g(campos_nearest, "campos_nearest", -1, 3), g(intrinsic_nearest, "intrinsic_nearest", 3, 3)
    img = None if images_nearest is None else _lib.require_gpu(images_nearest, "images_nearest", torch.float32)
    if img is not None and img.dim() == 5:
        img = img[0]
    w2c = None
    if w2c_nearest is not None:
        w2c = g(w2c_nearest, "w2c_nearest", -1, 4, 4)
    elif invert:
        w2c = torch.inverse(c2w).contiguous()
    return RayInputs(*cam, c2w, camn, intr, img, w2c, fw)
