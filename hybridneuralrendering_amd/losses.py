"""The loss terms of the shipped training configurations on the device (SURVEY 8f "next" row 2, second half).

Mirror of the enabled part of BaseRenderingModel.compute_losses (models/base_rendering_model.py:1060-1245; items from
dev_scripts/w_scannet_etf/scene241.sh:146-151): masked colour MSE on `coarse_raycolor` + zero-one regulariser on
`conf_coefficient`, value and both gradients from two small HIP kernels instead of masked_select copies and an autograd graph.
"""
import ctypes

import torch

from . import _lib
from ._lib import HnrError


def _loss_call(color, conf, gt, ray_mask, zero_epsilon, w_color, w_zero_one, frame_weight, conf_rows, want_grads=True):
    """One hnr_shipped_loss[_rows] launch pair: returns (out4, g_color, g_conf) -- all device tensors, nothing is read back."""
    L = _lib.lib()
    c = _lib.require_gpu(color.detach(), "coarse_raycolor", torch.float32).reshape(-1, 3)
    g = _lib.require_gpu(gt, "gt_image", torch.float32).reshape(-1, 3)
    m = _lib.require_gpu(ray_mask, "ray_mask").reshape(-1)
    if m.dtype != torch.int8:
        m = m.to(torch.int8)
    x = _lib.require_gpu(conf.detach(), "conf_coefficient", torch.float32).reshape(-1)
    if g.shape[0] != c.shape[0] or m.shape[0] != c.shape[0]:
        raise HnrError("shipped_loss: coarse_raycolor, gt_image and ray_mask disagree on the number of rays")
    R = int(c.shape[0])
    if conf_rows and (R == 0 or x.shape[0] % R):
        raise HnrError("shipped_loss: conf_rows needs conf_coefficient with one row per ray of the batch")
    dev = c.device
    out = torch.empty((4,), dtype=torch.float32, device=dev)
    g_c, g_x = (torch.empty_like(c), torch.empty_like(x)) if want_grads else (None, None)
    scratch = torch.empty((int(L.hnr_shipped_loss_scratch_bytes()),), dtype=torch.uint8, device=dev)
    p = _lib.ptr
    with torch.cuda.device(dev):
        if isinstance(frame_weight, torch.Tensor):
            # the item's scalar on the device (one float): read by the kernel, so a captured step replays with other values
            if not conf_rows:
                raise HnrError("shipped_loss: a device frame_weight needs conf_rows=True")
            fw = _lib.require_gpu(frame_weight, "frame_weight", torch.float32).reshape(-1)
            _lib.check(L.hnr_shipped_loss_rows_fw(p(c), p(g), p(m), R, p(x), int(x.shape[0] // R), float(zero_epsilon), float(w_color), float(w_zero_one),
                                                  p(fw), p(out), p(g_c) if want_grads else None, p(g_x) if want_grads else None, p(scratch),
                                                  _lib.stream()), "hnr_shipped_loss_rows_fw")
        elif conf_rows:
            _lib.check(L.hnr_shipped_loss_rows(p(c), p(g), p(m), R, p(x), int(x.shape[0] // R), float(zero_epsilon), float(w_color), float(w_zero_one),
                                               float(frame_weight), p(out), p(g_c) if want_grads else None, p(g_x) if want_grads else None, p(scratch),
                                               _lib.stream()), "hnr_shipped_loss_rows")
        else:
            _lib.check(L.hnr_shipped_loss(p(c), p(g), p(m), R, p(x), x.shape[0], float(zero_epsilon), float(w_color), float(w_zero_one),
                                          float(frame_weight), p(out), p(g_c) if want_grads else None, p(g_x) if want_grads else None, p(scratch),
                                          _lib.stream()), "hnr_shipped_loss")
    return out, g_c, g_x


class _ShippedLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, color, conf, gt, ray_mask, zero_epsilon, w_color, w_zero_one, frame_weight, conf_rows):
        out, g_c, g_x = _loss_call(color, conf, gt, ray_mask, zero_epsilon, w_color, w_zero_one, frame_weight, conf_rows)
        ctx.save_for_backward(g_c, g_x)
        ctx.shapes = (color.shape, conf.shape)
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, g_total, _g_out):
        g_c, g_x = ctx.saved_tensors
        cs, xs = ctx.shapes
        return (g_c * g_total).reshape(cs), (g_x * g_total).reshape(xs), None, None, None, None, None, None, None


def _fw(frame_weight):
    """The dataset item's scalar loss weight (models/base_rendering_model.py:1205) as a Python float.  A device tensor is refused: reading it
    would be a host synchronisation inside the training step (convert it once where the item is loaded)."""
    if frame_weight is None:
        return 1.0
    if isinstance(frame_weight, torch.Tensor):
        if frame_weight.is_cuda:
            raise HnrError("frame_weight (the item's scalar loss weight) must be a Python float or a CPU tensor, not a device tensor: "
                           "the per-view weights of the feature merge are `frame_weight_nearest`")
        if frame_weight.numel() != 1:
            raise HnrError("frame_weight is the item's scalar loss weight (1 value), got %d values" % frame_weight.numel())
        return float(frame_weight.reshape(-1)[0])
    return float(frame_weight)


def shipped_loss(coarse_raycolor, conf_coefficient, gt_image, ray_mask, zero_epsilon, w_color=1.0, w_zero_one=1e-4, frame_weight=None, conf_rows=False):
    """Returns (loss_total, parts) with parts = tensor {total, colour MSE, zero-one mean, valid rays}; loss_total is differentiable
    w.r.t. coarse_raycolor [.., R, 3] and conf_coefficient (any shape).  frame_weight: the dataset item's scalar (or None).
    conf_rows: conf_coefficient holds one row per ray of the BATCH ([R, SR, K], what render_train returns) and the rows of rays with
    ray_mask = 0 are left out on the device -- instead of indexing it with the mask first (a masked copy, a host read of the number of
    valid rays, and an index_put in the backward pass)."""
    return _ShippedLoss.apply(coarse_raycolor, conf_coefficient, gt_image, ray_mask, zero_epsilon, w_color, w_zero_one, _fw(frame_weight), bool(conf_rows))


def shipped_loss_grads(coarse_raycolor, conf_coefficient, gt_image, ray_mask, zero_epsilon, w_color=1.0, w_zero_one=1e-4, frame_weight=None, conf_rows=True,
                       device_frame_weight=None):
    """The loss terms and their gradients without an autograd graph: (parts [4] = {total, colour MSE, zero-one mean, valid rays},
    d total / d coarse_raycolor [R,3], d total / d conf_coefficient (flat)) -- what train.train_step feeds to the backward pass.
    device_frame_weight: a one-float device tensor holding the item's scalar (a captured step; the kernel reads it)."""
    fw = device_frame_weight if device_frame_weight is not None else _fw(frame_weight)
    return _loss_call(coarse_raycolor, conf_coefficient, gt_image, ray_mask, zero_epsilon, w_color, w_zero_one, fw, bool(conf_rows))


# ----------------------------------------------------------------------------------------------------------------------
# The depth term (hnr_depth_loss, csrc/depth_sup.hip): masked mean of (D - d)^2 over the rays with a hit and a measurement.  The reference's
# depth_loss_items branch (models/base_rendering_model.py:1209-1215) has no dataset that feeds it; include/hnr.h defines the term.
# ----------------------------------------------------------------------------------------------------------------------
def _depth_args(coarse_depth, gt_depth, ray_mask, w_depth):
    D = _lib.require_gpu(coarse_depth.detach(), "coarse_depth", torch.float32).reshape(-1)
    d = _lib.require_gpu(gt_depth, "gt_depth", torch.float32).reshape(-1)
    m = _lib.require_gpu(ray_mask, "ray_mask").reshape(-1)
    if m.dtype != torch.int8:
        m = m.to(torch.int8)
    R = int(D.shape[0])
    if R < 1 or d.shape[0] != R or m.shape[0] != R:
        raise HnrError("depth_loss: coarse_depth, gt_depth and ray_mask must hold one value per ray (%d, %d, %d)" % (R, d.shape[0], m.shape[0]))
    if d.device != D.device or m.device != D.device:
        raise HnrError("depth_loss: coarse_depth, gt_depth and ray_mask must be on one device")
    w = float(w_depth)
    if not (w >= 0.0 and w < float("inf")):
        raise HnrError("depth_loss: w_depth must be finite and >= 0, got %r" % (w_depth,))
    return D, d, m, R, w


def depth_loss_grads(coarse_depth, gt_depth, ray_mask, w_depth, total=None, want_grad=True):
    """The depth term without an autograd graph, one launch: (out3 = {L, n, w_depth L} on the device, d (w_depth L) / d coarse_depth [R]).
    L = mean over the rays with ray_mask > 0 and gt_depth > 0 of (coarse_depth - gt_depth)^2 (0 when there is none).  total: the `parts`
    tensor of shipped_loss_grads (or any float32 device tensor); w_depth L is added to its first element on the device, after the frame-weight
    scaling the shipped kernels applied, as the reference orders it (:1204-1215)."""
    L = _lib.lib()
    D, d, m, R, w = _depth_args(coarse_depth, gt_depth, ray_mask, w_depth)
    if total is not None:
        total = _lib.require_gpu(total, "total", torch.float32)
        if total.numel() < 1 or not total.is_contiguous() or total.device != D.device:
            raise HnrError("depth_loss: total must be a contiguous float32 tensor on the depth's device")
    out3 = torch.empty((3,), dtype=torch.float32, device=D.device)
    g = torch.empty_like(D) if want_grad else None
    p = _lib.ptr
    with torch.cuda.device(D.device):
        _lib.check(L.hnr_depth_loss(p(D), p(d), p(m), R, w, p(total), p(out3), p(g), None, _lib.stream()), "hnr_depth_loss")
    return out3, g


class _DepthLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, coarse_depth, gt_depth, ray_mask, w_depth):
        out3, g = depth_loss_grads(coarse_depth, gt_depth, ray_mask, w_depth)
        ctx.save_for_backward(g)
        ctx.shape = coarse_depth.shape
        ctx.mark_non_differentiable(out3)
        return out3[2].clone(), out3

    @staticmethod
    def backward(ctx, g_term, _g_out):
        (g,) = ctx.saved_tensors
        return (g * g_term).reshape(ctx.shape), None, None, None


def depth_loss(coarse_depth, gt_depth, ray_mask, w_depth=1.0):
    """(w_depth * L, out3 = {L, n, w_depth L}) over the same kernel; the first is differentiable w.r.t. coarse_depth (what
    render_train(want_depth=True) returns): `loss = shipped_loss(...)[0] + depth_loss(out["coarse_depth"], gt_depth, out["ray_mask"], w)[0]`."""
    return _DepthLoss.apply(coarse_depth, gt_depth, ray_mask, w_depth)


# ----------------------------------------------------------------------------------------------------------------------
# The patch SSIM term (hnr_ssim_loss, csrc/ssim_loss.hip): 1 - SSIM(win 7, sigma 1.5, data_range 1) over the patches of a patch-sampled batch.
# The reference's branch (models/base_rendering_model.py:1120-1143, pytorch_msssim's SSIM module of :27) is parked behind a pdb.set_trace() and the
# package is not a dependency here; include/hnr.h defines the term.  Not covered (each raises where it can be reached): MS-SSIM, other window
# sizes / sigmas / data_range, the commented-out patch-match and detail-aware losses, the TORCH_LIBRARY ops.
# ----------------------------------------------------------------------------------------------------------------------
SSIM_WIN_SIZE, SSIM_WIN_SIGMA, SSIM_MIN_PATCH, SSIM_MAX_PATCH = 7, 1.5, 7, 64


def ssim_window(win_size=SSIM_WIN_SIZE, win_sigma=SSIM_WIN_SIGMA):
    """The seven window values hnr_ssim_loss takes, a float32 CPU tensor: the torch ops of pytorch_msssim's _fspecial_gauss_1d in fp32."""
    if int(win_size) != SSIM_WIN_SIZE or float(win_sigma) != SSIM_WIN_SIGMA:
        raise HnrError("ssim_window: only win_size=7, win_sigma=1.5 (the reference's SSIM module, models/base_rendering_model.py:27) is supported")
    coords = torch.arange(SSIM_WIN_SIZE, dtype=torch.float32)
    coords -= SSIM_WIN_SIZE // 2
    g = torch.exp(-(coords ** 2) / (2 * SSIM_WIN_SIGMA ** 2))
    g /= g.sum()
    return g


def _ssim_check(who, n_rays, patch_num, patch_size, layout, w_ssim, norm_patches=None, frame_weight=1.0):
    """The argument checks of the SSIM term, shapes and host values only (no device) -> (signed patch_num for the library, patches of the call,
    norm_patches for the library (0 = the call's own), float w_ssim)."""
    if layout not in ("grid", "patch_major"):
        raise HnrError("%s: layout must be 'grid' or 'patch_major'" % who)
    if patch_num is None or patch_size is None:
        raise HnrError("%s: the SSIM term needs patch_num and patch_size (a patch-sampled batch)" % who)
    pn, ps = int(patch_num), int(patch_size)
    if ps < SSIM_MIN_PATCH or ps > SSIM_MAX_PATCH:
        raise HnrError("%s: patch_size %d outside %d..%d (a patch holds at least one 7 x 7 window and at most 64 x 64 rays)" % (who, ps, SSIM_MIN_PATCH, SSIM_MAX_PATCH))
    if pn < 1:
        raise HnrError("%s: patch_num must be >= 1, got %d" % (who, pn))
    n = pn if layout == "patch_major" else pn * pn
    if int(n_rays) != n * ps * ps:
        raise HnrError("%s: %d rays are not %d patches of %d x %d (layout %r)" % (who, int(n_rays), n, ps, ps, layout))
    w = float(w_ssim)
    if not (w >= 0.0 and w < float("inf")):
        raise HnrError("%s: w_ssim must be finite and >= 0, got %r" % (who, w_ssim))
    if not (float(frame_weight) >= 0.0 and float(frame_weight) < float("inf")):
        raise HnrError("%s: frame_weight must be finite and >= 0, got %r" % (who, frame_weight))
    norm = 0
    if norm_patches is not None:
        norm = int(norm_patches)
        if norm < n:
            raise HnrError("%s: norm_patches=%d is the batch-wide patch count and cannot be below the call's own %d" % (who, norm, n))
    return (-pn if layout == "patch_major" else pn), n, norm, w


def ssim_patch_loss_grads(color, gt, ray_mask, patch_num, patch_size, w_ssim, layout="grid", norm_patches=None, frame_weight=None,
                          device_frame_weight=None, total=None, g_color=None, want_grad=True):
    """The patch SSIM term without an autograd graph, two launches: (out4 = {L, SSIM, fw w_ssim L, hit rays} on the device,
    d (fw w_ssim L) / d color [R,3]).  color: what the colour losses see (the blurred colours when a blur module is on); layout "grid": patch_num^2
    patches of patch_size^2 rays tiled over the batch, "patch_major": patch_num whole patches packed (patch, y, x).  L = 1 - SSIM as include/hnr.h
    defines it (rays with ray_mask <= 0 count as zeros in both images and receive no gradient; no hit ray at all: L = 0).  norm_patches: the
    batch-wide patch count when the call holds a rank's share (parallel.shard_patches): the ranks' terms then add up to the whole batch's.
    frame_weight (host) / device_frame_weight (one float on the device) as for shipped_loss_grads.  total: the `parts` tensor of
    shipped_loss_grads; the term is added to its first element on the device.  g_color [R,3]: the gradient is ADDED to it in place (the buffer
    shipped_loss_grads returned) and it is returned; None: a new tensor (want_grad=False: none)."""
    who = "ssim_patch_loss"
    n_rays = color.numel() // 3 if isinstance(color, torch.Tensor) else -1
    fw = 1.0 if device_frame_weight is not None else _fw(frame_weight)
    pn, n, norm, w = _ssim_check(who, n_rays, patch_num, patch_size, layout, w_ssim, norm_patches, fw)
    L = _lib.lib()
    c = _lib.require_gpu(color.detach(), "color", torch.float32).reshape(-1, 3)
    g = _lib.require_gpu(gt, "gt_image", torch.float32).reshape(-1, 3)
    m = _lib.require_gpu(ray_mask, "ray_mask").reshape(-1)
    if m.dtype != torch.int8:
        m = m.to(torch.int8)
    if g.shape[0] != c.shape[0] or m.shape[0] != c.shape[0] or g.device != c.device or m.device != c.device:
        raise HnrError("%s: color, gt_image and ray_mask must hold the same rays on one device" % who)
    dev = c.device
    dfw = None
    if device_frame_weight is not None:
        dfw = _lib.require_gpu(device_frame_weight, "device_frame_weight", torch.float32).reshape(-1)
    if total is not None:
        total = _lib.require_gpu(total, "total", torch.float32)
        if total.numel() < 1 or total.device != dev:
            raise HnrError("%s: total must be a contiguous float32 tensor on the colours' device" % who)
    accumulate = g_color is not None
    if accumulate:
        if not (isinstance(g_color, torch.Tensor) and g_color.is_cuda and g_color.dtype == torch.float32 and g_color.is_contiguous()
                and g_color.numel() == c.numel() and g_color.device == dev):
            raise HnrError("%s: g_color must be a contiguous float32 [R,3] tensor on the colours' device" % who)
    elif want_grad:
        g_color = torch.empty_like(c)
    out4 = torch.empty((4,), dtype=torch.float32, device=dev)
    scratch = torch.empty((int(L.hnr_ssim_loss_scratch_bytes(n)) // 8,), dtype=torch.float64, device=dev)
    win = (ctypes.c_float * SSIM_WIN_SIZE)(*[float(v) for v in ssim_window()])
    p = _lib.ptr
    with torch.cuda.device(dev):
        _lib.check(L.hnr_ssim_loss(p(c), p(g), p(m), pn, int(patch_size), norm, win, w, fw, p(dfw), p(total), p(out4), p(g_color), int(accumulate),
                                   p(scratch), _lib.stream()), "hnr_ssim_loss")
    return out4, g_color


class _SsimPatchLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, color, gt, ray_mask, patch_num, patch_size, w_ssim, layout, norm_patches, frame_weight):
        out4, g = ssim_patch_loss_grads(color, gt, ray_mask, patch_num, patch_size, w_ssim, layout=layout, norm_patches=norm_patches,
                                        frame_weight=frame_weight)
        ctx.save_for_backward(g)
        ctx.shape = color.shape
        ctx.mark_non_differentiable(out4)
        return out4[2].clone(), out4

    @staticmethod
    def backward(ctx, g_term, _g_out):
        (g,) = ctx.saved_tensors
        return (g * g_term).reshape(ctx.shape), None, None, None, None, None, None, None, None


def ssim_patch_loss(color, gt, ray_mask, patch_num, patch_size, w_ssim=1.0, layout="grid", norm_patches=None, frame_weight=None):
    """(fw w_ssim L, out4 = {L, SSIM, fw w_ssim L, hit rays}) over the same kernels; the first is differentiable w.r.t. color, so the term works
    behind render_train and behind blur_update_output / learnable_blur_update_output:
    `loss = shipped_loss(col, ...)[0] + ssim_patch_loss(col, gt_image, out["ray_mask"], pn, ps, w)[0]`."""
    return _SsimPatchLoss.apply(color, gt, ray_mask, patch_num, patch_size, w_ssim, layout, norm_patches, frame_weight)
