"""torch.ops.hnr.*: the path as dispatcher-visible PyTorch ops (csrc/torch_ops/hnr_torch.cpp, TORCH_LIBRARY(hnr) over the C ABI of libhnr_hip.so).

SURVEY 8b asks for both op layers: the C ABI (include/hnr.h, bound by ctypes in _lib.py -- needs no torch headers) and registered torch ops.  The
ops are the same library calls with schemas: `hnr::grid_build`, `hnr::grid_free`, `hnr::march_query`, `hnr::nearest_view`, `hnr::point_view_attrs`
(the cloud initialisation of cloud_init.py), `hnr::alpha_pack`, `hnr::visual_hull_select`, `hnr::point_occlusion` (the synthetic scenes' visual-hull
masking and occlusion test, cloud_init.py), `hnr::featnet_forward`, `hnr::point_embed` (the init checkpoint's networks, mvs_init.py), `hnr::mvsnet_feature`,
`hnr::mvsnet_cost_volume`, `hnr::mvsnet_cost_reg`, `hnr::mvsnet_depth_head`, `hnr::mvsnet_depth_points` (the depth estimator, mvs_depth.py), `hnr::render_forward`
(NeuralPointsRayMarching.forward + fill_invalid in eval mode, /root/reference/models/neural_points_volumetric_model.py:257-391, :87-126) and
`hnr::render_train` (the same in train mode with the backward pass registered as its autograd formula; the reference leaves that to torch autograd,
models/mvs_points_volumetric_model.py:111-131).  This module loads the extension and builds the ops' argument lists from the host-side objects
(HybridRenderer, PointAggregator); the results are bit-identical to the ctypes route (tests/test_torch_ops_gpu.py).  No fallback: a missing
libhnr_torch.so raises."""
import os

import numpy as np
import torch

from ._lib import HnrError
from . import _lib, _raycall

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhnr_torch.so")
_loaded = False

# hnr_train_weights in struct order (_lib.TRAIN_WEIGHTS): parameter names of the reference's PointAggregator; the ops' output lists (_raycall.RAY_OUTPUTS)
TRAIN_WEIGHT_NAMES = [n for _f, names in _lib.TRAIN_WEIGHTS for n in ([names] if isinstance(names, str) else names)]
FORWARD_OUTPUTS, TRAIN_OUTPUTS = _raycall.FORWARD_OUTPUTS, _raycall.TRAIN_OUTPUTS
NCOUNTS = _lib.NCOUNTS


def _register_fakes():
    """Shape functions ("fake" / meta kernels) of the tensor-returning ops: what torch.compile, torch.export and FakeTensorMode need to trace through
    them without running a kernel.  Output shapes and dtypes are those of the C++ implementations (hnr_torch.cpp)."""
    f32, i32 = torch.float32, torch.int32

    @torch.library.register_fake("hnr::march_query")
    def _(grid, campos, raydir, tmid, SR, K, radius2, kernel_size, pad, knn_order):
        R, e = raydir.shape[0], raydir.new_empty
        return (e((R, SR, K), dtype=i32), e((R, SR, 3), dtype=f32), e((R,), dtype=i32), e((R,), dtype=torch.int8), e((NCOUNTS,), dtype=torch.int64))

    @torch.library.register_fake("hnr::render_forward")
    def _(grid, xyz, conf, dir, color, point_table, point_records, packed, campos, camrot, raydir, tmid, bg_color, w2c, intrinsic, campos_nearest, featmap,
          frame_w, SR, K, kernel_size, radius2, vsize_z, raydist_mode_unit, knn_order, slope, cap_samples):
        o = _raycall.RayOutputs.alloc(raydir.shape[0], SR, K, None, blend=False, weights=False, empty=raydir.new_empty)
        return [o.t[k] for k in FORWARD_OUTPUTS]

    def train_outs(inputs, SR):
        return list(_raycall.RayOutputs.alloc(inputs[7].shape[0], SR, 8, None, empty=inputs[7].new_empty).t.values())

    @torch.library.register_fake("hnr::render_train")
    def _(grid, inputs, weights, drop_lut, ray_drop, SR, kernel_size, radius2, vsize_z, raydist_mode_unit, knn_order, slope, cap_samples):
        return train_outs(inputs, SR)

    @torch.library.register_fake("hnr::render_train_fwd")
    def _(grid, inputs, weights, drop_lut, ray_drop, SR, kernel_size, radius2, vsize_z, raydist_mode_unit, knn_order, slope, cap_samples):
        raydir, tmid, img = inputs[7], inputs[8], inputs[13]
        V, H, W = (int(img.shape[0]), int(img.shape[1]), int(img.shape[2])) if img is not None and img.numel() > 0 else (0, 0, 0)
        # the workspace size is a host-side function of the shapes (no kernel runs)
        prm = _raycall.fill_params(_lib.TrainParams(), raydir.shape[0], SR, 8, tmid, kernel_size, radius2, vsize_z, raydist_mode_unit, V, max(int(cap_samples), 0), knn_order)
        prm.H, prm.W, prm.n_points, prm.slope = H, W, int(inputs[0].shape[-2]), float(slope)
        return train_outs(inputs, SR) + [raydir.new_empty((_raycall.train_workspace_bytes(prm) + _raycall.WS_ALIGN,), dtype=torch.uint8)]

    @torch.library.register_fake("hnr::render_train_bwd")
    def _(inputs, weights, fwd, g_raycolor, g_conf_coefficient, SR, kernel_size, radius2, vsize_z, raydist_mode_unit, knn_order, slope, cap_samples):
        N, e, img = int(inputs[0].shape[-2]), inputs[7].new_empty, inputs[13]
        views = img is not None and img.numel() > 0
        image_branch = lambda i: (16 <= i < 24) or i >= 32
        return [e((N, 32), dtype=f32), e((N,), dtype=f32), e((N, 3), dtype=f32), e((N, 3), dtype=f32)] + \
               [torch.empty_like(w) if (views or not image_branch(i)) else w.new_empty((0,)) for i, w in enumerate(weights)]


    @torch.library.register_fake("hnr::nearest_view")
    def _(xyz, campos, camdir):
        return xyz.new_empty((xyz.shape[0],), dtype=i32)

    @torch.library.register_fake("hnr::alpha_pack")
    def _(alphas):
        M, H, W = alphas.shape
        return alphas.new_empty((M, H, (W + 31) // 32), dtype=i32)

    @torch.library.register_fake("hnr::visual_hull_select")
    def _(xyz, conf, view, bits, cams, W, near_far, range_mask, capacity):
        n, rows, e = xyz.shape[0], max(capacity, 1), xyz.new_empty
        return (e((n,), dtype=torch.uint8), e((rows, 3), dtype=f32), e((rows if conf is not None else 0,), dtype=f32),
                e((rows if view is not None else 0,), dtype=i32), e((1,), dtype=torch.int64), e((1,), dtype=i32))

    @torch.library.register_fake("hnr::point_occlusion")
    def _(xyz, w2c, intrinsic, H, W, tolerate):
        return xyz.new_empty((xyz.shape[0],), dtype=torch.uint8)

    @torch.library.register_fake("hnr::point_view_attrs")
    def _(xyz, w2c, c2w, cam_pos_cam, intrinsic, H, W, feat, visible=None):
        n, e = xyz.shape[0], xyz.new_empty
        return (e((n, feat.shape[0] if feat is not None else 0), dtype=f32), e((n, 3), dtype=f32), e((n,), dtype=torch.uint8))

    @torch.library.register_fake("hnr::featnet_forward")
    def _(images, packed):
        V, _, H, W = images.shape
        H2, W2 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        e = images.new_empty
        return (e((V, 8, H, W), dtype=f32), e((V, 16, H2, W2), dtype=f32), e((V, 32, (H2 - 1) // 2 + 1, (W2 - 1) // 2 + 1), dtype=f32))

    @torch.library.register_fake("hnr::point_embed")
    def _(xyz, w2c, c2w, cam_pos_cam, intrinsic, image, x1, x2, x3, premlp, want_row, visible=None):
        n, e = xyz.shape[0], xyz.new_empty
        return (e((n, 32), dtype=f32), e((n, 3), dtype=f32), e((n, 3), dtype=f32), e((n, 63 if want_row else 0), dtype=f32))

    @torch.library.register_fake("hnr::mvsnet_feature")
    def _(images, packed):
        V, _, H, W = images.shape
        return images.new_empty((V, 32, ((H - 1) // 2 + 1 - 1) // 2 + 1, ((W - 1) // 2 + 1 - 1) // 2 + 1), dtype=f32)

    @torch.library.register_fake("hnr::mvsnet_cost_volume")
    def _(feat, proj, depth_values):
        return feat.new_empty((32, depth_values.shape[0], feat.shape[2], feat.shape[3]), dtype=f32)

    @torch.library.register_fake("hnr::mvsnet_cost_reg")
    def _(volume, packed):
        return volume.new_empty(tuple(volume.shape[1:]), dtype=f32)

    @torch.library.register_fake("hnr::mvsnet_depth_head")
    def _(logits, depth_values, want_prob):
        D, h, w = logits.shape
        e = logits.new_empty
        return (e((h, w), dtype=f32), e((h, w), dtype=f32), e((D, h, w) if want_prob else (0,), dtype=f32))

    @torch.library.register_fake("hnr::mvsnet_depth_points")
    def _(depth, conf, H, W, near, far, kt_inv):
        e = depth.new_empty
        return (e((H, W, 3), dtype=f32), e((H, W), dtype=f32), e((H, W), dtype=torch.uint8))


def load():
    """Registers torch.ops.hnr (once), with shape functions for tracing.  libhnr_torch.so links libhnr_hip.so next to it."""
    global _loaded
    if not _loaded:
        if not os.path.exists(LIB_PATH):
            raise HnrError("%s is missing: build it with `make -C hybridneuralrendering_amd/csrc` (__graft_entry__.build())" % LIB_PATH)
        _lib.lib()                                         # the ctypes handle first: both bindings share ONE loaded libhnr_hip.so
        torch.ops.load_library(LIB_PATH)
        _register_fakes()
        _loaded = True
    return torch.ops.hnr


def _handle(grid):
    h = grid.handle
    return int(h.value if hasattr(h, "value") else h)


def train_weight_list(aggregator):
    """The 44 parameter tensors hnr::render_train takes, in hnr_train_weights order."""
    prm = dict(aggregator.named_parameters())
    return [prm[n] for n in TRAIN_WEIGHT_NAMES]


def render_forward(renderer, cloud, raydir, campos, camrot, bg_color, near, far, c2w_nearest, campos_nearest, intrinsic_nearest, images_nearest,
                   frame_weight=None, w2c_nearest=None):
    """HybridRenderer.render_rays through torch.ops.hnr.render_forward: same grid, packed weights, per-point table and feature map (all cached by the
    renderer), one registered op instead of the ctypes call.  Returns the output dict of render_rays."""
    ops = load()
    opt, agg = renderer.opt, renderer.agg
    if getattr(cloud, "parts", None) is not None:
        raise _lib.HnrError("torch.ops.hnr.render_forward takes no Rw2c (per-point rotations of an edited scene); use HybridRenderer.render_rays")
    views = getattr(opt, "use_nearest", 4) != 0
    inp = _raycall.ray_inputs(raydir, campos, camrot, bg_color, c2w_nearest, campos_nearest, intrinsic_nearest, None, w2c_nearest, frame_weight, views=views)
    grid, hp = renderer.querier._grid_for(cloud.xyz[None])
    tmid = renderer.querier._tmid_for(float(near), float(far), opt.z_depth_dim, inp.raydir.shape[0], inp.raydir.device)
    fm = renderer.feature_map(images_nearest) if views else None
    pk, m3 = agg.packed(), agg.packed_mlp3()
    packed = [agg.packed_chain(), m3["cf"].packed, m3["mw"].packed, m3["mx"].packed, pk["mw_last_w"], pk["mw_last_b"], pk["fin_w"], pk["fin_b"]]
    packed = [t if t.dtype == torch.float32 else t.view(torch.uint8) for t in packed]
    out = ops.render_forward(_handle(grid), cloud.xyz, cloud.conf, cloud.dir, cloud.color, renderer.point_table(cloud), renderer.point_records(cloud), packed,
                             inp.campos, inp.camrot, inp.raydir, tmid, inp.bg_color, inp.w2c, inp.intrinsic, inp.campos_nearest, fm, inp.frame_w,
                             int(opt.SR), int(opt.K), [int(k) for k in opt.kernel_size], *_raycall.opt_scalars(opt, hp[0] ** 2),
                             1 if renderer.knn_order == "sorted" else 0, float(pk["slope"]), 0)
    return dict(zip(FORWARD_OUTPUTS, out))


def render_train(renderer, aggregator, xyz, emb, conf, pdir, color, raydir, campos, camrot, bg_color, near, far, c2w_nearest, campos_nearest,
                 intrinsic_nearest, images_nearest, frame_weight_nearest=None, tmid=None, drop_lut=None, ray_drop=None):
    """Differentiable render of one ray batch through torch.ops.hnr.render_train (autograd formula registered in C++): emb / conf / pdir / color may be the
    reference's nn.Parameters ([1,N,32], [1,N,1], [1,N,3], [1,N,3]); the aggregator's parameters receive gradients.  Returns the 13 outputs as a dict;
    coarse_raycolor and conf_coefficient are attached to the autograd graph.  drop_lut: train.drop_lut(opt, R, device) for the patch-drop pattern."""
    ops = load()
    opt = renderer.opt
    inp = _raycall.ray_inputs(raydir, campos, camrot, bg_color, c2w_nearest, campos_nearest, intrinsic_nearest, images_nearest, None, frame_weight_nearest,
                              "frame_weight_nearest", views=getattr(opt, "use_nearest", 4) != 0)
    grid, hp = renderer.querier._grid_for(xyz.detach()[None] if xyz.dim() == 2 else xyz.detach())
    if tmid is None:
        tmid = renderer.querier._tmid_for(float(near), float(far), opt.z_depth_dim, inp.raydir.shape[0], inp.raydir.device)
    inputs = [xyz.reshape(-1, 3), emb, conf, pdir, color, inp.campos, inp.camrot, inp.raydir, _lib.require_gpu(tmid, "tmid", torch.float32), inp.bg_color,
              inp.w2c, inp.intrinsic, inp.campos_nearest, inp.images, inp.frame_w]
    out = ops.render_train(_handle(grid), inputs, train_weight_list(aggregator), drop_lut, ray_drop, int(opt.SR), [int(k) for k in opt.kernel_size],
                           *_raycall.opt_scalars(opt, hp[0] ** 2), 0, float(aggregator.block1[1].negative_slope), 0)
    return dict(zip(TRAIN_OUTPUTS, out))


def nearest_view(campos, raydir, xyz, id_list=None):
    """cloud_init.nearest_view through torch.ops.hnr.nearest_view: [N,1] int64 (run/train_ft.py:48-57)."""
    ops = load()
    g = _lib.require_gpu
    return ops.nearest_view(g(xyz, "xyz", torch.float32).reshape(-1, 3), g(campos, "campos", torch.float32).reshape(-1, 3),
                            g(raydir, "raydir", torch.float32).reshape(-1, 3)).long().view(-1, 1)


def _flat(a, n):
    return [float(v) for v in np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32).reshape(n)]


def alpha_pack(alphas):
    """cloud_init.alpha_pack through torch.ops.hnr.alpha_pack: alphas [M,H,W] -> int32 [M,H,(W+31)//32]."""
    return load().alpha_pack(_lib.require_gpu(alphas, "alphas", torch.float32))


def visual_hull_select(xyz, bits, cams, W, near_far=None, range_mask=False, conf=None, view=None, capacity=None):
    """cloud_init.visual_hull_select through torch.ops.hnr.visual_hull_select: (mask [n] uint8, xyz [cap,3], conf [cap] or [0], view [cap] or [0],
    count [1] int64, status [1] int32).  bits / cams: AlphaMasks.bits / .cams; near_far: (near, far) or None."""
    from .cloud_init import _near_far_pair
    g = _lib.require_gpu
    xyz = g(xyz, "xyz", torch.float32).reshape(-1, 3)
    nf = _near_far_pair(near_far, "visual_hull_select")
    return load().visual_hull_select(xyz, None if conf is None else g(conf, "conf", torch.float32), None if view is None else g(view, "view", torch.int32),
                                     g(bits, "bits", torch.int32), g(cams, "cams", torch.float32), int(W), [] if nf is None else [float(v) for v in nf],
                                     bool(range_mask), int(xyz.shape[0] if capacity is None else capacity))


def point_occlusion(xyz, w2c, intrinsic, H, W, tolerate=0.1):
    """cloud_init.point_occlusion through torch.ops.hnr.point_occlusion: uint8 [n]."""
    return load().point_occlusion(_lib.require_gpu(xyz, "xyz", torch.float32).reshape(-1, 3), _flat(w2c, 16), _flat(intrinsic, 9), int(H), int(W),
                                  float(np.float32(tolerate)))


def point_view_attrs(xyz, w2c, c2w, cam_pos_cam, intrinsic, H, W, feat=None, visible=None):
    """cloud_init.point_view_attrs through torch.ops.hnr.point_view_attrs: (features [n,C], dir [n,3], mask [n] uint8); without `feat` the features are
    [n,0].  The matrices are host arrays (fp32 values travel exactly through the op's float[] arguments).  visible: point_occlusion's flags."""
    ops = load()
    flat = lambda a, n: [float(v) for v in np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32).reshape(n)]
    return ops.point_view_attrs(_lib.require_gpu(xyz, "xyz", torch.float32).reshape(-1, 3), flat(w2c, 16), flat(c2w, 16), flat(cam_pos_cam, 3), flat(intrinsic, 9),
                                int(H), int(W), None if feat is None else _lib.require_gpu(feat, "feat", torch.float32),
                                None if visible is None else _lib.require_gpu(visible, "visible", torch.uint8))


def featnet_forward(images, packed):
    """mvs_init.featnet_forward through torch.ops.hnr.featnet_forward: images [V,3,H,W], packed = FeatureNet.packed() -> (x1, x2, x3)."""
    ops = load()
    g = _lib.require_gpu
    return ops.featnet_forward(g(images, "images", torch.float32), g(packed, "packed", torch.float32))


def point_embed(xyz, w2c, c2w, cam_pos_cam, intrinsic, image, x1, x2, x3, premlp, want_row=False, visible=None):
    """mvs_init.point_embed through torch.ops.hnr.point_embed: (emb [n,32], color [n,3], dir [n,3], row [n,63] or [n,0]).  visible: point_occlusion's flags."""
    ops = load()
    g = _lib.require_gpu
    flat = lambda a, n: [float(v) for v in np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32).reshape(n)]
    return ops.point_embed(g(xyz, "xyz", torch.float32).reshape(-1, 3), flat(w2c, 16), flat(c2w, 16), flat(cam_pos_cam, 3), flat(intrinsic, 9),
                           g(image, "image", torch.float32), g(x1, "x1", torch.float32), g(x2, "x2", torch.float32), g(x3, "x3", torch.float32),
                           g(premlp, "premlp", torch.float32), bool(want_row), None if visible is None else g(visible, "visible", torch.uint8))


def mvsnet_feature(images, packed):
    """mvs_depth.feature_forward through torch.ops.hnr.mvsnet_feature: images [V,3,H,W], packed = MVSNet.packed()[0] -> [V,32,h,w]."""
    g = _lib.require_gpu
    return load().mvsnet_feature(g(images, "images", torch.float32), g(packed, "packed", torch.float32))


def mvsnet_cost_volume(features, proj, depth_values):
    """mvs_depth.cost_volume through torch.ops.hnr.mvsnet_cost_volume: features [V,32,h,w], proj [V,3,4] or [V,4,4], depth_values [D] -> [32,D,h,w]."""
    g = _lib.require_gpu
    return load().mvsnet_cost_volume(g(features, "features", torch.float32), g(proj, "proj", torch.float32)[:, :3].contiguous(),
                                     g(depth_values, "depth_values", torch.float32))


def mvsnet_cost_reg(volume, packed):
    """mvs_depth.cost_reg through torch.ops.hnr.mvsnet_cost_reg: volume [32,D,h,w], packed = MVSNet.packed()[1] -> logits [D,h,w]."""
    g = _lib.require_gpu
    return load().mvsnet_cost_reg(g(volume, "volume", torch.float32), g(packed, "packed", torch.float32))


def mvsnet_depth_head(logits, depth_values, want_prob=False):
    """mvs_depth.depth_head through torch.ops.hnr.mvsnet_depth_head: (depth [h,w], confidence [h,w], prob [D,h,w] or [0])."""
    g = _lib.require_gpu
    return load().mvsnet_depth_head(g(logits, "logits", torch.float32), g(depth_values, "depth_values", torch.float32), bool(want_prob))


def mvsnet_depth_points(depth, confidence, H, W, near, far, intrinsic):
    """mvs_depth.depth_points through torch.ops.hnr.mvsnet_depth_points: (cam_xyz [H,W,3], confidence [H,W], points_mask [H,W] uint8)."""
    from .mvs_depth import kt_inverse
    g = _lib.require_gpu
    return load().mvsnet_depth_points(g(depth, "depth", torch.float32), g(confidence, "confidence", torch.float32), int(H), int(W), float(np.float32(near)),
                                      float(np.float32(far)), [float(v) for v in kt_inverse(intrinsic).reshape(9)])
