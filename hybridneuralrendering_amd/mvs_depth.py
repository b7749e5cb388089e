"""Depth maps from the pretrained MVSNet, on the device (csrc/mvsnet.hip).

The reference starts a `load_points=0`, `manual_depth_view=1` scene from the depth maps of a pretrained estimator (run/train_ft.py:104-190):
`models/depth_estimators/mvsnet.py`, loaded by `MvsPointsModel.load_pretrained_d_est` from `--pre_d_est .../MVSNet/model_000014.ckpt`, then the tail
of `MvsPointsModel.gen_points` (models/mvs/mvs_points_model.py:300-341).  `MVSNet` here carries that network's parameter and buffer names, so the
checkpoint loads as it is, and runs it as HIP kernels, stage by stage: `feature_forward`, `cost_volume`, `cost_reg`, `depth_head`, `depth_points`.
`depth_views` is the `manual_depth_view == 1` branch of `gen_points`: its result is what `cloud_init.init_cloud_from_mvs_depth` takes.
Inference only (no backward, results carry no graph), GPU only (no CPU or torch fallback: `HnrError`).

NOT the `MVSNet.*` keys of a `*_net_mvs.pth`: those belong to another network (models/mvs/models.py, `cost_reg_2`, the `manual_depth_view=-1` path),
which `mvs_init.MvsInit` ignores and nothing here loads.
"""
import numpy as np
import torch
from torch import nn

from . import _lib
from ._lib import HnrError
from ._nets import NormParams, Packed, PackedWeights, filtered_state_dict, gpu_f32, host_f32, load_checked, load_checkpoint

EPS = 1e-5                                                       # nn.BatchNorm's eps
NUM_DEPTH = 192                                                  # gen_points' depth planes
FEATURE_LAYERS = ((3, 8, 3, 1), (8, 8, 3, 1), (8, 16, 5, 2), (16, 16, 3, 1), (16, 16, 3, 1), (16, 32, 5, 2), (32, 32, 3, 1))    # (cin, cout, kernel, stride)
REG_CONVS = ((32, 8, 1), (8, 16, 2), (16, 16, 1), (16, 32, 2), (32, 32, 1), (32, 64, 2), (64, 64, 1))                           # (cin, cout, stride)
REG_DECONVS = (("conv7", 64, 32), ("conv9", 32, 16), ("conv11", 16, 8))


def feature_shape(H, W):
    """(h, w) of the feature map and of the depth map."""
    return ((H - 1) // 2 + 1 - 1) // 2 + 1, ((W - 1) // 2 + 1 - 1) // 2 + 1


def feature_forward(images, packed):
    """hnr_mvsnet_feature: images [V,3,H,W], packed [MVSNET_FEATURE_PACKED_ELEMS] -> [V,32,h,w]."""
    images, packed = gpu_f32(images, "images"), gpu_f32(packed, "packed", (_lib.MVSNET_FEATURE_PACKED_ELEMS,))
    if images.dim() != 4 or images.shape[1] != 3:
        raise HnrError("feature_forward: images must be [V,3,H,W], got %s" % (tuple(images.shape),))
    V, _, H, W = (int(s) for s in images.shape)
    scratch = _lib.scratch("hnr_mvsnet_feature_scratch_elems", V, H, W, device=images.device, dtype=torch.float32,
                           what="feature_forward: unsupported shape V=%d H=%d W=%d (1 <= V <= 64, 4 <= H, W <= 32768)" % (V, H, W))
    out = torch.empty((V, 32) + feature_shape(H, W), dtype=torch.float32, device=images.device)
    _lib.call("hnr_mvsnet_feature", images, V, H, W, packed, out, scratch, scratch.numel(), _lib.STREAM)
    return out


def cost_volume(features, proj, depth_values):
    """hnr_mvsnet_cost_volume for one reference view: features [V,32,h,w], proj [V,3,4] (or [V,4,4]), depth_values [D] -> [32,D,h,w]."""
    features, proj, depth_values = gpu_f32(features, "features"), gpu_f32(proj, "proj"), gpu_f32(depth_values, "depth_values")
    if features.dim() != 4 or features.shape[1] != 32:
        raise HnrError("cost_volume: features must be [V,32,h,w], got %s" % (tuple(features.shape),))
    V, _, h, w = (int(s) for s in features.shape)
    if proj.dim() != 3 or proj.shape[0] != V or tuple(proj.shape[1:]) not in ((3, 4), (4, 4)) or depth_values.dim() != 1:
        raise HnrError("cost_volume: proj must be [V,3,4] or [V,4,4] and depth_values [D]")
    proj, D = proj[:, :3].contiguous(), int(depth_values.shape[0])
    if not (1 <= V <= 64 and 2 <= h <= 8192 and 2 <= w <= 8192 and 1 <= D <= 4096 and D * h * w <= 2 ** 26):
        raise HnrError("cost_volume: unsupported shape V=%d D=%d h=%d w=%d (V <= 64, 2 <= h, w <= 8192, D <= 4096, D*h*w <= 2^26)" % (V, D, h, w))
    out = torch.empty((32, D, h, w), dtype=torch.float32, device=features.device)
    _lib.call("hnr_mvsnet_cost_volume", features, V, h, w, proj, depth_values, D, out, _lib.STREAM)
    return out


def cost_reg(volume, packed):
    """hnr_mvsnet_cost_reg: volume [32,D,h,w], packed [MVSNET_REG_PACKED_ELEMS] -> logits [D,h,w].  D, h and w must be multiples of 8."""
    volume, packed = gpu_f32(volume, "volume"), gpu_f32(packed, "packed", (_lib.MVSNET_REG_PACKED_ELEMS,))
    if volume.dim() != 4 or volume.shape[0] != 32:
        raise HnrError("cost_reg: volume must be [32,D,h,w], got %s" % (tuple(volume.shape),))
    D, h, w = (int(s) for s in volume.shape[1:])
    scratch = _lib.scratch("hnr_mvsnet_cost_reg_scratch_elems", D, h, w, device=volume.device, dtype=torch.float32,
                           what="cost_reg: unsupported shape D=%d h=%d w=%d: each must be a multiple of 8 (the skip connections do not line up otherwise; the "
                                "reference fails there too), D <= 4096, h, w <= 8192, D*h*w <= 2^26" % (D, h, w))
    out = torch.empty((D, h, w), dtype=torch.float32, device=volume.device)
    _lib.call("hnr_mvsnet_cost_reg", volume, D, h, w, packed, out, scratch, scratch.numel(), _lib.STREAM)
    return out


def depth_head(logits, depth_values, want_prob=False):
    """hnr_mvsnet_depth_head: logits [D,h,w], depth_values [D] -> (depth [h,w], confidence [h,w], prob [D,h,w] or None)."""
    logits, depth_values = gpu_f32(logits, "logits"), gpu_f32(depth_values, "depth_values")
    if logits.dim() != 3 or tuple(depth_values.shape) != (logits.shape[0],):
        raise HnrError("depth_head: logits must be [D,h,w] and depth_values [D]")
    D, h, w = (int(s) for s in logits.shape)
    depth, conf = (torch.empty((h, w), dtype=torch.float32, device=logits.device) for _ in range(2))
    prob = torch.empty_like(logits) if want_prob else None
    _lib.call("hnr_mvsnet_depth_head", logits, depth_values, D, h, w, depth, conf, prob, _lib.STREAM)
    return depth, conf, prob


def kt_inverse(intrinsic):
    """inverse(K^T) in fp32 on the host, as mvs_utils.ndc_2_cam forms it."""
    from .cloud_init import _host_f32
    return torch.inverse(torch.from_numpy(_host_f32(intrinsic, (3, 3), "intrinsic")).t()).contiguous().numpy()


def depth_points(depth, confidence, H, W, near, far, intrinsic):
    """hnr_mvsnet_depth_points: depth, confidence [h,w] -> (cam_xyz [H,W,3], confidence [H,W], points_mask [H,W] bool)."""
    from .cloud_init import _cf
    depth, confidence = gpu_f32(depth, "depth"), gpu_f32(confidence, "confidence")
    if depth.dim() != 2 or confidence.shape != depth.shape:
        raise HnrError("depth_points: depth and confidence must be [h,w]")
    h, w, H, W = int(depth.shape[0]), int(depth.shape[1]), int(H), int(W)
    M = kt_inverse(intrinsic)
    cam = torch.empty((H, W, 3), dtype=torch.float32, device=depth.device)
    conf = torch.empty((H, W), dtype=torch.float32, device=depth.device)
    mask = torch.empty((H, W), dtype=torch.uint8, device=depth.device)
    _lib.call("hnr_mvsnet_depth_points", depth, confidence, h, w, H, W, float(np.float32(near)), float(np.float32(far)), _cf(M), cam, conf, mask,
              _lib.STREAM)
    return cam, conf, mask.bool()


class _ConvBnReLU(nn.Module):
    def __init__(self, conv):
        super().__init__()
        self.conv, self.bn = conv, NormParams(conv.out_channels)


def _normed(w, bn):
    """[w, running_mean, mul, bias] of one layer; mul = weight * rsqrt(running_var + eps) is folded here, once."""
    return [w, host_f32(bn.running_mean), host_f32(bn.weight) * torch.rsqrt(host_f32(bn.running_var) + EPS), host_f32(bn.bias)]


class _FeatureNet(nn.Module):
    def __init__(self):
        super().__init__()
        for i, (cin, cout, ks, stride) in enumerate(FEATURE_LAYERS):
            setattr(self, "conv%d" % i, _ConvBnReLU(nn.Conv2d(cin, cout, ks, stride=stride, padding=ks // 2, bias=False)))
        self.feature = nn.Conv2d(32, 32, 3, 1, 1)


class _CostRegNet(nn.Module):
    def __init__(self):
        super().__init__()
        for i, (cin, cout, stride) in enumerate(REG_CONVS):
            setattr(self, "conv%d" % i, _ConvBnReLU(nn.Conv3d(cin, cout, 3, stride=stride, padding=1, bias=False)))
        for name, cin, cout in REG_DECONVS:
            setattr(self, name, nn.Sequential(nn.ConvTranspose3d(cin, cout, 3, padding=1, output_padding=1, stride=2, bias=False), NormParams(cout)))
        self.prob = nn.Conv3d(8, 1, 3, stride=1, padding=1)


class MVSNet(PackedWeights, nn.Module):
    """The reference's depth estimator `MVSNet(refine=False)` in eval mode: its parameter and buffer names (`feature.conv0.conv.weight`, ...,
    `cost_regularization.conv7.1.running_var`, `cost_regularization.prob.bias`), its forward signature, HIP kernels inside."""

    def __init__(self, refine=False):
        super().__init__()
        if refine:
            raise HnrError("MVSNet: refine=True (RefineNet) is not implemented")
        self.refine = False
        self.feature = _FeatureNet()
        self.cost_regularization = _CostRegNet()
        self._packed = Packed()

    def load_pretrained(self, path_or_dict):
        """`MvsPointsModel.load_pretrained_d_est`: the checkpoint's ['model'] with `module.` stripped.  `num_batches_tracked` entries are ignored; a
        missing key is an HnrError."""
        ckpt = load_checkpoint(path_or_dict)
        load_checked(self, filtered_state_dict(ckpt["model"] if "model" in ckpt else ckpt), "MVSNet.load_pretrained")
        return self

    def pack_host(self):
        """(feature [MVSNET_FEATURE_PACKED_ELEMS], cost_reg [MVSNET_REG_PACKED_ELEMS]) fp32 on the CPU, the layouts of include/hnr.h."""
        fn, cr = self.feature, self.cost_regularization
        with torch.no_grad():
            parts = []
            for i in range(len(FEATURE_LAYERS)):
                blk = getattr(fn, "conv%d" % i)
                parts += _normed(host_f32(blk.conv.weight).permute(1, 2, 3, 0), blk.bn)
            parts += [host_f32(fn.feature.weight).permute(1, 2, 3, 0), host_f32(fn.feature.bias)]
            feat = torch.cat([p.contiguous().reshape(-1) for p in parts])
            parts = []
            for i in range(len(REG_CONVS)):
                blk = getattr(cr, "conv%d" % i)
                parts += _normed(host_f32(blk.conv.weight).permute(1, 2, 3, 4, 0), blk.bn)
            for name, _, _ in REG_DECONVS:
                seq = getattr(cr, name)
                parts += _normed(host_f32(seq[0].weight).permute(0, 2, 3, 4, 1), seq[1])             # ConvTranspose3d keeps [cin][cout][kz][ky][kx]
            parts += [host_f32(cr.prob.weight).permute(1, 2, 3, 4, 0), host_f32(cr.prob.bias)]
            reg = torch.cat([p.contiguous().reshape(-1) for p in parts])
        assert feat.numel() == _lib.MVSNET_FEATURE_PACKED_ELEMS and reg.numel() == _lib.MVSNET_REG_PACKED_ELEMS
        return feat, reg

    def image_features(self, imgs):
        """imgs [V,3,H,W] -> [V,32,h,w]: the feature maps of every view, computed once for all reference views."""
        return feature_forward(imgs, self.packed()[0])

    def forward(self, imgs, proj_matrices, depth_values, features=None, prob_only=False, want_prob=False):
        """imgs [B,V,3,H,W], proj_matrices [B,V,3,4] or [B,V,4,4], depth_values [B,D] -> (depth [B,h,w], photometric_confidence [B,h,w], features,
        prob_volume [B,D,h,w] or None).  features: a list of V maps [B,32,h,w], the reference's form (also what is returned), or one tensor [V,32,h,w]
        shared by every batch row (`depth_views`: the rows are the same images under other projections)."""
        if prob_only:
            raise HnrError("MVSNet: prob_only=True (the top-k path, manual_depth_view > 1) is not implemented")
        for t, name in ((imgs, "imgs"), (proj_matrices, "proj_matrices"), (depth_values, "depth_values")):
            if not isinstance(t, torch.Tensor):
                raise HnrError("MVSNet: %s must be a tensor" % name)
        if imgs.dim() != 5 or imgs.shape[2] != 3:
            raise HnrError("MVSNet: imgs must be [B,V,3,H,W], got %s" % (tuple(imgs.shape),))
        B, V, _, H, W = (int(s) for s in imgs.shape)
        if proj_matrices.dim() != 4 or tuple(proj_matrices.shape[:2]) != (B, V) or depth_values.dim() != 2 or depth_values.shape[0] != B:
            raise HnrError("MVSNet: proj_matrices must be [B,V,3,4] or [B,V,4,4] and depth_values [B,D]")
        h, w = feature_shape(H, W)
        D = int(depth_values.shape[1])
        if h % 8 or w % 8 or D % 8:
            raise HnrError("MVSNet: the depth map's height %d and width %d and the number of depth planes %d must be multiples of 8 (images of %dx%d: the "
                           "skip connections of the 3-D network do not line up otherwise, and the reference fails there too)" % (h, w, D, H, W))
        imgs, proj_matrices, depth_values = gpu_f32(imgs, "imgs"), gpu_f32(proj_matrices, "proj_matrices"), gpu_f32(depth_values, "depth_values")
        dev = self.feature.feature.weight.device
        if dev != imgs.device:
            raise HnrError("MVSNet: the module is on %s, imgs on %s" % (dev, imgs.device))
        feat_pk, reg_pk = self.packed()
        shared = isinstance(features, torch.Tensor)
        if features is None:
            per_row = self.image_features(imgs.reshape(B * V, 3, H, W)).reshape(B, V, 32, h, w)
            features = [per_row[:, v] for v in range(V)]
        elif shared:
            features = gpu_f32(features, "features", (V, 32, h, w))
        else:
            per_row = torch.stack([gpu_f32(f, "features[v]", (B, 32, h, w)) for f in features], dim=1)
        depths, confs, probs = [], [], []
        for b in range(B):
            vol = cost_volume(features if shared else per_row[b], proj_matrices[b], depth_values[b])
            d, c, p = depth_head(cost_reg(vol, reg_pk), depth_values[b], want_prob)
            depths.append(d); confs.append(c); probs.append(p)
        return torch.stack(depths), torch.stack(confs), features, (torch.stack(probs) if want_prob else None)


def check_options(opt, occlusion=None):
    if int(getattr(opt, "manual_depth_view", 1)) != 1:
        raise HnrError("depth_views: manual_depth_view=%r is not implemented (only 1: the expected depth of the pretrained estimator)" % opt.manual_depth_view)
    if float(getattr(opt, "manual_std_depth", 0.0) or 0.0) != 0.0:
        raise HnrError("depth_views: manual_std_depth != 0 (Gaussian depth sampling) is not implemented")
    if int(getattr(opt, "depth_occ", 0) or 0) > 0 and (occlusion is None or occlusion is False):
        raise HnrError("depth_views: depth_occ > 0 is not implemented without the keyword occlusion=True (the depth maps do not depend on it; the "
                       "embedding stage, MvsInit / init_cloud_from_mvs_depth, runs the occlusion test)")


def depth_views(batch, net, opt, occlusion=None):
    """The `manual_depth_view == 1` branch of `MvsPointsModel.gen_points` (models/mvs/mvs_points_model.py:300-341).  batch: the dataset item on the GPU
    -- images [1,N,3,H,W] (mvs_images, when present, is what the estimator sees), proj_mats [1,N,N,3,4] (row i: every view seen from view i),
    near_fars [1,N,2], near_fars_depth [1,2], intrinsics [1,N,3,3], w2cs [1,N,4,4] and optionally c2ws.  opt: init_view_num, depth_vid.
    Returns one dict per entry of depth_vid -- cam_xyz [H,W,3], confidence [H,W], points_mask [H,W], intrinsic, w2c[, c2w], image [3,H,W], depth [h,w] --
    the `views` of cloud_init.init_cloud_from_mvs_depth.  The feature maps are computed once, not once per entry of depth_vid.
    occlusion=True accepts opt.depth_occ > 0; nothing else changes: depth_occ does not enter this stage."""
    check_options(opt, occlusion)
    if not isinstance(net, MVSNet):
        raise HnrError("depth_views: net must be an mvs_depth.MVSNet")
    imgs = gpu_f32(batch["images"], "images")
    dimgs = gpu_f32(batch["mvs_images"], "mvs_images") if "mvs_images" in batch else imgs
    if dimgs.dim() != 5 or dimgs.shape[0] != 1 or dimgs.shape[2] != 3:
        raise HnrError("depth_views: images must be [1,N,3,H,W], got %s" % (tuple(dimgs.shape),))
    nv = int(opt.init_view_num)
    depth_vid = [int(v) for v in opt.depth_vid]
    if not 1 <= nv <= dimgs.shape[1] or not depth_vid or any(not 0 <= v < batch["proj_mats"].shape[1] for v in depth_vid):
        raise HnrError("depth_views: init_view_num=%d / depth_vid=%r do not fit %d views" % (nv, depth_vid, dimgs.shape[1]))
    H, W = int(dimgs.shape[-2]), int(dimgs.shape[-1])
    nfd = gpu_f32(batch["near_fars_depth"], "near_fars_depth")[0]
    interval = (nfd[1] - nfd[0]) / 192.
    depth_values = (nfd[0] + torch.arange(0, NUM_DEPTH, device=dimgs.device, dtype=torch.float32) * interval)[None, :]
    proj = gpu_f32(batch["proj_mats"], "proj_mats")[0, torch.as_tensor(depth_vid, dtype=torch.long, device=dimgs.device)][:, :nv]
    feats = net.image_features(dimgs[0, :nv])
    depth, conf, _, _ = net(dimgs[:, :nv].expand(len(depth_vid), -1, -1, -1, -1), proj, depth_values.expand(len(depth_vid), -1), features=feats)
    near_fars = batch["near_fars"].detach().float().cpu().numpy()[0]
    views = []
    for i, vid in enumerate(depth_vid):
        K = batch["intrinsics"][0, vid]
        cam, cf, mask = depth_points(depth[i], conf[i], H, W, near_fars[vid, 0], near_fars[vid, 1], K)
        v = dict(cam_xyz=cam, confidence=cf, points_mask=mask, intrinsic=K, w2c=batch["w2cs"][0, vid], image=imgs[0, vid], depth=depth[i])
        if "c2ws" in batch:
            v["c2w"] = batch["c2ws"][0, vid]
        views.append(v)
    return views
