"""Restatement of the pretrained depth estimator (models/depth_estimators/mvsnet.py, module.py: `MVSNet(refine=False)` in eval mode) and of the tail of
`MvsPointsModel.gen_points` for `manual_depth_view=1`, `manual_std_depth=0` (models/mvs/mvs_points_model.py:329-337, mvs_utils.ndc_2_cam) as plain torch
functional ops, in a dtype of the caller's choice (fp64: the truth the GPU tests measure against; fp32: the yardstick of what fp32 arithmetic in another
summation order costs).  No code of the package and none of the reference is imported: tests/test_mvs_depth.py pins it, in fp32, to the reference's own
outputs recorded in tests/golden/mvs_depth.npz (the reference itself cannot run in fp64: `homo_warping` builds an fp32 pixel grid).

  feature_net    seven conv (no bias) -> batch_norm (eval) -> relu, then `feature` (3x3, bias)
  cost_volume    homo_warping per view (the align_corners=True normalisation sampled with grid_sample's default align_corners=False: kept), then
                 sum f^2 / V - (sum f / V)^2
  cost_reg       CostRegNet; the skip is added after the activation
  depth_head     softmax over D, expected depth, idx = trunc(expected index), confidence = the four probabilities idx-1 .. idx+2
  depth_points   nearest upsampling, near <= d <= far, clamp((d - near) / (far - near), 0, 1) (what sample_by_gau is at std 0), depth2point / ndc_2_cam
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
FEATURE_STRIDES = (1, 1, 2, 1, 1, 2, 1)                           # conv0 .. conv6 of FeatureNet; pad = kernel // 2
REG_STRIDES = (1, 2, 1, 2, 1, 2, 1)                               # conv0 .. conv6 of CostRegNet


def _t(a, dtype):
    return (a.detach() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(dtype)


def state(sd, dtype):
    return {k: _t(v, dtype) for k, v in sd.items() if not k.endswith("num_batches_tracked")}


def _bn(x, sd, p):
    return F.batch_norm(x, sd[p + "running_mean"], sd[p + "running_var"], sd[p + "weight"], sd[p + "bias"], False, 0.0, EPS)


def feature_net(sd, images, dtype=torch.float64, prefix="feature."):
    """images [V,3,H,W] -> [V,32,h,w] in `dtype`."""
    sd, images = state(sd, dtype), _t(images, dtype)
    outs = []
    for x in images[:, None]:                                     # one view at a time, as the reference runs it
        for i, stride in enumerate(FEATURE_STRIDES):
            w = sd["%sconv%d.conv.weight" % (prefix, i)]
            x = F.relu(_bn(F.conv2d(x, w, None, stride=stride, padding=w.shape[-1] // 2), sd, "%sconv%d.bn." % (prefix, i)))
        outs.append(F.conv2d(x, sd[prefix + "feature.weight"], sd[prefix + "feature.bias"], padding=1))
    return torch.cat(outs, dim=0)


def warp(feat, proj, depth_values):
    """homo_warping for one view: feat [32,h,w], proj [3,4] (or [4,4]), depth_values [D] -> [32,D,h,w], in feat's dtype."""
    dtype = feat.dtype
    C, h, w = feat.shape
    D = depth_values.shape[0]
    rot, trans = proj[:3, :3], proj[:3, 3:4]
    y, x = torch.meshgrid(torch.arange(0, h, dtype=dtype), torch.arange(0, w, dtype=dtype), indexing="ij")
    xyz = torch.stack((x.reshape(-1), y.reshape(-1), torch.ones(h * w, dtype=dtype)))
    rot_depth_xyz = torch.matmul(rot, xyz).unsqueeze(1).repeat(1, D, 1) * depth_values.view(1, D, 1)
    p = rot_depth_xyz + trans.view(3, 1, 1)
    xy = p[:2] / p[2:3]
    grid = torch.stack((xy[0] / ((w - 1) / 2) - 1, xy[1] / ((h - 1) / 2) - 1), dim=2)
    out = F.grid_sample(feat[None], grid.view(1, D * h, w, 2), mode="bilinear", padding_mode="zeros", align_corners=False)
    return out.view(C, D, h, w)


def cost_volume(feats, proj, depth_values, dtype=torch.float64):
    """feats [V,32,h,w], proj [V,3,4] (or [V,4,4]), depth_values [D] -> the variance volume [32,D,h,w] in `dtype`, views ascending."""
    feats, proj, depth_values = _t(feats, dtype), _t(proj, dtype), _t(depth_values, dtype)
    V = feats.shape[0]
    s = q = 0
    for v in range(V):
        wv = warp(feats[v], proj[v], depth_values)
        s, q = s + wv, q + wv ** 2
    return q / V - (s / V) ** 2


def cost_reg(sd, volume, dtype=torch.float64, prefix="cost_regularization.", want_all=False):
    """volume [32,D,h,w] -> logits [D,h,w] in `dtype` (want_all: every layer's output, for stage-wise comparisons)."""
    sd, x = state(sd, dtype), _t(volume, dtype)[None]
    c = []
    for i, stride in enumerate(REG_STRIDES):
        x = F.relu(_bn(F.conv3d(x, sd["%sconv%d.conv.weight" % (prefix, i)], None, stride=stride, padding=1), sd, "%sconv%d.bn." % (prefix, i)))
        c.append(x)
    for name, skip in (("conv7", c[4]), ("conv9", c[2]), ("conv11", c[0])):
        y = F.conv_transpose3d(x, sd["%s%s.0.weight" % (prefix, name)], None, stride=2, padding=1, output_padding=1)
        x = skip + F.relu(_bn(y, sd, "%s%s.1." % (prefix, name)))
        c.append(x)
    out = F.conv3d(x, sd[prefix + "prob.weight"], sd[prefix + "prob.bias"], padding=1)[0, 0]
    return (out, [t[0] for t in c]) if want_all else out


def depth_head(logits, depth_values, dtype=torch.float64):
    """logits [D,h,w], depth_values [D] -> (depth [h,w], confidence [h,w], prob [D,h,w], expected index [h,w] before truncation) in `dtype`."""
    logits, depth_values = _t(logits, dtype), _t(depth_values, dtype)
    D = logits.shape[0]
    p = F.softmax(logits, dim=0)
    depth = torch.sum(p * depth_values.view(D, 1, 1), 0)
    sum4 = 4 * F.avg_pool3d(F.pad(p[None, None], pad=(0, 0, 0, 0, 1, 2)), (4, 1, 1), stride=1, padding=0)[0, 0]
    fidx = torch.sum(p * torch.arange(D, dtype=dtype).view(D, 1, 1), 0)
    conf = torch.gather(sum4, 0, fidx.long()[None])[0]
    return depth, conf, p, fidx


def depth_points(depth, conf, H, W, near, far, intrinsic=None, dtype=torch.float64, kt_inv=None):
    """depth, conf [h,w] -> (cam_xyz [H,W,3], confidence [H,W], points_mask [H,W] bool, upsampled depth [H,W]).  kt_inv: inverse(K^T) when the
    caller has formed it (the kernels take the fp32 one); None: torch.inverse in `dtype`, as ndc_2_cam does."""
    depth, conf = _t(depth, dtype), _t(conf, dtype)
    near, far = _t(np.asarray(near), dtype), _t(np.asarray(far), dtype)
    d = F.interpolate(depth[None, None], size=[H, W], mode="nearest")[0, 0]
    c = F.interpolate(conf[None, None], size=[H, W], mode="nearest")[0, 0]
    mask = torch.logical_and(d >= near, d <= far)
    z = torch.clamp((d - near) / (far - near), min=0.0, max=1.0)
    vx = torch.arange(W, dtype=dtype) / (W - 1)
    vy = torch.arange(H, dtype=dtype) / (H - 1)
    vy, vx = torch.meshgrid(vy, vx, indexing="ij")
    ndc = torch.stack([vx, vy, z], dim=-1)
    cam_z = ndc[..., 2:3] * (far - near) + near
    cam_xy = ndc[..., :2] * torch.tensor([[W - 1, H - 1]]) * cam_z
    M = torch.inverse(_t(intrinsic, dtype).t()) if kt_inv is None else _t(kt_inv, dtype)
    return torch.cat([cam_xy, cam_z], dim=-1) @ M, c, mask, d


def mvsnet(sd, imgs, proj, depth_values, dtype=torch.float64, features=None):
    """imgs [V,3,H,W], proj [V,3,4], depth_values [D] -> dict(features, volume, logits, depth, confidence, prob, fidx) of one reference view."""
    feats = feature_net(sd, imgs, dtype) if features is None else _t(features, dtype)
    vol = cost_volume(feats, proj, depth_values, dtype)
    logits = cost_reg(sd, vol, dtype)
    depth, conf, prob, fidx = depth_head(logits, depth_values, dtype)
    return dict(features=feats, volume=vol, logits=logits, depth=depth, confidence=conf, prob=prob, fidx=fidx)


def abs_err(a, b):
    """max|a - b|"""
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def ulp_of_max(b):
    """one fp32 ulp at the tensor's largest magnitude"""
    return float(np.spacing(np.float32(np.abs(np.asarray(b, np.float64)).max())))
