"""Restatement of the init checkpoint's two networks as plain torch functional ops, in a dtype of the caller's choice (fp64: the truth the GPU tests
measure against; fp32: the yardstick of what fp32 arithmetic in another summation order costs).  No code of the package and none of the reference is
imported: tests/test_mvs_init.py pins it, in fp64, to the reference's own outputs recorded in tests/golden/mvs_init.npz.

  feature_pyramid   FeatureNet(intermediate=True) in eval mode: conv (no bias) -> (x - running_mean) * mul + bias -> leaky_relu(0.01),
                    mul = rsqrt(running_var + eps) * (|weight| + eps), eps = 1e-5 (the activated batch norm's inference arithmetic); toplayer 1x1 with bias
  query_embedding   run/train_ft.py:759-760 for "imgfeat_0_0123 dir_0 point_conf", shading_feature_mlp_layer0 = 1, pointdir_w = True
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
LAYERS = (("conv0", ((3, 1), (3, 1))), ("conv1", ((5, 2), (3, 1), (3, 1))), ("conv2", ((5, 2), (3, 1), (3, 1))))          # (kernel, stride)


def _t(a, dtype):
    return (a.detach() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(dtype)


def state(sd, dtype):
    return {k: _t(v, dtype) for k, v in sd.items()}


def abn(x, sd, prefix):
    mul = torch.rsqrt(sd[prefix + "running_var"] + EPS) * (sd[prefix + "weight"].abs() + EPS)
    c = lambda v: v.view(1, -1, 1, 1)
    return F.leaky_relu((x - c(sd[prefix + "running_mean"])) * c(mul) + c(sd[prefix + "bias"]), 0.01)


def feature_pyramid(sd, images, dtype=torch.float64, prefix="FeatureNet."):
    """images [V,3,H,W] -> (x1 [V,8,H,W], x2 [V,16,H2,W2], x3 [V,32,H4,W4]) in `dtype`."""
    sd, x = state(sd, dtype), _t(images, dtype)
    outs = []
    for name, layers in LAYERS:
        for i, (ks, stride) in enumerate(layers):
            p = "%s%s.%d." % (prefix, name, i)
            x = abn(F.conv2d(x, sd[p + "conv.weight"], None, stride=stride, padding=ks // 2), sd, p + "bn.")
        outs.append(x)
    outs[2] = F.conv2d(outs[2], sd[prefix + "toplayer.weight"], sd[prefix + "toplayer.bias"])
    return tuple(outs)


def premlp(sd, rows, prefix="premlp."):
    h = F.leaky_relu(F.linear(rows, sd[prefix + "0.weight"], sd[prefix + "0.bias"]), 0.01)
    return F.leaky_relu(F.linear(h, sd[prefix + "2.weight"], sd[prefix + "2.bias"]), 0.01)


def project(xyz, w2c, K, dtype=torch.float64):
    """(cam [n,3], grid [n,2] in pixels) as train_ft.py:759 and homo_warp_nongrid form them."""
    xyz, w2c, K = _t(xyz, dtype), _t(w2c, dtype), _t(K, dtype)
    cam = (torch.cat([xyz, torch.ones_like(xyz[..., -1:])], dim=-1) @ w2c.transpose(0, 1))[..., :3]
    return cam, ((cam / cam[..., 2:3]) @ K.transpose(0, 1))[..., :2]


def query_rows(xyz, image, maps, c2w, w2c, K, dtype=torch.float64):
    """(rows [n,63] = [x1 | x2 | x3 | colour | dir | 1], mask [n] bool): what query_embedding hands to premlp."""
    image, c2w_t, w2c_t = _t(image, dtype), _t(c2w, dtype), _t(w2c, dtype)
    H, W = image.shape[-2:]
    cam, grid = project(xyz, w2c, K, dtype)
    mask = (grid[:, 0] >= 0) & (grid[:, 0] <= W - 1) & (grid[:, 1] >= 0) & (grid[:, 1] <= H - 1)
    g = grid[mask].clone()
    g[:, 0] = g[:, 0] / ((W - 1.0) / 2.0) - 1.0
    g[:, 1] = g[:, 1] / ((H - 1.0) / 2.0) - 1.0

    def sample(src):
        w = F.grid_sample(_t(src, dtype)[None], g[None, None], mode="bilinear", padding_mode="zeros", align_corners=True)[0, :, 0].t()
        full = torch.zeros((cam.shape[0], src.shape[0]), dtype=dtype)
        full[mask] = w
        return full
    cpc = (c2w_t[None, :, 3] @ w2c_t.transpose(0, 1))[..., :3]
    d = cam - cpc
    d = d / (torch.linalg.norm(d, dim=-1, keepdim=True) + 1e-6)
    d = d @ c2w_t[:3, :3].transpose(0, 1)
    rows = torch.cat([sample(m) for m in maps] + [sample(image), d, torch.ones((cam.shape[0], 1), dtype=dtype)], dim=-1)
    return rows, mask


def query_embedding(sd, xyz, image, c2w, w2c, K, dtype=torch.float64, maps=None):
    """(embedding [n,32], color [n,3], dir [n,3], conf [n,1], rows [n,63], mask [n]) in `dtype`; maps: the view's (x1, x2, x3) [C,Hl,Wl] when already there."""
    if maps is None:
        maps = [m[0] for m in feature_pyramid(sd, _t(image, dtype)[None], dtype)]
    rows, mask = query_rows(xyz, image, maps, c2w, w2c, K, dtype)
    return premlp(state(sd, dtype), rows), rows[:, 56:59], rows[:, 59:62], rows[:, 62:63], rows, mask


def rel_err(a, b):
    """max|a - b| / max|b|"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())
