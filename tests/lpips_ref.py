"""Restatement of LPIPS v0.1 (`lpips.LPIPS(net, version='0.1')`, eval mode, lpips=True, spatial=False) on torchvision's AlexNet / VGG-16 `features`, in
plain torch, switchable between fp32 and fp64.  Written from the published packages' definition (neither package is available here: not checked against
their source or their weight files); tests/test_lpips.py checks it against an independent nn.Sequential formulation.  The tolerances of
tests/test_lpips_gpu.py are the error of this restatement's fp32 run against its fp64 run.

Also the seeded rule the synthetic weights come from (they are not stored): `make_params(net, seed)`.
"""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
EPS = 1e-10
# (index in `features`, cin, cout, kernel, stride, padding)
ALEX = ((0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1), (10, 256, 256, 3, 1, 1))
VGG = tuple((i, cin, cout, 3, 1, 1) for i, cin, cout in (
    (0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256), (17, 256, 512), (19, 512, 512), (21, 512, 512),
    (24, 512, 512), (26, 512, 512), (28, 512, 512)))
CONVS = {"alex": ALEX, "vgg": VGG}
TAP_CONV = {"alex": (0, 3, 6, 8, 10), "vgg": (2, 7, 14, 21, 28)}            # the convolution whose ReLU is tap k
POOL_AFTER = {"alex": ((0, 3), (3, 3)), "vgg": ((2, 2), (7, 2), (14, 2), (21, 2))}   # (after the ReLU of conv i, kernel); stride 2, floor, no padding
TAP_CHANNELS = {"alex": (64, 192, 384, 256, 256), "vgg": (64, 128, 256, 512, 512)}
SLICE_ENDS = {"alex": (2, 5, 8, 10, 12), "vgg": (4, 9, 16, 23, 30)}


def param_shapes(net):
    d = OrderedDict()
    for i, cin, cout, k, _, _ in CONVS[net]:
        d["features.%d.weight" % i] = (cout, cin, k, k)
        d["features.%d.bias" % i] = (cout,)
    for k, c in enumerate(TAP_CHANNELS[net]):
        d["lin%d.model.1.weight" % k] = (1, c, 1, 1)
    return d


def make_params(net, seed, zero_bias=False):
    """Seeded synthetic weights (float32): convolutions He-scaled normal N(0, 2 / fan_in) with biases N(0, 0.05^2) (zero_bias: 0), so the activations
    neither die nor blow up through thirteen layers; `lin` = |N(0, 1)| / C, non-negative as the published ones are."""
    rs = np.random.RandomState(seed)
    out = OrderedDict()
    for name, shape in param_shapes(net).items():
        if name.startswith("lin"):
            v = np.abs(rs.standard_normal(shape)) / shape[1]
        elif name.endswith("weight"):
            v = rs.standard_normal(shape) * np.sqrt(2.0 / (shape[1] * shape[2] * shape[3]))
        else:
            v = rs.standard_normal(shape) * (0.0 if zero_bias else 0.05)
        out[name] = torch.from_numpy(v.astype(np.float32))
    return out


def cast(params, dtype):
    return {k: v.to(dtype) for k, v in params.items()}


def backbone(params):
    return {k: v for k, v in params.items() if k.startswith("features.")}


def lin_file(params):
    return {k: v for k, v in params.items() if k.startswith("lin")}


def lpips_state_dict(net, params, shift=SHIFT, scale=SCALE):
    """The same weights under the keys of `lpips.LPIPS.state_dict()`."""
    sd = OrderedDict()
    sd["scaling_layer.shift"] = torch.tensor(shift, dtype=torch.float32).reshape(1, 3, 1, 1)
    sd["scaling_layer.scale"] = torch.tensor(scale, dtype=torch.float32).reshape(1, 3, 1, 1)
    for i, *_ in CONVS[net]:
        j = 1 + next(s for s, end in enumerate(SLICE_ENDS[net]) if i < end)
        for f in ("weight", "bias"):
            sd["net.slice%d.%d.%s" % (j, i, f)] = params["features.%d.%s" % (i, f)]
    for k in range(5):
        sd["lin%d.model.1.weight" % k] = params["lin%d.model.1.weight" % k]
    for k in range(5):
        sd["lins.%d.model.1.weight" % k] = params["lin%d.model.1.weight" % k]
    return sd


def byte_values(dtype, shift=SHIFT, scale=SCALE):
    """[3,256]: network input of byte b in network channel c.  evaluate.py: float32(img) / 255.0, * 2 - 1.0 (numpy); ScalingLayer: (x - shift) / scale."""
    nd = np.float32 if dtype == torch.float32 else np.float64
    v = np.arange(256).astype(nd) / nd(255.0) * nd(2) - nd(1.0)
    v = torch.from_numpy(v)
    sh, sc = torch.tensor(shift).to(dtype), torch.tensor(scale).to(dtype)          # (float32 constants, as the package registers them)
    return (v[None, :] - sh[:, None]) / sc[:, None]


def prepare8(img8, gt8, dtype, channel_order="bgr", shift=SHIFT, scale=SCALE):
    """two [h,w,3] uint8 RGB arrays -> [2,3,h,w]; bgr: network channel c reads byte 2 - c."""
    table = byte_values(dtype, shift, scale)
    out = []
    for im in (img8, gt8):
        im = torch.from_numpy(np.ascontiguousarray(im)).long()
        if channel_order == "bgr":
            im = im.flip(-1)
        out.append(torch.stack([table[c][im[..., c]] for c in range(3)]))
    return torch.stack(out)


def scaling_layer(x, shift=SHIFT, scale=SCALE):
    sh, sc = torch.tensor(shift).to(x.dtype).reshape(1, 3, 1, 1), torch.tensor(scale).to(x.dtype).reshape(1, 3, 1, 1)
    return (x - sh) / sc


def features(net, params, x):
    """x [N,3,h,w] (the ScalingLayer's output) -> the five taps; params already in x's dtype."""
    taps, pools = [], dict(POOL_AFTER[net])
    for i, _, _, _, s, p in CONVS[net]:
        x = F.relu(F.conv2d(x, params["features.%d.weight" % i], params["features.%d.bias" % i], stride=s, padding=p))
        if i in TAP_CONV[net]:
            taps.append(x)
        if i in pools:
            x = F.max_pool2d(x, pools[i], 2)
    return taps


def normalize_tensor(f):
    return f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True)) + EPS)


def score(params, taps0, taps1):
    """taps of image 0 and of image 1 ([1,C,h,w] each) -> (d, [r_0 .. r_4]) as 0-dim tensors of the taps' dtype."""
    rs = []
    for k in range(5):
        diff = (normalize_tensor(taps0[k]) - normalize_tensor(taps1[k])) ** 2
        s = F.conv2d(diff, params["lin%d.model.1.weight" % k])
        rs.append(s.mean([2, 3]).reshape(()))
    d = rs[0]
    for r in rs[1:]:
        d = d + r
    return d, rs


def lpips_from_input(net, params, x):
    """x [2,3,h,w] (both images, prepared) -> row [d, r_0 .. r_4]"""
    taps = features(net, params, x)
    d, rs = score(params, [t[0:1] for t in taps], [t[1:2] for t in taps])
    return torch.stack([d] + rs)


def forward(net, params, in0, in1, dtype, shift=SHIFT, scale=SCALE):
    """The package's forward on [1,3,H,W] inputs in [-1, 1] -> row [d, r_0 .. r_4]."""
    x = torch.cat([scaling_layer(in0.to(dtype), shift, scale), scaling_layer(in1.to(dtype), shift, scale)])
    return lpips_from_input(net, cast(params, dtype), x)


def pair8(net, params, img8, gt8, dtype, channel_order="bgr", shift=SHIFT, scale=SCALE):
    """What run/evaluate.py computes for a pair of 8-bit RGB images (channel_order="bgr": as it feeds them) -> row [d, r_0 .. r_4]."""
    return lpips_from_input(net, cast(params, dtype), prepare8(img8, gt8, dtype, channel_order, shift, scale))


def seeded_images(h, w, seed):
    """(a, b, c): b = a plus noise of a few levels on a smooth image (a close pair, the case LPIPS is used for); c = a with a few pixels changed."""
    rs = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    base = np.stack([0.5 + 0.4 * np.sin(7 * yy + 3 * xx), 0.5 + 0.4 * np.cos(5 * xx - 2 * yy), 0.2 + 0.6 * yy * xx], -1)
    a = np.clip((base + rs.normal(0, 0.08, base.shape)) * 255, 0, 255).astype(np.uint8)
    b = np.clip(a.astype(np.int64) + rs.randint(-12, 13, a.shape), 0, 255).astype(np.uint8)
    c = a.copy()
    for _ in range(4):
        c[rs.randint(h), rs.randint(w)] = rs.randint(0, 256, 3)
    return a, b, c
