"""Restatement of RAFT's basic model (inference, test mode) in torch, written from the formulas of the paper and of include/hnr.h, switchable between
fp32 and fp64.  The reference's own modules force `.float()` in several places (corr.py, raft.py), so they cannot run in fp64; the tolerances of
tests/test_frame_weights_gpu.py are the error of this restatement's fp32 run against its fp64 run.  tests/test_frame_weights.py checks the fp32 run
against the recorded run of the reference (tests/golden/frame_weights.npz).

Also the seeded rule the weights of the fixture come from (they are not stored): `make_params(seed)`, driven by np.random.RandomState(seed) in the
order of `param_shapes()`.
"""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

ENC_BLOCKS = (("layer1.0", 64, 64, 1), ("layer1.1", 64, 64, 1), ("layer2.0", 64, 96, 2), ("layer2.1", 96, 96, 1), ("layer3.0", 96, 128, 2),
              ("layer3.1", 128, 128, 1))
BN_FIELDS = ("weight", "bias", "running_mean", "running_var")
SEED = 20


def _conv(d, name, cout, cin, kh, kw):
    d[name + ".weight"] = (cout, cin, kh, kw)
    d[name + ".bias"] = (cout,)


def _bn(d, name, ch):
    for f in BN_FIELDS:
        d[name + "." + f] = (ch,)


def param_shapes():
    """name -> shape, in the order the seeded rule draws them.  `norm3` of a stride-2 block of cnet is the same tensor as `downsample.1`."""
    d = OrderedDict()
    for enc, bn in (("fnet", False), ("cnet", True)):
        _conv(d, enc + ".conv1", 64, 3, 7, 7)
        if bn:
            _bn(d, enc + ".norm1", 64)
        for blk, cin, cout, stride in ENC_BLOCKS:
            p = "%s.%s" % (enc, blk)
            _conv(d, p + ".conv1", cout, cin, 3, 3)
            _conv(d, p + ".conv2", cout, cout, 3, 3)
            if bn:
                _bn(d, p + ".norm1", cout)
                _bn(d, p + ".norm2", cout)
            if stride != 1:
                _conv(d, p + ".downsample.0", cout, cin, 1, 1)
                if bn:
                    _bn(d, p + ".norm3", cout)
                    _bn(d, p + ".downsample.1", cout)
        _conv(d, enc + ".conv2", 256, 128, 1, 1)
    u = "update_block."
    _conv(d, u + "encoder.convc1", 256, 324, 1, 1)
    _conv(d, u + "encoder.convc2", 192, 256, 3, 3)
    _conv(d, u + "encoder.convf1", 128, 2, 7, 7)
    _conv(d, u + "encoder.convf2", 64, 128, 3, 3)
    _conv(d, u + "encoder.conv", 126, 256, 3, 3)
    for n in ("z1", "r1", "q1"):
        _conv(d, u + "gru.conv" + n, 128, 384, 1, 5)
    for n in ("z2", "r2", "q2"):
        _conv(d, u + "gru.conv" + n, 128, 384, 5, 1)
    _conv(d, u + "flow_head.conv1", 256, 128, 3, 3)
    _conv(d, u + "flow_head.conv2", 2, 256, 3, 3)
    _conv(d, u + "mask.0", 256, 128, 3, 3)
    _conv(d, u + "mask.2", 576, 256, 1, 1)
    return d


def make_params(seed=SEED):
    """The fixture's weights (fp32 tensors): the encoders' convolutions N(0, 2/fan_out) (their initialisation in the reference), the update block's
    convolutions N(0, 1/(3 fan_in)) (the variance of torch's default initialisation, which the reference leaves them with), biases +-0.2, batch-norm
    weight and variance in 0.5 .. 1.5, mean and bias +-0.2.  The stream of RandomState(seed) is frozen, so the values are too.
    (N(0, 2/fan_out) on the update block as well makes the flow head's two output channels sum 2304 inputs at a standard deviation of 0.33: the
    recurrence then moves hundreds of pixels per iteration, the flow reaches 4400 px after 20 and fp32 and fp64 differ by pixels -- measured by
    tests/golden/make_golden_frame_weights.py, whose assertions that rule cannot meet.)"""
    rs = np.random.RandomState(seed)
    sd = OrderedDict()
    for name, shape in param_shapes().items():
        if ".downsample.1." in name:
            sd[name] = sd[name.replace(".downsample.1.", ".norm3.")]
        elif len(shape) == 4 and name.startswith("update_block."):
            sd[name] = rs.standard_normal(shape) * np.sqrt(1.0 / (3.0 * shape[1] * shape[2] * shape[3]))
        elif len(shape) == 4:
            sd[name] = rs.standard_normal(shape) * np.sqrt(2.0 / (shape[0] * shape[2] * shape[3]))
        elif name.endswith(".running_var") or (name.endswith(".weight") and ".norm" in name):
            sd[name] = rs.uniform(0.5, 1.5, shape)
        else:
            sd[name] = rs.uniform(-0.2, 0.2, shape)
    return OrderedDict((k, torch.from_numpy(np.asarray(v, dtype=np.float32))) for k, v in sd.items())


def make_images(shape, seed=SEED):
    """image1 [3,H,W] uint8 of 16 grey levels, image2 = image1 rolled by (2, -3) pixels plus noise of -1 .. 1."""
    H, W = shape
    rs = np.random.RandomState(seed + 1000 + H + W)
    im1 = (rs.randint(0, 16, (3, H, W)) * 17).astype(np.int64)
    im2 = np.clip(np.roll(im1, (2, -3), axis=(1, 2)) + rs.randint(-1, 2, (3, H, W)), 0, 255)
    return im1.astype(np.uint8), im2.astype(np.uint8)


def cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def _c(sd, name, x, stride=1, padding=0):
    return F.conv2d(x, sd[name + ".weight"], sd[name + ".bias"], stride=stride, padding=padding)


def _norm(sd, name, x, bn):
    if bn:
        return F.batch_norm(x, sd[name + ".running_mean"], sd[name + ".running_var"], sd[name + ".weight"], sd[name + ".bias"], False, 0.0, 1e-5)
    return F.instance_norm(x, eps=1e-5)


def encoder(sd, enc, x, bn):
    """x [N,3,H,W] already scaled to -1 .. 1 -> [N,256,H/8,W/8]; instance norm (bn False) or eval-mode batch norm."""
    x = torch.relu(_norm(sd, enc + ".norm1", _c(sd, enc + ".conv1", x, 2, 3), bn))
    for blk, _, _, stride in ENC_BLOCKS:
        p = "%s.%s" % (enc, blk)
        y = torch.relu(_norm(sd, p + ".norm1", _c(sd, p + ".conv1", x, stride, 1), bn))
        y = torch.relu(_norm(sd, p + ".norm2", _c(sd, p + ".conv2", y, 1, 1), bn))
        if stride != 1:
            x = _norm(sd, p + ".norm3", _c(sd, p + ".downsample.0", x, stride, 0), bn)
        x = torch.relu(x + y)
    return _c(sd, enc + ".conv2", x)


def scale_image(img_u8, dtype):
    return 2 * (torch.as_tensor(img_u8).to(dtype) / 255.0) - 1.0


def corr_pyramid(f1, f2):
    """f1, f2 [256,h,w] -> four levels [h*w,h_l,w_l]."""
    c, h, w = f1.shape
    corr = torch.matmul(f1.reshape(c, h * w).t(), f2.reshape(c, h * w)) / torch.sqrt(torch.tensor(float(c)).to(f1.dtype))
    levels = [corr.reshape(h * w, 1, h, w)]
    for _ in range(3):
        levels.append(F.avg_pool2d(levels[-1], 2, stride=2))
    return [l[:, 0] for l in levels]


def lookup(levels, coords):
    """coords [2,h,w] (x, y) -> [324,h,w]: window (i, j) -> tap (x/2^l + i - 4, y/2^l + j - 4), channel l*81 + i*9 + j; bilinear, align_corners,
    zero outside."""
    _, h, w = coords.shape
    dt = coords.dtype
    c = coords.permute(1, 2, 0).reshape(h * w, 1, 1, 2)
    off = torch.linspace(-4, 4, 9).to(dt).to(coords.device)
    delta = torch.stack(torch.meshgrid(off, off, indexing="ij"), dim=-1)[None]            # [1,9,9,2]: delta[i][j] = (off_i, off_j), added to (x, y)
    out = []
    for l, lev in enumerate(levels):
        H, W = lev.shape[-2:]
        pos = c / 2 ** l + delta
        gx, gy = 2 * pos[..., 0:1] / (W - 1) - 1, 2 * pos[..., 1:2] / (H - 1) - 1
        s = F.grid_sample(lev[:, None], torch.cat([gx, gy], dim=-1), align_corners=True)
        out.append(s.reshape(h, w, 81))
    return torch.cat(out, dim=-1).permute(2, 0, 1).contiguous()


def update(sd, net, inp, corr, flow):
    """One application of the update block on [1,C,h,w] tensors -> (net, mask, delta_flow)."""
    u = "update_block."
    cor = torch.relu(_c(sd, u + "encoder.convc1", corr))
    cor = torch.relu(_c(sd, u + "encoder.convc2", cor, 1, 1))
    flo = torch.relu(_c(sd, u + "encoder.convf1", flow, 1, 3))
    flo = torch.relu(_c(sd, u + "encoder.convf2", flo, 1, 1))
    mot = torch.cat([torch.relu(_c(sd, u + "encoder.conv", torch.cat([cor, flo], dim=1), 1, 1)), flow], dim=1)
    x = torch.cat([inp, mot], dim=1)
    for n, pad in (("1", (0, 2)), ("2", (2, 0))):
        hx = torch.cat([net, x], dim=1)
        z = torch.sigmoid(_c(sd, u + "gru.convz" + n, hx, 1, pad))
        r = torch.sigmoid(_c(sd, u + "gru.convr" + n, hx, 1, pad))
        q = torch.tanh(_c(sd, u + "gru.convq" + n, torch.cat([r * net, x], dim=1), 1, pad))
        net = (1 - z) * net + z * q
    delta = _c(sd, u + "flow_head.conv2", torch.relu(_c(sd, u + "flow_head.conv1", net, 1, 1)), 1, 1)
    mask = .25 * _c(sd, u + "mask.2", torch.relu(_c(sd, u + "mask.0", net, 1, 1)))
    return net, mask, delta


def upsample(flow, mask):
    """flow [1,2,h,w], mask [1,576,h,w] -> [1,2,8h,8w]: convex combination of the 3x3 neighbourhood of 8 * flow."""
    _, _, h, w = flow.shape
    m = torch.softmax(mask.reshape(1, 1, 9, 8, 8, h, w), dim=2)
    nb = F.unfold(8 * flow, [3, 3], padding=1).reshape(1, 2, 9, 1, 1, h, w)
    up = torch.sum(m * nb, dim=2)                                                          # [1,2,8,8,h,w]
    return up.permute(0, 1, 4, 2, 5, 3).reshape(1, 2, 8 * h, 8 * w)


def grid(h, w, dtype):
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    return torch.stack([xs, ys]).to(dtype)


def forward(sd, im1_u8, im2_u8, iters, dtype=torch.float32, keep=()):
    """-> dict: flow_low [2,h,w], flow_up [2,H,W], fmaps [2,256,h,w], cnet [256,h,w] (tanh | relu applied), levels, and for every iteration index in
    `keep` a dict of that iteration's inputs and outputs (net_in, coords_in, corr, net, delta, mask)."""
    sd = cast(sd, dtype)
    with torch.no_grad():
        x1, x2 = scale_image(im1_u8, dtype)[None], scale_image(im2_u8, dtype)[None]
        fmaps = encoder(sd, "fnet", torch.cat([x1, x2]), False)
        cn = encoder(sd, "cnet", x1, True)
        net, inp = torch.tanh(cn[:, :128]), torch.relu(cn[:, 128:])
        levels = corr_pyramid(fmaps[0], fmaps[1])
        h, w = fmaps.shape[-2:]
        coords0 = grid(h, w, dtype)
        coords1 = coords0.clone()
        out = dict(fmaps=fmaps, cnet=torch.cat([net, inp], dim=1)[0], levels=levels, inp=inp[0], steps={})
        for it in range(iters):
            corr = lookup(levels, coords1)
            net_in, coords_in = net, coords1
            net, mask, delta = update(sd, net, inp, corr[None], (coords1 - coords0)[None])
            coords1 = coords1 + delta[0]
            if it in keep:
                out["steps"][it] = dict(net_in=net_in[0], coords_in=coords_in, corr=corr, net=net[0], delta=delta[0], mask=mask[0], coords=coords1)
        out["flow_low"] = coords1 - coords0
        out["flow_up"] = upsample(out["flow_low"][None], mask)[0]
        out["mask"] = mask[0]
    return out
