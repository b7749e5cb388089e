"""Restatement of the learnable blur module (models/base_rendering_model.py:827-1020, faster_version, without the conv block) and of its backward in
torch on the CPU: plain formulas, autograd for the gradients, in fp32 or fp64.  Plus the seeded cases and the error bound the comparison tests share."""
import numpy as np
import torch
import torch.nn.functional as F

NAMES = ["learn_blur_kernel_block.%d.%s" % (2 * l, k) for l in range(4) for k in ("weight", "bias")]


def patch_rays(pn, ps):
    """[pn * pn, ps * ps] ray indices of the grid layout: ray = row * S + col, S = pn * ps; patches row-major (:845-852)."""
    S = pn * ps
    idx = np.arange(S * S).reshape(pn, ps, pn, ps).transpose(0, 2, 1, 3).reshape(pn * pn, ps * ps)
    return torch.from_numpy(np.ascontiguousarray(idx))


def forward(color, gt, weights, cfg, dtype, slope=0.01, predictor_dtype=None):
    """color, gt [rays, 3]; weights: the eight tensors in NAMES order; cfg: pn (< 0: -pn patches packed patch-major), ps, ks, norm, mode, bmode.
    Returns (new colours [rays, 3], final kernels [N, ks, ks]) in `dtype`.  predictor_dtype: the predictor, normalisation and blend in that dtype
    (cast in, cast out), the rest in `dtype`."""
    pn, ps, ks = cfg["pn"], cfg["ps"], cfg["ks"]
    N = -pn if pn < 0 else pn * pn
    idx = torch.arange(N * ps * ps).reshape(N, ps * ps) if pn < 0 else patch_rays(pn, ps)
    color, gt = color.to(dtype).reshape(-1, 3), gt.to(dtype).reshape(-1, 3)
    cp, gp = color[idx], gt[idx]                                       # [N, ps*ps, 3]
    pd = predictor_dtype or dtype
    x = torch.cat([gp.mean(dim=-1), cp.mean(dim=-1)], dim=-1).to(pd)   # :887-889: ground truth first
    W = [w.to(pd) for w in weights]
    for l in range(4):
        x = x @ W[2 * l].t() + W[2 * l + 1]
        x = F.leaky_relu(x, slope) if l < 3 else torch.sigmoid(x)
    kk = ks * ks
    k = x[:, :kk] / x[:, :kk].sum(dim=-1, keepdim=True) if cfg["norm"] == 0 else torch.softmax(x[:, :kk], dim=-1)
    if cfg["mode"] == 4:
        w = x[:, -1:]
        ident = torch.zeros_like(k)
        ident[:, kk // 2] = 1.0
        k = w * k + (1 - w) * ident
        k = k / k.sum(dim=-1, keepdim=True)
    else:
        assert cfg["mode"] == 0
    k = k.to(dtype).reshape(N, 1, ks, ks)
    img = cp.reshape(N, ps, ps, 3).permute(3, 0, 1, 2)                 # [3, N, ps, ps]
    conv = F.conv2d(img, k, padding=ks // 2, groups=N)
    km = k.detach() if cfg["bmode"] == 2 else k
    mask = F.conv2d(torch.ones_like(img), km, padding=ks // 2, groups=N)
    out = conv / (mask + 1e-10) if cfg["bmode"] == 0 else conv + (1 - mask) * img
    res = torch.zeros_like(color).index_put((idx.reshape(-1),), out.permute(1, 2, 3, 0).reshape(-1, 3))
    return res, k.reshape(N, ks, ks)


def run(color, gt, upstream, weights, cfg, dtype, slope=0.01):
    """Forward and backward of sum(out * upstream): dict of NumPy arrays out, kernels, grad_color and one gradient per name in NAMES."""
    c = color.detach().to(dtype).reshape(-1, 3).clone().requires_grad_(True)
    W = [w.detach().to(dtype).clone().requires_grad_(True) for w in weights]
    out, k = forward(c, gt, W, cfg, dtype, slope)
    (out * upstream.to(dtype).reshape(-1, 3)).sum().backward()
    res = dict(out=out.detach().numpy(), kernels=k.detach().numpy(), grad_color=c.grad.numpy())
    for n, w in zip(NAMES, W):
        res[n] = w.grad.numpy()
    return res


def make_weights(ps, ks, mode, seed):
    """nn.Linear's default initialisation for the four layers, seeded; the last layer's is scaled up so that the sigmoid outputs spread."""
    g = torch.Generator().manual_seed(seed)
    dims = [2 * ps * ps, 128, 128, 128, ks * ks + (1 if mode == 4 else 0)]
    ws = []
    for l in range(4):
        bound = 1.0 / np.sqrt(dims[l])
        ws.append((torch.rand((dims[l + 1], dims[l]), generator=g) * 2 - 1) * bound * (4.0 if l == 3 else 1.0))
        ws.append((torch.rand((dims[l + 1],), generator=g) * 2 - 1) * bound)
    return ws


def make_case(n_patches, ps, seed):
    g = torch.Generator().manual_seed(seed)
    R = n_patches * ps * ps
    return torch.rand((R, 3), generator=g), torch.rand((R, 3), generator=g), torch.randn((R, 3), generator=g)


def make_mlp(weights, device, slope=0.01):
    import torch.nn as nn
    dims = [(w.shape[1], w.shape[0]) for w in weights[0::2]]
    layers = []
    for l, (i, o) in enumerate(dims):
        layers += [nn.Linear(i, o), nn.LeakyReLU(slope, inplace=True) if l < 3 else nn.Sigmoid()]
    m = nn.Sequential(*layers)
    with torch.no_grad():
        for l in range(4):
            m[2 * l].weight.copy_(weights[2 * l]); m[2 * l].bias.copy_(weights[2 * l + 1])
    return m.to(device)


def bound_check(got, f32, f64, factor=4.0):
    """The project's bound: max |got - fp64| <= factor * max |fp32 restatement - fp64| per tensor, with a floor of one fp32 ulp of the tensor's
    largest magnitude (for tensors where the fp32 restatement happens to be exact).  Returns (ok, err_got, err_f32, floor)."""
    r = np.asarray(f64, dtype=np.float64)
    e_new = float(np.abs(np.asarray(got, dtype=np.float64).reshape(r.shape) - r).max())
    e_ref = float(np.abs(np.asarray(f32, dtype=np.float64).reshape(r.shape) - r).max())
    floor = float(np.spacing(np.float32(np.abs(r).max())))
    return e_new <= max(factor * e_ref, floor), e_new, e_ref, floor
