"""Restatement of the patch SSIM term (include/hnr.h, "Patch SSIM term of the training loss"; csrc/ssim_loss.hip) in torch on the CPU.

`ssim_term` is the definition evaluated the way the kernel evaluates it: the two 7-tap "valid" passes, the per-window s with the three coefficients
of its ANALYTIC gradient, the two transposed passes, d(sum s)/dX = (G_a + (2 X) G_b) + Y G_c.  In float64 it is the reference value; in float32
every operation is a torch CPU op of its own, in the header's order (taps added in ascending order starting from zero, products first, no FMA), so
it is what the device computes up to the order of the fp64 sum of the s values.  `ssim_expr` is the same term as one differentiable torch expression
(for autograd).  `make_case` builds the test inputs of tests/test_ssim_loss*.py."""
import numpy as np
import torch

C1, C2 = 1e-4, 9e-4
WIN = 7


def window():
    """The seven fp32 window values the library is handed (losses.ssim_window restated: the ops of pytorch_msssim's _fspecial_gauss_1d)."""
    coords = torch.arange(WIN, dtype=torch.float32)
    coords -= WIN // 2
    g = torch.exp(-(coords ** 2) / (2 * 1.5 ** 2))
    g /= g.sum()
    return g


def n_patches(patch_num, layout):
    return int(patch_num) if layout == "patch_major" else int(patch_num) ** 2


def to_patches(t, patch_num, ps, layout):
    """[R, C] -> [n, C, ps, ps] (a copy)"""
    C = t.shape[-1]
    if layout == "patch_major":
        return t.reshape(patch_num, ps, ps, C).permute(0, 3, 1, 2).contiguous()
    return t.reshape(patch_num, ps, patch_num, ps, C).permute(0, 2, 4, 1, 3).reshape(patch_num * patch_num, C, ps, ps).contiguous()


def from_patches(p, patch_num, ps, layout):
    """[n, C, ps, ps] -> [R, C]"""
    C = p.shape[1]
    if layout == "patch_major":
        return p.permute(0, 2, 3, 1).reshape(-1, C).contiguous()
    return p.reshape(patch_num, patch_num, C, ps, ps).permute(0, 3, 1, 4, 2).reshape(-1, C).contiguous()


def _valid(q, g, dim):
    W = q.shape[dim] - (WIN - 1)
    acc = torch.zeros_like(q.narrow(dim, 0, W))
    for i in range(WIN):
        acc = acc + g[i] * q.narrow(dim, i, W)
    return acc


def _transposed(k, g, dim, ps):
    """out(y) = sum_{i <= min(6, y)} g[i] k(y - i), k zero beyond its W entries"""
    shape = list(k.shape)
    shape[dim] = ps - k.shape[dim]
    kp = torch.cat([k, torch.zeros(shape, dtype=k.dtype)], dim=dim)
    out = torch.zeros_like(kp)
    for i in range(WIN):
        o = out.narrow(dim, i, ps - i)
        o.copy_(o + g[i] * kp.narrow(dim, 0, ps - i))
    return out


def _windows(X, Y, g):
    """s and (a, b, c) per window, [n, C, W, W], in the header's operation order"""
    M = [_valid(_valid(q, g, 3), g, 2) for q in (X, Y, X * X, Y * Y, X * Y)]
    mx, my, exx, eyy, exy = M
    mxx, myy, mxy = mx * mx, my * my, mx * my
    sx, sy, sxy = exx - mxx, eyy - myy, exy - mxy
    A1, B1, A2, B2 = 2 * mxy + C1, (mxx + myy) + C1, 2 * sxy + C2, (sx + sy) + C2
    l, cs = A1 / B1, A2 / B2
    s = l * cs
    a = ((2 * (my - l * mx)) / B1) * cs + l * ((2 * (mx * cs - my)) / B2)
    b = -(s / B2)
    c = (2 * l) / B2
    return s, a, b, c


def _scalar(v, dtype):
    return torch.tensor(v, dtype=dtype)


def ssim_term(color, gt, ray_mask, patch_num, ps, w_ssim, layout="grid", norm_patches=None, frame_weight=1.0, dtype=torch.float64):
    """-> dict(L, ssim, term, hits, grad [R,3], s [n,3,W,W]) as tensors of `dtype` (hits: int).  color, gt: float32 [R,3]; ray_mask [R]."""
    n = n_patches(patch_num, layout)
    N = n if norm_patches is None else int(norm_patches)
    W = ps - (WIN - 1)
    g = window().to(dtype)
    m = torch.as_tensor(ray_mask).reshape(-1) > 0
    zero = torch.zeros((), dtype=dtype)
    X = to_patches(torch.where(m[:, None], torch.as_tensor(color).reshape(-1, 3).to(dtype), zero), patch_num, ps, layout)
    Y = to_patches(torch.where(m[:, None], torch.as_tensor(gt).reshape(-1, 3).to(dtype), zero), patch_num, ps, layout)
    s, a, b, c = _windows(X, Y, g)
    G = [_transposed(_transposed(k, g, 2, ps), g, 3, ps) for k in (a, b, c)]
    d = (G[0] + (2 * X) * G[1]) + Y * G[2]
    windows, denom = float(n * 3 * W * W), float(N * 3 * W * W)
    fw, w = _scalar(frame_weight, dtype), _scalar(w_ssim, dtype)
    nsc = -((fw * w) / _scalar(denom, dtype))
    grad = torch.where(m[:, None], from_patches(nsc * d, patch_num, ps, layout), zero)
    S = float(s.double().sum())
    hits = int(m.sum())
    ssim = _scalar(S / denom, dtype)
    L = _scalar((windows - S) / denom if hits > 0 else 0.0, dtype)
    return dict(L=L, ssim=ssim, term=(fw * w) * L, hits=hits, grad=grad, s=s)


def ssim_expr(color, gt, ray_mask, patch_num, ps, w_ssim, layout="grid", norm_patches=None, frame_weight=1.0):
    """The term fw w L as ONE differentiable torch expression of `color` (any float dtype, any device): masking, the two valid passes, s, the mean."""
    n = n_patches(patch_num, layout)
    N = n if norm_patches is None else int(norm_patches)
    W = ps - (WIN - 1)
    g = window().to(color.dtype).to(color.device)
    m = (ray_mask.reshape(-1) > 0)[:, None].to(color.dtype)

    def patches(t):
        C = t.shape[-1]
        if layout == "patch_major":
            return t.reshape(patch_num, ps, ps, C).permute(0, 3, 1, 2)
        return t.reshape(patch_num, ps, patch_num, ps, C).permute(0, 2, 4, 1, 3).reshape(n, C, ps, ps)
    X, Y = patches(color.reshape(-1, 3) * m), patches(gt.reshape(-1, 3).to(color.dtype) * m)

    def filt(q):
        r = sum(g[i] * q[..., i:i + W] for i in range(WIN))
        return sum(g[i] * r[..., i:i + W, :] for i in range(WIN))
    mx, my = filt(X), filt(Y)
    sx, sy, sxy = filt(X * X) - mx * mx, filt(Y * Y) - my * my, filt(X * Y) - mx * my
    s = (2 * mx * my + C1) / (mx * mx + my * my + C1) * (2 * sxy + C2) / (sx + sy + C2)
    if not bool((ray_mask > 0).any()):
        return (color * 0).sum()
    L = (n * 3 * W * W - s.sum()) / (N * 3 * W * W)
    return frame_weight * w_ssim * L


def bound(e_ref, scale):
    """The project's standing margin: 4 x max(the fp32 restatement's own error against fp64, one fp32 ulp-half of the largest magnitude)."""
    return 4.0 * max(float(e_ref), 2.0 ** -24 * float(scale))


# ---------------------------------------------------------------------------------------------------------------- test inputs
SHAPES = [(1, 7, "grid"), (2, 9, "grid"), (7, 8, "grid"), (1, 56, "grid"), (1, 64, "grid"), (3, 8, "patch_major"),
          # sizes at which the launch changes form (one wave and three channels at once up to 9; 256 lanes up to 32; 1024 beyond)
          (2, 10, "grid"), (1, 32, "grid"), (1, 33, "grid")]
MASKS = ["all", "tenth", "patch", "none"]
_CASES = {}


def make_case(patch_num, ps, layout, mask_kind, constant_patch=False):
    """-> (color [R,3] f32, gt [R,3] f32, ray_mask [R] int8) as torch CPU tensors; cached, never modified.  Smooth ground truth (a 5 x 5
    box-filtered uniform field per patch-sized tile of the batch), render = gt + 0.05 normal noise clamped to [-0.001, 1.001]."""
    key = (patch_num, ps, layout, mask_kind, constant_patch)
    if key in _CASES:
        return _CASES[key]
    n = n_patches(patch_num, layout)
    gen = torch.Generator().manual_seed(1000 * ps + 10 * n + MASKS.index(mask_kind))
    if layout == "patch_major":
        field = torch.rand((n, 3, ps + 4, ps + 4), generator=gen)
        gt_p = torch.nn.functional.avg_pool2d(field, 5, stride=1)
        gt = from_patches(gt_p, patch_num, ps, layout)
    else:
        S = patch_num * ps
        field = torch.rand((1, 3, S + 4, S + 4), generator=gen)
        gt = torch.nn.functional.avg_pool2d(field, 5, stride=1)[0].permute(1, 2, 0).reshape(-1, 3).contiguous()
    if constant_patch:                                                   # patch 0 constant in both images: sigma = 0, the C2 terms decide
        gp = to_patches(gt, patch_num, ps, layout)
        gp[0] = 0.37
        gt = from_patches(gp, patch_num, ps, layout)
    color = (gt + 0.05 * torch.randn(gt.shape, generator=gen)).clamp(-0.001, 1.001)
    if constant_patch:
        cp = to_patches(color, patch_num, ps, layout)
        cp[0] = 0.52
        color = from_patches(cp, patch_num, ps, layout)
    R = gt.shape[0]
    if mask_kind == "all":
        mask = torch.ones(R, dtype=torch.int8)
    elif mask_kind == "none":
        mask = torch.zeros(R, dtype=torch.int8)
    elif mask_kind == "tenth":
        mask = (torch.rand(R, generator=gen) >= 0.1).to(torch.int8)
    else:                                                                # the last patch missed as a whole
        mp = torch.ones((n, 1, ps, ps), dtype=torch.int8)
        mp[n - 1] = 0
        mask = from_patches(mp, patch_num, ps, layout).reshape(-1)
    _CASES[key] = (color.float().contiguous(), gt.float().contiguous(), mask.contiguous())
    return _CASES[key]


_REFS = {}


def references(patch_num, ps, layout, mask_kind, w_ssim, frame_weight=1.0, constant_patch=False, norm_patches=None):
    """(fp64 restatement, fp32 restatement) of a case, computed once."""
    key = (patch_num, ps, layout, mask_kind, w_ssim, frame_weight, constant_patch, norm_patches)
    if key not in _REFS:
        c, g, m = make_case(patch_num, ps, layout, mask_kind, constant_patch)
        _REFS[key] = tuple(ssim_term(c, g, m, patch_num, ps, w_ssim, layout, norm_patches, frame_weight, dtype=dt) for dt in (torch.float64, torch.float32))
    return _REFS[key]


def np32(t):
    return np.asarray(t.detach().cpu().numpy())
