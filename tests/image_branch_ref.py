"""Inputs and float64 restatements for tests/test_image_branch.py (CPU) and tests/test_image_branch_gpu.py: the reference-view ("image") branch --
reprojection into V views, truncation to a pixel + bounds rule, feature gather, merge over the views (models/aggregators/point_aggregators.py:1047-1217
of the reference) and the transpose of the gather and of F.interpolate.  Plain numpy / torch; imports nothing from the product."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

# ---- the shapes the GPU module runs; the CPU module checks the generated inputs of every one of them ---------------------------------------------
FWD_V = (1, 3, 5, 8)
FWD_N = (1, 37, 1100)              # 37 x 3 rows: waves straddle views; 1100: more than one 1024-thread block
FWD_HW = ((48, 64), (37, 51))
FWD_CASES = [(V, n, hw) for V in FWD_V for n in FWD_N for hw in FWD_HW]
# (V, n_valid, (H, W), second gradient source): every V in {1, 3, 8, 9}, every n_valid in {1, 37, 1100}, every image size and both forms of d_gFb occur;
# V = 9 (the `v >= 8` branch) with rows that straddle views (37) and with more than one block (1100); the large image with few and with many views
BWD_CASES = [(1, 1, (9, 7), False), (1, 37, (37, 51), True), (1, 1100, (48, 64), False), (1, 37, (203, 301), False),
             (3, 37, (48, 64), True), (3, 1100, (37, 51), False), (3, 1100, (203, 301), True), (3, 1, (203, 301), True),
             (8, 37, (9, 7), True), (8, 1100, (48, 64), True), (8, 1, (37, 51), False), (8, 1100, (203, 301), False),
             (9, 37, (48, 64), False), (9, 1100, (37, 51), True), (9, 1, (9, 7), True), (9, 1100, (9, 7), False)]


# the fused merge stage (tests/test_fused_stages_gpu.py), V = 4: a wave owns 8 samples (7, 8, 9), a workgroup 12 waves (97 = one sample in a second
# workgroup); 33 is run by the child processes of the other kernel forms only
FUSED_N = (1, 7, 8, 9, 37, 97, 1100)
FUSED_CASES = [(n, hw) for n in FUSED_N for hw in FWD_HW]
FUSED_CHILD_N = (1, 33, 1100)
FUSED_CHILD_HW = (37, 51)


def case_seed(V, n, hw):
    return 100000 * V + 10 * n + hw[0]


def all_sample_cases():
    """(seed, n, V, H, W) of every random_samples / make_views call of the GPU modules."""
    out = {(case_seed(V, n, hw), n, V, hw[0], hw[1]) for V, n, hw in FWD_CASES}
    out |= {(case_seed(V, n, hw), n, V, hw[0], hw[1]) for V, n, hw, _ in BWD_CASES}
    out |= {(case_seed(4, n, hw), n, 4, hw[0], hw[1]) for n, hw in FUSED_CASES}
    out |= {(case_seed(4, n, FUSED_CHILD_HW), n, 4, FUSED_CHILD_HW[0], FUSED_CHILD_HW[1]) for n in FUSED_CHILD_N}
    return sorted(out)


# ---- cameras ---------------------------------------------------------------------------------------------------------------------------------------
def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """c2w [4,4] float64 of a camera at `eye` looking along +z at `target` (x right, y down)."""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, eye
    return m


def make_views(seed, V, H, W):
    """V cameras on a ring of radius ~2 around the origin, looking at a point near it.  Returns dict(c2w [V,4,4] f32, w2c [V,4,4] f32 (float64
    inverse, rounded once), intrinsic [3,3] f32, campos_n [V,3] f32)."""
    rng = np.random.default_rng(seed + 77)
    c2w = np.zeros((V, 4, 4))
    for v in range(V):
        a = 2 * math.pi * (v + rng.uniform(-0.2, 0.2)) / max(V, 3)
        eye = np.array([2.0 * math.cos(a), 2.0 * math.sin(a), rng.uniform(-0.6, 0.6)])
        c2w[v] = look_at(eye, rng.uniform(-0.15, 0.15, size=3))
    c2w = c2w.astype(np.float32)
    f = 0.9 * W
    K = np.array([[f, 0, 0.5 * W], [0, f, 0.5 * H], [0, 0, 1]], np.float32)
    w2c = np.linalg.inv(c2w.astype(np.float64)).astype(np.float32)
    return dict(c2w=c2w, w2c=w2c, intrinsic=K, campos_n=np.ascontiguousarray(c2w[:, :3, 3]))


def project(xyz, w2c, K, dtype=torch.float64, den32=False):
    """neural_points_volumetric_model.py:248-255 with the product's operand: w2c given (not inverted here).  xyz [n,3] -> (fx, fy) [V,n] in `dtype`.
    den32: the denominator `depth + 1e-10` rounded to float32 as the reference's float32 program rounds it (the one rounding of that program a
    higher precision can see: 1e-10 is below half an ulp of every depth above 2e-3), everything else in `dtype`."""
    x = torch.as_tensor(xyz).to(dtype)
    m = torch.as_tensor(w2c).to(dtype)
    k = torch.as_tensor(K).to(dtype)
    h = torch.cat([x, torch.ones_like(x[:, :1])], dim=-1)                         # [n,4]
    c = torch.einsum("nk,vjk->vnj", h, m)[..., :3]                                # [V,n,3]
    i = torch.einsum("vnk,jk->vnj", c, k)
    d = i[..., 2:3] + 1e-10
    if den32:
        d = (i[..., 2:3].float() + 1e-10).to(dtype)
    q = i / d
    return q[..., 0], q[..., 1]


def pixels_from(fx, fy, H, W):
    """`.to(torch.int32)` (truncation toward zero) + bounds rule (point_aggregators.py:1077-1088), with the product's range guard spelt out: a
    coordinate that is not inside (-2e9, 2e9) -- or NaN -- is masked.  Returns int64 [..., 2] = (px, py), (-1, -1) where masked."""
    ok = (fx > -2.0e9) & (fx < 2.0e9) & (fy > -2.0e9) & (fy < 2.0e9)
    px = torch.where(ok, fx, torch.full_like(fx, -1.0)).trunc().long()
    py = torch.where(ok, fy, torch.full_like(fy, -1.0)).trunc().long()
    inval = (~ok) | (px < 0) | (px >= W) | (py < 0) | (py >= H)
    neg = torch.full_like(px, -1)
    return torch.stack([torch.where(inval, neg, px), torch.where(inval, neg, py)], dim=-1)


def restated_pixels(xyz, w2c, K, H, W, dtype=torch.float64, den32=False):
    fx, fy = project(xyz, w2c, K, dtype, den32)
    return pixels_from(fx, fy, H, W)


def random_samples(seed, n, views, H, W, outside=0.2):
    """n world positions [n,3] float32: most in front of a chosen view and inside its image, a share `outside` of them outside every view's image.
    A sample whose float64 fx or fy in ANY view lies within 1e-3 of an integer (0, W and H among them) is redrawn, so that the float32 and the
    float64 projection truncate to the same pixel.  Deterministic in (seed, n, views, H, W)."""
    rng = np.random.default_rng(seed)
    V = views["c2w"].shape[0]
    Kd = views["intrinsic"].astype(np.float64)
    out = np.zeros((n, 3), np.float32)
    for i in range(n):
        want_outside = rng.uniform() < outside
        for _ in range(10000):
            if want_outside:
                p = rng.uniform(-6.0, 6.0, size=3)
            else:
                v = int(rng.integers(V))
                z = rng.uniform(0.8, 3.2)
                u = np.array([rng.uniform(0, W), rng.uniform(0, H), 1.0])
                cam = np.linalg.solve(Kd, u) * z
                p = views["c2w"][v].astype(np.float64)[:3, :3] @ cam + views["c2w"][v].astype(np.float64)[:3, 3]
            p = p.astype(np.float32)
            fx, fy = project(p[None], views["w2c"], views["intrinsic"])
            f = torch.cat([fx.reshape(-1), fy.reshape(-1)])
            if bool(((f - f.round()).abs() < 1e-3).any()) or not bool(torch.isfinite(f).all()):
                continue
            pix = pixels_from(fx, fy, H, W)
            if want_outside and bool((pix[..., 0] >= 0).any()):
                continue
            break
        else:
            raise RuntimeError("random_samples: no admissible sample")
        out[i] = p
    return out


# ---- the hand-built table: every product of the projection is exact in float32 ------------------------------------------------------------------------
EDGE_W, EDGE_H = 64, 48
EDGE_K = np.array([[64, 0, 32], [0, 64, 24], [0, 0, 1]], np.float32)
EDGE_T = ((0, 0, 0), (1, -1, 0))                          # w2c translations of the two views (identity rotations)
M = None                                                  # masked
# Camera coordinates in view v are (x, y, z) + EDGE_T[v]; fx = 64 cx / (cz + 1e-10) + 32 cz / (cz + 1e-10), fy alike with 24.  Rows are written as
# (fx0, fy0, z) -> x = (fx0 - 32) z / 64, y = (fy0 - 24) z / 64 (dyadic: exact), or as a position.  View 1: fx1 = fx0 + 64 / z, fy1 = fy0 - 64 / z.
# The expected pixels are those of the reference's float32 program, where cz + 1e-10 == cz for these depths and every operation is exact.
# In FLOAT64 the 1e-10 is visible: at cz > 0 a coordinate that is a non-zero integer n comes out as n (1 - 1e-10) and truncates to n - 1 (-1 becomes
# pixel 0, W becomes W - 1); at cz < 0 it comes out as n (1 + 1e-10) and truncates to n.  The last column writes out the float64 pixels where they
# differ; the rows "... behind the camera" repeat the integer cases at cz < 0, where both precisions agree.
_EDGE_ROWS = [
    # what                                          fx0,    fy0,   z     view 0     view 1     float64 differs
    ("fx exactly 0",                                0.0,   10.5,  1.0,  (0, 10),   M,         {}),                        # view 1: fx = 64 = W, fy < 0
    ("fx exactly W - 1",                           63.0,   10.5,  2.0,  (63, 10),  M,         {0: (62, 10)}),
    ("fx exactly W",                               64.0,   10.5,  1.0,  M,         M,         {0: (63, 10)}),
    ("fy exactly H - 1",                            5.5,   47.0,  4.0,  (5, 47),   (21, 31),  {0: (5, 46), 1: (21, 30)}),
    ("fy exactly H",                                5.5,   48.0,  4.0,  M,         (21, 32),  {0: (5, 47), 1: (21, 31)}),
    ("fx = -0.5 truncates to pixel 0",             -0.5,   10.5,  2.0,  (0, 10),   M,         {}),                        # view 1: (31.5, -21.5)
    ("fx = -1",                                    -1.0,   10.5,  2.0,  M,         M,         {0: (0, 10)}),
    ("fy = -0.5 truncates to pixel 0",             10.5,   -0.5,  4.0,  (10, 0),   M,         {}),
    ("pixel (0,0)",                                 0.0,    0.0,  1.0,  (0, 0),    M,         {}),
    ("(-0.5,-0.5) behind the camera: pixel (0,0)",  -0.5,   -0.5, -2.0,  (0, 0),    M,         {}),                        # view 1: (-32.5, 31.5)
    ("behind the camera, inside the image",        16.5,   12.5, -1.0,  (16, 12),  M,         {}),                        # view 1: fx = -47.5
    ("behind the camera, inside view 1",           90.5,  -40.5, -1.0,  M,         (26, 23),  {}),
    ("view 1: fx exactly 0",                      -64.0,   69.5,  1.0,  M,         (0, 5),    {}),
    ("view 1: fx = -0.5",                         -32.5,   42.5,  2.0,  M,         (0, 10),   {}),
    ("view 1: fx exactly W - 1, fy exactly 0",     47.0,   16.0,  4.0,  (47, 16),  (63, 0),   {0: (46, 15), 1: (62, 0)}),
    ("view 1: fx exactly W",                       48.0,   16.5,  4.0,  (48, 16),  M,         {0: (47, 16), 1: (63, 0)}),
    ("middle",                                     33.25,  20.75, 4.0,  (33, 20),  (49, 4),   {}),
    ("fx exactly W behind the camera",             64.0,   10.5, -1.0,  M,         M,         {}),
    ("fx = W - 1, fy = H - 1 behind the camera",   63.0,   47.0, -2.0,  (63, 47),  M,         {}),
    ("fy exactly H behind the camera",              5.5,   48.0, -1.0,  M,         M,         {}),
    ("fx = -1 behind the camera",                  -1.0,   10.5, -2.0,  M,         M,         {}),
]
_EDGE_POSITIONS = [
    # what                                          x               y      z     view 0  view 1
    ("z = 0",                                       1.0,            0.0,   0.0,  M,      M,      {}),                     # fx = 64 / 1e-10
    ("z = 0 on the axis of view 0: 0 / 1e-10 = 0",  0.0,            0.0,   0.0,  (0, 0), M,      {}),                     # view 1: cx = 1 -> 6.4e11
    ("coordinate beyond +2e9",                      float(2 ** 25), 0.0,   1.0,  M,      M,      {}),                     # fx = 2^31 + 32
    ("coordinate beyond -2e9",                     -float(2 ** 25), 0.0,   1.0,  M,      M,      {}),
    ("both beyond 2e9",                             0.0, float(2 ** 26),   2.0,  M,      M,      {}),
]


def edge_samples():
    """Returns dict(xyz [n,3] f32, w2c [2,4,4] f32, c2w [2,4,4] f32, intrinsic, campos_n, H, W, names, expect int64 [2,n,2] with (-1,-1) = masked: the
    reference's float32 program; expect64: the same program in float64)."""
    names, xyz, exp, exp64 = [], [], [[], []], [[], []]
    rows = [(w, (fx0 - 32.0) * z / 64.0, (fy0 - 24.0) * z / 64.0, z, e0, e1, d) for w, fx0, fy0, z, e0, e1, d in _EDGE_ROWS] + _EDGE_POSITIONS
    for what, x, y, z, e0, e1, d64 in rows:
        names.append(what)
        xyz.append((x, y, z))
        for v, e in enumerate((e0, e1)):
            exp[v].append(e or (-1, -1))
            exp64[v].append(d64.get(v, e) or (-1, -1))
    xyz64 = np.array(xyz, np.float64)
    xyz32 = xyz64.astype(np.float32)
    assert np.array_equal(xyz32.astype(np.float64), xyz64)                       # every coordinate is a float32 value
    w2c = np.stack([np.eye(4, dtype=np.float32) for _ in EDGE_T])
    c2w = w2c.copy()
    for v, t in enumerate(EDGE_T):
        w2c[v, :3, 3] = t
        c2w[v, :3, 3] = [-a for a in t]
    return dict(xyz=xyz32, w2c=w2c, c2w=c2w, intrinsic=EDGE_K.copy(), campos_n=np.ascontiguousarray(c2w[:, :3, 3]), H=EDGE_H, W=EDGE_W, names=names,
                expect=torch.tensor(exp, dtype=torch.int64), expect64=torch.tensor(exp64, dtype=torch.int64))


# ---- float64 restatements -------------------------------------------------------------------------------------------------------------------------------
def conv_out(n):
    return (n - 1) // 2 + 1


def pyramid_sizes(H, W):
    H1, W1 = conv_out(H), conv_out(W)
    H2, W2 = conv_out(H1), conv_out(W1)
    return [(H1, W1), (H2, W2), (conv_out(H2), conv_out(W2))]


LEVEL_CH = ((3, 6), (9, 12), (21, 24))                    # (first feature-map channel, channels) of up(s1), up(s2), up(s3)


def upsample(x, H, W):
    return F.interpolate(x, size=(H, W), mode="bilinear", align_corners=False)


def upsample_transpose(g, Hs, Ws):
    """Transpose of F.interpolate(x [V,C,Hs,Ws], size = g.shape[2:], bilinear, align_corners=False) applied to g [V,C,H,W]: autograd of torch's own op."""
    x = torch.zeros((g.shape[0], g.shape[1], Hs, Ws), dtype=g.dtype, requires_grad=True)
    (upsample(x, g.shape[2], g.shape[3]) * g).sum().backward()
    return x.grad


def scatter_rows(rows, pix, V, H, W):
    """rows [V,n,48] (any float dtype) added into a zero [V,H,W,48] float64 map at pix [V,n,2]; masked rows and rows at pixel (0,0) are skipped
    (the feature there is the constant 0).  Also returns the same sum over |rows| and the number of rows added per pixel [V,H,W]."""
    g = torch.zeros((V * H * W, 48), dtype=torch.float64)
    ga = torch.zeros_like(g)
    cnt = torch.zeros((V * H * W,), dtype=torch.float64)
    px, py = pix[..., 0], pix[..., 1]
    keep = (px >= 0) & ~((px == 0) & (py == 0))
    key = (torch.arange(V)[:, None] * H + py) * W + px
    r = rows.double()
    g.index_add_(0, key[keep], r[keep])
    ga.index_add_(0, key[keep], r[keep].abs())
    cnt.index_add_(0, key[keep], torch.ones(int(keep.sum()), dtype=torch.float64))
    return g.view(V, H, W, 48), ga.view(V, H, W, 48), cnt.view(V, H, W), keep


def level_grads(g_fm, H, W):
    """g_fm [V,H,W,48] float64 -> the three level gradients [V,C,Hs,Ws] (channels 3..9, 9..21, 21..45)."""
    out = []
    for (c0, C), (Hs, Ws) in zip(LEVEL_CH, pyramid_sizes(H, W)):
        out.append(upsample_transpose(g_fm[..., c0:c0 + C].permute(0, 3, 1, 2).contiguous(), Hs, Ws))
    return out


def merge_ref(f, hm, w_last, b_last, vmask, frame_w, dtype):
    """sigmoid(Hm . w + b) * vmask * frame_w, sum_v f w / (sum_v w + 1e-6).  f [V,S,45], hm [V,S,64], vmask [V,S], frame_w [V] or None."""
    f, hm, w_last, b_last, vmask = (t.to(dtype) for t in (f, hm, w_last, b_last, vmask))
    wv = torch.sigmoid((hm * w_last).sum(-1) + b_last) * vmask
    if frame_w is not None:
        wv = wv * frame_w.to(dtype)[:, None]
    return (f * wv[..., None]).sum(0) / (wv.sum(0) + 1e-6)[:, None]


def delta_dirs(xyz, campos, campos_n, dtype=torch.float64):
    """neural_points_volumetric_model.py:296-310 in `dtype` (float64 unless told otherwise): [V,n,3]."""
    x = torch.as_tensor(xyz).to(dtype)
    cur = x - torch.as_tensor(campos).to(dtype)
    cur = cur / (torch.linalg.norm(cur, dim=-1, keepdim=True) + 1e-6)
    out = []
    for c in torch.as_tensor(campos_n).to(dtype):
        nv = x - c
        out.append(nv / (torch.linalg.norm(nv, dim=-1, keepdim=True) + 1e-6) - cur)
    return torch.stack(out)


# ---- the fused per-sample stages (csrc/mlp.hip: hnr_merge_stage, hnr_mixup_stage), restated ------------------------------------------------------------
def mlp_ref(x, Ws, bs, acts, slope, dtype, addend=None):
    """nn.Linear + LeakyReLU(slope) layers in `dtype`: x [..., K0]; bs[l] may be None; acts[l] != 0 applies the activation after layer l;
    addend [..., N0] is added to layer 0 before its activation.  Returns the list of every layer's output."""
    x = torch.as_tensor(x).to(dtype)
    outs = []
    for l, (W, b, a) in enumerate(zip(Ws, bs, acts)):
        y = x @ W.to(dtype).T
        if b is not None:
            y = y + b.to(dtype)
        if l == 0 and addend is not None:
            y = y + addend.to(dtype)
        x = torch.where(y > 0, y, y * slope) if a else y
        outs.append(x)
    return outs


def frame_weights_with_a_zero(valid):
    """Frame weights [V] in [0.5, 1.5) for a case whose validity mask is `valid` [V,n], with weight 0 on the view that is the ONLY unmasked view of
    the most samples (ties: the first), so that "every unmasked view has weight 0" occurs wherever the samples allow it.  Returns (frame_w f32 [V],
    the view, the number of such samples)."""
    valid = torch.as_tensor(valid).bool()
    only = valid & (valid.sum(0) == 1)[None]
    per_view = only.sum(1)
    z = int(per_view.argmax())
    V = valid.shape[0]
    fw = (0.5 + ((torch.arange(V) * 0.37 + 0.11) % 1.0)).float()
    fw[z] = 0.0
    return fw, z, int(per_view[z])


def merge_stage_ref(xyz, w2c, K, campos, campos_n, fm, H, W, pre, Ws, bs, w_last, b_last, frame_w, slope, dtype, pix=None, hidden_scale=1.0):
    """hnr_merge_stage restated: rows [fm[v, py, px, :45] | delta_dirs] [V,n,48] (a masked row reads pixel (0,0)); merge-weight MLP with first
    layer Ws[0] [64,48] without bias and the per-sample addend pre [n,64], then two [64,64] layers with bias, all LeakyReLU; then merge_ref.
    pix [V,n,2]: the pixels if they are given by a table, else the float64 restatement's (the generated samples truncate alike in every precision:
    tests/test_image_branch.py).  hidden_scale multiplies the last hidden activations (0: what the result is without them).
    Returns dict(merged [n,45], logits [V,n], valid [V,n], hidden [V,n,64])."""
    if pix is None:
        pix = restated_pixels(xyz, w2c, K, H, W)
    valid = pix[..., 0] >= 0
    px, py = pix[..., 0].clamp(min=0), pix[..., 1].clamp(min=0)
    V = pix.shape[0]
    f = torch.as_tensor(fm)[torch.arange(V)[:, None], py, px][..., :45].to(dtype)                   # [V,n,45]
    f = torch.where(valid[..., None], f, torch.zeros_like(f))
    rows = torch.cat([f, delta_dirs(xyz, campos, campos_n, dtype)], dim=-1)                         # [V,n,48]
    hm = mlp_ref(rows, Ws, bs, (1, 1, 1), slope, dtype, addend=torch.as_tensor(pre)[None])[-1] * hidden_scale
    w_last, b_last = torch.as_tensor(w_last).to(dtype), torch.as_tensor(b_last).to(dtype)
    logits = (hm * w_last).sum(-1) + b_last
    merged = merge_ref(f, hm, w_last, b_last, valid.to(dtype), frame_w, dtype)
    return dict(merged=merged, logits=logits, valid=valid, hidden=hm)


def mixup_ref(X7, CF, Ws, bs, w_fin, b_fin, slope, dtype):
    """hnr_mixup_stage restated: Y = color_mixup_block(X7[:, :90]) (acts 1, 1, 0); x = [Y + CF[:, :45] | CF[:, 45:128]];
    rgb = sigmoid(x w_fin^T + b_fin) * 1.002 - 0.001.  Returns dict(Y [S,45], pre [S,3] (before the sigmoid), rgb [S,3])."""
    Y = mlp_ref(torch.as_tensor(X7)[:, :90], Ws, bs, (1, 1, 0), slope, dtype)[-1]
    cf = torch.as_tensor(CF).to(dtype)
    x = torch.cat([Y + cf[:, :45], cf[:, 45:128]], dim=-1)
    p = x @ torch.as_tensor(w_fin).to(dtype).reshape(3, 128).T + torch.as_tensor(b_fin).to(dtype)
    return dict(Y=Y, pre=p, rgb=torch.sigmoid(p) * 1.002 - 0.001)


MERGE_SLOPE = 0.01
FUSED_CAMPOS = np.array([0.3, -0.2, 0.1], np.float32)


@functools.lru_cache(maxsize=None)
def _views_and_samples(n, hw):
    seed = case_seed(4, n, hw)
    views = make_views(seed, 4, hw[0], hw[1])
    return views, random_samples(seed, n, views, hw[0], hw[1])


@functools.lru_cache(maxsize=None)
def fused_merge_case(n, hw=None, base_n=None):
    """Host-side inputs of one hnr_merge_stage case (V = 4), all float32 and read-only by convention.  hw = None: the hand-built edge table with its
    two views laid out as views (0, 1, 1, 0) (n is ignored; pixels from `expect`); otherwise make_views / random_samples of case_seed(4, n, hw), or
    -- base_n given -- the base_n-sample set of that image size repeated cyclically to n samples (the per-sample rows pre and CF stay fresh).
    w_last is scaled so that the fp64 sigmoid logits have standard deviation 1.5 (n = 1: over its four rows)."""
    if hw is None:
        e = edge_samples()
        order = [0, 1, 1, 0]
        xyz, H, W = e["xyz"], e["H"], e["W"]
        w2c, campos_n, K, pix = e["w2c"][order].copy(), e["campos_n"][order].copy(), e["intrinsic"], e["expect"][order].clone()
        n, seed = xyz.shape[0], 4000
    else:
        H, W = hw
        views, xyz = _views_and_samples(base_n or n, hw)
        w2c, campos_n, K = views["w2c"], views["campos_n"], views["intrinsic"]
        pix = restated_pixels(xyz, w2c, K, H, W)
        if base_n:
            idx = np.arange(n) % base_n
            xyz, pix = np.ascontiguousarray(xyz[idx]), pix[:, torch.from_numpy(idx)]
        seed = case_seed(4, n, hw)
    g = torch.Generator().manual_seed(seed + 17)
    fm = torch.randn((4, H, W, 48), generator=g)
    fm[..., 45:] = 0
    fm[:, 0, 0, :] = 0                                        # hnr_image_features zeroes pixel (0,0): what a masked row gathers
    dims = [(64, 48), (64, 64), (64, 64)]
    Ws = [(torch.rand(d, generator=g) * 2 - 1) * (3.0 / d[1]) ** 0.5 for d in dims]
    bs = [None] + [(torch.rand(64, generator=g) - 0.5) * 0.2 for _ in range(2)]
    pre = torch.randn((n, 64), generator=g) * 0.5
    CF = torch.randn((n, 128), generator=g)
    w_last = torch.randn(64, generator=g)
    b_last = torch.randn(1, generator=g) * 0.1
    c = dict(n=n, H=H, W=W, xyz=xyz, w2c=w2c, K=K, campos=FUSED_CAMPOS, campos_n=campos_n, pix=pix, fm=fm, Ws=Ws, bs=bs, pre=pre, CF=CF, b_last=b_last,
             slope=MERGE_SLOPE)
    raw = merge_stage_ref(w_last=w_last, frame_w=None, dtype=torch.float64, **_ref_args(c))["logits"]
    c["w_last"] = (w_last.double() * (1.5 / float((raw - b_last.double()).std()))).float()
    return c


def _ref_args(c):
    return {k: c[k] for k in ("xyz", "w2c", "K", "campos", "campos_n", "fm", "H", "W", "pre", "Ws", "bs", "b_last", "slope", "pix") if k in c}


def fused_merge_refs(c, frame_w=None, **override):
    """(fp64 restatement, the same restatement in float32) of a fused_merge_case; `override` replaces inputs (campos_n=..., hidden_scale=...)."""
    a = dict(_ref_args(c), w_last=c["w_last"], frame_w=frame_w)
    a.update(override)
    return merge_stage_ref(dtype=torch.float64, **a), merge_stage_ref(dtype=torch.float32, **a)


MERGE_FACTOR, MERGE_FLOOR = 4.0, 3e-7                       # err <= 4 e32 + 3e-7


def merge_bound(r64, r32):
    e32 = float((r32["merged"].double() - r64["merged"]).abs().max())
    return e32, MERGE_FACTOR * e32 + MERGE_FLOOR


def merge_sensitivity(c, frame_w=None):
    """How far the fp64 merged columns move (max abs) when (a) the last hidden activations are zeroed, (b) campos_n of views 1 and 2 are swapped:
    a test that holds the kernel to `bound` sees those parts only if they move the result by much more than the bound."""
    r64, r32 = fused_merge_refs(c, frame_w)
    _, bound = merge_bound(r64, r32)
    cn = np.ascontiguousarray(c["campos_n"][[0, 2, 1, 3]])
    d_hidden = float((fused_merge_refs(c, frame_w, hidden_scale=0.0)[0]["merged"] - r64["merged"]).abs().max())
    d_swap = float((fused_merge_refs(c, frame_w, campos_n=cn)[0]["merged"] - r64["merged"]).abs().max())
    return bound, d_hidden, d_swap


@functools.lru_cache(maxsize=None)
def fused_mixup_case(S):
    """Host-side inputs of one hnr_mixup_stage case: X7 [S,90], CF [S,128], sigma [S], the color_mixup_block weights, and color_final_block scaled
    so that the fp64 pre-sigmoid values reach at most 1.9 in magnitude."""
    g = torch.Generator().manual_seed(9000 + S)
    dims = [(45, 90), (45, 45), (45, 45)]
    Ws = [(torch.rand(d, generator=g) * 2 - 1) * (3.0 / d[1]) ** 0.5 for d in dims]
    bs = [(torch.rand(45, generator=g) - 0.5) * 0.2 for _ in range(3)]
    X7 = torch.randn((S, 90), generator=g)
    CF = torch.randn((S, 128), generator=g)
    sigma = torch.rand((S,), generator=g) * 5
    w_fin = torch.randn((3, 128), generator=g)
    b_fin = torch.randn(3, generator=g) * 0.1
    c = dict(S=S, X7=X7, CF=CF, sigma=sigma, Ws=Ws, bs=bs, b_fin=b_fin, slope=MERGE_SLOPE)
    raw = mixup_ref(X7, CF, Ws, bs, w_fin, torch.zeros(3), MERGE_SLOPE, torch.float64)["pre"]
    c["w_fin"] = (w_fin.double() * ((1.9 - float(b_fin.abs().max())) / float(raw.abs().max()))).float()
    return c


def fused_mixup_refs(c):
    a = (c["X7"], c["CF"], c["Ws"], c["bs"], c["w_fin"], c["b_fin"], c["slope"])
    return mixup_ref(*a, torch.float64), mixup_ref(*a, torch.float32)


# ---- whole-path tests at V > 4: the fixture's four cameras plus copies of them moved by a few centimetres ---------------------------------------------
# (chosen so that no sample of the scannet_small render / train fixtures projects within float32 rounding of a pixel border of an extra view:
# tests/test_image_branch.py asserts it)
_EXTRA_SHIFT = np.array([[0.032, -0.006, 0.007], [-0.038, 0.014, 0.034], [0.026, 0.031, 0.013], [-0.020, 0.021, -0.023]], np.float32)        # metres, world axes


def extended_c2w(c2w4, V):
    """c2w [V,4,4] f32: the first min(V, 4) given cameras, then camera v - 4 translated by _EXTRA_SHIFT[v - 4] (same rotation)."""
    c2w4 = np.asarray(c2w4, np.float32)
    out = [c2w4[v].copy() for v in range(min(V, 4))]
    for v in range(4, V):
        m = c2w4[v - 4].copy()
        m[:3, 3] += _EXTRA_SHIFT[v - 4]
        out.append(m)
    return np.stack(out)
