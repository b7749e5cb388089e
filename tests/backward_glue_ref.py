"""Inputs, float64 references with per-element error bounds, and float32 restatements (in the kernels' operation order) of the glue kernels of the
training backward.  tests/test_backward_glue_gpu.py runs the kernels against the references; tests/test_backward_glue.py runs the float32
restatements against the same references with the same bounds, without a GPU: a bound that plain float32 arithmetic cannot meet is a mistake of
the derivation, not of a kernel.

The rule (U = 2^-24, the unit roundoff of float32):
  * a sum of n rounded products, added in any order (atomics included):  (n + 2) U sum |terms|, plus what the terms themselves carry in;
  * through expf / log1pf / sincosf / the sigmoid: the argument's bound times the derivative, plus 4 ulp (8 U relative) of each transcendental's
    value, plus one U per further rounded operation;
  * copies, permutations, integers and the kernels of two rounded operations per element: bit for bit.
Every bound below is written out next to the reference it belongs to.
"""
import numpy as np
import torch

U = 2.0 ** -24
F32 = np.float32
NCOUNTS = 9
CNT_VALID = 6                                       # HNR_CNT_SAMPLES_VALID (include/hnr.h)
CH_AUX_GROUP = 1280                                 # csrc/chain_defs.h: int32 pid[32], float w[32], 1024 further bytes per 32-row group
SENT = F32(-7.25)                                   # sentinel of float outputs
SENT_I = 0x5A5A5A5A
WORST = {}                                          # tensor name -> worst err / bound seen in this process


def sum_bound(abs_terms, n):
    return (n + 2) * U * abs_terms


def check(name, got, ref, bound):
    """max(err / bound) <= 1, printed per tensor; a zero bound demands the exact value."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), ref.shape)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.all(np.isfinite(got)), "%s: %d non-finite values" % (name, int((~np.isfinite(got)).sum()))
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    r = float(ratio.max()) if ratio.size else 0.0
    print("%-22s max err/bound = %.3f over %d" % (name, r, ratio.size))
    WORST[name] = max(WORST.get(name, 0.0), r)
    if r > 1.0:
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError("%s: err/bound = %.3f at %s (got %.9g, ref %.9g, bound %.3g)" % (name, r, i, got[i], ref[i], bound[i]))


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def check_bits(name, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    g = got.view(np.uint32) if got.dtype == F32 else got
    w = want.view(np.uint32) if want.dtype == F32 else want
    bad = int((g != w).sum())
    print("%-22s %d of %d differ" % (name, bad, g.size))
    if bad:
        i = np.unravel_index(int(np.argmax(g != w)), g.shape)
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, want %r" % (name, bad, g.size, i, got[i], want[i]))


def check_absmax(name, word, word0, values):
    """The published maximum (atomicMax on the bit pattern, exponent-exact: csrc/hnr_common.h absmax_publish) over `values`, from `word0`."""
    m = float(np.max(np.abs(values))) if np.size(values) else 0.0
    mb = int(bits(np.array([m], F32))[0])
    word, word0 = int(word), int(word0)
    print("%-22s word %#010x, max %#010x, before %#010x" % (name, word, mb, word0))
    if (mb >> 23) <= (word0 >> 23) and mb <= word0:
        assert word == word0, "%s: the larger word must stay" % name
        return
    if mb == 0:
        assert word == word0
        return
    assert (word >> 23) == (max(mb, word0) >> 23), "%s: exponent %d, the maximum's is %d" % (name, word >> 23, mb >> 23)
    assert word <= max(mb, word0) and word >= word0, name


def counts_of(n_valid):
    c = np.zeros((NCOUNTS,), np.int64)
    c[CNT_VALID] = n_valid
    return c


def wave_xor_sum(v, offs=(32, 16, 8, 4, 2, 1)):
    """The xor butterfly of a wave (or of a group of lanes) over the last axis: every lane ends with the same float32 sum."""
    idx = np.arange(v.shape[-1])
    for o in offs:
        v = v + v[..., idx ^ o]
    return v


def fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _waves_accumulate(contrib, n_valid, blocks):
    """Per-wave serial accumulation (sample s on wave s % n_waves), the block's 16 waves added in order, the blocks' atomics in block order."""
    n_waves = blocks * 16
    acc = np.zeros((n_waves,) + contrib.shape[1:], F32)
    for s0 in range(0, n_valid, n_waves):
        c = contrib[s0:s0 + n_waves]
        acc[:c.shape[0]] = acc[:c.shape[0]] + c
    acc = acc.reshape((blocks, 16) + contrib.shape[1:])
    blk = np.zeros((blocks,) + contrib.shape[1:], F32)
    for w in range(16):
        blk = blk + acc[:, w]
    return blk


def _atomics(pre, blk):
    out = pre.astype(F32).copy()
    for b in range(blk.shape[0]):
        out = out + blk[b]
    return out


# ================================================================================================ a. final colour
C1002 = F32(F32(1.0) + F32(2.0) * F32(0.001))


def persistent_blocks(cap):
    return max(1, min(512, (cap + 15) // 16))


def make_final(cap, n_valid, strides, seed):
    ldy, ldcf, ldgy, ldgcf = strides
    rng = np.random.default_rng(seed)
    items = cap + 7                                                   # R * SR > n_valid
    perm = rng.permutation(items).astype(np.int32)
    inp = dict(cap=cap, n_valid=n_valid, strides=strides, items=items)
    inp["vs_item"] = perm[:cap].copy()                                # an injection; entries past n_valid point at NaN items
    gdec = np.full((items, 4), np.nan, F32)
    gdec[perm[:n_valid]] = rng.standard_normal((n_valid, 4)).astype(F32) * np.where(rng.random((n_valid, 1)) < 0.3, 1e-3, 1.0).astype(F32)
    inp["g_decoded"] = gdec
    Y = np.full((cap, ldy), np.nan, F32)
    Y[:n_valid, :45] = rng.standard_normal((n_valid, 45)).astype(F32)
    CF = np.full((cap, ldcf), np.nan, F32)
    CF[:n_valid, :128] = rng.standard_normal((n_valid, 128)).astype(F32)
    inp["Y"], inp["CF"] = Y, CF
    # logits: row 0 spans about +-15 and beyond (saturated sigmoids), row 1 about +-1, row 2 about +-4
    inp["w_fin"] = (rng.standard_normal((3, 128)) * np.array([[0.6], [0.08], [0.3]])).astype(F32)
    inp["b_fin"] = np.array([0.3, -0.2, 0.1], F32)
    inp["g_w_pre"] = (0.5 * rng.standard_normal((3, 128))).astype(F32)
    inp["g_b_pre"] = np.array([0.7, -1.1, 0.4], F32)
    inp["counts"] = counts_of(n_valid)
    return inp


def ref_final(inp):
    """name -> (float64 reference, bound).  gCF [n_valid,128], g_w [3,128], g_b [3]."""
    n = inp["n_valid"]
    Y = torch.tensor(inp["Y"][:n, :45], dtype=torch.float64)
    CF = torch.tensor(inp["CF"][:n, :128], dtype=torch.float64, requires_grad=True)
    w = torch.tensor(inp["w_fin"], dtype=torch.float64, requires_grad=True)
    b = torch.tensor(inp["b_fin"], dtype=torch.float64, requires_grad=True)
    g = inp["g_decoded"][inp["vs_item"][:n]].astype(np.float64)
    x = torch.cat([Y + CF[:, :45], CF[:, 45:]], 1)
    colour = 1.002 * torch.sigmoid(x @ w.T + b) - 0.001
    (torch.tensor(g[:, 1:4]) * colour).sum().backward()
    gCF = CF.grad.numpy()
    g_w = inp["g_w_pre"].astype(np.float64) + w.grad.numpy()
    g_b = inp["g_b_pre"].astype(np.float64) + b.grad.numpy()
    # ---- bounds
    x = x.detach().numpy()
    w64, b64 = inp["w_fin"].astype(np.float64), inp["b_fin"].astype(np.float64)
    z = x @ w64.T + b64
    # z: 128 products of a rounded x (two roundings each) and the bias = 129 terms
    dz_ = sum_bound(np.abs(x) @ np.abs(w64).T + np.abs(b64), 129)
    sg = 1.0 / (1.0 + np.exp(-z))
    # sigmoid = 1 / (1 + expf(-z)): the argument through sg (1 - sg); expf's 4 ulp (8 U of e, d sg / d e = -sg^2, e sg = 1 - sg); the add and the division
    dsg = sg * (1 - sg) * dz_ + 8 * U * sg * (1 - sg) + 2 * U * sg
    gc = g[:, 1:4]
    dzv = gc * 1.002 * sg * (1 - sg)                                  # d loss / d logit
    # sg * (1 - sg): |1 - 2 sg| d sg and the subtraction's rounding; then the constant's rounding and three products
    ddz = np.abs(gc) * 1.002 * (np.abs(1 - 2 * sg) * dsg + U * sg * (1 - sg)) + 4 * U * np.abs(dzv)
    b_gCF = ddz @ np.abs(w64) + sum_bound(np.abs(dzv) @ np.abs(w64), 3)
    # weight sums: n_valid + 1 terms (the pre-loaded value), each product of dz and the rounded x
    b_gw = ddz.T @ np.abs(x) + sum_bound(np.abs(dzv).T @ np.abs(x) + np.abs(inp["g_w_pre"]), n + 2)
    b_gb = ddz.sum(0) + sum_bound(np.abs(dzv).sum(0) + np.abs(inp["g_b_pre"]), n + 1)
    return dict(gCF=(gCF, b_gCF), g_w=(g_w, b_gw), g_b=(g_b, b_gb))


def emul_final(inp):
    n, cap = inp["n_valid"], inp["cap"]
    Y, CF, w, b = inp["Y"][:n, :45], inp["CF"][:n, :128], inp["w_fin"], inp["b_fin"]
    g = inp["g_decoded"][inp["vs_item"][:n]]
    x = CF.copy()
    x[:, :45] = Y + CF[:, :45]
    dz = np.zeros((n, 3), F32)
    with np.errstate(over="ignore"):
        for j in range(3):
            r = x[:, :64] * w[j, :64] + x[:, 64:] * w[j, 64:]
            r = wave_xor_sum(r)[:, 0]
            sg = F32(1.0) / (F32(1.0) + np.exp(-(r + b[j])))
            dz[:, j] = g[:, 1 + j] * C1002 * sg * (F32(1.0) - sg)
    dx = dz[:, 0:1] * w[0] + dz[:, 1:2] * w[1]
    dx = dx + dz[:, 2:3] * w[2]
    blocks = persistent_blocks(cap)
    gw = _atomics(inp["g_w_pre"], _waves_accumulate(dz[:, :, None] * x[:, None, :], n, blocks))
    gb = _atomics(inp["g_b_pre"], _waves_accumulate(dz, n, blocks))
    return dict(gCF=dx, g_w=gw, g_b=gb)


# ================================================================================================ b. K-sums + alpha branch, 8 row slots per sample
def make_ksum(cap, n_valid, seed, slope=0.01):
    rng = np.random.default_rng(seed)
    rows = 8 * cap
    groups = (rows + 31) // 32 + 1
    inp = dict(cap=cap, n_valid=n_valid, slope=F32(slope), rows=rows)
    aw = (0.25 * rng.standard_normal(256)).astype(F32)
    ab = F32(0.35)
    # neighbour counts 0..8 as a prefix; a few samples with holes (the kernel tests every slot)
    cnt = rng.integers(0, 9, n_valid)
    if n_valid > 0:
        cnt[0] = 8
    if n_valid > 3:
        cnt[1], cnt[2] = 0, 1
    occ = np.arange(8)[None, :] < cnt[:, None]
    holes = rng.random(n_valid) < 0.1
    occ[holes] = rng.random((int(holes.sum()), 8)) < 0.5
    pid = np.full((groups * 32,), 0, np.int32)                        # rows past the valid ones: a valid id and a NaN weight (a read poisons)
    wv = np.full((groups * 32,), np.nan, F32)
    pid[:8 * n_valid] = np.where(occ, rng.integers(0, 1000, (n_valid, 8)), -1).reshape(-1)
    wv[:8 * n_valid] = np.where(occ, rng.random((n_valid, 8)), np.nan).reshape(-1).astype(F32)
    aux = rng.integers(0, 256, (groups, CH_AUX_GROUP), dtype=np.uint8)
    aux[:, 0:128] = pid.reshape(groups, 32).view(np.uint8)
    aux[:, 128:256] = wv.reshape(groups, 32).view(np.uint8)
    H4 = np.full((rows, 256), np.nan, F32)
    live = np.flatnonzero(occ.reshape(-1))
    if live.size:
        # y = h . alpha_w + alpha_b - 1 spread over about -30 .. 30: h0 moved along alpha_w to the target
        h0 = rng.standard_normal((live.size, 256))
        t = rng.uniform(-30, 30, live.size) + 1 - float(ab)
        a64 = aw.astype(np.float64)
        h = (h0 + ((t - h0 @ a64) / (a64 @ a64))[:, None] * a64).astype(F32)
        z = rng.random(h.shape)
        h[z < 0.01] = 0.0
        h[z > 0.99] = -0.0
        H4[live] = h
    gX5 = np.full((cap, 260), np.nan, F32)
    gX5[:n_valid, :256] = rng.standard_normal((n_valid, 256)).astype(F32) * np.where(rng.random((n_valid, 1)) < 0.3, 1e-3, 1.0).astype(F32)
    gs = np.full((cap,), np.nan, F32)
    gs[:n_valid] = rng.standard_normal(n_valid).astype(F32)
    inp.update(alpha_w=aw, alpha_b=np.array([ab], F32), aux=aux, pid=pid, w=wv, occ=occ, H4=H4, gX5=gX5, ldg5=260, g_sigma=gs,
               g_aw_pre=(0.5 * rng.standard_normal(256)).astype(F32), g_ab_pre=np.array([0.8], F32), counts=counts_of(n_valid))
    return inp


def ref_ksum(inp):
    n = inp["n_valid"]
    occ = inp["occ"].reshape(-1)
    live = np.flatnonzero(occ)
    aw, ab, slope = inp["alpha_w"].astype(np.float64), float(inp["alpha_b"][0]), float(inp["slope"])
    h = inp["H4"][live].astype(np.float64)
    w = inp["w"][live].astype(np.float64)
    s_of = live // 8
    gf = inp["gX5"][s_of, :256].astype(np.float64)
    gs = inp["g_sigma"][s_of].astype(np.float64)
    d = h @ aw
    y = d + ab - 1.0
    dy = sum_bound(np.abs(h) @ np.abs(aw) + abs(ab) + 1.0, 258)       # 256 products, the bias, the 1
    sig = 1.0 / (1.0 + np.exp(-y))
    sp = np.where(y > 20, y, np.log1p(np.exp(np.minimum(y, 50))))
    # softplus = log1pf(expf(y)): y through sigmoid(y); expf's 8 U of e through e / (1 + e); log1pf's 8 U of the value.  (y > 20: y itself, exact)
    dsp = sig * dy + 8 * U * sig + 8 * U * np.abs(sp)
    # sigmoid = e / (e + 1): y through sig (1 - sig); expf's 8 U of e (d sig / d e = (1 - sig)^2 and e (1 - sig) = sig); the add and the division
    # (y > 20: the kernel takes 1, 2e-9 away: inside 2 U sig)
    dsig = sig * (1 - sig) * dy + 8 * U * sig * (1 - sig) + 2 * U * sig
    da = w * gs * sig
    dda = np.abs(w * gs) * dsig + 2 * U * np.abs(da)
    f = np.where(inp["H4"][live] > 0, 1.0, slope)
    t1, t2 = w[:, None] * gf, da[:, None] * aw[None, :]
    gZ4 = np.zeros((inp["rows"], 256))
    gZ4[live] = (t1 + t2) * f
    # (w gX5 + da alpha_w) * factor: two products, their sum, the factor
    b_gZ4 = np.zeros_like(gZ4)
    b_gZ4[live] = f * (dda[:, None] * np.abs(aw)[None, :] + 4 * U * (np.abs(t1) + np.abs(t2)))
    hf = np.einsum("ij,ij->i", h, gf)
    g_wagg = np.zeros((inp["rows"],))
    g_wagg[live] = sp * gs + hf
    b_wagg = np.zeros_like(g_wagg)
    b_wagg[live] = np.abs(gs) * dsp + sum_bound(np.einsum("ij,ij->i", np.abs(h), np.abs(gf)) + np.abs(sp * gs), 257)
    g_aw = inp["g_aw_pre"].astype(np.float64) + da @ h
    b_aw = dda @ np.abs(h) + sum_bound(np.abs(da) @ np.abs(h) + np.abs(inp["g_aw_pre"]), live.size + 1)
    g_ab = inp["g_ab_pre"].astype(np.float64) + da.sum()
    b_ab = dda.sum() + sum_bound(np.abs(da).sum() + np.abs(inp["g_ab_pre"]), live.size + 1)
    return dict(gZ4=(gZ4[:8 * n], b_gZ4[:8 * n]), g_wagg=(g_wagg[:8 * n], b_wagg[:8 * n]), g_alpha_w=(g_aw, b_aw), g_alpha_b=(g_ab, b_ab))


def emul_ksum(inp):
    n, cap, slope = inp["n_valid"], inp["cap"], inp["slope"]
    occ = inp["occ"]
    aw, ab = inp["alpha_w"], inp["alpha_b"][0]
    H = np.nan_to_num(inp["H4"][:8 * n]).reshape(n, 8, 64, 4)
    gf = inp["gX5"][:n, :256].reshape(n, 1, 64, 4)
    a4 = aw.reshape(1, 1, 64, 4)

    def dot(v):
        p = H * v
        return wave_xor_sum(((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3])[..., 0]
    d, hf = dot(a4), dot(gf)
    w = np.nan_to_num(inp["w"][:8 * n]).reshape(n, 8)
    gs = inp["g_sigma"][:n, None]
    with np.errstate(over="ignore", invalid="ignore"):
        yv = (d + ab) - F32(1.0)
        ez = np.exp(yv)
        sp = np.where(yv > 20, yv, np.log1p(ez)).astype(F32)
        spd = np.where(yv > 20, F32(1.0), ez / (ez + F32(1.0))).astype(F32)
    da = w * gs * spd
    Hr = H.reshape(n, 8, 256)
    o = (w[..., None] * gf.reshape(n, 1, 256) + da[..., None] * aw) * np.where(Hr > 0, F32(1.0), slope)
    o = np.where(occ[..., None], o, F32(0.0)).astype(F32)
    gw = np.where(occ, sp * gs + hf, F32(0.0)).astype(F32)
    blocks = max(1, min(512, (cap + 15) // 16))
    # (the kernel adds a sample's up to eight slots one after another; here they are added first, then the sample: another fixed order)
    cw = np.zeros((n, 256), F32)
    cb = np.zeros((n,), F32)
    for k in range(8):
        cw = cw + np.where(occ[:, k, None], da[:, k, None] * Hr[:, k], F32(0.0))
        cb = cb + np.where(occ[:, k], da[:, k], F32(0.0))
    g_aw = _atomics(inp["g_aw_pre"], _waves_accumulate(cw, n, blocks))
    g_ab = _atomics(inp["g_ab_pre"], _waves_accumulate(cb[:, None], n, blocks))[0:1]
    return dict(gZ4=o.reshape(8 * n, 256), g_wagg=gw.reshape(8 * n), g_alpha_w=g_aw, g_alpha_b=g_ab)


# ================================================================================================ c. block3's seven extra input gradients
def make_extras(rows_cap, M, seed):
    rng = np.random.default_rng(seed)
    dZ3 = np.full((rows_cap, 256), np.nan, F32)
    dZ3[:M] = rng.standard_normal((M, 256)).astype(F32) * np.where(rng.random((M, 1)) < 0.3, 1e-3, 1.0).astype(F32)
    w30 = np.full((256, 263), np.nan, F32)                            # the kernel reads columns 256..262 only
    w30[:, 256:] = (0.2 * rng.standard_normal((256, 7))).astype(F32)
    return dict(rows_cap=rows_cap, M=M, dZ3=dZ3, w30=w30)


def ref_extras(inp):
    M = inp["M"]
    z, w = inp["dZ3"][:M].astype(np.float64), inp["w30"][:, 256:].astype(np.float64)
    return dict(gX3=(z @ w, sum_bound(np.abs(z) @ np.abs(w), 256)))


def emul_extras(inp):
    M = inp["M"]
    z, w = inp["dZ3"][:M], inp["w30"][:, 256:]
    acc = np.zeros((M, 16, 7), F32)
    for it in range(4):
        for q in range(4):
            nn = 4 * (np.arange(16) + 16 * it) + q                    # the sixteen lanes' columns at this step
            acc = fma32(z[:, nn, None], w[None, nn, :], acc)
    return dict(gX3=wave_xor_sum(np.moveaxis(acc, 1, -1), (1, 2, 4, 8))[..., 0])


# ================================================================================================ d. rows -> points
def make_gather(n_valid, seed, n_points=300, SR=4, K=8):
    rng = np.random.default_rng(seed)
    cap = n_valid + 5
    R = (cap + 7 + SR - 1) // SR
    items = R * SR
    perm = rng.permutation(items).astype(np.int32)
    vs_item = perm[:cap].copy()
    cnt = np.zeros((cap,), np.int32)
    cnt[:n_valid] = rng.integers(0, K + 1, n_valid)
    if n_valid:
        cnt[0] = K
    occ = np.arange(K)[None, :] < cnt[:n_valid, None]
    pidx = np.full((items, K), -1, np.int32)
    pidx[vs_item[:n_valid]] = np.where(occ, rng.integers(0, n_points, (n_valid, K)), -1)
    rows = 8 * cap
    row_pid = np.full((rows,), 7, np.int32)                           # rows past the count: a valid id that must not be counted
    row_pid[:8 * n_valid] = pidx[vs_item[:n_valid]].reshape(-1)
    weight = np.full((items, K), np.nan, F32)
    weight[vs_item[:n_valid]] = np.where(occ, rng.random((n_valid, K)), np.nan)
    gco = np.full((items, K), np.nan, F32)
    gco[vs_item[:n_valid]] = np.where(occ, rng.standard_normal((n_valid, K)), np.nan)
    raydir = rng.standard_normal((R, 3)).astype(F32)
    raydir /= np.linalg.norm(raydir, axis=1, keepdims=True).astype(F32)
    live = np.flatnonzero(occ.reshape(-1))
    gX3 = np.full((rows, 264), np.nan, F32)
    gX3[live, 256:263] = rng.standard_normal((live.size, 7)).astype(F32) * np.where(rng.random((live.size, 1)) < 0.3, 1e-3, 1.0).astype(F32)
    g_wagg = np.full((rows,), np.nan, F32)
    g_wagg[live] = rng.standard_normal(live.size).astype(F32)
    vs_off = np.full((cap,), 0, np.int32)
    vs_off[:n_valid] = 8 * np.arange(n_valid)
    return dict(n_valid=n_valid, cap=cap, R=R, SR=SR, K=K, n_points=n_points, rows=rows, vs_item=vs_item, vs_off=vs_off, vs_cnt=cnt, pidx=pidx, row_pid=row_pid,
                weight=weight, g_conf_out=gco, raydir=raydir, gX3=gX3, g_wagg=g_wagg, live=live, counts=counts_of(n_valid),
                g_conf_pre=rng.standard_normal(n_points).astype(F32), g_dir_pre=rng.standard_normal((n_points, 3)).astype(F32),
                g_color_pre=rng.standard_normal((n_points, 3)).astype(F32))


def ref_gather(inp, with_conf):
    """G8 rows (csrc/backward.hip gather_rows_bwd_kernel) and their float64 index_add by point id onto the pre-loaded buffers."""
    live = inp["live"]
    s = live // 8
    item = inp["vs_item"][s]
    e = (item, live % 8)
    g = inp["gX3"][live, 256:263].astype(np.float64)
    rd = inp["raydir"][item // inp["SR"]].astype(np.float64)
    t_w = inp["g_wagg"][live].astype(np.float64) * inp["weight"][e].astype(np.float64)
    t_c = inp["g_conf_out"][e].astype(np.float64) if with_conf else np.zeros_like(t_w)
    G8 = np.zeros((live.size, 8))
    B8 = np.zeros((live.size, 8))
    G8[:, 0:3] = g[:, 0:3]                                            # copies: exact
    G8[:, 3:6] = g[:, 3:6] + g[:, 6:7] * rd
    B8[:, 3:6] = sum_bound(np.abs(g[:, 3:6]) + np.abs(g[:, 6:7] * rd), 2)
    G8[:, 6] = t_w + t_c
    B8[:, 6] = sum_bound(np.abs(t_w) + np.abs(t_c), 2) if with_conf else U * np.abs(t_w)
    pid = inp["pidx"][e]
    P = inp["n_points"]
    S, SB, SA, N = np.zeros((P, 8)), np.zeros((P, 8)), np.zeros((P, 8)), np.zeros((P,))
    np.add.at(S, pid, G8)
    np.add.at(SB, pid, B8)
    np.add.at(SA, pid, np.abs(G8))
    np.add.at(N, pid, 1.0)
    pre = np.concatenate([inp["g_color_pre"], inp["g_dir_pre"], inp["g_conf_pre"][:, None]], 1).astype(np.float64)
    tot = pre + S[:, :7]
    btot = SB[:, :7] + (N[:, None] + 3) * U * (SA[:, :7] + np.abs(pre))          # a point's rows and the pre-loaded value: n + 1 terms
    touched = N > 0
    return dict(G8=(G8, B8), pid=pid, points=(tot, btot), touched=touched)


def emul_gather(inp, with_conf):
    live = inp["live"]
    item = inp["vs_item"][live // 8]
    e = (item, live % 8)
    g = inp["gX3"][live, 256:263]
    rd = inp["raydir"][item // inp["SR"]]
    G8 = np.zeros((live.size, 8), F32)
    G8[:, 0:3] = g[:, 0:3]
    G8[:, 3:6] = g[:, 3:6] + g[:, 6:7] * rd
    gc = inp["g_wagg"][live] * inp["weight"][e]
    G8[:, 6] = gc + inp["g_conf_out"][e] if with_conf else gc
    # (per point: its rows in ascending order, then onto the pre-loaded value.  The segment sum adds four partial sums instead: another fixed order)
    S = np.zeros((inp["n_points"], 8), F32)
    for r, p in zip(G8, inp["pidx"][e]):
        S[p] = S[p] + r
    pre = np.concatenate([inp["g_color_pre"], inp["g_dir_pre"], inp["g_conf_pre"][:, None]], 1)
    return dict(G8=G8, points=pre + S[:, :7])


# ================================================================================================ e. positional encoding of the embeddings
def make_point_rows(n, use_ids, use_dn, ld, seed):
    rng = np.random.default_rng(seed)
    n_cap = n + 5 if use_dn else n
    n_points = n_cap + 50 if use_ids else max(n_cap, 1)
    emb = (rng.standard_normal((n_points, 32)) * np.where(rng.random((n_points, 1)) < 0.3, 3.0, 0.5)).astype(F32)
    ids = rng.permutation(n_points)[:n_cap].astype(np.int32) if use_ids else None
    gE = np.full((max(n_cap, 1), ld), np.nan, F32)
    gE[:n, :224] = rng.standard_normal((n, 224)).astype(F32) * np.where(rng.random((n, 1)) < 0.3, 1e-3, 1.0).astype(F32)
    return dict(n=n, n_cap=n_cap, n_points=n_points, ld=ld, emb=emb, ids=ids, use_dn=use_dn, gE=gE, g_emb_pre=rng.standard_normal((n_points, 32)).astype(F32))


def point_rows_e64(emb_rows):
    """[e | sin(e 2^f), cos(e 2^f)] in the column layout of csrc/aggregate.hip point_rows_kernel: column 32 + 2 (3 d + f) (+ 1), torch float64."""
    f = torch.tensor([1.0, 2.0, 4.0], dtype=torch.float64)
    a = emb_rows[:, :, None] * f                                      # [n, 32, 3]
    return torch.cat([emb_rows, torch.stack([torch.sin(a), torch.cos(a)], -1).reshape(emb_rows.shape[0], 192)], 1)


def ref_point_rows(inp):
    n = inp["n"]
    rows = inp["ids"][:n] if inp["ids"] is not None else np.arange(n)
    e = torch.tensor(inp["emb"][rows], dtype=torch.float64, requires_grad=True)
    g = inp["gE"][:n, :224].astype(np.float64)
    (point_rows_e64(e) * torch.tensor(g)).sum().backward()
    pre = inp["g_emb_pre"][rows].astype(np.float64)
    ref = pre + e.grad.numpy()
    # g[d] + sum_f 2^f (cos g_sin - sin g_cos): the pre-loaded value, g[d] and six products = 8 terms; the stored sin / cos carry sincosf's 4 ulp
    a = inp["emb"][rows].astype(np.float64)[:, :, None] * np.array([1.0, 2.0, 4.0])
    gp = g[:, 32:].reshape(n, 32, 3, 2)
    terms = (np.array([1.0, 2.0, 4.0]) * (np.abs(np.cos(a) * gp[..., 0]) + np.abs(np.sin(a) * gp[..., 1]))).sum(-1)
    bound = sum_bound(np.abs(pre) + np.abs(g[:, :32]) + terms, 8) + 8 * U * terms
    return dict(rows=rows, g_emb=(ref, bound))


def emul_point_rows(inp):
    n = inp["n"]
    rows = inp["ids"][:n] if inp["ids"] is not None else np.arange(n)
    em = inp["emb"][rows]
    g = inp["gE"][:n, :224]
    acc = g[:, :32].copy()
    for f in range(3):
        a = em * F32(1 << f)
        sv, cv = np.sin(a), np.cos(a)
        col = 32 + 2 * (3 * np.arange(32) + f)
        acc = acc + F32(1 << f) * (cv * g[:, col] - sv * g[:, col + 1])
    return dict(g_emb=inp["g_emb_pre"][rows] + acc)


# ================================================================================================ i. the empty slots' share of d conf
def make_conf0(n, seed):
    rng = np.random.default_rng(seed)
    pidx = np.where(rng.random(n) < 0.4, -1, rng.integers(0, 1000, n)).astype(np.int32)
    g = rng.standard_normal(n).astype(F32)
    return dict(n=n, pidx=pidx, g=g, g_conf_pre=rng.standard_normal(6).astype(F32))


def ref_conf0(inp):
    t = inp["g"][inp["pidx"] < 0].astype(np.float64)
    pre = float(inp["g_conf_pre"][0])
    return dict(g_conf0=(np.array([pre + t.sum()]), np.array([sum_bound(abs(pre) + np.abs(t).sum(), t.size + 1)])))


def emul_conf0(inp):
    n = inp["n"]
    t = np.where(inp["pidx"] < 0, inp["g"], F32(0.0)).astype(F32)
    stride = 512 * 256
    acc = np.zeros((stride,), F32)
    for i0 in range(0, n, stride):
        c = t[i0:i0 + stride]
        acc[:c.size] = acc[:c.size] + c
    w = wave_xor_sum(acc.reshape(512, 4, 64))[..., 0]
    part = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
    w = wave_xor_sum((part[:256] + part[256:]).reshape(4, 64))[..., 0]
    return dict(g_conf0=np.array([inp["g_conf_pre"][0] + ((w[0] + w[1]) + (w[2] + w[3]))], F32))


# ================================================================================================ h / i. integer restatements
def ref_unique(row_pid, m, n_points):
    """numpy.unique over the rows < m whose pid >= 0: (ulist, counts per listed point, uidx [n_points])."""
    r = row_pid[:m]
    ul, cn = np.unique(r[r >= 0], return_counts=True)
    uidx = np.full((n_points,), -1, np.int32)
    uidx[ul] = np.arange(ul.size, dtype=np.int32)
    return ul.astype(np.int32), cn.astype(np.int32), uidx


def ref_ray_drop(mask, lut, explicit):
    m = mask > 0
    if explicit is not None:
        return (m & (explicit != 0)).astype(np.uint8)
    before = np.cumsum(m) - m                                         # number of valid rays before r
    return (m & (lut[before] != 0)).astype(np.uint8)


# ================================================================================================ the cases (shared by both test modules)
FINAL_SHAPES = [(1, 1), (17, 16), (40, 0), (300, 257), (9000, 8999)]                # (cap, n_valid); 8192 waves: the last takes two samples on some
FINAL_STRIDES = [(48, 128, 48, 128), (45, 128, 45, 128), (52, 136, 50, 132)]        # (ldy, ldcf, ldgy, ldgcf)
KSUM_SHAPES = [(1, 1), (16, 4), (16, 5), (40, 0), (8208, 8200)]
EXTRAS_SHAPES = [(32, 0), (32, 1), (32, 15), (32, 16), (32, 17), (33024, 33000)]    # (rows_cap, M); 2048 x 16 rows per trip
GATHER_N = [0, 1, 33, 700]
POINT_ROWS_N = [0, 1, 7, 8, 9, 3000]
CONF0_N = [1, 255, 131075]
