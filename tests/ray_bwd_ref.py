"""Inputs, float64 references with per-element error bounds, and float32 restatements (in the kernels' operation order) of the two transposes that open the
training backward: hnr_composite_bwd / hnr_composite_bwd_depth and hnr_merge_bwd / hnr_merge_bwd_max (csrc/backward.hip).  tests/test_ray_bwd_gpu.py runs
the kernels against the references; tests/test_ray_bwd.py runs the float32 restatements against the same references with the same bounds, and the closed
forms against float64 autograd, without a GPU.  Geometry, helpers and the rule of the bounds are those of tests/forward_glue_ref.py and
tests/backward_glue_ref.py (U = 2^-24):
  * a sum of n rounded products, added in any order (butterflies and atomics included): (n + 2) U sum |terms|, plus what the terms themselves carry in;
  * through expf and the sigmoid: the argument's bound times the derivative, plus 4 ulp (8 U relative) of expf's value, plus one U per further rounded operation;
    the divisions (hnr_div) are correctly rounded: one U;
  * a difference carries BOTH operands' bounds; a quotient by an inexact q is bounded with the smallest q the float32 run can hold (q - its bound, and never
    below the 1e-10 / 1e-6 that the kernels add), not with the first-order q: behind a saturated sample the two differ by orders of magnitude;
  * every rounded operation may also lose DN = 2^-126 (a result below the smallest normal float32, rounded on the denormal grid or flushed);
  * zeros by construction (an invalid sample, a masked ray, a dropped ray, a masked view, a frame weight of 0), copies and two-operation kernels: bit for bit.
"""
import numpy as np
import torch

from tests.backward_glue_ref import _atomics, check_absmax, counts_of, persistent_blocks  # noqa: F401
from tests.forward_glue_ref import (U, F32, SENT, WORST, E10, VSIZE_Z, sum_bound, check, check_bits, bits, wave_xor_sum, f64, cam64, z32,  # noqa: F401
                                    make_composite, padded, poisoned, ray_dist, ref_march, emul_march)

DN = 2.0 ** -126
EPS6 = F32(1e-6)

# ================================================================================================ composite backward
RAY_SR = [1, 2, 24, 63, 64, 65, 80]                 # <= 64: one wave per ray; above: one thread per ray
RAY_R = [1, 3, 4, 5, 257]                           # 4 rays per block in the wave form, 256 in the serial form
RAY_MODES = [(u, n) for u in (0, 1) for n in (False, True)]           # (unit mode, nsamp given)


def ray_K(R, SR):
    """K = 1 and K = 8 (the stride of pidx) on both forms and every R."""
    return 1 if (RAY_R.index(R) + RAY_SR.index(SR)) % 2 else 8


TOP_SIGMA = 50.0


def ray_seed(R, SR):
    return 100 * SR + R


def make_ray(R, SR, K, seed, top=TOP_SIGMA):
    """make_composite's geometry (small and large gaps, repeated and backward positions, holes, nsamp of 0 / 1 / SR in the first rays, ray 3 masked) with the
    sigma classes {0, U(0, min(60, 0.3 top)), top}.  The bounded cases take {0, U(0, 15), 50}: with {0, U(0, 60), 200} the derived bound of d sigma exceeded
    1e-3 |ref| on 24 .. 56 % of the live samples of the long rays in the plain distance mode (sigma dist reaches 20 behind a 0.1 gap, and every later
    sample inherits that q's bound), so sigma dist was lowered fourfold (<= 5), not the cap raised; 1 .. 8 % now (tests/test_ray_bwd.py asserts <= 10 %).
    top = 1e4 is the saturation case (q = 1e-10 behind such a sample: a bound there is honest and says nothing).  Ray 4: zero density on every sample
    (W = 0 with valid samples: kD = g_D / 1e-6)."""
    inp = make_composite(R, SR, K, seed)
    rng = np.random.default_rng(7000 + seed)
    sk = rng.choice(3, (R, SR), p=[0.15, 0.7, 0.15])
    inp["decoded"][..., 0] = np.where(sk == 0, 0.0, np.where(sk == 1, rng.uniform(0, min(60.0, 0.3 * top), (R, SR)), top)).astype(F32)
    if R > 4:
        inp["decoded"][4, :, 0] = 0.0
        inp["ray_mask"][4] = 1
    inp["g_raycolor"] = rng.standard_normal((R, 3)).astype(F32)
    inp["g_depth"] = rng.standard_normal(R).astype(F32)
    return inp


def make_ray_depth(R, SR, K, seed):
    """The inputs of the two objectives with the expected-depth term: make_ray's, with the density concentrated in a few well-separated samples.  A ray with
    nsamp >= 4 has three contributing samples (two for nsamp < 6), one drawn in each third (half) of its first nsamp slots, sigma in U(10, 30), made valid
    if the slot was a hole; every other sample has sigma = 0 (live, with a gradient, and an exact zero in W, A and S).  Rays with nsamp < 4, and ray 4,
    have no contributing sample: W = 0, kD = g_D / 1e-6.  Why: D is the w-weighted mean of z, so sum_s w_s (z_s - D) = 1e-6 D, and
      * a ray with ONE contributing sample c has z_c - D = 1e-6 z_c / (w_c + 1e-6): in float32 that is the rounding residue of D (U z_c ~ 1.5e-7 against
        2.5e-6 / w_c), so d sigma_c, and d sigma of the samples next to c, cannot be bounded within 1e-3 |ref| by any choice of sigma with w_c >= 1e-3;
        two contributing samples in adjacent slots (all that SR = 2 allows) are 0 .. 0.03 apart and meet the same residue;
      * with the density spread over the ray as in make_ray, every sample's z_s - D is a difference of neighbours, and the sums W and A carry (SR + 2) U.
    With the contributors apart by a third of the ray, |z_s - D| is 0.05 .. 1 for all but the samples next to the crossing of D, and the sums have three
    terms.  tests/test_ray_bwd.py asserts the 10 % condition against |ref| on these inputs for both objectives, every shape, every run."""
    inp = make_ray(R, SR, K, seed)
    rng = np.random.default_rng(9000 + seed)
    sig = np.zeros((R, SR), F32)
    for r in range(R):
        ns = int(inp["nsamp"][r])
        if ns < 4 or r == 4:
            continue
        k = 2 if ns < 6 else 3
        for i in range(k):
            s = int(rng.integers((i * ns) // k, ((i + 1) * ns) // k))
            sig[r, s] = rng.uniform(10.0, 30.0)
            if inp["pidx"][r, s, 0] < 0:
                inp["pidx"][r, s, :] = 7
    inp["decoded"][..., 0] = sig
    return inp


def make_ray_threshold(seed=11):
    """A ray with a sample whose distance is exactly 2 vsize_z, the unit mode's threshold (`>`: the distance stays): vsize_z is set to half of one small
    gap's float32 distance, which no position could be placed to hit through the rotated camera.  -> (inputs, (ray, slot))."""
    inp = make_ray(5, 24, 8, seed)
    d_f, _, _, valid = ray_dist(inp, False, 0)
    r = 2                                                             # nsamp = SR, not masked
    s = next(s for s in range(23) if valid[r, s] and 0.009 < d_f[r, s] < 0.031 and inp["decoded"][r, s, 0] > 0)
    inp["vsize_z"] = F32(d_f[r, s] / F32(2.0))
    for use_nsamp in (False, True):
        d1 = ray_dist(inp, use_nsamp, 1)[0]
        assert d1[r, s] == d_f[r, s] == F32(2.0) * inp["vsize_z"] and d1[r, s] != inp["vsize_z"]
    return inp, (r, s)


def pad_depth(inp):
    """Camera depth (float32, as the kernels form it) of the padding position, the world origin."""
    return z32(np.zeros((1, 3), F32), inp["campos"], inp["camrot"])[0]


def make_ray_pair(R, K, seed):
    """The same rays (nsamp <= 24) as the padded query leaves them, once in SR = 24 (wave form) and once in the first 24 slots of SR = 65 (serial form; slots
    24..64: position 0, no neighbour, decoded 0).  The padding's camera depth lies below every ray's running maximum, so the slot nsamp - 1 gets a distance
    of exactly 0 -> vsize_z in both runs (in SR = 24, slot 23 gets vsize_z as the last slot), and the 24 shared slots see the same operands."""
    a = make_ray(R, 24, K, seed)
    loc, pidx, dec = padded(a, True)
    z = z32(loc, a["campos"], a["camrot"])
    zmax = np.maximum.accumulate(z, 1)
    zp = pad_depth(a)
    has = a["nsamp"] > 0
    last = np.maximum(a["nsamp"] - 1, 0)
    assert np.all(zp < zmax[np.arange(R), last][has]), "the padding position must lie below each ray's running maximum of camera depths"
    assert np.all(a["nsamp"] <= 24)
    a["loc_w"], a["pidx"], a["decoded"] = loc, pidx, dec
    b = dict(a)
    b["SR"] = 65
    b["loc_w"] = np.zeros((R, 65, 3), F32)
    b["pidx"] = np.full((R, 65, K), -1, np.int32)
    b["decoded"] = np.zeros((R, 65, 4), F32)
    b["loc_w"][:, :24], b["pidx"][:, :24], b["decoded"][:, :24] = loc, pidx, dec
    return a, b


def ref_ray_bwd(inp, use_nsamp, unit_mode, colour=True, depth=False):
    """(d sigma, d rgb) of sum_r g_r . colour_r (+ g_D D_r), colour = sum_s w_s rgb_s + bg T_end, D = sum_s w_s z_s / (W + 1e-6), in closed form:
        d/d o_s = T_s gs_s - (sum_{j>s} w_j gs_j + (bg . g) T_end) / q_s,   gs_s = rgb_s . g + g_D (z_s - D) / (W + 1e-6),   d sigma = d o  rd  exp(-sigma rd)
    (test_ray_bwd.py holds it to float64 autograd).  The ray_dist decisions are taken in float32 (forward_glue_ref.ray_dist); (o, q, T, w) carry ref_march's
    bounds.  -> dict(g=(ref [R,SR,4], bound), live=[R,SR] samples with rd > 0 on rays that are not masked)."""
    R, SR = inp["R"], inp["SR"]
    d_f, _, _, valid = ray_dist(inp, use_nsamp, unit_mode)
    # the float32 distances (and, below, camera depths) as exact inputs: z32 / ray_dist restate the kernels' __fsub_rn / __fmul_rn / __fadd_rn chain, and
    # tests/test_forward_glue_gpu.py (test_composite, test_ray_march) holds that restatement to the device bit for bit and to the float64 geometry
    d64, bd = f64(d_f), np.zeros((R, SR))
    loc, _, dec = padded(inp, use_nsamp)
    sigma = np.where(valid, f64(dec[..., 0]), 0.0)
    rd, brd = np.where(valid, d64, 0.0), np.where(valid, bd, 0.0)
    # ref_march's (o, q, T, w) and bounds, with one refinement: sigma rd = 0 gives expf(-0) = 1, o = 0 and q = fl(1 + 1e-10f) = 1 exactly (an invalid
    # sample, a zero density), where ref_march grants expf its 4 ulp
    a = sigma * rd
    ba = sigma * brd + U * np.abs(a)
    e = np.exp(-a)
    be = np.where(a == 0, 0.0, e * ba + 8 * U * e + DN)
    o = 1.0 - e
    bo = np.where(a == 0, 0.0, be + U * np.abs(o))
    q = 1.0 - o + 1e-10
    bq = np.where(a == 0, 1e-10, bo + U * np.abs(1.0 - o) + U * q + U * 1e-10)
    T, bT = np.ones((R, SR + 1)), np.zeros((R, SR + 1))
    for s in range(SR):
        T[:, s + 1] = T[:, s] * q[:, s]
        bT[:, s + 1] = bT[:, s] * (q[:, s] + bq[:, s]) + T[:, s] * bq[:, s] + U * T[:, s + 1] + DN
    Te, bTe, T, bT = T[:, SR], bT[:, SR], T[:, :SR], bT[:, :SR]
    w = o * T
    bw = np.where(a == 0, 0.0, bo * (T + bT) + o * bT + U * w + DN)      # o = 0 exactly: w = 0 exactly, and adding it to a sum rounds nothing
    q_lo = np.maximum(q - bq, 1e-10 * (1 - 4 * U))                   # float32's q = fl(fl(1 - o) + 1e-10f) with 0 <= o <= 1
    g = f64(inp["g_raycolor"]) if colour else np.zeros((R, 3))
    rgb = f64(dec[..., 1:4])
    gs = (rgb * g[:, None, :]).sum(-1)
    bgs = sum_bound(np.abs(rgb * g[:, None, :]).sum(-1), 3)
    if depth:
        z, bz = f64(z32(loc, inp["campos"], inp["camrot"])), 0.0
        gD = f64(inp["g_depth"])
        W = w.sum(1)
        nz = (a != 0).sum(1)                                           # the terms of W, A and S that are not exact zeros
        bW = bw.sum(1) + sum_bound(W, nz)
        A = (w * z).sum(1)
        den = W + 1e-6
        bden = bW + U * den + U * 1e-6
        D = A / den
        # A and W share the weights' errors: they reach D = A / den through dD/dw_j = (z_j - D) / den; the two sums' own roundings do not cancel
        bD = ((bw * np.abs(z - D[:, None])).sum(1) + sum_bound(np.abs(w * z).sum(1), nz) + SR * DN +
              np.abs(D) * (sum_bound(W, nz) + U * den + U * 1e-6)) / den + U * np.abs(D) + DN
        kD = gD / den
        bkD = np.abs(kD) * bden / den + U * np.abs(kD) + DN
        diff = z - D[:, None]
        bdiff = bz + bD[:, None] + U * np.abs(diff)
        c = kD[:, None] * diff
        bc = bkD[:, None] * np.abs(diff) + np.abs(kD)[:, None] * bdiff + U * np.abs(c) + DN
        gs, bgs = gs + c, bgs + bc + U * np.abs(gs + c)
    bgg = (f64(inp["bg"]) * g).sum(1)
    b_bgg = sum_bound(np.abs(f64(inp["bg"]) * g).sum(1), 3)
    S, bS = np.zeros((R, SR)), np.zeros((R, SR))
    cur = bgg * Te
    bcur = b_bgg * Te + np.abs(bgg) * bTe + U * np.abs(cur) + DN
    for s in range(SR - 1, -1, -1):                                   # the suffix sum, one rounded product and one rounded addition per step
        S[:, s], bS[:, s] = cur, bcur
        t = gs[:, s] * w[:, s]
        bt = np.where(a[:, s] == 0, 0.0, bgs[:, s] * w[:, s] + np.abs(gs[:, s]) * bw[:, s] + U * np.abs(t) + DN)
        cur = cur + t
        bcur = bcur + bt + np.where(a[:, s] == 0, 0.0, U * np.abs(cur))
    x = S / q
    bx = bS / q_lo + np.abs(S) * bq / (q * q_lo) + U * np.abs(x) + DN
    p = T * gs
    bp = bT * np.abs(gs) + T * bgs + U * np.abs(p) + DN
    do = p - x
    bdo = bp + bx + U * np.abs(do)
    mm = do * rd
    bmm = bdo * rd + np.abs(do) * brd + U * np.abs(mm) + DN
    ds = mm * e
    bds = bmm * (e + be) + np.abs(mm) * be + U * np.abs(ds) + DN
    drgb = w[..., None] * g[:, None, :]
    bdrgb = bw[..., None] * np.abs(g[:, None, :]) + U * np.abs(drgb) + DN
    live = (rd > 0) & (inp["ray_mask"] != 0)[:, None]
    ref = np.concatenate([ds[..., None], drgb], -1)
    bound = np.concatenate([bds[..., None], bdrgb], -1)
    ref[~live], bound[~live] = 0.0, 0.0                              # invalid samples, masked rays: exact zeros
    return dict(g=(ref, bound), live=live)


def autograd_ray_bwd(inp, use_nsamp, unit_mode, colour=True, depth=False):
    """float64 autograd of the same objective, from the definition."""
    R, SR = inp["R"], inp["SR"]
    d_f, _, _, valid = ray_dist(inp, use_nsamp, unit_mode)
    d64 = f64(d_f)
    loc, _, dec = padded(inp, use_nsamp)
    x = torch.tensor(f64(dec), requires_grad=True)
    vt = torch.tensor(valid)
    zero = torch.zeros((), dtype=torch.float64)
    sigma = torch.where(vt, x[..., 0], zero)
    rd = torch.where(vt, torch.tensor(d64), zero)
    o = 1 - torch.exp(-sigma * rd)
    q = 1 - o + 1e-10
    T = torch.cumprod(torch.cat([torch.ones(R, 1, dtype=torch.float64), q], 1), 1)
    w = o * T[:, :SR]
    col = (w[..., None] * x[..., 1:]).sum(1) + torch.tensor(f64(inp["bg"])) * T[:, SR:]
    mask = torch.tensor(f64(inp["ray_mask"] != 0))
    loss = (col * torch.tensor(f64(inp["g_raycolor"])) * mask[:, None]).sum() if colour else zero
    if depth:
        z = torch.tensor(f64(z32(loc, inp["campos"], inp["camrot"])))
        D = (w * z).sum(1) / (w.sum(1) + 1e-6)
        loss = loss + (D * torch.tensor(f64(inp["g_depth"])) * mask).sum()
    loss.backward()
    return x.grad.numpy()


def emul_ray_bwd(inp, use_nsamp, unit_mode, colour=True, depth=False):
    """Both kernels' operations in their order, in float32 (the serial form; the wave form claims the same order)."""
    R, SR = inp["R"], inp["SR"]
    d_f, _, _, valid = ray_dist(inp, use_nsamp, unit_mode)
    loc, _, dec = padded(inp, use_nsamp)
    z = z32(loc, inp["campos"], inp["camrot"])
    rd = np.where(valid, d_f, F32(0.0)).astype(F32)
    sigma = np.where(valid, dec[..., 0], F32(0.0)).astype(F32)
    one = F32(1.0)
    T, A, W = np.ones((R,), F32), np.zeros((R,), F32), np.zeros((R,), F32)
    o_, T_ = np.zeros((R, SR), F32), np.zeros((R, SR), F32)
    g = inp["g_raycolor"] if colour else np.zeros((R, 3), F32)
    bg = inp["bg"]
    out = np.zeros((R, SR, 4), F32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for s in range(SR):
            o = one - np.exp(-sigma[:, s] * rd[:, s])
            o_[:, s], T_[:, s] = o, T
            if depth:
                w = o * T
                A = A + w * z[:, s]
                W = W + w
            T = T * ((one - o) + E10)
        S = ((bg[0] * g[:, 0] + bg[1] * g[:, 1]) + bg[2] * g[:, 2]) * T
        if depth:
            D = A / (W + EPS6)
            kD = inp["g_depth"] / (W + EPS6)
        for s in range(SR - 1, -1, -1):
            o, Ts = o_[:, s], T_[:, s]
            gs = (dec[:, s, 1] * g[:, 0] + dec[:, s, 2] * g[:, 1]) + dec[:, s, 3] * g[:, 2]
            if depth:
                gs = gs + kD * (z[:, s] - D)
            q = (one - o) + E10
            d_o = Ts * gs - S / q
            w = o * Ts
            S = S + gs * w
            out[:, s, 0] = (d_o * rd[:, s]) * np.exp(-sigma[:, s] * rd[:, s])
            out[:, s, 1], out[:, s, 2], out[:, s, 3] = w * g[:, 0], w * g[:, 1], w * g[:, 2]
    out[inp["ray_mask"] == 0] = 0.0
    return out.astype(F32)


def loose_count(magnitude, bound, live, rel=1e-3):
    """How many of the live samples' d sigma have a bound above rel x magnitude, and how many live samples there are."""
    return int((bound[..., 0][live] > rel * np.abs(magnitude[live])).sum()), int(live.sum())


# ================================================================================================ merge backward
MERGE_V = [1, 2, 3, 4, 5, 7, 8]                     # <= 4: merge_bwd_kernel<4, 16>; above: merge_bwd_kernel<8, 4>
MERGE_SHAPES = [(16, 1), (40, 37), (313, 300)]      # (cap, n_valid)
MERGE_BIG = (8232, 8229)                            # V = 2: 16 x 512 waves, the samples 8192.. are a wave's second trip
MERGE_STRIDES = [(90, 48, 64), (92, 52, 68)]        # (ldg7, ldgf, ldgz)
MERGE_SR = 3
LDGCF = 128


def merge_waves(V, cap):
    return persistent_blocks(cap) * (16 if V <= 4 else 4)


def make_merge(V, cap, n_valid, strides, fw_mode, drop, seed, slope=0.01):
    """fw_mode: None / "random" / "zero" (one frame weight exactly 0).  Rows n_valid .. cap - 1 of every view hold NaN in X6, Hm, vmask and gX7 (and the columns
    the kernel has no business in: X6[:, 45:], gX7[:, 90:]).  Logits Hm . w_last + b_last: N(0, 1.5) with rows at +-30 and +-25; +0 and -0 in Hm;
    sample 1 has every view masked, sample 2 one view left; masked-out views keep finite X6 rows (the forward's contract)."""
    ldg7, ldgf, ldgz = strides
    rng = np.random.default_rng(seed)
    n = n_valid
    rows = (np.arange(V)[:, None] * cap + np.arange(n)[None, :])
    inp = dict(V=V, cap=cap, n_valid=n, strides=strides, slope=F32(slope), SR=MERGE_SR, rows=rows, ld6=48, ldh=64)
    wl = (0.3 * rng.standard_normal(64)).astype(F32)
    bl = F32(0.15)
    X6 = np.full((V * cap, 48), np.nan, F32)
    X6[rows, :45] = rng.standard_normal((V, n, 45)).astype(F32)
    zr = rng.random((V, n, 64))
    keep = (zr >= 0.02) & (zr <= 0.98)                                # the others: signed zeros
    h0 = rng.standard_normal((V, n, 64)) * keep
    t = 1.5 * rng.standard_normal((V, n))
    special = [30.0, -30.0, 25.0, -25.0]
    for i, val in enumerate(special):
        if n > 3 + i:
            t[i % V, 3 + i] = val
    w64 = f64(wl)
    h = (h0 + ((t - float(bl) - h0 @ w64) / np.maximum((w64 * w64 * keep).sum(-1), 1e-3))[..., None] * w64 * keep).astype(F32)
    h[zr < 0.02] = 0.0
    h[zr > 0.98] = -0.0
    Hm = np.full((V * cap, 64), np.nan, F32)
    Hm[rows] = h
    vm = (rng.random((V, n)) < 0.75).astype(F32)
    if n > 2:
        vm[:, 1] = 0.0
        vm[:, 2] = 0.0
        vm[V - 1, 2] = 1.0
    for i in range(len(special)):                                     # the saturated rows take part
        if n > 3 + i:
            vm[i % V, 3 + i] = 1.0
    vmask = np.full((V * cap,), np.nan, F32)
    vmask[rows] = vm
    fw = None
    if fw_mode is not None:
        fw = rng.uniform(0.5, 1.5, V).astype(F32)
        if fw_mode == "zero":
            fw[V // 2] = 0.0
    n_rays = (cap + 4) // MERGE_SR + 2
    vs_item = np.sort(rng.permutation(n_rays * MERGE_SR)[:cap]).astype(np.int32)     # in range past the count too
    ray_drop = None
    if drop:
        ray_drop = (rng.random(n_rays) < 1.0 / 3).astype(np.uint8)
        ray_drop[vs_item[0] // MERGE_SR] = 1
        if vs_item[n - 1] // MERGE_SR != vs_item[0] // MERGE_SR:
            ray_drop[vs_item[n - 1] // MERGE_SR] = 0
    gX7 = np.full((cap, ldg7), np.nan, F32)
    gX7[:n, :90] = rng.standard_normal((n, 90)).astype(F32) * np.where(rng.random((n, 1)) < 0.3, 1e-3, 1.0).astype(F32)
    inp.update(X6=X6, Hm=Hm, vmask=vmask, w_last=wl, b_last=np.array([bl], F32), frame_w=fw, vs_item=vs_item, ray_drop=ray_drop, gX7=gX7,
               gCF0=rng.standard_normal((cap + 2, LDGCF)).astype(F32), g_w_pre=(0.5 * rng.standard_normal(64)).astype(F32), g_b_pre=np.array([0.8], F32),
               counts=counts_of(n), logits=t, hm_zero=(h == 0))
    inp["dropped"] = ray_drop[vs_item[:n] // MERGE_SR] != 0 if drop else np.zeros((n,), bool)
    return inp


def _merge_parts(inp):
    V, n, rows = inp["V"], inp["n_valid"], inp["rows"]
    f, hm, vm = f64(inp["X6"][rows, :45]), f64(inp["Hm"][rows]), f64(inp["vmask"][rows])
    fw = f64(inp["frame_w"]) if inp["frame_w"] is not None else np.ones((V,))
    dm = np.where(inp["dropped"][:, None], 0.0, f64(inp["gX7"][:n, 45:90]))
    return f, hm, vm, fw, dm


def ref_merge(inp):
    """The transpose of  merged[s, c] = sum_v f[v, s, c] wv[v, s] / (sum_v wv[v, s] + 1e-6),  wv = sigmoid(Hm . w_last + b_last) vmask frame_w
    (point_aggregators.py:1199-1217, :1286-1292), with the patch drop (:1222-1237: a dropped ray's merged45 has no gradient) and the LeakyReLU derivative on
    Hm, in closed form (test_ray_bwd.py holds it to float64 autograd).  name -> (float64 reference, bound): gF [V,n,48], gZ3 [V,n,64], g_w [64], g_b [1]."""
    V, n = inp["V"], inp["n_valid"]
    f, hm, vm, fw, dm = _merge_parts(inp)
    wl, bl, slope = f64(inp["w_last"]), float(inp["b_last"][0]), float(inp["slope"])
    d = hm @ wl + bl
    bd = sum_bound(np.abs(hm) @ np.abs(wl) + abs(bl), 65)             # 64 products through the butterfly, the bias
    sg = 1.0 / (1.0 + np.exp(-d))
    spp = sg * (1 - sg)
    bsg = spp * bd + 8 * U * spp + 2 * U * sg                         # expf's 4 ulp, the addition, the division (backward_glue_ref.ref_final)
    scale = vm * fw[:, None]
    bscale = U * scale if inp["frame_w"] is not None else 0.0 * scale
    wv = sg * scale
    bwv = bsg * scale + 2 * U * wv
    fsum = (f * wv[..., None]).sum(0)
    bfsum = (np.abs(f) * bwv[..., None]).sum(0) + sum_bound(np.abs(f * wv[..., None]).sum(0), V)
    wsum = wv.sum(0)
    bwsum = bwv.sum(0) + sum_bound(wsum, V)
    den = wsum + 1e-6
    bden = bwsum + U * den + U * 1e-6
    rden = (bden / den)[:, None]
    den_ = den[:, None]
    merged = fsum / den_
    bmerged = bfsum / den_ + np.abs(merged) * rden + U * np.abs(merged)
    num = dm[None] * wv[..., None]
    gF = np.zeros((V, n, 48))
    bgF = np.zeros((V, n, 48))
    gF[..., :45] = num / den_
    bgF[..., :45] = (np.abs(dm)[None] * bwv[..., None] + U * np.abs(num)) / den_ + np.abs(gF[..., :45]) * rden + U * np.abs(gF[..., :45])
    diff = f - merged[None]
    bdiff = bmerged[None] + U * np.abs(diff)
    pr = dm[None] * diff
    t = pr / den_
    bt = (np.abs(dm)[None] * bdiff + U * np.abs(pr)) / den_ + np.abs(t) * rden + U * np.abs(t)
    dwv = t.sum(-1)
    bdwv = bt.sum(-1) + sum_bound(np.abs(t).sum(-1), 64)              # the 64-lane butterfly
    dpre = dwv * scale * spp
    # ((d_wv scale) sg) (1 - sg): sg's error arrives through (1 - 2 sg) and its square (a saturated sg: 1 - sg = 0 in float32, 1e-13 in float64)
    bdpre = bdwv * scale * spp + np.abs(dwv) * bscale * spp + np.abs(dwv) * scale * (np.abs(1 - 2 * sg) * bsg + bsg * bsg) + 4 * U * np.abs(dpre)
    fac = np.where(inp["Hm"][inp["rows"]] > 0, 1.0, slope)
    gZ3 = dpre[..., None] * wl * fac
    bgZ3 = bdpre[..., None] * np.abs(wl) * fac + 2 * U * np.abs(gZ3)
    nt = n * V + 1                                                    # terms of a weight sum: every (sample, view) and the value in place
    g_w = f64(inp["g_w_pre"]) + np.einsum("vs,vsl->l", dpre, hm)
    b_w = np.einsum("vs,vsl->l", bdpre, np.abs(hm)) + sum_bound(np.einsum("vs,vsl->l", np.abs(dpre), np.abs(hm)) + np.abs(inp["g_w_pre"]), nt)
    g_b = f64(inp["g_b_pre"]) + dpre.sum()
    b_b = bdpre.sum() + sum_bound(np.abs(dpre).sum() + np.abs(inp["g_b_pre"]), nt)
    gcf = (inp["gCF0"][:n, :45] + inp["gX7"][:n, :45]).astype(F32)    # one float32 addition: bit for bit, dropped rays included
    return dict(gF=(gF, bgF), gZ3=(gZ3, bgZ3), g_w=(g_w, b_w), g_b=(g_b, b_b), gCF=gcf, scale=scale)


def autograd_merge(inp):
    V, n = inp["V"], inp["n_valid"]
    f, hm, vm, fw, dm = _merge_parts(inp)
    ft, ht = torch.tensor(f, requires_grad=True), torch.tensor(hm, requires_grad=True)
    w = torch.tensor(f64(inp["w_last"]), requires_grad=True)
    b = torch.tensor(f64(inp["b_last"]), requires_grad=True)
    wv = torch.sigmoid((ht * w).sum(-1) + b) * torch.tensor(vm * fw[:, None])
    merged = (ft * wv[..., None]).sum(0) / (wv.sum(0) + 1e-6)[:, None]
    (merged * torch.tensor(dm)).sum().backward()
    fac = np.where(inp["Hm"][inp["rows"]] > 0, 1.0, float(inp["slope"]))
    return dict(gF=ft.grad.numpy(), gZ3=ht.grad.numpy() * fac, g_w=f64(inp["g_w_pre"]) + w.grad.numpy(), g_b=f64(inp["g_b_pre"]) + b.grad.numpy())


def emul_merge(inp):
    """merge_bwd_kernel's operations in its order, in float32; the weight sums per wave (sample s on wave s % n_waves, views in turn), the block's waves in
    order, the blocks' atomics in block order (any order is within the bound)."""
    V, n, cap, rows = inp["V"], inp["n_valid"], inp["cap"], inp["rows"]
    one = F32(1.0)
    f = np.zeros((V, n, 64), F32)
    f[..., :45] = inp["X6"][rows, :45]
    hm, vm = inp["Hm"][rows], inp["vmask"][rows]
    wl, bl, slope = inp["w_last"], inp["b_last"][0], inp["slope"]
    dm = np.zeros((n, 64), F32)
    dm[:, :45] = np.where(inp["dropped"][:, None], F32(0.0), inp["gX7"][:n, 45:90])
    fw = inp["frame_w"]
    fsum, wsum = np.zeros((n, 64), F32), np.zeros((n,), F32)
    sg, wv, scale = np.zeros((V, n), F32), np.zeros((V, n), F32), np.zeros((V, n), F32)
    with np.errstate(over="ignore", under="ignore"):
        for v in range(V):
            d = wave_xor_sum(hm[v] * wl)[..., 0]
            sg[v] = one / (one + np.exp(-(d + bl)))
            scale[v] = vm[v] * (fw[v] if fw is not None else one)
            wv[v] = sg[v] * vm[v]
            if fw is not None:
                wv[v] = wv[v] * fw[v]
            fsum = fsum + f[v] * wv[v][:, None]
            wsum = wsum + wv[v]
        den = (wsum + EPS6)[:, None]
        merged = fsum / den
        gF = np.zeros((V, n, 48), F32)
        gZ3 = np.zeros((V, n, 64), F32)
        dpre = np.zeros((V, n), F32)
        for v in range(V):
            gF[v] = ((dm * wv[v][:, None]) / den)[:, :48]
            d_wv = wave_xor_sum((dm * (f[v] - merged)) / den)[..., 0]
            dpre[v] = d_wv * scale[v] * sg[v] * (one - sg[v])
            gZ3[v] = (dpre[v][:, None] * wl) * np.where(hm[v] > 0, one, slope)
    NW = 16 if V <= 4 else 4
    blocks = persistent_blocks(cap)
    n_waves = blocks * NW
    acc = np.zeros((n_waves, 65), F32)
    contrib = np.concatenate([dpre[..., None] * hm, dpre[..., None]], -1)                # [V, n, 65]: the weight terms, the bias term
    for s0 in range(0, n, n_waves):
        k = min(n_waves, n - s0)
        for v in range(V):
            acc[:k] = acc[:k] + contrib[v, s0:s0 + k]
    acc = acc.reshape(blocks, NW, 65)
    blk = np.zeros((blocks, 65), F32)
    for w in range(NW):
        blk = blk + acc[:, w]
    tot = _atomics(np.concatenate([inp["g_w_pre"], inp["g_b_pre"]]), blk)
    return dict(gF=gF, gZ3=gZ3, g_w=tot[:64], g_b=tot[64:], gCF=(inp["gCF0"][:n, :45] + inp["gX7"][:n, :45]).astype(F32))
