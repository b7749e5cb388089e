"""Inputs, float64 references with per-element error bounds, and float32 restatements (in the kernels' operation order) of the glue kernels of the
render forward (csrc/aggregate.hip, and hnr_chain_plan of csrc/chain.hip).  tests/test_forward_glue_gpu.py runs the kernels against the references;
tests/test_forward_glue.py runs the float32 restatements against the same references with the same bounds, and the index-only references against
brute-force loops, without a GPU.  Helpers and the rule of the bounds are those of tests/backward_glue_ref.py (U = 2^-24):
  * a sum of n rounded products, added in any order: (n + 2) U sum |terms|, plus what the terms themselves carry in;
  * through expf / log1pf / sinf / cosf / sincosf: the argument's bound times the derivative, plus 4 ulp (8 U relative) of the value, plus one U per
    further rounded operation; sqrt and the divisions are correctly rounded (one U);
  * a difference of two inexact values carries BOTH operands' bounds (the perspective `dists` columns and the ray distances cancel most of their
    operands' magnitude: the bound stays that of the operands), and an argument error e of sin / cos(x 2^f) arrives as 2^f e |cos| / |sin| (+ e^2 / 2);
  * copies, permutations, integers, clamps: bit for bit.
File:line in the docstrings name the reference project's code, as include/hnr.h does.
"""
import numpy as np

from tests.backward_glue_ref import U, F32, NCOUNTS, CNT_VALID, SENT, SENT_I, WORST, sum_bound, check, check_bits, bits, wave_xor_sum, C1002  # noqa: F401

CNT_SAMPLES, CNT_SMALL, CNT_TINY = 1, 7, 8          # HNR_CNT_SAMPLES, _SAMPLES_SMALL, _SAMPLES_TINY (include/hnr.h)
TINY = 2.0 ** -149                                  # the smallest float32 step: a transcendental's value next to zero
f64 = lambda a: np.asarray(a, np.float64)


def counts_of(n_items, n_valid):
    c = np.zeros((NCOUNTS,), np.int64)
    c[CNT_SAMPLES], c[CNT_VALID] = n_items, n_valid
    return c


# ================================================================================================ camera, w2pers, positional encoding
def make_camera(seed):
    """A camera that is not axis-aligned: a random rotation (columns = camera axes in the world) and a position off the origin."""
    rng = np.random.default_rng(1000 + seed)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return np.array([0.4, -0.7, 0.3], F32), q.astype(F32)


def cam_to_world(c, campos, camrot):
    """World positions (float32) of camera-space points c: the inverse of cam64 up to the rounding of the result."""
    return (f64(campos) + f64(c) @ f64(camrot).T).astype(F32)


def cam64(p, campos, camrot):
    """c[j] = sum_i (p - campos)[i] camrot[i][j] (neural_points.py:607-613) and its bound: the subtraction's rounding, three rounded products, two
    rounded additions: (1 + 3 + 2) U sum_i |shift_i camrot_ij|."""
    s = f64(p) - f64(campos)
    return s @ f64(camrot), 6 * U * (np.abs(s) @ np.abs(f64(camrot)))


def w2pers64(p, campos, camrot):
    """(x / z, y / z, z) (query_point_indices_worldcoords.py:96-103).  Quotient: the numerator's bound over |z|, the denominator's times |x / z^2|, one U."""
    c, bc = cam64(p, campos, camrot)
    z = c[..., 2:3]
    xy = c[..., :2] / z
    bxy = bc[..., :2] / np.abs(z) + np.abs(xy) * bc[..., 2:3] / np.abs(z) + U * np.abs(xy)
    return np.concatenate([xy, z], -1), np.concatenate([bxy, bc[..., 2:3]], -1)


def cam32(p, campos, camrot):
    s = p - campos
    cr = camrot
    return np.stack([(cr[0, j] * s[..., 0] + cr[1, j] * s[..., 1]) + cr[2, j] * s[..., 2] for j in range(3)], -1)


def w2pers32(p, campos, camrot):
    c = cam32(p, campos, camrot)
    return np.stack([c[..., 0] / c[..., 2], c[..., 1] / c[..., 2], c[..., 2]], -1)


def pe64(x, freqs, bx=0.0):
    """positional_encoding(x, freqs) (models/helpers/networks.py:175-190, ori=False): [sin, cos] interleaved per (dim, freq), column 2 (freqs d + f).
    Bound: the argument's bound 2^f bx through the derivative (+ its square / 2), and the transcendental's 4 ulp."""
    band = 2.0 ** np.arange(freqs)
    a = (f64(x)[..., None] * band).reshape(x.shape[:-1] + (-1,))
    ba = (np.broadcast_to(f64(bx), x.shape)[..., None] * band).reshape(a.shape)
    v = np.stack([np.sin(a), np.cos(a)], -1)
    b = np.stack([np.abs(np.cos(a)) * ba, np.abs(np.sin(a)) * ba], -1) + 0.5 * ba[..., None] ** 2 + 8 * U * np.abs(v) + TINY
    return v.reshape(a.shape[:-1] + (-1,)), b.reshape(a.shape[:-1] + (-1,))


def pe32(x, freqs):
    a = (x[..., None] * (2.0 ** np.arange(freqs)).astype(F32)).reshape(x.shape[:-1] + (-1,))
    return np.stack([np.sin(a), np.cos(a)], -1).reshape(a.shape[:-1] + (-1,)).astype(F32)


def make_cloud(n_points, campos, camrot, seed):
    """Points in front of the camera (camera depth 2 .. 4: every perspective divide is far from zero) with confidences below, at, between and above the
    1e-4 and 1 clamps (point_aggregators.py:1422-1424)."""
    rng = np.random.default_rng(2000 + seed)
    c = np.concatenate([rng.uniform(-1, 1, (n_points, 2)), rng.uniform(2, 4, (n_points, 1))], 1)
    conf = rng.uniform(0.01, 0.99, n_points).astype(F32)
    special = np.array([5e-5, 1e-4, -0.3, 1.0, 1.7, 0.0, np.nextafter(F32(1e-4), F32(1)), np.nextafter(F32(1), F32(0))], F32)
    conf[:min(special.size, n_points)] = special[:n_points]
    return dict(xyz=cam_to_world(c, campos, camrot), emb=(rng.standard_normal((n_points, 32)) * np.where(rng.random((n_points, 1)) < 0.3, 3.0, 0.5)).astype(F32),
                conf=conf, dir=rng.standard_normal((n_points, 3)).astype(F32), color=rng.random((n_points, 3)).astype(F32))


# ================================================================================================ 1. hnr_sample_plan, 2. hnr_chain_plan
PLAN_ITEMS = [0, 1, 1023, 1024, 1025, 3000]         # 1024 items per block of plan_scan_kernel


def make_plan(n_items, K, seed):
    """A work list that is a strict subset of the R * SR items; the unlisted items (and the list's entries past the count, which name them) all have K
    neighbours: reading one shifts every later offset."""
    rng = np.random.default_rng(seed)
    max_items = n_items + 37
    listed = np.sort(rng.permutation(max_items)[:n_items]).astype(np.int32)
    rest = np.setdiff1d(np.arange(max_items, dtype=np.int32), listed)
    work = np.concatenate([listed, rest]).astype(np.int32)           # work[n_items:]: in range, not listed
    nb = np.full((max_items,), K, np.int64)
    nb[listed] = rng.choice(np.arange(K + 1), n_items, p=np.r_[0.25, np.full(K, 0.75 / K)])
    if n_items > 8:
        nb[listed[:9]] = [0, 0, 1, 2, 3, 4, 5, K, 0]
    pidx = np.where(np.arange(K)[None, :] < nb[:, None], rng.integers(0, 500, (max_items, K)), -1).astype(np.int32)
    n_valid = int((nb[listed] > 0).sum())
    return dict(n_items=n_items, max_items=max_items, K=K, work=work, pidx=pidx, n_valid=n_valid, n_rows=int(nb[listed].sum()), counts=counts_of(n_items, n_valid))


def ref_plan(inp):
    """vs_item / vs_off / vs_cnt: the listed samples with >= 1 neighbour in list order, their neighbour counts and the exclusive prefix of those
    (`ray_valid`, point_aggregators.py:1441, and the boolean-mask row order of :924-935)."""
    w = inp["work"][:inp["n_items"]]
    nb = (inp["pidx"][w] >= 0).sum(1)
    v = nb > 0
    cnt = nb[v].astype(np.int32)
    return w[v].astype(np.int32), (np.cumsum(cnt) - cnt).astype(np.int32), cnt


def loop_plan(inp):
    item, off, cnt, rows = [], [], [], 0
    for i in range(inp["n_items"]):
        w = int(inp["work"][i])
        n = 0
        for k in range(inp["K"]):
            if inp["pidx"][w, k] >= 0:
                n += 1
        if n:
            item.append(w), off.append(rows), cnt.append(n)
            rows += n
    return np.array(item, np.int32), np.array(off, np.int32), np.array(cnt, np.int32)


def plan_fits(off, cnt, cap_samples, cap_rows):
    """The entries a call with these capacities writes (the others raise *d_overflow)."""
    return (np.arange(off.size) < cap_samples) & (off + cnt <= cap_rows)


def chain_class(nb, classes):
    """Row-slot class of a sample with nb neighbours (include/hnr.h, hnr_chain_plan): 1 = eight slots, 2 = four, 3 = two, 0 = not listed."""
    if classes == 0:
        return np.where(nb > 0, 1, 0)
    if classes == 1:
        return np.where(nb > 4, 1, np.where(nb > 0, 2, 0))
    return np.where(nb > 4, 1, np.where(nb > 2, 2, np.where(nb > 0, 3, 0)))


def ref_chain_plan(inp, classes):
    """numpy's stable partition of the listed samples by class -> (vs_item, n_small, n_tiny)."""
    w = inp["work"][:inp["n_items"]]
    cl = chain_class((inp["pidx"][w] >= 0).sum(1), classes)
    order = np.argsort(cl, kind="stable")
    order = order[cl[order] > 0]
    return w[order].astype(np.int32), int((cl == 2).sum()), int((cl == 3).sum())


def loop_chain_plan(inp, classes):
    lists = {1: [], 2: [], 3: []}
    for i in range(inp["n_items"]):
        w = int(inp["work"][i])
        n = sum(1 for k in range(inp["K"]) if inp["pidx"][w, k] >= 0)
        c = int(chain_class(np.array(n), classes))
        if c:
            lists[c].append(w)
    return np.array(lists[1] + lists[2] + lists[3], np.int32), len(lists[2]), len(lists[3])


# ================================================================================================ 3. hnr_gather_rows
GATHER_N = [1, 31, 32, 33, 70]                      # 32 samples per block
GATHER_K = [8, 9, 12, 16]                           # 9, 12, 16: the kbase loop and the weight sum across its passes


def make_gather_rows(n_valid, K, seed, n_points=200, SR=3):
    rng = np.random.default_rng(seed)
    campos, camrot = make_camera(seed)
    cloud = make_cloud(n_points, campos, camrot, seed)
    cap = n_valid + 3
    R = (cap + 5 + SR - 1) // SR
    items = R * SR
    vs_item = rng.permutation(items)[:cap].astype(np.int32)
    cnt = (1 + (np.arange(cap) + K - 1) % K).astype(np.int32)        # K, 1, 2, ..: neighbour counts 1..K within one call
    cnt[n_valid:] = K                                                # past the count: a wrong item (NaN position) with K rows at offset 0
    off = np.zeros((cap,), np.int32)
    off[:n_valid] = np.cumsum(cnt[:n_valid]) - cnt[:n_valid]
    rows = int(cnt[:n_valid].sum())
    pidx = rng.integers(0, n_points, (items, K)).astype(np.int32)    # unlisted items: valid ids
    loc_w = np.full((items, 3), np.nan, F32)
    for s in range(n_valid):
        it = vs_item[s]
        pidx[it, cnt[s]:] = -1
        if s < 8:
            pidx[it, 0] = s                                           # the points with the confidences on and around the clamps
        near = cloud["xyz"][pidx[it, 0]].astype(np.float64)
        loc_w[it] = (near + rng.uniform(-0.08, 0.08, 3)).astype(F32)
    loc_w[vs_item[0]] = cloud["xyz"][pidx[vs_item[0], 0]]           # a point on its sample: norm 0, the 1e-6 clamp (:825-833)
    raydir = rng.standard_normal((R, 3)).astype(F32)
    raydir /= np.linalg.norm(raydir, axis=1, keepdims=True).astype(F32)
    d = dict(n_valid=n_valid, cap=cap, K=K, SR=SR, R=R, items=items, rows=rows, n_points=n_points, campos=campos, camrot=camrot, vs_item=vs_item,
             vs_off=off, vs_cnt=cnt, pidx=pidx, loc_w=loc_w, raydir=raydir, counts=counts_of(items, n_valid))
    d.update(cloud)
    # row -> (sample, k, item, point)
    d["row_s"] = np.repeat(np.arange(n_valid), cnt[:n_valid])
    d["row_k"] = np.arange(rows) - off[d["row_s"]]
    d["row_item"] = vs_item[d["row_s"]]
    d["row_pid"] = pidx[d["row_item"], d["row_k"]]
    return d


def ref_gather_rows(inp):
    """name -> (float64 reference, bound) per neighbour row.  neural_points.py:709-720 (gather), :607-613 (w2pers), point_aggregators.py:1472-1480
    (dists), :825-833 and :1500-1501 (linear kernel, normalised), :1508-1512 (x clamp(conf)), :930 / :938 (encodings), :957-971 (block3 extras)."""
    cp, cr = inp["campos"], inp["camrot"]
    s, item, pid = inp["row_s"], inp["row_item"], inp["row_pid"]
    p, l = f64(inp["xyz"][pid]), f64(inp["loc_w"][item])
    pp, bpp = w2pers64(inp["xyz"][pid], cp, cr)
    sp, bsp = w2pers64(inp["loc_w"][item], cp, cr)
    d6, b6 = np.zeros((s.size, 6)), np.zeros((s.size, 6))
    d6[:, :3] = p - l
    b6[:, :3] = U * np.abs(d6[:, :3])                                 # one rounded subtraction of exact inputs
    for j in range(2):                                                # x z (point) - x z (sample): each product carries its factors' bounds and one U
        tp, ts = pp[:, j] * pp[:, 2], sp[:, j] * sp[:, 2]
        d6[:, 3 + j] = tp - ts
        b6[:, 3 + j] = (np.abs(pp[:, 2]) * bpp[:, j] + np.abs(pp[:, j]) * bpp[:, 2] + U * np.abs(tp)) + \
                       (np.abs(sp[:, 2]) * bsp[:, j] + np.abs(sp[:, j]) * bsp[:, 2] + U * np.abs(ts)) + U * np.abs(tp - ts)
    d6[:, 5] = pp[:, 2] - sp[:, 2]
    b6[:, 5] = bpp[:, 2] + bsp[:, 2] + U * np.abs(d6[:, 5])
    pe5 = pe64(d6, 5, b6)
    pe3 = pe64(inp["emb"][pid], 3)                                    # exact arguments (a float32 times a power of two)
    # weights: |d| = sqrt of three squares of once-rounded differences: (2 + 1) U per square, two additions, half of that through the root, the root's
    # own U: 3.5 U; 1 / max(|d|, 1e-6): 4.5 U -> 5 U.  The sum of cnt such positive terms, cnt - 1 additions: (cnt + 4) U.  The quotient: (cnt + 10) U.
    nrm = np.sqrt((d6[:, :3] ** 2).sum(1))
    wraw = 1.0 / np.maximum(nrm, float(F32(1e-6)))
    tot = np.zeros((inp["n_valid"],))
    np.add.at(tot, s, wraw)
    w = wraw / np.maximum(tot[s], float(F32(1e-8)))
    cnt = f64(inp["vs_cnt"][s])
    bw = (cnt + 10) * U * w
    confc = np.clip(inp["conf"][pid], F32(1e-4), F32(1.0))            # float32 clamp: exact
    wagg = w * f64(confc)
    dd, v = f64(inp["dir"][pid]), f64(inp["raydir"][item // inp["SR"]])
    ext, bext = np.zeros((s.size, 4)), np.zeros((s.size, 4))
    ext[:, :3] = dd - v
    bext[:, :3] = U * np.abs(ext[:, :3])
    ext[:, 3] = (dd * v).sum(1)
    bext[:, 3] = sum_bound(np.abs(dd * v).sum(1), 3)
    return dict(pe3=pe3, pe5=pe5, wagg=(wagg, bw * f64(confc) + U * np.abs(wagg)), weight=(w, bw), confc=confc, ext=(ext, bext))


def emul_gather_rows(inp):
    cp, cr = inp["campos"], inp["camrot"]
    s, item, pid, k = inp["row_s"], inp["row_item"], inp["row_pid"], inp["row_k"]
    p, l = inp["xyz"][pid], inp["loc_w"][item]
    pp, sp = w2pers32(p, cp, cr), w2pers32(l, cp, cr)
    d6 = np.zeros((s.size, 6), F32)
    d6[:, :3] = p - l
    d6[:, 3] = pp[:, 0] * pp[:, 2] - sp[:, 0] * sp[:, 2]
    d6[:, 4] = pp[:, 1] * pp[:, 2] - sp[:, 1] * sp[:, 2]
    d6[:, 5] = pp[:, 2] - sp[:, 2]
    nrm = np.sqrt((d6[:, 0] * d6[:, 0] + d6[:, 1] * d6[:, 1]) + d6[:, 2] * d6[:, 2])
    wraw = (F32(1.0) / np.maximum(nrm, F32(1e-6))).astype(F32)
    # per pass of eight slots: the butterfly over the pass's own lanes, then the other slots one after another (gather_rows_kernel, K > 8)
    w = np.zeros((s.size,), F32)
    for r in range(s.size):
        mine = np.zeros((8,), F32)
        base = 8 * (k[r] // 8)
        sel = (s == s[r])
        ks, ws = k[sel], wraw[sel]
        mine[ks[(ks >= base) & (ks < base + 8)] - base] = ws[(ks >= base) & (ks < base + 8)]
        tot = wave_xor_sum(mine, (1, 2, 4))[0]
        if inp["K"] > 8:
            extra = F32(0.0)
            for x in ws[(ks < base) | (ks >= base + 8)]:
                extra = F32(extra + x)
            tot = F32(tot + extra)
        w[r] = wraw[r] / np.maximum(tot, F32(1e-8))
    confc = np.clip(inp["conf"][pid], F32(1e-4), F32(1.0))
    dd, v = inp["dir"][pid], inp["raydir"][item // inp["SR"]]
    ext = np.zeros((s.size, 4), F32)
    ext[:, :3] = dd - v
    ext[:, 3] = (dd[:, 0] * v[:, 0] + dd[:, 1] * v[:, 1]) + dd[:, 2] * v[:, 2]
    return dict(pe3=pe32(inp["emb"][pid], 3), pe5=pe32(d6, 5), wagg=w * confc, weight=w, ext=ext)


# ================================================================================================ 4. hnr_ksum
KSUM_N = [1, 3, 4, 5, 257]                          # four waves (samples) per block


def make_ksum(n_valid, twelve, seed, SR=3):
    """Neighbour counts 1..8 in turn (`twelve`: every third sample has 12), alpha logits y = h . alpha_w + alpha_b - 1 over -30 .. 30 with rows exactly on
    both sides of y > 20, signed zeros in H4."""
    rng = np.random.default_rng(seed)
    cap = n_valid + 2
    cnt = (1 + np.arange(cap) % 8).astype(np.int32)
    if twelve:
        cnt[::3] = 12
    off = (np.cumsum(cnt) - cnt).astype(np.int32)
    rows = int(cnt[:n_valid].sum())
    cnt[n_valid:], off[n_valid:] = 8, 0                               # past the count: in range, wrong
    aw = (0.25 * rng.standard_normal(256)).astype(F32)
    ab = F32(0.35)
    a64 = f64(aw)
    z = rng.random((rows, 256))
    m = (z >= 0.01) & (z <= 0.99)                                     # the others: signed zeros
    h0 = rng.standard_normal((rows, 256)) * m
    y_t = rng.uniform(-30, 30, rows)
    y_t[:min(rows, 6)] = [19.0, 21.0, 25.0, -25.0, 19.9, 20.1][:min(rows, 6)]
    t = y_t + 1 - float(ab)
    h = (h0 + ((t - h0 @ a64) / ((a64 * a64 * m).sum(1)))[:, None] * a64 * m).astype(F32)
    h[z < 0.01] = 0.0
    h[z > 0.99] = -0.0
    R = (cap + 4 + SR - 1) // SR
    raydir = rng.standard_normal((R, 3)).astype(F32)
    raydir /= np.linalg.norm(raydir, axis=1, keepdims=True).astype(F32)
    return dict(n_valid=n_valid, cap=cap, SR=SR, R=R, rows=rows, vs_cnt=cnt, vs_off=off, vs_item=rng.permutation(R * SR)[:cap].astype(np.int32), H=h,
                wagg=(rng.random(rows) * np.where(rng.random(rows) < 0.2, 1e-3, 1.0)).astype(F32), alpha_w=aw, alpha_b=np.array([ab], F32), raydir=raydir,
                counts=counts_of(R * SR, n_valid), row_s=np.repeat(np.arange(n_valid), cnt[:n_valid]))


def ref_ksum(inp):
    """sigma = sum_k w softplus(alpha_k - 1) (point_aggregators.py:1005, :471-476; threshold 20), feat = sum_k w h_k (:1008-1026), and the view-direction
    encoding positional_encoding(viewdirs, 4, ori=True)[3:] = [sin x12 | cos x12] (:909-913)."""
    n, s = inp["n_valid"], inp["row_s"]
    h, w, aw, ab = f64(inp["H"]), f64(inp["wagg"]), f64(inp["alpha_w"]), float(inp["alpha_b"][0])
    y = h @ aw + ab - 1.0
    dy = sum_bound(np.abs(h) @ np.abs(aw) + abs(ab) + 1.0, 258)       # 256 products, the bias, the 1
    sig = 1.0 / (1.0 + np.exp(-y))
    sp = np.where(y > 20, y, np.log1p(np.exp(np.minimum(y, 50))))
    # log1pf(expf(y)): y through sigmoid(y); expf's 8 U of e through e / (1 + e); log1pf's 8 U of the value.  Next to y = 20 the float32 value may take the
    # other branch than float64's: the two differ by log1p(e^-y) < e^-20 there.
    dsp = sig * dy + 8 * U * sig + 8 * U * np.abs(sp) + np.where(np.abs(y - 20) <= dy, np.exp(-20.0), 0.0)
    sigma, bsig = np.zeros((n,)), np.zeros((n,))
    np.add.at(sigma, s, sp * w)
    np.add.at(bsig, s, w * dsp)
    asum = np.zeros((n,))
    np.add.at(asum, s, np.abs(sp * w))
    cnt = f64(inp["vs_cnt"][:n])
    feat, afeat = np.zeros((n, 256)), np.zeros((n, 256))
    np.add.at(feat, s, h * w[:, None])
    np.add.at(afeat, s, np.abs(h * w[:, None]))
    rd = inp["raydir"][inp["vs_item"][:n] // inp["SR"]]
    band = 2.0 ** np.arange(4)
    a = (f64(rd)[:, :, None] * band).reshape(n, 12)                  # exact arguments
    vd = np.concatenate([np.sin(a), np.cos(a)], 1)
    return dict(sigma=(sigma, bsig + (cnt + 2) * U * asum), feat=(feat, (cnt[:, None] + 2) * U * afeat), viewdir=(vd, 8 * U * np.abs(vd) + TINY))


def emul_ksum(inp):
    n = inp["n_valid"]
    aw, ab = inp["alpha_w"].reshape(64, 4), inp["alpha_b"][0]
    H = inp["H"].reshape(-1, 64, 4)
    p = H * aw
    d = wave_xor_sum(((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3])[..., 0]
    with np.errstate(over="ignore"):
        yv = (d + ab) - F32(1.0)
        sp = np.where(yv > 20, yv, np.log1p(np.exp(yv))).astype(F32)
    sigma, feat = np.zeros((n,), F32), np.zeros((n, 256), F32)
    for s in range(n):
        for r in range(inp["vs_off"][s], inp["vs_off"][s] + inp["vs_cnt"][s]):
            sigma[s] = sigma[s] + sp[r] * inp["wagg"][r]
            feat[s] = feat[s] + inp["H"][r] * inp["wagg"][r]
    rd = inp["raydir"][inp["vs_item"][:n] // inp["SR"]]
    a = (rd[:, :, None] * (2.0 ** np.arange(4)).astype(F32)).reshape(n, 12)
    return dict(sigma=sigma, feat=feat, viewdir=np.concatenate([np.sin(a), np.cos(a)], 1).astype(F32), y=yv)


# ================================================================================================ 5. hnr_final_color
FINAL_BLOCKS = 8192                                 # the grid's limit (hnr_final_color): 16 samples per block and trip
FINAL_SHAPES = [(4, 1), (6, 3), (6, 4), (8, 5), (16 * FINAL_BLOCKS + 24, 16 * FINAL_BLOCKS + 21)]      # (cap, n_valid); the last: a second trip of the sample loop
FINAL_LAYOUTS = [(48, 0, 128), (45, 0, 132), (48, 1, 128)]                                            # (ldy, offset of Y's base in floats, ldcf): vector, scalar, scalar


def make_final(cap, n_valid, ldy, ldcf, seed):
    rng = np.random.default_rng(seed)
    items = cap + 7
    vs_item = rng.permutation(items)[:cap].astype(np.int32)           # scattered; entries past the count name items that must stay untouched
    w = (rng.standard_normal((3, 128)) * np.array([[0.6], [0.08], [0.3]])).astype(F32)
    b = np.array([0.3, -0.2, 0.1], F32)
    Y = np.full((cap, ldy), np.nan, F32)
    CF = np.full((cap, ldcf), np.nan, F32)
    Y[:n_valid, :45] = rng.standard_normal((n_valid, 45)).astype(F32)
    cf = rng.standard_normal((n_valid, 128))
    # the first logit spread over -30 .. 30: CF moved along w[0]
    x = cf.copy()
    x[:, :45] += Y[:n_valid, :45]
    w0 = f64(w[0])
    t = np.linspace(-30, 30, n_valid) if n_valid > 1 else np.array([30.0])
    cf += ((t - float(b[0]) - x @ w0) / (w0 @ w0))[:, None] * w0
    CF[:n_valid, :128] = cf.astype(F32)
    sigma = np.full((cap,), np.nan, F32)
    sigma[:n_valid] = rng.random(n_valid).astype(F32) * 30
    return dict(cap=cap, n_valid=n_valid, ldy=ldy, ldcf=ldcf, items=items, vs_item=vs_item, Y=Y, CF=CF, w_fin=w, b_fin=b, sigma=sigma,
                counts=counts_of(items, n_valid))


def ref_final(inp):
    """rgb = 1.002 sigmoid(w x + b) - 0.001, x = [Y + CF[:, :45] | CF[:, 45:]] (point_aggregators.py:1294-1295, :1334, :478-482) -> (rgb, bound, logits)."""
    n = inp["n_valid"]
    x = f64(inp["CF"][:n, :128]).copy()
    x[:, :45] += f64(inp["Y"][:n, :45])
    w, b = f64(inp["w_fin"]), f64(inp["b_fin"])
    z = x @ w.T + b
    dz = sum_bound(np.abs(x) @ np.abs(w).T + np.abs(b), 129)          # 128 products of a once-rounded x and the bias (tests/backward_glue_ref.py ref_final)
    sg = 1.0 / (1.0 + np.exp(-z))
    dsg = sg * (1 - sg) * dz + 8 * U * sg * (1 - sg) + 2 * U * sg     # expf's 4 ulp, the addition, the division
    rgb = 1.002 * sg - 0.001
    # the two constants rounded to float32 (U each, relative), the product, the subtraction
    return rgb, 1.002 * dsg + 2 * U * 1.002 * sg + U * 0.001 + U * np.abs(rgb), z


def emul_final(inp):
    n = inp["n_valid"]
    x = inp["CF"][:n, :128].copy()
    x[:, :45] = inp["Y"][:n, :45] + x[:, :45]
    out = np.zeros((n, 3), F32)
    with np.errstate(over="ignore"):
        for j in range(3):
            p = (x * inp["w_fin"][j]).reshape(n, 16, 8)
            r = np.zeros((n, 16), F32)
            for e in range(8):
                r = r + p[:, :, e]
            r = wave_xor_sum(r, (1, 2, 4, 8))[:, 0]                   # the four DPP steps: pairs, quads, halves, the row
            sg = F32(1.0) / (F32(1.0) + np.exp(-(r + inp["b_fin"][j])))
            out[:, j] = sg * C1002 - F32(0.001)
    return out


# ================================================================================================ 6. hnr_composite, 7. hnr_ray_march
COMPOSITE_R = [1, 255, 256, 257, 600]               # 256 rays per block
COMPOSITE_SR = [1, 2, 24]
VSIZE_Z = F32(0.02)
E10 = F32(1e-10)


def make_composite(R, SR, K, seed):
    """Rays whose samples advance by a gap well below 2 vsize_z (0.01 .. 0.03), a gap well above it (0.1), no gap (the same position twice: dist = 0 exactly)
    or backwards (-0.05: the running maximum stays, dist = 0 exactly); holes in mid-ray; sigma of 0, moderate, and saturating (1e4)."""
    rng = np.random.default_rng(seed)
    campos, camrot = make_camera(seed)
    kind = rng.choice(4, (R, SR), p=[0.6, 0.15, 0.1, 0.15])
    kind[:, 0] = 0
    step = np.where(kind == 0, rng.uniform(0.01, 0.03, (R, SR)), np.where(kind == 1, 0.1, 0.0))
    step[:, 0] = 0.0
    zc = 2.0 + rng.random((R, 1)) + np.cumsum(step, 1) - np.where(kind == 3, 0.05, 0.0)      # a backward slot; the next one continues from the maximum
    c = np.stack([0.3 * zc, -0.2 * zc, zc], -1)
    loc_w = cam_to_world(c, campos, camrot)
    for s in range(1, SR):
        same = kind[:, s] == 2
        loc_w[same, s] = loc_w[same, s - 1]
    nsamp = rng.integers(0, SR + 1, R).astype(np.int32)
    nsamp[:3] = [0, 1, SR][:min(R, 3)]
    ray_mask = (rng.random(R) < 0.8).astype(np.int8)
    ray_mask[:3] = 1
    if R > 3:
        ray_mask[3] = 0
    pidx = rng.integers(0, 500, (R, SR, K)).astype(np.int32)
    pidx[rng.random((R, SR)) < 0.2] = -1                              # holes
    dec = rng.random((R, SR, 4)).astype(F32)
    sk = rng.choice(3, (R, SR), p=[0.15, 0.7, 0.15])
    dec[..., 0] = np.where(sk == 0, 0.0, np.where(sk == 1, rng.uniform(0, 60, (R, SR)), 1e4)).astype(F32)
    return dict(R=R, SR=SR, K=K, campos=campos, camrot=camrot, loc_w=loc_w, nsamp=nsamp, ray_mask=ray_mask, pidx=pidx, decoded=dec,
                bg=np.array([0.9, 0.2, 0.6], F32), vsize_z=VSIZE_Z)


def padded(inp, use_nsamp):
    """The inputs as the padded query leaves them (position 0, no neighbour in the slots past nsamp; neural_points_volumetric_model.py reads those)."""
    loc, pidx, dec = inp["loc_w"].copy(), inp["pidx"].copy(), inp["decoded"].copy()
    if use_nsamp:
        past = np.arange(inp["SR"])[None, :] >= inp["nsamp"][:, None]
        loc[past], pidx[past], dec[past] = 0.0, -1, 0.0
    return loc, pidx, dec


def poisoned(inp):
    """The same, with NaN / a wrong id past nsamp: the nsamp form must not read them."""
    loc, pidx, dec = inp["loc_w"].copy(), inp["pidx"].copy(), inp["decoded"].copy()
    past = np.arange(inp["SR"])[None, :] >= inp["nsamp"][:, None]
    loc[past], pidx[past], dec[past] = np.nan, 3, np.nan
    return loc, pidx, dec


def z32(loc, campos, camrot):
    return cam32(loc, campos, camrot)[..., 2]


def ray_dist(inp, use_nsamp, unit_mode):
    """ray_dist (neural_points_volumetric_model.py:331-339): the differences of the running maximum of the camera depths, the last slot and every difference
    below 1e-8 (and, in unit mode, above 2 vsize_z) replaced by vsize_z.  The decisions are taken on the float32 values, which the inputs keep exactly on
    (dist = 0) or well clear of the thresholds.  -> (dist float32 as the kernel forms it, dist float64, bound, ray_valid)."""
    loc, pidx, _ = padded(inp, use_nsamp)
    R, SR, vz = inp["R"], inp["SR"], inp["vsize_z"]
    z = z32(loc, inp["campos"], inp["camrot"])
    z_f = np.maximum.accumulate(z, 1)
    z64, bz = cam64(loc, inp["campos"], inp["camrot"])
    z64, bz = z64[..., 2], bz[..., 2]
    arg = np.zeros((R, SR), np.int64)                                 # the slot that holds the running maximum (decided in float32)
    for s in range(1, SR):
        arg[:, s] = np.where(z[:, s] > z_f[:, s - 1], s, arg[:, s - 1])
    zm64, bzm = np.take_along_axis(z64, arg, 1), np.take_along_axis(bz, arg, 1)
    d_f, d64, bd = np.full((R, SR), vz, F32), np.full((R, SR), float(vz)), np.zeros((R, SR))
    if SR > 1:
        d_f[:, :-1] = z_f[:, 1:] - z_f[:, :-1]
        d64[:, :-1] = zm64[:, 1:] - zm64[:, :-1]
        bd[:, :-1] = np.where(arg[:, 1:] == arg[:, :-1], 0.0, bzm[:, 1:] + bzm[:, :-1] + U * np.abs(d64[:, :-1]))
    sub = (d_f < F32(1e-8)) | ((d_f > F32(2.0) * vz) if unit_mode else False)
    d_f[sub], d64[sub], bd[sub] = vz, float(vz), 0.0
    valid = pidx[..., 0] >= 0
    return d_f, d64, bd, valid


def ref_march(dist, bdist, valid, feat, bg):
    """ray_march (models/rendering/diff_ray_marching.py:508-557): opacity = 1 - exp(-sigma dist), T the running product of (1 - opacity + 1e-10),
    blend weight = opacity T, colour = sum rgb weight (+ bg T_end).  name -> (float64, bound); `dist` carries the bound `bdist`."""
    R, SR = dist.shape
    sigma = np.where(valid, f64(feat[..., 0]), 0.0)
    rd = np.where(valid, dist, 0.0)
    a = sigma * rd
    ba = sigma * np.where(valid, bdist, 0.0) + U * np.abs(a)
    e = np.exp(-a)
    o = 1.0 - e
    bo = e * ba + 8 * U * e + U * np.abs(o)                           # the argument through e^-a, expf's 4 ulp, the subtraction
    f = 1.0 - o + 1e-10
    bf = bo + U * np.abs(1.0 - o) + U * f + U * 1e-10                 # two additions, the constant's rounding
    T, bT = np.ones((R, SR + 1)), np.zeros((R, SR + 1))
    for s in range(SR):
        T[:, s + 1] = T[:, s] * f[:, s]
        bT[:, s + 1] = bT[:, s] * f[:, s] + T[:, s] * bf[:, s] + U * T[:, s + 1]
    w = o * T[:, :SR]
    bw = bo * T[:, :SR] + o * bT[:, :SR] + U * w
    rgb = f64(feat[..., 1:4])
    col = (rgb * w[..., None]).sum(1)
    bcol = (rgb * bw[..., None]).sum(1)
    terms = (rgb * w[..., None]).sum(1)
    n = SR
    if bg is not None:
        col = col + f64(bg) * T[:, SR:]
        bcol = bcol + f64(bg) * bT[:, SR:]
        terms = terms + f64(bg) * T[:, SR:]
        n = SR + 1
    return dict(opacity=(o, bo), T=(T[:, :SR], bT[:, :SR]), T_end=(T[:, SR], bT[:, SR]), blend=(w, bw), color=(col, bcol + sum_bound(terms, n)))


def ref_composite(inp, use_nsamp, unit_mode):
    """ray_dist + ray_march + fill_invalid (diff_ray_marching.py:87-126): rays with ray_mask = 0 get the background colour, opacity 0, is_background 1."""
    d_f, d64, bd, valid = ray_dist(inp, use_nsamp, unit_mode)
    _, _, dec = padded(inp, use_nsamp)
    ref = ref_march(d64, bd, valid, dec, inp["bg"])
    off = inp["ray_mask"] == 0
    out = {}
    for k, fill in (("opacity", 0.0), ("blend", 0.0), ("T_end", 1.0), ("color", f64(inp["bg"]))):
        v, b = ref[k][0].copy(), ref[k][1].copy()
        v[off], b[off] = fill, 0.0
        out[k] = (v, b)
    return out


def emul_march(dist, valid, feat, bg):
    R, SR = dist.shape
    T, c = np.ones((R,), F32), np.zeros((R, 3), F32)
    o_, T_, w_ = np.zeros((R, SR), F32), np.zeros((R, SR), F32), np.zeros((R, SR), F32)
    with np.errstate(over="ignore", under="ignore"):
        for s in range(SR):
            sigma = np.where(valid[:, s], feat[:, s, 0], F32(0.0)).astype(F32)
            o = F32(1.0) - np.exp(-sigma * dist[:, s])
            w = o * T
            o_[:, s], T_[:, s], w_[:, s] = o, T, w
            c = c + feat[:, s, 1:4] * w[:, None]
            T = T * ((F32(1.0) - o) + E10)
    if bg is not None:
        c = c + bg * T[:, None]
    return dict(opacity=o_, T=T_, blend=w_, T_end=T, color=c)


def emul_composite(inp, use_nsamp, unit_mode):
    d_f, _, _, valid = ray_dist(inp, use_nsamp, unit_mode)
    _, _, dec = padded(inp, use_nsamp)
    out = emul_march(np.where(valid, d_f, F32(0.0)).astype(F32), valid, dec, inp["bg"])
    off = inp["ray_mask"] == 0
    out["opacity"][off], out["blend"][off], out["T_end"][off], out["color"][off] = 0.0, 0.0, 1.0, inp["bg"]
    return out


# ================================================================================================ 8. hnr_probe_outputs
PROBE_R = [1, 31, 32, 33]                           # eight lanes per ray, 32 rays per block


def make_probe(R, seed, SR=5, K=8, F=32, n_points=150):
    rng = np.random.default_rng(seed)
    campos, camrot = make_camera(seed)
    cloud = make_cloud(n_points, campos, camrot, seed)
    opacity = rng.random((R, SR)).astype(F32)
    opacity[::4, 3] = opacity[::4, 1] = F32(0.99)                     # an exact tie: the first maximum wins
    opacity[2::5] = 0.0                                               # an all-zero ray: slot 0
    loc_w = rng.standard_normal((R, SR, 3)).astype(F32)
    cnt = rng.integers(0, K + 1, (R, SR))
    occ = np.arange(K)[None, None, :] < cnt[..., None]
    pidx = np.where(occ, rng.integers(0, n_points, (R, SR, K)), -1).astype(np.int32)
    weight = np.where(occ, rng.random((R, SR, K)), 0.0).astype(F32)  # empty slots: point 0 with weight 0 (neural_points.py:711)
    conf_c = rng.uniform(1e-4, 1, (R, SR, K)).astype(F32)
    d = dict(R=R, SR=SR, K=K, F=F, n_points=n_points, opacity=opacity, loc_w=loc_w, pidx=pidx, weight=weight, conf_c=conf_c)
    d.update(cloud)
    return d


def ref_probe(inp):
    """neural_points_volumetric_model.py:392-416: the sample of maximum opacity (torch.max: the first), its position, the distance to the nearest of its K
    gathered points (empty slots gather point 0), and the weight x conf_coefficient sums of their attributes."""
    R, K = inp["R"], inp["K"]
    best = np.argmax(inp["opacity"], 1)                               # the first maximum
    r = np.arange(R)
    pid = np.maximum(inp["pidx"][r, best], 0)
    l = inp["loc_w"][r, best]
    dlt = f64(inp["xyz"][pid]) - f64(l)[:, None, :]
    nrm = np.sqrt((dlt ** 2).sum(-1))
    far = nrm.min(1)
    w = f64(inp["weight"][r, best]) * f64(inp["conf_c"][r, best])     # [R, K]
    out = dict(best=best, max_opacity=inp["opacity"][r, best], max_loc=l, far=(far, 4 * U * far))    # 3.5 U as in ref_gather_rows (no product with a clamp)
    for k in ("color", "dir", "conf", "emb"):
        a = f64(inp[k][pid]).reshape(R, K, -1)
        t = a * w[..., None]
        out[k] = (t.sum(1), (K + 3) * U * np.abs(t).sum(1))           # K products of a once-rounded weight
    return out


def emul_probe(inp):
    R, K = inp["R"], inp["K"]
    r = np.arange(R)
    best = np.zeros((R,), np.int64)
    bo = inp["opacity"][:, 0].copy()
    for s in range(1, inp["SR"]):
        o = inp["opacity"][:, s]
        best, bo = np.where(o > bo, s, best), np.where(o > bo, o, bo)
    pid = np.maximum(inp["pidx"][r, best], 0)
    l = inp["loc_w"][r, best]
    dlt = inp["xyz"][pid] - l[:, None, :]
    far = np.sqrt((dlt[..., 0] * dlt[..., 0] + dlt[..., 1] * dlt[..., 1]) + dlt[..., 2] * dlt[..., 2]).min(1)
    w = inp["weight"][r, best] * inp["conf_c"][r, best]
    out = dict(best=best, far=far)
    for k in ("color", "dir", "conf", "emb"):
        a = inp[k][pid].reshape(R, K, -1)
        acc = np.zeros((R, a.shape[-1]), F32)
        for j in range(K):
            acc = acc + a[:, j] * w[:, j, None]
        out[k] = acc
    return out


# ================================================================================================ 9. hnr_gather_points
POINTS_N = [1, 31, 32, 33]                          # eight lanes per entry, 32 entries per block


def make_points(n, seed, n_points=60):
    rng = np.random.default_rng(seed)
    campos, camrot = make_camera(seed)
    d = dict(n=n, n_points=n_points, campos=campos, camrot=camrot)
    d.update(make_cloud(n_points, campos, camrot, seed))
    pidx = rng.integers(0, n_points, n + 4).astype(np.int32)         # (the entries past n: valid ids)
    pidx[rng.random(n + 4) < 0.3] = -1
    if n > 1:
        pidx[1] = -1
    d["pidx"] = pidx
    return d


def ref_points(inp):
    """neural_points.py:709-720: the gather with the index clamped at 0, the mask, and w2pers (:607-613) of the gathered positions."""
    pid = np.maximum(inp["pidx"][:inp["n"]], 0)
    return dict(pid=pid, mask=(inp["pidx"][:inp["n"]] >= 0).astype(np.uint8), pers=w2pers64(inp["xyz"][pid], inp["campos"], inp["camrot"]))


def emul_points(inp):
    pid = np.maximum(inp["pidx"][:inp["n"]], 0)
    return dict(pers=w2pers32(inp["xyz"][pid], inp["campos"], inp["camrot"]))
