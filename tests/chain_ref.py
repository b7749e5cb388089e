"""Synthetic cases, a float64 reference and a float32 restatement of the fused per-neighbour chain (csrc/chain.hip: chain_gather_kernel; csrc/chain_ws.hip:
chain_ws_kernel + chain_sigma_kernel; csrc/chain.hip: chain_kernel<4>), in the manner of tests/forward_glue_ref.py, whose camera, cloud, counts and
per-row geometry (ref_gather_rows / emul_gather_rows) are used as they are.  No scene, no query, no fixture; numpy only, no GPU.

A SPEC is (n_big, n_small, n_tiny, cap, classes[, wide]): samples with more than four neighbours, with 3..4, with 1..2; the capacity passed to the entry
points; the layout hnr_chain_plan(classes) would list them in.  A spec with big samples only and classes = 0 is a plain one-class list whose samples
take every neighbour count 1..8 in turn.  The SAMPLES of a spec (items, neighbour ids, positions) depend on (n_big, n_small, n_tiny, seed, wide) only, so
that the same samples can be listed with 0, 1 or 2 classes and at several capacities: the references are computed once, on the one-class list
(ascending items), and re-ordered by `pos` (the place of every listed sample in the one-class list).

tests/test_chain_ref.py checks this module without a GPU; tests/test_chain_edges_gpu.py runs the kernels against it.
The bound of the device (tests/test_chain_gpu.py's): per row, relative to the row maximum of the float64 value, FACTOR x e32 + FLOOR with e32 the
same figure of emul_chain -- float32 on the CPU, never the device --, 1e-6 instead of 3e-7 for sigma (relative to the value).  E32_LIMIT keeps it
honest: a case whose float32 restatement is itself worse than 4e-6 of the row maximum would make the bound wide, and is not accepted.
"""
import functools

import numpy as np

from tests import forward_glue_ref as G
from tests.forward_glue_ref import F32, U, TINY, f64, CNT_VALID, CNT_SMALL, CNT_TINY, make_camera, make_cloud, counts_of   # noqa: F401

N_POINTS, SR, K = 300, 3, 8
SLOPE = float(F32(0.01))                            # nn.LeakyReLU's default, as the float the entry point receives
ALPHA_SCALE, ALPHA_BIAS = 30.0, 16.0               # alpha_branch x 30 and a bias that centres the logits: they span about -30 .. 30 (softplus' y > 20 branch)
FACTOR, FLOOR, FLOOR_SIGMA, E32_LIMIT = 2.5, 3e-7, 1e-6, 4e-6
LAYERS = ("H1", "H2", "H3", "H4")


# ================================================================================================ the shape lists (C = number of CUs: the grid's limit)
TILE_N = [1, 15, 16, 17, 127, 128, 129]             # one class, cap = n: around the 16-sample tile; grids of 1, 2, 8 and 9 (both branches of xcd_order)


def one(n, cap=None, wide=False):
    return (n, 0, 0, n if cap is None else cap, 0) + ((True,) if wide else ())


def grid_n(C):
    """One class, cap = n: every workgroup one tile; exactly one workgroup a second tile; two or three tiles each; one extra tile per XCD."""
    return [16 * C - 1, 16 * C, 16 * C + 1, 32 * C + 17, 16 * (C + 8) + 1]


def cap_cases(C):
    """(n_valid, cap): the count far below the capacity that sizes the grid and the workspace; the last has nothing to do."""
    return [(1, 16 * C), (17, 16 * C + 5), (16 * 9 + 3, 64 * C), (0, 64)]


def class_cases(C):
    """(n_big, n_small, n_tiny, cap): class boundaries inside a tile, empty classes, a class of one sample, a grid of 1 facing 3 tiles, a grid of 8 facing
    10 tiles, more tiles than workgroups in every class; the last: a capacity that cuts the list inside the small class (33 of 65 small samples with two
    classes; with one class the small class holds the tiny samples too)."""
    out = [(5, 6, 5, 16), (16, 32, 64, None), (17, 33, 65, None), (0, 1, 0, None), (0, 0, 1, None), (0, 0, 130, None), (113, 8, 7, 128),
           (16 * C + 1, 32 * C + 1, 64 * C + 1, None), (33, 65, 17, 33 + 33)]
    return [(b, s, t, b + s + t if cap is None else cap) for b, s, t, cap in out]


WIDE_SPECS = [one(17, wide=True), (17, 33, 65, 115, 1, True), (17, 33, 65, 115, 2, True)]


def all_specs(C):
    specs = [one(n) for n in TILE_N] + [one(n) for n in grid_n(C)] + [one(n, cap) for n, cap in cap_cases(C)]
    for b, s, t, cap in class_cases(C):
        specs += [(b, s, t, cap, classes) for classes in (1, 2)]
    return list(dict.fromkeys(specs + WIDE_SPECS))                   # (C = 8: three of GRID_N are in TILE_N already)


def seed_of(spec):
    """One seed per set of samples (the layouts and capacities of a set share it)."""
    return 11 + spec[0] + 3 * spec[1] + 7 * spec[2]


def is_wide(spec):
    return len(spec) > 5 and bool(spec[5])


# ================================================================================================ weights, samples, cases
@functools.lru_cache(maxsize=None)
def make_weights(wide=False):
    """block1.{0,2}, block3.{0,2}, alpha_branch.0 drawn like PointAggregator's initialisation (models/helpers/networks.py:83-122, :163-172: Xavier uniform
    with the LeakyReLU gain, nn.Linear's default biases), alpha_branch scaled so that the logits reach both sides of softplus' threshold.
    wide: block1.2's outputs scaled by 2^-6 .. 2^6 (undone in block3.0's columns), block3.2 by 3e-4 and alpha_branch by 1 / 3e-4."""
    rng = np.random.default_rng(77)
    gain = np.sqrt(2.0 / (1.0 + 0.01 ** 2))

    def lin(n_out, n_in, g):
        a = g * np.sqrt(2.0 / (n_in + n_out)) * np.sqrt(3.0)
        return rng.uniform(-a, a, (n_out, n_in)).astype(F32), rng.uniform(-1, 1, n_out).astype(F32) / F32(np.sqrt(n_in))

    w = {}
    w["w10"], w["b10"] = lin(256, 284, gain)
    w["w12"], w["b12"] = lin(256, 256, gain)
    w["w30"], w["b30"] = lin(256, 263, gain)
    w["w32"], w["b32"] = lin(256, 256, gain)
    aw, _ = lin(1, 256, 1.0)
    w["aw"], w["ab"] = (aw.reshape(256) * F32(ALPHA_SCALE)).astype(F32), np.array([ALPHA_BIAS], F32)
    if wide:
        s1 = np.exp2(np.random.default_rng(3).integers(-6, 7, 256)).astype(F32)
        w["w12"], w["b12"] = w["w12"] * s1[:, None], w["b12"] * s1
        w["w30"] = w["w30"].copy()
        w["w30"][:, :256] /= s1[None, :]
        w["w32"], w["b32"] = (w["w32"] * F32(3e-4)).astype(F32), (w["b32"] * F32(3e-4)).astype(F32)
        w["aw"] = (w["aw"] / F32(3e-4)).astype(F32)
    return {k: np.ascontiguousarray(v) for k, v in w.items()}


@functools.lru_cache(maxsize=None)
def _samples(n_big, n_small, n_tiny, seed, wide):
    """The samples of a spec in one-class order (ascending items).  Neighbour counts cycle through every value of the sample's class; the classes are
    interleaved along the items; unlisted items keep NaN positions and eight valid neighbours."""
    rng = np.random.default_rng(seed)
    campos, camrot = make_camera(seed)
    cloud = make_cloud(N_POINTS, campos, camrot, seed)
    if wide:
        cloud["emb"] = (cloud["emb"] * np.exp2(np.random.default_rng(1).integers(-6, 7, (N_POINTS, 1))).astype(F32)).astype(F32)
    total = n_big + n_small + n_tiny
    plain = n_small == 0 and n_tiny == 0
    nb_of = [(1 + (np.arange(n_big) + 7) % 8) if plain else (5 + (np.arange(n_big) + 3) % 4), 3 + (np.arange(n_small) + 1) % 2, 1 + (np.arange(n_tiny) + 1) % 2]
    R = (total + 11 + SR - 1) // SR
    items = R * SR
    perm = rng.permutation(items)
    item = np.sort(perm[:total]).astype(np.int32)
    cls = rng.permutation(np.repeat(np.arange(3), [n_big, n_small, n_tiny]))
    nb = np.zeros((total,), np.int64)
    for c in range(3):
        nb[cls == c] = nb_of[c]
    pidx = rng.integers(0, N_POINTS, (items, K)).astype(np.int32)
    sub = pidx[item]
    sub[np.arange(K)[None, :] >= nb[:, None]] = -1
    sub[:min(8, total), 0] = np.arange(min(8, total))                # the points with the confidences on and around the clamps; id 0
    for s in np.flatnonzero(nb >= 2)[:2]:
        sub[s, nb[s] - 1] = N_POINTS - 1                              # id N - 1, twice within the first tile
    pidx[item] = sub
    loc_w = np.full((items, 3), np.nan, F32)
    loc_w[item] = (cloud["xyz"][sub[:, 0]].astype(np.float64) + rng.uniform(-0.08, 0.08, (total, 3))).astype(F32)
    if total:
        loc_w[item[0]] = cloud["xyz"][sub[0, 0]]                      # a sample on its slot-0 point: norm 0, the 1e-6 clamp
    raydir = rng.standard_normal((R, 3)).astype(F32)
    raydir /= np.linalg.norm(raydir, axis=1, keepdims=True).astype(F32)
    d = dict(total=total, R=R, items=items, item=item, cls=cls, nb=nb, pidx=pidx, loc_w=loc_w, raydir=raydir, campos=campos, camrot=camrot,
             unlisted=np.sort(perm[total:]).astype(np.int32))
    d.update(cloud)
    w = make_weights(wide)
    x = np.concatenate([f64(cloud["emb"]), G.pe64(cloud["emb"], 3)[0]], 1)                # [emb | PE3(emb)]: block1.0's point-only 224 columns
    d["table64"] = x @ f64(w["w10"][:, :224]).T
    d["table"] = d["table64"].astype(F32)                             # rounded once: what the kernel and both references read
    return d


def make_chain(spec, seed=None):
    """The inputs of hnr_chain_gather* / hnr_chain_forward for a spec: the samples listed class by class as hnr_chain_plan(classes) lists them (ascending
    items inside a class), the first min(total, cap) of them kept, the counts it leaves, poison beyond the count."""
    n_big, n_small, n_tiny, cap, classes = spec[:5]
    wide = is_wide(spec)
    S = _samples(n_big, n_small, n_tiny, seed_of(spec) if seed is None else seed, wide)
    total = S["total"]
    key = np.zeros((total,), np.int64) if classes == 0 else np.minimum(S["cls"], classes)
    pos = np.argsort(key, kind="stable")                              # list place -> place in the one-class list
    n = min(total, cap)
    first = min(int((key == 0).sum()), n)
    second = min(int((key == 1).sum()), n - first)
    counts = counts_of(S["items"], total)
    counts[CNT_SMALL], counts[CNT_TINY] = (second, n - first - second) if classes > 1 else (n - first if classes else 0, 0)
    vs_item = S["unlisted"][np.arange(max(cap, 1) + 3) % S["unlisted"].size].copy()       # beyond the count: valid items that are not listed (NaN positions)
    vs_item[:n] = S["item"][pos[:n]]
    cnt = S["nb"][pos[:n]].astype(np.int32)
    off = (np.cumsum(cnt) - cnt).astype(np.int32)
    d = dict(S)
    d.update(make_weights(wide))
    d.update(spec=spec, n_valid=n, cap=cap, classes=classes, K=K, SR=SR, n_points=N_POINTS, pos=pos[:n], vs_item=vs_item.astype(np.int32), vs_cnt=cnt,
             vs_off=off, counts=counts, rows=int(cnt.sum()), key=key[pos[:n]])
    d["row_s"] = np.repeat(np.arange(n), cnt)
    d["row_k"] = np.arange(d["rows"]) - off[d["row_s"]]
    d["row_item"] = d["vs_item"][d["row_s"]]
    d["row_pid"] = d["pidx"][d["row_item"], d["row_k"]]
    return d


def one_class_of(spec):
    """The same samples in the one-class layout, all of them."""
    return (spec[0], spec[1], spec[2], spec[0] + spec[1] + spec[2], 0) + tuple(spec[5:])


# ================================================================================================ float64 reference, float32 restatement
def _softplus_m1(alpha, xp_exp=np.exp):
    y = alpha - 1
    with np.errstate(over="ignore"):
        return np.where(y > 20, y, np.log1p(xp_exp(np.minimum(y, 50))))


def ref_chain(case, table=None):
    """float64: H1 = LeakyReLU(PE5 W0d^T + b + table[pid]), H2, H3 on [H2 | colour | dir - v | dir . v], H4, alpha (point_aggregators.py:948, :957-972,
    :1005), X5 = sum_k wagg H4, sigma = sum_k wagg softplus(alpha - 1) (:1008-1026, :471-476), the view-direction columns (:909-913).  The rows'
    distances, PE5, extras and weights are ref_gather_rows'; `table`: the per-point addend (default: the float32 table the kernel reads)."""
    n, pid, s = case["n_valid"], case["row_pid"], case["row_s"]
    if n == 0:                                                        # nothing listed
        z = lambda *shape: np.zeros(shape)
        return dict(H1=z(0, 256), H2=z(0, 256), H3=z(0, 256), H4=z(0, 256), alpha=z(0), X5=z(0, 256), sigma=z(0), viewdir=(z(0, 24), z(0, 24)),
                    weight=(z(0), z(0)), confc=np.zeros((0,), F32), wagg=(z(0), z(0)), pe5=(z(0, 60), z(0, 60)), ext=z(0, 7))
    g = G.ref_gather_rows(case)
    tab = f64(case["table"] if table is None else table)
    lk = lambda x: np.where(x > 0, x, x * SLOPE)
    w = {k: f64(case[k]) for k in ("w10", "b10", "w12", "b12", "w30", "b30", "w32", "b32", "aw", "ab")}
    ext = np.concatenate([f64(case["color"][pid]), g["ext"][0]], 1)
    H1 = lk(g["pe5"][0] @ w["w10"][:, 224:284].T + w["b10"] + tab[pid])
    H2 = lk(H1 @ w["w12"].T + w["b12"])
    H3 = lk(np.concatenate([H2, ext], 1) @ w["w30"].T + w["b30"])
    H4 = lk(H3 @ w["w32"].T + w["b32"])
    alpha = H4 @ w["aw"] + w["ab"][0]
    wagg = g["wagg"][0]
    X5, sigma = np.zeros((n, 256)), np.zeros((n,))
    np.add.at(X5, s, H4 * wagg[:, None])
    np.add.at(sigma, s, wagg * _softplus_m1(alpha))
    a = (f64(case["raydir"][case["vs_item"][:n] // SR])[:, :, None] * 2.0 ** np.arange(4)).reshape(n, 12)      # exact arguments (forward_glue_ref.ref_ksum)
    vd = np.concatenate([np.sin(a), np.cos(a)], 1)
    return dict(H1=H1, H2=H2, H3=H3, H4=H4, alpha=alpha, X5=X5, sigma=sigma, viewdir=(vd, 8 * U * np.abs(vd) + TINY), weight=g["weight"], confc=g["confc"],
                wagg=g["wagg"], pe5=g["pe5"], ext=ext)


def _emul_rows(case, chunk=64):
    """emul_gather_rows over the case, `chunk` samples at a time (its weight loop compares every row with every other row of its input)."""
    n, s = case["n_valid"], case["row_s"]
    outs = []
    for a in range(0, n, chunk):
        r = (s >= a) & (s < a + chunk)
        sub = dict(case, row_s=s[r] - a, row_item=case["row_item"][r], row_pid=case["row_pid"][r], row_k=case["row_k"][r])
        outs.append(G.emul_gather_rows(sub))
    if not outs:
        return dict(pe5=np.zeros((0, 60), F32), wagg=np.zeros((0,), F32), ext=np.zeros((0, 4), F32))
    return {k: np.concatenate([o[k] for o in outs]) for k in ("pe5", "wagg", "ext")}


def emul_chain(case):
    """The same in float32: emul_gather_rows, float32 matrix products, float32 sums in row order."""
    n, pid, s = case["n_valid"], case["row_pid"], case["row_s"]
    g = _emul_rows(case)
    sl = F32(SLOPE)
    lk = lambda x: np.where(x > 0, x, x * sl).astype(F32)
    ext = np.concatenate([case["color"][pid], g["ext"]], 1).astype(F32)
    H1 = lk(g["pe5"] @ case["w10"][:, 224:284].T + case["b10"] + case["table"][pid])
    H2 = lk(H1 @ case["w12"].T + case["b12"])
    H3 = lk(np.concatenate([H2, ext], 1) @ case["w30"].T + case["b30"])
    H4 = lk(H3 @ case["w32"].T + case["b32"])
    alpha = (H4 @ case["aw"] + case["ab"][0]).astype(F32)
    X5, sigma = np.zeros((n, 256), F32), np.zeros((n,), F32)
    np.add.at(X5, s, H4 * g["wagg"][:, None])
    np.add.at(sigma, s, g["wagg"] * _softplus_m1(alpha).astype(F32))
    return dict(H1=H1, H2=H2, H3=H3, H4=H4, alpha=alpha, X5=X5, sigma=sigma)


def rel(a, ref):
    """max |a - ref| relative to the largest |ref| of the same row (tests/test_chain_gpu.py's _rel); a vector: relative to the value."""
    a, ref = f64(a), f64(ref)
    if a.size == 0:
        return 0.0
    den = np.maximum(np.abs(ref).max(-1, keepdims=True), 1e-30) if ref.ndim > 1 else np.maximum(np.abs(ref), 1e-30)
    return float((np.abs(a - ref) / den).max())


@functools.lru_cache(maxsize=None)
def base_refs(n_big, n_small, n_tiny, seed, wide):
    """(one-class case, float64 reference, e32 per stage) of a set of samples: computed once, never written."""
    spec = (n_big, n_small, n_tiny, n_big + n_small + n_tiny, 0) + ((True,) if wide else ())
    case = make_chain(spec, seed)
    r64, r32 = ref_chain(case), emul_chain(case)
    e32 = {k: rel(r32[k], r64[k]) for k in LAYERS + ("X5", "sigma")}
    return case, r64, e32


def refs(spec, seed=None):
    """(case, reference in the case's list order, e32) of a spec.  X5, sigma and the view-direction columns per listed sample; the rows' weight / confc
    per (item, slot) as `weight_at` / `confc_at` [items, 8] with the bound in `weight_bound_at` (valid at the listed slots only)."""
    seed = seed_of(spec) if seed is None else seed
    case = make_chain(spec, seed)
    base, r64, e32 = base_refs(spec[0], spec[1], spec[2], seed, is_wide(spec))
    pos = case["pos"]
    out = dict(X5=r64["X5"][pos], sigma=r64["sigma"][pos], viewdir=(r64["viewdir"][0][pos], r64["viewdir"][1][pos]))
    if case["classes"] == 0 and case["n_valid"] == base["n_valid"]:
        out.update({k: r64[k] for k in LAYERS})
    at = {k: np.zeros((case["items"], K)) for k in ("weight_at", "weight_bound_at", "confc_at")}
    at["weight_at"][base["row_item"], base["row_k"]] = r64["weight"][0]
    at["weight_bound_at"][base["row_item"], base["row_k"]] = r64["weight"][1]
    at["confc_at"][base["row_item"], base["row_k"]] = r64["confc"]
    out.update(at)
    return case, out, e32


def bound(e32, name):
    return FACTOR * e32[name] + (FLOOR_SIGMA if name == "sigma" else FLOOR)
