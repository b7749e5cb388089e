"""The small kernels between the heavy stages of hnr_render_train_backward, each alone through its STAGE entry point (include/hnr.h) with the grid the
step gives it, against float64 (tests/backward_glue_ref.py: references, per-element bounds derived from the kernels' operation counts, and the float32
restatements that tests/test_backward_glue.py holds to the same bounds without a GPU).  Inputs are synthetic: no scene, no fixture, no fused step.

Every test follows one pattern: input rows beyond the device-side count hold NaN (a read past the count poisons the result), outputs carry spare
rows / columns of a sentinel that must come back bit-unchanged, every index is in range and every device count <= the capacity passed.

 a. hnr_final_color_bwd / _max    autograd of sum g_rgb . (1.002 sigmoid(w x + b) - 0.001); logits to +-30; two samples per wave at cap 9000
 b. hnr_ksum_bwd_rows8            softplus / sigmoid at y in -30 .. 30, +-0 in H4, holes in the 8 slots, a partly filled 32-row group, two samples per wave
 c. hnr_extras_dgrad              M around the 16-row block, the stride loop at 33 000 rows
 d. hnr_gather_rows_bwd_rows -> hnr_segment_sum_rows_csr -> hnr_point_small_grads   G8 by its formula, then float64 index_add over a 300-point cloud
 e. hnr_point_rows_bwd            E from hnr_point_rows on the device; ids / no ids, device count / none, lde 224 / 232
 f. hnr_dleaky_add, g. hnr_sum_views   bit for bit against the float32 torch expression; both column-index branches, the stride loops
 h. hnr_unique_points             against numpy.unique, n_points around the 1024-point scan block, a list capacity below the number of touched points
 i. hnr_conf0_grad, hnr_w0fd_grad, hnr_ray_drop_flags

Worst err / bound per tensor on an MI355X (all shapes of a test together; 1 is the limit; 145 cases, 984 bit-for-bit comparisons with 0 differences):
  a. gCF 0.484, g_w_fin 0.177, g_b_fin 0.124        b. gZ4 0.672, g_wagg 0.005, g_alpha_w 0.032, g_alpha_b 0.008        c. gX3[:, 256:263] 0.003
  d. G8 0.985 (its one-product column has the bound U |x| of a single rounding), g_color | g_dir | g_conf 0.246
  e. E of the forward 0.249 (of sincosf's 4 ulp), g_emb 0.171        i. g_conf[0] 0.000
The float32 restatements reach the same figures on the CPU (tests/test_backward_glue.py), so no bound was widened.

Wrong kernels the module was seen to catch (scratch builds of the library, one change each, all of them changing values only):
  a. column 44 of Y left out of x; the second trip of the sample loop dropped (cap 9000 only); the maximum published one exponent low
  b. lane 8 k + 3 read for 8 k + 4; `h >= 0` for `h > 0` (the signed zeros); the second trip dropped (cap 8208 only)
  c. the stride loop's second trip one row late (33 000 rows only); the last butterfly step of the 16-lane sum left out
  d. raydir.z for raydir.y in G8; two direction columns swapped in hnr_point_small_grads
  e. the sin and cos terms swapped        f. one `c + 1 < n_add` guard dropped (the 45-column addends only)        g. the first of 8 views skipped
  h. the closing entry of seg_start without the last point's rows        i. `pidx <= 0` for `< 0`; column k + 127 for k + 128; the ray-drop
  block's base one short after a valid 1024th ray (R > 1024 only)
"""
import ctypes

import numpy as np
import pytest
import torch

from hybridneuralrendering_amd import _lib
from tests import backward_glue_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
SENT = R.SENT
BIG_WORD = 0x7F000000                               # larger than any finite maximum here: must stay


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _h(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _sent(*shape):
    return torch.full(shape, float(SENT), dtype=torch.float32, device="cuda:0")


def _i64(v):
    return torch.tensor([v], dtype=torch.int64, device="cuda:0")


def _word(v):
    return torch.tensor([v], dtype=torch.int32, device="cuda:0")     # (bit patterns below 2^31)


def _call(name, *args):
    a = [_lib.ptr(x) if isinstance(x, torch.Tensor) else x for x in args]
    _lib.check(getattr(_lib.lib(), name)(*a, _lib.stream()), name)


def _untouched(name, a, fill=SENT):
    a = np.asarray(a)
    want = np.full(a.shape, fill, a.dtype)
    R.check_bits(name + " (spare)", a, want)


# ================================================================================================ a
def _run_final(inp, word0):
    cap, n = inp["cap"], inp["n_valid"]
    ldy, ldcf, ldgy, ldgcf = inp["strides"]
    gY, gCF, gs = _sent(cap + 3, ldgy), _sent(cap + 3, ldgcf), _sent(cap + 3)
    gw, gb = _sent(3 * 128 + 4), _sent(3 + 5)
    gw[:384] = _d(inp["g_w_pre"]).reshape(-1)
    gb[:3] = _d(inp["g_b_pre"])
    head = [_d(inp["Y"]), ldy, _d(inp["CF"]), ldcf, _d(inp["w_fin"]), _d(inp["b_fin"]), _d(inp["vs_item"]), _d(inp["counts"]), cap, _d(inp["g_decoded"]),
            gY, ldgy, gCF, ldgcf, gs, gw, gb]
    if word0 is None:
        _call("hnr_final_color_bwd", *head)
        word = None
    else:
        w = _word(word0)
        _call("hnr_final_color_bwd_max", *head, w)
        word = int(_h(w)[0])
    return _h(gY), _h(gCF), _h(gs), _h(gw), _h(gb), word


@pytest.mark.parametrize("strides", R.FINAL_STRIDES)
@pytest.mark.parametrize("cap,n_valid", R.FINAL_SHAPES)
def test_final_colour_backward(cap, n_valid, strides):
    inp = R.make_final(cap, n_valid, strides, seed=cap)
    n = n_valid
    ref = R.ref_final(inp) if n else None
    for word0 in (None, 0) + ((BIG_WORD,) if cap <= 300 else ()):
        gY, gCF, gs, gw, gb, word = _run_final(inp, word0)
        _untouched("gY rows", gY[n:])
        _untouched("gY columns", gY[:n, 45:])
        _untouched("gCF rows", gCF[n:])
        _untouched("gCF columns", gCF[:n, 128:])
        _untouched("g_sigma", gs[n:])
        _untouched("g_w_fin", gw[384:])
        _untouched("g_b_fin", gb[3:])
        if n == 0:                                                    # nothing changes anywhere
            R.check_bits("g_w_fin", gw[:384], inp["g_w_pre"].reshape(-1))
            R.check_bits("g_b_fin", gb[:3], inp["g_b_pre"])
            assert word in (None, word0)
            continue
        R.check("gCF", gCF[:n, :128], *ref["gCF"])
        R.check_bits("gY = gCF[:, :45]", gY[:n, :45], gCF[:n, :45])
        R.check_bits("g_sigma", gs[:n], inp["g_decoded"][inp["vs_item"][:n], 0])
        R.check("g_w_fin", gw[:384].reshape(3, 128), *ref["g_w"])
        R.check("g_b_fin", gb[:3], *ref["g_b"])
        if word0 is not None:
            R.check_absmax("max |gY|", word, word0, gY[:n, :45])


# ================================================================================================ b
@pytest.mark.parametrize("cap,n_valid", R.KSUM_SHAPES)
def test_ksum_backward_rows8(cap, n_valid):
    inp = R.make_ksum(cap, n_valid, seed=cap + n_valid)
    n, rows = n_valid, inp["rows"]
    ref = R.ref_ksum(inp) if n else None
    dev = [_d(inp[k]) for k in ("H4", "aux", "alpha_w", "alpha_b", "counts", "gX5")]
    gsig = _d(inp["g_sigma"])
    for word0 in (0,) + ((BIG_WORD,) if cap <= 40 else ()):
        gZ4, gwagg = _sent(rows + 8, 256), _sent(rows + 8)
        gaw, gab, w = _sent(256 + 4), _sent(1 + 3), _word(word0)
        gaw[:256] = _d(inp["g_aw_pre"])
        gab[:1] = _d(inp["g_ab_pre"])
        _call("hnr_ksum_bwd_rows8", *dev, inp["ldg5"], gsig, float(inp["slope"]), cap, gZ4, gwagg, gaw, gab, w)
        gZ4, gwagg, gaw, gab, word = _h(gZ4), _h(gwagg), _h(gaw), _h(gab), int(_h(w)[0])
        _untouched("gZ4 rows", gZ4[8 * n:])
        _untouched("g_wagg rows", gwagg[8 * n:])
        _untouched("g_alpha_w", gaw[256:])
        _untouched("g_alpha_b", gab[1:])
        if n == 0:
            R.check_bits("g_alpha_w", gaw[:256], inp["g_aw_pre"])
            R.check_bits("g_alpha_b", gab[:1], inp["g_ab_pre"])
            assert word == word0
            continue
        R.check("gZ4", gZ4[:8 * n], *ref["gZ4"])                      # (rows of empty slots: bound 0, exact zeros)
        R.check("g_wagg", gwagg[:8 * n], *ref["g_wagg"])
        R.check("g_alpha_w", gaw[:256], *ref["g_alpha_w"])
        R.check("g_alpha_b", gab[:1], *ref["g_alpha_b"])
        R.check_absmax("max |gZ4|", word, word0, gZ4[:8 * n])


# ================================================================================================ c
@pytest.mark.parametrize("rows_cap,M", R.EXTRAS_SHAPES)
def test_extras_dgrad(rows_cap, M):
    inp = R.make_extras(rows_cap, M, seed=M)
    gX3 = _sent(rows_cap + 4, 264)
    _call("hnr_extras_dgrad", _d(inp["dZ3"]), _d(inp["w30"]), _i64(M), rows_cap, gX3)
    gX3 = _h(gX3)
    _untouched("gX3 columns 0..255", gX3[:, :256])
    _untouched("gX3 rows", gX3[M:])
    if M:
        R.check("gX3[:, 256:263]", gX3[:M, 256:263], *R.ref_extras(inp)["gX3"])
        R.check_bits("gX3[:, 263]", gX3[:M, 263], np.zeros((M,), F32))


# ================================================================================================ d
@pytest.mark.parametrize("n_valid", R.GATHER_N)
def test_rows_to_points(n_valid):
    inp = R.make_gather(n_valid, seed=n_valid)
    rows, cap, P = inp["rows"], inp["cap"], inp["n_points"]
    live = inp["live"]
    dead = np.setdiff1d(np.arange(rows + 4), live)
    head = [_d(inp[k]) for k in ("pidx", "raydir", "vs_item", "vs_off", "vs_cnt", "counts")]
    gX3, gwagg, weight, gco = _d(inp["gX3"]), _d(inp["g_wagg"]), _d(inp["weight"]), _d(inp["g_conf_out"])
    for with_conf in (False, True):
        ref = R.ref_gather(inp, with_conf)
        G8 = _sent(rows + 4, 8)
        _call("hnr_gather_rows_bwd_rows", *head, inp["SR"], inp["K"], cap, gX3, 264, gwagg, weight, gco if with_conf else None, G8)
        g8 = _h(G8)
        _untouched("G8 rows without a neighbour", g8[dead])
        R.check("G8", g8[live], *ref["G8"])                           # (columns 0..2 and 7: bound 0, exact)
    # the composed result (with d conf_coefficient): rows -> point-major lists -> per-point sums -> the point buffers
    uidx, ulist, row_u, count = torch.zeros(P, dtype=torch.int32, device="cuda:0"), _d(np.full(P + 1, -3, np.int32)), _d(np.full(rows, -3, np.int32)), _word(-3)
    scratch = torch.zeros(int(_lib.lib().hnr_unique_points_scratch_elems(P)), dtype=torch.int32, device="cuda:0")
    seg_start, seg_cnt, row_list = _d(np.full(P + 1, -3, np.int32)), _d(np.full(P, -3, np.int32)), _d(np.full(rows, -3, np.int32))
    _call("hnr_unique_points", _d(inp["row_pid"]), rows, _i64(8 * n_valid), P, uidx, ulist, P, row_u, count, scratch, seg_start, seg_cnt, row_list)
    n_u = int(_h(count)[0])
    assert n_u == int(ref["touched"].sum())
    P8 = _sent(P + 2, 8)
    _call("hnr_segment_sum_rows_csr", G8, 8, row_list, seg_start, seg_cnt, 8, n_u, P8, 8, None, 0, 0, None, 0, None)
    g_conf, g_dir, g_color = _sent(P + 3), _sent(P + 3, 3), _sent(P + 3, 3)
    g_conf[:P], g_dir[:P], g_color[:P] = _d(inp["g_conf_pre"]), _d(inp["g_dir_pre"]), _d(inp["g_color_pre"])
    _call("hnr_point_small_grads", P8, ulist, P, _i64(n_u), g_conf, g_dir, g_color)
    _untouched("P8 rows", _h(P8)[n_u:])
    g_conf, g_dir, g_color = _h(g_conf), _h(g_dir), _h(g_color)
    for nm, a in (("g_conf", g_conf), ("g_dir", g_dir), ("g_color", g_color)):
        _untouched(nm, a[P:])
    got = np.concatenate([g_color[:P], g_dir[:P], g_conf[:P, None]], 1)
    pre = np.concatenate([inp["g_color_pre"], inp["g_dir_pre"], inp["g_conf_pre"][:, None]], 1)
    t = ref["touched"]
    R.check_bits("untouched points", got[~t], pre[~t])
    if t.any():
        R.check("g_color | g_dir | g_conf", got[t], ref["points"][0][t], ref["points"][1][t])


# ================================================================================================ e
@pytest.mark.parametrize("ld", [224, 232])
@pytest.mark.parametrize("use_dn", [False, True])
@pytest.mark.parametrize("use_ids", [False, True])
@pytest.mark.parametrize("n", R.POINT_ROWS_N)
def test_point_rows_backward(n, use_ids, use_dn, ld):
    inp = R.make_point_rows(n, use_ids, use_dn, ld, seed=n)
    n_cap, P = inp["n_cap"], inp["n_points"]
    emb = _d(inp["emb"])
    ids = _d(inp["ids"]) if use_ids and n_cap else None
    E = torch.full((max(n_cap, 1), ld), float("nan"), dtype=torch.float32, device="cuda:0")
    _call("hnr_point_rows", emb, ids, n, 32, E, ld)                   # the forward's own sin / cos; rows n.. stay NaN
    g_emb = _sent(P + 2, 32)
    g_emb[:P] = _d(inp["g_emb_pre"])
    _call("hnr_point_rows_bwd", _d(inp["gE"]), ld, E, ld, ids, n_cap, _i64(n) if use_dn else None, g_emb)
    g_emb = _h(g_emb)
    _untouched("g_emb rows", g_emb[P:])
    ref = R.ref_point_rows(inp) if n else dict(rows=np.zeros((0,), np.int64))
    rest = np.setdiff1d(np.arange(P), ref["rows"])
    R.check_bits("points not listed", g_emb[rest], inp["g_emb_pre"][rest])
    if n:
        e = _h(E)[:n, :224].astype(np.float64)
        e64 = R.point_rows_e64(torch.tensor(inp["emb"][ref["rows"]], dtype=torch.float64)).numpy()
        R.check("E (forward)", e, e64, np.where(np.arange(224) < 32, 0.0, 8 * R.U * np.abs(e64) + 2.0 ** -149))      # copies exact, sincosf 4 ulp
        R.check("g_emb", g_emb[ref["rows"]], *ref["g_emb"])


# ================================================================================================ f
def _m_cases():
    return [(8, 0), (8, 1), (8, 7), (8300, 8200), (8, None)]          # (M_cap, *d_m); None: no device count.  8300 rows of 128: 1038 blocks > the 1024 of the grid


@pytest.mark.parametrize("M_cap,m", _m_cases())
@pytest.mark.parametrize("N,n_add,lda", [(128, 128, 128), (128, 45, 92), (128, None, 0), (48, 45, 48)])       # (48: 256 % 12 != 0, the branch that divides per element)
def test_dleaky_add(N, n_add, lda, M_cap, m):
    rng = np.random.default_rng(N + (n_add or 0) + M_cap)
    M = M_cap if m is None else m
    ldg, ldy, slope = N + 4, N + 8, F32(0.01)
    g0 = np.full((M_cap + 2, ldg), SENT, F32)
    g0[:M_cap, :N] = rng.standard_normal((M_cap, N)).astype(F32) * np.where(rng.random((M_cap, 1)) < 0.3, 1e-3, 1.0).astype(F32)
    y = np.full((M_cap, ldy), np.nan, F32)
    y[:M, :N] = rng.standard_normal((M, N)).astype(F32)
    z = rng.random((M, N))
    y[:M, :N][z < 0.05] = 0.0
    y[:M, :N][z > 0.95] = -0.0
    add = None
    if n_add is not None:
        add = np.full((M_cap, lda), np.nan, F32)                      # NaN beyond the n_add columns and the counted rows
        add[:M, :n_add] = rng.standard_normal((M, n_add)).astype(F32)
    for word0 in (0, BIG_WORD, None):
        g, w = _d(g0), (_word(word0) if word0 is not None else None)
        _call("hnr_dleaky_add", g, ldg, _d(add) if add is not None else None, lda, n_add or 0, _d(y), ldy, M_cap, _i64(m) if m is not None else None, N,
              float(slope), w)
        g = _h(g)
        R.check_bits("rows past the count, spare columns", np.concatenate([g[M:].reshape(-1), g[:M, N:].reshape(-1)]),
                     np.concatenate([g0[M:].reshape(-1), g0[:M, N:].reshape(-1)]))
        tg = torch.from_numpy(g0[:M, :N].copy())
        if add is not None:
            ta = torch.zeros(M, N)
            ta[:, :n_add] = torch.from_numpy(add[:M, :n_add].copy())
            tg = tg + ta
        want = torch.where(torch.from_numpy(y[:M, :N].copy()) > 0, tg, tg * float(slope)).numpy()
        R.check_bits("g", g[:M, :N], want)
        if word0 is not None:
            R.check_absmax("max |g|", int(_h(w)[0]), word0, g[:M, :N])


# ================================================================================================ g
@pytest.mark.parametrize("cap,n", [(20, 20), (20, 0), (17000, 16999)])                     # 17 000 rows of 64: 1063 blocks > 1024
@pytest.mark.parametrize("N", [64, 48])
@pytest.mark.parametrize("V", [1, 3, 4, 8])
def test_sum_views(V, N, cap, n):
    rng = np.random.default_rng(V + N + cap)
    ldi, ldo = N + 4, N + 8
    x = np.full((V, cap, ldi), np.nan, F32)
    x[:, :n, :N] = rng.standard_normal((V, n, N)).astype(F32) * np.where(rng.random((V, n, 1)) < 0.3, 1e-3, 1.0).astype(F32)
    want = torch.zeros(n, N)
    for v in range(V):
        want = want + torch.from_numpy(x[v, :n, :N].copy())
    for word0 in (0, BIG_WORD, None) if cap <= 20 else (0,):
        out, w = _sent(cap + 2, ldo), (_word(word0) if word0 is not None else None)
        _call("hnr_sum_views", _d(x), ldi, V, cap, _i64(n), N, out, ldo, w)
        out = _h(out)
        _untouched("out rows", out[n:])
        _untouched("out columns", out[:n, N:])
        R.check_bits("out", out[:n, :N], want.numpy())
        if word0 is not None:
            R.check_absmax("max |out|", int(_h(w)[0]), word0, out[:n, :N])
    if cap <= 20:                                                     # no device count: the capacity is the count
        out = _sent(cap + 2, ldo)
        _call("hnr_sum_views", _d(np.nan_to_num(x)), ldi, V, cap, None, N, out, ldo, None)
        R.check_bits("out (no count)", _h(out)[:n, :N], want.numpy())


# ================================================================================================ h
@pytest.mark.parametrize("M_cap", [8, 4096])
@pytest.mark.parametrize("n_points,cap", [(1, 1), (1023, 1023), (1024, 1024), (1025, 1025), (5000, 5000), (1025, 100)])
def test_unique_points(n_points, cap, M_cap):
    rng = np.random.default_rng(n_points + M_cap + cap)
    m = M_cap - 3
    row_pid = np.where(rng.random(M_cap) < 0.3, -1, rng.integers(0, n_points, M_cap)).astype(np.int32)       # rows m.. hold ids that must not count
    S = np.int32(-3)
    uidx, ulist, row_u, count = _d(np.full(n_points + 2, S)), _d(np.full(cap + 2, S)), _d(np.full(M_cap + 2, S)), _d(np.full(2, S))
    scratch = _d(np.full(int(_lib.lib().hnr_unique_points_scratch_elems(n_points)) + 2, S))
    seg_start, seg_cnt, row_list = _d(np.full(cap + 3, S)), _d(np.full(cap + 2, S)), _d(np.full(M_cap + 2, S))
    _call("hnr_unique_points", _d(row_pid), M_cap, _i64(m), n_points, uidx, ulist, cap, row_u, count, scratch, seg_start, seg_cnt, row_list)
    uidx, ulist, row_u, count, scratch, seg_start, seg_cnt, row_list = [_h(t) for t in (uidx, ulist, row_u, count, scratch, seg_start, seg_cnt, row_list)]
    ul, cn, ux = R.ref_unique(row_pid, m, n_points)
    n_u, k = ul.size, min(ul.size, cap)
    if (n_points, cap) == (1025, 100) and M_cap == 4096:
        assert n_u > cap                                              # the case is the one it is meant to be
    assert count[0] == n_u and count[1] == S
    R.check_bits("uidx", uidx, np.concatenate([ux, [S, S]]).astype(np.int32))
    R.check_bits("ulist", ulist, np.concatenate([ul[:k], np.full(cap + 2 - k, S)]).astype(np.int32))             # ascending; nothing past the capacity
    start = np.concatenate([[0], np.cumsum(cn)]).astype(np.int32)                                               # exclusive prefix + the closing entry
    n_start = n_u + 1 if n_u <= cap else cap
    R.check_bits("seg_start", seg_start, np.concatenate([start[:n_start], np.full(cap + 3 - n_start, S)]).astype(np.int32))
    R.check_bits("seg_cnt", seg_cnt, np.concatenate([cn[:k], np.zeros(cap - k), [S, S]]).astype(np.int32))
    counted = (np.arange(M_cap) < m) & (row_pid >= 0)
    R.check_bits("row_u", row_u, np.concatenate([np.where(counted, ux[np.maximum(row_pid, 0)], cap), [S, S]]).astype(np.int32))
    listed = int(start[k])
    _untouched("row_list past the segments", row_list[listed:], S)
    for u in range(k):
        seg = row_list[start[u]:start[u + 1]]
        want = np.flatnonzero(counted & (row_pid == ul[u]))
        assert seg.size == want.size and np.array_equal(np.sort(seg), want), (u, seg, want)
    _untouched("scratch", scratch[-2:], S)


# ================================================================================================ i
@pytest.mark.parametrize("n", R.CONF0_N)
def test_conf0_grad(n):
    inp = R.make_conf0(n, seed=n)
    g, pidx = _d(inp["g"]), _d(inp["pidx"])
    runs = []
    for _ in range(2):
        g_conf, scratch = _d(inp["g_conf_pre"]), _sent(512 + 2)
        _call("hnr_conf0_grad", g, pidx, n, scratch, g_conf)
        runs.append(_h(g_conf))
        _untouched("scratch", _h(scratch)[512:])
    R.check_bits("two runs", runs[0], runs[1])
    R.check_bits("g_conf[1:]", runs[0][1:], inp["g_conf_pre"][1:])
    R.check("g_conf[0]", runs[0][:1], *R.ref_conf0(inp)["g_conf0"])


def test_w0fd_grad():
    rng = np.random.default_rng(3)
    g = rng.standard_normal((64, 48)).astype(F32)
    gw0 = _sent(64 * 176 + 5)
    _call("hnr_w0fd_grad", _d(g), gw0)
    gw0 = _h(gw0)
    _untouched("past the matrix", gw0[64 * 176:])
    gw0 = gw0[:64 * 176].reshape(64, 176)
    R.check_bits("columns 0..44", gw0[:, :45], g[:, :45])
    R.check_bits("columns 173..175", gw0[:, 173:], g[:, 45:])
    _untouched("columns 45..172", gw0[:, 45:173])


@pytest.mark.parametrize("R_", [1, 63, 64, 1023, 1024, 1025, 3136])
def test_ray_drop_flags(R_):
    rng = np.random.default_rng(R_)
    mask = rng.integers(-1, 2, R_).astype(np.int8)
    lut = rng.integers(0, 2, R_).astype(np.uint8)                     # indexed by valid-ray row: never past the number of valid rays <= R
    explicit = rng.integers(0, 3, R_).astype(np.uint8)
    for l, e, want in ((lut, None, R.ref_ray_drop(mask, lut, None)), (lut, explicit, R.ref_ray_drop(mask, None, explicit)),
                       (None, None, np.zeros(R_, np.uint8))):
        out = _d(np.full(R_ + 3, 0x5A, np.uint8))
        _call("hnr_ray_drop_flags", _d(mask), R_, _d(l) if l is not None else None, _d(e) if e is not None else None, out)
        R.check_bits("flags", _h(out), np.concatenate([want, np.full(3, 0x5A, np.uint8)]))
