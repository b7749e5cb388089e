"""tests/chain_ref.py without a GPU: the float64 reference of the fused chain against torch.nn.Linear modules in float64 (the wiring: which columns of
block1.0 form the per-point table, the order of block3's extras, the K-sums), the float32 restatement against the reference on every shape of the lists
(C = 8 workgroups), the condition on e32 that keeps the device's bound honest, and the case builder's invariants."""
import numpy as np
import pytest
import torch

from tests import chain_ref as R
from tests import forward_glue_ref as G

C = 8
SPECS = R.all_specs(C)
_id = lambda spec: "-".join(str(int(x)) for x in spec)


def test_lists_hold_the_shapes_they_are_meant_to():
    assert R.TILE_N == [1, 15, 16, 17, 127, 128, 129]
    assert R.grid_n(C) == [127, 128, 129, 273, 257] and R.cap_cases(C) == [(1, 128), (17, 133), (147, 512), (0, 64)]
    cc = R.class_cases(C)
    assert cc[0] == (5, 6, 5, 16) and cc[6] == (113, 8, 7, 128) and cc[7] == (129, 257, 513, 899) and (0, 1, 0, 1) in cc and (0, 0, 1, 1) in cc and (0, 0, 130, 130) in cc
    b, s, t, cap = cc[-1]
    assert b < cap < b + s                                            # the capacity cuts the list inside the small class
    assert len(set(SPECS)) == len(SPECS) and set(R.one(n) for n in R.TILE_N + R.grid_n(C)) <= set(SPECS) and set(R.WIDE_SPECS) <= set(SPECS)


def test_reference_equals_linear_modules_in_float64():
    case = R.make_chain(R.one(17))
    ref = R.ref_chain(case, table=case["table64"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    act = torch.nn.LeakyReLU(R.SLOPE)
    block1 = torch.nn.Sequential(torch.nn.Linear(284, 256), act, torch.nn.Linear(256, 256), act).double()
    block3 = torch.nn.Sequential(torch.nn.Linear(263, 256), act, torch.nn.Linear(256, 256), act).double()
    alpha_branch = torch.nn.Sequential(torch.nn.Linear(256, 1)).double()
    with torch.no_grad():
        for seq, i, w, b in ((block1, 0, "w10", "b10"), (block1, 2, "w12", "b12"), (block3, 0, "w30", "b30"), (block3, 2, "w32", "b32")):
            seq[i].weight.copy_(t(case[w])); seq[i].bias.copy_(t(case[b]))
        alpha_branch[0].weight.copy_(t(case["aw"]).reshape(1, 256)); alpha_branch[0].bias.copy_(t(case["ab"]))
        pid = case["row_pid"]
        emb = case["emb"][pid]
        x1 = torch.cat([t(emb), t(G.pe64(emb, 3)[0]), t(ref["pe5"][0])], 1)                 # [emb 32 | PE3(emb) 192 | PE5(dists6) 60]
        assert x1.shape[1] == 284
        h1 = act(block1[0](x1))
        h2 = block1(x1)
        x3 = torch.cat([h2, t(case["color"][pid]), t(G.ref_gather_rows(case)["ext"][0])], 1)   # [H2 | colour 3 | dir - v 3 | dir . v 1]
        h3 = act(block3[0](x3))
        h4 = block3(x3)
        alpha = alpha_branch(h4)[:, 0]
        sp = torch.nn.functional.softplus(alpha - 1.0)
        wagg = t(ref["wagg"][0])
        seg = torch.from_numpy(case["row_s"])
        X5 = torch.zeros((17, 256), dtype=torch.float64).index_add_(0, seg, h4 * wagg[:, None])
        sigma = torch.zeros((17,), dtype=torch.float64).index_add_(0, seg, sp * wagg)
    for name, got in (("H1", h1), ("H2", h2), ("H3", h3), ("H4", h4), ("alpha", alpha), ("X5", X5), ("sigma", sigma)):
        e = R.rel(ref[name], got.numpy())
        print("%-6s %.2e" % (name, e))
        assert e <= 1e-12, (name, e)
    # the table is rounded once, and that rounding is all that separates the two tables
    assert np.array_equal(case["table"], case["table64"].astype(np.float32)) and R.rel(R.ref_chain(case)["H1"], ref["H1"]) < 2e-7
    # the logits reach both branches of softplus(y > 20) and its far negative side
    a = R.base_refs(129, 257, 513, R.seed_of((129, 257, 513)), False)[1]["alpha"]
    assert a.min() < -20 and a.max() > 25 and ((a - 1 > 20).mean() > 0.02) and ((a - 1 < 20).mean() > 0.5), (a.min(), a.max())


@pytest.mark.parametrize("spec", SPECS, ids=_id)
def test_float32_restatement_is_inside_the_device_bound_and_e32_is_small(spec):
    case, ref, e32 = R.refs(spec)
    print("e32: " + "  ".join("%s %.2e" % (k, v) for k, v in e32.items()))
    # the condition that keeps the bound honest
    for k in R.LAYERS + ("X5",):
        assert e32[k] <= R.E32_LIMIT, (k, e32[k])
    # the restatement on the case's OWN list (class order, cut at the capacity) against the reference re-ordered from the one-class list
    r32 = R.emul_chain(case)
    for k in ("X5", "sigma"):
        e = R.rel(r32[k], ref[k])
        print("%-6s %.2e of bound %.2e" % (k, e, R.bound(e32, k)))
        assert e <= R.bound(e32, k), (k, e, e32[k])
    if "H1" in ref:
        for k in R.LAYERS:
            assert R.rel(r32[k], ref[k]) <= R.bound(e32, k)
    assert not np.isnan(r32["X5"]).any() and not np.isnan(r32["sigma"]).any()


@pytest.mark.parametrize("spec", SPECS, ids=_id)
def test_case_invariants(spec):
    c = R.make_chain(spec)
    n_big, n_small, n_tiny, cap, classes = spec[:5]
    n, total, items = c["n_valid"], c["total"], c["items"]
    assert n == min(total, cap) and total == n_big + n_small + n_tiny and items == c["R"] * R.SR
    cnt = c["counts"]
    assert cnt[R.CNT_VALID] == total and cnt[G.CNT_SAMPLES] == items
    n_s, n_t = int(cnt[R.CNT_SMALL]), int(cnt[R.CNT_TINY])
    n_b = n - n_s - n_t
    assert 0 <= n_b and n_s + n_t <= n <= cap                        # every count <= the capacity
    assert c["vs_item"].shape == (max(cap, 1) + 3,) and c["vs_item"].min() >= 0 and c["vs_item"].max() < items
    assert c["pidx"].min() >= -1 and c["pidx"].max() < R.N_POINTS and c["raydir"].shape == (c["R"], 3)
    nb = (c["pidx"][c["vs_item"][:n]] >= 0).sum(1)
    assert np.array_equal(nb, c["vs_cnt"]) and nb.min(initial=1) >= 1
    assert ((c["pidx"][c["vs_item"][:n]] >= 0) == (np.arange(8)[None, :] < nb[:, None])).all()      # valid ids are a prefix of the slots
    # class membership as hnr_chain_plan(classes) decides it; ascending items inside a class
    want = G.chain_class(nb, classes)
    assert np.array_equal(want, np.r_[np.full(n_b, 1), np.full(n_s, 2), np.full(n_t, 3)])
    for lo, hi in ((0, n_b), (n_b, n_b + n_s), (n_b + n_s, n)):
        assert (np.diff(c["vs_item"][lo:hi]) > 0).all()
    if cap >= total:                                                  # every value the class allows
        for k, allowed in ((1, range(1, 9) if n_small + n_tiny == 0 else range(5, 9)), (2, range(3, 5) if classes == 2 else range(1, 5)), (3, range(1, 3))):
            have = set(nb[want == k].tolist())
            m = int((want == k).sum())
            assert have <= set(allowed) and (m < 8 or (classes == 1 and k == 2 and (n_small == 0 or n_tiny == 0)) or have == set(allowed)), (k, have)
    # the one-class list of the same samples holds them in ascending order, and `pos` finds every listed sample there
    base = R.make_chain(R.one_class_of(spec))
    assert (np.diff(base["vs_item"][:total]) > 0).all() and np.array_equal(base["vs_item"][c["pos"]], c["vs_item"][:n])
    # poison: beyond the count the list names items that are not listed, whose positions are NaN and whose eight slots are all valid ids
    past = c["vs_item"][n:]
    assert not np.isin(past, base["vs_item"][:total]).any() and np.isnan(c["loc_w"][past]).all() and (c["pidx"][past] >= 0).all()
    assert not np.isnan(c["loc_w"][c["vs_item"][:n]]).any()
    if total:
        rows = c["pidx"][base["vs_item"][:total]]
        assert rows[0, 0] == 0 and (rows == R.N_POINTS - 1).any()
        first = base["vs_item"][0]
        assert np.array_equal(c["loc_w"][first], c["xyz"][0])        # norm 0
    if total >= 8:
        assert np.array_equal(c["pidx"][base["vs_item"][:8], 0], np.arange(8))              # the confidences on and around both clamps
        assert c["conf"][1] == np.float32(1e-4) and c["conf"][3] == 1.0 and c["conf"][0] < 1e-4 and c["conf"][4] > 1
    if total >= 16:
        first_tile = c["pidx"][c["vs_item"][:min(n, 16)]]
        ids = first_tile[first_tile >= 0]
        assert ids.size > np.unique(ids).size or n < 4                # ids repeat within a tile
    assert np.isfinite(c["table"]).all() and c["table"].shape == (R.N_POINTS, 256)
