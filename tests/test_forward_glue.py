"""The bounds and index references of tests/test_forward_glue_gpu.py, checked without a GPU: for every case of that module a float32 restatement of the
kernel in its operation order (tests/forward_glue_ref.py) must lie within the per-element bound of the float64 reference (err / bound <= 1, printed per
tensor), and the index-only references (sample plan, chain plan, the probe's argmax) must equal brute-force loops.  A kernel that then exceeds a bound
on the device is wrong; the bound is not.  The tests also assert that the inputs reach what each case is for (both softplus branches, logits to +-30,
both sides of every threshold).  Worst ratios of the restatements: row gather 0.24 (PE3), 0.92 (PE5 of the distances: the cancelling perspective
columns through 2^4), 1.00 (the direction differences, whose bound is the U |x| of a single rounding), 0.28 / 0.29 (wagg, weights); K-sums 0.59,
view direction 0.22, sigma 0.005; final colour 0.85; composite 0.37 (opacity), 0.34 (blend weight), 0.27 (T), 0.23 (colour); ray march 0.49; probe
0.46 (distance), 0.28 (sums); xyz_pers 0.27.  The sums over hundreds of terms sit far below their worst-case bounds, here as on the device.
"""
import numpy as np
import pytest

from tests import forward_glue_ref as R

F32 = np.float32


@pytest.mark.parametrize("K", [8, 12])
@pytest.mark.parametrize("n_items", R.PLAN_ITEMS)
def test_plan_references_equal_the_loops(n_items, K):
    inp = R.make_plan(n_items, K, seed=n_items + K)
    assert inp["n_items"] < inp["max_items"] and set(inp["work"][:n_items]) < set(range(inp["max_items"]))
    for got, want in zip(R.ref_plan(inp), R.loop_plan(inp)):
        R.check_bits("plan", got, want)
    item, off, cnt = R.ref_plan(inp)
    assert item.size == inp["n_valid"] and int(cnt.sum()) == inp["n_rows"]
    if n_items > 8:
        assert (inp["pidx"][inp["work"][:n_items], 0] < 0).any()     # items without a neighbour
    for classes in (0, 1, 2):
        a, b = R.ref_chain_plan(inp, classes), R.loop_chain_plan(inp, classes)
        R.check_bits("chain plan", a[0], b[0])
        assert a[1:] == b[1:]
    R.check_bits("classes = 0", R.ref_chain_plan(inp, 0)[0], item)
    # the capacities one short: the last entry does not fit, the others do
    if item.size:
        assert R.plan_fits(off, cnt, item.size - 1, inp["n_rows"]).sum() == item.size - 1
        assert R.plan_fits(off, cnt, item.size, inp["n_rows"] - 1).sum() == item.size - 1


@pytest.mark.parametrize("K", R.GATHER_K)
@pytest.mark.parametrize("n_valid", R.GATHER_N)
def test_gather_rows_restatement_is_within_the_bounds(n_valid, K):
    inp = R.make_gather_rows(n_valid, K, seed=n_valid + K)
    ref, em = R.ref_gather_rows(inp), R.emul_gather_rows(inp)
    for k in ("pe3", "pe5", "wagg", "weight", "ext"):
        R.check(k, em[k], *ref[k])
    if n_valid >= K:
        assert set(inp["vs_cnt"][:n_valid]) == set(range(1, K + 1))
    c = inp["conf"][inp["row_pid"]]
    if n_valid >= 31:
        assert (c < F32(1e-4)).any() and (c == F32(1e-4)).any() and ((c > F32(1e-4)) & (c < 1)).any() and (c == 1).any() and (c > 1).any()
    assert (inp["loc_w"][inp["vs_item"][0]] == inp["xyz"][inp["pidx"][inp["vs_item"][0], 0]]).all()


@pytest.mark.parametrize("twelve", [False, True])
@pytest.mark.parametrize("n_valid", R.KSUM_N)
def test_ksum_restatement_is_within_the_bounds(n_valid, twelve):
    inp = R.make_ksum(n_valid, twelve, seed=n_valid + twelve)
    ref, em = R.ref_ksum(inp), R.emul_ksum(inp)
    for k in ("sigma", "feat", "viewdir"):
        R.check(k, em[k], *ref[k])
    if n_valid >= 4:
        y = em["y"]
        assert y.max() > 20 and (y < 20).any() and (y > 20).sum() >= 2
        h = inp["H"]
        assert ((h == 0) & ~np.signbit(h)).any() and ((h == 0) & np.signbit(h)).any()
    if n_valid >= 257:
        assert y.max() > 28 and y.min() < -28


@pytest.mark.parametrize("ldy,y_off,ldcf", R.FINAL_LAYOUTS)
@pytest.mark.parametrize("cap,n_valid", R.FINAL_SHAPES[:-1] + [(300, 290)])      # (the two-trip capacity adds nothing to the arithmetic: the device test runs it)
def test_final_colour_restatement_is_within_the_bounds(cap, n_valid, ldy, y_off, ldcf):
    inp = R.make_final(cap, n_valid, ldy, ldcf, seed=cap)
    rgb, bound, z = R.ref_final(inp)
    R.check("rgb", R.emul_final(inp), rgb, bound)
    if n_valid >= 3:
        assert z[:, 0].max() > 29.9 and z[:, 0].min() < -29.9


@pytest.mark.parametrize("unit_mode", [0, 1])
@pytest.mark.parametrize("use_nsamp", [False, True])
@pytest.mark.parametrize("SR", R.COMPOSITE_SR)
@pytest.mark.parametrize("R_", R.COMPOSITE_R)
def test_composite_restatement_is_within_the_bounds(R_, SR, use_nsamp, unit_mode):
    inp = R.make_composite(R_, SR, 8, seed=R_ + SR)
    ref, em = R.ref_composite(inp, use_nsamp, unit_mode), R.emul_composite(inp, use_nsamp, unit_mode)
    for k in ("opacity", "blend", "T_end", "color"):
        R.check(k, em[k], *ref[k])
    # ray_march on the same distances
    d_f, _, _, valid = R.ray_dist(inp, use_nsamp, unit_mode)
    _, _, dec = R.padded(inp, use_nsamp)
    for bg in (None, inp["bg"]):
        rm, emr = R.ref_march(R.f64(d_f), 0.0, valid, dec, bg), R.emul_march(d_f, valid, dec, bg)
        for k in ("opacity", "T", "blend", "T_end", "color"):
            R.check("march " + k, emr[k], *rm[k])
    if R_ >= 255 and SR == 24:
        # the thresholds: exact zeros (equal / backward depths), gaps on both sides of 2 vsize_z and well clear of it, saturated and zero opacity
        z = np.maximum.accumulate(R.z32(inp["loc_w"], inp["campos"], inp["camrot"]), 1)
        d = z[:, 1:] - z[:, :-1]
        assert (d == 0).any() and ((d > 0) & (d < F32(0.035))).any() and (d > F32(0.09)).any() and not ((d > 0) & (d < F32(0.009))).any()
        assert not ((d > F32(0.035)) & (d < F32(0.09))).any()
        assert (em["opacity"] == 1).any() and (em["opacity"][inp["ray_mask"] > 0] == 0).any()
        assert (inp["ray_mask"] == 0).any() and set((0, 1, SR)) <= set(inp["nsamp"])


@pytest.mark.parametrize("R_", R.PROBE_R)
def test_probe_restatement_is_within_the_bounds(R_):
    inp = R.make_probe(R_, seed=R_)
    ref, em = R.ref_probe(inp), R.emul_probe(inp)
    R.check_bits("argmax", em["best"], ref["best"])
    for r in range(R_):                                               # the first maximum, by a loop
        best = 0
        for s in range(1, inp["SR"]):
            if inp["opacity"][r, s] > inp["opacity"][r, best]:
                best = s
        assert best == ref["best"][r]
    for k in ("far", "color", "dir", "conf", "emb"):
        R.check(k, em[k].reshape(ref[k][0].shape), *ref[k])
    o = inp["opacity"]
    assert ((o == o.max(1, keepdims=True)).sum(1) > 1).any()          # a tie
    if R_ > 2:
        assert (o[2] == 0).all() and ref["best"][2] == 0
    assert (inp["pidx"][np.arange(R_), ref["best"]] < 0).any()


@pytest.mark.parametrize("n", R.POINTS_N)
def test_gather_points_restatement_is_within_the_bounds(n):
    inp = R.make_points(n, seed=n)
    R.check("xyz_pers", R.emul_points(inp)["pers"], *R.ref_points(inp)["pers"])
    if n > 1:
        assert (inp["pidx"][:n] < 0).any()


def test_w2pers_is_the_inverse_of_the_input_maker():
    cp, cr = R.make_camera(5)
    assert np.abs(R.f64(cr).T @ R.f64(cr) - np.eye(3)).max() < 1e-6 and np.abs(cr).min() > 0.02          # a rotation, not axis-aligned
    c = np.array([[0.5, -0.25, 3.0]])
    got, _ = R.cam64(R.cam_to_world(c, cp, cr), cp, cr)
    assert np.abs(got - c).max() < 1e-5
    v, _ = R.pe64(np.array([[0.5, 2.0]]), 3)
    want = [np.sin(0.5), np.cos(0.5), np.sin(1.0), np.cos(1.0), np.sin(2.0), np.cos(2.0), np.sin(2.0), np.cos(2.0), np.sin(4.0), np.cos(4.0), np.sin(8.0), np.cos(8.0)]
    assert np.allclose(v[0], want, rtol=0, atol=1e-15)
