"""The bounds of tests/test_backward_glue_gpu.py, checked without a GPU: for every case of that module, a float32 restatement of the kernel in its
operation order (tests/backward_glue_ref.py) must lie within the per-element bound of the float64 reference (err / bound <= 1).  A kernel that then
exceeds a bound on the device is wrong; the bound is not.  Worst ratios of the restatements: final colour 0.48 (gCF), K-sums 0.67 (gZ4), extras
0.003, rows -> points 0.99 (the one-product column of G8, whose bound is the U |x| of a single rounding) and 0.25 (the point sums), positional
encoding 0.17, conf0 0.000.  The sums over thousands of terms sit far below their worst-case bounds, here as on the device.
"""
import numpy as np
import pytest

from tests import backward_glue_ref as R


def _all(ref, emul, names):
    for k in names:
        R.check(k, emul[k], *ref[k])


@pytest.mark.parametrize("strides", R.FINAL_STRIDES)
@pytest.mark.parametrize("cap,n_valid", [c for c in R.FINAL_SHAPES if c[1] > 0])
def test_final_colour_restatement_is_within_the_bounds(cap, n_valid, strides):
    inp = R.make_final(cap, n_valid, strides, seed=cap)
    _all(R.ref_final(inp), R.emul_final(inp), ("gCF", "g_w", "g_b"))


@pytest.mark.parametrize("cap,n_valid", [c for c in R.KSUM_SHAPES if c[1] > 0])
def test_ksum_restatement_is_within_the_bounds(cap, n_valid):
    inp = R.make_ksum(cap, n_valid, seed=cap + n_valid)
    ref = R.ref_ksum(inp)
    _all(ref, R.emul_ksum(inp), ("gZ4", "g_wagg", "g_alpha_w", "g_alpha_b"))
    # the inputs reach what the case is for: both softplus branches, saturated sigmoids, signed zeros
    if n_valid >= 4:
        live = np.flatnonzero(inp["occ"].reshape(-1))
        h = inp["H4"][live]
        y = h.astype(np.float64) @ inp["alpha_w"].astype(np.float64) + float(inp["alpha_b"][0]) - 1
        assert y.max() > 20 and y.min() < -20
        assert ((h == 0) & ~np.signbit(h)).any() and ((h == 0) & np.signbit(h)).any()


@pytest.mark.parametrize("rows_cap,M", [c for c in R.EXTRAS_SHAPES if c[1] > 0])
def test_extras_restatement_is_within_the_bounds(rows_cap, M):
    inp = R.make_extras(rows_cap, M, seed=M)
    _all(R.ref_extras(inp), R.emul_extras(inp), ("gX3",))


@pytest.mark.parametrize("with_conf", [False, True])
@pytest.mark.parametrize("n_valid", [n for n in R.GATHER_N if n > 0])
def test_rows_to_points_restatement_is_within_the_bounds(n_valid, with_conf):
    inp = R.make_gather(n_valid, seed=n_valid)
    _all(R.ref_gather(inp, with_conf), R.emul_gather(inp, with_conf), ("G8", "points"))


@pytest.mark.parametrize("use_ids", [False, True])
@pytest.mark.parametrize("n", [n for n in R.POINT_ROWS_N if n > 0])
def test_point_rows_restatement_is_within_the_bounds(n, use_ids):
    inp = R.make_point_rows(n, use_ids, True, 232, seed=n)
    _all(R.ref_point_rows(inp), R.emul_point_rows(inp), ("g_emb",))


@pytest.mark.parametrize("n", R.CONF0_N)
def test_conf0_restatement_is_within_the_bounds(n):
    inp = R.make_conf0(n, seed=n)
    _all(R.ref_conf0(inp), R.emul_conf0(inp), ("g_conf0",))


def test_integer_restatements():
    ul, cn, uidx = R.ref_unique(np.array([3, -1, 5, 3, 9, 2], np.int32), 4, 10)
    assert ul.tolist() == [3, 5] and cn.tolist() == [2, 1] and uidx.tolist() == [-1, -1, -1, 0, -1, 1, -1, -1, -1, -1]
    mask = np.array([1, 0, 1, 1, -1, 1], np.int8)
    lut = np.array([0, 1, 1, 0, 1, 1], np.uint8)
    assert R.ref_ray_drop(mask, lut, None).tolist() == [0, 0, 1, 1, 0, 0]
    assert R.ref_ray_drop(mask, None, np.array([1, 1, 0, 2, 1, 1], np.uint8)).tolist() == [1, 0, 0, 1, 0, 1]
