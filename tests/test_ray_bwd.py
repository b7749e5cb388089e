"""tests/ray_bwd_ref.py without a GPU: the closed-form references against float64 autograd, the float32 restatements of hnr_composite_bwd[_depth] and
hnr_merge_bwd against the references within the derived bounds (the bounds tests/test_ray_bwd_gpu.py holds the kernels to: a bound that plain float32
arithmetic in the kernels' order cannot meet is a mistake of the derivation), and the conditions on the inputs: the bounds of the bounded composite cases
say something, the padding position lies below every ray's running maximum, and every branch the GPU module names is reached by the inputs it names it for.

"Say something": in every (distance mode, nsamp) run of every shape, at most 10 % of the live samples' d sigma have a bound above 1e-3 |ref|.  Asserted run by run
  * for the colour objective on ray_bwd_ref.make_ray's inputs (worst run 9.6 %);
  * for colour + depth and for the depth term alone on ray_bwd_ref.make_ray_depth's inputs, whose docstring derives why the depth term needs a few
    well-separated contributing samples (worst runs 6.3 % and 4.2 %);
  * for colour + depth on make_ray's inputs too where it holds, SR < 24 (worst run 1.9 %; on the long rays of those inputs the restatement is still held to
    the bounds, and the share, up to 37 %, is printed)."""
import numpy as np
import pytest

from tests import ray_bwd_ref as R

F32 = np.float32
VARIANTS = [(True, False), (True, True), (False, True)]              # (colour, depth): colour only, both, the depth term alone


def _cases():
    return [(r, sr) for sr in R.RAY_SR for r in R.RAY_R]


def _restatement_run(inp, use_nsamp, unit_mode, colour, depth, must_say_something):
    ref = R.ref_ray_bwd(inp, use_nsamp, unit_mode, colour, depth)
    g, b = ref["g"]
    got = R.emul_ray_bwd(inp, use_nsamp, unit_mode, colour, depth)
    R.check("d sigma", got[..., 0], g[..., 0], b[..., 0])
    R.check("d rgb", got[..., 1:], g[..., 1:], b[..., 1:])
    assert np.all(got[~ref["live"]] == 0)
    loose, live = R.loose_count(g[..., 0], b, ref["live"])
    print("unit %d nsamp %d colour %d depth %d: %d live d sigma, bound above 1e-3 |ref| on %d" % (unit_mode, use_nsamp, colour, depth, live, loose))
    if must_say_something:
        assert loose <= 0.10 * live


@pytest.mark.parametrize("R_,SR", _cases())
def test_composite_backward_restatement(R_, SR):
    K, seed = R.ray_K(R_, SR), R.ray_seed(R_, SR)
    inp, inp_d = R.make_ray(R_, SR, K, seed), R.make_ray_depth(R_, SR, K, seed)
    for unit_mode, use_nsamp in R.RAY_MODES:
        _restatement_run(inp, use_nsamp, unit_mode, True, False, True)
        _restatement_run(inp, use_nsamp, unit_mode, True, True, SR < 24)
        _restatement_run(inp_d, use_nsamp, unit_mode, True, True, True)
        _restatement_run(inp_d, use_nsamp, unit_mode, False, True, True)


def test_depth_inputs_have_no_lone_contributor():
    for R_, SR in ((257, 24), (257, 80), (5, 2)):
        inp = R.make_ray_depth(R_, SR, 8, R.ray_seed(R_, SR))
        for use_nsamp in (False, True):
            _, _, _, valid = R.ray_dist(inp, use_nsamp, 1)
            n = ((inp["decoded"][..., 0] > 0) & valid).sum(1)
            assert set(np.unique(n)) <= {0, 2, 3} and (SR < 4 or (n == 3).any())
            assert np.all(n[inp["nsamp"] < 4] == 0) and (R_ < 5 or n[4] == 0)


@pytest.mark.parametrize("R_,SR", [(5, 2), (257, 24), (5, 65)])
def test_composite_backward_closed_form_is_the_autograd(R_, SR):
    inp = R.make_ray(R_, SR, 8, seed=R_ + SR)
    for unit_mode, use_nsamp in R.RAY_MODES:
        for colour, depth in VARIANTS:
            g = R.ref_ray_bwd(inp, use_nsamp, unit_mode, colour, depth)["g"][0]
            ag = R.autograd_ray_bwd(inp, use_nsamp, unit_mode, colour, depth)
            live = R.ref_ray_bwd(inp, use_nsamp, unit_mode, colour, depth)["live"]
            # (autograd's d sigma of an invalid sample is 0 as well; its d rgb of a masked ray too)
            np.testing.assert_allclose(g, np.where(live[..., None], ag, 0.0), rtol=1e-9, atol=1e-12 * max(1.0, float(np.abs(ag).max())))


def test_composite_inputs_reach_their_branches():
    inp = R.make_ray(257, 24, 8, seed=257 + 24)
    assert list(inp["nsamp"][:3]) == [0, 1, 24] and inp["ray_mask"][3] == 0 and inp["ray_mask"][4] == 1
    assert np.all(inp["decoded"][4, :, 0] == 0) and float(inp["decoded"][..., 0].max()) == R.TOP_SIGMA
    d0, _, _, valid = R.ray_dist(inp, True, 0)
    d1 = R.ray_dist(inp, True, 1)[0]
    assert (d0 > 2 * R.VSIZE_Z).any() and not (d1 > 2 * R.VSIZE_Z).any()          # the 2 vsize_z threshold decides in unit mode only
    assert (~valid[np.arange(24)[None, :] < inp["nsamp"][:, None]]).any()            # holes inside nsamp
    ref = R.ref_ray_bwd(inp, True, 1, True, True)
    assert not ref["live"][0].any() and not ref["live"][3].any() and ref["live"][4].any()
    assert np.all(ref["g"][1][~ref["live"]] == 0)                                    # exact zeros are demanded there
    sat = R.make_ray(5, 24, 8, seed=1, top=1e4)
    assert float(sat["decoded"][..., 0].max()) == 1e4


def test_composite_distance_on_the_unit_threshold():
    inp, (r, s) = R.make_ray_threshold()                              # (asserts dist = 2 vsize_z at (r, s) itself)
    for use_nsamp in (False, True):
        for colour, depth in VARIANTS:
            ref = R.ref_ray_bwd(inp, use_nsamp, 1, colour, depth)
            assert ref["live"][r, s] and ref["g"][0][r, s, 0] != 0
            got = R.emul_ray_bwd(inp, use_nsamp, 1, colour, depth)
            R.check("d sigma", got[..., 0], ref["g"][0][..., 0], ref["g"][1][..., 0])
            R.check("d rgb", got[..., 1:], ref["g"][0][..., 1:], ref["g"][1][..., 1:])


@pytest.mark.parametrize("R_", [5, 257])
def test_wave_and_serial_embedding(R_):
    a, b = R.make_ray_pair(R_, 8, seed=R_)                            # (asserts the padding depth itself)
    assert R.pad_depth(a) < 1.0 and a["SR"] == 24 and b["SR"] == 65
    for unit_mode in (0, 1):
        for colour, depth in VARIANTS:
            ga = R.emul_ray_bwd(a, True, unit_mode, colour, depth)
            gb = R.emul_ray_bwd(b, True, unit_mode, colour, depth)
            R.check_bits("SR 24 in SR 65", gb[:, :24], ga)
            assert np.all(gb[:, 24:] == 0)


def test_composite_saturation_restatement_is_finite():
    inp = R.make_ray(257, 24, 8, seed=3, top=1e4)
    for unit_mode, use_nsamp in R.RAY_MODES:
        got = R.emul_ray_bwd(inp, use_nsamp, unit_mode, True, True)
        live = R.ref_ray_bwd(inp, use_nsamp, unit_mode, True, True)["live"]
        assert np.all(np.isfinite(got)) and np.all(got[~live] == 0)


# ================================================================================================ merge
def _merge_case(V, shape, i):
    fw_mode = (None, "random", "zero")[i % 3]
    return R.make_merge(V, shape[0], shape[1], R.MERGE_STRIDES[i % 2], fw_mode, drop=bool((i // 2) % 2), seed=100 * V + shape[0])


def _check_merge(inp, got, ref):
    R.check("gF", got["gF"], *ref["gF"])
    R.check("gZ3", got["gZ3"], *ref["gZ3"])
    R.check("g_w_last", got["g_w"], *ref["g_w"])
    R.check("g_b_last", got["g_b"], *ref["g_b"])
    R.check_bits("gCF", got["gCF"], ref["gCF"])
    dead = np.broadcast_to(inp["dropped"][None, :], ref["scale"].shape) | (ref["scale"] == 0)
    assert np.all(ref["gF"][1][dead] == 0) and np.all(ref["gZ3"][1][dead] == 0)       # a bound of 0: exact zeros are demanded
    assert np.all(got["gF"][dead] == 0) and np.all(got["gZ3"][dead] == 0)


@pytest.mark.parametrize("V", R.MERGE_V)
def test_merge_backward_restatement(V):
    for i, shape in enumerate(R.MERGE_SHAPES):
        for j in range(2):
            inp = _merge_case(V, shape, i + 3 * j + V)
            _check_merge(inp, R.emul_merge(inp), R.ref_merge(inp))


def test_merge_backward_restatement_second_trip():
    inp = R.make_merge(2, *R.MERGE_BIG, R.MERGE_STRIDES[1], "random", True, seed=8232)
    assert inp["n_valid"] > R.merge_waves(2, inp["cap"]) == 8192
    _check_merge(inp, R.emul_merge(inp), R.ref_merge(inp))


@pytest.mark.parametrize("V,fw_mode,drop", [(3, None, False), (4, "zero", True), (7, "random", True)])
def test_merge_backward_closed_form_is_the_autograd(V, fw_mode, drop):
    inp = R.make_merge(V, 313, 300, R.MERGE_STRIDES[0], fw_mode, drop, seed=V)
    ref, ag = R.ref_merge(inp), R.autograd_merge(inp)
    for k in ("gZ3", "g_w", "g_b"):
        np.testing.assert_allclose(ref[k][0], ag[k], rtol=1e-9, atol=1e-12 * max(1.0, float(np.abs(ag[k]).max())))
    np.testing.assert_allclose(ref["gF"][0][..., :45], ag["gF"], rtol=1e-9, atol=1e-14)
    assert np.all(ref["gF"][0][..., 45:] == 0)


def test_merge_inputs_reach_their_branches():
    inp = R.make_merge(4, 313, 300, R.MERGE_STRIDES[1], "zero", True, seed=4)
    n, rows = 300, inp["rows"]
    assert np.isnan(inp["X6"][:, 45:]).all() and np.isnan(inp["gX7"][:, 90:]).all()
    for k in ("X6", "Hm", "vmask"):
        a = inp[k].reshape(4, 313, -1)
        assert np.isnan(a[:, n:]).all() and np.isfinite(a[:, :n, :45 if k == "X6" else None]).all()
    assert np.isnan(inp["gX7"][n:]).all()
    logit = inp["Hm"][rows].astype(np.float64) @ inp["w_last"].astype(np.float64) + float(inp["b_last"][0])
    assert logit.max() > 29.9 and logit.min() < -29.9
    hz = inp["Hm"][rows]
    assert ((hz == 0) & ~np.signbit(hz)).any() and ((hz == 0) & np.signbit(hz)).any()
    vm = inp["vmask"][rows]
    assert vm[:, 1].sum() == 0 and vm[:, 2].sum() == 1
    assert (inp["frame_w"] == 0).sum() == 1
    share = inp["dropped"].mean()
    assert 0.15 < share < 0.55, share
    rays = inp["vs_item"][:n] // inp["SR"]
    assert len(np.unique(rays)) > n // 3                              # vs_item spreads the samples over the rays
    assert int(inp["vs_item"].max()) // inp["SR"] < inp["ray_drop"].size
    assert np.all(inp["g_w_pre"] != 0) and inp["g_b_pre"][0] != 0
    assert R.merge_waves(2, R.MERGE_BIG[0]) < R.MERGE_BIG[1] and R.merge_waves(2, R.MERGE_BIG[0] - 40) >= R.MERGE_BIG[0] - 40      # the smallest two-trip capacity class
