"""The geometric-consistency filter, CPU side: the NumPy restatement of the kernels (tests/geo_filter_ref.py) against the fixture the reference produced
(tests/golden/geo_filter.npz, make_golden_geo_filter.py), the refused options and the argument validation of the new entry points.

The generator guarantees that no pair-pixel sits within the stored margins of either threshold, no kept point within `margin_world` of a `ranges` face
and no confidence near depth_conf_thresh, so counts, masks, point order, per-view counts and confidences must be EQUAL; depths and coordinates are
within the stored bounds, which the generator measured as 4 x the reference's own fp32 error against the fp64 restatement on this scene."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import geo_filter_ref as R
from tests.golden_io import GOLD


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(GOLD, "geo_filter.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def restated(gold):
    """the fp32 restatement on the fixture scene, computed once: (count, depth_avg, Kinv, Einv)"""
    Kinv, Einv = R.inverses(gold["K"], gold["E"])
    count, avg = R.geo_consistency(gold["depth"], gold["K"], Kinv, gold["E"], Einv)
    return count, avg, Kinv, Einv


def compare_lists(got, gold, tag):
    """got: dict(world, cam, conf, view_counts) in concatenated form -- the comparison the CPU and the GPU test share."""
    np.testing.assert_array_equal(np.asarray(got["view_counts"], np.int64), gold["%s_counts" % tag])
    assert got["world"].shape == gold["a_world"].shape and got["cam"].shape == gold["a_cam"].shape
    np.testing.assert_array_equal(got["cam"][:, :2], gold["a_cam"][:, :2])                           # x, y of the input: copied, in the reference's order
    e_avg = np.abs(got["cam"][:, 2].astype(np.float64) - gold["a_cam"][:, 2]).max()
    e_w = np.abs(got["world"].astype(np.float64) - gold["a_world"]).max()
    print("record %s: %d points, depth error %.3e (bound %.3e), world error %.3e (bound %.3e)" % (tag, got["world"].shape[0], e_avg, float(gold["tol_avg"]), e_w,
                                                                                                   float(gold["tol_world"])))
    assert e_avg <= float(gold["tol_avg"]) and e_w <= float(gold["tol_world"])
    np.testing.assert_array_equal(got["conf"], gold["%s_conf" % tag])


def test_the_fixture_is_the_scene_the_generator_promises(gold):
    V, H, W = gold["depth"].shape
    assert (V, H, W) == (6, 48, 64) and int(gold["geo_cnsst_num"]) == 3
    assert sorted(np.unique(gold["count"]).tolist()) == list(range(V))                                # every count 0 .. V-1 occurs
    assert (gold["depth"] == 0).any() and not np.array_equal(gold["K"][4], gold["K"][0])
    assert (gold["conf"] > gold["conf_thresh"]).any() and (gold["conf"] < gold["conf_thresh"]).any()
    assert 0 < float(gold["margin_dist"]) < 1e-2 and 0 < float(gold["margin_rel"]) < 1e-3 and 0 < float(gold["margin_world"]) < 1e-4


def test_restated_counts_equal_the_reference_and_depths_are_within_the_bound(gold, restated):
    count, avg, _, _ = restated
    np.testing.assert_array_equal(count, gold["count"])
    err = np.abs(avg.astype(np.float64) - gold["depth_avg"]).max()
    print("depth_averaged: max error %.3e, bound %.3e" % (err, float(gold["tol_avg"])))
    assert err <= float(gold["tol_avg"])
    # the fp64 form agrees about every count as well (what the generator's margins promise)
    Ki64, Ei64 = R.inverses(gold["K"], gold["E"], np.float64)
    c64, a64 = R.geo_consistency(gold["depth"], gold["K"], Ki64, gold["E"], Ei64, np.float64)
    np.testing.assert_array_equal(c64, gold["count"])
    assert np.abs(a64 - gold["depth_avg"]).max() <= float(gold["tol_avg"])


def test_no_pair_pixel_of_the_restatement_is_near_a_threshold(gold, restated):
    _, _, Kinv, Einv = restated
    V = gold["depth"].shape[0]
    with np.errstate(invalid="ignore"):
        for r in range(V):
            for s in range(V):
                if r != s:
                    o = R.reproject(gold["depth"], gold["K"], Kinv, gold["E"], Einv, r, s)
                    assert not (np.abs(o["dist"].astype(np.float64) - 1.0) < 0.5 * float(gold["margin_dist"])).any()
                    assert not (np.abs(o["rel"].astype(np.float64) - 0.01) < 0.5 * float(gold["margin_rel"])).any()


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restated_selection_equals_the_reference(gold, restated, tag):
    count, avg, _, Einv = restated
    got = R.select(gold["cam_xyz"], gold["conf"], gold["points_mask"], count, avg, Einv, gold["conf_thresh"], int(gold["geo_cnsst_num"]), gold["ranges"],
                   table=R.conf_table() if tag == "b" else None)
    compare_lists(got, gold, tag)
    cuts = np.concatenate([[0], np.cumsum(gold["a_counts"])])
    for v in range(len(cuts) - 1):
        assert (got["view"][cuts[v]:cuts[v + 1]] == v).all()
    if tag == "b":
        assert not np.array_equal(gold["b_conf"], gold["a_conf"]) and (gold["b_conf"] < gold["a_conf"]).all()


def test_one_view_has_no_geometric_mask_and_keeps_its_depth(gold):
    Kinv, Einv = R.inverses(gold["K"][:1], gold["E"][:1])
    count, avg = R.geo_consistency(gold["depth"][:1], gold["K"][:1], Kinv, gold["E"][:1], Einv)
    assert (count == 0).all() and np.array_equal(avg, gold["depth"][:1])
    got = R.select(gold["cam_xyz"][:1], gold["conf"][:1], gold["points_mask"][:1], count, avg, Einv, gold["conf_thresh"], 3, [-100.0] * 6)
    assert got["view_counts"][0] == int(((gold["conf"][0] > gold["conf_thresh"]) & (gold["points_mask"][0] != 0)).sum()) > 0


def test_conf_table_is_the_expression_of_the_reference():
    from hybridneuralrendering_amd import geo_filter as gf
    tab = gf.conf_table()
    assert tab.dtype == np.float32 and tab.shape == (10,)
    np.testing.assert_array_equal(tab, R.conf_table())
    np.testing.assert_allclose(tab, 1 - 1 / 1.14869 ** np.arange(1, 11), rtol=1e-6)
    assert abs(tab[4] - 0.5) < 1e-4                                                                   # 1.14869 = 2^(1/5) to six digits: 1.14869^5 = 2 (1 - 1.8e-5)


def lists_of(gold, device="cpu"):
    V, H, W = gold["depth"].shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return ([t(gold["cam_xyz"][v]).reshape(1, 1, 1, H, W, 3) for v in range(V)], [t(gold["K"][v])[None] for v in range(V)], [t(gold["E"][v])[None] for v in range(V)],
            [t(gold["conf"][v])[None, None] for v in range(V)], [t(gold["points_mask"][v].astype(bool))[None, None] for v in range(V)])


def opt_of(gold, **kw):
    o = dict(manual_depth_view=1, depth_conf_thresh=float(gold["conf_thresh"]), geo_cnsst_num=int(gold["geo_cnsst_num"]), default_conf=-1.0, far_plane_shift=None,
             ranges=[float(r) for r in gold["ranges"]], vox_res=0)
    o.update(kw)
    return SimpleNamespace(**o)


def test_refused_options_raise(gold):
    from hybridneuralrendering_amd import cloud_init as ci, geo_filter as gf
    from hybridneuralrendering_amd._lib import HnrError
    args = lists_of(gold)
    with pytest.raises(HnrError, match="manual_depth_view"):
        gf.filter_by_masks_gpu(*args, opt_of(gold, manual_depth_view=2))
    with pytest.raises(HnrError, match="far_plane_shift"):
        gf.filter_by_masks_gpu(*args, opt_of(gold, far_plane_shift=0.5))
    with pytest.raises(HnrError, match="GPU"):
        gf.filter_by_masks_gpu(*args, opt_of(gold))                                                   # CPU tensors: no fallback
    with pytest.raises(HnrError, match="cpu2gpu"):
        gf.filter_by_masks_gpu(*args, opt_of(gold), cpu2gpu=True)
    two = [torch.zeros(1, 1, 2, 4, 4, 3)]
    with pytest.raises(HnrError, match="num_each_depth"):
        gf.filter_by_masks_gpu(two, args[1][:1], args[2][:1], args[3][:1], args[4][:1], opt_of(gold))
    with pytest.raises(HnrError, match="alphas"):
        ci.init_cloud_from_mvs_depth([dict()], opt_of(gold), alphas=[1])
    with pytest.raises(HnrError, match="manual_depth_view"):
        ci.init_cloud_from_mvs_depth([dict()], opt_of(gold, manual_depth_view=3))
    with pytest.raises(HnrError):
        ci.init_cloud_from_mvs_depth([], opt_of(gold))
    with pytest.raises(HnrError, match="same views"):
        gf.CameraTables(gold["K"][:2], gold["E"][:3], "cpu")
    tab = gf.CameraTables(gold["K"], [torch.from_numpy(e)[None] for e in gold["E"]], "cpu")           # host arrays and tensors alike; inverses in fp32 on the CPU
    Kinv, Einv = R.inverses(gold["K"], gold["E"])
    np.testing.assert_array_equal(tab.host["Kinv"], Kinv); np.testing.assert_array_equal(tab.host["Einv"], Einv)


def test_new_entry_points_reject_bad_arguments_without_touching_the_gpu():
    from hybridneuralrendering_amd import _lib
    L = _lib.lib()
    one, null, bad = ctypes.c_void_p(256), None, -1
    f = lambda n: (ctypes.c_float * n)(*([1.0] * n))
    gc = lambda **k: [k.get("depth", one), k.get("V", 6), k.get("H", 48), k.get("W", 64), k.get("K", one), one, k.get("E", one), one, k.get("count", one),
                      k.get("avg", one), null]
    for k in ("depth", "K", "E", "count", "avg"):
        assert L.hnr_geo_consistency(*gc(**{k: null})) == bad
        assert b"NULL" in L.hnr_last_error()
    for k, v in (("V", 0), ("V", -2), ("V", 65536), ("H", 1), ("W", 1), ("H", 0), ("W", 32769), ("H", -5)):
        assert L.hnr_geo_consistency(*gc(**{k: v})) == bad
        assert b"bad argument" in L.hnr_last_error()
    assert L.hnr_geo_consistency(*gc(V=4096, H=1024, W=1024)) == bad                                  # V*H*W > 2^30
    for shape in ((0, 48, 64), (6, 1, 64), (6, 48, 40000), (4096, 1024, 1024)):
        assert L.hnr_geo_filter_select_scratch_bytes(*shape) < 0
    # (the scratch size of a valid shape needs a device -- rocprim sizes its temporaries per architecture -- and is checked in test_geo_filter_gpu.py)
    sel = lambda **k: [k.get("cam", one), one, k.get("pm", one), one, one, k.get("V", 6), k.get("H", 48), k.get("W", 64), one, 0.5, k.get("geo", 3),
                       k.get("ranges", f(6)), None, k.get("world", one), one, one, one, k.get("cap", 100), k.get("counts", one), k.get("total", one),
                       k.get("status", one), k.get("scratch", one), 1 << 30, null]
    for k in ("cam", "pm", "world", "counts", "total", "status", "scratch"):
        assert L.hnr_geo_filter_select(*sel(**{k: null})) == bad
    assert L.hnr_geo_filter_select(*sel(ranges=None)) == bad
    assert b"NULL" in L.hnr_last_error()
    assert L.hnr_geo_filter_select(*sel(cap=-1)) == bad
    assert b"capacity" in L.hnr_last_error()
    assert L.hnr_geo_filter_select(*sel(V=0)) == bad and L.hnr_geo_filter_select(*sel(H=1)) == bad and L.hnr_geo_filter_select(*sel(W=70000)) == bad
    assert L.hnr_geo_filter_select(*sel(geo=-1)) == bad
    # the confidence variant of hnr_point_embed validates like hnr_point_embed
    pe = [null, 10] + [f(16), f(16), f(3), f(9)] + [48, 64] + [one] * 11
    assert L.hnr_point_embed_conf(*pe) == bad
