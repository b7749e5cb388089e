"""CPU-side checks of the visual-hull masking and the occlusion test (csrc/hull.hip, hybridneuralrendering_amd/cloud_init.py): the restatement
(tests/hull_ref.py) equals the reference's own masks, survivor order and visible flags recorded in tests/golden/hull.npz -- in fp32 and in fp64 --
and reproduces the recorded query_embedding(depth_occ=1) run; the new argument errors; the `occlusion` keyword.  Reads only the fixtures."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import hull_ref as R
from tests.golden_io import GOLD

RECORDS = [("off_none", False, False), ("on_none", True, False), ("off_nf", False, True), ("on_nf", True, True)]


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(GOLD, "hull.npz"))
    d = {k: z[k] for k in z.files}
    w = np.load(os.path.join(GOLD, "mvs_init.npz"))
    d["sd"] = {k[3:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("sd.")}
    return d


def test_fixture_is_small_and_holds_its_margins(gold):
    assert os.path.getsize(os.path.join(GOLD, "hull.npz")) < 1000000
    assert gold["h_alphas"].shape == (5, 40, 56) and sorted(np.unique(gold["h_alphas"]).tolist()) == [0.0, np.float32(0.05), np.float32(0.15), 1.0]
    for k in ("margin_px", "margin_z", "margin_px_occ", "margin_z_occ", "tol_emb", "tol_color", "tol_dir", "tol_xyz"):
        assert 0 < float(gold[k]) < 1e-3, k
    assert not np.array_equal(gold["h_K"][3], gold["h_K"][0])


@pytest.mark.parametrize("tag,range_on,nf", RECORDS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restated_hull_mask_equals_the_reference(gold, tag, range_on, nf, dtype):
    near_far = gold["near_far"] if nf else None
    on = R.alpha_on(gold["h_alphas"])
    got = R.visual_hull(gold["h_xyz"], on, gold["h_w2c"], gold["h_K"], near_far, range_on, dtype)
    np.testing.assert_array_equal(got, gold["h_mask_" + tag] != 0)
    one = R.visual_hull(gold["h_xyz"], on[2:3], gold["h_w2c"][2:3], gold["h_K"][2:3], near_far, range_on, dtype)
    np.testing.assert_array_equal(one, gold["h_mask_v2_" + tag] != 0)
    assert 0 < got.sum() < one.sum() < got.size


def test_survivor_order_and_overflow_of_the_restated_compaction(gold):
    mask = gold["h_mask_off_nf"] != 0
    conf, view = np.arange(mask.size, dtype=np.float32), np.arange(mask.size, dtype=np.int32)[::-1]
    n, over, (xyz, c, v) = R.select(mask, mask.size, gold["h_xyz"], conf, view)
    assert n == int(mask.sum()) and not over
    np.testing.assert_array_equal(xyz, gold["h_xyz"][mask])                         # `masking`: boolean indexing keeps the input order
    assert np.all(np.diff(c) > 0) and np.array_equal(v, view[mask])
    n2, over2, (short,) = R.select(mask, n - 1, gold["h_xyz"])
    assert n2 == n and over2 and short.shape[0] == n - 1


def test_packed_bits_round_trip(gold):
    on = R.alpha_on(gold["h_alphas"])
    bits = R.pack_bits(on)
    assert bits.shape == (5, 40, 2) and bits.dtype == np.uint32
    x = np.arange(56)
    np.testing.assert_array_equal(((bits[:, :, x >> 5] >> (x & 31).astype(np.uint32)) & 1) != 0, on)
    assert not (bits[:, :, 1] >> np.uint32(56 - 32)).any()                          # the padding bits


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restated_occlusion_equals_the_reference(gold, dtype):
    vis, inside, cell, z, zmin = R.occlusion(gold["o_xyz"], gold["h_w2c"][0], gold["h_K"][0], 40, 56, float(gold["tolerate"]), dtype, details=True)
    np.testing.assert_array_equal(vis, gold["o_visible"])
    hidden = inside & (vis == 0)
    assert hidden.sum() > 150 and (~inside).sum() > 100 and (z[inside] < 0).sum() > 20 and np.bincount(cell[inside]).max() >= 3
    # the tolerance decides: with none, the points 0.05 behind the front surface are hidden too
    tight = R.occlusion(gold["o_xyz"], gold["h_w2c"][0], gold["h_K"][0], 40, 56, 0.0, dtype)
    assert (tight <= vis).all() and int(vis.sum()) - int(tight.sum()) > 100
    # a permutation of the points permutes the flags
    perm = np.random.default_rng(3).permutation(vis.size)
    np.testing.assert_array_equal(R.occlusion(gold["o_xyz"][perm], gold["h_w2c"][0], gold["h_K"][0], 40, 56, float(gold["tolerate"]), dtype), vis[perm])


def test_restated_embedding_with_occlusion_reproduces_the_reference(gold):
    emb, col, pdir = R.embed_vis(gold["sd"], gold["o_xyz"], gold["o_image"], gold["h_c2w"][0], gold["h_w2c"][0], gold["h_K"][0], gold["o_visible"],
                                 conf=gold["o_conf"])
    for got, name, tol in ((emb, "o_emb", "tol_emb"), (col, "o_color", "tol_color"), (pdir, "o_dir", "tol_dir")):
        err = float(np.abs(got - gold[name].astype(np.float64)).max())
        print("%s: %.3e (tolerance %.3e)" % (name, err, float(gold[tol])))
        assert got.shape == gold[name].shape and err <= float(gold[tol]), name
    hidden = gold["o_visible"] == 0
    assert not col[hidden].any() and col[~hidden].any() and np.abs(pdir[hidden]).max() > 0.1
    # without the flags the recorded embedding is NOT reproduced: the occlusion matters in this scene
    inside = R.occlusion(gold["o_xyz"], gold["h_w2c"][0], gold["h_K"][0], 40, 56, 1e9)
    plain, _, _ = R.embed_vis(gold["sd"], gold["o_xyz"], gold["o_image"], gold["h_c2w"][0], gold["h_w2c"][0], gold["h_K"][0], inside, conf=gold["o_conf"])
    assert float(np.abs(plain - gold["o_emb"]).max()) > 100 * float(gold["tol_emb"])


def test_staged_record_is_consistent_with_the_restatement(gold):
    """The s_ scene: the filter's restatement, the hull mask and the grouping by view give the recorded points, in the recorded order.  The points
    themselves within tol_xyz: they depend on the fp32 inverse of w2c, which LAPACK forms a few ulp differently from one CPU to the next."""
    from tests import geo_filter_ref as GR
    Kinv, Einv = GR.inverses(gold["s_K"], gold["s_w2c"])
    depth = gold["s_cam_xyz"][..., 2]
    count, avg = GR.geo_consistency(depth, gold["s_K"], Kinv, gold["s_w2c"], Einv)
    flt = GR.select(gold["s_cam_xyz"], gold["s_conf"], gold["s_points_mask"], count, avg, Einv, float(gold["s_depth_conf_thresh"]), int(gold["s_geo_cnsst_num"]),
                    np.concatenate([gold["s_spacemin"], gold["s_spacemax"]]))
    keep = R.visual_hull(flt["world"], R.alpha_on(gold["h_alphas"]), gold["h_w2c"], gold["h_K"])
    assert 0 < keep.sum() < keep.size
    assert flt["world"][keep].shape == gold["s_xyz"].shape
    assert float(np.abs(flt["world"][keep].astype(np.float64) - gold["s_xyz"]).max()) <= float(gold["tol_xyz"])
    np.testing.assert_array_equal(flt["view"][keep], gold["s_view"])
    np.testing.assert_array_equal(flt["conf"][keep], gold["s_conf_out"][:, 0])
    assert np.all(np.diff(gold["s_view"]) >= 0) and len(np.unique(gold["s_view"])) == 3


def test_new_argument_errors(gold):
    from hybridneuralrendering_amd import cloud_init as ci
    from hybridneuralrendering_amd._lib import HnrError
    K, E, al = list(gold["h_K"]), list(gold["h_w2c"]), gold["h_alphas"]
    pts = torch.from_numpy(gold["h_xyz"])
    with pytest.raises(HnrError, match="GPU"):                                       # CPU tensors
        ci.alpha_masking(pts, [a[None] for a in al], K, None, E, None)
    with pytest.raises(HnrError, match="GPU"):
        ci.AlphaMasks(al, K, E, "cpu")
    with pytest.raises(HnrError, match="GPU"):
        ci.point_occlusion(pts, E[0], K[0], 40, 56)
    with pytest.raises(HnrError, match="GPU"):
        ci.visual_hull_select(pts, None)
    opt = SimpleNamespace(depth_conf_thresh=0.5, geo_cnsst_num=1, ranges=[-100.0] * 6, default_conf=-1.0, vox_res=0)
    views = [dict()]
    for bad in (al[0, 0], al[None], [al[0, 0, :]], [al[:2]], [], "x"):                # alphas of the wrong rank (validated before any view is touched)
        with pytest.raises(HnrError, match="alphas"):
            ci.init_cloud_from_mvs_depth(views, opt, alphas=bad, alpha_cameras=(K, E))
    with pytest.raises(HnrError, match="alphas: 5 maps but 4 intrinsics"):            # a camera count different from M
        ci.init_cloud_from_mvs_depth(views, opt, alphas=al, alpha_cameras=(K[:4], E))
    with pytest.raises(HnrError, match="alphas"):
        ci.init_cloud_from_mvs_depth(views, opt, alphas=[a[None] for a in al])       # no cameras
    with pytest.raises(HnrError, match="alphas"):
        ci.init_cloud_from_mvs_depth(views, opt, alphas=[a[None] for a in al], alpha_cameras=(K,))
    with pytest.raises(HnrError, match="near_far"):                                  # near_far not a pair
        ci.init_cloud_from_mvs_depth(views, opt, alphas=[a[None] for a in al], alpha_cameras=(K, E), near_far=[1.0, 2.0, 3.0])
    with pytest.raises(HnrError, match="near_far"):
        ci._near_far_pair(2.0, "alpha_masking")
    assert ci._near_far_pair((2.0, 3.4), "x").tolist() == [1.0, np.float32(3.4)] and ci._near_far_pair(None, "x") is None


def test_alpha_shapes_and_camera_count_are_checked_before_the_device(gold, monkeypatch):
    """AlphaMasks validates on the host: the rank of the maps and a camera count different from M raise before alpha_pack is reached."""
    from hybridneuralrendering_amd import cloud_init as ci
    from hybridneuralrendering_amd._lib import HnrError
    monkeypatch.setattr(ci, "_pack_on", lambda a, dev: (_ for _ in ()).throw(AssertionError("reached the device")))
    K, E, al = list(gold["h_K"]), list(gold["h_w2c"]), gold["h_alphas"]
    for bad in (al[0, 0], al[None], [al[:2]], [al[0], al[1][:, :50]], [], [1]):
        with pytest.raises(HnrError, match="alphas"):
            ci.AlphaMasks(bad, K, E, "cuda:0")
    with pytest.raises(HnrError, match="alphas: 5 maps but 4 intrinsics"):
        ci.AlphaMasks(al, K[:4], E, "cuda:0")
    with pytest.raises(HnrError, match="alphas: 5 maps but 5 intrinsics and 3 w2cs"):
        ci.AlphaMasks([a[None] for a in al], K, E[:3], "cuda:0")
    with pytest.raises(AssertionError, match="reached the device"):                 # a well-formed call gets as far as the device
        ci.AlphaMasks([torch.from_numpy(a)[None] for a in al], K, E, "cuda:0")


def test_occlusion_keyword_is_accepted_where_plain_depth_occ_raises():
    from hybridneuralrendering_amd import cloud_init as ci, mvs_depth, mvs_init
    from hybridneuralrendering_amd._lib import HnrError
    occ = SimpleNamespace(depth_occ=1, manual_depth_view=1, manual_std_depth=0.0)
    with pytest.raises(HnrError, match="occlusion=True"):
        mvs_init.MvsInit(occ)
    with pytest.raises(HnrError, match="depth_occ"):
        mvs_depth.check_options(occ)
    with pytest.raises(HnrError, match="occlusion=True"):
        mvs_depth.depth_views({}, None, occ)
    with pytest.raises(HnrError, match="occlusion=True"):
        ci.init_cloud_from_mvs_depth([dict()], SimpleNamespace(depth_occ=1, depth_conf_thresh=0.5, geo_cnsst_num=1))
    assert mvs_init.MvsInit(occ, occlusion=True).occlusion == pytest.approx(0.1)
    assert mvs_init.MvsInit(occ, occlusion=0.25).occlusion == 0.25
    assert mvs_init.MvsInit(SimpleNamespace(depth_occ=0), occlusion=True).occlusion is None and mvs_init.MvsInit().occlusion is None
    mvs_depth.check_options(occ, occlusion=True)
    with pytest.raises(HnrError, match="MVSNet"):                                    # past the option check: the next complaint is about the net
        mvs_depth.depth_views({}, None, occ, occlusion=True)
    with pytest.raises(HnrError, match="manual_std_depth"):                          # what stays out of scope still raises with the keyword
        mvs_depth.depth_views({}, None, SimpleNamespace(depth_occ=1, manual_std_depth=0.1), occlusion=True)
    with pytest.raises(HnrError, match="no view"):
        ci.init_cloud_from_mvs_depth([], SimpleNamespace(depth_occ=1, depth_conf_thresh=0.5, geo_cnsst_num=1), occlusion=True)
    assert mvs_init.occlusion_tolerance(occ, True, "x") == pytest.approx(0.1) and mvs_init.occlusion_tolerance(None, None, "x") is None
    with pytest.raises(HnrError, match="tolerance"):
        mvs_init.occlusion_tolerance(occ, -1.0, "x")


def test_c_entries_reject_bad_arguments_before_any_launch():
    from hybridneuralrendering_amd import _lib
    L = _lib.lib()
    P = ctypes.c_void_p
    one = P(256)                                                                    # never dereferenced: every call fails validation first
    f2 = (ctypes.c_float * 2)(2.0, 1.0)
    f16, f9 = (ctypes.c_float * 16)(), (ctypes.c_float * 9)()
    err = lambda: L.hnr_last_error().decode()
    assert L.hnr_alpha_pack(None, 1, 4, 4, one, None) != 0 and "hnr_alpha_pack" in err()
    assert L.hnr_alpha_pack(one, 0, 4, 4, one, None) != 0 and L.hnr_alpha_pack(one, 1, 4, 40000, one, None) != 0
    assert L.hnr_visual_hull_select_scratch_bytes(0) < 0 and L.hnr_visual_hull_select_scratch_bytes((1 << 30) + 1) < 0
    # (the scratch size of a valid n needs a device -- rocprim sizes its temporaries per architecture: tests/test_hull_gpu.py checks the short scratch)
    nb = 1 << 20
    ok = [one, one, one, 1000, one, one, 5, 40, 56, None, 0, one, one, one, one, 1000, one, one, one, nb, None]

    def hull(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return L.hnr_visual_hull_select(*a)
    assert hull(a0=None) != 0 and "hnr_visual_hull_select" in err()
    assert hull(a1=None) != 0 and hull(a2=None) != 0                                 # outputs without their inputs
    assert hull(a6=0) != 0 and hull(a7=0) != 0 and hull(a8=40000) != 0 and hull(a15=-1) != 0 and hull(a16=None) != 0 and hull(a17=None) != 0
    assert hull(a3=0) != 0 and "scratch" in err() and hull(a9=f2) != 0 and "near_far" in err()
    assert L.hnr_point_occlusion_scratch_bytes(40, 56) >= 4 * 40 * 56 and L.hnr_point_occlusion_scratch_bytes(1, 56) < 0
    assert L.hnr_point_occlusion_scratch_bytes(8192, 8192) < 0                       # 2^26 cells: the fp32 cell index would not be exact
    sb = L.hnr_point_occlusion_scratch_bytes(40, 56)
    assert L.hnr_point_occlusion(None, 10, f16, f9, 40, 56, 0.1, one, one, sb, None) != 0 and "hnr_point_occlusion" in err()
    assert L.hnr_point_occlusion(one, 0, f16, f9, 40, 56, 0.1, one, one, sb, None) != 0
    assert L.hnr_point_occlusion(one, 10, f16, f9, 40, 56, 0.1, one, one, sb - 1, None) != 0
    assert L.hnr_point_occlusion(one, 10, f16, f9, 40, 56, -0.1, one, one, sb, None) != 0
    assert L.hnr_point_occlusion(one, 10, f16, f9, 40, 56, float("nan"), one, one, sb, None) != 0


def test_torch_ops_carry_schemas_and_trace_with_fake_tensors():
    from torch._subclasses import FakeTensorMode
    from hybridneuralrendering_amd import torch_ops, _lib
    ops = torch_ops.load()
    assert str(ops.alpha_pack.default._schema) == "hnr::alpha_pack(Tensor alphas) -> Tensor"
    assert "Tensor? visible=None" in str(ops.point_embed.default._schema) and "Tensor? visible=None" in str(ops.point_view_attrs.default._schema)
    assert str(ops.visual_hull_select.default._schema).endswith("-> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
    with FakeTensorMode():
        c = lambda *s, dt=torch.float32: torch.empty(s, device="cuda", dtype=dt)
        bits = ops.alpha_pack(c(5, 40, 56))
        assert tuple(bits.shape) == (5, 40, 2) and bits.dtype == torch.int32
        o = ops.visual_hull_select(c(300, 3), c(300), None, bits, c(5, 21), 56, [1.0, 3.4], True, 7)
        assert [tuple(t.shape) for t in o] == [(300,), (7, 3), (7,), (0,), (1,), (1,)] and o[0].dtype == torch.uint8 and o[4].dtype == torch.int64
        vis = ops.point_occlusion(c(65, 3), [0.] * 16, [0.] * 9, 37, 53, 0.1)
        assert tuple(vis.shape) == (65,) and vis.dtype == torch.uint8
        e = ops.point_embed(c(65, 3), [0.] * 16, [0.] * 16, [0.] * 3, [0.] * 9, c(3, 37, 53), c(8, 37, 53), c(16, 19, 27), c(32, 10, 14),
                            c(_lib.PREMLP_PACKED_ELEMS), False, vis)
        assert [tuple(t.shape) for t in e] == [(65, 32), (65, 3), (65, 3), (65, 0)]
        a = ops.point_view_attrs(c(65, 3), [0.] * 16, [0.] * 16, [0.] * 3, [0.] * 9, 37, 53, c(8, 37, 53), visible=vis)
        assert [tuple(t.shape) for t in a] == [(65, 8), (65, 3), (65,)]
