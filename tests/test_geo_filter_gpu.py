"""The geometric-consistency filter on the GPU (csrc/geo_filter.hip, hybridneuralrendering_amd/geo_filter.py): both kernels bit-equal to the NumPy fp32
restatement (tests/geo_filter_ref.py) on the reference-generated fixture and on seeded scenes that are deliberately NOT boundary-safe (partial tiles,
one and two views, a view that looks away, an all-zero map), determinism, the overflow rule, filter_by_masks_gpu against the reference's recorded
lists, init_cloud_from_mvs_depth against its stages done by hand, and the `conf=` argument of the embedding calls.  Reads only the fixtures and the
restatements."""
import numpy as np
import pytest
import torch

from tests import geo_filter_ref as R
from tests.bits import DEV, assert_bits_equal, t
from tests.test_geo_filter import compare_lists, gold, lists_of, opt_of, restated  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def look_at_w2c(pos, target):
    pos, target = np.asarray(pos, np.float64), np.asarray(target, np.float64)
    z = target - pos; z /= np.linalg.norm(z)
    x = np.cross(np.array([0.0, 0.0, 1.0]), z); x /= np.linalg.norm(x)
    M = np.eye(4)
    M[:3, 0], M[:3, 1], M[:3, 2], M[:3, 3] = x, np.cross(z, x), z, pos
    return np.linalg.inv(M).astype(np.float32)


def seeded_scene(V, H, W, seed, away=None, zero=None):
    """V views of the plane y = 1 from poses in front of it, 0.3 % noise; view `away` looks the other way (the points of the others lie behind it, its
    own lie behind them), view `zero` has an all-zero depth map.  Nothing here keeps values away from the thresholds."""
    rng = np.random.default_rng(seed)
    K = np.tile(np.array([[0.9 * W, 0.0, (W - 1) / 2.0], [0.0, 0.9 * W, (H - 1) / 2.0], [0.0, 0.0, 1.0]], np.float32), (V, 1, 1))
    K[V - 1, 0, 0] *= 1.1
    E, depth = [], np.zeros((V, H, W), np.float32)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    for v in range(V):
        pos = [0.3 * (v - V / 2.0), -2.0 + 0.1 * v, 1.0 + 0.05 * v]
        tgt = [0.1 * v, 1.0, 1.0] if v != away else [0.1 * v, -5.0, 1.0]
        E.append(look_at_w2c(pos, tgt))
        c2w = np.linalg.inv(E[-1].astype(np.float64))
        dirs = np.stack([xx, yy, np.ones_like(xx)], -1) @ np.linalg.inv(K[v].astype(np.float64)).T @ c2w[:3, :3].T
        with np.errstate(divide="ignore", invalid="ignore"):
            tt = (1.0 - c2w[1, 3]) / dirs[..., 1]
        tt = np.where(tt > 0, tt, 3.0)                                       # the view that looks away sees a wall at depth 3
        depth[v] = (tt * (1.0 + 0.003 * rng.standard_normal((H, W)))).astype(np.float32)
    if zero is not None:
        depth[zero] = 0.0
    depth[0, H // 3:H // 3 + 3, W // 4:W // 4 + 4] = 0.0
    E = np.stack(E)
    Kinv, Einv = R.inverses(K, E)
    cam = np.stack([np.stack(R.mat3(Kinv[v], (xx.astype(np.float32) * depth[v]), (yy.astype(np.float32) * depth[v]), depth[v]), -1) for v in range(V)]).astype(np.float32)
    conf = rng.uniform(0.0, 1.0, size=(V, H, W)).astype(np.float32)
    pm = (rng.uniform(size=(V, H, W)) > 0.1).astype(np.uint8)
    return dict(depth=depth, K=K, E=E, Kinv=Kinv, Einv=Einv, cam_xyz=cam, conf=conf, points_mask=pm)


def run_both(sc, conf_thresh, geo_num, ranges, reassign, capacity=None):
    """(GPU outputs, restated outputs) of both kernels on one scene"""
    from hybridneuralrendering_amd import geo_filter as gf
    tab = gf.CameraTables(sc["K"], sc["E"], DEV)
    np.testing.assert_array_equal(tab.host["Kinv"], sc["Kinv"]); np.testing.assert_array_equal(tab.host["Einv"], sc["Einv"])
    count, avg = gf.geometric_consistency(t(sc["depth"]), tab)
    rc, ra = sc.get("ref_count"), sc.get("ref_avg")
    if rc is None:
        rc, ra = R.geo_consistency(sc["depth"], sc["K"], sc["Kinv"], sc["E"], sc["Einv"])
    np.testing.assert_array_equal(count.cpu().numpy(), rc)
    assert_bits_equal(avg, ra)
    out = gf.select_points(t(sc["cam_xyz"]), t(sc["conf"]), t(sc["points_mask"]), count, avg, tab, conf_thresh, geo_num, ranges, reassign=reassign, capacity=capacity)
    want = R.select(sc["cam_xyz"], sc["conf"], sc["points_mask"], rc, ra, sc["Einv"], conf_thresh, geo_num, ranges, table=R.conf_table() if reassign else None)
    return out, want, (count, avg, tab)


def check_select(out, want, V):
    meta = out["meta"].cpu().numpy()
    n = int(meta[-1])
    np.testing.assert_array_equal(meta[:V], want["view_counts"])
    assert n == want["world"].shape[0] and int(out["status"].item()) == 0
    for k in ("world", "cam", "conf"):
        assert_bits_equal(out[k][:n], want[k])
    np.testing.assert_array_equal(out["view"][:n].cpu().numpy(), want["view"])
    return n


def test_fixture_scene_is_bit_equal_to_the_restatement_and_two_runs_agree(gold, restated):
    sc = dict(gold, Kinv=restated[2], Einv=restated[3], ref_count=restated[0], ref_avg=restated[1])
    for reassign in (False, True):
        out, want, (count, avg, tab) = run_both(sc, float(gold["conf_thresh"]), int(gold["geo_cnsst_num"]), gold["ranges"], reassign)
        n = check_select(out, want, 6)
        assert n == int(gold["a_counts"].sum())
        out2, _, (count2, avg2, _) = run_both(sc, float(gold["conf_thresh"]), int(gold["geo_cnsst_num"]), gold["ranges"], reassign)
        assert_bits_equal(avg2, avg); np.testing.assert_array_equal(count2.cpu().numpy(), count.cpu().numpy())
        for k in ("world", "cam", "conf", "view"):
            assert_bits_equal(out2[k][:n], out[k][:n])


@pytest.mark.parametrize("name,V,H,W,kw", [("tile tails", 3, 47, 61, {}), ("two views", 2, 24, 40, {}), ("one view", 1, 17, 33, {}),
                                           ("a view looks away", 4, 24, 36, dict(away=2)), ("an all-zero map", 4, 24, 36, dict(zero=1)),
                                           ("more views than one LDS round", 35, 9, 33, {})])
def test_seeded_scenes_are_bit_equal_to_the_restatement(name, V, H, W, kw):
    sc = seeded_scene(V, H, W, seed=V * 100 + H, **kw)
    lo, hi = [-100.0] * 3, [100.0] * 3
    lo[0] = -0.2                                                                                    # a face through the scene
    out, want, (count, avg, _) = run_both(sc, 0.4, min(2, max(V - 1, 0)), lo + hi, reassign=V > 2)
    n = check_select(out, want, V)
    c = count.cpu().numpy()
    print("%s: counts %s, %d kept" % (name, np.bincount(c.reshape(-1), minlength=V).tolist(), n))
    if V == 1:
        assert (c == 0).all() and n > 0
        assert_bits_equal(avg, sc["depth"])                                                          # averaged depth equals depth, no geometric mask
    else:
        assert c.max() > 0 and n > 0
    if "away" in kw:
        assert (c[kw["away"]] == 0).all()                                                            # nothing agrees with the view that looks away ...
        d0 = sc["depth"][0, H // 2, W // 2]
        p0 = R.mat3(sc["Kinv"][0], np.float32(W // 2) * d0, np.float32(H // 2) * d0, d0)
        assert R.mat34(R.pair(sc["E"][kw["away"]], sc["Einv"][0]), *p0)[2] < 0                       # ... for which view 0's points have a negative z
        assert not R.reproject(sc["depth"], sc["K"], sc["Kinv"], sc["E"], sc["Einv"], 0, kw["away"])["ok"].any()
    if "zero" in kw:
        assert (c[kw["zero"]] == 0).all() and (avg[kw["zero"]] == 0).all()
    # keep-everything ranges and a plain mask: the count is the mask's
    out2, want2, _ = run_both(sc, 0.4, 0, [-100.0] * 6, reassign=False)
    check_select(out2, want2, V)
    assert int(out2["meta"][-1]) == int(((sc["conf"] > np.float32(0.4)) & (sc["points_mask"] != 0)).sum())


def test_select_overflow_sets_the_status_reports_the_need_and_writes_nothing_past_the_buffer(gold, restated):
    from hybridneuralrendering_amd import geo_filter as gf, _lib
    from hybridneuralrendering_amd._lib import HnrError
    sc = dict(gold, Kinv=restated[2], Einv=restated[3], ref_count=restated[0], ref_avg=restated[1])
    need = int(gold["a_counts"].sum())
    full, want, (count, avg, tab) = run_both(sc, float(gold["conf_thresh"]), 3, gold["ranges"], False)
    cap, guard = need - 1, 64
    L = _lib.lib()
    big = dict(world=torch.full((cap + guard, 3), -777.0, device=DEV), cam=torch.full((cap + guard, 3), -777.0, device=DEV),
               conf=torch.full((cap + guard,), -777.0, device=DEV), view=torch.full((cap + guard,), -777, dtype=torch.int32, device=DEV))
    meta, status = torch.zeros((7,), dtype=torch.int64, device=DEV), torch.zeros((1,), dtype=torch.int32, device=DEV)
    nbytes = int(L.hnr_geo_filter_select_scratch_bytes(6, 48, 64))
    assert nbytes >= 2 * 4 * 6 * 48 * 64
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    import ctypes
    r = np.ascontiguousarray(gold["ranges"], dtype=np.float32)
    cam_d, conf_d, pm_d = t(gold["cam_xyz"]), t(gold["conf"]), t(gold["points_mask"])
    args = lambda sb: [_lib.ptr(cam_d), _lib.ptr(conf_d), _lib.ptr(pm_d), _lib.ptr(count), _lib.ptr(avg), 6, 48, 64,
                       _lib.ptr(tab.Einv), float(gold["conf_thresh"]), 3, r.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), None, _lib.ptr(big["world"]),
                       _lib.ptr(big["cam"]), _lib.ptr(big["conf"]), _lib.ptr(big["view"]), cap, ctypes.c_void_p(meta.data_ptr()),
                       ctypes.c_void_p(meta.data_ptr() + 48), _lib.ptr(status), _lib.ptr(scratch), sb, _lib.stream()]
    assert L.hnr_geo_filter_select(*args(nbytes - 1)) == -1 and b"scratch" in L.hnr_last_error()      # short scratch: refused before any launch
    assert torch.all(big["world"] == -777.0)
    _lib.check(L.hnr_geo_filter_select(*args(nbytes)), "hnr_geo_filter_select")
    torch.cuda.synchronize()
    assert int(status.item()) & gf.OVERFLOW and int(meta[-1].item()) == need
    np.testing.assert_array_equal(meta[:6].cpu().numpy(), gold["a_counts"])
    for k in big:
        assert torch.all(big[k][cap:] == -777)
        assert_bits_equal(big[k][:cap], full[k][:cap])                                               # what fitted is what an ample buffer holds
    with pytest.raises(HnrError, match="needs capacity %d" % need):
        gf.filter_by_masks_gpu(*lists_of(gold, DEV), opt_of(gold), capacity=cap)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_filter_by_masks_gpu_matches_the_reference_lists(gold, restated, tag):
    from hybridneuralrendering_amd import geo_filter as gf
    opt = opt_of(gold, default_conf=2.0 if tag == "b" else -1.0)
    cams, worlds, confs = gf.filter_by_masks_gpu(*lists_of(gold, DEV), opt, vis=True, return_w=True)
    assert len(cams) == len(worlds) == len(confs) == 6
    got = dict(world=torch.cat(worlds).cpu().numpy(), cam=torch.cat(cams).cpu().numpy(), conf=torch.cat(confs).cpu().numpy(), view_counts=[int(c.shape[0]) for c in cams])
    compare_lists(got, gold, tag)
    # camera matrices handed over on the host (tensors or arrays) give the same result as those on the GPU
    a = lists_of(gold, DEV)
    cams2, _, _ = gf.filter_by_masks_gpu(a[0], [k.cpu() for k in a[1]], [e.cpu().numpy() for e in a[2]], a[3], a[4], opt)
    assert_bits_equal(torch.cat(cams2), torch.cat(cams))


@pytest.fixture(scope="module")
def net():
    import os
    from tests.golden_io import GOLD
    from hybridneuralrendering_amd.mvs_init import MvsInit
    z = np.load(os.path.join(GOLD, "mvs_init.npz"))
    m = MvsInit()
    m.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")}, strict=False)
    return m.to(DEV)


def fixture_views(gold, rng, with_cam=True):
    V, H, W = gold["depth"].shape
    images = rng.uniform(0, 1, size=(V, 3, H, W)).astype(np.float32)
    views = []
    for v in range(V):
        d = dict(confidence=t(gold["conf"][v]), points_mask=t(gold["points_mask"][v].astype(bool)), intrinsic=gold["K"][v], w2c=gold["E"][v], image=t(images[v]))
        d.update(cam_xyz=t(gold["cam_xyz"][v])) if with_cam else d.update(depth=t(gold["depth"][v]))
        views.append(d)
    return views, images


@pytest.mark.parametrize("with_net", [False, True])
def test_init_cloud_from_mvs_depth_equals_its_stages_done_by_hand(gold, net, with_net):
    from hybridneuralrendering_amd import cloud_init as ci, geo_filter as gf, voxel
    opt = opt_of(gold, vox_res=40, point_features_dim=32, feature_init_method="rand")
    views, images = fixture_views(gold, np.random.default_rng(3))
    torch.manual_seed(0)
    out = ci.init_cloud_from_mvs_depth(views, opt, init_net=net if with_net else None)
    # by hand, with the existing functions
    _, worlds, confs = gf.filter_by_masks_gpu(*lists_of(gold, DEV), opt)
    vid = torch.cat([torch.full((w.shape[0],), v, dtype=torch.int32, device=DEV) for v, w in enumerate(worlds)])
    cen, _, midx = voxel.construct_vox_points_closest(torch.cat(worlds).contiguous(), 40)
    conf, vid = torch.cat(confs)[midx], vid[midx]
    perm, ids = ci.group_by_view(vid.contiguous())
    assert 0 < cen.shape[0] < torch.cat(worlds).shape[0] and len(torch.unique(ids)) == 6
    assert_bits_equal(out["xyz"], cen[perm])
    assert_bits_equal(out["conf"], conf[perm].reshape(1, -1, 1))                                     # the filtered confidence, through the voxel pick and the regrouping
    np.testing.assert_array_equal(out["view_of_point"].cpu().numpy(), ids.cpu().numpy())
    assert out["view_of_point"].dtype == torch.int64 and tuple(out["color"].shape) == (1, cen.shape[0], 3) and tuple(out["embedding"].shape) == (1, cen.shape[0], 32)
    Einv = R.inverses(gold["K"], gold["E"])[1]
    xyz, cf = out["xyz"], out["conf"][0, :, 0].contiguous()
    for v, s, e in ci.view_segments(ids.cpu().numpy()):
        if with_net:
            emb, col, pdir, c, row = net.embed_points(xyz[s:e], t(images[v]), Einv[v], gold["E"][v], gold["K"][v], conf=cf[s:e], want_row=True)
            assert_bits_equal(out["embedding"][0, s:e], emb[0])
            assert_bits_equal(row[:, 62], cf[s:e])                                                   # premlp saw the confidence in the row's last column
            assert_bits_equal(c, cf[s:e].reshape(1, -1, 1))
        else:
            _, col, pdir, c = ci.query_point_attributes(xyz[s:e], t(images[v]), Einv[v], gold["E"][v], gold["K"][v], conf=cf[s:e])
            assert_bits_equal(c, cf[s:e].reshape(1, -1, 1))
        assert_bits_equal(out["color"][0, s:e], col[0]); assert_bits_equal(out["dir"][0, s:e], pdir[0])
    # views given as depth planes: cam_xyz is formed from K^-1; same counts, points within the fixture's world bound
    views_d, _ = fixture_views(gold, np.random.default_rng(3), with_cam=False)
    if not with_net:
        out_d = ci.init_cloud_from_mvs_depth(views_d, opt_of(gold, vox_res=0, point_features_dim=32, feature_init_method="rand"))
        assert out_d["xyz"].shape[0] == int(gold["a_counts"].sum())
        assert np.abs(out_d["xyz"].cpu().numpy().astype(np.float64) - gold["a_world"]).max() <= float(gold["tol_world"])
        # the dataset's crop folded into the range mask equals cropping afterwards
        lo, hi = gold["a_world"].min(0) + np.float32(0.3), gold["a_world"].max(0) - np.float32(0.2)
        out_c = ci.init_cloud_from_mvs_depth(views, opt_of(gold, vox_res=0, point_features_dim=32, feature_init_method="rand"), spacemin=lo, spacemax=hi)
        w = torch.cat(worlds).cpu().numpy()
        m = np.all(w - lo[None] >= 0, axis=1) & np.all(hi[None] - w >= 0, axis=1)                    # train_ft.py:145-147
        assert 0 < m.sum() < w.shape[0]
        assert_bits_equal(out_c["xyz"], w[m])


def test_embed_points_without_conf_is_unchanged_and_with_conf_keeps_the_rule(gold, net):
    """conf=None must be the parent's call: hnr_point_embed itself, which now forwards to the confidence variant with a NULL array -- the same kernel
    reading the constant 1 it read before; a confidence of ones must therefore give the same bits too.  With a real confidence premlp keeps THE RULE of
    tests/test_mvs_init_gpu.py against the fp64 restatement on the rows it saw."""
    import os
    from tests import mvs_init_ref as MR
    from tests.golden_io import GOLD
    from hybridneuralrendering_amd import cloud_init as ci, mvs_init
    z = np.load(os.path.join(GOLD, "mvs_init.npz"))
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")}
    rng = np.random.default_rng(11)
    v = 2
    img = t(rng.uniform(0, 1, size=(3, 48, 64)).astype(np.float32))
    Einv = R.inverses(gold["K"], gold["E"])[1]
    xyz = t(gold["a_world"][:777])
    base = net.embed_points(xyz, img, Einv[v], gold["E"][v], gold["K"][v], want_row=True)
    feats = net.get_image_features(img[None, None])
    raw = mvs_init.point_embed(xyz, gold["E"][v], Einv[v], ci.cam_pos_cam(Einv[v], gold["E"][v]), gold["K"][v], img, feats[1][0], feats[2][0], feats[3][0],
                               net.premlp_packed(), want_row=True)
    assert_bits_equal(base[0][0], raw[0]); assert_bits_equal(base[4], raw[3])
    assert torch.all(base[3] == 1.0) and torch.all(base[4][:, 62] == 1.0)
    ones = net.embed_points(xyz, img, Einv[v], gold["E"][v], gold["K"][v], conf=torch.ones(777, device=DEV), want_row=True)
    for a, b in zip(base, ones):
        assert_bits_equal(a, b)
    assert torch.all(net.embed_points(xyz, img, Einv[v], gold["E"][v], gold["K"][v], default_conf=0.15)[3] == np.float32(0.15))
    cf = t(rng.uniform(0.05, 1.0, size=777).astype(np.float32))
    emb, col, pdir, c, row = net.embed_points(xyz, img, Einv[v], gold["E"][v], gold["K"][v], default_conf=0.15, conf=cf, want_row=True)
    assert_bits_equal(row[:, :62], base[4][:, :62]); assert_bits_equal(row[:, 62], cf); assert_bits_equal(c[0, :, 0], cf)
    rows = row.cpu()
    truth = MR.premlp(MR.state(sd, torch.float64), rows.double()).numpy()
    yard = MR.premlp(MR.state(sd, torch.float32), rows).numpy()
    e_hip, e_t = MR.rel_err(emb[0].cpu().numpy(), truth), MR.rel_err(yard, truth)
    print("premlp with a confidence: hip %.3e, torch fp32 %.3e" % (e_hip, e_t))
    assert e_t > 0 and e_hip <= 4.0 * e_t
    assert not np.array_equal(emb[0].cpu().numpy(), base[0][0].cpu().numpy())
