"""The depth estimator on the GPU (csrc/mvsnet.hip, hybridneuralrendering_amd/mvs_depth.py) against the fp64 restatement (tests/mvs_depth_ref.py, pinned to
the reference by tests/test_mvs_depth.py): every stage alone, the whole chain, `depth_views`, determinism, the torch ops, and the cloud built from
`depth_views`' output.  Reads only the fixtures and the restatement.

THE RULE, as in tests/test_mvs_init_gpu.py: error = max|a - truth| per tensor, truth in fp64; the yardstick is the error of the restatement run in fp32
on the CPU on the same inputs, with one fp32 ulp of the truth's largest magnitude as its floor; the HIP error may be at most 4 x the yardstick (only the
summation order differs).  A stage's inputs are the fp64 restatement's outputs of the stage before, rounded to fp32, so errors do not compound.

The two discrete steps are handled by exclusion: pixels whose fp64 expected index lies within 1e-3 of an integer (the confidence's four bins) and
pixels whose fp64 depth lies within 1e-5 * far of `near` or `far` (the mask) are left out, at most 2 % of a map; everywhere else idx and the mask must
be equal.

Shapes: the fixture's four (deepest level 1x1x1 -- every tap there is padding --, 2x2x3, 1x1x2, odd 3x3x2) and (3, 24, 96, 160) for the tile edges of the
3-D kernels, whose blocks cover 32 x 4 x 4 outputs (x, y, z; 32 x 4 x 2 at stride 2 and on the deepest level): 24 x 24 x 40 gives 6 x 6 x 2 tiles with a
ragged last one along x, its 6 x 6 x 10 and 3 x 3 x 5 levels ragged ones along y and z, and the 2-D kernels' 32 x 8 tiles are ragged on the 48 x 80 and
24 x 40 levels.  Measured ratios (the largest 1.5): profiles/mvs_depth_tests.txt."""
import numpy as np
import pytest
import torch

from tests import mvs_depth_ref as R
from tests.bits import DEV, assert_bits_equal, bits, t
from tests.test_mvs_depth import load_gold

pytestmark = pytest.mark.gpu

MARGIN = 4.0
EXTRA = (3, 24, 96, 160)
CASES = [0, 1, 2, 3, 4]


def f32(x):
    return x.to(torch.float32)


def rule(got, truth, yard, what, sel=None):
    """THE RULE on one tensor (sel: a boolean mask of the entries that take part)."""
    g, tr, y = (np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, np.float64) for a in (got, truth, yard))
    assert g.shape == tr.shape, (what, g.shape, tr.shape)
    floor = R.ulp_of_max(tr)
    if sel is not None:
        g, tr, y = g[sel], tr[sel], y[sel]
    e_hip, e_t = float(np.abs(g - tr).max()), float(np.abs(y - tr).max())
    print("%s: hip %.3e, restatement fp32 %.3e, ulp of max %.3e -> ratio %.2f" % (what, e_hip, e_t, floor, e_hip / max(e_t, floor)))
    assert np.isfinite(g).all() and e_hip <= MARGIN * max(e_t, floor), (what, e_hip, e_t, floor)


def extra_case():
    V, D, H, W = EXTRA
    rng = np.random.default_rng(160)
    h, w = H // 4, W // 4
    K = np.array([[1.1 * w, 0, 0.5 * w, 0], [0, 1.1 * w, 0.5 * h, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    proj = [np.eye(4)]
    for v in range(1, V):
        E = np.eye(4)
        a = rng.uniform(-0.05, 0.05)
        E[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        E[:3, 3] = rng.uniform(0.15, 0.35, 3) * rng.choice([-1.0, 1.0], 3) * [1.0, 1.0, 0.3]
        proj.append(K @ E @ np.linalg.inv(K))
    return dict(V=V, D=D, H=H, W=W, images=(rng.integers(0, 16, size=(V, 3, H, W)) / np.float32(15)).astype(np.float32),
                proj=np.stack(proj).astype(np.float32), depth_values=(2.0 + np.arange(D, dtype=np.float32) * np.float32(2.0 / D)).astype(np.float32))


@pytest.fixture(scope="module")
def gold():
    g = load_gold()
    g["cases"].append(extra_case())
    return g


@pytest.fixture(scope="module")
def net(gold):
    from hybridneuralrendering_amd.mvs_depth import MVSNet
    return MVSNet().load_pretrained(dict(gold["sd"])).to(DEV)


def image_intrinsic(H, W):
    return np.array([[1.1 * W, 0, 0.5 * W], [0, 1.1 * W, 0.5 * H], [0, 0, 1]], dtype=np.float32)


@pytest.fixture(scope="module")
def stages(gold):
    """Per case, once: the fp64 chain, each stage's fp32-rounded input, and per stage the fp64 truth and the fp32 yardstick ON that input."""
    from hybridneuralrendering_amd.mvs_depth import kt_inverse
    out, sd = [], gold["sd"]
    for c in gold["cases"]:
        proj, dv = c["proj"], c["depth_values"]
        s = dict(chain64=R.mvsnet(sd, c["images"], proj, dv, torch.float64), chain32=R.mvsnet(sd, c["images"], proj, dv, torch.float32))
        s["feat_in"] = f32(s["chain64"]["features"])
        s["vol64"], s["vol32"] = R.cost_volume(s["feat_in"], proj, dv, torch.float64), R.cost_volume(s["feat_in"], proj, dv, torch.float32)
        s["vol_in"] = f32(s["vol64"])
        s["logits64"], s["logits32"] = R.cost_reg(sd, s["vol_in"], torch.float64), R.cost_reg(sd, s["vol_in"], torch.float32)
        s["logits_in"] = f32(s["logits64"])
        s["head64"], s["head32"] = R.depth_head(s["logits_in"], dv, torch.float64), R.depth_head(s["logits_in"], dv, torch.float32)
        s["depth_in"], s["conf_in"] = f32(s["head64"][0]), f32(s["head64"][1])
        lo, hi = float(s["depth_in"].min()), float(s["depth_in"].max())
        s["near"], s["far"] = np.float32(lo + 0.3 * (hi - lo)), np.float32(lo + 0.8 * (hi - lo))                 # inside the range: the mask cuts through the map
        s["K"] = image_intrinsic(c["H"], c["W"])
        s["kt_inv"] = kt_inverse(s["K"])                                                                         # the fp32 inverse the kernels are given
        s["pts64"] = R.depth_points(s["depth_in"], s["conf_in"], c["H"], c["W"], s["near"], s["far"], dtype=torch.float64, kt_inv=s["kt_inv"])
        s["pts32"] = R.depth_points(s["depth_in"], s["conf_in"], c["H"], c["W"], s["near"], s["far"], dtype=torch.float32, kt_inv=s["kt_inv"])
        out.append(s)
    return out


def tag(c):
    return "(%d, %d, %d, %d)" % (c["V"], c["D"], c["H"], c["W"])


def index_selection(fidx64):
    """Pixels whose expected index is not within 1e-3 of an integer; at most 2 % may be left out."""
    f = fidx64.numpy()
    sel = np.abs(f - np.round(f)) >= 1e-3
    assert (~sel).mean() <= 0.02, "more than 2 %% of the map within 1e-3 of an integer index: %.3f" % (~sel).mean()
    return sel


def mask_selection(depth64_up, near, far):
    d = depth64_up.numpy()
    sel = (np.abs(d - float(near)) >= 1e-5 * float(far)) & (np.abs(d - float(far)) >= 1e-5 * float(far))
    assert (~sel).mean() <= 0.02, "more than 2 %% of the map within 1e-5 * far of near / far: %.3f" % (~sel).mean()
    return sel


@pytest.mark.parametrize("i", CASES)
def test_feature_net_alone(gold, net, stages, i):
    from hybridneuralrendering_amd import mvs_depth as md
    c, s = gold["cases"][i], stages[i]
    got = md.feature_forward(t(c["images"]), net.packed()[0])
    assert tuple(got.shape) == (c["V"], 32, c["H"] // 4, c["W"] // 4) and not got.requires_grad
    rule(got, s["chain64"]["features"], s["chain32"]["features"], "features " + tag(c))


@pytest.mark.parametrize("i", CASES)
def test_cost_volume_alone(gold, net, stages, i):
    from hybridneuralrendering_amd import mvs_depth as md
    c, s = gold["cases"][i], stages[i]
    got = md.cost_volume(t(s["feat_in"]), t(c["proj"]), t(c["depth_values"]))
    rule(got, s["vol64"], s["vol32"], "cost volume " + tag(c))
    if i == 0:                                                           # [V,4,4] projections give the same bits as their first three rows
        assert_bits_equal(md.cost_volume(t(s["feat_in"]), t(c["proj"][:, :3]), t(c["depth_values"])), got)


def test_cost_volume_reads_nothing_for_coordinates_that_are_not_finite_or_far_off(gold, stages):
    """View 1 projects to q.z = 0 (a division by zero: inf or NaN coordinates), view 2 a million pixels away: both contribute zero, so the volume is
    that of the three views with zero samples for two of them: f0^2 / 3 - (f0 / 3)^2, finite everywhere."""
    from hybridneuralrendering_amd import mvs_depth as md
    c, s = gold["cases"][0], stages[0]
    proj = c["proj"][:, :3].copy()
    proj[1] = 0.0
    proj[1, 0, 0] = 1.0
    proj[2] = np.array([[1, 0, 0, 1e6], [0, 1, 0, -1e6], [0, 0, 0, 1]], dtype=np.float32)
    got = md.cost_volume(t(s["feat_in"]), t(proj), t(c["depth_values"])).cpu()
    assert torch.isfinite(got).all()
    want = []
    for dtype in (torch.float64, torch.float32):
        w0 = R.warp(s["feat_in"][0].to(dtype), torch.from_numpy(proj[0]).to(dtype), torch.from_numpy(c["depth_values"]).to(dtype))
        want.append(w0 ** 2 / 3 - (w0 / 3) ** 2)
    rule(got, want[0], want[1], "cost volume with two views that contribute nothing")


@pytest.mark.parametrize("i", CASES)
def test_cost_regularisation_alone(gold, net, stages, i):
    from hybridneuralrendering_amd import mvs_depth as md
    c, s = gold["cases"][i], stages[i]
    got = md.cost_reg(t(s["vol_in"]), net.packed()[1])
    assert tuple(got.shape) == (c["D"], c["H"] // 4, c["W"] // 4)
    rule(got, s["logits64"], s["logits32"], "logits " + tag(c))


@pytest.mark.parametrize("i", CASES)
def test_depth_head_alone(gold, stages, i):
    from hybridneuralrendering_amd import mvs_depth as md
    c, s = gold["cases"][i], stages[i]
    depth, conf, prob = md.depth_head(t(s["logits_in"]), t(c["depth_values"]), want_prob=True)
    d64, c64, p64, fidx64 = s["head64"]
    d32, c32, p32, _ = s["head32"]
    rule(depth, d64, d32, "depth " + tag(c))
    rule(prob, p64, p32, "prob " + tag(c))
    sel = index_selection(fidx64)
    rule(conf, c64, c32, "confidence " + tag(c), sel)
    # idx itself: the kernel's confidence is, bit for bit, the ascending fp32 sum of ITS probabilities over the bins idx-1 .. idx+2
    idx, p = fidx64.long().numpy(), prob.cpu().numpy()
    want = np.zeros(idx.shape, np.float32)
    for k in range(-1, 3):
        kk = idx + k
        ok = (kk >= 0) & (kk < c["D"])
        want = (want + np.where(ok, np.take_along_axis(p, np.clip(kk, 0, c["D"] - 1)[None], 0)[0], np.float32(0))).astype(np.float32)
    np.testing.assert_array_equal(bits(conf)[sel], bits(want)[sel])
    assert md.depth_head(t(s["logits_in"]), t(c["depth_values"]))[2] is None


@pytest.mark.parametrize("i", CASES)
def test_depth_points_alone(gold, stages, i):
    from hybridneuralrendering_amd import mvs_depth as md
    c, s = gold["cases"][i], stages[i]
    cam, conf, mask = md.depth_points(t(s["depth_in"]), t(s["conf_in"]), c["H"], c["W"], s["near"], s["far"], s["K"])
    cam64, conf64, mask64, d_up = s["pts64"]
    assert tuple(cam.shape) == (c["H"], c["W"], 3) and mask.dtype == torch.bool
    rule(cam, cam64, s["pts32"][0], "cam_xyz " + tag(c))
    assert_bits_equal(conf, f32(conf64))                                 # nearest upsampling copies
    sel = mask_selection(d_up, s["near"], s["far"])
    np.testing.assert_array_equal(mask.cpu().numpy()[sel], mask64.numpy()[sel])
    assert 0.05 < mask64.float().mean() < 0.95


def test_depth_points_nearest_rule_when_the_image_is_no_multiple_of_the_map(gold, stages):
    """50 x 70 from 8 x 8: torch's `nearest` source index, floor(dst * (in / out)) in fp32."""
    from hybridneuralrendering_amd import mvs_depth as md
    s = stages[0]
    K = image_intrinsic(50, 70)
    cam, conf, mask = md.depth_points(t(s["depth_in"]), t(s["conf_in"]), 50, 70, s["near"], s["far"], K)
    cam64, conf64, mask64, d_up = R.depth_points(s["depth_in"], s["conf_in"], 50, 70, s["near"], s["far"], dtype=torch.float64, kt_inv=md.kt_inverse(K))
    cam32 = R.depth_points(s["depth_in"], s["conf_in"], 50, 70, s["near"], s["far"], dtype=torch.float32, kt_inv=md.kt_inverse(K))[0]
    assert_bits_equal(conf, f32(conf64))
    rule(cam, cam64, cam32, "cam_xyz 50x70 from 8x8")
    np.testing.assert_array_equal(mask.cpu().numpy(), mask64.numpy())


@pytest.mark.parametrize("i", CASES)
def test_whole_chain_against_fp64(gold, net, stages, i):
    """images -> depth, confidence, probability volume through MVSNet.forward, the yardstick taken end to end."""
    c, s = gold["cases"][i], stages[i]
    depth, conf, feats, prob = net(t(c["images"])[None], t(c["proj"])[None], t(c["depth_values"])[None], want_prob=True)
    assert tuple(depth.shape) == (1, c["H"] // 4, c["W"] // 4) and len(feats) == c["V"] and tuple(feats[0].shape) == (1, 32, c["H"] // 4, c["W"] // 4)
    a, b = s["chain64"], s["chain32"]
    rule(depth[0], a["depth"], b["depth"], "chain depth " + tag(c))
    rule(prob[0], a["prob"], b["prob"], "chain prob " + tag(c))
    rule(conf[0], a["confidence"], b["confidence"], "chain confidence " + tag(c), index_selection(a["fidx"]))
    # the reference's `features` argument: the maps handed back in give the same bits, and no probability volume unless asked for
    again = net(t(c["images"])[None], t(c["proj"])[None], t(c["depth_values"])[None], features=feats)
    assert_bits_equal(again[0], depth); assert_bits_equal(again[1], conf)
    assert again[3] is None


def batch_of(c, near_far):
    """A dataset item for depth_views: row i of proj_mats is `every view seen from view i`; here row 1 is row 0 with its views rolled, row 2 row 0."""
    V, H, W = c["V"], c["H"], c["W"]
    proj = np.stack([c["proj"][:, :3], np.roll(c["proj"][:, :3], 1, axis=0), c["proj"][:, :3]])[:, :V]
    rng = np.random.default_rng(7)
    w2cs = np.tile(np.eye(4, dtype=np.float32), (V, 1, 1))
    w2cs[:, :3, 3] = rng.uniform(-0.2, 0.2, size=(V, 3)).astype(np.float32)
    K = np.tile(image_intrinsic(H, W), (V, 1, 1))
    return dict(images=t(rng.uniform(0, 1, size=(1, V, 3, H, W)).astype(np.float32)), mvs_images=t(c["images"])[None], proj_mats=t(proj[:V])[None],
                near_fars=t(np.tile(np.asarray(near_far, np.float32), (V, 1)))[None], near_fars_depth=t(np.array([[2.0, 4.0]], np.float32)),
                intrinsics=t(K)[None], w2cs=t(w2cs)[None])


def test_depth_views_against_fp64(gold, net, stages):
    """The manual_depth_view == 1 branch on the first fixture shape: 192 depth planes from near_fars_depth, mvs_images for the estimator, two entries of
    depth_vid, points and mask with each view's near_fars; end to end against fp64 with the yardstick taken end to end."""
    from types import SimpleNamespace
    from hybridneuralrendering_amd import mvs_depth as md
    c, sd = gold["cases"][0], gold["sd"]
    dv = (np.float32(2.0) + np.arange(192, dtype=np.float32) * np.float32((4.0 - 2.0) / 192.)).astype(np.float32)
    b0 = batch_of(c, (2.0, 4.0))
    proj = b0["proj_mats"][0].cpu().numpy()
    ref64 = [R.mvsnet(sd, c["images"], proj[v], dv, torch.float64) for v in (0, 1)]
    ref32 = [R.mvsnet(sd, c["images"], proj[v], dv, torch.float32) for v in (0, 1)]
    lo, hi = float(ref64[0]["depth"].min()), float(ref64[0]["depth"].max())
    near, far = np.float32(lo + 0.3 * (hi - lo)), np.float32(lo + 0.8 * (hi - lo))
    batch = batch_of(c, (near, far))
    opt = SimpleNamespace(init_view_num=3, depth_vid="01", manual_depth_view=1, manual_std_depth=0.0, depth_occ=0)
    views = md.depth_views(batch, net, opt)
    assert len(views) == 2
    for v, view in enumerate(views):
        K = batch["intrinsics"][0, v].cpu().numpy()
        kti = md.kt_inverse(K)
        p64 = R.depth_points(ref64[v]["depth"], ref64[v]["confidence"], c["H"], c["W"], near, far, dtype=torch.float64, kt_inv=kti)
        p32 = R.depth_points(ref32[v]["depth"], ref32[v]["confidence"], c["H"], c["W"], near, far, dtype=torch.float32, kt_inv=kti)
        rule(view["depth"], ref64[v]["depth"], ref32[v]["depth"], "depth_views depth, view %d" % v)
        rule(view["cam_xyz"], p64[0], p32[0], "depth_views cam_xyz, view %d" % v)
        up = lambda m: np.repeat(np.repeat(m, 4, axis=0), 4, axis=1)
        sel_i = up(index_selection(ref64[v]["fidx"]))
        rule(view["confidence"], p64[1], p32[1], "depth_views confidence, view %d" % v, sel_i)
        sel_m = mask_selection(p64[3], near, far)
        np.testing.assert_array_equal(view["points_mask"].cpu().numpy()[sel_m], p64[2].numpy()[sel_m])
        assert 0.02 < p64[2].float().mean() < 0.98
        assert_bits_equal(view["image"], batch["images"][0, v]); assert_bits_equal(view["intrinsic"], batch["intrinsics"][0, v])
        assert_bits_equal(view["w2c"], batch["w2cs"][0, v])
    assert not torch.equal(views[0]["depth"], views[1]["depth"])


def test_two_runs_give_the_same_bits(gold, net, stages):
    from hybridneuralrendering_amd import mvs_depth as md
    for i in (1, 4):
        c, s = gold["cases"][i], stages[i]
        calls = (lambda: (md.feature_forward(t(c["images"]), net.packed()[0]),),
                 lambda: (md.cost_volume(t(s["feat_in"]), t(c["proj"]), t(c["depth_values"])),),
                 lambda: (md.cost_reg(t(s["vol_in"]), net.packed()[1]),),
                 lambda: md.depth_head(t(s["logits_in"]), t(c["depth_values"]), want_prob=True),
                 lambda: md.depth_points(t(s["depth_in"]), t(s["conf_in"]), c["H"], c["W"], s["near"], s["far"], s["K"]),
                 lambda: net(t(c["images"])[None], t(c["proj"])[None], t(c["depth_values"])[None], want_prob=True)[:2])
        for call in calls:
            for a, b in zip(call(), call()):
                assert_bits_equal(a, b)


def test_torch_ops_equal_the_ctypes_path(gold, net, stages):
    from hybridneuralrendering_amd import mvs_depth as md, torch_ops
    c, s = gold["cases"][1], stages[1]
    fpk, rpk = net.packed()
    assert_bits_equal(torch_ops.mvsnet_feature(t(c["images"]), fpk), md.feature_forward(t(c["images"]), fpk))
    assert_bits_equal(torch_ops.mvsnet_cost_volume(t(s["feat_in"]), t(c["proj"]), t(c["depth_values"])), md.cost_volume(t(s["feat_in"]), t(c["proj"]), t(c["depth_values"])))
    assert_bits_equal(torch_ops.mvsnet_cost_reg(t(s["vol_in"]), rpk), md.cost_reg(t(s["vol_in"]), rpk))
    for a, b in zip(torch_ops.mvsnet_depth_head(t(s["logits_in"]), t(c["depth_values"]), True), md.depth_head(t(s["logits_in"]), t(c["depth_values"]), True)):
        assert_bits_equal(a, b)
    assert tuple(torch_ops.mvsnet_depth_head(t(s["logits_in"]), t(c["depth_values"]))[2].shape) == (0,)
    a = torch_ops.mvsnet_depth_points(t(s["depth_in"]), t(s["conf_in"]), c["H"], c["W"], s["near"], s["far"], s["K"])
    b = md.depth_points(t(s["depth_in"]), t(s["conf_in"]), c["H"], c["W"], s["near"], s["far"], s["K"])
    assert_bits_equal(a[0], b[0]); assert_bits_equal(a[1], b[1]); assert_bits_equal(a[2], b[2].to(torch.uint8))


def test_unsupported_calls_raise_on_the_gpu(gold, net):
    from hybridneuralrendering_amd import mvs_depth as md
    from hybridneuralrendering_amd._lib import HnrError
    z = lambda *s: torch.zeros(s, device=DEV)
    with pytest.raises(HnrError, match="multiples of 8"):
        net(z(1, 3, 3, 36, 32), z(1, 3, 3, 4), z(1, 8))
    with pytest.raises(HnrError, match="multiple of 8"):
        md.cost_reg(z(32, 8, 9, 8), net.packed()[1])
    with pytest.raises(HnrError, match="prob_only"):
        net(z(1, 3, 3, 32, 32), z(1, 3, 3, 4), z(1, 8), prob_only=True)
    with pytest.raises(HnrError):
        net(z(1, 3, 3, 32, 32).cpu(), z(1, 3, 3, 4), z(1, 8))
    with pytest.raises(HnrError):
        md.MVSNet()(z(1, 3, 3, 32, 32), z(1, 3, 3, 4), z(1, 8))               # the module was left on the CPU


def test_init_cloud_from_depth_views_equals_the_maps_fed_by_hand(gold, net):
    """Three views of the second fixture shape: the cloud from depth_views' dicts, and from dicts written by hand out of the stage calls."""
    from types import SimpleNamespace
    from hybridneuralrendering_amd import cloud_init as ci, mvs_depth as md
    c = gold["cases"][1]
    batch = batch_of(c, (2.0, 4.0))
    opt = SimpleNamespace(init_view_num=3, depth_vid=[0, 1, 2], manual_depth_view=1, manual_std_depth=0.0, depth_occ=0, depth_conf_thresh=0.0, geo_cnsst_num=0,
                          default_conf=-1.0, far_plane_shift=None, ranges=[-100.0] * 6, vox_res=60, point_features_dim=32, feature_init_method="rand")
    views = md.depth_views(batch, net, opt)
    torch.manual_seed(0)
    out = ci.init_cloud_from_mvs_depth(views, opt)
    dv = t((np.float32(2.0) + np.arange(192, dtype=np.float32) * np.float32(2.0 / 192.)).astype(np.float32))
    assert_bits_equal(dv, batch["near_fars_depth"][0, 0] + torch.arange(0, 192, device=DEV, dtype=torch.float32) * ((batch["near_fars_depth"][0, 1] - batch["near_fars_depth"][0, 0]) / 192.))
    feats = net.image_features(batch["mvs_images"][0])
    hand = []
    for v in range(3):
        depth, conf, _ = md.depth_head(md.cost_reg(md.cost_volume(feats, batch["proj_mats"][0, v], dv), net.packed()[1]), dv)
        cam, cf, mask = md.depth_points(depth, conf, c["H"], c["W"], 2.0, 4.0, batch["intrinsics"][0, v])
        hand.append(dict(cam_xyz=cam, confidence=cf, points_mask=mask, intrinsic=batch["intrinsics"][0, v], w2c=batch["w2cs"][0, v], image=batch["images"][0, v]))
        assert_bits_equal(views[v]["cam_xyz"], cam); assert_bits_equal(views[v]["confidence"], cf)
    torch.manual_seed(0)
    want = ci.init_cloud_from_mvs_depth(hand, opt)
    n = out["xyz"].shape[0]
    assert n > 100 and len(torch.unique(out["view_of_point"])) == 3
    for k in ("xyz", "embedding", "color", "dir", "conf", "view_of_point"):
        assert_bits_equal(out[k], want[k])
