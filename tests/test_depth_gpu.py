"""Expected-depth maps on the GPU: hnr_ray_depth against fp64, the depth term of the composite transpose against fp64 autograd, the render
paths against the CPU oracle's blend weights, a plane of known depth, depth-supervised training gradients against the oracle's autograd, and
the module / driver surfaces.  Depth: D = sum_s w_s z_s / (sum_s w_s + 1e-6), w = blend weight, z = camera-space depth of the shading sample
(the compute_depth branch of models/neural_points_volumetric_model.py:381-385, `ray_ts` read as sample_loc[..., 2])."""
import numpy as np
import pytest
import torch

from tests.golden_io import load_render, load_train, torch_inputs

pytestmark = pytest.mark.gpu

W_DEPTH = 0.1              # weight of the depth term in the training tests


def _zc(loc_w, campos, rot):
    """The composite's z in fp32, operation by operation: ((r2 s0 + r5 s1) + r8 s2), s = p - campos."""
    f = np.float32
    s = loc_w.astype(f) - campos.astype(f)
    r = rot.astype(f)
    return (s[..., 0] * r[0, 2] + s[..., 1] * r[1, 2]) + s[..., 2] * r[2, 2]


def _ray_depth(bw, loc_w, nsamp, mask, campos, rot):
    from hybridneuralrendering_amd.render import ray_depth
    dev = torch.device("cuda:0")
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return ray_depth(t(bw), t(loc_w), t(nsamp), t(mask), t(campos), t(rot))


@pytest.mark.parametrize("SR", [1, 24, 80])
@pytest.mark.parametrize("padded", [True, False])
def test_ray_depth_matches_fp64(SR, padded):
    rng = np.random.default_rng(SR * 2 + padded)
    R = 517
    campos = rng.normal(size=3).astype(np.float32)
    rot = np.linalg.qr(rng.normal(size=(3, 3)))[0].astype(np.float32)
    cam = np.concatenate([rng.normal(size=(R, SR, 2)) * 0.1, 0.5 + 3 * rng.uniform(size=(R, SR, 1))], axis=-1)
    loc_w = (cam @ rot.T.astype(np.float64) + campos).astype(np.float32)
    bw = (rng.uniform(size=(R, SR)) * (rng.uniform(size=(R, SR)) > 0.3)).astype(np.float32)
    nsamp = rng.integers(0, SR + 1, size=R).astype(np.int32)
    mask = (rng.uniform(size=R) > 0.15).astype(np.int8)
    inside = np.arange(SR)[None, :] < nsamp[:, None]
    if padded:
        bw[~inside], loc_w[~inside] = 0.0, 0.0                   # the padding values of the query / composite outputs
    else:
        bw[~inside], loc_w[~inside] = np.nan, np.nan             # unwritten slots: must not be read
    bw_in = bw.copy()
    bw_in[mask == 0] = np.nan                                    # rays without neighbours are not read either
    z = _zc(np.nan_to_num(loc_w), campos, rot).astype(np.float64)
    w = np.where(inside, bw, 0.0).astype(np.float64)
    ref = np.where(mask > 0, (w * z).sum(-1) / (w.sum(-1) + 1e-6), 0.0)
    got = _ray_depth(bw_in, loc_w, None if padded else nsamp, mask, campos, rot)
    again = _ray_depth(bw_in, loc_w, None if padded else nsamp, mask, campos, rot)
    assert torch.equal(got, again)                               # fixed summation order
    g = got.cpu().numpy().astype(np.float64)
    assert np.all(g[mask == 0] == 0.0)
    np.testing.assert_allclose(g, ref, rtol=2e-6, atol=0)
    # R = 0: nothing launched, nothing written
    from hybridneuralrendering_amd import _lib
    assert _lib.lib().hnr_ray_depth(None, None, None, None, None, None, 0, SR, None, _lib.stream()) == 0


@pytest.mark.parametrize("R,SR,unit", [(300, 24, 1), (64, 80, 1), (129, 64, 0), (5, 1, 1)])
def test_composite_backward_with_depth_matches_autograd(R, SR, unit):
    """hnr_composite_bwd_depth vs fp64 autograd of sum(g_col . colour) + sum(g_D D) (setup and tolerances of test_composite_bwd_gpu.py);
    with NULL g_depth it is hnr_composite_bwd bit for bit."""
    from hybridneuralrendering_amd import _lib
    L = _lib.lib()
    K = 8
    g = torch.Generator().manual_seed(R * 100 + SR)
    vz = 0.008
    campos = torch.randn(3, generator=g)
    rot, _ = torch.linalg.qr(torch.randn(3, 3, generator=g))
    depth = torch.cumsum(torch.rand(R, SR, generator=g) * 3 * vz * (torch.rand(R, SR, generator=g) > 0.2), dim=1) + 0.5
    lateral = torch.randn(R, SR, 2, generator=g) * 0.1
    cam = torch.cat([lateral, depth[..., None]], dim=-1)
    loc_w = (cam @ rot.T + campos).float().contiguous()
    nsamp = torch.randint(0, SR + 1, (R,), generator=g, dtype=torch.int32)
    pidx = torch.randint(-1, 50, (R, SR, K), generator=g, dtype=torch.int32)
    pidx[torch.arange(SR)[None, :] >= nsamp[:, None]] = -1
    ray_mask = (torch.rand(R, generator=g) > 0.15).to(torch.int8)
    decoded = torch.cat([torch.nn.functional.softplus(torch.randn(R, SR, 1, generator=g)) * 40, torch.rand(R, SR, 3, generator=g)], dim=-1).contiguous()
    bg = torch.rand(3, generator=g)
    g_col = torch.randn(R, 3, generator=g)
    g_dep = torch.randn(R, generator=g)

    inside = (torch.arange(SR)[None, :] < nsamp[:, None])
    z = ((torch.where(inside[..., None], loc_w, torch.zeros_like(loc_w)) - campos) @ rot[:, 2]).float()
    zn = z.numpy()
    dist = np.zeros((R, SR), np.float32)
    for r in range(R):
        zmax = zn[r, 0]
        for s in range(SR):
            if s + 1 < SR:
                nz = max(zmax, zn[r, s + 1]); d = np.float32(nz - zmax); zmax = nz
            else:
                d = np.float32(vz)
            if d < 1e-8 or (unit and d > 2 * np.float32(vz)):
                d = np.float32(vz)
            dist[r, s] = d
    valid = inside & (pidx[..., 0] >= 0)
    dec64 = decoded.double().requires_grad_(True)
    sigma = torch.where(valid, dec64[..., 0], torch.zeros((), dtype=torch.float64))
    rd = torch.where(valid, torch.from_numpy(dist).double(), torch.zeros((), dtype=torch.float64))
    o = 1 - torch.exp(-sigma * rd)
    q = 1 - o + 1e-10
    T = torch.cumprod(torch.cat([torch.ones(R, 1, dtype=torch.float64), q[:, :-1]], dim=1), dim=1)
    w = o * T
    col = (w[..., None] * dec64[..., 1:]).sum(1) + bg.double() * (T[:, -1] * q[:, -1])[:, None]
    D = (w * z.double()).sum(1) / (w.sum(1) + 1e-6)
    m = ray_mask.double()
    ((col * g_col.double() * m[:, None]).sum() + (D * g_dep.double() * m).sum()).backward()
    ref = dec64.grad.float().numpy()

    dev = torch.device("cuda:0")
    t = lambda x: x.to(dev).contiguous()
    P = _lib.ptr
    args = [t(decoded), t(loc_w), t(pidx), t(ray_mask), t(nsamp), t(campos), t(rot.contiguous()), t(bg), t(g_col), t(g_dep)]

    def run(fn, g_depth):
        out = torch.full((R, SR, 4), 7.0, dtype=torch.float32, device=dev)
        a = [P(x) for x in args[:8]] + [R, SR, K, vz, unit, P(args[8])]
        if fn == "hnr_composite_bwd":
            rc = L.hnr_composite_bwd(*a, P(out), _lib.stream())
        else:
            rc = L.hnr_composite_bwd_depth(*a, g_depth, P(out), _lib.stream())
        _lib.check(rc, fn)
        return out

    got = run("hnr_composite_bwd_depth", P(args[9])).cpu().numpy()
    rtol, atol = 2e-4, 2e-5 * max(1.0, float(np.abs(ref).max()))
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol)
    if SR > 1:
        # the depth term is really there: the colour-only transpose misses this reference (with one sample per ray D = z w / (w + 1e-6)
        # hardly depends on w)
        colour_only = run("hnr_composite_bwd", None).cpu().numpy()
        assert (np.abs(colour_only - ref) > rtol * np.abs(ref) + atol).any()
    # NULL depth gradient: the colour-only kernels, same bits
    assert torch.equal(run("hnr_composite_bwd_depth", None), run("hnr_composite_bwd", None))


def _render_setup(tag):
    from hybridneuralrendering_amd import scenes
    from hybridneuralrendering_amd.aggregator import PointAggregator
    from hybridneuralrendering_amd.render import HybridRenderer, PointCloud
    d = load_render(tag)
    dev = torch.device("cuda:0")
    opt = scenes.default_opt(**{k: v for k, v in d["opt"].items()})
    agg = PointAggregator(opt)
    agg.load_state_dict(d["sd"], strict=True)
    agg = agg.to(dev)
    ti = torch_inputs(d, dev)
    cloud = PointCloud(ti["xyz"], ti["emb"], ti["conf"], ti["pdir"], ti["color"])
    return d, ti, opt, cloud, HybridRenderer(opt, agg, dev)


def test_render_depth_matches_oracle_and_leaves_the_other_outputs_alone():
    """render_rays(want_depth=True) on both paths (single call, un-padded; staged, padded and un-padded) against the depth formed from the CPU
    oracle's blend_weight and sample_loc[..., 2]; colour / opacity / mask bit-identical to the same call without depth."""
    from oracle import render_oracle as ro
    d, ti, opt, cloud, rnd = _render_setup("scannet_small")
    near, far = d["near_far"]
    dev = ti["raydir"].device
    tc = torch_inputs(d)
    q = dict(sample_pidx=d["q_sample_pidx"], sample_loc_w=d["q_sample_loc_w"], ray_mask=d["q_ray_mask"])
    with torch.no_grad():
        ref = ro.render(tc["xyz"], tc["emb"], tc["conf"], tc["pdir"], tc["color"], d["sd"], q, tc["campos"], tc["camrotc2w"], tc["raydir"],
                        tc["bg_color"], tc["c2w_nearest"], tc["campos_nearest"], tc["intrinsic_nearest"], tc["images_nearest"], d["opt"]["vsize"])
    w = ref["blend_weight"][0, ..., 0].double()
    z = ref["sample_loc"][0, ..., 2].double()
    rows = np.nonzero(d["q_ray_mask"])[0]
    dref = np.zeros(len(d["q_ray_mask"]))
    dref[rows] = ((w * z).sum(-1) / (w.sum(-1) + 1e-6)).numpy()
    wsum = np.zeros(len(d["q_ray_mask"]))
    wsum[rows] = w.sum(-1).numpy()
    w2c = torch.inverse(ti["c2w_nearest"][0].cpu()).to(dev)

    def render(want_depth, pad, single):
        rnd.single_call = single
        try:
            o = rnd.render_rays(cloud, ti["raydir"][0], ti["campos"][0], ti["camrotc2w"][0], ti["bg_color"][0], near, far, ti["c2w_nearest"][0],
                                ti["campos_nearest"][0], ti["intrinsic_nearest"][0], ti["images_nearest"][0], w2c_nearest=w2c, pad=pad,
                                want_depth=want_depth)
        finally:
            rnd.single_call = True
        rnd.check_status(o)
        return o

    depths = {}
    for name, pad, single in (("single call", False, True), ("staged padded", True, True), ("staged un-padded", False, False)):
        plain, dep = render(False, pad, single), render(True, pad, single)
        assert "coarse_depth" not in plain
        for k in ("coarse_raycolor", "coarse_point_opacity", "coarse_is_background", "ray_mask"):
            assert torch.equal(plain[k], dep[k]), (name, k)
        np.testing.assert_array_equal(dep["ray_mask"].cpu().numpy(), d["q_ray_mask"])
        got = dep["coarse_depth"].cpu().numpy().astype(np.float64)
        assert got.shape == (len(d["q_ray_mask"]),)
        assert np.all(got[d["q_ray_mask"] == 0] == 0.0), name
        err = np.abs(got - dref)
        print("%s: max |dD| %.2e (%.2e on rays with W >= 0.05), depth range %.3f .. %.3f" % (
            name, err.max(), err[wsum >= 0.05].max(), dref[rows].min(), dref[rows].max()))
        assert err.max() < 1e-3 * max(1.0, np.abs(dref).max()), name
        depths[name] = dep["coarse_depth"]
    assert len(rows) > 100 and np.abs(dref[rows]).max() > 0.1
    # the three paths composite the same blend weights: the same depth bits
    assert torch.equal(depths["single call"], depths["staged padded"])
    assert torch.equal(depths["single call"], depths["staged un-padded"])


def test_depth_of_a_fronto_parallel_plane():
    """A plane of points at camera depth z0: every valid sample has a neighbour within the query radius, so the weighted mean of the samples'
    depths, D (W + 1e-6) / W, lies within that radius of z0 whatever the weights are."""
    from hybridneuralrendering_amd import scenes
    from hybridneuralrendering_amd.aggregator import PointAggregator
    from hybridneuralrendering_amd.render import HybridRenderer, PointCloud
    dev = torch.device("cuda:0")
    sc = scenes.make_scene("scene0241", 1000, 3, w=64, h=48)
    opt = sc.opt
    c2w = sc.c2w
    z0 = 1.5
    assert opt.near_plane < z0 < opt.far_plane
    xs, ys = np.meshgrid(np.arange(-1.0, 1.0, 0.006), np.arange(-0.8, 0.8, 0.006), indexing="ij")      # wider than the view at z0
    cam = np.stack([xs.ravel(), ys.ravel(), np.full(xs.size, z0)], axis=-1)
    xyz = (cam @ c2w[:3, :3].T.astype(np.float64) + c2w[:3, 3]).astype(np.float32)
    nrm = np.repeat(-c2w[:3, 2][None], xyz.shape[0], axis=0).astype(np.float32)
    emb, conf, pdir, color = scenes.point_attributes(nrm, 3, feat_dim=opt.point_features_dim)
    torch.manual_seed(0)
    agg = PointAggregator(opt)
    with torch.no_grad():
        agg.alpha_branch[0].weight.mul_(30.0)
        agg.alpha_branch[0].bias.fill_(30.0)
    agg = agg.to(dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cloud = PointCloud(t(xyz), t(emb), t(conf), t(pdir), t(color))
    rnd = HybridRenderer(opt, agg, dev)
    rays = scenes.camera_rays(scenes.pixel_grid(sc.w, sc.h), sc.intrinsic, c2w)
    out = rnd.render_rays(cloud, t(rays), t(c2w[:3, 3]), t(c2w[:3, :3]), t(sc.bg_color), sc.near, sc.far, t(sc.c2w_nearest), t(sc.c2w_nearest[:, :3, 3]),
                          t(sc.intrinsic), t(sc.images_nearest), want_depth=True)
    rnd.check_status(out)
    radius = float(rnd.querier._grid_for(cloud.xyz[None])[1][0])
    mask = out["ray_mask"].cpu().numpy() > 0
    # the weight sum from a second call that asks for the blend weights (same kernels, same bits)
    W = rnd.render_rays(cloud, t(rays), t(c2w[:3, 3]), t(c2w[:3, :3]), t(sc.bg_color), sc.near, sc.far, t(sc.c2w_nearest), t(sc.c2w_nearest[:, :3, 3]),
                        t(sc.intrinsic), t(sc.images_nearest), want_weights=True)["blend_weight"].double().sum(-1).cpu().numpy()
    D = out["coarse_depth"].double().cpu().numpy()
    hit = mask & (W >= 0.05)
    assert hit.sum() > 0.5 * mask.size, (int(hit.sum()), mask.size)
    mean_z = D[hit] * (W[hit] + 1e-6) / W[hit]
    print("plane at %.3f: %d rays, mean z %.5f .. %.5f, radius %.4f" % (z0, int(hit.sum()), mean_z.min(), mean_z.max(), radius))
    assert np.abs(mean_z - z0).max() <= radius * (1 + 1e-5) + 1e-5
    assert np.all(D[~mask] == 0.0)


# ------------------------------------------------------------------------------------------------ training
def _train_batch():
    """The fresh batch of tests/test_train_gpu.py::test_train_step_matches_oracle_on_a_fresh_batch + a random ground-truth depth."""
    from hybridneuralrendering_amd import scenes
    from oracle import query_oracle as qo
    from tests.test_train_gpu import _setup
    d, ti, opt, agg, path = _setup()
    rng = np.random.default_rng(5)
    patch = 28
    x0, y0 = 20, 9
    px, py = np.meshgrid(np.arange(x0, x0 + patch), np.arange(y0, y0 + patch), indexing="ij")
    pix = np.stack([px, py], axis=-1).reshape(-1, 2).astype(np.int32)
    raydir = scenes.camera_rays(pix, d["intrinsic"], d["c2w"])
    near, far = d["near_far"]
    o = d["opt"]
    tmid = qo.tmid_table(float(near), float(far), o["z_depth_dim"])[None].repeat(raydir.shape[0], 0)
    tmid = (tmid + rng.uniform(-0.3, 0.3, size=tmid.shape) * (far - near) / o["z_depth_dim"] * 0.5).astype(np.float32)
    gt = rng.uniform(0, 1, size=(1, raydir.shape[0], 3)).astype(np.float32)
    gt_depth = rng.uniform(float(near), float(far), size=raydir.shape[0]).astype(np.float32)
    hp = qo.hyperparameters(d["xyz"], o["vsize"], o["vscale"], o["kernel_size"], o["ranges"], o["radius_limit_scale"])
    grid = qo.OracleGrid(d["xyz"], hp["origin"], hp["cell"], hp["dims"], o["query_size"], o["P"], o["max_o"])
    q = grid.query(d["c2w"][:3, 3], raydir, tmid, o["SR"], o["K"], hp["radius2"], o["kernel_size"])
    return d, ti, opt, agg, path, raydir, tmid, gt, gt_depth, q


def _oracle_grads_with_depth(d, q, raydir, gt, gt_depth, dtype):
    """The oracle's render in train mode + autograd of (shipped loss + W_DEPTH * MSE(depth, gt_depth) over the valid rays), composed here from
    oracle.render_oracle's outputs (blend_weight, sample_loc) like its train_step composes the shipped loss."""
    from oracle import render_oracle as ro
    o = d["opt"]
    tc = torch_inputs(d)
    drop = ro.drop_patch_rays(int(o["dilation_setup"].split("_")[1]), int(o["dilation_setup"].split("_")[0]), o["drop_ratio"])
    c = lambda x: x.to(dtype) if isinstance(x, torch.Tensor) and x.is_floating_point() else x
    q = dict(q, sample_loc_w=torch.as_tensor(np.ascontiguousarray(q["sample_loc_w"])).to(dtype))
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        leaves = {k: c(tc[k]).clone().requires_grad_(True) for k in ("emb", "conf", "pdir", "color")}
        sdl = {k: c(v).clone().requires_grad_(True) for k, v in d["sd"].items()}
        out = ro.render(c(tc["xyz"]), leaves["emb"], leaves["conf"], leaves["pdir"], leaves["color"], sdl, q, c(tc["campos"]), c(tc["camrotc2w"]),
                        c(torch.from_numpy(raydir)[None]), c(tc["bg_color"]), c(tc["c2w_nearest"]), c(tc["campos_nearest"]), c(tc["intrinsic_nearest"]),
                        c(tc["images_nearest"]), o["vsize"], 1, is_train=True, drop_ray_rows=drop)
        loss, lc, lz = ro.shipped_loss(out["full_coarse_raycolor"], out["ray_mask"], out["conf_coefficient"], c(torch.from_numpy(gt)),
                                       float(d["zero_epsilon"]))
        w = out["blend_weight"][0, ..., 0]
        D = (w * out["sample_loc"][0, ..., 2]).sum(-1) / (w.sum(-1) + 1e-6)
        rows = torch.from_numpy(np.nonzero(q["ray_mask"])[0])
        ld = torch.nn.functional.mse_loss(D, c(torch.from_numpy(gt_depth))[rows])
        total = loss + W_DEPTH * ld
        total.backward()
    finally:
        torch.set_default_dtype(old)
    grads = {"neural_points.points_embeding": leaves["emb"].grad, "neural_points.points_conf": leaves["conf"].grad,
             "neural_points.points_dir": leaves["pdir"].grad, "neural_points.points_color": leaves["color"].grad}
    for k, v in sdl.items():
        if v.grad is not None:
            grads["aggregator." + k] = v.grad
    return grads, total.item(), ld.item(), D.detach().double().numpy()


def _hip_step(d, ti, agg, path, raydir, tmid, gt, gt_depth, want_depth, depth_in_loss):
    from hybridneuralrendering_amd.train import render_train
    from tests.test_train_gpu import _leaves, _loss
    dev = ti["emb"].device
    near, far = d["near_far"]
    agg.zero_grad(set_to_none=True)
    emb, conf, pdir, color = _leaves(ti)
    out = render_train(path, agg, ti["xyz"], emb, conf, pdir, color, torch.from_numpy(raydir).to(dev), ti["campos"][0], ti["camrotc2w"][0],
                       ti["bg_color"][0], near, far, ti["c2w_nearest"][0], ti["campos_nearest"][0], ti["intrinsic_nearest"][0],
                       ti["images_nearest"][0], tmid=torch.from_numpy(tmid).to(dev), want_depth=want_depth)
    loss, _, _ = _loss(out, torch.from_numpy(gt[0]).to(dev), float(d["zero_epsilon"]))
    ld = None
    if depth_in_loss:
        m = out["ray_mask"] > 0
        ld = torch.nn.functional.mse_loss(out["coarse_depth"][m], torch.from_numpy(gt_depth).to(dev)[m])
        loss = loss + W_DEPTH * ld
    loss.backward()
    got = {"neural_points.points_embeding": emb.grad, "neural_points.points_conf": conf.grad,
           "neural_points.points_dir": pdir.grad, "neural_points.points_color": color.grad}
    for k, prm in agg.named_parameters():
        if prm.grad is not None:
            got["aggregator." + k] = prm.grad.clone()
    return out, loss, ld, got


def test_depth_supervised_training_gradients_match_the_oracle():
    from tests.test_train_gpu import _check_grads, TOL_POINTS
    d, ti, opt, agg, path, raydir, tmid, gt, gt_depth, q = _train_batch()
    ref, total, ld_ref, D_ref = _oracle_grads_with_depth(d, q, raydir, gt, gt_depth, torch.float32)
    out, loss, ld, got = _hip_step(d, ti, agg, path, raydir, tmid, gt, gt_depth, True, True)
    np.testing.assert_array_equal(out["ray_mask"].cpu().numpy(), q["ray_mask"])
    assert out["coarse_depth"].requires_grad and out["coarse_depth"].shape == (raydir.shape[0],)
    rows = np.nonzero(q["ray_mask"])[0]
    D = out["coarse_depth"].detach().double().cpu().numpy()
    assert np.abs(D[rows] - D_ref).max() < 1e-3 * max(1.0, np.abs(D_ref).max())
    np.testing.assert_allclose([loss.item(), ld.item()], [total, ld_ref], rtol=1e-4)
    _check_grads(got, ref, "depth vs oracle", tol_weights=TOL_POINTS)
    ref64, _, _, _ = _oracle_grads_with_depth(d, q, raydir, gt, gt_depth, torch.float64)
    _check_grads(got, ref64, "depth vs fp64", tol_weights=TOL_POINTS)
    # the depth term changed the gradients (a backward that dropped it would not match the references above)
    _, _, _, plain = _hip_step(d, ti, agg, path, raydir, tmid, gt, gt_depth, False, False)
    e = plain["neural_points.points_embeding"]
    assert float((got["neural_points.points_embeding"] - e).abs().max()) > 1e-2 * float(e.abs().max())


# weight gradients the training backward forms with float atomics (alpha branch, last merge-weight layer, final colour
# layer, the reference-view CNN): their last bits depend on the order the atomics land in, which an extra launch in the step can change
ATOMIC_GRADS = ("aggregator.alpha_branch.", "aggregator.aux_merge_weight_block.6.", "aggregator.color_final_block.", "aggregator.aux_block_s")


def test_depth_requested_but_unused_leaves_the_gradients_unchanged():
    """coarse_depth asked for but not in the loss: the backward is the colour-only one (autograd hands the depth no gradient), so the point
    gradients and the order-fixed weight gradients are bit-identical to a run without depth; the float-atomic ones agree to their rounding."""
    d, ti, opt, agg, path, raydir, tmid, gt, gt_depth, q = _train_batch()
    out0, loss0, _, g0 = _hip_step(d, ti, agg, path, raydir, tmid, gt, gt_depth, False, False)
    out1, loss1, _, g1 = _hip_step(d, ti, agg, path, raydir, tmid, gt, gt_depth, True, False)
    assert "coarse_depth" not in out0 and out1["coarse_depth"].requires_grad
    assert torch.equal(out0["coarse_raycolor"], out1["coarse_raycolor"]) and loss0.item() == loss1.item()
    assert set(g0) == set(g1)
    for k in g0:
        if k.startswith(ATOMIC_GRADS):
            np.testing.assert_allclose(g1[k].cpu().numpy(), g0[k].cpu().numpy(), rtol=1e-5, atol=1e-6 * float(g0[k].abs().max()), err_msg=k)
        else:
            np.testing.assert_array_equal(g1[k].cpu().numpy(), g0[k].cpu().numpy(), err_msg=k)


# ------------------------------------------------------------------------------------------------ module and driver
def _depth_net(npts, net, opt):
    from hybridneuralrendering_amd.modules import NeuralPointsRayMarching, find_blend_function, find_render_function, find_tone_map
    return NeuralPointsRayMarching(tonemap_func=find_tone_map("off"), render_func=find_render_function("radiance"),
                                   blend_func=find_blend_function("alpha"), aggregator=net.aggregator, is_compute_depth=True, neural_points=npts,
                                   opt=opt, num_pos_freqs=opt.num_pos_freqs, num_viewdir_freqs=opt.num_viewdir_freqs)


def test_module_emits_coarse_depth_in_eval_and_train():
    import tests.test_modules_gpu as tm
    d, ti, opt, npts, net, dev = tm._build("scannet_small")
    inp = tm._inputs(d, ti, dev)
    rows = np.nonzero(d["q_ray_mask"])[0]
    net_d = _depth_net(npts, net, opt)
    with torch.no_grad():
        plain = net(**inp)
        out = net_d(**inp)
    assert tuple(out["coarse_depth"].shape) == (1, len(rows))
    # weight keeps the aggregator's [1,R',SR,K] (the reference would overwrite it with the blend weight, :383)
    assert torch.equal(out["weight"], plain["weight"]) and out["weight"].dim() == 4
    for k in ("coarse_raycolor", "coarse_point_opacity", "blend_weight", "conf_coefficient"):
        assert torch.equal(out[k], plain[k]), k
    near, far = torch.min(inp["near"]).item(), torch.max(inp["far"]).item()          # as the module reads them
    full = net_d.renderer().render_rays(npts.cloud(), ti["raydir"][0], ti["campos"][0], ti["camrotc2w"][0], ti["bg_color"][0], near, far,
                                        ti["c2w_nearest"][0], ti["campos_nearest"][0], ti["intrinsic_nearest"][0], ti["images_nearest"][0],
                                        want_weights=True, pad=True, want_depth=True)
    assert torch.equal(out["coarse_depth"][0], full["coarse_depth"][torch.from_numpy(rows).to(dev)])

    # train mode: the depth is attached to autograd and a depth loss back-propagates through the HIP backward
    dt = load_train("scannet_small")
    orig = tm.load_render
    tm.load_render = lambda tag: dt
    try:
        d, ti, opt, npts, net, dev = tm._build("scannet_small")
    finally:
        tm.load_render = orig
    assert opt.is_train == 1
    net_d = _depth_net(npts, net, opt)
    net_d.train()
    out = net_d(**tm._inputs(d, ti, dev), tmid=torch.from_numpy(d["tmid"]).to(dev))
    dep = out["coarse_depth"]
    rows = np.nonzero(d["q_ray_mask"])[0]
    assert tuple(dep.shape) == (1, len(rows)) and dep.requires_grad
    loss = torch.nn.functional.mse_loss(dep, torch.full_like(dep, 2.0))
    loss.backward()
    g = npts.points_embeding.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0


def test_render_image_depth():
    from hybridneuralrendering_amd.driver import render_image
    from tests.test_render_gpu import _chunk_loop_frame
    dev = torch.device("cuda:0")
    z, frame, cloud, rnd = _chunk_loop_frame(dev)
    plain = render_image(rnd, cloud, frame)
    got = render_image(rnd, cloud, frame, depth=True)
    chunked = render_image(rnd, cloud, frame, chunk_rays=int(z["chunk"]), depth=True)
    assert "depth" not in plain
    assert torch.equal(plain["image"], got["image"]) and torch.equal(plain["ray_mask"], got["ray_mask"])
    pix = torch.from_numpy(z["pix"]).to(dev).long()
    h, w = got["image"].shape[:2]
    assert tuple(got["depth"].shape) == (h, w)
    assert torch.equal(got["depth"][pix[:, 1], pix[:, 0]], got["coarse_depth"])
    cast = torch.zeros((h, w), dtype=torch.bool, device=dev)
    cast[pix[:, 1], pix[:, 0]] = True
    assert float(got["depth"][~cast].abs().max()) == 0.0
    assert bool((got["coarse_depth"][got["ray_mask"] == 0] == 0).all()) and float(got["coarse_depth"].max()) > 0
    # the per-ray depth is render_rays' (the whole frame is one launch here)
    near, far = float(frame["near"].min()), float(frame["far"].max())
    rr = rnd.render_rays(cloud, frame["raydir"][0], frame["campos"][0], frame["camrotc2w"][0], frame["bg_color"][0], near, far,
                         frame["c2w_nearest"][0], frame["campos_nearest"][0], frame["intrinsic_nearest"][0], frame["images_nearest"][0], want_depth=True)
    assert torch.equal(rr["coarse_depth"], got["coarse_depth"])
    assert float((chunked["coarse_depth"] - got["coarse_depth"]).abs().max()) < 1e-4 * float(got["coarse_depth"].abs().max())
