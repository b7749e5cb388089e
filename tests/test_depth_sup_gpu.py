"""GPU tests of depth supervision (csrc/depth_sup.hip and its wiring): the per-ray gt_depth of frames.BatchSampler bit-equal to the NumPy restatement
tests/depth_sup_ref.py, hnr_depth_loss (value within the derived bound of fp64, gradient bit-equal, sentinels, run-to-run bits, autograd form),
train_step(gt_depth=, w_depth=) against the same launches made by hand and against the fp64 oracle, CapturedTrainStep with gt_depth as a graph
input fed by the sampler, and the depth-error row of a rendered frame alone and inside the test-set evaluator."""
import numpy as np
import pytest
import torch

from tests import depth_sup_ref as R
from tests import frames_ref as FR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 12345.0
F, H, W, HD, WD = 3, 24, 32, 18, 24
K_COLOUR = np.array([[30.0, 0, 15.5], [0, 30.0, 11.5], [0, 0, 1]], np.float32)
K_DEPTH = np.array([[36.3, 0, 10.7], [0, 35.9, 8.2], [0, 0, 1]], np.float32)          # a narrower view: rays in the outer part of the colour frame leave it
_CACHE = {}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _raw_depth(shape, seed):
    """uint16 frames: mostly valid values, and 0, one below depth_min, one above depth_max and 65535 planted all over."""
    rng = np.random.default_rng(seed)
    d = rng.integers(300, 8001, size=shape).astype(np.uint16)
    pick = rng.uniform(size=shape)
    for lo, v in ((0.00, 0), (0.05, 299), (0.10, 8001), (0.15, 65535), (0.20, 40000)):
        d[(pick >= lo) & (pick < lo + 0.05)] = v
    return d


def _bank(kind):
    """kind: "u16" | "f32" | "kd" (18 x 24 depth frames with their own intrinsic) | "none" -> (FrameBank, frames_ref.RefBank, depth frames, kwargs)"""
    from hybridneuralrendering_amd.frames import FrameBank
    if kind in _CACHE:
        return _CACHE[kind]
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, size=(F, H, W, 3)).astype(np.uint8)
    c2w = np.stack([np.eye(4, dtype=np.float32)] * F)
    for f in range(F):
        c2w[f, :3, :3] = np.linalg.qr(rng.normal(size=(3, 3)))[0].astype(np.float32)
        c2w[f, :3, 3] = rng.normal(size=3).astype(np.float32)
    depth, kw = None, {}
    if kind == "u16":
        depth = _raw_depth((F, H, W), 2)
    elif kind == "f32":
        depth = (_raw_depth((F, H, W), 3).astype(np.float32) / np.float32(1000)).astype(np.float32)
    elif kind == "kd":
        depth, kw = _raw_depth((F, HD, WD), 4), dict(depth_intrinsic=K_DEPTH)
    bank = FrameBank(img, c2w, K_COLOUR, DEV, **(dict(depth=depth, **kw) if depth is not None else {}))
    ref = FR.RefBank(img, c2w, K_COLOUR, _np(bank.w2c))
    _CACHE[kind] = (bank, ref, depth, kw)
    return _CACHE[kind]


def _same_item(got, ref, what):
    for k, want in ref.items():
        have = _np(got["camrot" if k == "camrotc2w" and k not in got else k])
        assert have.dtype == want.dtype and have.shape == want.shape and np.array_equal(have, want), (what, k)


def _want_depth(depth, kw, row, pix):
    Kd = kw.get("depth_intrinsic")
    return R.gt_depth(depth, row, pix[:, 0], pix[:, 1], K_COLOUR if Kd is not None else None, Kd)


# ------------------------------------------------------------------------------------------------ lookup
@pytest.mark.parametrize("kind", ["u16", "f32", "kd"])
@pytest.mark.parametrize("mode,shape_kw", [("random", dict(size=12)), ("dilated", dict(dilation_setup="3_4_1_2"))], ids=["random", "dilated"])
def test_gt_depth_follows_the_frame_and_equals_the_restatement(kind, mode, shape_kw):
    """Two consecutive next() calls whose schedule names different frames (144 rays: more than one wave, not a multiple of 64): every old output and
    gt_depth bit-equal to the restatements; gt_depth follows frame_row."""
    from hybridneuralrendering_amd.frames import BatchSampler
    bank, ref, depth, kw = _bank(kind)
    seed, sched = 77, [2, 1]
    s = BatchSampler(bank, mode, margin=1, seed=seed, near=0.1, far=8.0, **shape_kw).set_schedule(sched)
    seen = []
    for step in range(2):
        got = s.next()
        want = FR.batch(ref, sched, mode, seed, step, margin=1, **shape_kw)
        _same_item(got, want, (kind, mode, step))
        assert int(got["frame_row"][0]) == sched[step] and got["gt_depth"].shape == (144,) and got["gt_depth"].dtype == torch.float32
        gd = _np(got["gt_depth"])
        assert np.array_equal(gd, _want_depth(depth, kw, sched[step], want["pixel_idx"])), (kind, mode, step)
        assert (gd > 0).any() and (gd == 0).any()
        seen.append(gd.copy())
    assert not np.array_equal(seen[0], seen[1])
    if kind == "kd":
        _u, _v, inside = R.depth_pixels(want["pixel_idx"][:, 0], want["pixel_idx"][:, 1], HD, WD, K_COLOUR, K_DEPTH)
        assert (~inside).any() and inside.any() and np.all(gd[~inside] == 0)               # rays that map outside the depth frame read 0


@pytest.mark.parametrize("kind", ["u16", "f32", "kd"])
def test_item_gt_depth_for_a_whole_frame_and_for_given_pixels(kind):
    from hybridneuralrendering_amd.frames import BatchSampler
    bank, ref, depth, kw = _bank(kind)
    s = BatchSampler(bank, "random", size=4, margin=0, near=0.1, far=8.0)
    for row in (0, 2):
        got = s.item(row)
        px, py = FR.no_crop_pixels(H, W, 0)
        _same_item(got, FR.item(ref, row, px, py), (kind, row))
        pix = np.stack([px, py], -1).astype(np.float32)
        gd = _np(got["gt_depth"])
        assert gd.shape == (H * W,) and np.array_equal(gd, _want_depth(depth, kw, row, pix))
        if kind != "kd":                                                                     # the whole frame is the depth frame, value rule applied
            assert np.array_equal(gd.reshape(H, W), R.depth_value(depth[row]))
            assert (gd == 0).mean() > 0.2 and gd.max() <= 8.0 and gd[gd > 0].min() >= np.float32(0.3)
    # 130 given pixels: fractional ones truncate, pixels outside the frame read 0
    rng = np.random.default_rng(8)
    pix = np.stack([rng.uniform(-3, W + 3, 130), rng.uniform(-3, H + 3, 130)], -1).astype(np.float32)
    pix[:4] = [[-0.5, 0.0], [0.0, -1.0], [W - 0.25, H - 0.25], [float(W), 3.0]]
    got = s.item(1, pixels=pix)
    gd = _np(got["gt_depth"])
    assert np.array_equal(gd, _want_depth(depth, kw, 1, pix)) and (gd > 0).any()
    if kind != "kd":
        assert gd[1] == 0 and gd[3] == 0 and gd[0] == R.depth_value(depth[1][0:1, 0:1])[0, 0]


def test_a_bank_without_depth_keeps_its_keys_and_its_bits():
    """No depth: the old key set, and next() / item() outputs bit-equal to those of the bank WITH depth (the old three launches are untouched)."""
    from hybridneuralrendering_amd.frames import BatchSampler
    plain, ref, _d, _kw = _bank("none")
    deep = _bank("u16")[0]
    assert plain._dc is None and plain.depth is None
    mk = lambda b: BatchSampler(b, "dilated", dilation_setup="3_4_1_2", margin=1, seed=5, near=0.1, far=8.0, bg_color="random").set_schedule([1, 0, 2])
    a, b = mk(plain), mk(deep)
    for step in range(3):
        x, y = a.next(), b.next()
        assert "gt_depth" not in x and sorted(set(y) - set(x)) == ["gt_depth"]
        assert sorted(x) == sorted(["raydir", "pixel_idx", "gt_image", "campos", "camrot", "camrotc2w", "c2w", "intrinsic", "frame_weight", "bg_color",
                                    "frame_row", "patch_table", "near", "far", "h", "w"])
        _same_item(x, FR.batch(ref, [1, 0, 2], "dilated", 5, step, margin=1, dilation_setup="3_4_1_2", bg="random"), step)
        for k, v in x.items():
            if isinstance(v, torch.Tensor):
                assert torch.equal(v, y[k]), k
    x, y = a.item(2), b.item(2)
    assert "gt_depth" not in x and all(torch.equal(v, y[k]) for k, v in x.items() if isinstance(v, torch.Tensor))
    # out= with gt_depth on a bank without depth: the key is not an output there, nothing is written
    g = torch.full((144,), SENTINEL, device=DEV)
    a.next(out=dict(gt_depth=g))
    assert bool((g == SENTINEL).all())


def test_next_out_writes_gt_depth_from_the_samplers_own_row_and_pixels():
    """out holds gt_depth but neither frame_row nor pixel_idx: the sampler binds its own; only the given tensors are written; capturable."""
    from hybridneuralrendering_amd.frames import BatchSampler
    bank, ref, depth, kw = _bank("kd")
    mk = lambda: BatchSampler(bank, "random", size=12, margin=1, seed=31, near=0.1, far=8.0).set_schedule([0, 2, 1])
    s = mk()
    buf = torch.full((144 + 128,), SENTINEL, device=DEV)
    out = dict(gt_depth=buf[64:64 + 144], gt_image=torch.empty((144, 3), device=DEV))
    dev = torch.device(DEV)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        assert s.next(out=out) is out                                                       # step 0: warm-up, binds the tensors
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    want = FR.batch(ref, [0, 2, 1], "random", 31, 0, margin=1, size=12)
    assert np.array_equal(_np(out["gt_depth"]), _want_depth(depth, kw, 0, want["pixel_idx"])) and np.array_equal(_np(out["gt_image"]), want["gt_image"])
    assert bool((buf[:64] == SENTINEL).all()) and bool((buf[64 + 144:] == SENTINEL).all())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        s.next(out=out)
    for step in (1, 2, 3):
        graph.replay()
        torch.cuda.synchronize()
        want = FR.batch(ref, [0, 2, 1], "random", 31, step, margin=1, size=12)
        assert np.array_equal(_np(out["gt_depth"]), _want_depth(depth, kw, [0, 2, 1][step % 3], want["pixel_idx"])), step
    assert int(s.step.item()) == 4


# ------------------------------------------------------------------------------------------------ loss
def _loss_case(n, pattern, seed):
    rng = np.random.default_rng(seed)
    D = rng.uniform(0.2, 6.0, size=n).astype(np.float32)
    gt = (D + rng.normal(0, 0.3, size=n)).astype(np.float32).clip(0.31, 7.9)
    mask = (rng.uniform(size=n) > 0.2).astype(np.int8)
    if pattern == "mixed":
        gt[rng.uniform(size=n) < 0.3] = 0.0
        if n == 1:
            mask[:], gt[:] = 1, 2.5
    elif pattern == "none":
        gt[mask > 0] = 0.0
    else:
        mask[:] = 1
    return D, gt, mask


def _padded(n, dtype=torch.float32, pad=64):
    big = torch.full((n + 2 * pad,), SENTINEL, dtype=dtype, device=DEV)
    return big, big[pad:pad + n]


def _intact(big, n, pad=64):
    return bool((big[:pad] == SENTINEL).all()) and bool((big[pad + n:] == SENTINEL).all())


def _raw_loss(D, gt, mask, w, total0):
    from hybridneuralrendering_amd import _lib
    L = _lib.lib()
    n = len(D)
    tD, tg, tm = _t(D), _t(gt), _t(mask)
    b_out, out3 = _padded(3)
    b_g, g = _padded(n)
    b_tot, tot = _padded(4)
    tot[:] = torch.tensor([total0, 1.0, 2.0, 3.0], device=DEV)
    P = _lib.ptr
    _lib.check(L.hnr_depth_loss(P(tD), P(tg), P(tm), n, float(w), P(tot), P(out3), P(g), None, _lib.stream()), "hnr_depth_loss")
    torch.cuda.synchronize()
    assert _intact(b_out, 3) and _intact(b_g, n) and _intact(b_tot, 4)
    assert _np(tot)[1:].tolist() == [1.0, 2.0, 3.0]                                          # only the first word of the total is touched
    return _np(out3).copy(), _np(g).copy(), _np(tot)[0].copy()


@pytest.mark.parametrize("pattern", ["none", "all", "mixed"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 3136, 70000])
def test_depth_loss_value_gradient_and_total(n, pattern):
    from hybridneuralrendering_amd import losses
    D, gt, mask = _loss_case(n, pattern, n + len(pattern))
    w, total0 = 0.1, np.float32(0.75)
    out3, g, tot = _raw_loss(D, gt, mask, w, total0)
    r_out3, r_g, r_tot = R.depth_loss(D, gt, mask, w, total=total0)
    m = R.loss_mask(gt, mask)
    cnt, L64 = int(m.sum()), R.depth_loss_fp64(D, gt, mask)
    print("R %d %s: n %d  L %.9g  fp64 %.9g  rel err %.2e (bound %.2e)  bits equal the restatement: %s" % (
        n, pattern, cnt, out3[0], L64, abs(float(out3[0]) - L64) / L64 if L64 else 0.0, R.LOSS_REL_BOUND, out3[0] == r_out3[0]))
    assert out3[1] == cnt
    assert g.tobytes() == r_g.tobytes()                                                      # the gradient, bit for bit
    assert abs(float(out3[0]) - L64) <= R.LOSS_REL_BOUND * L64
    assert out3[2] == np.float32(np.float32(w) * out3[0])
    if cnt == 0:
        assert pattern == "none" and not out3.any() and not g.any() and tot.tobytes() == total0.tobytes()      # the total's bits stay
    else:
        assert tot == np.float32(total0 + out3[2]) and np.all(g[~m] == 0) and g[m].any()
    out3b, gb, totb = _raw_loss(D, gt, mask, w, total0)
    assert out3b.tobytes() == out3.tobytes() and gb.tobytes() == g.tobytes() and totb.tobytes() == tot.tobytes()      # two runs, the same bits
    # the Python forms: value only, raw, and under autograd
    o3, none = losses.depth_loss_grads(_t(D), _t(gt), _t(mask), w, want_grad=False)
    assert none is None and _np(o3).tobytes() == out3.tobytes()
    Dt = _t(D).requires_grad_(True)
    term, o3 = losses.depth_loss(Dt, _t(gt), _t(mask), w)
    term.backward()
    assert _np(term) == out3[2] and _np(o3).tobytes() == out3.tobytes() and _np(Dt.grad).tobytes() == g.tobytes()


# ------------------------------------------------------------------------------------------------ the fused step
def _step_batch():
    if "step" not in _CACHE:
        from tests.test_depth_gpu import _train_batch
        d, ti, opt, agg, path, raydir, tmid, gt, gt_depth, q = _train_batch()
        gt_depth = gt_depth.copy()
        gt_depth[::3] = 0.0                                                                  # a third of the rays carry no measurement
        _CACHE["step"] = (d, ti, opt, agg, path, raydir, tmid, gt, gt_depth, q)
    return _CACHE["step"]


def _oracle_grads_masked_depth(d, q, raydir, gt, gt_depth, w_depth, dtype):
    """tests/test_depth_gpu.py::_oracle_grads_with_depth with the depth term of this feature: the mean over the valid rays WITH a measurement."""
    from oracle import render_oracle as ro
    from tests.golden_io import torch_inputs
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
        gd = c(torch.from_numpy(gt_depth))[rows]
        has = gd > 0
        ld = ((D - gd)[has] ** 2).mean()
        total = loss + w_depth * ld
        total.backward()
    finally:
        torch.set_default_dtype(old)
    grads = {"neural_points.points_embeding": leaves["emb"].grad, "neural_points.points_conf": leaves["conf"].grad,
             "neural_points.points_dir": leaves["pdir"].grad, "neural_points.points_color": leaves["color"].grad}
    for k, v in sdl.items():
        if v.grad is not None:
            grads["aggregator." + k] = v.grad
    return grads, total.item(), ld.item(), int(has.sum())


def _fused(extra):
    from hybridneuralrendering_amd.train import train_step
    from tests.test_train_gpu import _leaves
    d, ti, opt, agg, path, raydir, tmid, gt, gt_depth, q = _step_batch()
    near, far = d["near_far"]
    emb, conf, pdir, color = _leaves(ti)
    return train_step(path, agg, ti["xyz"], emb, conf, pdir, color, _t(raydir), ti["campos"][0], ti["camrotc2w"][0], ti["bg_color"][0], near, far,
                      ti["c2w_nearest"][0], ti["campos_nearest"][0], ti["intrinsic_nearest"][0], ti["images_nearest"][0], _t(gt[0]),
                      zero_epsilon=float(d["zero_epsilon"]), tmid=_t(tmid), assign_grads=False, **extra)


def _by_hand(w_depth):
    """The launches of the depth step, one by one"""
    from hybridneuralrendering_amd import _lib
    from hybridneuralrendering_amd.losses import shipped_loss_grads
    from hybridneuralrendering_amd.render import PointCloud
    d, ti, opt, agg, path, raydir, tmid, gt, gt_depth, q = _step_batch()
    near, far = d["near_far"]
    cloud = PointCloud(ti["xyz"], ti["emb"], ti["conf"], ti["pdir"], ti["color"])
    out, S = path.forward(cloud, _t(raydir), ti["campos"][0], ti["camrotc2w"][0], ti["bg_color"][0], near, far, ti["c2w_nearest"][0],
                          ti["campos_nearest"][0], ti["intrinsic_nearest"][0], ti["images_nearest"][0], tmid=_t(tmid), want_depth=True)
    parts, g_col, g_cc = shipped_loss_grads(out["coarse_raycolor"], out["conf_coefficient"], _t(gt[0]), out["ray_mask"], float(d["zero_epsilon"]), 1.0, 1e-4,
                                            None, conf_rows=True)
    parts0 = parts.clone()
    R_ = raydir.shape[0]
    out3, g_depth = torch.empty(3, device=DEV), torch.empty(R_, device=DEV)
    P = _lib.ptr
    _lib.check(_lib.lib().hnr_depth_loss(P(out["coarse_depth"]), P(_t(gt_depth)), P(out["ray_mask"]), R_, float(w_depth), P(parts), P(out3), P(g_depth),
                                         None, _lib.stream()), "hnr_depth_loss")
    pg, ag = path.backward(S, g_col, g_cc, g_depth)
    return out, parts0, parts, out3, pg, ag


def _grads_equal(pg, ag, pg2, ag2, what):
    from tests.test_depth_gpu import ATOMIC_GRADS
    assert set(pg) == set(pg2) and set(ag) == set(ag2)
    for k in pg:
        assert torch.equal(pg[k], pg2[k]), (what, k)
    for k in ag:
        if ("aggregator." + k).startswith(ATOMIC_GRADS):                                    # float-atomic weight gradients: the allowance of test_depth_gpu.py
            np.testing.assert_allclose(_np(ag2[k]), _np(ag[k]), rtol=1e-5, atol=1e-6 * float(ag[k].abs().max()), err_msg="%s %s" % (what, k))
        else:
            assert torch.equal(ag[k], ag2[k]), (what, k)


def test_train_step_with_depth_equals_the_launches_made_by_hand_and_the_fp64_oracle():
    from tests.test_depth_gpu import W_DEPTH
    from tests.test_train_gpu import _check_grads, TOL_POINTS
    d, ti, opt, agg, path, raydir, tmid, gt, gt_depth, q = _step_batch()
    out, pg, ag = _fused(dict(gt_depth=_t(gt_depth), w_depth=W_DEPTH))
    pg, ag = {k: v.clone() for k, v in pg.items()}, {k: v.clone() for k, v in ag.items()}
    h_out, parts0, parts, out3, h_pg, h_ag = _by_hand(W_DEPTH)
    np.testing.assert_array_equal(_np(out["ray_mask"]), q["ray_mask"])
    assert torch.equal(out["coarse_depth"], h_out["coarse_depth"]) and torch.equal(out["coarse_raycolor"], h_out["coarse_raycolor"])
    assert torch.equal(out["loss"], parts) and torch.equal(out["loss_depth"], out3) and out["loss"].shape == (4,) and out["loss_depth"].shape == (3,)
    n_expected = int(((q["ray_mask"] > 0) & (gt_depth > 0)).sum())
    assert int(out3[1]) == n_expected and 0 < n_expected < int((q["ray_mask"] > 0).sum())
    # total = the shipped total + w L, one fp32 add on the device; the other three entries are the shipped kernels'
    assert _np(parts)[0] == np.float32(_np(parts0)[0] + _np(out3)[2]) and torch.equal(parts[1:], parts0[1:]) and float(out3[2]) > 0
    _grads_equal(pg, ag, h_pg, h_ag, "fused vs by hand")
    # ... and the depth term of the restatement on the step's own depth
    r_out3, r_g, _ = R.depth_loss(_np(out["coarse_depth"]), gt_depth, _np(out["ray_mask"]), W_DEPTH)
    assert r_out3[1] == n_expected and abs(float(_np(out3)[0]) - float(r_out3[0])) <= 2 * R.LOSS_REL_BOUND * float(r_out3[0])
    # the fp64 oracle with the same masked mean, tolerances of tests/test_depth_gpu.py
    ref64, total64, ld64, n64 = _oracle_grads_masked_depth(d, q, raydir, gt, gt_depth, W_DEPTH, torch.float64)
    assert n64 == n_expected
    print("total %.8g (fp64 %.8g)  depth term %.8g (fp64 %.8g)" % (float(out["loss"][0]), total64, float(out3[0]), ld64))
    np.testing.assert_allclose([float(out["loss"][0]), float(out3[0])], [total64, ld64], rtol=1e-3)     # (the depth tolerance of tests/test_depth_gpu.py)
    got = {"neural_points.points_" + k.split("_", 1)[1]: v for k, v in pg.items()}
    got.update({"aggregator." + k: v for k, v in ag.items()})
    _check_grads(got, ref64, "depth step vs fp64", tol_weights=TOL_POINTS)
    # the term acts: the embedding gradient moves by more than 1 % of its maximum
    _o, pg0, _ag0 = _fused({})
    e = pg0["points_embeding"]
    assert float((pg["points_embeding"] - e).abs().max()) > 1e-2 * float(e.abs().max())


def test_train_step_without_depth_is_the_old_step_and_bad_arguments_raise():
    from hybridneuralrendering_amd._lib import HnrError
    d, ti, opt, agg, path, raydir, tmid, gt, gt_depth, q = _step_batch()
    out0, pg0, ag0 = _fused({})
    pg0, ag0 = {k: v.clone() for k, v in pg0.items()}, {k: v.clone() for k, v in ag0.items()}
    out1, pg1, ag1 = _fused(dict(gt_depth=None, w_depth=0.0))
    assert "coarse_depth" not in out0 and "loss_depth" not in out0 and sorted(out0) == sorted(out1)
    for k in ("loss", "coarse_raycolor", "conf_coefficient", "ray_mask"):
        assert torch.equal(out0[k], out1[k]), k
    _grads_equal(pg0, ag0, pg1, ag1, "gt_depth=None")
    n = raydir.shape[0]
    for extra in (dict(w_depth=0.1), dict(gt_depth=torch.from_numpy(gt_depth), w_depth=0.1), dict(gt_depth=_t(gt_depth[:n - 1]), w_depth=0.1),
                  dict(gt_depth=_t(gt_depth), w_depth=-1.0), dict(gt_depth=_t(gt_depth).double(), w_depth=0.1)):
        with pytest.raises(HnrError):
            _fused(extra)


# ------------------------------------------------------------------------------------------------ captured
def _scene_bank(d, ti):
    """Five frames of the golden scene's camera and frame size with depth, V = 4 reference views: what a sampler needs to fill cap.inputs."""
    from hybridneuralrendering_amd.frames import FrameBank
    rng = np.random.default_rng(12)
    V, h, w = (int(s) for s in ti["images_nearest"][0].shape[:3])
    n = 5
    img = rng.integers(0, 256, size=(n, h, w, 3)).astype(np.uint8)
    c2w = np.stack([d["c2w"].astype(np.float32)] * n)
    near, far = d["near_far"]
    depth = rng.integers(int(near * 1000) + 1, int(far * 1000), size=(n, h, w)).astype(np.uint16)
    depth[rng.uniform(size=depth.shape) < 0.25] = 0
    bank = FrameBank(img, c2w, d["intrinsic"], DEV, depth=depth, depth_min=float(near), depth_max=float(far))
    bank.set_nearest(np.stack([rng.permutation(n)[:V] for _ in range(n)]).astype(np.int32))
    return bank, depth


def test_captured_step_with_depth_and_the_optimizer_against_eager_steps():
    """CapturedTrainStep with gt_depth in the sample and a DeviceAdam: two replays with two gt_depth inputs against two eager
    train_step(optimizer=) calls from the same start -- after each step every parameter equals the Adam restatement applied to the step's own
    gradients (tests/test_device_adam_gpu.py's comparison), the first steps agree bit for bit in loss, depth and point gradients (the same
    parameters), and the depth term follows its input.  Then sampler.next(out=cap.inputs); cap.step() as a whole iteration."""
    from hybridneuralrendering_amd.train import CapturedTrainStep, train_step
    from hybridneuralrendering_amd.frames import BatchSampler
    from hybridneuralrendering_amd._lib import HnrError
    from tests.test_device_adam_gpu import _train_scene, _Mirror
    from tests.test_depth_gpu import W_DEPTH
    rng = np.random.default_rng(3)
    res = {}
    for form in ("eager", "captured"):
        d, ti, opt, agg, path, leaves, named, optim, near, far, gt, kw = _train_scene()
        emb, conf, pdir, color = leaves.values()
        n = int(ti["raydir"][0].shape[0])
        if "gd" not in res:
            res["gd"] = [_t(np.where(rng.uniform(size=n) < 0.3, 0.0, rng.uniform(near, far, size=n)).astype(np.float32)) for _ in range(2)]
        mirror = _Mirror(named, leaves)
        steps = []
        if form == "eager":
            for i in range(2):
                out, pg, ag = train_step(path, agg, ti["xyz"], emb, conf, pdir, color, ti["raydir"][0], ti["campos"][0], ti["camrotc2w"][0], ti["bg_color"][0],
                                         near, far, ti["c2w_nearest"][0], ti["campos_nearest"][0], ti["intrinsic_nearest"][0], ti["images_nearest"][0], gt,
                                         optimizer=optim, gt_depth=res["gd"][i], w_depth=W_DEPTH, **kw)
                mirror.advance(optim, pg, ag, "eager depth step %d" % i)
                steps.append((out["loss"].clone(), out["loss_depth"].clone(), out["coarse_depth"].clone(), pg["points_embeding"].clone()))
        else:
            sample = dict(raydir=ti["raydir"][0], campos=ti["campos"][0], camrot=ti["camrotc2w"][0], bg_color=ti["bg_color"][0],
                          c2w_nearest=ti["c2w_nearest"][0], campos_nearest=ti["campos_nearest"][0], intrinsic_nearest=ti["intrinsic_nearest"][0],
                          images_nearest=ti["images_nearest"][0], gt_image=gt, tmid=kw["tmid"], gt_depth=res["gd"][0])
            with pytest.raises(HnrError):                                                    # a weight, but no depth in the sample
                CapturedTrainStep(path, agg, ti["xyz"], emb, conf, pdir, color, {k: v for k, v in sample.items() if k != "gt_depth"}, near, far,
                                  zero_epsilon=kw["zero_epsilon"], optimizer=optim, w_depth=W_DEPTH)
            cap = CapturedTrainStep(path, agg, ti["xyz"], emb, conf, pdir, color, sample, near, far, zero_epsilon=kw["zero_epsilon"], optimizer=optim,
                                    w_depth=W_DEPTH)
            torch.cuda.synchronize()
            assert optim.counters() == (0, 1000) and "gt_depth" in cap.inputs
            for i in range(2):
                out, pg, ag = cap.step(gt_depth=res["gd"][i])
                torch.cuda.synchronize()
                mirror.advance(optim, pg, ag, "replay %d" % i)
                steps.append((out["loss"].clone(), out["loss_depth"].clone(), out["coarse_depth"].clone(), pg["points_embeding"].clone()))
            assert optim.counters() == (2, 1002)
            # the sampler feeds the captured step in place: gt_depth lands in cap.inputs with no other copy
            bank, depth = _scene_bank(d, ti)
            s = BatchSampler(bank, "random", size=int(round(n ** 0.5)), margin=2, seed=9, near=near, far=far).set_schedule([3, 1])
            assert s.R == n
            ptr = cap.inputs["gt_depth"].data_ptr()
            assert s.next(out=cap.inputs) is cap.inputs and cap.inputs["gt_depth"].data_ptr() == ptr
            pix = _np(s._own[("pixel_idx", n)])
            want = R.gt_depth(depth, 3, pix[:, 0], pix[:, 1], depth_min=float(near), depth_max=float(far))
            assert np.array_equal(_np(cap.inputs["gt_depth"]), want) and (want > 0).any() and (want == 0).any()
            out, pg, ag = cap.step()
            torch.cuda.synchronize()
            assert optim.counters() == (3, 1003) and bool(torch.isfinite(out["loss"]).all())
            m = R.loss_mask(want, _np(out["ray_mask"]))
            assert int(out["loss_depth"][1]) == int(m.sum())
        res[form] = steps
    e, c = res["eager"], res["captured"]
    for k in range(4):                                                                       # step 0: the same parameters, the same bits
        assert torch.equal(e[0][k], c[0][k]), k
    assert float(e[0][1][1]) > 0 and not torch.equal(e[0][1], e[1][1])
    # step 1 starts from parameters that differ in the float-atomic gradients' last bits
    np.testing.assert_allclose(_np(c[1][1]), _np(e[1][1]), rtol=1e-4)
    np.testing.assert_allclose(_np(c[1][0]), _np(e[1][0]), rtol=1e-4)


# ------------------------------------------------------------------------------------------------ metrics
def test_depth_metrics_row_of_one_frame():
    from hybridneuralrendering_amd.metrics import depth_frame_metrics, derive_depth, DM_NCOLS
    rng = np.random.default_rng(21)
    n = 24 * 32
    D = rng.uniform(0.2, 6.0, size=n).astype(np.float32)
    gt = (D * rng.uniform(0.6, 1.5, size=n)).astype(np.float32)
    gt[rng.uniform(size=n) < 0.3] = 0.0
    mask = (rng.uniform(size=n) > 0.2).astype(np.int8)
    D[mask == 0] = 0.0
    D[7], mask[7], gt[7] = 0.0, 1, 2.0                                                       # a hit whose depth is 0: counted, never inside delta
    table = torch.full((3, DM_NCOLS), SENTINEL, dtype=torch.float64, device=DEV)
    out = depth_frame_metrics(dict(coarse_depth=_t(D), ray_mask=_t(mask)), dict(gt_depth=_t(gt)[None]), out=table, row=1)
    row = _np(out)[1]
    assert (_np(out)[0] == SENTINEL).all() and (_np(out)[2] == SENTINEL).all()
    m = (mask > 0) & (gt > 0)
    D64, d64 = D.astype(np.float64)[m], gt.astype(np.float64)[m]
    e = np.abs(D64 - d64)
    with np.errstate(divide="ignore"):
        delta = np.maximum(D64 / d64, d64 / D64)
    assert row[0] == m.sum() and row[4] == (delta < 1.25).sum() and 0 < row[4] < row[0]
    np.testing.assert_allclose(row[1:4], [e.sum(), (e * e).sum(), (e / d64).sum()], rtol=1e-12, atol=0)
    want = R.depth_metrics(D, gt, mask)                                                      # the restatement has the kernel's order: the same bits
    assert np.array_equal(row[[0, 1, 2, 4]], want[[0, 1, 2, 4]])
    np.testing.assert_allclose(row[3], want[3], rtol=1e-14)                                  # (its terms are quotients: one rounding each, whoever divides)
    again = _np(depth_frame_metrics(dict(coarse_depth=_t(D), ray_mask=_t(mask)), dict(gt_depth=_t(gt))))[0]
    assert again.tobytes() == row.tobytes()
    dd = derive_depth(row)
    np.testing.assert_allclose([dd["depth_abs"][0], dd["depth_rmse"][0], dd["depth_absrel"][0], dd["depth_d1"][0]],
                               [e.mean(), np.sqrt((e * e).mean()), (e / d64).mean(), (delta < 1.25).mean()], rtol=1e-12)
    # nothing to compare: zeros, and NaN means
    none = _np(depth_frame_metrics(dict(coarse_depth=_t(D), ray_mask=_t(mask)), dict(gt_depth=_t(np.zeros_like(gt)))))[0]
    assert not none.any() and np.isnan(derive_depth(none)["depth_rmse"][0])


def test_evaluator_depth_rows_equal_single_calls_and_leave_the_rest_alone():
    from hybridneuralrendering_amd.driver import evaluate_frames
    from hybridneuralrendering_amd.metrics import depth_frame_metrics
    from hybridneuralrendering_amd._lib import HnrError
    from tests.test_metrics_gpu import _golden_frame
    z, frame, cloud, rnd, gt, pix = _golden_frame(11)
    rng = np.random.default_rng(4)
    n = gt.shape[0]
    gds = []
    for _ in range(2):
        gd = rng.uniform(0.5, 4.0, size=n).astype(np.float32)
        gd[rng.uniform(size=n) < 0.3] = 0.0
        gds.append(gd)
    frames = [dict(frame, gt_depth=_t(gd)[None]) for gd in gds]
    seen, seen_d = [], []
    ev0 = evaluate_frames(rnd, cloud, frames, on_frame=lambda i, o: seen.append(o))
    ev1 = evaluate_frames(rnd, cloud, frames, on_frame=lambda i, o: seen_d.append(o), depth=True)
    for o, od in zip(seen, seen_d):
        assert sorted(set(od) - set(o)) == ["coarse_depth", "depth"]
        for k in o:
            assert torch.equal(o[k], od[k]), k                                               # image, colours, mask: bit-equal
    assert ev0.table.cpu().numpy().tobytes() == ev1.table.cpu().numpy().tobytes() and ev1.n == 2 and ev0.depth_table is None
    for i, (od, fr) in enumerate(zip(seen_d, frames)):
        single = _np(depth_frame_metrics(od, fr))[0]
        assert _np(ev1.depth_table)[i].tobytes() == single.tobytes()
        want = R.depth_metrics(_np(od["coarse_depth"]), gds[i], _np(od["ray_mask"]))
        assert np.array_equal(single[[0, 1, 2, 4]], want[[0, 1, 2, 4]]) and abs(single[3] - want[3]) <= 1e-14 * want[3]
    s0, s1 = ev0.summary(), ev1.summary()
    assert sorted(set(s1) - set(s0)) == ["depth_abs", "depth_absrel", "depth_d1", "depth_n", "depth_rmse"]
    for k in s0:
        if k != "mean":
            assert np.array_equal(s0[k], s1[k], equal_nan=True), k
    assert (s1["depth_n"] > 0).all() and (s1["depth_rmse"] > 0).all() and s1["depth_abs"][0] != s1["depth_abs"][1]
    assert s1["mean"]["depth_rmse"] == float(np.mean(s1["depth_rmse"]))
    with pytest.raises(HnrError):
        evaluate_frames(rnd, cloud, [frame], depth=True)                                     # no gt_depth in the frame
