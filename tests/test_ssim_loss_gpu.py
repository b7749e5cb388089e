"""GPU tests of the patch SSIM term (csrc/ssim_loss.hip and its wiring).

hnr_ssim_loss against the fp64 restatement tests/ssim_loss_ref.py on the smallest shapes at which each code path can go wrong -- L, SSIM and the
gradient within 4 x max(the fp32 restatement's own error, 2^-24 of the largest magnitude), exact hit counts, accumulate = written + base bit for
bit, sentinels, run-to-run bits, the total with a host and a device frame weight, the Python forms -- and train_step(w_ssim=) against the same
launches made by hand, against render_train + the torch-autograd forms of the losses, with w_ssim = 0, and captured in a graph.

Every figure is printed as an `SSIM_RATIO` line before it is asserted (profiles/ssim_loss_tests.txt is those lines of one run)."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import ssim_loss_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 12345.0
W_SSIM, FW, TOTAL0 = 0.2, 0.7, 0.75
PAD = 64
_WORLD = {}


def _np(t):
    return t.detach().cpu().numpy()


def _padded(shape, fill=None):
    n = int(np.prod(shape))
    big = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float32, device=DEV)
    view = big[PAD:PAD + n].view(*shape)
    if fill is not None:
        view.copy_(fill)
    return big, view


def _intact(big):
    return bool((big[:PAD] == SENTINEL).all()) and bool((big[-PAD:] == SENTINEL).all())


def _raw(c, g, m, pn, ps, layout, w=W_SSIM, fw=FW, device_fw=False, norm=0, base=None, total0=TOTAL0):
    """One hnr_ssim_loss call through ctypes into guarded buffers -> (out4, gradient buffer, total[4]) as NumPy copies."""
    from hybridneuralrendering_amd import _lib
    L = _lib.lib()
    n = R.n_patches(pn, layout)
    b_out, out4 = _padded((4,))
    b_g, grad = _padded(tuple(c.shape), fill=base)
    b_tot, tot = _padded((4,), fill=torch.tensor([total0, 1.0, 2.0, 3.0]))
    scratch = torch.full((2 * n + 2 * PAD,), SENTINEL, dtype=torch.float64, device=DEV)
    dfw = torch.tensor([fw], dtype=torch.float32, device=DEV) if device_fw else None
    win = (ctypes.c_float * 7)(*[float(v) for v in R.window()])
    P = _lib.ptr
    _lib.check(L.hnr_ssim_loss(P(c), P(g), P(m), -pn if layout == "patch_major" else pn, ps, norm, win, w, 1.0 if device_fw else fw, P(dfw), P(tot), P(out4),
                               P(grad), int(base is not None), P(scratch[PAD:PAD + 2 * n]), _lib.stream()), "hnr_ssim_loss")
    torch.cuda.synchronize()
    assert _intact(b_out) and _intact(b_g) and _intact(b_tot) and _intact(scratch)
    t = _np(tot).copy()
    assert t[1:].tolist() == [1.0, 2.0, 3.0]                                # only the first word of the total is touched
    return _np(out4).copy(), _np(grad).copy(), t[0]


def _check_case(pn, ps, layout, mask_kind, constant_patch=False):
    from hybridneuralrendering_amd import losses
    c, g, m = (t.to(DEV) for t in R.make_case(pn, ps, layout, mask_kind, constant_patch))
    r64, r32 = R.references(pn, ps, layout, mask_kind, W_SSIM, FW, constant_patch)
    out4, grad, tot = _raw(c, g, m, pn, ps, layout)
    tag = "%dx%d %s %s%s" % (pn, ps, layout, mask_kind, " constant" if constant_patch else "")
    mask = R.np32(R.make_case(pn, ps, layout, mask_kind, constant_patch)[2]) > 0
    # value and gradient against fp64, within 4 x the fp32 restatement's own error (floor: 2^-24 of the largest magnitude)
    figures = []
    for name, got, k in (("L", out4[0], "L"), ("SSIM", out4[1], "ssim"), ("grad", grad, "grad")):
        want = R.np32(r64[k]).astype(np.float64)
        e_new = float(np.abs(np.asarray(got, np.float64) - want).max())
        e_ref = float(np.abs(R.np32(r32[k]).astype(np.float64) - want).max())
        scale = float(np.abs(want).max())
        b = R.bound(e_ref, scale)
        print("SSIM_RATIO %s %s: |fp64| %.4e  device off by %.3e  fp32 restatement off by %.3e  bound %.3e  ratio %.2f" % (
            tag, name, scale, e_new, e_ref, b, e_new / (b / 4) if b > 0 else 0.0))
        figures.append((name, e_new, b))
    for name, e_new, b in figures:
        assert e_new <= b, (tag, name, e_new, b)
    assert out4[3] == r64["hits"] == int(mask.sum())                        # the hit-ray count, exactly
    assert out4[2] == np.float32(np.float32(np.float32(FW) * np.float32(W_SSIM)) * out4[0])
    assert not grad[~mask].any()                                            # exactly 0 on missed rays
    if r64["hits"] == 0:
        assert out4[0] == 0 and out4[2] == 0 and not grad.any() and tot.tobytes() == np.float32(TOTAL0).tobytes()
    else:
        assert tot == np.float32(np.float32(TOTAL0) + out4[2]) and grad.any() and 0 < out4[0] < 1
    # two runs, the same bits
    out4b, gradb, totb = _raw(c, g, m, pn, ps, layout)
    assert out4b.tobytes() == out4.tobytes() and gradb.tobytes() == grad.tobytes() and totb.tobytes() == tot.tobytes()
    # the device frame weight: the same bits
    out4d, gradd, totd = _raw(c, g, m, pn, ps, layout, device_fw=True)
    assert out4d.tobytes() == out4.tobytes() and gradd.tobytes() == grad.tobytes() and totd.tobytes() == tot.tobytes()
    # accumulate = the base buffer + the written gradient, one fp32 add per element
    base = torch.randn(tuple(c.shape), generator=torch.Generator().manual_seed(ps), dtype=torch.float32).to(DEV)
    out4a, acc, _tot = _raw(c, g, m, pn, ps, layout, base=base)
    want = _np(base + torch.from_numpy(grad).to(DEV))
    assert out4a.tobytes() == out4.tobytes() and acc.tobytes() == want.tobytes()
    # the Python forms: graph-free (written, accumulated, value only) and under autograd
    kw = dict(layout=layout, frame_weight=FW)
    o4, gp = losses.ssim_patch_loss_grads(c, g, m, pn, ps, W_SSIM, **kw)
    assert _np(o4).tobytes() == out4.tobytes() and _np(gp).tobytes() == grad.tobytes()
    buf, parts = base.clone(), torch.tensor([TOTAL0, 1.0, 2.0, 3.0], device=DEV)
    o4, gq = losses.ssim_patch_loss_grads(c, g, m, pn, ps, W_SSIM, device_frame_weight=torch.tensor([FW], device=DEV), total=parts, g_color=buf, layout=layout)
    assert gq is buf and _np(buf).tobytes() == want.tobytes() and _np(parts)[0] == tot and _np(o4).tobytes() == out4.tobytes()
    o4, none = losses.ssim_patch_loss_grads(c, g, m, pn, ps, W_SSIM, want_grad=False, **kw)
    assert none is None and _np(o4).tobytes() == out4.tobytes()
    x = c.clone().requires_grad_(True)
    term, o4 = losses.ssim_patch_loss(x, g, m, pn, ps, W_SSIM, **kw)
    term.backward()
    assert _np(term) == out4[2] and _np(o4).tobytes() == out4.tobytes() and _np(x.grad).tobytes() == grad.tobytes()


@pytest.mark.parametrize("mask_kind", R.MASKS)
@pytest.mark.parametrize("pn,ps,layout", R.SHAPES, ids=["%dx%d-%s" % s for s in R.SHAPES])
def test_ssim_loss_value_gradient_and_total(pn, ps, layout, mask_kind):
    """Measured on one MI355X (profiles/ssim_loss_tests.txt): in every case the device's L, SSIM and gradient are off from fp64 by exactly what the
    fp32 restatement is off by (largest: L 2.5e-6, for the single window of 1 x 7; with the constant patch 1.1e-5), i.e. a quarter of the bound at the most."""
    _check_case(pn, ps, layout, mask_kind)


def test_constant_patch_where_the_c2_terms_decide():
    _check_case(2, 9, "grid", "all", constant_patch=True)


def test_identical_images_give_exactly_zero():
    c, g, m = (t.to(DEV) for t in R.make_case(7, 8, "grid", "tenth"))
    out4, grad, tot = _raw(g, g, m, 7, 8, "grid")
    assert out4[0] == 0 and out4[1] == 1 and out4[2] == 0 and tot == np.float32(TOTAL0)


def test_a_ranks_share_with_the_batch_wide_count_adds_up_to_the_whole_batch():
    n, ps = 6, 8
    c, g, m = (t.to(DEV) for t in R.make_case(n, ps, "patch_major", "tenth"))
    whole = _raw(c, g, m, n, ps, "patch_major")
    h = 3 * ps * ps
    a = _raw(c[:h].contiguous(), g[:h].contiguous(), m[:h].contiguous(), 3, ps, "patch_major", norm=n)
    b = _raw(c[h:].contiguous(), g[h:].contiguous(), m[h:].contiguous(), 3, ps, "patch_major", norm=n)
    assert np.concatenate([a[1], b[1]]).tobytes() == whole[1].tobytes()     # a ray's gradient is its own patch's, whatever the rank
    assert a[0][3] + b[0][3] == whole[0][3]
    for k in (0, 1, 2):                                                     # L, SSIM share, term: three fp32 roundings apart at most
        assert abs(float(a[0][k]) + float(b[0][k]) - float(whole[0][k])) <= 3 * 2.0 ** -24 * max(float(whole[0][k]), 0.5), k


# ------------------------------------------------------------------------------------------------ the fused step
def _world():
    """The small training golden's scene (tests/test_train_gpu.py::_setup, as tests/test_depth_sup_gpu.py uses it) with a fresh dilated 7_8 batch:
    56 x 56 rays over and around the 64 x 48 frame, jittered depth tables, a smooth random ground truth; the aggregator
    carries the learnable blur predictor (seeded), which the other two forms leave alone."""
    if "w" in _WORLD:
        return _WORLD["w"]
    from hybridneuralrendering_amd import scenes
    from hybridneuralrendering_amd.aggregator import PointAggregator
    from hybridneuralrendering_amd.render import HybridRenderer
    from hybridneuralrendering_amd.train import TrainPath
    from oracle import query_oracle as qo
    from tests import blur_learn_ref as BR
    from tests.golden_io import load_train, torch_inputs
    d = load_train("scannet_small")
    dev = torch.device(DEV)
    pn, ps = 7, 8
    o = dict(d["opt"])
    o.update(dilation_setup="7_8_1_8", learnable_blur_kernel=1, learnable_blur_kernel_conv=0, learnable_blur_kernel_size=9, learnable_blur_patch_size=ps,
             learnable_blur_kernel_mode=4, learnable_blur_kernel_norm=0, boundary_mode=1)
    opt = scenes.default_opt(**o)
    agg = PointAggregator(opt)
    agg.load_state_dict(d["sd"], strict=False)
    with torch.no_grad():
        for n, w in zip(BR.NAMES, BR.make_weights(ps, 9, 4, 7)):
            agg.get_parameter(n).copy_(w)
    agg = agg.to(dev)
    ti = torch_inputs(d, dev)
    path = TrainPath(HybridRenderer(opt, agg, dev))
    near, far = d["near_far"]
    rng = np.random.default_rng(11)
    S = pn * ps
    px, py = np.meshgrid(np.arange(4, 4 + S), np.arange(-4, -4 + S), indexing="ij")
    pix = np.stack([px, py], axis=-1).reshape(-1, 2).astype(np.int32)
    raydir = scenes.camera_rays(pix, d["intrinsic"], d["c2w"])
    tmid = qo.tmid_table(float(near), float(far), o["z_depth_dim"])[None].repeat(raydir.shape[0], 0)
    tmid = (tmid + rng.uniform(-0.3, 0.3, size=tmid.shape) * (far - near) / o["z_depth_dim"] * 0.5).astype(np.float32)
    field = torch.rand((1, 3, S + 4, S + 4), generator=torch.Generator().manual_seed(3))
    gt = torch.nn.functional.avg_pool2d(field, 5, stride=1)[0].permute(1, 2, 0).reshape(-1, 3).contiguous()
    x = SimpleNamespace(d=d, ti=ti, opt=opt, agg=agg, path=path, pn=pn, ps=ps, near=near, far=far, tmid=torch.from_numpy(tmid).to(dev), gt=gt.to(dev),
                        zero_epsilon=float(d["zero_epsilon"]), raydir=torch.from_numpy(raydir).to(dev))
    x.args = (x.raydir, ti["campos"][0], ti["camrotc2w"][0], ti["bg_color"][0], near, far, ti["c2w_nearest"][0], ti["campos_nearest"][0],
              ti["intrinsic_nearest"][0], ti["images_nearest"][0])
    _WORLD["w"] = x
    return x


def _leaves(ti):
    mk = lambda t: t.clone().requires_grad_(True)
    return mk(ti["emb"]), mk(ti["conf"]), mk(ti["pdir"]), mk(ti["color"])


def _form_kw(x, form):
    from hybridneuralrendering_amd.blur import LearnableBlur
    from tests.test_train_gpu import _blur_kernels
    if form == "blur_kernels":
        return dict(blur_kernels=_blur_kernels(torch.device(DEV)))
    if form == "learnable_blur":
        return dict(learnable_blur=LearnableBlur(x.agg, x.opt, x.pn, x.ps))
    return {}


def _fused(x, extra, **more):
    from hybridneuralrendering_amd.train import train_step
    emb, conf, pdir, color = _leaves(x.ti)
    out, pg, ag = train_step(x.path, x.agg, x.ti["xyz"], emb, conf, pdir, color, *x.args, x.gt, zero_epsilon=x.zero_epsilon, w_color=1.0, w_zero_one=1e-4,
                             frame_weight=FW, tmid=x.tmid, assign_grads=False, **extra, **more)
    return ({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}, {k: v.clone() for k, v in pg.items()},
            {k: v.clone() for k, v in ag.items()})


def _by_hand(x, extra):
    """The launches of the step with the SSIM term, one by one, hnr_ssim_loss through ctypes"""
    from hybridneuralrendering_amd import _lib
    from hybridneuralrendering_amd.blur import blur_select, blur_select_bwd
    from hybridneuralrendering_amd.losses import shipped_loss_grads
    from hybridneuralrendering_amd.render import PointCloud
    ti = x.ti
    cloud = PointCloud(ti["xyz"], ti["emb"], ti["conf"], ti["pdir"], ti["color"])
    o, S = x.path.forward(cloud, *x.args, tmid=x.tmid)
    col = o["coarse_raycolor"]
    lb = extra.get("learnable_blur")
    if "blur_kernels" in extra:
        col, sel, kk = blur_select(col, x.gt, extra["blur_kernels"], x.pn, x.ps)
    elif lb is not None:
        col = lb.forward(col, x.gt)
    parts, g_col, g_cc = shipped_loss_grads(col, o["conf_coefficient"], x.gt, o["ray_mask"], x.zero_epsilon, 1.0, 1e-4, FW, conf_rows=True)
    parts0, g_col0 = parts.clone(), g_col.clone()
    n = x.pn * x.pn
    out4 = torch.empty(4, device=DEV)
    scratch = torch.empty(2 * n, dtype=torch.float64, device=DEV)
    win = (ctypes.c_float * 7)(*[float(v) for v in R.window()])
    P = _lib.ptr
    _lib.check(_lib.lib().hnr_ssim_loss(P(col.contiguous()), P(x.gt), P(o["ray_mask"]), x.pn, x.ps, 0, win, W_SSIM, FW, None, P(parts), P(out4), P(g_col), 1,
                                        P(scratch), _lib.stream()), "hnr_ssim_loss")
    g_sum = g_col.clone()
    g_blur = {}
    if "blur_kernels" in extra:
        g_col = blur_select_bwd(g_col, kk, sel, x.pn, x.ps)
    elif lb is not None:
        g_col, g_blur = lb.backward(g_col)
    pg, ag = x.path.backward(S, g_col, g_cc)
    ag = dict(ag)
    ag.update({k: v.clone() for k, v in g_blur.items()})
    return dict(o=o, col=col.clone(), parts0=parts0, parts=parts.clone(), out4=out4, g_col0=g_col0, g_sum=g_sum, pg={k: v.clone() for k, v in pg.items()},
                ag={k: v.clone() for k, v in ag.items()})


def _autograd(x, extra):
    """render_train + the blur module's autograd form + shipped_loss + ssim_patch_loss + backward()"""
    from hybridneuralrendering_amd import blur as B
    from hybridneuralrendering_amd.losses import shipped_loss, ssim_patch_loss
    from hybridneuralrendering_amd.train import render_train
    emb, conf, pdir, color = _leaves(x.ti)
    x.agg.zero_grad(set_to_none=True)
    o = render_train(x.path, x.agg, x.ti["xyz"], emb, conf, pdir, color, *x.args, tmid=x.tmid)
    col = o["coarse_raycolor"]
    if "blur_kernels" in extra:
        col = B.blur_update_output(col[None], x.gt[None], extra["blur_kernels"], x.pn, x.ps)[0]
    elif "learnable_blur" in extra:
        col = B.learnable_blur_update_output(col[None], x.gt[None], x.agg.blur_predictor(), x.opt, x.pn, x.ps)[0]
    loss, parts = shipped_loss(col, o["conf_coefficient"], x.gt, o["ray_mask"], x.zero_epsilon, 1.0, 1e-4, frame_weight=FW, conf_rows=True)
    term, out4 = ssim_patch_loss(col, x.gt, o["ray_mask"], x.pn, x.ps, W_SSIM, frame_weight=FW)
    (loss + term).backward()
    ref = {"neural_points.points_embeding": emb.grad, "neural_points.points_conf": conf.grad, "neural_points.points_dir": pdir.grad,
           "neural_points.points_color": color.grad}
    for n, q in x.agg.named_parameters():
        if q.grad is not None:
            ref["aggregator." + n] = q.grad.clone()
    x.agg.zero_grad(set_to_none=True)
    return float((loss + term).detach()), out4, ref


def _same_grads(pg, ag, pg2, ag2, what):
    from tests.test_blur_learn_gpu import ATOMIC_PREFIXES, ATOMIC_REL
    assert set(pg) == set(pg2) and set(ag) == set(ag2), what
    for k in pg:
        assert torch.equal(pg[k], pg2[k]), (what, k)
    for k in ag:
        if k.startswith(ATOMIC_PREFIXES):                                   # the few float-atomic weight gradients: tests/test_train_gpu.py's bound
            sc = float(ag2[k].abs().max())
            assert float((ag[k] - ag2[k]).abs().max()) <= (1e-3 if ag2[k].numel() == 1 else ATOMIC_REL) * max(sc, 1e-30), (what, k)
        else:
            assert torch.equal(ag[k], ag2[k]), (what, k)


@pytest.mark.parametrize("form", ["plain", "blur_kernels", "learnable_blur"])
def test_train_step_with_ssim_equals_the_launches_made_by_hand_and_the_autograd_form(form):
    from tests.test_train_gpu import _check_grads
    x = _world()
    extra = _form_kw(x, form)
    out, pg, ag = _fused(x, extra, w_ssim=W_SSIM, patch_num=x.pn, patch_size=x.ps)
    h = _by_hand(x, extra)
    hits = int((out["ray_mask"] > 0).sum())
    assert hits > 0
    # bit for bit: outputs, the term, the total, every gradient
    assert torch.equal(out["loss"], h["parts"]) and torch.equal(out["loss_ssim"], h["out4"]) and out["loss_ssim"].shape == (4,)
    assert int(out["loss_ssim"][3]) == hits and 0 < float(out["loss_ssim"][0]) < 1
    assert _np(h["parts"])[0] == np.float32(_np(h["parts0"])[0] + _np(h["out4"])[2]) and torch.equal(h["parts"][1:], h["parts0"][1:])
    if form != "plain":
        assert torch.equal(out["blurred_raycolor"].reshape(-1, 3), h["col"].reshape(-1, 3))
    _same_grads(pg, ag, h["pg"], h["ag"], "fused vs by hand (%s)" % form)
    # the term on the step's own colours is the restatement's, and the colour gradient gained exactly its gradient
    r64 = R.ssim_term(h["col"].reshape(-1, 3).cpu(), x.gt.cpu(), out["ray_mask"].cpu(), x.pn, x.ps, W_SSIM, frame_weight=FW)
    r32 = R.ssim_term(h["col"].reshape(-1, 3).cpu(), x.gt.cpu(), out["ray_mask"].cpu(), x.pn, x.ps, W_SSIM, frame_weight=FW, dtype=torch.float32)
    e_ref = float((r32["grad"].double() - r64["grad"]).abs().max())
    added = (h["g_sum"].double() - h["g_col0"].double()).cpu()
    # (g + v - g is v up to one rounding of the sum)
    assert float((added - r64["grad"]).abs().max()) <= R.bound(e_ref, float(r64["grad"].abs().max())) + 2.0 ** -24 * float(h["g_sum"].abs().max())
    assert abs(float(out["loss_ssim"][0]) - float(r64["L"])) <= R.bound(abs(float(r32["L"]) - float(r64["L"])), float(r64["L"]))
    # the autograd form, tolerances of tests/test_train_gpu.py
    total, out4, ref = _autograd(x, extra)
    if form == "learnable_blur":                                            # (that module's autograd form sums in another order: its colours differ in last bits)
        np.testing.assert_allclose(_np(out4), _np(out["loss_ssim"]), rtol=1e-5)
    else:
        assert torch.equal(out4, out["loss_ssim"])
    np.testing.assert_allclose(float(out["loss"][0]), total, rtol=1e-6)
    got = {"neural_points." + k: v for k, v in pg.items()}
    got.update({"aggregator." + k: v for k, v in ag.items()})
    assert set(ref) <= set(got)
    _check_grads(got, ref, "ssim step vs autograd (%s)" % form)
    # the term acts: the embedding gradient moves by more than 1 % of its maximum
    _o, pg0, _a = _fused(x, extra, patch_num=x.pn, patch_size=x.ps)
    e = pg0["points_embeding"]
    assert float((pg["points_embeding"] - e).abs().max()) > 1e-2 * float(e.abs().max())


def test_w_ssim_zero_is_the_step_without_the_argument_and_a_random_batch_raises():
    from hybridneuralrendering_amd._lib import HnrError
    x = _world()
    out0, pg0, ag0 = _fused(x, {})
    out1, pg1, ag1 = _fused(x, {}, w_ssim=0.0)
    assert sorted(out0) == sorted(out1) and "loss_ssim" not in out0
    for k in ("loss", "coarse_raycolor", "conf_coefficient", "ray_mask"):
        assert torch.equal(out0[k], out1[k]), k
    _same_grads(pg0, ag0, pg1, ag1, "w_ssim=0")
    for more in (dict(w_ssim=0.1), dict(w_ssim=0.1, patch_num=7, patch_size=7), dict(w_ssim=-0.1, patch_num=7, patch_size=8),
                 dict(w_ssim=0.1, patch_num=14, patch_size=4), dict(w_ssim=0.1, patch_num=7, patch_size=8, ssim_norm_patches=48),
                 dict(w_ssim=0.1, patch_num=7, patch_size=8, patch_layout="random")):
        with pytest.raises(HnrError):                                       # no patches / not the batch's patches / a patch below the window
            _fused(x, {}, **more)


def test_captured_step_with_ssim_replays_the_eager_step():
    from hybridneuralrendering_amd.train import CapturedTrainStep
    from hybridneuralrendering_amd._lib import HnrError
    x = _world()
    ti = x.ti
    sample = dict(raydir=x.raydir, campos=ti["campos"][0], camrot=ti["camrotc2w"][0], bg_color=ti["bg_color"][0], c2w_nearest=ti["c2w_nearest"][0],
                  campos_nearest=ti["campos_nearest"][0], intrinsic_nearest=ti["intrinsic_nearest"][0], images_nearest=ti["images_nearest"][0],
                  gt_image=x.gt, tmid=x.tmid, frame_weight=FW)
    emb, conf, pdir, color = _leaves(ti)
    with pytest.raises(HnrError):                                           # a weight, but no patches
        CapturedTrainStep(x.path, x.agg, ti["xyz"], emb, conf, pdir, color, sample, x.near, x.far, zero_epsilon=x.zero_epsilon, w_ssim=W_SSIM)
    cap = CapturedTrainStep(x.path, x.agg, ti["xyz"], emb, conf, pdir, color, sample, x.near, x.far, zero_epsilon=x.zero_epsilon, patch_num=x.pn,
                            patch_size=x.ps, w_ssim=W_SSIM)
    out, pg, ag = cap.step(assign_grads=False)
    torch.cuda.synchronize()
    e_out, e_pg, e_ag = _fused(x, {}, w_ssim=W_SSIM, patch_num=x.pn, patch_size=x.ps)
    assert torch.equal(out["loss"], e_out["loss"]) and torch.equal(out["loss_ssim"], e_out["loss_ssim"])
    assert torch.equal(out["coarse_raycolor"], e_out["coarse_raycolor"])
    _same_grads(pg, ag, e_pg, e_ag, "captured vs eager")
    # another item weight through the graph's input: the term follows it
    out, pg, ag = cap.step(assign_grads=False, frame_weight=0.35)
    torch.cuda.synchronize()
    assert float(out["loss_ssim"][0]) == float(e_out["loss_ssim"][0])
    assert float(out["loss_ssim"][2]) == float(np.float32(np.float32(np.float32(0.35) * np.float32(W_SSIM)) * _np(out["loss_ssim"])[0]))
