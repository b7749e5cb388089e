"""The learnable blur module as three launches (blur.LearnableBlur) and inside the fused training step, on the GPU.

Bound of the fp64 comparisons (tests/blur_learn_ref.py::bound_check): the device's error against the fp64 restatement is at most 4 x the error of the
fp32 restatement against fp64 on the same inputs, per tensor, with a floor of one fp32 ulp of the tensor's largest magnitude.  The lines that start
with BLUR_LEARN_RATIO are what profiles/blur_learn_tests.txt records."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import adam_ref
from tests import blur_learn_ref as R
from tests.golden_io import blur_learn_case, load_train, torch_inputs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 12345.0
# the weight gradients that are float-atomic sums (tests/test_train_gpu.py:443-446): equal up to the order of their additions
ATOMIC_REL = 2e-6


def _opt(cfg):
    return SimpleNamespace(learnable_blur_kernel_size=cfg["ks"], learnable_blur_kernel_conv=0, learnable_blur_kernel_norm=cfg["norm"],
                           learnable_blur_kernel_mode=cfg["mode"], boundary_mode=cfg["bmode"])


def _np(t):
    return t.detach().cpu().numpy()


def _device_run(lb, color, gt, up):
    out = lb.forward(color.to(DEV), gt.to(DEV)).clone()
    kern = lb.kernels.clone()
    g_color, grads = lb.backward(up.to(DEV))
    res = dict(out=_np(out), kernels=_np(kern), grad_color=_np(g_color))
    res.update({n: _np(g) for n, g in grads.items()})
    return res


def _report(what, got, f32, f64):
    bad = []
    for k in ["out", "kernels", "grad_color"] + R.NAMES:
        ok, e_new, e_ref, floor = R.bound_check(got[k], f32[k], f64[k])
        print("BLUR_LEARN_RATIO %s %s: hip %.3e, restatement fp32 %.3e, ulp of max %.3e -> ratio %.2f" % (what, k, e_new, e_ref, floor, e_new / max(e_ref, floor)))
        if not ok:
            bad.append((k, e_new, e_ref, floor))
    assert not bad, (what, bad)


@pytest.mark.parametrize("tag", ["a", "c"])
def test_learnable_blur_object_matches_reference_golden(tag):
    """LearnableBlur.forward / backward vs the imported reference's recorded colours, colour gradients and all eight parameter gradients
    (a: the shipped configuration; c: boundary_mode 2), with tests/test_blur_gpu.py's tolerances for the same quantities."""
    from hybridneuralrendering_amd.blur import LearnableBlur
    cfg, color, gt, up, predictor, blocks, exp = blur_learn_case(tag, device=DEV)
    lb = LearnableBlur(predictor, _opt(cfg), cfg["pn"], cfg["ps"])
    got = _device_run(lb, color, gt, up)
    np.testing.assert_allclose(got["out"], exp["out"][0], rtol=0, atol=2e-6)
    np.testing.assert_allclose(got["grad_color"], exp["grad_color"][0], rtol=0, atol=5e-6)
    for l in range(4):
        for k in ("weight", "bias"):
            g = exp["grads"]["0.%d.%s" % (2 * l, k)]
            np.testing.assert_allclose(got["learn_blur_kernel_block.%d.%s" % (2 * l, k)], g, rtol=0, atol=2e-5 * max(1.0, float(np.abs(g).max())))


# (pn < 0: patch-major).  n_in = 18 is no multiple of 4 and n_out = 2; softmax + mode 0 + boundary 0; the largest footprint (n_in = 512: 16 weight
# tiles in layer 0, n_out = 226: two output chunks in the last layer, every LDS array full); three patch-major patches (a workgroup with an empty
# fourth slot) under each boundary rule
SHAPES = [dict(pn=2, ps=3, ks=1, mode=4, norm=0, bmode=1), dict(pn=2, ps=4, ks=3, mode=0, norm=1, bmode=0), dict(pn=1, ps=16, ks=15, mode=4, norm=0, bmode=1),
          dict(pn=-3, ps=8, ks=9, mode=4, norm=0, bmode=0), dict(pn=-3, ps=8, ks=9, mode=4, norm=0, bmode=1), dict(pn=-3, ps=8, ks=9, mode=4, norm=0, bmode=2)]


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_small_and_awkward_shapes_against_fp64(i):
    from hybridneuralrendering_amd.blur import LearnableBlur
    cfg = SHAPES[i]
    n = -cfg["pn"] if cfg["pn"] < 0 else cfg["pn"] ** 2
    weights = R.make_weights(cfg["ps"], cfg["ks"], cfg["mode"], 10 + i)
    color, gt, up = R.make_case(n, cfg["ps"], 20 + i)
    f32, f64 = R.run(color, gt, up, weights, cfg, torch.float32), R.run(color, gt, up, weights, cfg, torch.float64)
    lb = LearnableBlur(R.make_mlp(weights, DEV), _opt(cfg), abs(cfg["pn"]), cfg["ps"], layout="patch_major" if cfg["pn"] < 0 else "grid")
    _report("shape %d %s" % (i, "/".join("%s=%d" % kv for kv in cfg.items())), _device_run(lb, color, gt, up), f32, f64)


def test_patch_major_shards_equal_the_grid_run():
    """Forward colours and colour gradients of patch-major shards are the grid run's bits on the same rays; the shards' parameter gradients, summed
    in fp64, match the grid's within the fp64 bound (the grid's own p-ascending chain is another order of the same terms)."""
    from hybridneuralrendering_amd.blur import LearnableBlur
    from hybridneuralrendering_amd.parallel import shard_patches
    cfg = dict(pn=3, ps=8, ks=9, mode=4, norm=0, bmode=1)
    weights = R.make_weights(8, 9, 4, 3)
    color, gt, up = R.make_case(9, 8, 4)
    mlp = R.make_mlp(weights, DEV)
    full = _device_run(LearnableBlur(mlp, _opt(cfg), 3, 8), color, gt, up)
    f32, f64 = R.run(color, gt, up, weights, cfg, torch.float32), R.run(color, gt, up, weights, cfg, torch.float64)
    total = {n: np.zeros(full[n].shape, dtype=np.float64) for n in R.NAMES}
    for rank in range(2):
        ids, rays = shard_patches(3, 8, 2, rank)
        part = _device_run(LearnableBlur(mlp, _opt(cfg), ids.numel(), 8, layout="patch_major"), color[rays], gt[rays], up[rays])
        assert np.array_equal(part["out"], full["out"][rays.numpy()]) and np.array_equal(part["grad_color"], full["grad_color"][rays.numpy()])
        assert np.array_equal(part["kernels"], full["kernels"][ids.numpy()])
        for n in R.NAMES:
            total[n] += part[n].astype(np.float64)
    bad = []
    for n in R.NAMES:
        ok, e_new, e_ref, floor = R.bound_check(total[n], f32[n], f64[n])
        print("BLUR_LEARN_RATIO shards summed %s: hip %.3e, restatement fp32 %.3e, ulp of max %.3e -> ratio %.2f" % (n, e_new, e_ref, floor, e_new / max(e_ref, floor)))
        if not ok:
            bad.append((n, e_new, e_ref, floor))
    assert not bad, bad


def _guarded(n, fill=SENTINEL):
    big = torch.full((n + 64,), fill, dtype=torch.float32, device=DEV)
    return big, big[:n]


def test_two_runs_are_bit_identical_and_nothing_is_written_out_of_bounds():
    """The C entry points on caller buffers with 64 sentinel floats behind every output, every gradient and the workspace: two runs give the same
    bits everywhere, the sentinels are intact.  7 patches: one full workgroup and one with an empty slot."""
    from hybridneuralrendering_amd import _lib
    L = _lib.lib()
    pn, ps, ks, mode = -7, 8, 9, 4
    n, n_in, n_out = 7, 128, 82
    weights = [w.to(DEV).contiguous() for w in R.make_weights(ps, ks, mode, 5)]
    color, gt, up = (t.to(DEV).contiguous() for t in R.make_case(n, ps, 6))
    prm = _lib.BlurLearnParams(pn, ps, ks, mode, 0, 1, 0.01)
    w = _lib.BlurLearnWeights()
    for l in range(4):
        w.w[l], w.b[l] = weights[2 * l].data_ptr(), weights[2 * l + 1].data_ptr()
    nbytes = int(L.hnr_blur_learn_workspace_bytes(n, ps, ks, mode))
    assert nbytes > 0 and nbytes % 4 == 0

    def once():
        bufs = dict(ws=_guarded(nbytes // 4), out=_guarded(n * ps * ps * 3), kernels=_guarded(n * ks * ks), g_color=_guarded(n * ps * ps * 3))
        gw = _lib.BlurLearnWeights()
        for l in range(4):
            bufs["gw%d" % l], bufs["gb%d" % l] = _guarded(weights[2 * l].numel()), _guarded(weights[2 * l + 1].numel())
            gw.w[l], gw.b[l] = bufs["gw%d" % l][1].data_ptr(), bufs["gb%d" % l][1].data_ptr()
        p = lambda k: ctypes.c_void_p(bufs[k][1].data_ptr())
        _lib.check(L.hnr_blur_learn_forward(ctypes.byref(prm), ctypes.byref(w), _lib.ptr(color), _lib.ptr(gt), p("ws"), nbytes, p("out"), p("kernels"),
                                            _lib.stream()), "hnr_blur_learn_forward")
        _lib.check(L.hnr_blur_learn_backward(ctypes.byref(prm), ctypes.byref(w), _lib.ptr(color), _lib.ptr(up), p("ws"), nbytes, p("g_color"),
                                             ctypes.byref(gw), _lib.stream()), "hnr_blur_learn_backward")
        torch.cuda.synchronize()
        for k, (big, t) in bufs.items():
            assert bool((big[t.numel():] == SENTINEL).all()), "sentinels behind %s" % k
            if k != "ws":
                assert not bool((t == SENTINEL).any()), "%s was not written completely" % k
        return {k: t.clone() for k, (big, t) in bufs.items()}
    a, b = once(), once()
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert float(a["kernels"].reshape(n, -1).sum(dim=1).sub(1).abs().max()) < 1e-5


# ---------------------------------------------------------------------------------------------------------------- inside the training step
def _setup(seed=7):
    """tests/test_train_gpu.py::_setup() on the small training golden, with the blur predictor switched on (the golden's state dict has no
    predictor: seeded weights, the same for every call with the same seed)."""
    from hybridneuralrendering_amd import scenes
    from hybridneuralrendering_amd.aggregator import PointAggregator
    from hybridneuralrendering_amd.render import HybridRenderer
    from hybridneuralrendering_amd.train import TrainPath
    d = load_train("scannet_small")
    dev = torch.device(DEV)
    pn, ps = (int(x) for x in d["opt"]["dilation_setup"].split("_")[:2])
    o = dict(d["opt"])
    o.update(learnable_blur_kernel=1, learnable_blur_kernel_conv=0, learnable_blur_kernel_size=9, learnable_blur_patch_size=ps, learnable_blur_kernel_mode=4,
             learnable_blur_kernel_norm=0, boundary_mode=1)
    opt = scenes.default_opt(**o)
    assert opt.is_train == 1
    agg = PointAggregator(opt)
    missing = agg.load_state_dict(d["sd"], strict=False)
    assert not missing.unexpected_keys and sorted(missing.missing_keys) == sorted(R.NAMES)
    with torch.no_grad():
        for n, w in zip(R.NAMES, R.make_weights(ps, 9, 4, seed)):
            agg.get_parameter(n).copy_(w)
    agg = agg.to(dev)
    ti = torch_inputs(d, dev)
    path = TrainPath(HybridRenderer(opt, agg, dev))
    near, far = d["near_far"]
    x = SimpleNamespace(d=d, ti=ti, opt=opt, agg=agg, path=path, pn=pn, ps=ps, near=near, far=far, tmid=torch.from_numpy(d["tmid"]).to(dev),
                        gt=torch.from_numpy(d["gt"][0]).to(dev), zero_epsilon=float(d["zero_epsilon"]))
    x.args = (ti["raydir"][0], ti["campos"][0], ti["camrotc2w"][0], ti["bg_color"][0], near, far, ti["c2w_nearest"][0], ti["campos_nearest"][0],
              ti["intrinsic_nearest"][0], ti["images_nearest"][0])
    return x


def _leaves(ti):
    mk = lambda t: t.clone().requires_grad_(True)
    return mk(ti["emb"]), mk(ti["conf"]), mk(ti["pdir"]), mk(ti["color"])


def _close_atomic(a, b, what):
    sc = float(b.abs().max())
    assert float((a - b).abs().max()) <= (1e-3 if b.numel() == 1 else ATOMIC_REL) * max(sc, 1e-30), what


ATOMIC_PREFIXES = ("alpha_branch.", "color_final_block.", "aux_merge_weight_block.6.", "aux_block_s")


def _same_grads(ag, ref, what):
    for n in ref:
        if n.startswith(ATOMIC_PREFIXES):
            _close_atomic(ag[n], ref[n], (what, n))
        else:
            assert torch.equal(ag[n], ref[n]), (what, n)


def test_fused_step_equals_the_same_launches_made_by_hand():
    """train_step(learnable_blur=lb) against path.forward -> lb.forward -> losses.shipped_loss_grads -> lb.backward -> path.backward: bit for bit in the
    loss parts, the blurred colours, the four point gradients, every aggregator gradient and the eight predictor gradients (the few float-atomic
    weight gradients: tests/test_train_gpu.py's 2e-6 relative bound).  .grad is assigned under the aggregator's names.  The module changed the colours."""
    from hybridneuralrendering_amd.blur import LearnableBlur
    from hybridneuralrendering_amd.losses import shipped_loss_grads
    from hybridneuralrendering_amd.render import PointCloud
    from hybridneuralrendering_amd.train import train_step
    x = _setup()
    ti = x.ti
    lb = LearnableBlur(x.agg, x.opt, x.pn, x.ps)
    # by hand
    emb, conf, pdir, color = _leaves(ti)
    cloud = PointCloud(ti["xyz"], emb.detach(), conf.detach(), pdir.detach(), color.detach())
    o, S = x.path.forward(cloud, *x.args, tmid=x.tmid)
    col = lb.forward(o["coarse_raycolor"], x.gt)
    parts, g_col, g_cc = shipped_loss_grads(col, o["conf_coefficient"], x.gt, o["ray_mask"], x.zero_epsilon, 1.0, 1e-4, 0.7, conf_rows=True)
    g_col2, g_blur = lb.backward(g_col)
    pg, ag = x.path.backward(S, g_col2, g_cc)
    ref = dict(parts=parts.clone(), col=col.clone(), kern=lb.kernels.clone(), pg={k: v.clone() for k, v in pg.items()}, ag={k: v.clone() for k, v in ag.items()},
               blur={k: v.clone() for k, v in g_blur.items()})
    # the step
    emb2, conf2, pdir2, color2 = _leaves(ti)
    x.agg.zero_grad(set_to_none=True)
    out, pg2, ag2 = train_step(x.path, x.agg, ti["xyz"], emb2, conf2, pdir2, color2, *x.args, x.gt, zero_epsilon=x.zero_epsilon, w_color=1.0, w_zero_one=1e-4,
                               frame_weight=0.7, tmid=x.tmid, learnable_blur=lb)
    assert torch.equal(out["loss"], ref["parts"])
    assert torch.equal(out["blurred_raycolor"], ref["col"]) and torch.equal(out["blur_kernels_pred"], ref["kern"])
    assert out["blur_kernels_pred"].shape == (x.pn * x.pn, 9, 9)
    for k in ref["pg"]:
        assert torch.equal(pg2[k], ref["pg"][k]), k
    _same_grads(ag2, ref["ag"], "aggregator")
    assert sorted(n for n in ag2 if n.startswith("learn_blur_kernel_block.")) == sorted(R.NAMES)
    for n in R.NAMES:
        assert torch.equal(ag2[n], ref["blur"][n]), n
        assert torch.equal(x.agg.get_parameter(n).grad, ref["blur"][n]) and float(ref["blur"][n].abs().max()) > 0, n
    assert emb2.grad is not None and torch.equal(emb2.grad.reshape(-1, 32), pg2["points_embeding"])
    # without reuse_outputs the step hands out gradient tensors of its own, not the module's static buffers: a second step adds to .grad
    assert all(ag2[n].data_ptr() != g_blur[n].data_ptr() for n in R.NAMES)
    train_step(x.path, x.agg, ti["xyz"], emb2, conf2, pdir2, color2, *x.args, x.gt, zero_epsilon=x.zero_epsilon, w_color=1.0, w_zero_one=1e-4,
               frame_weight=0.7, tmid=x.tmid, learnable_blur=lb)
    for n in R.NAMES:
        assert torch.equal(x.agg.get_parameter(n).grad, ref["blur"][n] + ref["blur"][n]), n
    assert not torch.equal(out["blurred_raycolor"].reshape(-1, 3), out["coarse_raycolor"].reshape(-1, 3))
    # learnable_blur=None: the outputs carry nothing of the module
    out0, _pg, ag0 = train_step(x.path, x.agg, ti["xyz"], emb2, conf2, pdir2, color2, *x.args, x.gt, zero_epsilon=x.zero_epsilon, tmid=x.tmid, assign_grads=False)
    assert "blurred_raycolor" not in out0 and not any(n.startswith("learn_blur_kernel_block.") for n in ag0)


def _autograd_form(x, leaves, predictor_dtype):
    """render_train + the blur module in autograd form + shipped_loss + backward.  predictor_dtype None: blur.learnable_blur_update_output as it is;
    torch.float64: the same with the predictor, the normalisation and the blend evaluated in fp64 on a copy of the predictor (cast in, cast out)."""
    import copy
    from hybridneuralrendering_amd import blur as B
    from hybridneuralrendering_amd.losses import shipped_loss
    from hybridneuralrendering_amd.train import render_train
    emb, conf, pdir, color = leaves
    x.agg.zero_grad(set_to_none=True)
    o = render_train(x.path, x.agg, x.ti["xyz"], emb, conf, pdir, color, *x.args, tmid=x.tmid)
    c = o["coarse_raycolor"][None]
    if predictor_dtype is None:
        pred_mod = x.agg.blur_predictor()
        col = B.learnable_blur_update_output(c, x.gt[None], pred_mod, x.opt, x.pn, x.ps)[0]
    else:
        pred_mod = copy.deepcopy(x.agg.blur_predictor()).to(predictor_dtype)
        n, ks = x.pn * x.pn, 9
        gray = B._GrayPatches.apply(c, x.gt[None], x.pn, x.ps)
        pred = pred_mod(gray.view(n, -1).to(predictor_dtype))
        k = pred[:, 0:ks * ks].view(n, 1, ks, ks)
        k = k / torch.sum(k, dim=(2, 3), keepdim=True)
        w = pred[:, -1][..., None, None, None]
        ident = torch.zeros_like(k)
        ident[:, :, ks // 2, ks // 2] = 1.0
        k = w * k + (1 - w) * ident
        k = (k / torch.sum(k, dim=(2, 3), keepdim=True)).to(torch.float32)
        col = B._BlurApply.apply(c, k, x.pn, x.ps, 1)[0]
    loss, parts = shipped_loss(col, o["conf_coefficient"], x.gt, o["ray_mask"], x.zero_epsilon, 1.0, 1e-4, frame_weight=0.7, conf_rows=True)
    loss.backward()
    res = {"loss": parts[0:1].detach().clone(), "points_embeding": emb.grad, "points_conf": conf.grad, "points_dir": pdir.grad, "points_color": color.grad}
    for n, q in x.agg.named_parameters():
        if n.startswith("learn_blur_kernel_block."):
            res[n] = pred_mod.get_parameter(n[len("learn_blur_kernel_block."):]).grad
        elif q.grad is not None:
            res[n] = q.grad
    return {k: _np(v).astype(np.float64) for k, v in res.items()}


def test_fused_step_against_the_autograd_form():
    """E_ref = |fp32 autograd form - fp64-predictor form|, E_new = |fused step - fp64-predictor form|: E_new <= 4 E_ref (ulp floor) for the loss, each
    point-gradient tensor and each weight-gradient tensor.

    The few weight gradients that the training backward sums with float atomics (ATOMIC_PREFIXES; tests/test_train_gpu.py:443-446) differ from run to
    run of the SAME form in their last bits, the fp64-predictor form's included, so for them the reference carries that spread itself: measured
    here, alpha_branch.0.bias (one scalar) came out 2 ulp from the reference in the fused step while the fp32 autograd form happened to hit it
    exactly (E_ref = 0).  Their floor is therefore the suite's atomic-sum bound (2e-6 of the tensor's largest magnitude, 1e-3 for a lone scalar)
    instead of one ulp; every other tensor has the one-ulp floor."""
    from hybridneuralrendering_amd.blur import LearnableBlur
    from hybridneuralrendering_amd.train import train_step
    x = _setup()
    f32 = _autograd_form(x, _leaves(x.ti), None)
    f64 = _autograd_form(x, _leaves(x.ti), torch.float64)
    lb = LearnableBlur(x.agg, x.opt, x.pn, x.ps)
    emb, conf, pdir, color = _leaves(x.ti)
    out, pg, ag = train_step(x.path, x.agg, x.ti["xyz"], emb, conf, pdir, color, *x.args, x.gt, zero_epsilon=x.zero_epsilon, w_color=1.0, w_zero_one=1e-4,
                             frame_weight=0.7, tmid=x.tmid, learnable_blur=lb, assign_grads=False)
    got = {"loss": out["loss"][0:1]}
    got.update(pg)
    got.update(ag)
    assert sorted(got) == sorted(f64), (sorted(set(got) ^ set(f64)))
    bad = []
    for k in sorted(f64):
        ok, e_new, e_ref, floor = R.bound_check(_np(got[k]), f32[k], f64[k])
        if k.startswith(ATOMIC_PREFIXES):
            floor = (1e-3 if f64[k].size == 1 else ATOMIC_REL) * float(np.abs(f64[k]).max())
            ok = e_new <= max(4.0 * e_ref, floor)
        print("BLUR_LEARN_RATIO step vs autograd %s: fused %.3e, autograd fp32 %.3e, ulp of max %.3e -> ratio %.2f" % (k, e_new, e_ref, floor, e_new / max(e_ref, floor)))
        if not ok:
            bad.append((k, e_new, e_ref, floor))
    assert not bad, bad


class _Points(torch.nn.Module):
    def __init__(self, ti):
        super().__init__()
        for n, k in (("points_embeding", "emb"), ("points_conf", "conf"), ("points_dir", "pdir"), ("points_color", "color")):
            setattr(self, n, torch.nn.Parameter(ti[k].clone()))

    def leaves(self):
        return self.points_embeding, self.points_conf, self.points_dir, self.points_color


def _world(seed=7):
    from hybridneuralrendering_amd.blur import LearnableBlur
    from hybridneuralrendering_amd.optim import ShellOptimizers
    x = _setup(seed)
    x.opt.lr, x.opt.plr, x.opt.lr_policy, x.opt.lr_decay_exp, x.opt.lr_decay_iters = 5e-4, 2e-3, "iter_exponential_decay", 0.1, 1000000
    x.pts = _Points(x.ti)
    x.so = ShellOptimizers(x.opt, x.agg, x.pts, total_steps=1000)
    x.lb = LearnableBlur(x.agg, x.opt, x.pn, x.ps)
    return x


def _eager(x, gt=None):
    from hybridneuralrendering_amd.train import train_step
    emb, conf, pdir, color = x.pts.leaves()
    return train_step(x.path, x.agg, x.ti["xyz"], emb, conf, pdir, color, *x.args, x.gt if gt is None else gt, zero_epsilon=x.zero_epsilon, tmid=x.tmid,
                      learnable_blur=x.lb, optimizer=x.so)


def test_optimizer_updates_the_predictor_inside_the_step():
    """optimizer=ShellOptimizers: after one step all eight learn_blur_kernel_block.* tensors have changed, their _version has advanced, .grad is not
    assigned, and the update is tests/adam_ref.py's restatement applied to the step's own gradient buffers."""
    x = _world()
    params = {n: x.agg.get_parameter(n) for n in R.NAMES}
    before = {n: (_np(q).copy(), q._version) for n, q in params.items()}
    out, pg, ag = _eager(x)
    rows = _np(x.so.scalars())
    for n, q in params.items():
        p0, v0 = before[n]
        assert q._version > v0 and q.grad is None, n
        assert not np.array_equal(_np(q), p0), n
        want, m1, v1 = adam_ref.update_f32(p0, _np(ag[n]).reshape(p0.shape), np.zeros_like(p0), np.zeros_like(p0), rows[0])
        assert np.array_equal(_np(q).view(np.uint32), want.view(np.uint32)), n
        st = x.so.optimizer.state[q]
        assert np.array_equal(_np(st["exp_avg"]), m1) and np.array_equal(_np(st["exp_avg_sq"]), v1), n
    assert x.so.counters() == (1, 1001)


def _copy_state(src, dst):
    """dst's parameters, Adam moments and counters := src's (two worlds built by _world with the same seed: the same parameter order)."""
    with torch.no_grad():
        for (n, a), (m, b) in zip(list(src.agg.named_parameters()) + list(src.pts.named_parameters()),
                                  list(dst.agg.named_parameters()) + list(dst.pts.named_parameters())):
            assert n == m
            b.copy_(a)
            for k in ("exp_avg", "exp_avg_sq"):
                dst.so.optimizer.state[b][k].copy_(src.so.optimizer.state[a][k])
        dst.so.optimizer._counters.copy_(src.so.optimizer._counters)


def _snapshot(out, pg, ag):
    return dict(loss=out["loss"].clone(), col=out["blurred_raycolor"].clone(), kern=out["blur_kernels_pred"].clone(), pg={k: v.clone() for k, v in pg.items()},
                ag={k: v.clone() for k, v in ag.items()})


def _same_step(a, b, what):
    assert torch.equal(a["loss"], b["loss"]), (what, a["loss"], b["loss"])
    assert torch.equal(a["col"], b["col"]) and torch.equal(a["kern"], b["kern"]), what
    for k in b["pg"]:
        assert torch.equal(a["pg"][k], b["pg"][k]), (what, k)
    assert sorted(a["ag"]) == sorted(b["ag"])
    _same_grads(a["ag"], b["ag"], what)


def test_captured_step_with_the_predictor_and_the_optimizer_inside():
    """CapturedTrainStep(learnable_blur=, optimizer=): two graphs built from equal initial states replay bit-identically; three replays equal three
    eager train_step calls, each made from the state and inputs its replay started from (bit for bit, apart from the float-atomic weight gradients,
    which get the 2e-6 bound -- the parameters they update may then differ in a last bit, so the states are made equal again before every step);
    another gt_image through step(gt_image=...) changes blur_kernels_pred."""
    from hybridneuralrendering_amd.train import CapturedTrainStep
    A, B, C = _world(), _world(), _world()

    def capture(x):
        ti = x.ti
        sample = dict(raydir=ti["raydir"][0], campos=ti["campos"][0], camrot=ti["camrotc2w"][0], bg_color=ti["bg_color"][0], c2w_nearest=ti["c2w_nearest"][0],
                      campos_nearest=ti["campos_nearest"][0], intrinsic_nearest=ti["intrinsic_nearest"][0], images_nearest=ti["images_nearest"][0],
                      gt_image=x.gt, tmid=x.tmid)
        emb, conf, pdir, color = x.pts.leaves()
        return CapturedTrainStep(x.path, x.agg, ti["xyz"], emb, conf, pdir, color, sample, x.near, x.far, zero_epsilon=x.zero_epsilon, optimizer=x.so,
                                 learnable_blur=x.lb)
    cap_a, cap_b = capture(A), capture(B)
    torch.cuda.synchronize()
    assert A.so.counters() == (0, 1000)                       # warm-up and capture moved nothing
    names = [n for n, _q in A.agg.named_parameters()]
    for i in range(3):
        if i > 0:
            _copy_state(A, B)
            _copy_state(A, C)
        v0 = A.agg.get_parameter(R.NAMES[0])._version
        sa, sb, sc = _snapshot(*cap_a.step()), _snapshot(*cap_b.step()), _snapshot(*_eager(C))
        torch.cuda.synchronize()
        _same_step(sb, sa, "graph B vs graph A, replay %d" % i)
        _same_step(sc, sa, "eager vs graph A, step %d" % i)
        assert A.agg.get_parameter(R.NAMES[0])._version > v0
        for n in names:
            pa, pb, pc = A.agg.get_parameter(n), B.agg.get_parameter(n), C.agg.get_parameter(n)
            if n.startswith(ATOMIC_PREFIXES):
                _close_atomic(pb, pa, n); _close_atomic(pc, pa, n)
            else:
                assert torch.equal(pb, pa) and torch.equal(pc, pa), (i, n)
    assert A.so.counters() == (3, 1003)
    k0 = cap_a.out["blur_kernels_pred"].clone()
    out, _pg, _ag = cap_a.step(gt_image=torch.rand_like(A.gt))
    torch.cuda.synchronize()
    assert not torch.equal(out["blur_kernels_pred"], k0)
