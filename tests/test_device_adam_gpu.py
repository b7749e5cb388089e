"""The device optimiser step (csrc/adam.hip, hybridneuralrendering_amd/optim.py) on the GPU: bit-equal to the NumPy restatement (tests/adam_ref.py),
the tick's scalars against Python doubles, against torch.optim.Adam, determinism and graph capture, inside the training step, the `_version`
rule, prune / grow, and the state-dict exchange with torch.

Not asserted (documented in include/hnr.h): subnormal intermediates and NaN / inf gradients."""
import copy

import numpy as np
import pytest
import torch

from tests import adam_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 12345.0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _np(t):
    return t.detach().cpu().numpy()


def _slot(shape, pad, seed, scale=0.3):
    """A tensor of `shape` inside a larger buffer with `pad` sentinel floats in front (pad = 64: 16-byte aligned; 65: 4 bytes off) and 64 behind."""
    n = int(np.prod(shape))
    big = torch.full((pad + n + 64,), SENTINEL, dtype=torch.float32, device=DEV)
    g = torch.Generator().manual_seed(seed)
    t = big[pad:pad + n].view(shape)
    t.copy_((torch.randn(shape, generator=g) * scale).to(DEV))
    assert t.is_contiguous() and t.data_ptr() % 16 == (4 * pad) % 16
    return big, t


def _sentinels_ok(big, pad, n):
    return bool((big[:pad] == SENTINEL).all()) and bool((big[pad + n:] == SENTINEL).all())


def _unit_case():
    """Two groups over tensors of the sizes at which the kernel takes another path: below / at / above a wave's 16-byte pass, one chunk - 1, one chunk
    + 5 (a whole chunk and a tail chunk), the reference's [1,N,1] / [N,32] shapes (multi-chunk), and two tensors whose p and g sit 4 bytes off a
    16-byte boundary (the one-element-per-lane path, one of them longer than a chunk)."""
    from hybridneuralrendering_amd import _lib
    C = _lib.ADAM_CHUNK
    shapes = [((1,), 64), ((3,), 64), ((255,), 64), ((256,), 64), ((257,), 64), ((C - 1,), 64), ((C + 5,), 64), ((1, 1000, 1), 64), ((1000, 32), 64),
              ((1027,), 65), ((C + 5,), 65)]
    slots = []
    for i, (shape, pad) in enumerate(shapes):
        bp, p = _slot(shape, pad, 100 + i)
        bg, g = _slot(shape, pad, 200 + i, scale=0.0)
        slots.append(dict(shape=shape, pad=pad, n=int(np.prod(shape)), bp=bp, p=p, bg=bg, g=g, group=i % 2, p0=_np(p).copy()))
    return slots


def _unit_grads(slots, step):
    """Gradients over five decades with zero rows; the last eighth of every tensor (at least its last element when it has 8 or more) is never touched."""
    rng = np.random.default_rng(1000 + step)
    for s in slots:
        n = s["n"]
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, -1, n)).astype(np.float32)
        g[rng.random(n) < 0.5] = 0.0
        if n >= 8:
            g[-(n // 8):] = 0.0
        s["g"].copy_(torch.from_numpy(g.reshape(s["shape"])).to(DEV))


def _unit_optimizer(slots):
    from hybridneuralrendering_amd.optim import DeviceAdam
    groups = [dict(params=[s["p"] for s in slots if s["group"] == 0], lr=5e-4, lr_decay_exp=0.1, lr_decay_iters=1000000),
              dict(params=[s["p"] for s in slots if s["group"] == 1], lr=2e-3, betas=(0.8, 0.99), eps=1e-6, lr_decay_exp=0.5, lr_decay_iters=1000)]
    return DeviceAdam(groups)


def _run_unit(steps=5, check=True):
    slots = _unit_case()
    opt = _unit_optimizer(slots)
    opt.set_iteration(700)
    ref = [dict(p=_np(s["p"]).copy(), m=np.zeros(s["shape"], np.float32), v=np.zeros(s["shape"], np.float32)) for s in slots]
    for step in range(steps):
        _unit_grads(slots, step)
        opt.step({s["p"]: s["g"] for s in slots})
        if not check:
            continue
        rows = _np(opt.scalars())                                     # the scalars the device wrote feed the restatement
        for s, r in zip(slots, ref):
            r["p"], r["m"], r["v"] = R.update_f32(r["p"], _np(s["g"]), r["m"], r["v"], rows[s["group"]])
            st = opt.state[s["p"]]
            for name, got in (("p", s["p"]), ("m", st["exp_avg"]), ("v", st["exp_avg_sq"])):
                assert _same_bits(_np(got), r[name]), (step, s["shape"], s["pad"], name, float(np.abs(_np(got) - r[name]).max()))
    return slots, opt, ref


def test_update_is_bit_equal_to_the_fp32_restatement():
    slots, opt, ref = _run_unit()
    for s, r in zip(slots, ref):
        assert _sentinels_ok(s["bp"], s["pad"], s["n"]) and _sentinels_ok(s["bg"], s["pad"], s["n"]), s["shape"]
        if s["n"] >= 8:                                                # never-touched elements: bit-unchanged, their state zero
            k = s["n"] // 8
            assert _same_bits(_np(s["p"]).reshape(-1)[-k:], s["p0"].reshape(-1)[-k:])
            assert not _np(opt.state[s["p"]]["exp_avg"]).reshape(-1)[-k:].any()
            assert float(np.abs(_np(s["p"]) - s["p0"]).max()) > 0      # ... while the rest moved
    assert opt.counters() == (5, 705)


def test_tick_scalars_match_python_doubles():
    """The device row against Python's doubles at relative 1e-12: pow in fp64 is good to a few 1e-16 on either side (amplified ~1e3 x by the
    cancellation in 1 - beta2^step at step 1), and a wrong formula shows at 1e-3 or more."""
    from hybridneuralrendering_amd.optim import DeviceAdam
    p, q = torch.zeros(5, device=DEV), torch.zeros(7, device=DEV)
    hyper = [dict(lr=5e-4, betas=(0.9, 0.999), eps=1e-8, lr_decay_exp=0.1, lr_decay_iters=1000000),
             dict(lr=2e-3, betas=(0.8, 0.99), eps=1e-6, lr_decay_exp=0.5, lr_decay_iters=1000)]
    opt = DeviceAdam([dict(params=[p], **hyper[0]), dict(params=[q], **hyper[1])])
    grads = {p: torch.ones_like(p), q: torch.ones_like(q)}

    def check(step, it):
        rows = _np(opt.scalars())
        assert rows.shape == (2, R.ROW)
        for gi, h in enumerate(hyper):
            want = R.tick_row(h["lr"], h["betas"][0], h["betas"][1], h["eps"], h["lr_decay_exp"], h["lr_decay_iters"], step, it)
            np.testing.assert_allclose(rows[gi], want, rtol=1e-12, atol=0, err_msg="group %d step %d it %d" % (gi, step, it))
    for n in range(1, 6):                                              # iteration n: step n, schedule exponent (n - 1) / decay_iters
        opt.step(grads)
        check(n, n - 1)
    opt.set_iteration(123456)
    opt.step(grads)
    check(6, 123456)
    assert opt.counters() == (6, 123457)
    opt._counters[0:1].fill_(99999)                                    # adam_step 100 000: beta1^step underflows, bc2 is within 1e-43 of 1
    opt.step(grads)
    check(100000, 123457)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_device_step_against_torch_adam(seed):
    """The CPU test's comparison (tests/test_device_adam.py) with the device in the restatement's place: 40 steps on 4096 x 32, the schedule running
    on the device from iteration 123456, against torch's fp64 run; the device may err at most 4 x what torch's own fp32 run errs."""
    from hybridneuralrendering_amd.optim import DeviceAdam
    c = R.CASE
    p0, gs = R.case_inputs(seed)
    ref, t32 = R.torch_case(seed, "float64"), R.torch_case(seed, "float32")
    p = torch.from_numpy(p0).to(DEV)
    opt = DeviceAdam([dict(params=[p], lr=c["lr0"], betas=(c["beta1"], c["beta2"]), eps=c["eps"], lr_decay_exp=c["decay_exp"], lr_decay_iters=c["decay_iters"])])
    opt.set_iteration(c["it0"])
    g = torch.empty_like(p)
    for t in range(c["T"]):
        g.copy_(torch.from_numpy(gs[t]).to(DEV))
        opt.step({p: g})
    st = opt.state[p]
    for name, mine, theirs, r in zip("pmv", (p, st["exp_avg"], st["exp_avg_sq"]), t32, ref):
        e_mine, e_torch = R.max_err(_np(mine), r), R.max_err(theirs, r)
        print("seed %d %s: device %.3e  torch fp32 %.3e  ratio %.2f" % (seed, name, e_mine, e_torch, e_mine / e_torch))
        assert e_torch > 0
        assert e_mine <= 4.0 * e_torch, (name, e_mine, e_torch)
    k = c["N"] // 16
    assert _same_bits(_np(p)[-k:], p0[-k:])


def test_two_runs_and_a_captured_step_are_bit_identical():
    a_slots, a_opt, _ = _run_unit(check=False)
    b_slots, b_opt, _ = _run_unit(check=False)
    for a, b in zip(a_slots, b_slots):
        assert _same_bits(_np(a["p"]), _np(b["p"])), a["shape"]
        for k in ("exp_avg", "exp_avg_sq"):
            assert _same_bits(_np(a_opt.state[a["p"]][k]), _np(b_opt.state[b["p"]][k]))
    # step() captured once, replayed three times == three eager steps
    e_slots, c_slots = _unit_case(), _unit_case()
    e_opt, c_opt = _unit_optimizer(e_slots), _unit_optimizer(c_slots)
    _unit_grads(e_slots, 0)
    _unit_grads(c_slots, 0)
    for _ in range(3):
        e_opt.step({s["p"]: s["g"] for s in e_slots})
    grads = {s["p"]: s["g"] for s in c_slots}
    c_opt.prepare(grads)
    v0 = c_slots[0]["p"]._version
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c_opt.step(grads)
    assert c_opt.counters() == (0, 0)                                  # a capture runs nothing
    for _ in range(3):
        graph.replay()
        c_opt.mark_updated()
    torch.cuda.synchronize()
    assert c_opt.counters() == (3, 3) and e_opt.counters() == (3, 3)
    assert c_slots[0]["p"]._version > v0
    for a, b in zip(e_slots, c_slots):
        assert _same_bits(_np(a["p"]), _np(b["p"])), a["shape"]
        for k in ("exp_avg", "exp_avg_sq"):
            assert _same_bits(_np(e_opt.state[a["p"]][k]), _np(c_opt.state[b["p"]][k]))
        assert _sentinels_ok(b["bp"], b["pad"], b["n"])
    assert np.array_equal(_np(e_opt.scalars()), _np(c_opt.scalars()))


# ------------------------------------------------------------------------------------------------ inside the training step
def _train_scene():
    from tests.test_train_gpu import _setup, _leaves
    from hybridneuralrendering_amd.optim import DeviceAdam
    d, ti, opt, agg, path = _setup()
    dev = ti["emb"].device
    leaves = dict(zip(("points_embeding", "points_conf", "points_dir", "points_color"), _leaves(ti)))
    named = list(agg.named_parameters())
    optim = DeviceAdam([dict(params=[q for _n, q in named], names=[n for n, _q in named], lr=5e-4, lr_decay_exp=0.1, lr_decay_iters=1000000),
                        dict(params=list(leaves.values()), names=list(leaves), lr=2e-3, lr_decay_exp=0.1, lr_decay_iters=1000000)])
    optim.set_iteration(1000)
    near, far = d["near_far"]
    kw = dict(tmid=torch.from_numpy(d["tmid"]).to(dev), zero_epsilon=float(d["zero_epsilon"]))
    gt = torch.from_numpy(d["gt"][0]).to(dev)
    return d, ti, opt, agg, path, leaves, named, optim, near, far, gt, kw


class _Mirror:
    """The restatement's copy of every parameter and its state; advance() applies one step with the device's scalars and the step's own gradients."""

    def __init__(self, named, leaves):
        self.params = [(n, q, 0) for n, q in named] + [(n, q, 1) for n, q in leaves.items()]
        self.p = {n: _np(q).copy() for n, q, _g in self.params}
        self.m = {n: np.zeros_like(a) for n, a in self.p.items()}
        self.v = {n: np.zeros_like(a) for n, a in self.p.items()}

    def advance(self, optim, pg, ag, what):
        rows = _np(optim.scalars())
        grads = dict(ag)
        grads.update(pg)
        moved = 0
        for n, q, gi in self.params:
            if n in grads:
                g = _np(grads[n]).reshape(self.p[n].shape)
                self.p[n], self.m[n], self.v[n] = R.update_f32(self.p[n], g, self.m[n], self.v[n], rows[gi])
                moved += 1
            assert _same_bits(_np(q), self.p[n]), (what, n)
            st = optim.state[q]
            assert _same_bits(_np(st["exp_avg"]), self.m[n]) and _same_bits(_np(st["exp_avg_sq"]), self.v[n]), (what, n)
            assert q.grad is None, (what, n)
        assert moved >= 20 + 4


def test_train_step_with_the_optimizer_inside():
    """Three train_step(..., optimizer=...) calls: after each, every parameter equals the restatement applied to that step's own pg / ag and the
    previous values, bit for bit (per step: the CNN gradients' float-atomic last bits differ run to run, the update of given gradients does not);
    .grad stays None.  optimizer=None still assigns .grad."""
    from hybridneuralrendering_amd.train import train_step
    d, ti, opt, agg, path, leaves, named, optim, near, far, gt, kw = _train_scene()
    emb, conf, pdir, color = leaves.values()
    mirror = _Mirror(named, leaves)

    def step(**extra):
        return train_step(path, agg, ti["xyz"], emb, conf, pdir, color, ti["raydir"][0], ti["campos"][0], ti["camrotc2w"][0], ti["bg_color"][0], near, far,
                          ti["c2w_nearest"][0], ti["campos_nearest"][0], ti["intrinsic_nearest"][0], ti["images_nearest"][0], gt, **kw, **extra)
    losses = []
    for i in range(3):
        out, pg, ag = step(optimizer=optim)
        mirror.advance(optim, pg, ag, "eager step %d" % i)
        losses.append(float(out["loss"][0]))
    assert optim.counters() == (3, 1003)
    assert all(np.isfinite(losses)) and len(set(losses)) == 3           # the parameters moved: another loss every step
    _o, pg, ag = step()
    assert emb.grad is not None and torch.equal(emb.grad.reshape(-1, 32), pg["points_embeding"]) and agg.block1[0].weight.grad is not None
    assert optim.counters() == (3, 1003)


def test_captured_train_step_with_the_optimizer_inside():
    """CapturedTrainStep(..., optimizer=...): one replay = one whole iteration.  The construction (warm-up steps, capture) moves nothing; after
    each of three replays every parameter equals the restatement applied to the replay's own gradients."""
    from hybridneuralrendering_amd.train import CapturedTrainStep
    d, ti, opt, agg, path, leaves, named, optim, near, far, gt, kw = _train_scene()
    emb, conf, pdir, color = leaves.values()
    mirror = _Mirror(named, leaves)
    sample = dict(raydir=ti["raydir"][0], campos=ti["campos"][0], camrot=ti["camrotc2w"][0], bg_color=ti["bg_color"][0], c2w_nearest=ti["c2w_nearest"][0],
                  campos_nearest=ti["campos_nearest"][0], intrinsic_nearest=ti["intrinsic_nearest"][0], images_nearest=ti["images_nearest"][0],
                  gt_image=gt, tmid=kw["tmid"])
    cap = CapturedTrainStep(path, agg, ti["xyz"], emb, conf, pdir, color, sample, near, far, zero_epsilon=kw["zero_epsilon"], optimizer=optim)
    torch.cuda.synchronize()
    assert optim.counters() == (0, 1000)
    for n, q, _g in mirror.params:
        assert _same_bits(_np(q), mirror.p[n]), n
    v0 = emb._version
    for i in range(3):
        out, pg, ag = cap.step()
        torch.cuda.synchronize()
        mirror.advance(optim, pg, ag, "replay %d" % i)
        assert emb._version > v0
        v0 = emb._version
    assert optim.counters() == (3, 1003)


def test_cached_renderer_follows_an_optimizer_step():
    """The `_version` rule: after one optimiser step, the renderer that rendered before the step (packed weights, feature map, per-point table and
    record cache all filled) gives what a fresh renderer over clones of the updated parameters gives.  Without the bump in DeviceAdam.step the
    cached renderer returns the old image."""
    from hybridneuralrendering_amd.train import train_step
    from hybridneuralrendering_amd.aggregator import PointAggregator
    from hybridneuralrendering_amd.render import HybridRenderer, PointCloud
    d, ti, opt, agg, path, leaves, named, optim, near, far, gt, kw = _train_scene()
    emb, conf, pdir, color = leaves.values()
    rnd = path.r

    def render(renderer, cloud):
        renderer.opt.is_train = 0                                      # an evaluation render: no depth jitter
        try:
            out = renderer.render_rays(cloud, ti["raydir"][0], ti["campos"][0], ti["camrotc2w"][0], ti["bg_color"][0], near, far, ti["c2w_nearest"][0],
                                       ti["campos_nearest"][0], ti["intrinsic_nearest"][0], ti["images_nearest"][0])
        finally:
            renderer.opt.is_train = 1
        return out["coarse_raycolor"].clone()
    cloud = PointCloud(ti["xyz"], emb, conf, pdir, color)
    before = render(rnd, cloud)
    assert 200 <= before.shape[0] <= 4096
    for _ in range(2):
        train_step(path, agg, ti["xyz"], emb, conf, pdir, color, ti["raydir"][0], ti["campos"][0], ti["camrotc2w"][0], ti["bg_color"][0], near, far,
                   ti["c2w_nearest"][0], ti["campos_nearest"][0], ti["intrinsic_nearest"][0], ti["images_nearest"][0], gt, optimizer=optim, **kw)
    cached = render(rnd, cloud)
    opt2 = copy.copy(opt)
    agg2 = PointAggregator(opt2)
    agg2.load_state_dict({k: v.detach().clone() for k, v in agg.state_dict().items()}, strict=True)
    agg2 = agg2.to(DEV)
    fresh = render(HybridRenderer(opt2, agg2, torch.device(DEV)),
                   PointCloud(ti["xyz"].clone(), emb.detach().clone(), conf.detach().clone(), pdir.detach().clone(), color.detach().clone()))
    assert float((fresh - before).abs().max()) > 1e-4                   # the steps moved the image ...
    assert torch.equal(cached, fresh)                                   # ... and the cached renderer saw it


# ------------------------------------------------------------------------------------------------ prune / grow, state dicts
def _check_fresh_step(so, what):
    """One step with seeded gradients on every parameter equals the restatement from zero state on the buffers as they are now."""
    optim = so.optimizer
    rng = np.random.default_rng(5)
    items = [(n, p, gi) for gi, g in enumerate(optim.param_groups) for n, p in zip(optim._names[gi], g["params"])]
    before = {n: _np(p).copy() for n, p, _gi in items}
    grads = {n: torch.from_numpy((rng.standard_normal(tuple(p.shape)) * 1e-3).astype(np.float32)).to(DEV) for n, p, _gi in items}
    for n, p, _gi in items:
        st = optim.state[p]
        assert st["exp_avg"].shape == p.shape and not bool(st["exp_avg"].any()) and not bool(st["exp_avg_sq"].any()), (what, n)
    so.step(grads)
    rows = _np(so.scalars())
    for n, p, gi in items:
        want, m, v = R.update_f32(before[n], _np(grads[n]), np.zeros_like(before[n]), np.zeros_like(before[n]), rows[gi])
        assert _same_bits(_np(p), want), (what, n)
        assert _same_bits(_np(optim.state[p]["exp_avg"]), m) and _same_bits(_np(optim.state[p]["exp_avg_sq"]), v), (what, n)
    return rows


def test_rebuild_after_prune_and_grow():
    from tests.test_modules_gpu import _build
    from hybridneuralrendering_amd.optim import ShellOptimizers
    d, ti, opt, npts, net, dev = _build("scannet_small")
    opt.lr, opt.plr, opt.lr_policy, opt.lr_decay_exp, opt.lr_decay_iters = 5e-4, 2e-3, "iter_exponential_decay", 0.1, 1000000
    so = ShellOptimizers(opt, net.aggregator, npts)
    assert [len(g["params"]) for g in so.param_groups] == [len(list(net.aggregator.parameters())), 4]
    _check_fresh_step(so, "fresh")
    assert so.counters() == (1, 1)
    n0 = int(npts.xyz.shape[0])
    with torch.no_grad():
        npts.points_conf[0, ::3, 0] = 0.01
        n1 = int((npts.points_conf[0, :, 0] >= 0.1).sum())           # (the step above moved the confidences too)
    assert 0 < n1 <= n0 - (n0 + 2) // 3
    npts.prune(0.1)
    so.rebuild(20000)
    assert so.counters() == (0, 20000)
    assert so.param_groups[1]["params"][0] is npts.points_embeding and npts.points_embeding.shape[1] == n1
    rows = _check_fresh_step(so, "after prune")
    np.testing.assert_allclose(rows[:, 0], [R.schedule_lr(5e-4, 0.1, 1e6, 20000), R.schedule_lr(2e-3, 0.1, 1e6, 20000)], rtol=1e-12)
    assert so.counters() == (1, 20001) and rows[0, 9] == 1.0
    add = 3000
    g = torch.Generator().manual_seed(4)
    cam = torch.from_numpy(d["c2w"][:3, 3]) + torch.from_numpy(d["c2w"][:3, 2]) * 0.25
    add_xyz = (cam[None] + (torch.rand((add, 3), generator=g) - 0.5) * torch.tensor([0.2, 0.2, 0.01])).to(dev)
    npts.grow_points(add_xyz, torch.zeros(add, 32, device=dev), torch.rand((add, 3), generator=g).to(dev), torch.zeros(add, 3, device=dev),
                     torch.ones(add, 1, device=dev))
    so.rebuild(40000)
    assert so.counters() == (0, 40000) and so.param_groups[1]["params"][0].shape[1] == n1 + add
    rows = _check_fresh_step(so, "after grow")
    np.testing.assert_allclose(rows[1, 0], R.schedule_lr(2e-3, 0.1, 1e6, 40000), rtol=1e-12)


def _exchange_params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(s, generator=g) * 0.3).to(DEV)) for s in ((300, 32), (1, 777, 3), (45,))]


def _exchange_grads(params, step):
    rng = np.random.default_rng(50 + step)
    return [torch.from_numpy((rng.standard_normal(tuple(p.shape)) * 10.0 ** rng.uniform(-5, -1, tuple(p.shape))).astype(np.float32)).to(DEV) for p in params]


def _four_x(mine, theirs, start, grads, row, what):
    """The 4 x rule for ONE step from a common fp32 state: both against the fp64 restatement of that step."""
    for i, ((p, m, v), (tp, tm, tv), (sp, sm, sv), g) in enumerate(zip(mine, theirs, start, grads)):
        ref = R.update_f64(sp, _np(g), sm, sv, row)
        for name, a, b, r in zip("pmv", (p, m, v), (tp, tm, tv), ref):
            e_mine, e_torch = R.max_err(a, r), R.max_err(b, r)
            print("%s tensor %d %s: device %.3e torch %.3e" % (what, i, name, e_mine, e_torch))
            assert e_torch > 0 and e_mine <= 4.0 * e_torch, (what, i, name, e_mine, e_torch)


def test_state_dict_exchange_with_torch_adam():
    from hybridneuralrendering_amd.optim import DeviceAdam
    hyper = dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8)
    # ---- DeviceAdam -> torch.optim.Adam
    mine_p, their_p = _exchange_params(3), _exchange_params(3)
    mine = DeviceAdam([dict(params=mine_p, lr_decay_exp=0.1, lr_decay_iters=1000000, **hyper)])
    mine.set_iteration(123456)
    for s in range(3):
        mine.step(dict(zip(mine_p, _exchange_grads(mine_p, s))))
    theirs = torch.optim.Adam([dict(params=their_p, **hyper)])
    theirs.load_state_dict(copy.deepcopy(mine.state_dict()))         # (state_dict hands out the live state tensors, as torch's does; torch keeps what it is given)
    assert all(theirs.state[a]["exp_avg"].data_ptr() != mine.state[b]["exp_avg"].data_ptr() for a, b in zip(their_p, mine_p))
    with torch.no_grad():
        for a, b in zip(their_p, mine_p):
            a.copy_(b)
    assert theirs.param_groups[0]["lr"] == pytest.approx(R.schedule_lr(2e-3, 0.1, 1e6, 123459), rel=1e-12)
    start = [(_np(p).copy(), _np(mine.state[p]["exp_avg"]).copy(), _np(mine.state[p]["exp_avg_sq"]).copy()) for p in mine_p]
    grads = _exchange_grads(mine_p, 3)
    mine.step(dict(zip(mine_p, grads)))
    for p, g in zip(their_p, grads):
        p.grad = g.clone()
    theirs.step()
    assert all(float(theirs.state[p]["step"]) == 4.0 for p in their_p) and mine.counters()[0] == 4
    _four_x([(_np(p), _np(mine.state[p]["exp_avg"]), _np(mine.state[p]["exp_avg_sq"])) for p in mine_p],
            [(_np(p), _np(theirs.state[p]["exp_avg"]), _np(theirs.state[p]["exp_avg_sq"])) for p in their_p], start, grads, _np(mine.scalars())[0],
            "device -> torch")
    # ---- torch.optim.Adam -> DeviceAdam
    their_p, mine_p = _exchange_params(4), _exchange_params(4)
    theirs = torch.optim.Adam([dict(params=their_p, **hyper)])
    for s in range(3):
        for p, g in zip(their_p, _exchange_grads(their_p, s)):
            p.grad = g
        theirs.step()
    mine = DeviceAdam([dict(params=mine_p, **hyper)])
    mine.load_state_dict(theirs.state_dict())
    with torch.no_grad():
        for a, b in zip(mine_p, their_p):
            a.copy_(b)
    assert mine.counters() == (3, 0)
    start = [(_np(p).copy(), _np(theirs.state[p]["exp_avg"]).copy(), _np(theirs.state[p]["exp_avg_sq"]).copy()) for p in their_p]
    grads = _exchange_grads(their_p, 3)
    mine.step(dict(zip(mine_p, grads)))
    for p, g in zip(their_p, grads):
        p.grad = g.clone()
    theirs.step()
    _four_x([(_np(p), _np(mine.state[p]["exp_avg"]), _np(mine.state[p]["exp_avg_sq"])) for p in mine_p],
            [(_np(p), _np(theirs.state[p]["exp_avg"]), _np(theirs.state[p]["exp_avg_sq"])) for p in their_p], start, grads, _np(mine.scalars())[0],
            "torch -> device")
