"""CPU checks of the device optimiser (hybridneuralrendering_amd/optim.py, csrc/adam.hip): the NumPy restatement of its arithmetic against
torch.optim.Adam, the schedule against LambdaLR, the state-dict layout, option handling and the C entry points' argument checks.  No GPU."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import adam_ref as R


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_matches_torch_adam_on_the_cpu(seed):
    """The restated arithmetic against torch.optim.Adam(foreach=False), both against torch's fp64 run of the same 40 steps: the fp32 restatement
    may err at most 4 x what torch's own fp32 run errs (the project's usual margin; measured 1.00 - 1.52 x, torch's errors about 5e-7 / 2.4e-9 /
    6.6e-11 for p / m / v), and the fp64 restatement is the fp64 run up to rounding: <= 1e-12 x max|ref| (about ten fp64 roundings per step and
    element, 40 steps: 4e-14 relative, with a decade and a half for the cancellation in m + w1 (g - m))."""
    p0, gs = R.case_inputs(seed)
    ref = R.torch_case(seed, "float64")
    t32 = R.torch_case(seed, "float32")
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    q, n, w = p0.astype(np.float64), np.zeros(p0.shape), np.zeros(p0.shape)
    tiny = np.finfo(np.float32).tiny
    for t, g in enumerate(gs):
        row = R.case_row(t)
        p, m, v = R.update_f32(p, g, m, v, row)
        q, n, w = R.update_f64(q, g, n, w, row)
        for a in (m, v, R.f32(row[6]) * g):                                  # no subnormal state or product with these inputs
            nz = np.abs(a[a != 0])
            assert nz.size == 0 or nz.min() >= tiny
    for name, mine, mine64, theirs, r in zip("pmv", (p, m, v), (q, n, w), t32, ref):
        e_mine, e_torch = R.max_err(mine, r), R.max_err(theirs, r)
        print("seed %d %s: restatement %.3e  torch fp32 %.3e  ratio %.2f  | fp64 restatement %.3e" % (seed, name, e_mine, e_torch, e_mine / e_torch,
                                                                                                        R.max_err(mine64, r)))
        assert e_torch > 0
        assert e_mine <= 4.0 * e_torch, (name, e_mine, e_torch)
        assert R.max_err(mine64, r) <= 1e-12 * np.abs(r).max(), name
    k = R.CASE["N"] // 16
    assert np.array_equal(p[-k:].view(np.uint32), p0[-k:].view(np.uint32))    # never-touched rows: bit-unchanged
    assert not m[-k:].any() and not v[-k:].any()


def _lambda_lr(opt, last_epoch=-1):
    """get_scheduler(optimizer, opt) of the reference for lr_policy 'iter_exponential_decay' (models/helpers/networks.py:56-61)."""
    def lambda_rule(it):
        return pow(opt.lr_decay_exp, it / opt.lr_decay_iters)
    return lambda o: torch.optim.lr_scheduler.LambdaLR(o, lr_lambda=lambda_rule, last_epoch=last_epoch)


def test_schedule_formula_matches_lambda_lr():
    from hybridneuralrendering_amd import optim
    opt = SimpleNamespace(lr_decay_exp=0.1, lr_decay_iters=1000000)
    lr0 = 0.002
    P = torch.nn.Parameter(torch.zeros(3))
    o = torch.optim.Adam([P], lr=lr0)
    sch = _lambda_lr(opt)(o)
    for n in range(1, 6):                                                    # iteration n (1-based) runs with the rate n - 1 scheduler steps left
        want = o.param_groups[0]["lr"]
        assert R.schedule_lr(lr0, 0.1, 1e6, n - 1) == pytest.approx(want, rel=1e-15)
        assert lr0 * optim.schedule_factor(n - 1, 0.1, 1000000) == pytest.approx(want, rel=1e-15)
        assert R.tick_row(lr0, 0.9, 0.999, 1e-8, 0.1, 1e6, n, n - 1)[0] == pytest.approx(want, rel=1e-15)
        P.grad = torch.zeros(3); o.step(); sch.step()
    # init_scheduler(total_steps): total_steps scheduler.step() calls on a fresh scheduler (LambdaLR's closed form: the constructor's last_epoch)
    o2 = torch.optim.Adam([P], lr=lr0)
    o2.param_groups[0]["initial_lr"] = lr0
    _lambda_lr(opt, last_epoch=123455)(o2)
    want = o2.param_groups[0]["lr"]
    assert want == pytest.approx(lr0 * 0.1 ** 0.123456, rel=1e-12)
    assert R.schedule_lr(lr0, 0.1, 1e6, 123456) == pytest.approx(want, rel=1e-15)
    o3 = torch.optim.Adam([P], lr=lr0)                                       # ... the closed form is the loop
    s3 = _lambda_lr(opt)(o3)
    for _ in range(7):
        P.grad = torch.zeros(3); o3.step(); s3.step()
    o4 = torch.optim.Adam([P], lr=lr0)
    o4.param_groups[0]["initial_lr"] = lr0
    _lambda_lr(opt, last_epoch=6)(o4)
    assert o3.param_groups[0]["lr"] == o4.param_groups[0]["lr"]


def _two_groups():
    torch.manual_seed(0)
    a = [torch.nn.Parameter(torch.randn(5, 7)), torch.nn.Parameter(torch.randn(7))]
    b = [torch.nn.Parameter(torch.randn(1, 11, 3))]
    return [dict(params=a, lr=5e-4), dict(params=b, lr=2e-3, eps=1e-7)]


def test_state_dict_has_torch_adams_layout():
    from hybridneuralrendering_amd.optim import DeviceAdam
    groups = _two_groups()
    theirs = torch.optim.Adam([dict(g) for g in groups], betas=(0.9, 0.999))
    for g in groups:
        for p in g["params"]:
            p.grad = torch.ones_like(p)
    theirs.step()
    mine = DeviceAdam([dict(g, lr_decay_exp=0.1, lr_decay_iters=1000000) for g in groups])
    a, b = mine.state_dict(), theirs.state_dict()
    assert sorted(a) == sorted(b) == ["param_groups", "state"]
    assert sorted(a["state"]) == sorted(b["state"]) == [0, 1, 2]
    for i in b["state"]:
        assert sorted(a["state"][i]) == sorted(b["state"][i]) == ["exp_avg", "exp_avg_sq", "step"]
        for k in ("exp_avg", "exp_avg_sq", "step"):
            assert a["state"][i][k].shape == b["state"][i][k].shape and a["state"][i][k].dtype == b["state"][i][k].dtype, (i, k)
        assert float(a["state"][i]["step"]) == 0.0
    for ga, gb in zip(a["param_groups"], b["param_groups"]):
        assert ga["params"] == gb["params"]
        assert set(gb) <= set(ga)                                            # every key torch.optim.Adam.load_state_dict will look for
        assert ga["lr"] == gb["lr"] and tuple(ga["betas"]) == tuple(gb["betas"]) and ga["eps"] == gb["eps"]
        assert ga["initial_lr"] == gb["lr"] and ga["lr_decay_exp"] == 0.1
    # ... so each loads into the other (values: tests/test_device_adam_gpu.py)
    theirs.load_state_dict(a)
    mine.load_state_dict(b)
    assert mine.counters() == (1, 0)
    st = mine.state[groups[0]["params"][0]]
    assert torch.equal(st["exp_avg"], b["state"][0]["exp_avg"]) and float(st["exp_avg"].abs().max()) > 0
    mine.set_iteration(123456)
    assert mine.counters() == (1, 123456)
    assert mine.state_dict()["param_groups"][1]["lr"] == pytest.approx(2e-3 * 0.1 ** 0.123456, rel=1e-12)


def test_device_adam_refuses_what_it_does_not_implement():
    from hybridneuralrendering_amd.optim import DeviceAdam, ShellOptimizers
    from hybridneuralrendering_amd._lib import HnrError
    p = torch.nn.Parameter(torch.zeros(4))
    for bad in (dict(weight_decay=0.1), dict(amsgrad=True), dict(maximize=True), dict(lr=-1.0), dict(betas=(0.9, 1.0)), dict(lr_decay_iters=0)):
        with pytest.raises(HnrError):
            DeviceAdam([dict(params=[p], **bad)])
    with pytest.raises(HnrError):
        DeviceAdam([dict(params=[torch.nn.Parameter(torch.zeros(1))]) for _ in range(5)])           # more than 4 groups
    with pytest.raises(HnrError):
        DeviceAdam([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))])
    with pytest.raises(HnrError):
        DeviceAdam([p]).step({p: torch.zeros(4)})                             # CPU tensors: there is no CPU fallback
    # the shell's options
    agg = torch.nn.Linear(3, 2)
    pts = torch.nn.Module()
    pts.xyz = torch.nn.Parameter(torch.zeros(6, 3), requires_grad=False)
    pts.points_embeding = torch.nn.Parameter(torch.zeros(1, 6, 32))
    pts.points_conf = torch.nn.Parameter(torch.zeros(1, 6, 1))
    base = dict(lr=5e-4, plr=2e-3, lr_policy="iter_exponential_decay", lr_decay_exp=0.1, lr_decay_iters=1000000, alter_step=0, feedforward=0)
    for over, word in ((dict(alter_step=100), "alter_step"), (dict(lr_policy="lambda"), "lr_policy"), (dict(feedforward=1), "feedforward")):
        with pytest.raises(HnrError, match=word):
            ShellOptimizers(SimpleNamespace(**dict(base, **over)), agg, pts)
    so = ShellOptimizers(SimpleNamespace(**base), agg, pts, total_steps=77)
    g0, g1 = so.param_groups
    assert [tuple(q.shape) for q in g0["params"]] == [(2, 3), (2,)] and g0["lr"] == 5e-4
    assert g1["params"][0] is pts.points_embeding and g1["params"][1] is pts.points_conf and len(g1["params"]) == 2 and g1["lr"] == 2e-3
    assert all(g["betas"] == (0.9, 0.999) and g["lr_decay_exp"] == 0.1 and g["lr_decay_iters"] == 1000000 for g in (g0, g1))
    assert so.counters() == (0, 77)
    old = so.optimizer
    so.rebuild(500)
    assert so.optimizer is not old and so.counters() == (0, 500)


def test_adam_entry_points_reject_bad_arguments_without_touching_the_gpu():
    """The error convention of include/hnr.h for the optimiser's entries: HNR_ERR_BADARG and a text, before any HIP call."""
    from hybridneuralrendering_amd import _lib
    L = _lib.lib()
    null, bad = None, -1
    one = ctypes.c_void_p(0x1000)                                             # non-NULL, aligned, never dereferenced
    odd = ctypes.c_void_p(0x1004)
    assert L.hnr_adam_step(null, one, 2, one, one, 3, one, 5, null) == bad and b"NULL" in L.hnr_last_error()
    assert L.hnr_adam_step(one, one, 2, one, null, 3, one, 5, null) == bad
    assert L.hnr_adam_step(one, one, 2, one, one, 3, null, 5, null) == bad
    assert L.hnr_adam_step(one, one, 5, one, one, 3, one, 5, null) == bad and b"n_groups" in L.hnr_last_error()       # too many groups
    assert L.hnr_adam_step(one, one, 0, one, one, 3, one, 5, null) == bad
    assert L.hnr_adam_step(one, one, 2, one, one, 0, one, 5, null) == bad and b"n_tensors" in L.hnr_last_error()
    assert L.hnr_adam_step(one, one, 2, one, one, 3, one, -1, null) == bad and b"n_chunks" in L.hnr_last_error()
    assert L.hnr_adam_step(odd, one, 2, one, one, 3, one, 5, null) == bad and b"aligned" in L.hnr_last_error()
    assert L.hnr_adam_step(one, null, 2, one, one, 3, one, 5, null) == bad
    assert L.hnr_adam_step(one, one, 2, null, one, 3, one, 5, null) == bad
    assert L.hnr_adam_step(one, one, -1, one, one, 3, one, 5, null) == bad
    assert L.hnr_adam_step(one, one, 2, one, one, 5000, one, 5, null) == bad
    assert L.hnr_adam_step(one, one, 2, one, one, 3, ctypes.c_void_p(0x1002), 5, null) == bad and b"4-byte" in L.hnr_last_error()
    # the host-side plan: table checks and the chunk count
    tab = (_lib.AdamTensor * 3)()
    for i, n in enumerate((1, _lib.ADAM_CHUNK, 2 * _lib.ADAM_CHUNK + 5)):
        tab[i].p, tab[i].g, tab[i].m, tab[i].v, tab[i].n, tab[i].group = 0x1000, 0x2000, 0x3000, 0x4004, n, i % 2
    assert L.hnr_adam_plan(tab, 3, 2, None, 0) == 1 + 1 + 3
    chunks = (ctypes.c_int32 * 10)()
    assert L.hnr_adam_plan(tab, 3, 2, chunks, 5) == 5
    assert list(chunks) == [0, 0, 1, 0, 2, 0, 2, 1, 2, 2]
    assert L.hnr_adam_plan(tab, 3, 2, chunks, 4) == bad                                                                # table too short
    assert L.hnr_adam_plan(tab, 3, 1, None, 0) == bad and b"group" in L.hnr_last_error()
    assert L.hnr_adam_plan(None, 3, 2, None, 0) == bad
    assert L.hnr_adam_plan(tab, 3, 5, None, 0) == bad
    tab[1].n = -4
    assert L.hnr_adam_plan(tab, 3, 2, None, 0) == bad and b"negative" in L.hnr_last_error()
    tab[1].n, tab[2].g = 4, None
    assert L.hnr_adam_plan(tab, 3, 2, None, 0) == bad and b"NULL" in L.hnr_last_error()
    tab[2].g = 0x2002
    assert L.hnr_adam_plan(tab, 3, 2, None, 0) == bad and b"4-byte" in L.hnr_last_error()
    # the ctypes mirror has the header's layout
    assert ctypes.sizeof(_lib.AdamTensor) == 48 and _lib.AdamTensor.n.offset == 32 and _lib.AdamTensor.group.offset == 40
