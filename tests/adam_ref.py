"""NumPy restatement of the device optimiser step (csrc/adam.hip, include/hnr.h): the tick's fp64 scalars, and the element update in fp32 (every
operation rounded on its own, the six scalars rounded once from fp64) and in fp64.  Plus the seeded inputs the comparison tests share."""
import math

import numpy as np

f32 = np.float32
ROW = 10        # HNR_ADAM_ROW_DOUBLES: lr_t, bc1, bc2, lr_t / bc1, sqrt(bc2), 1 - beta1, 1 - beta2, beta2, eps, step


def schedule_lr(lr0, decay_exp, decay_iters, it):
    """The rate of the step that runs after `it` scheduler.step() calls (iteration n, 1-based: it = n - 1)."""
    return lr0 * pow(decay_exp, it / decay_iters)


def tick_row(lr0, beta1, beta2, eps, decay_exp, decay_iters, step, it):
    """The row adam_tick_kernel writes for a group: `step` = adam_step AFTER the increment, `it` = sched_it BEFORE it.  Python doubles."""
    lr_t = schedule_lr(lr0, decay_exp, decay_iters, it)
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    return np.array([lr_t, bc1, bc2, lr_t / bc1, math.sqrt(bc2), 1.0 - beta1, 1.0 - beta2, beta2, eps, float(step)], dtype=np.float64)


def update_f32(p, g, m, v, row):
    """One step on fp32 arrays of any (equal) shape with the scalars of `row`; returns (p', m', v').  NumPy rounds every fp32 operation on its
    own; its fp32 sqrt and divide are correctly rounded."""
    p, g, m, v = (np.asarray(a, dtype=f32) for a in (p, g, m, v))
    ss, bs, w1, w2, b2, e = (f32(row[i]) for i in (3, 4, 5, 6, 7, 8))
    with np.errstate(all="ignore"):
        m1 = m + w1 * (g - m)
        v1 = (v * b2) + ((w2 * g) * g)
        den = (np.sqrt(v1) / bs) + e
        p1 = p - ss * (m1 / den)
    assert p1.dtype == f32 and m1.dtype == f32 and v1.dtype == f32
    return p1, m1, v1


def update_f64(p, g, m, v, row):
    """The same expressions in fp64 with the unrounded scalars."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    ss, bs, w1, w2, b2, e = (float(row[i]) for i in (3, 4, 5, 6, 7, 8))
    m1 = m + w1 * (g - m)
    v1 = (v * b2) + ((w2 * g) * g)
    den = (np.sqrt(v1) / bs) + e
    return p - ss * (m1 / den), m1, v1


# ---- the shared comparison case: N rows x F, T steps, sparse per-row gradients over five decades, the schedule well under way
CASE = dict(N=4096, F=32, T=40, lr0=0.002, beta1=0.9, beta2=0.999, eps=1e-8, decay_exp=0.1, decay_iters=1e6, it0=123456)


def case_inputs(seed, N=CASE["N"], F=CASE["F"], T=CASE["T"]):
    """p0 [N,F] and T gradients: g = N(0,1) * 10^U(-6,-1) per row, 15 % of the rows non-zero per step, the first N/8 rows zero at step 0, the last
    N/16 rows never touched."""
    rng = np.random.default_rng(seed)
    p0 = (rng.standard_normal((N, F)) * 0.3).astype(f32)
    gs = []
    for t in range(T):
        g = (rng.standard_normal((N, F)) * 10.0 ** rng.uniform(-6, -1, (N, 1))).astype(f32)
        mask = rng.random((N, 1)) < 0.15
        if t == 0:
            mask[:N // 8] = False
        mask[-(N // 16):] = False
        gs.append((g * mask).astype(f32))
    return p0, gs


def case_row(t):
    """The tick's row for step t (0-based) of the shared case."""
    c = CASE
    return tick_row(c["lr0"], c["beta1"], c["beta2"], c["eps"], c["decay_exp"], c["decay_iters"], t + 1, c["it0"] + t)


_TORCH_RUNS = {}


def torch_case(seed, dtype_name):
    """(p, exp_avg, exp_avg_sq) as NumPy arrays after torch.optim.Adam(foreach=False) ran the shared case in `dtype_name` on the CPU, the group's lr
    set per step as LambdaLR with the reference's lambda_rule sets it.  Computed once per (seed, dtype)."""
    import torch
    key = (seed, dtype_name)
    if key not in _TORCH_RUNS:
        c = CASE
        dt = getattr(torch, dtype_name)
        p0, gs = case_inputs(seed)
        P = torch.nn.Parameter(torch.tensor(p0, dtype=dt))
        o = torch.optim.Adam([P], lr=c["lr0"], betas=(c["beta1"], c["beta2"]), eps=c["eps"], foreach=False)
        for t, g in enumerate(gs):
            for grp in o.param_groups:
                grp["lr"] = schedule_lr(c["lr0"], c["decay_exp"], c["decay_iters"], c["it0"] + t)
            P.grad = torch.tensor(g, dtype=dt)
            o.step()
        st = o.state[P]
        out = tuple(a.detach().numpy().copy() for a in (P, st["exp_avg"], st["exp_avg_sq"]))
        for a in out:
            a.setflags(write=False)
        _TORCH_RUNS[key] = out
    return _TORCH_RUNS[key]


def max_err(a, ref64):
    return float(np.abs(np.asarray(a, dtype=np.float64) - ref64).max())
