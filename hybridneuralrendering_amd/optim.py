"""The optimiser step and the learning-rate schedule on the device (csrc/adam.hip): every tensor of every parameter group in ONE launch behind a
single-thread tick launch, capturable, no host value in a step.

    DeviceAdam        <- the two torch.optim.Adam of the reference's setup_optimizer (models/mvs_points_volumetric_model.py:94-104), their
                         .step() calls (:111-131) and the LambdaLR scheduler of lr_policy 'iter_exponential_decay'
                         (models/helpers/networks.py:56-61, stepped at models/base_model.py:148-150)
    ShellOptimizers   <- setup_optimizer + init_scheduler for the shipped configuration (feedforward=0), and what run/train_ft.py:868-874 does with
                         them after prune / grow_points

Arithmetic (tests/adam_ref.py restates it): fp32, every operation rounded on its own, in the order of torch's _single_tensor_adam --
m' = m + w1 (g - m);  v' = v b2 + (w2 g) g;  den = sqrt(v') / bs + e;  p' = p - ss (m' / den) -- with the six scalars rounded once from the fp64
row the tick kernel wrote (lr_t / bc1, sqrt(bc2), ...).  No weight decay, no amsgrad, no maximize: the reference uses none, and a group that asks
for one is refused.

The step writes parameter memory behind torch's back, and the renderer caches values derived from the parameters: `step()` marks every parameter
it wrote (_cache.py, rule 3); after a graph replay that contains the step, `mark_updated()` does (CapturedTrainStep.step calls it).

One step counter per optimiser (`adam_step`), not one per parameter: a parameter that never receives a gradient is skipped, like in torch; one that
receives its FIRST gradient at a later step would get that step's bias correction where torch starts its own count at 1 -- no shipped configuration
does that (the parameters without a gradient -- `color_branch`, the image branch under use_nearest=0 -- never get one).
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._cache import mark_written
from ._lib import HnrError

_DEFAULTS = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, lr_decay_exp=1.0, lr_decay_iters=1)


def schedule_factor(it, lr_decay_exp, lr_decay_iters):
    """lambda_rule of 'iter_exponential_decay' (models/helpers/networks.py:57-59); `it` = scheduler.step() calls so far."""
    return pow(lr_decay_exp, it / lr_decay_iters)


class DeviceAdam:
    """param_groups: an iterable of tensors or of torch.optim.Adam's group dicts (`params`, `lr`, `betas`, `eps`) with two more keys,
    `lr_decay_exp` / `lr_decay_iters` (default 1.0 / 1: constant lr), and optionally `names` (one per parameter: the keys an explicit gradient
    mapping is looked up by).  At most 4 groups.  Parameters are contiguous fp32 tensors; `step` needs them on the GPU, everything else
    (construction, state_dict, load_state_dict) works wherever they live.

    The group dicts are read at construction and by load_state_dict; after changing one by hand call `sync_groups()`."""

    def __init__(self, param_groups):
        groups = list(param_groups)
        if not groups:
            raise HnrError("DeviceAdam: empty parameter list")
        if not isinstance(groups[0], dict):
            groups = [dict(params=groups)]
        if len(groups) > _lib.ADAM_MAX_GROUPS:
            raise HnrError("DeviceAdam: at most %d parameter groups, got %d" % (_lib.ADAM_MAX_GROUPS, len(groups)))
        self.param_groups, self._names = [], []
        seen = set()
        for gi, g in enumerate(groups):
            g = dict(g)
            names = g.pop("names", None)
            g["params"] = list(g["params"])
            for k in ("weight_decay", "amsgrad", "maximize"):
                if g.get(k):
                    raise HnrError("DeviceAdam: %s is not implemented (the reference's optimisers use none)" % k)
            for k, v in _DEFAULTS.items():
                g.setdefault(k, v)
            if names is not None and len(names) != len(g["params"]):
                raise HnrError("DeviceAdam: group %d has %d names for %d parameters" % (gi, len(names), len(g["params"])))
            for p in g["params"]:
                if not isinstance(p, torch.Tensor) or p.dtype != torch.float32 or not p.is_contiguous():
                    raise HnrError("DeviceAdam: parameters must be contiguous float32 tensors")
                if id(p) in seen:
                    raise HnrError("DeviceAdam: a parameter appears in more than one group")
                seen.add(id(p))
            self._check_group(gi, g)
            self.param_groups.append(g)
            self._names.append(list(names) if names is not None else None)
        params = [p for g in self.param_groups for p in g["params"]]
        if not params:
            raise HnrError("DeviceAdam: no parameters")
        if len(params) > _lib.ADAM_MAX_TENSORS:
            raise HnrError("DeviceAdam: at most %d tensors, got %d" % (_lib.ADAM_MAX_TENSORS, len(params)))
        self.device = params[0].device
        if any(p.device != self.device for p in params):
            raise HnrError("DeviceAdam: all parameters must live on one device")
        # state: first / second moment per parameter; {adam_step, sched_it}; the groups' hyper-parameters; the row the tick kernel writes
        self.state = {p: dict(exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p)) for p in params}
        self._counters = torch.zeros((2,), dtype=torch.int64, device=self.device)
        self._groups = torch.zeros((len(self.param_groups), _lib.ADAM_GROUP_DOUBLES), dtype=torch.float64, device=self.device)
        self._rows = torch.zeros((len(self.param_groups), _lib.ADAM_ROW_DOUBLES), dtype=torch.float64, device=self.device)
        self.sync_groups()
        self._tkey = self._ckey = None
        self._tensors = self._chunks = None
        self._n_tensors = self._n_chunks = 0
        self._written = []
        self._warm = False

    @staticmethod
    def _check_group(gi, g):
        b1, b2 = (float(b) for b in g["betas"])
        if not (float(g["lr"]) >= 0.0 and 0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0 and float(g["eps"]) >= 0.0):
            raise HnrError("DeviceAdam: group %d: need lr >= 0, 0 <= beta < 1, eps >= 0" % gi)
        if not (float(g["lr_decay_exp"]) > 0.0 and float(g["lr_decay_iters"]) > 0.0):
            raise HnrError("DeviceAdam: group %d: lr_decay_exp and lr_decay_iters must be positive" % gi)

    def sync_groups(self):
        """Uploads the groups' hyper-parameters (lr = the schedule's base rate lr0) to the device rows the tick kernel reads."""
        rows = []
        for gi, g in enumerate(self.param_groups):
            self._check_group(gi, g)
            rows.append([float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["lr_decay_exp"]), float(g["lr_decay_iters"])])
        self._groups.copy_(torch.tensor(rows, dtype=torch.float64))

    # ------------------------------------------------------------------------------------------------ the step
    def _gradient_list(self, grads):
        out = []
        for gi, g in enumerate(self.param_groups):
            names = self._names[gi]
            for pi, p in enumerate(g["params"]):
                if grads is None:
                    gr = p.grad
                else:
                    gr = grads.get(names[pi]) if names is not None else None
                    if gr is None and names is None:
                        gr = grads.get(p)
                if gr is None or p.numel() == 0:
                    continue                                       # no gradient: skipped, as torch.optim.Adam does
                if not (isinstance(gr, torch.Tensor) and gr.dtype == torch.float32 and gr.is_contiguous() and gr.device == p.device):
                    raise HnrError("DeviceAdam.step: a gradient must be a contiguous float32 tensor on the parameter's device")
                if gr.numel() != p.numel():
                    raise HnrError("DeviceAdam.step: a gradient has %d elements, its parameter %d" % (gr.numel(), p.numel()))
                out.append((p, gr, gi))
        if not out:
            raise HnrError("DeviceAdam.step: no parameter has a gradient")
        return out

    def _prepare(self, todo):
        """The device tables for this (parameter, gradient) set: the tensor table follows the pointers, the chunk table the sizes.  Rebuilt only
        when one of them changes (never under TrainPath.reuse_outputs or a captured step)."""
        if self.device.type != "cuda":
            raise HnrError("DeviceAdam.step: the parameters must be on the GPU (the HIP path has no CPU fallback)")
        tkey = tuple((p.data_ptr(), g.data_ptr(), gi) for p, g, gi in todo)
        if tkey == self._tkey:
            return
        if torch.cuda.is_current_stream_capturing():
            raise HnrError("DeviceAdam.step: the gradient buffers changed under a graph capture (the descriptor table is a host -> device copy); "
                           "call prepare(grads) with the buffers of the captured step first")
        n = len(todo)
        tab = (_lib.AdamTensor * n)()
        for i, (p, g, gi) in enumerate(todo):
            st = self.state[p]
            tab[i].p, tab[i].g, tab[i].m, tab[i].v = p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
            tab[i].n, tab[i].group = p.numel(), gi
        ckey = tuple((p.numel(), gi) for p, g, gi in todo)
        ng = len(self.param_groups)
        if ckey != self._ckey:
            nc = _lib.size("hnr_adam_plan", tab, n, ng, None, 0)
            chunks = np.zeros((max(nc, 1), 2), dtype=np.int32)
            nc = _lib.size("hnr_adam_plan", tab, n, ng, chunks.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), nc)
            self._chunks, self._n_chunks, self._ckey = torch.from_numpy(chunks).to(self.device), nc, ckey
        else:
            _lib.size("hnr_adam_plan", tab, n, ng, None, 0)
        raw = np.frombuffer(tab, dtype=np.uint8).copy()
        self._tensors = torch.from_numpy(raw).to(self.device)          # (torch allocations are at least 256-byte aligned)
        self._n_tensors, self._tkey = n, tkey
        self._written = [p for p, _g, _gi in todo]

    def prepare(self, grads=None):
        """Everything of a step that is not capturable, ahead of a capture: the descriptor tables for these gradient buffers, and the first
        launch of the two kernels (on private one-element buffers: nothing of the optimiser's state moves)."""
        self._prepare(self._gradient_list(grads))
        if not self._warm:
            dev = self.device
            z = torch.zeros((4, 4), dtype=torch.float32, device=dev)
            t = (_lib.AdamTensor * 1)()
            t[0].p, t[0].g, t[0].m, t[0].v, t[0].n, t[0].group = z[0].data_ptr(), z[1].data_ptr(), z[2].data_ptr(), z[3].data_ptr(), 1, 0
            dt = torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).to(dev)
            ch = torch.zeros((1, 2), dtype=torch.int32, device=dev)
            cnt, rows = torch.zeros((2,), dtype=torch.int64, device=dev), torch.zeros((1, _lib.ADAM_ROW_DOUBLES), dtype=torch.float64, device=dev)
            _lib.call("hnr_adam_step", cnt, self._groups, 1, rows, dt, 1, ch, 1, _lib.STREAM)
            torch.cuda.current_stream(dev).synchronize()            # (the private buffers die here)
            self._warm = True

    def step(self, grads=None):
        """One optimiser step on the current stream: the tick launch, then the update launch.  grads: a mapping (by the group's `names`, else by
        parameter) of gradient tensors read in place -- train_step's `pg` / `ag` dictionaries merged -- or None: the parameters' .grad fields."""
        self._prepare(self._gradient_list(grads))
        _lib.call("hnr_adam_step", self._counters, self._groups, len(self.param_groups), self._rows, self._tensors, self._n_tensors, self._chunks,
                  self._n_chunks, _lib.STREAM)
        self._warm = True
        self.mark_updated()

    def mark_updated(self):
        """Every parameter the last prepared step writes counts as modified in place (_cache.py, rule 3)."""
        mark_written(self._written)

    def zero_grad(self, set_to_none=True):
        for g in self.param_groups:
            for p in g["params"]:
                if p.grad is not None:
                    if set_to_none:
                        p.grad = None
                    else:
                        p.grad.detach_().zero_()

    def set_iteration(self, total_steps):
        """init_scheduler(total_steps) (models/mvs_points_volumetric_model.py:225-232: total_steps scheduler.step() calls): the next step runs with
        lr0 * lr_decay_exp^(total_steps / lr_decay_iters)."""
        if int(total_steps) < 0:
            raise HnrError("DeviceAdam.set_iteration: total_steps must be >= 0")
        self._counters[1:2].fill_(int(total_steps))

    def scalars(self):
        """The device rows [groups, 10] fp64 the last tick wrote: lr_t, bc1, bc2, lr_t / bc1, sqrt(bc2), 1 - beta1, 1 - beta2, beta2, eps, step."""
        return self._rows

    def counters(self):
        """(adam_step, sched_it) read from the device (a host synchronisation)."""
        c = self._counters.cpu()
        return int(c[0]), int(c[1])

    # ------------------------------------------------------------------------------------------------ state dict (torch.optim.Adam's layout)
    def state_dict(self):
        """torch.optim.Adam's layout: state[i] = {step, exp_avg, exp_avg_sq}, param_groups with `params` as indices.  A group's `lr` is the rate of
        the NEXT step and `initial_lr` the schedule's base rate, as LambdaLR leaves them; torch's remaining keys carry its defaults, so the
        dictionary loads into torch.optim.Adam.  Reads the counters (a host synchronisation)."""
        step, it = self.counters()
        extra = {k: v for k, v in torch.optim.Adam([torch.zeros(1)]).defaults.items() if k not in ("lr", "betas", "eps")}
        state, groups, i = {}, [], 0
        for g in self.param_groups:
            idx = []
            for p in g["params"]:
                st = self.state[p]
                state[i] = dict(step=torch.tensor(float(step), dtype=torch.float32), exp_avg=st["exp_avg"], exp_avg_sq=st["exp_avg_sq"])
                idx.append(i)
                i += 1
            d = dict(extra)
            d.update({k: v for k, v in g.items() if k != "params"})
            d["initial_lr"] = float(g["lr"])
            d["lr"] = float(g["lr"]) * schedule_factor(it, float(g["lr_decay_exp"]), float(g["lr_decay_iters"]))
            d["params"] = idx
            groups.append(d)
        return dict(state=state, param_groups=groups)

    def load_state_dict(self, sd):
        """A state saved by this class or by torch.optim.Adam over the same groups.  torch counts steps per parameter: they must agree.  The
        schedule's iteration is not part of an optimiser state (torch keeps it in the scheduler): set_iteration()."""
        groups = sd["param_groups"]
        if len(groups) != len(self.param_groups) or any(len(a["params"]) != len(b["params"]) for a, b in zip(groups, self.param_groups)):
            raise HnrError("DeviceAdam.load_state_dict: the parameter groups do not match")
        params = [p for g in self.param_groups for p in g["params"]]
        steps = set()
        for i, p in enumerate(params):
            st = sd["state"].get(i)
            if st is None:
                continue
            if tuple(st["exp_avg"].shape) != tuple(p.shape) or tuple(st["exp_avg_sq"].shape) != tuple(p.shape):
                raise HnrError("DeviceAdam.load_state_dict: state %d does not have its parameter's shape" % i)
            steps.add(int(round(float(st["step"]))))
        if len(steps) > 1:
            raise HnrError("DeviceAdam.load_state_dict: the parameters carry different step counts %s; this optimiser keeps one" % sorted(steps))
        for a, g in zip(groups, self.param_groups):
            for k in ("weight_decay", "amsgrad", "maximize"):
                if a.get(k):
                    raise HnrError("DeviceAdam.load_state_dict: %s is not implemented" % k)
            g["lr"] = float(a.get("initial_lr", a["lr"]))
            g["betas"], g["eps"] = tuple(float(b) for b in a["betas"]), float(a["eps"])
            g["lr_decay_exp"], g["lr_decay_iters"] = a.get("lr_decay_exp", g["lr_decay_exp"]), a.get("lr_decay_iters", g["lr_decay_iters"])
        self.sync_groups()
        with torch.no_grad():
            for i, p in enumerate(params):
                st = sd["state"].get(i)
                mine = self.state[p]
                if st is None:
                    mine["exp_avg"].zero_(); mine["exp_avg_sq"].zero_()
                else:
                    mine["exp_avg"].copy_(st["exp_avg"]); mine["exp_avg_sq"].copy_(st["exp_avg_sq"])
        self._counters[0:1].fill_(steps.pop() if steps else 0)


def merge_grads(pg, ag):
    """train_step's two gradient dictionaries as the one mapping DeviceAdam.step reads (point buffers by attribute name, weights by parameter name)."""
    d = dict(ag)
    d.update(pg)
    return d


class ShellOptimizers:
    """The reference's setup_optimizer + init_scheduler for the shipped configuration (feedforward=0), as ONE DeviceAdam:
    group 0 = the aggregator's parameters at opt.lr, group 1 = the neural_points parameters that require grad at opt.plr; betas (0.9, 0.999),
    lr_decay_exp / lr_decay_iters from opt.  `step(grads)` / `prepare` / `mark_updated` / `scalars` / `state_dict` ... are the optimiser's."""

    def __init__(self, opt, aggregator, neural_points, total_steps=0):
        if getattr(opt, "alter_step", 0) != 0:
            raise HnrError("ShellOptimizers: alter_step != 0 (alternating optimiser steps) is not implemented; no shipped script sets it")
        if getattr(opt, "feedforward", 0) != 0:
            raise HnrError("ShellOptimizers: feedforward != 0 (the mvs optimiser in place of the point optimiser) is not implemented")
        for k in ("lr", "plr", "lr_policy", "lr_decay_exp", "lr_decay_iters"):
            if not hasattr(opt, k):
                raise HnrError("ShellOptimizers: the options carry no %s" % k)
        if opt.lr_policy != "iter_exponential_decay":
            raise HnrError("ShellOptimizers: lr_policy %r is not implemented (every shipped script trains with iter_exponential_decay)" % (opt.lr_policy,))
        self.opt, self.aggregator, self.neural_points = opt, aggregator, neural_points
        self.optimizer = None
        self.rebuild(total_steps)

    def rebuild(self, total_steps=0):
        """After neural_points.prune / grow_points (run/train_ft.py:868-874: setup_optimizer + init_scheduler(total_steps)): fresh zero state for the
        buffers as they are now, adam_step = 0, the schedule at total_steps.  A CapturedTrainStep over the old buffers has to be rebuilt too."""
        opt = self.opt
        common = dict(betas=(0.9, 0.999), lr_decay_exp=float(opt.lr_decay_exp), lr_decay_iters=float(opt.lr_decay_iters))
        net = [(n, p) for n, p in self.aggregator.named_parameters()]
        pts = [(n, p) for n, p in self.neural_points.named_parameters() if p.requires_grad]
        groups = []
        for lr, named in ((float(opt.lr), net), (float(opt.plr), pts)):
            if named:
                groups.append(dict(params=[p for _n, p in named], names=[n for n, _p in named], lr=lr, **common))
        self.optimizer = DeviceAdam(groups)
        self.optimizer.set_iteration(int(total_steps))
        return self.optimizer

    def __getattr__(self, name):
        if name in ("step", "prepare", "mark_updated", "zero_grad", "set_iteration", "scalars", "counters", "state_dict", "load_state_dict", "param_groups"):
            return getattr(self.optimizer, name)
        raise AttributeError(name)
