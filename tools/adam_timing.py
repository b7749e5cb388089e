"""Times the device optimiser step (hybridneuralrendering_amd/optim.py; csrc/adam.hip) at the bench scale against torch.optim.Adam on buffers of
the same sizes on the same GPU.

  python tools/adam_timing.py [--out profiles/adam_timing.txt] [--points 2e6]

Steps (each a child process under its own time limit; the parent opens no GPU and stops at the first step that fails):
  optimizer   one whole optimiser step over the four point buffers (N x (32 + 1 + 3 + 3) floats) and the aggregator's parameter list, two groups:
              DeviceAdam (tick + one update launch) against torch.optim.Adam in three forms -- default, foreach=False, fused=True -- each on its own
              copy of the buffers, with .grad already in place (the clone train._assign_grads makes under reuse_outputs is NOT charged to torch).
              Medians of five alternating windows of about one second of back-to-back steps, device events; effective bandwidth = 28 B x elements /
              time (read p, g, m, v, write p, m, v) beside the ~6 TB/s the chip streams.  Before timing, one step of every form from the same state is
              compared with the device's.
  c3          the bench's C3 training step (56 x 56 rays, 2 M points, reuse_outputs) with the optimiser inside -- train_step(..., optimizer=) --
              against the same step followed by the two torch.optim.Adam steps the reference's shell runs (default form, .grad assigned without a
              copy), and the step alone.
"""
import argparse
import json
import math
import os
import subprocess
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEPS = (("optimizer", 420), ("c3", 420))
HBM_STREAM_TBS = 6.0


def alternating(fns, reps=5, target_ms=1000.0):
    """{name: (median ms per call, windows, calls per window)}: `reps` rounds, in each round one window of about target_ms per entry, in order."""
    import torch

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / calls
    calls = {k: max(1, int(math.ceil(target_ms / max(timed(fn, 3), 1e-3)))) for k, fn in fns.items()}
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            out[k].append(timed(fn, calls[k]))
    return {k: (sorted(v)[len(v) // 2], [round(x, 4) for x in v], calls[k]) for k, v in out.items()}


def _buffers(n_points, dev, seed):
    """([(name, tensor)] aggregator parameters, [(name, tensor)] point buffers) with the bench's sizes; seeded values."""
    import torch
    from hybridneuralrendering_amd import scenes
    from hybridneuralrendering_amd.aggregator import PointAggregator
    torch.manual_seed(seed)
    agg = PointAggregator(scenes.scene_opt("scene0241")).to(dev)
    net = [(n, p.detach().clone()) for n, p in agg.named_parameters()]
    g = torch.Generator(device="cpu").manual_seed(seed)
    pts = [(n, (torch.randn((1, n_points, c), generator=g) * 0.3).to(dev)) for n, c in (("points_embeding", 32), ("points_conf", 1), ("points_dir", 3),
                                                                                         ("points_color", 3))]
    return net, pts


def step_optimizer(n_points):
    import torch
    from hybridneuralrendering_amd.optim import DeviceAdam
    dev = torch.device("cuda:0")
    net, pts = _buffers(n_points, dev, 0)
    gen = torch.Generator(device="cpu").manual_seed(1)
    grads = {n: (torch.randn(p.shape, generator=gen) * 1e-3).to(dev) for n, p in net + pts}
    elements = sum(p.numel() for _n, p in net + pts)
    lr, plr = 5e-4, 2e-3
    ours = DeviceAdam([dict(params=[p for _n, p in net], names=[n for n, _p in net], lr=lr), dict(params=[p for _n, p in pts], names=[n for n, _p in pts], lr=plr)])
    forms = dict(torch_default={}, torch_single=dict(foreach=False), torch_fused=dict(fused=True))
    theirs = {}
    for k, kw in forms.items():
        a = [torch.nn.Parameter(p.clone()) for _n, p in net]
        b = [torch.nn.Parameter(p.clone()) for _n, p in pts]
        for q, (n, _p) in zip(a + b, net + pts):
            q.grad = grads[n]
        theirs[k] = (a + b, [torch.optim.Adam(a, lr=lr, betas=(0.9, 0.999), **kw), torch.optim.Adam(b, lr=plr, betas=(0.9, 0.999), **kw)])
    fns = dict(device=lambda: ours.step(grads))
    for k, (_q, opts) in theirs.items():
        fns[k] = (lambda o: (lambda: (o[0].step(), o[1].step())))(opts)
    # one step of every form from the same state: the forms agree with the device step
    diff = {}
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    for k, (q, _o) in theirs.items():
        diff[k] = max(float((x.detach() - p).abs().max()) for x, (_n, p) in zip(q, net + pts))
        assert diff[k] <= 1e-6, "the device step and %s disagree after one step: %g" % (k, diff[k])
    for _ in range(2):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    res = alternating(fns)
    rec = dict(step="optimizer", what="one optimiser step: %d points x 39 floats + %d aggregator tensors = %d elements, two groups" % (n_points, len(net), elements),
               elements=elements, bytes_per_step=28 * elements, hbm_stream_tbs=HBM_STREAM_TBS)
    for k, (med, wins, calls) in res.items():
        rec[k + "_ms"], rec[k + "_windows_ms"], rec[k + "_calls_per_window"] = round(med, 4), wins, calls
        rec[k + "_tbs"] = round(28 * elements / (med * 1e-3) / 1e12, 3)
    fastest = min((k for k in res if k != "device"), key=lambda k: res[k][0])
    rec.update(fastest_torch=fastest, fastest_torch_over_device=round(res[fastest][0] / res["device"][0], 3), max_abs_difference_after_one_step=diff,
               device_not_slower=bool(res["device"][0] <= res[fastest][0]))
    print("RESULT " + json.dumps(rec), flush=True)


def step_c3(n_points):
    import numpy as np
    import torch
    from hnr_bench.common import build_world
    from hybridneuralrendering_amd import scenes
    from hybridneuralrendering_amd.optim import DeviceAdam
    from hybridneuralrendering_amd.train import TrainPath, train_step
    dev = torch.device("cuda:0")
    args = SimpleNamespace(scene="scene0241", points=n_points, width=640, height=480, margin=10, knn_order=None)
    sc, opt, agg, cloud, rnd, cam = build_world(args, dev, 0)
    opt.is_train = 1
    rng = np.random.default_rng(17)
    x0, y0 = int(rng.integers(args.margin, sc.w - args.margin - 56)), int(rng.integers(args.margin, sc.h - args.margin - 56))
    px, py = np.meshgrid(np.arange(x0, x0 + 56), np.arange(y0, y0 + 56), indexing="ij")
    pix = np.stack([px, py], axis=-1).reshape(-1, 2).astype(np.int32)
    raydir = torch.from_numpy(scenes.camera_rays(pix, sc.intrinsic, sc.c2w)).to(dev)
    gt = torch.rand((raydir.shape[0], 3), device=dev)
    w2c = torch.inverse(cam["c2w_nearest"]).contiguous()
    names = ("points_embeding", "points_conf", "points_dir", "points_color")

    def world():
        """its own renderer-independent copies: leaves, an aggregator sharing nothing with the other side, a path with reused buffers"""
        from hybridneuralrendering_amd.aggregator import PointAggregator
        from hybridneuralrendering_amd.render import HybridRenderer
        a = PointAggregator(opt)
        a.load_state_dict({k: v.detach().clone() for k, v in agg.state_dict().items()})
        a = a.to(dev)
        for prm in a.parameters():
            prm.requires_grad_(True)
        r = HybridRenderer(opt, a, dev)
        path = TrainPath(r)
        path.reuse_outputs = True
        leaves = [t.clone().requires_grad_(True) for t in (cloud.emb, cloud.conf, cloud.dir, cloud.color)]
        return a, path, leaves

    def one(a, path, leaves, **kw):
        return train_step(path, a, cloud.xyz, leaves[0], leaves[1], leaves[2], leaves[3], raydir, cam["campos"], cam["camrot"], cam["bg"], sc.near, sc.far,
                          cam["c2w_nearest"], cam["campos_nearest"], cam["intrinsic"], cam["images"], gt, zero_epsilon=1e-3, w_color=1.0, w_zero_one=1e-4,
                          w2c_nearest=w2c, **kw)
    a1, p1, l1 = world()
    named = list(a1.named_parameters())
    ours = DeviceAdam([dict(params=[q for _n, q in named], names=[n for n, _q in named], lr=5e-4, lr_decay_exp=0.1, lr_decay_iters=1000000),
                       dict(params=l1, names=list(names), lr=2e-3, lr_decay_exp=0.1, lr_decay_iters=1000000)])
    a2, p2, l2 = world()
    t_net = torch.optim.Adam(list(a2.parameters()), lr=5e-4, betas=(0.9, 0.999))
    t_pts = torch.optim.Adam(l2, lr=2e-3, betas=(0.9, 0.999))
    a3, p3, l3 = world()

    def with_device():
        one(a1, p1, l1, optimizer=ours)

    def with_torch():
        # .grad = the step's own buffers (accumulate_grads=False: no 312 MB clone), then the shell's two steps
        one(a2, p2, l2, accumulate_grads=False)
        t_net.step(); t_pts.step()

    def step_alone():
        one(a3, p3, l3, assign_grads=False)
    fns = dict(step_with_device_adam=with_device, step_with_torch_adam=with_torch, step_alone=step_alone)
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    res = alternating(fns)
    rec = dict(step="c3", what="C3 training step (3136 rays, %d points, eager, reuse_outputs): with the device optimiser inside / followed by the two "
               "torch.optim.Adam steps / alone" % n_points)
    for k, (med, wins, calls) in res.items():
        rec[k + "_ms"], rec[k + "_windows_ms"], rec[k + "_calls_per_window"] = round(med, 4), wins, calls
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    ap.add_argument("--out", default=None)
    ap.add_argument("--points", type=float, default=2.0e6)
    ap.add_argument("--steps", default=",".join(s for s, _ in STEPS), help="the steps the parent runs, comma-separated")
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "adam_timing needs a GPU: there is no CPU fallback and no CPU timing"
        dict(optimizer=step_optimizer, c3=step_c3)[args.step](int(args.points))
        return 0
    lines = []
    for step, limit in STEPS:
        if step not in args.steps.split(","):
            continue
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--points", str(args.points)], capture_output=True, text=True,
                               timeout=limit)
        except subprocess.TimeoutExpired:
            print("step %s passed its time limit of %d s: stopping" % (step, limit))
            return 1
        got = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            print("step %s failed (exit %d): stopping\n%s\n%s" % (step, r.returncode, r.stdout[-1000:], r.stderr[-2000:]))
            return 1
        lines += got
        print(got[0], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/adam_timing.py on one MI355X: medians of five alternating one-second device-event windows; tbs = 28 B x elements / time\n")
            f.write("\n".join(l[len("RESULT "):] for l in lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
