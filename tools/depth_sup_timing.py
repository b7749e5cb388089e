"""Times depth supervision (csrc/depth_sup.hip; frames.FrameBank(depth=), train.train_step(gt_depth=, w_depth=)) at the bench's C3 training shape.

  python tools/depth_sup_timing.py [--out profiles/depth_sup_timing.txt] [--points 2e6]

Steps (each a child process under its own time limit; the parent opens no GPU and stops at the first step that fails):
  kernels   a bank of 200 depth frames of 480 x 640 (uint16, 123 MB) and a batch of 56 x 56 rays: the lookup launch alone (hnr_frame_depth_rays) and
            the loss launch alone (hnr_depth_loss, value + gradient + the add into the total), each beside its torch form without a host read -- an
            advanced-index gather, a division and two range tests; a masked mean and its gradient written with torch.where.
  c3        the bench's C3 training step (56 x 56 rays, 2 M points, reuse_outputs) as train_step(optimizer=DeviceAdam): with gt_depth, without it
            (the step as it was before depth supervision), and the same iteration in the autograd form -- render_train(want_depth=True), the three
            loss terms as torch expressions on its outputs, backward(), DeviceAdam.step() on .grad.  Each form has its own parameters and an
            optimiser with lr = 0 (the full update runs, the scene stays the same for all forms).  `--step c3 --only FORM --calls N` runs one form
            N times: under `rocprofv3 --kernel-trace --stats` that attributes the difference to launches.
Medians of five alternating windows of about one second of back-to-back calls, device events; the windows are printed (their spread is the noise).
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

STEPS = (("kernels", 300), ("c3", 480))
W_DEPTH = 0.1


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


def _record(rec, res):
    for k, (med, wins, calls) in res.items():
        rec[k + "_ms"], rec[k + "_windows_ms"], rec[k + "_calls_per_window"] = round(med, 5), wins, calls
        rec[k + "_spread_ms"] = round(max(wins) - min(wins), 5)
    print("RESULT " + json.dumps(rec), flush=True)


def step_kernels(_n_points):
    import ctypes
    import torch
    from hybridneuralrendering_amd import _lib
    dev = torch.device("cuda:0")
    L = _lib.lib()
    Fr, H, W, S = 200, 480, 640, 56
    R = S * S
    g = torch.Generator(device=dev).manual_seed(0)
    depth = torch.randint(0, 9000, (Fr, H, W), generator=g, device=dev, dtype=torch.int32).to(torch.int16)
    bank = _lib.DepthBankC(_lib.ptr(depth), None, 0, Fr, H, W, 1000.0, 0.3, 8.0)
    row = torch.tensor([137], dtype=torch.int32, device=dev)
    pix = torch.stack([torch.randint(10, W - 10, (R,), generator=g, device=dev), torch.randint(10, H - 10, (R,), generator=g, device=dev)], -1).float().contiguous()
    gt = torch.empty((R,), dtype=torch.float32, device=dev)
    P = _lib.ptr

    def lookup():
        L.hnr_frame_depth_rays(ctypes.byref(bank), P(row), P(pix), None, R, P(gt), _lib.stream())

    def lookup_torch():
        r = depth[row.long(), pix[:, 1].long(), pix[:, 0].long()].float() / 1000.0
        return torch.where((r >= 0.3) & (r <= 8.0), r, torch.zeros_like(r))
    lookup()
    torch.cuda.synchronize()
    ref = lookup_torch()                                          # (values >= 32768 do not occur in this bank: int16 reads as the raw value)
    # (torch's division is not correctly rounded: a raw 300 or 8000 may fall on the other side of the range there)
    assert float(((gt - ref).abs() > 1e-6).float().mean()) < 2e-3 and float((gt > 0).float().mean()) > 0.5, "the lookup disagrees with its torch form"
    D = (gt + 0.2 * torch.randn((R,), generator=g, device=dev)).contiguous()
    mask = (torch.rand((R,), generator=g, device=dev) > 0.2).to(torch.int8)
    total, out3, gd = torch.zeros((4,), device=dev), torch.empty((3,), device=dev), torch.empty((R,), device=dev)

    def loss():
        L.hnr_depth_loss(P(D), P(gt), P(mask), R, W_DEPTH, P(total), P(out3), P(gd), None, _lib.stream())

    def loss_torch():
        m = (mask > 0) & (gt > 0)
        n = m.sum().clamp(min=1).float()
        e = D - gt
        lv = torch.where(m, e * e, torch.zeros_like(e)).sum() / n
        total[0] += W_DEPTH * lv
        return lv, torch.where(m, e * (2.0 * W_DEPTH / n), torch.zeros_like(e))
    loss()
    torch.cuda.synchronize()
    lv, gr = loss_torch()
    assert abs(float(out3[0]) - float(lv)) <= 1e-5 * float(lv) and float((gd - gr).abs().max()) <= 1e-6, "the loss disagrees with its torch form"
    fns = dict(lookup=lookup, lookup_torch=lookup_torch, loss=loss, loss_torch=loss_torch)
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    res = alternating(fns)
    rec = dict(step="kernels", what="%d rays; bank of %d depth frames %d x %d uint16 (%.0f MB): hnr_frame_depth_rays alone, hnr_depth_loss alone (value, gradient, "
               "total += w L), each beside its torch form without a host read" % (R, Fr, H, W, depth.numel() * 2 / 1e6),
               lookup_not_slower_than_torch=bool(res["lookup"][0] <= res["lookup_torch"][0]), loss_not_slower_than_torch=bool(res["loss"][0] <= res["loss_torch"][0]))
    _record(rec, res)


def step_c3(n_points, only=None, calls=20):
    import numpy as np
    import torch
    from hnr_bench.common import build_world
    from hybridneuralrendering_amd import scenes
    from hybridneuralrendering_amd.optim import DeviceAdam
    from hybridneuralrendering_amd.train import TrainPath, train_step, render_train
    dev = torch.device("cuda:0")
    args = SimpleNamespace(scene="scene0241", points=n_points, width=640, height=480, margin=10, knn_order=None)
    sc, opt, agg, cloud, rnd, cam = build_world(args, dev, 0)
    opt.is_train = 1
    rng = np.random.default_rng(17)
    x0, y0 = int(rng.integers(args.margin, sc.w - args.margin - 56)), int(rng.integers(args.margin, sc.h - args.margin - 56))
    px, py = np.meshgrid(np.arange(x0, x0 + 56), np.arange(y0, y0 + 56), indexing="ij")
    pix = np.stack([px, py], axis=-1).reshape(-1, 2).astype(np.int32)
    raydir = torch.from_numpy(scenes.camera_rays(pix, sc.intrinsic, sc.c2w)).to(dev)
    R = int(raydir.shape[0])
    gt = torch.rand((R, 3), device=dev)
    gd = rng.uniform(float(sc.near), float(sc.far), size=R).astype(np.float32)
    gd[rng.uniform(size=R) < 0.25] = 0.0
    gt_depth = torch.from_numpy(gd).to(dev)
    w2c = torch.inverse(cam["c2w_nearest"]).contiguous()
    names = ("points_embeding", "points_conf", "points_dir", "points_color")

    def world():
        from hybridneuralrendering_amd.aggregator import PointAggregator
        from hybridneuralrendering_amd.render import HybridRenderer
        a = PointAggregator(opt)
        a.load_state_dict({k: v.detach().clone() for k, v in agg.state_dict().items()})
        a = a.to(dev)
        for prm in a.parameters():
            prm.requires_grad_(True)
        path = TrainPath(HybridRenderer(opt, a, dev))
        path.reuse_outputs = True
        leaves = [t.clone().requires_grad_(True) for t in (cloud.emb, cloud.conf, cloud.dir, cloud.color)]
        named = list(a.named_parameters())
        # lr = 0: the optimiser step runs in full (same launches, same bytes) but the parameters stay, so every form renders the SAME scene in every
        # window -- with a moving scene the forms' sample counts drift apart and the drift (~0.1 ms) hides the ~0.02 ms the depth term costs
        adam = DeviceAdam([dict(params=[q for _n, q in named], names=[n for n, _q in named], lr=0.0, lr_decay_exp=0.1, lr_decay_iters=1000000),
                           dict(params=leaves, names=list(names), lr=0.0, lr_decay_exp=0.1, lr_decay_iters=1000000)])
        return a, path, leaves, adam

    def fused(w, **kw):
        a, path, leaves, adam = w
        return train_step(path, a, cloud.xyz, leaves[0], leaves[1], leaves[2], leaves[3], raydir, cam["campos"], cam["camrot"], cam["bg"], sc.near, sc.far,
                          cam["c2w_nearest"], cam["campos_nearest"], cam["intrinsic"], cam["images"], gt, zero_epsilon=1e-3, w_color=1.0, w_zero_one=1e-4,
                          w2c_nearest=w2c, optimizer=adam, **kw)
    worlds = {}

    def own(k):                                                   # every form has parameters, buffers and optimiser state of its own
        if k not in worlds:
            worlds[k] = world()
        return worlds[k]

    def step_depth():
        fused(own(1), gt_depth=gt_depth, w_depth=W_DEPTH)

    def step_no_depth():
        fused(own(2))

    def autograd_depth():
        a, path, leaves, adam = own(3)
        for q in list(a.parameters()) + leaves:
            q.grad = None
        out = render_train(path, a, cloud.xyz, leaves[0], leaves[1], leaves[2], leaves[3], raydir, cam["campos"], cam["camrot"], cam["bg"], sc.near, sc.far,
                           cam["c2w_nearest"], cam["campos_nearest"], cam["intrinsic"], cam["images"], want_depth=True)
        m = out["ray_mask"] > 0
        lc = torch.nn.functional.mse_loss(out["coarse_raycolor"][m], gt[m])
        val = torch.clamp(out["conf_coefficient"][m], 1e-3, 1 - 1e-3)
        lz = torch.mean(torch.log(val) + torch.log(1 - val))
        md = m & (gt_depth > 0)
        ld = torch.nn.functional.mse_loss(out["coarse_depth"][md], gt_depth[md])
        (lc + 1e-4 * lz + W_DEPTH * ld).backward()
        adam.step()
    fns = dict(step_with_depth=step_depth, step_without_depth=step_no_depth, autograd_form_with_depth=autograd_depth)
    if only:                                                      # one form, a fixed number of calls: the run to put under a kernel trace
        for _ in range(3 + calls):
            fns[only]()
        torch.cuda.synchronize()
        print("RESULT " + json.dumps(dict(step="c3", only=only, calls=3 + calls)), flush=True)
        return
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    res = alternating(fns)
    d, n, a = res["step_with_depth"], res["step_without_depth"], res["autograd_form_with_depth"]
    spread = max(max(v[1]) - min(v[1]) for v in (d, a))
    rec = dict(step="c3", what="C3 training iteration (%d rays, %d points, eager, reuse_outputs, DeviceAdam inside): fused with gt_depth / fused without "
               "(the step before depth supervision) / autograd form with depth (render_train(want_depth=True) + torch loss expressions + backward() + "
               "DeviceAdam.step() on .grad); lr = 0 in all three, so the scene does not move" % (R, n_points),
               added_by_depth_ms=round(d[0] - n[0], 5), autograd_over_fused=round(a[0] / d[0], 3),
               fused_not_slower_than_autograd_within_spread=bool(d[0] <= a[0] + spread))
    _record(rec, res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    ap.add_argument("--out", default=None)
    ap.add_argument("--points", type=float, default=2.0e6)
    ap.add_argument("--steps", default=",".join(s for s, _ in STEPS), help="the steps the parent runs, comma-separated")
    ap.add_argument("--only", default=None, help="with --step c3: run this one form --calls times and stop (for `rocprofv3 --kernel-trace --stats -- python ...`)")
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "depth_sup_timing needs a GPU: there is no CPU fallback and no CPU timing"
        if args.step == "c3":
            step_c3(int(args.points), args.only, args.calls)
        else:
            step_kernels(int(args.points))
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
            f.write("# tools/depth_sup_timing.py on one MI355X: medians of five alternating one-second device-event windows, spread = max - min of the windows\n")
            f.write("\n".join(l[len("RESULT "):] for l in lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
