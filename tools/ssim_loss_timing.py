"""Times the patch SSIM term (csrc/ssim_loss.hip; losses.ssim_patch_loss*, train.train_step(w_ssim=)) at the C5 training shape: 49 dilated patches
of 8 x 8 rays, the pre-defined blur kernels, 2 M points.

  python tools/ssim_loss_timing.py [--out profiles/ssim_loss_timing.txt] [--points 2e6] [--parent-lib PATH]

Steps (each a child process under its own time limit; the parent opens no GPU and stops at the first step that fails):
  kernels   hnr_ssim_loss alone (two launches: value, gradient added in place, total) on 49 patches of 8 x 8, and on one patch of 56 x 56 and of
            64 x 64, each beside the same term in stock torch ops on the same GPU: masking, two grouped conv2d passes per filtered plane (one call
            over the five planes x three channels), the window formula, the mean, autograd back to the colours.
  c5        one eager iteration (56 x 56 rays, blur_kernels, reuse_outputs, DeviceAdam inside at lr = 0 so that every form renders the same scene):
            train_step with w_ssim, without it, and the same iteration as render_train + blur_update_output + the loss terms as torch expressions
            + backward() + DeviceAdam.step() on .grad.  `--step c5 --only FORM --calls N` runs one form N times (the run to put under a kernel trace).
            With --parent-lib (the parent commit's libhnr_hip.so, e.g. built in a `git worktree` of it) the step WITHOUT the term also runs through
            that library, loaded beside this build's in the same process and alternating with it -- the project's standing comparison
            (tools/edit_timing.py).
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

STEPS = (("kernels", 300), ("c5", 480))
W_SSIM, FW = 0.2, 0.7


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


def torch_ssim_term(color, gt, mask, pn, ps, w, fw, win2):
    """fw w (1 - SSIM) in stock torch ops, differentiable w.r.t. color; win2 = (row weight [15,1,1,7], column weight [15,1,7,1])"""
    import torch
    import torch.nn.functional as F
    m = (mask > 0).to(color.dtype)[:, None]

    def patches(t):
        return t.reshape(pn, ps, pn, ps, 3).permute(0, 2, 4, 1, 3).reshape(pn * pn, 3, ps, ps)
    X, Y = patches(color * m), patches(gt * m)
    planes = torch.cat([X, Y, X * X, Y * Y, X * Y], dim=1)
    f = F.conv2d(F.conv2d(planes, win2[0], groups=15), win2[1], groups=15)
    mx, my, exx, eyy, exy = f[:, 0:3], f[:, 3:6], f[:, 6:9], f[:, 9:12], f[:, 12:15]
    sx, sy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
    s = (2 * mx * my + 1e-4) / (mx * mx + my * my + 1e-4) * (2 * sxy + 9e-4) / (sx + sy + 9e-4)
    return (fw * w) * (1 - s.mean())


def _win2(dev):
    from hybridneuralrendering_amd.losses import ssim_window
    g = ssim_window().to(dev)
    return g.reshape(1, 1, 1, 7).repeat(15, 1, 1, 1).contiguous(), g.reshape(1, 1, 7, 1).repeat(15, 1, 1, 1).contiguous()


def step_kernels(_n_points):
    import torch
    from hybridneuralrendering_amd.losses import ssim_patch_loss_grads
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    win2 = _win2(dev)
    fns, rec = {}, dict(step="kernels")
    for tag, pn, ps in (("p49x8", 7, 8), ("p1x56", 1, 56), ("p1x64", 1, 64)):
        S = pn * ps
        field = torch.rand((1, 3, S + 4, S + 4), generator=gen, device=dev)
        gt = torch.nn.functional.avg_pool2d(field, 5, stride=1)[0].permute(1, 2, 0).reshape(-1, 3).contiguous()
        color = (gt + 0.05 * torch.randn(gt.shape, generator=gen, device=dev)).clamp(-0.001, 1.001).contiguous()
        mask = (torch.rand((S * S,), generator=gen, device=dev) >= 0.1).to(torch.int8)
        total, base = torch.zeros((4,), device=dev), torch.zeros_like(color)

        def ours(color=color, gt=gt, mask=mask, pn=pn, ps=ps, total=total, base=base):
            return ssim_patch_loss_grads(color, gt, mask, pn, ps, W_SSIM, frame_weight=FW, total=total, g_color=base)

        def stock(color=color, gt=gt, mask=mask, pn=pn, ps=ps, total=total, base=base):
            x = color.detach().requires_grad_(True)
            term = torch_ssim_term(x, gt, mask, pn, ps, W_SSIM, FW, win2)
            (g,) = torch.autograd.grad(term, x)
            total[0] += term.detach()
            base.add_(g)
            return term, g
        out4, _ = ssim_patch_loss_grads(color, gt, mask, pn, ps, W_SSIM, frame_weight=FW)
        _o, g_ours = ssim_patch_loss_grads(color, gt, mask, pn, ps, W_SSIM, frame_weight=FW)
        term, g_stock = stock()
        torch.cuda.synchronize()
        assert abs(float(out4[2]) - float(term)) <= 1e-5 * abs(float(term)) and float((g_ours - g_stock).abs().max()) <= 1e-4 * float(g_stock.abs().max()), \
            "the term disagrees with its torch form (%s)" % tag
        fns[tag], fns[tag + "_torch"] = ours, stock
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    res = alternating(fns)
    rec["what"] = ("hnr_ssim_loss alone (two launches: value, gradient added in place, total += fw w L) on 49 patches of 8 x 8, one of 56 x 56, one of "
                   "64 x 64, a tenth of the rays missed, each beside the term as grouped conv2d + autograd in stock torch ops on the same GPU")
    for tag in ("p49x8", "p1x56", "p1x64"):
        rec[tag + "_not_slower_than_torch"] = bool(res[tag][0] <= res[tag + "_torch"][0])
        rec[tag + "_torch_over_ours"] = round(res[tag + "_torch"][0] / res[tag][0], 2)
    _record(rec, res)


class _OtherLibrary:
    """Another build of libhnr_hip.so behind this build's ctypes signatures (every entry point it exports)."""

    def __init__(self, mine, path):
        import ctypes
        from hybridneuralrendering_amd import _lib
        self._mine = mine
        other = ctypes.CDLL(path)
        for name, (restype, argtypes) in _lib.SIGNATURES.items():
            if hasattr(other, name):
                fn = getattr(other, name)
                fn.restype, fn.argtypes = restype, argtypes
                setattr(self, name, fn)
        self._other = other

    def __getattr__(self, name):
        return getattr(self._mine, name)


def step_c5(n_points, only=None, calls=20, parent_lib=None):
    import numpy as np
    import torch
    from hnr_bench.common import build_world
    from hybridneuralrendering_amd import scenes
    from hybridneuralrendering_amd.blur import blur_update_output
    from hybridneuralrendering_amd.optim import DeviceAdam
    from hybridneuralrendering_amd.train import TrainPath, train_step, render_train
    dev = torch.device("cuda:0")
    args = SimpleNamespace(scene="scene0241", points=n_points, width=640, height=480, margin=10, knn_order=None)
    sc, opt, agg, cloud, rnd, cam = build_world(args, dev, 0)
    opt.is_train = 1
    pn, ps = 7, 8
    rng = np.random.default_rng(17)
    x0, y0 = int(rng.integers(args.margin, sc.w - args.margin - 56)), int(rng.integers(args.margin, sc.h - args.margin - 56))
    px, py = np.meshgrid(np.arange(x0, x0 + 56), np.arange(y0, y0 + 56), indexing="ij")
    pix = np.stack([px, py], axis=-1).reshape(-1, 2).astype(np.int32)
    raydir = torch.from_numpy(scenes.camera_rays(pix, sc.intrinsic, sc.c2w)).to(dev)
    R = int(raydir.shape[0])
    gt = torch.rand((R, 3), device=dev)
    kern = torch.from_numpy(np.ascontiguousarray(scenes.blur_kernels_v2())).to(dev)[None]
    w2c = torch.inverse(cam["c2w_nearest"]).contiguous()
    names = ("points_embeding", "points_conf", "points_dir", "points_color")
    win2 = _win2(dev)

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
        # lr = 0: the optimiser step runs in full (same launches, same bytes) but the parameters stay, so every form renders the SAME scene
        adam = DeviceAdam([dict(params=[q for _n, q in named], names=[n for n, _q in named], lr=0.0, lr_decay_exp=0.1, lr_decay_iters=1000000),
                           dict(params=leaves, names=list(names), lr=0.0, lr_decay_exp=0.1, lr_decay_iters=1000000)])
        return a, path, leaves, adam

    def fused(w, **kw):
        a, path, leaves, adam = w
        return train_step(path, a, cloud.xyz, leaves[0], leaves[1], leaves[2], leaves[3], raydir, cam["campos"], cam["camrot"], cam["bg"], sc.near, sc.far,
                          cam["c2w_nearest"], cam["campos_nearest"], cam["intrinsic"], cam["images"], gt, zero_epsilon=1e-3, w_color=1.0, w_zero_one=1e-4,
                          frame_weight=FW, w2c_nearest=w2c, optimizer=adam, blur_kernels=kern, patch_num=pn, patch_size=ps, **kw)
    worlds = {}

    def own(k):                                                   # every form has parameters, buffers and optimiser state of its own
        if k not in worlds:
            worlds[k] = world()
        return worlds[k]

    def step_ssim():
        fused(own(1), w_ssim=W_SSIM)

    def step_no_ssim():
        fused(own(2))

    def autograd_ssim():
        a, path, leaves, adam = own(3)
        for q in list(a.parameters()) + leaves:
            q.grad = None
        out = render_train(path, a, cloud.xyz, leaves[0], leaves[1], leaves[2], leaves[3], raydir, cam["campos"], cam["camrot"], cam["bg"], sc.near, sc.far,
                           cam["c2w_nearest"], cam["campos_nearest"], cam["intrinsic"], cam["images"])
        col = blur_update_output(out["coarse_raycolor"][None], gt[None], kern, pn, ps)[0].reshape(-1, 3)
        m = out["ray_mask"] > 0
        lc = torch.nn.functional.mse_loss(col[m], gt[m])
        val = torch.clamp(out["conf_coefficient"][m], 1e-3, 1 - 1e-3)
        lz = torch.mean(torch.log(val) + torch.log(1 - val))
        ls = torch_ssim_term(col, gt, out["ray_mask"], pn, ps, W_SSIM, FW, win2)
        ((lc + 1e-6) * FW + 1e-4 * lz + ls).backward()
        adam.step()
    fns = dict(step_with_ssim=step_ssim, step_without_ssim=step_no_ssim, autograd_form_with_ssim=autograd_ssim)
    if parent_lib:
        from hybridneuralrendering_amd import _lib
        mine = _lib.lib()
        other = _OtherLibrary(mine, parent_lib)

        def step_no_ssim_parent():
            _lib._lib = other
            try:
                fused(own(4))
            finally:
                _lib._lib = mine
        fns["step_without_ssim_parent_lib"] = step_no_ssim_parent
    if only:                                                      # one form, a fixed number of calls: the run to put under a kernel trace
        for _ in range(3 + calls):
            fns[only]()
        torch.cuda.synchronize()
        print("RESULT " + json.dumps(dict(step="c5", only=only, calls=3 + calls)), flush=True)
        return
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    res = alternating(fns)
    rec = dict(step="c5",
               what="C5 training iteration (%d rays = 49 patches of 8 x 8, blur_kernels, %d points, eager, reuse_outputs, DeviceAdam inside, lr = 0): fused "
               "with w_ssim / fused without / autograd form (render_train + blur_update_output + torch loss expressions incl. conv2d SSIM + backward() + "
               "DeviceAdam.step() on .grad)" % (R, n_points))
    d, n, a = res["step_with_ssim"], res["step_without_ssim"], res["autograd_form_with_ssim"]
    spread = max(max(v[1]) - min(v[1]) for v in (d, a))
    rec.update(added_by_ssim_ms=round(d[0] - n[0], 5), autograd_over_fused=round(a[0] / d[0], 3),
               fused_not_slower_than_autograd_within_spread=bool(d[0] <= a[0] + spread))
    if parent_lib:
        q = res["step_without_ssim_parent_lib"]
        spread = max(max(v[1]) - min(v[1]) for v in (n, q))
        rec.update(without_ssim_over_parent_lib=round(n[0] / q[0], 4), without_ssim_within_spread_of_parent_lib=bool(n[0] <= q[0] + spread))
    _record(rec, res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    ap.add_argument("--out", default=None)
    ap.add_argument("--points", type=float, default=2.0e6)
    ap.add_argument("--steps", default=",".join(s for s, _ in STEPS), help="the steps the parent runs, comma-separated")
    ap.add_argument("--only", default=None, help="with --step c5: run this one form --calls times and stop (for `rocprofv3 --kernel-trace --stats -- python ...`)")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="libhnr_hip.so of the parent commit's build: the step without the term also runs through it")
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "ssim_loss_timing needs a GPU: there is no CPU fallback and no CPU timing"
        if args.step == "c5":
            step_c5(int(args.points), args.only, args.calls, args.parent_lib)
        else:
            step_kernels(int(args.points))
        return 0
    lines = []
    for step, limit in STEPS:
        if step not in args.steps.split(","):
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--points", str(args.points)]
        if step == "c5" and args.parent_lib:
            cmd += ["--parent-lib", os.path.abspath(args.parent_lib)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
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
            f.write("# tools/ssim_loss_timing.py on one MI355X: medians of five alternating one-second device-event windows, spread = max - min of the windows\n")
            f.write("\n".join(l[len("RESULT "):] for l in lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
