"""Times the learnable blur module as three launches (blur.LearnableBlur; csrc/blur.hip) and the training iteration that contains it against the
autograd form, on the bench's training scene at the C5 shape (7 x 7 patches of 8 x 8 rays, 9 x 9 kernels, mode 4, boundary 1).

  python tools/blur_learn_timing.py [--out profiles/blur_learn_timing.txt] [--points 2e6]

Steps (each a child process under its own time limit; the parent opens no GPU and stops at the first step that fails):
  module      the blur module alone, forward + backward on fixed inputs: LearnableBlur.forward / .backward (three launches) against
              blur.learnable_blur_update_output + autograd (gradients of the colours and the eight parameters) on the same inputs.
  iteration   one whole training iteration, four forms in the same run, each on its own copy of the weights and point buffers:
              autograd_device_adam   render_train + learnable_blur_update_output + shipped_loss + backward(), then DeviceAdam.step() on .grad
              autograd_torch_adam    the same, then the two default torch.optim.Adam steps of the reference's shell
              fused_eager            train_step(learnable_blur=, optimizer=), reuse_outputs
              fused_captured         CapturedTrainStep(learnable_blur=, optimizer=).step()
  eager_loop  (not run by the parent) 20 fused eager iterations, for a kernel trace of its own.
Medians of five alternating windows of about one second of back-to-back calls, device events."""
import argparse
import copy
import json
import math
import os
import subprocess
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEPS = (("module", 300), ("iteration", 560))
PN, PS, KS = 7, 8, 9


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
        rec[k + "_ms"], rec[k + "_windows_ms"], rec[k + "_calls_per_window"] = round(med, 4), wins, calls
    return rec


def _blur_opt(opt):
    o = copy.copy(opt)
    o.is_train = 1
    o.learnable_blur_kernel, o.learnable_blur_kernel_conv, o.learnable_blur_kernel_size, o.learnable_blur_patch_size = 1, 0, KS, PS
    o.learnable_blur_kernel_mode, o.learnable_blur_kernel_norm, o.boundary_mode = 4, 0, 1
    o.dilation_setup = "%d_%d_1_8" % (PN, PS)
    return o


def step_module(_n_points):
    import torch
    from hybridneuralrendering_amd import scenes
    from hybridneuralrendering_amd.aggregator import PointAggregator
    from hybridneuralrendering_amd.blur import LearnableBlur, learnable_blur_update_output
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    opt = _blur_opt(scenes.scene_opt("scene0241"))
    agg = PointAggregator(opt).to(dev)
    g = torch.Generator().manual_seed(1)
    R = PN * PN * PS * PS
    color, gt, up = (torch.rand((R, 3), generator=g).to(dev) for _ in range(3))
    lb = LearnableBlur(agg, opt, PN, PS)
    predictor = agg.blur_predictor()
    prm = list(predictor.parameters())
    col = color.clone().requires_grad_(True)

    def fused():
        lb.forward(color, gt)
        lb.backward(up)

    def autograd():
        col.grad = None
        for q in prm:
            q.grad = None
        out = learnable_blur_update_output(col[None], gt[None], predictor, opt, PN, PS)
        torch.autograd.backward(out, up[None])
    fns = dict(three_launches=fused, autograd_form=autograd)
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    _g_color, grads = lb.backward(up)
    diff = max(float((grads["learn_blur_kernel_block.%d.%s" % (2 * l, k)] - getattr(predictor[2 * l], k).grad).abs().max()) for l in range(4)
               for k in ("weight", "bias"))
    assert diff < 1e-4, "the two forms disagree: %g" % diff
    res = alternating(fns)
    rec = _record(dict(step="module", what="blur module alone, forward + backward, %d patches of %dx%d, %dx%d kernels, mode 4, boundary 1" % (PN * PN, PS, PS, KS, KS)),
                  res)
    rec.update(autograd_over_three_launches=round(res["autograd_form"][0] / res["three_launches"][0], 3), max_abs_weight_gradient_difference=diff,
               three_launches_not_slower=bool(res["three_launches"][0] <= res["autograd_form"][0]))
    print("RESULT " + json.dumps(rec), flush=True)


def _iteration_world(n_points):
    import numpy as np
    import torch
    from hnr_bench.common import build_world
    from hybridneuralrendering_amd import scenes
    dev = torch.device("cuda:0")
    args = SimpleNamespace(scene="scene0241", points=n_points, width=640, height=480, margin=10, knn_order=None)
    sc, opt, agg, cloud, rnd, cam = build_world(args, dev, 0)
    opt = _blur_opt(opt)
    rng = np.random.default_rng(17)
    S = PN * PS
    x0, y0 = int(rng.integers(args.margin, sc.w - args.margin - S)), int(rng.integers(args.margin, sc.h - args.margin - S))
    px, py = np.meshgrid(np.arange(x0, x0 + S), np.arange(y0, y0 + S), indexing="ij")
    pix = np.stack([px, py], axis=-1).reshape(-1, 2).astype(np.int32)
    raydir = torch.from_numpy(scenes.camera_rays(pix, sc.intrinsic, sc.c2w)).to(dev)
    gt = torch.rand((raydir.shape[0], 3), device=dev)
    w2c = torch.inverse(cam["c2w_nearest"]).contiguous()
    torch.manual_seed(3)
    from hybridneuralrendering_amd.aggregator import PointAggregator
    proto = PointAggregator(opt)
    proto.load_state_dict({k: v.detach().cpu().clone() for k, v in agg.state_dict().items()}, strict=False)      # (the predictor keeps its seeded initialisation)
    state = {k: v.detach().clone() for k, v in proto.state_dict().items()}

    def world():
        """its own copies: leaves, an aggregator sharing nothing with the other forms, a path with reused buffers"""
        from hybridneuralrendering_amd.render import HybridRenderer
        from hybridneuralrendering_amd.train import TrainPath
        a = PointAggregator(opt)
        a.load_state_dict(state)
        a = a.to(dev)
        path = TrainPath(HybridRenderer(opt, a, dev))
        path.reuse_outputs = True
        leaves = [t.clone().requires_grad_(True) for t in (cloud.emb, cloud.conf, cloud.dir, cloud.color)]
        return a, path, leaves
    return SimpleNamespace(dev=dev, sc=sc, opt=opt, cloud=cloud, cam=cam, raydir=raydir, gt=gt, w2c=w2c, world=world)


def _device_adam(a, leaves):
    from hybridneuralrendering_amd.optim import DeviceAdam
    named = list(a.named_parameters())
    names = ("points_embeding", "points_conf", "points_dir", "points_color")
    return DeviceAdam([dict(params=[q for _n, q in named], names=[n for n, _q in named], lr=5e-4, lr_decay_exp=0.1, lr_decay_iters=1000000),
                       dict(params=leaves, names=list(names), lr=2e-3, lr_decay_exp=0.1, lr_decay_iters=1000000)])


def _forms(w):
    import torch
    from hybridneuralrendering_amd.blur import LearnableBlur, learnable_blur_update_output
    from hybridneuralrendering_amd.losses import shipped_loss
    from hybridneuralrendering_amd.train import CapturedTrainStep, render_train, train_step
    cam, sc, cloud = w.cam, w.sc, w.cloud
    rargs = (w.raydir, cam["campos"], cam["camrot"], cam["bg"], sc.near, sc.far, cam["c2w_nearest"], cam["campos_nearest"], cam["intrinsic"], cam["images"])

    def autograd_iteration(a, path, leaves):
        for t in leaves:
            t.grad = None
        a.zero_grad(set_to_none=True)
        o = render_train(path, a, cloud.xyz, leaves[0], leaves[1], leaves[2], leaves[3], *rargs)
        col = learnable_blur_update_output(o["coarse_raycolor"][None], w.gt[None], a.blur_predictor(), w.opt, PN, PS)[0]
        loss, _parts = shipped_loss(col, o["conf_coefficient"], w.gt, o["ray_mask"], 1e-3, 1.0, 1e-4, conf_rows=True)
        loss.backward()
    a1, p1, l1 = w.world()
    o1 = _device_adam(a1, l1)
    a2, p2, l2 = w.world()
    t_net, t_pts = torch.optim.Adam(list(a2.parameters()), lr=5e-4, betas=(0.9, 0.999)), torch.optim.Adam(l2, lr=2e-3, betas=(0.9, 0.999))
    a3, p3, l3 = w.world()
    o3, lb3 = _device_adam(a3, l3), LearnableBlur(a3, w.opt, PN, PS)
    a4, p4, l4 = w.world()
    o4, lb4 = _device_adam(a4, l4), LearnableBlur(a4, w.opt, PN, PS)
    sample = dict(raydir=w.raydir, campos=cam["campos"], camrot=cam["camrot"], bg_color=cam["bg"], c2w_nearest=cam["c2w_nearest"], w2c_nearest=w.w2c,
                  campos_nearest=cam["campos_nearest"], intrinsic_nearest=cam["intrinsic"], images_nearest=cam["images"], gt_image=w.gt)
    cap = CapturedTrainStep(p4, a4, cloud.xyz, l4[0], l4[1], l4[2], l4[3], sample, sc.near, sc.far, zero_epsilon=1e-3, w_color=1.0, w_zero_one=1e-4,
                            optimizer=o4, learnable_blur=lb4)

    def autograd_device_adam():
        autograd_iteration(a1, p1, l1)
        o1.step()

    def autograd_torch_adam():
        autograd_iteration(a2, p2, l2)
        t_net.step(); t_pts.step()

    def fused_eager():
        train_step(p3, a3, cloud.xyz, l3[0], l3[1], l3[2], l3[3], *rargs, w.gt, zero_epsilon=1e-3, w_color=1.0, w_zero_one=1e-4, w2c_nearest=w.w2c,
                   learnable_blur=lb3, optimizer=o3)

    def fused_captured():
        cap.step()
    return dict(autograd_device_adam=autograd_device_adam, autograd_torch_adam=autograd_torch_adam, fused_eager=fused_eager, fused_captured=fused_captured)


def step_iteration(n_points):
    import torch
    fns = _forms(_iteration_world(n_points))
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    res = alternating(fns)
    rec = _record(dict(step="iteration", what="one training iteration at the C5 shape (3136 rays, %d points, optimiser included), four forms" % n_points), res)
    old = min(res["autograd_device_adam"][0], res["autograd_torch_adam"][0])
    rec.update(fastest_autograd_over_fused_eager=round(old / res["fused_eager"][0], 3), fastest_autograd_over_fused_captured=round(old / res["fused_captured"][0], 3),
               fused_not_slower=bool(max(res["fused_eager"][0], res["fused_captured"][0]) <= old))
    print("RESULT " + json.dumps(rec), flush=True)


def step_eager_loop(n_points):
    import torch
    fn = _forms(_iteration_world(n_points))["fused_eager"]
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    print("RESULT " + json.dumps(dict(step="eager_loop", iterations=20)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS] + ["eager_loop"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--points", type=float, default=2.0e6)
    ap.add_argument("--steps", default=",".join(s for s, _ in STEPS), help="the steps the parent runs, comma-separated")
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "blur_learn_timing needs a GPU: there is no CPU fallback and no CPU timing"
        dict(module=step_module, iteration=step_iteration, eager_loop=step_eager_loop)[args.step](int(args.points))
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
            f.write("# tools/blur_learn_timing.py on one MI355X: medians of five alternating one-second device-event windows\n")
            f.write("\n".join(l[len("RESULT "):] for l in lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
