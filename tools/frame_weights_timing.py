"""Times the content-aware frame weights on the device (hybridneuralrendering_amd/flow.py, frame_weights.py; csrc/raft.hip, csrc/blur_score.hip)
against the same stages written with stock torch ops on the same GPU -- what the reference runs: `conv2d`, `instance_norm`, `batch_norm`, `matmul`,
`avg_pool2d`, `grid_sample`, `unfold` / `softmax` (tests/raft_ref.py, the restatement the tests use, in fp32 on the device) and, for the scoring, a
reflect-padded `conv2d` in fp64, `grid_sample(mode='nearest')` and `var`.

  python tools/frame_weights_timing.py [--out profiles/frame_weights_timing.txt]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/frame_weights_timing.py --step trace        (three pairs of the HIP chain, for the per-kernel times)

The parent opens no GPU: it runs every step as a child process of its own under its own time limit and stops at the first step that fails.  Each
child warms both sides up, then times five alternating windows per side, each about one second of back-to-back calls, with device events
(tools/cloud_init_timing.py::windows) and reports the median of the windows and their spread.  `scene` is one call per side of a 200-frame scene
(wall clock, the host reads included: one per scene on the HIP side, two per pair on the torch side, as the reference's script makes them).

Workload: one pair of 480x640, iters = 20 (a 60x80 feature map, a 4800 x 4800 correlation volume); weights from the tests' seeded rule (the arithmetic
does not depend on them)."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cloud_init_timing import report, windows          # noqa: E402

STEPS = (("encoders", 300), ("pyramid", 300), ("updates", 420), ("upsample", 300), ("scoring", 300), ("pair", 420), ("scene", 560))
H, W, ITERS, SCENE_FRAMES, BORDER = 480, 640, 20, 200, 20
UPDATE_GMAC_PER_PIXEL = (324 * 256 + 9 * 256 * 192 + 49 * 2 * 128 + 9 * 128 * 64 + 9 * 256 * 126 + 2 * 5 * 384 * 384 + 9 * 128 * 256 + 9 * 256 * 2) / 1e9


def setup(dev):
    import numpy as np
    import torch
    from hybridneuralrendering_amd.flow import RAFT
    from tests import raft_ref as R
    sd = R.make_params()
    net = RAFT().load_pretrained(dict(sd)).to(dev)
    rs = np.random.RandomState(0)
    base = rs.randint(0, 256, (H // 4 + 8, W // 4 + 8, 3)).astype(np.uint8)
    big = np.kron(base, np.ones((4, 4, 1), dtype=np.uint8))                # 4x4 blocks: structure at the scale the encoders see
    frames = np.stack([big[8 + 2 * k:8 + 2 * k + H, 12 - 3 * k:12 - 3 * k + W] for k in range(4)])
    frames = np.clip(frames.astype(np.int64) + rs.randint(-2, 3, frames.shape), 0, 255).astype(np.uint8)
    return net, {k: v.to(dev) for k, v in sd.items()}, torch.from_numpy(frames).to(dev), R


def stock_scoring(gray_pair, flow_up, border):
    """The script's scoring of one pair in stock torch ops on the device: (score_cur, score_ref) as 0-d tensors."""
    import torch
    import torch.nn.functional as F
    g = gray_pair.double()[:, None]
    box = F.conv2d(F.pad(g, (2, 2, 2, 2), mode="reflect"), torch.full((1, 1, 5, 5), 1.0 / 25.0, dtype=torch.float64, device=g.device))
    lap = torch.tensor([[0., 1., 0.], [1., -4., 1.], [0., 1., 0.]], dtype=torch.float64, device=g.device)[None, None]
    edge = F.conv2d(F.pad(box, (1, 1, 1, 1), mode="reflect"), lap)
    hh, ww = g.shape[-2:]
    ys, xs = torch.meshgrid(torch.arange(hh, device=g.device), torch.arange(ww, device=g.device), indexing="ij")
    v = torch.stack([xs, ys]).float()[None] + flow_up[None]
    grid = torch.stack([2.0 * v[:, 0] / max(ww - 1, 1) - 1.0, 2.0 * v[:, 1] / max(hh - 1, 1) - 1.0], dim=-1)
    mask = torch.zeros((1, 1, hh, ww), device=g.device)
    mask[..., border:hh - border, border:ww - border] = 1
    e2w = F.grid_sample(edge[1:2].float(), grid, mode="nearest", align_corners=False)
    m2w = F.grid_sample(mask, grid, mode="nearest", align_corners=False)
    used = (m2w * mask)[0, 0] == 1
    return edge[0, 0][used].var(unbiased=False), e2w[0, 0][used].double().var(unbiased=False)


def run_step(step):
    import torch
    from hybridneuralrendering_amd import _lib, flow, frame_weights as FW
    dev = torch.device("cuda:0")
    net, sd, frames, R = setup(dev)
    L = _lib.lib()
    fpk, cpk, upk = net.packed()
    h, w = H // 8, W // 8
    pair = frames[:2].permute(0, 3, 1, 2).float().contiguous()
    gray = FW.gray_from_rgb(frames)
    state, extra = {}, {}
    rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max())
    with torch.no_grad():
        # every step's inputs come from the HIP path's earlier stages
        fmaps = flow.encoder(pair, fpk, 0)
        cn = flow.encoder(pair[:1], cpk, 2)[0]
        pyr = flow.corr_pyramid(fmaps[0], fmaps[1])
        levels = flow.pyramid_levels(pyr, h, w)
        grid0 = R.grid(h, w, torch.float32).to(dev)
        scratch = torch.empty((int(L.hnr_raft_update_scratch_elems(h, w)),), dtype=torch.float32, device=dev)
        mask_buf = torch.empty((576, h, w), dtype=torch.float32, device=dev)

        def hip_updates():
            n, c = cn[:128].clone(), grid0.clone()
            for it in range(ITERS):
                _lib.check(L.hnr_raft_update(_lib.ptr(upk), _lib.ptr(pyr), _lib.ptr(n), _lib.ptr(cn[128:]), _lib.ptr(c), h, w, None,
                                             _lib.ptr(mask_buf) if it == ITERS - 1 else None, _lib.ptr(scratch), scratch.numel(), _lib.stream()), "hnr_raft_update")
            return c - grid0, mask_buf

        def stock_encoders(p):
            x = 2 * (p / 255.0) - 1.0
            c = R.encoder(sd, "cnet", x[:1], True)
            return R.encoder(sd, "fnet", x, False), torch.cat([torch.tanh(c[:, :128]), torch.relu(c[:, 128:])], dim=1)[0]

        def stock_updates(lv, c0):
            n, inp, c = c0[None, :128], c0[None, 128:], grid0
            for _ in range(ITERS):
                n, m, d = R.update(sd, n, inp, R.lookup(lv, c)[None], (c - grid0)[None])
                c = c + d[0]
            return c - grid0, m[0]

        def stock_flow(p):
            fm, c0 = stock_encoders(p)
            low, m = stock_updates(R.corr_pyramid(fm[0], fm[1]), c0)
            return low, R.upsample(low[None], m[None])[0]

        low, mask = hip_updates()
        low, mask = low.clone(), mask.clone()
        up = flow.upsample(low, mask)
        if step == "encoders":
            ours, theirs, what = lambda: (flow.encoder(pair, fpk, 0), flow.encoder(pair[:1], cpk, 2)[0]), lambda: stock_encoders(pair), "fnet on both images, cnet on the first, %dx%d" % (H, W)
        elif step == "pyramid":
            ours, theirs = lambda: tuple(flow.pyramid_levels(flow.corr_pyramid(fmaps[0], fmaps[1]), h, w)), lambda: tuple(R.corr_pyramid(fmaps[0], fmaps[1]))
            what = "all-pairs correlation %d x %d and three poolings" % (h * w, h * w)
        elif step == "updates":
            ours, theirs, what = hip_updates, lambda: stock_updates(levels, cn), "%d iterations of lookup + update block at %dx%d" % (ITERS, h, w)
        elif step == "upsample":
            ours, theirs, what = lambda: flow.upsample(low, mask), lambda: R.upsample(low[None], mask[None])[0], "convex upsampling %dx%d -> %dx%d" % (h, w, H, W)
        elif step == "scoring":
            def ours():
                e = FW.blur_edges(gray[:2])
                return FW.blur_score_pair(e[0], e[1], up, BORDER)[:2]
            theirs, what = lambda: torch.stack(stock_scoring(gray[:2], up, BORDER)), "edge maps of two frames + warp + variances, %dx%d" % (H, W)
        elif step == "pair":
            def ours():
                e = FW.blur_edges(gray[:2])
                return FW.blur_score_pair(e[0], e[1], net.flow_pair(pair, ITERS)[1], BORDER)[:2]
            theirs, what = lambda: torch.stack(stock_scoring(gray[:2], stock_flow(pair)[1], BORDER)), "one pair %dx%d, iters %d: flow + scoring" % (H, W, ITERS)
        else:
            idx = torch.arange(SCENE_FRAMES, device=dev) % 4
            imgs, grays = frames[idx], gray[idx]

            def ours():
                return FW.content_aware_weights(imgs, grays, net, border=BORDER, iters=ITERS)

            def theirs():
                cur, ref = [], []
                for f in range(SCENE_FRAMES):
                    g = min(f + 1, SCENE_FRAMES - 1)
                    p = imgs[[f, g]].permute(0, 3, 1, 2).float().contiguous()
                    a, b = stock_scoring(grays[[f, g]], stock_flow(p)[1], BORDER)
                    cur.append(a.item()); ref.append(b.item())
                return FW.weights_from_scores(cur, ref)
            FW.content_aware_weights(imgs[:3], grays[:3], net, border=BORDER, iters=ITERS)
            stock_scoring(grays[:2], stock_flow(pair)[1], BORDER)
            torch.cuda.synchronize()
            t0 = time.perf_counter(); wa = ours(); torch.cuda.synchronize(); ta = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter(); wb = theirs(); torch.cuda.synchronize(); tb = (time.perf_counter() - t0) * 1e3
            extra["max_rel_difference"] = float(abs(wa - wb).max() / abs(wb).max())
            report(step, "a scene of %d frames %dx%d, iters %d: images -> weights (one call per side, wall clock)" % (SCENE_FRAMES, H, W, ITERS), ta, tb, [ta], [tb], 1, 1, extra)
            return

        def run_ours():
            state["ours"] = ours()

        def run_theirs():
            state["theirs"] = theirs()
        run_ours(); run_theirs(); torch.cuda.synchronize()
        a, b = state["ours"], state["theirs"]
        a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
        extra["max_rel_difference"] = max(rel(x, y) for x, y in zip(a, b))
        ma, mb, ta, tb, ca, cb = windows(run_ours, run_theirs, 5)
    if step == "updates":
        gmac = UPDATE_GMAC_PER_PIXEL * h * w * ITERS
        extra.update(gmac=round(gmac, 1), hip_tflops=round(2 * gmac / ma, 2), torch_tflops=round(2 * gmac / mb, 2))
    report(step, what, ma, mb, ta, tb, ca, cb, extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS] + ["trace"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", default=",".join(s for s, _ in STEPS), help="the steps the parent runs, comma-separated")
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "frame_weights_timing needs a GPU: there is no CPU fallback and no CPU timing"
        if args.step == "trace":
            from hybridneuralrendering_amd import frame_weights as FW
            dev = torch.device("cuda:0")
            net, _, frames, _ = setup(dev)
            FW.content_aware_weights(frames[:3], FW.gray_from_rgb(frames[:3]), net, border=BORDER, iters=ITERS)
            torch.cuda.synchronize()
            return 0
        run_step(args.step)
        return 0
    lines = []
    for step, limit in STEPS:
        if step not in args.steps.split(","):
            continue
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print("step %s passed its time limit of %d s: stopping" % (step, limit))
            return 1
        got = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            print("step %s failed (exit %d): stopping\n%s" % (step, r.returncode, r.stderr[-2000:]))
            return 1
        lines += got
        print(got[0], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/frame_weights_timing.py: medians of alternating device-event windows, HIP path vs the same stage in stock torch ops\n")
            f.write("\n".join(l[len("RESULT "):] for l in lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
