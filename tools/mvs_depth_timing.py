"""Times the depth estimator on the device (hybridneuralrendering_amd/mvs_depth.py, csrc/mvsnet.hip) against the same stages written with stock torch
ops on the same GPU -- what the reference runs, with the batch norms folded once as the HIP path folds them: `conv2d` / `conv3d` / `conv_transpose3d` +
the folded affine + `relu`, `grid_sample` for the warps, `softmax` for the head.

  python tools/mvs_depth_timing.py [--out profiles/mvs_depth_timing.txt]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/mvs_depth_timing.py --step trace        (ten calls of the HIP chain, for the per-kernel times)

The parent opens no GPU: it runs every step (`feature`, `volume`, `costreg`, `head`, `points`, `whole`) as a child process of its own under its own time
limit and stops at the first step that fails.  Each child warms both sides up, then times five alternating windows per side, each about one second of
back-to-back calls, with device events (tools/cloud_init_timing.py::windows) and reports the median of the windows and their spread.  Inputs are on the
device on both sides; weights are random (the arithmetic does not depend on them).

Shape: the reference's, V = 3 views of 480x640, D = 192 depth planes, so a 120x160 depth map and a 32 x 192 x 120 x 160 cost volume; one reference view.
`costreg` also reports the share of the 78.6 TFLOP/s at which unpacked fp32 FMAs issue, from the network's multiply-add count at this shape."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cloud_init_timing import report, windows          # noqa: E402

STEPS = (("feature", 300), ("volume", 300), ("costreg", 420), ("head", 300), ("points", 300), ("whole", 420))          # (name, time limit in seconds)
V, D, H, W = 3, 192, 480, 640
PEAK_UNPACKED_FP32 = 78.6e12


def cost_reg_macs(D, h, w):
    """Multiply-adds of CostRegNet: a convolution counts 27 taps per output and input channel, a transposed one its 27 / 8 valid taps on average."""
    from hybridneuralrendering_amd.mvs_depth import REG_CONVS, REG_DECONVS
    n, total, level = D * h * w, 0, 1
    for cin, cout, stride in REG_CONVS:
        level *= stride ** 3
        total += 27 * cin * cout * n // level
    for _, cin, cout in REG_DECONVS:
        total += 27 * cin * cout * n // level                         # (27 taps per INPUT voxel)
        level //= 8
    return total + 27 * 8 * n


def random_net(dev):
    import torch
    from hybridneuralrendering_amd.mvs_depth import MVSNet
    torch.manual_seed(0)
    net = MVSNet()
    with torch.no_grad():
        for name, b in net.named_buffers():
            b.copy_(torch.rand(b.shape) * 0.4 - 0.2 if name.endswith("running_mean") else 0.5 + torch.rand(b.shape))
        for name, p in net.named_parameters():
            if p.dim() == 1:
                p.copy_(0.5 + torch.rand(p.shape) if name.endswith("weight") else torch.rand(p.shape) * 0.4 - 0.2)
    return net.to(dev)


def inputs(dev):
    import numpy as np
    import torch
    g = torch.Generator().manual_seed(1)
    imgs = torch.rand((V, 3, H, W), generator=g).to(dev)
    h, w = H // 4, W // 4
    K = np.array([[1.1 * w, 0, 0.5 * w, 0], [0, 1.1 * w, 0.5 * h, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    proj = [np.eye(4)]
    for v in range(1, V):
        E = np.eye(4)
        E[:3, 3] = [0.25 * (-1) ** v, 0.2, 0.05]
        proj.append(K @ E @ np.linalg.inv(K))
    proj = torch.from_numpy(np.stack(proj)[:, :3].astype(np.float32)).to(dev)
    dv = (2.0 + torch.arange(D, dtype=torch.float32) * (2.0 / D)).to(dev)
    Kimg = np.array([[577.59, 0, 318.9], [0, 578.73, 242.68], [0, 0, 1]], np.float32)
    return imgs, proj, dv, Kimg


def stock(net):
    """The five stages from stock torch ops; every norm folded to (mean, mul, bias) once."""
    import torch
    import torch.nn.functional as F
    from hybridneuralrendering_amd.mvs_depth import EPS, FEATURE_LAYERS, REG_CONVS, REG_DECONVS
    fold = lambda bn, nd: tuple(t.detach().view((1, -1) + (1,) * nd) for t in (bn.running_mean, bn.weight * torch.rsqrt(bn.running_var + EPS), bn.bias))
    fn, cr = net.feature, net.cost_regularization
    f2 = [(getattr(fn, "conv%d" % i).conv.weight.detach(), s, k // 2) + fold(getattr(fn, "conv%d" % i).bn, 2) for i, (_, _, k, s) in enumerate(FEATURE_LAYERS)]
    c3 = [(getattr(cr, "conv%d" % i).conv.weight.detach(), s) + fold(getattr(cr, "conv%d" % i).bn, 3) for i, (_, _, s) in enumerate(REG_CONVS)]
    t3 = [(getattr(cr, n)[0].weight.detach(),) + fold(getattr(cr, n)[1], 3) for n, _, _ in REG_DECONVS]

    def feature(imgs):
        x = imgs
        for w, s, p, mean, mul, bias in f2:
            x = F.relu((F.conv2d(x, w, None, stride=s, padding=p) - mean) * mul + bias)
        return F.conv2d(x, fn.feature.weight.detach(), fn.feature.bias.detach(), padding=1)

    def volume(feats, proj, dv):
        nv, _, h, w = feats.shape
        y, x = torch.meshgrid(torch.arange(0, h, dtype=torch.float32, device=feats.device), torch.arange(0, w, dtype=torch.float32, device=feats.device), indexing="ij")
        xyz = torch.stack((x.reshape(-1), y.reshape(-1), torch.ones(h * w, device=feats.device)))
        s = q = 0
        for v in range(nv):                                           # homo_warping
            p = (proj[v, :, :3] @ xyz).unsqueeze(1) * dv.view(1, -1, 1) + proj[v, :, 3].view(3, 1, 1)
            xy = p[:2] / p[2:3]
            grid = torch.stack((xy[0] / ((w - 1) / 2) - 1, xy[1] / ((h - 1) / 2) - 1), dim=2)
            wv = F.grid_sample(feats[v:v + 1], grid.view(1, -1, w, 2), mode="bilinear", padding_mode="zeros", align_corners=False).view(32, -1, h, w)
            s, q = s + wv, q + wv.pow(2)
        return q.div_(nv).sub_(s.div_(nv).pow_(2))

    def costreg(vol):
        x, c = vol[None], []
        for w, s, mean, mul, bias in c3:
            x = F.relu((F.conv3d(x, w, None, stride=s, padding=1) - mean) * mul + bias)
            c.append(x)
        for (w, mean, mul, bias), skip in zip(t3, (c[4], c[2], c[0])):
            x = skip + F.relu((F.conv_transpose3d(x, w, None, stride=2, padding=1, output_padding=1) - mean) * mul + bias)
        return F.conv3d(x, cr.prob.weight.detach(), cr.prob.bias.detach(), padding=1)[0, 0]

    def head(logits, dv):
        p = F.softmax(logits, dim=0)
        depth = torch.sum(p * dv.view(-1, 1, 1), 0)
        sum4 = 4 * F.avg_pool3d(F.pad(p[None, None], pad=(0, 0, 0, 0, 1, 2)), (4, 1, 1), stride=1, padding=0)[0, 0]
        idx = torch.sum(p * torch.arange(p.shape[0], device=p.device, dtype=torch.float32).view(-1, 1, 1), 0).long()
        return depth, torch.gather(sum4, 0, idx[None])[0]

    def points(depth, conf, near, far, kt_inv):
        d = F.interpolate(depth[None, None], size=[H, W], mode="nearest")[0, 0]
        c = F.interpolate(conf[None, None], size=[H, W], mode="nearest")[0, 0]
        mask = torch.logical_and(d >= near, d <= far)
        z = torch.clamp((d - near) / (far - near), min=0.0, max=1.0)
        vy, vx = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=d.device) / (H - 1), torch.arange(W, dtype=torch.float32, device=d.device) / (W - 1),
                                indexing="ij")
        cam_z = z * (far - near) + near
        cam = torch.stack([vx * (W - 1) * cam_z, vy * (H - 1) * cam_z, cam_z], dim=-1) @ kt_inv
        return cam, c, mask
    return dict(feature=feature, volume=volume, costreg=costreg, head=head, points=points)


def run_step(step):
    import torch
    from hybridneuralrendering_amd import mvs_depth as md
    dev = torch.device("cuda:0")
    net = random_net(dev)
    imgs, proj, dv, Kimg = inputs(dev)
    st = stock(net)
    fpk, rpk = net.packed()
    kt_inv = torch.from_numpy(md.kt_inverse(Kimg)).to(dev)
    near, far = 2.5, 3.5
    state, extra = {}, {}
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    with torch.no_grad():
        # every step's inputs come from the HIP path's earlier stages
        feats = md.feature_forward(imgs, fpk)
        vol = md.cost_volume(feats, proj, dv) if step in ("volume", "costreg", "head", "points") else None
        logits = md.cost_reg(vol, rpk) if step in ("costreg", "head", "points") else None
        if step in ("head", "points"):
            vol = None
            depth, conf, _ = md.depth_head(logits, dv)
        if step == "feature":
            ours, theirs, what = lambda: md.feature_forward(imgs, fpk), lambda: st["feature"](imgs), "feature net of %d views %dx%d" % (V, H, W)
        elif step == "volume":
            ours, theirs, what = lambda: md.cost_volume(feats, proj, dv), lambda: st["volume"](feats, proj, dv), "variance cost volume 32x%dx%dx%d from %d views" % (D, H // 4, W // 4, V)
        elif step == "costreg":
            ours, theirs, what = lambda: md.cost_reg(vol, rpk), lambda: st["costreg"](vol), "cost regularisation of 32x%dx%dx%d" % (D, H // 4, W // 4)
        elif step == "head":
            ours, theirs, what = lambda: md.depth_head(logits, dv)[:2], lambda: st["head"](logits, dv), "depth head over %dx%dx%d logits" % (D, H // 4, W // 4)
        elif step == "points":
            ours = lambda: md.depth_points(depth, conf, H, W, near, far, Kimg)
            theirs, what = lambda: st["points"](depth, conf, near, far, kt_inv), "points of a %dx%d depth map at %dx%d" % (H // 4, W // 4, H, W)
        else:
            def ours():
                d, c, _, _ = net(imgs[None], proj[None], dv[None])
                return md.depth_points(d[0], c[0], H, W, near, far, Kimg)

            def theirs():
                d, c = st["head"](st["costreg"](st["volume"](st["feature"](imgs), proj, dv)), dv)
                return st["points"](d, c, near, far, kt_inv)
            what = "images -> points, one reference view, V = %d, D = %d, %dx%d" % (V, D, H, W)

        def run_ours():
            state["ours"] = ours()

        def run_theirs():
            state["theirs"] = theirs()
        run_ours(); run_theirs(); torch.cuda.synchronize()
        a, b = state["ours"], state["theirs"]
        a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
        extra["max_rel_difference"] = max(rel(x.float(), y.float()) for x, y in zip(a, b))
        ma, mb, ta, tb, ca, cb = windows(run_ours, run_theirs, 5)
    if step == "costreg":
        macs = cost_reg_macs(D, H // 4, W // 4)
        extra.update(gmac=round(macs / 1e9, 2), hip_tflops=round(2 * macs / (ma * 1e-3) / 1e12, 2),
                     hip_share_of_unpacked_fp32_issue=round(2 * macs / (ma * 1e-3) / PEAK_UNPACKED_FP32, 4))
    report(step, what, ma, mb, ta, tb, ca, cb, extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS] + ["trace"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "mvs_depth_timing needs a GPU: there is no CPU fallback and no CPU timing"
        if args.step == "trace":
            from hybridneuralrendering_amd import mvs_depth as md
            dev = torch.device("cuda:0")
            net = random_net(dev)
            imgs, proj, dv, Kimg = inputs(dev)
            for _ in range(10):
                d, c, _, _ = net(imgs[None], proj[None], dv[None])
                md.depth_points(d[0], c[0], H, W, 2.5, 3.5, Kimg)
            torch.cuda.synchronize()
            return 0
        run_step(args.step)
        return 0
    lines = []
    for step, limit in STEPS:
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
            f.write("# tools/mvs_depth_timing.py: medians of alternating device-event windows, HIP path vs the same stage in stock torch ops\n")
            f.write("\n".join(l[len("RESULT "):] for l in lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
