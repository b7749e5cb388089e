"""Times the init checkpoint's networks on the device (hybridneuralrendering_amd/mvs_init.py, csrc/featnet.hip) against the same stages written with
stock torch ops on the same GPU -- what a user with a ROCm torch but without InPlaceABN could write by hand: per layer `conv2d` + the folded
affine + `leaky_relu` for the pyramid, `grid_sample` per level + an `nn.Sequential` for the embedding.

  python tools/featnet_timing.py [--out profiles/featnet_timing.txt]

The parent opens no GPU: it runs every step (`pyramid1`, `pyramid8`, `embed`) as a child process of its own under its own time limit and stops at the
first step that fails.  Each child warms both sides up, then times five alternating windows per side, each about one second of back-to-back calls,
with device events (tools/cloud_init_timing.py::windows) and reports the median of the windows and their spread.  Inputs are on the device on both
sides; weights are random (the arithmetic does not depend on them).

Sizes: the pyramid of one 480x640 view and of a batch of eight; hnr_point_embed for 200 k points of one 480x640 view."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cloud_init_timing import report, windows          # noqa: E402

STEPS = (("pyramid1", 180), ("pyramid8", 180), ("embed", 180))          # (name, time limit in seconds)


def random_net(dev):
    import torch
    from hybridneuralrendering_amd.mvs_init import MvsInit
    torch.manual_seed(0)
    net = MvsInit()
    with torch.no_grad():
        for name, b in net.named_buffers():
            b.copy_(torch.randn(b.shape) * 0.3 if name.endswith("running_mean") else 0.5 + torch.rand(b.shape))
        for name, p in net.named_parameters():
            if name.endswith("bn.weight"):
                p.copy_(0.5 + torch.rand(p.shape))
    return net.to(dev)


def stock_pyramid(net):
    """The same network from stock torch ops, the multiplier folded once as the HIP path folds it."""
    import torch
    import torch.nn.functional as F
    from hybridneuralrendering_amd.mvs_init import EPS, LAYERS
    layers = []
    for name, specs in LAYERS:
        for blk, (_, _, ks, stride) in zip(getattr(net.FeatureNet, name), specs):
            mul = torch.rsqrt(blk.bn.running_var + EPS) * (blk.bn.weight.detach().abs() + EPS)
            layers.append((blk.conv.weight.detach(), stride, ks // 2, blk.bn.running_mean.view(1, -1, 1, 1), mul.view(1, -1, 1, 1),
                           blk.bn.bias.detach().view(1, -1, 1, 1)))
    tw, tb = net.FeatureNet.toplayer.weight.detach(), net.FeatureNet.toplayer.bias.detach()

    def run(x):
        outs = []
        for i, (w, stride, pad, mean, mul, bias) in enumerate(layers):
            x = F.leaky_relu((F.conv2d(x, w, None, stride=stride, padding=pad) - mean) * mul + bias, 0.01)
            if i in (1, 4, 7):
                outs.append(x)
        outs[2] = F.conv2d(outs[2], tw, tb)
        return outs
    return run


def step_pyramid(V):
    import torch
    dev = torch.device("cuda:0")
    net = random_net(dev)
    img = torch.rand((V, 3, 480, 640), generator=torch.Generator().manual_seed(1)).to(dev)
    stock_run = stock_pyramid(net)
    state = {}

    def ours():
        state["ours"] = net.get_image_features(img[None])[1:]

    def stock():
        with torch.no_grad():
            state["stock"] = stock_run(img)
    ours(); stock(); torch.cuda.synchronize()
    worst = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(state["ours"], state["stock"]))
    ma, mb, ta, tb, ca, cb = windows(ours, stock, 5)
    report("pyramid%d" % V, "FeatureNet pyramid of %d view(s) 480x640" % V, ma, mb, ta, tb, ca, cb, dict(max_rel_difference=worst))


def step_embed():
    import numpy as np
    import torch
    import torch.nn.functional as F
    from hybridneuralrendering_amd import cloud_init as ci
    dev = torch.device("cuda:0")
    net = random_net(dev)
    g = torch.Generator().manual_seed(0)
    n, H, W = 200000, 480, 640
    image = torch.rand((3, H, W), generator=g).to(dev)
    K = np.array([[577.59, 0, 318.9], [0, 578.73, 242.68], [0, 0, 1]], np.float32)
    c2w = np.eye(4, dtype=np.float32)
    c2w[:3, 3] = [0.3, -0.2, 0.1]
    w2c = torch.inverse(torch.from_numpy(c2w)).numpy()
    cam = torch.stack([torch.rand(n, generator=g) * 1.4 - 0.7, torch.rand(n, generator=g) * 1.1 - 0.55, torch.ones(n)], -1) * (torch.rand((n, 1), generator=g) * 3 + 0.5)
    xyz = (cam + torch.tensor([0.3, -0.2, 0.1])).to(dev)
    Kd, c2wd, w2cd = torch.from_numpy(K).to(dev), torch.from_numpy(c2w).to(dev), torch.from_numpy(w2c).to(dev)
    feats = net.get_image_features(image[None, None])
    maps = [feats[1][0], feats[2][0], feats[3][0]]
    premlp = net.premlp
    state = {}

    def ours():
        state["ours"] = net.embed_points(xyz, image, c2w, w2c, K, feats=feats)

    def sample(src, grid, mask):                                      # extract_from_2d_grid
        w = F.grid_sample(src[None], grid[:, None, ...], mode="bilinear", padding_mode="zeros", align_corners=True)
        w = w.permute(0, 2, 3, 1).view(1, -1, src.shape[0])
        full = torch.zeros([1, mask.shape[1], src.shape[0]], device=dev)
        full[0, mask[0, :, 0], :] = w
        return full

    def stock():
        with torch.no_grad():
            cam_xyz = (torch.cat([xyz, torch.ones_like(xyz[..., -1:])], dim=-1) @ w2cd.t())[None, :, :3]
            grid = ((cam_xyz / cam_xyz[..., 2:3]) @ Kd.t()[None])[..., :2]
            mask = torch.prod(torch.cat([grid >= 0, grid <= torch.tensor([[[W - 1, H - 1]]], device=dev)], dim=-1), dim=-1, keepdim=True, dtype=torch.int8) > 0
            grid = torch.masked_select(grid, mask).reshape(1, -1, 2)
            grid[..., 0] = grid[..., 0] / ((W - 1.0) / 2.0) - 1.0
            grid[..., 1] = grid[..., 1] / ((H - 1.0) / 2.0) - 1.0
            col = sample(image, grid, mask)
            f = torch.cat([sample(m, grid, mask) for m in maps], dim=-1)
            cpc = (c2wd[None, :, 3] @ w2cd.t())[..., :3]
            dirs = cam_xyz[0] - cpc
            dirs = dirs / (torch.linalg.norm(dirs, dim=-1, keepdims=True) + 1e-6)
            dirs = (dirs @ c2wd[:3, :3].t())[None]
            conf = torch.ones_like(col[..., :1])
            state["stock"] = (premlp(torch.cat([f, col, dirs, conf], dim=-1)), col, dirs, conf)
    ours(); stock(); torch.cuda.synchronize()
    worst = max(float((a - b).abs().max()) for a, b in zip(state["ours"], state["stock"]))
    ma, mb, ta, tb, ca, cb = windows(ours, stock, 5)
    report("embed", "%d points of one 480x640 view: samples of image + 3 pyramid levels, premlp" % n, ma, mb, ta, tb, ca, cb, dict(max_abs_difference=worst))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "featnet_timing needs a GPU: there is no CPU fallback and no CPU timing"
        {"pyramid1": lambda: step_pyramid(1), "pyramid8": lambda: step_pyramid(8), "embed": step_embed}[args.step]()
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
            f.write("# tools/featnet_timing.py: medians of alternating device-event windows, HIP path vs the same stage in stock torch ops\n")
            f.write("\n".join(l[len("RESULT "):] for l in lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
