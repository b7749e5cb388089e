"""Times the cloud initialisation from depth frames (hybridneuralrendering_amd/cloud_init.py) against the same stages written with stock torch ops on
the same GPU -- what a user without this package's kernels has today: the reference's own formulas (data/scannet_ft_dataset.py:616-642,
run/train_ft.py:48-57, models/mvs/mvs_utils.py:299-315, :411-420) with torch.unique + index_add for the scatter mean torch_scatter would do.

  python tools/cloud_init_timing.py [--out profiles/cloud_init_timing.txt]

The parent opens no GPU: it runs every step (`fuse`, `nearest`, `attrs`) as a child process of its own under its own time limit and stops at the first
step that fails.  Each child warms both sides up, then times five alternating windows per side, each about one
second of back-to-back calls (the number of calls is sized from one timed call), with device events (a window ends in an event synchronise, so host reads
inside the torch side -- its boolean-mask index and torch.unique -- are paid for) and reports the median of the windows and their spread.

Sizes: 200 synthetic 480x640 uint16 frames (already on the device on both sides: no file or PCIe time), frame_vox_res 100; nearest view for
N = 2 M points and M = 300 cameras; attributes for 200 k points from one 480x640 image and one [32,120,160] feature map."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEPS = (("fuse", 420), ("nearest", 240), ("attrs", 180))          # (name, time limit in seconds)


def windows(fn_a, fn_b, reps, target_ms=1000.0):
    """Alternating event windows -> (median_a, median_b, all_a, all_b, calls_a, calls_b), times in ms PER CALL.  Each side's window holds as many
    back-to-back calls as fill about target_ms (sized from one timed call after the warm-up), so a short stage is not timed in a window that measures
    the clock and the scheduler."""
    import math
    import torch

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / calls
    calls = [max(1, int(math.ceil(target_ms / max(timed(fn, 3), 1e-3)))) for fn in (fn_a, fn_b)]
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(fn_a, calls[0]))
        tb.append(timed(fn_b, calls[1]))
    med = lambda v: sorted(v)[len(v) // 2]
    return med(ta), med(tb), ta, tb, calls[0], calls[1]


def report(step, what, ours, torch_ms, a, b, calls_a, calls_b, extra=None):
    rec = dict(step=step, what=what, hip_ms=round(ours, 4), torch_ms=round(torch_ms, 4), torch_over_hip=round(torch_ms / ours, 2),
               hip_calls_per_window=calls_a, torch_calls_per_window=calls_b,
               hip_windows_ms=[round(v, 4) for v in a], torch_windows_ms=[round(v, 4) for v in b])
    rec.update(extra or {})
    print("RESULT " + json.dumps(rec), flush=True)


def synthetic_frames(n_frames, dev):
    import numpy as np
    import torch
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:480, 0:640]
    frames, poses = [], []
    for k in range(8):                                                # 8 distinct depth images: rooms of smooth walls with holes
        d = 1500 + 300 * k + 600 * np.sin(xx / (90.0 + 7 * k)) * np.cos(yy / (70.0 + 5 * k)) + rng.normal(scale=4.0, size=xx.shape)
        d[rng.uniform(size=d.shape) < 0.05] = 0
        frames.append(torch.from_numpy(d.clip(0, 65535).astype(np.uint16).view(np.int16)).to(dev))
    for i in range(n_frames):
        a = 2 * np.pi * i / n_frames
        M = np.eye(4, dtype=np.float32)
        M[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
        M[:3, 3] = [0.02 * i, 0.0, 0.01 * i]
        poses.append(M)
    K = np.array([[577.59, 0, 318.9], [0, 578.73, 242.68], [0, 0, 1]], np.float32)
    return frames, poses, K


def step_fuse():
    import numpy as np
    import torch
    from hybridneuralrendering_amd.cloud_init import DepthFusion
    dev = torch.device("cuda:0")
    n_frames = 200
    frames, poses, K = synthetic_frames(n_frames, dev)
    poses_dev = [torch.from_numpy(p).to(dev) for p in poses]
    Ki_t = torch.inverse(torch.from_numpy(K)).t().to(dev)
    py, px = torch.meshgrid(torch.arange(0, 480, dtype=torch.float32, device=dev), torch.arange(0, 640, dtype=torch.float32, device=dev), indexing="ij")
    img_xy = torch.stack([px, py], dim=-1)
    state = {}

    def ours():
        f = DepthFusion(200 * 40000, dev, K, frame_vox_res=100)
        for i in range(n_frames):
            f.add(frames[i % 8], poses[i])
        state["ours"] = f.points()

    def vox_xyz(xyz, res):                                            # construct_vox_points_xyz with torch.unique + index_add for scatter_mean
        mn, mx = torch.min(xyz, dim=-2)[0], torch.max(xyz, dim=-2)[0]
        edge = torch.max(mx - mn) * 1.05
        smin = (mx + mn) / 2 - edge / 2
        sz = edge / res
        _, inv = torch.unique(torch.floor((xyz - smin[None]) / sz).to(torch.int32), dim=0, return_inverse=True)
        n = int(inv.max()) + 1
        s = torch.zeros((n, 3), device=xyz.device).index_add_(0, inv, xyz)
        c = torch.zeros((n,), device=xyz.device).index_add_(0, inv, torch.ones_like(inv, dtype=torch.float32))
        return s / c[:, None]

    def stock():
        allp = torch.zeros([0, 3], device=dev)
        for i in range(n_frames):
            raw = (frames[i % 8].to(torch.int32) & 0xffff).to(torch.float32) / 1000
            raw[raw > 8.0] = 0
            raw[raw < 0.3] = 0
            depth = raw[..., None]
            cam = torch.cat([img_xy * depth, depth], dim=-1) @ Ki_t
            cam = cam[cam[..., 2] > 0, :]
            cam = torch.cat([cam, torch.ones_like(cam[..., :1])], dim=-1)
            world = (cam.view(-1, 4) @ poses_dev[i].t())[..., :3]
            allp = torch.cat([allp, vox_xyz(world, 100)], dim=0)
        state["stock"] = allp
    ours(); stock(); torch.cuda.synchronize()
    a, b = state["ours"], state["stock"]
    # the torch side's matmuls round differently from the kernel's chained products, so a point within an ulp of a cell face may change voxel: the
    # two clouds need not have the same number of points; both counts are reported
    ma, mb, ta, tb, ca, cb = windows(ours, stock, 5)
    report("fuse", "%d frames 480x640, frame_vox_res 100" % n_frames, ma, mb, ta, tb, ca, cb,
           dict(per_frame_hip_ms=round(ma / n_frames, 4), per_frame_torch_ms=round(mb / n_frames, 4), hip_points=int(a.shape[0]), torch_points=int(b.shape[0])))


def step_nearest():
    import torch
    from hybridneuralrendering_amd.cloud_init import nearest_view
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    xyz = (torch.rand((2000000, 3), generator=g) * torch.tensor([8.0, 6.0, 3.0])).to(dev)
    campos = (torch.rand((300, 3), generator=g) * torch.tensor([8.0, 6.0, 3.0])).to(dev)
    d = torch.randn((300, 3), generator=g)
    camdir = (d / d.norm(dim=1, keepdim=True)).to(dev)
    state = {}

    def ours():
        state["ours"] = nearest_view(campos, camdir, xyz)

    def stock():                                                      # run/train_ft.py:48-57
        cam_ind = torch.zeros([0, 1], device=dev, dtype=torch.long)
        step = 10000
        for i in range(0, len(xyz), step):
            dists = xyz[i:min(len(xyz), i + step), None, :] - campos[None, ...]
            norm = torch.norm(dists, dim=-1)
            dirs = dists / (norm[..., None] + 1e-6)
            dists = norm / 200 + (1.1 - torch.sum(dirs * camdir[None, :], dim=-1))
            cam_ind = torch.cat([cam_ind, torch.argmin(dists, dim=1).view(-1, 1)], dim=0)
        state["stock"] = cam_ind
    ours(); stock(); torch.cuda.synchronize()
    differ = int((state["ours"] != state["stock"]).sum())
    ma, mb, ta, tb, ca, cb = windows(ours, stock, 5)
    report("nearest", "N = 2000000 points, M = 300 cameras", ma, mb, ta, tb, ca, cb, dict(views_that_differ=differ))


def step_attrs():
    import numpy as np
    import torch
    import torch.nn.functional as F
    from hybridneuralrendering_amd import cloud_init as ci
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    n, H, W = 200000, 480, 640
    image = torch.rand((3, H, W), generator=g).to(dev)
    fmap = torch.randn((32, 120, 160), generator=g).to(dev)
    K = np.array([[577.59, 0, 318.9], [0, 578.73, 242.68], [0, 0, 1]], np.float32)
    c2w = np.eye(4, dtype=np.float32)
    c2w[:3, 3] = [0.3, -0.2, 0.1]
    w2c = torch.inverse(torch.from_numpy(c2w)).numpy()
    cam = torch.stack([torch.rand(n, generator=g) * 1.4 - 0.7, torch.rand(n, generator=g) * 1.1 - 0.55, torch.ones(n)], -1) * (torch.rand((n, 1), generator=g) * 3 + 0.5)
    xyz = (cam + torch.tensor([0.3, -0.2, 0.1])).to(dev)
    Kd, c2wd, w2cd = torch.from_numpy(K).to(dev), torch.from_numpy(c2w).to(dev), torch.from_numpy(w2c).to(dev)
    state = {}

    def ours():
        state["ours"] = ci.query_point_attributes(xyz, image, c2w, w2c, K, feature_maps=[fmap])

    def sample(src, grid, mask):                                      # extract_from_2d_grid
        w = F.grid_sample(src[None], grid[:, None, ...], mode="bilinear", padding_mode="zeros", align_corners=True)
        w = w.permute(0, 2, 3, 1).view(1, -1, src.shape[0])
        full = torch.zeros([1, mask.shape[1], src.shape[0]], device=dev)
        full[0, mask[0, :, 0], :] = w
        return full

    def stock():
        cam_xyz = (torch.cat([xyz, torch.ones_like(xyz[..., -1:])], dim=-1) @ w2cd.t())[None, :, :3]
        grid = ((cam_xyz / cam_xyz[..., 2:3]) @ Kd.t()[None])[..., :2]
        mask = torch.prod(torch.cat([grid >= 0, grid <= torch.tensor([[[W - 1, H - 1]]], device=dev)], dim=-1), dim=-1, keepdim=True, dtype=torch.int8) > 0
        grid = torch.masked_select(grid, mask).reshape(1, -1, 2)
        grid[..., 0] = grid[..., 0] / ((W - 1.0) / 2.0) - 1.0
        grid[..., 1] = grid[..., 1] / ((H - 1.0) / 2.0) - 1.0
        col, feat = sample(image, grid, mask), sample(fmap, grid, mask)
        cpc = (c2wd[None, :, 3] @ w2cd.t())[..., :3]
        dirs = cam_xyz[0] - cpc
        dirs = dirs / (torch.linalg.norm(dirs, dim=-1, keepdims=True) + 1e-6)
        state["stock"] = (feat, col, (dirs @ c2wd[:3, :3].t())[None], torch.ones_like(col[..., :1]))
    ours(); stock(); torch.cuda.synchronize()
    worst = max(float((a - b).abs().max()) for a, b in zip(state["ours"], state["stock"]))
    ma, mb, ta, tb, ca, cb = windows(ours, stock, 5)
    report("attrs", "%d points, image [3,480,640] + feature map [32,120,160]" % n, ma, mb, ta, tb, ca, cb, dict(max_abs_difference=worst))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "cloud_init_timing needs a GPU: there is no CPU fallback and no CPU timing"
        {"fuse": step_fuse, "nearest": step_nearest, "attrs": step_attrs}[args.step]()
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
            f.write("# tools/cloud_init_timing.py: medians of alternating device-event windows, HIP path vs the same stage in stock torch ops\n")
            f.write("\n".join(l[len("RESULT "):] for l in lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
