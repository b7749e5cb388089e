"""Times the two stages of the synthetic scenes' start (hybridneuralrendering_amd/cloud_init.py, csrc/hull.hip) against the reference's own formulas
written with stock torch ops on the same GPU -- what a user without this package's kernels has today; the reference is not imported.

  python tools/hull_timing.py [--out profiles/hull_timing.txt]

  hull  N = 3 M points against M = 100 alpha views of 800 x 800 (the shape of dev_scripts/w_n360): hnr_visual_hull_select (mask + compaction of xyz,
        confidence and view) against mvs_utils.alpha_masking (:573-607: the loop over the views, a dozen full-length ops per view) + `masking`
        (train_ft.py:157), transcribed; the reference's two torch.cuda.empty_cache() calls per view are LEFT OUT of the torch side (they would only slow
        it down).  Packing the alphas into bits (hnr_alpha_pack, once per scene) is timed separately (`pack_ms`).  70 % of the points lie inside the
        ball and pass all 100 views (no early exit), 30 % in a cube around it.
  occ   200 k points in one 512 x 640 view: hnr_point_occlusion + hnr_point_embed_vis against homo_warp_nongrid_occ (:333-369) with a device-side
        scatter_reduce("amin") in place of the host scatter_min, extract_from_2d_grid (grid_sample of the image and the three pyramid levels) and premlp as
        two nn.functional.linear calls.  The image pyramid is given to both sides.

The parent opens no GPU: it runs every step as a child process of its own under its own time limit and stops at the first step that fails.  Each child
warms both sides up, then times five alternating windows per side, each about one second of back-to-back calls, with device events, and reports the
median of the windows (tools/geo_filter_timing.py's `windows`).

  python tools/hull_timing.py --step profile     (under `rocprofv3 --kernel-trace --stats -- python ...`: three calls of each stage)
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

STEPS = (("hull", 300), ("occ", 240))                 # (name, time limit in seconds)
NEAR_FAR = (2.0, 6.0)


def look_at(pos):
    import numpy as np
    pos = np.asarray(pos, np.float64)
    z = -pos / np.linalg.norm(pos)
    x = np.cross(np.array([0.0, 0.0, 1.0]), z); x /= np.linalg.norm(x)
    M = np.eye(4)
    M[:3, 0], M[:3, 1], M[:3, 2], M[:3, 3] = x, np.cross(z, x), z, pos
    return M


def hull_scene(N, M, H, W, dev):
    import numpy as np
    import torch
    rng = np.random.default_rng(0)
    K = np.tile(np.array([[1111.0, 0, W / 2], [0, 1111.0, H / 2], [0, 0, 1]], np.float32), (M, 1, 1))
    c2w = np.stack([look_at([4.0 * np.cos(a) * np.cos(e), 4.0 * np.sin(a) * np.cos(e), 4.0 * np.sin(e)])
                    for a, e in zip(rng.uniform(0, 2 * np.pi, M), rng.uniform(0.05, 1.2, M))])
    w2c = np.linalg.inv(c2w).astype(np.float32)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    alphas = torch.empty((M, H, W), device=dev)
    for m in range(M):                                              # the silhouette of the unit ball
        d = torch.stack([(xx + 0.5 - K[m, 0, 2]) / K[m, 0, 0], (yy + 0.5 - K[m, 1, 2]) / K[m, 1, 1], torch.ones_like(xx)], -1) @ torch.from_numpy(c2w[m, :3, :3].T.astype(np.float32)).to(dev)
        o = torch.from_numpy(c2w[m, :3, 3].astype(np.float32)).to(dev)
        b = d @ o
        alphas[m] = ((b * b - (d * d).sum(-1) * (o @ o - 1.0)) > 0).float()
    ball = rng.standard_normal((int(0.7 * N), 3))
    ball *= (0.98 * rng.uniform(size=(ball.shape[0], 1)) ** (1 / 3)) / np.linalg.norm(ball, axis=1, keepdims=True)
    pts = np.concatenate([ball, rng.uniform(-1.6, 1.6, size=(N - ball.shape[0], 3))]).astype(np.float32)
    pts = pts[rng.permutation(N)]
    return torch.from_numpy(pts).to(dev), alphas, K, w2c


def torch_alpha_masking(points, alphas, Ks, w2cs, near_far, range_on, H, W):
    """mvs_utils.alpha_masking in stock torch ops (empty_cache() calls left out); Ks / w2cs: device tensors per view"""
    import torch
    w_xyz1 = torch.cat([points[..., :3], torch.ones_like(points[..., :1])], dim=-1)
    hull = None
    for i in range(alphas.shape[0]):
        cam = w_xyz1 @ w2cs[i].t()
        if near_far is not None:
            nf = torch.logical_and(cam[..., 2] >= (near_far[0] - 1.0), cam[..., 2] <= near_far[1])
        cam = cam[..., :3] @ Ks[i].t()
        xy = torch.floor(cam[:, :2] / cam[:, -1:] + 0.0).long()
        rm = None
        if range_on:
            rm = torch.logical_and(xy >= torch.zeros((1, 2), dtype=xy.dtype, device=xy.device), xy < torch.as_tensor([[W, H]], dtype=xy.dtype, device=xy.device))
            rm = torch.prod(rm, dim=-1) > 0
        xy[..., 0] = torch.clamp(xy[..., 0], min=0, max=W - 1)
        xy[..., 1] = torch.clamp(xy[..., 1], min=0, max=H - 1)
        mask = alphas[i][xy[..., 1], xy[..., 0]]
        if rm is not None:
            mask = mask + (~rm).to(torch.float32)
        mask = mask > 0.1
        if near_far is not None:
            mask = mask * nf
        hull = mask if hull is None else hull * mask
    return hull > 0


def step_hull():
    import torch
    from hybridneuralrendering_amd import cloud_init as ci
    from geo_filter_timing import windows
    dev = torch.device("cuda:0")
    N, M, H, W = 3000000, 100, 800, 800
    pts, alphas, K, w2c = hull_scene(N, M, H, W, dev)
    conf, view = torch.rand(N, device=dev), torch.randint(0, M, (N,), device=dev, dtype=torch.int32)
    vid_f = view.float()[:, None]
    Ks, Es = [torch.from_numpy(k).to(dev) for k in K], [torch.from_numpy(e).to(dev) for e in w2c]
    masks = ci.AlphaMasks(alphas, K, w2c, dev)
    state = {}

    def ours():
        state["ours"] = ci.visual_hull_select(pts, masks, near_far=NEAR_FAR, range_mask=False, conf=conf, view=view, want_mask=False)

    def pack():
        state["bits"] = ci.alpha_pack(alphas)

    def stock():
        m = torch_alpha_masking(pts, alphas, Ks, Es, NEAR_FAR, False, H, W)
        state["stock"] = (m, pts[m, ...], vid_f[m, ...], conf[m, ...])                  # `masking`
    ours(); pack(); stock(); torch.cuda.synchronize()
    n = int(state["ours"]["count"].item())
    differ = int(n != int(state["stock"][0].sum().item()))
    same = bool(torch.equal(state["ours"]["xyz"][:n], state["stock"][1])) if not differ else False
    mp, _, tp, _, cp, _ = windows(pack, None, 5)
    ma, mb, ta, tb, ca, cb = windows(ours, stock, 5)
    rec = dict(step="hull", what="%d points x %d views of %dx%d: visual_hull_select vs alpha_masking + masking in torch ops (no empty_cache)" % (N, M, H, W),
               hip_ms=round(ma, 4), torch_ms=round(mb, 4), torch_over_hip=round(mb / ma, 2), slowest_hip_over_fastest_torch=round(max(ta) / min(tb), 5),
               pack_ms=round(mp, 4), pack_windows_ms=[round(v, 4) for v in tp], hip_calls_per_window=ca, torch_calls_per_window=cb,
               hip_windows_ms=[round(v, 4) for v in ta], torch_windows_ms=[round(v, 4) for v in tb], survivors=n, survivor_share=round(n / N, 4),
               counts_differ=differ, survivor_xyz_identical=same, alpha_bytes_float=M * H * W * 4, alpha_bytes_bits=int(masks.bits.numel()) * 4,
               hip_ns_per_point=round(ma * 1e6 / N, 3))
    print("RESULT " + json.dumps(rec), flush=True)


def occ_scene(n, H, W, dev):
    import numpy as np
    import torch
    from hybridneuralrendering_amd.mvs_init import MvsInit
    rng = np.random.default_rng(1)
    K = np.array([[577.59, 0, 318.9], [0, 578.73, 242.68], [0, 0, 1]], np.float32)
    c2w = look_at([0.0, -3.0, 0.5]).astype(np.float32)
    w2c = torch.inverse(torch.from_numpy(c2w)).numpy()
    gx, gy = rng.uniform(-20, W + 20, n), rng.uniform(-20, H + 20, n)
    z = np.where(rng.uniform(size=n) < 0.5, 2.0, np.where(rng.uniform(size=n) < 0.5, 2.05, 2.4)) + 0.01 * rng.standard_normal(n)
    cam = np.stack([(gx - K[0, 2]) / K[0, 0] * z, (gy - K[1, 2]) / K[1, 1] * z, z], -1)
    xyz = (cam @ c2w[:3, :3].astype(np.float64).T + c2w[:3, 3]).astype(np.float32)
    torch.manual_seed(0)
    net = MvsInit().to(dev)
    img = torch.rand((3, H, W), device=dev)
    return torch.from_numpy(xyz).to(dev), K, c2w, w2c, img, net, torch.rand(n, device=dev)


def torch_occ_embed(cam_xyz, conf, K, c2w, cpc, maps, img, prm, H, W, tolerate=0.1):
    """homo_warp_nongrid_occ (scatter on the device) + extract_from_2d_grid + the dir branch + premlp, for view 0 of the points' own view"""
    import torch
    import torch.nn.functional as F
    grid = ((cam_xyz[..., :3] / cam_xyz[..., 2:3]) @ K.t())[..., :2]
    mask = torch.prod(torch.cat([grid >= 0, torch.ceil(grid) <= torch.tensor([[W - 1, H - 1]], device=grid.device)], dim=-1), dim=-1, keepdim=True, dtype=torch.int8) > 0
    g = torch.masked_select(grid, mask).reshape(-1, 2)
    z = torch.masked_select(cam_xyz[:, 2], mask[..., 0])
    hard = torch.ceil(g)
    index = (hard[..., 0] * H + hard[..., 1]).long()
    zmin = torch.full((H * W,), float("inf"), device=z.device).scatter_reduce(0, index, z, "amin", include_self=True)
    block = z <= (zmin[index] + tolerate)
    mask = mask.clone()
    mask[mask.clone()] = block
    gs = g[block]
    gs = torch.stack([gs[:, 0] / ((W - 1.0) / 2.0) - 1.0, gs[:, 1] / ((H - 1.0) / 2.0) - 1.0], dim=-1)
    cols = []
    for src in list(maps) + [img]:
        w = F.grid_sample(src[None], gs[None, None], mode="bilinear", padding_mode="zeros", align_corners=True)[0, :, 0].t()
        full = torch.zeros((cam_xyz.shape[0], src.shape[0]), device=w.device)
        full[mask[:, 0]] = w
        cols.append(full)
    d = cam_xyz - cpc[None]
    d = d / (torch.linalg.norm(d, dim=-1, keepdim=True) + 1e-6)
    d = d @ c2w[:3, :3].t()
    rows = torch.cat(cols + [d, conf[:, None]], dim=-1)
    h = F.leaky_relu(F.linear(rows, prm[0], prm[1]), 0.01)
    return F.leaky_relu(F.linear(h, prm[2], prm[3]), 0.01), mask[:, 0]


def step_occ():
    import torch
    from hybridneuralrendering_amd import cloud_init as ci, mvs_init
    from geo_filter_timing import windows
    dev = torch.device("cuda:0")
    n, H, W = 200000, 512, 640
    xyz, K, c2w, w2c, img, net, conf = occ_scene(n, H, W, dev)
    feats = net.get_image_features(img[None, None])
    maps = [feats[i][0] for i in (1, 2, 3)]
    cpc = ci.cam_pos_cam(c2w, w2c)
    premlp = net.premlp_packed()
    tK, tc, tE, tcpc = (torch.from_numpy(a).to(dev) for a in (K, c2w, w2c, cpc))
    prm = [net.premlp[0].weight.detach(), net.premlp[0].bias.detach(), net.premlp[2].weight.detach(), net.premlp[2].bias.detach()]
    cam_xyz = (torch.cat([xyz, torch.ones_like(xyz[:, :1])], dim=-1) @ tE.t())[:, :3].contiguous()
    state = {}

    def ours():
        vis = ci.point_occlusion(xyz, w2c, K, H, W, 0.1)
        state["ours"] = (mvs_init.point_embed(xyz, w2c, c2w, cpc, K, img, *maps, premlp, conf=conf, visible=vis)[0], vis)

    def occ_only():
        state["vis"] = ci.point_occlusion(xyz, w2c, K, H, W, 0.1)

    def stock():
        state["stock"] = torch_occ_embed(cam_xyz, conf, tK, tc, tcpc, maps, img, prm, H, W)
    ours(); occ_only(); stock(); torch.cuda.synchronize()
    differ = int((state["ours"][1].bool() != state["stock"][1]).sum().item())
    agree = state["ours"][1].bool() == state["stock"][1]
    err = float((state["ours"][0] - state["stock"][0])[agree].abs().max().item())
    mo, _, to, _, co, _ = windows(occ_only, None, 5)
    ma, mb, ta, tb, ca, cb = windows(ours, stock, 5)
    rec = dict(step="occ", what="%d points in one %dx%d view: point_occlusion + point_embed(visible) vs homo_warp_nongrid_occ + grid_sample + premlp in torch ops" % (n, H, W),
               hip_ms=round(ma, 4), torch_ms=round(mb, 4), torch_over_hip=round(mb / ma, 2), slowest_hip_over_fastest_torch=round(max(ta) / min(tb), 5),
               occlusion_only_ms=round(mo, 4), occlusion_windows_ms=[round(v, 4) for v in to], hip_calls_per_window=ca, torch_calls_per_window=cb,
               hip_windows_ms=[round(v, 4) for v in ta], torch_windows_ms=[round(v, 4) for v in tb], visible=int(state["ours"][1].sum().item()),
               flags_that_differ=differ, max_abs_embedding_difference_where_flags_agree=err)
    print("RESULT " + json.dumps(rec), flush=True)


def step_profile():
    import torch
    from hybridneuralrendering_amd import cloud_init as ci, mvs_init
    dev = torch.device("cuda:0")
    pts, alphas, K, w2c = hull_scene(3000000, 100, 800, 800, dev)
    masks = ci.AlphaMasks(alphas, K, w2c, dev)
    for _ in range(3):
        ci.visual_hull_select(pts, masks, near_far=NEAR_FAR, want_mask=False)
    xyz, K1, c2w, w2c1, img, net, conf = occ_scene(200000, 512, 640, dev)
    feats = net.get_image_features(img[None, None])
    maps = [feats[i][0] for i in (1, 2, 3)]
    for _ in range(3):
        vis = ci.point_occlusion(xyz, w2c1, K1, 512, 640, 0.1)
        mvs_init.point_embed(xyz, w2c1, c2w, ci.cam_pos_cam(c2w, w2c1), K1, img, *maps, net.premlp_packed(), conf=conf, visible=vis)
    torch.cuda.synchronize()
    print("profiled: alpha_pack once, 3 x visual_hull_select (3 M points x 100 views), 3 x point_occlusion + point_embed (200 k points)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS] + ["profile"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "hull_timing needs a GPU: there is no CPU fallback and no CPU timing"
        dict(hull=step_hull, occ=step_occ, profile=step_profile)[args.step]()
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
        lines.append(got[0])
        print(got[0], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/hull_timing.py: medians of alternating device-event windows, HIP vs the reference's formulas in stock torch ops\n")
            f.write("\n".join(l[len("RESULT "):] for l in lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
