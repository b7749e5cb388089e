"""Times the geometric-consistency filter of MVS depth maps (hybridneuralrendering_amd/geo_filter.py, csrc/geo_filter.hip) against the reference's own
formulas written with stock torch ops on the same GPU -- what a user without this package's kernels has today: the double loop over the views of
models/mvs/filter_utils.py:157-297 (reprojection with three matrix inverses per ordered pair, grid_sample, the two thresholds, the masked sums, the
final mask, the boolean-mask indexing, range_mask_torch), transcribed here; the reference is not imported.

  python tools/geo_filter_timing.py [--out profiles/geo_filter_timing.txt]

The parent opens no GPU: it runs every step (`v8`, `v50`, `v200`) as a child process of its own under its own time limit and stops at the first step
that fails.  Each child warms both sides up, then times five alternating windows per side, each about one second of back-to-back calls (the number of
calls is sized from one timed call; a call longer than a window is a window of one call), with device events, and reports the median of the windows
and their spread.  The HIP side is geo_filter.filter_views as a user calls it: camera tables (host inverses + upload), depth extraction, both kernels
and the one host read; `kernel_ms` is hnr_geo_consistency alone, timed the same way.

Sizes: V = 8 and V = 50 views of 480 x 640 on both sides; V = 200 for the HIP side only -- one torch call there is 39 800 ordered pairs, minutes, so
its figure is EXTRAPOLATED from V = 50 by the pair count (the torch side is a fixed set of full-frame ops per ordered pair) and marked so in the output.
Inputs are resident on the device on both sides.  Scene: a plane seen from cameras on a line, 0.3 % depth noise, a confidence map around the threshold.

  python tools/geo_filter_timing.py --step profile     (under `rocprofv3 --kernel-trace --stats -- python ...`: three calls of the kernel at V = 50 and V = 200)
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEPS = (("v8", 240), ("v50", 420), ("v200", 300))                 # (name, time limit in seconds)
H, W = 480, 640
CONF_THRESH, GEO_NUM = 0.5, 3


def windows(fn_a, fn_b, reps, target_ms=1000.0):
    """Alternating event windows -> (median_a, median_b, all_a, all_b, calls_a, calls_b), times in ms PER CALL (fn_b None: one side only)."""
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
    fns = [f for f in (fn_a, fn_b) if f is not None]
    calls = [max(1, int(math.floor(target_ms / max(timed(fn, 1), 1e-3)))) for fn in fns]
    out = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            out[k].append(timed(fn, calls[k]))
    med = lambda v: sorted(v)[len(v) // 2]
    if fn_b is None:
        return med(out[0]), None, out[0], None, calls[0], None
    return med(out[0]), med(out[1]), out[0], out[1], calls[0], calls[1]


def scene(V, dev):
    """depth [V,H,W], cam_xyz [V,H,W,3], conf, points_mask on the device; K [V,3,3], E [V,4,4] on the host."""
    import numpy as np
    import torch
    rng = np.random.default_rng(0)
    K = np.tile(np.array([[577.59, 0, 318.9], [0, 578.73, 242.68], [0, 0, 1]], np.float32), (V, 1, 1))
    E = np.zeros((V, 4, 4), np.float32)
    depth = np.zeros((V, H, W), np.float32)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    pix = np.stack([xx, yy, np.ones_like(xx)], -1)
    for v in range(V):
        pos = np.array([2.0 * (v / max(V - 1, 1) - 0.5), -2.0 + 0.3 * np.sin(v), 1.0 + 0.2 * np.cos(2.0 * v)])
        z = np.array([0.3 * np.sin(0.7 * v), 3.0, 0.1 * np.cos(v)]); z /= np.linalg.norm(z)
        x = np.cross(np.array([0.0, 0.0, 1.0]), z); x /= np.linalg.norm(x)
        M = np.eye(4)
        M[:3, 0], M[:3, 1], M[:3, 2], M[:3, 3] = x, np.cross(z, x), z, pos
        E[v] = np.linalg.inv(M).astype(np.float32)
        dirs = pix @ np.linalg.inv(K[v].astype(np.float64)).T.astype(np.float32) @ M[:3, :3].T.astype(np.float32)
        depth[v] = ((1.0 - pos[1]) / dirs[..., 1]) * (1.0 + 0.003 * rng.standard_normal((H, W)).astype(np.float32))
    depth[:, 100:140, 200:260] = 0.0
    d = torch.from_numpy(depth).to(dev)
    Ki = torch.from_numpy(np.stack([torch.inverse(torch.from_numpy(k)).numpy() for k in K])).to(dev)
    p = torch.from_numpy(pix).to(dev)
    cam = torch.einsum("vij,hwj->vhwi", Ki, p) * d[..., None]
    conf = torch.from_numpy(rng.uniform(0.0, 1.0, size=(V, H, W)).astype(np.float32)).to(dev)
    pm = torch.from_numpy(rng.uniform(size=(V, H, W)) > 0.02).to(dev)
    return d, cam.contiguous(), conf, pm, K, E


def torch_filter(cam_list, K_list, E_list, conf_list, pm_list, ranges):
    """filter_by_masks_gpu (manual_depth_view = 1, no far_plane_shift) in stock torch ops, one ordered pair at a time."""
    import torch
    import torch.nn.functional as F
    V = len(cam_list)
    dev = cam_list[0].device
    gy, gx = torch.meshgrid(torch.arange(0, H, device=dev), torch.arange(0, W, device=dev), indexing="ij")
    fx, fy = gx.reshape(-1), gy.reshape(-1)
    one = torch.ones_like(fx)
    rng_t = torch.as_tensor(ranges, device=dev, dtype=torch.float32)
    worlds, cams, confs, counts = [], [], [], []
    for r in range(V):
        d_ref, K_r, E_r = cam_list[r][..., 2], K_list[r], E_list[r]
        total, n_ok = 0, 0
        for s in range(V):
            if s == r:
                continue
            d_src, K_s, E_s = cam_list[s][..., 2], K_list[s], E_list[s]
            p_ref = torch.matmul(torch.linalg.inv(K_r), torch.stack([fx, fy, one], dim=0) * d_ref.reshape(-1))
            p_src = torch.matmul(torch.matmul(E_s, torch.linalg.inv(E_r)), torch.cat([p_ref, one[None].to(p_ref.dtype)], dim=0))[:3]
            k_src = torch.matmul(K_s, p_src)
            xy = k_src[:2] / k_src[2:3]
            xs, ys = xy[0].reshape(H, W), xy[1].reshape(H, W)
            grid = torch.stack([xs * 2 / (W - 1) - 1, ys * 2 / (H - 1) - 1], dim=-1)[None]
            sd = F.grid_sample(d_src[None, None], grid, align_corners=True, mode="bilinear", padding_mode="border")
            p_back = torch.matmul(torch.linalg.inv(K_s), torch.cat([xy, one[None].to(xy.dtype)], dim=0) * sd.reshape(-1))
            p_rep = torch.matmul(torch.matmul(E_r, torch.linalg.inv(E_s)), torch.cat([p_back, one[None].to(p_back.dtype)], dim=0))[:3]
            d_rep = p_rep[2].reshape(H, W)
            k_rep = torch.matmul(K_r, p_rep)
            xy_rep = k_rep[:2] / k_rep[2:3]
            dist = torch.sqrt((xy_rep[0].reshape(H, W) - gx) ** 2 + (xy_rep[1].reshape(H, W) - gy) ** 2)
            rel = torch.abs(d_rep - d_ref) / d_ref
            ok = torch.logical_and(dist < 1, rel < 0.01)
            d_rep[~ok] = 0
            n_ok = n_ok + ok.to(torch.int32)
            total = total + d_rep
        avg = (total + d_ref) / (n_ok + 1)
        keep = torch.logical_and(conf_list[r] > CONF_THRESH, pm_list[r])
        if V > 1:
            keep = torch.logical_and(keep, n_ok >= GEO_NUM)
        cam = torch.cat([cam_list[r][..., :2][keep, :], avg[keep][..., None]], dim=-1)
        world = torch.cat([cam, torch.ones_like(cam[..., 0:1])], dim=-1) @ torch.inverse(E_r).transpose(0, 1)
        cf = conf_list[r][keep]
        m = torch.prod(torch.logical_and(world[..., :3] >= rng_t[None, :3], world[..., :3] <= rng_t[None, 3:]), dim=-1) > 0
        worlds.append(world[m][:, :3]); cams.append(cam[m]); confs.append(cf[m]); counts.append(n_ok)
    return cams, worlds, confs, counts


def step_views(V, with_torch):
    import types
    import numpy as np
    import torch
    from hybridneuralrendering_amd import geo_filter as gf
    dev = torch.device("cuda:0")
    depth, cam, conf, pm, K, E = scene(V, dev)
    ranges = [-0.9, -100.0, -100.0, 100.0, 100.0, 100.0]
    opt = types.SimpleNamespace(manual_depth_view=1, far_plane_shift=None, depth_conf_thresh=CONF_THRESH, geo_cnsst_num=GEO_NUM, default_conf=-1.0, ranges=ranges)
    state = {}

    def ours():
        state["ours"] = gf.filter_views(cam, conf, pm, gf.CameraTables(K, E, dev), opt)
    tab = gf.CameraTables(K, E, dev)

    def kernel():
        state["kernel"] = gf.geometric_consistency(depth, tab)
    cam_l, conf_l, pm_l = [cam[v] for v in range(V)], [conf[v] for v in range(V)], [pm[v] for v in range(V)]
    K_l, E_l = [torch.from_numpy(K[v]).to(dev) for v in range(V)], [torch.from_numpy(E[v]).to(dev) for v in range(V)]

    def stock():
        state["stock"] = torch_filter(cam_l, K_l, E_l, conf_l, pm_l, ranges)
    ours(); kernel(); torch.cuda.synchronize()
    pairs, px = V * (V - 1), H * W
    extra = dict(views=V, ordered_pairs=pairs, kept_points=int(state["ours"]["world"].shape[0]),
                 count_histogram=np.bincount(state["ours"]["count"].reshape(-1).cpu().numpy().clip(0, 8), minlength=9).tolist())
    mk, _, tk, _, ck, _ = windows(kernel, None, 5)
    extra.update(kernel_ms=round(mk, 4), kernel_windows_ms=[round(v, 4) for v in tk], kernel_calls_per_window=ck,
                 kernel_gather_bytes=pairs * px * 16, kernel_gather_GBps=round(pairs * px * 16 / (mk * 1e-3) / 1e9, 1),
                 kernel_ns_per_pair_pixel=round(mk * 1e6 / (pairs * px), 4))
    if with_torch:
        stock(); torch.cuda.synchronize()
        differ = sum(int((a != b).sum()) for a, b in zip(state["ours"]["count"], state["stock"][3]))
        extra.update(count_pixels_that_differ=differ, torch_kept_points=int(sum(w.shape[0] for w in state["stock"][1])))
        ma, mb, ta, tb, ca, cb = windows(ours, stock, 5)
        rec = dict(step="v%d" % V, what="%d views of %dx%d, filter_views vs the reference's formulas in torch ops" % (V, H, W), hip_ms=round(ma, 4),
                   torch_ms=round(mb, 4), torch_over_hip=round(mb / ma, 2), slowest_hip_over_fastest_torch=round(max(ta) / min(tb), 5),
                   hip_calls_per_window=ca, torch_calls_per_window=cb, hip_windows_ms=[round(v, 4) for v in ta], torch_windows_ms=[round(v, 4) for v in tb],
                   torch_ms_per_ordered_pair=round(mb / pairs, 5))
    else:
        ma, _, ta, _, ca, _ = windows(ours, None, 5)
        rec = dict(step="v%d" % V, what="%d views of %dx%d, filter_views only (the torch side is extrapolated by the parent)" % (V, H, W), hip_ms=round(ma, 4),
                   hip_calls_per_window=ca, hip_windows_ms=[round(v, 4) for v in ta])
    rec.update(extra)
    print("RESULT " + json.dumps(rec), flush=True)


def step_profile():
    import torch
    from hybridneuralrendering_amd import geo_filter as gf
    dev = torch.device("cuda:0")
    for V in (50, 200):
        depth, _, _, _, K, E = scene(V, dev)
        tab = gf.CameraTables(K, E, dev)
        for _ in range(3):
            gf.geometric_consistency(depth, tab)
        torch.cuda.synchronize()
        print("profiled V = %d: 3 calls, %d ordered pairs x %d pixels x 16 gather bytes each" % (V, V * (V - 1), H * W), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS] + ["profile"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "geo_filter_timing needs a GPU: there is no CPU fallback and no CPU timing"
        if args.step == "profile":
            step_profile()
        else:
            step_views(int(args.step[1:]), with_torch=args.step != "v200")
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
        rec = json.loads(got[0][len("RESULT "):])
        if step == "v200":                                            # the torch side by pair count, from the V = 50 measurement
            v50 = json.loads(lines[-1][len("RESULT "):])
            rec["torch_ms_EXTRAPOLATED_by_pair_count_from_v50"] = round(v50["torch_ms_per_ordered_pair"] * rec["ordered_pairs"], 1)
            rec["fastest_torch_window_EXTRAPOLATED_ms"] = round(min(v50["torch_windows_ms"]) / v50["ordered_pairs"] * rec["ordered_pairs"], 1)
            rec["torch_over_hip_EXTRAPOLATED"] = round(rec["torch_ms_EXTRAPOLATED_by_pair_count_from_v50"] / rec["hip_ms"], 2)
        lines.append("RESULT " + json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/geo_filter_timing.py: medians of alternating device-event windows, HIP filter vs the reference's formulas in stock torch ops\n")
            f.write("\n".join(l[len("RESULT "):] for l in lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
