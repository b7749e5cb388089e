"""Times the front and the back of a camera-path frame (csrc/path.hip) at the bench frame's shape: 480 x 640, V = 4 reference views out of T = 200
frames of uint8, margin 10, one GPU.

  python tools/path_timing.py [--out profiles/path_timing.txt] [--points 2e6]

Two forms of the same frame's glue -- the dataset item of a free camera in front of the renderer, the 8-bit frame behind it:
  (a) pair      PathSampler.next() (hnr_path_item: selection + header, rays, reference images) + hnr_frame_store into a device clip
  (b) composed  what a caller composes today: frames.nearest_by_pose on the host (the train directions are a per-scene table, built once, outside),
                a one-frame pose-only stand-in FrameBank + set_nearest, BatchSampler.item, render_image's scatter (torch.zeros + index-put) and
                hnr_frame_metrics for the bytes
and beside them
  frame         the whole bench frame (hnr_bench: 2 M points, one launch of the fused forward), the cost both forms sit next to
  sel8192       hnr_pose_views alone for one pose against T = 8192 cameras (the entry's limit)

The parent opens no GPU: the measurement runs in a child process under its own time limit.  The child warms everything up, then times five
alternating windows per form, each about one second of back-to-back calls (sized from one timed call), with device events; a window ends in an event
synchronise, so host work between launches is paid for.  Reported: the median of the windows and their range, per call.
`--step kernels` queues 200 pairs and nothing else: the run to put under `rocprofv3 --kernel-trace --stats` for the selection launch's device time."""
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

T, H, W, V, MARGIN, P = 200, 480, 640, 4, 10, 20
LIMIT = 600                                                             # the child's time limit in seconds


def cameras(n, seed):
    """n cameras on a ring looking inwards, jittered"""
    import numpy as np
    from hybridneuralrendering_amd import scenes
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        a = 2 * np.pi * i / n
        eye = np.array([3.5 * np.cos(a), 3.5 * np.sin(a), 0.5]) + rng.uniform(-0.2, 0.2, size=3)
        out.append(scenes.look_at(eye, rng.uniform(-0.2, 0.2, size=3)))
    return np.stack(out).astype(np.float32)


def make_bank(dev, n=T, h=H, w=W):
    import numpy as np
    import torch
    from hybridneuralrendering_amd.frames import FrameBank
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, size=(8, h, w, 3), dtype=np.uint8)
    images = np.ascontiguousarray(base[np.arange(n) % 8])               # the content does not matter to either form
    c2w = cameras(n, 1)
    K = np.array([[577.59, 0, 318.9], [0, 578.73, 242.68], [0, 0, 1]], np.float32)
    return FrameBank(torch.from_numpy(images), c2w, K, dev), c2w, K


def setup(dev):
    import numpy as np
    import torch
    from hybridneuralrendering_amd import _lib, frames
    bank, c2w, K = make_bank(dev)
    poses = cameras(P, 2)
    sampler = frames.PathSampler(poses, K, bank, V, margin=MARGIN, near=0.1, far=8.0)
    R = sampler.R
    col = torch.rand((R, 3), device=dev) * 1.2 - 0.1                    # stands in for the renderer's colours
    clip8 = torch.empty((P, H, W, 3), dtype=torch.uint8, device=dev)
    L = _lib.lib()
    p = _lib.ptr
    state = dict(k=0, j=0)

    def pair():
        item = sampler.next()
        k = state["k"] % P
        state["k"] += 1
        _lib.check(L.hnr_frame_store(p(col), p(item["pixel_idx"]), None, R, H, W, p(clip8[k]), None, None, _lib.stream()), "hnr_frame_store")
        state["a"] = item

    train_dirs = np.stack([frames.center_raydir(K, M, W, H)[0] for M in c2w])   # per-scene constants of the host selection
    train_pos, ids = c2w[:, :3, 3], np.arange(T)
    zero = np.zeros((1, H, W, 3), np.uint8)
    nbytes = int(L.hnr_frame_metrics_scratch_bytes(H, W, 11))
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    row = torch.zeros((6,), dtype=torch.float64, device=dev)
    gt_full = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    gt8 = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)

    def composed():
        j = state["j"] % P
        state["j"] += 1
        table = frames.nearest_by_pose(poses[j:j + 1], K, [-1], train_pos, train_dirs, ids, V, W, H, False)
        one = frames.FrameBank(zero, poses[j:j + 1], K, dev).set_nearest(table, reference=bank)
        item = frames.BatchSampler(one, "random", size=1, margin=MARGIN, near=0.1, far=8.0).item(0)
        img = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
        px, py = item["pixel_idx"][:, 0].to(torch.long), item["pixel_idx"][:, 1].to(torch.long)
        img[py, px] = col
        _lib.check(L.hnr_frame_metrics(p(img), p(gt_full), H, W, None, None, None, 0, 11, 2.0, p(row), p(clip8[j]), p(gt8), p(scratch), _lib.stream()),
                   "hnr_frame_metrics")
        state["b"] = item

    return SimpleNamespace(sampler=sampler, bank=bank, pair=pair, composed=composed, state=state, clip8=clip8, poses=poses, K=K)


def timed(fn, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def step_pair(n_points):
    import numpy as np
    import torch
    from hybridneuralrendering_amd import frames
    from hnr_bench.common import build_world, render_frame
    dev = torch.device("cuda:0")
    s = setup(dev)
    # the two forms give the same item and the same bytes for the same frame
    s.pair()
    s.composed()
    torch.cuda.synchronize()
    for name in ("raydir", "pixel_idx", "images_nearest", "c2w_nearest", "campos"):
        assert torch.equal(s.state["a"][name], s.state["b"][name]), name
    first = s.clip8[0].clone()
    s.sampler.set_step(0)
    s.state["k"] = 0
    s.pair()
    assert torch.equal(s.clip8[0], first), "hnr_frame_store and hnr_frame_metrics disagree on the bytes"
    # the bench frame
    args = SimpleNamespace(scene="scene0241", points=n_points, width=W, height=H, margin=MARGIN, chunk=0)
    sc, _opt, _agg, cloud, rnd, cam = build_world(args, dev, 0)

    def frame():
        rnd._fm_key = None                                              # a new frame has new reference views
        render_frame(rnd, cloud, cam, sc, 0)

    big, _c, _K = make_bank(dev, n=8192, h=6, w=8)
    sel = frames.PathSampler(s.poses[:1], s.K, big, V, near=0.1, far=8.0, num_times=3)

    def sel8192():
        sel.views()

    fns = (("pair", s.pair), ("composed", s.composed), ("frame", frame), ("sel8192", sel8192))
    for _, fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    calls = {n: max(1, int(math.ceil(1000.0 / max(timed(fn, 3), 1e-3)))) for n, fn in fns}
    win = {n: [] for n, _ in fns}
    for _ in range(5):
        for n, fn in fns:
            win[n].append(timed(fn, calls[n]))
    med = lambda v: sorted(v)[len(v) // 2]
    rec = dict(step="pair", what="%d frames %dx%d uint8, V = %d, margin %d, %d path poses; frame = the bench frame at %.3g points" % (T, H, W, V, MARGIN, P, n_points))
    for n, _ in fns:
        rec[n + "_ms"] = round(med(win[n]), 4)
        rec[n + "_windows_ms"] = [round(v, 4) for v in win[n]]
        rec[n + "_calls_per_window"] = calls[n]
    spread = max(max(win[n]) - min(win[n]) for n in ("pair", "composed"))
    rec["composed_over_pair"] = round(rec["composed_ms"] / rec["pair_ms"], 2)
    rec["pair_not_slower_than_composed_beyond_the_spread"] = bool(rec["pair_ms"] <= rec["composed_ms"] + spread)
    rec["pair_share_of_frame"] = round(rec["pair_ms"] / rec["frame_ms"], 4)
    rec["composed_share_of_frame"] = round(rec["composed_ms"] / rec["frame_ms"], 4)
    rec["sel8192_slower_than_a_frame"] = bool(rec["sel8192_ms"] > rec["frame_ms"])
    print("RESULT " + json.dumps(rec), flush=True)
    return 0 if rec["pair_not_slower_than_composed_beyond_the_spread"] else 1


def step_kernels(_n_points):
    import torch
    dev = torch.device("cuda:0")
    s = setup(dev)
    for _ in range(200):
        s.pair()
    torch.cuda.synchronize()
    print("RESULT " + json.dumps(dict(step="kernels", calls=200, last_step=int(s.sampler.step.item()))), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["pair", "kernels"])
    ap.add_argument("--points", type=float, default=2.0e6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "path_timing needs a GPU: there is no CPU fallback"
        return {"pair": step_pair, "kernels": step_kernels}[args.step](args.points)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", "pair", "--points", repr(args.points)], capture_output=True, text=True,
                           timeout=LIMIT)
    except subprocess.TimeoutExpired:
        print("the measurement passed its time limit of %d s" % LIMIT)
        return 1
    got = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if not got:
        print("the measurement failed (exit %d)\n%s" % (r.returncode, r.stderr[-2000:]))
        return 1
    print(got[0], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/path_timing.py: the glue of one path frame at the bench shape, medians of five alternating one-second device-event windows, ms per call\n")
            f.write("# pair = hnr_path_item + hnr_frame_store; composed = host nearest_by_pose + stand-in bank + BatchSampler.item + torch scatter + hnr_frame_metrics;\n")
            f.write("# frame = the whole bench frame; sel8192 = hnr_pose_views for one pose against 8192 cameras\n")
            f.write(got[0][len("RESULT "):] + "\n")
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
