"""Times one training batch drawn from a device-resident frame bank (hybridneuralrendering_amd/frames.py) at the C3 shape: 200 frames of 480x640
uint8, `random` 56 x 56 rays, V = 4 reference views, one GPU.

  python tools/frame_batch_timing.py [--out profiles/frame_batch_timing.txt]

Three forms of the same batch (pixel coordinates, raydir, gt_image, the four reference images as float32, their poses):
  (a) hip    BatchSampler.next(): three launches, frame number and step counter read on the device
  (b) torch  stock torch ops on the same device-resident uint8 bank: torch.randint, indexing, .float() / 255, a matmul for the rays
  (c) host   the reference's way (data/scannet_ft_dataset.py:821-960): numpy on the host from host arrays, then the uploads.  Decoding and resizing
             the five JPEGs -- most of the reference's cost -- are NOT included, so (c) flatters the host path.

The parent opens no GPU: the measurement runs in a child process under its own time limit.  The child warms all three up, then times five alternating
windows per form, each about one second of back-to-back calls (sized from one timed call), with device events; a window ends in an event
synchronise, so host work between launches is paid for.  Reported: the median of the windows and their range, per call.
`--step kernels` queues 200 next() calls and nothing else: the run to put under `rocprofv3 --kernel-trace --stats` for the kernel times."""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F, H, W, V, S, MARGIN = 200, 480, 640, 4, 56, 0
LIMIT = 300                                                             # the child's time limit in seconds


def make_bank(dev):
    import numpy as np
    import torch
    from hybridneuralrendering_amd.frames import FrameBank, nearest_by_id
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, size=(8, H, W, 3), dtype=np.uint8)
    images = np.ascontiguousarray(base[np.arange(F) % 8])               # 184 MB; the content does not matter to any of the three forms
    poses = []
    for i in range(F):
        a = 2 * np.pi * i / F
        M = np.eye(4, dtype=np.float32)
        M[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
        M[:3, 3] = [0.02 * i, 0.0, 0.01 * i]
        poses.append(M)
    c2w = np.stack(poses)
    K = np.array([[577.59, 0, 318.9], [0, 578.73, 242.68], [0, 0, 1]], np.float32)
    ids = np.arange(F) * 5
    bank = FrameBank(torch.from_numpy(images), c2w, K, dev, ids=ids, total_num_image=5 * F)
    table = nearest_by_id(ids, ids, V, exclude_self=True)
    bank.set_nearest(table)
    return bank, images, c2w, K, table


def step_batch():
    import numpy as np
    import torch
    from hybridneuralrendering_amd.frames import BatchSampler
    dev = torch.device("cuda:0")
    bank, images, c2w, K, table = make_bank(dev)
    sched = np.random.default_rng(1).permutation(F)
    sampler = BatchSampler(bank, "random", size=S, margin=MARGIN, seed=1, near=0.1, far=8.0).set_schedule(sched)
    R = S * S
    state = dict(i=0, j=0)
    table_dev = bank.nearest.long()
    K_dev = bank.intrinsic

    def hip():
        state["a"] = sampler.next()

    def stock():
        row = int(sched[state["i"] % F]); state["i"] += 1
        px = torch.randint(MARGIN, W - MARGIN, (R,), device=dev)
        py = torch.randint(MARGIN, H - MARGIN, (R,), device=dev)
        gt = bank.images[row, py, px].float() / 255
        x = (px.float() + 0.5 - K_dev[0, 2]) / K_dev[0, 0]
        y = (py.float() + 0.5 - K_dev[1, 2]) / K_dev[1, 1]
        M = bank.c2w[row]
        raydir = torch.stack([x, y, torch.ones_like(x)], dim=-1) @ M[:3, :3].t()
        nr = table_dev[row]
        c2w_n = bank.c2w[nr]
        state["b"] = dict(pixel_idx=torch.stack([px, py], dim=-1).float(), raydir=raydir, gt_image=gt, images_nearest=bank.images[nr].float() / 255,
                          c2w_nearest=c2w_n, w2c_nearest=bank.w2c[nr], campos_nearest=c2w_n[:, :3, 3], campos=M[:3, 3], camrotc2w=M[:3, :3])

    rng = np.random.default_rng(2)
    w2c_host = np.linalg.inv(c2w).astype(np.float32)

    def host():
        row = int(sched[state["j"] % F]); state["j"] += 1
        px = rng.integers(MARGIN, W - MARGIN, size=(S, S)).astype(np.float32)
        py = rng.integers(MARGIN, H - MARGIN, size=(S, S)).astype(np.float32)
        full = images[row].astype(np.float32) / 255                     # gt_image_full: the transform of the target frame
        gt = full[py.astype(np.int32), px.astype(np.int32)].reshape(-1, 3)
        x = (px + 0.5 - K[0, 2]) / K[0, 0]
        y = (py + 0.5 - K[1, 2]) / K[1, 1]
        raydir = (np.stack([x, y, np.ones_like(x)], axis=-1) @ c2w[row][:3, :3].T).reshape(-1, 3).astype(np.float32)
        nr = table[row]
        imgs = images[nr].astype(np.float32) / 255
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, non_blocking=True)
        state["c"] = dict(pixel_idx=up(np.stack([px, py], axis=-1).reshape(-1, 2)), raydir=up(raydir), gt_image=up(gt), images_nearest=up(imgs),
                          c2w_nearest=up(c2w[nr]), w2c_nearest=up(w2c_host[nr]), campos_nearest=up(c2w[nr][:, :3, 3]), campos=up(c2w[row][:3, 3]),
                          camrotc2w=up(c2w[row][:3, :3]))

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / calls
    fns = (("hip", hip), ("torch", stock), ("host", host))
    for _, fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for k in ("b", "c"):                                                # the three forms produce the same tensors
        for name in ("raydir", "gt_image", "images_nearest"):
            assert state[k][name].shape == state["a"][name].shape and state[k][name].dtype == state["a"][name].dtype, (k, name)
    calls = {n: max(1, int(math.ceil(1000.0 / max(timed(fn, 3), 1e-3)))) for n, fn in fns}
    win = {n: [] for n, _ in fns}
    for _ in range(5):
        for n, fn in fns:
            win[n].append(timed(fn, calls[n]))
    med = lambda v: sorted(v)[len(v) // 2]
    rec = dict(step="batch", what="%d frames %dx%d uint8, random %dx%d rays, V = %d" % (F, H, W, S, S, V))
    for n, _ in fns:
        rec[n + "_ms"] = round(med(win[n]), 4)
        rec[n + "_windows_ms"] = [round(v, 4) for v in win[n]]
        rec[n + "_calls_per_window"] = calls[n]
    rec["torch_over_hip"] = round(rec["torch_ms"] / rec["hip_ms"], 2)
    rec["host_over_hip"] = round(rec["host_ms"] / rec["hip_ms"], 2)
    rec["hip_beats_torch_by_more_than_the_spread"] = bool(max(win["hip"]) < min(win["torch"]))
    print("RESULT " + json.dumps(rec), flush=True)


def step_kernels():
    import numpy as np
    import torch
    from hybridneuralrendering_amd.frames import BatchSampler
    dev = torch.device("cuda:0")
    bank = make_bank(dev)[0]
    sampler = BatchSampler(bank, "random", size=S, margin=MARGIN, seed=1, near=0.1, far=8.0).set_schedule(np.arange(F))
    for _ in range(200):
        sampler.next()
    torch.cuda.synchronize()
    print("RESULT " + json.dumps(dict(step="kernels", calls=200, last_step=int(sampler.step.item()))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["batch", "kernels"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "frame_batch_timing needs a GPU: there is no CPU fallback"
        {"batch": step_batch, "kernels": step_kernels}[args.step]()
        return 0
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", "batch"], capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        print("the measurement passed its time limit of %d s" % LIMIT)
        return 1
    got = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not got:
        print("the measurement failed (exit %d)\n%s" % (r.returncode, r.stderr[-2000:]))
        return 1
    print(got[0], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/frame_batch_timing.py: one batch at the C3 shape, medians of five alternating one-second device-event windows, ms per call\n")
            f.write("# (a) hip = BatchSampler.next(), (b) torch = stock torch ops on the same device uint8 bank, (c) host = numpy + uploads (no JPEG decode)\n")
            f.write(got[0][len("RESULT "):] + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
