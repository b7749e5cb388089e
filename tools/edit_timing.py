"""Times the bench frame (2 M points, 640 x 480 minus a 10-pixel margin = 285 200 rays, one hnr_render_forward call) with and without the per-point
rotations of an edited scene (render.PartTable; csrc/chain.hip chain_gather_kernel<REC, ROT>), and this build against another build of the library.

  python tools/edit_timing.py [--out profiles/edit_timing.txt] [--parent path/to/the/parent/commit's/libhnr_hip.so] [--points 2e6]

Rows (one child process under its own time limit; the parent process opens no GPU):
  plain        the un-rotated frame with this build;
  plain_parent the same frame with hnr_render_forward of the library given by --parent (the parent commit's build: a `git worktree` of it,
               `make -C hybridneuralrendering_amd/csrc`), called in the same process on the same buffers -- expected equal to `plain`: the
               ROT = false kernels are the parent's instruction for instruction;
  rotated      the same frame, the cloud in two parts (points with x > median turned by 0.9 rad about (0.3, -0.5, 0.8)).
Medians of five alternating windows of about one second of back-to-back frames, device events.  Then one frame of `plain` and of `rotated` with the
library's stage events: the chain_gather stage times.  The pictures of plain and plain_parent are compared bit for bit before timing.
"""
import argparse
import ctypes
import json
import math
import os
import subprocess
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LIMIT_S = 540


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


class _OtherForward:
    """This build's library with hnr_render_forward taken from another build (same ABI up to the struct tail the other build does not read)."""

    def __init__(self, mine, path):
        self._mine = mine
        other = ctypes.CDLL(path)
        other.hnr_render_forward.restype = mine.hnr_render_forward.restype
        other.hnr_render_forward.argtypes = mine.hnr_render_forward.argtypes
        self.hnr_render_forward = other.hnr_render_forward
        self._other = other

    def __getattr__(self, name):
        return getattr(self._mine, name)


def child(n_points, parent):
    import numpy as np
    import torch
    from hnr_bench.common import build_world, render_frame
    from hybridneuralrendering_amd import _lib
    from hybridneuralrendering_amd.render import PointCloud
    dev = torch.device("cuda:0")
    args = SimpleNamespace(scene="scene0241", points=n_points, width=640, height=480, margin=10, knn_order=None)
    sc, opt, agg, cloud, rnd, cam = build_world(args, dev, 0)
    a = np.array([0.3, -0.5, 0.8])
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    rot = torch.from_numpy((np.eye(3) + np.sin(0.9) * K + (1 - np.cos(0.9)) * (K @ K)).astype(np.float32)).to(dev)
    part = (cloud.xyz[:, 0] > cloud.xyz[:, 0].median()).to(torch.int32)
    rotated = PointCloud(cloud.xyz, cloud.emb, cloud.conf, cloud.dir, cloud.color, Rw2c=(part, torch.stack([torch.eye(3, device=dev), rot])))
    mine = _lib.lib()
    frame = lambda c: render_frame(rnd, c, cam, sc, 0)[0]
    fns = dict(plain=lambda: frame(cloud))
    rec = dict(what="bench frame, %d points, %d rays, one hnr_render_forward call per frame" % (n_points, cam["raydir"].shape[0]))
    if parent:
        other = _OtherForward(mine, parent)

        def with_parent():
            _lib._lib = other
            try:
                return frame(cloud)
            finally:
                _lib._lib = mine
        fns["plain_parent"] = with_parent
        rec["plain_equals_parent_bit_for_bit"] = bool(torch.equal(fns["plain"](), with_parent()))
    fns["rotated"] = lambda: frame(rotated)
    rec["max_abs_colour_change_by_rotation"] = round(float((fns["rotated"]() - fns["plain"]()).abs().max()), 4)
    for _ in range(2):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    for k, (med, wins, calls) in alternating(fns).items():
        rec[k + "_ms"], rec[k + "_windows_ms"], rec[k + "_frames_per_window"] = round(med, 4), wins, calls
    for k, c in (("plain", cloud), ("rotated", rotated)):
        st = []
        for _ in range(5):
            timers = {}
            render_frame(rnd, c, cam, sc, 0, timers=timers)
            torch.cuda.synchronize()
            st.append(timers["_stage_events"][0].elapsed_ms())
        rec[k + "_chain_gather_ms"] = round(sorted(s["chain_gather"] for s in st)[2], 4)
        rec[k + "_chain_ms"] = round(sorted(s["chain"] for s in st)[2], 4)
    if parent:
        rec["plain_over_parent"] = round(rec["plain_ms"] / rec["plain_parent_ms"], 4)
    rec["rotated_over_plain"] = round(rec["rotated_ms"] / rec["plain_ms"], 4)
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None, help="libhnr_hip.so of the parent commit's build")
    ap.add_argument("--points", type=float, default=2.0e6)
    args = ap.parse_args()
    if args.child:
        import torch
        assert torch.cuda.is_available(), "edit_timing needs a GPU: there is no CPU fallback and no CPU timing"
        child(int(args.points), args.parent)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--points", str(args.points)] + (["--parent", os.path.abspath(args.parent)] if args.parent else [])
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S)
    except subprocess.TimeoutExpired:
        print("the timing run passed its time limit of %d s" % LIMIT_S)
        return 1
    got = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not got:
        print("the timing run failed (exit %d)\n%s\n%s" % (r.returncode, r.stdout[-1000:], r.stderr[-3000:]))
        return 1
    print(got[0], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/edit_timing.py on one MI355X: medians of five alternating one-second device-event windows, ms per frame; stage times: median of 5 frames\n")
            f.write(got[0][len("RESULT "):] + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
