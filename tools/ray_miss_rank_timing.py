"""Times the growth schedule's per-step bookkeeping -- the step's ray-miss loss and the table of the worst frames -- at the C3 shape: R = 56 x 56 = 3136
rays, a table of n = 11 frames (train_len 40, prob_num_step 4), one GPU.

  python tools/ray_miss_rank_timing.py [--out profiles/ray_miss_rank_timing.txt]

Two forms of the same update on the same device tensors:
  (a) hip    growth.RayMissRanking.update: one launch (csrc/rank.hip), the frame number read on the device, nothing read back
  (b) torch  stock torch ops written after the reference's lines (models/base_rendering_model.py:1153-1159, models/mvs_points_volumetric_model.py:162-172):
             masked_select twice, `if masked_output.shape[1] > 0`, MSELoss * the number of missed rays, `if torch.sum(mask) > 0`, a Python max() on
             device scalars, torch.sort -- its two host reads included (the size of the masked copy and the `if` on the mask sum; the max() is a third)

The parent opens no GPU: the measurement runs in a child process under its own time limit.  The child warms both forms up, then times five alternating
windows per form of back-to-back calls with device events, each sized for one second from a first timed run of three calls (which overestimates a
call: the recorded windows hold 14 672 and 2 409 calls, 0.24 s and 0.59 s); a window ends in an event synchronise, so host work between launches is
paid for.  Both forms also pay the device-to-device copy that stands in for the sampler's frame_row.  Reported: the median of the windows and their
range, per call."""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

R, TRAIN_LEN, NUM_STEP = 3136, 40, 4
LIMIT = 300                                                             # the child's time limit in seconds


def step_update():
    import numpy as np
    import torch
    from hybridneuralrendering_amd.growth import RayMissRanking
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    gt = t(rng.random((R, 3)).astype(np.float32))
    mask_np = (rng.random(R) > 0.2).astype(np.int8)
    col_np = rng.random((R, 3)).astype(np.float32)
    col_np[mask_np == 0] = 1.0
    out = dict(coarse_raycolor=t(col_np), ray_mask=t(mask_np))
    rows = t(rng.integers(0, TRAIN_LEN, size=4096).astype(np.int32))
    row = torch.zeros((1,), dtype=torch.int32, device=dev)
    rank = RayMissRanking(TRAIN_LEN, NUM_STEP, dev)
    state = dict(i=0, j=0)

    def hip():
        row.copy_(rows[state["i"] % 4096:state["i"] % 4096 + 1]); state["i"] += 1     # (the sampler's frame_row: a device-to-device copy, no host read)
        rank.update(out, gt, row)

    l2 = torch.nn.MSELoss()
    n = TRAIN_LEN // NUM_STEP + 1
    tab = dict(ids=torch.arange(n, dtype=torch.int32, device=dev), losses=torch.zeros(n, dtype=torch.float32, device=dev))
    color3, gt3, mask2 = out["coarse_raycolor"][None], gt[None], out["ray_mask"][None]

    def stock():
        row.copy_(rows[state["j"] % 4096:state["j"] % 4096 + 1]); state["j"] += 1
        miss = (mask2 == 0)[..., None].expand(-1, -1, 3)
        mo = torch.masked_select(color3, miss).reshape(1, -1, 3)
        mg = torch.masked_select(gt3, miss).reshape(1, -1, 3)
        if mo.shape[1] > 0:
            loss = l2(mo, mg) * mg.shape[1]
        else:
            loss = torch.tensor(0.0, dtype=torch.float32, device=dev)
        inds, losses = tab["ids"], tab["losses"]
        m = (inds - row[0]) == 0
        if torch.sum(m) > 0:
            losses[m] = max(loss, losses[m])
        else:
            inds[-1] = row[0]
            losses[-1] = loss
        losses, indices = torch.sort(losses, descending=True)
        tab["ids"], tab["losses"] = inds[indices], losses

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / calls
    fns = (("hip", hip), ("torch", stock))
    for _, fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    # both forms saw the same three frames and the same batch: the same losses, the same frames with a positive one (equal losses: the order is open)
    assert torch.allclose(rank.losses, tab["losses"], rtol=1e-5, atol=0), (rank.losses.tolist(), tab["losses"].tolist())
    assert sorted(rank.ids[rank.losses > 0].tolist()) == sorted(tab["ids"][tab["losses"] > 0].tolist())
    calls = {n_: max(1, int(math.ceil(1000.0 / max(timed(fn, 3), 1e-3)))) for n_, fn in fns}
    win = {n_: [] for n_, _ in fns}
    for _ in range(5):
        for n_, fn in fns:
            win[n_].append(timed(fn, calls[n_]))
    med = lambda v: sorted(v)[len(v) // 2]
    rec = dict(step="update", what="R = %d rays, table of %d frames" % (R, n))
    for n_, _ in fns:
        rec[n_ + "_ms"] = round(med(win[n_]), 5)
        rec[n_ + "_windows_ms"] = [round(v, 5) for v in win[n_]]
        rec[n_ + "_calls_per_window"] = calls[n_]
    rec["torch_over_hip"] = round(rec["torch_ms"] / rec["hip_ms"], 2)
    rec["hip_beats_torch_by_more_than_the_spread"] = bool(max(win["hip"]) < min(win["torch"]))
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["update"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "ray_miss_rank_timing needs a GPU: there is no CPU fallback"
        step_update()
        return 0
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", "update"], capture_output=True, text=True, timeout=LIMIT)
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
            f.write("# tools/ray_miss_rank_timing.py: the per-step ray-miss ranking at the C3 shape, medians of five alternating one-second device-event windows, ms per call\n")
            f.write("# (a) hip = RayMissRanking.update (one launch, no host read), (b) torch = the reference's lines in stock torch ops, two host reads included\n")
            f.write(got[0][len("RESULT "):] + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
