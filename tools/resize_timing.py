"""Times the device resize (csrc/resize.hip) at the ScanNet shape: raw frames of 968 x 1296 x 3 bytes to the bank's 480 x 640, LANCZOS, one GPU.

  python tools/resize_timing.py [--out profiles/resize_timing.txt] [--frames 200]

  (a) kernel    hnr_resize_u8 alone, raw frames already on the device: one frame and a chunk of 16, form "fused" and form "two_pass"; the C entry
                is called directly with tables and scratch prepared, so a call is one ctypes call (one launch, or two).  A one-frame call is
                short enough that the host's issue rate may still bound it; the chunk of 16 is the figure free of that doubt
  (b) ingest    `--frames` raw frames from host memory into a resident bank: device = per chunk of 16 a host -> device copy of the raw frames
                and hnr_resize_u8 into the bank's rows (what FrameBank.from_raw does); host = the reference's way, PIL.Image.resize per frame on
                the host (one thread) and a host -> device copy of the small frames.  Decoding is excluded on both sides: both start from decoded
                arrays.  The two banks are compared byte for byte before anything is timed.
  (c) traffic   bytes the fused form has to move (raw frame read once + resized frame written once) per second, at the chunk of 16, beside a
                device-to-device copy of the same number of bytes in the same run

The parent opens no GPU: the measurement runs in a child process under its own time limit.  The child warms everything up, then times five
alternating windows per form, each about one second of back-to-back calls (sized from a timing of the warmed-up call; at least one call), with device events; a
window ends in an event synchronise, so host work -- all of Pillow's -- is paid for.  Reported: the median of the windows, per call.
Conditions (the exit status is 1 when one fails): device ingest not slower than host ingest; fused not slower than two_pass, at one frame AND at 16."""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

h, w, H, W, C, CHUNK = 968, 1296, 480, 640, 3, 16
LIMIT = 900                                                             # the child's time limit in seconds


def timed(fn, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def step_measure(n_frames):
    import numpy as np
    import torch
    from PIL import Image
    from hybridneuralrendering_amd import _lib, frames
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, size=(8, h, w, C), dtype=np.uint8)
    raw = np.ascontiguousarray(base[np.arange(n_frames) % 8])           # decoded frames in host memory; the content does not matter to either side
    d1, d16 = torch.from_numpy(raw[:1]).to(dev), torch.from_numpy(raw[:CHUNK]).to(dev)
    o1, o16 = (torch.empty((n, H, W, C), dtype=torch.uint8, device=dev) for n in (1, CHUNK))
    assert frames.resize_form((h, w), (W, H), C) == "fused"
    bank_dev = torch.empty((n_frames, H, W, C), dtype=torch.uint8, device=dev)
    bank_host = torch.empty_like(bank_dev)

    def ingest_device():
        for i in range(0, n_frames, CHUNK):
            frames.resize_frames(raw[i:i + CHUNK], (W, H), out=bank_dev[i:i + CHUNK])

    def ingest_host():
        small = np.stack([np.asarray(Image.fromarray(f).resize((W, H), Image.LANCZOS)) for f in raw])
        bank_host.copy_(torch.from_numpy(small))

    moved = CHUNK * (h * w * C + H * W * C)
    c_src, c_dst = (torch.empty((moved // 2,), dtype=torch.uint8, device=dev) for _ in range(2))
    # (a) calls the C entry itself with everything prepared (tables on the device, scratch allocated): no Python wrapper in the timed loop
    L, p = _lib.lib(), _lib.ptr
    kh, bh, ch = frames._device_tables(w, W, "lanczos", dev)
    kv, bv, cv = frames._device_tables(h, H, "lanczos", dev)
    scratch = torch.empty((int(L.hnr_resize_u8_scratch_bytes(CHUNK, h, w, C, H, W)),), dtype=torch.uint8, device=dev)
    st = _lib.stream()

    def kernel(src, dst, n, form):
        args = (p(src), n, h, w, C, p(dst), H, W, p(bh), p(ch), kh, p(bv), p(cv), kv, _lib.RESIZE_FORMS[form], p(scratch), int(scratch.numel()), st)
        return lambda: _lib.check(L.hnr_resize_u8(*args), "hnr_resize_u8")

    fns = (("fused1", kernel(d1, o1, 1, "fused")), ("two_pass1", kernel(d1, o1, 1, "two_pass")),
           ("fused16", kernel(d16, o16, CHUNK, "fused")), ("two_pass16", kernel(d16, o16, CHUNK, "two_pass")),
           ("copy16", lambda: c_dst.copy_(c_src)),
           ("ingest_device", ingest_device), ("ingest_host", ingest_host))
    ingest_device()
    ingest_host()
    torch.cuda.synchronize()
    assert torch.equal(bank_dev, bank_host), "the device bank and the Pillow bank differ"
    for name, fn in fns:
        for _ in range(1 if name.startswith("ingest") else 20):
            fn()
    torch.cuda.synchronize()
    # the windows' call counts, from a timing of the warmed-up call over enough calls to be in steady state
    calls = {n: max(1, int(math.ceil(1000.0 / max(timed(fn, 1 if n.startswith("ingest") else 2000), 1e-4)))) for n, fn in fns}
    win = {n: [] for n, _ in fns}
    for _ in range(5):
        for n, fn in fns:
            win[n].append(timed(fn, calls[n]))
    med = lambda v: sorted(v)[len(v) // 2]
    rec = dict(step="measure", what="%d x %d x %d uint8 -> %d x %d, lanczos; ingest of %d frames in chunks of %d; Pillow %s on one host thread"
               % (h, w, C, H, W, n_frames, CHUNK, Image.__version__))
    for n, _ in fns:
        rec[n + "_ms"] = round(med(win[n]), 4)
        rec[n + "_windows_ms"] = [round(v, 4) for v in win[n]]
        rec[n + "_calls_per_window"] = calls[n]
    rec["two_pass_over_fused_1"] = round(rec["two_pass1_ms"] / rec["fused1_ms"], 2)
    rec["two_pass_over_fused_16"] = round(rec["two_pass16_ms"] / rec["fused16_ms"], 2)
    rec["host_over_device_ingest"] = round(rec["ingest_host_ms"] / rec["ingest_device_ms"], 2)
    rec["ingest_device_ms_per_frame"] = round(rec["ingest_device_ms"] / n_frames, 4)
    rec["ingest_host_ms_per_frame"] = round(rec["ingest_host_ms"] / n_frames, 4)
    rec["fused16_moved_bytes"] = moved
    rec["fused16_GB_per_s"] = round(moved / rec["fused16_ms"] / 1e6, 1)
    rec["copy16_GB_per_s"] = round(moved / rec["copy16_ms"] / 1e6, 1)
    rec["fused_share_of_copy_rate"] = round(rec["fused16_GB_per_s"] / rec["copy16_GB_per_s"], 3)
    rec["window_seconds"] = {n: round(rec[n + "_ms"] * calls[n] / 1e3, 2) for n, _ in fns}
    rec["fused_not_slower_than_two_pass"] = bool(rec["fused1_ms"] <= rec["two_pass1_ms"] and rec["fused16_ms"] <= rec["two_pass16_ms"])
    rec["device_ingest_not_slower_than_host"] = bool(rec["ingest_device_ms"] <= rec["ingest_host_ms"])
    print("RESULT " + json.dumps(rec), flush=True)
    return 0 if rec["fused_not_slower_than_two_pass"] and rec["device_ingest_not_slower_than_host"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["measure"])
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "resize_timing needs a GPU: there is no CPU fallback"
        return step_measure(args.frames)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", "measure", "--frames", str(args.frames)], capture_output=True, text=True,
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
            f.write("# tools/resize_timing.py: raw 968 x 1296 x 3 frames to 480 x 640 (LANCZOS), medians of five alternating one-second device-event windows, ms per call\n")
            f.write("# fused / two_pass = hnr_resize_u8 alone on 1 and on 16 resident frames; ingest_device = upload of the raw frames + resize into the bank;\n")
            f.write("# ingest_host = PIL.Image.resize per frame on the host + upload of the small frames (decode excluded on both sides); copy16 = a device copy moving fused16's bytes\n")
            f.write(got[0][len("RESULT "):] + "\n")
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
