"""Times LPIPS on the device (hybridneuralrendering_amd/perceptual.py; csrc/lpips.hip) against the same stages written with stock torch ops on the same
GPU: the backbone as `conv2d` / `relu` / `max_pool2d` on a batch of two (tests/lpips_ref.py::features, the ops of torchvision's nn.Sequential), the tap
arithmetic as the package writes it (normalize_tensor, the squared difference, the 1x1 `lin` convolution, the spatial mean) and the preparation as
run/evaluate.py writes it (float32(img) / 255, * 2 - 1, BGR order, the ScalingLayer), without its PNG round trip.

  python tools/lpips_timing.py [--out profiles/lpips_timing.txt]
  rocprofv3 --kernel-trace -d DIR -- python tools/lpips_timing.py --step trace      (four vgg pairs of the HIP chain at 460x620)
  python tools/lpips_timing.py --blocks DIR                                          (TFLOP/s per VGG block from that trace)

The parent opens no GPU: it runs every step as a child process of its own under its own time limit and stops at the first step that fails.  Each
child warms both sides up, checks that they agree (and prints the difference), then times five alternating windows per side, each about one second
of back-to-back calls, with device events (tools/cloud_init_timing.py::windows), and reports the medians and the windows.

Workloads: 460x620 (the reference's test frames) and 800x800; weights from the tests' seeded rule (the arithmetic does not depend on them)."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cloud_init_timing import report, windows          # noqa: E402

SIZES = ((460, 620), (800, 800))
KINDS = ("prepare", "score_alex", "score_vgg", "trunk_alex", "trunk_vgg", "pair_alex", "pair_vgg")
STEPS = tuple(("%s_%dx%d" % (k, h, w), 300) for h, w in SIZES for k in KINDS)
VGG_BLOCKS = ((0, 1), (2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12))


def conv_gmac(net, h, w):
    """GMAC of every convolution for a PAIR of h x w images, in network order."""
    from tests import lpips_ref as LR
    pools, out = dict(LR.POOL_AFTER[net]), []
    for i, cin, cout, k, s, p in LR.CONVS[net]:
        h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        out.append(2 * cin * cout * k * k * h * w / 1e9)
        if i in pools:
            h, w = (h - pools[i]) // 2 + 1, (w - pools[i]) // 2 + 1
    return out


def setup(net, h, w, dev):
    import torch
    from hybridneuralrendering_amd.perceptual import LPIPS
    from tests import lpips_ref as LR
    p = LR.make_params(net, 7 if net == "alex" else 8)
    m = LPIPS(net).load_pretrained(LR.lpips_state_dict(net, p)).to(dev)
    a, b, _ = LR.seeded_images(h, w, 5)
    return m, {k: v.to(dev) for k, v in p.items()}, torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), LR


def run_step(step):
    import torch
    kind, size = step.rsplit("_", 1)
    h, w = (int(v) for v in size.split("x"))
    net = kind.split("_")[1] if "_" in kind else "alex"
    kind = kind.split("_")[0]
    dev = torch.device("cuda:0")
    m, p, a8, b8, LR = setup(net, h, w, dev)
    shift = torch.tensor(LR.SHIFT, device=dev).reshape(1, 3, 1, 1)
    scale = torch.tensor(LR.SCALE, device=dev).reshape(1, 3, 1, 1)
    extra, state = {}, {}

    def stock_prepare():
        ims = []
        for im in (a8, b8):
            x = im.flip(-1).float() / 255.0                       # cv2.imread: BGR; evaluate.py: float32(img) / 255.0
            x = (x * 2 - 1.0).permute(2, 0, 1)[None]
            ims.append((x - shift) / scale)
        return torch.cat(ims)

    def stock_score(taps):
        d, rs = LR.score(p, [f[0:1] for f in taps], [f[1:2] for f in taps])
        return torch.stack([d] + rs)

    with torch.no_grad():
        x = m.prepare8(a8, b8)
        taps = m.tap_features(x)
        if kind == "prepare":
            ours, theirs, what = lambda: m.prepare8(a8, b8), stock_prepare, "two %dx%d uint8 images -> the network's input [2,3,h,w]" % (h, w)
        elif kind == "score":
            ours, theirs = lambda: m.score(taps, h, w)[0], lambda: stock_score(taps)
            what = "%s: five taps of a %dx%d pair -> (d, r_0 .. r_4)" % (net, h, w)
        elif kind == "trunk":
            ours, theirs = lambda: tuple(m.tap_features(x)), lambda: tuple(LR.features(net, p, x))
            what = "%s trunk alone (convolutions, ReLUs, pools) on a %dx%d pair" % (net, h, w)
            extra["gmac"] = round(sum(conv_gmac(net, h, w)), 2)
        else:
            ours, theirs = lambda: m.pair8(a8, b8)[0], lambda: stock_score(LR.features(net, p, stock_prepare()))
            what = "%s: the whole chain, two %dx%d uint8 images -> (d, r_0 .. r_4)" % (net, h, w)

        def run_ours():
            state["ours"] = ours()

        def run_theirs():
            state["theirs"] = theirs()
        for _ in range(2):
            run_ours(); run_theirs()
        torch.cuda.synchronize()
        ra, rb = state["ours"], state["theirs"]
        ra, rb = (ra, rb) if isinstance(ra, tuple) else ((ra,), (rb,))
        diff = max(float((u.double() - v.double()).abs().max() / v.double().abs().max()) for u, v in zip(ra, rb))
        extra["max_rel_difference"] = diff
        print("device against torch on the GPU, %s: largest difference %.3e of the largest magnitude" % (step, diff), flush=True)
        assert diff <= (1e-6 if kind == "prepare" else 1e-4), "the device and torch on the GPU disagree: %g" % diff
        ma, mb, ta, tb, ca, cb = windows(run_ours, run_theirs, 5)
    if "gmac" in extra:
        extra.update(hip_tflops=round(2 * extra["gmac"] / ma, 2), torch_tflops=round(2 * extra["gmac"] / mb, 2))
    report(step, what, ma, mb, ta, tb, ca, cb, extra)


def blocks_from_trace(folder, h=460, w=620):
    """TFLOP/s of lpips_conv_kernel per VGG block from a rocprofv3 --kernel-trace of `--step trace` (dispatches in launch order: 13 per pair)."""
    rows = []
    for path in glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += [r for r in csv.DictReader(f) if "lpips_conv_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert rows and len(rows) % 13 == 0, "expected a multiple of 13 convolution dispatches, found %d" % len(rows)
    ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows]
    pairs = len(ms) // 13
    med = [sorted(ms[i + 13 * k] for k in range(pairs))[pairs // 2] for i in range(13)]
    gmac = conv_gmac("vgg", h, w)
    out = []
    for b, layers in enumerate(VGG_BLOCKS):
        g, t = sum(gmac[i] for i in layers), sum(med[i] for i in layers)
        out.append(dict(block=b + 1, layers=len(layers), gmac=round(g, 2), ms=round(t, 4), tflops=round(2 * g / t, 2)))
    wide = [i for i in range(13) if i >= 1]                                # the 3x3 layers with 64 or more input channels
    g, t = sum(gmac[i] for i in wide), sum(med[i] for i in wide)
    return dict(step="vgg_blocks_%dx%d" % (h, w), what="lpips_conv_kernel per VGG block from one kernel trace (median of %d pairs)" % pairs, blocks=out,
                layers_ms=[round(v, 4) for v in med], cin_ge_64_tflops=round(2 * g / t, 2), trunk_conv_ms=round(sum(med), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS] + ["trace"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", default=",".join(s for s, _ in STEPS), help="the steps the parent runs, comma-separated")
    ap.add_argument("--blocks", default=None, help="folder of a rocprofv3 --kernel-trace run of --step trace")
    args = ap.parse_args()
    if args.blocks:
        print("RESULT " + json.dumps(blocks_from_trace(args.blocks)))
        return 0
    if args.step:
        import torch
        assert torch.cuda.is_available(), "lpips_timing needs a GPU: there is no CPU fallback and no CPU timing"
        if args.step == "trace":
            m, _, a8, b8, _ = setup("vgg", 460, 620, torch.device("cuda:0"))
            for _ in range(4):
                m.pair8(a8, b8)
            torch.cuda.synchronize()
            return 0
        run_step(args.step)
        return 0
    lines = []
    for step, limit in STEPS:
        if step not in args.steps.split(","):
            continue
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print("step %s passed its time limit of %d s: stopping" % (step, limit))
            return 1
        got = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            print("step %s failed (exit %d): stopping\n%s\n%s" % (step, r.returncode, r.stdout[-1000:], r.stderr[-2000:]))
            return 1
        lines += got
        print(got[0], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/lpips_timing.py: medians of five alternating one-second device-event windows, HIP path vs the same stage in stock torch ops\n")
            f.write("\n".join(l[len("RESULT "):] for l in lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
