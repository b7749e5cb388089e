"""Generates tests/golden/frame_weights.npz and tests/golden/raft_param_keys.json by running the REFERENCE's RAFT (raft/core/raft.py, basic model, eval,
test_mode=True) and its `warp` (raft/demo_content_aware_weights.py) on small inputs, in fp32 on the CPU.  Needs the reference checkout; the fixture
holds data only, and none of the reference's code is copied.

`raft/core` goes first on sys.path (its `utils` package collides with the top-level one of the reference); `cv2` is a stand-in module for the import of
the demo script, whose `DEVICE` is set to 'cpu'.

Weights are NOT stored: they come from tests/raft_ref.py::make_params(seed), a rule driven by np.random.RandomState(seed) whose stream is frozen
(encoders N(0, 2/fan_out), as the reference initialises them; the update block N(0, 1/(3 fan_in)), the variance torch's default leaves it with: at
2/fan_out there too the three assertions below fail -- flows of 4400 px, fp32 and fp64 pixels apart).  The json records every tensor's shape and its
fp64 sum and abs-sum, so that drift of the rule shows.  Images come from raft_ref.make_images (16 grey levels,
image 2 = image 1 rolled by (2, -3) plus noise of -1 .. 1) and ARE stored.

Recorded per shape: flow_low at iters 1, 3 and 20; flow_up whole at iters 20 and, at iters 1 and 3, every 4th pixel each way plus its fp64 sum and
abs-sum (nine whole fp32 flow_up maps would be 1.6 MB: over the limit for a committed file); fp64 sum and abs-sum of the encoder outputs, the four
pyramid levels and of corr, net, delta_flow and mask of iterations 1 and 20; the picks of the reference's `warp(., flow_up, mode='nearest')` (an index
image is warped, so the output IS the pick).

Asserted here, with the seeded rule: after 20 iterations some |flow| >= 2 px; the fp32 and fp64 restatements' flows agree to 1e-4 px; a share of the
lookup taps falls outside the map.

Run:  python tests/golden/make_golden_frame_weights.py
"""
import argparse
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from _ref_import import REF                                    # noqa: E402
from tests import raft_ref as R                                # noqa: E402

SHAPES = ((128, 160), (136, 200), (136, 152))
ITERS = (1, 3, 20)


def stats(t):
    a = t.detach().double().numpy()
    return np.array([a.sum(), np.abs(a).sum()])


def import_reference_raft():
    sys.path.insert(0, os.path.join(REF, "raft", "core"))
    sys.path.insert(1, os.path.join(REF, "raft"))
    if "cv2" not in sys.modules:
        try:
            import cv2  # noqa: F401
        except Exception:
            sys.modules["cv2"] = types.ModuleType("cv2")
    raft_mod = importlib.import_module("raft")
    demo = importlib.import_module("demo_content_aware_weights")
    demo.DEVICE = "cpu"
    return raft_mod, demo


def main():
    raft_mod, demo = import_reference_raft()
    args = argparse.Namespace(small=False, mixed_precision=False, alternate_corr=False)
    model = raft_mod.RAFT(args).eval()
    sd = R.make_params()
    want = {k: v for k, v in model.state_dict().items() if not k.endswith("num_batches_tracked")}
    assert list(R.param_shapes()) and set(want) == set(sd), set(want) ^ set(sd)
    assert all(tuple(want[k].shape) == tuple(sd[k].shape) for k in sd)
    model.load_state_dict(sd, strict=False)

    rec = {}

    class Recorder(raft_mod.CorrBlock):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            rec["levels"] = [c for c in self.corr_pyramid]
            rec["corr"] = []

        def __call__(self, coords):
            out = super().__call__(coords)
            rec["corr"].append(out)
            return out

    raft_mod.CorrBlock = Recorder
    model.fnet.register_forward_hook(lambda m, i, o: rec.__setitem__("fmaps", o))
    model.cnet.register_forward_hook(lambda m, i, o: rec.__setitem__("cnet", o))
    model.update_block.register_forward_hook(lambda m, i, o: rec.setdefault("upd", []).append(o))

    out = {"shapes": np.array(SHAPES), "iters": np.array(ITERS), "seed": np.array(R.SEED)}
    for si, (H, W) in enumerate(SHAPES):
        im1, im2 = R.make_images((H, W))
        p = "s%d." % si
        out[p + "image1"], out[p + "image2"] = im1, im2
        t1, t2 = torch.from_numpy(im1).float()[None], torch.from_numpy(im2).float()[None]
        for iters in ITERS:
            rec.pop("upd", None)
            with torch.no_grad():
                low, up = model(t1, t2, iters=iters, test_mode=True)
            q = p + "it%d." % iters
            out[q + "flow_low"] = low[0].numpy()
            if iters == 20:
                out[q + "flow_up"] = up[0].numpy()
            else:
                out[q + "flow_up_sub"] = up[0, :, ::4, ::4].numpy().copy()
                out[q + "flow_up_stats"] = stats(up)
        # the last run was iters = 20: its intermediates
        out[p + "stat.fmap1"], out[p + "stat.fmap2"], out[p + "stat.cnet"] = stats(rec["fmaps"][0]), stats(rec["fmaps"][1]), stats(rec["cnet"])
        for l in range(4):
            out[p + "stat.level%d" % l] = stats(rec["levels"][l])
        for it in (1, 20):
            net, mask, delta = rec["upd"][it - 1]
            for name, t in (("corr", rec["corr"][it - 1]), ("net", net), ("delta", delta), ("mask", mask)):
                out[p + "stat.it%d.%s" % (it, name)] = stats(t)
        # the reference's warp on an index image: 1 + pixel index, 0 outside
        idx = torch.arange(1, H * W + 1, dtype=torch.float32).reshape(1, 1, H, W)
        picked = demo.warp(idx, up, mode="nearest")[0, 0].numpy()
        assert (picked == np.rint(picked)).all()
        out[p + "it20.warp_pick"] = (picked.astype(np.int64) - 1).astype(np.int32)

        # the three conditions, with the restatement
        r32 = R.forward(sd, im1, im2, 20, torch.float32, keep=(19,))
        r64 = R.forward(sd, im1, im2, 20, torch.float64, keep=(19,))
        mag = float(r64["flow_up"].abs().max())
        d_low = float((r32["flow_low"].double() - r64["flow_low"]).abs().max())
        d_up = float((r32["flow_up"].double() - r64["flow_up"]).abs().max())
        h, w = H // 8, W // 8
        c = r64["steps"][19]["coords_in"]
        hl, wl = h // 8, w // 8
        x = c[0][..., None] / 8 + torch.arange(-4, 5)
        y = c[1][..., None] / 8 + torch.arange(-4, 5)
        outside = float(((x < 0) | (x > wl - 1)).double().mean()), float(((y < 0) | (y > hl - 1)).double().mean())
        print("shape %d (%d, %d): max |flow_up| %.2f px, fp32 vs fp64 flow_low %.2e flow_up %.2e px, level-3 taps outside x %.2f y %.2f; reference vs "
              "fp32 restatement flow_up %.2e" % (si, H, W, mag, d_low, d_up, outside[0], outside[1], float((r32["flow_up"] - up[0]).abs().max())))
        assert mag >= 2.0, mag
        assert d_low <= 1e-4 and d_up <= 1e-4, (d_low, d_up)
        assert min(outside) > 0.05, outside

    path = os.path.join(HERE, "frame_weights.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 1000000, size
    with open(os.path.join(HERE, "raft_param_keys.json"), "w") as f:
        json.dump({k: dict(shape=list(v.shape), sum=float(v.double().sum()), abs_sum=float(v.double().abs().sum())) for k, v in sd.items()}, f, indent=1,
                  sort_keys=True)
        f.write("\n")
    print("wrote %s (%d bytes) and raft_param_keys.json (%d keys)" % (path, size, len(sd)))


if __name__ == "__main__":
    main()
