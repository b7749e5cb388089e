"""Generates tests/golden/mvs_depth.npz and tests/golden/mvs_depth_param_keys.json by running the REFERENCE's pretrained-depth path of the
`load_points=0`, `manual_depth_view=1` start of a scene (run/train_ft.py:104-190) on small random inputs, in fp32 on the CPU.  Needs the reference
checkout (tests/golden/_ref_import.py, through make_golden_cloud_init.import_reference_modules); the fixture holds data only.

Reference code that runs (none is copied):
  models/depth_estimators/mvsnet.py   MVSNet(refine=False).eval(): the module, its names and its forward (module.py: homo_warping, depth_regression)
  models/mvs/mvs_points_model.py      MvsPointsModel.depth2point as an unbound method (-> mvs_utils.ndc_2_cam), fed what gau_single_sampler hands it for
                                      manual_std_depth = 0: `sample_by_gau` draws its noise on "cuda" and cannot run here; at std 0 it is
                                      clamp(ndc_depth, 0, 1), stated below and in tests/mvs_depth_ref.py

Weights and norm statistics are random, not identities: running mean +-0.2, variance and norm weight 0.5 - 1.5, bias +-0.2; convolution weights are
small integers times a power of two (so that 340 k of them compress: every value is an exact fp32 number either way); `prob.weight` is scaled x30 so
that the softmax is not flat (unscaled, the expected index sits within 0.05 of (D-1)/2 everywhere).  Images are multiples of 1/15, stored as uint8.
Cameras: one pinhole shared by the views, small rotations and translations, so that q.z > 0 everywhere and part of every source view falls outside
the frame (asserted).

Run:  python tests/golden/make_golden_mvs_depth.py
"""
import importlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden_cloud_init import import_reference_modules       # noqa: E402
from tests import mvs_depth_ref as R                              # noqa: E402

SHAPES = ((3, 8, 32, 32), (3, 16, 64, 96), (2, 8, 32, 64), (5, 24, 96, 64))         # (V, D, H, W)
POINT_SHAPES = (0, 2)                                                               # depth2point is recorded for these
IMAGE_LEVELS = 15
DEPTH_MIN, DEPTH_MAX = 2.0, 4.0


def randomise(net, g):
    u = lambda shape, lo, hi: lo + (hi - lo) * torch.rand(shape, generator=g)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if p.dim() >= 4:
                fan_in = p[:, 0].numel() if name.endswith(".0.weight") else p[0].numel()            # (ConvTranspose3d: [cin][cout][k][k][k])
                step = 2.0 ** np.round(np.log2(1.0 / np.sqrt(fan_in) / 9.0))        # integers -15 .. 15: standard deviation about 9 steps
                p.copy_(torch.randint(-15, 16, p.shape, generator=g).float() * step)
            elif name.endswith("weight"):
                p.copy_(u(p.shape, 0.5, 1.5))
            else:
                p.copy_(u(p.shape, -0.2, 0.2))
        for name, b in net.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(u(b.shape, -0.2, 0.2))
            elif name.endswith("running_var"):
                b.copy_(u(b.shape, 0.5, 1.5))
        net.cost_regularization.prob.weight.mul_(30.0)


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def cameras(V, h, w, rng):
    """proj [V,4,4]: view v seen from view 0, K E_v E_0^-1 K^-1 with E_0 = identity (proj[0] is the identity), K the pinhole of the h x w feature map."""
    K = np.array([[1.1 * w, 0, 0.5 * w, 0], [0, 1.1 * w, 0.5 * h, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)
    proj = [np.eye(4)]
    for v in range(1, V):
        E = np.eye(4)
        E[:3, :3] = rot(*rng.uniform(-0.05, 0.05, 3))
        E[:3, 3] = rng.uniform(0.15, 0.35, 3) * rng.choice([-1.0, 1.0], 3) * [1.0, 1.0, 0.3]
        proj.append(K @ E @ np.linalg.inv(K))
    return np.stack(proj).astype(np.float32), K[:3, :3].astype(np.float32)


def main():
    mu, ds, pm = import_reference_modules()
    mvsnet = importlib.import_module("models.depth_estimators.mvsnet")
    g = torch.Generator().manual_seed(47)
    rng = np.random.default_rng(47)
    net = mvsnet.MVSNet(refine=False).eval()
    randomise(net, g)
    sd = {k: v.clone() for k, v in net.state_dict().items() if not k.endswith("num_batches_tracked")}
    out = {"sd." + k: v.numpy() for k, v in sd.items()}
    out["shapes"] = np.array(SHAPES)
    for i, (V, D, H, W) in enumerate(SHAPES):
        h, w = H // 4, W // 4
        img8 = torch.randint(0, IMAGE_LEVELS + 1, (V, 3, H, W), generator=g).to(torch.uint8)
        imgs = img8.float() / IMAGE_LEVELS
        proj, K = cameras(V, h, w, rng)
        depth_values = (DEPTH_MIN + torch.arange(0, D, dtype=torch.float32) * ((DEPTH_MAX - DEPTH_MIN) / D))
        with torch.no_grad():
            depth, conf, feats, prob = net(imgs[None], torch.from_numpy(proj)[None], depth_values[None])
        feats = torch.cat(feats, dim=0)
        assert tuple(depth.shape) == (1, h, w) and tuple(prob.shape) == (1, D, h, w) and tuple(feats.shape) == (V, 32, h, w)
        # the cameras: q.z > 0 everywhere, and part of every source view outside the frame
        ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        pix = np.stack([xs.ravel(), ys.ravel(), np.ones(h * w)])
        for v in range(1, V):
            q = (proj[v, :3, :3].astype(np.float64) @ pix)[:, None, :] * depth_values.numpy()[None, :, None] + proj[v, :3, 3].astype(np.float64)[:, None, None]
            assert (q[2] > 0.5).all()
            px, py = q[0] / q[2], q[1] / q[2]
            outside = (px < 0) | (px > w - 1) | (py < 0) | (py > h - 1)
            assert 0.02 < outside.mean() < 0.9, (i, v, outside.mean())
        fidx = R.depth_head(R.cost_reg(sd, R.cost_volume(feats, proj, depth_values)), depth_values)[3].numpy()
        print("shape %d %s: expected index %.2f .. %.2f, depth %.3f .. %.3f, confidence %.3f .. %.3f" % (
            i, (V, D, H, W), fidx.min(), fidx.max(), float(depth.min()), float(depth.max()), float(conf.min()), float(conf.max())))
        p = "s%d." % i
        out.update({p + "images_u8": img8.numpy(), p + "proj": proj, p + "K": K, p + "depth_values": depth_values.numpy(), p + "depth": depth[0].numpy(),
                    p + "confidence": conf[0].numpy(), p + "prob": prob[0].numpy(), p + "features": feats.numpy()})
        if i in POINT_SHAPES:
            # the tail of gen_points (mvs_points_model.py:329-337) and gau_single_sampler's else branch, manual_std_depth = 0
            Kimg = torch.tensor([[1.1 * W, 0, 0.5 * W], [0, 1.1 * W, 0.5 * H], [0, 0, 1]], dtype=torch.float32)
            lo, hi = float(depth.min()), float(depth.max())
            near_far = torch.tensor([lo + 0.3 * (hi - lo), lo + 0.8 * (hi - lo)], dtype=torch.float32)              # the mask cuts through the map
            d_up = torch.nn.functional.interpolate(depth[:, None], size=[H, W], mode="nearest")
            c_up = torch.nn.functional.interpolate(conf[:, None], size=[H, W], mode="nearest")
            mask = torch.logical_and(d_up >= near_far[0], d_up <= near_far[1])
            ndc = (d_up - near_far[0]) / (near_far[1] - near_far[0])
            sampled = torch.clamp(ndc[:, None], min=0.0, max=1.0)                                                    # sample_by_gau at std 0
            _, cam_xyz = pm.MvsPointsModel.depth2point(None, sampled, Kimg[None], near_far)
            assert tuple(cam_xyz.shape) == (1, 1, 1, H, W, 3) and 0.05 < mask.float().mean() < 0.95
            out.update({p + "pts_K": Kimg.numpy(), p + "pts_near_far": near_far.numpy(), p + "pts_cam_xyz": cam_xyz[0, 0, 0].numpy(),
                        p + "pts_confidence": c_up[0, 0].numpy(), p + "pts_mask": mask[0, 0].numpy()})
    path = os.path.join(HERE, "mvs_depth.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 1000000, size
    with open(os.path.join(HERE, "mvs_depth_param_keys.json"), "w") as f:
        json.dump({k: list(v.shape) for k, v in sd.items()}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s (%d bytes) and mvs_depth_param_keys.json (%d keys)" % (path, size, len(sd)))


if __name__ == "__main__":
    main()
