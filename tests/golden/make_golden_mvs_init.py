"""Generates tests/golden/mvs_init.npz and tests/golden/mvs_init_param_keys.json by running the REFERENCE's own networks of the `load_points=2` point
initialisation (run/train_ft.py:751-765) on small random inputs, in fp64 and in fp32 on the CPU.  Needs the reference checkout
(tests/golden/_ref_import.py, through make_golden_cloud_init.import_reference_modules); the fixture holds data only.

Reference code that runs (none is copied):
  models/mvs/models.py            FeatureNet(intermediate=True, norm_act=AbnStandIn): the module, its names and its forward
  models/mvs/mvs_points_model.py  premlp_init(opt); MvsPointsModel.query_embedding / extract_2d with a stand-in `self` (shading_feature_mlp_layer0 = 1,
                                  "imgfeat_0_0123 dir_0 point_conf"), called as run/train_ft.py:759-760 calls it (pointdir_w=True)
  models/mvs/mvs_utils.py         homo_warp_nongrid, extract_from_2d_grid (its stray .cuda() neutralised)

Two stand-ins, both stated here because nothing on this side can pin them:
  * AbnStandIn takes the place of inplace_abn.InPlaceABN, a CUDA extension that is not installed.  Its forward is that package's documented inference
    arithmetic: y = leaky_relu((x - running_mean) * mul + bias, 0.01), mul = rsqrt(running_var + eps) * (|weight| + eps), eps = 1e-5.
  * homo_warp_nongrid casts its pixel grid to float32 whatever the input precision; F.grid_sample then refuses an fp64 feature map.  For the fp64 run
    only, `.to(torch.float32)` of an fp64 tensor is made the identity, so the whole chain stays fp64.

All weights and running statistics are random (negative bn.weight values included: the |weight| matters).  The share of points within EPS_PIX of the
frame border -- where fp32 and fp64 may disagree about the mask -- is asserted to be at most 1 %: the GPU test leaves exactly those out.

Run:  python tests/golden/make_golden_mvs_init.py
"""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden_cloud_init import import_reference_modules, look_at       # noqa: E402

V, H, W = 2, 37, 53
EPS_PIX = 1e-3
FEATURE_STR = ["imgfeat_0_0123", "dir_0", "point_conf"]


class AbnStandIn(nn.Module):
    def __init__(self, channels, eps=1e-5, slope=0.01):
        super().__init__()
        self.weight, self.bias = nn.Parameter(torch.ones(channels)), nn.Parameter(torch.zeros(channels))
        self.register_buffer("running_mean", torch.zeros(channels))
        self.register_buffer("running_var", torch.ones(channels))
        self.eps, self.slope = eps, slope

    def forward(self, x):
        mul = torch.rsqrt(self.running_var + self.eps) * (self.weight.abs() + self.eps)
        c = lambda v: v.view(1, -1, 1, 1)
        return nn.functional.leaky_relu((x - c(self.running_mean)) * c(mul) + c(self.bias), self.slope)


def randomise(net, premlp, g):
    r = lambda shape, s=1.0: torch.randn(shape, generator=g) * s
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("conv.weight") or name == "toplayer.weight":
                p.copy_(r(p.shape, 1.4 / np.sqrt(p[0].numel())))
            elif name.endswith("bn.weight"):
                p.copy_((0.5 + torch.rand(p.shape, generator=g)) * torch.where(torch.rand(p.shape, generator=g) < 0.4, -1.0, 1.0))
            else:
                p.copy_(r(p.shape, 0.3))
        for name, b in net.named_buffers():
            b.copy_(r(b.shape, 0.3) if name.endswith("running_mean") else 0.5 + 1.5 * torch.rand(b.shape, generator=g))
        for name, p in premlp.named_parameters():
            if name.endswith("bias"):
                p.copy_(r(p.shape, 0.2))
    assert any((p < 0).any() for n, p in net.named_parameters() if n.endswith("bn.weight"))


def main():
    mu, ds, pm = import_reference_modules()
    models = importlib.import_module("models.mvs.models")
    torch.Tensor.cuda = lambda self, *a, **k: self             # extract_from_2d_grid's stray .cuda()
    g = torch.Generator().manual_seed(31)
    rng = np.random.default_rng(31)
    net = models.FeatureNet(intermediate=True, norm_act=AbnStandIn).eval()
    opt = types.SimpleNamespace(point_features_dim=32, act_type="LeakyReLU", shading_feature_mlp_layer1=2)
    premlp = pm.premlp_init(opt).eval()
    randomise(net, premlp, g)
    sd = {"FeatureNet." + k: v.clone() for k, v in net.state_dict().items()}
    sd.update({"premlp." + k: v.clone() for k, v in premlp.state_dict().items()})
    out = {"sd." + k: v.numpy() for k, v in sd.items()}

    images = torch.rand((V, 3, H, W), generator=g, dtype=torch.float64)
    out["images"] = images.numpy()
    with torch.no_grad():
        net.double()
        f64 = net(images[None])
        net.float()
        f32 = net(images[None].float())
        net.double(); premlp.double()
    assert [tuple(t.shape) for t in f64] == [(V, 3, H, W), (V, 8, H, W), (V, 16, 19, 27), (V, 32, 10, 14)]
    errs = []
    for lvl in (1, 2, 3):
        out["x%d" % lvl] = f64[lvl].numpy()
        errs.append(float((f32[lvl].double() - f64[lvl]).abs().max() / f64[lvl].abs().max()))
    out["torch_fp32_rel_err"] = np.array(errs)
    print("pyramid: torch fp32 vs fp64, max|a-b|/max|b| per level:", ["%.2e" % e for e in errs])

    # ---- one view (image 0) and its points: inside the frame, outside it, behind the camera
    K = np.array([[40.0, 0.0, 26.0], [0.0, 41.0, 18.0], [0.0, 0.0, 1.0]])
    c2w = look_at([0.3, -1.5, 1.1], [0.4, 1.0, 0.9]).astype(np.float64)
    w2c = np.linalg.inv(c2w)
    mk = lambda n, sx, sy, sign: np.stack([rng.uniform(-sx, sx, n), rng.uniform(-sy, sy, n), np.ones(n)], -1) * (sign * rng.uniform(0.5, 4.0, size=(n, 1)))
    cam_pts = np.concatenate([mk(300, 0.62, 0.42, 1.0), mk(80, 2.0, 1.5, 1.0), mk(40, 0.62, 0.42, -1.0)])
    world = cam_pts @ c2w[:3, :3].T + c2w[:3, 3]
    world = world.astype(np.float32).astype(np.float64)                    # the GPU sees fp32 points: fp64 truth on the same values
    c2w, w2c, K = (a.astype(np.float32).astype(np.float64) for a in (c2w, w2c, K))
    tw, tc, tK = torch.from_numpy(world), torch.from_numpy(c2w), torch.from_numpy(K)
    tw2c = torch.from_numpy(w2c)
    cam_xyz = (torch.cat([tw, torch.ones_like(tw[..., -1:])], dim=-1) @ tw2c.transpose(0, 1))[..., :3]                    # run/train_ft.py:759
    me = types.SimpleNamespace(args=types.SimpleNamespace(appr_feature_str0=FEATURE_STR, depth_occ=0, shading_feature_mlp_layer0=1, ref_vid=0), premlp=premlp)
    me.extract_2d = types.MethodType(pm.MvsPointsModel.extract_2d, me)
    feats = [t[:1] for t in f64]
    orig_to = torch.Tensor.to
    torch.Tensor.to = lambda self, *a, **k: self if (a and a[0] is torch.float32 and self.dtype == torch.float64) else orig_to(self, *a, **k)
    try:
        with torch.no_grad():
            emb, col, pdir, conf = pm.MvsPointsModel.query_embedding(me, [H, W], cam_xyz[None], None, feats, tc[None, None], tw2c[None, None], tK[None, None], 0,
                                                                     pointdir_w=True)
    finally:
        torch.Tensor.to = orig_to
    assert emb.dtype == torch.float64 and tuple(emb.shape) == (1, world.shape[0], 32) and tuple(conf.shape) == (1, world.shape[0], 1)
    grid = ((cam_xyz / cam_xyz[:, 2:3]) @ tK.t())[:, :2].numpy()
    mask = (grid[:, 0] >= 0) & (grid[:, 0] <= W - 1) & (grid[:, 1] >= 0) & (grid[:, 1] <= H - 1)
    near = (np.abs(grid[:, 0]) < EPS_PIX) | (np.abs(grid[:, 0] - (W - 1)) < EPS_PIX) | (np.abs(grid[:, 1]) < EPS_PIX) | (np.abs(grid[:, 1] - (H - 1)) < EPS_PIX)
    share = float(near.mean())
    assert share <= 0.01, share
    assert 250 <= mask.sum() < world.shape[0] and (col[0].numpy()[~mask] == 0).all() and (conf == 1).all()
    out.update(q_xyz=world.astype(np.float32), q_c2w=c2w.astype(np.float32), q_w2c=w2c.astype(np.float32), q_K=K.astype(np.float32), q_mask=mask,
               q_emb=emb[0].numpy(), q_color=col[0].numpy(), q_dir=pdir[0].numpy(), q_conf=conf[0].numpy(), q_near_border_share=np.array([share]))
    print("query_embedding: %d points, %d inside the frame, %.2f %% within %g px of the border" % (world.shape[0], int(mask.sum()), 100 * share, EPS_PIX))

    path = os.path.join(HERE, "mvs_init.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 1000000, size
    with open(os.path.join(HERE, "mvs_init_param_keys.json"), "w") as f:
        json.dump({k: list(v.shape) for k, v in sd.items()}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s (%d bytes) and mvs_init_param_keys.json (%d keys)" % (path, size, len(sd)))


if __name__ == "__main__":
    main()
