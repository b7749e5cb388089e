"""Point embeddings from the MVS init checkpoint, on the device (csrc/featnet.hip).

The reference starts a `load_points=2` scene from LEARNED point embeddings (run/train_ft.py:751-765): the image of the view a point was given to goes
through `FeatureNet(intermediate=True)` (models/mvs/models.py:717-764, built from InPlaceABN, a CUDA extension), the four pyramid levels are sampled at
the point's projection and `[56 features | colour 3 | dir 3 | conf 1]` goes through `premlp` (models/mvs/mvs_points_model.py:22-34, :225-259).  Both
networks come from the published init checkpoint (`*_net_mvs.pth`).  `MvsInit` carries the reference's parameter names, so that file loads as it is,
and runs both networks as HIP kernels: `hnr_featnet_forward` and `hnr_point_embed`.  Inference only (no backward, results carry no graph), GPU only
(no CPU or torch fallback: `HnrError`).

The weights a fresh module starts from are torch's defaults, not the reference's `init_seq`: the module exists to load a checkpoint.
"""
import torch
from torch import nn

from . import _lib
from ._lib import HnrError
from ._nets import NormParams, Packed, PackedWeights, filtered_state_dict, host_f32, load_checked

EPS = 1e-5                                                       # InPlaceABN's eps (variance and |weight|)
SLOPE = 0.01                                                     # its activation_param, and premlp's LeakyReLU
LAYERS = (("conv0", ((3, 8, 3, 1), (8, 8, 3, 1))), ("conv1", ((8, 16, 5, 2), (16, 16, 3, 1), (16, 16, 3, 1))),
          ("conv2", ((16, 32, 5, 2), (32, 32, 3, 1), (32, 32, 3, 1))))             # (cin, cout, kernel, stride); pad = kernel // 2
FEATURE_STR = ["imgfeat_0_0123", "dir_0", "point_conf"]


def pyramid_shape(H, W):
    """((H, W), (H2, W2), (H4, W4)) of x1, x2, x3."""
    H2, W2 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return (H, W), (H2, W2), ((H2 - 1) // 2 + 1, (W2 - 1) // 2 + 1)


class _ConvBnReLU(nn.Module):
    def __init__(self, cin, cout, ks, stride):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, ks, stride=stride, padding=ks // 2, bias=False)
        self.bn = NormParams(cout)                                # InPlaceABN's names; its arithmetic: pack_host and the kernel's epilogue


def featnet_forward(images, packed):
    """hnr_featnet_forward: images [V,3,H,W], packed [FEATNET_PACKED_ELEMS] -> (x1 [V,8,H,W], x2 [V,16,H2,W2], x3 [V,32,H4,W4])."""
    images, packed = _lib.require_gpu(images, "images", torch.float32), _lib.require_gpu(packed, "packed", torch.float32)
    if images.dim() != 4 or images.shape[1] != 3:
        raise HnrError("featnet_forward: images must be [V,3,H,W], got %s" % (tuple(images.shape),))
    if packed.numel() != _lib.FEATNET_PACKED_ELEMS or packed.device != images.device:
        raise HnrError("featnet_forward: packed must hold %d values on the images' device" % _lib.FEATNET_PACKED_ELEMS)
    V, _, H, W = (int(s) for s in images.shape)
    dev = images.device
    scratch = _lib.scratch("hnr_featnet_scratch_elems", V, H, W, device=dev, dtype=torch.float32,
                           what="featnet_forward: unsupported shape V=%d H=%d W=%d (1 <= V <= 4096, 4 <= H, W <= 32768)" % (V, H, W))
    outs = [torch.empty((V, c, h, w), dtype=torch.float32, device=dev) for c, (h, w) in zip((8, 16, 32), pyramid_shape(H, W))]
    _lib.call("hnr_featnet_forward", images, V, H, W, packed, outs[0], outs[1], outs[2], scratch, scratch.numel(), _lib.STREAM)
    return tuple(outs)


def point_embed(xyz, w2c, c2w, cpc, intrinsic, image, x1, x2, x3, premlp, want_row=False, conf=None, visible=None):
    """hnr_point_embed for one view: (emb [n,32], color [n,3], dir [n,3], row [n,63] or None).  image [3,H,W]; x1 / x2 / x3 its pyramid, channels first.
    conf [n] (optional): the photometric confidence premlp sees in the row's last column (hnr_point_embed_conf); None: ones.
    visible [n] uint8 (optional, cloud_init.point_occlusion's flags, hnr_point_embed_vis): where it is 0 the point counts as outside the frame."""
    from .cloud_init import _cf, _host_f32
    xyz = _lib.require_gpu(xyz, "xyz", torch.float32).reshape(-1, 3)
    image = _lib.require_gpu(image, "image", torch.float32)
    if image.dim() != 3 or image.shape[0] != 3:
        raise HnrError("point_embed: image must be [3,H,W]")
    H, W = int(image.shape[1]), int(image.shape[2])
    maps = [_lib.require_gpu(m, name, torch.float32) for m, name in ((x1, "x1"), (x2, "x2"), (x3, "x3"))]
    for m, c, hw in zip(maps, (8, 16, 32), pyramid_shape(H, W)):
        if tuple(m.shape) != (c,) + hw:
            raise HnrError("point_embed: a pyramid level must be %s for a %dx%d image, got %s" % ((c,) + hw, H, W, tuple(m.shape)))
    premlp = _lib.require_gpu(premlp, "premlp", torch.float32)
    if premlp.numel() != _lib.PREMLP_PACKED_ELEMS:
        raise HnrError("point_embed: premlp must hold %d values" % _lib.PREMLP_PACKED_ELEMS)
    n, dev = int(xyz.shape[0]), xyz.device
    if any(t.device != dev for t in [image, premlp] + maps):
        raise HnrError("point_embed: every tensor must be on xyz's device")
    if conf is not None:
        conf = _lib.require_gpu(conf, "conf", torch.float32).reshape(-1)
        if conf.shape[0] != n or conf.device != dev:
            raise HnrError("point_embed: conf must hold one value per point, on xyz's device")
    if visible is not None:
        visible = _lib.require_gpu(visible, "visible", torch.uint8).reshape(-1)
        if visible.shape[0] != n or visible.device != dev:
            raise HnrError("point_embed: visible must hold one flag per point, on xyz's device")
    emb, color, pdir = (torch.empty((n, c), dtype=torch.float32, device=dev) for c in (32, 3, 3))
    row = torch.empty((n, 63), dtype=torch.float32, device=dev) if want_row else None
    if n > 0:
        a = [_host_f32(w2c, (4, 4), "w2c"), _host_f32(c2w, (4, 4), "c2w"), _host_f32(cpc, (3,), "cam_pos_cam"), _host_f32(intrinsic, (3, 3), "intrinsic")]
        head = (xyz, n, _cf(a[0]), _cf(a[1]), _cf(a[2]), _cf(a[3]), H, W, image, maps[0], maps[1], maps[2], premlp)
        if visible is not None:
            _lib.call("hnr_point_embed_vis", *head, conf, visible, emb, color, pdir, row, _lib.STREAM)
        elif conf is None:
            _lib.call("hnr_point_embed", *head, emb, color, pdir, row, _lib.STREAM)
        else:
            _lib.call("hnr_point_embed_conf", *head, conf, emb, color, pdir, row, _lib.STREAM)
    return emb, color, pdir, row


class FeatureNet(PackedWeights, nn.Module):
    """The reference's `FeatureNet(intermediate=True)` in eval mode: its parameter and buffer names, its forward signature, HIP kernels inside."""

    def __init__(self):
        super().__init__()
        for name, layers in LAYERS:
            setattr(self, name, nn.Sequential(*[_ConvBnReLU(*l) for l in layers]))
        self.toplayer = nn.Conv2d(32, 32, 1)
        self._packed = Packed()

    def pack_host(self):
        """fp32 [FEATNET_PACKED_ELEMS] on the CPU, the layout of include/hnr.h; mul = rsqrt(running_var + eps) * (|weight| + eps) is folded here, once."""
        parts = []
        with torch.no_grad():
            for name, _ in LAYERS:
                for blk in getattr(self, name):
                    w, bn = host_f32(blk.conv.weight), blk.bn
                    mul = torch.rsqrt(host_f32(bn.running_var) + EPS) * (host_f32(bn.weight).abs() + EPS)
                    parts += [w.permute(1, 2, 3, 0).reshape(-1), host_f32(bn.running_mean), mul, host_f32(bn.bias)]
            parts += [host_f32(self.toplayer.weight).reshape(-1), host_f32(self.toplayer.bias)]
            out = torch.cat([p.contiguous().reshape(-1) for p in parts])
        assert out.numel() == _lib.FEATNET_PACKED_ELEMS
        return out

    def forward(self, imgs):
        """imgs [B,V,3,H,W] -> [x [B*V,3,H,W], x1, x2, x3] (the reference's `intermediate` return)."""
        imgs = _lib.require_gpu(imgs, "imgs", torch.float32)
        if imgs.dim() != 5 or imgs.shape[2] != 3:
            raise HnrError("FeatureNet: imgs must be [B,V,3,H,W], got %s" % (tuple(imgs.shape),))
        if self.toplayer.weight.device != imgs.device:
            raise HnrError("FeatureNet: the module is on %s, imgs on %s" % (self.toplayer.weight.device, imgs.device))
        x = imgs.detach().reshape((-1,) + tuple(imgs.shape[2:]))
        return [x] + list(featnet_forward(x, self.packed()))


def occlusion_tolerance(opt, occlusion, what):
    """The tolerance of the occlusion test (cloud_init.point_occlusion) a call runs with, or None for no test.  opt.depth_occ > 0 is accepted only
    with the keyword: occlusion=True (the reference's 0.1, mvs_points_model.py:204) or a number; without depth_occ a number alone turns the test on."""
    occ = int(getattr(opt, "depth_occ", 0) or 0) > 0 if opt is not None else False
    given = occlusion is not None and occlusion is not False
    if occ and not given:
        raise HnrError("%s: depth_occ > 0 (occlusion-aware warps) is not implemented without the keyword occlusion=True" % what)
    if not given or (occlusion is True and not occ):
        return None
    tol = 0.1 if occlusion is True else float(occlusion)
    if not tol >= 0.0:
        raise HnrError("%s: occlusion must be True or a tolerance >= 0" % what)
    return tol


def check_options(opt, occlusion=None):
    """The shipped family only: anything else would need another row layout or another network."""
    fs = getattr(opt, "appr_feature_str0", FEATURE_STR)
    fs = fs.split() if isinstance(fs, str) else list(fs)
    if fs != FEATURE_STR:
        raise HnrError("MvsInit: appr_feature_str0=%r is not implemented (only %r)" % (fs, " ".join(FEATURE_STR)))
    for name, want in (("point_features_dim", 32), ("shading_feature_mlp_layer1", 2), ("act_type", "LeakyReLU")):
        if getattr(opt, name, want) != want:
            raise HnrError("MvsInit: %s=%r is not implemented (only %r)" % (name, getattr(opt, name), want))
    occlusion_tolerance(opt, occlusion, "MvsInit")
    if int(getattr(opt, "shading_feature_mlp_layer0", 1)) < 1:
        raise HnrError("MvsInit: shading_feature_mlp_layer0=0 leaves no premlp to run: use cloud_init.query_point_attributes")


class MvsInit(nn.Module):
    """`.FeatureNet` + `.premlp` under the names of the reference's MvsPointsModel, so that a `*_net_mvs.pth` loads with
    `load_state_dict(sd, strict=False)`: `MVSNet.*` keys and `num_batches_tracked` entries are ignored, every key this module owns must be there."""

    def __init__(self, opt=None, occlusion=None):
        super().__init__()
        if opt is not None:
            check_options(opt, occlusion)
        self.occlusion = occlusion_tolerance(opt, occlusion, "MvsInit")           # embed_points' default: 0.1 with occlusion=True and opt.depth_occ > 0
        self.FeatureNet = FeatureNet()
        self.premlp = nn.Sequential(nn.Linear(63, 32), nn.LeakyReLU(SLOPE, inplace=True), nn.Linear(32, 32), nn.LeakyReLU(SLOPE, inplace=True))
        self._packed = Packed()

    def load_state_dict(self, state_dict, strict=True, **kw):
        sd = filtered_state_dict(state_dict, strip=None, drop_prefixes=("MVSNet.",))
        return load_checked(self, sd, "MvsInit.load_state_dict", strict, " (pass strict=False to ignore them)", **kw)

    def premlp_packed(self):
        """[PREMLP_PACKED_ELEMS] on the device: W0^T [63][32], b0, W1^T [32][32], b1."""
        l0, l1 = self.premlp[0], self.premlp[2]

        def build():
            with torch.no_grad():
                return torch.cat([l0.weight.detach().float().t().reshape(-1), l0.bias.detach().float(), l1.weight.detach().float().t().reshape(-1),
                                  l1.bias.detach().float()]).contiguous()
        return self._packed.get([l0.weight, l0.bias, l1.weight, l1.bias], build)

    def invalidate_packed(self):
        """Drops the packed device copies of both networks' weights; needed only after replacing a parameter's storage with `p.data = ...`
        (in-place updates and load_state_dict are noticed by themselves)."""
        self._packed.invalidate()
        self.FeatureNet.invalidate_packed()

    def get_image_features(self, imgs):
        """imgs [B,V,3,H,W] -> [x, x1, x2, x3] (MvsPointsModel.get_image_features)."""
        return self.FeatureNet(imgs)

    def embed_points(self, xyz_world, image_chw, c2w, w2c, intrinsic, default_conf=-1, feats=None, want_row=False, conf=None, occlusion=None):
        """What run/train_ft.py:759-761 computes for the points of one view: (embedding [1,n,32], color [1,n,3], dir [1,n,3], conf [1,n,1]).
        image_chw [3,H,W] (or [1,3,H,W]); w2c None: the fp32 inverse of c2w, as the reference forms it.  feats: the view's [x, x1, x2, x3] from
        get_image_features when it is already there.  want_row: a fifth result, the [n,63] rows premlp saw.
        conf [n]: the points' photometric confidence (run/train_ft.py:176-180, the MVS start): premlp sees it in place of the ones and it is returned
        as [1,n,1], untouched by default_conf (which the reference applies on the depth-frame path only); None: today's ones.
        occlusion: a tolerance runs cloud_init.point_occlusion over these points first (`depth_occ = 1`: homo_warp_nongrid_occ for view 0 of the points'
        own view, w2c=None in extract_2d) and the hidden points are embedded as points outside the frame; None: the module's default (0.1 for
        MvsInit(opt, occlusion=True) with opt.depth_occ > 0, else no test); False: no test."""
        from . import cloud_init as ci
        img = _lib.require_gpu(image_chw, "image_chw", torch.float32)
        img = img.reshape(img.shape[-3:]).contiguous()
        if img.shape[0] != 3:
            raise HnrError("image_chw must be [3,H,W]")
        if feats is None:
            feats = self.get_image_features(img[None, None])
        w2c = torch.inverse(torch.from_numpy(ci._host_f32(c2w, (4, 4), "c2w"))).numpy() if w2c is None else w2c
        cpc = ci.cam_pos_cam(c2w, w2c)
        tol = self.occlusion if occlusion is None else (None if occlusion is False else (0.1 if occlusion is True else float(occlusion)))
        vis = None
        if tol is not None and int(xyz_world.numel()) > 0:
            vis = ci.point_occlusion(xyz_world, w2c, intrinsic, int(img.shape[1]), int(img.shape[2]), tol)
        emb, color, pdir, row = point_embed(xyz_world, w2c, c2w, cpc, intrinsic, img, feats[1][0], feats[2][0], feats[3][0], self.premlp_packed(), want_row,
                                            conf=conf, visible=vis)
        out = (emb[None], color[None], pdir[None],
               ci.point_conf(emb.shape[0], default_conf, emb.device) if conf is None else conf.detach().to(torch.float32).reshape(1, -1, 1).clone())
        return out + (row,) if want_row else out
