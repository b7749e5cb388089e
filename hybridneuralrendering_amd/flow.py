"""RAFT optical flow on the device (csrc/raft.hip): the flow half of the content-aware frame weights (frame_weights.py).

`RAFT` carries the parameter and buffer names of the reference's `raft/core/raft.py` basic model (`fnet.*`, `cnet.*`, `update_block.*`), so the published
`raft-things.pth` loads as it is, and runs it as HIP kernels, stage by stage: `encoder`, `corr_pyramid`, `lookup`, `update`, `upsample`; `forward` is the
single call `hnr_raft_flow`.  Only the configuration raft/demo_content_aware_weights.py runs is built: the basic model, fp32, inference,
`test_mode=True`, `flow_init=None`.  `alternate_corr` gives the same numbers up to rounding and is accepted and ignored.  GPU only: no CPU or torch
fallback (`HnrError`).
"""
import torch
from torch import nn

from . import _lib
from ._lib import HnrError
from ._nets import NormParams, Packed, PackedWeights, filtered_state_dict, gpu_f32, host_f32, load_checked, load_checkpoint

EPS = 1e-5
ENC_BLOCKS = (("layer1.0", 64, 64, 1), ("layer1.1", 64, 64, 1), ("layer2.0", 64, 96, 2), ("layer2.1", 96, 96, 1), ("layer3.0", 96, 128, 2),
              ("layer3.1", 128, 128, 1))
CORR_LEVELS, CORR_RADIUS = 4, 4
CORR_PLANES = CORR_LEVELS * (2 * CORR_RADIUS + 1) ** 2


def check_shape(H, W, what="RAFT"):
    if H % 8 or W % 8:
        raise HnrError("%s: H=%d and W=%d must be multiples of 8 (the reference's script never un-pads the flow, so its own warp fails on padded "
                       "sizes)" % (what, H, W))
    if H // 8 < 16 or W // 8 < 16:
        raise HnrError("%s: H/8=%d and W/8=%d must be at least 16 (below it the coarsest correlation level has an extent of 1, where the reference "
                       "divides by W-1 = 0)" % (what, H // 8, W // 8))
    if H > 4096 or W > 4096 or (H // 8) * (W // 8) > 16384:
        raise HnrError("%s: H=%d, W=%d is too large (H, W <= 4096, H/8*W/8 <= 16384: the correlation volume is materialised)" % (what, H, W))


def pyramid_shapes(h, w):
    out = [(h, w)]
    for _ in range(CORR_LEVELS - 1):
        out.append((out[-1][0] // 2, out[-1][1] // 2))
    return out


def encoder(images, packed, norm):
    """hnr_raft_encoder: images [N,3,H,W] (0..255), N = 1 or 2 -> [N,256,H/8,W/8].  norm: 0 instance norm, 1 folded batch norm, 2 folded batch norm
    then tanh | relu on the two halves of the channels."""
    images = gpu_f32(images, "images")
    if images.dim() != 4 or images.shape[1] != 3 or images.shape[0] not in (1, 2):
        raise HnrError("encoder: images must be [1 or 2,3,H,W], got %s" % (tuple(images.shape),))
    N, _, H, W = (int(s) for s in images.shape)
    check_shape(H, W, "encoder")
    packed = gpu_f32(packed, "packed", (_lib.size("hnr_raft_encoder_packed_elems"),))
    scratch = _lib.scratch("hnr_raft_encoder_scratch_elems", N, H, W, device=images.device, dtype=torch.float32)
    out = torch.empty((N, 256, H // 8, W // 8), dtype=torch.float32, device=images.device)
    _lib.call("hnr_raft_encoder", images, N, H, W, packed, int(norm), out, scratch, scratch.numel(), _lib.STREAM)
    return out


def corr_pyramid(fmap1, fmap2):
    """hnr_raft_corr_pyramid: fmap1, fmap2 [256,h,w] -> the four levels [h*w,h_l,w_l] as views of one buffer."""
    fmap1, fmap2 = gpu_f32(fmap1, "fmap1"), gpu_f32(fmap2, "fmap2", tuple(fmap1.shape))
    if fmap1.dim() != 3 or fmap1.shape[0] != 256:
        raise HnrError("corr_pyramid: fmap1 must be [256,h,w], got %s" % (tuple(fmap1.shape),))
    h, w = int(fmap1.shape[1]), int(fmap1.shape[2])
    check_shape(8 * h, 8 * w, "corr_pyramid")
    buf = _lib.scratch("hnr_raft_pyramid_elems", h, w, device=fmap1.device, dtype=torch.float32)
    scratch = _lib.scratch("hnr_raft_pyramid_scratch_elems", h, w, device=fmap1.device, dtype=torch.float32)
    _lib.call("hnr_raft_corr_pyramid", fmap1, fmap2, h, w, buf, scratch, scratch.numel(), _lib.STREAM)
    return buf


def pyramid_levels(buf, h, w):
    out, off = [], 0
    for hl, wl in pyramid_shapes(h, w):
        out.append(buf[off:off + h * w * hl * wl].view(h * w, hl, wl))
        off += h * w * hl * wl
    return out


def lookup(pyramid, coords):
    """hnr_raft_lookup: the pyramid buffer of corr_pyramid, coords [2,h,w] (x, y) -> [324,h,w]."""
    pyramid, coords = gpu_f32(pyramid, "pyramid"), gpu_f32(coords, "coords")
    if coords.dim() != 3 or coords.shape[0] != 2:
        raise HnrError("lookup: coords must be [2,h,w], got %s" % (tuple(coords.shape),))
    h, w = int(coords.shape[1]), int(coords.shape[2])
    check_shape(8 * h, 8 * w, "lookup")
    if pyramid.numel() != _lib.size("hnr_raft_pyramid_elems", h, w):
        raise HnrError("lookup: the pyramid does not belong to a %dx%d map" % (h, w))
    out = torch.empty((CORR_PLANES, h, w), dtype=torch.float32, device=coords.device)
    _lib.call("hnr_raft_lookup", pyramid, coords, h, w, out, _lib.STREAM)
    return out


def update(packed, pyramid, net, inp, coords, want_mask=False):
    """hnr_raft_update, one iteration: net [128,h,w], inp [128,h,w], coords [2,h,w] -> (net, coords, delta_flow [2,h,w], mask [576,h,w] or None); the
    inputs are left as they are."""
    net, inp, coords = gpu_f32(net, "net").clone(), gpu_f32(inp, "inp", tuple(net.shape)), gpu_f32(coords, "coords").clone()
    if net.dim() != 3 or net.shape[0] != 128 or tuple(coords.shape) != (2,) + tuple(net.shape[1:]):
        raise HnrError("update: net and inp must be [128,h,w] and coords [2,h,w]")
    h, w = int(net.shape[1]), int(net.shape[2])
    check_shape(8 * h, 8 * w, "update")
    packed = gpu_f32(packed, "packed", (_lib.size("hnr_raft_update_packed_elems"),))
    pyramid = gpu_f32(pyramid, "pyramid", (_lib.size("hnr_raft_pyramid_elems", h, w),))
    delta = torch.empty((2, h, w), dtype=torch.float32, device=net.device)
    mask = torch.empty((576, h, w), dtype=torch.float32, device=net.device) if want_mask else None
    scratch = _lib.scratch("hnr_raft_update_scratch_elems", h, w, device=net.device, dtype=torch.float32)
    _lib.call("hnr_raft_update", packed, pyramid, net, inp, coords, h, w, delta, mask, scratch, scratch.numel(), _lib.STREAM)
    return net, coords, delta, mask


def upsample(flow, mask):
    """hnr_raft_upsample: flow [2,h,w], mask [576,h,w] -> [2,8h,8w]."""
    flow, mask = gpu_f32(flow, "flow"), gpu_f32(mask, "mask")
    if flow.dim() != 3 or flow.shape[0] != 2 or tuple(mask.shape) != (576,) + tuple(flow.shape[1:]) or flow.shape[1] * flow.shape[2] > 16384:
        raise HnrError("upsample: flow must be [2,h,w] and mask [576,h,w], h*w <= 16384")
    h, w = int(flow.shape[1]), int(flow.shape[2])
    out = torch.empty((2, 8 * h, 8 * w), dtype=torch.float32, device=flow.device)
    _lib.call("hnr_raft_upsample", flow, mask, h, w, out, _lib.STREAM)
    return out


class _ResidualBlock(nn.Module):
    def __init__(self, cin, cout, stride, batch_norm):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, padding=1, stride=stride)
        self.conv2 = nn.Conv2d(cout, cout, 3, padding=1)
        if batch_norm:
            self.norm1, self.norm2 = NormParams(cout), NormParams(cout)
        if stride != 1:
            if batch_norm:
                self.norm3 = NormParams(cout)                           # (the reference registers it twice: as norm3 and as downsample.1)
                self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride=stride), self.norm3)
            else:
                self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride=stride))


class _BasicEncoder(nn.Module):
    def __init__(self, output_dim, batch_norm):
        super().__init__()
        self.batch_norm = batch_norm
        if batch_norm:
            self.norm1 = NormParams(64)
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3)
        for i in (1, 2, 3):
            a, b = ENC_BLOCKS[2 * i - 2], ENC_BLOCKS[2 * i - 1]
            setattr(self, "layer%d" % i, nn.Sequential(_ResidualBlock(a[1], a[2], a[3], batch_norm), _ResidualBlock(b[1], b[2], b[3], batch_norm)))
        self.conv2 = nn.Conv2d(128, output_dim, 1)

    def _layer(self, conv, norm, scale=1.0):
        """w [kh*kw][cinp][cout], bias [cout]; an eval-mode batch norm y = (x - mean) * mul + beta, mul = weight * rsqrt(var + eps), is folded in."""
        w, b = host_f32(conv.weight).double(), host_f32(conv.bias).double()
        if norm is not None:
            mul = host_f32(norm.weight).double() / torch.sqrt(host_f32(norm.running_var).double() + EPS)
            w, b = w * mul[:, None, None, None], (b - host_f32(norm.running_mean).double()) * mul + host_f32(norm.bias).double()
        return pack_layer(w * scale, b * scale)

    def pack_host(self):
        bn = self.batch_norm
        with torch.no_grad():
            parts = [self._layer(self.conv1, self.norm1 if bn else None)]
            for name, _, _, stride in ENC_BLOCKS:
                blk = self.get_submodule(name)
                parts.append(self._layer(blk.conv1, blk.norm1 if bn else None))
                parts.append(self._layer(blk.conv2, blk.norm2 if bn else None))
                if stride != 1:
                    parts.append(self._layer(blk.downsample[0], blk.norm3 if bn else None))
            parts.append(self._layer(self.conv2, None))
            return torch.cat(parts)


def pack_layer(w, b):
    """[cout,cin,kh,kw], [cout] -> fp32 [kh*kw*cinp*cout + cout]: the packed layer of include/hnr.h."""
    cout, cin, kh, kw = w.shape
    t = torch.zeros((kh * kw, cin + (cin & 1), cout), dtype=w.dtype)
    t[:, :cin] = w.permute(2, 3, 1, 0).reshape(kh * kw, cin, cout)
    return torch.cat([t.reshape(-1), b.reshape(-1)]).float()


class _FlowHead(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1, self.conv2 = nn.Conv2d(128, 256, 3, padding=1), nn.Conv2d(256, 2, 3, padding=1)


class _MotionEncoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.convc1, self.convc2 = nn.Conv2d(CORR_PLANES, 256, 1), nn.Conv2d(256, 192, 3, padding=1)
        self.convf1, self.convf2 = nn.Conv2d(2, 128, 7, padding=3), nn.Conv2d(128, 64, 3, padding=1)
        self.conv = nn.Conv2d(64 + 192, 128 - 2, 3, padding=1)


class _SepConvGRU(nn.Module):
    def __init__(self):
        super().__init__()
        for n in "zrq":
            setattr(self, "conv%s1" % n, nn.Conv2d(384, 128, (1, 5), padding=(0, 2)))
            setattr(self, "conv%s2" % n, nn.Conv2d(384, 128, (5, 1), padding=(2, 0)))


class _UpdateBlock(nn.Module):
    def __init__(self):
        super().__init__()
        self.encoder, self.gru, self.flow_head = _MotionEncoder(), _SepConvGRU(), _FlowHead()
        self.mask = nn.Sequential(nn.Conv2d(128, 256, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(256, 64 * 9, 1))

    def pack_host(self):
        e, g, fh = self.encoder, self.gru, self.flow_head
        p = lambda c, s=1.0: pack_layer(host_f32(c.weight) * s, host_f32(c.bias) * s)
        zr = lambda z, r: pack_layer(torch.cat([host_f32(z.weight), host_f32(r.weight)]), torch.cat([host_f32(z.bias), host_f32(r.bias)]))
        with torch.no_grad():
            return torch.cat([p(e.convc1), p(e.convc2), p(e.convf1), p(e.convf2), p(e.conv), zr(g.convz1, g.convr1), p(g.convq1), zr(g.convz2, g.convr2),
                              p(g.convq2), p(fh.conv1), p(fh.conv2), p(self.mask[0]), p(self.mask[2], 0.25)])


def _arg(args, name, default):
    if args is None:
        return default
    if isinstance(args, dict):
        return args.get(name, default)
    return getattr(args, name, default)


class RAFT(PackedWeights, nn.Module):
    """The reference's `RAFT(args)` basic model in eval mode: its parameter and buffer names, its forward signature, HIP kernels inside."""

    def __init__(self, args=None):
        super().__init__()
        if _arg(args, "small", False):
            raise HnrError("RAFT: small=True (the small model) is not implemented")
        if _arg(args, "mixed_precision", False):
            raise HnrError("RAFT: mixed_precision=True is not implemented (fp32 only)")
        if _arg(args, "dropout", 0):
            raise HnrError("RAFT: dropout > 0 belongs to training, which is not implemented")
        self.args = args                                         # alternate_corr: same numbers up to rounding; accepted and ignored
        self.hidden_dim = self.context_dim = 128
        self.fnet = _BasicEncoder(256, batch_norm=False)
        self.cnet = _BasicEncoder(256, batch_norm=True)
        self.update_block = _UpdateBlock()
        self._packed = Packed()
        self.eval()

    def train(self, mode=True):
        if mode:
            raise HnrError("RAFT: training mode is not implemented (inference only)")
        return super().train(False)

    def load_pretrained(self, path_or_dict):
        """The published checkpoint as it is (demo_content_aware_weights.py:96-97 loads it into a DataParallel): `module.` is stripped,
        `num_batches_tracked` entries are ignored, a missing or an unexpected key is an HnrError."""
        load_checked(self, filtered_state_dict(load_checkpoint(path_or_dict)), "RAFT.load_pretrained")
        return self

    def pack_host(self):
        """(fnet, cnet, update_block) fp32 on the CPU, the packed images of include/hnr.h."""
        f, c, u = self.fnet.pack_host(), self.cnet.pack_host(), self.update_block.pack_host()
        assert f.numel() == c.numel() == _lib.size("hnr_raft_encoder_packed_elems") and u.numel() == _lib.size("hnr_raft_update_packed_elems")
        return f, c, u

    def forward(self, image1, image2, iters=20, flow_init=None, upsample=True, test_mode=True):
        """image1, image2 [1,3,H,W], values 0..255 -> (flow_low [1,2,H/8,W/8], flow_up [1,2,H,W])."""
        if not test_mode:
            raise HnrError("RAFT: test_mode=False (the list of every iteration's flow, for training) is not implemented")
        if flow_init is not None:
            raise HnrError("RAFT: flow_init is not implemented")
        if not upsample:
            raise HnrError("RAFT: upsample=False is not implemented")
        for t, name in ((image1, "image1"), (image2, "image2")):
            if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[0] != 1 or t.shape[1] != 3:
                raise HnrError("RAFT: %s must be a tensor [1,3,H,W]" % name)
        if image1.shape != image2.shape:
            raise HnrError("RAFT: image1 %s and image2 %s differ in shape" % (tuple(image1.shape), tuple(image2.shape)))
        H, W = int(image1.shape[2]), int(image1.shape[3])
        check_shape(H, W)
        iters = int(iters)
        if not 1 <= iters <= 1024:
            raise HnrError("RAFT: iters=%d (1 .. 1024)" % iters)
        pair = torch.cat([gpu_f32(image1, "image1"), gpu_f32(image2, "image2")])
        low, up = self.flow_pair(pair, iters)
        return low[None], up[None]

    def flow_pair(self, pair, iters=20):
        """pair [2,3,H,W] fp32 on the device -> (flow_low [2,h,w], flow_up [2,H,W]): hnr_raft_flow."""
        dev = self.fnet.conv1.weight.device
        if dev != pair.device:
            raise HnrError("RAFT: the module is on %s, the images on %s" % (dev, pair.device))
        H, W = int(pair.shape[2]), int(pair.shape[3])
        fn, cn, ub = self.packed()
        low = torch.empty((2, H // 8, W // 8), dtype=torch.float32, device=dev)
        up = torch.empty((2, H, W), dtype=torch.float32, device=dev)
        scratch = _lib.scratch("hnr_raft_flow_scratch_elems", H, W, device=dev, dtype=torch.float32)
        _lib.call("hnr_raft_flow", pair, pair[1], H, W, fn, cn, ub, int(iters), low, up, scratch, scratch.numel(), _lib.STREAM)
        return low, up
