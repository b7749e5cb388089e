"""LPIPS v0.1 on the device (csrc/lpips.hip): the `lpips` (AlexNet) and `vgglpips` (VGG-16) columns of the reference's report_metrics.

`LPIPS(net)` stands in for `lpips.LPIPS(net=net, version='0.1')` in eval mode with the package's defaults (lpips=True, spatial=False) on top of
torchvision's `alexnet().features` / `vgg16().features[0:30]`: the user supplies the pretrained weights (`load_pretrained`), nothing is shipped.
`pair8` scores the two 8-bit images hnr_frame_metrics leaves on the device into a row of a device table, without a host read; `forward` has the
package's signature.  Stage functions (`prepare8`, `prepare_f32`, `tap_features`, `score`) expose the kernels one by one.  GPU only: no CPU or torch
fallback (`HnrError`).

Channel order.  run/evaluate.py reads its PNGs with cv2.imread, which returns BGR, and hands the channels to the network in that order (the comment
there says "should be RGB"; the code does not convert).  The numbers the reference publishes are therefore the BGR ones, and `channel_order="bgr"`
is the default of `pair8`; `"rgb"` is the textbook value (the order the backbones were trained on).  `forward` takes float tensors and feeds the
channels as given, as the package does.

Not built: spatial=True, squeeze, version 0.0, training of the `lin` layers, gradients.
"""
import ctypes

import numpy as np
import torch
from torch import nn

from . import _lib
from ._lib import HnrError
from .flow import pack_layer
from ._nets import Packed, PackedWeights, host_f32, load_checkpoint

NETS = {"alex": 0, "vgg": 1}
MIN_SIZE = {"alex": 31, "vgg": 16}
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
# (index in torchvision's `features`, cin, cout, kernel, stride, padding) and the slice of lpips' `net` that holds it
ALEX_CONVS = ((0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1), (10, 256, 256, 3, 1, 1))
VGG_CONVS = tuple((i, cin, cout, 3, 1, 1) for i, cin, cout in (
    (0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256), (17, 256, 512), (19, 512, 512), (21, 512, 512),
    (24, 512, 512), (26, 512, 512), (28, 512, 512)))
CONVS = {"alex": ALEX_CONVS, "vgg": VGG_CONVS}
SLICE_ENDS = {"alex": (2, 5, 8, 10, 12), "vgg": (4, 9, 16, 23, 30)}          # slice j holds features[SLICE_ENDS[j-1] : SLICE_ENDS[j]]
TAP_CHANNELS = {"alex": (64, 192, 384, 256, 256), "vgg": (64, 128, 256, 512, 512)}
NROW = 6                                                                   # d, r_0 .. r_4


def slice_of(net, index):
    """1-based slice of lpips' `net` that holds features[index]"""
    return 1 + next(j for j, end in enumerate(SLICE_ENDS[net]) if index < end)


def prep_table(shift=SHIFT, scale=SCALE):
    """[3,256] float32: what a byte becomes on its way into the network, in run/evaluate.py's fp32 operation order (float32(b) / 255.0, * 2 - 1.0) and
    the ScalingLayer's ((x - shift) / scale).  Row c belongs to network channel c."""
    v = np.arange(256, dtype=np.float32) / np.float32(255.0) * np.float32(2) - np.float32(1.0)
    return (v[None, :] - np.asarray(shift, np.float32)[:, None]) / np.asarray(scale, np.float32)[:, None]


class LPIPS(PackedWeights, nn.Module):
    """`lpips.LPIPS(net='alex'|'vgg')` in eval mode; parameters under torchvision's and the package's names (`features.<i>.*`, `lins.<k>.weight`)."""

    def __init__(self, net="alex", channel_order="bgr"):
        super().__init__()
        if net not in NETS:
            raise HnrError("LPIPS: net=%r (alex or vgg; squeeze is not implemented)" % (net,))
        if channel_order not in ("bgr", "rgb"):
            raise HnrError("LPIPS: channel_order=%r (bgr: what run/evaluate.py feeds the network; rgb: the textbook order)" % (channel_order,))
        self.net_name, self.channel_order = net, channel_order
        self.features = nn.ModuleDict({str(i): nn.Conv2d(cin, cout, k, stride=s, padding=p) for i, cin, cout, k, s, p in CONVS[net]})
        self.lins = nn.ModuleList([nn.Conv2d(c, 1, 1, bias=False) for c in TAP_CHANNELS[net]])
        self.register_buffer("shift", torch.tensor(SHIFT, dtype=torch.float32))
        self.register_buffer("scale", torch.tensor(SCALE, dtype=torch.float32))
        self._packed = Packed()
        self._scratch = {}
        self.loaded = False
        for p in self.parameters():
            p.requires_grad_(False)
        self.eval()

    def train(self, mode=True):
        if mode:
            raise HnrError("LPIPS: training mode is not implemented (inference only)")
        return super().train(False)

    # ---- weights -----------------------------------------------------------------------------------------------------------------------------------
    def load_pretrained(self, state_dict_or_path, lin=None):
        """Either (a) an `lpips.LPIPS.state_dict()` -- `net.slice<j>.<i>.weight|bias`, `lin<k>.model.1.weight` [1,C,1,1] (the `lins.<k>.*`
        duplicates are ignored), `scaling_layer.shift|scale` -- or (b) a torchvision backbone (`features.<i>.weight|bias`; `classifier.*` is ignored)
        plus `lin`: the package's `weights/v0.1/<net>.pth` (`lin<k>.model.1.weight`).  Paths go through torch.load as they are.  A missing key or a
        wrong shape is an HnrError that names the key."""
        sd = load_checkpoint(state_dict_or_path)
        if not hasattr(sd, "keys"):
            raise HnrError("LPIPS.load_pretrained: expected a state dict or a path to one")
        whole = any(k.startswith("net.slice") for k in sd.keys())
        if whole:
            if lin is not None:
                raise HnrError("LPIPS.load_pretrained: the state dict is a whole lpips.LPIPS one; `lin` must not be given with it")
            lin_sd = sd
        else:
            if lin is None:
                raise HnrError("LPIPS.load_pretrained: a torchvision backbone needs `lin`, the package's weights/v0.1/%s.pth" % self.net_name)
            lin_sd = load_checkpoint(lin)

        def take(d, key, shape):
            if key not in d:
                raise HnrError("LPIPS.load_pretrained: the state dict lacks %s" % key)
            t = torch.as_tensor(d[key])
            if tuple(t.shape) != tuple(shape):
                raise HnrError("LPIPS.load_pretrained: %s has shape %s, expected %s" % (key, tuple(t.shape), tuple(shape)))
            return t.detach().to(torch.float32)

        new = {}
        for i, cin, cout, k, _, _ in CONVS[self.net_name]:
            prefix = "net.slice%d.%d." % (slice_of(self.net_name, i), i) if whole else "features.%d." % i
            new["features.%d.weight" % i] = take(sd, prefix + "weight", (cout, cin, k, k))
            new["features.%d.bias" % i] = take(sd, prefix + "bias", (cout,))
        for k, c in enumerate(TAP_CHANNELS[self.net_name]):
            new["lins.%d.weight" % k] = take(lin_sd, "lin%d.model.1.weight" % k, (1, c, 1, 1))
        if whole:
            new["shift"] = take(sd, "scaling_layer.shift", (1, 3, 1, 1)).reshape(3)
            new["scale"] = take(sd, "scaling_layer.scale", (1, 3, 1, 1)).reshape(3)
        own = dict(self.named_parameters())
        own.update(dict(self.named_buffers()))
        with torch.no_grad():
            for name, t in new.items():
                own[name].copy_(t)
        self._packed.invalidate()
        self.loaded = True
        return self

    def pack_host(self):
        """fp32 [hnr_lpips_packed_elems(net)] on the CPU: the packed image of include/hnr.h."""
        f = host_f32
        with torch.no_grad():
            parts = [f(self.shift), f(self.scale), torch.zeros(2)]
            for i, *_ in CONVS[self.net_name]:
                conv = self.features[str(i)]
                parts.append(pack_layer(f(conv.weight), f(conv.bias)))
            parts += [f(l.weight).reshape(-1) for l in self.lins]
            return torch.cat(parts).contiguous()

    def packed(self):
        """The packed image on the module's device: packed once on the host, again only after the weights changed (load_pretrained, .to())."""
        if not self.loaded:
            raise HnrError("LPIPS: no weights loaded (load_pretrained); the package ships none")
        return super().packed()

    def check_packed(self, pk):
        n = _lib.size("hnr_lpips_packed_elems", NETS[self.net_name])
        if pk.numel() != n:
            raise HnrError("LPIPS: the packed image has %d elements, the library expects %d" % (pk.numel(), n))

    # ---- plumbing ----------------------------------------------------------------------------------------------------------------------------------
    def _net(self):
        return NETS[self.net_name]

    def _check_size(self, h, w, what):
        m = MIN_SIZE[self.net_name]
        if h < m or w < m or h > 4096 or w > 4096:
            raise HnrError("%s: %dx%d images (%s needs %d .. 4096 in both directions: below it the last tap has no pixel)" % (what, h, w, self.net_name, m))

    def _device(self, t, what):
        dev = self.shift.device
        if dev.type != "cuda":
            raise HnrError("%s: the module is on %s (move it to the GPU: there is no CPU fallback)" % (what, dev))
        if t.device != dev:
            raise HnrError("%s: the module is on %s, the images on %s" % (what, dev, t.device))
        return dev

    def scratch(self, h, w):
        """The scratch of one image size, kept: [bytes] uint8 on the module's device."""
        key = (h, w, str(self.shift.device))
        if key not in self._scratch:
            self._scratch[key] = _lib.scratch("hnr_lpips_scratch_bytes", self._net(), h, w, device=self.shift.device,
                                              what="hnr_lpips_scratch_bytes refused %s %dx%d" % (self.net_name, h, w))
        return self._scratch[key]

    def tap_dims(self, h, w):
        dims = (ctypes.c_int * 15)()
        _lib.call("hnr_lpips_tap_dims", self._net(), h, w, dims)
        return [tuple(dims[3 * k:3 * k + 3]) for k in range(5)]

    def _images8(self, img8, gt8, what):
        for t in (img8, gt8):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise HnrError("%s: the images must be tensors on the GPU (there is no CPU fallback)" % what)
            if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or not t.is_contiguous():
                raise HnrError("%s: the images must be contiguous [h, w, 3] uint8 tensors" % what)
        if img8.shape != gt8.shape:
            raise HnrError("%s: the images differ in shape: %s and %s" % (what, tuple(img8.shape), tuple(gt8.shape)))
        self._device(img8, what)
        return int(img8.shape[0]), int(img8.shape[1])

    def _images_f32(self, in0, in1, what):
        out = []
        for t in (in0, in1):
            t = _lib.require_gpu(t, what + ": in0 / in1", torch.float32).detach()
            if t.dim() != 4 or t.shape[0] != 1 or t.shape[1] != 3:
                raise HnrError("%s: the images must be [1,3,H,W], got %s" % (what, tuple(t.shape)))
            out.append(t)
        if out[0].shape != out[1].shape:
            raise HnrError("%s: the images differ in shape" % what)
        self._device(out[0], what)
        return out[0], out[1], int(out[0].shape[2]), int(out[0].shape[3])

    def _table(self, out, row, what):
        dev = self.shift.device
        if out is None:
            out = torch.zeros((1, NROW), dtype=torch.float64, device=dev)
        if not (out.is_cuda and out.dtype == torch.float64 and out.dim() == 2 and out.shape[1] == NROW and out.is_contiguous()):
            raise HnrError("%s: out must be a contiguous [capacity, %d] float64 table on the GPU" % (what, NROW))
        if not 0 <= row < out.shape[0]:
            raise HnrError("%s: row %d outside the table (%d rows)" % (what, row, out.shape[0]))
        return out

    # ---- stages (tests, tools) -----------------------------------------------------------------------------------------------------------------------
    def prepare8(self, img8, gt8):
        """hnr_lpips_prepare: two [h,w,3] uint8 RGB images -> [2,3,h,w] float32, the network's input."""
        h, w = self._images8(img8, gt8, "LPIPS.prepare8")
        x = torch.empty((2, 3, h, w), dtype=torch.float32, device=img8.device)
        _lib.call("hnr_lpips_prepare", img8, gt8, h, w, int(self.channel_order == "bgr"), self.packed(), x, _lib.STREAM)
        return x

    def prepare_f32(self, in0, in1):
        """hnr_lpips_prepare_f32: two [1,3,H,W] float images in [-1, 1] -> [2,3,H,W], the ScalingLayer's output."""
        a, b, h, w = self._images_f32(in0, in1, "LPIPS.prepare_f32")
        x = torch.empty((2, 3, h, w), dtype=torch.float32, device=a.device)
        _lib.call("hnr_lpips_prepare_f32", a, b, h, w, self.packed(), x, _lib.STREAM)
        return x

    def tap_features(self, x):
        """hnr_lpips_features: the network's input [2,3,h,w] -> the five taps, [2,C_k,h_k,w_k] each."""
        x = _lib.require_gpu(x, "LPIPS.tap_features: x", torch.float32)
        if x.dim() != 4 or x.shape[0] != 2 or x.shape[1] != 3:
            raise HnrError("LPIPS.tap_features: x must be [2,3,h,w], got %s" % (tuple(x.shape),))
        self._device(x, "LPIPS.tap_features")
        h, w = int(x.shape[2]), int(x.shape[3])
        self._check_size(h, w, "LPIPS.tap_features")
        taps = [torch.empty((2,) + d, dtype=torch.float32, device=x.device) for d in self.tap_dims(h, w)]
        ptrs = (ctypes.c_void_p * 5)(*[t.data_ptr() for t in taps])
        s = self.scratch(h, w)
        _lib.call("hnr_lpips_features", self._net(), x, h, w, self.packed(), ptrs, s, s.numel(), _lib.STREAM)
        return taps

    def score(self, taps, h, w, out=None, row=0):
        """hnr_lpips_score: the five taps of an h x w pair -> row [d, r_0 .. r_4] of a float64 device table."""
        self._check_size(h, w, "LPIPS.score")
        dims = self.tap_dims(h, w)
        taps = [_lib.require_gpu(t, "LPIPS.score: tap", torch.float32) for t in taps]
        if len(taps) != 5 or any(tuple(t.shape) != (2,) + d for t, d in zip(taps, dims)):
            raise HnrError("LPIPS.score: the taps of a %dx%d pair are %s (each for a batch of two)" % (h, w, dims))
        self._device(taps[0], "LPIPS.score")
        out = self._table(out, row, "LPIPS.score")
        ptrs = (ctypes.c_void_p * 5)(*[t.data_ptr() for t in taps])
        s = self.scratch(h, w)
        _lib.call("hnr_lpips_score", self._net(), ptrs, h, w, self.packed(), out[row], s, s.numel(), _lib.STREAM)
        return out

    # ---- the whole chain ---------------------------------------------------------------------------------------------------------------------------
    def pair8(self, img8, gt8, out=None, row=0):
        """hnr_lpips on two [h,w,3] uint8 RGB device images (those frame_metrics leaves in `images8`): row `row` of `out`, a [capacity, 6] float64
        device table (default: a fresh [1, 6] one), becomes [d, r_0 .. r_4].  No host read.  Returns the table."""
        h, w = self._images8(img8, gt8, "LPIPS.pair8")
        self._check_size(h, w, "LPIPS.pair8")
        out = self._table(out, row, "LPIPS.pair8")
        s = self.scratch(h, w)
        _lib.call("hnr_lpips", self._net(), img8, gt8, h, w, int(self.channel_order == "bgr"), self.packed(), out[row], s, s.numel(), _lib.STREAM)
        return out

    def forward(self, in0, in1, normalize=False, retPerLayer=False):
        """The package's forward: in0, in1 [1,3,H,W] float on the GPU, in [-1, 1] (normalize=True: in [0, 1]), channels fed as given ->
        [1,1,1,1] float32 on the device."""
        if retPerLayer:
            raise HnrError("LPIPS: retPerLayer=True is not implemented (pair8 / score give r_0 .. r_4)")
        a, b, h, w = self._images_f32(in0, in1, "LPIPS.forward")
        self._check_size(h, w, "LPIPS.forward")
        if normalize:
            a, b = 2 * a - 1, 2 * b - 1
        out = torch.zeros((1, NROW), dtype=torch.float64, device=a.device)
        s = self.scratch(h, w)
        _lib.call("hnr_lpips_f32", self._net(), a, b, h, w, self.packed(), out[0], s, s.numel(), _lib.STREAM)
        return out[0, 0].to(torch.float32).reshape(1, 1, 1, 1)
