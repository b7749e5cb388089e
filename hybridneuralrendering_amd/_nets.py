"""Host-side helpers of the pretrained inference nets (mvs_init, mvs_depth, flow, perceptual): argument checks, the norm layers' parameter holder,
checkpoint loading under the reference's key names, and the cache of a module's packed weights on the device."""
import torch
from torch import nn

from . import _lib
from ._cache import Derived as Packed          # a module's packed weights on the device: one cache entry (flow, perceptual, mvs_init, mvs_depth import it from here)
from ._lib import HnrError


def gpu_f32(t, name, shape=None):
    t = _lib.require_gpu(t, name, torch.float32).detach()
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise HnrError("%s must be %s, got %s" % (name, tuple(shape), tuple(t.shape)))
    return t


def host_f32(t):
    return t.detach().float().cpu()


class NormParams(nn.Module):
    """Parameter holder with the names of nn.BatchNorm and InPlaceABN; the arithmetic lives in the convolution kernels' epilogue or is folded into the
    packed weights (each net's pack_host)."""

    def __init__(self, ch):
        super().__init__()
        self.weight, self.bias = nn.Parameter(torch.ones(ch)), nn.Parameter(torch.zeros(ch))
        self.register_buffer("running_mean", torch.zeros(ch))
        self.register_buffer("running_var", torch.ones(ch))


def load_checkpoint(obj):
    """A path (str, bytes, os.PathLike) goes through torch.load onto the CPU; anything else is returned as it is."""
    if isinstance(obj, (str, bytes)) or hasattr(obj, "__fspath__"):
        return torch.load(obj, map_location="cpu")
    return obj


def filtered_state_dict(sd, strip="module.", drop_prefixes=()):
    """sd without its `num_batches_tracked` entries and the keys under drop_prefixes; a leading `strip` (DataParallel's `module.`) is removed."""
    return {(k[len(strip):] if strip and k.startswith(strip) else k): v for k, v in sd.items()
            if not k.endswith("num_batches_tracked") and not k.startswith(tuple(drop_prefixes))}


def load_checked(module, sd, who, strict=True, hint="", **kw):
    """nn.Module.load_state_dict(module, sd): a missing key is an HnrError, and so, under strict, is an unexpected one."""
    res = nn.Module.load_state_dict(module, sd, strict=False, **kw)
    if res.missing_keys:
        raise HnrError("%s: the checkpoint lacks %s" % (who, ", ".join(sorted(res.missing_keys))))
    if strict and res.unexpected_keys:
        raise HnrError("%s: unexpected keys %s%s" % (who, ", ".join(sorted(res.unexpected_keys)), hint))
    return res


class PackedWeights:
    """Mixin of an nn.Module that has `pack_host()` (a CPU tensor or a tuple of them) and a `Packed` in `self._packed`."""

    def check_packed(self, pk):
        """Sees pack_host()'s result before it is copied to the device and cached; raises if it is not what the library expects."""

    def packed(self):
        """pack_host()'s result on the module's device: packed once, again only after a parameter or buffer changed or moved."""
        dev = next(self.parameters()).device

        def build():
            pk = self.pack_host()
            self.check_packed(pk)
            return pk.to(dev) if isinstance(pk, torch.Tensor) else tuple(p.to(dev) for p in pk)
        return self._packed.get(list(self.parameters()) + list(self.buffers()), build)

    def invalidate_packed(self):
        """Needed only after replacing a parameter's storage with `p.data = ...` (_cache.py, rule 2)."""
        self._packed.invalidate()
