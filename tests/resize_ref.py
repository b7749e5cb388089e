"""NumPy restatement of Pillow's convolution resize for 8-bit images (src/libImaging/Resample.c, 8bpc path) and of the steps around it:
what csrc/resize.hip computes, written down so that tests can compare integers and bytes.  tests/test_resize.py holds this text to
PIL.Image.resize itself; the GPU tests hold the kernels to Pillow and to this.

Per axis, `n_in` -> `n_out` elements, filter of support S:
    scale = n_in / n_out, fs = max(scale, 1), support = S fs, ksize = 2 ceil(support) + 1, ss = 1 / fs
    centre = (xx + 0.5) scale, xmin = max(int(centre - support + 0.5), 0), xmax = min(int(centre + support + 0.5), n_in) - xmin
    w[x] = filter((x + xmin - centre + 0.5) ss), normalised by their sum in index order, then fixed point with 22 bits, rounded half away from zero
all in double with libm's sin / cos (math.sin: NumPy's vectorised sine is another implementation and may differ in the last bit).
One pass: out = clip8((2^21 + sum_x in[xmin + x] k[x]) >> 22), int32, arithmetic shift.  Horizontal first, rounded to uint8, then vertical; a pass
whose size does not change is skipped."""
import math

import numpy as np

PRECISION_BITS = 22
FILTERS = ("box", "bilinear", "hamming", "bicubic", "lanczos")           # the ids of hnr_resize_coeffs: 0 .. 4
SUPPORT = dict(box=0.5, bilinear=1.0, hamming=1.0, bicubic=2.0, lanczos=3.0)


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (0.54 + 0.46 * math.cos(x))


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


_FN = dict(box=_box, bilinear=_bilinear, hamming=_hamming, bicubic=_bicubic, lanczos=_lanczos)


def coeffs(n_in, n_out, filt="lanczos"):
    """-> (ksize, bounds [n_out,2] int32 (xmin, xmax), coef [n_out,ksize] int32; entries past xmax are 0)"""
    fn, S = _FN[filt], SUPPORT[filt]
    scale = float(n_in) / float(n_out)
    fs = scale if scale > 1.0 else 1.0
    support = S * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((n_out, 2), np.int32)
    coef = np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [fn((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, xmax)
        for x, v in enumerate(w):
            coef[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
    return ksize, bounds, coef


def pass_sums(img, bounds, coef, axis):
    """The int32 sums of one pass before the shift: img [..] uint8, resampled along `axis` -> int64 array (values fit int32)"""
    a = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((bounds.shape[0],) + a.shape[1:], np.int64)
    for xx, (xmin, xmax) in enumerate(bounds):
        k = coef[xx, :xmax].astype(np.int64).reshape((-1,) + (1,) * (a.ndim - 1))
        out[xx] = (1 << (PRECISION_BITS - 1)) + (a[xmin:xmin + xmax] * k).sum(axis=0)
    assert np.abs(out).max(initial=0) < (1 << 31)
    return np.moveaxis(out, 0, axis)


def resample_pass(img, bounds, coef, axis):
    return np.clip(pass_sums(img, bounds, coef, axis) >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize(img, size, filt="lanczos"):
    """img [h,w] or [h,w,C] uint8, size = (W, H) as Pillow orders it -> [H,W(,C)] uint8: Image.resize(size, filter) for modes L, RGB and the
    four channels of a premultiplied RGBA image"""
    img = np.asarray(img)
    W, H = int(size[0]), int(size[1])
    h, w = img.shape[:2]
    out = img
    if w != W:
        _, b, k = coeffs(w, W, filt)
        out = resample_pass(out, b, k, 1)
    if h != H:
        _, b, k = coeffs(h, H, filt)
        out = resample_pass(out, b, k, 0)
    return out.copy() if out is img else out


def premultiply(rgba):
    """[...,4] uint8 -> colours times alpha by Pillow's MULDIV255: ((t >> 8) + t) >> 8, t = c a + 128; alpha kept"""
    a = rgba[..., 3:4].astype(np.int32)
    t = rgba[..., :3].astype(np.int32) * a + 128
    out = rgba.copy()
    out[..., :3] = (((t >> 8) + t) >> 8).astype(np.uint8)
    return out


def unpremultiply(rgba):
    """[...,4] uint8 -> c when alpha is 0 or 255, else min(255 c / a, 255) with integer division; alpha kept"""
    a = rgba[..., 3:4].astype(np.int32)
    c = rgba[..., :3].astype(np.int32)
    q = np.minimum(255 * c // np.maximum(a, 1), 255)
    out = rgba.copy()
    out[..., :3] = np.where((a == 0) | (a == 255), c, q).astype(np.uint8)
    return out


def resize_rgba(img, size, filt="lanczos"):
    """Image.resize of a mode-RGBA image with a convolution filter: premultiply, resize the four channels, un-premultiply.  Pillow returns a copy
    of a same-size image before any of that (the round trip would change colours under partial alpha)."""
    img = np.asarray(img)
    if (int(size[0]), int(size[1])) == (img.shape[1], img.shape[0]):
        return img.copy()
    return unpremultiply(resize(premultiply(np.asarray(img)), size, filt))


def compose(rgba8):
    """data/nerf_synth360_ft_dataset.py:532-536 on a resized RGBA frame [...,4] uint8, float32 with every operation rounded on its own:
    c, a = u8 / 255; white = c a + (1 - a), black = c a, alpha = a, mask = (a > 0.1) as float32"""
    f = rgba8.astype(np.float32) / np.float32(255.0)
    c, a = f[..., :3], f[..., 3:4]
    black = c * a
    white = black + (np.float32(1.0) - a)
    return dict(white=white, black=black, alpha=a[..., 0], mask=(a[..., 0] > np.float32(0.1)).astype(np.float32))


def scaled_intrinsic(intrinsic, raw_wh, wh):
    """data/scannet_ft_dataset.py:178-179: row 0 times W / w_raw, row 1 times H / h_raw, the float32 array times a Python float, in place"""
    K = np.array(intrinsic, dtype=np.float32)
    K[0, :] *= (wh[0] / raw_wh[0])
    K[1, :] *= (wh[1] / raw_wh[1])
    return K
