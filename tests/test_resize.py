"""CPU checks of the device resize (csrc/resize.hip, frames.resize_frames / FrameBank.from_raw): the NumPy restatement tests/resize_ref.py against
PIL.Image.resize itself, hnr_resize_coeffs (a host function) against the restatement's integers, the intrinsic scaling, the compose arithmetic and
the bad-argument returns.  Every comparison is an equality of bytes, integers or bits.  No GPU is needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

from hybridneuralrendering_amd import _lib, frames
from hybridneuralrendering_amd._lib import HnrError

from tests import resize_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIL_FILTER = dict(box=Image.BOX, bilinear=Image.BILINEAR, hamming=Image.HAMMING, bicubic=Image.BICUBIC, lanczos=Image.LANCZOS)
# ((h, w) -> (H, W)): the shapes of the issue
RGB_SHAPES = [((968, 1296), (480, 640)), ((37, 53), (11, 17)), ((7, 9), (20, 23)), ((16, 16), (16, 5)), ((5, 40), (9, 40)), ((100, 100), (1, 1)),
              ((3, 3), (7, 2))]
RGBA_SHAPES = [((800, 800), (400, 400)), ((37, 53), (11, 17)), ((7, 9), (20, 23))]


def image(shape, channels, seed=0):
    a = np.random.default_rng(seed).integers(0, 256, size=tuple(shape) + (channels,), dtype=np.uint8)
    return a[..., 0] if channels == 1 else a


def pil_resize(a, HW, filt="lanczos"):
    return np.asarray(Image.fromarray(a).resize((HW[1], HW[0]), PIL_FILTER[filt]))


@pytest.mark.parametrize("shape,out", RGB_SHAPES)
def test_restatement_equals_pillow_lanczos_rgb(shape, out):
    a = image(shape, 3, seed=shape[0])
    np.testing.assert_array_equal(R.resize(a, (out[1], out[0])), pil_resize(a, out))


@pytest.mark.parametrize("shape,out", RGBA_SHAPES)
def test_restatement_equals_pillow_lanczos_rgba(shape, out):
    a = image(shape, 4, seed=shape[0])
    got = R.resize_rgba(a, (out[1], out[0]))
    np.testing.assert_array_equal(got, pil_resize(a, out))
    assert np.any(got != R.resize(a, (out[1], out[0])))            # RGBA mode is not four independent channels


def test_same_size_rgba_is_a_copy_as_pillows():
    """Image.resize returns a copy of a same-size image before the RGBA -> RGBa conversion: no premultiply round trip (which changes colours
    under partial alpha).  nerf_synth360_ft_dataset.py:531 with the default downSample = 1 is this case.  One axis changing takes the RGBA path."""
    a = image((20, 20), 4, seed=3)
    assert np.any(R.unpremultiply(R.premultiply(a)) != a)          # the round trip would show
    want = pil_resize(a, (20, 20))
    np.testing.assert_array_equal(want, a)
    np.testing.assert_array_equal(R.resize_rgba(a, (20, 20)), want)
    for out in ((10, 20), (20, 10)):
        np.testing.assert_array_equal(R.resize_rgba(a, (out[1], out[0])), pil_resize(a, out))


def test_restatement_equals_pillow_mode_l():
    a = image((37, 53), 1)
    np.testing.assert_array_equal(R.resize(a, (17, 11)), pil_resize(a, (11, 17)))
    a = image((7, 9), 1, seed=1)
    np.testing.assert_array_equal(R.resize(a, (23, 20)), pil_resize(a, (20, 23)))


def test_both_clip_branches_are_reached_and_equal_pillow():
    """A 0 / 255 image: LANCZOS overshoots below 0 and above 255, so the clamp of the horizontal pass decides bytes"""
    a = (np.random.default_rng(5).integers(0, 2, size=(37, 53, 3)) * 255).astype(np.uint8)
    _, b, k = R.coeffs(53, 17)
    sums = R.pass_sums(a, b, k, 1) >> R.PRECISION_BITS
    assert sums.size == 37 * 17 * 3 and (sums < 0).sum() > 0 and (sums > 255).sum() > 0
    np.testing.assert_array_equal(R.resize(a, (17, 11)), pil_resize(a, (11, 17)))


@pytest.mark.parametrize("filt", ["box", "bilinear", "hamming", "bicubic"])
def test_restatement_equals_pillow_other_filters(filt):
    for shape, out in (((37, 53), (11, 17)), ((7, 9), (20, 23))):
        a = image(shape, 3, seed=7)
        np.testing.assert_array_equal(R.resize(a, (out[1], out[0]), filt), pil_resize(a, out, filt))


def _axes():
    pairs = set()
    for (h, w), (H, W) in RGB_SHAPES + RGBA_SHAPES:
        pairs |= {(h, H), (w, W)}
    return sorted(pairs)


@pytest.mark.parametrize("filt", R.FILTERS)
def test_library_coefficient_tables_equal_the_restatement(filt):
    """hnr_resize_coeffs is a host function: ksize, bounds and every coefficient, all shapes of the issue, all five filters"""
    assert _lib.RESIZE_FILTERS[filt] == R.FILTERS.index(filt)
    for n_in, n_out in _axes():
        if filt != "lanczos" and n_in > 200:
            continue                                            # (the large axes once, with the filter the reference uses)
        frames._TABLES.clear()
        ksize, bounds, coef = frames.resize_tables(n_in, n_out, filt)
        rk, rb, rc = R.coeffs(n_in, n_out, filt)
        assert ksize == rk, (n_in, n_out)
        np.testing.assert_array_equal(bounds, rb)
        np.testing.assert_array_equal(coef, rc)
    assert frames.resize_tables(53, 17, filt) is frames.resize_tables(53, 17, filt)       # cached per (in, out, filter)


def test_python_constants_are_the_headers():
    src = open(os.path.join(ROOT, "include", "hnr.h")).read()
    val = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, src).group(1))
    assert (_lib.RESIZE_TILE_W, _lib.RESIZE_TILE_H, _lib.RESIZE_LDS_BUDGET) == (val("HNR_RESIZE_TILE_W"), val("HNR_RESIZE_TILE_H"), val("HNR_RESIZE_LDS_BUDGET"))
    assert _lib.RESIZE_FILTERS == {n: val("HNR_RESIZE_" + n.upper()) for n in R.FILTERS}
    assert _lib.RESIZE_FORMS == {n: val("HNR_RESIZE_" + n.upper()) for n in ("auto", "fused", "two_pass")}


def test_auto_form_follows_the_lds_budget():
    assert frames.resize_form((968, 1296), (640, 480)) == "fused"
    assert frames.resize_form((100, 100), (1, 1)) == "fused"
    assert frames.resize_form((4000, 4000), (8, 8), channels=4) == "two_pass"


def test_scaled_intrinsic_is_the_references_two_lines():
    K0 = np.array([[1170.187988, 0.0, 647.75], [0.0, 1170.187988, 483.75], [0.0, 0.0, 1.0]], dtype=np.float32)       # intrinsic_color-like
    for (w_raw, h_raw), (W, H) in (((1296, 968), (640, 480)), ((53, 37), (17, 11)), ((640, 480), (640, 480)), ((9, 7), (23, 20))):
        want = K0.copy()
        want[0, :] *= (W / w_raw)                                # data/scannet_ft_dataset.py:178-179
        want[1, :] *= (H / h_raw)
        got = frames.scaled_intrinsic(K0, (w_raw, h_raw), (W, H))
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
        assert R.scaled_intrinsic(K0, (w_raw, h_raw), (W, H)).tobytes() == want.tobytes()
        per = frames.scaled_intrinsic(np.stack([K0, 2 * K0]), (w_raw, h_raw), (W, H))
        assert per[0].tobytes() == want.tobytes() and per.shape == (2, 3, 3)
    assert K0[0, 0] == np.float32(1170.187988)                   # the input is not modified


def test_compose_restatement_equals_the_torch_expressions():
    """nerf_synth360_ft_dataset.py:532-536 with ToTensor's division, on all 65 536 (c, a) pairs"""
    c, a = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    rgba = np.stack([c, c[::-1], c.T, a], axis=-1)               # [256,256,4]: every (c, a) pair in channel 0
    img = torch.from_numpy(rgba).permute(2, 0, 1).to(torch.float32).div(255)     # ToTensor: (4, h, w)
    want = dict(white=img[:3] * img[-1:] + (1 - img[-1:]), black=img[:3] * img[-1:], alpha=img[-1], mask=(img[-1] > 0.1).to(torch.float32))
    got = R.compose(rgba)
    for k in ("white", "black"):
        assert got[k].dtype == np.float32 and got[k].tobytes() == want[k].permute(1, 2, 0).contiguous().numpy().tobytes(), k
    for k in ("alpha", "mask"):
        assert got[k].tobytes() == want[k].contiguous().numpy().tobytes(), k


def test_premultiply_restatement_round_trip_properties():
    c, a = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    rgba = np.stack([c, c, c, a], axis=-1)
    pre = R.premultiply(rgba)
    np.testing.assert_array_equal(pre[..., 3], a)
    np.testing.assert_array_equal(pre[a == 255], rgba[a == 255])
    assert not pre[a == 0][:, :3].any()
    want = np.asarray(Image.fromarray(rgba).convert("RGBa"))
    np.testing.assert_array_equal(pre, want)
    np.testing.assert_array_equal(R.unpremultiply(rgba), np.asarray(Image.frombytes("RGBa", (256, 256), rgba.tobytes()).convert("RGBA")))


def test_bad_arguments_return_before_any_gpu_call():
    L = _lib.lib()
    one, null, bad = ctypes.c_void_p(16), None, -1

    def refused(name, rc):
        assert rc == bad, name
        assert name.encode() in L.hnr_last_error(), (name, L.hnr_last_error())

    refused("hnr_resize_coeffs", L.hnr_resize_coeffs(0, 5, 4, null, null, 0))
    refused("hnr_resize_coeffs", L.hnr_resize_coeffs(5, 0, 4, null, null, 0))
    refused("hnr_resize_coeffs", L.hnr_resize_coeffs(5, 5, 5, null, null, 0))               # no sixth filter
    refused("hnr_resize_coeffs", L.hnr_resize_coeffs(5, 5, -1, null, null, 0))
    assert L.hnr_resize_coeffs(1296, 640, 4, null, null, 0) == 15                           # sizing call
    b, c = np.zeros((17, 2), np.int32), np.zeros((17, 21), np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    refused("hnr_resize_coeffs", L.hnr_resize_coeffs(53, 17, 4, p(b), null, 0))             # one table without the other
    refused("hnr_resize_coeffs", L.hnr_resize_coeffs(53, 17, 4, p(b), p(c), 17 * 21 - 1))   # coefficient table too small
    assert L.hnr_resize_coeffs(53, 17, 4, p(b), p(c), 17 * 21) == 21
    rs = [one, 1, 37, 53, 3, one, 11, 17, one, one, 21, one, one, 23, 0, one, 1 << 20, null]
    refused("hnr_resize_u8", L.hnr_resize_u8(*(rs[:4] + [2] + rs[5:])))                     # C = 2
    refused("hnr_resize_u8", L.hnr_resize_u8(*([null] + rs[1:])))
    refused("hnr_resize_u8", L.hnr_resize_u8(*(rs[:5] + [null] + rs[6:])))
    refused("hnr_resize_u8", L.hnr_resize_u8(*(rs[:1] + [0] + rs[2:])))                     # N = 0
    refused("hnr_resize_u8", L.hnr_resize_u8(*(rs[:6] + [0] + rs[7:])))                     # H = 0
    refused("hnr_resize_u8", L.hnr_resize_u8(*(rs[:8] + [null] + rs[9:])))                  # the width changes: its tables are needed
    refused("hnr_resize_u8", L.hnr_resize_u8(*(rs[:13] + [0] + rs[14:])))                   # ksize_v = 0
    refused("hnr_resize_u8", L.hnr_resize_u8(*(rs[:14] + [3] + rs[15:])))                   # form 3
    refused("hnr_resize_u8", L.hnr_resize_u8(*(rs[:14] + [2, null, 0, null])))              # two-pass without scratch
    big = [one, 1, 4000, 4000, 4, one, 8, 8, one, one, 3001, one, one, 3001, 1, one, 1 << 30, null]
    refused("hnr_resize_u8", L.hnr_resize_u8(*big))                                         # fused forced beyond the LDS budget
    assert L.hnr_resize_u8_scratch_bytes(3, 37, 53, 3, 11, 17) == 3 * 37 * 17 * 3
    assert L.hnr_resize_u8_scratch_bytes(3, 37, 53, 3, 37, 17) == 0 and L.hnr_resize_u8_scratch_bytes(3, 37, 53, 2, 11, 17) == -1
    assert L.hnr_resize_u8_form(37, 53, 5, 11, 17, 21, 23) == bad
    refused("hnr_rgba_premultiply", L.hnr_rgba_premultiply(null, one, 5, null))
    refused("hnr_rgba_unpremultiply", L.hnr_rgba_unpremultiply(one, null, 5, null))
    refused("hnr_rgba_unpremultiply", L.hnr_rgba_unpremultiply(one, one, -1, null))
    assert L.hnr_rgba_premultiply(null, null, 0, null) == 0                                 # nothing to do
    refused("hnr_rgba_compose", L.hnr_rgba_compose(one, 5, null, null, null, null, null))   # no output
    refused("hnr_rgba_compose", L.hnr_rgba_compose(null, 5, one, null, null, null, null))


def test_python_layer_rejects_what_it_cannot_run():
    rgb = np.zeros((2, 7, 9, 3), np.uint8)
    with pytest.raises(HnrError, match="GPU"):
        frames.resize_frames(rgb, (5, 4), device="cpu")
    with pytest.raises(HnrError, match="GPU"):
        frames.resize_frames(rgb, (5, 4), out=torch.zeros((2, 4, 5, 3), dtype=torch.uint8))
    with pytest.raises(HnrError, match="uint8"):
        frames.resize_frames(rgb.astype(np.float32), (5, 4), device="cuda")
    with pytest.raises(HnrError, match="C must be"):
        frames.resize_frames(np.zeros((7, 9, 2), np.uint8), (5, 4), device="cuda")
    with pytest.raises(HnrError, match="size"):
        frames.resize_frames(rgb, (0, 4), device="cuda")
    with pytest.raises(HnrError, match="RGBA"):
        frames.resize_frames(rgb, (5, 4), mode="RGBA", device="cuda")
    with pytest.raises(HnrError, match="filter"):
        frames.resize_frames(rgb, (5, 4), filter="nearest", device="cuda")
    with pytest.raises(HnrError, match="form"):
        frames.resize_frames(rgb, (5, 4), form="fast", device="cuda")
    with pytest.raises(HnrError, match="GPU"):
        frames.FrameBank.from_raw(rgb, np.tile(np.eye(4, dtype=np.float32), (2, 1, 1)), np.eye(3), (5, 4), "cpu")
    with pytest.raises(HnrError, match="GPU"):
        frames.compose_rgba(np.zeros((4, 5, 4), np.uint8))
