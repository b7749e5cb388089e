"""GPU checks of the device resize (csrc/resize.hip): hnr_resize_u8 in both forms against PIL.Image.resize itself, byte for byte -- the shapes of
tests/test_resize.py with C = 1, 3, 4, output sizes one past the tile, a source view at an odd byte offset, batches into rows of a larger bank --;
RGBA mode against Pillow; premultiply / un-premultiply / compose on all 65 536 (c, a) pairs; FrameBank.from_raw / ingest at the level of the dataset
item.  Every comparison is an equality of bytes or bits.  Pillow results are computed once per shape and shared."""
import ctypes
import functools

import numpy as np
import pytest
import torch
from PIL import Image

from hybridneuralrendering_amd import _lib, frames
from hybridneuralrendering_amd._lib import HnrError

from tests import resize_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TW, TH = _lib.RESIZE_TILE_W, _lib.RESIZE_TILE_H
PIL_FILTER = dict(box=Image.BOX, bilinear=Image.BILINEAR, hamming=Image.HAMMING, bicubic=Image.BICUBIC, lanczos=Image.LANCZOS)
PIL_MODE = {1: "L", 3: "RGB", 4: "CMYK"}                         # CMYK: four independent 8-bit channels (RGBA mode is tested on its own)
SMALL = [((37, 53), (11, 17)), ((7, 9), (20, 23)), ((16, 16), (16, 5)), ((5, 40), (9, 40)), ((100, 100), (1, 1)), ((3, 3), (7, 2)), ((800, 800), (400, 400))]
# one past the tile in each direction, reducing and enlarging; sizes follow the tile constants
EDGE = [((2 * (TH + 1) + 3, 2 * (TW + 1) + 1), (TH + 1, TW + 1)), (((TH + 1) // 2 + 1, (TW + 1) // 2 + 1), (TH + 1, TW + 1)),
        ((3 * TH + 2, TW + 1), (TH + 1, TW + 1)), ((TH + 1, 3 * TW + 2), (TH + 1, TW + 1))]


@functools.lru_cache(maxsize=None)
def case(shape, out, C, filt="lanczos", seed=0, binary=False):
    """(raw [h,w,C] uint8, what Pillow makes of it [H,W,C]) -- computed once, never modified"""
    rng = np.random.default_rng(seed + 1000 * C + shape[0])
    a = (rng.integers(0, 2, size=shape + (C,)) * 255).astype(np.uint8) if binary else rng.integers(0, 256, size=shape + (C,), dtype=np.uint8)
    im = Image.frombytes(PIL_MODE[C], (shape[1], shape[0]), a.tobytes())
    want = np.frombuffer(im.resize((out[1], out[0]), PIL_FILTER[filt]).tobytes(), np.uint8).reshape(out + (C,))
    a.setflags(write=False)
    return a, want


def run(a, out, form, filt="lanczos", **kw):
    return frames.resize_frames(a, (out[1], out[0]), filter=filt, form=form, device=DEV, **kw).cpu().numpy()


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("shape,out", SMALL + EDGE)
def test_both_forms_equal_pillow(shape, out, C):
    a, want = case(shape, out, C)
    fused, two = run(a, out, "fused"), run(a, out, "two_pass")
    np.testing.assert_array_equal(fused, want)
    np.testing.assert_array_equal(two, want)
    np.testing.assert_array_equal(run(a, out, "auto"), want)


def test_scannet_shape_once():
    """(968,1296) -> (480,640): both forms, and what "auto" takes there"""
    a, want = case((968, 1296), (480, 640), 3)
    assert frames.resize_form((968, 1296), (640, 480)) == "fused"
    np.testing.assert_array_equal(run(a, (480, 640), "auto"), want)
    np.testing.assert_array_equal(run(a, (480, 640), "two_pass"), want)


def test_clip_branches_on_a_binary_image():
    a, want = case((37, 53), (11, 17), 3, binary=True)
    _, b, k = R.coeffs(53, 17)
    sums = R.pass_sums(a, b, k, 1) >> R.PRECISION_BITS
    assert (sums < 0).any() and (sums > 255).any()
    for form in ("fused", "two_pass"):
        np.testing.assert_array_equal(run(a, (11, 17), form), want)


@pytest.mark.parametrize("filt", ["box", "bilinear", "hamming", "bicubic"])
def test_other_filters_equal_pillow(filt):
    for shape, out in (((37, 53), (11, 17)), ((7, 9), (20, 23))):
        a, want = case(shape, out, 3, filt=filt)
        for form in ("fused", "two_pass"):
            np.testing.assert_array_equal(run(a, out, form, filt=filt), want)


@pytest.mark.parametrize("C", [1, 3, 4])
def test_source_view_at_an_odd_byte_offset(C):
    shape, out = EDGE[0]
    a, want = case(shape, out, C)
    for off in (1, 3):
        buf = torch.zeros((a.size + 8,), dtype=torch.uint8, device=DEV)
        buf[off:off + a.size] = torch.from_numpy(a.copy()).reshape(-1).to(DEV)
        view = buf[off:off + a.size].view(shape + (C,))
        assert view.data_ptr() % 2 == 1
        for form in ("fused", "two_pass"):
            np.testing.assert_array_equal(frames.resize_frames(view, (out[1], out[0]), form=form).cpu().numpy(), want)


@pytest.mark.parametrize("form", ["fused", "two_pass"])
def test_batch_into_rows_of_a_larger_bank(form):
    shape, out, C = (37, 53), (11, 17), 3
    raws = [case(shape, out, C, seed=s) for s in (0, 1, 2)]
    raw = np.stack([r[0] for r in raws])
    n = out[0] * out[1] * C
    buf = torch.full((5 * n + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    bank = buf[:5 * n].view((5,) + out + (C,))
    got = frames.resize_frames(raw, (out[1], out[0]), out=bank[1:4], form=form)
    assert got.data_ptr() == bank[1].data_ptr()
    host = buf.cpu().numpy()
    assert (host[:n] == 0xA5).all() and (host[4 * n:] == 0xA5).all()                      # rows 0 and 4 and the strip behind the bank
    first = host[n:4 * n].reshape((3,) + out + (C,)).copy()
    for i, (a, want) in enumerate(raws):
        np.testing.assert_array_equal(first[i], want)
        np.testing.assert_array_equal(run(a, out, form), want)                            # N = 1 gives the frame's bytes
    frames.resize_frames(raw, (out[1], out[0]), out=bank[1:4], form=form)
    np.testing.assert_array_equal(buf.cpu().numpy(), host)                                # two runs, the same bits


def smallest_two_pass_square():
    """the smallest n for which (n, n) -> (1, 1) with four channels no longer fits the fused form's LDS budget"""
    n = 2
    while frames.resize_form((n, n), (1, 1), channels=4) == "fused":
        n += 1
    return n


def test_auto_picks_the_form_by_the_lds_budget():
    n = smallest_two_pass_square()
    assert 16 < n < 512
    L = _lib.lib()
    for m, form in ((n - 1, "fused"), (n, "two_pass")):
        assert frames.resize_form((m, m), (1, 1), channels=4) == form
        a, want = case((m, m), (1, 1), 4)
        np.testing.assert_array_equal(run(a, (1, 1), "auto"), want)
        np.testing.assert_array_equal(run(a, (1, 1), "two_pass"), want)
    with pytest.raises(HnrError, match="LDS"):
        run(case((n, n), (1, 1), 4)[0], (1, 1), "fused")
    np.testing.assert_array_equal(run(case((n - 1, n - 1), (1, 1), 4)[0], (1, 1), "fused"), case((n - 1, n - 1), (1, 1), 4)[1])
    # "auto" at the C level took the two-pass form: it asks for the scratch the fused form never touches
    kh = frames.resize_tables(n, 1)[0]
    one = ctypes.c_void_p(16)
    assert L.hnr_resize_u8(one, 1, n, n, 4, one, 1, 1, one, one, kh, one, one, kh, 0, None, 0, None) == -1 and b"scratch" in L.hnr_last_error()


@functools.lru_cache(maxsize=None)
def rgba_case(shape, out):
    a = np.random.default_rng(shape[0]).integers(0, 256, size=shape + (4,), dtype=np.uint8)
    a[: shape[0] // 3, :, 3] = 255                               # opaque and empty regions as well as every alpha in between
    a[-(shape[0] // 4):, :, 3] = 0
    want = np.asarray(Image.fromarray(a).resize((out[1], out[0]), Image.LANCZOS))
    a.setflags(write=False)
    return a, want


@pytest.mark.parametrize("shape,out", [((800, 800), (400, 400)), ((37, 53), (11, 17)), ((7, 9), (20, 23))])
def test_rgba_mode_equals_pillow(shape, out):
    a, want = rgba_case(shape, out)
    assert Image.fromarray(a).mode == "RGBA"
    forms = ("auto",) if shape[0] > 100 else ("fused", "two_pass")
    for form in forms:
        np.testing.assert_array_equal(run(a, out, form, mode="RGBA"), want)
    dev = torch.from_numpy(a.copy()).to(DEV)                     # a device input is not modified by the premultiply
    np.testing.assert_array_equal(frames.resize_frames(dev, (out[1], out[0]), mode="RGBA").cpu().numpy(), want)
    np.testing.assert_array_equal(dev.cpu().numpy(), a)


def test_same_size_rgba_is_a_copy_as_pillows():
    """Pillow copies a same-size image before it converts RGBA -> RGBa (the synthetic set's default 800 x 800 -> 800 x 800); one changing axis
    takes the premultiplied path"""
    a = np.random.default_rng(3).integers(0, 256, size=(20, 20, 4), dtype=np.uint8)
    assert np.any(R.unpremultiply(R.premultiply(a)) != a)
    for out in ((20, 20), (10, 20), (20, 10)):
        want = np.asarray(Image.fromarray(a).resize((out[1], out[0]), Image.LANCZOS))
        for form in ("auto", "fused", "two_pass"):
            np.testing.assert_array_equal(run(a, out, form, mode="RGBA"), want)
    np.testing.assert_array_equal(run(a, (20, 20), "auto", mode="RGBA"), a)
    batch = np.stack([a, a[::-1].copy()])
    np.testing.assert_array_equal(run(batch, (20, 20), "auto", mode="RGBA"), batch)


def all_pairs():
    c, a = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    return np.ascontiguousarray(np.stack([c, c[::-1], c.T, a], axis=-1))         # [256,256,4]: channel 0 x alpha is every (c, a) pair


def test_premultiply_and_unpremultiply_on_all_pairs():
    L, p = _lib.lib(), _lib.ptr
    rgba = all_pairs()
    n = 256 * 256
    for off in (0, 1):                                           # aligned and at an odd byte
        buf = torch.zeros((4 * n + 8,), dtype=torch.uint8, device=DEV)
        src = buf[off:off + 4 * n]
        src.copy_(torch.from_numpy(rgba).reshape(-1))
        dst = torch.full((4 * n + 16,), 0x5A, dtype=torch.uint8, device=DEV)
        _lib.check(L.hnr_rgba_premultiply(p(src), p(dst[8:8 + 4 * n]), n, _lib.stream()), "hnr_rgba_premultiply")
        got = dst.cpu().numpy()
        np.testing.assert_array_equal(got[8:8 + 4 * n].reshape(256, 256, 4), R.premultiply(rgba))
        assert (got[:8] == 0x5A).all() and (got[8 + 4 * n:] == 0x5A).all()
        dst.fill_(0x5A)
        _lib.check(L.hnr_rgba_unpremultiply(p(src), p(dst[8:8 + 4 * n]), n, _lib.stream()), "hnr_rgba_unpremultiply")
        got = dst.cpu().numpy()
        np.testing.assert_array_equal(got[8:8 + 4 * n].reshape(256, 256, 4), R.unpremultiply(rgba))
        assert (got[:8] == 0x5A).all() and (got[8 + 4 * n:] == 0x5A).all()
        _lib.check(L.hnr_rgba_premultiply(p(src), p(src), n, _lib.stream()), "hnr_rgba_premultiply")      # in place
        np.testing.assert_array_equal(src.cpu().numpy().reshape(256, 256, 4), R.premultiply(rgba))


def test_compose_on_all_pairs_subsets_and_sentinels():
    L, p = _lib.lib(), _lib.ptr
    rgba = all_pairs()
    n = 256 * 256
    img = torch.from_numpy(rgba).permute(2, 0, 1).to(torch.float32).div(255)                 # ToTensor, then nerf_synth360_ft_dataset.py:533-536 on the CPU
    want = dict(white=(img[:3] * img[-1:] + (1 - img[-1:])).permute(1, 2, 0).contiguous().numpy(), black=(img[:3] * img[-1:]).permute(1, 2, 0).contiguous().numpy(),
                alpha=img[-1].contiguous().numpy(), mask=(img[-1] > 0.1).numpy().astype(np.float32))
    src = torch.from_numpy(rgba).to(DEV)
    got = frames.compose_rgba(src, white=True, black=True, alpha=True, mask=True)
    for k, v in want.items():
        assert got[k].dtype == torch.float32 and got[k].cpu().numpy().tobytes() == v.tobytes(), k
        assert R.compose(rgba)[k].tobytes() == v.tobytes(), k
    one = frames.compose_rgba(src[None, 3:5])                    # [N,H,W,4] -> the defaults: white and alpha, with the frame dimension
    assert sorted(one) == ["alpha", "white"] and tuple(one["white"].shape) == (1, 2, 256, 3) and tuple(one["alpha"].shape) == (1, 2, 256)
    assert one["white"].cpu().numpy().tobytes() == want["white"][3:5].tobytes()
    # subsets at the C level: an output that is not asked for is not written, nothing is written outside the ones that are
    size = dict(white=3 * n, black=3 * n, alpha=n, mask=n)
    for subset in (("alpha",), ("white", "mask"), ("black",)):
        bufs = {k: torch.full((size[k] + 32,), -7.0, dtype=torch.float32, device=DEV) for k in size}
        args = [p(bufs[k][16:16 + size[k]]) if k in subset else None for k in ("white", "black", "alpha", "mask")]
        _lib.check(L.hnr_rgba_compose(p(src), n, *args, _lib.stream()), "hnr_rgba_compose")
        for k in size:
            h = bufs[k].cpu().numpy()
            assert (h[:16] == -7.0).all() and (h[16 + size[k]:] == -7.0).all(), (subset, k)
            if k in subset:
                assert h[16:16 + size[k]].tobytes() == want[k].tobytes(), (subset, k)
            else:
                assert (h == -7.0).all(), (subset, k)


def poses(F):
    c2w = np.tile(np.eye(4, dtype=np.float32), (F, 1, 1))
    c2w[:, :3, 3] = np.random.default_rng(3).uniform(-1, 1, size=(F, 3)).astype(np.float32)
    return c2w


def test_bank_from_raw_gives_the_items_of_the_pillow_bank():
    F, shape, out, V = 6, (37, 53), (11, 17), 2
    raw = np.stack([case(shape, out, 3, seed=s)[0] for s in range(F)])
    pil = np.stack([case(shape, out, 3, seed=s)[1] for s in range(F)])
    K_raw = np.array([[57.76, 0.0, 26.1], [0.0, 57.87, 18.3], [0.0, 0.0, 1.0]], dtype=np.float32)
    K_ref = K_raw.copy()
    K_ref[0, :] *= (out[1] / shape[1])                           # data/scannet_ft_dataset.py:178-179
    K_ref[1, :] *= (out[0] / shape[0])
    c2w = poses(F)
    table = frames.nearest_by_id(np.arange(F), np.arange(F), V, True)
    a = frames.FrameBank.from_raw(raw, c2w, K_raw, (out[1], out[0]), DEV, chunk=4).set_nearest(table)
    b = frames.FrameBank(pil, c2w, K_ref, DEV).set_nearest(table)
    assert a.images.dtype == torch.uint8 and torch.equal(a.images, b.images) and torch.equal(a.intrinsic, b.intrinsic)
    lst = frames.FrameBank.from_raw([torch.from_numpy(r.copy()) for r in raw], c2w, K_raw, (out[1], out[0]), DEV, chunk=1, form="two_pass")
    assert torch.equal(lst.images, b.images)
    sa, sb = (frames.BatchSampler(x, "random", size=4, near=0.1, far=8.0) for x in (a, b))
    for row in (0, 3, F - 1):
        ia, ib = sa.item(row), sb.item(row)
        assert sorted(ia) == sorted(ib)
        for k, v in ib.items():
            if isinstance(v, torch.Tensor):
                assert ia[k].dtype == v.dtype and ia[k].shape == v.shape and torch.equal(ia[k].view(torch.uint8), v.view(torch.uint8)), k
            else:
                assert ia[k] == v, k


def test_ingest_replaces_the_rows_it_is_given_only():
    F, shape, out = 5, (37, 53), (11, 17)
    pil = np.stack([case(shape, out, 3, seed=s)[1] for s in range(F)])
    bank = frames.FrameBank(pil, poses(F), np.eye(3, dtype=np.float32), DEV)
    new, want = case(shape, out, 3, seed=11)
    bank.ingest(2, new)
    got = bank.images.cpu().numpy()
    np.testing.assert_array_equal(got[2], want)
    np.testing.assert_array_equal(np.delete(got, 2, axis=0), np.delete(pil, 2, axis=0))
    two = np.stack([case(shape, out, 3, seed=s)[0] for s in (12, 13)])
    bank.ingest([4, 0], two)                                     # rows in any order
    got = bank.images.cpu().numpy()
    np.testing.assert_array_equal(got[4], case(shape, out, 3, seed=12)[1])
    np.testing.assert_array_equal(got[0], case(shape, out, 3, seed=13)[1])
    np.testing.assert_array_equal(got[[1, 3]], pil[[1, 3]])
    with pytest.raises(HnrError):
        bank.ingest(5, new)
    with pytest.raises(HnrError):
        bank.ingest([], np.zeros((0,) + shape + (3,), np.uint8))
    with pytest.raises(HnrError):
        frames.FrameBank(pil.astype(np.float32) / 255, poses(F), np.eye(3, dtype=np.float32), DEV).ingest(0, new)
