"""CPU checks of depth supervision (csrc/depth_sup.hip): the NumPy restatement tests/depth_sup_ref.py against fp64 within bounds derived from the
operation counts, the new struct's ctypes layout against the C header, the entry points' argument checks (they return before anything touches a
GPU) and FrameBank's depth arguments.  No GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import depth_sup_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24                 # unit roundoff of fp32


def _lib_loaded():
    from hybridneuralrendering_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib, _lib.lib()


def _case(n, seed, valid="mixed"):
    rng = np.random.default_rng(seed)
    D = rng.uniform(0.2, 6.0, size=n).astype(np.float32)
    gt = (D + rng.normal(0, 0.3, size=n)).astype(np.float32).clip(0.31, 7.9)
    mask = (rng.uniform(size=n) > 0.2).astype(np.int8)
    if valid == "mixed":
        gt[rng.uniform(size=n) < 0.3] = 0.0
    elif valid == "none":
        gt[mask > 0] = 0.0
    else:
        mask[:] = 1
    return D, gt, mask


def test_raw_values_follow_the_uint16_convention():
    """A raw 40000 travels as int16 -25536, reads as 40 m and so as 0 (beyond depth_max); the range ends are inside."""
    raw = np.array([0, 299, 300, 1234, 8000, 8001, 40000, 65535], np.uint16)
    q = lambda v: np.float32(v) / np.float32(1000)
    want = np.array([0, 0, q(300), q(1234), q(8000), 0, 0, 0], np.float32)
    got = R.depth_value(raw)
    assert got.dtype == np.float32 and np.array_equal(got, want) and want[2] == np.float32(0.3) and want[4] == 8.0
    as_i16 = raw.view(np.int16)
    assert as_i16[6] == 40000 - 65536 and as_i16[7] == -1
    assert np.array_equal(R.depth_value(as_i16), got)
    assert R.depth_value(np.array([40000 - 65536], np.int16))[0] == 0.0
    assert R.depth_value(np.array([-25536], np.int16), depth_max=50.0)[0] == np.float32(40.0)       # ... and as 40 m when the range allows it
    # float frames are copied, the range applies, a NaN is no measurement
    f = np.array([0.0, 0.29, 0.3, 2.5, 8.0, 8.5, np.nan], np.float32)
    assert np.array_equal(R.depth_value(f), np.array([0, 0, 0.3, 2.5, 8.0, 0, 0], np.float32))
    assert R.depth_value(np.array([4000], np.uint16), depth_div=4000.0)[0] == 1.0


def test_pixel_rule_against_fp64():
    """Without a depth intrinsic: the truncated pixel.  With one: the fp32 chain has six rounded operations on values below `mag`, so it can differ from
    the fp64 pixel only where the fp64 coordinate lies within 8 u mag of a pixel border; everywhere else the two agree, and both borders occur."""
    rng = np.random.default_rng(0)
    H, W, Hd, Wd = 48, 64, 18, 24
    px, py = rng.integers(0, W, 4000).astype(np.float32), rng.integers(0, H, 4000).astype(np.float32)
    u, v, inside = R.depth_pixels(px, py, H, W)
    assert inside.all() and np.array_equal(u, px.astype(np.int64)) and np.array_equal(v, py.astype(np.int64))
    u, v, inside = R.depth_pixels(np.array([-0.5, -1.0, 63.9, 64.0, np.nan], np.float32), np.zeros(5, np.float32), H, W)
    assert list(inside) == [True, False, True, False, False] and u[0] == 0 and u[2] == 63
    K = np.array([[70.0, 0, 31.5], [0, 70.0, 23.5], [0, 0, 1]], np.float32)
    Kd = np.array([[30.3, 0, 11.7], [0, 29.9, 8.6], [0, 0, 1]], np.float32)
    u, v, inside = R.depth_pixels(px, py, Hd, Wd, K, Kd)
    x64 = ((px.astype(np.float64) + 0.5) - K[0, 2]) / K[0, 0] * Kd[0, 0] + Kd[0, 2] + 0.5
    y64 = ((py.astype(np.float64) + 0.5) - K[1, 2]) / K[1, 1] * Kd[1, 1] + Kd[1, 2] + 0.5
    mag = 2 * max(W, H) + 2
    clear = (np.abs(x64 - np.round(x64)) > 8 * U * mag) & (np.abs(y64 - np.round(y64)) > 8 * U * mag)
    assert clear.mean() > 0.99
    u64, v64 = np.floor(x64).astype(np.int64), np.floor(y64).astype(np.int64)
    in64 = (u64 >= 0) & (u64 < Wd) & (v64 >= 0) & (v64 < Hd)
    assert np.array_equal(inside[clear], in64[clear])
    both = clear & in64
    assert np.array_equal(u[both], u64[both]) and np.array_equal(v[both], v64[both])
    assert 0.2 < in64.mean() < 0.95 and u64.min() < 0 and u64.max() >= Wd               # some rays leave the depth frame on either side
    # the two conventions differ by half a pixel: a colour ray leaves pixel px at px + 0.5, a depth texel u is centred at u.  A depth camera whose
    # principal point is the colour one's minus 0.5 maps every pixel to itself; the colour intrinsic itself puts px + 0.5 on the border of texels
    # px and px + 1 (a tie, decided by the last bit: a depth camera is never calibrated to that)
    Ks = K.copy()
    Ks[0, 2] -= 0.5
    Ks[1, 2] -= 0.5
    u, v, inside = R.depth_pixels(px, py, H, W, K, Ks)
    assert inside.all() and np.array_equal(u, px.astype(np.int64)) and np.array_equal(v, py.astype(np.int64))
    # gt_depth: the looked-up value, 0 outside, a bad row reads row 0
    frames = rng.integers(0, 9000, size=(3, Hd, Wd)).astype(np.uint16)
    g = R.gt_depth(frames, 2, px, py, K, Kd)
    u, v, inside = R.depth_pixels(px, py, Hd, Wd, K, Kd)
    assert np.array_equal(g[inside], R.depth_value(frames[2][v[inside], u[inside]])) and (g[~inside] == 0).all() and (g > 0).any()
    assert np.array_equal(R.gt_depth(frames, 7, px, py, K, Kd), R.gt_depth(frames, 0, px, py, K, Kd))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1025, 3136, 70000])
def test_loss_restatement_against_fp64(n):
    """L within LOSS_REL_BOUND (derived in depth_sup_ref.py) of the fp64 mean; the gradient within 3.1 u relative of the fp64 gradient -- its three
    rounded operations: the difference, the scale's quotient (2 w and float(n) are exact), the product."""
    D, gt, mask = _case(n, n)
    w = 0.1
    out3, g, total = R.depth_loss(D, gt, mask, w, total=np.float32(0.75))
    m = R.loss_mask(gt, mask)
    cnt = int(m.sum())
    L64 = R.depth_loss_fp64(D, gt, mask)
    assert out3.dtype == np.float32 and g.dtype == np.float32 and out3[1] == cnt
    if cnt == 0:
        assert out3[0] == 0 and out3[2] == 0 and not g.any() and total == np.float32(0.75)
        return
    assert abs(float(out3[0]) - L64) <= R.LOSS_REL_BOUND * L64
    assert out3[2] == np.float32(np.float32(w) * out3[0]) and total == np.float32(np.float32(0.75) + out3[2])
    g64 = np.where(m, 2.0 * float(np.float32(w)) / cnt * (D.astype(np.float64) - gt.astype(np.float64)), 0.0)
    assert np.all(np.abs(g - g64) <= 3.1 * U * np.abs(g64)) and np.all(g[~m] == 0) and g[m].any()
    # the fixed order is a sum: any order agrees to fp64 rounding
    sq = np.where(m, ((D - gt) * (D - gt)).astype(np.float64), 0.0)
    assert abs(R.ordered_sum(sq) - sq.sum()) <= n * 2.0 ** -53 * sq.sum()


def test_loss_restatement_edge_patterns():
    for valid in ("none", "all"):
        D, gt, mask = _case(300, 3, valid)
        out3, g, total = R.depth_loss(D, gt, mask, 0.5, total=np.float32(-0.0))
        if valid == "none":
            assert not out3.any() and not g.any() and np.signbit(total)             # the total's bits stay, a -0 included
        else:
            assert out3[1] == 300 and g.all()
    # w_depth = 0: the value is reported, nothing is added, the gradient is zero
    D, gt, mask = _case(100, 4, "all")
    out3, g, total = R.depth_loss(D, gt, mask, 0.0, total=np.float32(1.5))
    assert out3[0] > 0 and out3[2] == 0 and total == np.float32(1.5) and not g.any()


def test_metrics_restatement_against_plain_numpy():
    D, gt, mask = _case(24 * 32, 11)
    D[5] = 0.0
    row = R.depth_metrics(D, gt, mask)
    m = R.loss_mask(gt, mask)
    D64, d64 = D.astype(np.float64)[m], gt.astype(np.float64)[m]
    e = np.abs(D64 - d64)
    with np.errstate(divide="ignore"):
        delta = np.maximum(D64 / d64, d64 / D64)
    want = np.array([m.sum(), e.sum(), (e * e).sum(), (e / d64).sum(), (delta < 1.25).sum()])
    assert row[0] == want[0] and row[4] == want[4] and 0 < row[4] < row[0]
    np.testing.assert_allclose(row[1:4], want[1:4], rtol=1e-12, atol=0)
    from hybridneuralrendering_amd.metrics import derive_depth, DM_NCOLS
    dd = derive_depth(np.stack([row, np.zeros(DM_NCOLS)]))
    assert dd["depth_abs"][0] == row[1] / row[0] and dd["depth_n"][0] == row[0] and np.isnan(dd["depth_abs"][1])
    np.testing.assert_allclose([dd["depth_rmse"][0], dd["depth_absrel"][0], dd["depth_d1"][0]],
                               [np.sqrt(np.mean(e * e)), np.mean(e / d64), np.mean(delta < 1.25)], rtol=1e-12)


def test_depth_bank_struct_has_the_layout_of_the_c_header(tmp_path):
    from hybridneuralrendering_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    cname, cls = "hnr_depth_bank", _lib.DepthBankC
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hnr.h"', 'int main(void) {', '  printf("sizeof %%zu\\n", sizeof(%s));' % cname]
    for fname, _ in cls._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(%s, %s));' % (fname, cname, fname))
    lines += ['  printf("ncols %d\\n", HNR_DM_NCOLS);', '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == ctypes.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(got[fname]) == getattr(cls, fname).offset, fname
    from hybridneuralrendering_amd import metrics
    assert int(got["ncols"]) == metrics.DM_NCOLS == len(metrics.DM)
    # the frame structs this feature must not touch keep their sizes
    assert ctypes.sizeof(_lib.FrameBankC) == 72 and ctypes.sizeof(_lib.FrameBatchOut) == 18 * 8 and ctypes.sizeof(_lib.FrameBatchParams) == 64


def test_entry_points_reject_bad_arguments_without_a_gpu():
    _lib, L = _lib_loaded()
    P = ctypes.c_void_p(4096)               # never dereferenced: every call below fails its checks first
    bank = _lib.DepthBankC(P, None, 0, 3, 24, 32, 1000.0, 0.3, 8.0)
    ok = lambda **kw: _lib.DepthBankC(*[kw.get(n, getattr(bank, n)) for n, _ in _lib.DepthBankC._fields_])
    rays = lambda b, row=P, pix=P, K=None, R=10, out=P: L.hnr_frame_depth_rays(ctypes.byref(b) if b is not None else None, row, pix, K, R, out, None)
    assert rays(None) == -1 and b"NULL" in L.hnr_last_error()
    for kw in (dict(row=None), dict(pix=None), dict(out=None), dict(R=0), dict(R=-5), dict(R=(1 << 26) + 1)):
        assert rays(bank, **kw) == -1, kw
    for kw in (dict(d_depth=None), dict(F=0), dict(Hd=0), dict(Wd=-1), dict(Hd=1 << 14, Wd=1 << 13), dict(depth_div=0.0), dict(depth_div=-1.0),
               dict(depth_div=float("nan")), dict(depth_min=9.0), dict(d_depth_intrinsic=P)):            # (a depth intrinsic without the colour one)
        assert rays(ok(**kw)) == -1, kw
    loss = lambda D=P, gt=P, m=P, R=10, w=0.1, total=None, out3=P, g=None: L.hnr_depth_loss(D, gt, m, R, w, total, out3, g, None, None)
    for kw in (dict(D=None), dict(gt=None), dict(m=None), dict(out3=None), dict(R=0), dict(R=-1), dict(R=(1 << 26) + 1), dict(w=-0.5),
               dict(w=float("nan")), dict(w=float("inf"))):
        assert loss(**kw) == -1, kw
    met = lambda D=P, gt=P, m=P, R=10, row=P: L.hnr_depth_metrics(D, gt, m, R, row, None)
    for kw in (dict(D=None), dict(gt=None), dict(m=None), dict(row=None), dict(R=0), dict(R=-3)):
        assert met(**kw) == -1, kw
    assert b"hnr_depth_metrics" in L.hnr_last_error()


def test_frame_bank_validates_its_depth_arguments_before_any_upload():
    from hybridneuralrendering_amd.frames import FrameBank, HnrError
    import torch
    F, H, W = 3, 24, 32
    img = np.zeros((F, H, W, 3), np.uint8)
    c2w = np.stack([np.eye(4, dtype=np.float32)] * F)
    K = np.array([[30.0, 0, 16], [0, 30.0, 12], [0, 0, 1]], np.float32)
    mk = lambda **kw: FrameBank(img, c2w, K, "cuda:0", **kw)
    good = np.zeros((F, H, W), np.uint16)
    bad = [dict(depth=np.zeros((F, H, W), np.int32)), dict(depth=np.zeros((F, H, W), np.float64)), dict(depth=torch.zeros((F, H, W), dtype=torch.uint8)),
           dict(depth=np.zeros((F + 1, H, W), np.uint16)), dict(depth=np.zeros((F, H, W, 1), np.uint16)), dict(depth=np.zeros((H, W), np.uint16)),
           dict(depth=np.zeros((F, 18, 24), np.uint16)),                                   # another size needs the depth camera's intrinsic
           dict(depth=good, depth_div=0.0), dict(depth=good, depth_div=-1000.0), dict(depth=good, depth_min=9.0, depth_max=8.0),
           dict(depth=good, depth_intrinsic=np.eye(4, dtype=np.float32)), dict(depth=good, depth_intrinsic=np.zeros((F, 3, 3), np.float32)),
           dict(depth_intrinsic=K), dict(depth="depth.png")]
    for kw in bad:
        with pytest.raises(HnrError):
            mk(**kw)
    with pytest.raises(HnrError):
        FrameBank(img, c2w, K, "cpu", depth=good)


def test_step_arguments_are_checked_before_anything_is_queued():
    from hybridneuralrendering_amd.train import _depth_arg, HnrError
    import torch
    rays = torch.zeros((10, 3))
    assert _depth_arg("t", None, 0.0, rays) == (None, 0.0)
    for gt, w in ((None, 0.1), (torch.zeros(10), 0.1), (np.zeros(10, np.float32), 0.1)):          # a weight without depth; CPU tensors
        with pytest.raises(HnrError):
            _depth_arg("t", gt, w, rays)
