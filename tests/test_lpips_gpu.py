"""LPIPS on the device (csrc/lpips.hip) against the restatement of tests/lpips_ref.py.

THE RULE of tests/test_frame_weights_gpu.py (its `rule()` is used as it is): a stage is fed the fp64 restatement's inputs rounded to fp32; its output
must lie within 4 x the maximum error of the fp32 restatement against the fp64 restatement for that output on the same inputs (not below one ulp of
the output's largest magnitude), computed here on the CPU, never from device code.  For the scalar outputs (r_0 .. r_4, d) both sides of the
comparison are the maximum over all test pairs of the net, so one lucky fp32 result cannot tighten the bound.  The preparation is bit-equal.

Shapes (H, W).  vgg: (16, 16) -- a 1x1 last tap; (35, 50) -- taps 35x50, 17x25, 8x12, 4x6, 2x3: odd extents under floor pooling; (19, 70) -- the
convolution's pixel tiles are 8 rows x 32 columns (with 64 channels) and 4 x 32 (with 32): 19 = 2 x 8 + 3 = 4 x 4 + 3 and 70 = 2 x 32 + 6 exceed both
in both directions with a ragged remainder in both; the tap test runs every shape with either tile.
alex: (31, 31) -- a 1x1 last tap; (67, 91) -- taps 16x22, 7x10, 3x4; (75, 63).  Between them: 3-channel first layers, stride 4, 5x5 and 3x3 kernels,
input-channel chunks of 2, 4 and 8, a halo that crosses the image border on every side.  Two pairs per shape: a close pair (noise of a few levels)
and a pair that differs in four pixels only.  Measured ratios: profiles/lpips_tests.txt."""
import functools

import numpy as np
import pytest
import torch

from tests import lpips_ref as LR
from tests.bits import DEV, t
from tests.test_frame_weights_gpu import MARGIN, rule

pytestmark = pytest.mark.gpu

NETS = ("alex", "vgg")
SHAPES = {"vgg": ((16, 16), (35, 50), (19, 70)), "alex": ((31, 31), (67, 91), (75, 63))}
PAIRS = ("ab", "ac")
ROW = ("d", "r0", "r1", "r2", "r3", "r4")
BLACK_SHIFT, BLACK_SCALE = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)            # a second ScalingLayer under which a black byte is exactly 0


@functools.lru_cache(maxsize=None)
def params(net, zero_bias=False):
    return LR.make_params(net, 7 if net == "alex" else 8, zero_bias)


@functools.lru_cache(maxsize=None)
def images(net, si, pair):
    h, w = SHAPES[net][si]
    a, b, c = LR.seeded_images(h, w, 100 + 10 * si + (net == "vgg"))
    return a, (b if pair == "ab" else c)


@functools.lru_cache(maxsize=None)
def run(net, si, pair, dtype):
    """The restatement's whole run on one pair of bytes, computed once and shared: network input, taps, row."""
    a, b = images(net, si, pair)
    with torch.no_grad():
        p = LR.cast(params(net), dtype)
        x = LR.prepare8(a, b, dtype)
        taps = LR.features(net, p, x)
        d, rs = LR.score(p, [f[0:1] for f in taps], [f[1:2] for f in taps])
    return dict(x=x, taps=taps, row=torch.stack([d] + rs))


@functools.lru_cache(maxsize=None)
def model(net, channel_order="bgr"):
    from hybridneuralrendering_amd.perceptual import LPIPS
    return LPIPS(net, channel_order=channel_order).load_pretrained(LR.lpips_state_dict(net, params(net))).to(DEV)


def scalar_rule(got, truth, yard, what):
    """rule() for the six scalars of a row over all pairs: got, truth, yard [pairs, 6]; per column the maxima over the pairs on both sides."""
    got, truth, yard = (np.asarray(a, np.float64) for a in (got, truth, yard))
    assert got.shape == truth.shape == yard.shape and np.isfinite(got).all()
    for c, name in enumerate(ROW):
        floor = float(np.spacing(np.float32(np.abs(truth[:, c]).max())))
        e_hip, e_t = float(np.abs(got[:, c] - truth[:, c]).max()), float(np.abs(yard[:, c] - truth[:, c]).max())
        print("RATIO %s %s: hip %.3e, restatement fp32 %.3e, ulp of max %.3e -> ratio %.2f" % (what, name, e_hip, e_t, floor, e_hip / max(e_t, floor)))
        assert e_hip <= MARGIN * max(e_t, floor), (what, name, e_hip, e_t, floor)


@pytest.mark.parametrize("si", (0, 1, 2))
@pytest.mark.parametrize("net", NETS)
def test_preparation_is_bit_equal(net, si):
    a, b = images(net, si, "ab")
    for order in ("bgr", "rgb"):
        got = model(net, order).prepare8(t(a), t(b))
        want = LR.prepare8(a, b, torch.float32, order)
        assert got.dtype == torch.float32 and torch.equal(got.cpu(), want), order
    m = model(net)
    f0 = torch.from_numpy((np.float32(a) / 255.0 * 2 - 1.0).transpose(2, 0, 1).copy())[None]
    f1 = torch.from_numpy((np.float32(b) / 255.0 * 2 - 1.0).transpose(2, 0, 1).copy())[None]
    got = m.prepare_f32(t(f0), t(f1))
    assert torch.equal(got.cpu(), torch.cat([LR.scaling_layer(f0), LR.scaling_layer(f1)]))
    assert torch.equal(got, model(net, "rgb").prepare8(t(a), t(b)))


@pytest.mark.parametrize("tile", (1, 2))
@pytest.mark.parametrize("si", (0, 1, 2))
@pytest.mark.parametrize("net", NETS)
def test_five_taps_from_the_image(net, si, tile, monkeypatch):
    """tile: the convolution's two tiles (4 rows x 32 columns x 32 channels, 8 x 32 x 64); left alone, the library picks the small one at these sizes.
    Both must give the same bits."""
    monkeypatch.setenv("HNR_LPIPS_CONV_TILE", str(tile))
    x32 = run(net, si, "ab", torch.float64)["x"].float()
    with torch.no_grad():
        truth = LR.features(net, LR.cast(params(net), torch.float64), x32.double())
        yard = LR.features(net, LR.cast(params(net), torch.float32), x32)
    got = model(net).tap_features(t(x32))
    assert [tuple(g.shape) for g in got] == [tuple(f.shape) for f in truth]
    monkeypatch.delenv("HNR_LPIPS_CONV_TILE")
    assert all(torch.equal(a, b) for a, b in zip(got, model(net).tap_features(t(x32))))
    for k in range(5):
        assert float((truth[k] > 0).double().mean()) > 0.1
        rule(got[k], truth[k], yard[k], "%s %s tap %d %s" % (net, SHAPES[net][si], k, tuple(truth[k].shape[1:])))


@pytest.mark.parametrize("net", NETS)
def test_scores_from_recorded_fp64_taps(net):
    got, truth, yard = [], [], []
    p64, p32 = LR.cast(params(net), torch.float64), LR.cast(params(net), torch.float32)
    for si, (h, w) in enumerate(SHAPES[net]):
        for pair in PAIRS:
            taps32 = [f.float() for f in run(net, si, pair, torch.float64)["taps"]]
            with torch.no_grad():
                d, rs = LR.score(p64, [f[0:1].double() for f in taps32], [f[1:2].double() for f in taps32])
                truth.append(torch.stack([d] + rs).numpy())
                d, rs = LR.score(p32, [f[0:1] for f in taps32], [f[1:2] for f in taps32])
                yard.append(torch.stack([d] + rs).numpy())
            row = model(net).score([t(f) for f in taps32], h, w)
            assert row.dtype == torch.float64 and tuple(row.shape) == (1, 6)
            got.append(row[0].cpu().numpy())
    scalar_rule(got, truth, yard, "%s score" % net)


@pytest.mark.parametrize("net", NETS)
def test_whole_chain(net):
    got, truth, yard = [], [], []
    for si in range(3):
        for pair in PAIRS:
            a, b = images(net, si, pair)
            got.append(model(net).pair8(t(a), t(b))[0].cpu().numpy())
            truth.append(run(net, si, pair, torch.float64)["row"].numpy())
            yard.append(run(net, si, pair, torch.float32)["row"].numpy())
    assert min(r[0] for r in truth) > 0
    scalar_rule(got, truth, yard, "%s pair8" % net)


@pytest.mark.parametrize("net", NETS)
def test_identical_images_give_a_row_of_exact_zeros(net):
    a, _ = images(net, 1, "ab")
    out = torch.full((2, 6), 7.0, dtype=torch.float64, device=DEV)
    model(net).pair8(t(a), t(a), out=out, row=1)
    assert out.cpu().tolist() == [[7.0] * 6, [0.0] * 6]


@pytest.mark.parametrize("net", NETS)
def test_two_runs_are_bit_identical(net):
    a, b = images(net, 2, "ab")
    m = model(net)
    r1 = m.pair8(t(a), t(b)).clone()
    m.scratch(*SHAPES[net][2]).fill_(255)                             # the second run does not start from the same bytes (NaNs)
    r2 = m.pair8(t(a), t(b))
    assert torch.equal(r1, r2) and float(r1[0, 0]) > 0


@pytest.mark.parametrize("net", NETS)
def test_black_region_with_all_zero_features_stays_finite(net):
    """A second weight set: zero biases and a ScalingLayer under which a black byte is exactly 0 -- inside a black region every feature of every tap is
    zero, the norm is 0 and the pixel must contribute 0 / (0 + 1e-10) = 0."""
    from hybridneuralrendering_amd.perceptual import LPIPS
    h, w = SHAPES[net][1]
    a, b = (im.copy() for im in images(net, 1, "ab"))
    a[:, : (2 * w) // 3] = 0
    b[:, : (2 * w) // 3] = 0
    p = params(net, True)
    m = LPIPS(net).load_pretrained(LR.lpips_state_dict(net, p, BLACK_SHIFT, BLACK_SCALE)).to(DEV)
    with torch.no_grad():
        truth = LR.pair8(net, p, a, b, torch.float64, shift=BLACK_SHIFT, scale=BLACK_SCALE)
        yard = LR.pair8(net, p, a, b, torch.float32, shift=BLACK_SHIFT, scale=BLACK_SCALE)
        taps = LR.features(net, LR.cast(p, torch.float64), LR.prepare8(a, b, torch.float64, shift=BLACK_SHIFT, scale=BLACK_SCALE))
    assert all(bool((f.abs().sum(1) == 0).any()) for f in taps[:2]) and float(truth[0]) > 0
    got = m.pair8(t(a), t(b))[0].cpu().numpy()
    scalar_rule(got[None], truth.numpy()[None], yard.numpy()[None], "%s black region" % net)


@pytest.mark.parametrize("order", ("bgr", "rgb"))
@pytest.mark.parametrize("net", NETS)
def test_forward_equals_pair8_on_the_same_bytes(net, order):
    a, b = images(net, 1, "ab")
    m = model(net, order)
    f = lambda im: t((np.float32(im if order == "rgb" else im[..., ::-1]) / 255.0 * 2 - 1.0).transpose(2, 0, 1).copy())[None]
    d = m(f(a), f(b))
    assert tuple(d.shape) == (1, 1, 1, 1) and d.dtype == torch.float32 and d.is_cuda
    assert torch.equal(d.reshape(()), m.pair8(t(a), t(b))[0, 0].float())
    g = lambda im: t((np.float32(im if order == "rgb" else im[..., ::-1]) / np.float32(255.0)).transpose(2, 0, 1).copy())[None]
    d01 = m(g(a), g(b), normalize=True)                              # [0, 1] inputs: 2 x - 1 here, another rounding than evaluate.py's
    assert abs(float(d01) - float(d)) <= 1e-5 * float(d)


def _lpips_dict():
    return {"lpips": model("alex"), "vgglpips": model("vgg")}


def test_evaluator_rows_equal_single_calls(tmp_path):
    from hybridneuralrendering_amd.metrics import TestSetEvaluator, frame_metrics
    from tests.test_metrics_gpu import _three_frames
    frames = _three_frames()
    for save in (False, True):
        ev = TestSetEvaluator(4, device=DEV, save_images=save, lpips=_lpips_dict())
        plain = TestSetEvaluator(4, device=DEV, save_images=save)
        for out, frame, _ in frames:
            ev.add(out, frame)
            plain.add(out, frame)
        assert torch.equal(ev.table, plain.table)
        for k, (out, frame, _) in enumerate(frames):
            h, w = frame["h"], frame["w"]
            a8, b8 = (torch.zeros((h, w, 3), dtype=torch.uint8, device=DEV) for _ in range(2))
            frame_metrics(out, frame, images8=(a8, b8))
            for key, m in _lpips_dict().items():
                assert torch.equal(m.pair8(a8, b8)[0], ev.lpips_tables[key][k]), (key, k)
        assert all(float(tb[3].abs().max()) == 0 for tb in ev.lpips_tables.values())
    res = ev.write(str(tmp_path))
    assert [l.split(":")[0] for l in open(tmp_path / "scores.txt").read().splitlines()] == ["psnr", "ssim", "lpips", "vgglpips", "rmse"]
    assert len(res["lpips"]) == 3 and (res["vgglpips"] > 0).all() and res["mean"]["lpips"] == float(np.mean(res["lpips"]))
    np.testing.assert_array_equal(np.loadtxt(tmp_path / "lpips.txt"), res["lpips"])


def test_add_with_lpips_performs_no_host_synchronisation():
    from hybridneuralrendering_amd.metrics import TestSetEvaluator
    from tests.test_metrics_gpu import _three_frames
    frames = _three_frames()
    ev = TestSetEvaluator(3, device=DEV, lpips=_lpips_dict())
    ev.add(*frames[0][:2])                                   # (first call: the library loads, the weights are packed, the scratch is allocated)
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception as e:                                   # pragma: no cover
        pytest.skip("torch.cuda.set_sync_debug_mode is not supported by this torch build on ROCm: %r" % (e,))
    try:
        if torch.cuda.get_sync_debug_mode() != 2:
            pytest.skip("torch.cuda.set_sync_debug_mode('error') did not take effect in this torch build on ROCm")
        for out, frame, _ in frames[1:]:
            ev.add(out, frame)
        with pytest.raises(RuntimeError):
            ev.lpips_tables["lpips"][0, 0].item()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    s = ev.summary()
    assert len(s["lpips"]) == 3 and len(s["vgglpips"]) == 3


def test_evaluate_frames_with_lpips_leaves_frame_and_columns_bit_equal():
    from hybridneuralrendering_amd.driver import evaluate_frames
    from tests.test_metrics_gpu import _golden_frame
    z, frame, cloud, rnd, gt, pix = _golden_frame(11)
    seen, seen_l = [], []
    ev0 = evaluate_frames(rnd, cloud, [frame, frame], on_frame=lambda i, o: seen.append(o))
    ev1 = evaluate_frames(rnd, cloud, [frame, frame], on_frame=lambda i, o: seen_l.append(o), lpips=_lpips_dict())
    for o, ol in zip(seen, seen_l):
        assert sorted(o) == sorted(ol)
        for k in o:
            assert torch.equal(o[k], ol[k]), k
    assert ev0.table.cpu().numpy().tobytes() == ev1.table.cpu().numpy().tobytes() and ev1.n == 2
    s = ev1.summary()
    assert (s["lpips"] > 0).all() and (s["vgglpips"] > 0).all() and s["lpips"][0] == s["lpips"][1]
    assert "lpips" not in ev0.summary()
