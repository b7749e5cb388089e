"""LPIPS without a GPU: the restatement tests/lpips_ref.py against an independent nn.Sequential formulation, its invariances, the weight loader, the
argument checks of the C ABI and of the Python layer, and the evaluator's files."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
from torch import nn

from tests import lpips_ref as LR

NETS = ("alex", "vgg")
SMALL = {"alex": (67, 91), "vgg": (35, 50)}


@functools.lru_cache(maxsize=None)
def params(net, zero_bias=False):
    return LR.make_params(net, 7 if net == "alex" else 8, zero_bias)


def sequential(net, p, dtype):
    """torchvision's `features` layout: Conv2d / ReLU / MaxPool2d at torchvision's indices, cut into lpips' five slices."""
    layers, convs, pools = [], {c[0]: c for c in LR.CONVS[net]}, {}
    if net == "alex":
        pools = {2: 3, 5: 3}
        n = 12
    else:
        pools = {4: 2, 9: 2, 16: 2, 23: 2}
        n = 30
    i = 0
    while i < n:
        if i in convs:
            _, cin, cout, k, s, pad = convs[i]
            conv = nn.Conv2d(cin, cout, k, stride=s, padding=pad).to(dtype)
            with torch.no_grad():
                conv.weight.copy_(p["features.%d.weight" % i])
                conv.bias.copy_(p["features.%d.bias" % i])
            layers += [conv, nn.ReLU()]
            i += 2
        else:
            assert i in pools, i
            layers.append(nn.MaxPool2d(pools[i], 2))
            i += 1
    seq = nn.Sequential(*layers)
    ends = (0,) + LR.SLICE_ENDS[net]
    return [seq[ends[j]:ends[j + 1]] for j in range(5)]


@pytest.mark.parametrize("net", NETS)
def test_restatement_equals_the_sliced_sequential_formulation(net):
    h, w = SMALL[net]
    a, b, _ = LR.seeded_images(h, w, 1)
    p64 = LR.cast(params(net), torch.float64)
    x = LR.prepare8(a, b, torch.float64)
    taps = LR.features(net, p64, x)
    with torch.no_grad():
        y, other = x, []
        for s in sequential(net, p64, torch.float64):
            y = s(y)
            other.append(y)
    for k in range(5):
        assert taps[k].shape == other[k].shape and taps[k].shape[1] == LR.TAP_CHANNELS[net][k]
        assert float((taps[k] - other[k]).abs().max()) <= 1e-12 * float(other[k].abs().max())
        live = float((taps[k].amax(dim=(0, 2, 3)) > 0).double().mean())
        assert torch.isfinite(taps[k]).all() and live > 0.25, (k, live)
        assert 1e-3 < float(taps[k].abs().max()) < 1e3
    # the score, written the other way: per pixel and channel, in numpy
    d, rs = LR.score(p64, [t[0:1] for t in taps], [t[1:2] for t in taps])
    tot = 0.0
    for k in range(5):
        f0, f1 = other[k][0].numpy(), other[k][1].numpy()
        g0, g1 = f0 / (np.sqrt((f0 * f0).sum(0)) + 1e-10), f1 / (np.sqrt((f1 * f1).sum(0)) + 1e-10)
        r = float((p64["lin%d.model.1.weight" % k].numpy().reshape(-1, 1, 1) * (g0 - g1) ** 2).sum(0).mean())
        assert abs(r - float(rs[k])) <= 1e-12 * abs(r) and r > 0
        tot += r
    assert abs(tot - float(d)) <= 1e-12 * tot


def test_tap_shapes_of_the_issue():
    for net, hw, want in (("vgg", (16, 16), [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]), ("vgg", (35, 50), [(35, 50), (17, 25), (8, 12), (4, 6), (2, 3)]),
                          ("alex", (31, 31), [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]), ("alex", (67, 91), [(16, 22), (7, 10), (3, 4), (3, 4), (3, 4)])):
        p = LR.cast(params(net), torch.float32)
        taps = LR.features(net, p, torch.zeros((1, 3) + hw))
        assert [tuple(t.shape[2:]) for t in taps] == want


@pytest.mark.parametrize("net", NETS)
def test_identical_images_give_exactly_zero_and_d_is_symmetric(net):
    h, w = SMALL[net]
    a, b, _ = LR.seeded_images(h, w, 2)
    for dt in (torch.float32, torch.float64):
        assert LR.pair8(net, params(net), a, a, dt).tolist() == [0.0] * 6
        ab, ba = LR.pair8(net, params(net), a, b, dt), LR.pair8(net, params(net), b, a, dt)
        assert float(ab[0]) > 0
        assert float((ab - ba).abs().max()) <= (1e-6 if dt == torch.float32 else 1e-14) * float(ab[0])


@pytest.mark.parametrize("net", NETS)
def test_bgr_default_equals_rgb_on_reversed_inputs_and_reversed_first_layer(net):
    h, w = SMALL[net]
    a, b, _ = LR.seeded_images(h, w, 3)
    p = LR.cast(params(net), torch.float64)
    first = "features.0.weight"
    q = dict(p)
    q[first] = p[first].flip(1)
    x_bgr = LR.prepare8(a, b, torch.float64, "bgr")
    x_rgb = LR.prepare8(a[..., ::-1], b[..., ::-1], torch.float64, "rgb")
    assert torch.equal(x_bgr, x_rgb)                                # reversing the bytes = the bgr option
    # reversed channels with reversed shift, scale and first-layer weights: the same number
    x_rev = LR.prepare8(a, b, torch.float64, "rgb", shift=LR.SHIFT[::-1], scale=LR.SCALE[::-1]).flip(1)
    assert torch.equal(x_rev, x_bgr)
    r1 = LR.lpips_from_input(net, p, x_bgr)
    r2 = LR.lpips_from_input(net, q, x_bgr.flip(1))
    assert float((r1 - r2).abs().max()) <= 1e-13 * float(r1[0])
    assert abs(float(r1[0]) - float(LR.pair8(net, params(net), a, b, torch.float64, "rgb")[0])) > 1e-6 * float(r1[0])    # the order matters


def test_preparation_table_equals_the_fp32_expression_for_every_byte():
    from hybridneuralrendering_amd import perceptual
    table = perceptual.prep_table()
    assert table.dtype == np.float32 and table.shape == (3, 256)
    b = np.arange(256, dtype=np.uint8)
    for c in range(3):
        x = np.float32(b) / 255.0                                    # run/evaluate.py, line by line
        x = x * 2 - 1.0
        assert x.dtype == np.float32
        y = (torch.from_numpy(x).reshape(1, 1, 1, -1) - torch.tensor(LR.SHIFT[c])) / torch.tensor(LR.SCALE[c])
        assert y.dtype == torch.float32
        np.testing.assert_array_equal(table[c], y.reshape(-1).numpy())
    np.testing.assert_array_equal(table, LR.byte_values(torch.float32).numpy())


@pytest.mark.parametrize("net", NETS)
def test_loader_packs_both_key_layouts_identically(net):
    from hybridneuralrendering_amd.perceptual import LPIPS
    from hybridneuralrendering_amd._lib import HnrError
    p = params(net)
    whole = LR.lpips_state_dict(net, p)
    bb = dict(LR.backbone(p))
    bb["classifier.0.weight"] = torch.zeros(3, 3)
    a = LPIPS(net).load_pretrained(whole).pack_host()
    b = LPIPS(net).load_pretrained(bb, lin=LR.lin_file(p)).pack_host()
    assert a.dtype == torch.float32 and torch.equal(a, b)
    no_dups = {k: v for k, v in whole.items() if not k.startswith("lins.")}
    assert torch.equal(LPIPS(net).load_pretrained(no_dups).pack_host(), a)
    # layout: header, then w [taps][cinp][cout] + bias per layer, then the lin layers
    assert a[:8].tolist() == [np.float32(v) for v in LR.SHIFT + LR.SCALE] + [0.0, 0.0]
    _, cin, cout, k, _, _ = LR.CONVS[net][0]
    w = a[8:8 + k * k * 4 * cout].reshape(k * k, 4, cout)
    assert torch.equal(w[:, :3], p["features.0.weight"].permute(2, 3, 1, 0).reshape(k * k, 3, cout)) and float(w[:, 3].abs().max()) == 0.0
    tail = torch.cat([p["lin%d.model.1.weight" % j].reshape(-1) for j in range(5)])
    assert torch.equal(a[-tail.numel():], tail)
    # a missing key, a wrong shape: HnrError naming the key
    last = "net.slice5.%d.bias" % LR.CONVS[net][-1][0]
    with pytest.raises(HnrError, match=last.replace(".", r"\.")):
        LPIPS(net).load_pretrained({k: v for k, v in whole.items() if k != last})
    bad = dict(whole)
    bad["lin2.model.1.weight"] = torch.zeros(1, 5, 1, 1)
    with pytest.raises(HnrError, match=r"lin2\.model\.1\.weight"):
        LPIPS(net).load_pretrained(bad)
    with pytest.raises(HnrError, match="lin"):
        LPIPS(net).load_pretrained(LR.backbone(p))
    with pytest.raises(HnrError, match=r"lin4\.model\.1\.weight"):
        LPIPS(net).load_pretrained(LR.backbone(p), lin={k: v for k, v in LR.lin_file(p).items() if not k.startswith("lin4")})
    with pytest.raises(HnrError):
        LPIPS("squeeze")
    with pytest.raises(HnrError):
        LPIPS(net, channel_order="gbr")


def test_loader_reads_paths_and_repacks_after_a_second_load(tmp_path):
    from hybridneuralrendering_amd.perceptual import LPIPS
    p, p2 = params("alex"), LR.make_params("alex", 99)
    torch.save(LR.backbone(p), tmp_path / "alexnet.pth")
    torch.save(LR.lin_file(p), tmp_path / "alex.pth")
    m = LPIPS("alex").load_pretrained(str(tmp_path / "alexnet.pth"), lin=str(tmp_path / "alex.pth"))
    a = m.pack_host()
    assert torch.equal(a, LPIPS("alex").load_pretrained(LR.lpips_state_dict("alex", p)).pack_host())
    key = [(t.data_ptr(), t._version) for t in m.parameters()]
    m.load_pretrained(LR.lpips_state_dict("alex", p2))
    assert key != [(t.data_ptr(), t._version) for t in m.parameters()] and not torch.equal(m.pack_host(), a)


def test_c_abi_refuses_bad_arguments_without_a_gpu():
    from hybridneuralrendering_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(16)                                        # non-null, aligned; never dereferenced: the checks come first
    assert L.hnr_lpips_packed_elems(2) == -1 and L.hnr_lpips_packed_elems(-1) == -1
    elems = lambda net: 8 + sum(k * k * (cin + (cin & 1)) * cout + cout for _, cin, cout, k, _, _ in LR.CONVS[net]) + sum(LR.TAP_CHANNELS[net])
    assert L.hnr_lpips_packed_elems(0) == elems("alex") and L.hnr_lpips_packed_elems(1) == elems("vgg")
    assert L.hnr_lpips_scratch_bytes(0, 30, 64) == -1 and L.hnr_lpips_scratch_bytes(0, 64, 30) == -1 and L.hnr_lpips_scratch_bytes(0, 31, 31) > 0
    assert L.hnr_lpips_scratch_bytes(1, 15, 64) == -1 and L.hnr_lpips_scratch_bytes(1, 16, 16) > 0 and L.hnr_lpips_scratch_bytes(2, 64, 64) == -1
    assert L.hnr_lpips_scratch_bytes(1, 4097, 64) == -1
    big = 1 << 40
    for call, what in ((lambda: L.hnr_lpips(0, one, one, 30, 64, 1, one, one, one, big, None), "h=30"),
                     (lambda: L.hnr_lpips(1, one, one, 64, 15, 1, one, one, one, big, None), "w=15"),
                     (lambda: L.hnr_lpips(5, one, one, 64, 64, 1, one, one, one, big, None), "net=5"),
                     (lambda: L.hnr_lpips(0, one, one, 64, 64, 1, one, None, one, big, None), "NULL"),
                     (lambda: L.hnr_lpips(0, None, one, 64, 64, 1, one, one, one, big, None), "NULL"),
                     (lambda: L.hnr_lpips(0, one, one, 64, 64, 1, ctypes.c_void_p(20), one, one, big, None), "aligned"),
                     (lambda: L.hnr_lpips(0, one, one, 64, 64, 1, one, one, one, 10, None), "scratch"),
                     (lambda: L.hnr_lpips_f32(1, one, one, 8, 64, one, one, one, big, None), "h=8"),
                     (lambda: L.hnr_lpips_f32(1, one, one, 64, 64, one, None, one, big, None), "NULL"),
                     (lambda: L.hnr_lpips_prepare(None, one, 64, 64, 1, one, one, None), "NULL"),
                     (lambda: L.hnr_lpips_prepare(one, one, 0, 64, 1, one, one, None), "h=0"),
                     (lambda: L.hnr_lpips_prepare_f32(one, one, 64, 64, None, one, None), "NULL"),
                     (lambda: L.hnr_lpips_features(1, one, 64, 64, one, None, one, big, None), "NULL"),
                     (lambda: L.hnr_lpips_features(3, one, 64, 64, one, None, one, big, None), "net=3"),
                     (lambda: L.hnr_lpips_score(0, None, 64, 64, one, one, one, big, None), "NULL"),
                     (lambda: L.hnr_lpips_tap_dims(0, 20, 64, (ctypes.c_int * 15)()), "h=20")):
        rc = call()
        assert rc < 0 and what in L.hnr_last_error().decode(), (rc, what, L.hnr_last_error())
    dims = (ctypes.c_int * 15)()
    assert L.hnr_lpips_tap_dims(0, 67, 91, dims) == 0 and list(dims) == [64, 16, 22, 192, 7, 10, 384, 3, 4, 256, 3, 4, 256, 3, 4]
    assert L.hnr_lpips_tap_dims(1, 35, 50, dims) == 0 and list(dims) == [64, 35, 50, 128, 17, 25, 256, 8, 12, 512, 4, 6, 512, 2, 3]


def test_python_layer_refuses_cpu_tensors_and_a_model_without_weights():
    from hybridneuralrendering_amd.perceptual import LPIPS
    from hybridneuralrendering_amd._lib import HnrError
    m = LPIPS("alex").load_pretrained(LR.lpips_state_dict("alex", params("alex")))
    img = torch.zeros((64, 64, 3), dtype=torch.uint8)
    with pytest.raises(HnrError, match="GPU"):
        m.pair8(img, img)
    with pytest.raises(HnrError, match="GPU"):
        m(torch.zeros(1, 3, 64, 64), torch.zeros(1, 3, 64, 64))
    with pytest.raises(HnrError, match="GPU"):
        m.tap_features(torch.zeros(2, 3, 64, 64))
    with pytest.raises(HnrError, match="training"):
        m.train()
    with pytest.raises(HnrError, match="load_pretrained"):
        LPIPS("vgg").packed()


def _rows(n, seed):
    rs = np.random.RandomState(seed)
    rows = np.zeros((n, 6))
    rows[:, 0], rows[:, 1], rows[:, 2] = rs.randint(1000, 90000, n), 3 * 40 * 50, rs.uniform(0.5, 0.9, n)
    rows[:, 3], rows[:, 4], rows[:, 5] = rs.uniform(1e-3, 1e-2, n), rs.uniform(1e-3, 1e-2, n), 1500
    return rows


def test_write_without_lpips_leaves_exactly_the_three_files_of_today(tmp_path):
    from hybridneuralrendering_amd.metrics import TestSetEvaluator, derive
    rows = _rows(4, 0)
    res = TestSetEvaluator.from_rows(rows).write(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["psnr.txt", "rmse.txt", "scores.txt", "ssim.txt"]
    d = derive(rows)
    assert open(tmp_path / "scores.txt").read() == "".join("%s: %.6f\n" % (k, np.mean(d[k])) for k in ("psnr", "ssim", "rmse"))
    assert sorted(res) == sorted(list(d) + ["mean"]) and sorted(res["mean"]) == sorted(d)
    np.testing.assert_array_equal(np.loadtxt(tmp_path / "ssim.txt"), d["ssim"])


def test_write_with_lpips_rows_adds_the_two_files_in_the_order_of_evaluate_py(tmp_path):
    from hybridneuralrendering_amd.metrics import TestSetEvaluator, derive
    rows = _rows(4, 1)
    rs = np.random.RandomState(2)
    lp = {"vgglpips": rs.uniform(0, 0.1, (4, 6)), "lpips": rs.uniform(0, 0.1, (4, 6))}
    for v in lp.values():
        v[:, 0] = v[:, 1:].sum(1)
    ev = TestSetEvaluator.from_rows(rows, lpips_rows=lp)
    res = ev.write(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["lpips.txt", "psnr.txt", "rmse.txt", "scores.txt", "ssim.txt", "vgglpips.txt"]
    lines = open(tmp_path / "scores.txt").read().splitlines()
    assert [l.split(":")[0] for l in lines] == ["psnr", "ssim", "lpips", "vgglpips", "rmse"]
    assert lines[2] == "lpips: %.6f" % np.mean(lp["lpips"][:, 0]) and lines[3] == "vgglpips: %.6f" % np.mean(lp["vgglpips"][:, 0])
    np.testing.assert_array_equal(np.loadtxt(tmp_path / "vgglpips.txt"), lp["vgglpips"][:, 0])
    np.testing.assert_array_equal(res["lpips"], lp["lpips"][:, 0])
    np.testing.assert_array_equal(res["lpips_layers"], lp["lpips"][:, 1:])
    assert res["mean"]["vgglpips"] == float(np.mean(lp["vgglpips"][:, 0])) and "lpips_layers" not in res["mean"]
    d = derive(rows)
    assert lines[0] == "psnr: %.6f" % np.mean(d["psnr"]) and lines[4] == "rmse: %.6f" % np.mean(d["rmse"])
