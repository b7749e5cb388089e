"""CPU checks of the patch SSIM term: the restatement tests/ssim_loss_ref.py against itself (the analytic gradient the kernel forms = autograd of
the same expression in fp64; layouts; sharding by patches; identical images; an all-missed batch), the argument errors from Python and from the C
ABI without a device, and the exported symbols."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ssim_loss_ref as R

W_SSIM, FW = 0.2, 0.7


@pytest.mark.parametrize("mask_kind", ["all", "tenth", "patch"])
@pytest.mark.parametrize("pn,ps,layout", R.SHAPES, ids=["%dx%d-%s" % s for s in R.SHAPES])
def test_analytic_gradient_equals_autograd_in_fp64(pn, ps, layout, mask_kind):
    c, g, m = R.make_case(pn, ps, layout, mask_kind)
    ref = R.references(pn, ps, layout, mask_kind, W_SSIM, FW)[0]
    x = c.double().requires_grad_(True)
    term = R.ssim_expr(x, g.double(), m, pn, ps, W_SSIM, layout, frame_weight=FW)
    term.backward()
    scale = float(x.grad.abs().max())
    if ref["hits"] == 0:
        assert float(term.detach()) == 0.0 and scale == 0.0 and float(ref["term"]) == 0.0 and not ref["grad"].any()
        return
    assert scale > 0
    assert abs(float(term.detach()) - float(ref["term"])) <= 1e-12 * abs(float(term.detach()))
    assert float((ref["grad"] - x.grad).abs().max()) <= 1e-12 * scale
    assert not ref["grad"][m <= 0].any()                                   # exactly 0 on missed rays
    # the figures the fp32 form is off by (what the GPU test's bound is made of)
    r32 = R.references(pn, ps, layout, mask_kind, W_SSIM, FW)[1]
    print("SSIM_REF %dx%d %s %s: L %.6f  max|grad| %.3e  fp32 restatement off by L %.2e grad %.2e" % (
        pn, ps, layout, mask_kind, float(ref["L"]), scale, abs(float(r32["L"]) - float(ref["L"])), float((r32["grad"].double() - ref["grad"]).abs().max())))


def test_constant_patch_gradient_equals_autograd_in_fp64():
    c, g, m = R.make_case(2, 9, "grid", "all", constant_patch=True)
    ref = R.ssim_term(c, g, m, 2, 9, W_SSIM)
    x = c.double().requires_grad_(True)
    R.ssim_expr(x, g.double(), m, 2, 9, W_SSIM).backward()
    assert float((ref["grad"] - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())
    # sigma = 0 in patch 0: cs = 1 and s is the luminance factor -- up to the fp32 window's sum, which is 1 only to 1e-7: the variances come out
    # as x^2 (sum g2 - (sum g2)^2) ~ 1e-8, against C2 = 9e-4
    s0 = ref["s"][0]
    want = (2 * 0.52 * 0.37 + R.C1) / (0.52 ** 2 + 0.37 ** 2 + R.C1)
    assert float((s0 - want).abs().max()) < 1e-5


def test_grid_and_patch_major_layouts_of_the_same_patches_agree():
    pn, ps = 3, 8
    c, g, m = R.make_case(pn, ps, "grid", "tenth")
    a = R.ssim_term(c, g, m, pn, ps, W_SSIM, "grid")
    pm = lambda t: R.from_patches(R.to_patches(t.reshape(pn * pn * ps * ps, -1), pn, ps, "grid"), pn * pn, ps, "patch_major")
    b = R.ssim_term(pm(c), pm(g), pm(m).reshape(-1), pn * pn, ps, W_SSIM, "patch_major")
    assert float(a["L"]) == float(b["L"]) and a["hits"] == b["hits"]
    assert torch.equal(pm(a["grad"]), b["grad"])


def test_two_patch_major_halves_with_the_whole_count_sum_to_the_whole_batch():
    n, ps = 6, 8
    c, g, m = R.make_case(n, ps, "patch_major", "tenth")
    whole = R.ssim_term(c, g, m, n, ps, W_SSIM, "patch_major", frame_weight=FW)
    h = 3 * ps * ps
    parts = [R.ssim_term(c[s], g[s], m[s], 3, ps, W_SSIM, "patch_major", norm_patches=n, frame_weight=FW) for s in (slice(0, h), slice(h, 2 * h))]
    assert abs(float(parts[0]["L"]) + float(parts[1]["L"]) - float(whole["L"])) <= 1e-14
    assert abs(float(parts[0]["term"]) + float(parts[1]["term"]) - float(whole["term"])) <= 1e-14
    assert torch.equal(torch.cat([parts[0]["grad"], parts[1]["grad"]]), whole["grad"])     # a ray's gradient is its own patch's
    assert parts[0]["hits"] + parts[1]["hits"] == whole["hits"]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_identical_images_give_one_in_every_window_and_zero_loss(dtype):
    c, g, m = R.make_case(2, 9, "grid", "tenth")
    r = R.ssim_term(g, g, m, 2, 9, W_SSIM, dtype=dtype)
    assert bool((r["s"] == 1).all()) and float(r["L"]) == 0.0 and float(r["term"]) == 0.0 and float(r["ssim"]) == 1.0


def test_all_missed_batch_has_no_term_and_no_gradient():
    c, g, m = R.make_case(2, 9, "grid", "none")
    for dtype in (torch.float64, torch.float32):
        r = R.ssim_term(c, g, m, 2, 9, W_SSIM, dtype=dtype)
        assert r["hits"] == 0 and float(r["L"]) == 0.0 and float(r["term"]) == 0.0 and not r["grad"].any()


def test_window_helper_is_the_restatements_window():
    from hybridneuralrendering_amd import losses
    from hybridneuralrendering_amd._lib import HnrError
    g = losses.ssim_window()
    assert g.dtype == torch.float32 and g.shape == (7,) and torch.equal(g, R.window())
    want = np.exp(-(np.arange(7) - 3.0) ** 2 / (2 * 1.5 ** 2))
    np.testing.assert_allclose(g.numpy(), want / want.sum(), rtol=3e-7)
    assert abs(float(g.double().sum()) - 1) < 2e-7 and torch.equal(g, g.flip(0))
    for kw in (dict(win_size=11), dict(win_sigma=1.0)):                    # other windows are out of scope
        with pytest.raises(HnrError):
            losses.ssim_window(**kw)


def test_argument_errors_are_raised_from_python_without_a_device():
    from hybridneuralrendering_amd import losses, train
    from hybridneuralrendering_amd._lib import HnrError
    c, g, m = R.make_case(2, 9, "grid", "all")
    ok = dict(patch_num=2, patch_size=9, w_ssim=0.1)
    bad = [dict(ok, patch_size=6), dict(ok, patch_size=65), dict(ok, patch_num=3), dict(ok, w_ssim=-0.1), dict(ok, w_ssim=float("inf")),
           dict(ok, w_ssim=float("nan")), dict(ok, layout="rows"), dict(ok, layout="patch_major"), dict(ok, norm_patches=3), dict(ok, patch_num=0),
           dict(ok, frame_weight=-1.0)]
    for kw in bad:
        with pytest.raises(HnrError) as e:
            losses.ssim_patch_loss_grads(c, g, m, **kw)
        assert "GPU" not in str(e.value), (kw, str(e.value))                # the argument's own error, not the CPU tensor's
        with pytest.raises(HnrError):
            losses.ssim_patch_loss(c, g, m, **kw)
    with pytest.raises(HnrError) as e:                                     # good arguments: only the missing device is left to complain about
        losses.ssim_patch_loss_grads(c, g, m, **ok)
    assert "GPU" in str(e.value)
    # the step's own check: a "random" batch has no patches
    rays = torch.zeros(324, 3)
    assert train._ssim_arg("train_step", 0.0, None, None, "grid", rays) is None
    assert train._ssim_arg("train_step", 0.1, 2, 9, "grid", rays) == (2, 9, "grid", 0.1, None)
    for args in ((0.1, None, None, "grid"), (0.1, 2, 8, "grid"), (-0.1, 2, 9, "grid"), (0.1, 2, 9, "random")):
        with pytest.raises(HnrError):
            train._ssim_arg("train_step", *args, rays)


def test_library_exports_the_two_symbols_and_checks_arguments_before_any_launch():
    from hybridneuralrendering_amd import _lib
    L = _lib.lib()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "hnr_ssim_loss") and hasattr(raw, "hnr_ssim_loss_scratch_bytes")
    assert "hnr_ssim_loss" in _lib.SIGNATURES and "hnr_ssim_loss_scratch_bytes" in _lib.SIGNATURES
    assert L.hnr_ssim_loss_scratch_bytes(49) == 49 * 16 and L.hnr_ssim_loss_scratch_bytes(1) == 16
    one = ctypes.c_void_p(16)                                              # a non-NULL fake pointer; never dereferenced
    win = (ctypes.c_float * 7)(*[float(v) for v in R.window()])
    badwin = (ctypes.c_float * 7)(*([float("nan")] + [0.1] * 6))

    def call(pn=7, ps=8, norm=0, w=0.1, fw=1.0, win=win, color=one, out4=one, g=one, acc=0, scratch=one):
        return L.hnr_ssim_loss(color, one, one, pn, ps, norm, win, w, fw, None, None, out4, g, acc, scratch, None)
    for kw in (dict(ps=6), dict(ps=65), dict(pn=0), dict(norm=-1), dict(norm=48), dict(w=-1.0), dict(w=float("inf")), dict(w=float("nan")),
               dict(fw=-1.0), dict(fw=float("nan")), dict(win=None), dict(win=badwin), dict(color=None), dict(out4=None), dict(scratch=None),
               dict(g=None, acc=1), dict(pn=-3, norm=2)):
        assert call(**kw) == -1, kw                                        # HNR_ERR_BADARG
        assert b"hnr_ssim_loss" in L.hnr_last_error()
