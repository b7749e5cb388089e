"""Frame metrics without a GPU: the float64 restatement the GPU tests compare against (tests/metrics_ref.py) is itself checked against closed forms
and against the scikit-image formulation on scipy.ndimage.uniform_filter; hnr_frame_metrics refuses bad arguments before any HIP call; the
evaluator writes report_metrics' files (run/evaluate.py:89-97)."""
import ctypes
import math
import os

import numpy as np
import pytest

import tests.metrics_ref as mr


def _images(h, w, seed, noise=0.08):
    """a smooth float32 image in [0, 1] and a noisy copy: realistic window variances (SSIM neither 0 nor 1)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 3, h), np.linspace(0, 4, w), indexing="ij")
    base = np.stack([0.5 + 0.4 * np.sin(yy + xx), 0.5 + 0.4 * np.cos(3 * xx - yy), 0.3 + 0.1 * yy * np.sin(5 * xx)], axis=-1)
    gt = np.clip(base + rng.normal(0, 0.02, (h, w, 3)), 0, 1).astype(np.float32)
    img = (gt + rng.normal(0, noise, (h, w, 3))).astype(np.float32)
    return img, gt


def test_identical_images_give_ssim_one_psnr_inf_rmse_zero():
    img, _ = _images(37, 53, 0)
    A = mr.quantise(img)
    for L in (1.0, 2.0):
        for win in (7, 11):
            assert mr.ssim8(A, A, win, L) == 1.0
    S, n = mr.sqerr8(A, A)
    assert S == 0 and n == 37 * 53 * 3
    psnr, rmse = mr.psnr_rmse(S, n)
    assert psnr == float("inf") and rmse == 0.0


def test_two_constant_images_have_the_closed_form():
    """every variance is 0: SSIM = (2uv + C1) / (u^2 + v^2 + C1); PSNR = 20 log10(255 / |a - b|)"""
    for a, b in ((10, 200), (255, 0), (128, 127), (3, 77)):
        A, B = np.full((20, 31, 3), a, np.uint8), np.full((20, 31, 3), b, np.uint8)
        u, v = a / 255.0, b / 255.0
        for L in (1.0, 2.0):
            C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
            want = (2 * u * v + C1) / (u * u + v * v + C1)
            for win in (3, 11):
                # (the integer window sums make uxx - ux^2 cancel to rounding, not to exactly 0: |v| <= 2^-52, against C2 >= 9e-4)
                assert abs(mr.ssim8(A, B, win, L) - want) < 1e-12, (a, b, L, win)
        S, n = mr.sqerr8(A, B)
        psnr, rmse = mr.psnr_rmse(S, n)
        assert abs(psnr - 20 * math.log10(255.0 / abs(a - b))) < 1e-12 * abs(psnr) + 1e-12 and abs(rmse - abs(a - b) / 255.0) < 1e-15


def test_one_window_when_the_image_is_the_window():
    img, gt = _images(11, 11, 1)
    A, B = mr.quantise(img), mr.quantise(gt)
    vals = []
    for c in range(3):
        x, y = A[..., c].astype(np.float64) / 255, B[..., c].astype(np.float64) / 255
        NP = 121
        ux, uy = x.mean(), y.mean()
        vx, vy, vxy = ((x - ux) ** 2).sum() / (NP - 1), ((y - uy) ** 2).sum() / (NP - 1), ((x - ux) * (y - uy)).sum() / (NP - 1)
        C1, C2 = 0.02 ** 2, 0.06 ** 2
        vals.append((2 * ux * uy + C1) * (2 * vxy + C2) / ((ux * ux + uy * uy + C1) * (vx + vy + C2)))
    assert mr.window_sums(A[..., 0], 11).shape == (1, 1)
    assert abs(mr.ssim8(A, B, 11, 2.0) - np.mean(vals)) < 1e-12


@pytest.mark.parametrize("h,w", [(480, 640), (460, 620), (37, 53), (11, 11)])
def test_restatement_equals_the_scikit_image_formulation(h, w):
    """measured on these inputs: <= 1.3e-14 absolute, both L (printed below); the same formulation in float32 is 2e-7 away, which is why fp64 is
    asked for.  Bound: 1e-12, far above the one and far below the other."""
    img, gt = _images(h, w, 2)
    A, B = mr.quantise(img), mr.quantise(gt)
    X, Y = A.astype(np.float64) / 255.0, B.astype(np.float64) / 255.0
    for L in (1.0, 2.0):
        got, want = mr.ssim8(A, B, 11, L), mr.ssim_uniform_filter(X, Y, 11, L)
        print("%dx%d L=%g restatement %.17g uniform_filter %.17g diff %.2e" % (w, h, L, got, want, abs(got - want)))
        assert 0.0 < got < 1.0
        assert abs(got - want) <= 1e-12


def test_quantisation_is_the_fp32_product():
    """k / 255 and its neighbours: the bucket is decided by ONE float32 product (utils/visualizer.py:23-24)"""
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    x = np.concatenate([k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2)), np.float32([-0.5, 1.5, -0.0, 1.0])]).astype(np.float32)
    q = mr.quantise(x)
    want = np.floor(np.clip(x, 0, 1) * np.float32(255)).astype(np.uint8)
    np.testing.assert_array_equal(q, want)
    assert q[-4] == 0 and q[-3] == 255 and q[-1] == 255
    assert (q[:256].astype(int) - np.arange(256)).min() >= -1          # some k/255 * 255 round below k in float32: that is the contract


def test_c_abi_refuses_bad_arguments_without_touching_the_gpu():
    from hybridneuralrendering_amd import _lib
    L = _lib.lib()
    one, null = ctypes.c_void_p(4096), None
    bad = -1
    call = lambda image=one, gt=one, h=48, w=64, col=one, gtr=one, mask=one, R=100, win=11, dr=2.0, row=one, a8=null, b8=null, scratch=one: \
        L.hnr_frame_metrics(image, gt, h, w, col, gtr, mask, R, win, ctypes.c_float(dr), row, a8, b8, scratch, null)
    assert call(win=10) == bad and b"win" in L.hnr_last_error()          # even
    assert call(win=1) == bad
    assert call(h=9, w=64, win=11) == bad                                  # win > min(h, w)
    assert call(h=64, w=9, win=11) == bad
    assert call(h=48, w=64, win=33) == bad                                 # above the cap of the LDS tile (31 >= 11)
    assert call(dr=0.0) == bad and b"data_range" in L.hnr_last_error()
    assert call(dr=-1.0) == bad
    assert call(dr=float("nan")) == bad
    assert call(image=null) == bad
    assert call(gt=null) == bad
    assert call(row=null) == bad
    assert call(scratch=null) == bad
    assert call(h=0) == bad and call(w=0) == bad
    assert call(R=-1) == bad
    assert call(col=null) == bad and call(mask=null) == bad               # rays without their arrays
    assert call(a8=one) == bad                                             # one uint8 image without the other
    assert L.hnr_frame_metrics_scratch_bytes(460, 620, 11) == 20 * 29 * 7 * 8
    assert L.hnr_frame_metrics_scratch_bytes(460, 620, 12) == bad
    assert L.hnr_frame_metrics_scratch_bytes(11, 11, 11) == 7 * 8


def test_python_layer_refuses_cpu_tensors():
    import torch
    from hybridneuralrendering_amd import metrics
    from hybridneuralrendering_amd._lib import HnrError
    out = dict(image=torch.zeros(16, 16, 3), coarse_raycolor=torch.zeros(4, 3), ray_mask=torch.ones(4, dtype=torch.int8))
    frame = dict(h=16, w=16, pixel_idx=torch.zeros(4, 2), gt_image=torch.zeros(4, 3))
    with pytest.raises(HnrError):
        metrics.frame_metrics(out, frame)
    assert metrics.NCOLS == mr.NCOLS and [metrics.FM[k] for k in ("SQERR8", "N8", "SSIM", "MSE_FULL", "MSE_MASKED", "N_MASKED")] == list(range(6))


def _rows(n, h=24, w=32, win=7, L=2.0):
    rows, As, Bs = [], [], []
    rng = np.random.default_rng(5)
    for k in range(n):
        img, gt = _images(h, w, 10 + k, noise=0.03 * (k + 1))
        pix = np.stack(np.meshgrid(np.arange(w), np.arange(h), indexing="xy"), -1).reshape(-1, 2)
        mask = (rng.uniform(size=len(pix)) > 0.2).astype(np.int8)
        r, A, B = mr.row(img, gt, img[pix[:, 1], pix[:, 0]], gt[pix[:, 1], pix[:, 0]], mask, win, L)
        rows.append(r); As.append(A); Bs.append(B)
    return np.stack(rows), np.stack(As), np.stack(Bs)


def test_write_produces_the_files_of_report_metrics(tmp_path):
    from hybridneuralrendering_amd.metrics import TestSetEvaluator
    rows, As, Bs = _rows(3)
    ev = TestSetEvaluator.from_rows(rows, win=7)
    res = ev.write(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["psnr.txt", "rmse.txt", "scores.txt", "ssim.txt"]
    want = {"psnr": [], "rmse": [], "ssim": rows[:, mr.SSIM]}
    for r in rows:
        p, q = mr.psnr_rmse(int(r[mr.SQERR8]), int(r[mr.N8]))
        want["psnr"].append(p); want["rmse"].append(q)
    for key in ("psnr", "ssim", "rmse"):
        vals = np.loadtxt(tmp_path / (key + ".txt")).reshape(-1)
        np.testing.assert_allclose(vals, want[key], rtol=1e-15, atol=0)
        np.testing.assert_array_equal(vals, res[key])
    lines = open(tmp_path / "scores.txt").read().splitlines()
    assert [l.split(": ")[0] for l in lines] == ["psnr", "ssim", "rmse"]
    for l in lines:
        key, val = l.split(": ")
        assert val == "%.6f" % np.mean(want[key])
    assert res["mean"]["ssim"] == float(np.mean(rows[:, mr.SSIM]))
    np.testing.assert_array_equal(res["mse_full"], rows[:, mr.MSE_FULL])
    np.testing.assert_allclose(res["psnr_masked"], -10 * np.log10(rows[:, mr.MSE_MASKED]), rtol=1e-15)


def test_saved_pngs_reproduce_the_scores(tmp_path):
    """what run/evaluate.py would compute from the folder: read the PNGs back, run the restatement, compare with scores.txt"""
    from PIL import Image
    from hybridneuralrendering_amd.metrics import TestSetEvaluator
    rows, As, Bs = _rows(2, win=11, L=2.0)
    ev = TestSetEvaluator.from_rows(rows, img8=As, gt8=Bs)
    ev.write(str(tmp_path), ids=[0, 5])
    names = sorted(f for f in os.listdir(tmp_path) if f.endswith(".png"))
    assert names == ["step-0000-coarse_raycolor.png", "step-0000-gt_image.png", "step-0005-coarse_raycolor.png", "step-0005-gt_image.png"]
    got = {"psnr": [], "ssim": [], "rmse": []}
    for i in (0, 5):
        A = np.asarray(Image.open(tmp_path / ("step-%04d-coarse_raycolor.png" % i)))
        B = np.asarray(Image.open(tmp_path / ("step-%04d-gt_image.png" % i)))
        assert A.dtype == np.uint8 and A.shape == (24, 32, 3)
        p, q = mr.psnr_rmse(*mr.sqerr8(A, B))
        got["psnr"].append(p); got["rmse"].append(q); got["ssim"].append(mr.ssim8(A, B, 11, 2.0))
    text = "".join("%s: %.6f\n" % (k, np.mean(got[k])) for k in ("psnr", "ssim", "rmse"))
    assert open(tmp_path / "scores.txt").read() == text


def test_no_valid_ray_gives_nan_and_zero_in_the_restatement_and_in_derive():
    from hybridneuralrendering_amd import metrics
    img, gt = _images(16, 16, 3)
    r, _, _ = mr.row(img, gt, img.reshape(-1, 3), gt.reshape(-1, 3), np.zeros(256, np.int8), 7, 1.0)
    assert math.isnan(r[mr.MSE_MASKED]) and r[mr.N_MASKED] == 0
    d = metrics.derive(r[None])
    assert math.isnan(d["psnr_masked"][0]) and d["n_masked"][0] == 0 and np.isfinite(d["psnr"][0])
