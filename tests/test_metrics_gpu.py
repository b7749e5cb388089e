"""hnr_frame_metrics on the GPU against the float64 / exact-integer restatement (tests/metrics_ref.py, itself checked in tests/test_metrics.py).

Bounds (none of them measured from the code under test):
  * the uint8 images, S = sum (A - B)^2 and both counts: equal as integers;
  * SSIM: 1e-10 absolute.  The window sums are exact; a window value can lose about 1e-12 where the variances cancel against C2 >= 9e-4, and only if
    the operation order differs from the restatement's; the mean of m <= 2.8e5 values in [-1, 1] summed in ANY order is within m * 2^-53 = 3.1e-11;
  * PSNR / RMSE: 1e-12 relative (fp64 functions of an exact integer);
  * the two test losses: 1e-9 relative to the fp64 sum of the fp32 squares (n <= 1e6 terms, any order).
"""
import math

import numpy as np
import pytest
import torch

import tests.metrics_ref as mr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _seeded_frame(h, w, seed, margin=1, special=True, all_masked_out=False):
    """A frame whose cast rays leave a margin of uncast pixels (zero in both images).  Values include < 0, > 1, exactly k / 255 and k / 255 +- 1 ulp:
    where a product that is not ONE float32 operation would land in the other bucket."""
    rng = np.random.default_rng(seed)
    m = margin if min(h, w) > 2 * margin + 2 else 0
    xs, ys = np.arange(m, w - m), np.arange(m, h - m)
    pix = np.stack(np.meshgrid(xs, ys, indexing="xy"), -1).reshape(-1, 2)
    pix = pix[rng.permutation(len(pix))]                                   # rays in no particular order
    R = len(pix)
    yy, xx = pix[:, 1] / max(h - 1, 1), pix[:, 0] / max(w - 1, 1)
    gt = np.stack([0.5 + 0.45 * np.sin(5 * yy + 3 * xx), 0.5 + 0.45 * np.cos(7 * xx - 2 * yy), 0.2 + 0.7 * yy * xx], -1)
    gt = (gt + rng.normal(0, 0.02, gt.shape)).astype(np.float32)
    col = (gt + rng.normal(0, 0.06, gt.shape)).astype(np.float32)          # leaves [0, 1] on both sides here and there
    if special:
        n = min(R, 256 * 3)
        k = (np.arange(n) % 256).astype(np.float32) / np.float32(255)
        col.reshape(-1)[:n] = k
        col.reshape(-1)[n:2 * n] = np.nextafter(k, np.float32(-1))[:max(0, min(n, col.size - n))]
        gt.reshape(-1)[:n] = np.nextafter(k, np.float32(2))
        col.reshape(-1)[-3:] = np.float32([-0.25, 1.75, 1.0])
    mask = np.zeros(R, np.int8) if all_masked_out else (rng.uniform(size=R) > 0.15).astype(np.int8)
    image = mr.scatter(col, pix, h, w)
    out = dict(image=_t(image), coarse_raycolor=_t(col), ray_mask=_t(mask))
    frame = dict(h=h, w=w, pixel_idx=_t(pix.astype(np.float32))[None], gt_image=_t(gt)[None])
    host = dict(image=image, gt_full=mr.scatter(gt, pix, h, w), col=col, gt=gt, mask=mask)
    return out, frame, host


def _check_row(got, host, win, L, a8=None, b8=None, tag=""):
    want, A, B = mr.row(host["image"], host["gt_full"], host["col"], host["gt"], host["mask"], win, L)
    print("%s win=%d L=%g  S %d/%d  ssim %.15f (ref %.15f, diff %.2e)  mse_full rel %.2e  mse_masked rel %.2e" % (
        tag, win, L, got[mr.SQERR8], want[mr.SQERR8], got[mr.SSIM], want[mr.SSIM], abs(got[mr.SSIM] - want[mr.SSIM]),
        abs(got[mr.MSE_FULL] - want[mr.MSE_FULL]) / want[mr.MSE_FULL],
        abs(got[mr.MSE_MASKED] - want[mr.MSE_MASKED]) / want[mr.MSE_MASKED] if want[mr.N_MASKED] else 0.0))
    if a8 is not None:
        np.testing.assert_array_equal(a8.cpu().numpy(), A)
        np.testing.assert_array_equal(b8.cpu().numpy(), B)
    assert int(got[mr.SQERR8]) == int(want[mr.SQERR8]) and got[mr.SQERR8] == float(int(got[mr.SQERR8]))
    assert int(got[mr.N8]) == host["image"].size and int(got[mr.N_MASKED]) == int((host["mask"] > 0).sum())
    assert abs(got[mr.SSIM] - want[mr.SSIM]) <= 1e-10
    from hybridneuralrendering_amd.metrics import derive
    d = derive(got[None])
    psnr, rmse = mr.psnr_rmse(int(want[mr.SQERR8]), int(want[mr.N8]))
    if want[mr.SQERR8] == 0:                                  # the 8-bit images are identical: +inf, as compare_psnr gives
        assert d["psnr"][0] == float("inf") and d["rmse"][0] == 0.0
    else:
        assert abs(d["psnr"][0] - psnr) <= 1e-12 * abs(psnr) and abs(d["rmse"][0] - rmse) <= 1e-12 * rmse
    assert abs(got[mr.MSE_FULL] - want[mr.MSE_FULL]) <= 1e-9 * want[mr.MSE_FULL]
    if want[mr.N_MASKED]:
        assert abs(got[mr.MSE_MASKED] - want[mr.MSE_MASKED]) <= 1e-9 * want[mr.MSE_MASKED]
        assert abs(d["psnr_masked"][0] + 10 * math.log10(want[mr.MSE_MASKED])) <= 1e-8
    else:
        assert math.isnan(got[mr.MSE_MASKED])


@pytest.mark.parametrize("w,h", [(620, 460), (64, 48), (53, 37)])
@pytest.mark.parametrize("win", [7, 11])
@pytest.mark.parametrize("L", [1.0, 2.0])
def test_seeded_frames_match_the_restatement(w, h, win, L):
    from hybridneuralrendering_amd.metrics import frame_metrics
    out, frame, host = _seeded_frame(h, w, seed=w + win)
    a8, b8 = torch.zeros((h, w, 3), dtype=torch.uint8, device=DEV), torch.zeros((h, w, 3), dtype=torch.uint8, device=DEV)
    row = frame_metrics(out, frame, win=win, data_range=L, images8=(a8, b8))
    _check_row(row[0].cpu().numpy(), host, win, L, a8, b8, tag="%dx%d" % (w, h))


@pytest.mark.parametrize("win", [7, 11])
@pytest.mark.parametrize("L", [1.0, 2.0])
def test_an_image_of_one_window(win, L):
    from hybridneuralrendering_amd.metrics import frame_metrics
    out, frame, host = _seeded_frame(win, win, seed=win)
    row = frame_metrics(out, frame, win=win, data_range=L)
    _check_row(row[0].cpu().numpy(), host, win, L, tag="%dx%d" % (win, win))


def test_frame_without_a_valid_ray_gives_nan_and_count_zero():
    from hybridneuralrendering_amd.metrics import frame_metrics
    out, frame, host = _seeded_frame(37, 53, seed=3, all_masked_out=True)
    got = frame_metrics(out, frame, win=11)[0].cpu().numpy()
    assert math.isnan(got[mr.MSE_MASKED]) and got[mr.N_MASKED] == 0
    _check_row(got, host, 11, 2.0, tag="no valid ray")


def test_identical_images_on_the_device():
    from hybridneuralrendering_amd.metrics import frame_metrics, derive
    out, frame, host = _seeded_frame(48, 64, seed=9)
    frame["gt_image"] = out["coarse_raycolor"][None].clone()
    d = derive(frame_metrics(out, frame, win=11).cpu().numpy())
    assert d["sqerr8"][0] == 0 and d["psnr"][0] == float("inf") and d["rmse"][0] == 0 and d["ssim"][0] == 1.0 and d["mse_full"][0] == 0


def test_two_runs_give_identical_bits():
    from hybridneuralrendering_amd.metrics import frame_metrics
    out, frame, host = _seeded_frame(460, 620, seed=4)
    a = frame_metrics(out, frame, win=11).cpu().numpy()
    b = frame_metrics(out, frame, win=11).cpu().numpy()
    assert a.tobytes() == b.tobytes()


def _golden_frame(perturb_seed=None):
    """The 64x48, 2640-ray frame of tests/golden/render_frame_chunked.npz (uncast margin pixels) with the reference's own image as ground truth, or a
    seeded perturbation of it."""
    from tests.test_render_gpu import _chunk_loop_frame
    dev = torch.device(DEV)
    z, frame, cloud, rnd = _chunk_loop_frame(dev)
    pix = z["pix"].astype(np.int64)
    gt = np.ascontiguousarray(z["image"][pix[:, 1], pix[:, 0]]).astype(np.float32)
    if perturb_seed is not None:
        gt = (gt + np.random.default_rng(perturb_seed).normal(0, 0.05, gt.shape)).astype(np.float32)
    frame = dict(frame, gt_image=_t(gt)[None])
    return z, frame, cloud, rnd, gt, pix


@pytest.mark.parametrize("perturb_seed", [None, 11])
def test_golden_frame_rendered_by_render_image(perturb_seed):
    from hybridneuralrendering_amd.driver import render_image
    from hybridneuralrendering_amd.metrics import frame_metrics
    z, frame, cloud, rnd, gt, pix = _golden_frame(perturb_seed)
    h, w = frame["h"], frame["w"]
    out = render_image(rnd, cloud, frame)
    host = dict(image=out["image"].cpu().numpy(), gt_full=mr.scatter(gt, pix, h, w), col=out["coarse_raycolor"].cpu().numpy(), gt=gt,
                mask=out["ray_mask"].cpu().numpy())
    assert float(np.abs(host["image"][0]).max()) == 0.0 and float(np.abs(host["gt_full"][0]).max()) == 0.0      # margin rows: zero in both, and they count
    for win in (7, 11):
        for L in (1.0, 2.0):
            a8, b8 = torch.zeros((h, w, 3), dtype=torch.uint8, device=DEV), torch.zeros((h, w, 3), dtype=torch.uint8, device=DEV)
            got = frame_metrics(out, frame, win=win, data_range=L, images8=(a8, b8))[0].cpu().numpy()
            assert int(got[mr.N8]) == 3 * h * w
            _check_row(got, host, win, L, a8, b8, tag="golden frame (%s)" % ("reference image" if perturb_seed is None else "perturbed"))


def _three_frames():
    return [_seeded_frame(48, 64, seed=20 + k, special=(k == 0)) for k in range(3)]


def test_evaluator_equals_single_frame_calls_row_for_row(tmp_path):
    from hybridneuralrendering_amd.metrics import TestSetEvaluator, frame_metrics
    frames = _three_frames()
    ev = TestSetEvaluator(4, win=11, data_range=2.0, device=DEV, save_images=True)
    for out, frame, _ in frames:
        ev.add(out, frame)
    res = ev.summary()
    table = ev.table.cpu().numpy()
    for k, (out, frame, host) in enumerate(frames):
        single = frame_metrics(out, frame, win=11, data_range=2.0)[0].cpu().numpy()
        assert single.tobytes() == table[k].tobytes()
        np.testing.assert_array_equal(ev.img8[k].cpu().numpy(), mr.quantise(host["image"]))
    assert len(res["psnr"]) == 3 and (table[3] == 0).all()
    assert res["mean"]["psnr"] == float(np.mean(res["psnr"]))
    res2 = ev.write(str(tmp_path))
    assert open(tmp_path / "scores.txt").read() == "".join("%s: %.6f\n" % (k, np.mean(res[k])) for k in ("psnr", "ssim", "rmse"))
    from PIL import Image
    np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / "step-0002-gt_image.png")), mr.quantise(frames[2][2]["gt_full"]))
    np.testing.assert_array_equal(res2["ssim"], res["ssim"])


def test_add_performs_no_host_synchronisation():
    from hybridneuralrendering_amd.metrics import TestSetEvaluator
    frames = _three_frames()
    ev = TestSetEvaluator(3, device=DEV, save_images=True)
    ev.add(*frames[0][:2])                                   # (first call: the library loads, the image buffers are allocated)
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
        # the mode does catch a host read in this build: otherwise the loop above has shown nothing
        with pytest.raises(RuntimeError):
            ev.table[0, 0].item()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(ev.summary()["ssim"]) == 3


def test_evaluate_frames_leaves_the_rendered_frame_as_a_plain_call_gives_it():
    from hybridneuralrendering_amd.driver import render_image, evaluate_frames
    from hybridneuralrendering_amd.metrics import frame_metrics
    z, frame, cloud, rnd, gt, pix = _golden_frame(11)
    plain = render_image(rnd, cloud, frame)
    seen = []
    ev = evaluate_frames(rnd, cloud, [frame, frame], win=11, data_range=2.0, on_frame=lambda i, o: seen.append(o))
    assert len(seen) == 2 and ev.n == 2
    for o in seen:
        for k in ("image", "ray_mask", "coarse_raycolor"):
            assert torch.equal(o[k], plain[k]), k
        assert sorted(o) == sorted(plain)
    table = ev.table.cpu().numpy()
    single = frame_metrics(plain, frame, win=11, data_range=2.0)[0].cpu().numpy()
    assert table[0].tobytes() == single.tobytes() and table[1].tobytes() == single.tobytes()
    s = ev.summary()
    assert np.isfinite(s["mean"]["psnr"]) and 0 < s["mean"]["ssim"] < 1
