"""Float64 / exact-integer restatement of the frame metrics (include/hnr.h: hnr_frame_metrics) for the tests.  numpy only.  The product never
imports this file."""
import numpy as np

NCOLS = 6
SQERR8, N8, SSIM, MSE_FULL, MSE_MASKED, N_MASKED = range(6)


def quantise(img):
    """utils/visualizer.py:23-24 on a float32 array: the bytes of the PNG."""
    img = np.asarray(img)
    assert img.dtype == np.float32
    return (np.clip(img, 0, 1) * 255).astype(np.uint8)


def window_sums(a, win):
    """Sums of every win x win window that lies inside a [h, w] integer array, from an int64 integral image: [h - win + 1, w - win + 1], exact."""
    a = np.asarray(a, dtype=np.int64)
    ii = np.zeros((a.shape[0] + 1, a.shape[1] + 1), dtype=np.int64)
    ii[1:, 1:] = a.cumsum(0).cumsum(1)
    return ii[win:, win:] - ii[:-win, win:] - ii[win:, :-win] + ii[:-win, :-win]


def ssim8(A, B, win=11, L=2.0):
    """structural_similarity(B / 255, A / 255, win_size=win, multichannel=True) with data_range L, on uint8 images [h, w, 3]."""
    A, B = np.asarray(A), np.asarray(B)
    assert A.dtype == np.uint8 and B.dtype == np.uint8 and A.shape == B.shape and A.shape[2] == 3
    assert win % 2 == 1 and 3 <= win <= min(A.shape[:2])
    NP = float(win * win)
    dn1, dn2 = 255.0 * NP, 65025.0 * NP
    cov_norm = NP / (NP - 1.0)
    C1, C2 = (0.01 * L) * (0.01 * L), (0.03 * L) * (0.03 * L)
    per_channel = []
    for c in range(3):
        a, b = A[..., c].astype(np.int64), B[..., c].astype(np.int64)
        ux, uy = window_sums(a, win) / dn1, window_sums(b, win) / dn1
        uxx, uyy, uxy = window_sums(a * a, win) / dn2, window_sums(b * b, win) / dn2, window_sums(a * b, win) / dn2
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        A1, A2 = 2.0 * ux * uy + C1, 2.0 * vxy + C2
        B1, B2 = ux * ux + uy * uy + C1, vx + vy + C2
        per_channel.append(float(np.mean((A1 * A2) / (B1 * B2))))
    return (per_channel[0] + per_channel[1] + per_channel[2]) / 3.0


def sqerr8(A, B):
    d = np.asarray(A).astype(np.int64) - np.asarray(B).astype(np.int64)
    return int((d * d).sum()), int(d.size)


def psnr_rmse(S, n):
    """compare_psnr / sqrt(mean_squared_error) of run/evaluate.py on x = A / 255 from the integer S."""
    if S == 0:
        return float("inf"), 0.0
    mse8 = S / (65025.0 * n)
    return 10.0 * np.log10(1.0 / mse8), float(np.sqrt(mse8))


def frame_losses(image, gt_full, raycolor, gt_rays, ray_mask):
    """run/test_ft.py:233-243: squares in float32 (as torch forms them), sums in float64."""
    sq = (np.asarray(image, np.float32) - np.asarray(gt_full, np.float32)) ** 2
    assert sq.dtype == np.float32
    mse_full = float(sq.astype(np.float64).sum() / sq.size)
    on = np.asarray(ray_mask) > 0
    sqm = (np.asarray(raycolor, np.float32)[on] - np.asarray(gt_rays, np.float32)[on]) ** 2
    n = int(on.sum())
    mse_masked = float(sqm.astype(np.float64).sum() / (3.0 * n)) if n else float("nan")
    return mse_full, mse_masked, n


def scatter(values, pix, h, w):
    """run/test_ft.py:191-193 / :203-204: [R,3] values placed by pixel (x, y) into zeros [h, w, 3]."""
    full = np.zeros((h, w, 3), dtype=np.float32)
    pix = np.asarray(pix).astype(np.int64)
    full[pix[:, 1], pix[:, 0]] = values
    return full


def row(image, gt_full, raycolor, gt_rays, ray_mask, win=11, L=2.0):
    A, B = quantise(image), quantise(gt_full)
    S, n = sqerr8(A, B)
    mf, mm, nm = frame_losses(image, gt_full, raycolor, gt_rays, ray_mask)
    out = np.zeros(NCOLS)
    out[SQERR8], out[N8], out[SSIM], out[MSE_FULL], out[MSE_MASKED], out[N_MASKED] = S, n, ssim8(A, B, win, L), mf, mm, nm
    return out, A, B


def ssim_uniform_filter(X, Y, win=11, L=2.0):
    """The scikit-image formulation on what scikit-image itself calls: scipy.ndimage.uniform_filter in float64 over float images X, Y [h, w, 3]
    in [0, 1], the (win - 1) / 2 border cropped, mean per channel, mean over the channels (skimage/metrics/_structural_similarity.py)."""
    from scipy.ndimage import uniform_filter
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    NP = win * win
    cov_norm = NP / (NP - 1.0)
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    pad = (win - 1) // 2
    vals = []
    for c in range(3):
        x, y = X[..., c], Y[..., c]
        ux, uy = uniform_filter(x, size=win), uniform_filter(y, size=win)
        uxx, uyy, uxy = uniform_filter(x * x, size=win), uniform_filter(y * y, size=win), uniform_filter(x * y, size=win)
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
        vals.append(S[pad:S.shape[0] - pad, pad:S.shape[1] - pad].mean())
    return float(np.mean(vals))
