"""Restatement of the blur scoring of the content-aware frame weights in numpy, written from the formulas of include/hnr.h (hnr_blur_edges,
hnr_blur_score_pair).  cv2 is not available: the edge maps follow OpenCV's documented definitions of `blur` (normalised box filter) and
`Laplacian(ksize=1)` (aperture [[0,1,0],[1,-4,1],[0,1,0]]), both with BORDER_REFLECT_101."""
import numpy as np


def edges(gray_u8):
    """[H,W] uint8 -> [H,W] float64: Laplacian of the 5x5 box mean."""
    g = np.pad(np.asarray(gray_u8).astype(np.int64), 2, mode="reflect")
    H, W = gray_u8.shape
    s = np.zeros((H, W), dtype=np.int64)
    for dy in range(5):
        for dx in range(5):
            s += g[dy:dy + H, dx:dx + W]
    b = np.pad(s.astype(np.float64) * (1.0 / 25.0), 1, mode="reflect")
    return b[:-2, 1:-1] + b[1:-1, :-2] + b[1:-1, 2:] + b[2:, 1:-1] - 4.0 * b[1:-1, 1:-1]


def warp_picks(flow):
    """flow [2,H,W] float32 -> [H,W] int64: index of the pixel `warp(., flow, mode='nearest')` picks, -1 outside.  Separately rounded fp32 operations:
    v = x + fx;  g = 2 v / max(W-1, 1) - 1;  i = ((g + 1) W - 1) / 2 (grid_sample without align_corners);  round half to even."""
    f32 = np.float32
    flow = np.asarray(flow, dtype=f32)
    _, H, W = flow.shape
    ys, xs = np.meshgrid(np.arange(H, dtype=f32), np.arange(W, dtype=f32), indexing="ij")
    gx = f32(2.0) * (xs + flow[0]) / f32(max(W - 1, 1)) - f32(1.0)
    gy = f32(2.0) * (ys + flow[1]) / f32(max(H - 1, 1)) - f32(1.0)
    ix = ((gx + f32(1.0)) * f32(W) - f32(1.0)) / f32(2.0)
    iy = ((gy + f32(1.0)) * f32(H) - f32(1.0)) / f32(2.0)
    assert ix.dtype == f32 and iy.dtype == f32
    rx, ry = np.rint(ix), np.rint(iy)
    ok = (rx >= 0) & (rx < W) & (ry >= 0) & (ry < H)
    return np.where(ok, ry.astype(np.int64) * W + rx.astype(np.int64), -1)


def score_pair(edge1, edge2, flow, border=20):
    """-> (variance of edge 1, variance of the warped float32 edge 2, count, picks, used): population variances in float64 over the used pixels."""
    H, W = edge1.shape
    picks = warp_picks(flow)
    frame = np.zeros((H, W), dtype=bool)
    frame[border:H - border, border:W - border] = True
    used = frame & (picks >= 0) & frame.reshape(-1)[np.maximum(picks, 0)]
    a = np.asarray(edge1, dtype=np.float64)[used]
    b = np.asarray(edge2, dtype=np.float64).astype(np.float32).reshape(-1)[picks[used]].astype(np.float64)
    n = int(used.sum())
    if n == 0:
        return 0.0, 0.0, 0, picks, used
    return float(np.mean((a - a.mean()) ** 2)), float(np.mean((b - b.mean()) ** 2)), n, picks, used
