"""NumPy restatement of csrc/depth_sup.hip: the per-ray ground-truth depth of a batch, the depth term of the training loss with its gradient, and
the depth-error row of a rendered frame (include/hnr.h: hnr_frame_depth_rays, hnr_depth_loss, hnr_depth_metrics).

Every fp32 operation is rounded on its own in the order written; the GPU results that do not depend on a long sum (gt_depth, the gradient, the
counts) must equal these bit for bit.  The definitions:

  value     raw uint16 (carried as int16 with the uint16 bit pattern: a negative v means 65536 + v) -> d = float(raw) / depth_div, a division;
            float32 frames are copied; d = 0 unless depth_min <= d <= depth_max.  0 = no measurement.
  pixel     no depth intrinsic: (u, v) = ((int) px, (int) py), the texel gt_image reads.  Depth intrinsic Kd, colour intrinsic K:
            x = ((px + 0.5) - K02) / K00, y = ((py + 0.5) - K12) / K11 (the batch kernel's plane coordinates), u = (int) floor((x Kd00 + Kd02) + 0.5),
            v = (int) floor((y Kd11 + Kd12) + 0.5): integer pixel = centre.  (u, v) outside the depth frame: 0.
  loss      m = ray_mask > 0 and gt_depth > 0, n = sum m; L = float32(sum m (D - d)^2 / n), 0 when n = 0: each square in fp32 (difference, then
            square), THE SUM IN fp64 in the kernel's fixed order -- 1024 lanes, lane t adds r = t, t + 1024, ... in order; an xor butterfly
            (32, 16, .. 1) over each wave of 64; the sixteen waves in order.  out3 = {L, n, w L}; total += w L (one fp32 add, skipped when n = 0).
  gradient  g = m (D - d) * ((2 w) / float32(n)): the scale once in fp32; exactly 0 where m = 0 or n = 0.
  metrics   over m, in fp64 from the fp32 inputs: {n, sum |e|, sum e^2, sum |e| / d, #(D > 0 and D < 1.25 d and d < 1.25 D)}, e = D - d; the last is
            max(D / d, d / D) < 1.25 without a quotient (both products are exact in fp64); sums in the order above.
"""
import numpy as np

f32 = np.float32
LANES, WAVE = 1024, 64


def depth_value(raw, depth_div=1000.0, depth_min=0.3, depth_max=8.0):
    """raw: uint16, int16 (read as uint16) or float32 (metres) -> float32 depth, 0 outside [depth_min, depth_max]."""
    raw = np.asarray(raw)
    if raw.dtype == np.int16:
        raw = raw.view(np.uint16)
    if raw.dtype == np.uint16:
        d = (raw.astype(f32) / f32(depth_div)).astype(f32)
    else:
        assert raw.dtype == f32
        d = raw.copy()
    ok = (d >= f32(depth_min)) & (d <= f32(depth_max))
    return np.where(ok, d, f32(0)).astype(f32)


def depth_pixels(px, py, Hd, Wd, K=None, Kd=None):
    """px, py float32 [R] -> (u, v int64, inside bool)."""
    px, py = np.asarray(px, f32), np.asarray(py, f32)
    if Kd is None:
        with np.errstate(invalid="ignore"):
            in_u, in_v = (px > f32(-1)) & (px < f32(Wd)), (py > f32(-1)) & (py < f32(Hd))
        u = np.where(in_u, px, f32(0)).astype(np.int32).astype(np.int64)        # astype(int32) truncates toward zero, as (int)
        v = np.where(in_v, py, f32(0)).astype(np.int32).astype(np.int64)
        return u, v, in_u & in_v
    K, Kd = np.asarray(K, f32), np.asarray(Kd, f32)
    x = ((px + f32(0.5)) - K[0, 2]) / K[0, 0]
    y = ((py + f32(0.5)) - K[1, 2]) / K[1, 1]
    fu = np.floor((x * Kd[0, 0] + Kd[0, 2]) + f32(0.5)).astype(f32)
    fv = np.floor((y * Kd[1, 1] + Kd[1, 2]) + f32(0.5)).astype(f32)
    with np.errstate(invalid="ignore"):
        in_u, in_v = (fu >= f32(0)) & (fu < f32(Wd)), (fv >= f32(0)) & (fv < f32(Hd))
    u = np.where(in_u, fu, f32(0)).astype(np.int64)
    v = np.where(in_v, fv, f32(0)).astype(np.int64)
    return u, v, in_u & in_v


def gt_depth(depth_frames, row, px, py, K=None, Kd=None, depth_div=1000.0, depth_min=0.3, depth_max=8.0):
    """depth_frames [F,Hd,Wd]; row: the item's frame row (outside the bank: row 0) -> gt_depth float32 [R]."""
    depth_frames = np.asarray(depth_frames)
    F, Hd, Wd = depth_frames.shape
    row = int(row) if 0 <= int(row) < F else 0
    u, v, inside = depth_pixels(px, py, Hd, Wd, K, Kd)
    d = depth_value(depth_frames[row][v, u], depth_div, depth_min, depth_max)
    return np.where(inside, d, f32(0)).astype(f32)


def ordered_sum(terms):
    """The kernels' fp64 sum of `terms` [R] (float64, zeros where masked out): per lane, butterfly per wave, waves in order."""
    t = np.asarray(terms, np.float64)
    pad = (-len(t)) % LANES
    t = np.concatenate([t, np.zeros(pad)]).reshape(-1, LANES)
    acc = np.zeros(LANES)
    for trip in t:                                  # lane l: r = l, l + 1024, ...
        acc = acc + trip
    idx = np.arange(LANES)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[idx ^ o]
    total = 0.0
    for w in range(LANES // WAVE):
        total = total + acc[w * WAVE]
    return float(total)


def loss_mask(gt, ray_mask):
    return (np.asarray(ray_mask) > 0) & (np.asarray(gt, f32) > 0)


def depth_loss(D, gt, ray_mask, w_depth, total=None):
    """-> (out3 float32 {L, n, w L}, gradient float32 [R], total after the add or None)."""
    D, gt, w = np.asarray(D, f32), np.asarray(gt, f32), f32(w_depth)
    m = loss_mask(gt, ray_mask)
    n = int(m.sum())
    e = (D - gt).astype(f32)
    sq = np.where(m, (e * e).astype(f32), f32(0)).astype(np.float64)
    L = f32(ordered_sum(sq) / n) if n > 0 else f32(0)
    wl = f32(w * L)
    out3 = np.array([L, f32(n), wl], f32)
    if n > 0:
        sc = f32((f32(2) * w) / f32(n))
        g = np.where(m, (e * sc).astype(f32), f32(0)).astype(f32)
    else:
        g = np.zeros_like(D)
    if total is not None:
        total = f32(total) if n == 0 else f32(f32(total) + wl)
    return out3, g, total


def depth_loss_fp64(D, gt, ray_mask):
    """L in fp64 from the fp32 inputs (the reference value of the bound below)."""
    m = loss_mask(gt, ray_mask)
    if not m.any():
        return 0.0
    e = np.asarray(D, np.float64)[m] - np.asarray(gt, np.float64)[m]
    return float(np.mean(e * e))


# |L - L64| <= LOSS_REL_BOUND * L64.  A term: the fp32 difference carries a relative error u = 2^-24, its square 2u + u^2, the rounding of the square
# another u: (1 + u)^3 - 1 < 3.0000004 u per term, and all terms are >= 0, so the same bound holds for their sum; the fp64 additions add at most
# R * 2^-53 (R <= 2^26: 2^-27 <= u / 8), the fp64 quotient 2^-53, the final rounding to fp32 u.  4.2 u covers it.
LOSS_REL_BOUND = 4.2 * 2.0 ** -24


def depth_metrics(D, gt, ray_mask):
    """-> float64 [5] {n, sum |e|, sum e^2, sum |e| / d, #(delta < 1.25)}."""
    m = loss_mask(gt, ray_mask)
    D64, d64 = np.asarray(D, f32).astype(np.float64), np.asarray(gt, f32).astype(np.float64)
    e = np.abs(D64 - d64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(m, e / d64, 0.0)
    d1 = m & (D64 > 0) & (D64 < 1.25 * d64) & (d64 < 1.25 * D64)
    z = lambda a: np.where(m, a, 0.0)
    return np.array([float(m.sum()), ordered_sum(z(e)), ordered_sum(z(e * e)), ordered_sum(rel), float(d1.sum())], np.float64)
