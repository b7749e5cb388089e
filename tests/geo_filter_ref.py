"""NumPy restatement of csrc/geo_filter.hip (include/hnr.h gives the definitions): the geometric-consistency filter of MVS depth maps in explicitly
fp32, operation-by-operation order -- every array is float32 and every binary operation one rounded fp32 operation -- and the same formulas in fp64
(`dtype=np.float64`: the inverses are then taken in fp64 too).  No code of the package is imported: the GPU tests compare the kernels' bits with the
fp32 form, the fixture's generator measures the reference's fp32 error against the fp64 form."""
import numpy as np

f32 = np.float32


def inverses(K, E, dtype=np.float32):
    """(Kinv [V,3,3], Einv [V,4,4]).  fp32: torch.inverse on the CPU, as the package's host layer forms them; fp64: numpy."""
    if dtype == np.float64:
        return np.linalg.inv(np.asarray(K, np.float64)), np.linalg.inv(np.asarray(E, np.float64))
    import torch
    inv = lambda a: np.stack([torch.inverse(torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32))).numpy() for m in a])
    return inv(K), inv(E)


def mat3(M, a0, a1, a2):
    return [(M[c, 0] * a0 + M[c, 1] * a1) + M[c, 2] * a2 for c in range(3)]


def mat34(T, a0, a1, a2):
    return [((T[c, 0] * a0 + T[c, 1] * a1) + T[c, 2] * a2) + T[c, 3] for c in range(3)]


def pair(A, B):
    """rows 0..2 of A @ B, each entry ((a0*b0 + a1*b1) + a2*b2) + a3*b3"""
    T = np.zeros((3, 4), A.dtype)
    for i in range(3):
        for j in range(4):
            T[i, j] = ((A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]) + A[i, 3] * B[3, j]
    return T


def reproject(depth, K, Kinv, E, Einv, r, s, dtype=np.float32):
    """One ordered pair: dict(xs, ys, sd, depth_rep, dist, rel, ok), all [H,W]."""
    t = dtype
    D = np.asarray(depth, t)
    K, Kinv, E, Einv = (np.asarray(a, t) for a in (K, Kinv, E, Einv))
    V, H, W = D.shape
    fy, fx = np.meshgrid(np.arange(H, dtype=t), np.arange(W, dtype=t), indexing="ij")
    d = D[r]
    with np.errstate(all="ignore"):
        p = mat3(Kinv[r], fx * d, fy * d, d)
        q = mat34(pair(E[s], Einv[r]), *p)
        k = mat3(K[s], *q)
        xs, ys = k[0] / k[2], k[1] / k[2]
        cx, cy = np.fmin(np.fmax(xs, t(0)), t(W - 1)), np.fmin(np.fmax(ys, t(0)), t(H - 1))
        x0f, y0f = np.floor(cx), np.floor(cy)
        wx1, wx0, wy1, wy0 = cx - x0f, (x0f + t(1)) - cx, cy - y0f, (y0f + t(1)) - cy
        x0, y0 = np.clip(x0f.astype(np.int64), 0, W - 1), np.clip(y0f.astype(np.int64), 0, H - 1)
        x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
        S = D[s]
        sd = (((wx0 * wy0) * S[y0, x0] + (wx1 * wy0) * S[y0, x1]) + (wx0 * wy1) * S[y1, x0]) + (wx1 * wy1) * S[y1, x1]
        p2 = mat3(Kinv[s], xs * sd, ys * sd, sd)
        q2 = mat34(pair(E[r], Einv[s]), *p2)
        k2 = mat3(K[r], *q2)
        xr, yr = k2[0] / k2[2], k2[1] / k2[2]
        ex, ey = xr - fx, yr - fy
        dist = np.sqrt(ex * ex + ey * ey)
        rel = np.abs(q2[2] - d) / d
        ok = (dist < t(1)) & (rel < (f32(0.01) if t == np.float32 else 0.01))
    return dict(xs=xs, ys=ys, sd=sd, depth_rep=q2[2], dist=dist, rel=rel, ok=ok)


def geo_consistency(depth, K, Kinv, E, Einv, dtype=np.float32):
    """hnr_geo_consistency: (count [V,H,W] int32, depth_avg [V,H,W])."""
    t = dtype
    D = np.asarray(depth, t)
    V = D.shape[0]
    count, avg = np.zeros(D.shape, np.int32), np.zeros(D.shape, t)
    for r in range(V):
        cnt, acc = np.zeros(D.shape[1:], np.int32), np.zeros(D.shape[1:], t)
        for s in range(V):
            if s == r:
                continue
            o = reproject(D, K, Kinv, E, Einv, r, s, t)
            cnt = cnt + o["ok"].astype(np.int32)
            acc = acc + np.where(o["ok"], o["depth_rep"], t(0))
        count[r], avg[r] = cnt, (acc + D[r]) / (cnt + 1).astype(t)
    return count, avg


def conf_table():
    """the ten factors of reassign_conf, by the reference's own torch expression (filter_utils.py:296) on k = 1..10"""
    import torch
    return (1 - 1.0 / torch.pow(1.14869, torch.arange(1, 11, dtype=torch.int32))).numpy().astype(np.float32)


def select(cam_xyz, conf, points_mask, count, depth_avg, Einv, conf_thresh, geo_cnsst_num, ranges, table=None, dtype=np.float32):
    """hnr_geo_filter_select: dict(world [n,3], cam [n,3], conf [n], view [n] int32, view_counts [V] int64, keep [V,H,W] bool), views ascending,
    row-major pixels."""
    t = dtype
    cam_xyz, conf, avg, Einv = np.asarray(cam_xyz, t), np.asarray(conf, np.float32), np.asarray(depth_avg, t), np.asarray(Einv, t)
    count, pm = np.asarray(count), np.asarray(points_mask) != 0
    V = cam_xyz.shape[0]
    r = np.asarray(ranges, np.float32).astype(t)
    out = dict(world=[], cam=[], conf=[], view=[], view_counts=np.zeros((V,), np.int64), keep=np.zeros(count.shape, bool))
    for v in range(V):
        keep = (conf[v] > f32(conf_thresh)) & pm[v]
        if V > 1:
            keep &= count[v] >= int(geo_cnsst_num)
        cam = np.stack([cam_xyz[v, ..., 0], cam_xyz[v, ..., 1], avg[v]], axis=-1)
        w = np.stack(mat34(Einv[v], cam[..., 0], cam[..., 1], cam[..., 2]), axis=-1)
        if not np.asarray(ranges, np.float32)[0] <= f32(-99):
            with np.errstate(invalid="ignore"):
                keep &= np.all(w >= r[:3], axis=-1) & np.all(w <= r[3:], axis=-1)
        c = conf[v][keep]
        if table is not None:
            k = np.clip(count[v][keep] - int(geo_cnsst_num) + 1, 1, 10)
            c = c * np.asarray(table, np.float32)[k - 1]
        out["keep"][v] = keep
        out["world"].append(w[keep]); out["cam"].append(cam[keep]); out["conf"].append(c.astype(np.float32))
        out["view"].append(np.full((int(keep.sum()),), v, np.int32)); out["view_counts"][v] = int(keep.sum())
    for k in ("world", "cam", "conf", "view"):
        out[k] = np.concatenate(out[k])
    return out
