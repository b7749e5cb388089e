"""NumPy restatement of csrc/hull.hip (include/hnr.h gives the definitions): the alpha bits, the visual-hull masking with its ordered compaction and the
occlusion test, in explicitly fp32, operation-by-operation order -- every array is float32 and every binary operation one rounded fp32 operation -- and
the same formulas in fp64 (`dtype=np.float64`).  No code of the package is imported: the GPU tests compare the kernels' bits with the fp32 form, the
fixture's generator (tests/golden/make_golden_hull.py) measures the reference's fp32 error against the fp64 form."""
import numpy as np

f32 = np.float32


def alpha_on(alphas):
    """bool [M,H,W]: alpha > 0.1f (a NaN: false)"""
    with np.errstate(invalid="ignore"):
        return np.asarray(alphas, np.float32) > f32(0.1)


def pack_bits(on):
    """bool [M,H,W] -> uint32 [M,H,(W+31)//32]: bit (x & 31) of word x >> 5, padding bits 0 (hnr_alpha_pack)"""
    on = np.asarray(on, bool)
    M, H, W = on.shape
    Wp = (W + 31) // 32
    pad = np.zeros((M, H, Wp * 32), np.uint64)
    pad[..., :W] = on
    return (pad.reshape(M, H, Wp, 32) << np.arange(32, dtype=np.uint64)).sum(axis=-1).astype(np.uint32)


def hull_project(xyz, w2c, K, dtype=np.float32):
    """One view of hnr_visual_hull_select: (cam z [n], quotients q [n,2] before the floor)."""
    t = dtype
    xyz, w, K = np.asarray(xyz, np.float32).astype(t), np.asarray(w2c, np.float32).astype(t).reshape(4, 4), np.asarray(K, np.float32).astype(t).reshape(3, 3)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    cam = [((x * w[q, 0] + y * w[q, 1]) + z * w[q, 2]) + w[q, 3] for q in range(3)]
    p = [(cam[0] * K[q, 0] + cam[1] * K[q, 1]) + cam[2] * K[q, 2] for q in range(3)]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return cam[2], np.stack([p[0] / p[2], p[1] / p[2]], axis=-1)


def near_far_bounds(near_far, dtype=np.float32):
    """(near - 1, far): the difference in double; fp32: both rounded to float32, as the host layer forms them"""
    near, far = (float(v) for v in np.asarray(near_far, np.float64).reshape(2))
    return dtype(near - 1.0), dtype(far)


def hull_view_pass(xyz, on_v, w2c, K, near_far=None, range_mask=False, dtype=np.float32):
    """bool [n]: the points that pass ONE view (on_v: bool [H,W])."""
    t = dtype
    H, W = on_v.shape
    z, q = hull_project(xyz, w2c, K, t)
    uf, vf = np.floor(q[:, 0]), np.floor(q[:, 1])
    with np.errstate(invalid="ignore"):
        inside = (uf >= 0) & (uf < W) & (vf >= 0) & (vf < H)
        u = np.where(np.isfinite(uf), np.clip(uf, 0, W - 1), 0).astype(np.int64)         # the clamp in float, then the conversion; not finite: pixel 0
        v = np.where(np.isfinite(vf), np.clip(vf, 0, H - 1), 0).astype(np.int64)
        ok = on_v[v, u]
        if range_mask:
            ok = ok | ~inside
        if near_far is not None:
            lo, hi = near_far_bounds(near_far, t)
            ok = ok & (z >= lo) & (z <= hi)
    return ok


def visual_hull(xyz, on, w2cs, Ks, near_far=None, range_mask=False, dtype=np.float32):
    """hnr_visual_hull_select's mask: bool [n], true where every view passes (on: bool [M,H,W])."""
    keep = np.ones((np.asarray(xyz).shape[0],), bool)
    for m in range(on.shape[0]):
        keep &= hull_view_pass(xyz, on[m], w2cs[m], Ks[m], near_far, range_mask, dtype)
    return keep


def select(mask, capacity, *arrays):
    """The ordered compaction: (count, overflow, the first min(count, capacity) survivors of every array, in input order)."""
    idx = np.flatnonzero(mask)
    return int(idx.size), bool(idx.size > capacity), [np.asarray(a)[idx[:capacity]] for a in arrays]


def view_project(xyz, w2c, K, dtype=np.float32):
    """view_project of csrc/view_attrs.h: (cam [n,3], gx [n], gy [n])."""
    t = dtype
    xyz, w, K = np.asarray(xyz, np.float32).astype(t), np.asarray(w2c, np.float32).astype(t).reshape(4, 4), np.asarray(K, np.float32).astype(t).reshape(3, 3)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    cam = [((x * w[c, 0] + y * w[c, 1]) + z * w[c, 2]) + w[c, 3] for c in range(3)]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        q0, q1 = cam[0] / cam[2], cam[1] / cam[2]
        gx = (q0 * K[0, 0] + q1 * K[0, 1]) + K[0, 2]
        gy = (q0 * K[1, 0] + q1 * K[1, 1]) + K[1, 2]
    return np.stack(cam, axis=-1), gx, gy


def occlusion(xyz, w2c, K, H, W, tolerate=0.1, dtype=np.float32, details=False):
    """hnr_point_occlusion: uint8 [n].  details: also (in_frame [n], cell [n] (-1 outside), z [n], zmin of the point's cell [n] (inf outside))."""
    t = dtype
    cam, gx, gy = view_project(xyz, w2c, K, t)
    z = cam[:, 2]
    with np.errstate(invalid="ignore"):
        inside = (gx >= 0) & (gx <= W - 1) & (gy >= 0) & (gy <= H - 1)
    cell = np.full(z.shape, -1, np.int64)
    cell[inside] = np.ceil(gx[inside]).astype(np.int64) * H + np.ceil(gy[inside]).astype(np.int64)
    zbuf = np.full((H * W,), np.inf, t)
    np.minimum.at(zbuf, cell[inside], z[inside])
    zmin = np.full(z.shape, np.inf, t)
    zmin[inside] = zbuf[cell[inside]]
    vis = inside.copy()
    vis[inside] = z[inside] <= zmin[inside] + t(np.float32(tolerate))
    return (vis.astype(np.uint8), inside, cell, z, zmin) if details else vis.astype(np.uint8)


def embed_vis(sd, xyz, image, c2w, w2c, K, visible, conf=None, dtype=None):
    """query_embedding with the occlusion flags (tests/mvs_init_ref.py's restatement; a hidden point has zero features and colour, its direction, and
    still goes through premlp): (emb [n,32], color [n,3], dir [n,3]) as arrays."""
    import torch
    from tests import mvs_init_ref as MR
    dtype = torch.float64 if dtype is None else dtype
    maps = [m[0] for m in MR.feature_pyramid(sd, MR._t(image, dtype)[None], dtype)]
    rows, _ = MR.query_rows(xyz, image, maps, c2w, w2c, K, dtype)
    rows = rows.clone()
    rows[~torch.from_numpy(np.asarray(visible) != 0), :59] = 0
    if conf is not None:
        rows[:, 62] = MR._t(np.asarray(conf), dtype)
    emb = MR.premlp(MR.state(sd, dtype), rows)
    return emb.numpy(), rows[:, 56:59].numpy(), rows[:, 59:62].numpy()
