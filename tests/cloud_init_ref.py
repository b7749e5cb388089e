"""NumPy restatement of csrc/cloud_init.hip: the four stages of the depth-frame cloud initialisation in explicitly fp32, operation-by-operation
order (include/hnr.h gives the orders).  Every array below is float32 and every binary operation is one rounded fp32 operation; sums over a voxel are
sequential, in pixel order.  No code of the package is imported: the GPU tests compare the kernels' bits with these."""
import numpy as np

f32 = np.float32


def _f(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def backproject(depth, Ki, c2w, depth_div=1000.0, depth_min=0.3, depth_max=8.0):
    """depth [H,W] uint16 or float32 -> (world [H*W,3] of every pixel, kept [H*W] bool), row-major pixels."""
    depth = np.asarray(depth)
    H, W = depth.shape
    if depth.dtype == np.uint16:
        d = depth.astype(np.float32) / f32(depth_div)
    else:
        d = depth.astype(np.float32).copy()
    with np.errstate(invalid="ignore"):
        d[(d > f32(depth_max)) | (d < f32(depth_min))] = f32(0)
    d = d.reshape(-1)
    py, px = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    v0, v1, v2 = px.reshape(-1) * d, py.reshape(-1) * d, d
    Ki, M = _f(Ki).reshape(3, 3), _f(c2w).reshape(4, 4)
    cam = [(v0 * Ki[c, 0] + v1 * Ki[c, 1]) + v2 * Ki[c, 2] for c in range(3)]
    world = [((cam[0] * M[c, 0] + cam[1] * M[c, 1]) + cam[2] * M[c, 2]) + M[c, 3] for c in range(3)]
    with np.errstate(invalid="ignore"):
        kept = cam[2] > f32(0)
    return np.stack(world, axis=-1).astype(np.float32), kept


def space_of(pts, vox_res):
    """(space_min [3], vox_size) of mvs_utils.py:507-513 in fp32."""
    mn, mx = pts.min(axis=0), pts.max(axis=0)
    edge = f32(np.max(mx - mn) * f32(1.05))
    space_min = ((mx + mn) / f32(2) - edge / f32(2)).astype(np.float32)
    return space_min, f32(edge / f32(vox_res))


def cells_of(pts, space_min, vox_size, top=None):
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.floor((pts - space_min[None]) / vox_size)
    q = np.where(q >= 0, q, f32(0))                               # (NaN of a degenerate frame -> cell 0)
    if top is not None:
        q = np.minimum(q, f32(top))
    return q.astype(np.int64)


def vox_centroids(pts, vox_res):
    """construct_vox_points_xyz: (centroids [V,3] in lexicographic cell order, cells [V,3], inverse [n])."""
    pts = _f(pts)
    if pts.shape[0] == 0:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), np.zeros((0,), np.int64)
    bits = 1
    while (1 << bits) < int(vox_res) + 2:
        bits += 1
    smin, vsz = space_of(pts, vox_res)
    cell = cells_of(pts, smin, vsz, (1 << bits) - 1)
    key = (cell[:, 0] << (2 * bits)) | (cell[:, 1] << bits) | cell[:, 2]
    order = np.argsort(key, kind="stable")
    ks = key[order]
    heads = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    ends = np.concatenate([heads[1:], [len(ks)]])
    cen = np.zeros((len(heads), 3), np.float32)
    inv = np.zeros((len(ks),), np.int64)
    for v, (s, e) in enumerate(zip(heads, ends)):
        acc = np.zeros((3,), np.float32)
        for p in order[s:e]:
            acc = acc + pts[p]
        cen[v] = acc / f32(e - s)
        inv[order[s:e]] = v
    return cen, cell[order[heads]], inv


def fuse_frame(depth, Ki, c2w, frame_vox_res=100, depth_div=1000.0, depth_min=0.3, depth_max=8.0):
    """One hnr_depth_fuse_frame call: the points it appends."""
    world, kept = backproject(depth, Ki, c2w, depth_div, depth_min, depth_max)
    pts = world[kept]
    if frame_vox_res <= 0 or pts.shape[0] == 0:
        return pts
    return vox_centroids(pts, frame_vox_res)[0]


def range_crop(pts, ranges):
    pts, r = _f(pts), _f(ranges)
    if r[0] <= f32(-99):
        return pts
    with np.errstate(invalid="ignore"):
        m = np.all(pts >= r[None, :3], axis=1) & np.all(pts <= r[None, 3:], axis=1)
    return pts[m]


def view_scores(xyz, campos, camdir):
    """[N,M] fp32 scores of nearest_view."""
    p, c, r = _f(xyz)[:, None, :], _f(campos)[None], _f(camdir)[None]
    d = p - c
    n = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    u = d / (n + f32(1e-6))[..., None]
    return n / f32(200) + (f32(1.1) - ((u[..., 0] * r[..., 0] + u[..., 1] * r[..., 1]) + u[..., 2] * r[..., 2]))


def nearest_view(xyz, campos, camdir, chunk=4096):
    xyz = _f(xyz)
    out = np.zeros((xyz.shape[0],), np.int32)
    for s in range(0, xyz.shape[0], chunk):
        out[s:s + chunk] = np.argmin(view_scores(xyz[s:s + chunk], campos, camdir), axis=1)        # first minimum
    return out


def project(xyz, w2c, K):
    """(cam [n,3], gx [n], gy [n]) of hnr_point_view_attrs."""
    xyz, Wm, K = _f(xyz), _f(w2c).reshape(4, 4), _f(K).reshape(3, 3)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    cam = [((x * Wm[c, 0] + y * Wm[c, 1]) + z * Wm[c, 2]) + Wm[c, 3] for c in range(3)]
    with np.errstate(invalid="ignore", divide="ignore"):
        q0, q1 = cam[0] / cam[2], cam[1] / cam[2]
        gx = (q0 * K[0, 0] + q1 * K[0, 1]) + K[0, 2]
        gy = (q0 * K[1, 0] + q1 * K[1, 1]) + K[1, 2]
    return np.stack(cam, axis=-1), gx, gy


def view_attrs(xyz, w2c, c2w, cpc, K, H, W, feat=None):
    """(features [n,C] or None, dir [n,3], mask [n] uint8)."""
    cam, gx, gy = project(xyz, w2c, K)
    with np.errstate(invalid="ignore"):
        mask = (gx >= f32(0)) & (gx <= f32(W - 1)) & (gy >= f32(0)) & (gy <= f32(H - 1))
    cpc, R = _f(cpc).reshape(3), _f(c2w).reshape(4, 4)[:3, :3]
    e = cam - cpc[None]
    den = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]) + f32(1e-6)
    u = e / den[:, None]
    pdir = np.stack([(u[:, 0] * R[c, 0] + u[:, 1] * R[c, 1]) + u[:, 2] * R[c, 2] for c in range(3)], axis=-1).astype(np.float32)
    out = None
    if feat is not None:
        feat = _f(feat)
        C, Hl, Wl = feat.shape
        out = np.zeros((cam.shape[0], C), np.float32)
        idx = np.flatnonzero(mask)
        sx = (gx[idx] * f32(Wl - 1)) / f32(W - 1)
        sy = (gy[idx] * f32(Hl - 1)) / f32(H - 1)
        x0f, y0f = np.floor(sx), np.floor(sy)
        x1f, y1f = x0f + f32(1), y0f + f32(1)
        wx0, wx1, wy0, wy1 = x1f - sx, sx - x0f, y1f - sy, sy - y0f
        w00, w01, w10, w11 = wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        pad = np.zeros((C, Hl + 2, Wl + 2), np.float32)           # zero padding: texel (y, x) sits at (y + 1, x + 1)
        pad[:, 1:-1, 1:-1] = feat
        tex = lambda yy, xx: pad[:, np.clip(yy + 1, 0, Hl + 1), np.clip(xx + 1, 0, Wl + 1)].T
        val = ((w00[:, None] * tex(y0, x0) + w01[:, None] * tex(y0, x0 + 1)) + w10[:, None] * tex(y0 + 1, x0)) + w11[:, None] * tex(y0 + 1, x0 + 1)
        out[idx] = val
    return out, pdir, mask.astype(np.uint8)
