"""Generates tests/golden/geo_filter.npz by running the REFERENCE's own geometric-consistency filter (models/mvs/filter_utils.py) on a small synthetic
scene, on the CPU.  Needs the reference checkout (tests/golden/_ref_import.py); the fixture holds data only.

Reference functions called (none is copied):
  models/mvs/filter_utils.py  filter_by_masks_gpu (with reassign_conf and range_mask_torch), check_geometric_consistency_gpu,
                              reproject_with_depth_gpu
The per-pixel count and averaged depth of ALL pixels (filter_by_masks_gpu returns the kept ones only) are accumulated here from
check_geometric_consistency_gpu's own masks and reprojected depths, by the three expressions of filter_utils.py:256-259.

Scene: 6 views of 48 x 64 looking at a tilted plane from displaced poses (view 4 has its own intrinsic), 0.2 % multiplicative depth noise, per view one
block scaled by 1.05 and one hole of zeros, a confidence map on both sides of depth_conf_thresh, geo_cnsst_num = 3, `ranges` cutting off a strip; a
second record with default_conf > 1 (reassign_conf).

Boundary conditions ENFORCED here (asserted before the file is written), so that the reference alone decides every mask and nothing has to be left out
of a comparison:
  * no pair-pixel has its distance within `margin_dist` of 1 px or its relative depth difference within `margin_rel` of 0.01;
  * no point that passes the final mask lies within `margin_world` of a `ranges` face;
  * no confidence lies within 1e-4 of depth_conf_thresh (by construction of the map).
Offending reference pixels are zeroed and everything is re-run until this holds.  The margins are MEASURED on this scene: each is 4 x the largest
distance between the reference's fp32 value and the fp64 restatement (tests/geo_filter_ref.py with dtype=float64) -- for `dist` and `rel` over the
pair-pixels where either side is below twice the threshold (far from the threshold the values, and their errors, grow without bound and decide
nothing), for the world coordinates over the points that pass the final mask.  The tolerances on depth_averaged (`tol_avg`) and xyz_world
(`tol_world` = margin_world) come from the same measurement; all are stored in the fixture next to the data.

Run:  python tests/golden/make_golden_geo_filter.py
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

V, H, W = 6, 48, 64
CONF_THRESH, GEO_NUM = 0.7, 3


def look_at(pos, target):
    """w2c (OpenCV: +z forward, +y down) of a camera at pos looking at target."""
    pos, target = np.asarray(pos, np.float64), np.asarray(target, np.float64)
    z = target - pos; z /= np.linalg.norm(z)
    x = np.cross(np.array([0.0, 0.0, 1.0]), z); x /= np.linalg.norm(x)
    y = np.cross(z, x)
    M = np.eye(4)
    M[:3, 0], M[:3, 1], M[:3, 2], M[:3, 3] = x, y, z, pos
    return np.linalg.inv(M).astype(np.float32)


def make_scene(rng):
    K = np.tile(np.array([[60.0, 0.0, 31.5], [0.0, 60.0, 23.5], [0.0, 0.0, 1.0]], np.float32), (V, 1, 1))
    K[4] = np.array([[66.0, 0.0, 30.0], [0.0, 64.5, 25.0], [0.0, 0.0, 1.0]], np.float32)
    E = np.stack([look_at([0.25 * (v - 2.5), -2.0 + 0.05 * v, 1.0 + 0.08 * ((v * 3) % 5 - 2)], [0.05 * v, 1.0, 1.0]) for v in range(V)])
    nrm, off = np.array([0.25, -1.0, 0.15]), -1.0                 # the plane n . X = off (through (0, 1, 0) ...), tilted against every view axis
    depth = np.zeros((V, H, W), np.float32)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    for v in range(V):
        c2w = np.linalg.inv(E[v].astype(np.float64))
        dirs = np.stack([xx, yy, np.ones_like(xx)], -1) @ np.linalg.inv(K[v].astype(np.float64)).T @ c2w[:3, :3].T
        t = (off - c2w[:3, 3] @ nrm) / (dirs @ nrm)               # z of the camera ray is 1: t is the depth
        d = t * (1.0 + 0.002 * rng.standard_normal((H, W)))
        by, bx = 6 + 5 * v, 8 + 7 * v
        d[by:by + 7, bx:bx + 9] *= 1.05
        hy, hx = 30 - 3 * v, 40 - 5 * v
        d[hy:hy + 5, hx:hx + 6] = 0.0
        depth[v] = d.astype(np.float32)
    conf = rng.uniform(0.2, 1.0, size=(V, H, W)).astype(np.float32)
    near = np.abs(conf - np.float32(CONF_THRESH)) < 1e-4
    conf[near] = np.float32(CONF_THRESH + 0.01)
    pmask = rng.uniform(size=(V, H, W)) > 0.03
    return depth, K, E, conf, pmask


def main():
    import make_golden_cloud_init as G                         # _ref_import + the stand-ins for the modules this image lacks (torch_scatter, kornia, ...)
    G.import_reference_modules()
    fu = importlib.import_module("models.mvs.filter_utils")
    fu.tqdm = lambda x, *a, **k: x
    import geo_filter_ref as R
    rng = np.random.default_rng(7)
    depth, K, E, conf, pmask = make_scene(rng)
    Kt, Et = torch.from_numpy(K), torch.from_numpy(E)
    fy, fx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")

    def ref_pairs(depth):
        """the reference's fp32 (ok, depth_rep, dist, rel) of every ordered pair, [V,V,H,W]"""
        D = torch.from_numpy(depth)
        ok, drep = np.zeros((V, V, H, W), bool), np.zeros((V, V, H, W), np.float32)
        dist, rel = np.full((V, V, H, W), np.inf, np.float32), np.full((V, V, H, W), np.inf, np.float32)
        for r in range(V):
            for s in range(V):
                if s == r:
                    continue
                m, _, dr, _, _ = fu.check_geometric_consistency_gpu(D[r], Kt[r], Et[r], D[s], Kt[s], Et[s])
                ok[r, s], drep[r, s] = m.numpy(), dr.numpy()
                dr2, xr, yr, _, _, _ = fu.reproject_with_depth_gpu(D[r], Kt[r], Et[r], D[s], Kt[s], Et[s])
                dist[r, s] = torch.sqrt((xr - fx) ** 2 + (yr - fy) ** 2).numpy()          # filter_utils.py:209-213 on the reference's own outputs
                rel[r, s] = (torch.abs(dr2 - D[r]) / D[r]).numpy()
        return ok, drep, dist, rel

    def f64_pairs(depth):
        Ki64, Ei64 = R.inverses(K, E, np.float64)
        dist, rel = np.full((V, V, H, W), np.inf), np.full((V, V, H, W), np.inf)
        ok = np.zeros((V, V, H, W), bool)
        for r in range(V):
            for s in range(V):
                if s != r:
                    o = R.reproject(depth, K, Ki64, E, Ei64, r, s, np.float64)
                    dist[r, s], rel[r, s], ok[r, s] = o["dist"], o["rel"], o["ok"]
        return ok, dist, rel

    def near_err(a32, a64, thr):
        with np.errstate(invalid="ignore"):
            m = (np.minimum(a32.astype(np.float64), a64) < 2 * thr) & np.isfinite(a32) & np.isfinite(a64)
            return float(np.abs(a32.astype(np.float64) - a64)[m].max())

    Kinv32, Einv32 = R.inverses(K, E)
    Einv64 = np.linalg.inv(E.astype(np.float64))
    ranges = None
    for it in range(50):
        ok32, drep32, dist32, rel32 = ref_pairs(depth)
        ok64, dist64, rel64 = f64_pairs(depth)
        margin_dist, margin_rel = 4 * near_err(dist32, dist64, 1.0), 4 * near_err(rel32, rel64, 0.01)
        count = ok32.sum(axis=1).astype(np.int32)
        acc = np.zeros((V, H, W), np.float32)
        for s in range(V):                                                                  # filter_utils.py:257, ascending source view
            for r in range(V):
                if s != r:
                    acc[r] = acc[r] + drep32[r, s]
        avg32 = ((torch.from_numpy(acc) + torch.from_numpy(depth)) / (torch.from_numpy(count) + 1)).numpy()
        cam_xyz = np.stack([((torch.inverse(Kt[v]) @ (torch.stack([fx.reshape(-1), fy.reshape(-1), torch.ones(H * W, dtype=torch.long)], 0) *
                                                      torch.from_numpy(depth[v]).reshape(-1))).t().reshape(H, W, 3)).numpy() for v in range(V)])
        pre = (conf > np.float32(CONF_THRESH)) & pmask & (count >= GEO_NUM)                 # final_mask, before the range mask
        cam = np.concatenate([cam_xyz[..., :2], avg32[..., None]], -1)
        world32 = np.stack([(torch.cat([torch.from_numpy(cam[v]), torch.ones(H, W, 1)], -1) @ torch.inverse(Et[v]).t()).numpy()[..., :3] for v in range(V)])
        world64 = np.stack([cam[v].astype(np.float64) @ Einv64[v][:3, :3].T + Einv64[v][:3, 3] for v in range(V)])
        margin_world = 4 * float(np.abs(world32.astype(np.float64) - world64)[pre].max())
        if ranges is None:                                                                  # cut a strip off along x, once, from the first pass
            lo, hi = world64[pre].min(0) - 0.5, world64[pre].max(0) + 0.5
            lo[0] = np.quantile(world64[pre][:, 0], 0.08)
            ranges = np.concatenate([lo, hi]).astype(np.float32)
        with np.errstate(invalid="ignore"):
            bad_pair = ((np.abs(dist64 - 1.0) < margin_dist) | (np.abs(dist32.astype(np.float64) - 1.0) < margin_dist) |
                        (np.abs(rel64 - 0.01) < margin_rel) | (np.abs(rel32.astype(np.float64) - 0.01) < margin_rel)).any(axis=1)
        face = np.abs(world64[..., None, :] - ranges.astype(np.float64).reshape(2, 3)).min(axis=(-1, -2)) < margin_world
        bad = bad_pair | (face & pre)
        print("pass %d: margins dist %.3e rel %.3e world %.3e; %d offending pixels" % (it, margin_dist, margin_rel, margin_world, int(bad.sum())))
        if not bad.any():
            break
        depth[bad] = 0.0
    assert not bad.any(), "the scene did not settle"
    assert np.array_equal(ok32, ok64), "the fp64 restatement disagrees with the reference about a mask away from the thresholds"
    Ki64, Ei64 = R.inverses(K, E, np.float64)
    c64, a64 = R.geo_consistency(depth, K, Ki64, E, Ei64, np.float64)
    assert np.array_equal(c64, count)
    tol_avg = 4 * float(np.abs(avg32.astype(np.float64) - a64).max())
    print("counts 0..5: %s pixels; tol_avg %.3e" % (np.bincount(count.reshape(-1), minlength=V).tolist(), tol_avg))

    out = dict(depth=depth, K=K, E=E, conf=conf, points_mask=pmask.astype(np.uint8), cam_xyz=cam_xyz, count=count, depth_avg=avg32,
               conf_thresh=np.float32(CONF_THRESH), geo_cnsst_num=np.int32(GEO_NUM), ranges=ranges, margin_dist=np.float64(margin_dist),
               margin_rel=np.float64(margin_rel), margin_world=np.float64(margin_world), tol_avg=np.float64(tol_avg), tol_world=np.float64(margin_world))
    for tag, default_conf in (("a", -1.0), ("b", 2.0)):
        opt = types.SimpleNamespace(manual_depth_view=1, depth_conf_thresh=CONF_THRESH, geo_cnsst_num=GEO_NUM, default_conf=default_conf,
                                    far_plane_shift=None, ranges=[float(r) for r in ranges])
        cams, worlds, confs = fu.filter_by_masks_gpu([torch.from_numpy(cam_xyz[v]).reshape(1, 1, 1, H, W, 3) for v in range(V)], [Kt[v][None] for v in range(V)],
                                                     [Et[v][None] for v in range(V)], [torch.from_numpy(conf[v].copy())[None, None] for v in range(V)],
                                                     [torch.from_numpy(pmask[v])[None, None] for v in range(V)], opt)
        n = [int(c.shape[0]) for c in cams]
        print("record %s: %s kept points per view" % (tag, n))
        assert min(n) > 0 and sum(n) < int(pre.sum())                                       # the ranges cut something off
        out["%s_counts" % tag] = np.array(n, np.int64)
        out["%s_conf" % tag] = torch.cat(confs).numpy()
        if tag == "a":
            out["a_cam"], out["a_world"] = torch.cat(cams).numpy(), torch.cat(worlds).numpy()
            w = out["a_world"].astype(np.float64)
            assert (np.abs(w[:, None, :] - ranges.astype(np.float64).reshape(2, 3)).min(axis=(-1, -2)) >= margin_world).all()
        else:
            assert np.array_equal(torch.cat(cams).numpy(), out["a_cam"]) and np.array_equal(torch.cat(worlds).numpy(), out["a_world"])
            assert not np.array_equal(out["b_conf"], out["a_conf"])
    assert (conf > CONF_THRESH).any() and (conf < CONF_THRESH).any() and len(np.unique(count)) == V
    path = os.path.join(HERE, "geo_filter.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 1000000, size
    print("wrote %s (%d bytes)" % (path, size))


if __name__ == "__main__":
    main()
