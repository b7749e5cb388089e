"""Cloud initialisation from depth frames, CPU side: the NumPy restatement of the kernels (tests/cloud_init_ref.py) against the fixture the reference
produced (tests/golden/cloud_init.npz, make_golden_cloud_init.py), argument validation of the new entry points and the host logic of
init_cloud_from_depth.

Tolerances come from the arithmetic, not from the code under test.  u = 2^-24 is the unit round-off of fp32.  A chained fp32 dot product of n terms
is within n*u*sum|terms| of the exact value (with the rounding of the operands' own products folded into n); the reference's torch matmul computes
the same dot products in another order (and possibly fused), so it is within the same bound of the exact value, and the two differ by at most twice
the bound.  The generator guarantees that no point or centroid sits within 1e-3 cell of a cell boundary and that view scores are separated by 1e-4,
so cells, voxel sets, picks and views must be EQUAL."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import cloud_init_ref as R
from tests.golden_io import GOLD

U = 2.0 ** -24


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(GOLD, "cloud_init.npz"))
    return {k: z[k] for k in z.files}


def backproject_bound(depth_u16, Ki, c2w):
    """per-element float64 bound E_w [H*W,3] on |fp32 world - exact world| for either implementation"""
    H, W = depth_u16.shape
    d = (depth_u16.astype(np.float32) / np.float32(1000)).astype(np.float64).reshape(-1)
    d[(d > 8.0) | (d < 0.3)] = 0
    py, px = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    v = np.stack([px.reshape(-1) * d, py.reshape(-1) * d, d], -1)
    Ki, M = Ki.astype(np.float64), c2w.astype(np.float64)
    cam = v @ Ki.T
    e_cam = 4 * U * (np.abs(v) @ np.abs(Ki).T)                          # 3 terms + the rounding of v = pixel * d
    e_w = e_cam @ np.abs(M[:3, :3]).T + 4 * U * (np.abs(cam) @ np.abs(M[:3, :3]).T + np.abs(M[:3, 3])[None])
    return e_w


def centroid_bound(pts, inv, e_pt):
    """[V,3] bound on |centroid - reference centroid|: the mean of the members' own bounds + a sequential fp32 sum of cnt terms and the division, on
    both sides: 2 (cnt + 1) u max|member|"""
    V = int(inv.max()) + 1
    cnt = np.bincount(inv, minlength=V).astype(np.float64)
    mean_e = np.stack([np.bincount(inv, weights=e_pt[:, c], minlength=V) for c in range(3)], -1) / cnt[:, None]
    order = np.argsort(inv, kind="stable")
    starts = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(int)
    amax = np.stack([np.maximum.reduceat(np.abs(pts[order, c]), starts) for c in range(3)], -1)
    return mean_e + 2 * (cnt[:, None] + 1) * U * amax, cnt


def frame_slices(counts):
    o = np.concatenate([[0], np.cumsum(counts)])
    return [slice(int(o[i]), int(o[i + 1])) for i in range(len(counts))]


def test_backprojection_matches_the_reference_within_the_dot_product_bound(gold):
    Ki = gold["depth_intrinsic_inv"]
    for i, sl in enumerate(frame_slices(gold["bp_counts"])):
        world, kept = R.backproject(gold["frames"][i], Ki, gold["poses"][i])
        ref = gold["bp_xyz"][sl]
        assert int(kept.sum()) == ref.shape[0]
        bound = 2 * backproject_bound(gold["frames"][i], Ki, gold["poses"][i])[kept]
        err = np.abs(world[kept].astype(np.float64) - ref.astype(np.float64))
        print("frame %d: %d points, max error %.3e, min bound %.3e, worst error/bound %.3f" % (i, ref.shape[0], err.max(), bound.min(), (err / bound).max()))
        assert (err <= bound).all()
    world, kept = R.backproject(gold["frames"][4], Ki, gold["poses"][4])           # the all-zero frame: nothing kept
    assert not kept.any() and R.fuse_frame(gold["frames"][4], Ki, gold["poses"][4], 100).shape == (0, 3)


@pytest.mark.parametrize("res", [12, 100])
def test_frame_voxels_equal_the_reference_and_centroids_are_within_the_bound(gold, res):
    Ki = gold["depth_intrinsic_inv"]
    bp, fu = frame_slices(gold["bp_counts"]), frame_slices(gold["fuse%d_counts" % res])
    for i in range(4):
        world, kept = R.backproject(gold["frames"][i], Ki, gold["poses"][i])
        pts = world[kept]
        cen, cells, inv = R.vox_centroids(pts, res)
        ref_cen = gold["fuse%d_xyz" % res][fu[i]]
        # the reference's voxel of each of its centroids, in the space the reference formed from ITS points (no centroid is within 1e-3 cell of a boundary)
        smin, vsz = R.space_of(gold["bp_xyz"][bp[i]], res)
        ref_cells = R.cells_of(ref_cen, smin, vsz)
        assert cen.shape == ref_cen.shape and np.array_equal(cells, ref_cells)                       # same voxel set, same (lexicographic) order
        e_pt = 2 * backproject_bound(gold["frames"][i], Ki, gold["poses"][i])[kept]
        bound, cnt = centroid_bound(pts, inv, e_pt)
        err = np.abs(cen.astype(np.float64) - ref_cen.astype(np.float64))
        print("res %d frame %d: %d voxels (up to %d points), worst error/bound %.3f" % (res, i, cen.shape[0], int(cnt.max()), (err / bound).max()))
        assert (err <= bound).all()


def test_range_crop_equals_the_reference(gold):
    np.testing.assert_array_equal(R.range_crop(gold["fuse100_xyz"], gold["ranges"]), gold["crop_xyz"])
    assert 0.8 * gold["fuse100_xyz"].shape[0] < gold["crop_xyz"].shape[0] < 0.95 * gold["fuse100_xyz"].shape[0]
    keep_all = np.array([-100, 0, 0, 0, 0, 0], np.float32)
    np.testing.assert_array_equal(R.range_crop(gold["fuse100_xyz"], keep_all), gold["fuse100_xyz"])


def test_final_voxels_and_selected_indices_equal_the_reference(gold):
    from oracle import voxel_oracle as vo
    xyz, res = gold["s2_xyz"], int(gold["s2_res"][0])
    cen, cells, inv = R.vox_centroids(xyz, res)
    np.testing.assert_array_equal(cells, gold["s2_grid"])
    cnt = np.bincount(inv).astype(np.float64)
    amax = np.abs(xyz).max()
    assert (np.abs(cen.astype(np.float64) - gold["s2_centroid"].astype(np.float64)) <= 2 * (cnt[:, None] + 1) * U * amax).all()
    ocen, ogrid, omidx, oinv, _ = vo.construct_vox_points_closest(xyz, res)                          # what the package's stage 3 restates (tests/test_voxel.py)
    np.testing.assert_array_equal(ogrid, gold["s2_grid"])
    np.testing.assert_array_equal(ocen, cen)
    np.testing.assert_array_equal(omidx, gold["s2_min_idx"])


@pytest.mark.parametrize("M", [5, 70])
def test_nearest_view_equals_the_reference(gold, M):
    ind = R.nearest_view(gold["nv_xyz"], gold["nv_campos%d" % M], gold["nv_camdir%d" % M])
    np.testing.assert_array_equal(ind, gold["nv_ind%d" % M][:, 0])
    assert len(np.unique(ind)) > 3


def attr_bounds(gold, fmap):
    """(bound [n] on |sample value - reference|, ulp4): pixel-position bound x largest neighbouring-texel difference + 4 ulp."""
    xyz, Wm, K = gold["at_xyz"].astype(np.float64), gold["at_w2c"].astype(np.float64), gold["at_K"].astype(np.float64)
    H, W = gold["at_image"].shape[1:]
    C, Hl, Wl = fmap.shape
    cam = xyz @ Wm[:3, :3].T + Wm[:3, 3]
    e_cam = 4 * U * (np.abs(xyz) @ np.abs(Wm[:3, :3]).T + np.abs(Wm[:3, 3])[None])
    with np.errstate(divide="ignore", invalid="ignore"):
        q = cam[:, :2] / cam[:, 2:3]
        e_q = (e_cam[:, :2] + np.abs(q) * e_cam[:, 2:3]) / np.abs(cam[:, 2:3]) + U * np.abs(q)
        e_g = e_q @ np.abs(K[:2, :2]).T + 4 * U * (np.abs(q) @ np.abs(K[:2, :2]).T + np.abs(K[:2, 2])[None])
    scale = np.array([(Wl - 1) / (W - 1), (Hl - 1) / (H - 1)])
    # to sample coordinates (two more roundings each side; the reference goes through [-1,1]: four roundings of values up to the map size)
    e_s = 2 * (e_g * scale[None] + 2 * U * np.array([Wl, Hl])[None]) + 4 * U * np.array([Wl, Hl])[None]
    f = fmap.astype(np.float64)
    dmax = max(np.abs(np.diff(f, axis=2)).max(), np.abs(np.diff(f, axis=1)).max())
    ulp4 = 4 * np.spacing(np.float32(np.abs(fmap).max()))
    return (e_s[:, 0] + e_s[:, 1]) * dmax + ulp4


def test_point_attributes_match_the_reference(gold):
    H, W = gold["at_image"].shape[1:]
    cpc = (torch.from_numpy(gold["at_c2w"])[:, 3][None] @ torch.from_numpy(gold["at_w2c"]).t())[0, :3].numpy()
    col, pdir, mask = R.view_attrs(gold["at_xyz"], gold["at_w2c"], gold["at_c2w"], cpc, gold["at_K"], H, W, gold["at_image"])
    feat, _, _ = R.view_attrs(gold["at_xyz"], gold["at_w2c"], gold["at_c2w"], cpc, gold["at_K"], H, W, gold["at_fmap"])
    np.testing.assert_array_equal(mask, gold["at_mask"])
    assert mask[-1] == 1 and R.project(gold["at_xyz"][-1:], gold["at_w2c"], gold["at_K"])[1][0] == np.float32(W - 1)          # the point exactly on gx = W-1
    assert 0 < mask.sum() < len(mask) and (col[mask == 0] == 0).all() and (feat[mask == 0] == 0).all()
    for got, ref, fmap, name in ((col, gold["at_color"], gold["at_image"], "colour"), (feat, gold["at_feat"], gold["at_fmap"], "feature")):
        bound = attr_bounds(gold, fmap)[:, None]
        err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
        m = mask > 0
        print("%s: max error %.3e, worst error/bound %.3f" % (name, err[m].max(), (err[m] / np.broadcast_to(bound, err.shape)[m]).max()))
        assert (err[m] <= np.broadcast_to(bound, err.shape)[m]).all() and (err[~m] == 0).all()
    # unit-vector components, about ten rounded operations of 2^-24 each, threefold margin
    assert np.abs(pdir.astype(np.float64) - gold["at_dir"].astype(np.float64)).max() <= 2e-6
    assert (gold["at_conf"] == 1).all()


def test_restated_bilinear_is_grid_sample():
    """The restatement's sampling rule against torch's F.grid_sample(align_corners=True, zeros) directly, on sample positions given exactly."""
    rng = np.random.default_rng(5)
    fmap = rng.normal(size=(4, 7, 9)).astype(np.float32)
    H, W = 7, 9
    # identity camera, K = I: gx = x / z, gy = y / z with z = 1 -> exact sample positions
    pts = np.stack([rng.uniform(0, W - 1, 300), rng.uniform(0, H - 1, 300), np.ones(300)], -1).astype(np.float32)
    pts[:5, 0], pts[5:10, 1] = [0, W - 1, 3, 8, 4], [0, H - 1, 2, 6, 3]
    eye4, eye3 = np.eye(4, dtype=np.float32), np.eye(3, dtype=np.float32)
    got, _, mask = R.view_attrs(pts, eye4, eye4, np.zeros(3, np.float32), eye3, H, W, fmap)
    g = torch.from_numpy(np.stack([pts[:, 0] / ((W - 1) / 2) - 1, pts[:, 1] / ((H - 1) / 2) - 1], -1).astype(np.float32))[None, None]
    ref = torch.nn.functional.grid_sample(torch.from_numpy(fmap)[None], g, mode="bilinear", padding_mode="zeros", align_corners=True)[0, :, 0].t().numpy()
    assert mask.all()
    np.testing.assert_allclose(got, ref, rtol=0, atol=16 * U * np.abs(fmap).max() * 4)


def test_new_entry_points_reject_bad_arguments_without_touching_the_gpu():
    from hybridneuralrendering_amd import _lib
    L = _lib.lib()
    one, null, bad = ctypes.c_void_p(256), None, -1
    f = lambda n: (ctypes.c_float * n)(*([1.0] * n))
    # (positive sizes need a device -- rocprim sizes its temporaries per architecture -- and are checked in test_cloud_init_gpu.py)
    assert L.hnr_depth_fuse_scratch_bytes(0, 640) < 0 and L.hnr_depth_fuse_scratch_bytes(480, -1) < 0 and L.hnr_depth_fuse_scratch_bytes(1 << 14, 1 << 14) < 0
    args = lambda **k: [k.get("depth", one), 1, k.get("H", 480), k.get("W", 640), k.get("Ki", f(9)), f(16), 1000.0, 0.3, 8.0, k.get("res", 100), one,
                        k.get("cap", 100), k.get("count", one), k.get("status", one), one, k.get("scratch", 1 << 30), null]
    assert L.hnr_depth_fuse_frame(*args(depth=null)) == bad
    assert L.hnr_depth_fuse_frame(*args(Ki=None)) == bad
    assert L.hnr_depth_fuse_frame(*args(count=null)) == bad and L.hnr_depth_fuse_frame(*args(status=null)) == bad
    assert L.hnr_depth_fuse_frame(*args(H=0)) == bad and L.hnr_depth_fuse_frame(*args(W=-3)) == bad
    assert L.hnr_depth_fuse_frame(*args(cap=0)) == bad
    assert b"capacity" in L.hnr_last_error()
    assert L.hnr_depth_fuse_frame(*args(res=1 << 22)) == bad
    assert L.hnr_depth_fuse_frame(*args(scratch=1000)) == bad
    assert b"scratch" in L.hnr_last_error()
    assert L.hnr_range_crop_scratch_bytes(0) < 0 and L.hnr_range_crop_scratch_bytes((1 << 30) + 1) < 0
    assert L.hnr_range_crop(one, one, 100, None, ctypes.c_void_p(512), one, one, 1 << 20, null) == bad
    assert L.hnr_range_crop(null, one, 100, f(6), ctypes.c_void_p(512), one, one, 1 << 20, null) == bad
    assert L.hnr_range_crop(one, one, 0, f(6), ctypes.c_void_p(512), one, one, 1 << 20, null) == bad
    assert L.hnr_range_crop(one, one, 100, f(6), ctypes.c_void_p(512), one, one, 16, null) == bad
    assert L.hnr_nearest_view(null, 10, one, one, 5, one, null) == bad and L.hnr_nearest_view(one, 10, one, one, 5, null, null) == bad
    assert L.hnr_nearest_view(one, 0, one, one, 5, one, null) == bad and L.hnr_nearest_view(one, 10, one, one, 0, one, null) == bad
    va = lambda **k: [k.get("xyz", one), k.get("n", 10), k.get("w2c", f(16)), f(16), f(3), f(9), k.get("H", 48), k.get("W", 64), k.get("feat", one), k.get("C", 3),
                      48, 64, k.get("out", one), one, one, null]
    assert L.hnr_point_view_attrs(*va(xyz=null)) == bad and L.hnr_point_view_attrs(*va(w2c=None)) == bad
    assert L.hnr_point_view_attrs(*va(n=0)) == bad and L.hnr_point_view_attrs(*va(H=1)) == bad and L.hnr_point_view_attrs(*va(C=0)) == bad
    assert L.hnr_point_view_attrs(*va(feat=null)) == bad                                            # samples wanted without a map


def test_host_logic_of_init_cloud_from_depth():
    from types import SimpleNamespace
    from hybridneuralrendering_amd import cloud_init as ci
    from hybridneuralrendering_amd._lib import HnrError
    # grouping: ascending view id, contiguous segments
    assert ci.view_segments(np.array([2, 2, 2, 5, 7, 7], np.int32)) == [(2, 0, 3), (5, 3, 4), (7, 4, 6)]
    assert ci.view_segments(np.array([], np.int32)) == [] and ci.view_segments(np.array([4], np.int32)) == [(4, 0, 1)]
    # default_conf (train_ft.py:761): applied only inside (0, 1)
    for dc, want in ((-1, 1.0), (0.0, 1.0), (0.15, 0.15), (1.0, 1.0), (2.0, 1.0)):
        c = ci.point_conf(4, dc, "cpu")
        assert c.shape == (1, 4, 1) and torch.all(c == np.float32(want))
    with pytest.raises(HnrError, match="resample_pnts"):
        ci.init_cloud_from_depth([], SimpleNamespace(resample_pnts=1), None, None, None)
    with pytest.raises(HnrError):
        ci.init_cloud_from_depth([], SimpleNamespace(resample_pnts=0), torch.zeros(3, 3), torch.zeros(3, 3), None)      # CPU cameras: no fallback
    with pytest.raises(HnrError, match="capacity"):
        ci.DepthFusion(0, "cuda", np.eye(3))
    with pytest.raises(HnrError):
        ci.DepthFusion(10, "cpu", np.eye(3))
    # cam_pos_cam is the reference's expression (mvs_points_model.py:242-244), fp32 on the CPU
    c2w = np.array([[0.6, -0.8, 0, 1.5], [0.8, 0.6, 0, -2.0], [0, 0, 1, 0.7], [0, 0, 0, 1]], np.float32)
    w2c = torch.inverse(torch.from_numpy(c2w)).numpy()
    cpc = ci.cam_pos_cam(c2w, w2c)
    assert cpc.dtype == np.float32 and cpc.shape == (3,) and np.abs(cpc).max() < 1e-5
