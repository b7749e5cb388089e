"""hnr_render_forward: the whole forward path as ONE C-ABI call (csrc/render_forward.hip), no host read between query and composite.
 * renders the reference-generated golden fixtures through the single entry (models/neural_points_volumetric_model.py:257-391);
 * equals the stage-by-stage path bit for bit;
 * a workspace capacity below the number of valid samples is reported in the status word, never written past."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_render_gpu import _setup, _psnr

pytestmark = pytest.mark.gpu


def _render(rnd, cloud, ti, d, **kw):
    near, far = d["near_far"]
    w2c = torch.inverse(ti["c2w_nearest"][0].cpu()).to(ti["raydir"].device)
    return rnd.render_rays(cloud, ti["raydir"][0], ti["campos"][0], ti["camrotc2w"][0], ti["bg_color"][0], near, far, ti["c2w_nearest"][0],
                           ti["campos_nearest"][0], ti["intrinsic_nearest"][0], ti["images_nearest"][0], w2c_nearest=w2c, **kw)


@pytest.mark.parametrize("tag", ["scannet_small", "synth_small"])
def test_single_call_renders_the_reference_golden_and_equals_the_staged_path(tag, monkeypatch):
    d, ti, opt, cloud, rnd = _setup(tag)
    assert rnd.single_call and rnd.dense == "f16x2"
    calls = []
    import hybridneuralrendering_amd.render as RM
    orig = RM.HybridRenderer._single_call
    monkeypatch.setattr(RM.HybridRenderer, "_single_call", lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1])
    # no tensor of the path may be read on the host while the frame is queued
    host_reads = []
    for name in ("cpu", "item", "tolist"):
        f = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, (lambda f, name: lambda self, *a, **k: (host_reads.append(name), f(self, *a, **k))[1])(f, name))
    rnd.feature_map(ti["images_nearest"][0]); rnd.point_table(cloud); rnd.agg.packed_chain(); rnd.agg.packed_mlp3()      # per-checkpoint / per-frame set-up
    rnd.querier._grid_for(cloud.xyz[None])
    near, far = d["near_far"]
    w2c = torch.inverse(ti["c2w_nearest"][0].cpu()).to(ti["raydir"].device)
    host_reads.clear()
    out = rnd.render_rays(cloud, ti["raydir"][0], ti["campos"][0], ti["camrotc2w"][0], ti["bg_color"][0], float(near), float(far), ti["c2w_nearest"][0],
                          ti["campos_nearest"][0], ti["intrinsic_nearest"][0], ti["images_nearest"][0], w2c_nearest=w2c, want_weights=True)
    assert calls and not host_reads, host_reads
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert int(out["status"][0]) == 0 and int(out["status"][1]) == int(out["counts"][6])
    got = out["coarse_raycolor"].cpu().numpy()
    assert np.abs(got - d["full_coarse_raycolor"][0]).max() < 2e-4 and _psnr(got, d["full_coarse_raycolor"][0]) > 70.0
    np.testing.assert_array_equal(out["ray_mask"].cpu().numpy(), d["q_ray_mask"])
    rows = np.nonzero(d["q_ray_mask"])[0]
    np.testing.assert_allclose(out["weight"].cpu().numpy()[rows], d["weight"][0], rtol=0, atol=2e-6)
    # the same kernels driven stage by stage from Python (exactly sized buffers, one host read): identical pixels
    rnd.single_call = False
    ref = _render(rnd, cloud, ti, d, want_weights=True)
    for k in ("coarse_raycolor", "coarse_point_opacity", "coarse_is_background", "decoded", "ray_mask", "weight", "conf_coefficient", "blend_weight"):
        assert torch.equal(out[k], ref[k]), k


def test_workspace_capacity_overflow_is_reported_not_overrun():
    from hybridneuralrendering_amd import _lib, _raycall
    d, ti, opt, cloud, rnd = _setup("scannet_small")
    full = _render(rnd, cloud, ti, d)
    torch.cuda.synchronize()
    n_valid = int(full["counts"][6])
    L, p = _lib.lib(), _lib.ptr
    dev = ti["raydir"].device
    raydir = ti["raydir"][0].contiguous()
    R, SR, K = raydir.shape[0], int(opt.SR), int(opt.K)
    grid, hp = rnd.querier._grid_for(cloud.xyz[None])
    near, far = d["near_far"]
    tmid = rnd.querier._tmid_for(float(near), float(far), opt.z_depth_dim, R, dev)
    fm = rnd.feature_map(ti["images_nearest"][0])
    cap = n_valid - 100
    prm = _raycall.fill_params(_lib.RenderParams(), R, SR, K, tmid, opt.kernel_size, float(np.float32(hp[0] ** 2)), float(np.float32(opt.vsize[2])), 1, 4, cap, 0)
    assert prm.tmid_stride == 0 and prm.cap_samples == cap
    nbytes = int(L.hnr_render_workspace_bytes(ctypes.byref(prm)))
    guard = 4096
    ws, ws_ptr = _raycall.workspace(nbytes + guard, dev)
    off = ws_ptr.value - ws.data_ptr()
    ws[off + nbytes:] = 0xAB
    pk, agg, m3, ptab = rnd.agg.packed(), rnd.agg, rnd.agg.packed_mlp3(), rnd.point_table(cloud)
    w2c = torch.inverse(ti["c2w_nearest"][0].cpu()).to(dev).contiguous()
    cl = _lib.RenderCloud(p(cloud.xyz), p(cloud.conf), p(cloud.dir), p(cloud.color), p(ptab), int(ptab.stride(0)))
    wt = _lib.RenderWeights(p(agg.packed_chain()), p(m3["cf"].packed), p(m3["mw"].packed), p(m3["mx"].packed),
                            p(pk["mw_last_w"]), p(pk["mw_last_b"]), p(pk["fin_w"]), p(pk["fin_b"]), float(pk["slope"]))
    cam = _lib.RenderCamera(p(ti["campos"][0].contiguous()), p(ti["camrotc2w"][0].contiguous()), p(raydir), p(tmid), p(ti["bg_color"][0].contiguous()))
    vw = _lib.RenderViews(p(w2c), p(ti["intrinsic_nearest"][0].contiguous()), p(ti["campos_nearest"][0].contiguous()), p(fm), int(fm.shape[1]), int(fm.shape[2]), None)
    o = _raycall.RayOutputs.alloc(R, SR, K, dev, blend=False, weights=False)
    col, counts, status, out = o.t["coarse_raycolor"], o.t["counts"], o.t["status"], o.struct()
    _lib.check(L.hnr_render_forward(grid.handle, ctypes.byref(prm), ctypes.byref(cl), ctypes.byref(wt), ctypes.byref(cam), ctypes.byref(vw),
                                    ctypes.c_void_p(ws.data_ptr() + off), nbytes, ctypes.byref(out), _lib.stream()), "hnr_render_forward")
    torch.cuda.synchronize()
    assert int(status[0]) == 1 and int(status[1]) == n_valid and int(counts[6]) == cap
    assert bool((ws[off + nbytes:] == 0xAB).all())                                # nothing written past the workspace
    assert bool(torch.isfinite(col).all())
    # rays whose samples all fit below the capacity are complete
    same = (col == full["coarse_raycolor"]).all(dim=1)
    assert int(same.sum()) > 0.9 * R
    # too small a workspace is refused up front
    with pytest.raises(_lib.HnrError):
        _lib.check(L.hnr_render_forward(grid.handle, ctypes.byref(prm), ctypes.byref(cl), ctypes.byref(wt), ctypes.byref(cam), ctypes.byref(vw),
                                        ctypes.c_void_p(ws.data_ptr() + off), nbytes // 2, ctypes.byref(out), _lib.stream()), "hnr_render_forward")


@pytest.mark.parametrize("tag", ["scannet_small", "synth_small"])
def test_fused_merge_stage_equals_its_three_kernel_form(tag):
    """hnr_merge_stage (reprojection + gather + merge-weight MLP + weighted merge in one launch) against hnr_proj_rows + hnr_mlp3_forward +
    hnr_merge on the same frame: same arithmetic except the order of the 64-term dot product of the last merge-weight layer."""
    d, ti, opt, cloud, rnd = _setup(tag)
    rnd.single_call = False
    a = _render(rnd, cloud, ti, d)
    rnd.fuse_merge = False
    b = _render(rnd, cloud, ti, d)
    assert float((a["decoded"] - b["decoded"]).abs().max()) < 2e-6
    assert float((a["coarse_raycolor"] - b["coarse_raycolor"]).abs().max()) < 2e-6
    assert torch.equal(a["decoded"][..., 0], b["decoded"][..., 0])              # densities do not pass through the image branch


@pytest.mark.parametrize("tag", ["scannet_small", "synth_small"])
def test_fused_mixup_stage_equals_its_two_kernel_form(tag):
    """hnr_mixup_stage (color_mixup_block + residual + color_final_block + decode in one launch) against hnr_mlp3_forward + hnr_final_color on the
    same frame: the same arithmetic in the same order, so the decoded rows are equal bit for bit."""
    d, ti, opt, cloud, rnd = _setup(tag)
    rnd.single_call = False
    a = _render(rnd, cloud, ti, d)
    rnd.fuse_mixup = False
    b = _render(rnd, cloud, ti, d)
    assert torch.equal(a["decoded"], b["decoded"])
    assert torch.equal(a["coarse_raycolor"], b["coarse_raycolor"])


def test_c1_chair_batch_through_the_single_call_matches_the_imported_reference():
    """BASELINE config C1 (nerf_synthetic/chair 200x200, one 32x32 = 1024-ray batch, 100 k points, SR 80, P 12, max_o 410000;
    dev_scripts/w_n360/chair_hybrid.sh) on the HIP path: hnr_render_forward against tests/golden/render_c1_chair.npz -- the outputs of the imported
    reference's NeuralPointsRayMarching.forward + fill_invalid on the same batch (models/neural_points_volumetric_model.py:257-391, :87-126)."""
    from tests.golden_io import c1_chair
    from hybridneuralrendering_amd.aggregator import PointAggregator
    from hybridneuralrendering_amd.render import HybridRenderer, PointCloud
    sc, pix, raydir, sd, exp = c1_chair()
    opt = sc.opt
    assert raydir.shape == (1024, 3) and opt.SR == 80 and opt.P == 12 and opt.max_o == 410000 and sc.xyz.shape[0] == 100000
    dev = torch.device("cuda:0")
    agg = PointAggregator(opt)
    agg.load_state_dict(sd, strict=True)
    agg = agg.to(dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rnd = HybridRenderer(opt, agg, dev)
    assert rnd.single_call and rnd.dense == "f16x2" and rnd.knn_order == "reference"
    cloud = PointCloud(t(sc.xyz), t(sc.emb), t(sc.conf), t(sc.dir), t(sc.color))
    out = rnd.render_rays(cloud, t(raydir), t(sc.c2w[:3, 3]), t(sc.c2w[:3, :3]), t(sc.bg_color), sc.near, sc.far, t(sc.c2w_nearest),
                          t(sc.c2w_nearest[:, :3, 3]), t(sc.intrinsic), t(sc.images_nearest), w2c_nearest=torch.inverse(torch.from_numpy(sc.c2w_nearest)).to(dev))
    torch.cuda.synchronize()
    assert "status" in out and int(out["status"][0]) == 0                       # the single-call entry ran; no capacity overflow
    counts = out["counts"].cpu().numpy()
    from hybridneuralrendering_amd._lib import CNT
    assert int(counts[CNT["SAMPLES"]]) == exp["counts"]["n_samples"] and int(counts[CNT["NEIGHBOURS"]]) == exp["counts"]["n_neighbours"]
    np.testing.assert_array_equal(out["ray_mask"].cpu().numpy(), exp["ray_mask"].reshape(-1))
    got = out["coarse_raycolor"].cpu().numpy()
    assert np.abs(got - exp["full_coarse_raycolor"][0]).max() < 2e-4 and _psnr(got, exp["full_coarse_raycolor"][0]) > 70.0       # fp32 max-abs tolerance of the path (1e-4 on the bench frame)
    np.testing.assert_allclose(out["coarse_point_opacity"].cpu().numpy(), exp["full_coarse_point_opacity"][0], rtol=0, atol=2e-4)
    np.testing.assert_allclose(out["coarse_is_background"].cpu().numpy().reshape(-1), exp["full_coarse_is_background"].reshape(-1), rtol=0, atol=2e-4)
