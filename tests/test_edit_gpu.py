"""Edited scenes on the GPU: per-point rotations `Rw2c` as a part table through chain_gather_kernel<REC, ROT = true> (csrc/chain.hip).

 * golden parity: tests/golden/render_edit_parts.npz (two parts) and render_edit_uni.npz (the 2-D form) -- the reference's forward over the scene,
   rays and weights of render_scannet_small.npz (tests/golden/make_golden_edit.py) -- with the asserts and tolerances of
   tests/test_render_gpu.py::test_full_path_matches_reference_golden;
 * identity rotations are free (bit-equal to the call without Rw2c), the three input forms agree bit for bit in every renderer mode;
 * the gather entry points on a synthetic plan against the fp32 restatement of tests/edit_ref.py;
 * what is not implemented raises; prune / grow_points keep Rw2c aligned with the points.

View-direction encoding bound: sinf / cosf of an fp32 argument against fp64 of the same argument within 4 ulp of the result, 8 U |ref| + 2^-149
with U = 2^-24 -- the bound the project's fp64 checks use for these functions (tests/backward_glue_ref.py, tests/test_backward_glue_gpu.py: "sincosf
4 ulp"); tests/test_chain_gpu.py itself only compares these columns bit for bit with the per-layer path, which has no rotated form."""
import os
import tempfile

import numpy as np
import pytest
import torch

from tests.golden_io import GOLD, load_render, torch_inputs
from tests import edit_ref

pytestmark = pytest.mark.gpu

TOL_DECODED_SIGMA_REL = 2e-4
TOL_RGB = 2e-4
TOL_RAYCOLOR = 2e-4
TOL_OPACITY = 2e-4
U = 2.0 ** -24

_CACHE = {}


def _setup():
    """Scene, weights and renderer of the twin fixture, built once for this module (nothing in it is changed by a test)."""
    if "s" not in _CACHE:
        from hybridneuralrendering_amd import scenes
        from hybridneuralrendering_amd.aggregator import PointAggregator
        from hybridneuralrendering_amd.render import HybridRenderer
        d = load_render("scannet_small")
        dev = torch.device("cuda:0")
        opt = scenes.default_opt(**d["opt"])
        agg = PointAggregator(opt)
        agg.load_state_dict(d["sd"], strict=True)
        agg = agg.to(dev)
        ti = torch_inputs(d, dev)
        w2c = torch.inverse(ti["c2w_nearest"][0].cpu()).to(dev)
        _CACHE["s"] = (d, ti, opt, agg, HybridRenderer(opt, agg, dev), w2c, dev)
    return _CACHE["s"]


def _cloud(ti, Rw2c=None):
    from hybridneuralrendering_amd.render import PointCloud
    return PointCloud(ti["xyz"], ti["emb"], ti["conf"], ti["pdir"], ti["color"], Rw2c=Rw2c)


def _render(rnd, cloud, d, ti, w2c, **kw):
    near, far = d["near_far"]
    return rnd.render_rays(cloud, ti["raydir"][0], ti["campos"][0], ti["camrotc2w"][0], ti["bg_color"][0], near, far, ti["c2w_nearest"][0],
                           ti["campos_nearest"][0], ti["intrinsic_nearest"][0], ti["images_nearest"][0], w2c_nearest=w2c, **kw)


def _rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return torch.from_numpy((np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)).astype(np.float32))


def _psnr(a, b):
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return 99.0 if mse == 0 else -10.0 * np.log10(mse)


@pytest.mark.parametrize("tag", ["parts", "uni"])
def test_rotated_render_matches_reference_golden(tag):
    d, ti, opt, agg, rnd, w2c, dev = _setup()
    z = np.load(os.path.join(GOLD, "render_edit_%s.npz" % tag), allow_pickle=False)
    part_rot = torch.from_numpy(z["part_rot"]).to(dev)
    if tag == "parts":
        Rw2c = part_rot[torch.from_numpy(z["part"].astype(np.int64)).to(dev)]                # the reference's [N,3,3]
    else:
        Rw2c = part_rot[0]                                                                   # its 2-D form
    cloud = _cloud(ti, Rw2c)
    assert cloud.parts is not None and cloud.parts.n_parts == z["part_rot"].shape[0]
    out = _render(rnd, cloud, d, ti, w2c, want_weights=True, pad=True)
    torch.cuda.synchronize()
    out_np = _render(rnd, cloud, d, ti, w2c, pad=False)
    assert torch.equal(out_np["coarse_raycolor"], out["coarse_raycolor"])
    assert torch.equal(out_np["coarse_point_opacity"], out["coarse_point_opacity"])
    rows = np.nonzero(d["q_ray_mask"])[0]
    np.testing.assert_array_equal(out["ray_mask"].cpu().numpy(), d["q_ray_mask"])
    np.testing.assert_array_equal(out["sample_pidx"].cpu().numpy()[rows], d["q_sample_pidx"])
    dec = out["decoded"].cpu().numpy()[rows]
    ref = z["decoded_features"][0]
    scale = np.maximum(1.0, np.abs(ref[..., 0]))
    err_sigma = np.abs(dec[..., 0] - ref[..., 0]) / scale
    err_rgb = np.abs(dec[..., 1:] - ref[..., 1:])
    bad = (err_rgb.max(-1) > TOL_RGB)
    print("%s: flipped-pixel samples %d of %d, max|dRGB| %.2e (others %.2e), max rel dSigma %.2e" % (
        tag, int(bad.sum()), bad.size, float(err_rgb.max()), float(err_rgb[~bad].max()), float(err_sigma.max())))
    assert bad.sum() <= max(2, int(2e-3 * bad.size)), (int(bad.sum()), float(err_rgb.max()))
    assert err_sigma.max() < TOL_DECODED_SIGMA_REL, float(err_sigma.max())
    # weight / conf_coefficient come from the un-rotated offsets: the twin's (asserted equal to the reference's rotated run by the generator)
    np.testing.assert_allclose(out["weight"].cpu().numpy()[rows], d["weight"][0], rtol=0, atol=2e-6)
    np.testing.assert_allclose(out["conf_coefficient"].cpu().numpy()[rows], d["conf_coefficient"][0], rtol=0, atol=1e-7)
    col = out["coarse_raycolor"].cpu().numpy()
    opa = out["coarse_point_opacity"].cpu().numpy()
    isbg = out["coarse_is_background"].cpu().numpy()
    ok = np.ones(len(col), bool)
    ok[rows[bad.any(-1)]] = False
    print("%s: max|dColor| %.2e  max|dOpacity| %.2e  PSNR %.1f dB" % (tag, float(np.abs(col[ok] - z["full_coarse_raycolor"][0][ok]).max()),
                                                                     float(np.abs(opa - z["full_coarse_point_opacity"][0]).max()),
                                                                     _psnr(col, z["full_coarse_raycolor"][0])))
    assert np.abs(col[ok] - z["full_coarse_raycolor"][0][ok]).max() < TOL_RAYCOLOR
    assert np.abs(opa - z["full_coarse_point_opacity"][0]).max() < TOL_OPACITY
    assert np.abs(isbg - z["full_coarse_is_background"][0][:, 0]).max() < TOL_OPACITY
    assert np.abs(out["blend_weight"].cpu().numpy()[rows] - z["blend_weight"][0][..., 0]).max() < TOL_OPACITY
    assert _psnr(col, z["full_coarse_raycolor"][0]) > 70.0
    # and the picture did move: the twin without rotations is far outside the tolerance
    assert np.abs(col - d["full_coarse_raycolor"][0]).max() > 0.05


def test_identity_rotations_render_bit_equal():
    d, ti, opt, agg, rnd, w2c, dev = _setup()
    n = ti["xyz"].shape[0]
    eye = torch.eye(3, device=dev)
    base = _render(rnd, _cloud(ti), d, ti, w2c)
    forms = [eye.expand(n, 3, 3).contiguous(), eye, (torch.zeros(n, dtype=torch.int32, device=dev), eye[None])]
    for R in forms:
        out = _render(rnd, _cloud(ti, R), d, ti, w2c)
        for k in ("coarse_raycolor", "coarse_point_opacity", "decoded"):
            assert torch.equal(out[k], base[k]), k
    # the kernel's own identity: a table with an identity part beside a rotated one that no point uses runs the ROT kernels
    two = (torch.zeros(n, dtype=torch.int32, device=dev), torch.stack([eye, _rot([0, 0, 1], 0.7).to(dev)]))
    cloud = _cloud(ti, two)
    assert cloud.parts is not None
    out = _render(rnd, cloud, d, ti, w2c)
    for k in ("coarse_raycolor", "coarse_point_opacity", "decoded"):
        assert torch.equal(out[k], base[k]), k


def test_rotation_forms_agree_in_every_renderer_mode():
    from hybridneuralrendering_amd.render import HybridRenderer
    d, ti, opt, agg, rnd0, w2c, dev = _setup()
    n = ti["xyz"].shape[0]
    R = _rot([0.3, -0.5, 0.8], 0.9).to(dev)
    forms = [R.expand(n, 3, 3).contiguous(), R, (torch.zeros(n, dtype=torch.int64, device=dev), R[None])]
    ref = None
    for single_call in (True, False):
        for pad in (True, False):
            for knn in ("reference", "sorted"):
                rnd = HybridRenderer(opt, agg, dev)
                rnd.querier = rnd0.querier                                  # (one grid for all of them)
                rnd.single_call, rnd.knn_order = single_call, knn
                outs = [_render(rnd, _cloud(ti, f), d, ti, w2c, pad=pad, want_weights=(pad and not single_call)) for f in forms]
                for o in outs[1:]:
                    for k in ("coarse_raycolor", "coarse_point_opacity", "decoded"):
                        assert torch.equal(o[k], outs[0][k]), (single_call, pad, knn, k)
                if knn == "reference":
                    # single call, staged, padded, un-padded: one picture
                    ref = outs[0] if ref is None else ref
                    assert torch.equal(outs[0]["coarse_raycolor"], ref["coarse_raycolor"]) and torch.equal(outs[0]["decoded"], ref["decoded"])
    base = _render(rnd0, _cloud(ti), d, ti, w2c)
    assert float((ref["coarse_raycolor"] - base["coarse_raycolor"]).abs().max()) > 0.05


def test_render_image_chunks_carry_the_rotation():
    from hybridneuralrendering_amd import driver
    d, ti, opt, agg, rnd, w2c, dev = _setup()
    z = np.load(os.path.join(GOLD, "render_edit_parts.npz"), allow_pickle=False)
    cloud = _cloud(ti, (torch.from_numpy(z["part"].astype(np.int32)).to(dev), torch.from_numpy(z["part_rot"]).to(dev)))
    near, far = d["near_far"]
    frame = dict(raydir=ti["raydir"], pixel_idx=torch.from_numpy(d["pix"].astype(np.int64)).to(dev), campos=ti["campos"], camrotc2w=ti["camrotc2w"],
                 bg_color=ti["bg_color"], near=near, far=far, h=48, w=64, c2w_nearest=ti["c2w_nearest"], campos_nearest=ti["campos_nearest"],
                 intrinsic_nearest=ti["intrinsic_nearest"], images_nearest=ti["images_nearest"])
    whole = driver.render_image(rnd, cloud, frame, sharded=False)
    chunked = driver.render_image(rnd, cloud, frame, chunk_rays=257, sharded=False)
    assert torch.equal(whole["coarse_raycolor"], chunked["coarse_raycolor"])
    ref = z["full_coarse_raycolor"][0]
    assert _psnr(whole["coarse_raycolor"].cpu().numpy(), ref) > 70.0


# ---------------------------------------------------------------------------------------------------------------- stage level
def _plan(dev, n_rep=1, seed=3):
    """A synthetic plan: 40 rays x 24 slots, 0..8 neighbours per item from 400 points in 3 parts; the valid samples listed by class (8 / 4 / 2 row
    slots), every class ending in a partly filled tile.  n_rep > 1: the big class repeated, for more tiles than the grid has blocks."""
    g = torch.Generator().manual_seed(seed)
    N, R, SR = 400, 40, 24
    xyz = torch.randn(N, 3, generator=g)
    conf = torch.rand(N, generator=g)
    pdir = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    color = torch.rand(N, 3, generator=g)
    part = torch.randint(0, 3, (N,), generator=g, dtype=torch.int32)
    part_rot = torch.stack([torch.eye(3), _rot([0, 0, 1], 0.7), _rot([0.3, -0.5, 0.8], 0.9)])
    cnt = torch.randint(0, 9, (R * SR,), generator=g)
    pidx = torch.randint(0, N, (R * SR, 8), generator=g, dtype=torch.int32)
    pidx[torch.arange(8)[None, :] >= cnt[:, None]] = -1
    loc_w = torch.randn(R, SR, 3, generator=g)
    raydir = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    items = torch.arange(R * SR)
    big, small, tiny = items[cnt > 4], items[(cnt == 3) | (cnt == 4)], items[(cnt == 1) | (cnt == 2)]
    big = big.repeat(n_rep)
    assert len(big) % 16 and len(small) % 32 and len(tiny) % 64                 # partly filled last tiles
    vs = torch.cat([big, small, tiny]).to(torch.int32)
    t = lambda x: x.contiguous().to(dev)
    return dict(N=N, R=R, SR=SR, xyz=t(xyz), conf=t(conf), pdir=t(pdir), color=t(color), part=t(part), part_rot=t(part_rot), pidx=t(pidx.view(R, SR, 8)),
                loc_w=t(loc_w), raydir=t(raydir), vs=t(vs), n=(len(big), len(small), len(tiny)),
                campos=t(torch.tensor([0.1, -0.2, -4.0])), camrot=t(torch.eye(3)))


def _gather(P, rec, rot=True):
    """One of the four entry-point forms -> (pid per tile row, extras per tile row, X5, workspace)."""
    from hybridneuralrendering_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    dev = P["xyz"].device
    nv = int(P["vs"].shape[0])
    counts = torch.zeros(_lib.NCOUNTS, dtype=torch.int64, device=dev)
    counts[_lib.CNT["SAMPLES_VALID"]], counts[_lib.CNT["SAMPLES_SMALL"]], counts[_lib.CNT["SAMPLES_TINY"]] = nv, P["n"][1], P["n"][2]
    ws = torch.zeros((int(L.hnr_chain_workspace_bytes(nv)),), dtype=torch.uint8, device=dev)
    X5 = torch.zeros((nv, 280), dtype=torch.float32, device=dev)
    tail = (p(P["pidx"]), p(P["loc_w"]), p(P["raydir"]), p(P["campos"]), p(P["camrot"]), p(P["vs"]), p(counts), P["SR"], 8, nv, p(ws), p(X5), 280, None, None,
            _lib.stream())
    n_parts = int(P["part_rot"].shape[0]) if rot else 0
    if rec:
        r = torch.full((P["N"], 12), float("nan"), dtype=torch.float32, device=dev)
        _lib.check(L.hnr_point_records_parts(p(P["xyz"]), p(P["conf"]), p(P["pdir"]), p(P["color"]), p(P["part"]), P["N"], p(r), _lib.stream()),
                   "hnr_point_records_parts")
        want = torch.cat([P["xyz"], P["conf"][:, None], P["pdir"], P["color"], P["part"].float()[:, None], torch.zeros((P["N"], 1), device=dev)], dim=1)
        assert torch.equal(r, want)
        _lib.check(L.hnr_chain_gather_rec_parts(p(r), p(P["part_rot"]), n_parts, *tail), "hnr_chain_gather_rec_parts")
    else:
        _lib.check(L.hnr_chain_gather_parts(p(P["xyz"]), p(P["conf"]), p(P["pdir"]), p(P["color"]), p(P["part"]), p(P["part_rot"]), n_parts, *tail),
                   "hnr_chain_gather_parts")
    torch.cuda.synchronize()
    blocks = (nv + 15) // 16 + 2
    n_tiles = (P["n"][0] + 15) // 16 + (P["n"][1] + 31) // 32 + (P["n"][2] + 63) // 64
    aux = ws[blocks * 4 * 8192:][:n_tiles * 4 * 1280].view(n_tiles * 4, 1280)
    pid = aux[:, :128].contiguous().view(torch.int32).reshape(-1)
    ext = aux[:, 256:].contiguous().view(torch.float32).reshape(-1, 8)
    return pid, ext, X5, ws


def _expected(P):
    rs, rk = edit_ref.tile_rows(*P["n"])
    dev = P["xyz"].device
    items = P["vs"].long()
    pidx = P["pidx"].view(-1, 8)[items]
    pid, ext, v, _ = edit_ref.gather_rot_ref(P["xyz"], P["pdir"], P["color"], P["part"], P["part_rot"], pidx, P["loc_w"].view(-1, 3)[items],
                                             P["raydir"][items // P["SR"]])
    rs_t, rk_t = torch.from_numpy(rs).to(dev), torch.from_numpy(rk).to(dev)
    live = rs_t >= 0
    s = rs_t.clamp(min=0)
    pid_rows = torch.where(live, pid[s, rk_t], torch.full_like(rs_t, -1).int())
    ext_rows = torch.where(live[:, None], ext[s, rk_t], torch.zeros((), device=dev))
    ext_rows = torch.cat([ext_rows, torch.zeros((ext_rows.shape[0], 1), device=dev)], dim=1)
    return pid_rows.int(), ext_rows, v, pidx


def test_gather_entry_points_match_the_fp32_restatement():
    dev = torch.device("cuda:0")
    P = _plan(dev)
    assert all(k > 0 for k in P["n"]) and sum(P["n"]) > 300
    pid_e, ext_e, v, pidx = _expected(P)
    # samples whose slots mix parts are in the plan (slot 0 decides the view direction there)
    pp = torch.where(pidx >= 0, P["part"][pidx.clamp(min=0).long()], torch.full_like(pidx, -1))
    mixed = ((pp != pp[:, :1]) & (pidx >= 0)).any(-1)
    assert int(mixed.sum()) > 50
    pid_r, ext_r, X5_r, ws_r = _gather(P, rec=True)
    pid_n, ext_n, X5_n, ws_n = _gather(P, rec=False)
    assert torch.equal(ws_r, ws_n) and torch.equal(X5_r, X5_n)                      # records and four-buffer forms: the same bytes
    assert torch.equal(pid_r, pid_e)
    assert torch.equal(ext_r, ext_e), float((ext_r - ext_e).abs().max())
    ref = edit_ref.viewdir_encoding64(v)
    err = (X5_r[:, 256:280].double() - ref).abs()
    bound = 8 * U * ref.abs() + 2.0 ** -149
    print("view-direction encoding: max error / bound %.3f" % float((err / bound).max()))
    assert bool((err <= bound).all())
    assert bool((X5_r[:, :256] == 0).all())                                         # (the gather writes the 24 encoding columns only)
    # n_parts = 0: the plain kernels -- what hnr_chain_gather_rec / hnr_chain_gather write, and different from the rotated image
    pid0, ext0, X50, ws0 = _gather(P, rec=True, rot=False)
    pid1, ext1, X51, ws1 = _gather(P, rec=False, rot=False)
    assert torch.equal(ws0, ws1) and torch.equal(X50, X51) and torch.equal(pid0, pid_e) and not torch.equal(ext0, ext_e)
    I = dict(P, part_rot=torch.eye(3, device=dev).repeat(3, 1, 1).contiguous())      # identity parts through the ROT kernels: bit-equal to the plain ones
    pidI, extI, X5I, wsI = _gather(I, rec=True)
    assert torch.equal(wsI, ws0) and torch.equal(X5I, X50)


def test_gather_second_grid_stride_trip():
    """More 128-row tiles than the launch has blocks (16384): the tiles of the second trip hold what the restatement says."""
    dev = torch.device("cuda:0")
    P = _plan(dev, n_rep=630)
    n_tiles = (P["n"][0] + 15) // 16 + (P["n"][1] + 31) // 32 + (P["n"][2] + 63) // 64
    assert n_tiles > 16384 + 64
    pid_e, ext_e, v, _ = _expected(P)
    pid_r, ext_r, X5_r, _ = _gather(P, rec=True)
    assert torch.equal(pid_r, pid_e) and torch.equal(ext_r, ext_e)
    first = _plan(dev)
    _, _, X5_1, _ = _gather(first, rec=True)
    nb = first["n"][0]
    assert torch.equal(X5_r[629 * nb:630 * nb, 256:280], X5_1[:nb, 256:280])       # the last repeat of the big class = the small plan's


def test_bad_part_arguments_are_refused():
    from hybridneuralrendering_amd import _lib
    from hybridneuralrendering_amd._lib import HnrError
    L, p = _lib.lib(), _lib.ptr
    dev = torch.device("cuda:0")
    P = _plan(dev)
    x = torch.zeros(64, device=dev)
    for n_parts in (-1, 65537):
        with pytest.raises(HnrError, match="n_parts"):
            _lib.check(L.hnr_chain_gather_rec_parts(p(x), p(P["part_rot"]), n_parts, None, None, None, None, None, None, None, 24, 8, 16, None, None, 280,
                                                    None, None, None), "hnr_chain_gather_rec_parts")
    with pytest.raises(HnrError, match="part index"):
        _lib.check(L.hnr_chain_gather_parts(p(x), p(x), p(x), p(x), None, p(P["part_rot"]), 3, None, None, None, None, None, None, None, 24, 8, 16, None,
                                            None, 280, None, None, None), "hnr_chain_gather_parts")
    with pytest.raises(HnrError, match="d_part_rot"):
        _lib.check(L.hnr_chain_gather_parts(p(x), p(x), p(x), p(x), p(P["part"]), None, 3, None, None, None, None, None, None, None, 24, 8, 16, None,
                                            None, 280, None, None, None), "hnr_chain_gather_parts")
    with pytest.raises(HnrError):
        _lib.check(L.hnr_point_records_parts(p(x), p(x), p(x), p(x), None, 5, p(x), None), "hnr_point_records_parts")


# ---------------------------------------------------------------------------------------------------------------- guards, modules
def _modules(Rw2c_in_checkpoint=None, **opt_over):
    from hybridneuralrendering_amd import scenes
    from hybridneuralrendering_amd.modules import NeuralPoints, NeuralPointsRayMarching, find_blend_function, find_render_function, find_tone_map
    d, ti, _, agg, rnd, w2c, dev = _setup()
    opt = scenes.default_opt(**dict(d["opt"], **opt_over))
    ckpt = {"neural_points.xyz": ti["xyz"].cpu(), "neural_points.points_embeding": ti["emb"].cpu(), "neural_points.points_conf": ti["conf"].cpu(),
            "neural_points.points_dir": ti["pdir"].cpu(), "neural_points.points_color": ti["color"].cpu()}
    if Rw2c_in_checkpoint is not None:
        ckpt["neural_points.Rw2c"] = Rw2c_in_checkpoint.cpu()
    with tempfile.NamedTemporaryFile(suffix=".pth", delete=False) as f:
        torch.save(ckpt, f.name)
        path = f.name
    npts = NeuralPoints(opt.point_features_dim, int(ti["xyz"].shape[0]), opt, dev, checkpoint=path).to(dev)
    os.unlink(path)
    net = NeuralPointsRayMarching(tonemap_func=find_tone_map("off"), render_func=find_render_function("radiance"),
                                  blend_func=find_blend_function("alpha"), aggregator=agg, neural_points=npts, opt=opt,
                                  num_pos_freqs=opt.num_pos_freqs, num_viewdir_freqs=opt.num_viewdir_freqs)
    near, far = d["near_far"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    inp = dict(campos=ti["campos"], raydir=ti["raydir"], bg_color=ti["bg_color"], camrotc2w=ti["camrotc2w"],
               pixel_idx=t(d["pix"].astype(np.float32))[None], near=torch.tensor([[[near]]], device=dev, dtype=torch.float32),
               far=torch.tensor([[[far]]], device=dev, dtype=torch.float32), h=torch.tensor([48], device=dev), w=torch.tensor([64], device=dev),
               intrinsic=t(d["intrinsic"])[None], c2w=t(d["c2w"])[None], c2w_nearest=ti["c2w_nearest"], images_nearest=ti["images_nearest"],
               campos_nearest=ti["campos_nearest"], intrinsic_nearest=ti["intrinsic_nearest"], vid_angle_nearest=torch.zeros(1, 4, device=dev),
               frame_weight_nearest=torch.ones(1, 4, device=dev))
    return d, ti, opt, npts, net, inp, dev


def test_unsupported_combinations_raise(monkeypatch):
    from hybridneuralrendering_amd._lib import HnrError
    from hybridneuralrendering_amd.render import HybridRenderer
    from hybridneuralrendering_amd.train import TrainPath, train_step, render_train, CapturedTrainStep
    d, ti, opt, agg, rnd, w2c, dev = _setup()
    R = _rot([0, 0, 1], 0.7).to(dev)
    cloud = _cloud(ti, R)
    # HNR_DENSE=f32
    monkeypatch.setenv("HNR_DENSE", "f32")
    r32 = HybridRenderer(opt, agg, dev)
    r32.querier = rnd.querier
    monkeypatch.delenv("HNR_DENSE")
    assert r32.dense == "f32"
    with pytest.raises(HnrError, match="HNR_DENSE"):
        _render(r32, cloud, d, ti, w2c)
    _render(r32, _cloud(ti, torch.eye(3, device=dev)), d, ti, w2c)                  # (an identity is no rotation)
    # the training path
    near, far = d["near_far"]
    args = (ti["raydir"][0][:64].contiguous(), ti["campos"][0], ti["camrotc2w"][0], ti["bg_color"][0], near, far, ti["c2w_nearest"][0], ti["campos_nearest"][0],
            ti["intrinsic_nearest"][0], ti["images_nearest"][0])
    path = TrainPath(rnd)
    with pytest.raises(HnrError, match="Rw2c"):
        path.forward(cloud, *args)
    buf = (ti["xyz"], ti["emb"], ti["conf"], ti["pdir"], ti["color"])
    gt = torch.zeros(64, 3, device=dev)
    with pytest.raises(HnrError, match="Rw2c"):
        train_step(path, agg, *buf, *args, gt, Rw2c=R)
    with pytest.raises(HnrError, match="Rw2c"):
        render_train(path, agg, *buf, *args, Rw2c=R)
    with pytest.raises(HnrError, match="Rw2c"):
        CapturedTrainStep(path, agg, *buf, dict(raydir=args[0]), near, far, Rw2c=R)
    # the modules: training and prob = 1
    _, _, opt_t, npts, net, inp, _ = _modules(is_train=1)
    npts.editing_set_points(npts.xyz.detach(), npts.points_embeding.detach(), points_color=npts.points_color.detach(), points_dir=npts.points_dir.detach(),
                            points_conf=npts.points_conf.detach(), Rw2c=R)
    with pytest.raises(HnrError, match="Rw2c"):
        net(**inp)
    _, _, _, npts, net, inp, _ = _modules(Rw2c_in_checkpoint=R, prob=1)
    with pytest.raises(HnrError, match="prob"):
        with torch.no_grad():
            net(**inp)
    with pytest.raises(HnrError, match="eulers"):
        npts.set_points(npts.xyz.detach(), npts.points_embeding.detach(), eulers=torch.zeros(3, device=dev))


def test_modules_carry_Rw2c_through_checkpoint_set_prune_and_grow():
    from hybridneuralrendering_amd import edit
    z = np.load(os.path.join(GOLD, "render_edit_parts.npz"), allow_pickle=False)
    part = torch.from_numpy(z["part"].astype(np.int64))
    part_rot = torch.from_numpy(z["part_rot"])
    full = part_rot[part]
    d, ti, opt, npts, net, inp, dev = _modules(Rw2c_in_checkpoint=full)
    assert torch.equal(npts.Rw2c.cpu(), full)
    with torch.no_grad():
        out = net(**inp)
    rows = np.nonzero(d["q_ray_mask"])[0]
    assert np.abs(out["coarse_raycolor"][0].cpu().numpy() - z["full_coarse_raycolor"][0][rows]).max() < TOL_RAYCOLOR
    # the 14-tuple's sampled_Rw2c: gathered per neighbour, empty slots read point 0 (neural_points.py:711,720)
    tup = npts({k: inp[k] for k in ("pixel_idx", "camrotc2w", "campos", "near", "far", "h", "w", "intrinsic", "raydir")})
    pidx = torch.from_numpy(d["q_sample_pidx"]).long().clamp(min=0)
    assert torch.equal(tup[1][0].cpu(), full[pidx])
    # editing_set_points with edit.compose's table = the same cloud
    state = {"neural_points.xyz": ti["xyz"], "neural_points.points_embeding": ti["emb"], "neural_points.points_conf": ti["conf"],
             "neural_points.points_dir": ti["pdir"], "neural_points.points_color": ti["color"], "neural_points.Rw2c": full.to(dev)}
    _, _, _, npts2, net2, _, _ = _modules()
    edit.apply(npts2, edit.compose([edit.load_part(state)]))
    with torch.no_grad():
        out2 = net2(**inp)
    assert torch.equal(out2["coarse_raycolor"], out["coarse_raycolor"])
    # prune: the surviving cloud set afresh renders the same
    conf = npts.points_conf.detach().clone()
    conf[0, ::3, 0] = 0.01
    npts.points_conf = torch.nn.Parameter(conf, requires_grad=False)
    keep = conf[0, :, 0] >= 0.1
    npts.prune(0.1)
    assert torch.equal(npts.Rw2c.cpu(), full[keep.cpu()])
    with torch.no_grad():
        pruned = net(**inp)
    _, _, _, npts3, net3, _, _ = _modules()
    npts3.set_points(ti["xyz"][keep], ti["emb"][:, keep], points_color=ti["color"][:, keep], points_dir=ti["pdir"][:, keep], points_conf=conf[:, keep], parameter=True,
                     Rw2c=full.to(dev)[keep])
    with torch.no_grad():
        fresh = net3(**inp)
    assert torch.equal(pruned["coarse_raycolor"], fresh["coarse_raycolor"]) and torch.equal(pruned["ray_mask"], fresh["ray_mask"])
    # grow: the dropped points come back at the end with their rotations
    drop = ~keep
    npts.grow_points(ti["xyz"][drop], ti["emb"][0, drop], ti["color"][0, drop], ti["pdir"][0, drop], conf[0, drop], add_Rw2c=full.to(dev)[drop])
    order = torch.cat([torch.nonzero(keep)[:, 0], torch.nonzero(drop)[:, 0]])
    assert torch.equal(npts.Rw2c.cpu(), full[order.cpu()])
    with torch.no_grad():
        grown = net(**inp)
    npts3.set_points(ti["xyz"][order], ti["emb"][:, order], points_color=ti["color"][:, order], points_dir=ti["pdir"][:, order], points_conf=conf[:, order], parameter=True,
                     Rw2c=(part.to(dev)[order], part_rot.to(dev)))
    with torch.no_grad():
        fresh = net3(**inp)
    assert torch.equal(grown["coarse_raycolor"], fresh["coarse_raycolor"])
