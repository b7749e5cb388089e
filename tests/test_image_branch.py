"""The reference-view ("image") branch without a GPU: the inputs tests/test_image_branch_gpu.py feeds the kernels are what it assumes they are
(tests/image_branch_ref.py) -- the hand-built projection table means what it says, the generated samples truncate to the same pixel in float32 and in
float64 in every view of every case, the float64 restatements are the oracle's / torch's own -- and the test hook hnr_image_features_bwd_bbox refuses
bad arguments before any HIP call."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import image_branch_ref as ib


def _oracle_pixels(xyz, c2w, K, H, W, dtype):
    from oracle import render_oracle as ro
    t = lambda a: torch.as_tensor(a).to(dtype)
    return ro.gathered_pixels(t(xyz)[None], t(c2w)[None], t(K)[None], H, W)[:, 0]                 # [V,n,2]


def test_edge_table_means_what_it_says():
    """The written-out pixels are the oracle's in float64, in float32 (every product of the table is exact), and the restatement's."""
    e = ib.edge_samples()
    assert len(e["names"]) == e["xyz"].shape[0] == e["expect"].shape[1] >= 20
    for dtype, key in ((torch.float32, "expect"), (torch.float64, "expect64")):
        got = _oracle_pixels(e["xyz"], e["c2w"], e["intrinsic"], e["H"], e["W"], dtype)
        bad = [(e["names"][i], v, got[v, i].tolist(), e[key][v, i].tolist()) for v in range(2) for i in range(len(e["names"]))
               if not torch.equal(got[v, i], e[key][v, i])]
        assert not bad, (dtype, bad)
        assert torch.equal(ib.restated_pixels(e["xyz"], e["w2c"], e["intrinsic"], e["H"], e["W"], dtype), e[key])
    # float64 differs from the float32 program only where the table says so -- a non-zero integer coordinate in front of the camera, through the
    # `+ 1e-10` of the denominator -- and the float64 restatement with that one float32 rounding kept is the float32 program
    differs = (e["expect"] != e["expect64"]).any(-1)
    z = torch.as_tensor(e["xyz"])[:, 2]
    assert 8 <= int(differs.sum()) <= 16 and bool((z[None, :].expand(2, -1)[differs] > 0).all())
    assert torch.equal(ib.restated_pixels(e["xyz"], e["w2c"], e["intrinsic"], e["H"], e["W"], torch.float64, den32=True), e["expect"])
    # the float32 and float64 coordinates agree to the bit wherever they are finite and in range
    fx32, fy32 = ib.project(e["xyz"], e["w2c"], e["intrinsic"], torch.float32)
    fx64, fy64 = ib.project(e["xyz"], e["w2c"], e["intrinsic"], torch.float64, den32=True)
    small = fx64.abs() < 1e6
    assert torch.equal(fx32[small].double(), fx64[small]) and int(small.sum()) >= 2 * len(e["names"]) - 12
    small = fy64.abs() < 1e6
    assert torch.equal(fy32[small].double(), fy64[small])
    # the cases the table is there for
    ex = e["expect"]
    valid = ex[..., 0] >= 0
    assert int(((ex[..., 0] == 0) & (ex[..., 1] == 0)).sum()) >= 3                                 # pixel (0,0) as a VALID pixel
    assert bool((valid & (torch.as_tensor(e["xyz"])[None, :, 2] < 0)).any())                       # valid behind the camera
    assert bool((ex[..., 0] == e["W"] - 1).any()) and bool((ex[..., 1] == e["H"] - 1).any())
    assert not bool(valid[:, torch.as_tensor(e["xyz"])[:, 0].abs() > 1e6].any())


@pytest.mark.parametrize("seed,n,V,H,W", ib.all_sample_cases())
def test_generated_samples_truncate_alike_in_fp32_and_fp64(seed, n, V, H, W):
    views = ib.make_views(seed, V, H, W)
    xyz = ib.random_samples(seed, n, views, H, W)
    assert np.array_equal(xyz, ib.random_samples(seed, n, views, H, W))                            # deterministic
    p32 = _oracle_pixels(xyz, views["c2w"], views["intrinsic"], H, W, torch.float32)
    p64 = _oracle_pixels(xyz, views["c2w"], views["intrinsic"], H, W, torch.float64)
    flips = int((p32 != p64).any(-1).sum())
    assert flips == 0, flips
    # ... and the restatement on the kernels' own operand (w2c: the float64 inverse rounded once) is the oracle's
    assert torch.equal(ib.restated_pixels(xyz, views["w2c"], views["intrinsic"], H, W), p64)
    assert torch.equal(ib.restated_pixels(xyz, views["w2c"], views["intrinsic"], H, W, torch.float32), p64)
    fx, fy = ib.project(xyz, views["w2c"], views["intrinsic"])
    assert float(torch.minimum((fx - fx.round()).abs(), (fy - fy.round()).abs()).min()) >= 1e-3
    if n >= 37:
        valid = p64[..., 0] >= 0
        assert bool(valid.any()) and bool((~valid.any(0)).any())                                   # samples inside a view, samples outside every view


_FUSED_SETS = [(0, None)] + ib.FUSED_CASES + [(n, ib.FUSED_CHILD_HW) for n in ib.FUSED_CHILD_N if (n, ib.FUSED_CHILD_HW) not in ib.FUSED_CASES]


@pytest.mark.parametrize("n,hw", _FUSED_SETS, ids=["edge" if hw is None else "n%d_%dx%d" % (n, hw[0], hw[1]) for n, hw in _FUSED_SETS])
def test_fused_merge_stage_inputs_are_what_the_gpu_module_assumes(n, hw):
    """The V = 4 sets of tests/test_fused_stages_gpu.py: logits of a useful spread, samples merged to exactly 0 for both reasons, and a reference that
    moves by far more than the tolerance when the hidden activations or the view order of campos_nearest are wrong."""
    c = ib.fused_merge_case(n, hw)
    n = c["n"]
    r64, r32 = ib.fused_merge_refs(c)
    assert r64["merged"].shape == (n, 45) and r64["logits"].shape == (4, n) and bool(torch.isfinite(r64["merged"]).all())
    sd = float(r64["logits"].std())
    assert 0.5 <= sd <= 3.0, sd
    e32, bound = ib.merge_bound(r64, r32)
    assert e32 < 1e-5 and bound == 4 * e32 + 3e-7
    valid = r64["valid"]
    fw, z, n_only = ib.frame_weights_with_a_zero(valid)
    assert float(fw[z]) == 0.0 and int((fw == 0).sum()) == 1 and float(fw.min()) == 0.0 and float(fw[fw > 0].min()) >= 0.5
    if hw is None:
        assert torch.equal(c["pix"], ib.edge_samples()["expect"][[0, 1, 1, 0]])
        assert bool((~valid.any(0)).any())                  # (views 0 and 3, 1 and 2 are the same camera: no sample has one unmasked view only)
    if n >= 37 and hw is not None:
        assert int((~valid.any(0)).sum()) >= 3                                                      # masked in all four views
        assert n_only >= 1                                                                          # unmasked only where frame_w = 0
        assert int((valid.sum(0) >= 2).sum()) >= n // 4                                             # the merge weights matter: several views to weigh
    if n >= 37 or hw is None:
        for w in (None, fw):
            b, d_hidden, d_swap = ib.merge_sensitivity(c, w)
            assert d_hidden > 100 * b, (d_hidden, b)
            # (the edge table's views 1 and 2 are the same camera: nothing to swap there)
            assert d_swap > 100 * b or hw is None, (d_swap, b)


def test_fused_stage_restatements_are_torchs_own_layers():
    g = torch.Generator().manual_seed(2)
    x = torch.randn((9, 48), generator=g, dtype=torch.float64)
    Ws = [torch.randn(d, generator=g) for d in ((64, 48), (64, 64), (5, 64))]
    bs = [None, torch.randn(64, generator=g), torch.randn(5, generator=g)]
    add = torch.randn((9, 64), generator=g)
    y = F.leaky_relu(F.linear(x, Ws[0].double()) + add.double(), 0.01)
    y = F.leaky_relu(F.linear(y, Ws[1].double(), bs[1].double()), 0.01)
    y = F.linear(y, Ws[2].double(), bs[2].double())
    outs = ib.mlp_ref(x, Ws, bs, (1, 1, 0), 0.01, torch.float64, addend=add)
    assert len(outs) == 3 and outs[2].dtype == torch.float64
    torch.testing.assert_close(outs[2], y, rtol=0, atol=1e-12)
    assert ib.mlp_ref(x, Ws, bs, (1, 1, 0), 0.01, torch.float32)[2].dtype == torch.float32
    # the mix-up case: pre-sigmoid values inside +-2 (so that the sigmoid does not flatten an error), colours from them
    for S in (1, 33, 385):
        c = ib.fused_mixup_case(S)
        r64, r32 = ib.fused_mixup_refs(c)
        assert float(r64["pre"].abs().max()) <= 2.0 and r64["Y"].shape == (S, 45) and r32["rgb"].dtype == torch.float32
        x = torch.cat([r64["Y"] + c["CF"][:, :45].double(), c["CF"][:, 45:].double()], dim=1)
        torch.testing.assert_close(r64["rgb"], torch.sigmoid(F.linear(x, c["w_fin"].double(), c["b_fin"].double())) * 1.002 - 0.001, rtol=0, atol=1e-14)
    # frame weights: the zero goes to the view that is the only unmasked one of the most samples
    v = torch.tensor([[1, 0, 0, 1], [0, 0, 1, 1], [0, 0, 1, 0], [0, 0, 0, 0]]).bool()
    fw, z, k = ib.frame_weights_with_a_zero(v)
    assert (z, k) == (0, 1) or (z, k) == (2, 1)
    # delta view directions in float32 are the float64 ones to rounding
    e = ib.edge_samples()
    d64, d32 = ib.delta_dirs(e["xyz"], ib.FUSED_CAMPOS, e["campos_n"]), ib.delta_dirs(e["xyz"], ib.FUSED_CAMPOS, e["campos_n"], torch.float32)
    assert d32.dtype == torch.float32 and float((d32.double() - d64).abs().max()) < 1e-6


def test_fixture_samples_truncate_alike_in_their_first_views():
    """The scannet_small fixture's own samples against its first 1, 3 and 4 views (the V <= 4 cases of the whole-path tests)."""
    from tests.golden_io import load_render, torch_inputs
    from oracle import render_oracle as ro
    d = load_render("scannet_small")
    tc = torch_inputs(d)
    loc = torch.from_numpy(d["q_sample_loc_w"])
    H, W = d["images_nearest"].shape[1:3]
    for V in (1, 3, 4):
        p32 = ro.gathered_pixels(loc, tc["c2w_nearest"][:, :V], tc["intrinsic_nearest"], H, W)
        p64 = ro.gathered_pixels(loc.double(), tc["c2w_nearest"][:, :V].double(), tc["intrinsic_nearest"].double(), H, W)
        assert int((p32 != p64).any(-1).sum()) == 0, V


def test_extra_views_of_the_whole_path_tests_truncate_alike():
    """The appended views (V > 4): the fixture's cameras moved by a few centimetres.  Float32 and float64 agree on every (view, sample) row of the
    render fixture's and of the training fixture's samples."""
    from tests.golden_io import load_render, load_train
    from oracle import render_oracle as ro
    d = load_render("scannet_small")
    H, W = d["images_nearest"].shape[1:3]
    c2w = torch.from_numpy(ib.extended_c2w(d["c2w_nearest"], 8))[None]
    K = torch.from_numpy(d["intrinsic"])[None]
    assert np.array_equal(c2w[0, :4].numpy(), d["c2w_nearest"]) and np.array_equal(load_train("scannet_small")["c2w_nearest"], d["c2w_nearest"])
    for loc in (torch.from_numpy(d["q_sample_loc_w"]), torch.from_numpy(load_train("scannet_small")["q_sample_loc_w"])):
        p32 = ro.gathered_pixels(loc, c2w, K, H, W)
        p64 = ro.gathered_pixels(loc.double(), c2w.double(), K.double(), H, W)
        assert int((p32 != p64).any(-1).sum()) == 0
        assert all(int((p64[v, ..., 0] >= 0).sum()) > 1000 for v in range(8))                      # every extra view sees the scene


@pytest.mark.parametrize("Hs,Ws", ib.pyramid_sizes(9, 7))
def test_upsample_transpose_restatement_is_torchs(Hs, Ws):
    x = torch.randn((1, 2, Hs, Ws), dtype=torch.float64, generator=torch.Generator().manual_seed(Hs), requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: ib.upsample(t, 9, 7), (x,), eps=1e-6, atol=1e-9)
    # the transpose against the explicit matrix of the (linear) forward
    n = 2 * Hs * Ws
    J = torch.stack([ib.upsample(e.view(1, 2, Hs, Ws), 9, 7).reshape(-1) for e in torch.eye(n, dtype=torch.float64)], dim=1)      # [out, in]
    g = torch.randn((1, 2, 9, 7), dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    torch.testing.assert_close(ib.upsample_transpose(g, Hs, Ws).reshape(-1), J.t() @ g.reshape(-1), rtol=0, atol=1e-14)
    assert float(J.min()) >= 0.0                                                                   # non-negative weights: sum |w g| bounds are sums of |terms|


def test_scatter_restatement_skips_masked_rows_and_pixel_00():
    pix = torch.tensor([[[0, 0], [-1, -1], [2, 1], [2, 1]]])
    rows = torch.arange(4 * 48, dtype=torch.float32).view(1, 4, 48) - 90.0
    g, ga, cnt, keep = ib.scatter_rows(rows, pix, 1, 3, 4)
    assert keep.tolist() == [[False, False, True, True]]
    assert float(g[0, 0, 0].abs().max()) == 0 and float(cnt.sum()) == 2 and float(cnt[0, 1, 2]) == 2
    assert torch.equal(g[0, 1, 2], (rows[0, 2] + rows[0, 3]).double()) and torch.equal(ga[0, 1, 2], (rows[0, 2].abs() + rows[0, 3].abs()).double())


def test_clipped_cnn_backward_rejects_bad_arguments_without_touching_the_gpu():
    from hybridneuralrendering_amd import _lib
    L = _lib.lib()
    assert "hnr_image_features_bwd_bbox" in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), "hnr_image_features_bwd_bbox")
    null, one, bad = None, ctypes.c_void_p(16), -1
    arr = (ctypes.c_void_p * 6)(*[16] * 6)
    # hnr_image_features_bwd_bbox(img, V, H, W, conv_w, slope, scratch, g_pyramid, g_conv_w, g_conv_b, bbox, stream)
    assert L.hnr_image_features_bwd_bbox(one, 2, 48, 64, arr, 0.01, one, one, arr, arr, null, null) == bad                # NULL rectangle
    assert b"hnr_image_features_bwd_bbox" in L.hnr_last_error()
    assert L.hnr_image_features_bwd_bbox(null, 2, 48, 64, arr, 0.01, one, one, arr, arr, one, null) == bad                # NULL image
    assert L.hnr_image_features_bwd_bbox(one, 0, 48, 64, arr, 0.01, one, one, arr, arr, one, null) == bad                 # no views
    assert L.hnr_image_features_bwd_bbox(one, 2, 1, 64, arr, 0.01, one, one, arr, arr, one, null) == bad                  # H = 1
    assert L.hnr_image_features_bwd_bbox(one, 2, 48, 64, arr, 0.01, one, null, arr, arr, one, null) == bad                # NULL gradient pyramid
    assert b"hnr_image_features_bwd" in L.hnr_last_error()
