"""Content-aware frame weights on the device (csrc/raft.hip, csrc/blur_score.hip) against the restatements of tests/raft_ref.py and
tests/frame_weights_ref.py.

THE RULE for every fp32 stage, as in tests/test_mvs_depth_gpu.py: the stage is fed the fp64 restatement's inputs rounded to fp32; its output must lie
within 4 x the maximum error of the fp32 restatement against the fp64 restatement for that output on the same inputs (not below one ulp of the output's
largest magnitude), computed here on the CPU.  The bound comes from the restatement, never from the device code.  The whole flow at iters 1, 3 and
20 is held to the same rule.  The fp64 parts have derived bounds: edges 1e-11 (at most 30 fp64 terms of magnitude <= 1020), variances 1e-9 relative;
picks, used-pixel sets and counts are equal.

Shapes (H, W): (128, 160), (136, 200), (136, 152): feature maps 16x20, 17x25, 17x19 -- more than one 32-pixel tile with a ragged last one, pyramids
with odd extents under floor pooling and a coarsest level of extent 2, 126- and 2-channel layers (ragged 32-channel tiles).
Measured ratios: profiles/frame_weights_tests.txt."""
import functools

import numpy as np
import pytest
import torch

from tests import frame_weights_ref as FR
from tests import raft_ref as R
from tests.bits import DEV, t
from tests.test_frame_weights import fixture, params

pytestmark = pytest.mark.gpu

MARGIN = 4.0
SHAPES = [0, 1, 2]
LAST = 21                                                         # the restatement runs 21 iterations: the state after iteration 19 (0-based) is the input of the 21st


def rule(got, truth, yard, what):
    g, tr, y = (np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, np.float64) for a in (got, truth, yard))
    assert g.shape == tr.shape == y.shape, (what, g.shape, tr.shape, y.shape)
    floor = float(np.spacing(np.float32(np.abs(tr).max())))
    e_hip, e_t = float(np.abs(g - tr).max()), float(np.abs(y - tr).max())
    print("RATIO %s: hip %.3e, restatement fp32 %.3e, ulp of max %.3e -> ratio %.2f" % (what, e_hip, e_t, floor, e_hip / max(e_t, floor)))
    assert np.isfinite(g).all() and e_hip <= MARGIN * max(e_t, floor), (what, e_hip, e_t, floor)


def images(si):
    d = fixture()
    return d["s%d.image1" % si], d["s%d.image2" % si]


@functools.lru_cache(maxsize=None)
def run(si, dtype, a="image1", b="image2"):
    """The restatement's whole run (21 iterations) on a pair of the fixture's images of shape si; computed once and shared."""
    d = fixture()
    return R.forward(params(), d["s%d.%s" % (si, a)], d["s%d.%s" % (si, b)], LAST, dtype, keep=(0, 1, 2, 19, 20))


def flows_at(r, iters):
    """(flow_low, flow_up) after `iters` iterations of a run."""
    s = r["steps"][iters - 1]
    h, w = s["coords"].shape[-2:]
    low = s["coords"] - R.grid(h, w, s["coords"].dtype)
    return low, R.upsample(low[None], s["mask"][None])[0]


def both(fn, *inputs32):
    """(fp64 result, fp32 result) of a restatement stage on the same fp32 inputs."""
    with torch.no_grad():
        return fn(torch.float64, *[x.double() for x in inputs32]), fn(torch.float32, *inputs32)


def sd_of(dtype):
    return R.cast(params(), dtype)


@pytest.fixture(scope="module")
def net():
    from hybridneuralrendering_amd.flow import RAFT
    published = {"module." + k: v for k, v in params().items()}                 # the form of the published checkpoint's key list
    published["module.cnet.norm1.num_batches_tracked"] = torch.tensor(1)
    return RAFT().load_pretrained(published).to(DEV)


def pair_tensor(im1, im2):
    return t(np.stack([im1, im2]), torch.float32)


@pytest.mark.parametrize("si", SHAPES)
def test_encoder_instance_norm_on_both_images(net, si):
    from hybridneuralrendering_amd import flow
    im1, im2 = images(si)
    x = torch.from_numpy(np.stack([im1, im2]))
    truth, yard = both(lambda dt, *_: R.encoder(sd_of(dt), "fnet", R.scale_image(x, dt), False))
    got = flow.encoder(pair_tensor(im1, im2), net.packed()[0], 0)
    rule(got, truth, yard, "s%d fnet" % si)


@pytest.mark.parametrize("si", SHAPES)
def test_encoder_batch_norm(net, si):
    from hybridneuralrendering_amd import flow
    im1, _ = images(si)
    x = torch.from_numpy(im1)[None]
    truth, yard = both(lambda dt, *_: R.encoder(sd_of(dt), "cnet", R.scale_image(x, dt), True))
    img = t(im1[None], torch.float32)
    rule(flow.encoder(img, net.packed()[1], 1), truth, yard, "s%d cnet" % si)
    act = lambda c: torch.cat([torch.tanh(c[:, :128]), torch.relu(c[:, 128:])], dim=1)
    rule(flow.encoder(img, net.packed()[1], 2), act(truth), act(yard), "s%d cnet tanh|relu" % si)


@pytest.mark.parametrize("si", SHAPES)
def test_correlation_pyramid(si):
    from hybridneuralrendering_amd import flow
    f = run(si, torch.float64)["fmaps"].float()
    truth, yard = both(lambda dt, a, b: R.corr_pyramid(a, b), f[0], f[1])
    h, w = f.shape[-2:]
    got = flow.pyramid_levels(flow.corr_pyramid(t(f[0]), t(f[1])), h, w)
    assert [tuple(g.shape) for g in got] == [tuple(x.shape) for x in truth]
    for l in range(4):
        rule(got[l], truth[l], yard[l], "s%d pyramid level %d %s" % (si, l, tuple(truth[l].shape[1:])))


def lookup_coords(h, w):
    """The grid plus offsets: exactly on integers, fractional, just outside the map on every side, far outside."""
    c = R.grid(h, w, torch.float32)
    rs = np.random.RandomState(5)
    c = c + torch.from_numpy(rs.uniform(-6, 6, (2, h, w)).astype(np.float32))
    c[:, 0, :] = R.grid(h, w, torch.float32)[:, 0, :]                          # integers
    c[:, 1, :] = torch.round(c[:, 1, :])
    c[0, 2, :], c[1, 2, :] = -4.0 - 1e-3, float(h + 3) + 1e-3                  # window edge just outside the map: x + 4 < 0, y - 4 > h - 1
    c[0, 3, :], c[1, 3, :] = float(w + 3) + 1e-3, -4.0 - 1e-3
    c[0, 4, :], c[1, 4, :] = -5.0, float(h + 4)                                # the last tap exactly one pixel outside
    c[:, 5, :] = 1000.0
    c[:, 6, :] = -1000.0
    c[0, 7, :], c[1, 7, :] = float(w - 1), float(h - 1)                        # the map's last pixel
    return c


@pytest.mark.parametrize("si", SHAPES)
def test_lookup(si):
    from hybridneuralrendering_amd import flow
    levels = [l.float() for l in run(si, torch.float64)["levels"]]
    hw = levels[0].shape[0]
    h, w = levels[0].shape[-2:]
    coords = lookup_coords(h, w)
    truth, yard = both(lambda dt, c, *lv: R.lookup(list(lv), c), coords, *levels)
    assert float((truth == 0).double().mean()) > 0.2 and float((truth != 0).double().mean()) > 0.2
    buf = t(torch.cat([l.reshape(-1) for l in levels]))
    rule(flow.lookup(buf, t(coords)), truth, yard, "s%d lookup" % si)
    assert hw == h * w


@pytest.mark.parametrize("it", [0, 1, 19, 20])
@pytest.mark.parametrize("si", SHAPES)
def test_one_update_iteration(net, si, it):
    """From the state before iteration `it` (0-based) of the fp64 run: 0 is the initial state (flow 0), 1 the state after iteration 0, 20 the state after
    iteration 19."""
    from hybridneuralrendering_amd import flow
    r = run(si, torch.float64)
    s = r["steps"][it]
    levels = [l.float() for l in r["levels"]]
    net_in, inp, coords = s["net_in"].float(), r["inp"].float(), s["coords_in"].float()
    h, w = coords.shape[-2:]

    def stage(dt, n, i, c, *lv):
        corr = R.lookup(list(lv), c)
        n2, mask, delta = R.update(sd_of(dt), n[None], i[None], corr[None], (c - R.grid(h, w, dt))[None])
        return n2[0], c + delta[0], delta[0], mask[0]

    truth, yard = both(stage, net_in, inp, coords, *levels)
    buf = t(torch.cat([l.reshape(-1) for l in levels]))
    got = flow.update(net.packed()[2], buf, t(net_in), t(inp), t(coords), want_mask=True)
    for name, g, tr, y in zip(("net", "coords", "delta_flow", "mask"), got, truth, yard):
        rule(g, tr, y, "s%d update %d %s" % (si, it, name))
    # without the mask head nothing else changes
    got2 = flow.update(net.packed()[2], buf, t(net_in), t(inp), t(coords), want_mask=False)
    assert got2[3] is None and all(torch.equal(a, b) for a, b in zip(got[:3], got2[:3]))


@pytest.mark.parametrize("si", SHAPES)
def test_convex_upsampling(si):
    from hybridneuralrendering_amd import flow
    r = run(si, torch.float64)
    s = r["steps"][19]
    h, w = s["coords"].shape[-2:]
    low, mask = (s["coords"] - R.grid(h, w, torch.float64)).float(), s["mask"].float()
    truth, yard = both(lambda dt, f, m: R.upsample(f[None], m[None])[0], low, mask)
    rule(flow.upsample(t(low), t(mask)), truth, yard, "s%d upsample" % si)


@pytest.mark.parametrize("si", SHAPES)
def test_whole_flow(net, si):
    im1, im2 = images(si)
    r64, r32 = run(si, torch.float64), run(si, torch.float32)
    a, b = t(im1[None], torch.float32), t(im2[None], torch.float32)
    for iters in (1, 3, 20):
        low, up = net(a, b, iters=iters, test_mode=True)
        assert tuple(low.shape) == (1, 2, im1.shape[1] // 8, im1.shape[2] // 8) and tuple(up.shape) == (1, 2) + im1.shape[1:]
        (tl, tu), (yl, yu) = flows_at(r64, iters), flows_at(r32, iters)
        rule(low[0], tl, yl, "s%d flow_low iters %d" % (si, iters))
        rule(up[0], tu, yu, "s%d flow_up iters %d" % (si, iters))
    assert float(up.abs().max()) >= 2.0


def test_two_runs_are_bit_identical(net):
    im1, im2 = images(1)
    a, b = t(im1[None], torch.float32), t(im2[None], torch.float32)
    l1, u1 = net(a, b, iters=20)
    junk = torch.full((1 << 22,), float("nan"), device=DEV)                      # the next scratch does not start from the same bytes
    l2, u2 = net(a, b, iters=20)
    assert torch.equal(l1, l2) and torch.equal(u1, u2) and junk.numel()


def gray_planes(H, W, seed):
    rs = np.random.RandomState(seed)
    g = rs.randint(0, 256, (4, H, W)).astype(np.uint8)
    g[1] = (rs.randint(0, 2, (H, W)) * 255).astype(np.uint8)                     # extremes: |Laplacian| up to 4 * 255
    g[2] = 77                                                                  # flat: exactly 0 up to the rounding of 1/25
    return g


@pytest.mark.parametrize("si", SHAPES)
def test_edges(si):
    from hybridneuralrendering_amd import frame_weights as FW
    H, W = (int(v) for v in fixture()["shapes"][si])
    g = gray_planes(H, W, 11 + si)
    got = FW.blur_edges(t(g)).cpu().numpy()
    want = np.stack([FR.edges(p) for p in g])
    err = float(np.abs(got - want).max())
    print("RATIO s%d edges: max error %.3e of 1e-11" % (si, err))
    assert got.dtype == np.float64 and err <= 1e-11 and np.abs(want[1]).max() > 100


@pytest.mark.parametrize("si", SHAPES)
def test_scores_with_the_recorded_flow(si):
    from hybridneuralrendering_amd import frame_weights as FW
    d = fixture()
    H, W = (int(v) for v in d["shapes"][si])
    flow_up = d["s%d.it20.flow_up" % si]
    g = gray_planes(H, W, 21 + si)
    e1, e2 = FR.edges(g[0]), FR.edges(g[3])
    for border in (20, 0):
        v1, v2, n, picks, used = FR.score_pair(e1, e2, flow_up, border)
        row, pick, usedd = FW.blur_score_pair(t(e1), t(e2), t(flow_up), border, want_maps=True)
        row = row.cpu().numpy()
        np.testing.assert_array_equal(pick.cpu().numpy().astype(np.int64), picks)
        np.testing.assert_array_equal(usedd.cpu().numpy(), used)
        assert row[2] == n and 0 < n < H * W
        print("RATIO s%d border %d scores: relative errors %.3e %.3e of 1e-9, %d pixels" % (si, border, abs(row[0] - v1) / v1, abs(row[1] - v2) / v2, n))
        assert abs(row[0] - v1) <= 1e-9 * v1 and abs(row[1] - v2) <= 1e-9 * v2
        assert torch.equal(FW.blur_score_pair(t(e1), t(e2), t(flow_up), border), t(row))


def test_end_to_end_bank_of_four_frames(net):
    """Frames A, B, A, B of the first shape: pairs (A,B), (B,A), (A,B) and the last frame with itself.  The table equals the restatement's scoring applied
    to the DEVICE's own flows (so a nearest-pixel flip at a rounding boundary can neither hide a failure nor cause one), and those flows pass the flow
    rule."""
    from hybridneuralrendering_amd import frame_weights as FW
    from hybridneuralrendering_amd.frames import FrameBank  # noqa: F401  (the consumer of the result)
    A, B = images(0)
    names = ("image1", "image2", "image1", "image2")
    frames = np.stack([A, B, A, B]).transpose(0, 2, 3, 1).copy()
    imgs = t(frames)
    gray = FW.gray_from_rgb(imgs)
    assert gray.dtype == torch.uint8 and tuple(gray.shape) == (4, 128, 160)
    table, flows = FW.score_table(imgs, gray, net, border=20, iters=20, want_flows=True)
    table = table.cpu().numpy()
    g = gray.cpu().numpy()
    edges = [FR.edges(p) for p in g]
    for f in range(4):
        nb = min(f + 1, 3)
        tl, tu = flows_at(run(0, torch.float64, names[f], names[nb]), 20)
        yl, yu = flows_at(run(0, torch.float32, names[f], names[nb]), 20)
        rule(flows[f], tu, yu, "bank pair %d flow_up" % f)
        v1, v2, n, _, _ = FR.score_pair(edges[f], edges[nb], flows[f].cpu().numpy(), 20)
        assert table[f, 2] == n and n > 0
        assert abs(table[f, 0] - v1) <= 1e-9 * v1 and abs(table[f, 1] - v2) <= 1e-9 * v2
    assert np.array_equal(table[0], table[2])
    w = FW.content_aware_weights(imgs, gray, net, window_size=3, sliding_step=2, border=20, iters=20)
    assert w.dtype == np.float64 and w.shape == (4,)
    np.testing.assert_array_equal(w, FW.weights_from_scores(table[:, 0], table[:, 1], 3, 2))


def test_a_frame_without_used_pixels_raises(net, monkeypatch):
    from hybridneuralrendering_amd import frame_weights as FW
    from hybridneuralrendering_amd._lib import HnrError
    tab = torch.tensor([[1.0, 2.0, 50.0], [0.0, 0.0, 0.0], [1.0, 1.0, 9.0]], dtype=torch.float64, device=DEV)
    monkeypatch.setattr(FW, "score_table", lambda *a, **k: tab)
    with pytest.raises(HnrError, match=r"\[1\]"):
        FW.content_aware_weights(None, None, net)
    # ... and from the kernel: a flow that throws every pixel out of the frame gives the row (0, 0, 0)
    e = t(np.random.RandomState(0).standard_normal((128, 160)))
    row = FW.blur_score_pair(e, e, torch.full((2, 128, 160), 500.0, device=DEV), 20)
    assert row.cpu().tolist() == [0.0, 0.0, 0.0]
