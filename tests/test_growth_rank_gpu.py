"""The growth schedule on the device: hnr_ray_miss_rank (csrc/rank.hip) against the NumPy restatement (tests/growth_ref.py) and the reference's own
results (tests/golden/growth_rank.npz), growth.RayMissRanking's edges and capture, and growth.grow_pass end to end on a small scene."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import growth_ref as G
from tests.golden_io import GOLD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _launch(color, gt, mask, frame, ids, losses, n=None, R=None, last=True, null=()):
    """One raw call; the tensors are written in place.  Returns (rc, last [2] or None)."""
    from hybridneuralrendering_amd import _lib
    L = _lib.lib()
    out = torch.full((2,), -7.0, dtype=torch.float32, device=DEV) if last else None
    p = lambda name, t: None if (name in null or t is None) else _lib.ptr(t)
    rc = L.hnr_ray_miss_rank(p("color", color), p("gt", gt), p("mask", mask), int(mask.numel() if R is None else R), p("frame", frame), p("ids", ids),
                             p("losses", losses), int(losses.numel() if n is None else n), p("last", out), _lib.stream())
    torch.cuda.synchronize()
    return rc, out


def _batch(rng, R, p_miss=0.3):
    gt = rng.random((R, 3)).astype(np.float32)
    color = rng.random((R, 3)).astype(np.float32)
    mask = (rng.random(R) >= p_miss).astype(np.int8)
    color[mask == 0] = 1.0
    return color, gt, mask


def _ulp_close(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return bool(np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)))


# ------------------------------------------------------------------------------------------------ a. the kernel against the restatement
@pytest.mark.parametrize("R,n", [(1, 2), (49, 2), (63, 11), (64, 11), (65, 11), (3136, 11), (1000, 65), (4097, 1024)])
def test_kernel_equals_the_restatement(R, n):
    rng = np.random.default_rng(1000 * n + R)
    ids = rng.permutation(4 * n + 7)[:n].astype(np.int32)
    losses = np.sort(rng.random(n).astype(np.float32) * np.float32(R))[::-1].copy()
    losses[n - n // 3:] = 0.0                                                  # a tail of empty slots
    if n >= 8:
        losses[2] = losses[1]                                                   # a tie among the positive entries
    absent = int(4 * n + 100)
    cases = [(int(ids[0]), 0.3), (int(ids[n // 2]), 0.9), (absent, 0.3), (absent + 1, 0.0), (int(ids[-1]), 1.0)]
    for k, (frame, p_miss) in enumerate(cases):
        color, gt, mask = _batch(rng, R, p_miss)
        if k == 1 and R < 4:
            mask[:] = 0                                                         # (tiny batches: make sure a miss occurs at all)
        want_L, want_miss = G.ray_miss_loss(color, gt, mask)
        want_ids, want_losses = G.rank_update(ids, losses, frame, want_L)
        d_ids, d_losses = _t(ids), _t(losses)
        rc, last = _launch(_t(color), _t(gt), _t(mask), _t(np.array([frame], np.int32)), d_ids, d_losses)
        assert rc == 0
        got_last = last.cpu().numpy()
        print("R %d n %d case %d: L %.9g (want %.9g), missed %d" % (R, n, k, got_last[0], want_L, want_miss))
        assert got_last[0] == want_L and got_last[1] == np.float32(want_miss), (got_last, want_L, want_miss)
        np.testing.assert_array_equal(d_ids.cpu().numpy(), want_ids)
        assert _ulp_close(d_losses.cpu().numpy(), want_losses)
        ids, losses = want_ids, want_losses                                     # the next case starts from this state


# ------------------------------------------------------------------------------------------------ b. the reference's sequence
def test_golden_sequence_on_the_device():
    from hybridneuralrendering_amd import growth
    from tests.test_growth_rank import replay
    z = np.load(os.path.join(GOLD, "growth_rank.npz"))
    train_len, num_step = int(z["train_len"][0]), int(z["prob_num_step"][0])
    rank = growth.RayMissRanking(train_len, num_step, DEV, prob_tiers=z["prob_tiers"].tolist(), prob_kernel_size=z["prob_kernel_size"].tolist())
    one = growth.RayMissRanking(train_len, 1, DEV, prob_tiers=z["prob_tiers"].tolist(), prob_kernel_size=z["prob_kernel_size"].tolist())
    assert rank.n == z["ids"].shape[1] and one.n == 1
    color, gt, mask, frame = _t(z["color"]), _t(z["gt"]), _t(z["ray_mask"]), _t(z["frame"])
    ref_state = [G.new_table(train_len, num_step)]

    def update(k):
        out = dict(coarse_raycolor=color[k], ray_mask=mask[k])
        rank.update(out, gt[k], frame[k:k + 1], total_steps=int(z["total_steps"][k]))
        one.update(out, gt[k], int(z["frame"][k]), total_steps=int(z["total_steps"][k]))
        L, _ = G.ray_miss_loss(z["color"][k], z["gt"][k], z["ray_mask"][k])
        gated = G.probe_tier(int(z["total_steps"][k]), z["prob_tiers"], z["prob_kernel_size"]) is None
        if not gated:
            ref_state[0] = G.rank_update(*ref_state[0], int(z["frame"][k]), L)
            assert float(rank.last[0]) == float(L)
        # every entry, the zero-loss ones included, equals the restatement (the stable order)
        np.testing.assert_array_equal(rank.ids.cpu().numpy(), ref_state[0][0])
        assert _ulp_close(rank.losses.cpu().numpy(), ref_state[0][1])
        np.testing.assert_allclose(float(one.losses[0]), z["n1_losses"][k], rtol=G.loss_tolerance(49), atol=0)
        return rank.ids.cpu().numpy(), rank.losses.cpu().numpy(), L

    replay(z, update)
    assert rank.top_frames(train_len // num_step) == z["probe_30000_frames"].tolist()
    assert one.top_frames(5) == []
    rank.reset()
    np.testing.assert_array_equal(rank.ids.cpu().numpy(), z["reset_ids"])
    np.testing.assert_array_equal(rank.losses.cpu().numpy(), z["reset_losses"])


# ------------------------------------------------------------------------------------------------ c. edges
def test_ranking_edges():
    from hybridneuralrendering_amd import growth
    rng = np.random.default_rng(3)
    R = 70
    rank = growth.RayMissRanking(8, 4, DEV)                                     # three slots: frames 0, 1, 2 present with loss 0
    assert rank.n == 3 and rank.ids.tolist() == [0, 1, 2] and rank.losses.tolist() == [0, 0, 0]
    color, gt, mask = _batch(rng, R, 0.4)
    hit = np.ones(R, np.int8)
    L, n_miss = G.ray_miss_loss(color, gt, mask)
    out = dict(coarse_raycolor=_t(color), ray_mask=_t(mask))
    out_hit = dict(coarse_raycolor=_t(color), ray_mask=_t(hit))
    # no ray missed, an absent frame: loss 0 lands in the last slot
    last = rank.update(out_hit, _t(gt), 7)
    assert last.tolist() == [0.0, 0.0] and rank.ids.tolist() == [0, 1, 7] and rank.losses.tolist() == [0, 0, 0]
    # all rays missed
    allm = dict(coarse_raycolor=_t(np.ones((R, 3), np.float32)), ray_mask=_t(np.zeros(R, np.int8)))
    L_all, _ = G.ray_miss_loss(np.ones((R, 3), np.float32), gt, np.zeros(R, np.int8))
    last = rank.update(allm, _t(gt), 1)
    assert float(last[0]) == float(L_all) and float(last[1]) == R and rank.ids.tolist() == [1, 0, 7] and float(rank.worst()) == float(L_all)
    # the same positive loss for another frame: equal losses keep their slot order
    rank.update(allm, _t(gt), 7)
    assert rank.ids.tolist() == [1, 7, 0] and rank.losses.tolist() == [float(L_all), float(L_all), 0.0]
    # a present frame with a smaller loss keeps the larger one
    assert 0 < float(L) < float(L_all)
    rank.update(out, _t(gt), 1)
    assert rank.ids.tolist() == [1, 7, 0] and rank.losses.tolist() == [float(L_all), float(L_all), 0.0] and float(rank.last[0]) == float(L)
    # the frame number changes on the device between two launches: no host value involved
    row = _t(np.array([4], np.int32))
    step = _t(np.array([2], np.int32))
    rank.update(out, _t(gt), row)
    assert rank.ids.tolist() == [1, 7, 4]
    row.add_(step)
    rank.update(allm, _t(gt), row)
    assert rank.ids.tolist() == [1, 7, 6] and rank.top_frames(5) == [1, 7] and rank.top_frames(1) == [1]
    # a NaN in a missed ray's colour: reported, the table untouched
    bad = color.copy()
    bad[int(np.nonzero(mask == 0)[0][0]), 1] = np.nan
    keep = (rank.ids.clone(), rank.losses.clone())
    last = rank.update(dict(coarse_raycolor=_t(bad), ray_mask=_t(mask)), _t(gt), 1)
    assert np.isnan(float(last[0])) and float(last[1]) == n_miss
    assert torch.equal(rank.ids, keep[0]) and torch.equal(rank.losses, keep[1])
    # ... while a NaN in a ray that hit does not matter
    bad = color.copy()
    bad[int(np.nonzero(mask == 1)[0][0]), 0] = np.nan
    assert float(rank.update(dict(coarse_raycolor=_t(bad), ray_mask=_t(mask)), _t(gt), 1)[0]) == float(L)
    # state_dict round trip and the blur module's colour taking precedence
    sd = rank.state_dict()
    other = growth.RayMissRanking(8, 4, DEV).load_state_dict(sd)
    assert torch.equal(other.ids, rank.ids) and torch.equal(other.losses, rank.losses)
    both = dict(coarse_raycolor=_t(np.zeros((R, 3), np.float32)), blurred_raycolor=_t(color), ray_mask=_t(mask))
    assert float(other.update(both, _t(gt), 1)[0]) == float(L)
    # prob_num_step == 1: the running maximum, no ids
    one = growth.RayMissRanking(8, 1, DEV)
    assert one.n == 1
    one.update(allm, _t(gt), 3)
    one.update(out, _t(gt), 5)
    assert one.losses.tolist() == [float(L_all)] and one.ids.tolist() == [0] and one.top_frames(4) == []
    # behind the last tier nothing is launched
    gated = growth.RayMissRanking(8, 4, DEV, prob_tiers=[100, 200], prob_kernel_size=[3, 3, 3, 1, 1, 1])
    gated.update(allm, _t(gt), 5, total_steps=201)
    assert gated.losses.tolist() == [0, 0, 0]
    gated.update(allm, _t(gt), 5, total_steps=200)
    assert gated.ids.tolist() == [5, 0, 1]
    with pytest.raises(growth.HnrError):
        rank.update(dict(coarse_raycolor=_t(color[:5]), ray_mask=_t(mask)), _t(gt), 1)


def test_bad_arguments_leave_the_table_unchanged():
    rng = np.random.default_rng(4)
    R, n = 40, 5
    color, gt, mask = (_t(a) for a in _batch(rng, R, 0.5))
    frame = _t(np.array([9], np.int32))
    ids0, losses0 = np.arange(n, dtype=np.int32) + 20, np.linspace(1, 0, n).astype(np.float32)
    for kw in (dict(n=0), dict(n=-3), dict(n=1025), dict(R=-1), dict(R=(1 << 24) + 1), dict(null=("color",)), dict(null=("gt",)), dict(null=("mask",)),
               dict(null=("frame",)), dict(null=("ids",)), dict(null=("losses",))):
        ids, losses = _t(ids0), _t(losses0)
        rc, last = _launch(color, gt, mask, frame, ids, losses, **kw)
        assert rc == -1, kw
        assert ids.cpu().numpy().tolist() == ids0.tolist() and losses.cpu().numpy().tolist() == losses0.tolist() and last.tolist() == [-7.0, -7.0], kw
    # allowed: no d_miss_out; no d_ids with n == 1; an empty batch is a step with loss 0
    ids, losses = _t(ids0), _t(losses0)
    rc, _ = _launch(color, gt, mask, frame, ids, losses, last=False)
    got = ids.cpu().numpy().tolist()
    assert rc == 0 and 9 in got and int(ids0[-1]) not in got                    # the absent frame took the last slot, then the sort placed it
    l1 = _t(np.array([0.25], np.float32))
    rc, last = _launch(color, gt, mask, frame, None, l1, n=1)
    assert rc == 0 and float(l1[0]) == max(0.25, float(last[0]))
    ids, losses = _t(ids0), _t(losses0)
    rc, last = _launch(color, gt, mask, frame, ids, losses, R=0)
    assert rc == 0 and last.tolist() == [0.0, 0.0] and ids.cpu().numpy().tolist() == ids0[:-1].tolist() + [9] and float(losses[-1]) == 0.0


# ------------------------------------------------------------------------------------------------ d. capture
def test_update_is_capturable_and_reads_nothing_back():
    """update() captured in a torch.cuda.graph on one stream and replayed three times over changed static inputs equals three eager updates.  A host
    read inside update() would make the capture raise."""
    from hybridneuralrendering_amd import growth
    rng = np.random.default_rng(5)
    R = 200
    dev = torch.device(DEV)
    batches = [_batch(rng, R, p) for p in (0.2, 0.6, 0.35, 0.5)]
    frames = [3, 17, 9, 17]
    cap, eager = growth.RayMissRanking(40, 4, DEV), growth.RayMissRanking(40, 4, DEV)
    s_col, s_gt, s_mask, s_row = _t(batches[0][0]), _t(batches[0][1]), _t(batches[0][2]), _t(np.array([frames[0]], np.int32))
    out = dict(coarse_raycolor=s_col, ray_mask=s_mask)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        cap.update(out, s_gt, s_row)                                            # warm-up outside the capture, undone below
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    cap.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        last = cap.update(out, s_gt, s_row)
    assert last is cap.last
    for k in (1, 2, 3):
        color, gt, mask = batches[k]
        s_col.copy_(_t(color)); s_gt.copy_(_t(gt)); s_mask.copy_(_t(mask)); s_row.fill_(frames[k])
        graph.replay()
        torch.cuda.synchronize(dev)
        want = eager.update(dict(coarse_raycolor=_t(color), ray_mask=_t(mask)), _t(gt), frames[k])
        assert torch.equal(cap.last, want), k
        assert torch.equal(cap.ids, eager.ids) and torch.equal(cap.losses, eager.losses), k
    assert cap.ids[:2].tolist() == [17, 9] and float(cap.losses[1]) > 0


# ------------------------------------------------------------------------------------------------ e. grow_pass end to end
TIERS, KERNEL = [40000, 120000], [3, 3, 3, 1, 1, 1]


def _world(seed=9):
    """scene0241 at 30000 points with the points in front of the middle of camera 0's image removed, five synthetic frames (the scene's camera and its four
    reference cameras) in a bank, the ray-marching module over the cloud, a dilated-patch sampler of 256 rays."""
    from hybridneuralrendering_amd import scenes
    from hybridneuralrendering_amd.aggregator import PointAggregator
    from hybridneuralrendering_amd.frames import BatchSampler, FrameBank
    from hybridneuralrendering_amd.modules import NeuralPoints, NeuralPointsRayMarching, find_blend_function, find_render_function, find_tone_map
    from hybridneuralrendering_amd.train import TrainPath
    dev = torch.device(DEV)
    sc = scenes.make_scene("scene0241", 30000, seed, w=64, h=48)
    opt = sc.opt
    opt.load_points, opt.is_train, opt.dilation_setup = 0, 1, "4_4_1_3"
    opt.prob_mode, opt.prob_num_step, opt.prob_tiers, opt.prob_kernel_size, opt.prob_thresh, opt.prob_mul, opt.far_thresh, opt.bgmodel = 0, 2, TIERS, KERNEL, 0.7, 0.4, 0.0, "no"
    w2c = np.linalg.inv(sc.c2w.astype(np.float64))
    cam = sc.xyz.astype(np.float64) @ w2c[:3, :3].T + w2c[:3, 3]
    px = cam[:, 0] / cam[:, 2] * sc.intrinsic[0, 0] + sc.intrinsic[0, 2]
    py = cam[:, 1] / cam[:, 2] * sc.intrinsic[1, 1] + sc.intrinsic[1, 2]
    slab = (cam[:, 2] > 0) & (px > 20) & (px < 44) & (py > 14) & (py < 34)
    keep = ~slab
    assert 500 < int(slab.sum()) < 15000
    npts = NeuralPoints(32, int(keep.sum()), opt, dev)
    npts.set_points(_t(sc.xyz[keep]), _t(sc.emb[:, keep]), points_color=_t(sc.color[:, keep]), points_dir=_t(sc.dir[:, keep]), points_conf=_t(sc.conf[:, keep]))
    torch.manual_seed(0)
    agg = PointAggregator(opt)
    with torch.no_grad():                                                       # opaque surfaces: the probe asks for a sample with opacity > prob_thresh
        agg.alpha_branch[0].weight.mul_(30.0)                                   # (an untrained network's samples reach 0.35 at most with smoke()'s bias of 30)
        agg.alpha_branch[0].bias.fill_(300.0)
    agg = agg.to(dev)
    net = NeuralPointsRayMarching(tonemap_func=find_tone_map("off"), render_func=find_render_function("radiance"), blend_func=find_blend_function("alpha"),
                                  aggregator=agg, neural_points=npts, opt=opt, num_pos_freqs=opt.num_pos_freqs, num_viewdir_freqs=opt.num_viewdir_freqs)
    images = scenes.reference_images(5, sc.h, sc.w, seed + 1) * 0.8                                 # nowhere the white background
    c2w = np.concatenate([sc.c2w[None], sc.c2w_nearest])
    bank = FrameBank(images.astype(np.float32), c2w, sc.intrinsic, dev)
    bank.set_nearest(np.array([[1, 2, 3, 4], [0, 2, 3, 4], [0, 1, 3, 4], [0, 1, 2, 4], [0, 1, 2, 3]]))
    sampler = BatchSampler(bank, "dilated", dilation_setup=opt.dilation_setup, seed=3, near=sc.near, far=sc.far, bg_color=(1.0, 1.0, 1.0)).set_schedule([0, 3, 1, 4, 2])
    return SimpleNamespace(sc=sc, opt=opt, npts=npts, agg=agg, net=net, bank=bank, sampler=sampler, path=TrainPath(net.renderer()), dev=dev)


def _train_and_rank(wd, steps=5):
    from hybridneuralrendering_amd import growth
    from hybridneuralrendering_amd.train import train_step
    rank = growth.RayMissRanking(wd.bank.F, wd.opt.prob_num_step, wd.dev, prob_tiers=TIERS, prob_kernel_size=KERNEL)
    p = wd.npts
    for k in range(steps):
        b = wd.sampler.next()
        out, _pg, _ag = train_step(wd.path, wd.agg, p.xyz, p.points_embeding, p.points_conf, p.points_dir, p.points_color, b["raydir"], b["campos"], b["camrotc2w"],
                                   b["bg_color"], b["near"], b["far"], b["c2w_nearest"], b["campos_nearest"], b["intrinsic_nearest"], b["images_nearest"],
                                   b["gt_image"], w2c_nearest=b["w2c_nearest"], device_frame_weight=b["frame_weight"], assign_grads=False)
        rank.update(out, b["gt_image"], b["frame_row"], total_steps=50000 + k)
        want, n_miss = G.ray_miss_loss(out["coarse_raycolor"].cpu().numpy(), b["gt_image"].cpu().numpy(), out["ray_mask"].cpu().numpy())
        assert float(rank.last[0]) == float(want) and float(rank.last[1]) == n_miss
        # the missed rays' rows of the step's colour hold the background colour
        miss = out["ray_mask"] == 0
        assert bool((out["coarse_raycolor"][miss] == b["bg_color"]).all())
    return rank


def _probe_by_hand(wd, rows, query_size):
    """growth.probe_hole on the given bank rows, the module's forward expanded to all rays here (fill_invalid's part for the probed keys)."""
    from hybridneuralrendering_amd import growth
    opt = wd.opt
    old = (opt.prob, opt.is_train, opt.query_size)
    opt.prob, opt.is_train, opt.query_size = 1, 0, list(query_size)
    frames = []
    try:
        for row in rows:
            it = wd.sampler.item(row)
            with torch.no_grad():
                out = wd.net.forward(raydir=it["raydir"][None], pixel_idx=it["pixel_idx"][None], campos=it["campos"][None], camrotc2w=it["camrotc2w"][None],
                                     bg_color=it["bg_color"][None], near=torch.tensor([it["near"]]), far=torch.tensor([it["far"]]),
                                     c2w_nearest=it["c2w_nearest"][None], campos_nearest=it["campos_nearest"][None],
                                     intrinsic_nearest=it["intrinsic_nearest"][None], images_nearest=it["images_nearest"][None])
            valid = out["ray_mask"][0] > 0
            R = valid.shape[0]
            full = {"ray_mask": out["ray_mask"]}
            for k in ("coarse_raycolor", "ray_max_sample_loc_w", "ray_max_far_dist", "ray_max_shading_opacity", "shading_avg_color", "shading_avg_dir",
                      "shading_avg_conf", "shading_avg_embedding"):
                buf = torch.zeros((1, R, out[k].shape[-1]), device=wd.dev)
                if k == "coarse_raycolor":
                    buf[:] = it["bg_color"]
                buf[0, valid] = out[k][0]
                full[k] = buf
            frames.append((full, it["pixel_idx"][None], it["gt_image"], it["bg_color"]))
        return growth.probe_hole(frames, wd.bank.H, wd.bank.W, far_thresh=0.0, opacity_thresh=opt.prob_thresh, prob_mul=opt.prob_mul)
    finally:
        opt.prob, opt.is_train, opt.query_size = old


def _tail(npts, n0):
    return [npts.xyz[n0:], npts.points_embeding[0, n0:], npts.points_color[0, n0:], npts.points_dir[0, n0:], npts.points_conf[0, n0:]]


def test_grow_pass_end_to_end():
    from hybridneuralrendering_amd import growth, scenes
    wd = _world()
    opt, npts = wd.opt, wd.npts
    rank = _train_and_rank(wd)
    state = rank.state_dict()
    rows = rank.top_frames(wd.bank.F // opt.prob_num_step)
    print("ray-miss table: ids %s losses %s -> frames %s" % (rank.ids.tolist(), rank.losses.tolist(), rows))
    assert len(rows) >= 2 and float(rank.worst()) > 1e-5
    n0 = int(npts.xyz.shape[0])
    qs0 = opt.query_size
    tier, qs = growth.probe_tier(50000, TIERS, KERNEL)
    assert tier == 1 and qs == [1, 1, 1] and list(qs0) == [3, 3, 3]
    want = _probe_by_hand(wd, rows, qs)
    assert int(want[0].shape[0]) >= 10
    # tier past the last: 0 and nothing rendered; prob_mode 1 raises
    fwd = wd.net.forward
    wd.net.forward = lambda *a, **k: (_ for _ in ()).throw(AssertionError("rendered"))
    try:
        assert growth.grow_pass(wd.net, wd.sampler, rank, 120001, opt) == 0
        opt.prob_mode = 1
        with pytest.raises(growth.HnrError):
            growth.grow_pass(wd.net, wd.sampler, rank, 50000, opt)
    finally:
        opt.prob_mode = 0
        wd.net.forward = fwd
    assert torch.equal(rank.ids, state["ids"]) and npts.xyz.shape[0] == n0
    # the pass
    n_new = growth.grow_pass(wd.net, wd.sampler, rank, 50000, opt)
    print("grow_pass: %d new points over frames %s (cloud %d -> %d)" % (n_new, rows, n0, npts.xyz.shape[0]))
    assert n_new == int(want[0].shape[0]) and int(npts.xyz.shape[0]) == n0 + n_new and int(npts.points_conf.shape[1]) == n0 + n_new
    for got, w in zip(_tail(npts, n0), want):
        assert torch.equal(got, w)
    assert opt.prob == 0 and opt.is_train == 1 and opt.query_size is qs0
    assert rank.ids.tolist() == list(range(rank.n)) and not bool(rank.losses.any())
    # a following query (the training neighbourhood again) names new ids
    pixg = scenes.pixel_grid(wd.sc.w, wd.sc.h)
    rays = _t(scenes.camera_rays(pixg, wd.sc.intrinsic, wd.sc.c2w))
    res = npts.querier.query_points(_t(pixg)[None], None, npts.xyz[None], None, wd.sc.h, wd.sc.w, wd.sc.intrinsic, wd.sc.near, wd.sc.far, rays[None],
                                    _t(wd.sc.c2w[:3, 3])[None], _t(wd.sc.c2w[:3, :3])[None])
    assert int((res[0] >= n0).sum()) > 0
    assert tuple(npts.querier._grid_key[6]) == (3, 3, 3)
    # the same pass in chunks of 1024 rays on a second copy of the world: the same points bit for bit
    wd2 = _world()
    rank2 = growth.RayMissRanking(wd2.bank.F, opt.prob_num_step, wd2.dev).load_state_dict(state)
    assert growth.grow_pass(wd2.net, wd2.sampler, rank2, 50000, wd2.opt, chunk_rays=1024) == n_new
    for a, b in zip(_tail(wd2.npts, n0), _tail(npts, n0)):
        assert torch.equal(a, b)
    # nothing to probe: an empty table gives 0
    assert growth.grow_pass(wd2.net, wd2.sampler, rank2, 50000, wd2.opt) == 0
