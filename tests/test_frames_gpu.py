"""GPU tests of the device-resident frame bank and its batch sampler (hybridneuralrendering_amd/frames.py, csrc/frames.hip): every output bit-equal to
the NumPy restatement tests/frames_ref.py and to the dataset items the reference produced (tests/golden/frames.npz; `raydir` within the recorded
`raydir_tol`, the reference's BLAS product against the sequential fp32 form), capture in a hipGraph, and the training step / frame driver fed
straight from the sampler.  12 train frames, V = 4; 48 x 64 frames and a 47 x 61 crop whose frames start at odd byte offsets."""
import os

import numpy as np
import pytest
import torch

from tests import frames_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
MARGIN = 3
_CACHE = {}


def _gold():
    if "g" not in _CACHE:
        _CACHE["g"] = dict(np.load(os.path.join(ROOT, "tests", "golden", "frames.npz")))
    return _CACHE["g"]


def _banks(size=(48, 64), per_frame_K=False, as_float=False):
    """(device train bank, device test bank, reference train bank, reference test bank) of the golden frames, cropped to `size`; built once per variant."""
    from hybridneuralrendering_amd.frames import FrameBank, nearest_by_id
    key = (size, per_frame_K, as_float)
    if key in _CACHE:
        return _CACHE[key]
    g = _gold()
    h, w = size
    crop = lambda a: np.ascontiguousarray(a[:, :h, :w])
    tr_img, te_img = crop(g["train_images"]), crop(g["test_images"])
    assert tr_img.min() == 0 and tr_img.max() == 255                            # the uint8 test images hold 0 and 255
    if as_float:
        rng = np.random.default_rng(3)
        tr_img, te_img = rng.uniform(0, 1, size=tr_img.shape).astype(np.float32), rng.uniform(0, 1, size=te_img.shape).astype(np.float32)
    K = g["K"]
    Ktr, Kte = K, K
    if per_frame_K:
        Ktr = np.stack([K + np.array([[0.25 * f, 0, 0.5 * f], [0, 0.125 * f, -0.25 * f], [0, 0, 0]], np.float32) for f in range(tr_img.shape[0])])
        Kte = np.stack([K + np.array([[1.5 * f, 0, 1.0], [0, 2.0, 0.5 * f], [0, 0, 0]], np.float32) for f in range(te_img.shape[0])])
    total, wexp = int(g["total_num_image"][0]), float(g["weight_exp"][0])
    tr = FrameBank(tr_img, g["train_c2w"], Ktr, DEV, ids=g["train_ids"], weights=list(g["weights"]), weight_exp=wexp, total_num_image=total)
    te = FrameBank(te_img, g["test_c2w"], Kte, DEV, ids=g["test_ids"], total_num_image=total)
    n_tr = nearest_by_id(g["train_ids"], g["train_ids"], 4, exclude_self=True)
    n_te = nearest_by_id(g["test_ids"], g["train_ids"], 4, exclude_self=False)
    tr.set_nearest(n_tr)
    te.set_nearest(n_te, reference=tr)
    rtr = R.RefBank(tr_img, g["train_c2w"], Ktr, tr.w2c.cpu().numpy(), ids=g["train_ids"], weights=g["weights"], weight_exp=wexp, total_num_image=total)
    rte = R.RefBank(te_img, g["test_c2w"], Kte, te.w2c.cpu().numpy(), ids=g["test_ids"], total_num_image=total)
    rtr.set_nearest(n_tr)
    rte.set_nearest(n_te, reference=rtr)
    # the bank's inverse poses (torch.inverse on the device) against the fp64 inverse
    inv = np.linalg.inv(g["train_c2w"].astype(np.float64))
    assert np.abs(tr.w2c.cpu().numpy() - inv).max() < 1e-5
    _CACHE[key] = (tr, te, rtr, rte)
    return _CACHE[key]


def _same(got, ref, what):
    for k, want in ref.items():
        key = "camrot" if k == "camrotc2w" and k not in got else k
        have = got[key].cpu().numpy()
        assert have.dtype == want.dtype, (what, k, have.dtype, want.dtype)
        assert have.shape == want.shape, (what, k, have.shape, want.shape)
        assert np.array_equal(have, want), (what, k, float(np.abs(have.astype(np.float64) - want.astype(np.float64)).max()))


MODE_CASES = [("random", dict(size=7), dict(dir_norm=1, bg_color="random")), ("random", dict(size=8), dict(downweight_blurry_feats=1)),
              ("dilated", dict(dilation_setup="3_4_1_3"), dict()), ("patch", dict(size=8), dict(bg_color=(0.0, 0.5, 1.0)))]


@pytest.mark.parametrize("size", [(48, 64), (47, 61)], ids=["48x64", "47x61"])
@pytest.mark.parametrize("case", range(len(MODE_CASES)), ids=["random7", "random8", "dilated3x4", "patch8"])
def test_every_mode_equals_the_restatement_bit_for_bit(size, case):
    from hybridneuralrendering_amd.frames import BatchSampler
    tr, _te, rtr, _rte = _banks(size)
    mode, shape_kw, kw = MODE_CASES[case]
    seed, sched = 0x1234567890ABCDEF + case, [7, 0, 11]
    s = BatchSampler(tr, mode, margin=MARGIN, seed=seed, near=0.1, far=8.0, **shape_kw, **kw).set_schedule(sched)
    first = None
    for step in range(5):
        got = s.next()
        ref = R.batch(rtr, sched, mode, seed, step, margin=MARGIN, dir_norm=bool(kw.get("dir_norm")), bg=kw.get("bg_color", (1, 1, 1)),
                      downweight=bool(kw.get("downweight_blurry_feats")), **shape_kw)
        _same(got, ref, (mode, size, step))
        assert got["camrotc2w"] is got["camrot"] and got["h"] == size[0] and got["w"] == size[1] and got["near"] == 0.1 and got["far"] == 8.0
        if first is None:
            first = got
        assert all(got[k] is first[k] for k in got)                             # the same static tensors on every call
        px = got["pixel_idx"].cpu().numpy()
        assert px[:, 0].min() >= MARGIN and px[:, 0].max() < size[1] - MARGIN and px[:, 1].min() >= MARGIN and px[:, 1].max() < size[0] - MARGIN
    assert int(s.step.item()) == 5
    assert got["raydir"].shape[0] == (49 if case == 0 else 64 if case in (1, 3) else 144)


def test_items_equal_the_reference_goldens():
    """item(row, pixels = the golden pixel_idx) against what ScannetFtDataset.__getitem__ returned: the exact fields bit for bit, raydir within
    raydir_tol; item(row) is the golden no_crop item."""
    from hybridneuralrendering_amd.frames import BatchSampler
    g = _gold()
    tr, te, _rtr, _rte = _banks()
    tol = float(g["raydir_tol"][0])
    for case in g["item_cases"]:
        bank, row, base = (tr if str(case).startswith("train") else te), int(str(case)[-1]), "item_" + str(case)
        for mode in ("random", "random_norm", "patch", "dilated", "no_crop"):
            s = BatchSampler(bank, "random", size=4, margin=MARGIN, dir_norm=int(mode.endswith("_norm")), near=0.1, far=8.0, downweight_blurry_feats=1)
            pix = g["%s_%s_pixel_idx" % (base, mode)]
            got = s.item(row) if mode == "no_crop" else s.item(row, pixels=pix)
            f = lambda k: got[k].cpu().numpy()
            assert np.array_equal(f("pixel_idx"), pix), (case, mode)
            assert np.array_equal(f("gt_image"), g["%s_%s_gt_image" % (base, mode)]), (case, mode)
            err = float(np.abs(f("raydir").astype(np.float64) - g["%s_%s_raydir" % (base, mode)]).max())
            print("%s %s: %d rays, raydir max |d| vs the reference %.3g (tol %.3g)" % (case, mode, len(pix), err, tol))
            assert err <= tol, (case, mode, err)
        assert np.array_equal(f("images_nearest"), g[base + "_images_nearest"])
        for k in ("c2w_nearest", "campos_nearest", "campos", "camrotc2w", "c2w"):
            assert np.array_equal(f(k), g[base + "_" + k]), (case, k)
        for k in ("frame_weight", "frame_weight_nearest", "vid_angle_nearest"):
            assert np.array_equal(f(k), g[base + "_" + k].astype(np.float32)), (case, k)
        assert np.array_equal(f("intrinsic_nearest"), g["K"]) and int(f("frame_row")[0]) == row
        assert "patch_table" not in got and got["h"] == 48 and got["w"] == 64


@pytest.mark.parametrize("size", [(48, 64), (47, 61)], ids=["48x64", "47x61"])
def test_a_float32_bank_gives_bit_copies(size):
    from hybridneuralrendering_amd.frames import BatchSampler
    tr, _te, rtr, _rte = _banks(size, as_float=True)
    s = BatchSampler(tr, "random", size=7, margin=1, seed=9, near=0.1, far=8.0).set_schedule([3, 8])
    for step in range(2):
        _same(s.next(), R.batch(rtr, [3, 8], "random", 9, step, margin=1, size=7), ("float bank", size, step))
    got = s.item(5)
    px, py = R.no_crop_pixels(size[0], size[1], 1)
    _same(got, R.item(rtr, 5, px, py), ("float bank item", size))
    assert got["images_nearest"].dtype == torch.float32 and torch.equal(got["images_nearest"], tr.images[tr.nearest[5].long()])


def test_per_frame_intrinsics_are_honoured():
    from hybridneuralrendering_amd.frames import BatchSampler
    tr, te, rtr, rte = _banks(per_frame_K=True)
    s = BatchSampler(tr, "random", size=8, margin=MARGIN, seed=21, near=0.1, far=8.0).set_schedule([2, 9])
    rays = []
    for step in range(2):
        got = s.next()
        _same(got, R.batch(rtr, [2, 9], "random", 21, step, margin=MARGIN, size=8), ("per-frame K", step))
        assert np.array_equal(got["intrinsic"].cpu().numpy(), rtr.K[[2, 9][step]])
        rays.append(got["raydir"].clone())
    # the same pixels of one frame through another frame's K give other rays
    pix = torch.tensor([[10.0, 12.0], [40.0, 30.0]])
    a, b = s.item(2, pixels=pix)["raydir"], R.raydir(pix[:, 0].numpy(), pix[:, 1].numpy(), rtr.K[3], rtr.c2w[2][:3, :3])
    assert not np.array_equal(a.cpu().numpy(), b)
    ts = BatchSampler(te, "random", size=8, margin=MARGIN, near=0.1, far=8.0)
    px, py = R.no_crop_pixels(48, 64, MARGIN)
    _same(ts.item(1), R.item(rte, 1, px, py), "per-frame K, test bank")


def test_a_test_bank_takes_its_views_from_the_train_bank():
    from hybridneuralrendering_amd.frames import BatchSampler
    tr, te, rtr, rte = _banks()
    s = BatchSampler(te, "patch", size=8, margin=MARGIN, seed=4, near=0.1, far=8.0, downweight_blurry_feats=1).set_schedule([1, 0])
    for step in range(3):
        got = s.next()
        _same(got, R.batch(rte, [1, 0], "patch", 4, step, margin=MARGIN, size=8, downweight=True), ("test bank", step))
        row = [1, 0][step % 2]
        nr = te.nearest[row].long()
        assert torch.equal(got["c2w_nearest"], tr.c2w[nr]) and torch.equal(got["w2c_nearest"], tr.w2c[nr]) and torch.equal(got["frame_weight_nearest"], tr.weight[nr])
        # (NumPy's division, not torch's on the device: that one is not correctly rounded)
        assert np.array_equal(got["images_nearest"].cpu().numpy(), R.to_float(tr.images[nr].cpu().numpy())) and torch.equal(got["c2w"], te.c2w[row])
        assert float(got["frame_weight"]) == 1.0


def test_the_seed_decides_the_sequence():
    from hybridneuralrendering_amd.frames import BatchSampler
    tr = _banks()[0]
    mk = lambda seed: BatchSampler(tr, "random", size=8, margin=MARGIN, seed=seed, near=0.1, far=8.0).set_schedule([0, 1, 2])
    a, b, c = mk(5), mk(5), mk(6)
    differs = False
    for _ in range(3):
        pa, pb, pc = a.next()["pixel_idx"].clone(), b.next()["pixel_idx"].clone(), c.next()["pixel_idx"].clone()
        assert torch.equal(pa, pb)
        differs |= not torch.equal(pa, pc)
    assert differs
    assert not torch.equal(mk(5).next()["pixel_idx"], pa)                       # another step, another batch
    assert torch.equal(mk(5).set_step(2).next()["pixel_idx"], pa)               # resuming at a step gives that step's batch


@pytest.mark.parametrize("form", ["static", "out"])
def test_next_marks_what_it_wrote_and_the_feature_map_follows(form):
    """next() writes the same tensors on every call, from kernels torch knows nothing of: it marks them as written (_cache.py, rule 3), so a
    renderer that cached the feature map of the first frame's reference views builds the second frame's."""
    from hybridneuralrendering_amd import scenes
    from hybridneuralrendering_amd.aggregator import PointAggregator
    from hybridneuralrendering_amd.frames import BatchSampler
    from hybridneuralrendering_amd.render import HybridRenderer
    tr = _banks()[0]
    opt = scenes.default_opt()
    torch.manual_seed(0)
    agg = PointAggregator(opt).to(DEV)
    rnd = HybridRenderer(opt, agg, torch.device(DEV))
    s = BatchSampler(tr, "random", size=8, margin=MARGIN, near=0.1, far=8.0).set_schedule([7, 0])
    out = None if form == "static" else dict(images_nearest=torch.empty((4, 48, 64, 3), device=DEV), raydir=torch.empty((64, 3), device=DEV))
    a = s.next(out=out)
    img = a["images_nearest"]
    v0, first = img._version, img.clone()
    fm0 = rnd.feature_map(img).clone()
    assert torch.equal(fm0, agg.image_features(img))
    b = s.next(out=out)
    assert b["images_nearest"] is img and img._version > v0 and b["raydir"]._version > 0
    assert not torch.equal(img, first)                                          # (another frame, other reference views)
    fm1 = rnd.feature_map(img)
    assert torch.equal(fm1, agg.image_features(img)) and not torch.equal(fm1, fm0)


def test_next_is_capturable_and_replays_the_following_steps():
    """next() captured in a torch.cuda.graph on one side stream after a warm-up call and replayed three times gives the batches of steps 1..3 that a
    second sampler with the same seed gives eagerly; the counter ends at 4; the three-row schedule wraps."""
    from hybridneuralrendering_amd.frames import BatchSampler
    tr = _banks((47, 61))[0]
    dev = torch.device(DEV)
    mk = lambda: BatchSampler(tr, "dilated", dilation_setup="3_4_1_3", margin=MARGIN, seed=77, near=0.1, far=8.0, bg_color="random").set_schedule([4, 10, 6])
    cap, eager = mk(), mk()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        out = cap.next()                                                        # step 0: the static tensors exist before the capture
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        out2 = cap.next()
    assert all(out2[k] is out[k] for k in out)
    want = [{k: v.clone() for k, v in eager.next().items() if isinstance(v, torch.Tensor)} for _ in range(4)]
    rows = []
    for k in range(1, 4):
        graph.replay()
        torch.cuda.synchronize(dev)
        for name, t in want[k].items():
            assert torch.equal(out[name], t), (k, name)
        rows.append(int(out["frame_row"].item()))
    assert rows == [10, 6, 4] and int(cap.step.item()) == 4 and int(eager.step.item()) == 4
    assert not torch.equal(want[1]["pixel_idx"], want[2]["pixel_idx"])


def test_sampler_feeds_the_captured_training_step():
    """The train_scannet_small fixture's cloud and weights; its four reference views plus one target frame as a float32 bank.
    `sampler.next(out=cap.inputs); cap.step()` equals train_step(..., device_frame_weight=...) on the same batch tensors (the comparison of
    test_captured_train_step_replays_bit_identically_and_follows_its_inputs); keys of cap.inputs the sampler does not know keep their values."""
    from hybridneuralrendering_amd.frames import FrameBank, BatchSampler
    from hybridneuralrendering_amd.train import train_step, CapturedTrainStep
    from tests.test_train_gpu import _setup, _leaves
    d, ti, opt, agg, path = _setup()
    dev = ti["emb"].device
    near, far = (float(x) for x in d["near_far"])
    tmid = torch.from_numpy(d["tmid"]).to(dev)
    rng = np.random.default_rng(5)
    images = np.concatenate([d["images_nearest"], rng.uniform(0, 1, size=(1,) + d["images_nearest"].shape[1:]).astype(np.float32)])
    c2w = np.concatenate([d["c2w_nearest"], d["c2w"][None]])
    bank = FrameBank(images, c2w, d["intrinsic"], dev, weights=[1.0, 1.0, 1.0, 1.0, 0.7])
    bank.set_nearest(np.array([[1, 2, 3, 4], [0, 2, 3, 4], [0, 1, 3, 4], [0, 1, 2, 4], [0, 1, 2, 3]]))
    setup = str(d["opt"]["dilation_setup"])
    mk = lambda: BatchSampler(bank, "dilated", dilation_setup=setup, seed=13, near=near, far=far, bg_color=tuple(float(c) for c in d["bg_color"])).set_schedule([4])
    b = mk().next()
    assert b["raydir"].shape == ti["raydir"][0].shape and float(b["frame_weight"]) == float(np.float32(0.7))
    assert torch.equal(b["images_nearest"], ti["images_nearest"][0]) and torch.equal(b["c2w_nearest"], ti["c2w_nearest"][0])
    emb, conf, pdir, color = _leaves(ti)
    agg.zero_grad(set_to_none=True)
    out, pg, ag = train_step(path, agg, ti["xyz"], emb, conf, pdir, color, b["raydir"], b["campos"], b["camrotc2w"], b["bg_color"], b["near"], b["far"],
                             b["c2w_nearest"], b["campos_nearest"], b["intrinsic_nearest"], b["images_nearest"], b["gt_image"],
                             zero_epsilon=float(d["zero_epsilon"]), tmid=tmid, w2c_nearest=b["w2c_nearest"], device_frame_weight=b["frame_weight"])
    ref = (out["loss"].clone(), out["coarse_raycolor"].clone(), {k: v.clone() for k, v in pg.items()}, {k: v.clone() for k, v in ag.items()})
    # the device weight is what scaled the loss: the host-float form of the same step gives the same bits
    for t in (emb, conf, pdir, color):
        t.grad = None
    agg.zero_grad(set_to_none=True)
    out_h, _pg, _ag = train_step(path, agg, ti["xyz"], emb, conf, pdir, color, b["raydir"], b["campos"], b["camrotc2w"], b["bg_color"], near, far,
                                 b["c2w_nearest"], b["campos_nearest"], b["intrinsic_nearest"], b["images_nearest"], b["gt_image"],
                                 zero_epsilon=float(d["zero_epsilon"]), tmid=tmid, w2c_nearest=b["w2c_nearest"], frame_weight=float(np.float32(0.7)))
    assert torch.equal(out_h["loss"], ref[0])
    gt0 = torch.from_numpy(d["gt"][0]).to(dev)
    sample = dict(raydir=ti["raydir"][0], campos=ti["campos"][0], camrot=ti["camrotc2w"][0], bg_color=ti["bg_color"][0], c2w_nearest=ti["c2w_nearest"][0],
                  campos_nearest=ti["campos_nearest"][0], intrinsic_nearest=ti["intrinsic_nearest"][0], images_nearest=ti["images_nearest"][0],
                  gt_image=gt0, tmid=tmid, frame_weight=0.3)
    for t in (emb, conf, pdir, color):
        t.grad = None
    cap = CapturedTrainStep(path, agg, ti["xyz"], emb, conf, pdir, color, sample, near, far, zero_epsilon=float(d["zero_epsilon"]))
    s = mk()
    res = s.next(out=cap.inputs)
    assert res is cap.inputs
    assert torch.equal(cap.inputs["tmid"], tmid)                                 # an input the sampler does not know: untouched
    for k in ("raydir", "gt_image", "campos", "bg_color", "c2w_nearest", "w2c_nearest", "campos_nearest", "intrinsic_nearest", "images_nearest", "frame_weight"):
        assert torch.equal(cap.inputs[k].reshape(b[k].shape), b[k]), k
    assert torch.equal(cap.inputs["camrot"], b["camrot"])
    got, gpg, gag = cap.step()
    assert torch.equal(got["loss"], ref[0]), (got["loss"], ref[0])
    assert torch.equal(got["coarse_raycolor"], ref[1])
    for k in ref[2]:
        assert torch.equal(gpg[k], ref[2][k]), k
    for k in ref[3]:
        sc = float(ref[3][k].abs().max())
        # float-atomic sums in a few narrow layers; a lone scalar (aux_merge_weight_block.6.bias) is a sum of signed terms that nearly cancel
        assert float((gag[k] - ref[3][k]).abs().max()) <= (1e-3 if ref[3][k].numel() == 1 else 2e-6) * max(sc, 1e-30), k
    assert int(s.step.item()) == 1 and float(got["loss"][3]) > 0


def test_render_image_takes_the_sampler_item():
    """driver.render_image(renderer, cloud, sampler.item(row)) runs, and its image is zero exactly on the margin."""
    from hybridneuralrendering_amd.frames import FrameBank, BatchSampler
    from hybridneuralrendering_amd.driver import render_image
    from tests.test_render_gpu import _setup
    d, ti, opt, cloud, rnd = _setup("scannet_small")
    dev = ti["xyz"].device
    images = np.concatenate([d["images_nearest"], d["images_nearest"][:1]])
    c2w = np.concatenate([d["c2w_nearest"], d["c2w"][None]])
    bank = FrameBank(images, c2w, d["intrinsic"], dev)
    bank.set_nearest(np.array([[1, 2, 3, 4], [0, 2, 3, 4], [0, 1, 3, 4], [0, 1, 2, 4], [0, 1, 2, 3]]))
    near, far = (float(x) for x in d["near_far"])
    m = 5
    s = BatchSampler(bank, "random", size=8, margin=m, near=near, far=far)
    item = s.item(4)
    assert item["raydir"].shape[0] == (48 - 2 * m) * (64 - 2 * m)
    out = render_image(rnd, cloud, item)
    img = out["image"]
    assert tuple(img.shape) == (48, 64, 3) and int(out["ray_mask"].sum()) > 100
    inner = torch.zeros((48, 64), dtype=torch.bool, device=dev)
    inner[m:48 - m, m:64 - m] = True
    nz = img.abs().sum(dim=-1) > 0
    assert torch.equal(nz, inner)
    # the rays are the fixture camera's: the same pixels through the golden frame driver's own ray builder
    from hybridneuralrendering_amd import scenes
    pix = item["pixel_idx"].cpu().numpy().astype(np.int32)
    want = scenes.camera_rays(pix, d["intrinsic"], d["c2w"])
    assert np.abs(item["raydir"].cpu().numpy() - want).max() < 1e-5


def test_bad_arguments_raise():
    import ctypes
    from hybridneuralrendering_amd import _lib
    from hybridneuralrendering_amd.frames import FrameBank, BatchSampler, HnrError
    g = _gold()
    tr = _banks()[0]
    kw = dict(near=0.1, far=8.0)
    with pytest.raises(HnrError, match="empty range"):
        BatchSampler(tr, "random", size=8, margin=24, **kw)                     # the margin empties the range of py
    with pytest.raises(HnrError, match="larger than the frame"):
        BatchSampler(tr, "patch", size=49, **kw)
    with pytest.raises(HnrError):
        BatchSampler(tr, "dilated", dilation_setup="3_4_1_16", margin=MARGIN, **kw)     # (4 - 1) * 16 pixels do not fit 48 - 6
    with pytest.raises(HnrError):
        BatchSampler(tr, "random2", size=8, **kw)
    with pytest.raises(HnrError):
        BatchSampler(tr, "random", size=8)                                      # near / far missing
    s = BatchSampler(tr, "random", size=8, **kw)
    with pytest.raises(HnrError, match="no schedule"):
        s.next()
    with pytest.raises(HnrError):
        s.set_schedule([0, 12])
    s.set_schedule([0, 1])
    dev = torch.device(DEV)
    with pytest.raises(HnrError, match="raydir"):
        s.next(out=dict(raydir=torch.zeros((63, 3), device=dev)))
    with pytest.raises(HnrError, match="gt_image"):
        s.next(out=dict(gt_image=torch.zeros((64, 3), dtype=torch.float64, device=dev)))
    with pytest.raises(HnrError):
        s.next(out=dict(raydir=torch.zeros((64, 3))))                           # a host tensor
    assert int(s.step.item()) == 0                                              # nothing ran
    with pytest.raises(HnrError, match="outside the reference bank"):
        FrameBank(g["test_images"], g["test_c2w"], g["K"], DEV).set_nearest(np.array([[0, 1, 2, 12], [0, 1, 2, 3]]), reference=tr)
    with pytest.raises(HnrError):
        tr.__class__(g["test_images"][:, :40], g["test_c2w"], g["K"], DEV).set_nearest(np.zeros((2, 4), np.int32), reference=tr)   # another frame size
    with pytest.raises(HnrError):
        FrameBank(g["train_images"].astype(np.float64), g["train_c2w"], g["K"], DEV)
    with pytest.raises(HnrError):
        FrameBank(g["train_images"], g["train_c2w"], g["K"], "cpu")
    with pytest.raises(HnrError):
        s.item(12)
    # the C entry points: a negative status and a message, never an abort
    L = _lib.lib()
    assert L.hnr_frame_batch(None, None, None, 0, None, None, 0, None, None, None, 0, None) == -1 and b"hnr_frame_batch" in L.hnr_last_error()
    prm = _lib.FrameBatchParams(1, 49, 0, 0, 0, 0, 0, 0, 0, 0, (ctypes.c_float * 3)(1, 1, 1), 0)
    o = _lib.FrameBatchOut()
    assert L.hnr_frame_batch(ctypes.byref(tr._c), ctypes.byref(tr._c), _lib.ptr(tr.nearest), 4, ctypes.byref(prm), _lib.ptr(s.schedule), 2, _lib.ptr(s.step),
                             ctypes.byref(o), _lib.ptr(s._scratch), 16, None) == -1
    assert b"empty range" in L.hnr_last_error() and L.hnr_frame_batch_scratch_bytes(7, 1) == -1
    assert L.hnr_frame_item(ctypes.byref(tr._c), None, None, 0, 12, None, 10, 0, 0, (ctypes.c_float * 3)(1, 1, 1), 0, ctypes.byref(o), _lib.ptr(s._scratch), 16, None) == -1
