"""GPU tests of camera paths (csrc/path.hip, frames.PathSampler, driver.render_path):

 * hnr_pose_views against the NumPy restatement tests/path_ref.py, pick for pick and in order, with every tie it must decide;
 * hnr_path_item with the pose table set to a test bank's own cameras: every output bit-equal to BatchSampler.item(row) of that bank once its
   nearest table is views(); the device counter, poses rewritten on the device, capture in a hipGraph, sentinels behind every output;
 * hnr_frame_store: the bytes of hnr_frame_metrics, the floats of the torch scatter, nothing outside the frame it was given;
 * render_path end to end on the scannet_small twin scene against render_image on the same items."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import path_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_CACHE = {}


def _camera_bank(T, seed, H=6, W=8, per_frame_K=False, images=None, as_float=False, weights=False):
    """T look-at cameras as a FrameBank of H x W frames (tiny by default: the selection reads cameras only) -> (bank, c2w, K as uploaded)"""
    from hybridneuralrendering_amd.frames import FrameBank
    c2w, K = R.lookat_cameras(T, seed, W, H, focal=0.9375 * W)
    rng = np.random.default_rng(seed + 1000)
    if per_frame_K:
        K = np.stack([K + np.array([[0.25 * (f % 7), 0, 0.125 * (f % 5)], [0, 0.5 * (f % 3), -0.25 * (f % 4)], [0, 0, 0]], np.float32) for f in range(T)])
    if images is None:
        images = rng.integers(0, 256, size=(T, H, W, 3), dtype=np.uint8)
        if as_float:
            images = rng.uniform(0, 1, size=(T, H, W, 3)).astype(np.float32)
    w = list(rng.uniform(0.2, 1.0, size=T)) if weights else None
    return FrameBank(images, c2w, K, DEV, weights=w), c2w, K


# ---------------------------------------------------------------------------------------------------------------- hnr_pose_views
VIEW_CASES = [(40, 4, 7, 3), (64, 1, 1, 3), (120, 8, 65, 3), (257, 4, 65, 3), (1030, 8, 65, 12), (8192, 4, 3, 300)]


@pytest.mark.parametrize("T,V,Q,num_times", VIEW_CASES, ids=["T%d-V%d-Q%d" % c[:3] for c in VIEW_CASES])
@pytest.mark.parametrize("K_mode", ["shared", "per_query", "bank_per_frame"])
def test_pose_views_equal_the_restatement(T, V, Q, num_times, K_mode):
    from hybridneuralrendering_amd.frames import PathSampler
    H, W = 6, 8
    bank, tr, Ktr = _camera_bank(T, 10 + T, H, W, per_frame_K=(K_mode == "bank_per_frame"))
    qs, Kq = R.lookat_cameras(Q, 77 + T, W, H, focal=0.9375 * W)
    if K_mode == "per_query":
        Kq = np.stack([Kq + np.array([[0.5 * (q % 3), 0, 0.25 * (q % 5)], [0, 0.25 * (q % 4), 0.5 * (q % 2)], [0, 0, 0]], np.float32) for q in range(Q)])
    s = PathSampler(qs, Kq, bank, V, near=0.1, far=8.0, num_times=num_times)
    n1 = min(num_times * V, T // 10)
    assert s.n1 == n1 and n1 >= V
    got = s.views()
    want = R.pose_views(tr, Ktr, qs, Kq, W, H, V, n1)
    assert got.dtype == torch.int32 and tuple(got.shape) == (Q, V)
    assert np.array_equal(got.cpu().numpy(), want), (T, V, Q, K_mode)
    assert torch.equal(s.views(), got)                                           # two runs, identical bits


def test_pose_views_decide_ties_exclusions_and_the_smallest_candidate_set():
    from hybridneuralrendering_amd.frames import FrameBank, PathSampler, HnrError
    H, W, T, V = 6, 8, 60, 4
    tr, K = R.lookat_cameras(T, 5, W, H, focal=0.9375 * W)
    tr[41] = tr[17]                                                              # two identical train cameras
    tr[30] = tr[17]
    tr[30, :3, 3] += np.float32(0.25) * tr[17, :3, 2]                            # ... and one with the same direction (a step-1 tie alone) further back
    bank = FrameBank(np.zeros((T, H, W, 3), np.uint8), tr, K, DEV)
    q = tr[[17, 3, 9]].copy()
    s = PathSampler(q, K, bank, V, near=0.1, far=8.0)                            # n1 = min(12, 6) = 6
    got = s.views().cpu().numpy()
    assert np.array_equal(got, R.pose_views(tr, K, q, K, W, H, V, s.n1))
    assert got[0, 0] == 17 and got[0, 1] == 41 and 30 in got[0]                  # equal score and distance: the lower row first
    assert got[1, 0] == 3 and got[2, 0] == 9
    # exclude rows: hit (17: the next candidate moves up), not hit (6 is not query 1's first row), none
    ex = np.array([17, 6, -1], np.int32)
    gx = s.views(exclude_rows=ex).cpu().numpy()
    assert np.array_equal(gx, R.pose_views(tr, K, q, K, W, H, V, s.n1, exclude_rows=ex))
    assert gx[0, 0] == 41 and 17 not in gx[0] and np.array_equal(gx[1], got[1]) and np.array_equal(gx[2], got[2])
    # n1 == V: every candidate of step 1 is a view; an exclusion then has nothing left to give
    s4 = PathSampler(q, K, bank, V, near=0.1, far=8.0, num_times=1)
    assert s4.n1 == V
    g4 = s4.views().cpu().numpy()
    assert np.array_equal(g4, R.pose_views(tr, K, q, K, W, H, V, V))
    with pytest.raises(HnrError, match="excluded"):
        s4.views(exclude_rows=ex)
    # other poses than the sampler's own
    other, _ = R.lookat_cameras(9, 123, W, H)
    assert np.array_equal(s.views(torch.from_numpy(other).to(DEV)).cpu().numpy(), R.pose_views(tr, K, other, K, W, H, V, s.n1))


# ---------------------------------------------------------------------------------------------------------------- hnr_path_item
def _pair(size, V, as_float=False, per_frame_K=False):
    """(train bank of 10 V + 3 cameras, test bank of 5 cameras) with frames of size = (H, W); built once per variant"""
    key = ("pair", size, V, as_float, per_frame_K)
    if key not in _CACHE:
        H, W = size
        tr, _c, _K = _camera_bank(10 * V + 3, 31 + V, H, W, per_frame_K=per_frame_K, as_float=as_float, weights=True)
        te, _c, _K = _camera_bank(5, 57 + V, H, W, per_frame_K=per_frame_K, as_float=as_float)
        _CACHE[key] = (tr, te)
    return _CACHE[key]


def _same_item(got, want, what):
    keys = set(k for k in want if k not in ("gt_image", "frame_weight"))
    assert keys == set(got), (what, sorted(keys ^ set(got)))
    for k in keys:
        if isinstance(want[k], torch.Tensor):
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
            assert torch.equal(got[k], want[k]), (what, k)
        else:
            assert got[k] == want[k], (what, k)


ITEM_CASES = [((20, 24), 0, 4, False, False), ((20, 24), 2, 1, False, True), ((19, 25), 0, 8, False, False), ((19, 25), 2, 4, False, True),
              ((19, 25), 2, 4, True, False), ((20, 24), 0, 1, True, False), ((80, 96), 2, 8, False, False)]


@pytest.mark.parametrize("size,margin,V,as_float,per_frame_K", ITEM_CASES,
                         ids=["%dx%d-m%d-V%d%s%s" % (c[0][1], c[0][0], c[1], c[2], "-f32" if c[3] else "", "-Kpf" if c[4] else "") for c in ITEM_CASES])
def test_path_items_equal_the_bank_items_bit_for_bit(size, margin, V, as_float, per_frame_K):
    from hybridneuralrendering_amd.frames import BatchSampler, PathSampler
    tr, te = _pair(size, V, as_float, per_frame_K)
    kw = dict(margin=margin, dir_norm=int(V == 4), bg_color=(0.25, 0.5, 1.0), near=0.1, far=8.0, downweight_blurry_feats=int(V != 1))
    s = PathSampler(te.c2w, te.intrinsic, tr, V, **kw)
    assert s.P == 5 and s.poses.data_ptr() != te.c2w.data_ptr()                 # the sampler's own table
    views = s.views()
    te.set_nearest(views.cpu().numpy(), reference=tr)
    b = BatchSampler(te, "random", size=4, **kw)
    for row in (0, 3, 4):
        got, want = s.item(row), b.item(row)
        _same_item(got, want, (size, margin, V, row))
        assert got["camrotc2w"] is got["camrot"] and int(got["frame_row"]) == row
        assert got["raydir"].shape[0] == (size[0] - 2 * margin) * (size[1] - 2 * margin)
        assert torch.equal(got["c2w_nearest"], tr.c2w[views[row].long()])


def test_next_follows_the_device_counter_and_the_device_poses():
    from hybridneuralrendering_amd.frames import BatchSampler, PathSampler
    tr, te = _pair((19, 25), 4)
    kw = dict(margin=2, near=0.1, far=8.0)
    s = PathSampler(te.c2w, te.intrinsic, tr, 4, **kw)
    te.set_nearest(s.views().cpu().numpy(), reference=tr)
    b = BatchSampler(te, "random", size=4, **kw)
    first = None
    for k in range(3):
        got = s.next()
        _same_item(got, b.item(k), ("next", k))
        first = got if first is None else first
        assert all(got[n] is first[n] for n in got)                              # the same static tensors on every call
    assert int(s.step.item()) == 3
    s.set_step(s.P - 1)
    assert int(s.next()["frame_row"]) == s.P - 1 and int(s.next()["frame_row"]) == 0 and int(s.step.item()) == s.P + 1        # the counter wraps at P
    # poses rewritten on the device: frame 0 becomes the camera of bank row 3; its views follow the new pose
    new = te.c2w.clone()
    new[0] = te.c2w[3]
    s.set_poses(new)
    got, want = s.item(0), b.item(3)
    for k in ("raydir", "campos", "camrot", "c2w", "c2w_nearest", "w2c_nearest", "campos_nearest", "images_nearest", "frame_weight_nearest", "vid_angle_nearest"):
        assert torch.equal(got[k], want[k]), k
    assert int(got["frame_row"]) == 0
    s.poses[1].copy_(te.c2w[4])                                                  # ... or written in place by anything that runs on the device
    assert torch.equal(s.set_step(1).next()["c2w"], te.c2w[4])


def test_next_writes_into_given_tensors_and_nothing_behind_them():
    from hybridneuralrendering_amd.frames import PathSampler
    tr, te = _pair((19, 25), 4)
    s = PathSampler(te.c2w, te.intrinsic, tr, 4, margin=2, near=0.1, far=8.0, downweight_blurry_feats=1)
    want = s.item(2)
    bufs, out = {}, {}
    for k, (shape, dt) in s._shapes().items():
        n = int(np.prod(shape))
        fill = 0x5A5A5A5A if dt == torch.int32 else 12345.0
        bufs[k] = torch.full((n + 64,), fill, dtype=dt, device=DEV)
        out[k] = bufs[k][:n].view(shape)
    res = s.set_step(2).next(out=out)
    assert res is out
    for k, t in out.items():
        assert torch.equal(t, want[k]), k
        assert bool((bufs[k][t.numel():] == bufs[k][-1]).all()) and bufs[k][-1].item() in (0x5A5A5A5A, 12345.0), k
    # a subset: the others are not touched
    keep = {k: v.clone() for k, v in out.items()}
    s.next(out=dict(raydir=out["raydir"], camrotc2w=out["camrot"]))
    assert torch.equal(out["camrot"], s.item(3)["camrot"]) and all(torch.equal(out[k], keep[k]) for k in out if k not in ("raydir", "camrot"))


def test_next_is_capturable_and_replays_the_following_frames():
    """next() captured in a torch.cuda.graph on one side stream after a warm-up call and replayed three times gives frames 1..3 that a second
    sampler gives eagerly (tests/test_frames_gpu.py::test_next_is_capturable_and_replays_the_following_steps: one stream, no parallel branches)."""
    from hybridneuralrendering_amd.frames import PathSampler
    tr, te = _pair((19, 25), 4)
    dev = torch.device(DEV)
    mk = lambda: PathSampler(te.c2w[:3], te.intrinsic, tr, 4, margin=2, near=0.1, far=8.0)
    cap, eager = mk(), mk()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        out = cap.next()                                                        # frame 0: the static tensors exist before the capture
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
    assert rows == [1, 2, 0] and int(cap.step.item()) == 4 and int(eager.step.item()) == 4
    assert not torch.equal(want[1]["raydir"], want[2]["raydir"])


# ---------------------------------------------------------------------------------------------------------------- hnr_frame_store
def _metrics_bytes(img):
    """hnr_frame_metrics's d_img8 for a float image [h,w,3] on the device"""
    from hybridneuralrendering_amd import _lib
    L = _lib.lib()
    h, w = int(img.shape[0]), int(img.shape[1])
    nbytes = int(L.hnr_frame_metrics_scratch_bytes(h, w, 11))
    assert nbytes >= 0
    scratch = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=img.device)
    row = torch.zeros((64,), dtype=torch.float64, device=img.device)
    a8, b8 = torch.zeros((h, w, 3), dtype=torch.uint8, device=img.device), torch.zeros((h, w, 3), dtype=torch.uint8, device=img.device)
    p = _lib.ptr
    _lib.check(L.hnr_frame_metrics(p(img), p(torch.zeros_like(img)), h, w, None, None, None, 0, 11, 2.0, p(row), p(a8), p(b8), p(scratch), _lib.stream()),
               "hnr_frame_metrics")
    return a8


def _store(col, pix, depth, h, w, img8=None, image=None, dimg=None):
    from hybridneuralrendering_amd import _lib
    p = _lib.ptr
    _lib.check(_lib.lib().hnr_frame_store(p(col), p(pix), p(depth), int(pix.shape[0]), h, w, p(img8), p(image), p(dimg), _lib.stream()), "hnr_frame_store")


def test_frame_store_writes_the_bytes_of_frame_metrics_and_only_its_frame():
    h, w = 20, 24
    rng = np.random.default_rng(8)
    yy, xx = np.mgrid[0:h, 0:w]
    cast = ((xx + 2 * yy) % 7 != 3)                                              # the pixels no ray reaches
    cast[0, 0] = cast[h - 1, w - 1] = True
    px, py = xx[cast].astype(np.float32), yy[cast].astype(np.float32)
    n = px.shape[0]
    order = rng.permutation(n)                                                   # rays in no particular order
    px, py = px[order], py[order]
    col = rng.uniform(-0.2, 1.2, size=(n, 3)).astype(np.float32)
    special = np.array([-0.0, 0.0, -3.0, 7.0, np.inf, -np.inf, np.nan, 1.0, np.nextafter(np.float32(1), np.float32(0))] + [k / 255 for k in range(256)],
                       dtype=np.float32)
    col.reshape(-1)[:special.size] = special
    dep = rng.uniform(0.5, 4.0, size=n).astype(np.float32)
    # rays whose pixel is outside the frame (or no number): dropped
    out_px = np.array([[-1, 3], [w, 3], [5, h], [5, -2], [np.nan, 1], [2, np.inf], [-0.5, 0]], np.float32)
    pix = np.concatenate([np.stack([px, py], 1), out_px]).astype(np.float32)
    col_all = np.concatenate([col, np.full((len(out_px), 3), 0.77, np.float32)])
    dep_all = np.concatenate([dep, np.full(len(out_px), 9.0, np.float32)])
    tcol, tpix, tdep = (torch.from_numpy(a).to(DEV) for a in (col_all, pix, dep_all))
    # what torch scatters today (driver.render_image), from the rays inside
    ref = torch.zeros((h, w, 3), dtype=torch.float32, device=DEV)
    ref[torch.from_numpy(py).long().to(DEV), torch.from_numpy(px).long().to(DEV)] = tcol[:n]
    refd = torch.zeros((h, w), dtype=torch.float32, device=DEV)
    refd[torch.from_numpy(py).long().to(DEV), torch.from_numpy(px).long().to(DEV)] = tdep[:n]
    # one frame of a clip of five, sentinel everywhere
    clip8 = torch.full((5, h, w, 3), 0x5A, dtype=torch.uint8, device=DEV)
    clipf = torch.full((5, h, w, 3), 12345.0, dtype=torch.float32, device=DEV)
    clipd = torch.full((5, h, w), 12345.0, dtype=torch.float32, device=DEV)
    _store(tcol, tpix, tdep, h, w, clip8[2], clipf[2], clipd[2])
    assert torch.equal(clipf[2].view(torch.int32), ref.view(torch.int32))        # bit patterns: -0.0 and NaN included
    assert torch.equal(clipd[2], refd)
    assert torch.equal(clip8[2], _metrics_bytes(ref))
    assert np.array_equal(clip8[2].cpu().numpy(), R.quantise(ref.cpu().numpy()))
    miss = torch.from_numpy(~cast).to(DEV)
    assert int(miss.sum()) > 50 and not bool(clip8[2][miss].any()) and not bool(clipf[2][miss].any()) and not bool(clipd[2][miss].any())
    for k in (0, 1, 3, 4):
        assert bool((clip8[k] == 0x5A).all()) and bool((clipf[k] == 12345.0).all()) and bool((clipd[k] == 12345.0).all()), k
    # any subset of the outputs; a second store into the same frame clears what the first left
    only8 = torch.full((h, w, 3), 0x5A, dtype=torch.uint8, device=DEV)
    _store(tcol, tpix, None, h, w, img8=only8)
    assert torch.equal(only8, clip8[2])
    _store(tcol[:5], tpix[:5], tdep[:5], h, w, clip8[2], None, clipd[2])
    assert int((clipd[2] != 0).sum()) == 5 and int((clip8[2] != 0).any(dim=-1).sum()) <= 5
    # 1 x 1
    one8, onef = torch.full((3, 3), 0x5A, dtype=torch.uint8, device=DEV), torch.full((3, 3), 12345.0, device=DEV)
    c1 = torch.tensor([[0.5, 2.0, -1.0], [0.9, 0.9, 0.9]], device=DEV)
    _store(c1, torch.tensor([[0.0, 0.0], [1.0, 0.0]], device=DEV), None, 1, 1, one8[1], onef[1])
    assert one8[1].tolist() == [127, 255, 0] and torch.equal(onef[1], c1[0])
    assert bool((one8[[0, 2]] == 0x5A).all()) and bool((onef[[0, 2]] == 12345.0).all())


# ---------------------------------------------------------------------------------------------------------------- render_path
def _scene():
    """The scannet_small twin (cloud, weights, renderer) with a train bank of 40 frames around it -- its four reference views first -- and a test
    bank of three cameras (the twin's own, one of the synthetic ones, the twin's moved forward); built once."""
    if "scene" not in _CACHE:
        from hybridneuralrendering_amd import scenes
        from hybridneuralrendering_amd.frames import FrameBank
        from tests.test_render_gpu import _setup
        d, ti, opt, cloud, rnd = _setup("scannet_small")
        rng = np.random.default_rng(12)
        c2w = [M for M in d["c2w_nearest"]]
        imgs = [im for im in d["images_nearest"]]
        fwd = d["c2w"][:3, 2].astype(np.float64)
        for k in range(36):
            base = d["c2w_nearest"][k % 4].astype(np.float64)
            eye = base[:3, 3] + rng.uniform(-0.15, 0.15, size=3)
            target = eye + 2.0 * base[:3, 2] + rng.uniform(-0.2, 0.2, size=3)
            c2w.append(scenes.look_at(eye, target, up=-base[:3, 1]))
            imgs.append(np.clip(d["images_nearest"][k % 4] + rng.normal(0, 0.05, size=d["images_nearest"][0].shape), 0, 1).astype(np.float32))
        tr = FrameBank(np.stack(imgs).astype(np.float32), np.stack(c2w).astype(np.float32), d["intrinsic"], DEV)
        mid = d["c2w"].copy()
        mid[:3, 3] += (0.05 * fwd).astype(np.float32)
        te = FrameBank(np.zeros((3,) + d["images_nearest"].shape[1:], np.float32), np.stack([d["c2w"].reshape(4, 4), c2w[5], mid.reshape(4, 4)]).astype(np.float32),
                       d["intrinsic"], DEV)
        _CACHE["scene"] = (d, ti, cloud, rnd, tr, te)
    return _CACHE["scene"]


def _q(img):
    return torch.from_numpy(R.quantise(img.cpu().numpy())).to(img.device)


def test_render_path_equals_render_image_frame_by_frame(tmp_path):
    from hybridneuralrendering_amd import driver, paths
    from hybridneuralrendering_amd.frames import BatchSampler, PathSampler
    d, ti, cloud, rnd, tr, te = _scene()
    near, far = (float(x) for x in d["near_far"])
    kw = dict(margin=3, near=near, far=far, bg_color=tuple(float(c) for c in d["bg_color"].reshape(-1)))
    s = PathSampler(te.c2w, te.intrinsic, tr, 4, **kw)
    te.set_nearest(s.views().cpu().numpy(), reference=tr)
    b = BatchSampler(te, "random", size=4, **kw)
    clip = driver.render_path(rnd, cloud, s, depth=True, keep_float=True)
    assert len(clip) == 3 and clip.frames.dtype == torch.uint8 and tuple(clip.frames.shape) == (3, 48, 64, 3) and int(s.step.item()) == 3
    for k in range(3):
        ref = driver.render_image(rnd, cloud, b.item(k), depth=True)
        assert torch.equal(clip.frames[k], _q(ref["image"])), k
        assert torch.equal(clip.images[k], ref["image"]) and torch.equal(clip.depth[k], ref["depth"]), k
        assert int(clip.ray_hits[k]) == int(ref["ray_mask"].sum()) and int(clip.ray_hits[k]) > (100 if k == 0 else 0), k
    # chunked rendering and an explicit frame list give the same bytes; depth and the float frames are optional
    sub = driver.render_path(rnd, cloud, s, frames=[2, 0], chunk_rays=257)
    assert sub.depth is None and sub.images is None and torch.equal(sub.frames[0], clip.frames[2]) and torch.equal(sub.frames[1], clip.frames[0])
    assert int(s.step.item()) == 3                                              # an explicit list leaves the counter alone
    # two in-between poses of a key-frame path: render_image on the sampler's own item
    keys = np.stack([te.c2w[0].cpu().numpy(), te.c2w[1].cpu().numpy()])
    path = paths.keyframe_path(keys, 4)
    s2 = PathSampler(path, te.intrinsic, tr, 4, **kw)
    mid = driver.render_path(rnd, cloud, s2, frames=[1, 2])
    for k, f in enumerate((1, 2)):
        ref = driver.render_image(rnd, cloud, s2.item(f))
        assert torch.equal(mid.frames[k], _q(ref["image"])) and int(mid.ray_hits[k]) == int(ref["ray_mask"].sum()) > 0, f
    assert not torch.equal(mid.frames[0], mid.frames[1])
    # the files decode to the clip
    from PIL import Image
    files = clip.write(str(tmp_path), gif=True)
    assert [os.path.basename(f) for f in files] == ["step-%04d-coarse_raycolor.png" % k for k in range(3)] + ["coarse_raycolor.gif"]
    host = clip.to_numpy()
    assert sorted(host) == ["depth", "frames", "images", "ray_hits"]
    for k in range(3):
        assert np.array_equal(np.asarray(Image.open(files[k])), host["frames"][k])
    assert Image.open(files[3]).n_frames == 3


def test_render_path_carries_an_edited_cloud():
    from hybridneuralrendering_amd import driver, edit
    from hybridneuralrendering_amd.frames import PathSampler
    from hybridneuralrendering_amd.render import PointCloud
    from tests.test_edit_gpu import _rot
    d, ti, cloud, rnd, tr, te = _scene()
    near, far = (float(x) for x in d["near_far"])
    state = {"neural_points.xyz": ti["xyz"], "neural_points.points_embeding": ti["emb"], "neural_points.points_conf": ti["conf"],
             "neural_points.points_dir": ti["pdir"], "neural_points.points_color": ti["color"]}
    n = ti["xyz"].shape[0]
    half = torch.arange(n, device=ti["xyz"].device) < n // 2
    mat = torch.eye(4)
    mat[:3, :3] = _rot([0.2, -0.4, 0.9], 0.35)
    mat[:3, 3] = torch.tensor([0.02, -0.03, 0.01])
    c = edit.compose([edit.load_part(state, inds=half), edit.load_part(state, inds=~half, transform=mat)])
    edited = PointCloud(c["neural_points.xyz"], c["neural_points.points_embeding"], c["neural_points.points_conf"], c["neural_points.points_dir"],
                        c["neural_points.points_color"], Rw2c=(c["part"], c["part_rot"]))
    assert edited.parts is not None and edited.parts.n_parts == 2
    s = PathSampler(te.c2w, te.intrinsic, tr, 4, margin=3, near=near, far=far)
    clip = driver.render_path(rnd, edited, s, frames=[0])
    ref = driver.render_image(rnd, edited, s.item(0))
    assert torch.equal(clip.frames[0], _q(ref["image"])) and int(clip.ray_hits[0]) == int(ref["ray_mask"].sum()) > 100
    plain = driver.render_path(rnd, cloud, s, frames=[0])
    assert not torch.equal(plain.frames[0], clip.frames[0])                     # the edit shows


# ---------------------------------------------------------------------------------------------------------------- what is refused
def test_bad_arguments_raise():
    from hybridneuralrendering_amd import _lib, driver
    from hybridneuralrendering_amd.frames import PathSampler, HnrError
    tr, te = _pair((19, 25), 4)
    s = PathSampler(te.c2w, te.intrinsic, tr, 4, margin=2, near=0.1, far=8.0)
    dev = torch.device(DEV)
    with pytest.raises(HnrError, match="gt_image"):
        s.next(out=dict(gt_image=torch.zeros((s.R, 3), device=dev)))             # a free camera has no ground truth
    with pytest.raises(HnrError, match="raydir"):
        s.next(out=dict(raydir=torch.zeros((s.R - 1, 3), device=dev)))
    with pytest.raises(HnrError):
        s.next(out=dict(raydir=torch.zeros((s.R, 3))))                           # a host tensor
    assert int(s.step.item()) == 0                                              # nothing ran
    with pytest.raises(HnrError):
        s.item(5)
    with pytest.raises(HnrError, match="poses"):
        s.set_poses(te.c2w[:4])
    with pytest.raises(HnrError, match="device"):
        s.set_poses(te.c2w.cpu())
    with pytest.raises(HnrError, match="device"):
        s.views(te.c2w.cpu())
    with pytest.raises(HnrError):
        driver.render_path(None, None, s, frames=[5])
    with pytest.raises(HnrError):
        driver.render_path(None, None, s, frames=[])
    # the C entry points: a negative status and a message, never an abort, nothing launched
    L = _lib.lib()
    p = _lib.ptr
    bank = ctypes.byref(tr._c)
    views = torch.full((5, 4), -7, dtype=torch.int32, device=dev)
    assert L.hnr_pose_views(None, None, 0, None, 0, None, 0, 0, None, None) == -1 and b"hnr_pose_views" in L.hnr_last_error()
    for V, n1 in ((0, 4), (65, 70), (4, 3), (4, tr.F + 1)):
        assert L.hnr_pose_views(bank, p(s.poses), 5, p(s.intrinsic), 0, None, V, n1, p(views), None) == -1
    ex = torch.zeros((5,), dtype=torch.int32, device=dev)
    assert L.hnr_pose_views(bank, p(s.poses), 5, p(s.intrinsic), 0, p(ex), 4, 4, p(views), None) == -1          # n1 == V leaves no room for an exclusion
    assert L.hnr_pose_views(bank, p(s.poses), 0, p(s.intrinsic), 0, None, 4, 4, p(views), None) == -1
    assert bool((views == -7).all())
    o = _lib.FrameBatchOut()
    bg = (ctypes.c_float * 3)(1, 1, 1)
    gt = torch.full((s.R, 3), 5.0, device=dev)
    item = lambda o, scratch_bytes=512, i=0, step=None, margin=2: L.hnr_path_item(bank, p(s.poses), 5, p(s.intrinsic), 0, 4, 4, step, i, margin, 0, bg, 0,
                                                                                  ctypes.byref(o), p(s._scratch), scratch_bytes, None)
    assert item(o) == 0
    assert item(o, scratch_bytes=16) == -1 and b"scratch" in L.hnr_last_error()
    assert item(o, i=5) == -1 and item(o, i=-1) == -1 and item(o, margin=10) == -1
    o.d_gt_image = gt.data_ptr()
    assert item(o) == -1 and b"gt_image" in L.hnr_last_error()
    o = _lib.FrameBatchOut()
    o.d_frame_weight = gt.data_ptr()
    assert item(o) == -1
    assert bool((gt == 5.0).all())
    col = torch.zeros((4, 3), device=dev)
    pix = torch.zeros((4, 2), device=dev)
    img = torch.full((2, 2, 3), 9.0, device=dev)
    dimg = torch.full((2, 2), 9.0, device=dev)
    st = L.hnr_frame_store
    assert st(p(col), p(pix), None, 4, 2, 2, None, None, None, None) == -1 and b"hnr_frame_store" in L.hnr_last_error()      # no output
    assert st(p(col), p(pix), None, 4, 0, 2, None, p(img), None, None) == -1
    assert st(None, p(pix), None, 4, 2, 2, None, p(img), None, None) == -1
    assert st(p(col), None, None, 4, 2, 2, None, p(img), None, None) == -1
    assert st(p(col), p(pix), None, 4, 2, 2, None, None, p(dimg), None) == -1                                                # a depth image without depths
    assert st(p(col), p(pix), None, -1, 2, 2, None, p(img), None, None) == -1
    torch.cuda.synchronize()
    assert bool((img == 9.0).all()) and bool((dimg == 9.0).all())
