"""The call blocks of a ray batch (hybridneuralrendering_amd/_raycall.py) as the routes use them, on the scannet_small fixture: the result dicts of
render_rays and TrainPath.forward hold the table's keys, shapes and dtypes, the status word is clean, the library gets a 256-byte aligned workspace,
and TrainPath.reuse_outputs hands out the same tensors every step.  No numeric value is checked here: the routes' own tests do that."""
import functools

import pytest
import torch

from hybridneuralrendering_amd._raycall import FORWARD_OUTPUTS, RAY_OUTPUTS, TRAIN_OUTPUTS
from tests.test_train_gpu import _leaves, _setup

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _world(tag):
    """(fixture, inputs, opt, aggregator, path, render cloud), built once per fixture: nothing here is modified by a test."""
    from hybridneuralrendering_amd.render import PointCloud
    d, ti, opt, agg, path = _setup(tag)
    return d, ti, opt, agg, path, PointCloud(ti["xyz"], ti["emb"], ti["conf"], ti["pdir"], ti["color"])


def _args(d, ti, R):
    near, far = d["near_far"]
    return (ti["raydir"][0][:R].contiguous(), ti["campos"][0], ti["camrotc2w"][0], ti["bg_color"][0], float(near), float(far), ti["c2w_nearest"][0],
            ti["campos_nearest"][0], ti["intrinsic_nearest"][0], ti["images_nearest"][0])


def _check(out, keys, R, opt, absent=()):
    """Every key of `keys` is in `out` with the table's shape and dtype for (R, SR, K) -- or is None when listed in `absent`."""
    dims = dict(R=R, SR=int(opt.SR), K=int(opt.K))
    table = {key: (tuple(dims.get(s, s) for s in shape), dt) for key, _field, shape, dt in RAY_OUTPUTS}
    for k in keys:
        if k in absent:
            assert out[k] is None, k
        else:
            assert (tuple(out[k].shape), out[k].dtype) == table[k] and out[k].is_cuda and out[k].is_contiguous(), (k, out[k].shape, out[k].dtype)


def _spy_workspace(monkeypatch, name, index):
    """Records the workspace pointer argument of library call `name` (argument `index`)."""
    from hybridneuralrendering_amd import _lib
    L, seen = _lib.lib(), []
    orig = getattr(L, name)
    monkeypatch.setattr(L, name, lambda *a: (seen.append(a[index]), orig(*a))[1])
    return seen


@pytest.mark.parametrize("R", [None, 65])
def test_render_rays_result_dicts_follow_the_table(R, monkeypatch):
    d, ti, opt, agg, path, cloud = _world("scannet_small")
    R = int(ti["raydir"].shape[1]) if R is None else R
    rnd = path.r
    assert rnd.single_call and rnd.dense == "f16x2"
    seen = _spy_workspace(monkeypatch, "hnr_render_forward", 6)
    plain = rnd.render_rays(cloud, *_args(d, ti, R))
    assert set(plain) == set(FORWARD_OUTPUTS) | {"blend_weight"}
    _check(plain, plain, R, opt, absent=("blend_weight",))
    full = rnd.render_rays(cloud, *_args(d, ti, R), want_weights=True)
    assert tuple(full) == TRAIN_OUTPUTS
    _check(full, full, R, opt)
    depth = rnd.render_rays(cloud, *_args(d, ti, R), want_depth=True)
    assert set(depth) == set(FORWARD_OUTPUTS) | {"blend_weight", "coarse_depth"}
    _check(depth, set(depth) - {"coarse_depth"}, R, opt, absent=("blend_weight",))
    assert tuple(depth["coarse_depth"].shape) == (R,) and depth["coarse_depth"].dtype == torch.float32
    both = rnd.render_rays(cloud, *_args(d, ti, R), want_weights=True, want_depth=True)
    assert tuple(both) == TRAIN_OUTPUTS + ("coarse_depth",)
    torch.cuda.synchronize()
    for o in (plain, full, depth, both):
        assert int(o["status"][0]) == 0
    assert len(seen) == 4 and all(p.value and p.value % 256 == 0 for p in seen)


@pytest.mark.parametrize("R", [None, 65])
@pytest.mark.parametrize("tag", ["scannet_small", "scannet_small_nearest0"])
def test_train_forward_result_dict_follows_the_table(tag, R, monkeypatch):
    """A 2-D [R, D] tmid (the fixture's jittered table); scannet_small_nearest0: the same batch with use_nearest = 0."""
    d, ti, opt, agg, path, cloud = _world(tag)
    assert (getattr(opt, "use_nearest", 4) == 0) == tag.endswith("nearest0")
    R = int(ti["raydir"].shape[1]) if R is None else R
    tmid = torch.from_numpy(d["tmid"]).to(ti["raydir"].device)[:R].contiguous()
    assert tmid.dim() == 2 and tmid.shape[0] == R
    seen = _spy_workspace(monkeypatch, "hnr_render_train_forward", 8)
    out, S = path.forward(cloud, *_args(d, ti, R), tmid=tmid)
    assert tuple(out) == TRAIN_OUTPUTS
    _check(out, out, R, opt)
    out_d, S_d = path.forward(cloud, *_args(d, ti, R), tmid=tmid, want_depth=True)
    assert tuple(out_d) == TRAIN_OUTPUTS + ("coarse_depth",) and tuple(out_d["coarse_depth"].shape) == (R,) and out_d["coarse_depth"].dtype == torch.float32
    torch.cuda.synchronize()
    assert int(out["status"][0]) == 0 and int(out_d["status"][0]) == 0
    assert len(seen) == 2 and seen[0].value == S.ws_ptr.value and seen[1].value == S_d.ws_ptr.value
    for s in (S, S_d):
        assert s.ws_ptr.value % 256 == 0 and s.ws.data_ptr() <= s.ws_ptr.value and s.ws_ptr.value + s.nbytes <= s.ws.data_ptr() + s.ws.numel()
        assert (s.R, s.SR, s.K, s.dev, s.prm.tmid_stride) == (R, int(opt.SR), 8, tmid.device, tmid.shape[1]) and s.flat is None
    assert out["coarse_raycolor"].data_ptr() != out_d["coarse_raycolor"].data_ptr()          # reuse_outputs is off: fresh tensors


@pytest.mark.parametrize("reuse", [True, False])
def test_reuse_outputs_hands_out_the_same_tensors_every_step(reuse):
    from hybridneuralrendering_amd.train import TrainPath, train_step
    d, ti, opt, agg, path0, cloud = _world("scannet_small")
    path = TrainPath(path0.r)                             # a path of its own: the switch and its caches stay out of the shared one
    path.reuse_outputs = reuse
    R = 65
    tmid = torch.from_numpy(d["tmid"]).to(ti["raydir"].device)[:R].contiguous()
    gt = torch.from_numpy(d["gt"][0]).to(ti["raydir"].device)[:R].contiguous()
    emb, conf, pdir, color = _leaves(ti)
    steps = [train_step(path, agg, ti["xyz"], emb, conf, pdir, color, *_args(d, ti, R), gt, zero_epsilon=float(d["zero_epsilon"]), tmid=tmid,
                        assign_grads=False) for _ in range(2)]
    torch.cuda.synchronize()
    (o1, pg1, ag1), (o2, pg2, ag2) = steps                # both steps' results are alive: the allocator cannot hand an address out twice
    assert int(o1["status"][0]) == 0 and int(o2["status"][0]) == 0
    assert tuple(k for k in o1 if k in TRAIN_OUTPUTS) == TRAIN_OUTPUTS and sorted(pg1) == sorted(pg2) and sorted(ag1) == sorted(ag2)
    pairs = [(o1[k], o2[k]) for k in TRAIN_OUTPUTS] + [(pg1[k], pg2[k]) for k in pg1] + [(ag1[k], ag2[k]) for k in ag1]
    pairs += [(o1["_saved"].flat, o2["_saved"].flat), (o1["_saved"].ws, o2["_saved"].ws)]
    same = [a.data_ptr() == b.data_ptr() for a, b in pairs]
    assert all(same) if reuse else not any(same)
    assert o1["_saved"].flat_payload == o2["_saved"].flat_payload > 0
