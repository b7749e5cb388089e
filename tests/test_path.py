"""Camera paths on the host: the NumPy restatement of the view selection (tests/path_ref.py) against the reference's recorded picks and the host
selection frames.nearest_by_pose, paths.spherical_path against poses recorded from the reference (tests/golden/paths.npz), paths.keyframe_path's
properties, and the arguments PathSampler refuses before it touches a device."""
import os

import numpy as np
import pytest
import torch

from tests import path_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gold(name):
    return dict(np.load(os.path.join(ROOT, "tests", "golden", name)))


def test_restatement_equals_the_reference_ring_picks():
    g = _gold("frames.npz")
    W, H = (int(x) for x in g["ring_wh"])
    T, V = g["ring_c2w"].shape[0], g["ring_picks_test"].shape[1]
    n1 = min(3 * V, T // 10)
    assert np.array_equal(R.bank_dirs(g["ring_c2w"], g["ring_K"], W, H), g["ring_dirs"])
    assert np.array_equal(R.pose_views(g["ring_c2w"], g["ring_K"], g["ring_test_c2w"], g["ring_K"], W, H, V, n1), g["ring_picks_test"])
    q = g["ring_query_train"]
    got = R.pose_views(g["ring_c2w"], g["ring_K"], g["ring_c2w"][q], g["ring_K"], W, H, V, n1, exclude_rows=q)
    assert np.array_equal(got, g["ring_picks_train"])
    for row, picks in zip(q, got):
        assert row not in picks
    # without the exclude rows a train camera picks itself first
    assert np.array_equal(R.pose_views(g["ring_c2w"], g["ring_K"], g["ring_c2w"][q], g["ring_K"], W, H, V, n1)[:, 0], q)


def _gaps(tr, K, qs, V, n1, W, H):
    """per query: the smaller of the fp64 gaps at the two cuts (score n1-1 | n1, distance V-1 | V among the step-1 rows)"""
    d64 = lambda M: (lambda v: v / (np.linalg.norm(v) + 1e-5))(
        M[:3, :3].astype(np.float64) @ np.array([((W // 2) + 0.5 - K[0, 2]) / K[0, 0], ((H // 2) + 0.5 - K[1, 2]) / K[1, 1], 1.0]))
    dirs = np.stack([d64(M) for M in tr])
    out = []
    for M in qs:
        s = np.sort(-(dirs @ d64(M)))
        rows = np.argsort(-(dirs @ d64(M)), kind="stable")[:n1]
        e = np.sort(np.linalg.norm(tr[rows, :3, 3].astype(np.float64) - M[:3, 3].astype(np.float64), axis=1))
        out.append(min(s[n1] - s[n1 - 1], e[V] - e[V - 1] if n1 > V else np.inf))
    return np.asarray(out)


@pytest.mark.parametrize("T,V,Q,seed", [(40, 4, 7, 1), (64, 1, 1, 2), (257, 4, 65, 4), (257, 1, 7, 6)])
def test_restatement_equals_nearest_by_pose(T, V, Q, seed):
    from hybridneuralrendering_amd import frames
    W, H = 64, 48
    c2w, K = R.lookat_cameras(T + Q, seed, W, H)
    tr, qs = c2w[:T], c2w[T:]
    n1 = min(3 * V, T // 10)
    dirs = np.stack([frames.center_raydir(K, M, W, H)[0] for M in tr])
    host = frames.nearest_by_pose(qs, K, np.full(Q, -1), tr[:, :3, 3], dirs, np.arange(T), V, W, H, False)
    mine = R.pose_views(tr, K, qs, K, W, H, V, n1)
    gaps = _gaps(tr, K, qs, V, n1, W, H)
    keep = gaps >= 1e-5
    print("T %d V %d Q %d: smallest gap %.3g, %d of %d queries left out" % (T, V, Q, float(gaps.min()), int((~keep).sum()), Q))
    assert (~keep).sum() <= 0.05 * Q
    assert np.array_equal(mine[keep], host[keep])


def test_stable_order_decides_ties_and_nan():
    v = np.array([0.5, np.nan, 0.5, -0.0, 0.0, 1.0, np.nan], dtype=np.float32)
    assert R.stable_order(v).tolist() == [3, 4, 0, 2, 5, 1, 6]
    assert R.stable_order(v, descending=True).tolist() == [5, 0, 2, 3, 4, 1, 6]


def test_quantise_is_the_metrics_rule():
    from tests import metrics_ref
    x = np.array([-0.0, 0.0, -1.5, 1.5, np.inf, -np.inf, np.nan, 1.0, 0.999999, 0.5] + [k / 255 for k in range(256)], dtype=np.float32)
    q = R.quantise(x)
    assert q[:10].tolist() == [0, 0, 0, 255, 255, 0, 0, 255, 254, 127]
    fin = np.isfinite(x)
    assert np.array_equal(q[fin], (np.clip(x[fin], 0, 1) * np.float32(255)).astype(np.uint8))
    assert np.array_equal(q[fin], metrics_ref.quantise(x[fin]))                  # the rule tests/metrics_ref.py holds hnr_frame_metrics to


def test_spherical_path_equals_the_reference_render_poses():
    """The recorded poses are the reference's float32 / float64 mixed products; spherical_path rounds the same float32 factors and multiplies in
    float64.  Bound: two float32 4x4 products of entries <= max(radius, 1), three terms each -> 8 * 2^-24 * max(radius, 1) absolute."""
    from hybridneuralrendering_amd import paths
    g = _gold("paths.npz")
    p = paths.spherical_path()
    assert p.dtype == np.float32 and p.shape == (20, 4, 4)
    assert np.abs(p.astype(np.float64) - g["render_poses"]).max() <= 8 * 2.0 ** -24 * 4
    for n, el, rad in g["cases"]:
        got = paths.spherical_path(int(n), el, rad)
        want = g["poses_%d_%g_%g" % (int(n), el, rad)]
        assert got.shape == want.shape
        assert np.abs(got.astype(np.float64) - want).max() <= 8 * 2.0 ** -24 * max(rad, 1.0), (n, el, rad)
    # the closed form: on the sphere, looking at the origin, a proper rotation
    p = paths.spherical_path(9, -20.0, 3.0).astype(np.float64)
    assert np.abs(np.linalg.norm(p[:, :3, 3], axis=1) - 3.0).max() < 1e-6
    assert np.abs(np.cross(p[:, :3, 2], p[:, :3, 3])).max() < 1e-6 and (np.einsum("ni,ni->n", p[:, :3, 2], p[:, :3, 3]) < 0).all()
    assert np.abs(np.einsum("nij,nkj->nik", p[:, :3, :3], p[:, :3, :3]) - np.eye(3)).max() < 1e-6
    assert np.abs(np.linalg.det(p[:, :3, :3]) - 1).max() < 1e-6
    assert np.allclose(p[:, 3], [0, 0, 0, 1])


def test_keyframe_path_properties():
    from hybridneuralrendering_amd import paths
    from hybridneuralrendering_amd._lib import HnrError
    keys, _K = R.lookat_cameras(4, 11)
    p = paths.keyframe_path(keys, 10)
    assert p.dtype == np.float32 and p.shape == (10, 4, 4)
    for s, f in enumerate((0, 3, 6, 9)):
        assert np.array_equal(p[f], keys[s]), (s, f)                             # every key exactly, at its own frame
    rot = p[:, :3, :3].astype(np.float64)
    assert np.abs(np.einsum("nij,nkj->nik", rot, rot) - np.eye(3)).max() < 1e-6
    assert np.abs(np.linalg.det(rot) - 1).max() < 1e-6 and np.allclose(p[:, 3], [0, 0, 0, 1])
    # between two keys the rotation stays on the arc between them: no further from either than they are from each other
    ang = lambda A, B: np.arccos(np.clip((np.trace(A.T @ B) - 1) / 2, -1, 1))
    for f in (1, 2):
        assert ang(rot[f], rot[0]) <= ang(rot[0], rot[3]) + 1e-6 and ang(rot[f], rot[3]) <= ang(rot[0], rot[3]) + 1e-6
    # positions move (no frame repeats) and stay near the keys' hull
    assert (np.linalg.norm(np.diff(p[:, :3, 3], axis=0), axis=1) > 0).all()
    assert np.abs(p[:, :3, 3]).max() <= np.abs(keys[:, :3, 3]).max() * 1.5
    const = paths.keyframe_path(np.stack([keys[0]] * 3), 7)
    assert all(np.array_equal(f, keys[0]) for f in const)                        # identical keys: a constant path
    closed = paths.keyframe_path(keys, 13, closed=True)
    assert closed.shape == (13, 4, 4) and np.array_equal(closed[0], keys[0]) and np.array_equal(closed[-1], keys[0])
    for s, f in enumerate((0, 3, 6, 9)):
        assert np.array_equal(closed[f], keys[s])
    for bad in (dict(c2w_keys=keys[:1], n_frames=5), dict(c2w_keys=keys, n_frames=3), dict(c2w_keys=keys[:, :3], n_frames=9),
                dict(c2w_keys=keys, n_frames=4, closed=True)):
        with pytest.raises(HnrError):
            paths.keyframe_path(**bad)
    with pytest.raises(HnrError):
        paths.spherical_path(0)


def _stand_in_bank(T, H=48, W=64):
    """a FrameBank object without a device behind it: what PathSampler looks at before it uploads anything"""
    from hybridneuralrendering_amd.frames import FrameBank
    b = object.__new__(FrameBank)
    b.F, b.H, b.W, b.device = T, H, W, torch.device("cuda:0")
    return b


def test_path_sampler_refuses_bad_arguments_before_touching_the_device():
    from hybridneuralrendering_amd.frames import PathSampler, HnrError
    poses, K = R.lookat_cameras(5, 3)
    kw = dict(near=0.1, far=8.0)
    bank = _stand_in_bank(60)
    with pytest.raises(HnrError, match="n1"):
        PathSampler(poses, K, _stand_in_bank(39), 4, **kw)                       # floor(39 / 10) = 3 candidates for 4 views
    with pytest.raises(HnrError, match="n1"):
        PathSampler(poses, K, bank, 4, num_times=0, **kw)
    for V in (0, 65):
        with pytest.raises(HnrError, match="V"):
            PathSampler(poses, K, _stand_in_bank(1000), V, **kw)
    with pytest.raises(HnrError, match="8192"):
        PathSampler(poses, K, _stand_in_bank(8193), 4, **kw)
    with pytest.raises(HnrError, match="poses"):
        PathSampler(poses[:, :3], K, bank, 4, **kw)
    with pytest.raises(HnrError, match="poses"):
        PathSampler(poses[0], K, bank, 4, **kw)
    with pytest.raises(HnrError, match="finite"):
        PathSampler(np.where(np.arange(80).reshape(5, 4, 4) == 7, np.nan, poses), K, bank, 4, **kw)
    with pytest.raises(HnrError, match="intrinsic"):
        PathSampler(poses, np.stack([K] * 4), bank, 4, **kw)
    with pytest.raises(HnrError, match="intrinsic"):
        PathSampler(poses, K[:2], bank, 4, **kw)
    with pytest.raises(HnrError, match="device"):
        PathSampler(torch.from_numpy(poses), K, bank, 4, **kw)                   # a host tensor: arrays are uploaded, tensors must be resident
    with pytest.raises(HnrError, match="device"):
        PathSampler(poses, torch.from_numpy(K), bank, 4, **kw)
    with pytest.raises(HnrError, match="bg_color"):
        PathSampler(poses, K, bank, 4, bg_color="random", **kw)
    with pytest.raises(HnrError, match="bg_color"):
        PathSampler(poses, K, bank, 4, bg_color=(1, 1), **kw)
    with pytest.raises(HnrError, match="near"):
        PathSampler(poses, K, bank, 4)
    with pytest.raises(HnrError, match="empty range"):
        PathSampler(poses, K, bank, 4, margin=24, **kw)
    with pytest.raises(HnrError, match="FrameBank"):
        PathSampler(poses, K, None, 4, **kw)


def test_render_path_refuses_what_it_does_not_cover():
    from hybridneuralrendering_amd import driver
    from hybridneuralrendering_amd._lib import HnrError
    with pytest.raises(HnrError, match="PathSampler"):
        driver.render_path(None, None, object())
