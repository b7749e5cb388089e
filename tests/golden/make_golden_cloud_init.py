"""Generates tests/golden/cloud_init.npz by running the REFERENCE's own code for the `load_points=2` cloud initialisation (run/train_ft.py:687-770)
on small synthetic inputs.  Needs the reference checkout (tests/golden/_ref_import.py); the fixture holds data only.

Reference functions called (none is copied):
  data/scannet_ft_dataset.py  ScannetFtDataset.load_init_depth_points / read_depth with a stand-in `self` (cv2.imread and the pose files are served
                              from the synthetic frames), which calls mvs_utils.construct_vox_points_xyz
  models/mvs/mvs_utils.py     construct_vox_points_closest, homo_warp_nongrid, extract_from_2d_grid (its stray .cuda() neutralised)
  run/train_ft.py             nearest_view
  models/mvs/mvs_points_model.py  MvsPointsModel.query_embedding / extract_2d with a stand-in `self` (imgfeat + dir + point_conf branches)
torch_scatter is absent from this image: scatter_mean / scatter_min get the stand-ins of make_golden.py::gen_voxel (index_add in point order / first
minimum), pinned to the operators' definition by tests/test_voxel.py.

Boundary conditions ENFORCED here (asserted before the file is written), so that the reference alone decides every cell and every view and no case has
to be left out of a comparison:
  * no reference-run point or centroid lies within 1e-3 cell of a cell boundary in either voxel stage (offending depth pixels are zeroed / offending
    stage-2 points dropped, and everything is re-run until this holds);
  * every point's best and second-best view score differ by at least 1e-4 (offending points dropped);
  * no attribute point projects within 1e-3 pixel of the frame border, except the one placed exactly on gx = W-1.

Run:  python tests/golden/make_golden_cloud_init.py
"""
import ast
import importlib
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

H, W = 480, 640                     # load_init_depth_points hard-codes the frame size
RES_FRAME = (12, 100)
RES_FINAL = 24
EPS_CELL = 1e-3
EPS_SCORE = 1e-4


def _scatter_standins():
    def scatter_mean(src, index, dim=0):
        n = int(index.max()) + 1
        out = torch.zeros((n,) + src.shape[1:], dtype=src.dtype).index_add_(0, index, src)
        cnt = torch.zeros((n,), dtype=src.dtype).index_add_(0, index, torch.ones_like(index, dtype=src.dtype))
        return out / cnt[:, None]

    def scatter_min(src, index, dim=0):
        n = int(index.max()) + 1
        best = torch.full((n,), float("inf"), dtype=src.dtype)
        arg = torch.full((n,), -1, dtype=torch.long)
        for i in range(src.shape[0]):
            v = int(index[i])
            if src[i] < best[v]:
                best[v], arg[v] = src[i], i
        return best, arg
    sys.modules["torch_scatter"] = types.ModuleType("torch_scatter")
    sys.modules["torch_scatter"].__dict__.update(scatter_mean=scatter_mean, scatter_min=scatter_min, segment_coo=None)


def import_reference_modules():
    import _ref_import
    _ref_import.import_reference()
    _scatter_standins()
    for name in ("matplotlib", "matplotlib.pyplot"):
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                sys.modules[name] = types.ModuleType(name)
    ku = types.ModuleType("kornia.utils"); ku.create_meshgrid = None
    ws = types.ModuleType("warmup_scheduler"); ws.GradualWarmupScheduler = None; sys.modules["warmup_scheduler"] = ws
    sys.modules["kornia"].utils = ku; sys.modules["kornia.utils"] = ku; sys.modules["kornia"].__path__ = []
    sys.modules["kornia"].create_meshgrid = None
    sys.modules["cv2"].__dict__.setdefault("COLORMAP_JET", 2)
    tvt = sys.modules.get("torchvision.transforms")
    if tvt is not None and not hasattr(tvt, "__path__"):       # torchvision is a stand-in here: the dataset module also names .transforms.functional
        tvt.__path__ = []
        tvf = types.ModuleType("torchvision.transforms.functional"); sys.modules[tvf.__name__] = tvf; tvt.functional = tvf
    mu = importlib.import_module("models.mvs.mvs_utils")
    mu.print = lambda *a, **k: None
    ds = importlib.import_module("data.scannet_ft_dataset")
    ds.tqdm = lambda x, *a, **k: x
    pm = importlib.import_module("models.mvs.mvs_points_model")
    return mu, ds, pm


def reference_nearest_view():
    """run/train_ft.py::nearest_view.  The module itself starts a pycuda context on import, so the one function is compiled from the reference's file
    at generation time (ast), in a namespace that holds torch only."""
    import _ref_import
    path = os.path.join(_ref_import.REF, "run", "train_ft.py")
    tree = ast.parse(open(path).read(), path)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "nearest_view"]
    assert len(fn) == 1
    ns = {"torch": torch}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns["nearest_view"]


def look_at(pos, target):
    """c2w (OpenCV: +z forward, +y down) of a camera at pos looking at target."""
    pos, target = np.asarray(pos, np.float64), np.asarray(target, np.float64)
    z = target - pos; z /= np.linalg.norm(z)
    x = np.cross(np.array([0.0, 0.0, 1.0]), z); x /= np.linalg.norm(x)
    y = np.cross(z, x)
    M = np.eye(4)
    M[:3, 0], M[:3, 1], M[:3, 2], M[:3, 3] = x, y, z, pos
    return M.astype(np.float32)


def make_frames(rng):
    """Four frames: a 37x53 window + ~200 pixels scattered around it on a gently curved wall (uint16 millimetres), one frame with holes in the window,
    a few values outside [0.3 m, 8 m]; and one all-zero frame (kept out of the reference run)."""
    frames, poses = [], []
    for k in range(4):
        d = np.zeros((H, W), np.uint16)
        y0, x0 = 150 + 40 * k, 200 + 60 * k
        yy, xx = np.mgrid[0:H, 0:W]
        wall = 1500.0 + 400.0 * k + 0.9 * (xx - x0) + 0.5 * (yy - y0) + 25.0 * np.sin(xx / 7.0) * np.cos(yy / 5.0)
        d[y0:y0 + 37, x0:x0 + 53] = wall[y0:y0 + 37, x0:x0 + 53].astype(np.uint16)
        sy = rng.integers(max(0, y0 - 60), min(H, y0 + 100), size=200)
        sx = rng.integers(max(0, x0 - 80), min(W, x0 + 140), size=200)
        d[sy, sx] = wall[sy, sx].astype(np.uint16)
        if k == 1:                                             # holes inside the window
            hy, hx = rng.integers(y0, y0 + 37, size=120), rng.integers(x0, x0 + 53, size=120)
            d[hy, hx] = 0
        d[sy[:3], sx[:3]] = (9000, 250, 8001)                  # beyond depth_max / below depth_min: dropped by the range rule
        frames.append(d)
        poses.append(look_at([0.4 * k - 0.5, -2.0 + 0.1 * k, 1.2 + 0.05 * k], [0.3 * k, 1.0, 1.0]))
    frames.append(np.zeros((H, W), np.uint16))
    poses.append(look_at([0.0, -2.0, 1.0], [0.0, 1.0, 1.0]))
    return np.stack(frames), np.stack(poses)


class RefDepthRun:
    """load_init_depth_points with a stand-in `self`: frames come from memory through cv2.imread, poses from text files the reference reads itself."""

    def __init__(self, ds, K4):
        self.ds, self.K4 = ds, K4

    def __call__(self, frames, poses, ids, vox_res, ranges):
        cls = self.ds.ScannetFtDataset
        with tempfile.TemporaryDirectory() as tmp:
            os.makedirs(os.path.join(tmp, "scan", "exported", "pose"))
            table = {}
            for i in ids:
                np.savetxt(os.path.join(tmp, "scan", "exported", "pose", "%d.txt" % i), poses[i].astype(np.float64), fmt="%.9e")
                table[os.path.join(tmp, "scan", "exported/depth/%d.png" % i)] = frames[i]
            self.ds.cv2.imread = lambda path, flag=-1: table[path].copy()
            me = types.SimpleNamespace(depth_intrinsic=self.K4[:3, :3].copy(), all_id_list=list(ids), data_dir=tmp, scan="scan",
                                       opt=types.SimpleNamespace(ranges=list(ranges)))
            me.read_depth = types.MethodType(cls.read_depth, me)
            return cls.load_init_depth_points(me, device="cpu", vox_res=vox_res).numpy()


def cell_margin(pts, vox_res):
    """distance (in cells) of every coordinate to the nearest cell boundary, in the space the reference forms from these points (float64 of its fp32
    space_min / size)."""
    p = pts.astype(np.float32)
    mn, mx = p.min(0), p.max(0)
    edge = np.float32(np.max(mx - mn) * np.float32(1.05))
    smin = (mx + mn) / np.float32(2) - edge / np.float32(2)
    size = np.float32(edge / np.float32(vox_res))
    q = (p.astype(np.float64) - smin.astype(np.float64)) / float(size)
    return np.abs(q - np.round(q))


def main():
    mu, ds, pm = import_reference_modules()
    torch.Tensor.cuda = lambda self, *a, **k: self             # extract_from_2d_grid's stray .cuda()
    rng = np.random.default_rng(20)
    out = {}
    K4 = np.eye(4, dtype=np.float32)
    K4[0, 0], K4[1, 1], K4[0, 2], K4[1, 2] = 577.590698, 578.729797, 318.905426, 242.683609
    frames, poses = make_frames(rng)
    run = RefDepthRun(ds, K4)
    no_crop = [-100.0] * 6
    live = [0, 1, 2, 3]
    Ki = torch.inverse(torch.from_numpy(K4[:3, :3])).numpy()

    # ---- stage 1: zero depth pixels whose point (or whose voxel's centroid) sits within EPS_CELL of a cell boundary, at either resolution; re-run
    for it in range(50):
        changed = 0
        for i in live:
            raw = run(frames, poses, [i], 0, no_crop)                                  # the frame's kept points, pixel order
            with np.errstate(invalid="ignore"):
                d = frames[i].astype(np.float32) / np.float32(1000)
                d[(d > 8.0) | (d < 0.3)] = 0
            pix = np.flatnonzero(d.reshape(-1) > 0)                                    # kept <=> d > 0 for these cameras (asserted)
            assert len(pix) == raw.shape[0], (len(pix), raw.shape)
            bad = np.zeros((raw.shape[0],), bool)
            for res in RES_FRAME:
                bad |= (cell_margin(raw, res) < EPS_CELL).any(axis=1)
            if bad.any():
                frames[i].reshape(-1)[pix[bad]] = 0
                changed += int(bad.sum())
        if not changed:
            break
    assert not changed, "stage 1 did not settle"
    counts = []
    bp = []
    for i in live:
        raw = run(frames, poses, [i], 0, no_crop)
        for res in RES_FRAME:
            assert (cell_margin(raw, res) >= EPS_CELL).all()
        bp.append(raw); counts.append(raw.shape[0])
    out["bp_xyz"], out["bp_counts"] = np.concatenate(bp), np.array(counts, np.int64)
    for res in RES_FRAME:
        per = [run(frames, poses, [i], res, no_crop) for i in live]
        for raw, cen in zip(bp, per):                                                  # centroids, in the frame's own space
            p = raw.astype(np.float32)
            mn, mx = p.min(0), p.max(0)
            edge = np.float32(np.max(mx - mn) * np.float32(1.05))
            smin = (mx + mn) / np.float32(2) - edge / np.float32(2)
            q = (cen.astype(np.float64) - smin.astype(np.float64)) / float(np.float32(edge / np.float32(res)))
            assert (np.abs(q - np.round(q)) >= EPS_CELL).all(), "a stage-1 centroid sits on a cell boundary"
        out["fuse%d_xyz" % res] = np.concatenate(per)
        out["fuse%d_counts" % res] = np.array([p.shape[0] for p in per], np.int64)
        whole = run(frames, poses, live, res, no_crop)                                 # the reference's own loop over the frames + torch.cat
        assert np.array_equal(whole, out["fuse%d_xyz" % res])
        print("stage 1, res %d: %s kept pixels -> %s centroids" % (res, counts, out["fuse%d_counts" % res].tolist()))
    out["frames"], out["poses"], out["depth_intrinsic"], out["depth_intrinsic_inv"] = frames, poses, K4, Ki

    # ---- crop: ranges cutting off about a tenth of the fused cloud (scannet_ft_dataset.py:643-646 == train_ft.py:713-716)
    fused = out["fuse100_xyz"]
    lo, hi = fused.min(0) - 0.5, fused.max(0) + 0.5
    lo[0] = np.quantile(fused[:, 0], 0.06); hi[2] = np.quantile(fused[:, 2], 0.95)
    ranges = np.concatenate([lo, hi]).astype(np.float32)
    cropped = run(frames, poses, live, 100, [float(r) for r in ranges])
    out["ranges"], out["crop_xyz"] = ranges, cropped
    print("crop: %d -> %d points" % (fused.shape[0], cropped.shape[0]))
    assert 0.8 * fused.shape[0] < cropped.shape[0] < 0.95 * fused.shape[0]

    # ---- stage 2: construct_vox_points_closest at RES_FINAL; drop points near a cell boundary until none is left
    s2 = cropped
    for it in range(50):
        bad = (cell_margin(s2, RES_FINAL) < EPS_CELL).any(axis=1)
        if not bad.any():
            cen, grid, midx = mu.construct_vox_points_closest(torch.from_numpy(s2), RES_FINAL)
            p = s2.astype(np.float32)
            mn, mx = p.min(0), p.max(0)
            edge = np.float32(np.max(mx - mn) * np.float32(1.05))
            smin = (mx + mn) / np.float32(2) - edge / np.float32(2)
            q = (cen.numpy().astype(np.float64) - smin.astype(np.float64)) / float(np.float32(edge / np.float32(RES_FINAL)))
            assert (np.abs(q - np.round(q)) >= EPS_CELL).all(), "a stage-2 centroid sits on a cell boundary"
            break
        s2 = s2[~bad]
    assert not (cell_margin(s2, RES_FINAL) < EPS_CELL).any()
    out["s2_xyz"], out["s2_res"] = s2, np.array([RES_FINAL], np.int64)
    out["s2_centroid"], out["s2_grid"], out["s2_min_idx"] = cen.numpy(), grid.numpy(), midx.numpy()
    print("stage 2: %d points -> %d voxels" % (s2.shape[0], grid.shape[0]))

    # ---- nearest view: M = 5 and M = 70 cameras (the kernel stages 64 cameras per round: 70 crosses the chunk and the wavefront size)
    nearest_view = reference_nearest_view()
    sel = s2[midx.numpy()]
    cams = {}
    for M in (5, 70):
        pos = (rng.uniform(-1, 1, size=(M, 3)) * np.array([2.5, 1.0, 0.6]) + np.array([0.0, -2.0, 1.2])).astype(np.float32)
        tgt = rng.uniform(-1, 1, size=(M, 3)) * np.array([1.5, 0.3, 0.5]) + np.array([0.5, 1.0, 1.0])
        dirs = (tgt - pos); dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
        cams[M] = (pos, dirs)
    keep = np.ones((sel.shape[0],), bool)
    for M, (pos, dirs) in cams.items():
        d = sel[:, None, :].astype(np.float64) - pos[None].astype(np.float64)
        n = np.linalg.norm(d, axis=-1)
        score = n / 200 + (1.1 - np.sum(d / (n[..., None] + 1e-6) * dirs[None].astype(np.float64), axis=-1))
        part = np.sort(score, axis=1)
        keep &= (part[:, 1] - part[:, 0]) >= EPS_SCORE
    nv = sel[keep]
    out["nv_xyz"] = nv
    for M, (pos, dirs) in cams.items():
        ind = nearest_view(torch.from_numpy(pos), torch.from_numpy(dirs), torch.from_numpy(nv), None).numpy()
        d = nv[:, None, :].astype(np.float64) - pos[None].astype(np.float64)
        n = np.linalg.norm(d, axis=-1)
        score = n / 200 + (1.1 - np.sum(d / (n[..., None] + 1e-6) * dirs[None].astype(np.float64), axis=-1))
        part = np.sort(score, axis=1)
        assert ((part[:, 1] - part[:, 0]) >= EPS_SCORE).all() and np.array_equal(np.argmin(score, axis=1), ind[:, 0])
        out["nv_campos%d" % M], out["nv_camdir%d" % M], out["nv_ind%d" % M] = pos, dirs, ind
        print("nearest view, M = %d: %d points, %d views used" % (M, nv.shape[0], len(np.unique(ind))))

    # ---- attributes: one 48x64 view, an [8,12,16] feature map; points inside / outside the frame, behind the camera, one exactly on gx = W-1
    Hv, Wv = 48, 64
    Kv = np.array([[32.0, 0.0, 31.0], [0.0, 33.5, 23.25], [0.0, 0.0, 1.0]], np.float32)
    c2w = look_at([0.3, -1.5, 1.1], [0.4, 1.0, 0.9])
    w2c = torch.inverse(torch.from_numpy(c2w))
    image = rng.uniform(0, 1, size=(3, Hv, Wv)).astype(np.float32)
    fmap = rng.normal(size=(8, 12, 16)).astype(np.float32)
    ref_cam = lambda p: (torch.cat([p, torch.ones_like(p[..., -1:])], dim=-1) @ w2c.transpose(0, 1))[..., :3]      # run/train_ft.py:759
    n_in = 700
    cam_pts = np.concatenate([
        np.stack([rng.uniform(-0.9, 0.9, n_in), rng.uniform(-0.65, 0.65, n_in), np.ones(n_in)], -1) * rng.uniform(0.5, 4.0, size=(n_in, 1)),
        np.stack([rng.uniform(-2.5, 2.5, 200), rng.uniform(-2.0, 2.0, 200), np.ones(200)], -1) * rng.uniform(0.5, 4.0, size=(200, 1)),
        np.stack([rng.uniform(-0.9, 0.9, 100), rng.uniform(-0.65, 0.65, 100), np.ones(100)], -1) * -rng.uniform(0.5, 4.0, size=(100, 1))])
    world = (cam_pts @ c2w[:3, :3].astype(np.float64).T + c2w[:3, 3].astype(np.float64)).astype(np.float32)

    def grid_of(p):
        cam = ref_cam(torch.from_numpy(p))[None]
        g, m, _ = mu.homo_warp_nongrid(torch.from_numpy(c2w)[None], None, torch.from_numpy(Kv)[None], cam, Hv, Wv, filter=False)
        g = g[0].numpy().astype(np.float64)
        return np.stack([(g[:, 0] + 1) * (Wv - 1) / 2, (g[:, 1] + 1) * (Hv - 1) / 2], -1), m[0, :, 0].numpy()
    g, m = grid_of(world)
    with np.errstate(invalid="ignore"):
        near = (np.abs(g[:, 0]) < EPS_CELL) | (np.abs(g[:, 0] - (Wv - 1)) < EPS_CELL) | (np.abs(g[:, 1]) < EPS_CELL) | (np.abs(g[:, 1] - (Hv - 1)) < EPS_CELL)
    world = world[~near]
    # the point exactly on the right border: cam x == cam z in fp32 (K00 = 32, K01 = 0, K02 = 31: gx = 32 + 31), found by stepping world x
    # (the ONE place where the fixture looks at tests/cloud_init_ref.py, the restatement the tests check: the candidate must land on the border in the
    # reference's own fp32 arithmetic AND in the restatement's, otherwise the two would disagree about this point's mask by construction.  Only the
    # choice of this input point depends on it; every expected output stored below is computed by the reference alone.)
    sys.path.insert(0, os.path.dirname(HERE))
    import cloud_init_ref as R
    edge_pt = None
    base = (np.array([1.0, 0.2, 1.0]) * 1.7 @ c2w[:3, :3].astype(np.float64).T + c2w[:3, 3].astype(np.float64)).astype(np.float32)
    for step in range(-4000, 4000):
        cand = base.copy()
        cand[0] = base[0] + np.float32(step) * np.spacing(base[0])
        c_ref = ref_cam(torch.from_numpy(cand[None]))[0].numpy()
        c_our, gx, _ = R.project(cand[None], w2c.numpy(), Kv)
        if c_ref[0] == c_ref[2] and c_our[0, 0] == c_our[0, 2] and gx[0] == np.float32(Wv - 1):
            edge_pt = cand
            break
    assert edge_pt is not None, "no point exactly on gx = W-1 found"
    world = np.concatenate([world, edge_pt[None]]).astype(np.float32)
    g, m = grid_of(world)
    assert g[-1, 0] == Wv - 1 and bool(m[-1])
    cam_xyz = ref_cam(torch.from_numpy(world))[None]
    me = types.SimpleNamespace(args=types.SimpleNamespace(appr_feature_str0=["imgfeat_0_01", "dir_0", "point_conf"], depth_occ=0, shading_feature_mlp_layer0=0,
                                                          ref_vid=0))
    me.extract_2d = types.MethodType(pm.MvsPointsModel.extract_2d, me)
    img_feats = [torch.from_numpy(image)[None], torch.from_numpy(fmap)[None]]
    emb, col, pdir, conf = pm.MvsPointsModel.query_embedding(me, [Hv, Wv], cam_xyz, None, img_feats, torch.from_numpy(c2w)[None, None], w2c[None, None],
                                                             torch.from_numpy(Kv)[None, None], 0, pointdir_w=True)
    out["at_xyz"], out["at_image"], out["at_fmap"], out["at_c2w"], out["at_w2c"], out["at_K"] = world, image, fmap, c2w, w2c.numpy(), Kv
    out["at_feat"], out["at_color"], out["at_dir"], out["at_conf"], out["at_mask"] = emb[0].numpy(), col[0].numpy(), pdir[0].numpy(), conf[0].numpy(), m.astype(np.uint8)
    print("attributes: %d points, %d inside the frame, %d behind the camera" % (world.shape[0], int(m.sum()), int((cam_xyz[0, :, 2] < 0).sum())))
    path = os.path.join(HERE, "cloud_init.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 1000000, size
    print("wrote %s (%d bytes)" % (path, size))


if __name__ == "__main__":
    main()
