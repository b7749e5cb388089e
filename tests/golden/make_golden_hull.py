"""Generates tests/golden/hull.npz by running the REFERENCE's own visual-hull masking and occlusion-aware embedding on small synthetic scenes, on the
CPU.  Needs the reference checkout (tests/golden/_ref_import.py); the fixture holds data only.

Reference code that runs (none is copied):
  models/mvs/mvs_utils.py         alpha_masking, homo_warp_nongrid_occ, extract_from_2d_grid (its stray .cuda() neutralised)
  models/mvs/mvs_points_model.py  MvsPointsModel.query_embedding / extract_2d with a stand-in `self` and depth_occ = 1, called as run/train_ft.py:176-180
  models/mvs/models.py            FeatureNet(intermediate=True) with the AbnStandIn of make_golden_mvs_init.py, weights of tests/golden/mvs_init.npz
  run/train_ft.py                 `masking` and the statements of lines 143-190 of gen_points_filter_embeddings (spacemin crop, alpha_masking + masking,
                                  regrouping by view, query_embedding per view), compiled from the reference's file at generation time (ast), as
                                  make_golden_cloud_init.reference_nearest_view does: the module itself starts a pycuda context on import.
Stand-ins, stated here because nothing on this side can pin them:
  * torch_scatter is absent from this image.  scatter_min(src [B,n], index [B,n], dim=1) returns the per-index minimum (torch's scatter_reduce
    "amin"), which is the operator's documented definition; the argmin it also returns is not used by homo_warp_nongrid_occ, and None is handed back.
  * For the fp64 runs only, `.to(torch.float32)` of an fp64 tensor is the identity (make_golden_mvs_init.py), so the chain stays fp64.
  * `torch.as_tensor(..., device="cuda")` inside the train_ft.py statements loses its device argument.
The reference's fp32 intermediates (pixel quotients, camera depths) are not returned by its functions: they are RECORDED while the functions run, by a
proxy in place of the module's `torch` name whose floor / ceil note their argument, by Tensor.__ge__ (the near_far comparison) and by the scatter_min
stand-in (the masked camera depths).

Scenes (40 x 56 frames: not square, so a swapped H / W shows):
  h_*  M = 5 alpha views around a ball of radius 0.55 (view 3 has its own intrinsic), alpha values 0.0 / 0.05 outside and 0.15 / 1.0 inside the
       silhouette, view 2 with a lit left and top border (clamped lookups pass there: the records h_mask_v2_* are view 2 alone, M = 1); about 5 000
       candidate points: inside the ball, in a cube around it (outside every silhouette), in a large cube (outside some frames:
       clamped lookups; behind cameras; beyond near_far).  Four records: range mask off / on x near_far None / given.
  o_*  one view, points on three surfaces -- a front one at depth 2, one 0.05 behind it (inside the tolerance of 0.1) on the left, one 0.3 behind it
       (outside) on the right -- several points per cell, some outside the frame, some at negative depth; query_embedding(depth_occ=1) in fp64 and fp32.
  s_*  the staged start of a scene: three depth views of the ball -> the filter (tests/geo_filter_ref.py in fp32: the restatement the GPU filter is
       bit-equal to, tests/test_geo_filter_gpu.py) with the dataset's spacemin / spacemax -> the reference's train_ft.py:143-190 with the h_ alphas,
       vox_res = 0 (the voxel pick has its own fixture and its own boundary conditions, tests/golden/cloud_init.npz), depth_occ = 1.

Boundary conditions ENFORCED here (asserted before the file is written), so that the reference alone decides every mask and no comparison leaves
anything out.  Offending points are dropped (s_: their points_mask pixel is cleared) and everything is re-run until this holds:
  * no projected coordinate that can matter (inside the frame widened by 2 px) lies within `margin_px` of an integer; no quotient is non-finite;
  * no cam z lies within `margin_z` of near - 1, of far or of zmin + 0.1;
  * no ceil'd coordinate of the occlusion test lies within `margin_px_occ` of changing cell (the frame borders 0, W-1 and H-1 are integers too).
Each margin is 4 x the largest distance between an fp32 value -- the reference's recorded one, and the fp32 restatement's -- and the fp64 restatement
(tests/hull_ref.py), measured on these scenes over the coordinates that can matter.  tol_xyz (the s_ points) is 4 x the distance of the fp32 world points from the fp64 ones: the fp32 inverse of w2c differs by a few ulp from one CPU to the
next, so the s_ points are compared within it, and the s_ margins are widened by what such a shift can move a coordinate.  The embedding tolerances tol_emb / tol_color / tol_dir are 4 x the
largest difference between the reference's own fp32 and fp64 runs of the o_ scene (+ half an ulp: the fp64 results are stored rounded to fp32);
margins and tolerances are stored in the fixture.  The s_ record is the reference's fp32 run: the same tolerances apply to it, as both sides are then
fp32 evaluations of the same networks on images of the same kind, each within a quarter of the tolerance of the exact value.

Run:  python tests/golden/make_golden_hull.py
"""
import ast
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

M, H, W = 5, 40, 56
RADIUS = 0.55
NEAR_FAR = (2.0, 3.4)
TOL = 0.1
FEATURE_STR = ["imgfeat_0_0123", "dir_0", "point_conf"]
REC = [("off_none", False, False), ("on_none", True, False), ("off_nf", False, True), ("on_nf", True, True)]


class TorchProxy:
    """Stands for the name `torch` in a reference module: floor and ceil note their argument, as_tensor loses device=."""

    def __init__(self):
        self.floor_args, self.ceil_args = [], []

    def __getattr__(self, name):
        return getattr(torch, name)

    def floor(self, x):
        self.floor_args.append(x.detach().clone())
        return torch.floor(x)

    def ceil(self, x):
        self.ceil_args.append(x.detach().clone())
        return torch.ceil(x)

    def as_tensor(self, *a, **k):
        k.pop("device", None)
        return torch.as_tensor(*a, **k)


class Recorder:
    """While active: Tensor.__ge__ notes floating tensors compared with a Python number (cam z against near - 1)."""

    def __init__(self):
        self.ge_args = []

    def __enter__(self):
        self.orig = torch.Tensor.__ge__
        rec, orig = self.ge_args, self.orig

        def ge(t, other):
            if t.is_floating_point() and isinstance(other, (int, float, np.floating)):
                rec.append(t.detach().clone())
            return orig(t, other)
        torch.Tensor.__ge__ = ge
        return self

    def __exit__(self, *a):
        torch.Tensor.__ge__ = self.orig


class ScatterMin:
    """The stand-in of torch_scatter.scatter_min for homo_warp_nongrid_occ: the per-index minimum; notes its inputs."""

    def __init__(self):
        self.calls = []

    def __call__(self, src, index, dim=1):
        assert dim == 1 and src.dim() == 2 and src.shape == index.shape
        self.calls.append((src.detach().clone(), index.detach().clone()))
        out = torch.full((src.shape[0], int(index.max()) + 1), float("inf"), dtype=src.dtype)
        return out.scatter_reduce(1, index, src, "amin", include_self=True), None


def train_ft_statements(first, last):
    """(`masking`, the statements of gen_points_filter_embeddings with first <= line <= last) from the reference's run/train_ft.py"""
    import _ref_import
    path = os.path.join(_ref_import.REF, "run", "train_ft.py")
    tree = ast.parse(open(path).read(), path)
    fns = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
    ns = {"torch": torch}
    exec(compile(ast.Module(body=[fns["masking"]], type_ignores=[]), path, "exec"), ns)
    body = fns["gen_points_filter_embeddings"].body
    inner = [w for w in body if isinstance(w, ast.With)]
    assert len(inner) == 1
    stmts = [s for s in inner[0].body if first <= s.lineno <= last]
    assert stmts and stmts[0].lineno == first and stmts[-1].end_lineno == last, (stmts[0].lineno, stmts[-1].end_lineno)
    return ns["masking"], compile(ast.Module(body=stmts, type_ignores=[]), path, "exec")


def alpha_scene(look_at):
    K = np.tile(np.array([[45.0, 0.0, 27.5], [0.0, 45.0, 19.5], [0.0, 0.0, 1.0]], np.float32), (M, 1, 1))
    K[3] = np.array([[48.0, 0.0, 26.0], [0.0, 46.5, 21.0], [0.0, 0.0, 1.0]], np.float32)
    pos = [[3.0 * np.cos(a), 3.0 * np.sin(a), h] for a, h in zip(np.linspace(0.3, 0.3 + 2 * np.pi, M, endpoint=False), (0.4, -0.6, 1.0, 0.1, -0.9))]
    c2w = np.stack([look_at(p, [0.0, 0.0, 0.0]) for p in pos]).astype(np.float32)
    w2c = np.stack([torch.inverse(torch.from_numpy(m)).numpy() for m in c2w])
    alphas = np.zeros((M, H, W), np.float32)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    for m in range(M):
        d = np.stack([xx + 0.5, yy + 0.5, np.ones_like(xx)], -1) @ np.linalg.inv(K[m].astype(np.float64)).T @ c2w[m, :3, :3].astype(np.float64).T
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        o = c2w[m, :3, 3].astype(np.float64)
        b = d @ o
        hit = b * b - (o @ o - RADIUS ** 2) > 0
        par = (xx + yy).astype(np.int64)
        alphas[m] = np.where(hit, np.where(par % 3 == 0, 0.15, 1.0), np.where(par % 2 == 0, 0.05, 0.0))
    alphas[2][:, :4], alphas[2][:5, 4:] = 1.0, 0.15             # view 2: a lit left and top border, so that clamped lookups of its own can pass
    return alphas, K, c2w, w2c


def hull_points(rng):
    ball = rng.standard_normal((2600, 3))
    ball *= (0.62 * rng.uniform(size=(2600, 1)) ** (1 / 3)) / np.linalg.norm(ball, axis=1, keepdims=True)
    return np.concatenate([ball, rng.uniform(-1.5, 1.5, size=(1500, 3)), rng.uniform(-4.5, 4.5, size=(900, 3))]).astype(np.float32)


def int_dist(a):
    return np.abs(a - np.round(a))


def main():
    import hull_ref as R
    import geo_filter_ref as GR
    import make_golden_cloud_init as G
    from make_golden_mvs_init import AbnStandIn
    mu, _, pm = G.import_reference_modules()
    models = importlib.import_module("models.mvs.models")
    torch.Tensor.cuda = lambda self, *a, **k: self             # extract_from_2d_grid's stray .cuda(), and those of train_ft.py
    proxy, smin = TorchProxy(), ScatterMin()
    mu.torch, mu.scatter_min = proxy, smin
    rng = np.random.default_rng(11)
    alphas, K, c2w, w2c = alpha_scene(G.look_at)
    on = R.alpha_on(alphas)
    alpha_list = [a[None] for a in alphas]
    out = dict(h_alphas=alphas, h_K=K, h_c2w=c2w, h_w2c=w2c, near_far=np.array(NEAR_FAR, np.float64), tolerate=np.float32(TOL))

    def ref_hull(xyz, range_on, nf, views=tuple(range(M))):
        """the reference's mask + its recorded fp32 quotients [M,n,2] (and cam z [M,n] with near_far)"""
        opt = types.SimpleNamespace(alpha_range=1 if range_on else 0, inall_img=1)
        del proxy.floor_args[:]
        pick = lambda a: [a[v] for v in views]
        with Recorder() as rec:
            m = mu.alpha_masking(torch.from_numpy(xyz), pick(alpha_list), pick(K), pick(c2w), pick(w2c), NEAR_FAR if nf else None, opt=opt)
        q = np.stack([a.numpy() for a in proxy.floor_args])
        assert q.shape == (len(views), xyz.shape[0], 2) and (not nf or len(rec.ge_args) == len(views))
        return m.numpy(), q, (np.stack([a.numpy() for a in rec.ge_args]) if nf else None)

    # ---- h_: the candidate points, until no coordinate that matters is near a boundary
    xyz = hull_points(rng)
    lo_nf, hi_nf = NEAR_FAR[0] - 1.0, NEAR_FAR[1]
    for it in range(20):
        _, q_ref, z_ref = ref_hull(xyz, True, True)
        z64, q64, q32, z32 = [], [], [], []
        for m in range(M):
            a, b = R.hull_project(xyz, w2c[m], K[m], np.float64); z64.append(a); q64.append(b)
            a, b = R.hull_project(xyz, w2c[m], K[m], np.float32); z32.append(a); q32.append(b)
        z64, q64, q32, z32 = np.stack(z64), np.stack(q64), np.stack(q32).astype(np.float64), np.stack(z32).astype(np.float64)
        lim = np.array([W, H], np.float64)
        with np.errstate(invalid="ignore"):
            finite = np.isfinite(q64).all(-1) & np.isfinite(q_ref).all(-1) & np.isfinite(q32).all(-1)
            window = (q64 > -2) & (q64 < lim + 2)
            err_px = max(float(np.abs(q_ref - q64)[window & finite[..., None]].max()), float(np.abs(q32 - q64)[window & finite[..., None]].max()))
            err_z = max(float(np.abs(z_ref - z64).max()), float(np.abs(z32 - z64).max()))
            margin_px, margin_z = 4 * err_px, 4 * err_z
            near_int = window & ((int_dist(q64) < margin_px) | (int_dist(q_ref.astype(np.float64)) < margin_px) | (int_dist(q32) < margin_px))
            stray = ~window & (((q_ref > -1) & (q_ref < lim + 1)) | ((q32 > -1) & (q32 < lim + 1)))      # outside the window in fp64, inside the frame in fp32: never
            near_z = (np.abs(z64 - lo_nf) < margin_z) | (np.abs(z64 - hi_nf) < margin_z)
        bad = (~finite | near_int.any(-1) | stray.any(-1) | near_z).any(axis=0)
        print("hull pass %d: margin_px %.3e margin_z %.3e; %d of %d points offend" % (it, margin_px, margin_z, int(bad.sum()), xyz.shape[0]))
        if not bad.any():
            break
        xyz = xyz[~bad]
    assert not bad.any(), "the hull scene did not settle"
    out.update(h_xyz=xyz, margin_px=np.float64(margin_px), margin_z=np.float64(margin_z))
    masks = {}
    for tag, range_on, nf in REC:
        m, _, _ = ref_hull(xyz, range_on, nf)
        for dt in (np.float32, np.float64):
            assert np.array_equal(m, R.visual_hull(xyz, on, w2c, K, NEAR_FAR if nf else None, range_on, dt)), (tag, dt)
        masks[tag] = m
        out["h_mask_" + tag] = m.astype(np.uint8)
        m1, _, _ = ref_hull(xyz, range_on, nf, views=(2,))                                  # M = 1: view 2 alone, where clamped lookups decide
        for dt in (np.float32, np.float64):
            assert np.array_equal(m1, R.visual_hull(xyz, on[2:3], w2c[2:3], K[2:3], NEAR_FAR if nf else None, range_on, dt)), (tag, dt)
        masks["v2_" + tag] = m1
        out["h_mask_v2_" + tag] = m1.astype(np.uint8)
        print("record %-8s: %d of %d points survive, %d with view 2 alone" % (tag, int(m.sum()), xyz.shape[0], int(m1.sum())))
    # what the scene must contain
    inside_any = np.zeros((xyz.shape[0],), bool); outside_some = np.zeros_like(inside_any); behind = np.zeros_like(inside_any)
    for m in range(M):
        z, q = R.hull_project(xyz, w2c[m], K[m], np.float64)
        fl = np.floor(q)
        inf = (fl[:, 0] >= 0) & (fl[:, 0] < W) & (fl[:, 1] >= 0) & (fl[:, 1] < H)
        outside_some |= ~inf; behind |= z < 0
        if m == 2:
            outside_v2 = ~inf
        inside_any |= inf & on[m][np.clip(fl[:, 1], 0, H - 1).astype(int), np.clip(fl[:, 0], 0, W - 1).astype(int)]
    assert (~inside_any).sum() > 100 and outside_some.sum() > 300 and behind.sum() > 100
    assert masks["on_none"].sum() > masks["off_none"].sum() > masks["off_nf"].sum() > 500 and masks["on_none"].sum() > masks["on_nf"].sum()
    clamped = masks["v2_off_none"] & outside_v2                          # survivors of view 2 whose lookup was clamped, on the left and above the frame
    assert clamped.sum() > 50 and (~masks["v2_off_none"] & outside_v2).sum() > 50 and (masks["v2_on_none"] & ~masks["v2_off_none"]).any()
    assert set(np.unique(alphas)) == {np.float32(0.0), np.float32(0.05), np.float32(0.15), np.float32(1.0)}

    # ---- o_: the occlusion view
    g = torch.Generator().manual_seed(5)
    Ko, c2wo = K[0].astype(np.float64), c2w[0].astype(np.float64)

    def surface(depth, gx, gy):
        z = depth + 0.004 * rng.standard_normal(gx.shape[0])
        return np.stack([(gx - Ko[0, 2]) / Ko[0, 0] * z, (gy - Ko[1, 2]) / Ko[1, 1] * z, z], -1)
    ax, ay = rng.uniform(-5.0, W + 4.0, 1000), rng.uniform(-4.0, H + 3.0, 1000)                  # the front surface
    left, right = np.flatnonzero(ax < W / 2)[:330], np.flatnonzero(ax >= W / 2)[:330]
    jit = lambda i: (ax[i] + rng.uniform(-0.3, 0.3, i.size), ay[i] + rng.uniform(-0.3, 0.3, i.size))      # behind front points: mostly in their cells
    cam_pts = np.concatenate([surface(2.0, ax, ay), surface(2.05, *jit(left)), surface(2.3, *jit(right)),
                              surface(2.05, rng.uniform(-5.0, W / 2, 80), rng.uniform(-4.0, H + 3.0, 80)),
                              surface(2.3, rng.uniform(W / 2, W + 4.0, 80), rng.uniform(-4.0, H + 3.0, 80)),
                              surface(-2.0, rng.uniform(0.0, W - 1.0, 60), rng.uniform(0.0, H - 1.0, 60))])
    oxyz = (cam_pts @ c2wo[:3, :3].T + c2wo[:3, 3]).astype(np.float32)
    oxyz = oxyz[rng.permutation(oxyz.shape[0])]
    z = np.load(os.path.join(HERE, "mvs_init.npz"))
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")}
    net = models.FeatureNet(intermediate=True, norm_act=AbnStandIn).eval()
    net.load_state_dict({k[len("FeatureNet."):]: v for k, v in sd.items() if k.startswith("FeatureNet.")})
    opt_mlp = types.SimpleNamespace(point_features_dim=32, act_type="LeakyReLU", shading_feature_mlp_layer1=2)
    premlp = pm.premlp_init(opt_mlp).eval()
    premlp.load_state_dict({k[len("premlp."):]: v for k, v in sd.items() if k.startswith("premlp.")})
    me = types.SimpleNamespace(args=types.SimpleNamespace(appr_feature_str0=FEATURE_STR, depth_occ=1, shading_feature_mlp_layer0=1, ref_vid=0, init_view_num=1),
                               premlp=premlp, FeatureNet=net)
    me.extract_2d = types.MethodType(pm.MvsPointsModel.extract_2d, me)
    orig_to = torch.Tensor.to

    def query(xyz_w, conf, image, c2w_m, w2c_m, K_m, dtype):
        """query_embedding as train_ft.py:172-180 calls it (cam_xyz = [xyz 1] @ w2c^T) in `dtype`; + the recorded grid, masked cam z and cell index"""
        net.to(dtype); premlp.to(dtype)
        tw, tc, tE, tK = (torch.from_numpy(np.asarray(a)).to(dtype) for a in (xyz_w, c2w_m, w2c_m, K_m))
        cam_xyz = (torch.cat([tw, torch.ones_like(tw[..., 0:1])], dim=-1) @ tE.t())[..., :3]
        del proxy.ceil_args[:], smin.calls[:]
        if dtype == torch.float64:
            torch.Tensor.to = lambda self, *a, **k: self if (a and a[0] is torch.float32 and self.dtype == torch.float64) else orig_to(self, *a, **k)
        try:
            with torch.no_grad():
                feats = net(torch.from_numpy(image).to(dtype)[None, None])
                emb, col, pdir, cf = pm.MvsPointsModel.query_embedding(me, [H, W], cam_xyz[None], torch.from_numpy(conf).to(dtype)[None, :, None], feats,
                                                                       tc[None, None], tE[None, None], tK[None, None], 0, pointdir_w=True)
        finally:
            torch.Tensor.to = orig_to
        grid = proxy.ceil_args[0][0].numpy()
        zsrc, idx = smin.calls[0]
        return emb[0].numpy(), col[0].numpy(), pdir[0].numpy(), cf[0].numpy(), grid, zsrc[0].numpy(), idx[0].numpy()

    def occ_check(xyz_w, w2c_m, K_m, grid_ref, zsrc_ref, extra_px=0.0, extra_z=0.0):
        """(bad [n], margin_px_occ, margin_z_occ, visible of the fp64 restatement) of one view's points; extra_*: added to the margins"""
        vis64, ins64, cell64, z64, zmin64 = R.occlusion(xyz_w, w2c_m, K_m, H, W, TOL, np.float64, details=True)
        _, g64x, g64y = R.view_project(xyz_w, w2c_m, K_m, np.float64)
        c32, g32x, g32y = R.view_project(xyz_w, w2c_m, K_m, np.float32)
        g64, g32 = np.stack([g64x, g64y], -1), np.stack([g32x, g32y], -1).astype(np.float64)
        lim = np.array([W, H], np.float64)
        with np.errstate(invalid="ignore"):
            finite = np.isfinite(g64).all(-1) & np.isfinite(grid_ref).all(-1)
            window = (g64 > -2) & (g64 < lim + 1)
            sel = window & finite[..., None]
            err_px = max(float(np.abs(grid_ref - g64)[sel].max()), float(np.abs(g32 - g64)[sel].max()))
            stray = ~window & (((grid_ref > -1) & (grid_ref < lim)) | ((g32 > -1) & (g32 < lim)))
            mpx = 4 * err_px + extra_px
            near_int = window & ((int_dist(g64) < mpx) | (int_dist(grid_ref.astype(np.float64)) < mpx) | (int_dist(g32) < mpx))
        assert zsrc_ref.shape[0] == int(ins64.sum()), "the reference and the fp64 restatement disagree about the frame"
        err_z = max(float(np.abs(zsrc_ref.astype(np.float64) - z64[ins64]).max()), float(np.abs(c32[:, 2].astype(np.float64) - z64)[ins64].max()))
        near_z = ins64 & (np.abs(z64 - (zmin64 + np.float64(np.float32(TOL)))) < 4 * err_z + extra_z)
        return ~finite | near_int.any(-1) | stray.any(-1) | near_z, 4 * err_px, 4 * err_z, vis64

    def settle_frame(xyz_w, w2c_m, K_m):
        """drops the points whose frame mask is not settled, so that the reference and the restatement see the same in-frame set"""
        for _ in range(10):
            _, g64x, g64y = R.view_project(xyz_w, w2c_m, K_m, np.float64)
            with np.errstate(invalid="ignore"):
                edge = ~np.isfinite(g64x) | ~np.isfinite(g64y) | (int_dist(g64x) < 1e-3) | (int_dist(g64y) < 1e-3)
            if not edge.any():
                return xyz_w
            xyz_w = xyz_w[~edge]
        raise AssertionError("frame mask did not settle")

    image = torch.rand((3, H, W), generator=g, dtype=torch.float64).numpy().astype(np.float32)
    oxyz = settle_frame(oxyz, w2c[0], K[0])
    for it in range(20):
        oconf = rng.uniform(0.3, 1.0, oxyz.shape[0]).astype(np.float32)
        e32 = query(oxyz, oconf, image, c2w[0], w2c[0], K[0], torch.float32)
        bad, margin_px_occ, margin_z_occ, vis64 = occ_check(oxyz, w2c[0], K[0], e32[4], e32[5])
        print("occlusion pass %d: margin_px_occ %.3e margin_z_occ %.3e; %d of %d points offend" % (it, margin_px_occ, margin_z_occ, int(bad.sum()), oxyz.shape[0]))
        if not bad.any():
            break
        oxyz = oxyz[~bad]
    assert not bad.any(), "the occlusion scene did not settle"
    e64 = query(oxyz, oconf, image, c2w[0], w2c[0], K[0], torch.float64)
    # the reference's mask: homo_warp_nongrid_occ itself, on the same camera-space points
    cam32 = (torch.cat([torch.from_numpy(oxyz), torch.ones(oxyz.shape[0], 1)], dim=-1) @ torch.from_numpy(w2c[0]).t())[..., :3]
    _, mask_ref, _ = mu.homo_warp_nongrid_occ(torch.from_numpy(c2w[0])[None], None, torch.from_numpy(K[0])[None], cam32[None], H, W, tolerate=0.1)
    vis_ref = mask_ref[0, :, 0].numpy()
    vis32, ins32, cell32, z32o, _ = R.occlusion(oxyz, w2c[0], K[0], H, W, TOL, np.float32, details=True)
    assert np.array_equal(vis_ref, vis32 != 0) and np.array_equal(vis_ref, vis64 != 0)
    assert ((e32[1] != 0).any(-1) <= vis_ref).all() and ((e64[1] != 0).any(-1) <= vis_ref).all()       # colour only where visible
    counts = np.bincount(cell32[ins32], minlength=H * W)
    hidden = ins32 & ~vis_ref
    assert counts.max() >= 3 and (~ins32).sum() > 100 and (z32o[ins32] < 0).sum() > 20 and hidden.sum() > 150 and vis_ref.sum() > 600
    mid, back = np.abs(z32o - 2.05) < 0.03, np.abs(z32o - 2.3) < 0.03
    assert (mid & vis_ref).sum() > 150 and (back & hidden).sum() > 100 and (mid & hidden).sum() < 40, "the tolerance must decide: 0.05 behind is visible, 0.3 behind is hidden"
    # the fp64 truth is stored rounded to fp32 (size): half an ulp of the largest value joins each tolerance
    tol = [4 * float(np.abs(e32[i].astype(np.float64) - e64[i]).max()) + float(np.abs(e64[i]).max()) * 2.0 ** -24 for i in range(3)]
    print("occlusion: %d points, %d in frame, %d visible, %d hidden; tol emb %.2e color %.2e dir %.2e" % (oxyz.shape[0], int(ins32.sum()), int(vis_ref.sum()),
                                                                                                        int(hidden.sum()), *tol))
    out.update(o_xyz=oxyz, o_conf=oconf, o_image=image, o_visible=vis_ref.astype(np.uint8), o_emb=e64[0].astype(np.float32), o_color=e64[1].astype(np.float32), o_dir=e64[2].astype(np.float32),
               margin_px_occ=np.float64(margin_px_occ), margin_z_occ=np.float64(margin_z_occ), tol_emb=np.float64(tol[0]), tol_color=np.float64(tol[1]),
               tol_dir=np.float64(tol[2]))

    # ---- s_: the staged start of a scene
    V = 3
    # depth cameras of their own, between the alpha cameras: a point of a camera's own pixel grid projects ONTO integers in that camera
    sK = K[:V].copy(); sK[:, 0, 2] += 0.37; sK[:, 1, 2] -= 0.41
    sc2w = np.stack([G.look_at([3.0 * np.cos(a), 3.0 * np.sin(a), h], [0.0, 0.0, 0.0]) for a, h in zip((0.9, 1.25, 1.6), (0.2, -0.3, 0.5))]).astype(np.float32)
    sE = np.stack([torch.inverse(torch.from_numpy(m)).numpy() for m in sc2w])
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    depth = np.zeros((V, H, W), np.float32)
    for v in range(V):
        d = np.stack([xx, yy, np.ones_like(xx)], -1) @ np.linalg.inv(sK[v].astype(np.float64)).T          # camera rays with z = 1
        o = sc2w[v, :3, 3].astype(np.float64) - np.array([0.08, 0.0, 0.05])                              # a ball off the centre: a part of it sticks out of the hull
        dw = d @ sc2w[v, :3, :3].astype(np.float64).T
        a, b, c = (dw * dw).sum(-1), dw @ o, o @ o - (RADIUS * 0.97) ** 2
        disc = b * b - a * c
        t = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / a, 0.0)
        depth[v] = (t * (1.0 + 0.0005 * rng.standard_normal((H, W)))).astype(np.float32)
    simages = torch.rand((V, 3, H, W), generator=g, dtype=torch.float64).numpy().astype(np.float32)
    sconf = rng.uniform(0.75, 1.0, size=(V, H, W)).astype(np.float32)
    fy, fx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    cam_xyz = np.stack([((torch.inverse(torch.from_numpy(sK[v])) @ (torch.stack([fx.reshape(-1), fy.reshape(-1), torch.ones(H * W, dtype=torch.long)], 0) *
                                                                     torch.from_numpy(depth[v]).reshape(-1))).t().reshape(H, W, 3)).numpy() for v in range(V)])
    spacemin, spacemax = np.array([-0.7, -0.7, -0.45], np.float32), np.array([0.7, 0.7, 0.7], np.float32)
    sopt = types.SimpleNamespace(depth_conf_thresh=0.7, geo_cnsst_num=1, ranges=[-100.0] * 6, default_conf=-1.0, vox_res=0, alpha_range=0, inall_img=1, depth_occ=1,
                                 manual_depth_view=1, far_plane_shift=None)
    Kinv, Einv = GR.inverses(sK, sE)
    count, avg = GR.geo_consistency(depth, sK, Kinv, sE, Einv)
    masking, stmts = train_ft_statements(143, 190)
    pmask = depth > 0

    class Model:
        def query_embedding(self, HDWD, cam, conf, imgs, c2ws, w2cs, intrinsics, cam_vid, pointdir_w=True):
            del proxy.ceil_args[:], smin.calls[:]
            res = pm.MvsPointsModel.query_embedding(me, HDWD, cam, conf, net(imgs[:, :1]), c2ws, w2cs, intrinsics, cam_vid, pointdir_w=pointdir_w)
            self.recorded.append((proxy.ceil_args[0][0].numpy(), smin.calls[0][0][0].numpy()))
            return res
    net.float(); premlp.float()
    for it in range(30):
        flt = GR.select(cam_xyz, sconf, pmask, count, avg, Einv, sopt.depth_conf_thresh, sopt.geo_cnsst_num, np.concatenate([spacemin, spacemax]))
        pix = np.argwhere(flt["keep"])                                   # (v, y, x) of every filtered point, in the filter's order
        dataset = types.SimpleNamespace(spacemin=torch.from_numpy(spacemin), spacemax=torch.from_numpy(spacemax), alphas=alpha_list, intrinsics=list(K),
                                        cam2worlds=list(c2w), world2cams=list(w2c), near_far=NEAR_FAR, view_id_list=list(range(V)))
        model = Model(); model.recorded = []
        ns = dict(torch=proxy, np=np, tqdm=lambda x, *a, **k: x, masking=masking, mvs_utils=mu, dataset=dataset, opt=sopt, model=model, print=lambda *a, **k: None,
                  getattr=getattr, xyz_world_all=torch.from_numpy(flt["world"]), points_vid=torch.from_numpy(flt["view"].astype(np.float32))[:, None],
                  confidence_filtered_all=torch.from_numpy(flt["conf"]), HDWD_lst=[(H, W)] * V, extrinsics_all=[torch.from_numpy(sE[v])[None] for v in range(V)],
                  imgs_lst=[torch.from_numpy(simages[v])[None, None] for v in range(V)], c2ws_lst=[torch.from_numpy(sc2w[v])[None, None] for v in range(V)],
                  w2cs_lst=[torch.from_numpy(sE[v])[None, None] for v in range(V)], intrinsics_full_lst=[torch.from_numpy(sK[v])[None, None] for v in range(V)],
                  len=len, range=range)
        del proxy.floor_args[:]
        with torch.no_grad():
            exec(stmts, ns)
        n_before = flt["world"].shape[0]
        # the world points depend on the fp32 inverse of w2c, which LAPACK forms a few ulp differently from one CPU to the next: tol_xyz is 4 x the
        # distance of the fp32 points from the fp64 ones (fp64 inverse; the averaged depth taken as given, as make_golden_geo_filter.py does), and the
        # margins of the staged points are widened by what such a shift moves a pixel coordinate (shift_px) or a depth (3 tol_xyz)
        Einv64 = np.linalg.inv(sE.astype(np.float64))
        world64 = np.concatenate([flt["cam"][flt["view"] == v].astype(np.float64) @ Einv64[v][:3, :3].T + Einv64[v][:3, 3] for v in range(V)])
        tol_xyz = 4 * float(np.abs(flt["world"].astype(np.float64) - world64).max())
        zmin_all = min(float(np.abs(R.hull_project(flt["world"], w2c[m], K[m], np.float64)[0]).min()) for m in range(M))
        zmin_all = min([zmin_all] + [float(np.abs(R.view_project(flt["world"], sE[v], sK[v], np.float64)[0][:, 2]).min()) for v in range(V)])
        # g = f X / Z + c:  |dg| <= f / |Z| (|dX| + |X / Z| |dZ|), |dX|, |dZ| <= sqrt(3) tol_xyz (rotation rows have unit length), |X / Z| <= (W / 2 + 4) / f
        fmax, fmin = float(max(K[:, :2, :2].max(), sK[:, :2, :2].max())), float(min(K[:, 0, 0].min(), K[:, 1, 1].min(), sK[:, 0, 0].min(), sK[:, 1, 1].min()))
        shift_px = np.sqrt(3.0) * tol_xyz * fmax / zmin_all * (1.0 + (max(W, H) / 2 + 4) / fmin)
        margin_px_s = margin_px + shift_px
        # boundary conditions of the hull stage on the filtered points, and of the occlusion stage on each view's survivors
        q_ref = np.stack([a.numpy() for a in proxy.floor_args])
        bad = np.zeros((n_before,), bool)
        lim = np.array([W, H], np.float64)
        for m in range(M):
            _, q64 = R.hull_project(flt["world"], w2c[m], K[m], np.float64)
            _, q32 = R.hull_project(flt["world"], w2c[m], K[m], np.float32)
            for q in (q64, q_ref[m].astype(np.float64), q32.astype(np.float64)):
                bad |= (~np.isfinite(q).all(-1)) | (((q > -2) & (q < lim + 2)) & (int_dist(q) < margin_px_s)).any(-1)
            assert float(np.abs(q_ref[m] - q64).max()) * 4 <= margin_px and float(np.abs(q32 - q64).max()) * 4 <= margin_px, "the staged points err more than the h_ scene's"
        keep_h = R.visual_hull(flt["world"], on, w2c, K, None, False, np.float32)
        assert np.array_equal(keep_h, R.visual_hull(flt["world"], on, w2c, K, None, False, np.float64)) or bad.any()
        sxyz, svid = ns["xyz_world_all"].numpy(), flt["view"][keep_h]
        assert bad.any() or (sxyz.shape[0] == int(keep_h.sum()) and np.array_equal(sxyz, flt["world"][keep_h])), "regrouping by ascending view keeps the filter's order"
        if not bad.any():
            surv = np.flatnonzero(keep_h)
            for v, (grid_ref, zsrc_ref) in zip(sorted(set(svid.tolist())), model.recorded):
                idx = surv[svid == v]
                b, mpx, mz, _ = occ_check(flt["world"][idx], sE[v], sK[v], grid_ref, zsrc_ref, extra_px=shift_px, extra_z=3 * tol_xyz)
                assert mpx <= 4 * margin_px_occ and mz <= 4 * margin_z_occ
                bad[idx] |= b
        print("staged pass %d: %d filtered points, %d after the alphas; %d offend" % (it, n_before, int(keep_h.sum()), int(bad.sum())))
        if not bad.any():
            break
        off = pix[bad]
        pmask[off[:, 0], off[:, 1], off[:, 2]] = False
    assert not bad.any(), "the staged scene did not settle"
    semb, scol, sdir, scf = (ns[k][0].numpy() for k in ("points_embedding_all", "points_color_all", "points_dir_all", "points_conf_all"))
    n = sxyz.shape[0]
    assert semb.shape == (n, 32) and scol.shape == (n, 3) and sdir.shape == (n, 3) and scf.shape == (n, 1) and np.array_equal(scf[:, 0], flt["conf"][keep_h])
    assert len(set(svid.tolist())) == V and 150 < n < n_before and int(flt["keep"].sum()) < int((depth > 0).sum())
    vis_all = np.concatenate([R.occlusion(sxyz[svid == v], sE[v], sK[v], H, W, TOL) for v in range(V)])
    assert ((scol != 0).any(-1) <= (vis_all != 0)).all()                 # (a depth map has one point per pixel: the o_ scene is where the tolerance decides)
    print("staged: %d points, per view %s, %d hidden or outside their own frame; tol_xyz %.3e, shift_px %.3e" % (n, np.bincount(svid, minlength=V).tolist(),
                                                                                                                 int((vis_all == 0).sum()), tol_xyz, shift_px))
    assert zmin_all > 1.0 and shift_px < margin_px
    out.update(s_cam_xyz=cam_xyz, s_conf=sconf, s_points_mask=pmask.astype(np.uint8), s_K=sK, s_w2c=sE, s_c2w=sc2w, s_images=simages, s_spacemin=spacemin,
               s_spacemax=spacemax, s_depth_conf_thresh=np.float32(sopt.depth_conf_thresh), s_geo_cnsst_num=np.int32(sopt.geo_cnsst_num), s_xyz=sxyz, s_view=svid.astype(np.int64),
               s_emb=semb, s_color=scol, s_dir=sdir, s_conf_out=scf, tol_xyz=np.float64(tol_xyz))

    path = os.path.join(HERE, "hull.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 1000000, size
    print("wrote %s (%d bytes)" % (path, size))


if __name__ == "__main__":
    main()
