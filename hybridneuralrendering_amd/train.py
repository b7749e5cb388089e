"""Training step of the path: TWO library calls per step (hnr_render_train_forward / hnr_render_train_backward, csrc/render_train.hip),
wrapped in one torch.autograd.Function so the reference's shell (losses, optimisers, schedulers) works unchanged.

Counterpart of NeuralPointsRayMarching.forward in train mode (/root/reference/models/neural_points_volumetric_model.py:257-427:
jittered depths models/neural_points/query_point_indices_worldcoords.py:87, patch drop
models/aggregators/point_aggregators.py:1222-1237, straight-through conf clamp :1422-1424) and of what torch autograd derives from it
(models/mvs_points_volumetric_model.py:111-131).  Gradients are produced for points_embeding / points_conf / points_dir / points_color
and every aggregator parameter that takes part in the order-2 hybrid path (`color_branch` is constructed but unused, :542-553, and gets
none).  Differentiable outputs: coarse_raycolor and conf_coefficient (the two the shipped loss terms read,
dev_scripts/w_scannet_etf/scene241.sh:146-151) and, when asked for, coarse_depth (the compute_depth branch, :381-385, for a depth loss item,
models/base_rendering_model.py:1209-1215); every other output is returned detached.

Nothing here reads a device value: the library sizes every stage from device counters inside a workspace of `cap_samples` valid shading
samples (default R * SR, always enough); `TrainPath.check_status` reads the overflow word when the caller wants to (a host sync).
All arithmetic runs in libhnr_hip.so; torch supplies device memory and the stream.
"""
import ctypes

import numpy as np
import torch

from . import _lib, _raycall
from ._lib import HnrError
from . import querier as Q
from .render import _f32, PointCloud, ray_depth


def drop_patch_rays(patch_size, patch_num, drop_ratio):
    """point_aggregators.py:14-23 -- rows (of the patch_num*patch_size square batch) whose image feature is dropped."""
    flag = np.zeros((patch_size * patch_num, patch_size * patch_num), dtype=bool)
    n = int(patch_num * patch_num * drop_ratio)
    row, col = n // patch_num, n % patch_num
    flag[0:row * patch_size, :] = True
    flag[row * patch_size:row * patch_size + patch_size, 0:col * patch_size] = True
    return np.where(flag.flatten())[0]


def _drop_mode(opt):
    """None: no image-feature drop; "patch": the deterministic patch pattern; "random": an exact-size random subset of the valid rays."""
    if not (getattr(opt, "is_train", 0) and getattr(opt, "drop_ratio", 0) > 0 and getattr(opt, "random_position", 0) == 1):
        return None
    if not getattr(opt, "ray_points", 0) or getattr(opt, "drop_disturb_range", 0) != 0:
        raise HnrError("only ray-based image-feature drop with drop_disturb_range=0 is implemented (all 19 shipped scripts)")
    return "patch" if getattr(opt, "drop_patch", 0) else "random"


def drop_lut(opt, R, device):
    """[R] uint8 indexed by VALID-ray row: the reference applies `drop_ray_flag[ray_drop_positions, :]` to the R' compacted rays (:1225-1233),
    so the library looks the pattern up by the number of valid rays before a ray (hnr_render_train_forward's d_drop_lut)."""
    ps, pn = int(opt.dilation_setup.split("_")[1]), int(opt.dilation_setup.split("_")[0])
    pos = drop_patch_rays(ps, pn, opt.drop_ratio)
    lut = np.zeros((R,), dtype=np.uint8)
    lut[pos[pos < R]] = 1
    return torch.from_numpy(lut).to(device)


def ray_drop_flags(opt, ray_mask):
    """[R] uint8: rays whose merged image feature is zeroed at train time, from a ray mask (host-side form of what the library does with
    d_drop_lut; also the random mode's flag builder).  The reference indexes the drop pattern by VALID-ray row."""
    mode = _drop_mode(opt)
    if mode is None:
        return None
    R = ray_mask.shape[0]
    m = ray_mask > 0
    if mode == "random":
        # `random.sample(range(R'), int(R' * drop_ratio))` over the valid-ray rows (:1231-1232; Python's RNG there, torch's here):
        # an exact-size uniform subset, chosen on the device without reading R' back
        keys = torch.rand(R, device=ray_mask.device).masked_fill(~m, 2.0)
        rank = torch.empty(R, dtype=torch.long, device=ray_mask.device)
        rank[torch.argsort(keys)] = torch.arange(R, device=ray_mask.device)
        n_drop = (m.sum() * float(opt.drop_ratio)).to(torch.long)           # int() truncation, like the reference
        return (m & (rank < n_drop)).to(torch.uint8).contiguous()
    lut = drop_lut(opt, R, ray_mask.device).to(torch.bool)
    row = torch.cumsum(m.to(torch.int32), 0) - 1                      # valid-ray row of every ray
    return (m & lut[row.clamp(min=0).long()]).to(torch.uint8).contiguous()


# parameter name -> (field of hnr_train_weights, index or None), from the struct's table
_SLOTS = {n: (f, i) for f, names in _lib.TRAIN_WEIGHTS for i, n in ([(None, names)] if isinstance(names, str) else enumerate(names))}


def _fill_weights(tensors):
    """hnr_train_weights from {parameter name: contiguous fp32 GPU tensor}."""
    w = _lib.TrainWeights()
    for name, (fld, idx) in _SLOTS.items():
        t = tensors.get(name)
        p = ctypes.c_void_p(t.data_ptr()) if t is not None else None
        if idx is None:
            setattr(w, fld, p)
        else:
            getattr(w, fld)[idx] = p
    return w


class _Saved:
    """One forward's state, as `out["_saved"]` of train_step and the second result of TrainPath.forward."""
    __slots__ = (
        "flat",             # all weight gradients of the step as ONE fp32 buffer (set by backward): one all-reduce when the batch is sharded over ranks
        "flat_payload",     # number of floats of `flat` that hold gradients (a spare tail follows)
        "prm",              # the step's hnr_train_params
        "ws",               # the workspace tensor (uint8) with the kept activations; touched_points returns views into it
        "ws_ptr",           # its 256-byte aligned void* as the library got it
        "nbytes",           # hnr_render_train_workspace_bytes(prm)
        "dev",              # the batch's device
        "R", "SR", "K",     # rays, samples per ray, neighbours per sample
        # what the backward passes on, and references that keep the memory behind the blocks' pointers alive until then
        "V", "no_views", "wt", "weights", "cloud_t", "cl", "inp", "tmid", "cam", "vw", "out", "outs", "keep")

    def __init__(self, **fields):
        self.flat = self.flat_payload = None
        for k, v in fields.items():
            setattr(self, k, v)


def _no_rotation(who, Rw2c, xyz):
    """The training kernels (forward with kept activations, backward) carry no per-point rotations: an edited scene is rendered, not trained.
    A non-identity Rw2c raises instead of training against an un-rotated picture."""
    from .render import PartTable
    if Rw2c is not None and PartTable.make(Rw2c, int(xyz.reshape(-1, 3).shape[0]), xyz.device) is not None:
        raise HnrError("%s: Rw2c (per-point rotations of an edited scene) is not supported by the training path; render edited scenes with "
                       "HybridRenderer.render_rays / driver.render_image" % who)


class TrainPath:
    """Forward (activations kept in the library's workspace) and backward of one ray batch.  `renderer` is a HybridRenderer (grid cache)."""

    def __init__(self, renderer):
        self.r = renderer
        self.agg = renderer.agg
        self.opt = renderer.opt
        self.cap_samples = None            # valid-sample capacity of the workspace (None: R * SR, the worst case)
        self.timers = None                 # a dict: the library records HIP events at its stage boundaries (profiling; read them after a synchronise)
        self.workspace = None              # tools: a caller-owned uint8 tensor every forward uses instead of a fresh torch.empty (one step in flight at a time)
        self._lut = {}
        self._wcache = {}
        self._ocache = {}
        # reuse_outputs: every step writes its outputs and gradients into the SAME tensors (allocated once per batch shape) -- what a training loop wants
        # (the optimiser has consumed a step's gradients before the next step runs) and ~0.15 ms less Python between the launches of a step; off by default
        # because a caller that keeps two steps' results alive would see the first overwritten
        self.reuse_outputs = False

    # ---------------------------------------------------------------------------------------------- forward
    def forward(self, cloud, raydir, campos, camrot, bg_color, near, far, c2w_nearest, campos_nearest, intrinsic_nearest,
                images_nearest, frame_weight=None, tmid=None, ray_drop=None, w2c_nearest=None, want_depth=False):
        """w2c_nearest [V,4,4]: inverse(c2w_nearest) computed by the caller (torch.inverse may synchronise the host: a captured step passes it in).
        want_depth: the outputs also hold coarse_depth [R] (render.ray_depth over the padded query outputs and the blend weights; 0 where
        ray_mask = 0) -- one launch after the forward call; the backward takes its gradient (backward(g_depth=...))."""
        L, p = _lib.lib(), _lib.ptr
        r, opt = self.r, self.opt
        inp = _raycall.ray_inputs(raydir, campos, camrot, bg_color, c2w_nearest, campos_nearest, intrinsic_nearest, images_nearest, w2c_nearest,
                                  frame_weight, "frame_weight_nearest", invert=getattr(opt, "use_nearest", 4) != 0)
        raydir, campos, img, fw = inp.raydir, inp.campos, inp.images, inp.frame_w
        dev = raydir.device
        if getattr(cloud, "parts", None) is not None:
            raise HnrError("TrainPath: the cloud carries Rw2c (per-point rotations of an edited scene), which the training path does not support")
        if int(opt.K) != 8 or cloud.F != 32:
            raise HnrError("the training path is built for K = 8 neighbours and 32 point features (got K=%d, F=%d)" % (opt.K, cloud.F))
        R, SR, K = raydir.shape[0], int(opt.SR), 8
        if R == 0:
            raise HnrError("render_train: empty ray batch")
        grid, hp = r.querier._grid_for(cloud.xyz[None])
        if tmid is None:
            tmid = r.querier._tmid_for(float(near), float(far), opt.z_depth_dim, R, dev)
        tmid = _lib.require_gpu(tmid, "tmid", torch.float32)
        no_views = getattr(opt, "use_nearest", 4) == 0        # scene241.sh: image branch off, merged = 0 (point_aggregators.py:1257-1258)
        V, H, W = (0, 0, 0) if no_views else (int(img.shape[0]), int(img.shape[1]), int(img.shape[2]))
        prm = _raycall.fill_params_opt(_lib.TrainParams(), opt, R, K, tmid, hp[0] ** 2, V, self.cap_samples, 0)
        prm.H, prm.W, prm.n_points, prm.slope = H, W, int(cloud.xyz.shape[0]), float(self.agg.block1[1].negative_slope)
        nbytes = _raycall.train_workspace_bytes(prm)
        avail = _raycall.available_bytes(dev, capturing=torch.cuda.is_current_stream_capturing())
        if nbytes > 0.9 * avail:
            raise HnrError("render_train: the workspace for %d rays x SR %d (%.1f GB) does not fit the %.1f GB that are free; set TrainPath.cap_samples to the "
                           "number of valid shading samples a batch can produce" % (R, SR, nbytes / 1e9, avail / 1e9))
        ws, ws_ptr = _raycall.workspace(nbytes, dev, reuse=self.workspace)
        if self.reuse_outputs and self.workspace is None:
            self.workspace = ws                                  # (one step in flight at a time: the same workspace every step)
        # parameters as contiguous fp32 tensors under the reference's names (views of the nn.Parameters); the tensors and the ctypes block are kept
        # while the parameters stay where they are (an optimiser updates them in place): ~0.1 ms of Python per step otherwise
        pkey = tuple((n, q.data_ptr()) for n, q in self.agg.named_parameters() if n in _SLOTS)
        if self._wcache.get("key") != pkey:
            wt = {n: _lib.require_gpu(q.detach(), n, torch.float32) for n, q in self.agg.named_parameters() if n in _SLOTS}
            self._wcache = dict(key=pkey, wt=wt, weights=_fill_weights(wt))
        vw = None
        if V > 0:
            if fw is not None and fw.numel() != V:
                raise HnrError("frame_weight_nearest must hold one weight per reference view (%d), got %d values -- the item's scalar loss weight "
                               "`frame_weight` is a different input (train_step(frame_weight=...))" % (V, fw.numel()))
            vw = _lib.TrainViews(p(inp.w2c), p(inp.intrinsic), p(inp.campos_nearest), p(img), p(fw))
        lut = flags = None
        mode = _drop_mode(opt)
        if ray_drop is not None:
            # explicit [R] flags (a rank's slice of the batch-wide drop pattern when the batch is sharded over GPUs)
            flags = _lib.require_gpu(ray_drop, "ray_drop", torch.uint8).reshape(-1)
        elif mode == "patch" and V > 0:
            key = (R, str(opt.dilation_setup), float(opt.drop_ratio), str(dev))
            if self._lut.get("key") != key:                      # (a host -> device copy: once per batch shape, never inside a captured step)
                self._lut = dict(key=key, lut=drop_lut(opt, R, dev))
            lut = self._lut["lut"]
        elif mode == "random" and V > 0:
            # the random subset needs the ray mask first: one extra query launch (no host read), then explicit flags
            q0 = Q.march_query(grid, campos, raydir, tmid, SR, K, np.float32(hp[0] ** 2), opt.kernel_size, pad=True)
            flags = ray_drop_flags(opt, q0["ray_mask"])
        # all thirteen outputs, uninitialised; under reuse_outputs the same tensors (and their block) for every step of this batch shape
        okey = ("fwd", R, SR, K, str(dev))
        o = self._ocache.get(okey) if self.reuse_outputs else None
        if o is None:
            o = _raycall.RayOutputs.alloc(R, SR, K, dev)
            if self.reuse_outputs:
                self._ocache[okey] = o
        ev = None
        if self.timers is not None:
            ev = _lib.StageEvents(_lib.TRAIN_FWD_STAGES)
            self.timers.setdefault("fwd", []).append(ev)
        out = o.as_dict()
        S = _Saved(prm=prm, ws=ws, ws_ptr=ws_ptr, nbytes=nbytes, dev=dev, R=R, SR=SR, K=K, V=V, no_views=no_views, wt=self._wcache["wt"],
                   weights=self._wcache["weights"], cloud_t=(cloud.xyz, cloud.emb, cloud.conf, cloud.dir, cloud.color),
                   cl=_lib.TrainCloud(p(cloud.xyz), p(cloud.emb), p(cloud.conf), p(cloud.dir), p(cloud.color)), inp=inp, tmid=tmid, cam=inp.camera(tmid),
                   vw=vw, out=o.struct(ev.arr if ev is not None else None), outs=out, keep=(lut, flags, grid))
        with torch.cuda.device(dev):
            _lib.check(L.hnr_render_train_forward(grid.handle, ctypes.byref(prm), ctypes.byref(S.cl), ctypes.byref(S.weights), ctypes.byref(S.cam),
                                                  ctypes.byref(vw) if vw is not None else None, p(lut), p(flags), ws_ptr, nbytes, ctypes.byref(S.out),
                                                  _lib.stream()), "hnr_render_train_forward")
        if want_depth:
            out["coarse_depth"] = ray_depth(out["blend_weight"], out["sample_loc_w"], None, out["ray_mask"], campos, inp.camrot)
        self.last_step = (prm, nbytes)     # tools (bisect_train_forward.py): the step's parameter block and workspace size
        return out, S

    @staticmethod
    def touched_points(S):
        """(ids int32 [capacity] ascending, count int64 [1]) -- views INTO the step's workspace (valid until the next forward on it): the points the
        batch referenced, as the forward call left them on the device (hnr_render_train_touched).  No sort, no host read."""
        L = _lib.lib()
        ids, cnt, cap = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()
        _lib.check(L.hnr_render_train_touched(ctypes.byref(S.prm), S.ws_ptr, S.nbytes, ctypes.byref(ids), ctypes.byref(cnt), ctypes.byref(cap)),
                   "hnr_render_train_touched")
        base = S.ws.data_ptr()
        o_ids, o_cnt = ids.value - base, cnt.value - base
        return S.ws[o_ids:o_ids + 4 * cap.value].view(torch.int32), S.ws[o_cnt:o_cnt + 8].view(torch.int64)

    @staticmethod
    def check_status(out):
        """Reads the forward's status word (a host synchronisation): raises when the workspace capacity was exceeded."""
        st = out["status"].cpu()
        if int(st[0]) != 0:
            raise HnrError("render_train: %d valid shading samples exceed the workspace capacity (TrainPath.cap_samples); the extra ones were dropped" % int(st[1]))

    # ---------------------------------------------------------------------------------------------- backward
    def backward(self, S, g_raycolor, g_conf_out=None, g_depth=None):
        """Returns (point grads dict, aggregator grads dict keyed by parameter name).  g_depth [R]: gradient of the forward's coarse_depth
        (hnr_render_train_backward_depth); None: hnr_render_train_backward."""
        L = _lib.lib()
        dev, p = S.dev, _lib.ptr
        N = int(S.cloud_t[0].shape[0])
        g_raycolor = _lib.require_gpu(g_raycolor, "grad coarse_raycolor", torch.float32).reshape(S.R, 3)
        if g_conf_out is not None:
            g_conf_out = _lib.require_gpu(g_conf_out, "grad conf_coefficient", torch.float32).reshape(S.R, S.SR, S.K)
        if g_depth is not None:
            g_depth = _lib.require_gpu(g_depth, "grad coarse_depth", torch.float32).reshape(S.R)
        bkey = ("bwd", N, S.no_views, id(S.wt), str(dev))
        if self.reuse_outputs and bkey in self._ocache:
            pg, ag, gw, cg, flat, payload = self._ocache[bkey]
        else:
            pg = dict(points_embeding=_f32((N, 32), dev), points_conf=_f32((N,), dev), points_dir=_f32((N, 3), dev), points_color=_f32((N, 3), dev))
            skip = ()
            if S.no_views:
                skip = ("aux_block_", "aux_merge_weight_block.")     # image branch off: like unused parameters in the reference, no gradient
            names = [n for n in S.wt if not n.startswith(skip)]
            sizes = [int(S.wt[n].numel()) for n in names]
            offs = np.concatenate([[0], np.cumsum([(s + 63) // 64 * 64 for s in sizes])])
            flat = _f32((int(offs[-1]) + 64,), dev)               # one buffer for all weight gradients (256-byte aligned slices) + a spare tail (parallel.allreduce_weight_grads)
            ag = {n: flat[int(offs[i]):int(offs[i]) + sizes[i]].view(S.wt[n].shape) for i, n in enumerate(names)}
            gw = _fill_weights(ag)
            payload = int(offs[-1])
            cg = _lib.TrainCloudGrads(p(pg["points_embeding"]), p(pg["points_conf"]), p(pg["points_dir"]), p(pg["points_color"]))
            if self.reuse_outputs:
                self._ocache[bkey] = (pg, ag, gw, cg, flat, payload)
        S.flat, S.flat_payload = flat, payload                   # all weight gradients as ONE buffer: one all-reduce when the batch is sharded over ranks
        S.out.stage_events = None
        if self.timers is not None:
            ev = _lib.StageEvents(_lib.TRAIN_BWD_STAGES)
            self.timers.setdefault("bwd", []).append(ev)
            S.out.stage_events = ev.arr
        # hnr_render_train_backward_depth: the same call with the depth gradient behind the two others
        name = "hnr_render_train_backward" if g_depth is None else "hnr_render_train_backward_depth"
        with torch.cuda.device(dev):
            _lib.check(getattr(L, name)(ctypes.byref(S.prm), ctypes.byref(S.cl), ctypes.byref(S.weights), ctypes.byref(S.cam),
                                        ctypes.byref(S.vw) if S.vw is not None else None, S.ws_ptr, S.nbytes, ctypes.byref(S.out), p(g_raycolor), p(g_conf_out),
                                        *(() if g_depth is None else (p(g_depth),)), ctypes.byref(cg), ctypes.byref(gw), _lib.stream()), name)
        return pg, ag


class _RenderFn(torch.autograd.Function):
    """inputs: (path, static dict, emb, conf, dir, color, *aggregator parameters) -> (coarse_raycolor [R,3], conf_coefficient [R,SR,K]
    [, coarse_depth [R] when static["want_depth"]]).  The static dict carries the geometry / camera / image inputs (no gradient)."""

    @staticmethod
    def forward(ctx, path, static, emb, conf, pdir, color, *params):
        cloud = PointCloud(static["xyz"], emb, conf, pdir, color)
        out, S = path.forward(cloud, static["raydir"], static["campos"], static["camrot"], static["bg_color"], static["near"],
                              static["far"], static["c2w_nearest"], static["campos_nearest"], static["intrinsic_nearest"],
                              static["images_nearest"], frame_weight=static.get("frame_weight"), tmid=static.get("tmid"),
                              ray_drop=static.get("ray_drop"), want_depth=static.get("want_depth", False))
        ctx.path, ctx.S = path, S
        ctx.shapes = (emb.shape, conf.shape, pdir.shape, color.shape)
        ctx.param_names = static["param_names"]
        static["_out"] = out
        # an output the loss does not use arrives as None: the depth then takes the colour-only backward (no depth term at all), the colour and
        # conf_coefficient get the zeros autograd would have materialised
        ctx.set_materialize_grads(False)
        col, cc = out["coarse_raycolor"], out["conf_coefficient"]
        if "coarse_depth" in out:
            return col, cc, out["coarse_depth"]
        return col, cc

    @staticmethod
    def backward(ctx, g_col, g_cc, g_depth=None):
        S = ctx.S
        if g_col is None:
            g_col = torch.zeros((S.R, 3), dtype=torch.float32, device=S.dev)
        if g_cc is None:
            g_cc = torch.zeros((S.R, S.SR, S.K), dtype=torch.float32, device=S.dev)
        pg, ag = ctx.path.backward(S, g_col.contiguous(), g_cc.contiguous(), None if g_depth is None else g_depth.contiguous())
        es, cs, ds, ks = ctx.shapes
        grads = [None, None, pg["points_embeding"].reshape(es), pg["points_conf"].reshape(cs), pg["points_dir"].reshape(ds),
                 pg["points_color"].reshape(ks)]
        for n in ctx.param_names:
            grads.append(ag.get(n))
        ctx.S = None
        return tuple(grads)


def render_train(path, aggregator, xyz, emb, conf, pdir, color, raydir, campos, camrot, bg_color, near, far, c2w_nearest,
                 campos_nearest, intrinsic_nearest, images_nearest, frame_weight=None, tmid=None, ray_drop=None, want_depth=False, Rw2c=None):
    """Differentiable render of one ray batch.  emb/conf/pdir/color may be nn.Parameters (reference shapes [1,N,32], [1,N,1],
    [1,N,3], [1,N,3]); aggregator parameters receive gradients through the returned tensors.  Returns the output dict of
    TrainPath.forward with `coarse_raycolor` and `conf_coefficient` (and with want_depth `coarse_depth` [R]) attached to the autograd graph."""
    _no_rotation("render_train", Rw2c, xyz)
    names = [n for n, _ in aggregator.named_parameters()]
    params = [q for _, q in aggregator.named_parameters()]
    static = dict(xyz=xyz, raydir=raydir, campos=campos, camrot=camrot, bg_color=bg_color, near=near, far=far,
                  c2w_nearest=c2w_nearest, campos_nearest=campos_nearest, intrinsic_nearest=intrinsic_nearest,
                  images_nearest=images_nearest, frame_weight=frame_weight, tmid=tmid, ray_drop=ray_drop, param_names=names, want_depth=bool(want_depth))
    res = _RenderFn.apply(path, static, emb, conf, pdir, color, *params)
    out = dict(static.pop("_out"))
    out["coarse_raycolor"], out["conf_coefficient"] = res[0], res[1]
    if want_depth:
        out["coarse_depth"] = res[2]
    return out


def _queue_step(path, cloud, raydir, campos, camrot, bg_color, near, far, c2w_nearest, campos_nearest, intrinsic_nearest, images_nearest, gt_image,
                zero_epsilon, w_color, w_zero_one, frame_weight, tmid, ray_drop, frame_weight_nearest, blur, w2c_nearest, device_frame_weight=None,
                learnable_blur=None, gt_depth=None, w_depth=0.0, ssim=None):
    """The launches of one step, queued back to back on the current stream: forward -> [blur module] -> loss kernels -> [SSIM term] -> [depth term] ->
    [blur module backward] -> backward.  Nothing is read back; shared by train_step (eager) and CapturedTrainStep (inside a hipGraph capture).
    learnable_blur (blur.LearnableBlur): the learnable-kernel form of the blur module in the same two places; its eight gradients join `ag`.
    gt_depth [R] (checked by _depth_arg): the forward also forms coarse_depth, hnr_depth_loss adds w_depth * L to the total and its gradient goes
    into the backward (hnr_render_train_backward_depth); None: none of that.  ssim (from _ssim_arg): hnr_ssim_loss on the colours the colour losses
    see, its term added to the total and its gradient added in place to the colour gradient, so it travels back through the blur module; None: none
    of that."""
    from .losses import shipped_loss_grads, depth_loss_grads, ssim_patch_loss_grads
    from .blur import blur_select, blur_select_bwd
    out, S = path.forward(cloud, raydir, campos, camrot, bg_color, near, far, c2w_nearest, campos_nearest, intrinsic_nearest, images_nearest,
                          frame_weight=frame_weight_nearest, tmid=tmid, ray_drop=ray_drop, w2c_nearest=w2c_nearest, want_depth=gt_depth is not None)
    col = out["coarse_raycolor"]
    sel = None
    if blur is not None:
        # add_blur_sim=1 (models/mvs_points_volumetric_model.py:145-146 -> base_rendering_model.py:677-745): per patch, the pre-defined kernel whose
        # blurred render is closest to the ground truth replaces the render before the losses
        kernels, pn, ps = blur
        col, sel, kk = blur_select(col, gt_image, kernels, pn, ps)
    elif learnable_blur is not None:
        # learnable_blur_kernel=1 (models/mvs_points_volumetric_model.py:143-144 -> base_rendering_model.py:827-1020): one launch
        col = learnable_blur.forward(col, gt_image)
    parts, g_col, g_cc = shipped_loss_grads(col, out["conf_coefficient"], gt_image, out["ray_mask"], zero_epsilon, w_color, w_zero_one, frame_weight,
                                            conf_rows=True, device_frame_weight=device_frame_weight)
    loss_ssim = None
    if ssim is not None:
        # models/base_rendering_model.py:1120-1143: 1 - SSIM on the patches of `col`; parts[0] += fw w_ssim L, g_col += its gradient (two launches)
        s_pn, s_ps, s_layout, s_w, s_norm = ssim
        loss_ssim, g_col = ssim_patch_loss_grads(col, gt_image, out["ray_mask"], s_pn, s_ps, s_w, layout=s_layout, norm_patches=s_norm,
                                                 frame_weight=frame_weight, device_frame_weight=device_frame_weight, total=parts, g_color=g_col)
    g_depth = loss_depth = None
    if gt_depth is not None:
        # the depth of the UNBLURRED render (the blur module models the camera's colour response, not its geometry); parts[0] += w_depth * L
        loss_depth, g_depth = depth_loss_grads(out["coarse_depth"], gt_depth, out["ray_mask"], w_depth, total=parts)
    if blur is not None:
        g_col = blur_select_bwd(g_col, kk, sel, pn, ps)
    elif learnable_blur is not None:
        g_col, g_blur = learnable_blur.backward(g_col)        # two launches: per patch, then the weight / bias gradients
    pg, ag = path.backward(S, g_col, g_cc, g_depth)
    out = dict(out)
    out["loss"] = parts
    if loss_depth is not None:
        out["loss_depth"] = loss_depth
    if loss_ssim is not None:
        out["loss_ssim"] = loss_ssim
    if blur is not None:
        out["blurred_raycolor"], out["blur_select"] = col, sel
    elif learnable_blur is not None:
        ag = dict(ag)
        ag.update(g_blur)                                     # under the aggregator's parameter names: merge_grads / _assign_grads need no special case
        out["blurred_raycolor"], out["blur_kernels_pred"] = col, learnable_blur.kernels
    return out, S, pg, ag


def _learnable_arg(who, blur_kernels, learnable_blur):
    if learnable_blur is None:
        return None
    if blur_kernels is not None:
        raise HnrError("%s: blur_kernels (add_blur_sim=1) and learnable_blur (learnable_blur_kernel=1) are two branches of one step "
                       "(models/mvs_points_volumetric_model.py:143-147); give one of them" % who)
    from .blur import LearnableBlur
    if not isinstance(learnable_blur, LearnableBlur):
        raise HnrError("%s: learnable_blur must be a blur.LearnableBlur" % who)
    return learnable_blur


def _depth_arg(who, gt_depth, w_depth, raydir, patch_layout="grid"):
    """gt_depth [R] on the rays' device and w_depth >= 0, checked before anything is queued -> (gt_depth flat or None, float w_depth)."""
    w = float(w_depth)
    if gt_depth is None:
        if w != 0.0:
            raise HnrError("%s: w_depth=%g without gt_depth (frames.BatchSampler emits it for a FrameBank with depth frames)" % (who, w))
        return None, 0.0
    if not (w >= 0.0 and w < float("inf")):
        raise HnrError("%s: w_depth must be finite and >= 0, got %r" % (who, w_depth))
    if not isinstance(gt_depth, torch.Tensor) or not gt_depth.is_cuda or gt_depth.dtype != torch.float32:
        raise HnrError("%s: gt_depth must be a float32 tensor on the GPU (0 = no measurement)" % who)
    R = int(raydir.reshape(-1, 3).shape[0])
    if gt_depth.numel() != R or gt_depth.device != raydir.device:
        raise HnrError("%s: gt_depth must hold one depth per ray (%d) on %s, got %d on %s" % (who, R, raydir.device, gt_depth.numel(), gt_depth.device))
    if patch_layout == "patch_major":
        # whole-patch packing is a rank's share of a sharded batch (parallel.shard_patches): the masked mean's n would be the rank's own
        raise HnrError("%s: gt_depth is not supported for a rank's share of a sharded batch (patch_layout='patch_major'): the depth term's ray "
                       "count is local to the call" % who)
    return gt_depth.contiguous().reshape(-1), w


def _ssim_arg(who, w_ssim, patch_num, patch_size, patch_layout, raydir, norm_patches=None):
    """The SSIM term's arguments, checked before anything is queued -> None (w_ssim == 0: today's launches) or (patch_num, patch_size, layout,
    w_ssim, norm_patches) for losses.ssim_patch_loss_grads."""
    from .losses import _ssim_check
    w = float(w_ssim)
    if w == 0.0:
        if norm_patches is not None:
            raise HnrError("%s: ssim_norm_patches without w_ssim" % who)
        return None
    if not patch_num or not patch_size:
        raise HnrError("%s: w_ssim=%g needs a patch-sampled batch (patch_num, patch_size, patch_layout 'grid' | 'patch_major'; frames.BatchSampler's "
                       "'dilated' and 'patch' modes): a 'random' batch has no patches" % (who, w))
    _ssim_check(who, int(raydir.reshape(-1, 3).shape[0]), patch_num, patch_size, patch_layout, w, norm_patches)
    return (int(patch_num), int(patch_size), patch_layout, w, None if norm_patches is None else int(norm_patches))


def _blur_arg(blur_kernels, patch_num, patch_size, patch_layout):
    if blur_kernels is None:
        return None
    if patch_layout not in ("grid", "patch_major") or not patch_num or not patch_size:
        raise HnrError("train_step: blur_kernels need patch_num, patch_size and patch_layout 'grid' | 'patch_major'")
    return (blur_kernels, -int(patch_num) if patch_layout == "patch_major" else int(patch_num), int(patch_size))


def _assign_grads(aggregator, emb, conf, pdir, color, pg, ag, accumulate=True, cached=False):
    """Sets / adds to the .grad fields as autograd would.  `cached`: pg / ag are buffers the NEXT step overwrites in place (TrainPath.reuse_outputs,
    CapturedTrainStep): with accumulate a .grad never aliases them (first assignment clones, later ones add in place into the clone), so
    optimizer.zero_grad(set_to_none=False) and gradient accumulation see autograd's semantics; accumulate=False hands out the buffers themselves."""
    def put(t, g):
        if not (isinstance(t, torch.Tensor) and t.requires_grad):
            return
        g = g.reshape(t.shape)
        if not accumulate:
            t.grad = g
        elif t.grad is None:
            t.grad = g.clone() if cached else g
        elif t.grad.data_ptr() == g.data_ptr():
            raise HnrError("train_step: .grad of a parameter IS the step's own gradient buffer (an earlier step assigned it with accumulate_grads=False), "
                           "so its previous value is already overwritten; set the gradients to None or keep accumulate_grads=False")
        else:
            t.grad.add_(g)
    put(emb, pg["points_embeding"]); put(conf, pg["points_conf"]); put(pdir, pg["points_dir"]); put(color, pg["points_color"])
    for n, q in aggregator.named_parameters():
        if n in ag:
            put(q, ag[n])


def train_step(path, aggregator, xyz, emb, conf, pdir, color, raydir, campos, camrot, bg_color, near, far, c2w_nearest, campos_nearest,
               intrinsic_nearest, images_nearest, gt_image, zero_epsilon=1e-3, w_color=1.0, w_zero_one=1e-4, frame_weight=None, tmid=None,
               ray_drop=None, assign_grads=True, frame_weight_nearest=None, blur_kernels=None, patch_num=None, patch_size=None, patch_layout="grid",
               w2c_nearest=None, accumulate_grads=True, device_frame_weight=None, optimizer=None, learnable_blur=None, Rw2c=None, gt_depth=None,
               w_depth=0.0, w_ssim=0.0, ssim_norm_patches=None):
    """forward -> [blur module] -> shipped loss terms -> backward of one ray batch as groups of library launches queued back to back: no autograd
    graph, no masked copies, nothing read back to the host -- the body of the reference's optimize_parameters before its optimizer steps
    (models/neural_points_volumetric_model.py:202-214: self.forward(); loss_total.backward(), with compute_losses of
    models/base_rendering_model.py:1060-1245 in between).  Same arithmetic as render_train + losses.shipped_loss + loss.backward().

    blur_kernels [1,N,ks,ks] / [N,ks,ks] (the item's `blur_kernels`, add_blur_sim=1) with patch_num / patch_size / patch_layout: the blur-handling
    module between the render and the losses (models/mvs_points_volumetric_model.py:145-146, base_rendering_model.py:677-745) -- hnr_blur_select before
    the loss kernels, hnr_blur_select_bwd behind them; patch_layout="patch_major": the batch is `patch_num` whole patches packed (patch, y, x), a rank's
    share of a patch-sharded batch (parallel.shard_patches).  Same arithmetic as render_train + blur.blur_update_output + the loss + loss.backward().

    The reference has TWO frame-weight inputs and so has this call: `frame_weight` is the dataset item's scalar that multiplies loss_total
    (models/base_rendering_model.py:1205; a Python float or a CPU tensor -- converted once, no device read in the step) and
    `frame_weight_nearest` [V] / [1,V] the per-reference-view weights of the image-feature merge under downweight_blurry_feats
    (models/aggregators/point_aggregators.py:1203), a device tensor that only the forward / backward calls read.  `device_frame_weight` [1] float32
    on the device takes the place of `frame_weight` (left None) with no host read: the loss kernels read it, as in CapturedTrainStep --
    frames.BatchSampler's `frame_weight` output goes here.

    emb/conf/pdir/color and the aggregator's parameters are read as they are; with assign_grads their .grad fields are set (or added to,
    as autograd does -- also under TrainPath.reuse_outputs, where a .grad is then a private copy of the step's buffer, never the buffer the next
    step overwrites; accumulate_grads=False assigns the step's own buffers instead: no copy, valid until the next step).

    learnable_blur (a blur.LearnableBlur; not together with blur_kernels -- the reference's shell takes one of the two branches,
    models/mvs_points_volumetric_model.py:143-147): the learnable-kernel blur module (learnable_blur_kernel=1, base_rendering_model.py:827-1020) in the
    same two places -- hnr_blur_learn_forward before the loss kernels, hnr_blur_learn_backward (two launches) behind them.  Its eight gradients join the
    aggregator's under their parameter names (`learn_blur_kernel_block.0.weight` ...), so .grad or the optimiser sees them like every other one; the
    outputs gain `blurred_raycolor` and `blur_kernels_pred` [n_patches, ks, ks] (the module's static buffers, overwritten by its next forward; the eight
    gradients are the module's static buffers too under TrainPath.reuse_outputs and copies otherwise).  Same arithmetic as render_train + blur.learnable_blur_update_output +
    the loss + loss.backward() up to summation order.  Not covered: the conv-block predictor; and in sharded training the predictor's gradients are
    not part of parallel.allreduce_weight_grads' flat buffer -- the caller all-reduces those eight tensors.  None: exactly the launches above.

    optimizer (optim.DeviceAdam / optim.ShellOptimizers; None: exactly the path above): the optimiser step and the schedule tick are queued behind the
    backward on the same stream -- two more launches that read `pg` / `ag` in place -- and .grad is NOT assigned (the reference's
    optimizer.step() + neural_point_optimizer.step() + scheduler.step(), models/mvs_points_volumetric_model.py:111-131, models/base_model.py:148-150).
    The parameters are marked as written (_cache.py), so the renderer's caches follow the new weights.  With TrainPath.reuse_outputs the gradient buffers keep
    their addresses and the optimiser's descriptor table is uploaded once; without it, once per step.

    gt_depth [R] float32 on the device (metres, 0 = no measurement; frames.BatchSampler's `gt_depth` for a FrameBank with depth frames) with
    w_depth >= 0: depth supervision.  The forward also forms coarse_depth (want_depth), hnr_depth_loss -- one launch behind the shipped-loss
    kernels -- computes L = mean over the rays with a hit and a measurement of (coarse_depth - gt_depth)^2, adds w_depth * L to `loss`[0] (NOT
    scaled by the frame weight: the reference scales before it adds its depth items, models/base_rendering_model.py:1204-1215) and hands its gradient
    to the backward (hnr_render_train_backward_depth).  Depth supervises the UNBLURRED render: with a blur module the colour losses see the blurred
    colours, the depth term the depth as rendered.  The outputs gain `coarse_depth` and `loss_depth` = {L, rays counted, w_depth L}.  Same
    arithmetic as render_train(want_depth=True) + losses.depth_loss + backward().  None: exactly the launches above.  Not covered: a rank's share
    of a sharded batch (the ray count n is local; patch_layout="patch_major" raises, and a caller that shards by hand would have to all-reduce n),
    Rw2c clouds (raise), the TORCH_LIBRARY ops.

    w_ssim > 0 with patch_num / patch_size / patch_layout (a patch-sampled batch: frames.BatchSampler's "dilated" or "patch" mode; a "random" batch
    raises): the patch SSIM term of models/base_rendering_model.py:1120-1143 as include/hnr.h defines it.  hnr_ssim_loss -- two launches directly
    behind the shipped-loss kernels, on the same colours (the blurred ones when a blur module is on) -- adds frame_weight * w_ssim * (1 - SSIM) to
    `loss`[0] and ADDS its gradient in place to the colour gradient, before the depth term and before the blur module's backward, so it travels back
    through whichever blur module is on.  w_ssim is an absolute weight (the reference's branch takes color_loss_weights[i]).  The outputs gain
    `loss_ssim` = {L, SSIM, frame_weight w_ssim L, hit rays}.  ssim_norm_patches: with a rank's share of a patch-sharded batch
    (patch_layout="patch_major", parallel.shard_patches) the batch-wide patch count; the ranks' terms and gradients then add up to the whole
    batch's, so the term all-reduces by sum like the rest.  Same arithmetic as render_train + [blur module] + losses.shipped_loss +
    losses.ssim_patch_loss + backward().  w_ssim = 0: exactly the launches above.  Not covered: MS-SSIM, other windows / sigmas / data_range, patch
    sizes outside 7..64 (raise), the TORCH_LIBRARY ops.

    Returns (outputs dict with `loss` = {total, colour MSE, zero-one mean, valid rays} on the device and `_saved` = the step's
    state for TrainPath.touched_points / the flat weight-gradient buffer, point grads dict, aggregator grads dict keyed by parameter name)."""
    _no_rotation("train_step", Rw2c, xyz)           # (Rw2c: only so that a non-identity one raises; see _no_rotation)
    learnable_blur = _learnable_arg("train_step", blur_kernels, learnable_blur)
    gt_depth, w_depth = _depth_arg("train_step", gt_depth, w_depth, raydir, patch_layout)
    ssim = _ssim_arg("train_step", w_ssim, patch_num, patch_size, patch_layout, raydir, ssim_norm_patches)
    cloud = PointCloud(xyz, emb.detach(), conf.detach(), pdir.detach(), color.detach())
    out, S, pg, ag = _queue_step(path, cloud, raydir, campos, camrot, bg_color, near, far, c2w_nearest, campos_nearest, intrinsic_nearest, images_nearest,
                                 gt_image, zero_epsilon, w_color, w_zero_one, frame_weight, tmid, ray_drop, frame_weight_nearest,
                                 _blur_arg(blur_kernels, patch_num, patch_size, patch_layout), w2c_nearest, device_frame_weight=device_frame_weight,
                                 learnable_blur=learnable_blur, gt_depth=gt_depth, w_depth=w_depth, ssim=ssim)
    if learnable_blur is not None and not path.reuse_outputs:
        # LearnableBlur writes into its own static buffers; without reuse_outputs a step hands out gradient tensors of its own (240 KB)
        ag.update({n: ag[n].clone() for n in learnable_blur.names})
    out["_saved"] = S
    if optimizer is not None:
        from .optim import merge_grads
        optimizer.step(merge_grads(pg, ag))
    elif assign_grads:
        _assign_grads(aggregator, emb, conf, pdir, color, pg, ag, accumulate=bool(accumulate_grads), cached=bool(path.reuse_outputs))
    return out, pg, ag


class CapturedTrainStep:
    """train_step captured ONCE in a hipGraph (torch.cuda.CUDAGraph over the HIP graph API) and replayed per step.

    One step is ~150 launches of 10 - 50 us from three queues (the caller's stream and the library's two side streams, forked and joined with events
    inside the two library calls: stream capture follows them, so the graph keeps the three branches); replaying it removes the host's launch cost and
    the gaps between dependent launches -- what the reference pays per step in Python dispatch (models/neural_points_volumetric_model.py:202-214).
    Every launch size of the step is capacity-fixed and reads its true size from device counters, so ONE graph serves every batch of the same shape.

    Inputs live in static device buffers (`self.inputs`: raydir, campos, camrot, bg_color, c2w_nearest, w2c_nearest, campos_nearest, intrinsic_nearest,
    images_nearest, gt_image and, when given at construction, tmid, ray_drop, frame_weight_nearest, blur_kernels; `frame_weight` = one float);
    `step(**tensors)` copies what it is given into them and replays.  tmid=None at construction: the jittered depth tables are drawn INSIDE the graph
    (torch.rand under capture advances the registered generator state on every replay: a fresh jitter per step, as at
    models/neural_points/query_point_indices_worldcoords.py:87).  The weights and the point buffers are read through the pointers they had at capture:
    optimisers that update in place are fine; after prune / grow (new buffers) build a new CapturedTrainStep.  Outputs and gradients are static
    tensors overwritten by every replay.

    optimizer (optim.DeviceAdam / optim.ShellOptimizers; None: the graph ends with the backward, as before): the optimiser step and the schedule tick
    are captured behind the backward -- one replay = one whole iteration -- and .grad is never assigned.  The warm-up steps run WITHOUT the
    optimiser (they must not move the parameters); its descriptor table is uploaded before the capture, which needs the gradient buffers'
    addresses then: TrainPath.reuse_outputs is switched on for the path.  `step()` marks the parameters as written after the replay."""

    def __init__(self, path, aggregator, xyz, emb, conf, pdir, color, sample, near, far, zero_epsilon=1e-3, w_color=1.0, w_zero_one=1e-4,
                 patch_num=None, patch_size=None, patch_layout="grid", warmup=2, optimizer=None, learnable_blur=None, Rw2c=None, w_depth=0.0, w_ssim=0.0,
                 ssim_norm_patches=None):
        """sample: dict of example input tensors (see the class docstring) that fixes shapes and optional inputs.  learnable_blur: as for
        train_step (not together with a `blur_kernels` sample input); its buffers are static, so `blur_kernels_pred` follows every replay.
        A `gt_depth` [R] tensor in the sample captures the depth-supervised form of the step with the weight w_depth (train_step(gt_depth=,
        w_depth=)); it is an input like the others: `step(gt_depth=...)` copies it, `sampler.next(out=cap.inputs)` writes it in place.
        w_ssim > 0 (with patch_num / patch_size; ssim_norm_patches as for train_step): the patch SSIM term is captured with the step; it reads the
        item's frame weight from the `frame_weight` input like the shipped-loss kernels, and `out["loss_ssim"]` follows every replay."""
        _no_rotation("CapturedTrainStep", Rw2c, xyz)
        learnable_blur = _learnable_arg("CapturedTrainStep", sample.get("blur_kernels"), learnable_blur)
        self.path, self.agg = path, aggregator
        self.optimizer = optimizer
        if optimizer is not None:
            path.reuse_outputs = True
        self.leaves = (emb, conf, pdir, color)
        dev = xyz.device
        req = ("raydir", "campos", "camrot", "bg_color", "c2w_nearest", "campos_nearest", "intrinsic_nearest", "images_nearest", "gt_image")
        for k in req:
            if k not in sample:
                raise HnrError("CapturedTrainStep: sample input %r is missing" % k)
        _depth_arg("CapturedTrainStep", sample.get("gt_depth"), w_depth, sample["raydir"], patch_layout)
        ssim = _ssim_arg("CapturedTrainStep", w_ssim, patch_num, patch_size, patch_layout, sample["raydir"], ssim_norm_patches)
        st = {k: _lib.require_gpu(v, k).clone() for k, v in sample.items() if isinstance(v, torch.Tensor) and k != "frame_weight"}
        if "w2c_nearest" not in st:
            st["w2c_nearest"] = torch.inverse(st["c2w_nearest"].reshape(-1, 4, 4)).contiguous()
        fw0 = sample.get("frame_weight")
        fw0 = 1.0 if fw0 is None else (float(fw0.reshape(-1)[0].item()) if isinstance(fw0, torch.Tensor) else float(fw0))   # (construction time: a host read is fine)
        st["frame_weight"] = torch.full((1,), fw0, dtype=torch.float32, device=dev)
        self.inputs = st
        blur = _blur_arg(st.get("blur_kernels"), patch_num, patch_size, patch_layout)
        cloud = PointCloud(xyz, emb.detach(), conf.detach(), pdir.detach(), color.detach())

        def body():
            return _queue_step(path, cloud, st["raydir"], st["campos"], st["camrot"], st["bg_color"], near, far, st["c2w_nearest"], st["campos_nearest"],
                               st["intrinsic_nearest"], st["images_nearest"], st["gt_image"], zero_epsilon, w_color, w_zero_one, None, st.get("tmid"),
                               st.get("ray_drop"), st.get("frame_weight_nearest"), blur, st["w2c_nearest"], device_frame_weight=st["frame_weight"],
                               learnable_blur=learnable_blur, gt_depth=st.get("gt_depth"), w_depth=float(w_depth), ssim=ssim)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(max(1, int(warmup))):       # lazy one-time work of the library (kernel attributes, side streams, the grid) happens here, not under capture
                out, _S, _pg, _ag = body()
            if optimizer is not None:
                from .optim import merge_grads
                optimizer.prepare(merge_grads(_pg, _ag))   # (the table for the reused gradient buffers + the kernels' first launch: nothing of the state moves)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        TrainPath.check_status(out)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=side, capture_error_mode="thread_local"):
            self.out, self.S, self.pg, self.ag = body()
            if optimizer is not None:
                optimizer.step(merge_grads(self.pg, self.ag))
        self.out["_saved"] = self.S

    def step(self, assign_grads=True, frame_weight=None, **tensors):
        """Copies the given inputs into the static buffers (device-to-device, no synchronisation), replays the graph, returns (out, pg, ag) --
        the same static tensors every time."""
        for k, v in tensors.items():
            if k not in self.inputs:
                raise HnrError("CapturedTrainStep.step: %r was not an input at capture (have %s)" % (k, sorted(self.inputs)))
            self.inputs[k].copy_(v.reshape(self.inputs[k].shape), non_blocking=True)
        if "c2w_nearest" in tensors and "w2c_nearest" not in tensors:
            self.inputs["w2c_nearest"].copy_(torch.inverse(self.inputs["c2w_nearest"].reshape(-1, 4, 4)))
        if frame_weight is not None:
            self.inputs["frame_weight"].fill_(float(frame_weight))
        self.graph.replay()
        if self.optimizer is not None:
            self.optimizer.mark_updated()              # the replay wrote the parameters behind torch's back: the caches must see it (_cache.py, rule 3)
        elif assign_grads:
            emb, conf, pdir, color = self.leaves
            _assign_grads(self.agg, emb, conf, pdir, color, self.pg, self.ag, accumulate=False)
        return self.out, self.pg, self.ag
