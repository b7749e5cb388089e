"""Point-set maintenance on the device: hole probing -> new points.

Mirror of `probe_hole` in /root/reference/run/train_ft.py:450-569 without its driver plumbing (datasets, chunk loop, visualiser): the
caller renders the probed frames with `opt.prob = 1` (the ray_max_* / shading_avg_* outputs of NeuralPointsRayMarching,
models/neural_points_volumetric_model.py:392-416; here hnr_probe_outputs) and hands the per-ray outputs over; the selection of the
pixels that become points (:527-549: missed-ray neighbourhood, far-distance rule, opacity threshold) runs in csrc/probe.hip, the new
points' attributes are the selected rays' outputs (:551-560).  `NeuralPoints.grow_points` (modules.py) then appends them and drops the
cached voxel grid, so training continues in the same process -- the reference saves and exit()s here (:926-952).

The growth SCHEDULE around it (prob_mode 0, the shipped ScanNet configuration: dev_scripts/w_scannet_etf/scene241_hybrid.sh:135-141):
`RayMissRanking.update` after every optimisation step keeps the table of the frames with the worst ray-miss loss (csrc/rank.hip: one launch, no
host read), `probe_tier` gives the query neighbourhood of the current tier, and `grow_pass` -- every prob_freq steps -- renders exactly those frames
from the frame bank with prob = 1, selects the new points and appends them (run/train_ft.py:878-967).
"""
import ctypes
import itertools

import numpy as np
import torch

from . import _lib
from ._lib import HnrError


def probe_select(output, pixel_idx, gt_image, bg_color, height, width, far_thresh=0.0, opacity_thresh=0.7):
    """Indices (into the frame's rays) of the pixels that become new points, in the reference's order (row-major over the image).
    output: the prob == 1 output dict of one frame ([1, R, C] tensors; ray_mask [1, R]); pixel_idx [1, R, 2] (x, y); gt_image [R, 3]."""
    g = lambda t, n: _lib.require_gpu(t.to(torch.float32), n, torch.float32)
    pix = g(pixel_idx, "pixel_idx").reshape(-1, 2)
    R = pix.shape[0]
    rm = g(output["ray_mask"], "ray_mask").reshape(-1)
    col = g(output["coarse_raycolor"], "coarse_raycolor").reshape(-1, 3)
    far = g(output["ray_max_far_dist"], "ray_max_far_dist").reshape(-1)
    opa = g(output["ray_max_shading_opacity"], "ray_max_shading_opacity").reshape(-1)
    gt = g(gt_image, "gt_image").reshape(-1, 3)
    if not (rm.shape[0] == col.shape[0] == far.shape[0] == opa.shape[0] == gt.shape[0] == R):
        raise HnrError("probe_select: per-ray tensors disagree on the number of rays")
    dev = pix.device
    bg = (ctypes.c_float * 3)(*[float(v) for v in torch.as_tensor(bg_color).reshape(-1)[:3].tolist()])
    miss = torch.empty((height * width,), dtype=torch.int32, device=dev)
    sel = torch.empty((height * width,), dtype=torch.int32, device=dev)
    _lib.call("hnr_probe_select", pix, rm, gt, col, bg, far, opa, R, int(height), int(width), float(far_thresh), float(opacity_thresh), miss, sel,
              _lib.STREAM)
    return sel[sel > 0].long() - 1                    # boolean indexing walks the map in row-major order, like the reference's mask indexing (:551)


def probe_hole(frames, height, width, far_thresh=0.0, opacity_thresh=0.7, prob_mul=1.0):
    """frames: iterable of (output dict, pixel_idx [1,R,2], gt_image [R,3], bg_color [3]) in visiting order.
    Returns (add_xyz, add_embedding, add_color, add_dir, add_conf) as `probe_hole` does, including the reference's accumulation rule
    `add_conf = cat([add_conf, new]) * prob_mul` (:553-554), which rescales the earlier frames' confidences once more per later frame."""
    xyz = emb = col = dr = conf = None
    cat = lambda a, b: b if a is None else torch.cat([a, b], dim=0)
    for output, pixel_idx, gt_image, bg in frames:
        ids = probe_select(output, pixel_idx, gt_image, bg, height, width, far_thresh, opacity_thresh)
        take = lambda k: output[k].reshape(-1, output[k].shape[-1]).index_select(0, ids)
        xyz = cat(xyz, take("ray_max_sample_loc_w"))
        # a cloud without confidence / colour / direction buffers renders these outputs as None: the reference then returns None for them
        # (run/train_ft.py:545-550)
        conf = cat(conf, take("shading_avg_conf")) * prob_mul if output.get("shading_avg_conf") is not None else None
        col = cat(col, take("shading_avg_color")) if output.get("shading_avg_color") is not None else None
        dr = cat(dr, take("shading_avg_dir")) if output.get("shading_avg_dir") is not None else None
        emb = cat(emb, take("shading_avg_embedding"))
    if xyz is None:
        raise HnrError("probe_hole: no frame given")
    return xyz, emb, col, dr, conf


# ------------------------------------------------------------------------------------------------ the growth schedule
def probe_tier(total_steps, prob_tiers, prob_kernel_size):
    """The tier of the growth schedule at `total_steps`: tier = #(prob_tiers < total_steps) (run/train_ft.py:459, :880).  Returns (tier, query_size) --
    the tier's triple of prob_kernel_size (:461) -- or None behind the last tier (tier >= len(prob_kernel_size) // 3: no ranking update,
    models/mvs_points_volumetric_model.py:155, and no grow pass, run/train_ft.py:882).  prob_kernel_size None: (0, None), the cloud's own query_size."""
    if prob_kernel_size is None:
        return 0, None
    ks = [int(v) for v in np.asarray(prob_kernel_size).reshape(-1)]
    tier = int(np.sum(np.asarray(prob_tiers if prob_tiers is not None else [], dtype=np.float64).reshape(-1) < total_steps))
    if tier >= len(ks) // 3:
        return None
    return tier, ks[3 * tier:3 * tier + 3]


class RayMissRanking:
    """The table of the frames with the worst ray-miss loss, on the device (top_ray_miss_ids / top_ray_miss_loss of
    models/mvs_points_volumetric_model.py:154-185).

    n = train_len // prob_num_step + 1 slots for prob_num_step > 1, one slot (the running maximum, no frame ids) for prob_num_step == 1; `ids` =
    arange(n) int32 and `losses` = zeros(n) float32 as reset_ray_miss_ranking leaves them -- so frames 0 .. n-1 count as present from the start,
    like in the reference.  `update` is one launch (hnr_ray_miss_rank) that reads the frame number from device memory: nothing is read back, nothing
    allocated after the first call, capturable behind a captured training step.  Ties of equal losses keep their slot order and a non-finite loss
    leaves the table untouched."""

    def __init__(self, train_len, prob_num_step, device, prob_tiers=None, prob_kernel_size=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise HnrError("RayMissRanking: device must be a GPU (the HIP path has no CPU fallback)")
        train_len, prob_num_step = int(train_len), int(prob_num_step)
        if train_len < 1 or prob_num_step < 1:
            raise HnrError("RayMissRanking: train_len >= 1 and prob_num_step >= 1")
        self.train_len, self.prob_num_step = train_len, prob_num_step
        self.n = train_len // prob_num_step + 1 if prob_num_step > 1 else 1
        if self.n > 1024:
            raise HnrError("RayMissRanking: a table of %d frames (train_len // prob_num_step + 1) is beyond the kernel's 1024" % self.n)
        self.prob_tiers, self.prob_kernel_size = prob_tiers, prob_kernel_size
        self._ids0 = torch.arange(self.n, dtype=torch.int32, device=self.device)
        self.ids = self._ids0.clone()
        self.losses = torch.zeros((self.n,), dtype=torch.float32, device=self.device)
        self.last = torch.zeros((2,), dtype=torch.float32, device=self.device)          # {loss, number of missed rays} of the last update
        self._row = torch.zeros((1,), dtype=torch.int32, device=self.device)            # a Python frame number is uploaded into this

    def reset(self):
        """reset_ray_miss_ranking (:183-185), in place: a captured update keeps its pointers."""
        self.ids.copy_(self._ids0)
        self.losses.zero_()
        return self

    def state_dict(self):
        return {"ids": self.ids.clone(), "losses": self.losses.clone()}

    def load_state_dict(self, state):
        ids, losses = torch.as_tensor(state["ids"]), torch.as_tensor(state["losses"])
        if tuple(ids.shape) != (self.n,) or tuple(losses.shape) != (self.n,):
            raise HnrError("RayMissRanking.load_state_dict: the table has %d slots, got ids %s and losses %s" % (self.n, tuple(ids.shape), tuple(losses.shape)))
        self.ids.copy_(ids.to(torch.int32))
        self.losses.copy_(losses.to(torch.float32))
        return self

    def update(self, out, gt_image, frame_row, total_steps=None):
        """After an optimisation step: out = the dict of train.train_step / CapturedTrainStep.step (full-batch rows: ray_mask int8 [R], coarse_raycolor [R,3]
        and, when the blur module ran, blurred_raycolor -- the colour the loss kernels were given, which the reference writes over
        output["coarse_raycolor"], models/base_rendering_model.py:772), gt_image [R,3], frame_row the batch sampler's device int32 [1] (a Python int is
        uploaded).  total_steps: with the ranking's prob_tiers / prob_kernel_size, no launch behind the last tier (:155).  Returns `last`."""
        if total_steps is not None and probe_tier(total_steps, self.prob_tiers, self.prob_kernel_size) is None:
            return self.last
        color = out["blurred_raycolor"] if out.get("blurred_raycolor") is not None else out["coarse_raycolor"]
        g = _lib.require_gpu
        color, gt = g(color.detach(), "raycolor", torch.float32), g(gt_image, "gt_image", torch.float32)
        mask = g(out["ray_mask"], "ray_mask", torch.int8)
        R = int(mask.numel())
        if color.numel() != 3 * R or gt.numel() != 3 * R:
            raise HnrError("RayMissRanking.update: %d rays in ray_mask, but %d colour and %d gt_image values (the step's full-batch rows are expected)"
                           % (R, color.numel(), gt.numel()))
        if isinstance(frame_row, torch.Tensor):
            row = g(frame_row, "frame_row", torch.int32)
            if row.numel() != 1:
                raise HnrError("RayMissRanking.update: frame_row must hold one int32")
        else:
            row = self._row.fill_(int(frame_row))
        if color.device != self.device or gt.device != self.device or mask.device != self.device or row.device != self.device:
            raise HnrError("RayMissRanking.update: every tensor must live on %s" % self.device)
        _lib.call("hnr_ray_miss_rank", color, gt, mask, R, row, self.ids, self.losses, self.n, self.last, _lib.STREAM)
        return self.last

    def worst(self):
        """The largest loss in the table, a device tensor."""
        return self.losses[0]

    def top_frames(self, max_num):
        """The frames a grow pass probes, in table order: ids[:-1][losses[:-1] > 0][:max_num] (run/train_ft.py:476-477).  The one host read."""
        return [int(i) for i in self.ids[:-1][self.losses[:-1] > 0][:int(max_num)].tolist()]


PROBE_KEYS = ("ray_max_sample_loc_w", "ray_max_shading_opacity", "shading_avg_color", "shading_avg_dir", "shading_avg_conf", "shading_avg_embedding",
              "ray_max_far_dist")


def fill_probe_outputs(out, bg_color):
    """What `fill_invalid` does to a prob == 1 output (models/neural_points_volumetric_model.py:87-137) for the keys probe_hole reads: the rows of the valid
    rays scattered into all R rays -- coarse_raycolor over bg_color, the probe keys over zeros.  out: NeuralPointsRayMarching.forward's dict."""
    mask = out["ray_mask"]
    rows = torch.nonzero(mask[0])[:, 0]
    R = int(mask.shape[1])
    col = out["coarse_raycolor"]
    full = {"ray_mask": mask, "coarse_raycolor": (torch.ones((1, R, 3), dtype=col.dtype, device=col.device) * bg_color.reshape(1, 1, 3)).index_copy_(1, rows, col)}
    for k in PROBE_KEYS:
        v = out.get(k)
        full[k] = None if v is None else torch.zeros((1, R) + tuple(v.shape[2:]), dtype=v.dtype, device=v.device).index_copy_(1, rows, v)
    return full


def probe_frame(net, item, chunk_rays=0):
    """One frame of a grow pass: item = frames.BatchSampler.item(row); net.forward over all its rays (chunk_rays > 0: that many at a time; the probe runs
    without sample jitter, so the chunks give the same bits) with the options as they are set (the caller sets opt.prob = 1, opt.is_train = 0).
    Returns probe_hole's tuple (full-ray output dict, pixel_idx [1,R,2], gt_image [R,3], bg_color [3]) or None when no ray of the frame hit a point."""
    need = ("c2w_nearest", "campos_nearest", "intrinsic_nearest", "images_nearest")
    if any(k not in item for k in need):
        raise HnrError("probe_frame: the item has no reference views (FrameBank.set_nearest)")
    R = int(item["raydir"].shape[0])
    step = R if int(chunk_rays) <= 0 else int(chunk_rays)
    fixed = {k: item[k][None] for k in ("campos", "camrotc2w", "bg_color", "c2w", "intrinsic", "frame_weight_nearest", "vid_angle_nearest") + need if k in item}
    fixed.update(near=torch.tensor([float(item["near"])]), far=torch.tensor([float(item["far"])]), h=item["h"], w=item["w"])
    parts = []
    with torch.no_grad():
        for s in range(0, R, step):
            out = net.forward(raydir=item["raydir"][None, s:s + step], pixel_idx=item["pixel_idx"][None, s:s + step], **fixed)
            if "ray_max_shading_opacity" in out:
                parts.append(fill_probe_outputs(out, item["bg_color"]))
            else:                                             # no valid ray in the chunk: nothing to select there
                parts.append(None)
    if all(p is None for p in parts):
        return None
    proto = next(p for p in parts if p is not None)
    dev = item["raydir"].device
    for i, s in enumerate(range(0, R, step)):
        if parts[i] is None:
            n = min(step, R - s)
            z = {k: (None if proto[k] is None else torch.zeros((1, n) + tuple(proto[k].shape[2:]), dtype=proto[k].dtype, device=dev)) for k in PROBE_KEYS}
            z["ray_mask"] = torch.zeros((1, n), dtype=proto["ray_mask"].dtype, device=dev)
            z["coarse_raycolor"] = torch.ones((1, n, 3), dtype=torch.float32, device=dev) * item["bg_color"].reshape(1, 1, 3)
            parts[i] = z
    full = parts[0] if len(parts) == 1 else {k: (None if proto[k] is None else torch.cat([p[k] for p in parts], dim=1)) for k in proto}
    return full, item["pixel_idx"][None], item["gt_image"], item["bg_color"]


def grow_pass(net, sampler, ranking, total_steps, opt, chunk_rays=0):
    """One grow pass of the shipped schedule, prob_mode 0: the body of run/train_ft.py:878-967 without its exit().  net: modules.NeuralPointsRayMarching;
    sampler: a frames.BatchSampler over the TRAIN bank; ranking: the RayMissRanking kept up to date by `update`; opt: the options object (net.opt), with
    prob_mode, prob_num_step, prob_tiers, prob_kernel_size, prob_thresh, prob_mul, far_thresh, bgmodel.

    Returns 0 without rendering behind the last tier (probe_tier) or when far_thresh <= 0 and the worst ray-miss loss is <= 1e-5 ("nothing to probe",
    :881, :966).  Otherwise the frames ranking.top_frames(train_len // prob_num_step) are rendered whole, in table order, with opt.prob = 1,
    opt.is_train = 0 and opt.query_size = the tier's triple (all three restored afterwards, also on an error), growth.probe_hole selects the new points,
    the ranking is reset (prob_num_step > 1; also when nothing was selected, :564-565) and NeuralPoints.grow_points appends them.  Returns their number.

    The point buffers are NEW tensors afterwards: the caller rebuilds its optimisers (the reference restarts the process for that, :926-952) and any
    train.CapturedTrainStep, which holds the old buffers' pointers.  Not done here: visualiser dumps, checkpoint saving, prune."""
    if int(getattr(opt, "prob_mode", 0)) != 0:
        raise HnrError("grow_pass: only prob_mode 0 (the frames ranked by ray-miss loss) is implemented, got prob_mode=%r" % (opt.prob_mode,))
    if str(getattr(opt, "bgmodel", "no")).startswith("planepoints"):
        raise HnrError("grow_pass: bgmodel %r (filter_plane on the new points) is not supported" % (opt.bgmodel,))
    if int(opt.prob_num_step) <= 1 or ranking.n < 2:
        raise HnrError("grow_pass: prob_num_step == 1 keeps no frame ranking (the reference then probes all frames in a shuffled order); not implemented")
    tier = probe_tier(total_steps, getattr(opt, "prob_tiers", None), getattr(opt, "prob_kernel_size", None))
    if tier is None:
        return 0
    far_thresh = float(getattr(opt, "far_thresh", 0.0))
    if far_thresh <= 0 and not float(ranking.worst()) > 1e-5:
        return 0
    bank = sampler.bank
    num_step = int(opt.prob_num_step)
    rows = ranking.top_frames(bank.F // num_step)
    npnt = net.neural_points
    opts, saved = [], []
    for o in (opt, net.opt, npnt.opt):
        if o is not None and all(o is not q for q in opts):
            opts.append(o)
            saved.append((getattr(o, "prob", 0), getattr(o, "is_train", 0), o.query_size))
    n_new = 0
    try:
        for o in opts:
            o.prob, o.is_train = 1, 0
            if tier[1] is not None:
                o.query_size = list(tier[1])
        # one frame at a time (a generator: a frame's outputs are dropped once its points are taken); frames without a valid ray select nothing
        frames = (f for f in (probe_frame(net, sampler.item(row), chunk_rays) for row in rows) if f is not None)
        first = next(frames, None)
        add = None
        if first is not None:
            add = probe_hole(itertools.chain([first], frames), bank.H, bank.W, far_thresh=far_thresh, opacity_thresh=float(getattr(opt, "prob_thresh", 0.7)),
                             prob_mul=float(getattr(opt, "prob_mul", 1.0)))
        ranking.reset()
        if add is not None and int(add[0].shape[0]) > 0:
            # (still under the probe's query_size: the cached grid was built with it, and grow_points extends THAT grid; the querier's cache key holds
            # query_size, so the first query after the restore below rebuilds the grid when the tier's neighbourhood differs from the training one)
            npnt.grow_points(add[0], add[1], add[2], add[3], add[4])
            n_new = int(add[0].shape[0])
    finally:
        for o, (prob, is_train, qs) in zip(opts, saved):
            o.prob, o.is_train, o.query_size = prob, is_train, qs
    return n_new
