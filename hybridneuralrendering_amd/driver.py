"""Whole-frame render driver: the counterpart of the per-chunk loop of the reference's test / eval drivers.

/root/reference/run/test_ft.py:146-209 (and run/train_ft.py:294-351) slices a frame's rays into `random_sample_size**2`
(= 2304) ray chunks, runs the model per chunk (grid rebuild, projection of all N points, 4-view CNN + 221 MB upsample, three
host syncs -- 124 times per 620x460 frame) and scatters every chunk into an [H,W,3] numpy image through `.cpu()`.
Here a frame is ONE launch of the fused path over all its rays (the grid and the reference-view pyramid are built once),
the [H,W,3] image is assembled on the device by pixel index, and with torch.distributed the rays are sharded over the ranks
and reassembled on rank 0 with one gather (parallel.render_sharded).  Chunking is still available (`chunk_rays`) and gives
the same pixels at jitter 0 (tests/test_render_gpu.py::test_whole_frame_equals_the_reference_chunk_loop, against a frame the imported
reference rendered chunk by chunk).
"""
import os

import torch
import torch.distributed as dist

from . import _lib
from ._lib import HnrError
from . import parallel


def _frame_rows(renderer, cloud, frame, chunk_rays, sharded, group, depth):
    """The ray path of render_image: the frame's rays through render_rays (whole, chunked or sharded), the status words checked once per frame ->
    (rows [R, 4 or 5] = colour, mask, depth; None on the ranks that do not assemble), pixel_idx [R,2], h, w."""
    sq = lambda t, nd: t.reshape(t.shape[-nd:]) if isinstance(t, torch.Tensor) else t
    raydir = sq(frame["raydir"], 2)
    pix = sq(frame["pixel_idx"], 2)
    R = raydir.shape[0]
    if pix.shape[0] != R:
        raise HnrError("render_image: pixel_idx and raydir disagree on the number of rays")
    h, w = int(frame["h"]), int(frame["w"])
    near, far = float(torch.as_tensor(frame["near"]).min()), float(torch.as_tensor(frame["far"]).max())
    fw = frame.get("frame_weight_nearest")
    if sharded is None:
        sharded = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1

    statuses = []

    def render(rays):
        outs = []
        step = rays.shape[0] if chunk_rays <= 0 else chunk_rays
        for lo in range(0, rays.shape[0], max(step, 1)):
            o = renderer.render_rays(cloud, rays[lo:lo + step].contiguous(), sq(frame["campos"], 1), sq(frame["camrotc2w"], 2),
                                     sq(frame["bg_color"], 1), near, far, sq(frame["c2w_nearest"], 3), sq(frame["campos_nearest"], 2),
                                     sq(frame["intrinsic_nearest"], 2), sq(frame["images_nearest"], 4),
                                     frame_weight=None if fw is None else sq(fw, 1), want_depth=depth)
            statuses.append(o)
            cols = [o["coarse_raycolor"], o["ray_mask"].to(torch.float32)[:, None]] + ([o["coarse_depth"][:, None]] if depth else [])
            outs.append(torch.cat(cols, dim=1))
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)

    def render_auto(rays):
        """whole block in one launch; when the workspace does not fit (render_rays says so) halve the chunk until it does"""
        nonlocal chunk_rays
        for _ in range(8):
            try:
                return render(rays)
            except HnrError as e:
                if "in chunks" not in str(e):
                    raise
                chunk_rays = max((rays.shape[0] if chunk_rays <= 0 else chunk_rays) // 2, 1)
        return render(rays)

    rows = parallel.render_sharded(render_auto, raydir, group=group) if sharded else render_auto(raydir)
    # the device status words of this rank's launches, read once per frame (after everything is queued): an overflow of a workspace capacity
    # must not pass silently
    renderer.check_status([dict(status=o.get("status")) for o in statuses])
    return rows, pix, h, w


def render_image(renderer, cloud, frame, chunk_rays=0, sharded=None, group=None, depth=False):
    """frame: dict with the dataset item of the reference (data/scannet_ft_dataset.py:855-976), batch dim optional:
    raydir [R,3], pixel_idx [R,2] (x, y), campos [3], camrotc2w [3,3], bg_color [3], near, far, h, w, c2w_nearest [V,4,4],
    campos_nearest [V,3], intrinsic_nearest [3,3], images_nearest [V,H,W,3] (+ optional frame_weight_nearest [V]).
    Returns dict(image [h,w,3] (zero where no ray was cast: run/test_ft.py:191 scatters into np.zeros), ray_mask [R] i8, coarse_raycolor [R,3]) --
    on rank 0 when sharded, None on the other ranks.  depth=True adds depth [h,w] (zero where no ray was cast) and coarse_depth [R], the expected
    camera-space depth of every ray (render_rays(want_depth=True); 0 where ray_mask = 0); sharded, it travels as a fifth row column."""
    rows, pix, h, w = _frame_rows(renderer, cloud, frame, chunk_rays, sharded, group, depth)
    if rows is None:
        return None
    col, mask = rows[:, :3].contiguous(), rows[:, 3].to(torch.int8)
    img = torch.zeros((h, w, 3), dtype=torch.float32, device=col.device)        # test_ft.py:191 `np.zeros((height, width, 3))`: the margin stays zero
    px, py = pix[:, 0].to(col.device, torch.long), pix[:, 1].to(col.device, torch.long)
    img[py, px] = col                                            # test_ft.py:193 `visuals[key][y, x, :] = chunk`, on the device
    res = dict(image=img, ray_mask=mask, coarse_raycolor=col)
    if depth:
        d = rows[:, 4].contiguous()
        dimg = torch.zeros((h, w), dtype=torch.float32, device=col.device)
        dimg[py, px] = d
        res.update(depth=dimg, coarse_depth=d)
    return res


def evaluate_frames(renderer, cloud, frames, evaluator=None, win=11, data_range=2.0, save_images=False, chunk_rays=0, sharded=None, group=None, on_frame=None,
                    lpips=None, depth=False):
    """The reference's test pass over a test set (run/test_ft.py:127-260): render_image + one metrics row per frame (metrics.TestSetEvaluator.add:
    one launch behind the composite, no host read), frames being dataset items with gt_image [R,3].  Returns the evaluator -- summary() is
    the one host read, write(out_dir) leaves report_metrics' files -- on rank 0 when sharded, None on the other ranks.  render_image is called
    as it stands: the rendered frames are what a plain call gives; on_frame(index, render_out), when given, sees each of them (rank 0).
    lpips: a dict such as {"lpips": LPIPS('alex'), "vgglpips": LPIPS('vgg')} (perceptual.LPIPS with weights loaded) adds those columns
    (TestSetEvaluator(lpips=...)); the rendered frame and the existing columns do not change.  depth=True: the frames carry gt_depth [R] (metres,
    0 = no measurement: frames.BatchSampler.item of a bank with depth frames), render_image also forms the depth map (depth=True) and the
    evaluator keeps one depth-error row per frame (TestSetEvaluator(depth=True): depth_abs / depth_rmse / depth_absrel / depth_d1); colours and
    the existing columns do not change."""
    from .metrics import TestSetEvaluator
    frames = list(frames)
    if depth and any("gt_depth" not in f for f in frames):
        raise HnrError("evaluate_frames: depth=True needs gt_depth in every frame")
    for i, frame in enumerate(frames):
        out = render_image(renderer, cloud, frame, chunk_rays=chunk_rays, sharded=sharded, group=group, depth=bool(depth))
        if out is None:
            continue
        if on_frame is not None:
            on_frame(i, out)
        if evaluator is None:
            evaluator = TestSetEvaluator(len(frames), win=win, data_range=data_range, device=out["image"].device, save_images=save_images, lpips=lpips,
                                         depth=bool(depth))
        evaluator.add(out, frame)
    return evaluator


class Clip:
    """The frames of a rendered camera path, on the device: frames [P,h,w,3] uint8 (quantised as hnr_frame_metrics quantises: trunc(clip(x, 0, 1) *
    255)), ray_hits [P] int64 (rays of every frame that hit the cloud), and, when asked for, depth [P,h,w] float32 and images [P,h,w,3] float32."""

    def __init__(self, frames, ray_hits, depth=None, images=None):
        self.frames, self.ray_hits, self.depth, self.images = frames, ray_hits, depth, images

    def __len__(self):
        return int(self.frames.shape[0])

    def to_numpy(self):
        """The one host read: dict(frames, ray_hits[, depth][, images]) of NumPy arrays."""
        out = dict(frames=self.frames.cpu().numpy(), ray_hits=self.ray_hits.cpu().numpy())
        if self.depth is not None:
            out["depth"] = self.depth.cpu().numpy()
        if self.images is not None:
            out["images"] = self.images.cpu().numpy()
        return out

    def write(self, out_dir, name="coarse_raycolor", gif=False, fps=10):
        """step-%04d-<name>.png per frame (the file names of the reference's visualizer), and with gif=True <name>.gif of all frames; returns the
        list of files written."""
        from PIL import Image
        os.makedirs(out_dir, exist_ok=True)
        frames = self.frames.cpu().numpy()
        files = []
        for i, f in enumerate(frames):
            files.append(os.path.join(out_dir, "step-%04d-%s.png" % (i, name)))
            Image.fromarray(f).save(files[-1])
        if gif:
            files.append(os.path.join(out_dir, "%s.gif" % name))
            ims = [Image.fromarray(f) for f in frames]
            ims[0].save(files[-1], save_all=True, append_images=ims[1:], duration=max(int(round(1000.0 / fps)), 1), loop=0)
        return files


def render_path(renderer, cloud, sampler, frames=None, depth=False, chunk_rays=0, keep_float=False):
    """run/render_vid.py's loop, on the device: every frame of a camera path (frames.PathSampler) rendered through render_image's ray path and stored
    into a clip by hnr_frame_store -- one launch behind the composite instead of torch.zeros + index-put + a quantisation per frame, no host
    read besides the status words render_image also reads.  frames=None: the whole path, P frames in order from the sampler's device counter
    (`sampler.next()`); frames = a list of frame numbers: those (`sampler.item(i)`).  depth=True adds the expected-depth maps, keep_float=True the
    float32 frames.  Returns a Clip.  A cloud with per-part rotations (edit.compose: Rw2c) goes through as it does in render_image.
    Not covered: sharded rendering (world size > 1)."""
    from .frames import PathSampler
    if not isinstance(sampler, PathSampler):
        raise HnrError("render_path: sampler must be a frames.PathSampler")
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise HnrError("render_path: sharded rendering (world size > 1) is not covered; render the path on one rank")
    if frames is not None:
        frames = [int(i) for i in frames]
        if not frames or min(frames) < 0 or max(frames) >= sampler.P:
            raise HnrError("render_path: frames must be a non-empty list of frame numbers 0 .. %d" % (sampler.P - 1))
    n = sampler.P if frames is None else len(frames)
    dev, h, w = sampler.bank.device, sampler.bank.H, sampler.bank.W
    clip8 = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    clipd = torch.empty((n, h, w), dtype=torch.float32, device=dev) if depth else None
    clipf = torch.empty((n, h, w, 3), dtype=torch.float32, device=dev) if keep_float else None
    hits = torch.zeros((n,), dtype=torch.int64, device=dev)
    for k in range(n):
        item = sampler.next() if frames is None else sampler.item(frames[k])
        rows, pix, _h, _w = _frame_rows(renderer, cloud, item, chunk_rays, False, None, bool(depth))
        col = rows[:, :3].contiguous()
        d = rows[:, 4].contiguous() if depth else None
        hits[k] = rows[:, 3].sum().to(torch.int64)
        _lib.call("hnr_frame_store", col, pix.contiguous(), d, int(col.shape[0]), h, w, clip8[k], clipf[k] if keep_float else None,
                  clipd[k] if depth else None, _lib.STREAM)
    return Clip(clip8, hits, depth=clipd, images=clipf)
