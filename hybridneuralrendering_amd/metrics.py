"""Evaluation of rendered frames on the device: PSNR / SSIM / RMSE of the 8-bit images and the two test losses.

The second half of the reference's test pass (the first is driver.render_image).  After its chunk loop the reference computes the two
test losses per frame (run/test_ft.py:233-243), writes `coarse_raycolor` and `gt_image` as 8-bit PNGs (utils/visualizer.py:19-26) and
reads them back for PSNR / SSIM / RMSE (run/evaluate.py:34-97, called at run/test_ft.py:260): about ten host round trips, a PNG
encode and a PNG decode per frame, and scikit-image + OpenCV on the host.  Here a frame is one hnr_frame_metrics call behind the
composite (csrc/metrics.hip) that leaves one fp64 row in a device table; the table is read once per test set (`summary()`).

SSIM's `data_range`: the reference hands float images to scikit-image without a data_range, and scikit-image then uses the dtype range
of floats (-1..1, L = 2), so the SSIM the reference publishes is the L = 2 value; that is the default here.  L = 1 is the textbook
value for images in [0, 1].

LPIPS: the reference's other two columns (`lpips`, `vgglpips`) come from perceptual.LPIPS, which runs the pretrained AlexNet / VGG-16 the user
supplies (the package ships no weights).  `TestSetEvaluator(..., lpips={"lpips": LPIPS('alex'), "vgglpips": LPIPS('vgg')})` scores the 8-bit images
hnr_frame_metrics leaves on the device into a second device table per key; without `lpips` nothing changes.
"""
import os

import numpy as np
import torch

from . import _lib
from ._lib import HnrError

# the row hnr_frame_metrics writes (include/hnr.h: HNR_FM_*)
FM = dict(SQERR8=0, N8=1, SSIM=2, MSE_FULL=3, MSE_MASKED=4, N_MASKED=5)
NCOLS = 6
MAX_WIN = 31


def _sq(t, nd):
    return t.reshape(t.shape[-nd:])


def scatter_gt(frame, device):
    """gt_full [h,w,3]: the item's gt_image [R,3] placed by pixel_idx (x, y), zero where no ray was cast -- run/test_ft.py:203-204 -- on the device."""
    h, w = int(frame["h"]), int(frame["w"])
    gt = _lib.require_gpu(_sq(frame["gt_image"], 2).to(device), "gt_image", torch.float32)
    pix = _sq(frame["pixel_idx"], 2)
    if pix.shape[0] != gt.shape[0]:
        raise HnrError("frame_metrics: pixel_idx and gt_image disagree on the number of rays")
    full = torch.zeros((h, w, 3), dtype=torch.float32, device=device)
    full[pix[:, 1].to(device, torch.long), pix[:, 0].to(device, torch.long)] = gt
    return full, gt


def frame_metrics(render_out, frame, win=11, data_range=2.0, out=None, row=0, images8=None):
    """One frame's row of metrics, on the device, without a host synchronisation.

    render_out: what driver.render_image returns (image [h,w,3], coarse_raycolor [R,3], ray_mask [R]); frame: the dataset item it was rendered
    from, with gt_image [R,3] (batch dim optional).  out / row: a [capacity, NCOLS] float64 device table and the row to fill (default: a
    fresh [1, NCOLS] table).  images8: optional pair of [h,w,3] uint8 device tensors that receive the quantised image and ground truth
    (the bytes of the reference's PNGs).  Returns the table; columns are FM[...]; derive() turns rows into the reported numbers."""
    img = _lib.require_gpu(render_out["image"], "image", torch.float32)
    dev = img.device
    if img.dim() != 3 or img.shape[2] != 3:
        raise HnrError("frame_metrics: image must be [h, w, 3]")
    h, w = int(img.shape[0]), int(img.shape[1])
    if (h, w) != (int(frame["h"]), int(frame["w"])):
        raise HnrError("frame_metrics: the image is %dx%d, the frame says %dx%d" % (h, w, int(frame["h"]), int(frame["w"])))
    gt_full, gt = scatter_gt(frame, dev)
    col = _lib.require_gpu(render_out["coarse_raycolor"], "coarse_raycolor", torch.float32).reshape(-1, 3)
    mask = _lib.require_gpu(render_out["ray_mask"], "ray_mask").reshape(-1)
    if mask.dtype != torch.int8:
        mask = mask.to(torch.int8)
    R = int(col.shape[0])
    if gt.shape[0] != R or mask.shape[0] != R:
        raise HnrError("frame_metrics: coarse_raycolor, gt_image and ray_mask disagree on the number of rays")
    if out is None:
        out = torch.zeros((1, NCOLS), dtype=torch.float64, device=dev)
    if not (out.is_cuda and out.dtype == torch.float64 and out.dim() == 2 and out.shape[1] == NCOLS and out.is_contiguous()):
        raise HnrError("frame_metrics: out must be a contiguous [capacity, %d] float64 table on the GPU" % NCOLS)
    if not 0 <= row < out.shape[0]:
        raise HnrError("frame_metrics: row %d outside the table (%d rows)" % (row, out.shape[0]))
    a8 = b8 = None
    if images8 is not None:
        a8, b8 = images8
        for t in (a8, b8):
            if not (t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == (h, w, 3) and t.is_contiguous()):
                raise HnrError("frame_metrics: images8 must be two contiguous [h, w, 3] uint8 tensors on the GPU")
    scratch = _lib.scratch("hnr_frame_metrics_scratch_bytes", h, w, int(win), device=dev)
    _lib.call("hnr_frame_metrics", img, gt_full, h, w, col if R else None, gt if R else None, mask if R else None, R, int(win), float(data_range),
              out[row], a8, b8, scratch, _lib.STREAM)
    return out


def derive(rows):
    """Host side: [n, NCOLS] float64 rows -> the per-frame numbers the reference reports.  psnr / rmse / ssim are those of run/evaluate.py on
    the 8-bit images (psnr = +inf for identical images, as compare_psnr gives); psnr_full / psnr_masked are mse2psnr of the two test losses."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, NCOLS)
    S, n = rows[:, FM["SQERR8"]], rows[:, FM["N8"]]
    with np.errstate(divide="ignore", invalid="ignore"):
        mse8 = S / (65025.0 * n)
        res = dict(psnr=10.0 * np.log10(1.0 / mse8), ssim=rows[:, FM["SSIM"]].copy(), rmse=np.sqrt(mse8),
                   mse_full=rows[:, FM["MSE_FULL"]].copy(), psnr_full=-10.0 * np.log10(rows[:, FM["MSE_FULL"]]),
                   mse_masked=rows[:, FM["MSE_MASKED"]].copy(), psnr_masked=-10.0 * np.log10(rows[:, FM["MSE_MASKED"]]),
                   n_masked=rows[:, FM["N_MASKED"]].copy(), sqerr8=S.copy(), n8=n.copy())
    return res


# the row hnr_depth_metrics writes (include/hnr.h: HNR_DM_*)
DM = dict(N=0, ABS=1, SQ=2, ABSREL=3, D1=4)
DM_NCOLS = 5


def depth_frame_metrics(render_out, frame, out=None, row=0):
    """One frame's row of depth errors, on the device, without a host synchronisation (hnr_depth_metrics, one launch): over the rays with a hit
    (ray_mask > 0) and a measurement (gt_depth > 0), {n, sum |e|, sum e^2, sum |e| / d, #(max(D / d, d / D) < 1.25)} with e = D - d in fp64.
    render_out: driver.render_image(depth=True)'s result (coarse_depth [R], ray_mask [R]); frame: the item with gt_depth [R] (metres, 0 = no
    measurement; frames.BatchSampler.item of a bank with depth frames).  out / row: a [capacity, DM_NCOLS] float64 device table."""
    if "coarse_depth" not in render_out:
        raise HnrError("depth_frame_metrics: the render has no coarse_depth (driver.render_image(..., depth=True))")
    if "gt_depth" not in frame:
        raise HnrError("depth_frame_metrics: the frame has no gt_depth (a FrameBank with depth frames emits it)")
    D = _lib.require_gpu(render_out["coarse_depth"], "coarse_depth", torch.float32).reshape(-1)
    d = _lib.require_gpu(frame["gt_depth"], "gt_depth", torch.float32).reshape(-1)
    mask = _lib.require_gpu(render_out["ray_mask"], "ray_mask").reshape(-1)
    if mask.dtype != torch.int8:
        mask = mask.to(torch.int8)
    R = int(D.shape[0])
    if R < 1 or d.shape[0] != R or mask.shape[0] != R or d.device != D.device:
        raise HnrError("depth_frame_metrics: coarse_depth, gt_depth and ray_mask must hold one value per ray on one device")
    if out is None:
        out = torch.zeros((1, DM_NCOLS), dtype=torch.float64, device=D.device)
    if not (out.is_cuda and out.dtype == torch.float64 and out.dim() == 2 and out.shape[1] == DM_NCOLS and out.is_contiguous()):
        raise HnrError("depth_frame_metrics: out must be a contiguous [capacity, %d] float64 table on the GPU" % DM_NCOLS)
    if not 0 <= row < out.shape[0]:
        raise HnrError("depth_frame_metrics: row %d outside the table (%d rows)" % (row, out.shape[0]))
    _lib.call("hnr_depth_metrics", D, d, mask, R, out[row], _lib.STREAM)
    return out


def derive_depth(rows):
    """Host side: [n, DM_NCOLS] float64 rows -> per-frame depth_abs (mean |e|, metres), depth_rmse, depth_absrel (mean |e| / d), depth_d1 (the
    fraction of rays with max(D / d, d / D) < 1.25) and depth_n; NaN for a frame without a ray that has both a hit and a measurement."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, DM_NCOLS)
    n = rows[:, DM["N"]]
    with np.errstate(divide="ignore", invalid="ignore"):
        return dict(depth_abs=rows[:, DM["ABS"]] / n, depth_rmse=np.sqrt(rows[:, DM["SQ"]] / n), depth_absrel=rows[:, DM["ABSREL"]] / n,
                    depth_d1=rows[:, DM["D1"]] / n, depth_n=n.copy())


class TestSetEvaluator:
    """A [capacity, NCOLS] device table of per-frame rows: add() per frame (no host synchronisation), summary() = the one host read.

    write(out_dir) leaves psnr.txt / ssim.txt / rmse.txt (np.savetxt) and scores.txt ("key: %.6f" lines) exactly as report_metrics does
    (run/evaluate.py:89-97).  lpips: a dict key -> perceptual.LPIPS (the reference's keys are "lpips" for alex and "vgglpips" for vgg): add() also
    fills row n of a [capacity, 6] table per key (d, r_0 .. r_4), summary() gains the keys, write() leaves <key>.txt and lists the metrics in
    evaluate.py's order (psnr, ssim, lpips, vgglpips, rmse).  With save_images=True also step-%04d-coarse_raycolor.png / step-%04d-gt_image.png from the kernel's own
    uint8 images, so the reference's run/evaluate.py can be pointed at the same folder."""
    __test__ = False            # (not a pytest class, whatever its name starts with)

    ORDER = ("psnr", "ssim", "lpips", "vgglpips", "rmse")          # report_metrics' order; other lpips keys follow "vgglpips"

    def __init__(self, capacity, win=11, data_range=2.0, device="cuda:0", save_images=False, lpips=None, depth=False):
        if capacity <= 0:
            raise HnrError("TestSetEvaluator: capacity must be positive")
        # depth: add() also fills row n of a [capacity, DM_NCOLS] table of its own (depth_frame_metrics: the render needs coarse_depth, the frame
        # gt_depth) and summary() gains depth_abs / depth_rmse / depth_absrel / depth_d1 / depth_n; the other table does not change
        self.depth_table = torch.zeros((int(capacity), DM_NCOLS), dtype=torch.float64, device=device) if depth else None
        self._depth_host = None
        self.capacity, self.win, self.data_range, self.save_images = int(capacity), int(win), float(data_range), bool(save_images)
        self.table = torch.zeros((self.capacity, NCOLS), dtype=torch.float64, device=device)
        self.n = 0
        self.img8 = self.gt8 = None          # [capacity, h, w, 3] uint8, allocated by the first add()
        self._host = None
        self.lpips = dict(lpips) if lpips else {}
        for key in self.lpips:
            if key in ("psnr", "ssim", "rmse", "mean") or not isinstance(key, str):
                raise HnrError("TestSetEvaluator: %r cannot name an lpips column" % (key,))
        self.lpips_tables = {k: torch.zeros((self.capacity, 6), dtype=torch.float64, device=device) for k in self.lpips}
        self._pair8 = None                   # the scratch pair of add() when lpips is on and save_images off
        self._lpips_host = None

    @classmethod
    def from_rows(cls, rows, img8=None, gt8=None, win=11, data_range=2.0, lpips_rows=None):
        """An evaluator over rows computed elsewhere (another rank's table, an earlier run): summary() / write() only.  lpips_rows: key -> [n, 6]
        rows of the lpips tables."""
        rows = torch.as_tensor(np.asarray(rows, dtype=np.float64).reshape(-1, NCOLS))
        ev = cls(max(int(rows.shape[0]), 1), win=win, data_range=data_range, device=rows.device, save_images=img8 is not None)
        ev.table[:rows.shape[0]] = rows
        ev.n = int(rows.shape[0])
        if img8 is not None:
            ev.img8, ev.gt8 = torch.as_tensor(img8), torch.as_tensor(gt8)
        for key, lr in (lpips_rows or {}).items():
            lr = torch.as_tensor(np.asarray(lr, dtype=np.float64).reshape(-1, 6))
            if lr.shape[0] != ev.n:
                raise HnrError("TestSetEvaluator.from_rows: %d rows of %s for %d frames" % (lr.shape[0], key, ev.n))
            ev.lpips[key] = None
            ev.lpips_tables[key] = torch.zeros((ev.capacity, 6), dtype=torch.float64)
            ev.lpips_tables[key][:ev.n] = lr
        return ev

    def add(self, render_out, frame):
        if self.n >= self.capacity:
            raise HnrError("TestSetEvaluator: the table is full (%d frames)" % self.capacity)
        pair = None
        if self.save_images:
            h, w = int(frame["h"]), int(frame["w"])
            if self.img8 is None:
                dev = render_out["image"].device
                self.img8 = torch.zeros((self.capacity, h, w, 3), dtype=torch.uint8, device=dev)
                self.gt8 = torch.zeros((self.capacity, h, w, 3), dtype=torch.uint8, device=dev)
            if tuple(self.img8.shape[1:3]) != (h, w):
                raise HnrError("TestSetEvaluator: save_images needs frames of one size")
            pair = (self.img8[self.n], self.gt8[self.n])
        elif self.lpips:
            h, w = int(frame["h"]), int(frame["w"])
            if self._pair8 is None or tuple(self._pair8[0].shape[:2]) != (h, w):
                dev = render_out["image"].device
                self._pair8 = tuple(torch.zeros((h, w, 3), dtype=torch.uint8, device=dev) for _ in range(2))
            pair = self._pair8
        frame_metrics(render_out, frame, win=self.win, data_range=self.data_range, out=self.table, row=self.n, images8=pair)
        for key, model in self.lpips.items():
            if model is None:
                raise HnrError("TestSetEvaluator: %s has rows but no model (from_rows): add() is not available" % key)
            model.pair8(pair[0], pair[1], out=self.lpips_tables[key], row=self.n)
        if self.depth_table is not None:
            depth_frame_metrics(render_out, frame, out=self.depth_table, row=self.n)
        self.n += 1
        self._host = self._lpips_host = self._depth_host = None
        return self.n - 1

    def summary(self):
        """Reads the table (the only host read) -> dict of per-frame float64 arrays (derive()) + "mean": their means over the frames."""
        if self._host is None:
            self._host = self.table[:self.n].cpu().numpy()
        res = derive(self._host)
        if self.lpips_tables:
            if self._lpips_host is None:
                self._lpips_host = {k: t[:self.n].cpu().numpy() for k, t in self.lpips_tables.items()}
            for k, rows in self._lpips_host.items():
                res[k] = rows[:, 0].copy()
                res[k + "_layers"] = rows[:, 1:].copy()
        if self.depth_table is not None:
            if self._depth_host is None:
                self._depth_host = self.depth_table[:self.n].cpu().numpy()
            res.update(derive_depth(self._depth_host))
        with np.errstate(invalid="ignore"):
            res["mean"] = {k: (float(np.mean(v)) if len(v) else float("nan")) for k, v in res.items() if not k.endswith("_layers")}
        return res

    def write(self, out_dir, ids=None):
        """The files of report_metrics (+ the PNGs when save_images); ids: the step numbers of the frames (default 0, 1, ...).  Returns summary()."""
        res = self.summary()
        os.makedirs(out_dir, exist_ok=True)
        text = ""
        keys = [k for k in self.ORDER if k in ("psnr", "ssim", "rmse") or k in self.lpips_tables]
        extra = [k for k in self.lpips_tables if k not in keys]
        at = keys.index("rmse")
        for key in keys[:at] + extra + keys[at:]:
            np.savetxt(os.path.join(out_dir, key + ".txt"), res[key].reshape(-1))
            text += key + ": %.6f\n" % np.mean(res[key])
        with open(os.path.join(out_dir, "scores.txt"), "w") as f:
            f.write(text)
        if self.save_images and self.img8 is not None:
            from PIL import Image
            ids = list(range(self.n)) if ids is None else list(ids)
            a, b = self.img8[:self.n].cpu().numpy(), self.gt8[:self.n].cpu().numpy()
            for k, i in enumerate(ids):
                Image.fromarray(a[k]).save(os.path.join(out_dir, "step-%04d-coarse_raycolor.png" % i))
                Image.fromarray(b[k]).save(os.path.join(out_dir, "step-%04d-gt_image.png" % i))
        return res
