"""A scene's frames resident on the device and the ray batch of every training step drawn there (csrc/frames.hip).

The reference builds a batch on the host, per step: data/scannet_ft_dataset.py:736-976 (nerf_synth360_ft_dataset.py:643-800) decodes the target frame
and its nearest frames, draws pixel coordinates with numpy, builds `raydir` with get_dtu_raydir, gathers `gt_image` and uploads ~15 MB of float
reference images.  A train split is 200 - 1000 frames of 480 x 640 x 3 bytes: it fits on the device as it is.  `FrameBank` holds it there,
`BatchSampler.next()` writes the dataset item of the next step with at most three launches that read the frame number and the step counter from
device memory -- no upload, no host read, capturable in a hipGraph.  Image decoding stays the caller's (once per scene); the resize to the bank's
size -- Pillow's LANCZOS, the same bytes -- runs on the device: `FrameBank.from_raw`, `FrameBank.ingest`, `resize_frames` (csrc/resize.hip).
A bank may also hold the split's sensor depth frames (`FrameBank(depth=...)`): the batch then carries `gt_depth` per ray, written by a fourth
launch of the same kind (csrc/depth_sup.hip), for train.train_step(gt_depth=, w_depth=).

The nearest-view tables are per-frame constants and are computed on the host: `nearest_by_id` (ScanNet), `nearest_by_pose` (synthetic scenes).
tests/frames_ref.py restates the sampler's arithmetic in NumPy; the GPU results equal it bit for bit.
"""
import ctypes
import warnings

import numpy as np
import torch

from . import _lib
from ._cache import mark_written
from ._lib import HnrError

MODES = {"random": 0, "patch": 1, "dilated": 2}


def nearest_by_id(query_ids, train_ids, V, exclude_self, weights=None, select_high_quality=False, dynamic_nearest=False):
    """data/scannet_ft_dataset.py:771-812: for every query frame id the V train frames with the closest ids -> rows into train_ids, int32 [Q,V].
    exclude_self: drop a train frame whose id IS the query's (find_nearest_mode 0 always; find_nearest_mode 1 for the train split only).
    select_high_quality: of the int(1.5 V) closest, the V with the largest `weights` (train_weight_list).  Equal distances (frames at -5 and +5) keep
    the order of train_ids (a stable sort; the reference's np.argsort leaves it unspecified)."""
    if dynamic_nearest:
        raise HnrError("nearest_by_id: dynamic_nearest draws the number of views afresh every step, which changes tensor shapes; not supported")
    train_ids = np.asarray(train_ids)
    V = int(V)
    if V < 1 or train_ids.ndim != 1:
        raise HnrError("nearest_by_id: V >= 1 and a flat list of train ids")
    if select_high_quality and weights is None:
        raise HnrError("nearest_by_id: select_high_quality needs the train frames' weights")
    rows = []
    for vid in np.asarray(query_ids).reshape(-1):
        dist = np.abs(train_ids - vid)
        order = np.argsort(dist, kind="stable")
        skip = 1 if (exclude_self and dist[order[0]] == 0) else 0
        if select_high_quality:
            cand = order[skip:skip + int(V * 1.5)]
            cand = cand[np.argsort(-np.asarray(weights, dtype=np.float64)[cand], kind="stable")]
            pick = cand[:V]
        else:
            pick = order[skip:skip + V]
        if len(pick) != V:
            raise HnrError("nearest_by_id: %d train frames cannot give %d nearest views" % (len(train_ids), V))
        rows.append(pick)
    return np.asarray(rows, dtype=np.int32).reshape(-1, V)


def center_raydir(intrinsic, c2w, width, height):
    """nerf_synth360_ft_dataset.py:740-741: the normalised direction of pixel (width // 2, height // 2), get_dtu_raydir in NumPy as the reference runs it."""
    K, R = np.asarray(intrinsic, dtype=np.float32), np.asarray(c2w, dtype=np.float32)[:3, :3]
    pix = np.asarray([width, height]).astype(np.float32)[None, :] // 2
    x = (pix[..., 0] + 0.5 - K[0, 2]) / K[0, 0]
    y = (pix[..., 1] + 0.5 - K[1, 2]) / K[1, 1]
    d = np.stack([x, y, np.ones_like(x)], axis=-1) @ R.T
    return d / (np.linalg.norm(d, axis=-1, keepdims=True) + 1e-5)


def nearest_by_pose(query_c2w, query_intrinsic, query_ids, train_pos, train_dirs, train_ids, V, width, height, is_train, num_times=3):
    """`get_nearest_cam_id` (nerf_synth360_ft_dataset.py:49-74) for every query camera -> int32 [Q,V], entries of train_ids (which the reference uses as
    rows of its train arrays).  Step 1: the num_times * V train cameras (at most a tenth of them) whose direction train_dirs [T,3] is closest to
    the query's centre-pixel direction; step 2: of those the V closest in position train_pos [T,3]; the query itself is skipped when is_train.
    query_intrinsic: [3,3] or one per query."""
    train_pos, train_dirs, train_ids = np.asarray(train_pos), np.asarray(train_dirs), np.asarray(train_ids)
    K = np.asarray(query_intrinsic, dtype=np.float32)
    V = int(V)
    n1 = min(int(num_times) * V, int(len(train_ids) * 0.1))
    rows = []
    for q, (M, cid) in enumerate(zip(np.asarray(query_c2w, dtype=np.float32), np.asarray(query_ids).reshape(-1))):
        d = center_raydir(K[q] if K.ndim == 3 else K, M, width, height)
        idx1 = np.argsort(-train_dirs.dot(d[0]), kind="stable")[:n1]
        ids1, pos1 = train_ids[idx1], train_pos[idx1]
        idx2 = np.argsort(np.linalg.norm(pos1 - M[:3, 3], axis=1), kind="stable")
        skip = 1 if (len(idx2) and ids1[idx2[0]] == cid and is_train) else 0
        pick = ids1[idx2[skip:skip + V]]
        if len(pick) != V:
            raise HnrError("nearest_by_pose: %d train cameras leave %d candidates, fewer than the %d views asked for" % (len(train_ids), len(idx2) - skip, V))
        rows.append(pick)
    return np.asarray(rows, dtype=np.int32).reshape(-1, V)


# ---------------------------------------------------------------------------------------------------- raw frames to the bank's size (csrc/resize.hip)
_TABLES, _DEV_TABLES = {}, {}


def resize_tables(n_in, n_out, filter="lanczos"):
    """hnr_resize_coeffs for one axis -> (ksize, bounds [n_out,2] int32, coef [n_out,ksize] int32), NumPy arrays on the host; Pillow's own integers
    (tests/resize_ref.py).  Cached per (n_in, n_out, filter): a host function, no GPU is needed."""
    if filter not in _lib.RESIZE_FILTERS:
        raise HnrError("resize: filter must be one of %s, got %r (NEAREST is not a convolution filter and is not supported)" % (sorted(_lib.RESIZE_FILTERS), filter))
    key = (int(n_in), int(n_out), _lib.RESIZE_FILTERS[filter])
    t = _TABLES.get(key)
    if t is None:
        if key[0] < 1 or key[1] < 1:
            raise HnrError("resize: sizes must be >= 1, got %d -> %d" % key[:2])
        ksize = _lib.size("hnr_resize_coeffs", key[0], key[1], key[2], None, None, 0)
        bounds, coef = np.empty((key[1], 2), np.int32), np.empty((key[1], ksize), np.int32)
        _lib.size("hnr_resize_coeffs", key[0], key[1], key[2], bounds.ctypes.data_as(ctypes.c_void_p), coef.ctypes.data_as(ctypes.c_void_p), coef.size)
        if len(_TABLES) > 64:
            _TABLES.clear()
        _TABLES[key] = t = (int(ksize), bounds, coef)
    return t


def _device_tables(n_in, n_out, filter, device):
    """the tables of one axis on `device` (uploaded once per device and key): (ksize, bounds, coef)"""
    ksize, bounds, coef = resize_tables(n_in, n_out, filter)
    key = (str(device), int(n_in), int(n_out), filter)
    t = _DEV_TABLES.get(key)
    if t is None:
        if len(_DEV_TABLES) > 64:
            _DEV_TABLES.clear()
        # (uploaded on whatever stream is current and read from any stream afterwards with no event: safe because .to() of pageable host
        # memory returns only when the copy is done)
        _DEV_TABLES[key] = t = (ksize, torch.from_numpy(bounds).to(device), torch.from_numpy(coef).to(device))
    return t


def _raw_frames(raw, what):
    """[N,h,w,C] or [h,w,C] uint8, NumPy or torch, host or device -> (a torch tensor [N,h,w,C] where it is, whether a frame dimension was added)"""
    t = raw
    if isinstance(raw, np.ndarray):
        with warnings.catch_warnings():                       # np.asarray(PIL image) is read-only; the tensor is only ever read
            warnings.simplefilter("ignore", UserWarning)
            t = torch.from_numpy(np.ascontiguousarray(raw))
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
        raise HnrError("%s: frames must be uint8 (NumPy or torch), got %s" % (what, getattr(raw, "dtype", type(raw).__name__)))
    if t.dim() not in (3, 4):
        raise HnrError("%s: frames must be [N,h,w,C] or [h,w,C], got %s" % (what, tuple(t.shape)))
    single = t.dim() == 3
    t = t[None] if single else t
    if int(t.shape[3]) not in (1, 3, 4):
        raise HnrError("%s: C must be 1, 3 or 4, got %d" % (what, int(t.shape[3])))
    if min(int(s) for s in t.shape[:3]) < 1:
        raise HnrError("%s: sizes must be >= 1, got %s" % (what, tuple(t.shape)))
    return t, single


def resize_form(raw_hw, size, channels=3, filter="lanczos"):
    """Which form hnr_resize_u8 takes with form="auto" for frames of raw_hw = (h, w) -> size = (W, H): "fused" or "two_pass" (host only)."""
    (h, w), (W, H) = (int(v) for v in raw_hw), (int(v) for v in size)
    if min(h, w, H, W) < 1:
        raise HnrError("resize_form: sizes must be >= 1")
    kh = resize_tables(w, W, filter)[0] if w != W else 0
    kv = resize_tables(h, H, filter)[0] if h != H else 0
    return "fused" if _lib.size("hnr_resize_u8_form", h, w, int(channels), H, W, kh, kv) == 1 else "two_pass"


def resize_frames(raw, size, filter="lanczos", mode=None, out=None, form="auto", device=None):
    """PIL.Image.resize(size, filter) of every frame, on the device, the same bytes (hnr_resize_u8; definitions in include/hnr.h, restated in
    tests/resize_ref.py).  raw: [N,h,w,C] or [h,w,C] uint8, C = 1, 3 or 4, NumPy or torch, on the host (uploaded as it is) or on the device;
    size = (W, H) as Pillow orders it; filter "box" | "bilinear" | "hamming" | "bicubic" | "lanczos".  mode="RGBA": what Pillow does to a
    mode-RGBA image -- premultiply, resize, un-premultiply (the input is not modified); a same-size RGBA frame is a plain copy, as Pillow's.  Returns, or fills, a device uint8 tensor [N,H,W,C]
    ([H,W,C] for one frame): `out` may be rows of a bank.  form "auto" | "fused" | "two_pass" (same bytes).  The device is raw's, else out's, else
    `device`, else the current GPU.  Decoding (JPEG / PNG) stays the caller's; Pillow's box= and reducing_gap= are not covered."""
    what = "resize_frames"
    src, single = _raw_frames(raw, what)
    try:
        W, H = (int(v) for v in size)
    except (TypeError, ValueError):
        raise HnrError("%s: size must be (W, H), got %r" % (what, size))
    if W < 1 or H < 1:
        raise HnrError("%s: size must be >= 1, got %r" % (what, (W, H)))
    if form not in _lib.RESIZE_FORMS:
        raise HnrError("%s: form must be one of %s, got %r" % (what, sorted(_lib.RESIZE_FORMS), form))
    N, h, w, C = (int(s) for s in src.shape)
    if mode not in (None, "L", "RGB", "RGBA") or (mode is not None and len(mode) != C):
        raise HnrError("%s: mode %r does not fit %d channels (None, 'L', 'RGB' or 'RGBA'; 'RGBA' needs four)" % (what, mode, C))
    if filter not in _lib.RESIZE_FILTERS:
        raise HnrError("%s: filter must be one of %s, got %r" % (what, sorted(_lib.RESIZE_FILTERS), filter))
    if src.is_cuda:
        dev = src.device
    elif out is not None and isinstance(out, torch.Tensor):
        dev = out.device
    elif device is not None:
        dev = torch.device(device)
    else:
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    if dev.type != "cuda":
        raise HnrError("%s: the device must be a GPU (the HIP path has no CPU fallback)" % what)
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != torch.uint8 or not out.is_contiguous() or \
                tuple(out.shape) not in ((N, H, W, C),) + (((H, W, C),) if N == 1 else ()):
            raise HnrError("%s: out must be a contiguous uint8 tensor [%d,%d,%d,%d] on %s" % (what, N, H, W, C, dev))
    else:
        out = torch.empty((N, H, W, C), dtype=torch.uint8, device=dev)
    own = not src.is_cuda
    src = src.to(dev).contiguous()
    kh, bh, ch = _device_tables(w, W, filter, dev) if w != W else (0, None, None)
    kv, bv, cv = _device_tables(h, H, filter, dev) if h != H else (0, None, None)
    rgba = mode == "RGBA" and (w != W or h != H)        # Image.resize returns a copy of a same-size image BEFORE it converts RGBA -> RGBa
    if rgba:
        pre = src if own else torch.empty_like(src)
        _lib.call("hnr_rgba_premultiply", src, pre, N * h * w, _lib.STREAM)
        src = pre
    scratch = None
    if form == "two_pass" or (form == "auto" and _lib.size("hnr_resize_u8_form", h, w, C, H, W, kh, kv) == 2):
        scratch = torch.empty((max(_lib.size("hnr_resize_u8_scratch_bytes", N, h, w, C, H, W), 16),), dtype=torch.uint8, device=dev)
    _lib.call("hnr_resize_u8", src, N, h, w, C, out, H, W, bh, ch, kh, bv, cv, kv, _lib.RESIZE_FORMS[form], scratch,
              0 if scratch is None else int(scratch.numel()), _lib.STREAM)
    if rgba:
        _lib.call("hnr_rgba_unpremultiply", out, out, N * H * W, _lib.STREAM)
    mark_written([out])
    return out[0] if single and out.dim() == 4 else out


def compose_rgba(rgba8, white=True, black=False, alpha=True, mask=False):
    """nerf_synth360_ft_dataset.py:532-536 on resized RGBA frames (hnr_rgba_compose): rgba8 [N,H,W,4] (or [H,W,4]) uint8 on the device -> a dict of
    the float32 tensors asked for: "white" = c a + (1 - a) and "black" = c a [N,H,W,3] (what a FrameBank holds for a synthetic scene), "alpha" = a
    and "mask" = (a > 0.1) [N,H,W] (what cloud_init.AlphaMasks / alpha_masking take), c, a = u8 / 255.  The bits of the torch expressions on the CPU."""
    t, single = _raw_frames(rgba8, "compose_rgba")
    if not t.is_cuda:
        raise HnrError("compose_rgba: rgba8 must be on the GPU (the HIP path has no CPU fallback)")
    if int(t.shape[3]) != 4:
        raise HnrError("compose_rgba: rgba8 must have four channels, got %d" % int(t.shape[3]))
    if not (white or black or alpha or mask):
        raise HnrError("compose_rgba: no output asked for")
    t = t.contiguous()
    N, H, W = (int(s) for s in t.shape[:3])
    f = lambda *s: torch.empty(s, dtype=torch.float32, device=t.device)
    res = {}
    if white:
        res["white"] = f(N, H, W, 3)
    if black:
        res["black"] = f(N, H, W, 3)
    if alpha:
        res["alpha"] = f(N, H, W)
    if mask:
        res["mask"] = f(N, H, W)
    _lib.call("hnr_rgba_compose", t, N * H * W, res.get("white"), res.get("black"), res.get("alpha"), res.get("mask"), _lib.STREAM)
    return {k: v[0] for k, v in res.items()} if single else res


def scaled_intrinsic(intrinsic_raw, raw_wh, wh):
    """data/scannet_ft_dataset.py:178-179: the raw frames' intrinsic for frames resized from raw_wh = (w, h) to wh = (W, H) -- row 0 times W / w,
    row 1 times H / h, the float32 array times a Python float.  [3,3] or [F,3,3]; the input is not modified."""
    K = np.array(intrinsic_raw.detach().cpu() if isinstance(intrinsic_raw, torch.Tensor) else intrinsic_raw, dtype=np.float32)
    if K.shape[-2:] != (3, 3) or K.ndim not in (2, 3):
        raise HnrError("scaled_intrinsic: the intrinsic must be [3,3] or [F,3,3], got %s" % (K.shape,))
    K[..., 0, :] *= (wh[0] / raw_wh[0])
    K[..., 1, :] *= (wh[1] / raw_wh[1])
    return K


class FrameBank:
    """All frames of one split on the device: images [F,H,W,3] uint8 (stored as they are) or float32, c2w [F,4,4], w2c = torch.inverse(c2w) (computed
    once, on the device), intrinsic [3,3] shared or [F,3,3], weight[f] = float32(weights[f] ** weight_exp) (float64 arithmetic, as
    scannet_ft_dataset.py:758; ones without weights) and angle[f] = float32(ids[f] / total_num_image * 2 pi) (:830).  `ids`: the frames' vids
    (default 0..F-1); total_num_image defaults to max(ids) + 1.

    depth (optional): the split's sensor depth frames [F,Hd,Wd], stored as given -- raw uint16 (a NumPy uint16 array, or torch.int16 carrying the
    uint16 bit pattern, cloud_init.DepthFusion's convention: a negative value v means 65536 + v) divided by `depth_div` when read, or float32 metres.
    A value outside [depth_min, depth_max] reads as 0 = no measurement.  depth_intrinsic [3,3]: the depth camera's intrinsic when the depth frames
    have another size or calibration than the colour frames; without it (Hd,Wd) must equal (H,W) and a ray reads the texel gt_image reads.  With
    depth the samplers of this bank emit `gt_depth` [R] (hnr_frame_depth_rays; the definitions are in include/hnr.h and tests/depth_sup_ref.py)."""

    def __init__(self, images, c2w, intrinsic, device, ids=None, weights=None, weight_exp=1.0, total_num_image=None, depth=None, depth_div=1000.,
                 depth_min=0.3, depth_max=8.0, depth_intrinsic=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise HnrError("FrameBank: device must be a GPU (the HIP path has no CPU fallback)")
        images = torch.from_numpy(np.ascontiguousarray(images)) if isinstance(images, np.ndarray) else images
        if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.shape[3] != 3 or images.dtype not in (torch.uint8, torch.float32):
            raise HnrError("FrameBank: images must be [F,H,W,3] uint8 or float32")
        F, H, W = (int(s) for s in images.shape[:3])
        if F < 1 or H < 1 or W < 1 or H * W > (1 << 26):
            raise HnrError("FrameBank: F, H, W >= 1 and H * W <= 2^26")
        self.F, self.H, self.W = F, H, W
        depth, Kd = self._check_depth(depth, depth_div, depth_min, depth_max, depth_intrinsic)     # (before anything is uploaded)
        self.images = images.to(self.device).contiguous()
        c2w = torch.as_tensor(np.asarray(c2w.detach().cpu() if isinstance(c2w, torch.Tensor) else c2w, dtype=np.float32))
        if tuple(c2w.shape) != (F, 4, 4):
            raise HnrError("FrameBank: c2w must be [%d,4,4], got %s" % (F, tuple(c2w.shape)))
        self.c2w = c2w.to(self.device).contiguous()
        self.w2c = torch.inverse(self.c2w).contiguous()
        K = torch.as_tensor(np.asarray(intrinsic.detach().cpu() if isinstance(intrinsic, torch.Tensor) else intrinsic, dtype=np.float32))
        if tuple(K.shape) not in ((3, 3), (F, 3, 3)):
            raise HnrError("FrameBank: intrinsic must be [3,3] or [%d,3,3], got %s" % (F, tuple(K.shape)))
        self.intrinsic = K.to(self.device).contiguous()
        self.ids = np.arange(F) if ids is None else np.asarray(ids).reshape(-1)
        if self.ids.shape[0] != F:
            raise HnrError("FrameBank: %d ids for %d frames" % (self.ids.shape[0], F))
        total = int(self.ids.max()) + 1 if total_num_image is None else total_num_image
        if not total > 0:
            raise HnrError("FrameBank: total_num_image must be positive")
        if weights is None:
            w = np.ones((F,), np.float32)
        else:
            if len(weights) != F:
                raise HnrError("FrameBank: %d weights for %d frames" % (len(weights), F))
            w = np.array([np.float32(float(x) ** float(weight_exp)) for x in weights], dtype=np.float32)
        ang = np.array([np.float32((float(i) / float(total)) * 2 * np.pi) for i in self.ids], dtype=np.float32)
        self.weight, self.angle = torch.from_numpy(w).to(self.device), torch.from_numpy(ang).to(self.device)
        self.nearest, self.reference, self.V = None, self, 0
        self._c = _lib.FrameBankC(_lib.ptr(self.images), _lib.ptr(self.c2w), _lib.ptr(self.w2c), _lib.ptr(self.intrinsic), _lib.ptr(self.weight),
                                  _lib.ptr(self.angle), 1 if self.images.dtype == torch.float32 else 0, F, H, W, 1 if K.dim() == 3 else 0)
        self.depth = self.depth_intrinsic = self._dc = None
        if depth is not None:
            self.depth = depth.to(self.device).contiguous()
            self.depth_intrinsic = None if Kd is None else Kd.to(self.device).contiguous()
            self.depth_div, self.depth_min, self.depth_max = float(depth_div), float(depth_min), float(depth_max)
            self._dc = _lib.DepthBankC(_lib.ptr(self.depth), _lib.ptr(self.depth_intrinsic), 1 if self.depth.dtype == torch.float32 else 0, F,
                                       int(self.depth.shape[1]), int(self.depth.shape[2]), self.depth_div, self.depth_min, self.depth_max)

    def _check_depth(self, depth, depth_div, depth_min, depth_max, depth_intrinsic):
        """The depth arguments, validated before any upload -> (depth tensor as given or None, depth intrinsic [3,3] CPU tensor or None)."""
        if depth is None:
            if depth_intrinsic is not None:
                raise HnrError("FrameBank: depth_intrinsic without depth")
            return None, None
        if isinstance(depth, np.ndarray):
            if depth.dtype == np.uint16:                   # torch has no uint16 arithmetic: the bytes travel as int16, the kernel reads uint16
                depth = np.ascontiguousarray(depth).view(np.int16)
            if depth.dtype not in (np.int16, np.float32):
                raise HnrError("FrameBank: depth must be uint16 (raw) or float32 (metres), got %s" % depth.dtype)
            depth = torch.from_numpy(np.ascontiguousarray(depth))
        if not isinstance(depth, torch.Tensor) or depth.dtype not in (torch.int16, torch.float32):
            raise HnrError("FrameBank: depth must be uint16 (raw; torch.int16 with the uint16 bit pattern) or float32 (metres), got %s"
                           % getattr(depth, "dtype", type(depth)))
        if depth.dim() != 3 or int(depth.shape[0]) != self.F or int(depth.shape[1]) < 1 or int(depth.shape[2]) < 1 or \
                int(depth.shape[1]) * int(depth.shape[2]) > (1 << 26):
            raise HnrError("FrameBank: depth must be [%d,Hd,Wd] (one frame per image, Hd * Wd <= 2^26), got %s" % (self.F, tuple(depth.shape)))
        if depth.is_cuda and depth.device != self.device:
            raise HnrError("FrameBank: depth is on %s, the bank on %s" % (depth.device, self.device))
        if not (float(depth_div) > 0 and float(depth_min) <= float(depth_max)):
            raise HnrError("FrameBank: depth_div > 0 and depth_min <= depth_max")
        Kd = None
        if depth_intrinsic is not None:
            Kd = torch.as_tensor(np.asarray(depth_intrinsic.detach().cpu() if isinstance(depth_intrinsic, torch.Tensor) else depth_intrinsic, dtype=np.float32))
            if tuple(Kd.shape) != (3, 3):
                raise HnrError("FrameBank: depth_intrinsic must be [3,3], got %s" % (tuple(Kd.shape),))
        elif (int(depth.shape[1]), int(depth.shape[2])) != (self.H, self.W):
            raise HnrError("FrameBank: depth frames of %dx%d for colour frames of %dx%d need depth_intrinsic" % (int(depth.shape[1]), int(depth.shape[2]), self.H, self.W))
        return depth, Kd

    def set_nearest(self, table, reference=None):
        """table [F,V] int32: the rows of every frame's nearest reference frames in `reference` (default: this bank; a test-set bank names its
        train-set bank)."""
        ref = self if reference is None else reference
        if not isinstance(ref, FrameBank) or ref.device != self.device or (ref.H, ref.W) != (self.H, self.W):
            raise HnrError("FrameBank.set_nearest: the reference must be a FrameBank on the same device with the same frame size")
        t = np.asarray(table.detach().cpu() if isinstance(table, torch.Tensor) else table)
        if t.ndim != 2 or t.shape[0] != self.F or t.shape[1] < 1 or t.shape[1] > 64 or not np.issubdtype(t.dtype, np.integer):
            raise HnrError("FrameBank.set_nearest: the table must be integer [%d,V], 1 <= V <= 64, got %s %s" % (self.F, t.dtype, t.shape))
        if t.min() < 0 or t.max() >= ref.F:
            raise HnrError("FrameBank.set_nearest: a nearest row is outside the reference bank (0 .. %d)" % (ref.F - 1))
        self.nearest = torch.from_numpy(np.ascontiguousarray(t, dtype=np.int32)).to(self.device)
        self.reference, self.V = ref, int(t.shape[1])
        return self

    @classmethod
    def from_raw(cls, raw_images, c2w, intrinsic_raw, size, device, filter="lanczos", chunk=16, form="auto", **kwargs):
        """A uint8 bank from the frames as decoded: what `Image.open(...).resize(size, Image.LANCZOS)` per frame and the scaling of the intrinsic
        (scannet_ft_dataset.py:178-179, 742) give, with the resize on the device.  raw_images: [F,h,w,3] uint8 (NumPy or torch, host or device) or
        a sequence of [h,w,3] frames of one size; size = (W, H); intrinsic_raw: the RAW frames' intrinsic, [3,3] or [F,3,3].  The bank's image
        tensor is allocated once; the raw frames go through in chunks of `chunk` -- host -> device copy, then hnr_resize_u8 straight into the
        bank's rows -- so the device never holds the raw set.  Everything else (ids, weights, depth, ...) is the constructor's."""
        dev = torch.device(device)
        if dev.type != "cuda":
            raise HnrError("FrameBank.from_raw: device must be a GPU (the HIP path has no CPU fallback)")
        try:
            W, H = (int(v) for v in size)
        except (TypeError, ValueError):
            raise HnrError("FrameBank.from_raw: size must be (W, H), got %r" % (size,))
        chunk = int(chunk)
        if W < 1 or H < 1 or chunk < 1:
            raise HnrError("FrameBank.from_raw: size and chunk must be >= 1")
        seq = isinstance(raw_images, (list, tuple))
        F = len(raw_images) if seq else (int(raw_images.shape[0]) if getattr(raw_images, "ndim", 0) == 4 else 0)
        if F < 1:
            raise HnrError("FrameBank.from_raw: raw_images must be [F,h,w,3] or a non-empty sequence of [h,w,3] frames")
        first = raw_images[0]
        if getattr(first, "ndim", 0) != 3 or int(first.shape[2]) != 3:
            raise HnrError("FrameBank.from_raw: frames must be [h,w,3], got %s" % (tuple(getattr(first, "shape", ())),))
        h_raw, w_raw = int(first.shape[0]), int(first.shape[1])
        K = scaled_intrinsic(intrinsic_raw, (w_raw, h_raw), (W, H))
        images = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
        for i in range(0, F, chunk):
            part = raw_images[i:i + chunk]
            if seq:
                if len({tuple(p.shape) for p in part}) != 1:
                    raise HnrError("FrameBank.from_raw: frames %d .. %d are not of one size" % (i, i + len(part) - 1))
                part = torch.stack(list(part)) if isinstance(part[0], torch.Tensor) else np.stack([np.asarray(p) for p in part])
            if tuple(part.shape[1:]) != (h_raw, w_raw, 3):
                raise HnrError("FrameBank.from_raw: frames %d .. are %s, the first frame is %s" % (i, tuple(part.shape[1:]), (h_raw, w_raw, 3)))
            resize_frames(part, (W, H), filter=filter, out=images[i:i + int(part.shape[0])], form=form, device=dev)
        return cls(images, c2w, K, dev, **kwargs)

    def ingest(self, rows, raw, filter="lanczos", form="auto"):
        """Replaces rows of a uint8 bank with raw frames resized to the bank's size (a caller that decodes one frame at a time): rows an int or a
        list of ints, raw [h,w,3] or [n,h,w,3] uint8, one frame per row.  The same kernels as from_raw; poses and intrinsics stay as they are."""
        if self.images.dtype != torch.uint8:
            raise HnrError("FrameBank.ingest: the bank holds float32 images; only a uint8 bank takes raw frames")
        src, _ = _raw_frames(raw, "FrameBank.ingest")
        rows = [int(r) for r in np.asarray(rows).reshape(-1)]
        if len(rows) != int(src.shape[0]) or int(src.shape[3]) != 3:
            raise HnrError("FrameBank.ingest: %d rows for frames of shape %s ([n,h,w,3], one per row)" % (len(rows), tuple(src.shape)))
        if not rows:
            raise HnrError("FrameBank.ingest: no rows given")
        if min(rows) < 0 or max(rows) >= self.F:
            raise HnrError("FrameBank.ingest: a row is outside the bank (0 .. %d)" % (self.F - 1))
        if src.is_cuda and src.device != self.device:
            raise HnrError("FrameBank.ingest: raw is on %s, the bank on %s" % (src.device, self.device))
        i = 0
        while i < len(rows):                                   # runs of consecutive rows go in one call
            j = i + 1
            while j < len(rows) and rows[j] == rows[j - 1] + 1:
                j += 1
            resize_frames(src[i:j], (self.W, self.H), filter=filter, out=self.images[rows[i]:rows[i] + (j - i)], form=form, device=self.device)
            i = j
        return self


class _Sampler:
    """What BatchSampler and PathSampler share: the checks of the margin, the background colour and the output tensors, the item's host-side keys,
    and where next() writes.  A subclass has `bank`, `margin`, `near`, `far`, `_static = None`, `_bound = {}`, `_shapes()` (name -> (shape, dtype)
    of next()'s outputs), `_alloc()` (those tensors) and `_bind(tensors, what)`."""

    def _check_margin(self):
        H, W, m = self.bank.H, self.bank.W, self.margin
        if m < 0 or W - 2 * m <= 0 or H - 2 * m <= 0:
            raise HnrError("%s: margin %d leaves no pixel of a %dx%d frame (an empty range)" % (type(self).__name__, m, H, W))

    def _triple(self, bg_color):
        bg = tuple(float(c) for c in bg_color)
        if len(bg) != 3:
            raise HnrError("%s: bg_color must have three components" % type(self).__name__)
        return bg

    def _finish(self, t):
        d = dict(t)
        d["camrotc2w"] = d["camrot"]
        d.update(near=self.near, far=self.far, h=self.bank.H, w=self.bank.W)
        return d

    def _bind_outputs(self, tensors, sh, what):
        """name -> tensor  =>  hnr_frame_batch_out; every tensor that is an output (a name of `sh`) checked against the expected element count and
        dtype.  (gt_depth is no field of the struct: BatchSampler hands it to the depth launch.)"""
        o = _lib.FrameBatchOut()
        for k, t in tensors.items():
            if k not in sh:
                continue
            shape, dt = sh[k]
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != self.bank.device or t.dtype != dt or not t.is_contiguous() or \
                    t.numel() != int(np.prod(shape)):
                raise HnrError("%s: output %r must be a contiguous %s tensor of %s on %s, got %s %s" % (
                    what, k, dt, "x".join(str(s) for s in shape), self.bank.device, getattr(t, "dtype", type(t)), tuple(getattr(t, "shape", ()))))
            if k == "images_nearest" and t.data_ptr() % 16:
                raise HnrError("%s: images_nearest must be 16-byte aligned" % what)
            if k != "gt_depth":
                setattr(o, "d_" + k, t.data_ptr())
        return o

    def _next_outputs(self, out):
        """Where next(out) writes: (the dict it returns, what _bind made of its tensors).  out=None: the sampler's own static tensors, allocated and
        bound on the first call.  out = a dict: bound once per set of tensors (the bound image holds addresses, so address, size and dtype are its
        whole key).  The launches that follow write these tensors behind torch's back, at the same addresses call after call: rule 3 of _cache.py."""
        what = type(self).__name__ + ".next"
        if out is None:
            if self._static is None:
                t = self._alloc()
                self._static = (self._finish(t), self._bind(t, what))
            res, bound = self._static
        else:
            key = tuple((k, v.data_ptr(), v.numel(), v.dtype) for k, v in out.items() if isinstance(v, torch.Tensor))
            bound = self._bound.get(key)
            if bound is None:                                 # shapes and dtypes are checked once per set of tensors
                t = {k: v for k, v in out.items() if isinstance(v, torch.Tensor)}
                if "camrotc2w" in t:
                    if "camrot" in t and t["camrot"].data_ptr() != t["camrotc2w"].data_ptr():
                        raise HnrError("%s: out has both camrot and camrotc2w, and they are different tensors" % what)
                    t["camrot"] = t.pop("camrotc2w")
                if len(self._bound) > 16:
                    self._bound.clear()
                bound = self._bound[key] = self._bind(t, what)
            res = out
        sh = self._shapes()
        mark_written(v for k, v in res.items() if (k in sh or k == "camrotc2w") and isinstance(v, torch.Tensor))
        return res, bound


class BatchSampler(_Sampler):
    """The dataset item of every step, written on the device.

    mode "random" | "patch" (size x size rays) | "dilated" (dilation_setup "pn_ps_dlo_dhi": (pn ps)^2 rays in the layout of scenes.dilated_patch_batch and
    the blur module's "grid"); margin = opt.edge_filter; bg_color a triple or "random"; the definitions are in include/hnr.h and tests/frames_ref.py.
    `set_schedule(rows)` uploads the bank rows to visit (an epoch's permutation), used cyclically; `next()` writes the batch of step `step` -- the
    frame is schedule[step % len] -- and advances `step` on the device.  It returns the same static tensors on every call, allocates nothing after
    the first call, reads nothing back and is at most three launches on the current stream (capturable with torch.cuda.graph on one stream).
    `item(row, pixels=None)` is the explicit form without a counter (evaluation frames; fresh tensors).

    The dict has the dataset item's keys: raydir [R,3], pixel_idx [R,2] float32 (x, y), gt_image [R,3]; campos [3], camrotc2w = camrot [3,3], c2w [4,4],
    intrinsic [3,3]; c2w_nearest, w2c_nearest [V,4,4], campos_nearest [V,3], intrinsic_nearest [3,3], images_nearest [V,H,W,3] float32,
    frame_weight_nearest [V], vid_angle_nearest [V]; frame_weight [1] (device), bg_color [3], near, far, h, w; frame_row [1] int32 and, for
    patch / dilated, patch_table [pn^2,3] int32 (d, x0, y0).  A bank with depth frames adds gt_depth [R] float32 (metres, 0 = no measurement): one
    more launch behind the three, hnr_frame_depth_rays, which reads the frame row and the pixels the batch kernels just wrote -- still capturable;
    `next(out=...)` writes it when `out` holds that key.

    Both patch modes feed the patch SSIM term of train.train_step(w_ssim=) / losses.ssim_patch_loss: "dilated" with patch_num = pn, patch_size = ps
    (7 <= ps <= 64), "patch" as ONE size x size patch (patch_num = 1, patch_size = size <= 64) -- the sampler's `pn`, `ps` attributes, layout "grid".
    A "random" batch has no patches and the term raises for it."""

    def __init__(self, bank, mode, size=None, dilation_setup=None, margin=0, seed=0, dir_norm=0, bg_color=(1, 1, 1), near=None, far=None,
                 downweight_blurry_feats=0):
        if not isinstance(bank, FrameBank):
            raise HnrError("BatchSampler: bank must be a FrameBank")
        if mode not in MODES:
            raise HnrError("BatchSampler: mode must be one of %s (random2, proportional_random and dynamic_nearest are not supported)" % sorted(MODES))
        if near is None or far is None:
            raise HnrError("BatchSampler: near and far (the item's depth range) are required")
        self.bank, self.mode, self.margin = bank, mode, int(margin)
        self.near, self.far = float(near), float(far)
        H, W, m = bank.H, bank.W, self.margin
        self._check_margin()
        pn = ps = dlo = dhi = 0
        if mode == "dilated":
            try:
                pn, ps, dlo, dhi = (int(float(x)) for x in str(dilation_setup).split("_"))
            except ValueError:
                raise HnrError("BatchSampler: dilation_setup must be 'pn_ps_dlo_dhi', got %r" % (dilation_setup,))
            if pn < 1 or ps < 1 or dlo < 1 or dhi < dlo or pn * ps > 8192:
                raise HnrError("BatchSampler: dilation_setup %r: pn, ps >= 1, 1 <= dlo <= dhi" % (dilation_setup,))
            reach, S = (ps - 1) * dhi, pn * ps
        else:
            if size is None or int(size) < 1 or int(size) > 8192:
                raise HnrError("BatchSampler: mode %r needs 1 <= size <= 8192" % mode)
            S = int(size)
            reach = S - 1 if mode == "patch" else 0
        if mode != "random" and (W - m - reach <= m or H - m - reach <= m):
            raise HnrError("BatchSampler: a patch reaching %d pixels does not fit a %dx%d frame with margin %d (size larger than the frame: an empty range)"
                           % (reach + 1, H, W, m))
        self.S, self.R, self.pn, self.ps = S, S * S, (1 if mode == "patch" else pn), (S if mode == "patch" else ps)
        bg_random = isinstance(bg_color, str)
        if bg_random and bg_color != "random":
            raise HnrError("BatchSampler: bg_color must be a triple or 'random'")
        self.bg = (1.0, 1.0, 1.0) if bg_random else self._triple(bg_color)
        self.dir_norm, self.downweight = int(bool(dir_norm)), int(bool(downweight_blurry_feats))
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.seed = seed
        self.prm = _lib.FrameBatchParams(MODES[mode], S, pn, ps, dlo, dhi, m, self.dir_norm, int(bg_random), self.downweight, (ctypes.c_float * 3)(*self.bg), seed)
        dev = bank.device
        nbytes = _lib.size("hnr_frame_batch_scratch_bytes", MODES[mode], pn, what="BatchSampler: unsupported mode / patch count")
        self._scratch = torch.zeros((max(nbytes, 16),), dtype=torch.uint8, device=dev)
        self._item_scratch = torch.zeros((16,), dtype=torch.uint8, device=dev)
        self.step = torch.zeros((1,), dtype=torch.int64, device=dev)          # the step counter (read and advanced by the header kernel)
        self.schedule, self._n_schedule = None, 0
        self._static, self._bound, self._own = None, {}, {}

    # ------------------------------------------------------------------------------------------------ plumbing
    def _shapes(self, R=None):
        """R: the item's ray count (default: next()'s)"""
        b, R = self.bank, self.R if R is None else R
        V, H, W = b.V, b.H, b.W
        f, i = torch.float32, torch.int32
        sh = dict(raydir=((R, 3), f), pixel_idx=((R, 2), f), gt_image=((R, 3), f), campos=((3,), f), camrot=((3, 3), f), c2w=((4, 4), f), intrinsic=((3, 3), f),
                  frame_weight=((1,), f), bg_color=((3,), f), frame_row=((1,), i))
        if b._dc is not None:
            sh["gt_depth"] = ((R,), f)
        if V > 0:
            sh.update(c2w_nearest=((V, 4, 4), f), w2c_nearest=((V, 4, 4), f), campos_nearest=((V, 3), f), intrinsic_nearest=((3, 3), f),
                      images_nearest=((V, H, W, 3), f), frame_weight_nearest=((V,), f), vid_angle_nearest=((V,), f))
        if self.mode != "random" and R == self.R:
            sh["patch_table"] = ((self.pn * self.pn, 3), i)
        return sh

    def _alloc(self, R=None):
        """next()'s tensors, or, R given, those of an item of R rays (no patch_table)"""
        return {k: torch.empty(s, dtype=d, device=self.bank.device) for k, (s, d) in self._shapes(R).items() if R is None or k != "patch_table"}

    def _bind(self, tensors, what, R=None):
        """name -> tensor  =>  (hnr_frame_batch_out, the depth launch's tensors or None); every tensor checked against the expected element count
        and dtype.  gt_depth among the tensors: the lookup reads the item's frame_row, pixel_idx (and intrinsic, with a depth intrinsic) from the
        device, so outputs of those names that the caller did not give are bound to tensors of the sampler's own (allocated here, once per R)."""
        R = self.R if R is None else R
        sh = self._shapes(R)
        dep = None
        if "gt_depth" in sh and "gt_depth" in tensors:
            tensors = dict(tensors)
            for k in ("frame_row", "pixel_idx") + (("intrinsic",) if self.bank.depth_intrinsic is not None else ()):
                if k not in tensors:
                    if (k, R) not in self._own:
                        self._own[(k, R)] = torch.empty(sh[k][0], dtype=sh[k][1], device=self.bank.device)
                    tensors[k] = self._own[(k, R)]
            dep = (tensors["frame_row"], tensors["pixel_idx"], tensors.get("intrinsic"), tensors["gt_depth"])
        return self._bind_outputs(tensors, sh, what), dep

    def _depth_rays(self, dep, R):
        """gt_depth of the item just written: one launch behind the batch's, reading its frame_row / pixel_idx on the device"""
        row, pix, K, gt = dep
        _lib.call("hnr_frame_depth_rays", self.bank._dc, row, pix, K if self.bank.depth_intrinsic is not None else None, R, gt, _lib.STREAM)

    def _views(self):
        b = self.bank
        return (b.reference._c if b.V > 0 else None), (b.nearest if b.V > 0 else None), b.V

    # ------------------------------------------------------------------------------------------------ the interface
    def set_schedule(self, rows):
        """rows: the bank rows to visit, in order (an epoch's permutation); uploaded once, used cyclically.  The step counter keeps its value."""
        r = np.asarray(rows.detach().cpu() if isinstance(rows, torch.Tensor) else rows).reshape(-1)
        if r.size < 1 or r.size >= (1 << 31) or not np.issubdtype(r.dtype, np.integer):
            raise HnrError("BatchSampler.set_schedule: a non-empty list of integer bank rows")
        if r.min() < 0 or r.max() >= self.bank.F:
            raise HnrError("BatchSampler.set_schedule: a row is outside the bank (0 .. %d)" % (self.bank.F - 1))
        self.schedule, self._n_schedule = torch.from_numpy(np.ascontiguousarray(r, dtype=np.int32)).to(self.bank.device), int(r.size)
        return self

    def set_step(self, step):
        """Sets the device step counter (a host -> device fill; resuming a run)."""
        self.step.fill_(int(step))
        return self

    def next(self, out=None):
        """The batch of step `step`; step += 1 on the device.  out=None: the sampler's own static tensors (the same on every call).  out = a dict: the
        outputs whose keys are present in it ("camrot" or "camrotc2w" for the rotation) are written into those tensors and no others are touched
        -- `sampler.next(out=cap.inputs); cap.step()` is a training step with no copy and no host read.  Returns the dict written to."""
        if self.schedule is None:
            raise HnrError("BatchSampler.next: no schedule (set_schedule(rows) first)")
        res, (o, dep) = self._next_outputs(out)
        ref, nearest, V = self._views()
        _lib.call("hnr_frame_batch", self.bank._c, ref, nearest, V, self.prm, self.schedule, self._n_schedule, self.step, o, self._scratch,
                  int(self._scratch.numel()), _lib.STREAM)
        if dep is not None:
            self._depth_rays(dep, self.R)
        return res

    def item(self, row, pixels=None):
        """The item of bank row `row` with no counter: every pixel minus `margin` in scan-line order ('no_crop', scannet_ft_dataset.py:946-949), or the
        given pixel_idx [R,2] float32 (x, y; fractional pixels truncate for gt_image).  bg_color "random" gives white here."""
        row = int(row)
        if row < 0 or row >= self.bank.F:
            raise HnrError("BatchSampler.item: row %d is outside the bank (0 .. %d)" % (row, self.bank.F - 1))
        dev = self.bank.device
        if pixels is not None:
            pixels = torch.as_tensor(pixels, dtype=torch.float32).to(dev).reshape(-1, 2).contiguous()
            R = int(pixels.shape[0])
            if R < 1:
                raise HnrError("BatchSampler.item: pixels must be [R,2], R >= 1")
        else:
            R = (self.bank.W - 2 * self.margin) * (self.bank.H - 2 * self.margin)
        t = self._alloc(R)
        o, dep = self._bind(t, "BatchSampler.item", R)
        ref, nearest, V = self._views()
        _lib.call("hnr_frame_item", self.bank._c, ref, nearest, V, row, pixels, R, self.margin, self.dir_norm, (ctypes.c_float * 3)(*self.bg),
                  self.downweight, o, self._item_scratch, 16, _lib.STREAM)
        if dep is not None:
            self._depth_rays(dep, R)                      # (the row travels through the item's own frame_row word on the device)
        return self._finish(t)


class PathSampler(_Sampler):
    """The dataset item of a camera that is no row of a bank: frame i of a pose table, with the reference views chosen on the device (csrc/path.hip;
    the definitions are in include/hnr.h and tests/path_ref.py).

    poses [P,4,4] c2w (paths.spherical_path / paths.keyframe_path, or any array; a torch tensor must already be on the bank's device) and
    intrinsic [3,3] or [P,3,3] live on the device and are READ THERE by every item: `set_poses(t)` copies new poses in place, a viewer or a
    device-side path generator may write `self.poses` directly, and the next item follows.  reference_bank: the FrameBank the V reference views come
    from (H, W are its frame size); they are picked per item by get_nearest_cam_id's rule -- of the n1 = min(num_times V, T // 10) train cameras
    looking most nearly the same way, the V closest -- with ties decided (hnr_pose_views).  margin, dir_norm, bg_color (a triple), near, far and
    downweight_blurry_feats as BatchSampler.

    `next(out=None)` writes the item of frame step % P and advances the device counter `step`: the same static tensors on every call, no
    allocation after the first, no host read, at most three launches, capturable on one stream; `out` as BatchSampler.next.  `item(i)` is the explicit
    form (fresh tensors).  `views(poses=None)` is the [Q,V] table alone.  The dict has the keys driver.render_image reads -- raydir, pixel_idx,
    campos, camrotc2w = camrot, c2w, intrinsic, bg_color, near, far, h, w, c2w_nearest, w2c_nearest, campos_nearest, intrinsic_nearest,
    images_nearest, frame_weight_nearest, vid_angle_nearest -- and frame_row [1] = i.  A path frame has no gt_image, frame_weight or patch_table."""

    OUTPUTS = ("raydir", "pixel_idx", "campos", "camrot", "c2w", "intrinsic", "bg_color", "frame_row", "c2w_nearest", "w2c_nearest", "campos_nearest",
               "intrinsic_nearest", "images_nearest", "frame_weight_nearest", "vid_angle_nearest")

    def __init__(self, poses, intrinsic, reference_bank, V, margin=0, dir_norm=0, bg_color=(1, 1, 1), near=None, far=None, num_times=3,
                 downweight_blurry_feats=False):
        bank = reference_bank
        if not isinstance(bank, FrameBank):
            raise HnrError("PathSampler: reference_bank must be a FrameBank")
        if near is None or far is None:
            raise HnrError("PathSampler: near and far (the item's depth range) are required")
        self.bank, self.V, self.margin = bank, int(V), int(margin)
        self.near, self.far = float(near), float(far)
        if self.V < 1 or self.V > 64:
            raise HnrError("PathSampler: 1 <= V <= 64, got %d" % self.V)
        if bank.F > 8192:
            raise HnrError("PathSampler: at most 8192 reference cameras, the bank has %d" % bank.F)
        self.n1 = min(int(num_times) * self.V, bank.F // 10)
        if self.n1 < self.V:
            raise HnrError("PathSampler: n1 = min(num_times V, T // 10) = %d candidates of %d cameras cannot give %d views" % (self.n1, bank.F, self.V))
        if isinstance(bg_color, str):
            raise HnrError("PathSampler: bg_color must be a triple (%r is not supported for path frames)" % (bg_color,))
        self.bg = self._triple(bg_color)
        self._check_margin()
        H, W, m = bank.H, bank.W, self.margin
        self.R = (W - 2 * m) * (H - 2 * m)
        self.dir_norm, self.downweight = int(bool(dir_norm)), int(bool(downweight_blurry_feats))
        poses = self._poses(poses, None, "PathSampler")
        self.P = int(poses.shape[0])
        if isinstance(intrinsic, torch.Tensor):
            if not intrinsic.is_cuda or intrinsic.device != bank.device:
                raise HnrError("PathSampler: an intrinsic tensor must be on the bank's device %s, got %s" % (bank.device, intrinsic.device))
            K = intrinsic.to(torch.float32)
        else:
            K = torch.from_numpy(np.ascontiguousarray(intrinsic, dtype=np.float32))
        if tuple(K.shape) not in ((3, 3), (self.P, 3, 3)):
            raise HnrError("PathSampler: intrinsic must be [3,3] or [%d,3,3], got %s" % (self.P, tuple(K.shape)))
        dev = bank.device
        self.poses, self.intrinsic = poses.to(dev).contiguous().clone(), K.to(dev).contiguous().clone()      # the sampler's own tables
        self._K_per_pose = 1 if K.dim() == 3 else 0
        self._scratch = torch.zeros((_lib.PATH_SCRATCH_BYTES,), dtype=torch.uint8, device=dev)
        self.step = torch.zeros((1,), dtype=torch.int64, device=dev)          # the frame counter (read and advanced on the device)
        self._static, self._bound = None, {}

    # ------------------------------------------------------------------------------------------------ plumbing
    def _poses(self, poses, P, what):
        """[P,4,4] float32: an array is validated (finite) here, on the host; a tensor must be on the device already and is taken as it is"""
        if isinstance(poses, torch.Tensor):
            if not poses.is_cuda or poses.device != self.bank.device:
                raise HnrError("%s: a pose tensor must be on the bank's device %s, got %s" % (what, self.bank.device, poses.device))
            t = poses.to(torch.float32)
        else:
            a = np.ascontiguousarray(poses, dtype=np.float32)
            if a.ndim == 3 and not np.isfinite(a).all():
                raise HnrError("%s: a pose is not finite" % what)
            t = torch.from_numpy(a)
        if t.dim() != 3 or tuple(t.shape[1:]) != (4, 4) or t.shape[0] < 1 or (P is not None and t.shape[0] != P):
            raise HnrError("%s: poses must be [%s,4,4], got %s" % (what, "P" if P is None else P, tuple(t.shape)))
        return t

    def _shapes(self):
        b, V, R = self.bank, self.V, self.R
        f, i = torch.float32, torch.int32
        return dict(raydir=((R, 3), f), pixel_idx=((R, 2), f), campos=((3,), f), camrot=((3, 3), f), c2w=((4, 4), f), intrinsic=((3, 3), f), bg_color=((3,), f),
                    frame_row=((1,), i), c2w_nearest=((V, 4, 4), f), w2c_nearest=((V, 4, 4), f), campos_nearest=((V, 3), f), intrinsic_nearest=((3, 3), f),
                    images_nearest=((V, b.H, b.W, 3), f), frame_weight_nearest=((V,), f), vid_angle_nearest=((V,), f))

    def _alloc(self):
        return {k: torch.empty(s, dtype=d, device=self.bank.device) for k, (s, d) in self._shapes().items()}

    def _bind(self, tensors, what):
        for k in tensors:
            if k in ("gt_image", "frame_weight", "patch_table", "gt_depth"):
                raise HnrError("%s: a path frame has no %s (there is no ground truth for a free camera)" % (what, k))
        return self._bind_outputs(tensors, self._shapes(), what)

    def _launch(self, o, step, i):
        _lib.call("hnr_path_item", self.bank._c, self.poses, self.P, self.intrinsic, self._K_per_pose, self.V, self.n1, step, i, self.margin, self.dir_norm,
                  (ctypes.c_float * 3)(*self.bg), self.downweight, o, self._scratch, int(self._scratch.numel()), _lib.STREAM)

    # ------------------------------------------------------------------------------------------------ the interface
    def set_poses(self, poses):
        """New poses [P,4,4] (the same P) copied into the device table in place: captured graphs and later items read them."""
        self.poses.copy_(self._poses(poses, self.P, "PathSampler.set_poses"))
        return self

    def set_step(self, step):
        self.step.fill_(int(step))
        return self

    def views(self, poses=None, exclude_rows=None):
        """hnr_pose_views: the [Q,V] int32 rows of the reference bank for `poses` [Q,4,4] (default: the sampler's own table, with its intrinsic;
        other poses use the shared intrinsic, so the sampler's must be [3,3] or Q must be P).  exclude_rows [Q] int32 (-1 = none): the `is_train`
        rule -- a query that IS that train row does not pick itself; it needs one more candidate, n1 >= V + 1.  Stays on the device."""
        dev = self.bank.device
        p = self.poses if poses is None else self._poses(poses, None, "PathSampler.views").to(dev).contiguous()
        Q = int(p.shape[0])
        if self._K_per_pose and Q != self.P:
            raise HnrError("PathSampler.views: %d poses for per-pose intrinsics of %d" % (Q, self.P))
        ex = None
        if exclude_rows is not None:
            if self.n1 < self.V + 1:
                raise HnrError("PathSampler.views: n1 = %d candidates cannot give %d views plus an excluded row" % (self.n1, self.V))
            ex = torch.as_tensor(np.asarray(exclude_rows.detach().cpu() if isinstance(exclude_rows, torch.Tensor) else exclude_rows, dtype=np.int32))
            if tuple(ex.shape) != (Q,):
                raise HnrError("PathSampler.views: exclude_rows must be [%d], got %s" % (Q, tuple(ex.shape)))
            ex = ex.to(dev).contiguous()
        out = torch.empty((Q, self.V), dtype=torch.int32, device=dev)
        _lib.call("hnr_pose_views", self.bank._c, p, Q, self.intrinsic, self._K_per_pose, ex, self.V, self.n1, out, _lib.STREAM)
        return out

    def next(self, out=None):
        """The item of frame step % P; step += 1 on the device.  out=None: the sampler's own static tensors; out = a dict: the outputs whose keys
        are present in it ("camrot" or "camrotc2w" for the rotation) are written into those tensors and no others are touched."""
        res, o = self._next_outputs(out)
        self._launch(o, self.step, 0)
        return res

    def item(self, i):
        """The item of frame i of the table as it stands on the device, no counter; fresh tensors."""
        i = int(i)
        if i < 0 or i >= self.P:
            raise HnrError("PathSampler.item: frame %d is outside the path (0 .. %d)" % (i, self.P - 1))
        t = self._alloc()
        self._launch(self._bind(t, "PathSampler.item"), None, i)
        return self._finish(t)
