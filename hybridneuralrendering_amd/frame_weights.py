"""Content-aware frame weights on the device: what the reference reads from `frame_weights_step5/<scene>_frame_weight_step5.npy`
(data/scannet_ft_dataset.py:502) and makes with raft/demo_content_aware_weights.py.

Per pair of consecutive training frames: RAFT flow (flow.py, csrc/raft.hip), Laplacian edge maps in fp64 and the variance of both frames' edges over
the flow-aligned overlap (csrc/blur_score.hip).  Per pair nothing is read back; per scene ONE host read of a device table [F,3] fp64
(score_cur, score_ref, used-pixel count).  The chain rescale and the sliding-window weights (demo_content_aware_weights.py:186-220) run on the host in
fp64 numpy over F numbers, as the reference does.  The result goes straight into `frames.FrameBank(weights=...)`.

Decoding and resizing the JPEGs stay outside, as in frames.py: the grey planes are an input.  `gray_from_rgb` is a convenience (the BT.601 luma of
the decoded RGB, rounded); it is NOT `cv2.imread(path, 0)` of a JPEG, which decodes the luma plane directly.  cv2 is not a dependency: the edge maps
follow OpenCV's documented definitions of `blur` and `Laplacian(ksize=1)` with BORDER_REFLECT_101.
"""
import numpy as np
import torch

from . import _lib
from ._lib import HnrError


def _u8(t, name, dims):
    t = _lib.require_gpu(t, name, torch.uint8).detach()
    if t.dim() != dims:
        raise HnrError("%s must have %d dimensions, got %s" % (name, dims, tuple(t.shape)))
    return t


def gray_from_rgb(images_u8):
    """[F,H,W,3] uint8 -> [F,H,W] uint8: round(0.299 R + 0.587 G + 0.114 B).  Not cv2.imread(., 0) of a JPEG (see the module text)."""
    images_u8 = _u8(images_u8, "images_u8", 4)
    f = images_u8.float()
    return torch.clamp(torch.round(0.299 * f[..., 0] + 0.587 * f[..., 1] + 0.114 * f[..., 2]), 0, 255).to(torch.uint8)


def blur_edges(gray_u8):
    """hnr_blur_edges: grey planes [P,H,W] uint8 -> Laplacian of the 5x5 box mean [P,H,W] fp64 (`detect_blurry`, demo_content_aware_weights.py:78-92)."""
    gray_u8 = _u8(gray_u8, "gray_u8", 3)
    P, H, W = (int(s) for s in gray_u8.shape)
    if P < 1 or min(H, W) < 8:
        raise HnrError("blur_edges: gray_u8 must be [P >= 1, H >= 8, W >= 8], got %s" % (tuple(gray_u8.shape),))
    out = torch.empty((P, H, W), dtype=torch.float64, device=gray_u8.device)
    _lib.call("hnr_blur_edges", gray_u8, P, H, W, out, _lib.STREAM)
    return out


def _score_into(e1, e2, flow, H, W, border, row, pick, used, scratch):
    _lib.call("hnr_blur_score_pair", e1, e2, flow, H, W, border, row, pick, used, scratch, scratch.numel(), _lib.STREAM)


def blur_score_pair(edge1, edge2, flow_up, border=20, want_maps=False):
    """hnr_blur_score_pair: edge1, edge2 [H,W] fp64, flow_up [2,H,W] (or [1,2,H,W]) fp32 -> row [3] fp64 on the device = (variance of edge 1, variance of
    the warped edge 2, used-pixel count); with want_maps also (pick [H,W] int32: picked pixel index or -1, used [H,W] bool)."""
    edge1, edge2 = _lib.require_gpu(edge1, "edge1", torch.float64).detach(), _lib.require_gpu(edge2, "edge2", torch.float64).detach()
    flow_up = _lib.require_gpu(flow_up, "flow_up", torch.float32).detach()
    if flow_up.dim() == 4 and flow_up.shape[0] == 1:
        flow_up = flow_up[0]
    if edge1.dim() != 2 or edge2.shape != edge1.shape or tuple(flow_up.shape) != (2,) + tuple(edge1.shape):
        raise HnrError("blur_score_pair: edge1, edge2 must be [H,W] and flow_up [2,H,W]")
    H, W, border = int(edge1.shape[0]), int(edge1.shape[1]), int(border)
    if min(H, W) < 8 or border < 0 or 2 * border >= min(H, W):
        raise HnrError("blur_score_pair: a border of %d leaves nothing of a %dx%d frame (H, W >= 8)" % (border, H, W))
    dev = edge1.device
    row = torch.empty((3,), dtype=torch.float64, device=dev)
    pick = torch.empty((H, W), dtype=torch.int32, device=dev) if want_maps else None
    used = torch.empty((H, W), dtype=torch.uint8, device=dev) if want_maps else None
    scratch = _lib.scratch("hnr_blur_score_pair_scratch_bytes", H, W, device=dev)
    _score_into(edge1, edge2, flow_up.contiguous(), H, W, border, row, pick, used, scratch)
    return (row, pick, used.bool()) if want_maps else row


def score_table(images_u8, gray_u8, raft, border=20, iters=20, want_flows=False):
    """The device table [F,3] fp64 of a scene: row f = blur_score_pair of frames (f, f+1) under RAFT's flow f -> f+1; the last frame pairs with itself
    (demo_content_aware_weights.py:130-133).  Nothing is read back."""
    images_u8, gray_u8 = _u8(images_u8, "images_u8", 4), _u8(gray_u8, "gray_u8", 3)
    if images_u8.shape[-1] != 3 or tuple(gray_u8.shape) != tuple(images_u8.shape[:3]) or images_u8.shape[0] < 1:
        raise HnrError("content_aware_weights: images_u8 must be [F,H,W,3] and gray_u8 [F,H,W], got %s and %s" % (tuple(images_u8.shape), tuple(gray_u8.shape)))
    if not hasattr(raft, "flow_pair"):
        raise HnrError("content_aware_weights: raft must be a flow.RAFT")
    from .flow import check_shape
    F, H, W = (int(s) for s in gray_u8.shape)
    check_shape(H, W, "content_aware_weights")
    border = int(border)
    if border < 0 or 2 * border >= min(H, W):
        raise HnrError("content_aware_weights: a border of %d leaves nothing of a %dx%d frame" % (border, H, W))
    dev = images_u8.device
    edges = blur_edges(gray_u8)
    table = torch.empty((F, 3), dtype=torch.float64, device=dev)
    scratch = _lib.scratch("hnr_blur_score_pair_scratch_bytes", H, W, device=dev)
    flows = []
    for f in range(F):
        g = min(f + 1, F - 1)
        pair = images_u8[[f, g]].permute(0, 3, 1, 2).float().contiguous()
        _, up = raft.flow_pair(pair, iters)
        _score_into(edges[f], edges[g], up, H, W, border, table[f], None, None, scratch)
        if want_flows:
            flows.append(up)
    return (table, flows) if want_flows else table


def weights_from_scores(score_cur, score_ref, window_size=10, sliding_step=5):
    """demo_content_aware_weights.py:186-220 in fp64 numpy: the chained rescale (frame i+1's own score is brought to the scale of frame i's view of it:
    scale_{i+1} = ref_i * scale_i / cur_{i+1}), then the mean-normalised scores of every window [b, b + window_size), b = 0, sliding_step, ...,
    up to and including the first window that reaches the end, averaged over the windows that cover a frame."""
    cur, ref = np.asarray(score_cur, dtype=np.float64).reshape(-1), np.asarray(score_ref, dtype=np.float64).reshape(-1)
    n, window_size, sliding_step = cur.shape[0], int(window_size), int(sliding_step)
    if n < 1 or ref.shape[0] != n:
        raise HnrError("weights_from_scores: score_cur and score_ref must have the same length >= 1")
    if window_size < 1 or sliding_step < 1:
        raise HnrError("weights_from_scores: window_size and sliding_step must be positive")
    if sliding_step > window_size:
        raise HnrError("weights_from_scores: sliding_step %d > window_size %d leaves frames that no window covers (the reference divides 0 by 0 "
                       "there)" % (sliding_step, window_size))
    absolute, scale = np.empty(n), 1.0
    for i in range(n):
        absolute[i] = cur[i] * scale
        if i < n - 1:
            scale = (ref[i] * scale) / cur[i + 1]
    weight, count, begin = np.zeros(n), np.zeros(n), 0
    while True:
        end = min(begin + window_size, n)
        bundle = absolute[begin:end]
        weight[begin:end] += bundle / np.mean(bundle)
        count[begin:end] += 1
        if begin + window_size >= n:
            break
        begin += sliding_step
    return weight / count


def content_aware_weights(images_u8, gray_u8, raft, window_size=10, sliding_step=5, border=20, iters=20):
    """images_u8 [F,H,W,3] uint8 on the device (the training frames: every step-th frame of the scan, in order), gray_u8 [F,H,W] uint8 ->
    np.ndarray [F] float64: the content-aware weights."""
    table = score_table(images_u8, gray_u8, raft, border, iters).cpu().numpy()             # the one host read
    empty = np.nonzero(table[:, 2] == 0)[0]
    if empty.size:
        raise HnrError("content_aware_weights: no pixel of frame(s) %s survives the border and the warp (count 0)" % empty.tolist())
    return weights_from_scores(table[:, 0], table[:, 1], window_size, sliding_step)
