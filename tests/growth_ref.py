"""NumPy restatement of the growth schedule's bookkeeping (csrc/rank.hip, growth.RayMissRanking, growth.probe_tier): the ray-miss loss in the
kernel's operation order, the table update with a stable sort, the tier gate and the frame list of the grow pass.

Reference: models/base_rendering_model.py:1147-1159 (the `ray_miss` colour item), models/mvs_points_volumetric_model.py:154-185 (update_rank_ray_miss,
rank_ray_miss, setup, reset_ray_miss_ranking), run/train_ft.py:458-462, :472-477, :878-882.  tests/golden/growth_rank.npz holds what those functions
themselves return on a recorded sequence; test_growth_rank.py compares this file against it, test_growth_rank_gpu.py the device against both.
"""
import numpy as np

THREADS = 256          # lanes of the kernel's one workgroup; a wave is 64 of them


def ray_miss_loss(color, gt, ray_mask):
    """(L float32, number of missed rays) of one batch.  Differences and squares in fp32, each rounded once; fp64 sums in the kernel's order: lane t takes
    rays t, t + 256, ... (channels 0, 1, 2 of a ray in turn), a butterfly within each wave, the four waves in order; / 3 in fp64, one rounding to fp32."""
    color = np.asarray(color, np.float32).reshape(-1, 3)
    gt = np.asarray(gt, np.float32).reshape(-1, 3)
    miss = np.asarray(ray_mask).reshape(-1) == 0
    R = color.shape[0]
    assert gt.shape[0] == R and miss.shape[0] == R
    with np.errstate(invalid="ignore", over="ignore"):
        d = (color - gt).astype(np.float32)
        sq = (d * d).astype(np.float32).astype(np.float64)
    sq[~miss] = 0.0                                           # (adding +0.0 to a sum of non-negative terms changes nothing)
    per = -(-R // THREADS) if R else 0
    pad = np.zeros((per * THREADS, 3), np.float64)
    pad[:R] = sq
    pad = pad.reshape(per, THREADS, 3)
    acc = np.zeros(THREADS, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(per):
            for c in range(3):
                acc = acc + pad[k, :, c]
        lane = np.arange(THREADS)
        for o in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[lane ^ o]
        total = ((acc[0] + acc[64]) + acc[128]) + acc[192]
        n_miss = int(miss.sum())
        L = np.float32(total / 3.0) if n_miss > 0 else np.float32(0.0)
    return L, n_miss


def new_table(train_len, prob_num_step):
    """setup / reset_ray_miss_ranking (:174-185): (ids int32, losses float32); one slot without frame ids for prob_num_step == 1."""
    n = train_len // prob_num_step + 1 if prob_num_step > 1 else 1
    return np.arange(n, dtype=np.int32), np.zeros(n, np.float32)


def rank_update(ids, losses, frame_id, L):
    """rank_ray_miss (:162-172) on copies: the slot holding frame_id takes max(L, old), else the last slot is overwritten; then a descending STABLE sort
    (equal losses keep their slot order).  A non-finite L leaves the table as it was.  One slot (prob_num_step == 1): the running maximum (:158-159)."""
    ids, losses = np.array(ids, np.int32), np.array(losses, np.float32)
    L = np.float32(L)
    if not np.isfinite(L):
        return ids, losses
    if losses.shape[0] == 1:
        losses[0] = losses[0] if losses[0] > L else L
        return ids, losses
    m = ids == np.int32(frame_id)
    if m.any():
        losses[m] = np.where(losses[m] > L, losses[m], L)
    else:
        ids[-1], losses[-1] = frame_id, L
    order = np.argsort(-losses, kind="stable")
    return ids[order], losses[order]


def probe_tier(total_steps, prob_tiers, prob_kernel_size):
    """(tier, query_size or None) while a tier is left, None behind the last one (:155, run/train_ft.py:458-462, :879-882).  prob_kernel_size None:
    tier 0 with the cloud's own query_size (None)."""
    if prob_kernel_size is None:
        return 0, None
    tier = int(np.sum(np.asarray(prob_tiers) < total_steps))
    if tier >= len(prob_kernel_size) // 3:
        return None
    return tier, [int(v) for v in prob_kernel_size[3 * tier:3 * tier + 3]]


def top_frames(ids, losses, max_num):
    """run/train_ft.py:476-477: the frames with a positive loss, the last slot aside, in table order."""
    ids, losses = np.asarray(ids), np.asarray(losses)
    return [int(i) for i in ids[:-1][losses[:-1] > 0][:max_num]]


def loss_tolerance(R):
    """Relative bound between this fp64 sum and a float32 reduction of the same 3R non-negative terms (torch's MSELoss, then * the number of missed rays):
    log2(3R) levels of a pairwise float32 sum plus the roundings of the mean, the product and the final conversion."""
    return (np.log2(3 * R) + 8) * 2.0 ** -24
