"""Generates tests/golden/frames.npz by running the REFERENCE's own dataset code on small synthetic inputs.  Needs the reference checkout
(tests/golden/_ref_import.py); the fixture holds data only.

Reference functions called (none is copied):
  data/scannet_ft_dataset.py        ScannetFtDataset.__getitem__ with a stand-in `self` (JPEG frames and pose files in a temporary scan directory,
                                    transform = uint8 -> permute -> float / 255, what ToTensor computes), for random_sample = random, patch, dilated
                                    and no_crop; it calls data_utils.get_dtu_raydir
  data/nerf_synth360_ft_dataset.py  get_nearest_cam_id, on a ring of synthetic cameras, with get_dtu_raydir for the centre-pixel direction (:740-741)

Recorded: the decoded uint8 frames (np.asarray(Image.open(...))), poses, K, weights; for several frames the item's pixel_idx, raydir, gt_image,
images_nearest, c2w_nearest, campos_nearest, frame_weight, frame_weight_nearest, vid_angle_nearest; the nearest picks of every frame; and raydir_tol =
4 x the largest distance between the reference's raydir (a BLAS product) and the sequential fp32 form of tests/frames_ref.py over all recorded rays.

The ids (12 train frames at step 5, test ids 22 and 38) and V = 4 are chosen so that the cut after V (and after int(1.5 V) candidates) never splits a
pair of equal id distances: the picks are unambiguous as a set.

Run:  python tests/golden/make_golden_frames.py
"""
import importlib
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

H, W, V = 48, 64, 4
STEP, TOTAL = 5, 60
TRAIN_IDS = list(range(0, 60, STEP))
TEST_IDS = [22, 38]
WEIGHT_EXP = 2.0
MARGIN = 3
NEAR_FAR = (0.1, 8.0)


def make_image(rng, k):
    """smooth colour ramps + saturated 8x8 blocks (JPEG keeps exact 0 and 255 inside them)"""
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([127 + 100 * np.sin(xx / 9.0 + k), 127 + 100 * np.cos(yy / 7.0 + 0.5 * k), 40 + 3 * xx + yy - 2 * k], axis=-1)
    img = np.clip(img + rng.normal(0, 4, size=img.shape), 0, 255).astype(np.uint8)
    img[8:16, 8 * (k % 6):8 * (k % 6) + 8] = 0
    img[24:32, 8 * ((k + 2) % 7):8 * ((k + 2) % 7) + 8] = 255
    return img


def to_tensor(pil):
    """what torchvision's ToTensor computes for an 8-bit RGB image"""
    return torch.from_numpy(np.asarray(pil).copy()).permute(2, 0, 1).float() / 255


class RefItems:
    def __init__(self, ds, tmp, K, weights):
        self.ds, self.tmp, self.K, self.weights = ds, tmp, K, weights

    def __call__(self, split, index, mode, seed, size=8, dilation_setup="3_4_1_3", downweight=1, select_high_quality=0, dir_norm=0):
        ids = TRAIN_IDS if split == "train" else TEST_IDS
        opt = types.SimpleNamespace(use_frame_weight=1, weight_exp=WEIGHT_EXP, dynamic_nearest=0, use_nearest=V, select_high_quality=select_high_quality,
                                    find_nearest_mode=1, downweight_blurry_feats=downweight, edge_filter=MARGIN, random_sample_size=size,
                                    random_sample=mode, dilation_setup=dilation_setup, dir_norm=dir_norm)
        me = types.SimpleNamespace(id_list=ids, data_dir=self.tmp, scan="scan", img_wh=(W, H), transform=to_tensor, intrinsic=self.K, split=split, opt=opt,
                                   train_weight_list=self.weights, train_id_list=TRAIN_IDS, total_num_image=TOTAL, step=STEP, near_far=NEAR_FAR,
                                   bg_color=(1.0, 1.0, 1.0), blur_kernels=np.zeros((1, 3, 3), np.float32))
        np.random.seed(seed)
        random.seed(seed)
        return self.ds.ScannetFtDataset.__getitem__(me, index)


def main():
    import make_golden_cloud_init as G
    import frames_ref as R
    mu, ds, pm = G.import_reference_modules()
    ds.Image = Image
    rng = np.random.default_rng(7)
    out = {}
    K = np.array([[57.7, 0.0, 31.9], [0.0, 57.9, 24.3], [0.0, 0.0, 1.0]], np.float32)
    weights = [float(w) for w in rng.uniform(0.3, 1.0, size=len(TRAIN_IDS))]
    all_ids = TRAIN_IDS + TEST_IDS
    poses = {}
    for n, vid in enumerate(all_ids):
        a = 0.04 * vid
        poses[vid] = G.look_at([2.0 * np.cos(a), 2.0 * np.sin(a), 1.2 + 0.01 * vid], [0.1 * np.sin(3 * a), 0.2, 1.0])
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "scan", "exported", "pose"))
        os.makedirs(os.path.join(tmp, "scan", "exported", "color"))
        decoded = {}
        for n, vid in enumerate(all_ids):
            np.savetxt(os.path.join(tmp, "scan", "exported", "pose", "%d.txt" % vid), poses[vid].astype(np.float64), fmt="%.9e")
            path = os.path.join(tmp, "scan", "exported", "color", "%d.jpg" % vid)
            Image.fromarray(make_image(rng, n)).save(path, quality=92)
            decoded[vid] = np.asarray(Image.open(path)).copy()
            assert decoded[vid].shape == (H, W, 3) and decoded[vid].dtype == np.uint8
        run = RefItems(ds, tmp, K, weights)
        out["train_images"] = np.stack([decoded[v] for v in TRAIN_IDS])
        out["test_images"] = np.stack([decoded[v] for v in TEST_IDS])
        assert out["train_images"].min() == 0 and out["train_images"].max() == 255
        out["train_c2w"] = np.stack([poses[v] for v in TRAIN_IDS])
        out["test_c2w"] = np.stack([poses[v] for v in TEST_IDS])
        out["train_ids"], out["test_ids"] = np.array(TRAIN_IDS, np.int64), np.array(TEST_IDS, np.int64)
        out["K"], out["weights"], out["weight_exp"] = K, np.array(weights, np.float64), np.array([WEIGHT_EXP])
        out["total_num_image"], out["margin"], out["V"] = np.array([TOTAL]), np.array([MARGIN]), np.array([V])

        # ---- the nearest picks of every frame (as vids), plain and select_high_quality
        row_of = {v: i for i, v in enumerate(TRAIN_IDS)}
        for shq in (0, 1):
            for split, ids in (("train", TRAIN_IDS), ("test", TEST_IDS)):
                picks = []
                for i in range(len(ids)):
                    it = run(split, i, "random", 1, select_high_quality=shq)
                    ang = np.asarray(it["vid_angle_nearest"], np.float64)
                    vids = np.rint(ang / (2 * np.pi) * TOTAL).astype(np.int64)
                    assert np.array_equal(np.stack([poses[v] for v in vids]), it["c2w_nearest"].numpy())
                    picks.append([row_of[v] for v in vids])
                out["nearest_%s_shq%d" % (split, shq)] = np.array(picks, np.int32)
        # the cut never splits a pair of equal distances
        for ids in (TRAIN_IDS, TEST_IDS):
            for vid in ids:
                d = np.sort(np.abs(np.array(TRAIN_IDS) - vid))
                d = d[1:] if d[0] == 0 else d
                assert d[V - 1] != d[V] and d[int(V * 1.5) - 1] != d[int(V * 1.5)], vid

        # ---- items: the first train frame, a middle one, a test id; every mode
        worst, nrays, ndiff, ncomp = 0.0, 0, 0, 0
        cases = [("train", 0), ("train", 5), ("test", 0)]
        for ci, (split, index) in enumerate(cases):
            for mode in ("random", "patch", "dilated", "no_crop"):
                for dir_norm in ((0, 1) if mode == "random" else (0,)):
                    it = run(split, index, mode, 100 + ci, dir_norm=dir_norm)
                    tag = "item_%s%d_%s%s" % (split, index, mode, "_norm" if dir_norm else "")
                    pix = np.asarray(it["pixel_idx"], np.float32).reshape(-1, 2)
                    rd = it["raydir"].numpy()
                    out[tag + "_pixel_idx"], out[tag + "_raydir"] = pix, rd
                    out[tag + "_gt_image"] = np.asarray(it["gt_image"], np.float32)
                    assert np.asarray(it["gt_image"]).dtype == np.float32
                    c2w = poses[(TRAIN_IDS if split == "train" else TEST_IDS)[index]]
                    seq = R.raydir(pix[:, 0], pix[:, 1], K, c2w[:3, :3], bool(dir_norm))
                    diff = np.abs(seq.astype(np.float64) - rd.astype(np.float64))
                    worst, nrays, ndiff, ncomp = max(worst, float(diff.max())), nrays + len(pix), ndiff + int((diff > 0).sum()), ncomp + diff.size
                    if mode == "random" and not dir_norm:                            # the frame-level fields, once per frame
                        base = "item_%s%d" % (split, index)
                        out[base + "_images_nearest"] = np.asarray(it["images_nearest"], np.float32)
                        out[base + "_c2w_nearest"] = it["c2w_nearest"].numpy()
                        out[base + "_campos_nearest"] = it["campos_nearest"].numpy()
                        out[base + "_frame_weight"] = np.array([it["frame_weight"]], np.float64)
                        out[base + "_frame_weight_nearest"] = np.asarray(it["frame_weight_nearest"], np.float64)
                        out[base + "_vid_angle_nearest"] = np.asarray(it["vid_angle_nearest"], np.float64)
                        out[base + "_campos"], out[base + "_camrotc2w"], out[base + "_c2w"] = it["campos"].numpy(), it["camrotc2w"].numpy(), it["c2w"].numpy()
        out["item_cases"] = np.array(["%s%d" % c for c in cases])
        out["raydir_tol"] = np.array([4 * worst], np.float64)
        print("raydir: sequential fp32 vs the reference's BLAS product: max %.3g, %d of %d components differ (%.2f %%), %d rays -> raydir_tol %.3g"
              % (worst, ndiff, ncomp, 100.0 * ndiff / ncomp, nrays, 4 * worst))

    # ---- get_nearest_cam_id on a ring of synthetic cameras
    nd = importlib.import_module("data.nerf_synth360_ft_dataset")
    T = 60
    ang = np.sort(rng.uniform(0, 2 * np.pi, size=T))
    ring = np.stack([G.look_at([3.0 * np.cos(a), 3.0 * np.sin(a), 1.0 + 0.4 * np.sin(5 * a)], [0.0, 0.0, 0.8]) for a in ang])
    Ks = np.array([[60.0, 0.0, 32.0], [0.0, 60.0, 24.0], [0.0, 0.0, 1.0]], np.float32)
    wh = (W, H)
    center = np.asarray(wh).astype(np.float32)[None, :] // 2
    dirs = np.concatenate([nd.get_dtu_raydir(center, Ks, M[:3, :3], True) for M in ring]).astype(np.float32)
    pos = ring[:, :3, 3].copy()
    tids = np.arange(T)
    tang = rng.uniform(0, 2 * np.pi, size=3)
    tests = np.stack([G.look_at([3.0 * np.cos(a), 3.0 * np.sin(a), 1.1], [0.0, 0.0, 0.8]) for a in tang])
    picks_train, picks_test = [], []
    for q in (0, 17, 59):
        d = nd.get_dtu_raydir(center, Ks, ring[q][:3, :3], True)
        picks_train.append(nd.get_nearest_cam_id(ring[q][:3, 3], d, q, pos, dirs, tids, V, num_times=3, is_train=True))
    for q in range(len(tests)):
        d = nd.get_dtu_raydir(center, Ks, tests[q][:3, :3], True)
        picks_test.append(nd.get_nearest_cam_id(tests[q][:3, 3], d, q, pos, dirs, tids, V, num_times=3, is_train=False))
    out.update(ring_c2w=ring, ring_K=Ks, ring_pos=pos, ring_dirs=dirs, ring_query_train=np.array([0, 17, 59]), ring_test_c2w=tests,
               ring_picks_train=np.array(picks_train, np.int32), ring_picks_test=np.array(picks_test, np.int32), ring_wh=np.array(wh))
    path = os.path.join(HERE, "frames.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 1000000, size
    print("wrote %s (%d bytes, %d arrays)" % (path, size, len(out)))


if __name__ == "__main__":
    main()
