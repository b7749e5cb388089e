"""Generates tests/golden/growth_rank.npz by running the REFERENCE's own growth-schedule bookkeeping on a recorded sequence of small batches.  Needs the
reference checkout (tests/golden/_ref_import.py); the fixture holds data only.

Reference functions called (none is copied):
  models/base_rendering_model.py          BaseRenderingModel.compute_losses on a stand-in `self` -> loss_ray_miss_coarse_raycolor (:1147-1159)
  models/mvs_points_volumetric_model.py   setup (its table sizing), reset_ray_miss_ranking, rank_ray_miss, update_rank_ray_miss (:154-185): the methods are
                                          compiled from the file where it lies into a class of our own (the module's imports -- MVS nets, data
                                          loaders -- cannot be satisfied here), its parent's setup() replaced by a no-op
  run/train_ft.py                         probe_hole (:450-569), for the frames its take_top branch visits, the query_size it sets per tier and the
                                          ranking reset behind it; stand-in dataset / visualiser, a model whose test() returns rays that all hit

Sequence: train_len 40, prob_num_step 4 (a table of 11 slots), 60 steps of 49 rays; the frames are chosen while the reference runs so that every case
the kernel distinguishes occurs, and the generator asserts that on the reference's own results (see `main`).

Run:  python tests/golden/make_golden_growth.py
"""
import ast
import os
import random
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from _ref_import import REF, import_reference  # noqa: E402

TRAIN_LEN, NUM_STEP, R, STEPS = 40, 4, 49, 60
TIERS, KERNEL = [40000, 120000], [3, 3, 3, 1, 1, 1]           # dev_scripts/w_scannet_etf/scene241_hybrid.sh:138-139
BG = np.ones(3, np.float32)


def _reference_functions(path, names, cls=None):
    """The named functions of a reference source file (top level, or methods of class `cls`), compiled from the file where it lies into a namespace of
    our choosing -- the technique of make_golden.py.  Nothing of the source is stored; only the fixture it produces."""
    body = ast.parse(open(path).read()).body
    if cls is not None:
        body = [n for n in body if isinstance(n, ast.ClassDef) and n.name == cls][0].body
    keep = [n for n in body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(keep) == len(names), [n.name for n in keep]
    return compile(ast.Module(body=keep, type_ignores=[]), path, "exec")


def reference_model_class():
    """A class holding the reference's own ranking methods."""
    path = os.path.join(REF, "models", "mvs_points_volumetric_model.py")
    names = ("setup", "reset_ray_miss_ranking", "rank_ray_miss", "update_rank_ray_miss")
    ns = dict(torch=torch, np=np)
    exec(_reference_functions(path, names, cls="MvsPointsVolumetricModel"), ns)

    class Base:
        device = torch.device("cpu")

        def setup(self, opt):
            pass

    model = type("MvsPointsVolumetricModel", (Base,), {n: ns[n] for n in names})
    ns["MvsPointsVolumetricModel"] = model                     # the name its super(...) call resolves
    return model


def new_model(Model, prob_num_step=NUM_STEP, kernel=KERNEL):
    m = Model()
    m.opt = SimpleNamespace(prob_freq=10000, prob_num_step=prob_num_step, prob_kernel_size=kernel, prob_tiers=TIERS, kernel_size=[3, 3, 3], query_size=[3, 3, 3],
                            prob=0)
    m.setup(m.opt, train_len=TRAIN_LEN)
    return m


def ray_miss_loss(brm, color, gt, ray_mask):
    """compute_losses with the shipped colour items (scene241_hybrid.sh:146-147) -> the ray_miss item"""
    opt = SimpleNamespace(color_loss_items=["ray_masked_coarse_raycolor", "ray_miss_coarse_raycolor", "coarse_raycolor"], color_loss_weights=[1.0, 0.0, 0.0],
                          depth_loss_items=[], depth_loss_weights=[], bg_loss_items=[], bg_loss_weights=[], zero_one_loss_items=[], zero_one_loss_weights=[],
                          zero_epsilon=1e-3, l2_size_loss_items=[], l2_size_loss_weights=[], sparse_loss_weight=0, use_frame_weight=0)
    shell = SimpleNamespace(opt=opt, output=dict(coarse_raycolor=torch.from_numpy(color)[None], ray_mask=torch.from_numpy(ray_mask)[None]),
                            gt_image=torch.from_numpy(gt)[None], l2loss=torch.nn.MSELoss(), is_train=True, dilation_PatchSize=None, input={}, frame_weight=None)
    brm.BaseRenderingModel.compute_losses(shell)
    return shell.loss_ray_miss_coarse_raycolor


def make_batch(rng, p_miss):
    gt = (rng.integers(0, 256, size=(R, 3)).astype(np.float32) / np.float32(255)).astype(np.float32)
    gt[rng.random(R) < 0.25] = 1.0                                         # background-coloured ground truth: a miss there costs nothing
    color = rng.random((R, 3)).astype(np.float32)
    mask = (rng.random(R) >= p_miss).astype(np.int8)
    if p_miss >= 1.0:
        mask[:] = 0
    if p_miss <= 0.0:
        mask[:] = 1
    color[mask == 0] = BG                                                   # what the renderer leaves at a missed ray
    if rng.random() < 0.3:                                                  # ... and what the blur module can turn it into
        color[mask == 0] = (BG - rng.random((int((mask == 0).sum()), 3)) * 0.05).astype(np.float32)
    return color, gt, mask


def probe_frames(Model, state, test_steps):
    """The reference's probe_hole on a model holding the table `state`: (frames visited, query_size it set, table after the pass)."""
    code =_reference_functions(os.path.join(REF, "run", "train_ft.py"), ("probe_hole", "bloat_inds"))

    class TorchCPU:
        def __getattr__(self, n):
            return getattr(torch, n)

        @staticmethod
        def zeros(*a, **k):
            k.pop("device", None)
            return torch.zeros(*a, **k)

    class Bar:
        def __init__(self, it):
            self.it = it

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

        def __iter__(self):
            return iter(self.it)

        def set_description(self, *_):
            pass

    H, W = 6, 8
    pix = np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).astype(np.float32).reshape(1, H, W, 2)
    n_rays = H * W
    visited = []

    class ProbeModel(Model):
        def set_input(self, data):
            self.cur = data

        def test(self):
            n = self.cur["pixel_idx"].shape[1]
            z = lambda c: torch.zeros(1, n, c)
            return dict(coarse_raycolor=z(3), ray_mask=torch.ones(1, n), ray_max_sample_loc_w=z(3), ray_max_far_dist=z(1), ray_max_shading_opacity=z(1),
                        shading_avg_color=z(3), shading_avg_dir=z(3), shading_avg_conf=z(1), shading_avg_embedding=z(32))

    class Dataset:
        height, width = H, W

        def __len__(self):
            return TRAIN_LEN

        def get_item(self, i):
            visited.append(int(i))
            return dict(bg_color=torch.ones(3), raydir=torch.zeros(1, n_rays, 3), pixel_idx=torch.from_numpy(pix), gt_image=torch.zeros(n_rays, 3))

    model = new_model(ProbeModel)
    model.top_ray_miss_ids, model.top_ray_miss_loss = torch.from_numpy(state[0].copy()), torch.from_numpy(state[1].copy())
    vis = SimpleNamespace(reset=lambda: None, save_ref_views=lambda *a, **k: None, save_neural_points=lambda *a, **k: None, print_details=lambda *a, **k: None)
    opt = SimpleNamespace(point_features_dim=32, prob_kernel_size=KERNEL, prob_tiers=TIERS, prob_mode=0, prob_num_step=NUM_STEP, prob_top=1,
                          random_sample_size=8, far_thresh=0.0, prob_mul=0.4, bgmodel="no")
    ns = dict(torch=TorchCPU(), np=np, random=random, tqdm=Bar, print=lambda *a, **k: None)
    old_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        exec(code, ns)
        add = ns["probe_hole"](model, Dataset(), vis, opt, None, test_steps=test_steps, opacity_thresh=0.7)
    finally:
        torch.Tensor.cuda = old_cuda
    assert add[0].shape[0] == 0
    return visited, np.asarray(model.opt.query_size), model.top_ray_miss_ids.numpy().copy(), model.top_ray_miss_loss.numpy().copy()


def main():
    import_reference()
    import models.base_rendering_model as brm
    Model = reference_model_class()
    rng = np.random.default_rng(20241)
    model, model1 = new_model(Model), new_model(Model, prob_num_step=1)
    n = TRAIN_LEN // NUM_STEP + 1
    assert model.top_ray_miss_ids.tolist() == list(range(n)) and model.top_ray_miss_ids.dtype == torch.int32 and model.top_ray_miss_loss.shape == (n,)
    assert model1.top_ray_miss_loss.shape == (1,) and getattr(model1, "top_ray_miss_ids", None) is None

    # total_steps on both sides of the two tiers: 39990 .. 40009, then 119966 .. 120005 (the last five lie behind the last tier: no update)
    total_steps = np.array([39990 + k if k < 20 else 119966 + (k - 20) for k in range(STEPS)], np.int64)
    first = [12, 5, 20, 33, 7, 15, 28, 3, 39, 18, 25, 9, 31, 36]          # 14 frames with missed rays: the table fills with positive entries, then evicts
    seen = dict(no_miss=0, all_miss=0, present_smaller=0, absent_zero=0, evict_full=0)
    rec = dict(color=[], gt=[], ray_mask=[], frame=[], loss=[], ids=[], losses=[], n1=[])
    for k in range(STEPS):
        ids, losses = model.top_ray_miss_ids.numpy(), model.top_ray_miss_loss.numpy()
        absent = [f for f in range(TRAIN_LEN) if f not in ids.tolist()]
        if k < len(first):
            frame, p = first[k], float(rng.uniform(0.15, 0.9))
        elif k == 14:
            frame, p = int(ids[0]), 0.04                                   # the worst frame comes back with fewer misses
        elif k == 15:
            frame, p = absent[3], 0.0                                      # an absent frame without a missed ray
        elif k == 16:
            frame, p = absent[5], 1.0                                      # every ray missed
        elif k in (22, 37):
            frame, p = int(ids[int(rng.integers(0, n))]), 0.0
        else:
            frame, p = int(rng.integers(0, TRAIN_LEN)), float(rng.uniform(0.0, 0.8))
        color, gt, mask = make_batch(rng, p)
        loss = ray_miss_loss(brm, color, gt, mask)
        assert loss.dtype == torch.float32 and loss.dim() == 0
        n_miss = int((mask == 0).sum())
        gated = not (total_steps[k] <= TIERS[-1])
        if not gated:
            present = frame in ids.tolist()
            seen["no_miss"] += n_miss == 0
            seen["all_miss"] += n_miss == R
            seen["present_smaller"] += bool(present and float(loss) < float(losses[ids.tolist().index(frame)] if present else 0.0))
            seen["absent_zero"] += bool(not present and float(loss) == 0.0)
            seen["evict_full"] += bool(not present and (losses > 0).all() and float(loss) > 0)
        for m in (model, model1):
            m.input = {"id": torch.tensor([frame])}
            m.loss_ray_miss_coarse_raycolor = loss
            m.update_rank_ray_miss(int(total_steps[k]))
        if gated:
            assert np.array_equal(ids, model.top_ray_miss_ids.numpy()) and np.array_equal(losses, model.top_ray_miss_loss.numpy())
        pos = model.top_ray_miss_loss.numpy()
        pos = np.sort(pos[pos > 0].astype(np.float64))
        assert pos.size < 2 or np.min(np.diff(pos) / pos[1:]) > 1e-4, "two positive losses too close for the tolerance: draw another sequence"
        for key, v in (("color", color), ("gt", gt), ("ray_mask", mask), ("frame", frame), ("loss", float(loss)), ("ids", model.top_ray_miss_ids.numpy().copy()),
                       ("losses", model.top_ray_miss_loss.numpy().copy()), ("n1", float(model1.top_ray_miss_loss[0]))):
            rec[key].append(v)
    final_ids, final_losses = rec["ids"][-1], rec["losses"][-1]
    assert int((final_losses > 0).sum()) >= 8, final_losses
    assert all(v >= 1 for v in seen.values()), seen

    # the tier gate of update_rank_ray_miss (:155) at steps around both tiers, with the shipped tiers and with prob_kernel_size None
    gate_steps = np.array([1, 39999, 40000, 40001, 119999, 120000, 120001, 500000], np.int64)
    gate = {}
    for tag, kernel in (("shipped", KERNEL), ("none", None)):
        opened = []
        for s in gate_steps:
            m = new_model(Model, kernel=kernel)
            m.input, m.loss_ray_miss_coarse_raycolor = {"id": torch.tensor([20])}, torch.tensor(0.5)
            m.update_rank_ray_miss(int(s))
            opened.append(bool(m.top_ray_miss_loss[0] > 0))
        gate[tag] = np.array(opened)
    assert gate["shipped"].tolist() == [True] * 6 + [False] * 2 and gate["none"].all()

    # the grow pass's frame list (take_top), the query_size per tier and the reset behind the pass
    out = {}
    for s in (30000, 50000):
        visited, qs, ids_after, losses_after = probe_frames(Model, (final_ids, final_losses), s)
        out["probe_%d_frames" % s], out["probe_%d_query_size" % s] = np.array(visited, np.int32), qs.astype(np.int32)
        assert ids_after.tolist() == list(range(n)) and not losses_after.any()
    assert np.array_equal(out["probe_30000_frames"], out["probe_50000_frames"]) and len(out["probe_30000_frames"]) >= 8
    out.update(color=np.stack(rec["color"]), gt=np.stack(rec["gt"]), ray_mask=np.stack(rec["ray_mask"]), frame=np.array(rec["frame"], np.int32),
               total_steps=total_steps, loss=np.array(rec["loss"], np.float32), ids=np.stack(rec["ids"]).astype(np.int32),
               losses=np.stack(rec["losses"]).astype(np.float32), n1_losses=np.array(rec["n1"], np.float32),
               gate_steps=gate_steps, gate_shipped=gate["shipped"], gate_none=gate["none"], prob_tiers=np.array(TIERS, np.int64),
               prob_kernel_size=np.array(KERNEL, np.int32), train_len=np.array([TRAIN_LEN]), prob_num_step=np.array([NUM_STEP]),
               reset_ids=ids_after.astype(np.int32), reset_losses=losses_after.astype(np.float32))
    path = os.path.join(HERE, "growth_rank.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 100000, size
    print("wrote %s (%d bytes): %d steps, cases %s, %d positive entries at the end, frames %s" % (
        path, size, STEPS, {k: int(v) for k, v in seen.items()}, int((final_losses > 0).sum()), out["probe_30000_frames"].tolist()))


if __name__ == "__main__":
    main()
