"""CPU checks of the frame bank's batch sampler: the NumPy restatement (tests/frames_ref.py) against published Philox vectors and against the
dataset items the reference itself produced (tests/golden/frames.npz, written by tests/golden/make_golden_frames.py), and the host-side
nearest-view tables of hybridneuralrendering_amd/frames.py.  No library, no GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import frames_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "frames.npz")))


def test_philox_known_answers():
    """Philox4x32-10 of the Random123 distribution (kat_vectors): counter, key -> words."""
    hexw = lambda w: " ".join("%08x" % int(x) for x in w)
    assert hexw(R.philox4x32((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert hexw(R.philox4x32((0xffffffff,) * 4, (0xffffffff,) * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert hexw(R.philox4x32((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    # vectorised over the index, and the (seed, step) split into words
    w = R.words((0x299f31d0 << 32) | 0xa4093822, (0x85a308d3 << 32) | 0x243f6a88, 0x13198a2e, np.array([0x03707344, 0]))
    assert hexw([x[0] for x in w]) == "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_randint_stays_in_range():
    u = np.array([0, 1, 0x7fffffff, 0x80000000, 0xfffffffe, 0xffffffff], np.uint64)
    for lo, hi in ((3, 61), (0, 1 << 16), (-5, 7)):
        r = R.randint(u, lo, hi)
        assert r.min() == lo and r.max() == hi - 1 and (r >= lo).all() and (r < hi).all()
    assert (R.randint(u, 9, 10) == 9).all()                                     # a one-wide range
    with pytest.raises(AssertionError):
        R.randint(u, 4, 4)


def test_random_mode_covers_exactly_the_window():
    """20 000 steps of a 20 x 30 window (H = 26, W = 36, margin 3): every pixel of the window occurs, none outside it."""
    H, W, m = 26, 36, 3
    steps = np.arange(20000)
    w = R.words(11, steps, R.PURPOSE_RANDOM, 0)
    px, py = R.randint(w[0], m, W - m), R.randint(w[1], m, H - m)
    hit = np.zeros((H, W), bool)
    hit[py, px] = True
    want = np.zeros((H, W), bool)
    want[m:H - m, m:W - m] = True
    assert np.array_equal(hit, want)
    # ... and sample_pixels draws the same words ray by ray
    qx, qy, _ = R.sample_pixels("random", 11, 5, H, W, m, size=7)
    w5 = R.words(11, 5, R.PURPOSE_RANDOM, np.arange(49))
    assert np.array_equal(qx, R.randint(w5[0], m, W - m)) and np.array_equal(qy, R.randint(w5[1], m, H - m)) and len(qx) == 49


def test_dilated_patches_stay_inside_the_margin_and_the_table_rebuilds_the_pixels():
    H, W, m, pn, ps, dlo, dhi = 48, 64, 3, 3, 4, 1, 3
    seen = set()
    for step in range(300):
        px, py, tab = R.sample_pixels("dilated", 5, step, H, W, m, dilation_setup="3_4_1_3")
        assert tab.shape == (pn * pn, 3) and tab.dtype == np.int32
        assert (px >= m).all() and (px < W - m).all() and (py >= m).all() and (py < H - m).all()
        seen.update(int(d) for d in tab[:, 0])
        grid_x, grid_y = px.reshape(pn * ps, pn * ps), py.reshape(pn * ps, pn * ps)
        for pi in range(pn):
            for pj in range(pn):
                d, x0, y0 = (int(v) for v in tab[pi * pn + pj])
                assert dlo <= d <= dhi
                assert x0 + (ps - 1) * d < W - m and y0 + (ps - 1) * d < H - m
                bx, by = np.meshgrid(x0 + d * np.arange(ps), y0 + d * np.arange(ps))
                assert np.array_equal(grid_x[pi * ps:(pi + 1) * ps, pj * ps:(pj + 1) * ps], bx)
                assert np.array_equal(grid_y[pi * ps:(pi + 1) * ps, pj * ps:(pj + 1) * ps], by)
    assert seen == {1, 2, 3}                                                    # every d in [dlo, dhi]
    # the same layout as scenes.dilated_patch_batch builds from a table of (d, x0, y0)
    px, py, tab = R.sample_pixels("patch", 5, 3, H, W, m, size=8)
    assert tab.shape == (1, 3) and tab[0, 0] == 1
    assert np.array_equal(px.reshape(8, 8), np.broadcast_to(tab[0, 1] + np.arange(8), (8, 8)))
    assert np.array_equal(py.reshape(8, 8), np.broadcast_to(tab[0, 2] + np.arange(8)[:, None], (8, 8)))


def test_bg_random_takes_both_values():
    vals = {float(R.bg_random(3, s)[0]) for s in range(64)}
    assert vals == {0.0, 1.0}


def _golden_banks(g):
    train = R.RefBank(g["train_images"], g["train_c2w"], g["K"], np.linalg.inv(g["train_c2w"].astype(np.float64)).astype(np.float32), ids=g["train_ids"],
                      weights=g["weights"], weight_exp=float(g["weight_exp"][0]), total_num_image=int(g["total_num_image"][0]))
    test = R.RefBank(g["test_images"], g["test_c2w"], g["K"], np.linalg.inv(g["test_c2w"].astype(np.float64)).astype(np.float32), ids=g["test_ids"],
                     total_num_image=int(g["total_num_image"][0]))
    train.set_nearest(g["nearest_train_shq0"])
    test.set_nearest(g["nearest_test_shq0"], reference=train)
    return train, test


def test_nearest_by_id_equals_the_reference_picks(gold):
    from hybridneuralrendering_amd import frames
    g = gold
    V = int(g["V"][0])
    for split, exclude in (("train", True), ("test", False)):
        ids = g[split + "_ids"]
        got = frames.nearest_by_id(ids, g["train_ids"], V, exclude_self=exclude)
        ref = g["nearest_%s_shq0" % split]
        assert got.dtype == np.int32 and got.shape == ref.shape
        for q, vid in enumerate(ids):
            assert set(got[q]) == set(ref[q]), (split, vid)
            dist = np.abs(g["train_ids"] - vid)[ref[q]]
            if len(set(dist)) == V:                                             # no two distances equal: the order is the reference's too
                assert list(got[q]) == list(ref[q]), (split, vid)
        # select_high_quality: the weights are distinct, so the order inside the candidate set is decided
        got = frames.nearest_by_id(ids, g["train_ids"], V, exclude_self=exclude, weights=g["weights"], select_high_quality=True)
        assert np.array_equal(got, g["nearest_%s_shq1" % split]), split
    assert list(frames.nearest_by_id([15], [0, 5, 10, 15, 20, 25, 30], 4, exclude_self=True)[0]) == [2, 4, 1, 5]    # frames 10, 20, 5, 25
    with pytest.raises(frames.HnrError):
        frames.nearest_by_id([15], [0, 5, 10], 4, exclude_self=True)
    with pytest.raises(frames.HnrError):
        frames.nearest_by_id([15], [0, 5, 10, 15, 20, 25], 4, exclude_self=True, dynamic_nearest=True)


def test_nearest_by_pose_equals_the_reference_picks(gold):
    from hybridneuralrendering_amd import frames
    g = gold
    V, (w, h) = int(g["V"][0]), (int(x) for x in g["ring_wh"])
    tids = np.arange(g["ring_c2w"].shape[0])
    q = g["ring_query_train"]
    got = frames.nearest_by_pose(g["ring_c2w"][q], g["ring_K"], q, g["ring_pos"], g["ring_dirs"], tids, V, w, h, is_train=True)
    assert np.array_equal(got, g["ring_picks_train"])
    assert all(int(q[i]) not in got[i] for i in range(len(q)))
    nt = g["ring_test_c2w"].shape[0]
    got = frames.nearest_by_pose(g["ring_test_c2w"], g["ring_K"], np.arange(nt), g["ring_pos"], g["ring_dirs"], tids, V, w, h, is_train=False)
    assert np.array_equal(got, g["ring_picks_test"])


def test_restatement_reproduces_the_reference_items(gold):
    """From the golden's own pixel_idx: gt_image, images_nearest, the poses, float32 of the weights and angles bit for bit; raydir within raydir_tol
    (the reference multiplies by the rotation through BLAS, so its last bit is not the sequential one)."""
    g = gold
    train, test = _golden_banks(g)
    tol = float(g["raydir_tol"][0])
    assert 0 < tol < 1e-6
    n_items = 0
    for case in g["item_cases"]:
        bank, row = (train if case.startswith("train") else test), int(case[-1])
        base = "item_" + str(case)
        for mode in ("random", "random_norm", "patch", "dilated", "no_crop"):
            pix = g["%s_%s_pixel_idx" % (base, mode)]
            it = R.item(bank, row, pix[:, 0], pix[:, 1], dir_norm=mode.endswith("_norm"), downweight=True)
            assert np.array_equal(it["gt_image"], g["%s_%s_gt_image" % (base, mode)]), (case, mode)
            assert np.array_equal(it["pixel_idx"], pix)
            rd = g["%s_%s_raydir" % (base, mode)]
            assert it["raydir"].dtype == np.float32 and np.abs(it["raydir"].astype(np.float64) - rd).max() <= tol, (case, mode)
            n_items += 1
        assert np.array_equal(it["images_nearest"], g[base + "_images_nearest"]) and it["images_nearest"].dtype == np.float32
        assert np.array_equal(it["c2w_nearest"], g[base + "_c2w_nearest"]) and np.array_equal(it["campos_nearest"], g[base + "_campos_nearest"])
        assert np.array_equal(it["campos"], g[base + "_campos"]) and np.array_equal(it["camrotc2w"], g[base + "_camrotc2w"]) and np.array_equal(it["c2w"], g[base + "_c2w"])
        assert np.array_equal(it["frame_weight"], g[base + "_frame_weight"].astype(np.float32))
        assert np.array_equal(it["frame_weight_nearest"], g[base + "_frame_weight_nearest"].astype(np.float32))
        assert np.array_equal(it["vid_angle_nearest"], g[base + "_vid_angle_nearest"].astype(np.float32))
        assert np.array_equal(R.item(bank, row, pix[:, 0], pix[:, 1])["frame_weight_nearest"], np.ones((4,), np.float32))
    assert n_items == 15
    # the no_crop item is the scan-line window
    m = int(g["margin"][0])
    px, py = R.no_crop_pixels(48, 64, m)
    assert np.array_equal(np.stack([px, py], -1).astype(np.float32), g["item_train0_no_crop_pixel_idx"])
    assert g["train_images"].min() == 0 and g["train_images"].max() == 255


def test_frame_structs_have_the_layout_of_the_c_header(tmp_path):
    """hnr_frame_bank / hnr_frame_batch_params / hnr_frame_batch_out as a C compiler lays them out equal the ctypes mirrors in _lib.py."""
    from hybridneuralrendering_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    pairs = [("hnr_frame_bank", _lib.FrameBankC), ("hnr_frame_batch_params", _lib.FrameBatchParams), ("hnr_frame_batch_out", _lib.FrameBatchOut)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hnr.h"', 'int main(void) {']
    for cname, cls in pairs:
        lines.append('  printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {}
    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        a, b, c = ln.split()
        got[(a, b)] = int(c)
    for cname, cls in pairs:
        assert got[(cname, "sizeof")] == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert got[(cname, fname)] == getattr(cls, fname).offset, (cname, fname)
