"""The growth schedule's bookkeeping, CPU side: tests/growth_ref.py (the NumPy restatement of csrc/rank.hip and growth.RayMissRanking / probe_tier)
against tests/golden/growth_rank.npz, which holds what the reference's own compute_losses, rank_ray_miss, update_rank_ray_miss, setup,
reset_ray_miss_ranking and probe_hole returned on a recorded sequence (tests/golden/make_golden_growth.py)."""
import os

import numpy as np
import pytest

from tests import growth_ref as G
from tests.golden_io import GOLD


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "growth_rank.npz"))


def replay(z, update):
    """Feeds the recorded sequence to `update(k, frame) -> (ids, losses, loss)` and checks it against the reference after every step: the ids of the
    positive prefix equal, the losses within the float32-reduction bound.  Zero-loss entries are not compared: their order is the open tie."""
    R = z["ray_mask"].shape[1]
    tol = G.loss_tolerance(R)
    for k in range(z["frame"].shape[0]):
        ids, losses, loss = update(k)
        want_ids, want = z["ids"][k], z["losses"][k]
        npos = int((want > 0).sum())
        assert int((np.asarray(losses) > 0).sum()) == npos, k
        np.testing.assert_array_equal(np.asarray(ids)[:npos], want_ids[:npos], err_msg="step %d" % k)
        np.testing.assert_allclose(np.asarray(losses)[:npos], want[:npos], rtol=tol, atol=0, err_msg="step %d" % k)
        np.testing.assert_allclose(float(loss), float(z["loss"][k]), rtol=tol, atol=0, err_msg="step %d" % k)
        assert (float(loss) == 0.0) == (float(z["loss"][k]) == 0.0)


def test_golden_sequence_holds_every_case(gold):
    z = gold
    n = int(z["train_len"][0]) // int(z["prob_num_step"][0]) + 1
    assert z["ids"].shape == (60, n) and n == 11 and z["ray_mask"].shape == (60, 49)
    miss = (z["ray_mask"] == 0).sum(1)
    assert (miss == 0).any() and (miss == 49).any()
    assert int((z["losses"][-1] > 0).sum()) >= 8
    assert (z["total_steps"] <= 40000).any() and (z["total_steps"] > 40000).any() and (z["total_steps"] > 120000).any()


def test_restated_ranking_matches_reference_after_every_step(gold):
    z = gold
    state = {"t": G.new_table(int(z["train_len"][0]), int(z["prob_num_step"][0])), "one": G.new_table(int(z["train_len"][0]), 1)}
    assert state["one"][1].shape == (1,)

    def update(k):
        L, n_miss = G.ray_miss_loss(z["color"][k], z["gt"][k], z["ray_mask"][k])
        assert n_miss == int((z["ray_mask"][k] == 0).sum())
        if G.probe_tier(int(z["total_steps"][k]), z["prob_tiers"], z["prob_kernel_size"]) is not None:
            state["t"] = G.rank_update(*state["t"], int(z["frame"][k]), L)
            state["one"] = G.rank_update(*state["one"], int(z["frame"][k]), L)
        np.testing.assert_allclose(state["one"][1][0], z["n1_losses"][k], rtol=G.loss_tolerance(49), atol=0)
        return state["t"][0], state["t"][1], L

    replay(z, update)
    ids, losses = state["t"]
    frames = G.top_frames(ids, losses, int(z["train_len"][0]) // int(z["prob_num_step"][0]))
    assert frames == z["probe_30000_frames"].tolist() == z["probe_50000_frames"].tolist()
    r_ids, r_losses = G.new_table(int(z["train_len"][0]), int(z["prob_num_step"][0]))
    np.testing.assert_array_equal(r_ids, z["reset_ids"])
    np.testing.assert_array_equal(r_losses, z["reset_losses"])


def test_restated_tier_gate_matches_reference(gold):
    z = gold
    ks = z["prob_kernel_size"].tolist()
    for s, shipped, none in zip(z["gate_steps"], z["gate_shipped"], z["gate_none"]):
        assert (G.probe_tier(int(s), z["prob_tiers"], ks) is not None) == bool(shipped), s
        assert (G.probe_tier(int(s), z["prob_tiers"], None) is not None) == bool(none), s
    assert G.probe_tier(30000, z["prob_tiers"], ks) == (0, z["probe_30000_query_size"].tolist())
    assert G.probe_tier(50000, z["prob_tiers"], ks) == (1, z["probe_50000_query_size"].tolist())
    assert G.probe_tier(120001, z["prob_tiers"], ks) is None
    assert G.probe_tier(10 ** 9, z["prob_tiers"], None) == (0, None)


def test_package_probe_tier_equals_the_restatement(gold):
    from hybridneuralrendering_amd import growth
    z = gold
    ks = z["prob_kernel_size"].tolist()
    for s in list(z["gate_steps"]) + [0, 40000, 40001, 120000, 120001]:
        for kernel in (ks, None, " 3 3 3 1 1 1 ".split(), [3, 3, 3]):
            want = G.probe_tier(int(s), z["prob_tiers"], None if kernel is None else [int(v) for v in kernel])
            assert growth.probe_tier(int(s), z["prob_tiers"].tolist(), kernel) == want, (s, kernel)


def test_restated_table_edges():
    ids, losses = G.new_table(8, 4)                                            # 3 slots: frames 0, 1, 2 present with loss 0
    assert ids.tolist() == [0, 1, 2] and losses.tolist() == [0, 0, 0]
    ids, losses = G.rank_update(ids, losses, 7, 0.0)                           # absent, loss 0: lands in the last slot
    assert ids.tolist() == [0, 1, 7]
    ids, losses = G.rank_update(ids, losses, 1, 0.5)
    ids, losses = G.rank_update(ids, losses, 7, 0.5)                           # equal positive losses keep their slot order
    assert ids.tolist() == [1, 7, 0] and losses.tolist() == [0.5, 0.5, 0.0]
    ids, losses = G.rank_update(ids, losses, 1, 0.25)                          # present with a smaller loss: keeps the larger
    assert ids.tolist() == [1, 7, 0] and losses.tolist() == [0.5, 0.5, 0.0]
    ids, losses = G.rank_update(ids, losses, 5, 0.125)                         # absent: overwrites the last slot although it is the smallest
    assert ids.tolist() == [1, 7, 5]
    keep = (ids.copy(), losses.copy())
    ids, losses = G.rank_update(ids, losses, 1, np.float32("nan"))             # a non-finite loss leaves the table as it was
    assert np.array_equal(ids, keep[0]) and np.array_equal(losses, keep[1])
    assert G.top_frames(ids, losses, 2) == [1, 7] and G.top_frames(ids, losses, 1) == [1]
    L, n = G.ray_miss_loss(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0,)))
    assert L == 0 and n == 0
