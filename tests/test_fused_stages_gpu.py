"""The fused per-sample stages of csrc/mlp.hip through the C ABI against float64 restatements (tests/image_branch_ref.py: merge_stage_ref, mixup_ref;
their inputs are checked without a GPU in tests/test_image_branch.py):

 * hnr_merge_stage at V = 4 (merge_wp_kernel: reprojection, gather, 48 -> 64 -> 64 -> 64 merge-weight MLP with the per-sample addend, 64 -> 1
   sigmoid, merge over the views) on the hand-built pixel table and on generated sets of 1 .. 1100 samples and 96 CUs + 5 samples (the grid-stride
   tile loop); frame weights None / ones / with a zero; the same cases with mix-up rows of stride 90, which run mlp3_kernel<3,4,4,0,1,2> and must
   give the same bits; HNR_MERGE_RT = 2 and 4 in child processes (the knob is read once per process);
 * hnr_mixup_stage (mixfinal_wp_kernel) at 1 .. 384 CUs + 7 samples against float64 and, bit for bit, against hnr_mlp3_forward + hnr_final_color.

Bounds: merged columns |got - fp64| <= 4 e32 + 3e-7 with e32 = max |the same restatement in float32 on the CPU - fp64| (4: another summation order, as
for hnr_merge in tests/test_image_branch_gpu.py; 3e-7: the 22-bit split arithmetic, as in tests/test_mlp3_gpu.py); mix-up rows 2.5 e32 + 3e-7 relative
to the row maximum; colours 4 e32 + 1e-7.  Every test prints e32, the error and their ratio.

Physical rows differ from logical ones throughout (cap = n + 13, samples at permuted items); everything beyond the device count is NaN on the way in
and a sentinel on the way out.

Values recorded on an MI355X (256 CUs; profiles/fused_stage_tests.txt):
  hnr_merge_stage, 16 sets x 2 frame weights x 2 kernel forms: e32 1.5e-7 .. 3.6e-6, error 1.0e-7 .. 3.1e-6 (the largest at the 24 581-sample
  grid-stride case), at most 2.35 x e32 and 0.39 of the bound; the two forms equal bit for bit in every run, and so are HNR_MERGE_RT = 2 and 4
  (error at most 1.00 x e32 there);
  hnr_mixup_stage, 1 .. 98 311 samples: rows 1.6e-7 .. 6.4e-7 of the row maximum (at most 1.24 x e32), colours 4.5e-8 .. 1.1e-7 (at most 1.04 x e32);
  decoded rows and mix-up rows equal to hnr_mlp3_forward + hnr_final_color bit for bit at every size.
No case exceeded its bound, so no kernel was changed.  Four arithmetic-only edits of csrc/mlp.hip were tried against this module and
tests/test_mlp3_gpu.py on scratch builds (never committed); each fails here:
  frame-weight index rotated in merge_wp_kernel ((j + 1) & 3)   test_merge_stage_zero_frame_weight_equals_a_view_that_looks_away, and the two-form
                                                                 equality / fp64 bound of test_merge_stage_matches_... with a zero weight
  columns 90, 91 not zeroed in mixfinal_wp_kernel                test_mixup_stage_matches_fp64_and_its_two_kernel_form (all six sizes: NaN rows)
  layer-0 addend left out in merge_wp_kernel                     test_merge_stage_matches_the_fp64_restatement_in_both_kernel_forms (every set)
  tail layer reading layer 2's bias row                          test_mlp3_color_feature_tail_both_outputs_against_fp64 (tests/test_mlp3_gpu.py)
"""
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import image_branch_ref as ib
from tests.test_image_branch_gpu import _sample_buffers, _random_featmap, _t, PAD, SENT_F, CAMPOS, CNT_VALID

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _dev():
    return torch.device("cuda:0")


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _padded(x, cap):
    out = torch.full((cap,) + tuple(x.shape[1:]), NAN)
    out[:x.shape[0]] = x
    return _t(out)


# ================================================================================================ hnr_merge_stage
def _merge_key(name):
    """Case name -> arguments of ib.fused_merge_case."""
    if name == "edge":
        return (0, None)
    if name == "grid":
        return (96 * _cus() + 5, (48, 64), 1100)                       # more tiles than 12 waves x CUs: the grid-stride loop
    n, hw = name[1:].split("_")
    return (int(n), tuple(int(a) for a in hw.split("x")))


@functools.lru_cache(maxsize=None)
def _merge_device(key):
    """Device buffers of a case, built once and never written: samples at permuted items of loc_w, NaN beyond the count."""
    from hybridneuralrendering_amd.linear import FusedMlp3
    c = ib.fused_merge_case(*key)
    assert np.array_equal(c["campos"], CAMPOS)
    n = c["n"]
    cap = n + PAD
    loc, vs, counts = _sample_buffers(c["xyz"], n)
    d = dict(loc=loc, vs=vs, counts=counts, w2c=_t(c["w2c"]), K=_t(c["K"]), campos=_t(c["campos"]), campos_n=_t(c["campos_n"]), fm=_t(c["fm"]),
             pre=_padded(c["pre"], cap), CF=_padded(c["CF"], cap), w_last=_t(c["w_last"]), b_last=_t(c["b_last"]))
    d["mlp"] = FusedMlp3([_t(w) for w in c["Ws"]], [None if b is None else _t(b) for b in c["bs"]], (1, 1, 1))
    return c, d


def _run_merge(c, d, frame_w=None, ld7=92, **over):
    """One hnr_merge_stage call on a sentinel-filled X7 [cap, ld7]; `over` replaces device operands (w2c=..., fm=..., counts=...)."""
    from hybridneuralrendering_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    a = dict(d, **over)
    cap = c["n"] + PAD
    X7 = torch.full((cap, ld7), SENT_F, device=_dev())
    fw = _t(frame_w) if frame_w is not None else None
    _lib.check(L.hnr_merge_stage(p(a["loc"]), p(a["vs"]), p(a["counts"]), p(a["w2c"]), p(a["K"]), p(a["campos"]), p(a["campos_n"]), p(a["fm"]), 4, c["H"],
                                 c["W"], p(fw), p(a["pre"]), 64, p(a["mlp"].packed), p(a["w_last"]), p(a["b_last"]), p(a["CF"]), 128, cap, float(c["slope"]),
                                 p(X7), ld7, _lib.stream()), "hnr_merge_stage")
    torch.cuda.synchronize()
    return X7.cpu()


def _check_merge_rows(c, X7, ld7, pads_written):
    """The exact part: colour-feature columns copied, nothing beyond the count, padding columns zero where the kernel form writes them."""
    n = c["n"]
    assert torch.equal(X7[:n, :45], c["CF"][:, :45])
    assert bool((X7[n:] == SENT_F).all())
    if ld7 > 90:
        assert bool((X7[:n, 90:92] == (0.0 if pads_written else SENT_F)).all()) and bool((X7[:n, 92:] == SENT_F).all())
    return X7[:n, 45:90]


def _merge_error(what, c, got, frame_w, refs=None):
    r64, r32 = refs or ib.fused_merge_refs(c, frame_w)
    e32, bound = ib.merge_bound(r64, r32)
    err = float((got.double() - r64["merged"]).abs().max())
    print("merge_stage %s: e32 = %.3e  max |got - fp64| = %.3e  (%.2f x e32; bound %.3e)" % (what, e32, err, err / max(e32, 1e-30), bound))
    return e32, err, bound


MERGE_SETS = ["edge"] + ["n%d_%dx%d" % (n, hw[0], hw[1]) for n, hw in ib.FUSED_CASES] + ["grid"]


@pytest.mark.parametrize("name", MERGE_SETS)
def test_merge_stage_matches_the_fp64_restatement_in_both_kernel_forms(name):
    """Wave-per-tile form (ld7 = 92) and mlp3_kernel<3,4,4,0,1,2> (ld7 = 90: rows that cannot leave as 16-byte chunks) on the same operands: each
    within the fp64 bound, equal to each other bit for bit on columns 0..89 (csrc/mlp.hip: "element for element")."""
    c, d = _merge_device(_merge_key(name))
    n = c["n"]
    r64, r32 = ib.fused_merge_refs(c)
    valid = r64["valid"]
    sd = float(r64["logits"].std())
    assert 0.5 <= sd <= 3.0, sd                                                      # the sigmoid is not saturated: a wrong logit shows
    fw0, z, n_only = ib.frame_weights_with_a_zero(valid)
    if name == "grid":
        assert n > 96 * _cus() and (n + 7) // 8 > 12 * _cus()
        for w in (None, fw0):
            b, d_hidden, d_swap = ib.merge_sensitivity(c, w)
            assert d_hidden > 100 * b and d_swap > 100 * b, (d_hidden, d_swap, b)
    worst = []
    for tag, fw in (("frame_w=None", None), ("frame_w with a zero at view %d" % z, fw0)):
        refs = (r64, r32) if fw is None else ib.fused_merge_refs(c, fw)
        X = {ld7: _run_merge(c, d, fw, ld7) for ld7 in (92, 90)}
        for ld7, form in ((92, "wave-per-tile"), (90, "mlp3<3,4,4,0,1,2>")):
            got = _check_merge_rows(c, X[ld7], ld7, True)
            e32, err, bound = _merge_error("%s %s %s" % (name, form, tag), c, got, fw, refs)
            worst.append((err <= bound, name, form, tag, err, e32, bound))
            # merged to exactly 0: masked in all four views, or unmasked only in views of frame weight 0
            none = (valid.float() * (1.0 if fw is None else fw[:, None])).sum(0) == 0
            if n >= 37 or name == "edge":
                assert bool((~valid.any(0)).any()) and (fw is None or name == "edge" or int((none & valid.any(0)).sum()) == n_only >= 1)
            assert bool((got[none] == 0).all()), (name, form, tag)
            assert float(got[~none].abs().max()) > 0 if bool((~none).any()) else True
        same = X[92][:n, :90] == X[90][:n, :90]
        assert bool(same.all()), (name, tag, "the two kernel forms differ at (sample, column)", (~same).nonzero()[:4].tolist(),
                                  float((X[92][:n, :90] - X[90][:n, :90]).abs().max()))
        if fw is None:                                                                # unit weights are no weights: the same bits
            assert torch.equal(_run_merge(c, d, torch.ones(4), 92), X[92]) and torch.equal(_run_merge(c, d, torch.ones(4), 90), X[90])
    assert all(w[0] for w in worst), [w[1:] for w in worst if not w[0]]


@pytest.mark.parametrize("n", [37, 97])
def test_merge_stage_zero_frame_weight_equals_a_view_that_looks_away(n):
    """frame_w[v] = 0 against the same call with camera v replaced by one that sees nothing (every row masked) and weight 1: adding f x 0 and 0 is
    exact, so the rows are equal bit for bit -- which pins the view index of frame_w, w2c and campos_nearest (a rotated index moves the zero to
    another view).  On a feature map of its own, in both kernel forms."""
    c, d = _merge_device(_merge_key("n%d_37x51" % n))
    fm = _t(_random_featmap(4, c["H"], c["W"], 500 + n))
    away = np.zeros((4, 4), np.float32)
    away[0, 3], away[2, 3], away[3, 3] = -1.0e6, 1.0, 1.0                              # camera coordinates (-1e6, 0, 1) for every point: fx far below 0
    base = {ld7: _run_merge(c, d, None, ld7, fm=fm) for ld7 in (92, 90)}
    seen = set()
    for v in range(4):
        fw = torch.tensor([0.75, 1.25, 0.5, 1.5])
        fw[v] = 0.0
        fw1 = fw.clone()
        fw1[v] = 1.0
        w2c = c["w2c"].copy()
        w2c[v] = away
        assert bool((ib.restated_pixels(c["xyz"], w2c, c["K"], c["H"], c["W"])[v] == -1).all())
        for ld7 in (92, 90):
            a = _run_merge(c, d, fw, ld7, fm=fm)
            b = _run_merge(c, d, fw1, ld7, fm=fm, w2c=_t(w2c))
            assert torch.equal(a, b), (n, v, ld7)
            assert not torch.equal(a, base[ld7])
            seen.add(hashlib.sha1(a[:, :90].contiguous().numpy().tobytes()).hexdigest())
    assert len(seen) == 4                                                             # four different zeros, four different results (the same in both forms)


def test_merge_stage_with_no_valid_sample_writes_nothing():
    c, d = _merge_device(_merge_key("n37_48x64"))
    zero = torch.zeros((16,), dtype=torch.int64, device=_dev())
    for ld7 in (92, 90):
        assert bool((_run_merge(c, d, None, ld7, counts=zero) == SENT_F).all())


def _child_cases():
    """What a child process of the HNR_MERGE_RT test runs and prints; the parent calls it too (RT = 1: the wave-per-tile form)."""
    out = []
    for n in ib.FUSED_CHILD_N:
        c, d = _merge_device((n, ib.FUSED_CHILD_HW))
        valid = ib.fused_merge_refs(c)[0]["valid"]
        for k, fw in enumerate((None, ib.frame_weights_with_a_zero(valid)[0])):
            X = _run_merge(c, d, fw, 92)
            got = X[:c["n"], 45:90]
            r64, r32 = ib.fused_merge_refs(c, fw)
            e32, bound = ib.merge_bound(r64, r32)
            err = float((got.double() - r64["merged"]).abs().max())
            exact = torch.equal(X[:c["n"], :45], c["CF"][:, :45]) and bool((X[c["n"]:] == SENT_F).all())
            out.append((n, k, e32, err, int(exact), hashlib.sha1(X[:c["n"], :90].contiguous().numpy().tobytes()).hexdigest()))
    return out


_CHILD = r'''
import sys
sys.path.insert(0, sys.argv[1])
from tests import test_fused_stages_gpu as T
for rec in T._child_cases():
    print("FUSED_RT %d %d %.9e %.9e %d %s" % rec)
'''


@pytest.mark.parametrize("rt", [2, 4])
def test_merge_stage_workgroup_per_tile_forms_in_a_child_process(rt, tmp_path):
    """HNR_MERGE_RT = 2 / 4 select mlp3_kernel<3,4,4,0,1,2> / <3,4,4,0,1,4> for rows of stride 92 too; the knob is read once per process, so each
    runs in a fresh child (n = 1, 33, 1100; frame weights None and with a zero) and prints its figures; the parent holds them to the fp64 bound."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "fused_rt.py"
    script.write_text(_CHILD)
    p = subprocess.run([sys.executable, str(script), root], capture_output=True, text=True, timeout=300, env=dict(os.environ, HNR_MERGE_RT=str(rt)))
    assert p.returncode == 0, p.stderr[-2000:]
    recs = [l.split()[1:] for l in p.stdout.splitlines() if l.startswith("FUSED_RT ")]
    assert [(int(r[0]), int(r[1])) for r in recs] == [(n, k) for n in ib.FUSED_CHILD_N for k in (0, 1)], p.stdout[-2000:]
    mine = {(r[0], r[1]): r[5] for r in _child_cases()}
    bad = []
    for n, k, e32, err, exact, sha in recs:
        e32, err = float(e32), float(err)
        bound = ib.MERGE_FACTOR * e32 + ib.MERGE_FLOOR
        print("merge_stage n%s_37x51 HNR_MERGE_RT=%d frame_w=%s: e32 = %.3e  max |got - fp64| = %.3e  (%.2f x e32; bound %.3e)  bits equal to the wave-per-tile form: %s" % (
            n, rt, "None" if k == "0" else "zero", e32, err, err / max(e32, 1e-30), bound, sha == mine[(int(n), int(k))]))
        assert exact == "1", (n, k)
        if not err <= bound:
            bad.append((n, k, err, e32, bound))
    assert not bad, bad


# ================================================================================================ hnr_mixup_stage
def _mix_sizes():
    return [1, 31, 32, 33, 385, 384 * _cus() + 7]                                     # 32-sample tiles, 12 waves; the last one enters the grid-stride loop


@functools.lru_cache(maxsize=None)
def _mix_device(S):
    from hybridneuralrendering_amd.linear import FusedMlp3
    c = ib.fused_mixup_case(S)
    cap, items = S + PAD, S + 7
    rng = np.random.default_rng(S + 3)
    perm = rng.permutation(items).astype(np.int32)
    vs = np.full((cap,), perm[S], np.int32)                                           # entries beyond the count point at an item no sample owns
    vs[:S] = perm[:S]
    assert S < 3 or bool((np.diff(vs[:S]) < 0).any())                                 # not monotonic
    X7 = torch.full((cap, 92), NAN)
    X7[:S, :90] = c["X7"]                                                             # columns 90, 91: what torch.empty may hold
    counts = np.zeros((16,), np.int64)
    counts[CNT_VALID] = S
    d = dict(X7=_t(X7), CF=_padded(c["CF"], cap), sigma=_padded(c["sigma"], cap), vs=_t(vs), counts=_t(counts), w_fin=_t(c["w_fin"].reshape(-1)),
             b_fin=_t(c["b_fin"]), items=items, listed=torch.from_numpy(perm[:S].astype(np.int64)))
    d["mlp"] = FusedMlp3([_t(w) for w in c["Ws"]], [_t(b) for b in c["bs"]], (1, 1, 0))
    return c, d


def _run_mixup(c, d, fused, with_Y=True):
    from hybridneuralrendering_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    S = c["S"]
    cap = S + PAD
    dec = torch.full((d["items"], 4), SENT_F, device=_dev())
    Y = torch.full((cap, 48), SENT_F, device=_dev()) if (with_Y or not fused) else None
    if fused:
        _lib.check(L.hnr_mixup_stage(p(d["X7"]), 92, p(d["mlp"].packed), p(d["CF"]), 128, p(d["w_fin"]), p(d["b_fin"]), p(d["sigma"]), p(d["vs"]), p(d["counts"]),
                                     cap, float(c["slope"]), p(Y), 48 if Y is not None else 0, p(dec), _lib.stream()), "hnr_mixup_stage")
    else:
        d["mlp"](d["X7"], Y, cap, d["counts"], CNT_VALID, 1, slope=float(c["slope"]))
        _lib.check(L.hnr_final_color(p(Y), 48, p(d["CF"]), 128, p(d["w_fin"]), p(d["b_fin"]), p(d["sigma"]), p(d["vs"]), p(d["counts"]), cap, p(dec),
                                     _lib.stream()), "hnr_final_color")
    torch.cuda.synchronize()
    return dec.cpu(), (Y.cpu() if Y is not None else None)


@pytest.mark.parametrize("which", range(6))
def test_mixup_stage_matches_fp64_and_its_two_kernel_form(which):
    S = _mix_sizes()[which]
    c, d = _mix_device(S)
    r64, r32 = ib.fused_mixup_refs(c)
    assert float(r64["pre"].abs().max()) <= 2.0                                       # the colour sigmoid keeps a slope of at least 0.1
    dec, Y = _run_mixup(c, d, True)
    dec_noY, _ = _run_mixup(c, d, True, with_Y=False)
    dec_two, Y_two = _run_mixup(c, d, False)
    listed = d["listed"]
    # ---- exact: densities copied, unlisted items and rows beyond the count untouched, d_Y optional, the two-kernel form bit for bit (include/hnr.h)
    assert torch.equal(dec[listed, 0], c["sigma"])
    other = torch.ones(d["items"], dtype=torch.bool)
    other[listed] = False
    assert int(other.sum()) == 7 and bool((dec[other] == SENT_F).all()) and bool((Y[S:] == SENT_F).all())
    assert torch.equal(dec_noY, dec)
    assert torch.equal(dec_two, dec) and torch.equal(Y_two[:S, :45], Y[:S, :45])
    # ---- mix-up rows, relative to the row maximum (bound and yardstick of tests/test_mlp3_gpu.py, the yardstick evaluated on the CPU)
    den = r64["Y"].abs().amax(dim=1, keepdim=True).clamp_min(1e-30)
    e32 = float(((r32["Y"].double() - r64["Y"]).abs() / den).max())
    err = float(((Y[:S, :45].double() - r64["Y"]).abs() / den).max())
    print("mixup_stage S=%d rows: e32 = %.3e  max |got - fp64| / row max = %.3e  (%.2f x e32; bound %.3e)" % (S, e32, err, err / max(e32, 1e-30), 2.5 * e32 + 3e-7))
    # ---- colours
    e32c = float((r32["rgb"].double() - r64["rgb"]).abs().max())
    errc = float((dec[listed, 1:].double() - r64["rgb"]).abs().max())
    print("mixup_stage S=%d colours: e32 = %.3e  max |got - fp64| = %.3e  (%.2f x e32; bound %.3e)" % (S, e32c, errc, errc / max(e32c, 1e-30), 4 * e32c + 1e-7))
    assert err <= 2.5 * e32 + 3e-7, (S, err, e32)
    assert errc <= 4 * e32c + 1e-7, (S, errc, e32c)
