"""The fused per-neighbour chain at its tile, class and grid edges: hnr_chain_gather* + hnr_chain_forward (csrc/chain.hip: chain_gather_kernel, chain_kernel<4>;
csrc/chain_ws.hip: chain_ws_kernel, chain_sigma_kernel) through the C ABI on the synthetic cases of tests/chain_ref.py, against its float64 reference.
No scene, no query, no fixture.  tests/test_chain_ref.py checks the references and the case builder without a GPU.

Shapes (C = the device's CU count, which limits the grid):
  TILE_N      1, 15, 16, 17, 127, 128, 129 samples of 1..8 neighbours, cap = n: grids of 1, 2, 8 and 9 workgroups (the plain stride below 8, the XCD split from 8)
  GRID_N      16 C - 1, 16 C, 16 C + 1, 32 C + 17, 16 (C + 8) + 1: one tile per workgroup; one workgroup with a second tile; two or three each; one more per XCD
  CAP_CASES   1, 17 and 147 samples under capacities of 16 C .. 64 C (the capacity sizes the grid and the workspace, the count the tiles: most XCD ranges
              are empty or one tile), and no sample at all under a capacity of 64
  CLASS_CASES (big, small, tiny) samples listed with 1 and 2 classes: boundaries inside a tile, empty classes, a class of one sample, one workgroup facing 3
              tiles (cap 16), 8 facing 10 (cap 128), 112 C + 3 samples, a capacity that cuts the list inside the small class
  wide        embedding rows x 2^-6 .. 2^6, block1.2's outputs x 2^-6 .. 2^6, block3.2 x 3e-4 and alpha_branch x 1 / 3e-4, at 17 samples and at (17, 33, 65)

Every run follows one pattern: X5 [cap + 3, ld5] and sigma [cap + 3] start as a sentinel, ld5 is 280 or 288, the table's stride 256 or 264 with NaN in the
spare columns, the workspace is zero-filled and sized by hnr_chain_workspace_bytes(cap); list entries beyond the count name unlisted items whose positions
are NaN.  Then X5[:n, :256] per row relative to the row maximum <= 2.5 e32 + 3e-7, sigma <= 2.5 e32 + 1e-6 relative to the value (e32: the float32
restatement on the CPU; factor and floors are those of tests/test_chain_gpu.py), the view-direction columns inside 4 ulp, weight_out / conf_out inside
ref_gather_rows' bounds at the valid neighbour slots, and every other row, column and slot bit-unchanged; nothing NaN.

Recorded on an MI355X (C = 256; profiles/chain_edge_tests.txt): 59 cases in 14.1 s, the slowest 3.3 s (the 28 675-sample class case, which computes the
float64 and float32 references of its samples once for all its layouts); 979 bit-for-bit comparisons, none differing.
  X5       e32 <= 1.6e-6 of the row maximum, error <= 1.5e-6, at most 1.67 x e32 and 0.40 of the bound (one-class, class and HNR_CHAIN_RT = 4 cases alike)
  H1..H4   e32 <= 1.9e-6, error <= 1.7e-6, at most 1.11 x e32 and 0.40 of the bound
  sigma    e32 <= 1.7e-4 of the VALUE, error <= 8.6e-5, at most 2.5 x e32 and 0.75 of the bound: the figure is set by samples whose density is ~1e-13
           (logits near -30: the relative error of softplus there is the absolute error of the logit), so it says little about the other samples
  view direction 0.25, weight_out 0.39 of forward_glue_ref's per-element bounds

One case did miss its check, and a kernel changed for it: HNR_CHAIN_RT = 4 (chain_kernel<4>) gave X5 and sigma inside the float64 bound (X5 3.8e-7 at one
sample, e32 4.0e-7) but not the bits of the default kernel, at every size from one sample on: csrc/chain_ws.hip adds block1.2's k steps in the order
8..15, 0..7, chain_kernel<4> added them 0..15.  chain_kernel now runs that layer in the same order (h2_mfma_layer's KROT, csrc/hnr_h2.h); error against
float64 after the change 4.3e-7 at that sample, the default kernel's (1.3e-6 at most over the nine sizes, 1.12 x e32), bits equal at all nine sizes.
The training form chain_kernel<4, 3> (HNR_TRAIN_CHAIN_WS = 0) runs the same order now; tests/test_train_gpu.py holds it to the weight-stationary form as before.

Wrong kernels this module was seen to catch (scratch builds of the library, never committed; every edit changes values only and keeps every index in range):
  1. t_hi one tile short in the XCD split                        one-class n127 .. 16(C+8)+1 and all three capacity cases with a sample (rows left as the
                                                                 sentinel), their layer dumps, every class case with a grid of 8 or more, tile independence
  2. a 2-slot tile summed and stored as a 4-slot one             every classes = 2 case that lists a tiny sample but (0, 0, 1): the only sample there is the
                                                                 tile's first, whose pair sum and row are right either way (sigma is another kernel's)
  3. the next tile's point ids taken from the current tile       every case in which a workgroup runs a second tile: n129, 16C+1, 32C+17, 16(C+8)+1, their
                                                                 dumps, (5,6,5) at cap 16, (0,0,130), (113,8,7) at cap 128, the largest class case, tile independence
  4. block1.2's k steps 0..15 in row tile 2 only                 inside every float64 bound (it is fp32-class); caught by the bit comparisons: all 20 class
                                                                 cases against the one-class layout, tile independence, HNR_CHAIN_RT = 4
  5. an empty slot weighted like slot 0                          every case with an empty slot (all but n1, 1@16C, 0@64), against float64
  6. sin / cos swapped in one PE5 frequency of the gather        every case with a sample, layer 0's dump included
  7. chain_sigma_kernel summing a 2-slot sample over 4 lanes     the classes = 2 cases of 2. (sigma only)
  8. one workgroup more counted in XCD 0's stride (nb)           16C+1, 32C+17, 16(C+8)+1, (113,8,7) at cap 128, the largest class case, tile independence
Not caught, as sigma's floor says: softplus' threshold at y > 15 instead of 20 in chain_sigma_kernel (a relative change of at most e^-15 / 15 = 2e-8,
below the 1e-6 floor; all 59 cases pass).  A relative error of up to ~1e-4 in every sigma would pass too wherever e32 is that large.
"""
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from hybridneuralrendering_amd import _lib
from tests import chain_ref as R
from tests import forward_glue_ref as G

pytestmark = pytest.mark.gpu

F32 = np.float32
SENT = G.SENT
LAYOUTS = [(280, 256), (288, 264)]                  # (ld5, ldt)
_id = lambda spec: "-".join(str(int(x)) for x in spec)


@functools.lru_cache(maxsize=None)
def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _h(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _sent(*shape):
    return torch.full(shape, float(SENT), dtype=torch.float32, device="cuda:0")


def _call(name, *args):
    a = [_lib.ptr(x) if isinstance(x, torch.Tensor) else x for x in args]
    _lib.check(getattr(_lib.lib(), name)(*a, _lib.stream()), name)


def _note(test, what, e32=0.0, err=0.0, bound=0.0, bits=0):
    """One line per figure; the job that records profiles/chain_edge_tests.txt collects them."""
    print("[chain-edge] %s | %s | e32 %.3e err %.3e ratio %.2f share %.3f bits %d" % (test, what, e32, err, err / max(e32, 1e-30), err / bound if bound else 0.0, bits))


def _same(test, what, a, b):
    G.check_bits(what, np.ascontiguousarray(a), np.ascontiguousarray(b))
    _note(test, what, bits=1)


@functools.lru_cache(maxsize=None)
def _packed(wide):
    w = R.make_weights(wide)
    buf = torch.zeros((int(_lib.lib().hnr_chain_packed_bytes()),), dtype=torch.uint8, device="cuda:0")
    _call("hnr_chain_pack", _d(w["w10"][:, 224:284]), 60, *[_d(w[k]) for k in ("b10", "w12", "b12", "w30", "b30", "w32", "b32", "aw", "ab")], buf)
    torch.cuda.synchronize()
    return buf


def _launch(case, ld5=280, ldt=256, entry="gather", dbg_layer=None, forward=True, want_ws=False):
    """One gather (+ forward) on sentinel-filled outputs -> host arrays."""
    L = _lib.lib()
    cap, items, N = case["cap"], case["items"], case["n_points"]
    assert case["vs_item"].max() < items and case["pidx"].max() < N and case["n_valid"] <= cap and int(case["counts"][R.CNT_SMALL] + case["counts"][R.CNT_TINY]) <= cap
    ws = torch.zeros((int(L.hnr_chain_workspace_bytes(cap)),), dtype=torch.uint8, device="cuda:0")
    X5, sigma = _sent(cap + 3, ld5), _sent(cap + 3)
    wo, co = _sent(items, 8), _sent(items, 8)
    cloud = [_d(case[k]) for k in ("xyz", "conf", "dir", "color")]
    tail = [_d(case[k]) for k in ("pidx", "loc_w", "raydir", "campos", "camrot", "vs_item", "counts")] + [case["SR"], 8, cap, ws, X5, ld5, wo, co]
    if entry == "gather":
        _call("hnr_chain_gather", *cloud, *tail)
    elif entry == "parts0":
        _call("hnr_chain_gather_parts", *cloud, None, None, 0, *tail)
    else:
        rec = torch.full((N, 12), float("nan"), dtype=torch.float32, device="cuda:0")
        if entry == "rec":
            _call("hnr_point_records", *cloud, N, rec)
            _call("hnr_chain_gather_rec", rec, *tail)
        else:
            assert entry == "rec_parts1"
            _call("hnr_point_records_parts", *cloud, torch.zeros((N,), dtype=torch.int32, device="cuda:0"), N, rec)
            _call("hnr_chain_gather_rec_parts", rec, _d(np.eye(3, dtype=F32).reshape(1, 9)), 1, *tail)
    out = {}
    if forward:
        tab = np.full((N, ldt), np.nan, F32)
        tab[:, :256] = case["table"]
        dbg = None
        if dbg_layer is not None:
            dbg = torch.zeros((((cap + 15) // 16 + 2) * 128, 256), dtype=torch.float32, device="cuda:0")
        _call("hnr_chain_forward", ws, _d(tab), ldt, _packed(R.is_wide(case["spec"])), tail[6], cap, float(R.SLOPE), X5, ld5, sigma, dbg, dbg_layer or 0)
        if dbg is not None:
            out["dbg"] = _h(dbg)
    out.update(X5=_h(X5), sigma=_h(sigma), wo=_h(wo), co=_h(co))
    if want_ws:
        out["ws"] = _h(ws)
    return out


@functools.lru_cache(maxsize=None)
def _result(spec, ld5=280, ldt=256):
    return _launch(R.refs(spec)[0], ld5, ldt)


def _check(test, spec, out, ld5, case=None, ref=None, e32=None):
    """The pattern of the module docstring on one run."""
    if case is None:
        case, ref, e32 = R.refs(spec)
    n, cap = case["n_valid"], case["cap"]
    X5, sigma = out["X5"], out["sigma"]
    assert X5.shape == (cap + 3, ld5) and sigma.shape == (cap + 3,)
    assert not np.isnan(X5).any() and not np.isnan(sigma).any() and not np.isnan(out["wo"]).any() and not np.isnan(out["co"]).any()
    _same(test, "X5 rows beyond the count", X5[n:], np.full((cap + 3 - n, ld5), SENT, F32))
    _same(test, "X5 spare columns", X5[:n, 280:], np.full((n, ld5 - 280), SENT, F32))
    _same(test, "sigma beyond the count", sigma[n:], np.full((cap + 3 - n,), SENT, F32))
    for name, got in (("X5", X5[:n, :256]), ("sigma", sigma[:n])):
        err, b = R.rel(got, ref[name]), R.bound(e32, name)
        _note(test, "%s %s ld5=%d" % (_id(spec), name, ld5), e32[name], err, b)
        assert err <= b, "%s: %.3e of the row maximum, e32 %.3e, bound %.3e" % (name, err, e32[name], b)
    G.check("view direction", X5[:n, 256:280], *ref["viewdir"])
    it, k = case["row_item"], case["row_k"]
    G.check("weight_out", out["wo"][it, k], ref["weight_at"][it, k], ref["weight_bound_at"][it, k])
    _same(test, "conf_out", out["co"][it, k], ref["confc_at"][it, k].astype(F32))
    rest = np.ones(out["wo"].shape, bool)
    rest[it, k] = False
    _same(test, "weight_out elsewhere", out["wo"][rest], np.full((int(rest.sum()),), SENT, F32))
    _same(test, "conf_out elsewhere", out["co"][rest], np.full((int(rest.sum()),), SENT, F32))


# Cases by name (the CU count C is known on the device only): name -> spec
TILE_CASES = {"n%d" % n: (lambda C, n=n: R.one(n)) for n in R.TILE_N}
GRID_CASES = {name: (lambda C, i=i: R.one(R.grid_n(C)[i])) for i, name in enumerate(("16C-1", "16C", "16C+1", "32C+17", "16(C+8)+1"))}
CAP_CASES = {name: (lambda C, i=i: R.one(*R.cap_cases(C)[i])) for i, name in enumerate(("1@16C", "17@16C+5", "147@64C", "0@64"))}
WIDE_CASES = {"wide-n17": lambda C: R.WIDE_SPECS[0], "wide-17-33-65-classes1": lambda C: R.WIDE_SPECS[1], "wide-17-33-65-classes2": lambda C: R.WIDE_SPECS[2]}
CLASS_NAMES = ("5-6-5@16", "16-32-64", "17-33-65", "0-1-0", "0-0-1", "0-0-130", "113-8-7@128", "16C+1-32C+1-64C+1", "33-65-17@66")
CLASS_CASES = {"%s-classes%d" % (name, cl): (lambda C, i=i, cl=cl: R.class_cases(C)[i] + (cl,)) for i, name in enumerate(CLASS_NAMES) for cl in (1, 2)}
CASES = {**TILE_CASES, **GRID_CASES, **CAP_CASES, **WIDE_CASES, **CLASS_CASES}
assert len(R.class_cases(8)) == len(CLASS_NAMES) and len(R.grid_n(8)) == len(GRID_CASES) and len(R.cap_cases(8)) == len(CAP_CASES)


def _spec(name):
    return CASES[name](_cus())


def _names(*names):
    return pytest.mark.parametrize("name", [n for group in names for n in group])


# ================================================================================================ the tests
@_names(TILE_CASES, GRID_CASES, CAP_CASES, ["wide-n17"])
def test_one_class_edges_against_float64(name):
    spec = _spec(name)
    for ld5, ldt in LAYOUTS:
        _check("one_class", spec, _result(spec, ld5, ldt), ld5)
    _same("one_class", "the two layouts", _result(spec, 280, 256)["X5"][:, :280], _result(spec, 288, 264)["X5"][:, :280])
    _same("one_class", "the two layouts' sigma", _result(spec, 280, 256)["sigma"], _result(spec, 288, 264)["sigma"])
    if spec[3] and spec[0] == 0:                                      # nothing to do: the workspace stays as it was, too
        assert not _launch(R.refs(spec)[0], want_ws=True)["ws"].any()


@_names(TILE_CASES, list(GRID_CASES)[:3])
def test_layer_dumps_against_float64(name):
    """d_dbg of dbg_layer 0 .. 3 = H1 .. H4 (one-class layout: row 8 s + k of the padded layout holds neighbour k of sample s)."""
    spec = _spec(name)
    case, ref, e32 = R.refs(spec)
    prow = case["row_s"] * 8 + case["row_k"]
    for layer in range(4):
        out = _launch(case, dbg_layer=layer)
        name = R.LAYERS[layer]
        got = out["dbg"][prow]
        assert not np.isnan(got).any()
        err, b = R.rel(got, ref[name]), R.bound(e32, name)
        _note("layer_dumps", "%s %s" % (_id(spec), name), e32[name], err, b)
        assert err <= b, "%s: %.3e of the row maximum, e32 %.3e, bound %.3e" % (name, err, e32[name], b)
        # the dump form of the kernel produces the same sums
        _same("layer_dumps", "X5 of the dump run", out["X5"], _result(spec)["X5"])
        _same("layer_dumps", "sigma of the dump run", out["sigma"], _result(spec)["sigma"])


@_names(CLASS_CASES, list(WIDE_CASES)[1:])
def test_class_cases_against_float64_and_the_one_class_layout(name):
    spec = _spec(name)
    have = int(_lib.lib().hnr_chain_classes())
    assert have == 2, "the default kernel lists samples in up to two further classes"
    case, ref, e32 = R.refs(spec)
    n, pos = case["n_valid"], case["pos"]
    base = _result(R.one_class_of(spec))
    for ld5, ldt in LAYOUTS:
        out = _result(spec, ld5, ldt)
        _check("classes", spec, out, ld5)
        _same("classes", "X5 = the one-class layout's", out["X5"][:n, :280], base["X5"][pos][:, :280])
        _same("classes", "sigma = the one-class layout's", out["sigma"][:n], base["sigma"][pos])
        it, k = case["row_item"], case["row_k"]
        _same("classes", "weight_out = the one-class layout's", out["wo"][it, k], base["wo"][it, k])
    _check("classes", R.one_class_of(spec), base, 280)


ENTRIES = ("gather", "rec", "parts0", "rec_parts1")


@_names(TILE_CASES, ["17-33-65-classes2", "5-6-5@16-classes1"])
def test_four_gather_entry_points_are_bit_identical(name):
    """hnr_chain_gather, hnr_chain_gather_rec (48-byte point records), hnr_chain_gather_parts with no part and hnr_chain_gather_rec_parts with one identity
    part: the same workspace (compared whole), view-direction columns, weight_out and conf_out."""
    spec = _spec(name)
    case = R.refs(spec)[0]
    outs = [_launch(case, entry=e, forward=False, want_ws=True) for e in ENTRIES]
    assert outs[0]["ws"].any() and (outs[0]["wo"] != SENT).any()
    for e, o in zip(ENTRIES[1:], outs[1:]):
        for k in ("ws", "X5", "wo", "co"):
            _same("entry_points", "%s: %s" % (e, k), o[k], outs[0][k])
    _same("entry_points", "sigma untouched by the gather", outs[0]["sigma"], np.full(outs[0]["sigma"].shape, SENT, F32))


def test_tile_independence_at_one_tile_more_than_workgroups():
    """Dropping the first 5 of 16 C + 1 samples moves every other sample to another tile slot (and the list to one tile per workgroup): the same bits."""
    spec = R.one(16 * _cus() + 1)
    case = R.refs(spec)[0]
    full = _result(spec)
    counts = case["counts"].copy()
    counts[R.CNT_VALID] -= 5
    n = case["n_valid"] - 5
    part = _launch(dict(case, vs_item=np.ascontiguousarray(case["vs_item"][5:]), counts=counts, cap=n, n_valid=n))
    _same("tile_independence", "X5", part["X5"][:n], full["X5"][5:5 + n])
    _same("tile_independence", "sigma", part["sigma"][:n], full["sigma"][5:5 + n])
    _same("tile_independence", "beyond the count", part["X5"][n:], np.full((3, 280), SENT, F32))


def test_largest_case_is_deterministic():
    C = _cus()
    case = R.refs((16 * C + 1, 32 * C + 1, 64 * C + 1, 112 * C + 3, 2))[0]
    a, b = _launch(case, want_ws=True), _launch(case, want_ws=True)
    for k in ("X5", "sigma", "ws", "wo", "co"):
        _same("determinism", k, a[k], b[k])


# ================================================================================================ the compiler-scheduled kernel
def _rt_specs():
    return [R.one(n) for n in R.TILE_N + [16 * _cus() + 1]]


def _child_cases():
    """What the HNR_CHAIN_RT = 4 child runs and prints; the parent calls it too, with the default kernel."""
    recs = []
    for spec in _rt_specs():
        case, ref, e32 = R.refs(spec)
        out = _launch(case)
        _check("rt4", spec, out, 280, case, ref, e32)
        n = case["n_valid"]
        sha = hashlib.sha1(out["X5"][:n, :280].tobytes() + out["sigma"][:n].tobytes()).hexdigest()
        recs.append((spec[0], R.rel(out["X5"][:n, :256], ref["X5"]), R.rel(out["sigma"][:n], ref["sigma"]), sha))
    return recs


_CHILD = r'''
import sys
sys.path.insert(0, sys.argv[1])
from hybridneuralrendering_amd import _lib
from tests import test_chain_edges_gpu as T
assert int(_lib.lib().hnr_chain_classes()) == 0
for rec in T._child_cases():
    print("CHAIN_RT4 %d %.9e %.9e %s" % rec)
'''


def test_compiler_scheduled_kernel_in_a_child_process(tmp_path):
    """HNR_CHAIN_RT = 4 selects chain_kernel<4> (csrc/chain.hip); the knob is read once per process, so TILE_N and 16 C + 1 run in one fresh child, which
    holds every case to the pattern of this module; the parent repeats the float64 bound on the printed figures and compares the bits with the default kernel's."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "chain_rt4.py"
    script.write_text(_CHILD)
    p = subprocess.run([sys.executable, str(script), root], capture_output=True, text=True, timeout=300, env=dict(os.environ, HNR_CHAIN_RT="4"))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    recs = [l.split()[1:] for l in p.stdout.splitlines() if l.startswith("CHAIN_RT4 ")]
    specs = _rt_specs()
    assert [int(r[0]) for r in recs] == [s[0] for s in specs], p.stdout[-2000:]
    mine = _child_cases()
    for spec, (n, e5, es, sha), m in zip(specs, recs, mine):
        e32 = R.refs(spec)[2]
        for name, err in (("X5", float(e5)), ("sigma", float(es))):
            _note("rt4", "%s %s HNR_CHAIN_RT=4" % (_id(spec), name), e32[name], err, R.bound(e32, name))
            assert err <= R.bound(e32, name), (spec, name, err, e32[name])
        assert sha == m[3], "%s: HNR_CHAIN_RT=4 and the default kernel differ in X5 / sigma" % (spec,)
        _note("rt4", "%s bits equal to the default kernel" % _id(spec), bits=1)
