"""The small kernels between the heavy stages of the render forward (csrc/aggregate.hip; hnr_chain_plan of csrc/chain.hip), each alone through its C ABI
entry point (include/hnr.h) with the grid the entry point gives it, against float64 (tests/forward_glue_ref.py: references, per-element bounds derived
from the kernels' operation counts and operand magnitudes, and the float32 restatements that tests/test_forward_glue.py holds to the same bounds
without a GPU).  Inputs are synthetic: no scene, no fixture, no fused step.

Every test follows one pattern: input rows beyond a device-side count hold NaN (index rows: an in-range but wrong index), outputs carry spare rows /
columns of a sentinel that must come back bit-unchanged, every index is in range and every device count <= the capacity passed; decisions taken in
float32 (dist < 1e-8, > 2 vsize_z, the confidence clamps, y > 20, the argmax) see inputs exactly on a threshold or well clear of it.

 1. hnr_sample_plan      against a numpy loop; 0 .. 3000 listed items of a larger R * SR, K = 8 / 12, each capacity one short (overflow raised, nothing past it)
 2. hnr_chain_plan       classes 0 .. hnr_chain_classes() against numpy's stable partition; classes = 0 equals hnr_sample_plan's list
 3. hnr_gather_rows      both layouts, K = 8 / 9 / 12 / 16, neighbour counts 1 .. K, padded strides, weight_out absent / present, a rotated camera
 4. hnr_ksum             counts 1 .. 8 and 12, logits -30 .. 30 on both sides of y > 20, +-0 in H4, padded strides
 5. hnr_final_color      the vector loads of Y, the scalar loads (ldy = 45; a base 4 bytes off), a second trip of the sample loop, logits to +-30
 6. hnr_composite        R around the 256-ray block, SR 1 / 2 / 24, masked rays, nsamp absent / given (0, 1, SR; NaN beyond it), both distance modes
 7. hnr_ray_march        on the distances of 6, with / without a background; opacity and colour bit for bit those of hnr_composite (the two kernels'
                         per-sample arithmetic is operation for operation the same, and the build does not contract products into FMAs)
 8. hnr_probe_outputs    ties, all-zero rays, empty neighbour slots      9. hnr_gather_points    -1 entries

Worst err / bound per tensor on an MI355X (all shapes of a test together; 1 is the limit; 101 cases, 2522 bit-for-bit comparisons with 0 differences;
the whole module takes 3.6 s, its slowest case 0.32 s; profiles/forward_glue_tests.txt):
  3. PE3(emb) 0.250 (of sincosf's 4 ulp), PE5(dists6) 0.922, direction extras 1.000 (the differences' bound is the U |x| of a single rounding),
     wagg 0.284, weight_out 0.286        4. K-sums 0.586, view direction 0.247, sigma 0.005 (a 256-term dot under the softplus: its worst-case bound)
  5. rgb 0.886        6. colour 0.225, opacity 0.367, blend weight 0.253, T 0.247        7. colour 0.222, opacity 0.308, T 0.222, blend weight 0.228, T_end 0.210
  8. far distance 0.459, colour 0.170, dir 0.179, conf 0.164, embedding 0.279        9. xyz_pers 0.274
The float32 restatements reach the same figures on the CPU (tests/test_forward_glue.py) wherever no transcendental decides the worst element (PE5,
extras, wagg, weights, K-sums, sigma, composite colour, 8, 9: equal to three digits).  Where they depart the device's expf / sincosf round differently
from the host's libm inside the same 4 ulp: PE3 0.236, view direction 0.215, rgb 0.854 on the CPU (which does not run the two-trip capacity), opacity
0.371, blend weight 0.342, T 0.267; the CPU's ray-march figures (0.32 .. 0.49) are over all four distance variants, the device's over one.  No bound was widened.

Wrong kernels the module was seen to catch (scratch builds of the library, all of them changing values only and keeping every index in range):
  1. the block prefix of plan_scan_kernel without the block just before (1025 and 3000 items only); `<` for `<=` on cap_rows (the good call raises overflow)
  2. slot 1 for slot 2 in the choice between the 4- and 2-slot classes (classes = 2)
  3. sin and cos swapped in the 284-wide layout; the slots >= 8 of the other passes left out of the K > 8 weight sum (K = 9 / 12 / 16 only);
     the lower confidence clamp at 1e-3
  4. the weight of slot k + 1 for slot k inside the count (every case with a count above 1); sin and cos of the view direction swapped
  5. the second trip of the sample loop dropped (the large capacity only); column 44 of Y left out of the scalar loads (ldy = 45 and the offset base only)
  6. the running maximum of the depths dropped (SR = 24 only); unit mode's threshold at 6 vsize_z (SR = 2 and 24); is_background 0 on masked rays
  7. the validity flags ignored; the 1e-10 of the transmittance dropped (below the float64 bound of a rounded opacity: caught by the bit-for-bit comparison
     with hnr_composite alone)
  8. `>=` for `>` in the argmax (the ties)        9. x / z and y / z swapped in xyz_pers
Not caught, as the bound of sigma says: sigma lowered by 4e-5 on the samples with 12 neighbours (below the worst-case bound of the 256-term dot under the softplus).
"""
import numpy as np
import pytest
import torch

from hybridneuralrendering_amd import _lib
from tests import forward_glue_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
SENT, SENT_I = R.SENT, R.SENT_I


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _h(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _sent(*shape):
    return torch.full(shape, float(SENT), dtype=torch.float32, device="cuda:0")


def _sent_i(*shape):
    return torch.full(shape, SENT_I, dtype=torch.int32, device="cuda:0")


def _nan_rows(a, rows, ld):
    """a [n, c] in the first rows / columns of a NaN-filled [rows, ld] device buffer."""
    out = np.full((rows, ld), np.nan, F32)
    out[:a.shape[0], :a.shape[1]] = a
    return _d(out)


def _call(name, *args):
    a = [_lib.ptr(x) if isinstance(x, torch.Tensor) else x for x in args]
    _lib.check(getattr(_lib.lib(), name)(*a, _lib.stream()), name)


def _untouched(name, a, fill=SENT):
    a = np.asarray(a)
    R.check_bits(name + " (spare)", a, np.full(a.shape, fill, a.dtype))


# ================================================================================================ 1, 2
def _sample_plan(inp, n_alloc, cap_s, cap_r, flag0):
    n_blocks = (inp["max_items"] + 1023) // 1024
    out = [_sent_i(n_alloc) for _ in range(3)]
    scratch, flag = torch.zeros(2 * n_blocks + 2, dtype=torch.int32, device="cuda:0"), _d(np.array([flag0, SENT_I], np.int32))
    _call("hnr_sample_plan", _d(inp["work"]), _d(inp["pidx"]), _d(inp["counts"]), inp["K"], inp["max_items"], *out, cap_s, cap_r, scratch, flag)
    return [_h(t) for t in out], _h(flag)


@pytest.mark.parametrize("K", [8, 12])
@pytest.mark.parametrize("n_items", R.PLAN_ITEMS)
def test_sample_plan(n_items, K):
    inp = R.make_plan(n_items, K, seed=n_items + K)
    ref = R.loop_plan(inp)
    nv, nr = ref[0].size, inp["n_rows"]
    assert inp["counts"][R.CNT_SAMPLES] < inp["max_items"]
    runs = [(nv, nr, 1)] + ([(nv - 1, nr, 0), (nv, nr - 1, 0), (nv, nr, 1)] if nv else [])
    for cap_s, cap_r, flag0 in runs:
        got, flag = _sample_plan(inp, nv + 3, cap_s, cap_r, flag0)
        fits = R.plan_fits(ref[1], ref[2], cap_s, cap_r)
        assert flag[0] == (0 if fits.all() else 1) and flag[1] == SENT_I, (flag, cap_s, cap_r)
        for name, g, w in zip(("vs_item", "vs_off", "vs_cnt"), got, ref):
            R.check_bits(name, g[:nv][fits], w[fits])
            _untouched(name + " that do not fit", g[:nv][~fits], SENT_I)
            _untouched(name, g[nv:], SENT_I)


@pytest.mark.parametrize("n_items", R.PLAN_ITEMS)
def test_chain_plan(n_items):
    inp = R.make_plan(n_items, 8, seed=n_items + 8)
    nv = inp["n_valid"]
    n_blocks = (inp["max_items"] + 1023) // 1024
    work, pidx = _d(inp["work"]), _d(inp["pidx"])
    have = int(_lib.lib().hnr_chain_classes())
    assert 0 <= have <= 2
    for classes in range(have + 1):                                   # (the classes above hnr_chain_classes() are refused: tests/test_chain_gpu.py)
        want, n_small, n_tiny = R.ref_chain_plan(inp, classes)
        c0 = inp["counts"].copy()
        c0[R.CNT_SMALL], c0[R.CNT_TINY] = 77, 77
        counts, vs = _d(c0), _sent_i(nv + 3)
        scratch = torch.zeros(3 * n_blocks + 3, dtype=torch.int32, device="cuda:0")
        _call("hnr_chain_plan", work, pidx, counts, 8, inp["max_items"], classes, vs, nv, scratch)
        vs, counts = _h(vs), _h(counts)
        R.check_bits("vs_item (classes %d)" % classes, vs[:nv], want)
        _untouched("vs_item", vs[nv:], SENT_I)
        c0[R.CNT_SMALL], c0[R.CNT_TINY] = n_small, n_tiny
        R.check_bits("counts", counts, c0)
        if classes == 0:
            got, _ = _sample_plan(inp, nv + 3, nv, inp["n_rows"], 0)
            R.check_bits("hnr_sample_plan's vs_item", vs, got[0])


# ================================================================================================ 3
GATHER_LAYOUTS = [(False, 284, 264, False), (False, 288, 268, True), (True, 60, 264, True), (True, 64, 268, False)]     # (SPLIT, ld1, ld3, weight_out)


@pytest.mark.parametrize("K", R.GATHER_K)
@pytest.mark.parametrize("n_valid", R.GATHER_N)
def test_gather_rows(n_valid, K):
    inp = R.make_gather_rows(n_valid, K, seed=n_valid + K)
    ref = R.ref_gather_rows(inp)
    rows, items, pid = inp["rows"], inp["items"], inp["row_pid"]
    assert inp["vs_item"].max() < items and inp["pidx"].max() < inp["n_points"] and (inp["vs_off"] + inp["vs_cnt"])[:n_valid].max() == rows
    head = [_d(inp[k]) for k in ("xyz", "emb", "conf", "dir", "color")] + [32] + \
           [_d(inp[k]) for k in ("pidx", "loc_w", "raydir", "campos", "camrot", "vs_item", "vs_off", "vs_cnt", "counts")] + [inp["SR"], K, inp["cap"]]
    listed = np.zeros((items, K), bool)
    listed[inp["row_item"], inp["row_k"]] = True
    for split, ld1, ld3, with_w in GATHER_LAYOUTS:
        X1, X3, wagg = _sent(rows + 2, ld1), _sent(rows + 2, ld3), _sent(rows + 2)
        wo, co = (_sent(items, K), _sent(items, K)) if with_w else (None, None)
        rp = _sent_i(rows + 2) if split else None
        _call("hnr_gather_rows", *head, X1, ld1, X3, ld3, wagg, wo, co, rp)
        X1, X3, wagg = _h(X1), _h(X3), _h(wagg)
        n1 = 60 if split else 284
        _untouched("X1 rows", X1[rows:])
        _untouched("X1 padding columns", X1[:rows, n1:])
        if split:
            rp = _h(rp)
            R.check_bits("row_pid", rp[:rows], pid)
            _untouched("row_pid", rp[rows:], SENT_I)
            R.check("PE5(dists6)", X1[:rows, :60], *ref["pe5"])
        else:
            R.check_bits("embedding copy", X1[:rows, :32], inp["emb"][pid])
            R.check("PE3(emb)", X1[:rows, 32:224], *ref["pe3"])
            R.check("PE5(dists6)", X1[:rows, 224:284], *ref["pe5"])
        _untouched("X3[:, :256]", X3[:, :256])
        _untouched("X3 rows", X3[rows:])
        _untouched("X3 padding columns", X3[:rows, 263:])
        R.check_bits("colour", X3[:rows, 256:259], inp["color"][pid])
        R.check("direction extras", X3[:rows, 259:263], *ref["ext"])
        R.check("wagg", wagg[:rows], *ref["wagg"])
        _untouched("wagg", wagg[rows:])
        if with_w:
            wo, co = _h(wo), _h(co)
            R.check("weight_out", wo[inp["row_item"], inp["row_k"]], *ref["weight"])
            R.check_bits("conf_out", co[inp["row_item"], inp["row_k"]], ref["confc"])
            _untouched("weight_out past the neighbour counts", wo[~listed])
            _untouched("conf_out past the neighbour counts", co[~listed])


# ================================================================================================ 4
@pytest.mark.parametrize("twelve", [False, True])
@pytest.mark.parametrize("n_valid", R.KSUM_N)
def test_ksum(n_valid, twelve):
    inp = R.make_ksum(n_valid, twelve, seed=n_valid + twelve)
    ref = R.ref_ksum(inp)
    n, cap, rows = n_valid, inp["cap"], inp["rows"]
    assert (inp["vs_off"] + inp["vs_cnt"])[:n].max() == rows and inp["vs_item"].max() < inp["R"] * inp["SR"]
    wagg = _d(np.concatenate([inp["wagg"], np.full(8, np.nan, F32)]))
    tail = [_d(inp[k]) for k in ("alpha_w", "alpha_b", "vs_item", "vs_off", "vs_cnt", "raydir", "counts")] + [inp["SR"], cap]
    for ldh, ld5 in ((256, 280), (260, 284)):
        X5, sigma = _sent(cap + 1, ld5), _sent(cap + 1)
        _call("hnr_ksum", _nan_rows(inp["H"], rows + 8, ldh), ldh, wagg, *tail, X5, ld5, sigma)
        X5, sigma = _h(X5), _h(sigma)
        _untouched("X5 rows", X5[n:])
        _untouched("X5 columns from 280", X5[:n, 280:])
        _untouched("sigma", sigma[n:])
        R.check("K-sums", X5[:n, :256], *ref["feat"])
        R.check("view direction", X5[:n, 256:280], *ref["viewdir"])
        R.check("sigma", sigma[:n], *ref["sigma"])


# ================================================================================================ 5
@pytest.mark.parametrize("ldy,y_off,ldcf", R.FINAL_LAYOUTS)
@pytest.mark.parametrize("cap,n_valid", R.FINAL_SHAPES)
def test_final_colour(cap, n_valid, ldy, y_off, ldcf):
    inp = R.make_final(cap, n_valid, ldy, ldcf, seed=cap)
    rgb, bound, _ = R.ref_final(inp)
    n, items = n_valid, inp["items"]
    assert cap <= 16 * R.FINAL_BLOCKS or n_valid > 16 * R.FINAL_BLOCKS                # the large capacity takes the second trip
    ybuf = torch.full((cap * ldy + 4,), float("nan"), dtype=torch.float32, device="cuda:0")
    Y = ybuf[y_off:y_off + cap * ldy]
    Y.copy_(_d(inp["Y"]).reshape(-1))
    assert Y.data_ptr() % 16 == 4 * y_off
    dec = _sent(items + 1, 4)
    _call("hnr_final_color", Y, ldy, _d(inp["CF"]), ldcf, _d(inp["w_fin"]), _d(inp["b_fin"]), _d(inp["sigma"]), _d(inp["vs_item"]), _d(inp["counts"]), cap, dec)
    dec = _h(dec)
    it = inp["vs_item"][:n]
    rest = np.setdiff1d(np.arange(items + 1), it)
    _untouched("decoded entries not listed", dec[rest])
    R.check_bits("decoded[:, 0] = sigma", dec[it, 0], inp["sigma"][:n])
    R.check("rgb", dec[it, 1:4], rgb, bound)


# ================================================================================================ 6, 7
def _composite(inp, loc, pidx, dec, nsamp, unit_mode, blend, ray_mask=None):
    R_, SR = inp["R"], inp["SR"]
    col, opa, isbg = _sent(R_ + 2, 3), _sent(R_ + 2, SR), _sent(R_ + 2)
    bw = _sent(R_ + 2, SR) if blend else None
    _call("hnr_composite", _d(dec), _d(loc), _d(pidx), _d(inp["ray_mask"] if ray_mask is None else ray_mask), _d(nsamp) if nsamp is not None else None,
          _d(inp["campos"]), _d(inp["camrot"]), _d(inp["bg"]), R_, SR, inp["K"], float(inp["vsize_z"]), unit_mode, col, opa, isbg, bw)
    out = dict(color=_h(col), opacity=_h(opa), T_end=_h(isbg))
    if blend:
        out["blend"] = _h(bw)
    for k, v in out.items():
        _untouched(k + " rows", v[R_:])
    return out


@pytest.mark.parametrize("SR", R.COMPOSITE_SR)
@pytest.mark.parametrize("R_", R.COMPOSITE_R)
def test_composite(R_, SR):
    inp = R.make_composite(R_, SR, 8, seed=R_ + SR)
    for use_nsamp in (False, True):
        for unit_mode in (0, 1):
            ref = R.ref_composite(inp, use_nsamp, unit_mode)
            for blend in (False, True):
                if use_nsamp:
                    got = _composite(inp, *R.poisoned(inp), inp["nsamp"], unit_mode, blend)
                    pad = _composite(inp, *R.padded(inp, True), None, unit_mode, blend)
                    for k in got:
                        R.check_bits(k + ": nsamp form = padded form", got[k], pad[k])
                else:
                    got = _composite(inp, inp["loc_w"], inp["pidx"], inp["decoded"], None, unit_mode, blend)
                for k in got:
                    R.check(k, got[k][:R_], *ref[k])                  # (rays with ray_mask = 0: bound 0, the exact background / 0 / 1)


@pytest.mark.parametrize("SR", R.COMPOSITE_SR)
@pytest.mark.parametrize("R_", R.COMPOSITE_R)
def test_ray_march(R_, SR):
    inp = R.make_composite(R_, SR, 8, seed=R_ + SR)
    d_f, _, _, valid = R.ray_dist(inp, False, 1)
    dec = inp["decoded"]
    dist, val, feat = _d(d_f), _d(valid.astype(np.uint8)), _d(dec)
    for bg in (None, inp["bg"]):
        ref = R.ref_march(R.f64(d_f), 0.0, valid, dec, bg)
        col, opa, acc, bw, bgt = _sent(R_ + 2, 3), _sent(R_ + 2, SR), _sent(R_ + 2, SR), _sent(R_ + 2, SR), _sent(R_ + 2)
        _call("hnr_ray_march", dist, val, feat, _d(bg) if bg is not None else None, R_, SR, col, opa, acc, bw, bgt)
        got = dict(color=_h(col), opacity=_h(opa), T=_h(acc), blend=_h(bw), T_end=_h(bgt))
        for k, v in got.items():
            _untouched(k + " rows", v[R_:])
            R.check("march " + k, v[:R_], *ref[k])
    comp = _composite(inp, inp["loc_w"], inp["pidx"], dec, None, 1, True, ray_mask=np.ones(R_, np.int8))
    for k in ("opacity", "color", "blend", "T_end"):
        R.check_bits("hnr_composite's " + k, comp[k], got[k])


# ================================================================================================ 8
@pytest.mark.parametrize("R_", R.PROBE_R)
def test_probe_outputs(R_):
    inp = R.make_probe(R_, seed=R_)
    ref = R.ref_probe(inp)
    F = inp["F"]
    assert inp["pidx"].max() < inp["n_points"]
    o_op, o_loc, o_far, o_col, o_dir, o_conf, o_emb = _sent(R_ + 2), _sent(R_ + 2, 3), _sent(R_ + 2), _sent(R_ + 2, 3), _sent(R_ + 2, 3), _sent(R_ + 2), _sent(R_ + 2, F)
    _call("hnr_probe_outputs", *[_d(inp[k]) for k in ("opacity", "loc_w", "pidx", "weight", "conf_c", "xyz", "emb", "conf", "dir", "color")], F, R_, inp["SR"],
          inp["K"], o_op, o_loc, o_far, o_col, o_dir, o_conf, o_emb)
    got = dict(max_opacity=_h(o_op), max_loc=_h(o_loc), far=_h(o_far), color=_h(o_col), dir=_h(o_dir), conf=_h(o_conf), emb=_h(o_emb))
    for k, v in got.items():
        _untouched(k + " rows", v[R_:])
    R.check_bits("max_opacity", got["max_opacity"][:R_], ref["max_opacity"])
    R.check_bits("max_loc_w", got["max_loc"][:R_], ref["max_loc"])
    for k in ("far", "color", "dir", "conf", "emb"):
        R.check("probe " + k, got[k][:R_].reshape(ref[k][0].shape), *ref[k])


# ================================================================================================ 9
@pytest.mark.parametrize("n", R.POINTS_N)
def test_gather_points(n):
    inp = R.make_points(n, seed=n)
    ref = R.ref_points(inp)
    pid = ref["pid"]
    o_col, o_dir, o_conf, o_emb, o_pers, o_xyz = _sent(n + 2, 3), _sent(n + 2, 3), _sent(n + 2), _sent(n + 2, 32), _sent(n + 2, 3), _sent(n + 2, 3)
    o_mask = torch.full((n + 2,), 0x5A, dtype=torch.uint8, device="cuda:0")
    _call("hnr_gather_points", _d(inp["pidx"]), n, *[_d(inp[k]) for k in ("xyz", "emb", "conf", "dir", "color")], 32, _d(inp["campos"]), _d(inp["camrot"]),
          o_col, o_dir, o_conf, o_emb, o_pers, o_xyz, o_mask)
    for name, t, src in (("color", o_col, "color"), ("dir", o_dir, "dir"), ("conf", o_conf, "conf"), ("emb", o_emb, "emb"), ("xyz", o_xyz, "xyz")):
        v = _h(t)
        _untouched(name + " rows", v[n:])
        R.check_bits("gathered " + name, v[:n], inp[src][pid])
    m = _h(o_mask)
    R.check_bits("mask", m, np.concatenate([ref["mask"], np.full(2, 0x5A, np.uint8)]))
    pers = _h(o_pers)
    _untouched("xyz_pers rows", pers[n:])
    R.check("xyz_pers", pers[:n], *ref["pers"])
