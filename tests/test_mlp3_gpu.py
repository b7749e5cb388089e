"""hnr_mlp3_forward (csrc/mlp.hip): three fused dense layers, fp32 in / out on the two-term fp16 split arithmetic, against an fp64
evaluation of the same nn.Linear + LeakyReLU stack beside the per-layer fp32-MFMA kernel (hnr_linear_f32); the colour-feature stack with its
128 -> 64 tail (both outputs, 1 .. 128 CUs + 3 rows, padded rows, a device-side count below the capacity) and the segmented row mapping
(seg_stride > 0) of the merge-weight stack against the same rows run as one block.

Recorded on an MI355X (profiles/fused_stage_tests.txt): tail output 2.5e-7 .. 8.8e-7 of the row maximum where the fp32-MFMA yardstick is
3.0e-7 .. 1.3e-6 (layer 2's output alike); segments 1.7e-7 .. 5.8e-7 against 2.5e-7 .. 7.5e-7, equal to the contiguous block bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = {
    # name: (K0, N0, N1, N2, acts, with_addend)  -- the three per-sample MLPs of viewmlp (point_aggregators.py:1028-1037, :1199, :1285-1292)
    "color_feature": (280, 128, 128, 128, (1, 1, 1), False),
    "merge_weight": (48, 64, 64, 64, (1, 1, 1), True),
    "mixup": (90, 45, 45, 45, (1, 1, 0), False),
}


def _case(name, M, seed, scale_rows=False):
    from hybridneuralrendering_amd.linear import FusedMlp3, PackedLinear
    K0, N0, N1, N2, acts, add = CASES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(seed)
    dims = [(N0, K0), (N1, N0), (N2, N1)]
    Ws = [(torch.rand(d, generator=g) * 2 - 1) * (3.0 / d[1]) ** 0.5 for d in dims]
    bs = [(torch.rand(d[0], generator=g) - 0.5) * 0.2 for d in dims]
    if add:
        bs[0] = None
    lda = (K0 + 3) // 4 * 4
    A = torch.randn((M, lda), generator=g)
    A[:, K0:] = 7.0                                     # padding columns must be ignored
    if scale_rows:
        A *= torch.exp2(torch.randint(-12, 13, (M, 1), generator=g).float())
    R = ridx = None
    if add:
        R = torch.randn((max(M // 4, 1), N0), generator=g) * 0.5
        ridx = torch.randint(0, R.shape[0], (M,), generator=g).to(torch.int32)
    Wd, bd = [w.to(dev) for w in Ws], [None if b is None else b.to(dev) for b in bs]
    Ad = A.to(dev)
    f = FusedMlp3(Wd, bd, acts)
    ldc = (N2 + 3) // 4 * 4
    out = torch.full((M, ldc), float("nan"), device=dev)
    counts = torch.tensor([0, 0, M + 5, 0], dtype=torch.int64, device=dev)        # device-side row count larger than the capacity: capacity wins
    f(Ad, out, M, counts, 2, 1, slope=0.01, R=None if R is None else R.to(dev), ridx=None if ridx is None else ridx.to(dev))
    torch.cuda.synchronize()
    # fp64 reference and the per-layer fp32-MFMA path
    lk = lambda x: torch.where(x > 0, x, x * 0.01)
    x64 = A[:, :K0].double()
    x32 = Ad
    for l in range(3):
        y = x64 @ Ws[l].double().T + (bs[l].double() if bs[l] is not None else 0.0)
        if l == 0 and add:
            y = y + R.double()[ridx.long()]
        x64 = lk(y) if acts[l] else y
        pl = PackedLinear(Wd[l], bd[l])
        o32 = torch.zeros((M, (Ws[l].shape[0] + 3) // 4 * 4), device=dev)          # row strides are multiples of 4 floats
        if l == 0 and add:
            x32 = pl.gather_add(x32, R.to(dev), ridx.to(dev), out=o32, act=bool(acts[l]), slope=0.01, K=K0)
        else:
            x32 = pl(x32, out=o32, act=bool(acts[l]), slope=0.01, K=Ws[l].shape[1])
    ref = x64
    den = ref.abs().amax(dim=1, keepdim=True).clamp_min(1e-30)
    e_fused = float(((out[:, :N2].cpu().double() - ref).abs() / den).max())
    e_f32 = float(((x32[:, :N2].cpu().double() - ref).abs() / den).max())
    return e_fused, e_f32, out


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("M", [1, 130, 70001])
def test_mlp3_is_fp32_class_against_fp64(name, M):
    e_fused, e_f32, out = _case(name, M, seed=M + len(name))
    assert bool(torch.isfinite(out[:, :CASES[name][3]]).all())
    assert e_fused <= 2.5 * e_f32 + 3e-7, (name, M, e_fused, e_f32)


def test_mlp3_rows_of_very_different_magnitude():
    e_fused, e_f32, _ = _case("color_feature", 4099, seed=3, scale_rows=True)
    assert e_fused <= 2.5 * e_f32 + 3e-7, (e_fused, e_f32)


def test_mlp3_device_side_row_count_and_bad_arguments():
    from hybridneuralrendering_amd.linear import FusedMlp3
    from hybridneuralrendering_amd._lib import HnrError
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    Ws = [torch.randn(d, generator=g).to(dev) * 0.1 for d in ((45, 90), (45, 45), (45, 45))]
    f = FusedMlp3(Ws, [None, None, None], (1, 1, 0))
    A = torch.randn((1000, 92), generator=g).to(dev)
    full = torch.zeros((1000, 48), device=dev)
    f(A, full, 1000)
    part = torch.full((1000, 48), -5.0, device=dev)
    counts = torch.tensor([0, 0, 0, 0, 0, 0, 333], dtype=torch.int64, device=dev)
    f(A, part, 1000, counts, 6, 1)                        # only the first 333 rows exist according to the device counter
    assert torch.equal(part[:333], full[:333]) and bool((part[333:] == -5.0).all())
    with pytest.raises(HnrError):
        FusedMlp3([torch.zeros((200, 90), device=dev), Ws[1], Ws[2]], [None] * 3, (1, 1, 0))       # N > 128
    with pytest.raises(HnrError):
        FusedMlp3([torch.zeros((64, 100), device=dev), torch.zeros((64, 64), device=dev), torch.zeros((64, 64), device=dev)], [None] * 3, (1, 1, 1))(
            torch.zeros((4, 100), device=dev), torch.zeros((4, 64), device=dev), 4)                 # no kernel for these k-step counts


# ================================================================================================ the tail layer and the segmented row mapping
def _lk(x):
    return torch.where(x > 0, x, x * 0.01)


def _stack(dims, seed, first_bias=True):
    g = torch.Generator().manual_seed(seed)
    Ws = [(torch.rand(d, generator=g) * 2 - 1) * (3.0 / d[1]) ** 0.5 for d in dims]
    bs = [(torch.rand(d[0], generator=g) - 0.5) * 0.2 for d in dims]
    if not first_bias:
        bs[0] = None
    return Ws, bs, g


def _yardsticks(A, Ws, bs, acts, add=None, tail=False):
    """fp64 evaluation of the stack and the per-layer fp32-MFMA path (hnr_linear_f32) on clean contiguous rows A [M, K0] (host).  `tail`: the
    fourth layer reads layer 2's output.  Returns ([fp64 outputs per layer], [fp32-MFMA outputs per layer])."""
    from hybridneuralrendering_amd.linear import PackedLinear
    dev = torch.device("cuda:0")
    K0 = Ws[0].shape[1]
    x64, x32 = A[:, :K0].double(), torch.zeros((A.shape[0], (K0 + 3) // 4 * 4))
    x32[:, :K0] = A[:, :K0]
    x32 = x32.to(dev)
    o64, o32 = [], []
    for l, (W, b, a) in enumerate(zip(Ws, bs, acts)):
        if tail and l == 3:
            x64, x32 = o64[2], o32[2]
        y = x64 @ W.double().T + (b.double() if b is not None else 0.0)
        if l == 0 and add is not None:
            y = y + add[0].double()[add[1].long()]
        x64 = _lk(y) if a else y
        pl = PackedLinear(W.to(dev), None if b is None else b.to(dev))
        o = torch.zeros((A.shape[0], (W.shape[0] + 3) // 4 * 4), device=dev)
        if l == 0 and add is not None:
            x32 = pl.gather_add(x32, add[0].to(dev), add[1].to(dev), out=o, act=bool(a), slope=0.01, K=K0)
        else:
            x32 = pl(x32, out=o, act=bool(a), slope=0.01, K=W.shape[1])
        o64.append(x64)
        o32.append(x32)
    return o64, o32


def _rel_err(got, ref):
    den = ref.abs().amax(dim=1, keepdim=True).clamp_min(1e-30)
    return float(((got.cpu().double()[:, :ref.shape[1]] - ref).abs() / den).max())


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


TAIL_M = ["1", "63", "64", "65", "130", "grid"]                                    # 64-row tiles, two workgroups per CU: "grid" = 128 CUs + 3 rows


def _tail_case(M, lda, seed, scale_rows=False):
    """color_feature_branch 280 -> 128 -> 128 -> 128 with its 128 -> 64 tail (aux_merge_weight_block.0's colour-feature columns): both outputs against
    fp64, a device-side count M below the capacity M + 5, NaN in the padding columns and in the rows beyond the count."""
    from hybridneuralrendering_amd.linear import FusedMlp3
    dev = torch.device("cuda:0")
    dims = [(128, 280), (128, 128), (128, 128), (64, 128)]
    acts = (1, 1, 1, 0)
    Ws, bs, g = _stack(dims, seed)
    cap = M + 5
    A = torch.full((cap, lda), float("nan"))
    A[:M, :280] = torch.randn((M, 280), generator=g)
    if scale_rows:
        A[:M] *= torch.exp2(torch.randint(-12, 13, (M, 1), generator=g).float())
    f = FusedMlp3([w.to(dev) for w in Ws], [b.to(dev) for b in bs], acts)
    out = torch.full((cap, 128), -7.25, device=dev)
    out2 = torch.full((cap, 64), -7.25, device=dev)
    counts = torch.tensor([0, 0, M, 0], dtype=torch.int64, device=dev)
    f(A.to(dev), out, cap, counts, 2, 1, slope=0.01, out2=out2)
    torch.cuda.synchronize()
    assert bool((out[M:] == -7.25).all()) and bool((out2[M:] == -7.25).all())       # rows beyond the device count: untouched in both outputs
    o64, o32 = _yardsticks(A[:M], Ws, bs, acts, tail=True)
    res = []
    for name, got, l in (("out", out[:M], 2), ("out2 (tail)", out2[:M], 3)):
        assert bool(torch.isfinite(got).all())
        e_fused, e_f32 = _rel_err(got, o64[l]), _rel_err(o32[l], o64[l])
        print("mlp3 color_feature_tail M=%d lda=%d%s %s: fp32-MFMA yardstick %.3e  max |got - fp64| / row max = %.3e  (bound %.3e)" % (
            M, lda, " scaled rows" if scale_rows else "", name, e_f32, e_fused, 2.5 * e_f32 + 3e-7))
        res.append((name, e_fused, e_f32))
    # the tail is not a copy of anything: its reference differs from layer 2's by far more than the bound
    assert float((o64[3] - o64[2][:, :64]).abs().max()) > 1e-2
    return res


@pytest.mark.parametrize("lda", [280, 284])
@pytest.mark.parametrize("M", TAIL_M)
def test_mlp3_color_feature_tail_both_outputs_against_fp64(M, lda):
    M = 128 * _cus() + 3 if M == "grid" else int(M)
    for name, e_fused, e_f32 in _tail_case(M, lda, seed=M + lda):
        assert e_fused <= 2.5 * e_f32 + 3e-7, (name, M, lda, e_fused, e_f32)


def test_mlp3_color_feature_tail_rows_of_very_different_magnitude():
    for name, e_fused, e_f32 in _tail_case(4099, 280, seed=5, scale_rows=True):
        assert e_fused <= 2.5 * e_f32 + 3e-7, (name, e_fused, e_f32)


@pytest.mark.parametrize("V", [1, 3, 4, 8])
@pytest.mark.parametrize("n", [1, 37, 1100])
def test_mlp3_segmented_rows_equal_the_contiguous_block(V, n):
    """seg_stride > 0 (the (view, sample) rows of hnr_proj_rows, every training forward): the merge-weight stack with its per-sample addend on V
    segments of n rows at stride cap = n + 13.  Row v cap + s equals logical row v n + s of one contiguous block bit for bit, the gaps keep the
    sentinel, and the result is within the fp64 bound."""
    from hybridneuralrendering_amd.linear import FusedMlp3
    dev = torch.device("cuda:0")
    dims = [(64, 48), (64, 64), (64, 64)]
    acts = (1, 1, 1)
    Ws, bs, g = _stack(dims, 100 * V + n, first_bias=False)
    cap = n + 13
    rows = (torch.arange(V)[:, None] * cap + torch.arange(n)[None, :]).reshape(-1)  # physical row of logical row v n + s
    Ac = torch.randn((V * n, 48), generator=g)
    R = torch.randn((n, 64), generator=g) * 0.5
    perm = torch.randperm(n, generator=g).to(torch.int32)                           # row -> sample: not the identity
    ridx_c = perm.repeat(V)
    A = torch.full((V * cap, 48), float("nan"))
    A[rows] = Ac
    ridx = torch.zeros((V * cap,), dtype=torch.int32)
    ridx[rows] = ridx_c
    f = FusedMlp3([w.to(dev) for w in Ws], [None if b is None else b.to(dev) for b in bs], acts)
    counts = torch.tensor([0, 0, 0, 0, 0, 0, n], dtype=torch.int64, device=dev)
    Rd = R.to(dev)
    out = torch.full((V * cap, 64), -7.25, device=dev)
    f(A.to(dev), out, V * cap, counts, 6, V, slope=0.01, R=Rd, ridx=ridx.to(dev), seg_stride=cap)
    out_c = torch.full((V * n, 64), -7.25, device=dev)
    f(Ac.to(dev), out_c, V * n, counts, 6, V, slope=0.01, R=Rd, ridx=ridx_c.to(dev), seg_stride=0)
    torch.cuda.synchronize()
    out, out_c = out.cpu(), out_c.cpu()
    assert torch.equal(out[rows], out_c)
    gaps = torch.ones(V * cap, dtype=torch.bool)
    gaps[rows] = False
    assert int(gaps.sum()) == 13 * V and bool((out[gaps] == -7.25).all())
    o64, o32 = _yardsticks(Ac, Ws, bs, acts, add=(R, ridx_c))
    e_fused, e_f32 = _rel_err(out_c, o64[2]), _rel_err(o32[2], o64[2])
    print("mlp3 segments V=%d n=%d: fp32-MFMA yardstick %.3e  max |got - fp64| / row max = %.3e  (bound %.3e)" % (V, n, e_f32, e_fused, 2.5 * e_f32 + 3e-7))
    assert e_fused <= 2.5 * e_f32 + 3e-7, (V, n, e_fused, e_f32)
    # the addend matters at this tolerance: another row -> sample map is another result
    assert n == 1 or float((o64[2] - _yardsticks(Ac, Ws, bs, acts, add=(R, torch.arange(n, dtype=torch.int32).repeat(V)))[0][2]).abs().max()) > 1e-2


def test_mlp3_segment_count_above_the_stride_is_clipped_to_it():
    """A device count of cap + 50 with seg_stride = cap: every segment holds cap rows, none runs into the next."""
    from hybridneuralrendering_amd.linear import FusedMlp3
    dev = torch.device("cuda:0")
    V, cap = 3, 50
    Ws, bs, g = _stack([(64, 48), (64, 64), (64, 64)], 9, first_bias=False)
    A = torch.randn((V * cap, 48), generator=g)
    R = torch.randn((cap, 64), generator=g) * 0.5
    ridx = torch.randperm(cap, generator=g).to(torch.int32).repeat(V)
    f = FusedMlp3([w.to(dev) for w in Ws], [None if b is None else b.to(dev) for b in bs], (1, 1, 1))
    over = torch.tensor([0, 0, 0, 0, 0, 0, cap + 50], dtype=torch.int64, device=dev)
    out = torch.full((V * cap + 8, 64), -7.25, device=dev)
    f(A.to(dev), out, V * cap, over, 6, V, slope=0.01, R=R.to(dev), ridx=ridx.to(dev), seg_stride=cap)
    want = torch.full((V * cap, 64), -7.25, device=dev)
    f(A.to(dev), want, V * cap, None, 0, 1, slope=0.01, R=R.to(dev), ridx=ridx.to(dev))
    torch.cuda.synchronize()
    assert torch.equal(out[:V * cap], want) and bool((out[V * cap:] == -7.25).all())
    assert not bool((want == -7.25).any())
