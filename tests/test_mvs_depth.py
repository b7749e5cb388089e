"""CPU-side checks of the depth estimator (hybridneuralrendering_amd/mvs_depth.py, csrc/mvsnet.hip): the restatement (tests/mvs_depth_ref.py) run in fp32
reproduces the reference's own outputs recorded in tests/golden/mvs_depth.npz, the module carries the reference's parameter names and loads its
checkpoints, the packed images have the header's layout, unsupported options and shapes raise, and the C entries reject bad arguments before any launch.
Reads only the fixtures."""
import ctypes
import json
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import mvs_depth_ref as R
from tests.golden_io import GOLD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_gold():
    z = np.load(os.path.join(GOLD, "mvs_depth.npz"))
    d = {k: z[k] for k in z.files}
    d["sd"] = {k[3:]: torch.from_numpy(v) for k, v in d.items() if k.startswith("sd.")}
    d["cases"] = []
    for i, (V, D, H, W) in enumerate(d["shapes"]):
        c = {k[len("s%d." % i):]: v for k, v in d.items() if k.startswith("s%d." % i)}
        c.update(V=int(V), D=int(D), H=int(H), W=int(W), images=c["images_u8"].astype(np.float32) / np.float32(15))
        d["cases"].append(c)
    return d


@pytest.fixture(scope="module")
def gold():
    return load_gold()


def test_restatement_in_fp32_reproduces_the_reference(gold):
    """The restatement runs the same torch ops as the reference in the same order (the feature net one view at a time), so on the machine that wrote the
    fixture the two agree to the last bit: measured, 0 ulp of the tensor's largest value for the features, the probability volume, depth and confidence
    at all four shapes.  Another CPU or torch build may pick another convolution algorithm, that is another summation order: running the feature net on
    all views at once did that here and moved the features by up to 9 ulp and prob / depth / confidence by up to 7 / 4 / 6 ulp, and a second machine
    with another CPU gave 6.5 ulp for the features and 19 / 6 / 10.5 ulp for prob / depth / confidence.  The bounds leave a factor of about 4 over
    that: 32 ulp for the features, 64 ulp behind the 3-D network (its logits are scaled x30)."""
    assert [tuple(s) for s in gold["shapes"]] == [(3, 8, 32, 32), (3, 16, 64, 96), (2, 8, 32, 64), (5, 24, 96, 64)]
    for c in gold["cases"]:
        out = R.mvsnet(gold["sd"], c["images"], c["proj"], c["depth_values"], torch.float32)
        for name, ref, ulps in (("features", c["features"], 32), ("prob", c["prob"], 64), ("depth", c["depth"], 64), ("confidence", c["confidence"], 64)):
            got = out[name].numpy()
            assert got.dtype == np.float32 and got.shape == ref.shape, name
            e = R.abs_err(got, ref) / R.ulp_of_max(ref)
            print("%s %s: %.1f ulp of the largest value" % ((c["V"], c["D"], c["H"], c["W"]), name, e))
            assert e <= ulps, (name, e)
        # the recipe's promise: the softmax is not flat, the expected index moves over more than two bins
        assert float(out["fidx"].max() - out["fidx"].min()) > 2.0
    # the tail of gen_points against depth2point's recorded output
    for i in (0, 2):
        c = gold["cases"][i]
        cam, conf, mask, _ = R.depth_points(c["depth"], c["confidence"], c["H"], c["W"], c["pts_near_far"][0], c["pts_near_far"][1], c["pts_K"], torch.float32)
        assert R.abs_err(cam.numpy(), c["pts_cam_xyz"]) <= 4 * R.ulp_of_max(c["pts_cam_xyz"])
        np.testing.assert_array_equal(conf.numpy(), c["pts_confidence"])
        np.testing.assert_array_equal(mask.numpy(), c["pts_mask"])
        assert 0.05 < mask.float().mean() < 0.95


def test_module_carries_the_reference_parameter_names_and_shapes():
    from hybridneuralrendering_amd.mvs_depth import MVSNet
    want = json.load(open(os.path.join(GOLD, "mvs_depth_param_keys.json")))
    got = {k: list(v.shape) for k, v in MVSNet().state_dict().items()}
    assert got == want and len(want) == 89
    for k in ("feature.conv0.conv.weight", "feature.feature.bias", "cost_regularization.conv7.1.running_var", "cost_regularization.prob.bias"):
        assert k in got


def test_checkpoint_format_loads_and_a_missing_key_raises(gold, tmp_path):
    import hybridneuralrendering_amd as hnr
    from hybridneuralrendering_amd.mvs_depth import MVSNet
    from hybridneuralrendering_amd._lib import HnrError
    assert hnr.MVSNet is MVSNet and callable(hnr.depth_views)
    ckpt = {"model": {"module." + k: v for k, v in gold["sd"].items()}, "epoch": 14}
    ckpt["model"]["module.feature.conv0.bn.num_batches_tracked"] = torch.tensor(7)
    m = MVSNet().load_pretrained(ckpt)
    for k, v in m.state_dict().items():
        assert torch.equal(v, gold["sd"][k]), k
    path = str(tmp_path / "model_000014.ckpt")
    torch.save(ckpt, path)
    assert torch.equal(MVSNet().load_pretrained(path).cost_regularization.prob.bias, gold["sd"]["cost_regularization.prob.bias"])
    MVSNet().load_pretrained(dict(gold["sd"]))                                 # a bare state dict too
    for gone in ("feature.conv3.bn.running_var", "feature.feature.bias", "cost_regularization.conv9.0.weight", "cost_regularization.prob.weight"):
        with pytest.raises(HnrError, match=gone.replace(".", r"\.")):
            MVSNet().load_pretrained({"model": {k: v for k, v in ckpt["model"].items() if k != "module." + gone}})
    with pytest.raises(HnrError, match="unexpected"):
        MVSNet().load_pretrained(dict(gold["sd"], stray=torch.zeros(1)))
    with pytest.raises(HnrError):
        MVSNet(refine=True)


def test_pack_layout_matches_the_header(gold):
    from hybridneuralrendering_amd import _lib
    from hybridneuralrendering_amd.mvs_depth import MVSNet
    hdr = open(os.path.join(ROOT, "include", "hnr.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (HNR_MVSNET_\w+_PACKED_ELEMS) (\d+)", hdr)}
    assert defs == {"HNR_MVSNET_FEATURE_PACKED_ELEMS": _lib.MVSNET_FEATURE_PACKED_ELEMS, "HNR_MVSNET_REG_PACKED_ELEMS": _lib.MVSNET_REG_PACKED_ELEMS}
    sd = gold["sd"]
    feat, reg = MVSNet().load_pretrained(dict(sd)).pack_host()
    assert feat.dtype == reg.dtype == torch.float32 and feat.numel() == 40248 and reg.numel() == 298297
    fold = lambda p: sd[p + "weight"] * torch.rsqrt(sd[p + "running_var"] + 1e-5)                  # plain BatchNorm: no |weight|, eps on the variance only
    # feature net: w [cin][ky][kx][cout], mean, mul, bias per layer; `feature` closes it with w and bias
    assert torch.equal(feat[:216].view(3, 3, 3, 8), sd["feature.conv0.conv.weight"].permute(1, 2, 3, 0))
    assert torch.equal(feat[216:224], sd["feature.conv0.bn.running_mean"]) and torch.equal(feat[224:232], fold("feature.conv0.bn."))
    assert torch.equal(feat[232:240], sd["feature.conv0.bn.bias"])
    o2 = 240 + 8 * 9 * 8 + 24
    assert torch.equal(feat[o2:o2 + 3200].view(8, 5, 5, 16), sd["feature.conv2.conv.weight"].permute(1, 2, 3, 0))
    assert torch.equal(feat[-32:], sd["feature.feature.bias"]) and torch.equal(feat[-9248:-32].view(32, 3, 3, 32), sd["feature.feature.weight"].permute(1, 2, 3, 0))
    # 3-D network: w [cin][kz][ky][kx][cout]; the transposed layers' weights come as [cin][cout][...] from torch; `prob` closes it
    assert torch.equal(reg[:6912].view(32, 3, 3, 3, 8), sd["cost_regularization.conv0.conv.weight"].permute(1, 2, 3, 4, 0))
    assert torch.equal(reg[6912:6920], sd["cost_regularization.conv0.bn.running_mean"]) and torch.equal(reg[6920:6928], fold("cost_regularization.conv0.bn."))
    o7 = sum(ci * 27 * co + 3 * co for ci, co in ((32, 8), (8, 16), (16, 16), (16, 32), (32, 32), (32, 64), (64, 64)))
    assert torch.equal(reg[o7:o7 + 64 * 27 * 32].view(64, 3, 3, 3, 32), sd["cost_regularization.conv7.0.weight"].permute(0, 2, 3, 4, 1))
    assert torch.equal(reg[o7 + 64 * 27 * 32 + 32:o7 + 64 * 27 * 32 + 64], fold("cost_regularization.conv7.1."))
    assert torch.equal(reg[-1:], sd["cost_regularization.prob.bias"]) and torch.equal(reg[-217:-1].view(8, 3, 3, 3), sd["cost_regularization.prob.weight"][0])


def test_unsupported_shapes_options_and_cpu_tensors_raise(gold):
    from hybridneuralrendering_amd import mvs_depth as md
    from hybridneuralrendering_amd._lib import HnrError
    net = md.MVSNet()
    args = lambda V=3, D=8, H=32, W=32: (torch.zeros(1, V, 3, H, W), torch.zeros(1, V, 3, 4), torch.zeros(1, D))
    for bad in (dict(H=36), dict(W=36), dict(D=12), dict(H=16, D=4)):                              # h = 9, w = 9, D = 12: not multiples of 8
        with pytest.raises(HnrError, match="multiples of 8"):
            net(*args(**bad))
    with pytest.raises(HnrError, match="prob_only"):
        net(*args(), prob_only=True)
    with pytest.raises(HnrError, match="GPU"):                                                     # off the GPU there is nothing to fall back to
        net(*args())
    c = gold["cases"][0]
    cpu = torch.zeros
    for call in (lambda: md.feature_forward(cpu(1, 3, 32, 32), cpu(40248)), lambda: md.cost_volume(cpu(2, 32, 8, 8), cpu(2, 3, 4), cpu(8)),
                 lambda: md.cost_reg(cpu(32, 8, 8, 8), cpu(298297)), lambda: md.depth_head(cpu(8, 8, 8), cpu(8)),
                 lambda: md.depth_points(cpu(8, 8), cpu(8, 8), 32, 32, 2.0, 3.0, c["pts_K"])):
        with pytest.raises(HnrError):
            call()
    batch = dict(images=cpu(1, 3, 3, 32, 32), proj_mats=cpu(1, 3, 3, 3, 4), near_fars=cpu(1, 3, 2), near_fars_depth=cpu(1, 2), intrinsics=cpu(1, 3, 3, 3),
                 w2cs=cpu(1, 3, 4, 4))
    ok = dict(init_view_num=3, depth_vid=[0, 1, 2], manual_depth_view=1, manual_std_depth=0.0, depth_occ=0)
    for bad, word in ((dict(manual_std_depth=0.1), "manual_std_depth"), (dict(manual_depth_view=0), "manual_depth_view"),
                      (dict(manual_depth_view=5), "manual_depth_view"), (dict(depth_occ=1), "depth_occ")):
        with pytest.raises(HnrError, match=word):
            md.depth_views(batch, net, SimpleNamespace(**dict(ok, **bad)))
    with pytest.raises(HnrError, match="GPU"):
        md.depth_views(batch, net, SimpleNamespace(**ok))


def test_c_entries_reject_bad_arguments_without_touching_the_gpu():
    from hybridneuralrendering_amd import _lib
    L = _lib.lib()
    one, null, bad = ctypes.c_void_p(256), None, -1
    f9 = (ctypes.c_float * 9)(*([1.0] * 9))
    fs, rs = L.hnr_mvsnet_feature_scratch_elems, L.hnr_mvsnet_cost_reg_scratch_elems
    assert fs(0, 32, 32) < 0 and fs(65, 32, 32) < 0 and fs(1, 3, 32) < 0 and fs(1, 32, 32769) < 0
    assert fs(3, 32, 32) == 2 * 3 * 8 * 32 * 32 and fs(2, 37, 53) == 2 * 2 * max(8 * 37 * 53, 16 * 19 * 27, 32 * 10 * 14)
    assert rs(8, 9, 8) < 0 and rs(8, 8, 12) < 0 and rs(12, 8, 8) < 0 and rs(0, 8, 8) < 0 and rs(4096, 8192, 8) < 0          # not multiples of 8; too large
    N = 16 * 24 * 8
    assert rs(16, 24, 8) == 8 * N + 2 * N + 2 * N + N // 2 + N // 2 + N // 8 + N // 8
    fa = lambda **k: [k.get("img", one), k.get("V", 2), k.get("H", 32), k.get("W", 32), k.get("packed", one), k.get("feat", one), k.get("scratch", one),
                      k.get("ns", 1 << 30), null]
    for name in ("img", "packed", "feat", "scratch"):
        assert L.hnr_mvsnet_feature(*fa(**{name: null})) == bad, name
    assert b"NULL" in L.hnr_last_error()
    assert L.hnr_mvsnet_feature(*fa(H=3)) == bad and L.hnr_mvsnet_feature(*fa(V=0)) == bad
    assert L.hnr_mvsnet_feature(*fa(ns=100)) == bad and b"scratch" in L.hnr_last_error()
    va = lambda **k: [k.get("feat", one), k.get("V", 2), k.get("h", 8), k.get("w", 8), k.get("proj", one), k.get("dv", one), k.get("D", 8), k.get("vol", one), null]
    for name in ("feat", "proj", "dv", "vol"):
        assert L.hnr_mvsnet_cost_volume(*va(**{name: null})) == bad, name
    assert L.hnr_mvsnet_cost_volume(*va(V=0)) == bad and L.hnr_mvsnet_cost_volume(*va(V=65)) == bad and L.hnr_mvsnet_cost_volume(*va(D=0)) == bad
    assert L.hnr_mvsnet_cost_volume(*va(h=1)) == bad and L.hnr_mvsnet_cost_volume(*va(D=4096, h=8192, w=8192)) == bad
    ra = lambda **k: [k.get("vol", one), k.get("D", 8), k.get("h", 8), k.get("w", 8), k.get("packed", one), k.get("logits", one), k.get("scratch", one),
                      k.get("ns", 1 << 30), null]
    for name in ("vol", "packed", "logits", "scratch"):
        assert L.hnr_mvsnet_cost_reg(*ra(**{name: null})) == bad, name
    assert L.hnr_mvsnet_cost_reg(*ra(h=9)) == bad and b"multiples of 8" in L.hnr_last_error()
    assert L.hnr_mvsnet_cost_reg(*ra(D=12)) == bad and L.hnr_mvsnet_cost_reg(*ra(w=20)) == bad
    assert L.hnr_mvsnet_cost_reg(*ra(ns=100)) == bad and b"scratch" in L.hnr_last_error()
    ha = lambda **k: [k.get("logits", one), k.get("dv", one), k.get("D", 8), k.get("h", 8), k.get("w", 8), k.get("depth", one), k.get("conf", one), null, null]
    for name in ("logits", "dv", "depth", "conf"):
        assert L.hnr_mvsnet_depth_head(*ha(**{name: null})) == bad, name
    assert L.hnr_mvsnet_depth_head(*ha(D=0)) == bad and L.hnr_mvsnet_depth_head(*ha(w=1)) == bad
    pa = lambda **k: [k.get("depth", one), k.get("conf", one), k.get("h", 8), k.get("w", 8), k.get("H", 32), k.get("W", 32), 2.0, 3.0, k.get("M", f9),
                      k.get("cam", one), k.get("cout", one), k.get("mask", one), null]
    for name in ("depth", "conf", "M", "cam", "cout", "mask"):
        assert L.hnr_mvsnet_depth_points(*pa(**{name: null})) == bad, name
    assert L.hnr_mvsnet_depth_points(*pa(H=1)) == bad and L.hnr_mvsnet_depth_points(*pa(h=33)) == bad and L.hnr_mvsnet_depth_points(*pa(w=0)) == bad


def test_torch_ops_carry_schemas_and_trace_with_fake_tensors():
    from torch._subclasses import FakeTensorMode
    from hybridneuralrendering_amd import torch_ops, _lib
    ops = torch_ops.load()
    assert str(ops.mvsnet_feature.default._schema).endswith("-> Tensor")
    assert str(ops.mvsnet_depth_head.default._schema).endswith("-> (Tensor, Tensor, Tensor)")
    assert str(ops.mvsnet_depth_points.default._schema).endswith("-> (Tensor, Tensor, Tensor)")
    with FakeTensorMode():
        c = lambda *s: torch.empty(s, device="cuda", dtype=torch.float32)
        feat = ops.mvsnet_feature(c(3, 3, 64, 96), c(_lib.MVSNET_FEATURE_PACKED_ELEMS))
        assert tuple(feat.shape) == (3, 32, 16, 24)
        vol = ops.mvsnet_cost_volume(feat, c(3, 3, 4), c(16))
        assert tuple(vol.shape) == (32, 16, 16, 24)
        logits = ops.mvsnet_cost_reg(vol, c(_lib.MVSNET_REG_PACKED_ELEMS))
        assert tuple(logits.shape) == (16, 16, 24)
        assert [tuple(t.shape) for t in ops.mvsnet_depth_head(logits, c(16), True)] == [(16, 24), (16, 24), (16, 16, 24)]
        d, cf, p = ops.mvsnet_depth_head(logits, c(16), False)
        assert tuple(p.shape) == (0,)
        o = ops.mvsnet_depth_points(d, cf, 64, 96, 2.0, 3.0, [0.0] * 9)
        assert [tuple(t.shape) for t in o] == [(64, 96, 3), (64, 96), (64, 96)] and o[2].dtype == torch.uint8
