"""hybridneuralrendering_amd/_raycall.py without a GPU and without the library: the output table against the struct, the name tuples and the weight
table against literal copies of what the routes spelled by hand before, the shared parameter fields, the allocated shapes, the aligned workspace."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from hybridneuralrendering_amd import _lib, _raycall, torch_ops, train
from hybridneuralrendering_amd._raycall import RAY_OUTPUTS, RayOutputs

# literal copies, taken from the hand-written tables this module replaced
THIRTEEN = ("coarse_raycolor", "coarse_point_opacity", "coarse_is_background", "blend_weight", "ray_mask", "decoded", "sample_pidx", "sample_loc_w",
            "ray_nsamp", "counts", "status", "weight", "conf_coefficient")
TEN = ("coarse_raycolor", "coarse_point_opacity", "coarse_is_background", "ray_mask", "decoded", "sample_pidx", "sample_loc_w", "ray_nsamp",
       "counts", "status")
WEIGHT_NAMES = (
    ["block1.0.weight", "block1.0.bias", "block1.2.weight", "block1.2.bias", "block3.0.weight", "block3.0.bias", "block3.2.weight", "block3.2.bias",
     "alpha_branch.0.weight", "alpha_branch.0.bias"]
    + ["color_feature_branch.%d.weight" % l for l in (0, 2, 4)] + ["color_feature_branch.%d.bias" % l for l in (0, 2, 4)]
    + ["aux_merge_weight_block.%d.weight" % l for l in (0, 2, 4, 6)] + ["aux_merge_weight_block.%d.bias" % l for l in (0, 2, 4, 6)]
    + ["color_mixup_block.%d.weight" % l for l in (0, 2, 4)] + ["color_mixup_block.%d.bias" % l for l in (0, 2, 4)]
    + ["color_final_block.0.weight", "color_final_block.0.bias"]
    + ["aux_block_s%d.%d.weight" % (s, l) for s in (1, 2, 3) for l in (0, 2)] + ["aux_block_s%d.%d.bias" % (s, l) for s in (1, 2, 3) for l in (0, 2)])
WEIGHT_FIELDS = ["block1_0_w", "block1_0_b", "block1_2_w", "block1_2_b", "block3_0_w", "block3_0_b", "block3_2_w", "block3_2_b", "alpha_w", "alpha_b",
                 "cf_w", "cf_b", "mw_w", "mw_b", "mx_w", "mx_b", "fin_w", "fin_b", "conv_w", "conv_b"]
ARRAYS = dict(cf_w=3, cf_b=3, mw_w=4, mw_b=4, mx_w=3, mx_b=3, conv_w=6, conv_b=6)


def _slots_by_hand():
    slots = {}
    for nm, fld in (("block1.0", "block1_0"), ("block1.2", "block1_2"), ("block3.0", "block3_0"), ("block3.2", "block3_2"), ("alpha_branch.0", "alpha"),
                    ("color_final_block.0", "fin")):
        slots[nm + ".weight"] = (fld + "_w", None)
        slots[nm + ".bias"] = (fld + "_b", None)
    for i, l in enumerate((0, 2, 4)):
        slots["color_feature_branch.%d.weight" % l] = ("cf_w", i); slots["color_feature_branch.%d.bias" % l] = ("cf_b", i)
        slots["color_mixup_block.%d.weight" % l] = ("mx_w", i); slots["color_mixup_block.%d.bias" % l] = ("mx_b", i)
    for i, l in enumerate((0, 2, 4, 6)):
        slots["aux_merge_weight_block.%d.weight" % l] = ("mw_w", i); slots["aux_merge_weight_block.%d.bias" % l] = ("mw_b", i)
    for lvl in (1, 2, 3):
        for j, l in enumerate((0, 2)):
            slots["aux_block_s%d.%d.weight" % (lvl, l)] = ("conv_w", 2 * (lvl - 1) + j); slots["aux_block_s%d.%d.bias" % (lvl, l)] = ("conv_b", 2 * (lvl - 1) + j)
    return slots


def test_the_output_table_is_the_struct_in_order_and_the_name_tuples_come_from_it():
    fields = [f[0] for f in _lib.RenderOutputs._fields_]
    assert fields[-1] == "stage_events" and [o[1] for o in RAY_OUTPUTS] == fields[:-1]
    assert all(f[1] is _lib._P for f in _lib.RenderOutputs._fields_[:-1])
    assert torch_ops.TRAIN_OUTPUTS == THIRTEEN == _raycall.TRAIN_OUTPUTS and len(THIRTEEN) == 13
    assert torch_ops.FORWARD_OUTPUTS == TEN == _raycall.FORWARD_OUTPUTS
    assert isinstance(torch_ops.TRAIN_OUTPUTS, tuple) and isinstance(torch_ops.FORWARD_OUTPUTS, tuple)


def test_the_weight_table_walks_the_struct_in_order_and_gives_the_old_names_and_slots():
    assert [f for f, _ in _lib.TRAIN_WEIGHTS] == [f[0] for f in _lib.TrainWeights._fields_] == WEIGHT_FIELDS
    walked = []
    for (field, names), (_, ctype) in zip(_lib.TRAIN_WEIGHTS, _lib.TrainWeights._fields_):
        if field in ARRAYS:
            assert isinstance(names, list) and len(names) == ARRAYS[field] and ctype._length_ == ARRAYS[field] and ctype._type_ is _lib._P
            walked += names
        else:
            assert isinstance(names, str) and ctype is _lib._P
            walked.append(names)
    assert walked == WEIGHT_NAMES and len(walked) == 44 == len(set(walked))
    assert torch_ops.TRAIN_WEIGHT_NAMES == WEIGHT_NAMES and isinstance(torch_ops.TRAIN_WEIGHT_NAMES, list)
    assert train._SLOTS == _slots_by_hand() and len(train._SLOTS) == 44
    # the pointer block that the table fills: a name lands in its field and index, an absent one stays NULL
    w = train._fill_weights({})
    assert w.block1_0_w is None and w.conv_b[5] is None and ctypes.sizeof(w) == 44 * ctypes.sizeof(ctypes.c_void_p)


def _opt():
    return SimpleNamespace(SR=24, K=8, kernel_size=[3, 3, 3], vsize=[0.008, 0.008, 0.008], raydist_mode_unit=1)


@pytest.mark.parametrize("tmid, stride", [(torch.zeros(400), 0), (torch.zeros(65, 128), 128)])
def test_fill_params_fills_both_blocks_alike(tmid, stride):
    opt, r2 = _opt(), 0.016 ** 2 * 3.7
    a = _raycall.fill_params_opt(_lib.RenderParams(), opt, 65, 8, tmid, r2, 4, None, 1)
    b = _raycall.fill_params_opt(_lib.TrainParams(), opt, 65, 8, tmid, np.float32(r2), 4, 0, 1)
    shared = [f for f, _ in _lib.RenderParams._fields_]
    assert shared == ["R", "SR", "K", "D", "tmid_stride", "kernel_size", "radius2", "vsize_z", "raydist_mode_unit", "V", "cap_samples", "knn_order"]
    assert set(shared) < {f for f, _ in _lib.TrainParams._fields_}
    for f in shared:
        va, vb = getattr(a, f), getattr(b, f)
        assert (list(va), list(vb)) == ([3, 3, 3], [3, 3, 3]) if f == "kernel_size" else va == vb, f
    assert (a.R, a.SR, a.K, a.D, a.tmid_stride, a.V, a.cap_samples, a.knn_order, a.raydist_mode_unit) == (65, 24, 8, tmid.shape[-1], stride, 4, 65 * 24, 1, 1)
    assert a.radius2 == float(np.float32(r2)) != r2 and a.vsize_z == float(np.float32(0.008)) != 0.008
    assert (b.H, b.W, b.n_points, b.slope) == (0, 0, 0, 0.0)                          # the train route's own fields are left to it
    c = _raycall.fill_params(_lib.TrainParams(), 65, 24, 8, tmid, (3, 3, 1), 0.25, 0.5, 0, 0, 100, 0)
    assert (c.cap_samples, list(c.kernel_size), c.radius2, c.vsize_z, c.raydist_mode_unit, c.V) == (100, [3, 3, 1], 0.25, 0.5, 0, 0)
    assert _raycall.opt_scalars(SimpleNamespace(vsize=[1, 1, 0.5]), 2.0) == (2.0, 0.5, 0)         # raydist_mode_unit absent: off


@pytest.mark.parametrize("R, SR, K", [(1, 1, 8), (65, 24, 8)])
def test_alloc_gives_the_tables_shapes_and_dtypes(R, SR, K):
    expect = dict(coarse_raycolor=((R, 3), torch.float32), coarse_point_opacity=((R, SR), torch.float32), coarse_is_background=((R,), torch.float32),
                  blend_weight=((R, SR), torch.float32), ray_mask=((R,), torch.int8), decoded=((R, SR, 4), torch.float32),
                  sample_pidx=((R, SR, K), torch.int32), sample_loc_w=((R, SR, 3), torch.float32), ray_nsamp=((R,), torch.int32),
                  counts=((_lib.NCOUNTS,), torch.int64), status=((2,), torch.int32), weight=((R, SR, K), torch.float32),
                  conf_coefficient=((R, SR, K), torch.float32))
    o = RayOutputs.alloc(R, SR, K, "cpu")
    assert tuple(o.t) == THIRTEEN == tuple(o.as_dict())
    for k, t in o.as_dict().items():
        assert (tuple(t.shape), t.dtype, t.device.type) == (*expect[k], "cpu") and t.is_contiguous(), k
    assert o.as_dict() is not o.as_dict() and all(a is b for a, b in zip(o.as_dict().values(), o.t.values()))
    part = RayOutputs.alloc(R, SR, K, "cpu", blend=False, weights=False)
    for k in THIRTEEN:
        absent = k in ("blend_weight", "weight", "conf_coefficient")
        assert (part.t[k] is None) == absent and (part.as_dict()[k] is None) == absent, k
    assert [k for k, t in RayOutputs.alloc(R, SR, K, "cpu", weights=False).t.items() if t is None] == ["weight", "conf_coefficient"]
    assert [k for k, t in RayOutputs.alloc(R, SR, K, "cpu", blend=False).t.items() if t is None] == ["blend_weight"]
    # a shape function's allocator (a tensor's new_empty) gives the same list
    fake = RayOutputs.alloc(R, SR, K, None, empty=torch.zeros(1, dtype=torch.float64).new_empty)
    assert [(tuple(t.shape), t.dtype) for t in fake.t.values()] == [expect[k] for k in THIRTEEN]


@pytest.mark.parametrize("nbytes", [0, 1, 255, 256, 1000, 65537])
def test_workspace_pointer_is_aligned_and_its_bytes_fit(nbytes):
    ws, ptr = _raycall.workspace(nbytes, "cpu")
    assert ws.dtype == torch.uint8 and ws.dim() == 1
    assert ptr.value % 256 == 0 and ws.data_ptr() <= ptr.value and ptr.value + nbytes <= ws.data_ptr() + ws.numel()
    # a caller's tensor is taken when it is long enough (also at an odd address), a shorter one is not
    own = torch.empty(nbytes + 256 + 3, dtype=torch.uint8)[3:]
    ws2, ptr2 = _raycall.workspace(nbytes, "cpu", reuse=own)
    assert ws2 is own and ptr2.value % 256 == 0 and own.data_ptr() <= ptr2.value and ptr2.value + nbytes <= own.data_ptr() + own.numel()
    ws3, _ = _raycall.workspace(nbytes, "cpu", reuse=own[1:])
    assert ws3 is not own and ws3.numel() == nbytes + 256
