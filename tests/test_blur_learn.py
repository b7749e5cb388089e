"""Learnable blur module inside the fused training step, host side: the CPU restatement against the reference's goldens, the new entry points in
the library and the ctypes table, the ctypes mirrors' layout, LearnableBlur's validation (no device involved), train_step's argument check."""
import ctypes
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import blur_learn_ref as R
from tests.golden_io import blur_learn_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hnr_blur_learn_workspace_bytes", "hnr_blur_learn_forward", "hnr_blur_learn_backward")


@pytest.mark.parametrize("tag", ["a", "c"])
def test_fp32_restatement_reproduces_the_reference_goldens(tag):
    """tests/blur_learn_ref.py in fp32 vs what the imported reference recorded (a: 7x7 patches of 8x8, ks 9, norm 0, mode 4, boundary 1 -- the shipped
    configuration; c: boundary 2), with the tolerances tests/test_blur_gpu.py uses for the same quantities."""
    cfg, color, gt, up, predictor, blocks, exp = blur_learn_case(tag)
    assert cfg["conv"] == 0
    weights = [p.detach() for p in predictor.parameters()]
    got = R.run(color[0], gt[0], up[0], weights, cfg, torch.float32, slope=float(predictor[1].negative_slope))
    np.testing.assert_allclose(got["out"], exp["out"][0], rtol=0, atol=2e-6)
    np.testing.assert_allclose(got["grad_color"], exp["grad_color"][0], rtol=0, atol=5e-6)
    for l in range(4):
        for k in ("weight", "bias"):
            g = exp["grads"]["0.%d.%s" % (2 * l, k)]
            np.testing.assert_allclose(got["learn_blur_kernel_block.%d.%s" % (2 * l, k)], g, rtol=0, atol=2e-5 * max(1.0, float(np.abs(g).max())))


def test_library_exports_the_new_entry_points_and_the_table_binds_them():
    from hybridneuralrendering_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert hasattr(L, s), "libhnr_hip.so does not export %s" % s
        assert s in _lib.SIGNATURES, s
    assert _lib.SIGNATURES["hnr_blur_learn_workspace_bytes"][0] is ctypes.c_int64


def test_new_ctypes_structs_have_the_layout_of_the_c_header(tmp_path):
    from hybridneuralrendering_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    pairs = [("hnr_blur_learn_params", _lib.BlurLearnParams), ("hnr_blur_learn_weights", _lib.BlurLearnWeights)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hnr.h"', 'int main(void) {']
    for cname, cls in pairs:
        lines.append('  printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
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
        assert got[(cname, "size")] == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert got[(cname, fname)] == getattr(cls, fname).offset, (cname, fname)


def test_c_abi_rejects_bad_arguments_without_touching_the_gpu():
    from hybridneuralrendering_amd import _lib
    L = _lib.lib()
    assert L.hnr_blur_learn_workspace_bytes(49, 8, 9, 4) >= 4 * 49 * (128 + 3 * 128 + 82 + 81 + 3 * 128 + 82)
    for bad in ((0, 8, 9, 4), (49, 17, 9, 4), (49, 8, 8, 4), (49, 8, 17, 4), (49, 8, 9, 2)):
        assert L.hnr_blur_learn_workspace_bytes(*bad) < 0
        assert b"hnr_blur_learn_workspace_bytes" in L.hnr_last_error()
    prm = _lib.BlurLearnParams(7, 8, 9, 4, 0, 1, 0.01)
    w = _lib.BlurLearnWeights()
    one = ctypes.c_void_p(16)
    assert L.hnr_blur_learn_forward(ctypes.byref(prm), ctypes.byref(w), one, one, one, 1 << 30, one, None, None) < 0      # NULL weights
    assert b"NULL weight" in L.hnr_last_error()
    for l in range(4):
        w.w[l], w.b[l] = 16, 16
    assert L.hnr_blur_learn_forward(ctypes.byref(prm), ctypes.byref(w), one, one, one, 64, one, None, None) < 0           # workspace too small
    assert b"workspace" in L.hnr_last_error()
    assert L.hnr_blur_learn_forward(ctypes.byref(prm), ctypes.byref(w), None, one, one, 1 << 30, one, None, None) < 0
    assert L.hnr_blur_learn_backward(ctypes.byref(prm), ctypes.byref(w), one, one, one, 1 << 30, one, None, None) < 0     # no gradient block
    for field, v in (("kernel_mode", 2), ("kernel_norm", 2), ("boundary_mode", 3), ("kernel_size", 4), ("patch_size", 17), ("patch_num", 0)):
        p2 = _lib.BlurLearnParams(7, 8, 9, 4, 0, 1, 0.01)
        setattr(p2, field, v)
        assert L.hnr_blur_learn_forward(ctypes.byref(p2), ctypes.byref(w), one, one, one, 1 << 30, one, None, None) < 0, field
        assert L.hnr_blur_learn_backward(ctypes.byref(p2), ctypes.byref(w), one, one, one, 1 << 30, one, ctypes.byref(w), None) < 0, field


def _opt(**kw):
    d = dict(learnable_blur_kernel_size=9, learnable_blur_kernel_conv=0, learnable_blur_kernel_norm=0, learnable_blur_kernel_mode=4, boundary_mode=1)
    d.update(kw)
    return SimpleNamespace(**d)


def test_learnable_blur_validates_on_the_host(monkeypatch):
    """Every unsupported option raises HnrError from the constructor; nothing there touches a device (CPU modules, and torch.empty is watched)."""
    from hybridneuralrendering_amd.blur import LearnableBlur
    from hybridneuralrendering_amd._lib import HnrError
    mlp = R.make_mlp(R.make_weights(8, 9, 4, 0), "cpu")
    real_empty = torch.empty

    def no_device(*a, **k):
        assert "cuda" not in str(k.get("device", "cpu")), "device allocation during validation"
        return real_empty(*a, **k)
    monkeypatch.setattr(torch, "empty", no_device)
    lb = LearnableBlur(mlp, _opt(), 7, 8)
    assert lb.n_patches == 49 and list(lb.parameters()) == R.NAMES and lb.kernels is None
    assert LearnableBlur(SimpleNamespace(learn_blur_kernel_block=mlp), _opt(), 5, 8, layout="patch_major").n_patches == 5
    with pytest.raises(HnrError, match="learnable_blur_update_output"):
        LearnableBlur(mlp, _opt(learnable_blur_kernel_conv=1), 7, 8)
    for kw in (dict(learnable_blur_kernel_mode=2), dict(learnable_blur_kernel_mode=1), dict(learnable_blur_kernel_norm=2), dict(boundary_mode=3),
               dict(learnable_blur_kernel_size=8), dict(learnable_blur_kernel_size=17), dict(learnable_blur_kernel_mode=0)):   # (mode 0 wants 81 outputs)
        with pytest.raises(HnrError):
            LearnableBlur(mlp, _opt(**kw), 7, 8)
    for pn, ps, layout in ((7, 17, "grid"), (7, 4, "grid"), (0, 8, "grid"), (7, 8, "rows")):
        with pytest.raises(HnrError):
            LearnableBlur(mlp, _opt(), pn, ps, layout=layout)
    act = lambda: nn.LeakyReLU(inplace=True)
    wrong = [nn.Sequential(nn.Linear(128, 128), act(), nn.Linear(128, 128), act(), nn.Linear(128, 82), nn.Sigmoid()),                       # three layers
             nn.Sequential(nn.Linear(128, 128), nn.ReLU(), nn.Linear(128, 128), act(), nn.Linear(128, 128), act(), nn.Linear(128, 82), nn.Sigmoid()),
             nn.Sequential(nn.Linear(128, 64), act(), nn.Linear(64, 128), act(), nn.Linear(128, 128), act(), nn.Linear(128, 82), nn.Sigmoid()),
             nn.Sequential(nn.Linear(128, 128), act(), nn.Linear(128, 128), act(), nn.Linear(128, 128), act(), nn.Linear(128, 82), nn.Tanh()),
             nn.Sequential(nn.Linear(128, 128), act(), nn.Linear(128, 128), nn.LeakyReLU(0.2), nn.Linear(128, 128), act(), nn.Linear(128, 82), nn.Sigmoid()),
             nn.Linear(128, 82), SimpleNamespace(learn_blur_kernel_block=None)]
    for m in wrong:
        with pytest.raises(HnrError):
            LearnableBlur(m, _opt(), 7, 8)
    # a valid object with CPU parameters refuses to run: no CPU fallback
    with pytest.raises(HnrError):
        lb.forward(torch.zeros(49 * 64, 3), torch.zeros(49 * 64, 3))


def test_train_step_refuses_both_blur_arguments():
    """The reference's shell takes exactly one of the two blur branches (mvs_points_volumetric_model.py:143-147): both arguments raise before anything
    is queued (no GPU needed); so does something that is not a LearnableBlur."""
    from hybridneuralrendering_amd.blur import LearnableBlur
    from hybridneuralrendering_amd.train import train_step, CapturedTrainStep
    from hybridneuralrendering_amd._lib import HnrError
    lb = LearnableBlur(R.make_mlp(R.make_weights(8, 9, 4, 0), "cpu"), _opt(), 7, 8)
    z = torch.zeros(3)
    args = (None, None) + (z,) * 16
    with pytest.raises(HnrError, match="one of them"):
        train_step(*args, blur_kernels=torch.zeros(1, 2, 5, 5), patch_num=7, patch_size=8, learnable_blur=lb)
    with pytest.raises(HnrError, match="LearnableBlur"):
        train_step(*args, learnable_blur=object())
    with pytest.raises(HnrError, match="one of them"):
        CapturedTrainStep(None, None, z, z, z, z, z, dict(blur_kernels=torch.zeros(1, 2, 5, 5)), 0.1, 1.0, learnable_blur=lb)
