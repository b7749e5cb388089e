"""Expected-depth maps (compute_depth) without a GPU: the module accepts is_compute_depth, the three depth entry points are exported and bound,
and they refuse bad arguments before any HIP call (include/hnr.h error convention)."""
import ctypes

DEPTH_SYMBOLS = ("hnr_ray_depth", "hnr_composite_bwd_depth", "hnr_render_train_backward_depth")


def test_ray_marching_module_constructs_with_compute_depth():
    from hybridneuralrendering_amd import scenes
    from hybridneuralrendering_amd.modules import NeuralPointsRayMarching, find_blend_function, find_render_function, find_tone_map
    opt = scenes.default_opt()
    net = NeuralPointsRayMarching(tonemap_func=find_tone_map("off"), render_func=find_render_function("radiance"),
                                  blend_func=find_blend_function("alpha"), aggregator=None, is_compute_depth=True, neural_points=None, opt=opt)
    assert net.return_depth is True


def test_depth_entry_points_are_exported_and_bound():
    from hybridneuralrendering_amd import _lib
    L = _lib.lib()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in DEPTH_SYMBOLS:
        assert s in _lib.SIGNATURES, s
        assert hasattr(raw, s), s
        assert getattr(L, s).argtypes is not None, s


def test_depth_entry_points_reject_bad_arguments_without_touching_the_gpu():
    from hybridneuralrendering_amd import _lib
    L = _lib.lib()
    null = None
    one = ctypes.c_void_p(16)                                   # a non-NULL fake pointer; never dereferenced
    bad = -1                                                    # HNR_ERR_BADARG
    # hnr_ray_depth(blend_weight, loc_w, nsamp, ray_mask, campos, camrot, R, SR, depth, stream)
    assert L.hnr_ray_depth(one, one, null, one, one, one, -1, 24, one, null) == bad
    assert b"hnr_ray_depth" in L.hnr_last_error() and b"size" in L.hnr_last_error()
    assert L.hnr_ray_depth(one, one, null, one, one, one, 10, 0, one, null) == bad                 # SR = 0
    assert L.hnr_ray_depth(null, one, null, one, one, one, 10, 24, one, null) == bad               # NULL blend weight
    assert b"NULL" in L.hnr_last_error()
    assert L.hnr_ray_depth(one, one, null, one, one, one, 10, 24, null, null) == bad               # NULL output
    assert L.hnr_ray_depth(null, null, null, null, null, null, 0, 24, null, null) == 0            # R = 0: nothing to do
    # hnr_composite_bwd_depth: hnr_composite_bwd's arguments + d_g_depth after d_g_raycolor (may be NULL)
    assert L.hnr_composite_bwd_depth(one, one, one, one, null, one, one, one, -5, 24, 8, 0.008, 1, one, one, one, null) == bad
    assert b"hnr_composite_bwd_depth" in L.hnr_last_error()
    assert L.hnr_composite_bwd_depth(one, one, one, one, null, one, one, one, 5, 24, 8, 0.008, 1, null, one, one, null) == bad   # NULL colour grad
    assert b"NULL" in L.hnr_last_error()
    assert L.hnr_composite_bwd_depth(one, one, one, one, null, one, one, one, 5, 24, 8, 0.008, 1, one, one, null, null) == bad   # NULL output
    assert L.hnr_composite_bwd_depth(null, null, null, null, null, null, null, null, 0, 24, 8, 0.008, 1, null, null, null, null) == 0
    # hnr_render_train_backward_depth: NULL parameter block, negative sizes
    assert L.hnr_render_train_backward_depth(null, null, null, null, null, null, 0, null, null, null, null, null, null, null) == bad
    assert b"hnr_render_train_backward_depth" in L.hnr_last_error()
    prm = _lib.TrainParams()
    prm.R, prm.SR, prm.K, prm.D = -4, 24, 8, 400
    assert L.hnr_render_train_backward_depth(ctypes.byref(prm), None, None, None, None, one, 1 << 20, None, one, null, one, None, None,
                                             null) == bad
    prm.R, prm.cap_samples, prm.n_points, prm.slope = 16, 16 * 24, 100, 0.01
    assert L.hnr_render_train_backward_depth(ctypes.byref(prm), None, None, None, None, one, 1 << 20, None, null, null, one, None, None,
                                             null) == bad                                         # NULL blocks and colour gradient
    assert b"hnr_render_train_backward_depth" in L.hnr_last_error()
