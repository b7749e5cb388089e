"""Generates tests/golden/render_edit_parts.npz and render_edit_uni.npz: the reference's forward over the scene, camera, rays and weights of
render_scannet_small.npz with per-point rotations `neural_points.Rw2c` (models/neural_points/neural_points.py:720,
models/aggregators/point_aggregators.py:894-971), on the CPU.  Needs the reference checkout (tests/golden/_ref_import.py); data only is written.

  render_edit_parts.npz  a 3-D Rw2c [N,3,3] with two parts: identity for the points with x <= median(x), a rotation by 0.9 rad about
                         (0.3, -0.5, 0.8) / |.| for the others (positions are NOT moved: the rotation alone is under test)
  render_edit_uni.npz    the 2-D form: one [3,3] matrix for every point, 0.7 rad about z

The net is built by make_golden.gen_render with the arguments of the twin fixture (its own file goes to a temporary directory); the inputs are
asserted equal to the committed twin's arrays, so only the part index, the part matrices and the outputs that depend on the rotation are stored.
`weight` and `conf_coefficient` are formed before viewmlp from the un-rotated offsets: asserted equal to the twin's and not stored.

Run:  python tests/golden/make_golden_edit.py
"""
import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
from _ref_import import import_reference  # noqa: E402

KEEP = ("decoded_features", "coarse_raycolor", "coarse_point_opacity", "blend_weight")
FULL = ("coarse_raycolor", "coarse_point_opacity", "coarse_is_background", "coarse_mask")


def axis_angle(axis, angle):
    """Rodrigues' formula in fp64, rounded once to fp32."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], np.float64)
    return (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)).astype(np.float32)


def run(ref, net, inputs, Rw2c):
    grabbed = {}
    h = net.aggregator.register_forward_hook(lambda mod, args, res: grabbed.update(decoded=res[0]))
    net.neural_points.Rw2c = Rw2c
    with torch.no_grad():
        out = net(**inputs)
    h.remove()
    opt = net.opt
    shell = SimpleNamespace(input={}, opt=opt, tonemap_func=ref.drf.find_tone_map(opt.which_tonemap_func))
    full = ref.vol.NeuralPointsVolumetricModel.fill_invalid(shell, dict(out), inputs)
    res = {k: out[k].numpy() for k in KEEP if k != "decoded_features"}
    res["decoded_features"] = grabbed["decoded"].numpy()
    res["weight"], res["conf_coefficient"] = out["weight"].numpy(), out["conf_coefficient"].numpy()
    for k in FULL:
        res["full_" + k] = full[k].numpy()
    return res


def main():
    ref = import_reference()
    twin = dict(np.load(os.path.join(HERE, "render_scannet_small.npz"), allow_pickle=False))
    real_here = mg.HERE
    with tempfile.TemporaryDirectory() as tmp:
        mg.HERE = tmp                                  # gen_render's own file is the twin again: not kept
        try:
            net, inputs, out0 = mg.gen_render(ref, "scannet_small", "scene0241", 12000, 11, 64, 48, 600, opt_over=dict(agg_axis_weight=None),
                                              size=(1.0, 0.8, 0.6))
        finally:
            mg.HERE = real_here
        regen = dict(np.load(os.path.join(tmp, "render_scannet_small.npz"), allow_pickle=False))
    # same scene, camera, rays, weights and query as the committed twin
    for k in ("xyz", "emb", "conf", "pdir", "color", "pix", "raydir", "c2w", "c2w_nearest", "intrinsic", "images_nearest", "bg_color", "near_far",
              "q_sample_pidx", "q_sample_loc_w", "q_ray_mask"):
        np.testing.assert_array_equal(regen[k], twin[k], err_msg=k)
    for k in twin:
        if k.startswith("sd."):
            np.testing.assert_array_equal(regen[k], twin[k], err_msg=k)
    xyz = twin["xyz"]
    n = xyz.shape[0]

    # ---- two parts
    part = (xyz[:, 0] > np.median(xyz[:, 0])).astype(np.uint8)
    part_rot = np.stack([np.eye(3, dtype=np.float32), axis_angle([0.3, -0.5, 0.8], 0.9)])
    eye = run(ref, net, inputs, torch.eye(3).expand(n, 3, 3).contiguous())
    np.testing.assert_array_equal(eye["coarse_raycolor"], twin["coarse_raycolor"])            # an all-identity [N,3,3] changes nothing
    res = run(ref, net, inputs, torch.from_numpy(part_rot[part.astype(np.int64)]))
    # slot 0 decides a sample's view direction: count the samples where that shows
    pidx = twin["q_sample_pidx"]
    valid = pidx[..., 0] >= 0
    pp = np.where(pidx >= 0, part[np.clip(pidx, 0, None)], 255)
    mixed = valid & ((pp == 0).any(-1) & (pp == 1).any(-1))
    write("render_edit_parts.npz", twin, res, part, part_rot,
          "max|d colour| vs twin %.3f; %d of %d valid samples mix parts, on %d rays" % (
              float(np.abs(res["coarse_raycolor"] - twin["coarse_raycolor"]).max()), int(mixed.sum()), int(valid.sum()), int(mixed.any(-1).sum())))

    # ---- the 2-D form
    Rz = axis_angle([0.0, 0.0, 1.0], 0.7)
    res = run(ref, net, inputs, torch.from_numpy(Rz))
    write("render_edit_uni.npz", twin, res, np.zeros(n, np.uint8), Rz[None],
          "max|d colour| vs twin %.3f" % float(np.abs(res["coarse_raycolor"] - twin["coarse_raycolor"]).max()))


def write(name, twin, res, part, part_rot, note):
    np.testing.assert_array_equal(res["weight"], twin["weight"])
    np.testing.assert_array_equal(res["conf_coefficient"], twin["conf_coefficient"])
    save = dict(part=part, part_rot=part_rot)
    for k in KEEP:
        save[k] = res[k]
    for k in FULL:
        save["full_" + k] = res["full_" + k]
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **save)
    print("%s: %s, %.2f MB" % (name, note, os.path.getsize(path) / 1e6))


if __name__ == "__main__":
    main()
