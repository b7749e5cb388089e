"""Generates tests/golden/paths.npz by running the REFERENCE's own render-path code.  Needs the reference checkout (tests/golden/_ref_import.py);
the fixture holds data only.

Reference functions called (none is copied):
  data/nerf_synth360_ft_dataset.py  pose_spherical and NerfSynth360FtDataset.get_render_poses (:77-83, :235-239), the latter on a stand-in `self`
                                    that holds nothing but blender2opencv; when that module does not import, data/load_blender.py's pose_spherical
                                    and blender2opencv (the same expressions)

Recorded: `render_poses` [20,4,4] float64 as get_render_poses leaves them (stride 20, elevation -30, radius 4) and, for other arguments,
`poses_<n>_<elevation>_<radius>` = stack(pose_spherical(angle, elevation, radius) @ blender2opencv) over linspace(-180, 180, n + 1)[:-1], with the
argument triples in `cases` [k,3].

Run:  python tests/golden/make_golden_paths.py
"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

CASES = [(20, -30.0, 4.0), (7, 15.0, 2.5), (1, 0.0, 1.0)]


def main():
    from _ref_import import import_reference, REF
    try:
        import_reference()
    except Exception as e:                                       # the render path needs none of the hot-path modules
        print("hot-path modules did not import (%s); going on with the dataset module alone" % e)
        if REF not in sys.path:
            sys.path.insert(0, REF)
    out = {}
    try:
        ds = importlib.import_module("data.nerf_synth360_ft_dataset")
        pose_spherical = ds.pose_spherical
        me = types.SimpleNamespace(blender2opencv=np.array([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 0], [0, 0, 0, 1]]))
        ds.NerfSynth360FtDataset.get_render_poses(me)
        assert me.total == 20
        out["render_poses"] = np.asarray(me.render_poses, dtype=np.float64)
        b2cv = me.blender2opencv
        source = "data/nerf_synth360_ft_dataset.py"
    except Exception as e:
        print("data.nerf_synth360_ft_dataset did not import (%s); using data.load_blender" % e)
        lb = importlib.import_module("data.load_blender")
        pose_spherical, b2cv = lb.pose_spherical, lb.blender2opencv
        out["render_poses"] = np.stack([pose_spherical(a, -30.0, 4) @ b2cv for a in np.linspace(-180, 180, 20 + 1)[:-1]], 0).astype(np.float64)
        source = "data/load_blender.py"
    for n, el, rad in CASES:
        out["poses_%d_%g_%g" % (n, el, rad)] = np.stack([pose_spherical(a, el, rad) @ b2cv for a in np.linspace(-180, 180, n + 1)[:-1]], 0).astype(np.float64)
    out["cases"] = np.asarray(CASES, dtype=np.float64)
    out["source"] = np.asarray(source)
    path = os.path.join(HERE, "paths.npz")
    np.savez_compressed(path, **out)
    print("wrote %s from %s: %s" % (path, source, {k: v.shape for k, v in out.items()}))


if __name__ == "__main__":
    main()
