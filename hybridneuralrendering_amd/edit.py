"""Scene editing: cut parts out of trained point clouds, move them rigidly and merge them into one cloud that renders with per-point
rotations (the reference's run/editiing.py:123-137, :189-212).

    parts = [edit.load_part("a/latest_net_ray_marching.pth"),                                         # everything, where it is
             edit.load_part("b/latest_net_ray_marching.pth", "b/parts_index/chair.txt", "b/transforms/move.txt")]
    composed = edit.compose(parts)
    edit.apply(model.neural_points, composed)        # = neural_points.editing_set_points(..., Rw2c=(part, part_rot))

A part moves with xyz' = Rot xyz + Tran; its points' local frame moves with it through Rw2c' = Rot (a source without rotations) or
Rw2c_src Rot^T (:201).  The rotations are kept as a PART TABLE -- part_rot [P,3,3] and one part index per point -- which is what the gather
kernel reads (csrc/chain.hip, chain_gather_kernel<REC, ROT = true>); nothing here expands to [N,3,3].  Stock torch ops on the tensors' device:
this runs once per edit.
"""
import numpy as np
import torch

from ._lib import HnrError

MAX_PARTS = 65536
_KEYS = ("points_embeding", "points_conf", "points_dir", "points_color")


def load_part(src, inds=None, transform=None, map_location=None):
    """One part of an edit: (state dict, bool mask [N], 4x4 transform).
    src: a `*_net_ray_marching.pth` path or a state dict with the `neural_points.*` keys.
    inds: None (all points), a bool mask [N], or the path of a `parts_index/*.txt` file (np.loadtxt: one 0 / 1 per point, :127,136).
    transform: None (identity), a 4x4 matrix, or the path of a `transforms/*.txt` file (np.loadtxt, :126,128)."""
    state = torch.load(src, map_location=map_location) if isinstance(src, (str, bytes)) or hasattr(src, "__fspath__") else src
    if "neural_points.xyz" not in state:
        raise HnrError("edit.load_part: no neural_points.xyz in the checkpoint")
    if "neural_points.eulers" in state:
        raise HnrError("edit.load_part: per-point `eulers` are unsupported (no shipped script writes them); only Rw2c is")
    xyz = state["neural_points.xyz"]
    dev, n = xyz.device, int(xyz.shape[0])
    if inds is None:
        mask = torch.ones(n, dtype=torch.bool, device=dev)
    else:
        if isinstance(inds, (str, bytes)) or hasattr(inds, "__fspath__"):
            inds = np.loadtxt(inds)
        mask = torch.as_tensor(inds, dtype=torch.bool, device=dev).reshape(-1)           # (:191)
        if mask.shape[0] != n:
            raise HnrError("edit.load_part: the index mask has %d entries, the cloud %d points" % (mask.shape[0], n))
    if transform is None:
        mat = torch.eye(4, dtype=torch.float32, device=dev)
    else:
        if isinstance(transform, (str, bytes)) or hasattr(transform, "__fspath__"):
            transform = np.loadtxt(transform)
        mat = torch.as_tensor(transform, dtype=torch.float32, device=dev)
        if tuple(mat.shape) != (4, 4):
            raise HnrError("edit.load_part: the transform must be 4x4 (got %s)" % (tuple(mat.shape),))
    return dict(state=state, inds=mask, transform=mat)


def _source_table(state, mask):
    """(part index of the selected points, part_rot [P,3,3]) of a source's own Rw2c, or (None, None)."""
    R = state.get("neural_points.Rw2c")
    if R is None:
        return None, None
    R = R.detach().to(torch.float32)
    k = int(mask.sum())
    if R.dim() == 2:
        return torch.zeros(k, dtype=torch.int64, device=R.device), R[None]
    rot, inv = torch.unique(R.reshape(-1, 9)[mask], dim=0, return_inverse=True)
    return inv, rot.reshape(-1, 3, 3)


def compose(parts):
    """Merge parts (load_part results, or (state, inds, transform) tuples) in list order.  Returns the reference's checkpoint keys
    `neural_points.xyz` [N,3], `.points_embeding` / `.points_conf` / `.points_dir` / `.points_color` [1,N,C] and the part table:
    `part` [N] int32, `part_rot` [P,3,3] float32 (Rw2c of point i = part_rot[part[i]]; expand_Rw2c gives the reference's [N,3,3])."""
    if len(parts) == 0:
        raise HnrError("edit.compose: no parts")
    xyz_all, part_all, rot_all, feats = [], [], [], {k: [] for k in _KEYS}
    n_rot = 0
    for p in parts:
        if not isinstance(p, dict):
            p = dict(state=p[0], inds=p[1], transform=p[2])
        state, mask, mat = p["state"], p["inds"], p["transform"]
        xyz = state["neural_points.xyz"].detach()
        mask = torch.as_tensor(mask, dtype=torch.bool, device=xyz.device)
        mat = torch.as_tensor(mat, dtype=torch.float32, device=xyz.device)
        Rot, Tran = mat[:3, :3], mat[:3, 3]
        sel = xyz[mask].to(torch.float32)
        xyz_all.append(sel @ Rot.transpose(0, 1) + Tran)                                   # (:196-199)
        idx, rot = _source_table(state, mask)
        if rot is None:
            idx, rot = torch.zeros(sel.shape[0], dtype=torch.int64, device=xyz.device), Rot[None]
        else:
            rot = rot.to(xyz.device) @ Rot.transpose(0, 1)                                 # (:201: w2c is reversed against movement)
        part_all.append(idx.to(xyz.device) + n_rot)
        rot_all.append(rot)
        n_rot += int(rot.shape[0])
        if n_rot > MAX_PARTS:
            raise HnrError("edit.compose: more than %d distinct rotations (%d so far); the part table holds at most %d" % (MAX_PARTS, n_rot, MAX_PARTS))
        for k in _KEYS:
            t = state.get("neural_points." + k)
            if t is None:
                raise HnrError("edit.compose: a part has no neural_points.%s" % k)
            feats[k].append(t.detach()[:, mask, :])
    out = {"neural_points.xyz": torch.cat(xyz_all, dim=0)}
    for k in _KEYS:
        out["neural_points." + k] = torch.cat(feats[k], dim=1)
    out["part"] = torch.cat(part_all, dim=0).to(torch.int32)
    out["part_rot"] = torch.cat(rot_all, dim=0).contiguous()
    return out


def expand_Rw2c(composed):
    """The reference's Rw2c_all [N,3,3] of a composed cloud (36 bytes per point: for comparisons, not for rendering)."""
    return composed["part_rot"][composed["part"].long()]


def apply(neural_points, composed):
    """editing_set_points (neural_points.py:473-487) with the composed cloud; the part table goes through as it is."""
    neural_points.editing_set_points(composed["neural_points.xyz"], composed["neural_points.points_embeding"],
                                     points_color=composed["neural_points.points_color"], points_dir=composed["neural_points.points_dir"],
                                     points_conf=composed["neural_points.points_conf"], Rw2c=(composed["part"], composed["part_rot"]))
    return neural_points
