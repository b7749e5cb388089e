"""Restatements for the scene-editing tests (tests/test_edit.py, tests/test_edit_gpu.py).

compose_ref64: run/editiing.py:196-209 in fp64 -- per part xyz' = [xyz 1] Mat^T, Rw2c' = Rot (a source without rotations) or Rw2c_src Rot^T,
  expanded to one matrix per point, features taken unchanged for the selected indices, parts concatenated in list order.  (The reference expands a
  source's Rw2c with `Rw2c[None].expand(len(xyz))`, which only works for a 2-D source; a 3-D source is indexed by the mask here, the only reading
  that keeps one matrix per selected point.)

gather_rot_ref: what chain_gather_kernel<ROT = true> writes per neighbour row, elementwise in fp32 with the kernel's operation order
  (models/aggregators/point_aggregators.py:894-898, 908, 927, 967-971): y = R x is y_i = (R[i][0] x_0 + R[i][1] x_1) + R[i][2] x_2, every product
  and sum rounded on its own (separate torch ops: nothing is contracted).  The sample's view direction is turned by the rotation of the point
  in SLOT 0, a neighbour's offset and stored direction by its own point's.
"""
import numpy as np
import torch


def compose_ref64(parts):
    """parts: list of (state dict, bool mask, 4x4) -> dict of fp64 arrays: xyz [N,3], Rw2c [N,3,3], emb / conf / dir / color [1,N,C]."""
    xyz_all, R_all = [], []
    feats = {k: [] for k in ("points_embeding", "points_conf", "points_dir", "points_color")}
    for state, mask, mat in parts:
        mask = np.asarray(mask).astype(bool)
        mat = np.asarray(mat, np.float64)
        Rot, Tran = mat[:3, :3], mat[:3, 3]
        Mat = np.eye(4)
        Mat[:3, :3], Mat[:3, 3] = Rot, Tran
        xyz = np.asarray(state["neural_points.xyz"], np.float64)[mask]
        xyz = (np.concatenate([xyz, np.ones_like(xyz[:, :1])], -1) @ Mat.T)[:, :3]
        src = state.get("neural_points.Rw2c")
        if src is None:
            Rw2c = np.broadcast_to(Rot, (len(xyz), 3, 3))
        else:
            src = np.asarray(src, np.float64)
            Rw2c = np.broadcast_to(src @ Rot.T, (len(xyz), 3, 3)) if src.ndim == 2 else src[mask] @ Rot.T
        xyz_all.append(xyz)
        R_all.append(Rw2c)
        for k in feats:
            feats[k].append(np.asarray(state["neural_points." + k], np.float64)[:, mask, :])
    out = dict(xyz=np.concatenate(xyz_all, 0), Rw2c=np.concatenate(R_all, 0))
    for k, v in feats.items():
        out[k] = np.concatenate(v, 1)
    return out


def rot3(R, x):
    """R [...,3,3], x [...,3] fp32 -> R x with the kernel's rounding order."""
    return torch.stack([(R[..., i, 0] * x[..., 0] + R[..., i, 1] * x[..., 1]) + R[..., i, 2] * x[..., 2] for i in range(3)], dim=-1)


def gather_rot_ref(xyz, pdir, color, part, part_rot, pidx, loc_w, raydir):
    """pidx [S,8] int (-1: empty), loc_w [S,3], raydir [S,3] (the sample's ray); the point buffers [N,3], part [N] integer, part_rot [P,3,3].
    Returns pid [S,8], ext [S,8,7] = [colour | dir' - v' | dir' . v'] (zeros in empty slots), v' [S,3], the rotated offsets [S,8,3]."""
    S = pidx.shape[0]
    valid = pidx >= 0
    pi = pidx.clamp(min=0).long()
    R = part_rot[part.long()[pi]]                                   # [S,8,3,3]
    R0 = R[:, 0]                                                    # slot 0's point
    v = rot3(R0, raydir)                                            # [S,3]
    d = xyz[pi] - loc_w[:, None, :]
    dr = rot3(R, d)
    dd = rot3(R, pdir[pi])
    vb = v[:, None, :].expand(S, 8, 3)
    dot = (dd[..., 0] * vb[..., 0] + dd[..., 1] * vb[..., 1]) + dd[..., 2] * vb[..., 2]
    ext = torch.cat([color[pi], dd - vb, dot[..., None]], dim=-1)
    ext = torch.where(valid[..., None], ext, torch.zeros_like(ext))
    return pidx, ext, v, torch.where(valid[..., None], dr, torch.zeros_like(dr))


def viewdir_encoding64(v):
    """positional_encoding(v, 4, ori=True)[3:] in fp64 of the fp32 arguments v * 2^f (exact products): [sin x12 | cos x12], column 4 d + f."""
    x = (v.double()[:, :, None] * (2.0 ** torch.arange(4, device=v.device, dtype=torch.float64))).reshape(v.shape[0], 12)
    return torch.cat([torch.sin(x), torch.cos(x)], dim=-1)


def tile_rows(n_big, n_small, n_tiny):
    """(sample index or -1, slot) of every row of the gather's 128-row tiles (csrc/chain_defs.h: 16 samples x 8 slots, then 32 x 4, then 64 x 2;
    every class ends in a partly filled tile)."""
    rows_s, rows_k = [], []
    first = 0
    for kc, n in enumerate((n_big, n_small, n_tiny)):
        per, slots = 16 << kc, 8 >> kc
        for t in range((n + per - 1) // per):
            r = np.arange(128)
            s = first + t * per + (r >> (3 - kc))
            rows_s.append(np.where(s < first + n, s, -1))
            rows_k.append(r & (slots - 1))
        first += n
    return np.concatenate(rows_s), np.concatenate(rows_k)
