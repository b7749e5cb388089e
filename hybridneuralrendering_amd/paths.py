"""Camera paths on the host: the c2w poses frames.PathSampler / driver.render_path draw.  float64 arithmetic, float32 [n,4,4] results, the
reference's camera convention (x right, y down, z forward: what its datasets hold after `@ blender2opencv`).

`spherical_path` is the orbit of the synthetic scenes (data/nerf_synth360_ft_dataset.py:235-239, get_render_poses over pose_spherical);
`keyframe_path` is for scanned scenes, where the reference has nothing: a curve through poses the user picked (train cameras, a viewer's bookmarks).
"""
import numpy as np

from ._lib import HnrError


def spherical_path(n=20, elevation=-30.0, radius=4.0):
    """`get_render_poses`: pose_spherical(angle, elevation, radius) @ blender2opencv for angle in linspace(-180, 180, n + 1)[:-1] -> [n,4,4] float32.
    The camera sits at `radius` from the origin and looks at it.  As the reference, the factors are rounded to float32 when they are formed
    (its trans_t / rot_phi / rot_theta are float32 arrays) and the products run in float64."""
    n = int(n)
    if n < 1 or not radius > 0:
        raise HnrError("spherical_path: n >= 1 and radius > 0")
    f32 = lambda rows: np.asarray(rows, dtype=np.float32).astype(np.float64)
    phi = float(elevation) / 180. * np.pi
    trans = f32([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, radius], [0, 0, 0, 1]])
    rphi = f32([[1, 0, 0, 0], [0, np.cos(phi), -np.sin(phi), 0], [0, np.sin(phi), np.cos(phi), 0], [0, 0, 0, 1]])
    flip = np.array([[-1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=np.float64)
    b2cv = np.diag([1.0, -1.0, -1.0, 1.0])
    out = []
    for angle in np.linspace(-180, 180, n + 1)[:-1]:
        th = angle / 180. * np.pi
        rth = f32([[np.cos(th), 0, -np.sin(th), 0], [0, 1, 0, 0], [np.sin(th), 0, np.cos(th), 0], [0, 0, 0, 1]])
        out.append(flip @ (rth @ (rphi @ trans)) @ b2cv)
    return np.stack(out, 0).astype(np.float32)


def _quat(R):
    """unit quaternion (w, x, y, z) of a rotation matrix (Shepperd's branches: the largest of w, x, y, z is the pivot)"""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
        q = [0.0, 0.0, 0.0, 0.0]
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i], q[1 + j], q[1 + k] = 0.25 * s, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s
    q = np.asarray(q, dtype=np.float64)
    return q / np.linalg.norm(q)


def _rot(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=np.float64)


def _slerp(q0, q1, u):
    """the shorter arc from q0 to q1; nearly parallel quaternions: normalised linear interpolation"""
    d = float(np.dot(q0, q1))
    if d < 0:
        q1, d = -q1, -d
    if d > 1 - 1e-10:
        q = q0 + u * (q1 - q0)
    else:
        w = np.arccos(d)
        q = (np.sin((1 - u) * w) * q0 + np.sin(u * w) * q1) / np.sin(w)
    return q / np.linalg.norm(q)


def keyframe_path(c2w_keys, n_frames, closed=False):
    """A path of `n_frames` frames through the key poses c2w_keys [k,4,4] (k >= 2) -> [n_frames,4,4] float32.  An open path has k - 1 segments and
    ends on the last key; a closed one has k segments, the last returning to the first key (its last frame IS the first key again).  Key s sits at
    frame round(s (n_frames - 1) / segments) and is reproduced exactly (its own float32 values); n_frames >= segments + 1, so every key has a frame
    of its own.  Between two keys the frames are evenly spaced in the segment's parameter u: the position follows the uniform Catmull-Rom spline
    through the keys (the end tangents of an open path use the end key twice) and the rotation is the slerp of the two keys' quaternions along
    the shorter arc."""
    keys = np.asarray(c2w_keys)
    n_frames = int(n_frames)
    if keys.ndim != 3 or keys.shape[1:] != (4, 4) or keys.shape[0] < 2:
        raise HnrError("keyframe_path: c2w_keys must be [k,4,4] with k >= 2, got %s" % (keys.shape,))
    if not np.isfinite(keys).all():
        raise HnrError("keyframe_path: a key pose is not finite")
    k = keys.shape[0]
    segs = k if closed else k - 1
    if n_frames < segs + 1:
        raise HnrError("keyframe_path: %d keys%s need n_frames >= %d" % (k, " on a closed path" if closed else "", segs + 1))
    k64 = keys.astype(np.float64)
    pos = k64[:, :3, 3]
    quats = [_quat(M[:3, :3]) for M in k64]
    key = (lambda i: i % k) if closed else (lambda i: min(max(i, 0), k - 1))
    at = [(2 * s * (n_frames - 1) + segs) // (2 * segs) for s in range(segs + 1)]        # round half up, in integers
    out = np.empty((n_frames, 4, 4), dtype=np.float32)
    for s in range(segs):
        p0, p1, p2, p3 = (pos[key(s + o)] for o in (-1, 0, 1, 2))
        out[at[s]] = keys[key(s)]
        for f in range(at[s] + 1, at[s + 1]):
            u = (f - at[s]) / (at[s + 1] - at[s])
            M = np.eye(4)
            M[:3, 3] = 0.5 * ((2 * p1) + (-p0 + p2) * u + (2 * p0 - 5 * p1 + 4 * p2 - p3) * u * u + (-p0 + 3 * p1 - 3 * p2 + p3) * u ** 3)
            if np.array_equal(k64[key(s), :3, :3], k64[key(s + 1), :3, :3]):
                M[:3, :3] = k64[key(s), :3, :3]                 # a held orientation stays the key's own matrix, bit for bit
            else:
                M[:3, :3] = _rot(_slerp(quats[key(s)], quats[key(s + 1)], u))
            out[f] = M
    out[n_frames - 1] = keys[key(segs)]
    return out
