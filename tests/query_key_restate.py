"""The sort key of option query_sort (include/tmpt.h, tmpt_query_keys) restated
in float32 numpy: every operation rounds once to float32, as the header states.

  inv[a] = 32 / fmax(box.max[a] - box.min[a], 1e-30)
  c[a]   = int(fmin(fmax((o[a] - box.min[a]) * inv[a], 0), 31))
  q[a]   = int(fmin(fmax((d[a] + 1) * 4, 0), 7))
  key    = morton3(c.x, c.y, c.z) << 9 | q.x << 6 | q.y << 3 | q.z
  a NaN anywhere in o or d: 0xFFFFFF

``keys(rays, box)``                   rays (n, 6) or (n, 8) float32 -> uint32 (n,)
``keys(rays, box, swap_yz=True)``     the same with y and z swapped in morton3: the
                                      mutation test_query_keys.py must see
"""
import numpy as np

f32 = np.float32
NAN_KEY = np.uint32(0xFFFFFF)


def _spread5(v):
    v = v.astype(np.uint32)
    return (v & 1) | ((v & 2) << 2) | ((v & 4) << 4) | ((v & 8) << 6) | ((v & 16) << 8)


def morton3(x, y, z):
    """x in the lowest bit of each triple."""
    return _spread5(x) | (_spread5(y) << 1) | (_spread5(z) << 2)


def keys(rays, box, swap_yz=False):
    rays = np.asarray(rays, f32)
    box = np.asarray(box, f32).reshape(6)
    o, d = rays[:, 0:3], rays[:, 3:6]
    with np.errstate(all="ignore"):
        ext = box[3:6] - box[0:3]
        inv = f32(32.0) / np.fmax(ext, f32(1e-30))
        assert inv.dtype == f32
        c = np.fmin(np.fmax((o - box[0:3]) * inv, f32(0.0)), f32(31.0))
        q = np.fmin(np.fmax((d + f32(1.0)) * f32(4.0), f32(0.0)), f32(7.0))
        assert c.dtype == f32 and q.dtype == f32
    nan = np.isnan(rays[:, :6]).any(1)
    c = np.where(nan[:, None], f32(0.0), c).astype(np.int32).astype(np.uint32)
    q = np.where(nan[:, None], f32(0.0), q).astype(np.int32).astype(np.uint32)
    m = morton3(c[:, 0], c[:, 2], c[:, 1]) if swap_yz else morton3(c[:, 0], c[:, 1], c[:, 2])
    k = (m << 9) | (q[:, 0] << 6) | (q[:, 1] << 3) | q[:, 2]
    return np.where(nan, NAN_KEY, k).astype(np.uint32)
