"""The camera pre-pass's entries (tmpt_camera_rays) restated from the oracle's
pieces, for any camera and frame: shared by test_gpu_cam_rays.py (the cameras of
test_gpu_cameras.py at 24x16x8) and call_kinds.py (the call-order matrix).
"""
import numpy as np

import oracle

f32 = np.float32


def _step(x):
    """xorshift32 (maths.cpp:5-13), checked against the oracle's in camera_samples_expect."""
    x ^= (x << 13) & 0xFFFFFFFF
    x ^= x >> 17
    x ^= (x << 15) & 0xFFFFFFFF
    return x


def camera_samples_expect(cam, W, H, SPP):
    """The whole W x H x SPP frame's camera samples through the camera array cam:
    (uint32[H, W, SPP, 7] origin, direction, RNG state after the camera's draws;
    disk tries[H, W, SPP]), as tests/render_restate.py::aov_expect makes its rays."""
    assert _step(12345) == int(oracle.xorshift_seq(12345, 1)[0])
    inv_w, inv_h = f32(1) / f32(W), f32(1) / f32(H)
    out = np.zeros((H, W, SPP, 7), np.uint32)
    tries = np.zeros((H, W, SPP), np.int32)
    for y in range(H):
        for x in range(W):
            seed = oracle.pixel_seed(x, y, W)
            for s in range(SPP):
                st = oracle.sample_seed(seed, s)
                r = oracle.float01_seq(st, 2)
                state = _step(_step(st))
                o, d, after = oracle.get_ray(cam, float((f32(x) + r[0]) * inv_w), float((f32(y) + r[1]) * inv_h), state)
                out[y, x, s, 0:3], out[y, x, s, 3:6], out[y, x, s, 6] = o.view(np.uint32), d.view(np.uint32), after
                n, z = 0, state
                while z != after:  # two draws per try of the lens disk
                    z = _step(_step(z))
                    n += 1
                    assert n < 64
                tries[y, x, s] = n
    out.setflags(write=False)
    return out, tries
