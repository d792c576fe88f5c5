"""The denoiser (tmpt_denoise / Scene.denoise) against a numpy float32
restatement of the contract in include/tmpt.h (tmpt_denoise_desc), bit for bit:
one rounding per operation, the taps in the stated order, no tolerance.  The
restatement is written from the header, not from the kernel."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import toymeshpathtracer_amd as tm
from conftest import ROOT, data

pytestmark = pytest.mark.gpu

f32 = np.float32
CHECK_LIB = os.path.join(ROOT, "toymeshpathtracer_amd", "_lib_check", "libtmpt.so")
H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], f32)


def _dot(a, b):  # (ax*bx + ay*by) + az*bz
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def pack(rad):
    """pack_pixel(col, 1.0f) (main.cpp:224-233): uint8(saturate(sqrtf(k)) * 255), alpha 255."""
    out = np.full(rad.shape[:-1] + (4,), 255, np.uint8)
    out[..., :3] = (np.minimum(np.maximum(np.sqrt(rad[..., :3]), f32(0)), f32(1)) * f32(255)).astype(np.uint8)
    return out


def np_denoise(rad, aov, spp, levels=0, normal_exp=-1, sigma_depth=0.0, sigma_direct=0.0):
    """include/tmpt.h, tmpt_denoise_desc, restated: float32 arrays, one numpy
    operation per operation of the contract."""
    h, w = rad.shape[:2]
    levels = levels or 5
    normal_exp = 5 if normal_exp < 0 else normal_exp
    sigma_depth = f32(sigma_depth) if sigma_depth else f32(1) / f32(h)
    sigma_direct = f32(sigma_direct) if sigma_direct else f32(0.05)
    hits = aov["hits"]
    cov = hits > 0
    nrm = np.ascontiguousarray(aov["normal"], f32)
    nh = nrm * (f32(1) / np.sqrt(np.fmax(_dot(nrm, nrm), f32(1e-30))))[..., None]
    with np.errstate(all="ignore"):  # zb is read only where cov
        zb = np.where(cov, aov["depth"] * (f32(spp) / hits.astype(f32)), f32(1)).astype(f32)
    dl = np.ascontiguousarray(aov["direct"], f32)
    cur = np.ascontiguousarray(rad, f32).copy()
    for level in range(levels):
        s = 1 << level
        csum = np.zeros((h, w, 3), f32)
        wsum = np.zeros((h, w), f32)
        for j in range(-2, 3):
            for i in range(-2, 3):
                # the pixels p whose tap q = p + s (i, j) lies in the frame
                py = slice(max(0, -s * j), min(h, h - s * j))
                px = slice(max(0, -s * i), min(w, w - s * i))
                if py.start >= py.stop or px.start >= px.stop:
                    continue
                qy = slice(py.start + s * j, py.stop + s * j)
                qx = slice(px.start + s * i, px.stop + s * i)
                covp, covq = cov[py, px], cov[qy, qx]
                if i == 0 and j == 0:
                    wt = np.full(covp.shape, H5[2] * H5[2], f32)
                else:
                    base = H5[i + 2] * H5[j + 2]
                    c = np.fmax(f32(0), _dot(nh[py, px], nh[qy, qx]))
                    for _ in range(normal_exp):
                        c = c * c
                    g = base * c
                    zp, zq = zb[py, px], zb[qy, qx]
                    with np.errstate(all="ignore"):
                        rz = (zp - zq) / ((sigma_depth * np.fmin(zp, zq)) * f32(s * max(abs(i), abs(j))))
                        g = g * (f32(1) / (f32(1) + rz * rz))
                        rd = (dl[py, px] - dl[qy, qx]) / sigma_direct
                        g = g * (f32(1) / (f32(1) + rd * rd))
                    wt = np.where(covp, g, base).astype(f32)
                take = covp == covq
                csum[py, px] = np.where(take[..., None], csum[py, px] + cur[qy, qx, :3] * wt[..., None], csum[py, px])
                wsum[py, px] = np.where(take, wsum[py, px] + wt, wsum[py, px])
        nxt = cur.copy()  # .w passes through
        nxt[..., :3] = csum / wsum[..., None]
        cur = nxt
    assert cur.dtype == f32
    return cur


def _bits_equal(got, want, what=""):
    a, b = np.ascontiguousarray(got, f32).view(np.uint32), np.ascontiguousarray(want, f32).view(np.uint32)
    bad = np.argwhere(a != b)
    assert len(bad) == 0, f"{what}: {len(bad)} of {a.size} floats differ, first at {bad[0]}: " \
                          f"{got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}"


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v)).astype(f32)


def synthetic(w, h, spp=8, seed=1):
    """A frame with every edge the weights know: a sky region (hits = 0) with an
    irregular border and hits < spp along it, a normal crease (perpendicular,
    and one of 10 degrees), a depth step on a slanted depth ramp, a step in
    `direct`, and a covered pixel whose normal sums to exactly 0."""
    rng = np.random.default_rng(seed * 1000 + w * 37 + h)
    rad = (rng.random((h, w, 4)) * 4).astype(f32)
    aov = np.zeros((h, w), tm.AOV_DTYPE)
    y, x = np.mgrid[0:h, 0:w]
    border = 0.62 * h + 0.18 * h * np.sin(x * 0.9) + rng.integers(-1, 2, (h, w))
    sky = y > border
    if w * h == 1:
        sky[:] = False
    hits = np.full((h, w), spp, np.uint32)
    edge = ~sky & (np.roll(sky, 1, 0) | np.roll(sky, -1, 0) | np.roll(sky, 1, 1) | np.roll(sky, -1, 1))
    hits[edge] = rng.integers(1, spp, int(edge.sum()))
    hits[sky] = 0
    up, side = _unit([0.1, 1.0, 0.2]), _unit([1.0, -0.1, 0.0])
    ten = _unit(np.asarray(up, np.float64) + np.tan(np.radians(10.0)) * np.cross(up, [0.0, 0.0, 1.0]))
    nrm = np.empty((h, w, 3), f32)
    nrm[:] = up
    nrm[x >= (2 * w) // 5] = side   # perpendicular crease
    nrm[x >= (4 * w) // 5] = ten    # and 10 degrees off the first region's
    cover = (hits.astype(f32) / f32(spp))
    nrm = nrm * (cover * (f32(0.8) + f32(0.2) * rng.random((h, w)).astype(f32)))[..., None]  # sums of hit normals / spp
    t = f32(3.0) + f32(0.05) * x.astype(f32) + f32(0.02) * y.astype(f32)   # slanted ramp
    t = t + np.where(y >= h // 3, f32(1.5), f32(0)).astype(f32)            # depth step
    direct = np.where((x + y) % max(2, w // 2) < max(1, w // 4), f32(0.85), f32(0.05)).astype(f32) * cover
    if w * h > 8:
        inner = np.argwhere(~sky & ~edge)
        inner = inner if len(inner) else np.argwhere(~sky)
        cy, cx = inner[len(inner) // 2]
        nrm[cy, cx] = 0   # the hit normals of this pixel cancel exactly
    aov["normal"], aov["depth"], aov["direct"] = nrm, (t * cover).astype(f32), direct
    aov["hits"], aov["lit"] = hits, (hits // 2)
    aov["tri_id"] = np.where(hits > 0, 3, -1)
    aov["normal"][sky], aov["depth"][sky], aov["direct"][sky] = 0, 0, 0
    return rad, aov, spp


@functools.lru_cache(maxsize=None)
def _cube_scene_args():
    return tm.load_scene(data("cube.obj"))


def _any_scene():
    tris, bmin, bmax = _cube_scene_args()
    return tm.Scene(tris, bounds=(bmin, bmax))


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (37, 23), (130, 9)])
def test_synthetic_frames_bit_for_bit(gpu, w, h):
    rad, aov, spp = synthetic(w, h)
    cov = aov["hits"] > 0
    if w * h > 8:
        assert cov.any() and not cov.all() and ((aov["hits"] > 0) & (aov["hits"] < spp)).any()
        assert (cov & (np.abs(aov["normal"]).sum(-1) == 0)).any()
    with _any_scene() as sc:
        for levels in range(1, 7):
            for nexp in (0, 5, 8):
                want = np_denoise(rad, aov, spp, levels, nexp)
                for lds in (0, 1):
                    sc.set_option("denoise_lds", lds)
                    got, img = sc.denoise(rad, aov, spp, levels=levels, normal_exp=nexp)
                    _bits_equal(got, want, f"{w}x{h} levels={levels} normal_exp={nexp} denoise_lds={lds}")
                    assert np.array_equal(img, pack(want))
        sc.set_option("denoise_lds", -1)
        # the defaults by their 0 / -1 values, other sigmas, and the filter in place
        want = np_denoise(rad, aov, spp)
        got, img = sc.denoise(rad, aov, spp)
        _bits_equal(got, want, "defaults")
        _bits_equal(got, np_denoise(rad, aov, spp, 5, 5, f32(1) / f32(h), f32(0.05)), "defaults spelled out")
        for levels in (1, 2, 5):
            want = np_denoise(rad, aov, spp, levels, 3, 0.05, 0.3)
            buf = rad.copy()
            got, img = sc.denoise(buf, aov, spp, levels=levels, normal_exp=3, sigma_depth=0.05, sigma_direct=0.3,
                                  out=buf)
            assert got is buf
            _bits_equal(buf, want, f"in place, levels={levels}")
            assert np.array_equal(img, pack(want))
    assert (want[..., 3].view(np.uint32) == rad[..., 3].view(np.uint32)).all()  # .w passes through


def test_no_leakage_across_coverage(gpu):
    rad, aov, spp = synthetic(37, 23)
    cov = aov["hits"] > 0
    rng = np.random.default_rng(5)
    sky_changed, cov_changed = rad.copy(), rad.copy()
    sky_changed[~cov] = (rng.random((int((~cov).sum()), 4)) * 9).astype(f32)
    cov_changed[cov] = (rng.random((int(cov.sum()), 4)) * 9).astype(f32)
    with _any_scene() as sc:
        base, _ = sc.denoise(rad, aov, spp)
        a, _ = sc.denoise(sky_changed, aov, spp)
        b, _ = sc.denoise(cov_changed, aov, spp)
    u = lambda v: v.view(np.uint32)
    assert (u(a)[cov] == u(base)[cov]).all() and (u(a)[~cov][:, :3] != u(base)[~cov][:, :3]).any()
    assert (u(b)[~cov] == u(base)[~cov]).all() and (u(b)[cov][:, :3] != u(base)[cov][:, :3]).any()


@functools.lru_cache(maxsize=None)
def _frame(name, w, h, spp):
    tris, bmin, bmax = tm.load_scene(data(name))
    cam = tm.Camera.for_scene(bmin, bmax, w, h)
    with tm.Scene(tris, bounds=(bmin, bmax)) as sc:
        rad, _, _ = sc.trace_radiance(cam, w, h, spp)
        aov, _ = sc.trace_aov(cam, w, h, spp)
    return rad, aov


@pytest.mark.parametrize("name,w,h", [("suzanne.obj", 64, 36), ("cube.obj", 32, 18)])
def test_real_frame_bit_for_bit(gpu, name, w, h):
    spp = 4
    rad, aov = _frame(name, w, h, spp)
    cov = aov["hits"] > 0
    assert cov.any() and not cov.all()
    want = np_denoise(rad, aov, spp)
    with _any_scene() as sc:
        for lds in (0, 1, -1):
            sc.set_option("denoise_lds", lds)
            got, img = sc.denoise(rad, aov, spp)
            _bits_equal(got, want, f"{name} denoise_lds={lds}")
            assert np.array_equal(img, pack(want))
    assert not np.array_equal(want[..., :3], rad[..., :3])


def _rmse(a, b):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float(np.sqrt((d * d).mean()))


@pytest.mark.parametrize("name", ["suzanne.obj", "teapot.obj"])
def test_it_denoises(gpu, name):
    """RMSE against the 512-spp frame, over r, g, b, with the defaults:
    the filtered 4-spp frame is closer than the 4-spp frame."""
    w, h = 96, 54
    noisy, aov = _frame(name, w, h, 4)
    truth, _ = _frame(name, w, h, 512)
    with _any_scene() as sc:
        den, _ = sc.denoise(noisy, aov, 4)
    e_noisy, e_den = _rmse(noisy, truth), _rmse(den, truth)
    print(f"{name} {w}x{h}: E_noisy = {e_noisy:.5f}  E_den = {e_den:.5f}  ratio {e_den / e_noisy:.3f}")
    assert e_den < e_noisy


def test_device_pointers(gpu):
    import torch

    w, h, spp = 64, 36, 4
    rad, aov = _frame("suzanne.obj", w, h, spp)
    with _any_scene() as sc:
        want, want8 = sc.denoise(rad, aov, spp)
        one, _ = sc.denoise(rad, aov, spp, levels=1)
        t_in = torch.from_numpy(rad).to("cuda:0")
        t_aov = torch.from_numpy(aov.view(np.uint8).reshape(h, w, 32).copy()).to("cuda:0")
        t_out = torch.full((h, w, 4), 7.0, dtype=torch.float32, device="cuda:0")
        t_8 = torch.full((h, w, 4), 7, dtype=torch.uint8, device="cuda:0")
        size = dict(width=w, height=h)
        assert sc.denoise(t_in.data_ptr(), t_aov.data_ptr(), spp, out=(t_out.data_ptr(), t_8.data_ptr()),
                          **size) == (None, None)
        got, got8 = t_out.cpu().numpy(), t_8.cpu().numpy()
        t_8.fill_(9)
        sc.denoise(t_in.data_ptr(), t_aov.data_ptr(), spp, out=(None, t_8.data_ptr()), **size)  # bytes alone
        only8 = t_8.cpu().numpy()
        assert t_in.cpu().numpy().tobytes() == rad.tobytes()  # the input is not written
        t_one = t_in.clone()
        sc.denoise(t_one.data_ptr(), t_aov.data_ptr(), spp, levels=1, out=(t_one.data_ptr(), None), **size)
        sc.denoise(t_in.data_ptr(), t_aov.data_ptr(), spp, out=(t_in.data_ptr(), None), **size)  # in place
        inplace, inplace1 = t_in.cpu().numpy(), t_one.cpu().numpy()
    assert got.tobytes() == want.tobytes() and np.array_equal(got8, want8) and np.array_equal(only8, want8)
    assert inplace.tobytes() == want.tobytes() and inplace1.tobytes() == one.tobytes()


def test_denoise_leaves_the_progressive_state_alone(gpu):
    w, h, spp = 32, 18, 8
    tris, bmin, bmax = tm.load_scene(data("suzanne.obj"))
    cam = tm.Camera.for_scene(bmin, bmax, w, h)
    with tm.Scene(tris, bounds=(bmin, bmax)) as sc:
        once, rays = sc.trace_image(cam, w, h, spp, seed_mode=tm.SEED_PIXEL)
        rad, _, _ = sc.trace_radiance(cam, w, h, spp)
        aov, _ = sc.trace_aov(cam, w, h, spp)
        alone, _ = sc.denoise(rad, aov, spp)
        passes = sc.trace_progressive(cam, w, h, spp, [3, 5], seed_mode=tm.SEED_PIXEL)
        done, _, r_a = next(passes)
        between, _ = sc.denoise(rad, aov, spp)
        done, last, r_b = next(passes)
    assert done == spp and np.array_equal(last, once) and r_a + r_b == rays
    assert between.tobytes() == alone.tobytes()


def test_cli_denoise_png(gpu, tmp_path):
    from PIL import Image

    w, h, spp = 32, 18, 4
    cli = os.path.join(os.path.dirname(tm.lib_path), "tmpt")
    out = str(tmp_path / "den.png")
    r = subprocess.run([cli, str(w), str(h), str(spp), data("suzanne.obj"), "--seed", "sample", "--denoise", out,
                        "--out", str(tmp_path / "frame.png")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rad, aov = _frame("suzanne.obj", w, h, spp)
    with _any_scene() as sc:
        _, want8 = sc.denoise(rad, aov, spp)
    assert np.array_equal(np.asarray(Image.open(out).convert("RGBA"))[::-1], want8)  # flipped on write
    for extra in (["--seed", "row"], ["--seed", "sample", "--gpus", "2"]):
        r = subprocess.run([cli, str(w), str(h), str(spp), data("suzanne.obj"), "--denoise", out] + extra,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--denoise" in r.stdout


CHILD = r'''
import hashlib, json, sys
sys.path.insert(0, sys.argv[1])
import toymeshpathtracer_amd as tm
tris, bmin, bmax = tm.load_scene(sys.argv[2])
out = {}
try:
    with tm.Scene(tris, bounds=(bmin, bmax)) as sc:
        cam = tm.Camera.for_scene(bmin, bmax, 64, 36)
        rad, _, _ = sc.trace_radiance(cam, 64, 36, 4)
        aov, _ = sc.trace_aov(cam, 64, 36, 4)
        for lds in (0, 1):
            sc.set_option("denoise_lds", lds)
            den, img = sc.denoise(rad, aov, 4)
            out[str(lds)] = [hashlib.sha256(den.tobytes()).hexdigest(), hashlib.sha256(img.tobytes()).hexdigest()]
except tm.TmptError as e:
    out["error"] = str(e)
print(json.dumps(out))
'''


@pytest.mark.skipif(not os.path.exists(CHECK_LIB),
                    reason="checked build not built (make -C toymeshpathtracer_amd/csrc CHECK=1)")
def test_denoise_checked_build(gpu):
    """The checked library filters the same frame to the same bits."""
    env = dict(os.environ, TMPT_NO_TORCH="1", TMPT_LIB_PATH=CHECK_LIB)
    env.pop("TMPT_CHECK_SELFTEST", None)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, data("suzanne.obj")], capture_output=True, text=True,
                       timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert "error" not in got, got
    rad, aov = _frame("suzanne.obj", 64, 36, 4)
    with _any_scene() as sc:
        den, img = sc.denoise(rad, aov, 4)
    want = [hashlib.sha256(den.tobytes()).hexdigest(), hashlib.sha256(img.tobytes()).hexdigest()]
    assert got == {"0": want, "1": want}
