"""tmpt_render_moments (Scene.trace_moments) on the device: the luminance moments
against the restatement (noise_aware_restate.moments_expect) over the
reference's own per-sample colours (tests/golden/ref/trace_<case>.npz, 32x18x8),
and every other output against trace_adaptive of the same scene, bit for bit.
Floats are compared as bits; there is no tolerance."""
import functools

import numpy as np
import pytest

import toymeshpathtracer_amd as tm
from noise_aware_restate import moments_expect
from render_restate import same_bits
from test_gpu_reference_trace import CASES, CASE_IDS, SPP_MIN, SPP_STEP, TAU, _adaptive, _camera, _case, _scene

pytestmark = pytest.mark.gpu

f32 = np.float32


def _same_outputs(got, want, what):
    """(radiance, rgba8, spp_map, rays, info) of trace_moments against trace_adaptive's."""
    same_bits(got[0], want[0], what + " radiance")
    assert np.array_equal(got[1], want[1]), what + " bytes"
    assert np.array_equal(got[2], want[2]), what + " spp map"
    assert got[3] == want[3], f"{what}: rays {got[3]} vs {want[3]}"
    assert got[4] == want[4], f"{what}: info {got[4]} vs {want[4]}"


def _split(res):
    """trace_moments' result as (moments, the five things trace_adaptive returns)."""
    rad, mom, img, cnt, rays, info = res
    return mom, (rad, img, cnt, rays, info)


@functools.lru_cache(maxsize=None)
def _sample_colours(name):
    return _case(name)["col"][tm.SEED_SAMPLE]


@pytest.mark.parametrize("name,waves", CASES, ids=CASE_IDS)
def test_uniform_equals_reference(gpu, name, waves):
    """ad NULL (spp_min=None): one pass, every pixel at spp -- 8, 3 and 2."""
    c = _case(name)
    w, h = c["w"], c["h"]
    cam = _camera(name)
    with _scene(name, waves) as sc:
        for spp in (8, 3, 2):
            what = f"{name} uniform x{spp}, path_waves {waves}"
            mom, rest = _split(sc.trace_moments(cam, w, h, spp))
            assert mom.shape == (h, w, 4) and mom.dtype == f32
            same_bits(mom, moments_expect(_sample_colours(name), spp), what + " moments")
            assert (rest[2] == spp).all() and rest[4]["passes"] == 1 and rest[4]["pass_pixels"] == [w * h]
            _same_outputs(rest, sc.trace_adaptive(cam, w, h, spp, spp_min=spp), what)


@pytest.mark.parametrize("name,waves", CASES, ids=CASE_IDS)
def test_adaptive_equals_reference(gpu, name, waves):
    """Schedule 2, 4, 6, 8: the moments at each pixel's own count; with radius 1 too."""
    c = _case(name)
    w, h, cap = c["w"], c["h"], c["spp"]
    cam = _camera(name)
    want_n = _adaptive(name)[0]
    assert len(np.unique(want_n)) >= 3
    with _scene(name, waves) as sc:
        for radius in (0, 1):
            what = f"{name} tau {TAU[name]} radius {radius}, path_waves {waves}"
            mom, rest = _split(sc.trace_moments(cam, w, h, cap, SPP_MIN, SPP_STEP, TAU[name], radius=radius))
            _same_outputs(rest, sc.trace_adaptive(cam, w, h, cap, SPP_MIN, SPP_STEP, TAU[name], radius=radius), what)
            n_p = rest[2]
            if radius == 0:
                assert np.array_equal(n_p, want_n), what
            else:
                assert (n_p >= want_n).all(), what  # monotone in the radius (include/tmpt.h)
            same_bits(mom, moments_expect(_sample_colours(name), n_p), what + " moments")
            same_bits(mom[..., 2], f32(1) / n_p.astype(f32), what + " 1/n")
            assert (mom[..., 3] == 1).all()


@pytest.mark.parametrize("name", ["cube", "room"])
def test_sample_base_moves_the_window(gpu, name):
    """sample_base = 4 at spp 4: the moments of samples 4 .. 7 of the fixture."""
    c = _case(name)
    w, h = c["w"], c["h"]
    with _scene(name, 5) as sc:
        sc.set_option("sample_base", 4)
        mom, rest = _split(sc.trace_moments(_camera(name), w, h, 4))
        want = sc.trace_adaptive(_camera(name), w, h, 4, spp_min=4)
    same_bits(mom, moments_expect(_sample_colours(name)[:, :, 4:8], 4), f"{name} sample_base 4")
    _same_outputs(rest, want, f"{name} sample_base 4")


def test_shard_tiles_assemble(gpu):
    name = "room"
    c = _case(name)
    w, h, cap = c["w"], c["h"], c["spp"]
    cam = _camera(name)
    band, shards = 4, 3
    with _scene(name, 5) as sc:
        for kw in (dict(), dict(spp_min=SPP_MIN, spp_step=SPP_STEP, threshold=TAU[name], radius=1)):
            whole, rest = _split(sc.trace_moments(cam, w, h, cap, band_rows=band, **kw))
            frame = np.full((h, w, 4), np.nan, f32)
            f_n = np.zeros((h, w), np.int32)
            rays = 0
            for k in range(shards):
                mom, part = _split(sc.trace_moments(cam, w, h, cap, band_rows=band, shard=k, num_shards=shards, **kw))
                rows = tm.tile_row_to_y(w, h, band, k, shards)
                assert mom.shape == (len(rows), w, 4)
                frame[rows], f_n[rows] = mom, part[2]
                rays += part[3]
            same_bits(frame, whole, f"shards {kw}")
            assert np.array_equal(f_n, rest[2]) and rays == rest[3]


def test_device_pointers(gpu):
    import torch

    name = "cube"
    c = _case(name)
    w, h, cap = c["w"], c["h"], c["spp"]
    cam = _camera(name)
    args = (cam, w, h, cap, SPP_MIN, SPP_STEP, TAU[name])
    with _scene(name, 5) as sc:
        want_mom, want = _split(sc.trace_moments(*args))
        t32 = torch.full((h, w, 4), 7.0, dtype=torch.float32, device="cuda:0")
        tm4 = torch.full((h, w, 4), 7.0, dtype=torch.float32, device="cuda:0")
        t8 = torch.full((h, w, 4), 7, dtype=torch.uint8, device="cuda:0")
        tn = torch.full((h, w), 7, dtype=torch.int32, device="cuda:0")
        res = sc.trace_moments(*args, out=(t32.data_ptr(), tm4.data_ptr(), t8.data_ptr(), tn.data_ptr()))
        assert res[:4] == (None, None, None, None) and res[4] == want[3] and res[5] == want[4]
        got = (t32.cpu().numpy(), tm4.cpu().numpy(), t8.cpu().numpy(), tn.cpu().numpy())
        tm4.fill_(3.0)
        sc.trace_moments(*args, out=(None, tm4.data_ptr(), None, None))  # the moments alone
        only = tm4.cpu().numpy()
        with pytest.raises(tm.TmptError, match="moments_out"):
            sc.trace_moments(*args, out=(t32.data_ptr(), None, None, None))
        with pytest.raises(tm.TmptError, match="aligned"):
            sc.trace_moments(*args, out=(None, tm4.data_ptr() + 4, None, None))
    same_bits(got[1], want_mom, "device moments")
    same_bits(only, want_mom, "device moments alone")
    same_bits(got[0], want[0], "device radiance")
    assert np.array_equal(got[2], want[1]) and np.array_equal(got[3], want[2])


def test_moments_leave_the_progressive_state_alone(gpu):
    name = "room"
    c = _case(name)
    w, h, spp = c["w"], c["h"], c["spp"]
    cam = _camera(name)
    with _scene(name, 5) as sc:
        once, rays = sc.trace_image(cam, w, h, spp, seed_mode=tm.SEED_SAMPLE)
        alone = sc.trace_moments(cam, w, h, 4)
        passes = sc.trace_progressive(cam, w, h, spp, [3, 5], seed_mode=tm.SEED_SAMPLE)
        done, _, r_a = next(passes)
        assert done == 3
        between = sc.trace_moments(cam, w, h, 4)  # between the two passes
        done, last, r_b = next(passes)
    assert done == spp and np.array_equal(last, once) and r_a + r_b == rays
    same_bits(between[1], alone[1], "moments between two passes")
    _same_outputs(_split(between)[1], _split(alone)[1], "between two passes")
