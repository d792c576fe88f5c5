"""The camera pre-pass of sample seeding (render option cam_pre: k_cam_rays
makes a pass's camera samples on full waves, the 5-wave sample kernels read
them) -- its entries against a CPU restatement from the oracle's pieces, a
render with it against the same render without it on one scene object, against
the oracle's frame, and the fallback when the buffer does not fit.
Tolerance: none -- bits, bytes and counts.
"""
import functools

import numpy as np
import pytest

import oracle
import toymeshpathtracer_amd as tm
from cam_rays_restate import camera_samples_expect
from conftest import data
from test_gpu_cameras import CAMERAS, _camera

f32 = np.float32
W, H, SPP = 24, 16, 8          # the entries' frame
RW, RH, RSPP = 160, 90, 16     # the on / off renders


@functools.lru_cache(maxsize=None)
def _expect(cam_name):
    """The whole 24x16x8 frame's camera samples through camera cam_name over
    suzanne (cam_rays_restate.camera_samples_expect)."""
    return camera_samples_expect(_camera("suzanne", cam_name).as_array(), W, H, SPP)


def _suzanne():
    tris, bmin, bmax = tm.load_scene(data("suzanne.obj"))
    return tris, (bmin, bmax)


@pytest.fixture(scope="module")
def suzanne_scene(gpu):
    tris, bounds = _suzanne()
    with tm.Scene(tris, bounds=bounds) as sc:
        yield sc


@pytest.mark.gpu
@pytest.mark.parametrize("cam_name", CAMERAS)
def test_entries_match_the_restatement(suzanne_scene, cam_name):
    """Origin, direction and RNG word of every entry, bit for bit, over one
    shard, shard 2 of 3 in bands of 1 and 2 rows, the pass [4, 8), and the pass
    [1, 7), whose 6 samples do not fill the pre-pass's blocks of 4."""
    want, tries = _expect(cam_name)
    # the rejection loop's divergent exit is covered, not assumed: ~4.6 % of the
    # samples take three or more tries (pinhole draws too, with lens radius 0)
    assert int((tries >= 3).sum()) >= 1 and int(tries.min()) >= 1, np.bincount(tries.ravel())
    cam = _camera("suzanne", cam_name)
    for band, shard, n, s0, cnt in ((0, 0, 1, 0, 0), (1, 1, 3, 0, 0), (2, 1, 3, 0, 0), (0, 0, 1, 4, 4), (0, 0, 1, 1, 6)):
        got = suzanne_scene.camera_rays(cam, W, H, SPP, spp_begin=s0, spp_count=cnt, band_rows=band, shard=shard,
                                        num_shards=n)
        ys = tm.tile_row_to_y(W, H, band, shard, n) if n > 1 else np.arange(H)
        c = cnt or SPP
        assert got.shape == (len(ys) * W, c, 8) and len(ys) > 0
        exp = want[ys][:, :, s0:s0 + c, :].reshape(len(ys) * W, c, 7)
        bad = np.argwhere(got[..., :7] != exp)
        assert len(bad) == 0, f"{cam_name} band {band} shard {shard}/{n} pass {s0}+{c}: {len(bad)} words differ, " \
                              f"first (slot, sample, word) {bad[0]}"
        assert not (got[..., 7] & ~np.uint32(3)).any()


def _render(sc, cam, w, h, spp, **kw):
    img, rays = sc.trace_image(cam, w, h, spp, seed_mode=tm.SEED_SAMPLE, **kw)
    st = sc.stats()
    return img.tobytes(), rays, (st.tie_queries, st.root_misses, st.crack_queries, st.redo_samples)


def _on_off(sc, cam, what, w=RW, h=RH, spp=RSPP, **kw):
    """One render with the pre-pass and one without on the same scene object:
    frame bytes, rays and the tie / root / crack / redo statistics equal, and
    the first really ran the pre-pass."""
    sc.set_option("cam_pre", 1)
    on = _render(sc, cam, w, h, spp, **kw)
    assert sc.get_option("cam_rays_used") == 1, what
    sc.set_option("cam_pre", 0)
    off = _render(sc, cam, w, h, spp, **kw)
    assert sc.get_option("cam_rays_used") == 0, what
    assert on[1:] == off[1:], f"{what}: rays / (ties, root misses, cracks, redo) {on[1:]} != {off[1:]}"
    assert on[0] == off[0], f"{what}: frames differ"
    return off


OPTION_CASES = [{"sample_block": 1}, {"sample_block": 2}, {"sample_block": 8}, {"sample_tail": 0}, {"sample_tail": -1},
                {"sbuf_pair": 0}, {"sbuf_pair": 1}, {"tie_defer": 0}, {"tie_defer": 1}, {"tie_rule": 1}]


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["suzanne", "cube"])
def test_on_equals_off(gpu, scene):
    """cam_pre 1 against 0 at 160x90x16, path_waves 5: the block sizes, the
    tail, the paired stores, the tie rules, the cameras whose rays miss the root
    box, shard 3 of 3, a two-pass progressive render and tmpt_render_radiance."""
    tris, bmin, bmax = tm.load_scene(data(scene + ".obj"))
    cam = tm.Camera.for_scene(bmin, bmax, RW, RH)
    with tm.Scene(tris, bounds=(bmin, bmax), options={"path_waves": 5}) as sc:
        defaults = {k: sc.get_option(k) for case in OPTION_CASES for k in case}
        for case in OPTION_CASES:
            for k, v in case.items():
                sc.set_option(k, v)
            _on_off(sc, cam, f"{scene} {case}")
            for k in case:
                sc.set_option(k, defaults[k])
        _on_off(sc, cam, f"{scene} shard 3 of 3", band_rows=1, shard=2, num_shards=3)
        misses = 0
        for name in ("away", "far"):
            if scene == "suzanne":  # test_gpu_cameras.py places them around suzanne
                misses += _on_off(sc, _camera("suzanne", name), f"{scene} camera {name}")[2][1]
        assert scene != "suzanne" or misses > 0  # the root box test was made, through the entries' flag
        # a two-pass progressive render: both passes' previews, and the state carried between them
        for on in (1, 0):
            sc.set_option("cam_pre", on)
            frames = [(img.tobytes(), rays, sc.get_option("cam_rays_used"))
                      for _, img, rays in sc.trace_progressive(cam, RW, RH, RSPP, [8, 8], seed_mode=tm.SEED_SAMPLE)]
            assert [f[2] for f in frames] == [on, on]
            if on:
                prog_on = frames
            else:
                assert [f[:2] for f in frames] == [f[:2] for f in prog_on]
        # the float radiance, as bits
        rad = {}
        for on in (1, 0):
            sc.set_option("cam_pre", on)
            r, img, rays = sc.trace_radiance(cam, RW, RH, RSPP)
            assert sc.get_option("cam_rays_used") == on
            rad[on] = (r.view(np.uint32).tobytes(), img.tobytes(), rays)
        assert rad[1] == rad[0]
        sc.set_option("sbuf_max", 1)  # without the colour buffer: the SUMS kernels
        for rule in (0, 1):  # ties for the octree, or the lowest index
            sc.set_option("tie_rule", rule)
            for on in (1, 0):
                sc.set_option("cam_pre", on)
                r, img, rays = sc.trace_radiance(cam, RW, RH, RSPP)
                assert sc.get_option("cam_rays_used") == on
                rad[on] = (r.view(np.uint32).tobytes(), img.tobytes(), rays)
            assert rad[1] == rad[0]


@pytest.mark.gpu
def test_on_equals_off_with_ties_and_cracks(gpu):
    """The wall in a crack of teapot's octree (test_gpu_parity.py's frame): tied
    and crack queries answered over the octree, deferred or in the main loop."""
    import octree_kat as K
    tris, bmin, bmax = oracle.load_scene(data("teapot.obj"))
    tris, ax, p = K.crack_wall_scene(tris, bmin, bmax)
    frm = p.astype(np.float64).copy()
    frm[ax] -= 3.0
    frm[(ax + 1) % 3] += 0.7
    w, h, spp = 96, 64, 16
    cam = tm.Camera.create(frm.astype(np.float32), p, [0, 1, 0] if ax != 1 else [1, 0, 0], 20.0, w / h, 0.0, 3.0)
    with tm.Scene(tris, bounds=(bmin, bmax), options={"path_waves": 5}) as sc:
        seen = 0
        for defer in (0, 1, -1):
            sc.set_option("tie_defer", defer)
            off = _on_off(sc, cam, f"crack_wall tie_defer {defer}", w, h, spp)
            seen += off[2][0] + off[2][2] + off[2][3]
        assert seen > 0  # ties, cracks or re-traced samples: the frame exercises them


@pytest.mark.gpu
def test_oracle_frame(suzanne_scene):
    """Suzanne 160x90x8 with the pre-pass: the oracle's frame under SEED_SAMPLE, byte for byte."""
    tris, (bmin, bmax) = _suzanne()
    cam = tm.Camera.for_scene(bmin, bmax, RW, RH)
    osc = oracle.Scene(tris, accel=oracle.ACCEL_OCTREE, tie=oracle.TIE_VISIT, bmin=bmin, bmax=bmax)
    ref, ref_rays = osc.render(cam.as_array(), RW, RH, 8, seed_mode=oracle.SEED_SAMPLE)
    suzanne_scene.set_option("cam_pre", 1)
    img, rays = suzanne_scene.trace_image(cam, RW, RH, 8, seed_mode=tm.SEED_SAMPLE)
    assert suzanne_scene.get_option("cam_rays_used") == 1
    assert rays == ref_rays and np.array_equal(img, ref)


@pytest.mark.gpu
def test_fallback_when_the_buffer_does_not_fit(suzanne_scene):
    """cam_pre_max one byte below the call's need: the render runs without the
    pre-pass; exactly at the need: with it; the same frame either way."""
    sc = suzanne_scene
    tris, (bmin, bmax) = _suzanne()
    cam = tm.Camera.for_scene(bmin, bmax, RW, RH)
    need = 32 * RW * RH * RSPP
    sc.set_option("cam_pre", 1)
    try:
        sc.set_option("cam_pre_max", need - 1)
        below = _render(sc, cam, RW, RH, RSPP)
        assert sc.get_option("cam_rays_used") == 0
        sc.set_option("cam_pre_max", need)
        at = _render(sc, cam, RW, RH, RSPP)
        assert sc.get_option("cam_rays_used") == 1
    finally:
        sc.set_option("cam_pre_max", 0)
    assert below == at


def test_options_are_checked():
    """cam_pre and cam_pre_max are in the option table, with their ranges
    (no GPU: the options are parsed before any device work)."""
    tris = np.zeros((1, 9), np.float32)
    for bad, msg in (("cam_pre=2", "out of range"), ("cam_pre=-2", "out of range"), ("cam_pre=0.5", "integer"),
                     ("cam_pre_max=-1", "out of range"), ("cam_rays_used=1", "unknown option")):
        with pytest.raises(tm.TmptError, match=msg):
            tm.Scene(tris, options=bad)
    if tm.device_count() == 0:
        for good in ("cam_pre=1", "cam_pre=-1, cam_pre_max=1e9", {"cam_pre": 0, "cam_pre_max": 0}):
            with pytest.raises(tm.TmptError, match="device"):
                tm.Scene(tris, options=good)
    assert "tmpt_camera_rays" in tm.EXPORTS
