"""The call-order matrix's driver and comparison (tests/call_order.py) proved on
a fake scene in pure Python whose kinds keep state between calls on purpose --
as tests/test_bvh_check.py proves bvh_check by mutations: the driver reports
exactly the guilty (A, B) pairs, with the history and the part that differs, and
passes the clean ones; the comparison notices one flipped bit, a ray count off
by one, a changed statistic and a changed route marker.  No GPU.
"""
import numpy as np
import pytest

from call_order import CallFailed, Kind, Result, compare, first_difference, run_pairs

BASE, BIG, TINY = (5, 3, 2), (9, 4, 2), (2, 1, 2)


class FakeScene:
    """What struct Scene keeps, in small: a grow-only buffer, a mode word, the
    last call's statistic."""

    def __init__(self, world="fake"):
        self.world = world
        self.buf = np.zeros(0, np.uint8)
        self.mode = 0
        self.last_rays = 0
        self.closed = False

    def close(self):
        self.closed = True


def _frame(size, salt):
    w, h, spp = size
    return ((np.arange(w * h * 4, dtype=np.uint32) * 7 + salt + spp) % 251).astype(np.uint8).reshape(h, w, 4)


def stat_stale(scene, size):
    """Reports the statistic the call before it left: it never writes its own."""
    return Result({"image": _frame(size, 1)}, 10, {"extend_rays": scene.last_rays}, {"engine": 1})


def grow(scene, size):
    """A grow-only buffer with a stale tail: the call fills its own n bytes but
    sums the whole buffer, so what a larger frame left behind shows."""
    n = size[0] * size[1]
    if scene.buf.size < n:
        scene.buf = np.zeros(n, np.uint8)
    scene.buf[:n] = 1 + np.arange(n) % 5
    img = _frame(size, 2)
    img[0, 0, 0] = scene.buf.sum() % 256  # the bug: buf[:n] was meant
    scene.last_rays = rays = int(np.count_nonzero(scene.buf))  # and here
    return Result({"image": img}, rays, {"extend_rays": rays}, {"engine": 2})


def mode_leak(scene, size):
    """Chooses its route by a mode word, sets the word and never puts it back."""
    route = scene.mode
    scene.mode = 1
    scene.last_rays = 30
    return Result({"image": _frame(size, 3)}, 30, {"extend_rays": 30}, {"engine": 3 + route})


def clean(scene, size):
    """A function of its arguments alone."""
    scene.last_rays = 40
    return Result({"image": _frame(size, 4)}, 40, {"extend_rays": 40}, {"engine": 5})


# stat_stale first: as B it then follows A alone, not a long history
KINDS = {k.name: k for k in (Kind("stat_stale", stat_stale, world="fake"), Kind("grow", grow, world="fake"),
                             Kind("mode_leak", mode_leak, world="fake"), Kind("clean", clean, world="fake"))}


def _baseline():
    return {(name, world, BASE): k.fn(FakeScene(world), BASE) for name, k in KINDS.items() for world in ("fake", "tied")}


def _run(a, a_size, kinds=KINDS, **kw):
    scenes = []

    def make(world):
        assert world == "fake"
        scenes.append(FakeScene(world))
        return scenes[-1]

    bad = run_pairs(make, kinds, a, a_size, BASE, _baseline(), **kw)
    assert len(scenes) == 1 and scenes[0].closed  # one scene per scene definition, closed at the end
    return bad


def _pairs(bad):
    """{(A, B): the parts reported} out of the driver's texts."""
    out = {}
    for text in bad:
        head, what = text.split(": ", 1)
        a, b = head.split(" B=")
        out.setdefault((a[2:].split("(")[0], b.split("(")[0]), []).append(what.split(":")[0].split(" ")[0])
    return out


def test_the_driver_reports_exactly_the_guilty_pairs():
    found = {}
    for a in KINDS:
        for size in (BIG, TINY):
            for pair, parts in _pairs(_run(a, size)).items():
                found[pair + (size,)] = sorted(parts)
    assert found == {
        # the stale tail shows only after a larger frame of the same kind
        ("grow", "grow", BIG): ["bytes", "rays", "stat"],
        # the mode word its own earlier call left
        ("mode_leak", "mode_leak", BIG): ["route"], ("mode_leak", "mode_leak", TINY): ["route"],
        # the stale statistic, after every kind that writes one
        ("grow", "stat_stale", BIG): ["stat"], ("grow", "stat_stale", TINY): ["stat"],
        ("mode_leak", "stat_stale", BIG): ["stat"], ("mode_leak", "stat_stale", TINY): ["stat"],
        ("clean", "stat_stale", BIG): ["stat"], ("clean", "stat_stale", TINY): ["stat"],
    }


def test_a_report_names_the_pair_the_part_and_the_history():
    bad = _run("grow", BIG)
    text = next(t for t in bad if "B=grow" in t and "bytes" in t)
    assert text.startswith("A=grow(9, 4, 2) B=grow(5, 3, 2) on fake: bytes of image: 1 of 15 records differ, first at (0, 0)")
    assert text.endswith("calls so far on the fake scene: grow(9, 4, 2) stat_stale(5, 3, 2) grow(9, 4, 2) grow(5, 3, 2)")
    rays = next(t for t in bad if "B=grow" in t and "rays" in t)
    assert "rays: 36 != 15" in rays
    stat = next(t for t in _run("clean", TINY))
    assert "B=stat_stale(5, 3, 2) on fake: stat extend_rays: 40 != 0" in stat and "clean(2, 1, 2) stat_stale(5, 3, 2)" in stat
    route = next(t for t in _run("mode_leak", BIG) if "B=mode_leak" in t)
    assert "route engine: 4 != 3" in route


def test_clean_kinds_pass():
    only = {"clean": KINDS["clean"]}
    assert _run("clean", BIG, kinds=only) == [] and _run("clean", TINY, kinds=only) == []
    assert _run("stat_stale", BIG) == [] and _run("stat_stale", TINY) == []


def route_by_world(scene, size):
    """Takes a route of its own on the `tied` definition, as the split and deferring
    renders do, and only there leaves a queue unreset for the next call of its kind."""
    n = 7
    if scene.world == "tied":
        n += scene.mode
        scene.mode = 2
    scene.last_rays = n
    return Result({"image": _frame(size, 5)}, n, {"extend_rays": n}, {"engine": 6 if scene.world == "tied" else 5})


def test_every_kind_runs_on_every_scene_definition():
    """A kind whose own definition is another one still plays A and B on every
    definition: its route there is taken before each B, and a leak that only that
    route has is reported, on that definition alone."""
    kinds = dict(KINDS, route_by_world=Kind("route_by_world", route_by_world, world="tied"))
    scenes = []

    def make(world):
        scenes.append(FakeScene(world))
        return scenes[-1]

    base = _baseline()
    for world in ("fake", "tied"):
        base["route_by_world", world, BASE] = route_by_world(FakeScene(world), BASE)
    bad = run_pairs(make, kinds, "route_by_world", BIG, BASE, base)
    assert [sc.world for sc in scenes] == ["fake", "tied"] and all(sc.closed for sc in scenes)
    own = [t for t in bad if "B=route_by_world" in t]
    assert len(own) == 2 and all(" on tied: " in t for t in own)  # rays and the statistic
    assert "rays: 9 != 7" in own[0] and "calls so far on the tied scene: route_by_world(9, 4, 2) stat_stale" in own[0]
    # mode_leak reads the same word: after route_by_world on `tied` its route flips too (mode 2)
    assert any("B=mode_leak(5, 3, 2) on tied: route engine: 5 != 3" in t for t in bad)
    assert not any(" on fake: " in t and "B=route_by_world" in t for t in bad)
    # worlds= narrows the run
    scenes.clear()
    run_pairs(make, kinds, "clean", BIG, BASE, base, worlds=["tied"])
    assert [sc.world for sc in scenes] == ["tied"]


def test_the_check_of_a_runs_on_every_call_of_a_and_reports_once():
    seen = []

    def a_check(res, scene):
        seen.append(res.rays)
        return ["clean(9, 4, 2): its frame is not the reference's"]

    bad = _run("clean", BIG, kinds={"clean": KINDS["clean"], "mode_leak": KINDS["mode_leak"]}, a_check=a_check)
    assert seen == [40, 40] and len(bad) == 1 and bad[0].startswith("clean(9, 4, 2): its frame") and "calls so far" in bad[0]


def test_a_call_that_raises_ends_the_run_with_its_history():
    def boom(scene, size):
        raise RuntimeError("device lost")

    kinds = dict(KINDS, boom=Kind("boom", boom, world="fake"))
    with pytest.raises(CallFailed, match=r"boom\(5, 3, 2\) raised RuntimeError: device lost\n.*clean\(9, 4, 2\) boom"):
        _run("clean", BIG, kinds=kinds)


def _result():
    rec = np.zeros((3, 2), np.dtype([("t", np.float32), ("id", np.int32)]))
    rec["t"] = np.arange(6, dtype=np.float32).reshape(3, 2)
    return Result({"image": _frame(BASE, 0), "radiance": np.linspace(0, 1, 60, dtype=np.float32).reshape(3, 5, 4),
                   "records": rec}, 1234, {"extend_rays": 1000, "tie_path": 1, "pass_pixels": (15, 7)},
                  {"cam_rays_used": 1, "shadow_split_used": 3, "msg": "refused"}, {"render_ms": 0.5})


def test_compare_equal_results():
    a, b = _result(), _result()
    b.seen["render_ms"] = 9.0  # not compared
    assert compare(a, b) == []
    assert first_difference(a.arrays["records"], b.arrays["records"]) is None


def test_compare_notices_one_flipped_bit():
    a, b = _result(), _result()
    b.arrays["radiance"].view(np.uint32)[2, 3, 1] ^= 1  # the last mantissa bit of one float
    assert a.arrays["radiance"][2, 3, 1] != b.arrays["radiance"][2, 3, 1]
    bad = compare(b, a)
    assert len(bad) == 1 and bad[0].startswith("bytes of radiance: 1 of 15 records differ, first at (2, 3)")
    a, b = _result(), _result()
    b.arrays["image"][1, 4, 2] ^= 0x80
    assert [t.split(",")[0] for t in compare(b, a)] == ["bytes of image: 1 of 15 records differ"]
    assert "first at (1, 4)" in compare(b, a)[0]
    a, b = _result(), _result()
    b.arrays["records"]["id"][2, 1] = 1  # a structured record: one element is the record
    assert "bytes of records: 1 of 6 records differ, first at (2, 1)" in compare(b, a)[0]
    # -0.0 against 0.0: equal as numbers, not as bytes
    a, b = _result(), _result()
    b.arrays["radiance"][0, 0, 0] = -0.0
    assert a.arrays["radiance"][0, 0, 0] == b.arrays["radiance"][0, 0, 0] and len(compare(b, a)) == 1


def test_compare_notices_shape_dtype_and_missing_arrays():
    a, b = _result(), _result()
    b.arrays["image"] = b.arrays["image"].reshape(5, 3, 4)
    assert "shape / dtype" in compare(b, a)[0]
    b = _result()
    del b.arrays["radiance"]
    assert compare(b, a)[0].startswith("bytes: arrays")
    b = _result()
    b.arrays["extra"] = np.zeros(1)
    assert compare(b, a)[0].startswith("bytes: arrays")


def test_compare_notices_rays_stats_and_route_markers():
    a = _result()
    b = _result()
    b.rays += 1
    assert compare(b, a) == ["rays: 1235 != 1234"]
    b = _result()
    b.rays = None
    assert compare(b, a) == ["rays: None != 1234"]
    b = _result()
    b.stats["tie_path"] = 2
    assert compare(b, a) == ["stat tie_path: 2 != 1"]
    b = _result()
    b.stats["pass_pixels"] = (15, 8)
    assert compare(b, a) == ["stat pass_pixels: (15, 8) != (15, 7)"]
    b = _result()
    del b.stats["extend_rays"]
    assert compare(b, a)[0].startswith("stat: fields")
    b = _result()
    b.route["shadow_split_used"] = 0
    assert compare(b, a) == ["route shadow_split_used: 0 != 3"]
    b = _result()
    b.route["msg"] = "accepted"
    assert compare(b, a) == ["route msg: 'accepted' != 'refused'"]
