"""The call-order matrix's driver and comparison, free of any GPU or library
import: tests/test_gpu_call_order.py runs them over the real call kinds
(tests/call_kinds.py), tests/test_call_order_harness.py proves them on a fake
scene whose kinds leak state on purpose.

A call kind is a function (scene, size) -> Result.  The matrix holds that B
after A on one scene returns exactly what B returns on a fresh scene.
"""
import numpy as np


class Result:
    """What one call returned, in comparable parts:
    arrays  name -> ndarray, compared as bytes
    rays    the call's ray count, or None where the call has none
    stats   name -> value: the whitelisted statistics the call writes
    route   name -> value: the route markers and read-only route options
    seen    anything else (every statistic, say), for a baseline's own
            assertions; not compared"""

    def __init__(self, arrays=None, rays=None, stats=None, route=None, seen=None):
        self.arrays = dict(arrays or {})
        self.rays = rays
        self.stats = dict(stats or {})
        self.route = dict(route or {})
        self.seen = dict(seen or {})


class Kind:
    """name; fn(scene, size) -> Result; world: the scene definition on which the
    kind takes the route it is named for (it runs on every definition);
    sample: a sample-seeded render (plays A at 1024 spp too)."""

    def __init__(self, name, fn, world="suzanne", sample=False):
        self.name, self.fn, self.world, self.sample = name, fn, world, sample
        self.__doc__ = fn.__doc__


def first_difference(a, b):
    """None if the two arrays hold the same bytes in the same shape, else a
    text naming the first record that differs (a record: the last axis of a
    plain array, one element of a structured one)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"shape / dtype {a.shape} {a.dtype} != {b.shape} {b.dtype}"
    if a.tobytes() == b.tobytes():
        return None
    plain = a.dtype.fields is None and a.ndim > 1
    lead = a.shape[:-1] if plain else a.shape
    rec = a.dtype.itemsize * (a.shape[-1] if plain else 1)
    ra = np.frombuffer(a.tobytes(), np.uint8).reshape(-1, rec)
    rb = np.frombuffer(b.tobytes(), np.uint8).reshape(-1, rec)
    bad = np.nonzero((ra != rb).any(1))[0]
    at = tuple(int(i) for i in np.unravel_index(int(bad[0]), lead)) if lead else ()
    return f"{bad.size} of {ra.shape[0]} records differ, first at {at}: {a[at]!r} != {b[at]!r}"


def compare(got, want):
    """Every part of two Results: the list of differences, each naming its part
    -- bytes (with the first differing record), rays, the named statistic, the
    named route marker.  Empty when they are equal."""
    bad = []
    if sorted(got.arrays) != sorted(want.arrays):
        bad.append(f"bytes: arrays {sorted(got.arrays)} != {sorted(want.arrays)}")
    for name in want.arrays:
        if name in got.arrays:
            d = first_difference(got.arrays[name], want.arrays[name])
            if d:
                bad.append(f"bytes of {name}: {d}")
    if got.rays != want.rays:
        bad.append(f"rays: {got.rays} != {want.rays}")
    for part, g, w in (("stat", got.stats, want.stats), ("route", got.route, want.route)):
        if sorted(g) != sorted(w):
            bad.append(f"{part}: fields {sorted(g)} != {sorted(w)}")
        for name in w:
            if name in g and g[name] != w[name]:
                bad.append(f"{part} {name}: {g[name]!r} != {w[name]!r}")
    return bad


class CallFailed(AssertionError):
    pass


def _call(kind, scene, size, history):
    history.append(f"{kind.name}{tuple(size)}")
    try:
        return kind.fn(scene, size)
    except Exception as e:  # nothing more runs on that scene: a device fault must end the test
        raise CallFailed(f"{history[-1]} raised {type(e).__name__}: {e}\n  calls so far: {' '.join(history)}") from e


def run_pairs(make_scene, kinds, a_name, a_size, b_size, baseline, a_check=None, worlds=None):
    """On one scene per scene definition (`worlds`; by default every definition a
    kind names as its own), for every kind B in table order: A at a_size, then B at
    b_size, and B's result against baseline[B name, world, b_size].  The scene is
    never rebuilt between the B's, so the histories get long; every kind plays B
    on every definition, so each A takes every route it has before each B.
    make_scene(world) -> an object with close(); kinds: name -> Kind, ordered;
    a_check(result of A, scene) -> differences (A's own result against a reference,
    where there is a cheap one), reported once each.
    -> the mismatches, each with A, a_size, B, the part that differs and the
    calls made so far on that scene.  A call that raises ends the run (CallFailed)."""
    a = kinds[a_name]
    bad = []
    if worlds is None:
        worlds = []
        for k in kinds.values():
            if k.world not in worlds:
                worlds.append(k.world)
    for world in worlds:
        scene = make_scene(world)
        history = []
        try:
            for b in kinds.values():
                first = _call(a, scene, a_size, history)
                for d in a_check(first, scene) if a_check else ():
                    if not any(x.startswith(d) for x in bad):
                        bad.append(f"{d}\n  calls so far on the {world} scene: {' '.join(history)}")
                got = _call(b, scene, b_size, history)
                for d in compare(got, baseline[b.name, world, tuple(b_size)]):
                    bad.append(f"A={a_name}{tuple(a_size)} B={b.name}{tuple(b_size)} on {world}: {d}\n"
                               f"  calls so far on the {world} scene: {' '.join(history)}")
        finally:
            scene.close()
    return bad
