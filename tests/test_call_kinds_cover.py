"""The call-order matrix's table keeps up with the scene handle: every public
method of toymeshpathtracer_amd.Scene is exercised by some kind of
tests/call_kinds.py (call_kinds.COVERS) or stands in EXEMPT with its reason, so
an entry point cannot be added without joining the matrix
(tests/test_gpu_call_order.py) or saying why not.  No GPU: introspection and
the header's text only.
"""
import inspect
import os
import re

import call_kinds as K
import toymeshpathtracer_amd as tm
from conftest import ROOT

#: public Scene methods no kind has to name, each with its reason
EXEMPT = {
    "close": "ends a handle; test_gpu_call_order.py::test_close_after_every_kind closes after every kind",
    "stats": "reads the last call's statistics; every kind reads them into its Result (call_kinds._stats)",
    "get_option": "reads an option; every kind reads the options it sets and its route markers through it",
    "set_option": "every kind sets its options through call_kinds.options(), which puts them back",
    "hit_scene": "the single-ray wrapper over hit_scene_batch, which hit_closest and hit_any_ranged cover",
    "trace_progressive": "a generator over trace_image passes; test_between_progressive_passes runs every kind "
                         "between two such passes",
    "query_keys": "a static host-only check hook (tmpt_query_keys): it takes no scene and leaves none changed",
}


def public_methods(cls):
    """The names a caller of `cls` can call: functions and static methods not starting with '_'."""
    return sorted(name for name, _ in inspect.getmembers(cls, callable) if not name.startswith("_"))


def uncovered(cls, covers=None, exempt=None):
    """-> the public methods of cls that no kind names and EXEMPT does not list."""
    covers = K.COVERS if covers is None else covers
    named = {m for methods, _ in covers.values() for m in methods}
    return [m for m in public_methods(cls) if m not in named and m not in (EXEMPT if exempt is None else exempt)]


def header_options():
    """The option names of include/tmpt.h's "Scene options" comment: the words that open an entry."""
    text = open(os.path.join(ROOT, "include", "tmpt.h")).read()
    block = text[text.index("Build options (only at creation)"):text.index("int tmpt_scene_create_ex(")]
    names = set()
    for line in block.splitlines():
        m = re.match(r" \*   ([a-z_0-9]+(?:, [a-z_0-9]+)*),?(?:  |$)", line)
        if m:
            names.update(m.group(1).split(", "))
    return names


def test_every_public_method_is_covered_or_exempt():
    assert uncovered(tm.Scene) == []


def test_the_table_and_the_cover_list_agree():
    assert list(K.COVERS) == list(K.KINDS)
    assert len(K.KINDS) == 40
    for name, (methods, options) in K.COVERS.items():
        assert methods, f"{name} names no method"
        for m in methods:
            assert callable(getattr(tm.Scene, m, None)), f"{name}: Scene has no method {m}"
        for o in options:
            assert o in header_options(), f"{name}: include/tmpt.h lists no option {o}"
    for m, reason in EXEMPT.items():
        assert callable(getattr(tm.Scene, m, None)) and reason, m
    named = {m for methods, _ in K.COVERS.values() for m in methods}
    assert not named & set(EXEMPT), named & set(EXEMPT)


def test_header_options_are_found():
    """The parse that the option check rests on: entries that open a line alone, in a list, and
    read-only ones."""
    found = header_options()
    for o in ("sample_base", "query_sort", "query_sorted", "octree_build", "path_waves", "path_waves_used", "update_kind",
              "rowspec_stream", "help", "pair", "denoise_lds", "builder"):
        assert o in found, o
    assert "no_such_option" not in found


def test_a_new_entry_point_is_named():
    """The guard itself: a Scene with one more public method fails the check, by that method's name."""
    class Wider(tm.Scene):
        def trace_something_new(self):
            pass

        def _private(self):
            pass

    assert uncovered(Wider) == ["trace_something_new"]
    assert uncovered(tm.Scene, covers={k: v for k, v in K.COVERS.items() if k != "sample_plan"}) == ["sample_plan"]
    assert "hit_scene" in uncovered(tm.Scene, exempt={})
