"""Device-resident queries without a GPU: the entry points are declared and
exported with the ABI version kept, the Python mirror of tmpt_hit_desc has the
declared layout, tmpt_scene_hit_device refuses a null scene before any device
call, the new options are documented beside the others, and
Scene.hit_scene_device's argument errors that need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import toymeshpathtracer_amd as tm
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "tmpt.h")
NEW = ("tmpt_scene_hit_device", "tmpt_query_keys", "tmpt_query_plan")
OPTIONS = ("query_sort", "query_top", "query_max", "query_chunk", "query_grid", "query_ms", "query_sort_ms",
           "query_chunks", "query_sorted")


def test_header_declares_and_the_library_exports():
    text = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", tm.lib_path], capture_output=True, text=True).stdout
    for name in NEW:
        assert name in tm.EXPORTS and hasattr(tm._lib, name)
        assert f"int {name}(" in text
        assert re.search(rf" T {name}$", out, flags=re.M)
    assert tm.abi_version() == 9  # additive: detected by symbol, the version stays
    assert "#define TMPT_ABI_VERSION 9 " in text
    assert callable(tm.Scene.hit_scene_device) and callable(tm.query_keys)
    for opt in OPTIONS:  # documented beside the others
        assert re.search(rf"^ \*   (\w+, )*{opt}\b", text, flags=re.M), opt
    # the older calls keep their signatures
    assert "int tmpt_scene_hit(const tmpt_scene* scene, const float* rays, int64_t n, float tmin, float tmax," in text
    assert "int tmpt_scene_hit_ranged(const tmpt_scene* scene, const float* rays8, int64_t n, int32_t any_hit," in text


def test_hit_desc_layout():
    d = tm._HitDesc
    assert ctypes.sizeof(d) == 56
    want = dict(n=0, ranged=8, any_hit=12, tmin=16, tmax=20, flags=24, reserved0=28, wait_stream=32, reserved=40)
    assert {f: getattr(d, f).offset for f, _ in d._fields_} == want
    # and the header's struct, field for field
    text = open(HEADER).read()
    body = text[text.index("typedef struct {\n    int64_t  n;"):text.index("} tmpt_hit_desc;")]
    names = re.findall(r"^\s+\w+\s+([\w, ]+?)(?:\[\d+\])?;", body, flags=re.M)
    flat = [n.strip() for group in names for n in group.split(",")]
    assert flat == [f for f, _ in d._fields_], flat


def _fn():
    return tm._sig("tmpt_scene_hit_device", ctypes.c_int, [ctypes.c_void_p] * 6)


def test_null_scene_is_refused_before_any_device_call():
    d = tm._HitDesc()
    d.n = 4
    rc = _fn()(None, ctypes.byref(d), 0x1000, 0x2000, None, None)
    assert rc == -22 and "tmpt_scene_hit_device: null scene" in tm._last_error().decode()
    rc = _fn()(None, None, None, None, None, None)  # the scene comes first
    assert rc == -22 and "tmpt_scene_hit_device: null scene" in tm._last_error().decode()


def test_python_refuses_what_is_not_a_device_tensor():
    sc = tm.Scene.__new__(tm.Scene)  # no device: the checks below come before any call into the library
    sc._h, sc.device = None, 0
    if tm.torch is None:
        with pytest.raises(tm.TmptError, match="needs torch"):
            sc.hit_scene_device(np.zeros((4, 6), np.float32), 0.0, 1.0)
        return
    torch = tm.torch
    with pytest.raises(ValueError, match="torch tensor"):
        sc.hit_scene_device(np.zeros((4, 6), np.float32), 0.0, 1.0)
    with pytest.raises(ValueError, match="is on cpu"):
        sc.hit_scene_device(torch.zeros((4, 6)), 0.0, 1.0)
    with pytest.raises(ValueError, match="both t_min and t_max"):
        sc.hit_scene_device(torch.zeros((4, 6)), 0.0)
