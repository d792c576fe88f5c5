"""The radiance render's and the denoiser's surface without a GPU: the two
entry points, tmpt_denoise_desc against its ctypes mirror, the descriptor's
range checks (they run before anything that needs a scene or a device), the
denoise_lds option's parsing, the Python methods, the CLI's usage line."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import toymeshpathtracer_amd as tm
from conftest import ROOT

FIELDS = ("width", "height", "spp", "levels", "normal_exp", "flags", "sigma_depth", "sigma_direct", "wait_stream",
          "reserved")


def test_entry_points_are_declared_and_exported():
    lib = ctypes.CDLL(tm.lib_path)
    out = subprocess.run(["nm", "-D", "--defined-only", tm.lib_path], capture_output=True, text=True).stdout
    for name in ("tmpt_render_radiance", "tmpt_denoise"):
        assert name in tm.EXPORTS
        assert hasattr(lib, name)
        assert re.search(rf" T {name}$", out, flags=re.M)
    assert tm.abi_version() == 9  # additive: detected by symbol, the version stays
    assert callable(tm.Scene.trace_radiance) and callable(tm.Scene.denoise)


def test_desc_layout_matches_the_ctypes_mirror(tmp_path):
    src = tmp_path / "d.c"
    offs = ", ".join(f"offsetof(tmpt_denoise_desc, {f})" for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tmpt.h"\n'
                   'int main(void){ printf("%zu' + ' %zu' * len(FIELDS) + '\\n", sizeof(tmpt_denoise_desc), '
                   + offs + '); return 0; }\n')
    exe = tmp_path / "d"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()))
    d = tm._DenoiseDesc
    assert got[0] == ctypes.sizeof(d) == 56
    assert tuple(f for f, _ in d._fields_) == FIELDS
    assert got[1:] == [getattr(d, f).offset for f in FIELDS]
    assert got[1:] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40]


def _desc(**kw):
    d = tm._DenoiseDesc()
    d.width, d.height, d.spp, d.normal_exp = 8, 4, 4, -1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(d, f32=True, u8=True):
    """tmpt_denoise without a scene: a descriptor that passes its checks ends
    at the null scene, one that does not is refused by name before that."""
    rad = np.zeros((4, 8, 4), np.float32)
    aov = np.zeros((4, 8), tm.AOV_DTYPE)
    img = np.zeros((4, 8, 4), np.uint8)
    rc = tm._denoise(None, ctypes.byref(d), rad.ctypes.data_as(ctypes.c_void_p), aov.ctypes.data_as(ctypes.c_void_p),
                     rad.ctypes.data_as(ctypes.c_void_p) if f32 else None,
                     img.ctypes.data_as(ctypes.c_void_p) if u8 else None)
    return rc, tm._last_error().decode()


@pytest.mark.parametrize("kw,msg", [(dict(levels=7), "levels"), (dict(levels=-1), "levels"),
                                    (dict(normal_exp=9), "normal_exp"), (dict(normal_exp=-2), "normal_exp"),
                                    (dict(sigma_depth=-1.0), "sigma_depth"), (dict(sigma_direct=-0.5), "sigma_direct"),
                                    (dict(sigma_depth=float("inf")), "sigma_depth"),
                                    (dict(sigma_direct=float("nan")), "sigma_direct"),
                                    (dict(width=0), "width"), (dict(height=10001), "height"),
                                    (dict(spp=0), "samplesPerPixel"), (dict(flags=2), "flag")])
def test_descriptor_ranges_are_checked_before_any_device_work(kw, msg):
    rc, err = _call(_desc(**kw))
    assert rc == -22 and msg in err, (rc, err)


def test_outputs_and_pointers_are_checked():
    rc, err = _call(_desc(), f32=False, u8=False)
    assert rc == -22 and "no output" in err, (rc, err)
    for good in (_desc(), _desc(levels=6, normal_exp=8, sigma_depth=0.5, sigma_direct=2.0), _desc(levels=1, normal_exp=0)):
        rc, err = _call(good)  # every value in range: the call gets as far as the missing scene
        assert rc == -22 and "null argument" in err, (rc, err)
    rc, err = (tm._denoise(None, None, None, None, None, None), tm._last_error().decode())
    assert rc == -22 and "descriptor" in err, (rc, err)


def test_radiance_null_arguments():
    d = tm._desc(8, 4, 2, tm.SEED_SAMPLE)
    rays = ctypes.c_uint64()
    rc = tm._render_radiance(None, None, ctypes.byref(d), None, None, ctypes.byref(rays))
    assert rc == -22 and "tmpt_render_radiance" in tm._last_error().decode()


def test_denoise_lds_option_is_parsed_before_any_device_work():
    tris = np.zeros((1, 9), np.float32)
    for bad in ("denoise_lds=2", "denoise_lds=-2"):
        with pytest.raises(tm.TmptError, match="out of range"):
            tm.Scene(tris, options=bad)
    with pytest.raises(tm.TmptError, match="integer"):
        tm.Scene(tris, options="denoise_lds=0.5")


def test_cli_usage_mentions_denoise():
    cli = os.path.join(os.path.dirname(tm.lib_path), "tmpt")
    r = subprocess.run([cli], capture_output=True, text=True)
    assert r.returncode == 1 and "Usage" in r.stdout and "--denoise" in r.stdout
