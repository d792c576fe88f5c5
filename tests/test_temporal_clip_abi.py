"""History clipping's surface without a GPU: the entry point,
tmpt_temporal_clip_desc against its mirror, every argument check in the header's
order (none needs a scene: the scene is the last thing the call looks at), the
Python method's own argument errors, the CLI's usage."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import temporal_clip_restate as K
import toymeshpathtracer_amd as tm
from conftest import ROOT

DESC_FIELDS = ("width", "height", "flags", "n_max", "sigma_depth", "gamma", "radius", "reserved0", "wait_stream",
               "reserved")
# the call's pointers, in its order
PTRS = ("cur", "stat", "mot", "pmot", "hist", "aux", "aux_hist", "aux_out", "f32", "u8")


def _fn():
    return tm._sig("tmpt_temporal_clip", ctypes.c_int, [ctypes.c_void_p] * 12)


def test_entry_point_is_declared_and_exported():
    lib = ctypes.CDLL(tm.lib_path)
    out = subprocess.run(["nm", "-D", "--defined-only", tm.lib_path], capture_output=True, text=True).stdout
    assert "tmpt_temporal_clip" in tm.EXPORTS and hasattr(lib, "tmpt_temporal_clip")
    assert re.search(r" T tmpt_temporal_clip$", out, flags=re.M)
    assert tm.abi_version() == 9  # additive: detected by symbol, the version stays
    assert callable(tm.Scene.temporal_clip)


def test_layout_matches_the_mirror(tmp_path):
    src = tmp_path / "d.c"
    offs = ", ".join(f"offsetof(tmpt_temporal_clip_desc, {f})" for f in DESC_FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tmpt.h"\n'
                   'int main(void){ printf("%zu' + ' %zu' * len(DESC_FIELDS) + '\\n", sizeof(tmpt_temporal_clip_desc), '
                   + offs + '); return 0; }\n')
    exe = tmp_path / "d"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()))
    d = tm._TemporalClipDesc
    assert got[0] == ctypes.sizeof(d) == 56
    assert tuple(f for f, _ in d._fields_) == DESC_FIELDS
    assert got[1:] == [getattr(d, f).offset for f in DESC_FIELDS] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40]


def _desc(**kw):
    d = tm._TemporalClipDesc()
    d.width, d.height = 8, 4
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(d, ptrs=None, **given):
    """The call without a scene.  Host frames of 8 x 4 by default: cur, mot, pmot,
    hist and both outputs given, stat and the aux triple not; given[name] = True /
    False adds or removes one; ptrs = {name: address} sets raw addresses."""
    frame = lambda: np.zeros((4, 8, 4), np.float32)
    bufs = dict(cur=frame(), stat=frame(), mot=np.zeros((4, 8), tm.MOTION_DTYPE), pmot=np.zeros((4, 8), tm.MOTION_DTYPE),
                hist=frame(), aux=frame(), aux_hist=frame(), aux_out=frame(), f32=frame(), u8=np.zeros((4, 8, 4), np.uint8))
    on = dict(cur=True, stat=False, mot=True, pmot=True, hist=True, aux=False, aux_hist=False, aux_out=False, f32=True,
              u8=True)
    on.update(given)
    a = [bufs[k].ctypes.data if on[k] else None for k in PTRS]
    for k, v in (ptrs or {}).items():
        a[PTRS.index(k)] = v
    rc = _fn()(None, ctypes.byref(d) if d is not None else None, *a)
    return rc, tm._last_error().decode()


def test_checks_in_order():
    rc, err = _call(None)
    assert rc == -22 and "tmpt_temporal_clip: null descriptor" in err, (rc, err)
    inf, nan = float("inf"), float("nan")
    dev = tm.FLAG_OUT_DEVICE
    steps = [
        (dict(d=_desc(width=0)), "width"), (dict(d=_desc(width=10001)), "width"),
        (dict(d=_desc(height=0)), "height"), (dict(d=_desc(height=10001)), "height"),
        (dict(cur=False), "null argument"), (dict(mot=False), "null argument"), (dict(pmot=False), "null argument"),
        (dict(hist=False), "null argument"),
        (dict(aux=True), "all three or none"), (dict(aux_hist=True), "all three or none"),
        (dict(aux_out=True), "all three or none"), (dict(aux=True, aux_hist=True), "all three or none"),
        (dict(aux=True, aux_out=True), "all three or none"), (dict(aux_hist=True, aux_out=True), "all three or none"),
        (dict(f32=False, u8=False), "no output"),
        (dict(f32=False, u8=False, aux=True, aux_hist=True, aux_out=True), "no output"),
        (dict(d=_desc(n_max=0.5)), "n_max"), (dict(d=_desc(n_max=-1.0)), "n_max"), (dict(d=_desc(n_max=inf)), "n_max"),
        (dict(d=_desc(n_max=nan)), "n_max"),
        (dict(d=_desc(sigma_depth=-0.1)), "sigma_depth"), (dict(d=_desc(sigma_depth=inf)), "sigma_depth"),
        (dict(d=_desc(sigma_depth=nan)), "sigma_depth"),
        (dict(d=_desc(gamma=-0.5)), "gamma"), (dict(d=_desc(gamma=inf)), "gamma"), (dict(d=_desc(gamma=nan)), "gamma"),
        (dict(d=_desc(radius=-1)), "radius"), (dict(d=_desc(radius=4)), "radius"),
        (dict(d=_desc(flags=2)), "flag"), (dict(d=_desc(flags=8)), "flag"),
    ]
    for kw, msg in steps:
        kw = dict(kw)
        rc, err = _call(kw.pop("d", _desc()), **kw)
        assert rc == -22 and "tmpt_temporal_clip: " in err and msg in err, (msg, rc, err)
    # each device pointer's alignment (rgba8_out: 4 bytes)
    al = {k: 0x10000 * (i + 1) for i, k in enumerate(PTRS)}
    for k in PTRS:
        p = dict(al)
        p[k] += 2 if k == "u8" else 8
        rc, err = _call(_desc(flags=dev), ptrs=p)
        assert rc == -22 and "aligned" in err, (k, rc, err)
    # overlaps, host and device form: either output on any frame whose neighbours are read, by one pixel
    n = 8 * 4 * 16
    for out in ("f32", "aux_out"):
        for frame in ("hist", "aux_hist", "cur", "stat"):
            for a, b in ((0x4000, 0x4000), (0x4000, 0x4000 + n - 16), (0x4000 + n - 16, 0x4000)):
                p = dict(al)
                p[frame], p[out] = a, b
                for flags in (dev, 0):
                    rc, err = _call(_desc(flags=flags), ptrs=p)
                    assert rc == -22 and "overlaps" in err and frame.replace("hist", "history") in err, (out, frame, rc, err)
    # order between the groups: size < pointer < n_max < sigma_depth < gamma < radius < flag < alignment < overlap < scene
    chain = [(dict(width=0), "width"), (None, "null argument"), (dict(n_max=0.25), "n_max"),
             (dict(sigma_depth=-1.0), "sigma_depth"), (dict(gamma=-1.0), "gamma"), (dict(radius=7), "radius"),
             (dict(flags=dev | 2), "flag")]
    for i, (_, msg) in enumerate(chain):
        fields = {}
        for kw, _ in chain[i:]:
            fields.update(kw or {})
        rc, err = _call(_desc(**fields), cur=i > 1)
        assert rc == -22 and msg in err, (i, msg, rc, err)
    rc, err = _call(_desc(), aux=True, f32=False, u8=False)  # the aux triple with the missing pointers, before "no output"
    assert rc == -22 and "all three or none" in err
    p = dict(al, cur=0x10008, f32=al["hist"])  # misaligned and overlapping
    rc, err = _call(_desc(flags=dev), ptrs=p)
    assert rc == -22 and "aligned" in err, (rc, err)
    # everything in range: as far as the missing scene
    for d, kw in ((_desc(), {}), (_desc(n_max=1.0, sigma_depth=3.0, gamma=3e38, radius=3), dict(u8=False)),
                  (_desc(n_max=500.0, gamma=0.5, radius=1), dict(f32=False)), (_desc(radius=2), dict(stat=True)),
                  (_desc(), dict(aux=True, aux_hist=True, aux_out=True, stat=True)),
                  (_desc(flags=dev | tm.FLAG_WAIT_STREAM), dict(ptrs=al)),
                  (_desc(flags=dev), dict(ptrs=dict(al, aux_out=al["aux"]))),  # aux_out may be aux_cur
                  (_desc(flags=dev), dict(ptrs=dict(al, f32=al["hist"] + n, stat=None, aux=None, aux_hist=None, aux_out=None)))):
        rc, err = _call(d, **kw)
        assert rc == -22 and "null scene" in err, (kw, rc, err)


def test_python_argument_errors():
    sc = tm.Scene.__new__(tm.Scene)  # no device: the checks below come before any call into the library
    sc._h, sc.device = None, 0
    rad, mot = np.zeros((4, 8, 4), np.float32), np.zeros((4, 8), tm.MOTION_DTYPE)
    with pytest.raises(ValueError, match="go together"):
        sc.temporal_clip(rad, mot, mot, rad, aux=rad)
    with pytest.raises(ValueError, match="go together"):
        sc.temporal_clip(rad, mot, mot, rad, aux_history=rad)
    with pytest.raises(ValueError, match="width, height and out"):
        sc.temporal_clip(0x1000, 0x2000, 0x3000, 0x4000)
    with pytest.raises(ValueError, match="width, height and out"):
        sc.temporal_clip(0x1000, 0x2000, 0x3000, 0x4000, width=8, height=4)
    for bad in (dict(history=rad[:2]), dict(motion=mot[:, :3]), dict(stat=rad[:, :5]), dict(aux=rad[1:], aux_history=rad),
                dict(aux=rad, aux_history=rad[..., :3])):
        a = dict(radiance=rad, motion=mot, prev_motion=mot, history=rad)
        a.update(bad)
        with pytest.raises(ValueError, match="one whole frame"):
            sc.temporal_clip(**a)
    for out in (np.zeros((4, 8, 4), np.float64), np.zeros((4, 8, 3), np.float32), np.zeros((8, 8, 4), np.float32)[::2], [1]):
        with pytest.raises(ValueError, match="out must be"):
            sc.temporal_clip(rad, mot, mot, rad, out=out)
    # the library's own refusals come through as TmptError, before any device work
    for kw, msg in ((dict(gamma=-1.0), "gamma"), (dict(radius=4), "radius"), (dict(n_max=0.5), "n_max"),
                    (dict(out=rad), "overlaps rgba32f_cur"), (dict(stat=np.zeros_like(rad), aux=rad, aux_history=rad), "null scene")):
        with pytest.raises(tm.TmptError, match=msg):
            sc.temporal_clip(rad, mot, mot, np.zeros_like(rad), **kw)


def test_the_restatement_names_the_library_defaults():
    """tmpt_temporal_clip_desc's zeros, as the header words them, are the restatement's constants."""
    text = open(os.path.join(ROOT, "include", "tmpt.h")).read()
    m = re.search(r"Defaults n_max = ([0-9.]+), gamma = ([0-9.]+), radius = ([0-9]+):", text)
    assert m, "the header states the defaults"
    assert (float(m.group(1)), float(m.group(2)), int(m.group(3))) == (float(K.N_MAX_DEFAULT), float(K.GAMMA_DEFAULT),
                                                                       K.RADIUS_DEFAULT)


def test_cli_usage_mentions_clip():
    cli = os.path.join(os.path.dirname(tm.lib_path), "tmpt")
    r = subprocess.run([cli], capture_output=True, text=True)
    assert r.returncode == 1 and "Usage" in r.stdout and "--clip" in r.stdout
    obj = os.path.join(ROOT, "data", "cube.obj")
    for extra in (["--clip"], ["--clip", "1.5,2"], ["--twist", "10,2", "--clip", "1,1,8"], ["--twist", "10,2", "--clip"]):
        r = subprocess.run([cli, "8", "4", "1", obj, "--seed", "sample"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--clip needs --temporal" in r.stdout, (extra, r.stdout)
    r = subprocess.run([cli, "8", "4", "1", obj, "--seed", "sample", "--twist", "10,2", "--temporal", "--clip", "x"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "invalid --clip argument" in r.stdout, r.stdout
