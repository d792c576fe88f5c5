"""The C-ABI library loads and exports every symbol include/tmpt.h declares
(no GPU needed: nothing here launches a kernel)."""
import ctypes
import os
import re
import subprocess

import pytest

import toymeshpathtracer_amd as tm
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "tmpt.h")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(tmpt_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_expected_surface():
    names = declared_functions()
    assert set(names) == set(tm.EXPORTS), set(names) ^ set(tm.EXPORTS)


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(tm.lib_path)
    missing = [n for n in declared_functions() if not hasattr(lib, n)]
    assert not missing, missing
    out = subprocess.run(["nm", "-D", "--defined-only", tm.lib_path], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (tmpt_[a-z0-9_]+)$", out, flags=re.M))
    assert set(declared_functions()) <= exported


def test_no_oracle_or_torch_in_the_product_library():
    """The product links HIP only: never the oracle (test infrastructure)."""
    # resolve the library's own dependencies, not whatever a torch import left
    # on LD_LIBRARY_PATH (torch/lib holds a libamdhip64 of the same soname)
    env = {k: v for k, v in os.environ.items() if k != "LD_LIBRARY_PATH"}
    out = subprocess.run(["ldd", tm.lib_path], capture_output=True, text=True, env=env).stdout
    # library names and paths only (the load addresses are random hex: "c10" occurs in them)
    libs = " ".join(re.findall(r"(\S+\.so[.0-9]*)", out))
    assert "oracle" not in libs and "torch" not in libs and "c10" not in libs, out
    syms = subprocess.run(["nm", "-D", tm.lib_path], capture_output=True, text=True).stdout
    assert "orc_" not in syms


def test_abi_version_and_error_channel():
    assert tm.abi_version() == 9
    with pytest.raises(tm.TmptError) as e:
        tm.load_scene("/definitely/missing.obj")
    assert "missing.obj" in str(e.value)


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "tmpt.h"\nint main(void){ tmpt_render_desc d; tmpt_stats s; (void)d; (void)s;'
                   ' return tmpt_abi_version() == TMPT_ABI_VERSION ? 0 : 1; }\n')
    exe = tmp_path / "t"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                        "-o", str(exe), tm.lib_path, f"-Wl,-rpath,{os.path.dirname(tm.lib_path)}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0


def test_struct_layouts_match_ctypes(tmp_path):
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tmpt.h"\n'
                   'int main(void){ printf("%zu %zu %zu %zu\\n", sizeof(tmpt_camera), sizeof(tmpt_render_desc),'
                   ' sizeof(tmpt_stats), offsetof(tmpt_stats, build_ms)); printf("%zu %zu\\n", offsetof(tmpt_render_desc, spp_begin), offsetof(tmpt_render_desc, wait_stream));'
                   ' return 0; }\n')
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()
    want = [ctypes.sizeof(tm._Camera), ctypes.sizeof(tm._Desc), ctypes.sizeof(tm._Stats),
            tm._Stats.build_ms.offset, tm._Desc.spp_begin.offset, tm._Desc.wait_stream.offset]
    assert list(map(int, got)) == want


def test_cli_usage_without_gpu():
    cli = os.path.join(os.path.dirname(tm.lib_path), "tmpt")
    r = subprocess.run([cli], capture_output=True, text=True)
    assert r.returncode == 1 and "Usage" in r.stdout
    r = subprocess.run([cli, "0", "10", "1", "x.obj"], capture_output=True, text=True)
    assert r.returncode == 1 and "invalid width" in r.stdout
    r = subprocess.run([cli, "10", "10", "2000", "x.obj"], capture_output=True, text=True)
    assert r.returncode == 1 and "invalid samplesPerPixel" in r.stdout


def test_product_library_reads_no_environment_knobs():
    """The library's control plane is the per-scene options API (tmpt.h "Scene
    options"); in the product build only the host's OBJ / PNG thread counts
    come from the environment (the diagnostic TMPT_DIAG build adds traces, the
    checked TMPT_CHECK build its self-test switch)."""
    csrc = os.path.join(ROOT, "toymeshpathtracer_amd", "csrc")
    names = set()
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".cpp", ".h")):
            text = open(os.path.join(csrc, f)).read()
            text = re.sub(r"#ifdef TMPT_(DIAG|CHECK)\b.*?#endif", "", text, flags=re.S)
            names |= set(re.findall(r'getenv\("([A-Z_0-9]+)"\)', text))
            names |= set(re.findall(r'(?:env_int|host_threads)\("([A-Z_0-9]+)"', text))
    assert names <= {"TMPT_OBJ_THREADS", "TMPT_PNG_THREADS", "TMPT_OBJ_CHUNK", "TMPT_PNG_STRIP"}, names


def test_scene_options_are_checked_before_any_device_work():
    """tmpt_scene_create_ex parses its options first: an unknown key, a bad
    value or a value out of range is -22 with a message; valid options get as
    far as the device lookup (no GPU here)."""
    import numpy as np
    tris = np.zeros((1, 9), np.float32)
    for bad, msg in (("bogus=1", "unknown option"), ("leaf_max=0", "out of range"), ("leaf_max=x", "bad value"),
                     ("builder=kd", "bad value"), ("sample_block=3", "power of two"), ("leaf_max", "no value"),
                     ("pilot=1.5", "integer"), ("row_occ=2", "0 \\(auto\\), 4 or 5"), ("path_waves=3", "0 \\(auto\\), 4 or 5")):
        with pytest.raises(tm.TmptError, match=msg):
            tm.Scene(tris, options=bad)
    if tm.device_count() == 0:
        for good in ("builder=lbvh, leaf_max=4", {"collapse": "sah", "ploc_radius": 8}, "", None, "row_occ=4"):
            with pytest.raises(tm.TmptError, match="device"):
                tm.Scene(tris, options=good)


def test_stats_mirror_matches_the_struct():
    """RenderStats (the Python face of tmpt_stats) carries every field of the
    ctypes mirror except the reserved words, in order, so Scene.stats() can
    build it without a GPU render having run."""
    fields = [f for f, _ in tm._Stats._fields_ if not f.startswith("reserved")]
    assert list(tm.RenderStats._fields if hasattr(tm.RenderStats, "_fields") else
                tm.RenderStats.__dataclass_fields__) == fields
    assert "tie_path" in fields


def test_check_hook_arguments_are_checked_before_any_device_work():
    """tmpt_scene_dump_bvh and tmpt_radix_sort test their arguments first: -22 with a
    message for each bad one, in the documented order, with no scene and no GPU.  (The
    checks that need a scene -- a short buffer, SoA asked of an AoS scene -- are in
    test_gpu_bvh_structure.py.)"""
    lib = ctypes.CDLL(tm.lib_path)
    dump, sort = lib.tmpt_scene_dump_bvh, lib.tmpt_radix_sort
    dump.restype = sort.restype = ctypes.c_int
    dump.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                     ctypes.c_uint64, ctypes.c_void_p]
    sort.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32]
    lib.tmpt_last_error.restype = ctypes.c_char_p
    info = (ctypes.c_int32 * 8)()
    assert dump(None, 0, None, 0, None, 0, info) == -22 and b"null argument" in lib.tmpt_last_error()
    k = (ctypes.c_uint32 * 4)()
    for args, msg in (((None, k, k, 4, 0), b"bits out of range"), ((None, k, k, 4, 33), b"bits out of range"),
                      ((None, k, k, -1, 32), b"n out of range"), ((None, k, k, (1 << 22) + 1, 32), b"n out of range"),
                      ((None, None, k, 4, 32), b"null argument"), ((None, k, None, 4, 32), b"null argument"),
                      ((None, k, k, 4, 32), b"null scene"), ((None, None, None, 0, 8), b"null scene")):
        assert sort(*args) == -22 and msg in lib.tmpt_last_error(), (args[3:], lib.tmpt_last_error())
