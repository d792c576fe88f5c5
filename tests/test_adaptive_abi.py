"""Adaptive sampling's ABI and its restatement, without a GPU: the header declares
tmpt_render_adaptive and its two structs as the ctypes mirrors lay them out, the
restatement (adaptive_restate.py) degenerates to radiance_expect at both ends
of the threshold range, and every case the GPU tests run spreads its pixels
over several counts -- a condition on the inputs, so a GPU run cannot pass
vacuously."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import toymeshpathtracer_amd as tm
from adaptive_restate import (CASES, CASE_IDS, adaptive_expect, camera, case_expect, oracle_scene, scene_samples,
                              schedule)
from conftest import ROOT
from render_restate import radiance_expect, same_bits

f32 = np.float32
HEADER = os.path.join(ROOT, "include", "tmpt.h")


def test_header_declares_the_entry_point_and_structs(tmp_path):
    text = open(HEADER).read()
    assert "tmpt_render_adaptive" in tm.EXPORTS
    for word in ("int tmpt_render_adaptive(", "} tmpt_adaptive_desc;", "} tmpt_adaptive_info;"):
        assert word in text, word
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tmpt.h"\n'
                   'int main(void){ printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(tmpt_adaptive_desc), '
                   'offsetof(tmpt_adaptive_desc, threshold), sizeof(tmpt_adaptive_info), '
                   'offsetof(tmpt_adaptive_info, samples), offsetof(tmpt_adaptive_info, pass_pixels), '
                   'sizeof(((tmpt_adaptive_info*)0)->pass_pixels)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    d, i = tm._AdaptiveDesc, tm._AdaptiveInfo
    want = [ctypes.sizeof(d), d.threshold.offset, ctypes.sizeof(i), i.samples.offset, i.pass_pixels.offset,
            i.pass_pixels.size]
    assert got == want == [32, 8, 528, 8, 16, 512]


def test_the_library_exports_the_entry_point():
    assert hasattr(tm._lib, "tmpt_render_adaptive")
    assert tm.abi_version() == 9  # additive


def test_schedule():
    assert schedule(16, 4, 4) == [4, 8, 12, 16]
    assert schedule(19, 6, 5) == [6, 11, 16, 19]
    assert schedule(12, 2, 3) == [2, 5, 8, 11, 12]
    assert schedule(16, 16, 4) == [16]


@pytest.fixture(scope="module")
def suzanne():
    return scene_samples("suzanne.obj", 32, 18, 16)


def _uniform(spp):
    return radiance_expect(oracle_scene("suzanne.obj"), camera("suzanne.obj", 32, 18).as_array(), 32, 18, spp,
                           tm.SEED_SAMPLE)


def test_tau_one_is_the_frame_at_spp_min(suzanne):
    col, rays = suzanne
    n_p, rad, total, pass_pixels = adaptive_expect(col, rays, 4, 4, 1.0)
    want, want_rays = _uniform(4)
    assert (n_p == 4).all() and pass_pixels == [32 * 18]
    same_bits(rad, want, "tau 1")
    assert total == want_rays


def test_spp_min_at_the_cap_is_the_frame_at_the_cap(suzanne):
    col, rays = suzanne
    n_p, rad, total, pass_pixels = adaptive_expect(col, rays, 16, 4, 0.02)
    want, want_rays = _uniform(16)
    assert (n_p == 16).all() and pass_pixels == [32 * 18]
    same_bits(rad, want, "spp_min = cap")
    assert total == want_rays
    # and tau 0 runs every pixel of this frame to the cap (no pixel's samples agree exactly)
    n_0, rad_0, total_0, pp_0 = adaptive_expect(col, rays, 4, 4, 0.0)
    assert (n_0 == 16).all() and pp_0 == [32 * 18] * 4 and total_0 == want_rays
    same_bits(rad_0, want, "tau 0")


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_gpu_cases_spread_over_the_counts(case):
    n_p, rad, total, pass_pixels = case_expect(case)
    counts = {int(n): int((n_p == n).sum()) for n in np.unique(n_p)}
    print(case, counts, "samples", int(n_p.sum()), "of", n_p.size * case[3], "pass_pixels", pass_pixels)
    assert sum(1 for v in counts.values() if v >= 3) >= 3, counts
    assert set(counts) <= set(schedule(case[3], case[4], case[5]))
    assert np.isfinite(rad).all()
    assert int(n_p.sum()) == sum(p * (b - a) for p, a, b in
                                 zip(pass_pixels, [0] + schedule(case[3], case[4], case[5]),
                                     schedule(case[3], case[4], case[5])))
