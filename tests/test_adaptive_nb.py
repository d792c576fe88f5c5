"""Adaptive sampling's neighbourhood rule (tmpt_adaptive_desc.radius) without a
GPU: the header declares the field where the ctypes mirror puts it, the
restatement (adaptive_nb_restate.py) is adaptive_restate's at radius 0, monotone
in the radius and clipped to the band, and every case the GPU tests run moves
enough pixels off their radius-0 counts that no GPU run can pass vacuously --
with a dilation that drops the carry across a 32- or 64-column seam giving
another map on the 100-wide frame."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import toymeshpathtracer_amd as tm
from adaptive_nb_restate import NB_CASES, NB_IDS, adaptive_nb_expect, counts_of, nb_case_expect, neighbourhood_any
from adaptive_restate import CASES, CASE_IDS, adaptive_expect, case_expect, scene_samples, schedule
from conftest import ROOT
from render_restate import same_bits

HEADER = os.path.join(ROOT, "include", "tmpt.h")

#: the figures of the cases as first measured (a second restatement's cross-check): counts, and where
#: given pass_pixels, rays and the pixels whose count differs from the radius-0 count
FIGURES = {
    "suzanne-32x18x16-4-4-tau0.02-r1-band0": ({4: 188, 8: 114, 12: 43, 16: 231}, None, None, 291),
    "suzanne-100x28x12-4-4-tau0.02-r2-band0": ({4: 1539, 8: 489, 12: 772}, [2800, 1261, 772], 48018, 1003),
    "teapot-24x14x12-2-3-tau0.02-r1-band0": ({2: 131, 5: 17, 8: 32, 11: 27, 12: 129}, None, None, None),
    "suzanne-37x11x16-4-4-tau0.02-r8-band0": ({8: 88, 12: 22, 16: 297}, None, None, None),
    "suzanne-37x11x16-4-4-tau0.02-r8-band3": ({4: 63, 8: 63, 12: 22, 16: 259}, None, None, None),
    "cube-16x9x19-6-5-tau0.01-index-r1-band0": ({6: 17, 16: 7, 19: 120}, None, None, None),
    "suzanne-37x11x16-4-4-tau0.02-r2-band3": (None, [407, 236, 149, 127], 9784, None),
    "suzanne-37x11x16-4-4-tau0.02-r2-band0": (None, [407, 273, 166, 147], 10234, None),
    "suzanne-37x11x16-4-4-tau0.02-r2-band1": ({4: 226, 8: 71, 12: 11, 16: 99}, None, None, None),
}


def test_header_declares_radius(tmp_path):
    text = open(HEADER).read()
    assert "int32_t radius;" in text
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tmpt.h"\n'
                   'int main(void){ printf("%zu %zu %zu %zu %zu\\n", sizeof(tmpt_adaptive_desc), '
                   'offsetof(tmpt_adaptive_desc, threshold), offsetof(tmpt_adaptive_desc, radius), '
                   'offsetof(tmpt_adaptive_desc, reserved), sizeof(((tmpt_adaptive_desc*)0)->reserved)); '
                   'return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    d = tm._AdaptiveDesc
    want = [ctypes.sizeof(d), d.threshold.offset, d.radius.offset, d.reserved.offset, d.reserved.size]
    assert got == want == [32, 8, 12, 16, 16]
    assert tm.abi_version() == 9  # additive


def test_trace_adaptive_takes_radius_last():
    params = list(inspect.signature(tm.Scene.trace_adaptive).parameters.values())
    assert params[-1].name == "radius" and params[-1].default == 0
    assert tm._AdaptiveDesc().radius == 0


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_radius_zero_is_the_own_rule(case):
    name, w, h, cap, spp_min, spp_step, tau, index = case
    col, rays = scene_samples(name, w, h, cap, index)
    want = case_expect(case)
    for band_rows in (0, 1, 4):  # radius 0 does not depend on the bands
        got = adaptive_nb_expect(col, rays, spp_min, spp_step, tau, 0, band_rows)
        assert np.array_equal(got[0], want[0]) and got[2] == want[2] and got[3] == want[3]
        same_bits(got[1], want[1], "radius 0")


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_monotone_in_the_radius(case):
    name, w, h, cap, spp_min, spp_step, tau, index = case
    col, rays = scene_samples(name, w, h, cap, index)
    n0 = case_expect(case)[0]
    n1 = adaptive_nb_expect(col, rays, spp_min, spp_step, tau, 1, 0)[0]
    n2 = adaptive_nb_expect(col, rays, spp_min, spp_step, tau, 2, 0)[0]
    assert (n2 >= n1).all() and (n1 >= n0).all()
    assert (n2 > n1).any() and (n1 > n0).any()


def test_the_neighbourhood_by_its_definition():
    own = np.zeros((7, 9), bool)
    own[3, 4] = True
    assert neighbourhood_any(own, 1, 0).sum() == 9 and neighbourhood_any(own, 2, 0).sum() == 25
    assert neighbourhood_any(own, 8, 0).all()
    got = neighbourhood_any(own, 2, 3)  # bands of rows 0-2, 3-5, 6: only row 3's band is reached
    assert got[3:6, 2:7].all() and got.sum() == 15
    assert neighbourhood_any(own, 2, 1).sum() == 5  # 1-row bands: horizontal reach only
    own[:] = False
    own[0, 0] = True
    assert neighbourhood_any(own, 2, 0).sum() == 9  # clipped by the frame


def test_band_clause():
    """With band_rows = 3 the frame is four independent frames, one per band."""
    name, w, h, cap, r, band = "suzanne.obj", 37, 11, 16, 2, 3
    col, rays = scene_samples(name, w, h, cap)
    n_p, rad, total, pass_pixels = adaptive_nb_expect(col, rays, 4, 4, 0.02, r, band)
    parts = [adaptive_nb_expect(col[y:y + band], rays[y:y + band], 4, 4, 0.02, r, 0) for y in range(0, h, band)]
    assert [p[0].shape[0] for p in parts] == [3, 3, 3, 2]
    assert np.array_equal(np.concatenate([p[0] for p in parts]), n_p)
    same_bits(np.concatenate([p[1] for p in parts]), rad, "bands")
    assert sum(p[2] for p in parts) == total
    whole = adaptive_nb_expect(col, rays, 4, 4, 0.02, r, 0)
    differ = int((whole[0] != n_p).sum())
    print("band_rows 3 against 0:", differ, "pixels differ")
    assert differ == 50 and (whole[0] >= n_p).all()


@pytest.mark.parametrize("case", NB_CASES, ids=NB_IDS)
def test_gpu_cases_move_pixels_off_their_own_counts(case):
    name, w, h, cap, spp_min, spp_step, tau, index, radius, band_rows = case
    n_p, rad, total, pass_pixels = nb_case_expect(case)
    col, rays = scene_samples(name, w, h, cap, index)
    n_0 = adaptive_expect(col, rays, spp_min, spp_step, tau)[0]
    counts = counts_of(n_p)
    moved = int((n_p != n_0).sum())
    print(case, counts, "pass_pixels", pass_pixels, "rays", total, "moved", moved, "of", n_p.size)
    assert sum(1 for v in counts.values() if v >= 3) >= 3, counts
    assert set(counts) <= set(schedule(cap, spp_min, spp_step))
    assert 10 * moved >= n_p.size, (moved, n_p.size)
    assert (n_p < cap).any() and (n_p >= n_0).all()
    assert np.isfinite(rad).all()
    want_counts, want_pp, want_rays, want_moved = FIGURES[NB_IDS[NB_CASES.index(case)]]
    assert want_counts is None or counts == want_counts
    assert want_pp is None or pass_pixels == want_pp
    assert want_rays is None or total == want_rays
    assert want_moved is None or moved == want_moved


def test_the_routes_frame_moves_pixels_too():
    """suzanne 64x36x20 (4, 8) at radius 1, the frame test_gpu_adaptive_nb.py runs through every route."""
    col, rays = scene_samples("suzanne.obj", 64, 36, 20)
    n_0 = adaptive_expect(col, rays, 4, 8, 0.02)[0]
    n_1 = adaptive_nb_expect(col, rays, 4, 8, 0.02, 1, 0)[0]
    counts, moved = counts_of(n_1), int((n_1 != n_0).sum())
    print(counts, "moved", moved, "of", n_1.size)
    assert set(counts) == {4, 12, 20} and min(counts.values()) >= 3
    assert 10 * moved >= n_1.size and (n_1 >= n_0).all()


def _no_carry(seam):
    """A wrong dilation: the neighbourhood does not reach across a column that is a multiple of seam."""
    def dilate(own, radius, band_rows):
        out = np.zeros_like(own)
        for x0 in range(0, own.shape[1], seam):
            out[:, x0:x0 + seam] = neighbourhood_any(own[:, x0:x0 + seam], radius, band_rows)
        return out
    return dilate


@pytest.mark.parametrize("seam", [32, 64])
def test_a_word_seam_bug_cannot_pass(seam):
    """On the 100-wide case a dilation that loses the carry between 32- or 64-bit
    words gives another map, so the GPU's cannot hide one."""
    case = NB_CASES[1]
    name, w, h, cap, spp_min, spp_step, tau, index, radius, band_rows = case
    assert w == 100 and radius == 2
    col, rays = scene_samples(name, w, h, cap, index)
    wrong = adaptive_nb_expect(col, rays, spp_min, spp_step, tau, radius, band_rows, dilate=_no_carry(seam))[0]
    bad = np.argwhere(wrong != nb_case_expect(case)[0])
    print("seam", seam, len(bad), "pixels differ, columns", sorted({int(x) for _, x in bad}))
    assert len(bad) == {32: 13, 64: 8}[seam]  # as first measured: columns 30-33 and 64-65; 64-65
    # the first pixels to go wrong lie within the radius of a seam
    assert any(int(x) % seam in (seam - 2, seam - 1, 0, 1) for _, x in bad)
