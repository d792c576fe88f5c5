"""The oracle's octree and the library's flagging against the reference itself
(CPU; no GPU).

tests/golden/ref/ holds what the compiled, unmodified reference answered
(tests/golden/make_ref_fixtures.py; cases and formats in tests/ref_cases.py):
Scene::HitScene on a few thousand rays per case -- the adversarial families of
geometry_cases.py, four soups, and grid, crack_wall, cube, suzanne and teapot
with rays aimed at their octree's planes -- and its CLI's frames of six OBJs.

Tolerance: none.  The oracle's octree (oracle/tmpt_oracle.c, our restatement of
scene.cpp) must give the reference's hit bit and hit record bit for bit on every
ray, and its row-seeded frame the reference's PNG byte for byte with the printed
ray count.  The library's host hooks must flag every ray on which the
reference's answer differs from the exact closest hit otherwise than by a tie
on t or a root-box rejection (what the device then re-answers over the octree),
and build an octree of the oracle's node count and digest.
"""
import functools
import os

import numpy as np
import pytest
from PIL import Image

import oracle
import ref_cases as C
import toymeshpathtracer_amd as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_HITS = os.path.join(ROOT, "oracle", "_ref", "ref_hits")


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _batch(sc, rays8):
    """hit_batch range group by range group -> (ids, records)."""
    ids, rec = np.full(len(rays8), -1, np.int32), np.zeros((len(rays8), 7), np.float32)
    for lo, hi, sel in C.range_groups(rays8):
        ids[sel], rec[sel] = sc.hit_batch(rays8[sel, :6], lo, hi)
    return ids, rec


@functools.lru_cache(maxsize=None)
def _case(name):
    """The fixture, the oracle octree's answers and the exact closest hits: once per case."""
    fx = C.load_hits(name)
    osc = oracle.Scene(fx["tris"], accel=oracle.ACCEL_OCTREE, tie=oracle.TIE_VISIT, bmin=fx["bmin"], bmax=fx["bmax"])
    ex = oracle.Scene(fx["tris"], accel=oracle.ACCEL_BVH, tie=oracle.TIE_INDEX, bmin=fx["bmin"], bmax=fx["bmax"])
    rid, rh = _batch(osc, fx["rays"])
    eid, eh = _batch(ex, fx["rays"])
    boxes, _ = osc.octree_nodes()
    out = dict(fx=fx, rid=rid, rh=rh, eid=eid, eh=eh, nodes=len(boxes), root=boxes[0].copy(),
               digest=osc.octree_digest())
    for a in (rid, rh, eid, eh):
        a.setflags(write=False)
    return out


def test_fixture_list_is_complete():
    """Every case of ref_cases.py has its fixture, and its box is main.cpp:312's."""
    for name in C.HIT_CASES:
        fx = C.load_hits(name)
        assert fx["rays"].shape[1] == 8 and fx["hit"].shape == (len(fx["rays"]),) and fx["rec"].shape[1] == 7
        assert np.array_equal(_u32(fx["box"]), _u32(C.octree_box(fx["bmin"], fx["bmax"])))
        assert np.array_equal(_u32(fx["box"]), _u32(np.concatenate(tm.octree_bounds(fx["bmin"], fx["bmax"]))))
    assert set(C.frames_json()) == set(C.FRAME_CASES)


@pytest.mark.parametrize("name", C.HIT_CASES)
def test_oracle_octree_equals_reference(name):
    """Hit bit and the seven record floats of every ray, bit for bit."""
    c = _case(name)
    fx = c["fx"]
    assert np.array_equal(_u32(c["root"]), _u32(fx["box"]))
    hit = fx["hit"].astype(bool)
    wrong = np.nonzero((c["rid"] >= 0) != hit)[0]
    assert wrong.size == 0, f"{wrong.size} hit bits differ, first rays {wrong[:5]}"
    rec = np.nonzero((_u32(c["rh"][hit]) != _u32(fx["rec"][hit])).any(1))[0]
    assert rec.size == 0, f"{rec.size} records differ, first rays {np.nonzero(hit)[0][rec[:5]]}"
    assert hit.sum() > len(hit) // 4


@pytest.mark.parametrize("name", C.HIT_CASES)
def test_fresh_reference_run_equals_fixture(name, tmp_path):
    """With the compiled reference at hand: it answers today what the fixture holds."""
    if not os.path.exists(REF_HITS):
        pytest.skip("oracle/_ref/ref_hits not built (make -C oracle/ref, needs a reference checkout)")
    fx = C.load_hits(name)
    hit, rec = C.run_ref_hits(REF_HITS, fx["tris"], fx["box"], fx["rays"], tmp_path)
    assert np.array_equal(hit, fx["hit"]) and np.array_equal(_u32(rec), _u32(fx["rec"]))


def _classes(c):
    """The reference's answer (the fixture) against the exact closest hit: ray
    indices of ties on t, root-box rejections and the rest."""
    fx = c["fx"]
    hit, ehit = fx["hit"].astype(bool), c["eid"] >= 0
    both = hit & ehit
    diff = (hit != ehit) | (both & (_u32(fx["rec"]) != _u32(c["eh"])).any(1))
    tie = diff & both & (_u32(fx["rec"][:, 6]) == _u32(c["eh"][:, 6]))
    root_ok = np.zeros(len(hit), bool)
    for lo, hi, sel in C.range_groups(fx["rays"]):
        root_ok[sel] = oracle.ray_box(fx["rays"][sel, :6], fx["box"], lo, hi)
    root = diff & ~hit & ~root_ok
    return diff, tie, root, diff & ~tie & ~root


@pytest.mark.parametrize("name", C.HIT_CASES)
def test_library_flags_what_the_reference_answers_differently(name):
    """tmpt_octree_flags is non-zero on every ray of class "other"; the
    library's host octree has the oracle's node count and digest."""
    c = _case(name)
    fx = c["fx"]
    diff, tie, root, other = _classes(c)
    flags, _ = tm.octree_flags(fx["tris"], fx["box"][:3], fx["box"][3:], fx["rays"], c["eh"][:, 6], c["eid"])
    hits = c["eid"] >= 0
    print(f"{name}: rays {len(diff)} differ {int(diff.sum())} tie {int(tie.sum())} root {int(root.sum())} "
          f"other {int(other.sum())}; flagged {int((flags[hits] > 0).sum())} of {int(hits.sum())} exact hits "
          f"(flat {int((flags[hits] & 1 > 0).sum())}, crack {int((flags[hits] & 2 > 0).sum())}); nodes {c['nodes']}")
    unflagged = np.nonzero(other & (flags == 0))[0]
    assert unflagged.size == 0, f"{unflagged.size} unflagged deviations, first rays {unflagged[:5]}"
    d = tm.octree_digest(fx["tris"], fx["box"][:3], fx["box"][3:])
    assert (d["nodes"], d["digest"]) == (c["nodes"], c["digest"])


def test_hit_fixtures_are_not_vacuous():
    """From the oracle alone: on at least 1,000 fixture rays the octree's answer
    is not the exact closest hit."""
    total = {name: int((_case(name)["rid"] != _case(name)["eid"]).sum()) for name in C.HIT_CASES}
    print(total)
    assert sum(total.values()) >= 1000, total


# ---------------------------------------------------------------- frames
@functools.lru_cache(maxsize=None)
def _frame(name, accel, tie):
    tris, bmin, bmax = oracle.load_scene(C.frame_obj_path(name, _TMP[0]))
    f = C.frames_json()[name]
    cam = oracle.camera_for_scene(bmin, bmax, f["width"], f["height"])
    sc = oracle.Scene(tris, accel=accel, tie=tie, bmin=bmin, bmax=bmax)
    return sc.render(cam, f["width"], f["height"], f["spp"], seed_mode=oracle.SEED_ROW)


_TMP = [None]


@pytest.fixture(scope="module", autouse=True)
def _obj_dir(tmp_path_factory):
    _TMP[0] = tmp_path_factory.mktemp("ref_obj")


@pytest.mark.parametrize("name", C.FRAME_CASES)
def test_obj_exports_round_trip(name):
    """The OBJ a frame was made from holds the case's triangles bit for bit
    (and the committed exports are what the generators give today)."""
    if name == "cube":
        return
    want = C.frame_tris(name)
    if name not in C.REGENERATED_OBJ:
        assert open(os.path.join(C.REF_DIR, name + ".obj")).read() == C.obj_text(want)
    tris, _, _ = oracle.load_scene(C.frame_obj_path(name, _TMP[0]))
    assert np.array_equal(_u32(tris[:-2]), _u32(want))
    t2, lo, hi = C.with_floor(want)
    assert np.array_equal(_u32(tris), _u32(t2))


@pytest.mark.parametrize("name", C.FRAME_CASES)
def test_oracle_frame_equals_reference_png(name):
    """Row seeding, the reference's camera: the PNG byte for byte, the printed K Rays."""
    img, rays = _frame(name, oracle.ACCEL_OCTREE, oracle.TIE_VISIT)
    ref = np.asarray(Image.open(os.path.join(C.REF_DIR, f"frame_{name}.png")).convert("RGBA"))
    diff = np.nonzero((img[::-1] != ref).any(-1))  # PNGs are written flipped (main.cpp:341)
    assert diff[0].size == 0, f"{diff[0].size} pixels differ, first at {list(zip(*diff))[:5]}"
    assert round(rays / 1000.0, 1) == C.frames_json()[name]["krays"]


def test_frame_fixtures_are_not_vacuous():
    """From the oracle alone: at least one frame is not the exact-BVH frame."""
    px = {}
    for name in C.FRAME_CASES:
        a, _ = _frame(name, oracle.ACCEL_OCTREE, oracle.TIE_VISIT)
        b, _ = _frame(name, oracle.ACCEL_BVH, oracle.TIE_INDEX)
        px[name] = int((a != b).any(-1).sum())
    print(px)
    assert max(px.values()) >= 1, px
