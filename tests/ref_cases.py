"""The cases pinned to the reference itself (test helper).

tests/golden/make_ref_fixtures.py runs the compiled reference (oracle/ref/Makefile
-> oracle/_ref/ref_hits and tmpt_ref) on these cases and commits what it answers
under tests/golden/ref/; test_reference_pin.py (CPU) holds the oracle to those
answers and test_gpu_reference_mode.py (GPU) the library.  The GPU tests read
the fixtures only: scenes and rays are stored in them, not regenerated.

hits_<case>.npz   tris (n, 3, 3), bmin, bmax (the bounds tm.Scene takes), box (6,
                  the octree's root box, main.cpp:312), rays (m, 8) {origin,
                  direction, tmin, tmax}, hit (m,) int8, rec (m, 7) float32
frame_<case>.png  tmpt_ref's output.png of <case>.obj; frames.json holds the
                  size and the printed "K Rays" of each

Ray ranges: the G.rays part of every case is queried with G.ray_range(tris) (1e-3
.. 1e7 at unit scale), the rays aimed at the octree's own planes and the crack
wall (octree_kat.py) with the reference's constants 0.001 .. 1e7 (main.cpp:30-31).
The latter are made only for the scenes with a modest octree (grid, crack_wall,
cube, suzanne, teapot): they walk every leaf list in Python, and the families'
octrees have up to 900,000 nodes.
"""
import io
import json
import os
import zipfile

import numpy as np

import geometry_cases as G

HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(HERE, "golden", "ref")
DATA = os.path.join(os.path.dirname(HERE), "data")

SLOW_FAMILIES = ("coincident130", "coincident200", "coincident1000")  # 4 .. 36 s of reference octree build
FAMILIES = tuple(n for n in G.NON_SWEEP if n not in SLOW_FAMILIES)
SOUPS = ("soup3", "soup64", "soup272", "soup4096")
KAT_SCENES = ("grid", "crack_wall", "cube", "suzanne", "teapot")
HIT_CASES = FAMILIES + SOUPS + KAT_SCENES

N_RAYS, N_PER_KIND, N_WALL, RAY_SEED = 4000, 500, 2000, 7
REF_RANGE = (0.001, 1.0e7)  # kMinT, kMaxT (main.cpp:30-31)

# frames: (w, h, spp); the two families are the unit-scale ones of which the
# reference's own camera (main.cpp:295-307) sees most
FRAME_SIZE = (160, 90, 2)
FRAME_CASES = ("grid", "child_order", "cube", "crack_wall", "samebox_fan150", "segments200")
REGENERATED_OBJ = ("crack_wall",)  # teapot-sized: written by the script and the tests, not committed


def octree_box(bmin, bmax):
    """main.cpp:296-297,312 in float32: bounds -+ 0.7 x size."""
    lo, hi = np.asarray(bmin, np.float32), np.asarray(bmax, np.float32)
    extra = ((hi - lo) * np.float32(0.7)).astype(np.float32)
    return np.concatenate([lo - extra, hi + extra]).astype(np.float32)


def with_floor(tris):
    """The case as LoadScene (main.cpp:132-162) would hand it over: the two floor
    triangles appended, and the bounds of the case alone."""
    t = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    v = t.reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    e = ((hi - lo) * np.float32(0.7)).astype(np.float32)
    x0, x1, z0, z1, y = lo[0] - e[0], hi[0] + e[0], lo[2] - e[2], hi[2] + e[2], lo[1]
    floor = np.array([[[x0, y, z0], [x0, y, z1], [x1, y, z0]],
                      [[x0, y, z1], [x1, y, z1], [x1, y, z0]]], np.float32)
    return np.concatenate([t, floor]), lo, hi


def obj_text(tris):
    """An OBJ of the triangles, three vertices each, %.9g: float32 survives it."""
    t = np.asarray(tris, np.float32).reshape(-1, 3)
    lines = ["v %.9g %.9g %.9g" % tuple(float(x) for x in v) for v in t]
    lines += ["f %d %d %d" % (3 * i + 1, 3 * i + 2, 3 * i + 3) for i in range(len(t) // 3)]
    return "\n".join(lines) + "\n"


def _obj_tris(name):
    """Triangles of a committed OBJ without the floor."""
    import oracle
    tris, bmin, bmax = oracle.load_scene(os.path.join(DATA, name + ".obj"))
    return tris[:-2], bmin, bmax


def crack_wall_tris():
    """teapot plus a wall lying in a crack of its octree (octree_kat.crack_wall_scene),
    the wall last: (tris without the floor, the wall's axis)."""
    import oracle
    import octree_kat as K
    tris, bmin, bmax = oracle.load_scene(os.path.join(DATA, "teapot.obj"))
    t2, ax, _ = K.crack_wall_scene(tris, bmin, bmax)
    return np.concatenate([tris[:-2], t2[-1:]]), ax


def frame_tris(name):
    """The triangles a frame case's OBJ holds (the reference adds the floor)."""
    import octree_kat as K
    if name == "grid":
        return K.grid_scene()[0]
    if name == "child_order":
        return K.child_order_case()[0]
    if name == "crack_wall":
        return crack_wall_tris()[0]
    if name == "cube":
        return _obj_tris("cube")[0]
    return G.case(name)


def frame_obj_path(name, tmp_dir):
    """Path of the case's OBJ: the committed one, or (REGENERATED_OBJ) written into tmp_dir."""
    if name == "cube":
        return os.path.join(DATA, "cube.obj")
    if name not in REGENERATED_OBJ:
        return os.path.join(REF_DIR, name + ".obj")
    path = os.path.join(str(tmp_dir), name + ".obj")
    with open(path, "w") as f:
        f.write(obj_text(frame_tris(name)))
    return path


def hit_scene(name):
    """-> (tris, bmin, bmax) of a hit case: what tm.Scene(tris, bounds=(bmin, bmax)) takes."""
    import octree_kat as K
    if name in FAMILIES or name in SOUPS:
        tris = G.case(name)
        v = tris.reshape(-1, 3)
        return tris, v.min(0), v.max(0)
    if name == "grid":
        return K.grid_scene()
    if name == "crack_wall":
        return with_floor(crack_wall_tris()[0])
    tris, bmin, bmax = _obj_tris(name)
    t2, lo, hi = with_floor(tris)
    assert np.array_equal(lo, bmin) and np.array_equal(hi, bmax)
    return t2, bmin, bmax


def hit_rays(name, tris, bmin, bmax):
    """-> rays (m, 8) float32 of a hit case."""
    import octree_kat as K
    r6, rng = G.rays(tris, N_RAYS, RAY_SEED)
    parts = [np.concatenate([r6, np.tile(np.array(rng, np.float32), (len(r6), 1))], 1)]
    if name in KAT_SCENES:
        adv, _ = K.adversarial_rays(tris, bmin, bmax, N_PER_KIND, seed=RAY_SEED)
        if name == "crack_wall":  # the wall stands before the two floor triangles
            adv = np.concatenate([adv, K.crack_wall_rays(tris[-3], crack_wall_tris()[1], N_WALL, seed=RAY_SEED)])
        parts.append(np.concatenate([adv, np.tile(np.array(REF_RANGE, np.float32), (len(adv), 1))], 1))
    return np.ascontiguousarray(np.concatenate(parts).astype(np.float32))


def run_ref_hits(exe, tris, box, rays, tmp_dir):
    """The reference's answers: (hit int8 (m,), rec float32 (m, 7))."""
    import subprocess
    t = np.ascontiguousarray(np.asarray(tris, np.float32).reshape(-1, 9))
    r = np.ascontiguousarray(np.asarray(rays, np.float32).reshape(-1, 8))
    fin, fout = os.path.join(str(tmp_dir), "ref_hits.in"), os.path.join(str(tmp_dir), "ref_hits.out")
    with open(fin, "wb") as f:
        f.write(np.array([len(t), len(r)], np.int32).tobytes())
        f.write(np.asarray(box, np.float32).tobytes())
        f.write(t.tobytes())
        f.write(r.tobytes())
    subprocess.run([exe, fin, fout], check=True)
    raw = open(fout, "rb").read()
    assert len(raw) == len(r) * 29
    hit = np.frombuffer(raw, np.int8, len(r)).copy()
    rec = np.frombuffer(raw[len(r):], np.float32).reshape(-1, 7).copy()
    return hit, rec


def hits_path(name):
    return os.path.join(REF_DIR, f"hits_{name}.npz")


def save_npz(path, arrays):
    """np.savez_compressed with fixed member dates: the same arrays give the same file."""
    with zipfile.ZipFile(path, "w") as z:
        for key, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def load_hits(name):
    """The committed fixture of a hit case, arrays read-only."""
    with np.load(hits_path(name)) as z:
        out = {k: z[k] for k in z.files}
    for a in out.values():
        a.setflags(write=False)
    return out


def range_groups(rays8):
    """[(tmin, tmax, indices)] of the distinct ranges among rays (m, 8)."""
    pairs = np.unique(rays8[:, 6:], axis=0)
    return [(float(lo), float(hi), np.nonzero((rays8[:, 6] == lo) & (rays8[:, 7] == hi))[0]) for lo, hi in pairs]


def frames_json():
    with open(os.path.join(REF_DIR, "frames.json")) as f:
        return json.load(f)
