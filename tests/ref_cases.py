"""The cases pinned to the reference itself (test helper).

tests/golden/make_ref_fixtures.py runs the compiled reference (oracle/ref/Makefile
-> oracle/_ref/ref_hits, ref_trace and tmpt_ref) on these cases and commits what it answers
under tests/golden/ref/; test_reference_pin.py (CPU) holds the oracle to those
answers and test_gpu_reference_mode.py (GPU) the library; the float shading
chain (ref_trace, TRACE_CASES) is held by test_reference_trace_pin.py (CPU, the
oracle) and test_gpu_reference_trace.py (GPU, the library).  The GPU tests read
the fixtures only: scenes and rays are stored in them, not regenerated.

hits_<case>.npz   tris (n, 3, 3), bmin, bmax (the bounds tm.Scene takes), box (6,
                  the octree's root box, main.cpp:312), rays (m, 8) {origin,
                  direction, tmin, tmax}, hit (m,) int8, rec (m, 7) float32
frame_<case>.png  tmpt_ref's output.png of <case>.obj; frames.json holds the
                  size and the printed "K Rays" of each

trace_<case>.npz  one 32x18 frame of 8 samples a pixel through oracle/_ref/ref_trace
                  (the reference's GetRay, HitScene and Trace(), main.cpp:82-119,
                  212-218, sample by sample): tris, bmin, bmax, box, cam (13:
                  Camera::Camera's arguments), size {w, h, spp}, chains_sample /
                  chains_pixel (k, 4) uint32 {x, y, state, count}; of sample
                  seeding s_ray (n, 6), s_state_ray, s_hit int8, s_tn (n, 4) {t,
                  normal}, s_col (n, 3), s_state, s_rays; of pixel seeding p_col,
                  p_state, p_rays; n = h * w * spp in the order y, x, sample

Regenerate all of it with
    make -C oracle/ref && python tests/golden/make_ref_fixtures.py

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


# ---------------------------------------------------------------- per-sample float radiance (ref_trace)
TRACE_SIZE = (32, 18, 8)  # w, h, spp
TRACE_CASES = ("cube", "room", "room_open", "grid")
TRACE_WORDS = 17  # ref_trace's words per sample (oracle/ref/ref_trace.cpp)
#: what the cases must reach, counted from the reference's answers alone (trace_counts)
TRACE_FLOORS = dict(full_depth=500, late_sky=200, back_face=300, camera_miss=1000, partial_pixels=100)

_QUADS = ((0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3))  # -x +x -y +y -z +z
# two rotations with rational sines (9/41 about z, 11/61 about x): no face of the
# room lies on an octree plane, and no libm call stands between the text and the floats
_RZ = np.array([[40 / 41, -9 / 41, 0], [9 / 41, 40 / 41, 0], [0, 0, 1]])
_RX = np.array([[1, 0, 0], [0, 60 / 61, -11 / 61], [0, 11 / 61, 60 / 61]])
_ROOM_TURN = _RX @ _RZ


def box_tris(lo, hi, inward, faces=range(6)):
    """Two triangles per listed face of the box [lo, hi], their normals
    (cross(v1 - v0, v2 - v1), maths.cpp:303-305) pointing into the box or out of it."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    out = []
    for f in faces:
        q = _QUADS[f]
        for a, b in ((q[2], q[1]), (q[3], q[2])):
            out.append([c[q[0]], c[a], c[b]] if inward else [c[q[0]], c[b], c[a]])
    return np.array(out, np.float64)


def room_tris(open_top):
    """A room [-1, 1]^3 whose walls face inward (Scatter aims along the stored
    normal, main.cpp:71-72, so a path inside stays inside), without its ceiling
    if open_top, and three boxes in it: two facing outward like any solid, one
    facing inward, which the camera therefore sees from behind -- its light term
    takes the flipped normal (main.cpp:66) while the path scatters off the
    stored one and goes on inside that box.  All of it turned by _ROOM_TURN."""
    parts = [box_tris([-1, -1, -1], [1, 1, 1], True, [f for f in range(6) if not (open_top and f == 3)]),
             box_tris([0.0, -0.95, 0.1], [0.5, -0.2, 0.6], False),
             box_tris([-0.6, -0.7, 0.3], [-0.2, 0.1, 0.8], True),
             box_tris([0.3, 0.2, -0.3], [0.6, 0.5, 0.0], False)]
    return (np.concatenate(parts) @ _ROOM_TURN.T).astype(np.float32)


def room_camera(w, h):
    """Camera::Camera's 13 arguments: the eye 0.02 inside the room's -x wall,
    looking along the wall into the room, with a lens of radius 0.06.  A third of
    the lens is outside the closed room: a sample drawn there misses everything
    where the pixel looks along the wall, and elsewhere comes back in through the
    wall's back face -- so even the closed room has pixels of which only some
    samples hit."""
    frm = np.array([-0.98, 0.05, -0.6]) @ _ROOM_TURN.T
    at = np.array([-0.55, -0.3, 0.9]) @ _ROOM_TURN.T
    dist = float(np.float32(np.sqrt(((frm - at) ** 2).sum())))
    return np.array(list(frm) + list(at) + [0.0, 1.0, 0.0, 75.0, np.float32(w) / np.float32(h), 0.12, dist], np.float32)


def ref_camera_args(bmin, bmax, w, h, aperture):
    """main.cpp:296-307 in float32, one rounding per operation: the arguments
    the reference gives Camera::Camera for a scene of these OBJ bounds."""
    f = np.float32
    lo, hi = np.asarray(bmin, f), np.asarray(bmax, f)
    size = hi - lo
    center = (lo + hi) * f(0.5)
    frm = center + size * np.array([0.3, 0.6, 1.2], f)
    at = center + size * np.array([0.0, -0.1, 0.0], f)
    d = frm - at
    dist = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    assert dist.dtype == f and center.dtype == f and frm.dtype == f
    return np.concatenate([frm, at, np.array([0, 1, 0, 60, f(w) / f(h), aperture, dist], f)]).astype(f)


def trace_scene(name):
    """-> (tris, bmin, bmax, cam13) of a trace case.

    Every case must show at least TRACE_FLOORS["partial_pixels"] pixels of which
    only some samples hit; at 32x18 the reference's own view of cube and of grid
    has 47 and 36 (the silhouettes are that short), so two cameras are adjusted:
      cube  the reference's placement and aperture (main.cpp:296-307), but focused
            at 0.1 instead of on the scene, so the lens draw decides near every
            silhouette whether a sample hits;
      grid  a pinhole (aperture 0: the lens draw still advances the state) close
            above the floor's plane with a narrow field of view: the floor is a
            sliver whose two edges cross the frame below the grid's outline."""
    w, h, _ = TRACE_SIZE
    f = np.float32
    if name in ("room", "room_open"):
        tris = room_tris(name == "room_open")
        v = tris.reshape(-1, 3)
        return tris, v.min(0), v.max(0), room_camera(w, h)
    if name == "cube":
        tris, bmin, bmax = hit_scene("cube")
        cam = ref_camera_args(bmin, bmax, w, h, 0.03)
        cam[12] = 0.1
        return tris, bmin, bmax, cam
    tris, bmin, bmax = with_floor(frame_tris(name))  # grid: the octree's ties steer the float paths
    size, center = bmax - bmin, (bmin + bmax) * f(0.5)
    frm, at = center + size * np.array([0.3, -0.485, 1.6], f), center + size * np.array([0, -0.2, 0], f)
    return tris, bmin, bmax, np.concatenate([frm, at, np.array([0, 1, 0, 28, f(w) / f(h), 0, 1], f)]).astype(f)


def seed_chains(w, h, spp, sample_seeding):
    """uint32 (k, 4) {x, y, state, count} in the order y, x (, sample): sample
    seeding is a chain of one sample per sample from its jumped state
    (oracle.sample_seed), pixel seeding one chain of spp samples per pixel from
    oracle.pixel_seed."""
    import oracle
    out = []
    for y in range(h):
        for x in range(w):
            seed = oracle.pixel_seed(x, y, w)
            if sample_seeding:
                out += [(x, y, oracle.sample_seed(seed, s), 1) for s in range(spp)]
            else:
                out.append((x, y, seed, spp))
    return np.array(out, np.uint32)


def run_ref_trace(exe, tris, box, cam, w, h, chains, tmp_dir):
    """The reference's answers per sample, chain after chain: dict of ray (n, 6)
    float32, state_ray uint32, hit int8, tn (n, 4) float32 {t, normal}, col (n, 3)
    float32, state uint32, rays int32."""
    import subprocess
    t = np.ascontiguousarray(np.asarray(tris, np.float32).reshape(-1, 9))
    ch = np.ascontiguousarray(np.asarray(chains, np.uint32).reshape(-1, 4))
    fin, fout = os.path.join(str(tmp_dir), "ref_trace.in"), os.path.join(str(tmp_dir), "ref_trace.out")
    with open(fin, "wb") as f:
        f.write(np.array([len(t), len(ch), w, h], np.int32).tobytes())
        f.write(np.asarray(box, np.float32).reshape(6).tobytes())
        f.write(np.asarray(cam, np.float32).reshape(13).tobytes())
        f.write(t.tobytes())
        f.write(ch.tobytes())
    subprocess.run([exe, fin, fout], check=True)
    n = int(ch[:, 3].sum())
    raw = np.fromfile(fout, np.uint32)
    assert raw.size == n * TRACE_WORDS
    raw = raw.reshape(n, TRACE_WORDS)
    f32 = lambda a: np.ascontiguousarray(a).view(np.float32)
    return dict(ray=f32(raw[:, 0:6]), state_ray=raw[:, 6].copy(), hit=raw[:, 7].astype(np.int8),
                tn=f32(raw[:, 8:12]), col=f32(raw[:, 12:15]), state=raw[:, 15].copy(),
                rays=raw[:, 16].astype(np.int32))


def trace_path(name):
    return os.path.join(REF_DIR, f"trace_{name}.npz")


def load_trace(name):
    """The committed fixture of a trace case, arrays read-only."""
    with np.load(trace_path(name)) as z:
        out = {k: z[k] for k in z.files}
    for a in out.values():
        a.setflags(write=False)
    return out


def trace_counts(fx):
    """What a trace fixture's sample-seeded samples reach, from the reference's
    answers alone: samples of exactly 20 rays (ten bounces, the cap of
    main.cpp:33,89), samples that left to the sky after three or more bounces
    (2 k + 1 rays, k >= 3), first hits seen from behind (dot(normal, dir) >= 0,
    main.cpp:66), camera rays that miss, pixels of which 1 .. spp - 1 samples
    hit, non-finite colour floats (both seedings)."""
    w, h, spp = (int(v) for v in fx["size"])
    rays, hit = fx["s_rays"], fx["s_hit"].astype(bool)
    n, d = fx["s_tn"][:, 1:4], fx["s_ray"][:, 3:6]
    facing = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]
    per_pixel = hit.reshape(h * w, spp).sum(1)
    return dict(full_depth=int((rays == 20).sum()), late_sky=int(((rays >= 7) & (rays % 2 == 1)).sum()),
                back_face=int((hit & (facing >= 0)).sum()), camera_miss=int((~hit).sum()),
                partial_pixels=int(((per_pixel > 0) & (per_pixel < spp)).sum()),
                non_finite=int((~np.isfinite(fx["s_col"])).sum() + (~np.isfinite(fx["p_col"])).sum()))


def check_trace_counts(counts):
    """The floors of TRACE_FLOORS over {case: trace_counts}: the first four over
    all cases together, partial pixels in each case, and no non-finite colour."""
    assert set(counts) == set(TRACE_CASES), sorted(counts)
    for key in ("full_depth", "late_sky", "back_face", "camera_miss"):
        total = sum(c[key] for c in counts.values())
        assert total >= TRACE_FLOORS[key], (key, total, counts)
    for name, c in counts.items():
        assert c["partial_pixels"] >= TRACE_FLOORS["partial_pixels"], (name, c)
        assert c["non_finite"] == 0, (name, c)
