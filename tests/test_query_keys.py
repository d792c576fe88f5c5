"""The sort key of option query_sort without a GPU: tmpt_query_keys (the host
compiles the function the key kernel compiles, csrc/tmpt_query_key.h) against
its float32 numpy restatement (query_key_restate.py), word for word, on every
ray family of ray_cases.py over four scenes -- one of them flat, so one axis of
the box has extent 0 and the 1e-30 floor decides -- plus rays with NaN and
+-inf in each component, origins exactly on both faces of the box and
directions with components exactly -1, 0, -0 and 1; both strides.  One
mutation of the restatement (y and z swapped in morton3) must break the
equality, so the comparison is shown to see the bits.  And the sizes of the
call's chunk loop (tmpt_query_plan) up to 2^40 rays."""
import ctypes

import numpy as np
import pytest

import query_key_restate as Q
import ray_cases as R
import test_ray_cases as P
import toymeshpathtracer_amd as tm

f32 = np.float32
SCENES = ("soup272", "uniform_sheet", "translated_3e5", "scaled_1e-4")


def vertex_box(tris):
    v = np.asarray(tris, f32).reshape(-1, 3)
    return np.concatenate([v.min(0), v.max(0)]).astype(f32)


def special_rays(box, seed):
    """NaN and +-inf in each component, origins on both box faces, directions of exact -1, 0, -0, 1."""
    rng = np.random.default_rng(seed)
    lo, hi = box[:3].astype(np.float64), box[3:].astype(np.float64)
    n = 64
    base = np.concatenate([(lo + rng.random((n, 3)) * (hi - lo)), rng.normal(size=(n, 3))], 1)
    base[:, 3:] /= np.linalg.norm(base[:, 3:], axis=1, keepdims=True)
    base = base.astype(f32)
    out = []
    for comp in range(6):
        for val in (np.nan, np.inf, -np.inf):
            r = base[:8].copy()
            r[:, comp] = val
            out.append(r)
    for ax in range(3):  # exactly on the lower and the upper face, and one ulp either side
        for face in (box[ax], box[3 + ax]):
            for v in (face, np.nextafter(face, f32(-np.inf)), np.nextafter(face, f32(np.inf))):
                r = base[:8].copy()
                r[:, ax] = v
                out.append(r)
    for ax in range(3):
        for val in (f32(-1.0), f32(0.0), f32(-0.0), f32(1.0)):
            r = base[:8].copy()
            r[:, 3 + ax] = val
            out.append(r)
    grid = np.array(np.meshgrid(*[[-1.0, -0.0, 0.0, 1.0]] * 3), f32).reshape(3, -1).T  # all 64 sign / zero directions
    r = base[:64].copy()
    r[:, 3:] = grid
    out.append(r)
    return np.concatenate(out).astype(f32)


@pytest.fixture(scope="module", params=SCENES)
def scene_rays(request):
    tris = P.tris_of(request.param)
    box = vertex_box(tris)
    fam = dict(P.rays_of(request.param))
    fam["special"] = special_rays(box, 11)
    return request.param, box, fam


def test_keys_equal_the_restatement(scene_rays):
    name, box, fam = scene_rays
    if name == "uniform_sheet":
        assert (box[3:] - box[:3] == 0).sum() == 1  # the 1e-30 floor is exercised
    seen = set()
    for family, rays in fam.items():
        want = Q.keys(rays, box)
        got6 = tm.query_keys(rays, box)
        r8 = R.ranged(rays, P.SEED)
        got8 = tm.query_keys(r8, box)
        for got, stride in ((got6, 6), (got8, 8)):
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (f"{name} {family} stride {stride}: {bad.size} keys differ, first ray {bad[0]} "
                                   f"{rays[bad[0]]} hook {got[bad[0]]:#x} restated {want[bad[0]]:#x}")
        assert (want <= 0xFFFFFF).all()
        seen.update(np.unique(want).tolist())
    nan = np.isnan(fam["special"][:, :6]).any(1)
    assert nan.sum() == 48 and (tm.query_keys(fam["special"], box)[nan] == 0xFFFFFF).all()
    assert (tm.query_keys(fam["special"], box)[~nan] != 0xFFFFFF).all()  # +-inf is clamped, not flagged
    assert len(seen) > 500, len(seen)  # the rays spread over the key space


def test_the_comparison_sees_a_mutation(scene_rays):
    """y and z swapped in the restatement's morton3: the keys of rays inside the box must differ."""
    name, box, fam = scene_rays
    rays = np.concatenate([fam["axis"], fam["near_axis"]])
    got = tm.query_keys(rays, box)
    assert (got == Q.keys(rays, box)).all()
    differ = int((got != Q.keys(rays, box, swap_yz=True)).sum())
    assert differ > len(rays) // 4, (name, differ)


def test_key_fields():
    """The corners of the fields: cell 0 and 31 per axis, direction step 0 and 7, x lowest."""
    box = np.array([0, 0, 0, 32, 32, 32], f32)
    ray = lambda o, d: np.array([list(o) + list(d)], f32)  # noqa: E731
    k = lambda o, d: int(tm.query_keys(ray(o, d), box)[0])  # noqa: E731
    assert k((0, 0, 0), (-1, -1, -1)) == 0
    assert k((0, 0, 0), (1, -1, -1)) == 7 << 6 and k((0, 0, 0), (-1, 1, -1)) == 7 << 3 and k((0, 0, 0), (-1, -1, 1)) == 7
    assert k((1, 0, 0), (-1, -1, -1)) == 1 << 9 and k((0, 1, 0), (-1, -1, -1)) == 2 << 9
    assert k((0, 0, 1), (-1, -1, -1)) == 4 << 9 and k((2, 0, 0), (-1, -1, -1)) == 8 << 9
    assert k((31.5, 31.5, 31.5), (1, 1, 1)) == 0xFFFFFF  # every field at its top: all 24 bits
    assert k((1e30, 1e30, 1e30), (5, 5, 5)) == 0xFFFFFF and k((-1e30, -5, -0.0), (-7, -1.5, -1)) == 0
    assert k((0, 0, 0), (0, -0.0, 0.25)) == (4 << 6) | (4 << 3) | 5


def test_query_keys_argument_checks():
    fn = tm._sig("tmpt_query_keys", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p,
                                                   ctypes.c_void_p])
    rays, box, keys = np.zeros((4, 8), f32), np.zeros(6, f32), np.zeros(4, np.uint32)
    r, b, k = rays.ctypes.data, box.ctypes.data, keys.ctypes.data
    for args, msg in (((r, -1, 6, b, k), "n < 0"), ((None, 4, 6, b, k), "null rays or keys"),
                      ((r, 4, 6, b, None), "null rays or keys"), ((r, 4, 7, b, k), "stride is 6 or 8"),
                      ((r, 4, 0, b, k), "stride is 6 or 8"), ((r, 4, 8, None, k), "null box"),
                      ((None, -1, 7, None, None), "n < 0"), ((None, 4, 7, None, k), "null rays or keys"),
                      ((r, 4, 7, None, k), "stride is 6 or 8")):  # and the order between them
        assert fn(*args) == -22 and f"tmpt_query_keys: {msg}" in tm._last_error().decode(), (args, tm._last_error())
    assert fn(None, 0, 6, b, None) == 0 and fn(r, 4, 8, b, k) == 0
    with pytest.raises(ValueError):
        tm.query_keys(np.zeros((4, 7), f32), box)
    with pytest.raises(ValueError):
        tm.query_keys(rays, np.zeros(5, f32))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, (1 << 22) - 1, 1 << 22, (1 << 22) + 1, (1 << 31) + 5, (1 << 40) - 3, 1 << 40])
@pytest.mark.parametrize("chunk", [64, 128, 1000, 1 << 22])
def test_chunk_loop_sizes(n, chunk):
    """Sorted: chunks of `chunk` rays, the last partial, together exactly n; unsorted: one launch.
    The grid never exceeds what is resident, the cap or the chunk's blocks; the overflow
    stacks follow the grid (112 words per lane), the sort buffers the chunk."""
    resident = 1280
    p = tm.query_plan(n, True, chunk, 0, resident)
    assert p["chunks"] == -(-n // chunk) and p["chunk_n"] == min(n, chunk)
    assert (p["chunks"] - 1) * p["chunk_n"] + p["last_n"] == n and 1 <= p["last_n"] <= p["chunk_n"]
    assert p["grid"] == min(resident, -(-p["chunk_n"] // 256)) and p["chunk_n"] <= 1 << 22
    assert p["ovf_bytes"] == p["grid"] * 256 * 112 * 4
    assert p["sort_bytes"] >= 16 * p["chunk_n"] + 1024 and p["sort_bytes"] < 17 * p["chunk_n"] + 4096
    u = tm.query_plan(n, False, chunk, 0, resident)
    assert (u["chunks"], u["chunk_n"], u["last_n"], u["sort_bytes"]) == (1, n, n, 0)
    assert u["grid"] == min(resident, -(-n // 256))
    assert tm.query_plan(n, False, chunk, 1, resident)["grid"] == 1
    assert tm.query_plan(n, True, chunk, 3, resident)["grid"] == min(3, p["grid"])


def test_query_plan_argument_checks():
    assert tm.query_plan(0, True) == dict(chunks=0, chunk_n=0, last_n=0, grid=0, ovf_bytes=0, sort_bytes=0)
    for kw, msg in ((dict(n=-1), "n < 0"), (dict(n=5, sorted=2), "sorted"), (dict(n=5, chunk=63), "chunk"),
                    (dict(n=5, chunk=(1 << 22) + 1), "chunk"), (dict(n=5, grid_cap=-1), "grid_cap"),
                    (dict(n=5, resident=0), "resident")):
        a = dict(n=5, sorted=1)
        a.update(kw)
        with pytest.raises(tm.TmptError, match=msg):
            tm.query_plan(**a)
