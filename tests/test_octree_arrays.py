"""The octree as arrays, without a GPU: tmpt_octree_arrays' two methods and
the surface of both check hooks.

Method 0 is the host recursion tmpt_scene_build_octree runs by default; method
1 runs the passes of the device build (option octree_build=device;
csrc/tmpt_octree_build.h) as host loops -- the very functions the kernels
call, one loop per kernel: level-order lists, overlap counts, prefix sums,
bottom-up subtree sizes, top-down preorder indices.  So the relayout
arithmetic of the device build is proved here, on every adversarial family,
before and apart from any GPU run.

Tolerance: none.  Nodes, reference words, info and the grid's bits are equal
between the methods; the arrays' digest is tmpt_octree_digest's and the
oracle's; the leaf lists are the oracle's.
"""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
import ref_cases as C
import toymeshpathtracer_amd as tm
from conftest import ROOT

OBJ_FIXTURES = ("child_order", "grid", "samebox_fan150", "segments200")
DATA_SCENES = ("cube", "suzanne", "teapot")
TINY = (0, 1, 10, 11, 12)
DIGEST_WORDS = 120_000  # the FNV walk below is a Python loop: scenes up to this many words


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def tiny_scene(n):
    """n small triangles about one point (so that 11 of them split the root and
    some children keep more than one), and their root box."""
    rng = np.random.default_rng(1000 + n)
    c = rng.uniform(-1.0, 1.0, (n, 1, 3))
    t = (c + rng.uniform(-0.6, 0.6, (n, 3, 3))).astype(np.float32)
    lo, hi = tm.octree_bounds(np.full(3, -1.5, np.float32), np.full(3, 1.75, np.float32))
    return t, lo, hi


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (tris, root box min, root box max) of a named case."""
    if name.startswith("tiny"):
        return tiny_scene(int(name[4:]))
    if name in C.HIT_CASES and name not in OBJ_FIXTURES:
        fx = C.load_hits(name)
        return fx["tris"], fx["box"][:3].copy(), fx["box"][3:].copy()
    path = os.path.join(C.REF_DIR, name + ".obj") if name in OBJ_FIXTURES else os.path.join(ROOT, "data", name + ".obj")
    tris, bmin, bmax = tm.load_scene(path)
    lo, hi = tm.octree_bounds(bmin, bmax)
    return tris, lo, hi


CASES = tuple(f"tiny{n}" for n in TINY) + OBJ_FIXTURES + tuple(n for n in C.HIT_CASES if n not in OBJ_FIXTURES)
assert all(n in CASES for n in DATA_SCENES)


def same_octree(a, b):
    """-> what differs between two results of octree_arrays / dump_octree (empty: nothing)."""
    bad = []
    if a["info"] != b["info"]:
        bad.append(f"info {a['info']} != {b['info']}")
    for key in ("nodes", "refs", "grid"):
        x, y = _u32(a[key]), _u32(b[key])
        if x.shape != y.shape:
            bad.append(f"{key}: shape {x.shape} != {y.shape}")
        elif not np.array_equal(x, y):
            w = np.nonzero((x != y).reshape(len(x), -1).any(1))[0]
            bad.append(f"{key}: {w.size} rows differ, first {w[:5]}")
    return bad


def digest(arr):
    """tmpt_octree_digest's FNV-1a (csrc/tmpt_octree.cpp octree_digest) over the arrays."""
    nodes, refs = arr["nodes"], arr["refs"]
    words = []
    for nd in nodes:
        words += [int(nd[0]), int(nd[1]), int(nd[2]), int(nd[4]), int(nd[5]), int(nd[6])]
        r = int(np.int32(nd[7]))
        words.append(0 if r < 0 else 1)
        if r >= 0:
            words += [int(v) & 0xFFFFFFFF for v in refs[r:r + 1 + int(refs[r])]]
    h = 1469598103934665603
    for b in np.array(words, np.uint32).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def check_structure(arr):
    """The arrays are a preorder tree: skip links nest, leaves' lists lie back to back."""
    nodes, refs, info = arr["nodes"], arr["refs"], arr["info"]
    skip, ref = nodes[:, 3].astype(np.int64), nodes[:, 7].view(np.int32).astype(np.int64)
    n = len(nodes)
    assert info["nodes"] == n and skip[0] == n and (skip > np.arange(n)).all() and (skip <= n).all()
    leaf = ref >= 0
    assert (skip[leaf] == np.nonzero(leaf)[0] + 1).all() and int(leaf.sum()) == info["leaves"]
    counts = refs[ref[leaf]].astype(np.int64)
    assert np.array_equal(ref[leaf], np.concatenate([[0], np.cumsum(counts + 1)[:-1]]))
    assert info["refs"] == len(refs) == int((counts + 1).sum())


@pytest.mark.parametrize("name", CASES)
def test_level_passes_equal_the_recursion(name):
    """Method 1 equals method 0 word for word: nodes, refs, info, the grid's bits."""
    tris, lo, hi = scene(name)
    a, b = tm.octree_arrays(tris, lo, hi, 0), tm.octree_arrays(tris, lo, hi, 1)
    print(f"{name}: {a['info']}")
    bad = same_octree(b, a)
    assert not bad, "\n".join(bad)
    check_structure(a)
    d = tm.octree_digest(tris, lo, hi)
    assert (d["nodes"], d["leaves"], d["refs"], d["depth"]) == (a["info"]["nodes"], a["info"]["leaves"],
                                                                a["info"]["refs"] - a["info"]["leaves"], a["info"]["depth"])
    flags, grid13 = tm.octree_flags(tris, lo, hi, np.zeros((len(tris), 6), np.float32), np.ones(len(tris), np.float32),
                                    np.arange(len(tris), dtype=np.int32))
    assert int((flags & 1).sum()) == a["info"]["flat"]
    g = a["grid"]  # reach, drift, r0, 1/cell, cell, band  against  r0, 1/cell, cell, band, reach
    assert np.array_equal(_u32(np.concatenate([g[4:16], g[0:1]])), _u32(grid13))
    assert np.array_equal(_u32(g[1:4]), _u32(np.float32(2.0) * g[13:16]))


def test_tiny_cases_cover_the_first_split():
    """0, 1 and 10 triangles: a leaf root holding them all; 11 and 12: a split root."""
    for n in TINY:
        a = tm.octree_arrays(*scene(f"tiny{n}"), 1)
        if n <= 10:
            assert a["info"] == dict(nodes=1, leaves=1, refs=n + 1, depth=0, flat=a["info"]["flat"])
            assert list(a["refs"]) == [n] + list(range(n)) and int(np.int32(a["nodes"][0, 7])) == 0
        else:
            assert a["info"]["nodes"] >= 9 and a["info"]["depth"] >= 1 and int(a["nodes"][0, 7].view(np.int32)) == -1


@pytest.mark.parametrize("name", [n for n in CASES if not n.startswith("tiny")])
def test_digest_and_leaves_equal_the_oracle(name):
    """tmpt_octree_digest's value is the oracle octree's on every case; where the
    arrays are small enough for the FNV walk in Python (DIGEST_WORDS), their own
    digest is that value too, and every box and every leaf's list is the oracle's."""
    tris, lo, hi = scene(name)
    a = tm.octree_arrays(tris, lo, hi, 1)
    osc = _oracle_scene(name)
    boxes, _ = osc.octree_nodes()
    assert np.array_equal(_u32(boxes[0]), _u32(np.concatenate([lo, hi])))  # the same root box
    lib = tm.octree_digest(tris, lo, hi)["digest"]
    assert lib == osc.octree_digest() and len(boxes) == a["info"]["nodes"]
    if 7 * a["info"]["nodes"] + a["info"]["refs"] > DIGEST_WORDS:
        return
    assert digest(a) == lib
    order = oracle_preorder(osc)
    assert np.array_equal(np.concatenate([a["nodes"][:, 0:3], a["nodes"][:, 4:7]], 1), _u32(boxes[order]))
    ref = a["nodes"][:, 7].view(np.int32)
    for i in np.nonzero(ref >= 0)[0]:
        r = int(ref[i])
        assert np.array_equal(a["refs"][r + 1:r + 1 + int(a["refs"][r])], osc.octree_leaf(int(order[i]))), (name, i)


def oracle_preorder(osc):
    """The oracle's node numbers (its storage order) in depth-first preorder, children 0..7."""
    _, info = osc.octree_nodes()
    order, stack = [], [0]
    while stack:
        i = stack.pop()
        order.append(i)
        first = int(info[i, 0])
        if first >= 0:
            stack.extend(range(first + 7, first - 1, -1))
    return np.array(order, np.int64)


def _oracle_scene(name):
    """The oracle's octree of a case whose root box is main.cpp:312's box of known bounds."""
    if name in C.HIT_CASES and name not in OBJ_FIXTURES:
        fx = C.load_hits(name)
        return oracle.Scene(fx["tris"], accel=oracle.ACCEL_OCTREE, tie=oracle.TIE_VISIT, bmin=fx["bmin"], bmax=fx["bmax"])
    path = os.path.join(C.REF_DIR, name + ".obj")
    tris, bmin, bmax = oracle.load_scene(path)
    return oracle.Scene(tris, accel=oracle.ACCEL_OCTREE, tie=oracle.TIE_VISIT, bmin=bmin, bmax=bmax)


# ---------------------------------------------------------------- the hooks' surface
def _arrays_fn():
    return tm._sig("tmpt_octree_arrays", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                                        ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                        ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p])


def _dump_fn():
    return tm._sig("tmpt_scene_dump_octree", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                                            ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                            ctypes.c_void_p])


def test_entry_points_are_declared_and_exported():
    lib = ctypes.CDLL(tm.lib_path)
    out = subprocess.run(["nm", "-D", "--defined-only", tm.lib_path], capture_output=True, text=True).stdout
    header = open(os.path.join(ROOT, "include", "tmpt.h")).read()
    for sym in ("tmpt_scene_dump_octree", "tmpt_octree_arrays"):
        assert sym in tm.EXPORTS and hasattr(lib, sym)
        assert re.search(rf" T {sym}$", out, flags=re.M)
        assert re.search(rf"^int {sym}\(", header, flags=re.M)
    assert tm.abi_version() == 9  # additive: detected by symbol, the version stays
    assert "still 9, additive: the render options octree_build and octree_dev_max" in header
    for key in ("octree_build", "octree_dev_max"):
        assert re.search(rf"^ \*   {key} ", header, flags=re.M), key
    assert callable(tm.Scene.dump_octree) and callable(tm.octree_arrays)


def test_arrays_checks_in_order():
    tris, lo, hi = scene("tiny12")
    t = np.ascontiguousarray(tris.reshape(-1, 9))
    info, grid = np.zeros(5, np.int64), np.zeros(16, np.float32)
    nodes, refs = np.zeros((64, 8), np.uint32), np.zeros(256, np.int32)
    good = dict(tris=t.ctypes.data, n=len(t), lo=lo.ctypes.data, hi=hi.ctypes.data, method=1, nodes=nodes.ctypes.data,
                nw=nodes.size, refs=refs.ctypes.data, rw=refs.size, info=info.ctypes.data, grid=grid.ctypes.data)

    def call(**kw):
        a = dict(good, **kw)
        rc = _arrays_fn()(a["tris"], a["n"], a["lo"], a["hi"], a["method"], a["nodes"], a["nw"], a["refs"], a["rw"],
                          a["info"], a["grid"])
        return rc, tm._last_error().decode()

    # the header's order: each wrong argument with every later one wrong too
    chain = [(dict(n=-1), "n < 0"), (dict(tris=None), "null triangles"), (dict(lo=None), "null bounds"),
             (dict(method=2), "method"), (dict(info=None), "null info"), (dict(refs=None), "go together")]
    for i, (_, msg) in enumerate(chain):
        kw = {}
        for k, _ in chain[i:]:
            kw.update(k)
        if i == 0:
            kw.pop("tris")  # (n < 0 with triangles given: the first check alone decides)
        rc, err = call(**kw)
        assert rc == -22 and "tmpt_octree_arrays: " in err and msg in err, (i, msg, rc, err)
    for kw, msg in ((dict(hi=None), "null bounds"), (dict(method=-1), "method"), (dict(nodes=None), "go together"),
                    (dict(nw=8), "node buffer too small"), (dict(rw=3), "reference buffer too small")):
        rc, err = call(**kw)
        assert rc == -22 and msg in err, (kw, rc, err)
    rc, err = call(nw=8, rw=3)
    assert rc == -22 and "node buffer too small" in err
    # sizes alone, without a grid; then the arrays
    rc, _ = call(nodes=None, refs=None, nw=0, rw=0, grid=None)
    assert rc == 0 and info[0] >= 9 and info[2] > 0
    rc, _ = call(n=0, tris=None)
    assert rc == 0 and list(info[:4]) == [1, 1, 1, 0]
    rc, _ = call()
    want = tm.octree_arrays(tris, lo, hi, 0)
    assert rc == 0 and np.array_equal(nodes[:info[0]], want["nodes"]) and np.array_equal(refs[:info[2]], want["refs"])


def test_dump_checks_come_before_any_device_call():
    info = np.zeros(5, np.int64)
    buf = np.zeros(8, np.uint32)
    for args, msg in (((None, None, 0, None, 0, None, None), "null scene"),
                      ((None, buf.ctypes.data, 8, None, 0, None, None), "null scene")):
        rc = _dump_fn()(*args)
        assert rc == -22 and "tmpt_scene_dump_octree: " + msg in tm._last_error().decode()


def test_option_names():
    """octree_build takes host / device by name as tie_rule takes its names; both keys
    are unknown to nothing that parses options without a device."""
    h = ctypes.c_void_p()
    create = tm._sig("tmpt_scene_create_ex", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                                            ctypes.c_char_p, ctypes.c_void_p])
    for text, msg in ((b"octree_build=2", "out of range"), (b"octree_build=gpu", "bad value"),
                      (b"octree_build=0.5", "takes an integer"), (b"octree_dev_max=-1", "out of range")):
        rc = create(None, 0, 0, text, ctypes.byref(h))
        assert rc == -22 and msg in tm._last_error().decode(), (text, tm._last_error())


def test_cli_usage_mentions_octree():
    cli = os.path.join(os.path.dirname(tm.lib_path), "tmpt")
    r = subprocess.run([cli], capture_output=True, text=True)
    assert r.returncode == 1 and "--octree host|device" in r.stdout
    r = subprocess.run([cli, "8", "4", "1", os.path.join(ROOT, "data", "cube.obj"), "--octree", "gpu"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "invalid --octree argument" in r.stdout, r.stdout
