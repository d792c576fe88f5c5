"""The device-built BVH against the build restated on the host, word for word.

test_gpu_bvh_structure.py proves every build valid; which valid tree the
builder must produce -- the key's bit order, PLOC's window and ties, the order of
the survivors and of the leaf slots, which child the collapse opens, the SAH
optimum -- is pinned here: for every (case, options) of bvh_build_restate.pairs
the dump of tm.Scene equals bvh_build_restate.build() in info, in the triangle
records raw, and in all 16 words of every node once the device's nodes are
renumbered breadth-first (bvh_check.canonical; the numbering within a level is
the build's one nondeterminism).  No tolerance and no exception: that no node
extent of these cases sits on an exponent boundary, where the device's
double-precision log2 could differ, is asserted on the CPU
(test_bvh_build_restate.py), which also proves the restatement stage by stage and
shows, by mutation, that each rule changes a dump compared here.
"""
import numpy as np
import pytest

import bvh_build_restate as R
import bvh_check as B
import geometry_cases as G
import toymeshpathtracer_amd as tm

pytestmark = pytest.mark.gpu

INFO_KEYS = ("n", "n_nodes4", "depth4", "builder_iters", "leaf_max", "count_shift", "link_bits")
PAIRS = R.pairs(G.NON_SWEEP)
CASES = list(dict.fromkeys(name for name, _ in PAIRS))


def _slots(nodes, i, cs):
    d = B.Decoded(nodes[i:i + 1], cs)
    out = [f"origin {d.origin[0].tolist()} exp {d.exp[0].tolist()} mask {int(d.mask[0]):#x}"]
    for k in range(4):
        kind = "empty" if not d.valid[0, k] else (f"leaf first {d.first[0, k]} count {d.count[0, k]}" if d.leaf[0, k]
                                                  else f"node {d.link[0, k]}")
        out.append(f"  slot {k}: {kind} qlo {d.qlo[0, k].tolist()} qhi {d.qhi[0, k].tolist()}")
    return "\n".join(out)


def compare(dump, want):
    """-> what differs between a device dump and the restated one (empty: nothing)."""
    bad = []
    got_info = {k: dump["info"][k] for k in INFO_KEYS}
    want_info = {k: want["info"][k] for k in INFO_KEYS}
    if got_info != want_info:
        bad.append(f"info: device {got_info}, restated {want_info}")
    a, b = np.asarray(dump["tris"], np.uint32), np.asarray(want["tris"], np.uint32)
    if a.shape != b.shape:
        bad.append(f"tris: {a.shape} on the device, {b.shape} restated")
    elif (a != b).any():
        at = np.argwhere(a != b)[0]
        bad.append(f"tris: record {at[0]} word {at[1]} is {a[tuple(at)]:#x} on the device (triangle {a[at[0], 9] >> 1}), "
                   f"{b[tuple(at)]:#x} restated (triangle {b[at[0], 9] >> 1}); {int((a != b).any(1).sum())} records differ")
    try:
        a = B.canonical(dump)
    except ValueError as e:
        return bad + [str(e)]
    b = want["nodes"]
    if a.shape != b.shape:
        bad.append(f"nodes: {a.shape[0]} on the device, {b.shape[0]} restated")
    rows = min(a.shape[0], b.shape[0])
    diff = (a[:rows] != b[:rows]).any(1)
    if diff.any():
        i = int(np.argmax(diff))
        words = np.nonzero(a[i] != b[i])[0].tolist()
        bad.append(f"nodes: {int(diff.sum())} of {rows} differ, first node {i} (canonical numbering) in words {words}\n"
                   f" device   {_slots(a, i, dump['info']['count_shift'])}\n"
                   f" restated {_slots(b, i, want['info']['count_shift'])}")
    return bad


@pytest.mark.parametrize("name", CASES)
def test_device_build_equals_the_restated_build(gpu, name):
    tris = R.case_tris(name)
    bad = []
    for opts in [o for case, o in PAIRS if case == name]:
        want = R.cached_build(name, tris, opts)
        with tm.Scene(tris, options=opts or None) as sc:
            dump = sc.dump_bvh()
        bad += [f"{name} [{R.opt_id(opts)}]: {b}" for b in compare(dump, want)]
        i = dump["info"]
        print(f"{name} [{R.opt_id(opts)}]: n {i['n']} nodes {i['n_nodes4']} depth {i['depth4']} "
              f"builder_iters {i['builder_iters']}")
    assert not bad, "\n".join(bad[:12])


@pytest.mark.parametrize("n", [0, 1, 2])
@pytest.mark.parametrize("opts", [{}, {"leaf_max": 1}, {"collapse": "sah", "leaf_max": 1}, {"builder": "lbvh"}],
                         ids=R.opt_id)
def test_tiny_scenes(gpu, opts, n):
    """The control flow of n = 0, 1, 2: no node; one leaf under one node; one PLOC pass."""
    tris = G.soup(n, 11) if n else np.zeros((0, 3, 3), np.float32)
    with tm.Scene(tris, options=opts or None) as sc:
        dump = sc.dump_bvh()
    bad = compare(dump, R.build(tris, opts))
    assert not bad, "\n".join(bad)
