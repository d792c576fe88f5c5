"""The BVH checker (bvh_check.py) proved on the CPU: dumps encoded from a
median-split reference tree pass every rule, and each single mutation of a
clean dump produces a finding that names the rule it breaks.  Also here: the
restated link layout against the static_assert values of tmpt_internal.h.
No GPU and no library call: the hooks' argument checks are in test_abi.py.
"""
import copy
import functools

import numpy as np
import pytest

import bvh_check as B
import geometry_cases as G

CLEAN_SOUPS = (1, 2, 3, 5, 64, 300)
CLEAN_FAMILIES = ("flat_z", "translated_3e5", "scaled_1e-4", "anisotropic", "one_cell")


@functools.lru_cache(maxsize=None)
def _clean(name, leaf_max=2):
    tris = G.case(name)
    tris.setflags(write=False)
    return tris, B.reference_dump(tris, leaf_max)


@pytest.mark.parametrize("name", [G.sweep_name(n) for n in CLEAN_SOUPS] + list(CLEAN_FAMILIES))
@pytest.mark.parametrize("leaf_max", [2, 16])
def test_reference_trees_pass(name, leaf_max):
    tris, dump = _clean(name, leaf_max)
    bad = B.check(tris, dump, {"leaf_max": leaf_max}, pop_key=B.pop_key_bits(dump["info"]["link_bits"]), soa=dump)
    assert not bad, "\n".join(bad)
    assert np.array_equal(B.canonical(dump), dump["nodes"])  # the encoder numbers breadth-first already
    assert B.cost(dump, tris) > 0.0


def test_empty_scene():
    dump = B.reference_dump(np.zeros((0, 3, 3), np.float32))
    assert B.check(np.zeros((0, 3, 3), np.float32), dump) == []
    dump["tris"][0, 3] = 1
    assert any(b.startswith("tri-null") for b in B.check(np.zeros((0, 3, 3), np.float32), dump))


# ---------------------------------------------------------------- mutations
def _set_q(dump, node, plane, slot, value):
    w = int(dump["nodes"][node, 4 + plane])
    w = (w & ~(255 << (8 * slot))) | ((value & 255) << (8 * slot))
    dump["nodes"][node, 4 + plane] = w


def _leaf_slots(d):
    return np.argwhere(d.valid & d.leaf)


def _inner_slots(d):
    return np.argwhere(d.valid & ~d.leaf)


def m_qhi_minus(dump, d):
    # a hi face: every clean one lies less than a quantum outside its union, so one step in is inside it
    node, slot = np.argwhere(d.valid & (d.qhi[..., 0] >= 1))[-1]
    _set_q(dump, node, 1, slot, int(d.qhi[node, slot, 0]) - 1)


def m_qlo_plus(dump, d):
    # the lo face at q = 0 touches its union exactly: the origin is that child's minimum
    node, slot = np.argwhere(d.valid & (d.qlo[..., 1] == 0))[-1]
    _set_q(dump, node, 2, slot, 1)


def m_qhi_loose(dump, d):
    node, slot = np.argwhere(d.valid & (d.qhi[..., 2] <= 253))[0]
    _set_q(dump, node, 5, slot, int(d.qhi[node, slot, 2]) + 2)


def m_exp_plus(dump, d):
    dump["nodes"][0, 3] += 1 << 8  # ey + 1


def m_origin_ulp(dump, d):
    dump["nodes"][-1, 2] += 1


def m_count_plus(dump, d):
    node, slot = _leaf_slots(d)[0]
    dump["nodes"][node, 12 + slot] += 1 << dump["info"]["count_shift"]


def m_count_minus(dump, d):
    node, slot = np.argwhere(d.valid & d.leaf & (d.count >= 2))[0]
    dump["nodes"][node, 12 + slot] -= 1 << dump["info"]["count_shift"]


def m_first_plus(dump, d):
    node, slot = _leaf_slots(d)[1]
    dump["nodes"][node, 12 + slot] += 1


def m_swap_links(dump, d):
    ls = _leaf_slots(d)
    a = ls[0]
    b = next(x for x in ls if x[0] != a[0])
    n = dump["nodes"]
    n[a[0], 12 + a[1]], n[b[0], 12 + b[1]] = n[b[0], 12 + b[1]], n[a[0], 12 + a[1]]


def m_link_back(dump, d):
    node, slot = _inner_slots(d)[-1]
    dump["nodes"][node, 12 + slot] = node - 1 if node > 0 else 0


def m_dag(dump, d):
    ins = _inner_slots(d)
    a = ins[-1]
    b = next(x for x in ins[::-1] if d.link[tuple(x)] != d.link[tuple(a)])
    dump["nodes"][a[0], 12 + a[1]] = d.link[tuple(b)]  # two links to one node, none to the other


def m_mask(dump, d):
    dump["nodes"][0, 3] &= ~np.uint32(1 << 24)


def m_empty_box(dump, d):
    node, slot = np.argwhere(~d.valid)[0]
    _set_q(dump, node, 0, slot, 3)
    _set_q(dump, node, 1, slot, 9)


def m_stray_bit(dump, d):
    node, slot = _leaf_slots(d)[-1]
    dump["nodes"][node, 12 + slot] |= 1 << dump["info"]["link_bits"]


def m_e2z(dump, d):
    dump["tris"][dump["info"]["n"] // 2, 8] ^= 1


def m_swap_index(dump, d):
    t = dump["tris"]
    t[0, 9], t[1, 9] = t[1, 9], t[0, 9]


def m_null_record(dump, d):
    dump["tris"][dump["info"]["n"], 0] = 0x3F800000


def m_flat_bit(dump, d):
    dump["tris"][3, 9] |= 1


def m_depth(dump, d):
    dump["info"]["depth4"] += 1


MUTATIONS = [
    ("qhi-1", m_qhi_minus, "box-contain"), ("qlo+1", m_qlo_plus, "box-contain"), ("qhi+2", m_qhi_loose, "box-tight"),
    ("exponent+1", m_exp_plus, "box-exp"), ("origin+1ulp", m_origin_ulp, "box-origin"),
    ("count+1", m_count_plus, "leaf-partition"), ("count-1", m_count_minus, "leaf-partition"),
    ("first+1", m_first_plus, "leaf-partition"), ("links-swapped", m_swap_links, "box-"),
    ("link-to-earlier", m_link_back, "tree-order"), ("dag", m_dag, "tree-reach"), ("mask-bit", m_mask, "slot-mask"),
    ("empty-slot-box", m_empty_box, "slot-empty"), ("stray-link-bit", m_stray_bit, "link-bits"),
    ("e2.z+1ulp", m_e2z, "tri-bits"), ("index-words-swapped", m_swap_index, "tri-bits"),
    ("record-n", m_null_record, "tri-null"), ("flat-bit", m_flat_bit, "tri-flat"), ("info-depth4", m_depth, "tree-depth"),
]


@pytest.mark.parametrize("case", ["soup64", "soup300", "anisotropic"])
@pytest.mark.parametrize("mutation", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_each_mutation_is_caught(mutation, case):
    """No mutation is skipped: each applies to each of these cases (all have empty slots,
    leaves of two, inner links on two levels), or the test fails.  one_cell is not among
    them: its 502 triangles fill every slot of the reference tree."""
    _, mutate, rule = mutation
    tris, clean = _clean(case)
    dump = copy.deepcopy(clean)
    mutate(dump, B.Decoded(clean["nodes"], clean["info"]["count_shift"]))
    assert any((dump[k] != clean[k]).any() for k in ("nodes", "tris")) or dump["info"] != clean["info"]
    bad = B.check(tris, dump, {"leaf_max": 2})
    assert any(b.startswith(rule) for b in bad), f"expected a {rule} finding, got {bad}"


def test_soa_plane_word_is_caught():
    tris, clean = _clean("soup64")
    for key, at in (("nodes", (5, 13)), ("tris", (7, 4))):
        soa = copy.deepcopy(clean)
        soa[key][at] ^= 0x100
        bad = B.check(tris, clean, {"leaf_max": 2}, soa=soa)
        assert [b for b in bad if b.startswith("soa")] and all(b.startswith("soa") for b in bad), bad


def test_canonical_form_undoes_a_renumbering():
    """Two nodes of one level exchanged (records and the links to them): raw dumps differ,
    the checker still passes, the canonical forms are equal."""
    tris, clean = _clean("soup300")
    d = B.Decoded(clean["nodes"], clean["info"]["count_shift"])
    a, b = 2, 3  # both at depth 1 of a 300-triangle tree
    dump = copy.deepcopy(clean)
    dump["nodes"][[a, b]] = dump["nodes"][[b, a]]
    for node, slot in _inner_slots(d):
        if d.link[node, slot] in (a, b):
            dump["nodes"][b if node == a else a if node == b else node, 12 + slot] = a + b - d.link[node, slot]
    assert (dump["nodes"] != clean["nodes"]).any()
    assert B.check(tris, dump, {"leaf_max": 2}) == []
    assert np.array_equal(B.canonical(dump), B.canonical(clean))


# ---------------------------------------------------------------- restated layout
def test_link_layout_against_the_header_static_asserts():
    """The values tmpt_internal.h asserts at compile time (namespace link_checks)."""
    assert B.link_layout(66453, 2, 16700) == (17, 18)
    assert B.pop_key_bits(18) == 13 and B.pop_key_mask(13) == 0x7FFC0000
    assert B.pop_key_bits(18, 9) == 9 and B.pop_key_mask(9) == 0x7FC00000
    assert B.pop_key_bits(18, 0) == 0 and B.pop_key_bits(18, 8) == 0 and B.pop_key_mask(0) == 0
    assert B.link_layout(66453, 16, 9000)[1] == 21 and B.pop_key_bits(21) == 10
    assert B.link_layout(1 << 21, 2, 1 << 20)[1] == 23 and B.pop_key_bits(23) == 0
    assert B.link_layout(1 << 21, 1, 1 << 21)[1] == 22 and B.pop_key_bits(22) == 9
    assert B.pop_key_bits(B.link_layout(12, 2, 5)[1]) == 16 and B.pop_key_mask(16) == 0x7FFF8000
    assert B.link_layout(3, 1, 1000)[1] == 10
    assert B.link_layout((1 << 27) - 1, 16, 1 << 26)[1] == 31
    leaf = B.leaf_link(2, 66452, 17)
    assert leaf & ((1 << 17) - 1) == 66452 and ((leaf >> 17) & 15) + 1 == 2


def test_padded_box_is_float32_op_by_op():
    t = np.array([[[1.0, 2.0, 3.0], [1.5, 2.0, -3.0], [0.25, 2.0, 3e5]]], np.float32)
    lo, hi = B.tri_boxes(t)
    f = np.float32
    for a, (l, h) in enumerate(((0.25, 1.5), (2.0, 2.0), (-3.0, 3e5))):
        pad = f(f(f(1e-5) * f(max(abs(f(l)), abs(f(h))) + f(f(h) - f(l)))) + f(1e-30))
        assert lo[0, a] == f(f(l) - pad) and hi[0, a] == f(f(h) + pad)
    assert B.f32_units(np.array([1.0, -2.0 ** -149, 0.0, 2.0 ** -126], np.float32)).tolist() == [1 << 149, -1, 0, 1 << 23]
