"""The restated BVH build (bvh_build_restate.py) proved on the CPU.

(a) every restated dump of the device comparison's (case, options) pairs passes
    bvh_check.check, and no node extent of them lies on a boundary of the exponent
    rule (there the device's double-precision log2 could differ: the comparison in
    test_gpu_bvh_build_exact.py makes no exception for it);
(b) the stages against oracles written another way: PLOC's nearest neighbour against a
    double loop, the Karras tree against the recursive definition, the SAH collapse
    against the enumeration of every collapse, the keys against a loop over bits;
(c) every single-rule mutation of the restatement changes the canonical dump of a pair the
    GPU test runs -- so a device that departed from the rule would fail there.
"""
import functools
import itertools

import numpy as np
import pytest

import bvh_build_restate as R
import bvh_check as B
import geometry_cases as G

f32 = np.float32
PAIRS = R.pairs(G.NON_SWEEP)
CASES = list(dict.fromkeys(name for name, _ in PAIRS))


@functools.lru_cache(maxsize=None)
def _tris(name):
    t = R.case_tris(name)
    t.setflags(write=False)
    return t


# ---------------------------------------------------------------- (a)
def test_the_pairs_are_the_cases_and_options_asked_for():
    names = set(CASES)
    assert {f"soup{n}" for n in (3, 4, 5, 63, 64, 65, 255, 256, 257, 288, 1023, 1024, 1025, 4096)} <= names
    assert {R.REPLACED.get(f, f) for f in G.NON_SWEEP} <= names and {"suzanne", "teapot"} <= names
    small = [n for n in CASES if n not in R.LARGE]
    ids = [R.opt_id(o) for o in R.ALL_OPTIONS]
    assert len(ids) == 11
    have = {(n, R.opt_id(o)) for n, o in PAIRS}
    assert {(n, i) for n in small for i in ids} - have == R.TRIMMED
    for n in R.LARGE:
        assert {(n, i) for i in ("default", "builder=lbvh", "collapse=sah")} <= have


@pytest.mark.parametrize("name", CASES)
def test_restated_dumps_pass_the_checker(name):
    tris = _tris(name)
    for opts in [o for case, o in PAIRS if case == name]:
        dump = R.cached_build(name, tris, opts)
        bad = B.check(tris, dump, opts)
        assert not bad, f"{name} [{R.opt_id(opts)}]: " + "\n".join(bad[:5])
        assert np.array_equal(B.canonical(dump), dump["nodes"])  # numbered breadth-first already
        assert dump["near_exponent_boundary"] == 0, f"{name} [{R.opt_id(opts)}]: replace this case"
        lbvh = opts.get("builder") == "lbvh" or name == "nested200" or len(tris) == 1
        assert (dump["info"]["builder_iters"] == 0) == lbvh


def test_the_replaced_case_is_on_the_boundary():
    """Why translated_1e4 is not compared: extents of exactly 255 * 2^-9 or 255 * 2^-10."""
    tris = G.case("translated_1e4")
    assert sum(R.build(tris, o)["near_exponent_boundary"] for o in ({}, {"leaf_max": 1})) > 0


@pytest.mark.parametrize("n", [0, 1, 2])
def test_tiny_scenes(n):
    tris = G.soup(n, 11) if n else np.zeros((0, 3, 3), f32)
    for opts in ({}, {"leaf_max": 1}, {"collapse": "sah", "leaf_max": 1}, {"builder": "lbvh"}):
        dump = R.build(tris, opts)
        assert B.check(tris, dump, opts) == []
        want = {0: (0, 0), 1: (1, 1), 2: (1, 1)}[n]
        assert (dump["info"]["n_nodes4"], dump["info"]["depth4"]) == want
        assert dump["info"]["builder_iters"] == (1 if n == 2 and "builder" not in opts else 0)
    if n == 0:
        assert R.build(tris)["info"] == B.reference_dump(tris)["info"]


# ---------------------------------------------------------------- (b) keys
def test_keys_against_a_loop_over_bits():
    rng = np.random.default_rng(5)
    cent = rng.random((500, 3)).astype(f32) * f32(3.0) - f32(1.0)
    cent[:, 1] = f32(0.25)  # zero extent: 0.5 -> cell 512
    q = R.quantised(cent)
    lo, hi = cent.min(0), cent.max(0)
    for i in range(500):
        for a in (0, 2):
            x = f32(f32(cent[i, a] - lo[a]) / f32(hi[a] - lo[a]))
            assert q[i, a] == min(int(f32(x * f32(1024))), 1023)  # int(): truncation; x >= 0
        assert q[i, 1] == 512
    assert q[:, 0].max() == 1023 and q[:, 0].min() == 0  # x = 1 gives 1024, clamped
    keys = R.morton_keys(cent)
    for i in range(500):
        want = 0
        for b in range(10):
            for a in range(3):  # bit b of x lands above bit b of y above bit b of z
                want |= ((int(q[i, a]) >> b) & 1) << (3 * b + 2 - a)
        assert int(keys[i]) == want
    order = R.sorted_order(np.array([5, 1, 5, 1, 0], np.uint32))
    assert order.tolist() == [4, 1, 3, 0, 2]


# ---------------------------------------------------------------- (b) PLOC nearest neighbour
@functools.lru_cache(maxsize=None)
def _boxes(kind):
    rng = np.random.default_rng(17)
    if kind == "random":
        lo = rng.random((300, 3)).astype(f32)
        hi = lo + (rng.random((300, 3)) * 0.2).astype(f32)
    elif kind == "lattice":  # unit cubes at few lattice points: equal boxes and many equal union areas
        lo = rng.integers(0, 3, (300, 3)).astype(f32)
        hi = lo + f32(1.0)
    else:  # fewer clusters than the radius
        lo = rng.integers(0, 2, (7, 3)).astype(f32)
        hi = lo + f32(1.0)
    n = len(lo)
    area = [[None] * n for _ in range(n)]
    for i in range(n):
        for j in range(i):
            e = [f32(max(hi[i, a], hi[j, a]) - min(lo[i, a], lo[j, a])) for a in range(3)]
            area[i][j] = area[j][i] = f32(f32(f32(e[0] * e[1]) + f32(e[1] * e[2])) + f32(e[2] * e[0]))
    return lo, hi, area


@pytest.mark.parametrize("pair", [0, 1])
@pytest.mark.parametrize("r", [1, 4, 32, 256])
@pytest.mark.parametrize("kind", ["random", "lattice", "few"])
def test_ploc_neighbour_against_a_double_loop(kind, r, pair):
    lo, hi, area = _boxes(kind)
    n = len(lo)
    got = R.ploc_nn(lo, hi, r, pair)
    ties = 0
    for i in range(n):
        window = [j for j in range(max(0, i - r), min(n - 1, i + r) + 1) if j != i]
        rank = (lambda j: (area[i][j], i ^ j)) if pair else (lambda j: (area[i][j], j))
        want = min(window, key=rank)
        ties += sum(area[i][j] == area[i][want] for j in window) > 1
        assert got[i] == want, (i, int(got[i]), want)
    if kind == "lattice" and r >= 4:
        assert ties > n // 4  # the tie rule decides for many clusters here


# ---------------------------------------------------------------- (b) Karras
def _recursive_splits(big, a, b, out):
    """[a, b] of the sorted keys key * 2^32 + index splits below the highest bit in which its
    first and last key differ."""
    if a == b:
        return
    bit = (big[a] ^ big[b]).bit_length() - 1
    s = max(i for i in range(a, b + 1) if not (big[i] >> bit) & 1)
    out[(a, b)] = s
    _recursive_splits(big, a, s, out)
    _recursive_splits(big, s + 1, b, out)


@pytest.mark.parametrize("kind", ["runs", "equal", "distinct", "two", "three"])
def test_karras_against_the_recursive_definition(kind):
    rng = np.random.default_rng(23)
    keys = {"runs": np.sort(rng.choice(rng.integers(0, 1 << 30, 12), 300)),  # 12 values: runs of ~25 equal keys
            "equal": np.full(257, 12345), "distinct": np.sort(rng.choice(1 << 30, 300, replace=False)),
            "two": np.array([7, 7]), "three": np.array([0, 1 << 29, 1 << 29])}[kind].astype(np.uint32)
    n = len(keys)
    child, rng_ = R.karras(keys)
    want = {}
    _recursive_splits([(int(k) << 32) | i for i, k in enumerate(keys)], 0, n - 1, want)
    got = {}
    for i in range(n - 1):
        c0, c1 = child[i]
        s = ~c0 if c0 < 0 else c0  # the left child ends at the split, and is node `split` when internal
        assert (~c1 if c1 < 0 else c1) == s + 1
        got[tuple(rng_[i])] = s
        for c, (a, b) in ((c0, (rng_[i][0], s)), (c1, (s + 1, rng_[i][1]))):
            assert (a == b) if c < 0 else tuple(rng_[c]) == (a, b)
    assert rng_[0] == (0, n - 1) and got == want and len(got) == n - 1


# ---------------------------------------------------------------- (b) SAH collapse
def _random_tree(rng, k):
    """A random binary tree over k leaves (slots left to right) with random leaf boxes."""
    blo = rng.random((k, 3)).astype(f32)
    bhi = blo + (rng.random((k, 3)) * 0.5).astype(f32)
    child, rngs = [], []

    def make(a, b):
        if a == b:
            return ~a
        i = len(child)
        child.append(None)
        rngs.append((a, b))
        s = int(rng.integers(a, b))
        child[i] = (make(a, s), make(s + 1, b))
        return i

    root = make(0, k - 1)
    lo, hi = np.zeros((len(child), 3), f32), np.zeros((len(child), 3), f32)
    for i in reversed(range(len(child))):  # children are numbered after their parent
        bx = [(blo[~c], bhi[~c]) if c < 0 else (lo[c], hi[c]) for c in child[i]]
        lo[i], hi[i] = np.minimum(bx[0][0], bx[1][0]), np.maximum(bx[0][1], bx[1][1])
    return R.Tree(child, rngs, lo, hi, np.arange(k), root), blo, bhi


def _area64(lo, hi):
    e = np.asarray(hi, np.float64) - np.asarray(lo, np.float64)
    return e[0] * e[1] + e[1] * e[2] + e[2] * e[0]


def _least_cost(tree, blo, bhi, leaf_max, c_leaf, c_tri):
    """The least cost over every collapse, each enumerated: a wide node takes any 2..4 subtrees
    that partition its leaves; a subtree of <= leaf_max triangles may be a leaf."""

    def cuts(c):
        if c < 0:
            return [[c]]
        l, r = tree.child[c]
        return [[c]] + [a + b for a in cuts(l) for b in cuts(r) if len(a) + len(b) <= 4]

    @functools.lru_cache(maxsize=None)
    def best(c):
        if c < 0:
            return _area64(blo[~c], bhi[~c]) * (c_leaf + c_tri)
        an = _area64(tree.lo[c], tree.hi[c])
        found = [an * 1.0 + sum(best(x) for x in cut) for cut in cuts(c) if len(cut) >= 2]
        if tree.count(c) <= leaf_max:
            found.append(an * (c_leaf + c_tri * tree.count(c)))
        return min(found)

    return best(tree.root)


def _cost_of(out, n, c_leaf, c_tri):
    """The cost of a collapse as collapse() returns it, in float64 from the same boxes."""
    klo, khi, links, _ = out
    cs = B.bits_for(n)
    total = 0.0
    for node in range(len(links)):
        for k in range(4):
            if np.isfinite(klo[node][k][0]):
                a = _area64(klo[node][k], khi[node][k])
                leaf = links[node][k] >> 31
                total += a * (c_leaf + c_tri * (((links[node][k] >> cs) & 15) + 1)) if leaf else a
    if len(links) > 1 or np.isfinite(klo[0][1][0]):  # not the tree that is one leaf: the root node itself
        total +=_area64(np.min(klo[0], 0), np.max(khi[0], 0))
    return total


# The float32 programme against float64, with the same boxes and the float32 cost constants.
# A term is area * factor: the area (3 differences, 3 products of two of them, 2 sums) is within
# (1 + u)^5 of exact, u = 2^-24, the leaf factor c_leaf + c_tri * cnt within (1 + u)^2, their
# product adds one rounding: (1 + u)^8.  A collapse of <= 10 triangles has at most 10 leaves
# and 9 nodes, 19 terms, so at most 18 additions lie above a term: what the programme holds for
# a collapse is within (1 + u)^26 of its exact cost, and it keeps the least of what it holds
# (rounding is monotone).  So exact(chosen) <= exact(least) * ((1 + u) / (1 - u))^26, which is
# below 1 + 53 u.
SAH_BOUND = 53 * 2.0 ** -24


@pytest.mark.parametrize("costs", [(0.7, 0.5), (0.2, 2.0)])
@pytest.mark.parametrize("leaf_max", [1, 2, 4])
def test_sah_collapse_against_every_collapse(leaf_max, costs):
    rng = np.random.default_rng(31)
    c_leaf, c_tri = float(f32(costs[0])), float(f32(costs[1]))
    shapes = set()
    for k in itertools.chain(range(2, 11), [10] * 12):
        tree, blo, bhi = _random_tree(rng, k)
        out = R.collapse(tree, blo, bhi, k, leaf_max, costs)
        chosen = _cost_of(out, k, c_leaf, c_tri)
        least = _least_cost(tree, blo, bhi, leaf_max, c_leaf, c_tri)
        assert least * (1 - 1e-15) <= chosen <= least * (1 + SAH_BOUND), (k, chosen, least)
        greedy = _cost_of(R.collapse(tree, blo, bhi, k, leaf_max, None), k, c_leaf, c_tri)
        assert greedy >= least * (1 - 1e-15)
        shapes.add(greedy > least * (1 + SAH_BOUND))
    assert True in shapes  # the optimum is not what any collapse gives: the greedy one costs more


# ---------------------------------------------------------------- (c) mutations
# mutation -> the smallest (case, options) of the device comparison found to show it
KILLED_BY = {
    "key-axes-swapped": ("soup3", {}),
    "key-round": ("soup255", {}),
    "order-unstable": ("coincident3", {}),
    "delta-no-index": ("coincident3", {"builder": "lbvh"}),
    "window-short-low": ("soup4", {"ploc_radius": 1}),
    "window-short-high": ("soup65", {"ploc_radius": 4}),
    "window-block": ("soup257", {}),
    "tie-high": ("coincident3", {}),
    "rule1-never": ("points200", {}),
    "rule1-always": ("coincident17", {}),
    "merge-high": ("soup63", {}),
    "slots-right-first": ("soup3", {}),
    "open-first": ("soup4", {"leaf_max": 1}),
    "open-smallest": ("soup4", {"leaf_max": 1}),
    "open-tie-last": ("coincident17", {"builder": "lbvh"}),
    "open-right-in-slot": ("soup3", {"leaf_max": 1}),
    "sah-leaf-strict": ("sah_tie2", {"collapse": "sah"}),
    "sah-k4-last": ("points200", {"collapse": "sah"}),
    "sah-no-ctri": ("soup5", {"collapse": "sah"}),
    "fallback-order": ("coincident17", {}),
}
# Equal keys without the index term are no hierarchy at all (Karras's construction needs
# distinct keys): the mutated stage links a child out of range, and that is how it shows.
NO_TREE = ("delta-no-index",)
# x = 0 for a zero extent moves every key of the scene by one and the same constant in that
# axis's bits: neither the order nor any key XOR changes, so no dump can show it
# (test_zero_extent_value_cannot_show_in_a_dump).
EQUIVALENT = ("key-zero-extent-0",)


def test_the_table_covers_every_mutation():
    assert set(KILLED_BY) | set(EQUIVALENT) == set(R.MUTATIONS) and not set(KILLED_BY) & set(EQUIVALENT)
    have = {(n, R.opt_id(o)) for n, o in PAIRS}
    assert all((n, R.opt_id(o)) in have for n, o in KILLED_BY.values())


@pytest.mark.parametrize("mut", list(KILLED_BY))
def test_each_mutation_changes_a_compared_dump(mut):
    name, opts = KILLED_BY[mut]
    tris = _tris(name)
    clean = R.cached_build(name, tris, opts)
    try:
        dump = R.build(tris, opts, mut)
    except R.RestateError:
        assert mut in NO_TREE
        return
    assert mut not in NO_TREE
    assert B.check(tris, dump, opts) == []  # still a valid tree: only the comparison can tell
    assert (dump["nodes"].shape != clean["nodes"].shape or (dump["nodes"] != clean["nodes"]).any()
            or (dump["tris"] != clean["tris"]).any())


@pytest.mark.parametrize("name", ["flat_x", "flat_y", "flat_z", "collinear_centroids", "coincident17"])
def test_zero_extent_value_cannot_show_in_a_dump(name):
    tris = _tris(name)
    cent = R.centroids(tris)
    clean, mutated = R.morton_keys(cent), R.morton_keys(cent, "key-zero-extent-0")
    x = clean ^ mutated
    axes = np.nonzero(cent.max(0) - cent.min(0) == 0)[0]
    assert axes.size and (x == x[0]).all()
    assert int(x[0]) == sum(int(R.expand10(512)) << (2 - int(a)) for a in axes)  # the mutation is live
    assert np.array_equal(R.sorted_order(clean), R.sorted_order(mutated))
    for opts in ({}, {"builder": "lbvh"}):
        a, b = R.cached_build(name, tris, opts), R.build(tris, opts, "key-zero-extent-0")
        assert np.array_equal(a["nodes"], b["nodes"]) and np.array_equal(a["tris"], b["tris"])
