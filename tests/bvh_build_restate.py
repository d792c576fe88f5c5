"""The BVH build (tmpt_bvh.hip) restated on the host, one function per stage.

Plain numpy and Python: float32 with one rounding per operation, in the device's
order of operations (the device code is built without contraction, with a
correctly rounded divide and without flushing denormals).  ``build(tris, opts)``
returns a dump of the form Scene.dump_bvh() gives, its nodes numbered
breadth-first in child-slot order -- the form ``bvh_check.canonical`` puts a device
dump into -- so the two can be compared word for word
(test_gpu_bvh_build_exact.py).  No stage calls the GPU library or the oracle.
The rules, from DESIGN.md section 4 and the kernels' comments:

leaf boxes   bvh_check.tri_boxes; centroid = 0.5f * (lo + hi) of the unpadded
             min / max; centroid bounds = their exact min / max
keys         per axis x = ext > 0 ? (c - lo) / ext : 0.5, q = min(max(x * 1024, 0), 1023)
             truncated; key = expand10(qx) << 2 | expand10(qy) << 1 | expand10(qz)
order        a stable sort of (key, index)
Karras       delta = clz(key XOR), 32 + clz(i ^ j) for equal keys, -1 outside the
             array; boxes refitted bottom-up with min / max
PLOC         window max(0, i - r) .. min(N - 1, i + r); half area (dx dy + dy dz) + dz dx
             of the float32 union; rule 0: the lowest index among equal areas; rule 1:
             the least i ^ j among them; mutual pairs merge into the lower position, the
             survivors keep their order; until one cluster is left; then the leaves are
             renumbered top-down, the left subtree's slots first
greedy       from the two children, while fewer than 4: open the internal candidate of
             more than leaf_max triangles with the largest box area (strict >, the
             first wins a tie); its left child takes its slot, its right is appended
SAH          k_sah_level's float32 dynamic programme and sah_expand's order of roots
control      n = 0, 1, 2; builder=lbvh; PLOC rule 0; 3 * depth4 + 1 > 128: rule 1; still
             too deep: the Karras tree and builder_iters = 0
encoding     bvh_check.encode_nodes, the encoder of bvh_check.reference_dump

``mut`` names one single-rule mutation (MUTATIONS) for test_bvh_build_restate.py:
the comparison with the device is worth what those mutations change.
"""
import numpy as np

import bvh_check as B

f32 = np.float32
DEFAULTS = {"builder": "ploc", "leaf_max": 2, "collapse": "greedy", "sah_c_leaf": 0.7, "sah_c_tri": 0.5,
            "ploc_radius": 32}
BLOCK = 256

MUTATIONS = {
    "key-axes-swapped": "x and y exchanged in the key",
    "key-round": "q rounded to nearest where the rule truncates",
    "key-zero-extent-0": "ext == 0 gives x = 0, not 0.5",
    "order-unstable": "equal keys in descending index order",
    "delta-no-index": "equal keys: delta = 32, without clz(i ^ j)",
    "window-short-low": "window i - r + 1 .. i + r",
    "window-short-high": "window i - r .. i + r - 1",
    "window-block": "window clipped at multiples of 256",
    "tie-high": "rule 0 keeps the highest index among equal areas",
    "rule1-never": "a PLOC tree too deep goes straight to the Karras tree",
    "rule1-always": "PLOC rule 1 from the first build on",
    "merge-high": "a mutual pair merges into the higher position",
    "slots-right-first": "the right subtree's slots come first",
    "open-first": "the greedy collapse opens the first eligible child",
    "open-smallest": "the greedy collapse opens the smallest child",
    "open-tie-last": "the greedy collapse gives a tie in area to the last child",
    "open-right-in-slot": "the opened child's right takes its slot, its left is appended",
    "sah-leaf-strict": "the DP takes a leaf on cl < ci",
    "sah-k4-last": "k4 takes the last minimum",
    "sah-no-ctri": "c_tri taken as 0",
    "fallback-order": "PLOC rule 1 is tried before rule 0",
}


class RestateError(Exception):
    """The stages did not give a tree (only a mutation does that)."""


# ---------------------------------------------------------------- leaves, keys, order
def centroids(tris):
    """-> float32 [n, 3]: 0.5f * (lo + hi) of the unpadded vertex min / max."""
    t = np.asarray(tris, f32).reshape(-1, 3, 3)
    return f32(0.5) * (t.min(1) + t.max(1))


def expand10(v):
    """The device's expand10: the products are taken modulo 2^32 (the masks do that here)."""
    v = np.asarray(v, np.uint64)
    for mul, mask in ((0x00010001, 0xFF0000FF), (0x00000101, 0x0F00F00F), (0x00000011, 0xC30C30C3),
                      (0x00000005, 0x49249249)):
        v = (v * np.uint64(mul)) & np.uint64(mask)
    return v.astype(np.uint32)


def quantised(cent, mut=None):
    """-> uint32 [n, 3]: the 10-bit cell of every centroid per axis."""
    cent = np.asarray(cent, f32)
    lo, hi = cent.min(0), cent.max(0)
    ext = hi - lo
    pos = ext > 0
    with np.errstate(all="ignore"):
        x = (cent - lo) / np.where(pos, ext, f32(1))
    x = np.where(pos, x, f32(0.0 if mut == "key-zero-extent-0" else 0.5))
    q = np.minimum(np.maximum(x * f32(1024), f32(0)), f32(1023))
    assert q.dtype == f32
    if mut == "key-round":
        q = np.minimum(np.floor(q + f32(0.5)), f32(1023))
    return q.astype(np.uint32)  # truncation


def morton_keys(cent, mut=None):
    q = quantised(cent, mut)
    if mut == "key-axes-swapped":
        q = q[:, [1, 0, 2]]
    return (expand10(q[:, 0]) << np.uint32(2)) | (expand10(q[:, 1]) << np.uint32(1)) | expand10(q[:, 2])


def sorted_order(keys, mut=None):
    """-> int64 [n]: the triangle index at every sorted slot (stable in the index)."""
    keys = np.asarray(keys, np.uint32)
    if mut == "order-unstable":
        return np.lexsort((-np.arange(len(keys)), keys))
    return np.argsort(keys, kind="stable")


# ---------------------------------------------------------------- binary trees
class Tree:
    """A binary tree over sorted slots.  child [m][2]: >= 0 an internal node, < 0 the leaf
    ~slot; range [m][2] the slots a node covers (inclusive); lo / hi float32 [m, 3] its box;
    vals [n] the triangle at every slot; root (for n = 1: ~0, with no internal node)."""

    def __init__(self, child, rng, lo, hi, vals, root, passes=0):
        self.child, self.range, self.lo, self.hi = child, rng, lo, hi
        self.vals, self.root, self.passes = np.asarray(vals, np.int64), root, passes

    def count(self, c):
        return 1 if c < 0 else self.range[c][1] - self.range[c][0] + 1


def _postorder(child, root, n):
    """Internal nodes, children before parents; RestateError unless it is a tree over n leaves."""
    m = len(child)
    seen_n, seen_l = [False] * m, [False] * n
    order, stack = [], [(root, False)]
    while stack:
        c, done = stack.pop()
        if done:
            order.append(c)
            continue
        if not -n <= c < m:
            raise RestateError(f"child {c} is out of range")
        if c < 0:
            if seen_l[~c]:
                raise RestateError(f"leaf {~c} reached twice")
            seen_l[~c] = True
            continue
        if seen_n[c]:
            raise RestateError(f"node {c} reached twice")
        seen_n[c] = True
        stack.append((c, True))
        stack.append((child[c][1], False))
        stack.append((child[c][0], False))
    if not (all(seen_l) and len(order) == max(n - 1, 0)):
        raise RestateError("not every leaf and node is reached")
    return order


def _clz32(x):
    return 32 - int(x).bit_length()


def karras(keys, mut=None):
    """Karras 2012, Fig. 4, over sorted keys -> (child, range) of the n - 1 internal nodes, root 0."""
    k = [int(v) for v in keys]
    n = len(k)

    def delta(i, j):
        if j < 0 or j > n - 1:
            return -1
        if k[i] == k[j]:
            return 32 if mut == "delta-no-index" else 32 + _clz32(i ^ j)
        return _clz32(k[i] ^ k[j])

    child, rng = [], []
    for i in range(n - 1):
        d = 1 if delta(i, i + 1) - delta(i, i - 1) >= 0 else -1
        dmin = delta(i, i - d)
        lmax = 2
        while delta(i, i + lmax * d) > dmin:
            lmax *= 2
        l, t = 0, lmax >> 1
        while t >= 1:
            if delta(i, i + (l + t) * d) > dmin:
                l += t
            t >>= 1
        j = i + l * d
        dnode = delta(i, j)
        s, t = 0, l
        while True:
            t = (t + 1) >> 1
            if delta(i, i + (s + t) * d) > dnode:
                s += t
            if t <= 1:
                break
        gamma = i + s * d + min(d, 0)
        lo, hi = min(i, j), max(i, j)
        child.append((~gamma if lo == gamma else gamma, ~(gamma + 1) if hi == gamma + 1 else gamma + 1))
        rng.append((lo, hi))
    return child, rng


def karras_tree(keys, order, blo, bhi, mut=None):
    """The Karras hierarchy with its boxes refitted bottom-up (min / max of the two children)."""
    n = len(keys)
    child, rng = karras(keys, mut)
    lo, hi = np.zeros((n - 1, 3), f32), np.zeros((n - 1, 3), f32)
    box = lambda c: (blo[order[~c]], bhi[order[~c]]) if c < 0 else (lo[c], hi[c])
    for c in _postorder(child, 0, n):
        (al, ah), (bl, bh) = box(child[c][0]), box(child[c][1])
        lo[c], hi[c] = np.minimum(al, bl), np.maximum(ah, bh)
    return Tree(child, rng, lo, hi, order, 0)


# ---------------------------------------------------------------- PLOC
def half_area(lo, hi):
    e = hi - lo
    return (e[..., 0] * e[..., 1] + e[..., 1] * e[..., 2]) + e[..., 2] * e[..., 0]


def ploc_nn(lo, hi, r, pair, mut=None):
    """-> int64 [N]: every cluster's nearest neighbour within the window, by the half area
    of the float32 union.  lo / hi float32 [N, 3] in position order."""
    N = lo.shape[0]
    w = min(r, N - 1)
    i = np.arange(N)[:, None]
    d = np.arange(-w, w + 1)[None, :]
    j = i + d
    ok = (j >= 0) & (j < N) & (d != 0)
    if mut == "window-short-low":
        ok &= d > -r
    if mut == "window-short-high":
        ok &= d < r
    if mut == "window-block":
        ok &= (j // BLOCK) == (i // BLOCK)
    jc = np.clip(j, 0, N - 1)
    with np.errstate(all="ignore"):
        area = half_area(np.minimum(lo[:, None, :], lo[jc]), np.maximum(hi[:, None, :], hi[jc]))
    assert area.dtype == f32
    area = np.where(ok, area, f32(np.inf))
    tie = ok & (area == area.min(1)[:, None])
    if pair:
        at = np.where(tie, i ^ jc, np.iinfo(np.int64).max).argmin(1)
    elif mut == "tie-high":
        at = tie.shape[1] - 1 - tie[:, ::-1].argmax(1)
    else:
        at = tie.argmax(1)  # ascending j, strict <: the lowest index among equal areas
    return np.arange(N) + d[0, at]


def ploc_tree(order, blo, bhi, r, pair, mut=None):
    """PLOC over the sorted leaves -> Tree, its leaves renumbered top-down."""
    n = len(order)
    lo, hi = blo[order].copy(), bhi[order].copy()
    cid = [~s for s in range(n)]
    child, size, nlo, nhi = [], [], [], []
    passes = 0
    while len(cid) > 1:
        N = len(cid)
        nn = ploc_nn(lo, hi, r, pair, mut)
        at = np.arange(N)
        mutual = nn[nn] == at
        first = np.nonzero(mutual & (at < nn))[0]
        if first.size == 0:
            raise RestateError("PLOC made no progress")
        keep = np.ones(N, bool)
        for a in first:
            b = int(nn[a])
            c0, c1 = cid[a], cid[b]
            child.append((c0, c1))
            size.append((1 if c0 < 0 else size[c0]) + (1 if c1 < 0 else size[c1]))
            ul, uh = np.minimum(lo[a], lo[b]), np.maximum(hi[a], hi[b])
            nlo.append(ul)
            nhi.append(uh)
            at_pos, gone = (b, a) if mut == "merge-high" else (a, b)
            cid[at_pos], lo[at_pos], hi[at_pos] = len(child) - 1, ul, uh
            keep[gone] = False
        cid = [c for c, k in zip(cid, keep) if k]
        lo, hi = lo[keep], hi[keep]
        passes += 1
    root = cid[0]
    # top-down leaf renumbering: a subtree covers one contiguous slot range
    off = [0] * len(child)
    new_slot = np.zeros(n, np.int64)
    stack = [root]
    while stack:
        k = stack.pop()
        c0, c1 = child[k]
        s0, s1 = (1 if c0 < 0 else size[c0]), (1 if c1 < 0 else size[c1])
        o0, o1 = (off[k] + s1, off[k]) if mut == "slots-right-first" else (off[k], off[k] + s0)
        for c, o in ((c0, o0), (c1, o1)):
            if c < 0:
                new_slot[~c] = o
            else:
                off[c] = o
                stack.append(c)
    relabel = lambda c: ~int(new_slot[~c]) if c < 0 else c
    child = [(relabel(a), relabel(b)) for a, b in child]
    rng = [(off[k], off[k] + size[k] - 1) for k in range(len(child))]
    vals = np.zeros(n, np.int64)
    vals[new_slot] = order
    return Tree(child, rng, np.array(nlo, f32).reshape(-1, 3), np.array(nhi, f32).reshape(-1, 3), vals, root, passes)


# ---------------------------------------------------------------- collapse
def box_area(lo, hi):
    dx, dy, dz = hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]
    return (dx * dy + dy * dz) + dz * dx


def sah_dp(tree, blo, bhi, leaf_max, c_leaf, c_tri, mut=None):
    """k_sah_level over every internal node -> (F [m][5] float32, dec [m]).  dec: bit 0 a leaf,
    bits 1..2 k4, bits 3.. the split bk of the forests of 2, 3, 4 roots."""
    c_leaf, c_tri = f32(c_leaf), f32(0.0 if mut == "sah-no-ctri" else c_tri)
    inf = f32(np.inf)
    m = len(tree.child)
    F, dec = [None] * m, [0] * m

    def child_f(c):
        if c < 0:
            t = tree.vals[~c]
            v = box_area(blo[t], bhi[t]) * (c_leaf + c_tri)
            return [None, v, v, v, v]
        return F[c]

    with np.errstate(all="ignore"):
        for nd in _postorder(tree.child, tree.root, len(tree.vals)):
            fl, fr = child_f(tree.child[nd][0]), child_f(tree.child[nd][1])
            an = box_area(tree.lo[nd], tree.hi[nd])
            cnt = tree.count(nd)
            best4, k4 = inf, 1
            for k in (1, 2, 3):
                v = fl[k] + fr[4 - k]
                if v <= best4 if mut == "sah-k4-last" else v < best4:
                    best4, k4 = v, k
            ci = an * f32(1.0) + best4
            cl = an * (c_leaf + c_tri * f32(cnt)) if cnt <= leaf_max else inf
            f = [None] * 5
            d = 0
            if cl < ci if mut == "sah-leaf-strict" else cl <= ci:
                f[1] = cl
                d |= 1
            else:
                f[1] = ci
            d |= k4 << 1
            for j in (2, 3, 4):
                bs, bk = f[j - 1], 0
                for k in range(1, j):
                    v = fl[k] + fr[j - k]
                    if v < bs:
                        bs, bk = v, k
                f[j] = bs
                d |= bk << (3 + 2 * (j - 2))
            assert all(type(v) is f32 for v in f[1:])
            F[nd], dec[nd] = f, d
    return F, dec


def sah_expand(tree, dec, c, j):
    """The roots of c's forest of at most j roots, left to right."""
    if c < 0 or j == 1:
        return [c]
    k = (dec[c] >> (3 + 2 * (j - 2))) & 3
    if k == 0:
        return sah_expand(tree, dec, c, j - 1)
    return sah_expand(tree, dec, tree.child[c][0], k) + sah_expand(tree, dec, tree.child[c][1], j - k)


def greedy_children(tree, src, leaf_max, mut=None):
    cand = list(tree.child[src])
    while len(cand) < 4:
        best, best_a = -1, f32(np.inf if mut == "open-smallest" else -1.0)
        for k, c in enumerate(cand):
            if c >= 0 and tree.count(c) > leaf_max:
                a = box_area(tree.lo[c], tree.hi[c])
                if mut == "open-first":
                    better = best < 0
                elif mut == "open-smallest":
                    better = a < best_a
                elif mut == "open-tie-last":
                    better = a >= best_a
                else:
                    better = a > best_a
                if better:
                    best, best_a = k, a
        if best < 0:
            break
        l, r = tree.child[cand[best]]
        if mut == "open-right-in-slot":
            l, r = r, l
        cand[best] = l
        cand.append(r)
    return cand


def collapse(tree, blo, bhi, n, leaf_max, sah=None, mut=None):
    """The top-down collapse to 4-wide, level by level, the nodes numbered breadth-first in
    slot order -> (klo, khi, links, depth4), or None: too deep for the traversal stack
    (3 * levels + 1 > 128, decided as the device decides it, after each level)."""
    cs = B.bits_for(n)
    dec = None
    if sah is not None and n >= 2:
        dec = sah_dp(tree, blo, bhi, leaf_max, sah[0], sah[1], mut)[1]

    def is_leaf(c):
        return c < 0 or ((dec[c] & 1) != 0 if dec is not None else tree.count(c) <= leaf_max)

    def box(c):
        return (blo[tree.vals[~c]], bhi[tree.vals[~c]]) if c < 0 else (tree.lo[c], tree.hi[c])

    inf3 = np.full(3, np.inf, f32)
    klo, khi, links = [], [], []
    level, total, levels = [tree.root], 1, 0
    while level:
        nxt = []
        for src in level:
            if is_leaf(src):
                cand = [src]
            elif dec is not None:
                k4 = (dec[src] >> 1) & 3
                cand = sah_expand(tree, dec, tree.child[src][0], k4) + sah_expand(tree, dec, tree.child[src][1], 4 - k4)
            else:
                cand = greedy_children(tree, src, leaf_max, mut)
            row = []
            for c in cand:
                if c < 0:
                    row.append(B.leaf_link(1, ~c, cs))
                elif is_leaf(c):
                    row.append(B.leaf_link(tree.count(c), tree.range[c][0], cs))
                else:
                    row.append(total)
                    total += 1
                    nxt.append(c)
            pad = 4 - len(cand)
            bx = [box(c) for c in cand]
            klo.append([b[0] for b in bx] + [inf3] * pad)
            khi.append([b[1] for b in bx] + [-inf3] * pad)
            links.append(row + [0x80000000 | n] * pad)
        levels += 1
        level = nxt
        if 3 * levels + 1 > B.STACK_TOTAL:
            return None
    return klo, khi, links, levels


def near_exponent_boundary(klo, khi):
    """How many node extents lie within 2^-40 relative of a boundary 255 * 2^k of the
    exponent rule: there the device's double-precision log2 may give either neighbour."""
    lo, hi = np.array(klo, f32).min(1), np.array(khi, f32).max(1)
    count = 0
    for x in (B.f32_units(hi) - B.f32_units(lo)).ravel():
        x = max(int(x), B._EXT_FLOOR)
        for s in range(max(0, x.bit_length() - 9), x.bit_length() - 6):
            if abs(x - (255 << s)) << 40 <= (255 << s):
                count += 1
                break
    return count


# ---------------------------------------------------------------- the whole build
def options(opts):
    o = dict(DEFAULTS)
    for k, v in (opts or {}).items():
        if k != "layout":
            if k not in o:
                raise KeyError(k)
            o[k] = v
    return o


_ploc_memo = {}


def _ploc_tree_once(tris, order, blo, bhi, r, pair, mut):
    """ploc_tree, kept for the last few inputs: the binary tree does not depend on leaf_max
    or the collapse, so the option sets of one case share it (nothing changes a Tree)."""
    key = (tris.tobytes(), r, pair, mut)
    if key not in _ploc_memo:
        if len(_ploc_memo) >= 8:
            _ploc_memo.clear()
        _ploc_memo[key] = ploc_tree(order, blo, bhi, r, pair, mut)
    return _ploc_memo[key]


def build(tris, opts=None, mut=None):
    """-> {"nodes", "tris", "info"} as Scene.dump_bvh() gives them, the nodes in canonical
    numbering; and "near_exponent_boundary", the count near_exponent_boundary() gives."""
    o = options(opts)
    tris = np.asarray(tris, f32).reshape(-1, 3, 3)
    n = tris.shape[0]
    leaf_max = int(o["leaf_max"])
    rec = np.zeros((n + 1, 12), np.uint32)
    if n == 0:
        info = {"n": 0, "n_nodes4": 0, "depth4": 0, "leaf_max": 0, "count_shift": 0, "link_bits": 31,
                "builder_iters": 0, "soa": 0}
        return {"nodes": np.zeros((0, 16), np.uint32), "tris": rec, "info": info, "near_exponent_boundary": 0}
    blo, bhi = B.tri_boxes(tris)
    keys = morton_keys(centroids(tris), mut)
    order = sorted_order(keys, mut)
    skeys = keys[order]
    sah = (o["sah_c_leaf"], o["sah_c_tri"]) if o["collapse"] in ("sah", 1) else None
    iters = 0
    if n == 1:
        tree = Tree([], [], np.zeros((0, 3), f32), np.zeros((0, 3), f32), order, ~0)
        out = collapse(tree, blo, bhi, n, leaf_max, None, mut)
    else:
        out = None
        if o["builder"] not in ("lbvh", 1):
            rules = {"rule1-never": (0,), "rule1-always": (1,), "fallback-order": (1, 0)}.get(mut, (0, 1))
            for pair in rules:
                tree = _ploc_tree_once(tris, order, blo, bhi, int(o["ploc_radius"]), pair, mut)
                iters = tree.passes
                out = collapse(tree, blo, bhi, n, leaf_max, sah, mut)
                if out is not None:
                    break
        if out is None:
            tree = karras_tree(skeys, order, blo, bhi, mut)
            iters = 0
            out = collapse(tree, blo, bhi, n, leaf_max, sah, mut)
        if out is None:
            raise RestateError("the Karras tree is too deep for the traversal stack")
    klo, khi, links, depth4 = out
    idx = tree.vals
    t = tris[idx]
    rec[:n, :9] = np.concatenate([t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]], 1).view(np.uint32)
    rec[:n, 9] = 2 * idx
    cs, lb = B.link_layout(n, leaf_max, B.n_internal(n))
    info = {"n": n, "n_nodes4": len(links), "depth4": depth4, "leaf_max": leaf_max, "count_shift": cs,
            "link_bits": lb, "builder_iters": iters, "soa": 0}
    return {"nodes": B.encode_nodes(klo, khi, links), "tris": rec, "info": info,
            "near_exponent_boundary": near_exponent_boundary(klo, khi)}


# ---------------------------------------------------------------- cases of the device comparison
SOUPS = (3, 4, 5, 63, 64, 65, 255, 256, 257, 288, 1023, 1024, 1025)
ALL_OPTIONS = ({}, {"builder": "lbvh"}, {"leaf_max": 1}, {"leaf_max": 4}, {"leaf_max": 16}, {"collapse": "sah"},
               {"collapse": "sah", "sah_c_leaf": 0.2, "sah_c_tri": 2.0}, {"collapse": "sah", "leaf_max": 4},
               {"ploc_radius": 1}, {"ploc_radius": 4}, {"ploc_radius": 256})
LARGE = ("soup4096", "suzanne", "teapot")
LARGE_OPTIONS = ({}, {"builder": "lbvh"}, {"collapse": "sah"})


def opt_id(opts):
    return ",".join(f"{k}={v}" for k, v in opts.items()) or "default"


# translated_1e4 is replaced: at 1e4 a coordinate's ulp is 2^-10 .. 2^-9, every extent a multiple
# of it, and node extents of exactly 255 ulps (0.249, 0.498: the size of a small node of this
# soup) occur in every seed tried -- right on the exponent rule's boundary, where the
# comparison would lean on the device's log2 being exact.  At 1e2 the same soup has none;
# translated_3e5 (255 ulps exceed the scene) keeps the far translation.
REPLACED = {"translated_1e4": "translated_1e2"}
# a (case, options) the restatement needs more than about 5 s for (17 s: 999 passes of rule 0
# with 513-wide windows before rule 1 is tried); r = 256 over equal boxes stays with coincident200
TRIMMED = {("coincident1000", "ploc_radius=256")}
# sah_tie2: a triangle and its copy shifted along x by the float32 at which, under
# collapse=sah with the default costs, the root's leaf cost an * (c_leaf + 2 c_tri) and its
# node cost an + (a0 + a1) * (c_leaf + c_tri) are one and the same float32 (found by walking
# the shift float by float across the crossing): the one case where `cl <= ci` and `cl < ci`
# part -- one leaf of two triangles against a node of two leaves
EXTRA = ("sah_tie2",)
SAH_TIE_SHIFT = float.fromhex("0x1.9e81f8p+0")


def pairs(families):
    """Every (case name, options) the device comparison runs; families: geometry_cases.NON_SWEEP."""
    out = [(f"soup{n}", o) for n in SOUPS for o in ALL_OPTIONS]
    out += [(REPLACED.get(name, name), o) for name in families for o in ALL_OPTIONS]
    out += [(name, o) for name in EXTRA for o in ALL_OPTIONS]
    out += [(name, o) for name in LARGE for o in LARGE_OPTIONS]
    return [(name, o) for name, o in out if (name, opt_id(o)) not in TRIMMED]


def case_tris(name):
    """The triangles of a case: a geometry_cases name, an OBJ scene of data/ (read by the
    library's host loader, the only use of the library here), or a replacement (REPLACED)."""
    import geometry_cases as G
    if name in ("suzanne", "teapot"):
        import toymeshpathtracer_amd as tm
        from conftest import data
        return tm.load_scene(data(name + ".obj"))[0]
    if name == "sah_tie2":
        one = np.array([[0.25, 0.25, 0.25], [0.75, 0.375, 0.25], [0.375, 0.75, 0.5]], f32)
        return np.stack([one, one + np.array([SAH_TIE_SHIFT, 0, 0], f32)]).astype(f32)
    if name == "translated_1e2":
        return (G.soup(300, G._seed("moved")) + np.array([1e2, -2e2, 5e1])).astype(f32)
    return G.case(name)


_cache = {}


def cached_build(name, tris, opts):
    """build() once per (case, options) and process: the CPU and the GPU file share the dumps."""
    key = (name, opt_id(opts))
    if key not in _cache:
        _cache[key] = build(tris, opts)
    return _cache[key]
