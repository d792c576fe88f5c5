"""The built BVH checked exhaustively from a host dump (Scene.dump_bvh).

Pure numpy and Python integers: neither the GPU library nor the oracle is
imported here.  ``check()`` takes the triangles as given, a dump and the build
options and returns a list of findings (empty: nothing wrong), each beginning
with the name of the rule it breaks.  What the rules restate, in this file's
own words, from tmpt_internal.h and DESIGN.md section 3:

node (16 words)  [0..2] origin.xyz, f32 bits; [3] bytes 0..2 the exponents ex,
    ey, ez as SIGNED bytes (scale 2^e), byte 3 the child-valid mask; [4..9] the
    planes qlo.x qhi.x qlo.y qhi.y qlo.z qhi.z, child k in byte k; [10, 11] 0;
    [12..15] the links.  A child's box is origin + q * 2^e, taken exactly.
link  an internal child is its node index; a leaf is
    bit 31 | (count - 1) << count_shift | first, with count_shift = bits(n) and
    link_bits = max(count_shift + bits(leaf_max - 1), bits(n_internal - 1))
    where n_internal = n - 1 (1 for n = 1) and bits(v) is v's bit length;
    the pop key has K = min(31 - link_bits, 16, cap) bits, 0 where K < 9.
triangle record (12 words)  v0.xyz, e1 = v1 - v0, e2 = v2 - v0 (f32, each
    difference rounded once), [9] = 2 * index | flat mark, [10, 11] = 0; record
    n is the null triangle, all zero.
triangle box  lo / hi = the f32 min / max of the vertices, widened per axis by
    pad = kBoxPadRel * (max(|lo|, |hi|) + (hi - lo)) + 1e-30f, every operation
    rounded to f32 (kBoxPadRel = 1e-5f).

Rules (the names findings carry):
  tree-reach    from node 0 every index in [0, n_nodes4) is reached exactly once
  tree-order    an internal child's index exceeds its parent's
  tree-levels   depth L's nodes fill one contiguous range straight after depth L-1's
  tree-depth    the measured depth equals info depth4 (and stats bvh4_depth)
  stack         3 * depth4 + 1 <= 128
  info          n, n_nodes4 (and stats bvh4_nodes), leaf_max agree with the build
  slot-mask     valid children fill slots 0..nc-1: mask = (1 << nc) - 1
  slot-nc       nc >= 2, except the tree that is one leaf
  slot-empty    an empty slot has qlo = 255, qhi = 0 on every axis and the link bit 31 | n
  slot-pad      words [10, 11] are 0
  link-bits     bits 30..link_bits of every link are 0
  link-layout   (count_shift, link_bits) equal the restated layout
  pop-key       option pop_key_bits equals the restated formula
  leaf-partition  the leaf ranges [first, first + count) partition [0, n)
  leaf-count    1 <= count <= leaf_max
  leaf-greedy   collapse=greedy: no internal child heads <= leaf_max triangles
  tri-perm      [9] >> 1 over records 0..n-1 is a permutation of 0..n-1
  tri-bits      v0, e1, e2 equal the f32 numpy values of that triangle bit for bit
  tri-pad       words [10, 11] of every record are 0
  tri-null      record n is all zero
  tri-flat      bit 0 of [9] is set exactly on the expected (octree-flat) triangles
  box-contain   the decoded child box contains the union U of the padded boxes
                beneath it, on all six faces (exact integers, units of 2^-149)
  box-tight     each face lies less than one quantum 2^e outside U
  box-origin    origin = the minimum of the children's U per axis (equal as
                numbers: the sign of a zero is not compared)
  box-exp       e is the least exponent in [-126, 127] with
                255 * 2^e >= max(extent, 1e-30), extent the exact f32 difference.
                Exception: the device takes e from a double-precision log2, so
                where the extent is within 2^-40 relative of 255 * 2^k for the k
                at the boundary, either neighbour passes.
  soa           dump_bvh("soa") equals dump_bvh("aos") word for word

``canonical()`` renumbers a dump's nodes breadth-first in child-slot order;
``reference_dump()`` builds a dump from a median-split reference tree with the
documented encoding (the project's own naive builder, and the proof that the
rules above can be met); ``cost()`` is the surface-area cost of a dump.
"""
from fractions import Fraction

import numpy as np

STACK_TOTAL = 128
POP_KEY_MIN, POP_KEY_MAX = 9, 16
BOX_PAD_REL = np.float32(1e-5)
BOX_PAD_ABS = np.float32(1e-30)
# max(extent, 1e-30) in units of 2^-149: the double 1e-30, rounded up to a whole unit
_EXT_FLOOR = -((-Fraction(1e-30) * 2 ** 149).__floor__())
AXES = "xyz"


# ---------------------------------------------------------------- restated layout
def bits_for(v):
    return int(v).bit_length()


def link_layout(n, leaf_max, n_internal):
    """-> (count_shift, link_bits) of a scene of n triangles."""
    cs = bits_for(n)
    leaf = cs + bits_for(leaf_max - 1)
    node = bits_for(n_internal - 1 if n_internal else 0)
    return cs, max(leaf, node)


def pop_key_bits(link_bits, cap=-1):
    k = min(31 - link_bits, POP_KEY_MAX)
    if cap >= 0:
        k = min(k, cap)
    return 0 if k < POP_KEY_MIN else k


def pop_key_mask(k):
    return (((1 << k) - 1) << (31 - k)) if k else 0


def leaf_link(count, first, count_shift):
    return 0x80000000 | ((count - 1) << count_shift) | first


def n_internal(n):
    return n - 1 if n >= 2 else 1


# ---------------------------------------------------------------- exact numbers
def f32_units(a):
    """float32 array -> object array of Python ints: the values in units of 2^-149 (exact)."""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.int64)
    e, m = (b >> 23) & 255, b & 0x7FFFFF
    mag = np.where(e == 0, m, m | (1 << 23)).astype(object) << np.maximum(e - 1, 0).astype(object)
    return np.where(b >> 31 != 0, -mag, mag)


def least_exponent(extent_units):
    """The least e in [-126, 127] with 255 * 2^e >= max(extent, 1e-30); the extent in units of 2^-149."""
    x = max(int(extent_units), _EXT_FLOOR)
    s = max(0, x.bit_length() - 8)
    if (255 << s) < x:
        s += 1
    return min(127, max(-126, s - 149))


def tri_boxes(tris):
    """-> (lo, hi) float32 [n, 3]: the padded triangle boxes, op by op in f32."""
    t = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    lo, hi = t.min(1), t.max(1)
    pad = BOX_PAD_REL * (np.maximum(np.abs(lo), np.abs(hi)) + (hi - lo)) + BOX_PAD_ABS
    assert pad.dtype == np.float32
    return lo - pad, hi + pad


# ---------------------------------------------------------------- decoding
class Decoded:
    """The fields of a dump's node words."""

    def __init__(self, nodes, count_shift):
        w = np.asarray(nodes, np.uint32).reshape(-1, 16)
        self.origin = w[:, 0:3].copy().view(np.float32)
        self.exp = ((w[:, 3:4] >> (8 * np.arange(3, dtype=np.uint32))) & 255).astype(np.int8).astype(np.int64)
        self.mask = (w[:, 3] >> 24).astype(np.int64)
        sh = 8 * np.arange(4, dtype=np.uint32)
        q = ((w[:, 4:10, None] >> sh) & 255).astype(np.int64)  # [node, plane, slot]
        self.qlo = q[:, 0::2].transpose(0, 2, 1)  # [node, slot, axis]
        self.qhi = q[:, 1::2].transpose(0, 2, 1)
        self.pad = w[:, 10:12]
        self.link = w[:, 12:16].astype(np.int64)
        self.valid = ((self.mask[:, None] >> np.arange(4)) & 1).astype(bool)
        self.leaf = (self.link >> 31) != 0
        self.first = self.link & ((1 << count_shift) - 1)
        self.count = ((self.link >> count_shift) & 15) + 1


def _levels(d, n4, bad):
    """Breadth-first from node 0 -> list of index arrays per depth (in slot order)."""
    seen = np.zeros(n4, bool)
    seen[0] = True
    levels, cur, end = [np.zeros(1, np.int64)], np.zeros(1, np.int64), 1
    while True:
        m = d.valid[cur] & ~d.leaf[cur]
        ch, par = d.link[cur][m], np.repeat(cur, 4).reshape(-1, 4)[m]
        out = ch >= n4
        if out.any():
            bad.append(f"tree-reach: node {par[out][0]} links to {ch[out][0]}, beyond n_nodes4 {n4}")
        back = ~out & (ch <= par)
        if back.any():
            bad.append(f"tree-order: node {par[back][0]} has child {ch[back][0]}, not above it")
        ch = ch[~out]
        u, cnt = np.unique(ch, return_counts=True)
        twice = u[(cnt > 1) | seen[u]]
        if twice.size:
            bad.append(f"tree-reach: node {twice[0]} is reached more than once ({twice.size} such at depth {len(levels)})")
        fresh = ~seen[ch]
        _, firsts = np.unique(ch, return_index=True)
        keep = np.zeros(ch.size, bool)
        keep[firsts] = True
        ch = ch[fresh & keep]
        if ch.size == 0:
            break
        if not np.array_equal(np.sort(ch), np.arange(end, end + ch.size)):
            bad.append(f"tree-levels: depth {len(levels)} holds {ch.size} nodes {ch.min()}..{ch.max()}, "
                       f"not the range {end}..{end + ch.size - 1}")
        seen[ch] = True
        end += ch.size
        levels.append(ch)
        cur = ch
    if not seen.all():
        miss = np.nonzero(~seen)[0]
        bad.append(f"tree-reach: {miss.size} nodes are never reached, first {miss[0]}")
    return levels


def canonical(dump):
    """The dump's nodes renumbered breadth-first in child-slot order (uint32 [n_nodes4, 16]):
    two builds of one input are equal in this form whatever order their levels were numbered in."""
    nodes = np.asarray(dump["nodes"], np.uint32)
    n4 = nodes.shape[0]
    if n4 == 0:
        return nodes.copy()
    d = Decoded(nodes, dump["info"]["count_shift"])
    order, new = [0], {0: 0}
    for old in order:  # grows as it is walked
        for k in range(4):
            if d.valid[old, k] and not d.leaf[old, k]:
                c = int(d.link[old, k])
                if c in new or c >= n4:
                    raise ValueError(f"canonical: node {c} reached twice or out of range")
                new[c] = len(order)
                order.append(c)
    out = nodes[np.array(order)].copy()
    dn = Decoded(out, dump["info"]["count_shift"])
    remap = np.zeros(n4, np.uint32)
    remap[np.array(order)] = np.arange(len(order), dtype=np.uint32)
    inner = dn.valid & ~dn.leaf
    links = out[:, 12:16]
    links[inner] = remap[links[inner]]
    return out


# ---------------------------------------------------------------- the checker
def check(tris, dump, opts=None, stats=None, pop_key=None, flat=None, soa=None):
    """-> findings.  tris: the triangles as given to the build; dump: Scene.dump_bvh();
    opts: the build options; stats: Scene.stats() (bvh4_nodes, bvh4_depth, n_tris compared);
    pop_key: get_option("pop_key_bits"); flat: bool [n], the triangles expected to carry the
    flat mark (None: none); soa: the dump_bvh("soa") of the same scene."""
    opts = dict(opts or {})
    bad = []
    tris = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    n = tris.shape[0]
    info = dump["info"]
    nodes = np.asarray(dump["nodes"], np.uint32)
    rec = np.asarray(dump["tris"], np.uint32)
    n4 = info["n_nodes4"]
    leaf_max = int(opts.get("leaf_max", 2))
    if info["n"] != n or rec.shape != (n + 1, 12):
        return [f"info: n {info['n']}, {rec.shape[0]} records for {n} triangles"]
    if nodes.shape != (n4, 16):
        return [f"info: n_nodes4 {n4} but {nodes.shape[0]} node records"]
    if stats is not None:
        if stats.bvh4_nodes != n4 or stats.n_tris != n:
            bad.append(f"info: stats bvh4_nodes {stats.bvh4_nodes} n_tris {stats.n_tris}, dump {n4} {n}")
        if stats.bvh4_depth != info["depth4"]:
            bad.append(f"tree-depth: stats bvh4_depth {stats.bvh4_depth}, info depth4 {info['depth4']}")
    if soa is not None:
        for key in ("nodes", "tris"):
            a, b = np.asarray(dump[key], np.uint32), np.asarray(soa[key], np.uint32)
            if a.shape != b.shape:
                bad.append(f"soa: {key} {b.shape} from the planes, {a.shape} from the records")
            elif (a != b).any():
                at = np.argwhere(a != b)[0]
                bad.append(f"soa: {key} record {at[0]} word {at[1]}: {b[tuple(at)]:#x} in the planes, "
                           f"{a[tuple(at)]:#x} in the records ({int((a != b).sum())} words differ)")
        if soa["info"] != info:
            bad.append(f"soa: info {soa['info']} != {info}")
    # ---- triangle records
    if rec[n].any():
        bad.append(f"tri-null: record {n} is not all zero: {rec[n]}")
    if n == 0:
        if n4 != 0 or info["depth4"] != 0:
            bad.append(f"info: the empty scene has n_nodes4 {n4}, depth4 {info['depth4']}")
        return bad
    if info["leaf_max"] != leaf_max:
        bad.append(f"info: leaf_max {info['leaf_max']}, built with {leaf_max}")
    idx = (rec[:n, 9] >> 1).astype(np.int64)
    if rec[:n, 10:].any():
        bad.append(f"tri-pad: record {np.nonzero(rec[:n, 10:].any(1))[0][0]} has non-zero padding words")
    perm_ok = idx.max() < n and np.array_equal(np.sort(idx), np.arange(n))
    if not perm_ok:
        bad.append("tri-perm: the index words of records 0..n-1 are no permutation of 0..n-1")
        return bad
    t = tris[idx]
    want = np.concatenate([t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]], 1)
    assert want.dtype == np.float32
    diff = np.argwhere(want.view(np.uint32) != rec[:n, :9])
    if diff.size:
        names = [f"{v}.{a}" for v in ("v0", "e1", "e2") for a in AXES]
        bad.append(f"tri-bits: record {diff[0][0]} (triangle {idx[diff[0][0]]}) {names[diff[0][1]]} is "
                   f"{rec[diff[0][0], diff[0][1]]:#x}, not {want.view(np.uint32)[tuple(diff[0])]:#x} "
                   f"({len(diff)} words differ)")
    marks = np.zeros(n, bool)
    marks[idx] = (rec[:n, 9] & 1).astype(bool)
    expect = np.zeros(n, bool) if flat is None else np.asarray(flat, bool)
    if (marks != expect).any():
        w = np.nonzero(marks != expect)[0]
        bad.append(f"tri-flat: {w.size} triangles carry the wrong flat mark, first {w[0]} "
                   f"(marked {marks.sum()}, expected {expect.sum()})")
    # ---- layout
    cs, lb = link_layout(n, leaf_max, n_internal(n))
    if (info["count_shift"], info["link_bits"]) != (cs, lb):
        bad.append(f"link-layout: (count_shift, link_bits) = ({info['count_shift']}, {info['link_bits']}), "
                   f"restated ({cs}, {lb})")
    if pop_key is not None and int(pop_key) != pop_key_bits(lb, int(opts.get("pop_key_cap", -1))):
        bad.append(f"pop-key: option pop_key_bits {pop_key}, restated {pop_key_bits(lb)}")
    if 3 * info["depth4"] + 1 > STACK_TOTAL:
        bad.append(f"stack: depth4 {info['depth4']} overruns the traversal stack")
    if n4 < 1:
        return bad + [f"info: n_nodes4 {n4} for {n} triangles"]
    d = Decoded(nodes, cs)
    # ---- slots
    nc = d.valid.sum(1)
    w = np.nonzero(d.mask != (1 << nc) - 1)[0]
    if w.size:
        bad.append(f"slot-mask: node {w[0]} has mask {d.mask[w[0]]:#x}: valid children do not fill slots 0..nc-1")
    one_leaf = n4 == 1 and nc[0] == 1 and d.leaf[0, 0] and d.first[0, 0] == 0 and d.count[0, 0] == n
    w = np.nonzero(nc < 2)[0]
    if w.size and not one_leaf:
        bad.append(f"slot-nc: node {w[0]} has {nc[w[0]]} children")
    empty = ~d.valid
    wrong = empty & ((d.qlo != 255).any(2) | (d.qhi != 0).any(2))
    if wrong.any():
        at = np.argwhere(wrong)[0]
        bad.append(f"slot-empty: node {at[0]} slot {at[1]} is empty but its box is not the inverted one "
                   f"(qlo {d.qlo[tuple(at)]}, qhi {d.qhi[tuple(at)]})")
    wrong = empty & (d.link != (0x80000000 | n))
    if wrong.any():
        at = np.argwhere(wrong)[0]
        bad.append(f"slot-empty: node {at[0]} slot {at[1]} is empty but links to {d.link[tuple(at)]:#x}, "
                   f"not the null leaf")
    if d.pad.any():
        bad.append(f"slot-pad: node {np.nonzero(d.pad.any(1))[0][0]} has non-zero words [10, 11]")
    stray = ((d.link & 0x7FFFFFFF) >> info["link_bits"]) != 0
    if stray.any():
        at = np.argwhere(stray)[0]
        bad.append(f"link-bits: node {at[0]} slot {at[1]} link {d.link[tuple(at)]:#x} uses bits at or above "
                   f"link_bits {info['link_bits']}")
    # ---- tree
    before = len(bad)
    levels = _levels(d, n4, bad)
    if len(levels) != info["depth4"]:
        bad.append(f"tree-depth: measured depth {len(levels)}, info depth4 {info['depth4']}")
    tree_ok = not any(b.startswith(("tree-reach", "tree-order")) for b in bad[before:])
    # ---- leaves
    lm = d.valid & d.leaf
    first, count = d.first[lm], d.count[lm]
    w = np.nonzero(count > leaf_max)[0]
    if w.size:
        at = np.argwhere(lm)[w[0]]
        bad.append(f"leaf-count: node {at[0]} slot {at[1]} holds {count[w[0]]} triangles, leaf_max {leaf_max}")
    o = np.argsort(first, kind="stable")
    f, c = first[o], count[o]
    ends = f + c
    part_ok = f.size > 0 and f[0] == 0 and ends[-1] == n and np.array_equal(f[1:], ends[:-1])
    if not part_ok:
        where = "no leaves" if not f.size else (
            f"first leaf starts at {f[0]}" if f[0] != 0 else
            f"record {ends[:-1][f[1:] != ends[:-1]][0]} is lost or doubled" if not np.array_equal(f[1:], ends[:-1])
            else f"the last leaf ends at {ends[-1]}, n = {n}")
        bad.append(f"leaf-partition: the leaf ranges do not partition [0, {n}): {where}")
    if not (tree_ok and part_ok):
        return bad  # the box rules need a tree and its leaves
    # ---- unions, bottom-up once: U of every valid slot, triangle counts
    blo, bhi = tri_boxes(tris)
    blo, bhi = blo[idx], bhi[idx]  # leaf order
    slo = np.full((n4, 4, 3), np.inf, np.float32)
    shi = np.full((n4, 4, 3), -np.inf, np.float32)
    scount = np.zeros((n4, 4), np.int64)
    nlo = np.zeros((n4, 3), np.float32)
    nhi = np.zeros((n4, 3), np.float32)
    ncount = np.zeros(n4, np.int64)
    for lev in reversed(levels):
        v, lf = d.valid[lev], d.leaf[lev]
        for k in range(4):
            leaf_k = lev[v[:, k] & lf[:, k]]
            if leaf_k.size:
                f0, c0 = d.first[leaf_k, k], d.count[leaf_k, k]
                lo, hi = blo[f0].copy(), bhi[f0].copy()
                for j in range(1, int(c0.max())):
                    m = c0 > j
                    lo[m] = np.minimum(lo[m], blo[f0[m] + j])
                    hi[m] = np.maximum(hi[m], bhi[f0[m] + j])
                slo[leaf_k, k], shi[leaf_k, k], scount[leaf_k, k] = lo, hi, c0
            inner_k = lev[v[:, k] & ~lf[:, k]]
            if inner_k.size:
                ch = d.link[inner_k, k]
                slo[inner_k, k], shi[inner_k, k], scount[inner_k, k] = nlo[ch], nhi[ch], ncount[ch]
        nlo[lev], nhi[lev], ncount[lev] = slo[lev].min(1), shi[lev].max(1), scount[lev].sum(1)
    if opts.get("collapse", "greedy") in ("greedy", 0):
        small = d.valid & ~d.leaf & (scount <= leaf_max)
        if small.any():
            at = np.argwhere(small)[0]
            bad.append(f"leaf-greedy: node {at[0]} slot {at[1]} is a node over {scount[tuple(at)]} triangles: "
                       f"it would have been one leaf")
    # ---- boxes, in exact integers (units of 2^-149)
    if not (np.isfinite(d.origin).all() and np.isfinite(nlo).all() and np.isfinite(nhi).all()):
        return bad + ["box-origin: a node origin or a triangle box is not finite"]
    ulo, uhi = f32_units(np.where(d.valid[..., None], slo, 0)), f32_units(np.where(d.valid[..., None], shi, 0))
    org = f32_units(d.origin)
    want_org = f32_units(nlo)
    w = np.argwhere(org != want_org)
    if w.size:
        bad.append(f"box-origin: node {w[0][0]} origin.{AXES[w[0][1]]} is {d.origin[tuple(w[0])]!r}, the children's "
                   f"minimum is {nlo[tuple(w[0])]!r} ({len(w)} differ)")
    if (d.exp < -126).any():
        bad.append(f"box-exp: node {np.argwhere(d.exp < -126)[0][0]} has an exponent below -126")
        return bad
    quant = np.left_shift(1, (d.exp + 149).astype(object))  # [node, axis]
    dlo = org[:, None, :] + d.qlo.astype(object) * quant[:, None, :]
    dhi = org[:, None, :] + d.qhi.astype(object) * quant[:, None, :]
    val = np.broadcast_to(d.valid[..., None], dlo.shape)
    for nm, out in (("lo", val & (dlo > ulo)), ("hi", val & (dhi < uhi))):
        if out.any():
            at = np.argwhere(out)[0]
            bad.append(f"box-contain: node {at[0]} slot {at[1]} {nm}.{AXES[at[2]]} lies inside the union of its "
                       f"triangles' boxes ({int(out.sum())} faces)")
    for nm, out in (("lo", val & (ulo - dlo >= quant[:, None, :])), ("hi", val & (dhi - uhi >= quant[:, None, :]))):
        if out.any():
            at = np.argwhere(out)[0]
            bad.append(f"box-tight: node {at[0]} slot {at[1]} {nm}.{AXES[at[2]]} lies a quantum or more outside "
                       f"the union ({int(out.sum())} faces)")
    ext = f32_units(nhi) - want_org
    for i, a in np.argwhere(np.frompyfunc(least_exponent, 1, 1)(ext).astype(np.int64) != d.exp):
        x, got = max(int(ext[i, a]), _EXT_FLOOR), int(d.exp[i, a])
        e = least_exponent(x)
        # the stated exception: an extent within 2^-40 relative of the boundary 255 * 2^k
        k = min(got, e) + 149
        if abs(got - e) == 1 and k >= 0 and abs(x - (255 << k)) << 40 <= (255 << k):
            continue
        bad.append(f"box-exp: node {i} axis {AXES[a]} has exponent {got}, the least that covers its extent is {e}")
        break
    return bad


# ---------------------------------------------------------------- cost
def cost(dump, tris):
    """Sum over valid child slots of area(decoded box) / area(root union) x (1 for a node,
    the triangle count for a leaf), in float64."""
    info = dump["info"]
    d = Decoded(dump["nodes"], info["count_shift"])
    sc = np.ldexp(1.0, d.exp)  # [node, axis]
    lo = d.origin.astype(np.float64)[:, None, :] + d.qlo * sc[:, None, :]
    hi = d.origin.astype(np.float64)[:, None, :] + d.qhi * sc[:, None, :]
    e = hi - lo
    area = e[..., 0] * e[..., 1] + e[..., 1] * e[..., 2] + e[..., 2] * e[..., 0]
    blo, bhi = tri_boxes(tris)
    r = bhi.max(0).astype(np.float64) - blo.min(0).astype(np.float64)
    root = r[0] * r[1] + r[1] * r[2] + r[2] * r[0]
    weight = np.where(d.leaf, d.count, 1)
    return float((area * weight)[d.valid].sum() / root)


# ---------------------------------------------------------------- reference tree and encoder
def encode_nodes(klo, khi, links):
    """The documented node encoding: klo / khi [node, slot, axis] the children's float32 boxes
    (an empty slot: +inf / -inf), links [node, slot] (an empty slot: the null leaf) ->
    uint32 [node, 16].  Origin = the children's minimum, the least exponent per axis, faces
    quantised outward in exact integers, empty slots inverted."""
    klo, khi = np.array(klo, np.float32), np.array(khi, np.float32)  # [node, slot, axis]
    n4 = klo.shape[0]
    links = np.array(links, np.int64)
    valid = np.isfinite(klo[..., 0])
    lo, hi = klo.min(1), khi.max(1)
    olo = f32_units(lo)
    exp = np.frompyfunc(least_exponent, 1, 1)(f32_units(hi) - olo).astype(np.int64)
    quant = np.left_shift(1, (exp + 149).astype(object))[:, None, :]
    v3 = valid[..., None]
    ql = (f32_units(np.where(v3, klo, 0)) - olo[:, None, :]) // quant
    qh = -((olo[:, None, :] - f32_units(np.where(v3, khi, 0))) // quant)
    ql = np.where(v3, np.clip(ql.astype(np.int64), 0, 255), 255)
    qh = np.where(v3, np.clip(qh.astype(np.int64), 0, 255), 0)
    nodes = np.zeros((n4, 16), np.uint32)
    nodes[:, 0:3] = lo.view(np.uint32)
    nodes[:, 3] = ((exp & 255) << (8 * np.arange(3))).sum(1) | (((1 << valid.sum(1)) - 1) << 24)
    sh = 8 * np.arange(4)
    for a in range(3):
        nodes[:, 4 + 2 * a] = (ql[:, :, a] << sh).sum(1)
        nodes[:, 5 + 2 * a] = (qh[:, :, a] << sh).sum(1)
    nodes[:, 12:16] = links
    return nodes


def reference_dump(tris, leaf_max=2):
    """A dump (AoS form) of the median-split reference tree of the triangles: split along the
    largest extent of the box centres, sorted by centre along it, at cnt // 2, leaves of at
    most leaf_max; collapsed to 4-wide by opening a node's children into the grandchildren;
    numbered breadth-first; encoded by the documented rule."""
    tris = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    n = tris.shape[0]
    cs, lb = link_layout(n, leaf_max, n_internal(n)) if n else (0, 31)
    info = {"n": n, "n_nodes4": 0, "depth4": 0, "leaf_max": leaf_max if n else 0, "count_shift": cs,
            "link_bits": lb, "builder_iters": 0, "soa": 0}
    rec = np.zeros((n + 1, 12), np.uint32)
    if n == 0:
        return {"nodes": np.zeros((0, 16), np.uint32), "tris": rec, "info": info}
    cen = 0.5 * (tris.min(1).astype(np.float64) + tris.max(1))
    plo, phi = tri_boxes(tris)
    order = []  # leaf order
    # binary tree: ("leaf", first, count, lo, hi) or ("node", left, right, lo, hi), lo / hi the union

    def build(ids):
        if len(ids) <= leaf_max:
            order.extend(ids.tolist())
            return ("leaf", len(order) - len(ids), len(ids), plo[ids].min(0), phi[ids].max(0))
        c = cen[ids]
        ax = int(np.argmax(c.max(0) - c.min(0)))
        ids = ids[np.argsort(c[:, ax], kind="stable")]
        h = len(ids) // 2
        left, right = build(ids[:h]), build(ids[h:])
        return ("node", left, right, np.minimum(left[3], right[3]), np.maximum(left[4], right[4]))

    root = build(np.arange(n))
    idx = np.array(order)
    t = tris[idx]
    rec[:n, :9] = np.concatenate([t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]], 1).view(np.uint32)
    rec[:n, 9] = 2 * idx

    def wide_children(b):
        if b[0] == "leaf":
            return [b]
        out = []
        for c in b[1:3]:
            out += list(c[1:3]) if c[0] == "node" else [c]
        return out

    # breadth-first numbering in slot order
    queue, depth_of, klo, khi, links = [root], [1], [], [], []
    i = 0
    while i < len(queue):
        kids = wide_children(queue[i])
        row = []
        for c in kids:
            if c[0] == "leaf":
                row.append(leaf_link(c[2], c[1], cs))
            else:
                row.append(len(queue))
                queue.append(c)
                depth_of.append(depth_of[i] + 1)
        pad = 4 - len(kids)
        klo.append([c[3] for c in kids] + [np.full(3, np.inf, np.float32)] * pad)
        khi.append([c[4] for c in kids] + [np.full(3, -np.inf, np.float32)] * pad)
        links.append(row + [0x80000000 | n] * pad)
        i += 1
    nodes = encode_nodes(klo, khi, links)
    info["n_nodes4"], info["depth4"] = len(queue), max(depth_of)
    return {"nodes": nodes, "tris": rec, "info": info}


def closest_hit(dump, rays, tmin, tmax, mt):
    """The linear scan over the device's own records: every triangle a leaf names, by
    Moller-Trumbore (mt: the module tests/mt_numpy.py, whose operation order this keeps) on
    the dumped v0, e1, e2 -> (ids int32, t float32), the lowest index on a tie in t, -1 / inf
    on a miss.  rays (r, 6) float32."""
    f32 = np.float32
    info = dump["info"]
    d = Decoded(dump["nodes"], info["count_shift"])
    lm = d.valid & d.leaf
    slots = np.concatenate([np.arange(f, f + c) for f, c in zip(d.first[lm], d.count[lm])] or [np.zeros(0, np.int64)])
    rec = np.asarray(dump["tris"], np.uint32)[slots]
    v = rec[:, :9].copy().view(f32)
    tid = (rec[:, 9] >> 1).astype(np.int64)
    rays = np.asarray(rays, f32)
    col = lambda a: tuple(a[..., c] for c in range(3))
    o, dr = col(rays[:, None, 0:3]), col(rays[:, None, 3:6])
    v0, e1, e2 = col(v[None, :, 0:3]), col(v[None, :, 3:6]), col(v[None, :, 6:9])
    with np.errstate(all="ignore"):
        pvec = mt._cross(dr, e2)
        det = mt._dot(e1, pvec)
        ok = ~((det > -mt.EPS) & (det < mt.EPS))
        inv = mt.ONE / det
        tvec = mt._sub(o, v0)
        u = mt._dot(tvec, pvec) * inv
        ok &= ~((u < mt.ZERO) | (u > mt.ONE))
        qvec = mt._cross(tvec, e1)
        w = mt._dot(dr, qvec) * inv
        ok &= ~((w < mt.ZERO) | (u + w > mt.ONE))
        t = mt._dot(e2, qvec) * inv
        ok &= (t >= f32(tmin)) & (t <= f32(tmax))
    assert t.dtype == f32
    t = np.where(ok, t, f32(np.inf))
    best = t.min(1) if t.shape[1] else np.full(rays.shape[0], np.inf, f32)
    cand = np.where(t == best[:, None], tid[None, :], np.iinfo(np.int64).max)
    ids = np.where(np.isfinite(best), cand.min(1) if t.shape[1] else -1, -1).astype(np.int32)
    return ids, best
