#!/usr/bin/env python3
"""Stochastic model of one k_path wave in sample seeding: the voted traversal
rounds, the shading rounds and the camera stash with its riders (DESIGN.md
section 5, "The shading round's divisions and camera block").  No GPU: it prices rules,
it does not measure them.

  python tools/wave_model.py [samples per lane] [seed]

A lane runs units of BLK samples.  A sample is a chain of queries: a closest-hit
query; on a hit (P_HIT) a shadow query (traced with P_LIT, else only counted)
and, below MAX_DEPTH, the scattered ray.  A query is a bag of node and leaf
steps drawn to the measured means (profiles/README_r09.md: 14.9 nodes and 5.1
triangle tests in leaves of <= 2 per closest-hit query, 5.3 and 1.1 per shadow
query); its first TOP node steps stand on LDS-resident nodes.  The kernel's
rules: a wave shades once SHADE_MIN lanes wait or none traverses; a shading
round ends with up to TOP_WALK load-free node rounds for lanes on a top node;
then up to STEPS voted rounds (a leaf round when more lanes stand on a leaf).
Round costs in node rounds: node 1, leaf 1.3, top-walk 0.65, shading 3.8 of
which the camera block 1.0 (charged only when it runs).

What it got right and wrong (profiles/README_r10.md): the lanes at a shading
round and the block's rate without the stash (0.96 of rounds, measured 0.948)
and with it (0.51, measured 0.599).  Wrong: the fixed price of a run.  With
seven lanes instead of 4.5 in the block its share of wave time fell from 9.0 to
8.4 %, not by half -- the disk rejection loop runs until its last lane accepts
-- so the stash lost 2 % where this model promised it 2 %."""
import random
import sys

LANES, STEPS, SHADE_MIN, BLK, MAX_DEPTH = 64, 16, 16, 8, 10
P_HIT, P_LIT = 0.915, 0.6  # 13.3 rays per sample on the bench frame
MEAN = {"closest": (14.9, 3.4), "shadow": (5.3, 0.75)}  # node, leaf steps
TOP, TOP_WALK = 3, 3
COST = {"node": 1.0, "leaf": 1.3, "top": 0.65, "shade": 2.8, "camera": 1.0}


def draw(rng, mean):  # geometric, mean `mean`, at least 0
    n, p = 0, 1.0 / (1.0 + mean)
    while rng.random() > p:
        n += 1
    return n


class Lane:
    def __init__(self):
        self.smp, self.depth, self.kind = BLK, 0, None  # no unit yet
        self.node = self.leaf = self.top = 0
        self.stash = False

    def start(self, rng, kind):
        self.kind = kind
        self.node, self.leaf = 1 + draw(rng, MEAN[kind][0] - 1), draw(rng, MEAN[kind][1])
        self.top = min(TOP, self.node)

    def in_query(self):
        return self.node + self.leaf > 0

    def at_leaf(self, rng):  # where the lane stands: the top nodes first, then at random
        return self.top == 0 and rng.random() * (self.node + self.leaf) < self.leaf


def run(samples_per_lane, seed, stash):
    rng = random.Random(seed)
    lanes = [Lane() for _ in range(LANES)]
    t = {k: 0.0 for k in ("cost", "node_r", "node_l", "leaf_r", "leaf_l", "shade_r", "shade_l", "shade_t", "cam_r",
                          "cam_l", "samples", "ondemand")}
    while t["samples"] < samples_per_lane * LANES:
        need = [l for l in lanes if not l.in_query()]
        if len(need) >= SHADE_MIN or len(need) == LANES:
            t["shade_r"] += 1
            t["shade_l"] += len(need)
            t["shade_t"] += LANES - len(need)
            demand, started = [], set()
            for l in need:
                cam = False
                if l.smp >= BLK:  # a new unit: nothing crosses it
                    l.smp, l.depth, l.stash, cam = 0, 0, False, True
                elif l.kind == "closest" and rng.random() < P_HIT:  # Scatter
                    l.depth += 1
                    if rng.random() < P_LIT:
                        l.start(rng, "shadow")
                    elif l.depth < MAX_DEPTH:
                        l.start(rng, "closest")
                    else:
                        cam = True
                elif l.kind == "shadow" and l.depth < MAX_DEPTH:
                    l.start(rng, "closest")
                else:
                    cam = True  # sky, or MAX_DEPTH hits: the sample is done
                if cam and l.kind is not None and l.smp < BLK:
                    t["samples"] += 1
                    l.smp += 1
                    l.depth = 0
                if l.in_query():
                    started.add(l)
                elif l.smp < BLK:  # starts sample l.smp: from its entry, or on demand
                    if stash and l.stash:
                        l.stash = False
                    else:
                        demand.append(l)
                    l.start(rng, "closest")
                    started.add(l)
                else:
                    l.kind = None  # takes a unit next round (the supply never ends here)
            cost = COST["shade"]
            if demand:
                riders = [l for l in lanes if stash and l not in started and not l.stash and l.smp + 1 < BLK
                          and l.kind is not None] if stash else []
                for l in riders:
                    l.stash = True
                cost += COST["camera"]
                t["cam_r"] += 1
                t["cam_l"] += len(demand) + len(riders)
                t["ondemand"] += len(demand)
            t["cost"] += cost
            for _ in range(TOP_WALK):
                on_top = [l for l in lanes if l.top > 0]
                if not on_top:
                    break
                for l in on_top:
                    l.top -= 1
                    l.node -= 1
                t["cost"] += COST["top"]
        for _ in range(STEPS):
            q = [l for l in lanes if l.in_query()]
            if not q:
                break
            leafs = [l for l in q if l.at_leaf(rng)]
            leaf_round = 2 * len(leafs) > len(q)
            step = leafs if leaf_round else [l for l in q if l not in leafs]
            for l in step:
                if leaf_round:
                    l.leaf -= 1
                else:
                    l.node -= 1
                    l.top = max(0, l.top - 1)
            kind = "leaf" if leaf_round else "node"
            t[kind + "_r"] += 1
            t[kind + "_l"] += len(step)
            t["cost"] += COST[kind]
    return t


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 400
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    res = {s: run(n, seed, s) for s in (False, True)}
    for s, t in res.items():
        print(f"stash {'on ' if s else 'off'}: lanes per node round {t['node_l'] / t['node_r']:.1f}, per leaf round "
              f"{t['leaf_l'] / t['leaf_r']:.1f}; at a shading round {t['shade_l'] / t['shade_r']:.1f} shading / "
              f"{t['shade_t'] / t['shade_r']:.1f} traversing; camera block in {t['cam_r'] / t['shade_r']:.2f} of shading "
              f"rounds, {t['cam_l'] / max(1, t['cam_r']):.1f} lanes per run; {t['ondemand'] / t['samples']:.2f} of "
              f"samples on demand; shading {100 * (t['shade_r'] * COST['shade'] + t['cam_r'] * COST['camera']) / t['cost']:.1f} % "
              f"of wave time; cost per sample {t['cost'] / t['samples']:.3f}")
    a, b = (res[s]["cost"] / res[s]["samples"] for s in (False, True))
    print(f"frame cost with the stash: {100 * (b / a - 1):+.2f} % (before the stash's own loads and stores)")


if __name__ == "__main__":
    main()
