"""Regenerates tests/golden/ref/ from the compiled reference.

    make -C oracle/ref            # needs a checkout of the reference, see its Makefile
    python tests/golden/make_ref_fixtures.py [hit case ... | trace]

Runs oracle/_ref/ref_trace (the reference's GetRay, HitScene and Trace(), sample
by sample) on every trace case of tests/ref_cases.py, oracle/_ref/ref_hits (its
HitScene) on every hit case and oracle/_ref/tmpt_ref (its CLI) on every frame
case, and writes trace_<case>.npz, hits_<case>.npz, frame_<case>.png,
frames.json and the small OBJ exports.  The trace cases must reach the floors of
ref_cases.TRACE_FLOORS, counted from the reference's answers, or the run fails.
The same inputs give the same files byte for byte (ref_cases.save_npz; the PNGs
are tmpt_ref's own output.png).
"""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ref_cases as C  # noqa: E402

REF_BIN = os.path.join(ROOT, "oracle", "_ref")


def make_hits(name, tmp):
    tris, bmin, bmax = C.hit_scene(name)
    box = C.octree_box(bmin, bmax)
    rays = C.hit_rays(name, tris, bmin, bmax)
    hit, rec = C.run_ref_hits(os.path.join(REF_BIN, "ref_hits"), tris, box, rays, tmp)
    C.save_npz(C.hits_path(name), {"tris": tris, "bmin": bmin, "bmax": bmax, "box": box, "rays": rays,
                                   "hit": hit, "rec": rec})
    print(f"hits_{name}: {len(tris)} triangles, {len(rays)} rays, {int(hit.sum())} hits, "
          f"{os.path.getsize(C.hits_path(name)) >> 10} KiB")


def make_frame(name, tmp):
    w, h, spp = C.FRAME_SIZE
    if name != "cube" and name not in C.REGENERATED_OBJ:
        with open(os.path.join(C.REF_DIR, name + ".obj"), "w") as f:
            f.write(C.obj_text(C.frame_tris(name)))
    obj = C.frame_obj_path(name, tmp)
    out = subprocess.run([os.path.join(REF_BIN, "tmpt_ref"), str(w), str(h), str(spp), obj], cwd=tmp, check=True,
                         capture_output=True, text=True).stdout
    krays = float(re.search(r"- ([0-9.]+) K Rays,", out).group(1))
    shutil.move(os.path.join(tmp, "output.png"), os.path.join(C.REF_DIR, f"frame_{name}.png"))
    print(f"frame_{name}: {w}x{h}x{spp}, {krays} K rays")
    return {"width": w, "height": h, "spp": spp, "krays": krays}


def make_trace(name, tmp):
    """trace_<name>.npz: the case's frame through ref_trace, sample seeding (every
    field) and pixel seeding (colour, state out and ray count).  -> trace_counts."""
    w, h, spp = C.TRACE_SIZE
    tris, bmin, bmax, cam = C.trace_scene(name)
    box = C.octree_box(bmin, bmax)
    exe = os.path.join(REF_BIN, "ref_trace")
    ch_s, ch_p = C.seed_chains(w, h, spp, True), C.seed_chains(w, h, spp, False)
    s = C.run_ref_trace(exe, tris, box, cam, w, h, ch_s, tmp)
    p = C.run_ref_trace(exe, tris, box, cam, w, h, ch_p, tmp)
    fx = {"tris": tris, "bmin": bmin, "bmax": bmax, "box": box, "cam": cam, "size": np.array([w, h, spp], np.int32),
          "chains_sample": ch_s, "chains_pixel": ch_p}
    fx.update({"s_" + k: v for k, v in s.items()})
    fx.update({"p_" + k: p[k] for k in ("col", "state", "rays")})
    C.save_npz(C.trace_path(name), fx)
    counts = C.trace_counts(fx)
    print(f"trace_{name}: {len(tris)} triangles, {w}x{h}x{spp}, {counts}, {os.path.getsize(C.trace_path(name)) >> 10} KiB")
    return counts


def main(argv):
    os.makedirs(C.REF_DIR, exist_ok=True)
    only = set(argv)
    with tempfile.TemporaryDirectory() as tmp:
        if not only or only & {"trace"}:  # "trace": the trace cases alone
            C.check_trace_counts({name: make_trace(name, tmp) for name in C.TRACE_CASES})
            only.discard("trace")
            if argv and not only:
                return
        for name in C.HIT_CASES:
            if not only or name in only:
                make_hits(name, tmp)
        if not only:
            frames = {name: make_frame(name, tmp) for name in C.FRAME_CASES}
            with open(os.path.join(C.REF_DIR, "frames.json"), "w") as f:
                json.dump(frames, f, indent=1, sort_keys=True)
                f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
