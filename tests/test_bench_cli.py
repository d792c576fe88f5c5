"""bench.py's own interface: a plain run does only what the headline figure
needs (what else it measures sits behind --full), --steps sets the number of
timed steps, and --dump-outputs writes what the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOVED = ("roofline", "cpu_baseline", "parity_sample", "host_paths")  # null without --full; seed_modes: empty
LIMIT = 64 * 10**6


def _bench(args):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1"] + args, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]
    return json.loads(lines[0])


def test_dump_outputs_samples_a_large_frame(tmp_path):
    """A frame above 64 MB as float32 (the 4K config's) is written as the same
    seeded sample of its rows in every run, all files together under the limit."""
    sys.path.insert(0, ROOT)
    import bench
    h, w = 2160, 3840
    frame = (np.arange(h * w * 4, dtype=np.uint32) % 251).astype(np.uint8).reshape(h, w, 4)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), frame, 12345)
    a = {n: np.load(tmp_path / "a" / n) for n in sorted(os.listdir(tmp_path / "a"))}
    b = {n: np.load(tmp_path / "b" / n) for n in sorted(os.listdir(tmp_path / "b"))}
    assert sorted(a) == sorted(b) == ["image.npy", "image_rows.npy", "rays.npy"]
    assert all(np.array_equal(a[n], b[n]) for n in a)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in a) <= LIMIT
    rows = a["image_rows.npy"].astype(np.int64)
    assert 0 < len(rows) < h and np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < h
    assert np.array_equal(a["image.npy"], frame[rows].astype(np.float32))
    assert a["rays.npy"].tolist() == [12345.0]


def test_dump_outputs_keeps_a_frame_under_the_limit_whole(tmp_path):
    frame = (np.arange(90 * 160 * 4, dtype=np.uint32) % 251).astype(np.uint8).reshape(90, 160, 4)
    sys.path.insert(0, ROOT)
    import bench
    bench.dump_outputs(str(tmp_path), frame, 7)
    assert sorted(os.listdir(tmp_path)) == ["image.npy", "rays.npy"]
    img = np.load(tmp_path / "image.npy")
    assert img.dtype == np.float32 and np.array_equal(img, frame.astype(np.float32))


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(gpu, tmp_path):
    """Without --full the line carries none of the side measurements; the dumped
    frame is the frame --save writes, the dumped ray count the step's."""
    png = tmp_path / "frame.png"
    line = _bench(["--config", "suzanne360", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "out"),
                   "--save", str(png)])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "MRays/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    # value = rays / elapsed in MRays/s and ms_per_step = elapsed / steps: the same timed
    # region, so they agree to the line's rounding (both to 2 decimals: half a unit each, and some)
    rel = 0.006 / line["ms_per_step"] + 0.006 / line["value"] + 1e-6
    assert line["value"] == pytest.approx(line["config"]["rays_per_step"] / line["ms_per_step"] / 1e3, rel=rel)
    assert line["seed_modes"] == {} and all(line[k] is None for k in MOVED)
    assert line["reference_octree"]["index_rule"] is None
    assert sorted(os.listdir(tmp_path / "out")) == ["image.npy", "rays.npy"]
    img = np.load(tmp_path / "out" / "image.npy")
    assert img.dtype == np.float32 and img.shape == (360, 640, 4)
    # the frame's row 0 is the lowest rendered row; the PNG is written flipped, top row first
    assert np.array_equal(img[::-1], np.asarray(Image.open(png).convert("RGBA")).astype(np.float32))
    assert np.load(tmp_path / "out" / "rays.npy").tolist() == [float(line["config"]["rays_per_step"])]


@pytest.mark.gpu
def test_full_run_measures_the_rest(gpu):
    """--full: the other seeding modes, the index tie rule, the roofline, the CPU
    baseline with its parity sample and the host paths are all in the line."""
    line = _bench(["--config", "suzanne360", "--steps", "2", "--warmup", "1", "--full", "--cpu-seconds", "0.5"])
    assert set(line["seed_modes"]) == {"pixel", "row"} and all(v["value"] > 0 for v in line["seed_modes"].values())
    assert all(line[k] is not None for k in MOVED)
    assert line["parity_sample"]["pixels_checked"] > 0 and line["parity_sample"]["pixels_differ"] == 0
    assert line["cpu_baseline"]["value"] > 0 and line["roofline"]["avg_launch_ms"] > 0
    assert line["reference_octree"]["index_rule"]["value"] > 0
