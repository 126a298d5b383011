"""Cover (egg_cover): wall-clock time of a call on every path against the floor of any caller-side
method, the four downloads it would need.  One JSON line per measurement.

    python scripts/gpu_cover_bench.py [--scenes config3,separate16k] [--grids 256,1024] [--scales 1,12] [--zooms 1] [--owners 0,1]
                                      [--paths auto,lanes,wave,direct] [--repeats 20] [--model] [--label TEXT]
    python scripts/gpu_cover_bench.py --bench-spread THIS.jsonl PARENT.jsonl [--label TEXT]

scenes: config3 = 4,096 batches, 4 per site (bench.py's, 704,512 particles); separate16k = 16,384 separate batches; small = 256
batches, 4 per site (for --model).  Three
exact-order steps first, so that the positions are no longer the templates.
A grid of n x n cells spans the box of the scene's particles; with a scale whose discs would exceed 64 cells in radius the
cell grows until they do not (the grid then covers more than the scene).  --zooms z makes the grid span 1 / z of that box about
its centre: the cells are z times finer and a disc's footprint z * z times larger, which is how the footprint sweep behind
EGG_CV_LANES_CELLS is run; the EGGSIM_COVER_* overrides in the environment are recorded with every line.  cover_to() (planes left in torch tensors on the
device) and cover() (planes copied back into numpy) are timed with and without the owner plane, on path auto and on the
forced paths lanes, wave and direct: the median, the minimum and the maximum of `repeats` calls after 3 warm-up calls.
Before anything is timed the four paths are compared with each other, plane for plane.
The FLOOR is what every caller-side method needs first: the downloads of x, y, radius and batch_id of both types, timed alone
in the same run on the same state.  --model also times those downloads plus tests/cover_model.py in numpy, once, and
compares it with the device (minutes per case at these sizes).
--bench-spread reads the JSON lines of bench.py runs at this build and at the parent's (alternating runs, one file each)
and prints the means, the parent's run-to-run spread and whether this build's mean lies inside it."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench import grid_positions  # noqa: E402

SCENES = {"config3": (4096, 4), "separate16k": (16384, 1), "small": (256, 4)}
PATHS = ("auto", "lanes", "wave", "direct")


def timed(fn, repeats, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * statistics.median(ts), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts), "repeats": repeats}


def scene_handle(scene):
    from egg_fluid_simulation_amd import SimulationHandler
    h = SimulationHandler()
    n, overlap = SCENES[scene]
    xs, ys, _ = grid_positions(n, overlap=overlap)
    h.add_many(xs, ys, 50, 15)
    for _ in range(3):
        h.step(1 / 60, 2, 3)
    return h


def downloads(h):
    return [[h.download(w, f) for w in (0, 1)] for f in ("x", "y", "radius", "batch_id")]


def calls(scene, grids, scales, zooms, owners, paths, repeats, model, label):
    import torch
    h = scene_handle(scene)
    n_w, n_y = h.get_n_particles()
    d = downloads(h)
    lo = (min(float(d[0][w].min()) for w in (0, 1)), min(float(d[1][w].min()) for w in (0, 1)))
    hi = (max(float(d[0][w].max()) for w in (0, 1)), max(float(d[1][w].max()) for w in (0, 1)))
    r_max = max(float(d[2][w].max()) for w in (0, 1))
    floor = timed(lambda: downloads(h), repeats)
    overrides = {k: os.environ[k] for k in ("EGGSIM_COVER_TILE_CELLS", "EGGSIM_COVER_LANES_CELLS", "EGGSIM_COVER_WAVES_PER_CU") if k in os.environ}
    for n, scale, zoom in ((n, scale, zoom) for n in grids for scale in scales for zoom in zooms):
        if True:
            # zoom z: the grid spans 1 / z of the scene's box about its centre, so a cell is z times finer
            cell = max((hi[0] - lo[0]) / zoom / n, (hi[1] - lo[1]) / zoom / n, scale * r_max / 63.0)
            origin, shape = (0.5 * (lo[0] + hi[0]) - 0.5 * n * cell, 0.5 * (lo[1] + hi[1]) - 0.5 * n * cell), (n, n)
            base = {"what": "cover", "name": scene, "particles": n_w + n_y, "batches": len(h.list_ids()), "grid": n, "zoom": zoom, "cell": cell,
                    "scale": scale, "disc_cells": scale * r_max / cell, "downloads": floor, "overrides": overrides, "label": label}
            want = h.cover(origin, cell, shape, scale, owner=True, path="direct")
            for path in PATHS[:3]:
                got = h.cover(origin, cell, shape, scale, owner=True, path=path)
                assert np.array_equal(got.cover, want.cover) and np.array_equal(got.owner, want.owner) and got[3:10] == want[3:10], (scene, n, scale, path)
            if model:
                import cover_model as cm
                t0 = time.perf_counter()
                dd = downloads(h)
                ref = cm.cover(origin + (cell,) + shape, scale, dd[0], dd[1], dd[2], dd[3])
                base["downloads_and_model_ms"] = 1e3 * (time.perf_counter() - t0)
                assert np.array_equal(ref[0], want.cover) and np.array_equal(ref[1], want.owner) and tuple(ref[2:]) == tuple(want[3:10])
                base["equal_to_model"] = True
            cover = torch.zeros((2, n, n), dtype=torch.int32, device="cuda:0")
            owner = torch.zeros((2, n, n), dtype=torch.int32, device="cuda:0")
            for with_owner in owners:
                for path in paths:
                    t = h.cover_to(origin, cell, shape, cover, owner if with_owner else None, scale, path=path)
                    to = timed(lambda: h.cover_to(origin, cell, shape, cover, owner if with_owner else None, scale, path=path), repeats)
                    host = timed(lambda: h.cover(origin, cell, shape, scale, owner=with_owner, path=path), repeats) if path == "auto" else None
                    print(json.dumps(dict(base, owner=with_owner, path=path, cover_to=to, cover=host, inside=t.inside, dropped=t.dropped, hits=t.hits,
                                          covered_any=t.covered_any, units=[t.units_lanes, t.units_wave, t.units_direct],
                                          cover_to_faster_than_downloads=to["median_ms"] < floor["median_ms"])), flush=True)
    h.close()


def bench_spread(this_path, parent_path, label):
    def ms(path):
        out = []
        with open(path) as f:
            for line in f:
                line = line.strip()
                if line.startswith("{") and "ms_per_step" in line:
                    out.append(json.loads(line)["ms_per_step"])
        return out
    this, parent = ms(this_path), ms(parent_path)
    lo, hi = min(parent), max(parent)
    mean = statistics.mean(this)
    print(json.dumps({"what": "bench", "this_ms_per_step": this, "parent_ms_per_step": parent, "this_mean": mean,
                      "parent_mean": statistics.mean(parent), "parent_min": lo, "parent_max": hi, "parent_spread": hi - lo,
                      "this_mean_inside_parent_spread": lo <= mean <= hi, "label": label}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="config3,separate16k")
    ap.add_argument("--grids", default="256,1024")
    ap.add_argument("--scales", default="1,12")
    ap.add_argument("--zooms", default="1")
    ap.add_argument("--owners", default="0,1")
    ap.add_argument("--paths", default=",".join(PATHS))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--bench-spread", nargs=2, default=None)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if a.bench_spread:
        bench_spread(a.bench_spread[0], a.bench_spread[1], a.label)
        return
    import torch
    torch.cuda.init()  # (before libeggsim.so: see tests/conftest.py)
    for scene in a.scenes.split(","):
        calls(scene, [int(v) for v in a.grids.split(",")], [float(v) for v in a.scales.split(",")],
              [float(v) for v in a.zooms.split(",")], [bool(int(v)) for v in a.owners.split(",")], a.paths.split(","), a.repeats, a.model, a.label)


if __name__ == "__main__":
    main()
