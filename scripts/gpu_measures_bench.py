"""Measures (egg_measure): wall-clock time of a call against what a caller does without it, and
bench.py at two builds in alternating runs.  One JSON line per measurement.

    python scripts/gpu_measures_bench.py [--scenes config3,separate16k] [--ids 1,64,all] [--repeats 30] [--label TEXT]
    python scripts/gpu_measures_bench.py --bench-spread THIS.jsonl PARENT.jsonl [--label TEXT]

scenes: config3 = 4,096 batches, 4 per site (bench.py's, 704,512 particles); separate16k = 16,384 separate batches.  Three
exact-order steps first, so that positions and velocities are no longer the templates.
A list of n ids: batches spread evenly over the scene; `all` is ids=None, every live batch.  measure_table() (the records
copied back into a numpy array) and measure_to() (the records left in a torch tensor on the device) are timed: the median
and the minimum of `repeats` calls after 3 warm-up calls.
The YARDSTICK is what a caller does on a build without measures, once: download x, y, vx, vy, radius and inv_mass of both
types (and batch_id, to find the atoms) and apply the rule in numpy (record_of of tests/measure_model.py) to every requested
atom.  Before anything is timed the device's table is compared with it integer for integer.
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

SCENES = {"config3": (4096, 4), "separate16k": (16384, 1)}


def timed(fn, repeats, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * statistics.median(ts), "min_ms": 1e3 * min(ts), "repeats": repeats}


def scene_handle(scene):
    from egg_fluid_simulation_amd import SimulationHandler
    h = SimulationHandler()
    n, overlap = SCENES[scene]
    xs, ys, _ = grid_positions(n, overlap=overlap)
    h.add_many(xs, ys, 50, 15)
    for _ in range(3):
        h.step(1 / 60, 2, 3)
    return h


def yardstick(h, ids):
    """the caller's way on a build without measures; returns (table, ms)"""
    import measure_model as mm
    t0 = time.perf_counter()
    table = np.zeros((len(ids), 2, 24), dtype=np.int64)
    for w in (0, 1):
        cols = [h.download(w, f) for f in ("x", "y", "vx", "vy", "radius", "inv_mass")]
        bid = h.download(w, "batch_id").astype(np.int64)
        first = np.flatnonzero(np.r_[True, bid[1:] != bid[:-1]])  # (a batch's particles are one run)
        run = {int(bid[a]): (int(a), int(b)) for a, b in zip(first, np.r_[first[1:], bid.size])}
        for k, i in enumerate(ids):
            if i in run:
                a, b = run[i]
                table[k, w] = mm.record_of(*(c[a:b] for c in cols))
    return table, 1e3 * (time.perf_counter() - t0)


def calls(scene, counts, repeats, label):
    import torch
    h = scene_handle(scene)
    every = h.list_ids()
    n_w, n_y = h.get_n_particles()
    for count in counts:
        ids = None if count == "all" else [every[(2 * k + 1) * len(every) // (2 * int(count))] for k in range(int(count))]
        listed = every if ids is None else ids
        want, y_ms = yardstick(h, listed)
        got = h.measure_table(ids)
        assert np.array_equal(got, want), (scene, count)
        out = torch.zeros((len(listed), 2, 24), dtype=torch.int64, device="cuda:0")
        assert h.measure_to(out, ids) == len(listed) and np.array_equal(out.cpu().numpy(), want), (scene, count)
        table = timed(lambda: h.measure_table(ids), repeats)
        to = timed(lambda: h.measure_to(out, ids), repeats)
        named = timed(lambda: h.measure(ids), repeats)
        print(json.dumps({"what": "measure", "name": scene, "particles": n_w + n_y, "batches": len(every), "ids": len(listed),
                          "measure_table": table, "measure_to": to, "measure_named": named, "yardstick_ms": y_ms,
                          "equal_to_yardstick": True, "ratio_table": y_ms / table["median_ms"], "ratio_to": y_ms / to["median_ms"],
                          "label": label}), flush=True)
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
    ap.add_argument("--ids", default="1,64,all")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--bench-spread", nargs=2, default=None)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if a.bench_spread:
        bench_spread(a.bench_spread[0], a.bench_spread[1], a.label)
        return
    import torch
    torch.cuda.init()  # (before libeggsim.so: see tests/conftest.py)
    for scene in a.scenes.split(","):
        calls(scene, a.ids.split(","), a.repeats, a.label)


if __name__ == "__main__":
    main()
