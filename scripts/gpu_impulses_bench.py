"""Impulses (egg_impulse): wall-clock time of a call against what a caller does without it, and
bench.py at two builds in alternating runs.  One JSON line per measurement.

    python scripts/gpu_impulses_bench.py [--scenes config3,separate16k] [--records 1,8,64] [--repeats 30] [--label TEXT]
    python scripts/gpu_impulses_bench.py --bench-spread THIS.jsonl PARENT.jsonl [--label TEXT]

scenes: config3 = 4,096 batches, 4 per site (bench.py's, 704,512 particles); separate16k = 16,384 separate batches.  Three
exact-order steps first, so that positions and velocities are no longer the templates.
A list of n records: record k is a disc of radius 120 px around a site of the scene (the sites spread evenly over it), with
the four actions and the two weights in turn.  impulse() is timed with and without results: the median and the minimum of
`repeats` calls after 3 warm-up calls (every call edits the velocities the call before it left; that changes no cost).
The YARDSTICK is what a caller does on a build without impulses, once, on a second handle built the same way: download x, y
and batch_id to find the batches a region touches, export each of them, apply the rule in numpy (tests/impulse_model.py),
remove the batch and import it again at its key.  Before anything is timed the subject takes the same list once, and all six
fields of every particle of both handles are compared bit for bit, the totals integer for integer.
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
FIELDS = ("x", "y", "vx", "vy", "last_x", "last_y")
RADIUS = 120.0


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
    return h, np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)


def records_of(n, xs, ys):
    """n records around sites spread evenly over the scene: kick, blast, swirl, brake in turn, flat / linear / by inverse mass"""
    out = []
    for k in range(n):
        j = (2 * k + 1) * xs.size // (2 * n)
        cx, cy = float(xs[j]), float(ys[j])
        disc = ("disc", cx, cy, RADIUS)
        if k % 4 == 0:
            out.append(("kick", disc, 3.0, -2.0, dict(by_inv_mass=k % 8 == 0)))
        elif k % 4 == 1:
            out.append(("blast", disc, cx, cy, 40.0, dict(linear=True)))
        elif k % 4 == 2:
            out.append(("swirl", disc, cx, cy, 0.5, dict(linear=k % 8 == 2)))
        else:
            out.append(("brake", disc, 0.0, 0.0, 0.25))
    return out


def yardstick(h, records):
    """the caller's way on a build without impulses; returns (touched batches, ms)"""
    import impulse_model as im
    t0 = time.perf_counter()
    canon = im.canonical(records)
    touched = set()
    for w in (0, 1):
        x, y, bid = (h.download(w, f) for f in ("x", "y", "batch_id"))
        for rec in canon:
            ins, _, _ = im._test(rec[1], x, y)
            touched.update(int(i) for i in np.unique(bid[ins]))
    for i in sorted(touched):
        info, ws, ys = h.export_batch(i)
        bid = [np.full(ws.shape[1], i, dtype=np.int64), np.full(ys.shape[1], i, dtype=np.int64)]
        nvx, nvy, _ = im.apply(records, [ws[0], ys[0]], [ws[1], ys[1]], [ws[2], ys[2]], [ws[3], ys[3]], [ws[6], ys[6]], bid)
        ws[2], ws[3], ys[2], ys[3] = nvx[0], nvy[0], nvx[1], nvy[1]
        h.remove(i)
        h.import_batch(info, ws, ys)
    return len(touched), 1e3 * (time.perf_counter() - t0)


def calls(scene, counts, repeats, label):
    import impulse_model as im
    for n in counts:
        h, xs, ys = scene_handle(scene)
        twin, _, _ = scene_handle(scene)
        n_w, n_y = h.get_n_particles()
        records = records_of(n, xs, ys)
        cols = [[h.download(w, f) for w in (0, 1)] for f in ("x", "y", "vx", "vy", "inv_mass")]
        bid = [h.download(w, "batch_id").astype(np.int64) for w in (0, 1)]
        _, _, want = im.apply(records, *cols, bid)
        got = h.impulse(records)
        assert [tuple(r) for r in got] == want, (scene, n)
        touched, y_ms = yardstick(twin, records)
        equal = all(np.array_equal(h.download(w, f).view(np.uint64), twin.download(w, f).view(np.uint64)) for w in (0, 1) for f in FIELDS)
        assert equal, (scene, n)
        twin.close()
        n_arr, arr = h._c_impulses(records)
        with_results = timed(lambda: h._impulse_table(n_arr, arr, True), repeats)
        named = timed(lambda: h.impulse(records), repeats)
        without = timed(lambda: h._impulse_table(n_arr, arr, False), repeats)
        print(json.dumps({"what": "impulse", "name": scene, "particles": n_w + n_y, "batches": int(xs.size), "records": n,
                          "edited": [sum(r.count[w] for r in got) for w in (0, 1)], "touched_batches": touched,
                          "with_results": with_results, "with_results_named": named, "without_results": without, "yardstick_ms": y_ms,
                          "bit_equal_to_yardstick": equal, "ratio_with_results": y_ms / with_results["median_ms"],
                          "ratio_without_results": y_ms / without["median_ms"], "label": label}), flush=True)
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
    ap.add_argument("--records", default="1,8,64")
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
        calls(scene, [int(v) for v in a.records.split(",")], a.repeats, a.label)


if __name__ == "__main__":
    main()
