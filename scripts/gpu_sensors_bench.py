"""Sensors (egg_set_sensors): wall-clock time of a read against what a caller does without them, and
the step time with a list set and never read.  One JSON line per measurement.

    python scripts/gpu_sensors_bench.py [--what reads,steps] [--scenes config3,separate16k] [--repeats 30] [--steps 200]
                                        [--warmup 30] [--modes unset,set] [--package-root DIR] [--label TEXT]

scenes: config3 = 4,096 batches, 4 per site (bench.py's, 704,512 particles); separate16k = 16,384 separate batches.
reads (exact order, 3 steps so that the positions are no longer the templates): per scene, sensor_sums() with 1, 8 and 64 disc
sensors spread over the grid, and sensor_batches over 1, 256 and all ids with 8 sensors -- the median and the minimum of
`repeats` calls after 3 warm-up calls.  The YARDSTICK is what a caller does on a build without sensors for the same answer:
download(w, "x"), download(w, "y") -- and download(w, "batch_id") for the per-batch counts -- of both types, and the rule in
vectorised numpy (`numpy_sums`, `numpy_batches`), on the same state in the same run; its integers are checked against the
read's.  The yardstick's repeats are a fifth of the read's (it is some hundred times slower).
steps: ms per step over a steady window with the list never set (`unset`, the only mode an earlier commit has) and with 64
sensors set and never read (`set`); --package-root imports the package from another checkout (mode unset only), so that two
builds can be compared in one session, alternating.
The grid cap's developer override (EGGSIM_SENSOR_WAVES_PER_CU) is read at every call, as every such override is."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import grid_positions  # noqa: E402

SCENES = {"config3": (4096, 4), "separate16k": (16384, 1)}
SCALE = 65536.0


def discs(n, xs, ys):
    """n disc sensors of radius 120 px on a diagonal across the grid"""
    lo_x, hi_x, lo_y, hi_y = float(min(xs)), float(max(xs)), float(min(ys)), float(max(ys))
    return [("disc", lo_x + (hi_x - lo_x) * (k + 0.5) / n, lo_y + (hi_y - lo_y) * (k + 0.5) / n, 120.0) for k in range(n)]


def numpy_masks(sensors, x, y):
    for _kind, cx, cy, R in sensors:
        dx = x - cx
        dy = y - cy
        yield dx * dx + dy * dy <= R * R


def numpy_sums(h, sensors):
    """the caller's way to sensor_sums() for disc sensors on in-range positions: four downloads and numpy"""
    out = [[], []]
    for w in (0, 1):
        x, y = h.download(w, "x"), h.download(w, "y")
        qx, qy = np.rint(x * SCALE).astype(np.int64), np.rint(y * SCALE).astype(np.int64)
        for m in numpy_masks(sensors, x, y):
            out[w].append((int(np.count_nonzero(m)), int(qx[m].sum()), int(qy[m].sum())))
    return [(a, b) for a, b in zip(out[0], out[1])]


def numpy_batches(h, sensors, ids):
    """the caller's way to sensor_batches(ids): six downloads and numpy"""
    out = np.zeros((len(ids), len(sensors), 2), dtype=np.int32)
    ids = np.asarray(ids, dtype=np.int64)
    for w in (0, 1):
        x, y, b = h.download(w, "x"), h.download(w, "y"), h.download(w, "batch_id").astype(np.int64)
        for k, m in enumerate(numpy_masks(sensors, x, y)):
            per_id = np.bincount(b[m], minlength=int(ids.max()) + 1)
            out[:, k, w] = per_id[ids]
    return out


def timed(fn, repeats, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * statistics.median(ts), "min_ms": 1e3 * min(ts), "repeats": repeats}


def scene_handle(scene, order="exact"):
    from egg_fluid_simulation_amd import SimulationHandler
    h = SimulationHandler()
    n, overlap = SCENES[scene]
    xs, ys, _ = grid_positions(n, overlap=overlap)
    if order == "relaxed":
        h.set_solver_order("relaxed")
        h.set_colliders([("half_plane", 0.0, -1.0, -(float(max(ys)) + 200.0))])
        h.set_forces([("uniform", 0.0, 980.0)])
    ids = h.add_many(xs, ys, 50, 15)
    return h, xs, ys, [int(i) for i in ids]


def reads(scene, repeats, label):
    h, xs, ys, ids = scene_handle(scene)
    for _ in range(3):
        h.step(1 / 60, 2, 3)
    n_w, n_y = h.get_n_particles()
    base = {"name": scene, "particles": n_w + n_y, "batches": len(ids), "label": label}
    for n in (1, 8, 64):
        sensors = discs(n, xs, ys)
        h.set_sensors(sensors)
        got = h.sensor_sums()
        assert got[0] == numpy_sums(h, sensors) and got[1] == [0, 0]
        t = timed(h.sensor_sums, repeats)
        y = timed(lambda: numpy_sums(h, sensors), max(3, repeats // 5), warm=1)
        inside = sum(per_type[w][0] for per_type in got[0] for w in (0, 1))
        print(json.dumps(dict(base, what="sensor_sums", sensors=n, inside=inside, read=t, yardstick=y,
                              ratio=y["median_ms"] / t["median_ms"])), flush=True)
    sensors = discs(8, xs, ys)
    h.set_sensors(sensors)
    for m in (1, 256, len(ids)):
        pick = ids[:: max(1, len(ids) // m)][:m]
        assert np.array_equal(h.sensor_batches(pick), numpy_batches(h, sensors, pick))
        t = timed(lambda: h.sensor_batches(pick), repeats)
        y = timed(lambda: numpy_batches(h, sensors, pick), max(3, repeats // 5), warm=1)
        print(json.dumps(dict(base, what="sensor_batches", sensors=8, ids=len(pick), read=t, yardstick=y,
                              ratio=y["median_ms"] / t["median_ms"])), flush=True)
    h.close()


def steps(scene, order, mode, n_steps, warmup, label):
    h, xs, ys, _ids = scene_handle(scene, order)
    if mode == "set":
        h.set_sensors(discs(64, xs, ys))
    for _ in range(warmup):
        h.step(1 / 60, 2, 3)
    h.synchronize()
    s0 = h.stats()
    t0 = time.perf_counter()
    for _ in range(n_steps):
        h.step(1 / 60, 2, 3)
    h.synchronize()
    dt = time.perf_counter() - t0
    s1 = h.stats()
    print(json.dumps({"name": scene, "what": "step", "order": order, "mode": mode, "steps": n_steps, "warmup": warmup,
                      "ms_per_step": 1e3 * dt / n_steps, "launches_per_step": (s1["kernel_launches"] - s0["kernel_launches"]) / n_steps,
                      "label": label}), flush=True)
    h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="reads,steps")
    ap.add_argument("--scenes", default="config3,separate16k")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--modes", default="unset,set")
    ap.add_argument("--orders", default="exact,relaxed")
    ap.add_argument("--package-root", default=None)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if a.package_root:
        sys.path.insert(0, os.path.abspath(a.package_root))
    for scene in a.scenes.split(","):
        if "reads" in a.what.split(","):
            reads(scene, a.repeats, a.label)
        if "steps" in a.what.split(","):
            for order in a.orders.split(","):
                for mode in a.modes.split(","):
                    steps(scene, order, mode, a.steps, a.warmup, a.label)


if __name__ == "__main__":
    main()
