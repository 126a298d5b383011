"""Probes (egg_probe): wall-clock time of a call against what a caller does without them, the
kernels' own times from a kernel trace, and the sweep of the grid cap.  One JSON line per measurement.

    python scripts/gpu_probes_bench.py [--what calls,sweep,trace] [--scenes config3,separate16k] [--repeats 30]
                                       [--counts 1,8,64] [--workloads reach32,inf,rays] [--label TEXT]
    python scripts/gpu_probes_bench.py --summarise KERNEL_TRACE.csv [--repeats 30] [--counts ...] [--workloads ...]

scenes: config3 = 4,096 batches, 4 per site (bench.py's, 704,512 particles); separate16k = 16,384 separate batches.
calls (exact order, 3 steps so that the positions are no longer the templates): per scene, workload and number of probes,
probe() -- the median and the minimum of `repeats` calls after 3 warm-up calls.  The workloads: `reach32`, points with a
reach of 32 px on a diagonal across the grid; `inf`, the same points with reach = inf; `rays`, segments across the whole
scene.  The YARDSTICK is what a caller does on a build without probes for the same answer: download of x, y, radius and
batch_id of both types and the model's rule in numpy (tests/probe_model.py), on the same state in the same run; its hits
are checked against the call's, field for field.  The yardstick's repeats are a fifth of the call's.
sweep: the `inf` workload of config3 only, for the grid cap this process runs with (EGGSIM_PROBE_WAVES_PER_CU, read at
every call, as every such override is: one process per value still keeps the values' records apart).
trace: exactly `repeats` calls per (scene config3, workload, count) and nothing else that launches a probe kernel, to be
run under a kernel trace; --summarise reads the trace's CSV back, cuts the probe kernels' records into those groups by their
order and prints the median time of the scan and of the finishing kernel per group."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench import grid_positions  # noqa: E402

SCENES = {"config3": (4096, 4), "separate16k": (16384, 1)}
INF = float("inf")


def probes_of(workload, n, xs, ys):
    lo_x, hi_x, lo_y, hi_y = float(min(xs)), float(max(xs)), float(min(ys)), float(max(ys))
    at = [(lo_x + (hi_x - lo_x) * (k + 0.5) / n, lo_y + (hi_y - lo_y) * (k + 0.5) / n) for k in range(n)]
    if workload == "reach32":
        return [("point", x + 3.0, y - 2.0, 32.0) for x, y in at]
    if workload == "inf":
        return [("point", x + 3.0, y - 2.0) for x, y in at]
    return [("ray", lo_x - 100.0, y, hi_x + 100.0, y + 37.0, 0.5) for _, y in at]


def numpy_probe(h, probes):
    """the caller's way to probe(): eight downloads and the model's rule in numpy"""
    import probe_model as pm
    parts = []
    for w in (0, 1):
        x, y, r, b = (h.download(w, f) for f in ("x", "y", "radius", "batch_id"))
        parts.append(pm.particles_of(x, y, r, b, _Identity()))  # (batches added in one go: a batch's key is its id)
    return pm.probe(probes, parts)


class _Identity(dict):
    def __missing__(self, k):
        return k


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
    ids = h.add_many(xs, ys, 50, 15)
    for _ in range(3):
        h.step(1 / 60, 2, 3)
    return h, xs, ys, [int(i) for i in ids]


def plain(hits):
    return [tuple(None if t is None else tuple(t) for t in pair) for pair in hits]


def calls(scene, workloads, counts, repeats, label, yardstick=True):
    h, xs, ys, ids = scene_handle(scene)
    n_w, n_y = h.get_n_particles()
    base = {"name": scene, "particles": n_w + n_y, "batches": len(ids), "label": label,
            "waves_per_cu": os.environ.get("EGGSIM_PROBE_WAVES_PER_CU", "default")}
    for workload in workloads:
        for n in counts:
            probes = probes_of(workload, n, xs, ys)
            got = plain(h.probe(probes))
            found = sum(1 for pair in got for t in pair if t is not None)
            t = timed(lambda: h.probe(probes), repeats)
            row = dict(base, what="probe", workload=workload, probes=n, found=found, call=t)
            if yardstick:
                assert got == numpy_probe(h, probes), (scene, workload, n)
                y = timed(lambda: numpy_probe(h, probes), max(3, repeats // 5), warm=1)
                row.update(yardstick=y, ratio=y["median_ms"] / t["median_ms"])
            print(json.dumps(row), flush=True)
    h.close()


def trace(workloads, counts, repeats):
    h, xs, ys, _ids = scene_handle("config3")
    for workload in workloads:
        for n in counts:
            probes = probes_of(workload, n, xs, ys)
            for _ in range(repeats):
                h.probe(probes)
    h.close()


def summarise(path, workloads, counts, repeats, label):
    rows = {"egg_probe_scan_kernel": [], "egg_probe_finish_kernel": []}
    with open(path, newline="") as f:
        for rec in csv.DictReader(f):
            name = rec["Kernel_Name"].split("(")[0].strip()
            if name in rows:
                rows[name].append((int(rec["Start_Timestamp"]), int(rec["End_Timestamp"]) - int(rec["Start_Timestamp"])))
    groups = [(w, n) for w in workloads for n in counts]
    for name in rows:
        rows[name].sort()
        assert len(rows[name]) == repeats * len(groups), (name, len(rows[name]))
    for g, (workload, n) in enumerate(groups):
        scan = [d for _, d in rows["egg_probe_scan_kernel"][g * repeats:(g + 1) * repeats]]
        finish = [d for _, d in rows["egg_probe_finish_kernel"][g * repeats:(g + 1) * repeats]]
        print(json.dumps({"name": "config3", "what": "kernels", "workload": workload, "probes": n, "calls": repeats,
                          "scan_us": statistics.median(scan) / 1e3, "finish_us": statistics.median(finish) / 1e3,
                          "finish_share": statistics.median(finish) / (statistics.median(scan) + statistics.median(finish)),
                          "label": label}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="calls")
    ap.add_argument("--scenes", default="config3,separate16k")
    ap.add_argument("--workloads", default="reach32,inf,rays")
    ap.add_argument("--counts", default="1,8,64")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    workloads, counts = a.workloads.split(","), [int(c) for c in a.counts.split(",")]
    if a.summarise:
        summarise(a.summarise, workloads, counts, a.repeats, a.label)
        return
    what = a.what.split(",")
    if "calls" in what:
        for scene in a.scenes.split(","):
            calls(scene, workloads, counts, a.repeats, a.label)
    if "sweep" in what:
        calls("config3", ["inf"], counts, a.repeats, a.label, yardstick=False)
    if "trace" in what:
        trace(workloads, counts, a.repeats)


if __name__ == "__main__":
    main()
