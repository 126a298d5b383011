"""Fields (egg_field): wall-clock time of a call against what a caller does without them, the
kernel's own time from a kernel trace, and the sweeps of the grid cap and of the tile size.  One JSON line per measurement.

    python scripts/gpu_fields_bench.py [--what calls,sweep,trace] [--scenes config3,separate16k] [--repeats 30]
                                       [--grids 64,256,1024,fine] [--label TEXT]
    python scripts/gpu_fields_bench.py --summarise KERNEL_TRACE.csv [--repeats 30] [--grids ...]

scenes: config3 = 4,096 batches, 4 per site (bench.py's, 704,512 particles); separate16k = 16,384 separate batches.
grids: `64`, `256`, `1024` = that many cells per side over the scene's bounding box (cells coarser than a particle at
64, about a particle at 1,024); `fine` = 1,024 x 1,024 cells of 1 px around the scene's centre (finer than a particle;
the particles beyond it are outside); `away` (trace only) = a 256 x 256 grid that holds no particle, so that the kernel
runs its first pass and nothing else.
calls (exact order, 3 steps so that the positions are no longer the templates): per scene, grid, with and without
velocities, path auto and direct, field() and field_to() into torch tensors -- the median and the minimum of `repeats`
calls after 3 warm-up calls.  The YARDSTICK is what a caller does on a build without fields for the same planes: the
downloads of x, y (and vx, vy) of both types and the model's rule in numpy (tests/field_model.py: np.add.at), on the same
state in the same run; its planes are checked against the call's, integer for integer.  The yardstick runs 3 times.
sweep: field_to() per scene with velocities at `256` and `fine`, for EGGSIM_FIELD_WAVES_PER_CU in 1 .. 32 and
EGGSIM_FIELD_TILE_CELLS in 0 .. 1,024 (both read at every call).
trace: exactly `repeats` calls of field_to() per (scene config3, grid, velocity, path) and nothing else that launches a
field kernel, to be run under a kernel trace; --summarise reads the trace's CSV back, cuts the field kernels' records into
those groups by their order and prints the median kernel time per group and, against the `away` grid of the same
instantiation, the share of the time that the second pass and its atomics take."""
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
KERNELS = {False: "egg_field_count_kernel", True: "egg_field_velocity_kernel"}


def grid_of(name, xs, ys):
    """(x0, y0, cell, nx, ny)"""
    lo_x, hi_x, lo_y, hi_y = float(min(xs)) - 60.0, float(max(xs)) + 60.0, float(min(ys)) - 60.0, float(max(ys)) + 60.0
    if name == "fine":
        return (0.5 * (lo_x + hi_x) - 512.0, 0.5 * (lo_y + hi_y) - 512.0, 1.0, 1024, 1024)
    if name == "away":
        return (hi_x + 1000.0, hi_y + 1000.0, 1.0, 256, 256)
    n = int(name)
    return (lo_x, lo_y, max(hi_x - lo_x, hi_y - lo_y) / n, n, n)


def numpy_field(h, grid, velocity):
    """the caller's way to field(): four to eight downloads and the model's rule in numpy"""
    import field_model as fm
    d = [[h.download(w, f) for w in (0, 1)] for f in (("x", "y", "vx", "vy") if velocity else ("x", "y"))]
    return fm.field(grid, d[0], d[1], d[2] if velocity else None, d[3] if velocity else None, "both", velocity)


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


def tensors(grid, velocity):
    import torch
    shape = (2, grid[4], grid[3])
    count = torch.zeros(shape, dtype=torch.int32, device="cuda:0")
    return (count,) + ((torch.zeros(shape, dtype=torch.int64, device="cuda:0"), torch.zeros(shape, dtype=torch.int64, device="cuda:0"))
                       if velocity else (None, None))


def env_label():
    return {"waves_per_cu": os.environ.get("EGGSIM_FIELD_WAVES_PER_CU", "default"), "tile_cells": os.environ.get("EGGSIM_FIELD_TILE_CELLS", "default")}


def calls(scene, grids, repeats, label):
    h, xs, ys, ids = scene_handle(scene)
    n_w, n_y = h.get_n_particles()
    base = dict({"name": scene, "particles": n_w + n_y, "batches": len(ids), "label": label}, **env_label())
    for name in grids:
        grid = grid_of(name, xs, ys)
        origin, cell, shape = grid[:2], grid[2], grid[3:]
        for velocity in (False, True):
            want = numpy_field(h, grid, velocity)
            y = timed(lambda: numpy_field(h, grid, velocity), 3, warm=0)
            for path in ("auto", "direct"):
                f = h.field(origin, cell, shape, "both", velocity, path)
                assert all((a is None and b is None) or (a == b).all() for a, b in zip(f[:3], want[:3])) and tuple(f[3:6]) == tuple(want[3:]), (scene, name)
                t = timed(lambda: h.field(origin, cell, shape, "both", velocity, path), repeats)
                planes = tensors(grid, velocity)
                t_to = timed(lambda: h.field_to(origin, cell, shape, *planes, path=path), repeats)
                assert (planes[0].cpu().numpy() == want[0]).all()
                print(json.dumps(dict(base, what="field", grid=name, cell_px=cell, cells=shape[0] * shape[1], velocity=velocity, path=path,
                                      inside=f.inside, outside=f.outside, units_tiled=f.units_tiled, units_direct=f.units_direct,
                                      field=t, field_to=t_to, yardstick=y, ratio=y["median_ms"] / t["median_ms"],
                                      ratio_to=y["median_ms"] / t_to["median_ms"])), flush=True)
    h.close()


def sweep(scene, grids, repeats, label):
    h, xs, ys, _ids = scene_handle(scene)
    for name in grids:
        grid = grid_of(name, xs, ys)
        planes = tensors(grid, True)
        for key, values in (("EGGSIM_FIELD_WAVES_PER_CU", (1, 2, 4, 8, 16, 32)), ("EGGSIM_FIELD_TILE_CELLS", (0, 16, 64, 256, 1024))):
            for v in values:
                os.environ[key] = str(v)
                t = timed(lambda: h.field_to(grid[:2], grid[2], grid[3:], *planes), repeats)
                f = h.field_to(grid[:2], grid[2], grid[3:], *planes)
                print(json.dumps(dict({"name": scene, "what": "sweep", "grid": name, "velocity": True, "label": label, "field_to": t,
                                       "units_tiled": f.units_tiled, "units_direct": f.units_direct}, **env_label())), flush=True)
            del os.environ[key]
    h.close()


def trace_groups(grids):
    return [(g, v, p) for g in list(grids) + ["away"] for v in (False, True) for p in ("auto", "direct")]


def trace(grids, repeats):
    h, xs, ys, _ids = scene_handle("config3")
    for name, velocity, path in trace_groups(grids):
        grid = grid_of(name, xs, ys)
        planes = tensors(grid, velocity)
        for _ in range(repeats):
            h.field_to(grid[:2], grid[2], grid[3:], *planes, path=path)
    h.close()


def summarise(path, grids, repeats, label):
    rows = []
    with open(path, newline="") as f:
        for rec in csv.DictReader(f):
            name = rec["Kernel_Name"].split("(")[0].strip()
            if name in KERNELS.values():
                rows.append((int(rec["Start_Timestamp"]), name, int(rec["End_Timestamp"]) - int(rec["Start_Timestamp"])))
    rows.sort()
    groups = trace_groups(grids)
    assert len(rows) == repeats * len(groups), len(rows)
    med = {}
    for g, key in enumerate(groups):
        part = rows[g * repeats:(g + 1) * repeats]
        assert all(name == KERNELS[key[1]] for _, name, _ in part), key
        med[key] = statistics.median(d for _, _, d in part) / 1e3
    for name, velocity, path in groups:
        first_pass = med[("away", velocity, path)]
        us = med[(name, velocity, path)]
        print(json.dumps({"name": "config3", "what": "kernel", "grid": name, "velocity": velocity, "path": path, "calls": repeats, "kernel_us": us,
                          "first_pass_only_us": first_pass, "second_pass_and_atomics_share": max(0.0, 1.0 - first_pass / us), "label": label}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="calls")
    ap.add_argument("--scenes", default="config3,separate16k")
    ap.add_argument("--grids", default="64,256,1024,fine")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    grids = a.grids.split(",")
    if a.summarise:
        summarise(a.summarise, grids, a.repeats, a.label)
        return
    what = a.what.split(",")
    import torch
    torch.cuda.init()  # (before libeggsim.so: see tests/conftest.py; field_to's planes are torch tensors)
    if "calls" in what:
        for scene in a.scenes.split(","):
            calls(scene, grids, a.repeats, a.label)
    if "sweep" in what:
        for scene in a.scenes.split(","):
            sweep(scene, [g for g in grids if g in ("256", "fine")] or grids, a.repeats, a.label)
    if "trace" in what:
        trace(grids, a.repeats)


if __name__ == "__main__":
    main()
