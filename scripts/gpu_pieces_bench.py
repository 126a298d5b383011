"""Pieces (egg_pieces): wall-clock time of a call against what a caller does without it, the kernels'
own time from a kernel trace, the number of sweeps, the sweep of the workgroup cap, and the wall experiment.  One JSON line
per measurement.

    python scripts/gpu_pieces_bench.py [--what calls,big,sweeps,cap,trace,experiment] [--scenes config3,separate16k]
                                       [--repeats 30] [--label TEXT]
    python scripts/gpu_pieces_bench.py --summarise KERNEL_TRACE.csv [--repeats 30]
    python scripts/gpu_pieces_bench.py --what reach      (no device: the CPU models)

scenes: config3 = 4,096 batches, 4 per site (bench.py's, 704,512 particles); separate16k = 16,384 separate batches.
calls (exact order, 3 steps so that the positions are no longer the templates): pieces() for every id and for one id, and
piece_labels(), with the default reach -- the median and the minimum of `repeats` calls after 3 warm-up calls.  The YARDSTICK
is what a caller does on a build without pieces: the downloads of x, y, radius and batch_id of both types and the model's
rule in numpy (tests/pieces_model.py) per atom, on the same state in the same run; its records and labels are checked
against the call's, integer for integer.  The yardstick runs once.
big: one batch whose white is one atom of 4,096 particles, alone on the handle.
sweeps: EGGSIM_PIECES_SWEEPS makes the library print the sweeps of a call's atoms on stderr; the scenes are one fresh default
egg, four default eggs after five steps, config 3, and the two chains of 300 of the hand table.
cap: pieces() for every id per scene, for EGGSIM_PIECES_GROUPS_PER_CU in 1 .. 32 (read at every call).
trace: exactly `repeats` calls per group and nothing else that launches a pieces kernel, to be run under a kernel trace;
--summarise reads the trace's CSV back and prints the median kernel time per group.
experiment: relaxed order, one default egg held at its target (300, 300), a vertical wall that starts at x = 240 and crosses
the egg at 540 px/s for 30 steps, then stands still for 60 more; pieces() per step.
reach: the smallest reach that makes one default egg one piece, per step, on the CPU models of both solver orders."""
import argparse
import csv
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
KERNELS = ("egg_pieces_wave_kernel", "egg_pieces_block_kernel")
TRACE_GROUPS = (("config3, every id", "egg_pieces_wave_kernel"), ("config3, one id", "egg_pieces_wave_kernel"),
                ("one default egg", "egg_pieces_wave_kernel"), ("one atom of 4,096", "egg_pieces_block_kernel"),
                ("one atom of 4,096, its yolk", "egg_pieces_wave_kernel"))


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
    return h, [int(i) for i in ids]


def big_handle():
    from egg_fluid_simulation_amd import SimulationHandler
    h = SimulationHandler()
    i = h.add(300.0, 300.0, 50, 15, None, None, 4096, 12)
    for _ in range(3):
        h.step(1 / 60, 2, 3)
    return h, i


def numpy_pieces(h, ids, reach, labels):
    """the caller's way to pieces(): eight downloads and the model's rule in numpy, atom by atom"""
    import pieces_model as pm
    records = {}
    out_labels = []
    for w in (0, 1):
        x, y, r, bid = (h.download(w, f) for f in ("x", "y", "radius", "batch_id"))
        starts = np.concatenate(([0], np.flatnonzero(np.diff(bid)) + 1, [bid.size])) if bid.size else np.zeros(1, dtype=np.int64)
        where = {int(bid[a]): (int(a), int(b)) for a, b in zip(starts[:-1], starts[1:])}
        lab_all = np.full(bid.size, -1, dtype=np.int32)
        for i in (where if labels else ids):
            if i not in where:
                records[i, w] = pm.ZERO
                continue
            a, b = where[i]
            lab = pm.labels_of(x[a:b], y[a:b], r[a:b], reach[w])
            lab_all[a:b] = lab
            records[i, w] = pm.record_of(x[a:b], y[a:b], lab)
        out_labels.append(lab_all)
    return [(records[i, 0], records[i, 1]) for i in ids], out_labels


def raw(h, ids, reach):
    return [tuple(tuple(int(v) for v in rec) for rec in pair)
            for pair in h._piece_table(h._c_pieces_spec(reach, "both"), None if ids is None else np.ascontiguousarray(ids, dtype=np.int64))]


def calls(scene, repeats, label):
    h, ids = scene_handle(scene)
    n_w, n_y = h.get_n_particles()
    spec = h._c_pieces_spec(None, "both")
    reach = (spec.reach[0], spec.reach[1])
    base = {"name": scene, "particles": n_w + n_y, "batches": len(ids), "reach": reach, "label": label,
            "groups_per_cu": os.environ.get("EGGSIM_PIECES_GROUPS_PER_CU", "default")}
    one = [ids[len(ids) // 2]]
    t0 = time.perf_counter()
    want, want_labels = numpy_pieces(h, ids, reach, True)
    y_all = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    want_one, _ = numpy_pieces(h, one, reach, False)
    y_one = 1e3 * (time.perf_counter() - t0)
    assert raw(h, None, None) == want and raw(h, one, None) == want_one, scene
    got_labels = h.piece_labels()
    assert all(np.array_equal(a, b) for a, b in zip(got_labels, want_labels)), scene
    whole = sum(1 for pair in want if all(r[1] == 1 for r in pair))
    t_all = timed(lambda: h.pieces(), repeats)
    t_raw = timed(lambda: h._piece_table(spec, None), repeats)
    t_one = timed(lambda: h.pieces(one), repeats)
    t_lab = timed(lambda: h.piece_labels(), repeats)
    print(json.dumps(dict(base, what="pieces", whole_batches=whole, largest_atom=max(r[0] for pair in want for r in pair),
                          every_id=t_all, every_id_records_only=t_raw, one_id=t_one, labels=t_lab,
                          yardstick_every_id_with_labels_ms=y_all, yardstick_one_id_ms=y_one,
                          ratio_every_id=y_all / t_all["median_ms"], ratio_one_id=y_one / t_one["median_ms"],
                          ratio_labels=y_all / t_lab["median_ms"])), flush=True)
    h.close()


def big(repeats, label):
    h, i = big_handle()
    spec = h._c_pieces_spec(None, "both")
    reach = (spec.reach[0], spec.reach[1])
    t0 = time.perf_counter()
    want, want_labels = numpy_pieces(h, [i], reach, True)
    y = 1e3 * (time.perf_counter() - t0)
    assert raw(h, None, None) == want and all(np.array_equal(a, b) for a, b in zip(h.piece_labels(), want_labels))
    for r in (None, 1.0, 0.5):
        t = timed(lambda: h.pieces(None, r), repeats)
        print(json.dumps({"name": "one atom of 4,096", "what": "big", "reach": r, "record": raw(h, None, r)[0][0], "pieces": t,
                          "white_only": timed(lambda: h.pieces(None, r, "white"), repeats), "yardstick_ms": y if r is None else None,
                          "label": label}), flush=True)
    h.close()


def chain_handle(order):
    """the chains of 300 of the hand table (tests/test_pieces_model.py), placed through export_batch / import_batch"""
    import warnings

    from egg_fluid_simulation_amd import EggWarning, SimulationHandler
    src = SimulationHandler()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", EggWarning)
        i = src.add(0.0, 0.0, 50, 15, None, None, 300, 2)
    info, ws, ys = src.export_batch(i)
    for p in range(300):
        ws[0, order[p]] = ws[4, order[p]] = 7.0 * p
        ws[1, order[p]] = ws[5, order[p]] = 0.0
        ws[2, order[p]] = ws[3, order[p]] = 0.0
        ws[7, order[p]] = 4.0
    h = SimulationHandler()
    h.import_batch(dict(info, key=1), ws, ys)
    src.close()
    return h


def sweeps(label):
    from egg_fluid_simulation_amd import SimulationHandler
    os.environ["EGGSIM_PIECES_SWEEPS"] = "1"

    def say(name, h, reach, types="both"):
        print(json.dumps({"what": "sweeps", "name": name, "reach": reach, "types": types, "label": label,
                          "note": "the next stderr line `egg_pieces sweeps:` belongs to this call"}), flush=True)
        sys.stderr.flush()
        h.pieces(None, reach, types)
        sys.stderr.flush()
    h = SimulationHandler()
    h.add(300.0, 300.0)
    say("one fresh default egg", h, None)
    say("one fresh default egg", h, 1.0)
    h.close()
    h = SimulationHandler()
    for x, y in ((300.0, 300.0), (360.0, 310.0), (330.0, 250.0), (420.0, 330.0)):
        h.add(x, y)
    for _ in range(5):
        h.update(1 / 60, 1 / 60, 2, 3)
    say("four default eggs after five steps", h, None)
    say("four default eggs after five steps", h, 1.0)
    h.close()
    h, _ = scene_handle("config3")
    say("config3", h, None)
    say("config3", h, 1.0)
    h.close()
    for name, order in (("chain of 300, index 0 at the far end", [299 - p for p in range(300)]),
                        ("chain of 300 in snake order", [p // 2 if p % 2 == 0 else 299 - p // 2 for p in range(300)]),
                        ("chain of 300, index = position", list(range(300)))):
        h = chain_handle(order)
        say(name, h, 1.0, "white")
        h.close()
    h, _ = big_handle()
    say("one atom of 4,096", h, None, "white")
    say("one atom of 4,096", h, 0.5, "white")
    h.close()
    del os.environ["EGGSIM_PIECES_SWEEPS"]


def cap(scene, repeats, label):
    h, _ids = scene_handle(scene)
    spec = h._c_pieces_spec(None, "both")
    for v in (1, 2, 4, 8, 16, 32):
        os.environ["EGGSIM_PIECES_GROUPS_PER_CU"] = str(v)
        t = timed(lambda: h._piece_table(spec, None), repeats)
        print(json.dumps({"name": scene, "what": "cap", "groups_per_cu": v, "every_id_records_only": t, "label": label}), flush=True)
    del os.environ["EGGSIM_PIECES_GROUPS_PER_CU"]
    h.close()


def trace(repeats):
    from egg_fluid_simulation_amd import SimulationHandler
    h, ids = scene_handle("config3")
    spec = h._c_pieces_spec(None, "both")
    one = np.ascontiguousarray([ids[len(ids) // 2]], dtype=np.int64)
    for _ in range(repeats):
        h._piece_table(spec, None)
    for _ in range(repeats):
        h._piece_table(spec, one)
    h.close()
    h = SimulationHandler()
    h.add(300.0, 300.0)
    for _ in range(repeats):
        h._piece_table(spec, None)
    h.close()
    h, _ = big_handle()
    for _ in range(repeats):  # (two launches per call: the white atom in the block class, the yolk atom in the wave class)
        h._piece_table(spec, None)
    h.close()


def summarise(path, repeats, label):
    rows = []
    with open(path, newline="") as f:
        for rec in csv.DictReader(f):
            name = rec["Kernel_Name"].split("(")[0].strip()
            if name in KERNELS:
                rows.append((int(rec["Start_Timestamp"]), name, int(rec["End_Timestamp"]) - int(rec["Start_Timestamp"])))
    rows.sort()
    assert len(rows) == repeats * len(TRACE_GROUPS), len(rows)
    head, tail = rows[:3 * repeats], rows[3 * repeats:]
    parts = [head[g * repeats:(g + 1) * repeats] for g in range(3)]
    parts += [[r for r in tail if r[1] == KERNELS[1]], [r for r in tail if r[1] == KERNELS[0]]]
    for (group, kernel), part in zip(TRACE_GROUPS, parts):
        assert len(part) == repeats and all(name == kernel for _, name, _ in part), group
        ds = [d / 1e3 for _, _, d in part]
        print(json.dumps({"what": "kernel", "name": group, "kernel": kernel, "calls": repeats, "kernel_us": statistics.median(ds),
                          "min_us": min(ds), "max_us": max(ds), "label": label}), flush=True)


def experiment(label):
    from egg_fluid_simulation_amd import SimulationHandler
    for speed in (540.0, 2160.0):
        h = SimulationHandler()
        h.set_solver_order("relaxed")
        i = h.add(300.0, 300.0)
        h.set_colliders([("wall", 240.0, 0.0, 240.0, 600.0)])
        h.set_collider_motion([(speed, 0.0)])
        rows = []
        for step in range(91):
            if step == 30:
                h.set_collider_motion([])
            white, yolk = h.pieces([i])[0]
            tight_w, tight_y = h.pieces([i], 1.25)[0]
            wall_x = h.get_colliders()[0][1]
            rows.append({"step": step, "wall_x": wall_x, "white": tuple(white), "yolk": tuple(yolk), "white_reach_1.25": tuple(tight_w),
                         "yolk_reach_1.25": tuple(tight_y), "whole": h.is_whole(i)})
            assert h.update(1 / 60, 1 / 60, 2, 3) == 1
        for row in rows:
            print(json.dumps(dict(row, what="experiment", wall_speed=speed, label=label)), flush=True)
        h.close()


def smallest_reach(x, y, r):
    """the smallest reach under which the atom is one piece: the largest edge of the minimum spanning tree of d / (ra + rb)"""
    n = x.size
    d = np.sqrt((x[:, None] - x[None, :]) ** 2 + (y[:, None] - y[None, :]) ** 2) / (r[:, None] + r[None, :])
    inside = np.zeros(n, dtype=bool)
    inside[0] = True
    best = d[0].copy()
    worst = 0.0
    for _ in range(n - 1):
        best[inside] = np.inf
        k = int(np.argmin(best))
        worst = max(worst, float(best[k]))
        inside[k] = True
        best = np.minimum(best, d[k])
    return worst


def reach_table(label):
    """one default egg, update(1/60, 1/60, 2, 3) per step, on the CPU models of both orders"""
    import pieces_model as pm
    from relaxed_model import RelaxedModel, rm
    for order in ("exact", "relaxed"):
        m = RelaxedModel(relaxed=order == "relaxed")
        m.add(300.0, 300.0)
        for step in range(121):
            if step in (0, 1, 5, 30, 60, 120):
                row = {"what": "reach", "order": order, "step": step, "label": label}
                for w, name in ((0, "white"), (1, "yolk")):
                    x, y, r = (np.asarray(m.field(w, off), dtype=np.float64) for off in (rm.X, rm.Y, rm.RADIUS))
                    need = smallest_reach(x, y, r)
                    above = pm.record_of(x, y, pm.labels_of(x, y, r, need * (1 + 1e-9)))[1]
                    below = pm.record_of(x, y, pm.labels_of(x, y, r, need * (1 - 1e-9)))[1]
                    row[name] = {"n": int(x.size), "smallest_reach": need, "pieces_just_above": above, "pieces_just_below": below}
                print(json.dumps(row), flush=True)
            if step < 120:
                m.update(1 / 60, 1 / 60, 2, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="calls")
    ap.add_argument("--scenes", default="config3,separate16k")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise, a.repeats, a.label)
        return
    what = a.what.split(",")
    if "reach" in what:
        reach_table(a.label)
        what.remove("reach")
    if not what:
        return
    import torch
    torch.cuda.init()  # (before libeggsim.so: see tests/conftest.py)
    if "calls" in what:
        for scene in a.scenes.split(","):
            calls(scene, a.repeats, a.label)
    if "big" in what:
        big(a.repeats, a.label)
    if "sweeps" in what:
        sweeps(a.label)
    if "cap" in what:
        for scene in a.scenes.split(","):
            cap(scene, a.repeats, a.label)
    if "trace" in what:
        trace(a.repeats)
    if "experiment" in what:
        experiment(a.label)


if __name__ == "__main__":
    main()
