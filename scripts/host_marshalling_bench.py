"""The host-side marshalling helpers a frame reaches between steps -- _c_probes, _c_impulses (and through it _c_sensors),
_c_field_spec and _c_measure_spec -- timed on the CPU: no device, no library.  One JSON line per measurement.

    python scripts/host_marshalling_bench.py [--repeat 7] [--number 2000] [--tree DIR]
    python scripts/host_marshalling_bench.py --against PARENT_DIR [--rounds 3] [--repeat 7] [--number 2000]

Each helper converts a list of 1 record and a list of 16 (the two specs: one call, with and without a region); a
measurement is the time of one call in microseconds, `timeit` over `number` calls, `repeat` times: the median, the lowest
and the highest.  --tree times the package of another checkout of this repository.  --against alternates runs of PARENT_DIR
and of this tree, `rounds` each in processes of their own, and prints per helper this tree's median of medians beside the
span of the parent's repeats and whether it lies above it."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import timeit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def subjects():
    from egg_fluid_simulation_amd import SimulationHandler as H
    probe = [("point", 100.0, 200.0, 50.0, "white"), ("ray", 0.0, 0.0, 300.0, 400.0, 2.0)]
    regions = [("disc", 100.0, 200.0, 50.0), ("box", 100.0, 200.0, 30.0, 40.0, 0.5, "yolk"), ("capsule", 0.0, 0.0, 10.0, 10.0, 5.0),
               {"kind": "half_plane", "nx": 0.0, "ny": 1.0, "off": 3.0}]
    impulse = [("kick", regions[0], 1.0, 2.0), ("blast", regions[1], 100.0, 200.0, 90.0, {"linear": True}), ("swirl", regions[2], 0.0, 0.0, 1.5),
               ("brake", regions[3], 0.0, 0.0, 1.0, {"id": 7})]
    out = {}
    for n in (1, 16):
        out["_c_probes/%d" % n] = lambda v=[probe[k % 2] for k in range(n)]: H._c_probes(v)
        out["_c_sensors/%d" % n] = lambda v=[regions[k % 4] for k in range(n)]: H._c_sensors(v)
        out["_c_impulses/%d" % n] = lambda v=[impulse[k % 4] for k in range(n)]: H._c_impulses(v)
    out["_c_field_spec"] = lambda: H._c_field_spec((0.0, 0.0), 6.25, (48, 32), "both", "auto")
    out["_c_measure_spec"] = lambda: H._c_measure_spec(None, "both")
    out["_c_measure_spec/region"] = lambda: H._c_measure_spec(regions[1], "white")
    return out


def measure(repeat, number):
    rows = []
    for name, fn in subjects().items():
        fn()
        us = [1e6 * t / number for t in timeit.repeat(fn, number=number, repeat=repeat)]
        rows.append({"helper": name, "median_us": statistics.median(us), "min_us": min(us), "max_us": max(us), "repeat": repeat, "number": number})
    return rows


def run_tree(tree, repeat, number):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", tree, "--repeat", str(repeat), "--number", str(number)],
                         check=True, capture_output=True, text=True).stdout
    return [json.loads(line) for line in out.splitlines() if line.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--number", type=int, default=2000)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--against")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.against is None:
        sys.path.insert(0, os.path.abspath(a.tree))
        for row in measure(a.repeat, a.number):
            print(json.dumps(row))
        return
    runs = {"parent": [], "this": []}
    for _ in range(a.rounds):
        runs["parent"].append(run_tree(a.against, a.repeat, a.number))
        runs["this"].append(run_tree(ROOT, a.repeat, a.number))
    for k, first in enumerate(runs["this"][0]):
        parent, this = ([r[k] for r in runs[which]] for which in ("parent", "this"))
        lo, hi = min(r["min_us"] for r in parent), max(r["max_us"] for r in parent)
        mine = statistics.median(r["median_us"] for r in this)
        print(json.dumps({"helper": first["helper"], "parent_median_us": statistics.median(r["median_us"] for r in parent), "parent_min_us": lo,
                          "parent_max_us": hi, "this_median_us": mine, "this_min_us": min(r["min_us"] for r in this),
                          "this_max_us": max(r["max_us"] for r in this), "above_parent_spread": mine > hi, "rounds": a.rounds,
                          "repeat": a.repeat, "number": a.number}))


if __name__ == "__main__":
    main()
