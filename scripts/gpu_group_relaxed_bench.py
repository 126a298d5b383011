"""Relaxed order on a device group (egg_group_set_solver_order, DESIGN.md section 2.7 "Several devices") against one
relaxed handle, on one GPU: ms per step and steps/s of each scene as ONE handle and as groups of 2 and 4 handles on
the same device, the legs alternating inside every repeat; the halo records and bytes per pass and the ghost fraction
(ghost entries per pass / particles).  One JSON line per (scene, leg, repeat), then one summary line per (scene, leg)
with the median and the spread over the repeats.

    python scripts/gpu_group_relaxed_bench.py [--scenes config3,b16k,pile] [--legs 1,2,4] [--steps 60] [--warmup 10]
                                              [--repeats 3]

Several handles on ONE device measure the protocol's cost (more launches, the ghost passes, the events), not any
scaling: a multi-GPU node is needed for that.  `--legs 1` alone, run with EGGSIM_LIB pointing at another build, gives
the single-handle number of that build for a before / after comparison."""
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


def scene(name):
    if name == "config3":
        xs, ys, _ = grid_positions(4096, overlap=4)
    elif name == "b16k":
        xs, ys, _ = grid_positions(16384, overlap=1)
    elif name == "pile":  # 64 batches 8 x 8 at 20 px (an egg is 100 px across), centred on x = 0
        g = (np.arange(8) - 3.5) * 20.0
        xs, ys = np.repeat(g, 8), np.tile(g, 8)
    else:
        raise SystemExit("unknown scene %r" % name)
    return np.asarray(xs, np.float64), np.asarray(ys, np.float64)


def cuts_for(xs, n):
    """n slabs with equal batch counts (cuts at x quantiles: through the middle of the pile)"""
    if n == 1:
        return None
    inner = [float(np.quantile(xs, k / n)) for k in range(1, n)]
    if len(set(inner)) < len(inner) or inner[0] <= xs.min():
        lo, hi = float(xs.min()), float(xs.max())
        inner = [lo + (hi - lo) * k / n for k in range(1, n)]
    return [-np.inf] + inner + [np.inf]


def run(name, n, steps, warmup):
    from egg_fluid_simulation_amd import SimulationGroup, SimulationHandler
    xs, ys = scene(name)
    if n == 1:
        sim = SimulationHandler()
        sim.set_solver_order("relaxed")
        sim.add_many(xs, ys, 50, 15)
        handles = [sim]
        sync = sim.synchronize
    else:
        sim = SimulationGroup([0] * n, cuts=cuts_for(xs, n))
        sim.set_solver_order("relaxed")
        for x, y in zip(xs, ys):
            sim.add(x, y, 50, 15)
        handles = sim.handles

        def sync():
            for h in handles:
                h.synchronize()
    for _ in range(warmup):
        sim.step(1 / 60, 2, 3)
    sync()
    c0 = sim.halo_counters() if n > 1 else dict(passes=0, records=0, bytes=0)
    t0 = time.perf_counter()
    for _ in range(steps):
        sim.step(1 / 60, 2, 3)
    sync()
    dt = time.perf_counter() - t0
    c1 = sim.halo_counters() if n > 1 else c0
    particles = sum(sum(h.get_n_particles()) for h in handles)
    passes = max(1, c1["passes"] - c0["passes"])
    records = (c1["records"] - c0["records"]) / passes
    out = dict(scene=name, handles=n, batches=len(xs), particles=particles, steps=steps, warmup=warmup,
               ms_per_step=1e3 * dt / steps, steps_per_sec=steps / dt,
               halo_records_per_pass=records, halo_bytes_per_pass=(c1["bytes"] - c0["bytes"]) / passes,
               ghost_fraction=records / particles,
               migrations=sim.counters()["migrations"] if n > 1 else 0,
               pair_solves=sum(h.stats()["pair_solves"] for h in handles),
               lib=os.environ.get("EGGSIM_LIB", "default"))
    sim.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="config3,b16k,pile")
    ap.add_argument("--legs", default="1,2,4")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    legs = [int(v) for v in a.legs.split(",")]
    for name in a.scenes.split(","):
        res = {n: [] for n in legs}
        for rep in range(a.repeats):
            for n in legs:  # alternating: drift of the machine lands on every leg alike
                r = run(name, n, a.steps, a.warmup)
                r["repeat"] = rep
                res[n].append(r)
                print(json.dumps(r), flush=True)
        for n in legs:
            ms = [r["ms_per_step"] for r in res[n]]
            last = res[n][-1]
            print(json.dumps(dict(summary=True, scene=name, handles=n, repeats=a.repeats,
                                  ms_per_step_median=statistics.median(ms), ms_per_step_min=min(ms),
                                  ms_per_step_max=max(ms), steps_per_sec_median=1e3 / statistics.median(ms),
                                  halo_records_per_pass=last["halo_records_per_pass"],
                                  halo_bytes_per_pass=last["halo_bytes_per_pass"],
                                  ghost_fraction=last["ghost_fraction"], lib=last["lib"])), flush=True)


if __name__ == "__main__":
    main()
