"""draw() of a device group (egg_group_render, DESIGN.md section 2.6 "Several devices") against one handle's draw, on one
GPU: ms per draw() with rgba = NULL (the image stays on the device) of each scene as ONE handle and as groups of 2 and 4
handles on the same device, the legs alternating inside every repeat.  One JSON line per (scene, leg, repeat), then one
summary line per (scene, leg) with the median and the range over the repeats and the ratio group / single.

    python scripts/gpu_group_draw_bench.py [--scenes config2,b16k] [--legs 1,2,4] [--draws 40] [--warmup 5] [--repeats 3]

Several handles on ONE device measure the cost of the gather and its launches, not a transfer between devices: a multi-GPU
node is needed for that (56 B per remote particle cross a link per draw).  `--legs 1` alone, run with EGGSIM_LIB pointing
at another build, gives the single-handle number of that build for a before / after comparison.  For kernel times run
the script under `rocprofv3 --kernel-trace --stats` with `--repeats 1`: the gather is egg_group_gather_kernel."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import grid_positions  # noqa: E402
from scripts.gpu_group_relaxed_bench import cuts_for  # noqa: E402

GATHER_BYTES_PER_PARTICLE = 112  # seven doubles read, seven written


def scene(name):
    if name == "config2":  # BASELINE config 2: 256 batches, 44,032 particles (profiles/r02_render_cfg2.md)
        xs, ys, _ = grid_positions(256)
    elif name == "b16k":
        xs, ys, _ = grid_positions(16384, overlap=1)
    else:
        raise SystemExit("unknown scene %r" % name)
    return np.asarray(xs, np.float64), np.asarray(ys, np.float64)


def run(name, n, draws, warmup):
    from egg_fluid_simulation_amd import SimulationGroup, SimulationHandler, _ffi
    xs, ys = scene(name)
    lo_x, lo_y = float(xs.min()) - 120.0, float(ys.min()) - 120.0
    size = int(min(max(xs.max() - xs.min(), ys.max() - ys.min()) + 240.0, 2800.0))
    if n == 1:
        sim = SimulationHandler()
        sim.add_many(xs, ys, 50, 15)
        render, ptr = sim._lib.egg_render, sim._h
    else:
        sim = SimulationGroup([0] * n, cuts=cuts_for(xs, n))
        for x, y in zip(xs, ys):
            sim.add(x, y, 50, 15)
        render, ptr = sim._lib.egg_group_render, sim._g
    sim.set_solver_order("relaxed")  # (the scene only has to be stepped once; no hand-overs while it is set up)
    for _ in range(2):
        sim.step(1 / 60, 2, 3)
    p = _ffi.EggRenderParams()
    sim._lib.egg_default_render_params(C.byref(p))
    p.screen_w = p.screen_h = size
    p.origin_x, p.origin_y = lo_x, lo_y
    p.interpolation_alpha = 0.5
    for _ in range(warmup):
        assert render(ptr, C.byref(p), None) == 0
    t0 = time.perf_counter()
    for _ in range(draws):
        assert render(ptr, C.byref(p), None) == 0  # (returns after a synchronise of the render stream)
    dt = time.perf_counter() - t0
    particles = sum(sim.get_n_particles())
    out = dict(scene=name, handles=n, batches=len(xs), particles=particles, draws=draws, warmup=warmup, screen=size,
               ms_per_draw=1e3 * dt / draws, gather_bytes_per_draw=GATHER_BYTES_PER_PARTICLE * particles if n > 1 else 0,
               lib=os.environ.get("EGGSIM_LIB", "default"))
    sim.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="config2,b16k")
    ap.add_argument("--legs", default="1,2,4")
    ap.add_argument("--draws", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    legs = [int(v) for v in a.legs.split(",")]
    for name in a.scenes.split(","):
        res = {n: [] for n in legs}
        for rep in range(a.repeats):
            for n in legs:  # alternating: drift of the machine lands on every leg alike
                r = run(name, n, a.draws, a.warmup)
                r["repeat"] = rep
                res[n].append(r)
                print(json.dumps(r), flush=True)
        single = statistics.median(r["ms_per_draw"] for r in res[legs[0]])
        for n in legs:
            ms = [r["ms_per_draw"] for r in res[n]]
            print(json.dumps(dict(summary=True, scene=name, handles=n, repeats=a.repeats, particles=res[n][-1]["particles"],
                                  ms_per_draw_median=statistics.median(ms), ms_per_draw_min=min(ms), ms_per_draw_max=max(ms),
                                  ratio_to_first_leg=statistics.median(ms) / single, lib=res[n][-1]["lib"])), flush=True)


if __name__ == "__main__":
    main()
