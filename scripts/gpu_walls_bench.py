"""Relaxed order with wall colliders (EGG_COLLIDER_WALL, DESIGN.md section 2.7 "Walls"): ms per step, wall-clock time and
HIP-event kernel time (EGG_OPT_TIMING), after a warm-up, over a steady window.  One JSON line per mode; measured the way
scripts/gpu_surfaces_bench.py measures.

    python scripts/gpu_walls_bench.py [--steps 200] [--warmup 30] [--modes segment,wall,wall_friction] [--package-root DIR] [--label TEXT]

The scene is config 3 (4,096 batches, 4 per site: bench.py's) under gravity (one uniform field, mode (b) of
profiles/r13_forces.md) over a floor 10 px below the centres of the lowest row of batches, so that row lies on it from the
first step on.  The floor is one thin collider from 1,000 px left of the grid to 1,000 px right of it.
modes: segment = the floor as a segment, a list without walls (the collider instantiation of the gather kernel, as
before walls existed); wall = the floor as a wall (the wall instantiation, default surfaces); wall_friction = the same
with friction 0.5; segment_friction = the segment with friction 0.5 (the surface instantiation).
--package-root imports the package from another checkout (a build of an earlier commit: the segment modes only), so that
two builds can be compared in one session, alternating.  Run one mode per process for a figure that is to be relied on.
Relaxed numbers are NOT the project's headline: that is bench.py, exact order."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import grid_positions  # noqa: E402

MODES = {"segment": ("segment", None), "wall": ("wall", None), "wall_friction": ("wall", [0.5]), "segment_friction": ("segment", [0.5])}


def run(mode, steps, warmup):
    from egg_fluid_simulation_amd import WHITE, YOLK, SimulationHandler, _ffi
    h = SimulationHandler()
    h.set_solver_order("relaxed")
    xs, ys, _ = grid_positions(4096, overlap=4)
    kind, surfaces = MODES[mode]
    floor = float(max(ys)) + 10.0
    h.set_colliders([(kind, float(min(xs)) - 1000.0, floor, float(max(xs)) + 1000.0, floor)])
    h.set_forces([("uniform", 0.0, 980.0)])
    if surfaces is not None:
        h.set_collider_surfaces(surfaces)
    h.add_many(xs, ys, 50, 15)
    for _ in range(warmup):
        h.step(1 / 60, 2, 3)
    h.set_option(_ffi.OPT_TIMING, 1)
    h.synchronize()
    s0 = h.stats()
    t0 = time.perf_counter()
    kernel_ms = 0.0
    for _ in range(steps):
        h.step(1 / 60, 2, 3)
        kernel_ms += h.stats()["last_step_kernel_ms"]  # the slower of the two types' streams
    h.synchronize()
    dt = time.perf_counter() - t0
    s1 = h.stats()
    n_w, n_y = h.get_n_particles()
    out = {"name": "config3_floor", "mode": mode, "particles": n_w + n_y, "warmup": warmup, "steps": steps,
           "ms_per_step": 1e3 * dt / steps, "kernel_ms_per_step": kernel_ms / steps,
           "kernel_ms_white": s1["kernel_ms_sum"][WHITE] / max(1, s1["timed_steps"]),
           "kernel_ms_yolk": s1["kernel_ms_sum"][YOLK] / max(1, s1["timed_steps"]),
           "pair_solves_per_step": (s1["pair_solves"] - s0["pair_solves"]) / steps,
           "hits_per_step": sum(h.collider_hits()) / (warmup + steps),
           "grips_per_step": sum(h.collider_grips()) / (warmup + steps),
           "launches_per_step": (s1["kernel_launches"] - s0["kernel_launches"]) / steps}
    h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--modes", default="segment,wall,wall_friction")
    ap.add_argument("--package-root", default=None)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if a.package_root:
        sys.path.insert(0, os.path.abspath(a.package_root))
    for mode in a.modes.split(","):
        print(json.dumps(dict(run(mode, a.steps, a.warmup), label=a.label)), flush=True)


if __name__ == "__main__":
    main()
