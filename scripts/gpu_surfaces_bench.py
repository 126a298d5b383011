"""Relaxed order with collider surfaces (egg_set_collider_surfaces, DESIGN.md section 2.7 "Collider surfaces"): ms per step,
wall time and HIP-event kernel time (EGG_OPT_TIMING), after a warm-up, over a steady window.  One JSON line per mode;
measured the way scripts/gpu_forces_bench.py measures.

    python scripts/gpu_surfaces_bench.py [--steps 200] [--warmup 30] [--modes off,on] [--package-root DIR] [--label TEXT]

The scene is config 3 (4,096 batches, 4 per site: bench.py's) under gravity (one uniform field, mode (b) of
profiles/r13_forces.md) over a floor: a half-plane 10 px below the centres of the lowest row of batches, so that row lies
on it from the first step on.
modes: off = the floor without surfaces (the collider instantiation of the gather kernel); on = the floor with
friction 0.5 (the surface instantiation); velocity = the floor with a surface velocity and no friction (must equal off:
the same kernels are launched).
--package-root imports the package from another checkout (a build of an earlier commit: mode off only), so that two
builds can be compared in one session, alternating.  Run one mode per process for a figure that is to be relied on.
Relaxed numbers are NOT the project's headline: that is bench.py, exact order."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import grid_positions  # noqa: E402

SURFACES = {"off": None, "on": [0.5], "velocity": [(0.0, 100.0, 0.0)]}


def run(mode, steps, warmup):
    from egg_fluid_simulation_amd import WHITE, YOLK, SimulationHandler, _ffi
    h = SimulationHandler()
    h.set_solver_order("relaxed")
    xs, ys, _ = grid_positions(4096, overlap=4)
    h.set_colliders([("half_plane", 0.0, -1.0, -(float(max(ys)) + 10.0))])
    h.set_forces([("uniform", 0.0, 980.0)])
    if SURFACES[mode] is not None:
        h.set_collider_surfaces(SURFACES[mode])
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
           "grips_per_step": sum(h.collider_grips()) / (warmup + steps) if hasattr(h, "collider_grips") else 0,
           "launches_per_step": (s1["kernel_launches"] - s0["kernel_launches"]) / steps}
    h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--modes", default="off,on")
    ap.add_argument("--package-root", default=None)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if a.package_root:
        sys.path.insert(0, os.path.abspath(a.package_root))
    for mode in a.modes.split(","):
        print(json.dumps(dict(run(mode, a.steps, a.warmup), label=a.label)), flush=True)


if __name__ == "__main__":
    main()
