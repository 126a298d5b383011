"""Relaxed order on config 3 of bench.py with cohesion off and on (EGG_OPT_COHESION, DESIGN.md section 2.7 "Cohesion"): ms
per step, wall time and HIP-event kernel time, after a warm-up, over a steady window, and the cohesion pairs per step.  One
JSON line per mode; measured the way scripts/gpu_relaxed_bench.py measures.

    python scripts/gpu_cohesion_bench.py [--steps 200] [--warmup 30] [--modes off,default,white3] [--package-root DIR]

modes: off = EGG_OPT_COHESION 0; default = effective with the default configs (white's band is empty: only yolk coheres);
white3 = effective with white cohesion_interaction_distance_factor 3.  --package-root imports the package from another
checkout (a build of an earlier commit: mode off only), so that two builds can be compared in one session, alternating.
Relaxed numbers are NOT the project's headline: that is bench.py, exact order."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import grid_positions  # noqa: E402


def run(mode, steps, warmup):
    from egg_fluid_simulation_amd import WHITE, YOLK, SimulationHandler, _ffi
    h = SimulationHandler()
    h.set_solver_order("relaxed")
    if mode == "white3":
        h.set_white_config({"cohesion_interaction_distance_factor": 3})
    if mode != "off":
        h.set_cohesion("effective")
    xs, ys, _ = grid_positions(4096, overlap=4)
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
    out = {"name": "config3", "mode": mode, "particles": n_w + n_y, "warmup": warmup, "steps": steps,
           "ms_per_step": 1e3 * dt / steps, "kernel_ms_per_step": kernel_ms / steps,
           "kernel_ms_white": s1["kernel_ms_sum"][WHITE] / max(1, s1["timed_steps"]),
           "kernel_ms_yolk": s1["kernel_ms_sum"][YOLK] / max(1, s1["timed_steps"]),
           "pair_solves_per_step": (s1["pair_solves"] - s0["pair_solves"]) / steps,
           "cohesion_solves_per_step": (s1.get("cohesion_solves", 0) - s0.get("cohesion_solves", 0)) / steps,
           "launches_per_step": (s1["kernel_launches"] - s0["kernel_launches"]) / steps}
    h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--modes", default="off,default,white3")
    ap.add_argument("--package-root", default=None)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if a.package_root:
        sys.path.insert(0, os.path.abspath(a.package_root))
    for mode in a.modes.split(","):
        print(json.dumps(dict(run(mode, a.steps, a.warmup), label=a.label)), flush=True)


if __name__ == "__main__":
    main()
