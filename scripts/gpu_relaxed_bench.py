"""Exact vs relaxed solver order (EGG_OPT_SOLVER_ORDER) on the scenes of bench.py: ms per step,
wall time and HIP-event kernel time, after a warm-up, over a steady window.  One JSON line per (scene, order).

    python scripts/gpu_relaxed_bench.py [--steps 200] [--warmup 30] [--scenes config3,b16k,b64k] [--orders exact,relaxed]

Relaxed numbers are NOT the project's headline: that is bench.py, exact order."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import grid_positions  # noqa: E402

SCENES = {"config3": (4096, 4), "b16k": (16384, 1), "b64k": (65536, 1)}


def run(n_batches, overlap, order, steps, warmup):
    from egg_fluid_simulation_amd import WHITE, YOLK, SimulationHandler, _ffi
    h = SimulationHandler()
    h.set_solver_order(order)
    xs, ys, _ = grid_positions(n_batches, overlap=overlap)
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
    out = {"scene": "%d batches, %d per site" % (n_batches, overlap), "order": order, "particles": n_w + n_y,
           "warmup": warmup, "steps": steps, "ms_per_step": 1e3 * dt / steps, "steps_per_sec": steps / dt,
           "kernel_ms_per_step": kernel_ms / steps,
           "kernel_ms_white": s1["kernel_ms_sum"][WHITE] / max(1, s1["timed_steps"]),
           "kernel_ms_yolk": s1["kernel_ms_sum"][YOLK] / max(1, s1["timed_steps"]),
           "pair_solves_per_step": (s1["pair_solves"] - s0["pair_solves"]) / steps,
           "max_pass_pairs_white": s1["max_pass_visits"][WHITE],
           "relaxed_steps": s1["relaxed_steps"] - s0["relaxed_steps"]}
    h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--scenes", default="config3,b16k,b64k")
    ap.add_argument("--orders", default="exact,relaxed")
    a = ap.parse_args()
    for scene in a.scenes.split(","):
        nb, ov = SCENES[scene]
        for order in a.orders.split(","):
            print(json.dumps(dict(run(nb, ov, order, a.steps, a.warmup), name=scene)), flush=True)


if __name__ == "__main__":
    main()
