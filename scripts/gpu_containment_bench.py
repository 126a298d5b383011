"""Relaxed order with yolk containment (egg_set_containment, DESIGN.md section 2.7 "Containment"): ms per step, wall time
and HIP-event kernel time (EGG_OPT_TIMING), after a warm-up, over a steady window that ends in a synchronise.  One JSON
line per (scene, mode); measured the way scripts/gpu_coupling_bench.py measures.

    python scripts/gpu_containment_bench.py [--steps 200] [--warmup 30] [--scenes config3,separate16k]
                                            [--modes off,on] [--package-root DIR] [--label TEXT]

scenes: config3 = 4,096 batches, 4 per site (bench.py's config 3); separate16k = 16,384 separate batches.
modes: off = containment never set (its surface is not called, so the mode also runs on a build of the parent commit);
on = set_containment(2, 1).  Coupling and adhesion stay off: containment does not need them.
--package-root imports the package from another checkout (a build of an earlier commit: mode off only), so that two
builds can be compared in one session, alternating.  Run one mode per process for a figure that is to be relied on.
The line also carries the bytes the rule needs per step -- per sub-step 2 x 16 B per white particle plus 24 B per atom for
the summary, 20 B read and 16 B written per yolk particle for the projection -- to set against the two kernels' time from a
rocprofv3 --kernel-trace --stats run of their own.
Relaxed numbers are NOT the project's headline: that is bench.py, exact order."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import grid_positions  # noqa: E402

SCENES = {"config3": (4096, 4), "separate16k": (16384, 1)}


CONTAINMENT = {"off": None, "on": (2.0, 1.0)}
S, C = 2, 3


def run(scene, mode, steps, warmup):
    from egg_fluid_simulation_amd import WHITE, YOLK, SimulationHandler, _ffi
    h = SimulationHandler()
    h.set_solver_order("relaxed")
    batches, overlap = SCENES[scene]
    xs, ys, _ = grid_positions(batches, overlap=overlap)
    if CONTAINMENT[mode]:
        h.set_containment(*CONTAINMENT[mode])
    h.add_many(xs, ys, 50, 15)
    for _ in range(warmup):
        h.step(1 / 60, S, C)
    h.set_option(_ffi.OPT_TIMING, 1)
    h.synchronize()
    s0 = h.stats()
    t0 = time.perf_counter()
    kernel_ms = 0.0
    for _ in range(steps):
        h.step(1 / 60, S, C)
        kernel_ms += h.stats()["last_step_kernel_ms"]  # the slower of the two types' streams
    h.synchronize()
    dt = time.perf_counter() - t0
    s1 = h.stats()
    n_w, n_y = h.get_n_particles()
    import egg_fluid_simulation_amd
    out = {"package": os.path.relpath(os.path.dirname(egg_fluid_simulation_amd.__file__), ROOT), "name": scene, "mode": mode, "particles": n_w + n_y, "warmup": warmup, "steps": steps,
           "ms_per_step": 1e3 * dt / steps, "kernel_ms_per_step": kernel_ms / steps,
           "kernel_ms_white": s1["kernel_ms_sum"][WHITE] / max(1, s1["timed_steps"]),
           "kernel_ms_yolk": s1["kernel_ms_sum"][YOLK] / max(1, s1["timed_steps"]),
           "pair_solves_per_step": (s1["pair_solves"] - s0["pair_solves"]) / steps,
           "containment_hits_per_step": h.containment_hits() / (warmup + steps) if CONTAINMENT[mode] else 0,
           "summary_bytes_per_step": S * (32 * n_w + 24 * batches), "projection_bytes_per_step": S * 36 * n_y,
           "launches_per_step": (s1["kernel_launches"] - s0["kernel_launches"]) / steps}
    h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--scenes", default="config3,separate16k")
    ap.add_argument("--modes", default="off,on")
    ap.add_argument("--package-root", default=None)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if a.package_root:
        sys.path.insert(0, os.path.abspath(a.package_root))
    for scene in a.scenes.split(","):
        for mode in a.modes.split(","):
            print(json.dumps(dict(run(scene, mode, a.steps, a.warmup), label=a.label)), flush=True)


if __name__ == "__main__":
    main()
