"""Relaxed order with collider contacts (egg_set_collider_contacts, DESIGN.md section 2.7 "Collider contacts"): ms per step,
wall-clock time and HIP-event kernel time (EGG_OPT_TIMING), after a warm-up, over a steady window.  One JSON line per (scene,
mode); measured the way scripts/gpu_bodies_bench.py measures, on its scenes and its list -- a floor (a wall), a side, a ball
(the disc) and a plate above the grid -- with the ball 1 px under the plate.

    python scripts/gpu_contacts_bench.py [--steps 200] [--warmup 30] [--scenes config3,separate16k] [--modes unset,bodies,contacts]
                                         [--package-root DIR] [--label TEXT]

scenes: config3 = 4,096 batches, 4 per site (bench.py's); separate16k = 16,384 separate batches.  Both under gravity.
modes: unset = neither loads, bodies nor contacts are ever set (the only mode an earlier commit has); off = loads on, the two
bodies and set_collider_contacts with every record off (must launch what bodies launch); bodies = loads on, the plate and
the ball are heavy bodies, the plate starts at PLATE_V towards the ball: they pass through each other; contacts = the same
with the floor, the ball and the plate contact-enabled: the plate reaches the ball inside the warm-up, the one fire (e = 0)
leaves both at the same speed, and from then on every sub-step evaluates the two pairs (floor-ball, ball-plate) and neither fires: what is timed is
the machinery, S more one-wave launches per step and two small copies, not the arithmetic of a fire.
--package-root imports the package from another checkout (a build of an earlier commit: mode unset only), so that two
builds can be compared in one session, alternating.  Run one (scene, mode) per process for a figure that is to be relied on.
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
PLATE_V = (0.0, 2.0)    # px/s, towards the grid; it does not reach it inside the window
PLATE_BODY = (1.0e-6, 0.0, 0.0, 0.0, 0.0, 0.0)
BALL_BODY = (1.0e-6, 1.0e-9, 0.0, 0.0, 0.0, 0.0)
BALL_R = 20.0


def run(scene, mode, steps, warmup):
    from egg_fluid_simulation_amd import WHITE, YOLK, SimulationHandler, _ffi
    h = SimulationHandler()
    h.set_solver_order("relaxed")
    n, overlap = SCENES[scene]
    xs, ys, _ = grid_positions(n, overlap=overlap)
    floor, left, mid = float(max(ys)) + 10.0, float(min(xs)) - 60.0, 0.5 * (float(min(xs)) + float(max(xs)))
    plate = float(min(ys)) - 200.0
    ball_y = plate + BALL_R + 1.0  # 1 px under the plate: the plate is there after 30 steps
    h.set_colliders([("wall", float(min(xs)) - 1000.0, floor, float(max(xs)) + 1000.0, floor), ("half_plane", 1.0, 0.0, left),
                     ("disc", mid, ball_y, BALL_R), ("half_plane", 0.0, 1.0, plate)])
    h.set_collider_surfaces([0.5, None, None, None])
    h.set_forces([("uniform", 0.0, 980.0)])
    if mode != "unset":
        h.set_collider_loads(True)
    if mode != "unset":
        h.set_collider_motion([None, None, None, PLATE_V])
        h.set_collider_spin([None, None, (mid, ball_y, 0.125), None])
        h.set_collider_bodies([None, None, BALL_BODY, PLATE_BODY])
    if mode == "off":
        h.set_collider_contacts([None] * 4)
    if mode == "contacts":
        h.set_collider_contacts([True, None, True, True])
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
    out = {"name": scene, "mode": mode, "particles": n_w + n_y, "warmup": warmup, "steps": steps,
           "ms_per_step": 1e3 * dt / steps, "kernel_ms_per_step": kernel_ms / steps,
           "kernel_ms_white": s1["kernel_ms_sum"][WHITE] / max(1, s1["timed_steps"]),
           "kernel_ms_yolk": s1["kernel_ms_sum"][YOLK] / max(1, s1["timed_steps"]),
           "pair_solves_per_step": (s1["pair_solves"] - s0["pair_solves"]) / steps,
           "hits_per_step": sum(h.collider_hits()) / (warmup + steps),
           "launches_per_step": (s1["kernel_launches"] - s0["kernel_launches"]) / steps,
           "contact_solves_per_step": (h.collider_contact_solves() if hasattr(h, "collider_contact_solves") else 0) / (warmup + steps),
           "ball": list(h.get_colliders()[2]), "ball_motion": list(h.get_collider_motion()[2]),
           "plate": list(h.get_colliders()[3]), "plate_motion": list(h.get_collider_motion()[3])}
    h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--scenes", default="config3,separate16k")
    ap.add_argument("--modes", default="unset,bodies,contacts")
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
