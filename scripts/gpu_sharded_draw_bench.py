"""draw() of a ShardedSimulationHandler (DESIGN.md section 2.6 "Several processes") beside the single handle's draw() on
the same scene, on ONE GPU, in one run: (a) one SimulationHandler, (b) 2 and 4 sharded ranks over gloo.  Per leg: the
median wall time of a draw() (image copied to the host included, as both forms do) after a warm-up draw; for (b) also
the draw_counters() per draw of the render rank and the bytes the wire model predicts (56 B per particle that is not on
the render rank + 8 B per message).

    python scripts/gpu_sharded_draw_bench.py [--scenes config2,config3] [--legs one,shard2,shard4] [--draws 7]
                                             [--leg-timeout 240]

Every leg is a fresh child process per rank, each under its own `timeout`; the first failing child ends the run.  Ranks
on one card over gloo measure what the PROTOCOL costs (the pack, one message per rank and type through host memory, the
staging copy, the placement) -- not xGMI: nothing here runs on two physical GPUs."""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import grid_positions  # noqa: E402
from scripts.gpu_group_relaxed_bench import cuts_for  # noqa: E402


def scene(name):
    if name == "config2":    # BASELINE config 2: 256 separate batches
        xs, ys, _ = grid_positions(256)
    elif name == "config3":  # BASELINE config 3: 4096 batches, four per site
        xs, ys, _ = grid_positions(4096, overlap=4)
    else:
        raise SystemExit("unknown scene %r" % name)
    return np.asarray(xs, np.float64), np.asarray(ys, np.float64)


def child(a):
    import torch  # noqa: F401  (before libeggsim.so: see tests/conftest.py)
    from egg_fluid_simulation_amd import SimulationHandler
    xs, ys = scene(a.scene)
    origin = (float(xs.min()) - 120.0, float(ys.min()) - 120.0)
    side = int(min(max(xs.max() - xs.min(), ys.max() - ys.min()) + 240.0, 2800.0))
    out = dict(scene=a.scene, leg=a.leg, rank=a.rank, batches=len(xs), draws=a.draws, screen=side)
    dist = None
    if a.leg == "one":
        sim = SimulationHandler()
        sim.set_solver_order("relaxed")  # (the scene only has to be stepped; no hand-overs while it is set up)
        sim.add_many(xs, ys, 50, 15)
        local = sim
    else:
        import torch.distributed as dist
        from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler, SlabLayout
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(a.port), RANK=str(a.rank), WORLD_SIZE=str(a.world))
        dist.init_process_group("gloo", rank=a.rank, world_size=a.world)
        cuts = cuts_for(xs, a.world)
        cuts[0], cuts[-1] = float(xs.min()) - 1e6, float(xs.max()) + 1e6
        sim = ShardedSimulationHandler(SlabLayout(cuts), a.rank, dist, lambda: SimulationHandler(device=0), device="cpu")
        sim.set_solver_order("relaxed")
        for x, y in zip(xs, ys):
            sim.add(float(x), float(y), 50, 15)
        local = sim.local
    try:
        for _ in range(2):
            sim.step(1 / 60, 2, 3)
        sim.draw((side, side), origin, interpolation_alpha=0.5)  # warm-up: texture, canvases, buffers
        local.synchronize()
        c0 = sim.draw_counters() if dist else None
        times = []
        for _ in range(a.draws):
            if dist:
                dist.barrier()
            t0 = time.perf_counter()
            sim.draw((side, side), origin, interpolation_alpha=0.5)
            times.append(1e3 * (time.perf_counter() - t0))
        total = sum(sim.get_n_particles())
        out.update(ms_per_draw_median=statistics.median(times), ms_per_draw_min=min(times), ms_per_draw_max=max(times), particles=total)
        if dist:
            c1, mine = sim.draw_counters(), sum(local.get_n_particles())
            out.update(messages_per_draw=(c1["messages"] - c0["messages"]) / a.draws, bytes_per_draw=(c1["bytes"] - c0["bytes"]) / a.draws,
                       host_ms_per_draw=1e3 * (c1["host_seconds"] - c0["host_seconds"]) / a.draws, particles_local=mine)
            if a.rank == 0:
                out["model_bytes_per_draw"] = 56 * (total - mine) + 8 * 2 * (a.world - 1)
        print(json.dumps(out), flush=True)
    finally:
        if dist:
            dist.destroy_process_group()


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def run_leg(a, name, leg):
    world = int(leg[5:]) if leg.startswith("shard") else 1
    port = free_port()
    procs = []
    for r in range(world):
        cmd = ["timeout", "-k", "10", str(a.leg_timeout), sys.executable, os.path.abspath(__file__), "--child", "--scene", name,
               "--leg", leg, "--rank", str(r), "--world", str(world), "--port", str(port), "--draws", str(a.draws)]
        procs.append(subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True))
    rows = []
    for p in procs:
        stdout, _ = p.communicate()
        if p.returncode != 0:
            for q in procs:
                q.wait()
            raise SystemExit("leg %s of %s: a child ended with status %s; nothing more is started" % (leg, name, p.returncode))
        rows += [json.loads(line) for line in stdout.splitlines() if line.startswith("{")]
    root = [r for r in rows if r["rank"] == 0][0]
    return dict(root, ranks=world, ms_per_draw_slowest_rank=max(r["ms_per_draw_median"] for r in rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="config2,config3")
    ap.add_argument("--legs", default="one,shard2,shard4")
    ap.add_argument("--draws", type=int, default=7)
    ap.add_argument("--leg-timeout", type=int, default=240)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--scene")
    ap.add_argument("--leg")
    ap.add_argument("--rank", type=int, default=0)
    ap.add_argument("--world", type=int, default=1)
    ap.add_argument("--port", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return child(a)
    for name in a.scenes.split(","):
        for leg in a.legs.split(","):
            print(json.dumps(run_leg(a, name, leg)), flush=True)


if __name__ == "__main__":
    main()
