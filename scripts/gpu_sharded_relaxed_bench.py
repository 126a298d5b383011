"""Relaxed order on a ShardedSimulationHandler (DESIGN.md section 2.7 "Several processes") against the existing forms,
on ONE GPU, in one run: (a) one relaxed handle, (b) a 2-handle SimulationGroup, (c) 2 and 4 sharded ranks over gloo.
Per leg: ms per step; for (c) also the host microseconds per pass spent in the halo exchange, the host
synchronisations per pass, and the ghost records and bytes per pass (per rank, the slowest rank's time).

    python scripts/gpu_sharded_relaxed_bench.py [--scenes config3,b16k] [--legs one,group2,shard2,shard4] [--steps 40]
                                                [--warmup 10] [--repeats 2] [--leg-timeout 240]

Every leg is a fresh child process per rank, each under its own `timeout`; the legs alternate inside every repeat, and
the first failing child ends the run.  Ranks on one card over gloo measure what the PROTOCOL costs (per-pass
collectives and messages through host memory, the host synchronisations, every rank's cell table sized for all
particles) -- not xGMI and not scaling: nothing here runs on two physical GPUs."""
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

from scripts.gpu_group_relaxed_bench import cuts_for, scene  # noqa: E402


def child(a):
    import torch  # noqa: F401  (before libeggsim.so: see tests/conftest.py)
    from egg_fluid_simulation_amd import SimulationGroup, SimulationHandler
    xs, ys = scene(a.scene)
    out = dict(scene=a.scene, leg=a.leg, rank=a.rank, batches=len(xs), steps=a.steps, warmup=a.warmup)
    if a.leg in ("one", "group2"):
        if a.leg == "one":
            sim = SimulationHandler()
            sim.set_solver_order("relaxed")
            sim.add_many(xs, ys, 50, 15)
            handles = [sim]
        else:
            sim = SimulationGroup([0, 0], cuts=cuts_for(xs, 2))
            sim.set_solver_order("relaxed")
            for x, y in zip(xs, ys):
                sim.add(x, y, 50, 15)
            handles = sim.handles

        def sync():
            for h in handles:
                h.synchronize()

        for _ in range(a.warmup):
            sim.step(1 / 60, 2, 3)
        sync()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            sim.step(1 / 60, 2, 3)
        sync()
        dt = time.perf_counter() - t0
        out.update(ms_per_step=1e3 * dt / a.steps, particles=sum(sum(h.get_n_particles()) for h in handles))
        print(json.dumps(out), flush=True)
        return
    import torch.distributed as dist
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler, SlabLayout
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(a.port), RANK=str(a.rank), WORLD_SIZE=str(a.world))
    dist.init_process_group("gloo", rank=a.rank, world_size=a.world)
    try:
        cuts = cuts_for(xs, a.world)
        cuts[0], cuts[-1] = float(xs.min()) - 1e6, float(xs.max()) + 1e6
        sh = ShardedSimulationHandler(SlabLayout(cuts), a.rank, dist, lambda: SimulationHandler(device=0), device="cpu")
        sh.set_solver_order("relaxed")
        for x, y in zip(xs, ys):
            sh.add(float(x), float(y), 50, 15)
        for _ in range(a.warmup):
            sh.step(1 / 60, 2, 3)
        sh.local.synchronize()
        dist.barrier()
        h = sh.halo
        p0, r0, s0, y0, m0, c0 = h.passes, h.records, h.host_seconds, h.host_syncs, h.messages, h.collectives
        t0 = time.perf_counter()
        for _ in range(a.steps):
            sh.step(1 / 60, 2, 3)
        sh.local.synchronize()
        dt = time.perf_counter() - t0
        passes = h.passes - p0
        out.update(ms_per_step=1e3 * dt / a.steps, particles=sum(sh.local.get_n_particles()),
                   exchange_us_per_pass=1e6 * (h.host_seconds - s0) / passes, host_syncs_per_pass=(h.host_syncs - y0) / passes,
                   records_per_pass=(h.records - r0) / passes, bytes_per_pass=40 * (h.records - r0) / passes,
                   messages_per_pass=(h.messages - m0) / passes, collectives_per_pass=(h.collectives - c0) / passes,
                   migrations=sh.migrations)
        print(json.dumps(out), flush=True)
    finally:
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
               "--leg", leg, "--rank", str(r), "--world", str(world), "--port", str(port), "--steps", str(a.steps),
               "--warmup", str(a.warmup)]
        procs.append(subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True))
    rows = []
    for p in procs:
        stdout, _ = p.communicate()
        if p.returncode != 0:
            for q in procs:
                q.wait()
            raise SystemExit("leg %s of %s: a child ended with status %s; nothing more is started" % (leg, name, p.returncode))
        rows += [json.loads(line) for line in stdout.splitlines() if line.startswith("{")]
    slow = max(rows, key=lambda r: r["ms_per_step"])
    row = dict(slow, particles=sum(r["particles"] for r in rows), ranks=world)
    for k in ("records_per_pass", "bytes_per_pass"):
        if k in slow:
            row[k + "_all_ranks"] = sum(r[k] for r in rows)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="config3,b16k")
    ap.add_argument("--legs", default="one,group2,shard2,shard4")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=2)
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
    legs = a.legs.split(",")
    for name in a.scenes.split(","):
        res = {leg: [] for leg in legs}
        for rep in range(a.repeats):
            for leg in legs:  # alternating: drift of the machine lands on every leg alike
                row = run_leg(a, name, leg)
                row["repeat"] = rep
                res[leg].append(row)
                print(json.dumps(row), flush=True)
        for leg in legs:
            ms = [r["ms_per_step"] for r in res[leg]]
            print(json.dumps(dict(summary=True, scene=name, leg=leg, repeats=a.repeats, ms_per_step_median=statistics.median(ms),
                                  ms_per_step_min=min(ms), ms_per_step_max=max(ms))), flush=True)


if __name__ == "__main__":
    main()
