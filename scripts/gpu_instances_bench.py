"""The instanced-draw record of one frame, both types ("The instanced-draw record"), on one GPU:
host wall time per frame of

    (a) download_instance_data(w)            seven blocking float64 downloads per type, interleaved and narrowed on the host
    (b) instances(w, color=False)            one pack kernel and one 28 B-per-particle copy per type (colour unchanged)
    (c) instances_begin() .. sleep of one step's duration .. instances_end(w): the time spent blocked in the two ends

for a single handle, and (a) against (b) for a device group (--group N handles on this device) and for a sharded scene
(--ranks N processes on this card over gloo: NOT a multi-GPU figure).  The methods alternate inside every repeat.  One
JSON line per (scene, form, method, repeat), then one summary line per (scene, form, method) with mean, standard deviation
and the ratio to (a); the condition of the issue -- (b) no slower than (a) within two standard deviations of (a)'s own
repeats -- is evaluated in the summary line of (b).

    python scripts/gpu_instances_bench.py [--scenes config3,config2] [--frames 200] [--warmup 10] [--repeats 5]
                                          [--group 2] [--ranks 2] [--jsonl PATH]
    python scripts/gpu_instances_bench.py --tree PARENT_CHECKOUT --methods a --group 0 --ranks 0 --jsonl PATH2
    rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d DIR -o run -- \
        python scripts/gpu_instances_bench.py --kernel-run --frames 50
    python scripts/gpu_instances_bench.py --report OUT.md --jsonl PATH [--jsonl2 PATH2] --kernel-trace DIR/run_kernel_trace.csv
                                          [--copy-stats DIR/run_memory_copy_stats.csv] [--trace-out REDUCED.csv]

The first error ends the script with a non-zero status: nothing more is started on the GPU after a leg has failed; a leg
that is not wanted is switched off beforehand (--group 0, --ranks 0, --methods).  --tree imports the package from another
built checkout -- the parent commit's, for a "before" figure of (a) from the parent's own build.  --kernel-run packs
config 3 and config 2 and nothing else: the pack is egg_instances_kernel.  --report needs no GPU: it writes the markdown
table from the rows of earlier runs and the profiler's per-dispatch trace (kernel time per launch size, told apart by the
grid size), with the byte model (84 B per particle through the kernel: seven doubles read, seven floats written; 28 B per
particle to the host) next to what was measured."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import grid_positions  # noqa: E402

KERNEL_BYTES_PER_PARTICLE = 84   # 7 x 8 B read + 28 B written (the colour mesh, when packed, adds 16 B written)
RECORD_BYTES = 28
DOWNLOAD_BYTES_PER_PARTICLE = 56  # what (a) moves over the link


def scene(name):
    if name == "config2":  # BASELINE config 2: 256 batches, 44,032 particles
        xs, ys, _ = grid_positions(256)
    elif name == "config3":  # BASELINE config 3: 4,096 batches, four to a site, 704,512 particles
        xs, ys, _ = grid_positions(4096, overlap=4)
    else:
        raise SystemExit("unknown scene %r" % name)
    return np.asarray(xs, np.float64), np.asarray(ys, np.float64)


def cuts_for(xs, n):
    """x-slabs with about the same number of batches each"""
    q = np.quantile(np.unique(xs), [k / n for k in range(1, n)])
    return [-1e9] + [float(v) + 1.0 for v in q] + [1e9]


def frame_a(sim):
    return [sim.download_instance_data(w) for w in (0, 1)]


def frame_b(sim):
    return [sim.instances(w, color=False) for w in (0, 1)]


def timed(frames, warmup, one):
    for _ in range(warmup):
        one()
    t0 = time.perf_counter()
    for _ in range(frames):
        one()
    return 1e3 * (time.perf_counter() - t0) / frames


def single(name, a, emit):
    from egg_fluid_simulation_amd import SimulationHandler
    xs, ys = scene(name)
    h = SimulationHandler()
    h.add_many(xs, ys, 50, 15)
    for _ in range(2):
        h.step(1 / 60, 2, 3)
    h.synchronize()
    t0 = time.perf_counter()
    h.step(1 / 60, 2, 3)
    h.synchronize()
    step_s = time.perf_counter() - t0
    n = sum(h.get_n_particles())
    form = "single" if not a.tree else "single, the checkout given by --tree"
    if "b" in a.methods:
        want = [d.astype(np.float32) for d in frame_a(h)]
        got = frame_b(h)
        assert all(np.array_equal(g[0].view(np.uint32), w.view(np.uint32)) for g, w in zip(got, want)), "the two paths disagree"

    def blocked():
        h.instances_begin()
        time.sleep(step_s)
        t = time.perf_counter()
        h.instances_end(0)
        h.instances_end(1)
        return time.perf_counter() - t

    for rep in range(a.repeats):
        if "a" in a.methods:
            emit(dict(scene=name, form=form, method="a", repeat=rep, particles=n, ms_per_frame=timed(a.frames, a.warmup, lambda: frame_a(h))))
        if "b" in a.methods:
            emit(dict(scene=name, form=form, method="b", repeat=rep, particles=n, ms_per_frame=timed(a.frames, a.warmup, lambda: frame_b(h))))
        if "c" in a.methods:
            for _ in range(a.warmup):
                blocked()
            emit(dict(scene=name, form=form, method="c", repeat=rep, particles=n, step_ms=1e3 * step_s,
                      ms_per_frame=1e3 * statistics.mean(blocked() for _ in range(a.frames))))
    h.close()


def group(name, a, emit):
    from egg_fluid_simulation_amd import SimulationGroup
    xs, ys = scene(name)
    g = SimulationGroup([0] * a.group, cuts=cuts_for(xs, a.group))
    for x, y in zip(xs, ys):
        g.add(x, y, 50, 15)
    g.set_solver_order("relaxed")  # (the scene only has to be stepped: no hand-overs while it is set up)
    for _ in range(2):
        g.step(1 / 60, 2, 3)
    n = sum(g.get_n_particles())
    form = "group of %d handles on one device" % a.group
    for rep in range(a.repeats):
        emit(dict(scene=name, form=form, method="a", repeat=rep, particles=n, ms_per_frame=timed(a.frames, a.warmup, lambda: frame_a(g))))
        emit(dict(scene=name, form=form, method="b", repeat=rep, particles=n, ms_per_frame=timed(a.frames, a.warmup, lambda: frame_b(g))))
    g.close()


def _rank(rank, world, port, name, frames, warmup, repeats, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from egg_fluid_simulation_amd import SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler, SlabLayout
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        xs, ys = scene(name)
        sh = ShardedSimulationHandler(SlabLayout(cuts_for(xs, world)), rank, dist, lambda: SimulationHandler(device=0), device="cpu")
        sh.set_solver_order("relaxed", 1.8)
        for x, y in zip(xs, ys):
            sh.add(float(x), float(y), 50, 15)
        for _ in range(2):
            sh.step(1 / 60, 2, 3)
        n = sum(sh.get_n_particles())
        rows = []
        for rep in range(repeats):
            for method, one in (("a", lambda: frame_a(sh)), ("b", lambda: frame_b(sh))):
                dist.barrier()
                rows.append(dict(method=method, repeat=rep, particles=n, ms_per_frame=timed(frames, warmup, one)))
        q.put((rank, "ok", rows))
    except Exception:
        import traceback
        q.put((rank, "error: " + traceback.format_exc(), None))
    finally:
        dist.destroy_process_group()


def sharded(name, a, emit):
    import socket

    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(r, a.ranks, port, name, a.frames, a.warmup, a.repeats, q)) for r in range(a.ranks)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in procs:
            rank, outcome, rows = q.get(timeout=300)
            if outcome != "ok":
                raise SystemExit(outcome)
            res[rank] = rows
    finally:
        for p in procs:
            p.join(30)
            if p.is_alive():
                p.kill()  # (a rank that waits for one that failed)
    form = "sharded, %d ranks on one card over gloo" % a.ranks
    for row in res[0]:  # the render rank's clock: it returns when the arrays are there
        emit(dict(scene=name, form=form, **row))


def summarise(rows):
    keys = []
    for r in rows:
        k = (r["scene"], r["form"], r["method"])
        if k not in keys:
            keys.append(k)
    out = []
    for k in keys:
        ms = [r["ms_per_frame"] for r in rows if (r["scene"], r["form"], r["method"]) == k]
        base = [r["ms_per_frame"] for r in rows if (r["scene"], r["form"], r["method"]) == (k[0], k[1], "a")]
        s = dict(summary=True, scene=k[0], form=k[1], method=k[2], repeats=len(ms), particles=[r for r in rows if r["scene"] == k[0]][0]["particles"],
                 ms_mean=statistics.mean(ms), ms_median=statistics.median(ms), ms_sd=statistics.stdev(ms) if len(ms) > 1 else 0.0,
                 ms_min=min(ms), ms_max=max(ms))
        if base:
            s["ratio_to_a"] = s["ms_mean"] / statistics.mean(base)
            if k[2] == "b":
                sd_a = statistics.stdev(base) if len(base) > 1 else 0.0
                s["allowed_ms"] = statistics.mean(base) + 2 * sd_a
                s["not_slower_than_a"] = bool(s["ms_mean"] <= s["allowed_ms"])
        parent = [r["ms_per_frame"] for r in rows if (r["scene"], r["method"]) == (k[0], "a") and "--tree" in r["form"]]
        if parent and k[1] == "single" and k[2] == "b":  # against (a) as the parent commit's own build runs it
            s["parent_a_mean"], s["parent_a_sd"] = statistics.mean(parent), statistics.stdev(parent) if len(parent) > 1 else 0.0
            s["ratio_to_parent_a"] = s["ms_mean"] / s["parent_a_mean"]
            s["not_slower_than_parent_a"] = bool(s["ms_mean"] <= s["parent_a_mean"] + 2 * s["parent_a_sd"])
        steps = [r["step_ms"] for r in rows if (r["scene"], r["form"], r["method"]) == k and "step_ms" in r]
        if steps:
            s["step_ms"] = steps[0]
        out.append(s)
    return out


def kernel_run(frames):
    from egg_fluid_simulation_amd import SimulationHandler
    for name in ("config3", "config2"):
        xs, ys = scene(name)
        h = SimulationHandler()
        h.add_many(xs, ys, 50, 15)
        h.step(1 / 60, 2, 3)
        for _ in range(frames):
            frame_b(h)
        print(json.dumps(dict(kernel_run=True, scene=name, frames=frames, particles=h.get_n_particles())), flush=True)
        h.close()


def _col(row, *names):
    """a column of a profiler CSV whose spelling differs between versions"""
    low = {k.lower(): v for k, v in row.items()}
    for n in names:
        if n.lower() in low:
            return low[n.lower()]
    raise KeyError(names)


def kernel_table(a, meta, out):
    """egg_instances_kernel per launch size from the per-dispatch trace: the grid size tells the four sizes apart"""
    rows = [r for r in csv.DictReader(open(a.kernel_trace)) if _col(r, "Kernel_Name").startswith("egg_instances_kernel")]
    if a.trace_out:  # the reduced trace that is kept with the report
        with open(a.trace_out, "w") as f:
            f.write("Kernel_Name,Grid_Size,Start_Timestamp,End_Timestamp\n")
            for r in rows:
                f.write("%s,%s,%s,%s\n" % (_col(r, "Kernel_Name"), _col(r, "Grid_Size", "Grid_Size_X"), _col(r, "Start_Timestamp"),
                                           _col(r, "End_Timestamp")))
    sizes = {}
    for m in meta:
        for w, n in enumerate(m["particles"]):
            sizes[(n + 255) // 256 * 256] = (m["scene"], ("white", "yolk")[w], n)
    by_grid = {}
    for r in rows:
        by_grid.setdefault(int(_col(r, "Grid_Size", "Grid_Size_X")), []).append(
            (int(_col(r, "End_Timestamp")) - int(_col(r, "Start_Timestamp"))) / 1e3)
    out += ["`rocprofv3 --kernel-trace` over `--kernel-run` (%s), one row per launch size (grid size = particles rounded up to 256)." %
            ", ".join("%s: %d frames" % (m["scene"], m["frames"]) for m in meta),
            "The same source arrays are packed again and again and fit the 256 MiB Infinity Cache: these are CACHE-WARM times,",
            "and the bytes/s are not an HBM figure.  Byte model: %d B per particle (seven doubles read, seven floats written)." % KERNEL_BYTES_PER_PARTICLE, "",
            "| launch | particles | calls | median us | min us | max us | model MB | TB/s at the median |", "|---|---|---|---|---|---|---|---|"]
    for grid in sorted(by_grid, reverse=True):
        us = by_grid[grid]
        scene_, kind, n = sizes.get(grid, ("?", "?", grid))
        mb = n * KERNEL_BYTES_PER_PARTICLE / 1e6
        out.append("| %s %s | %d | %d | %.2f | %.2f | %.2f | %.2f | %.2f |" % (scene_, kind, n, len(us), statistics.median(us), min(us), max(us), mb,
                                                                           mb / statistics.median(us)))


def report(a):
    rows = []
    for path in (a.jsonl, a.jsonl2):
        if path:
            rows += [json.loads(line) for line in open(path) if line.strip().startswith("{")]
    sums = summarise([r for r in rows if "ms_per_frame" in r and not r.get("summary")])
    meta = [r for r in rows if r.get("kernel_run")]
    frames = sorted({r["frames"] for r in rows if "ms_per_frame" in r and "frames" in r})
    out = ["# The instanced-draw record per frame: `download_instance_data` against `instances` (one MI355X)", "",
           "Produced by `scripts/gpu_instances_bench.py` (its docstring has the commands).  Host wall time per frame, both types,",
           "around calls that end in a device synchronise; %s frames per timed window; the methods alternate inside every" % "/".join(str(f) for f in frames),
           "repeat; mean, median and standard deviation over the repeats.  (a) `download_instance_data`, (b) `instances(color=False)`:",
           "the data mesh only, the colour mesh is NOT fetched (a frame without a colour change); (c) time blocked in `instances_end`",
           "after `instances_begin` and a host sleep of one step's duration.  Sharded rows are ranks on ONE card over gloo,",
           "not a multi-GPU figure.  Rows marked --tree ran (a) from the parent commit's own checkout and build, as a process",
           "of its own before the other rows, in the same session on the same card.", "",
           "| scene | form | method | particles | mean ms | median ms | sd | min .. max | ratio to (a) | (b) <= (a) + 2 sd(a) |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for s in sums:
        verdict = "" if "not_slower_than_a" not in s else ("yes" if s["not_slower_than_a"] else "NO") + " (%.3f ms allowed)" % s["allowed_ms"]
        out.append("| %s | %s | (%s) | %d | %.3f | %.3f | %.3f | %.3f .. %.3f | %s | %s |" % (
            s["scene"], s["form"], s["method"], s["particles"], s["ms_mean"], s["ms_median"], s["ms_sd"], s["ms_min"], s["ms_max"],
            "%.3f" % s["ratio_to_a"] if "ratio_to_a" in s and s["method"] != "a" else "", verdict))
    for s in sums:
        if "parent_a_mean" in s:
            out += ["", "%s, single, (b) against (a) of the parent commit's build: %.3f ms against %.3f +- %.3f ms, ratio %.3f: %s." % (
                s["scene"], s["ms_mean"], s["parent_a_mean"], s["parent_a_sd"], s["ratio_to_parent_a"],
                "not slower" if s["not_slower_than_parent_a"] else "SLOWER")]
    out += ["", "What (b) moves: %d B per particle to the host instead of %d B, narrowed on the device." % (RECORD_BYTES, DOWNLOAD_BYTES_PER_PARTICLE)]
    for s in sums:
        if s["method"] == "b" and s["form"] == "single":
            out.append("%s: %.1f MB in %.3f ms = %.1f GB/s effective into the caller's pageable arrays, two pack launches and two" % (
                s["scene"], s["particles"] * RECORD_BYTES / 1e6, s["ms_mean"], s["particles"] * RECORD_BYTES / s["ms_mean"] / 1e6))
            out.append("synchronisations included (how that splits into link, staging and launch time: the copy statistics below, as far as they go).")
    for s in sums:
        if s["method"] == "c":
            out += ["", "%s: the host slept %.2f ms (one `_step` of the scene) between begin and end." % (s["scene"], s["step_ms"])]
    out += ["", "## The pack kernel", ""]
    if a.kernel_trace and os.path.exists(a.kernel_trace):
        kernel_table(a, meta, out)
    else:
        out.append("not measured")
    out += ["", "## Copies of the same profiler run (`--memory-copy-trace --stats`, all four mesh sizes mixed)", ""]
    if a.copy_stats and os.path.exists(a.copy_stats):
        out += ["| copy | calls | mean us | min us | max us |", "|---|---|---|---|---|"]
        for r in csv.DictReader(open(a.copy_stats)):
            out.append("| %s | %s | %.2f | %.2f | %.2f |" % (r["Name"], r["Calls"], float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))
    else:
        out.append("not measured")
    open(a.report, "w").write("\n".join(out) + "\n")
    print("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="config3,config2")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--methods", default="a,b,c", help="methods of the single-handle leg")
    ap.add_argument("--group", type=int, default=2, help="handles of the device-group leg (0: skip it)")
    ap.add_argument("--ranks", type=int, default=2, help="processes of the sharded leg, all on this card over gloo (0: skip it)")
    ap.add_argument("--tree", default=None, help="import the package from this built checkout instead of this one")
    ap.add_argument("--jsonl", default=None)
    ap.add_argument("--jsonl2", default=None)
    ap.add_argument("--kernel-run", action="store_true")
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--copy-stats", default=None)
    ap.add_argument("--trace-out", default=None)
    ap.add_argument("--report", default=None)
    a = ap.parse_args()
    a.methods = a.methods.split(",")
    if a.report:
        return report(a)
    if a.tree:
        sys.path.insert(0, os.path.abspath(a.tree))
    if a.kernel_run:
        return kernel_run(a.frames)
    rows = []
    sink = open(a.jsonl, "w") if a.jsonl else None

    def emit(r):
        r.setdefault("frames", a.frames)
        rows.append(r)
        line = json.dumps(r)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    for name in a.scenes.split(","):  # (an exception in any leg ends the script: nothing more is started on the GPU)
        single(name, a, emit)
        if a.group:
            group(name, a, emit)
        if a.ranks:
            sharded(name, a, emit)
    for s in summarise(list(rows)):
        emit(s)


if __name__ == "__main__":
    main()
