"""ShardedSimulationHandler in relaxed order ("Several processes"): ranks are spawned processes on
GPU 0 over gloo, exactly as in test_gpu_sharded.py (at most 4 ranks + this process), every child joined with a time
limit.  Every comparison is np.array_equal: against the CPU model tests/relaxed_model.py for the first scene, against
ONE relaxed SimulationHandler in this process otherwise (test_gpu_relaxed.py pins that to the model) -- never against
another sharded run.

`add` of the sharded handler always creates both particle types with the default counts, so a rank with yolk-less or
white-less input cannot occur; a rank that owns nothing can, and is covered (scene 4, and every scene after its
batches have strayed)."""
import math
import os
import socket
import sys

import numpy as np
import pytest

from conftest import ROOT, circle_target, load_golden
from relaxed_model import RelaxedModel

pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "vx", "vy", "last_x", "last_y")
BAD_X = 1.0e12  # cells beyond +-2^30: the case test_gpu_relaxed.py uses


# ------------------------------------------------------------------------------------------------ scenes
# A scene is a list of RUNS; a run = dict(cuts, centers, S, C, omega, steps, target(gid, k) -> (x, y) or None,
# orders = [(first step, order)], mix = step()/update() alternate, bad = add a batch at BAD_X and expect the step to fail)

def _four_batches_runs(world):
    centers = [tuple(float(v) for v in c) for c in load_golden("four_batches")["centers"]]
    cuts = [-2000.0, 10.0, 2000.0] if world == 2 else [-2000.0, -10.0, 20.0, 2000.0]  # through the cluster
    return [dict(cuts=cuts, centers=centers, S=S, C=C, omega=omega, steps=8, target="circle",
                 probe=(S, C) in ((2, 3), (1, 1)) and omega == 1.0)  # probe: _probe_launches after the run
            for S, C in ((2, 3), (1, 1), (3, 2)) for omega in (1.0, 1.8)]


def _swap2_target(centers):
    def target(gid, step):
        cx, cy = centers[gid - 1]
        t = min(1.0, step / 40.0)
        return (cx + (480.0 if cx < 1000 else -480.0) * t, cy + 10.0 * t)
    return target


def _swap4_target(centers):
    def target(gid, step):
        cx, cy = centers[gid - 1]
        t = min(1.0, step / 45.0)
        if gid <= 3:
            return (cx + 1000.0 * t, cy + 15.0 * t)
        if 7 <= gid <= 9:
            return (cx - 470.0 * t, cy)
        return (cx, cy)
    return target


def _cfg4_centers():
    return [(100.0 + 160.0 * c, 100.0 + 160.0 * r) for r in range(6) for c in range(16)]


def _scene(name, world):
    if name == "four_batches":
        return _four_batches_runs(world)
    if name == "swap2":  # test_gpu_sharded._scenario: two columns swap sides through each other
        centers = [(760.0, 150.0 + 300.0 * k) for k in range(5)] + [(1240.0, 150.0 + 300.0 * k) for k in range(5)]
        return [dict(cuts=[0.0, 1000.0, 2000.0], centers=centers, S=2, C=3, omega=1.8, steps=70, target="swap2", mix=True)]
    if name == "swap4":  # test_gpu_sharded._scenario4
        rows = [150.0, 450.0, 750.0]
        centers = ([(420.0, y) for y in rows] + [(900.0, y + 20.0) for y in rows] + [(1420.0, y - 10.0) for y in rows] +
                   [(2100.0, y) for y in rows])
        return [dict(cuts=[0.0, 600.0, 1200.0, 1800.0, 2400.0], centers=centers, S=2, C=3, omega=1.8, steps=60, target="swap4",
                     mix=True)]
    if name == "small":
        return [
            # coincident batches split over the ranks: three batches at ONE site next to the cut; before the first step
            # id 2 is handed to rank 1 (it sits within the halo of rank 1's slab and stays there)
            dict(cuts=[0.0, 1000.0, 2000.0], centers=[(990.0, 300.0)] * 3, S=2, C=3, omega=1.8, steps=12, target=None,
                 move={2: 1}),
            # a rank that owns nothing
            dict(cuts=[0.0, 1000.0, 2000.0], centers=[(300.0, 300.0), (330.0, 310.0), (700.0, 300.0)], S=2, C=3, omega=1.8,
                 steps=6, target=None),
            # mode switches exact -> relaxed -> exact mid-run
            # (the two-column swap: ten batches keep the exact order's yolk budget from binding)
            dict(cuts=[0.0, 1000.0, 2000.0], centers=[(760.0, 150.0 + 300.0 * k) for k in range(5)] +
                 [(1240.0, 150.0 + 300.0 * k) for k in range(5)], S=2, C=3, omega=1.8, steps=45, target="swap2",
                 orders=[(0, "exact"), (15, "relaxed"), (30, "exact")]),
        ]
    if name == "cfg4":  # test_gpu_sharded._worker_cfg4: no batch comes near a cut
        return [dict(cuts=[20.0 + 640.0 * k for k in range(5)], centers=_cfg4_centers(), S=2, C=3, omega=1.8, steps=8,
                     target="cfg4")]
    if name == "bad":
        return [dict(cuts=[0.0, 1000.0, 2000.0], centers=[(300.0, 300.0), (1500.0, 300.0), (BAD_X, 0.0)], S=2, C=3, omega=1.8,
                     steps=1, target=None, bad=True)]
    raise KeyError(name)


def _target_fn(run):
    kind, centers = run["target"], run["centers"]
    if kind is None:
        return None
    if kind == "circle":
        return lambda gid, k: circle_target(centers[gid - 1], k)
    if kind == "swap2":
        return _swap2_target(centers)
    if kind == "swap4":
        return _swap4_target(centers)
    if kind == "cfg4":
        return lambda gid, k: (centers[gid - 1][0] + 20.0 * math.cos(0.5 * k), centers[gid - 1][1] + 20.0 * math.sin(0.5 * k))
    raise KeyError(kind)


def _drive(sim, run, set_order, after_add=None):
    """the same calls on a sharded handler, one handler or the model"""
    gids = [sim.add(x, y, 50, 15) for x, y in run["centers"]]
    if after_add is not None:
        after_add()
    target = _target_fn(run)
    orders = dict(run.get("orders", [(0, "relaxed")]))
    for k in range(run["steps"]):
        if k in orders:
            set_order(orders[k], run["omega"])
        if target is not None:
            for g in gids:
                sim.set_target_position(g, *target(g, k))
        if run.get("mix") and k % 2 == 1:
            assert sim.update(1 / 60, 1 / 60, run["S"], run["C"]) == 1
        else:
            sim.step(1 / 60, run["S"], run["C"])
    return gids


# ------------------------------------------------------------------------------------------------ ranks

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _state(sh):
    out = {}
    for which in (0, 1):
        b = sh.local.download(which, "batch_id")
        cols = [sh.local.download(which, f) for f in FIELDS]
        out[which] = {sh.global_id[int(l)]: [c[b == l].tolist() for c in cols] for l in np.unique(b)}
    return out


def _probe_launches(sh, run):
    """one more step after a run's results are taken: the increase of the handle's kernel_launches from its start to
    its commit (the stray rule after the commit launches a centroid kernel of its own), the particles the handle holds
    per type and, per pass, (partners, white records received, yolk records received)"""
    passes, exchange, rebalance, after = [], sh.halo.exchange, sh._rebalance_relaxed, []

    def spy(p):
        pointers, counts = exchange(p)
        passes.append((len(sh.halo.partners), int(counts[:, 0].sum()), int(counts[:, 1].sum())))
        return pointers, counts

    def committed():
        after.append(sh.local.stats()["kernel_launches"])
        return rebalance()

    sh.halo.exchange, sh._rebalance_relaxed = spy, committed
    # a hand-over after a step makes the next one rebuild the atom and key tables (one launch each per type): the step
    # counted is one that follows a step without hand-over (sh.migrations is the same number on every rank)
    handed_over = True
    for _ in range(4):
        del passes[:], after[:]
        moved = sh.migrations
        n = list(sh.local.get_n_particles())
        before = sh.local.stats()["kernel_launches"]
        sh.step(1 / 60, run["S"], run["C"])
        if not handed_over:
            break
        handed_over = sh.migrations != moved
    else:
        raise AssertionError("the scene kept handing batches over")
    del sh.halo.exchange, sh._rebalance_relaxed
    return dict(delta=after[0] - before, n=n, passes=passes)


def _worker(rank, world, port, name, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from egg_fluid_simulation_amd import EggError, SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler, SlabLayout
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        results = []
        for run in _scene(name, world):
            sh = ShardedSimulationHandler(SlabLayout(run["cuts"]), rank, dist, lambda: SimulationHandler(device=0), device="cpu")
            res = {}
            if run.get("bad"):
                sh.set_solver_order("relaxed", run["omega"])
                for x, y in run["centers"]:
                    sh.add(x, y, 50, 15)
                before = _state(sh)
                try:
                    sh.step(1 / 60, run["S"], run["C"])
                    res["raised"] = None
                except EggError as e:
                    res["raised"] = str(e)
                res["unchanged"] = all(np.array_equal(np.array(before[w][g]), np.array(v), equal_nan=True)
                                       for w, per in _state(sh).items() for g, v in per.items())
                res["steps"] = sh.local.stats()["steps"]
            else:
                def set_order(order, omega):
                    sh.set_solver_order(order, omega)

                def hand_over():  # run["move"]: batches placed on another rank before the first step
                    for g, dest in sorted(run.get("move", {}).items()):
                        src = sh.owner[g]
                        if rank == src:
                            sh._send_batches([g], dest)
                        elif rank == dest:
                            sh._recv_batches(1, src)
                        sh.owner[g] = dest
                        sh._keys_stale = True

                _drive(sh, run, set_order, hand_over)
                st = sh.local.stats()
                res.update(state=_state(sh), pos=sh.positions(), pairs=st["pair_solves"], steps=st["steps"],
                           relaxed=st["relaxed_steps"], redo=st["redo_steps"], halo=sh.halo_counters(), owner=dict(sh.owner),
                           migrations=sh.migrations, claim_bytes=sh.exchange.bytes_exchanged, n_local=len(sh.local_id),
                           order=sh.get_solver_order(), collectives=sh.halo.collectives)
                if run.get("probe"):
                    res["launches"] = _probe_launches(sh, run)
            results.append(res)
        q.put((rank, "ok", results))
    except Exception:
        import traceback
        q.put((rank, "error: " + traceback.format_exc(), None))
    finally:
        dist.destroy_process_group()


def _spawn(name, world):
    import queue
    import time

    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, name, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    deadline = time.time() + 300
    while len(res) < world and time.time() < deadline:
        try:
            rank, outcome, results = q.get(timeout=2)
            assert outcome == "ok", outcome
            res[rank] = results
        except queue.Empty:
            if any(p.exitcode not in (None, 0) for p in procs):
                break
    for p in procs:
        p.join(20)
        if p.is_alive():
            p.kill()  # the exact child started above
    assert len(res) == world and all(p.exitcode == 0 for p in procs), "a rank failed: see its traceback above"
    return res


# ------------------------------------------------------------------------------------------------ references

class _One:
    """ONE SimulationHandler doing what the ranks did"""

    def __init__(self, egg, run):
        self.h = egg.SimulationHandler()
        self.gids = _drive(self.h, run, lambda order, omega: self.h.set_solver_order(order, omega))

    def field(self, which, f):
        return self.h.download(which, f), self.h.download(which, "batch_id")

    def position(self, g):
        return self.h.get_position(g)

    @property
    def pairs(self):
        return self.h.stats()["pair_solves"]


class _Model:
    """the CPU model doing what the ranks did"""

    def __init__(self, run):
        self.m = RelaxedModel(relaxed=True, relaxation=run["omega"])

        class Sim:  # step() of the handlers = one update of the model
            add = staticmethod(self.m.add)
            set_target_position = staticmethod(self.m.set_target_position)

            @staticmethod
            def step(delta, S, C):
                self.m.update(delta, delta, S, C)

        def set_order(order, omega):
            self.m.relaxed = order == "relaxed"

        self.gids = _drive(Sim, run, set_order)

    def field(self, which, f):
        n = len(self.m.state(which)[0]) // len(self.gids)
        return self.m.state(which)[FIELDS.index(f)], np.repeat(np.array(self.gids), n)

    def position(self, g):
        return tuple(self.m.get_position(g))

    @property
    def pairs(self):
        return self.m.pair_solves


def _compare(res, world, i, ref, what, pairs=True):
    """the i-th run of every rank against the reference: every field of every particle, the batch centroids on every
    rank, the pair counts summed over the ranks"""
    for which in (0, 1):
        seen = set()
        for f_i, f in enumerate(FIELDS):
            want, b = ref.field(which, f)
            for r in range(world):
                for g, cols in res[r][i]["state"][which].items():
                    seen.add((r, g))
                    assert np.array_equal(np.array(cols[f_i]), want[b == g]), "%s: type %d field %s batch %d" % (what, which, f, g)
        assert sorted(g for _, g in seen) == sorted(ref.gids), what  # every batch on exactly one rank
    for g in ref.gids:
        for r in range(world):
            assert tuple(res[r][i]["pos"][g]) == tuple(ref.position(g)), "%s: centroid %d on rank %d" % (what, g, r)
    if pairs:
        assert sum(res[r][i]["pairs"] for r in range(world)) == ref.pairs, what
    for r in range(1, world):
        assert res[r][i]["owner"] == res[0][i]["owner"], "all ranks agree on who owns what"


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


# ------------------------------------------------------------------------------------------------ tests

def _check_launches(got, run, what):
    """The launch sequence of a relaxed step driven through egg_rx_*, counted: per type the rank holds, the single
    handle's S + 5 S C + 1 (begin / mid, five launches per pass, end), one pack launch per pass that has partners and
    one unpack launch per pass in which records of the type arrived (at most 16 partners: one launch each)."""
    S, C = run["S"], run["C"]
    print("%s: %s" % (what, got))
    assert len(got["passes"]) == S * C
    want = 0
    for w in (0, 1):
        if got["n"][w] > 0:
            want += S + 5 * S * C + 1
            want += sum(1 for p in got["passes"] if p[0] > 0) + sum(1 for p in got["passes"] if p[1 + w] > 0)
    assert got["delta"] == want, what


@pytest.mark.parametrize("world", [2, 3])
def test_four_batches_cut_through_the_cluster_match_the_model(world):
    """scene 1: (S, C) in {(2, 3), (1, 1), (3, 2)} x omega in {1.0, 1.8}, moving targets, against RelaxedModel"""
    res = _spawn("four_batches", world)
    for i, run in enumerate(_scene("four_batches", world)):
        what = "world %d S=%d C=%d omega=%g" % (world, run["S"], run["C"], run["omega"])
        _compare(res, world, i, _Model(run), what)
        for r in range(world):
            halo = res[r][i]["halo"]
            assert halo["passes"] == run["steps"] * run["S"] * run["C"], what
            assert halo["bytes"] == 40 * halo["records"]
            assert res[r][i]["relaxed"] == res[r][i]["steps"] == run["steps"]
        assert sum(res[r][i]["halo"]["records"] for r in range(world)) > 0, what
        assert all(res[r][i]["halo"]["records"] > 0 for r in range(world) if res[r][i]["n_local"]), what
        assert ("launches" in res[0][i]) == ((run["S"], run["C"]) in ((2, 3), (1, 1)) and run["omega"] == 1.0)
        for r in range(world):
            if "launches" in res[r][i]:
                _check_launches(res[r][i]["launches"], run, "%s rank %d" % (what, r))


@pytest.mark.parametrize("name,world", [("swap2", 2), ("swap4", 4)])
def test_columns_cross_the_cuts_without_hand_over_before_a_step(egg, name, world):
    """scene 2: batches cross cuts and meet across them, step() and update() mixed.  Nothing is handed over before a
    step (the claim exchange of the exact protocol never runs), every step runs once, ownership changes only through
    the post-step stray rule."""
    res = _spawn(name, world)
    run = _scene(name, world)[0]
    _compare(res, world, 0, _One(egg, run), name)
    for r in range(world):
        out = res[r][0]
        assert out["steps"] == out["relaxed"] == run["steps"] and out["redo"] == 0
        assert out["claim_bytes"] == 0, "the exact protocol's claim exchange ran"
        assert out["halo"]["passes"] == run["steps"] * 6
    assert sum(res[r][0]["halo"]["records"] for r in range(world)) > 0, "the columns must meet across a cut"
    assert res[0][0]["migrations"] > 0, "the stray rule must have moved the batches that crossed"
    layout_owner = {g + 1: int(np.searchsorted(run["cuts"][1:-1], x, side="right")) for g, (x, _) in enumerate(run["centers"])}
    assert res[0][0]["owner"] != layout_owner


def test_coincident_empty_rank_and_mode_switches(egg):
    """scenes 3, 4 and 6 on two ranks"""
    res = _spawn("small", 2)
    runs = _scene("small", 2)
    # 3: ids 1 and 3 on rank 0 and id 2 on rank 1, all at one site: the coincident normal uses the GLOBAL key difference
    _compare(res, 2, 0, _One(egg, runs[0]), "coincident")
    assert res[0][0]["owner"] == {1: 0, 2: 1, 3: 0}
    assert res[0][0]["halo"]["records"] > 0 and res[1][0]["halo"]["records"] > 0
    # 4: rank 1 owns nothing: it still takes part in every collective and counts every step
    _compare(res, 2, 1, _One(egg, runs[1]), "empty rank")
    assert res[1][1]["n_local"] == 0 and res[1][1]["state"] == {0: {}, 1: {}}
    assert res[1][1]["steps"] == res[1][1]["relaxed"] == runs[1]["steps"]
    assert res[1][1]["halo"] == dict(passes=runs[1]["steps"] * 6, records=0, bytes=0)
    # 6: exact -> relaxed -> exact against one handle doing the same switches (pair counts are not compared: the exact
    # protocol may discard and re-run a step)
    _compare(res, 2, 2, _One(egg, runs[2]), "mode switches", pairs=False)
    for r in (0, 1):
        assert res[r][2]["relaxed"] == 15 and res[r][2]["order"] == "exact"
        assert res[r][2]["halo"]["passes"] == 15 * 6


def test_config4_layout_no_ghosts_but_boxes_every_pass(egg):
    """scene 5: the cluster never nears a cut: no ghost record travels, the box all-gather still runs every pass"""
    res = _spawn("cfg4", 4)
    run = _scene("cfg4", 4)[0]
    _compare(res, 4, 0, _One(egg, run), "cfg4")
    for r in range(4):
        out = res[r][0]
        assert out["halo"] == dict(passes=8 * 6, records=0, bytes=0)
        assert out["collectives"] == 8 * 6
        assert out["migrations"] == 0 and out["n_local"] == 24


def test_failed_step_fails_on_every_rank_and_commits_nothing():
    """scene 7: one batch at x = 1e12 on the last rank: a status flag, not a fault"""
    res = _spawn("bad", 2)
    for r in (0, 1):
        out = res[r][0]
        assert out["raised"] is not None and "relaxed order" in out["raised"], out
        assert out["unchanged"] and out["steps"] == 0


def test_world_one(egg):
    """scene 8: one rank just steps its handler"""
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler, SlabLayout
    run = _four_batches_runs(2)[0]
    sh = ShardedSimulationHandler(SlabLayout([-2000.0, 2000.0]), 0, None, lambda: egg.SimulationHandler(device=0))
    gids = _drive(sh, run, lambda order, omega: sh.set_solver_order(order, omega))
    ref = _Model(run)
    assert sh.get_solver_order() == "relaxed"
    for which in (0, 1):
        for f in FIELDS:
            assert np.array_equal(sh.local.download(which, f), ref.field(which, f)[0]), f
    assert sh.local.stats()["pair_solves"] == ref.pairs
    assert sh.halo_counters() == dict(passes=run["steps"] * 6, records=0, bytes=0)
    assert [tuple(sh.positions()[g]) for g in gids] == [ref.position(g) for g in gids]
