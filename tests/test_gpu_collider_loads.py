"""Collider loads of the relaxed pass (egg_set_collider_loads; DESIGN.md section 2.7, "Collider loads") on the device against
the CPU model tests/load_model.py, bit for bit: the hand table of tests/test_load_model.py (two particles per type: a wave
with two lanes in use), one scene per collider flavour the loads kernels stand in for -- plain, surfaces, walls, motion,
motion with pivots, spin -- without and with effective cohesion, a batch smaller than a wave, device groups of 2 and 3
handles on GPU 0 with cuts through the particles that touch the colliders, a ShardedSimulationHandler (two ranks are spawned
processes on GPU 0 over gloo, as in test_gpu_collider_spin.py), and a failed step.

Compared: the raw int64 sums and the dropped count, the doubles collider_loads() returns, and -- loads only observe -- x, y,
vx, vy, last_x, last_y of every particle and every counter against the model and against the same handle with loads off,
which launches what it always launched."""
import functools

import numpy as np
import pytest

import test_collider_census as cc
import test_load_model as tl
from conftest import ROOT
from load_model import LoadModel, convert
from test_gpu_collider_surfaces import FIELDS, _assert_snapshot
from test_gpu_collider_walls import CUTS, LAUNCHES, THREE

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
S, C, H60 = tl.S, tl.C, tl.H60


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _assert_loads(h, step, what):
    """the handle's sums, dropped count and sub-step are the model's integers; its doubles the model's doubles"""
    sums, dropped, sub = h.collider_load_sums()
    print("%s: sums %s dropped %d" % (what, sums, dropped))
    assert (sums, dropped, sub) == step["sums"], what
    assert h.collider_loads() == step["loads"] == convert(sums, sub), what


# ------------------------------------------------------------------------------------------------ the hand table
KEYS = ("damping", "follow_strength", "min_radius", "max_radius", "min_mass", "max_mass")


def _hand_handle(egg, name):
    h = egg.SimulationHandler()
    h.set_solver_order("relaxed")
    w, y = tl.hand_configs(name)
    h.set_white_config({k: w[k] for k in KEYS})
    h.set_yolk_config({k: y[k] for k in KEYS})
    return h


@pytest.mark.parametrize("name", sorted(tl.CASES))
def test_hand_case(egg, name):
    m, mi = tl.hand_model(name)
    src = _hand_handle(egg, name)
    i = src.add(*cc.HAND_TARGET, cc.HAND_RADIUS, cc.HAND_RADIUS, None, None, 2, 2)
    info, ws, ys = src.export_batch(i)
    for state, w in ((ws, WHITE), (ys, YOLK)):
        for p, ((x, y), (vx, vy)) in enumerate(tl.hand_spots(name)[w]):
            state[0, p] = state[4, p] = x
            state[1, p] = state[5, p] = y
            state[2, p], state[3, p] = vx, vy
    for loads in (True, False):
        h = _hand_handle(egg, name)
        tl.hand_configure(h, name, loads)
        assert h.import_batch(info, ws, ys) == i == mi
        assert h.get_collider_loads_enabled() == loads and h.collider_load_sums() == ([(0, 0, 0)] * len(tl.CASES[name]["colliders"]), 0, 0.0)
        assert h.update(*tl.ONE) == 1
        for w in (WHITE, YOLK):
            for k, f in enumerate(FIELDS):
                assert np.array_equal(h.download(w, f), m.state(w)[k]), (name, loads, w, f)
        assert h.collider_hits() == m.collider_hits and h.collider_grips() == m.collider_grips
        if loads:
            _assert_loads(h, dict(sums=m.collider_load_sums(), loads=m.collider_loads()), name)
            assert h.collider_load_sums()[0] == tl.hand_expected(name, m)  # (and the closed form, once more)
        else:
            assert h.collider_load_sums() == ([(0, 0, 0)] * len(tl.CASES[name]["colliders"]), 0, 0.0)


# ------------------------------------------------------------------------------------------------ one handle, every flavour
@pytest.mark.parametrize("cohesion", [False, True], ids=["plain", "cohesive"])
@pytest.mark.parametrize("name", sorted(tl.FLAVOURS))
def test_one_handle_matches_the_model_and_itself_without_loads(egg, name, cohesion):
    ref = tl.flavour_run(name, cohesion)
    assert ref["kept"] > 0
    on = tl.flavour_configure(egg.SimulationHandler(), name, cohesion, loads=True)
    off = tl.flavour_configure(egg.SimulationHandler(), name, cohesion, loads=False)
    counts = {id(on): [], id(off): []}
    for h in (on, off):
        assert [h.add(300.0, 300.0, 50, 15)] == ref["ids"]
    for k, step in enumerate(ref["steps"]):
        for h in (on, off):
            before = h.stats()["kernel_launches"]
            assert h.update(H60, H60, S, C) == 1
            counts[id(h)].append(h.stats()["kernel_launches"] - before)
            _assert_snapshot(h, step["snapshot"], "%s step %d" % (name, k + 1))
            assert [tuple(c) for c in h.get_colliders()] == [tuple(c) for c in step["colliders"]]
            assert [tuple(s) for s in h.get_collider_spin()] == [tuple(s) for s in step["spins"]]
        _assert_loads(on, step, "%s %s step %d" % (name, "cohesive" if cohesion else "plain", k + 1))
        assert off.collider_load_sums() == ([(0, 0, 0)] * len(tl.FLAVOURS[name][0]), 0, 0.0)
        for w in (WHITE, YOLK):  # the same handle with loads off, bit for bit
            for f in FIELDS:
                assert np.array_equal(on.download(w, f), off.download(w, f)), (name, k, w, f)
    # with loads off a step launches what it launched before loads existed; with loads on as many (the first step builds atoms besides)
    assert counts[id(off)][1:] == [LAUNCHES] * (len(ref["steps"]) - 1), counts
    assert counts[id(on)] == counts[id(off)]
    if cohesion:
        assert ref["steps"][-1]["cohered"] > 0


def test_a_batch_smaller_than_a_wave(egg):
    """37 white and 9 yolk particles: one wave per type, partly filled, where a reduction over the wave goes wrong first"""
    m = tl.flavour_configure(tl.flavour_model(False), "srf")
    h = tl.flavour_configure(egg.SimulationHandler(), "srf")
    assert m.add(300.0, 300.0, 50, 15, 37, 9) == h.add(300.0, 300.0, 50, 15, None, None, 37, 9)
    assert h.get_n_particles(1) == (37, 9)
    for k in range(3):
        m.update(H60, H60, S, C)
        assert h.update(H60, H60, S, C) == 1
        _assert_loads(h, dict(sums=m.collider_load_sums(), loads=m.collider_loads()), "small step %d" % (k + 1))
        for w in (WHITE, YOLK):
            for q, f in enumerate(FIELDS):
                assert np.array_equal(h.download(w, f), m.state(w)[q]), (k, w, f)
    assert m.load_contributions > 0 and min(m.collider_hits) > 0


# ------------------------------------------------------------------------------------------------ bookkeeping on the device
def test_a_failed_step_leaves_the_previous_loads_and_setters_zero_them(egg):
    ref = tl.flavour_run("spin", False)
    src = egg.SimulationHandler()
    src.add(300.0, 300.0, 50, 15)
    j = src.add(330.0, 100.0, 50, 15)
    info, ws, ys = src.export_batch(j)
    ws[0, 7] = float("nan")
    h = tl.flavour_configure(egg.SimulationHandler(), "spin")
    h.add(300.0, 300.0, 50, 15)
    for k in range(2):
        assert h.update(H60, H60, S, C) == 1
    _assert_loads(h, ref["steps"][1], "before the failed step")
    held = h.collider_load_sums(), h.collider_loads()
    assert h.import_batch(info, ws, ys) == j
    with pytest.raises(egg.EggError, match="relaxed order: a position is NaN"):
        h.step(H60, S, C)
    assert (h.collider_load_sums(), h.collider_loads()) == held
    h.remove(j)
    assert h.update(H60, H60, S, C) == 1
    _assert_loads(h, ref["steps"][2], "the step after the failed one")
    n = len(tl.FLAVOURS["spin"][0])
    h.set_collider_loads(True)  # the switch zeroes the stored loads ...
    assert h.collider_load_sums() == ([(0, 0, 0)] * n, 0, 0.0) and h.collider_loads() == [(0.0, 0.0, 0.0)] * n
    assert h.update(H60, H60, S, C) == 1
    _assert_loads(h, ref["steps"][3], "the fourth step")
    h.set_colliders([tl.BALL])  # ... and so does a new list, which keeps the switch
    assert h.collider_load_sums() == ([(0, 0, 0)], 0, 0.0) and h.get_collider_loads_enabled()
    assert h.update(H60, H60, S, C) == 1
    assert h.collider_load_sums()[0] != [(0, 0, 0)] and h.collider_load_sums()[2] == H60 / S


def test_the_switch_is_accepted_anywhere_but_in_flight(egg):
    e = egg.SimulationHandler()  # exact order, an empty list: accepted, and nothing is recorded
    e.set_collider_loads(True)
    assert e.get_collider_loads_enabled() and e.collider_loads() == [] and e.collider_load_sums() == ([], 0, 0.0)
    e.add(0.0, 0.0, 50, 15)
    e.step(H60, S, C)
    assert e.collider_load_sums() == ([], 0, 0.0)
    e.step_begin(H60, S, C)
    with pytest.raises(egg.EggError, match="egg_set_collider_loads: a step is in flight"):
        e.set_collider_loads(False)
    e.step_end(True)
    assert e.get_collider_loads_enabled()
    g = egg.SimulationGroup([0, 0], cuts=CUTS[2])
    g.set_solver_order("relaxed")
    g.set_colliders([tl.BALL])
    g.set_collider_loads(True)
    g.add(240.0, 300.0, 50, 15)
    g.add(360.0, 300.0, 50, 15)
    g.handles[1].set_collider_loads(False)
    with pytest.raises(egg.EggError, match="egg_group_set_collider_loads"):
        g.step(H60, S, C)
    g.set_collider_loads(True)
    g.step(H60, S, C)
    assert g.collider_load_sums()[2] == H60 / S


# ------------------------------------------------------------------------------------------------ device groups
GROUP_SCENES = {2: (("spin", True), ("col", False)), 3: (("spin", True),)}


@pytest.mark.parametrize("n_handles", [2, 3])
def test_device_group_equals_one_handle_and_the_model(egg, n_handles):
    """three overlapping eggs, cuts in x through the particles that touch the colliders: every handle sums what its own
    particles did, and the integers added over the handles are one handle's and the model's"""
    for name, cohesion in GROUP_SCENES[n_handles]:
        ref = tl.flavour_run(name, cohesion, THREE)
        assert ref["kept"] > 0
        g = tl.flavour_configure(egg.SimulationGroup([0] * n_handles, cuts=CUTS[n_handles]), name, cohesion)
        h = tl.flavour_configure(egg.SimulationHandler(), name, cohesion)
        ids = [g.add(x, y, 50, 15) for x, y in THREE]
        assert [h.add(x, y, 50, 15) for x, y in THREE] == ids == ref["ids"]
        assert len({g.owner(i)[0] for i in ids}) == n_handles
        for k, step in enumerate(ref["steps"]):
            g.step(H60, S, C)
            h.step(H60, S, C)
            what = "%s, %d handles, step %d" % (name, n_handles, k + 1)
            _assert_loads(h, step, what + ": one handle")
            _assert_loads(g, step, what + ": the group")
            own = [b.collider_load_sums()[0] for b in g.handles]
            assert sum(1 for s in own if any(t != (0, 0, 0) for t in s)) >= 2, own  # (the cut goes through what touches)
        for w in (WHITE, YOLK):
            got = g.particles(w, FIELDS)
            cat = np.concatenate([np.array(got[i]) for i in sorted(got)], axis=1)
            for q, f in enumerate(FIELDS):
                assert np.array_equal(cat[q], h.download(w, f)), "%s type %d field %s" % (name, w, f)
        assert g.collider_hits() == h.collider_hits() == ref["steps"][-1]["hits"]


# ------------------------------------------------------------------------------------------------ sharded
SHARDED = ("spin", True)
SHARDED_CUTS = [-2000.0, 300.0, 2000.0]


def _worker(rank, world, port, q):
    import os
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from egg_fluid_simulation_amd import SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler, SlabLayout
    from test_gpu_sharded_relaxed import _state
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        name, cohesion = SHARDED
        sh = ShardedSimulationHandler(SlabLayout(SHARDED_CUTS), rank, dist, lambda: SimulationHandler(device=0), device="cpu")
        tl.flavour_configure(sh, name, cohesion)
        for x, y in THREE:
            sh.add(x, y, 50, 15)
        steps = []
        for k in range(tl.FLAVOURS[name][5]):
            sh.step(H60, S, C)
            steps.append(dict(sums=sh.collider_load_sums(), loads=sh.collider_loads(), own=sh.local.collider_load_sums()))
        q.put((rank, "ok", dict(state=_state(sh), steps=steps, hits=sh.collider_hits(), enabled=sh.get_collider_loads_enabled())))
    except Exception:
        import traceback
        q.put((rank, "error: " + traceback.format_exc(), None))
    finally:
        dist.destroy_process_group()


def _spawn(world):
    import queue
    import time

    import torch.multiprocessing as mp
    from test_gpu_sharded_relaxed import _free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
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


def test_sharded_two_ranks_match_the_model():
    """two ranks on one GPU, the cut through the eggs and across the turning colliders: the all-reduced integers are the
    model's after every step, on both ranks, and each rank's own sums are a part of them"""
    res = _spawn(2)
    name, cohesion = SHARDED
    ref = tl.flavour_run(name, cohesion, THREE)
    last = ref["steps"][-1]
    ids = ref["ids"]
    for w in (WHITE, YOLK):
        n = last["state"][w].shape[1] // len(ids)
        for r in (0, 1):
            for gid, cols in res[r]["state"][w].items():
                for k, f in enumerate(FIELDS):
                    assert np.array_equal(np.array(cols[k]), last["state"][w][k][(gid - 1) * n:gid * n]), (w, f, gid)
    for r in (0, 1):
        assert res[r]["enabled"] and res[r]["hits"] == last["hits"]
        for k, step in enumerate(ref["steps"]):
            got = res[r]["steps"][k]
            assert (got["sums"][0], got["sums"][1], got["sums"][2]) == step["sums"], (r, k)
            assert got["loads"] == step["loads"], (r, k)
    for k, step in enumerate(ref["steps"]):
        own = [res[r]["steps"][k]["own"] for r in (0, 1)]
        assert all(any(t != (0, 0, 0) for t in o[0]) for o in own), (k, own)  # (both ranks hold particles that touch)
        added = [tuple(a + b for a, b in zip(s0, s1)) for s0, s1 in zip(own[0][0], own[1][0])]
        assert added == step["sums"][0] and own[0][1] + own[1][1] == step["sums"][1], k
