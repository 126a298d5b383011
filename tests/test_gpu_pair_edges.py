"""The pair arithmetic of the relaxed step (the collision and the cohesion branch of rx_gather, egg_rx_couple_kernel; DESIGN.md
section 2.7) on the device where the other device files do not go: the exact edges of the rule, every normal of a
coincident pair, the clamp, skipped and tiny pairs, every neighbour cell, the visit order of a sum, a coupling compliance
that is not zero, factors that are not 2, types whose tables differ in size, partners that are ghosts.  Everything is
compared as tests/test_gpu_coupling.py compares it -- x, y, vx, vy, last_x, last_y of every particle, the environments, the
batch positions, pair_solves, cohesion_solves, viscosity_pairs, collider_hits, collider_grips and coupling_solves, bit for
bit against the CPU model -- and every comparison is preceded by the assertion, on the model's census
(tests/pair_census.py), that the scene takes the branches it is there for.  The scenes, those assertions and the check that
a wrong rule would change a scene's state live in tests/test_pair_census.py, which needs no device.

Which test reaches which label of the census (sites: C a type's collision branch, white and yolk alike; K its cohesion
branch; W / Y the white / yolk side of the coupling pass):

  test_hand_case                 one tiny handle per case of test_pair_census.CASES (4 particles per type; 8 or 10 where index
                                 differences up to 7 or 8 are needed), the state imported, one update of (S, C) = (1, 1):
      touching, and one ulp beyond it (apart)                         C (x and y axis), W, Y (axis, and 6-8-10 with factor 2.5)
      coincident_0 .. coincident_7                                    C; W, Y: each from both signs of the index difference
      tiny beside a second partner (averaged_2)                       C, W, Y
      touching beside a second partner (averaged_2)                   C, W, Y
      skipped (pair_solves, coupling_solves stay 0)                   C, W, Y
      clamp_hi                                                        C, W, Y
      coheres, reach_edge and one ulp beyond it, other_batch, clamp_lo   K
      a partner in each of the eight neighbour cells, across the origin   C, W, Y
      three partners in three cells (averaged_3: the order of the sum)    C, W, Y
      factor 0.1: H = max(1.0, ...) takes the 1.0                     W, Y
      strength 0.5 and a second update of (2, 2): the compliance follows the sub-step   W, Y
      closed forms: touching, coincident_0 at C and coincident_1 at W / Y, clamp_hi at C, W, Y, clamp_lo, tiny
  test_coupling_sweep            one default egg, a moving target, 6 steps: (factor, strength) = (2, 0.25), (1.25, 0.9),
                                 (0.1, 1.0), (3, 0) at (S, C) = (1, 1) and (3, 2), and one run that changes the pair before
                                 every step (off in the third): fires, apart, unclamped at W, Y with a compliance > 0
  test_unequal_types             613 + 2 and 2 + 613 particles, coupling on: tables of 2048 and 1024 slots
  test_device_group_ghosts, test_sharded_ghosts   test_pair_census.CUT_CASES on two handles / two ranks, the cut between the
                                 two particles: touching, coincident_1 and coincident_3 (by the global keys) at C, other_batch
                                 beside a mate that coheres at K; a ghost travelled

Shapes: 4 to 10 particles per type in a hand case and a cut case, one default egg (157 + 15) in the sweep, 615 particles in
test_unequal_types.  No scene is at the workload's size.  `dead` has no device case (tests/pair_census.py: it cannot occur).

Out of scope: NaN positions (they fail the step at the insert kernel), the exact-order solver (tests/test_gpu_exact_edges.py), viscosity's own pair
weights, rx_force, coupling on groups (refused by design)."""
import numpy as np
import pytest

import test_pair_census as pc
from conftest import ROOT, circle_target
from relaxed_model import rm
from test_gpu_coupling import _assert_snapshot

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
FIELDS = ("x", "y", "vx", "vy", "last_x", "last_y")
INF = float("inf")
MOST_BATCHES = max(len(c["spots"][WHITE]) for c in pc.CASES.values()) // 2


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


# ------------------------------------------------------------------------------------------------ the hand table
@pytest.fixture(scope="module")
def tiny(egg):
    """the batch infos of as many tiny batches as the largest case needs, exported once from a handle with the default
    configs -- and with them which row of the nine carries what"""
    src = egg.SimulationHandler()
    infos = []
    for b in range(MOST_BATCHES):
        i = src.add(*pc.HAND_TARGET, pc.HAND_RADIUS, pc.HAND_RADIUS, None, None, 2, 2)
        info, ws, ys = src.export_batch(i)
        assert i == b + 1 and ws.shape == ys.shape == (9, 2)
        for state, cfg in zip((ws, ys), rm.default_configs()):
            t = state[8]  # the mass parameter
            assert (0.0 < t).all() and (t < 1.0).all()
            assert state[6].tolist() == [1 / rm.mix(cfg["min_mass"], cfg["max_mass"], float(v)) for v in t]
            assert state[7].tolist() == [rm.mix(cfg["min_radius"], cfg["max_radius"], float(v)) for v in t]
            assert (state[2:4] == 0.0).all() and np.array_equal(state[0:2], state[4:6])
        infos.append(info)
    return infos


def _hand_handle(egg, name):
    c = pc.CASES[name]
    h = egg.SimulationHandler()
    h.set_solver_order("relaxed")
    keys = sorted(set(pc.BASE) | set(pc.CONFIGS[c["cfg"]]))
    w, y = pc.hand_configs(name)
    h.set_white_config({k: w[k] for k in keys})
    h.set_yolk_config({k: y[k] for k in keys})
    if c["cohesion"]:
        h.set_cohesion("effective")
    if c["coupling"]:
        h.set_coupling(*c["coupling"])
    return h


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_hand_case(egg, tiny, name):
    m = pc.assert_hand_labels(name)  # the branches, on the model, first
    _, ids, first = pc.hand_model(name)
    h = _hand_handle(egg, name)
    ws, ys = pc.hand_columns(name, WHITE), pc.hand_columns(name, YOLK)
    for b, i in enumerate(ids):
        assert h.import_batch(tiny[b], ws[:, 2 * b:2 * b + 2], ys[:, 2 * b:2 * b + 2]) == i
    for k, u in enumerate(pc.hand_updates(name)):
        assert h.update(*u) == 1
        if k == 0:
            assert h.stats()["pair_solves"] == first
    _assert_snapshot(h, pc.snapshot(m, ids), name)
    for w, want in (pc.hand_closed_form(name) or {}).items():
        for p, xy in want.items():
            assert (float(h.download(w, "x")[p]), float(h.download(w, "y")[p])) == xy, (name, w, p)


# ------------------------------------------------------------------------------------------------ the coupling sweep
@pytest.mark.parametrize("coupling,sc", pc.SWEEP_KEPT + (("changing", (3, 2)),))
def test_coupling_sweep(egg, coupling, sc):
    S, C = sc
    m, i, snaps = pc.assert_sweep(coupling, S, C)  # cross pairs fire in every step, the egg ends elsewhere than with (2, 1)
    h = egg.SimulationHandler()
    h.set_solver_order("relaxed")
    assert h.add(*pc.SWEEP_CENTER, 50, 15) == i
    for k, snap in enumerate(snaps):
        pair = pc.CHANGING[k] if coupling == "changing" else coupling
        h.set_coupling(*pair)
        h.set_target_position(i, *circle_target(pc.SWEEP_CENTER, k))
        assert h.update(pc.H60, pc.H60, S, C) == 1
        _assert_snapshot(h, snap, "coupling %s, S=%d, C=%d, step %d" % (pair, S, C, k + 1))
        assert h.coupling() == pair


# ------------------------------------------------------------------------------------------------ unequal types
@pytest.mark.parametrize("name", sorted(pc.UNEQUAL))
def test_unequal_types(egg, name):
    m, i, snaps = pc.assert_unequal(name)  # the two tables differ in size (from the counts), cross pairs fire in every step
    nw, ny = pc.UNEQUAL[name]
    h = egg.SimulationHandler()
    h.set_solver_order("relaxed")
    h.set_coupling(*pc.BASELINE)
    assert h.add(*pc.SWEEP_CENTER, 50, 50, None, None, nw, ny) == i
    assert tuple(h.get_n_particles()) == (nw, ny)
    for k, snap in enumerate(snaps):
        h.set_target_position(i, *circle_target(pc.SWEEP_CENTER, k))
        assert h.update(pc.H60, pc.H60, 2, 2) == 1
        _assert_snapshot(h, snap, "%s, step %d" % (name, k + 1))


# ------------------------------------------------------------------------------------------------ ghost partners
def _assert_surface(h, snap, what):
    from test_gpu_collider_surfaces import _assert_snapshot as surface
    surface(h, snap, what)


@pytest.mark.parametrize("name", pc.CUT_CASES)
def test_device_group_ghosts(egg, name):
    """two handles on one GPU, the cut between the two particles of the pair: each meets the other as a ghost"""
    m, ids, snaps = pc.assert_cut_labels(name)
    batches, cut, _ = pc.cut_case(name)
    g = egg.SimulationGroup([0, 0], cuts=[-INF, cut, INF])
    one = egg.SimulationHandler()
    for o in (g, one):
        o.set_solver_order("relaxed")
        o.set_white_config(pc.WHITE3)
        o.set_cohesion("effective")
        assert [o.add(x, y, R, R, None, None, 2, 2) for x, y, R in batches] == ids
    assert [g.owner(i)[0] for i in ids] == [0 if x < cut else 1 for x, y, R in batches]
    assert {g.owner(i)[0] for i in ids} == {0, 1}
    for (_, _, S, C), snap in zip(pc.CUT_UPDATES, snaps):
        g.step(pc.H60, S, C)
        one.step(pc.H60, S, C)
        for w in (WHITE, YOLK):
            got = g.particles(w, FIELDS)
            cat = np.concatenate([np.array(got[i]) for i in sorted(got)], axis=1)
            for k, f in enumerate(FIELDS):
                assert np.array_equal(cat[k], snap["state"][w][k]), "%s type %d field %s: the group against the model" % (name, w, f)
        for i in ids:
            assert g.get_position(i) == snap["pos"][i]
        _assert_surface(one, snap, "%s: the one handle" % name)
        assert sum(b.stats()["pair_solves"] for b in g.handles) == snap["pairs"]
        assert sum(b.stats()["cohesion_solves"] for b in g.handles) == snap["cohered"]
    halo = g.halo_counters()
    assert halo["records"] > 0 and halo["bytes"] == 40 * halo["records"]  # a ghost travelled
    if name == "cut_other_batch":  # the mates cohered on their own handles, beside the ghosts that must not
        assert snaps[-1]["cohered"] > 0


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
        results = {}
        for name in pc.CUT_CASES:
            batches, cut, _ = pc.cut_case(name)
            sh = ShardedSimulationHandler(SlabLayout([-2000.0, cut, 2000.0]), rank, dist, lambda: SimulationHandler(device=0), device="cpu")
            sh.set_solver_order("relaxed")
            sh.set_white_config(pc.WHITE3)
            sh.set_cohesion("effective")
            gids = [sh.add(x, y, R, R, None, None, 2, 2) for x, y, R in batches]
            for _, _, S, C in pc.CUT_UPDATES:
                sh.step(pc.H60, S, C)
            st = sh.local.stats()
            results[name] = dict(gids=gids, state=_state(sh), pos=sh.positions(), pairs=st["pair_solves"], cohered=st["cohesion_solves"],
                                 halo=sh.halo_counters(), owner=dict(sh.owner))
        q.put((rank, "ok", results))
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


def test_sharded_ghosts():
    """two ranks on one GPU (three processes with this one), every cut case in turn: the fields gathered from both ranks
    are the model's, the summed counters are the model's, ghost records travelled"""
    want = {name: pc.assert_cut_labels(name) for name in pc.CUT_CASES}
    res = _spawn(2)
    for name, (m, ids, snaps) in want.items():
        snap = snaps[-1]
        batches, cut, _ = pc.cut_case(name)
        assert all(res[r][name]["gids"] == ids for r in (0, 1))
        assert res[0][name]["owner"] == {i: (0 if x < cut else 1) for i, (x, y, R) in zip(ids, batches)}
        for w in (WHITE, YOLK):
            seen = []
            for r in (0, 1):
                for gid, cols in res[r][name]["state"][w].items():
                    seen.append(gid)
                    for k, f in enumerate(FIELDS):
                        assert np.array_equal(np.array(cols[k]), snap["state"][w][k][2 * (gid - 1):2 * gid]), "%s: type %d field %s batch %d" % (name, w, f, gid)
            assert sorted(seen) == ids
        for r in (0, 1):
            assert {g: tuple(p) for g, p in res[r][name]["pos"].items()} == snap["pos"], name
            halo = res[r][name]["halo"]
            assert halo["records"] > 0 and halo["bytes"] == 40 * halo["records"], name
        assert sum(res[r][name]["pairs"] for r in (0, 1)) == snap["pairs"], name
        assert sum(res[r][name]["cohered"] for r in (0, 1)) == snap["cohered"], name
