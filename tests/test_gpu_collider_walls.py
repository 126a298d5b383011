"""Wall colliders of the relaxed pass (EGG_COLLIDER_WALL; DESIGN.md section 2.7, "Walls") on the device against the CPU model
tests/wall_model.py, bit for bit: on one handle (the plain and the cohesive wall instantiation of the gather kernel), on
device groups of 2 and 3 handles on GPU 0 (the two group instantiations) and on a ShardedSimulationHandler (two ranks are
spawned processes on GPU 0 over gloo, as in test_gpu_collider_surfaces.py).

Compared: x, y, vx, vy, last_x, last_y of every particle, the environments, the batch positions, pair_solves,
cohesion_solves, viscosity_pairs, collider_hits and collider_grips.  The start of the sub-step (prev) cannot be downloaded;
the velocities are (position - prev) / sub-step, so theirs are its bits.

Every scene drags eggs across a wall -- the target jumps to the far side before the third step, and from the fifth step
on the follow constraint carries particles over it inside one sub-step -- and asserts on the model that the wall caught
particles of every type it covers: no case passes on the segment branch alone."""
import functools
import math

import numpy as np
import pytest

from conftest import ROOT
from relaxed_model import rm
from surface_model import SurfaceModel
from test_gpu_collider_surfaces import FIELDS, _assert_snapshot, _snapshot
from wall_model import WallModel

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
INF = math.inf
S, C = 2, 3
WHITE3 = dict(cohesion_interaction_distance_factor=3, cohesion_strength=0.99)
CONFIGS = {
    "default": dict(white={}, cohesion=False, viscosity=(0.0, 0.0)),
    "cohesion": dict(white=WHITE3, cohesion=True, viscosity=(0.0, 0.0)),
    "viscosity": dict(white={}, cohesion=False, viscosity=(0.5, 0.5)),
    "both": dict(white=WHITE3, cohesion=True, viscosity=(0.5, 1.0)),
}
WALL = ("wall", 100.0, 380.0, 500.0, 380.0)
ONE = ((300.0, 300.0),)                                   # one default batch: 157 + 15 particles, three waves, the last partly filled
THREE = ((240.0, 300.0), (300.0, 310.0), (360.0, 300.0))  # overlapping batches either side of the cuts below
CUTS = {2: [-INF, 300.0, INF], 3: [-INF, 270.0, 330.0, INF]}  # in x, across the wall: every device owns a stretch of it
DROP = 180.0  # the targets go this far down, across the wall
# name: (config, colliders, surfaces, forces, centers, steps)
SCENES = {
    "alone": ("default", (WALL,), None, (), ONE, 8),
    "order": ("default", (("half_plane", 1.0, 0.0, 270.0), WALL, ("disc", 330.0, 368.0, 10.0)), None, (), ONE, 8),
    "friction": ("default", (WALL,), ((0.5, 60.0, 0.0),), (), ONE, 8),
    "cohesion": ("cohesion", (WALL,), None, (), ONE, 8),
    "viscosity": ("viscosity", (WALL,), None, (), ONE, 8),
    "force": ("default", (WALL,), None, (("uniform", 200.0, 600.0),), ONE, 8),
    "white_only": ("default", (WALL[:5] + ("white",),), None, (), ONE, 8),
    # the group and wire scenes: everything at once, and the plain group instantiation
    "three_all": ("both", (("half_plane", 1.0, 0.0, 200.0), WALL, ("disc", 330.0, 368.0, 10.0)), (0.0, (0.4, -50.0, 0.0), 0.2),
                  (("uniform", 0.0, 400.0),), THREE, 10),
    "three_plain": ("default", (WALL,), None, (), THREE, 6),
}
COVERS_YOLK = {name: name != "white_only" for name in SCENES}


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _model(cfg, colliders, surfaces, forces, cls=WallModel):
    w, y = rm.default_configs()
    c = CONFIGS[cfg]
    m = cls(dict(w, **c["white"]), y, cohesion=c["cohesion"])
    m.set_viscosity(*c["viscosity"])
    m.set_colliders(colliders)
    m.set_forces(forces)
    if surfaces is not None:
        m.set_collider_surfaces(surfaces)
    return m


def _configure(h, cfg, colliders, surfaces, forces):
    """a SimulationHandler, SimulationGroup or ShardedSimulationHandler set up as _model sets the model up"""
    c = CONFIGS[cfg]
    h.set_solver_order("relaxed")
    if c["white"]:
        h.set_white_config(c["white"])
    if c["cohesion"]:
        h.set_cohesion("effective")
    h.set_viscosity(*c["viscosity"])
    h.set_colliders(list(colliders))
    h.set_forces(list(forces))
    if surfaces is not None:
        h.set_collider_surfaces(list(surfaces))
    return h


def _drive(o, ids, centers, k):
    """before the third step every target jumps across the wall"""
    if k == 2:
        for i, (cx, cy) in zip(ids, centers):
            o.set_target_position(i, cx, cy + DROP)


@functools.lru_cache(maxsize=None)
def _model_run(name):
    """the scene on the model, once: snapshots after every step, shared by the tests that need them and never changed"""
    cfg, colliders, surfaces, forces, centers, steps = SCENES[name]
    m = _model(cfg, colliders, surfaces, forces)
    ids = [m.add(cx, cy, 50, 15) for cx, cy in centers]
    snaps = {}
    for k in range(steps):
        _drive(m, ids, centers, k)
        m.update(1 / 60, 1 / 60, S, C)
        snaps[k + 1] = dict(_snapshot(m, ids), catches=list(m.wall_catches))
    n = [m.n_particles(w) // len(ids) for w in (WHITE, YOLK)]
    caught_batches = [sorted({k // n[w] + 1 for k in m.caught_ever[w]}) for w in (WHITE, YOLK)]
    return dict(ids=ids, snaps=snaps, catches=list(m.wall_catches), caught_batches=caught_batches, colliders=m.colliders,
                surfaces=[tuple(s) for s in m.surfaces])


def _assert_reaches_the_branch(name, ref):
    """the wall caught particles of every type it covers -- in every batch -- and the run is not the segment's"""
    ids = ref["ids"]
    print("%s: model catches %s of hits %s, batches with caught particles %s" %
          (name, ref["catches"], ref["snaps"][max(ref["snaps"])]["hits"], ref["caught_batches"]))
    assert ref["catches"][WHITE] > 0 and ref["caught_batches"][WHITE] == ids
    if COVERS_YOLK[name]:
        assert ref["catches"][YOLK] > 0 and ref["caught_batches"][YOLK] == ids
    else:
        assert ref["catches"][YOLK] == 0
    last = ref["snaps"][max(ref["snaps"])]
    assert np.isfinite(last["state"][WHITE]).all() and np.isfinite(last["state"][YOLK]).all()
    line = SCENES[name][1][[c[0] for c in SCENES[name][1]].index("wall")][2]
    assert float(last["state"][WHITE][1].max()) < line  # (no white has crossed)
    assert (float(last["state"][YOLK][1].max()) < line) == COVERS_YOLK[name]


LAUNCHES = 2 * (2 + 5 * S * C + 1)  # both types: begin and mid, five launches per pass, end


# ---- one handle
@pytest.mark.parametrize("name", ["alone", "order", "friction", "cohesion", "viscosity", "force", "white_only"])
def test_one_handle_matches_the_model(egg, name):
    cfg, colliders, surfaces, forces, centers, steps = SCENES[name]
    ref = _model_run(name)
    _assert_reaches_the_branch(name, ref)
    if name == "friction":
        assert min(ref["snaps"][steps]["grips"]) > 0
    if name == "cohesion":
        assert ref["snaps"][steps]["cohered"] > 0
    h = _configure(egg.SimulationHandler(), cfg, colliders, surfaces, forces)
    assert h.get_colliders()[[c[0] for c in colliders].index("wall")][0] == "wall"
    ids = [h.add(cx, cy, 50, 15) for cx, cy in centers]
    assert ids == ref["ids"]
    launches = []
    for k in range(steps):
        _drive(h, ids, centers, k)
        before = h.stats()["kernel_launches"]
        assert h.update(1 / 60, 1 / 60, S, C) == 1
        launches.append(h.stats()["kernel_launches"] - before)
        if k + 1 == 1 or k + 1 >= 5:  # (before the drag; from the step of the first catches on, every step)
            _assert_snapshot(h, ref["snaps"][k + 1], "%s step %d" % (name, k + 1))
    if CONFIGS[cfg]["viscosity"] == (0.0, 0.0):  # five launches per pass with a wall as without (the first step builds atoms besides)
        assert launches[1:] == [LAUNCHES] * (steps - 1), launches


def test_a_wall_that_catches_nothing_is_the_segment_scene(egg):
    """an egg lowered slowly onto a wall under a uniform force (the target goes down 1 px a sub-step, a quarter of a
    radius: the egg is pressed onto the wall and nothing crosses it): the list holds a wall, so the wall instantiation runs, with
    default surfaces -- and every bit is the SEGMENT scene's on the model that does not know the wall.  Then the list is
    toggled: friction on the wall, surfaces reset with [] (the records the wall kernels read are the defaults again), a
    segment in its place (the collider kernels as they were), the wall again."""
    def lowered(kind):
        return [(kind, 100.0, 350.0, 500.0, 350.0)]
    forces = (("uniform", 0.0, 600.0),)
    h = _configure(egg.SimulationHandler(), "default", lowered("wall"), None, forces)
    never = _configure(egg.SimulationHandler(), "default", (), None, ())
    m = _model("default", lowered("segment"), None, forces, cls=SurfaceModel)
    w = _model("default", lowered("wall"), None, forces)
    ids = [h.add(300.0, 300.0, 50, 15)]
    assert [o.add(300.0, 300.0, 50, 15) for o in (m, w, never)] == [ids[0]] * 3
    launches, k = [], 0

    def step(what):
        nonlocal k
        for o in (h, m, w):
            o.set_target_position(ids[0], 300.0, 300.0 + 2.0 * (k + 1))
        before = h.stats()["kernel_launches"]
        assert h.update(1 / 60, 1 / 60, S, C) == 1
        launches.append(h.stats()["kernel_launches"] - before)
        for o in (m, w):
            o.update(1 / 60, 1 / 60, S, C)
        k += 1
        _assert_snapshot(h, _snapshot(m, ids), "step %d, %s, against the segment model" % (k, what))
        _assert_snapshot(h, _snapshot(w, ids), "step %d, %s, against the wall model" % (k, what))

    for _ in range(4):
        step("a wall with default surfaces")
    hits = m.collider_hits[WHITE]
    assert w.wall_catches == [0, 0] and hits > 0 and h.collider_grips() == [0, 0]
    # friction on the wall, and off again with []
    for o in (h, m, w):
        o.set_collider_surfaces([(0.5, 40.0, 0.0)])
    for _ in range(2):
        step("a wall with friction")
    assert m.collider_grips[WHITE] > 0
    grips = list(m.collider_grips)
    for o in (h, m, w):
        o.set_collider_surfaces([])
    assert h.get_collider_surfaces() == [(0.0, 0.0, 0.0)]
    for _ in range(2):
        step("surfaces reset")
    assert m.collider_grips == grips
    # a segment in its place: a list without a wall
    h.set_colliders(lowered("segment"))
    w.set_colliders(lowered("segment"))
    for _ in range(2):
        step("a segment")
    h.set_colliders(lowered("wall"))
    w.set_colliders(lowered("wall"))
    for _ in range(2):
        step("the wall again")
    assert w.wall_catches == [0, 0] and m.collider_hits[WHITE] > hits + 8  # (every phase met the collider)
    for _ in range(2):
        before = never.stats()["kernel_launches"]
        assert never.update(1 / 60, 1 / 60, S, C) == 1
    assert launches[1:] == [never.stats()["kernel_launches"] - before] * (len(launches) - 1) == [LAUNCHES] * (len(launches) - 1)


def test_a_failed_step_counts_no_catch_as_a_hit(egg):
    cfg, colliders, surfaces, forces, centers, steps = SCENES["alone"]
    ref = _model_run("alone")
    h = _configure(egg.SimulationHandler(), cfg, colliders, surfaces, forces)
    ids = [h.add(cx, cy, 50, 15) for cx, cy in centers]
    for k in range(6):
        _drive(h, ids, centers, k)
        h.step(1 / 60, S, C)
    assert h.collider_hits() == ref["snaps"][6]["hits"] and min(ref["snaps"][6]["catches"]) > 0
    assert ref["snaps"][7]["catches"][WHITE] > ref["snaps"][6]["catches"][WHITE]  # (the failing step would catch, too)
    far = h.add(1.0e12, 0.0, 50, 15)  # its cells lie beyond +-2^30: the step fails, after its passes have caught
    with pytest.raises(egg.EggError, match="relaxed order"):
        h.step(1 / 60, S, C)
    assert h.collider_hits() == ref["snaps"][6]["hits"]
    h.remove(far)
    h.step(1 / 60, S, C)
    _assert_snapshot(h, ref["snaps"][7], "the step after the failed one")


# ---- device groups
@pytest.mark.parametrize("n_handles", [2, 3])
def test_device_group_equals_one_handle_and_the_model(egg, n_handles):
    """cuts in x through the overlapping batches and across the wall: every device owns particles the wall catches, and
    holds ghosts near the wall that it must not sweep (their own device does, from their own prev)"""
    for name in ("three_all",) + (("three_plain",) if n_handles == 2 else ()):
        cfg, colliders, surfaces, forces, centers, steps = SCENES[name]
        ref = _model_run(name)
        _assert_reaches_the_branch(name, ref)
        g = _configure(egg.SimulationGroup([0] * n_handles, cuts=CUTS[n_handles]), cfg, colliders, surfaces, forces)
        h = _configure(egg.SimulationHandler(), cfg, colliders, surfaces, forces)
        assert g.get_colliders() == h.get_colliders() and [c[0] for c in g.get_colliders()] == [c[0] for c in colliders]
        assert all(b.get_colliders() == h.get_colliders() for b in g.handles)
        ids = [g.add(x, y, 50, 15) for x, y in centers]
        assert [h.add(x, y, 50, 15) for x, y in centers] == ids == ref["ids"]
        assert len({g.owner(i)[0] for i in ids}) == n_handles  # (every device owns a batch, every batch was caught)
        for k in range(steps):
            _drive(g, ids, centers, k)
            _drive(h, ids, centers, k)
            g.step(1 / 60, S, C)
            h.step(1 / 60, S, C)
        for w in (WHITE, YOLK):
            got = g.particles(w, FIELDS)
            cat = np.concatenate([np.array(got[i]) for i in sorted(got)], axis=1)
            for k, f in enumerate(FIELDS):
                assert np.array_equal(cat[k], h.download(w, f)), "%s type %d field %s" % (name, w, f)
        for i in ids:
            assert g.get_position(i) == h.get_position(i)
        assert sum(b.stats()["pair_solves"] for b in g.handles) == h.stats()["pair_solves"]
        assert g.collider_hits() == h.collider_hits() and g.collider_grips() == h.collider_grips()
        assert all(min(b.collider_hits()) > 0 for b in g.handles)  # (every device's own particles met the wall)
        assert g.halo_counters()["records"] > 0
        _assert_snapshot(h, ref["snaps"][steps], "%s: the one handle" % name)


# ------------------------------------------------------------------------------------------------ sharded
SHARDED = "three_all"
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
        cfg, colliders, surfaces, forces, centers, steps = SCENES[SHARDED]
        sh = ShardedSimulationHandler(SlabLayout(SHARDED_CUTS), rank, dist, lambda: SimulationHandler(device=0), device="cpu")
        _configure(sh, cfg, colliders, surfaces, forces)
        gids = [sh.add(x, y, 50, 15) for x, y in centers]
        for k in range(steps):
            _drive(sh, gids, centers, k)
            sh.step(1 / 60, S, C)
        st = sh.local.stats()
        q.put((rank, "ok", dict(state=_state(sh), pos=sh.positions(), pairs=st["pair_solves"], cohered=st["cohesion_solves"],
                                hits=sh.collider_hits(), grips=sh.collider_grips(), own_hits=sh.local.collider_hits(),
                                colliders=sh.get_colliders(), surfaces=sh.get_collider_surfaces(), halo=sh.halo_counters())))
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
    """two ranks on one GPU, the cut across the wall; cohesion, viscosity, friction and a force on: the fields gathered from
    both ranks are the model's, nothing new travels (a ghost record stays 40 bytes)"""
    res = _spawn(2)
    ref = _model_run(SHARDED)
    _assert_reaches_the_branch(SHARDED, ref)
    snap = ref["snaps"][SCENES[SHARDED][5]]
    ids = sorted(snap["pos"])
    for w in (WHITE, YOLK):
        n = snap["state"][w].shape[1] // len(ids)
        seen = []
        for r in (0, 1):
            for gid, cols in res[r]["state"][w].items():
                seen.append(gid)
                for k, f in enumerate(FIELDS):
                    want = snap["state"][w][k][(gid - 1) * n:gid * n]
                    assert np.array_equal(np.array(cols[k]), want), "type %d field %s batch %d" % (w, f, gid)
        assert sorted(seen) == ids
    types = {1: "white", 2: "yolk", 3: "both"}
    for r in (0, 1):
        assert {g: tuple(p) for g, p in res[r]["pos"].items()} == snap["pos"]
        assert res[r]["hits"] == snap["hits"] and res[r]["grips"] == snap["grips"]
        assert [tuple(c) for c in res[r]["colliders"]] == [(c[0],) + tuple(c[1:(5 if c[0] in ("wall", "segment") else 4)]) + (types[c[5]],)
                                                           for c in ref["colliders"]]
        assert [tuple(s) for s in res[r]["surfaces"]] == ref["surfaces"]
        assert res[r]["halo"]["records"] > 0 and res[r]["halo"]["bytes"] == 40 * res[r]["halo"]["records"]
        assert min(res[r]["own_hits"]) > 0
    assert [sum(res[r]["own_hits"][w] for r in (0, 1)) for w in (WHITE, YOLK)] == snap["hits"]
    assert sum(res[r]["pairs"] for r in (0, 1)) == snap["pairs"]
    assert sum(res[r]["cohered"] for r in (0, 1)) == snap["cohered"] > 0
