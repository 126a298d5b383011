"""Viscosity of the relaxed step (egg_set_viscosity; DESIGN.md section 2.7, "Viscosity") on the device against the CPU model
tests/viscosity_model.py, bit for bit -- positions, velocities, the environment reductions and the pair counter: on one
handle (the viscous rank kernel and the viscosity gather), on a device group (several handles on GPU 0: their group twins,
ghosts that carry u), pass by pass through the egg_rx_* calls, and on a ShardedSimulationHandler (ranks are spawned
processes on GPU 0 over gloo, as in test_gpu_forces.py)."""
import functools

import numpy as np
import pytest

from conftest import ROOT, circle_target
from relaxed_model import rm
from test_gpu_colliders import CONFIGS, CUTS, ENV_KEYS, FIELDS, SCENE, SHARDED_CUTS, _centers
from test_gpu_colliders import _assert_snapshot as _assert_collider_snapshot
from test_gpu_colliders import _snapshot as _collider_snapshot
from test_gpu_forces import EVERYTHING, FORCES
from viscosity_model import ViscosityModel

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
BOTH = (0.5, 1.0)  # (white, yolk) coefficients of the scenes with viscosity on both types
SNAPSHOTS = (1, 6, 12)


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _model(cfg="default", cohesion=False, colliders=(), forces=(), visc=(0.0, 0.0)):
    w, y = rm.default_configs()
    m = ViscosityModel(dict(w, **CONFIGS[cfg]), y, cohesion=cohesion)
    m.set_colliders(colliders)
    m.set_forces(forces)
    m.set_viscosity(*visc)
    return m


def _configure(h, cfg="default", cohesion=False, colliders=(), forces=(), visc=(0.0, 0.0)):
    h.set_solver_order("relaxed")
    if CONFIGS[cfg]:
        h.set_white_config(CONFIGS[cfg])
    if cohesion:
        h.set_cohesion("effective")
    h.set_colliders(list(colliders))
    h.set_forces(list(forces))
    h.set_viscosity(*visc)
    return h


def _handle(egg, **kw):
    return _configure(egg.SimulationHandler(), **kw)


def _snapshot(m, ids):
    return dict(_collider_snapshot(m, ids), vpairs=list(m.viscosity_pairs))


def _assert_snapshot(h, snap, what):
    _assert_collider_snapshot(h, snap, what)
    print("%s: viscosity pairs %s" % (what, h.viscosity_pairs()))
    assert h.viscosity_pairs() == snap["vpairs"], what


# ------------------------------------------------------------------------------------------------ smallest shapes
A, B = (295.0, 296.0), (307.0, 296.0)
SHAPES = {  # batches (spot, radius, white and yolk particles each)
    # A batch holds two particles of a type at least (add refuses a count of 1), so the lone particle and the coincident
    # pair come as batches of two: a batch's first particle starts on the centre and its second 283 px away, so neither
    # has a neighbour within H and prev keeps its bits; two such batches on one spot are two coincident pairs per type and
    # nothing else within H.  (The exactly coincident pair inside ONE pass is tests/test_viscosity_model.py's.)
    "one": [(A, 400, 2)],
    "coincident": [(A, 400, 2), (A, 400, 2)],  # two such batches on one spot: two coincident pairs of each type
    "wave": [(A, 28, 65)],                     # crosses a wave's edge
    "block": [(A, 28, 129), (B, 28, 128)],     # 257 particles in two batches that overlap: crosses a workgroup's edge
}
STEPS = 3


@functools.lru_cache(maxsize=None)
def _small_model_run(shape, S, C, visc):
    """the snapshot after every step on the model, computed once and never changed"""
    m = _model(visc=visc)
    ids = [m.add(x, y, r, r, n, n) for (x, y), r, n in SHAPES[shape]]
    out = []
    for _ in range(STEPS):
        m.update(1 / 60, 1 / 60, S, C)
        out.append(_snapshot(m, ids))
    return ids, out


def _small_case(egg, shape, S, C, visc):
    ids, ref = _small_model_run(shape, S, C, visc)
    _, plain = _small_model_run(shape, S, C, (0.0, 0.0))
    # the case is worth relying on: on the model every type with a coefficient has pairs within H and committed velocities
    # that differ from the c = 0 run's; a type without a coefficient, and the lone particles of "one", have neither.  The
    # one exception: in "coincident" with S = 1, C = 3 the three collision passes of the first sub-step push the yolk's two
    # coincident pairs further apart than H before the only viscosity pass of the step, and they stay apart: there the white
    # alone has pairs (1 of them).
    for w in (WHITE, YOLK):
        on = visc[w] > 0 and shape != "one" and not (shape == "coincident" and (S, C) == (1, 3) and w == YOLK)
        assert (ref[-1]["vpairs"][w] > 0) == on, (shape, w)
        assert (not np.array_equal(ref[-1]["state"][w][2:4], plain[-1]["state"][w][2:4])) == on, (shape, w)
    h = _handle(egg, visc=visc)
    assert [h.add(x, y, r, r, None, None, n, n) for (x, y), r, n in SHAPES[shape]] == ids
    for k in range(STEPS):
        assert h.update(1 / 60, 1 / 60, S, C) == 1
        _assert_snapshot(h, ref[k], "%s, S=%d, C=%d, c=%s, step %d" % (shape, S, C, visc, k + 1))
    assert h.viscosity() == visc


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("S", [1, 2, 3])  # rx_end only; rx_mid once; rx_mid twice
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_smallest_shapes(egg, shape, S, C):
    _small_case(egg, shape, S, C, BOTH)


@pytest.mark.parametrize("visc", [(1.0, 0.0), (0.0, 0.25)])
@pytest.mark.parametrize("shape", ["coincident", "block"])
def test_one_type_only(egg, shape, visc):
    _small_case(egg, shape, 2, 3, visc)


# ------------------------------------------------------------------------------------------------ with everything on
@functools.lru_cache(maxsize=None)
def _model_run(cfg, cohesion, visc=BOTH, S=2, C=3):
    """four_batches with moving targets among SCENE and FORCES on the model, once per (config, cohesion, coefficients):
    snapshots after SNAPSHOTS, shared by the tests that need them and never changed"""
    m, centers = _model(cfg, cohesion, SCENE, FORCES, visc), _centers()
    ids = [m.add(cx, cy, 50, 15) for cx, cy in centers]
    out = {}
    for k in range(max(SNAPSHOTS)):
        for i, c in zip(ids, centers):
            m.set_target_position(i, *circle_target(c, k))
        m.update(1 / 60, 1 / 60, S, C)
        if k + 1 in SNAPSHOTS:
            out[k + 1] = _snapshot(m, ids)
    return out


def _check_reference(cfg, cohesion, visc=BOTH):
    """the scene is worth relying on: on the model the pair counter is not zero and the committed velocities differ from
    the c = 0 run's, for every type with a coefficient"""
    ref, bare = _model_run(cfg, cohesion, visc), _model_run(cfg, cohesion, (0.0, 0.0))
    assert bare[1]["vpairs"] == [0, 0] and min(ref[1]["hits"]) > 0
    for w in (WHITE, YOLK):
        assert (ref[1]["vpairs"][w] > 0) == (visc[w] > 0)
        assert (not np.array_equal(ref[1]["state"][w][2:4], bare[1]["state"][w][2:4])) == (visc[w] > 0)
    assert (ref[max(SNAPSHOTS)]["cohered"] > 0) == cohesion
    return ref


@pytest.mark.parametrize("cfg,cohesion", EVERYTHING)
def test_one_handle_with_everything_on(egg, cfg, cohesion):
    ref = _check_reference(cfg, cohesion)
    h, centers = _handle(egg, cfg=cfg, cohesion=cohesion, colliders=SCENE, forces=FORCES, visc=BOTH), _centers()
    ids = [h.add(cx, cy, 50, 15) for cx, cy in centers]
    for k in range(max(SNAPSHOTS)):
        for i, c in zip(ids, centers):
            h.set_target_position(i, *circle_target(c, k))
        assert h.update(1 / 60, 1 / 60, 2, 3) == 1
        if k + 1 in SNAPSHOTS:
            _assert_snapshot(h, ref[k + 1], "%s step %d" % (cfg, k + 1))


def _assert_group(g, ids, snap, what):
    for w in (WHITE, YOLK):
        got = g.particles(w, FIELDS)
        cat = np.concatenate([np.array(got[i]) for i in sorted(got)], axis=1)
        for q, f in enumerate(FIELDS):
            assert np.array_equal(cat[q], snap["state"][w][q]), "%s type %d field %s" % (what, w, f)
        env = g.get_environment(w)
        for key in ENV_KEYS:
            assert env[key] == snap["env"][w][key], "%s type %d env %s" % (what, w, key)
    for i in ids:
        assert g.get_position(i) == snap["pos"][i], what
    assert sum(b.stats()["pair_solves"] for b in g.handles) == snap["pairs"], what
    assert sum(b.stats()["cohesion_solves"] for b in g.handles) == snap["cohered"], what
    assert g.collider_hits() == snap["hits"], what
    print("%s: viscosity pairs %s" % (what, g.viscosity_pairs()))
    assert g.viscosity_pairs() == snap["vpairs"], what


@pytest.mark.parametrize("n_handles", [2, 3])
@pytest.mark.parametrize("cfg,cohesion,visc", [EVERYTHING[0] + (BOTH,), EVERYTHING[1] + (BOTH,), EVERYTHING[0] + ((1.0, 0.0),)])
def test_device_group_with_everything_on(egg, cfg, cohesion, visc, n_handles):
    """cuts through the cluster: a pair within H across a cut smooths both sides, through ghosts that carry u"""
    ref = _check_reference(cfg, cohesion, visc)
    g = _configure(egg.SimulationGroup([0] * n_handles, cuts=CUTS[n_handles]), cfg, cohesion, SCENE, FORCES, visc)
    assert g.viscosity() == visc and all(b.viscosity() == visc for b in g.handles)
    centers = _centers()
    ids = [g.add(x, y, 50, 15) for x, y in centers]
    assert len({g.owner(i)[0] for i in ids}) >= 2
    S, C = 2, 3
    for k in range(max(SNAPSHOTS)):
        for i, c in zip(ids, centers):
            g.set_target_position(i, *circle_target(c, k))
        g.step(1 / 60, S, C)
        if k + 1 in SNAPSHOTS:
            _assert_group(g, ids, ref[k + 1], "%d handles, %s, c=%s, step %d" % (n_handles, cfg, visc, k + 1))
    halo = g.halo_counters()
    assert halo["records"] > 0 and halo["passes"] == max(SNAPSHOTS) * (S * C + S)


def test_a_group_whose_handles_differ_refuses_to_step(egg):
    g = egg.SimulationGroup([0, 0], cuts=CUTS[2])
    g.set_solver_order("relaxed")
    g.set_viscosity(0.5, 0.5)
    ids = [g.add(x, y, 50, 15) for x, y in _centers()]
    g.step(1 / 60, 2, 3)
    pairs = g.viscosity_pairs()
    assert min(pairs) > 0
    g.handles[1].set_viscosity(0.5, 0.25)
    with pytest.raises(egg.EggError, match="differ in their viscosity"):
        g.step(1 / 60, 2, 3)
    assert g.viscosity_pairs() == pairs
    g.set_viscosity(0.5, 0.5)
    g.step(1 / 60, 2, 3)
    assert len(ids) == 4 and g.viscosity_pairs()[WHITE] > pairs[WHITE]


# ------------------------------------------------------------------------------------------------ toggling, rules
def test_toggling(egg):
    h, m = _handle(egg), _model()
    centers = _centers()
    ids = [h.add(cx, cy, 50, 15) for cx, cy in centers]
    assert [m.add(cx, cy, 50, 15) for cx, cy in centers] == ids
    S, C = 2, 3
    launches = {}
    for visc in ((0.0, 0.0), BOTH, (1.0, 0.0), (0.0, 0.0)):
        h.set_viscosity(*visc)
        m.set_viscosity(*visc)
        for _ in range(2):
            before = h.stats()["kernel_launches"]
            assert h.update(1 / 60, 1 / 60, S, C) == 1
            m.update(1 / 60, 1 / 60, S, C)
            launches.setdefault(visc, []).append(h.stats()["kernel_launches"] - before)
            _assert_snapshot(h, _snapshot(m, ids), "c=%s" % (visc,))
    # counted the way test_gpu_relaxed.test_launches_of_one_step counts (a handle's first step builds its per-particle atoms
    # besides): five launches more per sub-step for each type with a coefficient, the parent's count without
    parent = 2 * (S + 5 * S * C + 1)
    assert launches[(0.0, 0.0)][1:] == [parent] * 3
    assert launches[BOTH] == [parent + 2 * 5 * S] * 2 and launches[(1.0, 0.0)] == [parent + 5 * S] * 2
    assert min(m.viscosity_pairs) > 0
    # after on -> off a step gives the bits of a handle that never had a coefficient, from the same state
    a, b = egg.SimulationHandler(), egg.SimulationHandler()
    for x in (a, b):
        x.set_solver_order("relaxed")
        for cx, cy in centers:
            x.add(cx, cy, 50, 15)
    a.set_viscosity(*BOTH)
    a.set_viscosity(0.0, 0.0)
    for _ in range(2):
        counts = []
        for x in (a, b):
            before = x.stats()["kernel_launches"]
            assert x.update(1 / 60, 1 / 60, S, C) == 1
            counts.append(x.stats()["kernel_launches"] - before)
        assert counts[0] == counts[1]
    for w in (WHITE, YOLK):
        for f in FIELDS:
            assert np.array_equal(a.download(w, f), b.download(w, f)), (w, f)
    assert a.viscosity_pairs() == [0, 0]


def test_rules(egg):
    h = _handle(egg, visc=(0.25, 1.0))
    h.add(400.0, 300.0, 50, 15)
    nan = float("nan")
    lib = egg._ffi.load()
    for bad in ((nan, 0.0), (0.0, nan), (-0.5, 0.0), (0.0, 1.5), (float("inf"), 0.0)):
        arr = (egg._ffi.C.c_double * 2)(*bad)
        assert lib.egg_set_viscosity(h._h, arr) == egg._ffi.EGG_ERR_INVALID_ARGUMENT  # (the library's own check)
        assert b"outside [0, 1]" in lib.egg_last_error(h._h)
        with pytest.raises(egg.EggError, match="outside"):
            h.set_viscosity(*bad)
        assert h.viscosity() == (0.25, 1.0)
    assert lib.egg_set_viscosity(h._h, None) == egg._ffi.EGG_ERR_INVALID_ARGUMENT
    with pytest.raises(egg.EggError, match="exact order has no viscosity"):
        h.set_solver_order("exact")
    assert h.get_solver_order() == "relaxed" and h.viscosity() == (0.25, 1.0)
    h.set_viscosity(0.0, 1.0)
    with pytest.raises(egg.EggError, match="exact order has no viscosity"):
        h.set_solver_order("exact")
    h.set_viscosity()
    h.set_solver_order("exact")
    h.set_viscosity(0.0, 0.0)  # both zero is always accepted
    for bad in ((0.5, 0.0), (0.0, 1.0)):
        with pytest.raises(egg.EggError, match="relaxed order"):
            h.set_viscosity(*bad)
    assert h.viscosity() == (0.0, 0.0)
    h.step_begin(1 / 60, 2, 3)
    with pytest.raises(egg.EggError, match="in flight"):
        h.set_viscosity(0.0, 0.0)
    h.step_end(True)
    # the group: the same rules, and refused values change no handle
    g = egg.SimulationGroup([0, 0], cuts=CUTS[2])
    g.set_viscosity(0.0, 0.0)
    with pytest.raises(egg.EggError, match="relaxed order"):
        g.set_viscosity(0.5, 0.5)
    g.set_solver_order("relaxed")
    g.set_viscosity(0.5, 0.75)
    with pytest.raises(egg.EggError, match="outside"):
        g.set_viscosity(0.5, 2.0)
    assert g.viscosity() == (0.5, 0.75) and all(b.viscosity() == (0.5, 0.75) for b in g.handles)
    with pytest.raises(egg.EggError, match="exact order has no viscosity"):
        g.set_solver_order("exact")
    assert g.get_solver_order() == "relaxed"
    g.set_viscosity()
    g.set_solver_order("exact")


def test_a_failed_step_adds_nothing_and_commits_nothing(egg):
    h, m = _handle(egg, visc=BOTH), _model(visc=BOTH)
    ids = [h.add(300.0, 300.0, 50, 15)]
    assert [m.add(300.0, 300.0, 50, 15)] == ids
    assert h.update(1 / 60, 1 / 60, 2, 3) == 1
    m.update(1 / 60, 1 / 60, 2, 3)
    pairs = h.viscosity_pairs()
    assert min(pairs) > 0
    h.set_forces([("uniform", 1.0e18, 0.0)])  # throws the particles beyond cell +-2^30: the bad-cell flag fails the step
    with pytest.raises(egg.EggError, match="relaxed order"):
        h.step(1 / 60, 2, 3)
    assert h.stats()["steps"] == 1 and h.viscosity_pairs() == pairs
    h.set_forces([])
    assert h.update(1 / 60, 1 / 60, 2, 3) == 1
    m.update(1 / 60, 1 / 60, 2, 3)
    _assert_snapshot(h, _snapshot(m, ids), "after the failed step")


def _drive_wire(egg, h, S, C, commit):
    """one relaxed step pass by pass through the egg_rx_* calls, with no other rank: no partner, no message"""
    none_boxes, none = np.zeros((0, 2, 5), dtype=np.int32), np.zeros((0, 2), dtype=np.int64)
    h.rx_begin(1 / 60, S, C)
    for sub in range(S):
        h.rx_substep(sub)
        passes = [sub * C + c for c in range(C)]
        if any(h.viscosity()):
            passes.append(egg._ffi.RX_VISCOSITY_PASS + sub)
        for p in passes:
            boxes = h.rx_get_boxes(p)
            if p >= egg._ffi.RX_VISCOSITY_PASS:  # a type without a coefficient sits the pass out
                assert [int(b[4]) for b in boxes] == [0 if c > 0 else 1 for c in h.viscosity()]
            assert h.rx_pack(p, none_boxes).shape == (0, 2)
            h.rx_run_pass(p, none.astype(np.uint64), none)
    bad, _pairs, _records = h.rx_check()
    assert not bad
    h.rx_end(commit)


@pytest.mark.parametrize("visc", [BOTH, (0.0, 0.75)])
def test_pass_by_pass_and_a_discarded_step(egg, visc):
    """the egg_rx_* sequence with EGG_RX_VISCOSITY_PASS + sub on one handle: a discarded step adds nothing to the counter and
    commits nothing, a committed one is the model's; the sequence rules hold"""
    S, C = 2, 3
    h, m = _handle(egg, visc=visc), _model(visc=visc)
    ids = [h.add(x, y, 50, 15) for x, y in _centers()[:2]]
    assert [m.add(x, y, 50, 15) for x, y in _centers()[:2]] == ids
    n = h.get_n_particles()
    for w in (WHITE, YOLK):
        h.rx_set_keys(w, ids, [0, n[w] // 2], n[w])
    before = [np.array([h.download(w, f) for f in FIELDS]) for w in (WHITE, YOLK)]
    _drive_wire(egg, h, S, C, False)
    assert h.viscosity_pairs() == [0, 0] and h.stats()["steps"] == 0
    for w in (WHITE, YOLK):
        assert np.array_equal(np.array([h.download(w, f) for f in FIELDS]), before[w])
    for k in range(2):
        _drive_wire(egg, h, S, C, True)
        m.update(1 / 60, 1 / 60, S, C)
        _assert_snapshot(h, _snapshot(m, ids), "pass by pass, c=%s, step %d" % (visc, k + 1))
    assert max(h.viscosity_pairs()) > 0
    # out of sequence: the viscosity pass before the sub-step's collision passes have run, the next sub-step and the check
    # before the viscosity pass has run
    V = egg._ffi.RX_VISCOSITY_PASS
    none = np.zeros((0, 2), dtype=np.int64)
    h.rx_begin(1 / 60, S, C)
    h.rx_substep(0)
    with pytest.raises(egg.EggError, match="out of sequence"):
        h.rx_get_boxes(V)
    for p in range(C):
        h.rx_run_pass(p, none.astype(np.uint64), none)
    with pytest.raises(egg.EggError, match="out of sequence"):
        h.rx_substep(1)
    with pytest.raises(egg.EggError, match="out of sequence"):
        h.rx_run_pass(C, none.astype(np.uint64), none)
    with pytest.raises(egg.EggError, match="out of sequence"):
        h.rx_get_boxes(V + 1)
    h.rx_run_pass(V, none.astype(np.uint64), none)
    h.rx_substep(1)
    h.rx_end(False)
    # refused while both coefficients are 0
    h.set_viscosity(0.0, 0.0)
    h.rx_begin(1 / 60, 1, 1)
    h.rx_substep(0)
    h.rx_run_pass(0, none.astype(np.uint64), none)
    with pytest.raises(egg.EggError, match="both coefficients are 0"):
        h.rx_get_boxes(V)
    h.rx_end(False)


# ------------------------------------------------------------------------------------------------ sharded
# (config, cohesion, coefficients, steps, cuts).  "cut": through the cluster.  "empty": every batch on rank 0, rank 1 holds
# no particle of either type and still walks the sequence with its viscosity passes -- with both coefficients, and with one
# type's alone (a batch always has particles of both types, so no rank can hold one type only; what a type without
# particles does on a rank is what the empty rank does for both).
SHARDED_LAYOUTS = {"cut": SHARDED_CUTS, "empty": [-2000.0, 1000.0, 2000.0]}
SHARDED = [EVERYTHING[0] + (BOTH, 12, "cut"), EVERYTHING[1] + (BOTH, 6, "cut"), EVERYTHING[0] + ((1.0, 0.0), 1, "cut"),
           EVERYTHING[0] + ((0.0, 0.0), 1, "cut"), EVERYTHING[0] + (BOTH, 6, "empty"), EVERYTHING[0] + ((0.0, 0.25), 1, "empty")]


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
        out = {}
        for cfg, cohesion, visc, steps, cuts in SHARDED:
            sh = ShardedSimulationHandler(SlabLayout(SHARDED_LAYOUTS[cuts]), rank, dist, lambda: SimulationHandler(device=0), device="cpu")
            _configure(sh, cfg, cohesion, SCENE, FORCES, visc)
            centers = _centers()
            gids = [sh.add(x, y, 50, 15) for x, y in centers]
            for k in range(steps):
                for gid, c in zip(gids, centers):
                    sh.set_target_position(gid, *circle_target(c, k))
                sh.step(1 / 60, 2, 3)
                if k + 1 in SNAPSHOTS:
                    st = sh.local.stats()
                    out[(cfg, visc, cuts, k + 1)] = dict(state=_state(sh), pos=sh.positions(), n_local=sum(sh.local.get_n_particles()), pairs=st["pair_solves"], cohered=st["cohesion_solves"],
                                                   hits=sh.collider_hits(), vpairs=sh.viscosity_pairs(), visc=sh.viscosity(),
                                                   env=[sh.get_environment(w) for w in (WHITE, YOLK)], halo=sh.halo_counters())
        q.put((rank, "ok", out))
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
    """two ranks on one GPU, the cut through the cluster, with everything on; cohesion off, then on, then white only; then
    every batch on rank 0 and rank 1 empty: the fields gathered from both ranks are the model's (and so the single
    handle's, which the tests above hold to the model), and the halo counters of every rank, the empty one too, show
    exactly S more passes per step than the same scene with both coefficients 0"""
    res = _spawn(2)
    S, C = 2, 3
    for cfg, cohesion, visc, steps, cuts in SHARDED:
        ref = _check_reference(cfg, cohesion, visc) if any(visc) else _model_run(cfg, cohesion, visc)
        for step in [s for s in SNAPSHOTS if s <= steps]:
            snap, got = ref[step], [res[r][(cfg, visc, cuts, step)] for r in (0, 1)]
            what = "%s c=%s %s step %d" % (cfg, visc, cuts, step)
            ids = sorted(snap["pos"])
            for w in (WHITE, YOLK):
                n = snap["state"][w].shape[1] // len(ids)
                seen = []
                for r in (0, 1):
                    for gid, cols in got[r]["state"][w].items():
                        seen.append(gid)
                        for k, f in enumerate(FIELDS):
                            want = snap["state"][w][k][(gid - 1) * n:gid * n]
                            assert np.array_equal(np.array(cols[k]), want), "%s type %d field %s batch %d" % (what, w, f, gid)
                assert sorted(seen) == ids
                envs = [got[r]["env"][w] for r in (0, 1) if got[r]["env"][w] is not None]
                assert len(envs) == 1
                for key in ENV_KEYS:
                    assert envs[0][key] == snap["env"][w][key], "%s type %d env %s" % (what, w, key)
            for r in (0, 1):
                assert {g: tuple(p) for g, p in got[r]["pos"].items()} == snap["pos"]
                assert got[r]["hits"] == snap["hits"] and got[r]["visc"] == visc
                assert got[r]["vpairs"] == snap["vpairs"], what  # (all-reduced: every rank reports the sum)
                assert (got[r]["halo"]["records"] > 0) == (cuts == "cut"), what
                assert (got[r]["n_local"] > 0) == (cuts == "cut" or r == 0), what
                assert got[r]["halo"]["passes"] == step * (S * C + (S if any(visc) else 0)), what
            assert sum(got[r]["pairs"] for r in (0, 1)) == snap["pairs"]
            assert sum(got[r]["cohered"] for r in (0, 1)) == snap["cohered"]
