"""Force fields of the relaxed step (egg_set_forces; DESIGN.md section 2.7, "Forces") on the device against the CPU model
tests/force_model.py, bit for bit: on one handle (the begin and mid kernels' force instantiations), on a device group
(several handles on GPU 0: their group instantiations) and on a ShardedSimulationHandler (ranks are spawned processes on
GPU 0 over gloo, as in test_gpu_colliders.py)."""
import functools

import numpy as np
import pytest

from conftest import ROOT, circle_target
from force_model import ForceModel
from relaxed_model import rm
from test_gpu_colliders import CONFIGS, CUTS, ENV_KEYS, FIELDS, INF, SCENE, SHARDED_CUTS, _assert_snapshot, _centers, _snapshot
from test_gpu_colliders import _model_run as _collider_model_run

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
# Gravity, a repelling radial field and a yolk-only vortex over the four_batches cluster (centres (0, 0), (30, 10),
# (-20, 40), (200, 200)) among the colliders' SCENE.  The radial field's centre lies on the 2-handle cut and the sharded
# cut (x = 10) and its reach of 120 px covers the cuts of the 3-handle group (x = -5, 25); the vortex covers them too.  On
# the CPU model both bounded fields act on particles of every type they cover from the first step on (the tests assert
# the model's counts).
FORCES = (("uniform", 0.0, 980.0), ("radial", 10.0, 30.0, -4000.0, 120.0), ("vortex", 40.0, 20.0, 2500.0, 90.0, "yolk"))
SNAPSHOTS = (1, 8, 20)
EVERYTHING = [("default", False), ("white3", True)]  # (config, cohesion)


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _model(cfg="default", cohesion=False, colliders=(), forces=()):
    w, y = rm.default_configs()
    m = ForceModel(dict(w, **CONFIGS[cfg]), y, cohesion=cohesion)
    m.set_colliders(colliders)
    m.set_forces(forces)
    return m


def _handle(egg, cfg="default", cohesion=False, colliders=(), forces=()):
    h = egg.SimulationHandler()
    h.set_solver_order("relaxed")
    if CONFIGS[cfg]:
        h.set_white_config(CONFIGS[cfg])
    if cohesion:
        h.set_cohesion("effective")
    h.set_colliders(list(colliders))
    h.set_forces(list(forces))
    return h


def _step_both(h, m, S=2, C=3):
    assert h.update(1 / 60, 1 / 60, S, C) == 1
    m.update(1 / 60, 1 / 60, S, C)


# ------------------------------------------------------------------------------------------------ smallest shapes
SMALL = {
    "uniform": ("uniform", 0.0, 980.0),
    "radial_in": ("radial", 315.0, 296.0, 4000.0, 80.0),
    "radial_out": ("radial", 315.0, 296.0, -4000.0, 80.0),
    "vortex": ("vortex", 315.0, 296.0, 4000.0, 80.0),
}
SPOTS = [(295.0, 296.0), (307.0, 296.0)]


@functools.lru_cache(maxsize=None)
def _small_model_run(field, n_batches, S, steps=6):
    """1 or 2 batches of 2 white and 2 yolk particles under one field (None: no field) on the model: the snapshot after
    every step and the field's counts, computed once and never changed"""
    m = _model(forces=[SMALL[field]] if field else [])
    ids = [m.add(x, y, 28, 28, 2, 2) for x, y in SPOTS[:n_batches]]
    out = []
    for _ in range(steps):
        m.update(1 / 60, 1 / 60, S, 3)
        out.append(_snapshot(m, ids))
    return ids, out, list(m.force_acts)


@pytest.mark.parametrize("S", [1, 2, 3])  # only rx_begin; rx_mid once; rx_mid twice
@pytest.mark.parametrize("n_batches", [1, 2])
@pytest.mark.parametrize("field", sorted(SMALL))
def test_smallest_shapes(egg, field, n_batches, S):
    ids, ref, acts = _small_model_run(field, n_batches, S)
    _, plain, _ = _small_model_run(None, n_batches, S)
    # the case is worth relying on: the field moved particles of both types in the very first step
    for w in (WHITE, YOLK):
        assert not np.array_equal(ref[0]["state"][w], plain[0]["state"][w]), "the field does not act on type %d" % w
        assert field == "uniform" or acts[w] > 0
    h = _handle(egg, forces=[SMALL[field]])
    assert [h.add(x, y, 28, 28, None, None, 2, 2) for x, y in SPOTS[:n_batches]] == ids
    for k in range(6):
        assert h.update(1 / 60, 1 / 60, S, 3) == 1
        _assert_snapshot(h, ref[k], "%s, %d tiny batches, S=%d, step %d" % (field, n_batches, S, k + 1))
    got = h.get_forces()
    assert got == [SMALL[field] + ("both",)]


def test_masks_and_order(egg):
    """a white-only uniform field and a yolk-only radial field together; then a list of three fields, in both orders: the
    device adds them in list order, as the model does"""
    masked = [("uniform", 0.0, 980.0, "white"), ("radial", 315.0, 296.0, -4000.0, 80.0, "yolk")]
    three = [("uniform", 0.1, 980.0), ("radial", 315.0, 296.0, 4000.0, 80.0), ("vortex", 300.0, 290.0, -3000.0, 60.0)]
    plain = _small_model_run(None, 2, 2)[1]
    for forces in (masked, three, three[::-1]):
        h, m = _handle(egg, forces=forces), _model(forces=forces)
        ids = [h.add(x, y, 28, 28, None, None, 2, 2) for x, y in SPOTS]
        assert [m.add(x, y, 28, 28, 2, 2) for x, y in SPOTS] == ids
        for k in range(6):
            _step_both(h, m)
            _assert_snapshot(h, _snapshot(m, ids), "%d fields, step %d" % (len(forces), k + 1))
            if k == 0:
                for w in (WHITE, YOLK):
                    assert not np.array_equal(m.state(w), plain[0]["state"][w])
        assert (m.force_acts[WHITE] > 0) == (forces is not masked) and m.force_acts[YOLK] > 0
    # under the masked list the white is the white of gravity alone and the yolk the yolk of the radial field alone
    alone = _small_model_run("uniform", 2, 2)[1][5]
    assert np.array_equal(_h_state(egg, masked, WHITE), alone["state"][WHITE])
    assert np.array_equal(_h_state(egg, masked, YOLK), _small_model_run("radial_out", 2, 2)[1][5]["state"][YOLK])


def _h_state(egg, forces, w):
    h = _handle(egg, forces=forces)
    for x, y in SPOTS:
        h.add(x, y, 28, 28, None, None, 2, 2)
    for _ in range(6):
        assert h.update(1 / 60, 1 / 60, 2, 3) == 1
    return np.array([h.download(w, f) for f in FIELDS])


# ------------------------------------------------------------------------------------------------ with everything on
@functools.lru_cache(maxsize=None)
def _model_run(cfg, cohesion, forces=FORCES, S=2, C=3):
    """four_batches with moving targets among SCENE and FORCES on the model, once per (config, cohesion): snapshots after
    SNAPSHOTS, shared by the tests that need them and never changed"""
    m, centers = _model(cfg, cohesion, SCENE, forces), _centers()
    ids = [m.add(cx, cy, 50, 15) for cx, cy in centers]
    out = {}
    for k in range(max(SNAPSHOTS)):
        for i, c in zip(ids, centers):
            m.set_target_position(i, *circle_target(c, k))
        m.update(1 / 60, 1 / 60, S, C)
        if k + 1 in SNAPSHOTS:
            out[k + 1] = dict(_snapshot(m, ids), acts=list(m.force_acts))
    return out


def _check_reference(cfg, cohesion):
    ref, bare = _model_run(cfg, cohesion), _collider_model_run(cfg, cohesion, 2, 3)  # (the same scene without forces)
    assert min(ref[1]["acts"]) > 0 and min(ref[1]["hits"]) > 0, "a field or the colliders do not act on the model"
    assert (ref[20]["cohered"] > 0) == cohesion
    for w in (WHITE, YOLK):
        assert not np.array_equal(ref[1]["state"][w], bare[1]["state"][w])
    return ref


@pytest.mark.parametrize("cfg,cohesion", EVERYTHING)
def test_one_handle_with_everything_on(egg, cfg, cohesion):
    ref = _check_reference(cfg, cohesion)
    h, centers = _handle(egg, cfg, cohesion, SCENE, FORCES), _centers()
    ids = [h.add(cx, cy, 50, 15) for cx, cy in centers]
    for k in range(max(SNAPSHOTS)):
        for i, c in zip(ids, centers):
            h.set_target_position(i, *circle_target(c, k))
        assert h.update(1 / 60, 1 / 60, 2, 3) == 1
        if k + 1 in SNAPSHOTS:
            _assert_snapshot(h, ref[k + 1], "%s step %d" % (cfg, k + 1))


@pytest.mark.parametrize("n_handles", [2, 3])
@pytest.mark.parametrize("cfg,cohesion", EVERYTHING)
def test_device_group_with_everything_on(egg, cfg, cohesion, n_handles):
    """cuts through the cluster and the fields: every device accelerates the particles it owns, and what it moved are
    ghosts of its neighbours in the sub-step's passes"""
    ref = _check_reference(cfg, cohesion)
    g = egg.SimulationGroup([0] * n_handles, cuts=CUTS[n_handles])
    g.set_solver_order("relaxed")
    if CONFIGS[cfg]:
        g.set_white_config(CONFIGS[cfg])
    if cohesion:
        g.set_cohesion("effective")
    g.set_colliders(list(SCENE))
    g.set_forces(list(FORCES))
    assert g.get_forces() == [f if isinstance(f[-1], str) else f + ("both",) for f in FORCES]
    assert all(b.get_forces() == g.get_forces() for b in g.handles)
    centers = _centers()
    ids = [g.add(x, y, 50, 15) for x, y in centers]
    assert len({g.owner(i)[0] for i in ids}) >= 2
    for k in range(max(SNAPSHOTS)):
        for i, c in zip(ids, centers):
            g.set_target_position(i, *circle_target(c, k))
        g.step(1 / 60, 2, 3)
        if k + 1 not in SNAPSHOTS:
            continue
        snap, what = ref[k + 1], "%d handles, %s, step %d" % (n_handles, cfg, k + 1)
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
    assert g.halo_counters()["records"] > 0


def test_a_group_whose_handles_differ_refuses_to_step(egg):
    g = egg.SimulationGroup([0, 0], cuts=CUTS[2])
    g.set_solver_order("relaxed")
    g.set_forces([SMALL["uniform"]])
    ids = [g.add(x, y, 50, 15) for x, y in _centers()]
    g.step(1 / 60, 2, 3)
    g.handles[1].set_forces([("uniform", 0.0, 981.0)])
    with pytest.raises(egg.EggError, match="differ in their force fields"):
        g.step(1 / 60, 2, 3)
    g.set_forces([SMALL["uniform"]])
    g.step(1 / 60, 2, 3)
    assert len(ids) == 4


# ------------------------------------------------------------------------------------------------ toggling, rules
def test_toggling(egg):
    h, m, never = _handle(egg), _model(), _handle(egg)
    centers = _centers()
    ids = [h.add(cx, cy, 50, 15) for cx, cy in centers]
    assert [m.add(cx, cy, 50, 15) for cx, cy in centers] == ids == [never.add(cx, cy, 50, 15) for cx, cy in centers]
    launches = []
    for forces in ((), FORCES, ()):
        h.set_forces(list(forces))
        m.set_forces(forces)
        assert len(h.get_forces()) == len(forces)
        for _ in range(2):
            before = h.stats()["kernel_launches"]
            _step_both(h, m)
            launches.append(h.stats()["kernel_launches"] - before)
            _assert_snapshot(h, _snapshot(m, ids), "with %d fields" % len(forces))
    assert min(m.force_acts) > 0
    # with forces a step launches as many kernels as without (counted the way test_gpu_relaxed.test_launches_of_one_step
    # counts; a handle's first step builds its per-particle atoms besides) ...
    assert launches[1:] == [2 * (2 + 5 * 2 * 3 + 1)] * 5
    # ... and after the clear a step launches what a handle launches that never had a list, and gives its bits when it
    # starts from the same state
    a, b = egg.SimulationHandler(), egg.SimulationHandler()
    for x in (a, b):
        x.set_solver_order("relaxed")
        for cx, cy in centers:
            x.add(cx, cy, 50, 15)
    a.set_forces(list(FORCES))
    a.set_forces([])
    for _ in range(3):
        counts = []
        for x in (a, b):
            before = x.stats()["kernel_launches"]
            assert x.update(1 / 60, 1 / 60, 2, 3) == 1
            counts.append(x.stats()["kernel_launches"] - before)
        assert counts[0] == counts[1]
    for w in (WHITE, YOLK):
        for f in FIELDS:
            assert np.array_equal(a.download(w, f), b.download(w, f)), (w, f)
    assert a.stats()["pair_solves"] == b.stats()["pair_solves"]
    for _ in range(2):
        before = never.stats()["kernel_launches"]
        assert never.update(1 / 60, 1 / 60, 2, 3) == 1
    assert never.stats()["kernel_launches"] - before == launches[-1]


def test_rules(egg):
    good = [("uniform", 0.0, 980.0), ("radial", 400.0, 300.0, -4000.0, 60.0, "white")]
    h, m = _handle(egg, forces=good), _model(forces=good)
    ids = [h.add(400.0, 300.0, 50, 15)]
    assert [m.add(400.0, 300.0, 50, 15)] == ids
    stored = h.get_forces()
    assert stored == [("uniform", 0.0, 980.0, "both"), ("radial", 400.0, 300.0, -4000.0, 60.0, "white")]
    lib, EF = egg._ffi.load(), egg._ffi.EggForce
    nan, inf = float("nan"), float("inf")
    bad_lists = [
        [("uniform", 0.0, 1.0)] * 17,                          # n outside 0 .. 16
        [good[0], ("uniform", nan, 0.0)],                      # a parameter that is not finite
        [good[0], ("uniform", 0.0, inf)],
        [good[0], ("radial", 0.0, -inf, 1.0, 1.0)],
        [good[0], ("vortex", 0.0, 0.0, nan, 1.0)],
        [good[0], ("radial", 0.0, 0.0, 1.0, inf)],
        [good[0], ("radial", 0.0, 0.0, 1.0, 0.0)],             # R <= 0
        [good[0], ("vortex", 0.0, 0.0, 1.0, -2.0)],
    ]
    for bad in bad_lists:
        with pytest.raises(egg.EggError, match="egg_set_forces: " + ("n = 17" if len(bad) == 17 else "field 1")):
            h.set_forces(bad)
        assert h.get_forces() == stored
    for kind, mask in ((3, 3), (-1, 3), (1, 0), (1, 4), (1, -1)):  # an unknown kind, a mask of 0 or with bits beyond 3
        arr = (EF * 2)()
        arr[0].kind, arr[0].type_mask, arr[0].p[3] = 1, 3, 1.0
        arr[1].kind, arr[1].type_mask, arr[1].p[3] = kind, mask, 1.0
        assert lib.egg_set_forces(h._h, 2, arr) == egg._ffi.EGG_ERR_INVALID_ARGUMENT
        assert b"field 1" in lib.egg_last_error(h._h)
        assert h.get_forces() == stored
    assert lib.egg_set_forces(h._h, -1, None) == egg._ffi.EGG_ERR_INVALID_ARGUMENT
    assert lib.egg_set_forces(h._h, 1, None) == egg._ffi.EGG_ERR_INVALID_ARGUMENT
    with pytest.raises(egg.EggError, match="clear the list first"):
        h.set_solver_order("exact")  # exact order with a list set
    assert h.get_solver_order() == "relaxed" and h.get_forces() == stored
    for _ in range(2):  # the list every refusal left alone is the one the steps use
        _step_both(h, m)
    _assert_snapshot(h, _snapshot(m, ids), "after the refusals")
    assert min(m.force_acts) == 0 < m.force_acts[WHITE]  # (the radial field is white-only)
    # a full list of 16 round-trips
    full = [("vortex", float(k), 2.0 * k, -1.5 * k, 1.0 + k, ("white", "yolk", "both")[k % 3]) for k in range(16)]
    h.set_forces(full)
    assert h.get_forces() == full
    # exact order: an empty list is accepted, a non-empty one is not
    e = egg.SimulationHandler()
    e.set_forces([])
    with pytest.raises(egg.EggError, match="relaxed order"):
        e.set_forces(good)
    assert e.get_forces() == []
    h.set_forces([])
    h.set_solver_order("exact")
    # while a step is in flight
    h.step_begin(1 / 60, 2, 3)
    with pytest.raises(egg.EggError, match="in flight"):
        h.set_forces([])
    h.step_end(True)
    # the group: the same rules, and a refused list changes no handle
    g = egg.SimulationGroup([0, 0], cuts=[-INF, 0.0, INF])
    g.set_forces([])
    with pytest.raises(egg.EggError, match="relaxed order"):
        g.set_forces(good)
    g.set_solver_order("relaxed")
    g.set_forces(good)
    for bad in bad_lists:
        with pytest.raises(egg.EggError):
            g.set_forces(bad)
    assert g.get_forces() == stored and all(b.get_forces() == stored for b in g.handles)
    with pytest.raises(egg.EggError, match="clear the list first"):
        g.set_solver_order("exact")
    assert g.get_solver_order() == "relaxed"
    g.set_forces([])
    g.set_solver_order("exact")


def test_a_thrown_particle_fails_the_step_and_commits_nothing(egg):
    """an acceleration that throws the particles beyond cell +-2^30 fails the step through the bad-cell flag"""
    h, m = _handle(egg), _model()
    ids = [h.add(300.0, 300.0, 50, 15)]
    assert [m.add(300.0, 300.0, 50, 15)] == ids
    _step_both(h, m)
    h.set_forces([("uniform", 1.0e18, 0.0)])
    with pytest.raises(egg.EggError, match="relaxed order"):
        h.step(1 / 60, 2, 3)
    assert h.stats()["steps"] == 1
    h.set_forces([])
    _step_both(h, m)
    _assert_snapshot(h, _snapshot(m, ids), "after the failed step")


# ------------------------------------------------------------------------------------------------ sharded
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
        for cfg, cohesion in EVERYTHING:
            sh = ShardedSimulationHandler(SlabLayout(SHARDED_CUTS), rank, dist, lambda: SimulationHandler(device=0), device="cpu")
            sh.set_solver_order("relaxed")
            if CONFIGS[cfg]:
                sh.set_white_config(CONFIGS[cfg])
            if cohesion:
                sh.set_cohesion("effective")
            sh.set_colliders(list(SCENE))
            sh.set_forces(list(FORCES))
            centers = _centers()
            gids = [sh.add(x, y, 50, 15) for x, y in centers]
            for k in range(max(SNAPSHOTS)):
                for gid, c in zip(gids, centers):
                    sh.set_target_position(gid, *circle_target(c, k))
                sh.step(1 / 60, 2, 3)
                if k + 1 in SNAPSHOTS:
                    st = sh.local.stats()
                    out[(cfg, k + 1)] = dict(state=_state(sh), pos=sh.positions(), pairs=st["pair_solves"], cohered=st["cohesion_solves"],
                                             hits=sh.collider_hits(), n_forces=len(sh.get_forces()),
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
    """two ranks on one GPU, the cut through the cluster, the colliders and the fields; cohesion off, then on: the fields
    gathered from both ranks are the model's after steps 1, 8 and 20"""
    res = _spawn(2)
    for cfg, cohesion in EVERYTHING:
        ref = _check_reference(cfg, cohesion)
        for step in SNAPSHOTS:
            snap, got = ref[step], [res[r][(cfg, step)] for r in (0, 1)]
            ids = sorted(snap["pos"])
            for w in (WHITE, YOLK):
                n = snap["state"][w].shape[1] // len(ids)
                seen = []
                for r in (0, 1):
                    for gid, cols in got[r]["state"][w].items():
                        seen.append(gid)
                        for k, f in enumerate(FIELDS):
                            want = snap["state"][w][k][(gid - 1) * n:gid * n]
                            assert np.array_equal(np.array(cols[k]), want), "%s step %d type %d field %s batch %d" % (cfg, step, w, f, gid)
                assert sorted(seen) == ids
                envs = [got[r]["env"][w] for r in (0, 1) if got[r]["env"][w] is not None]
                assert len(envs) == 1
                for key in ENV_KEYS:
                    assert envs[0][key] == snap["env"][w][key], "%s step %d type %d env %s" % (cfg, step, w, key)
            for r in (0, 1):
                assert {g: tuple(p) for g, p in got[r]["pos"].items()} == snap["pos"]
                assert got[r]["hits"] == snap["hits"] and got[r]["n_forces"] == len(FORCES)
                assert got[r]["halo"]["records"] > 0
            assert sum(got[r]["pairs"] for r in (0, 1)) == snap["pairs"]
            assert sum(got[r]["cohered"] for r in (0, 1)) == snap["cohered"]
