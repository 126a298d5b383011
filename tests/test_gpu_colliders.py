"""Static colliders of the relaxed pass (egg_set_colliders; DESIGN.md section 2.7, "Colliders") on the device against the
CPU model tests/collider_model.py, bit for bit: on one handle (the four gather instantiations: cohesion off / on), on a
device group (several handles on GPU 0: projected particles in the halo) and on a ShardedSimulationHandler (ranks are
spawned processes on GPU 0 over gloo, as in test_gpu_cohesion.py)."""
import functools
import math

import numpy as np
import pytest

from collider_model import ColliderModel
from conftest import ROOT, circle_target, load_golden
from relaxed_model import DIRS, rm

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
FIELDS = ("x", "y", "vx", "vy", "last_x", "last_y")
ENV_KEYS = ("min_x", "min_y", "max_x", "max_y", "centroid_x", "centroid_y", "max_radius", "max_velocity",
            "last_centroid_x", "last_centroid_y")
INF = math.inf
CONFIGS = {"default": {}, "white3": dict(cohesion_interaction_distance_factor=3, cohesion_strength=0.99)}
# four_batches (centres (0, 0), (30, 10), (-20, 40), (200, 200), targets on circles of 100 px around them) inside a
# container of radius 150 px around (50, 60): it holds the fourth batch back from the first step on.  Then a half-plane
# under the cluster (y >= -10 + r; its normal is given unnormalised), a wall through the cluster and a white-only disc in
# its middle, in this order.  On the CPU model every one of the four moves particles of every type it covers, and every
# batch is moved by some collider in the first step already (test_parity_with_model asserts hits > 0 per type).  The
# container, the wall and the disc lie across every cut of the group and sharded tests below.
SCENE = (("container", 50.0, 60.0, 150.0), ("half_plane", 0.0, 3.0, -30.0), ("segment", -40.0, 50.0, 120.0, 50.0),
         ("disc", 10.0, 20.0, 15.0, "white"))


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _model(cfg="default", cohesion=False, colliders=()):
    w, y = rm.default_configs()
    m = ColliderModel(dict(w, **CONFIGS[cfg]), y, cohesion=cohesion)
    m.set_colliders(colliders)
    return m


def _handle(egg, cfg="default", cohesion=False, colliders=()):
    h = egg.SimulationHandler()
    h.set_solver_order("relaxed")
    if CONFIGS[cfg]:
        h.set_white_config(CONFIGS[cfg])
    if cohesion:
        h.set_cohesion("effective")
    h.set_colliders(list(colliders))
    return h


def _centers():
    return [tuple(float(v) for v in c) for c in load_golden("four_batches")["centers"]]


def _snapshot(m, ids):
    return dict(state=[m.state(w) for w in (WHITE, YOLK)],
                env=[dict(m._last_white_env if w == WHITE else m._last_yolk_env) for w in (WHITE, YOLK)],
                pos={int(i): tuple(m.get_position(int(i))) for i in ids}, pairs=m.pair_solves,
                visits=[max(m.relaxed_pass_pairs[w::2]) for w in (WHITE, YOLK)], cohered=m.cohesion_solves,
                hits=list(m.collider_hits))


@functools.lru_cache(maxsize=None)
def _model_run(cfg, cohesion, S, C, steps=(1, 8, 20)):
    """four_batches with moving targets among SCENE on the model, once per (config, cohesion, S, C): snapshots after
    `steps`, shared by the tests that need them and never changed"""
    m, centers = _model(cfg, cohesion, SCENE), _centers()
    ids = [m.add(cx, cy, 50, 15) for cx, cy in centers]
    out = {}
    for k in range(max(steps)):
        for i, c in zip(ids, centers):
            m.set_target_position(i, *circle_target(c, k))
        m.update(1 / 60, 1 / 60, S, C)
        if k + 1 in steps:
            out[k + 1] = _snapshot(m, ids)
    return out


def _assert_snapshot(h, snap, what):
    for w in (WHITE, YOLK):
        for k, f in enumerate(FIELDS):
            assert np.array_equal(h.download(w, f), snap["state"][w][k]), "%s type %d field %s" % (what, w, f)
        env = h.get_environment(w)
        for key in ENV_KEYS:
            assert env[key] == snap["env"][w][key], "%s type %d env %s" % (what, w, key)
    for i, p in snap["pos"].items():
        assert h.get_position(i) == p, "%s position %d" % (what, i)
    st = h.stats()
    print("%s: pair_solves %d, cohesion_solves %d, hits %s" % (what, st["pair_solves"], st["cohesion_solves"], h.collider_hits()))
    assert st["pair_solves"] == snap["pairs"], what
    assert st["max_pass_visits"] == snap["visits"], what
    assert st["cohesion_solves"] == snap["cohered"], what
    assert h.collider_hits() == snap["hits"], what


def _assert_same(h, m, ids, what):
    _assert_snapshot(h, _snapshot(m, ids), what)


def _step_both(h, m, ids, centers, k, S=2, C=3, moving=True):
    if moving:
        for i, c in zip(ids, centers):
            t = circle_target(c, k)
            h.set_target_position(i, *t)
            m.set_target_position(i, *t)
    assert h.update(1 / 60, 1 / 60, S, C) == 1
    m.update(1 / 60, 1 / 60, S, C)


# the batch is added at (295, 296) and sent to a target 40 px beyond the collider's edge at x = 315
SMALL = {
    "half_plane": (("half_plane", -1.0, 0.0, -315.0), (355.0, 296.0)),
    "disc": (("disc", 365.0, 296.0, 50.0), (355.0, 296.0)),
    "container": (("container", 295.0, 296.0, 20.0), (355.0, 296.0)),
    "segment": (("segment", 315.0, 250.0, 315.0, 340.0), (355.0, 296.0)),
}


@pytest.mark.parametrize("n_batches", [1, 2])
@pytest.mark.parametrize("kind", sorted(SMALL))
def test_smallest_shapes(egg, kind, n_batches):
    collider, target = SMALL[kind]
    h, m = _handle(egg, colliders=[collider]), _model(colliders=[collider])
    spots = [(295.0, 296.0), (307.0, 296.0)][:n_batches]
    ids = [h.add(x, y, 28, 28, None, None, 2, 2) for x, y in spots]
    assert [m.add(x, y, 28, 28, 2, 2) for x, y in spots] == ids
    for i in ids:
        h.set_target_position(i, *target)
        m.set_target_position(i, *target)
    for k in range(6):
        _step_both(h, m, ids, spots, k, moving=False)
        _assert_same(h, m, ids, "%s, %d tiny batches, step %d" % (kind, n_batches, k + 1))
    assert min(m.collider_hits) > 0
    got = h.get_colliders()
    assert len(got) == 1 and got[0][0] == kind and got[0][-1] == "both"
    assert got[0][1:-1] == tuple(m.colliders[0][1:1 + len(got[0]) - 2])  # (a half-plane's normal comes back normalised)


def test_a_particle_on_a_discs_centre(egg):
    """white particle 1 and yolk particle 0 rest exactly on their batch's target with the other particle of the type far
    away: nothing moves them before step 5b of the first pass, where a disc centred on the target sends them out along
    DIRS[key & 7].  (add does not put a particle there: the state goes in through egg_import_batch.)"""
    src = egg.SimulationHandler()
    i = src.add(300.0, 300.0, 28, 28, None, None, 2, 2)
    info, ws, ys = src.export_batch(i)
    m = _model(colliders=[("disc", 300.0, 300.0, 5.0)])
    assert m.add(300.0, 300.0, 28, 28, 2, 2) == i
    for state, data, on in ((ws, m._white_data, 1), (ys, m._yolk_data, 0)):
        for p in (0, 1):
            x, y = (300.0, 300.0) if p == on else (300.0 + 90.0 * (p + 1), 250.0)
            state[0, p] = state[4, p] = x
            state[1, p] = state[5, p] = y
            state[2, p] = state[3, p] = 0.0
            for off, v in ((rm.X, x), (rm.Y, y), (rm.LAST_X, x), (rm.LAST_Y, y), (rm.VX, 0.0), (rm.VY, 0.0)):
                data[rm.offset(p + 1) + off] = v
    h = _handle(egg, colliders=[("disc", 300.0, 300.0, 5.0)])
    assert h.import_batch(info, ws, ys) == i
    assert h.update(1 / 60, 1 / 60, 1, 1) == 1
    m.update(1 / 60, 1 / 60, 1, 1)
    _assert_same(h, m, [i], "on the centre, first step")
    for w, on in ((WHITE, 1), (YOLK, 0)):
        r = h.download(w, "radius")[on]
        assert (h.download(w, "x")[on], h.download(w, "y")[on]) == (300.0 + DIRS[on, 0] * (5.0 + r), 300.0 + DIRS[on, 1] * (5.0 + r))
    assert m.collider_hits == [1, 1]
    for k in range(3):
        _step_both(h, m, [i], None, k, moving=False)
    _assert_same(h, m, [i], "on the centre, later")


@pytest.mark.parametrize("S,C", [(2, 3), (3, 2), (1, 1)])
@pytest.mark.parametrize("cfg,cohesion", [("default", False), ("white3", True)])
def test_parity_with_model(egg, cfg, cohesion, S, C):
    ref = _model_run(cfg, cohesion, S, C)
    assert min(ref[1]["hits"]) > 0, "the container of radius 150 px does not bind on the model"
    assert (ref[20]["cohered"] > 0) == cohesion
    h, centers = _handle(egg, cfg, cohesion, SCENE), _centers()
    ids = [h.add(cx, cy, 50, 15) for cx, cy in centers]
    for k in range(20):
        for i, c in zip(ids, centers):
            h.set_target_position(i, *circle_target(c, k))
        assert h.update(1 / 60, 1 / 60, S, C) == 1
        if k + 1 in (1, 20):
            _assert_snapshot(h, ref[k + 1], "%s S=%d C=%d step %d" % (cfg, S, C, k + 1))


def test_toggling(egg):
    h, m, never = _handle(egg), _model(), _handle(egg)
    centers = _centers()
    ids = [h.add(cx, cy, 50, 15) for cx, cy in centers]
    assert [m.add(cx, cy, 50, 15) for cx, cy in centers] == ids == [never.add(cx, cy, 50, 15) for cx, cy in centers]
    k, hits, launches = 0, [], []
    other = (("half_plane", 1.0, 1.0, -40.0, "yolk"), ("disc", 0.0, 0.0, 30.0))
    for colliders in (SCENE, (), other):
        h.set_colliders(list(colliders))
        m.set_colliders(colliders)
        assert len(h.get_colliders()) == len(colliders)
        for _ in range(3):
            before = h.stats()["kernel_launches"]
            _step_both(h, m, ids, centers, k)
            launches.append(h.stats()["kernel_launches"] - before)
            k += 1
            _assert_same(h, m, ids, "step %d with %d colliders" % (k, len(colliders)))
        hits.append(sum(m.collider_hits))
    assert 0 < hits[0] == hits[1] < hits[2]
    # with colliders a pass still takes five launches, and after the clear a step launches what a handle launches that
    # never had any (counted the way test_gpu_relaxed.test_launches_of_one_step counts; a handle's first step builds its
    # per-particle atoms besides)
    for j in range(2):
        before = never.stats()["kernel_launches"]
        for i, c in zip(ids, centers):
            never.set_target_position(i, *circle_target(c, j))
        assert never.update(1 / 60, 1 / 60, 2, 3) == 1
    plain = never.stats()["kernel_launches"] - before
    assert launches[1:] == [plain] * 8 == [2 * (2 + 5 * 2 * 3 + 1)] * 8


def test_refusals(egg):
    good = [("container", 400.0, 300.0, 12.0), ("half_plane", 0.0, -4.0, -330.0, "white")]
    h, m = _handle(egg, colliders=good), _model(colliders=good)
    ids = [h.add(400.0, 300.0, 50, 15)]
    assert [m.add(400.0, 300.0, 50, 15)] == ids
    stored = h.get_colliders()
    assert stored == [("container", 400.0, 300.0, 12.0, "both"), ("half_plane", 0.0, -1.0, -330.0, "white")]
    lib, C, EC = egg._ffi.load(), egg._ffi.C, egg._ffi.EggCollider
    nan, inf = float("nan"), float("inf")
    bad_lists = [
        [("disc", 0.0, 0.0, 1.0)] * 65,                       # n outside 0 .. 64
        [good[0], ("disc", nan, 0.0, 1.0)],                   # a parameter that is not finite
        [good[0], ("disc", 0.0, 0.0, inf)],
        [good[0], ("segment", 0.0, 0.0, 1.0, -inf)],
        [good[0], ("half_plane", 1.0, 0.0, nan)],
        [good[0], ("disc", 0.0, 0.0, -1.0)],                  # R < 0
        [good[0], ("container", 0.0, 0.0, -0.5)],
        [good[0], ("half_plane", 0.0, 0.0, 1.0)],             # a normal shorter than eps
        [good[0], ("half_plane", 1e-9, 0.0, 1.0)],
    ]
    k = 0
    for bad in bad_lists:
        with pytest.raises(egg.EggError, match="egg_set_colliders: " + ("n = 65" if len(bad) == 65 else "collider 1")):
            h.set_colliders(bad)
        assert h.get_colliders() == stored
    for kind, mask in ((4, 3), (-1, 3), (1, 0), (1, 4), (1, -1)):  # an unknown kind, a mask of 0 or with bits beyond 3
        arr = (EC * 2)()
        arr[0].kind, arr[0].type_mask, arr[0].p[2] = 1, 3, 1.0
        arr[1].kind, arr[1].type_mask, arr[1].p[2] = kind, mask, 1.0
        assert lib.egg_set_colliders(h._h, 2, arr) == egg._ffi.EGG_ERR_INVALID_ARGUMENT
        assert b"collider 1" in lib.egg_last_error(h._h)
        assert h.get_colliders() == stored
    assert lib.egg_set_colliders(h._h, -1, None) == egg._ffi.EGG_ERR_INVALID_ARGUMENT
    assert lib.egg_set_colliders(h._h, 1, None) == egg._ffi.EGG_ERR_INVALID_ARGUMENT
    with pytest.raises(egg.EggError, match="clear the list first"):
        h.set_solver_order("exact")  # exact order with a list set
    assert h.get_solver_order() == "relaxed" and h.get_colliders() == stored
    for _ in range(2):  # the list every refusal left alone is the one the steps use
        _step_both(h, m, ids, None, k, moving=False)
    _assert_same(h, m, ids, "after the refusals")
    assert min(m.collider_hits) > 0
    # exact order: an empty list is accepted, a non-empty one is not
    e = egg.SimulationHandler()
    e.set_colliders([])
    with pytest.raises(egg.EggError, match="relaxed order"):
        e.set_colliders(good)
    assert e.get_colliders() == [] and e.collider_hits() == [0, 0]
    h.set_colliders([])
    h.set_solver_order("exact")
    # while a step is in flight
    h.step_begin(1 / 60, 2, 3)
    with pytest.raises(egg.EggError, match="in flight"):
        h.set_colliders([])
    h.step_end(True)
    # the group: the same rules, and a refused list changes no handle
    g = egg.SimulationGroup([0, 0], cuts=[-INF, 0.0, INF])
    g.set_colliders([])
    with pytest.raises(egg.EggError, match="relaxed order"):
        g.set_colliders(good)
    g.set_solver_order("relaxed")
    g.set_colliders(good)
    for bad in bad_lists:
        with pytest.raises(egg.EggError):
            g.set_colliders(bad)
    assert g.get_colliders() == stored and all(b.get_colliders() == stored for b in g.handles)
    with pytest.raises(egg.EggError, match="clear the list first"):
        g.set_solver_order("exact")
    assert g.get_solver_order() == "relaxed"
    g.set_colliders([])
    g.set_solver_order("exact")


def test_a_failed_step_adds_no_hits(egg):
    wall = [("half_plane", -1.0, 0.0, -310.0)]
    h, m = _handle(egg, colliders=wall), _model(colliders=wall)
    ids = [h.add(300.0, 300.0, 50, 15)]
    assert [m.add(300.0, 300.0, 50, 15)] == ids
    _step_both(h, m, ids, None, 0, moving=False)
    assert h.collider_hits() == m.collider_hits and min(m.collider_hits) > 0
    far = h.add(1.0e12, 0.0, 50, 15)  # its cells lie beyond +-2^30: the step fails, after its passes have projected
    with pytest.raises(egg.EggError, match="relaxed order"):
        h.step(1 / 60, 2, 3)
    assert h.collider_hits() == m.collider_hits and h.stats()["steps"] == 1
    h.remove(far)
    _step_both(h, m, ids, None, 1, moving=False)
    for w in (WHITE, YOLK):
        for k, f in enumerate(FIELDS):
            assert np.array_equal(h.download(w, f), m.state(w)[k]), (w, f)
    assert h.collider_hits() == m.collider_hits


CUTS = {2: [-INF, 10.0, INF], 3: [-INF, -5.0, 25.0, INF]}  # through the four_batches cluster, the wall and the container


@pytest.mark.parametrize("n_handles", [2, 3])
def test_device_group_equals_one_handle(egg, n_handles):
    """cuts through the cluster: the wall and the container of SCENE lie across them, so particles a device has projected
    are ghosts of its neighbours in the next pass.  Cohesion on: the group-cohesive instantiation; the plain group one
    runs in the 2-handle case besides."""
    for cfg, cohesion, steps in (("white3", True, 20),) + ((("default", False, 8),) if n_handles == 2 else ()):
        g = egg.SimulationGroup([0] * n_handles, cuts=CUTS[n_handles])
        g.set_solver_order("relaxed")
        if CONFIGS[cfg]:
            g.set_white_config(CONFIGS[cfg])
        if cohesion:
            g.set_cohesion("effective")
        g.set_colliders(list(SCENE))
        h, centers = _handle(egg, cfg, cohesion, SCENE), _centers()
        assert g.get_colliders() == h.get_colliders() and len(h.get_colliders()) == len(SCENE)
        ids = [g.add(x, y, 50, 15) for x, y in centers]
        assert [h.add(x, y, 50, 15) for x, y in centers] == ids
        assert len({g.owner(i)[0] for i in ids}) >= 2
        for k in range(steps):
            for i, c in zip(ids, centers):
                t = circle_target(c, k)
                g.set_target_position(i, *t)
                h.set_target_position(i, *t)
            g.step(1 / 60, 2, 3)
            h.step(1 / 60, 2, 3)
        for w in (WHITE, YOLK):
            got = g.particles(w, FIELDS)
            cat = np.concatenate([np.array(got[i]) for i in sorted(got)], axis=1)
            for k, f in enumerate(FIELDS):
                assert np.array_equal(cat[k], h.download(w, f)), "type %d field %s" % (w, f)
        for i in ids:
            assert g.get_position(i) == h.get_position(i)
        one = h.stats()
        assert sum(b.stats()["pair_solves"] for b in g.handles) == one["pair_solves"]
        assert sum(b.stats()["cohesion_solves"] for b in g.handles) == one["cohesion_solves"]
        assert g.collider_hits() == h.collider_hits()
        assert g.collider_hits() == [sum(b.collider_hits()[w] for b in g.handles) for w in (WHITE, YOLK)]
        assert sum(1 for b in g.handles if sum(b.collider_hits()) > 0) >= 2  # (more than one device projected)
        assert g.halo_counters()["records"] > 0
        # the single handle itself is the model's (a step of the shared run)
        _assert_snapshot(h, _model_run(cfg, cohesion, 2, 3)[steps], "the one handle")


# ------------------------------------------------------------------------------------------------ sharded
SHARDED_CUTS = [-2000.0, 10.0, 2000.0]
SHARDED_STEPS = 8


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
        sh = ShardedSimulationHandler(SlabLayout(SHARDED_CUTS), rank, dist, lambda: SimulationHandler(device=0), device="cpu")
        sh.set_solver_order("relaxed")
        sh.set_white_config(CONFIGS["white3"])
        sh.set_cohesion("effective")
        sh.set_colliders(list(SCENE))
        centers = _centers()
        gids = [sh.add(x, y, 50, 15) for x, y in centers]
        for k in range(SHARDED_STEPS):
            for gid, c in zip(gids, centers):
                sh.set_target_position(gid, *circle_target(c, k))
            sh.step(1 / 60, 2, 3)
        st = sh.local.stats()
        q.put((rank, "ok", dict(state=_state(sh), pos=sh.positions(), pairs=st["pair_solves"], cohered=st["cohesion_solves"],
                                hits=sh.collider_hits(), own_hits=sh.local.collider_hits(), n_colliders=len(sh.get_colliders()),
                                halo=sh.halo_counters())))
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
    """two ranks on one GPU, the cut through the cluster, the wall and the container; cohesion on: the fields gathered
    from both ranks are the model's, and so are the all-reduced hits"""
    res = _spawn(2)
    snap = _model_run("white3", True, 2, 3)[SHARDED_STEPS]
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
    for r in (0, 1):
        assert {g: tuple(p) for g, p in res[r]["pos"].items()} == snap["pos"]
        assert res[r]["hits"] == snap["hits"] and res[r]["n_colliders"] == len(SCENE)
        assert res[r]["halo"]["records"] > 0 and res[r]["halo"]["bytes"] == 40 * res[r]["halo"]["records"]
    assert [sum(res[r]["own_hits"][w] for r in (0, 1)) for w in (WHITE, YOLK)] == snap["hits"]
    assert all(sum(res[r]["own_hits"]) > 0 for r in (0, 1)) and min(snap["hits"]) > 0
    assert sum(res[r]["pairs"] for r in (0, 1)) == snap["pairs"]
    assert sum(res[r]["cohered"] for r in (0, 1)) == snap["cohered"] > 0
