"""Effective cohesion (EGG_OPT_COHESION = 1; DESIGN.md section 2.7, "Cohesion") on the device against the CPU model
tests/cohesion_model.py, bit for bit: on one handle, on a device group (several handles on GPU 0: the ghosts' batch
tags) and on a ShardedSimulationHandler (ranks are spawned processes on GPU 0 over gloo, as in
test_gpu_sharded_relaxed.py: the tag in the upper half of a record's key word)."""
import functools
import math

import numpy as np
import pytest

from cohesion_model import CohesiveModel
from conftest import ROOT, circle_target, load_golden
from relaxed_model import RelaxedModel, rm

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
FIELDS = ("x", "y", "vx", "vy", "last_x", "last_y")
ENV_KEYS = ("min_x", "min_y", "max_x", "max_y", "centroid_x", "centroid_y", "max_radius", "max_velocity",
            "last_centroid_x", "last_centroid_y")
INF = math.inf
# "default": white's band (md, reach] is empty (both factors 2), yolk's is 16 .. 24 px; "white3": white's is too
CONFIGS = {"default": {}, "white3": dict(cohesion_interaction_distance_factor=3, cohesion_strength=0.99)}


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _model(cfg="default", cohesion=True):
    w, y = rm.default_configs()
    return CohesiveModel(dict(w, **CONFIGS[cfg]), y, cohesion=cohesion)


def _handle(egg, cfg="default", cohesion=True):
    h = egg.SimulationHandler()
    h.set_solver_order("relaxed")
    if CONFIGS[cfg]:
        h.set_white_config(CONFIGS[cfg])
    if cohesion:
        h.set_cohesion("effective")
    return h


def _pair(egg, cfg="default"):
    return _handle(egg, cfg), _model(cfg)


def _centers():
    return [tuple(float(v) for v in c) for c in load_golden("four_batches")["centers"]]


def _snapshot(m, ids):
    return dict(state=[m.state(w) for w in (WHITE, YOLK)],
                env=[dict(m._last_white_env if w == WHITE else m._last_yolk_env) for w in (WHITE, YOLK)],
                pos={int(i): tuple(m.get_position(int(i))) for i in ids}, pairs=m.pair_solves,
                visits=[max(m.relaxed_pass_pairs[w::2]) for w in (WHITE, YOLK)], cohered=m.cohesion_solves)


@functools.lru_cache(maxsize=None)
def _model_run(cfg, S, C, steps=(1, 8, 20)):
    """four_batches with moving targets on the model, once per (config, S, C): snapshots after `steps`, shared by the
    tests that need them and never changed"""
    m, centers = _model(cfg), _centers()
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
    print("%s: pair_solves %d, cohesion_solves %d" % (what, st["pair_solves"], st["cohesion_solves"]))
    assert st["pair_solves"] == snap["pairs"], what
    assert st["max_pass_visits"] == snap["visits"], what
    assert st["cohesion_solves"] == snap["cohered"], what


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


@pytest.mark.parametrize("S,C", [(2, 3), (3, 2), (1, 1)])
@pytest.mark.parametrize("cfg", ["default", "white3"])
def test_parity_with_model(egg, cfg, S, C):
    ref = _model_run(cfg, S, C)
    h, centers = _handle(egg, cfg), _centers()
    ids = [h.add(cx, cy, 50, 15) for cx, cy in centers]
    for k in range(20):
        for i, c in zip(ids, centers):
            h.set_target_position(i, *circle_target(c, k))
        assert h.update(1 / 60, 1 / 60, S, C) == 1
        if k + 1 in (1, 20):
            _assert_snapshot(h, ref[k + 1], "%s S=%d C=%d step %d" % (cfg, S, C, k + 1))
    assert h.stats()["cohesion_solves"] > 0


def test_smallest_shapes(egg):
    """two particles per type and batch, some 20 px apart (inside both bands); then two such batches 12 px apart: cross-batch
    pairs come into the band as candidates and must not cohere.  That they do come is shown by a model that cannot tell
    the batches apart (every BATCH_ID made equal): it counts more cohesion pairs than the true one, which the device equals."""
    for second in (None, (307.0, 296.0)):
        h, m = _pair(egg, "white3")
        blind = _model("white3")
        spots = [(295.0, 296.0)] + ([second] if second else [])
        ids = [h.add(x, y, 28, 28, None, None, 2, 2) for x, y in spots]
        assert [m.add(x, y, 28, 28, 2, 2) for x, y in spots] == ids == [blind.add(x, y, 28, 28, 2, 2) for x, y in spots]
        for data in (blind._white_data, blind._yolk_data):
            for p in range(1, 2 * len(spots) + 1):
                data[rm.offset(p) + rm.BATCH_ID] = 1
        for k in range(6):
            _step_both(h, m, ids, spots, k, moving=False)
            blind.update(1 / 60, 1 / 60, 2, 3)
            _assert_same(h, m, ids, "%d tiny batches, step %d" % (len(spots), k + 1))
        assert m.cohesion_solves > 0
        assert (blind.cohesion_solves > m.cohesion_solves) == (second is not None)


def test_coincident_batches(egg):
    h, m = _pair(egg, "white3")
    centers = [(300.0, 300.0)] * 4 + [(700.0, 300.0)]
    ids = [h.add(cx, cy, 50, 15) for cx, cy in centers]
    assert [m.add(cx, cy, 50, 15) for cx, cy in centers] == ids
    for k in range(10):
        _step_both(h, m, ids, centers, k, moving=False)
    _assert_same(h, m, ids, "coincident")
    assert m.cohesion_solves > 0


def test_toggling(egg):
    h, m = _pair(egg, "white3")
    centers = _centers()
    ids = [h.add(cx, cy, 50, 15) for cx, cy in centers]
    assert [m.add(cx, cy, 50, 15) for cx, cy in centers] == ids
    k, counts = 0, []
    for mode in ("effective", "reference", "effective"):
        h.set_cohesion(mode)
        assert h.get_cohesion() == mode
        m.cohesion = mode == "effective"
        for _ in range(5):
            _step_both(h, m, ids, centers, k)
            k += 1
        _assert_same(h, m, ids, "after 5 steps in %s" % mode)
        counts.append(m.cohesion_solves)
    assert 0 < counts[0] == counts[1] < counts[2]


def test_mutations(egg):
    h, m = _pair(egg, "white3")
    centers = _centers()
    ids = [h.add(cx, cy, 50, 15) for cx, cy in centers]
    assert [m.add(cx, cy, 50, 15) for cx, cy in centers] == ids
    for k in range(3):
        _step_both(h, m, ids, centers, k)
    h.remove(ids[1])  # a middle batch: the atom indices behind it shift
    m.remove(ids[1])
    centers, ids = [centers[0]] + centers[2:], [ids[0]] + ids[2:]
    for k in range(3, 6):
        _step_both(h, m, ids, centers, k)
    _assert_same(h, m, ids, "after remove")
    i_new = h.add(60.0, -30.0, 40, 12)
    assert m.add(60.0, -30.0, 40, 12) == i_new
    centers, ids = centers + [(60.0, -30.0)], ids + [i_new]
    for k in range(6, 9):
        _step_both(h, m, ids, centers, k)
    _assert_same(h, m, ids, "after add")
    change = dict(cohesion_strength=0.9, cohesion_interaction_distance_factor=2.5)
    h.set_white_config(change)
    m._white_config.update(change)
    h.set_yolk_config(dict(cohesion_strength=0.5, cohesion_interaction_distance_factor=2.25))
    m._yolk_config.update(cohesion_strength=0.5, cohesion_interaction_distance_factor=2.25)
    before = m.cohesion_solves
    for k in range(9, 12):
        _step_both(h, m, ids, centers, k)
    _assert_same(h, m, ids, "after the live config change")
    assert m.cohesion_solves > before


def test_refusals(egg):
    opt = egg._ffi.OPT_COHESION
    h = egg.SimulationHandler()
    h.add(400, 300, 50, 15)
    assert (h.get_cohesion(), h.get_solver_order()) == ("reference", "exact")
    with pytest.raises(egg.EggError, match="relaxed order"):
        h.set_cohesion("effective")  # exact order
    assert (h.get_cohesion(), h.get_solver_order()) == ("reference", "exact")
    h.set_cohesion("reference")  # (what it is already: fine in any order)
    h.set_solver_order("relaxed")
    for bad in (2, -1, 0.5, float("nan"), float("inf")):
        with pytest.raises(egg.EggError):
            h.set_option(opt, bad)
    for bad in ("on", 1, None):
        with pytest.raises(egg.EggError):
            h.set_cohesion(bad)
    assert h.get_cohesion() == "reference"
    h.step(1 / 60, 2, 3)
    assert h.stats()["cohesion_solves"] == 0
    h.set_cohesion("effective")
    with pytest.raises(egg.EggError, match="cohesion off first"):
        h.set_solver_order("exact")
    assert (h.get_cohesion(), h.get_solver_order()) == ("effective", "relaxed")
    h.step(1 / 60, 2, 3)
    assert h.stats()["relaxed_steps"] == 2 and h.stats()["cohesion_solves"] > 0
    # while rx_begin is open
    h.rx_set_keys(WHITE, [1], [0], h.get_n_particles()[WHITE])
    h.rx_set_keys(YOLK, [1], [0], h.get_n_particles()[YOLK])
    h.rx_begin(1 / 60, 2, 3)
    with pytest.raises(egg.EggError, match="in flight"):
        h.set_cohesion("reference")
    with pytest.raises(egg.EggError, match="in flight"):
        h.set_solver_order("exact")
    h.rx_end(False)
    assert (h.get_cohesion(), h.get_solver_order()) == ("effective", "relaxed")
    h.set_cohesion("reference")
    h.set_solver_order("exact")
    h.step(1 / 60, 2, 3)
    # while step_begin is open (exact order)
    h.step_begin(1 / 60, 2, 3)
    with pytest.raises(egg.EggError, match="in flight"):
        h.set_option(opt, 0)
    h.step_end(True)
    assert (h.get_cohesion(), h.get_solver_order()) == ("reference", "exact")
    # the group: the same rules, and a refused value changes no handle
    g = egg.SimulationGroup([0, 0], cuts=[-INF, 0.0, INF])
    with pytest.raises(egg.EggError, match="relaxed order"):
        g.set_cohesion("effective")
    lib = egg._ffi.load()
    g.set_solver_order("relaxed")
    assert lib.egg_group_set_cohesion(g._g, 2) < 0 and lib.egg_group_set_cohesion(g._g, -1) < 0
    assert g.get_cohesion() == "reference"
    g.set_cohesion("effective")
    with pytest.raises(egg.EggError, match="cohesion off first"):
        g.set_solver_order("exact")
    assert (g.get_cohesion(), g.get_solver_order()) == ("effective", "relaxed")
    for b in g.handles:  # every handle is still relaxed and cohesive: switching to exact is refused on each
        with pytest.raises(egg.EggError, match="cohesion off first"):
            b.set_option(egg._ffi.OPT_SOLVER_ORDER, 0)


@pytest.mark.parametrize("S,C", [(2, 3), (1, 1)])
def test_launches_of_one_step(egg, S, C):
    """a cohesive pass still takes five launches: counted the way test_gpu_relaxed.test_launches_of_one_step counts"""
    h, centers = _handle(egg, "white3"), _centers()
    ids = [h.add(cx, cy, 50, 15) for cx, cy in centers]
    h.update(1 / 60, 1 / 60, S, C)
    before = h.stats()
    for i, c in zip(ids, centers):
        h.set_target_position(i, *circle_target(c, 1))
    h.update(1 / 60, 1 / 60, S, C)
    after = h.stats()
    assert all(n > 0 for n in h.get_n_particles()) and after["cohesion_solves"] > before["cohesion_solves"]
    assert after["kernel_launches"] - before["kernel_launches"] == 2 * (S + 5 * S * C + 1)


CUTS = {2: [-INF, 10.0, INF], 3: [-INF, -5.0, 25.0, INF]}  # through the four_batches cluster


@pytest.mark.parametrize("n_handles", [2, 3])
def test_device_group_equals_one_handle(egg, n_handles):
    """cuts through the cluster: every handle gathers over its own batches plus ghosts of the others', all in one
    another's bands.  A handle owns whole batches, so a ghost must never cohere with a local particle: its tag, unpacked
    from the upper half of its key word, is what keeps it from doing so (a lost tag would read 0, the first batch's)."""
    g = egg.SimulationGroup([0] * n_handles, cuts=CUTS[n_handles])
    g.set_solver_order("relaxed")
    g.set_white_config(CONFIGS["white3"])
    g.set_cohesion("effective")
    h, centers = _handle(egg, "white3"), _centers()
    ids = [g.add(x, y, 50, 15) for x, y in centers]
    assert [h.add(x, y, 50, 15) for x, y in centers] == ids
    assert len({g.owner(i)[0] for i in ids}) >= 2
    for k in range(20):
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
    assert sum(b.stats()["cohesion_solves"] for b in g.handles) == one["cohesion_solves"] > 0
    hc = g.halo_counters()
    assert hc["records"] > 0 and hc["bytes"] == 40 * hc["records"]
    # the single handle itself is the model's (step 20 of the shared run)
    _assert_snapshot(h, _model_run("white3", 2, 3)[20], "the one handle")


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
        results = []
        for mode in ("effective", "reference"):
            sh = ShardedSimulationHandler(SlabLayout(SHARDED_CUTS), rank, dist, lambda: SimulationHandler(device=0), device="cpu")
            sh.set_solver_order("relaxed")
            sh.set_white_config(CONFIGS["white3"])
            sh.set_cohesion(mode)
            centers = _centers()
            gids = [sh.add(x, y, 50, 15) for x, y in centers]
            for k in range(SHARDED_STEPS):
                for gid, c in zip(gids, centers):
                    sh.set_target_position(gid, *circle_target(c, k))
                sh.step(1 / 60, 2, 3)
            st = sh.local.stats()
            results.append(dict(state=_state(sh), pos=sh.positions(), pairs=st["pair_solves"], cohered=st["cohesion_solves"],
                                halo=sh.halo_counters(), owner=dict(sh.owner), mode=sh.get_cohesion()))
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


def test_sharded_two_ranks_match_the_model():
    """two ranks on one GPU, the cut through the cluster, white factor 3: with cohesion on the ranks' particles are the
    cohesive model's, with it off (the same ranks, a fresh scene) the relaxed model's -- today's result"""
    res = _spawn(2)
    on = _model_run("white3", 2, 3)[SHARDED_STEPS]
    m_off = _model("white3", cohesion=False)
    centers = _centers()
    ids = [m_off.add(cx, cy, 50, 15) for cx, cy in centers]
    for k in range(SHARDED_STEPS):
        for i, c in zip(ids, centers):
            m_off.set_target_position(i, *circle_target(c, k))
        m_off.update(1 / 60, 1 / 60, 2, 3)
    assert isinstance(m_off, RelaxedModel) and m_off.cohesion_solves == 0
    for i, (mode, snap) in enumerate((("effective", on), ("reference", _snapshot(m_off, ids)))):
        for w in (WHITE, YOLK):
            n = snap["state"][w].shape[1] // len(ids)
            seen = []
            for r in (0, 1):
                assert res[r][i]["mode"] == mode
                for gid, cols in res[r][i]["state"][w].items():
                    seen.append(gid)
                    for k, f in enumerate(FIELDS):
                        want = snap["state"][w][k][(gid - 1) * n:gid * n]
                        assert np.array_equal(np.array(cols[k]), want), "%s: type %d field %s batch %d" % (mode, w, f, gid)
            assert sorted(seen) == ids
        for r in (0, 1):
            assert {g: tuple(p) for g, p in res[r][i]["pos"].items()} == snap["pos"], mode
            halo = res[r][i]["halo"]
            assert halo["records"] > 0 and halo["bytes"] == 40 * halo["records"], mode
        assert sum(res[r][i]["pairs"] for r in (0, 1)) == snap["pairs"], mode
        assert sum(res[r][i]["cohered"] for r in (0, 1)) == snap["cohered"], mode
    assert on["cohered"] > 0
