"""Yolk containment of the relaxed step (egg_set_containment; DESIGN.md section 2.7, "Containment") on the device against
the CPU model tests/containment_model.py, bit for bit: x, y, vx, vy, last_x, last_y of every particle, the environments,
the batch positions, every counter of the family and containment_hits -- on one handle (egg_rx_contain_sum_kernel at the
wave tail, exactly one row and a second row; egg_rx_contain_kernel), on device groups of 2 and 3 handles on GPU 0 and on two
sharded ranks over gloo (egg_rx_contain_group_kernel and the widened box), where coupling and adhesion do not exist.

The model is containment on top of the adhesion band on top of the coupling pass on top of tests/wall_model.py's WallModel
(tests/test_containment_model.py's Hand), so that one class covers every scene below."""
import functools

import numpy as np
import pytest

import test_containment_model as cm
import test_gpu_adhesion as ga
from conftest import ROOT, circle_target
from relaxed_model import rm
from test_gpu_collider_walls import CONFIGS, CUTS, DROP, SCENES, THREE, _configure
from test_gpu_colliders import FIELDS, SHARDED_CUTS, _centers
from test_gpu_colliders import SCENE as FOUR_SCENE
from test_gpu_coupling import _same_bits
from test_gpu_forces import EVERYTHING as FORCES_EVERYTHING
from test_gpu_forces import FORCES

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
H60 = 1 / 60
ON, A3 = ga.ON, ga.A3
SNUG = (0.25, 0.5)  # a quarter of the white's RMS radius cuts through the yolk of a default egg (50 px white, 15 px yolk)
TIGHT = (0.75, 1.0)  # three quarters of the white's RMS radius: yolk particles lie beyond it in every sub-step


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _model(containment=None, coupling=None, adhesion=None, cfg="default", colliders=(), surfaces=None, forces=()):
    w, y = rm.default_configs()
    c = CONFIGS[cfg]
    m = cm.Hand(dict(w, **c["white"]), y, cohesion=c["cohesion"])
    m.set_viscosity(*c["viscosity"])
    m.set_colliders(colliders)
    m.set_forces(forces)
    if surfaces is not None:
        m.set_collider_surfaces(surfaces)
    if coupling is not None:
        m.set_coupling(*coupling)
    if adhesion is not None:
        m.set_adhesion(*adhesion)
    if containment is not None:
        m.set_containment(*containment)
    return m


def _handle(egg, containment=None, coupling=None, adhesion=None, cfg="default", colliders=(), surfaces=None, forces=()):
    h = _configure(egg.SimulationHandler(), cfg, colliders, surfaces, forces)
    if coupling is not None:
        h.set_coupling(*coupling)
    if adhesion is not None:
        h.set_adhesion(*adhesion)
    if containment is not None:
        h.set_containment(*containment)
    return h


def _snapshot(m, ids):
    return dict(ga._snapshot(m, ids), contained=m.containment_hits)


def _assert_snapshot(h, snap, what):
    ga._assert_snapshot(h, snap, what)
    print("%s: containment hits %d" % (what, h.containment_hits()))
    assert h.containment_hits() == snap["contained"], what


# ------------------------------------------------------------------------------------------------ 1: one handle, small
# (spot, white particles, yolk particles), radius 28 px for both types: the batches overlap.  White counts 63, 64 and 65
# reach the wave tail, exactly one row and a second row of the summary's lane loop; after the first step the middle batch
# goes and two more come (130: three rows; 2: one lane), so the atom index is not the batch id.
FIRST = (((295.0, 296.0), 63, 15), ((307.0, 296.0), 64, 2), ((301.0, 306.0), 65, 15))
LATER = (((289.0, 304.0), 130, 2), ((311.0, 288.0), 2, 15))
SMALL_STEPS = 3


def _small_script(obj, S, C, add, remove):
    """the scene on a model or a handle: yields the live ids after every step"""
    ids = [add(obj, x, y, nw, ny) for (x, y), nw, ny in FIRST]
    for k in range(SMALL_STEPS):
        if k == 1:
            remove(obj, ids[1])
            ids = [ids[0], ids[2]] + [add(obj, x, y, nw, ny) for (x, y), nw, ny in LATER]
        assert obj.update(H60, H60, S, C) == 1
        yield list(ids)


@functools.lru_cache(maxsize=None)
def _small_model_run(S, C, containment):
    """the snapshot after every step on the model, computed once and never changed"""
    m = _model(containment)
    out = [(ids, _snapshot(m, ids)) for ids in _small_script(m, S, C, lambda o, x, y, nw, ny: o.add(x, y, 28, 28, nw, ny),
                                                              lambda o, i: o.remove(i))]
    return out, dict(getattr(m, "containment_census", {}))


@pytest.mark.parametrize("strength", [1.0, 0.5])
@pytest.mark.parametrize("S,C", [(2, 3), (1, 1), (3, 2)])
def test_one_handle_against_the_model(egg, S, C, strength):
    ref, census = _small_model_run(S, C, (TIGHT[0], strength))
    plain, _ = _small_model_run(S, C, None) if (S, C, strength) == (2, 3, 1.0) else (None, None)
    # the case is worth relying on: particles are projected in every step, and some are left alone
    hits = [0] + [snap["contained"] for _, snap in ref]
    assert all(b > a for a, b in zip(hits, hits[1:])) and census["inside"] > 0
    assert census["hit_rigid" if strength == 1.0 else "hit_soft"] == hits[-1]
    if plain:
        assert not np.array_equal(ref[0][1]["state"][YOLK], plain[0][1]["state"][YOLK])
    h = _handle(egg, (TIGHT[0], strength))
    steps = _small_script(h, S, C, lambda o, x, y, nw, ny: o.add(x, y, 28, 28, None, None, nw, ny), lambda o, i: o.remove(i))
    for k, ids in enumerate(steps):
        assert ids == ref[k][0]
        _assert_snapshot(h, ref[k][1], "small, S=%d, C=%d, strength %s, step %d" % (S, C, strength, k + 1))
    assert h.containment() == (TIGHT[0], strength)


# ------------------------------------------------------------------------------------------------ 2: everything at once
@functools.lru_cache(maxsize=None)
def _everything_run(steps=8):
    # (test_gpu_adhesion's EVERYTHING, not test_gpu_forces': it is the superset -- that scene's cohesion, colliders, forces and
    # viscosity plus a wall, a surface, coupling and adhesion; test_gpu_forces' list picks the sharded scene's config below)
    m = _model(SNUG, ON, A3, **ga.EVERYTHING)
    i = m.add(300.0, 300.0, 50, 15)
    out = []
    for k in range(steps):
        if k == 2:  # before the third step the target jumps across the wall
            m.set_target_position(i, 300.0, 300.0 + DROP)
        m.update(H60, H60, 2, 3)
        out.append(dict(_snapshot(m, [i]), catches=list(m.wall_catches)))
    return i, out


def test_everything_on_at_once(egg):
    """effective cohesion, a container plus a wall with a surface, a uniform force, viscosity on both types, coupling,
    adhesion and containment, on one handle against the model"""
    i, ref = _everything_run()
    last = ref[-1]
    print("model: catches %s, hits %s, grips %s, viscosity pairs %s, cohered %d, coupling solves %d, adhesion solves %d, "
          "containment hits %d" % (last["catches"], last["hits"], last["grips"], last["visc"], last["cohered"], last["coupled"],
                                   last["adhered"], last["contained"]))
    assert min(last["catches"]) > 0 and min(last["hits"]) > 0 and min(last["grips"]) > 0 and min(last["visc"]) > 0
    assert last["cohered"] > 0 and last["coupled"] > 0 and last["adhered"] > 0 and last["contained"] > 0
    h = _handle(egg, SNUG, ON, A3, **ga.EVERYTHING)
    assert h.add(300.0, 300.0, 50, 15) == i
    for k, snap in enumerate(ref):
        if k == 2:
            h.set_target_position(i, 300.0, 300.0 + DROP)
        assert h.update(H60, H60, 2, 3) == 1
        _assert_snapshot(h, snap, "everything, step %d" % (k + 1))


# ------------------------------------------------------------------------------------------------ 3: off is off, launches
def _run_counting(h, S, C, steps=3):
    per_step = []
    for _ in range(steps):
        before = h.stats()["kernel_launches"]
        assert h.update(H60, H60, S, C) == 1
        per_step.append(h.stats()["kernel_launches"] - before)
    return per_step


@pytest.mark.parametrize("coupling", [None, ON])
def test_off_is_off_and_acting_adds_s_launches_per_type(egg, coupling):
    centers = ((300.0, 300.0), (330.0, 310.0))
    S, C = 2, 3

    def fresh(prepare):
        h = _handle(egg, None, coupling)
        for cx, cy in centers:
            h.add(cx, cy, 50, 15)
        prepare(h)
        return h

    never = fresh(lambda h: None)
    base = _run_counting(never, S, C)
    for prepare, what in ((lambda h: h.set_containment(0), "set_containment(0)"),
                          (lambda h: h.set_containment(0.0, 0.25), "factor 0 with a strength"),
                          (lambda h: (h.set_containment(*SNUG), h.set_containment()), "set and cleared")):
        other = fresh(prepare)
        assert _run_counting(other, S, C) == base, what
        _same_bits(never, other, what)
        assert other.containment_hits() == 0 and other.containment()[0] == 0.0
    on = fresh(lambda h: h.set_containment(*SNUG))
    assert _run_counting(on, S, C) == [n + 2 * S for n in base]  # one launch per sub-step and type
    assert on.containment_hits() > 0
    on.set_containment(0)
    assert _run_counting(on, S, C, 2) == base[1:]


def test_one_type_alone_cannot_arise(egg):
    """`factor > 0` acts on a handle that holds particles of both types.  A handle with one type populated and the other
    empty cannot be made through the public surface: add and import_batch refuse a batch without particles of a type.  This
    pins the refusals; the reachable form of the condition -- both types empty -- is the next test."""
    h = _handle(egg, TIGHT)
    with pytest.raises(egg.EggError, match="yolk particle count cannot be 1 or negative"):
        h.add(300.0, 300.0, 50, 15, None, None, 157, 0)
    with pytest.raises(egg.EggError, match="white particle count cannot be 1 or negative"):
        h.add(300.0, 300.0, 50, 15, None, None, 0, 15)
    import ctypes
    lib, one, out = egg._ffi.load(), ctypes.c_double(300.0), ctypes.c_int64()
    for nw, ny in ((157, 0), (0, 15)):  # (the library's own check, under the wrapper's)
        rc = lib.egg_add_many(h._h, 1, ctypes.addressof(one), ctypes.addressof(one), 50.0, 15.0, nw, ny, ctypes.addressof(out))
        assert rc == egg._ffi.EGG_ERR_INVALID_ARGUMENT and b"particle count cannot be 1 or negative" in lib.egg_last_error(h._h)
    src = egg.SimulationHandler()
    info, ws, ys = src.export_batch(src.add(300.0, 300.0, 50, 15))
    for key, cols in (("n_yolk", (ws, ys[:, :0])), ("n_white", (ws[:, :0], ys))):
        with pytest.raises(egg.EggError):
            h.import_batch(dict(info, **{key: 0}), *cols)
    assert sum(h.get_n_particles()) == 0
    assert h.import_batch(info, ws, ys) == 1  # ... and the whole batch is taken


@pytest.mark.parametrize("n_handles", [1, 2])
def test_a_handle_without_particles_launches_nothing_more(egg, n_handles):
    """both types empty with factor > 0: a handle that holds no batch -- alone, or the member of a device group whose slab is
    empty -- steps as it does without containment: the same launches, no hits; and beside it the populated member equals,
    bit for bit, a handle that holds the scene alone"""
    S, C = 2, 3
    centers = ((300.0, 300.0), (330.0, 310.0))
    if n_handles == 1:
        hs = [_handle(egg, c) for c in (None, SNUG)]
        launches = [_run_counting(h, S, C) for h in hs]
        assert launches[0] == launches[1]
        assert hs[1].containment_hits() == 0 and hs[1].containment() == SNUG and hs[1].stats()["steps"] == hs[0].stats()["steps"]
        return
    groups = []
    for containment in (None, SNUG):
        g = egg.SimulationGroup([0, 0], cuts=[-float("inf"), 1000.0, float("inf")])  # every batch on handle 0
        g.set_solver_order("relaxed")
        if containment:
            g.set_containment(*containment)
        ids = [g.add(x, y, 50, 15) for x, y in centers]
        assert {g.owner(i)[0] for i in ids} == {0}
        per_step = []
        for _ in range(3):
            before = [b.stats()["kernel_launches"] for b in g.handles]
            g.step(H60, S, C)
            per_step.append([b.stats()["kernel_launches"] - n for b, n in zip(g.handles, before)])
        groups.append((g, per_step))
    (off, base), (on, acting) = groups
    assert sum(on.handles[1].get_n_particles()) == 0
    assert [p[1] for p in acting] == [p[1] for p in base]            # the empty member: nothing more
    assert [p[0] for p in acting] == [p[0] + 2 * S for p in base]    # the populated one: one launch per sub-step and type
    assert on.handles[1].containment_hits() == 0 and on.containment_hits() == on.handles[0].containment_hits() > 0
    alone = _handle(egg, SNUG)
    for x, y in centers:
        alone.add(x, y, 50, 15)
    for _ in range(3):
        alone.step(H60, S, C)
    for w in (WHITE, YOLK):
        for f in FIELDS:
            assert np.array_equal(on.handles[0].download(w, f), alone.download(w, f)), (w, f)
    assert on.containment_hits() == alone.containment_hits()


# ------------------------------------------------------------------------------------------------ 4: device groups
GROUP_SCENE = SCENES["three_all"]  # (config, colliders, surfaces, forces, centers, steps): cohesion, viscosity, a wall, a surface, a force
GROUP_CONTAINMENT = (0.25, 0.5)  # (a default egg's yolk starts well inside its white: a quarter of the white's RMS radius cuts through it)


@functools.lru_cache(maxsize=None)
def _single_handle_run():
    """the group's scene on ONE handle, once: fields and counters after every step (the tests above hold one handle to the
    model)"""
    import egg_fluid_simulation_amd as egg
    cfg, colliders, surfaces, forces, centers, steps = GROUP_SCENE
    assert centers == THREE and steps == 10
    h = _configure(egg.SimulationHandler(), cfg, colliders, surfaces, forces)
    h.set_containment(*GROUP_CONTAINMENT)
    ids = [h.add(x, y, 50, 15) for x, y in centers]
    out = []
    for k in range(steps):
        for i, c in zip(ids, centers):
            h.set_target_position(i, *circle_target(c, k))
        h.step(H60, 2, 3)
        out.append(dict(state=[np.array([h.download(w, f) for f in FIELDS]) for w in (WHITE, YOLK)], contained=h.containment_hits(),
                        pairs=h.stats()["pair_solves"], hits=h.collider_hits(), visc=h.viscosity_pairs(),
                        pos={i: h.get_position(i) for i in ids}))
    return ids, out


@pytest.mark.parametrize("n_handles", [2, 3])
def test_device_group_equals_one_handle(egg, n_handles):
    """cuts through the cluster: every handle summarises and projects the batches it holds, nothing travels for it, and the
    box of a sub-step's first pass covers the projected positions"""
    ids, ref = _single_handle_run()
    assert all(b["contained"] > a["contained"] for a, b in zip([dict(contained=0)] + ref, ref))
    cfg, colliders, surfaces, forces, centers, steps = GROUP_SCENE
    g = _configure(egg.SimulationGroup([0] * n_handles, cuts=CUTS[n_handles]), cfg, colliders, surfaces, forces)
    g.set_containment(*GROUP_CONTAINMENT)
    assert g.containment() == GROUP_CONTAINMENT and all(b.containment() == GROUP_CONTAINMENT for b in g.handles)
    assert [g.add(x, y, 50, 15) for x, y in centers] == ids
    assert len({g.owner(i)[0] for i in ids}) >= 2
    for k in range(steps):
        for i, c in zip(ids, centers):
            g.set_target_position(i, *circle_target(c, k))
        g.step(H60, 2, 3)
        what = "%d handles, step %d" % (n_handles, k + 1)
        for w in (WHITE, YOLK):
            got = g.particles(w, FIELDS)
            cat = np.concatenate([np.array(got[i]) for i in sorted(got)], axis=1)
            for q, f in enumerate(FIELDS):
                assert np.array_equal(cat[q], ref[k]["state"][w][q]), "%s type %d field %s" % (what, w, f)
        print("%s: containment hits %d" % (what, g.containment_hits()))
        assert g.containment_hits() == ref[k]["contained"] == sum(b.containment_hits() for b in g.handles), what
        assert sum(b.stats()["pair_solves"] for b in g.handles) == ref[k]["pairs"], what
        assert g.collider_hits() == ref[k]["hits"] and g.viscosity_pairs() == ref[k]["visc"], what
        assert {i: g.get_position(i) for i in ids} == ref[k]["pos"], what
    assert g.halo_counters()["records"] > 0


def test_a_group_whose_handles_differ_refuses_to_step(egg):
    g = egg.SimulationGroup([0, 0], cuts=CUTS[2])
    g.set_solver_order("relaxed")
    g.set_containment(*SNUG)
    for x, y in THREE:
        g.add(x, y, 50, 15)
    g.step(H60, 2, 3)
    hits = g.containment_hits()
    assert hits > 0
    g.handles[1].set_containment(SNUG[0], 0.25)
    with pytest.raises(egg.EggError, match="differ in their containment"):
        g.step(H60, 2, 3)
    assert g.containment_hits() == hits
    g.set_containment(*SNUG)
    g.step(H60, 2, 3)
    assert g.containment_hits() > hits
    with pytest.raises(egg.EggError, match="exact order has no yolk containment"):
        g.set_solver_order("exact")
    with pytest.raises(egg.EggError, match="not a finite number"):
        g.set_containment(float("nan"), 1.0)
    assert g.containment() == SNUG


# ------------------------------------------------------------------------------------------------ 5: rules
def test_rules(egg):
    h = _handle(egg, (1.5, 0.25))
    h.add(400.0, 300.0, 50, 15)
    nan, inf = float("nan"), float("inf")
    lib = egg._ffi.load()
    for bad in ((nan, 1.0), (-0.5, 1.0), (inf, 1.0), (1.0, nan), (1.0, -0.1), (1.0, 1.5)):
        assert lib.egg_set_containment(h._h, *bad) == egg._ffi.EGG_ERR_INVALID_ARGUMENT  # (the library's own check)
        assert b"egg_set_containment" in lib.egg_last_error(h._h)
        with pytest.raises(egg.EggError, match="not a finite number|outside"):
            h.set_containment(*bad)
        assert h.containment() == (1.5, 0.25)
    with pytest.raises(egg.EggError, match="exact order has no yolk containment"):
        h.set_solver_order("exact")
    assert h.get_solver_order() == "relaxed" and h.containment() == (1.5, 0.25)
    assert h.update(H60, H60, 2, 3) == 1
    h.set_containment(0.0, 0.25)
    h.set_solver_order("exact")
    h.set_containment(0.0, 1.0)  # factor 0 is always accepted
    with pytest.raises(egg.EggError, match="relaxed order"):
        h.set_containment(*TIGHT)
    assert h.containment() == (0.0, 1.0)
    h.step_begin(H60, 2, 3)
    with pytest.raises(egg.EggError, match="in flight"):
        h.set_containment(0.0, 1.0)
    h.step_end(True)
    # ... and between egg_rx_begin and egg_rx_end, where it acts
    h.set_solver_order("relaxed")
    h.set_containment(*TIGHT)
    n = h.get_n_particles()
    for w in (WHITE, YOLK):
        h.rx_set_keys(w, [1], [0], n[w])
    h.rx_begin(H60, 1, 1)
    with pytest.raises(egg.EggError, match="in flight"):
        h.set_containment(0.0, 1.0)
    h.rx_end(False)
    assert h.containment() == TIGHT


def test_a_failed_step_adds_nothing_and_commits_nothing(egg):
    """a NaN position in the white gives a NaN centre: no comparison holds, the insert fails the step, nothing is committed
    or counted; the handle then goes on as the model says"""
    src = egg.SimulationHandler()
    src.add(300.0, 300.0, 50, 15)
    j = src.add(330.0, 310.0, 50, 15)
    info, ws, ys = src.export_batch(j)
    ws[0, 7] = float("nan")
    h, m = _handle(egg, SNUG), _model(SNUG)
    i = h.add(300.0, 300.0, 50, 15)
    assert m.add(300.0, 300.0, 50, 15) == i != j
    assert h.update(H60, H60, 2, 3) == 1
    m.update(H60, H60, 2, 3)
    hits = h.containment_hits()
    assert hits == m.containment_hits > 0
    before = [h.download(w, f) for w in (WHITE, YOLK) for f in ("x", "y")]
    assert h.import_batch(info, ws, ys) == j  # a second egg with one NaN position
    launches = h.stats()["kernel_launches"]
    with pytest.raises(egg.EggError, match="relaxed order: a position is NaN"):
        h.step(H60, 2, 3)
    assert h.stats()["steps"] == 1 and h.containment_hits() == hits
    assert h.stats()["kernel_launches"] > launches  # (the launches of a failed step are counted, as ever)
    n = [len(b) for b in before[::2]]
    for k, (w, f) in enumerate((w, f) for w in (WHITE, YOLK) for f in ("x", "y")):
        assert np.array_equal(h.download(w, f)[:n[k // 2]], before[k]), (w, f)
    h.remove(j)
    assert h.update(H60, H60, 2, 3) == 1
    m.update(H60, H60, 2, 3)
    _assert_snapshot(h, _snapshot(m, [i]), "after the failed step")


# ------------------------------------------------------------------------------------------------ 6: sharded
SHARDED_CFG, SHARDED_COHESION = FORCES_EVERYTHING[1]  # ("white3", effective cohesion), among FOUR_SCENE and FORCES
SHARDED_CONTAINMENT, SHARDED_STEPS = (0.25, 0.5), 3


def _sharded_configure(h):
    from test_gpu_colliders import CONFIGS as WHITE_CONFIGS
    h.set_solver_order("relaxed")
    h.set_white_config(WHITE_CONFIGS[SHARDED_CFG])
    h.set_cohesion("effective")
    h.set_colliders(list(FOUR_SCENE))
    h.set_forces(list(FORCES))
    h.set_viscosity(0.5, 1.0)
    h.set_containment(*SHARDED_CONTAINMENT)
    return h


@functools.lru_cache(maxsize=None)
def _sharded_model_run():
    from test_gpu_colliders import CONFIGS as WHITE_CONFIGS
    w, y = rm.default_configs()
    m = cm.Hand(dict(w, **WHITE_CONFIGS[SHARDED_CFG]), y, cohesion=SHARDED_COHESION)
    m.set_colliders(FOUR_SCENE)
    m.set_forces(FORCES)
    m.set_viscosity(0.5, 1.0)
    m.set_containment(*SHARDED_CONTAINMENT)
    centers = _centers()
    ids = [m.add(cx, cy, 50, 15) for cx, cy in centers]
    out = []
    for k in range(SHARDED_STEPS):
        for i, c in zip(ids, centers):
            m.set_target_position(i, *circle_target(c, k))
        m.update(H60, H60, 2, 3)
        out.append(dict(state=[m.state(w) for w in (WHITE, YOLK)], contained=m.containment_hits, pairs=m.pair_solves,
                        visc=list(m.viscosity_pairs), pos={int(i): tuple(m.get_position(int(i))) for i in ids}))
    return ids, out


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
        _sharded_configure(sh)
        centers = _centers()
        gids = [sh.add(x, y, 50, 15) for x, y in centers]
        out = []
        for k in range(SHARDED_STEPS):
            for gid, c in zip(gids, centers):
                sh.set_target_position(gid, *circle_target(c, k))
            sh.step(H60, 2, 3)
            out.append(dict(state=_state(sh), pos=sh.positions(), n_local=sum(sh.local.get_n_particles()),
                            pairs=sh.local.stats()["pair_solves"], contained=sh.containment_hits(),
                            local_contained=sh.local.containment_hits(), visc=sh.viscosity_pairs(),
                            containment=sh.containment(), halo=sh.halo_counters()))
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
    """two ranks on one GPU over gloo, the cut through the four_batches cluster, with cohesion, colliders, forces, viscosity
    and containment: through egg_rx_* every rank contains the batches it holds; the fields gathered from both ranks and the
    all-reduced hits are the model's"""
    ids, ref = _sharded_model_run()
    assert all(b["contained"] > a["contained"] for a, b in zip([dict(contained=0)] + ref, ref))
    res = _spawn(2)
    for k, snap in enumerate(ref):
        got = [res[r][k] for r in (0, 1)]
        what = "sharded, step %d" % (k + 1)
        assert all(g["n_local"] > 0 for g in got) and all(g["containment"] == SHARDED_CONTAINMENT for g in got)
        for w in (WHITE, YOLK):
            n = snap["state"][w].shape[1] // len(ids)
            seen = []
            for r in (0, 1):
                for gid, cols in got[r]["state"][w].items():
                    seen.append(gid)
                    for q, f in enumerate(FIELDS):
                        want = snap["state"][w][q][(gid - 1) * n:gid * n]
                        assert np.array_equal(np.array(cols[q]), want), "%s type %d field %s batch %d" % (what, w, f, gid)
            assert sorted(seen) == sorted(ids)
        print("%s: containment hits %s (per rank %s)" % (what, got[0]["contained"], [g["local_contained"] for g in got]))
        assert got[0]["contained"] == got[1]["contained"] == snap["contained"] == sum(g["local_contained"] for g in got), what
        assert min(g["local_contained"] for g in got) > 0, what
        assert sum(g["pairs"] for g in got) == snap["pairs"], what
        assert got[0]["visc"] == got[1]["visc"] == snap["visc"], what
        assert all(g["halo"]["records"] > 0 for g in got), what
