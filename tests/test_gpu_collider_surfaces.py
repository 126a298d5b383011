"""Collider surfaces of the relaxed pass (egg_set_collider_surfaces; DESIGN.md section 2.7, "Collider surfaces") on the device
against the CPU model tests/surface_model.py, bit for bit: on one handle (the four surface instantiations of the gather
kernel: cohesion off / on), on a device group (several handles on GPU 0) and on a ShardedSimulationHandler (ranks are
spawned processes on GPU 0 over gloo, as in test_gpu_colliders.py)."""
import functools
import math

import numpy as np
import pytest

from conftest import ROOT, circle_target, load_golden
from relaxed_model import rm
from surface_model import SurfaceModel
from viscosity_model import ViscosityModel

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
FIELDS = ("x", "y", "vx", "vy", "last_x", "last_y")
ENV_KEYS = ("min_x", "min_y", "max_x", "max_y", "centroid_x", "centroid_y", "max_radius", "max_velocity",
            "last_centroid_x", "last_centroid_y")
INF = math.inf
# configs: the default; white that coheres (with effective cohesion and viscosity on: the cohesive instantiations and the
# viscosity pass that rewrites prev after the sub-step's last collision pass); no follow constraint (forces alone move)
CONFIGS = {
    "default": dict(white={}, yolk={}, cohesion=False, viscosity=(0.0, 0.0)),
    "white3": dict(white=dict(cohesion_interaction_distance_factor=3, cohesion_strength=0.99), yolk={}, cohesion=True,
                   viscosity=(0.5, 1.0)),
    "free": dict(white=dict(follow_strength=0), yolk=dict(follow_strength=0), cohesion=False, viscosity=(0.0, 0.0)),
}
# the scene of test_gpu_colliders.py -- four_batches inside a container, over a floor, across a wall, around a white-only
# disc -- under gravity, with a surface per collider: a rough container, a conveyor floor, a wall without friction (its
# velocity alone does nothing) and a rough disc that also moves
SCENE = (("container", 50.0, 60.0, 150.0), ("half_plane", 0.0, 3.0, -30.0), ("segment", -40.0, 50.0, 120.0, 50.0),
         ("disc", 10.0, 20.0, 15.0, "white"))
SURFACES = (0.6, (0.3, 90.0, 0.0), (0.0, 500.0, 500.0), (0.2, -40.0, 25.0))
GRAVITY = (("uniform", 0.0, 400.0),)


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _model(cfg="default", colliders=(), surfaces=None, forces=(), cls=SurfaceModel):
    w, y = rm.default_configs()
    c = CONFIGS[cfg]
    m = cls(dict(w, **c["white"]), dict(y, **c["yolk"]), cohesion=c["cohesion"])
    m.set_viscosity(*c["viscosity"])
    m.set_colliders(colliders)
    m.set_forces(forces)
    if surfaces is not None:
        m.set_collider_surfaces(surfaces)
    return m


def _configure(h, cfg="default", colliders=(), surfaces=None, forces=()):
    """a SimulationHandler, SimulationGroup or ShardedSimulationHandler set up as _model sets the model up"""
    c = CONFIGS[cfg]
    h.set_solver_order("relaxed")
    if c["white"]:
        h.set_white_config(c["white"])
    if c["yolk"]:
        h.set_yolk_config(c["yolk"])
    if c["cohesion"]:
        h.set_cohesion("effective")
    h.set_viscosity(*c["viscosity"])
    h.set_colliders(list(colliders))
    h.set_forces(list(forces))
    if surfaces is not None:
        h.set_collider_surfaces(list(surfaces))
    return h


def _handle(egg, *args, **kwargs):
    return _configure(egg.SimulationHandler(), *args, **kwargs)


def _centers():
    return [tuple(float(v) for v in c) for c in load_golden("four_batches")["centers"]]


def _snapshot(m, ids):
    return dict(state=[m.state(w) for w in (WHITE, YOLK)],
                env=[dict(m._last_white_env if w == WHITE else m._last_yolk_env) for w in (WHITE, YOLK)],
                pos={int(i): tuple(m.get_position(int(i))) for i in ids}, pairs=m.pair_solves,
                cohered=m.cohesion_solves, hits=list(m.collider_hits), grips=list(getattr(m, "collider_grips", [0, 0])),
                sticks=list(getattr(m, "grip_sticks", [0, 0])), visc=list(m.viscosity_pairs))


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
    print("%s: pair_solves %d, hits %s, grips %s (model sticks %s)" % (what, st["pair_solves"], h.collider_hits(), h.collider_grips(),
                                                                      snap["sticks"]))
    assert st["pair_solves"] == snap["pairs"], what
    assert st["cohesion_solves"] == snap["cohered"], what
    assert h.collider_hits() == snap["hits"], what
    assert h.collider_grips() == snap["grips"], what
    assert h.viscosity_pairs() == snap["visc"], what


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


# ---- smallest shapes: tiny batches (2 + 2 particles of radius 4, the fewest add accepts) at (295, 296) [and (301, 296)] --
# particles at (295, 296), (296.7, 276.3) [and 6 px to the right] --, every collider already in touch with them, no follow
# constraint, a uniform force into (+x) and along (+y) the collider
SMALL = {
    "half_plane": ("half_plane", -1.0, 0.0, -298.0),
    "disc": ("disc", 340.0, 290.0, 45.0),
    "container": ("container", 300.0, 290.0, 10.0),
    "segment": ("segment", 298.5, 250.0, 298.5, 340.0),
}
PUSH = (("uniform", 900.0, 600.0),)
STICK_MU, SLIDE_MU = 50.0, 1.0e-4


def small_scene(kind, n_batches, mu, make, add):
    """(object, ids) of the smallest-shapes scene; `make(cfg, colliders, surfaces, forces)` builds the model or the handle"""
    colliders = [SMALL[kind]] if kind in SMALL else [SMALL["half_plane"], ("disc", 296.0, 286.0, 8.0), SMALL["segment"]]
    surfaces = [mu] if kind in SMALL else [0.0, mu, (mu, 0.0, -60.0)]  # mixed: the first collider has mu = 0
    o = make("free", colliders, surfaces, PUSH)
    return o, [add(o, x, y) for x, y in [(295.0, 296.0), (301.0, 296.0)][:n_batches]]


def _small_model(kind, n_batches, mu):
    return small_scene(kind, n_batches, mu, _model, lambda m, x, y: m.add(x, y, 28, 28, 2, 2))


@pytest.mark.parametrize("n_batches", [1, 2])
@pytest.mark.parametrize("branch,mu", [("stick", STICK_MU), ("slide", SLIDE_MU)])
@pytest.mark.parametrize("kind", sorted(SMALL) + ["mixed"])
def test_smallest_shapes(egg, kind, branch, mu, n_batches):
    m, ids = _small_model(kind, n_batches, mu)
    h, hids = small_scene(kind, n_batches, mu, functools.partial(_handle, egg),
                          lambda o, x, y: o.add(x, y, 28, 28, None, None, 2, 2))
    assert hids == ids
    _step_both(h, m, ids, None, 0, moving=False)
    _assert_same(h, m, ids, "%s, %s, %d tiny batches" % (kind, branch, n_batches))
    # the branch the run is for really fires on the model
    sticks, slides = sum(m.grip_sticks), sum(m.collider_grips) - sum(m.grip_sticks)
    assert (sticks if branch == "stick" else slides) > 0, (sticks, slides)
    got = h.get_collider_surfaces()
    assert got == [tuple(s) for s in m.surfaces] and len(got) == len(h.get_colliders())
    if kind == "mixed":
        assert got[0] == (0.0, 0.0, 0.0) and m.collider_hits[WHITE] > m.collider_grips[WHITE] > 0


# ---- corner cases
def _import_pair(egg, m, spots, colliders, surfaces, forces, cfg="free", radius=28):
    """a handle holding one tiny batch whose two particles per type sit at `spots[type]` with zero velocity, and the model in
    the same state (add does not put a particle on a chosen spot: the state goes in through egg_import_batch)"""
    src = egg.SimulationHandler()
    i = src.add(300.0, 300.0, radius, radius, None, None, 2, 2)
    info, ws, ys = src.export_batch(i)
    assert m.add(300.0, 300.0, radius, radius, 2, 2) == i
    for state, data, w in ((ws, m._white_data, WHITE), (ys, m._yolk_data, YOLK)):
        for p in (0, 1):
            x, y = spots[w][p]
            state[0, p] = state[4, p] = x
            state[1, p] = state[5, p] = y
            state[2, p] = state[3, p] = 0.0
            for off, v in ((rm.X, x), (rm.Y, y), (rm.LAST_X, x), (rm.LAST_Y, y), (rm.VX, 0.0), (rm.VY, 0.0)):
                data[rm.offset(p + 1) + off] = v
    h = _handle(egg, cfg, colliders, surfaces, forces)
    assert h.import_batch(info, ws, ys) == i
    return h, i


CENTRE = dict(colliders=[("disc", 300.0, 300.0, 5.0)], surfaces=[(0.5, 240.0, -90.0)], forces=(),
              spots=[[(570.0, 250.0), (300.0, 300.0)], [(300.0, 300.0), (480.0, 250.0)]])
# (a batch of radius 400: the follow constraint is slack within 40 px of the target (300, 300), so nothing but gravity and
# the floor y <= 305 - r touches the four particles, which start 2 px inside the floor and 30 / 16 px apart)
DROP = dict(colliders=[("half_plane", 0.0, -1.0, -305.0)], surfaces=[3.0], forces=(("uniform", 0.0, 800.0),), radius=400,
            spots=[[(285.0, 303.0), (315.0, 303.0)], [(292.0, 303.0), (308.0, 303.0)]])


def centre_model():
    return _model("free", CENTRE["colliders"], CENTRE["surfaces"], CENTRE["forces"])


def drop_model():
    return _model("free", DROP["colliders"], DROP["surfaces"], DROP["forces"])


def test_a_particle_on_a_discs_centre(egg):
    """white particle 1 and yolk particle 0 rest exactly on the disc's centre, the other particle of the type far away: the
    projection sends them out along DIRS[key & 7] with pen = m, and the surface -- it moves, so the displacement relative to
    it has a tangential part -- grips them in that very pass"""
    m = centre_model()
    h, i = _import_pair(egg, m, CENTRE["spots"], CENTRE["colliders"], CENTRE["surfaces"], CENTRE["forces"])
    assert h.update(1 / 60, 1 / 60, 1, 1) == 1
    m.update(1 / 60, 1 / 60, 1, 1)
    assert m.collider_hits == [1, 1] and m.collider_grips == [1, 1]
    _assert_same(h, m, [i], "on the centre, first step")
    for k in range(3):
        _step_both(h, m, [i], None, k, moving=False)
    _assert_same(h, m, [i], "on the centre, later")


def test_a_container_smaller_than_the_particles(egg):
    """R < r = 4: m = 0, the projection puts every particle on the centre with pen = d"""
    colliders, surfaces = [("container", 300.0, 290.0, 3.0)], [0.4]
    m, h = _model("free", colliders, surfaces, PUSH), _handle(egg, "free", colliders, surfaces, PUSH)
    ids = [h.add(295.0, 296.0, 28, 28, None, None, 2, 2)]
    assert [m.add(295.0, 296.0, 28, 28, 2, 2)] == ids
    for k in range(2):
        _step_both(h, m, ids, None, k, moving=False)
        _assert_same(h, m, ids, "container with R < r, step %d" % (k + 1))
    assert min(m.collider_grips) > 0
    for w in (WHITE, YOLK):  # (the projection puts a particle on the centre; the grip then takes tangential motion back)
        assert np.hypot(m.state(w)[0] - 300.0, m.state(w)[1] - 290.0).max() < 1.0


def test_a_straight_drop_grips_nothing(egg):
    """particles far from each other fall straight onto a floor: the displacement has no tangential part (tl2 == 0), so a
    rough floor counts hits and no grips"""
    m = drop_model()
    h, i = _import_pair(egg, m, DROP["spots"], DROP["colliders"], DROP["surfaces"], DROP["forces"], radius=DROP["radius"])
    for k in range(3):
        _step_both(h, m, [i], None, k, moving=False)
    assert min(m.collider_hits) > 0 and m.collider_grips == [0, 0]
    for w in (WHITE, YOLK):  # (straight: no particle has left its column)
        assert [float(v) for v in m.state(w)[0]] == [x for x, _ in DROP["spots"][w]]
    _assert_same(h, m, [i], "straight drop")
    assert h.collider_grips() == [0, 0]


CONVEYOR = dict(colliders=[("half_plane", 0.0, -1.0, -330.0)], surfaces=[(0.8, 150.0, 0.0)], forces=(("uniform", 0.0, 800.0),))


def conveyor_model(steps):
    m = _model("free", CONVEYOR["colliders"], CONVEYOR["surfaces"], CONVEYOR["forces"])
    ids = [m.add(300.0, 300.0, 50, 15)]
    x0 = float(np.mean(m.state(WHITE)[0]))
    for _ in range(steps):
        m.update(1 / 60, 1 / 60, 2, 3)
    return m, ids, float(np.mean(m.state(WHITE)[0])) - x0


def test_a_conveyor_drags_what_lies_on_it(egg):
    """a floor whose surface moves along +x under gravity straight down: no force has a tangential part, and the whites
    pick up the surface's direction"""
    steps = 6
    m, ids, travel = conveyor_model(steps)
    assert travel > 0.0 and min(m.collider_grips) > 0
    h = _handle(egg, "free", CONVEYOR["colliders"], CONVEYOR["surfaces"], CONVEYOR["forces"])
    assert [h.add(300.0, 300.0, 50, 15)] == ids
    for _ in range(steps):
        assert h.update(1 / 60, 1 / 60, 2, 3) == 1
    _assert_same(h, m, ids, "conveyor")
    assert float(np.mean(h.download(WHITE, "vx"))) > 0.0


# ---- parity
@functools.lru_cache(maxsize=None)
def _model_run(cfg, S, C, steps=(1, 8, 20)):
    """four_batches with moving targets among SCENE with SURFACES under GRAVITY on the model, once per (config, S, C):
    snapshots after `steps`, shared by the tests that need them and never changed"""
    m, centers = _model(cfg, SCENE, SURFACES, GRAVITY), _centers()
    ids = [m.add(cx, cy, 50, 15) for cx, cy in centers]
    out = {}
    for k in range(max(steps)):
        for i, c in zip(ids, centers):
            m.set_target_position(i, *circle_target(c, k))
        m.update(1 / 60, 1 / 60, S, C)
        if k + 1 in steps:
            out[k + 1] = _snapshot(m, ids)
    return out


@pytest.mark.parametrize("S,C", [(2, 3), (3, 2), (1, 1)])
@pytest.mark.parametrize("cfg", ["default", "white3"])
def test_parity_with_model(egg, cfg, S, C):
    ref = _model_run(cfg, S, C)
    assert min(ref[1]["grips"]) > 0, "no surface grips in the first step on the model"
    assert 0 < sum(ref[20]["sticks"]) < sum(ref[20]["grips"])  # (both branches)
    assert (ref[20]["cohered"] > 0) == (min(ref[20]["visc"]) > 0) == CONFIGS[cfg]["cohesion"]
    h, centers = _handle(egg, cfg, SCENE, SURFACES, GRAVITY), _centers()
    ids = [h.add(cx, cy, 50, 15) for cx, cy in centers]
    for k in range(20):
        for i, c in zip(ids, centers):
            h.set_target_position(i, *circle_target(c, k))
        assert h.update(1 / 60, 1 / 60, S, C) == 1
        if k + 1 in (1, 20):
            _assert_snapshot(h, ref[k + 1], "%s S=%d C=%d step %d" % (cfg, S, C, k + 1))


# ---- toggling
def test_toggling(egg):
    h, m, never = _handle(egg, "default", SCENE, None, GRAVITY), _model("default", SCENE, None, GRAVITY), _handle(egg)
    plain = _model("default", SCENE, None, GRAVITY, cls=ViscosityModel)  # (the model before surfaces existed)
    centers = _centers()
    ids = [h.add(cx, cy, 50, 15) for cx, cy in centers]
    assert [m.add(cx, cy, 50, 15) for cx, cy in centers] == ids == [never.add(cx, cy, 50, 15) for cx, cy in centers]
    assert [plain.add(cx, cy, 50, 15) for cx, cy in centers] == ids
    default = [(0.0, 0.0, 0.0)] * len(SCENE)
    assert h.get_collider_surfaces() == default
    k, launches = 0, []
    # unset, all default, velocity only: the collider model's bits, and no grips
    for surfaces in (None, [None] * len(SCENE), [(0.0, 70.0, -30.0)] * len(SCENE)):
        if surfaces is not None:
            h.set_collider_surfaces(surfaces)
            m.set_collider_surfaces(surfaces)
        for _ in range(2):
            before = h.stats()["kernel_launches"]
            for i, c in zip(ids, centers):
                plain.set_target_position(i, *circle_target(c, k))
            plain.update(1 / 60, 1 / 60, 2, 3)
            _step_both(h, m, ids, centers, k)
            launches.append(h.stats()["kernel_launches"] - before)
            k += 1
            _assert_same(h, m, ids, "step %d, surfaces %r" % (k, surfaces and surfaces[0]))
            _assert_same(h, plain, ids, "step %d against the collider model" % k)
    assert h.collider_grips() == [0, 0]
    # friction on: the surface model's bits, grips counted, not the collider model's bits any more
    h.set_collider_surfaces(list(SURFACES))
    m.set_collider_surfaces(SURFACES)
    assert h.get_collider_surfaces() == [tuple(s) for s in m.surfaces]
    for _ in range(2):
        before = h.stats()["kernel_launches"]
        _step_both(h, m, ids, centers, k)
        launches.append(h.stats()["kernel_launches"] - before)
        k += 1
        _assert_same(h, m, ids, "step %d with friction" % k)
    assert m.collider_grips[WHITE] > 0  # (in these two steps no yolk touches a collider with friction)
    grips = list(m.collider_grips)
    # set_colliders clears the surfaces; [] clears them too
    h.set_colliders(list(SCENE))
    m.set_colliders(SCENE)
    assert h.get_collider_surfaces() == default
    h.set_collider_surfaces([0.5] * len(SCENE))
    h.set_collider_surfaces([])
    assert h.get_collider_surfaces() == default
    for _ in range(2):
        before = h.stats()["kernel_launches"]
        _step_both(h, m, ids, centers, k)
        launches.append(h.stats()["kernel_launches"] - before)
        k += 1
        _assert_same(h, m, ids, "step %d after set_colliders" % k)
    assert m.collider_grips == grips
    # with surfaces, with friction or without, a step launches what a handle launches that never had a collider (counted
    # the way test_gpu_relaxed.test_launches_of_one_step counts; a handle's first step builds its per-particle atoms besides)
    for j in range(2):
        before = never.stats()["kernel_launches"]
        for i, c in zip(ids, centers):
            never.set_target_position(i, *circle_target(c, j))
        assert never.update(1 / 60, 1 / 60, 2, 3) == 1
    bare = never.stats()["kernel_launches"] - before
    assert launches[1:] == [bare] * (len(launches) - 1) == [2 * (2 + 5 * 2 * 3 + 1)] * (len(launches) - 1)


# ---- refusals
def test_refusals(egg):
    colliders = [("container", 400.0, 300.0, 12.0), ("half_plane", 0.0, -4.0, -330.0, "white")]
    good = [(0.5, 10.0, 0.0), 0.25]
    h, m = _handle(egg, "default", colliders, good, GRAVITY), _model("default", colliders, good, GRAVITY)
    ids = [h.add(400.0, 300.0, 50, 15)]
    assert [m.add(400.0, 300.0, 50, 15)] == ids
    stored = h.get_collider_surfaces()
    assert stored == [(0.5, 10.0, 0.0), (0.25, 0.0, 0.0)]
    nan, inf = float("nan"), float("inf")
    for bad, text in (([0.5], "n = 1"), ([0.5, 0.5, 0.5], "n = 3"),            # n is neither the collider count nor 0
                      ([0.5, -0.25], "collider 1"), ([0.5, nan], "collider 1"), ([0.5, inf], "collider 1"),  # friction
                      ([0.5, (0.1, nan, 0.0)], "collider 1"), ([0.5, (0.1, 0.0, -inf)], "collider 1"),       # velocity
                      ([(-1.0, 0.0, 0.0), 0.5], "collider 0")):
        with pytest.raises(egg.EggError, match="egg_set_collider_surfaces: " + text):
            h.set_collider_surfaces(bad)
        assert h.get_collider_surfaces() == stored
    lib = egg._ffi.load()
    assert lib.egg_set_collider_surfaces(h._h, 2, None) == egg._ffi.EGG_ERR_INVALID_ARGUMENT
    assert lib.egg_get_collider_grips(h._h, None) == egg._ffi.EGG_ERR_INVALID_ARGUMENT
    assert h.get_collider_surfaces() == stored
    h.set_collider_surfaces([(-0.0, -0.0, -0.0), (0.25, 0.0, -0.0)])  # a -0.0 is stored as +0.0, in every field
    assert all(math.copysign(1.0, v) == 1.0 for sf in h.get_collider_surfaces() for v in sf)
    h.set_collider_surfaces(good)
    for bad in ([(1.0, 2.0)], ["rough"], [object()]):  # what only the host can check
        with pytest.raises(egg.EggError, match="collider surface 0"):
            h.set_collider_surfaces(bad)
    for k in range(2):  # the records every refusal left alone are the ones the steps use
        _step_both(h, m, ids, None, k, moving=False)
    _assert_same(h, m, ids, "after the refusals")
    assert min(m.collider_grips) > 0
    # without colliders only n = 0 is accepted, in either order
    e = egg.SimulationHandler()
    e.set_collider_surfaces([])
    with pytest.raises(egg.EggError, match="n = 1"):
        e.set_collider_surfaces([0.5])
    assert e.get_collider_surfaces() == [] and e.collider_grips() == [0, 0]
    # while a step is in flight
    e.add(0.0, 0.0, 50, 15)
    e.step_begin(1 / 60, 2, 3)
    with pytest.raises(egg.EggError, match="in flight"):
        e.set_collider_surfaces([])
    e.step_end(True)
    # the group: the same rules, and a refused call changes no handle
    g = _configure(egg.SimulationGroup([0, 0], cuts=[-INF, 0.0, INF]), "default", colliders, good, GRAVITY)
    for bad in ([0.5], [0.5, -0.25], [0.5, (0.1, nan, 0.0)]):
        with pytest.raises(egg.EggError):
            g.set_collider_surfaces(bad)
    assert g.get_collider_surfaces() == stored and all(b.get_collider_surfaces() == stored for b in g.handles)
    g.handles[1].set_collider_surfaces([])  # handles that differ: the step is refused
    g.add(400.0, 300.0, 50, 15)
    with pytest.raises(egg.EggError, match="collider surfaces"):
        g.step(1 / 60, 2, 3)
    g.set_colliders(colliders)
    assert all(b.get_collider_surfaces() == [(0.0, 0.0, 0.0)] * 2 for b in g.handles)
    g.step(1 / 60, 2, 3)


def test_a_failed_step_adds_no_grips(egg):
    wall, rough = [("half_plane", -1.0, 0.0, -310.0)], [0.7]
    h, m = _handle(egg, "default", wall, rough, GRAVITY), _model("default", wall, rough, GRAVITY)
    ids = [h.add(300.0, 300.0, 50, 15)]
    assert [m.add(300.0, 300.0, 50, 15)] == ids
    _step_both(h, m, ids, None, 0, moving=False)
    assert h.collider_grips() == m.collider_grips and min(m.collider_grips) > 0
    far = h.add(1.0e12, 0.0, 50, 15)  # its cells lie beyond +-2^30: the step fails, after its passes have gripped
    with pytest.raises(egg.EggError, match="relaxed order"):
        h.step(1 / 60, 2, 3)
    assert h.collider_grips() == m.collider_grips and h.collider_hits() == m.collider_hits and h.stats()["steps"] == 1
    h.remove(far)
    _step_both(h, m, ids, None, 1, moving=False)
    for w in (WHITE, YOLK):
        for k, f in enumerate(FIELDS):
            assert np.array_equal(h.download(w, f), m.state(w)[k]), (w, f)
    assert h.collider_grips() == m.collider_grips


# ---- device groups
CUTS = {2: [-INF, 10.0, INF], 3: [-INF, -5.0, 25.0, INF]}  # through the four_batches cluster, the wall and the container


@pytest.mark.parametrize("n_handles", [2, 3])
def test_device_group_equals_one_handle(egg, n_handles):
    """cuts through the cluster: the colliders of SCENE lie across them, so particles a device has gripped are ghosts of
    its neighbours in the next pass.  white3: the group-cohesive surface instantiation and the viscosity halo; the plain
    group one runs in the 2-handle case besides."""
    for cfg, steps in (("white3", 20),) + ((("default", 8),) if n_handles == 2 else ()):
        g = _configure(egg.SimulationGroup([0] * n_handles, cuts=CUTS[n_handles]), cfg, SCENE, SURFACES, GRAVITY)
        h, centers = _handle(egg, cfg, SCENE, SURFACES, GRAVITY), _centers()
        assert g.get_collider_surfaces() == h.get_collider_surfaces() and len(h.get_collider_surfaces()) == len(SCENE)
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
        assert sum(b.stats()["pair_solves"] for b in g.handles) == h.stats()["pair_solves"]
        assert g.collider_hits() == h.collider_hits()
        assert g.collider_grips() == h.collider_grips()
        assert g.collider_grips() == [sum(b.collider_grips()[w] for b in g.handles) for w in (WHITE, YOLK)]
        assert sum(1 for b in g.handles if sum(b.collider_grips()) > 0) >= 2  # (more than one device gripped)
        assert g.halo_counters()["records"] > 0
        # the single handle itself is the model's (a step of the shared run)
        _assert_snapshot(h, _model_run(cfg, 2, 3)[steps], "the one handle")


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
        _configure(sh, "white3", SCENE, SURFACES, GRAVITY)
        centers = _centers()
        gids = [sh.add(x, y, 50, 15) for x, y in centers]
        for k in range(SHARDED_STEPS):
            for gid, c in zip(gids, centers):
                sh.set_target_position(gid, *circle_target(c, k))
            sh.step(1 / 60, 2, 3)
        st = sh.local.stats()
        q.put((rank, "ok", dict(state=_state(sh), pos=sh.positions(), pairs=st["pair_solves"], cohered=st["cohesion_solves"],
                                hits=sh.collider_hits(), grips=sh.collider_grips(), own_grips=sh.local.collider_grips(),
                                surfaces=sh.get_collider_surfaces(), halo=sh.halo_counters())))
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
    """two ranks on one GPU, the cut through the cluster and the colliders; cohesion and viscosity on: the fields gathered
    from both ranks are the model's, and so are the all-reduced grips"""
    res = _spawn(2)
    snap = _model_run("white3", 2, 3)[SHARDED_STEPS]
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
    want_surfaces = [tuple(s) for s in _model("default", SCENE, SURFACES).surfaces]
    for r in (0, 1):
        assert {g: tuple(p) for g, p in res[r]["pos"].items()} == snap["pos"]
        assert res[r]["hits"] == snap["hits"] and res[r]["grips"] == snap["grips"]
        assert [tuple(s) for s in res[r]["surfaces"]] == want_surfaces
        assert res[r]["halo"]["records"] > 0 and res[r]["halo"]["bytes"] == 40 * res[r]["halo"]["records"]
    assert [sum(res[r]["own_grips"][w] for r in (0, 1)) for w in (WHITE, YOLK)] == snap["grips"]
    assert all(sum(res[r]["own_grips"]) > 0 for r in (0, 1)) and min(snap["grips"]) > 0
    assert sum(res[r]["pairs"] for r in (0, 1)) == snap["pairs"]
    assert sum(res[r]["cohered"] for r in (0, 1)) == snap["cohered"] > 0
