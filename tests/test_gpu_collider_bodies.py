"""Collider bodies of the relaxed step (egg_set_collider_bodies; DESIGN.md section 2.7, "Collider bodies") on the device
against the CPU model tests/body_model.py, bit for bit: the hand table of tests/test_body_model.py, one default egg with a
plate, a hinge and a free disc together at three (S, C) -- once with cohesion and friction, once with coupling --, the same
list with every other relaxed feature on at once, a batch
smaller than a wave with 64 colliders (every lane of the integrator live) and with 3, a handle without particles, a failed
step, the launch counts, and the refusals.

Compared after every step: x, y, vx, vy, last_x, last_y of every particle, get_colliders(), the motions, the spins with
their pivots, the raw load sums, hits and grips."""
import functools

import numpy as np
import pytest

import test_body_model as tb
import test_collider_census as cc
import test_load_model as tl
from body_model import BodyModel
from adhesion_model import AdhesionMixin
from containment_model import ContainmentMixin
from coupling_model import CouplingMixin
from relaxed_model import rm
from test_gpu_collider_surfaces import FIELDS
from test_gpu_collider_walls import CONFIGS, CUTS, LAUNCHES

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
H60 = tl.H60
KEYS = ("damping", "follow_strength", "min_radius", "max_radius", "min_mass", "max_mass")


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _assert_step(h, want, what):
    """the handle after a step against the model's snapshot (tests/test_body_model.py's snap())"""
    for w in (WHITE, YOLK):
        for k, f in enumerate(FIELDS):
            assert np.array_equal(h.download(w, f), want["state"][w][k], equal_nan=True), "%s type %d field %s" % (what, w, f)
    assert [tuple(c) for c in h.get_colliders()] == [tuple(c) for c in want["colliders"]], what
    assert [tuple(v) for v in h.get_collider_motion()] == want["motions"], what
    assert [tuple(v) for v in h.get_collider_spin()] == want["spins"], what
    assert h.collider_load_sums() == want["sums"], what
    assert h.collider_hits() == want["hits"] and h.collider_grips() == want["grips"], what


# ------------------------------------------------------------------------------------------------ the hand table
@pytest.mark.parametrize("name", sorted(tb.CASES))
def test_hand_case(egg, name):
    m, steps = tb.hand_model(name)
    w, y = cc.hand_configs()
    h = egg.SimulationHandler()
    h.set_solver_order("relaxed")
    h.set_white_config({k: w[k] for k in KEYS})
    h.set_yolk_config({k: y[k] for k in KEYS})
    src = egg.SimulationHandler()
    src.set_white_config({k: w[k] for k in KEYS})
    src.set_yolk_config({k: y[k] for k in KEYS})
    i = src.add(*cc.HAND_TARGET, cc.HAND_RADIUS, cc.HAND_RADIUS, None, None, 2, 2)
    info, ws, ys = src.export_batch(i)
    for state, t in ((ws, WHITE), (ys, YOLK)):
        for p, ((px, py), (vx, vy)) in enumerate(tb.hand_spots(name)[t]):
            state[0, p] = state[4, p] = px
            state[1, p] = state[5, p] = py
            state[2, p], state[3, p] = vx, vy
    tb.hand_configure(h, name)
    assert [tuple(b) for b in h.get_collider_bodies()] == m.get_collider_bodies()
    assert h.import_batch(info, ws, ys) == i
    for k, want in enumerate(steps):
        assert h.update(*tb.hand_update(name)) == 1
        _assert_step(h, want, "%s step %d" % (name, k + 1))


# ------------------------------------------------------------------------------------------------ an egg, three bodies
class CoupledBodyModel(CouplingMixin, BodyModel):
    """BodyModel with the coupling pass"""


GROUND = tl.GROUND                                       # kinematic: keeps y <= 360
PLATE = ("half_plane", 0.0, 1.0, 232.0)                   # falls onto the egg's top
SEESAW = ("segment", 240.0, 352.0, 360.0, 346.0)          # hinged at its left end, under the egg
DISC = ("disc", 318.0, 228.0, 12.0)                       # free: falls, rolls off
LIST = (GROUND, PLATE, SEESAW, DISC)
BODIES = (None, (1.0 / 250.0, 0.0, 0.0, 400.0, 0.25, 0.0), (0.0, 2.0e-6, 0.0, 0.0, 0.0, 1.0), (1.0 / 40.0, 1.0 / 2880.0, 0.0, 400.0, 0.125, 0.5))
SPINS = (None, None, (240.0, 352.0, 0.0), (318.0, 228.0, 0.25))
MOTIONS = (None, (0.0, 90.0), None, (-10.0, 150.0))       # the plate and the disc are on their way down
ROUGH = (0.3, 0.2, 0.5, 0.4)
STEPS = 20


def _egg_configure(o, flavour):
    if not isinstance(o, BodyModel):
        o.set_solver_order("relaxed")
        if flavour == "cohesive":
            o.set_white_config(CONFIGS["cohesion"]["white"])
            o.set_cohesion("effective")
    o.set_colliders(list(LIST))
    o.set_forces([("uniform", 0.0, 400.0)])
    if flavour == "cohesive":
        o.set_collider_surfaces(list(ROUGH))
    else:
        o.set_coupling(1.0, 0.75)
    o.set_collider_motion(list(MOTIONS))
    o.set_collider_spin(list(SPINS))
    o.set_collider_loads(True)
    o.set_collider_bodies(list(BODIES))
    return o


@functools.lru_cache(maxsize=None)
def egg_run(flavour, S, C):
    """the scene on the model, once: the snapshot after every step; shared, never changed"""
    w, y = rm.default_configs()
    if flavour == "cohesive":
        m = BodyModel(dict(w, **CONFIGS["cohesion"]["white"]), y, cohesion=True)
    else:
        m = CoupledBodyModel(w, y)
    _egg_configure(m, flavour)
    i = m.add(300.0, 300.0, 50, 15)
    out = []
    for _ in range(STEPS):
        m.update(H60, H60, S, C)
        out.append(dict(tb.snap(m), coupled=getattr(m, "coupling_solves", 0)))
    return i, out


@pytest.mark.parametrize("flavour", ["cohesive", "coupled"])
@pytest.mark.parametrize("S,C", [(2, 3), (1, 1), (3, 2)])
def test_an_egg_with_a_plate_a_hinge_and_a_free_disc(egg, flavour, S, C):
    i, steps = egg_run(flavour, S, C)
    h = _egg_configure(egg.SimulationHandler(), flavour)
    assert h.add(300.0, 300.0, 50, 15) == i
    for k, want in enumerate(steps):
        assert h.update(H60, H60, S, C) == 1
        _assert_step(h, want, "%s (%d, %d) step %d" % (flavour, S, C, k + 1))
        if flavour == "coupled":
            assert h.coupling_solves() == want["coupled"]
    last = steps[-1]
    # every body has been touched and has moved: the plate and the disc are on their way, the seesaw has tipped
    for c in (1, 2, 3):
        assert any(any(step["sums"][0][c]) for step in steps), c
    assert last["colliders"][1][3] != PLATE[3] and last["colliders"][3][1:3] != DISC[1:3] and last["spins"][2][2] != 0.0
    assert last["colliders"][0] == steps[0]["colliders"][0]  # (the ground is kinematic and at rest)
    if flavour == "coupled":
        assert last["coupled"] > 0


class EverythingBodyModel(ContainmentMixin, AdhesionMixin, CouplingMixin, BodyModel):
    """BodyModel with the coupling pass, its adhesion band and containment"""


FENCE = ("wall", 262.0, 240.0, 262.0, 360.0)   # kinematic, left of the egg's middle: a list with a wall


def _everything_configure(o):
    if not isinstance(o, BodyModel):
        o.set_solver_order("relaxed")
    o.set_colliders(list(LIST) + [FENCE])
    o.set_forces([("uniform", 0.0, 400.0)])
    o.set_viscosity(0.5, 1.0)
    o.set_collider_surfaces(list(ROUGH) + [0.25])
    o.set_coupling(1.0, 0.75)
    o.set_adhesion(1.5, 0.5)
    o.set_containment(1.0, 0.5)
    o.set_collider_motion(list(MOTIONS) + [None])
    o.set_collider_spin(list(SPINS) + [None])
    o.set_collider_loads(True)
    o.set_collider_bodies(list(BODIES) + [None])
    return o


def test_bodies_with_every_other_feature_on(egg):
    """coupling with its adhesion band, containment, forces, viscosity, surfaces and a wall, all at once"""
    m = _everything_configure(EverythingBodyModel())
    h = _everything_configure(egg.SimulationHandler())
    assert m.add(300.0, 300.0, 50, 15) == h.add(300.0, 300.0, 50, 15)
    touched = set()
    for k in range(16):
        m.update(H60, H60, 2, 2)
        assert h.update(H60, H60, 2, 2) == 1
        want = tb.snap(m)
        _assert_step(h, want, "everything step %d" % (k + 1))
        touched |= {c for c, s in enumerate(want["sums"][0]) if any(s)}
    assert h.coupling_solves() == m.coupling_solves > 0 and h.adhesion_solves() == m.adhesion_solves > 0
    assert h.containment_hits() == m.containment_hits and h.viscosity_pairs() == m.viscosity_pairs and min(m.viscosity_pairs) > 0
    assert {1, 2, 3} <= touched and m.adhesion_acts() and m.containment_acts()


# ------------------------------------------------------------------------------------------------ a batch smaller than a wave
def _many(n):
    """n colliders over the small batch: the ground, a plate, then small discs inside the batch that fall as free bodies"""
    colliders, bodies, spins = [GROUND, ("half_plane", 0.0, 1.0, 262.0)], [None, BODIES[1]], [None, None]
    for k in range(n - 2):
        cx, cy = 258.0 + 5.0 * (k % 18), 322.0 - 14.0 * (k // 18)
        colliders.append(("disc", cx, cy, 3.0))
        bodies.append((1.0 / (4.0 + k), 1.0 / (30.0 + k), 0.5 * (k % 3 - 1), 300.0 + 10.0 * k, 0.0625 * (k % 4), 0.25) if k % 5 else None)
        spins.append((cx, cy, 0.125 * (k % 7 - 3)))
    return colliders, bodies, spins


def _small_configure(o, n):
    colliders, bodies, spins = _many(n)
    if not isinstance(o, BodyModel):
        o.set_solver_order("relaxed")
    o.set_colliders(colliders)
    o.set_forces([("uniform", 0.0, 400.0)])
    o.set_collider_spin(spins)
    o.set_collider_loads(True)
    o.set_collider_bodies(bodies)
    return o


@pytest.mark.parametrize("n", [64, 3])
def test_a_batch_smaller_than_a_wave(egg, n):
    """37 white and 9 yolk particles; with 64 colliders every lane of the integrator's wave holds one"""
    m = _small_configure(BodyModel(), n)
    h = _small_configure(egg.SimulationHandler(), n)
    assert m.add(300.0, 300.0, 50, 15, 37, 9) == h.add(300.0, 300.0, 50, 15, None, None, 37, 9)
    touched = set()
    for k in range(8):
        m.update(H60, H60, 2, 2)
        assert h.update(H60, H60, 2, 2) == 1
        want = tb.snap(m)
        _assert_step(h, want, "%d colliders step %d" % (n, k + 1))
        touched |= {c for c, s in enumerate(want["sums"][0]) if any(s)}
    assert len(h.get_colliders()) == n and touched - {0}, touched


def test_without_particles_a_body_still_falls(egg):
    """no batch at all: no stream has work of its own, and the integrator runs all the same"""
    m = _small_configure(BodyModel(), 3)
    h = _small_configure(egg.SimulationHandler(), 3)
    for k in range(2):
        m.update(H60, H60, 3, 1)
        assert h.update(H60, H60, 3, 1) == 1
        _assert_step(h, tb.snap(m), "empty step %d" % (k + 1))
    assert h.get_collider_motion()[1][1] > 0.0 and h.get_colliders()[1][3] > 262.0


def test_one_type_alone_cannot_arise(egg):
    """the driver needs no event with one type empty, but no call makes such a handle: add refuses a batch without particles
    of a type (tests/test_gpu_containment.py pins the library's own check)"""
    h = _small_configure(egg.SimulationHandler(), 3)
    with pytest.raises(egg.EggError, match="yolk particle count cannot be 1 or negative"):
        h.add(300.0, 300.0, 50, 15, None, None, 157, 0)
    with pytest.raises(egg.EggError, match="white particle count cannot be 1 or negative"):
        h.add(300.0, 300.0, 50, 15, None, None, 0, 15)


# ------------------------------------------------------------------------------------------------ bookkeeping on the device
def test_a_failed_step_advances_nothing(egg):
    i, steps = egg_run("coupled", 2, 3)
    src = egg.SimulationHandler()
    src.add(300.0, 300.0, 50, 15)
    j = src.add(330.0, 100.0, 50, 15)
    info, ws, ys = src.export_batch(j)
    ws[0, 7] = float("nan")
    h = _egg_configure(egg.SimulationHandler(), "coupled")
    assert h.add(300.0, 300.0, 50, 15) == i
    for k in range(2):
        assert h.update(H60, H60, 2, 3) == 1
    _assert_step(h, steps[1], "before the failed step")
    held = h.get_colliders(), h.get_collider_motion(), h.get_collider_spin(), h.collider_load_sums(), h.collider_loads(), h.get_collider_bodies()
    assert h.import_batch(info, ws, ys) == j
    with pytest.raises(egg.EggError, match="relaxed order: a position is NaN"):
        h.step(H60, 2, 3)
    assert (h.get_colliders(), h.get_collider_motion(), h.get_collider_spin(), h.collider_load_sums(), h.collider_loads(),
            h.get_collider_bodies()) == held
    h.remove(j)
    for k in (2, 3):  # the records on the device are the host's again: the next steps are the model's
        assert h.update(H60, H60, 2, 3) == 1
        _assert_step(h, steps[k], "step %d, after the failed one" % (k + 1))


def test_a_list_without_a_body_launches_what_it_launched(egg):
    """per step: the parent's count without a body (set or not), that plus S with one"""
    S, C = tl.S, tl.C
    counts = {}
    for name, bodies in (("unset", None), ("none", [None] * len(LIST)), ("bodies", list(BODIES))):
        h = egg.SimulationHandler()
        h.set_solver_order("relaxed")
        h.set_colliders(list(LIST))
        h.set_collider_spin(list(SPINS))
        h.set_collider_loads(True)
        if bodies is not None:
            h.set_collider_bodies(bodies)
        h.add(300.0, 300.0, 50, 15)
        counts[name] = []
        for _ in range(3):
            before = h.stats()["kernel_launches"]
            assert h.update(H60, H60, S, C) == 1
            counts[name].append(h.stats()["kernel_launches"] - before)
    print(counts)
    assert counts["unset"][1:] == [LAUNCHES] * 2 and counts["none"] == counts["unset"]  # (the first step builds atoms besides)
    assert counts["bodies"] == [c + S for c in counts["unset"]]


def test_the_refusals(egg):
    h = egg.SimulationHandler()
    h.set_solver_order("relaxed")
    h.set_colliders([PLATE, GROUND])
    h.set_collider_bodies([BODIES[1], None])
    h.add(300.0, 300.0, 50, 15)
    before = h.stats()["kernel_launches"], h.get_colliders()
    with pytest.raises(egg.EggError, match="egg_set_collider_loads"):  # loads off: before anything is launched
        h.step(H60, 2, 3)
    assert (h.stats()["kernel_launches"], h.get_colliders()) == before
    with pytest.raises(egg.EggError, match="collider bodies run on a single handle only"):
        h.rx_begin(H60, 2, 3)
    h.set_collider_loads(True)
    with pytest.raises(egg.EggError, match="collider bodies run on a single handle only"):
        h.rx_begin(H60, 2, 3)
    e = egg.SimulationHandler()  # (exact order: a step that can be in flight)
    e.add(0.0, 0.0, 50, 15)
    e.step_begin(H60, 2, 3)
    with pytest.raises(egg.EggError, match="egg_set_collider_bodies: a step is in flight"):
        e.set_collider_bodies([])
    e.step_end(True)
    arr = (egg._ffi.EggColliderBody * 2)()  # (the wrapper checks first; the library's own check, under it)
    arr[1].drag = -1.0
    with pytest.raises(egg.EggError, match="collider 1: drag"):
        h._check(h._lib.egg_set_collider_bodies(h._h, 2, arr))
    assert [tuple(b) for b in h.get_collider_bodies()] == [BODIES[1], (0.0,) * 6]
    h.set_colliders([PLATE])  # a new list resets the bodies
    assert h.get_collider_bodies() == [(0.0,) * 6]
    # a device group: its own setter takes no body, and a handle that holds one makes the group refuse to step
    g = egg.SimulationGroup([0, 0], cuts=CUTS[2])
    g.set_solver_order("relaxed")
    g.set_colliders([PLATE, GROUND])
    g.set_collider_loads(True)
    g.set_collider_bodies([None, None])
    with pytest.raises(egg.EggError, match="single SimulationHandler only"):
        g.set_collider_bodies([BODIES[1], None])
    g.add(240.0, 300.0, 50, 15)
    g.add(360.0, 300.0, 50, 15)
    g.step(H60, 2, 3)
    g.handles[1].set_collider_bodies([BODIES[1], None])
    with pytest.raises(egg.EggError, match="collider bodies run on a single handle only"):
        g.step(H60, 2, 3)
    g.handles[1].set_collider_bodies([])
    g.step(H60, 2, 3)
