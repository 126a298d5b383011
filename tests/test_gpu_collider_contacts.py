"""Collider contacts of the relaxed step (egg_set_collider_contacts; DESIGN.md section 2.7, "Collider contacts") on the device
against the CPU model tests/contact_model.py, bit for bit: the hand table of tests/test_contact_model.py, one default egg with
a floor, a hinged wall and a free ball that comes down on the egg's flank, on the wall and on the floor at three (S, C) --
plain, with cohesion and friction, with coupling --, a batch of 3 particles per type, a handle without particles, a failed
step, the launch counts, and the refusals.

Compared after every step: x, y, vx, vy, last_x, last_y of every particle, get_colliders(), the motions, the spins with
their pivots, the raw load sums, hits and grips, and collider_contact_solves()."""
import functools

import pytest

import test_collider_census as cc
import test_contact_model as tc
import test_load_model as tl
from contact_model import ContactModel
from coupling_model import CouplingMixin
from relaxed_model import rm
from test_gpu_collider_bodies import KEYS, _assert_step
from test_gpu_collider_walls import CONFIGS, CUTS, LAUNCHES

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
H60 = tl.H60


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _assert_contacts(h, want, what):
    _assert_step(h, want, what)
    assert h.collider_contact_solves() == want["solves"], what


# ------------------------------------------------------------------------------------------------ the hand table
@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_hand_case(egg, name):
    m, steps = tc.hand_model(name)
    w, y = cc.hand_configs()
    h = egg.SimulationHandler()
    h.set_solver_order("relaxed")
    h.set_white_config({k: w[k] for k in KEYS})
    h.set_yolk_config({k: y[k] for k in KEYS})
    tc.hand_configure(h, name)
    got, iterations = h.get_collider_contacts()
    assert ([(0.0, 0) if c is None else (c, 1) for c in got], iterations) == m.get_collider_contacts()
    if tc.CASES[name]["prev"] is not None:
        src = egg.SimulationHandler()
        src.set_white_config({k: w[k] for k in KEYS})
        src.set_yolk_config({k: y[k] for k in KEYS})
        i = src.add(*cc.HAND_TARGET, cc.HAND_RADIUS, cc.HAND_RADIUS, None, None, 2, 2)
        info, ws, ys = src.export_batch(i)
        for state, t in ((ws, WHITE), (ys, YOLK)):
            for p, ((px, py), (vx, vy)) in enumerate(tc.hand_spots(name)[t]):
                state[0, p] = state[4, p] = px
                state[1, p] = state[5, p] = py
                state[2, p], state[3, p] = vx, vy
        assert h.import_batch(info, ws, ys) == i
    for k, want in enumerate(steps):
        assert h.update(*tc.hand_update(name)) == 1
        _assert_contacts(h, want, "%s step %d" % (name, k + 1))


# ------------------------------------------------------------------------------------------------ an egg, a floor, a hinge, a ball
class CoupledContactModel(CouplingMixin, ContactModel):
    """ContactModel with the coupling pass"""


GROUND = tl.GROUND                                        # kinematic: keeps y <= 360
SEESAW = ("wall", 240.0, 352.0, 360.0, 346.0)             # hinged at its left end, under the egg; its right end in the ball's way
DISC = ("disc", 352.0, 322.0, 12.0)                       # free: thrown down along the egg's flank
LIST = (GROUND, SEESAW, DISC)
BODIES = (None, (0.0, 2.0e-6, 0.0, 0.0, 0.0, 1.0), (1.0 / 40.0, 1.0 / 2880.0, 0.0, 400.0, 0.125, 0.5))
SPINS = (None, (240.0, 352.0, 0.0), (352.0, 322.0, 0.25))
MOTIONS = (None, None, (-40.0, 900.0))
CONTACTS = (True, 0.0625, 0.125)
ROUGH = (0.3, 0.5, 0.4)
STEPS = 6
FLAVOURS = ("plain", "cohesive", "coupled")


def _egg_configure(o, flavour, contacts=CONTACTS, bodies=BODIES, loads=True):
    if not isinstance(o, ContactModel):
        o.set_solver_order("relaxed")
        if flavour == "cohesive":
            o.set_white_config(CONFIGS["cohesion"]["white"])
            o.set_cohesion("effective")
    o.set_colliders(list(LIST))
    o.set_forces([("uniform", 0.0, 400.0)])
    if flavour == "cohesive":
        o.set_collider_surfaces(list(ROUGH))
    elif flavour == "coupled":
        o.set_coupling(1.0, 0.75)
    o.set_collider_motion(list(MOTIONS))
    o.set_collider_spin(list(SPINS))
    o.set_collider_loads(loads)
    if bodies is not None:
        o.set_collider_bodies(list(bodies))
    if contacts is not None:
        o.set_collider_contacts(list(contacts), 3)
    return o


@functools.lru_cache(maxsize=None)
def egg_run(flavour, S, C):
    """the scene on the model, once: the snapshot after every step; shared, never changed"""
    w, y = rm.default_configs()
    if flavour == "cohesive":
        m = ContactModel(dict(w, **CONFIGS["cohesion"]["white"]), y, cohesion=True)
    elif flavour == "coupled":
        m = CoupledContactModel(w, y)
    else:
        m = ContactModel(w, y)
    _egg_configure(m, flavour)
    i = m.add(300.0, 300.0, 50, 15)
    out = []
    for _ in range(STEPS):
        m.update(H60, H60, S, C)
        out.append(dict(tc.snap(m), coupled=getattr(m, "coupling_solves", 0)))
    return i, out


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("S,C", [(2, 3), (1, 1), (3, 2)])
def test_an_egg_with_a_floor_a_hinge_and_a_free_ball(egg, flavour, S, C):
    i, steps = egg_run(flavour, S, C)
    h = _egg_configure(egg.SimulationHandler(), flavour)
    assert h.add(300.0, 300.0, 50, 15) == i
    for k, want in enumerate(steps):
        assert h.update(H60, H60, S, C) == 1
        _assert_contacts(h, want, "%s (%d, %d) step %d" % (flavour, S, C, k + 1))
        if flavour == "coupled":
            assert h.coupling_solves() == want["coupled"]
    last = steps[-1]
    # the ball has met the hinged wall's end and the floor (the fires) and the wall has tipped; the egg has pushed the ball (its
    # loads) wherever a step has more than one sub-step to catch its flank in
    assert last["solves"] >= 2 and last["spins"][1][2] != 0.0 and (S == 1 or any(any(step["sums"][0][2]) for step in steps))
    assert last["colliders"][0] == steps[0]["colliders"][0]  # (the ground is kinematic and at rest)


# ------------------------------------------------------------------------------------------------ three particles, and none
def _small_configure(o):
    if not isinstance(o, ContactModel):
        o.set_solver_order("relaxed")
    o.set_colliders([GROUND, ("disc", 300.0, 330.0, 12.0), ("disc", 310.0, 296.0, 10.0)])
    o.set_forces([("uniform", 0.0, 400.0)])
    o.set_collider_spin([None, (300.0, 330.0, 0.25), (310.0, 296.0, -0.5)])
    o.set_collider_motion([None, (0.0, 200.0), (-30.0, 500.0)])
    o.set_collider_loads(True)
    o.set_collider_bodies([None, BODIES[2], (1.0 / 25.0, 1.0 / 1250.0, 0.0, 400.0)])
    o.set_collider_contacts([True, 0.5, 1.0])
    return o


@pytest.mark.parametrize("particles", [3, 0])
def test_a_batch_of_three_particles_and_none(egg, particles):
    """a batch far smaller than a wave, and no batch at all: no stream has work of its own and both kernels run all the same"""
    m = _small_configure(ContactModel())
    h = _small_configure(egg.SimulationHandler())
    if particles:
        assert m.add(300.0, 352.0, 20, 8, particles, particles) == h.add(300.0, 352.0, 20, 8, None, None, particles, particles)
    for k in range(4):
        m.update(H60, H60, 3, 2)
        assert h.update(H60, H60, 3, 2) == 1
        _assert_contacts(h, tc.snap(m), "%d particles step %d" % (particles, k + 1))
    assert h.collider_contact_solves() > 0 and len(m.gaps()) == 3


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
    for k in range(3):
        assert h.update(H60, H60, 2, 3) == 1
    _assert_contacts(h, steps[2], "before the failed step")
    assert steps[2]["solves"] > 0

    def held():
        return (h.get_colliders(), h.get_collider_motion(), h.get_collider_spin(), h.collider_load_sums(), h.get_collider_bodies(),
                h.get_collider_contacts(), h.collider_contact_solves())

    before = held()
    assert h.import_batch(info, ws, ys) == j
    with pytest.raises(egg.EggError, match="relaxed order: a position is NaN"):
        h.step(H60, 2, 3)
    assert held() == before
    h.remove(j)
    for k in (3, 4):  # the records on the device are the host's again: the next steps are the model's
        assert h.update(H60, H60, 2, 3) == 1
        _assert_contacts(h, steps[k], "step %d, after the failed one" % (k + 1))


def test_only_acting_contacts_add_launches(egg):
    """per step: the parent's count (tests/test_gpu_collider_bodies.py's) with contacts unset and with a list set while bodies
    do not act -- no body, or every record off --, S more with bodies alone, and exactly S more than that with contacts acting"""
    S, C = tl.S, tl.C
    counts = {}
    for name, bodies, contacts in (("unset", None, None), ("on_without_a_body", None, CONTACTS), ("on_with_no_body_in_the_list", [None] * 3, CONTACTS),
                                   ("bodies", BODIES, None), ("bodies_all_off", BODIES, [None] * 3), ("acting", BODIES, CONTACTS)):
        h = _egg_configure(egg.SimulationHandler(), "plain", contacts=contacts, bodies=bodies)
        h.set_forces([])
        h.set_collider_motion([])
        h.add(300.0, 300.0, 50, 15)
        counts[name] = []
        for _ in range(3):
            before = h.stats()["kernel_launches"]
            assert h.update(H60, H60, S, C) == 1
            counts[name].append(h.stats()["kernel_launches"] - before)
        assert name == "acting" or h.collider_contact_solves() == 0, name
    print(counts)
    assert counts["unset"][1:] == [LAUNCHES] * 2  # (the first step builds atoms besides)
    assert counts["on_without_a_body"] == counts["on_with_no_body_in_the_list"] == counts["unset"]
    assert counts["bodies"] == counts["bodies_all_off"] == [c + S for c in counts["unset"]]
    assert counts["acting"] == [c + S for c in counts["bodies"]]


def test_the_refusals(egg):
    h = _egg_configure(egg.SimulationHandler(), "plain", loads=False)
    h.add(300.0, 300.0, 50, 15)
    before = h.stats()["kernel_launches"], h.get_colliders()
    with pytest.raises(egg.EggError, match="egg_set_collider_loads"):  # bodies with loads off: as before, nothing is launched
        h.step(H60, 2, 3)
    assert (h.stats()["kernel_launches"], h.get_colliders()) == before
    with pytest.raises(egg.EggError, match="collider bodies run on a single handle only"):
        h.rx_begin(H60, 2, 3)
    h.set_collider_bodies([])
    with pytest.raises(egg.EggError, match="egg_rx_begin: collider contacts run on a single handle only"):  # (whether or not they act)
        h.rx_begin(H60, 2, 3)
    with pytest.raises(egg.EggError, match="exact order has no collider contacts"):
        h.set_solver_order("exact")
    assert h.get_collider_contacts() == ([0.0, 0.0625, 0.125], 3)
    # the library's own checks, under the wrapper's: nothing changes
    arr = (egg._ffi.EggColliderContact * 3)()
    for field, value, match in (("restitution", 1.5, "collider 1: the restitution"), ("on", 2, "collider 1: on = 2"), ("reserved", 7, "collider 1: reserved = 7")):
        for k in range(3):
            arr[k].restitution, arr[k].on, arr[k].reserved = 0.0, 1, 0
        setattr(arr[1], field, value)
        with pytest.raises(egg.EggError, match=match):
            h._check(h._lib.egg_set_collider_contacts(h._h, 3, arr, 4))
    for n, iterations, match in ((2, 4, "n = 2, the list holds 3"), (3, 17, "17 iterations"), (3, -1, "-1 iterations")):
        arr[1].restitution, arr[1].on, arr[1].reserved = 0.0, 1, 0
        with pytest.raises(egg.EggError, match=match):
            h._check(h._lib.egg_set_collider_contacts(h._h, n, arr, iterations))
    assert h.get_collider_contacts() == ([0.0, 0.0625, 0.125], 3)
    h.set_collider_contacts([None, True, None], 0)  # 0 = the default
    assert h.get_collider_contacts() == ([None, 0.0, None], 4)
    h.set_colliders([GROUND])  # a new list clears the records
    assert h.get_collider_contacts() == ([None], 4) and h.collider_contact_solves() == 0
    e = egg.SimulationHandler()  # exact order: a list with nothing on is taken, a contact is not; and a step can be in flight
    e.set_collider_contacts([])
    e.add(0.0, 0.0, 50, 15)
    e.step_begin(H60, 2, 3)
    with pytest.raises(egg.EggError, match="egg_set_collider_contacts: a step is in flight"):
        e.set_collider_contacts([])
    e.step_end(True)
    # a device group: its own setter takes nothing that is on, and a handle that holds a contact makes the group refuse to step
    g = egg.SimulationGroup([0, 0], cuts=CUTS[2])
    g.set_solver_order("relaxed")
    g.set_colliders([GROUND, DISC])
    g.set_collider_loads(True)
    g.set_collider_contacts([None, None])
    with pytest.raises(egg.EggError, match="single SimulationHandler only"):
        g.set_collider_contacts([True, True])
    g.add(240.0, 300.0, 50, 15)
    g.add(360.0, 300.0, 50, 15)
    g.step(H60, 2, 3)
    g.handles[1].set_collider_contacts([True, True])
    with pytest.raises(egg.EggError, match="collider contacts run on a single handle only"):
        g.step(H60, 2, 3)
    g.handles[1].set_collider_contacts([])
    g.step(H60, 2, 3)
