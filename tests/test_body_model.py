"""tests/body_model.py, the definition of collider bodies ("Collider bodies"), against what the
definition promises: a hand table of tiny scenes (tests/test_gpu_collider_bodies.py runs the same table on the device), seven
wrong rules that each change a case, equality with LoadModel where the definition says so, the closed loop of a body nothing
touches, the momentum a plate takes against the loads the steps reported, and the plate experiment the loads section left
undone.  No device needed.

The hand scenes use the tiny batch of tests/test_collider_census.py: two particles per type of radius 2, no damping, no
follow constraint, h = 1 / 64.  White particle 0 and yolk particle 1 are under test, at the same spot, at rest; their mates
rest at REST, which no collider of the table reaches."""
import functools

import numpy as np
import pytest

import test_collider_census as cc
import test_load_model as tlm
from body_model import WRONG, ZERO, BodyModel, cayley, normalise
from load_model import LoadModel
from relaxed_model import rm

WHITE, YOLK = 0, 1
H64 = cc.H64
FLOOR = ("half_plane", 0.0, 1.0, -10.0)   # keeps y >= -10 + r = -8
BAR = ("segment", 0.0, 0.0, 16.0, 0.0)
BALL = ("disc", 0.0, 0.0, 3.0)
PEG = ("disc", 40.0, -30.0, 2.0)          # touches nothing: a kinematic neighbour that moves


def _case(colliders, bodies, prev, S, steps, surfaces=None, motions=None, spins=None):
    return dict(colliders=list(colliders), bodies=list(bodies), prev=prev, S=S, steps=steps, surfaces=surfaces, motions=motions, spins=spins)


CASES = {
    # a plate that rises into the particles 1 px inside it, with an acceleration and a drag: they push it back down
    "plate": _case([FLOOR], [(0.3, 0.0, 0.1, -37.3, 3.0, 0.0)], (16.0, -9.0), 2, 2, motions=[(1.7, 3.3)]),
    # a bar hinged at its left end, at rest: what lies on it 8 px out turns it
    "hinge": _case([BAR], [(0.0, 0.05, 0.0, 0.0, 0.0, 1.5)], (8.0, 1.5), 2, 2, spins=[(0.0, 0.0, 0.0)]),
    # a heavy free disc, rough, turning and accelerating into the particles: it meets them in every sub-step, and its pivot
    # (its centre) has moved by then
    "ball": _case([BALL], [(0.001, 0.00001, 0.0, 30000.0, 0.0, 0.0)], (1.0, 4.5), 3, 1, surfaces=[0.5], motions=[(0.0, 32.0)],
                  spins=[(0.0, 0.0, 2.0)]),
    # the plate again beside a kinematic collider that moves
    "neighbour": _case([FLOOR, PEG], [(0.3, 0.0), None], (16.0, -9.0), 2, 1, motions=[None, (64.0, 0.0)]),
    # a plate nothing reaches: free fall with drag, beside a hinge nothing reaches that spins down
    "untouched": _case([FLOOR, ("segment", 100.0, 100.0, 120.0, 100.0)], [(2.0, 0.0, 3.0, -5.0, 0.5, 0.0), (0.0, 1.0, 0.0, 0.0, 0.0, 2.0)],
                       (16.0, 0.0), 3, 2, motions=[(1.0, 0.0), None], spins=[None, (100.0, 100.0, 4.0)]),
}
CHANGED_BY = {
    "impulse_not_per_h": ("plate", "hinge", "ball"),
    "stale_pivot": ("ball",),
    "accel_first": ("plate",),
    "seen_kept": ("plate", "hinge"),
    "libm_turn": ("hinge",),
    "neighbours_stay": ("neighbour",),
    "drag_first": ("plate", "hinge"),
}


def hand_configure(o, name, loads=True):
    """the case's list on a model or a handle"""
    c = CASES[name]
    o.set_colliders(c["colliders"])
    if c["surfaces"] is not None:
        o.set_collider_surfaces(c["surfaces"])
    if c["motions"] is not None:
        o.set_collider_motion(c["motions"])
    if c["spins"] is not None:
        o.set_collider_spin(c["spins"])
    o.set_collider_loads(loads)
    o.set_collider_bodies(c["bodies"])


def hand_spots(name):
    tested, rest = (CASES[name]["prev"], (0.0, 0.0)), (cc.REST, (0.0, 0.0))
    return {w: [tested if p == cc.TESTED[w] else rest for p in (0, 1)] for w in (WHITE, YOLK)}


def hand_update(name):
    S = CASES[name]["S"]
    return (S * H64, S * H64, S, 1)


def snap(m):
    """what a step leaves, on a model or a handle's twin of it: compared after every step"""
    return dict(state=[m.state(w) for w in (WHITE, YOLK)], colliders=m.get_colliders(), motions=m.get_collider_motion(),
                spins=m.get_collider_spin(), sums=m.collider_load_sums(), hits=list(m.collider_hits), grips=list(m.collider_grips))


def same(a, b):
    return all(np.array_equal(a["state"][w], b["state"][w], equal_nan=True) for w in (WHITE, YOLK)) and \
        all(a[k] == b[k] for k in a if k != "state")


def hand_run(name, wrong=None, cls=BodyModel):
    m = cls(*cc.hand_configs()) if wrong is None else cls(*cc.hand_configs(), wrong=wrong)
    hand_configure(m, name)
    m.add(*cc.HAND_TARGET, cc.HAND_RADIUS, cc.HAND_RADIUS, 2, 2)
    for w, data in ((WHITE, m._white_data), (YOLK, m._yolk_data)):
        for p, ((x, y), (vx, vy)) in enumerate(hand_spots(name)[w]):
            for off, v in ((rm.X, x), (rm.Y, y), (rm.LAST_X, x), (rm.LAST_Y, y), (rm.VX, vx), (rm.VY, vy)):
                data[rm.offset(p + 1) + off] = v
    steps = []
    for _ in range(CASES[name]["steps"]):
        assert m.update(*hand_update(name)) == 1
        steps.append(snap(m))
    return m, steps


@functools.lru_cache(maxsize=None)
def hand_model(name):
    """the case on BodyModel, once: the model and the snapshot after every step; shared, never changed"""
    return hand_run(name)


# ---- the hand table
def test_the_table_reaches_what_it_is_for():
    plate = hand_model("plate")[1]
    assert plate[0]["sums"][0][0][1] != 0 and plate[0]["motions"][0][1] < 0.0   # pushed, and now on its way down
    hinge = hand_model("hinge")[1]
    assert hinge[0]["sums"][0][0][2] != 0 and hinge[-1]["spins"][0][2] < 0.0 and hinge[-1]["colliders"][0][4] < 0.0  # it tips
    assert hinge[-1]["colliders"][0][1:3] == (0.0, 0.0)                         # ... about its hinge
    ball = hand_model("ball")
    assert ball[0].collider_grips[WHITE] >= 2 and ball[1][0]["spins"][0][:2] == ball[1][0]["colliders"][0][1:3] != (0.0, 0.0)
    peg = hand_model("neighbour")[1][0]["colliders"][1]
    assert peg[1:3] == (42.0, -30.0)                                           # two sub-steps at 64 px/s
    assert hand_model("untouched")[1][-1]["sums"][0] == [(0, 0, 0)] * 2


@pytest.mark.parametrize("wrong", WRONG)
def test_a_wrong_rule_changes_a_case(wrong):
    assert CHANGED_BY[wrong]
    for name in CHANGED_BY[wrong]:  # (the cases named here; it may change others too)
        assert not all(same(a, b) for a, b in zip(hand_run(name, wrong)[1], hand_model(name)[1])), (wrong, name)


def test_every_wrong_rule_is_named():
    assert set(CHANGED_BY) == set(WRONG) and len(WRONG) >= 7


# ---- equality with today's step
FAR_PLATE, FAR_DISC = ("half_plane", 0.0, 1.0, -5000.0), ("disc", 2000.0, -3000.0, 5.0)


def _with_far_bodies(m, bodies):
    """tests/test_load_model.py's spin scene with two more colliders nothing reaches: a plate that moves and a disc that moves
    and spins about its own centre (so the turn it takes does not show in its geometry)"""
    colliders, surfaces, motions, spins, forces, _ = tlm.FLAVOURS["spin"]
    m.set_colliders(list(colliders) + [FAR_PLATE, FAR_DISC])
    m.set_forces(list(forces))
    m.set_collider_surfaces(list(surfaces) + [None, 0.3])
    m.set_collider_motion(list(motions) + [(7.0, -3.0), (-11.0, 5.0)])
    m.set_collider_spin(list(spins) + [(10.0, 20.0, 0.0), (2000.0, -3000.0, 0.7)])
    m.set_collider_loads(True)
    if bodies:
        m.set_collider_bodies([None] * len(colliders) + [(0.5, 0.0, 0.0, 0.0, 0.0, 0.0), (0.25, 0.125, 0.0, 0.0, 0.0, 0.0)])
    m.add(300.0, 300.0, 50, 15)
    return m


def test_untouched_bodies_at_one_sub_step_are_todays_step():
    """all bodies untouched, a = 0, drag = 0, S = 1: LoadModel with the same motions, bit for bit, step after step"""
    body = _with_far_bodies(tlm.flavour_model(True, BodyModel), True)
    load = _with_far_bodies(tlm.flavour_model(True, LoadModel), False)
    assert body.bodies_act()
    for k in range(3):
        body.update(tlm.H60, tlm.H60, 1, tlm.C)
        load.update(tlm.H60, tlm.H60, 1, tlm.C)
        assert same(snap(body), snap(load)), k
    assert min(body.collider_hits) > 0 and body.get_colliders()[-1][1:3] != FAR_DISC[1:3]


def test_without_a_body_any_step_is_todays_step():
    for bodies in ([], [None] * 7):
        body = _with_far_bodies(tlm.flavour_model(True, BodyModel), False)
        body.set_collider_bodies(bodies)
        load = _with_far_bodies(tlm.flavour_model(True, LoadModel), False)
        assert not body.bodies_act()
        for k in range(2):
            body.update(tlm.H60, tlm.H60, tlm.S, tlm.C)
            load.update(tlm.H60, tlm.H60, tlm.S, tlm.C)
            assert same(snap(body), snap(load)), k
    assert tlm.S > 1


def test_a_body_needs_loads_and_relaxed_order():
    m = BodyModel(*cc.hand_configs())
    hand_configure(m, "plate", loads=False)
    m.add(*cc.HAND_TARGET, cc.HAND_RADIUS, cc.HAND_RADIUS, 2, 2)
    before = snap(m)
    with pytest.raises(RuntimeError, match="set_collider_loads"):
        m.update(*hand_update("plate"))
    assert same(snap(m), before)
    m.set_colliders([FLOOR])  # the list resets the bodies
    assert m.get_collider_bodies() == [ZERO] and not m.has_body()
    assert m.update(*hand_update("plate")) >= 1  # (the refused update's time is still in the accumulator)
    assert normalise([None, (1, 2), (1, 2, -3, 4), (-0.0, 0, 0, -0.0, 0, 0)]) == \
        [ZERO, (1.0, 2.0, 0.0, 0.0, 0.0, 0.0), (1.0, 2.0, -3.0, 4.0, 0.0, 0.0), ZERO]
    assert str(normalise([(-0.0, 0.0)])[0][0]) == "0.0"


def test_a_failed_step_advances_nothing():
    m, steps = hand_run("plate")
    before = snap(m)

    def fails(*a, **k):
        raise FloatingPointError("a step that fails half way")

    held, m._post_solve = m._post_solve, fails
    with pytest.raises(FloatingPointError):
        m.update(*hand_update("plate"))
    m._post_solve = held
    after = snap(m)
    assert all(after[k] == before[k] for k in ("colliders", "motions", "spins", "sums"))


# ---- free fall
def test_an_untouched_body_follows_the_closed_loop():
    """rule 3 and rule 4 with J = 0, and rule 2 in front of them, computed here"""
    c = CASES["untouched"]
    (im, _, ax, ay, drag, _), (_, ii, _, _, _, sdrag) = c["bodies"]
    off, (vx, vy) = FLOOR[3], c["motions"][0]
    (x0, y0, x1, y1), (px, py, omega) = c["colliders"][1][1:5], c["spins"][1]
    turn = cayley(H64, omega)
    for _ in range(c["S"] * c["steps"]):
        off = off + (FLOOR[1] * (H64 * vx) + FLOOR[2] * (H64 * vy))
        vx = vx + 0.0 * im
        vy = vy + 0.0 * im
        vx = vx + H64 * ax
        vy = vy + H64 * ay
        f = 1.0 - H64 * drag
        vx, vy = vx * f, vy * f
        cs, sn = turn
        x0, y0 = px + (cs * (x0 - px) - sn * (y0 - py)), py + (sn * (x0 - px) + cs * (y0 - py))
        x1, y1 = px + (cs * (x1 - px) - sn * (y1 - py)), py + (sn * (x1 - px) + cs * (y1 - py))
        omega = (omega + 0.0 * ii) * (1.0 - H64 * sdrag)
        turn = cayley(H64, omega)
    last = hand_model("untouched")[1][-1]
    assert last["colliders"][0] == ("half_plane", 0.0, 1.0, off, "both") and last["motions"][0] == (vx, vy)
    assert last["colliders"][1] == ("segment", x0, y0, x1, y1, "both") and last["spins"][1] == (px, py, omega)
    assert 0.0 < omega < 4.0 and vy < 0.0


# ---- momentum balance
def test_a_plate_gains_the_momentum_the_loads_report():
    """drag = 0: v_end - v_start - (steps S h) a = inv_mass * the sum of the committed collider_loads() impulses, up to the
    roundings of both sides.  Per sub-step the model rounds J (two divisions), J inv_mass, h a and two additions: 6 operations;
    this side rounds the sum of the steps' impulses (steps), its product with inv_mass, (steps S h) a (3) and two subtractions.
    Every operation is off by at most half an ulp of its result, and no result exceeds `big`, so 2^-52 * big per operation
    bounds it with a factor of two to spare."""
    im, ay, S, steps = 0.004, 2000.0, 2, 6
    m = BodyModel(*cc.hand_configs())
    m.set_colliders([FLOOR])
    m.set_collider_loads(True)
    m.set_collider_bodies([(im, 0.0, 0.0, ay, 0.0, 0.0)])
    m.add(*cc.HAND_TARGET, cc.HAND_RADIUS, cc.HAND_RADIUS, 2, 2)
    for w, data in ((WHITE, m._white_data), (YOLK, m._yolk_data)):
        for p, (x, y) in enumerate(((16.0, -7.5), cc.REST) if cc.TESTED[w] == 0 else (cc.REST, (16.0, -7.5))):
            for off, v in ((rm.X, x), (rm.Y, y), (rm.LAST_X, x), (rm.LAST_Y, y), (rm.VX, 0.0), (rm.VY, 0.0)):
                data[rm.offset(p + 1) + off] = v
    total, big, touched = 0.0, 0.0, 0
    for _ in range(steps):
        assert m.update(S * H64, S * H64, S, 1) == 1
        jy = m.collider_loads()[0][1]
        touched += jy != 0.0
        total = total + jy
        big = max(big, abs(total) * im, abs(jy) * im, abs(m.get_collider_motion()[0][1]))
    assert touched >= 2 and m.collider_load_sums()[1] == 0
    v_end = m.get_collider_motion()[0][1]
    big = max(big, steps * S * H64 * ay)
    bound = (6 * steps * S + steps + 6) * 2.0 ** -52 * big
    residual = (v_end - 0.0 - (steps * S * H64) * ay) - im * total
    print("momentum balance: v_end = %.17g, residual = %.3g, bound = %.3g" % (v_end, residual, bound))
    assert abs(residual) <= bound


# ---- the plate experiment
GROUND = tlm.GROUND                     # keeps y <= 360 (y grows downwards)
G, PLATE_AT, STEPS = tlm.G, 225.0, 90   # the plate starts 25 px above the egg's top, at rest, and falls with the egg's gravity


def plate_run(inv_mass, steps=STEPS):
    m = BodyModel()
    m.set_colliders([("half_plane", 0.0, 1.0, PLATE_AT), GROUND])   # the plate keeps y >= its offset + r
    m.set_forces([("uniform", 0.0, G)])
    m.set_collider_loads(True)
    m.set_collider_bodies([(inv_mass, 0.0, 0.0, G), None])
    m.add(300.0, 300.0, 50, 15)
    series = []
    for _ in range(steps):
        m.update(tlm.H60, tlm.H60, tlm.S, tlm.C)
        series.append((m.get_colliders()[0][3], m.get_collider_motion()[0][1]))
    return m, series


def egg_mass(m):
    return sum(float(np.sum(1.0 / np.asarray(m.field(w, rm.INV_MASS), dtype=np.float64))) for w in (WHITE, YOLK))


def test_a_plate_laid_on_an_egg_is_held_up_by_it():
    probe = BodyModel()
    probe.add(300.0, 300.0, 50, 15)
    mass = egg_mass(probe)
    m, series = plate_run(1.0 / mass)  # a plate as heavy as the egg
    h = tlm.H60 / tlm.S
    off, v = PLATE_AT, 0.0
    for _ in range(STEPS * tlm.S):  # the plate nothing holds: rule 2, then rule 3 with J = 0
        off = off + 1.0 * (h * v)
        v = v + h * G
    rest, speed = series[-1]
    print("plate experiment: egg mass %.6g, plate mass %.6g, after %d steps the plate is at y = %.4f (free fall: %.1f), speed %.4g px/s"
          % (mass, mass, STEPS, rest, off, speed))
    assert rest < off  # higher: y grows downwards
    assert sum(m.collider_hits) > 0
    slack = 1e-9  # (a few ulps of a coordinate near 400, which are 6e-14)
    for w in (WHITE, YOLK):
        y, r = np.asarray(m.field(w, rm.Y)), np.asarray(m.field(w, rm.RADIUS))
        assert np.all(y - r >= rest - slack) and np.all(y + r <= 364.0 + slack), w
