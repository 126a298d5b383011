"""tests/contact_model.py, the definition of collider contacts ("Collider contacts"), against what the
definition promises: a hand table of tiny scenes (tests/test_gpu_collider_contacts.py runs the same table on the device),
eight wrong rules that each change a case, equality with BodyModel while contacts do not act, and the properties a user
expects -- a ball that lands on a floor and stays there, a ball a container keeps, balls that exchange their velocities, a seesaw that tips, and the free plate's
experiment with a ball in its place.  No device needed.

The hand scenes use the tiny batch of tests/test_collider_census.py as tests/test_body_model.py does: two particles per
type of radius 2, no damping, no follow constraint, h = 1 / 64; the particles under test rest at the case's `prev`."""
import functools
import math

import pytest

import test_body_model as tb
import test_collider_census as cc
import test_load_model as tlm
from contact_model import DEFAULT_ITERATIONS, OFF, WRONG, ContactModel, geometry, normalise
from relaxed_model import DIRS, rm

WHITE, YOLK = 0, 1
H64 = cc.H64
FAR = (40.0, 60.0)                                    # where the particles under test rest when the case wants none near
BALL = ("disc", 0.0, 0.0, 3.0)
FREE = (0.5, 0.02, 0.0, -100.0)                       # the ball's body: free, falling (y grows upwards in the hand scenes)
# every partner of rule 2, some 1.4 px from the ball: the rule first sees the pose one sub-step on, about 0.5 px away and closing
OTHERS = {
    "half_plane": ("half_plane", 0.0, 1.0, -4.4),
    "disc": ("disc", 0.5, -8.3, 4.0),
    "container": ("container", 30.0, 40.0, 54.5),   # (the particles rest inside it)
    "segment": ("segment", -8.0, -4.4, 8.0, -4.15),
    "wall": ("wall", -8.0, -4.5, 9.0, -4.3),
}


def _case(colliders, bodies, contacts, S=2, steps=2, iterations=DEFAULT_ITERATIONS, prev=FAR, motions=None, spins=None):
    return dict(colliders=list(colliders), bodies=list(bodies), contacts=list(contacts), iterations=iterations, prev=prev, S=S, steps=steps,
                surfaces=None, motions=motions, spins=spins)


CASES = {}
for _kind, _other in OTHERS.items():
    # the ball as b and as a, thrown at the partner; the partner is kinematic and at rest
    CASES["%s_then_ball" % _kind] = _case([_other, BALL], [None, FREE], [True, 0.25], motions=[None, (-30.0, -60.0)],
                                          spins=[None, (0.0, 0.0, 1.5)])
    CASES["ball_then_%s" % _kind] = _case([BALL, _other], [FREE, None], [0.25, True], motions=[(-30.0, -60.0), None],
                                          spins=[(0.0, 0.0, 1.5), None])
CASES.update({
    # two free balls head on, e = max(0.5, 1) = 1, one iteration
    "head_on": _case([("disc", -4.5, 0.0, 3.0), ("disc", 4.5, 0.5, 4.5)], [(0.5, 0.02), (0.25, 0.01)], [0.5, 1.0], iterations=1,
                     motions=[(50.0, 0.0), (-30.0, 3.0)], spins=[(-4.5, 0.0, 0.0), (4.5, 0.5, -2.0)]),
    # coincident centres, two apart in the list: DIRS[2]; the disc between them is off and overlaps both
    "coincident": _case([BALL, ("disc", 0.0, 0.0, 5.0), ("disc", 0.0, 0.0, 2.0)], [(0.5, 0.0), (1.0, 0.0), (1.0, 0.0)], [True, None, True], steps=1),
    # a ball that is exactly on a container's centre when the rule sees it (h v = (2, 2) to the bit), one apart: DIRS[1]; fast
    # enough to fire from there.  No particles: the container is smaller than the batch
    "centred": _case([("container", 0.0, 0.0, 4.5), ("disc", -2.0, -2.0, 3.0)], [None, (0.5, 0.0)], [True, True], S=1, steps=1, prev=None,
                     motions=[None, (128.0, 128.0)]),
    # a ball whose centre lies exactly on a segment: the segment's left normal
    "on_segment": _case([("segment", -6.0, -2.0, 6.0, 2.0), BALL], [None, (0.5, 0.0)], [True, True], S=1, steps=1),
    # ... and on a segment of no length: DIRS
    "on_point": _case([BALL, ("segment", 0.0, 0.0, 0.0, 0.0)], [(0.5, 0.0), None], [True, True], S=1, steps=1),
    # a ball that meets the end point of a segment obliquely, e = 1
    "end_point": _case([("segment", -20.0, -4.5, -3.2, -3.4), BALL], [None, FREE], [1.0, 0.0], motions=[None, (-40.0, -50.0)]),
    # a ball above a floor it does not reach in these steps: no pair fires
    "no_fire": _case([OTHERS["half_plane"], ("disc", 0.0, 30.0, 3.0)], [None, FREE], [True, True], spins=[None, (0.0, 30.0, 0.5)]),
    # no pairs at all: a free wall that falls through a half-plane, a ball whose partner is off, two kinematic colliders
    "non_pairs": _case([OTHERS["half_plane"], ("wall", -8.0, -3.0, 8.0, -3.0), BALL, ("disc", 40.0, -1.0, 3.0)],
                       [None, (0.5, 0.0, 0.0, -100.0), FREE, None], [True, True, None, True], motions=[None, (0.0, -50.0), (0.0, -50.0), (0.0, -50.0)]),
    # a wall hinged at its middle, at rest; a ball lands on its right arm, 5 px off the pivot
    "seesaw": _case([("wall", -10.0, -4.25, 10.0, -4.25), ("disc", 5.0, 0.0, 3.0)], [(0.0, 0.004), FREE], [True, True], steps=3,
                    motions=[None, (0.0, -48.0)], spins=[(0.0, -4.25, 0.0), (5.0, 0.0, 0.0)]),
    # a ball thrown into the corner of a floor and a side wall, past both in one sub-step: count = 2, and the mean of the two
    # leaves half of each overlap to the next iteration; four iterations and one
    "corner": _case([OTHERS["half_plane"], ("half_plane", 1.0, 0.0, -4.2), BALL], [None, None, FREE], [True, True, 0.5],
                    motions=[None, None, (-90.0, -110.0)]),
    "corner_once": _case([OTHERS["half_plane"], ("half_plane", 1.0, 0.0, -4.2), BALL], [None, None, FREE], [True, True, 0.5], iterations=1,
                         motions=[None, None, (-90.0, -110.0)]),
    # a ball on a floor between two balls that close in: count = 3, and the middle one takes three different impulses
    "squeezed": _case([("disc", -6.3, 0.2, 3.0), BALL, ("disc", 6.4, -0.3, 3.0), ("half_plane", 0.0, 1.0, -3.9)],
                      [(0.3, 0.0), FREE, (0.7, 0.0), None], [0.1, 0.2, 0.3, True], iterations=2,
                      motions=[(37.0, 1.0), (0.0, -52.3), (-53.0, 2.0), None]),
    # a ball that slides along the inside of a container at 200 px/s, 0.05 px from it when the rule first sees it: the gap bent
    # to the wall fires at once
    "sliding": _case([("container", 30.0, 40.0, 53.15), BALL], [None, FREE], [True, True], motions=[None, (160.0, -120.0)]),
    # a ball that comes down on a particle pair and on a floor at once: loads and contacts in one sub-step
    "with_particles": _case([OTHERS["half_plane"], BALL], [None, FREE], [True, True], prev=(4.0, -2.5), motions=[None, (0.0, -60.0)]),
})
CHANGED_BY = {
    "not_speculative": ("half_plane_then_ball", "head_on"),
    "target_without_max": ("head_on", "end_point"),
    "e_product": ("head_on", "ball_then_disc"),
    "not_averaged": ("corner", "squeezed"),
    "weight_no_rotation": ("seesaw",),
    "descending": ("squeezed",),
    "turn_stale": ("seesaw",),
    "wall_not_bent": ("sliding",),
}


def hand_configure(o, name, contacts=True):
    """the case's list on a model or a handle"""
    c = CASES[name]
    o.set_colliders(c["colliders"])
    if c["motions"] is not None:
        o.set_collider_motion(c["motions"])
    if c["spins"] is not None:
        o.set_collider_spin(c["spins"])
    o.set_collider_loads(True)
    o.set_collider_bodies(c["bodies"])
    if contacts:
        o.set_collider_contacts(c["contacts"], c["iterations"])


def hand_spots(name):
    tested, rest = (CASES[name]["prev"], (0.0, 0.0)), (cc.REST, (0.0, 0.0))
    return {w: [tested if p == cc.TESTED[w] else rest for p in (0, 1)] for w in (WHITE, YOLK)}


def hand_update(name):
    S = CASES[name]["S"]
    return (S * H64, S * H64, S, 1)


def snap(m):
    """tests/test_body_model.py's snap() and the counter"""
    return dict(tb.snap(m), solves=m.collider_contact_solves())


same = tb.same


def _plain(s):
    """a snapshot of this file without the counter, as tests/test_body_model.py's snap() has it"""
    return {k: v for k, v in s.items() if k != "solves"}


def hand_run(name, wrong=None, contacts=True, cls=ContactModel):
    m = cls(*cc.hand_configs()) if wrong is None else cls(*cc.hand_configs(), contact_wrong=wrong)
    hand_configure(m, name, contacts)
    if CASES[name]["prev"] is not None:  # (None: a case without particles)
        m.add(*cc.HAND_TARGET, cc.HAND_RADIUS, cc.HAND_RADIUS, 2, 2)
    for w, data in ((WHITE, m._white_data), (YOLK, m._yolk_data)):
        for p, ((x, y), (vx, vy)) in enumerate(hand_spots(name)[w] if CASES[name]["prev"] is not None else ()):
            for off, v in ((rm.X, x), (rm.Y, y), (rm.LAST_X, x), (rm.LAST_Y, y), (rm.VX, vx), (rm.VY, vy)):
                data[rm.offset(p + 1) + off] = v
    steps = []
    for _ in range(CASES[name]["steps"]):
        assert m.update(*hand_update(name)) == 1
        steps.append(snap(m) if contacts else tb.snap(m))
    return m, steps


@functools.lru_cache(maxsize=None)
def hand_model(name):
    """the case on ContactModel, once: the model and the snapshot after every step; shared, never changed"""
    return hand_run(name)


# ---- the hand table
def test_the_table_reaches_what_it_is_for():
    for kind in OTHERS:  # every shape pair fires, the ball as b and as a, and the ball turns round (e = 0.25)
        for name, ball in (("%s_then_ball" % kind, 1), ("ball_then_%s" % kind, 0)):
            m, steps = hand_model(name)
            assert steps[0]["solves"] > 0, name
            assert steps[0]["colliders"][1 - ball][1:5] == m.get_colliders()[1 - ball][1:5], name  # (a kinematic partner at rest stays)
            without = hand_run(name, contacts=False)[1]
            assert steps[-1]["motions"][ball] != without[-1]["motions"][ball], name
    # as a and as b the ball does the same up to the sign of n: here to the bit (two discs take the point on a's rim, which moves)
    for kind in sorted(set(OTHERS) - {"disc"}):
        one, two = hand_model("%s_then_ball" % kind)[1], hand_model("ball_then_%s" % kind)[1]
        assert [s["motions"][1] for s in one] == [s["motions"][0] for s in two] and [s["solves"] for s in one] == [s["solves"] for s in two], kind
    head = hand_model("head_on")[1]
    assert head[0]["solves"] == 1 and head[0]["motions"][0][0] < 0.0 < head[0]["motions"][1][0]
    co = hand_model("coincident")[1][0]
    assert co["solves"] > 0 and co["motions"][1] == (0.0, 0.0)                       # the disc that is off takes nothing
    assert co["motions"][0][0] == 0.0 and co["motions"][0][1] < 0.0 < co["motions"][2][1]  # along DIRS[2] = (0, 1)
    cen = hand_model("centred")[1][0]
    assert cen["solves"] > 0 and cen["motions"][1][0] == cen["motions"][1][1] < 128.0
    seg = hand_model("on_segment")[1][0]
    assert seg["solves"] > 0 and seg["motions"][1][0] < 0.0 < seg["motions"][1][1]      # the left normal of (12, 4) is (-4, 12) / l
    pt = hand_model("on_point")[1][0]
    assert pt["solves"] > 0 and pt["motions"][0][0] == pt["motions"][0][1] > 0.0        # pushed along DIRS[1]
    end = hand_model("end_point")[1]
    assert end[0]["solves"] > 0 and end[-1]["motions"][1][0] > -40.0 and end[-1]["motions"][1][1] > -50.0  # pushed along the oblique normal
    ex, ey = 16.8, 1.1
    assert ((0.0 - -20.0) * ex + (0.0 - -4.5) * ey) / (ex * ex + ey * ey) > 1.0         # (the closest point is the end point)
    quiet, plain = hand_model("no_fire")[1], hand_run("no_fire", contacts=False)[1]
    assert quiet[-1]["solves"] == 0 and all(tb.same(_plain(a), b) for a, b in zip(quiet, plain))
    none, bare = hand_model("non_pairs")[1], hand_run("non_pairs", contacts=False)[1]
    assert none[-1]["solves"] == 0 and all(tb.same(_plain(a), b) for a, b in zip(none, bare))
    assert none[-1]["colliders"][1][2] < -4.4 - 1.0                                     # the wall is through the half-plane
    saw = hand_model("seesaw")[1]
    assert saw[0]["solves"] > 0 and saw[-1]["spins"][0][2] < 0.0 and saw[-1]["spins"][0][:2] == (0.0, -4.25)  # the right arm goes down
    assert saw[-1]["colliders"][0][4] < -4.25 < saw[-1]["colliders"][0][2]
    assert hand_model("corner")[1][0]["solves"] > hand_model("corner_once")[1][0]["solves"] >= 2
    assert hand_model("squeezed")[1][0]["solves"] >= 3
    slide = hand_model("sliding")
    assert slide[1][0]["solves"] > hand_run("sliding", "wall_not_bent")[1][0]["solves"]  # (the bent gap fires where the straight one waits)
    both = hand_model("with_particles")[1]
    assert both[0]["solves"] > 0 and any(both[0]["sums"][0][1])
    assert {CASES[n]["iterations"] for n in CASES} >= {1, 4}
    assert any(0.0 in [c for c in CASES[n]["contacts"] if c is not None and c is not True] for n in CASES)  # e = 0 and e = 1
    assert any(1.0 in [c for c in CASES[n]["contacts"] if c is not None and c is not True] for n in CASES)


@pytest.mark.parametrize("wrong", WRONG)
def test_a_wrong_rule_changes_a_case(wrong):
    assert CHANGED_BY[wrong]
    for name in CHANGED_BY[wrong]:  # (the cases named here; it may change others too)
        assert not all(same(a, b) for a, b in zip(hand_run(name, wrong)[1], hand_model(name)[1])), (wrong, name)


def test_every_wrong_rule_is_named():
    assert set(CHANGED_BY) == set(WRONG) and len(WRONG) >= 7


def test_the_records_as_stored():
    assert normalise([None, True, 0.5, 0, 1, -0.0]) == [OFF, (0.0, 1), (0.5, 1), (0.0, 1), (1.0, 1), (0.0, 1)]
    m = ContactModel(*cc.hand_configs())
    hand_configure(m, "corner")
    assert m.get_collider_contacts() == ([(0.0, 1), (0.0, 1), (0.5, 1)], 4)
    m.set_collider_contacts([None, None, True], 0)  # 0 = the default
    assert m.get_collider_contacts() == ([OFF, OFF, (0.0, 1)], DEFAULT_ITERATIONS)
    m.set_colliders([BALL])                         # the list resets the records
    assert m.get_collider_contacts()[0] == [OFF] and not m.contacts_act()
    assert geometry(0, 1, ("wall", 0.0, 0.0, 1.0, 0.0, 3), ("half_plane", 0.0, 1.0, 0.0, 0.0, 3)) is None


# ---- contacts off: BodyModel to the bit
@pytest.mark.parametrize("contacts", [[], "off"])
def test_with_every_record_off_a_step_is_the_bodies_step(contacts):
    for name in sorted(tb.CASES):
        m = ContactModel(*cc.hand_configs())
        tb.hand_configure(m, name)
        m.set_collider_contacts([] if contacts == [] else [None] * len(tb.CASES[name]["colliders"]))
        assert not m.contacts_act()
        m.add(*cc.HAND_TARGET, cc.HAND_RADIUS, cc.HAND_RADIUS, 2, 2)
        for w, data in ((WHITE, m._white_data), (YOLK, m._yolk_data)):
            for p, ((x, y), (vx, vy)) in enumerate(tb.hand_spots(name)[w]):
                for off, v in ((rm.X, x), (rm.Y, y), (rm.LAST_X, x), (rm.LAST_Y, y), (rm.VX, vx), (rm.VY, vy)):
                    data[rm.offset(p + 1) + off] = v
        for want in tb.hand_model(name)[1]:
            assert m.update(*tb.hand_update(name)) == 1
            assert tb.same(tb.snap(m), want), name
        assert m.collider_contact_solves() == 0


def test_records_on_without_a_body_or_without_loads_do_not_act():
    m = ContactModel(*cc.hand_configs())
    m.set_colliders([OTHERS["half_plane"], BALL])
    m.set_collider_contacts([True, True])
    m.set_collider_loads(True)
    assert not m.contacts_act()          # no body
    m.set_collider_bodies([None, FREE])
    assert m.contacts_act()
    m.set_collider_loads(False)
    assert not m.contacts_act()          # (and a step raises, as with bodies alone)


def test_a_failed_step_advances_nothing():
    m, steps = hand_run("seesaw")
    before = snap(m)

    def fails(*a, **k):
        raise FloatingPointError("a step that fails half way")

    held, m._post_solve = m._post_solve, fails
    with pytest.raises(FloatingPointError):
        m.update(*hand_update("seesaw"))
    m._post_solve = held
    after = snap(m)
    assert all(after[k] == before[k] for k in ("colliders", "motions", "spins", "sums", "solves")) and before["solves"] > 0


# ---- the properties
DOWN = 980.0                                # y grows downwards in the egg's scenes
GROUND = tlm.GROUND                         # keeps y <= 364 - r
S, C, H60 = tlm.S, tlm.C, tlm.H60
RADIUS = 12.0
MASS_BALL = (1.0 / 40.0, 1.0 / 2880.0, 0.0, DOWN)
SPIN = 0.25  # every ball turns a little: the pivot of a body rides with it only while omega != 0 ("Collider bodies", step 2)


def _free_ball(colliders, bodies, contacts, motions, iterations=DEFAULT_ITERATIONS):
    """a model without particles; every disc spins about its own centre, as a free ball does"""
    m = ContactModel()
    m.set_colliders(colliders)
    m.set_collider_motion(motions)
    m.set_collider_spin([(c[1], c[2], SPIN) if c[0] == "disc" else None for c in colliders])
    m.set_collider_loads(True)
    m.set_collider_bodies(bodies)
    m.set_collider_contacts(contacts, iterations)
    return m


def _watch(m, steps, each):
    """runs `steps` steps of (S, C); each(m) is called after every sub-step's contacts, on the stored poses"""
    held = m._contacts

    def watched(h):
        held(h)
        each(m)

    m._contacts = watched
    for _ in range(steps):
        m.update(H60, H60, S, C)


def test_a_ball_lands_on_a_floor_and_stays():
    """no egg, e = 0, 120 steps: from the first fire on the gap after every sub-step is at least -1e-9 px (coordinates near 1e3
    round at about 1e-13: the bound sits four orders above), and the ball comes to rest: its speed ends below one sub-step of
    gravity.  The gap is read from the stored pose at the sub-step's end, which is where the sub-step before aimed."""
    m = _free_ball([GROUND, ("disc", 300.0, 200.0, RADIUS)], [None, MASS_BALL], [True, True], [None, None])
    seen = []
    _watch(m, 120, lambda mm: seen.append((mm.gaps()[(0, 1)], mm.collider_contact_solves() + mm._step_solves, mm.motions[1][1])))
    first = next(k for k, s in enumerate(seen) if s[1] > 0)
    gaps = [g for g, _, _ in seen[first:]]
    print("ball on a floor: first fire in sub-step %d of %d, min gap after it %.3g, last gap %.3g, last vy %.6g" %
          (first, len(seen), min(gaps), gaps[-1], seen[-1][2]))
    assert 0 < first < len(seen) - 100
    assert min(gaps) >= -1e-9
    fall = (H60 / S) * (H60 / S) * DOWN  # what gravity adds to h vn in a sub-step: a ball closer than that is stopped where it is
    assert -1e-9 <= gaps[-1] <= fall and gaps[-1] == gaps[-2 * S] and abs(m.get_collider_motion()[1][1]) == 0.0
    assert m.get_colliders()[1][2] <= 364.0 - RADIUS + 1e-9


def test_a_ball_in_a_container_stays_inside():
    """a ball that slides along the wall at some 400 px/s: the gap of rule 3 is bent to the circle, so the next pose's centre is
    at most R - r out; with a container's gap left at (R - r) - d it is 0.063 px beyond, (h vt)^2 / (2 d)"""
    R = 100.0
    m = _free_ball([("container", 300.0, 300.0, R), ("disc", 300.0, 300.0, RADIUS)], [None, MASS_BALL], [True, True], [None, (400.0, -50.0)])
    far = []

    def each(mm):
        c = mm.colliders[1]
        far.append(math.hypot(c[1] - 300.0, c[2] - 300.0))

    _watch(m, 120, each)
    print("ball in a container: farthest centre %.12f of %.1f allowed, %d fires" % (max(far), R - RADIUS, m.collider_contact_solves()))
    assert m.collider_contact_solves() > 0 and max(far) <= R - RADIUS + 1e-9


@pytest.mark.parametrize("e", [1.0, 0.0])
def test_head_on_balls(e):
    """two equal free balls, no gravity, head on along x.  e = 1: they exchange their velocities; e = 0: they end with equal
    velocities.  The summed momentum: a fire changes the two velocities by lam * n * inv_mass with the same lam, n and inv_mass and
    opposite signs, so the two additions round differently by at most half an ulp of the larger speed each, and the division by
    count = 1 is exact; with F fires the sum drifts by at most F * 2 * 2^-53 * vmax per component, doubled for the rounding of the
    sum itself."""
    v = 120.0
    m = _free_ball([("disc", 200.0, 300.0, RADIUS), ("disc", 260.0, 300.0, RADIUS)], [(0.025, 0.0), (0.025, 0.0)], [e, e], [(v, 0.0), (-v / 2, 0.0)])
    for _ in range(30):
        m.update(H60, H60, S, C)
    (ax, ay), (bx, by) = m.get_collider_motion()
    fires = m.collider_contact_solves()
    bound = 2.0 * (fires * 2.0 * 2.0 ** -53 * v)
    print("head-on e = %g: velocities %.17g, %.17g after %d fires; momentum off by %.3g (bound %.3g)" % (e, ax, bx, fires, (ax + bx) - v / 2, bound))
    assert fires > 0 and ay == 0.0 and by == 0.0
    assert abs((ax + bx) - v / 2) <= bound
    if e == 1.0:
        assert abs(ax - -v / 2) <= 1e-9 and abs(bx - v) <= 1e-9
    else:
        assert abs(ax - bx) <= 1e-9 and abs(ax - v / 4) <= 1e-9
    assert m.gaps()[(0, 1)] >= -1e-9


def test_a_ball_tips_a_seesaw():
    """a wall hinged at its middle (0, 1 / I), y downwards: a ball dropped on its right arm turns it clockwise on the screen,
    omega > 0 (x to y), and one dropped on the left arm the other way"""
    for side, sign in ((60.0, 1.0), (-60.0, -1.0)):
        m = _free_ball([("wall", 200.0, 340.0, 400.0, 340.0), ("disc", 300.0 + side, 300.0, RADIUS)], [(0.0, 1.0e-5), MASS_BALL], [True, True],
                       [None, None])
        m.set_collider_spin([(300.0, 340.0, 0.0), (300.0 + side, 300.0, SPIN)])
        for _ in range(30):
            m.update(H60, H60, S, C)
        omega = m.get_collider_spin()[0][2]
        print("seesaw, ball %+.0f px from the hinge: omega %.6g after %d fires" % (side, omega, m.collider_contact_solves()))
        assert m.collider_contact_solves() > 0 and omega * sign > 0.0
        assert m.get_collider_spin()[0][:2] == (300.0, 340.0)


def test_the_free_plate_experiment_with_a_ball():
    """tests/test_body_model.py's plate nothing holds is at off = 1321.4 after 90 steps.  A plate is a half-plane and meets no
    half-plane, so a ball stands in: from the plate's height, with the plate's gravity, it ends on the floor"""
    m = _free_ball([GROUND, ("disc", 300.0, tb.PLATE_AT, RADIUS)], [None, (1.0 / 40.0, 0.0, 0.0, tb.G)], [True, True], [None, None])
    m.set_forces([("uniform", 0.0, tb.G)])
    m.add(600.0, 300.0, 50, 15)  # (an egg beside it, which it never touches: the scene of the experiment)
    lowest = []
    for _ in range(tb.STEPS):
        m.update(H60, H60, S, C)
        lowest.append(m.get_colliders()[1][2] + RADIUS)
    print("free ball in place of the plate: lowest point %.9f after %d steps (the floor is at 364), %d fires" %
          (lowest[-1], tb.STEPS, m.collider_contact_solves()))
    assert m.collider_contact_solves() > 0 and max(lowest) <= 364.0 + 1e-9


def multi(scene, iterations, steps=60):
    """the corner and the ball between two balls of DESIGN.md: the deepest overlap of any pair over the run, and at its end"""
    if scene == "corner":
        m = _free_ball([GROUND, ("half_plane", 1.0, 0.0, 200.0), ("disc", 240.0, 320.0, RADIUS)], [None, None, MASS_BALL], [True] * 3,
                       [None, None, (-300.0, 100.0)], iterations)
    else:
        m = _free_ball([("disc", 250.0, 340.0, RADIUS), ("disc", 300.0, 340.0, RADIUS), ("disc", 350.0, 340.0, RADIUS), GROUND],
                       [MASS_BALL] * 3 + [None], [True] * 4, [(200.0, 0.0), None, (-200.0, 0.0), None], iterations)
    worst = []
    _watch(m, steps, lambda mm: worst.append(min(mm.gaps().values())))
    return min(worst), worst[-1], m.collider_contact_solves()


@pytest.mark.parametrize("scene", ["corner", "between"])
def test_multi_contact_scenes_are_recorded(scene):
    """no bound chosen in advance: what 1, 4 and 16 iterations leave is printed here and recorded in DESIGN.md"""
    for iterations in (1, 4, 16):
        deepest, last, fires = multi(scene, iterations)
        print("%s, %2d iterations: deepest gap %.6g px, gap at the end %.6g px, %d fires" % (scene, iterations, deepest, last, fires))
        assert fires > 0 and math.isfinite(deepest)
