"""tests/motion_model.py, the definition of collider motion ("Collider motion"), against what the
definition promises: a list at rest is the wall model bit for bit, a hand table of one-particle cases that each reach the
branch they are named for (tests/test_gpu_collider_motion.py runs the same table on the device), seven wrong rules that each
change a case, and the sweep experiment -- a wall the caller re-sets step by step passes through an egg, the same wall with
a motion carries it.  No device needed.

The hand cases use the tiny batch of tests/test_collider_census.py: two particles per type of radius 2, no damping, no
follow constraint, h = 1 / 64, so every coordinate below is a dyadic number and most results have a closed form.  White
particle 0 and yolk particle 1 are under test; their mates rest at REST, which no collider of the table reaches."""
import functools

import numpy as np
import pytest

import test_collider_census as cc
import test_wall_model as twm
from motion_model import WRONG, MotionModel, primed
from relaxed_model import rm

WHITE, YOLK = 0, 1
H64 = cc.H64
ONE, TWO = (H64, H64, 1, 1), (2 * H64, 2 * H64, 2, 1)  # update(): one sub-step of one pass; two sub-steps
V = ("wall", 0.0, -8.0, 0.0, 8.0)       # a vertical wall through the origin: a0 > 0 is the side x < x0
FLOOR = ("half_plane", 0.0, 1.0, -10.0)  # keeps y >= -10 + r
PAN = ("container", 0.0, 20.0, 30.0)     # holds the mates too
STICK, SLIDE = 8.0, 0.5


def _case(collider, motion, prev, vel=(0.0, 0.0), surface=None, update=ONE, steps=1, want=(), final=None, absent=()):
    return dict(collider=collider, motion=motion, prev=prev, vel=vel, surface=surface, update=update, steps=steps,
                want=set(want), final=final, absent=set(absent))


# name: the collider, its motion, the tested particle's start and velocity; `want` labels it must carry, `absent` labels it
# must not, `final` its position after the last step where that has a closed form
CASES = {
    # a wall at x = 0 that moves 4 px a sub-step over a particle at rest 3 px in front of it: caught, r in front of x = 4
    "sweep_from_the_left": _case(V, (256.0, 0.0), (3.0, 0.0), want={"catch_neg"}, final=(6.0, 0.0)),
    "sweep_from_the_right": _case(V, (-256.0, 0.0), (-3.0, 0.0), want={"catch_pos"}, final=(-6.0, 0.0)),
    "moving_away": _case(V, (-256.0, 0.0), (3.0, 0.0), want={"same_side", "wall_miss"}, final=(3.0, 0.0)),
    "with_the_wall": _case(V, (256.0, 0.0), (3.0, 0.0), vel=(256.0, 0.0), want={"same_side", "wall_miss"}, final=(7.0, 0.0)),
    # the sweep meets the wall's line beyond its end (tc = 1.25): the particle goes round
    "beyond_the_end": _case(V, (256.0, 0.0), (3.0, 12.0), want={"round", "wall_miss"}, final=(3.0, 12.0)),
    # the oblique wall of tests/test_wall_model.py moving down and right over a particle at rest below it
    "oblique": _case(("wall",) + twm.WALL, (64.0, -128.0), (1.25, 0.0), want={"catch_neg"}),
    # a floor that rises 2 px under a particle 1 px above it
    "rising_floor": _case(FLOOR, (0.0, 128.0), (0.0, -7.0), want={"half_plane_hit"}, final=(0.0, -6.0)),
    # a floor that slides along itself: n . v == 0, the geometry stays, the friction drags -- all of h v when it sticks
    "sliding_floor_stick": _case(FLOOR, (128.0, 0.0), (0.0, -9.0), surface=STICK, want={"half_plane_hit", "stick"}, final=(2.0, -8.0)),
    "sliding_floor_slide": _case(FLOOR, (128.0, 0.0), (0.0, -9.0), surface=SLIDE, want={"half_plane_hit", "slide"}, final=(0.5, -8.0)),
    "sliding_floor_smooth": _case(FLOOR, (128.0, 0.0), (0.0, -9.0), want={"half_plane_hit"}, final=(0.0, -8.0), absent={"stick", "slide"}),
    # a floor that only slides and does not reach the particle: nothing happens (|v| t is no offset)
    "sliding_floor_clear": _case(FLOOR, (128.0, 0.0), (0.0, -7.0), want={"half_plane_miss"}, final=(0.0, -7.0)),
    "disc": _case(("disc", 0.0, 0.0, 1.5), (128.0, 0.0), (5.0, 0.0), want={"disc_hit"}, final=(5.5, 0.0)),
    "container": _case(PAN, (0.0, 128.0), (0.0, -7.0), want={"container_hit"}, final=(0.0, -6.0)),
    # the surface's own velocity and the motion add up: (64, 0) + (64, 0) drags as (128, 0) does
    "surface_velocity_adds": _case(FLOOR, (64.0, 0.0), (0.0, -9.0), surface=(STICK, 64.0, 0.0), want={"stick"}, final=(2.0, -8.0)),
    # two sub-steps: the wall is at x = 4, then at x = 8; a particle at rest at x = 7 is passed in the second only
    "second_sub_step": _case(V, (256.0, 0.0), (7.0, 0.0), update=TWO, want={"same_side", "catch_neg"}, final=(10.0, 0.0)),
    # two sub-steps, a particle that follows the wall 3 px behind it: never caught (a carry by t v would catch it)
    "behind_the_wall_twice": _case(V, (256.0, 0.0), (-3.0, 0.0), vel=(256.0, 0.0), update=TWO, want={"same_side"}, final=(5.0, 0.0),
                                   absent={"catch_pos", "catch_neg", "round"}),
    # two steps: the second starts from the committed wall at x = 4; the particle, caught to x = 6, flies on at 192 px/s
    # to x = 9, 1 px in front of the wall now at x = 8, which pushes it on to x = 10
    "second_step": _case(V, (256.0, 0.0), (3.0, 0.0), steps=2, want={"catch_neg", "wall_hit"}, final=(10.0, 0.0)),
    # a floor that rises through two steps of two sub-steps: the particle rides it
    "rising_floor_two_steps": _case(FLOOR, (0.0, 128.0), (0.0, -7.0), update=TWO, steps=2, want={"half_plane_hit"}, final=(0.0, 0.0)),
}


def hand_spots(name):
    c = CASES[name]
    tested, rest = (c["prev"], c["vel"]), (cc.REST, (0.0, 0.0))
    return {w: [tested if p == cc.TESTED[w] else rest for p in (0, 1)] for w in (WHITE, YOLK)}


def hand_configure(o, name):
    """the case's list on a model or a handle"""
    c = CASES[name]
    o.set_colliders([c["collider"]])
    if c["surface"] is not None:
        o.set_collider_surfaces([c["surface"]])
    o.set_collider_motion([c["motion"]])


def hand_run(name, wrong=None, snapshot=None):
    """the case on the model; returns (model, batch id, what `snapshot(model)` returned after every step)"""
    c = CASES[name]
    m = MotionModel(*cc.hand_configs(), wrong=wrong)
    hand_configure(m, name)
    i = m.add(*cc.HAND_TARGET, cc.HAND_RADIUS, cc.HAND_RADIUS, 2, 2)
    for w, data in ((WHITE, m._white_data), (YOLK, m._yolk_data)):
        for p, ((x, y), (vx, vy)) in enumerate(hand_spots(name)[w]):
            for off, v in ((rm.X, x), (rm.Y, y), (rm.LAST_X, x), (rm.LAST_Y, y), (rm.VX, vx), (rm.VY, vy)):
                data[rm.offset(p + 1) + off] = v
    snaps = []
    for _ in range(c["steps"]):
        assert m.update(*c["update"]) == 1
        snaps.append(snapshot(m) if snapshot else None)
    return m, i, snaps


@functools.lru_cache(maxsize=None)
def hand_model(name):
    return hand_run(name)


def xy_of_tested(m, w):
    return tuple(float(v) for v in m.state(w)[:2, cc.TESTED[w]])


def assert_hand_labels(name):
    """the case reaches the branch it is named for, on the model, for the particle under test of either type"""
    m, _, _ = hand_model(name)
    c = CASES[name]
    for w in (WHITE, YOLK):
        got = m.labels_of(w, cc.TESTED[w])
        assert c["want"] <= got and not c["absent"] & got, (name, w, got)
        if c["final"] is not None:
            assert xy_of_tested(m, w) == c["final"], (name, w, xy_of_tested(m, w))
        assert np.isfinite(m.state(w)).all()
    assert m.pair_solves == 0
    return m


# ---- a list at rest
def test_all_motions_zero_is_the_wall_model_bit_for_bit():
    """the hold experiment of tests/test_wall_model.py with explicit zero motions, against WallModel itself"""
    a = twm.hold("wall")
    m = MotionModel()
    i = m.add(300.0, 300.0, 50, 15)
    m.set_colliders([("wall", 100.0, 380.0, 500.0, 380.0)])
    m.set_collider_motion([(0.0, -0.0)])
    assert m.get_collider_motion() == [(0.0, 0.0)] and not m.moving()
    for k in range(30):
        if k == 2:
            m.set_target_position(i, 300.0, 480.0)
        m.update(1 / 60, 1 / 60, 2, 3)
    for w in (WHITE, YOLK):
        assert np.array_equal(m.state(w), a.state(w))
    assert (m.collider_hits, m.collider_grips, m.wall_catches, m.pair_solves) == (a.collider_hits, a.collider_grips, a.wall_catches,
                                                                                   a.pair_solves)
    assert m.wall_catches == [202, 23] and m.colliders == a.colliders


def test_zero_motion_through_the_moving_arithmetic_is_the_wall_model_too():
    """t v == 0 and h v == 0 change no bit: the rule itself, with a motion of zero, is the wall rule"""
    import motion_model as mm
    import wall_model as wm
    rng = np.random.default_rng(5)
    col = wm.normalise([("half_plane", 0.3, 1.0, -2.0), ("wall",) + twm.WALL, ("disc", 1.0, 2.0, 1.5), ("container", 0.0, 0.0, 9.0)])
    x, y, px, py = (rng.uniform(-8, 8, 64) for _ in range(4))
    r = np.full(64, 2.0)
    surfaces = [(0.5, 3.0, -2.0)] * 4
    a = wm.project(x, y, r, px, py, 1 / 120, col, surfaces, 1)
    b = mm.project(x, y, r, px, py, 1 / 120, 3 / 120, col, surfaces, [(0.0, 0.0)] * 4, 1)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:6] == b[2:6] and a[5] > 0 and a[3] > 0


# ---- the hand table
@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_case(name):
    assert_hand_labels(name)


def test_the_wall_cases_by_hand():
    """the first case in Python floats, in the order of the definition"""
    h, vx, r = H64, 256.0, 2.0
    t = float(0 + 1) * h
    x0 = 0.0 + t * vx
    pvx = 3.0 + h * vx
    ex, ey = 0.0, 16.0
    a0 = ex * (0.0 - -8.0) - ey * (pvx - x0)
    a1 = ex * (0.0 - -8.0) - ey * (3.0 - x0)
    assert (x0, pvx, a0, a1) == (4.0, 7.0, -48.0, 16.0)
    u = a0 / (a0 - a1)
    hx = pvx + u * (3.0 - pvx)
    assert (u, hx) == (0.75, 4.0)
    assert ((hx - x0) * ex + (0.0 - -8.0) * ey) / 256.0 == 0.5
    assert xy_of_tested(hand_model("sweep_from_the_left")[0], WHITE) == (x0 + (ey / 16.0) * r, 0.0)
    m = hand_model("sweep_from_the_left")[0]
    assert m.wall_catches == [1, 1] and m.collider_hits == [1, 1]


def test_stick_on_a_moving_floor_moves_by_h_v():
    m = hand_model("sliding_floor_stick")[0]
    for w in (WHITE, YOLK):
        assert xy_of_tested(m, w)[0] - 0.0 == H64 * 128.0
    assert m.collider_grips == [1, 1] and m.grip_sticks == [1, 1]
    assert m.get_colliders() == [("half_plane", 0.0, 1.0, -10.0, "both")]  # (n . v == 0: the committed floor is the floor)


def test_the_commit_is_the_last_sub_steps_geometry():
    """get_colliders after step 1 is the expression with t = S h; the second step starts from it"""
    _, _, snaps = hand_run("second_step", snapshot=lambda m: m.get_colliders())
    assert snaps == [[("wall", 4.0, -8.0, 4.0, 8.0, "both")], [("wall", 8.0, -8.0, 8.0, 8.0, "both")]]
    _, _, snaps = hand_run("rising_floor_two_steps", snapshot=lambda m: m.get_colliders())
    assert snaps == [[("half_plane", 0.0, 1.0, -10.0 + (0.0 * 0.0 + 1.0 * (float(2) * H64 * 128.0)), "both")],
                     [("half_plane", 0.0, 1.0, -2.0, "both")]]
    # not a dyadic velocity: the commit is primed() at S h, bit for bit, and the motion persists
    m = MotionModel()
    m.set_colliders([("disc", 1.0, 2.0, 3.0), ("segment", 0.1, 0.2, 0.3, 0.4, "white")])
    m.set_collider_surfaces([0.25, None])
    m.set_collider_motion([(0.1, -0.7), None])
    before = list(m.colliders)
    m.add(300.0, 300.0, 50, 15)
    m.update(1 / 60, 1 / 60, 2, 3)
    h = max((1 / 60) / 2, rm.EPS)
    assert m.colliders == [primed(before[0], (0.1, -0.7), float(2) * h), before[1]]
    assert m.colliders[0][1:3] == (1.0 + (float(2) * h) * 0.1, 2.0 + (float(2) * h) * -0.7)
    assert m.get_collider_motion() == [(0.1, -0.7), (0.0, 0.0)] and m.surfaces == [(0.25, 0.0, 0.0), (0.0, 0.0, 0.0)]
    m.set_collider_surfaces([])
    assert m.get_collider_motion() == [(0.1, -0.7), (0.0, 0.0)]
    m.set_colliders([("disc", 1.0, 2.0, 3.0)])
    assert m.get_collider_motion() == [(0.0, 0.0)]


# ---- wrong rules
CHANGED_BY = {
    "sweep_uncarried": ("sweep_from_the_left", "with_the_wall"),
    "carry_t": ("behind_the_wall_twice",),
    "geometry_start": ("sweep_from_the_left", "rising_floor", "second_sub_step"),
    "friction_ignores_motion": ("sliding_floor_stick", "sliding_floor_slide"),
    "half_plane_speed": ("sliding_floor_clear", "sliding_floor_stick"),
    "commit_short": ("second_step", "rising_floor_two_steps"),
    "friction_carried_prev": ("sliding_floor_stick",),
}


def test_every_wrong_rule_is_named():
    assert sorted(CHANGED_BY) == sorted(WRONG)


@pytest.mark.parametrize("wrong", WRONG)
def test_a_wrong_rule_changes_a_case(wrong):
    """each wrong rule changes the final state of the cases listed for it -- and is not noise: the right rule run twice agrees"""
    for name in CHANGED_BY[wrong]:
        right, again, bad = hand_model(name)[0], hand_run(name)[0], hand_run(name, wrong=wrong)[0]
        assert all(np.array_equal(right.state(w), again.state(w)) for w in (WHITE, YOLK))
        assert any(not np.array_equal(right.state(w), bad.state(w)) for w in (WHITE, YOLK)) or right.colliders != bad.colliders, name
        assert xy_of_tested(bad, WHITE) != CASES[name]["final"] or right.colliders != bad.colliders, name


# ---- the sweep experiment ("Collider motion")
X0, SPEED, STEPS = 240.0, 540.0, 30  # 9 px a step, 4.5 px a sub-step: more than a particle's diameter (8 px) per step


def _wall_at(x):
    return ("wall", x, 0.0, x, 600.0)


@functools.lru_cache(maxsize=None)
def sweep(moving):
    """one default egg at its target (300, 300), all of it between x = 252 and x = 348, and a vertical wall from y = 0 to
    y = 600 that starts at x = 240, clear of it, and crosses it at 540 px/s.  moving: the wall has that motion; otherwise the
    caller sets a wall at rest anew before every step, where the moving one is at the end of that step.  Returns the model
    and, per step, how many particles lie behind the wall (x < the wall's) after it."""
    m = MotionModel()
    m.add(300.0, 300.0, 50, 15)
    lo = min(float(m.state(w)[0].min()) for w in (WHITE, YOLK))
    hi = max(float(m.state(w)[0].max()) for w in (WHITE, YOLK))
    assert X0 + 4.0 < lo and hi - lo > 90.0  # (clear of the egg, every particle in front of it)
    if moving:
        m.set_colliders([_wall_at(X0)])
        m.set_collider_motion([(SPEED, 0.0)])
    behind = []
    for k in range(STEPS):
        if not moving:
            m.set_colliders([_wall_at(X0 + (k + 1) * SPEED / 60)])
        m.update(1 / 60, 1 / 60, 2, 3)
        at = m.colliders[0][1]
        behind.append(sum(int(np.count_nonzero(m.state(w)[0] < at)) for w in (WHITE, YOLK)))
    assert m.colliders[0][1] > hi  # (the wall has crossed the egg's whole width)
    return m, behind


def test_sweep_a_wall_that_is_set_again_every_step_passes_through_the_egg():
    m, behind = sweep(False)
    print("re-set wall: behind after the last step %d of 172, most behind %d, hits %s, catches %s" % (behind[-1], max(behind), m.collider_hits,
                                                                                                  m.wall_catches))
    assert behind[-1] >= 1
    assert abs(m.colliders[0][1] - (X0 + STEPS * SPEED / 60)) < 1e-9


def test_sweep_a_moving_wall_carries_the_egg():
    m, behind = sweep(True)
    print("moving wall: behind %s, hits %s, catches %s, wall at %r" % (max(behind), m.collider_hits, m.wall_catches, m.colliders[0][1]))
    assert behind == [0] * STEPS
    assert min(m.wall_catches) > 0
    for w in (WHITE, YOLK):
        assert np.isfinite(m.state(w)).all()
        assert float(m.state(w)[0].min()) >= m.colliders[0][1] + 4.0 - 1e-9  # (a radius in front of it)
    h = (1 / 60) / 2
    x = X0
    for _ in range(STEPS):
        x = x + (float(2) * h) * SPEED
    assert m.colliders[0][1] == x
