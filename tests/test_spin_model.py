"""tests/spin_model.py, the definition of collider spin ("Collider spin"), against what the
definition promises: a list that does not turn is the motion model bit for bit, a hand table of tiny batches in which every
kind turns and every branch is reached (tests/test_gpu_collider_spin.py runs the same table on the device), nine wrong
rules that each change a case, the angles' sines and cosines are libm's, the whisk experiment -- a wall the caller re-sets
step by step passes through an egg, the same wall with a spin carries it -- and a roller that drags an egg sideways.  No
device needed.

The hand cases use the tiny batch of tests/test_collider_census.py: two particles per type of radius 2, no damping, no
follow constraint, h = 1 / 64.  White particle 0 and yolk particle 1 are under test; their mates rest at REST, which no
collider of the table moves.  omega = 16 rad/s is a quarter of a radian per sub-step."""
import ctypes
import functools
import math

import numpy as np
import pytest

import test_collider_census as cc
from motion_model import MotionModel
from relaxed_model import rm
from spin_model import WRONG, SpinModel, angle, pivot, primed

WHITE, YOLK = 0, 1
H64 = cc.H64
ONE, TWO = (H64, H64, 1, 1), (2 * H64, 2 * H64, 2, 1)  # update(): one sub-step of one pass; two sub-steps
W = 16.0                                  # rad/s: 0.25 rad per sub-step
BLADE = ("wall", 0.0, 0.0, 16.0, 0.0)     # a wall from its pivot (0, 0) along +x: a0 > 0 is the side y > 0
BAR = ("segment", 0.0, 0.0, 16.0, 0.0)
PADDLE = ("wall", -8.0, 0.0, 8.0, 0.0)    # ... turning about (0, -4) while it moves
FLOOR = ("half_plane", 0.0, 1.0, -10.0)   # keeps y >= -10 + r; tilts about (0, -10)
ROLLER = ("disc", 0.0, 0.0, 3.0)          # spins about its own centre
MOON = ("disc", 8.0, 0.0, 1.5)            # orbits (0, 0)
PAN = ("container", 0.0, 20.0, 30.0)      # holds the mates too; its centre orbits (0, 0)
STICK, SLIDE = 8.0, 0.5
O = (0.0, 0.0)


def _case(collider, spin, prev, vel=(0.0, 0.0), motion=None, surface=None, update=ONE, steps=1, want=(), final=None, absent=()):
    return dict(collider=collider, spin=spin, prev=prev, vel=vel, motion=motion, surface=surface, update=update, steps=steps,
                want=set(want) | {"turning"}, final=final, absent=set(absent))


# name: the collider, its spin (px, py, omega), the tested particle's start and velocity; `want` labels it must carry,
# `absent` labels it must not, `final` its position after the last step where that has a closed form
CASES = {
    # the blade turns a quarter radian up over a particle at rest 1 px above it: at x = 8 it is then 2.04 px up
    "whisk_ccw": _case(BLADE, O + (W,), (8.0, 1.0), want={"catch_pos"}),
    "whisk_cw": _case(BLADE, O + (-W,), (8.0, -1.0), want={"catch_neg"}),
    "turning_away": _case(BLADE, O + (-W,), (8.0, 3.0), want={"same_side", "wall_miss"}, final=(8.0, 3.0)),
    # a particle that goes round with the blade, 1 px in front of it: never caught
    "with_the_blade": _case(BLADE, O + (W,), (8.0, 1.0), vel=(-16.0, 128.0), want={"same_side"}, absent={"catch_pos", "catch_neg", "round"}),
    # 20 px out: the blade's line passes it, 4 px beyond the tip
    "beyond_the_tip": _case(BLADE, O + (W,), (20.0, 2.0), want={"round", "wall_miss"}, final=(20.0, 2.0)),
    # at the pivot, which is the blade's end: carried to the pivot itself, a0 == 0 exactly; the end then pushes it out
    "at_the_pivot": _case(BLADE, O + (W,), (0.0, 0.0), want={"no_side", "wall_hit"}),
    # a paddle that moves 1 px a sub-step while it turns about a pivot 4 px below its middle
    "paddle": _case(PADDLE, (0.0, -4.0, W), (4.0, 0.5), motion=(64.0, 0.0), want={"catch_pos"}),
    "paddle_twice": _case(PADDLE, (0.0, -4.0, W), (4.0, 2.5), motion=(64.0, 0.0), update=TWO, want={"same_side", "wall_hit"}),
    # two sub-steps, a particle that goes round with the blade, 3 px behind it: never caught (a carry by the whole angle of t
    # would put the second sub-step's start in front of the blade, and catch it)
    "behind_the_blade_twice": _case(BLADE, O + (W,), (12.0, -2.5), vel=(40.0, 192.0), update=TWO, want={"same_side", "wall_miss"},
                                    final=(13.25, 3.5), absent={"catch_pos", "catch_neg", "round", "wall_hit"}),
    # two sub-steps: the blade is 2.04 px up at x = 8, then 4.37; a particle at rest at 4.3 is passed in the second only
    "second_sub_step": _case(BLADE, O + (W,), (8.0, 4.3), update=TWO, want={"same_side", "wall_miss", "catch_pos"}),
    # two steps: the second starts from the committed blade, a quarter radian up
    "second_step": _case(BLADE, O + (W,), (8.0, 4.3), steps=2, want={"same_side", "catch_pos"}),
    "bar_hit": _case(BAR, O + (W,), (8.0, 3.5), want={"segment_hit"}, absent={"catch_pos", "catch_neg"}),
    "bar_miss": _case(BAR, O + (W,), (8.0, 8.0), want={"segment_miss"}, final=(8.0, 8.0)),
    # a floor that tilts an eighth of a radian about the point below the origin: up on the right, down on the left
    "tilting_floor": _case(FLOOR, (0.0, -10.0, W / 2), (16.0, -7.5), want={"half_plane_hit"}, absent={"stick", "slide"}),
    "tilting_floor_stick": _case(FLOOR, (0.0, -10.0, W / 2), (16.0, -7.5), surface=STICK, want={"half_plane_hit", "stick"}),
    "tilting_floor_slide": _case(FLOOR, (0.0, -10.0, W / 2), (16.0, -7.5), surface=1 / 64, want={"half_plane_hit", "slide"}),
    "tilting_floor_clear": _case(FLOOR, (0.0, -10.0, W / 2), (-16.0, -7.5), want={"half_plane_miss"}, final=(-16.0, -7.5)),
    # a disc that spins about its own centre keeps its geometry; the particle sinks 0.5 px into it at (0, 4.5) and comes out
    # at (0, 5), where the surface runs at -omega 5 = -80 px/s: 1.25 px a sub-step
    "roller_smooth": _case(ROLLER, O + (W,), (0.0, 4.5), want={"disc_hit"}, final=(0.0, 5.0), absent={"stick", "slide"}),
    "roller_stick": _case(ROLLER, O + (W,), (0.0, 4.5), surface=STICK, want={"disc_hit", "stick"}, final=(-1.25, 5.0)),
    "roller_slide": _case(ROLLER, O + (W,), (0.0, 4.5), surface=SLIDE, want={"disc_hit", "slide"}, final=(-0.25, 5.0)),
    # the surface's own velocity and the spin add up: 80 - 80 is a surface at rest where it touches, and nothing to grip
    "roller_cancels": _case(ROLLER, O + (W,), (0.0, 4.5), surface=(STICK, 80.0, 0.0), want={"disc_hit"}, final=(0.0, 5.0),
                            absent={"stick", "slide"}),
    "moon_hit": _case(MOON, O + (W,), (8.0, 4.0), want={"disc_hit"}),
    "moon_miss": _case(MOON, O + (W,), (8.0, -5.0), want={"disc_miss"}, final=(8.0, -5.0)),
    "pan_hit": _case(PAN, O + (W,), (24.0, 20.0), want={"container_hit"}),
    "pan_miss": _case(PAN, O + (W,), (0.0, 20.0), want={"container_miss"}, final=(0.0, 20.0)),
    # a spin of zero beside a motion: MotionModel's case "sweep_from_the_left", through the model with spins set
    "no_spin_beside": _case(("wall", 0.0, -8.0, 0.0, 8.0), (5.0, 5.0, 0.0), (3.0, 0.0), motion=(256.0, 0.0), want={"catch_neg"}, final=(6.0, 0.0),
                            absent={"turning"}),
}
CASES["no_spin_beside"]["want"].discard("turning")
EVERY_LABEL = {"turning", "catch_pos", "catch_neg", "round", "same_side", "no_side", "wall_hit", "wall_miss", "stick", "slide"} | {
    k + e for k in ("half_plane", "disc", "container", "segment") for e in ("_hit", "_miss")}


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
    if c["motion"] is not None:
        o.set_collider_motion([c["motion"]])
    o.set_collider_spin([c["spin"]])


def hand_run(name, wrong=None, snapshot=None):
    """the case on the model; returns (model, batch id, what `snapshot(model)` returned after every step)"""
    c = CASES[name]
    m = SpinModel(*cc.hand_configs(), wrong=wrong)
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
        mate = 1 - cc.TESTED[w]
        assert tuple(m.state(w)[:2, mate]) == cc.REST, (name, w)
    assert m.pair_solves == 0
    return m


# ---- a list that does not turn
def test_all_spins_zero_is_the_motion_model_bit_for_bit():
    """test_motion_model's sweep, with explicit zero spins (a pivot set, omega -0.0), against MotionModel itself"""
    a, b = MotionModel(), SpinModel()
    for m in (a, b):
        m.add(300.0, 300.0, 50, 15)
        m.set_colliders([("wall", 240.0, 0.0, 240.0, 600.0), ("disc", 300.0, 420.0, 30.0)])
        m.set_collider_surfaces([0.5, None])
        m.set_collider_motion([(540.0, 0.0), None])
    b.set_collider_spin([(7.0, -3.0, -0.0), None])
    assert b.get_collider_spin() == [(7.0, -3.0, 0.0), (0.0, 0.0, 0.0)] and not b.turning()
    for _ in range(12):
        a.update(1 / 60, 1 / 60, 2, 3)
        b.update(1 / 60, 1 / 60, 2, 3)
    for w in (WHITE, YOLK):
        assert np.array_equal(a.state(w), b.state(w))
    assert cc.counters(a) == cc.counters(b) and min(a.wall_catches) > 0
    assert a.colliders == b.colliders and b.get_collider_spin() == [(7.0, -3.0, 0.0), (0.0, 0.0, 0.0)]
    assert a.labels == b.labels


def test_a_collider_without_spin_beside_one_that_turns_takes_the_motion_rule():
    """omega == 0 is a branch per collider: its collider goes through motion_model.project, whatever the others do"""
    import motion_model as mm
    import spin_model as spm
    import wall_model as wm
    rng = np.random.default_rng(7)
    col = wm.normalise([("half_plane", 0.3, 1.0, -2.0), ("wall", -3.0, 1.0, 5.0, 2.0), ("disc", 1.0, 2.0, 1.5), ("container", 0.0, 0.0, 9.0)])
    x, y, px, py = (rng.uniform(-8, 8, 64) for _ in range(4))
    r = np.full(64, 2.0)
    surfaces = [(0.5, 3.0, -2.0)] * 4
    motions = [(3.0, 1.0), (-20.0, 40.0), (0.0, 0.0), (1.0, 1.0)]
    a = mm.project(x, y, r, px, py, 1 / 120, 3 / 120, col, surfaces, motions, 1)
    b = spm.project(x, y, r, px, py, 1 / 120, 3 / 120, 2 / 120, col, surfaces, motions, [(1.0, 2.0, 0.0)] * 4, 1)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:6] == b[2:6] and a[5] > 0 and a[3] > 0
    # ... and c = 1, s = 0 through the spin rule is NOT that: the expressions differ in their roundings
    ident = spm.primed(col[2], (0.1, 0.7), (0.3, 0.9, 1.0), 0.3, (1.0, 0.0))
    assert ident[1:3] != mm.primed(col[2], (0.1, 0.7), 0.3)[1:3] or ident[1] == 1.0 + 0.3 * 0.1


# ---- the hand table
@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_case(name):
    assert_hand_labels(name)


def test_the_table_reaches_every_label_and_turns_every_kind():
    got, kinds = set(), set()
    for name in CASES:
        m = hand_model(name)[0]
        for w in (WHITE, YOLK):
            got |= m.labels_of(w, cc.TESTED[w])
        if CASES[name]["spin"][2] != 0.0:
            kinds.add(CASES[name]["collider"][0])
    assert got == EVERY_LABEL, (got ^ EVERY_LABEL)
    assert kinds == {"half_plane", "disc", "container", "segment", "wall"}


def test_the_whisk_case_by_hand():
    """the first case in Python floats, in the order of the definition"""
    h, r = H64, 2.0
    t, ts = float(0 + 1) * h, float(0) * h
    c, s = math.cos(t * W), math.sin(t * W)
    ch, sh = math.cos(h * W), math.sin(h * W)
    Px, Py = 0.0 + t * 0.0, 0.0 + t * 0.0
    x0, y0 = Px + (c * 0.0 - s * 0.0), Py + (s * 0.0 + c * 0.0)
    x1, y1 = Px + (c * 16.0 - s * 0.0), Py + (s * 16.0 + c * 0.0)
    assert (x0, y0) == (0.0, 0.0) and (x1, y1) == (16.0 * c, 16.0 * s)
    ux, uy = 8.0 - (0.0 + ts * 0.0), 1.0 - (0.0 + ts * 0.0)
    pvx, pvy = Px + (ch * ux - sh * uy), Py + (sh * ux + ch * uy)
    ex, ey = x1 - x0, y1 - y0
    a0 = ex * (pvy - y0) - ey * (pvx - x0)
    a1 = ex * (1.0 - y0) - ey * (8.0 - x0)
    assert a0 > 0.0 and a1 < 0.0  # the carried start is above the blade, 1 px as before it turned; the particle is below it now
    assert abs(a0 - 16.0) < 1e-12
    l2 = ex * ex + ey * ey
    tq = ((8.0 - x0) * ex + (1.0 - y0) * ey) / l2
    qx, qy = x0 + tq * ex, y0 + tq * ey
    ln = math.sqrt(l2)
    want = (qx + ((-ey) / ln) * (0.0 + r), qy + (ex / ln) * (0.0 + r))
    m = hand_model("whisk_ccw")[0]
    assert xy_of_tested(m, WHITE) == want == xy_of_tested(m, YOLK)
    assert m.wall_catches == [1, 1] and m.collider_hits == [1, 1]
    # a radius above the turned blade
    assert abs((ex * (want[1] - y0) - ey * (want[0] - x0)) / ln - 2.0) < 1e-12


def test_a_roller_that_sticks_drags_by_h_omega_times_the_lever():
    m = hand_model("roller_stick")[0]
    for w in (WHITE, YOLK):
        assert xy_of_tested(m, w) == (0.0 - H64 * (W * (5.0 - 0.0)), 5.0)
    assert m.collider_grips == [1, 1] and m.grip_sticks == [1, 1]
    assert m.get_colliders() == [("disc", 0.0, 0.0, 3.0, "both")] and m.get_collider_spin() == [(0.0, 0.0, W)]  # (its geometry stays)


def test_the_commit_is_the_last_sub_steps_geometry_and_pivot():
    """get_colliders and get_collider_spin after a step are the expressions with t = S h; the second step starts from them"""
    _, _, snaps = hand_run("second_step", snapshot=lambda m: (m.get_colliders(), m.get_collider_spin()))
    c1, s1 = math.cos(H64 * W), math.sin(H64 * W)
    assert snaps[0] == ([("wall", 0.0, 0.0, 16.0 * c1, 16.0 * s1, "both")], [(0.0, 0.0, W)])
    x1, y1 = snaps[0][0][0][3:5]
    assert snaps[1] == ([("wall", 0.0, 0.0, 0.0 + (c1 * x1 - s1 * y1), 0.0 + (s1 * x1 + c1 * y1), "both")], [(0.0, 0.0, W)])
    # with a motion the pivot rides along; not dyadic: the commit is primed() at S h, bit for bit, and the spin persists
    m = SpinModel()
    m.set_colliders([("disc", 1.0, 2.0, 3.0), ("segment", 0.1, 0.2, 0.3, 0.4, "white"), ("half_plane", 0.6, 0.8, 5.0)])
    m.set_collider_surfaces([0.25, None, None])
    m.set_collider_motion([(0.1, -0.7), None, (3.0, 4.0)])
    m.set_collider_spin([(10.0, 20.0, 2.0), None, (-5.0, 9.0, -3.0)])
    before = list(m.colliders)
    m.add(300.0, 300.0, 50, 15)
    m.update(1 / 60, 1 / 60, 2, 3)
    h = max((1 / 60) / 2, rm.EPS)
    t = float(2) * h
    assert m.colliders[0] == primed(before[0], (0.1, -0.7), (10.0, 20.0, 2.0), t, (math.cos(t * 2.0), math.sin(t * 2.0)))
    assert m.colliders[1] == before[1]
    assert m.colliders[2] == primed(before[2], (3.0, 4.0), (-5.0, 9.0, -3.0), t, (math.cos(t * -3.0), math.sin(t * -3.0)))
    assert m.get_collider_spin() == [(10.0 + t * 0.1, 20.0 + t * -0.7, 2.0), (0.0, 0.0, 0.0), (-5.0 + t * 3.0, 9.0 + t * 4.0, -3.0)]
    assert m.get_collider_motion() == [(0.1, -0.7), (0.0, 0.0), (3.0, 4.0)] and m.surfaces[0] == (0.25, 0.0, 0.0)
    # the pivot's signed distance to the plane is kept
    (_, nx, ny, off, _, _), (px, py, _) = m.colliders[2], m.get_collider_spin()[2]
    assert abs((nx * px + ny * py - off) - (0.6 * -5.0 + 0.8 * 9.0 - 5.0)) < 1e-12
    m.set_collider_surfaces([])
    m.set_collider_motion([])
    assert m.get_collider_spin()[0][2] == 2.0
    m.set_colliders([("disc", 1.0, 2.0, 3.0)])
    assert m.get_collider_spin() == [(0.0, 0.0, 0.0)]


# ---- the host's sines and cosines
def test_math_cos_and_sin_are_libms_on_the_angles_the_tests_use():
    libm = ctypes.CDLL("libm.so.6")
    for f in (libm.cos, libm.sin):
        f.restype, f.argtypes = ctypes.c_double, [ctypes.c_double]
    h60 = (1 / 60) / 2
    angles = [float(k) * H64 * w for k in (1, 2) for w in (W, -W, W / 2)]
    angles += [float(k) * h60 * w for k in (1, 2) for w in (2.0, -3.0, WHISK_OMEGA, ROLLER_OMEGA, 0.1, 1e-9, 700.0)]
    angles += [h60 * w for w in (WHISK_OMEGA, ROLLER_OMEGA)]
    for a in angles:
        assert math.cos(a) == libm.cos(a) and math.sin(a) == libm.sin(a), a
        assert angle(a) == (libm.cos(a), libm.sin(a))


# ---- wrong rules
CHANGED_BY = {
    "pivot_unmoved": ("paddle", "paddle_twice"),
    "angle_start": ("whisk_ccw", "tilting_floor", "moon_hit"),
    "sweep_unrotated": ("whisk_ccw", "whisk_cw"),
    "sweep_full_angle": ("behind_the_blade_twice",),
    "friction_ignores_spin": ("roller_stick", "roller_slide", "tilting_floor_stick"),
    "friction_lever_prev": ("roller_stick", "tilting_floor_stick"),
    "half_plane_normal_fixed": ("tilting_floor", "tilting_floor_clear"),
    "commit_short": ("second_step",),
    "clockwise": ("whisk_ccw", "moon_hit", "pan_hit"),
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


# ---- the whisk experiment ("Collider spin")
PIVOT, REACH, START, WHISK_OMEGA, WHISK_STEPS = (300.0, 700.0), (300.0, 500.0), -0.25, 2.0, 18
# the egg's centre is 400 px from the pivot: 13.3 px a step there, 11.7 px at its near edge -- more than a particle's
# diameter (8 px) per step everywhere in the egg


def _blade(theta):
    """the wall from REACH[0] to REACH[1] px from the pivot, theta radians counter-clockwise of the direction to the egg"""
    dx, dy = math.sin(theta), -math.cos(theta)  # (theta = 0 points from the pivot at (300, 700) to the egg at (300, 300))
    return ("wall", PIVOT[0] + REACH[0] * dx, PIVOT[1] + REACH[0] * dy, PIVOT[0] + REACH[1] * dx, PIVOT[1] + REACH[1] * dy)


def behind_of(m, wall):
    """how many particles lie on the side the wall came from (counter-clockwise positive: the side a0 < 0 of a wall that
    points away from the pivot), and how many lie outside its span"""
    x0, y0, x1, y1 = wall
    ex, ey = x1 - x0, y1 - y0
    behind = out = 0
    for w in (WHITE, YOLK):
        x, y = m.state(w)[:2]
        a = ex * (y - y0) - ey * (x - x0)
        tc = ((x - x0) * ex + (y - y0) * ey) / (ex * ex + ey * ey)
        behind += int(np.count_nonzero(a < 0.0))
        out += int(np.count_nonzero((tc < 0.0) | (tc > 1.0)))
    return behind, out


@functools.lru_cache(maxsize=None)
def whisk(turning, omega=WHISK_OMEGA, steps=WHISK_STEPS):
    """one default egg at rest at its target (300, 300) and a wall on a ray from the pivot (300, 700), from 300 to 500 px out,
    that starts a quarter radian clockwise of the egg, clear of it, and turns through it.  turning: the wall has that spin;
    otherwise the caller sets a wall at rest anew before every step, at the pose the turning one ends that step.  Returns the
    model and, per step, (particles behind the wall after it, particles outside its span, the wall)."""
    m = SpinModel()
    m.add(300.0, 300.0, 50, 15)
    start = _blade(START)
    b0, out0 = behind_of(m, start[1:])
    assert (b0, out0) == (0, 0)
    for w in (WHITE, YOLK):  # clear of the egg: more than a radius from every particle
        x, y = m.state(w)[:2]
        ex, ey = start[3] - start[1], start[4] - start[2]
        assert ((ex * (y - start[2]) - ey * (x - start[1])) / math.hypot(ex, ey)).min() > 4.0 + 20.0
    if turning:
        m.set_colliders([start])
        m.set_collider_spin([PIVOT + (omega,)])
        poses = None
    else:
        poses = [c[2] for c in whisk(True, omega, steps)[1]]
    per_step = []
    for k in range(steps):
        if not turning:
            m.set_colliders([poses[k]])
        m.update(1 / 60, 1 / 60, 2, 3)
        wall = m.get_colliders()[0]
        per_step.append(behind_of(m, wall[1:5]) + (wall[:5],))
    return m, per_step


def test_whisk_a_wall_that_is_set_again_every_step_passes_through_the_egg():
    m, per_step = whisk(False)
    behind = [b for b, _, _ in per_step]
    print("re-set wall, omega %g: behind after the last step %d of 172, most behind %d, hits %s, catches %s" % (
        WHISK_OMEGA, behind[-1], max(behind), m.collider_hits, m.wall_catches))
    assert behind[-1] >= 86  # at least half the egg is left on the side the wall came from
    assert all(out == 0 for _, out, _ in per_step)


def test_whisk_a_turning_wall_carries_the_egg():
    m, per_step = whisk(True)
    behind = [b for b, _, _ in per_step]
    print("turning wall, omega %g: behind %s, hits %s, catches %s" % (WHISK_OMEGA, max(behind), m.collider_hits, m.wall_catches))
    assert behind == [0] * WHISK_STEPS
    assert all(out == 0 for _, out, _ in per_step)  # the whole egg stays inside the wall's span
    assert min(m.wall_catches) > 0
    for w in (WHITE, YOLK):
        assert np.isfinite(m.state(w)).all()
    # the wall has crossed the place the egg rested at: it is past the direction to (300, 300) by more than the egg's width
    wall = per_step[-1][2]
    theta = math.atan2(wall[3] - wall[1], -(wall[4] - wall[2]))
    assert theta > 0.25 and abs(theta - (START + WHISK_STEPS * WHISK_OMEGA / 60)) < 1e-9
    # the speed of the wall at the egg's near edge exceeds a particle's diameter per step
    assert (400.0 - 50.0) * WHISK_OMEGA / 60 > 8.0
    # every particle is a radius in front of it
    x0, y0, x1, y1 = wall[1:]
    for w in (WHITE, YOLK):
        x, y = m.state(w)[:2]
        assert ((x1 - x0) * (y - y0) - (y1 - y0) * (x - x0)).min() / math.hypot(x1 - x0, y1 - y0) >= 4.0 - 1e-9
    # the pivot does not move, the length of the wall drifts by roundings only
    assert m.get_collider_spin() == [PIVOT + (WHISK_OMEGA,)]
    assert abs(math.hypot(x1 - x0, y1 - y0) - 200.0) < 1e-9


# ---- the roller
ROLLER_OMEGA, ROLLER_STEPS, GRAVITY = 6.0, 30, 400.0
ROLLER_DISC = ("disc", 300.0, 470.0, 140.0)  # its top is at y = 330: the lowest fifth of the egg rests on it


@functools.lru_cache(maxsize=None)
def roller(mu, omega):
    """one default egg at (300, 300), no target pull beyond the default's, under a uniform force towards a large disc
    below it that spins about its own centre.  Returns (model, the centroid's x per step over both types)."""
    m = SpinModel()
    m.add(300.0, 300.0, 50, 15)
    m.set_forces([("uniform", 0.0, GRAVITY)])
    m.set_colliders([ROLLER_DISC])
    if mu:
        m.set_collider_surfaces([mu])
    m.set_collider_spin([ROLLER_DISC[1:3] + (omega,)])
    xs = []
    for _ in range(ROLLER_STEPS):
        m.update(1 / 60, 1 / 60, 2, 3)
        xs.append(float(np.concatenate([m.state(w)[0] for w in (WHITE, YOLK)]).mean()))
    return m, xs


def test_roller_a_spinning_disc_with_friction_moves_the_egg_sideways():
    spun, xs = roller(0.5, ROLLER_OMEGA)
    rest, xr = roller(0.5, 0.0)
    print("roller: centroid x after %d steps %.3f with omega %g, %.3f at rest; grips %s" % (ROLLER_STEPS, xs[-1], ROLLER_OMEGA, xr[-1],
                                                                                            spun.collider_grips))
    assert spun.collider_grips[WHITE] > 0
    # counter-clockwise positive in x/y: the top of the disc (smaller y) runs towards +x ... wx = -omega (y - Py), y < Py
    # Only the lowest fifth of the egg touches the disc and the follow constraint pulls the egg back, so the travel is small
    # against the surface's 14 px a step; without the spin's term in step 5c it is exactly zero (the test below).  Half a
    # pixel of the centroid is 86 px summed over the 172 particles.
    assert xs[-1] - xr[-1] > 0.5
    assert all(b - a > -1e-9 for a, b in zip(xr, xs))  # (never the other way)
    assert spun.get_colliders() == [ROLLER_DISC + ("both",)]  # the disc's geometry stays, step after step


def test_roller_without_friction_is_a_disc_at_rest_bit_for_bit():
    spun, xs = roller(0.0, ROLLER_OMEGA)
    rest, xr = roller(0.0, 0.0)
    assert spun.turning() and not rest.turning()
    for w in (WHITE, YOLK):
        assert np.array_equal(spun.state(w), rest.state(w))
    assert xs == xr and spun.collider_hits == rest.collider_hits and min(spun.collider_hits) > 0
    assert spun.collider_grips == [0, 0]


# ---- drift ("Collider spin": the limits)
def drift(steps=600, omega=2.0):
    """|n| - 1 of a half-plane and the length of a wall after `steps` committed steps of (1/60, 1/60, 2, 3) at omega"""
    m = SpinModel()
    m.set_colliders([("half_plane", 0.6, 0.8, 5.0), ("wall", 100.0, 380.0, 500.0, 380.0)])
    m.set_collider_spin([(20.0, -30.0, omega), (250.0, 300.0, omega)])
    for _ in range(steps):
        m.update(1 / 60, 1 / 60, 2, 3)
    (_, nx, ny, _, _, _), (_, x0, y0, x1, y1, _) = m.colliders
    return math.hypot(nx, ny) - 1.0, math.hypot(x1 - x0, y1 - y0) - 400.0


def test_drift_of_a_normal_and_of_a_walls_length_over_600_steps_is_roundings():
    dn, dl = drift()
    print("drift over 600 steps at 2 rad/s: |n| - 1 = %.3e, wall length - 400 = %.3e px" % (dn, dl))
    # per step a component of the normal takes three roundings of at most half an ulp of 1 each, and c c + s s is 1 to an
    # ulp: under 4 ulp a step.  An end point's coordinate stays below 1024 and takes at most four roundings a step: the
    # length moves by under 8 ulp(1024) a step.
    assert abs(dn) < 600 * 4 * 2.0 ** -53 and abs(dl) < 600 * 8 * 2.0 ** -53 * 1024.0
