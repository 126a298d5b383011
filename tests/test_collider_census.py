"""tests/collider_census.py -- which branch of steps 5b / 5c a particle takes -- and the scenes
tests/test_gpu_collider_edges.py runs on the device, checked here on the model alone.  No device needed.

  * the labels are right: on the HAND table and the edge applications of tests/test_wall_model.py the census names the
    branch those tests name;
  * recording is free: CensusModel and WallModel agree in every bit on every scene;
  * reach: every scene the device file runs reaches the labels it is there for, per type the collider covers and, for
    the scenes the device groups run, per batch;
  * sensitivity: wrong variants of the wall and the segment rule (VARIANTS) each change the final state of at least one
    of those scenes -- a kernel wrong in that way would fail the device file.

The scenes (the hand table CASES, the oblique wall, the oblique segment, the corner) are defined here and imported by the
device file.  Out of scope: NaN positions (a NaN cell fails the step before step 5b matters), the force step.  The
pair loop has a census of its own: tests/pair_census.py, tests/test_pair_census.py, tests/test_gpu_pair_edges.py."""
import functools

import numpy as np
import pytest

import surface_model as sm
import test_wall_model as twm
import wall_model as wm
from cohesion_model import CohesiveModel
from collider_census import CensusModel, classify
from relaxed_model import DIRS, rm
from test_gpu_collider_walls import _model as _configured_model
from wall_model import WallModel

WHITE, YOLK = 0, 1
GRIPS = {"stick", "slide", "no_tangent", "smooth", "caught_stick", "caught_slide", "caught_no_tangent", "caught_smooth"}


def same_state(a, b):
    return all(np.array_equal(a.state(w), b.state(w)) for w in (WHITE, YOLK))


def counters(m):
    return (m.pair_solves, m.cohesion_solves, list(m.viscosity_pairs), list(m.collider_hits), list(m.collider_grips),
            list(m.grip_sticks), list(m.wall_catches))


# ------------------------------------------------------------------------------------------------ the labels are right
# what the names of test_wall_model.HAND say, as labels of step 5b
HAND_LABELS = {
    "caught_from_above": {"catch_pos"},
    "caught_from_below": {"catch_neg"},
    "caught_inside_the_radius": {"catch_pos", "catch_inside_r"},
    "same_side_inside_the_radius": {"hit_inside"},
    "same_side_far": {"miss"},
    "beyond_the_end": {"round_end", "miss"},
    "beyond_the_end_inside_the_radius": {"round_end", "hit_end"},
    "before_the_start": {"round_start", "miss"},
}
assert sorted(HAND_LABELS) == sorted(twm.HAND)


def _one(x, y, r, px, py, collider, surface=None, h=1 / 120, i=0):
    """classify() on one particle: (set of labels, x, y)"""
    col = wm.normalise([collider])[0]
    srf = sm.normalise([surface])[0]
    lab, gx, gy = classify(np.array([x]), np.array([y]), np.array([r]), np.array([px]), np.array([py]), h, col, srf, 1, np.array([i]))
    return {name for name, lanes in lab.items() if lanes[0]}, float(gx[0]), float(gy[0])


def _against_by_hand(x, y, px, py, p, want):
    """the census of one application of wall p to a particle of radius 2 names `want` and agrees with test_wall_model's
    arithmetic by hand on whether it was caught, whether it was hit and where it went"""
    hx, hy, hit, nx, ny, pen, caught = twm.by_hand(x, y, 2.0, px, py, p)
    got, gx, gy = _one(x, y, 2.0, px, py, ("wall",) + tuple(p))
    assert got - GRIPS == want, (got, want)
    assert (gx, gy) == (hx, hy)
    assert bool(got & {"catch_pos", "catch_neg"}) == caught and ("miss" not in got) == hit
    assert got & GRIPS == ({"caught_smooth"} if caught else {"smooth"} if hit else set())


@pytest.mark.parametrize("name", sorted(twm.HAND))
def test_the_census_names_the_hand_table(name):
    (x, y), (px, py), caught = twm.HAND[name]
    assert bool(HAND_LABELS[name] & {"catch_pos", "catch_neg"}) == caught
    _against_by_hand(x, y, px, py, twm.WALL, HAND_LABELS[name])
    # a mask that does not cover the type
    assert _one(x, y, 2.0, px, py, ("wall",) + twm.WALL + ("yolk",)) == ({"masked"}, x, y)


def test_the_census_names_the_edges():
    """the applications of test_wall_model's edge tests (a position on the line, a start on the line, a degenerate wall)"""
    p = (0.0, 3.0, 8.0, 3.0)
    # test_a_position_exactly_on_the_line_is_caught
    _against_by_hand(2.0, 3.0, 1.0, 5.0, p, {"catch_pos", "catch_on_line", "catch_inside_r"})
    _against_by_hand(2.0, 3.0, 1.0, -1.5, p, {"catch_neg", "catch_on_line", "catch_inside_r"})
    # test_a_start_exactly_on_the_line_has_no_side
    _against_by_hand(2.0, -4.0, 1.0, 3.0, p, {"no_side", "miss"})
    _against_by_hand(2.0, 9.0, 1.0, 3.0, p, {"no_side", "miss"})
    _against_by_hand(2.0, 2.0, 1.0, 3.0, p, {"no_side", "hit_inside"})
    _against_by_hand(2.0, 3.0, 1.0, 3.0, p, {"no_side", "hit_inside", "on_it"})
    # test_a_degenerate_wall_is_the_segments_point
    q = (3.0, 3.0, 3.0, 3.0)
    _against_by_hand(4.0, 3.5, 1.0, 2.0, q, {"no_side", "point"})
    _against_by_hand(3.0, 3.0, 9.0, 9.0, q, {"no_side", "point", "on_it"})
    _against_by_hand(8.0, 8.0, -8.0, -8.0, q, {"no_side", "miss"})


@pytest.mark.parametrize("branch,mu", [("stick", 8.0), ("slide", 0.0009765625)])
@pytest.mark.parametrize("name", ["caught_from_above", "caught_from_below", "caught_inside_the_radius"])
def test_the_census_names_the_grip_after_a_catch(name, branch, mu):
    """test_wall_model.test_a_catch_with_friction's applications"""
    (x, y), (px, py), _ = twm.HAND[name]
    qx, qy, hit, nx, ny, pen, caught = twm.by_hand(x, y, 2.0, px, py, twm.WALL)
    wx, wy, took = twm.grip_by_hand(qx, qy, px, py, 1 / 120, mu, 30.0, -12.0, nx, ny, pen)
    got, gx, gy = _one(x, y, 2.0, px, py, ("wall",) + twm.WALL, (mu, 30.0, -12.0))
    assert took == branch and got & GRIPS == {"caught_" + branch} and (gx, gy) == (wx, wy)


def test_the_census_names_the_other_kinds():
    """one application each of a half-plane, a disc and a container, by hand"""
    assert _one(1.0, 1.0, 2.0, 1.0, 7.0, ("half_plane", 1.0, 0.0, 1.0))[0] == {"hit", "smooth"}
    assert _one(4.0, 1.0, 2.0, 1.0, 7.0, ("half_plane", 1.0, 0.0, 1.0))[0] == {"miss"}
    assert _one(4.0, 6.0, 2.0, 1.0, 7.0, ("disc", 4.0, 6.0, 1.5), i=3) == ({"hit", "centre", "smooth"}, 4.0 + DIRS[3, 0] * 3.5, 6.0 + DIRS[3, 1] * 3.5)
    assert _one(4.0, 7.0, 2.0, 1.0, 7.0, ("disc", 4.0, 6.0, 1.5), 2.0)[0] == {"hit", "stick"}  # (tl = 3, lim = 2 * 2.5)
    assert _one(4.0, 7.0, 2.0, 1.0, 7.0, ("disc", 4.0, 6.0, 1.5), 0.5)[0] == {"hit", "slide"}  # (lim = 0.5 * 2.5)
    assert _one(4.0, 9.5, 2.0, 1.0, 7.0, ("disc", 4.0, 6.0, 1.5))[0] == {"miss"}
    assert _one(4.0, 7.0, 2.0, 4.0, 8.0, ("container", 4.0, 6.0, 1.5), 0.5) == ({"hit", "clamped", "no_tangent"}, 4.0, 6.0)
    assert _one(4.0, 9.0, 2.0, 1.0, 7.0, ("container", 4.0, 6.0, 4.0))[0] == {"hit", "smooth"}
    assert _one(4.0, 7.0, 2.0, 1.0, 7.0, ("container", 4.0, 6.0, 4.0))[0] == {"miss"}


# ------------------------------------------------------------------------------------------------ a. the hand table
# One tiny batch (2 + 2 particles of radius 2) per case, its state set by hand: no damping, no follow constraint to
# speak of (strength 0, and the spots lie within the slack 2 sqrt(HAND_RADIUS) = 100 px of the target), one step of one
# sub-step of one pass with h = 1 / 64.  A particle at `prev` with velocity 64 (now - prev) meets the collider at
# prev + v / 64 = now, exactly: every coordinate is a dyadic number.  White particle 0 and yolk particle 1 are under
# test; the other particle of each type rests at REST, far from every collider and further from its mate than any pair
# reaches.
HAND_RADIUS, HAND_TARGET, REST, H64 = 2500.0, (0.0, 0.0), (1.0, 40.0), 1 / 64
TESTED = {WHITE: 0, YOLK: 1}
O = twm.WALL                 # the oblique wall of test_wall_model: a0 > 0 is the side above it
H = (0.0, 3.0, 8.0, 3.0)     # the horizontal wall of its edge tests: every ey term is zero
P = (3.0, 3.0, 3.0, 3.0)     # the degenerate one
MOVES = (30.0, -12.0)        # the surface velocity of test_wall_model.test_a_catch_with_friction; its two frictions:
STICK, SLIDE = 8.0, 0.0009765625
DISC, FLOOR = ("disc", 4.0, 6.0, 1.5), ("half_plane", 0.0, 1.0, -10.0)
PEN, CELL = ("container", 0.0, 0.0, 60.0), ("container", 4.0, 6.0, 1.5)


def _case(collider, now, prev, white, yolk=None, surface=None, then=None, mate=None):
    return dict(collider=collider, now=now, prev=prev, surface=surface, then=then, mate=mate,
                want={WHITE: set(white), YOLK: set(white if yolk is None else yolk)})


def _hand_want(name, caught):
    grip = {"caught_smooth"} if caught else set() if "miss" in HAND_LABELS[name] else {"smooth"}  # (surfaces unset)
    return HAND_LABELS[name] | grip


CASES = {"hand_" + name: _case(("wall",) + O, now, prev, _hand_want(name, caught)) for name, (now, prev, caught) in twm.HAND.items()}
CASES.update({
    # the oblique wall from its other side, and its ends
    "inside_the_radius_from_below": _case(("wall",) + O, (1.25, 2.0), (1.0, 0.0), {"catch_neg", "catch_inside_r", "caught_smooth"}),
    "same_side_inside_the_radius_below": _case(("wall",) + O, (1.25, 0.0), (0.5, -1.0), {"hit_inside", "smooth"}),
    "beyond_the_end_from_below": _case(("wall",) + O, (8.0, 5.0), (9.0, -3.0), {"round_end", "miss"}),
    "before_the_start_from_below": _case(("wall",) + O, (-6.0, 5.0), (-7.0, -3.0), {"round_start", "miss"}),
    "before_the_start_inside_the_radius": _case(("wall",) + O, (-5.0, 0.5), (-5.5, 3.0), {"round_start", "hit_start", "smooth"}),
    "before_the_start_inside_the_radius_from_below": _case(("wall",) + O, (-5.0, 1.5), (-5.5, -1.0), {"round_start", "hit_start", "smooth"}),
    "beyond_the_end_inside_the_radius_from_below": _case(("wall",) + O, (7.0, 2.0), (7.5, -1.0), {"round_end", "hit_end", "smooth"}),
    "start_cap_above": _case(("wall",) + O, (-5.0, 1.5), (-5.5, 2.0), {"hit_start", "smooth"}),
    "start_cap_below": _case(("wall",) + O, (-5.0, 0.5), (-5.5, 0.0), {"hit_start", "smooth"}),
    "end_cap_above": _case(("wall",) + O, (7.0, 2.0), (7.5, 2.5), {"hit_end", "smooth"}),
    "end_cap_below": _case(("wall",) + O, (7.0, 1.0), (7.5, 0.5), {"hit_end", "smooth"}),
    # a start so close below the wall that the ey term of a0 decides its side
    "close_below": _case(("wall",) + O, (5.5, 4.0), (5.0, 1.25), {"catch_neg", "caught_smooth"}),
    # the same line as a segment: what the wall catches crosses it or is pushed on, its caps are the wall's
    "segment_crossed": _case(("segment",) + O, (1.25, -3.5), (0.5, 4.0), {"miss"}),
    "segment_pushed_on": _case(("segment",) + O, (1.25, 0.5), (1.0, 2.0), {"hit_inside", "smooth"}),
    "segment_above": _case(("segment",) + O, (1.25, 2.5), (0.5, 3.0), {"hit_inside", "smooth"}),
    "segment_below": _case(("segment",) + O, (1.25, 0.0), (0.5, -1.0), {"hit_inside", "smooth"}),
    "segment_start_cap": _case(("segment",) + O, (-5.0, 0.5), (-5.5, 3.0), {"hit_start", "smooth"}),
    "segment_end_cap": _case(("segment",) + O, (7.0, 2.0), (7.5, -1.0), {"hit_end", "smooth"}),
    # the horizontal wall: the exact edges
    "on_the_line_from_above": _case(("wall",) + H, (2.0, 3.0), (1.0, 5.0), {"catch_pos", "catch_on_line", "catch_inside_r", "caught_smooth"}),
    "on_the_line_from_below": _case(("wall",) + H, (2.0, 3.0), (1.0, -1.5), {"catch_neg", "catch_on_line", "catch_inside_r", "caught_smooth"}),
    "across_from_above": _case(("wall",) + H, (2.0, 0.5), (1.0, 5.0), {"catch_pos", "caught_smooth"}),
    "across_from_below": _case(("wall",) + H, (2.0, 5.5), (1.0, 1.0), {"catch_neg", "caught_smooth"}),
    "no_side_down": _case(("wall",) + H, (2.0, -4.0), (1.0, 3.0), {"no_side", "miss"}),
    "no_side_up": _case(("wall",) + H, (2.0, 9.0), (1.0, 3.0), {"no_side", "miss"}),
    "no_side_inside_the_radius": _case(("wall",) + H, (2.0, 2.0), (1.0, 3.0), {"no_side", "hit_inside", "smooth"}),
    "no_side_on_it": _case(("wall",) + H, (2.0, 3.0), (1.0, 3.0), {"no_side", "hit_inside", "on_it", "smooth"}),
    "segment_on_it": _case(("segment",) + H, (2.0, 3.0), (1.0, 5.0), {"hit_inside", "on_it", "smooth"}),
    # two sub-steps: round the end in the first, under the wall in the second -- the straight line from the step's start
    # (last_x, last_y) to the end crosses the wall, the second sub-step's own path does not
    "round_the_end_and_under": _case(("wall",) + H, (9.0, 1.0), (8.25, 3.5), {"round_end", "miss"}, then=(0.25, -4.5)),
    # the other kinds.  DISC has m = 1.5 + 2; FLOOR keeps y >= -10 + 2; PEN (R = 60) holds every spot, CELL (R = 1.5 < r) has
    # m = 0 and puts whatever the type holds on its centre, the mate included
    "disc_hit": _case(DISC, (4.0, 8.0), (1.0, 7.0), {"hit", "smooth"}),
    "disc_centre": _case(DISC, (4.0, 6.0), (1.0, 7.0), {"hit", "centre", "smooth"}),
    "disc_miss": _case(DISC, (4.0, 10.0), (1.0, 7.0), {"miss"}),
    "disc_sticks": _case(DISC, (4.0, 8.0), (3.0, 9.0), {"hit", "stick"}, surface=(STICK, 0.0, 0.0)),
    "disc_centre_slides": _case(DISC, (4.0, 6.0), (1.0, 7.0), {"hit", "centre", "slide"}, surface=(SLIDE,) + MOVES),
    "half_plane_hit": _case(FLOOR, (2.0, -9.0), (1.0, -5.0), {"hit", "smooth"}),
    "half_plane_miss": _case(FLOOR, (2.0, -5.0), (1.0, -3.0), {"miss"}),
    "half_plane_slides": _case(FLOOR, (2.0, -9.0), (1.0, -5.0), {"hit", "slide"}, surface=(SLIDE,) + MOVES),
    "half_plane_straight": _case(FLOOR, (2.0, -9.0), (2.0, -5.0), {"hit", "no_tangent"}, surface=(STICK, 0.0, 0.0)),
    "container_hit": _case(PEN, (0.0, 59.0), (1.0, 57.0), {"hit", "smooth"}),
    "container_miss": _case(PEN, (2.0, 3.0), (1.0, 2.0), {"miss"}),
    "container_sticks": _case(PEN, (0.0, 59.0), (1.0, 57.0), {"hit", "stick"}, surface=(STICK, 0.0, 0.0)),
    "container_clamped": _case(CELL, (4.0, 7.0), (4.0, 8.0), {"hit", "clamped", "smooth"}, mate={"hit", "clamped", "smooth"}),
    "container_clamped_slides": _case(CELL, (4.0, 7.0), (3.0, 8.0), {"hit", "clamped", "slide"}, surface=(SLIDE,) + MOVES,
                                      mate={"hit", "clamped", "slide"}),
    # l2 == 0
    "point_wall": _case(("wall",) + P, (4.0, 3.5), (1.0, 2.0), {"no_side", "point", "smooth"}),
    "point_wall_on_it": _case(("wall",) + P, (3.0, 3.0), (9.0, 9.0), {"no_side", "point", "on_it", "smooth"}),
    "point_wall_far": _case(("wall",) + P, (8.0, 8.0), (-8.0, -8.0), {"no_side", "miss"}),
    "point_segment": _case(("segment",) + P, (4.0, 3.5), (1.0, 2.0), {"point", "smooth"}),
    "point_segment_on_it": _case(("segment",) + P, (3.0, 3.0), (9.0, 9.0), {"point", "on_it", "smooth"}),
    # a mask that does not cover the type
    "white_only": _case(("wall",) + O + ("white",), (1.25, -3.5), (0.5, 4.0), {"catch_pos", "caught_smooth"}, {"masked"}),
    "yolk_only": _case(("wall",) + O + ("yolk",), (1.25, 6.0), (2.0, -2.5), {"masked"}, {"catch_neg", "caught_smooth"}),
    # step 5c after a catch: pen = m + d
    "above_sticks": _case(("wall",) + O, (1.25, -3.5), (0.5, 4.0), {"catch_pos", "caught_stick"}, surface=(STICK,) + MOVES),
    "above_slides": _case(("wall",) + O, (1.25, -3.5), (0.5, 4.0), {"catch_pos", "caught_slide"}, surface=(SLIDE,) + MOVES),
    "below_sticks": _case(("wall",) + O, (1.25, 6.0), (2.0, -2.5), {"catch_neg", "caught_stick"}, surface=(STICK,) + MOVES),
    "below_slides": _case(("wall",) + O, (1.25, 6.0), (2.0, -2.5), {"catch_neg", "caught_slide"}, surface=(SLIDE,) + MOVES),
    "inside_the_radius_sticks": _case(("wall",) + O, (1.25, 0.5), (1.0, 2.0), {"catch_pos", "catch_inside_r", "caught_stick"}, surface=(STICK,) + MOVES),
    "inside_the_radius_slides": _case(("wall",) + O, (1.25, 0.5), (1.0, 2.0), {"catch_pos", "catch_inside_r", "caught_slide"}, surface=(SLIDE,) + MOVES),
    "above_sticks_at_rest": _case(("wall",) + O, (1.25, -3.5), (0.5, 4.0), {"catch_pos", "caught_stick"}, surface=(STICK, 0.0, 0.0)),
    "above_is_smooth": _case(("wall",) + O, (1.25, -3.5), (0.5, 4.0), {"catch_pos", "caught_smooth"}, surface=(0.0,) + MOVES),
    "straight_back": _case(("wall",) + H, (2.0, 1.0), (2.0, 5.0), {"catch_pos", "caught_no_tangent"}, surface=(STICK, 0.0, 0.0)),
    # step 5c of a wall that does not catch and of a segment: pen = m - d
    "wall_hit_sticks": _case(("wall",) + O, (1.25, 2.5), (0.5, 3.0), {"hit_inside", "stick"}, surface=(STICK,) + MOVES),
    "wall_hit_slides": _case(("wall",) + O, (1.25, 2.5), (0.5, 3.0), {"hit_inside", "slide"}, surface=(SLIDE,) + MOVES),
    "wall_hit_is_smooth": _case(("wall",) + O, (1.25, 2.5), (0.5, 3.0), {"hit_inside", "smooth"}, surface=(0.0,) + MOVES),
    "wall_hit_straight": _case(("wall",) + H, (2.0, 4.0), (2.0, 6.0), {"hit_inside", "no_tangent"}, surface=(STICK, 0.0, 0.0)),
    "end_cap_sticks": _case(("wall",) + O, (7.0, 2.0), (7.5, -1.0), {"round_end", "hit_end", "stick"}, surface=(STICK,) + MOVES),
    "segment_sticks": _case(("segment",) + O, (1.25, 0.0), (0.5, -1.0), {"hit_inside", "stick"}, surface=(STICK,) + MOVES),
    "segment_slides": _case(("segment",) + O, (1.25, 0.0), (0.5, -1.0), {"hit_inside", "slide"}, surface=(SLIDE,) + MOVES),
    "segment_straight": _case(("segment",) + H, (2.0, 4.0), (2.0, 6.0), {"hit_inside", "no_tangent"}, surface=(STICK, 0.0, 0.0)),
    "segment_start_cap_slides": _case(("segment",) + O, (-5.0, 0.5), (-5.5, 3.0), {"hit_start", "slide"}, surface=(SLIDE,) + MOVES),
})


# label: the case that starts above the oblique wall (a0 > 0), the one that starts below it
BOTH_SIDES = {
    "catch_inside_r": ("hand_caught_inside_the_radius", "inside_the_radius_from_below"),
    "hit_inside": ("hand_same_side_inside_the_radius", "same_side_inside_the_radius_below"),
    "hit_start": ("start_cap_above", "start_cap_below"),
    "hit_end": ("end_cap_above", "end_cap_below"),
    "round_start": ("hand_before_the_start", "before_the_start_from_below"),
    "round_end": ("hand_beyond_the_end", "beyond_the_end_from_below"),
    "caught_stick": ("above_sticks", "below_sticks"),
    "caught_slide": ("above_slides", "below_slides"),
}


def side_of(p, x, y):
    return (p[2] - p[0]) * (y - p[1]) - (p[3] - p[1]) * (x - p[0])


def hand_configs():
    w, y = rm.default_configs()
    extra = dict(damping=0, follow_strength=0, min_radius=2, max_radius=2)
    return dict(w, **extra), dict(y, **extra)


def hand_setup(name):
    """(spots, forces, update arguments) of the case.  spots: per type, per particle, (position at the start of the step,
    velocity).  A case with `then` runs two sub-steps, and a uniform force bends the path between them: with d1 = now -
    prev and d2 = then - now, a = (d2 - d1) / h^2 and the first velocity is d1 / h - h a."""
    c = CASES[name]
    (x, y), (px, py) = c["now"], c["prev"]
    vx, vy, forces, update = 64.0 * (x - px), 64.0 * (y - py), (), (H64, H64, 1, 1)
    if c["then"] is not None:
        ax, ay = (((c["then"][0] - x) - (x - px)) * 4096.0, ((c["then"][1] - y) - (y - py)) * 4096.0)
        vx, vy, forces, update = vx - H64 * ax, vy - H64 * ay, (("uniform", ax, ay),), (2 * H64, 2 * H64, 2, 1)
        assert (x + H64 * (64.0 * (x - px) + H64 * ax), y + H64 * (64.0 * (y - py) + H64 * ay)) == c["then"]
    tested, rest = ((px, py), (vx, vy)), (REST, (0.0, 0.0))
    first = (vx + H64 * forces[0][1], vy + H64 * forces[0][2]) if forces else (vx, vy)
    assert (px + H64 * first[0], py + H64 * first[1]) == (x, y)  # (exact: the collider meets `now`)
    return {w: [tested if p == TESTED[w] else rest for p in (0, 1)] for w in (WHITE, YOLK)}, forces, update


def hand_run(name, cls=CensusModel):
    """the case on a model of class `cls`: one step; returns (model, batch id)"""
    c = CASES[name]
    spots, forces, update = hand_setup(name)
    m = cls(*hand_configs())
    m.set_colliders([c["collider"]])
    m.set_forces(forces)
    if c["surface"] is not None:
        m.set_collider_surfaces([c["surface"]])
    i = m.add(*HAND_TARGET, HAND_RADIUS, HAND_RADIUS, 2, 2)
    for w, data in ((WHITE, m._white_data), (YOLK, m._yolk_data)):
        for p, ((x, y), (vx, vy)) in enumerate(spots[w]):
            for off, v in ((rm.X, x), (rm.Y, y), (rm.LAST_X, x), (rm.LAST_Y, y), (rm.VX, vx), (rm.VY, vy)):
                data[rm.offset(p + 1) + off] = v
    assert m.update(*update) == 1
    return m, i


@functools.lru_cache(maxsize=None)
def hand_model(name):
    return hand_run(name)


def assert_hand_labels(name):
    """the case takes the branch it is named for, on the model: the particle under test of either type carries exactly
    the labels of the table, its mate stays out of everything, and no pair was so much as looked at"""
    m, _ = hand_model(name)
    c = CASES[name]
    for w in (WHITE, YOLK):
        assert m.labels_of(w, TESTED[w]) == c["want"][w], (name, w, m.labels_of(w, TESTED[w]))
        mate = {"masked"} if c["want"][w] == {"masked"} else {"miss", "no_side"} if c["collider"] == ("wall",) + P else {"miss"}
        assert m.labels_of(w, 1 - TESTED[w]) == (c["mate"] or mate)
        if c["mate"] is not None:  # (CELL: the mate is put on the centre, or gripped on its way there)
            assert "hit" in c["mate"]
        elif c["then"] is None:  # (nothing has moved it; with `then` the force has, and it still meets nothing)
            assert [float(v) for v in m.state(w)[:, 1 - TESTED[w]]] == [REST[0], REST[1], 0.0, 0.0, REST[0], REST[1]]
        else:
            assert tuple(float(v) for v in m.state(w)[:2, TESTED[w]]) == c["then"]
        assert np.isfinite(m.state(w)).all()
    assert m.pair_solves == 0 and sum(m.viscosity_pairs) == 0 and m.cohesion_solves == 0
    return m


def hand_closed_form(name):
    """(x, y, vx, vy) of the particle under test per type where the case has a closed form, else None"""
    c = CASES[name]
    (x, y), (px, py) = c["now"], c["prev"]
    p, out = c["collider"][1:5], {}
    for w in (WHITE, YOLK):
        want = c["want"][w]
        if "catch_on_line" in want and c["collider"][1:5] == H and c["surface"] is None:
            gx, gy = x, 3.0 + (2.0 if py > 3.0 else -2.0)  # back to r from the line, on prev's side, straight
        elif "on_it" in want and c["surface"] is None:
            k = TESTED[w] & 7  # (the key of the particle: its index among the particles of its type)
            gx, gy = x + float(DIRS[k, 0]) * 2.0, y + float(DIRS[k, 1]) * 2.0
        elif c["surface"] is None and "centre" in want:  # out of the disc along DIRS[key & 7], to m = 1.5 + 2
            k = TESTED[w] & 7
            gx, gy = x + float(DIRS[k, 0]) * 3.5, y + float(DIRS[k, 1]) * 3.5
        elif c["surface"] is None and c["collider"] == FLOOR and "hit" in want:  # straight up to y = -10 + r
            gx, gy = x, -8.0
        elif c["surface"] is None and c["collider"] == PEN and "hit" in want and x == 0.0:  # back to R - r from the centre
            gx, gy = 0.0, 58.0
        elif c["surface"] is None and "clamped" in want:  # m = 0: onto the centre
            gx, gy = 4.0, 6.0
        elif "point" in want and c["surface"] is None:
            dx, dy = x - p[0], y - p[1]
            d = np.sqrt(np.float64(dx * dx + dy * dy))
            gx, gy = float(p[0] + (dx / d) * 2.0), float(p[1] + (dy / d) * 2.0)
        else:
            continue
        out[w] = (gx, gy, (gx - px) / H64, (gy - py) / H64)
    return out or None


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_case(name):
    m = assert_hand_labels(name)
    closed = hand_closed_form(name)
    for w, want in (closed or {}).items():
        assert tuple(float(v) for v in m.state(w)[:4, TESTED[w]]) == want
    plain, _ = hand_run(name, WallModel)  # recording is free
    assert same_state(m, plain) and counters(m) == counters(plain)


def test_the_case_of_the_issue():
    """a white particle at (1, 5) with v = (64, -128) lands at (2, 3), on the wall (0,3)-(8,3); it is caught to (2, 5)"""
    m = assert_hand_labels("on_the_line_from_above")
    assert hand_setup("on_the_line_from_above")[0][WHITE][0] == ((1.0, 5.0), (64.0, -128.0))
    assert [float(v) for v in m.state(WHITE)[:, 0]] == [2.0, 5.0, 64.0, 0.0, 1.0, 5.0]


def test_the_hand_table_holds_every_label():
    seen = {}
    for name, c in CASES.items():
        for w in (WHITE, YOLK):
            for lab in c["want"][w]:
                seen.setdefault((c["collider"][0], lab), set()).add((w, name))
    for kind, labels in (("half_plane", ("hit", "miss", "slide", "no_tangent", "smooth")),
                         ("disc", ("hit", "centre", "miss", "stick", "slide", "smooth")),
                         ("container", ("hit", "clamped", "miss", "stick", "slide", "smooth")),
                         ("segment", ("hit_inside", "hit_start", "hit_end", "on_it", "point", "miss", "stick", "slide", "no_tangent", "smooth")),
                         ("wall", ("hit_inside", "hit_start", "hit_end", "on_it", "point", "miss", "catch_pos", "catch_neg", "catch_inside_r",
                                   "catch_on_line", "no_side", "round_start", "round_end", "stick", "slide", "no_tangent", "smooth",
                                   "caught_stick", "caught_slide", "caught_no_tangent", "caught_smooth", "masked"))):
        for lab in labels:
            assert {w for w, _ in seen.get((kind, lab), ())} == {WHITE, YOLK}, (kind, lab)
    # from both sides where the label has a side
    for lab, (above, below) in BOTH_SIDES.items():
        for name, sign in ((above, 1.0), (below, -1.0)):
            c = CASES[name]
            assert c["collider"] == ("wall",) + O and lab in c["want"][WHITE] and lab in c["want"][YOLK]
            assert side_of(O, *c["prev"]) * sign > 0.0, (lab, name)


# ------------------------------------------------------------------------------------------------ b. - e. the scenes
OBLIQUE = (100.0, 330.0, 500.0, 430.0)
ROUGH = (0.4, 30.0, 7.5)
STARTS = ((300.0, 290.0), (280.0, 480.0), (490.0, 350.0), (110.0, 270.0))
TARGETS = ((320.0, 480.0), (300.0, 290.0), (540.0, 520.0), (60.0, 440.0))
# (the first target 240 px further right: the first batch is dragged along the wall into the third, across x = 400, the second
# cut of the group of three handles.  In the scene above no two batches of different handles of that group ever come near
# each other, so the group would exchange no ghost at all)
TARGETS_WIDE = ((560.0, 480.0),) + TARGETS[1:]
GRAVITY = (("uniform", 0.0, 400.0),)
CEILING, LEFT, RIGHT = ("half_plane", 0.0, 1.0, 275.0), ("wall", 200.0, 300.0, 300.0, 400.0), ("wall", 300.0, 400.0, 400.0, 300.0)
S, C = 2, 3
# name: (config of test_gpu_collider_walls.CONFIGS, colliders, surfaces, forces, starts, targets, steps)
SCENES = {
    # b. the oblique wall: the plain wall instantiation, the cohesive one, and everything on (what the groups run)
    "wall_default": ("default", (("wall",) + OBLIQUE,), (ROUGH,), (), STARTS, TARGETS, 10),
    "wall_both": ("both", (("wall",) + OBLIQUE,), (ROUGH,), (), STARTS, TARGETS, 10),
    "wall_all": ("both", (("wall",) + OBLIQUE,), (ROUGH,), GRAVITY, STARTS, TARGETS, 10),
    "wall_all_wide": ("both", (("wall",) + OBLIQUE,), (ROUGH,), GRAVITY, STARTS, TARGETS_WIDE, 10),
    # c. the same line as a segment, no wall in the list
    "segment_smooth": ("default", (("segment",) + OBLIQUE,), None, (), STARTS, TARGETS, 10),
    "segment_rough": ("default", (("segment",) + OBLIQUE,), (ROUGH,), (), STARTS, TARGETS, 10),
    # d. two walls that meet at (300, 400) under a ceiling, an egg driven into the corner
    "corner": ("default", (CEILING, LEFT, RIGHT), None, (), ((300.0, 320.0),), ((300.0, 500.0),), 8),
    "corner_reversed": ("default", (RIGHT, LEFT, CEILING), None, (), ((300.0, 320.0),), ((300.0, 500.0),), 8),
}
WALL_SCENES = ("wall_default", "wall_both", "wall_all", "wall_all_wide")
B_LABELS = ("catch_pos", "catch_neg", "catch_inside_r", "round_start", "round_end", "hit_start", "hit_end", "hit_inside")


def scene_run(name, cls=CensusModel, snapshot=None):
    """the scene on a model of class `cls`; snapshot(model, ids) is kept after every step.  The targets are set before
    the third step."""
    cfg, colliders, surfaces, forces, starts, targets, steps = SCENES[name]
    m = _configured_model(cfg, colliders, surfaces, forces, cls=cls)
    ids = [m.add(x, y, 50, 15) for x, y in starts]
    snaps = {}
    for k in range(steps):
        if k == 2:
            for i, (x, y) in zip(ids, targets):
                m.set_target_position(i, x, y)
        m.update(1 / 60, 1 / 60, S, C)
        if snapshot is not None:
            snaps[k + 1] = dict(snapshot(m, ids), catches=list(m.wall_catches),
                                sides={(w, lab, b): m.count(w, lab, batch=b) for w in (WHITE, YOLK) for lab in ("catch_pos", "catch_neg") for b in ids})
    return m, ids, snaps


@functools.lru_cache(maxsize=None)
def scene_model(name):
    """the scene on the CensusModel, once, with tests/test_gpu_collider_surfaces.py's snapshots after every step: shared by
    the tests that need it and never changed"""
    from test_gpu_collider_surfaces import _snapshot
    return scene_run(name, snapshot=_snapshot)


def crossed(name, w):
    """per batch: how many particles of type w end the scene on the other side of OBLIQUE's line than they began"""
    m, ids, _ = scene_model(name)
    begin = WallModel()
    for x, y in SCENES[name][4]:
        begin.add(x, y, 50, 15)
    over = side_of(OBLIQUE, *begin.state(w)[:2]) * side_of(OBLIQUE, *m.state(w)[:2]) < 0.0
    n = len(over) // len(ids)
    return [int(np.count_nonzero(over[b * n:(b + 1) * n])) for b in range(len(ids))]


def handle_gap(state):
    """the least distance between a particle of the first two of four equal batches and one of the last two"""
    x, y = state[:2]
    n = len(x) // 4
    return float(np.hypot(x[:2 * n, None] - x[None, 2 * n:], y[:2 * n, None] - y[None, 2 * n:]).min())


def assert_scene_reach(name):
    """what the scene is there for, on the model"""
    m, ids, snaps = scene_model(name)
    print("%s: census %s" % (name, [m.counts(w) for w in (WHITE, YOLK)]))
    for w in (WHITE, YOLK):
        assert np.isfinite(m.state(w)).all()
    if name in WALL_SCENES:
        if name in ("wall_all", "wall_all_wide"):
            # cuts at x = 200 and x = 400 give the fourth batch, the first two and the third to three handles.  In wall_all
            # no particle ever comes nearer than 90 px to a particle of another handle -- the widest reach is cohesion's 3 (r + r)
            # = 24 px --, so that group has no ghost to exchange; in wall_all_wide whites of the first and the third batch
            # come within a pair's reach 2 (r + r)
            gaps = [min(handle_gap(snaps[k]["state"][w]) for k in snaps) for w in (WHITE, YOLK)]
            assert (min(gaps) > 90.0) if name == "wall_all" else (gaps[WHITE] < 16.0), gaps
        for w in (WHITE, YOLK):
            for lab in B_LABELS + ("stick", "slide", "caught_stick", "caught_slide"):
                assert m.count(w, lab) > 0, (name, w, lab)
            # per batch (the device groups cut the scene in x): the first goes down across the wall, the second up, the
            # third round its end, the fourth round its start; every batch meets the wall and is caught
            for b, labs in ((1, ("catch_neg",)), (2, ("catch_pos",)), (3, ("catch_neg", "round_end", "hit_end")), (4, ("catch_neg", "round_start", "hit_start"))):
                for lab in labs + ("hit_inside", "catch_inside_r"):
                    assert m.count(w, lab, batch=ids[b - 1]) > 0, (name, w, b, lab)
            # hold: nothing of the two batches dragged across the wall's middle is on its far side
            # (in wall_all_wide part of the first batch is dragged round the wall's end)
            assert crossed(name, w)[1] == 0 and (crossed(name, w)[0] == 0 or name == "wall_all_wide")
        assert min(m.wall_catches) > 0 and (m.cohesion_solves > 0) == (min(m.viscosity_pairs) > 0) == (name != "wall_default")
    elif name.startswith("segment"):
        for w in (WHITE, YOLK):
            for lab in ("hit_start", "hit_end", "hit_inside") + (("stick", "slide") if name == "segment_rough" else ("smooth",)):
                assert m.count(w, lab) > 0, (name, w, lab)
            # leak: most of the two batches dragged across the segment's middle are on its far side
            n = m.n_particles(w) // len(ids)
            assert all(2 * k >= n for k in crossed(name, w)[:2]), crossed(name, w)
        assert m.wall_catches == [0, 0] and (sum(m.collider_grips) > 0) == (name == "segment_rough")
    else:
        walls = [c for c, col in enumerate(SCENES[name][1]) if col[0] == "wall"]
        ceiling = [c for c, col in enumerate(SCENES[name][1]) if col[0] == "half_plane"][0]
        for w in (WHITE, YOLK):
            assert (m.count(w, "hit", collider=ceiling) > 0) == (w == WHITE)  # (the yolk sits in the middle of the egg)
            assert m.count(w, "miss", collider=ceiling) > 0
            for c in walls:
                assert m.count(w, "catch_neg", collider=c) > 0 and m.count(w, "hit_inside", collider=c) > 0
        assert m.both_caught[WHITE] > 0  # (one particle, one pass, both walls: the second sweeps to where the first put it)
    return m, ids, snaps


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scene_reach_and_recording_is_free(name):
    m, ids, snaps = assert_scene_reach(name)
    plain, _, _ = scene_run(name, WallModel)
    assert same_state(m, plain) and counters(m) == counters(plain)


def test_the_oblique_wall_is_the_scene_of_the_issue():
    m, _, _ = scene_model("wall_default")
    want = dict(catch_pos=(184, 18), catch_neg=(277, 31), catch_inside_r=(306, 20), round_start=(318, 33), round_end=(383, 39),
                hit_start=(25, 2), hit_end=(28, 4), hit_inside=(2979, 353))
    assert {lab: (m.count(WHITE, lab), m.count(YOLK, lab)) for lab in want} == want


def test_the_order_of_the_corners_list_matters():
    a, b = scene_model("corner")[0], scene_model("corner_reversed")[0]
    assert not same_state(a, b)
    assert a.both_caught[WHITE] > 0 and b.both_caught[WHITE] > 0


# ------------------------------------------------------------------------------------------------ sensitivity
VARIANTS = ("swapped_normal", "a0_without_ey", "tc_up_to_2", "no_upper_clamp", "pen_m_minus_d", "sweep_from_last")


def variant_rule(variant, kind, x, y, r, px, py, lx, ly, p, idx):
    """the segment's (kind "segment") or the wall's rule over the lanes, wrong in the way `variant` names (None: right).
    Returns (x, y, hit, nx, ny, pen, caught)."""
    x0, y0, x1, y1 = p
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ex = x1 - x0
        ey = y1 - y0
        l2 = ex * ex + ey * ey
        t = np.zeros_like(x) if l2 == 0.0 else ((x - x0) * ex + (y - y0) * ey) / l2
        t = np.where(t < 0.0, 0.0, t)
        if variant != "no_upper_clamp":
            t = np.where(t > 1.0, 1.0, t)
        qx = x0 + t * ex
        qy = y0 + t * ey
        dx = x - qx
        dy = y - qy
        d2 = dx * dx + dy * dy
        m = 0.0 + r
        d = np.sqrt(d2)
        hit = d2 < m * m
        ux = np.where(d2 == 0.0, DIRS[idx & 7, 0], dx / d)
        uy = np.where(d2 == 0.0, DIRS[idx & 7, 1], dy / d)
        pen = m - d
        caught = np.zeros(len(x), dtype=bool)
        if kind == "wall":
            sx, sy = (lx, ly) if variant == "sweep_from_last" else (px, py)
            if variant == "a0_without_ey":
                a0 = ex * (sy - y0)
            else:
                a0 = ex * (sy - y0) - ey * (sx - x0)
            a1 = ex * (y - y0) - ey * (x - x0)
            opp = ((a0 > 0.0) & (a1 <= 0.0)) | ((a0 < 0.0) & (a1 >= 0.0))
            u = a0 / (a0 - a1)
            hx = sx + u * (x - sx)
            hy = sy + u * (y - sy)
            tc = ((hx - x0) * ex + (hy - y0) * ey) / np.float64(l2)
            caught = opp & (tc >= 0.0) & (tc <= (2.0 if variant == "tc_up_to_2" else 1.0))
            ln = np.sqrt(np.float64(l2))
            above = (a0 > 0.0) != (variant == "swapped_normal")
            ux = np.where(caught, np.where(above, (-ey) / ln, ey / ln), ux)
            uy = np.where(caught, np.where(above, ex / ln, (-ex) / ln), uy)
            pen = np.where(caught, pen if variant == "pen_m_minus_d" else m + d, pen)
            hit = hit | caught
    return np.where(hit, qx + ux * m, x), np.where(hit, qy + uy * m, y), hit, ux, uy, pen, caught


class VariantModel(WallModel):
    """WallModel whose segments and walls follow variant_rule(self.variant)"""
    variant = None

    def _solve_collision(self, particles, n_particles, *args, **kwargs):
        out = CohesiveModel._solve_collision(self, particles, n_particles, *args, **kwargs)
        if self.relaxed and self.colliders and n_particles:
            which = 0 if particles is self._white_data else 1
            base = [rm.offset(p) for p in range(1, n_particles + 1)]
            x, y, r, px, py, lx, ly = (np.array([particles[i + off] for i in base], dtype=np.float64)
                                       for off in (rm.X, rm.Y, rm.RADIUS, rm.PX, rm.PY, rm.LAST_X, rm.LAST_Y))
            idx = np.arange(n_particles)
            surfaces = self.surfaces if self.surfaces else [sm.DEFAULT] * len(self.colliders)
            for collider, surface in zip(self.colliders, surfaces):
                kind, p0, p1, p2, p3, mask = collider
                if kind not in ("segment", "wall"):
                    x, y, hits, grips, sticks = sm.project(x, y, r, px, py, self._sub_delta, [collider], [surface], 1 << which, idx)
                elif mask & (1 << which):
                    x, y, hit, nx, ny, pen, caught = variant_rule(self.variant, kind, x, y, r, px, py, lx, ly, (p0, p1, p2, p3), idx)
                    hits = int(np.count_nonzero(hit))
                    self.wall_catches[which] += int(np.count_nonzero(caught))
                    x, y, on, stuck = sm.grip(x, y, px, py, self._sub_delta, surface, nx, ny, pen, hit)
                    grips, sticks = int(np.count_nonzero(on)), int(np.count_nonzero(stuck))
                else:
                    continue
                self.collider_hits[which] += hits
                self.collider_grips[which] += grips
                self.grip_sticks[which] += sticks
            for k, i in enumerate(base):
                particles[i + rm.X] = float(x[k])
                particles[i + rm.Y] = float(y[k])
        return out


def _variant_class(variant):
    return type("Variant_%s" % variant, (VariantModel,), dict(variant=variant))


def test_the_right_variant_is_the_model():
    """variant None: the harness of the sensitivity test is WallModel, bit for bit"""
    for name in sorted(CASES):
        assert same_state(hand_run(name, _variant_class(None))[0], hand_model(name)[0]), name
    for name in ("wall_default", "segment_rough", "corner"):
        v = scene_run(name, _variant_class(None))[0]
        assert same_state(v, scene_model(name)[0]) and counters(v) == counters(scene_model(name)[0]), name


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_wrong_rule_changes_a_scene(variant):
    cls = _variant_class(variant)
    caught_by = [name for name in sorted(CASES) if not same_state(hand_run(name, cls)[0], hand_model(name)[0])]
    print("%s: caught by %s" % (variant, caught_by))
    assert caught_by, "no scene notices the variant %s" % variant
    if variant == "a0_without_ey":  # (the ey term decides a side only for a start close to the wall)
        assert caught_by == ["close_below"]
    if variant == "sweep_from_last":
        # only with a second sub-step do last_x / last_y differ from the sub-step's start, and only where the path bends does
        # that change a catch: ten steps of four eggs across the oblique wall do not notice
        assert caught_by == ["round_the_end_and_under"]
        assert same_state(scene_run("wall_default", cls)[0], scene_model("wall_default")[0])
    else:  # every other wrong rule changes the oblique wall's scene as well
        assert not same_state(scene_run("wall_default", cls)[0], scene_model("wall_default")[0])
