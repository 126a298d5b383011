"""tests/wall_model.py, the definition of the wall collider ("Walls"), against what the definition
promises: a list without walls is the surface model, a wall that never catches is a segment, single applications by hand in
Python floats, and the hold experiment -- an egg dragged across a segment passes through it, across a wall it does not.  No
device needed."""
import functools
import math

import numpy as np
import pytest

import collider_model as cm
import surface_model as sm
import wall_model as wm
from relaxed_model import DIRS, rm
from surface_model import SurfaceModel
from test_surface_model import SCENES, _by_hand as grip_by_hand, _scene
from wall_model import WallModel

WHITE, YOLK = 0, 1


# ---- a list without walls
@pytest.mark.parametrize("name", sorted(SCENES))
@pytest.mark.parametrize("surfaces", ["unset", "friction"])
def test_a_list_without_walls_is_the_surface_model(name, surfaces):
    colliders = SCENES[name] if isinstance(SCENES[name][0], tuple) else (SCENES[name],)
    given = None if surfaces == "unset" else [(0.4, 30.0, -10.0)] * len(colliders)
    cohesion, visc = name in ("disc", "corner"), 0.5 if name in ("container", "corner") else 0.0
    a = _scene(WallModel, colliders, given, cohesion, visc)
    b = _scene(SurfaceModel, colliders, given, cohesion, visc)
    assert a.colliders == b.colliders
    for w in (WHITE, YOLK):
        assert np.array_equal(a.state(w), b.state(w))
    assert a.collider_hits == b.collider_hits and sum(a.collider_hits) > 0
    assert (a.collider_grips, a.grip_sticks) == (b.collider_grips, b.grip_sticks)
    assert (sum(a.collider_grips) > 0) == (given is not None)
    assert (a.pair_solves, a.cohesion_solves, a.viscosity_pairs) == (b.pair_solves, b.cohesion_solves, b.viscosity_pairs)
    assert a.wall_catches == [0, 0]


def test_normalise_is_the_collider_models_with_one_more_kind():
    old = [("half_plane", 0.0, 3.0, -30.0), ("disc", 1.0, 2.0, 3.0, "white"), ("container", 1.0, 2.0, 3.0), ("segment", 1, 2, 3, 4, "yolk")]
    assert wm.normalise(old) == cm.normalise(old)
    assert wm.normalise([("wall", 1, 2, 3, 4), ("wall", 5, 6, 7, 8, "white")]) == [("wall", 1.0, 2.0, 3.0, 4.0, 3), ("wall", 5.0, 6.0, 7.0, 8.0, 1)]
    with pytest.raises(AssertionError):
        wm.normalise([("wall", 1, 2, 3)])


# ---- a wall that never catches is a segment
def _lowered(kind, surfaces, steps=10):
    """one default batch under a uniform force, its lowest particles 2.5 px above the collider, its target lowered by 2 px a
    step: 1 px a sub-step, a quarter of a radius, so the egg is pressed onto the collider and nothing ever crosses it"""
    w, y = rm.default_configs()
    m = WallModel(w, y)
    i = m.add(300.0, 300.0, 50, 15)
    m.set_colliders([(kind, 100.0, 350.0, 500.0, 350.0)])
    m.set_forces([("uniform", 0.0, 600.0)])
    if surfaces is not None:
        m.set_collider_surfaces(surfaces)
    hits = []
    for k in range(steps):
        m.set_target_position(i, 300.0, 300.0 + 2.0 * (k + 1))
        m.update(1 / 60, 1 / 60, 2, 3)
        hits.append(m.collider_hits[WHITE])
    assert hits[-1] > hits[-2] > hits[-3] > hits[0] > 0  # (it meets the collider at once and is still pressed onto it)
    return m


@pytest.mark.parametrize("surfaces", [None, [(0.5, 40.0, 0.0)]])
def test_an_egg_lowered_slowly_onto_a_wall_is_the_segment_scene(surfaces):
    a, b = _lowered("wall", surfaces), _lowered("segment", surfaces)
    assert a.wall_catches == [0, 0]
    for w in (WHITE, YOLK):
        assert np.array_equal(a.state(w), b.state(w))
    assert a.collider_hits == b.collider_hits and a.collider_hits[WHITE] > 0
    assert (a.collider_grips, a.grip_sticks) == (b.collider_grips, b.grip_sticks)
    assert (sum(a.collider_grips) > 0) == (surfaces is not None)


# ---- single applications by hand
def by_hand(x, y, r, px, py, p, i=0):
    """the wall's rule in Python floats (IEEE double, one rounding per operation), in the order of the definition.
    Returns (x, y, hit, nx, ny, pen, caught)."""
    x0, y0, x1, y1 = p
    ex = x1 - x0
    ey = y1 - y0
    l2 = ex * ex + ey * ey
    t = 0.0 if l2 == 0.0 else ((x - x0) * ex + (y - y0) * ey) / l2
    if t < 0.0:
        t = 0.0
    if t > 1.0:
        t = 1.0
    qx = x0 + t * ex
    qy = y0 + t * ey
    dx = x - qx
    dy = y - qy
    d2 = dx * dx + dy * dy
    m = 0.0 + r
    a0 = ex * (py - y0) - ey * (px - x0)
    a1 = ex * (y - y0) - ey * (x - x0)
    caught = False
    if (a0 > 0.0 and a1 <= 0.0) or (a0 < 0.0 and a1 >= 0.0):
        u = a0 / (a0 - a1)
        hx = px + u * (x - px)
        hy = py + u * (y - py)
        tc = ((hx - x0) * ex + (hy - y0) * ey) / l2
        caught = tc >= 0.0 and tc <= 1.0
    if caught:
        l, d = math.sqrt(l2), math.sqrt(d2)
        nx, ny = ((-ey) / l, ex / l) if a0 > 0.0 else (ey / l, (-ex) / l)
        return qx + nx * m, qy + ny * m, True, nx, ny, m + d, True
    if not d2 < m * m:
        return x, y, False, None, None, None, False
    d = math.sqrt(d2)
    ux, uy = (float(DIRS[i & 7, 0]), float(DIRS[i & 7, 1])) if d2 == 0.0 else (dx / d, dy / d)
    return qx + ux * m, qy + uy * m, True, ux, uy, m - d, False


def _apply(x, y, r, px, py, p, surface=None, mask="both", type_bit=1):
    col = wm.normalise([("wall",) + tuple(p) + (mask,)])
    out = wm.project([x], [y], [r], [px], [py], 1 / 120, col, sm.normalise([surface]) if surface is not None else [], type_bit)
    return (float(out[0][0]), float(out[1][0])) + out[2:6]


WALL = (-4.0, 1.0, 6.0, 1.5)  # a0 > 0 is the side above it (larger y)
# (position now, start of the sub-step, caught): radius 2 throughout
HAND = {
    "caught_from_above": ((1.25, -3.5), (0.5, 4.0), True),
    "caught_from_below": ((1.25, 6.0), (2.0, -2.5), True),
    "caught_inside_the_radius": ((1.25, 0.5), (1.0, 2.0), True),    # d < r on the far side: the segment would push it on
    "same_side_inside_the_radius": ((1.25, 2.5), (0.5, 3.0), False),  # the segment's hit
    "same_side_far": ((1.25, 9.0), (0.5, 12.0), False),               # nothing happens
    "beyond_the_end": ((9.0, -3.0), (8.0, 5.0), False),               # the path meets the line at tc > 1: round the wall
    "beyond_the_end_inside_the_radius": ((7.0, 0.75), (7.5, 3.0), False),  # ... and then the end point's disc rule
    "before_the_start": ((-7.0, -3.0), (-6.0, 5.0), False),           # tc < 0
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_one_application_by_hand(name):
    (x, y), (px, py), want_caught = HAND[name]
    r = 2.0
    ex_, ey_, hit, nx, ny, pen, caught = by_hand(x, y, r, px, py, WALL)
    assert caught == want_caught
    gx, gy, hits, grips, sticks, catches = _apply(x, y, r, px, py, WALL)
    assert (gx, gy) == (ex_, ey_) and (hits, catches) == (int(hit), int(caught)) and grips == 0
    # not caught: the segment's rule, bit for bit
    sx, sy, shits = cm.project([x], [y], [r], cm.normalise([("segment",) + WALL]), 1)
    if not caught:
        assert (gx, gy, hits) == (float(sx[0]), float(sy[0]), shits)
    else:  # caught: on prev's side, r from the line (to rounding: coordinates below 2^4, a handful of roundings < 1e-12)
        side = lambda qx, qy: (WALL[2] - WALL[0]) * (qy - WALL[1]) - (WALL[3] - WALL[1]) * (qx - WALL[0])  # noqa: E731
        assert side(gx, gy) * side(px, py) > 0.0 and side(x, y) * side(px, py) < 0.0
        assert abs(abs(side(gx, gy)) / math.hypot(WALL[2] - WALL[0], WALL[3] - WALL[1]) - r) < 1e-12
        assert (gx, gy) != (float(sx[0]), float(sy[0]))
    # a mask that does not cover the type leaves the particle alone
    assert _apply(x, y, r, px, py, WALL, mask="yolk") == (x, y, 0, 0, 0, 0)
    assert _apply(x, y, r, px, py, WALL, mask="yolk", type_bit=2)[:2] == (gx, gy)


def test_a_position_exactly_on_the_line_is_caught():
    """a1 == 0 with a0 != 0: u = 1, the path ends on the wall, the particle goes back to r from it; from either side"""
    p = (0.0, 3.0, 8.0, 3.0)
    for py, want_y in ((5.0, 5.0), (-1.5, 1.0)):
        got = _apply(2.0, 3.0, 2.0, 1.0, py, p)
        assert got == (2.0, want_y, 1, 0, 0, 1) == by_hand(2.0, 3.0, 2.0, 1.0, py, p)[:2] + (1, 0, 0, 1)


def test_a_start_exactly_on_the_line_has_no_side():
    """a0 == 0: not caught, whatever the position now -- the segment's rule"""
    p = (0.0, 3.0, 8.0, 3.0)
    for x, y in ((2.0, -4.0), (2.0, 9.0), (2.0, 2.0), (2.0, 3.0)):
        gx, gy, hits, grips, sticks, catches = _apply(x, y, 2.0, 1.0, 3.0, p)
        sx, sy, shits = cm.project([x], [y], [2.0], cm.normalise([("segment",) + p]), 1)
        assert (gx, gy, hits, catches) == (float(sx[0]), float(sy[0]), shits, 0)
        assert by_hand(x, y, 2.0, 1.0, 3.0, p)[:2] == (gx, gy)
    assert _apply(2.0, 3.0, 2.0, 1.0, 3.0, p)[:3] == (2.0 + 2.0, 3.0, 1)  # (on the wall itself, d2 == 0: DIRS[0] = (1, 0))


def test_a_degenerate_wall_is_the_segments_point():
    """l2 == 0: a0 == 0 as well, never caught; acts as a disc of radius 0 at the point"""
    p = (3.0, 3.0, 3.0, 3.0)
    for (x, y), (px, py) in (((4.0, 3.5), (1.0, 2.0)), ((3.0, 3.0), (9.0, 9.0)), ((8.0, 8.0), (-8.0, -8.0))):
        gx, gy, hits, grips, sticks, catches = _apply(x, y, 2.0, px, py, p)
        sx, sy, shits = cm.project([x], [y], [2.0], cm.normalise([("segment",) + p]), 1)
        assert (gx, gy, hits, catches) == (float(sx[0]), float(sy[0]), shits, 0)
        assert math.isfinite(gx) and math.isfinite(gy)
        assert by_hand(x, y, 2.0, px, py, p)[:2] == (gx, gy)


def test_a_nan_is_not_caught():
    nan = float("nan")
    # a NaN start: no side, so the segment's rule on the position now
    for x, y in ((1.25, -3.5), (1.25, 2.5)):
        gx, gy, hits, grips, sticks, catches = _apply(x, y, 2.0, nan, nan, WALL, surface=1.0)
        sx, sy, shits = cm.project([x], [y], [2.0], cm.normalise([("segment",) + WALL]), 1)
        assert (gx, gy, hits, catches) == (float(sx[0]), float(sy[0]), shits, 0)
    for px, py in ((nan, 4.0), (0.5, nan)):
        assert _apply(1.25, -3.5, 2.0, px, py, WALL)[2:] == (0, 0, 0, 0)
    # a NaN position is left alone
    for x, y in ((nan, -3.5), (1.25, nan), (nan, nan)):
        gx, gy, hits, grips, sticks, catches = _apply(x, y, 2.0, 0.5, 4.0, WALL, surface=1.0)
        assert (math.isnan(gx), math.isnan(gy)) == (math.isnan(x), math.isnan(y)) and (hits, grips, catches) == (0, 0, 0)
        assert (gx == x or math.isnan(x)) and (gy == y or math.isnan(y))


@pytest.mark.parametrize("branch,mu", [("stick", 8.0), ("slide", 0.0009765625)])
@pytest.mark.parametrize("name", ["caught_from_above", "caught_from_below", "caught_inside_the_radius"])
def test_a_catch_with_friction(name, branch, mu):
    """step 5c of a catch: n is the normal towards prev's side, pen = m + d"""
    (x, y), (px, py), _ = HAND[name]
    r, h, vx, vy = 2.0, 1 / 120, 30.0, -12.0
    qx, qy, hit, nx, ny, pen, caught = by_hand(x, y, r, px, py, WALL)
    assert caught
    ex, ey = WALL[2] - WALL[0], WALL[3] - WALL[1]
    t = ((x - WALL[0]) * ex + (y - WALL[1]) * ey) / (ex * ex + ey * ey)
    cx, cy = WALL[0] + t * ex, WALL[1] + t * ey
    assert pen == (0.0 + r) + math.sqrt((x - cx) * (x - cx) + (y - cy) * (y - cy)) > r
    wx, wy, took = grip_by_hand(qx, qy, px, py, h, mu, vx, vy, nx, ny, pen)
    assert took == branch, (took, pen)
    gx, gy, hits, grips, sticks, catches = _apply(x, y, r, px, py, WALL, surface=(mu, vx, vy))
    assert (gx, gy) == (wx, wy) != (qx, qy)
    assert (hits, grips, sticks, catches) == (1, 1, 1 if branch == "stick" else 0, 1)
    # the tangential move took nothing of the normal part (coordinates below 2^4: a handful of roundings stay below 1e-12)
    assert abs((gx - qx) * nx + (gy - qy) * ny) < 1e-12


def test_list_order_and_two_particles_that_cross_together():
    """each collider works on the result of the one before it; overlapping particles that cross together both land on the
    line r from the wall"""
    p = (0.0, 3.0, 8.0, 3.0)
    col = wm.normalise([("half_plane", 1.0, 0.0, 1.0), ("wall",) + p, ("disc", 4.0, 6.0, 1.5)])
    x, y, hits, grips, sticks, catches, ever = wm.project([1.0, 4.0, 4.0], [1.0, -2.0, -2.5], [2.0, 2.0, 1.0], [1.0, 4.0, 4.0], [7.0, 6.0, 6.5],
                                                    1 / 120, col, [], 1)
    # particle 0: the half-plane moves it to x = 3, the wall catches it at (3, 5), the disc (m = 3.5) pushes it out;
    # particles 1 and 2 cross together and land on y = 3 + r, inside the disc, which moves them last
    assert catches == 3 and hits == 1 + 3 + 3 and ever.all()
    first = wm.project([1.0, 4.0, 4.0], [1.0, -2.0, -2.5], [2.0, 2.0, 1.0], [1.0, 4.0, 4.0], [7.0, 6.0, 6.5], 1 / 120, col[:2], [], 1)
    assert [float(v) for v in first[0]] == [3.0, 4.0, 4.0] and [float(v) for v in first[1]] == [5.0, 5.0, 4.0]
    assert np.all(np.hypot(x - 4.0, y - 6.0) >= np.array([3.5, 3.5, 2.5]) - 1e-12)


# ---- the hold experiment ("Walls")
@functools.lru_cache(maxsize=None)
def hold(kind, types=None, steps=30):
    """one default batch at (300, 300) -- 157 white and 15 yolk particles, the largest y 347.5 -- above a collider along
    y = 380; before the third step the target goes to (300, 480), across it"""
    m = WallModel()
    i = m.add(300.0, 300.0, 50, 15)
    assert (m.n_particles(WHITE), m.n_particles(YOLK)) == (157, 15)
    assert round(max(float(m.state(w)[1].max()) for w in (WHITE, YOLK)), 1) == 347.5  # (32.5 px above the collider)
    m.set_colliders([(kind, 100.0, 380.0, 500.0, 380.0) + ((types,) if types else ())])
    for k in range(steps):
        if k == 2:
            m.set_target_position(i, 300.0, 480.0)
        m.update(1 / 60, 1 / 60, 2, 3)
    return m


def _beyond(m, w):
    return int(np.count_nonzero(m.state(w)[1] > 380.0))


def test_hold_a_wall_holds_the_egg():
    m = hold("wall")
    for w in (WHITE, YOLK):
        assert np.isfinite(m.state(w)).all()
        assert _beyond(m, w) == 0
        assert m.wall_catches[w] > 0
    top = max(float(m.state(w)[1].max()) for w in (WHITE, YOLK))
    print("wall: catches %s, hits %s, largest y %r" % (m.wall_catches, m.collider_hits, top))
    assert m.wall_catches == [202, 23] and top == 376.0  # (what this model gives: 380 - r exactly; 225 catches in all)
    assert all(h >= c for h, c in zip(m.collider_hits, m.wall_catches))  # (a catch is a hit)


def test_hold_a_segment_leaks():
    m = hold("segment")
    print("segment: hits %s, beyond %s" % (m.collider_hits, [_beyond(m, w) for w in (WHITE, YOLK)]))
    for w in (WHITE, YOLK):
        assert 2 * _beyond(m, w) >= m.n_particles(w)
    assert [_beyond(m, w) for w in (WHITE, YOLK)] == [157, 15] and m.collider_hits == [403, 26]  # (all of them, as measured)
    assert m.wall_catches == [0, 0]


def test_hold_a_white_only_wall_lets_the_yolk_through():
    m = hold("wall", "white")
    assert _beyond(m, WHITE) == 0 and m.wall_catches[WHITE] > 0
    assert _beyond(m, YOLK) == m.n_particles(YOLK) and m.wall_catches[YOLK] == 0 and m.collider_hits[YOLK] == 0
    for w in (WHITE, YOLK):
        assert np.isfinite(m.state(w)).all()
