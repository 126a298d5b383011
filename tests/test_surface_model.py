"""tests/surface_model.py, the definition of the collider surfaces ("Collider surfaces"), against what
the definition promises: default surfaces change nothing, one application per kind by hand (stick and slide), a straight
drop is left alone, and the incline experiment -- friction never lets an egg travel further.  No device needed."""
import functools
import math

import numpy as np
import pytest

import collider_model as cm
import surface_model as sm
from relaxed_model import DIRS, rm
from surface_model import SurfaceModel
from viscosity_model import ViscosityModel

WHITE, YOLK = 0, 1
WHITE3 = dict(cohesion_interaction_distance_factor=3, cohesion_strength=0.99)
SCENES = {
    "half_plane": ("half_plane", 2.0, 0.0, 320.0),
    "disc": ("disc", 300.0, 300.0, 30.0),
    "container": ("container", 400.0, 300.0, 60.0),
    "segment": ("segment", 250.0, 310.0, 350.0, 310.0),
    "corner": (("half_plane", 1.0, 0.0, 290.0), ("disc", 300.0, 300.0, 30.0)),
}


def _scene(cls, colliders, surfaces=None, cohesion=False, viscosity=0.0, steps=6):
    w, y = rm.default_configs()
    m = cls(dict(w, **WHITE3), y, cohesion=cohesion)
    m.add(300.0, 300.0, 50, 15)
    m.set_colliders(list(colliders))
    m.set_forces([("uniform", 300.0, 980.0)])
    m.set_viscosity(viscosity, viscosity)
    if surfaces is not None:
        m.set_collider_surfaces(surfaces)
    for _ in range(steps):
        m.update(1 / 60, 1 / 60, 2, 3)
    return m


@pytest.mark.parametrize("name", sorted(SCENES))
@pytest.mark.parametrize("surfaces", ["unset", "zeros", "velocity_only"])
def test_default_surfaces_are_the_viscosity_model(name, surfaces):
    colliders = SCENES[name] if isinstance(SCENES[name][0], tuple) else (SCENES[name],)
    given = {"unset": None, "zeros": [None] * len(colliders), "velocity_only": [(0.0, 250.0, -40.0)] * len(colliders)}[surfaces]
    cohesion, visc = name in ("disc", "corner"), 0.5 if name in ("container", "corner") else 0.0
    a = _scene(SurfaceModel, colliders, given, cohesion, visc)
    b = _scene(ViscosityModel, colliders, None, cohesion, visc)
    for w in (WHITE, YOLK):
        assert np.array_equal(a.state(w), b.state(w))
    assert a.collider_hits == b.collider_hits and sum(a.collider_hits) > 0
    assert (a.pair_solves, a.cohesion_solves, a.viscosity_pairs) == (b.pair_solves, b.cohesion_solves, b.viscosity_pairs)
    assert a.collider_grips == [0, 0]


def _by_hand(x, y, px, py, h, mu, vx, vy, nx, ny, pen):
    """step 5c in Python floats (IEEE double, one rounding per operation), in the order of the definition"""
    ex = (x - px) - h * vx
    ey = (y - py) - h * vy
    dn = ex * nx + ey * ny
    tx = ex - dn * nx
    ty = ey - dn * ny
    tl2 = tx * tx + ty * ty
    if not tl2 > 0.0:
        return x, y, None
    tl = math.sqrt(tl2)
    lim = mu * pen
    if tl <= lim:
        return x - tx, y - ty, "stick"
    f = lim / tl
    return x - tx * f, y - ty * f, "slide"


# one particle of radius 2 that the collider moves, and where it was at the start of the sub-step
HAND = {
    "half_plane": (("half_plane", 0.6, 0.8, 10.0), (7.0, 8.5), (6.25, 9.75)),
    "disc": (("disc", 3.0, -1.0, 5.0), (6.5, 2.25), (8.0, 0.5)),
    "container": (("container", 3.0, -1.0, 9.0), (9.5, 3.75), (7.0, 5.0)),
    "segment": (("segment", -4.0, 1.0, 6.0, 1.5), (1.25, 2.5), (0.5, 3.0)),
}


@pytest.mark.parametrize("kind", sorted(HAND))
@pytest.mark.parametrize("branch,mu", [("stick", 8.0), ("slide", 0.125)])
def test_one_application_by_hand(kind, branch, mu):
    collider, (x, y), (px, py) = HAND[kind]
    r, h, vx, vy = 2.0, 1 / 120, 30.0, -12.0
    col = cm.normalise([collider])
    qx, qy, hits = cm.project([x], [y], [r], col, 1)
    assert hits == 1
    qx, qy = float(qx[0]), float(qy[0])
    _, p0, p1, p2, p3, _ = col[0]
    if kind == "half_plane":
        s = (p0 * x + p1 * y) - (p2 + r)
        nx, ny, pen = p0, p1, -s
    else:
        cx, cy, m = p0, p1, p2 + r
        if kind == "segment":
            ex, ey = p2 - p0, p3 - p1
            t = min(max(((x - p0) * ex + (y - p1) * ey) / (ex * ex + ey * ey), 0.0), 1.0)
            cx, cy, m = p0 + t * ex, p1 + t * ey, 0.0 + r
        if kind == "container":
            m = p2 - r
        dx, dy = x - cx, y - cy
        d = math.sqrt(dx * dx + dy * dy)
        nx, ny, pen = dx / d, dy / d, (d - m if kind == "container" else m - d)
    assert pen > 0.0
    ex_, ey_, took = _by_hand(qx, qy, px, py, h, mu, vx, vy, nx, ny, pen)
    assert took == branch, (took, pen)
    gx, gy, hits, grips, sticks = sm.project([x], [y], [r], [px], [py], h, col, sm.normalise([(mu, vx, vy)]), 1)
    assert (float(gx[0]), float(gy[0])) == (ex_, ey_) != (qx, qy)
    assert (hits, grips, sticks) == (1, 1, 1 if branch == "stick" else 0)
    # the tangential move took nothing of the normal part: the depth along n is the projection's (to rounding; coordinates
    # below 2^4, so one rounding is below 2^-49 and a handful stay below 1e-12)
    assert abs((gx[0] - qx) * nx + (gy[0] - qy) * ny) < 1e-12
    # a mask that does not cover the type, and a collider that does not bind, grip nothing
    far = sm.project([px + 100.0], [py + 100.0], [r], [px], [py], h, cm.normalise([("disc", 3.0, -1.0, 5.0)]), sm.normalise([mu]), 1)
    assert far[2:] == (0, 0, 0)
    other = sm.project([x], [y], [r], [px], [py], h, cm.normalise([collider + ("yolk",)]), sm.normalise([mu]), 1)
    assert other[2:] == (0, 0, 0) and (other[0][0], other[1][0]) == (x, y)


def test_a_particle_on_a_discs_centre_grips_with_the_full_depth():
    """d2 == 0: n = DIRS[i & 7], d = 0 so pen = m"""
    n, r, h, mu = 9, 1.5, 1 / 120, 0.25
    x, y = np.full(n, 12.5), np.full(n, -3.25)
    px, py = x - 0.75, y + 0.5
    col = cm.normalise([("disc", 12.5, -3.25, 6.0)])
    gx, gy, hits, grips, _ = sm.project(x, y, np.full(n, r), px, py, h, col, sm.normalise([mu]), 1)
    assert hits == n and grips == n - 0
    for i in range(n):
        nx, ny = (float(v) for v in DIRS[i & 7])
        qx, qy = 12.5 + nx * 7.5, -3.25 + ny * 7.5
        ex, ey, took = _by_hand(qx, qy, float(px[i]), float(py[i]), h, mu, 0.0, 0.0, nx, ny, 7.5 - 0.0)
        assert took is not None and (float(gx[i]), float(gy[i])) == (ex, ey)


def test_a_container_smaller_than_the_particle_holds_it_at_the_centre():
    """R < r: m = 0, the particle lands on the centre, pen = d"""
    col = cm.normalise([("container", 4.0, 4.0, 1.0)])
    gx, gy, hits, grips, sticks = sm.project([7.0], [8.0], [2.0], [6.0], [8.5], 1 / 120, col, sm.normalise([0.5]), 1)
    ex, ey, took = _by_hand(4.0 + 0.6 * 0.0, 4.0 + 0.8 * 0.0, 6.0, 8.5, 1 / 120, 0.5, 0.0, 0.0, 0.6, 0.8, 5.0 - 0.0)
    assert (hits, grips) == (1, 1) and took is not None and (float(gx[0]), float(gy[0])) == (ex, ey)


def test_a_straight_drop_is_left_alone():
    """tl2 == 0: the displacement is along the normal -- position and grip count stay"""
    col = cm.normalise([("half_plane", 0.0, -1.0, -100.0)])
    x, y, r = np.array([10.0, 20.0]), np.array([99.5, 99.0]), np.array([2.0, 2.0])
    px, py = x.copy(), np.array([95.0, 96.0])
    qx, qy, _ = cm.project(x, y, r, col, 1)
    gx, gy, hits, grips, sticks = sm.project(x, y, r, px, py, 1 / 120, col, sm.normalise([3.0]), 1)
    assert hits == 2 and (grips, sticks) == (0, 0)
    assert np.array_equal(gx, qx) and np.array_equal(gy, qy)
    # a NaN is left alone by every comparison: no hit, no grip, the bits stay
    nan = np.array([np.nan])
    for c in HAND.values():
        ox, oy, h, g, _ = sm.project(nan, nan, [2.0], [1.0], [1.0], 1 / 120, cm.normalise([c[0]]), sm.normalise([1.0]), 1)
        assert np.isnan(ox[0]) and np.isnan(oy[0]) and (h, g) == (0, 0)
    # a NaN start of the sub-step: tl2 is NaN, !(tl2 > 0) holds, nothing happens
    ox, oy, h, g, _ = sm.project([10.0], [99.5], [2.0], nan, nan, 1 / 120, col, sm.normalise([1.0]), 1)
    assert (float(ox[0]), float(oy[0]), h, g) == (float(qx[0]), float(qy[0]), 1, 0)


def test_set_colliders_resets_the_surfaces():
    m = SurfaceModel()
    m.set_colliders([("disc", 0.0, 0.0, 1.0)])
    m.set_collider_surfaces([0.5])
    assert m.surfaces == [(0.5, 0.0, 0.0)]
    m.set_colliders([("disc", 0.0, 0.0, 1.0)])
    assert m.surfaces == []


# ---- the incline experiment ("Collider surfaces": the table) ----
INCLINE_MUS = (0.0, 0.1, 0.3, 0.6, 1.2)
INCLINE_DEG = 20.0


@functools.lru_cache(maxsize=None)
def incline(mu, cls=SurfaceModel, steps=60):
    """one default batch, follow_strength 0, on a floor (y <= 400 - r) under gravity tilted by INCLINE_DEG towards +x"""
    w, y = rm.default_configs()
    m = cls(dict(w, follow_strength=0), dict(y, follow_strength=0))
    m.add(300.0, 340.0, 50, 15)
    m.set_colliders([("half_plane", 0.0, -1.0, -400.0)])
    a = math.radians(INCLINE_DEG)
    m.set_forces([("uniform", 980.0 * math.sin(a), 980.0 * math.cos(a))])
    if mu is not None:
        m.set_collider_surfaces([mu])
    x0 = float(np.mean(np.concatenate([m.state(WHITE)[0], m.state(YOLK)[0]])))
    for _ in range(steps):
        m.update(1 / 60, 1 / 60, 2, 3)
    x1 = float(np.mean(np.concatenate([m.state(WHITE)[0], m.state(YOLK)[0]])))
    return m, x1 - x0


def test_incline_friction_never_lets_the_egg_travel_further():
    travel = []
    for mu in INCLINE_MUS:
        m, t = incline(mu)
        for w in (WHITE, YOLK):
            assert np.isfinite(m.state(w)).all(), (mu, w)
        grips = sum(m.collider_grips)
        print("mu %.2f: travel %.3f px, hits %d, grips %d, stick share %.3f" %
              (mu, t, sum(m.collider_hits), grips, sum(m.grip_sticks) / grips if grips else 0.0))
        assert (grips > 0) == (mu > 0.0)
        travel.append(t)
    assert travel[0] > 0.0  # (the frictionless egg does slide down the slope)
    assert all(b <= a for a, b in zip(travel, travel[1:])), travel
    # mu = 0 is the frictionless model, bit for bit
    a, b = incline(0.0)[0], incline(None, ViscosityModel)[0]
    for w in (WHITE, YOLK):
        assert np.array_equal(a.state(w), b.state(w))
    assert a.collider_hits == b.collider_hits
