"""tests/force_model.py, the definition of the force fields of the relaxed step ("Forces"), against
what the definition promises: the empty list, free fall against the closed recurrence, the radial field's reach and sign,
the vortex field's direction, the type mask, the immovable particle, and a scene that rests in a container.  No device
needed."""
import functools
import math

import numpy as np
import pytest

import force_model as fm
from collider_model import ColliderModel
from conftest import load_golden
from force_model import ForceModel
from relaxed_model import rm

WHITE, YOLK = 0, 1
WHITE3 = dict(cohesion_interaction_distance_factor=3, cohesion_strength=0.99)
U = 2.0 ** -53  # one rounding of a double, relative


@functools.lru_cache(maxsize=None)
def _run(forces, cohesion=False, steps=6, cls=ForceModel, colliders=(), white=()):
    w, y = rm.default_configs()
    m = cls(dict(w, **WHITE3, **dict(white)), y, cohesion=cohesion)
    m.add(300.0, 300.0, 50, 15)
    m.set_colliders(list(colliders))
    if forces is not None:
        m.set_forces(list(forces))
    for _ in range(steps):
        m.update(1 / 60, 1 / 60, 2, 3)
    return m


@pytest.mark.parametrize("cohesion", [False, True])
@pytest.mark.parametrize("colliders", [(), (("container", 300.0, 300.0, 40.0), ("half_plane", 0.0, -1.0, -320.0))])
def test_an_empty_list_is_the_collider_model(cohesion, colliders):
    a, b = _run((), cohesion, colliders=colliders), _run(None, cohesion, cls=ColliderModel, colliders=colliders)
    for w in (WHITE, YOLK):
        assert np.array_equal(a.state(w), b.state(w))
    assert (a.pair_solves, a.cohesion_solves, a.collider_hits) == (b.pair_solves, b.cohesion_solves, b.collider_hits)
    assert a.force_acts == [0, 0] and (sum(a.collider_hits) > 0) == bool(colliders)
    assert not np.array_equal(_run((("uniform", 0.0, 980.0),), cohesion, colliders=colliders).state(WHITE), b.state(WHITE))


def test_free_fall_follows_the_closed_recurrence():
    """The first particle of a type starts on the batch's centre, the only other one 283 px away and, with a follow strength
    of 0, drifting towards it by less than a pixel per step; the follow constraint is slack within 2 sqrt(400) = 40 px of the
    target and the fall stays below 30 px, so no pair and no constraint touches the first particle: a sub-step is v <- (v + dt g) damping, x <- x + dt v, bit for bit, and the speed approaches
    dt g damping / (1 - damping).  The speed read back is (x - px) / dt with x below 2^12: an error below 2^-41 * 120 < 1e-10
    px/s, against a terminal speed of some px/s; 1e-6 relative leaves orders of magnitude."""
    g = 50.0
    wc, yc = rm.default_configs()
    m = ForceModel(dict(wc, follow_strength=0), dict(yc, follow_strength=0))
    m.add(300.0, 300.0, 400.0, 400.0, 2, 2)
    m.set_forces([("uniform", 0.0, g)])
    dt = 1 / 60
    for w, cfg in ((WHITE, m._white_config), (YOLK, m._yolk_config)):
        d = 1 - min(max(cfg["damping"], 0), 1)
        assert 0 < d < 1
    for step in range(200):
        before = [m.state(w) for w in (WHITE, YOLK)]
        m.update(dt, dt, 1, 3)
        for w, cfg in ((WHITE, m._white_config), (YOLK, m._yolk_config)):
            d = 1 - min(max(cfg["damping"], 0), 1)
            x0, y0, vx0, vy0 = (float(before[w][k][0]) for k in range(4))
            vx, vy = (vx0 + dt * (0.0 + 0.0)) * d, (vy0 + dt * (0.0 + g)) * d
            st = m.state(w)
            assert (st[0][0], st[1][0]) == (x0 + dt * vx, y0 + dt * vy), (step, w)
            assert abs(st[1][0]) < 2.0 ** 12
    for w, cfg in ((WHITE, m._white_config), (YOLK, m._yolk_config)):
        d = 1 - min(max(cfg["damping"], 0), 1)
        terminal = dt * g * d / (1 - d)
        # d^200 of the distance to the terminal speed is left
        assert d ** 200 < 1e-9
        assert m.state(w)[3][0] == pytest.approx(terminal, rel=1e-6), w
        assert m.state(w)[2][0] == 0.0
        assert abs(m.state(w)[1][0] - 300.0) < 30.0
    assert m.force_acts == [0, 0] and m.pair_solves == 0  # (a uniform field has no condition)


def test_a_radial_field_reaches_from_its_centre_to_its_edge_exclusive():
    R, c = 80.0, (12.5, -3.25)
    x = np.array([c[0], c[0] + R, c[0] - R, c[0], c[0] + 81.0, c[0] + 3.0, c[0] - 40.0, c[0], np.nan])
    y = np.array([c[1], c[1], c[1], c[1] + R, c[1], c[1] + 4.0, c[1], c[1] - 79.0, 0.0])
    for strength in (4000.0, -4000.0):
        ax, ay, acts = fm.acceleration(x, y, fm.normalise([("radial", c[0], c[1], strength, R)]), 1)
        assert acts == 3
        # at the centre, on the edge, beyond it and at a NaN: exactly nothing (+0.0)
        for k in (0, 1, 2, 3, 4, 8):
            assert ax[k] == 0.0 and ay[k] == 0.0 and not math.copysign(1, ax[k]) < 0
        # inside: along the way to the centre for a positive strength, away for a negative one; linear falloff
        for k in (5, 6, 7):
            dx, dy = c[0] - x[k], c[1] - y[k]
            d = math.sqrt(dx * dx + dy * dy)
            s = strength * (1.0 - d / R)
            assert (ax[k], ay[k]) == (0.0 + (dx / d) * s, 0.0 + (dy / d) * s)
            assert (ax[k] * dx + ay[k] * dy > 0) == (strength > 0)
        assert math.hypot(ax[5], ay[5]) == pytest.approx(4000.0 * (1 - 5.0 / 80.0), rel=8 * U)  # (3, 4, 5)
        assert math.hypot(ax[6], ay[6]) == pytest.approx(2000.0, rel=8 * U)
    # a mask that does not cover the type: nothing, and nothing counted
    ax, ay, acts = fm.acceleration(x, y, fm.normalise([("radial", c[0], c[1], 4000.0, R, "yolk")]), 1)
    assert acts == 0 and not ax.any() and not ay.any()


def test_a_vortex_field_is_perpendicular_to_the_radius():
    rng = np.random.default_rng(7)
    c, R = (315.0, 296.0), 80.0
    x, y = c[0] + rng.uniform(-90, 90, 500), c[1] + rng.uniform(-90, 90, 500)
    f = fm.normalise([("vortex", c[0], c[1], 4000.0, R)])
    ax, ay, acts = fm.acceleration(x, y, f, 2)
    rx, ry, _ = fm.acceleration(x, y, fm.normalise([("radial", c[0], c[1], 4000.0, R)]), 2)
    dx, dy = c[0] - x, c[1] - y
    d = np.sqrt(dx * dx + dy * dy)
    inside = d < R
    assert acts == np.count_nonzero(inside) and 100 < acts < 500
    assert not ax[~inside].any() and not ay[~inside].any()
    # the radial field's acceleration turned by a quarter, bit for bit ...
    assert np.array_equal(ax, -ry) and np.array_equal(ay, rx)
    # ... so its product with the radius is two roundings of products of size |a| d away from 0
    a = np.hypot(ax, ay)
    assert np.all(np.abs(ax * dx + ay * dy)[inside] <= 8 * U * (a * d)[inside])
    assert np.allclose(a[inside], 4000.0 * (1.0 - d[inside] / R), rtol=16 * U, atol=0)
    # the sense: to the left of the centre (dx > 0, dy = 0) a positive strength accelerates along +y
    ax, ay, _ = fm.acceleration([c[0] - 20.0], [c[1]], f, 2)
    assert ax[0] == 0.0 and ay[0] == 4000.0 * (1.0 - 20.0 / R)


def test_masks_are_respected():
    free = _run(())
    white_only = _run((("uniform", 0.0, 980.0, "white"),))
    assert np.array_equal(free.state(YOLK), white_only.state(YOLK))
    assert not np.array_equal(free.state(WHITE), white_only.state(WHITE))
    yolk_only = _run((("radial", 310.0, 300.0, 4000.0, 80.0, "yolk"),))
    assert np.array_equal(free.state(WHITE), yolk_only.state(WHITE))
    assert not np.array_equal(free.state(YOLK), yolk_only.state(YOLK))
    assert yolk_only.force_acts[WHITE] == 0 and yolk_only.force_acts[YOLK] > 0
    both = _run((("uniform", 0.0, 980.0, "white"), ("radial", 310.0, 300.0, 4000.0, 80.0, "yolk")))
    assert np.array_equal(both.state(WHITE), white_only.state(WHITE))
    assert np.array_equal(both.state(YOLK), yolk_only.state(YOLK))
    # a field for both types acts on both
    ab = _run((("uniform", 0.1, 980.0), ("radial", 310.0, 300.0, 4000.0, 80.0)))
    assert min(ab.force_acts) > 0


def test_an_immovable_particle_takes_no_force():
    """masses of 3e8 .. 1e9: every white inverse mass is at most eps, the test the follow constraint itself uses"""
    heavy = (("min_mass", 3.0e8), ("max_mass", 1.0e9))
    fields = (("uniform", 0.0, 980.0), ("vortex", 310.0, 300.0, 4000.0, 80.0))
    free, forced = _run((), white=heavy), _run(fields, white=heavy)
    assert max(free.field(WHITE, rm.INV_MASS)) <= rm.EPS
    assert np.array_equal(free.state(WHITE), forced.state(WHITE))
    assert not np.array_equal(free.state(YOLK), forced.state(YOLK))
    assert forced.force_acts[WHITE] == 0 and forced.force_acts[YOLK] > 0
    assert _run(fields).force_acts[WHITE] > 0  # (the same fields do act on a white of ordinary mass)


def test_four_batches_rest_in_a_container_under_gravity():
    """60 steps: everything stays finite and inside the container, the last (here: only) collider, which holds to the
    bound of tests/test_collider_model.py: coordinates below 2^12, a projection a handful of roundings, 1e-9 px."""
    cx, cy, R = 50.0, 60.0, 150.0
    m = ForceModel()
    for x, y in [tuple(float(v) for v in c) for c in load_golden("four_batches")["centers"]]:
        m.add(x, y, 50, 15)
    m.set_colliders([("container", cx, cy, R)])
    m.set_forces([("uniform", 0.0, 980.0)])
    low = []
    for step in range(60):
        m.update(1 / 60, 1 / 60, 2, 3)
        for w in (WHITE, YOLK):
            st, r = m.state(w), np.asarray(m.field(w, rm.RADIUS), dtype=np.float64)
            assert np.isfinite(st).all(), (step, w)
            assert (np.hypot(st[0] - cx, st[1] - cy) - np.maximum(R - r, 0.0)).max() <= 1e-9, (step, w)
        low.append(float(np.mean(m.state(WHITE)[1])))
    assert sum(m.collider_hits) > 0
    # gravity acted: the whites hang lower (+y) than without it
    still = ForceModel()
    for x, y in [tuple(float(v) for v in c) for c in load_golden("four_batches")["centers"]]:
        still.add(x, y, 50, 15)
    still.set_colliders([("container", cx, cy, R)])
    for step in range(10):
        still.update(1 / 60, 1 / 60, 2, 3)
    assert low[9] > float(np.mean(still.state(WHITE)[1]))
