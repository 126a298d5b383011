"""tests/collider_model.py, the definition of the static colliders of the relaxed pass ("Colliders"),
against what the definition promises: a single collider holds after every step, the way out of a disc's centre, the
zero-length segment, the type mask, the empty list and the list order.  No device needed.

The bound of the single-collider tests: coordinates stay below 2^12, so one rounding is below 2^-41 < 1e-12 px; a
projection is a handful of roundings, and 1e-9 px leaves three orders of magnitude of margin."""
import functools

import numpy as np
import pytest

import collider_model as cm
from cohesion_model import CohesiveModel
from collider_model import ColliderModel
from relaxed_model import DIRS, rm

WHITE, YOLK = 0, 1
TOL = 1e-9
WHITE3 = dict(cohesion_interaction_distance_factor=3, cohesion_strength=0.99)

# a default egg is added at (300, 300) and keeps that target: beyond the half-plane, on the disc, outside the container,
# across the wall
SINGLE = {
    "half_plane": ("half_plane", 2.0, 0.0, 320.0),
    "disc": ("disc", 300.0, 300.0, 30.0),
    "container": ("container", 400.0, 300.0, 60.0),
    "segment": ("segment", 250.0, 310.0, 350.0, 310.0),
}


def _violation(collider, x, y, r):
    """by how much every particle violates the (normalised) collider, in px: <= 0 where it holds"""
    kind, p0, p1, p2, p3, _mask = collider
    if kind == "half_plane":
        return r - ((p0 * x + p1 * y) - p2)
    if kind == "disc":
        return (p2 + r) - np.hypot(x - p0, y - p1)
    if kind == "container":
        return np.hypot(x - p0, y - p1) - np.maximum(p2 - r, 0.0)
    ex, ey = p2 - p0, p3 - p1
    t = np.clip(((x - p0) * ex + (y - p1) * ey) / (ex * ex + ey * ey), 0.0, 1.0)
    return r - np.hypot(x - (p0 + t * ex), y - (p1 + t * ey))


def _fields(m, w):
    return m.state(w), np.asarray(m.field(w, rm.RADIUS), dtype=np.float64)


@pytest.mark.parametrize("kind", sorted(SINGLE))
def test_a_single_collider_holds_after_every_step(kind):
    m = ColliderModel()
    m.add(300.0, 300.0, 50, 15)
    m.set_colliders([SINGLE[kind]])
    worst = -np.inf
    for step in range(30):
        m.update(1 / 60, 1 / 60, 2, 3)
        for w in (WHITE, YOLK):
            st, r = _fields(m, w)
            assert np.abs(st[:2]).max() < 2.0 ** 12
            v = _violation(m.colliders[0], st[0], st[1], r).max()
            worst = max(worst, v)
            assert v <= TOL, "%s: step %d type %d violates by %g px" % (kind, step + 1, w, v)
    print("%s: worst violation %g px, hits %s" % (kind, worst, m.collider_hits))
    assert sum(m.collider_hits) > 0


def test_a_particle_on_a_discs_centre_leaves_along_its_direction():
    n = 19
    x, y, r = np.full(n, 12.5), np.full(n, -3.25), np.linspace(1.0, 4.0, n)
    px, py, hits = cm.project(x, y, r, cm.normalise([("disc", 12.5, -3.25, 6.0)]), 1)
    assert hits == n
    k = np.arange(n) & 7
    assert np.array_equal(px, 12.5 + DIRS[k, 0] * (6.0 + r)) and np.array_equal(py, -3.25 + DIRS[k, 1] * (6.0 + r))
    # the key picks the direction, not the place in the arrays
    qx, qy, _ = cm.project(x, y, r, cm.normalise([("disc", 12.5, -3.25, 6.0)]), 1, idx=np.arange(n) + 5)
    assert np.array_equal(qx[:-5], 12.5 + DIRS[k[5:], 0] * (6.0 + r[:-5]))
    # the same inside a model: the first white particle starts exactly on the centre
    m = ColliderModel()
    m.add(100.0, 100.0, 28, 28, 2, 2)
    st, rad = _fields(m, WHITE)
    m.set_colliders([("disc", st[0][0], st[1][0], 0.0, "white")])
    ex, ey, _ = cm.project(st[0], st[1], rad, m.colliders, 1)
    assert (ex[0], ey[0]) == (st[0][0] + 1.0 * rad[0], st[1][0] + 0.0 * rad[0])
    # a NaN position is left alone by every kind
    nan = np.array([np.nan])
    for c in SINGLE.values():
        ox, oy, h = cm.project(nan, nan, [2.0], cm.normalise([c]), 1)
        assert np.isnan(ox[0]) and np.isnan(oy[0]) and h == 0


@functools.lru_cache(maxsize=None)
def _run(colliders, cohesion=False, steps=6, cls=ColliderModel):
    w, y = rm.default_configs()
    m = cls(dict(w, **WHITE3), y, cohesion=cohesion)
    m.add(300.0, 300.0, 50, 15)
    if colliders is not None:
        m.set_colliders(list(colliders))
    for _ in range(steps):
        m.update(1 / 60, 1 / 60, 2, 3)
    return m


def test_a_zero_length_segment_is_a_disc_of_radius_zero():
    a, b = _run((("segment", 310.0, 300.0, 310.0, 300.0),)), _run((("disc", 310.0, 300.0, 0.0),))
    for w in (WHITE, YOLK):
        assert np.array_equal(a.state(w), b.state(w))
    assert a.collider_hits == b.collider_hits and sum(a.collider_hits) > 0


def test_a_white_only_collider_leaves_the_yolk_alone():
    free, held = _run(()), _run((("disc", 300.0, 300.0, 30.0, "white"),))
    assert np.array_equal(free.state(YOLK), held.state(YOLK))
    assert not np.array_equal(free.state(WHITE), held.state(WHITE))
    assert held.collider_hits[WHITE] > 0 and held.collider_hits[YOLK] == 0
    both = _run((("disc", 300.0, 300.0, 30.0),))
    assert both.collider_hits[YOLK] > 0 and np.array_equal(both.state(WHITE), held.state(WHITE))


@pytest.mark.parametrize("cohesion", [False, True])
def test_an_empty_list_is_the_cohesive_model(cohesion):
    a, b = _run((), cohesion), _run(None, cohesion, cls=CohesiveModel)
    for w in (WHITE, YOLK):
        assert np.array_equal(a.state(w), b.state(w))
    assert (a.pair_solves, a.cohesion_solves) == (b.pair_solves, b.cohesion_solves) and a.collider_hits == [0, 0]
    assert (a.cohesion_solves > 0) == cohesion


def test_the_list_order_matters():
    plane, disc = ("half_plane", 1.0, 0.0, 290.0), ("disc", 300.0, 300.0, 30.0)
    a, b = _run((plane, disc)), _run((disc, plane))
    assert not np.array_equal(a.state(WHITE), b.state(WHITE))
    # the last collider holds exactly, the one before it only approximately
    for m, last, first in ((a, 1, 0), (b, 1, 0)):
        st, r = _fields(m, WHITE)
        assert _violation(m.colliders[last], st[0], st[1], r).max() <= TOL
        assert _violation(m.colliders[first], st[0], st[1], r).max() > TOL
