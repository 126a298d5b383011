"""tests/viscosity_model.py, the definition of the viscosity of the relaxed step ("Viscosity"), against
what the definition promises: c = 0 is the parent model, a particle without a neighbour keeps its bits, a coincident pair
ends with equal displacements at c = 1, the blend is convex, and the jitter of section 2.7 falls with c.  No device needed."""
import functools

import numpy as np
import pytest

from conftest import load_golden
from force_model import ForceModel
from relaxed_model import rm
from viscosity_model import ViscosityModel, xsph

WHITE, YOLK = 0, 1
SCENE = (("container", 50.0, 60.0, 150.0), ("half_plane", 0.0, 3.0, -30.0))
FORCES = (("uniform", 0.0, 980.0),)


def _centers():
    return [tuple(float(v) for v in c) for c in load_golden("four_batches")["centers"]]


def _play(m, steps, S=2, C=3):
    ids = [m.add(x, y, 50, 15) for x, y in _centers()[:2]]
    for _ in range(steps):
        m.update(1 / 60, 1 / 60, S, C)
    return ids


@pytest.mark.parametrize("cohesion", [False, True])
def test_zero_coefficients_are_the_parent_model(cohesion):
    w, y = rm.default_configs()
    w = dict(w, cohesion_interaction_distance_factor=3, cohesion_strength=0.99)
    a, b, c = ViscosityModel(w, y, cohesion=cohesion), ForceModel(w, y, cohesion=cohesion), ViscosityModel(w, y, cohesion=cohesion)
    for m in (a, b, c):
        m.set_colliders(list(SCENE))
        m.set_forces(list(FORCES))
    a.set_viscosity(0.0, 0.0)
    c.set_viscosity(0.5, 0.25)
    for m in (a, b, c):
        _play(m, 4)
    for t in (WHITE, YOLK):
        assert np.array_equal(a.state(t), b.state(t))
        assert not np.array_equal(c.state(t), b.state(t))  # (and a coefficient changes the committed state)
    assert (a.pair_solves, a.cohesion_solves, a.collider_hits) == (b.pair_solves, b.cohesion_solves, b.collider_hits)
    assert a.viscosity_pairs == [0, 0] and min(c.viscosity_pairs) > 0


def test_one_type_only():
    """white on, yolk off: the yolk is the parent's, bit for bit, and counts no pair"""
    a, b = ViscosityModel(), ForceModel()
    a.set_viscosity(1.0, 0.0)
    for m in (a, b):
        _play(m, 4)
    assert np.array_equal(a.state(YOLK), b.state(YOLK)) and not np.array_equal(a.state(WHITE), b.state(WHITE))
    assert a.viscosity_pairs[YOLK] == 0 < a.viscosity_pairs[WHITE]
    # positions within a sub-step are untouched: the last sub-step's pass changes the velocity alone, so after ONE step of
    # one sub-step the positions are the parent's and the velocities are not
    a, b = ViscosityModel(), ForceModel()
    a.set_viscosity(1.0, 1.0)
    for m in (a, b):
        _play(m, 1, S=1)
    for t in (WHITE, YOLK):
        assert np.array_equal(a.state(t)[:2], b.state(t)[:2]) and not np.array_equal(a.state(t)[2:4], b.state(t)[2:4])
    assert a.pair_solves == b.pair_solves


def test_a_particle_without_a_neighbour_keeps_its_bits():
    H = 8.0
    px, py = np.array([0.1]), np.array([0.7])
    npx, npy, pairs, _, _ = xsph([1.3], [2.9], px, py, [1.0], H, 1.0)
    assert npx.tobytes() == px.tobytes() and npy.tobytes() == py.tobytes() and pairs == 0
    # two particles exactly H apart (d2 < H H is false), two in cells that are not neighbours, and an immovable one beside
    # a neighbour: prev is not recomputed (x - (x - px) would round differently)
    x = np.array([0.1, 0.1 + H, 100.3, 100.3 + 3 * H, 50.1, 50.9])
    y = np.array([0.3, 0.3, 7.7, 7.7, 20.3, 20.4])
    px = 1e-3 / np.array([3.0, 7.0, 11.0, 13.0, 17.0, 19.0])  # (far from x: x - (x - px) loses px's low bits)
    py = y - np.array([0.021, 0.4, -0.19, 0.23, 0.1, 0.9])
    im = np.array([1.0, 1.0, 1.0, 1.0, 0.0, 1.0])
    assert (x[1] - x[0]) ** 2 == H * H
    npx, npy, pairs, _, _ = xsph(x, y, px, py, im, H, 1.0)
    assert npx[:5].tobytes() == px[:5].tobytes() and npy[:5].tobytes() == py[:5].tobytes()
    assert pairs == 1 and npx[5] != px[5]  # (the immovable particle still smooths its neighbour)
    assert np.all(x[:5] - (x[:5] - px[:5]) != px[:5])  # the case tells "keeps its bits" from "is recomputed"
    # NaN: every comparison is false, nothing moves and nothing is counted
    nan = float("nan")
    npx, npy, pairs, _, _ = xsph([nan, 1.0], [0.0, 0.0], [0.5, 0.5], [0.0, 0.0], [1.0, 1.0], H, 1.0)
    assert npx.tobytes() == np.array([0.5, 0.5]).tobytes() and pairs == 0


def test_two_coincident_particles_end_with_equal_displacements():
    x, y = np.array([3.0, 3.0]), np.array([4.0, 4.0])
    u = np.array([[0.25, -0.5], [-0.25, 0.5]])  # opposite displacements
    npx, npy, pairs, nux, nuy = xsph(x, y, x - u[:, 0], y - u[:, 1], [1.0, 1.0], 8.0, 1.0)
    assert pairs == 1
    # w = 1 - 0 / H = 1, sw = 1: each takes the other's displacement at c = 1 ...
    assert nux[0] == -0.25 and nux[1] == 0.25 and nuy[0] == 0.5 and nuy[1] == -0.5
    # ... and at c = 0.5 both end with the mean, equal ones
    _, _, _, hx, hy = xsph(x, y, x - u[:, 0], y - u[:, 1], [1.0, 1.0], 8.0, 0.5)
    assert hx[0] == hx[1] == 0.0 and hy[0] == hy[1] == 0.0
    # three coincident particles at c = 1: each ends with the mean of the two others
    x, y = np.full(3, 3.0), np.full(3, 4.0)
    ux = np.array([0.5, -0.25, 0.125])
    _, _, pairs, nux, _ = xsph(x, y, x - ux, y, np.ones(3), 8.0, 1.0)
    assert pairs == 3 and list(nux) == [(-0.25 + 0.125) / 2, (0.5 + 0.125) / 2, (0.5 - 0.25) / 2]
    assert (x - (x - ux)).tobytes() == ux.tobytes()  # (the displacements above are exact)


@pytest.mark.parametrize("c", [0.25, 0.5, 1.0])
def test_the_blend_is_convex(c):
    """each component of a particle's new u lies within the min / max of that component over the particle and its
    neighbours within H -- up to the rounding of the blend: u + c (s / sw) is three roundings of values no larger than the
    neighbourhood's span, so 4 ulps of the largest |u| bound the excess."""
    rng = np.random.default_rng(7)
    n, H = 300, 8.0
    x, y = rng.uniform(0.0, 60.0, n), rng.uniform(0.0, 60.0, n)
    ux, uy = rng.normal(0.0, 0.5, n), rng.normal(0.0, 0.5, n)
    im = np.ones(n)
    px, py = x - ux, y - uy
    ux, uy = x - px, y - py  # (as the pass takes them)
    _, _, pairs, nux, nuy = xsph(x, y, px, py, im, H, c)
    d2 = (x[:, None] - x[None, :]) ** 2 + (y[:, None] - y[None, :]) ** 2
    near = d2 < H * H  # (the particle itself included)
    assert pairs == (int(near.sum()) - n) // 2 > n
    slack = 4 * np.finfo(np.float64).eps * float(np.max(np.abs(np.concatenate([ux, uy]))))
    for u, nu in ((ux, nux), (uy, nuy)):
        lo = np.where(near, u[None, :], np.inf).min(axis=1)
        hi = np.where(near, u[None, :], -np.inf).max(axis=1)
        assert np.all(nu >= lo - slack) and np.all(nu <= hi + slack)
        assert float(np.ptp(nu)) < float(np.ptp(u))  # and the spread shrank


@functools.lru_cache(maxsize=None)
def _rest(c):
    """four_batches, S = 2, C = 3, 60 steps without target motion at coefficient c on both types"""
    m = ViscosityModel()
    ids = [m.add(x, y, 50, 15) for x, y in _centers()]
    m.set_viscosity(c, c)
    for _ in range(60):
        m.update(1 / 60, 1 / 60, 2, 3)
    return m, ids


def _jitter(m, w, n_batches=4):
    """section 2.7's metric: the mean speed of a particle relative to its batch"""
    s = m.state(w)
    n = s.shape[1] // n_batches
    rel = [np.hypot(s[2][k * n:(k + 1) * n] - s[2][k * n:(k + 1) * n].mean(), s[3][k * n:(k + 1) * n] - s[3][k * n:(k + 1) * n].mean())
           for k in range(n_batches)]
    return float(np.concatenate(rel).mean())


def test_the_jitter_falls_with_the_coefficient():
    """Section 2.7's jitter metric (white, as its omega table: 8.5 px/s at omega = 1.8) falls monotonically over c in
    {0, 0.25, 0.5, 1}, and the batches stay where the c = 0 run has them: the largest batch-centroid distance stays below a
    tenth of the smallest white batch extent (x extent + y extent) of the c = 0 run.  Nothing is asserted about absolute
    values.  Measured (DESIGN.md has the table): white 8.49 / 6.20 / 5.60 / 4.12 px/s, centroid distance 0 / 2.03 / 3.30 /
    4.76 px against extents of 138 px and more.  The yolk's 60 particles are printed, not asserted: 8.20 / 4.97 / 3.93 /
    5.42 px/s, not monotonic at c = 1."""
    base, ids = _rest(0.0)
    s = base.state(WHITE)
    n = s.shape[1] // 4
    extent = min(float(np.ptp(s[0][k * n:(k + 1) * n]) + np.ptp(s[1][k * n:(k + 1) * n])) for k in range(4))
    p0 = np.array([base.get_position(i) for i in ids])
    last = None
    for c in (0.0, 0.25, 0.5, 1.0):
        m, _ = _rest(c)
        assert not np.isnan(m.state(WHITE)).any() and not np.isnan(m.state(YOLK)).any()
        j = _jitter(m, WHITE)
        far = float(np.max(np.hypot(*(np.array([m.get_position(i) for i in ids]) - p0).T)))
        print("c = %.2f: white jitter %.3f px/s, yolk %.3f px/s, centroid distance %.3f px of %.1f px, pairs %s"
              % (c, j, _jitter(m, YOLK), far, extent, m.viscosity_pairs))
        assert last is None or j < last, c
        assert far < 0.1 * extent, c
        assert (min(m.viscosity_pairs) > 0) == (c > 0)
        last = j
