"""The definition of effective cohesion ("Cohesion") on the CPU: tests/cohesion_model.py against
tests/relaxed_model.py, against the closed form of one pair, and what it does to a batch's extent.  No device needed; the
device is held against the same model by tests/test_gpu_cohesion.py."""
import numpy as np
import pytest

from cohesion_model import CohesiveModel, cohesive_pass
from conftest import circle_target, load_golden
from relaxed_model import DEFAULT_RELAXATION, RelaxedModel, relaxed_pass, rm

WHITE, YOLK = 0, 1
S, C = 2, 3


def _run(model, steps, moving=True):
    centers = [tuple(c) for c in load_golden("four_batches")["centers"]]
    ids = [model.add(cx, cy, 50, 15) for cx, cy in centers]
    for k in range(steps):
        if moving:
            for i, c in zip(ids, centers):
                model.set_target_position(i, *circle_target(c, k))
        model.update(1 / 60, 1 / 60, S, C)
    return model


@pytest.fixture(scope="module")
def relaxed_20():
    return _run(RelaxedModel(relaxed=True), 20)


def test_off_equals_the_relaxed_model(relaxed_20):
    m = _run(CohesiveModel(cohesion=False), 20)
    for w in (WHITE, YOLK):
        assert np.array_equal(m.state(w), relaxed_20.state(w))
    assert m.pair_solves == relaxed_20.pair_solves and m.cohesion_solves == 0


def test_default_configs_on(relaxed_20):
    """white: both factors are 2, the band (md, reach] is empty; yolk: factor 3 against overlap 2, radius 4: 16 .. 24 px"""
    m = _run(CohesiveModel(cohesion=True), 20)
    assert np.array_equal(m.state(WHITE), relaxed_20.state(WHITE))
    assert not np.array_equal(m.state(YOLK), relaxed_20.state(YOLK))
    assert m.cohesion_solves > 0
    assert np.isfinite(m.state(YOLK)).all()


# one pair: equal inverse mass w, radius 4, overlap 2 -> md = 16; factor 3 -> reach = 24
W_INV, RADIUS, OVERLAP, FACTOR = 0.8, 4.0, 2.0, 3.0
ALPHA_COL, ALPHA_COH = 0.25, 0.125 / (1 / 120) ** 2 * 1e-4  # two different compliances, neither zero


def _pair_pass(d, batches=(7, 7), cohesion_compliance=ALPHA_COH, angle=0.7, omega=DEFAULT_RELAXATION):
    x = np.array([100.0, 100.0 + d * np.cos(angle)])
    y = np.array([50.0, 50.0 + d * np.sin(angle)])
    w = np.array([W_INV, W_INV])
    r = np.array([RADIUS, RADIUS])
    cell = 12.0
    cx, cy = np.floor(x / cell).astype(np.int64), np.floor(y / cell).astype(np.int64)
    assert abs(cx[0] - cx[1]) <= 1 and abs(cy[0] - cy[1]) <= 1  # candidates of each other
    out = cohesive_pass(x, y, w, r, cx, cy, np.array(batches), OVERLAP, ALPHA_COL, omega, FACTOR,
                        cohesion_compliance)
    return x, y, cx, cy, w, r, out


@pytest.mark.parametrize("d", [16.5, 20.0, 23.75])
def test_one_pair_in_the_band(d):
    x, y, _cx, _cy, _w, _r, (nx, ny, pairs, cohered) = _pair_pass(d)
    assert (pairs, cohered) == (1, 1)
    md = OVERLAP * (RADIUS + RADIUS)
    want = DEFAULT_RELAXATION * W_INV * (d - md) / (2 * W_INV + ALPHA_COH)  # n_i = 1
    ux, uy = (x[1] - x[0]) / d, (y[1] - y[0]) / d
    move0 = (nx[0] - x[0]) * ux + (ny[0] - y[0]) * uy     # along the axis, toward the other
    move1 = -((nx[1] - x[1]) * ux + (ny[1] - y[1]) * uy)
    # (1e-12 relative: the positions, near 100, carry 2^-46 px of rounding, some 1e-13 of the smallest move here)
    print("d = %g: moves %.17g, %.17g, closed form %.17g" % (d, move0, move1, want))
    assert abs(move0 - want) <= 1e-12 * want and abs(move1 - want) <= 1e-12 * want
    # the constraint's own correction (omega = 1) never brings the pair closer than the collision distance, however
    # stiff: each side moves w (d - md) / (2 w + alpha) <= (d - md) / 2.  (omega > 1 over-relaxes it, as it does a collision.)
    _, _, _, _, _, _, (sx, sy, _, _) = _pair_pass(d, cohesion_compliance=0.0, omega=1.0)
    assert np.hypot(sx[1] - sx[0], sy[1] - sy[0]) >= md * (1 - 1e-15)
    assert abs((nx[0] - x[0]) * -uy + (ny[0] - y[0]) * ux) <= 1e-12 * want  # nothing off the axis


def test_outside_the_band_nothing_moves():
    for d, batches in ((20.0, (7, 8)), (24.5, (7, 7)), (24.5, (7, 8))):
        x, y, _cx, _cy, _w, _r, (nx, ny, pairs, cohered) = _pair_pass(d, batches)
        assert (pairs, cohered) == (1, 0)
        assert np.array_equal(nx, x) and np.array_equal(ny, y)


@pytest.mark.parametrize("d", [0.0, 3.0, 16.0])
def test_a_colliding_pair_gets_the_collision_correction(d):
    """d <= md: bit-equal with cohesion on (same batch or not) and off, whatever the cohesion compliance"""
    x, y, cx, cy, w, r, (nx, ny, pairs, cohered) = _pair_pass(d)
    assert (pairs, cohered) == (1, 0)
    ox, oy, opairs = relaxed_pass(x, y, w, r, cx, cy, OVERLAP, ALPHA_COL, DEFAULT_RELAXATION)
    assert opairs == 1 and np.array_equal(nx, ox) and np.array_equal(ny, oy)
    assert d == 16.0 or not np.array_equal(nx, x)  # (at d = md exactly the violation is zero)
    _, _, _, _, _, _, (nx2, ny2, _, cohered2) = _pair_pass(d, (7, 8), cohesion_compliance=0.0)
    assert cohered2 == 0 and np.array_equal(nx2, ox) and np.array_equal(ny2, oy)


def _configs(**white):
    w, y = rm.default_configs()
    return dict(w, **white), y


def _white_extents(m):
    st = m.state(WHITE)
    n = st.shape[1] // 4
    out = []
    for b in range(4):
        x, y = st[0, b * n:(b + 1) * n], st[1, b * n:(b + 1) * n]
        out.append(float(np.sqrt(np.mean((x - x.mean()) ** 2 + (y - y.mean()) ** 2))))
    return out


def test_extent_falls_with_strength():
    """white factor 3 (band 16 .. 24 px at radius 4), 60 steps: every batch's white rms extent is smaller with cohesion
    on than off, not larger at a higher strength, and everything stays finite"""
    off = _run(RelaxedModel(*_configs(cohesion_interaction_distance_factor=3), relaxed=True), 60)
    assert np.isfinite(off.state(WHITE)).all()
    prev, e_off = None, _white_extents(off)
    for strength in (0.8, 0.99, 1.0):
        m = _run(CohesiveModel(*_configs(cohesion_interaction_distance_factor=3, cohesion_strength=strength),
                               cohesion=True), 60)
        for w in (WHITE, YOLK):
            assert np.isfinite(m.state(w)).all()
        e = _white_extents(m)
        print("strength %g: white rms extent per batch %s (off: %s), %d cohesion pairs" %
              (strength, ["%.1f" % v for v in e], ["%.1f" % v for v in e_off], m.cohesion_solves))
        assert all(a < b for a, b in zip(e, e_off)), (strength, e, e_off)
        if prev is not None:
            assert all(a <= b for a, b in zip(e, prev)), (strength, e, prev)
        prev = e
