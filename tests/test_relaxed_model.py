"""The relaxed-order CPU model (tests/relaxed_model.py): the subclass leaves the exact path
alone, hand-checked single pairs, and the quality of the relaxed result against the exact oracle.  No GPU needed."""
import math

import numpy as np

from conftest import circle_target, load_golden
from relaxed_model import DEFAULT_RELAXATION, DIRS, RelaxedModel, pair_shares, relaxed_pass

WHITE, YOLK = 0, 1
OVERLAP, COMPLIANCE = 2.0, (1 - (1 - 0.0025)) / (1 / 120) ** 2  # white defaults at S = 2, delta = 1/60


def _drive(sim, centers, steps, moving=True, S=2, C=3):
    ids = [sim.add(cx, cy, 50, 15) for cx, cy in centers]
    for k in range(steps):
        if moving:
            for i, c in zip(ids, centers):
                sim.set_target_position(i, *circle_target(c, k))
        sim.update(1 / 60, 1 / 60, S, C)
    return ids


def _oracle_state(o, w):
    return np.array([o.field(w, f) for f in ("x", "y", "vx", "vy", "last_x", "last_y")])


def test_flag_off_equals_oracle(oracle_mod):
    centers = [tuple(c) for c in load_golden("four_batches")["centers"]]
    m, o = RelaxedModel(relaxed=False), oracle_mod.Oracle()
    _drive(m, centers, 4)
    _drive(o, centers, 4)
    for w in (WHITE, YOLK):
        assert np.array_equal(m.state(w), _oracle_state(o, w))
    assert m.pair_solves == o.total_visited


def test_two_particle_overlap():
    # equal masses: each particle takes its own share, half of the separation the pair is short of
    x, y = np.array([10.0, 13.0]), np.array([5.0, 5.0])
    w, r = np.array([1.0, 1.0]), np.array([4.0, 4.0])
    nx, ny, pairs = relaxed_pass(x, y, w, r, [1, 1], [0, 0], OVERLAP, COMPLIANCE, 1.0)
    cax, cay, cbx, cby, counted, fired = pair_shares(10.0, 5.0, 13.0, 5.0, 1.0, 1.0, 4.0, 4.0, 1, OVERLAP, COMPLIANCE)
    assert bool(fired) and pairs == 1
    assert nx[0] == 10.0 + float(cax) and nx[1] == 13.0 + float(cbx)
    assert ny[0] == 5.0 + float(cay) and ny[1] == 5.0 + float(cby)
    assert float(cax) == -float(cbx) and float(cax) < 0
    gap = 16.0 - 3.0
    assert math.isclose(-float(cax), gap / 2 * 2 / (2 + COMPLIANCE), rel_tol=1e-12)


def test_coincident_pair_separates_along_dirs():
    for da in (1, 2, 3, 5, 7, 8):
        x = np.zeros(da + 1)
        y = np.zeros(da + 1)
        x[1:da] = 1000.0 * np.arange(1, da)  # fillers far away: particles 0 and da are the coincident pair
        w, r = np.ones(da + 1), np.full(da + 1, 4.0)
        cx = np.floor(x / 8.0).astype(np.int64)
        nx, ny, _ = relaxed_pass(x, y, w, r, cx, np.zeros(da + 1, dtype=np.int64), OVERLAP, COMPLIANCE, 1.0)
        d = DIRS[da & 7]
        step = (nx[da] - nx[0], ny[da] - ny[0])
        assert step[0] * d[0] + step[1] * d[1] > 0  # b moved away from a along DIRS[(b - a) & 7]
        assert abs(step[0] * d[1] - step[1] * d[0]) < 1e-12
        assert nx[0] == -nx[da] and ny[0] == -ny[da]


def test_three_in_a_row_averages():
    # a - b - c, 6 px apart, min distance 16: b's two shares cancel, a and c each have ONE pair with b and one with
    # each other, and move by the mean of their two shares
    x, y = np.array([0.0, 6.0, 12.0]), np.zeros(3)
    w, r = np.ones(3), np.full(3, 4.0)
    cx = np.zeros(3, dtype=np.int64)
    for omega in (1.0, DEFAULT_RELAXATION):
        nx, ny, pairs = relaxed_pass(x, y, w, r, cx, cx, OVERLAP, COMPLIANCE, omega)
        assert pairs == 3
        ab = pair_shares(0.0, 0.0, 6.0, 0.0, 1.0, 1.0, 4.0, 4.0, 1, OVERLAP, COMPLIANCE)
        ac = pair_shares(0.0, 0.0, 12.0, 0.0, 1.0, 1.0, 4.0, 4.0, 2, OVERLAP, COMPLIANCE)
        bc = pair_shares(6.0, 0.0, 12.0, 0.0, 1.0, 1.0, 4.0, 4.0, 1, OVERLAP, COMPLIANCE)
        assert nx[0] == 0.0 + ((0.0 + float(ab[0]) + float(ac[0])) * omega) / 2.0
        assert nx[1] == 6.0 + ((0.0 + float(ab[2]) + float(bc[0])) * omega) / 2.0
        assert nx[2] == 12.0 + ((0.0 + float(ac[2]) + float(bc[2])) * omega) / 2.0
        assert nx[1] == 6.0 and np.all(ny == 0.0)
        assert nx[0] < 0.0 and nx[2] > 12.0


def _max_overlap(x, y, r, factor=2.0):
    d = np.hypot(x[:, None] - x[None, :], y[:, None] - y[None, :])
    np.fill_diagonal(d, np.inf)
    return float(np.max(factor * (r[:, None] + r[None, :]) - d))


def test_quality_against_exact_oracle(oracle_mod):
    """four_batches with moving targets, 60 steps, at the default relaxation.  Observed (omega = 1.8): largest
    per-batch centroid distance from the exact path 12.81 px; largest white overlap depth 15.60 px (exact 14.95);
    white batch extents 0.63..0.76 of the exact path's."""
    centers = [tuple(c) for c in load_golden("four_batches")["centers"]]
    o, m = oracle_mod.Oracle(), RelaxedModel(relaxed=True)
    ids_o = _drive(o, centers, 60)
    ids_m = _drive(m, centers, 60)
    ref = np.array([o.get_position(i) for i in ids_o])
    got = np.array([m.get_position(i) for i in ids_m])
    assert np.all(np.isfinite(got))
    assert float(np.max(np.hypot(*(got - ref).T))) < 20.0
    for w, n in ((WHITE, 157), (YOLK, 15)):
        s = m.state(w)
        assert not np.isnan(s).any()
        xo, yo = o.positions(w)
        r = np.array(o.field(w, "radius"))
        assert _max_overlap(s[0], s[1], r) < 15.9
        for k in range(len(centers)):
            sl = slice(k * n, (k + 1) * n)
            e_m = np.ptp(s[0][sl]) + np.ptp(s[1][sl])
            e_o = np.ptp(np.asarray(xo)[sl]) + np.ptp(np.asarray(yo)[sl])
            assert 0.45 * e_o < e_m < 1.5 * e_o, (w, k, e_m, e_o)


def test_coincident_batches_separate():
    m = RelaxedModel(relaxed=True)
    for _ in range(4):
        m.add(300.0, 300.0, 50, 15)
    for _ in range(10):
        m.update(1 / 60, 1 / 60, 2, 3)
    for w in (WHITE, YOLK):
        s = m.state(w)
        n = m.n_particles(w) // 4
        for a in range(4):
            for b in range(a + 1, 4):
                d = np.hypot(s[0][a * n:(a + 1) * n] - s[0][b * n:(b + 1) * n], s[1][a * n:(a + 1) * n] - s[1][b * n:(b + 1) * n])
                assert float(d.min()) > 0.0

