"""tests/coupling_model.py, the definition of the white-yolk coupling pass (egg_set_coupling; DESIGN.md section 2.7,
"Coupling"), checked on the CPU: known answers by hand, the branches of the pair arithmetic, the plumbing of strength and
sub-step, off = ViscosityModel bit for bit, and the effect on an egg that rests on a floor."""
import functools

import numpy as np

import coupling_model
from conftest import circle_target
from coupling_model import CouplingModel, coupling_pass
from relaxed_model import DEFAULT_RELAXATION, DIRS, rm
from viscosity_model import ViscosityModel

WHITE, YOLK = 0, 1
OMEGA = DEFAULT_RELAXATION


def _cols(*particles):
    """(x, y, inverse mass, radius) arrays of particles given as tuples"""
    return tuple(np.array(c, dtype=np.float64) for c in zip(*particles))


def test_known_answer_pair():
    """one white and one yolk particle 4 px apart, radii 3 and 2, factor 1: md = 5, violation = -1, divisor = 1.5"""
    white, yolk = _cols((0.0, 0.0, 1.0, 3.0)), _cols((4.0, 0.0, 0.5, 2.0))
    (wx, wy), (yx, yy), solves, coincident = coupling_pass(white, yolk, 4.0, 4.0, 1.0, 0.0, OMEGA)
    correction = -(4.0 - 5.0) / (1.0 + 0.5)  # below the clamp |violation| = 1
    cax, cbx = -1.0 * correction * 1.0, 1.0 * correction * 0.5
    assert (solves, coincident) == (1, 0)
    assert wx[0] == 0.0 + (cax * OMEGA) / 1.0 and wy[0] == 0.0
    assert yx[0] == 4.0 + (cbx * OMEGA) / 1.0 and yy[0] == 0.0
    assert wx[0] < 0.0 < 4.0 < yx[0]  # pushed apart
    # a second yolk particle on the other side: the white one averages two shares (n = 2), each yolk one keeps n = 1; the
    # visit order inside the one cell is ascending yolk index
    yolk2 = _cols((4.0, 0.0, 0.5, 2.0), (0.0, -3.0, 0.5, 2.0))
    (wx, wy), (yx, yy), solves, _ = coupling_pass(white, yolk2, 4.0, 4.0, 1.0, 0.0, OMEGA)
    c2 = -(3.0 - 5.0) / 1.5
    assert solves == 2
    assert wx[0] == ((0.0 + cax) * OMEGA) / 2.0 and wy[0] == ((0.0 + -(-1.0) * c2 * 1.0) * OMEGA) / 2.0
    assert yx[0] == 4.0 + (cbx * OMEGA) / 1.0 and yy[1] == -3.0 + ((-1.0 * c2 * 0.5) * OMEGA) / 1.0
    # the clamp: a light pair cannot overshoot, |correction| <= |violation|
    (wx, _), (yx, _), _, _ = coupling_pass(_cols((0.0, 0.0, 0.25, 3.0)), _cols((4.0, 0.0, 0.25, 2.0)), 4.0, 4.0, 1.0, 0.0, OMEGA)
    assert wx[0] == 0.0 + ((-1.0 * 1.0 * 0.25) * OMEGA) / 1.0  # -violation / 0.5 = 2 clamped to 1
    # beyond the coupling distance nothing fires and the positions are copied
    (wx, wy), (yx, yy), solves, _ = coupling_pass(white, _cols((5.5, 0.0, 0.5, 2.0)), 4.0, 4.0, 1.0, 0.0, OMEGA)
    assert solves == 0 and (wx[0], wy[0], yx[0], yy[0]) == (0.0, 0.0, 5.5, 0.0)
    # ... and factor 2 reaches it: md = 10
    _, _, solves, _ = coupling_pass(white, _cols((5.5, 0.0, 0.5, 2.0)), 4.0, 4.0, 2.0, 0.0, OMEGA)
    assert solves == 1


def test_pairs_across_cells_and_negative_cells():
    """H = max(1, 1 * (3 + 2)) = 5: a pair across the cell edge at 0 (cells -1 and 0) fires, on both sides"""
    white, yolk = _cols((-0.5, -0.5, 1.0, 3.0)), _cols((0.5, 0.5, 1.0, 2.0))
    (wx, wy), (yx, yy), solves, _ = coupling_pass(white, yolk, 3.0, 2.0, 1.0, 0.0, OMEGA)
    assert solves == 1 and wx[0] < -0.5 and wy[0] < -0.5 and yx[0] > 0.5 and yy[0] > 0.5


def test_coincident_pair_normal():
    """d2 == 0: the normal is DIRS[(b - a) & 7] with a the white index and b the yolk index"""
    far = (1000.0, 1000.0, 1.0, 2.0)
    for a, b in ((0, 3), (2, 0), (1, 1), (0, 7), (3, 1)):
        white = [(-1000.0 - k, 0.0, 1.0, 3.0) for k in range(a)] + [(1.0, 1.0, 1.0, 3.0)]
        yolk = [(far[0] + k,) + far[1:] for k in range(b)] + [(1.0, 1.0, 1.0, 2.0)]
        (wx, wy), (yx, yy), solves, coincident = coupling_pass(_cols(*white), _cols(*yolk), 3.0, 2.0, 1.0, 0.0, OMEGA)
        nx, ny = DIRS[(b - a) & 7]
        correction = -(0.0 - 5.0) / 2.0
        assert (solves, coincident) == (1, 1)
        assert wx[a] == 1.0 + ((-nx * correction * 1.0) * OMEGA) / 1.0 and wy[a] == 1.0 + ((-ny * correction * 1.0) * OMEGA) / 1.0
        assert yx[b] == 1.0 + ((nx * correction * 1.0) * OMEGA) / 1.0 and yy[b] == 1.0 + ((ny * correction * 1.0) * OMEGA) / 1.0


def test_massless_pair_is_skipped():
    """wsum < eps: the pair is skipped and not counted; a pair of which one side has mass fires and moves that side only"""
    white, yolk = _cols((0.0, 0.0, 0.0, 3.0)), _cols((1.0, 0.0, 0.0, 2.0))
    (wx, wy), (yx, yy), solves, _ = coupling_pass(white, yolk, 3.0, 2.0, 1.0, 0.0, OMEGA)
    assert solves == 0 and (wx[0], wy[0], yx[0], yy[0]) == (0.0, 0.0, 1.0, 0.0)
    (wx, _), (yx, _), solves, _ = coupling_pass(white, _cols((1.0, 0.0, 1.0, 2.0)), 3.0, 2.0, 1.0, 0.0, OMEGA)
    assert solves == 1 and wx[0] == 0.0 and yx[0] > 1.0


def test_strength_gives_the_compliance(monkeypatch):
    """compliance = (1 - strength) / sub_delta^2 with the step's sub-step (L:1337-1341), and it softens the correction"""
    seen = []
    real = coupling_model.coupling_pass

    def spy(white, yolk, wr, yr, factor, compliance, omega, *rest):
        seen.append((factor, compliance, omega))
        return real(white, yolk, wr, yr, factor, compliance, omega, *rest)

    monkeypatch.setattr(coupling_model, "coupling_pass", spy)
    m = CouplingModel(relaxed=True)
    m.add(0.0, 0.0, 50, 15)
    m.set_coupling(1.5, 0.75)
    m.update(1 / 60, 1 / 60, 3, 1)
    sub = max((1 / 60) / 3, rm.EPS)
    assert seen == [(1.5, (1 - 0.75) / (sub * sub), m.relaxation)] * 3  # once per sub-step
    assert m.coupling_solves > 0
    # by hand: divisor = wsum + compliance
    white, yolk = _cols((0.0, 0.0, 1.0, 3.0)), _cols((4.0, 0.0, 0.5, 2.0))
    (wx, _), _, _, _ = coupling_pass(white, yolk, 4.0, 4.0, 1.0, 2.5, OMEGA)
    assert wx[0] == 0.0 + ((-1.0 * (1.0 / (1.5 + 2.5)) * 1.0) * OMEGA) / 1.0


def _run(model, steps, coupling=None, S=2, C=3):
    centers = [(0.0, 0.0), (30.0, 10.0), (-20.0, 40.0)]
    ids = [model.add(cx, cy, 50, 15) for cx, cy in centers]
    if coupling is not None:
        model.set_coupling(*coupling)
    for k in range(steps):
        for i, c in zip(ids, centers):
            model.set_target_position(i, *circle_target(c, k))
        model.update(1 / 60, 1 / 60, S, C)
    return [model.state(w) for w in (WHITE, YOLK)]


def test_factor_zero_is_the_viscosity_model():
    plain = ViscosityModel(relaxed=True)
    plain.set_viscosity(0.5, 1.0)
    ref = _run(plain, 4)
    for coupling in (None, (0.0, 1.0), (0.0, 0.25)):
        m = CouplingModel(relaxed=True)
        m.set_viscosity(0.5, 1.0)
        got = _run(m, 4, coupling)
        for w in (WHITE, YOLK):
            assert np.array_equal(got[w], ref[w]), (coupling, w)
        assert m.coupling_solves == 0 and m.pair_solves == plain.pair_solves
    on = CouplingModel(relaxed=True)
    on.set_viscosity(0.5, 1.0)
    got = _run(on, 4, (2.0, 1.0))
    assert on.coupling_solves > 0 and not np.array_equal(got[WHITE], ref[WHITE]) and not np.array_equal(got[YOLK], ref[YOLK])
    # exact order never couples
    exact = CouplingModel(relaxed=False)
    exact.set_coupling(2.0, 1.0)
    _run(exact, 1)
    assert exact.coupling_solves == 0


@functools.lru_cache(maxsize=None)
def overlaps_on_the_floor(coupling):
    """one default egg under gravity on a floor 40 px below its target, 60 steps: the white-yolk pairs closer than
    ra + rb at the end"""
    m = CouplingModel(relaxed=True)
    m.set_forces([("uniform", 0.0, 980.0)])
    m.set_colliders([("half_plane", 0.0, -1.0, -40.0)])  # keeps y <= 40 - r
    m.add(0.0, 0.0, 50, 15)
    if coupling:
        m.set_coupling(*coupling)
    for _ in range(60):
        m.update(1 / 60, 1 / 60, 2, 3)
    (wx, wy), (yx, yy) = (m.state(w)[:2] for w in (WHITE, YOLK))
    wr, yr = (np.array(m.field(w, rm.RADIUS)) for w in (WHITE, YOLK))
    d2 = (wx[:, None] - yx[None, :]) ** 2 + (wy[:, None] - yy[None, :]) ** 2
    return int(np.count_nonzero(d2 < (wr[:, None] + yr[None, :]) ** 2)), m.coupling_solves


def test_coupling_keeps_white_and_yolk_apart():
    """the effect: without coupling the yolk lies in the white on the floor; with set_coupling(2, 1) strictly fewer
    white-yolk pairs overlap ("Coupling", records both counts)"""
    without, none = overlaps_on_the_floor(None)
    with_, solves = overlaps_on_the_floor((2.0, 1.0))
    print("white-yolk pairs closer than ra + rb after 60 steps: %d without coupling, %d with set_coupling(2, 1)" % (without, with_))
    assert none == 0 and solves > 0
    assert with_ < without
