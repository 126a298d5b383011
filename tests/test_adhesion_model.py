"""tests/adhesion_model.py, the definition of white-yolk adhesion (egg_set_adhesion; DESIGN.md section 2.7, "Adhesion"),
checked on the CPU: off is CouplingModel bit for bit, a hand table of tiny batches that reaches every label of the census on
both sides, seven wrong rules that each change a case, the pass's own guarantee, and the effect on a yolk under gravity.

The hand table is tests/test_pair_census.py's in form: batches of 2 + 2 particles with imported state, target (0, 0),
follow radius 100 px, every particle at rest, so the first coupling pass starts from exactly the spots of the table.  Radii
are 2 (md = 8 with factor 2; rd = 10 with reach 2.5, the hypotenuse of 6-8-10; rd = 12 with reach 3), a particle's mass is
min_mass (`lo`) or max_mass (`hi`) of its config, and a particle a case does not need is parked on a ring.  White particles
2 b, 2 b + 1 and yolk particles 2 b, 2 b + 1 belong to batch b.  tests/test_gpu_adhesion.py runs every case on the device."""
import functools

import numpy as np
import pytest

import test_pair_census as pc
from adhesion_model import LABELS, RULES, SIDES, AdhesionMixin, AdhesionModel, adhesion_cell, adhesion_pass
from coupling_model import CouplingMixin, CouplingModel
from relaxed_model import DEFAULT_RELAXATION, rm
from test_coupling_model import _cols, _run
from wall_model import WallModel

WHITE, YOLK = 0, 1
OMEGA = DEFAULT_RELAXATION
H60 = 1 / 60
ON, A25, A3 = (2.0, 1.0), (2.5, 1.0), (3.0, 1.0)


class Hand(AdhesionMixin, CouplingMixin, WallModel):
    """the family's most derived member with the band: what tests/test_gpu_adhesion.py holds the device to"""


# ------------------------------------------------------------------------------------------------ off is off
@pytest.mark.parametrize("coupling,adhesion", [((2.0, 1.0), (0.0, 1.0)), ((2.0, 1.0), (2.0, 0.5)), ((2.0, 0.5), (1.5, 1.0)),
                                               (None, (3.0, 1.0)), ((0.0, 1.0), (3.0, 0.25))])
def test_off_is_the_coupling_model(coupling, adhesion):
    """reach 0, reach <= factor (an empty band) and coupling off: CouplingModel bit for bit on the scene of
    tests/test_coupling_model.py (three overlapping batches, moving targets, viscosity on both types)"""
    plain = CouplingModel(relaxed=True)
    plain.set_viscosity(0.5, 1.0)
    ref = _run(plain, 4, coupling)
    m = AdhesionModel(relaxed=True)
    m.set_viscosity(0.5, 1.0)
    m.set_adhesion(*adhesion)
    got = _run(m, 4, coupling)
    for w in (WHITE, YOLK):
        assert np.array_equal(got[w], ref[w]), w
    assert (m.coupling_solves, m.pair_solves, m.adhesion_solves) == (plain.coupling_solves, plain.pair_solves, 0)
    assert not hasattr(m, "adhesion_census")  # the band's pass never ran


def test_on_differs_and_exact_order_never_adheres():
    plain = CouplingModel(relaxed=True)
    ref = _run(plain, 4, ON)
    m = AdhesionModel(relaxed=True)
    m.set_adhesion(*A3)
    got = _run(m, 4, ON)
    assert m.adhesion_solves > 0 and not np.array_equal(got[WHITE], ref[WHITE]) and not np.array_equal(got[YOLK], ref[YOLK])
    exact = AdhesionModel(relaxed=False)
    exact.set_coupling(*ON)
    exact.set_adhesion(*A3)
    _run(exact, 1)
    assert exact.adhesion_solves == 0 and exact.coupling_solves == 0


# ------------------------------------------------------------------------------------------------ known answers
def test_known_answer_pair():
    """one white and one yolk particle of one batch 9 px apart, radii 2, factor 2, reach 2.5: md = 8, rd = 10, the pair
    adheres with violation = +1 and divisor = 1.5, and is pulled together"""
    white, yolk = _cols((0.0, 0.0, 1.0, 2.0)), _cols((9.0, 0.0, 0.5, 2.0))
    (wx, wy), (yx, yy), coupled, _, adhered, census = adhesion_pass(white, yolk, [7], [7], 2.0, 2.0, 2.0, 0.0, 2.5, 0.0, OMEGA)
    correction = -(9.0 - 8.0) / (1.0 + 0.5)
    assert (coupled, adhered) == (0, 1)
    assert wx[0] == 0.0 + ((-1.0 * correction * 1.0) * OMEGA) / 1.0 and wy[0] == 0.0
    assert yx[0] == 9.0 + ((1.0 * correction * 0.5) * OMEGA) / 1.0 and yy[0] == 0.0
    assert 0.0 < wx[0] < yx[0] < 9.0  # pulled together
    assert census["white_side"] == census["yolk_side"] == dict(dict.fromkeys(LABELS, 0), adheres=1, unclamped=1)
    # another batch: nothing
    (wx, _), (yx, _), coupled, _, adhered, census = adhesion_pass(white, yolk, [7], [8], 2.0, 2.0, 2.0, 0.0, 2.5, 0.0, OMEGA)
    assert (coupled, adhered, wx[0], yx[0]) == (0, 0, 0.0, 9.0) and census["white_side"]["other_batch"] == 1
    # adhesion's own compliance: divisor = wsum + compliance
    (wx, _), _, _, _, adhered, _ = adhesion_pass(white, yolk, [7], [7], 2.0, 2.0, 2.0, 0.0, 2.5, 2.5, OMEGA)
    assert adhered == 1 and wx[0] == 0.0 + ((-1.0 * (-1.0 / (1.5 + 2.5)) * 1.0) * OMEGA) / 1.0
    # inside md the pair couples as ever, with coupling's compliance
    near = _cols((4.0, 0.0, 0.5, 2.0))
    (wx, _), _, coupled, _, adhered, _ = adhesion_pass(white, near, [7], [7], 2.0, 2.0, 2.0, 0.5, 2.5, 0.0, OMEGA)
    assert (coupled, adhered) == (1, 0) and wx[0] == 0.0 + ((-1.0 * (-(4.0 - 8.0) / (1.5 + 0.5)) * 1.0) * OMEGA) / 1.0
    assert adhesion_cell(2.0, 2.0, 2.0, 2.5) == 10.0 and adhesion_cell(0.1, 0.1, 2.0, 3.0) == 1.0


# ------------------------------------------------------------------------------------------------ the hand table
SPECK = 2.0 ** -31  # a radius: ra + rb = 2^-30, md = 2^-29 = 1.9e-9 and rd = 3 2^-30 = 2.8e-9, both < eps = 1e-8
CONFIGS = dict(pc.CONFIGS, speck=dict(min_radius=SPECK, max_radius=SPECK))
UP85 = pc.UP85


def _case(white, yolk, want, cfg="plain", coupling=ON, adhesion=A25, then=False, solves=None):
    """white / yolk: per particle of the type, in index order, (x, y) or (x, y, "hi") -- "lo" unless said -- or None:
    parked.  want: the labels both sides of the pass take in the first update, exactly (the parked particles lie out of
    every cell neighbourhood: they add none).  then: a second update with
    (S, C) = (2, 2).  solves: (coupling_solves, adhesion_solves) after the first update."""
    assert len(white) == len(yolk) and len(white) % 2 == 0
    return dict(spots={WHITE: tuple(white), YOLK: tuple(yolk)}, want=set(want), cfg=cfg, coupling=coupling, adhesion=adhesion,
                then=then, solves=solves)


CASES = {
    "adheres": _case([(0.0, 0.0), None], [(9.0, 0.0), None], {"adheres", "unclamped"}, solves=(0, 1)),
    "adheres_diagonal_negative": _case([(-0.5, -0.5), None], [(-6.5, -8.0), None], {"adheres", "unclamped"}, solves=(0, 1)),
    "reach_edge": _case([(0.5, 0.5), None], [(6.5, 8.5), None], {"adheres", "reach_edge", "unclamped"}, solves=(0, 1)),
    "beyond_reach": _case([(0.5, 0.5), None], [(6.5, UP85), None], {"beyond"}, solves=(0, 0)),
    # a pair at exactly md couples with a zero share: whether it fired shows in n of the white particle, which a second
    # yolk particle of its batch pulls from the other side (and the mirror: the yolk particle between two white ones)
    "md_edge": _case([(0.0, 0.0), None], [(8.0, 0.0), (-9.0, 0.0)], {"couples", "md_edge", "adheres", "unclamped"}, solves=(1, 1)),
    "md_edge_mirror": _case([(8.0, 0.0), (-9.0, 0.0)], [(0.0, 0.0), None], {"couples", "md_edge", "adheres", "unclamped"}, solves=(1, 1)),
    # white 0 of batch 0 and yolk 2 of batch 1
    "other_batch": _case([(0.0, 0.0), None, None, None], [None, None, (9.0, 0.0), None], {"other_batch"}, solves=(0, 0)),
    "adheres_beside_another_batch": _case([(0.0, 0.0), None, None, None], [(0.0, 9.0), None, (9.0, 0.0), None],
                                          {"adheres", "unclamped", "other_batch"}, solves=(0, 1)),
    "skipped": _case([(0.0, 0.0, "hi"), None], [(9.0, 0.0, "hi"), None], {"skipped"}, cfg="heavy", solves=(0, 0)),
    # stiff: wsum = 0.5 and compliance 0, so -violation / divisor = -2 |violation| is clamped to -|violation|
    "clamped": _case([(0.0, 0.0), None], [(9.0, 0.0), None], {"adheres", "clamped"}, cfg="stiff", solves=(0, 1)),
    # 1 + 5 2^-31 is exact: d = 2.5 2^-30 lies in the band of two specks, and current < eps: a zero normal, n counts
    "tiny": _case([(1.0, 0.0), None], [(1.0 + 5 * SPECK, 0.0), None], {"adheres", "tiny", "unclamped"}, cfg="speck", adhesion=A3,
                  solves=(0, 1)),
    # an overlapping pair of one batch couples, with COUPLING's compliance (strength 0.5); the band's is 0
    "couples_first": _case([(0.0, 0.0), None], [(4.0, 0.0), None], {"couples", "unclamped"}, coupling=(2.0, 0.5), adhesion=A3,
                           solves=(1, 0)),
    # ... and a pair in the band takes ADHESION's (strength 0.25), which depends on the sub-step: the second update runs two
    "own_strength": _case([(0.0, 0.0), None], [(9.0, 0.0), None], {"adheres", "unclamped"}, adhesion=(2.5, 0.25), then=True,
                          solves=(0, 1)),
    # 9 px apart in cells 0 and 1 of size H = 10 -- at the cell size 8 of the factor alone they would lie two cells apart
    "cell_of_the_reach": _case([(7.5, 0.5), None], [(16.5, 0.5), None], {"adheres", "unclamped"}, solves=(0, 1)),
    # one white particle in cell (0, 0) of size H = 12 with an adhering partner in cell (-1, 1) and a coupling one in cell
    # (0, -1), and the mirror
    "three_cells": _case([(6.0, 6.0), None], [(-3.5, 13.0), (9.0, -0.5)], {"adheres", "couples", "unclamped"}, adhesion=A3,
                         solves=(1, 1)),
    "three_cells_mirror": _case([(-3.5, 13.0), (9.0, -0.5)], [(6.0, 6.0), None], {"adheres", "couples", "unclamped"}, adhesion=A3,
                                solves=(1, 1)),
}


def hand_configs(name):
    c = CASES[name]
    w, y = rm.default_configs()
    extra = dict(pc.BASE, **CONFIGS[c["cfg"]])
    return dict(w, **extra), dict(y, **extra)


def hand_config_keys(name):
    return sorted(set(pc.BASE) | set(CONFIGS[CASES[name]["cfg"]]))


def hand_spots(name, which):
    """per particle of the type: (x, y, mass parameter t)"""
    out = []
    for p, s in enumerate(CASES[name]["spots"][which]):
        s = pc.PARK[which][p] if s is None else s
        out.append((float(s[0]), float(s[1]), 1.0 if len(s) > 2 and s[2] == "hi" else 0.0))
    return out


def hand_columns(name, which):
    """the nine rows of egg_export_batch for the type's particles (x y vx vy last_x last_y inverse mass radius t), [9, n]"""
    cfg = hand_configs(name)[which]
    cols = np.zeros((9, len(CASES[name]["spots"][which])))
    for p, (x, y, t) in enumerate(hand_spots(name, which)):
        mass = rm.mix(cfg["min_mass"], cfg["max_mass"], t)
        assert mass == (cfg["max_mass"] if t else cfg["min_mass"])  # (exact at t = 0 and t = 1)
        cols[:, p] = (x, y, 0.0, 0.0, x, y, 1 / mass, rm.mix(cfg["min_radius"], cfg["max_radius"], t), t)
    assert (cols[7] == cfg["max_radius"]).all()
    return cols


def hand_updates(name):
    return [(H60, H60, 1, 1)] + ([(H60, H60, 2, 2)] if CASES[name]["then"] else [])


def hand_run(name, rule=None):
    """the case on the model; returns (model, batch ids, (coupling_solves, adhesion_solves) and the census after the
    first update)"""
    c = CASES[name]
    m = Hand(*hand_configs(name))
    m.adhesion_rule = rule
    m.set_coupling(*c["coupling"])
    m.set_adhesion(*c["adhesion"])
    ids = [m.add(*pc.HAND_TARGET, pc.HAND_RADIUS, pc.HAND_RADIUS, 2, 2) for _ in range(len(c["spots"][WHITE]) // 2)]
    for w, data in ((WHITE, m._white_data), (YOLK, m._yolk_data)):
        cols = hand_columns(name, w)
        for p in range(cols.shape[1]):
            x, y, _, _, _, _, inv, radius, t = (float(v) for v in cols[:, p])
            for off, v in ((rm.X, x), (rm.Y, y), (rm.PX, x), (rm.PY, y), (rm.LAST_X, x), (rm.LAST_Y, y), (rm.VX, 0.0), (rm.VY, 0.0),
                           (rm.MASS_T, t), (rm.MASS, 1 / inv), (rm.INV_MASS, inv), (rm.RADIUS, radius)):
                data[rm.offset(p + 1) + off] = v
    first = None
    for u in hand_updates(name):
        assert m.update(*u) == 1
        if first is None:
            first = ((m.coupling_solves, m.adhesion_solves), {s: dict(m.adhesion_census[s]) for s in SIDES})
    return m, ids, first


@functools.lru_cache(maxsize=None)
def hand_model(name):
    return hand_run(name)


def hand_labels(name):
    """side -> the labels the side took in the first update"""
    _, _, (_, census) = hand_model(name)
    return {side: {label for label, v in census[side].items() if v} for side in SIDES}


def outputs(m):
    return [m.state(w) for w in (WHITE, YOLK)], (m.pair_solves, m.coupling_solves, m.adhesion_solves)


def same_outputs(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and a[1] == b[1]


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_case(name):
    """every case takes the branches it is named for on BOTH sides, which count the same pairs; the state stays finite"""
    m, _, (solves, census) = hand_model(name)
    c = CASES[name]
    assert m.adhesion_acts()
    for side in SIDES:
        assert hand_labels(name)[side] == c["want"], (name, side, census[side])
    assert census["white_side"] == census["yolk_side"], name
    if c["solves"] is not None:
        assert solves == c["solves"], (name, solves)
    assert solves == (census["white_side"]["couples"], census["white_side"]["adheres"])
    for w in (WHITE, YOLK):
        assert np.isfinite(m.state(w)).all()


def test_the_hand_table_holds_every_label():
    reached = {side: set().union(*(hand_labels(name)[side] for name in CASES)) for side in SIDES}
    for side in SIDES:
        assert reached[side] == set(LABELS), (side, set(LABELS) - reached[side])
    for label in LABELS:
        print("%-12s %s" % (label, ", ".join(n for n in sorted(CASES) if label in hand_labels(n)["white_side"])))


def test_closed_forms():
    """by hand: omega 1.8, n = 1 unless said, lo masses 1 (wsum = 2), strength 1"""
    m, _, _ = hand_model("adheres")  # violation +1, correction -1/2: each side moves 0.5 * 1.8 = 0.9 towards the other
    assert (m.state(WHITE)[0, 0], m.state(YOLK)[0, 0]) == (0.0 + ((-1.0 * -0.5 * 1.0) * OMEGA) / 1.0, 9.0 + ((1.0 * -0.5 * 1.0) * OMEGA) / 1.0)
    m, _, _ = hand_model("reach_edge")  # d = 10, normal (0.6, 0.8), violation +2, correction -1
    assert (m.state(WHITE)[0, 0], m.state(WHITE)[1, 0]) == (0.5 + ((-(6.0 / 10.0) * -1.0 * 1.0) * OMEGA) / 1.0,
                                                            0.5 + ((-(8.0 / 10.0) * -1.0 * 1.0) * OMEGA) / 1.0)
    m, _, _ = hand_model("md_edge")  # n = 2: the zero share of the touching pair halves the pull of the other
    assert m.state(WHITE)[0, 0] == 0.0 + (((0.0 + 0.0) + -(-1.0) * -0.5 * 1.0) * OMEGA) / 2.0
    m, _, _ = hand_model("clamped")  # wsum 0.5: correction -2 clamped to -1, each side moves 0.25 * 1.8: the pair ends at md + 0.1
    assert (m.state(WHITE)[0, 0], m.state(YOLK)[0, 0]) == (0.0 + ((-1.0 * -1.0 * 0.25) * OMEGA) / 1.0, 9.0 + ((1.0 * -1.0 * 0.25) * OMEGA) / 1.0)
    m, _, _ = hand_model("tiny")  # a zero normal: nothing moves
    assert (m.state(WHITE)[0, 0], m.state(YOLK)[0, 0]) == (1.0, 1.0 + 5 * SPECK)
    for name in ("beyond_reach", "other_batch", "skipped"):
        m, _, _ = hand_model(name)
        for w in (WHITE, YOLK):
            assert [tuple(v) for v in m.state(w)[:2].T] == [s[:2] for s in hand_spots(name, w)], (name, w)


# ------------------------------------------------------------------------------------------------ wrong rules
CAUGHT_BY = {
    "no_batch_test": ("other_batch", "adheres_beside_another_batch"),
    "reach_lt": ("reach_edge",),
    "target_rd": ("adheres", "clamped", "own_strength"),
    "coupling_compliance": ("own_strength",),
    "cell_from_factor": ("cell_of_the_reach",),
    "adhesion_first": ("couples_first",),
}


def test_every_rule_is_caught():
    assert set(CAUGHT_BY) | {"per_type_tag"} == set(RULES)


@pytest.mark.parametrize("rule", sorted(CAUGHT_BY))
def test_a_wrong_rule_changes_a_case(rule):
    """a kernel wrong in that way would fail tests/test_gpu_adhesion.py's hand table"""
    for name in CAUGHT_BY[rule]:
        right, _, _ = hand_model(name)
        wrong, _, _ = hand_run(name, rule)
        assert not same_outputs(outputs(right), outputs(wrong)), (rule, name)


def test_a_per_type_tag_changes_a_pass():
    """rule 7, a tag that skips the batches without particles of the type.  add refuses such a batch (a particle count
    cannot be 0 or 1), so the case lives at the pass: whites of batches 1, 2, 3, yolks of batches 1 and 3; the white of
    batch 2 lies 9 px from the yolk of batch 3, whose per-type tag would be 1 on both"""
    white = _cols((0.0, 0.0, 1.0, 2.0), (40.0, 0.0, 1.0, 2.0), (80.0, 0.0, 1.0, 2.0))
    yolk = _cols((9.0, 0.0, 1.0, 2.0), (49.0, 0.0, 1.0, 2.0))
    args = (white, yolk, [1, 2, 3], [1, 3], 2.0, 2.0, 2.0, 0.0, 2.5, 0.0, OMEGA)
    (wx, _), (yx, _), _, _, adhered, census = adhesion_pass(*args)
    assert adhered == 1 and census["white_side"]["other_batch"] == 1 and (wx[1], yx[1]) == (40.0, 49.0)
    (wx, _), (yx, _), _, _, adhered, _ = adhesion_pass(*args, rule="per_type_tag")
    assert adhered == 2 and (wx[1], yx[1]) != (40.0, 49.0)


# ------------------------------------------------------------------------------------------------ the pass's guarantee
@pytest.mark.parametrize("omega", [1.0, 0.5])
def test_an_adhering_pair_never_ends_closer_than_md(omega):
    """with omega <= 1 and nothing else acting on the pair (n = 1 on both sides), its own share leaves an adhering pair at
    md or beyond: the pair closes by |correction| wsum omega, |correction| <= violation / (wsum + compliance) <= violation /
    wsum without the clamp and <= violation with it, so by at most violation.  Tolerance: a dozen roundings at magnitude <=
    1e4, relative 1e-12."""
    rng = np.random.default_rng(20261019)
    n = 400
    ra, rb = rng.uniform(0.5, 3.0, n), rng.uniform(0.5, 3.0, n)
    wa, wb = rng.uniform(0.05, 2.0, n), rng.uniform(0.05, 2.0, n)
    factor, reach = 1.5, 3.0
    md, rd = factor * (ra + rb), reach * (ra + rb)
    d = md + (rd - md) * rng.uniform(0.001, 0.999, n)
    angle = rng.uniform(0.0, 2 * np.pi, n)
    ax = 100.0 * np.arange(n) - 20000.0  # 100 px between the pairs: no particle has a second partner (H <= 18)
    ay = rng.uniform(-50.0, 50.0, n)
    bx, by = ax + d * np.cos(angle), ay + d * np.sin(angle)
    for compliance in (0.0, 0.7):
        (wx, wy), (yx, yy), coupled, _, adhered, census = adhesion_pass((ax, ay, wa, ra), (bx, by, wb, rb), np.arange(n), np.arange(n),
                                                                       3.0, 3.0, factor, 0.0, reach, compliance, omega)
        assert (coupled, adhered) == (0, n) and census["white_side"]["clamped"] > 0 and census["white_side"]["unclamped"] > 0
        after = np.hypot(yx - wx, yy - wy)
        before = np.hypot(bx - ax, by - ay)
        assert (after < before).all() and (after >= md * (1 - 1e-12)).all()


# ------------------------------------------------------------------------------------------------ the effect
@functools.lru_cache(maxsize=None)
def yolk_under_gravity(adhesion, g=4000.0, steps=30):
    """one default egg, coupling (2, 1), gravity on the yolk alone, (S, C) = (2, 3): the distance between the centroids
    of the two types at the end"""
    m = AdhesionModel(relaxed=True)
    m.set_forces([("uniform", 0.0, g, "yolk")])
    m.add(0.0, 0.0, 50, 15)
    m.set_coupling(*ON)
    if adhesion:
        m.set_adhesion(*adhesion)
    for _ in range(steps):
        m.update(H60, H60, 2, 3)
    (wx, wy), (yx, yy) = (m.state(w)[:2] for w in (WHITE, YOLK))
    finite = bool(np.isfinite(m.state(WHITE)).all() and np.isfinite(m.state(YOLK)).all())
    return float(np.hypot(yx.mean() - wx.mean(), yy.mean() - wy.mean())), m.adhesion_solves, finite


def test_adhesion_keeps_the_yolk_by_its_white():
    """the effect: under gravity on the yolk alone the follow constraint is all that holds the yolk; with set_adhesion(3, 1)
    its centroid hangs strictly closer to the white's ("Adhesion", records both distances)"""
    without, none, finite0 = yolk_under_gravity(None)
    with_, solves, finite1 = yolk_under_gravity(A3)
    print("white-yolk centroid distance after 30 steps at 4000 px/s^2: %.17g px without adhesion, %.17g px with set_adhesion(3, 1)"
          % (without, with_))
    assert finite0 and finite1
    assert none == 0 and solves > 0
    assert with_ < without
