"""tests/pair_census.py -- which branch of the pair arithmetic a pair evaluation of the relaxed step takes (DESIGN.md
section 2.7) -- and the hand table tests/test_gpu_pair_edges.py runs on the device, checked here on the model alone.  No
device needed.

  a. recording is free: PairCensusModel and the un-instrumented model agree in every bit on the coupling and cohesion
     scenes the device files run;
  b. the gap, as a fact: which labels the device scenes of test_gpu_relaxed.py, test_gpu_cohesion.py and test_gpu_coupling.py
     reach (EXISTING), and which they never do;
  c. the hand table CASES: tiny batches of 2 + 2 particles with imported state, each case asserting the labels it is there
     for; together they reach every label at every site where it can occur (test_the_hand_table_holds_every_label prints the
     table of DESIGN.md);
  d. closed forms by hand;
  e. sensitivity: each of eight wrong rules (RULES), patched into a copy of the model, changes the final state or a counter
     of the cases named in CAUGHT_BY -- a kernel wrong in that way would fail the device file.

The hand table.  Every batch has its target at (0, 0) and the follow radius 2 sqrt(HAND_RADIUS) = 100 px; every particle
rests (zero velocity) within it, so pre-solve and follow leave it where it was put and the first pass that looks at pairs --
the coupling pass where coupling is on, else the first collision pass -- starts from exactly the spots of the table (each
case asserts it).  Radii are 2, the overlap factor 2 (md = 8), both types' cohesion factor 2.5 (reach = 10, the hypotenuse of
6-8-10, so that a pair at exactly the reach lies in neighbouring cells of size 5), the coupling factor 2 or 2.5 (H = 8 or
10).  A particle's mass is min_mass (`lo`) or max_mass (`hi`) of its type's config: its mass parameter t (row 8 of the
nine-row exported state; row 6 is the inverse mass, row 7 the radius) is 0 or 1, and mix(lo, hi, t) is exact there.  A
particle the case does not need is parked on a ring (white 60 px, yolk 84 px from the origin), out of every reach."""
import functools
import math

import numpy as np
import pytest

from cohesion_model import CohesiveModel
from conftest import circle_target, load_golden
from coupling_model import CouplingMixin, CouplingModel
from pair_census import REACHABLE, SITES, TYPE, PairCensusModel, classify
from relaxed_model import DEFAULT_RELAXATION, DIRS, RelaxedModel, pair_shares, rm
from wall_model import WallModel

WHITE, YOLK = 0, 1
OMEGA = DEFAULT_RELAXATION
H60 = 1 / 60
COL = ("collision:white", "collision:yolk")
COH = ("cohesion:white", "cohesion:yolk")
CPL = ("couple_white_side", "couple_yolk_side")


class Plain(CouplingMixin, WallModel):
    """the un-instrumented model: tests/test_gpu_coupling.py's"""


def same_state(a, b):
    return all(np.array_equal(a.state(w), b.state(w)) for w in (WHITE, YOLK))


def counters(m):
    return (m.pair_solves, m.cohesion_solves, m.coupling_solves, m.coupling_coincident, list(m.viscosity_pairs),
            list(m.collider_hits), list(m.collider_grips))


# ------------------------------------------------------------------------------------------------ the labels are right
def _one(a, b, wa=1.0, wb=1.0, da=1, overlap=2.0, compliance=9.0, cohesion=None, eps=rm.EPS):
    """classify() on one pair of radius-2 particles: the set of (site kind, label), and the shares"""
    args = ([a[0]], [a[1]], [b[0]], [b[1]], [wa], [wb], [2.0], [2.0], [da], overlap)
    lab, shares, counted, collides, coheres = classify(*args, compliance, eps, cohesion=cohesion)
    ref = pair_shares(*args, compliance, eps)
    assert bool(ref[4][0]) == bool(counted[0]) and bool(ref[5][0]) == bool(collides[0])
    return {name for name, lanes in lab.items() if lanes[0]}, tuple(float(s[0]) for s in shares)


def test_the_census_names_one_evaluation():
    C, K = "collision", "cohesion"
    assert _one((0, 0), (8, 0))[0] == {(C, "fires"), (C, "touching"), (C, "unclamped")}
    assert _one((0, 0), (np.nextafter(8.0, 9.0), 0))[0] == {(C, "apart")}
    assert _one((0, 0), (4, 0), 1e-9, 1e-9)[0] == {(C, "skipped")}
    assert _one((0, 0), (4, 0), 0.25, 0.25, compliance=0.0) == ({(C, "fires"), (C, "clamp_hi")}, (-1.0, -0.0, 1.0, 0.0))
    assert _one((1, 0), (1 + 2.0 ** -30, 0)) == ({(C, "fires"), (C, "tiny"), (C, "unclamped")}, (-0.0, -0.0, 0.0, 0.0))
    for d in range(-9, 10):
        got, shares = _one((3, 3), (3, 3), da=d)
        assert got == {(C, "fires"), (C, "coincident_%d" % (d & 7)), (C, "unclamped")}
        c = 8.0 / 11.0
        assert shares == (-float(DIRS[d & 7, 0]) * c * 1.0, -float(DIRS[d & 7, 1]) * c * 1.0, float(DIRS[d & 7, 0]) * c * 1.0, float(DIRS[d & 7, 1]) * c * 1.0)
    same, other = (np.array([True]), 2.5, 4.0), (np.array([False]), 2.5, 4.0)
    assert _one((0.5, 0.5), (6.5, 8.5), cohesion=same)[0] == {(K, "coheres"), (K, "reach_edge"), (K, "unclamped")}
    assert _one((0.5, 0.5), (6.5, np.nextafter(8.5, 9.0)), cohesion=same)[0] == {(C, "apart")}
    assert _one((0, 0), (9, 0), cohesion=other)[0] == {(C, "apart"), (K, "other_batch")}
    assert _one((0, 0), (9, 0), 0.25, 0.25, cohesion=(np.array([True]), 2.5, 0.0)) == ({(K, "coheres"), (K, "clamp_lo")}, (0.25, 0.0, -0.25, -0.0))
    assert _one((0, 0), (8, 0), cohesion=same)[0] == {(C, "fires"), (C, "touching"), (C, "unclamped")}  # a collision first


def test_dead_needs_a_negative_compliance():
    """divisor = wsum + compliance < eps with wsum >= eps needs compliance < 0, which no strength in [0, 1] gives (see
    tests/pair_census.py): the label exists for the classifier's and pair_shares' zero shares alone, on the CPU"""
    got, shares = _one((0, 0), (4, 0), compliance=-2.0)
    assert got == {("collision", "fires"), ("collision", "dead")} and shares == (0.0, 0.0, 0.0, 0.0)
    got, shares = _one((0, 0), (9, 0), cohesion=(np.array([True]), 2.5, -2.0))
    assert got == {("cohesion", "coheres"), ("cohesion", "dead")} and shares == (0.0, 0.0, 0.0, 0.0)
    assert all(float(v[0]) == 0.0 for v in pair_shares([0.0], [0.0], [4.0], [0.0], [1.0], [1.0], [2.0], [2.0], [1], 2.0, -2.0)[:4])
    for strength in (0.0, 0.25, 1.0, -3.0, 7.0):
        assert rm.ReferenceModel._strength_to_compliance(strength, H60) >= 0.0


# ------------------------------------------------------------------------------------------------ a., b. the device scenes
WHITE3 = dict(cohesion_interaction_distance_factor=3, cohesion_strength=0.99)


def _centers():
    return [tuple(float(v) for v in c) for c in load_golden("four_batches")["centers"]]


def _scene_model(cls, white=None, cohesion=False, coupling=None, relaxation=None, colliders=(), surfaces=None, forces=(), viscosity=None):
    w, y = rm.default_configs()
    m = cls(dict(w, **(white or {})), y, relaxation=relaxation, cohesion=cohesion)
    if viscosity:
        m.set_viscosity(*viscosity)
    m.set_colliders(colliders)
    m.set_forces(forces)
    if surfaces is not None:
        m.set_collider_surfaces(surfaces)
    if coupling:
        m.set_coupling(*coupling)
    return m


def _moving(m, centers, S, C, steps, moving=True, counts=(50, 15)):
    ids = [m.add(cx, cy, *counts) for cx, cy in centers]
    for k in range(steps):
        if moving:
            for i, c in zip(ids, centers):
                m.set_target_position(i, *circle_target(c, k))
        m.update(H60, H60, S, C)
    return m


def _coincident_pair(m):
    """tests/test_gpu_coupling.py's test_a_coincident_white_yolk_pair"""
    m.add(300.0, 300.0, 28, 28, 2, 2)
    for data, on in ((m._white_data, 1), (m._yolk_data, 0)):
        for p in (0, 1):
            x, y = (300.0, 300.0) if p == on else (300.0 + 90.0 * (p + 1), 250.0 + 400.0 * on)
            for off, v in ((rm.X, x), (rm.Y, y), (rm.LAST_X, x), (rm.LAST_Y, y), (rm.VX, 0.0), (rm.VY, 0.0)):
                data[rm.offset(p + 1) + off] = v
    m.update(H60, H60, 1, 1)
    for _ in range(3):
        m.update(H60, H60, 2, 3)
    return m


def _everything(m):
    import test_gpu_collider_walls as tw
    i = m.add(300.0, 300.0, 50, 15)
    for k in range(8):
        if k == 2:
            m.set_target_position(i, 300.0, 300.0 + tw.DROP)
        m.update(H60, H60, 2, 3)
    return m


def _smallest(m):
    for x, y in ((295.0, 296.0), (307.0, 296.0)):
        m.add(x, y, 28, 28, 2, 2)
    for _ in range(6):
        m.update(H60, H60, 2, 3)
    return m


def _everything_kwargs():
    import test_gpu_collider_walls as tw
    return dict(white=WHITE3, cohesion=True, viscosity=(0.5, 1.0), colliders=(("container", 300.0, 330.0, 160.0), tw.WALL),
                surfaces=(0.2, (0.4, -50.0, 0.0)), forces=(("uniform", 0.0, 400.0),), coupling=(2.0, 1.0))


def _steps(m, ids, centers, ks, S=2, C=3):
    for k in ks:
        for i, c in zip(ids, centers):
            m.set_target_position(i, *circle_target(c, k))
        m.update(H60, H60, S, C)


def _mutations(m, change, spans):
    """test_mutations_between_relaxed_steps / cohesion's test_mutations: a middle batch removed, one added, a live config change"""
    centers = _centers()
    ids = [m.add(cx, cy, 50, 15) for cx, cy in centers]
    _steps(m, ids, centers, spans[0])
    m.remove(ids[1])
    centers, ids = [centers[0]] + centers[2:], [ids[0]] + ids[2:]
    _steps(m, ids, centers, spans[1])
    centers, ids = centers + [(60.0, -30.0)], ids + [m.add(60.0, -30.0, 40, 12)]
    _steps(m, ids, centers, spans[2])
    m._white_config.update(change[WHITE])
    m._yolk_config.update(change[YOLK])
    _steps(m, ids, centers, spans[3])
    return m


def _switching(m, attribute):
    """test_mode_switches (exact, relaxed, exact: the census sees the relaxed passes) / cohesion's test_toggling (on, off, on)"""
    centers = _centers()
    ids = [m.add(cx, cy, 50, 15) for cx, cy in centers]
    for n, on in enumerate((True, False, True) if attribute == "cohesion" else (False, True, False)):
        setattr(m, attribute, on)
        _steps(m, ids, centers, range(5 * n, 5 * n + 5))
    return m


def _rules(m):
    """test_rules: the steps it takes with (1.5, 0.25) -- it compares nothing to the model"""
    m.add(400.0, 300.0, 50, 15)
    for _ in range(3):
        m.update(H60, H60, 2, 3)
    return m


def _off_is_off(m):
    """test_off_is_off at (2, 3): five steps coupled, two uncoupled"""
    for c in ((300.0, 300.0), (330.0, 310.0)):
        m.add(*c, 50, 15)
    for k in range(7):
        if k == 5:
            m.set_coupling(0)
        m.update(H60, H60, 2, 3)
    return m


GRID = tuple((40.0 * (k % 8) - 140.0, 40.0 * (k // 8) - 140.0) for k in range(64))
SAME_SPOT = ((300.0, 300.0),) * 4 + ((700.0, 300.0),)
# name: (how the model is set up, how it is driven): the device scenes of the three files, each as its test runs it
EXISTING = {
    "relaxed_parity_2_3": (dict(relaxation=1.5), lambda m: _moving(m, _centers(), 2, 3, 20)),
    "relaxed_parity_1_1": (dict(relaxation=1.0), lambda m: _moving(m, _centers(), 1, 1, 20)),
    "relaxed_coincident_batches": (dict(), lambda m: _moving(m, SAME_SPOT, 2, 3, 10, moving=False)),
    "cohesion_parity_default": (dict(cohesion=True), lambda m: _moving(m, _centers(), 2, 3, 20)),
    "cohesion_parity_white3": (dict(white=WHITE3, cohesion=True), lambda m: _moving(m, _centers(), 3, 2, 20)),
    "cohesion_smallest_shapes": (dict(white=WHITE3, cohesion=True), _smallest),
    "cohesion_coincident_batches": (dict(white=WHITE3, cohesion=True), lambda m: _moving(m, SAME_SPOT, 2, 3, 10, moving=False)),
    "coupling_one_egg": (dict(coupling=(2.0, 1.0)), lambda m: _moving(m, ((300.0, 300.0),), 2, 3, 10)),
    "coupling_four_batches": (dict(coupling=(2.0, 1.0)), lambda m: _moving(m, _centers(), 3, 1, 6)),
    "coupling_coincident_pair": (dict(coupling=(2.0, 1.0)), _coincident_pair),
    "coupling_everything": (None, _everything),
    "coupling_dense_grid": (dict(coupling=(2.0, 1.0)), lambda m: _moving(m, GRID, 2, 1, 6)),
    "relaxed_mutations": (dict(), lambda m: _mutations(m, (dict(max_mass=2.5), dict(min_mass=0.5)), (range(4), range(4, 7), range(7, 10), range(10, 14)))),
    "relaxed_mode_switches": (dict(), lambda m: _switching(m, "relaxed")),
    "cohesion_toggling": (dict(white=WHITE3, cohesion=True), lambda m: _switching(m, "cohesion")),
    "cohesion_mutations": (dict(white=WHITE3, cohesion=True), lambda m: _mutations(
        m, (dict(cohesion_strength=0.9, cohesion_interaction_distance_factor=2.5), dict(cohesion_strength=0.5, cohesion_interaction_distance_factor=2.25)),
        (range(3), range(3, 6), range(6, 9), range(9, 12)))),
    "coupling_rules": (dict(coupling=(1.5, 0.25)), _rules),
    "coupling_off_is_off": (dict(coupling=(2.0, 1.0)), _off_is_off),
}
# Left out, and why.  The other (S, C) / omega parametrizations of the three parity tests, test_launches_of_one_step and the
# second (S, C) of test_off_is_off run the scenes above with other pass counts.  The device-group and sharded tests of the
# three files run four_batches as cohesion_parity_white3 / relaxed_parity_2_3 do and are held to one handle's result, so
# their pair evaluations are these.  test_one_type_without_particles has no cross pair at all (and skips where add refuses
# an empty type).  test_surface, test_refusals, test_bad_positions_fail_without_commit and
# test_a_failed_step_adds_nothing_and_commits_nothing are about errors: their committed steps are one default egg's, as in
# coupling_one_egg.  test_full_size_config3_sites (4096 batches) is too slow on a Python model; it repeats the site of
# relaxed_coincident_batches -- four batches on one spot -- 1024 times.
# what no device scene reached before the hand table: the labels below are absent from every scene of EXISTING
NEVER = ("skipped", "touching", "tiny", "clamp_hi", "clamp_lo", "reach_edge")
_B = {"apart", "fires", "unclamped"}
_BA, _K, _KO = _B | {"alone"}, {"coheres", "unclamped"}, {"coheres", "unclamped", "other_batch"}
_C0, _C7 = {"coincident_0"}, {"coincident_7"}
_CW, _CY = {"coincident_2", "coincident_5", "coincident_7"}, {"coincident_5", "coincident_6", "coincident_7"}
# scene -> site -> the labels it takes, exactly (averaged_n left out); a site not named takes none.  Coincident pairs occur
# only where batches were added on one spot (a type's own pass: two or three normals) and where a batch's first white and
# first yolk particle still rest on its centre (the coupling pass: key difference 0, or the one pair (0 - 1) & 7 put there
# by hand); white's cohesion band (md, reach] is empty with the default factors
EXISTING_LABELS = {
    "relaxed_parity_2_3": {COL[0]: _BA, COL[1]: _BA},
    "relaxed_parity_1_1": {COL[0]: _B, COL[1]: _B},
    "relaxed_coincident_batches": {COL[0]: _BA | _CW, COL[1]: _BA | _CY},
    "cohesion_parity_default": {COL[0]: _BA, COL[1]: _BA, COH[1]: _KO},
    "cohesion_parity_white3": {COL[0]: _B, COL[1]: _B, COH[0]: _KO, COH[1]: _KO},
    "cohesion_smallest_shapes": {COL[0]: _B, COL[1]: _B, COH[0]: _KO, COH[1]: _KO},
    "cohesion_coincident_batches": {COL[0]: _B | _CW, COL[1]: _BA | _CY, COH[0]: _KO, COH[1]: _KO},
    "coupling_one_egg": {COL[0]: _BA, COL[1]: _BA, CPL[0]: _BA, CPL[1]: _BA},
    "coupling_four_batches": {COL[0]: _BA, COL[1]: _BA, CPL[0]: _BA, CPL[1]: _BA},
    "coupling_coincident_pair": {COL[0]: {"alone"}, COL[1]: {"alone"}, CPL[0]: {"alone", "fires", "unclamped"} | _C7, CPL[1]: {"alone", "fires", "unclamped"} | _C7},
    "coupling_everything": {COL[0]: _BA, COL[1]: _B, COH[0]: _K, COH[1]: _K, CPL[0]: _BA | _C0, CPL[1]: _BA | _C0},
    "coupling_dense_grid": {COL[0]: _BA, COL[1]: _BA, CPL[0]: _BA, CPL[1]: _BA},
    "relaxed_mutations": {COL[0]: _BA, COL[1]: _BA},
    "relaxed_mode_switches": {COL[0]: _BA, COL[1]: _BA},
    "cohesion_toggling": {COL[0]: _B, COL[1]: _BA, COH[0]: _KO, COH[1]: _KO},
    "cohesion_mutations": {COL[0]: _B, COL[1]: _BA, COH[0]: _KO, COH[1]: _KO},
    # (the egg rests: its first white and first yolk particle stay on the centre; a second batch's first particles have
    # the key difference 15 - 157, whose normal is 2)
    "coupling_rules": {COL[0]: _B, COL[1]: _BA, CPL[0]: _BA | _C0, CPL[1]: _B | _C0},
    "coupling_off_is_off": {COL[0]: _BA, COL[1]: _BA, CPL[0]: _BA | _C0 | {"coincident_2"}, CPL[1]: _BA | _C0 | {"coincident_2"}},
}


@functools.lru_cache(maxsize=None)
def existing_model(name, cls=PairCensusModel):
    kwargs, drive = EXISTING[name]
    return drive(_scene_model(cls, **(_everything_kwargs() if kwargs is None else kwargs)))


@pytest.mark.parametrize("name", sorted(EXISTING))
def test_what_the_existing_device_scenes_reach(name):
    """b.: the labels of the device scenes of the three files, exactly -- and with them what they never reach: nothing of
    NEVER at any site, no clamp, no skipped pair, at most three of the eight normals at a type's own pass and one at a time
    in the coupling pass.  The hand table below is there for the rest."""
    m = existing_model(name)
    print("%s: %s" % (name, {s: m.counts(s) for s in SITES if m.counts(s)}))
    for site in SITES:
        got = {lab for lab in m.labels(site) if not lab.startswith("averaged_")}
        assert got == EXISTING_LABELS[name].get(site, set()), (name, site, got)
        assert not got & set(NEVER)


@pytest.mark.parametrize("name", ["cohesion_smallest_shapes", "relaxed_parity_1_1", "coupling_one_egg", "coupling_four_batches",
                                  "coupling_coincident_pair", "coupling_everything"])
def test_recording_is_free(name):
    """a.: the census changes no bit and no counter"""
    m, plain = existing_model(name), existing_model(name, Plain)
    assert same_state(m, plain) and counters(m) == counters(plain)
    assert m.evaluations > 0 and not hasattr(plain, "census")


def test_the_plain_models_are_the_family():
    """with nothing else set the most derived model is CouplingModel, CohesiveModel or RelaxedModel"""
    a = _moving(_scene_model(PairCensusModel, coupling=(2.0, 1.0)), ((300.0, 300.0),), 2, 3, 3)
    c = CouplingModel()
    c.set_coupling(2.0, 1.0)
    assert same_state(a, _moving(c, ((300.0, 300.0),), 2, 3, 3))
    w, y = rm.default_configs()
    a = _moving(_scene_model(PairCensusModel, white=WHITE3, cohesion=True), _centers(), 2, 3, 2)
    assert same_state(a, _moving(CohesiveModel(dict(w, **WHITE3), y, cohesion=True), _centers(), 2, 3, 2))
    a = _moving(_scene_model(PairCensusModel, relaxation=1.5), _centers(), 2, 3, 2)
    assert same_state(a, _moving(RelaxedModel(relaxed=True, relaxation=1.5), _centers(), 2, 3, 2))


# ------------------------------------------------------------------------------------------------ c. the hand table
HAND_RADIUS, HAND_TARGET = 2500.0, (0.0, 0.0)
BASE = dict(min_radius=2, max_radius=2, cohesion_interaction_distance_factor=2.5)
CONFIGS = {
    "plain": {},                                   # the default masses (lo = 1; hi = 1.8 white, 1.35 yolk) and strengths
    "heavy": dict(max_mass=1e9),                   # hi: inverse mass 1e-9, two of them have wsum = 2e-9 < eps
    # lo: mass 4, so wsum = 0.5; strength 1 has compliance 0: divisor = 0.5 and |violation / divisor| = 2 |violation|
    "stiff": dict(min_mass=4, max_mass=8, collision_strength=1, cohesion_strength=1),
}
RING = ((60.0, 0.0), (52.0, 30.0), (30.0, 52.0), (0.0, 60.0), (-30.0, 52.0), (-52.0, 30.0), (-60.0, 0.0), (-52.0, -30.0),
        (-30.0, -52.0), (0.0, -60.0), (30.0, -52.0), (52.0, -30.0))
PARK = {WHITE: RING, YOLK: tuple((1.4 * x, 1.4 * y) for x, y in RING)}
UP8, UP85 = float(np.nextafter(8.0, 9.0)), float(np.nextafter(8.5, 9.0))
TINY = 2.0 ** -30  # 9.3e-10 < eps, and 1 + TINY is exact
FIVE = ((30.0, 0.0), (0.0, 30.0), (-30.0, 0.0), (0.0, -30.0), (0.0, 0.0))
EIGHT = ((30.0, 0.0), (21.0, 21.0), (0.0, 30.0), (-21.0, 21.0), (-30.0, 0.0), (-21.0, -21.0), (0.0, -30.0), (21.0, -21.0))
FIRED, TOUCH = {"fires", "unclamped"}, {"fires", "touching", "unclamped"}


def _case(white, yolk=None, cfg="plain", cohesion=False, coupling=None, want=None, then=False, pairs=None, **more):
    """white / yolk: per particle of the type, in index order, (x, y) or (x, y, "hi") -- "lo" unless said -- or None: parked.
    yolk None: the white spots (the two types do not meet without coupling).  want: site -> the labels the site takes,
    exactly; a site it does not name takes none.  then: a second update with (S, C) = (2, 2).  pairs: pair_solves after the
    first update."""
    yolk = white if yolk is None else yolk
    assert len(white) == len(yolk) and len(white) % 2 == 0
    return dict(spots={WHITE: tuple(white), YOLK: tuple(yolk)}, cfg=cfg, cohesion=cohesion, coupling=coupling, want=want or {},
                then=then, pairs=pairs, **more)


def _both(labels, sites=COL):
    return {s: set(labels) for s in sites}


def _coincident(pairs, n, spots):
    """n particles per type; pair k of `pairs` rests on spots[k], every other particle is parked"""
    out = [None] * n
    for (a, b), s in zip(pairs, spots):
        out[a] = out[b] = s
    return out


def _coupled_coincident(perm):
    """white particle i and yolk particle perm[i] rest on EIGHT[i]: eight cross pairs with index differences perm[i] - i"""
    yolk = [None] * 8
    for i, j in enumerate(perm):
        yolk[j] = EIGHT[i]
    return list(EIGHT), yolk


def _ks(diffs):
    return {"coincident_%d" % (d & 7) for d in diffs}


ODD, EVEN = (7, 6, 5, 4, 3, 2, 1, 0), (6, 5, 4, 3, 2, 1, 0, 7)  # differences 7, 5, 3, 1, -1, -3, -5, -7 and 6, 4, 2, 0, -2, -4, -6, 0
A_PAIRS, B_PAIRS = ((0, 8), (1, 7), (2, 6), (3, 5), (4, 9)), ((0, 1), (2, 9), (3, 6), (4, 5), (7, 8))
ALONE = {"alone"}
ON, ON25 = (2.0, 1.0), (2.5, 1.0)
CASES = {
    # ---- a type's own pass: the collision site (both types run the same spots)
    # (a touching pair has violation 0 and a zero share: whether it fired shows in n of particle 0, which a third particle pushes)
    "touching_x": _case([(0.0, 0.0), (8.0, 0.0), (-4.0, 0.0), None], want=_both(TOUCH | {"averaged_2", "alone"}), pairs=4),
    "touching_y": _case([(0.0, 0.0), (0.0, 8.0), (0.0, -4.0), None], want=_both(TOUCH | {"averaged_2", "alone"})),
    "beyond_touching": _case([(0.0, 0.0), (UP8, 0.0)], want=_both({"apart", "alone"}), pairs=2),
    "skipped": _case([(0.0, 0.0, "hi"), (4.0, 0.0, "hi")], cfg="heavy", want=_both({"skipped", "alone"}), pairs=0),
    "heavy_and_light": _case([(0.0, 0.0, "hi"), (4.0, 0.0)], cfg="heavy", want=_both(FIRED), pairs=2),
    "clamp_hi": _case([(0.0, 0.0), (4.0, 0.0)], cfg="stiff", want=_both({"fires", "clamp_hi"})),
    "tiny": _case([(1.0, 0.0), (1.0 + TINY, 0.0), (5.0, 0.0), None], want=_both({"fires", "tiny", "unclamped", "averaged_2", "alone"})),
    "coincident_a": _case(_coincident(A_PAIRS, 10, FIVE), want=_both(FIRED | _ks((8, 6, 4, 2, 5)))),
    "coincident_b": _case(_coincident(B_PAIRS, 10, FIVE), want=_both(FIRED | _ks((1, 7, 3)))),
    # one particle with three partners in three cells (cell size 5): (-1, 1), (0, -1), (1, 0) in that order, x offset outer
    # (of the partners only the last two are in neighbouring cells, and collide: averaged_2)
    # (the yolk's first partner lies elsewhere in its cell: with the white's spots the yolk's three shares happen to add up
    # to the same bits in either order)
    "three_cells": _case([(2.0, 2.0), (-3.1, 7.9), (2.9, -2.2), (6.1, 3.3)], [(2.0, 2.0), (-0.7, 5.1), (2.9, -2.2), (6.1, 3.3)], want=_both(FIRED | {"averaged_2", "averaged_3"})),
    # ---- the cohesion site (effective cohesion on)
    "beyond_touching_coheres": _case([(0.0, 0.0), (UP8, 0.0)], cohesion=True, want=_both({"coheres", "unclamped"}, COH)),
    "reach_edge": _case([(0.5, 0.5), (6.5, 8.5)], cohesion=True, want=_both({"coheres", "reach_edge", "unclamped"}, COH)),
    "beyond_reach": _case([(0.5, 0.5), (6.5, UP85)], cohesion=True, want=_both({"apart", "alone"})),
    "other_batch": _case([(0.0, 0.0), None, (9.0, 0.0), None], cohesion=True, want=dict(_both({"apart", "alone"}), **_both({"other_batch"}, COH))),
    "coheres_beside_another_batch": _case([(0.0, 0.0), (0.0, 9.0), (9.0, 0.0), None], cohesion=True,
                                          want=dict(_both({"apart", "alone"}), **_both({"coheres", "unclamped", "other_batch"}, COH))),
    "clamp_lo": _case([(0.0, 0.0), (9.0, 0.0)], cfg="stiff", cohesion=True, want=_both({"coheres", "clamp_lo"}, COH)),
    # ---- the coupling pass (white and yolk spots differ; the types' own passes then meet nothing: every particle is alone)
    "couple_touching": _case([(0.0, 0.0), None], [(8.0, 0.0), None], coupling=ON, want=dict(_both(ALONE), **_both(TOUCH | ALONE, CPL))),
    "couple_touching_diagonal": _case([(0.5, 0.5), None], [(6.5, 8.5), None], coupling=ON25, want=dict(_both(ALONE), **_both(TOUCH | ALONE, CPL))),
    "couple_beyond_touching": _case([(0.5, 0.5), None], [(6.5, UP85), None], coupling=ON25, want=dict(_both(ALONE), **_both({"apart", "alone"}, CPL))),
    "couple_skipped": _case([(0.0, 0.0, "hi"), None], [(4.0, 0.0, "hi"), None], cfg="heavy", coupling=ON,
                            want=dict(_both(ALONE), **_both({"skipped", "alone"}, CPL))),
    "couple_clamp_hi": _case([(0.0, 0.0), None], [(4.0, 0.0), None], cfg="stiff", coupling=ON,
                             want=dict(_both(ALONE), **_both({"fires", "clamp_hi", "alone"}, CPL))),
    # a touching cross pair has a zero share too: whether it fired shows in n of the particle that a second partner of the
    # other type pushes -- the white one (beside: two yolks) or the yolk one (mirror: two whites; 12 px apart, they never meet)
    "couple_touching_beside": _case([(0.0, 0.0), None], [(8.0, 0.0), (-4.0, 0.0)], coupling=ON,
                                    want={"collision:white": ALONE, "collision:yolk": ALONE, "couple_white_side": TOUCH | {"averaged_2", "alone"},
                                          "couple_yolk_side": TOUCH}),
    "couple_touching_mirror": _case([(8.0, 0.0), (-4.0, 0.0)], [(0.0, 0.0), None], coupling=ON,
                                    want={"collision:white": ALONE, "collision:yolk": ALONE, "couple_yolk_side": TOUCH | {"averaged_2", "alone"},
                                          "couple_white_side": TOUCH}),
    # ... and the mirror of couple_tiny: the yolk particle beside a tiny white one and a second white one at d = 4
    "couple_tiny_mirror": _case([(1.0 + TINY, 0.0), (5.0, 0.0)], [(1.0, 0.0), None], coupling=ON,
                                want={"collision:yolk": ALONE, "collision:white": FIRED, "couple_yolk_side": {"fires", "tiny", "unclamped", "averaged_2", "alone"},
                                      "couple_white_side": {"fires", "tiny", "unclamped"}}),
    "couple_tiny": _case([(1.0, 0.0), None], [(1.0 + TINY, 0.0), (5.0, 0.0)], coupling=ON,
                         want={"collision:white": ALONE, "collision:yolk": FIRED, "couple_white_side": {"fires", "tiny", "unclamped", "averaged_2", "alone"},
                               "couple_yolk_side": {"fires", "tiny", "unclamped"}}),
    "couple_coincident_odd": _case(*_coupled_coincident(ODD), coupling=ON, want=dict(_both(ALONE), **_both(FIRED | _ks((7, 5, 3, 1, -1, -3, -5, -7)), CPL))),
    "couple_coincident_even": _case(*_coupled_coincident(EVEN), coupling=ON, want=dict(_both(ALONE), **_both(FIRED | _ks((6, 4, 2, 0, -2, -4, -6)), CPL))),
    # factor 0.1: md = 0.4 and H = max(1.0, 0.8) takes the 1.0.  White 0 meets yolk 0 on its own spot (index difference 0) and
    # yolk 1 a quarter pixel away in the same cell; white 2 and yolk 2 lie 0.2 px apart across the cell edge at x = 21
    "couple_small_factor": _case([(0.5, 0.5), None, (20.9, 0.5), None], [(0.5, 0.5), (0.75, 0.5), (21.1, 0.5), None], coupling=(0.1, 1.0),
                                 want={"collision:white": ALONE, "collision:yolk": FIRED | ALONE,
                                       "couple_white_side": FIRED | {"coincident_0", "averaged_2", "alone"},
                                       "couple_yolk_side": FIRED | {"coincident_0", "alone"}}),
    # a compliance (1 - 0.5) / h^2 that depends on the sub-step: the second update runs two sub-steps
    "couple_compliance": _case([(0.0, 0.0), None], [(4.0, 0.0), None], coupling=(2.0, 0.5), then=True, want=dict(_both(ALONE), **_both(FIRED | ALONE, CPL))),
    # one white particle with three yolk partners in three cells of size H = 8, and the mirror
    "couple_three_cells": _case([(4.0, 4.0), None, None, None], [(-2.1, 8.9), (5.7, -0.6), (9.1, 5.3), None], coupling=ON,
                                want=dict(_both(ALONE), couple_white_side=FIRED | {"averaged_3", "alone"}, couple_yolk_side=FIRED | ALONE)),
    "couple_three_cells_mirror": _case([(-2.1, 8.9), (5.7, -0.6), (9.1, 5.3), None], [(4.0, 4.0), None, None, None], coupling=ON,
                                       want=dict(_both(ALONE), couple_yolk_side=FIRED | {"averaged_3", "alone"}, couple_white_side=FIRED | ALONE)),
}
# pairs found through each of the eight neighbour cells, across the origin: particle 0 in cell (0, 0), particle 1 in cell (ox, oy)
# (which finds particle 0 through (-ox, -oy)); cell size 5 for a type's own pass, H = 8 for the coupling pass
CELLS = tuple((ox, oy) for ox in (-1, 0, 1) for oy in (-1, 0, 1) if (ox, oy) != (0, 0))
for _ox, _oy in CELLS:
    _tag = "%s%s" % ("m0p"[_ox + 1], "m0p"[_oy + 1])
    CASES["cell_" + _tag] = _case([(2.0, 2.0), (2.0 + 4.0 * _ox, 2.0 + 4.0 * _oy)], want=_both(FIRED), cells=(5.0, (_ox, _oy)))
    CASES["couple_cell_" + _tag] = _case([(4.0, 4.0), None], [(4.0 + 5.0 * _ox, 4.0 + 5.0 * _oy), None], coupling=ON,
                                         want=dict(_both(ALONE), **_both(FIRED | ALONE, CPL)), cells=(8.0, (_ox, _oy)))


def hand_configs(name):
    c = CASES[name]
    w, y = rm.default_configs()
    return dict(w, **BASE, **CONFIGS[c["cfg"]]), dict(y, **BASE, **CONFIGS[c["cfg"]])


def hand_spots(name, which):
    """per particle of the type: (x, y, mass parameter t)"""
    out = []
    for p, s in enumerate(CASES[name]["spots"][which]):
        s = PARK[which][p] if s is None else s
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
    assert (cols[7] == 2.0).all()
    return cols


def hand_updates(name):
    return [(H60, H60, 1, 1)] + ([(H60, H60, 2, 2)] if CASES[name]["then"] else [])


def hand_run(name, cls=PairCensusModel, updates=None):
    """the case on a model of class `cls`; returns (model, batch ids, pair_solves after the first update)"""
    c = CASES[name]
    m = cls(*hand_configs(name), cohesion=c["cohesion"])
    if c["coupling"]:
        m.set_coupling(*c["coupling"])
    ids = [m.add(*HAND_TARGET, HAND_RADIUS, HAND_RADIUS, 2, 2) for _ in range(len(c["spots"][WHITE]) // 2)]
    for w, data in ((WHITE, m._white_data), (YOLK, m._yolk_data)):
        cols = hand_columns(name, w)
        for p in range(cols.shape[1]):
            x, y, _, _, _, _, inv, radius, t = (float(v) for v in cols[:, p])
            for off, v in ((rm.X, x), (rm.Y, y), (rm.PX, x), (rm.PY, y), (rm.LAST_X, x), (rm.LAST_Y, y), (rm.VX, 0.0), (rm.VY, 0.0),
                           (rm.MASS_T, t), (rm.MASS, 1 / inv), (rm.INV_MASS, inv), (rm.RADIUS, radius)):
                data[rm.offset(p + 1) + off] = v
    first = None
    for u in (hand_updates(name) if updates is None else updates):
        assert m.update(*u) == 1
        first = m.pair_solves if first is None else first
    return m, ids, first


@functools.lru_cache(maxsize=None)
def hand_model(name):
    return hand_run(name)


def assert_hand_labels(name):
    """the case takes the branches it is named for, on the model: every site takes exactly the labels of the table, the
    first pass that looks at pairs starts from the spots of the table, and the state stays finite"""
    m, ids, first = hand_model(name)
    c = CASES[name]
    for site in SITES:
        assert m.labels(site) == c["want"].get(site, set()), (name, site, m.counts(site))
    for w in (WHITE, YOLK):
        site = "couple_%s_side" % TYPE[w] if c["coupling"] else "collision:" + TYPE[w]
        x, y = m.starts[site][0]
        assert [(float(a), float(b)) for a, b in zip(x, y)] == [s[:2] for s in hand_spots(name, w)], (name, w)
        assert np.isfinite(m.state(w)).all()
    if c["pairs"] is not None:
        assert first == c["pairs"], (name, first)
    if name == "couple_small_factor":
        assert m.coupling_cell() == 1.0 and math.floor(20.9) != math.floor(21.1)
    if "cells" in c:  # the partner lies in the neighbour cell the case is named for, across the origin for a negative one
        size, (ox, oy) = c["cells"]
        (ax, ay, _), (bx, by, _) = hand_spots(name, WHITE)[0], hand_spots(name, YOLK if c["coupling"] else WHITE)[0 if c["coupling"] else 1]
        assert (math.floor(ax / size), math.floor(ay / size)) == (0, 0) and (math.floor(bx / size), math.floor(by / size)) == (ox, oy)
    return m


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_case(name):
    m = assert_hand_labels(name)
    plain, _, _ = hand_run(name, Plain)  # recording is free
    assert same_state(m, plain) and counters(m) == counters(plain)
    for w, want in (hand_closed_form(name) or {}).items():
        for p, xy in want.items():
            assert tuple(float(v) for v in m.state(w)[:2, p]) == xy, (name, w, p)


# label -> site -> the cases that are there for it (every one asserts it through its `want`)
def table_of_labels():
    rows = {}
    for name in sorted(CASES):
        for site, labels in CASES[name]["want"].items():
            for lab in labels:
                rows.setdefault((lab, site), []).append(name)
    return rows


def test_the_hand_table_holds_every_label():
    """every label except `dead` is reached by a named case at every site where it can occur; the table goes to DESIGN.md"""
    rows = table_of_labels()
    for lab, sites in REACHABLE.items():
        for site in sites:
            assert rows.get((lab, site)), (lab, site)
    for site in COL + CPL:
        assert rows.get(("alone", site)) and rows.get(("averaged_2", site)), site
    assert rows.get(("averaged_3", "collision:white")) and rows.get(("averaged_3", "couple_white_side")) and rows.get(("averaged_3", "couple_yolk_side"))
    assert not any(lab == "dead" for lab, _ in rows)
    # for the coupling pass each normal from both signs of the index difference, yolk index - white index
    diffs = [j - i for perm in (ODD, EVEN) for i, j in enumerate(perm)]
    for k in range(1, 8):
        assert k in diffs and k - 8 in diffs
    assert 0 in diffs
    print("%-14s %-18s %s" % ("label", "site", "cases"))
    for (lab, site), names in sorted(rows.items()):
        short = names if len(names) <= 4 else names[:3] + ["... (%d)" % len(names)]
        print("%-14s %-18s %s" % (lab, site, ", ".join(short)))


# ------------------------------------------------------------------------------------------------ d. closed forms
def hand_closed_form(name):
    """{type: {particle: (x, y) after the first update}} where the case has a closed form, worked out by hand below"""
    c = CASES[name]
    if name in ("couple_touching", "couple_touching_diagonal"):
        # violation = 0: the pair fires (n = 1) with a zero share; nothing moves, no later pass finds anything either
        return {w: {0: hand_spots(name, w)[0][:2]} for w in (WHITE, YOLK)}
    if name in ("couple_touching_beside", "couple_touching_mirror"):
        # the particle at the origin touches one partner (a zero share that counts) and lies 4 px from the other: violation -4,
        # wsum 2, compliance 0 (strength 1), correction 2, below the clamp; pushed along +x, halved by the average: n = 2
        return {WHITE if name == "couple_touching_beside" else YOLK: {0: (0.0 + ((2.0 + 0.0) * OMEGA) / 2.0, 0.0)}}
    if name in ("touching_x", "touching_y"):
        # particle 1 touches particle 0 and meets nobody else: n = 1, a zero share, it stays.  Particle 0 has n = 2: the zero
        # share of the touching pair and the push of particle 2 at d = 4 (violation -4), halved by the average
        out = {}
        for w, strength in ((WHITE, 1 - 0.0025), (YOLK, 1 - 0.001)):
            correction = 4.0 / (2.0 + (1 - strength) / (H60 * H60))
            moved = 0.0 + (((0.0 + 0.0) + 1.0 * correction * 1.0) * OMEGA) / 2.0  # (a of the pair (0, 2), whose normal points away from it)
            out[w] = {1: hand_spots(name, w)[1][:2], 0: (moved, 0.0) if name == "touching_x" else (0.0, moved)}
        return out
    if name == "clamp_hi":
        # d = 4, md = 8: violation -4, divisor 0.5, correction 8 clamped to 4; shares -/+ 4 * 0.25 = -/+ 1, n = 1, omega 1.8
        return {w: {0: (0.0 + (-1.0 * OMEGA) / 1.0, 0.0), 1: (4.0 + (1.0 * OMEGA) / 1.0, 0.0)} for w in (WHITE, YOLK)}
    if name == "couple_clamp_hi":
        # the same numbers in the coupling pass; the types' own passes then find nothing (different types)
        return {WHITE: {0: (0.0 + (-1.0 * OMEGA) / 1.0, 0.0)}, YOLK: {0: (4.0 + (1.0 * OMEGA) / 1.0, 0.0)}}
    if name == "clamp_lo":
        # d = 9: violation +1, divisor 0.5, correction -2 clamped to -1; shares +/- 1 * 0.25: pulled together by 0.25 * 1.8 each
        return {w: {0: (0.0 + (0.25 * OMEGA) / 1.0, 0.0), 1: (9.0 + (-0.25 * OMEGA) / 1.0, 0.0)} for w in (WHITE, YOLK)}
    if name == "coincident_a":
        # pair (0, 8) on FIVE[0] = (30, 0): k = 8 & 7 = 0, the normal (1, 0); violation -8, wsum 2 and the type's collision
        # compliance (1 - strength) / h^2; below the clamp.  a = 0 goes against the normal, b = 8 along it
        out = {}
        for w, strength in ((WHITE, 1 - 0.0025), (YOLK, 1 - 0.001)):
            correction = 8.0 / (2.0 + (1 - strength) / (H60 * H60))
            out[w] = {0: (30.0 + ((-1.0 * correction * 1.0) * OMEGA) / 1.0, 0.0 + ((-0.0 * correction * 1.0) * OMEGA) / 1.0),
                      8: (30.0 + ((1.0 * correction * 1.0) * OMEGA) / 1.0, 0.0)}
        return out
    if name == "couple_coincident_odd":
        # white 3 and yolk ODD[3] = 4 on EIGHT[3] = (-21, 21): k = 1, the normal (s, s); compliance 0 (strength 1): correction
        # 8 / 2 = 4 = |violation| / 2; the white particle goes against the normal, the yolk one along it
        s = float(DIRS[1, 0])
        return {WHITE: {3: (-21.0 + ((-s * 4.0 * 1.0) * OMEGA) / 1.0, 21.0 + ((-s * 4.0 * 1.0) * OMEGA) / 1.0)},
                YOLK: {4: (-21.0 + ((s * 4.0 * 1.0) * OMEGA) / 1.0, 21.0 + ((s * 4.0 * 1.0) * OMEGA) / 1.0)}}
    if name == "tiny":
        # particle 0 meets particle 1 (tiny: zero share, counted) and particle 2 at d = 4 (violation -4): n = 2
        out = {}
        for w, strength in ((WHITE, 1 - 0.0025), (YOLK, 1 - 0.001)):
            correction = 4.0 / (2.0 + (1 - strength) / (H60 * H60))
            out[w] = {0: (1.0 + (((0.0 + -0.0) + -1.0 * correction * 1.0) * OMEGA) / 2.0, 0.0)}
        return out
    return None


def test_closed_forms_cover_the_issue():
    """a touching pair, one coincident pair per site, a clamped pair (and more): the cases with a closed form"""
    have = {name for name in CASES if hand_closed_form(name)}
    assert {"touching_x", "couple_touching", "coincident_a", "couple_coincident_odd", "clamp_hi", "clamp_lo", "couple_clamp_hi", "tiny"} <= have
    # (coincident_a's form is per type: both collision sites; couple_coincident_odd's covers both sides of the coupling pass)


# ------------------------------------------------------------------------------------------------ e. wrong rules
RULES = ("collision_lt", "reach_lt", "no_clamp", "tiny_not_counted", "a_minus_b", "compliance_from_delta", "yolk_takes_cax", "y_outer")
# rule -> cases that must notice it (the test asserts these, and prints every case that does)
# (rule, side of the coupling pass) -> the cases in which that side's own particle notices the rule when it holds on that side
# alone: a slip in one role of the coupling kernel is caught by the state of that role's type, not by coupling_solves
ONE_SIDE = {
    ("collision_lt", WHITE): ("couple_touching_beside",), ("collision_lt", YOLK): ("couple_touching_mirror",),
    ("tiny_not_counted", WHITE): ("couple_tiny",), ("tiny_not_counted", YOLK): ("couple_tiny_mirror",),
    ("no_clamp", WHITE): ("couple_clamp_hi",), ("no_clamp", YOLK): ("couple_clamp_hi",),
    ("a_minus_b", WHITE): ("couple_coincident_odd", "couple_coincident_even"), ("a_minus_b", YOLK): ("couple_coincident_odd", "couple_coincident_even"),
    ("compliance_from_delta", WHITE): ("couple_compliance",), ("compliance_from_delta", YOLK): ("couple_compliance",),
    ("y_outer", WHITE): ("couple_three_cells",), ("y_outer", YOLK): ("couple_three_cells_mirror",),
    ("yolk_takes_cax", YOLK): ("couple_clamp_hi", "couple_cell_pp", "couple_coincident_odd"),
}
CAUGHT_BY = {
    "collision_lt": ("touching_x", "touching_y", "couple_touching", "couple_touching_diagonal", "couple_touching_beside", "couple_touching_mirror"),
    "reach_lt": ("reach_edge",),
    "no_clamp": ("clamp_hi", "clamp_lo", "couple_clamp_hi"),
    "tiny_not_counted": ("tiny", "couple_tiny", "couple_tiny_mirror"),
    "a_minus_b": ("coincident_a", "coincident_b", "couple_coincident_odd", "couple_coincident_even"),
    "compliance_from_delta": ("couple_compliance",),
    "yolk_takes_cax": ("couple_clamp_hi", "couple_cell_pp", "couple_coincident_odd"),
    "y_outer": ("three_cells", "couple_three_cells", "couple_three_cells_mirror"),
}


def rule_pair(rule, ax, ay, bx, by, wa, wb, ra, rb, da, overlap, compliance, eps, cohesion=None):
    """one pair in plain Python floats, wrong in the way `rule` names (None: right).
    Returns (counted, kind, shares, tiny): kind None, "collision" or "cohesion"."""
    wsum = wa + wb
    if wsum < eps:
        return False, None, None, False
    dx, dy = bx - ax, by - ay
    d2 = dx * dx + dy * dy
    md = overlap * (ra + rb)
    kind = "collision" if (d2 < md * md if rule == "collision_lt" else d2 <= md * md) else None
    if kind is None and cohesion is not None:
        same, factor, cohesion_compliance = cohesion
        reach = factor * (ra + rb)
        if same and (d2 < reach * reach if rule == "reach_lt" else d2 <= reach * reach):
            kind, compliance = "cohesion", cohesion_compliance
    if kind is None:
        return True, None, None, False
    divisor = wsum + compliance
    if divisor < eps:
        return True, kind, (0.0, 0.0, 0.0, 0.0), False
    current = math.sqrt(d2)
    violation = current - md
    tiny = False
    if d2 == 0.0:
        k = (-da if rule == "a_minus_b" else da) & 7
        nx, ny = float(DIRS[k, 0]), float(DIRS[k, 1])
    elif current < eps:
        nx, ny, tiny = 0.0, 0.0, True
    else:
        nx, ny = dx / current, dy / current
    correction = -violation / divisor
    if rule != "no_clamp":
        correction = rm.clamp(correction, -abs(violation), abs(violation))
    return True, kind, (-nx * correction * wa, -ny * correction * wa, nx * correction * wb, ny * correction * wb), tiny


def _cell_order(rule):
    if rule == "y_outer":
        return [(ox, oy) for oy in (-1, 0, 1) for ox in (-1, 0, 1)]
    return [(ox, oy) for ox in (-1, 0, 1) for oy in (-1, 0, 1)]


class RuleModel(CouplingMixin, WallModel):
    """the model whose pair loops are written out particle by particle in plain Python and follow rule_pair(self.rule)"""
    rule = None
    side = None  # WHITE or YOLK: the rule holds on that side of the coupling pass alone (and in no pass of a type's own)

    def _step(self, delta, n_sub_steps, n_collision_steps, visit_logs=None):
        self._whole_delta = max(delta, rm.EPS)
        super()._step(delta, n_sub_steps, n_collision_steps, visit_logs)

    def _columns(self, data, n, offs):
        return [[data[rm.offset(p) + off] for p in range(1, n + 1)] for off in offs]

    def _solve_collision(self, particles, n, spatial_hash, collided, overlap, compliance, factor, cohesion_compliance, max_n, visit_log=None):
        assert self.relaxed and not self.colliders
        rule = self.rule if self.side is None else None
        if n == 0:
            self.relaxed_pass_pairs.append(0)
            return 0, False
        x, y, w, r, cx, cy, batch = self._columns(particles, n, (rm.X, rm.Y, rm.INV_MASS, rm.RADIUS, rm.CELL_X, rm.CELL_Y, rm.BATCH_ID))
        cells = {}
        for j in range(n):
            cells.setdefault((cx[j], cy[j]), []).append(j)
        pairs = cohered = 0
        out = []
        for i in range(n):
            sx = sy = 0.0
            fired = 0
            for ox, oy in _cell_order(rule):
                for j in cells.get((cx[i] + ox, cy[i] + oy), ()):
                    if j == i:
                        continue
                    a, b = min(i, j), max(i, j)
                    coh = (batch[a] == batch[b], factor, cohesion_compliance) if self.cohesion else None
                    counted, kind, s, tiny = rule_pair(rule, x[a], y[a], x[b], y[b], w[a], w[b], r[a], r[b], b - a, overlap, compliance, rm.EPS, coh)
                    pairs += counted and j > i
                    if kind is None:
                        continue
                    cohered += kind == "cohesion" and j > i
                    sx, sy = (sx + s[0], sy + s[1]) if i == a else (sx + s[2], sy + s[3])
                    fired += not (tiny and rule == "tiny_not_counted")
            out.append((x[i] + (sx * self.relaxation) / fired, y[i] + (sy * self.relaxation) / fired) if fired else (x[i], y[i]))
        for p, (nx, ny) in enumerate(out):
            particles[rm.offset(p + 1) + rm.X], particles[rm.offset(p + 1) + rm.Y] = nx, ny
        self.relaxed_pass_pairs.append(pairs)
        self.cohesion_solves += cohered
        return pairs, False

    def _couple(self):
        nw, ny = self._total_n_white_particles, self._total_n_yolk_particles
        if not (self.relaxed and self.coupling_factor > 0.0 and nw and ny):
            return
        f = self.coupling_factor
        H = max(1.0, f * (self._white_config["max_radius"] + self._yolk_config["max_radius"]))
        cols = [self._columns(data, n, (rm.X, rm.Y, rm.INV_MASS, rm.RADIUS)) for data, n in ((self._white_data, nw), (self._yolk_data, ny))]
        cells = []
        for x, y, _, _ in cols:
            table = {}
            for j in range(len(x)):
                table.setdefault((math.floor(x[j] / H), math.floor(y[j] / H)), []).append(j)
            cells.append(table)
        (wx, wy, ww, wr), (yx, yy, yw, yr) = cols
        new = []
        for own in (WHITE, YOLK):
            rule = self.rule if self.side in (None, own) else None
            h = self._whole_delta if rule == "compliance_from_delta" else self._coupling_sub_delta
            compliance = (1.0 - self.coupling_strength) / (h * h)
            x, y = cols[own][:2]
            out = []
            for i in range(len(x)):
                sx = sy = 0.0
                fired = 0
                for ox, oy in _cell_order(rule):
                    for j in cells[1 - own].get((math.floor(x[i] / H) + ox, math.floor(y[i] / H) + oy), ()):
                        a, b = (i, j) if own == WHITE else (j, i)
                        counted, kind, s, tiny = rule_pair(rule, wx[a], wy[a], yx[b], yy[b], ww[a], yw[b], wr[a], yr[b], b - a, f, compliance, rm.EPS)
                        if kind is None:
                            continue
                        mine = s[:2] if own == WHITE or rule == "yolk_takes_cax" else s[2:]
                        sx, sy = sx + mine[0], sy + mine[1]
                        fired += not (tiny and rule == "tiny_not_counted")
                        self.coupling_solves += own == WHITE
                        self.coupling_coincident += own == WHITE and wx[a] == yx[b] and wy[a] == yy[b]
                out.append((x[i] + (sx * self.relaxation) / fired, y[i] + (sy * self.relaxation) / fired) if fired else (x[i], y[i]))
            new.append(out)
        for data, out in zip((self._white_data, self._yolk_data), new):
            for p, (nx, ny) in enumerate(out):
                data[rm.offset(p + 1) + rm.X], data[rm.offset(p + 1) + rm.Y] = nx, ny


def _rule_class(rule, side=None):
    return type("Rule_%s_%s" % (rule, side), (RuleModel,), dict(rule=rule, side=side))


def test_the_right_rule_is_the_model():
    """rule None: the harness of the sensitivity test is the model, bit for bit, on every case of the hand table"""
    for name in sorted(CASES):
        m, v = hand_model(name)[0], hand_run(name, _rule_class(None))[0]
        assert same_state(m, v) and counters(m) == counters(v), name


@pytest.mark.parametrize("rule", RULES)
def test_a_wrong_rule_changes_a_case(rule):
    cls = _rule_class(rule)
    caught_by = []
    for name in sorted(CASES):
        m, v = hand_model(name)[0], hand_run(name, cls)[0]
        if not (same_state(m, v) and counters(m) == counters(v)):
            caught_by.append(name)
    print("%s: caught by %s" % (rule, caught_by))
    assert set(CAUGHT_BY[rule]) <= set(caught_by), (rule, caught_by)
    for name in CAUGHT_BY[rule]:  # a case without coupling runs the same site for both types: either type's state notices
        if not CASES[name]["coupling"]:
            m, v = hand_model(name)[0], hand_run(name, cls)[0]
            assert all(not np.array_equal(m.state(w), v.state(w)) for w in (WHITE, YOLK)), (rule, name)
    for (r, side), names in ONE_SIDE.items():  # the rule on one side of the coupling pass alone: that side's type moves elsewhere
        for name in names if r == rule else ():
            m, v = hand_model(name)[0], hand_run(name, _rule_class(rule, side))[0]
            assert not np.array_equal(m.state(side), v.state(side)), (rule, side, name)
    if rule == "compliance_from_delta":  # (one sub-step: delta / S is delta)
        assert caught_by == ["couple_compliance"]
        one = [(H60, H60, 1, 1)]
        assert same_state(hand_run("couple_compliance", cls, one)[0], hand_run("couple_compliance", Plain, one)[0])
    for on_cut, names in (("collision_lt", ("cut_touching",)), ("a_minus_b", ("cut_coincident_1", "cut_coincident_3"))):
        for name in names if rule == on_cut else ():  # ... and the pair across a cut
            v = _scene_model(cls, white=WHITE3, cohesion=True)
            for x, y, R in cut_case(name)[0]:
                v.add(x, y, R, R, 2, 2)
            for u in CUT_UPDATES:
                v.update(*u)
            assert all(not np.array_equal(cut_model(name)[0].state(w), v.state(w)) for w in (WHITE, YOLK)), (rule, name)
    if rule == "y_outer":  # the particle with three partners, of each type and on each side of the coupling pass
        for name, types in (("three_cells", (WHITE, YOLK)), ("couple_three_cells", (WHITE,)), ("couple_three_cells_mirror", (YOLK,))):
            m, v = hand_model(name)[0], hand_run(name, cls)[0]
            assert all(not np.array_equal(m.state(w)[:2, 0], v.state(w)[:2, 0]) for w in types), name
    if rule in ("collision_lt", "reach_lt"):  # one ulp further out both rules agree
        assert not {"beyond_touching", "beyond_reach", "couple_beyond_touching"} & set(caught_by)


# ------------------------------------------------------------------------------------------------ f. pairs across a cut
# A device group and a ShardedSimulationHandler own whole batches and take no imported state, so the pairs a cut splits are
# built with add() alone: a batch of two particles per type has its first particle exactly on its centre (the spiral's
# radius is sqrt(0 / n) = 0) and its second 0.707 R away.  Default radii (4: md = 16), white's cohesion factor 3 like yolk's
# (reach 24), effective cohesion on.  Both types run the same spots.  A same-batch pair is never split -- a handle owns the
# whole batch --, so `coheres` has no ghost partner; what a ghost's batch tag must do is keep it from cohering
# (`other_batch`), also beside a mate that does cohere, and also when the ghost's batch and the particle's own are both
# the first of their handle.
CUT_UPDATES = ((H60, H60, 1, 1), (H60, H60, 2, 2))


def _probe(R):
    """(radius of the first particle, position of the second) of a 2 + 2 batch of radius R added at (0, 0)"""
    m = Plain()
    m.add(0.0, 0.0, R, R, 2, 2)
    assert m.state(WHITE)[:2, 0].tolist() == [0.0, 0.0] == m.state(YOLK)[:2, 0].tolist()  # (exactly on the centre)
    assert m.state(WHITE)[:2, 1].tolist() == m.state(YOLK)[:2, 1].tolist()
    assert m.field(WHITE, rm.RADIUS)[0] == m.field(YOLK, rm.RADIUS)[0]
    return float(m.field(WHITE, rm.RADIUS)[0]), tuple(float(v) for v in m.state(WHITE)[:2, 1])


@functools.lru_cache(maxsize=None)
def cut_case(name):
    """(batches as (x, y, R), the cut in x, [(site kind, label, particle, particle)]: the two particles, of different
    batches either side of the cut, that take the label with one another)"""
    r1, (px, py) = _probe(6.0)
    md = 2.0 * (r1 + r1)
    assert px > 0.25
    return {
        "cut_touching": (((0.0, 0.0, 6.0), (md, 0.0, 6.0)), md / 2, [("collision", "touching", 0, 2)]),
        # the second batch's centre is the first batch's second particle: global keys 1 and 2, and with a batch in between
        # (far away, on the first handle) 1 and 4 -- while on its own handle the second batch's particle has local index 0
        "cut_coincident_1": (((0.0, 0.0, 6.0), (px, py, 6.0)), px / 2, [("collision", "coincident_1", 1, 2)]),
        "cut_coincident_3": (((0.0, 0.0, 6.0), (-200.0, 0.0, 6.0), (px, py, 6.0)), px / 2, [("collision", "coincident_3", 1, 4)]),
        # R = 28: the second particle lies 19.8 px below the first (19.2 after the follow), inside the band (16, 24], and coheres
        # with it -- y = 23 puts the two into neighbouring cells of size 12; the other batch's first particle lies 20 px away
        # across the cut, inside the band too
        "cut_other_batch": (((0.0, 23.0, 28.0), (20.0, 23.0, 28.0)), 10.0, [("cohesion", "other_batch", 0, 2), ("cohesion", "coheres", 0, 1),
                                                                        ("cohesion", "coheres", 2, 3)]),
    }[name]


CUT_CASES = ("cut_touching", "cut_coincident_1", "cut_coincident_3", "cut_other_batch")


@functools.lru_cache(maxsize=None)
def cut_model(name):
    """the case on the census model: (model, ids, snapshots of tests/test_gpu_coupling.py's kind after every update)"""
    from test_gpu_collider_surfaces import _snapshot
    batches, cut, _ = cut_case(name)
    m = _scene_model(PairCensusModel, white=WHITE3, cohesion=True)
    ids = [m.add(x, y, R, R, 2, 2) for x, y, R in batches]
    snaps = []
    for u in CUT_UPDATES:
        assert m.update(*u) == 1
        snaps.append(_snapshot(m, ids))
    return m, ids, snaps


def assert_cut_labels(name):
    m, ids, snaps = cut_model(name)
    batches, cut, want = cut_case(name)
    for kind, label, p, q in want:
        for w in (WHITE, YOLK):
            site = "%s:%s" % (kind, TYPE[w])
            assert label in m.labels_of(site, p) and label in m.labels_of(site, q), (name, site, label)
        if label != "coheres":  # the two belong to batches whose centres lie either side of the cut
            assert (batches[p // 2][0] < cut) != (batches[q // 2][0] < cut), (name, label)
        else:
            assert p // 2 == q // 2
    if name.startswith("cut_coincident"):
        k = int(name[-1])
        for w in (WHITE, YOLK):
            x, y = m.starts["collision:" + TYPE[w]][0]
            p, q = want[0][2:]
            assert (x[p], y[p]) == (x[q], y[q]) and (q - p) & 7 == k
    for w in (WHITE, YOLK):
        assert np.isfinite(m.state(w)).all()
    return m, ids, snaps


@pytest.mark.parametrize("name", CUT_CASES)
def test_cut_case(name):
    m, ids, snaps = assert_cut_labels(name)
    batches = cut_case(name)[0]
    plain = _scene_model(Plain, white=WHITE3, cohesion=True)
    for x, y, R in batches:
        plain.add(x, y, R, R, 2, 2)
    for u in CUT_UPDATES:
        plain.update(*u)
    assert same_state(m, plain) and counters(m) == counters(plain)


# ------------------------------------------------------------------------------------------------ g. the coupling sweep
# one default egg (157 + 15 particles) whose target moves on the circle, six steps.  BASELINE is the only pair the device
# files held to the model so far.  (0.1, 1.0) has md = 0.8 px and H = max(1.0, 0.8) = 1.0; at (S, C) = (1, 1) no cross pair
# fires in the third step, so that combination is left to the hand case couple_small_factor.
BASELINE = (2.0, 1.0)
SWEEP = ((2.0, 0.25), (1.25, 0.9), (0.1, 1.0), (3.0, 0.0))
SWEEP_SC = ((1, 1), (3, 2))
SWEEP_CENTER, SWEEP_STEPS = (300.0, 300.0), 6
SWEEP_KEPT = tuple((cp, sc) for cp in SWEEP for sc in SWEEP_SC if (cp, sc) != ((0.1, 1.0), (1, 1)))
CHANGING = ((2.0, 0.25), (1.25, 0.9), (0.0, 1.0), (0.1, 1.0), (3.0, 0.0), (2.0, 1.0))  # set before step 1, 2, ...: off in the third


def snapshot(m, ids):
    from test_gpu_collider_surfaces import _snapshot
    return dict(_snapshot(m, ids), coupled=m.coupling_solves)


@functools.lru_cache(maxsize=None)
def sweep_run(coupling, S, C):
    """the egg on the census model with `coupling` (a pair, or "changing": CHANGING[k] before step k + 1): (model, id,
    snapshot after every step)"""
    m = _scene_model(PairCensusModel)
    i = m.add(*SWEEP_CENTER, 50, 15)
    snaps = []
    for k in range(SWEEP_STEPS):
        m.set_coupling(*(CHANGING[k] if coupling == "changing" else coupling))
        m.set_target_position(i, *circle_target(SWEEP_CENTER, k))
        assert m.update(H60, H60, S, C) == 1
        snaps.append(snapshot(m, [i]))
    return m, i, snaps


def assert_sweep(coupling, S, C):
    """cross pairs fire in every step (every step in which coupling is on), and the egg ends elsewhere than with BASELINE"""
    m, i, snaps = sweep_run(coupling, S, C)
    fired = [b["coupled"] - a["coupled"] for a, b in zip([dict(coupled=0)] + snaps, snaps)]
    on = [(CHANGING[k] if coupling == "changing" else coupling)[0] > 0.0 for k in range(SWEEP_STEPS)]
    assert all((n > 0) == o for n, o in zip(fired, on)), (coupling, S, C, fired)
    base = sweep_run(BASELINE, S, C)[2]
    for w in (WHITE, YOLK):
        assert not np.array_equal(snaps[-1]["state"][w], base[-1]["state"][w]), (coupling, S, C, w)
    for site in CPL:
        assert {"fires", "apart", "unclamped"} <= m.labels(site)
    if coupling == (0.1, 1.0):
        assert m.coupling_cell() == 1.0 and 0.1 * (4 + 4) < 1.0
    return m, i, snaps


@pytest.mark.parametrize("coupling,sc", SWEEP_KEPT + (("changing", (3, 2)),))
def test_sweep_on_the_model(coupling, sc):
    assert_sweep(coupling, *sc)


def test_the_sweep_leaves_one_combination_to_the_hand_table():
    m, i, snaps = sweep_run((0.1, 1.0), 1, 1)
    assert snaps[2]["coupled"] == snaps[1]["coupled"] > 0  # no cross pair fires in the third step
    assert "couple_small_factor" in CASES and CASES["couple_small_factor"]["coupling"] == (0.1, 1.0)


# ------------------------------------------------------------------------------------------------ h. unequal types
# one batch whose types differ in count so far that their hash tables differ in size: the host sizes a type's table as
# the least power of two >= 1024 that is >= 2 n, so 613 particles get 2048 slots and 2 get 1024.  With coupling on, each
# side of the coupling pass walks the OTHER type's table: a mask taken from the own type's would miss cells.
UNEQUAL = {"many_whites": (613, 2), "many_yolks": (2, 613)}
UNEQUAL_UPDATES = 3


def table_slots(n):
    """the host's sizing rule, restated: reserve_relaxed() in egg_fluid_simulation_amd/csrc/eggsim_host_relaxed.hip (`table = 1024;
    while (table < 2 * ne) table <<= 1`, ne = the type's particles plus ghosts; a single handle has no ghosts).  The library
    does not report the size: if that rule changes, change this one with it, or the two tables of UNEQUAL may come out equal
    on the device while this test still says they differ."""
    slots = 1024
    while slots < 2 * n:
        slots *= 2
    return slots


@functools.lru_cache(maxsize=None)
def unequal_run(name):
    nw, ny = UNEQUAL[name]
    m = _scene_model(PairCensusModel, coupling=BASELINE)
    i = m.add(*SWEEP_CENTER, 50, 50, nw, ny)
    snaps = []
    for k in range(UNEQUAL_UPDATES):
        m.set_target_position(i, *circle_target(SWEEP_CENTER, k))
        assert m.update(H60, H60, 2, 2) == 1
        snaps.append(snapshot(m, [i]))
    return m, i, snaps


def assert_unequal(name):
    m, i, snaps = unequal_run(name)
    nw, ny = UNEQUAL[name]
    assert table_slots(nw) != table_slots(ny) and {table_slots(nw), table_slots(ny)} == {1024, 2048}
    assert all(n % 64 and n % 256 for n in (nw, ny))
    fired = [b["coupled"] - a["coupled"] for a, b in zip([dict(coupled=0)] + snaps, snaps)]
    assert min(fired) > 0, fired
    for site in CPL:
        assert {"fires", "apart"} <= m.labels(site), (name, site)
    return m, i, snaps


@pytest.mark.parametrize("name", sorted(UNEQUAL))
def test_unequal_types_on_the_model(name):
    assert_unequal(name)
