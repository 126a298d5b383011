"""The census of the exact-order pair projection (tests/exact_census.py) without a device: classify() on single evaluations,
the hand table that plants every guard-deciding pair, the wrong rules the table must notice, and which labels the existing
device scenes reach.  tests/test_gpu_exact_edges.py runs the hand table on the device under every projection site.

The hand table: 1 to 5 batches of 2 particles per type; every particle rests inside its batch's follow radius (target (0, 0),
batch radius 2500: the follow distance is 100), so pre-solve and the follow constraint move nothing and the first collision
pass sees the planted geometry.  Both types carry the same spots.  Radius 2 and overlap 2.5: md = 10, cell size 5.  One
update of (S, C) = (1, 1), then one of (2, 3).  The budget of n particles is 0.05 n^2 pairs per pass -- 1 pair for 2 or 4
particles, 4 for 8, 5 for 10 --, so the planted pair is always particle 0's first visit.

label             case(s) that plant it (both collision sites; asserted on the census by assert_case)
  axis_x            axis_x: four pairs, dx = (+0) - (+0), (-0) - (+0), (+0) - (-0), (-0) - (-0)
  axis_y            axis_y (the same on the other axis), clamp_hi_axis, at_eps
  edge              edge (6-8-10, moves nothing), edge_negzero (moves nothing but turns the -0.0 of particle 0's x into +0.0).
                    An edge pair ON an axis cannot be visited: md is two cells, and cells two apart are not neighbours
  fast              inside_edge (one ulp inside the edge), clamp_hi, heavy_and_light, cells_a, cells_b, budget_cut
  apart             outside_edge (one ulp outside)
  coincident_same   coincident_same_negzero at (-0.0, -0.0); below_eps_subnormal (5e-324 apart: d2 underflows to 0)
  coincident_other  coincident_other at (-0.0, -0.0)
  below_eps         below_eps_1e9, below_eps_1e160
  tiny_component    tiny_component (dx = 5e-324 beside dy = 4), below_eps_1e160, below_eps_subnormal
  clamp_hi          clamp_hi (3-4-5), clamp_hi_axis: collision_strength 1, masses of 4; lands at x = -0.5 and 6.5
  unclamped         every other firing case
  guarded           guarded (inverse masses 1e-9 + 1e-9); pair_solves stays 0
  budget cut        budget_cut: the cut falls on the planted pair (0, 1), the pair (2, 3) waits for the next pass
  neighbour cells   cells_a, cells_b: particle 0 in cell (0, 0), a partner in each of the eight neighbour cells, across the origin
follow sites: rests (every case), rests_at_edge (follow_edge: (-0.0, 100.0)), pulled (pulled), massless (guarded)"""
import functools
import math

import numpy as np
import pytest

import exact_census as ec
from exact_census import WHITE, YOLK, ExactCensusModel, classify, classify_follow
from oracle import reference_model as rm
from oracle.reference_model import ReferenceModel

H60 = 1 / 60
UPDATES = ((H60, H60, 1, 1), (H60, H60, 2, 3))
FIELDS = ("x", "y", "vx", "vy", "last_x", "last_y")
OFFSETS = (rm.X, rm.Y, rm.VX, rm.VY, rm.LAST_X, rm.LAST_Y)
HAND_RADIUS, HAND_TARGET = 2500.0, (0.0, 0.0)
BASE = dict(min_radius=2, max_radius=2, cohesion_interaction_distance_factor=2.5, collision_overlap_factor=2.5)
CONFIGS = {
    "plain": {},
    "heavy": dict(max_mass=1e9),  # "hi": inverse mass 1e-9
    "stiff": dict(min_mass=4, max_mass=8, collision_strength=1),  # wsum 0.5, compliance 0: correction = 2 |violation|
}
RING = ((60.0, 0.0), (52.0, 30.0), (30.0, 52.0), (0.0, 60.0), (-30.0, 52.0), (-52.0, 30.0), (-60.0, 0.0), (-52.0, -30.0),
        (-30.0, -52.0), (0.0, -60.0))
PARK = {WHITE: RING, YOLK: tuple((1.4 * x, 1.4 * y) for x, y in RING)}
NZ = -0.0
IN85, OUT85 = float(np.nextafter(8.5, 0.0)), float(np.nextafter(8.5, 9.0))
CELLS = tuple((ox, oy) for ox in (-1, 0, 1) for oy in (-1, 0, 1) if (ox, oy) != (0, 0))


def _cell_spots(cells):
    return [(2.0, 2.0)] + [(2.25 + 4.0 * ox, 1.5 + 4.0 * oy) for ox, oy in cells] + [None] * 5


def _case(spots, cfg="plain", want=(), first=None, follow=("rests",)):
    """spots: per particle (x, y) or (x, y, "hi") or None (parked on the ring); want: labels both collision sites must take;
    first: labels the very first evaluation of either site must carry (the planted pair (0, 1)); follow: labels of the follow sites"""
    assert len(spots) % 2 == 0
    return dict(spots=tuple(spots), cfg=cfg, want=set(want), first=set(want if first is None else first), follow=set(follow))


CASES = {
    "axis_x": _case([(0.0, 1.0), (0.0, 5.0), (0.0, 31.0), (NZ, 35.0), (NZ, 61.0), (0.0, 65.0), (NZ, -29.0), (NZ, -25.0)], want={"fires", "axis_x", "unclamped"}),
    "axis_y": _case([(1.0, 0.0), (5.0, 0.0), (31.0, 0.0), (35.0, NZ), (61.0, NZ), (65.0, 0.0), (-29.0, NZ), (-25.0, NZ)], want={"fires", "axis_y", "unclamped"}),
    "coincident_same_negzero": _case([(NZ, NZ), (NZ, NZ)], want={"fires", "coincident_same", "unclamped"}),
    "coincident_other": _case([(NZ, NZ), None, (NZ, NZ), None], want={"fires", "coincident_other", "unclamped"}),
    "edge": _case([(0.5, 0.5), (6.5, 8.5)], want={"fires", "edge", "unclamped"}),
    "edge_negzero": _case([(NZ, 0.5), (6.0, 8.5)], want={"fires", "edge", "unclamped"}),
    "inside_edge": _case([(0.5, 0.5), (6.5, IN85)], want={"fires", "fast", "unclamped"}),
    "outside_edge": _case([(0.5, 0.5), (6.5, OUT85)], want={"apart"}),
    "below_eps_1e9": _case([(0.0, 0.0), (1e-9, 0.0)], want={"fires", "below_eps", "unclamped"}),
    "below_eps_1e160": _case([(0.0, 0.0), (1e-160, 0.0)], want={"fires", "below_eps", "tiny_component", "unclamped"}),
    "below_eps_subnormal": _case([(0.0, 0.0), (5e-324, 0.0)], want={"fires", "coincident_same", "tiny_component", "unclamped"}),
    "tiny_component": _case([(0.0, 0.0), (5e-324, 4.0)], want={"fires", "tiny_component", "unclamped"}),
    "at_eps": _case([(0.0, 0.0), (1e-8, 0.0)], want={"fires", "axis_y", "unclamped"}),
    "clamp_hi": _case([(1.0, 2.0), (4.0, 6.0)], cfg="stiff", want={"fires", "clamp_hi", "fast"}),
    "clamp_hi_axis": _case([(1.0, 2.0), (5.0, 2.0)], cfg="stiff", want={"fires", "clamp_hi", "axis_y"}),
    "guarded": _case([(0.0, 0.0, "hi"), (4.0, 0.0, "hi")], cfg="heavy", want={"guarded"}, follow={"massless"}),
    "heavy_and_light": _case([(0.0, 0.0, "hi"), (4.0, 3.0)], cfg="heavy", want={"fires", "fast", "unclamped"}, follow={"massless", "rests"}),
    "cells_a": _case(_cell_spots(CELLS[:4]), want={"fires", "fast", "unclamped"}),
    "cells_b": _case(_cell_spots(CELLS[4:]), want={"fires", "fast", "unclamped"}),
    "budget_cut": _case([(1.0, 2.0), (4.0, 6.0), (31.0, 2.0), (34.0, 6.0)], want={"fires", "fast", "unclamped"}),
    "follow_edge": _case([(NZ, 100.0), None], follow={"rests_at_edge", "rests"}),
    "pulled": _case([(0.0, 150.0), None], follow={"pulled", "rests"}),
}
# a wrong rule -> the case whose bits (or pair count) it changes
CAUGHT_BY = {"edge_excluded": "edge_negzero", "eps_inclusive": "at_eps", "zero_sign_lost": "axis_x", "no_plus_zero": "coincident_same_negzero",
             "guard_counts": "guarded", "clamp_missing": "clamp_hi", "follow_edge_pulls": "follow_edge"}

# ballast beside the planted batches (tests/test_gpu_exact_edges.py: what each device variant needs)
FAR_N, FAR_CENTER, FAR_PITCH = 64, (5000.0, 0.0), 12.0  # one batch of 64 + 64 resting particles on an 8 x 8 grid: lifts the budget
# (64: more than the 60 particles up to which small islands are packed into one tile, so it stays a tile of its own)
BLOB_CENTER = (-150.0, 0.0)                            # two default batches on one centre: 314 white particles in one island
MANY, MANY_PITCH, MANY_ORIGIN, MANY_RADIUS = 1030, 400.0, 20000.0, 100.0  # more one-tile groups than an MI355X has SIMDs
BALLAST = (None, "far", "blob", "many")


def configs(name):
    w, y = rm.default_configs()
    return dict(w, **BASE, **CONFIGS[CASES[name]["cfg"]]), dict(y, **BASE, **CONFIGS[CASES[name]["cfg"]])


def spots(name, which):
    out = []
    for p, s in enumerate(CASES[name]["spots"]):
        s = PARK[which][p] if s is None else s
        out.append((float(s[0]), float(s[1]), 1.0 if len(s) > 2 else 0.0))
    return out


def _columns(cfg, rows):
    """the nine rows of egg_export_batch (x y vx vy last_x last_y inverse mass radius t) for (x, y, t) rows, t in {0, 1}"""
    cols = np.zeros((9, len(rows)))
    for p, (x, y, t) in enumerate(rows):
        mass = cfg["max_mass"] if t else cfg["min_mass"]
        assert rm.mix(cfg["min_mass"], cfg["max_mass"], t) == mass
        # a coordinate at -0.0 carries a velocity of -0.0: pre-solve's x + h v keeps the sign only then (-0.0 + 0.0 is +0.0)
        vx, vy = (-0.0 if v == 0.0 and math.copysign(1.0, v) < 0 else 0.0 for v in (x, y))
        cols[:, p] = (x, y, vx, vy, x, y, 1 / mass, rm.mix(cfg["min_radius"], cfg["max_radius"], t), t)
    return cols


def columns(name, which):
    return _columns(configs(name)[which], spots(name, which))


def far_columns(name, which):
    grid = [(FAR_CENTER[0] + FAR_PITCH * (k % 8 - 3.5), FAR_CENTER[1] + FAR_PITCH * (k // 8 - 3.5), 0.0) for k in range(FAR_N)]
    return _columns(configs(name)[which], grid)


def many_centers(name):
    """MANY ballast batches on a far grid, each of one white particle fewer than the case plants (at least 2) and 2 yolk
    ones: with one tile to a group every ballast tile is a group of its own, and the planted particles -- one tile, or
    islands of two -- are within a factor of two of them, hence in the same launch class (retile(): a class holds the tiles
    with more than half the particles of its largest)"""
    k = np.arange(MANY)
    return MANY_ORIGIN + MANY_PITCH * (k % 40), MANY_ORIGIN + MANY_PITCH * (k // 40), max(2, len(CASES[name]["spots"]) - 1)


def _write(data, cols, first_particle):
    for p in range(cols.shape[1]):
        x, y, vx, vy, _, _, inv, radius, t = (float(v) for v in cols[:, p])
        for off, v in ((rm.X, x), (rm.Y, y), (rm.PX, x), (rm.PY, y), (rm.LAST_X, x), (rm.LAST_Y, y), (rm.VX, vx), (rm.VY, vy),
                       (rm.MASS_T, t), (rm.MASS, 1 / inv), (rm.INV_MASS, inv), (rm.RADIUS, radius)):
            data[rm.offset(first_particle + p + 1) + off] = v


def bits(values):
    return np.array(values, dtype=np.float64).view(np.uint64)


def snapshot(m, ids):
    return dict(state={w: {f: bits(m.field(w, off)) for f, off in zip(FIELDS, OFFSETS)} for w in (WHITE, YOLK)},
                pos={i: tuple(bits(m.get_position(i)).tolist()) for i in ids}, pairs=getattr(m, "pair_solves", None))


def run(name, ballast=None, rule=None, cls=ExactCensusModel):
    """the case on a model; returns (model, ids of the planted batches, [snapshot after every update])"""
    assert ballast in BALLAST
    m = cls(*configs(name), rule=rule) if cls is ExactCensusModel else cls(*configs(name))
    n = len(CASES[name]["spots"])
    ids = [m.add(*HAND_TARGET, HAND_RADIUS, HAND_RADIUS, 2, 2) for _ in range(n // 2)]
    for w, data in ((WHITE, m._white_data), (YOLK, m._yolk_data)):
        _write(data, columns(name, w), 0)
    if ballast == "far":
        m.add(*FAR_CENTER, HAND_RADIUS, HAND_RADIUS, FAR_N, FAR_N)
        for w, data in ((WHITE, m._white_data), (YOLK, m._yolk_data)):
            _write(data, far_columns(name, w), n)
    elif ballast == "blob":
        for _ in range(2):
            m.add(*BLOB_CENTER, 50, 15, 157, 15)  # (a default batch's counts: the radius of 2 here would make 625)
    elif ballast == "many":
        xs, ys, nw = many_centers(name)
        for x, y in zip(xs, ys):
            m.add(float(x), float(y), MANY_RADIUS, MANY_RADIUS, nw, 2)
    snaps = []
    for u in UPDATES:
        assert m.update(*u) == 1
        snaps.append(snapshot(m, ids))
    return m, ids, snaps


@functools.lru_cache(maxsize=None)
def model(name, ballast=None):
    return run(name, ballast)


def assert_case(name, ballast=None):
    """the case takes the branches it is there for, on the model (with the ballast of the device variant, if any)"""
    m, ids, snaps = model(name, ballast)
    c = CASES[name]
    for w, site in enumerate(ec.COLLISION_SITES):
        assert c["want"] <= m.labels(site), (name, ballast, site, m.census[site])
        if not c["want"]:  # (a lone particle beside a parked one: the case is about the follow site)
            continue
        a, b, labels = m.first[site][0]  # the planted pair is the very first evaluation
        assert (a, b) == (0, 2 if name == "coincident_other" else 1) and c["first"] <= labels, (name, site, m.first[site][0])
        assert not m.labels(site) & set(ec.UNREACHABLE)
        for f in FIELDS:
            assert np.isfinite(snaps[-1]["state"][w][f].view(np.float64)).all()
    for site in ec.FOLLOW_SITES:
        assert c["follow"] <= m.labels(site), (name, site, m.census[site])
    return m, ids, snaps


def same(a, b):
    return all(np.array_equal(a["state"][w][f], b["state"][w][f]) for w in (WHITE, YOLK) for f in FIELDS) and a["pos"] == b["pos"]


# ------------------------------------------------------------------------------------------------ classify() alone
def _one(a, b, wa=1.0, wb=1.0, same_batch=True, compliance=9.0, ra=2.0):
    return classify(a[0], a[1], b[0], b[1], wa, wb, ra, ra, same_batch, 2.5, compliance)


def test_classify_names_one_evaluation():
    assert _one((0.0, 0.0), (3.0, 4.0)) == {"fires", "unclamped", "fast"}
    assert _one((0.0, 0.0), (6.0, 8.0)) == {"fires", "edge", "unclamped"}
    assert _one((0.0, 0.0), (6.0, OUT85 - 0.5)) == {"apart"} and _one((0.0, 0.0), (0.0, 11.0)) == {"apart"}
    assert _one((0.0, 0.0), (NZ, 4.0)) == {"fires", "axis_x", "unclamped"} and _one((NZ, 0.0), (4.0, 0.0)) == {"fires", "axis_y", "unclamped"}
    assert _one((1.0, 1.0), (1.0, 1.0)) == {"fires", "coincident_same", "unclamped"}
    assert _one((1.0, 1.0), (1.0, 1.0), same_batch=False) == {"fires", "coincident_other", "unclamped"}
    assert _one((0.0, 0.0), (1e-9, 0.0)) == {"fires", "below_eps", "unclamped"}
    assert _one((0.0, 0.0), (5e-324, 4.0)) == {"fires", "tiny_component", "unclamped"}
    assert _one((0.0, 0.0), (3.0, 4.0), 0.25, 0.25, compliance=0.0) == {"fires", "clamp_hi", "fast"}
    assert _one((0.0, 0.0), (3.0, 4.0), 1e-9, 1e-9) == {"guarded"}
    assert classify_follow(0.0, 99.0, 0.0, 0.0, 1.0, 50.0) == "rests" and classify_follow(NZ, 100.0, 0.0, 0.0, 1.0, 50.0) == "rests_at_edge"
    assert classify_follow(0.0, 101.0, 0.0, 0.0, 1.0, 50.0) == "pulled" and classify_follow(0.0, 101.0, 0.0, 0.0, 1e-8, 50.0) == "massless"


def test_labels_that_cannot_occur_in_a_step():
    """dead needs a negative compliance, huge_divisor a mass below 2^-299, huge_reach a radius beyond 2^298"""
    assert "dead" in _one((0.0, 0.0), (3.0, 4.0), compliance=-2.0)
    assert "huge_divisor" in _one((0.0, 0.0), (3.0, 4.0), wa=2.0 ** 301) and "fast" not in _one((0.0, 0.0), (3.0, 4.0), wa=2.0 ** 301)
    assert "huge_reach" in _one((0.0, 0.0), (3.0, 4.0), ra=2.0 ** 299)
    assert not _one((0.0, 0.0), (3.0, 4.0), compliance=1e16) & set(ec.UNREACHABLE)  # the largest compliance a step can have


# ------------------------------------------------------------------------------------------------ the hand table
@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_case(name):
    m, ids, snaps = assert_case(name)
    plain, _, plain_snaps = run(name, cls=ReferenceModel)  # recording is free
    assert all(same(a, b) for a, b in zip(snaps, plain_snaps))
    assert m.pair_solves == 0 if name in ("guarded", "follow_edge", "pulled") else m.pair_solves > 0
    start = {w: (bits([s[0] for s in spots(name, w)]), bits([s[1] for s in spots(name, w)])) for w in (WHITE, YOLK)}
    for w in (WHITE, YOLK):
        x, y = snaps[0]["state"][w]["x"], snaps[0]["state"][w]["y"]
        if name in ("edge", "outside_edge", "guarded"):  # nothing moves, no zero to change
            assert np.array_equal(x, start[w][0]) and np.array_equal(y, start[w][1])
        if name == "edge_negzero":  # violation 0: the shares are zeros, and particle 0's -0.0 + 0.0 is +0.0
            assert x.tolist() == bits([0.0, 6.0]).tolist() and y.tolist() == bits([0.5, 8.5]).tolist()
        if name == "coincident_same_negzero":  # the cohesion block's + 0.0, then a zero normal
            assert x.tolist() == y.tolist() == bits([0.0, 0.0]).tolist()
        if name == "coincident_other":  # no cohesion block: the self particle keeps its -0.0
            assert x[[0, 2]].tolist() == y[[0, 2]].tolist() == bits([NZ, 0.0]).tolist()
        if name == "clamp_hi_axis":  # |violation| = 6, inverse masses 1/4: 1.5 each
            assert x.tolist() == bits([-0.5, 6.5]).tolist() and y.tolist() == bits([2.0, 2.0]).tolist()
        # a: x + (-nx c w), b: x + (nx c w), c > 0.  dx = (-0) - (+0) = -0.0 is the one negative zero: b keeps its -0.0 there (a lost
        # sign of dx would make it +0.0); a -0.0 of a stays wherever dx = +0.0, a -0.0 of b becomes +0.0 there
        if name == "axis_x":
            assert x.tolist() == bits([0.0, 0.0, 0.0, NZ, NZ, 0.0, NZ, 0.0]).tolist()
        if name == "axis_y":
            assert y.tolist() == bits([0.0, 0.0, 0.0, NZ, NZ, 0.0, NZ, 0.0]).tolist()
    if name == "budget_cut":
        assert ("collision:white", 0, 1) in m.cut_on and ("collision:yolk", 0, 1) in m.cut_on
        assert [(a, b) for a, b, _ in m.first["collision:white"]] == [(0, 1)]
    if name.startswith("cells_"):
        want = CELLS[:4] if name == "cells_a" else CELLS[4:]
        s = spots(name, WHITE)
        assert (math.floor(s[0][0] / 5.0), math.floor(s[0][1] / 5.0)) == (0, 0)
        assert tuple((math.floor(x / 5.0), math.floor(y / 5.0)) for x, y, _ in s[1:5]) == want
        assert {(a, b) for a, b, _ in m.first["collision:white"]} >= {(0, 1), (0, 2), (0, 3), (0, 4)}


def test_the_hand_table_holds_every_label():
    reached = {site: set() for site in ec.COLLISION_SITES + ec.FOLLOW_SITES}
    for name in CASES:
        m, _, _ = model(name)
        for site in reached:
            reached[site] |= m.labels(site)
    for site in ec.COLLISION_SITES:
        assert reached[site] == set(ec.COLLISION_LABELS), (site, set(ec.COLLISION_LABELS) ^ reached[site])
    for site in ec.FOLLOW_SITES:
        assert reached[site] == set(ec.FOLLOW_LABELS), (site, reached[site])
    # all four sign combinations of the aligned coordinate
    for name, k in (("axis_x", 0), ("axis_y", 1)):
        signs = {(math.copysign(1.0, a[k]), math.copysign(1.0, b[k])) for a, b in zip(CASES[name]["spots"][0::2], CASES[name]["spots"][1::2])}
        assert len(signs) == 4


@pytest.mark.parametrize("ballast", ["far", "blob"])
def test_the_ballast_leaves_the_planted_pairs_alone(ballast):
    """with the ballast of a device variant the planted pair is still the first evaluation and carries its labels"""
    for name in ("axis_x", "edge_negzero", "clamp_hi", "guarded", "cells_b"):
        m, _, _ = assert_case(name, ballast)
        if ballast == "far":
            assert m.cuts == 0  # ... and the budget does not bind any more
        else:  # (30 yolk particles in one spot: the yolk budget of the blob scene binds, the white one must not in the first pass)
            assert not any(site == "collision:white" for site, _, _ in m.cut_on[:1])


# ------------------------------------------------------------------------------------------------ wrong rules
@pytest.mark.parametrize("rule", ec.RULES)
def test_a_wrong_rule_changes_a_case(rule):
    name = CAUGHT_BY[rule]
    _, _, right = model(name)
    _, _, wrong = run(name, rule=rule)
    assert not (same(right[-1], wrong[-1]) and right[-1]["pairs"] == wrong[-1]["pairs"]), (rule, name)
    if rule != "guard_counts":  # (a counted guarded pair shows in pair_solves alone: a 2-particle scene has no other pair to cut)
        assert not same(right[0], wrong[0]), (rule, name)


def test_the_rules_are_each_caught_by_a_case_of_their_own():
    assert set(CAUGHT_BY) == set(ec.RULES) and set(CAUGHT_BY.values()) <= set(CASES)


# ------------------------------------------------------------------------------------------------ existing device scenes
def _drive(m, centers, steps, S=2, C=3, counts=(40, 8), move=(5.0, 3.0)):
    ids = [m.add(x, y, 50, 15, *counts) for x, y in centers]
    for k in range(steps):
        for i, (x, y) in zip(ids, centers):
            m.set_target_position(i, x + move[0] * k, y + move[1] * k)
        m.update(H60, H60, S, C)
    return m


def _fuzz_like(seed):
    rng = np.random.default_rng(seed)
    m = ExactCensusModel()
    centers = [tuple(float(v) for v in rng.uniform(0, 120, 2)) for _ in range(3)]
    return _drive(m, centers, 6, counts=(int(rng.integers(20, 40)), 8), move=tuple(float(v) for v in rng.uniform(-6, 6, 2)))


def _mass(tweak):
    w, y = rm.default_configs()
    return _drive(ExactCensusModel(dict(w, **tweak), dict(y, **tweak)), [(300.0, 300.0), (340.0, 320.0)], 4)


def _sub_eps():
    m = ExactCensusModel()
    for x, y, wr, yr, wn, yn in ((0.0, 0.0, 40.0, 40.0, 2, 2), (0.0, 0.0, 40.0, 40.0, 2, 2), (200.0, 50.0, 1e-9, 1e-9, 12, 6)):
        m.add(x, y, wr, yr, wn, yn)
    for k in range(3):
        m.update(H60, H60, 2, 3)
    return m


EXISTING = {
    "fuzz_1": lambda: _fuzz_like(1), "fuzz_2": lambda: _fuzz_like(2), "fuzz_3": lambda: _fuzz_like(3),
    "mass_mixed": lambda: _mass(dict(max_mass=1e9)), "mass_all_guarded": lambda: _mass(dict(min_mass=3e8, max_mass=1e9)),
    "sub_eps": _sub_eps,
    "config3_coincident": lambda: _drive(ExactCensusModel(), [(300.0, 300.0)] * 4, 3, move=(0.0, 0.0)),
}
GUARD_DECIDING = {"edge", "axis_x", "axis_y", "tiny_component", "clamp_hi"}


@pytest.mark.parametrize("name", sorted(EXISTING))
def test_what_the_existing_device_scenes_reach(name):
    """the scenes of test_gpu_fuzz.random_session, test_gpu_round2's mass and sub-eps cases and config 3's coincident batches
    at reduced size: none plants an aligned pair, an edge pair, a tiny component or the clamp (the table in exact_census.py)"""
    m = EXISTING[name]()
    got = {site: sorted(m.labels(site)) for site in ec.COLLISION_SITES + ec.FOLLOW_SITES}
    print(name, got, "pairs", m.pair_solves, "cut passes", m.cuts)
    for site in ec.COLLISION_SITES:
        assert not m.labels(site) & GUARD_DECIDING, (name, site, m.census[site])
