"""The rule of the probes (include/eggsim.h, "probes"; tests/probe_model.py) on a hand table: per case a few batches with a
few particles (x, y, radius) per type, a list of probes, and -- written down by hand -- the winner of every (probe, type):
which batch, which index in it, and the score as a literal.  Every number of the table is chosen so that the rule's
arithmetic is exact and can be followed on paper (the comments do).  Every wrong rule of probe_model.WRONG_RULES is told
from the right one by at least one case.  tests/test_gpu_probes.py runs the same table on the device.  No GPU."""
import math

import numpy as np
import pytest

import probe_model as pm

UP, DOWN = math.inf, -math.inf
NAN = float("nan")
E = 2.0 ** -20  # a step that every product below still holds exactly


def nxt(v, towards):
    return float(np.nextafter(v, towards))


# a batch holds at least two particles of each type: these stand far from every probe and ray of the table
FILL = [(1.0e6, 1.0e6, 1.0), (1.0e6 + 8.0, 1.0e6, 1.0)]
X_RAY = ("ray", 0.0, 0.0, 10.0, 0.0)  # along +x: ex = 10, ey = 0, l2 = 100, b = 10 fx


def batch(key, white, yolk):
    """a batch by its key; its id is its position in the case's list + 1 (the order of the imports)"""
    return dict(key=key, white=list(white) + FILL[:max(0, 2 - len(white))], yolk=list(yolk) + FILL[:max(0, 2 - len(yolk))])


# name: batches (in id order), probes, want = per probe (white, yolk), each None or (position of the batch in the list, index
# in the batch, score); first = per probe what pick / raycast make of the pair
CASES = {
    # d2 = 9 + 16 = 25 = reach reach is a candidate; the yolk is one ulp further out: 25 + 2 * 5 ulp(5) > 25
    "point_at_the_reach": dict(
        batches=[batch(1, [(3.0, 4.0, 1.0)], [(0.0, nxt(5.0, UP), 1.0)])],
        probes=[("point", 0.0, 0.0, 5.0), ("point", 0.0, 0.0, nxt(5.0, DOWN))],
        want=[((0, 0, 25.0), None), (None, None)], first=["white", None]),
    # reach = 0 holds exactly a centre on the point
    "point_reach_zero": dict(
        batches=[batch(1, [(7.0, -2.0, 1.0), (7.0, nxt(-2.0, UP), 1.0)], [(7.5, -2.0, 1.0)])],
        probes=[("point", 7.0, -2.0, 0.0)],
        want=[((0, 0, 0.0), None)], first=["white"]),
    # reach = inf (the default): the nearest, wherever it is; 900 + 1600 and 360000 + 640000
    "point_reach_inf": dict(
        batches=[batch(1, [(1000.0, 0.0, 1.0), (-30.0, 40.0, 2.0)], [(600.0, 800.0, 3.0)])],
        probes=[("point", 0.0, 0.0)],
        want=[((0, 1, 2500.0), (0, 0, 1000000.0))], first=["white"]),
    # three particles of one batch at d2 = 25: the lowest index
    "point_tie_in_a_batch": dict(
        batches=[batch(1, [(9.0, 9.0, 1.0), (5.0, 0.0, 1.0), (0.0, 5.0, 1.0), (-5.0, 0.0, 1.0)], [(0.0, -5.0, 1.0), (-3.0, 4.0, 1.0)])],
        probes=[("point", 0.0, 0.0)],
        want=[((0, 1, 25.0), (0, 0, 25.0))], first=["white"]),
    # two coincident batches: the one imported first (id 1) has the HIGHER key, so the lower key is id 2
    "point_coincident_batches": dict(
        batches=[batch(2, [(10.0, 10.0, 1.0)], [(10.0, 10.0, 0.5)]), batch(1, [(10.0, 10.0, 1.0)], [(10.0, 10.0, 0.5)])],
        probes=[("point", 10.0, 10.0), ("point", 13.0, 14.0, 5.0, "yolk")],
        want=[((1, 0, 0.0), (1, 0, 0.0)), (None, (1, 0, 25.0))], first=["white", "yolk"]),
    # white and yolk at the same score: both are reported, pick takes the white
    "point_white_and_yolk_equal": dict(
        batches=[batch(1, [(3.0, 4.0, 1.0)], [(-4.0, 3.0, 2.0)])],
        probes=[("point", 0.0, 0.0)],
        want=[((0, 0, 25.0), (0, 0, 25.0))], first=["white"]),
    # a NaN coordinate is a candidate for nothing, however near its other coordinate is
    "point_nan_position": dict(
        batches=[batch(1, [(NAN, 0.0, 1.0), (6.0, 8.0, 1.0)], [(0.0, NAN, 1.0), (NAN, NAN, 1.0)])],
        probes=[("point", 0.0, 0.0, 50.0)],
        want=[((0, 1, 100.0), None)], first=["white"]),
    # a NaN radius is a candidate for nothing, although a point probe compares centres only
    "point_nan_radius": dict(
        batches=[batch(1, [(1.0, 0.0, NAN), (6.0, 8.0, 1.0)], [(0.0, 2.0, NAN), (0.0, 3.0, NAN)])],
        probes=[("point", 0.0, 0.0, 50.0)],
        want=[((0, 1, 100.0), None)], first=["white"]),
    # the mask excludes the nearer type
    "point_mask": dict(
        batches=[batch(1, [(1.0, 0.0, 1.0)], [(2.0, 0.0, 1.0)])],
        probes=[("point", 0.0, 0.0, math.inf, "yolk"), ("point", 0.0, 0.0, math.inf, "white"), ("point", 0.0, 0.0, math.inf, 3)],
        want=[(None, (0, 0, 4.0)), ((0, 0, 1.0), None), ((0, 0, 1.0), (0, 0, 4.0))], first=["yolk", "white", "white"]),
    # the ray starts inside the white disc (c = 1 - 4): t = 0; the yolk ahead: c = 25 - 1, b = -50, q = 2500 - 2400,
    # t = (50 - 10) / 100
    "ray_start_inside": dict(
        batches=[batch(1, [(1.0, 0.0, 2.0)], [(5.0, 0.0, 1.0)])],
        probes=[X_RAY],
        want=[((0, 0, 0.0), (0, 0, 0.4))], first=["white"]),
    # exactly on the rim: c = 4 - 4 = 0 and c = 9 - 9 = 0 are candidates with t = 0, also for a disc beside the ray's line
    "ray_start_on_the_rim": dict(
        batches=[batch(1, [(2.0, 0.0, 2.0)], [(0.0, 3.0, 3.0)])],
        probes=[X_RAY],
        want=[((0, 0, 0.0), (0, 0, 0.0))], first=["white"]),
    # tangent: c = 26 - 1 = 25 and 29 - 4 = 25, q = 2500 - 100 * 25 = 0, t = 50 / 100
    "ray_tangent": dict(
        batches=[batch(1, [(5.0, 1.0, 1.0)], [(5.0, -2.0, 2.0)])],
        probes=[X_RAY],
        want=[((0, 0, 0.5), (0, 0, 0.5))], first=["white"]),
    # 2^-20 further from the line: c = 25 + 2^-19 + 2^-40 exactly, q = -100 (2^-19 + 2^-40) < 0
    "ray_just_missing": dict(
        batches=[batch(1, [(5.0, 1.0 + E, 1.0)], [(5.0, -(2.0 + E), 2.0)])],
        probes=[X_RAY],
        want=[(None, None)], first=[None]),
    # the end of the segment: c = 121 - 1, b = -110, q = 12100 - 12000, t = (110 - 10) / 100 = 1 is a hit; 2^-20 further
    # along (every product is exact, q = 100 again) t = (100 + 10 * 2^-20) / 100 > 1 is none
    "ray_end": dict(
        batches=[batch(1, [(11.0, 0.0, 1.0)], [(11.0 + E, 0.0, 1.0)])],
        probes=[X_RAY],
        want=[((0, 0, 1.0), None)], first=["white"]),
    # a disc behind the start: b = 50 and b = 30 are not < 0, although the ray's LINE passes through both
    "ray_disc_behind": dict(
        batches=[batch(1, [(-5.0, 0.0, 1.0)], [(-3.0, 0.0, 1.0)])],
        probes=[X_RAY],
        want=[(None, None)], first=[None]),
    # pad turns a miss into a hit: white c = 34 - 1 (q < 0) becomes 34 - 9 = 25, tangent; yolk c = 41 - 4 becomes 41 - 16
    "ray_pad": dict(
        batches=[batch(1, [(5.0, 3.0, 1.0)], [(5.0, -4.0, 2.0)])],
        probes=[X_RAY, X_RAY + (2.0,), X_RAY + (2.0, "yolk")],
        want=[(None, None), ((0, 0, 0.5), (0, 0, 0.5)), (None, (0, 0, 0.5))], first=[None, "white", "yolk"]),
    # two discs at equal t, in two batches whose keys run against their ids, and two in one batch
    "ray_equal_t": dict(
        batches=[batch(2, [(5.0, 1.0, 1.0)], [(9.0, 9.0, 1.0), (5.0, 2.0, 2.0), (5.0, -2.0, 2.0)]),
                 batch(1, [(5.0, -1.0, 1.0)], [(9.0, 9.0, 1.0), (8.0, 8.0, 1.0)])],
        probes=[X_RAY],
        want=[((1, 0, 0.5), (0, 1, 0.5))], first=["white"]),
}

# the case(s) that must notice each wrong rule
NOTICED_BY = {
    "strict_reach": ["point_at_the_reach", "point_reach_zero"],
    "ties_to_highest": ["point_tie_in_a_batch", "point_coincident_batches", "ray_equal_t"],
    "ties_by_id": ["point_coincident_batches", "ray_equal_t"],
    "ray_ignores_radius": ["ray_start_inside", "ray_tangent", "ray_pad"],
    "ray_ignores_pad": ["ray_pad"],
    "inside_is_a_miss": ["ray_start_inside", "ray_start_on_the_rim"],
    "behind_accepted": ["ray_disc_behind"],
    "beyond_accepted": ["ray_end"],
    "nan_is_a_candidate": ["point_nan_radius"],
    "mask_ignored": ["point_mask", "ray_pad"],
}


def particles(name):
    """(white, yolk) of a case in the layout of a handle: batches in ascending key, ids by position in the case's list"""
    case = CASES[name]
    out = []
    for t in ("white", "yolk"):
        rows = [(p, b["key"], i, pos + 1) for pos, b in sorted(enumerate(case["batches"]), key=lambda e: e[1]["key"])
                for i, p in enumerate(b[t])]
        out.append(dict(x=np.array([r[0][0] for r in rows]), y=np.array([r[0][1] for r in rows]), radius=np.array([r[0][2] for r in rows]),
                        key=np.array([r[1] for r in rows], dtype=np.int64), index=np.array([r[2] for r in rows], dtype=np.int64),
                        id=np.array([r[3] for r in rows], dtype=np.int64)))
    return tuple(out)


def expected(name, ids=None):
    """the hits of a case from the hand-written winners: (id, index, score, x, y, radius); `ids` = the ids the batches got
    where they were imported (by default position + 1)"""
    case = CASES[name]
    out = []
    for pair in case["want"]:
        hits = []
        for t, won in zip(("white", "yolk"), pair):
            if won is None:
                hits.append(None)
                continue
            pos, index, score = won
            x, y, r = case["batches"][pos][t][index]
            hits.append((pos + 1 if ids is None else ids[pos], index, score, x, y, r))
        out.append(tuple(hits))
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_case(name):
    case = CASES[name]
    got = pm.probe(case["probes"], particles(name))
    assert got == expected(name)
    assert [None if f is None else f[0] for f in map(pm.first, got)] == case["first"]
    for pair in got:
        for hit in pair:
            assert hit is None or (isinstance(hit[0], int) and isinstance(hit[1], int) and all(isinstance(v, float) for v in hit[2:]))


@pytest.mark.parametrize("wrong", pm.WRONG_RULES)
def test_every_wrong_rule_is_noticed(wrong):
    assert sorted(NOTICED_BY) == sorted(pm.WRONG_RULES)
    for name in NOTICED_BY[wrong]:
        assert pm.probe(CASES[name]["probes"], particles(name), wrong=wrong) != expected(name), (wrong, name)


def test_the_table_covers_what_the_rule_distinguishes():
    names = set(CASES)
    assert {n for n in names if n.startswith("point_")} >= {"point_at_the_reach", "point_reach_zero", "point_reach_inf", "point_tie_in_a_batch",
                                                            "point_coincident_batches", "point_white_and_yolk_equal", "point_nan_position",
                                                            "point_nan_radius", "point_mask"}
    assert {n for n in names if n.startswith("ray_")} >= {"ray_start_inside", "ray_start_on_the_rim", "ray_tangent", "ray_just_missing", "ray_end",
                                                          "ray_disc_behind", "ray_pad", "ray_equal_t"}
    # the exact quantities the comments claim
    c, s = pm.evaluate("ray", [0.0, 0.0, 10.0, 0.0, 0.0], [5.0, 11.0 + E], [1.0 + E, 0.0], [1.0, 1.0])
    assert list(c) == [False, False] and s[1] == (100.0 + 10.0 * E) / 100.0 and s[1] > 1.0
    c, s = pm.evaluate("point", [0.0, 0.0, 5.0], [0.0], [nxt(5.0, UP)], [1.0])
    assert not c[0] and s[0] > 25.0


def test_the_impact_and_the_first_of_a_pair():
    assert pm.impact(X_RAY[1:], 0.4) == (4.0, 0.0) and pm.impact((1.0, 2.0, 3.0, -2.0), 0.5) == (2.0, 0.0)
    a, b = (1, 0, 2.0, 0.0, 0.0, 1.0), (2, 3, 2.0, 1.0, 1.0, 1.0)
    assert pm.first((a, b)) == ("white", a) and pm.first((None, b)) == ("yolk", b) and pm.first((None, None)) is None
    assert pm.first((b, (2, 3, 1.5, 1.0, 1.0, 1.0)))[0] == "yolk" and pm.first((a, None)) == ("white", a)


def test_the_list_as_the_library_takes_it():
    got = pm.canonical([("point", 1.0, 2.0), ("point", 1.0, 2.0, 3.0, "yolk"), ("ray", 0.0, 0.0, 1.0, 1.0), ("ray", 0.0, 0.0, 1.0, 1.0, 0.5, 1)])
    assert got == [("point", 3, [1.0, 2.0, math.inf, 0.0, 0.0]), ("point", 2, [1.0, 2.0, 3.0, 0.0, 0.0]),
                   ("ray", 3, [0.0, 0.0, 1.0, 1.0, 0.0]), ("ray", 1, [0.0, 0.0, 1.0, 1.0, 0.5])]
    good = ("point", 0.0, 0.0)
    for bad, index in (([("ring", 0.0, 0.0)], 0), ([good, ("point", 0.0, 0.0, -1.0)], 1), ([("point", NAN, 0.0)], 0),
                       ([("point", math.inf, 0.0)], 0), ([("point", 0.0, 0.0, -math.inf)], 0), ([good, good, ("ray", 0.0, 0.0, 1.0, 1.0, -0.5)], 2),
                       ([("ray", 0.0, 0.0, 1.0, math.inf)], 0), ([("ray", 0.0, 0.0, 1.0, 1.0, math.inf)], 0), ([("ray", 2.0, 3.0, 2.0, 3.0)], 0),
                       ([("ray", 0.0, 0.0, 0.5e-8, 0.0)], 0), ([("point", 0.0, 0.0, 1.0, "none")], 0), ([("point", 0.0, 0.0, 1.0, 0)], 0),
                       ([("point", 0.0)], 0)):
        with pytest.raises(ValueError, match="probe %d" % index):
            pm.canonical(bad)
    with pytest.raises(ValueError, match="0 .. 64"):
        pm.canonical([good] * 65)
    assert len(pm.canonical([good] * 64)) == 64 and pm.canonical([]) == []
    assert pm.canonical([("ray", 0.0, 0.0, 1e-8, 0.0)])[0][0] == "ray"  # (l2 == eps eps is a ray)


def test_particles_of_numbers_the_runs():
    a = pm.particles_of([0.0] * 6, [0.0] * 6, [1.0] * 6, [4, 4, 2, 2, 2, 9], {4: 1, 2: 5, 9: 7})
    assert list(a["index"]) == [0, 1, 0, 1, 2, 0] and list(a["key"]) == [1, 1, 5, 5, 5, 7] and list(a["id"]) == [4, 4, 2, 2, 2, 9]
    assert pm.particles_of([], [], [], [], {})["index"].size == 0
