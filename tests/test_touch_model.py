"""The hand table of the touches (tests/touch_model.py; include/eggsim_touch.h): tiny scenes with the
records written out by hand.  The GPU tests (test_gpu_touches.py) run the same table on the device.  No GPU here."""
import math

import numpy as np
import pytest

import touch_model as tm

Q = 65536  # q(1.0)
BIG = 2.0 ** 37  # BIG * 65536 reaches 2^53: a particle there is dropped from the sums


def _b(white, yolk=()):
    return dict(white=list(white), yolk=list(yolk))


ROW = [_b([(0.0, 0.0, 1.0)]), _b([(2.0, 0.0, 1.0)]), _b([(4.0, 0.0, 1.0)])]
ROW_12 = (0, 2, 1, 1, 0, 2 * Q, 0)   # batch 1 with batch 2, either way round, behind (entry, type)
ROW_23 = (0, 3, 1, 1, 0, 6 * Q, 0)

# name -> batches (batch k has the id k + 1), the ids asked for, the reach per type, the mask, the records by hand
CASES = {
    # radii 4 and 4, 8 apart on x, reach 1: d2 = 64 = L * L exactly
    "on_the_boundary": dict(batches=[_b([(0.0, 0.0, 4.0)]), _b([(8.0, 0.0, 4.0)])], ids=[1, 2], reach=(1.0, 1.0), mask=3,
                            want=[(0, 0, 2, 1, 1, 0, 8 * Q, 0), (1, 0, 1, 1, 1, 0, 8 * Q, 0)]),
    "one_ulp_beyond": dict(batches=[_b([(0.0, 0.0, 4.0)]), _b([(math.nextafter(8.0, 9.0), 0.0, 4.0)])], ids=[1, 2], reach=(1.0, 1.0), mask=3,
                           want=[]),
    # 3-4-5: d2 = 25 = (2 + 3)^2
    "three_four_five": dict(batches=[_b([(0.0, 0.0, 2.0)]), _b([(3.0, 4.0, 3.0)])], ids=[1, 2], reach=(1.0, 1.0), mask=3,
                            want=[(0, 0, 2, 1, 1, 0, 3 * Q, 4 * Q), (1, 0, 1, 1, 1, 0, 3 * Q, 4 * Q)]),
    # radii 1 and 3, 4.3 apart: 18.49 <= (1.1 * 4)^2 = 19.36, and 18.49 > 4^2
    "unequal_radii_reach_1_1": dict(batches=[_b([(0.0, 0.0, 1.0)]), _b([(4.3, 0.0, 3.0)])], ids=[1, 2], reach=(1.1, 1.1), mask=3,
                                    want=[(0, 0, 2, 1, 1, 0, 281805, 0), (1, 0, 1, 1, 1, 0, 281805, 0)]),
    "unequal_radii_reach_1": dict(batches=[_b([(0.0, 0.0, 1.0)]), _b([(4.3, 0.0, 3.0)])], ids=[1, 2], reach=(1.0, 1.0), mask=3, want=[]),
    "nan_centre": dict(batches=[_b([(0.0, 0.0, 1.0), (float("nan"), 0.0, 1.0)]), _b([(1.0, 0.0, 1.0)])], ids=[1, 2], reach=(1.0, 1.0), mask=3,
                       want=[(0, 0, 2, 1, 1, 0, Q, 0), (1, 0, 1, 1, 1, 0, Q, 0)]),
    # the pair far out touches and is dropped from the sums; the pair at the origin carries them
    "beyond_the_limit": dict(batches=[_b([(BIG, 0.0, 1.0), (0.0, 0.0, 1.0)]), _b([(BIG + 1.0, 0.0, 1.0), (1.0, 0.0, 1.0)])], ids=[1, 2],
                             reach=(1.0, 1.0), mask=3, want=[(0, 0, 2, 2, 2, 1, Q, 0), (1, 0, 1, 2, 2, 1, Q, 0)]),
    "every_pair_dropped": dict(batches=[_b([(BIG, 0.0, 1.0)]), _b([(BIG + 1.0, 0.0, 1.0)])], ids=[1], reach=(1.0, 1.0), mask=3,
                               want=[(0, 0, 2, 1, 1, 1, 0, 0)]),
    # three in a row: the middle one touches both, the ends do not touch each other
    "three_in_a_row": dict(batches=ROW, ids=[1, 2, 3], reach=(1.0, 1.0), mask=3,
                           want=[(0,) + ROW_12, (1, 0, 1) + ROW_12[2:], (1,) + ROW_23, (2, 0, 2) + ROW_23[2:]]),
    "repeated_and_reversed": dict(batches=ROW, ids=[3, 2, 2, 1], reach=(1.0, 1.0), mask=3,
                                  want=[(0, 0, 2) + ROW_23[2:], (1, 0, 1) + ROW_12[2:], (1,) + ROW_23, (2, 0, 1) + ROW_12[2:], (2,) + ROW_23,
                                        (3,) + ROW_12]),
    # two batches on the same two spots: 4 pairs over 2 particles; sx = 0 + Q + Q + 2 Q
    "coincident": dict(batches=[_b([(0.0, 0.0, 1.0), (1.0, 0.0, 1.0)]), _b([(0.0, 0.0, 1.0), (1.0, 0.0, 1.0)])], ids=[1, 2], reach=(1.0, 1.0),
                       mask=3, want=[(0, 0, 2, 4, 2, 0, 4 * Q, 0), (1, 0, 1, 4, 2, 0, 4 * Q, 0)]),
    # the whites are apart, the yolks touch; the white of 1 lies on the yolk of 2, which is no touch
    "only_in_yolk": dict(batches=[_b([(0.0, 0.0, 1.0)], [(0.0, 0.0, 1.0)]), _b([(10.0, 0.0, 1.0)], [(1.5, 0.0, 1.0)])], ids=[1, 2],
                         reach=(1.0, 1.0), mask=3, want=[(0, 1, 2, 1, 1, 0, 98304, 0), (1, 1, 1, 1, 1, 0, 98304, 0)]),
    "only_in_yolk_white_mask": dict(batches=[_b([(0.0, 0.0, 1.0)], [(0.0, 0.0, 1.0)]), _b([(10.0, 0.0, 1.0)], [(1.5, 0.0, 1.0)])], ids=[1, 2],
                                    reach=(1.0, 1.0), mask=1, want=[]),
    # a reach per type: the whites touch at 3, the yolks at 0.5 do not
    "reach_per_type": dict(batches=[_b([(0.0, 0.0, 1.0)], [(0.0, 0.0, 1.0)]), _b([(5.0, 0.0, 1.0)], [(1.5, 0.0, 1.0)])], ids=[2], reach=(3.0, 0.5),
                           mask=3, want=[(0, 0, 1, 1, 1, 0, 5 * Q, 0)]),
}


def particles_of(batches):
    """(white, yolk) dicts of x, y, radius, batch_id as a handle would download them: batch k has the id k + 1"""
    out = []
    for kind in ("white", "yolk"):
        rows = [(x, y, r, k + 1) for k, b in enumerate(batches) for x, y, r in b[kind]]
        arr = np.array(rows, dtype=np.float64).reshape(-1, 4)
        out.append(dict(x=arr[:, 0], y=arr[:, 1], radius=arr[:, 2], batch_id=arr[:, 3]))
    return tuple(out)


def _answer(case, rule=None):
    return tm.touches(particles_of(case["batches"]), case["ids"], case["reach"], case["mask"], rule)


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_table(name):
    assert _answer(CASES[name]) == CASES[name]["want"]


@pytest.mark.parametrize("rule", tm.WRONG_RULES)
def test_every_wrong_rule_is_noticed(rule):
    noticed = [name for name in sorted(CASES) if _answer(CASES[name], rule) != CASES[name]["want"]]
    print(rule, noticed)
    assert noticed


def test_the_rules_the_issue_names_are_all_there():
    assert set(tm.WRONG_RULES) >= {"strict", "max_radius", "same_batch", "cross_type", "one_sided_sum", "pairs_for_particles"}
    # each is noticed where it should be
    assert _answer(CASES["on_the_boundary"], "strict") == [] and _answer(CASES["three_four_five"], "max_radius") == []
    assert (0, 0, 1, 1, 1, 0, 0, 0) in _answer(CASES["on_the_boundary"], "same_batch")
    assert (0, 0, 2, 1, 1, 0, 98304, 0) in _answer(CASES["only_in_yolk"], "cross_type")
    assert _answer(CASES["three_four_five"], "one_sided_sum")[0] == (0, 0, 2, 1, 1, 0, 0, 0)
    assert _answer(CASES["coincident"], "pairs_for_particles")[0] == (0, 0, 2, 4, 4, 0, 4 * Q, 0)


def random_scene(seed, n_batches=12, most=40, spread=60.0):
    """batches of mixed sizes and radii around a few centres, so that some touch and some do not"""
    rng = np.random.default_rng(seed)
    batches = []
    for _ in range(n_batches):
        cx, cy = rng.uniform(0.0, spread, 2)
        parts = []
        for _kind in range(2):
            n = int(rng.integers(1, most + 1))
            parts.append([(float(cx + rng.normal(0.0, 4.0)), float(cy + rng.normal(0.0, 4.0)), float(rng.choice([0.5, 1.0, 2.5]))) for _ in range(n)])
        batches.append(_b(parts[0], parts[1]))
    return batches


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_a_to_b_and_b_to_a_agree(seed):
    """symmetry: pairs, sx and sy (and dropped) of a -> b equal those of b -> a; particles need not"""
    batches = random_scene(seed)
    ids = list(range(1, len(batches) + 1))
    recs = tm.touches(particles_of(batches), ids, (1.1, 1.0))
    assert recs and recs == sorted(recs, key=lambda r: r[:3])
    by = {(ids[r[0]], r[1], r[2]): r for r in recs}
    for (a, w, b), r in by.items():
        back = by[(b, w, a)]
        assert (r[3], r[5], r[6], r[7]) == (back[3], back[5], back[6], back[7]), (a, w, b)
        assert 1 <= r[4] <= r[3] and a != b
    assert any(by[(a, w, b)][4] != by[(b, w, a)][4] for (a, w, b) in by)  # (particles is one-sided)


def test_handed_in_discs_and_keys():
    """records_of with handed-in discs: a key leaves that batch out, -1 leaves none out; the contact point by two divisions"""
    parts = tm.labelled(particles_of(ROW))
    disc = (np.array([2.0]), np.array([0.0]), np.array([1.0]))
    assert tm.records_of([(2, 0) + disc], parts, (1.0, 1.0)) == [(0, 0, 1, 1, 1, 0, 2 * Q, 0), (0,) + ROW_23]
    assert [r[2] for r in tm.records_of([(-1, 0) + disc], parts, (1.0, 1.0))] == [1, 2, 3]
    assert tm.records_of([(-1, 1) + disc], parts, (1.0, 1.0)) == []  # (no yolk in the scene)
    assert tm.contact((0,) + ROW_23) == (3.0, 0.0) and tm.contact(CASES["every_pair_dropped"]["want"][0]) is None
    assert tm.contact(CASES["coincident"]["want"][0]) == (0.5, 0.0)
