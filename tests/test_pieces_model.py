"""The model of the pieces (tests/pieces_model.py) against an independent brute-force union-find written here, the HAND TABLE
of tiny atoms with hand-written records (tests/test_gpu_pieces.py runs the same table on the device), and the wrong rules
the table must notice: each of them changes at least one record of the table."""
import math

import numpy as np
import pytest

import pieces_model as pm

S = 65536  # 2^16: a coordinate c that is a multiple of 2^-16 adds c * S to a sum
NAN = float("nan")
P37 = 2.0 ** 37  # * 2^16 = 2^53: the first coordinate that is dropped
ONE_YOLK = [(500.0, 500.0, 4.0)]  # (a batch is imported with both types; one particle is one piece, a single, its own body)
Y1 = (1, 1, 1, 0, 1, 0, 500 * S, 500 * S)
FAR = math.nextafter(16.0, math.inf)


def _line(n, step, r, x0=0.0, y=0.0, order=None):
    """n particles on a line, `step` apart; order[p] = the index of the particle at position p (default p)"""
    spots = [None] * n
    for p in range(n):
        spots[p if order is None else order[p]] = (x0 + step * p, y, r)
    return spots


FAR_END = [299 - p for p in range(300)]  # index 0 sits at the far end of the line
SNAKE = [p // 2 if p % 2 == 0 else 299 - p // 2 for p in range(300)]  # 0, 299, 1, 298, ..: every hop goes against the index order
CHAIN_SX = 7 * S * sum(range(300))

# name -> batches (key, white, yolk; a particle is (x, y, radius)), reach (white, yolk), records per batch ((white), (yolk)),
# each (n, pieces, largest, first, singles, dropped, sx, sy) written by hand
CASES = {
    "one particle": dict(batches=[dict(key=1, white=[(10.0, 20.0, 4.0)], yolk=ONE_YOLK)], reach=(1.0, 1.0),
                         records=[((1, 1, 1, 0, 1, 0, 10 * S, 20 * S), Y1)]),
    "two linked": dict(batches=[dict(key=1, white=[(0.0, 0.0, 4.0), (6.0, 0.0, 4.0)], yolk=ONE_YOLK)], reach=(1.0, 1.0),
                       records=[((2, 1, 2, 0, 0, 0, 6 * S, 0), Y1)]),
    # radii 4 and 4: L = reach * 8.  Exactly at the edge is linked (<=): 8 px apart with reach 1, 16 px apart with reach 2
    "edge, reach 1": dict(batches=[dict(key=1, white=[(0.0, 0.0, 4.0), (8.0, 0.0, 4.0)], yolk=ONE_YOLK)], reach=(1.0, 1.0),
                          records=[((2, 1, 2, 0, 0, 0, 8 * S, 0), Y1)]),
    "edge, 16 px": dict(batches=[dict(key=1, white=[(0.0, 0.0, 4.0), (16.0, 0.0, 4.0)], yolk=ONE_YOLK)], reach=(2.0, 1.0),
                        records=[((2, 1, 2, 0, 0, 0, 16 * S, 0), Y1)]),
    # the same pair one ulp farther: 16 + 2^-48, squared above 256; llrint((16 + 2^-48) * 2^16) = 2^20
    "one ulp beyond the edge": dict(batches=[dict(key=1, white=[(0.0, 0.0, 4.0), (FAR, 0.0, 4.0)], yolk=ONE_YOLK)], reach=(2.0, 1.0),
                                    records=[((2, 2, 1, 0, 2, 0, 0, 0), Y1)]),
    "chain of 300, index 0 at the far end": dict(batches=[dict(key=1, white=_line(300, 7.0, 4.0, order=FAR_END), yolk=ONE_YOLK)],
                                                 reach=(1.0, 1.0), records=[((300, 1, 300, 0, 0, 0, CHAIN_SX, 0), Y1)]),
    "chain of 300 in snake order": dict(batches=[dict(key=1, white=_line(300, 7.0, 4.0, order=SNAKE), yolk=ONE_YOLK)],
                                        reach=(1.0, 1.0), records=[((300, 1, 300, 0, 0, 0, CHAIN_SX, 0), Y1)]),
    # eight particles on the rim of a square, 6 apart: neighbours are linked, (6, 0) - (12, 6) at 8.49 are not
    "ring": dict(batches=[dict(key=1, white=[(0.0, 0.0, 4.0), (6.0, 0.0, 4.0), (12.0, 0.0, 4.0), (12.0, 6.0, 4.0), (12.0, 12.0, 4.0),
                                             (6.0, 12.0, 4.0), (0.0, 12.0, 4.0), (0.0, 6.0, 4.0)], yolk=ONE_YOLK)], reach=(1.0, 1.0),
                 records=[((8, 1, 8, 0, 0, 0, 48 * S, 48 * S), Y1)]),
    # indices 1, 3, 5 at 0, 6, 12 and indices 0, 2, 4 at 100, 106, 112: equal sizes, the body is the piece of label 0
    "two clusters of equal size": dict(batches=[dict(key=1, white=[(100.0, 0.0, 4.0), (0.0, 0.0, 4.0), (106.0, 0.0, 4.0), (6.0, 0.0, 4.0),
                                                                   (112.0, 0.0, 4.0), (12.0, 0.0, 4.0)], yolk=ONE_YOLK)], reach=(1.0, 1.0),
                                       records=[((6, 2, 3, 0, 0, 0, 318 * S, 0), Y1)]),
    # indices 0, 1, 2 stray, the body is 3 .. 7 at x = 0, 6, .., 24 and y = 1.5
    "a body with three strays": dict(batches=[dict(key=1, white=[(-100.0, 0.0, 4.0), (200.0, 0.0, 4.0), (0.0, 300.0, 4.0)] +
                                                   _line(5, 6.0, 4.0, y=1.5), yolk=ONE_YOLK)], reach=(1.0, 1.0),
                                     records=[((8, 4, 5, 3, 3, 0, 60 * S, 5 * 3 * S // 2), Y1)]),
    "coincident particles": dict(batches=[dict(key=1, white=[(3.0, 3.0, 4.0)] * 3 + [(50.0, 3.0, 4.0)], yolk=ONE_YOLK)], reach=(1.0, 1.0),
                                 records=[((4, 2, 3, 0, 1, 0, 9 * S, 9 * S), Y1)]),
    # small ones (radius 1) at 0 and 10 are not linked (L = 2), the big one (radius 6) at 5 links both (L = 7)
    "unequal radii, a bridge": dict(batches=[dict(key=1, white=[(0.0, 0.0, 1.0), (10.0, 0.0, 1.0), (5.0, 0.0, 6.0)], yolk=ONE_YOLK)],
                                    reach=(1.0, 1.0), records=[((3, 1, 3, 0, 0, 0, 15 * S, 0), Y1)]),
    # the same without the bridge in reach: the big one has radius 2.5, L = 3.5 < 5
    "unequal radii, no bridge": dict(batches=[dict(key=1, white=[(0.0, 0.0, 1.0), (10.0, 0.0, 1.0), (5.0, 0.0, 2.5)], yolk=ONE_YOLK)],
                                     reach=(1.0, 1.0), records=[((3, 3, 1, 0, 3, 0, 0, 0), Y1)]),
    "a NaN position": dict(batches=[dict(key=1, white=[(0.0, 0.0, 4.0), (NAN, 0.0, 4.0), (6.0, 2.0, 4.0)], yolk=[(NAN, NAN, 4.0)])],
                           reach=(1.0, 1.0), records=[((3, 2, 2, 0, 1, 0, 6 * S, 2 * S), (1, 1, 1, 0, 1, 1, 0, 0))]),
    # 2^37 * 2^16 = 2^53 is not below 2^53: both body particles are dropped, the stray at 0 is no part of the body
    "a coordinate at 2^37 px": dict(batches=[dict(key=1, white=[(P37, 0.0, 4.0), (P37 + 6.0, 1.0, 4.0), (0.0, 0.0, 4.0)], yolk=ONE_YOLK)],
                                    reach=(1.0, 1.0), records=[((3, 2, 2, 0, 1, 2, 0, 0), Y1)]),
    "white linked and yolk broken": dict(batches=[dict(key=1, white=_line(4, 6.0, 4.0), yolk=_line(4, 6.0, 2.0, y=50.0))], reach=(1.0, 1.0),
                                         records=[((4, 1, 4, 0, 0, 0, 36 * S, 0), (4, 4, 1, 0, 4, 0, 0, 50 * S))]),
    # 10 apart with radius 4: L = 8 for the white, 12 for the yolk
    "different reach per type": dict(batches=[dict(key=1, white=_line(3, 10.0, 4.0), yolk=_line(3, 10.0, 4.0, y=50.0))], reach=(1.0, 1.5),
                                     records=[((3, 3, 1, 0, 3, 0, 0, 0), (3, 1, 3, 0, 0, 0, 30 * S, 150 * S))]),
    # batch 1 at 0, 12, 24 and batch 2 at 6, 18, 30: 6 apart across the batches, 12 inside a batch
    "two batches that interleave": dict(batches=[dict(key=1, white=_line(3, 12.0, 4.0), yolk=ONE_YOLK),
                                                 dict(key=2, white=_line(3, 12.0, 4.0, x0=6.0), yolk=ONE_YOLK)], reach=(1.0, 1.0),
                                        records=[((3, 3, 1, 0, 3, 0, 0, 0), Y1), ((3, 3, 1, 0, 3, 0, 6 * S, 0), Y1)]),
}


def particles_of(batches):
    """the model's view of a table case: the arrays a handle that imported `batches` in order would download (ids 1, 2, ..)"""
    out = []
    for name in ("white", "yolk"):
        rows = [(x, y, r, k + 1) for k, b in enumerate(batches) for x, y, r in b[name]]
        cols = np.array(rows, dtype=np.float64).reshape(len(rows), 4)
        out.append(dict(x=cols[:, 0].copy(), y=cols[:, 1].copy(), radius=cols[:, 2].copy(), batch_id=cols[:, 3].copy()))
    return tuple(out)


def _table(name, rule=None):
    case = CASES[name]
    ids = list(range(1, len(case["batches"]) + 1))
    return pm.pieces(particles_of(case["batches"]), ids, case["reach"], 3, rule)[0]


def _union_find(spots, reach):
    """connected components by brute force over all pairs, Python floats, nothing shared with the model: the labels"""
    n = len(spots)
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for i in range(n):
        xi, yi, ri = spots[i]
        for j in range(i + 1, n):
            xj, yj, rj = spots[j]
            dx, dy = xi - xj, yi - yj
            L = reach * (ri + rj)
            if dx * dx + dy * dy <= L * L:
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    return [find(i) for i in range(n)]


def _record_by_hand(spots, labels):
    n = len(spots)
    if n == 0:
        return pm.ZERO
    size = {}
    for lab in labels:
        size[lab] = size.get(lab, 0) + 1
    largest = max(size.values())
    first = min(lab for lab, s in size.items() if s == largest)
    dropped = sx = sy = 0
    for (x, y, _), lab in zip(spots, labels):
        if lab != first:
            continue
        fx, fy = x * 65536.0, y * 65536.0
        if abs(fx) < 2.0 ** 53 and abs(fy) < 2.0 ** 53:
            sx += round(fx)
            sy += round(fy)
        else:
            dropped += 1
    return (n, len(size), largest, first, sum(1 for s in size.values() if s == 1), dropped, sx, sy)


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_gives_the_hand_written_records(name):
    assert _table(name) == CASES[name]["records"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_equals_brute_force_union_find(name):
    case = CASES[name]
    ids = list(range(1, len(case["batches"]) + 1))
    records, labels = pm.pieces(particles_of(case["batches"]), ids, case["reach"])
    at = [0, 0]
    for k, b in enumerate(case["batches"]):
        for w, t in enumerate(("white", "yolk")):
            want = _union_find(b[t], case["reach"][w])
            assert list(labels[w][at[w]:at[w] + len(want)]) == want, (name, k, t)
            assert records[k][w] == _record_by_hand(b[t], want), (name, k, t)
            at[w] += len(want)


def test_model_equals_union_find_on_random_atoms():
    rng = np.random.default_rng(30)
    for trial in range(20):
        n = int(rng.integers(1, 90))
        spots = [(float(x), float(y), float(r)) for x, y, r in zip(rng.uniform(0, 60, n), rng.uniform(0, 60, n), rng.choice([1.0, 2.0, 3.5], n))]
        reach = float(rng.choice([0.75, 1.0, 1.5]))
        want = _union_find(spots, reach)
        cols = np.array(spots)
        got = pm.labels_of(cols[:, 0], cols[:, 1], cols[:, 2], reach)
        assert list(got) == want, trial
        assert pm.record_of(cols[:, 0], cols[:, 1], got) == _record_by_hand(spots, want), trial
    assert len(set(want)) > 1  # (the last trial is in pieces: the draw is not one blob throughout)


def test_masks_ids_and_labels_of_the_model():
    case = CASES["two batches that interleave"]
    parts = particles_of(case["batches"])
    both, labels = pm.pieces(parts, [1, 2], case["reach"])
    assert [list(lab) for lab in labels] == [[0, 1, 2, 0, 1, 2], [0, 0]]
    rec, lab = pm.pieces(parts, [2, 2, 1], case["reach"], 1)
    assert rec == [(both[1][0], pm.ZERO), (both[1][0], pm.ZERO), (both[0][0], pm.ZERO)] and list(lab[1]) == [-1, -1]
    rec, lab = pm.pieces(parts, [2], case["reach"], 2)
    assert rec == [(pm.ZERO, both[1][1])] and list(lab[0]) == [-1] * 6 and list(lab[1]) == [-1, 0]
    rec, lab = pm.pieces(parts, [], case["reach"])
    assert rec == [] and list(lab[0]) == [-1] * 6 and list(lab[1]) == [-1, -1]
    assert pm.summary(pm.ZERO) is None and pm.summary((3, 2, 2, 0, 1, 2, 0, 0)) == (3, 2, 2, 0, 1, 2, None, None)
    assert pm.summary((2, 1, 2, 0, 0, 0, 6 * S, -3 * S)) == (2, 1, 2, 0, 0, 0, 3.0, -1.5)


@pytest.mark.parametrize("rule", pm.WRONG_RULES)
def test_the_table_notices_a_wrong_rule(rule):
    changed = [name for name in sorted(CASES) if _table(name, rule) != CASES[name]["records"]]
    print(rule, "changes", changed)
    assert changed, rule
    expected = {"strict": "edge, 16 px", "max_radius": "two linked", "cross_batch": "two batches that interleave",
                "tie_high": "two clusters of equal size", "one_sweep": "chain of 300 in snake order"}
    assert expected[rule] in changed, (rule, changed)
