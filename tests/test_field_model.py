"""The CPU model of the fields (tests/field_model.py) against a hand table: every expectation below was written by hand from
the rule in include/eggsim.h, cell by cell; none was taken from the model or from the device.  The same table runs on the
device in tests/test_gpu_fields.py.

A case: a grid (x0, y0, cell, nx, ny), a type mask, whether velocities are asked for, and the particles per type as
(x, y, vx, vy).  Its expectation: the non-zero words of each plane as {(w, iy, ix): value} and the three totals.  Cells of
side 8 keep inv = 0.125 and every product exact, so a position on an edge is on it in the arithmetic too.

WRONG rules (field_model.WRONG_RULES): each is a plausible misreading of the rule; at least one case must notice each."""
import math

import numpy as np
import pytest

import field_model as fm

UP, DOWN = math.inf, -math.inf
NAN, INF = math.nan, math.inf
S = 65536.0


def nxt(v, toward):
    return math.nextafter(v, toward)


def at_rest(*spots):
    return [(x, y, 0.0, 0.0) for x, y in spots]


CASES = {
    # a centre on an interior cell edge belongs to the upper cell; one ulp below it to the lower
    "interior_edge": dict(
        grid=(0.0, 0.0, 8.0, 4, 3), types="both", velocity=False,
        spots=(at_rest((16.0, 4.0), (nxt(16.0, DOWN), 4.0)), at_rest((4.0, 8.0), (4.0, nxt(8.0, DOWN)))),
        count={(0, 0, 2): 1, (0, 0, 1): 1, (1, 1, 0): 1, (1, 0, 0): 1}, inside=(2, 2), outside=(0, 0), dropped=(0, 0)),
    # the lower grid edge is inside, the upper one outside: x in [10, 42), y in [20, 44)
    "grid_edges": dict(
        grid=(10.0, 20.0, 8.0, 4, 3), types="both", velocity=False,
        spots=(at_rest((10.0, 20.0), (42.0, 30.0), (nxt(42.0, DOWN), 30.0), (nxt(10.0, DOWN), 30.0)),
               at_rest((12.0, 44.0), (12.0, nxt(44.0, DOWN)), (12.0, 20.0))),
        count={(0, 0, 0): 1, (0, 1, 3): 1, (1, 2, 0): 1, (1, 0, 0): 1}, inside=(2, 2), outside=(2, 1), dropped=(0, 0)),
    # -0.0 >= 0.0 holds: cell 0
    "negative_zero": dict(
        grid=(0.0, 0.0, 8.0, 2, 2), types="both", velocity=False,
        spots=(at_rest((-0.0, 1.0), (1.0, -0.0)), at_rest((-1e-300, 1.0), (1.0, 1.0))),
        count={(0, 0, 0): 2, (1, 0, 0): 1}, inside=(2, 1), outside=(0, 1), dropped=(0, 0)),
    # a NaN or an infinity in a position: every comparison fails, the particle is outside
    "nan_and_infinity": dict(
        grid=(0.0, 0.0, 8.0, 4, 4), types="both", velocity=False,
        spots=(at_rest((NAN, 1.0), (1.0, NAN), (INF, 1.0), (-INF, 1.0), (9.0, 17.0)), at_rest((1.0, INF), (1.0, 1.0))),
        count={(0, 2, 1): 1, (1, 0, 0): 1}, inside=(1, 1), outside=(4, 1), dropped=(0, 0)),
    # a grid of one cell, [-4, 4) x [-4, 4)
    "one_by_one": dict(
        grid=(-4.0, -4.0, 8.0, 1, 1), types="both", velocity=False,
        spots=(at_rest((0.0, 0.0), (3.9, -3.9), (4.0, 0.0)), at_rest((-4.0, -4.0), (0.0, 4.0))),
        count={(0, 0, 0): 2, (1, 0, 0): 1}, inside=(2, 1), outside=(1, 1), dropped=(0, 0)),
    # scaled velocities on a tie go to the even integer: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4, -0.5 -> 0, -1.5 -> -2, -2.5 -> -2
    "velocity_ties": dict(
        grid=(0.0, 0.0, 8.0, 2, 2), types="both", velocity=True,
        spots=([(1.0, 1.0, 0.5 / S, 1.5 / S), (1.0, 1.0, 2.5 / S, 1.0), (9.0, 1.0, 3.5 / S, -0.5 / S)],
               [(1.0, 9.0, -1.5 / S, -2.5 / S), (9.0, 9.0, 1.0, -1.0)]),
        count={(0, 0, 0): 2, (0, 0, 1): 1, (1, 1, 0): 1, (1, 1, 1): 1},
        svx={(0, 0, 0): 2, (0, 0, 1): 4, (1, 1, 0): -2, (1, 1, 1): 65536},
        svy={(0, 0, 0): 65538, (1, 1, 0): -2, (1, 1, 1): -65536}, inside=(3, 2), outside=(0, 0), dropped=(0, 0)),
    # a scaled velocity that reaches 2^53 (vx = 2^37), or is not finite, drops the particle: not counted, not summed; one ulp
    # below the limit is counted with 2^53 - 1; a particle outside is outside whatever its velocity
    "velocity_limit": dict(
        grid=(0.0, 0.0, 8.0, 2, 2), types="both", velocity=True,
        spots=([(1.0, 1.0, 2.0 ** 37, 0.0), (1.0, 1.0, nxt(2.0 ** 37, DOWN), 1.0), (9.0, 1.0, 0.0, NAN), (9.0, 1.0, INF, 0.0),
                (100.0, 1.0, NAN, NAN)], [(1.0, 1.0, 0.0, -2.0 ** 37), (1.0, 1.0, -1.0, 0.0)]),
        count={(0, 0, 0): 1, (1, 0, 0): 1}, svx={(0, 0, 0): 2 ** 53 - 1, (1, 0, 0): -65536}, svy={(0, 0, 0): 65536},
        inside=(1, 1), outside=(1, 0), dropped=(3, 1)),
    # the same particles without velocities: nothing is read, nothing is dropped
    "velocity_limit_count_only": dict(
        grid=(0.0, 0.0, 8.0, 2, 2), types="both", velocity=False,
        spots=([(1.0, 1.0, 2.0 ** 37, 0.0), (1.0, 1.0, nxt(2.0 ** 37, DOWN), 1.0), (9.0, 1.0, 0.0, NAN), (9.0, 1.0, INF, 0.0),
                (100.0, 1.0, NAN, NAN)], [(1.0, 1.0, 0.0, -2.0 ** 37), (1.0, 1.0, -1.0, 0.0)]),
        count={(0, 0, 0): 2, (0, 0, 1): 2, (1, 0, 0): 2}, inside=(4, 2), outside=(1, 0), dropped=(0, 0)),
    # a mask leaves the other type's planes and totals zero
    "mask_white": dict(
        grid=(0.0, 0.0, 8.0, 2, 2), types="white", velocity=False,
        spots=(at_rest((1.0, 1.0), (9.0, 9.0)), at_rest((9.0, 1.0), (1.0, 9.0), (50.0, 50.0))),
        count={(0, 0, 0): 1, (0, 1, 1): 1}, inside=(2, 0), outside=(0, 0), dropped=(0, 0)),
    "mask_yolk": dict(
        grid=(0.0, 0.0, 8.0, 2, 2), types="yolk", velocity=True,
        spots=([(1.0, 1.0, 1.0, 1.0), (9.0, 9.0, 2.0 ** 40, 0.0)], [(9.0, 1.0, 0.25, -0.5), (1.0, 9.0, 0.0, 0.0), (50.0, 50.0, 1.0, 1.0)]),
        count={(1, 0, 1): 1, (1, 1, 0): 1}, svx={(1, 0, 1): 16384}, svy={(1, 0, 1): -32768}, inside=(0, 2), outside=(0, 1), dropped=(0, 0)),
    # (x - x0) * inv against (x - x0) / cell: with cell = 0.1 the inverse is exactly 10.0 and 4.3 * 10.0 rounds to 43.0, while
    # 4.3 / 0.1 rounds to 42.99999999999999 (found by a search over multiples of the cell; test_the_division_pair re-derives it)
    "multiplication_not_division": dict(
        grid=(0.0, 0.0, 0.1, 64, 1), types="both", velocity=False,
        spots=(at_rest((4.3, 0.05), (0.05, 0.05)), at_rest((0.05, 0.05), (0.05, 0.05))),
        count={(0, 0, 43): 1, (0, 0, 0): 1, (1, 0, 0): 2}, inside=(2, 2), outside=(0, 0), dropped=(0, 0)),
}


def arrays(name):
    """per-type arrays (xs, ys, vxs, vys) of a case"""
    spots = CASES[name]["spots"]
    return tuple([np.array([s[k] for s in spots[w]], dtype=np.float64) for w in (0, 1)] for k in range(4))


def expected(name):
    """the hand-written expectation as field_model.field returns it"""
    case = CASES[name]
    _, _, _, nx, ny = case["grid"]
    planes = []
    for key, dtype in (("count", np.int32), ("svx", np.int64), ("svy", np.int64)):
        if key != "count" and not case["velocity"]:
            planes.append(None)
            continue
        plane = np.zeros((2, ny, nx), dtype=dtype)
        for at, value in case.get(key, {}).items():
            plane[at] = value
        planes.append(plane)
    return tuple(planes) + (case["inside"], case["outside"], case["dropped"])


def same(a, b):
    return all((p is None and q is None) or (p is not None and q is not None and p.dtype == q.dtype and np.array_equal(p, q))
               for p, q in zip(a[:3], b[:3])) and tuple(a[3:]) == tuple(b[3:])


def run(name, wrong=None):
    case = CASES[name]
    xs, ys, vxs, vys = arrays(name)
    return fm.field(case["grid"], xs, ys, vxs, vys, case["types"], case["velocity"], wrong)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_model_gives_the_hand_written_answer(name):
    got = run(name)
    assert same(got, expected(name)), (name, got)
    case = CASES[name]
    for w in (0, 1):  # the invariant on the totals
        n = len(case["spots"][w]) if fm.MASKS[case["types"]] >> w & 1 else 0
        assert got[3][w] + got[4][w] + got[5][w] == n and int(got[0][w].sum()) == got[3][w], (name, w)


@pytest.mark.parametrize("wrong", fm.WRONG_RULES)
def test_every_wrong_rule_is_noticed_by_some_case(wrong):
    noticed = [name for name in sorted(CASES) if not same(run(name, wrong), expected(name))]
    print(wrong, "noticed by", noticed)
    assert noticed, wrong


def test_the_table_covers_what_it_promises():
    assert set(fm.WRONG_RULES) == {"rounding", "closed_upper_edge", "swapped_xy", "column_major", "ignored_mask", "drop_counts", "division"}
    assert any(c["grid"][3:] == (1, 1) for c in CASES.values())
    assert any(math.copysign(1.0, s[0]) < 0 and s[0] == 0.0 for c in CASES.values() for t in c["spots"] for s in t)
    assert any(math.isnan(s[0]) for c in CASES.values() for t in c["spots"] for s in t)
    assert any(math.isinf(s[0]) for c in CASES.values() for t in c["spots"] for s in t)
    assert {c["types"] for c in CASES.values()} == {"both", "white", "yolk"}
    assert all(len(t) >= 2 for c in CASES.values() for t in c["spots"])  # (a batch of the device tests holds two particles at least)


def test_the_division_pair():
    """the (x, x0, cell) of the table's last case, re-derived: one multiplication by the inverse and one division land in
    different cells, and a search over multiples of the cell finds such positions"""
    x, x0, cell = np.float64(4.3), np.float64(0.0), np.float64(0.1)
    inv = np.float64(1.0) / cell
    assert inv == 10.0 and (x - x0) * inv == 43.0 and (x - x0) / cell == 42.99999999999999
    found = [k for k in range(1, 200) if int((cell * k - x0) * inv) != int((cell * k - x0) / cell)]
    assert 43 in found, found


def test_velocity_of_a_cell():
    count, svx, svy = expected("velocity_ties")[:3]
    v = fm.velocity(count, svx, svy)
    assert v.shape == (2, 2, 2, 2) and v.dtype == np.float64
    assert tuple(v[0, 0, 0]) == ((2.0 / S) / 2.0, (65538.0 / S) / 2.0) and tuple(v[1, 1, 1]) == (1.0, -1.0)
    assert tuple(v[0, 0, 1]) == (4.0 / S, 0.0) and np.isnan(v[0, 1]).all() and np.isnan(v[1, 0]).all()


def test_grids_the_library_refuses():
    for grid in ((0.0, 0.0, 1.0, 0, 4), (0.0, 0.0, 1.0, 4, -1), (0.0, 0.0, 1.0, 1024, 1025), (0.0, 0.0, 0.0, 4, 4), (0.0, 0.0, -1.0, 4, 4),
                 (0.0, 0.0, NAN, 4, 4), (0.0, 0.0, INF, 4, 4), (0.0, 0.0, 5e-324, 4, 4), (NAN, 0.0, 1.0, 4, 4), (0.0, -INF, 1.0, 4, 4)):
        with pytest.raises(ValueError):
            fm.check_grid(*grid)
    fm.check_grid(0.0, 0.0, 1.0, 1024, 1024)
