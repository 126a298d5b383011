"""The rule of the sensors (include/eggsim.h, "sensors"; tests/sensor_model.py) on a hand table: per case a list of sensors,
a few positions per type, and -- written down by hand -- which positions every sensor holds and how many (particle, sensor)
incidences are dropped.  The expected integers follow from that by Python's own round(), which rounds ties to even, not by
the model.  Every wrong rule of sensor_model.WRONG_RULES is told from the right one by at least one case.
tests/test_gpu_sensors.py runs the same table on the device.  No GPU."""
import math

import numpy as np
import pytest

import sensor_model as sm

UP, DOWN = math.inf, -math.inf


def nxt(v, towards):
    return float(np.nextafter(v, towards))


NAN, FAR = float("nan"), 2.0 ** 40
Q = 2.0 ** -16  # one step of the position grid

# name: sensors, spots = (white positions, yolk positions), inside = per sensor (white spot indices, yolk spot indices) that
# COUNT, dropped = [white, yolk]
CASES = {
    # d2 == R R is inside, the next position out is not; the next one in is
    "disc_edge": dict(
        sensors=[("disc", 100.0, 50.0, 5.0)],
        spots=([(105.0, 50.0), (nxt(105.0, UP), 50.0), (nxt(105.0, DOWN), 50.0)],
               [(100.0, 55.0), (100.0, nxt(55.0, UP))]),
        inside=[((0, 2), (0,))], dropped=[0, 0]),
    # s == 0.0 is inside; the normal (0, 2) is normalised to (0, 1), so y just below 10 is outside
    "half_plane_edge": dict(
        sensors=[("half_plane", 0.0, 2.0, 10.0)],
        spots=([(3.0, 10.0), (3.0, nxt(10.0, DOWN)), (3.0, nxt(10.0, UP))],
               [(0.0, 20.0), (0.0, 0.0)]),
        inside=[((0, 2), (0,))], dropped=[0, 0]),
    # the side the normal points to, for a normal that points down and left
    "half_plane_side": dict(
        sensors=[("half_plane", -1.0, 0.0, -4.0), ("half_plane", 0.0, -1.0, 2.0)],  # x <= 4; y <= -2
        spots=([(4.0, 0.0), (nxt(4.0, UP), 0.0)], [(0.0, -2.0), (0.0, nxt(-2.0, UP))]),
        inside=[((0,), (0, 1)), ((), (0,))], dropped=[0, 0]),
    # a box corner: both tests must hold; hx belongs to the first axis
    "box_corner": dict(
        sensors=[("box", 10.0, 20.0, 4.0, 2.0, 1.0, 0.0)],
        spots=([(14.0, 22.0), (nxt(14.0, UP), 22.0), (14.0, nxt(22.0, UP)), (nxt(14.0, DOWN), nxt(22.0, DOWN))],
               [(13.0, 20.0), (10.0, 23.0)]),
        inside=[((0, 3), (0,))], dropped=[0, 0]),
    # an axis that is not a unit vector is normalised: (0, 3) becomes (0, 1), so the long side lies along y
    "box_axis": dict(
        sensors=[("box", 0.0, 0.0, 4.0, 2.0, 0.0, 3.0)],
        spots=([(0.0, 4.0), (0.0, nxt(4.0, UP)), (2.0, 0.0), (nxt(2.0, UP), 0.0)], [(-2.0, -4.0), (3.0, 0.0)]),
        inside=[((0, 2), (0,))], dropped=[0, 0]),
    # a box given by an angle: a quarter turn puts the long side along y (cos is 6e-17 there, which moves no spot below)
    "box_angle": dict(
        sensors=[("box", 0.0, 0.0, 4.0, 2.0, math.pi / 2)],
        spots=([(0.0, 3.0), (3.0, 0.0)], [(1.5, -3.5), (-2.5, 0.0)]),
        inside=[((0,), (0,))], dropped=[0, 0]),
    # both capsule ends: t is clamped, so the band ends in half discs
    "capsule_ends": dict(
        sensors=[("capsule", 0.0, 0.0, 10.0, 0.0, 2.0)],
        spots=([(-2.0, 0.0), (nxt(-2.0, DOWN), 0.0), (12.0, 0.0), (nxt(12.0, UP), 0.0)],
               [(5.0, 2.0), (5.0, nxt(2.0, UP))]),
        inside=[((0, 2), (0,))], dropped=[0, 0]),
    # l2 == 0: the capsule is a disc about its point
    "capsule_degenerate": dict(
        sensors=[("capsule", 7.0, 7.0, 7.0, 7.0, 1.0)],
        spots=([(8.0, 7.0), (nxt(8.0, UP), 7.0)], [(7.0, 7.0), (9.0, 9.0)]),
        inside=[((0,), (0,))], dropped=[0, 0]),
    # R = 0 holds exactly its centre, and its segment
    "radius_zero": dict(
        sensors=[("disc", 5.0, 5.0, 0.0), ("capsule", 0.0, 0.0, 10.0, 0.0, 0.0)],
        spots=([(5.0, 5.0), (nxt(5.0, UP), 5.0)], [(5.0, 0.0), (5.0, Q)]),
        inside=[((0,), ()), ((), (0,))], dropped=[0, 0]),
    # a NaN position is inside nothing and is not dropped
    "nan": dict(
        sensors=[("disc", 0.0, 0.0, 1e6), ("half_plane", 1.0, 0.0, -1e6), ("box", 0.0, 0.0, 1e6, 1e6, 0.0), ("capsule", 0.0, 0.0, 1.0, 1.0, 1e6)],
        spots=([(NAN, 0.0), (1.0, 1.0)], [(0.0, NAN), (2.0, 2.0)]),
        inside=[((1,), (1,))] * 4, dropped=[0, 0]),
    # 2^40 scales to 2^56: dropped once per sensor that holds it, counted nowhere; an infinity likewise
    "far": dict(
        sensors=[("half_plane", 1.0, 0.0, 0.0), ("disc", 0.0, 0.0, 10.0), ("half_plane", 0.0, 1.0, 1.0)],
        spots=([(FAR, 0.0), (1.0, 0.0), (math.inf, 5.0)], [(3.0, FAR), (3.0, 3.0)]),
        inside=[((1,), (1,)), ((1,), (1,)), ((), (1,))], dropped=[2, 2]),  # (0 * inf is a NaN: the third holds no infinity)
    # masks 1, 2 and 3 over the same disc
    "masks": dict(
        sensors=[("disc", 0.0, 0.0, 3.0, "white"), ("disc", 0.0, 0.0, 3.0, "yolk"), ("disc", 0.0, 0.0, 3.0, "both")],
        spots=([(1.0, 1.0), (-2.0, 0.5)], [(0.0, -1.0), (5.0, 5.0)]),
        inside=[((0, 1), ()), ((), (0,)), ((0, 1), (0,))], dropped=[0, 0]),
    # llrint: ties go to even, and negative values round, not truncate
    "rounding": dict(
        sensors=[("disc", 0.0, 0.0, 100.0)],
        spots=([(1.0 + 1.5 * Q, -1.75 * Q), (1.0 + 0.5 * Q, 2.5 * Q)], [(0.5 * Q, 1.5 * Q), (0.75 * Q, 0.0)]),
        inside=[((0, 1), (0, 1))], dropped=[0, 0]),
    "empty_list": dict(sensors=[], spots=([(1.0, 1.0), (0.0, 0.0)], [(2.0, 2.0), (0.0, 0.0)]), inside=[], dropped=[0, 0]),
    # 64 sensors: disc k has radius k + 0.5
    "sixty_four": dict(
        sensors=[("disc", 0.0, 0.0, k + 0.5) for k in range(64)],
        spots=([(10.0, 0.0), (40.0, 0.0)], [(0.0, 63.0), (0.0, 64.0)]),
        inside=[(tuple(i for i, r in enumerate((10, 40)) if k >= r), (0,) if k >= 63 else ()) for k in range(64)], dropped=[0, 0]),
}

# the case(s) that must notice each wrong rule
NOTICED_BY = {
    "strict": ["disc_edge", "half_plane_edge", "box_corner", "capsule_ends", "radius_zero"],
    "other_side": ["half_plane_edge", "half_plane_side"],
    "unnormalised": ["half_plane_edge", "box_axis"],
    "ignored_mask": ["masks"],
    "swapped_uv": ["box_corner", "box_angle"],
    "unclamped_t": ["capsule_ends"],
    "truncation": ["rounding"],
    "drop_counts": ["far"],
}


def arrays(name):
    """(xs, ys) of a case: per type one float64 array"""
    spots = CASES[name]["spots"]
    return ([np.array([p[0] for p in spots[w]], dtype=np.float64) for w in (0, 1)],
            [np.array([p[1] for p in spots[w]], dtype=np.float64) for w in (0, 1)])


def expected(name):
    """`(sums, dropped)` of a case from the hand-written membership, with Python's round (ties to even)"""
    case = CASES[name]
    sums = []
    for per_type in case["inside"]:
        rec = []
        for w in (0, 1):
            held = [case["spots"][w][i] for i in per_type[w]]
            rec.append((len(held), sum(round(x * 65536.0) for x, _ in held), sum(round(y * 65536.0) for _, y in held)))
        sums.append(tuple(rec))
    return sums, list(case["dropped"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_case(name):
    xs, ys = arrays(name)
    got = sm.read(CASES[name]["sensors"], xs, ys)
    assert got == expected(name)
    assert all(isinstance(v, int) for per_type in got[0] for rec in per_type for v in rec)
    # per batch: everything is one batch, so its counts are the totals' counts (a dropped particle counts in neither)
    per_batch = sm.read_batches(CASES[name]["sensors"], xs, ys, (np.full(xs[0].size, 7), np.full(xs[1].size, 7)), [7, 8, 7])
    want = np.array([[rec[0][0], rec[1][0]] for rec in got[0]], dtype=np.int32).reshape(len(got[0]), 2)
    assert per_batch.dtype == np.int32 and per_batch.shape == (3, len(got[0]), 2)
    assert np.array_equal(per_batch[0], want) and np.array_equal(per_batch[2], want) and not per_batch[1].any()


@pytest.mark.parametrize("wrong", sm.WRONG_RULES)
def test_every_wrong_rule_is_noticed(wrong):
    assert sorted(NOTICED_BY) == sorted(sm.WRONG_RULES)
    for name in NOTICED_BY[wrong]:
        xs, ys = arrays(name)
        assert sm.read(CASES[name]["sensors"], xs, ys, wrong=wrong) != expected(name), (wrong, name)


def test_the_centroid_is_two_divisions_of_the_integers():
    xs, ys = arrays("rounding")
    sums, _ = sm.read(CASES["rounding"]["sensors"], xs, ys)
    assert sums == [((2, 131074, 0), (2, 1, 2))]
    assert sm.readings(sums) == [{"count": (2, 2), "centroid": ((131074 / 65536.0 / 2.0, 0.0), (1 / 65536.0 / 2.0, 2 / 65536.0 / 2.0))}]
    assert sm.readings([((0, 0, 0), (3, 3 * 65536, -6 * 65536))]) == [{"count": (0, 3), "centroid": (None, (1.0, -2.0))}]


def test_the_list_as_it_is_stored():
    got = sm.canonical([("half_plane", 0.0, 2.0, 10.0, "yolk"), ("box", 1.0, 2.0, 3.0, 4.0, 0.0, -5.0), ("capsule", 1.0, 2.0, 3.0, 4.0, 5.0),
                        ("box", 0.0, 0.0, 1.0, 1.0, math.pi / 2, "white")])
    assert got[0] == ("half_plane", 2, [0.0, 1.0, 10.0, 0.0, 0.0, 0.0])
    assert got[1] == ("box", 3, [1.0, 2.0, 3.0, 4.0, 0.0, -1.0])
    assert got[2] == ("capsule", 3, [1.0, 2.0, 3.0, 4.0, 5.0, 0.0])  # (parameters a kind does not use are 0)
    assert got[3][1] == 1 and got[3][2][4:] == [math.cos(math.pi / 2), 1.0]
    for bad, index in (([("disc", 0.0, 0.0, -1.0)], 0), ([("disc", 0.0, 0.0, 1.0), ("box", 0.0, 0.0, 1.0, -1.0, 1.0, 0.0)], 1),
                       ([("half_plane", 0.0, 1e-9, 0.0)], 0), ([("box", 0.0, 0.0, 1.0, 1.0, 0.0, 0.0)], 0),
                       ([("disc", 0.0, math.inf, 1.0)], 0), ([("capsule", 0.0, 0.0, 1.0, 1.0, NAN)], 0), ([("ring", 0.0, 0.0, 1.0)], 0),
                       ([("disc", 0.0, 0.0, 1.0, "none")], 0), ([("disc", 0.0, 0.0, 1.0)] * 2 + [("capsule", 0.0, 0.0, 1.0, 1.0, -2.0)], 2)):
        with pytest.raises(ValueError, match="sensor %d" % index):
            sm.canonical(bad)
    with pytest.raises(ValueError, match="0 .. 64"):
        sm.canonical([("disc", 0.0, 0.0, 1.0)] * 65)
    assert len(sm.canonical([("disc", 0.0, 0.0, 1.0)] * 64)) == 64 and sm.canonical([]) == []
