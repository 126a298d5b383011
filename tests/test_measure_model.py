"""The measures (egg_measure) as far as the rule can be checked without a device: the numpy model
tests/measure_model.py against a hand table of atoms whose records were worked on paper, the wrong rules the table must
notice, and the values the wrappers derive from a record.  tests/test_gpu_measures.py holds the device against the same
model; tests/test_measure_surface.py holds the header, the bindings and the documents."""
import math

import numpy as np
import pytest

import measure_model as mm

S = 65536
SM = 1 << 32
NAN = float("nan")

# name -> the particles of ONE white atom as rows (x, y, vx, vy, radius, inv_mass), a region or None, and the record by hand
GOOD = [(1.0, 0.0, 1.0, 2.0, 1.0, 1.0), (3.0, 0.0, -1.0, 3.0, 1.0, 0.5)]
GOOD_RECORD = dict(sx=4 * S, sy=0, sm=3 * SM, smx=7 * S, smy=0, spx=-S, spy=8 * S, se=25 * S, lo_x=0, lo_y=-S, hi_x=4 * S, hi_y=S,
                   max_v2=10 * S, ox_q=2 * S, oy_q=0, dropped_central=0, sxx=2 * S, sxy=0, syy=0, sl=4 * S, max_reach=2 * S)
CASES = {
    # m = 2: every sum is the one particle's term, the origin is the particle and only its radius reaches out
    "one": dict(rows=[(1.0, 2.0, 3.0, -4.0, 0.5, 0.5)], region=None,
                record=dict(atom=1, n=1, dropped=0, sx=S, sy=2 * S, sm=2 * SM, smx=2 * S, smy=4 * S, spx=6 * S, spy=-8 * S, se=50 * S,
                            lo_x=S // 2, lo_y=3 * S // 2, hi_x=3 * S // 2, hi_y=5 * S // 2, max_v2=25 * S, ox_q=S, oy_q=2 * S,
                            dropped_central=0, sxx=0, sxy=0, syy=0, sl=0, max_reach=S // 2)),
    # sx = -7 over three particles: C division gives -2 (-7 / 3 = -2.33 toward zero), a floor gives -3
    "negative_origin": dict(rows=[(-1.0 / S, 0.0, 0.0, 0.0, 0.0, 1.0), (-2.0 / S, 0.0, 0.0, 0.0, 0.0, 1.0), (-4.0 / S, 0.0, 0.0, 0.0, 0.0, 1.0)],
                            region=None,
                            record=dict(atom=3, n=3, dropped=0, sx=-7, sy=0, sm=3 * SM, smx=-7, smy=0, spx=0, spy=0, se=0, lo_x=-4, lo_y=0,
                                        hi_x=-1, hi_y=0, max_v2=0, ox_q=-2, oy_q=0, dropped_central=0, sxx=0, sxy=0, syy=0, sl=0, max_reach=2)),
    # sx = -2 over three: the origin is 0 (a floor gives -1; the unquantised centroid -2/3 brings the reach down to 1.33 -> 1)
    "thirds": dict(rows=[(0.0, 0.0, 0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0, 0.0, 0.0, 1.0), (-2.0 / S, 0.0, 0.0, 0.0, 0.0, 1.0)], region=None,
                   record=dict(atom=3, n=3, dropped=0, sx=-2, sy=0, sm=3 * SM, smx=-2, smy=0, spx=0, spy=0, se=0, lo_x=-2, lo_y=0, hi_x=0,
                               hi_y=0, max_v2=0, ox_q=0, oy_q=0, dropped_central=0, sxx=0, sxy=0, syy=0, sl=0, max_reach=2)),
    # -0.0 and 0.0: every quantised term is the integer 0, in either order
    "signed_zeros": dict(rows=[(-0.0, 0.0, 0.0, 0.0, 0.0, 1.0), (0.0, -0.0, 0.0, 0.0, 0.0, 1.0)], region=None,
                         record=dict(atom=2, n=2, dropped=0, sx=0, sy=0, sm=2 * SM, smx=0, smy=0, spx=0, spy=0, se=0, lo_x=0, lo_y=0, hi_x=0,
                                     hi_y=0, max_v2=0, ox_q=0, oy_q=0, dropped_central=0, sxx=0, sxy=0, syy=0, sl=0, max_reach=0)),
    # two good particles (m = 1 and m = 2) alone ...
    "good": dict(rows=GOOD, region=None, record=dict(GOOD_RECORD, atom=2, n=2, dropped=0)),
    # ... and among a NaN velocity, x = 2^37 (x S = 2^53 is not below the limit) and inv_mass = 0 (m = inf): the three are
    # dropped and nothing else moves, though each lies outside the box of the good ones
    "dropped": dict(rows=[(-100.0, 7.0, NAN, 0.0, 1.0, 1.0), GOOD[0], (2.0 ** 37, 0.0, 0.0, 0.0, 1.0, 1.0), GOOD[1], (50.0, 50.0, 0.0, 0.0, 1.0, 0.0)],
                    region=None, record=dict(GOOD_RECORD, atom=5, n=5, dropped=3)),
    # seven particles at 0 and one at 2^21: the origin is 2^18; the seven give (2^18)^2 S = 2^52 each, the far one 49 * 2^52,
    # beyond the limit: it is kept by pass 1 and dropped by pass 2
    "dropped_central": dict(rows=[(0.0, 0.0, 0.0, 0.0, 0.0, 1.0)] * 7 + [(2.0 ** 21, 0.0, 0.0, 0.0, 0.0, 1.0)], region=None,
                            record=dict(atom=8, n=8, dropped=0, sx=2 ** 37, sy=0, sm=8 * SM, smx=2 ** 37, smy=0, spx=0, spy=0, se=0, lo_x=0,
                                        lo_y=0, hi_x=2 ** 37, hi_y=0, max_v2=0, ox_q=2 ** 34, oy_q=0, dropped_central=1, sxx=7 * 2 ** 52,
                                        sxy=0, syy=0, sl=0, max_reach=2 ** 34)),
    # a disc about the first good particle holds it alone: the atom has 2 particles, 1 is measured
    "region_part": dict(rows=GOOD, region=("disc", 1.0, 0.0, 0.5),
                        record=dict(atom=2, n=1, dropped=0, sx=S, sy=0, sm=SM, smx=S, smy=0, spx=S, spy=2 * S, se=5 * S, lo_x=0, lo_y=-S,
                                    hi_x=2 * S, hi_y=S, max_v2=5 * S, ox_q=S, oy_q=0, dropped_central=0, sxx=0, sxy=0, syy=0, sl=0, max_reach=S)),
    # a region over both whose own mask is yolk only: nothing of the white is measured
    "region_other_type": dict(rows=GOOD, region=("disc", 1.0, 0.0, 10.0, "yolk"), record=dict(dict.fromkeys(mm.FIELDS, 0), atom=2)),
}


def _particles(rows, batch=1):
    cols = np.array(rows, dtype=np.float64).reshape(-1, 6).T
    white = dict(zip(("x", "y", "vx", "vy", "radius", "inv_mass"), cols), batch_id=np.full(len(rows), batch))
    return white, dict(white, **{k: v[:0] for k, v in white.items()})


def _record(case, rule=None, order=None):
    rows = case["rows"] if order is None else [case["rows"][i] for i in order]
    return tuple(mm.measure(_particles(rows), [1], case["region"], 3, rule)[0][0].tolist()) if rule != "double_extremes" else \
        _raw(rows, case["region"], rule)


def _raw(rows, region, rule):
    """record_of itself (its tuple may hold doubles under a wrong rule, which an int64 table would hide)"""
    white, _ = _particles(rows)
    assert region is None
    return mm.record_of(*(white[k] for k in ("x", "y", "vx", "vy", "radius", "inv_mass")), rule=rule)


def _is(rec, want):
    """integer for integer: same values AND every entry an int (a double -0.0 equals 0 and is not the same bits)"""
    return len(rec) == 24 and all(isinstance(a, int) and not isinstance(a, bool) and a == b for a, b in zip(rec, want))


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_table(name):
    case = CASES[name]
    want = tuple(case["record"][f] for f in mm.FIELDS)
    assert len(case["record"]) == 24
    got = _record(case)
    assert got == want, [(f, a, b) for f, a, b in zip(mm.FIELDS, got, want) if a != b]
    # no answer depends on the order of the particles
    n = len(case["rows"])
    assert _record(case, order=list(range(n))[::-1]) == want
    assert _record(case, order=[(3 * i + 1) % n for i in range(n)] if n % 3 else list(range(1, n)) + [0]) == want


def test_the_dropped_leave_the_others_unchanged():
    alone, among = CASES["good"]["record"], CASES["dropped"]["record"]
    assert {f: v for f, v in among.items() if f not in ("atom", "n", "dropped")} == {f: v for f, v in alone.items() if f not in ("atom", "n", "dropped")}
    # each of the three alone is an atom with nothing kept: fields 3 .. 23 are 0
    for row in (CASES["dropped"]["rows"][i] for i in (0, 2, 4)):
        rec = _record(dict(rows=[row], region=None))
        assert rec == (1, 1, 1) + (0,) * 21, row
    # every particle dropped by pass 2: fields 19 .. 23 are 0 and the origin stands
    rec = _record(dict(rows=[(0.0, 0.0, 0.0, 0.0, 0.0, 1.0), (2.0 ** 36, 0.0, 0.0, 0.0, 0.0, 1.0)], region=None))
    assert rec[:3] == (2, 2, 0) and rec[16:19] == (2 ** 51, 0, 2) and rec[19:] == (0,) * 5 and rec[3] == 2 ** 52


# which case notices which wrong rule
NOTICED_BY = {"floor": ("negative_origin", "thirds"), "double_extremes": ("signed_zeros",), "centroid_origin": ("thirds",),
              "dropped_extremes": ("dropped",), "inv_mass": ("good", "one")}


def test_the_table_notices_the_wrong_rules():
    assert set(NOTICED_BY) == set(mm.WRONG_RULES)
    for rule, names in NOTICED_BY.items():
        for name in names:
            case = CASES[name]
            want = tuple(case["record"][f] for f in mm.FIELDS)
            n = len(case["rows"])
            got = [_record(case, rule, order) for order in (None, list(range(n))[::-1])]
            assert not all(_is(g, want) for g in got), (rule, name)
            assert all(_is(_record(case, None, order), want) for order in (None, list(range(n))[::-1])), name
    # what each one changes, by hand
    assert _record(CASES["negative_origin"], "floor")[16] == -3 and _record(CASES["thirds"], "floor")[16] == -1
    assert _record(CASES["thirds"], "centroid_origin")[23] == 1
    assert _record(CASES["dropped"], "dropped_extremes")[11] == -101 * S
    assert _record(CASES["good"], "inv_mass")[5] == 3 * SM // 2
    # extremes on doubles: the values agree, the bits of a zero do not -- and they follow the order of the particles
    a, b = (_record(CASES["signed_zeros"], "double_extremes", order) for order in (None, [1, 0]))
    assert a == b and [math.copysign(1.0, v) for v in a[11:15]] != [math.copysign(1.0, v) for v in b[11:15]]


def test_requests_masks_and_repeats():
    white, _ = _particles(CASES["good"]["rows"], batch=7)
    other, _ = _particles(CASES["one"]["rows"], batch=9)
    both = {k: np.concatenate([white[k], other[k]]) for k in white}
    yolk, _ = _particles(CASES["one"]["rows"], batch=7)
    good = tuple(CASES["good"]["record"][f] for f in mm.FIELDS)
    one = tuple(CASES["one"]["record"][f] for f in mm.FIELDS)
    table = mm.measure((both, yolk), [9, 7, 9, 8])
    assert table.shape == (4, 2, 24) and table.dtype == np.int64
    assert tuple(table[0, 0]) == one and tuple(table[1, 0]) == good and tuple(table[2, 0]) == one and tuple(table[1, 1]) == one
    assert not table[0, 1].any() and not table[3].any()  # a type the batch lacks, a batch without particles
    assert not mm.measure((both, yolk), [7], mask=2)[0, 0].any() and tuple(mm.measure((both, yolk), [7], mask=2)[0, 1]) == one
    assert mm.measure((both, yolk), []).shape == (0, 2, 24)


def test_derived_values_follow_the_stated_formulas():
    from egg_fluid_simulation_amd.simulation_handler import Measure, SimulationHandler
    rec = tuple(CASES["good"]["record"][f] for f in mm.FIELDS)
    m = Measure(*rec)
    d = mm.derived(rec)
    assert Measure._fields == mm.FIELDS and m.kept == 2 and m.mass == 3.0 == d["mass"]
    assert m.centroid == (2.0, 0.0) == d["centroid"] and m.center_of_mass == (7.0 / 3.0, 0.0) == d["center_of_mass"]
    assert m.momentum == (-1.0, 8.0) == d["momentum"] and m.velocity == (-1.0 / 3.0, 8.0 / 3.0) == d["velocity"]
    assert m.kinetic_energy == 12.5 == d["kinetic_energy"] and m.bounds == (0.0, -1.0, 4.0, 1.0) == d["bounds"]
    assert m.max_speed == math.sqrt(10.0) == d["max_speed"] and m.origin == (2.0, 0.0) and m.reach == 2.0 == d["reach"] and m.spin == 4.0 == d["spin"]
    assert m.axes() == (1.0, 0.0, 0.0) == mm.axes(rec)  # dx = -1, +1: variance 1 along x, none along y
    turned = Measure(*(rec[:19] + (0, 0, 8 * S) + rec[22:]))
    assert turned.axes() == (2.0, 0.0, 0.5 * math.pi)
    # nothing kept: no centroid, no bounds, no axes; nothing measured: the wrappers give None
    gone = Measure(*((1, 1, 1) + (0,) * 21))
    assert gone.centroid is None and gone.bounds is None and gone.center_of_mass is None and gone.velocity is None and gone.axes() is None
    assert gone.max_speed == 0.0 and mm.derived((1, 0, 0) + (0,) * 21) is None
    table = np.array([[rec, (2, 0, 0) + (0,) * 21]], dtype=np.int64)
    assert SimulationHandler._measures(table) == [(m, None)]
