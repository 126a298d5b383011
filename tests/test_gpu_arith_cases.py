"""The hand-expanded f64 division and square roots of csrc/eggsim_tile.h on the directed operands of tests/arith_cases.py
(egg_selftest_arith_operands returns the raw results, nothing is judged on the device): every quotient and every root must
be numpy's, bit for bit -- tests/test_arith_cases.py shows on a rational subset that numpy's are the exactly rounded ones,
and that these operands notice a division handed the wrong faithful reciprocal.

Measured, not asserted: how often the root core's reciprocal `rroot` is not the correctly rounded 1 / root (the quotient
n / root must be right either way; figures in profiles/r26_arith_hard_cases.md)."""
import numpy as np
import pytest

import arith_cases as ac

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def results():
    import egg_fluid_simulation_amd as egg
    from egg_fluid_simulation_amd import _ffi
    n, d, x, fam = ac.cases()
    out = egg.SimulationHandler().selftest_arith_operands(n, d, x)
    assert out.shape == (n.size, len(_ffi.ARITH_COLUMNS))
    return n, d, x, fam, {name: out[:, k] for k, name in enumerate(_ffi.ARITH_COLUMNS)}


def _mismatches(got, want, fam):
    bad = _bits(got) != _bits(want)
    return int(bad.sum()), {ac.FAMILIES[f]: int(c) for f, c in enumerate(np.bincount(fam[bad], minlength=len(ac.FAMILIES))) if c}, np.flatnonzero(bad)[:4]


def _compare(results, select):
    n, d, x, fam, got = results
    with np.errstate(all="raise"):
        root = np.sqrt(x)
        want = dict(div=n / d, sqrt=root, root=root, div_root=n / root, op_div=n / d, op_sqrt=root, op_div_sqrt=n / root)
    report = {name: _mismatches(np.where(select, got[name], ref), ref, fam) for name, ref in want.items()}
    for name, (count, by_family, first) in report.items():
        print("%-12s %d mismatches of %d %s" % (name, count, int(select.sum()), by_family or ""))
        for i in first:
            print("    n %s d %s x %s: got %s want %s" % (float(n[i]).hex(), float(d[i]).hex(), float(x[i]).hex(), float(got[name][i]).hex(), float(want[name][i]).hex()))
    bad = _bits(got["op_div"]) != _bits(want["op_div"])
    pairs = sorted({(float(np.frexp(n[i])[0]).hex(), float(np.frexp(d[i])[0]).hex()) for i in np.flatnonzero(bad & select)})
    if pairs:
        print("operand mantissas (n, d) egg_div misrounds:", pairs)
    return {k: v[:2] for k, v in report.items() if v[0]}


def test_directed_operands_bit_for_bit(results):
    """the families the hand expansions were written against: 64,308 triples, every column"""
    fam = results[3]
    assert not _compare(results, fam != ac.FAMILIES.index("div_near_ones"))


def test_divisors_next_to_a_power_of_two(results):
    """the 2,688 triples of `div_near_ones`.  Up to round 25, and with the compiler's bare `/` to this day, 42 of them come
    out one unit of the last place short in magnitude -- three operand pairs at seven scales and with either sign, each
    1 / (2 D) from a rounding midpoint:
        0x1.6666666666663p+0 / 0x1.ffffffffffffbp+0 (D = 2^53 - 5):  0x1.6666666666666p-1, exactly rounded 0x1.6666666666667p-1
        0x1.5d1745d1745cap+0 / 0x1.ffffffffffff5p+0 (D = 2^53 - 11): ...5d1p-1, exactly rounded 0x1.5d1745d1745d2p-1
        0x1.276276276275bp+0 / 0x1.ffffffffffff3p+0 (D = 2^53 - 13): ...762p-1, exactly rounded 0x1.2762762762763p-1
    v_rcp_f64 and two Newton steps leave the reciprocal of 2 - k 2^-52 one unit low (measured for k = 3 .. 13), and the
    quotient sequence needs the nearest one.  egg_rcp_refined now finishes the reciprocal, and egg_div the operator's quotient,
    by comparing exact residuals (csrc/eggsim_tile.h); every division of the exact path goes through one of the two."""
    fam = results[3]
    assert not _compare(results, fam == ac.FAMILIES.index("div_near_ones"))


def test_hand_expansion_equals_the_operator(results):
    """the hand expansions and egg_div / sqrt, which project_pair_reference and the follow constraint use, are one arithmetic on
    all 66,996 triples"""
    n, d, x, fam, got = results
    for mine, theirs in (("div", "op_div"), ("sqrt", "op_sqrt"), ("root", "op_sqrt"), ("div_root", "op_div_sqrt")):
        bad = np.flatnonzero(_bits(got[mine]) != _bits(got[theirs]))
        assert bad.size == 0, (mine, theirs, bad.size, [(float(n[i]).hex(), float(d[i]).hex(), float(x[i]).hex()) for i in bad[:4]])


def test_rroot_census(results):
    """how often rroot is the other faithful neighbour of 1 / root, per family: a figure, not a condition"""
    n, d, x, fam, got = results
    root, rroot = got["root"], got["rroot"]
    nearest = 1.0 / root
    off = _bits(rroot).astype(np.int64) - _bits(nearest).astype(np.int64)
    differs = off != 0
    print("rroot != correctly rounded 1 / root: %d of %d" % (int(differs.sum()), n.size))
    for f, name in enumerate(ac.FAMILIES):
        sel = fam == f
        print("    %-12s %6d of %6d" % (name, int((differs & sel).sum()), int(sel.sum())))
    print("    largest distance: %d units of the last place" % int(np.abs(off).max()))
    assert np.isfinite(rroot).all() and (rroot > 0).all()
