"""The directed operands of tests/arith_cases.py, without a device: that they are what they claim to be, that numpy may
stand in for exact arithmetic on them, and that they would notice the error they are built for.

The device part is tests/test_gpu_arith_cases.py."""
import math
import random
from fractions import Fraction

import numpy as np
import pytest

import arith_cases as ac

SUBSET = 4096


@pytest.fixture(scope="module")
def table():
    return ac.cases()


@pytest.fixture(scope="module")
def subset(table):
    """4,096 of the near-midpoint division cases (both regimes and the composition), chosen once"""
    n, d, x, fam = table
    hard = np.flatnonzero(fam <= ac.FAMILIES.index("compose"))
    pick = np.array(sorted(random.Random(7).sample(list(hard), SUBSET)))
    return pick


def test_the_table_is_what_the_docstring_says(table):
    n, d, x, fam = table
    counts = dict(zip(ac.FAMILIES, np.bincount(fam, minlength=len(ac.FAMILIES)).tolist()))
    print("operand triples per family:", counts, "total", len(n))
    assert all(counts[f] > 0 for f in ac.FAMILIES)
    assert 2 ** 15 < len(n) <= 2 ** 17  # about 2^16
    lo, hi = 2.0 ** ac.LO_EXP, 2.0 ** ac.HI_EXP
    for v in (np.abs(n), np.abs(d)):
        assert (v >= lo).all() and (v <= hi).all()
    assert (x >= lo * lo).all() and (x <= hi * hi).all()
    # both ends of every window are there themselves
    assert (np.abs(d) == lo).any() and (np.abs(d) == hi).any() and (x == lo * lo).any() and (x == hi * hi).any()
    assert (np.abs(n) < 2 * lo).any() and (np.abs(n) > hi / 2).any()
    # both regimes, both signs of a numerator, |n| <= c in the composition
    lt, ge, co = (fam == ac.FAMILIES.index(f) for f in ("div_mid_lt", "div_mid_ge", "compose"))
    assert lt.sum() > 4096 and ge.sum() > 4096
    assert (np.abs(n[co]) <= np.abs(d[co])).all() and (n[co] < 0).any() and (n[co] > 0).any()
    assert np.array_equal(np.sqrt(x[co]), np.abs(d[co]))  # x = fl(c c): the root is c


def test_division_cases_lie_next_to_a_midpoint(table, subset):
    n, d, x, fam = table
    worst = Fraction(0)
    for i in subset:
        D, _ = ac.decompose(abs(float(d[i])))
        assert D % 2 == 1
        dist = ac.midpoint_distance(float(n[i]), float(d[i]))
        assert dist <= Fraction(1, D), (i, float(n[i]).hex(), float(d[i]).hex())
        worst = max(worst, dist)
    print("largest distance from a midpoint: %.3g units of the last place" % float(worst))


def test_numpy_is_exactly_rounded_on_the_subset(table, subset):
    """the licence to use numpy's `/` and sqrt as the reference for the whole table"""
    n, d, x, fam = table
    with np.errstate(all="raise"):
        quo, root = n / d, np.sqrt(x)
        nq = n / root
    for i in subset:
        assert float(quo[i]) == ac.round_quotient(float(n[i]), float(d[i])), i
        assert float(root[i]) == ac.round_sqrt(float(x[i])), i
        assert float(nq[i]) == ac.round_quotient(float(n[i]), float(root[i])), i
    # ... every case with a divisor next to a power of two, and every square-root case, for they are few
    for i in np.flatnonzero(fam == ac.FAMILIES.index("div_near_ones")):
        assert float(quo[i]) == ac.round_quotient(float(n[i]), float(d[i])) and float(nq[i]) == ac.round_quotient(float(n[i]), float(root[i])), i
    for i in np.flatnonzero(fam >= ac.FAMILIES.index("sqrt_mid")):
        assert float(root[i]) == ac.round_sqrt(float(x[i])) == math.sqrt(float(x[i])), i


def test_the_set_notices_a_faithful_but_not_nearest_reciprocal(table, subset):
    """egg_div_with_rcp in rational arithmetic: with the correctly rounded reciprocal it rounds every case correctly, with
    the other faithful neighbour it misrounds at least 10 % of the N < D family (a quarter, in fact) -- and none of as many
    random numerators"""
    n, d, x, fam = table
    lt = [i for i in subset if fam[i] != ac.FAMILIES.index("div_mid_ge")]
    assert len(lt) > 1000 and not any(fam[i] == ac.FAMILIES.index("div_near_ones") for i in lt)
    bad_nearest = bad_other = bad_random = 0
    rng = random.Random(3)
    for i in lt:
        ni, di = float(n[i]), float(d[i])
        want = ac.round_quotient(ni, di)
        r0, r1 = ac.reciprocals(di)
        bad_nearest += ac.div_with_rcp_model(ni, di, r0) != want
        bad_other += ac.div_with_rcp_model(ni, di, r1) != want
        nr = math.copysign(math.ldexp(rng.randrange(2 ** 52, 2 ** 53), math.frexp(ni)[1] - 53), ni)
        bad_random += ac.div_with_rcp_model(nr, di, r1) != ac.round_quotient(nr, di)
    print("N < D cases %d: misrounded with the nearest reciprocal %d, with the other faithful one %d (%.1f %%); random numerators %d"
          % (len(lt), bad_nearest, bad_other, 100.0 * bad_other / len(lt), bad_random))
    assert bad_nearest == 0
    assert bad_other >= 0.10 * len(lt)
    assert bad_random < 0.01 * len(lt)
