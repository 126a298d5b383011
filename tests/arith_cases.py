"""Directed operands for the hand-expanded f64 division and square root of csrc/eggsim_tile.h (egg_rcp_refined,
egg_div_with_rcp, egg_sqrt_core, egg_sqrt_rcp_core).  Test helper, not collected.

egg_selftest_arith draws random mantissas.  The sequence q = n r; rem = fma(-d, q, n); fma(rem, r, q) is correct for the
correctly rounded reciprocal r; with the other faithful neighbour it misrounds the quotients that lie next to a rounding
midpoint, and random operands never produce those (tests/test_arith_cases.py measures both).  This file builds such operands
with Python integers only:

  div_mid_lt, div_mid_ge   for an odd 53-bit D the N with N 2^53 = k D + (D +- 1) / 2 (N < D, quotient in [1/2, 1)) or
                           N 2^52 = k D + (D +- 1) / 2 (D <= N < 2^53, quotient in [1, 2)): N = ((D +- 1) / 2 * 2^-s) mod D.
                           The quotient is k + 1/2 +- 1/(2 D) units of its last place.  D: random, and 2^52 + 1, 2^52 + 3,
                           2^53 - 1, 2^53 - 3.  x = fl(d d), whose root is |d|: n / root through the root core's reciprocal is
                           the projection's normalisation dx / current on the same hard pair.
  compose                  the kernel's own composition at the solver's scale: x = fl(c c), numerators of either sign that are
                           hard for c, |n| <= c (the div_mid_lt construction), c between 2^-20 and 2^5
  div_near_ones            D = 2^53 - k and 2^52 + k, k = 1, 3 .. 31, numerators of either sign 1, 3, 5 and 7 half-units of 1 / D
                           from a midpoint, both regimes
  div_exact                n == d; d a power of two; zero remainders (n = q d with short q and d)
  sqrt_mid                 x = C^2 + C, C^2 + C +- 1 (C of 26 bits and of a few bits), at an even and at an odd exponent; the
                           53-bit neighbours of a rounding midpoint of the root: 1 + k 2^-52 (root 1 + k 2^-53 - ...) and
                           4 - k 2^-51 (root 2 - k 2^-52 ... : half units for odd k), k = 1 .. 63
  sqrt_square              perfect squares C^2, at an even and at an odd exponent

every one of them scaled over the windows the code claims -- |n|, |d| in [2^-300, 2^300], x in [2^-600, 2^600] -- including
EGG_ARITH_LO = 2^-300 and EGG_ARITH_HI = 2^300 themselves (as a power-of-two divisor and as the root of x = 2^-600, 2^600).
Every triple is inside the windows.  cases() returns about 2^16 triples."""
import math
import random
from fractions import Fraction

import numpy as np

FAMILIES = ("div_mid_lt", "div_mid_ge", "compose", "div_near_ones", "div_exact", "sqrt_mid", "sqrt_square")
LO_EXP, HI_EXP = -300, 300
SPECIAL_D = (2 ** 52 + 1, 2 ** 52 + 3, 2 ** 53 - 1, 2 ** 53 - 3)
# (exponent of n's unit, of d's): both ends of the window alone and against each other, the solver's range, in between
DIV_SCALES = ((-52, -52), (-352, -352), (247, 247), (-352, 247), (247, -352), (-79, -72), (98, -202))
SQRT_EXPONENTS = (0, -600, 546, -54, 10, 300, -301)  # of x's unit; a 53-bit mantissa at 2^546 ends below 2^600


def midpoint_numerators(D, regime, offsets=(1, -1)):
    """the numerators N (53-bit integers) whose quotient by the odd D lies |s| / (2 D) units of the last place from a
    rounding midpoint, s in `offsets` (odd); regime "lt": 2^52 <= N < D, "ge": D <= N < 2^53"""
    assert D % 2 == 1 and 2 ** 52 <= D < 2 ** 53
    inv = pow(2 ** (53 if regime == "lt" else 52), -1, D)
    out = []
    for s in offsets:
        N = ((D + s) // 2 * inv) % D
        if regime == "ge":
            N += D
        if 2 ** 52 <= N < 2 ** 53:
            out.append(N)
    return out


def _triple(N, en, D, ed):
    n, d = math.ldexp(N, en), math.ldexp(D, ed)
    return n, d, d * d


def cases(seed=1, n_random_d=4500):
    """(n, d, x, family) as numpy arrays: float64 operands and the index into FAMILIES"""
    rng = random.Random(seed)
    rows = []

    def add(fam, n, d, x):
        assert 2.0 ** LO_EXP <= abs(n) <= 2.0 ** HI_EXP and 2.0 ** LO_EXP <= abs(d) <= 2.0 ** HI_EXP, (fam, n, d)
        assert 2.0 ** (2 * LO_EXP) <= x <= 2.0 ** (2 * HI_EXP), (fam, x)
        rows.append((n, d, x, FAMILIES.index(fam)))

    ds = list(SPECIAL_D) + [rng.randrange(2 ** 52, 2 ** 53) | 1 for _ in range(n_random_d)]
    for regime in ("lt", "ge"):
        for D in ds:
            for N in midpoint_numerators(D, regime):
                for en, ed in DIV_SCALES:
                    add("div_mid_" + regime, *_triple(N, en, D, ed))
    # the kernel's composition: c between 2^-20 and 2^5, the numerator of either sign and no larger than c
    for D in ds:
        for N in midpoint_numerators(D, "lt"):
            e = rng.randrange(-72, -46)
            for sign in (1, -1):
                add("compose", *_triple(sign * N, e, D, e))
    # divisors next to a power of two, where a Newton-refined reciprocal is the least certain to be the nearest one (measured
    # on an MI355X: v_rcp_f64 and two Newton steps leave 1 / (2 - k 2^-52) one unit low for k = 3, 5, .. 13, and the
    # compiler's `/` misrounds with it), with the numerators 1, 3, 5, 7 half-units of 1 / D from a midpoint
    for D in [2 ** 53 - k for k in range(1, 32, 2)] + [2 ** 52 + k for k in range(1, 32, 2)]:
        for regime in ("lt", "ge"):
            for N in midpoint_numerators(D, regime, (1, -1, 3, -3, 5, -5, 7, -7)):
                for en, ed in DIV_SCALES:
                    for sign in (1, -1):
                        add("div_near_ones", *_triple(sign * N, en, D, ed))
    # exact quotients
    for k in range(400):
        M = rng.randrange(2 ** 52, 2 ** 53)
        for en, ed in DIV_SCALES[:5]:
            add("div_exact", *_triple(M, en, M, ed))               # n == d up to the scale
            add("div_exact", *_triple(M, en, 1, ed + 52))          # d a power of two
        q, dd = rng.randrange(2 ** 25, 2 ** 26), rng.randrange(2 ** 25, 2 ** 26) | 1
        add("div_exact", *_triple(q * dd, -52, dd, -25))           # zero remainder
    for M in (2 ** 52, 2 ** 53 - 1, 2 ** 52 + 1):
        for n_exp, d_exp in ((LO_EXP, LO_EXP), (HI_EXP, HI_EXP), (LO_EXP, HI_EXP), (HI_EXP, LO_EXP), (0, LO_EXP), (0, HI_EXP)):
            n = math.ldexp(M, n_exp - 52) if n_exp < HI_EXP else math.ldexp(M, n_exp - 53)
            d = math.ldexp(1.0, d_exp)                             # EGG_ARITH_LO and EGG_ARITH_HI themselves; x = 2^-600, 2^600
            add("div_exact", n, d, d * d)

    def sqrt_rows(fam, mantissas):
        for X in mantissas:
            if not 0 < X < 2 ** 53:
                continue
            for e in SQRT_EXPONENTS:
                for odd in (0, 1):
                    x = math.ldexp(X, e + odd)
                    if not 2.0 ** (2 * LO_EXP) <= x <= 2.0 ** (2 * HI_EXP):
                        continue
                    N = rng.randrange(2 ** 52, 2 ** 53)
                    add(fam, math.ldexp(N, -52), math.ldexp(rng.randrange(2 ** 52, 2 ** 53) | 1, -52), x)

    cs = [rng.randrange(2 ** 25, 2 ** 26) for _ in range(150)] + [1, 2, 3, 5, 2 ** 26 - 1, 2 ** 25, 94906265]
    sqrt_rows("sqrt_mid", [C * C + C + t for C in cs for t in (0, 1, -1)])
    sqrt_rows("sqrt_mid", [2 ** 52 + k for k in range(1, 64)] + [2 ** 53 - k for k in range(1, 64)])
    sqrt_rows("sqrt_square", [C * C for C in cs])
    n, d, x, fam = (np.array(col) for col in zip(*rows))
    return n.astype(np.float64), d.astype(np.float64), x.astype(np.float64), fam.astype(np.int64)


# ---------------------------------------------------------------------------------------- exact references (rational)
def decompose(v):
    """(M, e) with v == M 2^e, M an integer of 53 bits"""
    m, e = math.frexp(v)
    return int(math.ldexp(m, 53)), e - 53


def exact_quotient(n, d):
    return Fraction(n) / Fraction(d)


def midpoint_distance(n, d):
    """|frac - 1/2| of the exact quotient in units of its last place (53 bits), as a Fraction"""
    q = abs(exact_quotient(n, d))
    q *= Fraction(2) ** (52 - (q.numerator.bit_length() - q.denominator.bit_length()))
    while q >= 2 ** 53:
        q /= 2
    while q < 2 ** 52:
        q *= 2
    return abs(q - math.floor(q) - Fraction(1, 2))


def round_quotient(n, d):
    """n / d correctly rounded (an integer true division is)"""
    return float(exact_quotient(n, d))


def round_sqrt(x):
    """sqrt(x) correctly rounded (nearest, ties to even), by the integer square root"""
    M, e = decompose(x)
    if e % 2:
        M, e = 2 * M, e - 1
    Ms = M << 56                      # 108 to 110 bits: a root of 55
    r = math.isqrt(Ms)
    inexact = r * r != Ms
    low, r53 = r & 3, r >> 2
    if low == 3 or (low == 2 and (inexact or r53 & 1)):  # beyond the midpoint, or on it and odd
        r53 += 1
    return math.ldexp(r53, (e - 56) // 2 + 2)


def div_with_rcp_model(n, d, r):
    """egg_div_with_rcp in rational arithmetic: every operation rounded once, the two FMAs as FMAs"""
    q = float(Fraction(n) * Fraction(r))
    rem = float(Fraction(n) - Fraction(d) * Fraction(q))
    return float(Fraction(q) + Fraction(rem) * Fraction(r))


def reciprocals(d):
    """(the correctly rounded 1 / d, the other faithful neighbour: the double on the far side of the exact value)"""
    exact = 1 / Fraction(d)
    r0 = float(exact)
    assert Fraction(r0) != exact  # (d is no power of two)
    r1 = math.nextafter(r0, -math.inf if Fraction(r0) > exact else math.inf)
    return r0, r1
