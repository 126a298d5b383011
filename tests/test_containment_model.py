"""tests/containment_model.py, the definition of yolk containment (egg_set_containment; DESIGN.md section 2.7,
"Containment"), checked on the CPU: off is AdhesionModel bit for bit, hand cases with closed forms, the summation order,
seven wrong rules that each change a named case, and the effect on a yolk under gravity.

A hand case is one batch with imported state in the form of tests/test_pair_census.py: target (0, 0), follow radius 2500 px,
radii 2, every particle at rest, so the first sub-step's containment starts from exactly the spots of the table.  Particles
of one type stay more than 8 px (the collision distance) apart before and after the projection, so the closed forms hold
at the end of the update."""
import functools

import numpy as np
import pytest

import test_pair_census as pc
from adhesion_model import AdhesionMixin, AdhesionModel
from containment_model import LABELS, RULES, ContainmentMixin, ContainmentModel, project, sequential_sum, summary, wsum
from coupling_model import CouplingMixin
from relaxed_model import rm
from test_coupling_model import _run
from wall_model import WallModel

WHITE, YOLK = 0, 1
H60 = 1 / 60
ON, A3, C2 = (2.0, 1.0), (3.0, 1.0), (2.0, 1.0)


class Hand(ContainmentMixin, AdhesionMixin, CouplingMixin, WallModel):
    """the family's most derived member with containment: what tests/test_gpu_containment.py holds the device to"""


# ------------------------------------------------------------------------------------------------ off is off
@pytest.mark.parametrize("containment", [None, (0.0, 1.0), (0.0, 0.25)])
def test_off_is_the_adhesion_model(containment):
    plain = AdhesionModel(relaxed=True)
    plain.set_viscosity(0.5, 1.0)
    plain.set_adhesion(*A3)
    ref = _run(plain, 3, ON)
    m = ContainmentModel(relaxed=True)
    m.set_viscosity(0.5, 1.0)
    m.set_adhesion(*A3)
    if containment:
        m.set_containment(*containment)
    got = _run(m, 3, ON)
    for w in (WHITE, YOLK):
        assert np.array_equal(got[w], ref[w]), w
    assert (m.pair_solves, m.coupling_solves, m.adhesion_solves, m.containment_hits) == \
        (plain.pair_solves, plain.coupling_solves, plain.adhesion_solves, 0)
    assert not hasattr(m, "containment_census")


def test_on_differs_without_coupling_and_exact_order_never_contains():
    plain = ContainmentModel(relaxed=True)
    ref = _run(plain, 3)
    m = ContainmentModel(relaxed=True)
    m.set_containment(0.5, 1.0)  # (tight: half the white's RMS radius)
    got = _run(m, 3)
    assert m.containment_acts() and m.containment_hits > 0 and m.coupling_solves == 0
    assert np.array_equal(got[WHITE], ref[WHITE])  # one-way, and without coupling the types never meet
    assert not np.array_equal(got[YOLK], ref[YOLK])
    exact = ContainmentModel(relaxed=False)
    exact.set_containment(0.5, 1.0)
    _run(exact, 2)
    assert not exact.containment_acts() and exact.containment_hits == 0


# ------------------------------------------------------------------------------------------------ hand cases
def _case(white, yolk, containment, coupling=None, cfg="plain"):
    """white / yolk: per particle, (x, y) or (x, y, "hi") -- "lo" unless said"""
    return dict(spots={WHITE: tuple(white), YOLK: tuple(yolk)}, containment=containment, coupling=coupling, cfg=cfg)


PAIR = [(-8.0, 0.0), (8.0, 0.0)]  # cx = cy = 0, q = 64 twice, rho = 8: L = 8 exactly with factor 1
CASES = {
    "edge": _case(PAIR, [(8.0, 0.0), (0.0, -3.0)], (1.0, 1.0)),
    "rigid": _case(PAIR, [(16.0, 0.0), (0.0, -3.0)], (1.0, 1.0)),
    "soft": _case(PAIR, [(16.0, 0.0), (0.0, -3.0)], (1.0, 0.5)),
    "unequal_masses": _case([(-8.0, 0.0), (8.0, 0.0, "hi")], [(16.0, 0.0), (0.0, -3.0)], (1.0, 1.0)),
    # four whites: q = 64, 64, 25, 25, rho = sqrt(44.5) = 6.67 while the farthest white is 8 px out
    "four_whites": _case(PAIR + [(0.0, -5.0), (0.0, 5.0)], [(7.5, 0.0), (-2.0, 0.0)], (1.0, 1.0)),
    # coupling pushes white 1 and yolk 0 apart (6 px < md = 8) before the disc is taken from the moved white
    "coupled": _case(PAIR, [(14.0, 0.0), (0.0, -3.0)], (1.0, 1.0), coupling=ON),
    # 130 whites on three rings and a second row of lanes: the sums round, and in the stated order
    "rings": _case([(r * np.cos(0.7 * k * k), r * np.sin(0.7 * k * k)) for k, r in
                    ((k, 400.0 + 9.0 * k + (k % 7) / 7.0) for k in range(130))], [(3000.0, 0.0), (0.0, -3.0)], (1.0, 0.5)),
}
WANT = {"edge": {"edge", "inside"}, "rigid": {"hit_rigid", "inside"}, "soft": {"hit_soft", "inside"},
        "unequal_masses": {"hit_rigid", "inside"}, "four_whites": {"hit_rigid", "inside"}, "coupled": {"hit_rigid", "inside"},
        "rings": {"hit_soft", "inside"}}


def hand_run(name, rule=None):
    c = CASES[name]
    w, y = rm.default_configs()
    extra = dict(pc.BASE, **pc.CONFIGS[c["cfg"]])
    cfgs = (dict(w, **extra), dict(y, **extra))
    m = Hand(*cfgs)
    m.containment_rule = rule
    m.set_containment(*c["containment"])
    if c["coupling"]:
        m.set_coupling(*c["coupling"])
    ids = [m.add(*pc.HAND_TARGET, pc.HAND_RADIUS, pc.HAND_RADIUS, len(c["spots"][WHITE]), len(c["spots"][YOLK]))]
    for which, data in ((WHITE, m._white_data), (YOLK, m._yolk_data)):
        cfg = cfgs[which]
        for p, s in enumerate(c["spots"][which]):
            t = 1.0 if len(s) > 2 and s[2] == "hi" else 0.0
            mass = rm.mix(cfg["min_mass"], cfg["max_mass"], t)
            x, y_ = float(s[0]), float(s[1])
            for off, v in ((rm.X, x), (rm.Y, y_), (rm.PX, x), (rm.PY, y_), (rm.LAST_X, x), (rm.LAST_Y, y_), (rm.VX, 0.0), (rm.VY, 0.0),
                           (rm.MASS_T, t), (rm.MASS, mass), (rm.INV_MASS, 1 / mass), (rm.RADIUS, 2.0)):
                data[rm.offset(p + 1) + off] = v
    assert m.update(H60, H60, 1, 1) == 1
    return m, ids


@functools.lru_cache(maxsize=None)
def hand_model(name):
    return hand_run(name)


def outputs(m):
    return [m.state(w) for w in (WHITE, YOLK)], (m.pair_solves, m.coupling_solves, m.containment_hits)


def same_outputs(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and a[1] == b[1]


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_case(name):
    m, _ = hand_model(name)
    assert m.containment_acts()
    assert {k for k, v in m.containment_census.items() if v} == WANT[name], m.containment_census
    assert sum(m.containment_census.values()) == 2  # one label per (yolk particle, sub-step)
    assert m.containment_hits == m.containment_census["hit_rigid"] + m.containment_census["hit_soft"]
    for w in (WHITE, YOLK):
        assert np.isfinite(m.state(w)).all()


def test_closed_forms():
    """two whites at (-8, 0) and (8, 0), factor 1: L == 8 exactly"""
    assert summary([-8.0, 8.0], [0.0, 0.0], 1.0) == (0.0, 0.0, 8.0)
    m, _ = hand_model("edge")  # d == L: not a hit, nothing moves
    assert m.containment_hits == 0 and tuple(m.state(YOLK)[:2, 0]) == (8.0, 0.0)
    m, _ = hand_model("rigid")  # keep = 8 + 0 * 8, s = 1/2
    assert m.containment_hits == 1 and tuple(m.state(YOLK)[:2, 0]) == (8.0, 0.0)
    m, _ = hand_model("soft")  # keep = 8 + 0.5 * 8 = 12, s = 3/4
    assert m.containment_hits == 1 and tuple(m.state(YOLK)[:2, 0]) == (12.0, 0.0)
    m, _ = hand_model("unequal_masses")  # no mass in the rule
    assert m.containment_hits == 1 and tuple(m.state(YOLK)[:2, 0]) == (8.0, 0.0)
    m, _ = hand_model("four_whites")
    L = 1.0 * np.sqrt((((0.0 + 64.0) + 25.0) + (64.0 + 25.0)) / 4.0)  # lanes 0..3, then the butterfly's last two rounds
    assert tuple(m.state(YOLK)[:2, 0]) == (0.0 + 7.5 * (L / 7.5), 0.0)
    for name in CASES:  # one-way: without coupling the white ends where it was put, and the inner yolk particle stays
        if CASES[name]["coupling"] or name == "rings":  # (the rings lie beyond the follow distance: their white moves)
            continue
        m, _ = hand_model(name)
        assert tuple(m.state(YOLK)[:2, 1]) == CASES[name]["spots"][YOLK][1], name
        assert [tuple(v) for v in m.state(WHITE)[:2].T] == [tuple(float(t) for t in s[:2]) for s in CASES[name]["spots"][WHITE]]
    # the projection on its own: a NaN or an empty white never hits
    nan, inf = float("nan"), float("inf")
    nx, ny, hit, _ = project([16.0, nan, 3.0], [0.0, 0.0, nan], 0.0, 0.0, 8.0, 1.0)
    assert hit.tolist() == [True, False, False] and nx[0] == 8.0 and np.isnan(nx[1]) and nx[2] == 3.0
    cx, cy, L = summary([], [], 2.0)
    assert L == inf and not project([1e300], [1e300], cx, cy, L, 1.0)[2].any()
    assert not project([16.0], [0.0], nan, 0.0, nan, 1.0)[2].any()  # a NaN in the white: a NaN centre, no hit


# ------------------------------------------------------------------------------------------------ the summation order
@pytest.mark.parametrize("n", [63, 64, 65, 130])
def test_wsum_is_the_stated_order_and_not_a_sequential_sum(n):
    rng = np.random.default_rng(20261019 + n)
    differ = 0
    for _ in range(20):
        v = rng.uniform(350.0, 450.0, n)
        # the definition, written out lane by lane
        a = [0.0] * 64
        for k in range(n):
            a[k % 64] = a[k % 64] + float(v[k])
        for d in (32, 16, 8, 4, 2, 1):
            a = [a[l] + a[l ^ d] for l in range(64)]
        assert len(set(a)) == 1  # every lane ends with the same bits
        assert wsum(v) == a[0]
        assert abs(wsum(v) - sequential_sum(v)) <= 1e-9 * n  # (both are sums)
        differ += wsum(v) != sequential_sum(v)
    print("n = %d: wsum differs from the sequential sum in %d of 20 draws" % (n, differ))
    assert differ > 0


def test_wsum_of_two_is_the_plain_sum():
    rng = np.random.default_rng(2)
    for _ in range(200):
        v = rng.uniform(350.0, 450.0, 2)
        assert wsum(v) == v[0] + v[1] == sequential_sum(v)
    assert wsum([]) == 0.0 and wsum([-0.0]) == 0.0 and not np.signbit(wsum([-0.0]))


# ------------------------------------------------------------------------------------------------ wrong rules
CAUGHT_BY = {
    "ge": ("edge",),  # (the counter: the position is the same)
    "sequential": ("rings",),
    "both_types": ("rigid", "soft"),
    "mass_weighted": ("unequal_masses",),
    "max_distance": ("four_whites",),
    "before_coupling": ("coupled",),
    "keep_times_strength": ("soft",),
}


def test_every_rule_is_caught():
    assert set(CAUGHT_BY) == set(RULES)


@pytest.mark.parametrize("rule", sorted(CAUGHT_BY))
def test_a_wrong_rule_changes_a_case(rule):
    for name in CAUGHT_BY[rule]:
        right, _ = hand_model(name)
        wrong, _ = hand_run(name, rule)
        assert not same_outputs(outputs(right), outputs(wrong)), (rule, name)
    if rule == "ge":
        assert hand_run("edge", rule)[0].containment_hits == 1 and hand_model("edge")[0].containment_hits == 0


# ------------------------------------------------------------------------------------------------ the effect
@functools.lru_cache(maxsize=None)
def yolk_under_gravity(g, adhesion, containment, steps=30):
    """one default egg, coupling (2, 1), gravity on the yolk alone, (S, C) = (2, 3): the farthest yolk particle's distance
    from the white's centroid at the end, the white's RMS radius, the hits, all finite"""
    m = ContainmentModel(relaxed=True)
    m.set_forces([("uniform", 0.0, g, "yolk")])
    m.add(0.0, 0.0, 50, 15)
    m.set_coupling(*ON)
    if adhesion:
        m.set_adhesion(*adhesion)
    if containment:
        m.set_containment(*containment)
    for _ in range(steps):
        m.update(H60, H60, 2, 3)
    (wx, wy), (yx, yy) = (m.state(w)[:2] for w in (WHITE, YOLK))
    finite = bool(np.isfinite(m.state(WHITE)).all() and np.isfinite(m.state(YOLK)).all())
    cx, cy = wx.mean(), wy.mean()
    far = float(np.hypot(yx - cx, yy - cy).max())
    rms = float(np.sqrt(((wx - cx) ** 2 + (wy - cy) ** 2).mean()))
    return far, rms, m.containment_hits, finite


@pytest.mark.parametrize("g,adhesion", [(60000.0, A3), (20000.0, None)])
def test_containment_keeps_the_yolk_inside_its_white(g, adhesion):
    """the effect: where the adhesion band has been left (or there is none), set_containment(2, 1) keeps the farthest yolk
    particle strictly closer to the white's centroid ("Containment", records the four distances)"""
    without, rms0, none, finite0 = yolk_under_gravity(g, adhesion, None)
    with_, rms1, hits, finite1 = yolk_under_gravity(g, adhesion, C2)
    print("farthest yolk particle from the white's centroid after 30 steps at %g px/s^2, adhesion %s: %.17g px (white RMS radius "
          "%.17g px) without containment, %.17g px (%.17g px) with set_containment(2, 1), %d hits"
          % (g, adhesion, without, rms0, with_, rms1, hits))
    assert finite0 and finite1
    assert none == 0 and hits > 0
    assert with_ < without


def test_every_label_but_no_white_is_reached():
    """`no_white` (a batch without white particles, L = +inf) is part of the rule but cannot arise through add or
    import_batch, which refuse a batch without particles of a type: the model never produces it, and only summary([]) and
    project are checked for it, directly, in test_closed_forms"""
    reached = set().union(*({k for k, v in hand_model(n)[0].containment_census.items() if v} for n in CASES))
    assert reached == set(LABELS) - {"no_white"}
