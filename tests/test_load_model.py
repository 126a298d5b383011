"""tests/load_model.py, the definition of collider loads ("Collider loads"), against what the
definition promises: a hand table of tiny batches whose sums have a closed form and which reaches every kind and every
rule of the bookkeeping (tests/test_gpu_collider_loads.py runs the same table on the device), six wrong rules that each
change a case's sums, loads that only observe -- positions and counters are SpinModel's bit for bit on scenes of every
collider flavour --, the bookkeeping of a step (zeros, a failed step, a new list), and the effect: the floor under a settled
egg carries a share of its weight.  No device needed.

The hand cases use the tiny batch of tests/test_collider_census.py: two particles per type of radius 2, no damping, no
follow constraint, h = 1 / 64.  White particle 0 and yolk particle 1 are under test, at the same spot; their mates rest at
REST, which no collider of the table moves.  With m the mass of a tested particle (1 / its inverse mass), a case lists,
per collider, the reaction (ux, uy, uz) / m of one tested particle: exact binary fractions, so the expected integers are
rint(m * value * scale) per type, added."""
import functools

import numpy as np
import pytest

import test_collider_census as cc
from load_model import IMPULSE_SCALE, TORQUE_SCALE, WRONG, LoadModel, convert, wrap64
from relaxed_model import rm
from spin_model import SpinModel

WHITE, YOLK = 0, 1
H64 = cc.H64
ONE = (H64, H64, 1, 1)
FLOOR = ("half_plane", 0.0, 1.0, -10.0)        # keeps y >= -10 + r = -8
ROLLER = ("disc", 0.0, 0.0, 3.0)
PAN = ("container", 0.0, 20.0, 30.0)           # holds the mates too
BAR = ("segment", 0.0, 0.0, 16.0, 0.0)
FENCE = ("wall", 0.0, -8.0, 0.0, 8.0)
PEG = ("disc", 13.0, -8.0, 2.0)                # beside the spot the floor lifts the particle to
S2 = float.fromhex("0x1.6a09e667f3bcdp-1")      # sqrt(1/2): the way out of a disc's centre for key 1
HEAVY, HUGE = 9.0e7, 1.0e30                    # 1 / HEAVY > eps = 1e-8 > 1 / HUGE


def _case(colliders, prev, vel=(0.0, 0.0), surfaces=None, motions=None, spins=None, mass=(None, None), want=None, dropped=0,
          types=(WHITE, YOLK), per_type=None):
    return dict(colliders=list(colliders), prev=prev, vel=vel, surfaces=surfaces, motions=motions, spins=spins, mass=mass, want=want,
                dropped=dropped, types=types, per_type=per_type)


# name: the list, the tested particles' start (and velocity), and `want`: per collider the (ux, uy, uz) / m of ONE tested
# particle (None: nothing touches that collider); `types`: the types that contribute; `per_type`: want per type where the two
# differ (the way out of a disc's centre goes by the particle's key)
CASES = {
    # at rest 1 px inside the floor: lifted from (16, -9) to (16, -8); about the origin the lever is x = 16
    "half_plane": _case([FLOOR], (16.0, -9.0), want=[(0.0, -1.0, -16.0)]),
    # half a px inside the disc, straight above its centre: out at (0, 5)
    "disc": _case([ROLLER], (0.0, 4.5), want=[(0.0, -0.5, 0.0)]),
    # at the centre itself, d2 == 0: out along the direction of the particle's key, to (5, 0) and to (5 S2, 5 S2); the
    # reaction goes through the centre, which is the origin: no moment (for key 1 the difference of two equal products)
    "disc_centre": _case([ROLLER], (0.0, 0.0), per_type={WHITE: [(-5.0, 0.0, 0.0)], YOLK: [(-(S2 * 5.0), -(S2 * 5.0), 0.0)]}),
    # 1 px outside the container's inner radius 28: back to (28, 20)
    "container": _case([PAN], (29.0, 20.0), want=[(1.0, 0.0, -20.0)]),
    # 1.5 px above the bar: out at (8, 2)
    "segment": _case([BAR], (8.0, 1.5), want=[(0.0, -0.5, -4.0)]),
    # through the fence from the left, 2 px in one sub-step: back to x = -2 from x = 1 (a catch)
    "wall_caught": _case([FENCE], (-1.0, 0.0), vel=(128.0, 0.0), want=[(3.0, 0.0, 0.0)]),
    # at rest 1 px right of the fence: out at x = 2 (a hit, no catch)
    "wall_not_caught": _case([FENCE], (1.0, 0.0), want=[(-1.0, 0.0, 0.0)]),
    # 1 px a sub-step along the floor, 1 px inside it: mu = 8 sticks (the whole px is taken back), mu = 0.5 slides (half of it)
    "stick": _case([FLOOR], (16.0, -9.0), vel=(64.0, 0.0), surfaces=[8.0], want=[(1.0, -1.0, -16.0 + 8.0)]),
    "slide": _case([FLOOR], (16.0, -9.0), vel=(64.0, 0.0), surfaces=[0.5], want=[(0.5, -1.0, -16.5 + 4.0)]),
    "smooth": _case([FLOOR], (16.0, -9.0), vel=(64.0, 0.0), want=[(0.0, -1.0, -17.0)]),
    # the floor rises 1 px in the sub-step: it keeps y >= -7 at its end
    "moving": _case([FLOOR], (16.0, -8.5), motions=[(0.0, 64.0)], want=[(0.0, -1.5, -24.0)]),
    # the roller of tests/test_spin_model.py: spins at 16 rad/s, sticks: from (0, 4.5) to (-1.25, 5), about its centre
    "turning": _case([ROLLER], (0.0, 4.5), surfaces=[8.0], spins=[(0.0, 0.0, 16.0)], want=[(1.25, -0.5, 0.625 - 6.25)]),
    # a pivot that turns nothing still is the point the torque is about: the lever is 16 - 10
    "pivot_at_rest": _case([FLOOR], (16.0, -9.0), spins=[(10.0, -10.0, 0.0)], want=[(0.0, -1.0, -6.0)]),
    # ... and it rides on the motion: 1 px along the floor in the sub-step, which leaves the floor where it is
    "pivot_rides": _case([FLOOR], (16.0, -9.0), motions=[(64.0, 0.0)], spins=[(10.0, -10.0, 0.0)], want=[(0.0, -1.0, -5.0)]),
    # the yolk is too heavy to be moved by anything but a collider: it is projected, and contributes nothing
    "immovable": _case([FLOOR], (16.0, -9.0), mass=(None, HUGE), want=[(0.0, -1.0, -16.0)], types=(WHITE,)),
    "white_only": _case([FLOOR + ("white",)], (16.0, -9.0), want=[(0.0, -1.0, -16.0)], types=(WHITE,)),
    # the floor lifts it to (16, -8), where the peg reaches it and pushes it to (17, -8): in list order, each on the result of
    # the one before (the other way round the peg would meet it at (16, -9))
    "two_in_one_pass": _case([FLOOR, PEG], (16.0, -9.0), want=[(0.0, -1.0, -16.0), (-1.0, 0.0, -8.0)]),
    "nothing_touched": _case([FLOOR, PEG], (40.0, 0.0), want=[None, None]),
    # 202 px inside the floor with a mass of 9e7: 202 * 9e7 * 2^20 is beyond 2^53, so both contributions are dropped whole
    "dropped": _case([FLOOR], (16.0, -210.0), mass=(HEAVY, HEAVY), want=[None], dropped=2),
    # ... and 1 px inside it the same mass is counted
    "heavy": _case([FLOOR], (16.0, -9.0), mass=(HEAVY, HEAVY), want=[(0.0, -1.0, -16.0)]),
}


def hand_configs(name):
    w, y = cc.hand_configs()
    for cfg, mass in zip((w, y), CASES[name]["mass"]):
        if mass is not None:
            cfg.update(min_mass=mass, max_mass=mass)
    return w, y


def hand_spots(name):
    c = CASES[name]
    tested, rest = (c["prev"], c["vel"]), (cc.REST, (0.0, 0.0))
    return {w: [tested if p == cc.TESTED[w] else rest for p in (0, 1)] for w in (WHITE, YOLK)}


def hand_configure(o, name, loads=True):
    """the case's list on a model or a handle"""
    c = CASES[name]
    o.set_colliders(c["colliders"])
    if c["surfaces"] is not None:
        o.set_collider_surfaces(c["surfaces"])
    if c["motions"] is not None:
        o.set_collider_motion(c["motions"])
    if c["spins"] is not None:
        o.set_collider_spin(c["spins"])
    o.set_collider_loads(loads)


def hand_run(name, wrong=None, loads=True):
    m = LoadModel(*hand_configs(name), wrong=wrong)
    hand_configure(m, name, loads)
    i = m.add(*cc.HAND_TARGET, cc.HAND_RADIUS, cc.HAND_RADIUS, 2, 2)
    for w, data in ((WHITE, m._white_data), (YOLK, m._yolk_data)):
        for p, ((x, y), (vx, vy)) in enumerate(hand_spots(name)[w]):
            for off, v in ((rm.X, x), (rm.Y, y), (rm.LAST_X, x), (rm.LAST_Y, y), (rm.VX, vx), (rm.VY, vy)):
                data[rm.offset(p + 1) + off] = v
    assert m.update(*ONE) == 1
    return m, i


@functools.lru_cache(maxsize=None)
def hand_model(name):
    return hand_run(name)


def hand_expected(name, m):
    """the case's sums from its closed form and the masses the model holds"""
    c = CASES[name]
    sums = [[0, 0, 0] for _ in c["colliders"]]
    for w in c["types"]:
        mass = 1.0 / float(m.field(w, rm.INV_MASS)[cc.TESTED[w]])
        want = c["per_type"][w] if c["per_type"] else c["want"]
        for k, u in enumerate(want):
            if u is None:
                continue
            for q, scale in enumerate((IMPULSE_SCALE, IMPULSE_SCALE, TORQUE_SCALE)):
                sums[k][q] += int(np.rint((mass * u[q]) * scale))
    return [tuple(s) for s in sums]


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_case(name):
    m, _ = hand_model(name)
    c = CASES[name]
    sums, dropped, h = m.collider_load_sums()
    assert h == H64 and dropped == c["dropped"], (name, dropped)
    assert sums == hand_expected(name, m), (name, sums, hand_expected(name, m))
    for w in (WHITE, YOLK):  # the mates rest where they were: nothing of the table touches them
        assert tuple(m.state(w)[:2, 1 - cc.TESTED[w]]) == cc.REST, (name, w)
    want = c["per_type"][WHITE] if c["per_type"] else c["want"]
    for k, u in enumerate(want):
        if u is None:
            assert sums[k] == (0, 0, 0)  # exactly: a collider nothing touches
    assert m.collider_loads() == convert(sums, H64)
    mass_w = 1.0 / float(m.field(WHITE, rm.INV_MASS)[0])
    if name == "half_plane":  # once by hand, all the way: both types, two divisions
        mass_y = 1.0 / float(m.field(YOLK, rm.INV_MASS)[1])
        sy = int(np.rint(-mass_w * 2.0 ** 20)) + int(np.rint(-mass_y * 2.0 ** 20))
        assert m.collider_loads()[0][:2] == (0.0, (float(sy) / 2.0 ** 20) / H64)


def test_the_table_reaches_what_it_is_for():
    kinds = {c[0] for case in CASES.values() for c in case["colliders"]}
    assert kinds == {"half_plane", "disc", "container", "segment", "wall"}
    assert hand_model("wall_caught")[0].wall_catches == [1, 1] and hand_model("wall_not_caught")[0].wall_catches == [0, 0]
    assert hand_model("wall_not_caught")[0].collider_hits == [1, 1]
    assert hand_model("stick")[0].grip_sticks == [1, 1] and hand_model("slide")[0].grip_sticks == [0, 0]
    assert hand_model("slide")[0].collider_grips == [1, 1] and hand_model("smooth")[0].collider_grips == [0, 0]
    assert hand_model("turning")[0].turning() and hand_model("moving")[0].moving()
    assert not hand_model("pivot_at_rest")[0].turning() and hand_model("pivot_at_rest")[0].spins
    assert not hand_model("half_plane")[0].spins
    m = hand_model("immovable")[0]
    assert not float(m.field(YOLK, rm.INV_MASS)[1]) > rm.EPS and m.collider_hits == [1, 1]  # (projected all the same)
    assert hand_model("white_only")[0].collider_hits == [1, 0]
    assert hand_model("two_in_one_pass")[0].collider_hits == [2, 2]
    assert hand_model("nothing_touched")[0].collider_hits == [0, 0]
    assert hand_model("dropped")[0].load_contributions == 0 and hand_model("heavy")[0].load_contributions == 2
    assert float(hand_model("heavy")[0].field(WHITE, rm.INV_MASS)[0]) > rm.EPS


# ---- the wrong rules
CHANGED_BY = {
    "sign": ("half_plane", "turning"),
    "grip_left_out": ("stick", "slide", "turning"),
    "pivot_unmoved": ("pivot_rides",),
    "immovable_counted": ("immovable",),
    "scale_after_sum": (),  # (no case is named: rint(a) + rint(b) differs from rint(a + b) wherever the fractions say so)
    "about_before": ("half_plane", "turning"),
}


def test_every_wrong_rule_is_named():
    assert set(CHANGED_BY) == set(WRONG)


@pytest.mark.parametrize("wrong", WRONG)
def test_a_wrong_rule_changes_a_case(wrong):
    if wrong == "scale_after_sum":  # both types add into one sum: scaled once, the two halves round together in some case
        changed = [n for n in sorted(CASES) if hand_run(n, wrong=wrong)[0].collider_load_sums()[0] != hand_model(n)[0].collider_load_sums()[0]]
        print("scale_after_sum changes", changed)
        assert changed
    for name in CHANGED_BY[wrong]:
        right, _ = hand_model(name)
        other, _ = hand_run(name, wrong=wrong)
        # (the sums or the dropped count: an immovable particle's mass is so large that its contribution, once counted, is dropped)
        assert other.collider_load_sums()[:2] != right.collider_load_sums()[:2], (wrong, name)
        for w in (WHITE, YOLK):  # (the positions are the same: the rule only observes)
            assert np.array_equal(other.state(w), right.state(w), equal_nan=True)
    # every other case of the table that the wrong rule does not concern stays as it is
    if wrong in ("pivot_unmoved", "immovable_counted"):
        assert hand_run("half_plane", wrong=wrong)[0].collider_load_sums() == hand_model("half_plane")[0].collider_load_sums()


# ---- loads only observe: scenes of every collider flavour, shared with tests/test_gpu_collider_loads.py
S, C = 2, 3
H60 = 1 / 60
EDGE = ("half_plane", 1.0, 0.0, 262.0)
BALL = ("disc", 330.0, 300.0, 20.0)
RING = ("container", 300.0, 300.0, 62.0)
RAIL = ("segment", 250.0, 345.0, 350.0, 340.0)
GATE = ("wall", 100.0, 352.0, 500.0, 346.0)
LIST = (EDGE, BALL, RING, RAIL)
ROUGH = ((0.3, -15.0, 0.0), 0.2, None, (0.5, 20.0, 0.0))
GRAVITY = (("uniform", 0.0, 400.0),)
# name: (colliders, surfaces, motions, spins, forces, steps)
FLAVOURS = {
    "col": (LIST, None, None, None, GRAVITY, 3),
    "srf": (LIST, ROUGH, None, None, GRAVITY, 3),
    "wall": (LIST + (GATE,), ROUGH + (0.4,), None, None, GRAVITY, 4),
    "mov": (LIST + (GATE,), ROUGH + (0.4,), ((30.0, 0.0), (-60.0, 12.0), None, (0.0, -45.0), (0.0, -90.0)), None, GRAVITY, 4),
    "mov_pivots": (LIST + (GATE,), ROUGH + (0.4,), ((30.0, 0.0), (-60.0, 12.0), None, (0.0, -45.0), (0.0, -90.0)),
                   ((262.0, 300.0, 0.0), None, (300.0, 300.0, -0.0), (300.0, 342.0, 0.0), None), GRAVITY, 3),
    "spin": (LIST + (GATE,), ROUGH + (0.4,), ((30.0, 0.0), (-60.0, 12.0), None, (0.0, -45.0), (0.0, -90.0)),
             ((262.0, 300.0, 0.2), (300.0, 300.0, -3.0), None, (300.0, 342.0, 0.5), (300.0, 349.0, -0.4)), GRAVITY, 4),
}


def flavour_configure(o, name, cohesion=False, loads=True):
    """a model, SimulationHandler, SimulationGroup or ShardedSimulationHandler set up for the scene"""
    colliders, surfaces, motions, spins, forces, _ = FLAVOURS[name]
    if not isinstance(o, SpinModel):
        o.set_solver_order("relaxed")
        if cohesion:
            from test_gpu_collider_walls import CONFIGS
            o.set_white_config(CONFIGS["cohesion"]["white"])
            o.set_cohesion("effective")
    o.set_colliders(list(colliders))
    o.set_forces(list(forces))
    if surfaces is not None:
        o.set_collider_surfaces(list(surfaces))
    if motions is not None:
        o.set_collider_motion(list(motions))
    if spins is not None:
        o.set_collider_spin(list(spins))
    if loads is not None:
        o.set_collider_loads(loads)
    return o


def flavour_model(cohesion, cls=LoadModel):
    from test_gpu_collider_walls import CONFIGS
    w, y = rm.default_configs()
    return cls(dict(w, **CONFIGS["cohesion" if cohesion else "default"]["white"]), y, cohesion=cohesion)


def _snap(m):
    return dict(state=[m.state(w) for w in (WHITE, YOLK)], pairs=m.pair_solves, cohered=m.cohesion_solves, hits=list(m.collider_hits),
                grips=list(m.collider_grips), sticks=list(m.grip_sticks), catches=list(m.wall_catches), colliders=m.get_colliders(),
                spins=m.get_collider_spin())


@functools.lru_cache(maxsize=None)
def flavour_run(name, cohesion=False, centers=((300.0, 300.0),)):
    """the scene on LoadModel with loads on, once: after every step the snapshot and the loads; shared, never changed"""
    from test_gpu_collider_surfaces import _snapshot
    m = flavour_configure(flavour_model(cohesion), name)
    ids = [m.add(x, y, 50, 15) for x, y in centers]
    out = []
    for _ in range(FLAVOURS[name][5]):
        m.update(H60, H60, S, C)
        out.append(dict(_snap(m), sums=m.collider_load_sums(), loads=m.collider_loads(), snapshot=_snapshot(m, ids)))
    return dict(ids=ids, steps=out, kept=m.load_contributions)


@pytest.mark.parametrize("name", sorted(FLAVOURS))
def test_loads_only_observe(name):
    """SpinModel, which knows no loads, and LoadModel with loads off give LoadModel's positions and counters with loads on"""
    ref = flavour_run(name, name == "spin")
    assert ref["kept"] > 0
    for cls, loads in ((SpinModel, None), (LoadModel, False)):
        m = flavour_configure(flavour_model(name == "spin", cls), name, loads=loads)
        m.add(300.0, 300.0, 50, 15)
        for k in range(FLAVOURS[name][5]):
            m.update(H60, H60, S, C)
            got, want = _snap(m), ref["steps"][k]
            for w in (WHITE, YOLK):
                assert np.array_equal(got["state"][w], want["state"][w]), (name, cls.__name__, k, w)
            assert {q: got[q] for q in got if q != "state"} == {q: want[q] for q in want if q not in ("state", "sums", "loads", "snapshot")}
        if cls is LoadModel:
            assert m.collider_load_sums() == ([(0, 0, 0)] * len(FLAVOURS[name][0]), 0, 0.0)
    last = ref["steps"][-1]
    assert min(last["hits"]) > 0 and np.isfinite(last["state"][WHITE]).all()
    assert any(s != (0, 0, 0) for s in last["sums"][0]) and last["sums"][2] == H60 / S


def test_the_hand_cases_only_observe_too():
    for name in sorted(CASES):
        on, off = hand_model(name)[0], hand_run(name, loads=False)[0]
        for w in (WHITE, YOLK):
            assert np.array_equal(on.state(w), off.state(w), equal_nan=True), name
        assert (on.collider_hits, on.collider_grips, on.wall_catches) == (off.collider_hits, off.collider_grips, off.wall_catches)
        assert off.collider_load_sums() == ([(0, 0, 0)] * len(CASES[name]["colliders"]), 0, 0.0)


# ---- the bookkeeping of a step
def test_the_sums_cover_one_step_and_a_failed_step_keeps_them():
    m = flavour_configure(flavour_model(False), "col")
    m.add(300.0, 300.0, 50, 15)
    m.update(H60, H60, S, C)
    first = m.collider_load_sums()
    assert first == flavour_run("col")["steps"][0]["sums"] and first[0][1] != (0, 0, 0)
    m.update(H60, H60, S, C)
    second = m.collider_load_sums()
    assert second == flavour_run("col")["steps"][1]["sums"] != first  # (one step's, not the running total)

    def fails(*a, **k):
        raise FloatingPointError("a step that fails half way")

    held, m._post_solve = m._post_solve, fails
    with pytest.raises(FloatingPointError):
        m.update(H60, H60, S, C)
    m._post_solve = held
    assert m.collider_load_sums() == second
    # setting the list zeroes them and keeps the switch; so does the switch itself
    m.set_colliders([BALL])
    assert m.collider_load_sums() == ([(0, 0, 0)], 0, 0.0) and m.get_collider_loads_enabled()
    assert m.collider_loads() == [(0.0, 0.0, 0.0)]
    m.update(H60, H60, S, C)
    assert m.collider_load_sums()[0] != [(0, 0, 0)]
    m.set_collider_loads(True)
    assert m.collider_load_sums() == ([(0, 0, 0)], 0, 0.0)
    # off, exact order, an empty list: accepted, and nothing is recorded
    m.set_collider_loads(False)
    m.update(H60, H60, S, C)
    assert m.collider_load_sums() == ([(0, 0, 0)], 0, 0.0)
    e = LoadModel(relaxed=False)
    e.set_collider_loads(True)
    e.add(300.0, 300.0, 50, 15)
    e.update(H60, H60, S, C)
    assert e.collider_load_sums() == ([], 0, 0.0) and e.collider_loads() == []


def test_wrap64_is_twos_complement():
    assert wrap64(2 ** 63 - 1) == 2 ** 63 - 1 and wrap64(2 ** 63) == -2 ** 63 and wrap64(-2 ** 63 - 1) == 2 ** 63 - 1 and wrap64(-5) == -5


# ---- the effect: an egg on a floor
GROUND = ("half_plane", 0.0, -1.0, -364.0)  # keeps y <= 364 - r = 360 (y grows downwards): 8 px below the egg while its
G = 980.0                                   # target is at y = 300; after HOVER steps the target goes down by 30 px
HOVER, SETTLE = 5, 120


@functools.lru_cache(maxsize=None)
def settled():
    m = LoadModel()
    m.set_colliders([GROUND])
    m.set_forces([("uniform", 0.0, G)])
    m.set_collider_loads(True)
    i = m.add(300.0, 300.0, 50, 15)
    series = []
    for k in range(SETTLE):
        if k == HOVER:
            m.set_target_position(i, 300.0, 330.0)
        m.update(H60, H60, S, C)
        series.append((m.collider_loads()[0], sum(m.collider_hits)))
    mass = sum(float(np.sum(1.0 / np.asarray(m.field(w, rm.INV_MASS), dtype=np.float64))) for w in (WHITE, YOLK))
    return m, series, mass


def test_the_floor_under_an_egg_carries_weight_in_the_direction_of_gravity():
    m, series, mass = settled()
    # before anything touches the floor every load is exactly zero
    first_touch = next(k for k, (_, hits) in enumerate(series) if hits > 0)
    assert first_touch >= HOVER and all(series[k][0] == (0.0, 0.0, 0.0) for k in range(first_touch))
    # settled: the mean force on the floor over a step, j / delta, points the way gravity does (+y)
    tail = [series[k][0][1] / H60 for k in range(SETTLE - 30, SETTLE)]
    assert all(f > 0.0 for f in tail)
    share = float(np.mean(tail)) / (mass * G)
    print("floor load after %d steps: mean jy / delta over the last 30 = %.6g, total mass %.6g, share of m g = %.4f" %
          (SETTLE, float(np.mean(tail)), mass, share))
    assert m.collider_load_sums()[1] == 0
