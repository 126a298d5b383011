"""Touches on the device (egg_touches / egg_touches_of / egg_group_touches; include/eggsim_touch.h)
against tests/touch_model.py, evaluated on the handle's own downloads.  Every comparison is ==: every output is an integer.
Scenes are built through _scene of test_gpu_probes.py."""
import ctypes as C

import numpy as np
import pytest

import test_touch_model as tt
import touch_model as tm
from conftest import ROOT
from test_gpu_probes import EGGS, _relaxed_scene, _scene

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
FIELDS = ("x", "y", "vx", "vy", "last_x", "last_y")
H60, S, CS = 1 / 60, 2, 3
INF = float("inf")
MASKS = {"white": 1, "yolk": 2, "both": 3}


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _keyed(batches):
    """the batches as _scene takes them; a batch is imported with at least one particle of each type, so where a scene has none
    the batch gets a filler far from everything, 1,000 from the next one: it touches nothing at any reach used here"""
    def some(spots, k):
        return spots if spots else [(1.0e6 + 1000.0 * k, 1.0e6, 0.25)]
    return [dict(key=k + 1, white=some(b["white"], k), yolk=some(b["yolk"], k)) for k, b in enumerate(batches)]


def _parts(h):
    return tuple(dict(x=h.download(w, "x"), y=h.download(w, "y"), radius=h.download(w, "radius"), batch_id=h.download(w, "batch_id"))
                 for w in (WHITE, YOLK))


def _reach_of(h, reach):
    if reach is None:
        return (float(h._white_config["collision_overlap_factor"]), float(h._yolk_config["collision_overlap_factor"]))
    return tuple(reach) if isinstance(reach, (tuple, list)) else (reach, reach)


def _want(h, ids, reach=None, types="both", parts=None):
    ids = h.list_ids() if ids is None else ids
    return tm.touches(parts or _parts(h), ids, _reach_of(h, reach), MASKS[types])


def _rows(table):
    return [tuple(r) for r in np.asarray(table).reshape(-1, 8).tolist()]


def _assert_touches(h, ids, reach=None, types="both", what="", parts=None):
    """h.touch_table is the model's answer over h's own downloads; returns it"""
    want = _want(h, ids, reach, types, parts)
    got = h.touch_table(ids, reach, types)
    print("%s: %d records, first %s" % (what, len(want), want[:2]))
    assert got.dtype == np.int64 and got.shape == (len(want), 8)
    assert _rows(got) == want, what
    return want


def _lists(want, n):
    """what touches() makes of the model's records"""
    res = [([], []) for _ in range(n)]
    for rec in want:
        point = tm.contact(rec)
        res[rec[0]][rec[1]].append((rec[2], rec[3], rec[4], rec[5]) + (point if point else (None, None)))
    return res


# ------------------------------------------------------------------------------------------------ the hand table
@pytest.mark.parametrize("name", sorted(tt.CASES))
def test_hand_case(egg, name):
    case = tt.CASES[name]
    h, ids = _scene(egg, _keyed(case["batches"]))
    assert ids == list(range(1, len(ids) + 1))
    types = {1: "white", 2: "yolk", 3: "both"}[case["mask"]]
    assert _rows(h.touch_table(case["ids"], case["reach"], types)) == case["want"]
    back = case["ids"][::-1]
    assert _assert_touches(h, back, case["reach"], types, name + " reversed") == \
        sorted(((len(back) - 1 - r[0],) + r[1:] for r in case["want"]), key=lambda r: r[:3])
    got = h.touches(case["ids"], case["reach"], types)
    assert [tuple([tuple(t) for t in side] for side in pair) for pair in got] == [tuple(pair) for pair in _lists(case["want"], len(case["ids"]))]
    for pair in got:
        for side in pair:
            for t in side:
                assert t._fields == ("other", "pairs", "particles", "dropped", "x", "y") and type(t.other) is int
    for a in ids:
        others = sorted({r[2] for r in _want(h, [a], case["reach"], types)})
        assert h.touching(a, None, case["reach"], types) == others
        assert [h.touching(a, b, case["reach"], types) for b in ids] == [b in others for b in ids]


# ------------------------------------------------------------------------------------------------ the seams of the kernel
def _line(n, x0=100.0):
    """n particles of radius 1 on a line, 3 apart: none touches another"""
    return [(x0 + 3.0 * i, 0.0, 1.0) for i in range(n)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_other_atom_sizes_on_every_seam(egg, n):
    """the other atom has n particles (2,049: three units, whose partial records must merge); one-particle batches each touch
    exactly ONE of them, at index 0, 63, 64 and the last one; one touches none of them and one huge disc touches all"""
    spots = sorted({i for i in (0, 63, 64, n - 1) if i < n})
    batches = [tt._b(_line(n))] + [tt._b([(100.0 + 3.0 * i, 1.5, 0.6)]) for i in spots]
    batches += [tt._b([(100.0 + 1.5 * n, 50.0, 0.6)]), tt._b([(100.0 + 1.5 * n, 0.0, 100000.0)])]
    h, ids = _scene(egg, _keyed(batches))
    parts = _parts(h)
    want = _assert_touches(h, None, 1.0, "white", "n = %d" % n, parts)
    by = {(ids[r[0]], r[2]): r for r in want}
    for k, i in enumerate(spots):
        assert by[(ids[1 + k], ids[0])][3:6] == (1, 1, 0) and by[(ids[0], ids[1 + k])][3:6] == (1, 1, 0)
        assert by[(ids[1 + k], ids[0])][6] == int(np.rint((100.0 + 3.0 * i) * 65536.0)) * 2
    assert [r[2] for r in want if r[0] == len(ids) - 2] == [ids[-1]]  # (the lonely one touches the huge disc alone)
    assert by[(ids[-1], ids[0])][3:6] == (n, n, 0) and by[(ids[0], ids[-1])][3:6] == (n, 1, 0)
    assert _assert_touches(h, [ids[-1], ids[0], ids[-1]], 1.0, "both", "listed", parts)


@pytest.mark.parametrize("m", [1, 64, 65, 1025])
def test_query_atom_sizes(egg, m):
    """the QUERY atom has m particles; another batch touches its first, its last and (from 3 on) a middle one"""
    spots = sorted({0, m // 2, m - 1})
    h, ids = _scene(egg, _keyed([tt._b(_line(m), _line(2, 0.0)), tt._b([(100.0 + 3.0 * i, 1.5, 0.6) for i in spots], [(1.0, 0.5, 0.5)])]))
    parts = _parts(h)
    want = _assert_touches(h, [ids[0]], 1.0, "both", "m = %d" % m, parts)
    assert [r[:6] for r in want] == [(0, 0, ids[1], len(spots), len(spots), 0), (0, 1, ids[1], 1, 1, 0)]
    assert _assert_touches(h, [ids[1], ids[0]], 1.0, "both", "both ways", parts)


@pytest.fixture(scope="module")
def chain(egg):
    """129 one-particle batches in a row, each touching its neighbours"""
    h, ids = _scene(egg, _keyed([tt._b([(2.0 * k, 0.0, 1.0)], [(2.0 * k, 5.0, 1.0)]) for k in range(129)]))
    return h, ids, _parts(h)


@pytest.mark.parametrize("length", [1, 63, 64, 65, 129])
def test_query_list_lengths(chain, length):
    """the rounds of one lane per query: 2 queries per id and type, so 64 queries are 32 ids of both types or 64 of one"""
    h, ids, parts = chain
    order = np.random.default_rng(length).permutation(len(ids)).tolist()
    listed = [ids[order[k % len(order)]] for k in range(length)]
    for types in ("white", "both"):
        want = _assert_touches(h, listed, 1.0, types, "%d ids, %s" % (length, types), parts)
        assert len(want) >= length * (1 if types == "white" else 2)
    if length == 129:
        assert len(_assert_touches(h, None, 1.0, "both", "every batch", parts)) == 2 * (2 * 129 - 2)


# ------------------------------------------------------------------------------------------------ the record buffer
def _raw(h, spec, ids, cap, out):
    n = C.c_int64(-7)
    arr = None if ids is None else np.ascontiguousarray(ids, dtype=np.int64)
    rc = h._lib.egg_touches(h._h, None if spec is None else C.byref(spec), 0 if ids is None else arr.size, None if ids is None else arr.ctypes.data,
                            cap, None if out is None else out.ctypes.data, C.byref(n))
    return rc, n.value


def test_more_records_than_the_first_buffer(egg):
    """one large disc and 300 one-particle batches inside its reach: 300 records, beyond EGG_TC_FIRST_RECORDS = 256.  The
    first call runs its launches twice, the second once: the buffer belongs to the handle."""
    from egg_fluid_simulation_amd import _ffi
    small = [tt._b([(3.0 * (k % 20), 3.0 * (k // 20), 1.0)]) for k in range(300)]
    h, ids = _scene(egg, _keyed([tt._b([(30.0, 22.0, 100.0)])] + small))
    spec = _ffi.EggTouchSpec((C.c_double * 2)(1.0, 1.0), 1, 0)
    want = _want(h, [ids[0]], 1.0, "white")
    assert len(want) == 300 and len(want) > 256
    out = np.zeros(400, dtype=[("slot", "<i4"), ("pairs", "<i4"), ("particles", "<i4"), ("dropped", "<i4"), ("other", "<i8"), ("sx", "<i8"), ("sy", "<i8")])
    launches = []
    for _ in range(2):
        before = h.stats()["kernel_launches"]
        assert _raw(h, spec, [ids[0]], 400, out) == (0, 300)
        launches.append(h.stats()["kernel_launches"] - before)
        assert [(0, 0, int(r["other"]), int(r["pairs"]), int(r["particles"]), int(r["dropped"]), int(r["sx"]), int(r["sy"])) for r in out[:300]] == want
    print("launches", launches)
    assert launches == [4, 2]  # (one round of two launches, run twice by the call that found the buffer short)
    assert _rows(h.touch_table([ids[0]], 1.0, "white")) == want  # (the Python twin asks again with the size the call named)
    assert _assert_touches(h, ids[:70], 1.0, "white", "70 queries against 301 batches")


# ------------------------------------------------------------------------------------------------ the cull
def test_pairs_on_the_boundary_at_the_edges_of_their_boxes(egg):
    """d2 == L * L exactly, the two particles at the facing edges (axis-aligned) and corners (diagonal) of their units' boxes"""
    left = [(0.0, 0.0, 4.0), (-30.0, -1.0, 1.0), (-20.0, -30.0, 0.5), (-5.0, -5.0, 1.0)]
    right = [(8.0, 0.0, 4.0), (40.0, 3.0, 1.0), (30.0, 30.0, 0.5), (20.0, 1.0, 1.0)]
    low = [(0.0, 0.0, 2.0), (-30.0, -1.0, 1.0), (-20.0, -30.0, 0.5), (-6.0, -5.0, 1.0)]
    high = [(3.0, 4.0, 3.0), (40.0, 5.0, 1.0), (30.0, 30.0, 0.5), (20.0, 14.0, 1.0)]
    for a, b, what in ((left, right, "axis-aligned"), (low, high, "diagonal")):
        h, ids = _scene(egg, _keyed([tt._b(a, [(500.0, 500.0, 1.0)]), tt._b(b, [(900.0, 500.0, 1.0)])]))
        want = _assert_touches(h, None, 1.0, "both", what)
        assert [r[:6] for r in want] == [(0, 0, ids[1], 1, 1, 0), (1, 0, ids[0], 1, 1, 0)], what
        assert _assert_touches(h, None, 0.999999, "both", what + ", a shade less") == []


@pytest.mark.parametrize("seed", [11, 12])
def test_randomised_scenes(egg, seed):
    """a few dozen batches of up to 200 particles, mixed radii, every reach: the cull skips nothing the rule accepts"""
    h, ids = _scene(egg, _keyed(tt.random_scene(seed, n_batches=30, most=200, spread=120.0)))
    parts = _parts(h)
    counts = []
    for reach in (0.5, 1.0, 1.1, 3.0):
        counts.append(len(_assert_touches(h, None, reach, "both", "seed %d, reach %g" % (seed, reach), parts)))
    assert 0 < counts[0] < counts[-1] < 2 * 30 * 29  # (some touch, not all)
    assert _assert_touches(h, ids[::3], (1.1, 0.5), "both", "a reach per type", parts)


# ------------------------------------------------------------------------------------------------ a real scene
@pytest.mark.parametrize("order", ["relaxed", "exact"])
def test_four_eggs_after_five_steps(egg, order):
    h = egg.SimulationHandler()
    if order == "relaxed":
        _relaxed_scene(h)
    ids = [h.add(x, y) for x, y in EGGS]
    for _ in range(5):
        assert h.update(H60, H60, S, CS) == 1
    parts = _parts(h)
    for types in ("white", "yolk", "both"):
        want = _assert_touches(h, None, None, types, "%s, %s" % (order, types), parts)
        assert (types == "yolk") or any(r[1] == WHITE for r in want)
    assert h.touching(ids[0], ids[1]) and ids[1] in h.touching(ids[0])


# ------------------------------------------------------------------------------------------------ touches_of
def test_touches_of_a_batchs_own_discs(egg):
    h, ids = _scene(egg, _keyed(tt.random_scene(5, n_batches=10, most=60, spread=40.0)))
    parts = _parts(h)
    labelled = tm.labelled(parts)
    for i in ids[:4]:
        _info, ws, ys = h.export_batch(i)
        discs = (ws[[0, 1, 7]].T, ys[[0, 1, 7]].T)
        rows = h.touches([i], 1.1)[0]
        assert h.touches_of(discs, 1.1, "both", key=i) == rows
        assert h.touches_of(discs[0], 1.1, "white", key=i) == (rows[0], []) and h.touches_of(discs[1], 1.1, "yolk", key=i) == ([], rows[1])
        # without a key the batch itself is among the answers
        want = tm.records_of([(-1, 0) + tuple(discs[0].T), (-1, 1) + tuple(discs[1].T)], labelled, (1.1, 1.1))
        got = h.touches_of(discs, 1.1, "both")
        assert [[t[:4] for t in side] for side in got] == [[r[2:6] for r in want if r[1] == w] for w in (0, 1)]
        assert any(t.other == i for t in got[0] + got[1])
    assert h.touches_of(np.zeros((0, 3))) == ([], [])
    with pytest.raises(egg.EggError, match="a radius is not finite"):
        h.touches_of([(0.0, 0.0, INF)])


# ------------------------------------------------------------------------------------------------ around a step
def _state(h):
    return [h.download(w, f) for w in (WHITE, YOLK) for f in FIELDS]


def _same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a, b))


def test_calls_around_a_step_in_flight(egg):
    h = egg.SimulationHandler()
    ids = [h.add(x, y) for x, y in EGGS[:2]]
    held, state = h.touch_table(), _state(h)
    assert held.shape[0] > 0
    h.step_begin(H60, S, CS)
    with pytest.raises(egg.EggError, match=r"egg_touches: a step is in flight \(egg_step_begin without egg_step_end\)"):
        h.touches()
    with pytest.raises(egg.EggError, match=r"egg_touches_of: a step is in flight \(egg_step_begin"):
        h.touches_of([(300.0, 300.0, 5.0)])
    with pytest.raises(egg.EggError, match="egg_touches: a step is in flight"):
        h.touching(ids[0], ids[1])
    h.step_end(False)
    assert _same(state, _state(h)) and np.array_equal(h.touch_table(), held)
    h.step_begin(H60, S, CS)
    h.step_end(True)
    _assert_touches(h, None, None, "both", "after the committed step")
    # the other side: a relaxed step opened through the wire calls
    r = _relaxed_scene(egg.SimulationHandler())
    r.add(300.0, 300.0)
    r.step(H60, S, CS)
    held = r.touch_table()
    r.rx_set_keys(WHITE, [1], [0], r.get_n_particles()[WHITE])
    r.rx_set_keys(YOLK, [1], [0], r.get_n_particles()[YOLK])
    r.rx_begin(H60, S, CS)
    with pytest.raises(egg.EggError, match=r"egg_touches: a step is in flight \(egg_rx_begin without egg_rx_end\)"):
        r.touches()
    with pytest.raises(egg.EggError, match=r"egg_touches_of: a step is in flight \(egg_rx_begin"):
        r.touches_of([(300.0, 300.0, 5.0)])
    r.rx_end(False)
    assert np.array_equal(r.touch_table(), held)


def test_a_call_only_observes(egg):
    """the same relaxed scene with and without touch calls: equal particles, equal launches per step; a call changes no
    download and no counter but kernel_launches"""
    a, b = _relaxed_scene(egg.SimulationHandler()), _relaxed_scene(egg.SimulationHandler())
    for h in (a, b):
        for x, y in EGGS:
            h.add(x, y)
    launches = {id(a): [], id(b): []}
    for k in range(3):
        for h in (a, b):
            before = h.stats()["kernel_launches"]
            assert h.update(H60, H60, S, CS) == 1
            launches[id(h)].append(h.stats()["kernel_launches"] - before)
        state, stats = _state(a), a.stats()
        first = a.touch_table()
        after = a.stats()
        assert after["kernel_launches"] - stats["kernel_launches"] == 2  # (8 queries: one round of two launches)
        assert {key: v for key, v in after.items() if key != "kernel_launches"} == {key: v for key, v in stats.items() if key != "kernel_launches"}
        for _ in range(10):
            assert np.array_equal(a.touch_table(), first)
        assert _same(state, _state(a)) and _same(_state(a), _state(b)), k
    assert launches[id(a)] == launches[id(b)], launches
    assert a.collider_hits() == b.collider_hits() and a.elapsed == b.elapsed


# ------------------------------------------------------------------------------------------------ the refusals of the C ABI
def test_a_refused_call_leaves_the_callers_buffers_as_they_were(egg):
    from egg_fluid_simulation_amd import _ffi
    h, ids = _scene(egg, _keyed(tt.ROW))
    nan = float("nan")

    def spec(rw=1.0, ry=1.0, mask=3, flags=0):
        return _ffi.EggTouchSpec((C.c_double * 2)(rw, ry), mask, flags)

    def filled():
        out = np.zeros(16, dtype=np.dtype([("b", "u1", 40)]))
        out["b"] = 0x5A
        return out

    untouched = filled().tobytes()
    stats = h.stats()
    for sp, listed, cap, text in ((None, ids, 16, "spec is NULL"), (spec(rw=nan), ids, 16, r"reach\[0\] = nan"), (spec(ry=0.0), ids, 16, r"reach\[1\] = 0"),
                                  (spec(rw=INF), ids, 16, r"reach\[0\] = inf"), (spec(ry=-1.0), ids, 16, r"reach\[1\] = -1"),
                                  (spec(mask=0), ids, 16, "type_mask 0"), (spec(mask=4), ids, 16, "type_mask 4"), (spec(flags=2), ids, 16, "unknown flags 0x2"),
                                  (spec(), [ids[0], 77], 16, "no batch with id `77`"), (spec(), ids, -1, "cap = -1")):
        out = filled()
        rc, n = _raw(h, sp, listed, cap, out)
        assert rc < 0 and n == -7, text
        with pytest.raises(egg.EggError, match="egg_touches: " + text):
            h._check(rc)
        assert out.tobytes() == untouched, text
    n = C.c_int64(-7)
    out = filled()
    lib, one = h._lib, np.ascontiguousarray(ids, dtype=np.int64)
    assert lib.egg_touches(h._h, C.byref(spec()), -1, one.ctypes.data, 16, out.ctypes.data, C.byref(n)) < 0 and "n_ids = -1" in h._message()
    assert lib.egg_touches(h._h, C.byref(spec()), 2, None, 16, out.ctypes.data, C.byref(n)) < 0 and "n_ids = 2 without a list" in h._message()
    assert lib.egg_touches(h._h, C.byref(spec()), 3, one.ctypes.data, 16, None, C.byref(n)) < 0 and "cap = 16 without a buffer" in h._message()
    assert lib.egg_touches(h._h, C.byref(spec()), 3, one.ctypes.data, 16, out.ctypes.data, None) < 0 and "n_out is NULL" in h._message()
    # handed-in discs: a negative count, a type outside 0 .. 1, a radius that is not finite, discs without arrays
    x, y, r = (np.array(v, dtype=np.float64) for v in ([2.0, 2.0], [0.0, 0.0], [1.0, 1.0]))

    def of(queries, radii=r, arrays=True):
        q = (_ffi.EggTouchQuery * len(queries))(*[_ffi.EggTouchQuery(*t) for t in queries])
        return lib.egg_touches_of(h._h, C.byref(spec()), len(queries), C.cast(q, C.c_void_p), x.ctypes.data if arrays else None, y.ctypes.data,
                                  radii.ctypes.data, 16, out.ctypes.data, C.byref(n))
    for queries, radii, arrays, text in (([(-1, 0, -1)], r, True, "query 0: count -1 is negative"), ([(-1, 0, 1), (-1, 2, 1)], r, True, "query 1: type 2"),
                                         ([(-1, 0, 2)], np.array([1.0, INF]), True, "the radius of disc 1 is not finite"),
                                         ([(-1, 0, 2)], np.array([nan, 1.0]), True, "the radius of disc 0 is not finite"),
                                         ([(-1, 0, 2)], r, False, "2 discs without x, y or r")):
        assert of(queries, radii, arrays) < 0 and ("egg_touches_of: " + text) in h._message(), text
    assert lib.egg_touches_of(h._h, C.byref(spec()), -1, None, None, None, None, 16, out.ctypes.data, C.byref(n)) < 0 and "n_queries = -1" in h._message()
    assert n.value == -7 and out.tobytes() == untouched and h.stats() == stats  # (nothing was launched, nothing written)
    # the short buffer: n_out is the size of the answer, out stays as it was
    rc, count = _raw(h, spec(), ids, 3, out)
    assert rc < 0 and count == 4 and out.tobytes() == untouched
    with pytest.raises(egg.EggError, match="egg_touches: the answer holds 4 records, the buffer 3"):
        h._check(rc)
    assert _raw(h, spec(), ids, 0, None) == (rc, 4)
    rc, count = _raw(h, spec(), ids, 4, out)
    assert (rc, count) == (0, 4) and out.tobytes()[160:] == untouched[160:]  # (the answer takes 4 records, not one more)
    assert of([(2, 0, 1), (-1, 0, 1)]) == 0 and n.value == 5  # (key 2 leaves batch 2 out: 2 records; no key: 3)
    # the wrappers' own checks, and a handle without particles
    with pytest.raises(egg.EggError, match="reach must be finite and above 0"):
        h.touches(None, 0.0)
    with pytest.raises(egg.EggError, match="types must be"):
        h.touch_table(None, None, "red")
    with pytest.raises(egg.EggError, match="no batch with id `9`"):
        h.touching(ids[0], 9)
    empty = egg.SimulationHandler()
    assert empty.touches() == [] and empty.touch_table().shape == (0, 8) and empty.touches_of([(0.0, 0.0, 1.0)]) == ([], [])
    assert h.touches([]) == [] and h.touch_table([]).shape == (0, 8)


# ------------------------------------------------------------------------------------------------ device groups
CUTS = {2: [-INF, 335.0, INF], 3: [-INF, 320.0, 372.0, INF]}


@pytest.mark.parametrize("n_handles,eggs", [(2, EGGS[1::-1] + EGGS[2:]), (3, EGGS)])
def test_device_group_equals_one_handle(egg, n_handles, eggs):
    g = _relaxed_scene(egg.SimulationGroup([0] * n_handles, cuts=CUTS[n_handles]))
    h = _relaxed_scene(egg.SimulationHandler())
    ids = [g.add(x, y) for x, y in eggs]
    assert [h.add(x, y) for x, y in eggs] == ids
    owners = [g.owner(i)[0] for i in ids]
    assert len(set(owners)) == n_handles and owners[0] != owners[1]  # (the two overlapping eggs live on different handles)
    listed = [ids[3], ids[0], ids[3], ids[1]]
    for k in range(2):
        want = _assert_touches(h, None, None, "both", "one handle, step %d" % k)
        assert any(ids[r[0]] == ids[0] and r[2] == ids[1] for r in want)  # (a touching pair across two handles)
        assert _rows(g.touch_table()) == want and g.touches() == h.touches()
        assert _rows(g.touch_table(listed, 1.1, "white")) == _assert_touches(h, listed, 1.1, "white", "listed, step %d" % k)
        assert [g.touching(i) for i in ids] == [h.touching(i) for i in ids] and g.touching(ids[0], ids[1])
        _info, ws, _ys = h.export_batch(ids[0])
        assert g.touches_of(ws[[0, 1, 7]].T, None, "white", key=ids[0]) == (h.touches([ids[0]], None, "white")[0][0], [])
        g.step(H60, S, CS)
        h.step(H60, S, CS)
    with pytest.raises(egg.EggError, match="egg_group_touches: no batch with id `77`"):
        g.touches([ids[0], 77])
    with pytest.raises(egg.EggError, match="reach must be finite"):
        g.touches(None, -1.0)
    assert g.touches([]) == []


# ------------------------------------------------------------------------------------------------ sharded
SHARDED_CUTS = [-2000.0, 335.0, 2.0 ** 41]


def _worker(rank, world, port, q):
    import os
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from egg_fluid_simulation_amd import SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler, SlabLayout
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sh = _relaxed_scene(ShardedSimulationHandler(SlabLayout(SHARDED_CUTS), rank, dist, lambda: SimulationHandler(device=0), device="cpu"))
        ids = [sh.add(x, y, 50, 15) for x, y in EGGS[1::-1] + EGGS[2:]]
        steps = []
        for _ in range(2):
            steps.append(dict(every=sh.touch_table().tolist(), listed=sh.touch_table([ids[3], ids[0], ids[3], ids[1]], 1.1, "white").tolist(),
                              lists=[[[tuple(t) for t in side] for side in pair] for pair in sh.touches()], owned=len(sh.local.list_ids()),
                              touching=[sh.touching(i) for i in ids], of=[[tuple(t) for t in side] for side in sh.touches_of([(330.0, 300.0, 20.0)])]))
            sh.step(H60, S, CS)
        q.put((rank, "ok", dict(steps=steps, empty=sh.touches([]))))
    except Exception:
        import traceback
        q.put((rank, "error: " + traceback.format_exc(), None))
    finally:
        dist.destroy_process_group()


def _spawn(world):
    import queue
    import time

    import torch.multiprocessing as mp
    from test_gpu_sharded_relaxed import _free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    deadline = time.time() + 300
    while len(res) < world and time.time() < deadline:
        try:
            rank, outcome, results = q.get(timeout=2)
            assert outcome == "ok", outcome
            res[rank] = results
        except queue.Empty:
            if any(p.exitcode not in (None, 0) for p in procs):
                break
    for p in procs:
        p.join(20)
        if p.is_alive():
            p.kill()  # the exact child started above
    assert len(res) == world and all(p.exitcode == 0 for p in procs), "a rank failed: see its traceback above"
    return res


def test_sharded_two_ranks_equal_one_handle(egg):
    """two ranks on one GPU (three processes with the GPU open), the cut between the two overlapping eggs: the gathered and
    added records are one handle's on both ranks"""
    res = _spawn(2)
    h = _relaxed_scene(egg.SimulationHandler())
    ids = [h.add(x, y, 50, 15) for x, y in EGGS[1::-1] + EGGS[2:]]
    for k in range(2):
        want = _assert_touches(h, None, None, "both", "one handle, step %d" % k)
        listed = _assert_touches(h, [ids[3], ids[0], ids[3], ids[1]], 1.1, "white", "listed, step %d" % k)
        assert any(r[0] == 0 and r[2] == ids[1] for r in want)
        for r in (0, 1):
            got = res[r]["steps"][k]
            assert [tuple(t) for t in got["every"]] == want and [tuple(t) for t in got["listed"]] == listed, (r, k)
            assert got["lists"] == [[[tuple(t) for t in side] for side in pair] for pair in h.touches()], (r, k)
            assert got["touching"] == [h.touching(i) for i in ids] and 1 <= got["owned"] < len(ids)
            assert got["of"] == [[tuple(t) for t in side] for side in h.touches_of([(330.0, 300.0, 20.0)])]
        h.step(H60, S, CS)
    assert res[0]["empty"] == [] and res[1]["empty"] == []
