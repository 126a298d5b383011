"""Measures (egg_measure) on the device against the CPU model tests/measure_model.py evaluated on
the handle's own downloads: every comparison is == on integers, or on doubles derived from them by the same host formula;
there is no tolerance.

A scene of eight batches whose white counts sit on every seam of the kernel (1, 63, 64, 65: the chunk of a wave; 1,023,
1,024, 1,025: the one-wave and the 256-thread walk; 2,100: several chunks of the latter) under moving targets in exact and
in relaxed order with colliders and a force, and after a swirl; every batch, repeated ids, one id; a region that cuts atoms
and one with a white-only mask; a batch imported with a NaN, an infinity and a 2^37 coordinate; the hand table of
tests/test_measure_model.py; measure_to into a torch tensor and its refusals; calls around a step in flight on both sides;
a call only observes; one launch per call; a device group, and two and four sharded ranks on GPU 0 over gloo; at_rest."""
import ctypes as C
import warnings

import numpy as np
import pytest

import measure_model as mm
import test_measure_model as tm
from conftest import ROOT
from test_gpu_probes import _template

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
FIELDS = ("x", "y", "vx", "vy", "last_x", "last_y", "radius", "inv_mass", "mass_t", "batch_id")
H60, S, CS = 1 / 60, 2, 3
INF = float("inf")
MASKS = {"both": 3, "white": 1, "yolk": 2}
COUNTS = (1, 63, 64, 65, 1023, 1024, 1025, 2100)
SPOTS = [(300.0 + 500.0 * (k % 4), 300.0 + 500.0 * (k // 4)) for k in range(8)]
COLLIDERS = [("container", 1050.0, 550.0, 1500.0), ("disc", 560.0, 300.0, 30.0)]
FORCE = [("uniform", 0.0, 300.0)]


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _particles(h):
    """the model's view of a handle: its downloads"""
    return tuple({k: h.download(w, k) for k in ("x", "y", "vx", "vy", "radius", "inv_mass", "batch_id")} for w in (WHITE, YOLK))


def _state(h):
    return [h.download(w, f) for w in (WHITE, YOLK) for f in FIELDS]


def _same(a, b):
    return all(np.array_equal(p.view(np.uint64) if p.dtype == np.float64 else p, q.view(np.uint64) if q.dtype == np.float64 else q) for p, q in zip(a, b))


def _assert_measure(h, ids, region, types, what, parts=None):
    """h.measure_table is the model's table over h's own downloads, integer for integer, and h.measure derives what the model
    derives; returns the table"""
    parts = _particles(h) if parts is None else parts
    listed = h.list_ids() if ids is None else list(ids)
    want = mm.measure(parts, listed, region, MASKS[types])
    got = h.measure_table(ids, region, types)
    assert got.dtype == np.int64 and got.shape == (len(listed), 2, 24), what
    bad = np.argwhere(got != want)
    print("%s: %d records, %d words differ%s" % (what, 2 * len(listed), len(bad), "" if not len(bad) else ": first %s device %d model %d" % (
        (listed[bad[0][0]], ("white", "yolk")[bad[0][1]], mm.FIELDS[bad[0][2]]), got[tuple(bad[0])], want[tuple(bad[0])])))
    assert np.array_equal(got, want), what
    for pair, rows in zip(h.measure(ids, region, types), want):
        for m, rec in zip(pair, rows):
            d = mm.derived(rec)
            assert (m is None) == (d is None), what
            if m is not None:
                assert tuple(m) == tuple(int(v) for v in rec) and all(type(v) is int for v in m)
                for name in ("kept", "mass", "centroid", "center_of_mass", "momentum", "velocity", "kinetic_energy", "bounds", "max_speed",
                             "origin", "reach", "spin"):
                    assert getattr(m, name) == d[name], (what, name)
                assert m.axes() == mm.axes(rec), what
    return want


def _eight(egg, order):
    """(handle, ids): a one-particle white atom (imported: add creates no batch of one) and seven added batches with the
    other white counts; the last one without yolk where add accepts that"""
    h = egg.SimulationHandler()
    if order == "relaxed":
        h.set_solver_order("relaxed")
        h.set_colliders(COLLIDERS)
        h.set_forces(FORCE)
    info, ws, ys = _template(egg, 1, 2)
    ws, ys = ws.copy(), ys.copy()
    for state, spots in ((ws, [SPOTS[0]]), (ys, [(SPOTS[0][0] - 20.0, SPOTS[0][1]), (SPOTS[0][0] + 20.0, SPOTS[0][1])])):
        for p, (x, y) in enumerate(spots):
            state[0, p] = state[4, p] = x
            state[1, p] = state[5, p] = y
            state[2, p] = state[3, p] = 0.0
    ids = [h.import_batch(dict(info, key=1, target_x=SPOTS[0][0], target_y=SPOTS[0][1]), ws, ys)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", egg.EggWarning)
        for k, n in enumerate(COUNTS[1:], 1):
            x, y = SPOTS[k]
            radius = 50 if n < 1000 else 120
            if k == 7:
                try:
                    ids.append(h.add(x, y, radius, 15, None, None, n, 0))
                    continue
                except egg.EggError:
                    pass  # (add refuses a batch without yolk: the default count then)
            ids.append(h.add(x, y, radius, 15, None, None, n))
    assert [h.get_n_particles(i)[0] for i in ids] == list(COUNTS)
    return h, ids


def _drive(h, ids, k):
    for j, i in enumerate(ids):
        x, y = SPOTS[j]
        h.set_target_position(i, x + 40.0 * np.cos(0.7 * k + j), y + 40.0 * np.sin(0.7 * k + j))
    assert h.update(H60, H60, S, CS) == 1


# ------------------------------------------------------------------------------------------------ the eight atoms on the seams
@pytest.mark.parametrize("order", ["exact", "relaxed"])
def test_eight_batches_under_moving_targets(egg, order):
    h, ids = _eight(egg, order)
    _assert_measure(h, None, None, "both", order + ": before a step")
    for k in range(4):
        _drive(h, ids, k)
    parts = _particles(h)
    before = h.stats()["kernel_launches"]
    every = _assert_measure(h, None, None, "both", order + ": every batch", parts)
    assert h.stats()["kernel_launches"] - before == 2  # (_assert_measure calls twice: ONE launch per call)
    assert [int(r[0][0]) for r in every] == list(COUNTS) and all(int(r[0][1]) == n and int(r[0][2]) == 0 for r, n in zip(every, COUNTS))
    assert all(int(r[0][15]) > 0 for r in every[1:])  # (they move)
    listed = [ids[7], ids[0], ids[7], ids[4], ids[4], ids[5]]
    assert np.array_equal(_assert_measure(h, listed, None, "both", order + ": repeated", parts), every[[ids.index(i) for i in listed]])
    assert np.array_equal(_assert_measure(h, [ids[6]], None, "both", order + ": one id", parts), every[6:7])
    assert np.array_equal(_assert_measure(h, None, None, "both", order + ": every batch again", parts), every)
    white = _assert_measure(h, None, None, "white", order + ": white", parts)
    yolk = _assert_measure(h, ids[::-1], None, "yolk", order + ": yolk, reversed", parts)
    assert np.array_equal(white[:, 0], every[:, 0]) and not white[:, 1].any() and np.array_equal(yolk[::-1, 1], every[:, 1]) and not yolk[:, 0].any()
    assert h.measure_table([]).shape == (0, 2, 24) and h.measure([]) == []
    # a region that cuts atoms: a half-plane through the second column of eggs and a capsule along the second row
    cut = _assert_measure(h, None, ("half_plane", 1.0, 0.05, 815.0), "both", order + ": a half-plane", parts)
    assert any(0 < int(r[0][1]) < int(r[0][0]) for r in cut) and np.array_equal(cut[:, :, 0], every[:, :, 0])
    cut = _assert_measure(h, listed, ("capsule", 200.0, 800.0, 1900.0, 820.0, 60.0), "both", order + ": a capsule", parts)
    assert any(0 < int(r[0][1]) < int(r[0][0]) for r in cut)
    # a region with a white-only mask under types = "both": the yolk atoms are there, none of their particles is measured
    masked = _assert_measure(h, None, ("disc", 1050.0, 550.0, 5000.0, "white"), "both", order + ": a white-only disc", parts)
    assert np.array_equal(masked[:, 0], every[:, 0]) and np.array_equal(masked[:, 1, 0], every[:, 1, 0]) and not masked[:, 1, 1:].any()
    assert all(pair[1] is None for pair in h.measure(None, ("disc", 1050.0, 550.0, 5000.0, "white")))
    # after a swirl the angular momentum about the origin is there
    for j, i in enumerate(ids):
        h.stir(SPOTS[j][0], SPOTS[j][1], 400.0, 3.0 if j % 2 else -2.0, id=i)
    spun = _assert_measure(h, None, None, "both", order + ": after a swirl")
    assert all(abs(int(r[0][22])) > 65536 for r in spun[1:]) and not np.array_equal(spun[:, :, 22], every[:, :, 22])
    _drive(h, ids, 5)
    _assert_measure(h, None, None, "both", order + ": the step after the swirl")


# ------------------------------------------------------------------------------------------------ placed particles
def _placed(egg, batches):
    """(handle, ids): batches of rows (x, y, vx, vy, radius, inv_mass) per type, imported at rest in the list's order"""
    h = egg.SimulationHandler()
    ids = []
    for key, (white, yolk) in enumerate(batches, 1):
        info, ws, ys = _template(egg, len(white), len(yolk))
        ws, ys = ws.copy(), ys.copy()
        for state, rows in ((ws, white), (ys, yolk)):
            for p, (x, y, vx, vy, r, im) in enumerate(rows):
                state[0, p] = state[4, p] = x
                state[1, p] = state[5, p] = y
                state[2, p], state[3, p], state[6, p], state[7, p] = vx, vy, im, r
        ids.append(h.import_batch(dict(info, key=key), ws, ys))
    return h, ids


@pytest.mark.parametrize("name", sorted(tm.CASES))
def test_hand_case(egg, name):
    case = tm.CASES[name]
    h, ids = _placed(egg, [(case["rows"], [(5.0, 5.0, 0.0, 0.0, 1.0, 1.0)])])
    got = _assert_measure(h, None, case["region"], "both", name)
    assert tuple(int(v) for v in got[0][0]) == tuple(case["record"][f] for f in mm.FIELDS)  # (the model's and the hand-written one)


def test_a_nan_an_infinity_and_a_far_coordinate(egg):
    rows = [(10.0 + p, 20.0 - p, 1.0, 0.5 * p, 2.0, 1.0 + 0.25 * p) for p in range(70)]
    bad = list(rows)
    bad[3] = (float("nan"), 17.0, 1.0, 1.5, 2.0, 1.75)
    bad[64] = (74.0, INF, 1.0, 32.0, 2.0, 17.0)
    bad[69] = (2.0 ** 37, -49.0, 1.0, 34.5, 2.0, 18.25)
    h, ids = _placed(egg, [(rows, rows[:5]), (bad, bad[:5])])
    got = _assert_measure(h, None, None, "both", "a NaN, an infinity, 2^37")
    assert [int(v) for v in got[1][0][:3]] == [70, 70, 3] and [int(v) for v in got[1][1][:3]] == [5, 5, 1] and int(got[0][0][2]) == 0
    keep = [p for p in range(70) if p not in (3, 64, 69)]
    alone, _ = _placed(egg, [([rows[p] for p in keep], rows[:2])])
    assert np.array_equal(alone.measure_table()[0][0][3:], got[1][0][3:])  # (the others are unchanged by their presence)
    _assert_measure(h, None, ("box", 40.0, 0.0, 30.0, 40.0, 0.3), "both", "the same under a box")


# ------------------------------------------------------------------------------------------------ measure_to
EGGS = ((300.0, 300.0), (360.0, 310.0), (330.0, 250.0), (420.0, 330.0))
CONTAINER = [("container", 350.0, 300.0, 140.0)]
GRAVITY = [("uniform", 0.0, 400.0)]


def _relaxed_scene(h):
    h.set_solver_order("relaxed")
    h.set_colliders(CONTAINER)
    h.set_forces(GRAVITY)
    return h


def _four_eggs(egg, order):
    h = egg.SimulationHandler()
    if order == "relaxed":
        _relaxed_scene(h)
    return h, [h.add(x, y) for x, y in EGGS]


def test_measure_to_fills_a_torch_tensor_and_refuses_what_it_cannot(egg):
    import torch
    from egg_fluid_simulation_amd import _ffi
    h, ids = _four_eggs(egg, "exact")
    for _ in range(2):
        h.update(H60, H60, S, CS)
    dev = torch.device("cuda:0")
    region = ("disc", 340.0, 300.0, 45.0)
    out = torch.full((6, 2, 24), 77, dtype=torch.int64, device=dev)  # (stale contents, and two rows more than the call fills)
    assert h.measure_to(out) == 4
    assert np.array_equal(out[:4].cpu().numpy(), h.measure_table()) and bool((out[4:] == 77).all())
    listed = [ids[2], ids[2], ids[0]]
    assert h.measure_to(out, listed, region, "yolk") == 3
    assert np.array_equal(out[:3].cpu().numpy(), h.measure_table(listed, region, "yolk")) and not out[:3, 0].any() and bool((out[4:] == 77).all())
    assert h.measure_to((out.data_ptr(), 8 * out.numel()), [ids[1]]) == 1 and np.array_equal(out[:1].cpu().numpy(), h.measure_table([ids[1]]))
    assert h.measure_to(out, []) == 0
    # the refusals: the buffer stays as it was
    out.fill_(55)
    spec = h._c_measure_spec(None, "both")
    host = np.full((4, 2, 24), 55, dtype=np.int64)
    raw = torch.full((4 * 2 * 24 * 8 + 16,), 55, dtype=torch.uint8, device=dev)
    before = h.stats()
    for address, capacity, text in ((host.ctypes.data, host.nbytes, "is not 1536 bytes of memory of device 0"), (raw.data_ptr() + 3, 1536, "not aligned to 8 bytes"),
                                    (out.data_ptr(), 1535, "capacity_bytes = 1535"), (0, 1536, "out is NULL"), (out.data_ptr(), -1, "capacity_bytes = -1")):
        rc = h._lib.egg_measure_to(h._h, C.byref(spec), 0, None, C.c_void_p(address), capacity)
        assert rc == _ffi.EGG_ERR_INVALID_ARGUMENT and "egg_measure_to: " in h._message() and text in h._message(), (text, h._message())
    with pytest.raises(egg.EggError, match="capacity_bytes = 1152"):
        h.measure_to(out[:3])
    with pytest.raises(egg.EggError, match="must hold int64"):
        h.measure_to(out.to(torch.int32))
    with pytest.raises(egg.EggError, match="must be contiguous"):
        h.measure_to(out[:, :, ::2])
    with pytest.raises(egg.EggError, match="no batch with id `99`"):
        h.measure_to(out, [ids[0], 99])
    assert bool((out == 55).all()) and bool((raw == 55).all()) and (host == 55).all() and h.stats() == before


# ------------------------------------------------------------------------------------------------ refusals, in flight, observing
def test_refusals_leave_the_table_as_the_caller_filled_it(egg):
    from egg_fluid_simulation_amd import _ffi
    h, ids = _four_eggs(egg, "exact")

    def spec_of(flags=0, mask=3, region=None):
        spec = h._c_measure_spec(region, "both")
        if region is None:
            spec.flags = flags
        spec.type_mask = mask
        return spec

    def call(spec, n, listed, with_out=True, rc=_ffi.EGG_ERR_INVALID_ARGUMENT, text=""):
        out = np.full((16, 2, 24), 0x5A5A, dtype=np.int64)
        arr = None if listed is None else np.ascontiguousarray(listed, dtype=np.int64)
        before = h.stats()
        got = h._lib.egg_measure(h._h, None if spec is None else C.byref(spec), n, None if arr is None else arr.ctypes.data,
                                 out.ctypes.data if with_out else None)
        assert got == rc, (text, got)
        assert text in h._message(), (text, h._message())
        assert (out == 0x5A5A).all() and h.stats() == before, text

    call(None, 0, None, text="egg_measure: spec is NULL")
    call(spec_of(), 0, None, with_out=False, text="egg_measure: out is NULL")
    call(spec_of(), -1, None, text="egg_measure: n_ids = -1 without a list")
    call(spec_of(), 2, None, text="egg_measure: n_ids = 2 without a list")
    call(spec_of(), 2, [ids[0], 99], rc=_ffi.EGG_ERR_UNKNOWN_ID, text="egg_measure: no batch with id `99`")
    call(spec_of(), 1, [0], rc=_ffi.EGG_ERR_UNKNOWN_ID, text="egg_measure: no batch with id `0`")
    for flags in (2, 3, -1, 1 << 20):
        call(spec_of(flags=flags), 0, None, text="egg_measure: unknown flag bits %d" % flags)
    for mask in (0, 4, -1):
        call(spec_of(mask=mask), 1, [ids[0]], text="egg_measure: type_mask %d" % mask)
    bad = spec_of(region=("disc", 0.0, 0.0, 1.0))
    bad.region.p[2] = -1.0
    call(bad, 0, None, text="egg_measure: region 0 (disc): radius -1 is negative")
    bad.region.kind = 9
    call(bad, 0, None, text="egg_measure: region 0: unknown kind 9")
    # without the flag the region is ignored and need not be valid
    bad.flags = 0
    out = np.zeros((4, 2, 24), dtype=np.int64)
    assert h._lib.egg_measure(h._h, C.byref(bad), 0, None, out.ctypes.data) == _ffi.EGG_OK and np.array_equal(out, h.measure_table())
    # the wrappers' own checks
    for kw, text in ((dict(types="none"), "measure_table: types must be"), (dict(types=0), "types must be"), (dict(ids=[1.5, "a"]), "ids must be None or a list"),
                     (dict(region=("ring", 0, 0, 1)), "measure_table: region"), (dict(region=("half_plane", 0.0, 0.0, 1.0)), "below eps")):
        with pytest.raises(egg.EggError, match=text):
            h.measure(**kw)
    with pytest.raises(egg.EggError, match="below eps"):
        h.measure([], ("half_plane", 0.0, 0.0, 1.0))  # (checked though nothing is asked for)
    # a handle without batches: nothing to report, nothing launched
    empty = egg.SimulationHandler()
    assert empty.measure() == [] and empty.measure_table().shape == (0, 2, 24) and empty.stats()["kernel_launches"] == 0
    with pytest.raises(egg.EggError, match="no batch with id `1`"):
        empty.measure([1])


def test_calls_around_a_step_in_flight(egg):
    import torch
    h, ids = _four_eggs(egg, "exact")
    held = h.measure_table()
    state = _state(h)
    out = torch.full((4, 2, 24), 7, dtype=torch.int64, device="cuda:0")
    h.step_begin(H60, S, CS)
    with pytest.raises(egg.EggError, match=r"egg_measure: a step is in flight \(egg_step_begin without egg_step_end\)"):
        h.measure()
    with pytest.raises(egg.EggError, match=r"egg_measure_to: a step is in flight \(egg_step_begin"):
        h.measure_to(out)
    with pytest.raises(egg.EggError, match="egg_measure: a step is in flight"):
        h.at_rest(ids[0], 1.0)
    h.step_end(False)
    assert _same(state, _state(h)) and np.array_equal(h.measure_table(), held) and bool((out == 7).all())
    h.step_begin(H60, S, CS)
    h.step_end(True)
    _assert_measure(h, None, None, "both", "after the committed step")
    # the other side: a relaxed step opened through the wire calls
    r = _relaxed_scene(egg.SimulationHandler())
    r.add(300.0, 300.0)
    r.step(H60, S, CS)
    held = r.measure_table()
    r.rx_set_keys(WHITE, [1], [0], r.get_n_particles()[WHITE])
    r.rx_set_keys(YOLK, [1], [0], r.get_n_particles()[YOLK])
    r.rx_begin(H60, S, CS)
    with pytest.raises(egg.EggError, match=r"egg_measure: a step is in flight \(egg_rx_begin without egg_rx_end\)"):
        r.measure()
    with pytest.raises(egg.EggError, match=r"egg_measure_to: a step is in flight \(egg_rx_begin"):
        r.measure_to(out)
    r.rx_end(False)
    assert np.array_equal(r.measure_table(), held) and bool((out == 7).all())


def test_a_call_only_observes(egg):
    """the same relaxed scene with and without measure calls: equal particles, equal launches per step; a call changes no
    download and no counter but kernel_launches, which rises by exactly 1"""
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
        first = a.measure_table()
        after = a.stats()
        assert after["kernel_launches"] - stats["kernel_launches"] == 1
        assert {key: v for key, v in after.items() if key != "kernel_launches"} == {key: v for key, v in stats.items() if key != "kernel_launches"}
        for _ in range(20):
            assert np.array_equal(a.measure_table(), first)
        assert np.array_equal(a.measure_table(None, ("disc", 340.0, 300.0, 45.0))[:, :, 0], first[:, :, 0])
        assert a.stats()["kernel_launches"] - after["kernel_launches"] == 21 and _same(state, _state(a))
        assert _same(_state(a), _state(b)), k
    assert launches[id(a)] == launches[id(b)], launches
    assert a.collider_hits() == b.collider_hits() and a.elapsed == b.elapsed


def test_at_rest_flips_as_a_kicked_egg_settles_under_a_full_brake(egg):
    h = egg.SimulationHandler()
    i, j = h.add(300.0, 300.0), h.add(900.0, 300.0)
    everywhere = ("disc", 300.0, 300.0, 200.0)
    assert h.at_rest(i, 0.0) and h.at_rest(j, 0.0)  # (fresh eggs do not move)
    h.kick(everywhere, 30.0, -40.0, id=i)
    assert not h.at_rest(i, 49.0) and h.at_rest(i, 50.0) and h.at_rest(j, 0.0)
    m = h.measure([i])[0]
    assert m[WHITE].max_speed == 50.0 and m[YOLK].max_speed == 50.0 and m[WHITE].kinetic_energy > 0.0
    h.brake(everywhere, 1.0, id=i)
    for types in ("both", "white", "yolk"):
        assert h.at_rest(i, 0.0, types)
    h.kick(everywhere + ("yolk",), 3.0, 4.0, id=i)
    assert h.at_rest(i, 1.0, "white") and not h.at_rest(i, 1.0, "yolk") and not h.at_rest(i, 1.0) and h.at_rest(i, 5.0)


# ------------------------------------------------------------------------------------------------ device groups
CUTS = {2: [-INF, 335.0, INF], 3: [-INF, 320.0, 372.0, INF]}
REGION = ("box", 345.0, 300.0, 60.0, 25.0, 0.4)


@pytest.mark.parametrize("n_handles,eggs", [(2, EGGS[1::-1] + EGGS[2:]), (3, EGGS)])
def test_device_group_equals_one_handle(egg, n_handles, eggs):
    g = _relaxed_scene(egg.SimulationGroup([0] * n_handles, cuts=CUTS[n_handles]))
    h = _relaxed_scene(egg.SimulationHandler())
    ids = [g.add(x, y) for x, y in eggs]
    assert [h.add(x, y) for x, y in eggs] == ids
    assert len({g.owner(i)[0] for i in ids}) == n_handles
    assert not hasattr(g, "measure_to")
    listed = [ids[3], ids[0], ids[3], ids[1]]
    for k in range(3):
        want = _assert_measure(h, None, None, "both", "one handle, step %d" % k)
        assert np.array_equal(g.measure_table(), want) and g.measure() == h.measure()
        assert np.array_equal(g.measure_table(listed, REGION, "white"), _assert_measure(h, listed, REGION, "white", "listed, step %d" % k))
        assert [g.at_rest(i, 20.0) for i in ids] == [h.at_rest(i, 20.0) for i in ids]
        g.step(H60, S, CS)
        h.step(H60, S, CS)
    with pytest.raises(egg.EggError, match="egg_group_measure: no batch with id `77`"):
        g.measure([ids[0], 77])
    with pytest.raises(egg.EggError, match="below eps"):
        g.measure([], ("half_plane", 0.0, 0.0, 1.0))
    assert g.measure([]) == []


# ------------------------------------------------------------------------------------------------ sharded
SHARDED_CUTS = {2: [-2000.0, 335.0, 2.0 ** 41], 4: [-2000.0, 315.0, 345.0, 390.0, 2.0 ** 41]}


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
        sh = _relaxed_scene(ShardedSimulationHandler(SlabLayout(SHARDED_CUTS[world]), rank, dist, lambda: SimulationHandler(device=0), device="cpu"))
        ids = [sh.add(x, y, 50, 15) for x, y in EGGS[1::-1] + EGGS[2:]]
        steps = []
        for _ in range(3):
            steps.append(dict(every=sh.measure_table(), listed=sh.measure_table([ids[3], ids[0], ids[3], ids[1]], REGION, "white"),
                              rest=[sh.at_rest(i, 20.0) for i in ids], owned=len(sh.local.list_ids()),
                              speed=[None if m[0] is None else m[0].max_speed for m in sh.measure()]))
            sh.step(H60, S, CS)
        q.put((rank, "ok", dict(steps=steps, empty=sh.measure([]), has_to=hasattr(sh, "measure_to"))))
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


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_ranks_equal_one_handle(egg, world):
    """the ranks on one GPU, the cuts between the overlapping eggs: the summed tables are one handle's table on every rank"""
    res = _spawn(world)
    h = _relaxed_scene(egg.SimulationHandler())
    ids = [h.add(x, y, 50, 15) for x, y in EGGS[1::-1] + EGGS[2:]]
    listed = [ids[3], ids[0], ids[3], ids[1]]
    for k in range(3):
        every = _assert_measure(h, None, None, "both", "one handle, step %d" % k)
        for r in range(world):
            got = res[r]["steps"][k]
            assert np.array_equal(got["every"], every) and np.array_equal(got["listed"], h.measure_table(listed, REGION, "white")), (r, k)
            assert got["rest"] == [h.at_rest(i, 20.0) for i in ids] and got["speed"] == [m[0].max_speed for m in h.measure()], (r, k)
        assert sum(res[r]["steps"][k]["owned"] for r in range(world)) == 4 and max(res[r]["steps"][k]["owned"] for r in range(world)) < 4
        h.step(H60, S, CS)
    assert all(res[r]["empty"] == [] and not res[r]["has_to"] for r in range(world))
