"""Impulses (egg_impulse) on the device against the CPU model tests/impulse_model.py evaluated on the
handle's own downloads: every comparison is ==, bit for bit; there is no tolerance.

The hand table of tests/test_impulse_model.py (particles placed through export_batch / import_batch), batch sizes on every
seam of the kernel, 64 records with a different answer on every lane and records that chain through one particle, masks and
id filters that leave a type or a batch untouched, the dynamics against the reference model with the same edit, subject
against a freshly imported twin in both solver orders (a blast that makes the next step widen claims included), the
refusals, what an impulse leaves alone, device groups of 2 and 3 handles on GPU 0 and a ShardedSimulationHandler of two
spawned ranks on GPU 0 over gloo."""
import numpy as np
import pytest

import impulse_model as im
import test_impulse_model as ti
from conftest import ROOT

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
FIELDS = ("x", "y", "vx", "vy", "last_x", "last_y")
H60, S, C = 1 / 60, 2, 3
INF = float("inf")


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _placed(egg, white, yolk, v=None, inv_mass=None):
    """(handle, id) of one batch whose particles sit at the given positions, with the given velocities (at rest without)
    and inverse masses (the batch's own without)"""
    src = egg.SimulationHandler()
    i = src.add(0.0, 0.0, 50, 15, None, None, len(white), len(yolk))
    info, ws, ys = src.export_batch(i)
    for t, (state, spots) in enumerate(((ws, white), (ys, yolk))):
        assert state.shape[1] == len(spots)
        for p, (x, y) in enumerate(spots):
            state[0, p] = state[4, p] = x
            state[1, p] = state[5, p] = y
            state[2, p], state[3, p] = (0.0, 0.0) if v is None else v[t][p]
            if inv_mass is not None:
                state[6, p] = inv_mass[t][p]
    h = egg.SimulationHandler()
    assert h.import_batch(info, ws, ys) == i
    return h, i


def _state(h, fields=FIELDS):
    return {(w, f): h.download(w, f) for w in (WHITE, YOLK) for f in fields}


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)) for k in a)


def _model(h, records, ids=None):
    """the model's (vx, vy, results) for h's own downloads; ids translates the records' ids to what batch_id downloads"""
    cols = [[h.download(w, f) for w in (WHITE, YOLK)] for f in ("x", "y", "vx", "vy", "inv_mass")]
    bid = [h.download(w, "batch_id").astype(np.int64) for w in (WHITE, YOLK)]
    return im.apply(records, *cols, bid, known_ids=set(h.list_ids()))


def _results(model_results):
    from egg_fluid_simulation_amd.simulation_handler import ImpulseResult
    return [ImpulseResult(*r) for r in model_results]


def _assert_impulse(h, records, what):
    """h.impulse(records) leaves the model's bits in vx, vy, returns the model's totals and moves nothing else"""
    before = _state(h)
    want_vx, want_vy, want = _model(h, records)
    got = h.impulse(records)
    after = _state(h)
    print("%s: %s" % (what, got[:3]))
    assert got == _results(want), what
    for w in (WHITE, YOLK):
        assert np.array_equal(after[w, "vx"].view(np.uint64), want_vx[w].view(np.uint64)), (what, w, "vx")
        assert np.array_equal(after[w, "vy"].view(np.uint64), want_vy[w].view(np.uint64)), (what, w, "vy")
        for f in ("x", "y", "last_x", "last_y"):
            assert np.array_equal(after[w, f].view(np.uint64), before[w, f].view(np.uint64)), (what, w, f)
    return got


# ------------------------------------------------------------------------------------------------ the hand table
@pytest.mark.parametrize("name", sorted(ti.CASES))
def test_hand_case(egg, name):
    case = ti.CASES[name]
    h, _ = _placed(egg, *case["spots"], v=case["v"], inv_mass=case["inv_mass"])
    got = _assert_impulse(h, case["records"], name)
    assert got == _results(case["results"])  # (and the hand-written numbers, once more)
    for w in (WHITE, YOLK):
        assert list(zip(h.download(w, "vx").tolist(), h.download(w, "vy").tolist())) == case["after"][w], (name, w)


# ------------------------------------------------------------------------------------------------ the kernel's seams
@pytest.mark.parametrize("n", [2, 64, 65, 1024, 1025, 2500])
def test_batch_sizes_on_every_seam(egg, n):
    """n particles per type on a line of which a disc covers about half, a different value per particle through the linear
    weight, the inverse mass and the swirl's arm: lanes of a partly filled wave, the step to a second chunk, the unit
    boundary at 1,024 and three units"""
    t = np.arange(n, dtype=np.float64)
    white = list(zip(-100.0 + 200.0 * t / max(n - 1, 1), 0.125 * np.cos(t)))
    yolk = list(zip(-10.0 + 150.0 * t / max(n - 1, 1), 3.0 + 0.01 * np.sin(t)))
    v = [[(0.25 * np.sin(p), 0.5 * np.cos(p)) for p in range(n)]] * 2
    h, _ = _placed(egg, white, yolk, v=v)
    records = [("kick", ("disc", -60.0, 0.0, 65.0), 3.0, -1.0, dict(linear=True, by_inv_mass=True)),
               ("swirl", ("disc", -60.0, 0.0, 65.0), 1.0, 2.0, 0.75),
               ("blast", ("capsule", -200.0, 0.0, 0.0, 0.0, 30.0, "white"), 5.0, 5.0, 40.0, dict(linear=True)),
               ("brake", ("half_plane", 1.0, 0.0, 20.0), 1.0, 1.0, 0.25)]
    got = _assert_impulse(h, records, "n = %d" % n)
    assert 0 < got[0].count[WHITE] < n and 0 < got[0].count[YOLK] < n and got[2].count[YOLK] == 0 and sum(sum(r.skipped) for r in got) == 0
    assert h.impulse(records, results=False) is None  # (the same edit once more, without totals)
    again = _state(h, ("vx", "vy"))
    h2, _ = _placed(egg, white, yolk, v=v)
    h2.impulse(records)
    h2.impulse(records)
    assert _same(again, _state(h2, ("vx", "vy")))


def test_64_records_with_a_different_answer_on_every_lane_and_chains(egg):
    white = [(1.0 * p, 5.0) for p in range(200)]
    yolk = [(2.0 * p, -5.0) for p in range(130)]
    h, _ = _placed(egg, white, yolk)
    records = [("kick", ("half_plane", 1.0, 0.0, 3.0 * k + 0.5, "white" if k % 3 == 0 else "both"), 0.5 + k, -1.0) for k in range(64)]
    got = _assert_impulse(h, records, "64 records")
    assert len({(r.count[WHITE], r.sdvx[WHITE]) for r in got}) == 64 and all(r.count[YOLK] == 0 for r in got[::3])
    # records that chain through one particle: each finds what the one before it left
    disc = ("disc", 199.0, 5.0, 0.5)
    chain = []
    for k in range(16):
        chain += [("kick", disc, 1.0 + k, 0.125 * k), ("brake", disc, -3.0, 2.0, 0.5), ("swirl", disc, 190.0, 0.0, 0.0625 * k),
                  ("blast", disc, 100.0, 100.0, -7.0 - k)]
    got = _assert_impulse(h, chain, "a chain of 64")
    assert all(r.count == (1, 0) for r in got)


def test_masks_and_ids_that_leave_a_type_or_a_batch_untouched(egg):
    h = egg.SimulationHandler()
    ids = [h.add(x, y) for x, y in ((300.0, 300.0), (330.0, 310.0), (900.0, 300.0))]
    for _ in range(2):
        h.update(H60, H60, S, C)
    everywhere = ("disc", 320.0, 300.0, 1e4)
    bid = [h.download(w, "batch_id").astype(np.int64) for w in (WHITE, YOLK)]
    for types, other in (("white", YOLK), ("yolk", WHITE)):
        before = _state(h)
        got = _assert_impulse(h, [("kick", everywhere + (types,), 1.0, 2.0), ("swirl", everywhere + (types,), 320.0, 300.0, 0.5)], types)
        after = _state(h)
        assert got[0].count[other] == 0 and got[0].count[1 - other] == bid[1 - other].size
        assert all(np.array_equal(before[other, f].view(np.uint64), after[other, f].view(np.uint64)) for f in FIELDS)
    before = _state(h)
    got = _assert_impulse(h, [("blast", everywhere, 310.0, 300.0, 30.0, dict(id=ids[1], by_inv_mass=True)),
                              ("brake", everywhere, 0.0, 0.0, 0.5, dict(id=ids[2]))], "by id")
    after = _state(h)
    for w in (WHITE, YOLK):
        mine = bid[w] == ids[0]
        assert mine.any() and got[0].count[w] == np.count_nonzero(bid[w] == ids[1]) and got[1].count[w] == np.count_nonzero(bid[w] == ids[2])
        for f in FIELDS:
            assert np.array_equal(before[w, f][mine].view(np.uint64), after[w, f][mine].view(np.uint64)), (w, f)
        assert not np.array_equal(before[w, "vx"][~mine], after[w, "vx"][~mine])


# ------------------------------------------------------------------------------------------------ dynamics
def test_dynamics_against_the_reference_model(egg):
    """two tiny batches, three exact-order steps, a kick plus a linear blast, three more steps: all six fields equal the
    reference model's, which gets the same edit in its particle arrays from impulse_model"""
    import oracle.reference_model as rm
    centres = ((300.0, 300.0), (318.0, 306.0))
    h, m = egg.SimulationHandler(), rm.ReferenceModel()
    for x, y in centres:
        assert h.add(x, y, 20, 8, None, None, 12, 5) == m.add(x, y, 20, 8, 12, 5)
    offsets = dict(zip(FIELDS, (rm.X, rm.Y, rm.VX, rm.VY, rm.LAST_X, rm.LAST_Y)))

    def compare(what):
        for w in (WHITE, YOLK):
            for f in FIELDS:
                want = np.array(m.field(w, offsets[f]), dtype=np.float64)
                assert np.array_equal(h.download(w, f).view(np.uint64), want.view(np.uint64)), (what, w, f)

    for _ in range(3):
        assert h.update(H60, H60, S, C) == 1
        m.update(H60, H60, S, C)
    compare("before the impulse")
    records = [("kick", ("half_plane", 1.0, 0.0, 305.0), 40.0, -25.0), ("blast", ("disc", 309.0, 303.0, 25.0), 309.0, 303.0, 120.0, dict(linear=True))]
    cols = [[np.array(m.field(w, off), dtype=np.float64) for w in (WHITE, YOLK)] for off in (rm.X, rm.Y, rm.VX, rm.VY, rm.INV_MASS)]
    bid = [np.array(m.field(w, rm.BATCH_ID), dtype=np.int64) for w in (WHITE, YOLK)]
    nvx, nvy, want = im.apply(records, *cols, bid)
    for w, data in ((WHITE, m._white_data), (YOLK, m._yolk_data)):
        for p in range(nvx[w].size):
            data[rm.offset(p + 1) + rm.VX] = float(nvx[w][p])
            data[rm.offset(p + 1) + rm.VY] = float(nvy[w][p])
    got = h.impulse(records)
    assert got == _results(want) and min(got[0].count + got[1].count) > 0
    compare("after the impulse")
    for k in range(3):
        assert h.update(H60, H60, S, C) == 1
        m.update(H60, H60, S, C)
        compare("step %d after the impulse" % (k + 1))


# ------------------------------------------------------------------------------------------------ caches
EGGS = ((300.0, 300.0), (360.0, 310.0), (330.0, 250.0), (420.0, 330.0))
CONTAINER = [("container", 350.0, 300.0, 400.0)]
GRAVITY = [("uniform", 0.0, 400.0)]
GENTLE = [("kick", ("disc", 330.0, 300.0, 60.0), 30.0, -10.0, dict(by_inv_mass=True)), ("swirl", ("disc", 360.0, 310.0, 40.0, "yolk"), 360.0, 310.0, 1.5)]
STRONG = [("blast", ("disc", 345.0, 300.0, 150.0), 345.0, 300.0, 6000.0, dict(linear=True))]  # 100 px per step at the centre


def _scene(egg, order):
    h = egg.SimulationHandler()
    if order == "relaxed":
        h.set_solver_order("relaxed")
        h.set_colliders(CONTAINER)
        h.set_forces(GRAVITY)
    return h


@pytest.mark.parametrize("order,records", [("exact", GENTLE), ("exact", STRONG), ("relaxed", GENTLE), ("relaxed", STRONG)],
                         ids=["exact-gentle", "exact-strong", "relaxed-gentle", "relaxed-strong"])
def test_subject_against_a_freshly_imported_twin(egg, order, records):
    """four default eggs, five steps, an impulse, five more steps.  The twin is a fresh handle built at the moment of the
    impulse by export, the model's edit in numpy, import: it has no lists, tiles or claims from before the edit.  Subject and
    twin match bit for bit after the five further steps; the strong blast makes the next exact-order step widen claims."""
    h = _scene(egg, order)
    ids = [h.add(x, y) for x, y in EGGS]
    for _ in range(5):
        assert h.update(H60, H60, S, C) == 1
    twin = _scene(egg, order)
    exports = [h.export_batch(i) for i in ids]
    want_vx, want_vy, want = _model(h, records)
    bid = [h.download(w, "batch_id").astype(np.int64) for w in (WHITE, YOLK)]
    for i, (info, ws, ys) in zip(ids, exports):
        for w, state in ((WHITE, ws), (YOLK, ys)):
            state[2], state[3] = want_vx[w][bid[w] == i], want_vy[w][bid[w] == i]
        assert twin.import_batch(info, ws, ys) == i
    assert h.impulse(records) == _results(want)
    assert _same(_state(h), _state(twin))
    redo = h.stats()["redo_steps"]
    for k in range(5):
        assert h.update(H60, H60, S, C) == 1 and twin.update(H60, H60, S, C) == 1
        assert _same(_state(h), _state(twin)), (order, k)
    moved = max(float(np.abs(h.download(WHITE, "vx")).max()), float(np.abs(h.download(WHITE, "vy")).max()))
    print("%s: largest |v| after five more steps %.1f, steps run again since the impulse: %d" % (order, moved, h.stats()["redo_steps"] - redo))
    assert np.isfinite(moved)
    if order == "exact" and records is STRONG:  # (the blast threw particles out of their tiles' claims: steps were run again)
        assert h.stats()["redo_steps"] > redo


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_change_nothing(egg):
    h = egg.SimulationHandler()
    ids = [h.add(x, y) for x, y in EGGS[:2]]
    h.update(H60, H60, S, C)
    before = _state(h)
    good = ("kick", ("disc", 300.0, 300.0, 100.0), 1.0, 0.0)
    for record, what in ti.BAD[1:]:
        with pytest.raises(egg.EggError, match="record 2"):
            h.impulse([good, good, record])
        assert _same(before, _state(h)), what
    with pytest.raises(egg.EggError, match="no batch with id `99`"):
        h.impulse([good, ("kick", ("disc", 300.0, 300.0, 100.0), 1.0, 0.0, dict(id=99))])
    with pytest.raises(egg.EggError, match="0 .. 64 records"):
        h.impulse([good] * 65)
    assert _same(before, _state(h))
    # through the C ABI: n outside 0 .. 64, n > 0 without a list, an unknown action, unknown flag bits
    from egg_fluid_simulation_amd import _ffi
    n, arr = h._c_impulses([good, good])
    for call, text in ((lambda: h._c("impulse")(-1, arr, None), "n = -1"), (lambda: h._c("impulse")(65, arr, None), "n = 65"),
                       (lambda: h._c("impulse")(2, None, None), "without a list")):
        assert call() == -2 and text in h._lib.egg_last_error(h._h).decode()
    arr[1].action = 4
    assert h._c("impulse")(2, arr, None) == -2 and "record 1: unknown action 4" in h._lib.egg_last_error(h._h).decode()
    arr[1].action, arr[1].flags = 0, 4
    assert h._c("impulse")(2, arr, None) == -2 and "record 1 (kick): unknown flag bits 4" in h._lib.egg_last_error(h._h).decode()
    arr[1].flags, arr[1].id = 0, 99
    assert h._c("impulse")(2, arr, None) == -1 and "record 1: no batch with id `99`" in h._lib.egg_last_error(h._h).decode()  # EGG_ERR_UNKNOWN_ID
    arr[1].id = _ffi.IMPULSE_NO_BATCH
    arr[0].id = _ffi.IMPULSE_NO_BATCH
    launches = h.stats()["kernel_launches"]
    assert h._c("impulse")(2, arr, None) == 0 and h.stats()["kernel_launches"] == launches  # (every record inert: nothing is launched)
    assert _same(before, _state(h))
    # in flight
    h.step_begin(H60, S, C)
    with pytest.raises(egg.EggError, match=r"egg_impulse: a step is in flight \(egg_step_begin without egg_step_end\)"):
        h.impulse([good])
    h.step_end(False)
    assert _same(before, _state(h))
    r = _scene(egg, "relaxed")
    r.add(300.0, 300.0)
    r.step(H60, S, C)
    held = _state(r)
    r.rx_set_keys(WHITE, [1], [0], r.get_n_particles()[WHITE])
    r.rx_set_keys(YOLK, [1], [0], r.get_n_particles()[YOLK])
    r.rx_begin(H60, S, C)
    with pytest.raises(egg.EggError, match=r"egg_impulse: a step is in flight \(egg_rx_begin without egg_rx_end\)"):
        r.kick(("disc", 300.0, 300.0, 100.0), 1.0, 0.0)
    r.rx_end(False)
    assert _same(held, _state(r))
    # what succeeds: no record, no results, no particles
    assert h.impulse([]) == [] and h.impulse([], results=False) is None and _same(before, _state(h))
    assert h.impulse([good], results=False) is None and not _same(before, _state(h))
    empty = egg.SimulationHandler()
    launches = empty.stats()["kernel_launches"]
    assert empty.impulse([good]) == _results([((0, 0),) * 4]) and empty.stats()["kernel_launches"] == launches
    assert empty.kick(("disc", 0.0, 0.0, 1.0), 1.0, 1.0).count == (0, 0)
    assert ids == h.list_ids()


def test_only_the_velocities_move(egg):
    h = egg.SimulationHandler()
    ids = [h.add(x, y) for x, y in EGGS[:3]]
    for _ in range(3):
        h.update(H60, H60, S, C)

    def rest():
        stats = h.stats()
        stats.pop("kernel_launches")
        return dict(fields={k: v.tobytes() for k, v in _state(h, ("x", "y", "last_x", "last_y", "inv_mass", "radius", "mass_t", "batch_id")).items()},
                    elapsed=h.elapsed, targets=[h.get_target_position(i) for i in ids],
                    env=[{k: v for k, v in h.get_environment(w).items() if k != "max_velocity"} for w in (WHITE, YOLK)],
                    positions=[h.get_position(i) for i in ids], counts=h.get_n_particles(), ids=h.list_ids(), stats=stats,
                    version=h.instances(WHITE, color=False)[2])

    held, v = rest(), _state(h, ("vx", "vy"))
    launches = h.stats()["kernel_launches"]
    a = h.blast(330.0, 300.0, 80.0, 200.0)
    b = h.stir(330.0, 300.0, 80.0, 2.0, types="yolk")
    c = h.brake(("half_plane", 0.0, 1.0, 300.0), 0.5)
    d = h.kick(("box", 330.0, 300.0, 40.0, 20.0, 0.3), 5.0, 5.0, id=ids[0])
    assert min(a.count) > 0 and b.count[WHITE] == 0 and b.count[YOLK] > 0 and min(c.count) > 0 and d.count[WHITE] > 0
    assert h.stats()["kernel_launches"] == launches + 8  # (two launches per call with results)
    h.impulse([("kick", ("disc", 330.0, 300.0, 80.0), 1.0, 1.0)], results=False)
    assert h.stats()["kernel_launches"] == launches + 9  # (one without)
    assert rest() == held and not _same(v, _state(h, ("vx", "vy")))
    for w in (WHITE, YOLK):  # (the environment is measured per call: max_velocity is that of the velocities as they are now)
        assert h.get_environment(w)["max_velocity"] > 0.0
    assert h.update(H60, H60, S, C) == 1  # (and the step after it runs)


# ------------------------------------------------------------------------------------------------ device groups
CUTS = {2: [-INF, 335.0, INF], 3: [-INF, 320.0, 372.0, INF]}  # through the eggs inside the first record's disc
GROUP_RECORDS = GENTLE + [("brake", ("half_plane", 0.0, 1.0, 300.0), 5.0, 0.0, 0.25)]


def _group_lists(ids):
    return [GROUP_RECORDS, [("blast", ("disc", 345.0, 300.0, 150.0), 345.0, 300.0, 300.0, dict(linear=True, id=ids[1])),
                            ("kick", ("disc", 345.0, 300.0, 150.0), 3.0, 4.0, dict(id=ids[3])), GROUP_RECORDS[0]]]


@pytest.mark.parametrize("n_handles", [2, 3])
def test_device_group_equals_one_handle(egg, n_handles):
    g = egg.SimulationGroup([0] * n_handles, cuts=CUTS[n_handles])
    h = egg.SimulationHandler()
    for s in (g, h):
        s.set_solver_order("relaxed")
        s.set_colliders(CONTAINER)
        s.set_forces(GRAVITY)
    ids = [g.add(x, y) for x, y in EGGS]
    assert [h.add(x, y) for x, y in EGGS] == ids and len({g.owner(i)[0] for i in ids}) == n_handles
    for k, records in enumerate(_group_lists(ids)):
        g.step(H60, S, C)
        h.step(H60, S, C)
        want = h.impulse(records)
        assert g.impulse(records) == want and min(want[0].count) > 0, k
        for w in (WHITE, YOLK):
            for f in FIELDS:
                assert np.array_equal(g.download(w, f).view(np.uint64), h.download(w, f).view(np.uint64)), (k, w, f)
    g.step(H60, S, C)
    h.step(H60, S, C)
    for w in (WHITE, YOLK):
        for f in FIELDS:
            assert np.array_equal(g.download(w, f).view(np.uint64), h.download(w, f).view(np.uint64)), ("after", w, f)
    before = [g.download(w, f) for w in (WHITE, YOLK) for f in FIELDS]
    with pytest.raises(egg.EggError, match="no batch with id `77`"):
        g.impulse([GROUP_RECORDS[0], ("kick", ("disc", 0.0, 0.0, 1e4), 1.0, 1.0, dict(id=77))])
    with pytest.raises(egg.EggError, match="record 1"):
        g.impulse([GROUP_RECORDS[0], ("brake", ("disc", 0.0, 0.0, 1e4), 0.0, 0.0, 2.0)])
    assert all(np.array_equal(a, b) for a, b in zip(before, [g.download(w, f) for w in (WHITE, YOLK) for f in FIELDS]))


# ------------------------------------------------------------------------------------------------ sharded
SHARDED_CUTS = [-2000.0, 335.0, 2.0 ** 41]


def _worker(rank, world, port, q):
    import os
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from egg_fluid_simulation_amd import EggError, SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler, SlabLayout
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sh = ShardedSimulationHandler(SlabLayout(SHARDED_CUTS), rank, dist, lambda: SimulationHandler(device=0), device="cpu")
        sh.set_solver_order("relaxed")
        sh.set_colliders(CONTAINER)
        sh.set_forces(GRAVITY)
        ids = [sh.add(x, y, 50, 15) for x, y in EGGS]
        steps = []
        for records in _group_lists(ids):
            sh.step(H60, S, C)
            got = sh.impulse(records)
            own = {gid: {(w, f): sh.local.download(w, f)[sh.local.download(w, "batch_id") == lid].tobytes()
                         for w in (WHITE, YOLK) for f in FIELDS} for gid, lid in sh.local_id.items()}
            steps.append(dict(results=[tuple(r) for r in got], own=own))
        errors = []
        for bad in ([GROUP_RECORDS[0], ("kick", ("disc", 0.0, 0.0, 1e4), 1.0, 1.0, dict(id=77))],
                    [GROUP_RECORDS[0], ("brake", ("disc", 0.0, 0.0, 1e4), 0.0, 0.0, 2.0)]):
            try:
                sh.impulse(bad)
                errors.append("accepted")
            except EggError as e:
                errors.append(str(e))
        q.put((rank, "ok", dict(steps=steps, errors=errors)))
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
    """two ranks on one GPU (three processes with the GPU open): the all-reduced totals are one handle's on both ranks, and
    every particle a rank owns has the bits one handle leaves in it"""
    res = _spawn(2)
    h = egg.SimulationHandler()
    h.set_solver_order("relaxed")
    h.set_colliders(CONTAINER)
    h.set_forces(GRAVITY)
    ids = [h.add(x, y, 50, 15) for x, y in EGGS]
    for k, records in enumerate(_group_lists(ids)):
        h.step(H60, S, C)
        want = h.impulse(records)
        bid = [h.download(w, "batch_id") for w in (WHITE, YOLK)]
        owned = set()
        for r in (0, 1):
            got = res[r]["steps"][k]
            assert got["results"] == [tuple(t) for t in want], (r, k)
            for gid, fields in got["own"].items():
                owned.add(gid)
                for (w, f), raw in fields.items():
                    assert raw == h.download(w, f)[bid[w] == gid].tobytes(), (r, k, gid, w, f)
        assert owned == set(ids) and all(res[r]["steps"][k]["own"] for r in (0, 1))  # (both ranks own batches)
    for r in (0, 1):
        assert "no batch with id `77`" in res[r]["errors"][0] and "record 1" in res[r]["errors"][1], res[r]["errors"]
