"""Sensors (egg_set_sensors) on the device against the CPU model tests/sensor_model.py: every
comparison is equality of integers, or of the doubles the stated formula derives from them.

The hand table of tests/test_sensor_model.py (particles placed through export_batch / import_batch), batch sizes on every
seam of the kernel (two lanes, a full wave, one more, a full unit, one more, three units), 64 sensors with a different
answer on every lane, masks that leave a type untouched, four default eggs after 5 relaxed and after 5 exact-order steps
against the model on the downloads, per-batch reads (permuted, repeated and unknown ids, moved atoms), reads around a step
in flight, sensors only observe, device groups of 2 and 3 handles on GPU 0 and a ShardedSimulationHandler of two spawned
ranks on GPU 0 over gloo."""
import numpy as np
import pytest

import sensor_model as sm
import test_sensor_model as ts
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


def _placed(egg, white, yolk):
    """(handle, id) of one batch whose particles sit at the given positions, at rest"""
    src = egg.SimulationHandler()
    i = src.add(0.0, 0.0, 50, 15, None, None, len(white), len(yolk))
    info, ws, ys = src.export_batch(i)
    for state, spots in ((ws, white), (ys, yolk)):
        assert state.shape[1] == len(spots)
        for p, (x, y) in enumerate(spots):
            state[0, p] = state[4, p] = x
            state[1, p] = state[5, p] = y
            state[2, p] = state[3, p] = 0.0
    h = egg.SimulationHandler()
    assert h.import_batch(info, ws, ys) == i
    return h, i


def _downloads(h):
    return ([h.download(w, "x") for w in (WHITE, YOLK)], [h.download(w, "y") for w in (WHITE, YOLK)],
            [h.download(w, "batch_id").astype(np.int64) for w in (WHITE, YOLK)])


def _assert_reads(h, sensors, what, ids=None):
    """every read of h is the model's over h's own downloads; returns the sums"""
    xs, ys, bid = _downloads(h)
    want = sm.read(sensors, xs, ys)
    got = h.sensor_sums()
    print("%s: %s dropped %s" % (what, got[0][:4], got[1]))
    assert got == want, what
    assert h.sensors() == sm.readings(want[0]), what
    ids = h.list_ids() if ids is None else ids
    per_batch = h.sensor_batches(ids)
    assert per_batch.dtype == np.int32 and np.array_equal(per_batch, sm.read_batches(sensors, xs, ys, bid, ids)), what
    return got


def _stored(sensors):
    types = {1: "white", 2: "yolk", 3: "both"}
    return [(kind,) + tuple(p[:sm.N_PARAMS[kind]]) + (types[mask],) for kind, mask, p in sm.canonical(sensors)]


# ------------------------------------------------------------------------------------------------ the hand table
@pytest.mark.parametrize("name", sorted(ts.CASES))
def test_hand_case(egg, name):
    case = ts.CASES[name]
    h, i = _placed(egg, *case["spots"])
    assert h.sensor_sums() == ([], [0, 0]) and h.sensors() == [] and h.sensor_batches([i]).shape == (1, 0, 2)
    h.set_sensors(case["sensors"])
    assert h.get_sensors() == _stored(case["sensors"])
    got = _assert_reads(h, case["sensors"], name)
    assert got == ts.expected(name)  # (and the hand-written membership, once more)
    h.set_sensors([])
    assert h.get_sensors() == [] and h.sensor_sums() == ([], [0, 0])


# ------------------------------------------------------------------------------------------------ the kernel's seams
SEAM_SENSORS = [("disc", 0.0, 0.0, 100.0), ("half_plane", 1.0, 0.0, 0.0, "white"), ("box", 10.0, 0.0, 30.0, 5.0, 0.3),
                ("capsule", -50.0, -20.0, 50.0, 20.0, 6.0, "yolk"), ("half_plane", -1.0, -1.0, 40.0)]


@pytest.mark.parametrize("n", [2, 64, 65, 1024, 1025, 2500])
def test_batch_sizes_on_every_seam(egg, n):
    """n particles per type on a line across every region's edge: lanes of a partly filled wave, the step to a second chunk,
    the unit boundary at 1,024 and three units"""
    t = np.arange(n, dtype=np.float64)
    white = list(zip(-130.0 + 260.0 * t / max(n - 1, 1), 0.125 * np.cos(t)))
    along = -120.0 + 240.0 * t / max(n - 1, 1)
    yolk = list(zip(along, 0.4 * along + 0.01 * np.sin(t)))  # (along the capsule's axis)
    h, i = _placed(egg, white, yolk)
    h.set_sensors(SEAM_SENSORS)
    sums, dropped = _assert_reads(h, SEAM_SENSORS, "n = %d" % n, [i, i])
    counts = [per_type[w][0] for per_type in sums for w in (0, 1)]
    assert dropped == [0, 0] and sum(1 for c in counts if 0 < c < n) >= (5 if n >= 64 else 1), counts  # (the edges cut the lines)


def test_64_sensors_with_a_different_answer_on_every_lane(egg):
    sensors = [("half_plane", 1.0, 0.0, 3.0 * k + 0.5, "white" if k % 3 == 0 else "both") for k in range(64)]
    white = [(1.0 * p, 5.0) for p in range(200)]
    yolk = [(2.0 * p, -5.0) for p in range(130)]
    h, _ = _placed(egg, white, yolk)
    h.set_sensors(sensors)
    sums, _ = _assert_reads(h, sensors, "64 sensors")
    assert len({per_type[WHITE] for per_type in sums}) == 64
    assert len({per_type[YOLK] for k, per_type in enumerate(sums) if k % 3}) == 64 - 22
    assert all(per_type[YOLK] == (0, 0, 0) for per_type in sums[::3])


def test_masks_that_leave_a_type_untouched(egg):
    white = [(1.0 * p, 0.0) for p in range(70)]
    yolk = [(1.0 * p, 1.0) for p in range(70)]
    h, _ = _placed(egg, white, yolk)
    for types, other in (("white", YOLK), ("yolk", WHITE)):
        sensors = [("disc", 0.0, 0.0, 30.5, types), ("half_plane", 1.0, 0.0, 60.0, types)]
        h.set_sensors(sensors)
        sums, _ = _assert_reads(h, sensors, types)
        assert [per_type[other] for per_type in sums] == [(0, 0, 0)] * 2
        assert [per_type[1 - other][0] for per_type in sums] == [31, 10]


# ------------------------------------------------------------------------------------------------ eggs that move
EGGS = ((300.0, 300.0), (360.0, 310.0), (330.0, 250.0), (420.0, 330.0))
EGG_SENSORS = [("disc", 330.0, 300.0, 60.0), ("disc", 360.0, 310.0, 25.0, "yolk"), ("box", 380.0, 320.0, 70.0, 30.0, 0.4),
               ("half_plane", 0.0, 1.0, 300.0), ("capsule", 250.0, 380.0, 450.0, 380.0, 40.0, "white"), ("half_plane", 1.0, 0.0, 345.0)]
CONTAINER = [("container", 350.0, 300.0, 140.0)]
GRAVITY = [("uniform", 0.0, 400.0)]


def _relaxed_scene(h):
    h.set_solver_order("relaxed")
    h.set_colliders(CONTAINER)
    h.set_forces(GRAVITY)
    return h


@pytest.mark.parametrize("order", ["relaxed", "exact"])
def test_four_eggs_after_five_steps(egg, order):
    h = egg.SimulationHandler()
    if order == "relaxed":
        _relaxed_scene(h)
    ids = [h.add(x, y) for x, y in EGGS]
    h.set_sensors(EGG_SENSORS)
    before = _assert_reads(h, EGG_SENSORS, order + ": before a step")
    for _ in range(5):
        assert h.update(H60, H60, S, C) == 1
    after = _assert_reads(h, EGG_SENSORS, order + ": after 5 steps", ids[::-1])
    assert before != after  # (something moved)
    assert all(per_type[w][0] > 0 for k, per_type in enumerate(after[0]) for w in (0, 1) if sm.canonical(EGG_SENSORS)[k][1] >> w & 1)


def test_sensor_batches_orders_unknown_ids_and_moved_atoms(egg):
    h = egg.SimulationHandler()
    ids = [h.add(x, y) for x, y in EGGS]
    h.set_sensors(EGG_SENSORS)
    xs, ys, bid = _downloads(h)
    order = [ids[2], ids[0], ids[3], ids[0], ids[1]]
    got = h.sensor_batches(order)
    assert np.array_equal(got, sm.read_batches(EGG_SENSORS, xs, ys, bid, order)) and np.array_equal(got[1], got[3]) and got.any()
    assert h.sensor_batches([]).shape == (0, len(EGG_SENSORS), 2)
    with pytest.raises(egg.EggError, match="no batch with id `99`"):
        h.sensor_batches([ids[0], 99])
    h.remove(ids[1])
    new = h.add(350.0, 290.0, 40, 12)
    with pytest.raises(egg.EggError, match="no batch with id `%d`" % ids[1]):
        h.sensor_batches([ids[1]])
    _assert_reads(h, EGG_SENSORS, "after remove and add", [new, ids[3], ids[0], ids[2]])


def test_reads_around_a_step_in_flight(egg):
    h = egg.SimulationHandler()
    ids = [h.add(x, y) for x, y in EGGS[:2]]
    h.set_sensors(EGG_SENSORS)
    held = h.sensor_sums(), h.sensor_batches(ids)
    h.step_begin(H60, S, C)
    with pytest.raises(egg.EggError, match="egg_read_sensors: a step is in flight"):
        h.sensor_sums()
    with pytest.raises(egg.EggError, match="egg_read_sensor_batches: a step is in flight"):
        h.sensor_batches(ids)
    with pytest.raises(egg.EggError, match="egg_set_sensors: a step is in flight"):
        h.set_sensors([])
    assert h.get_sensors() == _stored(EGG_SENSORS)
    h.step_end(False)
    assert h.sensor_sums() == held[0] and np.array_equal(h.sensor_batches(ids), held[1])
    h.step_begin(H60, S, C)
    h.step_end(True)
    assert _assert_reads(h, EGG_SENSORS, "after the committed step")[0] != held[0][0]


def test_a_bad_list_changes_nothing(egg):
    h, _ = _placed(egg, [(0.0, 0.0), (1.0, 1.0)], [(0.0, 0.0), (1.0, 1.0)])
    good = [("disc", 0.0, 0.0, 0.5)]
    h.set_sensors(good)
    for bad, index in (([("disc", 0.0, 0.0, 1.0), ("disc", 0.0, 0.0, -1.0)], 1), ([("half_plane", 0.0, 1e-9, 0.0)], 0),
                       ([("box", 0.0, 0.0, 1.0, 1.0, 0.0, 0.0)], 0), ([("capsule", 0.0, 0.0, 1.0, 1.0, float("nan"))], 0),
                       ([good[0]] * 3 + [("box", 0.0, 0.0, -1.0, 1.0, 0.0)], 3)):
        with pytest.raises(egg.EggError, match="sensor %d" % index):
            h.set_sensors(bad)
        assert h.get_sensors() == _stored(good) and h.sensor_sums()[0] == [((1, 0, 0), (1, 0, 0))]
    empty = egg.SimulationHandler()  # a handle without particles: zeros
    empty.set_sensors(good)
    assert empty.sensor_sums() == ([((0, 0, 0), (0, 0, 0))], [0, 0]) and empty.sensors() == [{"count": (0, 0), "centroid": (None, None)}]


def test_sensors_only_observe(egg):
    """the same relaxed scene with and without a list: equal particles, equal launches per step, and a read changes no step
    counter"""
    a, b = _relaxed_scene(egg.SimulationHandler()), _relaxed_scene(egg.SimulationHandler())
    for h in (a, b):
        for x, y in EGGS:
            h.add(x, y)
    a.set_sensors(EGG_SENSORS)
    launches = {id(a): [], id(b): []}
    for k in range(4):
        for h in (a, b):
            before = h.stats()["kernel_launches"]
            assert h.update(H60, H60, S, C) == 1
            launches[id(h)].append(h.stats()["kernel_launches"] - before)
        stats = a.stats()
        a.sensor_sums()
        a.sensor_batches(a.list_ids())
        assert a.stats()["steps"] == stats["steps"] == k + 1 and a.stats()["relaxed_steps"] == stats["relaxed_steps"]
        for w in (WHITE, YOLK):
            for f in FIELDS:
                assert np.array_equal(a.download(w, f), b.download(w, f)), (k, w, f)
    assert launches[id(a)] == launches[id(b)], launches
    assert a.collider_hits() == b.collider_hits() and a.elapsed == b.elapsed


# ------------------------------------------------------------------------------------------------ device groups
CUTS = {2: [-INF, 335.0, INF], 3: [-INF, 320.0, 372.0, INF]}  # through the eggs inside sensor 0
FAR_EGG = (2.0 ** 40, 300.0)  # its scaled x reaches 2^56: every sensor that holds it drops its particles


@pytest.mark.parametrize("n_handles", [2, 3])
def test_device_group_equals_one_handle(egg, n_handles):
    g = _relaxed_scene(egg.SimulationGroup([0] * n_handles, cuts=CUTS[n_handles]))
    h = _relaxed_scene(egg.SimulationHandler())
    ids = [g.add(x, y) for x, y in EGGS]
    assert [h.add(x, y) for x, y in EGGS] == ids
    assert len({g.owner(i)[0] for i in ids}) == n_handles
    for s in (g, h):
        s.set_sensors(EGG_SENSORS)
    assert g.get_sensors() == h.get_sensors() == _stored(EGG_SENSORS)
    for k in range(3):
        g.step(H60, S, C)
        h.step(H60, S, C)
        want = _assert_reads(h, EGG_SENSORS, "one handle, step %d" % (k + 1))
        assert g.sensor_sums() == want and g.sensors() == h.sensors(), k
        order = [ids[3], ids[0], ids[0], ids[2], ids[1]]
        assert np.array_equal(g.sensor_batches(order), h.sensor_batches(order)), k
        own = [b.sensor_sums()[0][0] for b in g.handles]
        assert sum(1 for per_type in own if per_type[WHITE][0] > 0) == n_handles, own  # (the cuts go through sensor 0)
    # dropped: an egg too far out to quantise, held by the half-planes that look right and down
    far = g.add(*FAR_EGG)
    assert h.add(*FAR_EGG) == far
    want = _assert_reads(h, EGG_SENSORS, "one handle with the far egg")
    assert min(want[1]) > 0 and g.sensor_sums() == want
    assert np.array_equal(g.sensor_batches([far] + ids), h.sensor_batches([far] + ids)) and not h.sensor_batches([far]).any()
    with pytest.raises(egg.EggError, match="no batch with id `77`"):
        g.sensor_batches([ids[0], 77])


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
        sh = _relaxed_scene(ShardedSimulationHandler(SlabLayout(SHARDED_CUTS), rank, dist, lambda: SimulationHandler(device=0), device="cpu"))
        ids = [sh.add(x, y, 50, 15) for x, y in EGGS]
        sh.set_sensors(EGG_SENSORS)
        order = [ids[3], ids[0], ids[0], ids[2], ids[1]]
        steps = []
        for _ in range(3):
            sh.step(H60, S, C)
            steps.append(dict(sums=sh.sensor_sums(), readings=sh.sensors(), batches=sh.sensor_batches(order).tolist(),
                              own=sh.local.sensor_sums()))
        far = sh.add(FAR_EGG[0], FAR_EGG[1], 50, 15)
        last = dict(sums=sh.sensor_sums(), batches=sh.sensor_batches([far] + ids).tolist(), far=far)
        try:
            sh.sensor_batches([ids[0], 77])
            last["unknown"] = "accepted"
        except EggError as e:
            last["unknown"] = str(e)
        q.put((rank, "ok", dict(steps=steps, last=last, stored=sh.get_sensors())))
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
    """two ranks on one GPU (three processes with the GPU open), the cut through the eggs inside sensor 0: the all-reduced
    integers are one handle's on both ranks, and each rank's own are a part of them"""
    res = _spawn(2)
    h = _relaxed_scene(egg.SimulationHandler())
    ids = [h.add(x, y, 50, 15) for x, y in EGGS]
    h.set_sensors(EGG_SENSORS)
    order = [ids[3], ids[0], ids[0], ids[2], ids[1]]
    for k in range(3):
        h.step(H60, S, C)
        want = _assert_reads(h, EGG_SENSORS, "one handle, step %d" % (k + 1))
        for r in (0, 1):
            got = res[r]["steps"][k]
            assert got["sums"] == want and got["readings"] == h.sensors(), (r, k)
            assert got["batches"] == h.sensor_batches(order).tolist(), (r, k)
        own = [res[r]["steps"][k]["own"] for r in (0, 1)]
        assert all(o[0][0][WHITE][0] > 0 for o in own), own  # (both ranks hold particles inside sensor 0)
        added = [tuple(tuple(a + b for a, b in zip(t0, t1)) for t0, t1 in zip(s0, s1)) for s0, s1 in zip(own[0][0], own[1][0])]
        assert added == want[0], k
    far = h.add(FAR_EGG[0], FAR_EGG[1], 50, 15)
    want = _assert_reads(h, EGG_SENSORS, "one handle with the far egg")
    assert min(want[1]) > 0
    for r in (0, 1):
        last = res[r]["last"]
        assert last["far"] == far and last["sums"] == want and last["batches"] == h.sensor_batches([far] + ids).tolist(), r
        assert "no batch with id `77`" in last["unknown"], last["unknown"]
        assert [tuple(s) for s in res[r]["stored"]] == _stored(EGG_SENSORS)
