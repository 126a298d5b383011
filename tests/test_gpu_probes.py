"""Probes (egg_probe) on the device against the CPU model tests/probe_model.py evaluated on the
handle's own downloads: every comparison is == field for field, there is no tolerance, the rule is exact.

The hand table of tests/test_probe_model.py (particles placed through export_batch / import_batch, keys against ids where
the table says so), batch sizes on every seam of the scan with the winner on every seam and exact ties across a chunk and
across a unit boundary, 64 probes with a different answer on every lane, masks, four default eggs after five steps in both
solver orders, coincident batches, calls around a step in flight, the refusals of the C ABI with the caller's hits
untouched, probes only observe, device groups of 2 and 3 handles on GPU 0 and a ShardedSimulationHandler of two spawned
ranks on GPU 0 over gloo."""
import ctypes as C
import warnings

import numpy as np
import pytest

import probe_model as pm
import test_probe_model as tp
from conftest import ROOT

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
FIELDS = ("x", "y", "vx", "vy", "last_x", "last_y")
H60, S, CS = 1 / 60, 2, 3
INF = float("inf")


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


_templates = {}


def _template(egg, nw, ny):
    """(info, white_state, yolk_state) of a batch of nw + ny particles as export_batch gives it"""
    if (nw, ny) not in _templates:
        src = egg.SimulationHandler()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", egg.EggWarning)  # ("only 2 particles will be created": that is the point)
            i = src.add(0.0, 0.0, 50, 15, None, None, max(nw, 2), max(ny, 2))  # (a batch is added with at least 2 of a type)
        info, ws, ys = src.export_batch(i)
        _templates[nw, ny] = (dict(info, n_white=nw, n_yolk=ny), ws[:, :nw].copy(), ys[:, :ny].copy())
    return _templates[nw, ny]


def _scene(egg, batches):
    """(handle, ids): the batches -- dict(key, white, yolk), a particle (x, y, radius) -- imported in the list's order, at rest"""
    h = egg.SimulationHandler()
    ids = []
    for b in batches:
        info, ws, ys = _template(egg, len(b["white"]), len(b["yolk"]))
        ws, ys = ws.copy(), ys.copy()
        for state, spots in ((ws, b["white"]), (ys, b["yolk"])):
            for p, (x, y, r) in enumerate(spots):
                state[0, p] = state[4, p] = x
                state[1, p] = state[5, p] = y
                state[2, p] = state[3, p] = 0.0
                state[7, p] = r
        ids.append(h.import_batch(dict(info, key=b["key"]), ws, ys))
    return h, ids


def _particles(h):
    """the model's view of a handle: its downloads, the keys from export_batch"""
    key_of = {i: h.export_batch(i)[0]["key"] for i in h.list_ids()}
    return tuple(pm.particles_of(h.download(w, "x"), h.download(w, "y"), h.download(w, "radius"), h.download(w, "batch_id"), key_of)
                 for w in (WHITE, YOLK))


def _plain(hits):
    return [tuple(None if t is None else tuple(t) for t in pair) for pair in hits]


def _assert_probes(h, probes, what):
    """h.probe is the model's answer over h's own downloads; returns it"""
    want = pm.probe(probes, _particles(h))
    got = h.probe(probes)
    print("%s: %s" % (what, got[:3]))
    assert _plain(got) == want, what
    for pair in got:
        for t in pair:
            assert t is None or (t._fields == ("id", "index", "score", "x", "y", "radius") and type(t.id) is int and type(t.score) is float)
    return want


# ------------------------------------------------------------------------------------------------ the hand table
@pytest.mark.parametrize("name", sorted(tp.CASES))
def test_hand_case(egg, name):
    case = tp.CASES[name]
    h, ids = _scene(egg, case["batches"])
    assert ids == list(range(1, len(ids) + 1))
    got = _assert_probes(h, case["probes"], name)
    assert got == tp.expected(name, ids)  # (and the hand-written winners, once more)
    for probe, pair, first in zip(pm.canonical(case["probes"]), got, case["first"]):
        kind, mask, p = probe
        if kind == "point":
            found = h.pick(p[0], p[1], p[2], mask)
            assert found == pm.first(pair) and (None if found is None else found[0]) == first
        else:
            found = h.raycast(p[0], p[1], p[2], p[3], p[4], mask)
            want = pm.first(pair)
            assert found == (None if want is None else want + (pm.impact(p, want[1][2]),)) and (None if found is None else found[0]) == first


# ------------------------------------------------------------------------------------------------ the scan's seams
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_batch_sizes_on_every_seam(egg, n):
    """n particles per type on a line, one pixel apart.  The unique winner in turn at the first lane, the last lane of a
    chunk, the first particle of a unit's second chunk, the last particle of the batch and the first particle of the second
    unit; then exact ties between the neighbours across a chunk boundary (63 | 64: one wave holds both) and across a unit
    boundary (1023 | 1024: two waves hold one each)."""
    white = [(1.0 * i, 0.0, 0.25) for i in range(n)]
    yolk = [(1.0 * i, 100.0, 0.25) for i in range(n)]
    h, _ = _scene(egg, [dict(key=1, white=white, yolk=yolk)])
    winners = [i for i in (0, 63, 64, n - 1, 1024) if i < n]
    probes, wanted = [], []
    for i in winners:
        probes += [("point", i + 0.25, 50.0), ("point", i - 0.25, 0.125, 0.5, "white"), ("ray", 1.0 * i, 105.0, 1.0 * i, -5.0)]
        wanted += [(i, i), (i, None), (i, i)]
    for i in (63, 1023):  # particles i and i + 1 tie exactly: d2 = 0.25, and t = 0 for a ray that starts inside both padded discs
        if i + 1 < n:
            probes += [("point", i + 0.5, 0.0), ("point", i + 0.5, 100.0, 0.5, "yolk"), ("ray", i + 0.5, 0.0, i + 0.5, 100.0, 0.25)]
            wanted += [(i, i), (None, i), (i, i)]
    got = _assert_probes(h, probes, "n = %d" % n)
    assert [tuple(None if t is None else t[1] for t in pair) for pair in got] == wanted
    if n > 1024:
        tie = got[len(winners) * 3 + 3]
        assert tie[WHITE][2] == 0.25 and tie[YOLK][2] == 10000.25


def test_64_probes_with_a_different_answer_on_every_lane(egg):
    white = [(3.0 * p, 0.0, 1.0) for p in range(200)]
    yolk = [(3.0 * p + 1.0, 50.0, 1.0) for p in range(130)]
    h, _ = _scene(egg, [dict(key=1, white=white, yolk=yolk)])
    probes = [("point", 15.0 * k + 0.5, 0.25) for k in range(32)] + \
             [("ray", 15.0 * k + 6.5, 80.0, 15.0 * k + 6.5, -10.0, 0.0, "both" if k % 3 else "white") for k in range(32)]
    got = _assert_probes(h, probes, "64 probes")
    assert len(set(got)) == 64
    assert [pair[WHITE][1] for pair in got] == [5 * k for k in range(32)] + [5 * k + 2 for k in range(32)]
    assert [None if pair[YOLK] is None else pair[YOLK][1] for pair in got[32:]] == [5 * k + 2 if k % 3 and 5 * k + 2 < 130 else None for k in range(32)]


def test_masks_that_leave_a_type_untouched(egg):
    white = [(1.0 * p, 0.0, 0.5) for p in range(70)]
    yolk = [(1.0 * p, 1.0, 0.5) for p in range(70)]
    h, _ = _scene(egg, [dict(key=1, white=white, yolk=yolk)])
    for types, other in (("white", YOLK), ("yolk", WHITE)):
        probes = [("point", 30.25, 0.5, INF, types), ("ray", 65.0, -5.0, 65.0, 5.0, 0.0, types), ("point", 500.0, 0.0, 1.0, types)]
        got = _assert_probes(h, probes, types)
        assert [pair[other] for pair in got] == [None] * 3  # (no unit of the other type is scanned)
        assert [None if pair[1 - other] is None else pair[1 - other][1] for pair in got] == [30, 65, None]


# ------------------------------------------------------------------------------------------------ eggs that move
EGGS = ((300.0, 300.0), (360.0, 310.0), (330.0, 250.0), (420.0, 330.0))
EGG_PROBES = [("point", 330.0, 300.0), ("point", 330.0, 300.0, 3.0), ("point", 0.0, 0.0), ("point", 360.0, 310.0, INF, "yolk"),
              ("point", 1000.0, 1000.0, 32.0), ("point", 420.0, 330.0, 32.0, "white"), ("point", 345.0, 280.0, 0.0),
              ("point", 300.5, 299.5, 8.0),
              ("ray", 100.0, 300.0, 600.0, 300.0), ("ray", 600.0, 310.0, 100.0, 290.0, 2.0), ("ray", 330.0, 100.0, 330.0, 500.0, 0.0, "yolk"),
              ("ray", 330.0, 305.0, 400.0, 305.0, 20.0), ("ray", 100.0, 100.0, 150.0, 150.0), ("ray", 100.0, 100.0, 600.0, 600.0, 0.5, "white"),
              ("ray", 420.0, 500.0, 420.0, 330.0), ("ray", 0.0, 0.0, 1000.0, 1000.0, 1000.0)]
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
    for x, y in EGGS:
        h.add(x, y)
    assert len(EGG_PROBES) == 16
    before = _assert_probes(h, EGG_PROBES, order + ": before a step")
    for _ in range(5):
        assert h.update(H60, H60, S, CS) == 1
    after = _assert_probes(h, EGG_PROBES, order + ": after 5 steps")
    assert before != after  # (something moved)
    assert after[0][WHITE] is not None and after[8][WHITE] is not None and after[15] == ((1, 0, 0.0) + after[15][WHITE][3:],
                                                                                        (1, 0, 0.0) + after[15][YOLK][3:])
    assert h.pick(330.0, 300.0) == pm.first(after[0]) and h.pick(1000.0, 1000.0, 32.0) is None
    hit = h.raycast(100.0, 300.0, 600.0, 300.0)
    assert hit == pm.first(after[8]) + (pm.impact(EGG_PROBES[8][1:], pm.first(after[8])[1][2]),)


def test_coincident_batches(egg):
    """two eggs added at the same place, probed before any step: every particle has a twin at its own position in the other
    batch, and the twin of the lower key wins"""
    h = egg.SimulationHandler()
    a, b = h.add(300.0, 300.0), h.add(300.0, 300.0)
    got = _assert_probes(h, EGG_PROBES, "coincident")
    parts = _particles(h)
    for w in (WHITE, YOLK):
        n = parts[w]["x"].size // 2
        if np.array_equal(parts[w]["x"][:n], parts[w]["x"][n:]) and np.array_equal(parts[w]["y"][:n], parts[w]["y"][n:]):
            assert all(pair[w] is None or pair[w][0] == a for pair in got), w
        else:
            pytest.skip("the two batches do not coincide")  # (the comparison with the model above has been made)
    assert a < b and any(pair[WHITE] is not None for pair in got)


def test_calls_around_a_step_in_flight(egg):
    h = egg.SimulationHandler()
    for x, y in EGGS[:2]:
        h.add(x, y)
    held = h.probe(EGG_PROBES)
    state = [h.download(w, f) for w in (WHITE, YOLK) for f in FIELDS]
    h.step_begin(H60, S, CS)
    with pytest.raises(egg.EggError, match=r"egg_probe: a step is in flight \(egg_step_begin without egg_step_end\)"):
        h.probe(EGG_PROBES)
    with pytest.raises(egg.EggError, match="egg_probe: a step is in flight"):
        h.pick(330.0, 300.0)
    h.step_end(False)
    assert all(np.array_equal(a, b) for a, b in zip(state, [h.download(w, f) for w in (WHITE, YOLK) for f in FIELDS]))
    assert h.probe(EGG_PROBES) == held
    h.step_begin(H60, S, CS)
    h.step_end(True)
    assert _assert_probes(h, EGG_PROBES, "after the committed step") != _plain(held)


def _raw(h, n, records, hits):
    arr = None
    if records is not None:
        arr = (h._lib.egg_probe.argtypes[2]._type_ * max(len(records), 1))()
        for k, (kind, mask, p) in enumerate(records):
            arr[k].kind, arr[k].type_mask = kind, mask
            for i, v in enumerate(p):
                arr[k].p[i] = v
    return h._lib.egg_probe(h._h, n, arr, hits)


def test_a_bad_list_leaves_the_hits_as_the_caller_filled_them(egg):
    from egg_fluid_simulation_amd import _ffi
    h, _ = _scene(egg, [dict(key=1, white=[(0.0, 0.0, 1.0), (3.0, 4.0, 1.0)], yolk=[(0.0, 0.0, 1.0), (1.0, 1.0, 1.0)])])
    good = (0, 3, [0.0, 0.0, INF, 0.0, 0.0])
    nan = float("nan")

    def filled():
        hits = (_ffi.EggProbeHit * 130)()
        C.memset(hits, 0x5A, C.sizeof(hits))
        return hits

    untouched = bytes(filled())
    for n, records, text in ((-1, [good], "n = -1"), (65, [good] * 65, "n = 65"), (1, None, "n = 1 without a list"),
                             (2, [good, (2, 3, [0.0] * 5)], "probe 1: unknown kind 2"), (1, [(-1, 3, [0.0] * 5)], "probe 0: unknown kind"),
                             (3, [good, good, (0, 0, [0.0, 0.0, 1.0, 0.0, 0.0])], "probe 2: type_mask 0"),
                             (1, [(1, 4, [0.0, 0.0, 1.0, 1.0, 0.0])], "probe 0: type_mask 4"),
                             (2, [good, (0, 3, [nan, 0.0, 1.0, 0.0, 0.0])], r"probe 1 \(point\): parameter 0 is a NaN"),
                             (1, [(1, 3, [0.0, 0.0, 1.0, 1.0, nan])], r"probe 0 \(ray\): parameter 4 is a NaN"),
                             (1, [(0, 3, [0.0, INF, 1.0, 0.0, 0.0])], r"probe 0 \(point\): parameter 1 is not finite"),
                             (1, [(0, 3, [0.0, 0.0, -INF, 0.0, 0.0])], r"probe 0 \(point\): parameter 2 is not finite"),
                             (1, [(1, 3, [0.0, 0.0, INF, 1.0, 0.0])], r"probe 0 \(ray\): parameter 2 is not finite"),
                             (1, [(1, 3, [0.0, 0.0, 1.0, 1.0, INF])], r"probe 0 \(ray\): parameter 4 is not finite"),
                             (2, [good, (0, 1, [0.0, 0.0, -1.0, 0.0, 0.0])], r"probe 1 \(point\): reach -1 is negative"),
                             (1, [(1, 2, [0.0, 0.0, 1.0, 1.0, -0.5])], r"probe 0 \(ray\): pad -0.5 is negative"),
                             (2, [good, (1, 3, [2.0, 3.0, 2.0, 3.0, 0.0])], r"probe 1 \(ray\): degenerate"),
                             (1, [(1, 3, [0.0, 0.0, 0.5e-8, 0.0, 0.0])], r"probe 0 \(ray\): degenerate")):
        hits = filled()
        with pytest.raises(egg.EggError, match="egg_probe: " + text):
            h._check(_raw(h, n, records, hits))
        assert bytes(hits) == untouched, text
    with pytest.raises(egg.EggError, match="egg_probe: n = 1 without hits"):
        h._check(_raw(h, 1, [good], None))
    hits = filled()
    assert _raw(h, 0, [good], hits) == 0 and _raw(h, 0, None, None) == 0 and bytes(hits) == untouched  # (n == 0 writes nothing)
    # parameters a kind does not use are ignored; a ray of exactly eps is a ray; the answer takes 2 n records, not one more
    assert _raw(h, 2, [(0, 3, [0.0, 0.0, INF, nan, -INF]), (1, 3, [0.0, 500.0, 1e-8, 500.0, 0.0])], hits) == 0
    assert bytes(hits)[4 * C.sizeof(_ffi.EggProbeHit):] == untouched[4 * C.sizeof(_ffi.EggProbeHit):]
    assert [(t.found, t.id, t.key, t.index, t.score) for t in hits[:4]] == [(1, 1, 1, 0, 0.0), (1, 1, 1, 0, 0.0), (0, 0, 0, 0, 0.0), (0, 0, 0, 0, 0.0)]
    # the wrappers' own checks, and a handle without particles: found = 0 everywhere
    with pytest.raises(egg.EggError, match="probe 1: kind must be one of point, ray"):
        h.probe([("point", 0.0, 0.0), ("disc", 0.0, 0.0, 1.0)])
    empty = egg.SimulationHandler()
    hits = filled()
    assert _raw(empty, 2, [good, good], hits) == 0 and bytes(hits)[:4 * C.sizeof(_ffi.EggProbeHit)] == bytes(4 * C.sizeof(_ffi.EggProbeHit))
    assert empty.probe([("point", 0.0, 0.0), ("ray", 0.0, 0.0, 1.0, 1.0)]) == [(None, None)] * 2 and empty.pick(0.0, 0.0) is None


def test_probes_only_observe(egg):
    """the same relaxed scene with and without probe calls: equal particles, equal launches per step; 100 calls change no
    position and no counter"""
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
        stats = a.stats()
        state = [a.download(w, f) for w in (WHITE, YOLK) for f in FIELDS]
        first = a.probe(EGG_PROBES)
        for _ in range(99):
            assert a.probe(EGG_PROBES) == first
        assert a.stats() == stats and a.stats()["steps"] == k + 1
        assert all(np.array_equal(p, q) for p, q in zip(state, [a.download(w, f) for w in (WHITE, YOLK) for f in FIELDS]))
        for w in (WHITE, YOLK):
            for f in FIELDS:
                assert np.array_equal(a.download(w, f), b.download(w, f)), (k, w, f)
    assert launches[id(a)] == launches[id(b)], launches
    assert a.collider_hits() == b.collider_hits() and a.elapsed == b.elapsed


# ------------------------------------------------------------------------------------------------ device groups
CUTS = {2: [-INF, 335.0, INF], 3: [-INF, 320.0, 372.0, INF]}
# the ray that starts inside many padded discs of both overlapping eggs, and the one that starts inside every disc: all tie
# at t = 0, so the winner is particle 0 of the oldest batch, whichever handle owns it
TIED = (11, 15)


@pytest.mark.parametrize("n_handles,eggs", [(2, EGGS[1::-1] + EGGS[2:]), (3, EGGS)])
def test_device_group_equals_one_handle(egg, n_handles, eggs):
    g = _relaxed_scene(egg.SimulationGroup([0] * n_handles, cuts=CUTS[n_handles]))
    h = _relaxed_scene(egg.SimulationHandler())
    ids = [g.add(x, y) for x, y in eggs]
    assert [h.add(x, y) for x, y in eggs] == ids
    owners = [g.owner(i)[0] for i in ids]
    assert len(set(owners)) == n_handles and owners[0] != owners[1]  # (the two overlapping eggs live on different handles)
    for k in range(3):
        want = _assert_probes(h, EGG_PROBES, "one handle, step %d" % k)
        assert _plain(g.probe(EGG_PROBES)) == want, k
        assert want[TIED[0]][WHITE][0] == ids[0] and want[TIED[0]][WHITE][2] == 0.0
        assert want[TIED[1]][WHITE][:3] == (ids[0], 0, 0.0) and want[TIED[1]][YOLK][:3] == (ids[0], 0, 0.0)
        own = [b.probe(EGG_PROBES) for b in g.handles]
        assert len({(None if o[TIED[1]][WHITE] is None else o[TIED[1]][WHITE].score) for o in own}) == 1  # (every handle holds a tied one)
        assert g.pick(330.0, 300.0) == h.pick(330.0, 300.0) and g.raycast(100.0, 300.0, 600.0, 300.0) == h.raycast(100.0, 300.0, 600.0, 300.0)
        g.step(H60, S, CS)
        h.step(H60, S, CS)
    with pytest.raises(egg.EggError, match=r"probe 0 \(ray\): degenerate"):
        g.probe([("ray", 1.0, 1.0, 1.0, 1.0)])
    assert g.probe([]) == []


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
        for x, y in EGGS[1::-1] + EGGS[2:]:
            sh.add(x, y, 50, 15)
        steps = []
        for _ in range(3):
            steps.append(dict(hits=_plain(sh.probe(EGG_PROBES)), own=_plain(sh.local.probe(EGG_PROBES)), pick=sh.pick(330.0, 300.0),
                              ray=sh.raycast(100.0, 300.0, 600.0, 300.0)))
            sh.step(H60, S, CS)
        q.put((rank, "ok", dict(steps=steps, empty=sh.probe([]))))
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
    """two ranks on one GPU (three processes with the GPU open), the cut between the two overlapping eggs, the older of which
    lives on rank 1: the gathered and selected hits are one handle's on both ranks, ties included"""
    res = _spawn(2)
    h = _relaxed_scene(egg.SimulationHandler())
    ids = [h.add(x, y, 50, 15) for x, y in EGGS[1::-1] + EGGS[2:]]
    for k in range(3):
        want = _assert_probes(h, EGG_PROBES, "one handle, step %d" % k)
        for r in (0, 1):
            got = res[r]["steps"][k]
            assert got["hits"] == want, (r, k)
            assert got["pick"] == h.pick(330.0, 300.0) and got["ray"] == h.raycast(100.0, 300.0, 600.0, 300.0), (r, k)
        own = [res[r]["steps"][k]["own"] for r in (0, 1)]
        assert all(o[TIED[1]][WHITE] is not None and o[TIED[1]][WHITE][2] == 0.0 for o in own), own  # (both ranks hold a tied particle)
        assert want[TIED[1]][WHITE][:2] == (ids[0], 0)
        h.step(H60, S, CS)
    assert res[0]["empty"] == [] and res[1]["empty"] == []
