"""Pieces (egg_pieces) on the device against the CPU model tests/pieces_model.py evaluated on the
handle's own downloads: every comparison is ==, there is no tolerance, every output is an integer.

The hand table of tests/test_pieces_model.py (particles placed through export_batch / import_batch), atom sizes on every
seam of the two launch classes with the chain broken at the first lane, the last lane and a chunk boundary, an atom over
the cap, four default eggs after five steps in both solver orders, ids repeated and reversed, masks, piece_labels, calls
around a step in flight, the refusals of the C ABI with the caller's buffers untouched, a call only observes, device groups
of 2 and 3 handles on GPU 0 and a ShardedSimulationHandler of two spawned ranks on GPU 0 over gloo."""
import ctypes as C

import numpy as np
import pytest

import pieces_model as pm
import test_pieces_model as tp
from conftest import ROOT
from test_gpu_probes import _scene

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
FIELDS = ("x", "y", "vx", "vy", "last_x", "last_y", "radius", "batch_id")
H60, S, CS = 1 / 60, 2, 3
INF = float("inf")
MASKS = {"both": 3, "white": 1, "yolk": 2}
WAVE_ATOM, BLOCK = 512, 256  # EGG_PC_WAVE_ATOM, EGG_PC_BLOCK: the largest atom of the one-wave class, the threads of the other


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _particles(h):
    """the model's view of a handle: its downloads"""
    return tuple({k: h.download(w, k) for k in ("x", "y", "radius", "batch_id")} for w in (WHITE, YOLK))


def _reach(h, reach):
    spec = h._c_pieces_spec(reach, "both")
    return (spec.reach[0], spec.reach[1])


def _assert_pieces(h, ids, reach, types, what, parts=None):
    """h.pieces is the model's answer over h's own downloads, record for record; returns the model's records"""
    parts = _particles(h) if parts is None else parts
    listed = h.list_ids() if ids is None else list(ids)
    want, _ = pm.pieces(parts, listed, _reach(h, reach), MASKS[types])
    got = h.pieces(ids, reach, types)
    print("%s: %s" % (what, got[:2]))
    assert [tuple(None if t is None else tuple(t) for t in pair) for pair in got] == [tuple(pm.summary(r) for r in pair) for pair in want], what
    raw = h._piece_table(h._c_pieces_spec(reach, types), None if ids is None else np.ascontiguousarray(listed, dtype=np.int64))
    assert [tuple(tuple(int(v) for v in rec) for rec in pair) for pair in raw] == want, what
    for pair in got:
        for t in pair:
            assert t is None or (t._fields == ("n", "pieces", "largest", "first", "singles", "dropped", "x", "y") and type(t.n) is int)
    return want


def _assert_labels(h, reach, types, what, parts=None):
    parts = _particles(h) if parts is None else parts
    _, want = pm.pieces(parts, h.list_ids(), _reach(h, reach), MASKS[types])
    got = h.piece_labels(reach, types)
    for w in (WHITE, YOLK):
        assert got[w].dtype == np.int32 and np.array_equal(got[w], want[w]), (what, w)
    return want


# ------------------------------------------------------------------------------------------------ the hand table
@pytest.mark.parametrize("name", sorted(tp.CASES))
def test_hand_case(egg, name):
    case = tp.CASES[name]
    h, ids = _scene(egg, case["batches"])
    assert ids == list(range(1, len(ids) + 1))
    parts = _particles(h)
    assert _assert_pieces(h, None, case["reach"], "both", name, parts) == case["records"]  # (the model's and the hand-written ones)
    assert _assert_pieces(h, ids[::-1], case["reach"], "both", name + ", reversed", parts) == case["records"][::-1]
    _assert_labels(h, case["reach"], "both", name, parts)
    for i, rec in zip(ids, case["records"]):
        assert h.is_whole(i, case["reach"]) == all(r[1] == 1 for r in rec)
        assert h.is_whole(i, case["reach"], "white") == (rec[0][1] == 1) and h.is_whole(i, case["reach"], "yolk") == (rec[1][1] == 1)


# ------------------------------------------------------------------------------------------------ the seams of the launch classes
def _chain(n, gap_after):
    """n particles of radius 4 on a line, 7 apart (linked under reach 1), index = position, with a gap behind particle
    `gap_after` (None: no gap)"""
    return [(7.0 * p + (100.0 if gap_after is not None and p > gap_after else 0.0), 0.0, 4.0) for p in range(n)]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4095, 4096])
def test_atom_sizes_on_every_seam(egg, n):
    """A lane of the one-wave class owns the particles t, t + 64, ..; a thread of the other class t, t + 256, ..; atoms above
    512 particles take the second class, 4,096 is the cap.  Per size three white chains, broken behind the first lane, before
    the last lane and at a chunk boundary of the class, and one unbroken yolk chain of the same size."""
    chunk = 64 if n <= WAVE_ATOM else BLOCK
    breaks = [g for g in (0, n - 2, chunk - 1) if 0 <= g < n - 1]
    batches = [dict(key=1, white=_chain(n, None), yolk=_chain(n, None))]
    batches += [dict(key=2 + k, white=_chain(n, g), yolk=[(0.0, 50.0, 4.0)]) for k, g in enumerate(breaks)]
    h, ids = _scene(egg, batches)
    parts = _particles(h)
    before = h.stats()["kernel_launches"]
    want = _assert_pieces(h, None, 1.0, "both", "n = %d" % n, parts)
    launches = (h.stats()["kernel_launches"] - before) // 2  # (_assert_pieces calls twice)
    assert launches == (2 if n > WAVE_ATOM else 1)  # (the single yolk particles are of the one-wave class)
    assert want[0] == ((n, 1, n, 0, int(n == 1), 0, 7 * 65536 * (n * (n - 1) // 2), 0),) * 2
    for k, g in enumerate(breaks):
        head, rest = g + 1, n - g - 1
        rec = want[1 + k][WHITE]
        assert rec[:5] == (n, 2, max(head, rest), 0 if head >= rest else head, (head == 1) + (rest == 1)), (n, g)
    labels = _assert_labels(h, 1.0, "both", "n = %d" % n, parts)
    assert labels[WHITE][:n].max() == 0


def test_an_atom_over_the_cap_is_refused_and_nothing_is_written(egg):
    from egg_fluid_simulation_amd import _ffi
    h, ids = _scene(egg, [dict(key=1, white=_chain(4097, None), yolk=[(0.0, 50.0, 4.0), (6.0, 50.0, 4.0)]),
                          dict(key=2, white=_chain(5, 1), yolk=[(0.0, 90.0, 4.0)])])
    assert _ffi.PIECES_MAX_ATOM == 4096
    with pytest.raises(egg.EggError, match=r"egg_pieces: batch `1` has 4097 white particles, an atom holds at most 4096"):
        h.pieces()
    with pytest.raises(egg.EggError, match="batch `1` has 4097 white particles"):
        h.pieces([2, 1], 1.0)
    with pytest.raises(egg.EggError, match="batch `1` has 4097 white particles"):
        h.piece_labels(1.0)
    spec = h._c_pieces_spec(1.0, "both")
    out = (_ffi.EggPieceSummary * 4)()
    C.memset(out, 0x5A, C.sizeof(out))
    untouched = bytes(out)
    lw, ly = np.full(4102, 77, dtype=np.int32), np.full(3, 77, dtype=np.int32)
    before = h.stats()
    assert h._lib.egg_pieces(h._h, C.byref(spec), 0, None, out, lw.ctypes.data, ly.ctypes.data) == _ffi.EGG_ERR_UNSUPPORTED
    assert bytes(out) == untouched and (lw == 77).all() and (ly == 77).all() and h.stats() == before
    # a call that leaves that batch -- or that type -- out succeeds
    parts = _particles(h)
    assert _assert_pieces(h, [2], 1.0, "both", "the small batch", parts) == [((5, 2, 3, 2, 0, 0, (14 + 21 + 28 + 300) * 65536, 0),
                                                                             (1, 1, 1, 0, 1, 0, 0, 90 * 65536))]
    assert _assert_pieces(h, None, 1.0, "yolk", "yolk only", parts)[0] == (pm.ZERO, (2, 1, 2, 0, 0, 0, 6 * 65536, 100 * 65536))
    assert h.is_whole(1, 1.0, "yolk") and not h.is_whole(2, 1.0)
    _assert_labels(h, 1.0, "yolk", "yolk labels", parts)


# ------------------------------------------------------------------------------------------------ eggs that move
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


@pytest.mark.parametrize("order", ["relaxed", "exact"])
def test_four_eggs_after_five_steps(egg, order):
    h, ids = _four_eggs(egg, order)
    assert _reach(h, None) == (2.0, 3.0)  # max(collision_overlap_factor, cohesion_interaction_distance_factor) of the default config
    start = _assert_pieces(h, None, None, "both", order + ": before a step")
    assert all(rec[1] == 1 and rec[2] == rec[0] for pair in start for rec in pair)  # (a fresh egg is whole under the default reach)
    assert all(h.is_whole(i) for i in ids)
    for _ in range(5):
        assert h.update(H60, H60, S, CS) == 1
    parts = _particles(h)
    after = _assert_pieces(h, None, None, "both", order + ": after 5 steps, default reach", parts)
    tight = _assert_pieces(h, None, 1.0, "both", order + ": after 5 steps, reach 1", parts)
    assert start != after and tight != after
    assert _assert_pieces(h, None, (1.0, 3.0), "both", order + ": reach per type", parts) == [(t[0], a[1]) for t, a in zip(tight, after)]
    _assert_labels(h, None, "both", order, parts)
    _assert_labels(h, 1.0, "both", order + ", reach 1", parts)
    for i, pair in zip(ids, tight):
        assert h.is_whole(i, 1.0) == all(rec[1] == 1 for rec in pair)


def test_ids_repeated_and_in_reverse_order(egg):
    h, ids = _four_eggs(egg, "relaxed")
    for _ in range(2):
        h.update(H60, H60, S, CS)
    parts = _particles(h)
    every = _assert_pieces(h, None, 1.25, "both", "every batch", parts)
    assert _assert_pieces(h, ids[::-1], 1.25, "both", "reversed", parts) == every[::-1]
    listed = [ids[2], ids[0], ids[2], ids[2], ids[3], ids[0]]
    assert _assert_pieces(h, listed, 1.25, "both", "repeated", parts) == [every[ids.index(i)] for i in listed]
    assert h.pieces([], 1.25) == []
    assert _assert_pieces(h, None, 1.25, "both", "every batch again", parts) == every  # (the table of every batch is rebuilt after a listed call)
    h.remove(ids[1])
    assert _assert_pieces(h, None, 1.25, "both", "after a removal") == every[:1] + every[2:]
    with pytest.raises(egg.EggError, match="egg_pieces: no batch with id `%d`" % ids[1]):
        h.pieces([ids[0], ids[1]])


def test_masks(egg):
    h, ids = _four_eggs(egg, "exact")
    h.update(H60, H60, S, CS)
    parts = _particles(h)
    both = _assert_pieces(h, None, 1.0, "both", "both", parts)
    white = _assert_pieces(h, None, 1.0, "white", "white", parts)
    yolk = _assert_pieces(h, None, 1.0, "yolk", "yolk", parts)
    assert white == [(p[0], pm.ZERO) for p in both] and yolk == [(pm.ZERO, p[1]) for p in both]
    assert h.pieces(None, 1.0, 1) == h.pieces(None, 1.0, "white") and h.pieces(None, 1.0, 2)[0][WHITE] is None
    for types, other in (("white", YOLK), ("yolk", WHITE)):
        labels = _assert_labels(h, 1.0, types, types, parts)
        assert (labels[other] == -1).all() and (labels[1 - other] >= 0).all()


def test_calls_around_a_step_in_flight(egg):
    h, ids = _four_eggs(egg, "exact")
    held = h.pieces()
    state = [h.download(w, f) for w in (WHITE, YOLK) for f in FIELDS]
    h.step_begin(H60, S, CS)
    with pytest.raises(egg.EggError, match=r"egg_pieces: a step is in flight \(egg_step_begin without egg_step_end\)"):
        h.pieces()
    with pytest.raises(egg.EggError, match="egg_pieces: a step is in flight"):
        h.piece_labels()
    with pytest.raises(egg.EggError, match="egg_pieces: a step is in flight"):
        h.is_whole(ids[0])
    h.step_end(False)
    assert all(np.array_equal(a, b) for a, b in zip(state, [h.download(w, f) for w in (WHITE, YOLK) for f in FIELDS]))
    assert h.pieces() == held
    h.step_begin(H60, S, CS)
    h.step_end(True)
    _assert_pieces(h, None, 1.0, "both", "after the committed step")


def test_every_refusal_leaves_the_buffers_as_the_caller_filled_them(egg):
    from egg_fluid_simulation_amd import _ffi
    h, ids = _four_eggs(egg, "exact")
    n_white, n_yolk = h.get_n_particles()
    nan = float("nan")

    def spec_of(rw=1.0, ry=1.0, mask=3):
        return _ffi.EggPiecesSpec((C.c_double * 2)(rw, ry), mask, 0)

    def call(spec, n, listed, with_out=True, rc=_ffi.EGG_ERR_INVALID_ARGUMENT, text=""):
        out = (_ffi.EggPieceSummary * 16)()
        C.memset(out, 0x5A, C.sizeof(out))
        untouched = bytes(out)
        lw, ly = np.full(n_white, 77, dtype=np.int32), np.full(n_yolk, 77, dtype=np.int32)
        arr = None if listed is None else np.ascontiguousarray(listed, dtype=np.int64)
        before = h.stats()
        got = h._lib.egg_pieces(h._h, None if spec is None else C.byref(spec), n, None if arr is None else arr.ctypes.data,
                                out if with_out else None, lw.ctypes.data, ly.ctypes.data)
        assert got == rc, (text, got)
        assert text in h._message(), (text, h._message())
        assert bytes(out) == untouched and (lw == 77).all() and (ly == 77).all() and h.stats() == before, text

    call(None, 0, None, text="egg_pieces: spec is NULL")
    call(spec_of(), 0, None, with_out=False, text="egg_pieces: out is NULL")
    call(spec_of(), -1, None, text="egg_pieces: n_ids = -1 without a list")
    call(spec_of(), 2, None, text="egg_pieces: n_ids = 2 without a list")
    call(spec_of(), 2, [ids[0], 99], rc=_ffi.EGG_ERR_UNKNOWN_ID, text="egg_pieces: no batch with id `99`")
    call(spec_of(), 1, [0], rc=_ffi.EGG_ERR_UNKNOWN_ID, text="egg_pieces: no batch with id `0`")
    for rw, ry, text in ((0.0, 1.0, "reach[0] = 0"), (1.0, -1.0, "reach[1] = -1"), (nan, 1.0, "reach[0] = nan"), (1.0, INF, "reach[1] = inf"),
                         (-INF, 1.0, "reach[0] = -inf")):
        call(spec_of(rw, ry), 0, None, text="egg_pieces: " + text)
    for mask in (0, 4, -1):
        call(spec_of(mask=mask), 1, [ids[0]], text="egg_pieces: type_mask %d" % mask)
    # the wrappers' own checks
    for kw, text in ((dict(reach=0.0), "reach must be finite and above 0"), (dict(reach=(1.0, nan)), "reach must be finite and above 0"),
                     (dict(reach=(1.0, 2.0, 3.0)), "reach must be None, a number or"), (dict(reach="far"), "reach must be None, a number or"),
                     (dict(types="none"), "pieces: types must be"), (dict(types=0), "pieces: types must be"), (dict(ids=[1.5, "a"]), "ids must be None or a list")):
        with pytest.raises(egg.EggError, match=text):
            h.pieces(**kw)
    # a handle without batches: nothing to report, nothing launched
    empty = egg.SimulationHandler()
    assert empty.pieces() == [] and [a.size for a in empty.piece_labels()] == [0, 0] and empty.stats()["kernel_launches"] == 0
    with pytest.raises(egg.EggError, match="no batch with id `1`"):
        empty.pieces([1])


def test_a_call_only_observes(egg):
    """the same relaxed scene with and without pieces calls: equal particles, equal launches per step; a call changes no
    download and no counter but kernel_launches, which rises by at most 2"""
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
        state = [a.download(w, f) for w in (WHITE, YOLK) for f in FIELDS]
        stats = a.stats()
        first = a.pieces()
        after = a.stats()
        assert 1 <= after["kernel_launches"] - stats["kernel_launches"] <= 2
        assert {key: v for key, v in after.items() if key != "kernel_launches"} == {key: v for key, v in stats.items() if key != "kernel_launches"}
        for _ in range(20):
            assert a.pieces() == first
        labels = a.piece_labels()
        assert all(np.array_equal(p, q) for p, q in zip(labels, a.piece_labels()))
        assert all(np.array_equal(p, q) for p, q in zip(state, [a.download(w, f) for w in (WHITE, YOLK) for f in FIELDS]))
        for w in (WHITE, YOLK):
            for f in FIELDS:
                assert np.array_equal(a.download(w, f), b.download(w, f)), (k, w, f)
    assert launches[id(a)] == launches[id(b)], launches
    assert a.collider_hits() == b.collider_hits() and a.elapsed == b.elapsed


# ------------------------------------------------------------------------------------------------ device groups
CUTS = {2: [-INF, 335.0, INF], 3: [-INF, 320.0, 372.0, INF]}


def _plain(res):
    return [tuple(None if t is None else tuple(t) for t in pair) for pair in res]


@pytest.mark.parametrize("n_handles,eggs", [(2, EGGS[1::-1] + EGGS[2:]), (3, EGGS)])
def test_device_group_equals_one_handle(egg, n_handles, eggs):
    g = _relaxed_scene(egg.SimulationGroup([0] * n_handles, cuts=CUTS[n_handles]))
    h = _relaxed_scene(egg.SimulationHandler())
    ids = [g.add(x, y) for x, y in eggs]
    assert [h.add(x, y) for x, y in eggs] == ids
    assert len({g.owner(i)[0] for i in ids}) == n_handles
    assert not hasattr(g, "piece_labels")
    for k in range(3):
        for reach in (None, 1.0):
            want = _assert_pieces(h, None, reach, "both", "one handle, step %d" % k)
            assert _plain(g.pieces(None, reach)) == _plain(h.pieces(None, reach)) == [tuple(pm.summary(r) for r in pair) for pair in want], k
            listed = [ids[3], ids[0], ids[3], ids[1]]
            assert _plain(g.pieces(listed, reach, "white")) == _plain(h.pieces(listed, reach, "white"))
            assert [g.is_whole(i, reach) for i in ids] == [h.is_whole(i, reach) for i in ids]
        g.step(H60, S, CS)
        h.step(H60, S, CS)
    with pytest.raises(egg.EggError, match="egg_group_pieces: no batch with id `77`"):
        g.pieces([ids[0], 77])
    assert g.pieces([]) == []


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
        for _ in range(3):
            steps.append(dict(default=_plain(sh.pieces()), tight=_plain(sh.pieces(None, 1.0)),
                              listed=_plain(sh.pieces([ids[3], ids[0], ids[3], ids[1]], 1.0, "white")),
                              whole=[sh.is_whole(i, 1.0) for i in ids], owned=len(sh.local.list_ids())))
            sh.step(H60, S, CS)
        q.put((rank, "ok", dict(steps=steps, empty=sh.pieces([]), labels=hasattr(sh, "piece_labels"))))
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
    """two ranks on one GPU (three processes with the GPU open), the cut between the two overlapping eggs: the summed tables
    are one handle's records on both ranks"""
    res = _spawn(2)
    h = _relaxed_scene(egg.SimulationHandler())
    ids = [h.add(x, y, 50, 15) for x, y in EGGS[1::-1] + EGGS[2:]]
    for k in range(3):
        _assert_pieces(h, None, 1.0, "both", "one handle, step %d" % k)
        for r in (0, 1):
            got = res[r]["steps"][k]
            assert got["default"] == _plain(h.pieces()) and got["tight"] == _plain(h.pieces(None, 1.0)), (r, k)
            assert got["listed"] == _plain(h.pieces([ids[3], ids[0], ids[3], ids[1]], 1.0, "white")), (r, k)
            assert got["whole"] == [h.is_whole(i, 1.0) for i in ids], (r, k)
        assert 0 < res[0]["steps"][k]["owned"] < 4 and res[0]["steps"][k]["owned"] + res[1]["steps"][k]["owned"] == 4
        h.step(H60, S, CS)
    assert res[0]["empty"] == [] and res[1]["empty"] == [] and not res[0]["labels"]
