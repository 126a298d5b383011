"""The reads of ShardedSimulationHandler that add integers over the ranks, on real collectives: two gloo ranks on the CPU
with stand-in local handlers that answer rank-dependent integers, and a `dist` that records every collective it carries.
Each reduced read returns the sum on both ranks after exactly one all_reduce(SUM) of an int64 tensor (field: one per
present plane and one for the totals), probe gathers instead, an unknown id is refused before anything travels, and a
one-rank object built without a process group answers every read from its own handle.  No device."""
import os
import sys
import types

import numpy as np
import pytest

from conftest import ROOT

N_BATCHES = 5         # global ids 1 .. 5; id g lives on rank g % world
N_SENSORS = 2
N_COLLIDERS = 3
GRID = (4, 3)         # nx, ny
MEASURE_WORDS = 24
READS = ["collider_hits", "collider_grips", "collider_load_sums", "sensor_sums", "sensor_batches", "field", "field_velocity", "pieces",
         "impulse", "measure_table", "viscosity_pairs", "containment_hits"]


def _row(lid, words):
    """what the stand-in answers for the batch with local id `lid`: the same on whichever rank holds it"""
    return (1000 * lid + np.arange(words, dtype=np.int64))


class _Local:
    """the least a local handler must offer to the reduced reads; every integer depends on the rank or on the batch"""

    def __init__(self, rank):
        self.rank = rank

    def add_many_keyed(self, xs, ys, keys, white_radius=None, yolk_radius=None, **counts):
        return [100 + int(keys[0])]  # the local id of a batch

    def collider_hits(self):
        return [10 + self.rank, 20 + 2 * self.rank]

    def collider_grips(self):
        return [30 + self.rank, 40 + 3 * self.rank]

    def viscosity_pairs(self):
        return [50 + self.rank, 60 + 5 * self.rank]

    def containment_hits(self):
        return 70 + 7 * self.rank

    def collider_load_sums(self):
        return [(k + self.rank, -k - 2 * self.rank, (1 << 40) + k) for k in range(N_COLLIDERS)], 3 + self.rank, 0.25

    def get_sensors(self):
        return [("disc", 0.0, 0.0, 1.0, "both")] * N_SENSORS

    def sensor_sums(self):
        return [((k + self.rank, 2 * k - self.rank, 1 << 41), (k, self.rank, -3)) for k in range(N_SENSORS)], [self.rank, 2 + self.rank]

    def sensor_batches(self, lids):
        return np.stack([_row(lid, 2 * N_SENSORS).reshape(N_SENSORS, 2) for lid in lids]).astype(np.int32)

    def _probe_table(self, n, arr):
        # per probe (white, yolk): (score, key, index, id, x, y, radius); rank 1 scores lower on white, rank 0 on yolk
        return [((2.0 - self.rank, 7 + self.rank, k, 7 + self.rank, 1.5, 2.5, 3.5), (1.0 + self.rank, 9 + self.rank, k, 9 + self.rank, 4.5, 5.5, 6.5))
                for k in range(n)]

    def _field_planes(self, spec, velocity):
        shape = (2, spec.ny, spec.nx)
        count = (np.arange(2 * spec.ny * spec.nx, dtype=np.int32).reshape(shape) + self.rank)
        svx = count.astype(np.int64) * (1 << 33) if velocity else None
        svy = -count.astype(np.int64) - self.rank if velocity else None
        totals = types.SimpleNamespace(inside=[5 + self.rank, 6], outside=[7, 8 + self.rank], dropped=[self.rank, 0], units_tiled=2 + self.rank, units_direct=1)
        return count, svx, svy, totals

    def _piece_table(self, spec, lids):
        return np.stack([_row(lid, 16).reshape(2, 8) for lid in lids])

    def _impulse_table(self, n, arr, results=True):
        return (np.arange(8 * n, dtype=np.int64).reshape(n, 8) * (1 + self.rank)) if results else None

    def _measure_check(self, spec):
        pass

    def _measure_table(self, spec, lids):
        return np.stack([_row(lid, 2 * MEASURE_WORDS).reshape(2, MEASURE_WORDS) for lid in lids])


class _Recorder:
    """torch.distributed with every collective written down: (name, dtype, shape, op)"""

    def __init__(self, dist):
        self._dist, self.calls, self.ReduceOp = dist, [], dist.ReduceOp

    def all_reduce(self, tensor, op=None):
        self.calls.append(("all_reduce", str(tensor.dtype), tuple(tensor.shape), "SUM" if op == self._dist.ReduceOp.SUM else str(op)))
        return self._dist.all_reduce(tensor, op=op)

    def all_gather(self, parts, tensor):
        self.calls.append(("all_gather", str(tensor.dtype), tuple(tensor.shape), None))
        return self._dist.all_gather(parts, tensor)

    def __getattr__(self, name):  # (anything else a read reached for would show up here)
        self.calls.append((name, None, None, None))
        return getattr(self._dist, name)


class _Untouched:
    """the `dist` of a one-rank object: nothing may reach for it"""

    def __getattr__(self, name):
        raise AssertionError("a one-rank object touched dist.%s" % name)


def _plain(v):
    """a read's answer as plain Python: arrays as (dtype, nested lists), namedtuples as tuples"""
    if isinstance(v, np.ndarray):
        return (str(v.dtype), v.tolist())
    if isinstance(v, (tuple, list)):
        return [_plain(x) for x in v]
    return v


def _read(sh, name):
    ids = [3, 1, 3, 4]  # (out of order, one twice, of both ranks)
    if name == "sensor_batches":
        return sh.sensor_batches(ids)
    if name == "field":
        return sh.field((0.0, 0.0), 1.0, GRID)
    if name == "field_velocity":
        return sh.field((0.0, 0.0), 1.0, GRID, velocity=True)
    if name == "pieces":
        return sh.pieces(ids, reach=1.5)
    if name == "impulse":
        return sh.impulse([("kick", ("disc", 0.0, 0.0, 5.0), 1.0, 2.0), ("brake", ("disc", 0.0, 0.0, 5.0), 0.0, 0.0, 1.0, {"id": 2})])
    if name == "measure_table":
        return sh.measure_table(ids)
    return getattr(sh, name)()


def _build(rank, world, dist):
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler, SlabLayout
    sh = ShardedSimulationHandler(SlabLayout([100.0 * k for k in range(world + 1)]), rank, dist, lambda: _Local(rank), device="cpu")
    for gid in range(1, N_BATCHES + 1):
        assert sh.add(100.0 * (gid % world) + 50.0, 10.0) == gid
    return sh


def _refusals(sh, calls):
    """an unknown id is refused with the present text, before any collective"""
    from egg_fluid_simulation_amd import EggError
    out = []
    for call, text in ((lambda: sh.sensor_batches([1, 77]), "[ERROR] In SimulationHandler.sensor_batches: no batch with id `77`"),
                       (lambda: sh.pieces([77, 1]), "[ERROR] In SimulationHandler.pieces: no batch with id `77`"),
                       (lambda: sh.measure_table([1, 77]), "[ERROR] In SimulationHandler.measure: no batch with id `77`")):
        before = len(calls)
        with pytest.raises(EggError) as e:
            call()
        out.append((str(e.value) == text, len(calls) - before))
    return out


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        rec = _Recorder(dist)
        sh = _build(rank, world, rec)
        got = {}
        for name in READS + ["probe"]:
            before = len(rec.calls)
            answer = sh.probe([("point", 1.0, 2.0), ("ray", 0.0, 0.0, 1.0, 1.0)]) if name == "probe" else _read(sh, name)
            got[name] = (_plain(answer), rec.calls[before:])
        got["refusals"] = _refusals(sh, rec.calls)
        q.put((rank, "ok", got))
    except Exception:  # surface the traceback in the parent instead of a queue timeout
        import traceback
        q.put((rank, "error: " + traceback.format_exc(), None))
    finally:
        dist.destroy_process_group()


def _one_handle(world):
    """what ONE handle holding everything answers: the stand-ins' integers added over the ranks, by the reads' own code on a
    one-rank object whose local handler adds the stand-ins of every rank"""
    ranks = [_Local(r) for r in range(world)]

    class Sum(_Local):
        def __init__(self):
            _Local.__init__(self, 0)

        def collider_hits(self):
            return np.sum([r.collider_hits() for r in ranks], axis=0).tolist()

        def collider_grips(self):
            return np.sum([r.collider_grips() for r in ranks], axis=0).tolist()

        def viscosity_pairs(self):
            return np.sum([r.viscosity_pairs() for r in ranks], axis=0).tolist()

        def containment_hits(self):
            return sum(r.containment_hits() for r in ranks)

        def collider_load_sums(self):
            parts = [r.collider_load_sums() for r in ranks]
            return [tuple(int(v) for v in np.sum([p[0][k] for p in parts], axis=0)) for k in range(N_COLLIDERS)], sum(p[1] for p in parts), 0.25

        def sensor_sums(self):
            parts = [r.sensor_sums() for r in ranks]
            sums = [tuple(tuple(int(v) for v in np.sum([p[0][k][w] for p in parts], axis=0)) for w in (0, 1)) for k in range(N_SENSORS)]
            return sums, np.sum([p[1] for p in parts], axis=0).tolist()

        def _field_planes(self, spec, velocity):
            parts = [r._field_planes(spec, velocity) for r in ranks]
            planes = [sum(p[k] for p in parts) if velocity or k == 0 else None for k in range(3)]
            t = [p[3] for p in parts]
            totals = types.SimpleNamespace(**{f: np.sum([getattr(x, f) for x in t], axis=0).tolist() for f in ("inside", "outside", "dropped")},
                                           units_tiled=sum(x.units_tiled for x in t), units_direct=sum(x.units_direct for x in t))
            return planes[0], planes[1], planes[2], totals

        def _impulse_table(self, n, arr, results=True):
            return sum(r._impulse_table(n, arr, results) for r in ranks) if results else None

    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler, SlabLayout
    sh = ShardedSimulationHandler(SlabLayout([0.0, 100.0 * world]), 0, _Untouched(), Sum)
    for gid in range(1, N_BATCHES + 1):
        assert sh.add(100.0 * (gid % world) + 50.0, 10.0) == gid
    return {name: _plain(_read(sh, name)) for name in READS}


def test_every_reduced_read_is_the_sum_after_one_int64_all_reduce():
    import torch.multiprocessing as mp
    from test_sharded_draw_exchange import _free_port
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in procs:
            rank, outcome, got = q.get(timeout=120)
            assert outcome == "ok", outcome
            res[rank] = got
    finally:
        for p in procs:
            p.join(30)
            if p.is_alive():
                p.kill()
                p.join(10)
    assert all(p.exitcode == 0 for p in procs)
    want = _one_handle(world)
    reduce_one = lambda shape: ("all_reduce", "torch.int64", shape, "SUM")
    planes = (2, GRID[1], GRID[0])
    shapes = {"collider_hits": [(2,)], "collider_grips": [(2,)], "viscosity_pairs": [(2,)], "containment_hits": [(1,)],
              "collider_load_sums": [(3 * N_COLLIDERS + 1,)], "sensor_sums": [(6 * N_SENSORS + 2,)], "sensor_batches": [(4, N_SENSORS, 2)],
              "field": [planes, (8,)], "field_velocity": [planes, planes, planes, (8,)], "pieces": [(4, 2, 8)], "impulse": [(2, 8)],
              "measure_table": [(4, 2, MEASURE_WORDS)]}
    for name in READS:
        for rank in range(world):
            answer, calls = res[rank][name]
            assert answer == want[name], (name, rank)
            assert calls == [reduce_one(shape) for shape in shapes[name]], (name, rank, calls)
    # the dtypes of the answers are the single handle's: int32 batches and counts, int64 sums and tables
    assert res[0]["sensor_batches"][0][0] == "int32" and res[0]["measure_table"][0][0] == "int64"
    assert [p[0] for p in res[0]["field_velocity"][0][:3]] == ["int32", "int64", "int64"] and res[0]["field"][0][1:3] == [None, None]
    for rank in range(world):
        answer, calls = res[rank]["probe"]
        assert calls == [("all_gather", "torch.int64", (2, 2, 7), None)], calls
        # per (probe, type) the lower score wins, whichever rank holds it: white from rank 1, yolk from rank 0
        assert answer == [[[8, k, 1.0, 1.5, 2.5, 3.5], [9, k, 1.0, 4.5, 5.5, 6.5]] for k in (0, 1)], answer
        assert res[rank]["refusals"] == [(True, 0)] * 3, res[rank]["refusals"]


def test_a_one_rank_object_without_a_process_group_answers_every_read_itself():
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler, SlabLayout
    for dist in (None, _Untouched()):
        sh = ShardedSimulationHandler(SlabLayout([0.0, 100.0]), 0, dist, lambda: _Local(0))
        for gid in range(1, N_BATCHES + 1):
            assert sh.add(50.0, 10.0) == gid
        own = sh.local
        lids = [103, 101, 103, 104]
        assert sh.collider_hits() == own.collider_hits() and sh.collider_grips() == own.collider_grips()
        assert sh.viscosity_pairs() == own.viscosity_pairs() and sh.containment_hits() == own.containment_hits()
        assert sh.collider_load_sums() == own.collider_load_sums() and sh.sensor_sums() == own.sensor_sums()
        got = _read(sh, "sensor_batches")
        assert got.dtype == np.int32 and np.array_equal(got, own.sensor_batches(lids))
        for velocity in (False, True):
            f = sh.field((0.0, 0.0), 1.0, GRID, velocity=velocity)
            count, svx, svy, t = own._field_planes(sh._c_field_spec((0.0, 0.0), 1.0, GRID, "both", "auto"), velocity)
            assert np.array_equal(f.count, count) and f.count.dtype == np.int32
            assert (f.svx is None and f.svy is None) if not velocity else (np.array_equal(f.svx, svx) and np.array_equal(f.svy, svy))
            assert (f.inside, f.outside, f.dropped, f.units_tiled, f.units_direct) == (tuple(t.inside), tuple(t.outside), tuple(t.dropped), 2, 1)
        assert _read(sh, "pieces") == sh._piece_summaries(own._piece_table(None, lids))
        assert _read(sh, "impulse") == sh._impulse_results(own._impulse_table(2, None))
        got = _read(sh, "measure_table")
        assert got.dtype == np.int64 and np.array_equal(got, own._measure_table(None, lids))
        hits = sh.probe([("point", 1.0, 2.0)])
        assert [tuple(h) for h in hits[0]] == [(7, 0, 2.0, 1.5, 2.5, 3.5), (9, 0, 1.0, 4.5, 5.5, 6.5)]
        from egg_fluid_simulation_amd import EggError
        with pytest.raises(EggError, match="In SimulationHandler.pieces: no batch with id `77`"):
            sh.pieces([77])


def test_the_two_helpers_hold_the_only_sum_over_the_ranks():
    """the text the per-method source assertions now follow to: the rank sum is one int64 all_reduce(SUM) that a one-rank object
    skips, and the owner-filled table ends in it"""
    import inspect
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    src = inspect.getsource(ShardedSimulationHandler._all_reduce_sum)
    assert src.count("self.dist.all_reduce(") == 1 and "ReduceOp.SUM" in src and "dtype=np.int64" in src
    assert src.index("self.world == 1") < src.index("self.dist.")
    src = inspect.getsource(ShardedSimulationHandler._owner_table)
    assert src.count("self._all_reduce_sum(") == 1 and "self.dist" not in src and src.index("raise EggError(") < src.index("self._all_reduce_sum(")
    for name in READS + ["sensors", "collider_loads", "pieces", "measure"]:  # no read reduces by hand
        if hasattr(ShardedSimulationHandler, name):
            assert "self.dist" not in inspect.getsource(getattr(ShardedSimulationHandler, name)), name
