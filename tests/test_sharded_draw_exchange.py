"""The gather behind ShardedSimulationHandler.draw() (egg_fluid_simulation_amd/sharding.py) on the CPU: 2 and 4 gloo ranks,
no GPU.  The local handlers are numpy stand-ins that know only their OWN batches and answer draw_pack / draw_source_* by
address, as the library does.  Batches interleave over the ranks so that no rank holds a contiguous range of global keys,
one rank owns nothing, a batch is removed from the middle of the id range, and a hand-over leaves a rank's local ids in
another order than the global ids.  What the render rank assembles must equal, element for element, the arrays of ONE
stand-in holding everything, and the message and byte counts must equal the wire model's: per collective and non-render
rank ONE message of 7 x 8 B per particle it holds + one 8 B status word."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest

from conftest import ROOT

DRAW_ROWS = [0, 1, 4, 5, 2, 3, 7]  # x, y, last_x, last_y, vx, vy, radius in the 9-row state of export_batch
N_BATCHES = 12
REMOVED, MOVED, OVERRIDE = 5, 9, {3: (11, 4), 10: (2, 7)}


def _counts(gid):
    return OVERRIDE.get(gid, (6 + gid % 5, 3 + gid % 3))


def _state(gid, which):
    n = _counts(gid)[which]
    return gid * 1000.0 + which * 500.0 + 50.0 * np.arange(9)[:, None] + np.arange(n)[None, :] + 0.25


class _Fake:
    """what ShardedSimulationHandler needs of a local handler, over this rank's batches alone"""

    def __init__(self):
        self.batches = {}   # local id -> (key, [white state, yolk state])
        self.next_lid = 1
        self.shadow = {}

    def _new(self, key, states):
        lid = self.next_lid
        self.next_lid += 1
        self.batches[lid] = (int(key), states)
        return lid

    def add_many_keyed(self, xs, ys, keys, white_radius=None, yolk_radius=None, white_n_particles=None, yolk_n_particles=None):
        gid = int(keys[0])
        want = (white_n_particles, yolk_n_particles)
        for which in (0, 1):  # the overrides reach the owner
            assert want[which] == (OVERRIDE[gid][which] if gid in OVERRIDE else None)
        return [self._new(gid, [_state(gid, 0), _state(gid, 1)])]

    def get_n_particles(self, lid=None):
        if lid is None:
            return tuple(sum(s[w].shape[1] for _k, s in self.batches.values()) for w in (0, 1))
        return tuple(self.batches[lid][1][w].shape[1] for w in (0, 1))

    def remove(self, lid):
        del self.batches[lid]

    def export_batch(self, lid):
        key, (ws, ys) = self.batches[lid]
        info = dict(key=key, target_x=1.0 * key, target_y=2.0 * key, white_radius=50.0, yolk_radius=15.0, n_white=ws.shape[1],
                    n_yolk=ys.shape[1])
        return info, ws, ys

    def import_batch(self, info, ws, ys):
        return self._new(info["key"], [np.array(ws), np.array(ys)])

    def _mine(self, which):  # particles lie in ascending KEY, whatever the local ids are
        parts = [s[which][DRAW_ROWS] for _k, s in sorted(self.batches.values(), key=lambda b: b[0])]
        return np.concatenate(parts, axis=1) if parts else np.zeros((7, 0))

    def draw_pack(self, which, pointer, cap):
        m = np.ascontiguousarray(self._mine(which))
        assert m.shape[1] <= cap
        if m.size:
            ctypes.memmove(int(pointer), m.ctypes.data, m.nbytes)

    def draw_source_layout(self, which, total, atom_offset, atom_color):
        off = np.asarray(atom_offset)
        assert len(off) == len(atom_color) and (len(off) == 0 or off[0] == 0) and np.all(np.diff(off) > 0)
        self.shadow[which] = np.full((7, int(total)), np.nan)
        self.layout = (int(total), off.tolist())

    def draw_source_place(self, which, pointer, n, run_src, run_dst):
        if n == 0:  # (the render rank owns nothing of the type: only the in-flight check is made)
            assert not pointer and len(run_src) == 0
            return
        if pointer:
            msg = np.frombuffer(ctypes.string_at(int(pointer), 56 * int(n)), dtype=np.float64).reshape(7, int(n))
        else:
            msg = self._mine(which)
            assert msg.shape[1] == n
        sh = self.shadow[which]
        ends = list(run_src[1:]) + [int(n)]
        assert len(run_src) >= 1 and run_src[0] == 0
        for a, b, d in zip(run_src, ends, run_dst):
            assert b > a and d >= 0 and d + (b - a) <= sh.shape[1]
            assert np.all(np.isnan(sh[:, d:d + b - a]))  # every destination has exactly one source
            sh[:, d:d + b - a] = msg[:, a:b]

    def draw_source_download(self, which, field, n):
        from egg_fluid_simulation_amd import _ffi
        sh = self.shadow[which]
        assert sh.shape[1] == n and not np.isnan(sh).any()
        return sh[_ffi.DRAW_FIELDS.index(field)].copy()


def _owner_rank(world, gid, phase):
    """rank that holds batch `gid` at its add: interleaved with one rank left empty (rank 2 of four; with two ranks the
    second phase puts everything on rank 1, so the render rank itself owns nothing)"""
    if phase == 1:
        return world - 1
    return [0, 1, 3][gid % 3] if world == 4 else gid % 2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, root, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler, SlabLayout
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        out = []
        for phase in (0, 1):
            sh = ShardedSimulationHandler(SlabLayout([100.0 * k for k in range(world + 1)]), rank, dist, _Fake, device="cpu", root=root)
            snaps = []

            def snap(tag):
                data = [sh.download_instance_data(w) for w in (0, 1)]
                ids = sh.download(0, "batch_id")
                snaps.append(dict(tag=tag, data=[None if d is None else d.tolist() for d in data],
                                  ids=None if ids is None else ids.tolist(), counters=sh.draw_counters(), owner=dict(sh.owner),
                                  lids=dict(sh.local_id), n=sh.get_n_particles(), listed=sh.list_ids()))

            def add(gid):
                x = 100.0 * _owner_rank(world, gid, phase) + 50.0
                got = sh.add(x, 10.0, 50, 15, None, None, *OVERRIDE.get(gid, (None, None)))
                assert got == gid

            for gid in range(1, N_BATCHES + 1):
                add(gid)
            snap("added")
            sh.remove(REMOVED)
            snap("removed")
            if phase == 0:  # MOVED goes to the rank that holds batches on both sides of it in id order
                src, dest = sh.owner[MOVED], sh.owner[MOVED - 1]
                assert src != dest
                if rank == src:
                    sh._send_batches([MOVED], dest)
                elif rank == dest:
                    sh._recv_batches(1, src)
                sh.owner[MOVED] = dest
                sh._keys_stale = True
                snap("moved")
            add(N_BATCHES + 1)
            snap("added again")
            out.append(snaps)
        q.put((rank, "ok", out))
    except Exception:  # surface the traceback in the parent instead of a queue timeout
        import traceback
        q.put((rank, "error: " + traceback.format_exc(), None))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,root", [(2, 0), (4, 0), (2, 1), (4, 2)])  # (rank 2 of four owns nothing in the first phase)
def test_the_render_rank_assembles_one_handlers_arrays(world, root):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, root, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in procs:
        rank, outcome, got = q.get(timeout=180)
        assert outcome == "ok", outcome
        res[rank] = got
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for phase in (0, 1):
        n_snaps = len(res[root][phase])
        assert n_snaps == (4 if phase == 0 else 3)
        sent = {r: [0, 0] for r in range(world)}  # the model's (messages, bytes) per rank so far
        for k in range(n_snaps):
            at_root = res[root][phase][k]
            live = at_root["listed"]
            assert all(res[r][phase][k]["listed"] == live and res[r][phase][k]["owner"] == at_root["owner"] for r in range(world))
            one = _Fake()  # ONE stand-in holding every live batch
            for gid in live:
                one._new(gid, [_state(gid, 0), _state(gid, 1)])
            for which in (0, 1):
                want = one._mine(which).T
                assert np.array_equal(np.array(at_root["data"][which]), want), (phase, at_root["tag"], which)
                others = [r for r in range(world) if r != root]
                for r in others:
                    assert res[r][phase][k]["data"][which] is None  # answered on the render rank only
                # one collective of this type: every other rank sends what it holds + the status word
                for r in others:
                    held = sum(_counts(g)[which] for g in live if at_root["owner"][g] == r)
                    for rr in (r, root):
                        sent[rr][0] += 1
                        sent[rr][1] += 56 * held + 8
            assert at_root["ids"] == [g for g in live for _ in range(_counts(g)[0])]
            for r in range(world):
                snap = res[r][phase][k]
                assert snap["n"] == (sum(_counts(g)[0] for g in live), sum(_counts(g)[1] for g in live))
                assert snap["counters"]["messages"] == sent[r][0] and snap["counters"]["bytes"] == sent[r][1], (phase, k, r)
                assert snap["counters"]["draws"] == 2 * (k + 1)
            # the scene is what the docstring promises
            owners = [at_root["owner"][g] for g in live]
            if phase == 0:
                for r in set(owners):  # no rank holds a contiguous range of the global order
                    idx = [i for i, o in enumerate(owners) if o == r]
                    assert idx[-1] - idx[0] + 1 > len(idx)
                assert set(owners) == ({0, 1, 3} if world == 4 else {0, 1})
            else:
                assert set(owners) == {world - 1}
            if at_root["tag"] == "moved":
                dest = at_root["owner"][MOVED]
                lids = res[dest][phase][k]["lids"]
                by_gid = [lids[g] for g in sorted(lids)]
                assert by_gid != sorted(by_gid)  # local ids no longer ascend with the global ids
        assert REMOVED not in res[root][phase][-1]["listed"] and N_BATCHES + 1 in res[root][phase][-1]["listed"]
