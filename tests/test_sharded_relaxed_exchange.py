"""HaloExchange (egg_fluid_simulation_amd/sharding.py) on the CPU: 2 and 4 gloo ranks, no GPU.  The exchange is driven
with injected boxes and injected record arrays -- a numpy stand-in for the handler's rx_get_boxes / rx_pack / rx_fetch
that knows only its OWN particles and the boxes that came over the wire -- and every rank must end up with exactly the
ghost records tests/group_relaxed_model.ghosts_of predicts for it from the global picture: the same set of keys, the
payloads bit for bit, and the right counters."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest

from conftest import ROOT

import group_relaxed_model as grm

PASSES = ("dense", "empty", "reach", "separated")


def _scene(world, kind, which, seed):
    """one type's particles of one pass, the global picture: owner, cx, cy, payload [n, 4] (x, y, inverse mass, radius), key.
    Rank k's particles sit in the cells [20 k, 20 k + 19] in x, give or take what the pass is about."""
    rng = np.random.default_rng(1000 * seed + 10 * which + world)
    owner, cx, cy = [], [], []
    for k in range(world):
        m = 40 + 7 * k + 5 * which
        lo, hi = 20 * k - 2, 20 * k + 21          # dense: neighbours overlap by a few cells
        if kind == "separated":
            lo, hi = 20 * k + 3, 20 * k + 16      # six cells between neighbours: nobody has a ghost
        if kind == "empty":
            # a rank with an empty box: the last rank has no white particle, rank 0 has no yolk particle, and with four
            # ranks rank 1 owns nothing at all
            if (which == 0 and k == world - 1) or (which == 1 and k == 0) or (world == 4 and k == 1):
                m = 0
        x = rng.integers(lo, hi + 1, m)
        y = rng.integers(0, 12, m)
        if kind == "reach" and k == 0 and m:
            x[0], y[0] = 20 * (world - 1) + 5, 6  # rank 0's box reaches past its direct neighbour, over every slab
        owner += [k] * m
        cx += x.tolist()
        cy += y.tolist()
    owner, cx, cy = np.array(owner), np.array(cx, dtype=np.int64), np.array(cy, dtype=np.int64)
    n = len(owner)
    perm = rng.permutation(n)  # keys interleave the ranks, as batch ids do
    payload = np.stack([cx * 8.0 + rng.random(n) * 8.0, cy * 8.0 + rng.random(n) * 8.0, 1.0 / (1.0 + rng.random(n)),
                        4.0 + rng.random(n)], axis=1)
    return owner, cx, cy, payload, perm.astype(np.int64)


class _Source:
    """what HaloExchange needs of a handler, over this rank's particles alone"""

    def __init__(self, rank, world):
        self.rank = rank
        self.mine = []  # [pass][which] -> (cx, cy, words [m, 5] int64)
        for p, kind in enumerate(PASSES):
            per = []
            for which in (0, 1):
                owner, cx, cy, payload, key = _scene(world, kind, which, p)
                loc = owner == rank
                words = np.concatenate([payload[loc].view(np.int64), key[loc][:, None]], axis=1)
                per.append((cx[loc], cy[loc], words))
            self.mine.append(per)
        self.messages = None

    def rx_get_boxes(self, p):
        out = np.zeros((2, 5), dtype=np.int32)
        for which in (0, 1):
            cx, cy, _ = self.mine[p][which]
            out[which] = (cx.min(), cy.min(), cx.max(), cy.max(), 0) if len(cx) else (0, 0, 0, 0, 1)
        return out

    def rx_pack(self, p, boxes):
        boxes = np.asarray(boxes).reshape(-1, 2, 5)
        counts = np.zeros((len(boxes), 2), dtype=np.int64)
        self.messages = []
        for k, both in enumerate(boxes):
            per = []
            for which, b in enumerate(both):
                cx, cy, words = self.mine[p][which]
                take = np.zeros(len(cx), dtype=bool)
                if not b[4]:
                    take = (cx >= b[0] - 1) & (cx <= b[2] + 1) & (cy >= b[1] - 1) & (cy <= b[3] + 1)
                sel = words[take][::-1]  # (any order will do)
                counts[k, which] = len(sel)
                per.append(np.concatenate([[len(sel)], sel.reshape(-1)]).astype(np.int64))
            self.messages.append(per)
        return counts

    def rx_fetch(self, pointers):
        for k, row in enumerate(np.asarray(pointers).reshape(-1, 2)):
            for which, ptr in enumerate(row):
                if int(ptr):
                    m = np.ascontiguousarray(self.messages[k][which])
                    ctypes.memmove(int(ptr), m.ctypes.data, m.nbytes)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from egg_fluid_simulation_amd.sharding import HaloExchange
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ex = HaloExchange(_Source(rank, world), rank, world, group=dist, device="cpu")
        got = []
        for p in range(len(PASSES)):
            pointers, counts = ex.exchange(p)
            per = []
            for which in (0, 1):
                rec = ex.received(which)
                # what rx_run_pass would be handed: the same messages, by address
                words = []
                for ptr, c in zip(pointers[:, which], counts[:, which]):
                    if c:
                        raw = np.frombuffer(ctypes.string_at(int(ptr), 8 * (1 + 5 * int(c))), dtype=np.int64)
                        assert raw[0] == c
                        words.append(raw[1:].reshape(-1, 5))
                by_ptr = np.concatenate(words) if words else np.zeros((0, 5), dtype=np.int64)
                assert np.array_equal(by_ptr, rec)
                per.append(rec.tolist())
            got.append((per, list(ex.partners), dict(passes=ex.passes, records=ex.records, bytes=ex.bytes,
                                                     collectives=ex.collectives)))
        q.put((rank, "ok", got))
    except Exception:  # surface the traceback in the parent instead of a queue timeout
        import traceback
        q.put((rank, "error: " + traceback.format_exc(), None))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_every_rank_receives_exactly_its_ghosts(world):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
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
    for rank in range(world):
        records = 0
        for p, kind in enumerate(PASSES):
            per, partners, counters = res[rank][p]
            expect_partners = set()
            for which in (0, 1):
                owner, cx, cy, payload, key = _scene(world, kind, which, p)
                gh = grm.ghosts_of(owner, cx, cy, rank)
                want = np.concatenate([payload[gh].view(np.int64), key[gh][:, None]], axis=1)
                have = np.array(per[which], dtype=np.int64).reshape(-1, 5)
                assert sorted(have[:, 4].tolist()) == sorted(key[gh].tolist()), (rank, kind, which)
                assert len(set(have[:, 4].tolist())) == len(have)  # nothing twice
                assert np.array_equal(have[np.argsort(have[:, 4])], want[np.argsort(want[:, 4])]), (rank, kind, which)
                records += int(gh.sum())
                expect_partners |= set(owner[gh].tolist())
                if kind == "empty" and not (owner == rank).any():
                    assert len(have) == 0  # an empty box draws nothing
            # a partner is a rank within reach; whoever sends a ghost is one, and nobody is when nobody has a ghost
            assert expect_partners <= set(partners), (rank, kind)
            if kind == "separated":
                assert partners == [] and all(len(v) == 0 for v in per)
            if kind == "reach" and world == 4:
                assert (set(partners) == {1, 2, 3}) if rank == 0 else (0 in partners)
            assert counters["passes"] == p + 1 and counters["collectives"] == p + 1
            assert counters["records"] == records and counters["bytes"] == 40 * records
        assert records > 0
