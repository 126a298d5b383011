"""draw() and the rest of the SimulationHandler surface on ShardedSimulationHandler ("Several
processes"): every rank's particles travel to one render rank, are put into the order of ONE handle and drawn by the
single handle's kernels.  The rule under test: whatever the sharded object returns or draws equals, BIT FOR BIT, what ONE
SimulationHandler in the parent, driven by the same calls, returns or draws -- np.array_equal everywhere, no tolerance,
never one sharded run against another.  Ranks are spawned processes on GPU 0 over gloo, as in test_gpu_sharded_relaxed.py:
at most 4 ranks + the parent, each child joined with a time limit, the queue read with a time limit, no retries.  One
image is also held against oracle/render_model.py directly, so that the chain ends at the model."""
import math
import os
import socket
import sys
import warnings

import numpy as np
import pytest

from conftest import ROOT, circle_target, load_golden

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
SIZE, ORIGIN, ALPHA, CLEAR = (600, 560), (-190.0, -180.0), 0.35, (0.1, 0.2, 0.3, 1.0)
WIDE = dict(size=(1240, 760), origin=(380.0, 0.0))  # the column-swap scenes


# ------------------------------------------------------------------------------------------------ scenes
# A scene PLAYS the same calls on a ShardedSimulationHandler (every rank) and on one SimulationHandler (the parent) and
# calls probe(tag, ...) where the two are compared.

def _configs(kind):
    from egg_fluid_simulation_amd import default_configs
    white, yolk = default_configs()
    if kind == "styled":  # outline_thickness = 0 on one type: the outline branch is the only one that sets the draw colour
        white = dict(white, outline_thickness=2.5, highlight_strength=0.6, shadow_strength=0.7, texture_scale=10.0, motion_blur=0.002)
        yolk = dict(yolk, outline_thickness=0.0, highlight_strength=1.5, shadow_strength=0.4)
    return white, yolk


# Exact order over several ranks needs a collision budget that cannot bind (sharding.py, "Not covered"): every scene has
# at least ten batches, as the scenes of test_gpu_sharded.py have.
FILLERS = [(-300.0, -100.0), (-170.0, -100.0), (330.0, -100.0), (460.0, -100.0), (-300.0, 330.0), (460.0, 330.0)]
TEN = [(300.0, 300.0), (700.0, 300.0), (340.0, 320.0)] + [(150.0 + 130.0 * k, 520.0) for k in range(7)]


def _play_four_batches(sim, probe, order):
    centers = [tuple(float(v) for v in c) for c in load_golden("four_batches")["centers"]] + FILLERS
    if order != "exact":
        sim.set_solver_order(order, 1.8)
    ids = [sim.add(x, y, 50, 15) for x, y in centers]
    probe("before the first step")  # nothing is drawn
    for k in range(12):
        for i, c in zip(ids, centers):
            if c not in FILLERS:
                sim.set_target_position(i, *circle_target(c, k))
        sim.step(1 / 60, 2, 3)
        if k + 1 in (1, 6, 12):
            probe("step %d" % (k + 1))


def _play_swap(sim, probe, centers, target, steps, probes, orders, view):
    ids = [sim.add(x, y, 50, 15) for x, y in centers]
    for k in range(steps):
        if k in orders:
            sim.set_solver_order(orders[k], 1.8)
        for g in ids:
            sim.set_target_position(g, *target(g, k))
        if k % 2 == 1:
            assert sim.update(1 / 60, 1 / 60, 2, 3) == 1
        else:
            sim.step(1 / 60, 2, 3)
        if k + 1 in probes:
            probe("step %d" % (k + 1), **view)


def _play_swap2(sim, probe):  # test_gpu_sharded_relaxed's two columns that swap sides; exact -> relaxed -> exact
    from test_gpu_sharded_relaxed import _swap2_target
    centers = [(760.0, 150.0 + 300.0 * k) for k in range(5)] + [(1240.0, 150.0 + 300.0 * k) for k in range(5)]
    _play_swap(sim, probe, centers, _swap2_target(centers), 70, (10, 32, 48, 70), {22: "relaxed", 44: "exact"},
               dict(size=(700, 1400), origin=(650.0, 50.0)))


def _play_swap4(sim, probe):
    from test_gpu_sharded_relaxed import _swap4_target
    rows = [150.0, 450.0, 750.0]
    centers = ([(420.0, y) for y in rows] + [(900.0, y + 20.0) for y in rows] + [(1420.0, y - 10.0) for y in rows] +
               [(2100.0, y) for y in rows])
    _play_swap(sim, probe, centers, _swap4_target(centers), 60, (12, 36, 60), {}, dict(size=(2000, 900), origin=(300.0, 0.0)))


def _play_colours(sim, probe):
    """per-batch colours, the shared colour table, both switches, a live config change, remove + add, update()'s alpha"""
    sim._use_particle_color = True
    a = sim.add(300.0, 300.0, 50, 15, [0.9, 0.3, 0.3, 1.0], [0.2, 0.8, 0.4, 1.0])
    b = sim.add(700.0, 320.0, 50, 15)                                   # colourless: shares the config's tables
    c = sim.add(340.0, 330.0, 40, 12, None, [0.3, 0.3, 1.0, 1.0], 90, 20)   # count overrides
    d = sim.add(660.0, 280.0, 50, 15, [1.5, 0.5, -0.5, 1.0])            # out of range: add warns and does not clamp
    for k in range(6):
        sim.add(150.0 + 140.0 * k, 520.0, 50, 15)
    last = d + 6
    assert sim.get_n_particles(c) == (90, 20)
    for _ in range(3):
        sim.step(1 / 60, 2, 3)
    probe("particle colours")
    sim.set_white_color(b, 0.2, 0.9, 0.9)                               # retints the TYPE through the shared table
    sim.set_yolk_color(a, 1.0, 1.0, 0.0, 0.5)
    probe("retinted")
    sim._use_lighting = False
    sim._use_particle_color = False
    probe("no lighting, config colours")
    sim._use_lighting = True
    white = sim.get_white_config()
    sim.set_white_config(dict(white, min_radius=white["min_radius"] * 1.25, max_mass=white["max_mass"] * 1.5, color=[0.5, 0.6, 0.7, 1.0]))
    sim.set_white_color(b, 0.1, 0.2, 0.3)                               # the config's table is a new one: b keeps its own
    for i in (a, b, c, d):
        sim.set_target_position(i, 500.0, 300.0)
    for _ in range(3):
        sim.step(1 / 60, 2, 3)                                          # mass and radius re-derived
    probe("after a live set_white_config")
    sim.remove(b)                                                       # the middle of the id range
    e = sim.add(720.0, 300.0, 50, 15)
    assert e == last + 1 and sim.list_ids() == [a, c, d] + list(range(d + 1, last + 1)) + [e]
    assert sim.update(0.021, 1 / 60, 2, 3) == 1                         # leaves an interpolation_alpha of 0.26
    probe("after remove and add", alpha=None)                           # None takes the object's own
    assert sim.get_target_position(a) == (500.0, 300.0)


SCENES = {
    # name: (cuts per world, configs, play)
    "four_exact": ({1: [-2000.0, 2000.0], 2: [-2000.0, 10.0, 2000.0], 4: [-2000.0, 10.0, 400.0, 2000.0, 4000.0]}, "default",
                   lambda sim, probe: _play_four_batches(sim, probe, "exact")),
    "four_relaxed": ({2: [-2000.0, 10.0, 2000.0], 4: [-2000.0, -10.0, 20.0, 2000.0, 4000.0]}, "default",  # (rank 3 owns nothing)
                     lambda sim, probe: _play_four_batches(sim, probe, "relaxed")),
    "swap2": ({2: [0.0, 1000.0, 2000.0]}, "default", _play_swap2),
    "swap4": ({4: [0.0, 600.0, 1200.0, 1800.0, 2400.0]}, "default", _play_swap4),
    "colours": ({1: [0.0, 2000.0], 2: [0.0, 500.0, 2000.0], 4: [0.0, 500.0, 2000.0, 4000.0, 6000.0]}, "styled", _play_colours),
}


def _canvas(sim, which):
    from egg_fluid_simulation_amd import EggError
    try:
        return sim.render_canvas(which)
    except EggError as e:
        return str(e).split(":")[-1]  # (no canvas: nothing was drawn)


def _probe_of(sim, record):
    def probe(tag, size=SIZE, origin=ORIGIN, alpha=ALPHA, **kw):
        ids = sim.list_ids()
        local = getattr(sim, "local", None)  # (a sharded object: what this rank holds while it is probed)
        record.append(dict(
            n_local=None if local is None else local.get_n_particles(), tag=tag, image=sim.draw(size, origin, interpolation_alpha=alpha, clear=CLEAR, **kw),
            canvas=[_canvas(sim, w) for w in (WHITE, YOLK)], env=[sim.get_environment(w) for w in (WHITE, YOLK)],
            inst=[sim.download_instance_data(w) for w in (WHITE, YOLK)], ids=ids, pos=[sim.get_position(i) for i in ids],
            n=sim.get_n_particles(), n_each=[sim.get_n_particles(i) for i in ids], alpha=sim.interpolation_alpha,
            elapsed=sim.elapsed))
    return probe


# ------------------------------------------------------------------------------------------------ ranks

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _sharded(rank, cuts, configs, dist):
    from egg_fluid_simulation_amd import SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler, SlabLayout
    white, yolk = _configs(configs)
    return ShardedSimulationHandler(SlabLayout(cuts), rank, dist, lambda: SimulationHandler(white, yolk, device=0), device="cpu")


def _worker(rank, world, port, name, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from egg_fluid_simulation_amd import EggError
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        record = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if name == "in_flight":
                sh = _sharded(rank, [0.0, 500.0, 2000.0], "default", dist)
                for x, y in TEN:
                    sh.add(x, y, 50, 15)
                for _ in range(3):
                    sh.step(1 / 60, 2, 3)
                probe = _probe_of(sh, record)
                probe("before")
                if rank == 1:
                    sh.local.step_begin(1 / 60, 2, 3)  # a step open on ONE rank's handle: the draw is refused on the host
                try:
                    sh.draw(SIZE, ORIGIN, interpolation_alpha=ALPHA, clear=CLEAR)
                    record.append(dict(tag="refused", raised=None))
                except EggError as e:
                    record.append(dict(tag="refused", raised=str(e)))
                if rank == 1:
                    sh.local.step_end(False)
                probe("after")
            else:
                cuts, configs, play = SCENES[name]
                sh = _sharded(rank, cuts[world], configs, dist)
                play(sh, _probe_of(sh, record))
            extra = dict(owner=dict(sh.owner), migrations=sh.migrations, counters=sh.draw_counters(), halo=sh.halo_counters(),
                         n_local=sh.local.get_n_particles())
        q.put((rank, "ok", (record, extra)))
    except Exception:
        import traceback
        q.put((rank, "error: " + traceback.format_exc(), None))
    finally:
        dist.destroy_process_group()


def _spawn(name, world):
    import queue
    import time

    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, name, q)) for r in range(world)]
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


# ------------------------------------------------------------------------------------------------ comparison

def _same_probe(got, want, what, root):
    """one probe of one rank against the parent's single handle"""
    assert got["tag"] == want["tag"]
    # replicated answers: the same on every rank
    assert got["ids"] == want["ids"] and got["n"] == want["n"] and got["n_each"] == want["n_each"], what
    assert np.array_equal(np.array(got["pos"]), np.array(want["pos"])), what + ": get_position"
    assert got["alpha"] == want["alpha"] and got["elapsed"] == want["elapsed"], what
    if not root:  # the render rank answers the rest
        assert got["image"] is None and got["env"] == [None, None] and got["canvas"] == [None, None]
        assert all(v is None for v in got["inst"]), what
        return
    a, b = got["image"], want["image"]
    print(what, "screen: differing values", int((a != b).sum()), "max |diff|", float(np.abs(a - b).max()))
    assert a.shape == b.shape and np.array_equal(a, b), what + ": screen"
    for w in (WHITE, YOLK):
        cg, ch = got["canvas"][w], want["canvas"][w]
        if isinstance(ch, str):
            assert isinstance(cg, str), what
        else:
            assert cg[0].shape == ch[0].shape and np.array_equal(cg[0], ch[0]) and cg[1] == ch[1], "%s: canvas %d" % (what, w)
        assert len(got["env"][w]) == 10 and sorted(got["env"][w]) == sorted(want["env"][w])
        for k, v in want["env"][w].items():
            assert np.array_equal(got["env"][w][k], v), "%s: environment %d %s: %r != %r" % (what, w, k, got["env"][w][k], v)
        assert got["inst"][w].shape == want["inst"][w].shape and got["inst"][w].shape[1] == 7
        assert np.array_equal(got["inst"][w], want["inst"][w]), "%s: instance data %d" % (what, w)


def _one_handler(egg, name):
    """ONE SimulationHandler in this process doing what the ranks did"""
    _cuts, configs, play = SCENES[name]
    h = egg.SimulationHandler(*_configs(configs))
    record = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        play(h, _probe_of(h, record))
    return record


def _run(egg, name, world):
    want = _one_handler(egg, name)
    res = _spawn(name, world)
    for rank in range(world):
        record, _extra = res[rank]
        assert len(record) == len(want) > 0
        for got, ref in zip(record, want):
            _same_probe(got, ref, "%s, %d ranks, rank %d, %s" % (name, world, rank, ref["tag"]), rank == 0)
    return res, want


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


# ------------------------------------------------------------------------------------------------ tests

@pytest.mark.parametrize("world", [1, 2, 4])
def test_exact_order_cut_through_the_cluster(egg, world):
    res, want = _run(egg, "four_exact", world)
    first, last = want[0], want[-1]
    assert first["tag"] == "before the first step" and isinstance(first["canvas"][0], str)  # nothing drawn: the clear colour
    assert np.array_equal(first["image"], np.broadcast_to(np.float32(CLEAR), first["image"].shape))
    assert last["image"][..., 3].max() > 0.9 and not np.array_equal(want[1]["image"], last["image"])  # it is in the picture, and moves
    if world > 1:
        assert len(set(res[0][1]["owner"].values())) >= 2  # the batches lie on several ranks
        c = res[0][1]["counters"]
        assert c["draws"] == 4 * 5 and c["messages"] == 4 * 6 * (world - 1)  # per probe: draw (2 types) + 2 environments + 2 downloads


@pytest.mark.parametrize("world", [2, 4])
def test_relaxed_order_cut_through_the_cluster(egg, world):
    res, _want = _run(egg, "four_relaxed", world)
    assert sum(res[r][1]["halo"]["records"] for r in range(world)) > 0  # the cluster lay on both sides of a cut
    if world == 4:
        assert res[3][1]["n_local"] == (0, 0)  # a rank that owns nothing is normal


def test_two_columns_swap_sides_exact_relaxed_exact(egg):
    res, _want = _run(egg, "swap2", 2)
    assert res[0][1]["migrations"] > 0  # drawn before, during and after the hand-overs


def test_four_slabs_columns_cross(egg):
    res, _want = _run(egg, "swap4", 4)
    assert res[0][1]["migrations"] > 0


@pytest.mark.parametrize("world", [1, 2, 4])
def test_colours_switches_live_config_remove_and_add(egg, world):
    res, want = _run(egg, "colours", world)
    images = {p["tag"]: p["image"] for p in want}
    assert not np.array_equal(images["particle colours"], images["retinted"])
    assert not np.array_equal(images["retinted"], images["no lighting, config colours"])
    assert 0.2 < want[-1]["alpha"] < 0.3
    if world == 4:  # (slabs wider than a claim swept towards its target: two ranks own nothing)
        assert res[2][1]["n_local"] == (0, 0) and res[3][1]["n_local"] == (0, 0)
    # the wire model: per collective and sender 56 B per particle it holds + one 8 B status word
    if world == 2:
        sent = res[1][1]["counters"]
        assert sent["messages"] == 6 * len(want)
        assert res[0][1]["counters"]["bytes"] == sent["bytes"]  # the render rank received exactly that
        # per probe three collectives per type (draw, environment, instance data), each 56 B per particle held + 8 B
        assert sent["bytes"] == sum(3 * (56 * p["n_local"][w] + 8) for p in res[1][0] for w in (WHITE, YOLK))


def test_a_step_in_flight_on_one_rank_refuses_the_draw_on_every_rank(egg):
    h = egg.SimulationHandler()
    for x, y in TEN:
        h.add(x, y, 50, 15)
    for _ in range(3):
        h.step(1 / 60, 2, 3)
    want = []
    probe = _probe_of(h, want)
    probe("before")
    probe("after")
    res = _spawn("in_flight", 2)
    for rank in (0, 1):
        before, refused, after = res[rank][0]
        assert refused["raised"] is not None, "rank %d drew while rank 1 had a step open" % rank
        _same_probe(before, want[0], "in flight, rank %d, before" % rank, rank == 0)
        _same_probe(after, want[1], "in flight, rank %d, after" % rank, rank == 0)  # and the next draw is bit-equal
    assert "a step is in flight" in res[1][0][1]["raised"] and "rank 1 could not pack" in res[0][0][1]["raised"]


def test_messages_in_device_memory_are_packed_and_placed_without_staging(egg):
    """With RCCL the wire tensors live on the GPU: egg_draw_pack writes straight into the tensor that is sent and
    egg_draw_source_place reads straight from the tensor that was received.  One process, no wire: a torch device tensor
    is the message of a second handle, placed beside the render handle's own particles in interleaved key order; the
    placed arrays must be the two handles' own arrays, batch by batch."""
    import torch
    a, b = egg.SimulationHandler(), egg.SimulationHandler()
    for k, (x, y) in enumerate(TEN):
        (a if k % 2 == 0 else b).add_many_keyed([x], [y], [k + 1], 50, 15)  # keys interleave the two handles
    for h in (a, b):
        for _ in range(2):
            h.step(1 / 60, 2, 3)
    for which in (WHITE, YOLK):
        n_each = a.get_n_particles(1)[which]
        na, nb = a.get_n_particles()[which], b.get_n_particles()[which]
        assert na == nb == 5 * n_each
        msg = torch.full((7 * nb + 3,), -1.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        b.draw_pack(which, msg.data_ptr(), nb)
        host = msg.cpu().numpy()
        mine, theirs = a.download_instance_data(which), b.download_instance_data(which)
        assert np.array_equal(host[:7 * nb].reshape(7, nb).T, theirs)  # written in place ...
        assert np.all(host[7 * nb:] == -1.0)                           # ... and nowhere else
        a.draw_source_layout(which, na + nb, n_each * np.arange(len(TEN)), np.ones((len(TEN), 4), np.float32))
        a.draw_source_place(which, 0, na, n_each * np.arange(5), 2 * n_each * np.arange(5))
        a.draw_source_place(which, msg.data_ptr(), nb, n_each * np.arange(5), 2 * n_each * np.arange(5) + n_each)
        want = np.stack([mine.reshape(5, n_each, 7), theirs.reshape(5, n_each, 7)], axis=1).reshape(-1, 7)
        assert not np.array_equal(want[:, 0], want[:, 2])  # (stepped: last_x is not x)
        for f, name in enumerate(("x", "y", "last_x", "last_y", "vx", "vy", "radius")):
            assert np.array_equal(a.draw_source_download(which, name, na + nb), want[:, f]), (which, name)


def test_sharded_image_matches_the_render_model(egg, oracle_mod):
    """a sharded image against oracle/render_model.py fed with the oracle's states, as
    tests/test_gpu_group_draw.py::test_group_image_matches_the_render_model does for a group"""
    from oracle import render_model as model
    o = oracle_mod.Oracle()
    for x, y in TEN:
        o.add(x, y, 50, 15)
    for _ in range(3):
        o.step(1 / 60, 2, 3)
    got = _spawn("in_flight", 2)[0][0][0]  # the probe before the refusal: ten batches over two ranks, three steps
    states = [{k: o.field(w, k) for k in ("x", "y", "last_x", "last_y", "vx", "vy", "radius")} for w in (WHITE, YOLK)]
    for w in (WHITE, YOLK):
        for f, k in enumerate(("x", "y", "last_x", "last_y", "vx", "vy", "radius")):
            assert np.array_equal(got["inst"][w][:, f], states[w][k]), (w, k)
    colors = [np.ones((states[w]["x"].size, 4), np.float32) for w in (WHITE, YOLK)]
    ref, canvases = model.render(states, [o.env(w) for w in (WHITE, YOLK)], model.DEFAULT_RENDER, colors, SIZE, ALPHA, ORIGIN, None, None, CLEAR)
    for w in (WHITE, YOLK):
        canvas, (x0, y0) = got["canvas"][w]
        assert canvas.shape == canvases[w].shape and np.array_equal(canvas, canvases[w]), w
        env = o.env(w)
        assert (x0, y0) == (env["centroid_x"] - 0.5 * canvas.shape[1], env["centroid_y"] - 0.5 * canvas.shape[0])
        for k, v in got["env"][w].items():
            if k in env:
                assert v == env[k], (w, k)
    assert got["image"].shape == ref.shape and np.array_equal(got["image"], ref)
    assert got["image"][..., 3].max() > 0.9
