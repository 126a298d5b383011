"""The instanced-draw record packed on the device (egg_get_instances, egg_instances_begin / _end, egg_group_get_instances,
egg_draw_source_instances; DESIGN.md section 2.6, "The instanced-draw record").

Every DATA comparison is bit for bit (view(np.uint32)) against the existing download path --
download_instance_data(which).astype(np.float32) of ONE SimulationHandler -- and every COLOUR comparison against the
array the test builds itself from the colours it passed to add / set_white_color / set_yolk_color / set_white_config, by
the rule of DESIGN 2.6 (`_Colours` below).  Nothing is compared against the new code's own output, except where the
point is that two forms of it return the same bytes (two halves vs synchronous, device vs host destination, two packs of
one state).  Sharded ranks are spawned processes on GPU 0 over gloo, as in test_gpu_sharded_draw.py: at most 4 ranks +
the parent, every child joined with a time limit, the queue read with a time limit, no retries."""
import copy
import math
import os
import sys
import warnings

import numpy as np
import pytest

from conftest import ROOT, circle_target, load_golden

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
INF = math.inf


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    diff = int((_bits(got) != _bits(want)).sum())
    print(what, got.shape, "differing values:", diff)
    assert diff == 0, what


def _want_data(h, which):
    """the existing path: seven float64 downloads, interleaved and narrowed on the host"""
    return h.download_instance_data(which).astype(np.float32).reshape(-1, 7)


class _Colours:
    """The rule of DESIGN 2.6 / include/eggsim.h, from the calls the test makes: per batch and type the rgba its particles
    carry.  add: white unless _use_particle_color, else the colour argument (not clamped) or -- none given -- the
    config's colour at that moment; set_*_color: the batch's particles take the clamped colour, and so does the config's
    table while the batch shares it; set_*_config: the config gets a new table, every batch keeps what it has."""

    def __init__(self, egg):
        white, yolk = egg.default_configs()
        self.cfg = [list(white["color"]), list(yolk["color"])]
        self.flag = False
        self.pcolor, self.own, self.counts = {}, {}, {}

    def add(self, bid, counts, white=None, yolk=None):
        self.counts[bid] = counts
        self.own[bid] = [white is not None, yolk is not None]
        self.pcolor[bid] = [[1.0, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0]]
        if self.flag:
            self.pcolor[bid] = [list(c) if c is not None else list(self.cfg[w]) for w, c in enumerate((white, yolk))]

    def set_color(self, bid, which, rgba):
        c = [min(max(float(v), 0.0), 1.0) for v in rgba]
        self.pcolor[bid][which] = c
        if not self.own[bid][which]:
            self.cfg[which] = list(c)

    def set_config_color(self, which, rgba):
        self.cfg[which] = list(rgba)
        for own in self.own.values():
            own[0] = own[1] = True  # (the Python surface re-sends both render configs: both types get new tables)

    def remove(self, bid):
        for t in (self.pcolor, self.own, self.counts):
            del t[bid]

    def mesh(self, which):
        rows = [np.tile(np.float32(self.pcolor[b][which]), (self.counts[b][which], 1)) for b in sorted(self.pcolor)]
        return np.concatenate(rows) if rows else np.zeros((0, 4), np.float32)


def _check(sim, ref, colours, what, which=(WHITE, YOLK)):
    """sim.instances() against ref's download path and the colour model; returns the version"""
    version = None
    for w in which:
        got = sim.instances(w)
        assert len(got) == 3
        data, color, v = got
        _same_bits(data, _want_data(ref, w), "%s: data %d" % (what, w))
        if colours is not None:
            _same_bits(color, colours.mesh(w), "%s: colour %d" % (what, w))
        d2, c2, v2 = sim.instances(w, color=False)
        assert c2 is None and v2 == v and np.array_equal(_bits(d2), _bits(data))
        assert version in (None, v)
        version = v
    return version


# ------------------------------------------------------------------------------------------------ one handle: data

@pytest.mark.parametrize("name", ["four_batches", "cfg1_moving"])
def test_single_handle_data_on_the_goldens(egg, name):
    g = load_golden(name)
    centers = [tuple(float(v) for v in c) for c in g["centers"]]
    S, C = int(g["substeps"]), int(g["collision_steps"])
    h = egg.SimulationHandler()
    assert h.instances(WHITE)[0].shape == (0, 7) and h.instances(YOLK)[1].shape == (0, 4)  # zero particles is valid
    ids = [h.add(x, y, 50, 15) for x, y in centers]
    _check(h, h, None, "%s, before the first step" % name)  # last_x / last_y: whatever the download returns then
    for k in range(30):
        if bool(g["moving"]):
            for i, c in zip(ids, centers):
                h.set_target_position(i, *circle_target(c, k))
        assert h.update(1 / 60, 1 / 60, S, C) == 1
        if k + 1 in (1, 30):
            _check(h, h, None, "%s, step %d" % (name, k + 1))
    data = h.instances(WHITE)[0]
    assert np.abs(data[:, 4:6]).max() > 0 and not np.array_equal(data[:, 0], data[:, 2])  # velocities and last positions are live


def test_single_handle_data_config2_full_size(egg):
    from bench import grid_positions
    xs, ys, _side = grid_positions(256)
    h = egg.SimulationHandler()
    ids = h.add_many(xs, ys, 50, 15)
    assert sum(h.get_n_particles()) == 44032
    for k in range(3):
        dx, dy = circle_target((0.0, 0.0), 2 * k)
        h.set_target_positions(ids, xs + dx, ys + dy)
        h.step(1 / 60, 2, 3)
    _check(h, h, None, "config 2, step 3")
    # determinism: two packs of the same state are byte-equal, colour included
    for w in (WHITE, YOLK):
        a, b = h.instances(w), h.instances(w)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


@pytest.mark.parametrize("order", ["exact", "relaxed"])
def test_single_handle_data_after_remove_and_add(egg, order):
    centers = [tuple(float(v) for v in c) for c in load_golden("four_batches")["centers"]]
    h = egg.SimulationHandler()
    if order == "relaxed":
        h.set_solver_order("relaxed")
    ids = [h.add(x, y, 50, 15) for x, y in centers]
    for k in range(4):
        for i, c in zip(ids, centers):
            h.set_target_position(i, *circle_target(c, k))
        h.step(1 / 60, 2, 3)
    v0 = _check(h, h, None, order + ", stepped")
    h.remove(ids[1])
    v1 = _check(h, h, None, order + ", removed")
    for _ in range(2):
        h.step(1 / 60, 2, 3)
    new = h.add(60.0, -40.0, 40, 12, None, None, 90, 20)
    v2 = _check(h, h, None, order + ", added")
    for _ in range(3):
        h.step(1 / 60, 2, 3)
    v3 = _check(h, h, None, order + ", stepped again")
    assert v0 < v1 < v2 == v3 and h.get_n_particles(new) == (90, 20)
    if order == "relaxed":
        assert h.stats()["relaxed_steps"] == 9
    with pytest.raises(egg.EggError, match="buffer holds"):  # cap too small: the existing status, nothing written
        h.instances_to(WHITE, np.empty(7, np.float32).ctypes.data, 0, 1)


# ------------------------------------------------------------------------------------------------ one handle: colour

def _colour_scene(egg, sim, ref, probe):
    """plays the colour calls on `sim` (and on `ref`, when that is another object) and on the model; probe(tag, model)
    after every call that can change a colour"""
    m = _Colours(egg)
    both = [sim] if ref is sim else [sim, ref]

    def add(x, y, white=None, yolk=None, counts=(157, 15), **kw):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # (an out-of-range colour argument warns and is not clamped)
            got = [s.add(x, y, 50, 15, copy.copy(white), copy.copy(yolk), **kw) for s in both]
        assert len(set(got)) == 1
        m.add(got[0], counts, white, yolk)
        return got[0]

    def each(f):
        for s in both:
            f(s)

    def flag(on):
        m.flag = on
        for s in both:
            s._use_particle_color = on
    flag(True)
    a = add(300.0, 300.0, [0.9, 0.3, 0.3, 1.0], [0.2, 0.8, 0.4, 1.0])
    b = add(700.0, 320.0)                                  # colourless: shares the config's tables
    c = add(340.0, 330.0, None, [0.3, 0.3, 1.0, 1.0], (90, 20), white_n_particles=90, yolk_n_particles=20)
    d = add(660.0, 280.0, [1.5, 0.5, -0.5, 1.0])           # out of range: add does not clamp
    for k in range(6):
        add(150.0 + 140.0 * k, 520.0)
    each(lambda s: s.step(1 / 60, 2, 3))
    probe("particle colours", m)
    each(lambda s: s.set_white_color(b, 0.2, 0.9, 0.9))    # ... and the config's table, which b shares
    m.set_color(b, WHITE, [0.2, 0.9, 0.9, 1.0])
    probe("set_white_color on a colourless batch", m)
    e = add(900.0, 300.0)                                  # takes the retinted config colour
    probe("a colourless batch after the retint", m)
    each(lambda s: s.set_yolk_color(a, 1.0, 1.0, 0.0, 0.5))
    m.set_color(a, YOLK, [1.0, 1.0, 0.0, 0.5])
    probe("set_yolk_color on a coloured batch", m)
    white = sim.get_white_config()
    each(lambda s: s.set_white_config(dict(white, color=[0.5, 0.6, 0.7, 1.0])))
    m.set_config_color(WHITE, [0.5, 0.6, 0.7, 1.0])
    probe("set_white_config", m)
    each(lambda s: s.set_white_color(b, 0.1, 0.2, 0.3))    # the config's table is a new one: b keeps its own
    m.set_color(b, WHITE, [0.1, 0.2, 0.3, 1.0])
    f = add(1100.0, 300.0)                                 # the new config colour, not b's
    probe("after the config change", m)
    each(lambda s: s.remove(c))
    m.remove(c)
    probe("removed", m)
    flag(False)
    probe("_use_particle_color off: what the particles carry stays", m)
    g = add(1300.0, 300.0, [0.3, 0.3, 0.3, 1.0])           # created white whatever the argument is (L:985-990)
    probe("a batch added with the switch off", m)
    assert len({a, b, c, d, e, f, g}) == 7
    return m


def test_single_handle_colour_and_version(egg):
    h = egg.SimulationHandler()
    versions = []

    def probe(tag, m):
        v = _check(h, h, m, tag)
        h.update(1 / 60)                                   # stands still over update
        assert h.instances(WHITE)[2] == v and h.instances(YOLK, color=False)[2] == v
        versions.append(v)
    m = _colour_scene(egg, h, h, probe)
    print("colour versions", versions)
    assert all(b > a for a, b in zip(versions, versions[1:])) and len(versions) == 9
    assert len({tuple(c[0]) for c in m.pcolor.values()}) >= 5  # the scene has distinct colours to tell apart


def test_all_white_with_particle_colour_off(egg):
    h = egg.SimulationHandler()
    m = _Colours(egg)
    for k, col in enumerate(([0.9, 0.1, 0.1, 1.0], None, [0.1, 0.1, 0.9, 0.5])):
        m.add(h.add(200.0 + 200.0 * k, 300.0, 50, 15, col, col), (157, 15), col, col)
    h.step(1 / 60, 2, 3)
    _check(h, h, m, "switch off")
    for w in (WHITE, YOLK):
        assert np.array_equal(h.instances(w)[1], np.ones((h.get_n_particles()[w], 4), np.float32))


# ------------------------------------------------------------------------------------------------ two halves

def test_two_halves_return_the_synchronous_bytes(egg):
    centers = [tuple(float(v) for v in c) for c in load_golden("four_batches")["centers"]]
    h = egg.SimulationHandler()
    h._use_particle_color = True
    ids = [h.add(x, y, 50, 15, [0.1 * (k + 1), 0.5, 0.5, 1.0], None) for k, (x, y) in enumerate(centers)]
    frames, kept = [], []
    for k in range(3):
        for i, c in zip(ids, centers):
            h.set_target_position(i, *circle_target(c, k))
        h.step(1 / 60, 2, 3)
        sync = [h.instances(w) for w in (WHITE, YOLK)]
        h.instances_begin()
        with pytest.raises(egg.EggError, match="has not been ended"):  # a second begin without an end
            h.instances_begin()
        got = [h.instances_end(w) for w in (WHITE, YOLK)]
        with pytest.raises(egg.EggError, match="no egg_instances_begin is open"):
            h.instances_end(WHITE)
        for w in (WHITE, YOLK):
            assert got[w][0].tobytes() == sync[w][0].tobytes() and got[w][1].tobytes() == sync[w][1].tobytes(), (k, w)
            assert got[w][2] == sync[w][2] and not got[w][0].flags.writeable
            _same_bits(np.array(got[w][0]), _want_data(h, w), "two halves, frame %d, type %d" % (k, w))
        frames.append(got)
        kept.append([(got[w][0].copy(), got[w][1].copy()) for w in (WHITE, YOLK)])
    for w in (WHITE, YOLK):
        addr = [f[w][0].ctypes.data for f in frames]
        caddr = [f[w][1].ctypes.data for f in frames]
        assert addr[0] != addr[1] and addr[0] == addr[2]  # two buffers alternate: consecutive frames come from different ones
        assert caddr[0] == caddr[1] == caddr[2] and frames[0][w][2] == frames[2][w][2]  # no colour change: pointer and version stand
        # ... and the views of the frame before the last still hold its bytes: only the second following begin reuses a buffer
        assert frames[1][w][0].tobytes() == kept[1][w][0].tobytes() and frames[2][w][0].tobytes() == kept[2][w][0].tobytes()
        assert kept[1][w][0].tobytes() != kept[2][w][0].tobytes()
    before = frames[2][WHITE][1].copy()
    h.set_white_color(ids[0], 0.0, 1.0, 0.0)
    h.instances_begin((WHITE,))
    data, color, version = h.instances_end(WHITE)
    with pytest.raises(egg.EggError):
        h.instances_end(YOLK)  # not in the mask
    assert version > frames[2][WHITE][2] and color.ctypes.data != frames[2][WHITE][1].ctypes.data
    assert np.array_equal(frames[2][WHITE][1], before)  # the colour handed out last keeps its bytes in the other buffer
    assert np.array_equal(color[:157], np.tile(np.float32([0.0, 1.0, 0.0, 1.0]), (157, 1))) and np.array_equal(color[157:], before[157:])


def test_begin_is_refused_while_a_step_is_in_flight(egg):
    h = egg.SimulationHandler()
    for k in range(3):
        h.add(300.0 + 200.0 * k, 300.0, 50, 15)
    h.step(1 / 60, 2, 3)
    h.step_begin(1 / 60, 2, 3)
    with pytest.raises(egg.EggError, match="a step is in flight"):
        h.instances_begin()
    with pytest.raises(egg.EggError, match="a step is in flight"):
        h.instances(WHITE)
    h.step_end(True)
    _check(h, h, None, "after the refused begin")  # the handle is usable afterwards
    h.instances_begin()
    h.step(1 / 60, 2, 3)  # a step between begin and end runs behind the pack: the frame is the one of the begin
    want = [_want_data(h, w) for w in (WHITE, YOLK)]
    got = [h.instances_end(w)[0] for w in (WHITE, YOLK)]
    for w in (WHITE, YOLK):
        assert np.array_equal(_bits(got[w][:, 0:2]), _bits(want[w][:, 2:4]))  # its positions are the next frame's last_x / last_y
        assert not np.array_equal(got[w][:, 0:2], want[w][:, 0:2])


def test_device_memory_destination(egg):
    import torch
    h = egg.SimulationHandler()
    h._use_particle_color = True
    for k in range(5):
        h.add(300.0 + 120.0 * k, 300.0, 50, 15, [0.2 * k, 0.5, 0.5, 1.0], None)
    for _ in range(2):
        h.step(1 / 60, 2, 3)
    for w in (WHITE, YOLK):
        data, color, version = h.instances(w)
        n = data.shape[0]
        d = torch.zeros(7 * n + 1, dtype=torch.float32, device="cuda:0")
        c = torch.zeros(4 * n, dtype=torch.float32, device="cuda:0")
        assert h.instances_to(w, d.data_ptr(), c.data_ptr(), n) == (n, version)
        torch.cuda.synchronize()
        assert d[:7 * n].cpu().numpy().tobytes() == data.tobytes() and c.cpu().numpy().tobytes() == color.tobytes()
        assert float(d[7 * n]) == 0.0  # nothing past the last record
        d.zero_()
        assert h.instances_to(w, d.data_ptr() + 4, 0, n) == (n, version)  # 4-byte aligned only: packed aside, copied in
        torch.cuda.synchronize()
        assert d[1:].cpu().numpy().tobytes() == data.tobytes() and float(d[0]) == 0.0


# ------------------------------------------------------------------------------------------------ device group

GROUP_CUTS = {2: [-INF, 10.0, INF], 4: [-INF, -10.0, 15.0, 100.0, INF]}  # through the cluster of four_batches


@pytest.mark.parametrize("order", ["exact", "relaxed"])
@pytest.mark.parametrize("n_handles", [2, 4])
def test_group_equals_one_handle(egg, n_handles, order):
    centers = [tuple(float(v) for v in c) for c in load_golden("four_batches")["centers"]]
    g = egg.SimulationGroup([0] * n_handles, cuts=GROUP_CUTS[n_handles])
    h = egg.SimulationHandler()
    m = _Colours(egg)
    m.flag = True
    for s in (g, h):
        if order == "relaxed":
            s.set_solver_order("relaxed")
        s._use_particle_color = True
    cols = [([0.9, 0.3, 0.3, 1.0], None), (None, None), (None, [0.3, 0.3, 1.0, 0.5]), ([0.1, 0.9, 0.1, 1.0], [0.9, 0.9, 0.1, 1.0])]
    ids = []
    for (x, y), (wc, yc) in zip(centers, cols):
        ids.append(g.add(x, y, 50, 15, wc, yc))
        assert h.add(x, y, 50, 15, wc, yc) == ids[-1]
        m.add(ids[-1], (157, 15), wc, yc)
    assert len({g.owner(i)[0] for i in ids}) >= 2  # the batches start on different handles
    v = [_check(g, h, m, "%s, %d handles, before the first step" % (order, n_handles))]
    owners = {tuple(g.owner(i)[0] for i in ids)}
    for k in range(30):
        for i, c in zip(ids, centers):
            for s in (g, h):
                s.set_target_position(i, *circle_target(c, k))
        g.step(1 / 60, 2, 3)
        h.step(1 / 60, 2, 3)
        owners.add(tuple(g.owner(i)[0] for i in ids))
        if k + 1 in (1, 10, 30):
            v.append(_check(g, h, m, "%s, %d handles, step %d" % (order, n_handles, k + 1)))
    print("owners seen", sorted(owners), "migrations", g.counters()["migrations"])
    assert g.counters()["migrations"] > 0 and len(owners) > 1  # compared before and after steps that hand batches over
    assert len(set(v)) == 1  # hand-overs change no colour and no count
    for s in (g, h):
        s.set_yolk_color(ids[1], 0.4, 0.5, 0.6)
    m.set_color(ids[1], YOLK, [0.4, 0.5, 0.6, 1.0])
    for s in (g, h):
        s.remove(ids[0])
    m.remove(ids[0])
    assert _check(g, h, m, "%s, %d handles, retinted and removed" % (order, n_handles)) > v[-1]


# ------------------------------------------------------------------------------------------------ sharded

SHARD_CUTS = {2: [-2000.0, 10.0, 2000.0], 4: [-2000.0, 10.0, 400.0, 2000.0, 4000.0]}
FILLERS = [(-300.0, -100.0), (-170.0, -100.0), (330.0, -100.0), (460.0, -100.0), (-300.0, 330.0), (460.0, 330.0)]


def _shard_scene(egg, sim, probe):
    """ten batches (a budget that cannot bind), the cluster of four_batches cut by the slabs; colours on some"""
    centers = [tuple(float(v) for v in c) for c in load_golden("four_batches")["centers"]] + FILLERS
    m = _Colours(egg)
    m.flag = True
    sim._use_particle_color = True
    ids = []
    for k, (x, y) in enumerate(centers):
        wc = [0.1 * k, 0.5, 1.0 - 0.1 * k, 1.0] if k % 3 == 0 else None
        yc = [0.5, 0.1 * k, 0.5, 0.75] if k % 4 == 1 else None
        ids.append(sim.add(x, y, 50, 15, wc, yc))
        m.add(ids[-1], (157, 15), wc, yc)
    probe("before the first step", m)
    for k in range(12):
        for i, c in zip(ids, centers):
            if c not in FILLERS:
                sim.set_target_position(i, *circle_target(c, k))
        sim.step(1 / 60, 2, 3)
        if k + 1 in (1, 12):
            probe("step %d" % (k + 1), m)
    sim.set_white_color(ids[1], 0.2, 0.9, 0.9)
    m.set_color(ids[1], WHITE, [0.2, 0.9, 0.9, 1.0])
    sim.remove(ids[4])
    m.remove(ids[4])
    probe("retinted and removed", m)


def _shard_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    import egg_fluid_simulation_amd as egg
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler, SlabLayout
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        record = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sh = ShardedSimulationHandler(SlabLayout(SHARD_CUTS[world]), rank, dist, lambda: egg.SimulationHandler(device=0), device="cpu")

            def probe(tag, m):
                before = sh.draw_counters()["messages"]
                got = [sh.instances(w) for w in (WHITE, YOLK)]
                record.append(dict(tag=tag, got=got, messages=sh.draw_counters()["messages"] - before, n_local=sh.local.get_n_particles()))
            _shard_scene(egg, sh, probe)
        q.put((rank, "ok", (record, sh.migrations)))
    except Exception:
        import traceback
        q.put((rank, "error: " + traceback.format_exc(), None))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_equals_one_handle(egg, world):
    import queue
    import time

    import torch.multiprocessing as mp
    from test_gpu_sharded_draw import _free_port
    want = []
    h = egg.SimulationHandler()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _shard_scene(egg, h, lambda tag, m: want.append(dict(tag=tag, data=[_want_data(h, w) for w in (WHITE, YOLK)],
                                                             color=[m.mesh(w) for w in (WHITE, YOLK)])))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_shard_worker, args=(r, world, port, q)) for r in range(world)]
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
    versions = []
    for k, ref in enumerate(want):
        for rank in range(world):
            rec = res[rank][0][k]
            assert rec["tag"] == ref["tag"]
            assert rec["messages"] == (2 * (world - 1) if rank == 0 else 2)  # ONE gather per call and type
            if rank != 0:
                assert rec["got"] == [None, None]  # answered on the render rank only
                continue
            for w in (WHITE, YOLK):
                data, color, version = rec["got"][w]
                what = "%d ranks, %s, type %d" % (world, ref["tag"], w)
                _same_bits(data, ref["data"][w], what + ": data")
                _same_bits(color, ref["color"][w], what + ": colour")
            versions.append(rec["got"][0][2])
            assert rec["got"][1][2] == versions[-1]
    assert versions[0] == versions[1] == versions[2] < versions[3]
    assert len({res[r][0][1]["n_local"] for r in range(world)}) > 1  # the particles lie on several ranks
