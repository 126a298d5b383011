"""Fields (egg_field) on the device against the CPU model tests/field_model.py run on the handle's
own downloads: every comparison is equality of integers.

The hand table of tests/test_field_model.py (particles placed through export_batch / import_batch), batch sizes on every
seam of the scan (two lanes, a full wave, one more, a full unit, one more, three units), the seams of the grid (1 x 1, one
row, one column, nx = 65) and of the tile (a unit whose rectangle is exactly EGG_FD_TILE_CELLS cells and one of one cell
more, every particle in one cell, every particle in a cell of its own, a unit half and wholly outside), path="direct"
against path="auto" on every case, count-only against velocity, field_to into torch tensors, four default eggs after 5
relaxed and after 5 exact-order steps, a 1,024 x 1,024 grid, fields only observe, a step in flight, device groups of 2 and
3 handles on GPU 0 and a ShardedSimulationHandler of two spawned ranks on GPU 0 over gloo."""
import ctypes as C

import numpy as np
import pytest

import field_model as fm
import test_field_model as tf
from conftest import ROOT

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
FIELDS = ("x", "y", "vx", "vy", "last_x", "last_y")
H60, S, C3 = 1 / 60, 2, 3
INF = float("inf")
TILE_CELLS = 1024  # EGG_FD_TILE_CELLS


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _placed(egg, white, yolk):
    """a handle with one batch whose particles have the given (x, y, vx, vy)"""
    src = egg.SimulationHandler()
    i = src.add(0.0, 0.0, 50, 15, None, None, len(white), len(yolk))
    info, ws, ys = src.export_batch(i)
    for state, spots in ((ws, white), (ys, yolk)):
        assert state.shape[1] == len(spots)
        a = np.asarray(spots, dtype=np.float64).reshape(len(spots), 4)
        state[0] = state[4] = a[:, 0]
        state[1] = state[5] = a[:, 1]
        state[2], state[3] = a[:, 2], a[:, 3]
    h = egg.SimulationHandler()
    assert h.import_batch(info, ws, ys) == i
    return h


def _model(h, grid, types, velocity):
    d = [[h.download(w, f) for w in (WHITE, YOLK)] for f in ("x", "y", "vx", "vy")]
    return fm.field(grid, d[0], d[1], d[2], d[3], types, velocity)


def _as_model(f):
    return (f.count, f.svx, f.svy, f.inside, f.outside, f.dropped)


def _assert_field(h, grid, what, types="both", velocity=True):
    """field() of h on both paths is the model's over h's own downloads; returns the automatic path's Field"""
    x0, y0, cell, nx, ny = grid
    want = _model(h, grid, types, velocity)
    auto = h.field((x0, y0), cell, (nx, ny), types, velocity)
    direct = h.field((x0, y0), cell, (nx, ny), types, velocity, "direct")
    print("%s: inside %s outside %s dropped %s tiled %d direct %d | direct path: tiled %d direct %d" % (
        what, auto.inside, auto.outside, auto.dropped, auto.units_tiled, auto.units_direct, direct.units_tiled, direct.units_direct))
    assert auto.count.dtype == np.int32 and auto.count.shape == (2, ny, nx), what
    assert tf.same(_as_model(auto), want), what
    assert tf.same(_as_model(direct), want) and direct.units_tiled == 0, what
    assert direct.units_direct == auto.units_tiled + auto.units_direct, what  # (the units that hold a particle inside)
    for w in (0, 1):
        n = h.get_n_particles()[w] if fm.MASKS[types] >> w & 1 else 0
        assert auto.inside[w] + auto.outside[w] + auto.dropped[w] == n, (what, w)
    if velocity:  # count-only: nothing is dropped, and the count plane is the same wherever nothing was
        plain = h.field((x0, y0), cell, (nx, ny), types, False)
        assert plain.svx is None and plain.svy is None and plain.dropped == (0, 0), what
        assert tf.same(_as_model(plain), _model(h, grid, types, False)), what
        if auto.dropped == (0, 0):
            assert np.array_equal(plain.count, auto.count) and plain.inside == auto.inside, what
        assert np.array_equal(auto.velocity(), fm.velocity(auto.count, auto.svx, auto.svy), equal_nan=True), what
    return auto


# ------------------------------------------------------------------------------------------------ the hand table
@pytest.mark.parametrize("name", sorted(tf.CASES))
def test_hand_case(egg, name):
    case = tf.CASES[name]
    h = _placed(egg, *case["spots"])
    x0, y0, cell, nx, ny = case["grid"]
    for path in ("auto", "direct"):
        got = h.field((x0, y0), cell, (nx, ny), case["types"], case["velocity"], path)
        assert tf.same(_as_model(got), tf.expected(name)), (name, path, got)
    _assert_field(h, case["grid"], name, case["types"], case["velocity"])


# ------------------------------------------------------------------------------------------------ the seams of the scan
def _line(n, x_from, x_to, slope, wobble):
    t = np.arange(n, dtype=np.float64)
    x = x_from + (x_to - x_from) * t / max(n - 1, 1)
    return list(zip(x, slope * x + wobble * np.cos(t), 3.0 * np.sin(t), -2.0 * np.cos(0.5 * t)))


@pytest.mark.parametrize("n", [2, 64, 65, 1024, 1025, 2500])
def test_batch_sizes_on_every_seam(egg, n):
    """n particles per type on a line that enters and leaves the grid: lanes of a partly filled wave, the step to a second
    chunk, the unit boundary at 1,024 and three units"""
    h = _placed(egg, _line(n, -130.0, 130.0, 0.05, 0.125), _line(n, -90.0, 150.0, 0.4, 0.01))
    f = _assert_field(h, (-100.0, -30.0, 3.0, 65, 21), "n = %d" % n)
    assert f.dropped == (0, 0) and (n < 64 or (0 < f.inside[0] < n and 0 < f.inside[1] < n)), f[3:]  # (the edges cut the lines)


# ------------------------------------------------------------------------------------------------ the seams of the grid and of the tile
def _cloud(n, seed, cx, cy, sx, sy):
    r = np.random.RandomState(seed)
    return list(zip(cx + sx * r.standard_normal(n), cy + sy * r.standard_normal(n), 40.0 * r.standard_normal(n), 40.0 * r.standard_normal(n)))


@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (37, 1), (65, 2)])
def test_grid_shapes(egg, shape):
    nx, ny = shape
    cell = 70.0 / max(nx, ny)
    wx, wy = nx * cell, ny * cell  # clouds about as wide as the grid: a good part of each type lies outside
    h = _placed(egg, _cloud(300, 1, 0.5 * wx, 0.5 * wy, 0.6 * wx, 0.6 * wy), _cloud(130, 2, 0.4 * wx, 0.6 * wy, 0.6 * wx, 0.6 * wy))
    f = _assert_field(h, (0.0, 0.0, cell, nx, ny), "%d x %d" % shape)
    assert all(0 < f.inside[w] and 0 < f.outside[w] for w in (0, 1)), f[3:]


def _corners(n, c0, c1, cell):
    """n particles at rest in the middle of cell c0, the last one in the middle of cell c1"""
    spots = [((c0[0] + 0.5) * cell, (c0[1] + 0.5) * cell, 1.0, -1.0)] * (n - 1)
    return spots + [((c1[0] + 0.5) * cell, (c1[1] + 0.5) * cell, 0.5, 0.25)]


@pytest.mark.parametrize("rect,tiled", [((32, 32), True), ((41, 25), False), ((1024, 1), True), ((1, 1025), False)])
def test_the_tile_threshold(egg, rect, tiled):
    """one white unit whose rectangle of cells is rect[0] x rect[1] -- exactly EGG_FD_TILE_CELLS cells, or one more -- and one
    yolk unit in a single cell: units_tiled / units_direct say which path ran"""
    assert rect[0] * rect[1] == TILE_CELLS + (0 if tiled else 1)
    white = _corners(70, (3, 2), (3 + rect[0] - 1, 2 + rect[1] - 1), 4.0)
    h = _placed(egg, white, _corners(20, (5, 5), (5, 5), 4.0))
    f = _assert_field(h, (0.0, 0.0, 4.0, rect[0] + 6, rect[1] + 6), "rect %d x %d" % rect)
    assert (f.units_tiled, f.units_direct) == ((2, 0) if tiled else (1, 1)), f[6:]
    assert f.count[0, 2, 3] == 69 and f.count[0, 2 + rect[1] - 1, 3 + rect[0] - 1] == 1 and f.count[1, 5, 5] == 20


def test_all_particles_in_one_cell(egg):
    h = _placed(egg, _cloud(2500, 3, 20.0, 12.0, 0.5, 0.5), _cloud(2500, 4, 20.0, 12.0, 0.5, 0.5))
    f = _assert_field(h, (0.0, 0.0, 8.0, 5, 3), "one cell")
    assert f.count[0, 1, 2] == f.count[1, 1, 2] == 2500 and f.count.sum() == 5000 and (f.units_tiled, f.units_direct) == (6, 0)


def test_every_particle_in_a_cell_of_its_own(egg):
    p = np.arange(2500)
    spots = list(zip(p % 64 + 0.5, p // 64 + 0.5, 1.0 + p, -1.0 * p))
    h = _placed(egg, spots, spots[:1500])
    f = _assert_field(h, (0.0, 0.0, 1.0, 64, 40), "own cells")
    assert f.count.max() == 1 and f.inside == (2500, 1500) and f.units_tiled == 5  # (1,024 consecutive cells are 16 rows of 64)


def test_units_half_and_wholly_outside(egg):
    h = _placed(egg, _cloud(1500, 5, 0.0, 20.0, 15.0, 10.0), _cloud(400, 6, -500.0, -500.0, 10.0, 10.0))
    f = _assert_field(h, (0.0, 0.0, 2.0, 40, 40), "outside")
    assert 0 < f.inside[0] < 1500 and f.inside[1] == 0 and f.outside[1] == 400 and not f.count[1].any()
    assert f.units_tiled + f.units_direct == 2  # (the yolk's unit holds nothing: neither path)


def test_masks_and_a_handle_without_particles(egg):
    h = _placed(egg, _cloud(100, 7, 20.0, 20.0, 8.0, 8.0), _cloud(100, 8, 20.0, 20.0, 8.0, 8.0))
    for types, other in (("white", YOLK), ("yolk", WHITE), (1, YOLK), (2, WHITE)):
        f = _assert_field(h, (0.0, 0.0, 4.0, 10, 10), "mask %s" % types, {1: "white", 2: "yolk"}.get(types, types))
        g = h.field((0.0, 0.0), 4.0, (10, 10), types, True)
        assert not g.count[other].any() and not g.svx[other].any() and g.inside[other] == g.outside[other] == 0 and g.count[1 - other].any()
        assert np.array_equal(g.count, f.count)
    empty = egg.SimulationHandler()
    before = empty.stats()["kernel_launches"]
    f = empty.field((0.0, 0.0), 4.0, (10, 10), velocity=True)
    assert not f.count.any() and not f.svx.any() and f[3:] == ((0, 0), (0, 0), (0, 0), 0, 0) and np.isnan(f.velocity()).all()
    assert empty.stats()["kernel_launches"] == before  # (nothing to launch)


# ------------------------------------------------------------------------------------------------ refusals
def test_a_bad_call_writes_nothing(egg):
    from egg_fluid_simulation_amd import _ffi
    h = _placed(egg, _cloud(10, 9, 5.0, 5.0, 2.0, 2.0), _cloud(10, 10, 5.0, 5.0, 2.0, 2.0))
    count = np.full((2, 4, 4), 77, dtype=np.int32)
    svx, svy = np.full((2, 4, 4), 78, dtype=np.int64), np.full((2, 4, 4), 79, dtype=np.int64)
    totals = _ffi.EggFieldTotals()
    totals.units_tiled = 55
    good = dict(x0=0.0, y0=0.0, cell=4.0, nx=4, ny=4, type_mask=3, path=0)
    planes = dict(count=count.ctypes.data, svx=svx.ctypes.data, svy=svy.ctypes.data)
    nan = float("nan")

    def call(spec=None, **p):
        s = _ffi.EggFieldSpec(**dict(good, **(spec or {})))
        q = _ffi.EggFieldPlanes(**dict(planes, **p))
        return h._lib.egg_field(h._h, C.byref(s), C.byref(q), C.byref(totals))
    for spec, p, text in ((dict(nx=0), {}, "nx, ny"), (dict(ny=-3), {}, "nx, ny"), (dict(nx=1024, ny=1025), {}, "nx, ny"),
                          (dict(cell=0.0), {}, "cell"), (dict(cell=-1.0), {}, "cell"), (dict(cell=nan), {}, "cell"), (dict(cell=INF), {}, "cell"),
                          (dict(cell=5e-324), {}, "cell"), (dict(x0=nan), {}, "x0, y0"), (dict(y0=INF), {}, "x0, y0"),
                          (dict(type_mask=0), {}, "type_mask"), (dict(type_mask=4), {}, "type_mask"), (dict(path=2), {}, "path"),
                          ({}, dict(count=None), "count is NULL"), ({}, dict(svx=None), "svx and svy"), ({}, dict(svy=None), "svx and svy")):
        assert call(spec, **p) == _ffi.EGG_ERR_INVALID_ARGUMENT, (spec, p)
        assert text in h._lib.egg_last_error(h._h).decode(), (spec, p, h._lib.egg_last_error(h._h))
    assert h._lib.egg_field(h._h, None, C.byref(_ffi.EggFieldPlanes(**planes)), C.byref(totals)) == _ffi.EGG_ERR_INVALID_ARGUMENT
    assert h._lib.egg_field(h._h, C.byref(_ffi.EggFieldSpec(**good)), None, C.byref(totals)) == _ffi.EGG_ERR_INVALID_ARGUMENT
    assert (count == 77).all() and (svx == 78).all() and (svy == 79).all() and totals.units_tiled == 55
    assert call() == 0 and count.sum() == totals.inside[0] + totals.inside[1] > 0 and totals.units_tiled == 2
    for bad, text in ((dict(shape=(0, 4)), "nx and ny are at least 1"), (dict(cell=0.0), "cell must be finite and above 0"),
                      (dict(types="none"), "types must be"), (dict(path="fast"), "path must be")):
        with pytest.raises(egg.EggError, match=text):
            h.field(**dict(dict(origin=(0.0, 0.0), cell=4.0, shape=(4, 4)), **bad))


def test_a_step_in_flight(egg):
    h = egg.SimulationHandler()
    for x, y in EGGS[:2]:
        h.add(x, y)
    held = _assert_field(h, EGG_GRID, "before")
    h.step_begin(H60, S, C3)
    with pytest.raises(egg.EggError, match="egg_field: a step is in flight"):
        h.field(EGG_GRID[:2], EGG_GRID[2], EGG_GRID[3:])
    import torch
    count = torch.full((2, 64, 64), 7, dtype=torch.int32, device="cuda:0")
    with pytest.raises(egg.EggError, match="egg_field_to: a step is in flight"):
        h.field_to(EGG_GRID[:2], EGG_GRID[2], EGG_GRID[3:], count)
    assert bool((count == 7).all())
    h.step_end(False)
    assert tf.same(_as_model(h.field(EGG_GRID[:2], EGG_GRID[2], EGG_GRID[3:], velocity=True)), _as_model(held))
    h.step_begin(H60, S, C3)
    h.step_end(True)
    assert not tf.same(_as_model(_assert_field(h, EGG_GRID, "after the committed step")), _as_model(held))


# ------------------------------------------------------------------------------------------------ field_to
def test_field_to_fills_torch_tensors(egg):
    import torch
    from egg_fluid_simulation_amd import _ffi
    h = _placed(egg, _cloud(1500, 11, 30.0, 30.0, 12.0, 12.0), _cloud(700, 12, 35.0, 25.0, 6.0, 6.0))
    origin, cell, shape = (0.0, 0.0), 1.5, (37, 41)
    want = h.field(origin, cell, shape, velocity=True)
    assert tf.same(_as_model(want), _model(h, origin + (cell,) + shape, "both", True))
    dev = torch.device("cuda:0")
    count = torch.full((2, 41, 37), 123, dtype=torch.int32, device=dev)  # (stale contents: the call zeroes them itself)
    svx = torch.full((2, 41, 37), -5, dtype=torch.int64, device=dev)
    svy = torch.full((2, 41, 37), 9, dtype=torch.int64, device=dev)
    for path in ("auto", "direct"):
        t = h.field_to(origin, cell, shape, count, svx, svy, path=path)
        assert np.array_equal(count.cpu().numpy(), want.count) and np.array_equal(svx.cpu().numpy(), want.svx)
        assert np.array_equal(svy.cpu().numpy(), want.svy) and t[:3] == want[3:6] and (path == "auto" or t.units_tiled == 0)
    count.fill_(55)
    t = h.field_to(origin, cell, shape, count.data_ptr(), types="yolk")  # (an address; count only; one type)
    assert np.array_equal(count.cpu().numpy()[1], want.count[1]) and not count[0].any() and t.inside == (0, want.inside[1]) and t.dropped == (0, 0)
    # an empty handle zero-fills on the device
    count.fill_(55)
    t = egg.SimulationHandler().field_to(origin, cell, shape, count)
    assert not count.any() and t == ((0, 0), (0, 0), (0, 0), 0, 0)
    # refused with the tensors untouched: a misaligned pointer (by the wrapper, and by the library itself), a tensor of
    # another size or type, host memory, svx without svy
    count.fill_(55)
    svx.fill_(-5)
    raw = torch.zeros(2 * 41 * 37 * 8 + 16, dtype=torch.uint8, device=dev)
    with pytest.raises(egg.EggError, match="svx is not aligned to 8 bytes"):
        h.field_to(origin, cell, shape, count, raw.data_ptr() + 4, svy)
    with pytest.raises(egg.EggError, match="count is not aligned to 4 bytes"):
        h.field_to(origin, cell, shape, raw.data_ptr() + 2)
    with pytest.raises(egg.EggError, match="svx and svy are given together"):
        h.field_to(origin, cell, shape, count, svx)
    with pytest.raises(egg.EggError, match="count must hold 2 x 41 x 37 elements"):
        h.field_to(origin, cell, shape, count[:1], svx, svy)
    with pytest.raises(egg.EggError, match="count must hold int32"):
        h.field_to(origin, cell, shape, svx)
    spec = _ffi.EggFieldSpec(0.0, 0.0, cell, 37, 41, 3, 0)
    totals = _ffi.EggFieldTotals()
    host = np.full((2, 41, 37), 3, dtype=np.int32)
    for planes, text in ((_ffi.EggFieldPlanes(count.data_ptr(), raw.data_ptr() + 4, svy.data_ptr()), "svx is not aligned to 8 bytes"),
                         (_ffi.EggFieldPlanes(count.data_ptr(), svx.data_ptr(), raw.data_ptr() + 12), "svy is not aligned to 8 bytes"),
                         (_ffi.EggFieldPlanes(raw.data_ptr() + 1, None, None), "count is not aligned to 4 bytes"),
                         (_ffi.EggFieldPlanes(host.ctypes.data, None, None), "count is not 12136 bytes of memory of device 0"),
                         (_ffi.EggFieldPlanes(count.data_ptr(), svx.data_ptr(), host.ctypes.data), "svy is not 24272 bytes of memory of device 0")):
        assert h._lib.egg_field_to(h._h, C.byref(spec), C.byref(planes), C.byref(totals)) == _ffi.EGG_ERR_INVALID_ARGUMENT, text
        assert text in h._lib.egg_last_error(h._h).decode(), (text, h._lib.egg_last_error(h._h))
    assert bool((count == 55).all()) and bool((svx == -5).all()) and np.array_equal(svy.cpu().numpy(), want.svy) and (host == 3).all()
    assert not raw.any() and totals.inside[0] == 0


# ------------------------------------------------------------------------------------------------ eggs that move
EGGS = ((300.0, 300.0), (360.0, 310.0), (330.0, 250.0), (420.0, 330.0))
EGG_GRID = (200.0, 180.0, 4.5, 64, 64)  # [200, 488) x [180, 468): the four eggs with room around them
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
    before = _assert_field(h, EGG_GRID, order + ": before a step")
    for _ in range(5):
        assert h.update(H60, H60, S, C3) == 1
    after = _assert_field(h, EGG_GRID, order + ": after 5 steps")
    assert not np.array_equal(before.count, after.count) and after.svx.any() and after.svy.any()  # (something moved)
    _assert_field(h, (250.0, 250.0, 1.0, 100, 60), order + ": cells finer than a particle, half the scene")


def test_a_full_size_grid(egg):
    h = egg.SimulationHandler()
    for x, y in EGGS:
        h.add(x, y)
    f = h.field((200.0, 180.0), 0.28125, (1024, 1024))
    want = _model(h, (200.0, 180.0, 0.28125, 1024, 1024), "both", False)
    assert tf.same(_as_model(f), want) and f.count.sum() == sum(f.inside) > 0
    with pytest.raises(egg.EggError, match="nx \\* ny at most 1048576"):
        h.field((200.0, 180.0), 0.28125, (1024, 1025))


def test_fields_only_observe(egg):
    """two handles stepped alike, one calling field() between steps: equal particles in every download, equal launches per
    step, and kernel_launches differs by the field calls alone"""
    a, b = _relaxed_scene(egg.SimulationHandler()), _relaxed_scene(egg.SimulationHandler())
    for h in (a, b):
        for x, y in EGGS:
            h.add(x, y)
    calls = 0
    for k in range(4):
        for h in (a, b):
            assert h.update(H60, H60, S, C3) == 1
        stats = a.stats()
        a.field(EGG_GRID[:2], EGG_GRID[2], EGG_GRID[3:], velocity=True)
        a.field(EGG_GRID[:2], EGG_GRID[2], EGG_GRID[3:], "white", False, "direct")
        calls += 2
        after = a.stats()
        assert after["kernel_launches"] == stats["kernel_launches"] + 2
        assert {key: v for key, v in after.items() if key != "kernel_launches"} == {key: v for key, v in stats.items() if key != "kernel_launches"}
        for w in (WHITE, YOLK):
            for f in FIELDS:
                assert np.array_equal(a.download(w, f), b.download(w, f)), (k, w, f)
    assert a.stats()["kernel_launches"] - b.stats()["kernel_launches"] == calls
    assert a.collider_hits() == b.collider_hits() and a.elapsed == b.elapsed


# ------------------------------------------------------------------------------------------------ device groups
CUTS = {2: [-INF, 335.0, INF], 3: [-INF, 320.0, 372.0, INF]}  # through the eggs
FAR_EGG = (900.0, 300.0)  # outside the grid: counted in `outside`


@pytest.mark.parametrize("n_handles", [2, 3])
def test_device_group_equals_one_handle(egg, n_handles):
    g = _relaxed_scene(egg.SimulationGroup([0] * n_handles, cuts=CUTS[n_handles]))
    h = _relaxed_scene(egg.SimulationHandler())
    ids = [g.add(x, y) for x, y in EGGS]
    assert [h.add(x, y) for x, y in EGGS] == ids
    assert len({g.owner(i)[0] for i in ids}) == n_handles
    origin, cell, shape = EGG_GRID[:2], EGG_GRID[2], EGG_GRID[3:]
    for k in range(3):
        g.step(H60, S, C3)
        h.step(H60, S, C3)
        want = _assert_field(h, EGG_GRID, "one handle, step %d" % (k + 1))
        for velocity in (True, False):
            got = g.field(origin, cell, shape, velocity=velocity)
            assert tf.same(_as_model(got), _as_model(h.field(origin, cell, shape, velocity=velocity))), (k, velocity)
        own = [b.field(origin, cell, shape).inside[WHITE] for b in g.handles]
        assert all(n > 0 for n in own) and sum(own) == want.inside[WHITE], own  # (every handle holds a part)
        assert tf.same(_as_model(g.field(origin, cell, shape, "yolk", True, "direct")), _as_model(h.field(origin, cell, shape, "yolk", True)))
    far = g.add(*FAR_EGG)
    assert h.add(*FAR_EGG) == far
    got, want = g.field(origin, cell, shape, velocity=True), _assert_field(h, EGG_GRID, "one handle with the far egg")
    assert tf.same(_as_model(got), _as_model(want)) and min(want.outside) > 0
    with pytest.raises(egg.EggError, match="cell"):
        g.field(origin, -1.0, shape)
    assert not hasattr(g, "field_to")


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
        for x, y in EGGS:
            sh.add(x, y, 50, 15)
        origin, cell, shape = EGG_GRID[:2], EGG_GRID[2], EGG_GRID[3:]
        steps = []
        for _ in range(3):
            sh.step(H60, S, C3)
            steps.append(dict(velocity=tuple(sh.field(origin, cell, shape, velocity=True)), plain=tuple(sh.field(origin, cell, shape, "white")),
                              own=sh.local.field(origin, cell, shape).inside))
        sh.add(FAR_EGG[0], FAR_EGG[1], 50, 15)
        last = tuple(sh.field(origin, cell, shape, velocity=True, path="direct"))
        q.put((rank, "ok", dict(steps=steps, last=last, has_to=hasattr(sh, "field_to"))))
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
    """two ranks on one GPU (three processes with the GPU open), the cut through the eggs: the all-reduced planes are one
    handle's on both ranks, and each rank's own are a part of them"""
    res = _spawn(2)
    h = _relaxed_scene(egg.SimulationHandler())
    for x, y in EGGS:
        h.add(x, y, 50, 15)
    origin, cell, shape = EGG_GRID[:2], EGG_GRID[2], EGG_GRID[3:]
    for k in range(3):
        h.step(H60, S, C3)
        want = _assert_field(h, EGG_GRID, "one handle, step %d" % (k + 1))
        plain = h.field(origin, cell, shape, "white")
        for r in (0, 1):
            got = res[r]["steps"][k]
            assert tf.same(got["velocity"][:6], _as_model(want)) and tf.same(got["plain"][:6], _as_model(plain)), (r, k)
        own = [res[r]["steps"][k]["own"] for r in (0, 1)]
        assert all(o[WHITE] > 0 for o in own) and tuple(a + b for a, b in zip(*own)) == want.inside, own
    h.add(FAR_EGG[0], FAR_EGG[1], 50, 15)
    want = _assert_field(h, EGG_GRID, "one handle with the far egg")
    for r in (0, 1):
        assert tf.same(res[r]["last"][:6], _as_model(want)) and res[r]["last"][6] == 0 and min(want.outside) > 0, r
        assert res[r]["has_to"] is False
