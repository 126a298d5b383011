"""Cover (egg_cover) on the device against the CPU model tests/cover_model.py run on the handle's own
downloads: every comparison is equality of integers, and every case runs on all four paths (auto, direct, lanes, wave).

The hand table of tests/test_cover_model.py (particles placed through export_batch / import_batch, radius included), batch
sizes on every seam of the scan, the seams of the grid (1 x 1, one row, one column, nx = 65), of the tile (a unit whose union
rectangle is exactly EGG_CV_TILE_CELLS cells and one of one cell more) and of the footprint (every disc exactly at the
lanes / wave bound, and one disc one cell above it), mixed radii in one wave, scale 1 and 12 on four default eggs after 5
relaxed and after 5 exact-order steps, the owner map while batches come and go, the types, cover_to into torch tensors and
its refusals, a step in flight, cover only observes, device groups of 2 and 3 handles on GPU 0 and a
ShardedSimulationHandler of two spawned ranks on GPU 0 over gloo."""
import ctypes as C

import numpy as np
import pytest

import cover_model as cm
import test_cover_model as tc
from conftest import ROOT
from test_gpu_probes import _template

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
FIELDS = ("x", "y", "vx", "vy", "last_x", "last_y", "radius")
H60, S, C3 = 1 / 60, 2, 3
INF = float("inf")
PATHS = ("auto", "direct", "lanes", "wave")
TILE_CELLS, LANES_CELLS = 4096, 784  # EGG_CV_TILE_CELLS, EGG_CV_LANES_CELLS (= EGG_CV_WAVE_CELLS: auto never takes the wave path)
RADIUS_ROW = 7  # of a batch's state rows: x, y, vx, vy, last_x, last_y, inv_mass, radius, mass_t


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _placed(egg, batches):
    """a handle with one batch per entry (ids 1, 2, ... in the list's order) whose particles have the given (x, y, radius)"""
    h = egg.SimulationHandler()
    for key, (white, yolk) in enumerate(batches, 1):
        info, ws, ys = _template(egg, len(white), len(yolk))
        ws, ys = ws.copy(), ys.copy()
        for state, spots in ((ws, white), (ys, yolk)):
            assert state.shape == (9, len(spots))
            a = np.asarray(spots, dtype=np.float64).reshape(len(spots), 3)
            state[0] = state[4] = a[:, 0]
            state[1] = state[5] = a[:, 1]
            state[2] = state[3] = 0.0
            state[RADIUS_ROW] = a[:, 2]
        assert h.import_batch(dict(info, key=key), ws, ys) == key
    return h


def _model(h, grid, scale, types, owner=True):
    d = [[h.download(w, f) for w in (WHITE, YOLK)] for f in ("x", "y", "radius", "batch_id")]
    return cm.cover(grid, scale, d[0], d[1], d[2], d[3], types, owner)


def _as_model(c):
    return (c.cover, c.owner, c.inside, c.outside, c.dropped, c.hits, c.covered, c.covered_both, c.covered_any)


def _assert_cover(h, grid, what, scale=1.0, types="both"):
    """cover() of h on all four paths, with the owner plane, is the model's over h's own downloads; returns path -> Cover"""
    x0, y0, cell, nx, ny = grid
    want = _model(h, grid, scale, types)
    got = {path: h.cover((x0, y0), cell, (nx, ny), scale, types, True, path) for path in PATHS}
    for path, c in got.items():
        print("%s / %s: inside %s outside %s dropped %s hits %s covered %s both %d any %d | units lanes %d wave %d direct %d" % (
            what, path, c.inside, c.outside, c.dropped, c.hits, c.covered, c.covered_both, c.covered_any, c.units_lanes, c.units_wave, c.units_direct))
        assert c.cover.dtype == np.int32 and c.cover.shape == (2, ny, nx) and c.owner.dtype == np.int32 and c.cell == cell, (what, path)
        assert cm.same(_as_model(c), want), (what, path)
    units = [c.units_lanes + c.units_wave + c.units_direct for c in got.values()]  # (the units that hold a disc inside)
    assert len(set(units)) == 1 and got["direct"].units_direct == units[0], (what, units)
    assert got["lanes"].units_wave == 0 and got["wave"].units_lanes == 0, what
    # a union beyond the tile is direct on every path; auto also sends a unit with a footprint above the bound there, never to the wave path
    assert got["lanes"].units_direct == got["wave"].units_direct <= got["auto"].units_direct and got["auto"].units_wave == 0, what
    for w in (0, 1):
        n = h.get_n_particles()[w] if cm.MASKS[types] >> w & 1 else 0
        assert want[2][w] + want[3][w] + want[4][w] == n, (what, w)
    plain = h.cover((x0, y0), cell, (nx, ny), scale, types)
    assert plain.owner is None and cm.same(_as_model(plain)[2:], want[2:]) and np.array_equal(plain.cover, want[0]), what
    assert plain.area() == tuple(n * (cell * cell) for n in want[6] + want[7:9]), what
    return got


# ------------------------------------------------------------------------------------------------ the hand table
@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_hand_case(egg, name):
    case = tc.CASES[name]
    h = _placed(egg, case["batches"])
    x0, y0, cell, nx, ny = case["grid"]
    for path in PATHS:
        got = h.cover((x0, y0), cell, (nx, ny), case["scale"], case["types"], True, path)
        assert cm.same(_as_model(got), tc.expected(name)), (name, path, got)
    _assert_cover(h, case["grid"], name, case["scale"], case["types"])


# ------------------------------------------------------------------------------------------------ the seams of the scan
def _line(n, x_from, x_to, slope, wobble, radius):
    t = np.arange(n, dtype=np.float64)
    x = x_from + (x_to - x_from) * t / max(n - 1, 1)
    return list(zip(x, slope * x + wobble * np.cos(t), radius * (1.0 + 0.5 * np.sin(0.37 * t))))


@pytest.mark.parametrize("n", [2, 64, 65, 1024, 1025, 2500])
def test_batch_sizes_on_every_seam(egg, n):
    """n particles per type on a line that enters and leaves the grid: lanes of a partly filled wave, the step to a second
    chunk, the unit boundary at 1,024 and three units"""
    h = _placed(egg, [(_line(n, -130.0, 130.0, 0.05, 0.125, 2.0), _line(n, -90.0, 150.0, 0.4, 0.01, 5.0))])
    c = _assert_cover(h, (-100.0, -30.0, 3.0, 65, 21), "n = %d" % n)["auto"]
    assert c.dropped == (0, 0) and (n < 64 or (0 < c.inside[0] < n and 0 < c.inside[1] < n)), c[3:]  # (the edges cut the lines)


def _cloud(n, seed, cx, cy, sx, sy, r_lo, r_hi):
    rng = np.random.default_rng(seed)
    return list(zip(rng.normal(cx, sx, n), rng.normal(cy, sy, n), rng.uniform(r_lo, r_hi, n)))


@pytest.mark.parametrize("grid", [(10.0, 10.0, 40.0, 1, 1), (0.0, 28.0, 1.5, 37, 1), (28.0, 0.0, 1.5, 1, 37), (-5.0, 25.0, 1.0, 65, 2)])
def test_grid_seams(egg, grid):
    h = _placed(egg, [(_cloud(300, 3, 30.0, 30.0, 12.0, 12.0, 0.0, 3.0), _cloud(130, 4, 30.0, 26.0, 8.0, 3.0, 0.5, 6.0))])
    c = _assert_cover(h, grid, "grid %r" % (grid,))["auto"]
    assert c.hits[0] > 0 and c.hits[1] > 0


def test_tile_seams(egg):
    """a unit whose union rectangle holds exactly EGG_CV_TILE_CELLS cells takes a tile path, one cell more goes direct"""
    grid = (0.0, 0.0, 1.0, 70, 70)
    fits = _placed(egg, [([(0.5, 0.5, 0.4), (63.5, 63.5, 0.4)], [(0.5, 0.5, 0.4), (30.5, 30.5, 0.4)])])
    got = _assert_cover(fits, grid, "union 64 x 64")
    assert 64 * 64 == TILE_CELLS and (got["auto"].units_lanes, got["auto"].units_wave, got["auto"].units_direct) == (2, 0, 0)
    assert (got["wave"].units_wave, got["lanes"].units_lanes, got["direct"].units_direct) == (2, 2, 2)
    over = _placed(egg, [([(0.5, 0.5, 0.4), (64.5, 63.5, 0.4)], [(0.5, 0.5, 0.4), (30.5, 30.5, 0.4)])])
    got = _assert_cover(over, grid, "union 65 x 64")
    for path in PATHS:  # (the white unit is direct on every path; the yolk unit follows the path)
        assert got[path].units_direct == (2 if path == "direct" else 1), path
    assert got["auto"].hits == (2, 2)


def test_footprint_seams(egg):
    """every disc exactly at the bound of the lanes path (a 28 x 28 rectangle: 784 cells) and one disc one row above it (28 x 29):
    that unit goes direct, or to the wave path where it is forced"""
    grid = (0.0, 0.0, 1.0, 60, 60)
    at = [(14.0 + 28.0 * (k % 2), 14.0 + 28.0 * (k // 2 % 2), 13.9) for k in range(64)]  # fxl = .1, fxh = 27.9 in its 28 cells; union 56 x 56
    got = _assert_cover(_placed(egg, [(at, at[:3])]), grid, "every footprint 784 cells")
    assert LANES_CELLS == 28 * 28 and (got["auto"].units_lanes, got["auto"].units_wave, got["auto"].units_direct) == (2, 0, 0)
    assert (got["wave"].units_wave, got["direct"].units_direct) == (2, 2)
    above = at[:40] + [(14.0, 14.2, 13.9)] + at[41:]  # fyl = .3, fyh = 28.1: 29 rows, 812 cells
    got = _assert_cover(_placed(egg, [(above, at[:3])]), grid, "one footprint of 812 cells")
    assert (got["auto"].units_lanes, got["auto"].units_wave, got["auto"].units_direct) == (1, 0, 1)
    assert (got["lanes"].units_lanes, got["wave"].units_wave) == (2, 2)


def test_mixed_radii_in_one_wave(egg):
    rng = np.random.default_rng(8)
    spots = list(zip(rng.uniform(0.0, 60.0, 64), rng.uniform(0.0, 60.0, 64), rng.choice([0.0, 0.3, 1.0, 2.5, 7.0, 20.0], 64)))
    h = _placed(egg, [(spots, spots[:20])])
    got = _assert_cover(h, (0.0, 0.0, 1.0, 60, 60), "mixed radii")
    assert got["auto"].units_direct >= 1 and got["wave"].units_wave >= 1  # (the discs of 20 cells in radius lie above the bound)
    _assert_cover(h, (0.0, 0.0, 0.25, 240, 240), "mixed radii, fine cells: some discs beyond the span")


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
    before = _assert_cover(h, EGG_GRID, order + ": before a step")["auto"]
    for _ in range(5):
        assert h.update(H60, H60, S, C3) == 1
    after = _assert_cover(h, EGG_GRID, order + ": after 5 steps")["auto"]
    assert not np.array_equal(before.cover, after.cover) and after.covered_both > 0
    drawn = _assert_cover(h, EGG_GRID, order + ": the discs as they are drawn", scale=12.0)["auto"]
    assert drawn.covered_any > after.covered_any and drawn.dropped == (0, 0) and set(np.unique(drawn.owner)) == {-1, 1, 2, 3, 4}
    _assert_cover(h, (250.0, 250.0, 1.0, 100, 60), order + ": cells finer than a particle, half the scene")


def test_owner_follows_the_batches(egg):
    """the lowest id wins; the middle batch is removed, then a batch is added"""
    h = egg.SimulationHandler()
    ids = [h.add(300.0 + 25.0 * k, 300.0) for k in range(3)]
    grid = (220.0, 220.0, 2.0, 90, 80)
    first = _assert_cover(h, grid, "three overlapping eggs", scale=3.0)["auto"]
    assert set(np.unique(first.owner)) == {-1} | set(ids) and first.covered_any < first.covered[0] + first.covered[1]
    both = (first.cover[0] > 1) & (first.owner[0] == ids[0])
    assert both.any()  # (cells under several discs, owned by the oldest batch)
    h.remove(ids[1])
    second = _assert_cover(h, grid, "the middle egg removed", scale=3.0)["auto"]
    assert set(np.unique(second.owner)) == {-1, ids[0], ids[2]}
    new = h.add(330.0, 310.0)
    third = _assert_cover(h, grid, "an egg added", scale=3.0)["auto"]
    assert new not in ids and set(np.unique(third.owner)) == {-1, ids[0], ids[2], new}


def test_owner_by_key(egg):
    """EGG_COVER_OWNER_KEYS: the owner plane holds the smallest KEY -- what a group and sharded ranks merge by -- where the ids
    of a handle that got its batches in another order would name another batch"""
    from egg_fluid_simulation_amd import _ffi
    h = egg.SimulationHandler()
    spots = {30: [(3.5, 1.5, 1.5)], 20: [(2.5, 1.5, 1.5)], 10: [(4.5, 1.5, 1.5)]}
    for key in (30, 20, 10):  # ids 1, 2, 3: the reverse of the keys' order
        info, ws, ys = _template(egg, 1, 1)
        ws, ys = ws.copy(), ys.copy()
        for state in (ws, ys):
            state[0] = state[4] = spots[key][0][0]
            state[1] = state[5] = spots[key][0][1]
            state[2] = state[3] = 0.0
            state[RADIUS_ROW] = spots[key][0][2]
        assert h.import_batch(dict(info, key=key), ws, ys) == {30: 1, 20: 2, 10: 3}[key]
    grid = (0.0, 0.0, 1.0, 8, 3)
    by_id = _assert_cover(h, grid, "three batches, ids against keys")["auto"]
    d = [[h.download(w, f) for w in (WHITE, YOLK)] for f in ("x", "y", "radius", "batch_id")]
    keys = [np.array([{1: 30, 2: 20, 3: 10}[int(i)] for i in d[3][w]]) for w in (WHITE, YOLK)]
    want = cm.cover(grid, 1.0, d[0], d[1], d[2], keys)
    for path in range(4):
        cover, owner = np.zeros((2, 3, 8), dtype=np.int32), np.zeros((2, 3, 8), dtype=np.int32)
        spec, totals = _ffi.EggCoverSpec(0.0, 0.0, 1.0, 1.0, 8, 3, 3, path | _ffi.COVER_OWNER_KEYS), _ffi.EggCoverTotals()
        assert h._lib.egg_cover(h._h, C.byref(spec), C.byref(_ffi.EggCoverPlanes(cover.ctypes.data, owner.ctypes.data)), C.byref(totals)) == 0
        assert np.array_equal(cover, want[0]) and np.array_equal(owner, want[1]) and tuple(totals.hits) == want[5], path
    assert by_id.owner[0][1][3] == 1 and want[1][0][1][3] == 10 and set(np.unique(want[1])) == {-1, 10, 20}  # (the youngest lies under the two others)


@pytest.mark.parametrize("types", ["white", "yolk", "both"])
def test_types(egg, types):
    h = egg.SimulationHandler()
    for x, y in EGGS[:2]:
        h.add(x, y)
    c = _assert_cover(h, EGG_GRID, "types = " + types, 2.0, types)["auto"]
    for w, name in ((WHITE, "white"), (YOLK, "yolk")):
        if types not in (name, "both"):
            assert not c.cover[w].any() and (c.owner[w] == -1).all() and c.inside[w] + c.outside[w] + c.dropped[w] == 0
        else:
            assert c.covered[w] > 0


# ------------------------------------------------------------------------------------------------ cover_to
def test_cover_to_fills_torch_tensors(egg):
    import torch
    from egg_fluid_simulation_amd import _ffi
    h = _placed(egg, [(_cloud(1500, 11, 30.0, 30.0, 12.0, 12.0, 0.2, 3.0), _cloud(700, 12, 35.0, 25.0, 6.0, 6.0, 0.2, 5.0))])
    origin, cell, shape = (0.0, 0.0), 1.5, (37, 41)
    want = h.cover(origin, cell, shape, owner=True)
    assert cm.same(_as_model(want), _model(h, origin + (cell,) + shape, 1.0, "both"))
    dev = torch.device("cuda:0")
    cover = torch.full((2, 41, 37), 123, dtype=torch.int32, device=dev)  # (stale contents: the call presets them itself)
    owner = torch.full((2, 41, 37), 9, dtype=torch.int32, device=dev)
    for path in PATHS:
        t = h.cover_to(origin, cell, shape, cover, owner, path=path)
        assert np.array_equal(cover.cpu().numpy(), want.cover) and np.array_equal(owner.cpu().numpy(), want.owner), path
        assert tuple(t[:8]) == tuple(want[2:10]), path
    cover.fill_(55)
    t = h.cover_to(origin, cell, shape, cover.data_ptr(), types="yolk")  # (an address; no owner; one type)
    assert np.array_equal(cover.cpu().numpy()[1], want.cover[1]) and not cover[0].any() and t.inside == (0, want.inside[1])
    # an empty handle fills cover with 0 and owner with -1 on the device and launches nothing
    cover.fill_(55)
    empty = egg.SimulationHandler()
    t = empty.cover_to(origin, cell, shape, cover, owner)
    assert not cover.any() and bool((owner == -1).all()) and tuple(t[1:]) == ((0, 0),) * 5 + (0, 0, 0, 0, 0) and empty.stats()["kernel_launches"] == 0
    # refused with the tensors untouched: a misaligned, a host-side and a too-short pointer, a tensor of another size or type
    cover.fill_(55)
    owner.fill_(-5)
    raw = torch.zeros(2 * 41 * 37 * 4 + 16, dtype=torch.uint8, device=dev)
    big = torch.zeros(20 << 20, dtype=torch.uint8, device=dev)  # (an allocation of its own: its last KiB is too short for a plane)
    short = big.data_ptr() + big.numel() - 1024
    with pytest.raises(egg.EggError, match="cover is not aligned to 4 bytes"):
        h.cover_to(origin, cell, shape, raw.data_ptr() + 2)
    with pytest.raises(egg.EggError, match="owner is not aligned to 4 bytes"):
        h.cover_to(origin, cell, shape, cover, raw.data_ptr() + 1)
    with pytest.raises(egg.EggError, match="cover must hold 2 x 41 x 37 elements"):
        h.cover_to(origin, cell, shape, cover[:1], owner)
    with pytest.raises(egg.EggError, match="owner must hold int32"):
        h.cover_to(origin, cell, shape, cover, raw)
    spec = _ffi.EggCoverSpec(0.0, 0.0, cell, 1.0, 37, 41, 3, 0)
    totals = _ffi.EggCoverTotals()
    totals.units_wave = 55
    host = np.full((2, 41, 37), 3, dtype=np.int32)
    for planes, text in ((_ffi.EggCoverPlanes(raw.data_ptr() + 1, None), "cover is not aligned to 4 bytes"),
                         (_ffi.EggCoverPlanes(host.ctypes.data, None), "cover is not 12136 bytes of memory of device 0"),
                         (_ffi.EggCoverPlanes(cover.data_ptr(), host.ctypes.data), "owner is not 12136 bytes of memory of device 0"),
                         (_ffi.EggCoverPlanes(short, None), "cover is not 12136 bytes of memory of device 0"),
                         (_ffi.EggCoverPlanes(cover.data_ptr(), short), "owner is not 12136 bytes of memory of device 0")):
        assert h._lib.egg_cover_to(h._h, C.byref(spec), C.byref(planes), C.byref(totals)) == _ffi.EGG_ERR_INVALID_ARGUMENT, text
        assert text in h._lib.egg_last_error(h._h).decode(), (text, h._lib.egg_last_error(h._h))
    assert bool((cover == 55).all()) and bool((owner == -5).all()) and (host == 3).all() and not big.any()
    assert not raw.any() and totals.units_wave == 55


def test_refusals_leave_the_planes_alone(egg):
    from egg_fluid_simulation_amd import _ffi
    h = egg.SimulationHandler()
    h.add(300.0, 300.0)
    cover, owner = np.full((2, 4, 4), 77, dtype=np.int32), np.full((2, 4, 4), 78, dtype=np.int32)
    planes, totals = _ffi.EggCoverPlanes(cover.ctypes.data, owner.ctypes.data), _ffi.EggCoverTotals()
    good = dict(x0=290.0, y0=290.0, cell=4.0, scale=1.0, nx=4, ny=4, type_mask=3, path=0)
    for bad, text in ((dict(nx=0), "nx, ny = 0, 4"), (dict(nx=1 << 11, ny=1 << 10), "nx * ny at most 1048576"), (dict(cell=0.0), "cell = 0"),
                      (dict(cell=float("nan")), "cell = nan"), (dict(x0=INF), "is not finite"), (dict(scale=0.0), "scale = 0"),
                      (dict(scale=INF), "scale = inf"), (dict(type_mask=0), "type_mask 0"), (dict(type_mask=4), "type_mask 4"),
                      (dict(path=4), "unknown path 4"), (dict(path=-1), "unknown path -1"), (dict(x0=4.0 * 2.0 ** 20 - 15.0), "does not resolve its coordinates"),
                      (dict(y0=-4.0 * 2.0 ** 20 - 1.0), "does not resolve its coordinates")):
        spec = _ffi.EggCoverSpec(**dict(good, **bad))
        assert h._lib.egg_cover(h._h, C.byref(spec), C.byref(planes), C.byref(totals)) == _ffi.EGG_ERR_INVALID_ARGUMENT, text
        assert text in h._lib.egg_last_error(h._h).decode(), (text, h._lib.egg_last_error(h._h))
    assert h._lib.egg_cover(h._h, C.byref(_ffi.EggCoverSpec(**good)), C.byref(_ffi.EggCoverPlanes(None, owner.ctypes.data)), C.byref(totals)) == _ffi.EGG_ERR_INVALID_ARGUMENT
    assert h._lib.egg_cover(h._h, None, C.byref(planes), C.byref(totals)) == _ffi.EGG_ERR_INVALID_ARGUMENT
    assert h._lib.egg_cover(h._h, C.byref(_ffi.EggCoverSpec(**good)), None, C.byref(totals)) == _ffi.EGG_ERR_INVALID_ARGUMENT
    assert (cover == 77).all() and (owner == 78).all() and h.stats()["kernel_launches"] == 0
    assert h._lib.egg_cover(h._h, C.byref(_ffi.EggCoverSpec(**good)), C.byref(planes), C.byref(totals)) == 0
    assert cover.sum() == totals.hits[0] + totals.hits[1] > 0 and set(np.unique(owner)) <= {-1, 1} and h.stats()["kernel_launches"] == 2
    spec = _ffi.EggCoverSpec(**dict(good, x0=4.0 * 2.0 ** 20 - 16.0))  # (the last grid that resolves its coordinates)
    assert h._lib.egg_cover(h._h, C.byref(spec), C.byref(planes), C.byref(totals)) == 0 and not cover.any()
    for bad, text in ((dict(shape=(0, 4)), "nx and ny are at least 1"), (dict(cell=0.0), "cell must be finite and above 0"), (dict(scale=-1.0), "scale must be"),
                      (dict(types="none"), "types must be"), (dict(path="fast"), "path must be")):
        with pytest.raises(egg.EggError, match=text):
            h.cover(**dict(dict(origin=(0.0, 0.0), cell=4.0, shape=(4, 4)), **bad))


def test_a_step_in_flight(egg):
    h = egg.SimulationHandler()
    for x, y in EGGS[:2]:
        h.add(x, y)
    held = _assert_cover(h, EGG_GRID, "before")["auto"]
    h.step_begin(H60, S, C3)
    with pytest.raises(egg.EggError, match="egg_cover: a step is in flight"):
        h.cover(EGG_GRID[:2], EGG_GRID[2], EGG_GRID[3:])
    import torch
    cover = torch.full((2, 64, 64), 7, dtype=torch.int32, device="cuda:0")
    with pytest.raises(egg.EggError, match="egg_cover_to: a step is in flight"):
        h.cover_to(EGG_GRID[:2], EGG_GRID[2], EGG_GRID[3:], cover)
    assert bool((cover == 7).all())
    h.step_end(False)
    assert cm.same(_as_model(h.cover(EGG_GRID[:2], EGG_GRID[2], EGG_GRID[3:], owner=True)), _as_model(held))
    h.step_begin(H60, S, C3)
    h.step_end(True)
    assert not cm.same(_as_model(_assert_cover(h, EGG_GRID, "after the committed step")["auto"]), _as_model(held))


def test_cover_only_observes(egg):
    """two handles stepped alike, one calling cover() between steps: equal particles in every download, and of the stats
    only kernel_launches moves, by 2 per call"""
    a, b = _relaxed_scene(egg.SimulationHandler()), _relaxed_scene(egg.SimulationHandler())
    for h in (a, b):
        for x, y in EGGS:
            h.add(x, y)
    calls = 0
    for k in range(4):
        for h in (a, b):
            assert h.update(H60, H60, S, C3) == 1
        stats = a.stats()
        a.cover(EGG_GRID[:2], EGG_GRID[2], EGG_GRID[3:], 12.0, owner=True)
        a.cover(EGG_GRID[:2], EGG_GRID[2], EGG_GRID[3:], 1.0, "white", False, "direct")
        calls += 2
        after = a.stats()
        assert after["kernel_launches"] == stats["kernel_launches"] + 4
        assert {key: v for key, v in after.items() if key != "kernel_launches"} == {key: v for key, v in stats.items() if key != "kernel_launches"}
        for w in (WHITE, YOLK):
            for f in FIELDS:
                assert np.array_equal(a.download(w, f), b.download(w, f)), (k, w, f)
    assert a.stats()["kernel_launches"] - b.stats()["kernel_launches"] == 2 * calls
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
        want = _assert_cover(h, EGG_GRID, "one handle, step %d" % (k + 1), scale=6.0)["auto"]
        for owner in (True, False):
            got = g.cover(origin, cell, shape, 6.0, owner=owner)
            assert cm.same(_as_model(got), _as_model(h.cover(origin, cell, shape, 6.0, owner=owner))), (k, owner)
        own = [b.cover(origin, cell, shape, 6.0) for b in g.handles]
        assert all(c.inside[WHITE] > 0 for c in own) and sum(c.inside[WHITE] for c in own) == want.inside[WHITE]  # (every handle holds a part)
        assert sum(c.covered[WHITE] for c in own) > want.covered[WHITE]  # (covered is not additive: the eggs overlap across the cut)
        assert cm.same(_as_model(g.cover(origin, cell, shape, 6.0, "yolk", True, "direct")), _as_model(h.cover(origin, cell, shape, 6.0, "yolk", True)))
    g.remove(ids[1])
    h.remove(ids[1])
    far = g.add(*FAR_EGG)
    assert h.add(*FAR_EGG) == far
    got, want = g.cover(origin, cell, shape, 6.0, owner=True), _assert_cover(h, EGG_GRID, "one handle with the far egg", scale=6.0)["auto"]
    assert cm.same(_as_model(got), _as_model(want)) and min(want.outside) > 0 and set(np.unique(got.owner)) == {-1, ids[0], ids[2], ids[3]}
    with pytest.raises(egg.EggError, match="cell"):
        g.cover(origin, -1.0, shape)
    assert not hasattr(g, "cover_to")


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
            steps.append(dict(owned=tuple(sh.cover(origin, cell, shape, 6.0, owner=True)), plain=tuple(sh.cover(origin, cell, shape, 6.0, "white")),
                              own=sh.local.cover(origin, cell, shape, 6.0).inside))
        sh.add(FAR_EGG[0], FAR_EGG[1], 50, 15)
        last = tuple(sh.cover(origin, cell, shape, 6.0, owner=True, path="direct"))
        q.put((rank, "ok", dict(steps=steps, last=last, has_to=hasattr(sh, "cover_to"))))
    except Exception:
        import traceback
        q.put((rank, "error: " + traceback.format_exc(), None))
    finally:
        dist.destroy_process_group()


def _cut(answer):
    """a Cover as a tuple -> the part the model names (without cell and the units)"""
    return answer[:2] + answer[3:10]


def test_sharded_two_ranks_equal_one_handle(egg):
    """two ranks on one GPU (three processes with the GPU open), the cut through the eggs: the merged planes are one
    handle's on both ranks, and each rank's own are a part of them"""
    res = _spawn(2)
    h = _relaxed_scene(egg.SimulationHandler())
    for x, y in EGGS:
        h.add(x, y, 50, 15)
    origin, cell, shape = EGG_GRID[:2], EGG_GRID[2], EGG_GRID[3:]
    for k in range(3):
        h.step(H60, S, C3)
        want = _assert_cover(h, EGG_GRID, "one handle, step %d" % (k + 1), scale=6.0)["auto"]
        plain = h.cover(origin, cell, shape, 6.0, "white")
        for r in (0, 1):
            got = res[r]["steps"][k]
            assert cm.same(_cut(got["owned"]), _as_model(want)) and cm.same(_cut(got["plain"]), _as_model(plain)), (r, k)
        own = [res[r]["steps"][k]["own"] for r in (0, 1)]
        assert all(o[WHITE] > 0 for o in own) and tuple(a + b for a, b in zip(*own)) == want.inside, own
    h.add(FAR_EGG[0], FAR_EGG[1], 50, 15)
    want = h.cover(origin, cell, shape, 6.0, owner=True)
    for r in (0, 1):
        assert cm.same(_cut(res[r]["last"]), _as_model(want)) and not res[r]["has_to"], r


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
