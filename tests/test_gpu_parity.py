"""Parity of the device path, called through the C ABI (libeggsim.so via the Python mirror of
SimulationHandler), with the golden vectors and the CPU oracle.  Positions are compared bit for
bit: the kernel reproduces the reference's pair order exactly, so the north star's 1e-4 relative
tolerance (asserted too) is met with zero difference."""
import math

import os

import numpy as np
import pytest

from conftest import GOLDEN_CASES, circle_target, load_golden, replay_golden

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
REL_TOL = 1e-4  # BASELINE.json north_star: positions within 1e-4 relative of the CPU reference


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _dev_state(h, w):
    return np.array([h.download(w, "x"), h.download(w, "y"), h.download(w, "vx"), h.download(w, "vy")])


def _bits(a):
    """the bit patterns: np.array_equal on floats cannot tell -0.0 from +0.0"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_close(dev, ref, what):
    assert np.all(np.abs(dev - ref) <= REL_TOL * np.maximum(1.0, np.abs(ref))), what  # the stated tolerance
    assert np.array_equal(_bits(dev), _bits(ref)), what + ": not bit-exact"  # what the kernel actually achieves (the sign of a zero included)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_device_matches_golden(egg, name):
    g = load_golden(name)
    h = egg.SimulationHandler()
    seen = []

    def check(step, tag, arr):
        _assert_close(arr, g["%s_step%d" % (tag, step)], "%s step %d %s" % (name, step, tag))
        seen.append(step)

    ids = replay_golden(g, h, _dev_state, check)
    last = int(g["snap_steps"][-1])
    cen = np.array([h.get_position(i) for i in ids])
    assert np.array_equal(cen, g["centroid_step%d" % last])
    assert len(seen) == 2 * len(g["snap_steps"])
    assert h.stats()["pair_solves"] == int(g["visits"].sum())


def test_initial_state_matches_golden(egg):
    g = load_golden("cfg1_static")
    h = egg.SimulationHandler()
    h.add(400, 300, 50, 15)
    for w, key in ((WHITE, "init_white"), (YOLK, "init_yolk")):
        got = np.array([h.download(w, f) for f in ("x", "y", "mass_t", "inv_mass", "radius")])
        assert np.array_equal(got, g[key])


def _grid(n, pitch=160.0, x0=100.0):
    side = int(math.ceil(math.sqrt(n)))
    return (np.array([x0 + pitch * (k % side) for k in range(n)]), np.array([x0 + pitch * (k // side) for k in range(n)]))


def _run_both(egg, oracle_mod, xs, ys, steps, moving, configure=None):
    h = egg.SimulationHandler()
    if configure:
        configure(h)
    o = oracle_mod.Oracle()
    ids = h.add_many(xs, ys, 50, 15)
    for x, y in zip(xs, ys):
        o.add(float(x), float(y), 50, 15)
    for k in range(steps):
        if moving:
            dx, dy = circle_target((0.0, 0.0), k)
            h.set_target_positions(ids, xs + dx, ys + dy)
            for i, x, y in zip(ids, xs, ys):
                o.set_target_position(int(i), float(x + dx), float(y + dy))
        assert h.update(1 / 60) == 1
        o.update(1 / 60)
    return h, o, ids


def _assert_same_state(h, o):
    for w in (WHITE, YOLK):
        xo, yo = o.positions(w)
        _assert_close(h.download(w, "x"), xo, "x type %d" % w)
        _assert_close(h.download(w, "y"), yo, "y type %d" % w)
        _assert_close(h.download(w, "vx"), o.field(w, "vx"), "vx type %d" % w)
    assert h.stats()["pair_solves"] == o.total_visited


@pytest.mark.parametrize("S,C", [(1, 1), (1, 2), (2, 1), (3, 1), (4, 1), (5, 1), (8, 1), (3, 2), (4, 3)])
def test_substep_and_pass_variants_vs_oracle(egg, oracle_mod, S, C):
    """Every (sub-steps, collision passes) shape of the reference's clear policy (L:1905-1912): with ONE pass
    per sub-step the hash lists and `collided` are never cleared inside a step, so sub-step s sees s
    generations of cell entries.  Two scenes: a single batch (the budget cuts every yolk pass -> exact-budget
    tile, `collided` looked up in the cut lists) and nine batches moving through each other."""
    for xs, ys, moving in ((np.array([400.0]), np.array([300.0]), True), (_grid(9, pitch=120.0) + (True,))):
        h = egg.SimulationHandler()
        o = oracle_mod.Oracle()
        ids = h.add_many(xs, ys, 50, 15)
        for x, y in zip(xs, ys):
            o.add(float(x), float(y), 50, 15)
        for k in range(8):
            dx, dy = circle_target((0.0, 0.0), 2 * k)
            h.set_target_positions(ids, xs + dx, ys + dy)
            for i, x, y in zip(ids, xs, ys):
                o.set_target_position(int(i), float(x + dx), float(y + dy))
            h.step(1 / 60, S, C)
            o.step(1 / 60, S, C)
        _assert_same_state(h, o)


@pytest.mark.parametrize("moving", [False, True])
def test_config2_256_batches_vs_oracle(egg, oracle_mod, moving):
    xs, ys = _grid(256)
    h, o, ids = _run_both(egg, oracle_mod, xs, ys, 12, moving)
    _assert_same_state(h, o)
    assert h.stats()["n_tiles"][0] == 256  # non-overlapping batches stay independent tiles
    gx, gy = h.get_positions(ids)
    ref = np.array([o.get_position(int(i)) for i in ids])
    assert np.array_equal(gx, ref[:, 0]) and np.array_equal(gy, ref[:, 1])


def test_config3_coincident_batches_vs_oracle(egg, oracle_mod):
    # BASELINE config 3 layout at reduced count: every 4 consecutive batches share one centre
    sites = 24
    sx, sy = _grid(sites, pitch=400.0)
    xs, ys = np.repeat(sx, 4), np.repeat(sy, 4)
    h, o, _ = _run_both(egg, oracle_mod, xs, ys, 6, False)
    _assert_same_state(h, o)
    assert h.stats()["max_tile_particles"][0] == 4 * 157


def test_full_size_config2_properties(egg, oracle_mod):
    """Beyond BASELINE config-2 size (4096 batches, 704k particles): the sequential oracle follows
    for 2 steps and every particle must agree; then determinism (a second handler, 4096
    independently scheduled workgroups, reproduces every bit)."""
    xs, ys = _grid(4096)
    h, o, ids = _run_both(egg, oracle_mod, xs, ys, 2, False)
    _assert_same_state(h, o)
    # 4096 white islands, one workgroup each; the 15-particle yolk islands share workgroups four by four
    assert h.stats()["n_tiles"] == [4096, 1024]
    # determinism: a second handler reproduces the state bit for bit
    h2 = egg.SimulationHandler()
    h2.add_many(xs, ys, 50, 15)
    for _ in range(2):
        h2.update(1 / 60)
    for w in (WHITE, YOLK):
        assert np.array_equal(h.download(w, "x"), h2.download(w, "x"))


def test_result_is_independent_of_tiling(egg):
    """Tiles only decide which workgroup runs which particles: packing islands into shared tiles,
    wider claim margins or forcing a single tile must not change one bit."""
    from egg_fluid_simulation_amd import _ffi
    xs, ys = _grid(36)  # the forced single tile (5652 white particles) runs in the global-memory-state kernel
    ref = None
    for opts in ({}, {_ffi.OPT_TILE_TARGET_PARTICLES: 0}, {_ffi.OPT_FUSE_TYPES: 0}, {_ffi.OPT_TILE_TARGET_PARTICLES: 700}, {_ffi.OPT_CLAIM_MARGIN_CELLS: 6},
                 {_ffi.OPT_FORCE_SINGLE_TILE: 1}, {_ffi.OPT_FORCE_CELL_HASH: 1}):
        h = egg.SimulationHandler()
        for k, v in opts.items():
            h.set_option(k, v)
        ids = h.add_many(xs, ys, 50, 15)
        for k in range(8):
            dx, dy = circle_target((0.0, 0.0), 3 * k)
            h.set_target_positions(ids, xs + dx, ys + dy)
            h.update(1 / 60)
        state = [h.download(w, f) for w in (WHITE, YOLK) for f in ("x", "y", "vx", "vy")]
        if ref is None:
            ref = state
            assert h.stats()["n_tiles"][0] == 36
        else:
            assert all(np.array_equal(a, b) for a, b in zip(ref, state)), opts
        if _ffi.OPT_FORCE_CELL_HASH in opts:
            assert all(c > 0 for c in h.stats()["cell_hash"]), h.stats()["cell_hash"]


@pytest.mark.skipif(os.environ.get("EGGSIM_PACKED") == "1", reason="asserts the one-launch mode; EGGSIM_PACKED=1 forces the packed pipeline")
def test_one_launch_for_both_types_on_a_shared_chip(egg, oracle_mod):
    """300 batches: more white tiles than CUs, so the narrow kernel variants run and -- by default -- the tiles
    of both types (three launch classes here) go into ONE grid; with one launch per class on two streams the
    bits must be the same, and both must be the oracle's"""
    from egg_fluid_simulation_amd import _ffi
    xs, ys = _grid(300)
    h, o, _ = _run_both(egg, oracle_mod, xs, ys, 3, True)
    assert h.stats()["fused_launch"] == 1
    _assert_same_state(h, o)
    h2 = egg.SimulationHandler()
    h2.set_option(_ffi.OPT_FUSE_TYPES, 0)
    ids = h2.add_many(xs, ys, 50, 15)
    for k in range(3):
        dx, dy = circle_target((0.0, 0.0), k)
        h2.set_target_positions(ids, xs + dx, ys + dy)
        assert h2.update(1 / 60) == 1
    assert h2.stats()["fused_launch"] == 0
    for w in (WHITE, YOLK):
        for f in ("x", "y", "vx", "vy"):
            assert np.array_equal(h.download(w, f), h2.download(w, f)), (w, f)


def test_large_island_falls_back_to_global_memory_state(egg, oracle_mod):
    """4 x 4 batches at 95 px pitch overlap into ONE island of 2512 white particles, far beyond what
    fits in LDS.  The step kernel then keeps the tile's state in global memory; results stay exact.
    (Index limit: 32766 particles of one type in one island.)"""
    k = np.arange(16)
    xs, ys = 500.0 + 95.0 * (k % 4), 500.0 + 95.0 * (k // 4)
    h, o, _ = _run_both(egg, oracle_mod, xs, ys, 3, False)
    _assert_same_state(h, o)
    assert h.stats()["max_tile_particles"][0] == 16 * 157


def test_global_memory_state_variant_on_ordinary_tiles(egg, oracle_mod):
    """the same fallback kernel forced onto ordinary tiles (incl. the exact-budget yolk tile of a small
    handler and a moving multi-batch case) must not change a bit"""
    from egg_fluid_simulation_amd import _ffi
    xs, ys = _grid(12, pitch=140.0)  # close enough to merge now and then
    h, o, _ = _run_both(egg, oracle_mod, xs, ys, 10, True,
                        configure=lambda hh: hh.set_option(_ffi.OPT_FORCE_GLOBAL_STATE, 1))
    _assert_same_state(h, o)
    h1, o1, _ = _run_both(egg, oracle_mod, np.array([400.0]), np.array([300.0]), 10, True,
                          configure=lambda hh: hh.set_option(_ffi.OPT_FORCE_GLOBAL_STATE, 1))
    _assert_same_state(h1, o1)


def test_batches_that_merge_and_separate(egg, oracle_mod):
    """two batches driven through each other: tiles must merge while they touch and split after"""
    h = egg.SimulationHandler()
    o = oracle_mod.Oracle()
    a, b = h.add(0, 0, 50, 15), h.add(400, 0, 50, 15)
    o.add(0, 0, 50, 15), o.add(400, 0, 50, 15)
    tiles = []
    for k in range(90):
        t = min(1.0, k / 60.0)
        for s in (h, o):
            s.set_target_position(a, 400 * t, 0.0)
            s.set_target_position(b, 400 * (1 - t), 0.0)
        h.update(1 / 60)
        o.update(1 / 60)
        tiles.append(h.stats()["n_tiles"][0])
    _assert_same_state(h, o)
    assert tiles[0] == 2 and min(tiles) == 1


def test_fast_blobs_keep_their_tiles(egg, oracle_mod):
    """targets 2.6k px away: the blobs accelerate to ~300 px (38 cells) per step.  Claims are sized per
    side from the reported last sub-step travel run through the solver's own recurrence, so every
    step validates at the first attempt; batches whose swept claims reach each other share a tile."""
    xs, ys = _grid(16, pitch=500.0)
    h = egg.SimulationHandler()
    o = oracle_mod.Oracle()
    ids = h.add_many(xs, ys, 50, 15)
    for x, y in zip(xs, ys):
        o.add(float(x), float(y), 50, 15)
    h.set_target_positions(ids, xs + 2500.0, ys + 900.0)
    for i, x, y in zip(ids, xs, ys):
        o.set_target_position(int(i), float(x + 2500.0), float(y + 900.0))
    tiles = []
    for _ in range(15):
        h.update(1 / 60)
        o.update(1 / 60)
        tiles.append(h.stats()["n_tiles"][0])
    _assert_same_state(h, o)
    moved = h.get_positions(ids)[0] - xs
    assert moved.min() > 400  # they really did fly
    assert h.stats()["redo_steps"] <= 2  # predicted, not discovered by failing
    assert tiles[0] == 16 and min(tiles) >= 4  # at worst the 4 batches of a row (500 px apart) share a tile


def test_hand_expanded_division_is_bit_identical_to_operator(egg):
    """the projection's VCC-free division must equal `/` for every operand pair in its window"""
    h = egg.SimulationHandler()
    for seed in (1, 2, 3):
        assert h.selftest_arith(1 << 26, seed) == 0  # 3 x 67M random operand pairs


def test_sqrt_and_division_are_correctly_rounded_on_device(egg, oracle_mod):
    """the parity argument needs IEEE sqrt and division in the kernel; a follow-only run exercises
    exactly one sqrt, two normalising divisions and one lambda division per particle"""
    cfg = dict(oracle_mod.DEFAULT_WHITE, collision_overlap_factor=0.0)  # nothing ever in collision range
    from egg_fluid_simulation_amd.default_config import default_configs
    w, y = default_configs()
    w["collision_overlap_factor"] = 0.0
    y["collision_overlap_factor"] = 0.0
    h = egg.SimulationHandler(w, y)
    o = oracle_mod.Oracle(cfg, dict(oracle_mod.DEFAULT_YOLK, collision_overlap_factor=0.0))
    rng = np.random.RandomState(7)
    # well separated batches (pitch 2000 px) with irrational-ish offsets, each pulled ~300 px
    gx, gy = _grid(40, pitch=2000.0, x0=-7000.0)
    xs, ys = gx + rng.uniform(-50, 50, 40), gy + rng.uniform(-50, 50, 40)
    ids = h.add_many(xs, ys, 50, 15)
    for x, yy in zip(xs, ys):
        o.add(float(x), float(yy), 50, 15)
    tx, ty = xs + rng.uniform(-300, 300, 40), ys + rng.uniform(-300, 300, 40)
    h.set_target_positions(ids, tx, ty)
    for i, a, b in zip(ids, tx, ty):
        o.set_target_position(int(i), float(a), float(b))
    for _ in range(5):
        h.update(1 / 60)
        o.update(1 / 60)
    _assert_same_state(h, o)
