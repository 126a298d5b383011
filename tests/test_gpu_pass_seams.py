"""The seams of a packed collision pass (csrc/eggsim_packed.hip): the first list pass of every sub-step does the
per-particle work in front of it itself (egg_pk_lists_first_kernel: gather, pre-solve, follow, the atoms' claim flags,
the other status block; egg_pk_lists_stale_mid_kernel: post-solve, pre-solve, follow), and the list kernels run at a
register budget that lets eight waves share a SIMD.

Every scene is stepped by the packed pipeline as it runs by default and, beside it, by a second handle under
EGGSIM_TUNE = 384 (bit 7: the separate begin / mid launches and the host's memset; bit 8 was meant for the fused pass's
entry and exit code, whose rework did not pay and is not in the library, so it changes nothing).  Both are compared bit for
bit with the sequential CPU oracle after every step -- positions, velocities, the pair-solve count -- and with each other
in the deepest level they saw."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
N_W = 157  # white particles of a default batch


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _pair(egg, monkeypatch, walk, options=(), **kw):
    """the scene's two device handles: default seams, and both old paths (EGGSIM_TUNE is read when a handle is created)"""
    from egg_fluid_simulation_amd import _ffi
    hs = []
    for tune in ("0", "384"):
        monkeypatch.setenv("EGGSIM_TUNE", tune)
        h = egg.SimulationHandler(**kw)
        h.set_option(_ffi.OPT_PACKED, 1)
        h.set_option(_ffi.OPT_LEVEL_WALK, walk)
        for k, v in options:
            h.set_option(k, v)
        hs.append(h)
    monkeypatch.setenv("EGGSIM_TUNE", "0")
    return hs


def _same(hs, o, tag):
    for h in hs:
        for w in (WHITE, YOLK):
            for f in ("x", "y", "vx", "vy"):
                a, b = h.download(w, f), o.field(w, f)
                assert a.shape == b.shape and np.array_equal(a, b), (tag, w, f)
        assert h.stats()["pair_solves"] == o.total_visited, tag
    assert hs[0].stats()["max_levels"] == hs[1].stats()["max_levels"], tag


def _add(hs, o, x, y, wr=50, yr=15):
    ids = {h.add(x, y, wr, yr) for h in hs} | {o.add(x, y, wr, yr)}
    assert len(ids) == 1
    return ids.pop()


def _target(hs, o, i, x, y):
    for s in hs + [o]:
        s.set_target_position(i, x, y)


def _step(hs, o, S, C):
    for s in hs + [o]:
        s.step(1 / 60, S, C)


def _dense(egg, oracle_mod, monkeypatch, S, C, options=()):
    """three sites of four coincident batches: 628-particle tiles on 512 threads (a thread owns two particles), groups of
    two tiles and of one tile; batch 0's target moves 2 px per step"""
    from egg_fluid_simulation_amd import _ffi
    hs, o = _pair(egg, monkeypatch, 2, options), oracle_mod.Oracle()
    ids = [_add(hs, o, 300.0 + 260.0 * site, 300.0) for site in range(3) for _ in range(4)]
    for step in range(6):
        _target(hs, o, ids[0], 300.0 + 2.0 * step, 300.0)
        _step(hs, o, S, C)
        _same(hs, o, (S, C, step))
    for h in hs:
        st = h.stats()
        assert st["pk_variants"][WHITE] & _ffi.PK_VARIANT_PASS_FUSED and st["max_tile_particles"][WHITE] == 4 * N_W, st


@pytest.mark.parametrize("S,C", [(1, 1), (2, 1), (2, 3), (3, 2)])
def test_dense_islands(egg, oracle_mod, monkeypatch, S, C):
    _dense(egg, oracle_mod, monkeypatch, S, C)


def test_four_islands_per_executor(egg, oracle_mod, monkeypatch):
    from egg_fluid_simulation_amd import _ffi
    _dense(egg, oracle_mod, monkeypatch, 2, 3, ((_ffi.OPT_GROUP_PARTICLES, 2560),))


@pytest.mark.parametrize("walk", [1, 2])
@pytest.mark.parametrize("S,C", [(1, 3), (2, 3)])
def test_sparse_tiles(egg, oracle_mod, monkeypatch, S, C, walk):
    """14 separate batches, several tiles per group; the targets move every step, so the tiles are formed, planned and
    their records uploaded in front of the folded first pass of every step"""
    hs, o = _pair(egg, monkeypatch, walk), oracle_mod.Oracle()
    n = 14
    xs = 100.0 + 95.0 * (np.arange(n) % 5)
    ys = 100.0 + 95.0 * (np.arange(n) // 5)
    ids = [_add(hs, o, float(a), float(b)) for a, b in zip(xs, ys)]
    for k in range(6):
        dx, dy = 30.0 * np.cos(0.4 * k), 30.0 * np.sin(0.4 * k)
        for i, a, b in zip(ids, xs, ys):
            _target(hs, o, i, float(a + dx), float(b + dy))
        _step(hs, o, S, C)
        _same(hs, o, (S, C, walk, k))
    from egg_fluid_simulation_amd import _ffi
    want = {1: _ffi.PK_VARIANT_LEVELS_INORDER, 2: _ffi.PK_VARIANT_LEVELS_OOO}[walk]
    for h in hs:
        st = h.stats()
        assert st["packed"][WHITE] >= 1 and st["retiles"] > 2, st
        assert st["pk_variants"][WHITE] & (_ffi.PK_VARIANT_LEVELS_INORDER | _ffi.PK_VARIANT_LEVELS_OOO) == want, st


@pytest.mark.parametrize("walk", [1, 2])
def test_tiles_under_one_wave(egg, oracle_mod, monkeypatch, walk):
    """small batches (35 / 9: fewer white particles than a wave has lanes) beside default ones"""
    hs, o = _pair(egg, monkeypatch, walk), oracle_mod.Oracle()
    ids = []
    for k in range(8):
        x, y = 100.0 + 170.0 * (k % 4), 100.0 + 170.0 * (k // 4)
        ids.append(_add(hs, o, x, y, 35, 9) if k % 2 else _add(hs, o, x, y))
    for step in range(6):
        _target(hs, o, ids[1], 270.0 + 3.0 * step, 100.0)
        _step(hs, o, 2, 3)
        _same(hs, o, (walk, step))
    for h in hs:
        assert h.stats()["packed"][WHITE] >= 1
    assert hs[0].download(WHITE, "x").size < 8 * N_W


@pytest.mark.parametrize("walk", [1, 2])
def test_slow_pairs(egg, oracle_mod, monkeypatch, walk):
    """every inverse mass in [eps / 2, eps) passes the tile-wide fast-path test; masses below eps / 2 in one batch fail it,
    so the folded first pass decides `all_fast` false from the (inverse mass, radius) it has just gathered"""
    from egg_fluid_simulation_amd.default_config import default_configs
    tweak = dict(min_mass=1.0 / 0.7e-8, max_mass=1.0 / 0.3e-8)  # inverse masses 0.3e-8 .. 0.7e-8: both sides of eps / 2
    w, y = default_configs()
    w.update(tweak)
    y.update(tweak)
    hs = _pair(egg, monkeypatch, walk, white_config=w, yolk_config=y)
    o = oracle_mod.Oracle()
    o.set_config(WHITE, dict(oracle_mod.DEFAULT_WHITE, **tweak))
    o.set_config(YOLK, dict(oracle_mod.DEFAULT_YOLK, **tweak))
    for cx, cy in [(300.0, 300.0)] * 4 + [(700.0, 300.0), (700.0, 480.0)]:
        _add(hs, o, cx, cy)
    for step in range(4):
        _step(hs, o, 2, 3)
        _same(hs, o, (walk, step))
    inv = o.field(WHITE, "inv_mass")
    assert (inv < 0.5e-8).any() and (inv >= 0.5e-8).any() and (inv < 1e-8).all()
    for h in hs:
        assert h.stats()["packed"][WHITE] >= 1 and h.stats()["max_tile_particles"][WHITE] == 4 * N_W


def test_inverse_masses_between_half_eps_and_eps(egg, oracle_mod, monkeypatch):
    """the tweak of test_gpu_round2's case of this name as it stands: `all_fast` holds, no pair fails the mass guard"""
    from egg_fluid_simulation_amd.default_config import default_configs
    tweak = dict(min_mass=1.0 / 0.7e-8, max_mass=1.0 / 0.6e-8)
    w, y = default_configs()
    w.update(tweak)
    y.update(tweak)
    hs = _pair(egg, monkeypatch, 2, white_config=w, yolk_config=y)
    o = oracle_mod.Oracle()
    o.set_config(WHITE, dict(oracle_mod.DEFAULT_WHITE, **tweak))
    o.set_config(YOLK, dict(oracle_mod.DEFAULT_YOLK, **tweak))
    for cx, cy in [(300.0, 300.0)] * 4 + [(700.0, 300.0), (700.0, 480.0)]:
        _add(hs, o, cx, cy)
    for step in range(4):
        _step(hs, o, 2, 3)
        _same(hs, o, step)
    inv = o.field(WHITE, "inv_mass")
    assert (inv >= 0.5e-8).all() and (inv < 1e-8).all()


def test_claim_failure_flags_are_cleared_by_the_next_first_pass(egg, oracle_mod, monkeypatch):
    """one batch whose target jumps 600 px at step 2 among eight resting ones: its particles leave their claims, the step
    is re-run with wider ones -- and the flags of that step are gone when the next step's first pass has run, so the
    re-runs stop"""
    hs, o = _pair(egg, monkeypatch, 0), oracle_mod.Oracle()
    ids = [_add(hs, o, 100.0 + 170.0 * (k % 3), 100.0 + 170.0 * (k // 3)) for k in range(9)]
    redo = []
    for step in range(7):
        if step == 2:
            _target(hs, o, ids[4], 270.0 + 600.0, 270.0)
        before = [h.stats()["redo_steps"] for h in hs]
        _step(hs, o, 2, 3)
        _same(hs, o, step)
        redo.append([h.stats()["redo_steps"] - b for h, b in zip(hs, before)])
    for k in range(len(hs)):
        assert redo[2][k] > 0, redo        # the jump is met by a failed claim
        assert redo[6][k] == 0, redo       # ... and four steps later no step is re-run any more
    for h in hs:
        assert h.stats()["packed"][WHITE] >= 1


def test_a_second_claim_failure_widens_only_its_own_batch(egg, oracle_mod, monkeypatch):
    """What a flag left standing would do: the host reads the flags only when a launch reports a failed claim, and doubles
    the extra margin of every flagged batch.  Batch 4 fails at step 2; when the distant batch 8 fails at step 9, a
    stale flag of batch 4 would widen batch 4 again with every re-run and change how the tiles are formed from then on.
    The handle that clears the flags inside the first list pass must form the same tiles, step by step, and re-run the
    same steps as the one whose flags the host clears with a memset (EGGSIM_TUNE bit 7) -- and both match the oracle."""
    hs, o = _pair(egg, monkeypatch, 0), oracle_mod.Oracle()
    ids = [_add(hs, o, 100.0 + 170.0 * (k % 3), 100.0 + 170.0 * (k // 3)) for k in range(9)]
    redo = []
    for step in range(13):
        if step == 2:
            _target(hs, o, ids[4], 270.0 + 600.0, 270.0)
        if step == 9:
            _target(hs, o, ids[8], 440.0, 440.0 + 600.0)
        before = [h.stats()["redo_steps"] for h in hs]
        _step(hs, o, 2, 3)
        _same(hs, o, step)
        st = [h.stats() for h in hs]
        redo.append([s["redo_steps"] - b for s, b in zip(st, before)])
        print(step, redo[-1], [(s["n_tiles"], s["max_tile_particles"]) for s in st])
        assert st[0]["n_tiles"] == st[1]["n_tiles"] and st[0]["max_tile_particles"] == st[1]["max_tile_particles"], (step, st)
        assert redo[-1][0] == redo[-1][1], (step, redo)
    assert redo[2][0] > 0 and redo[9][0] > 0, redo  # both jumps are met by failed claims


def test_tiles_whose_list_pass_needs_more_than_64_kib_of_lds(egg, oracle_mod, monkeypatch, capfd):
    """Two islands of 20 touching batches each (3,140 particles per tile): the list kernels of such a class ask for more
    dynamic LDS than a kernel gets unasked, which the folded first passes must be granted like the plain ones.  The LDS
    of the class is read from the library's own EGGSIM_DEBUG line."""
    import re
    monkeypatch.setenv("EGGSIM_DEBUG", "1")
    hs, o = _pair(egg, monkeypatch, 0), oracle_mod.Oracle()
    ids = []
    for cluster in range(2):
        for k in range(20):
            ids.append(_add(hs, o, 100.0 + 95.0 * (k % 5) + 3000.0 * cluster, 100.0 + 95.0 * (k // 5)))
    for step in range(3):
        _target(hs, o, ids[0], 100.0 + 4.0 * step, 100.0)
        _step(hs, o, 2, 3)
        _same(hs, o, step)
    err = capfd.readouterr().err
    lds = [int(m) for m in re.findall(r"type 0 packed class: .*? lists: \d+ threads, \d+ staged partners, (\d+) B LDS", err)]
    print("fresh list pass LDS per white packed class:", sorted(set(lds)))
    for h in hs:
        st = h.stats()
        assert st["packed"][WHITE] >= 1 and st["n_tiles"][WHITE] == 2 and st["max_tile_particles"][WHITE] == 20 * N_W, st
    assert lds and max(lds) > 64 * 1024, lds
