"""The LDS hash table that keys a tile's cells when its claim box is too large for a dense grid (retile() in
csrc/eggsim_host_tiling.hip; DESIGN.md section 2.1, "Cells"): `atomicCAS` insert with linear probing, cell_meta() lookups,
neighbour keys by integer arithmetic on x << 16 | y, one key table per hash generation.  The fused step kernels, the packed
pipeline's list kernels and the stale-pass rules all branch on it.  Exact-budget tiles always take that branch (they claim
64 cells around their particles), the white tiles of compact scenes never do.

Two scenes reach it by themselves -- separated default eggs whose yolk budget binds (exact-budget mode puts every yolk
particle into ONE tile that spans the scene) and a wide add --; everything else forces it with the test hook
EGG_OPT_FORCE_CELL_HASH.  Every comparison is bit for bit against the CPU oracle or the goldens, and every test that is
about the hash table asserts through stats()["cell_hash"] that it ran."""
import warnings

import numpy as np
import pytest

from conftest import GOLDEN_CASES, circle_target, load_golden, replay_golden

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
STATE = ("x", "y", "vx", "vy")


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _handler(egg, white=None, yolk=None, hook=True, **options):
    """a handler with the hook set (and further options by their _ffi name without the OPT_ prefix)"""
    from egg_fluid_simulation_amd import _ffi
    h = egg.SimulationHandler(white, yolk)
    if hook:
        h.set_option(_ffi.OPT_FORCE_CELL_HASH, 1)
    for name, value in options.items():
        h.set_option(getattr(_ffi, "OPT_" + name), value)
    return h


def _bits(a):
    """the bit patterns: np.array_equal on floats cannot tell -0.0 from +0.0"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(h, o, tag):
    for w in (WHITE, YOLK):
        for f in STATE:
            a, b = h.download(w, f), o.field(w, f)
            assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), (tag, w, f)
    assert h.stats()["pair_solves"] == o.total_visited, tag


def _hashed(h, types=(WHITE, YOLK)):
    """the hash table keyed the cells of every class of `types` that the most recent step launched"""
    st = h.stats()
    assert all(st["cell_hash"][w] > 0 for w in types), st["cell_hash"]
    return st


def _oracle_box(o, w):
    """cells of the dense grid over the type's particles: what retile() compares with its limit (claims come on top)"""
    cx, cy = o.field(w, "cell_x"), o.field(w, "cell_y")
    return int((cx.max() - cx.min() + 4) * (cy.max() - cy.min() + 4))


# ------------------------------------------------------------------------------------------------ (a) no hook: ordinary scenes

SEPARATED_EGGS = {2: [(0.0, 0.0), (1200.0, 900.0)],
                  3: [(0.0, 0.0), (1200.0, 900.0), (-400.0, 700.0)],
                  4: [(0.0, 0.0), (700.0, 500.0), (-400.0, 700.0), (900.0, -300.0)]}


@pytest.mark.parametrize("n_eggs", sorted(SEPARATED_EGGS))
def test_separated_default_eggs_run_on_the_hash_table(egg, oracle_mod, n_eggs):
    """A few default eggs spread over a screen, nothing forced: 15 n yolk particles make 0.05 N^2 = 45 / 101.25 / 180 pairs
    per pass, the first steps visit more, so the yolk type is re-run in exact-budget mode -- ONE tile whose claim box spans
    the scene (9k-12k cells against the dense grid's 2,048).  The hash table then runs together with the budget cut and
    the stale pass's lookup of `collided` in the cut lists.  (The oracle cuts 30, 11 and 8 yolk passes in these ten steps;
    with three and four eggs only in steps 1 and 2, and the device leaves exact-budget mode after eight uncut steps --
    i.e. AFTER step 10: every step here runs in it.)"""
    centers = SEPARATED_EGGS[n_eggs]
    h, o = _handler(egg, hook=False), oracle_mod.Oracle()
    for x, y in centers:
        assert h.add(x, y, 50, 15) == o.add(x, y, 50, 15)
    cut_passes = 0
    for s in range(10):
        for i, (x, y) in enumerate(centers):
            h.set_target_position(i + 1, x + 3.0 * s, y - 2.0 * s)
            o.set_target_position(i + 1, x + 3.0 * s, y - 2.0 * s)
        h.step(1 / 60, 2, 3)
        o.step(1 / 60, 2, 3)
        _same(h, o, (n_eggs, s))
        cut_now = sum(p["cut"] for p in o.pass_stats() if p["which"] == YOLK)
        assert not any(p["cut"] for p in o.pass_stats() if p["which"] == WHITE)
        cut_passes += cut_now
        st = h.stats()
        print("eggs %d step %d: oracle cut %d yolk passes, yolk box %d cells; device single_tile %s cell_hash %s" %
              (n_eggs, s + 1, cut_now, _oracle_box(o, YOLK), st["single_tile"], st["cell_hash"]))
        assert _oracle_box(o, YOLK) > 2048  # too large for the dense grid whatever the claims add
        if s == 0 or cut_now:
            assert cut_now and st["single_tile"][YOLK] == 1, (s, st["single_tile"])
        assert st["cell_hash"][YOLK] > 0 and st["cell_hash"][WHITE] == 0, (s, st["cell_hash"])
    assert cut_passes == {2: 30, 3: 11, 4: 8}[n_eggs]


# ------------------------------------------------------------------------------------------------ (b) no hook: a wide add

def test_wide_add_goes_from_hash_table_to_grid(egg, oracle_mod):
    """157 white particles over a disc of radius 300: 5,256 cells at step 1, below the grid's 2,048 only after step 4, so the
    first steps run on the hash table and a later one is the first on the dense grid -- every step is compared.  The
    length of the run comes from the oracle: its white box (dcx + 4)(dcy + 4) has been below 512 cells for two steps
    running at step 11 (462 cells at step 10, 324 at step 11), plus four steps, 15 in all.  The four are there because
    the device's CLAIMS are wider than that box while the particles fall inwards at up to 2,300 px/s (claims are padded by
    the predicted travel): measured on an MI355X the tile stays on the hash table up to and including step 12 (box 256
    cells) and step 13 is the first on the grid.  (The yolk goes into exact-budget mode at step 8 and is on the hash
    table from then on, as every exact-budget tile is: see test_option_round_trip_and_counter.)"""
    h, o = _handler(egg, hook=False), oracle_mod.Oracle()
    assert h.add(100.0, 100.0, 300.0, 150.0, None, None, 157, 60) == o.add(100.0, 100.0, 300.0, 150.0, 157, 60)
    used, small, rule_step = [], 0, None
    while rule_step is None or len(used) < rule_step + 4:
        assert len(used) < 40
        h.step(1 / 60, 2, 3)
        o.step(1 / 60, 2, 3)
        _same(h, o, len(used))
        box = _oracle_box(o, WHITE)
        small = small + 1 if box < 512 else 0
        if rule_step is None and small == 2:
            rule_step = len(used) + 1
        used.append(h.stats()["cell_hash"][WHITE])
        print("wide add step %d: oracle white box %d cells, device cell_hash %s" % (len(used), box, h.stats()["cell_hash"]))
    assert (rule_step, len(used)) == (11, 15)
    assert used[0] > 0 and used[-1] == 0, used


# ------------------------------------------------------------------------------------------------ (c) goldens under the hook

def _golden_state(h, w):
    return np.array([h.download(w, f) for f in STATE])


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_goldens_on_the_hash_table(egg, name):
    g = load_golden(name)
    h = _handler(egg)

    def check(step, tag, arr):
        assert np.array_equal(arr, g["%s_step%d" % (tag, step)]), (name, step, tag)
        _hashed(h)

    ids = replay_golden(g, h, _golden_state, check)
    assert np.array_equal(np.array([h.get_position(i) for i in ids]), g["centroid_step%d" % int(g["snap_steps"][-1])])
    st = _hashed(h)
    assert st["pair_solves"] == int(g["visits"].sum())


@pytest.mark.parametrize("walk", [1, 2])
@pytest.mark.parametrize("name", ["cfg1_moving", "four_batches", "substeps_3_2", "substeps_2_1"])
def test_goldens_on_the_hash_table_packed(egg, name, walk):
    """pk_build_grid / pk_visit_fresh / pk_visit_stale through cell_meta(), with both level walks"""
    g = load_golden(name)
    h = _handler(egg, PACKED=1, LEVEL_WALK=walk)

    def check(step, tag, arr):
        assert np.array_equal(arr, g["%s_step%d" % (tag, step)]), (name, step, tag)

    replay_golden(g, h, _golden_state, check)
    st = _hashed(h)
    assert st["pair_solves"] == int(g["visits"].sum())
    assert st["packed"][WHITE] > 0  # (one batch: the yolk budget binds and that type runs the exact-budget fused tile)


# ------------------------------------------------------------------------------------------------ (d) hash generations

THREE_CENTERS = [(300.0, 300.0), (340.0, 320.0), (900.0, 300.0)]  # two overlapping batches and one apart


def _run_three(h, o, S, C, steps=6):
    for x, y in THREE_CENTERS:
        assert h.add(x, y, 50, 15) == o.add(x, y, 50, 15)
    for k in range(steps):
        for i, c in enumerate(THREE_CENTERS):
            t = circle_target(c, 2 * k)
            h.set_target_position(i + 1, *t)
            o.set_target_position(i + 1, *t)
        h.step(1 / 60, S, C)
        o.step(1 / 60, S, C)
        _same(h, o, (S, C, k))
        _hashed(h)


@pytest.mark.parametrize("S,C", [(1, 1), (2, 1), (3, 1), (4, 1), (8, 1), (3, 2), (4, 3)])
def test_hash_generations(egg, oracle_mod, S, C):
    """one collision pass per sub-step never clears the cells inside a step: up to eight generations, each with a key
    table of its own (the _mg kernel variants from three generations on)"""
    _run_three(_handler(egg), oracle_mod.Oracle(), S, C)


@pytest.mark.parametrize("S,C", [(2, 1), (2, 2), (2, 3)])
def test_hash_generations_packed(egg, oracle_mod, S, C):
    """the stale pass of the packed pipeline: pk_visit_stale looks both generations up through cell_meta()"""
    h = _handler(egg, PACKED=1)
    _run_three(h, oracle_mod.Oracle(), S, C)
    assert h.stats()["packed"][WHITE] > 0


# ------------------------------------------------------------------------------------------------ (e) kernel variants

# two overlapping batches, one apart, twelve particles within 1e-9 of each other, one batch flying through the scene
MATRIX_BATCHES = [(300.0, 300.0, 50.0, 15.0, 157, 15), (340.0, 320.0, 50.0, 15.0, 157, 15), (900.0, 100.0, 50.0, 15.0, 157, 15),
                  (200.0, 650.0, 1e-9, 1e-9, 12, 6), (-600.0, 300.0, 50.0, 15.0, 157, 15)]
MATRIX_STEPS = 8


def _matrix_targets(k):
    out = [(x + 4.0 * k, y - 3.0 * k) for x, y, *_ in MATRIX_BATCHES[:4]]
    return out + [(-600.0 + 2500.0, 300.0 + 900.0)]  # far away: the blob accelerates to tens of cells per step


_matrix_reference = []


def _matrix_oracle(oracle_mod):
    """the oracle's state after every step of the matrix scene, computed once for all legs"""
    if not _matrix_reference:
        o = oracle_mod.Oracle()
        for x, y, wr, yr, wn, yn in MATRIX_BATCHES:
            o.add(x, y, wr, yr, wn, yn)
        for k in range(MATRIX_STEPS):
            for i, t in enumerate(_matrix_targets(k)):
                o.set_target_position(i + 1, *t)
            o.step(1 / 60, 2, 3)
            _matrix_reference.append(([[o.field(w, f) for f in STATE] for w in (WHITE, YOLK)], o.total_visited))
    return _matrix_reference


MATRIX_LEGS = [{}, dict(FORCE_SINGLE_TILE=1), dict(FORCE_GLOBAL_STATE=1), dict(THREADS_PER_PARTICLE=1), dict(THREADS_PER_PARTICLE=3),
               dict(TILE_TARGET_PARTICLES=0), dict(TILE_TARGET_PARTICLES=700), dict(FUSE_TYPES=0), dict(PACKED=1, LEVEL_WALK=1),
               dict(PACKED=1, LEVEL_WALK=2)]


@pytest.mark.parametrize("options", MATRIX_LEGS, ids=["-".join("%s=%d" % kv for kv in leg.items()) or "hook_only" for leg in MATRIX_LEGS])
def test_variant_matrix_on_the_hash_table(egg, oracle_mod, options):
    """every kernel variant the host can pick, each with the hash table forced: all equal the oracle, hence each other"""
    reference = _matrix_oracle(oracle_mod)
    h = _handler(egg, **options)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for k, (x, y, wr, yr, wn, yn) in enumerate(MATRIX_BATCHES):
            assert h.add(x, y, wr, yr, None, None, wn, yn) == k + 1
    for k in range(MATRIX_STEPS):
        for i, t in enumerate(_matrix_targets(k)):
            h.set_target_position(i + 1, *t)
        h.step(1 / 60, 2, 3)
        state, visited = reference[k]
        for w in (WHITE, YOLK):
            for f, ref in zip(STATE, state[w]):
                assert np.array_equal(h.download(w, f), ref), (options, k, w, f)
        assert _hashed(h)["pair_solves"] == visited, (options, k)
    if "PACKED" in options:
        assert h.stats()["packed"][WHITE] > 0


# ------------------------------------------------------------------------------------------------ (f) dense islands

def test_dense_island_on_the_hash_table(egg, oracle_mod):
    """four coincident default batches: 628 white particles in one island, visit lists in global memory (_gl variant)"""
    h, o = _handler(egg), oracle_mod.Oracle()
    for _ in range(4):
        assert h.add(300.0, 300.0, 50, 15) == o.add(300.0, 300.0, 50, 15)
    for k in range(4):
        h.step(1 / 60, 2, 3)
        o.step(1 / 60, 2, 3)
        _same(h, o, k)
        _hashed(h)
    assert h.stats()["max_tile_particles"][WHITE] == 4 * 157


def test_large_island_in_global_memory_on_the_hash_table(egg, oracle_mod):
    """the 4 x 4 island of test_large_island_falls_back_to_global_memory_state: 2,512 white particles, state in global memory
    (_gs variant), a hash table of 4,096 slots"""
    k = np.arange(16)
    xs, ys = 500.0 + 95.0 * (k % 4), 500.0 + 95.0 * (k // 4)
    h, o = _handler(egg), oracle_mod.Oracle()
    h.add_many(xs, ys, 50, 15)
    for x, y in zip(xs, ys):
        o.add(float(x), float(y), 50, 15)
    for _ in range(3):
        h.step(1 / 60, 2, 3)
        o.step(1 / 60, 2, 3)
    _same(h, o, "4 x 4 island")
    assert _hashed(h)["max_tile_particles"][WHITE] == 16 * 157


# ------------------------------------------------------------------------------------------------ (g) mass guard, budget

@pytest.mark.parametrize("centers", [[(300.0, 300.0)], [(300.0, 300.0), (340.0, 320.0), (300.0, 350.0)]],
                         ids=["one_batch_exact_budget", "three_overlapping"])
def test_mass_guard_on_the_hash_table(egg, oracle_mod, centers):
    """test_mass_guard_pairs_match_oracle, tweak "mixed": pairs the guard w_i + w_j < eps (L:1601) marks in `collided`
    without projecting or counting them"""
    from egg_fluid_simulation_amd.default_config import default_configs
    tweak = dict(max_mass=1e9)
    w, y = default_configs()
    w.update(tweak)
    y.update(tweak)
    h, o = _handler(egg, w, y), oracle_mod.Oracle()
    o.set_config(WHITE, dict(oracle_mod.DEFAULT_WHITE, **tweak))
    o.set_config(YOLK, dict(oracle_mod.DEFAULT_YOLK, **tweak))
    for cx, cy in centers:
        assert h.add(cx, cy, 50, 15) == o.add(cx, cy, 50, 15)
    for step in range(8):
        for i, (cx, cy) in enumerate(centers):
            h.set_target_position(i + 1, cx + 5.0 * step, cy + 3.0 * step)
            o.set_target_position(i + 1, cx + 5.0 * step, cy + 3.0 * step)
        h.step(1 / 60, 2, 3)
        o.step(1 / 60, 2, 3)
        _same(h, o, (len(centers), step))
        _hashed(h)
    inv = o.field(WHITE, "inv_mass")
    assert int((inv[:, None] + inv[None, :] < 1e-8).sum()) > 0  # the case does reach the guard


def test_budget_cuts_both_types_on_the_hash_table(egg, oracle_mod):
    """test_budget_cuts_both_types, radii (24, 12): passes of both types cut by the budget return (L:1657-1658), the stale
    passes look `collided` up in the cut lists"""
    h, o = _handler(egg), oracle_mod.Oracle()
    assert h.add(100.0, 100.0, 24.0, 12.0) == o.add(100.0, 100.0, 24.0, 12.0)
    cut = {WHITE: False, YOLK: False}
    for step in range(15):
        h.set_target_position(1, 100.0 + 2.0 * step, 100.0 + 1.5 * step)
        o.set_target_position(1, 100.0 + 2.0 * step, 100.0 + 1.5 * step)
        h.step(1 / 60, 2, 3)
        o.step(1 / 60, 2, 3)
        for s in o.pass_stats():
            cut[s["which"]] = cut[s["which"]] or bool(s["cut"])
        _hashed(h)
    _same(h, o, "budget")
    assert cut[WHITE] and cut[YOLK], cut


# ------------------------------------------------------------------------------------------------ (h) randomised sessions

@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_session_on_the_hash_table(egg, oracle_mod, seed):
    """the sessions of test_random_session_matches_oracle (adds, removes, teleports, live configs, changing shapes): table
    sizes and probe chains change from step to step"""
    from egg_fluid_simulation_amd import _ffi
    from test_gpu_fuzz import random_session
    h = random_session(egg, oracle_mod, seed, configure=lambda hh: hh.set_option(_ffi.OPT_FORCE_CELL_HASH, 1))
    _hashed(h)


# ------------------------------------------------------------------------------------------------ (i) surface

def test_option_round_trip_and_counter(egg, oracle_mod):
    """0 / 1 / 0 on one handle: the counter follows from the next step on, the results never change.  The compact default
    scene is twelve eggs, not one or two: with a few eggs the yolk budget binds, and an exact-budget tile claims 64 cells
    around its particles (retile(): no neighbour to keep apart from), more than the dense grid's 16,384 cells -- such a
    tile is on the hash table whatever its size (config 1's yolk, for one)."""
    from egg_fluid_simulation_amd import _ffi
    h, o = _handler(egg, hook=False), oracle_mod.Oracle()
    assert h.stats()["cell_hash"] == [0, 0]  # a fresh handle
    for k in range(12):  # a compact default scene whose budgets do not bind
        x, y = 100.0 + 150.0 * (k % 4), 100.0 + 150.0 * (k // 4)
        assert h.add(x, y, 50, 15) == o.add(x, y, 50, 15)
    for value, expect_hash in ((None, False), (1, True), (0, False), (7, True), (0, False)):
        if value is not None:
            h.set_option(_ffi.OPT_FORCE_CELL_HASH, value)
        retiles = h.stats()["retiles"]
        for _ in range(2):
            h.step(1 / 60, 2, 3)
            o.step(1 / 60, 2, 3)
            _same(h, o, (value, expect_hash))
            st = h.stats()
            assert st["single_tile"] == [0, 0]
            assert [c > 0 for c in st["cell_hash"]] == [expect_hash, expect_hash], (value, st["cell_hash"])
        if value is not None:
            assert h.stats()["retiles"] > retiles  # the option marks both tilings dirty
    with pytest.raises(egg.EggError):
        h.set_option(_ffi.OPT_FORCE_CELL_HASH + 1, 1)  # still the last option


def test_relaxed_order_ignores_the_option(egg):
    """relaxed order has a hash table of its own: the option is accepted, changes no bit and leaves the counter alone"""
    from egg_fluid_simulation_amd import _ffi
    from relaxed_model import DEFAULT_RELAXATION, RelaxedModel
    centers = [tuple(c) for c in load_golden("four_batches")["centers"]]
    h, m = _handler(egg, hook=False), RelaxedModel(relaxed=True, relaxation=DEFAULT_RELAXATION)
    h.set_solver_order("relaxed")
    h.set_option(_ffi.OPT_FORCE_CELL_HASH, 1)
    ids = [h.add(cx, cy, 50, 15) for cx, cy in centers]
    assert [m.add(cx, cy, 50, 15) for cx, cy in centers] == ids
    for k in range(3):
        for i, c in zip(ids, centers):
            t = circle_target(c, k)
            h.set_target_position(i, *t)
            m.set_target_position(i, *t)
        assert h.update(1 / 60, 1 / 60, 2, 3) == 1
        m.update(1 / 60, 1 / 60, 2, 3)
    fields = ("x", "y", "vx", "vy", "last_x", "last_y")
    for w in (WHITE, YOLK):
        dev, ref = np.array([h.download(w, f) for f in fields]), m.state(w)
        for k, f in enumerate(fields):
            assert np.array_equal(dev[k], ref[k]), (w, f)
    st = h.stats()
    assert st["pair_solves"] == m.pair_solves and st["relaxed_steps"] == 3 and st["cell_hash"] == [0, 0]
