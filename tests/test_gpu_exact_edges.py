"""The exact-order pair projection on the device where random scenes do not go: the hand table of tests/test_exact_census.py
-- aligned pairs with every sign of zero, the exact edge and one ulp either side of it, coincident pairs at (-0.0, -0.0),
separations below eps down to a subnormal one, the clamp, the mass guard, every neighbour cell, the budget cut -- under every
live site of the projection (csrc/eggsim_tile.h):

  variant        options                                                       site                           stats() must show
  fused          none, no ballast: the budget of 2 to 10 particles binds       scheduler of the fused step kernel  packed 0
  tpp1, tpp3     THREADS_PER_PARTICLE 1 / 3, state in LDS (the pair cache)     project_pair<CACHED = true>    packed 0
  tpp1_gs, tpp3_gs   ... with FORCE_GLOBAL_STATE = 1                           project_pair<CACHED = false>   packed 0
  hash           FORCE_CELL_HASH = 1                                           the same scheduler, hashed cells   cell_hash > 0
  chain          PACKED = 1, LEVEL_WALK = 1                                    egg_pk_exec_chain_kernel (project_pair_predicated)   packed >= 1, EXEC_CHAIN
  exec           ... with TILE_TARGET_PARTICLES = 0, GROUP_PARTICLES = 1 and 1,030 ballast batches: one tile to a group, more
                 groups than the chip has SIMDs                                egg_pk_exec_kernel (project_pair<true>)   packed >= 1, EXEC
  levexec        PACKED = 1, LEVEL_WALK = 2 beside an island of 314 white particles   egg_pk_levexec_kernel (predicated)   PASS_FUSED
  (project_pair_reference is the fallback inside each of them: every case whose census has no `fast` takes it)

Ballast (tests/test_exact_census.py): `far` is one resting batch of 64 + 64 particles 5,000 px away, which lifts the
budget off the planted pairs and makes a second tile (a type that is one tile runs in single-tile mode and never packs);
`many` and `blob` as the table says.  Every run first asserts, on the model WITH that ballast, that the planted pair is the
first evaluation of either type and carries the labels the case is named for (assert_case), then compares x, y, vx, vy,
last_x, last_y of every particle on their bit patterns, pair_solves after either update, and the batch positions.

Which label by which case: the table in tests/test_exact_census.py's docstring.  Every case of it runs under every variant
(184 runs of 2 to 10 planted particles per type; 2 + 64, 2 + 314 or 2 + 1,030 x (1 to 9) with the ballast), so that table holds at
every site.  Measured on an MI355X: all 184 equal the model bit for bit.

Exceptions to "every label under every site": none among axis_x, axis_y, edge, coincident_same, coincident_other,
below_eps, guarded, clamp_hi, fast.  Under `levexec` the yolk type (30 + n particles: its budget binds) runs the
exact-budget fused tile, so that site is asserted for the white type only; `exec` is asserted for the white type only as
well (the yolk ballast is two particles to a batch).  The follow cases (follow_edge, pulled) run under `fused` and `chain` only:
the follow constraint is not a projection site."""
import warnings

import numpy as np
import pytest

import test_exact_census as tc

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1

# variant -> (ballast, options by their _ffi name without OPT_)
VARIANTS = {
    "fused": (None, {}),
    "tpp1": ("far", dict(THREADS_PER_PARTICLE=1)),
    "tpp3": ("far", dict(THREADS_PER_PARTICLE=3)),
    "tpp1_gs": ("far", dict(THREADS_PER_PARTICLE=1, FORCE_GLOBAL_STATE=1)),
    "tpp3_gs": ("far", dict(THREADS_PER_PARTICLE=3, FORCE_GLOBAL_STATE=1)),
    "hash": ("far", dict(FORCE_CELL_HASH=1)),
    "chain": ("far", dict(PACKED=1, LEVEL_WALK=1)),
    "exec": ("many", dict(PACKED=1, LEVEL_WALK=1, TILE_TARGET_PARTICLES=0, GROUP_PARTICLES=1)),
    "levexec": ("blob", dict(PACKED=1, LEVEL_WALK=2)),
}
PROJECTION_CASES = sorted(set(tc.CASES) - {"follow_edge", "pulled"})
RUNS = [(c, v) for v in VARIANTS for c in PROJECTION_CASES] + [(c, v) for v in ("fused", "chain") for c in ("follow_edge", "pulled")]


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


@pytest.fixture(scope="module")
def infos(egg):
    """the batch infos of the tiny planted batches and of the `far` ballast batch, exported once from a default handle"""
    src = egg.SimulationHandler()
    tiny = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for b in range(5):
            i = src.add(*tc.HAND_TARGET, tc.HAND_RADIUS, tc.HAND_RADIUS, None, None, 2, 2)
            tiny.append(src.export_batch(i)[0])
        far = src.export_batch(src.add(*tc.FAR_CENTER, tc.HAND_RADIUS, tc.HAND_RADIUS, None, None, tc.FAR_N, tc.FAR_N))[0]
    return tiny, far


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_same(h, snap, ids, tag):
    for w in (WHITE, YOLK):
        for f in tc.FIELDS:
            got = _bits(h.download(w, f))
            assert got.shape == snap["state"][w][f].shape and np.array_equal(got, snap["state"][w][f]), (tag, w, f)
    assert h.stats()["pair_solves"] == snap["pairs"], tag
    for i in ids:
        assert tuple(_bits(h.get_position(i)).tolist()) == snap["pos"][i], (tag, i)


def _assert_variant(h, variant, tag):
    from egg_fluid_simulation_amd import _ffi
    st = h.stats()
    if variant in ("fused", "tpp1", "tpp3", "tpp1_gs", "tpp3_gs", "hash"):
        assert st["packed"] == [0, 0], (tag, st["packed"])
        if variant == "hash":
            assert all(c > 0 for c in st["cell_hash"]), (tag, st["cell_hash"])
    elif variant == "chain":
        assert st["packed"][WHITE] >= 1 and st["packed"][YOLK] >= 1, (tag, st["packed"])
        for w in (WHITE, YOLK):
            assert st["pk_variants"][w] & _ffi.PK_VARIANT_EXEC_CHAIN and not st["pk_variants"][w] & (_ffi.PK_VARIANT_EXEC | _ffi.PK_VARIANT_PASS_FUSED), (tag, st["pk_variants"])
    elif variant == "exec":
        assert st["packed"][WHITE] >= 1, (tag, st["packed"])
        assert st["pk_variants"][WHITE] & _ffi.PK_VARIANT_EXEC and not st["pk_variants"][WHITE] & (_ffi.PK_VARIANT_EXEC_CHAIN | _ffi.PK_VARIANT_PASS_FUSED), (tag, st["pk_variants"])
    elif variant == "levexec":
        assert st["packed"][WHITE] >= 1 and st["pk_variants"][WHITE] & _ffi.PK_VARIANT_PASS_FUSED, (tag, st["packed"], st["pk_variants"])
        assert st["max_tile_particles"][WHITE] >= 314, (tag, st["max_tile_particles"])


@pytest.mark.parametrize("name,variant", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_hand_case(egg, infos, name, variant):
    from egg_fluid_simulation_amd import _ffi
    ballast, options = VARIANTS[variant]
    m, ids, snaps = tc.assert_case(name, ballast)  # the branches, on the model with this ballast, first
    tiny, far = infos
    h = egg.SimulationHandler()
    w, y = tc.configs(name)
    keys = sorted(set(tc.BASE) | set(tc.CONFIGS[tc.CASES[name]["cfg"]]))
    h.set_white_config({k: w[k] for k in keys})
    h.set_yolk_config({k: y[k] for k in keys})
    for k, v in options.items():
        h.set_option(getattr(_ffi, "OPT_" + k), v)
    ws, ys = tc.columns(name, WHITE), tc.columns(name, YOLK)
    for b, i in enumerate(ids):
        assert h.import_batch(tiny[b], ws[:, 2 * b:2 * b + 2], ys[:, 2 * b:2 * b + 2]) == i
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if ballast == "far":
            h.import_batch(far, tc.far_columns(name, WHITE), tc.far_columns(name, YOLK))
        elif ballast == "blob":
            for _ in range(2):
                h.add(*tc.BLOB_CENTER, 50, 15, None, None, 157, 15)
        elif ballast == "many":
            xs, ys_, nw = tc.many_centers(name)
            h.add_many(xs, ys_, tc.MANY_RADIUS, tc.MANY_RADIUS, nw, 2)
    assert tuple(h.get_n_particles()) == (len(m.field(WHITE, tc.rm.X)), len(m.field(YOLK, tc.rm.X)))
    for k, (u, snap) in enumerate(zip(tc.UPDATES, snaps)):
        assert h.update(*u) == 1
        _assert_same(h, snap, ids, (name, variant, "update %d" % (k + 1)))
        _assert_variant(h, variant, (name, variant, k))
