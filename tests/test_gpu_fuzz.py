"""Randomised sessions against the CPU oracle (fixed seeds): batches of different sizes are added and removed
while the simulation runs, targets drift, jump and collide, configs change live, and the (sub-steps, passes)
shape changes from step to step.  After every few steps every particle of both types must agree bit for bit
and the visited-pair counters must match: whatever the tiling, kernel variant or recovery path the host
picked along the way, the result is the reference's sequential result."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _bits(a):
    """the bit patterns: np.array_equal on floats cannot tell -0.0 from +0.0"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(h, o, tag):
    for w in (WHITE, YOLK):
        for f in ("x", "y", "vx", "vy"):
            a, b = h.download(w, f), o.field(w, f)
            assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), (tag, w, f)
    assert h.stats()["pair_solves"] == o.total_visited, tag


def random_session(egg, oracle_mod, seed, configure=None):
    """one session of `seed` on a fresh handler (after configure(h), if given) and a fresh oracle, compared every six
    steps and at the end; returns the handler"""
    from egg_fluid_simulation_amd.default_config import default_configs
    rng = np.random.default_rng(seed)
    h, o = egg.SimulationHandler(), oracle_mod.Oracle()
    if configure:
        configure(h)
    live = {}  # id -> [x, y, vx, vy] of the target

    def add():
        x, y = rng.uniform(-300, 900, 2)
        wr = float(rng.choice([20.0, 35.0, 50.0, 64.0]))
        yr = float(rng.choice([9.0, 15.0, 20.0]))
        a = h.add(float(x), float(y), wr, yr)
        b = o.add(float(x), float(y), wr, yr)
        assert a == b
        live[a] = [float(x), float(y), *rng.uniform(-6, 6, 2)]

    for _ in range(int(rng.integers(3, 9))):
        add()
    shapes = [(2, 3), (2, 3), (2, 3), (1, 1), (1, 3), (2, 1), (3, 1), (4, 2), (5, 1)]
    for step in range(100):
        r = rng.random()
        if r < 0.10 and len(live) < 14:
            add()
        elif r < 0.16 and len(live) > 1:
            victim = int(rng.choice(sorted(live)))
            h.remove(victim)
            o.remove(victim)
            del live[victim]
        elif r < 0.20:
            w, y = default_configs()
            kw = dict(damping=float(rng.uniform(0.05, 0.6)), collision_strength=float(rng.uniform(0.7, 1.0)),
                      follow_strength=float(rng.uniform(0.9, 1.0)))
            w.update(kw)
            h.set_white_config(w)
            o.set_config(WHITE, dict(oracle_mod.DEFAULT_WHITE, **kw))
        for i, t in live.items():
            if rng.random() < 0.04:  # teleport the target: the blob races after it
                t[0], t[1] = (float(v) for v in rng.uniform(-300, 900, 2))
            t[0] += t[2]
            t[1] += t[3]
            if rng.random() < 0.1:
                t[2], t[3] = (float(v) for v in rng.uniform(-6, 6, 2))
            h.set_target_position(i, t[0], t[1])
            o.set_target_position(i, t[0], t[1])
        S, C = shapes[int(rng.integers(len(shapes)))]
        h.step(1 / 60, S, C)
        o.step(1 / 60, S, C)
        if step % 6 == 5:
            _same(h, o, (seed, step))
    _same(h, o, (seed, "end"))
    for i in live:
        assert h.get_position(i) == o.get_position(i)
    return h


@pytest.mark.parametrize("seed", list(range(1, 11)))
def test_random_session_matches_oracle(egg, oracle_mod, seed):
    random_session(egg, oracle_mod, seed)


def test_crowded_scene_on_a_shared_chip(egg, oracle_mod):
    """320 batches (more white tiles than CUs: the narrow kernel variants, several launch classes in one grid)
    wandering into each other for 30 steps: islands merge and split, claims get widened, steps get re-run"""
    rng = np.random.default_rng(5)
    n = 320
    side = 18
    xs = 100.0 + 170.0 * (np.arange(n) % side)
    ys = 100.0 + 170.0 * (np.arange(n) // side)
    h, o = egg.SimulationHandler(), oracle_mod.Oracle()
    ids = h.add_many(xs, ys, 50, 15)
    for x, y in zip(xs, ys):
        o.add(float(x), float(y), 50, 15)
    vel = rng.uniform(-2.5, 2.5, (n, 2))  # neighbours meet here and there; faster and the whole scene chains into
    # one island beyond the 32,766-particle limit of a tile
    tx, ty = xs.copy(), ys.copy()
    tiles_seen = []
    for step in range(30):
        tx += vel[:, 0]
        ty += vel[:, 1]
        h.set_target_positions(ids, tx, ty)
        for i, a, b in zip(ids, tx, ty):
            o.set_target_position(int(i), float(a), float(b))
        h.step(1 / 60, 2, 3)
        o.step(1 / 60, 2, 3)
        tiles_seen.append(h.stats()["n_tiles"][0])
        if step % 10 == 9:
            _same(h, o, step)
    # the run starts with more white tiles than CUs (narrow variants, one grid for all classes) and ends with
    # many islands merged
    assert max(tiles_seen) > 256 and min(tiles_seen) < n, (tiles_seen[0], tiles_seen[-1])


CONFIG_CORNERS = [
    dict(collision_strength=1.0),                       # compliance exactly 0
    dict(collision_strength=0.0, follow_strength=0.0),  # softest constraints
    dict(follow_strength=1.0, damping=1.0),             # velocities wiped every sub-step
    dict(damping=0.0),                                  # nothing damped
    dict(min_radius=4.0, max_radius=4.0, min_mass=2.0, max_mass=2.0),  # identical particles
    dict(collision_overlap_factor=3.5),                 # larger cells through the overlap factor
    dict(cohesion_interaction_distance_factor=5.0),     # cell size from the (dead) cohesion factor, L:1760
    dict(max_radius=9.0, min_radius=1.0, max_mass=50.0),  # wide radius / mass spread
]


@pytest.mark.parametrize("tweak", CONFIG_CORNERS, ids=[",".join(sorted(t)) for t in CONFIG_CORNERS])
def test_config_corners_match_oracle(egg, oracle_mod, tweak):
    """solver configurations at and beyond the edges of the default file: every particle bit for bit"""
    from egg_fluid_simulation_amd.default_config import default_configs
    w, y = default_configs()
    w.update(tweak)
    y.update(tweak)
    h = egg.SimulationHandler(w, y)
    o = oracle_mod.Oracle()
    o.set_config(WHITE, dict(oracle_mod.DEFAULT_WHITE, **tweak))
    o.set_config(YOLK, dict(oracle_mod.DEFAULT_YOLK, **tweak))
    cs = [(300.0, 300.0), (380.0, 330.0), (900.0, 100.0)]
    for x, yy in cs:
        h.add(x, yy, 50, 15)
        o.add(x, yy, 50, 15)
    for step in range(12):
        for i, (x, yy) in enumerate(cs):
            h.set_target_position(i + 1, x + 4.0 * step, yy - 3.0 * step)
            o.set_target_position(i + 1, x + 4.0 * step, yy - 3.0 * step)
        h.step(1 / 60, 2, 3)
        o.step(1 / 60, 2, 3)
    _same(h, o, tweak)


@pytest.mark.parametrize("radii", [(20.0, 9.0), (24.0, 12.0), (30.0, 9.0)])
def test_budget_cuts_both_types(egg, oracle_mod, radii):
    """one small blob: 0.05 N^2 is below the adjacent pairs of BOTH particle types, so passes of both are cut
    by the budget return (L:1657-1658) and the stale passes look `collided` up in the cut lists"""
    h, o = egg.SimulationHandler(), oracle_mod.Oracle()
    h.add(100.0, 100.0, *radii)
    o.add(100.0, 100.0, *radii)
    cut = {WHITE: False, YOLK: False}
    for step in range(15):
        h.set_target_position(1, 100.0 + 2.0 * step, 100.0 + 1.5 * step)
        o.set_target_position(1, 100.0 + 2.0 * step, 100.0 + 1.5 * step)
        h.step(1 / 60, 2, 3)
        o.step(1 / 60, 2, 3)
        for s in o.pass_stats():
            cut[s["which"]] = cut[s["which"]] or bool(s["cut"])
    _same(h, o, radii)
    assert cut[WHITE] and cut[YOLK], cut
