"""The relaxed-order solver (EGG_OPT_SOLVER_ORDER = 1) on the device against the CPU model
tests/relaxed_model.py.  Every comparison is bit for bit: the kernel and the model evaluate the same definition
operation for operation."""

import numpy as np
import pytest

import bench
from conftest import circle_target, load_golden
from relaxed_model import DEFAULT_RELAXATION, RelaxedModel

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
FIELDS = ("x", "y", "vx", "vy", "last_x", "last_y")
ENV_KEYS = ("min_x", "min_y", "max_x", "max_y", "centroid_x", "centroid_y", "max_radius", "max_velocity",
            "last_centroid_x", "last_centroid_y")


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _dev_state(h, w):
    return np.array([h.download(w, f) for f in FIELDS])


def _assert_same(h, m, ids, what=""):
    for w in (WHITE, YOLK):
        dev, ref = _dev_state(h, w), m.state(w)
        for k, f in enumerate(FIELDS):
            assert np.array_equal(dev[k], ref[k]), "%s type %d field %s" % (what, w, f)
        env_m = m._last_white_env if w == WHITE else m._last_yolk_env
        env_d = h.get_environment(w)
        for key in ENV_KEYS:
            assert env_d[key] == env_m[key], "%s type %d env %s" % (what, w, key)
    for i in ids:
        assert h.get_position(int(i)) == tuple(m.get_position(int(i))), "%s position %d" % (what, i)
    assert h.stats()["pair_solves"] == m.pair_solves, what


def _pair(egg, relaxed=True, relaxation=None):
    h = egg.SimulationHandler()
    m = RelaxedModel(relaxed=relaxed, relaxation=DEFAULT_RELAXATION if relaxation is None else relaxation)
    if relaxed:
        h.set_solver_order("relaxed", relaxation)
    return h, m


def _four_batches(h, m):
    centers = [tuple(c) for c in load_golden("four_batches")["centers"]]
    ids = [h.add(cx, cy, 50, 15) for cx, cy in centers]
    assert [m.add(cx, cy, 50, 15) for cx, cy in centers] == ids
    return centers, ids


def _step_both(h, m, ids, centers, k, S=2, C=3, moving=True):
    if moving:
        for i, c in zip(ids, centers):
            tx, ty = circle_target(c, k)
            h.set_target_position(i, tx, ty)
            m.set_target_position(i, tx, ty)
    assert h.update(1 / 60, 1 / 60, S, C) == 1
    m.update(1 / 60, 1 / 60, S, C)


def test_surface(egg):
    h = egg.SimulationHandler()
    assert h.get_solver_order() == "exact"
    h.add(400, 300, 50, 15)
    h.step(1 / 60, 2, 3)
    assert h.stats()["relaxed_steps"] == 0
    for bad in (0.0, -1.0, 2.5, float("nan"), float("inf")):
        with pytest.raises(egg.EggError):
            h.set_solver_order("relaxed", bad)
        with pytest.raises(egg.EggError):
            h.set_option(egg._ffi.OPT_RELAXATION, bad)
    assert h.get_solver_order() == "exact"
    with pytest.raises(egg.EggError):
        h.set_solver_order("chaotic")
    with pytest.raises(egg.EggError):
        h.set_option(egg._ffi.OPT_SOLVER_ORDER, 2)
    h.set_option(egg._ffi.OPT_RELAXATION, 2.0)  # the closed end of the range
    h.set_solver_order("relaxed", 1.0)
    assert h.get_solver_order() == "relaxed"
    h.step(1 / 60, 2, 3)
    h.update(1 / 60)
    st = h.stats()
    assert st["relaxed_steps"] == 2 and st["steps"] == 3
    h.prepare_step()  # nothing to prepare
    with pytest.raises(egg.EggError):
        h.step_begin()
    with pytest.raises(egg.EggError):
        h.get_claims(h.list_ids())
    h.set_solver_order("exact")
    h.step(1 / 60, 2, 3)
    assert h.stats()["relaxed_steps"] == 2 and h.stats()["steps"] == 4
    h.step_begin()
    h.step_end(True)


def test_timing_counts_relaxed_steps(egg):
    h = egg.SimulationHandler()
    h.add_many(np.array([100.0, 400.0]), np.array([100.0, 100.0]), 50, 15)
    h.set_solver_order("relaxed")
    h.set_option(egg._ffi.OPT_TIMING, 1)
    for _ in range(3):
        h.step(1 / 60, 2, 3)
    st = h.stats()
    assert st["timed_steps"] == 3 and st["kernel_ms"][0] > 0 and st["kernel_ms_sum"][0] >= st["kernel_ms"][0]


@pytest.mark.parametrize("S,C", [(2, 3), (3, 2), (2, 1), (1, 1)])
@pytest.mark.parametrize("omega", [1.0, 1.5])
def test_parity_with_model(egg, S, C, omega):
    h, m = _pair(egg, relaxation=omega)
    centers, ids = _four_batches(h, m)
    for k in range(20):
        _step_both(h, m, ids, centers, k, S, C)
        if k in (0, 19):
            _assert_same(h, m, ids, "S=%d C=%d omega=%g step %d" % (S, C, omega, k + 1))
    assert h.stats()["max_pass_visits"][0] == max(m.relaxed_pass_pairs[0::2])


@pytest.mark.parametrize("S,C", [(2, 3), (1, 1)])
def test_launches_of_one_step(egg, S, C):
    """The launch sequence of a relaxed step, counted: per populated type S begin / mid kernels, five launches per
    collision pass (insert, scan, scatter, rank, gather) and the end kernel.  Taken over the second step: the first
    also builds the per-particle atom table."""
    h, m = _pair(egg)
    centers, ids = _four_batches(h, m)
    _step_both(h, m, ids, centers, 0, S, C)
    before = h.stats()["kernel_launches"]
    _step_both(h, m, ids, centers, 1, S, C)
    delta = h.stats()["kernel_launches"] - before
    print("single handle S=%d C=%d: %d launches" % (S, C, delta))
    assert all(n > 0 for n in h.get_n_particles())
    assert delta == 2 * (S + 5 * S * C + 1)


def test_coincident_batches(egg):
    h, m = _pair(egg)
    centers = [(300.0, 300.0)] * 4 + [(700.0, 300.0)]
    ids = [h.add(cx, cy, 50, 15) for cx, cy in centers]
    for cx, cy in centers:
        m.add(cx, cy, 50, 15)
    for k in range(10):
        _step_both(h, m, ids, centers, k, moving=False)
    _assert_same(h, m, ids, "coincident")
    for w in (WHITE, YOLK):
        x, y = h.download(w, "x"), h.download(w, "y")
        n = len(x) // 5
        for a in range(4):
            for b in range(a + 1, 4):
                d = np.hypot(x[a * n:(a + 1) * n] - x[b * n:(b + 1) * n], y[a * n:(a + 1) * n] - y[b * n:(b + 1) * n])
                assert float(d.min()) > 0.0


def test_mutations_between_relaxed_steps(egg):
    h, m = _pair(egg)
    centers, ids = _four_batches(h, m)
    for k in range(4):
        _step_both(h, m, ids, centers, k)
    h.remove(ids[1])
    m.remove(ids[1])
    centers, ids = [centers[0]] + centers[2:], [ids[0]] + ids[2:]
    for k in range(4, 7):
        _step_both(h, m, ids, centers, k)
    _assert_same(h, m, ids, "after remove")
    i_new = h.add(60.0, -30.0, 40, 12)
    assert m.add(60.0, -30.0, 40, 12) == i_new
    centers, ids = centers + [(60.0, -30.0)], ids + [i_new]
    for k in range(7, 10):
        _step_both(h, m, ids, centers, k)
    _assert_same(h, m, ids, "after add")
    # a live config change: mass is re-derived at the next step (L:1731-1744).  (A radius change is checked against
    # its closed form below, not against the model: oracle/reference_model.py lets _post_solve's max_radius overwrite
    # the environment's config max_radius before the next sub-step's pre-solve, where the C oracle and the device keep
    # the config's value.)
    h.set_white_config({"max_mass": 2.5})
    m._white_config.update(max_mass=2.5)
    h.set_yolk_config({"min_mass": 0.5})
    m._yolk_config.update(min_mass=0.5)
    for k in range(10, 14):
        _step_both(h, m, ids, centers, k)
    _assert_same(h, m, ids, "after config change")
    assert np.array_equal(h.download(WHITE, "inv_mass"), np.array(m.field(WHITE, 10)))
    h.set_white_config({"max_radius": 5.0})
    h.step(1 / 60, 2, 3)
    t = h.download(WHITE, "mass_t")
    assert np.array_equal(h.download(WHITE, "radius"), 4 * (1 - t) + 5.0 * t)  # mix(min_radius, max_radius, t), M:33-35


def test_mode_switches(egg):
    h, m = _pair(egg, relaxed=False)
    centers, ids = _four_batches(h, m)
    k = 0
    for order in ("exact", "relaxed", "exact"):
        h.set_solver_order(order)
        m.relaxed = order == "relaxed"
        for _ in range(5):
            _step_both(h, m, ids, centers, k)
            k += 1
        _assert_same(h, m, ids, "after %s" % order)
    assert h.stats()["relaxed_steps"] == 5
    # a handle back in exact order steps like a fresh handle that imported the same batches: no stale tiling survives
    fresh = egg.SimulationHandler()
    fresh_ids = [fresh.import_batch(*h.export_batch(i)) for i in ids]
    for kk in range(k, k + 4):
        for hh, hids in ((h, ids), (fresh, fresh_ids)):
            for i, c in zip(hids, centers):
                hh.set_target_position(i, *circle_target(c, kk))
            hh.step(1 / 60, 2, 3)
    for w in (WHITE, YOLK):
        assert np.array_equal(_dev_state(h, w), _dev_state(fresh, w))


def test_bad_positions_fail_without_commit(egg):
    h = egg.SimulationHandler()
    h.set_solver_order("relaxed")
    h.add(1.0e12, 0.0, 50, 15)  # its cells lie beyond +-2^30
    before = _dev_state(h, WHITE)
    with pytest.raises(egg.EggError, match="relaxed order"):
        h.step(1 / 60, 2, 3)
    assert np.array_equal(_dev_state(h, WHITE), before, equal_nan=True)
    assert h.stats()["steps"] == 0
    # a NaN position, brought in through import_batch
    src = egg.SimulationHandler()
    i = src.add(300.0, 300.0, 50, 15)
    info, ws, ys = src.export_batch(i)
    ws[0, 3] = float("nan")
    g = egg.SimulationHandler()
    g.set_solver_order("relaxed")
    g.import_batch(info, ws, ys)
    before = _dev_state(g, WHITE)
    with pytest.raises(egg.EggError, match="relaxed order"):
        g.step(1 / 60, 2, 3)
    assert np.array_equal(_dev_state(g, WHITE), before, equal_nan=True)


def _cells(x, y, cell):
    return np.floor(x / cell).astype(np.int64), np.floor(y / cell).astype(np.int64)


def test_full_size_config3_sites(egg):
    """BASELINE config 3 (4,096 batches, 4 coincident per site, sites 400 px apart) in relaxed order.  A site's result
    cannot depend on the rest of the scene while no particle comes within one cell of another site's (asserted from the
    downloaded positions), so 8 sites are checked against the model run on that site alone, at the same coordinates."""
    xs, ys, side = bench.grid_positions(4096, overlap=4)
    steps = 20
    hs = []
    for _ in range(2):
        h = egg.SimulationHandler()
        h.set_solver_order("relaxed")
        ids = h.add_many(xs, ys, 50, 15)
        for _ in range(steps):
            assert h.update(1 / 60) == 1
        hs.append((h, ids))
    h, ids = hs[0]
    for w in (WHITE, YOLK):  # two handles, identical arrays
        assert np.array_equal(_dev_state(h, w), _dev_state(hs[1][0], w))
    nw, ny = h.get_n_particles(int(ids[0]))
    n_sites = 4096 // 4
    cell = {WHITE: 8.0, YOLK: 12.0}  # max(1, max_radius * max(overlap factor, cohesion factor)), L:1756-1760
    # site separation: per type, every site's cell box at least 2 cells (plus one of margin) away from every other's
    for w, per in ((WHITE, nw), (YOLK, ny)):
        cx, cy = _cells(h.download(w, "x"), h.download(w, "y"), cell[w])
        cx, cy = cx.reshape(n_sites, 4 * per), cy.reshape(n_sites, 4 * per)
        lo_x, hi_x, lo_y, hi_y = cx.min(1), cx.max(1), cy.min(1), cy.max(1)
        gap_x = np.maximum(lo_x[:, None] - hi_x[None, :], lo_x[None, :] - hi_x[:, None])
        gap_y = np.maximum(lo_y[:, None] - hi_y[None, :], lo_y[None, :] - hi_y[:, None])
        gap = np.maximum(gap_x, gap_y)
        np.fill_diagonal(gap, 1 << 30)
        assert int(gap.min()) >= 3, "sites came within reach of each other (type %d)" % w
    sites = sorted({0, side - 1, n_sites - side, n_sites - 1, 1, side + 1, n_sites // 2 + 3, n_sites // 3})
    assert len(sites) == 8
    for site in sites:
        m = RelaxedModel(relaxed=True)
        for b in range(4):
            m.add(float(xs[4 * site + b]), float(ys[4 * site + b]), 50, 15)
        for _ in range(steps):
            m.update(1 / 60, 1 / 60, 2, 3)
        for w, per in ((WHITE, nw), (YOLK, ny)):
            sl = slice(4 * site * per, 4 * (site + 1) * per)
            dev, ref = _dev_state(h, w)[:, sl], m.state(w)
            for k, f in enumerate(FIELDS):
                assert np.array_equal(dev[k], ref[k]), "site %d type %d field %s" % (site, w, f)
        for b in range(4):
            assert h.get_position(int(ids[4 * site + b])) == tuple(m.get_position(b + 1))
