"""Relaxed order on a device group (egg_group_set_solver_order, DESIGN.md section 2.7 "Several devices"): every pass
runs on every handle over its own particles plus ghosts of its neighbours', and the group gives ONE relaxed handle's
results bit for bit.  All groups here are several handles on GPU 0.  The single relaxed handle is pinned to the CPU
model by tests/test_gpu_relaxed.py; one scene is also held against the model directly."""
import math

import numpy as np
import pytest

from conftest import circle_target, load_golden
from relaxed_model import RelaxedModel

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
FIELDS = ("x", "y", "vx", "vy", "last_x", "last_y")
INF = math.inf


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _pair(egg, cuts, omega=None):
    g = egg.SimulationGroup([0] * (len(cuts) - 1), cuts=cuts)
    g.set_solver_order("relaxed", omega)
    h = egg.SimulationHandler()
    h.set_solver_order("relaxed", omega)
    return g, h


def _single_batches(h, w):
    """{id: fields[6, n]} of one handle (batches laid out in ascending id)"""
    cols = np.array([h.download(w, f) for f in FIELDS])
    out, off = {}, 0
    for i in sorted(h.list_ids()):
        n = h.get_n_particles(i)[w]
        out[i] = cols[:, off:off + n]
        off += n
    return out


def _assert_same(g, h, what=""):
    for w in (WHITE, YOLK):
        got = g.particles(w, FIELDS)
        ref = _single_batches(h, w)
        assert sorted(got) == sorted(ref), what
        for i in ref:
            for k, f in enumerate(FIELDS):
                assert np.array_equal(got[i][k], ref[i][k]), "%s type %d batch %d field %s" % (what, w, i, f)
    for i in sorted(h.list_ids()):
        assert g.get_position(i) == h.get_position(i), "%s position %d" % (what, i)
    assert sum(b.stats()["pair_solves"] for b in g.handles) == h.stats()["pair_solves"], what


def _add_both(g, h, centers, *more):
    ids = [g.add(x, y, *more) for x, y in centers]
    assert [h.add(x, y, *more) for x, y in centers] == ids
    return ids


def _step_both(g, h, S=2, C=3):
    g.step(1 / 60, S, C)
    h.step(1 / 60, S, C)


def _move_both(g, h, i, x, y):
    g.set_target_position(i, x, y)
    h.set_target_position(i, x, y)


CUTS = {2: [-INF, 10.0, INF], 3: [-INF, -5.0, 25.0, INF]}


@pytest.mark.parametrize("omega", [1.0, 1.8])
@pytest.mark.parametrize("S,C", [(2, 3), (1, 1), (3, 2)])
@pytest.mark.parametrize("n_handles", [2, 3])
def test_four_batches_across_cuts(egg, n_handles, S, C, omega):
    centers = [tuple(c) for c in load_golden("four_batches")["centers"]]
    g, h = _pair(egg, CUTS[n_handles], omega)
    ids = _add_both(g, h, centers, 50, 15)
    assert len({g.owner(i)[0] for i in ids}) >= 2  # the cluster is cut
    for k in range(30):
        for i, c in zip(ids, centers):
            _move_both(g, h, i, *circle_target(c, k))
        _step_both(g, h, S, C)
    _assert_same(g, h, "n=%d S=%d C=%d omega=%g" % (n_handles, S, C, omega))
    hc = g.halo_counters()
    assert hc["passes"] == 30 * S * C and hc["records"] > 0 and hc["bytes"] == 40 * hc["records"]
    assert g.counters()["discarded_steps"] == 0


@pytest.mark.parametrize("S,C", [(2, 3), (1, 1)])
@pytest.mark.parametrize("n_handles", [2, 3])
def test_launches_of_one_step(egg, n_handles, S, C):
    """The launch sequence of a relaxed group step, counted per handle: per type the handle holds, the single handle's
    S + 5 S C + 1 (begin / mid, five launches per pass, end) and, when another handle holds the type too, one pack and
    one unpack launch per pass.  The group's step then reads the batch positions of every handle that owns batches for
    its stray rule: one centroid launch (egg_get_positions_many).  Taken over the second step: the first also builds
    the atom and key tables."""
    centers = [tuple(c) for c in load_golden("four_batches")["centers"]]
    g, h = _pair(egg, CUTS[n_handles])
    ids = _add_both(g, h, centers, 50, 15)
    for i, c in zip(ids, centers):
        _move_both(g, h, i, *circle_target(c, 0))
    g.step(1 / 60, S, C)
    owners = [g.owner(i)[0] for i in ids]
    before = [b.stats()["kernel_launches"] for b in g.handles]
    for i, c in zip(ids, centers):
        _move_both(g, h, i, *circle_target(c, 1))
    g.step(1 / 60, S, C)
    assert [g.owner(i)[0] for i in ids] == owners  # (nothing migrated: the handles hold what they held)
    delta = [b.stats()["kernel_launches"] - n for b, n in zip(g.handles, before)]
    held = [b.get_n_particles() for b in g.handles]
    print("group of %d S=%d C=%d: launches %s, particles %s" % (n_handles, S, C, delta, held))
    assert sum(1 for n in held if n[WHITE] > 0) >= 2
    for k, b in enumerate(g.handles):
        want = 1 if k in owners else 0  # the stray rule's centroid launch
        for w in (WHITE, YOLK):
            if held[k][w] > 0:
                shared = sum(1 for n in held if n[w] > 0) > 1
                want += S + 5 * S * C + 1 + (2 * S * C if shared else 0)
        assert delta[k] == want, "handle %d" % k


def test_group_matches_the_model(egg):
    centers = [tuple(c) for c in load_golden("four_batches")["centers"]]
    g = egg.SimulationGroup([0, 0, 0], cuts=CUTS[3])
    g.set_solver_order("relaxed")
    m = RelaxedModel(relaxed=True)
    ids = [g.add(x, y, 50, 15) for x, y in centers]
    assert [m.add(x, y, 50, 15) for x, y in centers] == ids
    for k in range(12):
        for i, c in zip(ids, centers):
            t = circle_target(c, k)
            g.set_target_position(i, *t)
            m.set_target_position(i, *t)
        g.step(1 / 60, 2, 3)
        m.update(1 / 60, 1 / 60, 2, 3)
    for w in (WHITE, YOLK):
        got = g.particles(w, FIELDS)
        ref = m.state(w)
        cat = np.concatenate([np.array(got[i]) for i in sorted(got)], axis=1)
        for k, f in enumerate(FIELDS):
            assert np.array_equal(cat[k], ref[k]), (w, f)
    assert sum(b.stats()["pair_solves"] for b in g.handles) == m.pair_solves


def test_global_key_in_the_coincident_normal(egg):
    # batches 1 and 3 coincide in slab 0, batch 2 sits in slab 1: on device 0 the local index difference of a coincident
    # pair (1 batch apart) is not the global one (2 batches apart)
    g, h = _pair(egg, [-INF, 120.0, INF], 1.0)
    ids = _add_both(g, h, [(100.0, 100.0), (140.0, 100.0), (100.0, 100.0)], 50, 15)
    assert [g.owner(i)[0] for i in ids] == [0, 1, 0]
    for _ in range(10):
        _step_both(g, h)
    _assert_same(g, h, "coincident")


def _pile(spacing=20.0, n=8, cx=0.0, cy=0.0):
    return [(cx + spacing * (i - (n - 1) / 2), cy + spacing * (j - (n - 1) / 2)) for i in range(n) for j in range(n)]


def test_dense_pile_on_a_cut(egg):
    g, h = _pair(egg, [-INF, -300.0, 0.0, 300.0, INF])
    _add_both(g, h, _pile(), 50, 15)
    for _ in range(20):
        _step_both(g, h)
    _assert_same(g, h, "pile")
    hc = g.halo_counters()
    assert hc["records"] > 0 and hc["bytes"] > 0 and hc["passes"] == 20 * 6
    # control: every batch far from every cut -> no ghosts at all
    g2, h2 = _pair(egg, [-INF, -1000.0, 0.0, 1000.0, INF])
    _add_both(g2, h2, [(-2000.0, 0.0), (-500.0, 0.0), (500.0, 0.0), (2000.0, 0.0)], 50, 15)
    for _ in range(5):
        _step_both(g2, h2)
    _assert_same(g2, h2, "control")
    assert g2.halo_counters()["records"] == 0 and g2.halo_counters()["passes"] == 5 * 6


def test_mutations_between_steps(egg):
    g, h = _pair(egg, [-INF, 60.0, INF])
    centers = [(0.0, 0.0), (40.0, 10.0), (80.0, 0.0), (100.0, 40.0)]
    ids = _add_both(g, h, centers, 50, 15)
    for _ in range(5):
        _step_both(g, h)
    _assert_same(g, h, "before mutations")
    g.remove(2)
    h.remove(2)
    for _ in range(3):
        _step_both(g, h)
    _assert_same(g, h, "after remove")
    assert _add_both(g, h, [(50.0, -20.0)], 50, 15) == [5]
    for _ in range(3):
        _step_both(g, h)
    _assert_same(g, h, "after add")
    assert g.owner(1)[0] == 0
    for k in range(40):  # batch 1 is driven across the cut, through the others, to the far side
        _move_both(g, h, 1, min(10.0 * k, 400.0), 0.0)
        _step_both(g, h)
    _assert_same(g, h, "after the crossing")
    assert g.counters()["migrations"] >= 1 and g.owner(1)[0] == 1
    assert g.counters()["discarded_steps"] == 0
    assert ids == [1, 2, 3, 4]


def test_mode_switches(egg):
    centers = [tuple(c) for c in load_golden("four_batches")["centers"]]
    g, h = _pair(egg, CUTS[2])
    ids = _add_both(g, h, centers, 50, 15)
    for k in range(10):
        for i, c in zip(ids, centers):
            _move_both(g, h, i, *circle_target(c, k))
        _step_both(g, h)
    _assert_same(g, h, "relaxed")
    assert g.counters()["discarded_steps"] == 0
    before = g.counters()
    g.set_solver_order("exact")
    h.set_solver_order("exact")
    assert g.get_solver_order() == "exact"
    for k in range(10, 20):
        for i, c in zip(ids, centers):
            _move_both(g, h, i, *circle_target(c, k))
        _step_both(g, h)
    _assert_same(g, h, "exact after relaxed")
    # the exact protocol hands the islands that span the cut over again
    assert g.counters()["migrations"] > before["migrations"] or g.counters()["discarded_steps"] > 0
    assert len({g.owner(i)[0] for i in ids[:3]}) == 1
    assert sum(b.stats()["relaxed_steps"] for b in g.handles) == 2 * 10


def _handle_state(g):
    return [np.array([b.download(w, f) for f in FIELDS]) for b in g.handles for w in (WHITE, YOLK)]


def test_bad_position_fails_on_every_handle_without_commit(egg):
    g, h = _pair(egg, [-INF, 10.0, INF])
    _add_both(g, h, [tuple(c) for c in load_golden("four_batches")["centers"]], 50, 15)
    for _ in range(3):
        _step_both(g, h)
    assert _add_both(g, h, [(1e12, 0.0)], 50, 15) == [5]
    assert g.owner(5)[0] == 1
    before = _handle_state(g)
    steps = [b.stats()["steps"] for b in g.handles]
    with pytest.raises(egg.EggError, match="relaxed order"):
        g.step(1 / 60, 2, 3)
    with pytest.raises(egg.EggError, match="relaxed order"):
        h.step(1 / 60, 2, 3)
    after = _handle_state(g)
    for a, b in zip(before, after):
        assert np.array_equal(a, b, equal_nan=True)  # last_x / last_y included
    assert [b.stats()["steps"] for b in g.handles] == steps
    g.remove(5)
    h.remove(5)
    for _ in range(3):
        _step_both(g, h)
    _assert_same(g, h, "after the failed step")


def test_surface(egg):
    g = egg.SimulationGroup([0, 0], cuts=[-INF, 0.0, INF])
    assert g.get_solver_order() == "exact"
    assert g.halo_counters() == dict(passes=0, records=0, bytes=0)
    for bad in ("fast", 1, None):
        with pytest.raises(egg.EggError):
            g.set_solver_order(bad)
    for bad in (0.0, -1.0, 2.5, float("nan"), float("inf")):
        with pytest.raises(egg.EggError):
            g.set_solver_order("relaxed", bad)
    assert g.get_solver_order() == "exact"
    lib = egg._ffi.load()
    assert lib.egg_group_set_solver_order(g._g, 7, -1.0) < 0
    assert lib.egg_group_set_solver_order(g._g, 1, float("nan")) < 0
    assert lib.egg_group_set_solver_order(g._g, 1, 2.5) < 0
    g.set_solver_order("relaxed", 1.2)
    assert g.get_solver_order() == "relaxed"
    for k in range(12):  # (twelve batches: the exact steps below stay clear of the yolk budget 0.05 N^2, L:1752-1753)
        g.add(-1800.0 + 330.0 * k, 0.0, 50, 15)
    with pytest.raises(egg.EggError):
        g.handles[0].step_begin(1 / 60, 2, 3)
    g.step(1 / 60, 2, 3)
    assert all(b.stats()["relaxed_steps"] == 1 for b in g.handles)
    g.set_solver_order("exact")
    assert g.get_solver_order() == "exact"
    g.step(1 / 60, 2, 3)
    assert all(b.stats()["relaxed_steps"] == 1 and b.stats()["steps"] == 2 for b in g.handles)
