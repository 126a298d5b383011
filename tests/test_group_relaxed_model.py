"""The relaxed pass split over device-group slabs with ghost halos (tests/group_relaxed_model.py)
equals the undivided pass bit for bit: the halo rule, on the CPU.  Also the group's relaxed-order interface.  No GPU."""
import inspect

import numpy as np
import pytest

from conftest import circle_target, load_golden
from group_relaxed_model import GroupRelaxedModel, decomposed_pass, ghosts_of
from relaxed_model import RelaxedModel, relaxed_pass

WHITE, YOLK = 0, 1
OVERLAP, COMPLIANCE = 2.0, (1 - (1 - 0.0025)) / (1 / 120) ** 2


def _drive(sim, centers, steps, S=2, C=3):
    ids = [sim.add(cx, cy, 50, 15) for cx, cy in centers]
    for k in range(steps):
        for i, c in zip(ids, centers):
            sim.set_target_position(i, *circle_target(c, k))
        sim.update(1 / 60, 1 / 60, S, C)
    return ids


@pytest.mark.parametrize("cuts", [[-np.inf, 10.0, np.inf], [-np.inf, -5.0, 25.0, np.inf]])
def test_cuts_through_four_batches_equal_one_model(cuts):
    centers = [tuple(c) for c in load_golden("four_batches")["centers"]]
    one, split = RelaxedModel(relaxed=True), GroupRelaxedModel(cuts, relaxed=True)
    _drive(one, centers, 6)
    _drive(split, centers, 6)
    for w in (WHITE, YOLK):
        assert np.array_equal(one.state(w), split.state(w))
    assert one.pair_solves == split.pair_solves
    assert split.ghost_records > 0  # the cuts run through the cluster: the halo was needed


def test_coincident_batches_across_a_cut_equal_one_model():
    # batches 1 and 3 at one site, batch 2 on the other side of the cut: the key difference of a coincident pair is not
    # its index difference inside either slab
    centers = [(100.0, 100.0), (140.0, 100.0), (100.0, 100.0)]
    one, split = RelaxedModel(relaxed=True, relaxation=1.0), GroupRelaxedModel([-np.inf, 120.0, np.inf], relaxed=True,
                                                                                relaxation=1.0)
    _drive(one, centers, 4)
    _drive(split, centers, 4)
    for w in (WHITE, YOLK):
        assert np.array_equal(one.state(w), split.state(w))
    assert one.pair_solves == split.pair_solves


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_partitions_equal_the_whole_pass(seed):
    rng = np.random.default_rng(seed)
    n = 400
    x, y = rng.uniform(0, 60, n), rng.uniform(0, 60, n)
    x[10:20], y[10:20] = x[5], y[5]  # coincident particles
    w = rng.uniform(0.5, 2.0, n)
    r = rng.uniform(1.0, 3.0, n)
    cell = 6.0
    cx, cy = np.floor(x / cell).astype(np.int64), np.floor(y / cell).astype(np.int64)
    owner = rng.integers(0, 4, n)
    ex, ey, ep = relaxed_pass(x, y, w, r, cx, cy, OVERLAP, COMPLIANCE, 1.8)
    gx, gy, gp, records = decomposed_pass(x, y, w, r, cx, cy, owner, OVERLAP, COMPLIANCE, 1.8, seed=seed)
    assert np.array_equal(ex, gx) and np.array_equal(ey, gy)
    assert ep == gp
    assert records > 0


def test_ghosts_are_the_grown_box():
    cx = np.array([0, 1, 2, 3, 5, 1])
    cy = np.array([0, 0, 0, 0, 0, 2])
    owner = np.array([0, 0, 1, 1, 1, 1])
    # owner 0 spans cells x 0..1, y 0: grown x -1..2, y -1..1 -> the particle in cell (2, 0) only
    assert list(np.flatnonzero(ghosts_of(owner, cx, cy, 0))) == [2]


def test_group_exposes_relaxed_order():
    from egg_fluid_simulation_amd import _ffi
    from egg_fluid_simulation_amd.group import SimulationGroup
    for name in ("egg_group_set_solver_order", "egg_group_get_halo_counters"):
        assert name in _ffi._SIGNATURES and name in _ffi.EXPORTED_SYMBOLS
    for meth in ("set_solver_order", "get_solver_order", "halo_counters"):
        assert callable(getattr(SimulationGroup, meth, None)), meth
    assert list(inspect.signature(SimulationGroup.set_solver_order).parameters) == ["self", "order", "relaxation"]


class _FakeHandle:
    def __init__(self, counts, x):
        self.counts, self.x = counts, np.asarray(x, dtype=np.float64)

    def download(self, which, field):
        return self.x if field == "x" else -self.x

    def get_n_particles(self, lid):
        return self.counts[lid], 0


def test_particles_skips_removed_ids():
    """particles() walks every id ever issued: a removed id in the middle does not hide the ones after it"""
    from egg_fluid_simulation_amd.group import SimulationGroup
    from egg_fluid_simulation_amd.simulation_handler import EggError
    g = SimulationGroup.__new__(SimulationGroup)
    owners = {1: (0, 1), 3: (0, 2), 4: (1, 1)}  # id 2 was removed

    def owner(gid):
        if gid not in owners:
            raise EggError("no batch")
        return owners[gid]

    g.owner = owner
    g._n_issued = 4
    g.handles = [_FakeHandle({1: 2, 2: 1}, [1.0, 2.0, 3.0]), _FakeHandle({1: 2}, [7.0, 8.0])]
    out = g.particles(WHITE)
    assert sorted(out) == [1, 3, 4]
    assert list(out[3][0]) == [3.0] and list(out[4][1]) == [-7.0, -8.0]
    g._g = None  # (nothing to destroy)
