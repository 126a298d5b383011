"""Every instantiation of the relaxed collision pass's gather, run: the seven flavours a collider list can select -- none,
colliders, surfaces, walls, motion, spin, loads -- without and with effective cohesion, each on a single SimulationHandler
(the plain instantiations) and on a SimulationGroup of two handles on device 0 (the group instantiations): 28 kernels.

The scene is small: four overlapping batches of a few dozen particles astride the group's cut, S = 2, C = 2, three steps.
The collider list of a flavour is the least that selects it, each adding to the one before: a half-plane; a friction; a
wall; a motion that is not zero; a spin that is not zero; loads on.  Compared, group against handle: x, y, vx, vy of every
particle bit for bit, hits, grips, cohesion solves, pair solves and the raw load sums; and the launches of a step against
the counts test_gpu_relaxed.py and test_gpu_group_relaxed.py state in their test_launches_of_one_step."""
import math

import numpy as np
import pytest

from conftest import circle_target

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
S, C, STEPS = 2, 2, 3
INF = math.inf
CUT = 300.0
CENTERS = ((272.0, 300.0), (296.0, 308.0), (309.0, 294.0), (333.0, 303.0))  # two either side of the cut, all overlapping
RADII, COUNTS = (30.0, 10.0), (48, 24)  # white and yolk: radius of the disc a batch is spread over, particles
WHITE3 = dict(cohesion_interaction_distance_factor=3, cohesion_strength=0.99)
EDGE = ("half_plane", 1.0, 0.0, 262.0)  # x >= 262: the leftmost batch reaches to x = 242, so the plane always has work
GATE = ("wall", 200.0, 322.0, 400.0, 318.0)  # under the cluster's middle, across the cut
FIELDS = ("x", "y", "vx", "vy")
# flavour: (colliders, surfaces, motions, spins, loads), each the one before and one thing more
FLAVOURS = {
    "none": ((), None, None, None, False),
    "col": ((EDGE,), None, None, None, False),
    "srf": ((EDGE,), (0.3,), None, None, False),
    "wall": ((EDGE, GATE), (0.3, None), None, None, False),
    "mov": ((EDGE, GATE), (0.3, None), ((12.0, 0.0), None), None, False),
    "spin": ((EDGE, GATE), (0.3, None), ((12.0, 0.0), None), (None, (300.0, 320.0, 0.4)), False),
    "load": ((EDGE, GATE), (0.3, None), ((12.0, 0.0), None), (None, (300.0, 320.0, 0.4)), True),
}


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _configure(o, flavour, cohesion):
    colliders, surfaces, motions, spins, loads = FLAVOURS[flavour]
    o.set_solver_order("relaxed")
    if cohesion:
        o.set_white_config(WHITE3)
        o.set_cohesion("effective")
    o.set_colliders(list(colliders))
    if surfaces is not None:
        o.set_collider_surfaces(list(surfaces))
    if motions is not None:
        o.set_collider_motion(list(motions))
    if spins is not None:
        o.set_collider_spin(list(spins))
    if loads:
        o.set_collider_loads(True)
    return o


@pytest.mark.parametrize("cohesion", [False, True], ids=["plain", "cohesive"])
@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_group_equals_handle(egg, flavour, cohesion):
    h = _configure(egg.SimulationHandler(), flavour, cohesion)
    g = _configure(egg.SimulationGroup([0, 0], cuts=[-INF, CUT, INF]), flavour, cohesion)
    ids = [h.add(x, y, *RADII, None, None, *COUNTS) for x, y in CENTERS]
    assert [g.add(x, y, *RADII, None, None, *COUNTS) for x, y in CENTERS] == ids
    owners = [g.owner(i)[0] for i in ids]
    assert sorted(set(owners)) == [0, 1]
    for k in range(STEPS):
        for i, c in zip(ids, CENTERS):
            t = circle_target(c, k)
            h.set_target_position(i, *t)
            g.set_target_position(i, *t)
        before = h.stats()["kernel_launches"], [b.stats()["kernel_launches"] for b in g.handles]
        h.step(1 / 60, S, C)
        g.step(1 / 60, S, C)
    what = "%s, %s" % (flavour, "cohesive" if cohesion else "plain")

    # the launches of the last step (the first also builds the atom and key tables): what the two tests of that name count
    assert [g.owner(i)[0] for i in ids] == owners  # (nothing migrated: the handles hold what they held)
    held = [b.get_n_particles() for b in g.handles]
    assert all(n > 0 for n in h.get_n_particles()) and all(n[w] > 0 for n in held for w in (WHITE, YOLK))
    delta = h.stats()["kernel_launches"] - before[0]
    deltas = [b.stats()["kernel_launches"] - n for b, n in zip(g.handles, before[1])]
    print("%s: launches of a step: handle %d, group %s" % (what, delta, deltas))
    assert delta == 2 * (S + 5 * S * C + 1), what
    # per handle and type the single handle's count, a pack and an unpack per pass (both handles hold both types), and the
    # stray rule's centroid launch of a handle that owns batches
    assert deltas == [2 * (S + 5 * S * C + 1 + 2 * S * C) + 1] * 2, what

    for w in (WHITE, YOLK):
        got = g.particles(w, FIELDS)
        cat = np.concatenate([np.array(got[i]) for i in sorted(got)], axis=1)
        for q, f in enumerate(FIELDS):
            assert np.array_equal(cat[q], h.download(w, f)), "%s: type %d field %s" % (what, w, f)
    hs, gs = h.stats(), [b.stats() for b in g.handles]
    counts = dict(hits=h.collider_hits(), grips=h.collider_grips(), cohered=hs["cohesion_solves"], pairs=hs["pair_solves"],
                  loads=h.collider_load_sums())
    print("%s: %s" % (what, counts))
    assert g.collider_hits() == counts["hits"] and g.collider_grips() == counts["grips"], what
    assert sum(s["cohesion_solves"] for s in gs) == counts["cohered"], what
    assert sum(s["pair_solves"] for s in gs) == counts["pairs"] > 0, what
    assert g.collider_load_sums() == counts["loads"], what
    # the scene exercises what the flavour adds: the plane always has particles to move; sums only with loads on
    colliders, loads = FLAVOURS[flavour][0], FLAVOURS[flavour][4]
    assert (sum(counts["hits"]) > 0) == bool(colliders), what
    assert (counts["loads"][2] > 0.0) == loads, what
    assert (counts["cohered"] > 0) == cohesion, what
