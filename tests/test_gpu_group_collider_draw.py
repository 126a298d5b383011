"""Colliders in the picture on a device group ("Collider styles"): egg_group_render draws handle 0's
list and styles, egg_group_get_collider_pose mixes handle 0's two lists at the group's alpha.  A group of 2 and of 3 handles
on one device plays the egg scene of tests/collider_draw_model.py, with a cut between two eggs and the disc moving;
whatever it draws or returns equals ONE SimulationHandler's, bit for bit -- and that handler's styled image is held against
the numpy model in tests/test_gpu_collider_draw.py."""
import numpy as np
import pytest

import collider_draw_model as cdm

pytestmark = pytest.mark.gpu

INF = float("inf")
EGGS = (cdm.EGG["at"], cdm.EGG_SECOND)


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


@pytest.fixture(scope="module")
def one_handle(egg):
    h = egg.SimulationHandler()
    cdm.play_egg_scene(h, EGGS, cdm.EGG_DISC_MOTION)
    assert 0.0 < h.interpolation_alpha < 1.0
    last, cur = h.get_collider_pose(0.0), h.get_colliders()
    assert last != cur  # the disc has moved: the pose is a mix
    out = cdm.probe_egg_scene(h)
    # the chain ends at the model: the over layer on the plain draw's pixels the under layer left alone is checked in
    # test_gpu_collider_draw.py; here the poses against the model's
    own = h.interpolation_alpha
    assert out["poses"] == [cdm.pose(last, cur, t) for t in (0.0, cdm.EGG_VIEW["alpha"], 1.0, 1.7, own)]
    assert not np.array_equal(out["plain"], out["styled"]) and not np.array_equal(out["styled"], out["styled, own alpha"])
    return out


def same(a, b):
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    if isinstance(a, (list, tuple)) and a and isinstance(a[-1], np.ndarray):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


@pytest.mark.parametrize("cuts", [[-INF, cdm.EGG_CUT, INF], [-INF, cdm.EGG_CUT, 400.0, INF]], ids=["2 handles", "3 handles"])
def test_a_group_draws_and_poses_as_one_handle(egg, one_handle, cuts):
    g = egg.SimulationGroup([0] * (len(cuts) - 1), cuts=cuts)
    cdm.play_egg_scene(g, EGGS, cdm.EGG_DISC_MOTION)
    assert [g.owner(i)[0] for i in g.list_ids()] == [0, 1]  # an egg on each side of the cut
    got = cdm.probe_egg_scene(g)
    assert sorted(got) == sorted(one_handle)
    for key, want in one_handle.items():
        assert same(got[key], want), key
    # a refused call changes no handle
    g.set_collider_styles(cdm.EGG_STYLES_UNDER)
    with pytest.raises(egg.EggError, match="n = 2, the list holds 3"):
        g.set_collider_styles([None, None])
    assert g.get_collider_styles() == [h.get_collider_styles() for h in g.handles][0] == [h.get_collider_styles() for h in g.handles][-1]
    assert [s["layer"] for s in g.get_collider_styles()] == ["under"] * 3
    g.close()
