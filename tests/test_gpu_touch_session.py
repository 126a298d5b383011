"""Touches across a session (egg_touches): the unit tables of a handle's touch state follow the atoms,
so every population change between two calls -- an add, a removal at the front, in the middle and at the end, an import in
front of everything, a hand-over to another handle and back -- is followed by a call whose answer is held against
tests/touch_model.py on the handle's downloads at that moment.  The sessions of tests/observer_session.py keep their batches
500 px apart, where nothing touches; this one keeps its eggs in a heap."""
import numpy as np
import pytest

import touch_model as tm
from test_gpu_probes import _relaxed_scene
from test_gpu_touches import _assert_touches, _rows

pytestmark = pytest.mark.gpu

H60, S, CS = 1 / 60, 2, 3
HEAP = [(300.0, 300.0), (340.0, 310.0), (320.0, 260.0), (380.0, 330.0), (290.0, 350.0)]
COUNTS = [(63, 15), (64, 15), (1025, 15), (65, 15), (64, 15)]  # white, yolk: the seams of a unit table


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _observe(h, what):
    """every live batch, then a listed call (reversed, one id twice) with another reach and mask: both against the model"""
    ids = h.list_ids()
    want = _assert_touches(h, None, None, "both", what)
    listed = ids[::-1] + ids[:1]
    _assert_touches(h, listed, (1.1, 3.0), "white", what + ", listed")
    assert {r[2] for r in want} <= set(ids)  # (no record names a batch that has left)
    return want


@pytest.mark.parametrize("order", ["exact", "relaxed"])
def test_touches_follow_the_population(egg, order):
    h = egg.SimulationHandler()
    if order == "relaxed":
        _relaxed_scene(h)
    ids = [h.add(x, y, 50, 15, None, None, nw, ny) for (x, y), (nw, ny) in zip(HEAP, COUNTS)]
    first = _observe(h, "five eggs in a heap")
    assert first and {r[2] for r in first} == set(ids)  # (every egg touches another)
    assert h.update(H60, H60, S, CS) == 1
    _observe(h, "after a step")
    h.remove(ids[2])  # a middle one, with more than 1,024 white particles ahead of survivors
    after = _observe(h, "the large middle egg removed")
    assert ids[2] not in {r[2] for r in after} and len(h.list_ids()) == 4
    with pytest.raises(egg.EggError, match="no batch with id `%d`" % ids[2]):
        h.touches([ids[0], ids[2]])
    h.remove(ids[0])  # the first one in layout order
    _observe(h, "the first egg removed")
    new = h.add(305.0, 305.0, 50, 15, None, None, 65, 15)  # a new id, appended
    assert new not in ids
    got = _observe(h, "an egg added where the first one lay")
    assert new in {r[2] for r in got}
    h.remove(ids[4])  # the last of the old ones
    _observe(h, "the last old egg removed")
    # a hand-over: the batch leaves for another handle and comes back in front of everything, by its key
    other = egg.SimulationHandler()
    if order == "relaxed":
        _relaxed_scene(other)
    info, ws, ys = h.export_batch(ids[1])
    h.remove(ids[1])
    gone = _observe(h, "an egg handed over")
    there = other.import_batch(info, ws, ys)
    assert _rows(other.touch_table()) == []  # (alone on its handle: it touches nothing)
    discs = (ws[[0, 1, 7]].T, ys[[0, 1, 7]].T)
    of = h.touches_of(discs, None, "both")
    info2, ws2, ys2 = other.export_batch(there)
    other.remove(there)
    back = h.import_batch(info2, ws2, ys2)
    assert h.list_ids()[0] == back or back in h.list_ids()
    again = _observe(h, "and taken back")
    assert len(again) > len(gone)
    # what the discs touched while the batch was away is what the batch touches now
    assert [[t[:4] for t in side] for side in of] == [[t[:4] for t in side] for side in h.touches([back])[0]]
    assert h.update(H60, H60, S, CS) == 1
    _observe(h, "after the last step")
    for i in h.list_ids():
        h.remove(i)
    assert h.touches() == [] and h.touch_table().shape == (0, 8)
    h.add(300.0, 300.0, 50, 15, None, None, 64, 15)
    assert _rows(h.touch_table()) == [] and h.touches() == [([], [])]


def test_the_model_is_evaluated_on_what_the_handle_holds(egg):
    """the comparison above reads batch_id from the handle: the layout after a removal is the handle's, not the test's"""
    h = egg.SimulationHandler()
    ids = [h.add(x, y, 50, 15, None, None, 20, 5) for x, y in HEAP[:3]]
    h.remove(ids[1])
    assert sorted(set(h.download(0, "batch_id").astype(np.int64).tolist())) == [ids[0], ids[2]]
    want = _assert_touches(h, None, 3.0, "both", "two of three")
    assert want and tm.contact(want[0]) is not None
