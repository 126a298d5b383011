"""The collider records on the device depend on the settings in force, not on the order in which they were reached
("The collider tables on the device").

Every case builds handle A by walking a sequence of setter calls and handle B by setting, on a fresh handle, the state A
reports at the end of the walk; both then hold the same batch, run two steps (n_substeps = 2, n_collision_steps = 3), and
must agree bit for bit: x, y, vx, vy, last_x, last_y of every particle, get_colliders(), get_collider_motion(),
get_collider_spin(), collider_hits(), collider_grips() and collider_load_sums().  A walk is made twice: "plain", setter after
setter, and "stepped", with one committed step of the still empty handle behind every setter -- a step is what carries
a table to the device, so only the stepped walk leaves the tables of the intermediate settings there.  (In the stepped walk
moving and turning colliders advance during the walk: B starts from the list, the motions and the pivots A has arrived at.)
The first sequence's B is also compared with tests/spin_model.py, so the file is anchored to the model and not only to the
code under test.

The scene: one batch of 64 + 3 white particles (one full wave and a ragged one) and 5 yolk particles at (300, 300), and
three colliders placed so that particles touch each: a half-plane from above, a disc inside the white, and a wall (or, in
the lists without a wall, a segment in its place) through the yolk.

A step that is not committed: collider bodies run on one handle only, and egg_step_begin / egg_rx_begin refuse such a
handle in relaxed order, so the one step with bodies that can end without a commit is a failed one -- a batch with a NaN
position, as in test_gpu_collider_bodies.py::test_a_failed_step_advances_nothing."""
import numpy as np
import pytest

from relaxed_model import rm
from spin_model import SpinModel
from test_gpu_collider_surfaces import FIELDS, _assert_snapshot, _snapshot
from test_gpu_collider_walls import CUTS

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
S, C = 2, 3
H60 = 1 / 60
BATCH = (300.0, 300.0, 50, 15, None, None, 67, 5)
PLANE = ("half_plane", 0.0, 1.0, 262.0)         # keeps y - 262 >= radius: the top of the white
DISC = ("disc", 272.0, 322.0, 14.0)             # inside the white
WALL = ("wall", 306.0, 250.0, 306.0, 350.0)     # through the yolk
SEGMENT = ("segment",) + WALL[1:]
LIST, NO_WALL = [PLANE, DISC, WALL], [PLANE, DISC, SEGMENT]
# (the half-plane moves and does not turn: a turned normal read back and set again would be normalised a second time)
SPINS = [None, (285.0, 330.0, -3.0), (306.0, 300.0, 1.5)]
PIVOTS = [None, (285.0, 330.0, 0.0), (306.0, 300.0, 0.0)]
MOTIONS = [(0.0, 30.0), (40.0, -20.0), (-60.0, 0.0)]
SURFACES = [(0.4, 10.0, 0.0), 0.3, (0.2, -5.0, 5.0)]
BODIES = [None, (1.0 / 40.0, 1.0 / 2880.0, 0.0, 400.0, 0.125, 0.5), None]

# name: the walk, setter after setter, behind set_solver_order("relaxed")
WALKS = {
    "spin_motion_cleared": [("set_colliders", LIST), ("set_collider_spin", SPINS), ("set_collider_motion", MOTIONS), ("set_collider_motion", [])],
    "motion_spin_cleared": [("set_colliders", LIST), ("set_collider_motion", MOTIONS), ("set_collider_spin", SPINS), ("set_collider_spin", [])],
    "surfaces_spin_surfaces_cleared": [("set_colliders", LIST), ("set_collider_surfaces", SURFACES), ("set_collider_spin", SPINS),
                                       ("set_collider_surfaces", [])],
    "loads_pivots_spin": [("set_colliders", NO_WALL), ("set_collider_loads", True), ("set_collider_spin", PIVOTS), ("set_collider_spin", SPINS)],
    "wall_list_replaced_under_motion": [("set_colliders", LIST), ("set_collider_motion", MOTIONS), ("set_colliders", NO_WALL),
                                        ("set_collider_motion", MOTIONS)],
}
# ... and what the plain walk leaves in force: (colliders, surfaces, motions, spins, loads), None = never set or cleared
FINAL = {
    "spin_motion_cleared": (LIST, None, None, SPINS, False),
    "motion_spin_cleared": (LIST, None, MOTIONS, None, False),
    "surfaces_spin_surfaces_cleared": (LIST, None, None, SPINS, False),
    "loads_pivots_spin": (NO_WALL, None, None, SPINS, True),
    "wall_list_replaced_under_motion": (NO_WALL, None, MOTIONS, None, False),
}


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _fresh(egg, group=False):
    h = egg.SimulationGroup([0, 0], cuts=CUTS[2]) if group else egg.SimulationHandler()
    h.set_solver_order("relaxed")
    return h


def _records(h):
    return dict(colliders=h.get_colliders(), surfaces=h.get_collider_surfaces(), motions=h.get_collider_motion(), spins=h.get_collider_spin(),
                loads=h.get_collider_loads_enabled(), bodies=h.get_collider_bodies())


def _set_records(h, r):
    """the state r, set directly"""
    h.set_colliders(r["colliders"])
    h.set_collider_surfaces(r["surfaces"])
    h.set_collider_motion(r["motions"])
    h.set_collider_spin(r["spins"])
    h.set_collider_loads(r["loads"])
    h.set_collider_bodies(r["bodies"])
    return h


def _as_stored(final):
    """what the getters return for the state `final` names"""
    colliders, surfaces, motions, spins, loads = final
    n = len(colliders)
    return dict(colliders=[tuple(c) + ("both",) for c in colliders],
                surfaces=[(0.0, 0.0, 0.0)] * n if surfaces is None else [(s, 0.0, 0.0) if isinstance(s, float) else tuple(s) for s in surfaces],
                motions=[(0.0, 0.0)] * n if motions is None else [tuple(m) for m in motions],
                spins=[(0.0, 0.0, 0.0)] * n if spins is None else [(0.0, 0.0, 0.0) if s is None else tuple(s) for s in spins],
                loads=loads, bodies=[(0.0,) * 6] * n)


def _bits(h, i):
    """the particle fields of batch i as integers: a comparison bit for bit, a NaN or a zero's sign included"""
    if hasattr(h, "handles"):
        return [[np.array(h.particles(w, FIELDS)[i][k]).view(np.uint64).tolist() for k in range(len(FIELDS))] for w in (WHITE, YOLK)]
    return [[h.download(w, f).view(np.uint64).tolist() for f in FIELDS] for w in (WHITE, YOLK)]


def _observe(h, i):
    return dict(particles=_bits(h, i), colliders=h.get_colliders(), motions=h.get_collider_motion(), spins=h.get_collider_spin(),
                hits=h.collider_hits(), grips=h.collider_grips(), sums=h.collider_load_sums())


def _two_steps(h, i, since=None):
    """two steps; the observation after each, the counters since `since`"""
    out = []
    for _ in range(2):
        h.step(H60, S, C)
        o = _observe(h, i)
        if since is not None:
            o["hits"] = [a - b for a, b in zip(o["hits"], since["hits"])]
            o["grips"] = [a - b for a, b in zip(o["grips"], since["grips"])]
        out.append(o)
    return out


def _assert_equal_runs(a, b, what):
    for k, (oa, ob) in enumerate(zip(a, b)):
        for key in ("colliders", "motions", "spins", "hits", "grips", "sums", "particles"):
            assert oa[key] == ob[key], "%s: step %d: %s differs" % (what, k + 1, key)
    assert sum(a[-1]["hits"]) > 0, what  # (the colliders did something)


def _walk(h, calls, stepped):
    for name, arg in calls:
        getattr(h, name)(arg)
        if stepped:
            h.step(H60, S, C)
    return h


@pytest.mark.parametrize("stepped", [False, True], ids=["plain", "stepped"])
@pytest.mark.parametrize("name", sorted(WALKS))
def test_a_walk_ends_where_the_direct_setting_starts(egg, name, stepped):
    a = _walk(_fresh(egg), WALKS[name], stepped)
    reached = _records(a)
    if not stepped:
        assert reached == _as_stored(FINAL[name])
    else:  # (the empty steps of the walk have advanced what moves and turns, and nothing else)
        want = _as_stored(FINAL[name])
        assert [c[0] for c in reached["colliders"]] == [c[0] for c in want["colliders"]]
        assert (reached["surfaces"], reached["motions"], [s[2] for s in reached["spins"]], reached["loads"]) == \
               (want["surfaces"], want["motions"], [s[2] for s in want["spins"]], want["loads"])
    b = _set_records(_fresh(egg), reached)
    assert _records(b) == reached
    i = a.add(*BATCH)
    assert b.add(*BATCH) == i and tuple(a.get_n_particles()) == tuple(b.get_n_particles()) == (67, 5)
    run_a, run_b = _two_steps(a, i), _two_steps(b, i)
    _assert_equal_runs(run_a, run_b, name)
    if name == "loads_pivots_spin":  # particles touch each of the three colliders: each has received a load in the first step
        sums = run_b[0]["sums"][0]
        assert len(sums) == 3 and all(any(v != 0 for v in one) for one in sums), sums
    if name == "spin_motion_cleared" and not stepped:
        _assert_the_model(b, i)


def _assert_the_model(b, i):
    """B of the first sequence after its two steps against tests/spin_model.py, as test_gpu_collider_spin.py compares"""
    w, y = rm.default_configs()
    m = SpinModel(w, y, cohesion=False)
    m.set_colliders(list(LIST))
    m.set_collider_spin(list(SPINS))
    assert m.add(*BATCH[:4], *BATCH[6:]) == i
    for _ in range(2):
        m.update(H60, H60, S, C)
    _assert_snapshot(b, _snapshot(m, [i]), "the directly set handle against the model")
    assert [tuple(c) for c in b.get_colliders()] == [tuple(c) for c in m.get_colliders()]
    assert [tuple(s) for s in b.get_collider_spin()] == [tuple(s) for s in m.get_collider_spin()]
    assert sum(m.wall_catches) > 0 and m.collider_hits[WHITE] > 0 and m.collider_hits[YOLK] > 0


# ------------------------------------------------------------------------------------------------ collider bodies
def _with_bodies(egg):
    h = _fresh(egg)
    h.set_colliders(LIST)
    h.set_collider_surfaces(SURFACES)
    h.set_collider_motion(MOTIONS)
    h.set_collider_spin(SPINS)
    h.set_collider_loads(True)
    h.set_collider_bodies(BODIES)
    return h


def test_a_step_that_is_not_committed_leaves_no_trace(egg):
    """bodies on, one step that fails, then two committed steps: as on a handle that never ran the failed step"""
    src = egg.SimulationHandler()
    src.add(*BATCH)
    j = src.add(330.0, 100.0, 50, 15)
    info, ws, ys = src.export_batch(j)
    ws[0, 7] = float("nan")
    a, b = _with_bodies(egg), _with_bodies(egg)
    i = a.add(*BATCH)
    assert b.add(*BATCH) == i
    held = _records(a)
    assert a.import_batch(info, ws, ys) == j
    with pytest.raises(egg.EggError, match="relaxed order: a position is NaN"):
        a.step(H60, S, C)
    a.remove(j)
    assert _records(a) == held
    run_a, run_b = _two_steps(a, i), _two_steps(b, i)
    _assert_equal_runs(run_a, run_b, "after a failed step")
    assert run_b[-1]["motions"][1] != held["motions"][1] and run_b[-1]["spins"][1][2] != held["spins"][1][2]  # (the body has been pushed)


def test_bodies_cleared_leave_the_motion_and_spin_the_commit_took(egg):
    """bodies on for a step, then cleared: the next steps run on the list, the motions and the spins that step has left, as on
    a fresh handle that is given them and the step's particles"""
    a = _with_bodies(egg)
    i = a.add(*BATCH)
    before = _records(a)
    a.step(H60, S, C)
    a.set_collider_bodies([])
    reached = _records(a)
    assert reached["motions"][1] != before["motions"][1] and reached["colliders"] != before["colliders"] and reached["bodies"] == [(0.0,) * 6] * 3
    info, ws, ys = a.export_batch(i)
    b = _set_records(_fresh(egg), reached)
    assert b.import_batch(info, ws, ys) == i and _records(b) == reached
    assert _bits(a, i) == _bits(b, i)
    run_a, run_b = _two_steps(a, i, since=_observe(a, i)), _two_steps(b, i)
    _assert_equal_runs(run_a, run_b, "bodies cleared")


# ------------------------------------------------------------------------------------------------ device groups
@pytest.mark.parametrize("name", ["spin_motion_cleared", "motion_spin_cleared"])
def test_a_group_walks_alike_and_a_refused_call_changes_nothing(egg, name):
    """two handles; in the middle of the walk a spin list of the wrong length is refused: the group then equals one that never
    made the call, and one handle"""
    calls = WALKS[name]
    a = _walk(_fresh(egg, group=True), calls[:2], False)
    held = _records(a), [_records(h) for h in a.handles]
    with pytest.raises(egg.EggError, match="n = 2, the list holds 3"):
        a.set_collider_spin(SPINS[:2])
    assert (_records(a), [_records(h) for h in a.handles]) == held
    _walk(a, calls[2:], False)
    never = _walk(_fresh(egg, group=True), calls, False)
    b = _set_records(_fresh(egg, group=True), _as_stored(FINAL[name]))
    one = _set_records(_fresh(egg), _as_stored(FINAL[name]))
    assert _records(a) == _records(never) == _records(b) == _as_stored(FINAL[name])
    i = a.add(*BATCH)
    assert never.add(*BATCH) == b.add(*BATCH) == one.add(*BATCH) == i
    run_a, run_never, run_b, run_one = (_two_steps(h, i) for h in (a, never, b, one))
    _assert_equal_runs(run_a, run_never, name + ": the group that never made the refused call")
    _assert_equal_runs(run_a, run_b, name + ": the group set directly")
    _assert_equal_runs(run_a, run_one, name + ": one handle")
    for h in a.handles:
        assert (h.get_colliders(), h.get_collider_motion(), h.get_collider_spin()) == \
               (run_a[-1]["colliders"], run_a[-1]["motions"], run_a[-1]["spins"])
