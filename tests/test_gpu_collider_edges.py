"""Steps 5b / 5c of the relaxed pass (rx_collide / rx_grip) on the device where the other device files do
not go: oblique walls, both sides of a wall, its ends, the exact edges of the rule, a corner of two walls.  Everything is
compared as tests/test_gpu_collider_walls.py compares it -- x, y, vx, vy, last_x, last_y of every particle, the
environments, the batch positions, pair_solves, cohesion_solves, viscosity_pairs, collider_hits and collider_grips, bit for
bit against the CPU model -- and every comparison is preceded by the assertion, on the model's census
(tests/collider_census.py), that the scene takes the branches it is there for.  The scenes, those assertions and the check
that a wrong rule would change a scene's state live in tests/test_collider_census.py, which needs no device.

Which test reaches which label of the census (W: a wall, S: a segment):

  test_hand_case                 one tiny batch per case of test_collider_census.CASES, its state imported, one step:
      hit_inside, hit_start, hit_end, on_it, point, miss                      W and S; hit_* from both sides of W
      catch_pos, catch_neg, catch_inside_r (both sides), catch_on_line (both sides), no_side, round_start, round_end
      (both sides), masked                                                     W
      stick, slide, no_tangent, smooth                                        W that does not catch, and S
      caught_stick, caught_slide (both sides), caught_no_tangent, caught_smooth   W
      half_plane hit, miss; disc hit, centre, miss; container hit, clamped, miss; each kind with stick or slide, smooth
      closed forms: catch_on_line, on_it and a disc's centre along DIRS[key & 7], point, the half-plane and container hits;
      the degenerate wall (3,3,3,3); a second sub-step
  test_oblique_wall              catch_pos, catch_neg, catch_inside_r, round_start, round_end, hit_start, hit_end, hit_inside,
                                 stick, slide, caught_stick, caught_slide: W, both types, 688 particles, the plain and the
                                 cohesive wall instantiation
  test_oblique_segment           hit_start, hit_end, hit_inside; smooth (the collider kernels) or stick, slide (the surface ones): S
  test_corner                    half_plane hit (white) and miss; catch_neg and hit_inside at each of two walls, one particle
                                 caught by both in one pass; either list order
  test_device_group, test_sharded_two_ranks   the labels of test_oblique_wall per batch, every handle its share

Out of scope: NaN positions (a NaN cell fails the step before step 5b matters), rx_force.  The pair loop of the gather
kernel has a census of its own: tests/pair_census.py, tests/test_pair_census.py, tests/test_gpu_pair_edges.py."""
import numpy as np
import pytest

import test_collider_census as cc
from conftest import ROOT
from test_gpu_collider_surfaces import FIELDS, _assert_snapshot, _snapshot
from test_gpu_collider_walls import _configure

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
INF = float("inf")
S, C = cc.S, cc.C


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


# ------------------------------------------------------------------------------------------------ a. the hand table
def _hand_handle(egg):
    h = egg.SimulationHandler()
    h.set_solver_order("relaxed")
    w, y = cc.hand_configs()
    h.set_white_config({k: w[k] for k in ("damping", "follow_strength", "min_radius", "max_radius")})
    h.set_yolk_config({k: y[k] for k in ("damping", "follow_strength", "min_radius", "max_radius")})
    return h


@pytest.fixture(scope="module")
def tiny(egg):
    """(id, info, white state, yolk state) of the tiny batch every case starts from, exported once"""
    src = _hand_handle(egg)
    i = src.add(*cc.HAND_TARGET, cc.HAND_RADIUS, cc.HAND_RADIUS, None, None, 2, 2)
    info, ws, ys = src.export_batch(i)
    assert ws.shape == ys.shape == (9, 2) and (ws[7] == 2.0).all() and (ys[7] == 2.0).all()  # (the radius)
    return i, info, ws, ys


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_hand_case(egg, tiny, name):
    m = cc.assert_hand_labels(name)  # the branch, on the model, first
    case = cc.CASES[name]
    spots, forces, update = cc.hand_setup(name)
    i, info, ws, ys = tiny
    assert cc.hand_model(name)[1] == i
    ws, ys = ws.copy(), ys.copy()
    for state, w in ((ws, WHITE), (ys, YOLK)):
        for p, ((x, y), (vx, vy)) in enumerate(spots[w]):
            state[0, p] = state[4, p] = x
            state[1, p] = state[5, p] = y
            state[2, p], state[3, p] = vx, vy
    h = _hand_handle(egg)
    h.set_colliders([case["collider"]])
    h.set_forces(list(forces))
    if case["surface"] is not None:
        h.set_collider_surfaces([case["surface"]])
    assert h.import_batch(info, ws, ys) == i
    assert h.update(*update) == 1
    _assert_snapshot(h, _snapshot(m, [i]), name)
    for w, want in (cc.hand_closed_form(name) or {}).items():
        got = tuple(float(h.download(w, f)[cc.TESTED[w]]) for f in ("x", "y", "vx", "vy"))
        assert got == want, (name, w)


# ------------------------------------------------------------------------------------------------ b. - d. one handle
def _run_one_handle(egg, name):
    """the scene on one handle against the model's snapshots: after the first step and after every step from the first catch
    (for a list without walls: the first hit) on"""
    cfg, colliders, surfaces, forces, starts, targets, steps = cc.SCENES[name]
    m, ids, snaps = cc.assert_scene_reach(name)
    first = min(k for k in snaps if sum(snaps[k]["catches"]) > 0 or (sum(m.wall_catches) == 0 and sum(snaps[k]["hits"]) > 0))
    assert 1 < first < steps
    h = _configure(egg.SimulationHandler(), cfg, colliders, surfaces, forces)
    assert [c[0] for c in h.get_colliders()] == [c[0] for c in colliders]
    assert [h.add(x, y, 50, 15) for x, y in starts] == ids
    for k in range(steps):
        if k == 2:
            for i, (x, y) in zip(ids, targets):
                h.set_target_position(i, x, y)
        assert h.update(1 / 60, 1 / 60, S, C) == 1
        if k + 1 == 1 or k + 1 >= first:
            _assert_snapshot(h, snaps[k + 1], "%s step %d" % (name, k + 1))
    return h


@pytest.mark.parametrize("name", cc.WALL_SCENES)
def test_oblique_wall(egg, name):
    _run_one_handle(egg, name)


@pytest.mark.parametrize("name", ["segment_smooth", "segment_rough"])
def test_oblique_segment(egg, name):
    h = _run_one_handle(egg, name)
    assert (sum(h.collider_grips()) > 0) == (name == "segment_rough")


@pytest.mark.parametrize("name", ["corner", "corner_reversed"])
def test_corner(egg, name):
    cc.test_the_order_of_the_corners_list_matters()
    _run_one_handle(egg, name)


# ------------------------------------------------------------------------------------------------ e. groups and ranks
GROUP = "wall_all"
# in x, across the wall.  In wall_all no particle comes within 90 px of one that another of the three handles owns
# (asserted on the model, test_collider_census.assert_scene_reach): the three handles run the scene whose first target lies
# further right, so that they have ghosts to exchange
CUTS = {2: [-INF, 300.0, INF], 3: [-INF, 200.0, 400.0, INF]}
GROUP_SCENE = {2: GROUP, 3: "wall_all_wide"}


def _assert_a_share_of_both_sides(snaps, ids, owned):
    """owned[h][k]: the batches handle or rank h owned after step k + 1.  A step's catches of a batch, per type and side
    (the census, per batch), go to the handle that owned the batch before and after that step.  One handle has caught
    particles of both types from above and from below."""
    share = [dict.fromkeys([(w, lab) for w in (WHITE, YOLK) for lab in ("catch_pos", "catch_neg")], 0) for _ in owned]
    for k in sorted(snaps):
        for (w, lab, b), n in snaps[k]["sides"].items():
            for h, after in enumerate(owned):
                if b in after[k - 1] and b in after[max(k - 2, 0)]:
                    share[h][(w, lab)] += n - (snaps[k - 1]["sides"][(w, lab, b)] if k > 1 else 0)
    print("catches per (type, side), per handle: %s" % share)
    assert any(min(s.values()) > 0 for s in share), share


@pytest.mark.parametrize("n_handles", [2, 3])
def test_device_group(egg, n_handles):
    name = GROUP_SCENE[n_handles]
    cfg, colliders, surfaces, forces, starts, targets, steps = cc.SCENES[name]
    m, ids, snaps = cc.assert_scene_reach(name)
    g = _configure(egg.SimulationGroup([0] * n_handles, cuts=CUTS[n_handles]), cfg, colliders, surfaces, forces)
    h = _configure(egg.SimulationHandler(), cfg, colliders, surfaces, forces)
    assert g.get_colliders() == h.get_colliders() and all(b.get_colliders() == h.get_colliders() for b in g.handles)
    assert [g.add(x, y, 50, 15) for x, y in starts] == ids == [h.add(x, y, 50, 15) for x, y in starts]
    assert len({g.owner(i)[0] for i in ids}) == n_handles  # (every handle owns a batch)
    owned = [[] for _ in range(n_handles)]
    for k in range(steps):
        if k == 2:
            for i, (x, y) in zip(ids, targets):
                g.set_target_position(i, x, y)
                h.set_target_position(i, x, y)
        g.step(1 / 60, S, C)
        h.step(1 / 60, S, C)
        for b in range(n_handles):
            owned[b].append({i for i in ids if g.owner(i)[0] == b})
    snap = snaps[steps]
    for w in (WHITE, YOLK):
        got = g.particles(w, FIELDS)
        cat = np.concatenate([np.array(got[i]) for i in sorted(got)], axis=1)
        for k, f in enumerate(FIELDS):
            assert np.array_equal(cat[k], h.download(w, f)), "type %d field %s: the group against the one handle" % (w, f)
            assert np.array_equal(cat[k], snap["state"][w][k]), "type %d field %s: the group against the model" % (w, f)
    for i in ids:
        assert g.get_position(i) == h.get_position(i) == snap["pos"][i]
    _assert_snapshot(h, snap, "%s: the one handle" % name)
    assert g.collider_hits() == snap["hits"] and g.collider_grips() == snap["grips"]
    for what, want in (("collider_hits", snap["hits"]), ("collider_grips", snap["grips"])):
        assert [sum(getattr(b, what)()[w] for b in g.handles) for w in (WHITE, YOLK)] == want, what
    assert sum(b.stats()["pair_solves"] for b in g.handles) == snap["pairs"]
    assert sum(b.stats()["cohesion_solves"] for b in g.handles) == snap["cohered"] > 0
    assert all(min(b.collider_hits()) > 0 for b in g.handles)  # (every handle's own particles of both types met the wall)
    halo = g.halo_counters()
    assert halo["records"] > 0 and halo["bytes"] == 40 * halo["records"]
    _assert_a_share_of_both_sides(snaps, ids, owned)


SHARDED_CUTS = [-2000.0, 300.0, 2000.0]


def _worker(rank, world, port, q):
    import os
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from egg_fluid_simulation_amd import SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler, SlabLayout
    from test_gpu_sharded_relaxed import _state
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg, colliders, surfaces, forces, starts, targets, steps = cc.SCENES[GROUP]
        sh = ShardedSimulationHandler(SlabLayout(SHARDED_CUTS), rank, dist, lambda: SimulationHandler(device=0), device="cpu")
        _configure(sh, cfg, colliders, surfaces, forces)
        gids = [sh.add(x, y, 50, 15) for x, y in starts]
        mine = []
        for k in range(steps):
            if k == 2:
                for gid, (x, y) in zip(gids, targets):
                    sh.set_target_position(gid, x, y)
            sh.step(1 / 60, S, C)
            mine.append(sorted(_state(sh)[WHITE]))
        st = sh.local.stats()
        q.put((rank, "ok", dict(state=_state(sh), pos=sh.positions(), pairs=st["pair_solves"], cohered=st["cohesion_solves"],
                                hits=sh.collider_hits(), grips=sh.collider_grips(), own_hits=sh.local.collider_hits(),
                                own_grips=sh.local.collider_grips(), owned=mine, halo=sh.halo_counters())))
    except Exception:
        import traceback
        q.put((rank, "error: " + traceback.format_exc(), None))
    finally:
        dist.destroy_process_group()


def _spawn(world):
    import queue
    import time

    import torch.multiprocessing as mp
    from test_gpu_sharded_relaxed import _free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    deadline = time.time() + 300
    while len(res) < world and time.time() < deadline:
        try:
            rank, outcome, results = q.get(timeout=2)
            assert outcome == "ok", outcome
            res[rank] = results
        except queue.Empty:
            if any(p.exitcode not in (None, 0) for p in procs):
                break
    for p in procs:
        p.join(20)
        if p.is_alive():
            p.kill()  # the exact child started above
    assert len(res) == world and all(p.exitcode == 0 for p in procs), "a rank failed: see its traceback above"
    return res


def test_sharded_two_ranks():
    """two ranks on one GPU, the cut across the oblique wall, everything on: the fields gathered from both ranks are the
    model's, the summed counters are the model's, nothing new travels (a ghost record stays 40 bytes)"""
    m, ids, snaps = cc.assert_scene_reach(GROUP)
    res = _spawn(2)
    snap = snaps[cc.SCENES[GROUP][6]]
    for w in (WHITE, YOLK):
        n = snap["state"][w].shape[1] // len(ids)
        seen = []
        for r in (0, 1):
            for gid, cols in res[r]["state"][w].items():
                seen.append(gid)
                for k, f in enumerate(FIELDS):
                    want = snap["state"][w][k][(gid - 1) * n:gid * n]
                    assert np.array_equal(np.array(cols[k]), want), "type %d field %s batch %d" % (w, f, gid)
        assert sorted(seen) == ids
    for r in (0, 1):
        assert {g: tuple(p) for g, p in res[r]["pos"].items()} == snap["pos"]
        assert res[r]["hits"] == snap["hits"] and res[r]["grips"] == snap["grips"]
        assert res[r]["halo"]["records"] > 0 and res[r]["halo"]["bytes"] == 40 * res[r]["halo"]["records"]
        assert min(res[r]["own_hits"]) > 0 and res[r]["owned"][0]  # (every rank owns a batch; its own particles met the wall)
    for what, want in (("own_hits", snap["hits"]), ("own_grips", snap["grips"])):
        assert [sum(res[r][what][w] for r in (0, 1)) for w in (WHITE, YOLK)] == want, what
    assert sum(res[r]["pairs"] for r in (0, 1)) == snap["pairs"]
    assert sum(res[r]["cohered"] for r in (0, 1)) == snap["cohered"] > 0
    _assert_a_share_of_both_sides(snaps, ids, [[set(after) for after in res[r]["owned"]] for r in (0, 1)])
