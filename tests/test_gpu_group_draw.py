"""draw() and the rest of the SimulationHandler surface on a device group (egg_group_render .., DESIGN.md section 2.6
"Several devices"): the particles of every handle are gathered to the device of handle 0 in global-key order and drawn
by the single handle's kernels.  The rule under test: whatever a group returns or draws equals, BIT FOR BIT, what one
handle holding the same batches returns or draws -- np.array_equal everywhere, no tolerance.  All groups here are
several handles on GPU 0.  One image is also held against oracle/render_model.py directly."""
import copy
import ctypes as C
import math
import warnings

import numpy as np
import pytest

from conftest import circle_target, load_golden

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
INF = math.inf
FIELDS = ("x", "y", "vx", "vy", "last_x", "last_y", "radius", "inv_mass", "mass_t", "batch_id")
SIZE, ORIGIN, ALPHA, CLEAR = (600, 560), (-190.0, -180.0), 0.35, (0.1, 0.2, 0.3, 1.0)
# four_batches: centres (0, 0), (30, 10), (-20, 40), (200, 200)
EXACT_CUTS = {1: None, 2: [-INF, 100.0, INF], 3: [-INF, -10.0, 100.0, INF], 4: [-INF, -10.0, 15.0, 100.0, INF]}
RELAXED_CUTS = {2: [-INF, 10.0, INF], 3: [-INF, -5.0, 25.0, INF]}  # through the cluster of the first three batches


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _pair(egg, cuts, order="exact", white=None, yolk=None):
    n = 1 if cuts is None else len(cuts) - 1
    g = egg.SimulationGroup([0] * n, cuts=cuts, white_config=copy.deepcopy(white), yolk_config=copy.deepcopy(yolk))
    h = egg.SimulationHandler(copy.deepcopy(white), copy.deepcopy(yolk))
    if order != "exact":
        g.set_solver_order(order)
        h.set_solver_order(order)
    return g, h


def _add_both(g, h, centers, *more, **kw):
    ids = [g.add(x, y, *more, **kw) for x, y in centers]
    assert [h.add(x, y, *more, **kw) for x, y in centers] == ids
    return ids


def _step_both(g, h, S=2, C=3):
    g.step(1 / 60, S, C)
    h.step(1 / 60, S, C)


def _move_both(g, h, i, x, y):
    g.set_target_position(i, x, y)
    h.set_target_position(i, x, y)


def _same_draw(g, h, what, size=SIZE, origin=ORIGIN, alpha=ALPHA, clear=CLEAR, **kw):
    """screen image, both canvases with their origins and all ten environment fields of both types"""
    a = g.draw(size, origin, interpolation_alpha=alpha, clear=clear, **kw)
    b = h.draw(size, origin, interpolation_alpha=alpha, clear=clear, **kw)
    print(what, "screen: differing values", int((a != b).sum()), "max |diff|", float(np.abs(a - b).max()))
    assert a.shape == b.shape and np.array_equal(a, b), what + ": screen"
    for w in (WHITE, YOLK):
        (cg, og), (ch, oh) = g.render_canvas(w), h.render_canvas(w)
        print(what, "canvas", w, cg.shape, ch.shape, og, oh)
        assert cg.shape == ch.shape and np.array_equal(cg, ch) and og == oh, "%s: canvas %d" % (what, w)
    _same_environment(g, h, what)
    return a


def _same_environment(g, h, what):
    for w in (WHITE, YOLK):
        eg, eh = g.get_environment(w), h.get_environment(w)
        assert len(eg) == 10 and sorted(eg) == sorted(eh)
        for k in eh:
            assert np.array_equal(eg[k], eh[k]), "%s: environment %d %s: %r != %r" % (what, w, k, eg[k], eh[k])


def _same_particles(g, h, what):
    for w in (WHITE, YOLK):
        for f in FIELDS:
            a, b = g.download(w, f), h.download(w, f)
            assert a.shape == b.shape and np.array_equal(a, b), "%s: type %d field %s" % (what, w, f)


def _four_batches(egg, cuts, order, draws=(1, 10, 30)):
    centers = [tuple(c) for c in load_golden("four_batches")["centers"]]
    g, h = _pair(egg, cuts, order)
    ids = _add_both(g, h, centers, 50, 15)
    if cuts is not None:
        assert len({g.owner(i)[0] for i in ids}) >= 2  # the batches start on different handles
    images, g.spread_at_draws = [], []
    for k in range(max(draws)):
        for i, c in zip(ids, centers):
            _move_both(g, h, i, *circle_target(c, k))
        _step_both(g, h)
        if k + 1 in draws:
            images.append(_same_draw(g, h, "%s, %s handles, step %d" % (order, "1" if cuts is None else len(cuts) - 1, k + 1)))
            g.spread_at_draws.append(len({g.owner(i)[0] for i in ids[:3]}))  # handles that hold a part of the cluster
    _same_particles(g, h, "after the draws")
    assert images[-1][..., 3].max() > 0.9 and not np.array_equal(images[0], images[-1])  # something is in the picture, and it moves
    return g, h


@pytest.mark.parametrize("n_handles", [1, 2, 3, 4])
def test_exact_order_four_batches(egg, n_handles):
    _four_batches(egg, EXACT_CUTS[n_handles], "exact")


@pytest.mark.parametrize("n_handles", [2, 3])
def test_relaxed_order_cut_through_a_cluster(egg, n_handles):
    g, h = _four_batches(egg, RELAXED_CUTS[n_handles], "relaxed")
    # one island on both sides of a cut while it was drawn: relaxed order hands nothing over before a step (the circling
    # targets carry the whole cluster into one slab later on)
    print("handles holding a part of the cluster at the draws", g.spread_at_draws)
    assert g.spread_at_draws[0] >= 2, g.spread_at_draws
    assert g.halo_counters()["records"] > 0 and g.counters()["discarded_steps"] == 0


def test_group_image_matches_the_render_model(egg, oracle_mod):
    """a group's image against oracle/render_model.py fed with the oracle's states, as
    tests/test_gpu_render.py::test_draw_matches_the_model does for one handle"""
    from oracle import render_model as model
    spots = [(100.0, 100.0), (300.0, 140.0), (190.0, 330.0)]
    g = egg.SimulationGroup([0, 0], cuts=[-INF, 200.0, INF])
    o = oracle_mod.Oracle()
    ids = [g.add(x, y, 50, 15) for x, y in spots]
    assert [o.add(x, y, 50, 15) for x, y in spots] == ids and [g.owner(i)[0] for i in ids] == [0, 1, 0]
    for s in (g, o):
        s.set_target_position(ids[1], 900.0, -400.0)
    for _ in range(6):
        g.step(1 / 60, 2, 3)
        o.step(1 / 60, 2, 3)
    for w in (WHITE, YOLK):
        for f in ("x", "y", "vx", "vy"):
            assert np.array_equal(g.download(w, f), o.field(w, f)), (w, f)
    size, origin, t, clear = (520, 470), (-40.0, -30.0), 0.35, (0.1, 0.2, 0.3, 1.0)
    image = g.draw(size, origin, interpolation_alpha=t, clear=clear)
    states = [{k: o.field(w, k) for k in ("x", "y", "last_x", "last_y", "vx", "vy", "radius")} for w in (WHITE, YOLK)]
    colors = [np.ones((states[w]["x"].size, 4), np.float32) for w in (WHITE, YOLK)]
    ref, canvases = model.render(states, [o.env(w) for w in (WHITE, YOLK)], model.DEFAULT_RENDER, colors, size, t, origin, None, None, clear)
    for w in (WHITE, YOLK):
        canvas, (x0, y0) = g.render_canvas(w)
        assert canvas.shape == canvases[w].shape and np.array_equal(canvas, canvases[w]), w
        env = o.env(w)
        assert (x0, y0) == (env["centroid_x"] - 0.5 * canvas.shape[1], env["centroid_y"] - 0.5 * canvas.shape[0])
        for k, v in g.get_environment(w).items():
            if k in env:
                assert v == env[k], (w, k)
    assert image.shape == ref.shape and np.array_equal(image, ref)
    assert np.unique(np.round(image[..., :3], 2).reshape(-1, 3), axis=0).shape[0] > 50


def test_colours_configs_and_a_hand_over(egg):
    white, yolk = egg.default_configs()
    white = dict(white, outline_thickness=2.5, highlight_strength=0.6, shadow_strength=0.7, texture_scale=10.0, motion_blur=0.002)
    yolk = dict(yolk, outline_thickness=0.0, highlight_strength=1.5, shadow_strength=0.4)
    g, h = _pair(egg, [-INF, 400.0, INF], white=white, yolk=yolk)
    for s in (g, h):
        s._use_particle_color = True
    assert g._use_particle_color and g._use_lighting
    # twelve batches: the yolk budget 0.05 N^2 stays slack (L:1752-1753), the exact protocol keeps the batches apart
    centers = [(100.0, 700.0)] + [(100.0 + 150.0 * (k % 6), 100.0 + 170.0 * (k // 6)) for k in range(11)]
    a = _add_both(g, h, centers[:1], 50, 15, white_color=[0.9, 0.5, 0.4, 0.8], yolk_color=[0.3, 0.9, 0.2, 1.0])[0]
    rest = _add_both(g, h, centers[1:], 50, 15)
    b = rest[0]
    assert g.owner(a)[0] == 0 and g.owner(rest[5])[0] == 1
    for _ in range(4):
        _step_both(g, h)
    for s in (g, h):
        s.set_yolk_color(b, 0.2, 0.3, 1.0, 0.6)   # b has no table of its own: the config is retinted (L:49-50)
        s.set_white_color(a, 0.1, 0.8, 0.7)       # a has: the config stays
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            s.set_white_color(99, 0.5, 0.5, 0.5)  # unknown id: a warning (L:259 style), nothing else
        assert any("no batch with id" in str(r.message) for r in rec)
    assert g.get_yolk_config()["color"] == h.get_yolk_config()["color"] == [0.2, 0.3, 1.0, 0.6]
    assert g.get_white_config()["color"] == h.get_white_config()["color"] == list(white["color"])
    lib, cg, ch = g._lib, egg._ffi.EggRenderConfig(), egg._ffi.EggRenderConfig()
    for w in (WHITE, YOLK):
        assert lib.egg_group_get_render_config(g._g, w, C.byref(cg)) == 0 and lib.egg_get_render_config(h._h, w, C.byref(ch)) == 0
        assert bytes(cg) == bytes(ch)
    size, origin = (1000, 860), (-20.0, -20.0)
    for instancing in (True, False):
        _same_draw(g, h, "colours, instancing %s" % instancing, size, origin, 1.0, (0, 0, 0, 0), use_instancing=instancing)
    for s in (g, h):
        s._use_lighting = False
        s.set_white_config(dict(outline_thickness=1.5, outline_color=[0.2, 0.1, 0.9, 1.0], highlight_strength=0.2))
        s.set_yolk_config(dict(outline_thickness=2.0, shadow_strength=1.1, color=[0.9, 0.8, 0.1, 1.0]))
        s.set_yolk_color(b, 0.7, 0.1, 0.1, 1.0)  # the config got a new table (L:1307-1311): b no longer retints it
    assert g.get_yolk_config() == h.get_yolk_config() and g.get_white_config() == h.get_white_config()
    image = _same_draw(g, h, "after set_*_config", size, origin, 0.5, CLEAR)
    # the coloured batch is driven across the cut until it has been handed over
    before = g.counters()["migrations"]
    for k in range(60):
        _move_both(g, h, a, min(100.0 + 12.0 * k, 700.0), 700.0)
        _step_both(g, h)
        if g.counters()["migrations"] > before and g.owner(a)[0] == 1:
            break
    assert g.counters()["migrations"] > before and g.owner(a)[0] == 1
    moved = _same_draw(g, h, "after the hand-over", size, origin, 0.5, CLEAR)
    assert not np.array_equal(image, moved)
    # the colour is in the picture: without it the image differs
    h.set_white_color(a, 1.0, 1.0, 1.0)
    assert not np.array_equal(h.draw(size, origin, interpolation_alpha=0.5, clear=CLEAR), moved)


def test_remove_add_empty_handle_and_nothing_to_draw(egg):
    clear = (0.5, 0.25, 0.125, 1.0)
    g, h = _pair(egg, [-INF, 1000.0, INF], "relaxed")
    ids = _add_both(g, h, [(100.0, 100.0), (160.0, 120.0), (300.0, 80.0)], 50, 15)
    assert {g.owner(i)[0] for i in ids} == {0} and g.handles[1].get_n_particles() == (0, 0)  # handle 1 owns nothing
    for s in (g, h):  # before the first step nothing is drawn (L:1997-1999, L:2118)
        image = s.draw((96, 80), clear=clear)
        assert image.shape == (80, 96, 4) and np.all(image == np.float32(clear))
        with pytest.raises(egg.EggError):
            s.render_canvas(WHITE)
    _same_environment(g, h, "before the first step")
    for _ in range(3):
        _step_both(g, h)
    _same_draw(g, h, "one handle empty", (420, 300), (0.0, 0.0))
    g.remove(ids[1])
    h.remove(ids[1])
    _step_both(g, h)
    _same_draw(g, h, "after remove", (420, 300), (0.0, 0.0))
    assert _add_both(g, h, [(1100.0, 90.0)], 50, 15) == [4] and g.owner(4)[0] == 1
    _same_draw(g, h, "after add, before its first step", (1300, 300), (0.0, 0.0))
    _step_both(g, h)
    _same_draw(g, h, "after add", (1300, 300), (0.0, 0.0))
    _same_particles(g, h, "after add")
    for i in (1, 3, 4):
        g.remove(i)
        h.remove(i)
    assert g.list_ids() == h.list_ids() == [] and g.get_n_particles() == h.get_n_particles() == (0, 0)
    for s in (g, h):
        assert np.all(s.draw((96, 80), clear=clear) == np.float32(clear))
        with pytest.raises(egg.EggError):
            s.render_canvas(YOLK)
    _same_environment(g, h, "empty")


def test_canvases_only_grow(egg):
    g, h = _pair(egg, [-INF, 250.0, INF], "relaxed")
    ids = _add_both(g, h, [(100.0, 100.0), (400.0, 140.0), (190.0, 430.0)], 50, 15)
    for _ in range(2):
        _step_both(g, h)
    _same_draw(g, h, "first", (64, 64))
    first = [g.render_canvas(w)[0].shape[:2] for w in (WHITE, YOLK)]
    assert first == [h.render_canvas(w)[0].shape[:2] for w in (WHITE, YOLK)]
    for s in (g, h):
        s.remove(ids[2])  # the bounds shrink, the canvases do not (L:1957-1970)
    for i in ids[:2]:
        _move_both(g, h, i, 250.0, 120.0)  # the targets move together
    for _ in range(12):
        _step_both(g, h)
        _same_draw(g, h, "shrinking", (64, 64))
        now = [g.render_canvas(w)[0].shape[:2] for w in (WHITE, YOLK)]
        assert now == [h.render_canvas(w)[0].shape[:2] for w in (WHITE, YOLK)]
        assert all(n[0] >= f[0] and n[1] >= f[1] for n, f in zip(now, first))
    env = g.get_environment(WHITE)
    assert env["max_y"] - env["min_y"] + 200 < first[WHITE][0]  # a fresh canvas would be much lower


@pytest.mark.parametrize("order", ["exact", "relaxed"])
def test_a_draw_between_steps_changes_nothing(egg, order):
    def run(draw):
        g = egg.SimulationGroup([0, 0], cuts=[-INF, 420.0, INF])
        g.set_solver_order(order)
        ids = [g.add(100.0 + 130.0 * (k % 6), 100.0 + 160.0 * (k // 6) + 40.0 * (k % 2), 50, 15) for k in range(12)]
        for step in range(10):
            for k, i in enumerate(ids[:6]):
                g.set_target_position(i, 100.0 + 130.0 * k + 15.0 * step, 100.0 + 40.0 * (k % 2) - 9.0 * step)
            g.update(1 / 60)
            if draw:
                g.draw((320, 240), origin=(0.0, 0.0), interpolation_alpha=0.5)
                g.get_environment(YOLK)
        by_batch = [g.particles(w, ("x", "y", "vx", "vy", "last_x", "last_y")) for w in (WHITE, YOLK)]
        return [g.download(w, f) for w in (WHITE, YOLK) for f in FIELDS], by_batch
    (plain, pb), (drawn, db) = run(False), run(True)
    assert all(np.array_equal(a, b) for a, b in zip(plain, drawn))
    for w in (WHITE, YOLK):
        assert sorted(pb[w]) == sorted(db[w])
        for i in pb[w]:
            assert all(np.array_equal(a, b) for a, b in zip(pb[w][i], db[w][i]))
        # download is particles() in one global order
        assert np.array_equal(np.concatenate([pb[w][i][0] for i in sorted(pb[w])]), plain[w * len(FIELDS)])


def test_the_rest_of_the_surface(egg):
    white, yolk = egg.default_configs()
    g, h = _pair(egg, [-INF, 500.0, INF], white=white, yolk=yolk)
    centers = [(100.0 + 150.0 * (k % 6), 100.0 + 170.0 * (k // 6)) for k in range(12)]
    ids = _add_both(g, h, centers, 50, 15)
    g.remove(5)
    h.remove(5)
    assert g.list_ids() == h.list_ids() == [i for i in ids if i != 5]
    assert g.get_n_particles() == h.get_n_particles() and g.get_n_particles(3) == h.get_n_particles(3) == (157, 15)
    with pytest.raises(egg.EggError, match="no batch with id"):
        g.get_n_particles(5)
    _move_both(g, h, 7, 123.5, -7.25)
    assert g.get_target_position(7) == h.get_target_position(7) == (123.5, -7.25)
    assert g.get_target_position(2) == h.get_target_position(2) == centers[1]
    with pytest.raises(egg.EggError, match="no batch with id"):
        g.get_target_position(5)
    assert g.update(0.04, 1 / 60) == h.update(0.04, 1 / 60) == 2  # a fractional rest stays in the accumulator (L:199-216)
    assert g.elapsed == h.elapsed and g.interpolation_alpha == h.interpolation_alpha and 0 < g.interpolation_alpha < 1
    _same_particles(g, h, "after update")
    _same_draw(g, h, "alpha from update", (1000, 420), (-20.0, -20.0), None, CLEAR)
    # a live config change: mass and radius are re-derived at the next step (L:1731-1744) on every handle
    for s in (g, h):
        s.set_white_config(dict(min_radius=3.0, max_radius=5.0, min_mass=1.0, max_mass=2.0))
        s.set_yolk_config(dict(min_radius=5.0, max_radius=6.0, max_mass=1.7))
    assert g.get_white_config() == h.get_white_config() and g.get_yolk_config() == h.get_yolk_config()
    for k in range(10):
        _move_both(g, h, 1, 100.0 + 20.0 * k, 100.0)
        _step_both(g, h)
    _same_particles(g, h, "after the config change")
    radii = g.download(WHITE, "radius")
    assert radii.min() >= 3.0 and radii.max() <= 5.0 and np.unique(radii).size > 20
    _same_draw(g, h, "after the config change", (1000, 420), (-20.0, -20.0))
    inst = g.download_instance_data(YOLK)
    assert inst.shape == (11 * 15, 7) and np.array_equal(inst, h.download_instance_data(YOLK))


def test_errors(egg):
    from egg_fluid_simulation_amd import _ffi
    g = egg.SimulationGroup([0, 0], cuts=[-INF, 500.0, INF])
    for k in range(12):
        g.add(100.0 + 150.0 * (k % 6), 100.0 + 170.0 * (k // 6), 50, 15)
    g.step(1 / 60, 2, 3)
    g.handles[1].step_begin(1 / 60, 2, 3)
    with pytest.raises(egg.EggError, match="a step is in flight on device 1"):
        g.draw((64, 64))
    with pytest.raises(egg.EggError, match="a step is in flight"):
        g.get_environment(WHITE)
    g.handles[1].step_end(False)
    g.draw((64, 64))
    lib = g._lib
    w, hh = C.c_int32(), C.c_int32()
    assert lib.egg_group_render_canvas(g._g, WHITE, None, 0, C.byref(w), C.byref(hh), None, None) == 0
    small = np.empty((4, 4, 4), np.float32)
    assert w.value * hh.value > 16
    rc = lib.egg_group_render_canvas(g._g, WHITE, small.ctypes.data_as(C.c_void_p), 16, None, None, None, None)
    assert rc == _ffi.EGG_ERR_INVALID_ARGUMENT and b"buffer holds 16 of" in lib.egg_group_last_error(g._g)
    assert lib.egg_group_render_canvas(g._g, 2, None, 0, None, None, None, None) == _ffi.EGG_ERR_INVALID_ARGUMENT
    assert lib.egg_group_download_particles(g._g, WHITE, 0, small.ctypes.data_as(C.c_void_p), 8) == _ffi.EGG_ERR_INVALID_ARGUMENT
    assert lib.egg_group_set_color(g._g, 99, YOLK, 0.0, 0.0, 0.0, 1.0) == _ffi.EGG_WARN_UNKNOWN_ID
    assert lib.egg_group_set_add_color(g._g, 99, YOLK, 0.0, 0.0, 0.0, 1.0) == _ffi.EGG_ERR_UNKNOWN_ID
    with pytest.raises(egg.EggError, match="screen of"):
        g.draw((0, 10))
