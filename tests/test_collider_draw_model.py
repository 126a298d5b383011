"""The numpy model of the colliders in the picture (tests/collider_draw_model.py) against the rules of DESIGN.md section
2.7, "Collider styles", on the CPU with no device; the table of wrong rules the scenes of tests/test_gpu_collider_draw.py
must notice; and the part of the new surface that needs no device: the style record's layout and the wrappers' argument
checks."""
import ctypes as C
import math

import numpy as np
import pytest

import collider_draw_model as cdm


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


WHITE_FILL = {"fill": (1.0, 1.0, 1.0, 1.0)}


def coverage(colliders, styles, size=(64, 48), layer="under"):
    """the coverage of an opaque white style over a cleared (0, 0, 0, 0) screen: the alpha channel"""
    return cdm.draw_colliders(cdm.clear_screen(size, (0, 0, 0, 0)), colliders, styles, (0.0, 0.0), layer)[..., 3]


def test_nothing_styled_leaves_every_bit_alone():
    rng = np.random.default_rng(5)
    screen = rng.standard_normal((cdm.SIZE[1], cdm.SIZE[0], 4)).astype(np.float32)
    screen[::3, ::2] = np.float32(-0.0)
    for styles in (None, [], [None] * len(cdm.ALONE), [{"line": (1, 1, 1, 1), "line_width": 0.0}] * len(cdm.ALONE),
                   [{"fill": (1, 1, 1, 0.0), "line": (1, 1, 1, 0.0), "line_width": 4.0}] * len(cdm.ALONE)):
        for layer in ("under", "over"):
            assert same_bits(cdm.draw_colliders(screen, cdm.ALONE, styles, (0.0, 0.0), layer), screen)
    # a visible collider leaves what it does not cover alone too, the sign of a zero included
    out = cdm.draw_colliders(screen, [("disc", 20.0, 20.0, 5.0)], [WHITE_FILL], (0.0, 0.0), "under")
    far = np.hypot(*np.meshgrid(np.arange(cdm.SIZE[0]) + 0.5 - 20.0, np.arange(cdm.SIZE[1]) + 0.5 - 20.0)) > 6.0
    assert same_bits(out[far], screen[far]) and not same_bits(out, screen)
    # and a segment's fill is ignored: it has no inside
    assert same_bits(cdm.draw_colliders(screen, [("segment", 5.0, 5.0, 50.0, 30.0)], [WHITE_FILL], (0.0, 0.0), "under"), screen)


def test_a_pixel_inside_a_disc_is_one_blend_of_the_fill():
    clear = np.float32([0.1, 0.2, 0.3, 1.0])
    fill = np.float32([0.9, 0.4, 0.2, 0.6])
    out = cdm.draw_colliders(cdm.clear_screen((64, 48), clear), [("disc", 30.5, 20.5, 15.0)], [{"fill": tuple(fill)}], (0.0, 0.0), "under")
    k = np.float32(1.0) - fill[3]
    want = np.float32([fill[0] * fill[3] + clear[0] * k, fill[1] * fill[3] + clear[1] * k, fill[2] * fill[3] + clear[2] * k,
                       fill[3] + clear[3] * k])
    assert same_bits(out[20, 25], want)  # 5 px from the centre, 10 px inside the rim
    assert same_bits(out[20, 60], clear)


def test_the_edge_ramp_is_one_pixel_wide():
    row = coverage([("half_plane", 1.0, 0.0, 30.25)], [WHITE_FILL])[10]  # solid where x < 30.25
    assert np.all(row[:29] == 1.0) and np.all(row[31:] == 0.0)
    assert row[29] == 1.0 and row[30] == np.float32(0.25)  # centres 29.5 (sd -0.75) and 30.5 (sd 0.25)
    cov = coverage([("disc", 32.0, 24.0, 10.3)], [WHITE_FILL])
    d = np.hypot(*np.meshgrid(np.arange(64) + 0.5 - 32.0, np.arange(48) + 0.5 - 24.0))
    assert np.all(cov[d <= 9.8] == 1.0) and np.all(cov[d >= 10.8] == 0.0)
    ramp = (d > 9.8) & (d < 10.8)
    assert np.all((cov[ramp] > 0) & (cov[ramp] < 1)) and np.allclose(cov[ramp], 10.8 - d[ramp], atol=1e-6)


def test_a_container_is_the_discs_complement():
    disc = coverage([("disc", 32.0, 24.0, 10.3)], [WHITE_FILL])
    cont = coverage([("container", 32.0, 24.0, 10.3)], [WHITE_FILL])
    assert np.allclose(disc + cont, 1.0, atol=1e-6)
    assert cont[24, 32] == 0.0 and cont[0, 0] == 1.0 and disc[24, 32] == 1.0 and disc[0, 0] == 0.0


def test_a_segment_of_width_w_covers_w_plus_one_pixels_and_has_round_ends():
    w = 3.0
    style = [{"line": (1.0, 1.0, 1.0, 1.0), "line_width": w}]
    cov = coverage([("segment", 10.0, 20.25, 40.0, 20.25)], style)
    col = cov[:, 25]
    dy = np.abs(np.arange(48) + 0.5 - 20.25)
    assert np.count_nonzero(col) == int(w) + 1 and np.array_equal(col > 0, dy < 0.5 + w / 2)
    assert np.all(col[dy <= w / 2 - 0.5] == 1.0)
    # beyond an end the distance is to the end point: a round cap, not a square one
    yy, xx = np.meshgrid(np.arange(48) + 0.5, np.arange(64) + 0.5, indexing="ij")
    r = np.hypot(xx - 40.0, yy - 20.25)
    beyond = xx > 40.0
    assert np.array_equal(cov[beyond] > 0, r[beyond] < 0.5 + w / 2)
    assert cov[18, 41] == 0.0 and cov[18, 39] > 0.0  # dx 1.5, dy 1.75: outside the cap, though inside a square one
    # the degenerate one is a dot
    dot = coverage([("wall", 30.0, 20.0, 30.0, 20.0)], style)
    assert np.array_equal(dot > 0, np.hypot(xx - 30.0, yy - 20.0) < 2.0)


def test_the_order_of_two_translucent_colliders_shows():
    a, b = ("disc", 28.0, 24.0, 10.0), ("disc", 36.0, 24.0, 10.0)
    sa, sb = {"fill": (1.0, 0.0, 0.0, 0.5)}, {"fill": (0.0, 0.0, 1.0, 0.5)}
    screen = cdm.clear_screen((64, 48), cdm.CLEAR)
    ab = cdm.draw_colliders(screen, [a, b], [sa, sb], (0.0, 0.0), "under")
    ba = cdm.draw_colliders(screen, [b, a], [sb, sa], (0.0, 0.0), "under")
    assert ab[24, 32, 2] > ab[24, 32, 0] and ba[24, 32, 0] > ba[24, 32, 2]  # the later one lies on top
    assert same_bits(ab[24, 20], ba[24, 20])  # where only one covers, the order does not matter
    # a layer is drawn on its own: "over" alone draws only the over entries
    over = cdm.draw_colliders(screen, [a, b], [sa, dict(sb, layer="over")], (0.0, 0.0), "over")
    assert same_bits(over, cdm.draw_colliders(screen, [b], [sb], (0.0, 0.0), "under"))


def _advanced(colliders):
    """MOVING one step of 1 / 60 s on, by hand: the wall translated, the segment turned about its pivot"""
    out = []
    for c, mo, sp in zip(colliders, cdm.MOVING_MOTION, cdm.MOVING_SPIN):
        p = list(c[1:5])
        if mo is not None:
            p = [p[0] + mo[0] / 60, p[1] + mo[1] / 60, p[2] + mo[0] / 60, p[3] + mo[1] / 60]
        if sp is not None:
            co, si = math.cos(sp[2] / 60), math.sin(sp[2] / 60)
            rot = lambda x, y: (sp[0] + co * (x - sp[0]) - si * (y - sp[1]), sp[1] + si * (x - sp[0]) + co * (y - sp[1]))
            p = list(rot(p[0], p[1]) + rot(p[2], p[3]))
        out.append((c[0],) + tuple(p) + c[5:])
    return out


def test_pose_at_the_ends_is_the_two_lists():
    last = [c + ("both",) for c in cdm.MOVING]
    cur = _advanced(last)
    assert cdm.pose(last, cur, 0.0) == last and cdm.pose(last, cur, 1.0) == cur
    assert cdm.pose(last, cur, -3.0) == last and cdm.pose(last, cur, 1.7) == cur  # clamped
    mid = cdm.pose(last, cur, 0.35)
    assert mid[0][1] == last[0][1] * (1.0 - 0.35) + cur[0][1] * 0.35 and mid[0][0] == "wall" and mid[0][-1] == "both"
    # a list that did not move stays where it is at every t -- up to the one rounding of p * (1 - t) + p * t
    still = cdm.pose(last, last, 0.35)
    assert all(a[0] == b[0] and np.allclose(a[1:5], b[1:5], rtol=4e-16, atol=0.0) for a, b in zip(still, last))
    # the chord: half way through a turn the segment's far end lies inside the arc by 1 - cos(angle / 2) of the lever arm
    arm = 40.0
    far = cdm.pose(last, cur, 0.5)[1]
    assert math.isclose(arm - math.hypot(far[3] - 50.0, far[4] - 40.0), arm * (1 - math.cos(9.0 / 120)), rel_tol=1e-9)


def _scenes(wrong=None):
    """the model's images of the scenes of the GPU tests, under one rule"""
    last = [c + ("both",) for c in cdm.MOVING]
    cur = _advanced(last)
    alone = [c + ("both",) for c in cdm.ALONE]
    full = [c + ("both",) for c in cdm.FULL]
    out = {}
    for name, clear in (("alone", cdm.CLEAR), ("alone, -0.0", cdm.CLEAR_NEGATIVE_ZERO)):
        out[name] = cdm.frame(cdm.SIZE, clear, alone, alone, cdm.ALONE_STYLES, (0.0, 0.0), 0.35, wrong)
    out["full"] = cdm.frame(cdm.SIZE, cdm.CLEAR, full, full, cdm.FULL_STYLES, (0.0, 0.0), 0.35, wrong)
    out["far"] = cdm.frame(cdm.SIZE, cdm.CLEAR, cdm.shifted(alone, cdm.FAR_ORIGIN), cdm.shifted(alone, cdm.FAR_ORIGIN), cdm.ALONE_STYLES,
                           cdm.FAR_ORIGIN, 0.35, wrong)
    for t in cdm.MOVING_TS:
        out["moving, t = %r" % (t,)] = cdm.frame(cdm.SIZE, cdm.CLEAR, last, cur, cdm.MOVING_STYLES, (0.0, 0.0), 0.6 if t is None else t, wrong)
    return out


@pytest.fixture(scope="module")
def right():
    return _scenes()


def test_the_scenes_show_what_they_are_meant_to(right):
    alone = right["alone"]
    assert not same_bits(alone, cdm.clear_screen(cdm.SIZE, cdm.CLEAR))
    # the far origin moves everything alike: up to the rounding of the coordinates it is the same picture
    assert np.abs(right["far"] - alone).max() < 1e-3
    # every collider of the full list reaches the picture: leaving any one out changes it
    full = [c + ("both",) for c in cdm.FULL]
    for k in (0, 31, 32, 63):
        styles = list(cdm.FULL_STYLES)
        styles[k] = None
        assert not same_bits(cdm.frame(cdm.SIZE, cdm.CLEAR, full, full, styles, (0.0, 0.0), 0.0), right["full"]), k
    # the off-screen collider and the unstyled one change nothing
    styles = list(cdm.ALONE_STYLES)
    styles[6] = None
    lone = [c + ("both",) for c in cdm.ALONE]
    assert same_bits(cdm.frame(cdm.SIZE, cdm.CLEAR, lone, lone, styles, (0.0, 0.0), 0.0), alone)


@pytest.mark.parametrize("wrong", cdm.WRONG_RULES)
def test_every_wrong_rule_changes_a_scene(right, wrong):
    got = _scenes(wrong)
    changed = [name for name in right if not same_bits(got[name], right[name])]
    print(wrong, "->", changed)
    assert changed, "no scene of the GPU tests tells `%s` from the right rule" % wrong


def test_style_record_and_wrapper_checks():
    from egg_fluid_simulation_amd import EggError, SimulationGroup, SimulationHandler, _ffi
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    assert C.sizeof(_ffi.EggColliderStyle) == 40
    assert [f[0] for f in _ffi.EggColliderStyle._fields_] == ["fill", "line", "line_width", "layer"]
    assert _ffi.EggColliderStyle.line_width.offset == 32 and _ffi.EggColliderStyle.layer.offset == 36
    for cls in (SimulationHandler, SimulationGroup, ShardedSimulationHandler):
        for name in ("set_collider_styles", "get_collider_styles", "get_collider_pose"):
            assert callable(getattr(cls, name)), (cls, name)
    for name in ("egg_set_collider_styles", "egg_get_collider_styles", "egg_get_collider_pose", "egg_group_set_collider_styles",
                 "egg_group_get_collider_styles", "egg_group_get_collider_pose"):
        assert name in _ffi.EXPORTED_SYMBOLS
    n, arr = SimulationHandler._c_styles([None, {"fill": (0.1, 0.2, 0.3, 0.4)}, {"line": (1, 1, 1, 1), "line_width": 2, "layer": "over"}])
    assert n == 3 and tuple(arr[0].fill) == (0.0,) * 4 and arr[0].line_width == 0.0 and arr[0].layer == 0
    assert tuple(arr[1].fill) == tuple(np.float32([0.1, 0.2, 0.3, 0.4]).tolist()) and arr[1].layer == 0
    assert arr[2].line_width == 2.0 and arr[2].layer == 1
    for k, bad in enumerate(("red", {"colour": (1, 1, 1, 1)}, {"fill": (1, 1, 1)}, {"fill": (1, 1, 1, 1.5)}, {"line": (0, 0, float("nan"), 1)},
                             {"line_width": -1.0}, {"line_width": 64.5}, {"line_width": float("nan")}, {"line_width": "wide"},
                             {"layer": "middle"}, {"layer": 1}, {"fill": 3})):
        with pytest.raises(EggError, match="collider style %d" % (k % 3)):
            SimulationHandler._c_styles([None] * (k % 3) + [bad])
