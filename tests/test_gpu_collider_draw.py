"""Colliders in the picture on the device ("Collider styles"): egg_render_colliders_kernel with its
tile culling against the unculled numpy model of tests/collider_draw_model.py, egg_get_collider_pose against the model's
pose.  Every image and every pose is compared for equality, bit for bit.  The screens are 100 x 84 px: the right and the
bottom tiles are partial.  The scenes with an egg state a screen of their own, 260 x 212 px (partial tiles again): an
egg's density blobs alone are wider than the small screen and would hide everything drawn under them."""
import ctypes as C

import numpy as np
import pytest

import collider_draw_model as cdm

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
H60 = 1 / 60
ZERO = (0.0, 0.0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b, what=""):
    print(what, "differing words:", int((bits(a) != bits(b)).sum()) if a.shape == b.shape else "shapes differ")
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def _as_stored(styles):
    """what get_collider_styles returns for visible styles: the defaults filled in, every number a float32"""
    out = []
    for s in styles:
        s = dict(cdm.STYLE_DEFAULTS, **s)
        out.append(dict(fill=tuple(float(np.float32(v)) for v in s["fill"]), line=tuple(float(np.float32(v)) for v in s["line"]),
                        line_width=float(np.float32(s["line_width"])), layer=s["layer"]))
    return out


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _relaxed(egg, colliders, styles=None):
    h = egg.SimulationHandler()
    h.set_solver_order("relaxed")
    h.set_colliders(colliders)
    if styles is not None:
        h.set_collider_styles(styles)
    return h


def _egg_handler(egg, steps=cdm.EGG["steps"]):
    """one egg of 50 + 15 particles over a half-plane floor, with gravity"""
    h = _relaxed(egg, cdm.EGG_COLLIDERS)
    h.set_forces([cdm.EGG["gravity"]])
    h.add(*cdm.EGG["at"], *cdm.EGG["radii"], None, None, *cdm.EGG["counts"])
    for _ in range(steps):
        h.step(H60, 2, 3)
    return h


def _alone(egg, colliders, styles, origin, clear):
    """a draw before the first step against the model applied to the clear"""
    h = _relaxed(egg, colliders, styles)
    image = h.draw(cdm.SIZE, origin, clear=clear)
    stored = h.get_colliders()
    assert h.get_collider_pose(0.0) == stored and h.get_collider_pose(0.3) == cdm.pose(stored, stored, 0.3)  # both lists are the list
    want = cdm.frame(cdm.SIZE, clear, stored, stored, styles, origin, 0.0)
    assert not same_bits(want, cdm.clear_screen(cdm.SIZE, clear), "model against the clear:")  # something is in the picture
    return image, want


@pytest.mark.parametrize("clear", [cdm.CLEAR, cdm.CLEAR_NEGATIVE_ZERO], ids=["opaque clear", "clear with -0.0"])
def test_colliders_alone_before_the_first_step(egg, clear):
    image, want = _alone(egg, cdm.ALONE, cdm.ALONE_STYLES, ZERO, clear)
    assert same_bits(image, want, "one of each kind:")
    if clear is cdm.CLEAR_NEGATIVE_ZERO:  # a pixel nothing covers keeps the sign of its zero
        untouched = bits(image)[..., 0] == 0x80000000
        assert untouched.any() and not untouched.all()


def test_a_full_list_uses_the_whole_mask(egg):
    image, want = _alone(egg, cdm.FULL, cdm.FULL_STYLES, ZERO, cdm.CLEAR)
    assert same_bits(image, want, "64 segments:")


def test_far_from_the_origin(egg):
    image, want = _alone(egg, cdm.shifted(cdm.ALONE, cdm.FAR_ORIGIN), cdm.ALONE_STYLES, cdm.FAR_ORIGIN, cdm.CLEAR)
    assert same_bits(image, want, "origin (1e6 + 0.25, -2e6):")


@pytest.fixture(scope="module")
def scene(egg):
    h = _egg_handler(egg)
    assert sum(h.collider_hits()) > 0  # the egg lies on something
    return h


ALPHA, ORIGIN = 0.35, (3.0, -2.0)


def _parent_draw(h):
    """the draw with styles unset: the path the existing render tests hold; its canvases and environments"""
    h.set_collider_styles([])
    plain = h.draw(cdm.EGG_SIZE, ORIGIN, interpolation_alpha=ALPHA, clear=cdm.CLEAR)
    canvases = [h.render_canvas(w)[0] for w in (WHITE, YOLK)]
    envs = [h.get_environment(w) for w in (WHITE, YOLK)]
    assert not same_bits(plain, cdm.clear_screen(cdm.EGG_SIZE, cdm.CLEAR), "the eggs against the clear:")  # the egg is in the picture
    return plain, canvases, envs


def test_under_the_eggs(egg, scene):
    from oracle import render_model
    h = scene
    plain, canvases, envs = _parent_draw(h)
    h.set_collider_styles(cdm.EGG_STYLES_UNDER)
    image = h.draw(cdm.EGG_SIZE, ORIGIN, interpolation_alpha=ALPHA, clear=cdm.CLEAR)
    for w in (WHITE, YOLK):  # the eggs are drawn as they were: same canvases
        assert same_bits(h.render_canvas(w)[0], canvases[w], "canvas %d:" % w)
    at = h.get_collider_pose(ALPHA)
    assert at == cdm.pose(h.get_colliders(), h.get_colliders(), ALPHA)  # (a static list)
    background = cdm.draw_colliders(cdm.clear_screen(cdm.EGG_SIZE, cdm.CLEAR), at, cdm.EGG_STYLES_UNDER, ORIGIN, "under")
    want = render_model.composite(background.copy(), canvases, envs, render_model.DEFAULT_RENDER, ORIGIN)
    # (the parent's composite on a new background -- and on the old one it is the parent's draw)
    assert same_bits(render_model.composite(cdm.clear_screen(cdm.EGG_SIZE, cdm.CLEAR), canvases, envs, render_model.DEFAULT_RENDER, ORIGIN), plain,
                     "model composite against the plain draw:")
    assert same_bits(image, want, "under the eggs:") and not same_bits(image, plain, "against the plain draw:")


def test_over_the_eggs_and_both_layers(egg, scene):
    from oracle import render_model
    h = scene
    plain, canvases, envs = _parent_draw(h)
    h.set_collider_styles(cdm.EGG_STYLES_OVER)
    at = h.get_collider_pose(ALPHA)
    image = h.draw(cdm.EGG_SIZE, ORIGIN, interpolation_alpha=ALPHA, clear=cdm.CLEAR)
    assert same_bits(image, cdm.draw_colliders(plain, at, cdm.EGG_STYLES_OVER, ORIGIN, "over"), "over the eggs:")
    h.set_collider_styles(cdm.EGG_STYLES_BOTH)
    image = h.draw(cdm.EGG_SIZE, ORIGIN, interpolation_alpha=ALPHA, clear=cdm.CLEAR)
    under = cdm.draw_colliders(cdm.clear_screen(cdm.EGG_SIZE, cdm.CLEAR), at, cdm.EGG_STYLES_BOTH, ORIGIN, "under")
    middle = render_model.composite(under.copy(), canvases, envs, render_model.DEFAULT_RENDER, ORIGIN)
    assert same_bits(image, cdm.draw_colliders(middle, at, cdm.EGG_STYLES_BOTH, ORIGIN, "over"), "both layers:")
    assert h.get_collider_styles() == _as_stored(cdm.EGG_STYLES_BOTH)


def test_interpolation_follows_the_particles_rule(egg):
    h = _relaxed(egg, cdm.MOVING)
    h.set_collider_motion(cdm.MOVING_MOTION)
    h.set_collider_spin(cdm.MOVING_SPIN)
    h.set_collider_styles(cdm.MOVING_STYLES)
    h.add(600.0, 600.0, 24.0, 8.0, None, None, 50, 15)  # (a step wants particles; these stay out of the picture)
    for _ in range(2):
        h.step(H60, 2, 3)
    before = h.get_colliders()
    assert h.update(0.021, H60, 2, 3) == 1  # the third step; leaves an interpolation_alpha of 0.26
    after = h.get_colliders()
    own = h.interpolation_alpha
    assert 0.0 < own < 1.0 and before != after and before != [c + ("both",) for c in cdm.MOVING]

    def poses_and_draws(last, cur):
        for t in cdm.MOVING_TS:
            want = cdm.pose(last, cur, own if t is None else t)
            assert h.get_collider_pose(t) == want, t
            image = h.draw(cdm.SIZE, ZERO, interpolation_alpha=t, clear=cdm.CLEAR)
            assert same_bits(image, cdm.frame(cdm.SIZE, cdm.CLEAR, last, cur, cdm.MOVING_STYLES, ZERO, own if t is None else t), "t = %r:" % (t,))

    h.set_collider_styles([])
    assert same_bits(h.draw(cdm.SIZE, ZERO, clear=cdm.CLEAR), cdm.clear_screen(cdm.SIZE, cdm.CLEAR), "no egg in the picture:")
    h.set_collider_styles(cdm.MOVING_STYLES)
    poses_and_draws(before, after)
    assert h.get_collider_pose(0.0) == before and h.get_collider_pose(1.0) == after and h.get_collider_pose(0.35) != h.get_collider_pose(1.0)
    # the setters that do not move the list leave both lists alone
    h.set_collider_motion(cdm.MOVING_MOTION)
    h.set_collider_spin(h.get_collider_spin())
    h.set_collider_surfaces([0.5, None])
    poses_and_draws(before, after)
    # a failed step too: a body with loads off is refused
    h.set_collider_bodies([(1.0, 0.0), None])
    with pytest.raises(egg.EggError):
        h.step(H60, 2, 3)
    assert h.get_colliders() == after
    poses_and_draws(before, after)
    h.set_collider_bodies([])
    # one more committed step moves both lists on
    h.step(H60, 2, 3)
    assert h.get_collider_pose(0.0) == after and h.get_collider_pose(1.0) == h.get_colliders() != after
    # a teleport is not interpolated: set_colliders of the same list sets both
    now = h.get_colliders()
    h.set_colliders(now)
    assert h.get_colliders() == now and h.get_collider_styles() == [None, None]
    for t in cdm.MOVING_TS:  # (p * (1 - t) + p * t is p up to one rounding: the rule is the mix, evaluated as it stands)
        at = h.get_collider_pose(t)
        assert at == cdm.pose(now, now, own if t is None else t), t
        assert all(a[0] == b[0] and np.allclose(a[1:5], b[1:5], rtol=4e-16, atol=0.0) for a, b in zip(at, now)), t
    assert h.get_collider_pose(0.0) == now and h.get_collider_pose(1.0) == now


def test_nothing_is_launched_for_nothing(egg):
    def delta(h):
        before = h.stats()["kernel_launches"]
        h.draw(cdm.EGG_SIZE, ORIGIN, interpolation_alpha=ALPHA, clear=cdm.CLEAR)
        return h.stats()["kernel_launches"] - before

    for steps in (0, 1):  # before the first step (only the clear) and with the eggs drawn
        never = _egg_handler(egg, steps)
        delta(never)  # (the first draw builds the density texture besides)
        base = delta(never)
        h = _egg_handler(egg, steps)
        delta(h)
        assert delta(h) == base
        for styles, more in (([], 0), ([None] * 3, 0), ([{"fill": (1, 1, 1, 0.0), "line": (1, 1, 1, 1), "line_width": 0.0}] * 3, 0),
                             (cdm.EGG_STYLES_UNDER, 1), (cdm.EGG_STYLES_OVER, 1), (cdm.EGG_STYLES_BOTH, 2), ([], 0)):
            h.set_collider_styles(styles)
            assert delta(h) == base + more, (steps, styles)


def test_refused_styles_name_the_collider_and_change_nothing(egg):
    from egg_fluid_simulation_amd import _ffi
    h = _relaxed(egg, cdm.EGG_COLLIDERS, cdm.EGG_STYLES_BOTH)
    stored = h.get_collider_styles()
    image = h.draw(cdm.SIZE, ORIGIN, clear=cdm.CLEAR)
    for n in (1, 2, 4):
        with pytest.raises(egg.EggError, match="n = %d, the list holds 3" % n):
            h.set_collider_styles([None] * n)

    def record(**kw):  # the library's own checks, behind the wrapper's
        arr = (_ffi.EggColliderStyle * 3)()
        for k in range(3):
            arr[k].fill[:] = (0.5, 0.5, 0.5, 0.5)
            arr[k].line_width = 2.0
        for name, v in kw.items():
            if isinstance(v, tuple):
                getattr(arr[1], name)[v[0]] = v[1]
            else:
                setattr(arr[1], name, v)
        return arr

    for kw, text in ((dict(fill=(0, 1.5)), "fill component 0"), (dict(fill=(3, float("nan"))), "fill component 3"),
                     (dict(line=(2, -0.1)), "line component 2"), (dict(line=(1, float("inf"))), "line component 1"),
                     (dict(line_width=64.5), "line width"), (dict(line_width=-1.0), "line width"), (dict(line_width=float("nan")), "line width"),
                     (dict(layer=2), "layer 2"), (dict(layer=-1), "layer -1")):
        rc = h._c("set_collider_styles")(3, record(**kw))
        assert rc == _ffi.EGG_ERR_INVALID_ARGUMENT, kw
        message = h._c("last_error")().decode()
        assert "collider 1" in message and text in message, message
    assert h._c("set_collider_styles")(3, None) == _ffi.EGG_ERR_INVALID_ARGUMENT
    assert h.get_collider_styles() == stored
    assert same_bits(h.draw(cdm.SIZE, ORIGIN, clear=cdm.CLEAR), image, "after the refusals:")
    # refused while a step is in flight; accepted in exact order, where there is no list to draw
    e = egg.SimulationHandler()
    e.add(300.0, 300.0, 50, 15)
    e.set_collider_styles([])
    with pytest.raises(egg.EggError, match="n = 1, the list holds 0"):
        e.set_collider_styles([None])
    e.step_begin(H60, 2, 3)
    with pytest.raises(egg.EggError, match="in flight"):
        e.set_collider_styles([])
    e.step_end(True)
    assert e.get_collider_styles() == [] and e.get_collider_pose() == []
