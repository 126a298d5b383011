"""numpy model of the colliders in the picture ("Collider styles"; include/eggsim.h): the pose a frame
draws and the one kernel that draws it, egg_render_colliders_kernel of csrc/eggsim_render.hip.  The same expressions in
the same order -- float64 for the distance, float32 for the blend, nothing contracted -- over EVERY pixel and EVERY
collider: there is no culling here, which is what the kernel's tile culling is held against, bit for bit.

Colliders are the tuples get_colliders returns, `(kind, parameters..., types)`; styles are what set_collider_styles takes,
`None` or a dict with the keys fill, line, line_width, layer and its defaults.  `wrong` names one deliberately wrong rule
(WRONG_RULES): the tests show that the scenes of the GPU tests tell each of them from the right one.

The module also holds the scenes the CPU test and the GPU tests share."""
import numpy as np

INSIDE = {"half_plane": True, "disc": True, "container": True, "segment": False, "wall": False}
LAYERS = {"under": 0, "over": 1, 0: 0, 1: 1}
STYLE_DEFAULTS = {"fill": (0.0, 0.0, 0.0, 0.0), "line": (0.0, 0.0, 0.0, 0.0), "line_width": 0.0, "layer": "under"}
WRONG_RULES = ("list order reversed", "layer ignored", "container sign flipped", "t not clamped", "pose not mixed",
               "line half-width doubled", "zero coverage blended")


def _params(c):
    p = [float(v) for v in c[1:] if not isinstance(v, str)]
    return p + [0.0] * (4 - len(p))


def pose(last, cur, t, wrong=None):
    """every parameter last * (1.0 - t) + cur * t in float64, t clamped to [0, 1]; kind and types from `cur`"""
    t = float(t)
    if wrong != "t not clamped":
        t = min(max(t, 0.0), 1.0)
    if wrong == "pose not mixed":
        t = 1.0
    out = []
    for a, b in zip(last, cur):
        n = len([v for v in b[1:] if not isinstance(v, str)])
        mixed = [pa * (1.0 - t) + pb * t for pa, pb in zip(_params(a), _params(b))]
        out.append((b[0],) + tuple(mixed[:n]) + tuple(v for v in b[1:] if isinstance(v, str)))
    return out


def style_of(style):
    """a style with its defaults, colours and width as float32; None stays None"""
    if style is None:
        return None
    s = dict(STYLE_DEFAULTS, **style)
    return dict(fill=np.asarray(s["fill"], np.float32), line=np.asarray(s["line"], np.float32),
                line_width=np.float32(s["line_width"]), layer=LAYERS[s["layer"]])


def visible(collider, style):
    s = style_of(style)
    return s is not None and bool((s["fill"][3] > 0 and INSIDE[collider[0]]) or (s["line"][3] > 0 and s["line_width"] > 0))


def signed_distance(collider, wx, wy, wrong=None):
    """float64 signed distance of the points (wx, wy) (broadcast) from one collider: negative on the solid side"""
    kind, p = collider[0], [np.float64(v) for v in _params(collider)]
    with np.errstate(all="ignore"):
        if kind == "half_plane":
            return (p[0] * wx + p[1] * wy) - p[2]
        if kind in ("segment", "wall"):
            ex, ey = p[2] - p[0], p[3] - p[1]
            l2 = ex * ex + ey * ey
            t = np.zeros(np.broadcast(wx, wy).shape) if l2 == 0.0 else ((wx - p[0]) * ex + (wy - p[1]) * ey) / l2
            t = np.where(t < 0.0, 0.0, t)
            t = np.where(t > 1.0, 1.0, t)
            qx, qy = p[0] + t * ex, p[1] + t * ey
            ddx, ddy = wx - qx, wy - qy
            return np.sqrt(ddx * ddx + ddy * ddy)
        dx, dy = wx - p[0], wy - p[1]
        d = np.sqrt(dx * dx + dy * dy)
        obstacle = kind == "disc" or (kind == "container" and wrong == "container sign flipped")
        return d - p[2] if obstacle else p[2] - d


def blend_alpha(dst, rgb, alpha):
    """the composite's "alpha" blend in float32: dst (..., 4), rgb (3,) float32, alpha (...) float32"""
    one = np.float32(1.0)
    k = one - alpha
    out = np.empty_like(dst)
    for q in range(3):
        out[..., q] = rgb[q] * alpha + dst[..., q] * k
    out[..., 3] = alpha + dst[..., 3] * k
    return out


def draw_colliders(screen, pose, styles, origin, layer, wrong=None):
    """the visible colliders of `layer` ("under" / "over") in list order onto a copy of `screen` ((H, W, 4) float32);
    world = pixel centre + origin.  styles None or []: nothing is drawn."""
    out = np.array(screen, dtype=np.float32, copy=True)
    if not styles:
        return out
    assert len(styles) == len(pose)
    h, w = out.shape[:2]
    wx = ((np.arange(w, dtype=np.float64) + 0.5) + np.float64(origin[0]))[None, :]
    wy = ((np.arange(h, dtype=np.float64) + 0.5) + np.float64(origin[1]))[:, None]
    order = list(zip(pose, styles))
    if wrong == "list order reversed":
        order.reverse()
    for c, style in order:
        s = style_of(style)
        if not visible(c, style) or (s["layer"] != LAYERS[layer] and wrong != "layer ignored"):
            continue
        sd = signed_distance(c, wx, wy, wrong) + np.zeros((h, w))
        if INSIDE[c[0]] and s["fill"][3] > 0:
            cf = np.fmin(np.fmax(0.5 - sd, 0.0), 1.0).astype(np.float32)
            new = blend_alpha(out, s["fill"], s["fill"][3] * cf)
            out = new if wrong == "zero coverage blended" else np.where((cf > 0)[..., None], new, out)
        if s["line_width"] > 0 and s["line"][3] > 0:
            half = 0.5 + 0.5 * np.float64(s["line_width"])
            if wrong == "line half-width doubled":
                half = 0.5 + np.float64(s["line_width"])
            cl = np.fmin(np.fmax(half - np.abs(sd), 0.0), 1.0).astype(np.float32)
            new = blend_alpha(out, s["line"], s["line"][3] * cl)
            out = new if wrong == "zero coverage blended" else np.where((cl > 0)[..., None], new, out)
    return out


def clear_screen(size, clear):
    return np.broadcast_to(np.asarray(clear, np.float32), (size[1], size[0], 4)).copy()


def frame(size, clear, last, cur, styles, origin, t, wrong=None):
    """a frame without eggs: the clear, then both layers at the pose of t"""
    at = pose(last, cur, t, wrong)
    under = draw_colliders(clear_screen(size, clear), at, styles, origin, "under", wrong)
    return draw_colliders(under, at, styles, origin, "over", wrong)


# ------------------------------------------------------------------------------------------------ shared scenes
SIZE = (100, 84)  # 16 px tiles: the right and the bottom tiles are partial
CLEAR = (0.1, 0.2, 0.3, 1.0)
CLEAR_NEGATIVE_ZERO = (-0.0, 0.0, -0.0, 0.0)
FAR_ORIGIN = (1.0e6 + 0.25, -2.0e6)


def shifted(colliders, origin):
    """the list moved by `origin` (a half-plane's offset by n . origin)"""
    out = []
    for c in colliders:
        p, tail = [v for v in c[1:] if not isinstance(v, str)], tuple(v for v in c[1:] if isinstance(v, str))
        if c[0] == "half_plane":
            p = [p[0], p[1], p[2] + (p[0] * origin[0] + p[1] * origin[1])]
        else:
            p = [v + origin[q % 2] for q, v in enumerate(p)] if c[0] in ("segment", "wall") else [p[0] + origin[0], p[1] + origin[1], p[2]]
        out.append((c[0],) + tuple(p) + tail)
    return out


# one of each kind (screen coordinates, origin (0, 0)); widths 0, 1.5 and 64; a fill only, a line only, both layers
ALONE = [
    ("half_plane", 0.6, -0.8, -40.0),           # oblique: solid below y = 0.75 x + 50
    ("disc", 40.0, 40.0, 11.0),                 # its rim passes 0.31 px from the tile corner (48, 48)
    ("disc", 70.3, 20.6, 0.2),                  # smaller than a pixel
    ("container", 50.0, 42.0, 38.0),            # smaller than the screen
    ("segment", 10.0, 70.0, 57.3, 23.9),        # ends inside a tile
    ("wall", 85.0, 60.0, 85.0, 60.0),           # degenerate: l2 == 0, a dot
    ("disc", 500.0, -300.0, 20.0),              # entirely off screen
    ("segment", 5.0, 5.0, 95.0, 5.0),           # no style
]
ALONE_STYLES = [
    {"fill": (0.2, 0.5, 0.3, 0.6), "line": (1.0, 1.0, 1.0, 0.8), "line_width": 1.5, "layer": "under"},
    {"fill": (0.9, 0.2, 0.1, 1.0), "layer": "over"},                                        # fill only (width 0)
    {"fill": (1.0, 1.0, 0.0, 1.0), "line": (0.0, 0.0, 0.0, 0.5), "line_width": 1.5, "layer": "over"},
    {"fill": (0.1, 0.1, 0.4, 0.5), "line": (0.8, 0.8, 1.0, 0.3), "line_width": 64.0, "layer": "under"},  # wider than a tile
    {"fill": (1.0, 0.0, 1.0, 1.0), "line": (1.0, 0.5, 0.0, 0.9), "line_width": 1.5, "layer": "over"},  # (a segment's fill is ignored)
    {"line": (0.0, 1.0, 1.0, 1.0), "line_width": 1.5, "layer": "under"},                    # line only
    {"fill": (1.0, 1.0, 1.0, 1.0), "line": (1.0, 1.0, 1.0, 1.0), "line_width": 64.0, "layer": "over"},
    None,
]

# a full list: 64 thin segments across the screen, all in one layer, so that collider k is bit k of the kernel's mask;
# 0, 31, 32 and 63 -- the ends of both halves of the mask -- are styled differently from the rest
FULL = [("segment", 1.5 * k, 0.0, 1.5 * k + 5.0, 84.0) for k in range(64)]
FULL_STYLES = [{"line": (1.0, 0.2, 0.1, 1.0), "line_width": 3.0, "layer": "under"} if k in (0, 31, 32, 63) else
               {"line": (0.2 + 0.01 * k, 1.0, 1.0 - 0.01 * k, 0.5), "line_width": 1.5, "layer": "under"} for k in range(64)]

# the interpolation scene: a wall with a motion and a segment with a spin
MOVING = [("wall", 20.0, 10.0, 30.0, 70.0), ("segment", 50.0, 40.0, 90.0, 40.0)]
MOVING_MOTION = [(240.0, 60.0), None]
MOVING_SPIN = [None, (50.0, 40.0, 9.0)]
MOVING_STYLES = [{"line": (1.0, 1.0, 1.0, 1.0), "line_width": 1.5, "layer": "under"},
                 {"line": (1.0, 0.0, 0.0, 0.7), "line_width": 1.5, "layer": "over"}]
MOVING_TS = (0.0, 0.35, 1.0, 1.7, None)

# the egg scene: one egg of 50 + 15 particles falls onto a half-plane floor; a disc over it, the floor under it
# (the density blobs of an egg reach some 45 px beyond its particles: this scene states a screen of its own, 260 x 212 px,
# again no multiple of the tile, on which the floor, the disc and the ring show beside the egg as well as under it)
EGG_SIZE = (260, 212)
EGG = dict(at=(130.0, 95.0), radii=(24.0, 8.0), counts=(50, 15), gravity=("uniform", 0.0, 400.0), steps=4)
EGG_COLLIDERS = [("half_plane", 0.0, -1.0, -115.0), ("disc", 205.0, 100.0, 14.0), ("container", 130.0, 100.0, 98.0)]
EGG_STYLES_UNDER = [{"fill": (0.3, 0.25, 0.2, 1.0), "line": (1.0, 1.0, 1.0, 1.0), "line_width": 1.5, "layer": "under"},
                    {"fill": (0.1, 0.6, 0.9, 0.5), "layer": "under"},
                    {"line": (0.5, 0.5, 0.5, 0.5), "line_width": 1.5, "layer": "under"}]
EGG_STYLES_OVER = [dict(s, layer="over") for s in EGG_STYLES_UNDER]
EGG_STYLES_BOTH = [EGG_STYLES_UNDER[0], EGG_STYLES_OVER[1], EGG_STYLES_UNDER[2]]
# for several handles or ranks: a second egg beyond a cut at x = 150, and the disc moving, so that the pose is a mix
EGG_SECOND = (175.0, 95.0)
EGG_CUT = 150.0
EGG_DISC_MOTION = [None, (90.0, -30.0), None]
EGG_VIEW = dict(origin=(3.0, -2.0), alpha=0.35)


def play_egg_scene(sim, eggs=(EGG["at"],), motion=None, steps=EGG["steps"]):
    """the egg scene on anything with the SimulationHandler surface"""
    sim.set_solver_order("relaxed")
    sim.set_colliders(EGG_COLLIDERS)
    sim.set_forces([EGG["gravity"]])
    if motion is not None:
        sim.set_collider_motion(motion)
    for at in eggs:
        sim.add(at[0], at[1], EGG["radii"][0], EGG["radii"][1], None, None, EGG["counts"][0], EGG["counts"][1])
    for _ in range(steps - 1):
        sim.step(1 / 60, 2, 3)
    assert sim.update(0.021, 1 / 60, 2, 3) == 1  # the last step; leaves an interpolation_alpha of 0.26


def probe_egg_scene(sim):
    """what the group and the sharded tests compare with one handle: the plain draw, the styled one, poses and styles"""
    view = dict(screen_size=EGG_SIZE, origin=EGG_VIEW["origin"], clear=CLEAR)
    sim.set_collider_styles([])
    out = dict(plain=sim.draw(interpolation_alpha=EGG_VIEW["alpha"], **view))
    sim.set_collider_styles(EGG_STYLES_BOTH)
    out["styled"] = sim.draw(interpolation_alpha=EGG_VIEW["alpha"], **view)
    out["styled, own alpha"] = sim.draw(**view)
    out["poses"] = [sim.get_collider_pose(t) for t in (0.0, EGG_VIEW["alpha"], 1.0, 1.7, None)]
    out["lists"] = (sim.get_colliders(), sim.get_collider_styles())
    sim.set_colliders(sim.get_colliders())  # both lists are the list now, and nothing is drawn
    out["after set_colliders"] = (sim.get_collider_pose(EGG_VIEW["alpha"]), sim.get_collider_styles(),
                                  sim.draw(interpolation_alpha=EGG_VIEW["alpha"], **view))
    return out
