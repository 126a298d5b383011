"""CPU model of the relaxed pass with wall colliders (EGG_COLLIDER_WALL; DESIGN.md section 2.7, "Walls").  Test helper, not
collected.

WallModel is tests/surface_model.py's SurfaceModel (so one model covers cohesion, colliders, forces, viscosity and surfaces
off and on) whose step 5b knows a fifth kind: `("wall", x0, y0, x1, y1[, types])`, a two-sided thin wall.  A particle that
starts a sub-step on one side cannot end a pass on the other.  With (x, y) the position the collider loop holds, prev the
particle's position at the start of the sub-step (PX / PY, what the pre-solve wrote and step 5c reads), r its radius:

  ex = x1 - x0, ey = y1 - y0, l2 = ex ex + ey ey
  t  = l2 == 0 ? 0 : ((x - x0) ex + (y - y0) ey) / l2, clamped to [0, 1]                    (as the segment)
  qx = x0 + t ex, qy = y0 + t ey, dx = x - qx, dy = y - qy, d2 = dx dx + dy dy, m = 0.0 + r   (as the segment)
  a0 = ex (prev.y - y0) - ey (prev.x - x0)        the side of the sub-step's start
  a1 = ex (y - y0)      - ey (x - x0)             the side of the position now
  opp = (a0 > 0 and a1 <= 0) or (a0 < 0 and a1 >= 0); caught = false
  opp:  u = a0 / (a0 - a1), hx = prev.x + u (x - prev.x), hy = prev.y + u (y - prev.y),
        tc = ((hx - x0) ex + (hy - y0) ey) / l2, caught = tc >= 0 and tc <= 1
  caught:      l = sqrt(l2), d = sqrt(d2), (nx, ny) = a0 > 0 ? ((-ey) / l, ex / l) : (ey / l, (-ex) / l),
               x = qx + nx m, y = qy + ny m; a hit; for step 5c n = (nx, ny), pen = m + d
  not caught:  the disc rule with centre (qx, qy) and R = 0, exactly as the segment.

A CATCH is one wall putting one particle back in one pass; `wall_catches` counts them per type over all steps (the library
has no such counter: a catch is a hit) and `caught_ever` holds, per type, the 0-based indices of the particles a wall has
caught at least once.  numpy float64 element-wise in exactly this order; every comparison is false for a NaN.  Written
from the definition, not from the kernel."""
import math

import numpy as np

import surface_model as sm
from cohesion_model import CohesiveModel
from collider_model import TYPES
from relaxed_model import rm
from surface_model import SurfaceModel

KINDS = ("half_plane", "disc", "container", "segment", "wall")


def normalise(colliders):
    """collider_model.normalise() with the fifth kind: tuples (kind, p0, p1, p2, p3, mask)"""
    out = []
    for c in colliders:
        c = tuple(c)
        types = "both"
        if isinstance(c[-1], str):
            c, types = c[:-1], c[-1]
        kind, p = c[0], [float(v) for v in c[1:]]
        assert kind in KINDS and len(p) == (4 if kind in ("segment", "wall") else 3)
        if kind == "half_plane":
            ln = math.sqrt(p[0] * p[0] + p[1] * p[1])
            p[0], p[1] = p[0] / ln, p[1] / ln
        out.append((kind, *(p + [0.0])[:4], TYPES[types]))
    return out


def wall(x, y, r, px, py, p, idx):
    """the rule of one wall p = (x0, y0, x1, y1) over the lanes (element-wise).  Returns (x, y, hit, nx, ny, pen, caught)."""
    x0, y0, x1, y1 = p
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ex = x1 - x0
        ey = y1 - y0
        l2 = ex * ex + ey * ey
        t = np.zeros_like(x) if l2 == 0.0 else ((x - x0) * ex + (y - y0) * ey) / l2
        t = np.where(t < 0.0, 0.0, t)
        t = np.where(t > 1.0, 1.0, t)
        qx = x0 + t * ex
        qy = y0 + t * ey
        dx = x - qx
        dy = y - qy
        d2 = dx * dx + dy * dy
        m = 0.0 + r
        a0 = ex * (py - y0) - ey * (px - x0)
        a1 = ex * (y - y0) - ey * (x - x0)
        opp = ((a0 > 0.0) & (a1 <= 0.0)) | ((a0 < 0.0) & (a1 >= 0.0))
        u = a0 / (a0 - a1)
        hx = px + u * (x - px)
        hy = py + u * (y - py)
        tc = ((hx - x0) * ex + (hy - y0) * ey) / np.float64(l2)
        caught = opp & (tc >= 0.0) & (tc <= 1.0)
        l = np.sqrt(np.float64(l2))
        d = np.sqrt(d2)
        nx = np.where(a0 > 0.0, (-ey) / l, ey / l)
        ny = np.where(a0 > 0.0, ex / l, (-ex) / l)
        cx = qx + nx * m
        cy = qy + ny * m
        # not caught: the segment's rule
        sx, sy, shit, sux, suy, spen = sm._disc(x, y, qx, qy, m, idx)
    return (np.where(caught, cx, sx), np.where(caught, cy, sy), caught | shit, np.where(caught, nx, sux),
            np.where(caught, ny, suy), np.where(caught, m + d, spen), caught)


def project(x, y, r, px, py, h, colliders, surfaces, type_bit, idx=None):
    """steps 5b and 5c over one particle type, the list taken collider by collider: a wall by wall(), every other kind by
    surface_model.project() on a list of one.  Returns (x, y, hits, grips, sticks, catches)."""
    x = np.array(x, dtype=np.float64)
    y = np.array(y, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    px = np.asarray(px, dtype=np.float64)
    py = np.asarray(py, dtype=np.float64)
    idx = np.arange(len(x)) if idx is None else np.asarray(idx, dtype=np.int64)
    surfaces = list(surfaces) if surfaces else [sm.DEFAULT] * len(colliders)
    assert len(surfaces) == len(colliders)
    hits = grips = sticks = catches = 0
    ever = np.zeros(len(x), dtype=bool)
    for collider, surface in zip(colliders, surfaces):
        kind, p0, p1, p2, p3, mask = collider
        if kind != "wall":
            x, y, h1, g1, s1 = sm.project(x, y, r, px, py, h, [collider], [surface], type_bit, idx)
            hits, grips, sticks = hits + h1, grips + g1, sticks + s1
            continue
        if not mask & type_bit:
            continue
        x, y, hit, nx, ny, pen, caught = wall(x, y, r, px, py, (p0, p1, p2, p3), idx)
        hits += int(np.count_nonzero(hit))
        catches += int(np.count_nonzero(caught))
        ever |= caught
        x, y, on, stuck = sm.grip(x, y, px, py, h, surface, nx, ny, pen, hit)
        grips += int(np.count_nonzero(on))
        sticks += int(np.count_nonzero(stuck))
    return x, y, hits, grips, sticks, catches, ever


class WallModel(SurfaceModel):
    """SurfaceModel whose collider projection knows the wall and counts its catches per type."""

    def __init__(self, white_config=None, yolk_config=None, relaxed=True, relaxation=None, cohesion=False):
        self.wall_catches = [0, 0]
        self.caught_ever = [set(), set()]
        super().__init__(white_config, yolk_config, relaxed, relaxation=relaxation, cohesion=cohesion)

    def set_colliders(self, colliders):
        self.colliders = normalise(colliders)
        self.surfaces = []

    def _solve_collision(self, particles, n_particles, *args, **kwargs):
        # SurfaceModel._solve_collision with this module's project()
        out = CohesiveModel._solve_collision(self, particles, n_particles, *args, **kwargs)
        if self.relaxed and self.colliders and n_particles:
            which = 0 if particles is self._white_data else 1
            base = [rm.offset(p) for p in range(1, n_particles + 1)]

            def col(off):
                return [particles[i + off] for i in base]

            x, y, hits, grips, sticks, catches, ever = project(col(rm.X), col(rm.Y), col(rm.RADIUS), col(rm.PX), col(rm.PY),
                                                         self._sub_delta, self.colliders, self.surfaces, 1 << which)
            for k, i in enumerate(base):
                particles[i + rm.X] = float(x[k])
                particles[i + rm.Y] = float(y[k])
            self.collider_hits[which] += hits
            self.collider_grips[which] += grips
            self.grip_sticks[which] += sticks
            self.wall_catches[which] += catches
            self.caught_ever[which].update(int(k) for k in np.flatnonzero(ever))
        return out
