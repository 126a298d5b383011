"""CPU model of the relaxed pass with static colliders (egg_set_colliders; DESIGN.md section 2.7, "Colliders").  Test helper,
not collected.

ColliderModel is tests/cohesion_model.py's CohesiveModel (so one model covers cohesion off and on) whose relaxed passes
end with step 5b: the position every particle of the type has just got -- whether or not a pair fired for it -- goes
through the colliders of `colliders` whose mask covers the type, in list order, each on the result of the one before.
With r the particle's radius and i its 0-based index among the particles of its type:

  half_plane (nx, ny, off)   s = (nx x + ny y) - (off + r); s < 0: x = x - s nx, y = y - s ny.  (nx, ny) is normalised once,
                             when the list is set: len = sqrt(nx nx + ny ny), stored nx / len, ny / len.
  disc (cx, cy, R)           dx = x - cx, dy = y - cy, d2 = dx dx + dy dy, m = R + r; d2 < m m: d = sqrt(d2),
                             (ux, uy) = (dx / d, dy / d) -- DIRS[i & 7] when d2 == 0 --, x = cx + ux m, y = cy + uy m.
  container (cx, cy, R)      m = R - r, 0 if that is negative; d2 > m m: d = sqrt(d2), x = cx + (dx / d) m, y = cy + (dy / d) m.
  segment (x0, y0, x1, y1)   ex = x1 - x0, ey = y1 - y0, l2 = ex ex + ey ey, t = l2 == 0 ? 0 : ((x - x0) ex + (y - y0) ey) / l2
                             clamped to [0, 1], q = (x0 + t ex, y0 + t ey); then the disc rule with centre q and R = 0.

numpy float64 element-wise in exactly this order; every comparison is false for a NaN.  A HIT is one collider moving one
particle in one pass (its condition held); `collider_hits` counts them per type over all steps.  Written from the
definition, not from the kernel."""
import math

import numpy as np

from cohesion_model import CohesiveModel
from relaxed_model import DIRS, rm

KINDS = ("half_plane", "disc", "container", "segment")
TYPES = {"white": 1, "yolk": 2, "both": 3}


def normalise(colliders):
    """the list as the library stores it: tuples (kind, p0, p1, p2, p3, mask), a half-plane's normal normalised"""
    out = []
    for c in colliders:
        c = tuple(c)
        types = "both"
        if isinstance(c[-1], str):
            c, types = c[:-1], c[-1]
        kind, p = c[0], [float(v) for v in c[1:]]
        assert kind in KINDS and len(p) == (4 if kind == "segment" else 3)
        if kind == "half_plane":
            ln = math.sqrt(p[0] * p[0] + p[1] * p[1])
            p[0], p[1] = p[0] / ln, p[1] / ln
        out.append((kind, *(p + [0.0])[:4], TYPES[types]))
    return out


def _disc(x, y, cx, cy, m, idx):
    dx = x - cx
    dy = y - cy
    d2 = dx * dx + dy * dy
    hit = d2 < m * m
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.sqrt(d2)
        ux = np.where(d2 == 0.0, DIRS[idx & 7, 0], dx / d)
        uy = np.where(d2 == 0.0, DIRS[idx & 7, 1], dy / d)
        return np.where(hit, cx + ux * m, x), np.where(hit, cy + uy * m, y), hit


def project(x, y, r, colliders, type_bit, idx=None):
    """step 5b over one particle type (0-based arrays; colliders as normalise() returns them).  Returns (x, y, hits)."""
    x = np.array(x, dtype=np.float64)
    y = np.array(y, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    idx = np.arange(len(x)) if idx is None else np.asarray(idx, dtype=np.int64)
    hits = 0
    for kind, p0, p1, p2, p3, mask in colliders:
        if not mask & type_bit:
            continue
        if kind == "half_plane":
            s = (p0 * x + p1 * y) - (p2 + r)
            hit = s < 0.0
            x, y = np.where(hit, x - s * p0, x), np.where(hit, y - s * p1, y)
        elif kind == "disc":
            x, y, hit = _disc(x, y, p0, p1, p2 + r, idx)
        elif kind == "container":
            m = p2 - r
            m = np.where(m < 0.0, 0.0, m)
            dx = x - p0
            dy = y - p1
            d2 = dx * dx + dy * dy
            hit = d2 > m * m
            with np.errstate(divide="ignore", invalid="ignore"):
                d = np.sqrt(d2)
                x, y = np.where(hit, p0 + (dx / d) * m, x), np.where(hit, p1 + (dy / d) * m, y)
        else:
            ex = p2 - p0
            ey = p3 - p1
            l2 = ex * ex + ey * ey
            t = np.zeros_like(x) if l2 == 0.0 else ((x - p0) * ex + (y - p1) * ey) / l2
            t = np.where(t < 0.0, 0.0, t)
            t = np.where(t > 1.0, 1.0, t)
            x, y, hit = _disc(x, y, p0 + t * ex, p1 + t * ey, 0.0 + r, idx)
        hits += int(np.count_nonzero(hit))
    return x, y, hits


class ColliderModel(CohesiveModel):
    """CohesiveModel whose relaxed passes project through `colliders` (set_colliders; the list may change between steps)."""

    def __init__(self, white_config=None, yolk_config=None, relaxed=True, relaxation=None, cohesion=False):
        self.colliders = []
        self.collider_hits = [0, 0]
        kw = {} if relaxation is None else dict(relaxation=relaxation)
        super().__init__(white_config, yolk_config, relaxed, cohesion=cohesion, **kw)

    def set_colliders(self, colliders):
        self.colliders = normalise(colliders)

    def _solve_collision(self, particles, n_particles, *args, **kwargs):
        out = super()._solve_collision(particles, n_particles, *args, **kwargs)
        if self.relaxed and self.colliders and n_particles:
            which = 0 if particles is self._white_data else 1
            base = [rm.offset(p) for p in range(1, n_particles + 1)]
            x, y, hits = project([particles[i + rm.X] for i in base], [particles[i + rm.Y] for i in base],
                                 [particles[i + rm.RADIUS] for i in base], self.colliders, 1 << which)
            for k, i in enumerate(base):
                particles[i + rm.X] = float(x[k])
                particles[i + rm.Y] = float(y[k])
            self.collider_hits[which] += hits
        return out
