"""CPU model of the relaxed pass with collider surfaces (egg_set_collider_surfaces; DESIGN.md section 2.7, "Collider
surfaces").  Test helper, not collected.

SurfaceModel is tests/viscosity_model.py's ViscosityModel (so one model covers cohesion, colliders, forces and viscosity off
and on) whose step 5b carries step 5c: every collider k of the list may have a surface (mu_k, vx_k, vy_k), default all
zeros.  Step 5c applies to collider k when its mask covers the type, its condition held in this pass (a hit) and
mu_k > 0.0, right after that collider's projection has been written into (x, y) and before the next collider sees the
result.  With prev the particle's position at the start of the sub-step (PX / PY, what the pre-solve wrote -- the
viscosity pass rewrites them only after the sub-step's last collision pass), h the sub-step, and the projection's own

  half_plane         n = (nx, ny) as stored,                                     pen = -s
  disc and segment   n = (ux, uy) as used by the projection (DIRS[i & 7] at d2 == 0), pen = m - d (a segment has m = 0 + r)
  container          n = (dx / d, dy / d),                                       pen = d - m

  ex = (x - prev.x) - h vx, ey = (y - prev.y) - h vy, dn = ex nx + ey ny, tx = ex - dn nx, ty = ey - dn ny,
  tl2 = tx tx + ty ty; !(tl2 > 0.0): nothing happens, nothing is counted; otherwise tl = sqrt(tl2), lim = mu pen;
  tl <= lim (stick): x = x - tx, y = y - ty; else (slide): f = lim / tl, x = x - tx f, y = y - ty f.

Either branch is one GRIP; `collider_grips` counts them per type over all steps, `grip_sticks` the stick branches among
them.  numpy float64 element-wise in exactly this order; every comparison is false for a NaN.  Written from the
definition, not from the kernel."""
import numpy as np

from cohesion_model import CohesiveModel
from collider_model import ColliderModel
from relaxed_model import DIRS, rm
from viscosity_model import ViscosityModel

DEFAULT = (0.0, 0.0, 0.0)


def normalise(surfaces):
    """the records as the library stores them: (mu, vx, vy) per collider; None is the default, a number is mu"""
    out = []
    for s in surfaces:
        if s is None:
            s = DEFAULT
        elif isinstance(s, (int, float)):
            s = (s, 0.0, 0.0)
        mu, vx, vy = (float(v) for v in s)
        assert mu >= 0.0
        out.append((mu + 0.0, vx + 0.0, vy + 0.0))  # (-0.0 is stored as +0.0)
    return out


def grip(x, y, px, py, h, surface, nx, ny, pen, hit):
    """step 5c of one collider over the lanes `hit` (element-wise).  Returns (x, y, gripped, stuck)."""
    mu, vx, vy = surface
    if not mu > 0.0:
        none = np.zeros(len(x), dtype=bool)
        return x, y, none, none
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ex = (x - px) - h * vx
        ey = (y - py) - h * vy
        dn = ex * nx + ey * ny
        tx = ex - dn * nx
        ty = ey - dn * ny
        tl2 = tx * tx + ty * ty
        on = hit & (tl2 > 0.0)
        tl = np.sqrt(tl2)
        lim = mu * pen
        stick = tl <= lim
        f = lim / tl
        gx = np.where(stick, x - tx, x - tx * f)
        gy = np.where(stick, y - ty, y - ty * f)
    return np.where(on, gx, x), np.where(on, gy, y), on, on & stick


def _disc(x, y, cx, cy, m, idx):
    """the disc rule of collider_model, returning the normal and the depth besides"""
    dx = x - cx
    dy = y - cy
    d2 = dx * dx + dy * dy
    hit = d2 < m * m
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.sqrt(d2)
        ux = np.where(d2 == 0.0, DIRS[idx & 7, 0], dx / d)
        uy = np.where(d2 == 0.0, DIRS[idx & 7, 1], dy / d)
        return np.where(hit, cx + ux * m, x), np.where(hit, cy + uy * m, y), hit, ux, uy, m - d


def project(x, y, r, px, py, h, colliders, surfaces, type_bit, idx=None):
    """steps 5b and 5c over one particle type (0-based arrays; colliders as collider_model.normalise() returns them,
    surfaces as normalise() does, one per collider, or empty for all default).  Returns (x, y, hits, grips, sticks)."""
    x = np.array(x, dtype=np.float64)
    y = np.array(y, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    px = np.asarray(px, dtype=np.float64)
    py = np.asarray(py, dtype=np.float64)
    idx = np.arange(len(x)) if idx is None else np.asarray(idx, dtype=np.int64)
    surfaces = list(surfaces) if surfaces else [DEFAULT] * len(colliders)
    assert len(surfaces) == len(colliders)
    hits = grips = sticks = 0
    for (kind, p0, p1, p2, p3, mask), surface in zip(colliders, surfaces):
        if not mask & type_bit:
            continue
        if kind == "half_plane":
            s = (p0 * x + p1 * y) - (p2 + r)
            hit = s < 0.0
            x, y = np.where(hit, x - s * p0, x), np.where(hit, y - s * p1, y)
            nx, ny, pen = p0, p1, -s
        elif kind == "disc":
            x, y, hit, nx, ny, pen = _disc(x, y, p0, p1, p2 + r, idx)
        elif kind == "container":
            m = p2 - r
            m = np.where(m < 0.0, 0.0, m)
            dx = x - p0
            dy = y - p1
            d2 = dx * dx + dy * dy
            hit = d2 > m * m
            with np.errstate(divide="ignore", invalid="ignore"):
                d = np.sqrt(d2)
                nx, ny, pen = dx / d, dy / d, d - m
                x, y = np.where(hit, p0 + nx * m, x), np.where(hit, p1 + ny * m, y)
        else:
            ex = p2 - p0
            ey = p3 - p1
            l2 = ex * ex + ey * ey
            t = np.zeros_like(x) if l2 == 0.0 else ((x - p0) * ex + (y - p1) * ey) / l2
            t = np.where(t < 0.0, 0.0, t)
            t = np.where(t > 1.0, 1.0, t)
            x, y, hit, nx, ny, pen = _disc(x, y, p0 + t * ex, p1 + t * ey, 0.0 + r, idx)
        hits += int(np.count_nonzero(hit))
        x, y, on, stuck = grip(x, y, px, py, h, surface, nx, ny, pen, hit)
        grips += int(np.count_nonzero(on))
        sticks += int(np.count_nonzero(stuck))
    return x, y, hits, grips, sticks


class SurfaceModel(ViscosityModel):
    """ViscosityModel whose collider projection carries the surfaces (set_collider_surfaces; set_colliders resets them)."""

    def __init__(self, white_config=None, yolk_config=None, relaxed=True, relaxation=None, cohesion=False):
        self.surfaces = []
        self.collider_grips = [0, 0]
        self.grip_sticks = [0, 0]
        self._sub_delta = None
        super().__init__(white_config, yolk_config, relaxed, relaxation=relaxation, cohesion=cohesion)

    def set_colliders(self, colliders):
        super().set_colliders(colliders)
        self.surfaces = []

    def set_collider_surfaces(self, surfaces):
        surfaces = normalise(surfaces)
        assert len(surfaces) in (0, len(self.colliders))
        self.surfaces = surfaces

    def _step(self, delta, n_sub_steps, n_collision_steps, visit_logs=None):
        self._sub_delta = max(delta / n_sub_steps, rm.EPS)  # (h of step 5c: the reference's sub_delta)
        return super()._step(delta, n_sub_steps, n_collision_steps, visit_logs)

    def _solve_collision(self, particles, n_particles, *args, **kwargs):
        # the projection of ColliderModel._solve_collision, replaced: the pass of the classes below it, then 5b with 5c
        out = CohesiveModel._solve_collision(self, particles, n_particles, *args, **kwargs)
        if self.relaxed and self.colliders and n_particles:
            which = 0 if particles is self._white_data else 1
            base = [rm.offset(p) for p in range(1, n_particles + 1)]

            def col(off):
                return [particles[i + off] for i in base]

            x, y, hits, grips, sticks = project(col(rm.X), col(rm.Y), col(rm.RADIUS), col(rm.PX), col(rm.PY), self._sub_delta,
                                                self.colliders, self.surfaces, 1 << which)
            for k, i in enumerate(base):
                particles[i + rm.X] = float(x[k])
                particles[i + rm.Y] = float(y[k])
            self.collider_hits[which] += hits
            self.collider_grips[which] += grips
            self.grip_sticks[which] += sticks
        return out


assert SurfaceModel._solve_collision is not ColliderModel._solve_collision
