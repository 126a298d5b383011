"""CPU model of the relaxed step with force fields (egg_set_forces; DESIGN.md section 2.7, "Forces").  Test helper, not
collected.

ForceModel is tests/collider_model.py's ColliderModel (so one model covers cohesion and colliders both off and on) whose
pre-solve is preceded by the force step.  In every sub-step of a relaxed step, for every particle of a type, with (x, y)
its position at the start of the sub-step, (vx, vy) the velocity the pre-solve is about to damp and im its inverse mass:

  1. !(im > eps): the particle takes no force.
  2. ax = +0.0, ay = +0.0; for every field of `forces` whose mask covers the type, in list order:
       uniform (gx, gy)             ax = ax + gx, ay = ay + gy
       radial (cx, cy, strength, R) dx = cx - x, dy = cy - y, d2 = dx dx + dy dy; d2 < R R and d2 > 0: d = sqrt(d2),
                                    w = 1 - d / R, s = strength w, ax = ax + (dx / d) s, ay = ay + (dy / d) s
       vortex (cx, cy, strength, R) the same dx, dy, d2, d, w, s and condition; ax = ax + (-(dy / d)) s, ay = ay + (dx / d) s
  3. vx = vx + sub_delta ax, vy = vy + sub_delta ay.

numpy float64 element-wise in exactly this order; every comparison is false for a NaN.  `force_acts` counts per type the
(particle, sub-step) pairs for which a bounded field's condition held, over all steps (a uniform field has no condition
and is not counted).  Written from the definition, not from the kernel."""
import numpy as np

from collider_model import TYPES, ColliderModel
from relaxed_model import rm

KINDS = ("uniform", "radial", "vortex")


def normalise(forces):
    """the list as the library stores it: tuples (kind, p0, p1, p2, p3, mask), unused parameters 0"""
    out = []
    for f in forces:
        f = tuple(f)
        types = "both"
        if isinstance(f[-1], str):
            f, types = f[:-1], f[-1]
        kind, p = f[0], [float(v) for v in f[1:]]
        assert kind in KINDS and len(p) == (2 if kind == "uniform" else 4)
        out.append((kind, *(p + [0.0, 0.0])[:4], TYPES[types]))
    return out


def acceleration(x, y, forces, type_bit):
    """step 2 over the particles of one type (forces as normalise() returns them).  Returns (ax, ay, acts)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    ax = np.zeros_like(x)
    ay = np.zeros_like(y)
    acts = 0
    for kind, p0, p1, p2, p3, mask in forces:
        if not mask & type_bit:
            continue
        if kind == "uniform":
            ax = ax + p0
            ay = ay + p1
            continue
        dx = p0 - x
        dy = p1 - y
        d2 = dx * dx + dy * dy
        on = (d2 < p3 * p3) & (d2 > 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            d = np.sqrt(d2)
            w = 1.0 - d / p3
            s = p2 * w
            if kind == "radial":
                ax = np.where(on, ax + (dx / d) * s, ax)
                ay = np.where(on, ay + (dy / d) * s, ay)
            else:
                ax = np.where(on, ax + (-(dy / d)) * s, ax)
                ay = np.where(on, ay + (dx / d) * s, ay)
        acts += int(np.count_nonzero(on))
    return ax, ay, acts


class ForceModel(ColliderModel):
    """ColliderModel whose pre-solve is preceded by the force step over `forces` (set_forces; the list may change between
    steps)."""

    def __init__(self, white_config=None, yolk_config=None, relaxed=True, relaxation=None, cohesion=False):
        self.forces = []
        self.force_acts = [0, 0]
        super().__init__(white_config, yolk_config, relaxed, relaxation=relaxation, cohesion=cohesion)

    def set_forces(self, forces):
        self.forces = normalise(forces)

    def _pre_solve(self, particles, n_particles, damping, delta, should_update_mass, min_mass, max_mass, *rest):
        if self.relaxed and self.forces and n_particles:
            which = 0 if particles is self._white_data else 1
            base = [rm.offset(p) for p in range(1, n_particles + 1)]

            def col(off):
                return np.array([particles[i + off] for i in base], dtype=np.float64)

            # the inverse mass the follow constraint of this sub-step tests (the pre-solve refreshes it on a config change)
            im = 1 / rm.mix(min_mass, max_mass, col(rm.MASS_T)) if should_update_mass else col(rm.INV_MASS)
            free = im > rm.EPS
            ax, ay, _ = acceleration(col(rm.X), col(rm.Y), self.forces, 1 << which)
            _, _, acts = acceleration(col(rm.X)[free], col(rm.Y)[free], self.forces, 1 << which)
            vx = np.where(free, col(rm.VX) + delta * ax, col(rm.VX))
            vy = np.where(free, col(rm.VY) + delta * ay, col(rm.VY))
            for k, i in enumerate(base):
                particles[i + rm.VX] = float(vx[k])
                particles[i + rm.VY] = float(vy[k])
            self.force_acts[which] += acts
        return super()._pre_solve(particles, n_particles, damping, delta, should_update_mass, min_mass, max_mass, *rest)
