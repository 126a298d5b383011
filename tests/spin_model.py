"""CPU model of the relaxed pass with collider spin (egg_set_collider_spin; DESIGN.md section 2.7, "Collider spin").  Test
helper, not collected.

SpinModel is tests/motion_model.py's MotionModel (so one model covers cohesion, colliders, forces, viscosity, surfaces,
walls and motion off and on) whose colliders may each carry a spin (px, py, omega): a rigid angular velocity omega in rad/s,
counter-clockwise positive in the project's x/y, about the pivot (px, py), in px at the start of the step.  Default zero.  A
collider whose omega is zero takes MotionModel's expressions exactly as they stand (motion_model.project on a list of
one).  For a collider whose omega is not zero, with h the sub-step, S the sub-step count, sub the 0-based sub-step and
(vx, vy) its motion:

  t  = float(sub + 1) * h;  ox = t vx, oy = t vy                     as MotionModel
  Px = px + ox, Py = py + oy                                          the pivot rides on the collider's motion
  c  = math.cos(t omega), s = math.sin(t omega)                       libm's, as the library's host computes them
  a point (qx, qy) of the stored geometry:  rx = qx - px, ry = qy - py,  qx' = Px + (c rx - s ry), qy' = Py + (s rx + c ry)
  disc, container: the centre is such a point, R unchanged;  segment, wall: both end points
  half_plane (nx, ny, off):  nx' = c nx - s ny, ny' = s nx + c ny,  off' = (nx' Px + ny' Py) + (off - (nx px + ny py))

and step 5b runs on the primed parameters.  A turning wall takes the side of the sub-step's start carried along with it
over ONE sub-step: ts = float(sub) * h, ch = math.cos(h omega), sh = math.sin(h omega),

  ux = prev.x - (px + ts vx), uy = prev.y - (py + ts vy);  pvx = Px + (ch ux - sh uy), pvy = Py + (sh ux + ch uy)

stand wherever the wall rule reads prev.  Step 5c takes the surface's velocity at the contact point, (x, y) being the
position the projection has just produced, and reads the true prev:

  wx = (sf.vx + vx) - omega (y - Py),  wy = (sf.vy + vy) + omega (x - Px)

When a step has run, the stored geometry and the stored pivot become the primed values with t = float(S) * h.

`labels[type]` is MotionModel's, with `turning` besides for every particle a collider with omega != 0 has looked at.
numpy float64 element-wise in exactly the order written, math.cos / math.sin for the angles; every comparison is false for
a NaN.  Written from the definition, not from the kernel.

`wrong` names one deliberately wrong rule (tests/test_spin_model.py shows that each changes a case's final state):
  pivot_unmoved            Px = px, Py = py
  angle_start              the angle is that of the sub-step's start, ts omega
  sweep_unrotated          the wall sweeps from prev + h v: MotionModel's carry only
  sweep_full_angle         the carry uses c, s of t
  friction_ignores_spin    wx = sf.vx + vx, wy = sf.vy + vy
  friction_lever_prev      the lever arm is taken from prev: (prev.y - Py), (prev.x - Px)
  half_plane_normal_fixed  nx' = nx, ny' = ny
  commit_short             the commit uses t = float(S - 1) * h
  clockwise                c, s, ch, sh are those of the negated angles"""
import math

import numpy as np

import motion_model as mm
import surface_model as sm
import wall_model as wm
from cohesion_model import CohesiveModel
from motion_model import MotionModel
from relaxed_model import rm
from wall_model import WallModel

WRONG = ("pivot_unmoved", "angle_start", "sweep_unrotated", "sweep_full_angle", "friction_ignores_spin", "friction_lever_prev",
         "half_plane_normal_fixed", "commit_short", "clockwise")
ZERO = (0.0, 0.0, 0.0)


def normalise(spins):
    """the records as the library stores them: (px, py, omega) per collider; None is a collider that does not turn"""
    out = []
    for s in spins:
        px, py, omega = (float(v) for v in (ZERO if s is None else s))
        assert math.isfinite(px) and math.isfinite(py) and math.isfinite(omega)
        out.append((px + 0.0, py + 0.0, omega + 0.0))  # (-0.0 is stored as +0.0)
    return out


def angle(a, wrong=None):
    """(cos, sin) of the angle a, by libm"""
    if wrong == "clockwise":
        a = -a
    return math.cos(a), math.sin(a)


def pivot(motion, spin, t, wrong=None):
    """the pivot at time t after the start of the step"""
    vx, vy = motion
    px, py, _ = spin
    if wrong == "pivot_unmoved":
        return px, py
    ox = t * vx
    oy = t * vy
    return px + ox, py + oy


def primed(collider, motion, spin, t, cs, wrong=None):
    """the turning collider at time t after the start of the step, cs = (cos, sin)(t omega)"""
    kind, p0, p1, p2, p3, mask = collider
    px, py, _ = spin
    c, s = cs
    Px, Py = pivot(motion, spin, t, wrong)

    def point(qx, qy):
        rx = qx - px
        ry = qy - py
        return Px + (c * rx - s * ry), Py + (s * rx + c * ry)

    if kind == "half_plane":
        nx = c * p0 - s * p1
        ny = s * p0 + c * p1
        if wrong == "half_plane_normal_fixed":
            nx, ny = p0, p1
        return (kind, nx, ny, (nx * Px + ny * Py) + (p2 - (p0 * px + p1 * py)), p3, mask)
    if kind in ("segment", "wall"):
        return (kind,) + point(p0, p1) + point(p2, p3) + (mask,)
    return (kind,) + point(p0, p1) + (p2, p3, mask)


def one(kind, p, x, y, r, idx):
    """step 5b of one collider that is no wall, on its parameters p: (x, y, hit, nx, ny, pen) as tests/surface_model.py
    defines them for step 5c"""
    p0, p1, p2, p3 = p
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if kind == "half_plane":
            s = (p0 * x + p1 * y) - (p2 + r)
            hit = s < 0.0
            return np.where(hit, x - s * p0, x), np.where(hit, y - s * p1, y), hit, p0, p1, -s
        if kind == "disc":
            return sm._disc(x, y, p0, p1, p2 + r, idx)
        if kind == "container":
            m = p2 - r
            m = np.where(m < 0.0, 0.0, m)
            dx = x - p0
            dy = y - p1
            d2 = dx * dx + dy * dy
            hit = d2 > m * m
            d = np.sqrt(d2)
            nx, ny = dx / d, dy / d
            return np.where(hit, p0 + nx * m, x), np.where(hit, p1 + ny * m, y), hit, nx, ny, d - m
        assert kind == "segment"
        ex = p2 - p0
        ey = p3 - p1
        l2 = ex * ex + ey * ey
        t = np.zeros_like(x) if l2 == 0.0 else ((x - p0) * ex + (y - p1) * ey) / l2
        t = np.where(t < 0.0, 0.0, t)
        t = np.where(t > 1.0, 1.0, t)
        return sm._disc(x, y, p0 + t * ex, p1 + t * ey, 0.0 + r, idx)


def project(x, y, r, px, py, h, t, ts, colliders, surfaces, motions, spins, type_bit, idx=None, wrong=None):
    """steps 5b and 5c over one particle type in a pass of the sub-step that starts at ts and ends at t, collider by
    collider: one that does not turn by motion_model.project() on a list of one, one that turns by the rule above.  Returns
    (x, y, hits, grips, sticks, catches, ever, labels) as motion_model.project() does."""
    x = np.array(x, dtype=np.float64)
    y = np.array(y, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    px = np.asarray(px, dtype=np.float64)
    py = np.asarray(py, dtype=np.float64)
    idx = np.arange(len(x)) if idx is None else np.asarray(idx, dtype=np.int64)
    surfaces = list(surfaces) if surfaces else [sm.DEFAULT] * len(colliders)
    motions = list(motions) if motions else [mm.ZERO] * len(colliders)
    spins = list(spins) if spins else [ZERO] * len(colliders)
    assert len(surfaces) == len(colliders) == len(motions) == len(spins)
    hits = grips = sticks = catches = 0
    ever = np.zeros(len(x), dtype=bool)
    labels = [set() for _ in range(len(x))]
    for collider, surface, motion, spin in zip(colliders, surfaces, motions, spins):
        if not collider[5] & type_bit:
            continue
        omega = spin[2]
        if omega == 0.0:  # MotionModel's expressions, exactly as they stand
            x, y, h1, g1, s1, c1, e1, l1 = mm.project(x, y, r, px, py, h, t, [collider], [surface], [motion], type_bit, idx)
            hits, grips, sticks, catches, ever = hits + h1, grips + g1, sticks + s1, catches + c1, ever | e1
            for k in range(len(x)):
                labels[k] |= l1[k]
            continue
        vx, vy = motion
        spx, spy, _ = spin
        mu, svx, svy = surface
        cs = angle((ts if wrong == "angle_start" else t) * omega, wrong)
        col = primed(collider, motion, spin, t, cs, wrong)
        kind = col[0]
        Px, Py = pivot(motion, spin, t, wrong)
        for k in range(len(x)):
            labels[k].add("turning")
        if kind != "wall":
            x, y, hit, nx, ny, pen = one(kind, col[1:5], x, y, r, idx)
            for k in range(len(x)):
                labels[k].add(kind + ("_hit" if hit[k] else "_miss"))
        else:
            if wrong == "sweep_unrotated":
                wx_, wy_ = px + h * vx, py + h * vy
            else:
                ch, sh = cs if wrong == "sweep_full_angle" else angle(h * omega, wrong)
                ux = px - (spx + ts * vx)
                uy = py - (spy + ts * vy)
                wx_ = Px + (ch * ux - sh * uy)
                wy_ = Py + (sh * ux + ch * uy)
            branch = mm.wall_branch(x, y, wx_, wy_, col[1:5])
            x, y, hit, nx, ny, pen, caught = wm.wall(x, y, r, wx_, wy_, col[1:5], idx)
            for k in range(len(x)):
                labels[k].add(branch[k])
                assert caught[k] == branch[k].startswith("catch")
                if not caught[k]:
                    labels[k].add("wall_hit" if hit[k] else "wall_miss")
            catches += int(np.count_nonzero(caught))
            ever |= caught
        hits += int(np.count_nonzero(hit))
        # step 5c: the surface's velocity at the contact point, the position the projection has just produced
        with np.errstate(invalid="ignore", over="ignore"):
            if wrong == "friction_ignores_spin":
                wvx, wvy = svx + vx, svy + vy
            elif wrong == "friction_lever_prev":
                wvx = (svx + vx) - omega * (py - Py)
                wvy = (svy + vy) + omega * (px - Px)
            else:
                wvx = (svx + vx) - omega * (y - Py)
                wvy = (svy + vy) + omega * (x - Px)
        x, y, on, stuck = sm.grip(x, y, px, py, h, (mu, wvx, wvy), nx, ny, pen, hit)
        grips += int(np.count_nonzero(on))
        sticks += int(np.count_nonzero(stuck))
        for k in np.flatnonzero(on):
            labels[k].add("stick" if stuck[k] else "slide")
    return x, y, hits, grips, sticks, catches, ever, labels


class SpinModel(MotionModel):
    """MotionModel whose colliders turn (set_collider_spin; set_colliders resets the spins, set_collider_motion and
    set_collider_surfaces do not)."""

    def __init__(self, white_config=None, yolk_config=None, relaxed=True, relaxation=None, cohesion=False, wrong=None):
        assert wrong is None or wrong in WRONG
        self.spins = []
        self.spin_wrong = wrong
        super().__init__(white_config, yolk_config, relaxed, relaxation=relaxation, cohesion=cohesion)

    def set_colliders(self, colliders):
        super().set_colliders(colliders)
        self.spins = []

    def set_collider_spin(self, spins):
        spins = normalise(spins)
        assert len(spins) in (0, len(self.colliders))
        self.spins = spins

    def get_collider_spin(self):
        return list(self.spins) if self.spins else [ZERO] * len(self.colliders)

    def turning(self):
        return any(s[2] != 0.0 for s in self.spins)

    def _step(self, delta, n_sub_steps, n_collision_steps, visit_logs=None):
        if not self.turning():  # a list that does not turn is the list without spin
            return super()._step(delta, n_sub_steps, n_collision_steps, visit_logs)
        self._n_sub, self._n_col = n_sub_steps, n_collision_steps
        out = WallModel._step(self, delta, n_sub_steps, n_collision_steps, visit_logs)
        # the commit: the geometry and the pivots of the step's end, the last sub-step's expressions
        t = float(n_sub_steps - 1 if self.spin_wrong == "commit_short" else n_sub_steps) * self._sub_delta
        motions = self.motions if self.motions else [mm.ZERO] * len(self.colliders)
        colliders, spins = [], []
        for c, m, s in zip(self.colliders, motions, self.spins):
            if s[2] == 0.0:
                colliders.append(mm.primed(c, m, t))
                spins.append(s)
            else:
                colliders.append(primed(c, m, s, t, angle(t * s[2], self.spin_wrong), self.spin_wrong))
                spins.append(pivot(m, s, t, self.spin_wrong) + (s[2],))
        self.colliders, self.spins = colliders, spins
        return out

    def _solve_collision(self, particles, n_particles, *args, **kwargs):
        if not self.turning():
            return super()._solve_collision(particles, n_particles, *args, **kwargs)
        # the reference's _step appends one entry to pass_log per type and pass, after the pass: the sub-step of this one
        sub = len(self.pass_log) // (2 * self._n_col)
        assert 0 <= sub < self._n_sub
        t = float(sub + 1) * self._sub_delta
        ts = float(sub) * self._sub_delta
        out = CohesiveModel._solve_collision(self, particles, n_particles, *args, **kwargs)
        if self.relaxed and self.colliders and n_particles:
            which = 0 if particles is self._white_data else 1
            base = [rm.offset(p) for p in range(1, n_particles + 1)]

            def col(off):
                return [particles[i + off] for i in base]

            x, y, hits, grips, sticks, catches, ever, labels = project(
                col(rm.X), col(rm.Y), col(rm.RADIUS), col(rm.PX), col(rm.PY), self._sub_delta, t, ts, self.colliders, self.surfaces,
                self.motions, self.spins, 1 << which, wrong=self.spin_wrong)
            for k, i in enumerate(base):
                particles[i + rm.X] = float(x[k])
                particles[i + rm.Y] = float(y[k])
                if labels[k]:
                    self.labels[which].setdefault(k, set()).update(labels[k])
            self.collider_hits[which] += hits
            self.collider_grips[which] += grips
            self.grip_sticks[which] += sticks
            self.wall_catches[which] += catches
            self.caught_ever[which].update(int(k) for k in np.flatnonzero(ever))
        return out
