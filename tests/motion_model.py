"""CPU model of the relaxed pass with collider motion (egg_set_collider_motion; DESIGN.md section 2.7, "Collider motion").
Test helper, not collected.

MotionModel is tests/wall_model.py's WallModel (so one model covers cohesion, colliders, forces, viscosity, surfaces and
walls off and on) whose colliders may each carry a motion (vx, vy) in px/s, a rigid translation, default zero.  The stored
list is the geometry at the start of the step.  With h the sub-step, S the sub-step count, sub the 0-based sub-step:

  t  = float(sub + 1) * h;  ox = t vx, oy = t vy                       every pass of the sub-step: the geometry at its end
  half_plane (nx, ny, off):        off' = off + (nx ox + ny oy)
  disc, container (cx, cy, R):     cx' = cx + ox, cy' = cy + oy
  segment, wall (x0, y0, x1, y1):  x0' = x0 + ox, y0' = y0 + oy, x1' = x1 + ox, y1' = y1 + oy

and step 5b runs on the primed parameters.  A wall takes the side of the sub-step's start in its own frame:
pvx = prev.x + h vx, pvy = prev.y + h vy stand wherever the wall rule reads prev (a0, hx, hy).  Step 5c takes the
surface's velocity plus the motion's, wx = sf.vx + vx, wy = sf.vy + vy, and reads the true prev.  When a step has run, the
stored geometry becomes the primed geometry with t = float(S) * h.

`labels[type]` maps a 0-based particle index to the set of branches it has taken, over all steps:
  a wall:        catch_pos (a0 > 0), catch_neg (a0 < 0), round (the sides differ, the path passes beyond an end), same_side,
                 no_side (a0 == 0 or a NaN), and for what the segment's rule then did: wall_hit / wall_miss
  another kind:  <kind>_hit / <kind>_miss
  step 5c:       stick, slide (after a hit of a collider with mu > 0)
`wall_catches` and `caught_ever` are WallModel's.  numpy float64 element-wise in exactly the order written; every
comparison is false for a NaN.  Written from the definition, not from the kernel.

`wrong` names one deliberately wrong rule (tests/test_motion_model.py shows that each changes a scene's final state):
  sweep_uncarried         the wall sweeps from prev itself
  carry_t                 ... from prev + t v
  geometry_start          t = float(sub) * h
  friction_ignores_motion wx = sf.vx, wy = sf.vy
  half_plane_speed        off' = off + |v| t
  commit_short            the commit uses t = float(S - 1) * h
  friction_carried_prev   step 5c reads prev + h v"""
import math

import numpy as np

import surface_model as sm
import wall_model as wm
from cohesion_model import CohesiveModel
from relaxed_model import rm
from wall_model import WallModel

WRONG = ("sweep_uncarried", "carry_t", "geometry_start", "friction_ignores_motion", "half_plane_speed", "commit_short",
         "friction_carried_prev")
ZERO = (0.0, 0.0)


def normalise(motions):
    """the records as the library stores them: (vx, vy) per collider; None is a collider at rest"""
    out = []
    for m in motions:
        vx, vy = (float(v) for v in (ZERO if m is None else m))
        assert math.isfinite(vx) and math.isfinite(vy)
        out.append((vx + 0.0, vy + 0.0))  # (-0.0 is stored as +0.0)
    return out


def primed(collider, motion, t, wrong=None):
    """the collider at time t after the start of the step"""
    kind, p0, p1, p2, p3, mask = collider
    vx, vy = motion
    ox = t * vx
    oy = t * vy
    if kind == "half_plane":
        if wrong == "half_plane_speed":
            return (kind, p0, p1, p2 + math.sqrt(vx * vx + vy * vy) * t, p3, mask)
        return (kind, p0, p1, p2 + (p0 * ox + p1 * oy), p3, mask)
    if kind in ("segment", "wall"):
        return (kind, p0 + ox, p1 + oy, p2 + ox, p3 + oy, mask)
    return (kind, p0 + ox, p1 + oy, p2, p3, mask)


def wall_branch(x, y, pwx, pwy, p):
    """which way the wall's first question went for every lane: the definition's a0, a1, tc once more, for the label only"""
    x0, y0, x1, y1 = p
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ex = x1 - x0
        ey = y1 - y0
        l2 = np.float64(ex * ex + ey * ey)
        a0 = ex * (pwy - y0) - ey * (pwx - x0)
        a1 = ex * (y - y0) - ey * (x - x0)
        opp = ((a0 > 0.0) & (a1 <= 0.0)) | ((a0 < 0.0) & (a1 >= 0.0))
        u = a0 / (a0 - a1)
        hx = pwx + u * (x - pwx)
        hy = pwy + u * (y - pwy)
        tc = ((hx - x0) * ex + (hy - y0) * ey) / l2
        on = (tc >= 0.0) & (tc <= 1.0)
    out = []
    for k in range(len(x)):
        if opp[k]:
            out.append(("catch_pos" if a0[k] > 0.0 else "catch_neg") if on[k] else "round")
        else:
            out.append("same_side" if (a0[k] > 0.0 or a0[k] < 0.0) else "no_side")
    return out


def project(x, y, r, px, py, h, t, colliders, surfaces, motions, type_bit, idx=None, wrong=None):
    """steps 5b and 5c over one particle type in a pass of the sub-step that ends at t, collider by collider: each is primed,
    a wall by wall_model.wall() from the carried start, every other kind by surface_model.project() on a list of one, step 5c
    with the surface's velocity plus the motion's.  Returns (x, y, hits, grips, sticks, catches, ever, labels); labels is a
    list of sets, one per lane."""
    x = np.array(x, dtype=np.float64)
    y = np.array(y, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    px = np.asarray(px, dtype=np.float64)
    py = np.asarray(py, dtype=np.float64)
    idx = np.arange(len(x)) if idx is None else np.asarray(idx, dtype=np.int64)
    surfaces = list(surfaces) if surfaces else [sm.DEFAULT] * len(colliders)
    motions = list(motions) if motions else [ZERO] * len(colliders)
    assert len(surfaces) == len(colliders) == len(motions)
    hits = grips = sticks = catches = 0
    ever = np.zeros(len(x), dtype=bool)
    labels = [set() for _ in range(len(x))]
    for collider, surface, motion in zip(colliders, surfaces, motions):
        if not collider[5] & type_bit:
            continue
        vx, vy = motion
        col = primed(collider, motion, t, wrong)
        kind = col[0]
        mu, svx, svy = surface
        moving = (mu, svx, svy) if wrong == "friction_ignores_motion" else (mu, svx + vx, svy + vy)
        cvx = px + h * vx  # the start of the sub-step, carried along with the collider
        cvy = py + h * vy
        fx, fy = (cvx, cvy) if wrong == "friction_carried_prev" else (px, py)  # what step 5c reads: the true prev
        if kind != "wall":
            bx, by = x, y
            x, y, h1, g1, s1 = sm.project(x, y, r, fx, fy, h, [col], [moving], type_bit, idx)
            hits, grips, sticks = hits + h1, grips + g1, sticks + s1
            # (the labels: which lanes this collider moved, and how step 5c ended, by running it without friction too)
            nx_, ny_, _, _, _ = sm.project(bx, by, r, fx, fy, h, [col], [sm.DEFAULT], type_bit, idx)
            hit = ~((nx_ == bx) & (ny_ == by)) & ~(np.isnan(bx) | np.isnan(by))
            gripped = hit & ~((nx_ == x) & (ny_ == y))
            for k in range(len(x)):
                labels[k].add(kind + ("_hit" if hit[k] else "_miss"))
            if g1:  # one lane at a time: which of the gripped lanes stuck
                for k in np.flatnonzero(gripped):
                    one = sm.project(bx[k:k + 1], by[k:k + 1], r[k:k + 1], fx[k:k + 1], fy[k:k + 1], h, [col], [moving], type_bit,
                                     idx[k:k + 1])
                    labels[k].add("stick" if one[4] else "slide")
            continue
        if wrong == "sweep_uncarried":
            wx, wy = px, py
        elif wrong == "carry_t":
            wx, wy = px + t * vx, py + t * vy
        else:
            wx, wy = cvx, cvy
        branch = wall_branch(x, y, wx, wy, col[1:5])
        x, y, hit, nx, ny, pen, caught = wm.wall(x, y, r, wx, wy, col[1:5], idx)
        for k in range(len(x)):
            labels[k].add(branch[k])
            assert caught[k] == branch[k].startswith("catch")
            if not caught[k]:
                labels[k].add("wall_hit" if hit[k] else "wall_miss")
        hits += int(np.count_nonzero(hit))
        catches += int(np.count_nonzero(caught))
        ever |= caught
        x, y, on, stuck = sm.grip(x, y, fx, fy, h, moving, nx, ny, pen, hit)
        grips += int(np.count_nonzero(on))
        sticks += int(np.count_nonzero(stuck))
        for k in np.flatnonzero(on):
            labels[k].add("stick" if stuck[k] else "slide")
    return x, y, hits, grips, sticks, catches, ever, labels


class MotionModel(WallModel):
    """WallModel whose colliders move (set_collider_motion; set_colliders resets the motions, set_collider_surfaces does not)."""

    def __init__(self, white_config=None, yolk_config=None, relaxed=True, relaxation=None, cohesion=False, wrong=None):
        assert wrong is None or wrong in WRONG
        self.motions = []
        self.wrong = wrong
        self.labels = [{}, {}]
        self._n_sub = self._n_col = None
        super().__init__(white_config, yolk_config, relaxed, relaxation=relaxation, cohesion=cohesion)

    def set_colliders(self, colliders):
        super().set_colliders(colliders)
        self.motions = []

    def set_collider_motion(self, motions):
        motions = normalise(motions)
        assert len(motions) in (0, len(self.colliders))
        self.motions = motions

    def get_collider_motion(self):
        return list(self.motions) if self.motions else [ZERO] * len(self.colliders)

    def moving(self):
        return any(v != 0.0 for m in self.motions for v in m)

    def get_colliders(self):
        """the stored list as SimulationHandler.get_colliders returns it"""
        names = {1: "white", 2: "yolk", 3: "both"}
        return [(c[0],) + tuple(c[1:(5 if c[0] in ("segment", "wall") else 4)]) + (names[c[5]],) for c in self.colliders]

    def labels_of(self, which, particle):
        return self.labels[which].get(particle, set())

    def _step(self, delta, n_sub_steps, n_collision_steps, visit_logs=None):
        self._n_sub, self._n_col = n_sub_steps, n_collision_steps
        out = super()._step(delta, n_sub_steps, n_collision_steps, visit_logs)
        if self.moving():  # the commit: the geometry of the step's end, the last sub-step's expression
            t = float(n_sub_steps - 1 if self.wrong == "commit_short" else n_sub_steps) * self._sub_delta
            self.colliders = [primed(c, m, t, self.wrong) for c, m in zip(self.colliders, self.motions)]
        return out

    def _solve_collision(self, particles, n_particles, *args, **kwargs):
        if not self.moving():  # a list at rest is the list without motion
            return super()._solve_collision(particles, n_particles, *args, **kwargs)
        # the reference's _step appends one entry to pass_log per type and pass, after the pass: the sub-step of this one
        sub = len(self.pass_log) // (2 * self._n_col)
        assert 0 <= sub < self._n_sub
        t = float(sub if self.wrong == "geometry_start" else sub + 1) * self._sub_delta
        out = CohesiveModel._solve_collision(self, particles, n_particles, *args, **kwargs)
        if self.relaxed and self.colliders and n_particles:
            which = 0 if particles is self._white_data else 1
            base = [rm.offset(p) for p in range(1, n_particles + 1)]

            def col(off):
                return [particles[i + off] for i in base]

            x, y, hits, grips, sticks, catches, ever, labels = project(
                col(rm.X), col(rm.Y), col(rm.RADIUS), col(rm.PX), col(rm.PY), self._sub_delta, t, self.colliders, self.surfaces,
                self.motions, 1 << which, wrong=self.wrong)
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
