"""CPU model of the relaxed step with collider bodies (egg_set_collider_bodies; DESIGN.md section 2.7, "Collider bodies").  Test
helper, not collected.

BodyModel is tests/load_model.py's LoadModel (so one model covers cohesion, colliders, forces, viscosity, surfaces, walls,
motion, spin and loads off and on) whose colliders may each carry a body

  (inv_mass, inv_inertia, ax, ay, drag, spin_drag)     all finite, all >= 0 except ax, ay; default all zero

inv_mass > 0 frees the translation, inv_inertia > 0 the rotation about the collider's spin pivot; a collider with both zero
is no body and stays kinematic.  ax, ay (px/s^2) act only when inv_mass > 0; drag and spin_drag are in 1/s.

Bodies ACT in a step when the order is relaxed, the list is not empty, some collider is a body, and collider loads are on.
A step with a body, relaxed order, a list and loads off raises before anything happens.  While bodies act:

  * every collider has a motion record (vx, vy), a spin record (px, py, omega) and a turn (c, s), zeros included.  The turn
    of a collider with inv_inertia > 0 is cayley(h, omega) below; any other keeps libm's (cos, sin)(h omega), h the sub-step.
  * every sub-step is posed to LoadModel's rules as the FIRST sub-step of a step over the current records: the geometry at
    t = h, the sub-step's start at ts = 0, the table's row of the sub-step and the row of one sub-step both the current
    turns, every rule of the most general flavour (SpinModel's project(); a collider whose omega is zero takes MotionModel's
    expressions, as there).  The torque of a contribution is about the current pivot riding on the current motion at t = h.
  * after the last collision pass of the sub-step of both types (and after viscosity), for every collider k, float64 in
    exactly this order:

    1. d = sums[k] - seen[k] (three int64, wrapping); seen[k] = sums[k]
       Jx = (float(dx) / 2**20) / h,  Jy = (float(dy) / 2**20) / h,  Jz = (float(dz) / 2**10) / h
    2. the stored geometry and the stored pivot become what the sub-step used: with (vx, vy), omega and (c, s) of the
       sub-step, omega != 0: spin_model.primed() and spin_model.pivot() at t = h with (c, s); otherwise motion_model.primed()
       at t = h, and the pivot stays (as a committed step of SpinModel leaves it).  Kinematic colliders advance too.
    3. if inv_mass > 0:    vx = vx + Jx * inv_mass;  vx = vx + h * ax;  (y likewise)
                           f = 1.0 - h * drag;  if not f > 0: f = 0.0;  vx = vx * f;  vy = vy * f
    4. if inv_inertia > 0: omega = omega + Jz * inv_inertia;  f = 1.0 - h * spin_drag;  if not f > 0: f = 0.0;  omega = omega * f
                           (c, s) = cayley(h, omega):  u = 0.5 * (h * omega);  den = 1.0 + u * u;  c = (1.0 - u * u) / den;
                                                       s = (u + u) / den

    cayley() turns by 2 atan(h omega / 2), not h omega: only + - * / occur, so host, device and numpy agree to the bit.
  * when the step has run, the stored list, motions and spins are those of the last sub-step's end.  The load sums still
    cover the whole step.  A step that raises leaves everything as it was.

A list with bodies therefore advances sub-step by sub-step, not by float(sub + 1) * h * v from the step's start: equal to
LoadModel's step by roundings only, and bit for bit at S = 1.  While bodies do not act -- none set, loads off in exact
order, an empty list -- a step is LoadModel's.  set_colliders resets the bodies; set_collider_motion, set_collider_spin and
set_collider_surfaces leave them.  Written from the definition, not from the kernel.

`wrong` names one deliberately wrong rule (tests/test_body_model.py shows that each changes a case):
  impulse_not_per_h     J = float(d) / scale, not divided by h
  stale_pivot           the torque of a contribution is taken about the pivot of the step's start
  accel_first           vx = vx + h * ax before vx = vx + Jx * inv_mass
  seen_kept             seen[k] is not updated: every sub-step takes the step's sums so far
  libm_turn             the turn of a free body is libm's (cos, sin)(h omega)
  neighbours_stay       step 2 skips the colliders that are no body
  drag_first            the damping is applied before the impulse (and before the acceleration)"""
import math

import motion_model as mm
import spin_model as sp
import surface_model as sm
from load_model import IMPULSE_SCALE, TORQUE_SCALE, LoadModel, wrap64
from relaxed_model import rm

WRONG = ("impulse_not_per_h", "stale_pivot", "accel_first", "seen_kept", "libm_turn", "neighbours_stay", "drag_first")
ZERO = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def normalise(bodies):
    """the records as the library stores them: six doubles per collider; None is a collider that is no body, short tuples
    are (inv_mass, inv_inertia) and (inv_mass, inv_inertia, ax, ay)"""
    out = []
    for b in bodies:
        b = ZERO if b is None else tuple(float(v) for v in b)
        assert len(b) in (2, 4, 6)
        b = b + ZERO[len(b):]
        assert all(math.isfinite(v) for v in b)
        assert b[0] >= 0.0 and b[1] >= 0.0 and b[4] >= 0.0 and b[5] >= 0.0
        out.append(tuple(v + 0.0 for v in b))  # (-0.0 is stored as +0.0)
    return out


def cayley(h, omega):
    """the turn (c, s) of one sub-step of a free body"""
    u = 0.5 * (h * omega)
    den = 1.0 + u * u
    return (1.0 - u * u) / den, (u + u) / den


def damped(v, h, drag):
    f = 1.0 - h * drag
    if not f > 0.0:
        f = 0.0
    return tuple(c * f for c in v)


class BodyModel(LoadModel):
    """LoadModel whose colliders may be bodies the step integrates from their own loads (set_collider_bodies)."""

    def __init__(self, white_config=None, yolk_config=None, relaxed=True, relaxation=None, cohesion=False, wrong=None):
        assert wrong is None or wrong in WRONG
        self.body_wrong = wrong
        self.bodies = []
        self._turns = None  # while bodies act: the turn (c, s) of every collider for the sub-step that runs
        self._start_spins = self._live_spins = None
        super().__init__(white_config, yolk_config, relaxed, relaxation=relaxation, cohesion=cohesion)

    def set_colliders(self, colliders):
        super().set_colliders(colliders)
        self.bodies = []

    def set_collider_bodies(self, bodies):
        bodies = normalise(bodies)
        assert len(bodies) in (0, len(self.colliders))
        self.bodies = bodies

    def get_collider_bodies(self):
        return list(self.bodies) if self.bodies else [ZERO] * len(self.colliders)

    def has_body(self):
        return any(b[0] > 0.0 or b[1] > 0.0 for b in self.bodies)

    def bodies_act(self):
        return self.relaxed and bool(self.colliders) and self.has_body() and self.loads_on

    # ---- the step
    def _step(self, delta, n_sub_steps, n_collision_steps, visit_logs=None):
        if self.relaxed and self.colliders and self.has_body() and not self.loads_on:
            raise RuntimeError("collider bodies need collider loads (set_collider_loads(True))")
        if not self.bodies_act():
            return super()._step(delta, n_sub_steps, n_collision_steps, visit_logs)
        n = len(self.colliders)
        h = max(delta / n_sub_steps, rm.EPS)
        held = (self.colliders, self.motions, self.spins)
        self.motions = list(self.motions) if self.motions else [mm.ZERO] * n
        self.spins = list(self.spins) if self.spins else [sp.ZERO] * n
        self._start_spins = list(self.spins)
        self._turns = [self._turn(k, h) if self.bodies[k][1] > 0.0 else (math.cos(h * self.spins[k][2]), math.sin(h * self.spins[k][2]))
                       for k in range(n)]
        self._seen = [(0, 0, 0)] * n
        self._ended = None
        try:
            out = super()._step(delta, n_sub_steps, n_collision_steps, visit_logs)
            self.colliders, self.motions, self.spins = self._ended  # (not the parents' commit from the step's start)
        except Exception:
            self.colliders, self.motions, self.spins = held
            raise
        finally:
            self._turns = self._start_spins = None
        return out

    def _turn(self, k, h):
        omega = self.spins[k][2]
        return (math.cos(h * omega), math.sin(h * omega)) if self.body_wrong == "libm_turn" else cayley(h, omega)

    def _solve_collision(self, particles, n_particles, *args, **kwargs):
        if self._turns is None:
            return super()._solve_collision(particles, n_particles, *args, **kwargs)
        # posed as the first sub-step: LoadModel takes the sub-step, and from it t and ts, from the length of the step's log
        held, self.pass_log = self.pass_log, []
        self._live_spins = self.spins  # (what the rules run on; LoadModel reads self.spins for the torque's pivot)
        if self.body_wrong == "stale_pivot":
            self.spins = [(s0[0], s0[1], s[2]) for s0, s in zip(self._start_spins, self.spins)]
        try:
            return super()._solve_collision(particles, n_particles, *args, **kwargs)
        finally:
            self.pass_log, self.spins = held, self._live_spins

    def _one(self, k, x, y, r, px, py, t, ts, type_bit, idx, smooth=False):
        if self._turns is None:
            return super()._one(k, x, y, r, px, py, t, ts, type_bit, idx, smooth)
        h = self._sub_delta
        assert t == h and ts == 0.0
        sf = [sm.DEFAULT if smooth or not self.surfaces else self.surfaces[k]]
        spins = [self._live_spins[k]]
        # the sub-step's turn stands for both rows of the table: spin_model.project() asks angle() for (c, s)(t omega) and
        # for (c, s)(h omega), and t = h
        held, turn = sp.angle, self._turns[k]
        sp.angle = lambda a, wrong=None: turn
        try:
            out = sp.project(x, y, r, px, py, h, t, ts, [self.colliders[k]], sf, [self.motions[k]], spins, type_bit, idx)
        finally:
            sp.angle = held
        return out

    def _post_solve(self, particles, n_particles, delta):
        if self._turns is not None and particles is self._white_data:  # once per sub-step, after both types' last pass
            self._integrate(self._sub_delta)
        return super()._post_solve(particles, n_particles, delta)

    def _integrate(self, h):
        wrong = self.body_wrong
        colliders, motions, spins, turns = [], [], [], []
        for k, (c, m, s, b) in enumerate(zip(self.colliders, self.motions, self.spins, self.bodies)):
            inv_mass, inv_inertia, ax, ay, drag, spin_drag = b
            # 1. the impulse of the sub-step
            sums = tuple(wrap64(v) for v in self._acc["q"][k])
            d = tuple(wrap64(a - z) for a, z in zip(sums, self._seen[k]))
            if wrong != "seen_kept":
                self._seen[k] = sums
            Jx = float(d[0]) / IMPULSE_SCALE
            Jy = float(d[1]) / IMPULSE_SCALE
            Jz = float(d[2]) / TORQUE_SCALE
            if wrong != "impulse_not_per_h":
                Jx, Jy, Jz = Jx / h, Jy / h, Jz / h
            # 2. advance by what the sub-step used
            vx, vy = m
            px, py, omega = s
            if wrong == "neighbours_stay" and not (inv_mass > 0.0 or inv_inertia > 0.0):
                pass
            elif omega != 0.0:
                c = sp.primed(c, m, s, h, self._turns[k])
                px, py = sp.pivot(m, s, h)
            else:
                c = mm.primed(c, m, h)
            turn = self._turns[k]
            # 3. translation
            if inv_mass > 0.0:
                if wrong == "drag_first":
                    vx, vy = damped((vx, vy), h, drag)
                if wrong == "accel_first":
                    vx = vx + h * ax
                    vy = vy + h * ay
                    vx = vx + Jx * inv_mass
                    vy = vy + Jy * inv_mass
                else:
                    vx = vx + Jx * inv_mass
                    vy = vy + Jy * inv_mass
                    vx = vx + h * ax
                    vy = vy + h * ay
                if wrong != "drag_first":
                    vx, vy = damped((vx, vy), h, drag)
            # 4. rotation
            if inv_inertia > 0.0:
                if wrong == "drag_first":
                    omega, = damped((omega,), h, spin_drag)
                omega = omega + Jz * inv_inertia
                if wrong != "drag_first":
                    omega, = damped((omega,), h, spin_drag)
                turn = (math.cos(h * omega), math.sin(h * omega)) if wrong == "libm_turn" else cayley(h, omega)
            colliders.append(c)
            motions.append((vx, vy))
            spins.append((px, py, omega))
            turns.append(turn)
        self.colliders, self.motions, self.spins, self._turns = colliders, motions, spins, turns
        self._ended = (colliders, motions, spins)
