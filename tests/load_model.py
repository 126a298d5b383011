"""CPU model of the relaxed pass with collider loads (egg_set_collider_loads; DESIGN.md section 2.7, "Collider loads").  Test
helper, not collected.

LoadModel is tests/spin_model.py's SpinModel (so one model covers cohesion, colliders, forces, viscosity, surfaces, walls,
motion and spin off and on) that also records, per collider, what steps 5b and 5c did to the particles.  The projection
itself is the parents': the list is taken collider by collider through the parents' own project() on a list of one, which
is how they define it, so positions and every counter are SpinModel's bit for bit whether loads are on or off.

One CONTRIBUTION is counted for every (collider c, particle, pass) in which c moved the particle (a hit) and the particle's
inverse mass im satisfies im > eps:

  (bx, by)  the position that entered collider c's rule;  (ax, ay)  the position that left it, step 5c's grip included
  m  = 1.0 / im
  ux = m * (bx - ax),  uy = m * (by - ay)                    the reaction: what the collider feels
  (Px, Py)  spin_model.pivot(motion, spin, t): the spin record's (px, py) riding on the motion at the sub-step's end t, also
            when omega == 0; (0.0, 0.0) when the model holds no spin records
  uz = (ax - Px) * uy - (ay - Py) * ux
  qx = rint(ux * 2**20), qy = rint(uy * 2**20), qz = rint(uz * 2**10)        as int64

numpy float64 element-wise in exactly this order.  If one of the three scaled values is not finite or reaches 2**53 in
magnitude the contribution is dropped whole and counted in `dropped`; otherwise the three integers are added to collider
c's sums (Python integers, wrapped to int64 at the commit).  Both types add into the same sums.  The sums cover one step:
they start at zero when a step starts and replace the stored ones when it has run; a step that raises leaves the stored
ones.  set_colliders and set_collider_loads zero the stored ones.  Written from the definition, not from the kernel.

`wrong` names one deliberately wrong rule (tests/test_load_model.py shows that each changes a case's sums):
  sign                  ux = m * (ax - bx), uy = m * (ay - by)
  grip_left_out         (ax, ay) is the position after step 5b, without step 5c
  pivot_unmoved         (Px, Py) = the spin record's (px, py)
  immovable_counted     a particle with !(im > eps) contributes too
  scale_after_sum       ux, uy, uz are summed as float64 and the sums are scaled and rounded once, at the commit
  about_before          the moment is taken about the particle's position before the rule: (Px, Py) = (bx, by).  (The lever
                        itself may start at either end: (b - a) is parallel to the reaction, so (bx - Px) uy - (by - Py) ux is the
                        same moment up to rounding.)"""
import numpy as np

import motion_model as mm
import spin_model as sp
import surface_model as sm
import wall_model as wm
from relaxed_model import rm
from spin_model import SpinModel

WRONG = ("sign", "grip_left_out", "pivot_unmoved", "immovable_counted", "scale_after_sum", "about_before")
IMPULSE_SCALE = 2.0 ** 20  # EGG_COLLIDER_LOAD_IMPULSE_SCALE
TORQUE_SCALE = 2.0 ** 10   # EGG_COLLIDER_LOAD_TORQUE_SCALE
LIMIT = 2.0 ** 53


def wrap64(v):
    """the Python integer v as the int64 an unbounded two's-complement sum wraps to"""
    return (int(v) + 2 ** 63) % 2 ** 64 - 2 ** 63


def convert(sums, h):
    """(jx, jy, torque) per collider from the integer sums and the sub-step h, with the library's two divisions"""
    if not h > 0.0:
        return [(0.0, 0.0, 0.0)] * len(sums)
    return [((float(sx) / IMPULSE_SCALE) / h, (float(sy) / IMPULSE_SCALE) / h, (float(sz) / TORQUE_SCALE) / h) for sx, sy, sz in sums]


def contribution(bx, by, ax, ay, im, Px, Py, wrong=None):
    """the scaled values (fx, fy, fz) of the lanes' contributions and which of them are kept (`ok`); float64 arrays"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        m = 1.0 / im
        if wrong == "sign":
            ux = m * (ax - bx)
            uy = m * (ay - by)
        else:
            ux = m * (bx - ax)
            uy = m * (by - ay)
        if wrong == "about_before":
            Px, Py = bx, by
        uz = (ax - Px) * uy - (ay - Py) * ux
        fx = ux * IMPULSE_SCALE
        fy = uy * IMPULSE_SCALE
        fz = uz * TORQUE_SCALE
        ok = (np.abs(fx) < LIMIT) & (np.abs(fy) < LIMIT) & (np.abs(fz) < LIMIT)  # (false for a NaN)
    return fx, fy, fz, ok, (ux, uy, uz)


class LoadModel(SpinModel):
    """SpinModel that records collider loads while set_collider_loads(True)."""

    def __init__(self, white_config=None, yolk_config=None, relaxed=True, relaxation=None, cohesion=False, wrong=None):
        assert wrong is None or wrong in WRONG
        self.load_wrong = wrong
        self.loads_on = False
        self.load_sums = []       # [(sx, sy, sz)] per collider, int64 as Python integers
        self.load_dropped = 0
        self.load_sub_delta = 0.0
        self.load_contributions = 0  # (kept contributions over all steps: for the tests' own reach assertions)
        self._acc = None
        super().__init__(white_config, yolk_config, relaxed, relaxation=relaxation, cohesion=cohesion)

    # ---- the switch and the read-out
    def _zero_loads(self):
        self.load_sums = [(0, 0, 0)] * len(self.colliders)
        self.load_dropped = 0
        self.load_sub_delta = 0.0

    def set_colliders(self, colliders):
        super().set_colliders(colliders)
        self._zero_loads()  # (the switch stays)

    def set_collider_loads(self, on):
        self.loads_on = bool(on)
        self._zero_loads()

    def get_collider_loads_enabled(self):
        return self.loads_on

    def collider_load_sums(self):
        sums = list(self.load_sums) + [(0, 0, 0)] * (len(self.colliders) - len(self.load_sums))
        return sums, self.load_dropped, self.load_sub_delta

    def collider_loads(self):
        sums, _, h = self.collider_load_sums()
        return convert(sums, h)

    # ---- the step
    def _acts(self):
        return self.loads_on and self.relaxed and bool(self.colliders)

    def _step(self, delta, n_sub_steps, n_collision_steps, visit_logs=None):
        if not self._acts():
            return super()._step(delta, n_sub_steps, n_collision_steps, visit_logs)
        n = len(self.colliders)
        self._acc = dict(q=[[0, 0, 0] for _ in range(n)], f=[[0.0, 0.0, 0.0] for _ in range(n)], dropped=0, kept=0)
        try:
            out = super()._step(delta, n_sub_steps, n_collision_steps, visit_logs)
            acc = self._acc
        finally:
            self._acc = None  # (a step that raises commits nothing: the stored loads stay)
        if self.load_wrong == "scale_after_sum":
            scales = (IMPULSE_SCALE, IMPULSE_SCALE, TORQUE_SCALE)
            self.load_sums = [tuple(wrap64(int(np.rint(f[k] * scales[k]))) for k in range(3)) for f in acc["f"]]
        else:
            self.load_sums = [tuple(wrap64(v) for v in q) for q in acc["q"]]
        self.load_dropped = acc["dropped"]
        self.load_sub_delta = self._sub_delta
        self.load_contributions += acc["kept"]
        return out

    def _one(self, k, x, y, r, px, py, t, ts, type_bit, idx, smooth=False):
        """collider k alone on the lanes, by the rule of the model's flavour: (x, y, hits, grips, sticks, catches, ever, labels)"""
        col = [self.colliders[k]]
        sf = [sm.DEFAULT if smooth or not self.surfaces else self.surfaces[k]]
        mo = [self.motions[k] if self.motions else mm.ZERO]
        h = self._sub_delta
        if self.turning():
            return sp.project(x, y, r, px, py, h, t, ts, col, sf, mo, [self.spins[k]], type_bit, idx, wrong=self.spin_wrong)
        if self.moving():
            return mm.project(x, y, r, px, py, h, t, col, sf, mo, type_bit, idx, wrong=self.wrong)
        return wm.project(x, y, r, px, py, h, col, sf, type_bit, idx) + (None,)

    def _hit_mask(self, k, bx, by, ax, ay, hits, r, px, py, t, ts, type_bit, idx):
        """which lanes collider k has hit: the lanes it moved, and -- where the count says that a hit left a position as it
        was -- whatever the rule says for each of the others alone"""
        changed = ~((ax == bx) & (ay == by)) & ~(np.isnan(bx) | np.isnan(by))
        if int(np.count_nonzero(changed)) == hits:
            return changed
        mask = changed.copy()
        for j in np.flatnonzero(~changed & ~(np.isnan(bx) | np.isnan(by))):
            s = slice(j, j + 1)
            mask[j] = self._one(k, bx[s], by[s], r[s], px[s], py[s], t, ts, type_bit, idx[s])[2] == 1
        assert int(np.count_nonzero(mask)) == hits
        return mask

    def _solve_collision(self, particles, n_particles, *args, **kwargs):
        if self._acc is None or not n_particles:
            return super()._solve_collision(particles, n_particles, *args, **kwargs)
        sub = len(self.pass_log) // (2 * self._n_col)
        assert 0 <= sub < self._n_sub
        t = float(sub + 1) * self._sub_delta
        ts = float(sub) * self._sub_delta
        held = self.colliders
        self.colliders = []  # the pass of the classes below the colliders: the pairs alone
        try:
            out = super()._solve_collision(particles, n_particles, *args, **kwargs)
        finally:
            self.colliders = held
        which = 0 if particles is self._white_data else 1
        type_bit = 1 << which
        base = [rm.offset(p) for p in range(1, n_particles + 1)]

        def col(off):
            return np.array([particles[i + off] for i in base], dtype=np.float64)

        x, y, r, px, py, im = col(rm.X), col(rm.Y), col(rm.RADIUS), col(rm.PX), col(rm.PY), col(rm.INV_MASS)
        idx = np.arange(n_particles)
        free = np.ones(n_particles, dtype=bool) if self.load_wrong == "immovable_counted" else im > rm.EPS
        labelled = self.turning() or self.moving()
        for k, collider in enumerate(self.colliders):
            if not collider[5] & type_bit:
                continue
            bx, by = x, y
            x, y, hits, grips, sticks, catches, ever, labels = self._one(k, bx, by, r, px, py, t, ts, type_bit, idx)
            self.collider_hits[which] += hits
            self.collider_grips[which] += grips
            self.grip_sticks[which] += sticks
            self.wall_catches[which] += catches
            self.caught_ever[which].update(int(j) for j in np.flatnonzero(ever))
            if labelled:
                for j in range(n_particles):
                    if labels[j]:
                        self.labels[which].setdefault(j, set()).update(labels[j])
            if not hits:
                continue
            mask = self._hit_mask(k, bx, by, x, y, hits, r, px, py, t, ts, type_bit, idx) & free
            if not mask.any():
                continue
            ax, ay = x, y
            if self.load_wrong == "grip_left_out":
                ax, ay = self._one(k, bx, by, r, px, py, t, ts, type_bit, idx, smooth=True)[:2]
            if self.spins:
                motion = self.motions[k] if self.motions else mm.ZERO
                Px, Py = (self.spins[k][0], self.spins[k][1]) if self.load_wrong == "pivot_unmoved" else sp.pivot(motion, self.spins[k], t)
            else:
                Px, Py = 0.0, 0.0
            fx, fy, fz, ok, u = contribution(bx[mask], by[mask], ax[mask], ay[mask], im[mask], Px, Py, self.load_wrong)
            self._acc["dropped"] += int(np.count_nonzero(~ok))
            self._acc["kept"] += int(np.count_nonzero(ok))
            for c3, f in enumerate((fx, fy, fz)):
                self._acc["q"][k][c3] += sum(int(v) for v in np.rint(f[ok]).astype(np.int64))
                self._acc["f"][k][c3] += float(np.sum(u[c3][ok]))
        for j, i in enumerate(base):
            particles[i + rm.X] = float(x[j])
            particles[i + rm.Y] = float(y[j])
        return out
