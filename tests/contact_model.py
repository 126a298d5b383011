"""CPU model of the relaxed step with collider contacts (egg_set_collider_contacts; DESIGN.md section 2.7, "Collider
contacts").  Test helper, not collected.

ContactModel is tests/body_model.py's BodyModel whose colliders may each carry a contact record (restitution, on):
restitution in [0, 1], on 0 or 1.  Contacts ACT in a step exactly when bodies act and some record is on.  While they act,
every sub-step ends, behind step 4 of "Collider bodies" and on what that step has just written -- the stored geometry and
pivots of the sub-step's end, the new velocities and spins --, with `iterations` rounds of the rule below, h the sub-step.
All of it is float64 in exactly the order written, no contraction, + - * / sqrt only; every comparison is false for a NaN.

1. The generalised body.  Collider k has the weights mk = inv_mass and ik = inv_inertia (both 0 when it is no body), the
   velocity (vx, vy), the spin omega about its stored pivot (Px, Py), and at a point (px, py) the velocity
       ux = vx - omega * (py - Py),   uy = vy + omega * (px - Px)

2. The pairs.  (a, b), a < b, is a pair when both are on, one of them is a disc, the other a half_plane, disc, container,
   segment or wall, and ((ma + ia) + mb) + ib > 0.  With (cx, cy, R) the disc, `push` the unit vector along which the other
   collider pushes the disc away, g the gap (negative: overlap) and (px, py) the contact point:
     disc a, disc b    dx = bx - ax, dy = by - ay, d2 = dx dx + dy dy, d = sqrt(d2); n = (dx / d, dy / d), DIRS[(b - a) & 7]
                       when d2 == 0; g = d - (Ra + Rb); p = (ax + nx Ra, ay + ny Ra).  n is this, a to b.
     half_plane        (nx, ny, off): g = (nx cx + ny cy) - (off + R); push = (nx, ny); p = (cx - nx R, cy - ny R)
     container         (qx, qy, Rc): dx = cx - qx, dy = cy - qy, d2, d as above; o = (dx / d, dy / d), DIRS[(b - a) & 7] when
                       d2 == 0; g = (Rc - R) - d; push = (-ox, -oy); p = (cx + ox R, cy + oy R).  A curved wall: rule 3
                       replaces g by the gap the tangential travel of the sub-step leaves, see there
     segment, wall     (x0, y0, x1, y1): ex = x1 - x0, ey = y1 - y0, l2 = ex ex + ey ey,
                       t = l2 == 0 ? 0 : ((cx - x0) ex + (cy - y0) ey) / l2 clamped to [0, 1], q = (x0 + t ex, y0 + t ey),
                       dx = cx - qx, dy = cy - qy, d2, d as above; push = (dx / d, dy / d); when d2 == 0 the left normal
                       ((-ey) / l, ex / l), l = sqrt(l2), and DIRS[(b - a) & 7] when l2 == 0 too; g = d - R; p = q
   For a pair with one disc, n = push when the disc is b and n = (-pushx, -pushy) when it is a: n points from a to b.
   Every other combination (two half-planes, a wall against a container, ...) is not a pair.

3. One iteration, for every pair from the velocities and spins of the iteration's start:
       vn = nx * (ubx - uax) + ny * (uby - uay)                 (the velocities of b and a at p)
       ca = (px - Pax) * ny - (py - Pay) * nx,  wa = ma + ia * (ca * ca);  cb, wb likewise;  w = wa + wb
   For a container with m = Rc - R > 0 the gap is first bent to the wall: a centre that travels h vt along the tangent of a
   circle of radius m leaves it by sqrt(d^2 + (h vt)^2) - d although g + h vn says it stays, so with the velocities of the
   disc at its centre c and of the container at its centre q (as in rule 1), both of the iteration's start,
       vt = ox * (udy - ucy) - oy * (udx - ucx);  s = h * vt;  q2 = m * m - s * s;  q2 < 0: q2 = 0;  g = sqrt(q2) - d
   which is (Rc - R) - d when nothing slides.  With this g the linear test below is exact for the circle: the next pose's
   centre is at most m from q.
   The pair FIRES when w > 0 and g + h * vn < 0, and then
       e = max(ea, eb);  t1 = (-g) / h;  t2 = -(e * vn);  target = t1 > t2 ? t1 : t2;  lam = (target - vn) / w
   b takes the impulse (lam nx, lam ny) at p and a takes (-(lam nx), -(lam ny)).  Collider k walks its partners j in ascending
   order, from sx = sy = sz = 0.0 and count = 0:  sx = sx + Jx, sy = sy + Jy, sz = sz + ((px - Pkx) * Jy - (py - Pky) * Jx),
   count += 1.  Then, when count > 0:
       mk > 0:  vx = vx + (sx * mk) / count,  vy = vy + (sy * mk) / count
       ik > 0:  omega = omega + (sz * ik) / count
   (constraint averaging: a collider in two contacts takes the mean of what each alone asks for).  A collider with both
   weights 0 is never changed.

4. `iterations` of these, each from the one before.  After the last one a collider with ik > 0 recomputes its turn with the
   integrator's four lines (body_model.cayley).

5. `contact_solves` counts the fires: one per (pair, sub-step, iteration), over committed steps.

Contacts change velocities, spins and turns only.  While contacts do not act a step is BodyModel's.  set_colliders resets
the records.  Written from the definition, not from the kernel.

`wrong` names one deliberately wrong rule (tests/test_contact_model.py shows that each changes a case):
  not_speculative       the pair fires when g < 0, without h * vn
  target_without_max    target = t1, whatever t2
  e_product             e = ea * eb
  not_averaged          no division by count
  weight_no_rotation    w = ma + mb
  descending            the partners are walked in descending order
  turn_stale            the turn is not recomputed after the last iteration
  wall_not_bent         a container's gap stays (Rc - R) - d"""
import math

from body_model import BodyModel, cayley
from relaxed_model import DIRS

WRONG = ("not_speculative", "target_without_max", "e_product", "not_averaged", "weight_no_rotation", "descending", "turn_stale", "wall_not_bent")
OFF = (0.0, 0)
DEFAULT_ITERATIONS = 4
OTHERS = ("half_plane", "disc", "container", "segment", "wall")


def normalise(contacts):
    """the records as the library stores them: (restitution, on) per collider; None is off, True is (0.0, 1), a number a
    restitution"""
    out = []
    for c in contacts:
        if c is None or c is False:
            out.append(OFF)
            continue
        e = 0.0 if c is True else float(c)
        assert math.isfinite(e) and 0.0 <= e <= 1.0
        out.append((e + 0.0, 1))
    return out


def _unit(dx, dy, d2, d, k8):
    if d2 == 0.0:
        return float(DIRS[k8, 0]), float(DIRS[k8, 1])
    return dx / d, dy / d


def geometry(a, b, ca, cb):
    """rule 2 for the colliders ca, cb = (kind, p0, p1, p2, p3, mask) at the indices a < b: (nx, ny, g, px, py, curve), or None
    where the shapes make no pair; curve is None, or (ox, oy, m, d, disc_is_b) of a container that rule 3 bends the gap to"""
    k8 = (b - a) & 7
    if ca[0] == "disc" and cb[0] == "disc":
        dx = cb[1] - ca[1]
        dy = cb[2] - ca[2]
        d2 = dx * dx + dy * dy
        d = math.sqrt(d2)
        nx, ny = _unit(dx, dy, d2, d, k8)
        return nx, ny, d - (ca[3] + cb[3]), ca[1] + nx * ca[3], ca[2] + ny * ca[3], None
    if ca[0] == "disc":
        disc, other, disc_is_b = ca, cb, False
    elif cb[0] == "disc":
        disc, other, disc_is_b = cb, ca, True
    else:
        return None
    cx, cy, R = disc[1:4]
    kind = other[0]
    curve = None
    if kind == "half_plane":
        ux, uy = other[1], other[2]
        g = (ux * cx + uy * cy) - (other[3] + R)
        px = cx - ux * R
        py = cy - uy * R
    elif kind == "container":
        dx = cx - other[1]
        dy = cy - other[2]
        d2 = dx * dx + dy * dy
        d = math.sqrt(d2)
        ox, oy = _unit(dx, dy, d2, d, k8)
        g = (other[3] - R) - d
        if other[3] - R > 0.0:
            curve = (ox, oy, other[3] - R, d, disc_is_b)
        ux, uy = -ox, -oy
        px = cx + ox * R
        py = cy + oy * R
    elif kind in ("segment", "wall"):
        x0, y0, x1, y1 = other[1:5]
        ex = x1 - x0
        ey = y1 - y0
        l2 = ex * ex + ey * ey
        t = 0.0 if l2 == 0.0 else ((cx - x0) * ex + (cy - y0) * ey) / l2
        if t < 0.0:
            t = 0.0
        if t > 1.0:
            t = 1.0
        px = x0 + t * ex
        py = y0 + t * ey
        dx = cx - px
        dy = cy - py
        d2 = dx * dx + dy * dy
        d = math.sqrt(d2)
        if d2 == 0.0 and l2 != 0.0:
            ln = math.sqrt(l2)
            ux, uy = (-ey) / ln, ex / ln
        else:
            ux, uy = _unit(dx, dy, d2, d, k8)
        g = d - R
    else:
        return None
    if disc_is_b:
        return ux, uy, g, px, py, curve
    return -ux, -uy, g, px, py, curve


def point_velocity(motion, spin, px, py):
    return motion[0] - spin[2] * (py - spin[1]), motion[1] + spin[2] * (px - spin[0])


class ContactModel(BodyModel):
    """BodyModel whose bodies also meet the other colliders (set_collider_contacts)."""

    def __init__(self, white_config=None, yolk_config=None, relaxed=True, relaxation=None, cohesion=False, wrong=None,
                 contact_wrong=None):
        assert contact_wrong is None or contact_wrong in WRONG
        self.contact_wrong = contact_wrong
        self.contacts = []
        self.contact_iterations = DEFAULT_ITERATIONS
        self.contact_solves = 0
        self._step_solves = 0
        super().__init__(white_config, yolk_config, relaxed, relaxation=relaxation, cohesion=cohesion, wrong=wrong)

    def set_colliders(self, colliders):
        super().set_colliders(colliders)
        self.contacts = []

    def set_collider_contacts(self, contacts, iterations=DEFAULT_ITERATIONS):
        contacts = normalise(contacts)
        assert len(contacts) in (0, len(self.colliders))
        assert 0 <= iterations <= 16
        self.contacts = contacts
        self.contact_iterations = iterations or DEFAULT_ITERATIONS

    def get_collider_contacts(self):
        return (list(self.contacts) if self.contacts else [OFF] * len(self.colliders)), self.contact_iterations

    def collider_contact_solves(self):
        return self.contact_solves

    def contacts_act(self):
        return self.bodies_act() and any(on for _, on in self.contacts)

    def _step(self, delta, n_sub_steps, n_collision_steps, visit_logs=None):
        self._step_solves = 0
        out = super()._step(delta, n_sub_steps, n_collision_steps, visit_logs)
        self.contact_solves += self._step_solves  # (a step that raises adds nothing)
        return out

    def _integrate(self, h):
        super()._integrate(h)
        if self.contacts_act():
            self._contacts(h)

    def _pairs(self):
        """rule 2: {(a, b): (nx, ny, g, px, py)} from the stored poses"""
        n = len(self.colliders)
        pairs = {}
        for a in range(n):
            for b in range(a + 1, n):
                if not (self.contacts[a][1] and self.contacts[b][1]):
                    continue
                ba, bb = self.bodies[a], self.bodies[b]
                if not ((ba[0] + ba[1]) + bb[0]) + bb[1] > 0.0:
                    continue
                geo = geometry(a, b, self.colliders[a], self.colliders[b])
                if geo is not None:
                    pairs[(a, b)] = geo
        return pairs

    def _contacts(self, h):
        wrong = self.contact_wrong
        n = len(self.colliders)
        pairs = self._pairs()
        motions, spins = list(self.motions), list(self.spins)
        for _ in range(self.contact_iterations):
            lams = {}
            for (a, b), (nx, ny, g, px, py, curve) in pairs.items():
                uax, uay = point_velocity(motions[a], spins[a], px, py)
                ubx, uby = point_velocity(motions[b], spins[b], px, py)
                if curve is not None and wrong != "wall_not_bent":
                    ox, oy, m, d, disc_is_b = curve
                    disc, cont = (b, a) if disc_is_b else (a, b)
                    udx, udy = point_velocity(motions[disc], spins[disc], self.colliders[disc][1], self.colliders[disc][2])
                    ucx, ucy = point_velocity(motions[cont], spins[cont], self.colliders[cont][1], self.colliders[cont][2])
                    vt = ox * (udy - ucy) - oy * (udx - ucx)
                    s = h * vt
                    q2 = m * m - s * s
                    if q2 < 0.0:
                        q2 = 0.0
                    g = math.sqrt(q2) - d
                vn = nx * (ubx - uax) + ny * (uby - uay)
                ca = (px - spins[a][0]) * ny - (py - spins[a][1]) * nx
                cb = (px - spins[b][0]) * ny - (py - spins[b][1]) * nx
                wa = self.bodies[a][0] + self.bodies[a][1] * (ca * ca)
                wb = self.bodies[b][0] + self.bodies[b][1] * (cb * cb)
                if wrong == "weight_no_rotation":
                    wa, wb = self.bodies[a][0], self.bodies[b][0]
                w = wa + wb
                fires = w > 0.0 and (g < 0.0 if wrong == "not_speculative" else g + h * vn < 0.0)
                if not fires:
                    continue
                ea, eb = self.contacts[a][0], self.contacts[b][0]
                e = ea * eb if wrong == "e_product" else (ea if ea > eb else eb)
                t1 = (-g) / h
                t2 = -(e * vn)
                target = t1 if t1 > t2 or wrong == "target_without_max" else t2
                lams[(a, b)] = (target - vn) / w
                self._step_solves += 1
            new_motions, new_spins = list(motions), list(spins)
            for k in range(n):
                sx = sy = sz = 0.0
                count = 0
                order = range(n - 1, -1, -1) if wrong == "descending" else range(n)
                for j in order:
                    key = (min(k, j), max(k, j))
                    if j == k or key not in lams:
                        continue
                    nx, ny, g, px, py, _ = pairs[key]
                    lam = lams[key]
                    Jx, Jy = lam * nx, lam * ny
                    if k == key[0]:
                        Jx, Jy = -Jx, -Jy
                    sx = sx + Jx
                    sy = sy + Jy
                    sz = sz + ((px - spins[k][0]) * Jy - (py - spins[k][1]) * Jx)
                    count += 1
                if count == 0:
                    continue
                cnt = 1.0 if wrong == "not_averaged" else float(count)
                mk, ik = self.bodies[k][0], self.bodies[k][1]
                if mk > 0.0:
                    new_motions[k] = (motions[k][0] + (sx * mk) / cnt, motions[k][1] + (sy * mk) / cnt)
                if ik > 0.0:
                    new_spins[k] = (spins[k][0], spins[k][1], spins[k][2] + (sz * ik) / cnt)
            motions, spins = new_motions, new_spins
        turns = list(self._turns)
        if wrong != "turn_stale":
            for k in range(n):
                if self.bodies[k][1] > 0.0:
                    turns[k] = cayley(h, spins[k][2])
        self.motions, self.spins, self._turns = motions, spins, turns
        self._ended = (self.colliders, motions, spins)

    def gaps(self):
        """{(a, b): g} of the stored poses, for the tests' properties"""
        return {key: geo[2] for key, geo in self._pairs().items()}
