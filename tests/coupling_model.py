"""CPU model of the relaxed step with white-yolk coupling (egg_set_coupling; DESIGN.md section 2.7, "Coupling").  Test
helper, not collected.

CouplingModel is tests/viscosity_model.py's ViscosityModel (so one model covers cohesion, colliders, forces and viscosity
off and on) with one cross-type pass per sub-step, after the follow of BOTH types and before the sub-step's first
collision pass.  The inherited _step handles the two types interleaved per phase and calls _solve_follow_constraint for
white, then for yolk: the pass hangs behind the second call.  CouplingMixin holds it, so that a test can put it on top of
tests/wall_model.py's WallModel as well.

With `factor` > 0 and particles of both types, H = max(1.0, factor (white max_radius + yolk max_radius)):

  * cells: floor(x / H), floor(y / H), per type, from the positions the follow has just written;
  * candidates of particle i of one type: every particle of the OTHER type in i's 3x3 cells, x offset -1..1 outer, y
    offset inner, ascending index (within its type) inside a cell;
  * pair (a, b), a the white particle, b the yolk one: relaxed_model.pair_shares with overlap = factor,
    compliance = (1 - strength) / sub_delta^2 and da = b - a of the two indices; white takes (cax, cay), yolk (cbx, cby);
  * sums start at +0.0 and add the shares in visit order, n_i counts the fired pairs;
    x_i = x_i + (sx * omega) / n_i when n_i > 0, else the position is copied; every pair reads start-of-pass positions.

`coupling_solves` counts the distinct cross pairs that fired (by the white side), over all steps; `coupling_coincident`
the fired pairs with d2 == 0.  numpy float64 element-wise in exactly this order.  Written from the definition, not from
the kernel."""
import numpy as np

from relaxed_model import pair_shares, rm
from viscosity_model import ViscosityModel


def _cells(v, H):
    with np.errstate(invalid="ignore"):
        return np.floor(v / H).astype(np.int64)


def couple_side(own, other, own_is_white, H, factor, compliance, omega, eps=rm.EPS):
    """One side of the coupling pass: `own` and `other` are (x, y, inverse mass, radius) of the two types at the start of
    the pass.  Returns (new x, new y of own, pairs that fired, fired pairs with d2 == 0)."""
    x, y, w, r = (np.asarray(v, dtype=np.float64) for v in own)
    ox_, oy_, ow, orad = (np.asarray(v, dtype=np.float64) for v in other)
    n, m = len(x), len(ox_)
    cx, cy = _cells(x, H), _cells(y, H)
    ocx, ocy = _cells(ox_, H), _cells(oy_, H)
    oidx = np.arange(m)
    idx = np.arange(n)
    order = np.lexsort((oidx, ocy, ocx))  # the other type's cells sorted by (cx, cy), ascending index inside a cell
    skx, sky = ocx[order], ocy[order]
    first = np.ones(m, dtype=bool)
    first[1:] = (skx[1:] != skx[:-1]) | (sky[1:] != sky[:-1])
    starts = np.flatnonzero(first)
    ends = np.append(starts[1:], m)
    ux, uy = skx[starts], sky[starts]
    sx = np.zeros(n)
    sy = np.zeros(n)
    cnt = np.zeros(n, dtype=np.int64)
    fired_total = coincident = 0
    for ox in (-1, 0, 1):
        for oy in (-1, 0, 1):
            qx, qy = cx + ox, cy + oy
            pos = np.searchsorted(ux * (1 << 32) + (uy + (1 << 31)), qx * (1 << 32) + (qy + (1 << 31)))
            posc = np.minimum(pos, len(ux) - 1)
            hit = (pos < len(ux)) & (ux[posc] == qx) & (uy[posc] == qy)
            st = np.where(hit, starts[posc], 0)
            en = np.where(hit, ends[posc], 0)
            for e in range(int((en - st).max())):
                valid = st + e < en
                j = order[np.minimum(st + e, m - 1)]
                if own_is_white:  # a = own (white), b = other (yolk)
                    cax, cay, _, _, _, fired = pair_shares(x, y, ox_[j], oy_[j], w, ow[j], r, orad[j], j - idx, factor,
                                                           compliance, eps)
                    mx, my = cax, cay
                    d2zero = (ox_[j] - x) * (ox_[j] - x) + (oy_[j] - y) * (oy_[j] - y) == 0.0
                else:  # a = other (white), b = own (yolk)
                    _, _, cbx, cby, _, fired = pair_shares(ox_[j], oy_[j], x, y, ow[j], w, orad[j], r, idx - j, factor,
                                                           compliance, eps)
                    mx, my = cbx, cby
                    d2zero = (x - ox_[j]) * (x - ox_[j]) + (y - oy_[j]) * (y - oy_[j]) == 0.0
                take = valid & fired
                sx = sx + np.where(take, mx, 0.0)  # (starts at +0.0 and never becomes -0.0: adding +0.0 is a no-op)
                sy = sy + np.where(take, my, 0.0)
                cnt += take
                fired_total += int(np.count_nonzero(take))
                coincident += int(np.count_nonzero(take & d2zero))
    nx, ny = x.copy(), y.copy()
    moved = cnt > 0
    nd = cnt[moved].astype(np.float64)
    nx[moved] = x[moved] + (sx[moved] * omega) / nd
    ny[moved] = y[moved] + (sy[moved] * omega) / nd
    return nx, ny, fired_total, coincident


def coupling_pass(white, yolk, white_max_radius, yolk_max_radius, factor, compliance, omega, eps=rm.EPS):
    """The coupling pass over both types, each (x, y, inverse mass, radius).  Returns
    ((new white x, y), (new yolk x, y), distinct pairs that fired, of them coincident)."""
    H = max(1.0, factor * (white_max_radius + yolk_max_radius))
    wx, wy, solves, coincident = couple_side(white, yolk, True, H, factor, compliance, omega, eps)
    yx, yy, seen, _ = couple_side(yolk, white, False, H, factor, compliance, omega, eps)
    assert seen == solves  # both sides evaluate one expression per pair
    return (wx, wy), (yx, yy), solves, coincident


class CouplingMixin:
    """the coupling pass on top of any model of the relaxed family (set_coupling; the values may change between steps)"""

    coupling_factor = 0.0
    coupling_strength = 1.0
    coupling_solves = 0
    coupling_coincident = 0

    def set_coupling(self, factor=0.0, strength=1.0):
        assert 0.0 <= factor < float("inf") and 0.0 <= strength <= 1.0
        self.coupling_factor, self.coupling_strength = float(factor), float(strength)

    def _step(self, delta, n_sub_steps, n_collision_steps, visit_logs=None):
        self._coupling_sub_delta = max(delta / n_sub_steps, rm.EPS)
        super()._step(delta, n_sub_steps, n_collision_steps, visit_logs)

    def _solve_follow_constraint(self, particles, *args):
        super()._solve_follow_constraint(particles, *args)
        if particles is self._yolk_data:  # the follow of both types has run
            self._couple()

    def _couple(self):
        nw, ny = self._total_n_white_particles, self._total_n_yolk_particles
        if not (self.relaxed and self.coupling_factor > 0.0 and nw and ny):
            return
        sides = []
        for data, n in ((self._white_data, nw), (self._yolk_data, ny)):
            base = [rm.offset(p) for p in range(1, n + 1)]
            sides.append((data, base, tuple(np.array([data[i + off] for i in base], dtype=np.float64)
                                            for off in (rm.X, rm.Y, rm.INV_MASS, rm.RADIUS))))
        compliance = self._strength_to_compliance(self.coupling_strength, self._coupling_sub_delta)
        new_w, new_y, solves, coincident = coupling_pass(sides[0][2], sides[1][2], self._white_config["max_radius"],
                                                         self._yolk_config["max_radius"], self.coupling_factor,
                                                         compliance, self.relaxation,
                                                         self._white_config.get("eps", rm.EPS))  # the white config's, both sides
        for (data, base, _), (nx, ny_) in zip(sides, (new_w, new_y)):
            for k, i in enumerate(base):
                data[i + rm.X] = float(nx[k])
                data[i + rm.Y] = float(ny_[k])
        self.coupling_solves += solves
        self.coupling_coincident += coincident


class CouplingModel(CouplingMixin, ViscosityModel):
    """ViscosityModel with the coupling pass"""
