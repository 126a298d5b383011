"""CPU model of the relaxed-order collision pass.  Test helper, not collected.

RelaxedModel is oracle.reference_model.ReferenceModel with _solve_collision replaced, while `relaxed` is set, by one
Jacobi pass with constraint averaging.  Every other phase (pre-solve, follow, spatial hash, post-solve, the update
accumulator, add / remove) is inherited unchanged.  The pass is evaluated with numpy float64 element-wise operations
(IEEE, correctly rounded, no contraction), operation for operation as csrc/eggsim_relaxed.hip, so the two agree bit for
bit:

  * cells: the CELL_X / CELL_Y the inherited _rebuild_spatial_hash has just written (floor(x / cell));
  * candidates of i: every other particle of the type in i's 3x3 cells, cells x offset -1..1 outer, y offset inner,
    ascending particle index inside a cell;
  * pair (a, b), a < b: the reference's collision correction from the start-of-pass positions (wsum < eps: skipped;
    d2 <= min_distance^2: fires), except that a coincident pair (d2 == 0) takes the normal DIRS[(b - a) & 7];
  * dx_i, dy_i start at +0.0 and add i's shares in visit order; n_i counts the fired pairs;
  * x_i += (dx_i * omega) / n_i when n_i > 0.

The pass returns (number of distinct pairs with wsum >= eps, False): no budget cut."""
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from oracle import reference_model as rm  # noqa: E402

_S = float.fromhex("0x1.6a09e667f3bcdp-1")  # sqrt(1/2), rounded
DIRS = np.array([(1.0, 0.0), (_S, _S), (0.0, 1.0), (-_S, _S), (-1.0, 0.0), (-_S, -_S), (0.0, -1.0), (_S, -_S)])
DEFAULT_RELAXATION = 1.8  # EGG_OPT_RELAXATION's default (how it was chosen)


def pair_shares(ax, ay, bx, by, wa, wb, ra, rb, da, overlap, compliance, eps=rm.EPS):
    """The collision correction of pairs (a, b), a < b, element-wise: (cax, cay, cbx, cby, counted, fired).
    da = b - a (picks the normal of a coincident pair)."""
    ax, ay, bx, by, wa, wb, ra, rb = (np.asarray(v, dtype=np.float64) for v in (ax, ay, bx, by, wa, wb, ra, rb))
    wsum = wa + wb
    counted = ~(wsum < eps)
    dx = bx - ax
    dy = by - ay
    d2 = dx * dx + dy * dy
    md = overlap * (ra + rb)
    fired = counted & (d2 <= md * md)
    divisor = wsum + compliance
    with np.errstate(divide="ignore", invalid="ignore"):
        current = np.sqrt(d2)
        violation = current - md
        small = current < eps
        nx = np.where(small, 0.0, dx / current)
        ny = np.where(small, 0.0, dy / current)
        coincident = d2 == 0.0
        k = np.asarray(da, dtype=np.int64) & 7
        nx = np.where(coincident, DIRS[k, 0], nx)
        ny = np.where(coincident, DIRS[k, 1], ny)
        correction = -violation / divisor
        max_correction = np.abs(violation)
        correction = np.where(correction < -max_correction, -max_correction, correction)
        correction = np.where(correction > max_correction, max_correction, correction)
        dead = divisor < eps
        cax = np.where(dead, 0.0, -nx * correction * wa)
        cay = np.where(dead, 0.0, -ny * correction * wa)
        cbx = np.where(dead, 0.0, nx * correction * wb)
        cby = np.where(dead, 0.0, ny * correction * wb)
    return cax, cay, cbx, cby, counted, fired


def relaxed_pass(x, y, w, r, cx, cy, overlap, compliance, omega, eps=rm.EPS):
    """One relaxed pass over one particle type (0-based arrays).  Returns (new x, new y, distinct pairs counted)."""
    n = len(x)
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if n == 0:
        return x.copy(), y.copy(), 0
    cx = np.asarray(cx, dtype=np.int64)
    cy = np.asarray(cy, dtype=np.int64)
    idx = np.arange(n)
    # cells sorted by (cx, cy), ascending index inside a cell (stable)
    order = np.lexsort((idx, cy, cx))
    skx, sky = cx[order], cy[order]
    first = np.ones(n, dtype=bool)
    first[1:] = (skx[1:] != skx[:-1]) | (sky[1:] != sky[:-1])
    starts = np.flatnonzero(first)
    ends = np.append(starts[1:], n)
    ux, uy = skx[starts], sky[starts]
    dxs = np.zeros(n)
    dys = np.zeros(n)
    cnt = np.zeros(n, dtype=np.int64)
    pairs = 0
    for ox in (-1, 0, 1):
        for oy in (-1, 0, 1):
            qx, qy = cx + ox, cy + oy
            # locate cell (qx, qy) among the unique cells (sorted lexicographically)
            pos = np.searchsorted(ux * (1 << 32) + (uy + (1 << 31)), qx * (1 << 32) + (qy + (1 << 31)))
            posc = np.minimum(pos, len(ux) - 1)
            hit = (pos < len(ux)) & (ux[posc] == qx) & (uy[posc] == qy)
            st = np.where(hit, starts[posc], 0)
            en = np.where(hit, ends[posc], 0)
            for e in range(int((en - st).max())):
                valid = st + e < en
                j = order[np.minimum(st + e, n - 1)]
                valid &= j != idx
                a = np.minimum(idx, j)
                b = np.maximum(idx, j)
                cax, cay, cbx, cby, counted, fired = pair_shares(x[a], y[a], x[b], y[b], w[a], w[b], r[a], r[b], b - a,
                                                                 overlap, compliance, eps)
                mine = idx == a
                sx = np.where(mine, cax, cbx)
                sy = np.where(mine, cay, cby)
                take = valid & fired
                # (dx starts at +0.0 and never becomes -0.0, so adding +0.0 for the lanes that take nothing is a no-op)
                dxs = dxs + np.where(take, sx, 0.0)
                dys = dys + np.where(take, sy, 0.0)
                cnt += take
                pairs += int(np.count_nonzero(valid & counted & (j > idx)))
    nx_, ny_ = x.copy(), y.copy()
    moved = cnt > 0
    nd = cnt[moved].astype(np.float64)
    nx_[moved] = x[moved] + (dxs[moved] * omega) / nd
    ny_[moved] = y[moved] + (dys[moved] * omega) / nd
    return nx_, ny_, pairs


class RelaxedModel(rm.ReferenceModel):
    """ReferenceModel whose collision passes are relaxed while `relaxed` is set (it may change between steps)."""

    def __init__(self, white_config=None, yolk_config=None, relaxed=False, relaxation=DEFAULT_RELAXATION):
        self.relaxed = relaxed
        self.relaxation = relaxation
        self.relaxed_pass_pairs = []  # per pass of the most recent step: distinct pairs counted
        self.pair_solves = 0  # pairs counted over all steps (egg_stats.pair_solves)
        super().__init__(white_config, yolk_config)
        self.pair_solves = 0

    def _step(self, delta, n_sub_steps, n_collision_steps, visit_logs=None):
        self.relaxed_pass_pairs = []
        super()._step(delta, n_sub_steps, n_collision_steps, visit_logs)
        self.pair_solves += sum(n for (_, _, _, n, _) in self.pass_log)

    def _solve_collision(self, particles, n_particles, spatial_hash, collided, collision_overlap_factor,
                         collision_compliance, cohesion_interaction_distance_factor, cohesion_compliance,
                         max_n_collisions, visit_log=None):
        if not self.relaxed:
            return super()._solve_collision(particles, n_particles, spatial_hash, collided, collision_overlap_factor,
                                            collision_compliance, cohesion_interaction_distance_factor,
                                            cohesion_compliance, max_n_collisions, visit_log)
        if n_particles == 0:
            self.relaxed_pass_pairs.append(0)
            return 0, False
        base = [rm.offset(p) for p in range(1, n_particles + 1)]

        def col(off):
            return np.array([particles[i + off] for i in base], dtype=np.float64)

        cx = np.array([particles[i + rm.CELL_X] for i in base], dtype=np.int64)
        cy = np.array([particles[i + rm.CELL_Y] for i in base], dtype=np.int64)
        x, y = col(rm.X), col(rm.Y)
        nx, ny, pairs = relaxed_pass(x, y, col(rm.INV_MASS), col(rm.RADIUS), cx, cy, collision_overlap_factor,
                                     collision_compliance, self.relaxation)
        for k, i in enumerate(base):
            particles[i + rm.X] = float(nx[k])
            particles[i + rm.Y] = float(ny[k])
        self.relaxed_pass_pairs.append(pairs)
        return pairs, False

    # readout helpers
    def state(self, which):
        return np.array([self.field(which, off) for off in (rm.X, rm.Y, rm.VX, rm.VY, rm.LAST_X, rm.LAST_Y)],
                        dtype=np.float64)

    def n_particles(self, which):
        return self._total_n_white_particles if which == 0 else self._total_n_yolk_particles
