"""CPU model of the relaxed pass with effective cohesion (EGG_OPT_COHESION = 1; DESIGN.md section 2.7, "Cohesion").  Test
helper, not collected.

CohesiveModel is tests/relaxed_model.py's RelaxedModel whose relaxed pass, while `cohesion` is set, lets a pair that does
not collide cohere.  Pair (a, b), a < b, candidates and visit order as in the relaxed pass; with md = overlap (ra + rb),
reach = cohesion_interaction_distance_factor (ra + rb) and d2 from the pass's start positions:

  * d2 <= md^2: the collision correction, unchanged (collision compliance, the coincident pair's normal);
  * otherwise, when a and b carry the same BATCH_ID and d2 <= reach^2: the SAME expressions in the same order with the
    cohesion compliance -- the target distance stays md, so violation = current - md > 0 and the pair is pulled together,
    never closer than the collision distance;
  * a pair fires at most one of the two; n_i counts the fired pairs of either kind, shares add in visit order.

numpy float64 element-wise, operation for operation as the cohesive instantiations of csrc/eggsim_relaxed.hip: the two
kinds share relaxed_model.pair_shares, evaluated once per compliance.  With `cohesion` unset every pass is RelaxedModel's.
`cohesion_solves` counts the distinct pairs whose cohesion branch fired, over all steps (egg_stats.cohesion_solves)."""
import numpy as np

import relaxed_model as rxm
from relaxed_model import rm


def cohesive_pass(x, y, w, r, cx, cy, batch, overlap, compliance, omega, factor, cohesion_compliance, eps=rm.EPS):
    """One relaxed pass with effective cohesion over one particle type (0-based arrays; batch: any integer that is equal
    for two particles exactly when they share a batch).  Returns (new x, new y, distinct pairs counted, distinct pairs
    that cohered)."""
    n = len(x)
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if n == 0:
        return x.copy(), y.copy(), 0, 0
    w = np.asarray(w, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    cx = np.asarray(cx, dtype=np.int64)
    cy = np.asarray(cy, dtype=np.int64)
    batch = np.asarray(batch, dtype=np.int64)
    idx = np.arange(n)
    order = np.lexsort((idx, cy, cx))  # cells sorted by (cx, cy), ascending index inside a cell
    skx, sky = cx[order], cy[order]
    first = np.ones(n, dtype=bool)
    first[1:] = (skx[1:] != skx[:-1]) | (sky[1:] != sky[:-1])
    starts = np.flatnonzero(first)
    ends = np.append(starts[1:], n)
    ux, uy = skx[starts], sky[starts]
    dxs = np.zeros(n)
    dys = np.zeros(n)
    cnt = np.zeros(n, dtype=np.int64)
    pairs = cohered = 0
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
                j = order[np.minimum(st + e, n - 1)]
                valid &= j != idx
                a = np.minimum(idx, j)
                b = np.maximum(idx, j)
                args = (x[a], y[a], x[b], y[b], w[a], w[b], r[a], r[b], b - a, overlap)
                col = rxm.pair_shares(*args, compliance, eps)
                coh = rxm.pair_shares(*args, cohesion_compliance, eps)
                counted, collides = col[4], col[5]
                dx = x[b] - x[a]
                dy = y[b] - y[a]
                d2 = dx * dx + dy * dy
                reach = factor * (r[a] + r[b])
                coheres = counted & ~collides & (batch[a] == batch[b]) & (d2 <= reach * reach)
                mine = idx == a
                sx = np.where(coheres, np.where(mine, coh[0], coh[2]), np.where(mine, col[0], col[2]))
                sy = np.where(coheres, np.where(mine, coh[1], coh[3]), np.where(mine, col[1], col[3]))
                take = valid & (collides | coheres)
                dxs = dxs + np.where(take, sx, 0.0)
                dys = dys + np.where(take, sy, 0.0)
                cnt += take
                pairs += int(np.count_nonzero(valid & counted & (j > idx)))
                cohered += int(np.count_nonzero(valid & coheres & (j > idx)))
    nx_, ny_ = x.copy(), y.copy()
    moved = cnt > 0
    nd = cnt[moved].astype(np.float64)
    nx_[moved] = x[moved] + (dxs[moved] * omega) / nd
    ny_[moved] = y[moved] + (dys[moved] * omega) / nd
    return nx_, ny_, pairs, cohered


class CohesiveModel(rxm.RelaxedModel):
    """RelaxedModel whose relaxed passes cohere while `cohesion` is set (it may change between steps, like `relaxed`)."""

    def __init__(self, white_config=None, yolk_config=None, relaxed=True, relaxation=rxm.DEFAULT_RELAXATION, cohesion=False):
        self.cohesion = cohesion
        self.cohesion_solves = 0
        super().__init__(white_config, yolk_config, relaxed, relaxation)

    def _solve_collision(self, particles, n_particles, spatial_hash, collided, collision_overlap_factor,
                         collision_compliance, cohesion_interaction_distance_factor, cohesion_compliance,
                         max_n_collisions, visit_log=None):
        if not (self.relaxed and self.cohesion) or n_particles == 0:
            return super()._solve_collision(particles, n_particles, spatial_hash, collided, collision_overlap_factor,
                                            collision_compliance, cohesion_interaction_distance_factor,
                                            cohesion_compliance, max_n_collisions, visit_log)
        base = [rm.offset(p) for p in range(1, n_particles + 1)]

        def col(off, dtype=np.float64):
            return np.array([particles[i + off] for i in base], dtype=dtype)

        nx, ny, pairs, cohered = cohesive_pass(col(rm.X), col(rm.Y), col(rm.INV_MASS), col(rm.RADIUS),
                                               col(rm.CELL_X, np.int64), col(rm.CELL_Y, np.int64),
                                               col(rm.BATCH_ID, np.int64), collision_overlap_factor, collision_compliance,
                                               self.relaxation, cohesion_interaction_distance_factor, cohesion_compliance)
        for k, i in enumerate(base):
            particles[i + rm.X] = float(nx[k])
            particles[i + rm.Y] = float(ny[k])
        self.relaxed_pass_pairs.append(pairs)
        self.cohesion_solves += cohered
        return pairs, False
