"""CPU model of the relaxed pass split over the handles of a device group ("Several devices").
Test helper, not collected.

Every particle has a global key (its index in one handle holding everything) and an owner (the slab that holds it).
Per pass and owner k:
  * box: the cells of k's particles, min / max cx and cy;
  * ghosts: every other owner's particle whose cell lies in that box grown by one cell on each side;
  * the pass of relaxed_model.relaxed_pass over k's particles plus the ghosts, in ANY entry order, with the global key
    in place of the index: ascending key inside a cell, pair (a, b) oriented by key, the coincident normal by the key
    difference, a pair counted only by the local side with the smaller key;
  * only k's own particles take the result.
GroupRelaxedModel runs RelaxedModel with this pass; it equals RelaxedModel bit for bit, which is the halo rule."""
import numpy as np

import relaxed_model as rx
from oracle import reference_model as rm


def keyed_pass(x, y, w, r, cx, cy, key, local, overlap, compliance, omega, eps=rm.EPS):
    """relaxed_pass over entries in any order, ordered by `key`; returns (new x, new y, pairs) -- positions of the
    entries that are not `local` are returned unchanged, and only local entries count pairs"""
    n = len(x)
    x, y, w, r = (np.asarray(v, dtype=np.float64) for v in (x, y, w, r))
    cx, cy, key = (np.asarray(v, dtype=np.int64) for v in (cx, cy, key))
    local = np.asarray(local, dtype=bool)
    if n == 0:
        return x.copy(), y.copy(), 0
    me = np.arange(n)
    order = np.lexsort((key, cy, cx))
    skx, sky = cx[order], cy[order]
    first = np.ones(n, dtype=bool)
    first[1:] = (skx[1:] != skx[:-1]) | (sky[1:] != sky[:-1])
    starts = np.flatnonzero(first)
    ends = np.append(starts[1:], n)
    ux, uy = skx[starts], sky[starts]
    dxs, dys = np.zeros(n), np.zeros(n)
    cnt = np.zeros(n, dtype=np.int64)
    pairs = 0
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
                valid &= j != me
                lower = key < key[j]  # this entry is side a of the pair
                a = np.where(lower, me, j)
                b = np.where(lower, j, me)
                cax, cay, cbx, cby, counted, fired = rx.pair_shares(x[a], y[a], x[b], y[b], w[a], w[b], r[a], r[b],
                                                                    key[b] - key[a], overlap, compliance, eps)
                sx = np.where(lower, cax, cbx)
                sy = np.where(lower, cay, cby)
                take = valid & fired
                dxs = dxs + np.where(take, sx, 0.0)
                dys = dys + np.where(take, sy, 0.0)
                cnt += take
                pairs += int(np.count_nonzero(valid & counted & lower & local))
    nx_, ny_ = x.copy(), y.copy()
    moved = (cnt > 0) & local
    nd = cnt[moved].astype(np.float64)
    nx_[moved] = x[moved] + (dxs[moved] * omega) / nd
    ny_[moved] = y[moved] + (dys[moved] * omega) / nd
    return nx_, ny_, pairs


def ghosts_of(owner, cx, cy, k):
    """particles of other owners within one cell of owner k's cell box"""
    loc = owner == k
    if not loc.any():
        return np.zeros(len(owner), dtype=bool)
    lox, hix = cx[loc].min() - 1, cx[loc].max() + 1
    loy, hiy = cy[loc].min() - 1, cy[loc].max() + 1
    return ~loc & (cx >= lox) & (cx <= hix) & (cy >= loy) & (cy <= hiy)


def decomposed_pass(x, y, w, r, cx, cy, owner, overlap, compliance, omega, seed=0, eps=rm.EPS):
    """relaxed_pass of the particles in global key order (0-based arrays), computed per owner over its particles plus
    its ghosts, each owner's entries in a shuffled order.  Returns (new x, new y, pairs, ghost records)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    cx, cy = np.asarray(cx, dtype=np.int64), np.asarray(cy, dtype=np.int64)
    owner = np.asarray(owner)
    keys = np.arange(len(x))
    out_x, out_y = x.copy(), y.copy()
    pairs = records = 0
    rng = np.random.default_rng(seed)
    for k in np.unique(owner):
        loc = owner == k
        gh = ghosts_of(owner, cx, cy, k)
        ent = rng.permutation(np.flatnonzero(loc | gh))
        nx_, ny_, p = keyed_pass(x[ent], y[ent], w[ent], r[ent], cx[ent], cy[ent], keys[ent], loc[ent], overlap,
                                 compliance, omega, eps)
        mine = loc[ent]
        out_x[ent[mine]] = nx_[mine]
        out_y[ent[mine]] = ny_[mine]
        pairs += p
        records += int(np.count_nonzero(gh))
    return out_x, out_y, pairs, records


class GroupRelaxedModel(rx.RelaxedModel):
    """RelaxedModel whose relaxed passes run decomposed: the owner of a particle is the x-slab [cuts[k], cuts[k + 1])
    its position lies in at the start of the pass (any partition would do: the halo rule does not depend on it)."""

    def __init__(self, cuts, **kw):
        self.cuts = np.asarray(cuts, dtype=np.float64)
        self.ghost_records = 0
        self._passes = 0
        super().__init__(**kw)

    def _solve_collision(self, particles, n_particles, spatial_hash, collided, collision_overlap_factor,
                         collision_compliance, cohesion_interaction_distance_factor, cohesion_compliance,
                         max_n_collisions, visit_log=None):
        if not self.relaxed or n_particles == 0:
            return super()._solve_collision(particles, n_particles, spatial_hash, collided, collision_overlap_factor,
                                            collision_compliance, cohesion_interaction_distance_factor,
                                            cohesion_compliance, max_n_collisions, visit_log)
        base = [rm.offset(p) for p in range(1, n_particles + 1)]

        def col(off):
            return np.array([particles[i + off] for i in base], dtype=np.float64)

        cx = np.array([particles[i + rm.CELL_X] for i in base], dtype=np.int64)
        cy = np.array([particles[i + rm.CELL_Y] for i in base], dtype=np.int64)
        x, y = col(rm.X), col(rm.Y)
        owner = np.searchsorted(self.cuts, x, side="right")
        self._passes += 1
        nx, ny, pairs, records = decomposed_pass(x, y, col(rm.INV_MASS), col(rm.RADIUS), cx, cy, owner,
                                                 collision_overlap_factor, collision_compliance, self.relaxation,
                                                 seed=self._passes)
        for k, i in enumerate(base):
            particles[i + rm.X] = float(nx[k])
            particles[i + rm.Y] = float(ny[k])
        self.relaxed_pass_pairs.append(pairs)
        self.ghost_records += records
        return pairs, False
