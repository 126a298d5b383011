"""CPU model of the relaxed step with viscosity (egg_set_viscosity; DESIGN.md section 2.7, "Viscosity").  Test helper, not
collected.

ViscosityModel is tests/force_model.py's ForceModel (so one model covers cohesion, colliders and forces off and on) whose
post-solve is preceded, for a type with coefficient c in (0, 1], by the XSPH pass.  It runs in every sub-step of a relaxed
step, after the sub-step's last collision pass (collider projection included) and before the velocity is taken.  Positions
are not touched; the pass rewrites PX / PY, the start-of-sub-step positions from which the post-solve derives the velocity.
With p_i the position of particle i, u_i = (p_i.x - prev_i.x, p_i.y - prev_i.y) (every u taken before any prev is rewritten)
and H the type's spatial_hash_cell_radius of the step:

  1. cells: floor(p / H), fresh from the current positions;
  2. candidates of i: every other particle of the type in i's 3x3 cells, x offset -1..1 outer, y offset inner, ascending
     particle index inside a cell;
  3. per candidate j: dx = p_j.x - p_i.x, dy = p_j.y - p_i.y, d2 = dx dx + dy dy; !(d2 < H H): skipped; otherwise
     d = sqrt(d2), w = 1 - d / H, sw = sw + w, sx = sx + w (u_j.x - u_i.x), sy = sy + w (u_j.y - u_i.y); sums start at +0.0;
  4. !(inv_mass_i > eps) or !(sw > 0): prev_i keeps its bits;
  5. otherwise nux = u_i.x + c (sx / sw), nuy = u_i.y + c (sy / sw), prev_i = (p_i.x - nux, p_i.y - nuy).

numpy float64 element-wise in exactly this order; every comparison is false for a NaN.  `viscosity_pairs` counts per type
the distinct pairs with d2 < H H over all viscosity passes of all steps.  Written from the definition, not from the
kernel."""
import numpy as np

from force_model import ForceModel
from relaxed_model import rm


def xsph(x, y, px, py, im, H, c, eps=rm.EPS):
    """the viscosity pass over one particle type (0-based arrays).  Returns (new px, new py, distinct pairs within H,
    new ux, new uy): px / py keep their bits where step 4 says so."""
    x, y, px, py, im = (np.asarray(v, dtype=np.float64) for v in (x, y, px, py, im))
    n = len(x)
    if n == 0:
        return px.copy(), py.copy(), 0, np.zeros(0), np.zeros(0)
    ux = x - px
    uy = y - py
    with np.errstate(invalid="ignore"):
        cx = np.floor(x / H).astype(np.int64)
        cy = np.floor(y / H).astype(np.int64)
    idx = np.arange(n)
    order = np.lexsort((idx, cy, cx))  # cells sorted by (cx, cy), ascending index inside a cell
    skx, sky = cx[order], cy[order]
    first = np.ones(n, dtype=bool)
    first[1:] = (skx[1:] != skx[:-1]) | (sky[1:] != sky[:-1])
    starts = np.flatnonzero(first)
    ends = np.append(starts[1:], n)
    qx_, qy_ = skx[starts], sky[starts]
    sw = np.zeros(n)
    sx = np.zeros(n)
    sy = np.zeros(n)
    pairs = 0
    H2 = H * H
    for ox in (-1, 0, 1):
        for oy in (-1, 0, 1):
            qx, qy = cx + ox, cy + oy
            pos = np.searchsorted(qx_ * (1 << 32) + (qy_ + (1 << 31)), qx * (1 << 32) + (qy + (1 << 31)))
            posc = np.minimum(pos, len(qx_) - 1)
            hit = (pos < len(qx_)) & (qx_[posc] == qx) & (qy_[posc] == qy)
            st = np.where(hit, starts[posc], 0)
            en = np.where(hit, ends[posc], 0)
            for e in range(int((en - st).max())):
                valid = st + e < en
                j = order[np.minimum(st + e, n - 1)]
                valid &= j != idx
                dx = x[j] - x
                dy = y[j] - y
                d2 = dx * dx + dy * dy
                take = valid & (d2 < H2)
                with np.errstate(invalid="ignore"):
                    d = np.sqrt(d2)
                    w = 1.0 - d / H
                    # (the sums start at +0.0; a lane that takes nothing keeps its bits)
                    sw = np.where(take, sw + w, sw)
                    sx = np.where(take, sx + w * (ux[j] - ux), sx)
                    sy = np.where(take, sy + w * (uy[j] - uy), sy)
                pairs += int(np.count_nonzero(take & (j > idx)))
    with np.errstate(invalid="ignore", divide="ignore"):
        move = (im > eps) & (sw > 0.0)
        nux = ux + c * (sx / sw)
        nuy = uy + c * (sy / sw)
        npx = np.where(move, x - nux, px)
        npy = np.where(move, y - nuy, py)
    return npx, npy, pairs, np.where(move, nux, ux), np.where(move, nuy, uy)


class ViscosityModel(ForceModel):
    """ForceModel whose post-solve is preceded by the viscosity pass of the types whose coefficient is not zero
    (set_viscosity; the coefficients may change between steps)."""

    def __init__(self, white_config=None, yolk_config=None, relaxed=True, relaxation=None, cohesion=False):
        self.viscosity = (0.0, 0.0)
        self.viscosity_pairs = [0, 0]
        super().__init__(white_config, yolk_config, relaxed, relaxation=relaxation, cohesion=cohesion)

    def set_viscosity(self, white=0.0, yolk=0.0):
        for v in (white, yolk):
            assert 0.0 <= v <= 1.0
        self.viscosity = (float(white), float(yolk))

    def _cell(self, which):
        config = self._white_config if which == 0 else self._yolk_config
        return max(1, config["max_radius"] * max(config["collision_overlap_factor"],
                                                 config["cohesion_interaction_distance_factor"]))

    def _post_solve(self, particles, n_particles, delta):
        which = 0 if particles is self._white_data else 1
        c = self.viscosity[which]
        if self.relaxed and c > 0.0 and n_particles:
            base = [rm.offset(p) for p in range(1, n_particles + 1)]

            def col(off):
                return np.array([particles[i + off] for i in base], dtype=np.float64)

            px, py, pairs, _, _ = xsph(col(rm.X), col(rm.Y), col(rm.PX), col(rm.PY), col(rm.INV_MASS),
                                       float(self._cell(which)), c)
            for k, i in enumerate(base):
                particles[i + rm.PX] = float(px[k])
                particles[i + rm.PY] = float(py[k])
            self.viscosity_pairs[which] += pairs
        return rm.ReferenceModel._post_solve(particles, n_particles, delta)
