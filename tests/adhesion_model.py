"""CPU model of the relaxed step with white-yolk adhesion (egg_set_adhesion; DESIGN.md section 2.7, "Adhesion").  Test
helper, not collected.

AdhesionMixin sits on tests/coupling_model.py's CouplingMixin the way CouplingMixin sits on the relaxed family: it holds
`reach` (0 = off) and `strength`, and replaces the coupling pass while adhesion ACTS, which it does in a step exactly when

  * coupling acts (factor > 0 and both types have particles),
  * reach > factor,
  * the solver order is relaxed.

Otherwise the pass is CouplingMixin's, untouched.  When it acts the coupling pass changes in three places:

  * cells: H = max(1.0, max(factor, reach) (white max_radius + yolk max_radius)); candidates, visit order (x offset
    outer, y offset inner, ascending index inside a cell) and the wsum < eps skip are the coupling pass's;
  * pair (a white, b yolk), md = factor (ra + rb), rd = reach (ra + rb), d2 from the start-of-pass positions:
    d2 <= md md: the coupling correction (relaxed_model.pair_shares with overlap = factor and coupling's compliance);
    otherwise, when a and b carry the same BATCH_ID and d2 <= rd rd: the adhesion branch -- pair_shares once more with
    the SAME target distance md and adhesion's own compliance (1 - strength) / sub_delta^2, so violation = current - md > 0
    and the pair is pulled together, never closer than md by its own share;
  * a pair fires at most one branch; n_i counts the fires of either kind, shares add in visit order, and
    x_i = x_i + (sx * omega) / n_i when n_i > 0.

`adhesion_solves` counts the distinct cross pairs whose adhesion branch fired (by the white side); `coupling_solves` keeps
counting coupling-branch fires only.  numpy float64 element-wise in exactly this order; written from the definition, not
from the kernel.

The census.  Every evaluation (one particle i looking at one candidate j of the other type) is labelled from its inputs
alone, per side ("white_side": the white particle evaluates, "yolk_side"), in `adhesion_census[side][label]`:

  skipped      wsum < eps
  couples      the coupling branch fired
  md_edge      d2 == md md exactly, still couples
  adheres      the adhesion branch fired
  reach_edge   d2 == rd rd exactly, adheres
  other_batch  in the band, different batch, nothing
  beyond       beyond rd
  tiny         current < eps in the band: adheres with a zero normal, zero shares, n still counts it
  clamped      a branch fired and the clamp +-|violation| bound the correction
  unclamped    a branch fired and it did not

`rule` (None in the model) names one deliberately WRONG rule for tests/test_adhesion_model.py's sensitivity test."""
import numpy as np

from coupling_model import CouplingMixin, _cells
from relaxed_model import pair_shares, rm
from viscosity_model import ViscosityModel

LABELS = ("skipped", "couples", "md_edge", "adheres", "reach_edge", "other_batch", "beyond", "tiny", "clamped", "unclamped")
SIDES = ("white_side", "yolk_side")
RULES = ("no_batch_test", "reach_lt", "target_rd", "coupling_compliance", "cell_from_factor", "adhesion_first", "per_type_tag")


def adhesion_cell(white_max_radius, yolk_max_radius, factor, reach):
    """H of the coupling pass while adhesion acts"""
    return max(1.0, max(factor, reach) * (white_max_radius + yolk_max_radius))


def adhere_side(own, other, own_batch, other_batch, own_is_white, H, factor, compliance, reach, adhesion_compliance, omega,
                eps=rm.EPS, rule=None):
    """One side of the coupling pass with the adhesion band: `own` and `other` are (x, y, inverse mass, radius) of the two
    types at the start of the pass, own_batch / other_batch an integer per particle that is equal for two particles
    exactly when one add created them.  Returns (new x, new y of own, pairs that coupled, of them coincident, pairs that
    adhered, {label: evaluations})."""
    x, y, w, r = (np.asarray(v, dtype=np.float64) for v in own)
    ox_, oy_, ow, orad = (np.asarray(v, dtype=np.float64) for v in other)
    tag, otag = np.asarray(own_batch, dtype=np.int64), np.asarray(other_batch, dtype=np.int64)
    n, m = len(x), len(ox_)
    cx, cy = _cells(x, H), _cells(y, H)
    ocx, ocy = _cells(ox_, H), _cells(oy_, H)
    idx = np.arange(n)
    order = np.lexsort((np.arange(m), ocy, ocx))  # the other type's cells sorted by (cx, cy), ascending index inside a cell
    skx, sky = ocx[order], ocy[order]
    first = np.ones(m, dtype=bool)
    first[1:] = (skx[1:] != skx[:-1]) | (sky[1:] != sky[:-1])
    starts = np.flatnonzero(first)
    ends = np.append(starts[1:], m)
    ux, uy = skx[starts], sky[starts]
    sx = np.zeros(n)
    sy = np.zeros(n)
    cnt = np.zeros(n, dtype=np.int64)
    coupled = coincident = adhered = 0
    census = dict.fromkeys(LABELS, 0)
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
                    args = (x, y, ox_[j], oy_[j], w, ow[j], r, orad[j], j - idx)
                else:  # a = other (white), b = own (yolk)
                    args = (ox_[j], oy_[j], x, y, ow[j], w, orad[j], r, idx - j)
                ax, ay, bx, by, wa, wb, ra, rb, _ = args
                col = pair_shares(*args, factor, compliance, eps)
                adh = pair_shares(*args, reach if rule == "target_rd" else factor,
                                  compliance if rule == "coupling_compliance" else adhesion_compliance, eps)
                counted, couples = col[4], col[5]
                dx = bx - ax
                dy = by - ay
                d2 = dx * dx + dy * dy
                md = factor * (ra + rb)
                rd = reach * (ra + rb)
                same = np.ones(n, dtype=bool) if rule == "no_batch_test" else tag == otag[j]
                within = d2 < rd * rd if rule == "reach_lt" else d2 <= rd * rd
                if rule == "adhesion_first":
                    adheres = counted & same & within
                    couples = couples & ~adheres
                else:
                    adheres = counted & ~couples & same & within
                mine_col, mine_adh = (col[0:2], adh[0:2]) if own_is_white else (col[2:4], adh[2:4])
                mx = np.where(adheres, mine_adh[0], mine_col[0])
                my = np.where(adheres, mine_adh[1], mine_col[1])
                take = valid & (couples | adheres)
                sx = sx + np.where(take, mx, 0.0)  # (starts at +0.0 and never becomes -0.0: adding +0.0 is a no-op)
                sy = sy + np.where(take, my, 0.0)
                cnt += take
                coupled += int(np.count_nonzero(valid & couples))
                coincident += int(np.count_nonzero(valid & couples & (d2 == 0.0)))
                adhered += int(np.count_nonzero(valid & adheres))
                # ---- the census: from the inputs of the evaluation alone
                with np.errstate(divide="ignore", invalid="ignore"):
                    wsum = wa + wb
                    current = np.sqrt(d2)
                    violation = current - md
                    raw = -violation / (wsum + np.where(adheres, adhesion_compliance, compliance))
                    bound = (raw < -np.abs(violation)) | (raw > np.abs(violation))
                fires = couples | adheres
                live = fires & ~(wsum + np.where(adheres, adhesion_compliance, compliance) < eps)
                for label, lanes in (("skipped", ~counted), ("couples", couples), ("md_edge", couples & (d2 == md * md)),
                                     ("adheres", adheres), ("reach_edge", adheres & (d2 == rd * rd)),
                                     ("other_batch", counted & ~fires & ~same & within),
                                     ("beyond", counted & ~fires & ~within), ("tiny", adheres & (current < eps)),
                                     ("clamped", live & bound), ("unclamped", live & ~bound)):
                    census[label] += int(np.count_nonzero(valid & lanes))
    nx, ny = x.copy(), y.copy()
    moved = cnt > 0
    nd = cnt[moved].astype(np.float64)
    nx[moved] = x[moved] + (sx[moved] * omega) / nd
    ny[moved] = y[moved] + (sy[moved] * omega) / nd
    return nx, ny, coupled, coincident, adhered, census


def _per_type_tags(batch):
    """the WRONG tag of rule per_type_tag: a batch's place among the batches that have particles of this type"""
    batch = np.asarray(batch, dtype=np.int64)
    return np.searchsorted(np.unique(batch), batch)


def adhesion_pass(white, yolk, white_batch, yolk_batch, white_max_radius, yolk_max_radius, factor, compliance, reach,
                  adhesion_compliance, omega, eps=rm.EPS, rule=None):
    """The coupling pass with the adhesion band over both types, each (x, y, inverse mass, radius).  Returns
    ((new white x, y), (new yolk x, y), distinct pairs that coupled, of them coincident, distinct pairs that adhered,
    {side: {label: evaluations}})."""
    H = adhesion_cell(white_max_radius, yolk_max_radius, factor, factor if rule == "cell_from_factor" else reach)
    if rule == "per_type_tag":
        white_batch, yolk_batch = _per_type_tags(white_batch), _per_type_tags(yolk_batch)
    wx, wy, coupled, coincident, adhered, cw = adhere_side(white, yolk, white_batch, yolk_batch, True, H, factor, compliance,
                                                           reach, adhesion_compliance, omega, eps, rule)
    yx, yy, seen_c, _, seen_a, cy = adhere_side(yolk, white, yolk_batch, white_batch, False, H, factor, compliance, reach,
                                                adhesion_compliance, omega, eps, rule)
    assert (seen_c, seen_a) == (coupled, adhered) and cw == cy  # both sides evaluate one expression per pair
    return (wx, wy), (yx, yy), coupled, coincident, adhered, {"white_side": cw, "yolk_side": cy}


class AdhesionMixin:
    """the adhesion band on top of CouplingMixin (set_adhesion; the values may change between steps)"""

    adhesion_reach = 0.0
    adhesion_strength = 1.0
    adhesion_solves = 0
    adhesion_rule = None  # (tests only: one of RULES)

    def set_adhesion(self, reach=0.0, strength=1.0):
        assert 0.0 <= reach < float("inf") and 0.0 <= strength <= 1.0
        self.adhesion_reach, self.adhesion_strength = float(reach), float(strength)

    def adhesion_acts(self):
        nw, ny = self._total_n_white_particles, self._total_n_yolk_particles
        return bool(self.relaxed and self.coupling_factor > 0.0 and nw and ny and self.adhesion_reach > self.coupling_factor)

    def _couple(self):
        if not self.adhesion_acts():
            return super()._couple()
        if not hasattr(self, "adhesion_census"):
            self.adhesion_census = {side: dict.fromkeys(LABELS, 0) for side in SIDES}
        sides = []
        for data, n in ((self._white_data, self._total_n_white_particles), (self._yolk_data, self._total_n_yolk_particles)):
            base = [rm.offset(p) for p in range(1, n + 1)]
            sides.append((data, base, tuple(np.array([data[i + off] for i in base], dtype=np.float64)
                                            for off in (rm.X, rm.Y, rm.INV_MASS, rm.RADIUS)),
                          np.array([data[i + rm.BATCH_ID] for i in base], dtype=np.int64)))
        compliance = self._strength_to_compliance(self.coupling_strength, self._coupling_sub_delta)
        adhesion_compliance = self._strength_to_compliance(self.adhesion_strength, self._coupling_sub_delta)
        new_w, new_y, coupled, coincident, adhered, census = adhesion_pass(
            sides[0][2], sides[1][2], sides[0][3], sides[1][3], self._white_config["max_radius"],
            self._yolk_config["max_radius"], self.coupling_factor, compliance, self.adhesion_reach, adhesion_compliance,
            self.relaxation, self._white_config.get("eps", rm.EPS), self.adhesion_rule)  # the white config's eps, both sides
        for (data, base, _, _), (nx, ny_) in zip(sides, (new_w, new_y)):
            for k, i in enumerate(base):
                data[i + rm.X] = float(nx[k])
                data[i + rm.Y] = float(ny_[k])
        self.coupling_solves += coupled
        self.coupling_coincident += coincident
        self.adhesion_solves += adhered
        for side in SIDES:
            for label, v in census[side].items():
                self.adhesion_census[side][label] += v


class AdhesionModel(AdhesionMixin, CouplingMixin, ViscosityModel):
    """CouplingModel with the adhesion band"""
