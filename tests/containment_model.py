"""CPU model of the relaxed step with yolk containment (egg_set_containment; DESIGN.md section 2.7, "Containment").  Test
helper, not collected.

ContainmentMixin sits on tests/adhesion_model.py's AdhesionMixin the way that sits on CouplingMixin: it holds `factor`
(0 = off) and `strength`, and its _couple() -- which the family calls once per sub-step, after the follow of both types
-- runs the coupling pass (with or without the adhesion band, or nothing) and then contains.  Containment ACTS in a
step exactly when factor > 0, both types have particles and the solver order is relaxed; it needs neither coupling nor
adhesion.

The summary of a batch's white, over its n white positions v[0 .. n) in the handle's particle order:

  wsum(v)   64 accumulators a[0 .. 63] start at +0.0; for k = l, l + 64, ... < n ascending: a[l] = a[l] + v[k]; then for
            d = 32, 16, 8, 4, 2, 1: a[l] = a[l] + a[l ^ d] for all l at once; the result is a[0]
  cx, cy    wsum(x) / n, wsum(y) / n
  q[k]      (x[k] - cx) (x[k] - cx) + (y[k] - cy) (y[k] - cy)
  rho, L    sqrt(wsum(q) / n), factor rho; n == 0: L = +inf (defined, not reachable: a batch always has white particles)

The projection of a yolk particle of the same batch:

  dx = x - cx, dy = y - cy, d = sqrt(dx dx + dy dy)
  d > L (false for a NaN): keep = L + (1 - strength) (d - L), s = keep / d, x = cx + dx s, y = cy + dy s; one hit

There is no mass test and the white is never moved.  numpy float64 element-wise in exactly this order; written from the
definition, not from the kernel.

`containment_hits` counts the projections over all steps.  The census labels every (yolk particle, sub-step) from its
inputs alone, in `containment_census[label]`:

  inside     d < L (or a comparison with a NaN): nothing
  edge       d == L exactly: nothing
  hit_rigid  d > L with strength == 1: lands on the disc's edge
  hit_soft   d > L with strength < 1
  no_white   the batch has no white particle: L = +inf (the rule defines it; add and import_batch refuse such a batch, so no
             scene reaches it)

`containment_rule` (None in the model) names one deliberately WRONG rule for tests/test_containment_model.py."""
import numpy as np

from adhesion_model import AdhesionMixin
from coupling_model import CouplingMixin
from relaxed_model import rm
from viscosity_model import ViscosityModel

LABELS = ("inside", "edge", "hit_rigid", "hit_soft", "no_white")
RULES = ("ge", "sequential", "both_types", "mass_weighted", "max_distance", "before_coupling", "keep_times_strength")
_LANES = np.arange(64)


def wsum(v):
    """the order-defined sum of the rule"""
    v = np.asarray(v, dtype=np.float64)
    a = np.zeros(64)
    for k0 in range(0, len(v), 64):
        row = v[k0:k0 + 64]
        a[:len(row)] = a[:len(row)] + row
    for d in (32, 16, 8, 4, 2, 1):
        a = a + a[_LANES ^ d]
    return a[0]


def sequential_sum(v):
    """v[0] + v[1] + ... from +0.0: what the rule is NOT"""
    acc = np.float64(0.0)
    for t in np.asarray(v, dtype=np.float64):
        acc = acc + t
    return acc


def summary(x, y, factor, total=wsum):
    """(cx, cy, L) of one batch's white positions"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = len(x)
    if n == 0:
        return np.float64("nan"), np.float64("nan"), np.float64("inf")
    nd = np.float64(n)
    with np.errstate(invalid="ignore", over="ignore"):
        cx = total(x) / nd
        cy = total(y) / nd
        q = (x - cx) * (x - cx) + (y - cy) * (y - cy)
        rho = np.sqrt(total(q) / nd)
        return cx, cy, np.float64(factor) * rho


def project(x, y, cx, cy, L, strength, ge=False, keep_times_strength=False):
    """the projection of the yolk positions (x, y) of one batch: (new x, new y, hit mask, d)"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        dx = x - cx
        dy = y - cy
        d = np.sqrt(dx * dx + dy * dy)
        hit = d >= L if ge else d > L
        keep = L * np.float64(strength) if keep_times_strength else L + (np.float64(1.0) - np.float64(strength)) * (d - L)
        s = keep / d
        nx = np.where(hit, cx + dx * s, x)
        ny = np.where(hit, cy + dy * s, y)
    return nx, ny, hit, d


class ContainmentMixin:
    """containment on top of the coupling / adhesion pass (set_containment; the values may change between steps)"""

    containment_factor = 0.0
    containment_strength = 1.0
    containment_hits = 0
    containment_rule = None  # (tests only: one of RULES)

    def set_containment(self, factor=0.0, strength=1.0):
        assert 0.0 <= factor < float("inf") and 0.0 <= strength <= 1.0
        self.containment_factor, self.containment_strength = float(factor), float(strength)

    def containment_acts(self):
        nw, ny = self._total_n_white_particles, self._total_n_yolk_particles
        return bool(self.relaxed and self.containment_factor > 0.0 and nw and ny)

    def _couple(self):
        if self.containment_rule == "before_coupling":
            self._contain()
            super()._couple()
            return
        super()._couple()
        self._contain()

    def _contain(self):
        if not self.containment_acts():
            return
        if not hasattr(self, "containment_census"):
            self.containment_census = dict.fromkeys(LABELS, 0)
        rule = self.containment_rule
        cols = {}
        for name, data, n in (("white", self._white_data, self._total_n_white_particles),
                              ("yolk", self._yolk_data, self._total_n_yolk_particles)):
            base = [rm.offset(p) for p in range(1, n + 1)]
            cols[name] = (data, base) + tuple(np.array([data[i + off] for i in base], dtype=np.float64)
                                              for off in (rm.X, rm.Y, rm.MASS, rm.BATCH_ID))
        _, _, wx, wy, wm, wb = cols["white"]
        ydata, ybase, yx, yy, ym, yb = cols["yolk"]
        total = sequential_sum if rule == "sequential" else wsum
        for b in np.unique(yb):  # (batches are independent: any order)
            mine = np.flatnonzero(yb == b)  # ascending: the handle's particle order
            w = np.flatnonzero(wb == b)
            if rule == "both_types":
                cx, cy, L = summary(np.concatenate((wx[w], yx[mine])), np.concatenate((wy[w], yy[mine])),
                                    self.containment_factor, total)
            else:
                cx, cy, L = summary(wx[w], wy[w], self.containment_factor, total)
            if rule == "mass_weighted" and len(w):
                cx, cy = total(wx[w] * wm[w]) / total(wm[w]), total(wy[w] * wm[w]) / total(wm[w])
            if rule == "max_distance" and len(w):
                L = np.float64(self.containment_factor) * np.sqrt(np.max((wx[w] - cx) * (wx[w] - cx) + (wy[w] - cy) * (wy[w] - cy)))
            nx, ny, hit, d = project(yx[mine], yy[mine], cx, cy, L, self.containment_strength, rule == "ge",
                                     rule == "keep_times_strength")
            for k, p in enumerate(mine):
                if hit[k]:
                    ydata[ybase[p] + rm.X] = float(nx[k])
                    ydata[ybase[p] + rm.Y] = float(ny[k])
            self.containment_hits += int(np.count_nonzero(hit))
            rigid = self.containment_strength == 1.0
            for label, lanes in (("no_white", np.full(len(mine), len(w) == 0)),
                                 ("edge", (d == L) & (len(w) > 0)),
                                 ("hit_rigid", hit & rigid), ("hit_soft", hit & (not rigid)),
                                 ("inside", ~hit & ~(d == L) & (len(w) > 0))):
                self.containment_census[label] += int(np.count_nonzero(lanes))


class ContainmentModel(ContainmentMixin, AdhesionMixin, CouplingMixin, ViscosityModel):
    """AdhesionModel with containment"""
