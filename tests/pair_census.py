"""Which branch of the pair arithmetic every pair evaluation of the relaxed step takes (the relaxed
pass, "Cohesion", "Coupling").  Test helper, not collected.

PairCensusModel is the family's most derived model -- tests/coupling_model.py's CouplingMixin on tests/wall_model.py's
WallModel, as in tests/test_gpu_coupling.py -- that, besides, records for every pair evaluation of every collision pass and
of every coupling pass which labelled branch it took, per SITE:

  collision:white, collision:yolk      the collision branch of a type's relaxed pass
  cohesion:white, cohesion:yolk        its cohesion branch (effective cohesion on)
  couple_white_side, couple_yolk_side  the coupling pass as the white particle, as the yolk particle evaluates it

An evaluation is one particle i looking at one candidate j, so a pair of one type is evaluated twice in a pass (once from
either side) and a cross pair once per side.  The labels come from classify(), which works from the inputs of one evaluation
alone -- the two positions, inverse masses and radii, the index difference, overlap (or the coupling factor), the
compliance, eps, and for cohesion whether the two share a batch, the reach factor and the cohesion compliance -- with the
formulas of the docstrings of relaxed_model.py, cohesion_model.py and coupling_model.py, written out once more here and
not taken from the kernel.  Recording changes no bit: the census is taken from the start-of-pass state in front of the very
call the un-instrumented model makes (tests/test_pair_census.py asserts the states equal), classify()'s own shares, counted
and fired flags are asserted equal to relaxed_model.pair_shares' at every evaluation, and its totals are asserted against
the pass's own counters (pairs counted, pairs that cohered, coupling solves and coincident ones).

Labels of a pair evaluation (one may carry several: `touching`, `coincident_k`, `tiny` and the clamp labels come on top of
`fires` or `coheres`):

  skipped        wsum < eps: not counted in pair_solves, nothing else is recorded
  apart          counted, nothing fires
  fires          the collision (coupling) correction runs: d2 <= md^2, md = overlap (ra + rb)
  touching       fires with d2 == md^2 exactly
  coincident_k   fires with d2 == 0: the normal is DIRS[k], k = (b - a) & 7, k = 0..7
  tiny           fires with 0 < current < eps: zero normal, zero share, but n still counts the pair
  coheres        the cohesion branch runs: no collision, same batch, d2 <= reach^2, reach = factor (ra + rb)
  reach_edge     coheres with d2 == reach^2 exactly
  other_batch    within reach, no collision, the batch differs: nothing fires (`apart` at the collision site as well)
  clamp_hi       correction > |violation| (collision and coupling: the violation is <= 0, the correction >= 0)
  clamp_lo       correction < -|violation| (cohesion only: its violation is positive)
  unclamped      fires or coheres, neither clamp
  dead           fires or coheres with divisor < eps: zero shares

and of a particle, per pass, at the collision site of its type or at its side of the coupling pass: `alone` (n == 0: the
position is copied bit for bit) and `averaged_n` for n >= 2 fired pairs.

`dead` cannot occur in a step: a pair that fires has wsum >= eps, and the compliance (1 - strength) / h^2 of a strength
clamped to [0, 1] is >= 0, so divisor = wsum + compliance >= wsum >= eps.  (tests/test_pair_census.py checks the label with
a negative compliance on classify() and pair_shares alone.)

Out of scope: NaN positions (they fail the step at the insert kernel), the exact-order solver (tests/exact_census.py has its census),
viscosity's own pair weights and the force step."""
import numpy as np

from coupling_model import CouplingMixin
from relaxed_model import DIRS, pair_shares, rm
from wall_model import WallModel

WHITE, YOLK = 0, 1
TYPE = ("white", "yolk")
SITES = ("collision:white", "collision:yolk", "cohesion:white", "cohesion:yolk", "couple_white_side", "couple_yolk_side")
COINCIDENT = tuple("coincident_%d" % k for k in range(8))
COLLISION_LABELS = ("skipped", "apart", "fires", "touching") + COINCIDENT + ("tiny", "clamp_hi", "unclamped")
COHESION_LABELS = ("coheres", "reach_edge", "other_batch", "clamp_lo", "unclamped")
# label -> the sites where it can occur in a step (`dead` nowhere, see above; clamp_lo at a collision or clamp_hi at a
# cohesion would need a violation of the other sign; a cohering pair lies beyond md > 0, so it is neither coincident nor tiny)
REACHABLE = {lab: tuple(s for s in SITES if not s.startswith("cohesion")) for lab in COLLISION_LABELS}
REACHABLE.update({lab: ("cohesion:white", "cohesion:yolk") for lab in COHESION_LABELS if lab != "unclamped"})
REACHABLE["unclamped"] = SITES


def candidates(cx, cy, ocx, ocy, same):
    """every evaluation of one pass as index arrays (i, j): i over the particles with cells (cx, cy), j over the particles
    with cells (ocx, ocy) that lie in i's 3x3 cells; `same`: the two sets are one, and i never meets itself.  (The order
    of the visits does not matter to the label of a visit.)"""
    n, m = len(cx), len(ocx)
    order = np.lexsort((np.arange(m), ocy, ocx))
    skey = ocx[order] * (1 << 32) + (ocy[order] + (1 << 31))  # ascending: the cells sorted by (x, y)
    out_i, out_j = [], []
    for ox in (-1, 0, 1):
        for oy in (-1, 0, 1):
            qx, qy = cx + ox, cy + oy
            # the run of (qx, qy) among the sorted cells
            key = qx * (1 << 32) + (qy + (1 << 31))
            st = np.searchsorted(skey, key, side="left")
            cnt = np.searchsorted(skey, key, side="right") - st
            i = np.repeat(np.arange(n), cnt)
            within = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            j = order[np.repeat(st, cnt) + within]
            if same:
                keep = i != j
                i, j = i[keep], j[keep]
            out_i.append(i)
            out_j.append(j)
    return np.concatenate(out_i), np.concatenate(out_j)


def classify(ax, ay, bx, by, wa, wb, ra, rb, da, overlap, compliance, eps=rm.EPS, cohesion=None):
    """pairs (a, b) element-wise.  cohesion: None, or (the two share a batch, the reach factor, the cohesion compliance).
    Returns (labels, shares, counted, collides, coheres): labels maps (site kind, label) -> boolean lanes with site kind
    "collision" or "cohesion"; shares = (cax, cay, cbx, cby) of the branch that runs."""
    ax, ay, bx, by, wa, wb, ra, rb = (np.asarray(v, dtype=np.float64) for v in (ax, ay, bx, by, wa, wb, ra, rb))
    da = np.asarray(da, dtype=np.int64)
    none = np.zeros(ax.shape, dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        wsum = wa + wb
        skipped = wsum < eps
        counted = ~skipped
        dx, dy = bx - ax, by - ay
        d2 = dx * dx + dy * dy
        md = overlap * (ra + rb)
        collides = counted & (d2 <= md * md)
        coheres = other = edge = none
        cc = compliance
        if cohesion is not None:
            same, factor, cc = cohesion
            reach = factor * (ra + rb)
            within = counted & ~collides & (d2 <= reach * reach)
            coheres, other = within & same, within & ~same
            edge = coheres & (d2 == reach * reach)
        runs = collides | coheres
        divisor = wsum + np.where(coheres, cc, compliance)
        dead = runs & (divisor < eps)
        current = np.sqrt(d2)
        violation = current - md
        coincident = d2 == 0.0
        tiny = ~coincident & (current < eps)
        k = da & 7
        nx = np.where(coincident, DIRS[k, 0], np.where(tiny, 0.0, dx / current))
        ny = np.where(coincident, DIRS[k, 1], np.where(tiny, 0.0, dy / current))
        raw = -violation / divisor
        limit = np.abs(violation)
        lo, hi = raw < -limit, raw > limit
        correction = np.where(lo, -limit, np.where(hi, limit, raw))
        shares = tuple(np.where(dead, 0.0, v) for v in (-nx * correction * wa, -ny * correction * wa,
                                                         nx * correction * wb, ny * correction * wb))
    lab = {("collision", "skipped"): skipped, ("collision", "apart"): counted & ~runs, ("collision", "fires"): collides,
           ("collision", "touching"): collides & (d2 == md * md), ("collision", "tiny"): collides & tiny,
           ("collision", "clamp_hi"): collides & ~dead & hi, ("collision", "clamp_lo"): collides & ~dead & lo,
           ("collision", "unclamped"): collides & ~dead & ~hi & ~lo, ("collision", "dead"): collides & dead,
           ("cohesion", "coheres"): coheres, ("cohesion", "reach_edge"): edge, ("cohesion", "other_batch"): other,
           ("cohesion", "clamp_hi"): coheres & ~dead & hi, ("cohesion", "clamp_lo"): coheres & ~dead & lo,
           ("cohesion", "unclamped"): coheres & ~dead & ~hi & ~lo, ("cohesion", "dead"): coheres & dead}
    for q in range(8):
        lab[("collision", "coincident_%d" % q)] = collides & coincident & (k == q)
    return lab, shares, counted, collides, coheres


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _against_pair_shares(args, compliance, eps, shares, counted, collides, lanes):
    """classify()'s shares over `lanes` and its flags are relaxed_model.pair_shares' (called with this compliance)"""
    ref = pair_shares(*args, compliance, eps)
    assert _same(ref[4], counted) and _same(ref[5], collides), "classify() and pair_shares() disagree on a flag"
    for mine, theirs in zip(shares, ref[:4]):
        assert _same(mine[lanes], theirs[lanes]), "classify() and pair_shares() disagree on a share"


class PairCensusModel(CouplingMixin, WallModel):
    """the model with the census.  census[site][label] is an array over the particles of the site's type (the side's type
    for the coupling sites): how often each, as the evaluating particle i, took that branch, over all passes of all steps.
    starts[site] holds the (x, y) every pass of the site started from, in order (the hand cases assert that the first is
    where the particles were put)."""

    def __init__(self, white_config=None, yolk_config=None, relaxed=True, relaxation=None, cohesion=False):
        self.census = {}
        self.starts = {}
        self.evaluations = 0
        self._totals = {}
        super().__init__(white_config, yolk_config, relaxed, relaxation=relaxation, cohesion=cohesion)

    # ---- recording
    def _add(self, site, label, lanes_of_i, n):
        have = self.census.setdefault(site, {}).get(label)
        if have is None or len(have) != n:  # (add / remove: the per-particle counts begin again, the totals go on)
            if have is not None:
                self._totals[(site, label)] = self._totals.get((site, label), 0) + int(have.sum())
            have = self.census[site][label] = np.zeros(n, dtype=np.int64)
        have += lanes_of_i

    def _per_particle(self, site, n_fired, n):
        self._add(site, "alone", n_fired == 0, n)
        for q in np.unique(n_fired[n_fired >= 2]):
            self._add(site, "averaged_%d" % q, n_fired == q, n)

    def _solve_collision(self, particles, n_particles, spatial_hash, collided, collision_overlap_factor, collision_compliance,
                         cohesion_interaction_distance_factor, cohesion_compliance, max_n_collisions, visit_log=None):
        which = WHITE if particles is self._white_data else YOLK
        before = self.cohesion_solves
        want = None
        if self.relaxed and n_particles:
            want = self._record_pass(which, particles, n_particles, collision_overlap_factor, collision_compliance,
                                     cohesion_interaction_distance_factor, cohesion_compliance)
        out = super()._solve_collision(particles, n_particles, spatial_hash, collided, collision_overlap_factor,
                                       collision_compliance, cohesion_interaction_distance_factor, cohesion_compliance,
                                       max_n_collisions, visit_log)
        if want is not None:
            pairs, cohered, alone, x, y = want
            assert out == (pairs, False) and self.cohesion_solves - before == cohered, "the census and the pass disagree on a counter"
            if not self.colliders:  # n == 0: copied bit for bit
                base = [rm.offset(p) for p in np.flatnonzero(alone) + 1]
                assert [particles[i + rm.X] for i in base] == list(x[alone]) and [particles[i + rm.Y] for i in base] == list(y[alone])
        return out

    def _record_pass(self, which, particles, n, overlap, compliance, factor, cohesion_compliance):
        base = [rm.offset(p) for p in range(1, n + 1)]
        x, y, w, r = (np.array([particles[i + off] for i in base], dtype=np.float64) for off in (rm.X, rm.Y, rm.INV_MASS, rm.RADIUS))
        cx, cy, batch = (np.array([particles[i + off] for i in base], dtype=np.int64) for off in (rm.CELL_X, rm.CELL_Y, rm.BATCH_ID))
        self.starts.setdefault("collision:" + TYPE[which], []).append((x, y))
        i, j = candidates(cx, cy, cx, cy, True)
        a, b = np.minimum(i, j), np.maximum(i, j)
        args = (x[a], y[a], x[b], y[b], w[a], w[b], r[a], r[b], b - a, overlap)
        coh = (batch[a] == batch[b], factor, cohesion_compliance) if self.cohesion else None
        lab, shares, counted, collides, coheres = classify(*args, compliance, cohesion=coh)
        _against_pair_shares(args, compliance, rm.EPS, shares, counted, collides, collides)
        if coh is not None:
            _against_pair_shares(args, cohesion_compliance, rm.EPS, shares, counted, collides, coheres)
        self.evaluations += len(i)
        for (kind, name), lanes in lab.items():
            if lanes.any():
                self._add("%s:%s" % (kind, TYPE[which]), name, np.bincount(i[lanes], minlength=n), n)
        n_fired = np.bincount(i[collides | coheres], minlength=n)
        self._per_particle("collision:" + TYPE[which], n_fired, n)
        first = i < j
        return int(np.count_nonzero(counted & first)), int(np.count_nonzero(coheres & first)), n_fired == 0, x, y

    def _couple(self):
        nw, ny = self._total_n_white_particles, self._total_n_yolk_particles
        on = bool(self.relaxed and self.coupling_factor > 0.0 and nw and ny)
        before = (self.coupling_solves, self.coupling_coincident)
        if on:
            want = self._record_coupling(nw, ny)
        super()._couple()
        if on:
            assert (self.coupling_solves - before[0], self.coupling_coincident - before[1]) == want, "the census and the coupling pass disagree"

    def coupling_cell(self):
        """H of the coupling pass"""
        return max(1.0, self.coupling_factor * (self._white_config["max_radius"] + self._yolk_config["max_radius"]))

    def _record_coupling(self, nw, ny):
        sides = []
        for data, n in ((self._white_data, nw), (self._yolk_data, ny)):
            base = [rm.offset(p) for p in range(1, n + 1)]
            sides.append(tuple(np.array([data[i + off] for i in base], dtype=np.float64) for off in (rm.X, rm.Y, rm.INV_MASS, rm.RADIUS)))
        H = self.coupling_cell()
        compliance = (1.0 - self.coupling_strength) / (self._coupling_sub_delta * self._coupling_sub_delta)
        eps = self._white_config.get("eps", rm.EPS)  # the white config's, both sides
        with np.errstate(invalid="ignore"):
            cells = [(np.floor(s[0] / H).astype(np.int64), np.floor(s[1] / H).astype(np.int64)) for s in sides]
        (wx, wy, ww, wr), (yx, yy, yw, yr) = sides
        solves = coincident = 0
        for own in (WHITE, YOLK):
            site = "couple_%s_side" % TYPE[own]
            self.starts.setdefault(site, []).append(sides[own][:2])
            i, j = candidates(*cells[own], *cells[1 - own], False)
            a, b = (i, j) if own == WHITE else (j, i)  # a the white particle, b the yolk one, whichever side evaluates
            args = (wx[a], wy[a], yx[b], yy[b], ww[a], yw[b], wr[a], yr[b], b - a, self.coupling_factor)
            lab, shares, counted, collides, _ = classify(*args, compliance, eps)
            _against_pair_shares(args, compliance, eps, shares, counted, collides, collides)
            self.evaluations += len(i)
            n = len(sides[own][0])
            for (kind, name), lanes in lab.items():
                if lanes.any():
                    assert kind == "collision"
                    self._add(site, name, np.bincount(i[lanes], minlength=n), n)
            self._per_particle(site, np.bincount(i[collides], minlength=n), n)
            if own == WHITE:
                solves = int(np.count_nonzero(collides))
                coincident = sum(int(np.count_nonzero(lab[("collision", name)])) for name in COINCIDENT)
            else:
                assert int(np.count_nonzero(collides)) == solves  # both sides evaluate one expression per pair
        return solves, coincident

    # ---- readout
    def count(self, site, label):
        """how often an evaluation at `site` took `label`"""
        have = self.census.get(site, {}).get(label)
        return self._totals.get((site, label), 0) + (0 if have is None else int(have.sum()))

    def counts(self, site):
        """{label: count} of the labels with a count > 0"""
        out = {label: self.count(site, label) for label in self.census.get(site, {})}
        return {label: v for label, v in out.items() if v > 0}

    def labels(self, site):
        return set(self.counts(site))

    def labels_of(self, site, particle):
        """the labels 0-based particle `particle` of the site's type took at least once, as the evaluating particle"""
        return {label for label, lanes in self.census.get(site, {}).items() if particle < len(lanes) and lanes[particle] > 0}
