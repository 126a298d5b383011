"""Which branch of steps 5b / 5c every particle takes ("Colliders", "Collider surfaces", "Walls").  Test
helper, not collected.

CensusModel is tests/wall_model.py's WallModel that, besides, records after every application of steps 5b / 5c, per
particle type and per collider index, which particles took which labelled branch.  The labels come from classify(), which
works from the inputs of one application alone -- the position (x, y) the collider meets, the radius r, the start of the
sub-step prev, the collider, its surface, the sub-step h -- with the formulas of the three model docstrings, written out
once more here and not taken from the kernel.  Recording changes nothing: CensusModel's pass is WallModel's with
the recording walk in front of the same wall_model.project() call, the state it reaches is WallModel's bit for bit
(tests/test_collider_census.py asserts it), and classify()'s own projection is asserted against project()'s at every
application.

Labels of step 5b (a lane may carry several: `centre`, `clamped`, `on_it` and the wall's flags come on top of a hit):

  half_plane   hit, miss
  disc         hit, centre (a hit with d2 == 0), miss
  container    hit, clamped (a hit with R - r < 0, so m = 0), miss
  segment, and a wall that does not catch
               hit_inside (a hit with 0 <= t <= 1 before the clamp), hit_start (t < 0), hit_end (t > 1), point (a hit with
               l2 == 0, instead of the three), on_it (a hit with d2 == 0, on top of them), miss
  wall         catch_pos (caught, a0 > 0), catch_neg (caught, a0 < 0), catch_inside_r (caught with d2 < m m),
               catch_on_line (caught with a1 == 0), no_side (a0 == 0), round_start (opp and tc < 0), round_end (opp and
               tc > 1)
  any kind     masked (the collider's mask does not cover the type: nothing else is recorded)

Labels of step 5c, over the lanes the collider has just moved: smooth (its friction is not > 0), no_tangent (!(tl2 > 0)),
stick, slide; after a catch the four are caught_smooth, caught_no_tangent, caught_stick, caught_slide.  The collider index
tells the kind.

Out of scope: NaN positions (a NaN cell fails the step before step 5b matters) and the force step.  The pair loop has a
census of its own: tests/pair_census.py, tests/test_pair_census.py, tests/test_gpu_pair_edges.py."""
import numpy as np

import surface_model as sm
import wall_model as wm
from cohesion_model import CohesiveModel
from relaxed_model import DIRS, rm
from wall_model import WallModel

SEGMENT_LABELS = ("hit_inside", "hit_start", "hit_end", "on_it", "point", "miss")
WALL_LABELS = ("catch_pos", "catch_neg", "catch_inside_r", "catch_on_line", "no_side", "round_start", "round_end")
GRIP_LABELS = ("stick", "slide", "no_tangent", "smooth")
LABELS = {
    "half_plane": ("hit", "miss"),
    "disc": ("hit", "centre", "miss"),
    "container": ("hit", "clamped", "miss"),
    "segment": SEGMENT_LABELS,
    "wall": SEGMENT_LABELS + WALL_LABELS,
}


def classify(x, y, r, px, py, h, collider, surface, type_bit, idx):
    """one collider (as wall_model.normalise() returns it) with its surface (as surface_model.normalise() does) over the
    lanes, element-wise.  Returns (labels, x, y): label -> boolean lanes, and the position steps 5b and 5c leave."""
    kind, p0, p1, p2, p3, mask = collider
    mu, svx, svy = surface
    n = len(x)
    none = np.zeros(n, dtype=bool)
    if not mask & type_bit:
        return {"masked": ~none}, x, y
    caught = none
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if kind == "half_plane":
            s = (p0 * x + p1 * y) - (p2 + r)
            hit = s < 0.0
            lab = {"hit": hit, "miss": ~hit}
            qx, qy = x - s * p0, y - s * p1
            nx, ny, pen = p0 + 0.0 * x, p1 + 0.0 * x, -s
        elif kind == "disc":
            dx, dy = x - p0, y - p1
            d2 = dx * dx + dy * dy
            m = p2 + r
            hit = d2 < m * m
            d = np.sqrt(d2)
            nx = np.where(d2 == 0.0, DIRS[idx & 7, 0], dx / d)
            ny = np.where(d2 == 0.0, DIRS[idx & 7, 1], dy / d)
            lab = {"hit": hit, "centre": hit & (d2 == 0.0), "miss": ~hit}
            qx, qy, pen = p0 + nx * m, p1 + ny * m, m - d
        elif kind == "container":
            m = p2 - r
            low = m < 0.0
            m = np.where(low, 0.0, m)
            dx, dy = x - p0, y - p1
            d2 = dx * dx + dy * dy
            hit = d2 > m * m
            d = np.sqrt(d2)
            nx, ny, pen = dx / d, dy / d, d - m
            lab = {"hit": hit, "clamped": hit & low, "miss": ~hit}
            qx, qy = p0 + nx * m, p1 + ny * m
        else:  # segment and wall
            ex, ey = p2 - p0, p3 - p1
            l2 = ex * ex + ey * ey
            t0 = np.zeros(n) if l2 == 0.0 else ((x - p0) * ex + (y - p1) * ey) / l2
            t = np.where(t0 < 0.0, 0.0, t0)
            t = np.where(t > 1.0, 1.0, t)
            cx, cy = p0 + t * ex, p1 + t * ey
            dx, dy = x - cx, y - cy
            d2 = dx * dx + dy * dy
            m = 0.0 + r
            d = np.sqrt(d2)
            lab = {}
            if kind == "wall":
                a0 = ex * (py - p1) - ey * (px - p0)
                a1 = ex * (y - p1) - ey * (x - p0)
                opp = ((a0 > 0.0) & (a1 <= 0.0)) | ((a0 < 0.0) & (a1 >= 0.0))
                u = a0 / (a0 - a1)
                hx, hy = px + u * (x - px), py + u * (y - py)
                tc = ((hx - p0) * ex + (hy - p1) * ey) / np.float64(l2)
                caught = opp & (tc >= 0.0) & (tc <= 1.0)
                ln = np.sqrt(np.float64(l2))
                wx = np.where(a0 > 0.0, (-ey) / ln, ey / ln)
                wy = np.where(a0 > 0.0, ex / ln, (-ex) / ln)
                lab.update(catch_pos=caught & (a0 > 0.0), catch_neg=caught & (a0 < 0.0), catch_inside_r=caught & (d2 < m * m),
                           catch_on_line=caught & (a1 == 0.0), no_side=a0 == 0.0, round_start=opp & (tc < 0.0),
                           round_end=opp & (tc > 1.0))
            seg = ~caught & (d2 < m * m)
            some = none if l2 == 0.0 else seg
            lab.update(hit_inside=some & (t0 >= 0.0) & (t0 <= 1.0), hit_start=some & (t0 < 0.0), hit_end=some & (t0 > 1.0),
                       on_it=seg & (d2 == 0.0), point=seg if l2 == 0.0 else none, miss=~caught & ~seg)
            nx = np.where(d2 == 0.0, DIRS[idx & 7, 0], dx / d)
            ny = np.where(d2 == 0.0, DIRS[idx & 7, 1], dy / d)
            pen = m - d
            if kind == "wall":
                nx, ny, pen = np.where(caught, wx, nx), np.where(caught, wy, ny), np.where(caught, m + d, pen)
            hit = caught | seg
            qx, qy = cx + nx * m, cy + ny * m
        x, y = np.where(hit, qx, x), np.where(hit, qy, y)
        # step 5c
        if not mu > 0.0:
            took = {"smooth": hit}
        else:
            gx = (x - px) - h * svx
            gy = (y - py) - h * svy
            dn = gx * nx + gy * ny
            tx, ty = gx - dn * nx, gy - dn * ny
            tl2 = tx * tx + ty * ty
            on = hit & (tl2 > 0.0)
            tl = np.sqrt(tl2)
            lim = mu * pen
            stick = on & (tl <= lim)
            f = lim / tl
            took = {"no_tangent": hit & ~on, "stick": stick, "slide": on & ~stick}
            x = np.where(stick, x - tx, np.where(on, x - tx * f, x))
            y = np.where(stick, y - ty, np.where(on, y - ty * f, y))
        for name, lanes in took.items():
            lab[name] = lanes & ~caught
            if kind == "wall":
                lab["caught_" + name] = lanes & caught
    return lab, x, y


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


class CensusModel(WallModel):
    """WallModel that records the labels.  census[type][(collider index, label)] is an array over the particles of the
    type: how often each took that branch, over all passes of all steps; both_caught[type] counts the passes in which
    one particle was caught by two or more walls of the list."""

    def __init__(self, white_config=None, yolk_config=None, relaxed=True, relaxation=None, cohesion=False):
        self.census = [{}, {}]
        self.both_caught = [0, 0]
        super().__init__(white_config, yolk_config, relaxed, relaxation=relaxation, cohesion=cohesion)

    def _solve_collision(self, particles, n_particles, *args, **kwargs):
        # WallModel._solve_collision, with the walk through the list in front of its project()
        out = CohesiveModel._solve_collision(self, particles, n_particles, *args, **kwargs)
        if self.relaxed and self.colliders and n_particles:
            which = 0 if particles is self._white_data else 1
            base = [rm.offset(p) for p in range(1, n_particles + 1)]

            def col(off):
                return [particles[i + off] for i in base]

            self._record(which, *(np.array(col(off), dtype=np.float64) for off in (rm.X, rm.Y, rm.RADIUS, rm.PX, rm.PY)))
            x, y, hits, grips, sticks, catches, ever = wm.project(col(rm.X), col(rm.Y), col(rm.RADIUS), col(rm.PX), col(rm.PY),
                                                                  self._sub_delta, self.colliders, self.surfaces, 1 << which)
            for k, i in enumerate(base):
                particles[i + rm.X] = float(x[k])
                particles[i + rm.Y] = float(y[k])
            self.collider_hits[which] += hits
            self.collider_grips[which] += grips
            self.grip_sticks[which] += sticks
            self.wall_catches[which] += catches
            self.caught_ever[which].update(int(k) for k in np.flatnonzero(ever))
        return out

    def _record(self, which, x, y, r, px, py):
        """the labels of one pass: the list collider by collider, each on what wall_model.project() made of the one before"""
        n = len(x)
        idx = np.arange(n)
        surfaces = self.surfaces if self.surfaces else [sm.DEFAULT] * len(self.colliders)
        catches = np.zeros(n, dtype=np.int64)
        for c, (collider, surface) in enumerate(zip(self.colliders, surfaces)):
            lab, cx, cy = classify(x, y, r, px, py, self._sub_delta, collider, surface, 1 << which, idx)
            x, y = wm.project(x, y, r, px, py, self._sub_delta, [collider], [surface], 1 << which, idx)[:2]
            assert _same(cx, x) and _same(cy, y), "classify() and wall_model.project() disagree on collider %d" % c
            for name, lanes in lab.items():
                if lanes.any():
                    have = self.census[which].setdefault((c, name), np.zeros(n, dtype=np.int64))
                    assert len(have) == n, "the census does not follow add / remove once it has begun"
                    have += lanes
            catches += lab.get("catch_pos", 0) | lab.get("catch_neg", 0)
        self.both_caught[which] += int(np.count_nonzero(catches >= 2))

    # ---- readout
    def count(self, which, label, collider=None, batch=None):
        """how often particles of type `which` (of batch `batch`, of all if None) took `label` (at collider index `collider`,
        at any if None)"""
        total, ids = 0, None
        for (c, name), lanes in self.census[which].items():
            if name == label and collider in (None, c):
                if batch is not None:
                    if ids is None:
                        ids = self._batch_ids(which, len(lanes))
                    lanes = lanes[ids == batch]
                total += int(lanes.sum())
        return total

    def _batch_ids(self, which, n):
        """the batch of every particle of the type, looked up once per particle count (the census refuses add / remove)"""
        have = self.__dict__.setdefault("_ids", {})
        if (which, n) not in have:
            data = self._white_data if which == 0 else self._yolk_data
            have[(which, n)] = np.array([data[rm.offset(p) + rm.BATCH_ID] for p in range(1, n + 1)])
        return have[(which, n)]

    def counts(self, which, collider=None, batch=None):
        """{label: count} of the labels with a count > 0"""
        names = sorted({name for (c, name) in self.census[which] if collider in (None, c)})
        out = {name: self.count(which, name, collider, batch) for name in names}
        return {name: v for name, v in out.items() if v > 0}

    def labels_of(self, which, particle, collider=None):
        """the labels 0-based particle `particle` of the type took at least once"""
        return {name for (c, name), lanes in self.census[which].items() if collider in (None, c) and lanes[particle] > 0}
