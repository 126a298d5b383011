"""Which branch of the pair projection every pair evaluation of the EXACT-order step takes (oracle/reference_model.py's
ReferenceModel; the device side is csrc/eggsim_tile.h: project_pair<CACHED>, project_pair_predicated and
project_pair_reference, and the guards that choose between the hand-expanded and the operator arithmetic).  Test helper, not
collected.  tests/pair_census.py is the same thing for the relaxed solver.

ExactCensusModel restates the model's collision loop (L:1548-1666) and its follow constraint (L:1435-1471) with one
addition: in front of every evaluation it calls classify() on the inputs of that evaluation alone -- the two positions,
inverse masses and radii, whether the two share a batch, overlap, compliance, eps -- and counts the labels per SITE
(collision:white, collision:yolk, follow:white, follow:yolk).  classify() is written from the reference's rules
(L:1514-1545, L:1596-1657, math.lua:53-60), not from the kernel.  Recording changes no bit: tests/test_exact_census.py
asserts the instrumented and the plain model's states equal bit for bit, and the loop asserts at every evaluation that
classify()'s `guarded` and `fires` are the branches it then takes.

Labels at collision:white and collision:yolk (one evaluation may carry several):

  guarded           wsum < eps: the pair is marked in `collided`, not counted, not projected (L:1601); nothing else is recorded
  apart             counted, d2 > md^2, md = overlap (ra + rb)
  fires             d2 <= md^2: the projection runs
  edge              fires with d2 == md^2 (violation 0 unless the root rounds)
  coincident_same   d2 == 0, one batch: the cohesion block's `+ 0.0` runs in front of the collision (L:1603-1630)
  coincident_other  d2 == 0, two batches
  below_eps         fires with 0 < current < eps: normalize() returns (0, 0) (math.lua:53-56)
  axis_x, axis_y    fires with dx == +-0 (dy == +-0) and current >= eps: the normal has a signed zero
  tiny_component    fires with 0 < |dx| < 2^-300 or 0 < |dy| < 2^-300 (subnormal differences near the origin)
  clamp_hi          fires, the correction exceeds |violation| and is clamped (L:1540-1542)
  unclamped         fires, not clamped (the violation is <= 0, so the lower clamp cannot bind)
  fast              fires and none of edge, coincident_*, below_eps, axis_*, tiny_component: the arithmetic the device expands by hand

Labels at follow:white and follow:yolk: rests (current < target), rests_at_edge (current == target exactly), pulled,
massless (inverse mass <= eps, L:1458).

Labels that cannot occur in a step of a scene with sane configs -- classify() names them, tests/test_exact_census.py
checks them on classify() alone:

  dead           fires with divisor < eps.  A pair that is not guarded has wsum >= eps, the compliance (1 - strength) / h^2 of
                 a strength clamped to [0, 1] is >= 0, so divisor = wsum + compliance >= eps.
  huge_divisor   divisor > 2^300.  compliance <= 1 / h^2 <= 1e16 (h >= eps, L:1723), so it needs an inverse mass beyond
                 2^299, a mass below 2^-299.
  huge_reach     md^2 > 2^600: a particle radius beyond 2^298.
  (the device sends all three to project_pair_reference by pair_needs_reference(); no scene here has such a config)

Out of scope: NaN positions and non-finite configs (the device fails the step), the relaxed solver (tests/pair_census.py).

What the existing device scenes reach: the census over each scene at reduced size, on the CPU, as
tests/test_exact_census.py test_what_the_existing_device_scenes_reach runs it (the same drivers: test_gpu_fuzz's drifting
batches with seeds 1-3, three batches of 20 to 40 + 8 particles, 6 steps; test_gpu_round2's mass tweaks on two overlapping
batches of 40 + 8, 4 steps, and its sub-eps scene without the default batch, 3 steps; config 3's four coincident batches of
40 + 8, 3 steps; every one at (S, C) = (2, 3)).  The labels are the same at both collision sites unless said:

  scene                   collision sites                                          follow sites
  fuzz 1, 2, 3            apart fires unclamped fast                               rests pulled (seed 1, white: rests_at_edge too)
  mass guard "mixed"      guarded apart fires unclamped fast                       rests pulled massless
  mass guard "all"        guarded                                                  massless
  sub-eps                 fires unclamped below_eps coincident_other               rests pulled
  config 3 coincident     apart fires unclamped fast; white: coincident_other      rests pulled
  reached by none of them: edge, axis_x, axis_y, tiny_component, clamp_hi, coincident_same (the test asserts the first five)

These are reduced scenes on the model, not the device runs themselves: a full-size random session may reach more.  What no
run can tell is whether it did -- that is what the hand table is for.
"""
import math

from oracle import reference_model as rm
from oracle.reference_model import ReferenceModel

WHITE, YOLK = 0, 1
TYPE = ("white", "yolk")
COLLISION_SITES = ("collision:white", "collision:yolk")
FOLLOW_SITES = ("follow:white", "follow:yolk")
COLLISION_LABELS = ("guarded", "apart", "fires", "edge", "coincident_same", "coincident_other", "below_eps", "axis_x", "axis_y",
                    "tiny_component", "clamp_hi", "unclamped", "fast")
FOLLOW_LABELS = ("rests", "rests_at_edge", "pulled", "massless")
UNREACHABLE = ("dead", "huge_divisor", "huge_reach")
ARITH_LO, ARITH_HI = 2.0 ** -300, 2.0 ** 300
RULES = ("edge_excluded", "eps_inclusive", "zero_sign_lost", "no_plus_zero", "guard_counts", "clamp_missing", "follow_edge_pulls")


def classify(ax, ay, bx, by, wa, wb, ra, rb, same_batch, overlap, compliance, eps=rm.EPS):
    """the labels of one evaluation of the collision loop, from its inputs alone"""
    if wa + wb < eps:
        return {"guarded"}
    out = set()
    dx, dy = bx - ax, by - ay
    d2 = dx * dx + dy * dy
    if d2 == 0.0:
        out.add("coincident_same" if same_batch else "coincident_other")
    md = overlap * (ra + rb)
    md2 = md * md
    if not d2 <= md2:
        out.add("apart")
        return out
    out.add("fires")
    if d2 == md2:
        out.add("edge")
    current = math.sqrt(d2)
    if 0.0 < current < eps:
        out.add("below_eps")
    if current >= eps:
        if dx == 0.0:
            out.add("axis_x")
        if dy == 0.0:
            out.add("axis_y")
    if 0.0 < abs(dx) < ARITH_LO or 0.0 < abs(dy) < ARITH_LO:
        out.add("tiny_component")
    divisor = (wa + wb) + compliance
    if divisor < eps:
        out.add("dead")
    else:
        violation = current - md
        out.add("clamp_hi" if -violation / divisor > abs(violation) else "unclamped")
    if divisor > ARITH_HI:
        out.add("huge_divisor")
    if md2 > 2.0 ** 600:
        out.add("huge_reach")
    if not out & {"edge", "coincident_same", "coincident_other", "below_eps", "axis_x", "axis_y", "tiny_component", "dead", "huge_divisor",
                  "huge_reach"}:
        out.add("fast")
    return out


def classify_follow(x, y, follow_x, follow_y, inverse_mass, batch_radius, eps=rm.EPS):
    if inverse_mass <= eps:
        return "massless"
    ddx, ddy = follow_x - x, follow_y - y
    current, target = math.sqrt(ddx * ddx + ddy * ddy), 2 * batch_radius
    return "pulled" if current > target else "rests_at_edge" if current == target else "rests"


class ExactCensusModel(ReferenceModel):
    """ReferenceModel with the census: census[site][label] counts evaluations over all passes of all steps; pair_solves sums
    the pairs every pass counted; cuts counts the passes the budget cut; first[site] lists (self, other, labels), 0-based, of
    the first pass of the site that evaluated anything.  rule: None, or one of RULES -- a deliberately wrong reading of the
    reference, for the test that the hand table would notice it."""

    def __init__(self, white_config=None, yolk_config=None, rule=None):
        assert rule is None or rule in RULES
        self.rule = rule
        self.census = {s: {} for s in COLLISION_SITES + FOLLOW_SITES}
        self.first = {}
        self.pair_solves = 0
        self.cuts = 0
        self.cut_on = []  # (site, self, other) of the pair a budget cut fell on
        super().__init__(white_config, yolk_config)

    def _count(self, site, labels):
        c = self.census[site]
        for lab in labels:
            c[lab] = c.get(lab, 0) + 1

    def labels(self, site):
        return set(self.census[site])

    def _which(self, particles):
        return WHITE if particles is self._white_data else YOLK

    # ---- L:1435-1471
    def _solve_follow_constraint(self, particles, n_particles, batch_id_to_radius, batch_id_to_follow_x, batch_id_to_follow_y, compliance):
        site = "follow:" + TYPE[self._which(particles)]
        eps = rm.EPS
        for particle_i in range(1, n_particles + 1):
            i = rm.offset(particle_i)
            batch_id = particles[i + rm.BATCH_ID]
            follow_x, follow_y = batch_id_to_follow_x[batch_id], batch_id_to_follow_y[batch_id]
            x, y = particles[i + rm.X], particles[i + rm.Y]
            inverse_mass = particles[i + rm.INV_MASS]
            label = classify_follow(x, y, follow_x, follow_y, inverse_mass, batch_id_to_radius[batch_id], eps)
            self._count(site, (label,))
            current_distance = rm.distance(x, y, follow_x, follow_y)
            target_distance = 2 * batch_id_to_radius[batch_id]
            beyond = current_distance >= target_distance if self.rule == "follow_edge_pulls" else current_distance > target_distance
            moves = inverse_mass > eps and beyond
            assert self.rule is not None or moves == (label == "pulled")
            if moves:
                dx, dy = rm.normalize(follow_x - x, follow_y - y)
                constraint_violation = current_distance - target_distance
                delta_lambda = constraint_violation / (inverse_mass + compliance)
                particles[i + rm.X] = particles[i + rm.X] + dx * delta_lambda * inverse_mass
                particles[i + rm.Y] = particles[i + rm.Y] + dy * delta_lambda * inverse_mass

    # ---- L:1514-1545 with math.lua:53-60
    def _project(self, ax, ay, bx, by, wa, wb, target_distance, compliance):
        dx, dy = bx - ax, by - ay
        current = rm.magnitude(dx, dy)
        below = current <= rm.EPS if self.rule == "eps_inclusive" else current < rm.EPS
        if below:
            dx, dy = 0.0, 0.0
        else:
            dx, dy = dx / current, dy / current
            if self.rule == "zero_sign_lost":
                dx, dy = (0.0 if dx == 0.0 else dx), (0.0 if dy == 0.0 else dy)
        violation = current - target_distance
        divisor = (wa + wb) + compliance
        if divisor < rm.EPS:
            return 0, 0, 0, 0
        correction = -violation / divisor
        if self.rule != "clamp_missing":
            correction = rm.clamp(correction, -abs(violation), abs(violation))
        return -dx * correction * wa, -dy * correction * wa, dx * correction * wb, dy * correction * wb

    # ---- L:1548-1666
    def _solve_collision(self, particles, n_particles, spatial_hash, collided, collision_overlap_factor, collision_compliance,
                         cohesion_interaction_distance_factor, cohesion_compliance, max_n_collisions, visit_log=None):
        site = "collision:" + TYPE[self._which(particles)]
        rule = self.rule
        eps = rm.EPS
        seen = []
        n_collided = 0
        cut = False
        for self_p in range(1, n_particles + 1):
            si = rm.offset(self_p)
            ws, rs, bs = particles[si + rm.INV_MASS], particles[si + rm.RADIUS], particles[si + rm.BATCH_ID]
            cell_x, cell_y = particles[si + rm.CELL_X], particles[si + rm.CELL_Y]
            for x_offset in (-1, 0, 1):
                for y_offset in (-1, 0, 1):
                    entry = spatial_hash.get(rm.xy_to_hash(cell_x + x_offset, cell_y + y_offset))
                    if entry is None:
                        continue
                    for other_p in entry:
                        if self_p == other_p:
                            continue
                        pair_hash = rm.xy_to_hash(min(self_p, other_p), max(self_p, other_p))
                        if collided.get(pair_hash) is True:
                            continue
                        collided[pair_hash] = True
                        oi = rm.offset(other_p)
                        wo, ro, bo = particles[oi + rm.INV_MASS], particles[oi + rm.RADIUS], particles[oi + rm.BATCH_ID]
                        sx, sy, ox, oy = particles[si + rm.X], particles[si + rm.Y], particles[oi + rm.X], particles[oi + rm.Y]
                        labels = classify(sx, sy, ox, oy, ws, wo, rs, ro, bs == bo, collision_overlap_factor, collision_compliance, eps)
                        self._count(site, labels)
                        seen.append((self_p - 1, other_p - 1, labels))
                        guarded = ws + wo <= eps if rule == "eps_inclusive" else ws + wo < eps
                        assert rule is not None or guarded == ("guarded" in labels)
                        if guarded:
                            if rule == "guard_counts":
                                n_collided += 1
                                if n_collided >= max_n_collisions:
                                    cut = True
                            if cut:
                                break
                            continue
                        if bs == bo and rule != "no_plus_zero" and rm.squared_distance(sx, sy, ox, oy) <= 0:  # interaction distance 0
                            c = self._project(sx, sy, ox, oy, ws, wo, 0, cohesion_compliance)
                            particles[si + rm.X], particles[si + rm.Y] = sx + c[0], sy + c[1]
                            particles[oi + rm.X], particles[oi + rm.Y] = ox + c[2], oy + c[3]
                        min_distance = collision_overlap_factor * (rs + ro)
                        sx, sy, ox, oy = particles[si + rm.X], particles[si + rm.Y], particles[oi + rm.X], particles[oi + rm.Y]
                        dist = rm.squared_distance(sx, sy, ox, oy)
                        fires = dist < min_distance * min_distance if rule == "edge_excluded" else dist <= min_distance * min_distance
                        assert rule is not None or fires == ("fires" in labels)
                        if fires:
                            c = self._project(sx, sy, ox, oy, ws, wo, min_distance, collision_compliance)
                            particles[si + rm.X], particles[si + rm.Y] = sx + c[0], sy + c[1]
                            particles[oi + rm.X], particles[oi + rm.Y] = ox + c[2], oy + c[3]
                        n_collided += 1
                        if visit_log is not None:
                            visit_log.append((self_p, other_p))
                        if n_collided >= max_n_collisions:
                            cut = True
                            self.cut_on.append((site, self_p - 1, other_p - 1))
                            break
                    if cut:
                        break
                if cut:
                    break
            if cut:
                break
        if seen and site not in self.first:
            self.first[site] = seen
        self.pair_solves += n_collided
        self.cuts += cut
        return n_collided, cut
