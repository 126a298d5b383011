"""The rule of the probes (include/eggsim.h, "probes") in numpy: the definition the device kernel
(csrc/eggsim_probes.hip), the device group and the sharded ranks are held to, field for field with ==.

A probe is a tuple `("point", x, y[, reach[, types]])` or `("ray", x0, y0, x1, y1[, pad[, types]])`; reach defaults to inf,
pad to 0, types ("both" | "white" | "yolk" or the mask 1 .. 3) to both.  The particles of one type are a dict of equally
long arrays: x, y, radius (float64), key, index, id (int64) -- the batch's key, the particle's 0-based index in the batch's run
of that type, the batch's id.  All arithmetic is float64 in exactly the order written; numpy's sqrt and / are correctly
rounded, as the device's are; every comparison is false for a NaN.

`wrong` names a deliberately wrong rule (WRONG_RULES): tests/test_probe_model.py shows that its hand table tells each of
them from the right one."""
import math

import numpy as np

MAX_PROBES = 64
KINDS = ("point", "ray")
N_PARAMS = {"point": 3, "ray": 5}
DEFAULT_LAST = {"point": math.inf, "ray": 0.0}
TYPES = {"white": 1, "yolk": 2, "both": 3}
EPS = 1e-8  # the white config's eps: a ray with l2 < EPS EPS is refused
WRONG_RULES = ("strict_reach", "ties_to_highest", "ties_by_id", "ray_ignores_radius", "ray_ignores_pad", "inside_is_a_miss",
               "behind_accepted", "beyond_accepted", "nan_is_a_candidate", "mask_ignored")


def canonical(probes):
    """the list as the library takes it: per probe (kind, type_mask, [5 parameters]); ValueError with the probe's index for
    what egg_probe refuses"""
    probes = list(probes)
    if len(probes) > MAX_PROBES:
        raise ValueError("a call takes 0 .. %d probes" % MAX_PROBES)
    out = []
    for k, q in enumerate(probes):
        q = tuple(q)
        kind = q[0] if q else None
        if kind not in KINDS:
            raise ValueError("probe %d: unknown kind %r" % (k, kind))
        n = N_PARAMS[kind]
        values, types = list(q[1:]), "both"
        if len(values) == n + 1 or (values and isinstance(values[-1], str)):
            types = values.pop()
        if len(values) == n - 1:
            values.append(DEFAULT_LAST[kind])
        if len(values) != n:
            raise ValueError("probe %d (%s): %d parameters" % (k, kind, len(values)))
        mask = TYPES.get(types) if isinstance(types, str) else types
        if mask not in (1, 2, 3):
            raise ValueError("probe %d: types %r" % (k, types))
        p = [float(v) for v in values]
        for i, v in enumerate(p):
            if math.isnan(v) or (math.isinf(v) and not (kind == "point" and i == 2 and v > 0)):
                raise ValueError("probe %d (%s): parameter %d is not finite" % (k, kind, i))
        if p[-1] < 0:
            raise ValueError("probe %d (%s): negative %s" % (k, kind, "reach" if kind == "point" else "pad"))
        if kind == "ray":
            ex, ey = p[2] - p[0], p[3] - p[1]
            l2 = ex * ex + ey * ey
            if not l2 >= EPS * EPS or math.isinf(l2):
                raise ValueError("probe %d (ray): degenerate" % k)
        out.append((kind, mask, p + [0.0] * (5 - n)))
    return out


def evaluate(kind, p, x, y, radius, wrong=None):
    """one probe against the arrays of one type: (candidate, score), a bool and a float64 array.  The score of a particle
    that is no candidate means nothing."""
    x, y, radius = (np.asarray(a, dtype=np.float64) for a in (x, y, radius))
    with np.errstate(all="ignore"):
        if kind == "point":
            px, py, reach = np.float64(p[0]), np.float64(p[1]), np.float64(p[2])
            dx, dy = x - px, y - py
            d2 = dx * dx + dy * dy
            if wrong == "nan_is_a_candidate":
                return ~(d2 > reach * reach), d2
            if wrong == "strict_reach":
                return (d2 < reach * reach) & (radius == radius), d2
            return (d2 <= reach * reach) & (radius == radius), d2
        x0, y0, x1, y1, pad = (np.float64(v) for v in p[:5])
        if wrong == "ray_ignores_pad":
            pad = np.float64(0.0)
        R = radius + pad
        if wrong == "ray_ignores_radius":
            R = np.zeros_like(radius) + pad
        fx, fy = x0 - x, y0 - y
        c = (fx * fx + fy * fy) - R * R
        inside = c <= 0.0
        ex, ey = x1 - x0, y1 - y0
        l2 = ex * ex + ey * ey
        b = fx * ex + fy * ey
        q = b * b - l2 * c
        t = (-b - np.sqrt(q)) / l2
        ahead = b < 0.0
        if wrong == "behind_accepted":
            ahead = np.ones_like(inside)
        within = t <= 1.0
        if wrong == "beyond_accepted":
            within = t == t
        hit = ~inside & ahead & (q >= 0.0) & within
        if wrong is None:
            assert not np.any(hit & (t < 0.0)), "t is never negative: sqrt(q) <= -b after rounding when c > 0"
        if wrong == "inside_is_a_miss":
            return hit, t
        return inside | hit, np.where(inside, 0.0, t)


def select(candidate, score, key, index, ident=None, wrong=None):
    """the position of the winner among the candidates, or None: the smallest score by <, among equal scores the smallest
    key, then the smallest index"""
    at = np.flatnonzero(candidate)
    if at.size == 0:
        return None
    if wrong is None:  # (no candidate's score is a NaN)
        ties = at[score[at] == score[at].min()]
        return int(ties[np.lexsort((index[ties], key[ties]))[0]])
    best = None
    order = key if wrong != "ties_by_id" else ident
    for i in at:
        if best is None or score[i] < score[best]:
            best = i
        elif score[i] == score[best]:
            earlier = (order[i], index[i]) < (order[best], index[best])
            if earlier != (wrong == "ties_to_highest"):
                best = i
    return int(best)


def probe(probes, particles, wrong=None):
    """per probe `(white_hit_or_None, yolk_hit_or_None)`, a hit being the tuple (id, index, score, x, y, radius) of Python
    ints and floats; `particles` = (white, yolk), see the module's text"""
    out = []
    for kind, mask, p in canonical(probes):
        pair = []
        for w in (0, 1):
            a = particles[w]
            if not (mask >> w & 1) and wrong != "mask_ignored" or len(a["x"]) == 0:
                pair.append(None)
                continue
            cand, score = evaluate(kind, p, a["x"], a["y"], a["radius"], wrong)
            i = select(cand, score, a["key"], a["index"], a["id"], wrong)
            pair.append(None if i is None else (int(a["id"][i]), int(a["index"][i]), float(score[i]), float(a["x"][i]),
                                                float(a["y"][i]), float(a["radius"][i])))
        out.append(tuple(pair))
    return out


def first(pair):
    """pick / raycast: None or `(type_name, hit)`, the lower score of the two types; an exact tie goes to white"""
    white, yolk = pair
    if white is None and yolk is None:
        return None
    if yolk is None or (white is not None and not yolk[2] < white[2]):
        return ("white", white)
    return ("yolk", yolk)


def impact(p, t):
    """the point of impact of a ray (x0, y0, x1, y1, ...) at t: (x0 + t ex, y0 + t ey)"""
    x0, y0, x1, y1 = (float(v) for v in p[:4])
    return (x0 + t * (x1 - x0), y0 + t * (y1 - y0))


def particles_of(x, y, radius, batch_id, key_of):
    """the arrays of one type from its downloads: a batch's particles are one run of equal batch_id, in download order;
    `key_of` maps a batch's id to its key"""
    batch_id = np.asarray(batch_id).astype(np.int64)
    n = batch_id.size
    starts = np.flatnonzero(np.r_[True, batch_id[1:] != batch_id[:-1]]) if n else np.zeros(0, dtype=np.int64)
    index = np.arange(n, dtype=np.int64) - np.repeat(starts, np.diff(np.r_[starts, n]))
    ids, inverse = np.unique(batch_id, return_inverse=True)
    key = np.array([key_of[int(b)] for b in ids], dtype=np.int64)[inverse] if n else np.zeros(0, dtype=np.int64)
    return dict(x=np.asarray(x, dtype=np.float64), y=np.asarray(y, dtype=np.float64), radius=np.asarray(radius, dtype=np.float64),
                key=key, index=index, id=batch_id)
