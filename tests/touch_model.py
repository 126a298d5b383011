"""The definition of the touches (egg_touches, include/eggsim_touch.h) in numpy.

A QUERY is a set of discs (x, y, r) of one type with a key: the atom of a listed batch (its key is the batch's id), or discs a
caller hands in.  Particle a of a query and particle b of the SAME type in a batch whose id differs from the query's key TOUCH
iff d2 <= L * L, float64 in exactly this order (the order of tests/pieces_model.py):

    dx = xa - xb;  dy = ya - yb;  d2 = dx * dx + dy * dy
    L  = reach[type] * (ra + rb)

(false when anything in it is a NaN).  Per (entry i of the query list, type w, other batch) with at least one touching pair
there is ONE record, the tuple (i, w, other, pairs, particles, dropped, sx, sy) of Python ints:

    pairs      the touching (a, b) pairs
    particles  the distinct particles b of the other batch in them
    dropped    the touching pairs in which a scaled coordinate of either particle reaches LIMIT or is not finite: they count
               in pairs and add nothing to the sums
    sx, sy     int64 two's complement sums over the remaining pairs of q(xa) + q(xb) and q(ya) + q(yb), q(v) = rint(v * SCALE)

Records are ordered by (i, w, other).  There is no cull here: the library's cull may only skip what this rule rejects.

`rule` switches on ONE of the wrong rules the hand table of tests/test_touch_model.py must notice; the library implements
rule=None.
"""
import numpy as np

SCALE = 65536.0  # EGG_SENSOR_POSITION_SCALE
LIMIT = 2.0 ** 53
WRONG_RULES = ("strict", "max_radius", "same_batch", "cross_type", "one_sided_sum", "pairs_for_particles")
_ROWS = 256  # query discs held against every particle at a time


def _wrap(v):
    return (v + 2 ** 63) % 2 ** 64 - 2 ** 63  # (an int64 sum wraps)


def _quantise(v):
    """(q(v) as a list of Python ints, ok): ok is false for a NaN, an infinity and a scaled value that reaches LIMIT"""
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.asarray(v, dtype=np.float64) * SCALE
        ok = np.abs(f) < LIMIT
    return [int(t) for t in np.rint(np.where(ok, f, 0.0))], ok


def touching(xa, ya, ra, xb, yb, rb, reach, rule=None):
    """the touch matrix of the discs a against the discs b: bool [len(a), len(b)]"""
    xa, ya, ra, xb, yb, rb = (np.asarray(v, dtype=np.float64) for v in (xa, ya, ra, xb, yb, rb))
    with np.errstate(invalid="ignore", over="ignore"):
        dx = xa[:, None] - xb[None, :]
        dy = ya[:, None] - yb[None, :]
        d2 = dx * dx + dy * dy
        if rule == "max_radius":
            L = float(reach) * np.maximum(ra[:, None], rb[None, :])
        else:
            L = float(reach) * (ra[:, None] + rb[None, :])
        return d2 < L * L if rule == "strict" else d2 <= L * L


def records_of(queries, particles, reach, mask=3, rule=None):
    """`queries` a list of (key, type, x, y, r), entry i of the list the i-th of them; `particles` = (white, yolk), each a dict of
    the arrays x, y, radius and label (the id, or the key, of each particle's batch); `reach` = (white, yolk).  Returns the
    ordered list of records."""
    out = []
    for i, (key, w, x, y, r) in enumerate(queries):
        w = int(w)
        if not mask >> w & 1:
            continue
        x, y, r = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (x, y, r))
        qxa, okxa = _quantise(x)
        qya, okya = _quantise(y)
        merged = {}
        for t in ((0, 1) if rule == "cross_type" else (w,)):
            p = particles[t]
            px, py, pr = (np.asarray(p[k], dtype=np.float64) for k in ("x", "y", "radius"))
            label = np.asarray(p["label"]).astype(np.int64)
            qxb, okxb = _quantise(px)
            qyb, okyb = _quantise(py)
            hits_a, hits_b = [], []
            for at in range(0, x.size, _ROWS):
                rows = slice(at, min(x.size, at + _ROWS))
                m = touching(x[rows], y[rows], r[rows], px, py, pr, reach[w], rule)
                if rule != "same_batch":
                    m &= (label != int(key))[None, :]
                a, b = np.nonzero(m)
                hits_a.append(a + at)
                hits_b.append(b)
            a = np.concatenate(hits_a) if hits_a else np.zeros(0, dtype=np.int64)
            b = np.concatenate(hits_b) if hits_b else np.zeros(0, dtype=np.int64)
            for other in np.unique(label[b]).tolist():
                sel = label[b] == other
                sa, sb = a[sel], b[sel]
                ok = okxa[sa] & okya[sa] & okxb[sb] & okyb[sb]
                sx = sum(qxa[u] + (0 if rule == "one_sided_sum" else qxb[v]) for u, v in zip(sa[ok].tolist(), sb[ok].tolist()))
                sy = sum(qya[u] + (0 if rule == "one_sided_sum" else qyb[v]) for u, v in zip(sa[ok].tolist(), sb[ok].tolist()))
                n_pairs = int(sa.size)
                n_b = n_pairs if rule == "pairs_for_particles" else int(np.unique(sb).size)
                old = merged.get(other, (0, 0, 0, 0, 0))
                merged[other] = (old[0] + n_pairs, old[1] + n_b, old[2] + int((~ok).sum()), old[3] + sx, old[4] + sy)
        for other in sorted(merged):
            n_pairs, n_b, dropped, sx, sy = merged[other]
            out.append((i, w, int(other), n_pairs, n_b, dropped, _wrap(sx), _wrap(sy)))
    out.sort(key=lambda rec: rec[:3])
    return out


def labelled(particles, label="batch_id"):
    """(white, yolk) dicts of download() arrays with `label` taken from the field named"""
    return tuple(dict(x=p["x"], y=p["y"], radius=p["radius"], label=np.asarray(p[label]).astype(np.int64)) for p in particles)


def touches(particles, ids, reach, mask=3, rule=None):
    """`particles` = (white, yolk), each a dict of the arrays x, y, radius, batch_id in download() order; `ids` the requested
    batch ids in the caller's order (an id may repeat); `reach` = (white, yolk).  The queries are the atoms of the listed
    batches, entry i of `ids` giving the queries 2 i (white) and 2 i + 1 (yolk); a record's entry is i."""
    parts = labelled(particles)
    queries = []
    for i in ids:
        for w in (0, 1):
            at = parts[w]["label"] == int(i)
            queries.append((int(i), w, parts[w]["x"][at], parts[w]["y"][at], parts[w]["radius"][at]))
    recs = records_of(queries, parts, reach, mask, rule)
    return [(rec[0] // 2,) + rec[1:] for rec in recs]


def contact(record):
    """the contact point of a record by the library's divisions: (x, y), or None while every pair was dropped"""
    _, _, _, pairs, _, dropped, sx, sy = record
    kept = pairs - dropped
    if kept <= 0:
        return None
    return ((float(sx) / (2.0 * kept)) / SCALE, (float(sy) / (2.0 * kept)) / SCALE)
