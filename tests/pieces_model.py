"""The definition of the pieces (egg_pieces, include/eggsim.h "pieces") in numpy.

An ATOM is the particles of one type of one batch, numbered by their index in the batch.  Two particles i, j of an atom are
LINKED iff d2 <= L * L, float64 in exactly this order:

    dx = x[i] - x[j];  dy = y[i] - y[j];  d2 = dx * dx + dy * dy
    L  = reach[type] * (radius[i] + radius[j])

(false when anything in it is a NaN).  A PIECE is a connected component, the LABEL of a particle the lowest index in its
piece, the BODY the largest piece and among equals the one with the lower label.  A record is the tuple
(n, pieces, largest, first, singles, dropped, sx, sy) of Python ints; an atom without particles, or of a type the mask leaves
out, is all zeros.

`rule` switches on ONE of the wrong rules the hand table of tests/test_pieces_model.py must notice; the library implements
rule=None.
"""
import numpy as np

SCALE = 65536.0  # EGG_SENSOR_POSITION_SCALE
LIMIT = 2.0 ** 53
ZERO = (0, 0, 0, 0, 0, 0, 0, 0)
WRONG_RULES = ("strict", "max_radius", "cross_batch", "tie_high", "one_sweep")
_ROWS = 512  # rows of the link matrix held at a time


def linked(x, y, r, reach, rows, rule=None):
    """the link matrix of the particles `rows` (a slice) against every particle: bool [len(rows), n]"""
    with np.errstate(invalid="ignore", over="ignore"):
        dx = x[rows, None] - x[None, :]
        dy = y[rows, None] - y[None, :]
        d2 = dx * dx + dy * dy
        if rule == "max_radius":
            L = reach * np.maximum(r[rows, None], r[None, :])
        else:
            L = reach * (r[rows, None] + r[None, :])
        return d2 < L * L if rule == "strict" else d2 <= L * L


def labels_of(x, y, r, reach, rule=None):
    """the label of every particle of one atom: min-label propagation with pointer jumping until a sweep changes nothing.
    Any other way to the connected components gives the same array: the fixed point is unique."""
    x, y, r = (np.asarray(v, dtype=np.float64) for v in (x, y, r))
    n = x.size
    label = np.arange(n, dtype=np.int64)
    # the links once, as a list of (i, j): the matrix is built in blocks of rows and never held whole
    ei, ej = [], []
    for at in range(0, n, _ROWS):
        i, j = np.nonzero(linked(x, y, r, float(reach), slice(at, min(n, at + _ROWS)), rule))
        ei.append(i + at)
        ej.append(j)
    ei, ej = (np.concatenate(e) if e else np.zeros(0, dtype=np.int64) for e in (ei, ej))
    while n:
        new = label.copy()
        np.minimum.at(new, ei, label[ej])  # the lowest label among the linked j
        new = new[new]  # pointer jumping
        if np.array_equal(new, label) or rule == "one_sweep":
            label = new
            break
        label = new
    return label.astype(np.int32)


def record_of(x, y, label, rule=None):
    """the record of one atom from its labels"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = int(x.size)
    if n == 0:
        return ZERO
    size = np.bincount(label, minlength=n)
    leads = np.flatnonzero(size > 0)
    largest = int(size.max())
    tied = leads[size[leads] == largest]
    first = int(tied.max() if rule == "tie_high" else tied.min())
    body = label == first
    with np.errstate(invalid="ignore", over="ignore"):
        fx, fy = x * SCALE, y * SCALE
        ok = (np.abs(fx) < LIMIT) & (np.abs(fy) < LIMIT)  # (false for a NaN and for an infinity)
    keep = body & ok
    sx = sum(int(v) for v in np.rint(fx[keep]))  # (Python ints: exact)
    sy = sum(int(v) for v in np.rint(fy[keep]))
    wrap = lambda v: (v + 2 ** 63) % 2 ** 64 - 2 ** 63  # (an int64 sum wraps; below 2^10 particles it cannot)
    return (n, int(leads.size), largest, first, int((size == 1).sum()), int((body & ~ok).sum()), wrap(sx), wrap(sy))


def pieces(particles, ids, reach, mask=3, rule=None):
    """`particles` = (white, yolk), each a dict of the arrays x, y, radius, batch_id in download() order; `ids` the requested
    batch ids in the caller's order (an id may repeat); `reach` = (white, yolk).  Returns (records, labels): records[k] =
    (white record, yolk record) of ids[k]; labels = (white, yolk) int32 arrays, -1 for a particle of an atom that was not asked
    for."""
    records = [[ZERO, ZERO] for _ in ids]
    labels = []
    for w in (0, 1):
        p = particles[w]
        x, y, r = (np.asarray(p[k], dtype=np.float64) for k in ("x", "y", "radius"))
        bid = np.asarray(p["batch_id"]).astype(np.int64)
        lab = np.full(x.size, -1, dtype=np.int32)
        labels.append(lab)
        if not mask >> w & 1:
            continue
        whole = labels_of(x, y, r, reach[w], rule) if rule == "cross_batch" else None
        done = {}
        for k, i in enumerate(ids):
            if i not in done:
                at = np.flatnonzero(bid == int(i))
                if at.size and not np.array_equal(at, np.arange(at[0], at[0] + at.size)):
                    raise ValueError("batch %d is not contiguous" % i)
                if whole is not None and at.size:  # the wrong rule: pieces joined through other batches' particles
                    own = whole[at]
                    atom = np.array([int(np.flatnonzero(own == v)[0]) for v in own], dtype=np.int32)
                else:
                    atom = labels_of(x[at], y[at], r[at], reach[w], rule)
                lab[at] = atom
                done[i] = record_of(x[at], y[at], atom, rule)
            records[k][w] = done[i]
    return [tuple(pair) for pair in records], tuple(labels)


def summary(record):
    """what the wrappers make of a record: None, or (n, pieces, largest, first, singles, dropped, x, y) with the body's centroid
    by the library's two divisions (None while every body particle was dropped)"""
    n, count, largest, first, singles, dropped, sx, sy = record
    if n == 0:
        return None
    kept = largest - dropped
    return (n, count, largest, first, singles, dropped, (float(sx) / SCALE) / float(kept) if kept else None,
            (float(sy) / SCALE) / float(kept) if kept else None)
