"""The rule of the measures (include/eggsim_measure.h) in numpy float64 and Python ints: the
definition the device kernel (csrc/eggsim_measures.hip) is held against.

An ATOM is the particles of one type of one batch.  A record is the tuple of the 24 Python ints FIELDS names.  Constants:
S = 2^16, SM = 2^32, LIM = 2^53; q(v) = rint(v) as an int, taken only where |v| < LIM; m = 1.0 / inv_mass.

A particle of type w of a requested batch is MEASURED when the mask has bit w and, with a region, the region's test holds
(tests/sensor_model.py, the region's own type mask included).  Pass 1, per measured particle: x*S, y*S, m*SM, (m*x)*S,
(m*y)*S, (m*vx)*S, (m*vy)*S, v2 = vx*vx + vy*vy then (m*v2)*S and v2*S, (x-r)*S, (y-r)*S, (x+r)*S, (y+r)*S; the particle is
KEPT iff all thirteen are below LIM in magnitude, otherwise it counts in `dropped`.  Pass 2: kept = n - dropped,
ox_q = sx / kept and oy_q = sy / kept truncated toward zero, ox = ox_q / S; per kept particle dx = x - ox, dy = y - oy,
d2 = dx*dx + dy*dy and the terms (dx*dx)*S, (dx*dy)*S, (dy*dy)*S, (m*(dx*vy - dy*vx))*S, (sqrt(d2) + r)*S; a kept particle
with one of them at or beyond LIM counts in `dropped_central`.  Extremes are taken on the quantised integers.  numpy float64
element-wise in exactly this order (numpy never contracts a product into a sum; sqrt and / are correctly rounded); every
comparison is false for a NaN.  Written from the header's text alone; it shares no code with the library.

`rule` switches on ONE of the wrong rules the hand table of tests/test_measure_model.py must notice; the library implements
rule=None.
"""
import math

import numpy as np

import sensor_model

S = 65536.0
SM = 4294967296.0
LIM = 2.0 ** 53
FIELDS = ("atom", "n", "dropped", "sx", "sy", "sm", "smx", "smy", "spx", "spy", "se", "lo_x", "lo_y", "hi_x", "hi_y", "max_v2",
          "ox_q", "oy_q", "dropped_central", "sxx", "sxy", "syy", "sl", "max_reach")
ZERO = (0,) * 24
WRONG_RULES = ("floor", "double_extremes", "centroid_origin", "dropped_extremes", "inv_mass")


def _wrap(v):
    return (int(v) + 2 ** 63) % 2 ** 64 - 2 ** 63  # (an int64 sum wraps)


def _q(v):
    """rint of the float64 array as Python ints (exact: every |v| is below 2^53)"""
    return [int(t) for t in np.rint(v)]


def _trunc_div(a, b, rule):
    if rule == "floor":
        return a // b
    return (abs(a) // b) * (1 if a >= 0 else -1)


def record_of(x, y, vx, vy, radius, inv_mass, measured=None, rule=None):
    """the record of one atom; `measured` a bool array (None: every particle)"""
    x, y, vx, vy, r, im = (np.asarray(v, dtype=np.float64) for v in (x, y, vx, vy, radius, inv_mass))
    atom = int(x.size)
    if atom == 0:
        return ZERO
    measured = np.ones(atom, dtype=bool) if measured is None else np.asarray(measured, dtype=bool)
    with np.errstate(all="ignore"):
        m = im.copy() if rule == "inv_mass" else 1.0 / im
        v2 = vx * vx + vy * vy
        terms = [x * S, y * S, m * SM, (m * x) * S, (m * y) * S, (m * vx) * S, (m * vy) * S, (m * v2) * S, v2 * S,
                 (x - r) * S, (y - r) * S, (x + r) * S, (y + r) * S]
        ok = np.ones(atom, dtype=bool)
        for t in terms:
            ok &= np.abs(t) < LIM  # (false for a NaN and for an infinity)
    keep = measured & ok
    n, dropped = int(measured.sum()), int((measured & ~ok).sum())
    kept = n - dropped
    rec = [atom, n, dropped] + [0] * 21
    if kept == 0:
        return tuple(rec)
    sums = [_wrap(sum(_q(t[keep]))) for t in terms[:8]]
    rec[3:11] = sums
    ext = (measured if rule == "dropped_extremes" else keep)
    if rule == "double_extremes":  # (the extremes stay doubles: the sign of a zero then depends on the order of the particles)
        lo_x, lo_y = (np.rint(np.min(t[ext])) for t in terms[9:11])
        hi_x, hi_y = (np.rint(np.max(t[ext])) for t in terms[11:13])
        max_v2 = np.rint(np.max(terms[8][ext]))
    else:
        with np.errstate(all="ignore"):
            safe = [np.where(np.abs(t) < LIM, t, 0.0) for t in terms]
        lo_x, lo_y = (min(_q(t[ext])) for t in safe[9:11])
        hi_x, hi_y = (max(_q(t[ext])) for t in safe[11:13])
        max_v2 = max(_q(safe[8][ext]))
    rec[11:16] = [lo_x, lo_y, hi_x, hi_y, max_v2]
    ox_q, oy_q = _trunc_div(sums[0], kept, rule), _trunc_div(sums[1], kept, rule)
    rec[16:18] = [ox_q, oy_q]
    if rule == "centroid_origin":
        ox, oy = float(np.mean(x[keep])), float(np.mean(y[keep]))
    else:
        ox, oy = float(ox_q) / S, float(oy_q) / S
    with np.errstate(all="ignore"):
        dx, dy = x - ox, y - oy
        d2 = dx * dx + dy * dy
        central = [(dx * dx) * S, (dx * dy) * S, (dy * dy) * S, (m * (dx * vy - dy * vx)) * S, (np.sqrt(d2) + r) * S]
        ok2 = np.ones(atom, dtype=bool)
        for t in central:
            ok2 &= np.abs(t) < LIM
    dc = int((keep & ~ok2).sum())
    rec[18] = dc
    both = keep & ok2
    if kept > dc:
        rec[19:23] = [_wrap(sum(_q(t[both]))) for t in central[:4]]
        rec[23] = max(_q(central[4][both]))
    return tuple(rec)


def measure(particles, ids, region=None, mask=3, rule=None, eps=1e-8):
    """`particles` = (white, yolk), each a dict of the arrays x, y, vx, vy, radius, inv_mass, batch_id in download() order;
    `ids` the requested batch ids in the caller's order (an id may repeat); `region` None or a region as the Python wrapper
    takes it.  Returns an int64 array [len(ids), 2, 24]."""
    sensor = None if region is None else sensor_model.canonical([region], eps)[0]
    out = np.zeros((len(ids), 2, 24), dtype=np.int64)
    for w in (0, 1):
        if not mask >> w & 1:
            continue
        p = particles[w]
        arrays = [np.asarray(p[k], dtype=np.float64) for k in ("x", "y", "vx", "vy", "radius", "inv_mass")]
        bid = np.asarray(p["batch_id"]).astype(np.int64)
        done = {}
        for k, i in enumerate(ids):
            if i not in done:
                at = np.flatnonzero(bid == int(i))
                a = [v[at] for v in arrays]
                measured = None
                if sensor is not None:
                    if sensor[1] >> w & 1:
                        with np.errstate(all="ignore"):
                            measured = np.asarray(sensor_model.inside(sensor, a[0], a[1]), dtype=bool)
                    else:
                        measured = np.zeros(at.size, dtype=bool)
                done[i] = record_of(*a, measured=measured, rule=rule)
            out[k, w] = done[i]
    return out


def derived(record):
    """what the wrappers derive from a record on the host, by their formulas: None where n == 0, else a dict"""
    r = dict(zip(FIELDS, (int(v) for v in record)))
    if r["n"] == 0:
        return None
    kept = r["n"] - r["dropped"]
    d = dict(r, kept=kept)
    mass = float(r["sm"]) / SM
    d["mass"] = mass
    d["centroid"] = ((float(r["sx"]) / S) / kept, (float(r["sy"]) / S) / kept) if kept else None
    d["center_of_mass"] = ((float(r["smx"]) / S) / mass, (float(r["smy"]) / S) / mass) if mass > 0.0 else None
    d["momentum"] = (float(r["spx"]) / S, float(r["spy"]) / S)
    d["velocity"] = (d["momentum"][0] / mass, d["momentum"][1] / mass) if mass > 0.0 else None
    d["kinetic_energy"] = 0.5 * float(r["se"]) / S
    d["bounds"] = (float(r["lo_x"]) / S, float(r["lo_y"]) / S, float(r["hi_x"]) / S, float(r["hi_y"]) / S) if kept else None
    d["max_speed"] = math.sqrt(float(r["max_v2"]) / S)
    d["origin"] = (float(r["ox_q"]) / S, float(r["oy_q"]) / S)
    d["reach"] = float(r["max_reach"]) / S
    d["spin"] = float(r["sl"]) / S
    return d


def axes(record):
    """(major standard deviation, minor standard deviation, angle of the major axis) from sxx, sxy, syy; None without a
    central particle"""
    r = dict(zip(FIELDS, (int(v) for v in record)))
    k = r["n"] - r["dropped"] - r["dropped_central"]
    if k <= 0:
        return None
    cxx, cxy, cyy = (float(r["sxx"]) / S) / k, (float(r["sxy"]) / S) / k, (float(r["syy"]) / S) / k
    half, diff = 0.5 * (cxx + cyy), 0.5 * (cxx - cyy)
    root = math.sqrt(diff * diff + cxy * cxy)
    return (math.sqrt(max(half + root, 0.0)), math.sqrt(max(half - root, 0.0)), 0.5 * math.atan2(2.0 * cxy, cxx - cyy))
