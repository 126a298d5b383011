"""The rule of the sensors (include/eggsim.h, "sensors") in numpy float64 and Python ints: the
definition the device kernel (csrc/eggsim_sensors.hip) is held against.

A sensor is given as the Python wrapper takes it: `(kind, parameters...[, types])`,
  ("half_plane", nx, ny, off)          s = (nx x + ny y) - off; inside iff s >= 0.0 (the normal normalised when the list is set)
  ("disc", cx, cy, R)                  dx = x - cx, dy = y - cy, d2 = dx dx + dy dy; inside iff d2 <= R R
  ("box", cx, cy, hx, hy, ux, uy)      u = dx ux + dy uy, v = dy ux - dx uy; inside iff |u| <= hx and |v| <= hy (the axis normalised
  ("box", cx, cy, hx, hy, angle)       when set; an angle goes through the host's cos / sin first)
  ("capsule", x0, y0, x1, y1, R)       e, l2, t, q as the segment collider; d2 to q; inside iff d2 <= R R
types = "both" | "white" | "yolk" (mask 3, 1, 2).  numpy float64 element-wise in exactly this order; every comparison is
false for a NaN.  A particle of type w inside sensor k adds 1, llrint(x 2^16), llrint(y 2^16) to the sensor's (count, sx, sy)
of type w; if a scaled coordinate is not finite or reaches 2^53 it adds nothing and dropped[w] counts it, once per sensor
it is inside.  Written from the header's text alone; it shares no code with the library.

`wrong` names ONE deliberately wrong rule (tests/test_sensor_model.py: a table case must tell each from the right one).
"""
import math

import numpy as np

SCALE = 65536.0
LIMIT = 2.0 ** 53
MAX_SENSORS = 64
KINDS = ("half_plane", "disc", "box", "capsule")
N_PARAMS = {"half_plane": 3, "disc": 3, "box": 6, "capsule": 5}
MASKS = {"white": 1, "yolk": 2, "both": 3}
WRONG_RULES = ("strict", "other_side", "unnormalised", "ignored_mask", "swapped_uv", "unclamped_t", "truncation",
               "drop_counts")


def canonical(sensors, eps=1e-8, wrong=None):
    """the list as egg_set_sensors stores it: [(kind, mask, [6 parameters])]; ValueError("sensor k: ...") for a list it refuses"""
    sensors = list(sensors)
    if len(sensors) > MAX_SENSORS:
        raise ValueError("a list holds 0 .. %d sensors" % MAX_SENSORS)
    out = []
    for k, s in enumerate(sensors):
        s = tuple(s)
        kind = s[0] if s else None
        if kind not in KINDS:
            raise ValueError("sensor %d: unknown kind %r" % (k, kind))
        values = list(s[1:])
        types = values.pop() if values and isinstance(values[-1], str) else "both"
        if types not in MASKS:
            raise ValueError("sensor %d: types %r" % (k, types))
        p = [float(v) for v in values]
        if kind == "box" and len(p) == 5:
            p = p[:4] + [math.cos(p[4]), math.sin(p[4])]
        if len(p) != N_PARAMS[kind]:
            raise ValueError("sensor %d (%s): %d parameters" % (k, kind, len(p)))
        if not all(math.isfinite(v) for v in p):
            raise ValueError("sensor %d (%s): a parameter is not finite" % (k, kind))
        negative = {"disc": p[2:3], "capsule": p[4:5], "box": p[2:4], "half_plane": []}[kind]
        if any(v < 0 for v in negative):
            raise ValueError("sensor %d (%s): a radius or half extent is negative" % (k, kind))
        if kind in ("half_plane", "box"):
            a = 4 if kind == "box" else 0
            length = math.sqrt(p[a] * p[a] + p[a + 1] * p[a + 1])
            if not (length >= eps) or not math.isfinite(length):
                raise ValueError("sensor %d (%s): the normal or axis is shorter than eps" % (k, kind))
            if wrong != "unnormalised":
                p[a], p[a + 1] = p[a] / length, p[a + 1] / length
        out.append((kind, MASKS[types], p + [0.0] * (6 - len(p))))
    return out


def _le(a, b, wrong):
    return a < b if wrong == "strict" else a <= b


def inside(sensor, x, y, wrong=None):
    """bool array: which of the positions (x, y) lie inside one canonical sensor (the mask is not looked at)"""
    kind, _mask, p = sensor
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == "half_plane":
            s = (p[0] * x + p[1] * y) - p[2]
            if wrong == "other_side":
                return s <= 0.0
            return s > 0.0 if wrong == "strict" else s >= 0.0
        if kind == "box":
            dx = x - p[0]
            dy = y - p[1]
            u = dx * p[4] + dy * p[5]
            v = dy * p[4] - dx * p[5]
            if wrong == "swapped_uv":
                u, v = v, u
            return _le(np.abs(u), p[2], wrong) & _le(np.abs(v), p[3], wrong)
        if kind == "disc":
            cx, cy, R = p[0], p[1], p[2]
        else:
            ex = p[2] - p[0]
            ey = p[3] - p[1]
            l2 = ex * ex + ey * ey
            t = np.zeros_like(x) if l2 == 0.0 else ((x - p[0]) * ex + (y - p[1]) * ey) / l2
            if wrong != "unclamped_t":
                t = np.where(t < 0.0, 0.0, t)
                t = np.where(t > 1.0, 1.0, t)
            cx = p[0] + t * ex
            cy = p[1] + t * ey
            R = p[4]
        dx = x - cx
        dy = y - cy
        d2 = dx * dx + dy * dy
        return _le(d2, R * R, wrong)


def _quantise(v, wrong):
    """(ok, Python ints) of the coordinates v scaled by 2^16: round to nearest, ties to even"""
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.asarray(v, dtype=np.float64) * SCALE
        ok = np.abs(f) < LIMIT  # (false for a NaN and for an infinity)
        g = np.where(ok, f, 0.0)
        q = np.trunc(g) if wrong == "truncation" else np.rint(g)
    return ok, [int(e) for e in q]


def read(sensors, xs, ys, wrong=None, eps=1e-8):
    """`(sums, dropped)` as SimulationHandler.sensor_sums returns them, for xs = (white x, yolk x), ys likewise"""
    sums, dropped, _ = _measure(sensors, xs, ys, wrong, eps)
    return sums, dropped


def _measure(sensors, xs, ys, wrong, eps):
    canon = canonical(sensors, eps, wrong)
    dropped = [0, 0]
    sums = []
    kept = []  # [sensor][type] bool array: the particles that count
    quant = []
    for w in (0, 1):
        okx, qx = _quantise(xs[w], wrong)
        oky, qy = _quantise(ys[w], wrong)
        quant.append((okx & oky, qx, qy))
    for sensor in canon:
        per_type, kept_k = [], []
        for w in (0, 1):
            ok, qx, qy = quant[w]
            if sensor[1] >> w & 1 or wrong == "ignored_mask":
                ins = inside(sensor, xs[w], ys[w], wrong)
            else:
                ins = np.zeros(np.asarray(xs[w]).shape, dtype=bool)
            keep = ins & ok
            dropped[w] += int(np.count_nonzero(ins & ~ok))
            count = int(np.count_nonzero(ins if wrong == "drop_counts" else keep))
            idx = np.flatnonzero(keep)
            per_type.append((count, sum(qx[i] for i in idx), sum(qy[i] for i in idx)))
            kept_k.append(keep)
        sums.append(tuple(per_type))
        kept.append(kept_k)
    return sums, dropped, kept


def read_batches(sensors, xs, ys, batch_ids, ids, wrong=None, eps=1e-8):
    """int32 [len(ids), n_sensors, 2] as SimulationHandler.sensor_batches returns it; batch_ids = (white, yolk) per-particle ids"""
    _, _, kept = _measure(sensors, xs, ys, wrong, eps)
    out = np.zeros((len(ids), len(kept), 2), dtype=np.int32)
    for i, gid in enumerate(ids):
        for k, kept_k in enumerate(kept):
            for w in (0, 1):
                out[i, k, w] = np.count_nonzero(kept_k[w] & (np.asarray(batch_ids[w]) == gid))
    return out


def readings(sums):
    """per sensor {"count": (white, yolk), "centroid": (white, yolk)} as SimulationHandler.sensors returns it"""
    return [{"count": tuple(c for c, _, _ in per_type),
             "centroid": tuple(((float(sx) / SCALE) / float(c), (float(sy) / SCALE) / float(c)) if c else None
                               for c, sx, sy in per_type)} for per_type in sums]
