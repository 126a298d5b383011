"""The rule of the impulses (include/eggsim_impulse.h) in numpy float64 and Python ints: the
definition the device kernel (csrc/eggsim_impulses.hip) is held against.

A record is `(action, region, params[, options])`:
  action   "kick" (ax, ay) | "blast" (cx, cy, s) | "swirl" (cx, cy, omega) | "brake" (ux, uy, k)
  region   a sensor region as the Python wrapper takes it (tests/sensor_model.py): checked and normalised per call
  options  a dict of `id` (None: every batch), `linear`, `by_inv_mass`
A particle of type w at the committed (x, y) is IN record k when the region's test holds, its mask has bit w and id is None or
the particle's batch.  w = 1.0; with linear w = 1.0 - sqrt(d2) / R with the test's own d2 and R, below 0.0 it is 0.0; with
by_inv_mass w = w * inv_mass.  The action gives (nvx, nvy) from the velocity the record finds, which is what the record before
it left; dvx = nvx - vx, fx = dvx * 2^16 and likewise y; the edit is accepted iff |fx| < 2^53 and |fy| < 2^53: then v = nv,
count += 1, sdvx += llrint(fx), sdvy += llrint(fy); otherwise the velocity stays and skipped += 1.  numpy float64 element-wise
in exactly this order (numpy never contracts a product into a sum; sqrt and / are correctly rounded); every comparison is
false for a NaN.  Written from the header's text alone; it shares no code with the library.
"""
import math

import numpy as np

import sensor_model

SCALE = 65536.0
LIMIT = 2.0 ** 53
MAX_IMPULSES = 64
ACTIONS = ("kick", "blast", "swirl", "brake")
N_PARAMS = {"kick": 2, "blast": 3, "swirl": 3, "brake": 3}


def canonical(records, eps=1e-8, known_ids=None):
    """the list as egg_impulse applies it: [(action, region, [3 parameters], id or None, linear, by_inv_mass)] with the region
    canonical; ValueError("record k: ...") for a list it refuses, KeyError for an unknown id (known_ids given)"""
    records = list(records)
    if len(records) > MAX_IMPULSES:
        raise ValueError("a call takes 0 .. %d records" % MAX_IMPULSES)
    out = []
    for k, r in enumerate(records):
        r = tuple(r)
        opts = dict(r[-1]) if r and isinstance(r[-1], dict) else {}
        if opts:
            r = r[:-1]
        action, region = r[0], r[1]
        a = tuple(r[2]) if len(r) == 3 and isinstance(r[2], (tuple, list)) else tuple(r[2:])
        if action not in ACTIONS:
            raise ValueError("record %d: unknown action %r" % (k, action))
        if set(opts) - {"id", "linear", "by_inv_mass"}:
            raise ValueError("record %d: unknown options" % k)
        try:
            sensor = sensor_model.canonical([region], eps)[0]
        except ValueError as e:
            raise ValueError("record %d: %s" % (k, e)) from None
        linear, by_inv_mass, gid = bool(opts.get("linear", False)), bool(opts.get("by_inv_mass", False)), opts.get("id")
        if linear:
            R = {"disc": sensor[2][2], "capsule": sensor[2][4]}.get(sensor[0])
            if R is None or not R > 0.0:
                raise ValueError("record %d: the linear weight is for a disc or a capsule with R > 0" % k)
        if by_inv_mass and action in ("swirl", "brake"):
            raise ValueError("record %d: the weight by inverse mass is for a kick or a blast" % k)
        if len(a) != N_PARAMS[action]:
            raise ValueError("record %d (%s): %d parameters" % (k, action, len(a)))
        a = [float(v) for v in a] + [0.0] * (3 - len(a))
        if not all(math.isfinite(v) for v in a):
            raise ValueError("record %d (%s): a parameter is not finite" % (k, action))
        if action == "brake" and not 0.0 <= a[2] <= 1.0:
            raise ValueError("record %d (brake): k outside [0, 1]" % k)
        if gid is not None and known_ids is not None and gid not in known_ids:
            raise KeyError("record %d: no batch with id %r" % (k, gid))
        out.append((action, sensor, a, gid, linear, by_inv_mass))
    return out


def _test(sensor, x, y):
    """(inside, d2, R) of one canonical region for the positions: d2 and R are the test's own for a disc and a capsule"""
    kind, _mask, p = sensor
    if kind in ("half_plane", "box"):
        return sensor_model.inside(sensor, x, y), None, None
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == "disc":
            cx, cy, R = p[0], p[1], p[2]
        else:
            ex = p[2] - p[0]
            ey = p[3] - p[1]
            l2 = ex * ex + ey * ey
            t = np.zeros_like(x) if l2 == 0.0 else ((x - p[0]) * ex + (y - p[1]) * ey) / l2
            t = np.where(t < 0.0, 0.0, t)
            t = np.where(t > 1.0, 1.0, t)
            cx = p[0] + t * ex
            cy = p[1] + t * ey
            R = p[4]
        dx = x - cx
        dy = y - cy
        d2 = dx * dx + dy * dy
        return d2 <= R * R, d2, R


def apply(records, x, y, vx, vy, inv_mass, batch_ids, eps=1e-8, known_ids=None):
    """Apply the list to both types.  Every argument but the list is a (white, yolk) pair of arrays; batch_ids the id of every
    particle's batch.  Returns `(nvx, nvy, results)`: the new velocities as a (white, yolk) pair of fresh float64 arrays and
    per record `((count_w, count_y), (sdvx_w, sdvx_y), (sdvy_w, sdvy_y), (skipped_w, skipped_y))` in Python ints.  The
    inputs are not changed."""
    canon = canonical(records, eps, known_ids)
    out_vx = [np.array(v, dtype=np.float64, copy=True) for v in vx]
    out_vy = [np.array(v, dtype=np.float64, copy=True) for v in vy]
    results = []
    for action, sensor, a, gid, linear, by_inv_mass in canon:
        res = [[0, 0], [0, 0], [0, 0], [0, 0]]
        for t in (0, 1):
            px = np.asarray(x[t], dtype=np.float64)
            py = np.asarray(y[t], dtype=np.float64)
            if not (sensor[1] >> t & 1) or px.size == 0:
                continue
            cvx, cvy = out_vx[t], out_vy[t]
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                ins, d2, R = _test(sensor, px, py)
                if gid is not None:
                    ins = ins & (np.asarray(batch_ids[t]) == gid)
                w = np.ones_like(px)
                if linear:
                    w = 1.0 - np.sqrt(d2) / R
                    w = np.where(w < 0.0, 0.0, w)
                if by_inv_mass:
                    w = w * np.asarray(inv_mass[t], dtype=np.float64)
                if action == "kick":
                    nvx = cvx + w * a[0]
                    nvy = cvy + w * a[1]
                elif action == "brake":
                    g = w * a[2]
                    nvx = cvx + g * (a[0] - cvx)
                    nvy = cvy + g * (a[1] - cvy)
                else:
                    dx = px - a[0]
                    dy = py - a[1]
                    if action == "blast":
                        b2 = dx * dx + dy * dy
                        ins = ins & (b2 > 0.0)
                        g = (w * a[2]) / np.sqrt(b2)
                        nvx = cvx + g * dx
                        nvy = cvy + g * dy
                    else:
                        g = w * a[2]
                        nvx = cvx - g * dy
                        nvy = cvy + g * dx
                dvx = nvx - cvx
                dvy = nvy - cvy
                fx = dvx * SCALE
                fy = dvy * SCALE
                ok = (np.abs(fx) < LIMIT) & (np.abs(fy) < LIMIT)  # (false for a NaN and for an infinity)
                take = ins & ok
                qx = np.rint(np.where(take, fx, 0.0))
                qy = np.rint(np.where(take, fy, 0.0))
            res[0][t] = int(np.count_nonzero(take))
            res[1][t] = sum(int(e) for e in qx[take])
            res[2][t] = sum(int(e) for e in qy[take])
            res[3][t] = int(np.count_nonzero(ins & ~ok))
            out_vx[t] = np.where(take, nvx, cvx)
            out_vy[t] = np.where(take, nvy, cvy)
        results.append(tuple(tuple(r) for r in res))
    return tuple(out_vx), tuple(out_vy), results
