"""The rule of the fields (include/eggsim.h, "fields") in numpy float64 and Python ints: the
definition the device kernel (csrc/eggsim_fields.hip) is held against.

A grid is `(x0, y0, cell, nx, ny)`: nx x ny square cells of side `cell`, cell (0, 0) with its lower corner at (x0, y0).
For a particle of type w whose bit is in the mask, at (x, y) with velocity (vx, vy), numpy float64 element-wise in exactly
this order:
    inv = 1.0 / cell (once);  fx = (x - x0) * inv;  fy = (y - y0) * inv
    inside iff fx >= 0.0 and fx < nx and fy >= 0.0 and fy < ny        (every comparison is false for a NaN)
    ix = trunc(fx), iy = trunc(fy) (-0.0 is cell 0); the planes are [2][ny][nx], row-major: plane[w][iy][ix]
    outside:  outside[w] += 1 and nothing else
    dropped:  inside, velocities requested, and vx * 2^16 or vy * 2^16 not finite or >= 2^53 in magnitude: dropped[w] += 1
    counted:  inside[w] += 1, count[w][iy][ix] += 1, svx[w][iy][ix] += rint(vx * 2^16), svy likewise (int64, ties to even)
Without velocities nothing is dropped and svx, svy are None.  Written from the header's text alone; it shares no code
with the library.

`wrong` names ONE deliberately wrong rule (tests/test_field_model.py: a table case must tell each from the right one).
"""
import math

import numpy as np

SCALE = 65536.0
LIMIT = 2.0 ** 53
MAX_CELLS = 1 << 20
MASKS = {"white": 1, "yolk": 2, "both": 3}
WRONG_RULES = ("rounding", "closed_upper_edge", "swapped_xy", "column_major", "ignored_mask", "drop_counts", "division")


def check_grid(x0, y0, cell, nx, ny):
    """ValueError for a grid egg_field refuses"""
    if nx < 1 or ny < 1 or nx * ny > MAX_CELLS:
        raise ValueError("nx, ny")
    if not (math.isfinite(cell) and cell > 0.0 and math.isfinite(1.0 / cell)):
        raise ValueError("cell")
    if not (math.isfinite(x0) and math.isfinite(y0)):
        raise ValueError("x0, y0")


def cells(grid, x, y, wrong=None):
    """(inside, ix, iy) of the positions: a bool array and two int64 arrays (0 where outside)"""
    x0, y0, cell, nx, ny = grid
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if wrong == "swapped_xy":
        x, y = y, x
    with np.errstate(invalid="ignore", over="ignore"):
        if wrong == "division":
            fx, fy = (x - np.float64(x0)) / np.float64(cell), (y - np.float64(y0)) / np.float64(cell)
        else:
            inv = np.float64(1.0) / np.float64(cell)
            fx, fy = (x - np.float64(x0)) * inv, (y - np.float64(y0)) * inv
        if wrong == "closed_upper_edge":
            inside = (fx >= 0.0) & (fx <= float(nx)) & (fy >= 0.0) & (fy <= float(ny))
        else:
            inside = (fx >= 0.0) & (fx < float(nx)) & (fy >= 0.0) & (fy < float(ny))
        sx, sy = np.where(inside, fx, 0.0), np.where(inside, fy, 0.0)
        if wrong == "rounding":
            ix, iy = np.rint(sx).astype(np.int64), np.rint(sy).astype(np.int64)
        else:
            ix, iy = np.trunc(sx).astype(np.int64), np.trunc(sy).astype(np.int64)
    if wrong in ("closed_upper_edge", "rounding"):  # (a wrong rule still has to land in a plane)
        ix, iy = np.minimum(ix, nx - 1), np.minimum(iy, ny - 1)
    return inside, ix, iy


def field(grid, xs, ys, vxs=None, vys=None, types="both", velocity=False, wrong=None):
    """(count, svx, svy, inside, outside, dropped) of per-type arrays xs = [white x, yolk x] etc.: int32 / int64 planes of
    shape (2, ny, nx) (svx, svy None without velocity) and three (white, yolk) tuples of Python ints"""
    x0, y0, cell, nx, ny = grid
    check_grid(x0, y0, cell, nx, ny)
    mask = types if isinstance(types, int) else MASKS[types]
    if wrong == "ignored_mask":
        mask = 3
    count = np.zeros((2, ny, nx), dtype=np.int32)
    svx = np.zeros((2, ny, nx), dtype=np.int64) if velocity else None
    svy = np.zeros((2, ny, nx), dtype=np.int64) if velocity else None
    n_in, n_out, n_drop = [0, 0], [0, 0], [0, 0]
    for w in (0, 1):
        if not mask >> w & 1:
            continue
        inside, ix, iy = cells(grid, xs[w], ys[w], wrong)
        n_out[w] = int((~inside).sum())
        keep = inside
        qx = qy = None
        if velocity:
            with np.errstate(invalid="ignore", over="ignore"):
                fx = np.asarray(vxs[w], dtype=np.float64) * SCALE
                fy = np.asarray(vys[w], dtype=np.float64) * SCALE
                ok = (np.abs(fx) < LIMIT) & (np.abs(fy) < LIMIT)  # (false for a NaN and for an infinity)
                qx = np.rint(np.where(ok, fx, 0.0)).astype(np.int64)
                qy = np.rint(np.where(ok, fy, 0.0)).astype(np.int64)
            n_drop[w] = int((inside & ~ok).sum())
            if wrong != "drop_counts":
                keep = inside & ok
        n_in[w] = int(keep.sum())
        at = (iy[keep], ix[keep]) if wrong != "column_major" else _column_major(iy[keep], ix[keep], nx, ny)
        np.add.at(count[w], at, 1)
        if velocity:
            np.add.at(svx[w], at, qx[keep])
            np.add.at(svy[w], at, qy[keep])
    return count, svx, svy, tuple(n_in), tuple(n_out), tuple(n_drop)


def _column_major(iy, ix, nx, ny):
    """the cell of a plane laid out [nx][ny], read back as [ny][nx]"""
    flat = ix * ny + iy
    return flat // nx, flat % nx


def velocity(count, svx, svy):
    """(2, ny, nx, 2) doubles: ((double)svx / 2^16) / (double)count and likewise for y, NaN where the count is 0"""
    out = np.full(count.shape + (2,), np.nan)
    for idx in zip(*np.nonzero(count)):
        n = float(int(count[idx]))
        out[idx + (0,)] = (float(int(svx[idx])) / SCALE) / n
        out[idx + (1,)] = (float(int(svy[idx])) / SCALE) / n
    return out
