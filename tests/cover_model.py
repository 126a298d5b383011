"""The cover (egg_cover; include/eggsim_cover.h) in numpy: the rule of the header, word for word, over
downloaded x, y, radius and batch_id.  Every operation is an IEEE double operation in the header's order, so the integers
are the device's.  `cover(...)` tests the rectangle the kernel tests; `cover(..., full=True)` tests every cell of the grid
for every inside disc, which is what the answer is defined as."""
import numpy as np

MAX_SPAN = 64.0  # EGG_COVER_MAX_SPAN
MAX_CELLS = 1 << 20  # EGG_COVER_MAX_CELLS
MASKS = {"white": 1, "yolk": 2, "both": 3, 1: 1, 2: 2, 3: 3}


def refused(grid):
    """the header's resolution refusal: !(max(|x0|, |y0|, |x0 + nx*cell|, |y0 + ny*cell|) <= cell * 0x1p20)"""
    x0, y0, cell, nx, ny = grid
    x0, y0, cell = np.float64(x0), np.float64(y0), np.float64(cell)
    reach = max(abs(x0), abs(y0), abs(x0 + np.float64(nx) * cell), abs(y0 + np.float64(ny) * cell))
    return not (reach <= cell * np.float64(2.0 ** 20))


def fate(grid, scale, x, y, radius):
    """per particle: 0 inside, 1 outside, 2 dropped; and R, fxl, fxh, fyl, fyh (meaningless where dropped)"""
    x0, y0, cell, nx, ny = grid
    x0, y0, cell = np.float64(x0), np.float64(y0), np.float64(cell)
    inv = np.float64(1.0) / cell
    x, y, radius = (np.asarray(v, dtype=np.float64) for v in (x, y, radius))
    with np.errstate(all="ignore"):
        R = np.float64(scale) * radius
        dropped = ~(np.isfinite(x) & np.isfinite(y)) | ~(R >= 0.0) | ~(R * inv <= MAX_SPAN)
        fxl, fxh = ((x - R) - x0) * inv, ((x + R) - x0) * inv
        fyl, fyh = ((y - R) - y0) * inv, ((y + R) - y0) * inv
        outside = (fxh < 0.0) | (fxl >= np.float64(nx)) | (fyh < 0.0) | (fyl >= np.float64(ny))
    return np.where(dropped, 2, np.where(outside, 1, 0)), R, fxl, fxh, fyl, fyh


def cover(grid, scale, x, y, radius, batch_id, types="both", owner=True, full=False):
    """(cover int32 [2][ny][nx], owner int32 [2][ny][nx] or None, inside, outside, dropped, hits, covered, covered_both,
    covered_any) of per-type lists x, y, radius, batch_id (index 0 white, 1 yolk)"""
    x0, y0, cell, nx, ny = grid
    x0, y0, cell = np.float64(x0), np.float64(y0), np.float64(cell)
    mask = MASKS[types]
    plane = np.zeros((2, ny, nx), dtype=np.int64)
    own = np.full((2, ny, nx), -1, dtype=np.int64)
    inside, outside, dropped, hits = [0, 0], [0, 0], [0, 0], [0, 0]
    cx = x0 + (np.arange(nx, dtype=np.float64) + 0.5) * cell
    cy = y0 + (np.arange(ny, dtype=np.float64) + 0.5) * cell
    for w in (0, 1):
        if not mask >> w & 1:
            continue
        px, py = np.asarray(x[w], dtype=np.float64), np.asarray(y[w], dtype=np.float64)
        ids = np.asarray(batch_id[w]).astype(np.int64)
        f, R, fxl, fxh, fyl, fyh = fate(grid, scale, px, py, radius[w])
        inside[w], outside[w], dropped[w] = int((f == 0).sum()), int((f == 1).sum()), int((f == 2).sum())
        for k in np.nonzero(f == 0)[0]:
            if full:
                ix0, ix1, iy0, iy1 = 0, nx - 1, 0, ny - 1
            else:  # clamped in double before the conversion
                ix0, ix1 = int(np.floor(max(fxl[k], 0.0))), int(np.floor(min(fxh[k], np.float64(nx - 1))))
                iy0, iy1 = int(np.floor(max(fyl[k], 0.0))), int(np.floor(min(fyh[k], np.float64(ny - 1))))
            dx, dy = cx[ix0:ix1 + 1] - px[k], cy[iy0:iy1 + 1] - py[k]
            with np.errstate(all="ignore"):
                hit = (dx * dx)[None, :] + (dy * dy)[:, None] <= R[k] * R[k]
            hits[w] += int(hit.sum())
            plane[w, iy0:iy1 + 1, ix0:ix1 + 1] += hit
            part = own[w, iy0:iy1 + 1, ix0:ix1 + 1]
            part[hit & ((part < 0) | (part > ids[k]))] = ids[k]
    a, b = plane[0] > 0, plane[1] > 0
    return (plane.astype(np.int32), own.astype(np.int32) if owner else None, tuple(inside), tuple(outside), tuple(dropped), tuple(hits),
            (int(a.sum()), int(b.sum())), int((a & b).sum()), int((a | b).sum()))


def same(a, b):
    """two answers (tuples as cover() returns, possibly cut short) are equal, planes by value"""
    if len(a) != len(b):
        return False
    for u, v in zip(a, b):
        if u is None or v is None:
            if u is not v:
                return False
        elif isinstance(u, np.ndarray) or isinstance(v, np.ndarray):
            if not np.array_equal(u, v):
                return False
        elif tuple(u) != tuple(v) if isinstance(u, (tuple, list)) else u != v:
            return False
    return True
