/* eggsim_cover.h -- the cover of libeggsim.so: three entry points, their spec, their planes and their totals.  Part of the C
 * ABI of include/eggsim.h, which includes this file at its end beside eggsim_impulse.h and eggsim_measure.h; it is not meant
 * to be included alone.  The main header's section list stands at 173 entry points, eggsim_impulse.h adds two,
 * eggsim_measure.h three; with these three the library exports 181. */
#ifndef EGGSIM_COVER_H
#define EGGSIM_COVER_H
#ifndef EGGSIM_H
#error "include eggsim.h, which brings this header along"
#endif

/* ---- cover: the particles' discs rastered into a grid -- area, depth, owner map (csrc/eggsim_cover.hip) ----
 * Not in the reference.  How much floor is covered, how deep, and by which egg: per cell and particle type the number of
 * discs that cover the cell's CENTRE and, on request, the oldest batch among them.  A call is STATELESS and READ-ONLY: it
 * reads the committed x, y, radius -- the arrays egg_download_particles returns -- in either solver order, stores nothing
 * and changes nothing.  tests/cover_model.py is the definition in numpy.
 * The grid: nx x ny square cells of side `cell`, the lower corner of cell (0, 0) at (x0, y0).  FP64 in exactly this order,
 * no contraction; every comparison is false for a NaN.
 * Once per call: inv = 1.0 / cell.  Cell centres: cx(ix) = x0 + ((double)ix + 0.5) * cell, cy(iy) = y0 + ((double)iy + 0.5) * cell.
 * Per particle of type w in type_mask, with committed (x, y) and radius:
 *   R = scale * radius.
 *   DROPPED iff !(isfinite(x) && isfinite(y)), or !(R >= 0.0), or !(R * inv <= EGG_COVER_MAX_SPAN): dropped[w] += 1,
 *   nothing else.  (A disc spans at most 130 x 130 cells.)
 *   Otherwise fxl = ((x - R) - x0) * inv, fxh = ((x + R) - x0) * inv, and fyl, fyh likewise.
 *   OUTSIDE iff fxh < 0.0 || fxl >= (double)nx || fyh < 0.0 || fyl >= (double)ny: outside[w] += 1, nothing else.
 *   Otherwise INSIDE: inside[w] += 1, and for EVERY cell (ix, iy) of the grid: dx = cx(ix) - x, dy = cy(iy) - y,
 *   d2 = dx*dx + dy*dy; the cell is covered iff d2 <= R*R.  Each covered cell: cover[w][iy][ix] += 1, hits[w] += 1,
 *   owner[w][iy][ix] = min(owner, batch id).
 * The answer is defined over every cell; the kernel tests only the rectangle ix in [floor(max(fxl, 0)), floor(min(fxh, nx-1))]
 * and iy likewise, clamped in double before the conversion to int.  That rectangle is conservative by half a cell while the
 * grid resolves its own coordinates, so a call refuses a grid with
 *   !(max(|x0|, |y0|, |x0 + nx*cell|, |y0 + ny*cell|) <= cell * 0x1p20).
 * Planes, each [2][ny][nx], row-major, [0] white and [1] yolk: `cover` int32, required; `owner` int32, optional (NULL: not
 * asked for): the smallest batch id among the covering discs of that type, -1 where there is none (an unsigned minimum over
 * a plane preset to 0xFFFFFFFF).  A handle whose largest live id does not fit 31 bits refuses `owner`.
 * Totals: covered[w] the cells with cover[w] > 0, covered_both the cells where both types are above 0, covered_any where
 * either is; inside + outside + dropped is the particles of each covered type.  Area is covered * cell * cell, mean depth
 * hits / covered.  covered, covered_both and covered_any are NOT ADDITIVE across handles: a group and sharded ranks recount
 * them from the merged planes.  units_lanes, units_wave, units_direct say how the device did the work; they are not part of
 * the answer.  Every output is an integer and every sum and minimum is order-free: the answer does not depend on the
 * schedule, on the device, or on how a scene is split over handles.
 * spec.scale is finite and above 0 (1: the simulated discs; 12: the discs as they are drawn).  spec.path: EGG_COVER_PATH_AUTO,
 * or one of the test hooks _DIRECT, _LANES, _WAVE; the planes are equal on every path.  The flag EGG_COVER_OWNER_KEYS, or-ed
 * into spec.path, makes `owner` hold the batches' KEYS (egg_batch_info.key: the position in the creation order, which a group
 * and sharded ranks use as the id of the whole scene) in place of the handle's ids, under the same 31-bit refusal: minima
 * over keys merge across handles, minima over a handle's own ids do not.
 * Everything is checked before anything is launched or written: EGG_ERR_INVALID_ARGUMENT for a NULL spec or planes, nx or
 * ny below 1 or nx * ny above EGG_COVER_MAX_CELLS, a cell or a scale that is not finite and above 0 (the cell's inverse is
 * finite too), an origin that is not finite, a type_mask outside 1 .. 3, an unknown path, a NULL cover, a grid that does
 * not resolve its coordinates, an owner plane with an id beyond 31 bits, a step in flight (egg_step_begin or egg_rx_begin
 * open).  A scene without covered particles fills cover with 0 and owner with -1 and launches nothing.  Of egg_get_stats
 * only kernel_launches moves, by at most 2 per call.
 * Limits: the cell's centre decides (no anti-aliased or fractional coverage); not the drawn density texture or its
 * threshold; no mass or velocity planes by disc; no per-batch planes beyond owner; no cover that rides on a collider, and
 * no colliders in the map. */
#define EGG_COVER_MAX_CELLS (1 << 20)   /* nx * ny */
#define EGG_COVER_MAX_SPAN 64.0         /* R * inv */
enum { EGG_COVER_PATH_AUTO = 0, EGG_COVER_PATH_DIRECT = 1, EGG_COVER_PATH_LANES = 2, EGG_COVER_PATH_WAVE = 3 };
enum { EGG_COVER_OWNER_KEYS = 0x100 };   /* flag bit of spec.path */
typedef struct { double x0, y0, cell, scale; int32_t nx, ny, type_mask, path; } egg_cover_spec;   /* 48 bytes */
typedef struct { int32_t *cover; int32_t *owner; } egg_cover_planes;   /* 16 bytes */
typedef struct {
    int64_t inside[2], outside[2], dropped[2], hits[2], covered[2], covered_both, covered_any;
    int32_t units_lanes, units_wave, units_direct, reserved;
} egg_cover_totals;   /* 112 bytes */
int egg_cover(egg_handle *h, const egg_cover_spec *spec, const egg_cover_planes *host_planes, egg_cover_totals *totals);

/* egg_cover into planes of the handle's device -- torch int32 tensors [2, ny, nx], say -- : the call zeroes `cover` and
 * presets `owner` itself, the planes are complete when it returns and only the totals are copied back.
 * EGG_ERR_INVALID_ARGUMENT for a plane that is not aligned to 4 bytes, not memory of the handle's device, or an allocation
 * that does not hold 2 * ny * nx * 4 bytes from it on; a refused call leaves the memory untouched. */
int egg_cover_to(egg_handle *h, const egg_cover_spec *spec, const egg_cover_planes *device_planes, egg_cover_totals *totals);

/* egg_cover for a device group: the same grid goes to every handle; the cover planes and the additive totals are added,
 * the owner planes -- taken with EGG_COVER_OWNER_KEYS: a batch's key is the group's id -- merged by unsigned minimum, and covered, covered_both,
 * covered_any recounted from the merged planes: one handle's answer, bit for bit.  Nothing is written before every handle
 * has answered. */
int egg_group_cover(egg_group *g, const egg_cover_spec *spec, const egg_cover_planes *host_planes, egg_cover_totals *totals);

#endif
