/* eggsim_measure.h -- the measures of libeggsim.so: three entry points, their spec and their record.  Part of the C ABI of
 * include/eggsim.h, which includes this file at its end beside eggsim_impulse.h; it is not meant to be included alone.  The
 * main header's section list stands at 173 entry points, eggsim_impulse.h adds two; with these three the library exports 178. */
#ifndef EGGSIM_MEASURE_H
#define EGGSIM_MEASURE_H
#ifndef EGGSIM_H
#error "include eggsim.h, which brings this header along"
#endif

/* ---- measures: per-batch mass, momentum, energy, extent and shape (csrc/eggsim_measures.hip) ----
 * Not in the reference.  What is this egg doing, as a body: per requested batch and particle type (an ATOM, as in pieces) one
 * record of 24 int64.  A call is STATELESS and READ-ONLY: it reads the committed x, y, vx, vy, radius, inv_mass -- the arrays
 * egg_download_particles returns -- in either solver order, stores nothing and changes nothing.  tests/measure_model.py is
 * the definition in numpy.  FP64 in exactly this order, no contraction, sqrt and / correctly rounded; every comparison is
 * false for a NaN.
 * Constants.  S = EGG_MEASURE_SCALE = 2^16, SM = EGG_MEASURE_MASS_SCALE = 2^32, LIM = 2^53.  q(v) = llrint(v) (int64, round to
 * nearest, ties to even), taken only after fabs(v) < LIM has been checked.  The mass of a particle is m = 1.0 / inv_mass.
 * Which particles.  A particle of type w of a requested batch is MEASURED when spec.type_mask has bit w and, if spec.flags
 * has EGG_MEASURE_REGION, the region's test holds: `region` is an egg_sensor, checked and normalised per call by the rule
 * egg_set_sensors uses, the test is the sensors' own with the region's type mask included.  Without the flag the region is
 * ignored and need not be valid.
 * Pass 1.  The terms of a measured particle: x*S, y*S, m*SM, (m*x)*S, (m*y)*S, (m*vx)*S, (m*vy)*S, with
 * v2 = vx*vx + vy*vy then (m*v2)*S and v2*S, and (x - radius)*S, (y - radius)*S, (x + radius)*S, (y + radius)*S.  The
 * particle is KEPT iff every one of these thirteen terms is below LIM in magnitude; otherwise it counts in `dropped` and
 * contributes to nothing.
 * Pass 2 needs pass 1 of the whole atom.  kept = n - dropped.  ox_q = sx / kept, oy_q = sy / kept as C int64 division
 * (truncation toward zero); ox = (double)ox_q / S, oy likewise: both exact.  For a kept particle dx = x - ox, dy = y - oy,
 * d2 = dx*dx + dy*dy; the terms: (dx*dx)*S, (dx*dy)*S, (dy*dy)*S, (m*(dx*vy - dy*vx))*S, (sqrt(d2) + radius)*S.  A kept
 * particle with any of these five at or beyond LIM counts in `dropped_central` and contributes to no pass-2 field.
 * The record (out[i][0] the white of id i, out[i][1] its yolk):
 *    0 atom             particles of the atom, regardless of the region
 *    1 n                measured particles
 *    2 dropped          measured but not kept
 *    3, 4 sx, sy        sums of q(x*S), q(y*S) over the kept
 *    5 sm               sum of q(m*SM)
 *    6, 7 smx, smy      sums of q((m*x)*S), q((m*y)*S)
 *    8, 9 spx, spy      sums of q((m*vx)*S), q((m*vy)*S): the momentum
 *   10 se               sum of q((m*v2)*S): twice the kinetic energy
 *   11 - 14 lo_x, lo_y, hi_x, hi_y   min q((x-r)*S), min q((y-r)*S), max q((x+r)*S), max q((y+r)*S)
 *   15 max_v2           max q(v2*S)
 *   16, 17 ox_q, oy_q   the origin of pass 2
 *   18 dropped_central
 *   19 - 21 sxx, sxy, syy   sums of q((dx*dx)*S), q((dx*dy)*S), q((dy*dy)*S)
 *   22 sl               sum of q((m*(dx*vy - dy*vx))*S): the angular momentum about the origin
 *   23 max_reach        max q((sqrt(d2)+r)*S)
 * Extremes are taken on the quantised integers, never on doubles; sums are two's complement int64.  With kept == 0 the
 * fields 3 to 23 are 0; with kept == dropped_central the fields 19 to 23 are 0.  For a type the mask leaves out, or one the
 * batch lacks, the whole record is 0.  Every output is an integer and every sum is order-free: the answer does not depend
 * on the schedule, on the device, or on how a scene is split over handles.
 * n_ids = 0 with ids = NULL means every live batch in egg_list_ids order; an id may repeat; n_ids = 0 with a list asks for
 * nothing.  Everything is checked before anything is launched or written: EGG_ERR_INVALID_ARGUMENT for a NULL spec or out,
 * n_ids < 0, ids NULL with n_ids > 0, unknown flag bits, a type_mask outside 1 .. 3, anything the region's check refuses
 * when the flag is set, a step in flight (egg_step_begin or egg_rx_begin open); EGG_ERR_UNKNOWN_ID for an unknown id.  A
 * handle without particles, or an empty id list, succeeds and launches nothing.  Of egg_get_stats only kernel_launches
 * moves, by at most 1 per call.
 * Limits: no per-region measure without a batch list; no measure that rides on a collider; one region per call; per type
 * only: white and yolk are combined from the integers by the caller. */
#define EGG_MEASURE_SCALE 65536.0            /* 2^16 */
#define EGG_MEASURE_MASS_SCALE 4294967296.0  /* 2^32 */
#define EGG_MEASURE_FIELDS 24
enum { EGG_MEASURE_REGION = 1 };   /* flag bits */
typedef struct { egg_sensor region; int32_t flags, type_mask; } egg_measure_spec;   /* 64 bytes */
typedef struct {
    int64_t atom, n, dropped, sx, sy, sm, smx, smy, spx, spy, se, lo_x, lo_y, hi_x, hi_y, max_v2, ox_q, oy_q, dropped_central,
        sxx, sxy, syy, sl, max_reach;
} egg_measure_record;   /* 192 bytes */
int egg_measure(egg_handle *h, const egg_measure_spec *spec, int64_t n_ids, const int64_t *ids, egg_measure_record *out /* host [n][2] */);

/* egg_measure into memory of the handle's device -- a torch int64 tensor [n, 2, 24], say -- : the table is complete when
 * the call returns and nothing is copied back.  EGG_ERR_INVALID_ARGUMENT for a pointer that is NULL, not aligned to 8 bytes,
 * not memory of the handle's device, or an allocation that does not hold n * 2 * 192 bytes from it on, and for a
 * capacity_bytes below that; a refused call leaves the memory untouched. */
int egg_measure_to(egg_handle *h, const egg_measure_spec *spec, int64_t n_ids, const int64_t *ids, void *device_out, int64_t capacity_bytes);

/* egg_measure for a device group: ids are the group's, every id is routed to the handle that owns the batch and that
 * handle's records are copied to the caller's rows: one handle's table, bit for bit.  Every handle checks the spec, and
 * the ids are checked, before anything is written. */
int egg_group_measure(egg_group *g, const egg_measure_spec *spec, int64_t n_ids, const int64_t *ids, egg_measure_record *out);

#endif
