/* eggsim_touch.h -- the touches of libeggsim.so: three entry points, their spec, their query and their record.  Part of the C
 * ABI of include/eggsim.h, which includes this file at its end, after eggsim_cover.h; it is not meant to be included alone.
 * The main header's section list stands at 173 entry points, eggsim_impulse.h adds two, eggsim_measure.h three,
 * eggsim_cover.h three; with these three the library exports 184. */
#ifndef EGGSIM_TOUCH_H
#define EGGSIM_TOUCH_H
#ifndef EGGSIM_H
#error "include eggsim.h, which brings this header along"
#endif

/* ---- touches: which eggs touch which, how much and where (csrc/eggsim_touches.hip) ----
 * Not in the reference as a call; the predicate is the one of its collision branch (L:1632-1653).  A call is STATELESS and
 * READ-ONLY: it reads the committed x, y, radius -- the arrays egg_download_particles returns -- in either solver order,
 * stores no answer and changes nothing.  tests/touch_model.py is the definition in numpy.
 * A QUERY is a set of discs (x, y, r) of one type with a key: the atom (the particles of one type) of a listed batch, its
 * discs read on the device and its key the batch's id; or discs the caller hands in (egg_touches_of).
 * Particle a of a query and particle b of the SAME type in a batch whose id (or key) differs from the query's key TOUCH iff
 * d2 <= L * L.  FP64 in exactly this order, no contraction; the test is false when anything in it is a NaN:
 *   dx = xa - xb; dy = ya - yb; d2 = dx*dx + dy*dy
 *   L = reach[type] * (ra + rb)
 * With reach[type] = the type's collision_overlap_factor a touch is exactly a pair the solver's collision branch acts on.
 * Touches are never across types and never inside the query's own batch (egg_pieces covers the latter).
 * Per (entry i of the list, type w, other batch) with at least one touching pair there is ONE egg_touch_record, all integers:
 *   slot       2 i + w
 *   other      the other batch's id -- or, under EGG_TOUCH_BY_KEYS in spec.flags, its key (egg_batch_info.key, which a group
 *              and sharded ranks use as the id of the whole scene); the query's key is then compared with keys as well
 *   pairs      the touching (a, b) pairs
 *   particles  the distinct particles b of the other batch that touch any a
 *   dropped    the touching pairs in which a scaled coordinate of either particle reaches 2^53 or is not finite: they count
 *              in pairs and add nothing to the sums
 *   sx, sy     int64 two's complement sums over the remaining pairs of q(xa) + q(xb) and q(ya) + q(yb), q(v) = rint(v *
 *              EGG_SENSOR_POSITION_SCALE), the quantisation of the sensors and the pieces.  The contact point is
 *              sx / (2 * (pairs - dropped)) / 65536.
 * Records are ordered by (slot, other), other ascending; a (slot, other) without a touching pair has no record.  Every field
 * is additive over any split of the other batch's particles -- which is why the number of distinct QUERY particles touched
 * is not in the record: ask the reverse direction.  Every output is an integer and every sum is order-free: the answer does
 * not depend on the schedule, on the device, or on how a scene is split over handles.
 * The device culls by boxes (DESIGN.md section 2.15 has the argument); the cull only skips what the rule rejects.
 * The answer: at most `cap` records into `out`; *n_out is ALWAYS the number of records of the answer.  If it exceeds cap,
 * nothing is written to `out` and the call returns EGG_ERR_INVALID_ARGUMENT with a message naming both numbers: call again
 * with that size (out may be NULL while cap is 0).
 * Everything is checked before anything is launched or written; a refused call leaves out, *n_out and egg_get_stats
 * untouched: EGG_ERR_INVALID_ARGUMENT for a NULL spec or n_out, a reach that is not finite or not above 0, a type_mask
 * outside 1 .. 3, unknown flags, a negative count or cap, a list without a count or a count without a list, a step in flight
 * (egg_step_begin or egg_rx_begin open); EGG_ERR_UNKNOWN_ID for an id that names no live batch; EGG_ERR_UNSUPPORTED for a
 * query of more than EGG_TOUCH_MAX_QUERY discs or a record whose pairs do not fit 31 bits.  Of egg_get_stats only
 * kernel_launches moves.
 * Limits: same type only, no white-yolk touches; colliders touch nothing; no touch that rides on a collider; no per-particle
 * partner lists; no depth of overlap; a batch id or key must fit 31 bits; no touches_to on a device tensor. */
#define EGG_TOUCH_MAX_QUERY (1 << 20)   /* discs of one query */
enum { EGG_TOUCH_BY_KEYS = 1 };          /* flag bit of spec.flags */
typedef struct { double reach[2]; int32_t type_mask, flags; } egg_touch_spec;   /* 24 bytes */
typedef struct { int64_t key; int32_t type, count; } egg_touch_query;           /* 16 bytes */
typedef struct { int32_t slot, pairs, particles, dropped; int64_t other, sx, sy; } egg_touch_record;   /* 40 bytes */

/* the queries are the atoms of the listed batches: n_ids = 0 and ids = NULL mean every live batch, in egg_list_ids order; ids
 * may repeat, in any order. */
int egg_touches(egg_handle *h, const egg_touch_spec *spec, int64_t n_ids, const int64_t *ids, int64_t cap, egg_touch_record *out,
                int64_t *n_out);

/* the queries are host discs: query i holds queries[i].count discs of type queries[i].type (0 white, 1 yolk), the discs of
 * all queries concatenated in x, y, r; slot = 2 i + type.  A batch of h whose id (or key, under EGG_TOUCH_BY_KEYS) equals
 * queries[i].key is left out for that query; -1 excludes nothing.  EGG_ERR_INVALID_ARGUMENT also for a type outside 0 .. 1, a
 * negative count, discs without arrays and a radius that is not finite. */
int egg_touches_of(egg_handle *h, const egg_touch_spec *spec, int64_t n_queries, const egg_touch_query *queries, const double *x,
                   const double *y, const double *r, int64_t cap, egg_touch_record *out, int64_t *n_out);

/* egg_touches for a device group: ids and `other` are the group's ids (EGG_TOUCH_BY_KEYS is implied: a batch's key on its
 * handle is the group's id).  A query's batch lives wholly on one handle, its partners on any: the owner answers egg_touches,
 * every other handle egg_touches_of with the batch's discs -- read through egg_export_batch, what a hand-over reads -- and
 * its key; the records of one (slot, other) are added and sorted: one handle's answer, bit for bit.  Handle 0 refuses a bad
 * spec; nothing is written before every handle has answered. */
int egg_group_touches(egg_group *g, const egg_touch_spec *spec, int64_t n_ids, const int64_t *ids, int64_t cap, egg_touch_record *out,
                      int64_t *n_out);

#endif
