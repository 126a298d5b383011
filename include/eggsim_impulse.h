/* eggsim_impulse.h -- the impulses of libeggsim.so: two entry points and their records.  Part of the C ABI of
 * include/eggsim.h, which includes this file at its end; it is not meant to be included alone.  The main header's section
 * list stands at 173 entry points; with these two the library exports 175. */
#ifndef EGGSIM_IMPULSE_H
#define EGGSIM_IMPULSE_H
#ifndef EGGSIM_H
#error "include eggsim.h, which brings this header along"
#endif

/* ---- impulses: push, blast, stir and brake the particles inside regions (csrc/eggsim_impulses.hip) ----
 * Not in the reference.  Sensors, probes, fields and pieces READ the committed state; an impulse ACTS on it: the particles
 * inside a region get a change of velocity, now, on the device.  A call is STATELESS: it takes an ordered list of at most
 * EGG_MAX_IMPULSES records, edits the COMMITTED velocities -- the arrays egg_download_particles returns for EGG_FIELD_VX /
 * EGG_FIELD_VY -- and returns integer totals per record.  The next step reads the stored velocity as it reads it after any
 * step (reference L:1411-1418), so the edit is a legal change of state in exact and in relaxed order alike; a step that
 * throws a particle out of its tile's claim is validated and run again as ever.  tests/impulse_model.py is the definition
 * in numpy.  FP64 in exactly this order, no contraction, sqrt and / correctly rounded; every comparison is false for a NaN.
 * Region and batch.  `region` is an egg_sensor with the sensors' four kinds and the same type mask, checked and normalised
 * per call by the rule egg_set_sensors uses.  A particle of type w at the committed (x, y) is IN record k when the sensor
 * test holds, the mask has bit w, and id is EGG_IMPULSE_ALL_BATCHES or the id of the particle's batch.  id =
 * EGG_IMPULSE_NO_BATCH is checked like any record and holds no particle: what a member of a device group or a rank passes
 * for a batch that another member owns.
 * Weight.  w = 1.0.  With EGG_IMPULSE_LINEAR, w = 1.0 - sqrt(d2) / R with the test's own d2 and R; if w < 0.0 then w = 0.0.
 * LINEAR is for DISC and CAPSULE with R > 0 only.  With EGG_IMPULSE_BY_INV_MASS then w = w * inv_mass (the committed
 * EGG_FIELD_INV_MASS); it is for KICK and BLAST only.
 * Actions.  (vx, vy) is the velocity record k finds: the velocity record k - 1 left.
 *   KICK   a = (ax, ay, -):    nvx = vx + w * ax, nvy = vy + w * ay.
 *   BLAST  a = (cx, cy, s):    dx = x - cx, dy = y - cy, d2 = dx * dx + dy * dy.  Unless d2 > 0.0 the record passes the
 *                              particle by: it is neither changed nor counted.  Otherwise g = (w * s) / sqrt(d2),
 *                              nvx = vx + g * dx, nvy = vy + g * dy.  s < 0 sucks.
 *   SWIRL  a = (cx, cy, omega): dx = x - cx, dy = y - cy, g = w * omega, nvx = vx - g * dy, nvy = vy + g * dx.  The sign is
 *                              that of collider spin.
 *   BRAKE  a = (ux, uy, k), 0 <= k <= 1: g = w * k, nvx = vx + g * (ux - vx), nvy = vy + g * (uy - vy).  (0, 0, 1) with flat
 *                              weight stops a particle exactly.
 * Parameters an action does not use are read as 0.
 * Accounting.  dvx = nvx - vx, fx = dvx * EGG_IMPULSE_SCALE, and the same for y.  The edit is accepted iff
 * fabs(fx) < 2^53 && fabs(fy) < 2^53.  When accepted: v = nv, count[w] += 1, sdvx[w] += llrint(fx), sdvy[w] += llrint(fy)
 * (int64, round to nearest, ties to even).  Otherwise the particle keeps its velocity for this record and skipped[w] += 1.
 * Only vx and vy are ever written.  Position, last_x / last_y, mass, targets, elapsed, color_version and the canvases stay
 * the last step's; of egg_get_stats only kernel_launches moves, by at most 2 per call.  egg_get_environment measures the
 * committed arrays on every call, so its max_velocity follows the edit and its other nine fields stay.  A draw between an
 * impulse and the next step smears by the new velocities, inside a padding that follows them too: a draw takes its
 * padding from the environment it measures.
 * Determinism.  Particles are independent, records are sequential per particle and the totals are integers: a device
 * group and sharded ranks leave the same bits in every particle and return one handle's totals, by summation.
 * Everything is checked before anything is launched or changed: EGG_ERR_INVALID_ARGUMENT, with the record's index in the
 * message, for n outside 0 .. EGG_MAX_IMPULSES, n > 0 without a list, an unknown action or unknown flag bits, LINEAR on a
 * half-plane, a box or a region with R == 0, BY_INV_MASS on SWIRL or BRAKE, a parameter that is not finite, k outside
 * [0, 1], everything egg_set_sensors refuses for the region, a step in flight (egg_step_begin or egg_rx_begin open);
 * EGG_ERR_UNKNOWN_ID for an id that is neither a sentinel nor known.  n == 0 and a handle without particles succeed and
 * launch nothing.  results == NULL is allowed: the totals are then neither finished nor copied.
 * Limits: no position edits; no impulse that rides on a collider; no per-particle result lists; nothing stored (forces act
 * every step in relaxed order). */
#define EGG_MAX_IMPULSES 64
#define EGG_IMPULSE_SCALE 65536.0            /* 2^16: sums are in 2^-16 px/s */
#define EGG_IMPULSE_ALL_BATCHES ((int64_t)-1)
#define EGG_IMPULSE_NO_BATCH ((int64_t)-2)
enum { EGG_IMPULSE_KICK = 0, EGG_IMPULSE_BLAST = 1, EGG_IMPULSE_SWIRL = 2, EGG_IMPULSE_BRAKE = 3 };
enum { EGG_IMPULSE_LINEAR = 1, EGG_IMPULSE_BY_INV_MASS = 2 };   /* flag bits */
typedef struct { egg_sensor region; int32_t action, flags; int64_t id; double a[3]; } egg_impulse_record;   /* 96 bytes */
typedef struct { int64_t count[2], sdvx[2], sdvy[2], skipped[2]; } egg_impulse_result;               /* 64 bytes */
int egg_impulse(egg_handle *h, int32_t n, const egg_impulse_record *list, egg_impulse_result *results /* [n] or NULL */);

/* egg_impulse for every handle of the group, with its rules: ids are the group's, an id known to no handle returns
 * EGG_ERR_UNKNOWN_ID, and a handle that does not own a record's batch runs that record inert (EGG_IMPULSE_NO_BATCH).  Every
 * handle first checks the list with every record inert, and the ids are checked, before any handle changes a particle.  Every particle ends with the bits one
 * handle with every batch leaves in it; the results are the handles' totals added: one handle's, bit for bit. */
int egg_group_impulse(egg_group *g, int32_t n, const egg_impulse_record *list, egg_impulse_result *results /* [n] or NULL */);

#endif
