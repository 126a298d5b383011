/*
 * eggsim.h -- C ABI of libeggsim.so: the MI355X (gfx950) implementation of the
 * XPBD particle step of Clemapfel/egg_fluid_simulation.
 *
 * The reference has no native/FFI layer; its boundary is the Lua class
 * `SimulationHandler` (simulation_handler.lua:9-419).  Every entry point below
 * is what a LuaJIT `ffi.cdef` wrapper of that class binds for the solver path
 * (the wrapper is lua/egg_fluid_simulation/simulation_handler.lua; the stub a
 * maintainer adds is shown in INTEGRATION.md).  Reference citations are
 * file:line into /root/reference/simulation_handler.lua ("L:").
 *
 * Conventions
 *  - plain C types only; scalars are double / int64_t / int32_t;
 *  - every call returns an int status: EGG_OK, a positive "warning class"
 *    status where the reference prints a warning and carries on, or a negative
 *    "error class" status where the reference throws (log.error);
 *  - egg_last_error(h) gives the message of the last non-OK status;
 *  - arrays are caller-owned and copied during the call;
 *  - one handle is used by one thread at a time (the reference is
 *    single-threaded, non-reentrant);
 *  - there is NO CPU fallback: creating a handle without a usable HIP device
 *    fails with EGG_ERR_NO_DEVICE.
 */
#ifndef EGGSIM_H
#define EGGSIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EGGSIM_ABI_VERSION 3

typedef struct egg_handle egg_handle;

enum {
    EGG_OK = 0,
    EGG_WARN_UNKNOWN_ID = 1,     /* set_target_position / remove on a missing id: warning, no throw (L:145, L:259) */
    EGG_WARN_FEW_PARTICLES = 2,  /* add: white_n < 10 or yolk_n < 5 (L:114-120); the batch IS created */
    EGG_ERR_UNKNOWN_ID = -1,     /* get_position / get_target_position / get_n_particles (L:273, L:286, L:415) */
    EGG_ERR_INVALID_ARGUMENT = -2, /* the reference's log.error paths in add/update (L:71-85, L:184-197) */
    EGG_ERR_NO_DEVICE = -3,
    EGG_ERR_DEVICE = -4,         /* a HIP call failed; message has the HIP error string */
    EGG_ERR_UNSUPPORTED = -5,    /* a configuration the device path does not implement yet */
    EGG_ERR_INTERNAL = -6
};

enum { EGG_WHITE = 0, EGG_YOLK = 1 };

/* The solver-relevant keys of a white/yolk config table (L:1152-1249, defaults in
 * simulation_handler_default_config.lua:10-68) plus the three hidden constants
 * (L:447-448, math.lua:2).  Values are taken as already validated/clamped by the
 * host wrapper (_load_config, L:1253-1320); the library re-applies the clamps the
 * step itself applies (L:1338, L:1768). */
typedef struct {
    double damping;
    double follow_strength;
    double cohesion_strength;
    double cohesion_interaction_distance_factor;
    double collision_strength;
    double collision_overlap_factor;
    double min_mass, max_mass;
    double min_radius, max_radius;
    double max_collision_fraction;     /* 0.05 */
    double mass_distribution_variance; /* 4 */
    double eps;                        /* 1e-8 */
} egg_config;

/* fills *cfg with the reference defaults for `which` */
int egg_default_config(int which, egg_config *cfg);

/* SimulationHandler(white_config, yolk_config) (L:425-459).  yolk == NULL means
 * "same as white" (L:426).  device = HIP device ordinal. */
int egg_create(const egg_config *white, const egg_config *yolk, int device, egg_handle **out);
void egg_destroy(egg_handle *h);
const char *egg_last_error(const egg_handle *h); /* h may be NULL: last create error */

/* set_white_config / set_yolk_config, get_*_config (L:226-248) */
int egg_set_config(egg_handle *h, int which, const egg_config *cfg);
int egg_get_config(const egg_handle *h, int which, egg_config *cfg);

/* add(x, y, white_radius, yolk_radius, ..., white_n, yolk_n) -> id (L:27-135).
 * Pass NaN for a radius and EGG_DEFAULT_COUNT for a count where the caller gave nil: the reference's
 * defaults apply (L:41-58).  Any other count <= 1 -- an explicit 0 or negative one included -- is the
 * reference's "particle count cannot be 1 or negative" error (L:79-85) and creates nothing.
 * Colors are render attributes and stay on the host side. */
#define EGG_DEFAULT_COUNT ((int64_t)-1)
int egg_add(egg_handle *h, double x, double y, double white_radius, double yolk_radius,
            int64_t white_n, int64_t yolk_n, int64_t *out_id);
/* n batches with identical radii in one call (bulk form for 10^4..10^5 batches) */
int egg_add_many(egg_handle *h, int64_t n, const double *xs, const double *ys, double white_radius,
                 double yolk_radius, int64_t white_n, int64_t yolk_n, int64_t *out_ids);
/* Multi-GPU sharding.  The reference keeps every batch of a handler in ONE array in creation order
 * (L:964-993), and the pair solver's results depend on that order.  When the batches are spread over
 * several handlers (one per GPU), each handler must lay its particles out in the global creation
 * order restricted to its batches: `key` is a batch's position in that global order.
 * egg_add_many_keyed appends (keys ascending and larger than every key present); egg_export_batch /
 * egg_import_batch move a batch with its complete particle state between handlers, the import
 * inserting it at its key's place.  State layout: 9 fields x n particles, field-major:
 * x, y, vx, vy, last_x, last_y, inv_mass, radius, mass_t.  The state buffers may be host memory or memory of the
 * handle's device (the copies use hipMemcpyDefault): a multi-GPU host hands a batch over device to device -- e.g.
 * straight into and out of the tensors an RCCL send / receive works on -- without a bounce through the host. */
typedef struct {
    int64_t key;
    double target_x, target_y;
    double white_radius, yolk_radius;
    int64_t n_white, n_yolk;
} egg_batch_info;
int egg_add_many_keyed(egg_handle *h, int64_t n, const double *xs, const double *ys, double white_radius,
                       double yolk_radius, int64_t white_n, int64_t yolk_n, const int64_t *keys, int64_t *out_ids);
int egg_export_batch(egg_handle *h, int64_t id, egg_batch_info *info, double *white_state, double *yolk_state);
int egg_import_batch(egg_handle *h, const egg_batch_info *info, const double *white_state, const double *yolk_state,
                     int64_t *out_id);

/* remove(id) (L:140-155, L:1037-1106) */
int egg_remove(egg_handle *h, int64_t id);

/* set_target_position / get_target_position (L:254-278) */
int egg_set_target(egg_handle *h, int64_t id, double x, double y);
int egg_set_targets_many(egg_handle *h, int64_t n, const int64_t *ids, const double *xs, const double *ys);
int egg_get_target(const egg_handle *h, int64_t id, double *x, double *y);

/* update(delta, step_delta, n_substeps, n_collision_steps) (L:168-222): runs the
 * fixed-step accumulator; *out_n_steps = number of _step calls made. */
int egg_update(egg_handle *h, double delta, double step_delta, int32_t n_substeps,
               int32_t n_collision_steps, int32_t *out_n_steps);
/* _step(delta, n_sub_steps, n_collision_steps) directly (L:1722) */
int egg_step(egg_handle *h, double delta, int32_t n_substeps, int32_t n_collision_steps);
/* Forms the tiles and claims the next _step(step_delta, n_substeps, n_collision_steps) will use, without
 * running it.  Multi-GPU: egg_get_bounds_many then returns each batch's CLAIM for that step, which
 * neighbouring ranks exchange to decide whether two batches on different ranks could interact. */
int egg_prepare_step(egg_handle *h, double step_delta, int32_t n_substeps, int32_t n_collision_steps);
/* A _step in two halves, so that a caller can overlap its own work (the multi-GPU neighbour exchange)
 * with the kernels: egg_step_begin forms the tiles and launches; egg_step_end(commit = 1) waits,
 * validates, re-runs if needed and commits -- begin + end(1) == egg_step; egg_step_end(commit = 0)
 * discards the launched step (the state is double-buffered, nothing was committed; the positions at the start of
 * the last committed step, which draw() reads and which share the buffer a launched step writes, are put back). */
int egg_step_begin(egg_handle *h, double delta, int32_t n_substeps, int32_t n_collision_steps);
int egg_step_end(egg_handle *h, int32_t commit);
/* Between egg_step_begin and egg_step_end: waits for the launched step and reports, per type, the most pairs it
 * visited in one collision pass and the budget 0.05 N^2 it is priced at (L:1657-1658, L:1752-1753) -- BEFORE
 * anything is committed.  Multi-GPU: the reference counts the visits of ALL particles against the budget, a rank
 * sees its own; the ranks add these up and discard the step when the sum could have tripped the early return. */
int egg_step_peek_visits(egg_handle *h, int64_t max_pass_visits[2], double budget[2]);
/* blocks until all device work of this handle is finished */
int egg_synchronize(egg_handle *h);

/* get_position(id) -> mean particle position of the batch (L:281-295, L:1134-1148) */
int egg_get_position(egg_handle *h, int64_t id, double *x, double *y);
int egg_get_positions_many(egg_handle *h, int64_t n, const int64_t *ids, double *xs, double *ys);

/* axis-aligned bounds (px) of each batch, white and yolk together: the cells the batch CLAIMS for the
 * upcoming step when the tiles are current (after egg_prepare_step), otherwise the spatial-hash cells
 * its particles occupy (L:1494-1495).  Used by the multi-GPU slab exchange; the
 * reference computes the same per-environment AABB in _post_solve (L:1703-1709). */
int egg_get_bounds_many(egg_handle *h, int64_t n, const int64_t *ids, double *lo_x, double *lo_y,
                        double *hi_x, double *hi_y);

/* per type: boxes[8 * k + 4 * type + {0,1,2,3}] = lo_x, lo_y, hi_x, hi_y (px) of batch k's claim for the
 * upcoming step (occupied cells if the tiles are not current); cell_sizes[type] = that type's hash cell.
 * Batches of different handlers are independent iff, for both types, their boxes are at least one cell
 * of that type apart in x or in y -- the criterion that separates tiles inside one handler. */
int egg_get_claims_many(egg_handle *h, int64_t n, const int64_t *ids, double *boxes, double *cell_sizes);

/* get_n_particles(id) / get_n_particles() with id < 0 (L:409-419) */
int egg_get_n_particles(const egg_handle *h, int64_t id, int64_t *n_white, int64_t *n_yolk);
/* list_ids (L:399-405): ids in creation order; returns the count in *n, copies min(*n, cap) ids */
int egg_list_ids(const egg_handle *h, int64_t cap, int64_t *ids, int64_t *n);
int egg_get_elapsed(const egg_handle *h, double *elapsed, double *interpolation_alpha);

/* particle fields for egg_download_particles */
enum {
    EGG_FIELD_X = 0, EGG_FIELD_Y, EGG_FIELD_VX, EGG_FIELD_VY, EGG_FIELD_LAST_X, EGG_FIELD_LAST_Y,
    EGG_FIELD_RADIUS, EGG_FIELD_INV_MASS, EGG_FIELD_MASS_T, EGG_FIELD_BATCH_ID, EGG_N_FIELDS
};
/* copies one field of every particle of `which`, in particle-index order, into dst
 * (doubles).  x,y,last_x,last_y,vx,vy,radius form the reference's instanced-draw
 * record (L:513-517, L:744-813). */
int egg_download_particles(egg_handle *h, int which, int field, double *dst, int64_t cap);

/* ---- the instanced-draw record, packed on the device (csrc/eggsim_instances.hip) ----
 * The reference uploads two per-particle meshes every frame (L:513-523, L:744-877): the data mesh -- floatvec4
 * (x, y, last_x, last_y), floatvec2 (vx, vy), float radius: egg_instance below -- and the colour mesh, floatvec4 rgba,
 * which it re-uploads only when colours change (L:519-520).  These entry points hand a host both meshes as its vertex
 * format lays them out, ready for love.data / mesh:setVertices: one kernel launch per type packs them on the device.
 * Each float is the round-to-nearest-even narrowing of the double egg_download_particles returns for that field;
 * particles are in particle-index order; nothing is interpolated (the reference's shader does that, L:2057-2058).  A
 * particle's colour is the rgba the splat of egg_render reads for it (L:978-990, L:1110-1129, the shared config table of
 * L:49-50 included).  color_version goes up whenever a call that can change any particle's colour or the particle count
 * succeeds (egg_set_color, egg_set_add_color, egg_set_render_flags, egg_set_render_config, egg_add*, egg_remove,
 * egg_import_batch) and stands still otherwise: a host skips its colour upload while the version stands. */
typedef struct { float x, y, last_x, last_y, vx, vy, radius; } egg_instance;   /* 28 B, L:513-517 */

/* synchronous: data[n] and, when color != NULL, color[4 n]; *n = particle count of `which`; dst host or device memory */
int egg_get_instances(egg_handle *h, int which, egg_instance *data, float *color, int64_t cap, int64_t *n,
                      uint64_t *color_version);
/* two halves: begin launches the pack and the copy into pinned buffers the handle owns and returns at once;
 * end waits for that and hands out the pointers, valid until the second following begin (two buffers alternate) */
int egg_instances_begin(egg_handle *h, int32_t type_mask);
int egg_instances_end(egg_handle *h, int which, const egg_instance **data, const float **color, int64_t *n,
                      uint64_t *color_version);
/* Details of the three calls above.  cap: particles `data` (and `color`) have room for; smaller than the particle count is
 * EGG_ERR_INVALID_ARGUMENT, nothing is written.  Zero particles is valid (*n = 0).  data may be NULL (colour only), n and
 * color_version may be NULL.  Before the first _step last_x / last_y are whatever egg_download_particles returns then.
 * type_mask: bit EGG_WHITE and / or bit EGG_YOLK (1, 2 or 3); egg_instances_end is called once per type of the mask, in
 * any order, and the begin is closed when every type of the mask has been handed out.  The handle skips its own colour
 * pack and copy while color_version stands: *color then points at the last one.  Later work of the handle (a _step, an
 * add, a remove) may be started between begin and end: what it enqueues on the handle's streams runs behind the pack, and
 * the pack reads the particle arrays and tables of its own only, nothing the host rewrites.  egg_instances_end itself only
 * waits and is never refused.  Refused while a step is in
 * flight (egg_step_begin or egg_rx_begin open), like egg_draw_pack; egg_instances_begin and egg_get_instances also while
 * a begin is open.  (egg_group_get_instances and egg_draw_source_instances, below, are the same pack over a device group
 * and over a scene sharded over processes.) */

/* The per-type reductions the reference's _post_solve / update_last_positions keep in its environment
 * (L:1669-1718, L:1795-1815) -- what :draw() sizes and places its canvases with (L:1946-1950, L:2007,
 * L:2132).  Computed on demand from the device arrays, bounds and maxima in parallel, the centroid sums
 * serially in particle order like the reference: after every _step they equal the reference's env fields
 * bit for bit.  (The reference's fields stay stale until the next _step when batches are added or removed
 * in between; these follow the arrays.)  Before the first _step: bounds +-inf, everything else 0. */
typedef struct {
    double min_x, min_y, max_x, max_y;        /* AABB including the particle radius */
    double centroid_x, centroid_y;            /* mean position */
    double max_radius, max_velocity;
    double last_centroid_x, last_centroid_y;  /* mean of the positions at the start of the most recent _step */
} egg_environment;
int egg_get_environment(egg_handle *h, int which, egg_environment *out);

/* ---- headless renderer: SimulationHandler:draw() (L:158-161) into a float32 RGBA image ----
 * The reference draws through LOVE / OpenGL: _update_canvases (L:1995-2113, simulation_handler_instanced_draw.glsl over
 * the texture of simulation_handler_particle_texture.glsl) splats every particle into one canvas per type, _draw_canvases
 * (L:2117-2175, simulation_handler_outline.glsl, simulation_handler_lighting.glsl) composites them.  These entry points run
 * the same passes as HIP kernels, for image-level regression without a window: float32 canvases sampled at pixel centres,
 * no MSAA, instances blended in particle order (what GL guarantees).  Colours are straight rgba in [0, 1]. */
typedef struct {
    float color[4], outline_color[4];  /* config.color / config.outline_color (default_config.lua:22-23, 54-55) */
    double outline_thickness;          /* px; 0 skips the outline pass AND its setColor (L:2137-2142) */
    double highlight_strength, shadow_strength;
    double texture_scale, motion_blur;
} egg_render_config;
int egg_default_render_config(int which, egg_render_config *cfg);
/* the render keys of set_white_config / set_yolk_config (L:226-236): the config gets a NEW colour table, batches created
 * without a colour keep the old one (L:1307-1311) */
int egg_set_render_config(egg_handle *h, int which, const egg_render_config *cfg);
int egg_get_render_config(const egg_handle *h, int which, egg_render_config *cfg);
/* the handler's hidden constants _use_particle_color, _use_lighting (L:448-449).  With use_particle_color == 0 (default)
 * particles are created white (L:985-990) whatever the batch colour is. */
int egg_set_render_flags(egg_handle *h, int32_t use_particle_color, int32_t use_lighting);
/* the white_color / yolk_color argument of add (L:22-23): the batch gets its own colour table; its particles take the
 * colour only when use_particle_color is set (L:978-990).  Call right after egg_add. */
int egg_set_add_color(egg_handle *h, int64_t id, int which, double r, double g, double b, double a);
/* set_white_color / set_yolk_color (L:328-398): components are clamped to [0, 1]; the batch's particles take the colour
 * (L:1110-1129).  A batch created without a colour argument shares the CONFIG's colour table (L:49-50), so the call
 * also changes config.color -- the colour _draw_canvases tints the whole type with; that aliasing is the reference's.
 * Unknown id: EGG_WARN_UNKNOWN_ID. */
int egg_set_color(egg_handle *h, int64_t id, int which, double r, double g, double b, double a);
typedef struct {
    int32_t screen_w, screen_h;      /* render target; world px = screen px + origin (love.graphics.translate) */
    double origin_x, origin_y;
    double interpolation_alpha;      /* NaN: the handle's (egg_update, L:216) */
    double threshold, smoothness;    /* _thresholding_threshold / _smoothness (L:444-445) */
    int32_t use_instancing;          /* 1: instanced_draw.glsl; 0: the draw loop L:2009-2052 (colour premultiplied by its alpha) */
    int32_t canvas_w[2], canvas_h[2];/* 0: from the environment's bounds (L:1945-1954), growing only over the calls */
    float clear[4];                  /* what the screen holds before draw() */
} egg_render_params;
int egg_default_render_params(egg_render_params *p);
/* draw(): clears the screen image to p->clear, runs both passes, copies screen_w * screen_h * 4 floats (row-major, RGBA)
 * into rgba (may be NULL: the image stays on the device).  Nothing is drawn before the first _step or while one of the
 * types has no particles (the reference has no canvas then: L:1997-1999, L:2118). */
int egg_render(egg_handle *h, const egg_render_params *p, float *rgba);
/* the density canvas of `which` as the last egg_render left it: *w x *h RGBA floats, its top-left corner in world px */
int egg_render_canvas(egg_handle *h, int which, float *rgba, int64_t cap_pixels, int32_t *w, int32_t *hgt, double *x0,
                      double *y0);
/* the particle density texture (L:620-682): *size x *size alpha values (all four channels of the texture hold them) */
int egg_render_particle_texture(egg_handle *h, float *alpha, int64_t cap, int32_t *size);

/* kernels of the packed pipeline (csrc/eggsim_packed.hip), for egg_stats.pk_kernel_ms */
enum {
    EGG_PK_KIND_BEGIN = 0, EGG_PK_KIND_MID, EGG_PK_KIND_LISTS_FRESH, EGG_PK_KIND_LISTS_STALE, EGG_PK_KIND_LEVELS,
    EGG_PK_KIND_SORT, EGG_PK_KIND_EXEC, EGG_PK_KIND_END, EGG_PK_KIND_REDUCE,
    EGG_PK_KIND_PASS, /* egg_pk_levexec_kernel: levels + sort + executor of a dense group in one launch */
    EGG_PK_N_KINDS
};

/* egg_stats.pk_variants: the kernel a phase of the packed pipeline runs depends on the regime (csrc/eggsim_packed.hip) */
enum {
    EGG_PK_VARIANT_LEVELS_INORDER = 1, /* egg_pk_levels_mr16_kernel: more groups than SIMDs */
    EGG_PK_VARIANT_LEVELS_OOO = 2,     /* egg_pk_levels_ooo_kernel (levels + sort in one launch): dense islands on a chip that is not full */
    EGG_PK_VARIANT_EXEC = 4,           /* egg_pk_exec_kernel */
    EGG_PK_VARIANT_EXEC_CHAIN = 8,     /* egg_pk_exec_chain_kernel: branch-free projection, executor waves alone on their SIMDs */
    EGG_PK_VARIANT_SORT_LDS = 16,      /* egg_pk_sort_kernel: sorted list assembled in LDS */
    EGG_PK_VARIANT_SORT_DIRECT = 32,   /* egg_pk_sort_direct_kernel */
    EGG_PK_VARIANT_PASS_FUSED = 64     /* egg_pk_levexec_kernel: out-of-order walk, sort and chain executor of a group in one launch */
};

/* counters of the device path, cumulative since creation */
typedef struct {
    int64_t steps;           /* _step calls executed */
    int64_t pair_solves;     /* visited pairs = n_collided increments (L:1657) */
    int64_t follow_solves;   /* follow-constraint evaluations (N * S per step) */
    int64_t kernel_launches;
    int64_t retiles;         /* host re-clusterings of particles into tiles */
    int64_t redo_steps;      /* steps re-run after a failed independence/budget check */
    int64_t n_tiles[2];      /* current tile count per type */
    int64_t max_tile_particles[2];
    double last_step_kernel_ms; /* device time of the step kernels of the most recent _step (HIP events) */
    int64_t single_tile[2];  /* 1 if that type currently runs in exact-budget single-tile mode */
    double kernel_ms[2];     /* device time of that type's step launches in the most recent _step (EGG_OPT_TIMING) */
    double kernel_ms_sum[2]; /* the same, summed over all committed steps since EGG_OPT_TIMING was switched on */
    int64_t timed_steps;
    int64_t max_pass_visits[2]; /* most pairs visited in one collision pass of the most recent _step, per type */
    double budget[2];           /* max_collision_fraction * N^2 of the most recent _step (L:1752-1753), per type */
    int64_t fused_launch;       /* 1 if the most recent _step ran both types' tiles in one launch (kernel_ms[0] == kernel_ms[1] is then that launch) */
    int64_t packed[2];          /* launch classes of that type currently stepped by the packed pipeline (one launch per phase) */
    /* EGG_OPT_TIMING = 2: HIP events around every launch of the packed pipeline, summed per kernel kind and type since the
     * option was set: [type][kind], kind as in EGG_PK_KIND_* below */
    double pk_kernel_ms[2][EGG_PK_N_KINDS];
    int64_t pk_kernel_launches[2][EGG_PK_N_KINDS];
    /* host wall time of _step's phases, summed since creation: [0] tiles and claims (re-clustering, packed plan), [1] uploads
     * and kernel launches, [2] waiting for the status block */
    double host_ms[3];
    /* packed pipeline: the longest chain of dependent pairs in one collision pass of the most recent _step, per type -- the
     * number of levels its executor ran one after the other (the path's latency floor: DESIGN.md section 4) */
    int64_t max_levels[2];
    /* packed pipeline: which kernel variants the classes of that type run (EGG_PK_VARIANT_* bits; several classes may differ) */
    int64_t pk_variants[2];
    /* _step calls executed in relaxed order (EGG_OPT_SOLVER_ORDER = 1); included in `steps` */
    int64_t relaxed_steps;
    /* effective cohesion (EGG_OPT_COHESION = 1): distinct pairs whose cohesion branch fired, summed over passes; each pair
     * counted once, by the holder of its smaller key, as pair_solves counts ("Cohesion") */
    int64_t cohesion_solves;
    /* launch classes of that type whose tiles keyed their cells by the LDS hash table instead of the dense grid in the most
     * recent exact-order _step (0: every class ran on the dense grid; DESIGN.md section 2.1, "Cells") */
    int64_t cell_hash[2];
} egg_stats;
int egg_get_stats(egg_handle *h, egg_stats *out);

/* Diagnostic: the step kernel expands its f64 divisions and square root by hand (see
 * eggsim_step.hip); this runs those expansions against `/` and sqrt() on n random operand pairs on
 * the device and returns the number of results that differ in any bit (must be 0). */
int egg_selftest_arith(egg_handle *h, int64_t n_operand_pairs, uint64_t seed, int64_t *mismatches);

/* Diagnostic: the same expansions on the CALLER's operands, nothing judged on the device.  For each of the `count`
 * triples (n[i], d[i], x[i]) out[8 i ..] receives: egg_div_with_rcp(n, d, egg_rcp_refined(d)); egg_sqrt_core(x); root and
 * rroot of egg_sqrt_rcp_core(x); egg_div_with_rcp(n, root, rroot); and what the rest of the exact path divides and roots
 * with: egg_div(n, d) (the `/` operator with its last place corrected), sqrt(x) and egg_div(n, sqrt(x)).  All four pointers
 * are host memory.  Operands outside the expansions' windows (|n|, |d| in [2^-300, 2^300], x in [2^-600, 2^600]) give
 * whatever the expansions make of them. */
int egg_selftest_arith_operands(egg_handle *h, int64_t count, const double *n, const double *d, const double *x, double *out /* 8 * count */);

/* tuning knobs (not part of the reference surface) */
enum {
    EGG_OPT_CLAIM_MARGIN_CELLS = 0, /* initial margin around an atom's cells when tiles are formed */
    EGG_OPT_TILE_TARGET_PARTICLES,  /* pack independent islands into tiles up to this size (0 = one island per tile; default 60: small islands share a wave) */
    EGG_OPT_TIMING,                 /* 1: record HIP events around the step kernels; 2: also around every launch of the packed pipeline (profiling runs: ~2 events per launch) */
    EGG_OPT_FORCE_SINGLE_TILE,      /* 1: always run each type as one tile (exact budget path) */
    EGG_OPT_THREADS_PER_PARTICLE,   /* lanes per particle: 0 automatic (3 for tiles that have a CU to themselves: visit lists built column-wise), 1 or 3 forced */
    EGG_OPT_SPIN_SLEEP,             /* -1 auto, 0 never, 1 always: idle dataflow waves sleep between polls */
    EGG_OPT_BUDGET_PARTICLES_WHITE, /* multi-GPU: N of the collision budget 0.05 N^2 (L:1752-1753) = particles of ALL ranks; -1 = local */
    EGG_OPT_BUDGET_PARTICLES_YOLK,
    EGG_OPT_FORCE_GLOBAL_STATE,     /* test hook: 1 = every tile keeps its state in global memory (the large-island fallback) */
    EGG_OPT_FUSE_TYPES,             /* 1 (default): white and yolk tiles share one launch when the chip holds several tiles per CU; 0: one launch per type */
    EGG_OPT_PACKED,                 /* packed pipeline (one launch per phase, pair projections of many islands packed into full waves): -1 automatic (large scenes), 0 never, 1 whenever a launch class is eligible */
    EGG_OPT_GROUP_PARTICLES,        /* packed pipeline: particles whose positions one wave of the pair executor keeps in LDS (0, the default: by scene size, 320..1280) */
    EGG_OPT_LEVEL_WALK,             /* packed pipeline, the pass that gives every pair its dependency level: 0 (default) by regime -- out of order for dense islands (> 256 particles) while the groups are no more than the chip's SIMDs, in order otherwise --, 1 always in order, 2 out of order everywhere */
    EGG_OPT_SOLVER_ORDER,           /* 0 (default): exact -- the reference's sequential Gauss-Seidel pair order, bit for bit; 1: relaxed --
                                     * every collision pass a Jacobi pass with constraint averaging: plausible,
                                     * deterministic, not the reference's numbers.  A relaxed handle steps by itself, inside an
                                     * egg_group (egg_group_set_solver_order) or pass by pass (egg_rx_*): egg_step_begin, egg_step_end and egg_get_claims_many
                                     * return EGG_ERR_UNSUPPORTED, egg_prepare_step does nothing.  Refused while a step is in flight. */
    EGG_OPT_RELAXATION,             /* omega of the relaxed pass, in (0, 2] (default EGG_RELAXATION_DEFAULT).  Refused while a step is in flight. */
    EGG_OPT_COHESION,               /* 0 (default): as the reference -- cohesion_strength and cohesion_interaction_distance_factor move no
                                     * particle (L:1608-1613 give same-batch pairs an interaction distance of 0); 1: effective -- in a relaxed
                                     * pass a same-batch pair beyond the collision distance overlap (ra + rb) but within factor (ra + rb) is
                                     * pulled back to the collision distance with the cohesion compliance ("Cohesion").
                                     * Relaxed order only: 1 is EGG_ERR_UNSUPPORTED on a handle in exact order, and EGG_OPT_SOLVER_ORDER = 0 is
                                     * EGG_ERR_UNSUPPORTED while cohesion is 1 (switch cohesion off first).  Refused while a step is in flight. */
    EGG_OPT_FORCE_CELL_HASH         /* test hook: 1 = every launch class of both types keys its cells by the LDS hash table (the fallback of tiles whose
                                     * claim box is too large for a dense grid), sized by the usual rule; 0 (default): by the size of the claim box.
                                     * Exact order only: relaxed order has a hash table of its own and ignores the option. */
};
#define EGG_SOLVER_EXACT 0
#define EGG_SOLVER_RELAXED 1
#define EGG_COHESION_REFERENCE 0
#define EGG_COHESION_EFFECTIVE 1
#define EGG_RELAXATION_DEFAULT 1.8
int egg_set_option(egg_handle *h, int option, double value);

/* ---- static colliders (not in the reference, which has no boundary of any kind; DESIGN.md section 2.7, "Colliders") ----
 * A handle holds an ordered list of at most EGG_MAX_COLLIDERS colliders.  In a RELAXED collision pass the position a
 * particle of a type in `type_mask` (bit 0 white, bit 1 yolk) is about to get is projected rigidly, collider after
 * collider in list order, each on the result of the one before -- whether or not a pair fired for it.  r is the
 * particle's radius; FP64 in exactly this order, no contraction; every comparison is false for a NaN.
 *   HALF_PLANE p = (nx, ny, off, -): keeps n . pos - off >= r.  s = (nx x + ny y) - (off + r); s < 0: x -= s nx, y -= s ny.
 *              The normal is normalised when the list is set (len = sqrt(nx nx + ny ny); nx / len, ny / len are stored
 *              and returned by egg_get_colliders).
 *   DISC       p = (cx, cy, R, -): an obstacle.  dx = x - cx, dy = y - cy, d2 = dx dx + dy dy, m = R + r; d2 < m m:
 *              d = sqrt(d2), x = cx + (dx / d) m, y = cy + (dy / d) m; at d2 == 0 the unit vector is the one a coincident
 *              pair with key difference (key & 7) takes, the key being the particle's index in one handle holding
 *              every batch (the global key in a group or between processes).
 *   CONTAINER  p = (cx, cy, R, -): the particle stays inside.  m = max(R - r, 0); d2 > m m: x = cx + (dx / d) m, y likewise.
 *   SEGMENT    p = (x0, y0, x1, y1): a wall of zero thickness.  e = p1 - p0, l2 = e . e,
 *              t = l2 == 0 ? 0 : clamp(((x - x0) ex + (y - y0) ey) / l2, 0, 1), q = p0 + t e; then DISC with centre q, R = 0.
 *              It looks only at the position a pass has produced: a particle carried more than r past it inside one
 *              sub-step lands on the far side and is pushed on.  A segment does not hold what moves fast; a WALL does.
 *   WALL       p = (x0, y0, x1, y1): a two-sided thin wall that sweeps.  A particle that starts a sub-step on one side
 *              cannot end a pass on the other, however far the pass moved it.  prev is the particle's position at the
 *              start of the sub-step (what step 5c reads).  e, l2, t, q as SEGMENT; dx = x - qx, dy = y - qy,
 *              d2 = dx dx + dy dy, m = 0 + r; then
 *                a0 = ex (prev.y - y0) - ey (prev.x - x0), a1 = ex (y - y0) - ey (x - x0);
 *                opp = (a0 > 0 && a1 <= 0) || (a0 < 0 && a1 >= 0); caught = false; if opp: u = a0 / (a0 - a1),
 *                hx = prev.x + u (x - prev.x), hy = prev.y + u (y - prev.y), tc = ((hx - x0) ex + (hy - y0) ey) / l2,
 *                caught = tc >= 0 && tc <= 1.
 *              caught: l = sqrt(l2), d = sqrt(d2), n = a0 > 0 ? ((-ey) / l, ex / l) : (ey / l, (-ex) / l) -- the unit normal
 *              towards prev's side --, x = qx + nx m, y = qy + ny m: one hit; for step 5c the normal is n and pen = m + d.
 *              Not caught: SEGMENT's rule, bit for bit.  A path that passes beyond an end (tc outside [0, 1]) goes round
 *              the wall; a sub-step that starts exactly on the line (a0 == 0) has no side and is not caught; a
 *              degenerate wall (l2 == 0, so a0 == 0) never catches and acts as SEGMENT's point; a NaN prev or position is
 *              not caught.  prev does not change inside a sub-step, so every pass sweeps from the same start (the
 *              viscosity pass rewrites prev only after the sub-step's last collision pass).  The sweep is against the
 *              list as it is: not against a list the caller changes between steps.  A catch adds no counter of its own.
 * Parameters a kind does not use are stored as 0.  The projection has no compliance, mass, friction or omega; velocities
 * follow from the post-solve, so a wall absorbs the normal velocity.  Colliders are drawn only where a style asks for it (egg_set_collider_styles
 * below; undrawn by default).  Applied in list order, a
 * particle in a corner satisfies the last collider exactly and the earlier ones only approximately.
 * Relaxed order only, as EGG_OPT_COHESION = 1: a non-empty list on a handle in exact order is EGG_ERR_UNSUPPORTED, and
 * EGG_OPT_SOLVER_ORDER = 0 is EGG_ERR_UNSUPPORTED while the list is not empty; an empty list is always accepted.
 * egg_set_colliders checks everything before it changes anything: EGG_ERR_INVALID_ARGUMENT, with the collider's index in
 * the message, for n outside 0 .. EGG_MAX_COLLIDERS, an unknown kind, a mask that is 0 or has bits beyond 3, a parameter
 * that is not finite, R < 0, a normal shorter than the white config's eps.  Refused while a step is in flight.  The list
 * goes to the device when it is set, never per step; with an empty list a step launches exactly what it launches without,
 * and a list without a WALL launches exactly what it launched before there were walls. */
#define EGG_MAX_COLLIDERS 64
enum { EGG_COLLIDER_HALF_PLANE = 0, EGG_COLLIDER_DISC = 1, EGG_COLLIDER_CONTAINER = 2, EGG_COLLIDER_SEGMENT = 3 };
enum { EGG_COLLIDER_WALL = 5 }; /* 4 is not a kind: it was refused as unknown before there were walls, and it stays refused */
typedef struct {
    int32_t kind;      /* EGG_COLLIDER_* */
    int32_t type_mask; /* bit 0 white, bit 1 yolk; never 0 */
    double p[4];
} egg_collider; /* 40 bytes */
int egg_set_colliders(egg_handle *h, int32_t n, const egg_collider *c); /* n == 0 clears */
/* the list as stored (normals normalised): the count in *n, min(*n, cap) colliders copied */
int egg_get_colliders(const egg_handle *h, int32_t cap, egg_collider *c, int32_t *n);
/* hits per type since the handle was created: one collider moving one particle in one pass is one hit.  Only committed
 * steps count: a step that fails or is discarded adds nothing. */
int egg_get_collider_hits(egg_handle *h, int64_t hits[2]);

/* ---- collider surfaces: Coulomb friction and surface velocity ("Collider surfaces") ----
 * Every collider of the list may carry a SURFACE: a friction coefficient mu >= 0 and a surface velocity (vx, vy) in px/s.
 * The default surface is all zeros, and a list whose surfaces are all default behaves exactly as one without surfaces.
 * Step 5c sits inside the collider loop: it applies to collider k when its mask covers the type, its condition held in
 * this pass (a hit) and mu_k > 0.0, right after that collider's projection has been written into (x, y) and before the
 * next collider sees the result.  prev is the particle's position at the start of the sub-step, h the sub-step
 * (delta / n_sub_steps, at least eps); n and pen are the projection's own values:
 *   HALF_PLANE        n = (nx, ny) as stored, pen = -s
 *   DISC and SEGMENT  n = the unit vector the projection used (the coincident pair's at d2 == 0), pen = m - d (d = 0 at
 *                     the centre; a segment has m = 0 + r)
 *   WALL              caught: n = the unit normal towards prev's side, pen = m + d; not caught: as SEGMENT
 *   CONTAINER         n = (dx / d, dy / d), pen = d - m
 * FP64 in exactly this order, no contraction, sqrt and / correctly rounded; every comparison is false for a NaN:
 *   ex = (x - prev.x) - h vx, ey = (y - prev.y) - h vy, dn = ex nx + ey ny, tx = ex - dn nx, ty = ey - dn ny,
 *   tl2 = tx tx + ty ty; !(tl2 > 0.0): nothing happens and nothing is counted; otherwise tl = sqrt(tl2), lim = mu pen;
 *   tl <= lim (stick): x = x - tx, y = y - ty; else (slide): f = lim / tl, x = x - tx f, y = y - ty f.
 * Either branch is one GRIP.  The tangential part of the sub-step's displacement relative to the surface is removed up to
 * mu times the depth the collider has just corrected; velocities follow from the post-solve, so a gripped particle loses
 * tangential velocity and a surface with a velocity drags what touches it (a conveyor; a pan the caller moves by setting
 * the list again).  The viscosity pass rewrites prev only after the sub-step's last collision pass: friction reads the
 * un-smoothed start of the sub-step.  The tangential move leaves a half-plane's constraint exact and a circle's by second
 * order, which the next pass projects again.
 * egg_set_collider_surfaces: n must equal the current collider count, or 0 (every surface back to default).  Everything is
 * checked before anything changes: EGG_ERR_INVALID_ARGUMENT, with the collider's index in the message, for an n that does
 * not match, a friction that is negative or not finite, a velocity that is not finite.  egg_set_colliders resets every
 * surface to default (the indices no longer mean anything).  A -0.0 is stored as +0.0.  Refused while a step is in flight.  The records go to the
 * device when they are set, never per step; while no friction is > 0 -- a velocity alone does nothing -- a step launches
 * exactly what it launches without surfaces. */
typedef struct {
    double friction; /* mu >= 0 */
    double vx, vy;   /* px/s */
} egg_collider_surface; /* 24 bytes */
int egg_set_collider_surfaces(egg_handle *h, int32_t n, const egg_collider_surface *s);
/* the surfaces as stored, one per collider (defaults included): the count in *n, min(*n, cap) records copied */
int egg_get_collider_surfaces(const egg_handle *h, int32_t cap, egg_collider_surface *s, int32_t *n);
/* grips per type since the handle was created, over committed steps only: a step that fails or is discarded adds nothing */
int egg_get_collider_grips(egg_handle *h, int64_t grips[2]);

/* ---- collider motion: a rigid velocity per collider, integrated on the device ("Collider motion") ----
 * Every collider of the list may carry a MOTION (vx, vy) in px/s, a rigid translation; the default is zero, and a list
 * whose motions are all zero behaves as a list without motion and launches exactly the kernels it launches without.  The
 * stored list is the geometry at the start of the step.  With h the sub-step (delta / n_sub_steps, at least eps), S the
 * sub-step count and sub the 0-based sub-step, every pass of sub-step sub uses the geometry at the sub-step's end:
 *   t  = (double)(sub + 1) * h;  ox = t vx, oy = t vy
 *   HALF_PLANE (nx, ny, off):        off' = off + (nx ox + ny oy)                       (the normal does not change)
 *   DISC, CONTAINER (cx, cy, R):     cx' = cx + ox, cy' = cy + oy
 *   SEGMENT, WALL (x0, y0, x1, y1):  x0' = x0 + ox, y0' = y0 + oy, x1' = x1 + ox, y1' = y1 + oy
 * and step 5b runs on the primed parameters as written above.  A moving WALL takes the side of the sub-step's start in
 * its own frame: pvx = prev.x + h vx, pvy = prev.y + h vy stand wherever the wall rule reads prev (a0, hx, hy).  A wall
 * that passes over a particle at rest catches it and carries it on its front side; a particle that moves exactly with the
 * wall is never caught: a particle that starts a sub-step on one side of a wall cannot end a pass on the other, whichever
 * of the two moved.  Step 5c takes the surface's velocity plus the motion's, and reads the true prev:
 *   wx = sf.vx + vx, wy = sf.vy + vy;  ex = (x - prev.x) - h wx, ey = (y - prev.y) - h wy;  the rest as written.
 * So a moving collider with mu > 0 drags what it touches.  FP64 in exactly this order, no contraction.
 * When a step is committed the stored geometry of every collider becomes its primed geometry with t = (double)S * h -- the
 * expression of the last sub-step, so the same bits -- and egg_get_colliders returns it; a failed or discarded step
 * advances nothing.  Motions and surfaces persist across steps.  Only walls sweep: a fast disc, half-plane or container can
 * still jump over a particle inside one sub-step.  No rotation, no acceleration: a caller changes a velocity between steps.
 * egg_set_collider_motion: n must equal the current collider count, or 0 (every motion back to zero).  Everything is
 * checked before anything changes: EGG_ERR_INVALID_ARGUMENT, with the collider's index in the message, for an n that does
 * not match or a component that is not finite.  It leaves geometry and surfaces alone; egg_set_colliders resets every
 * motion to zero, egg_set_collider_surfaces leaves them.  A -0.0 is stored as +0.0.  Refused while a step is in flight. */
typedef struct {
    double vx, vy; /* px/s */
} egg_collider_motion; /* 16 bytes */
int egg_set_collider_motion(egg_handle *h, int32_t n, const egg_collider_motion *m);
/* the motions as stored, one per collider (zeros included): the count in *n, min(*n, cap) records copied */
int egg_get_collider_motion(const egg_handle *h, int32_t cap, egg_collider_motion *m, int32_t *n);

/* ---- collider spin: a rigid angular velocity per collider about a pivot ("Collider spin") ----
 * Every collider of the list may carry a SPIN (px, py, omega): it turns about the pivot (px, py), in px at the start of the
 * step, at omega rad/s, counter-clockwise positive in the project's x/y.  The default is zero, and a list whose spins are all
 * zero behaves as a list without spin and launches exactly the kernels it launches without.  A collider whose omega is zero
 * takes the expressions of collider motion exactly as they stand.  For one whose omega is not zero, with h, S, sub, t, ox, oy
 * and (vx, vy) as above (its motion, zero by default):
 *   Px = px + ox, Py = py + oy                                   the pivot rides on the collider's motion
 *   c = cos(t omega), s = sin(t omega)                           computed on the host (libm), handed to the kernel
 *   a point (qx, qy) of the stored geometry:  rx = qx - px, ry = qy - py,
 *                                             qx' = Px + (c rx - s ry), qy' = Py + (s rx + c ry)
 *   DISC, CONTAINER: the centre is such a point, R unchanged;  SEGMENT, WALL: both end points
 *   HALF_PLANE (nx, ny, off):  nx' = c nx - s ny, ny' = s nx + c ny,
 *                              off' = (nx' Px + ny' Py) + (off - (nx px + ny py))   (the pivot's signed distance is kept)
 * and step 5b runs on the primed parameters.  A turning WALL takes the side of the sub-step's start carried along with it
 * over ONE sub-step: with ts = (double)sub * h, ch = cos(h omega), sh = sin(h omega) (host, once per step),
 *   ux = prev.x - (px + ts vx), uy = prev.y - (py + ts vy);  pvx = Px + (ch ux - sh uy), pvy = Py + (sh ux + ch uy)
 * stand wherever the wall rule reads prev.  Step 5c takes the surface's velocity at the contact point, (x, y) being the
 * position the projection has just produced, and reads the true prev:
 *   wx = (sf.vx + vx) - omega (y - Py), wy = (sf.vy + vy) + omega (x - Px)
 * So a disc that spins about its own centre keeps its geometry and drags what touches it when mu > 0.  FP64 in exactly this
 * order, no contraction.  When a step is committed the stored geometry, and the stored pivot, become the primed values with
 * t = (double)S * h, computed on the host from the c, s the last sub-step used, so the same bits; egg_get_colliders and
 * egg_get_collider_spin return them.  A failed or discarded step advances nothing.  There is no exact-order rule and no
 * counter of its own: a catch by a turning wall is a hit, a grip is a grip.  No angular acceleration; only walls sweep; a
 * half-plane's normal is not renormalised after it turns and end points are not re-spaced (DESIGN.md has the drift).
 * egg_set_collider_spin: n must equal the current collider count, or 0 (every spin back to zero).  Everything is checked
 * before anything changes: EGG_ERR_INVALID_ARGUMENT, with the collider's index in the message, for an n that does not match
 * or a component that is not finite.  It leaves geometry, surfaces and motions alone; egg_set_colliders resets every spin
 * to zero, egg_set_collider_motion and egg_set_collider_surfaces leave them.  A -0.0 is stored as +0.0 and counts as zero.
 * Refused while a step is in flight. */
typedef struct {
    double px, py; /* the pivot, px */
    double omega;  /* rad/s, counter-clockwise positive */
} egg_collider_spin; /* 24 bytes */
int egg_set_collider_spin(egg_handle *h, int32_t n, const egg_collider_spin *s);
/* the spins as stored, one per collider (zeros included): the count in *n, min(*n, cap) records copied */
int egg_get_collider_spin(const egg_handle *h, int32_t cap, egg_collider_spin *s, int32_t *n);

/* ---- collider loads: the impulse and torque a collider receives in a step ("Collider loads") ----
 * Steps 5b and 5c act one way: a collider moves particles and feels nothing.  With collider loads on, a RELAXED step with a
 * non-empty list also records, per collider, what it did to the particles, with the sign of what the collider feels.  It
 * only observes: positions and every counter are those of the same step with loads off, bit for bit.
 * One CONTRIBUTION is counted for every (collider c, particle, pass) in which c moved the particle (a hit) and the particle's
 * inverse mass im satisfies im > eps (the force step's own test, eps of the white config):
 *   (bx, by)  the position that entered collider c's rule;  (ax, ay)  the position that left it, step 5c's grip included
 *   m  = 1.0 / im
 *   ux = m * (bx - ax),  uy = m * (by - ay)                    the reaction: what the collider feels, in mass px
 *   (Px, Py)  the pivot of the sub-step: the collider's spin record's (px, py) riding on its motion at the sub-step's end,
 *             Px = px + t vx, Py = py + t vy, exactly as step 5b computes it, also when omega == 0; (0, 0) when the handle
 *             holds no spin records
 *   uz = (ax - Px) * uy - (ay - Py) * ux                       its moment about the pivot, in mass px^2
 * FP64 in exactly this order, no contraction.  Each contribution is quantised before it is added:
 *   qx = llrint(ux * EGG_COLLIDER_LOAD_IMPULSE_SCALE),  qy = llrint(uy * EGG_COLLIDER_LOAD_IMPULSE_SCALE),
 *   qz = llrint(uz * EGG_COLLIDER_LOAD_TORQUE_SCALE)           int64, round to nearest, ties to even
 * If one of the three scaled values is not finite or reaches 2^53 in magnitude, the contribution is dropped whole and
 * counted in `dropped`; otherwise the three integers are added to collider c's three sums.  Integer addition is
 * associative: the sums do not depend on the order of lanes, waves, devices or ranks, so a device group and sharded ranks
 * equal one handle bit for bit.  Both types add into the same sums (a collider's type mask decides who touches it).  The
 * resolution is 2^-20 (about 1e-6) mass px for the impulse and 2^-10 (about 1e-3) mass px^2 for the torque; the sums wrap
 * only beyond 2^63 (DESIGN.md has the bound).
 * The sums cover ONE step: cleared when a step starts, visible when it commits; a failed or discarded step leaves the values
 * of the step before.  A collider nothing touched reads exactly 0.  egg_set_colliders keeps the switch and zeroes the
 * stored loads; egg_set_collider_loads zeroes them too.
 * egg_set_collider_loads(h, on): off by default; accepted in either solver order and with an empty list (it acts only in a
 * relaxed step with a non-empty list); refused while a step is in flight.  With loads off a step launches exactly the
 * kernels it launches today, with the same arguments.
 * egg_get_collider_load_sums: the raw integers, sums[3 k + 0 .. 2] = (sum qx, sum qy, sum qz) of collider k for min(*n, cap)
 * colliders, the dropped count and the sub-step h of the step that produced them (0.0 while none has).
 * egg_get_collider_loads: {jx, jy, torque} with jx = ((double)sx / EGG_COLLIDER_LOAD_IMPULSE_SCALE) / h, jy likewise, and
 * torque = ((double)sz / EGG_COLLIDER_LOAD_TORQUE_SCALE) / h: the impulse in mass px/s (and the angular impulse in mass
 * px^2/s) the collider received over the step; all zeros while no step has produced any.  The MEAN FORCE over a step of
 * length delta is j / delta (and the mean torque is torque / delta).  No exact-order rule, no per-particle or per-type
 * loads, nothing from containment or coupling. */
#define EGG_COLLIDER_LOAD_IMPULSE_SCALE 1048576.0 /* 2^20 */
#define EGG_COLLIDER_LOAD_TORQUE_SCALE 1024.0     /* 2^10 */
typedef struct {
    double jx, jy; /* mass px/s */
    double torque; /* mass px^2/s, counter-clockwise positive in the project's x/y, about the collider's pivot */
} egg_collider_load; /* 24 bytes */
int egg_set_collider_loads(egg_handle *h, int on);
int egg_get_collider_loads_enabled(const egg_handle *h, int *on);
int egg_get_collider_load_sums(egg_handle *h, int32_t cap, int64_t *sums /* [n][3] */, int64_t *dropped, double *sub_delta, int32_t *n);
int egg_get_collider_loads(egg_handle *h, int32_t cap, egg_collider_load *out, int32_t *n);

/* ---- collider bodies: colliders the device integrates from their own loads ("Collider bodies") ----
 * Every collider of the list may carry a BODY {inv_mass, inv_inertia, ax, ay, drag, spin_drag}: inv_mass > 0 frees its
 * translation, inv_inertia > 0 its rotation about its spin pivot; a collider with both zero is no body and stays kinematic.
 * A hinge is (0, 1/I), a plate (1/M, 0), a free ball both.  ax, ay (px/s^2) act only when inv_mass > 0; drag and spin_drag are
 * in 1/s.  Bodies ACT in a step when the order is relaxed, the list is not empty, some collider is a body and collider loads
 * are on.  A relaxed step with a body, a list and loads off fails before anything is launched with EGG_ERR_UNSUPPORTED
 * (egg_set_collider_loads first).  With no body a step launches exactly the kernels it launches today, with the same
 * arguments.
 * While bodies act every collider has a motion, a spin and a turn (c, s) on the device, zeros included, and every sub-step
 * runs the rules of collider loads, motion and spin as the FIRST sub-step of a step over those records: the geometry at
 * t = h, the start at ts = 0, the turn standing for both rows of the table.  After the last pass of a sub-step of both
 * types (and after viscosity) one kernel does, for every collider k, FP64 in exactly this order, no contraction:
 *   1. d = sums[k] - seen[k] (three int64), seen[k] = sums[k];
 *      Jx = ((double)dx / 2^20) / h, Jy likewise, Jz = ((double)dz / 2^10) / h          the sub-step's impulse
 *   2. the stored geometry and the stored pivot become the primed values of collider motion / collider spin at t = h, with
 *      the velocity, omega and (c, s) the sub-step used (omega != 0: the spin expressions, and the pivot rides; otherwise the
 *      motion expressions, and the pivot stays, as at a commit).  The kinematic colliders of the list advance too.
 *   3. inv_mass > 0:     vx = vx + Jx * inv_mass; vx = vx + h * ax (y likewise);
 *                        f = 1 - h * drag; if (!(f > 0)) f = 0; vx = vx * f; vy = vy * f
 *   4. inv_inertia > 0:  omega = omega + Jz * inv_inertia; the same damping with spin_drag; then the next turn
 *                        u = 0.5 * (h * omega); den = 1 + u * u; c = (1 - u * u) / den; s = (u + u) / den
 * The turn of a free-turning body is this Cayley rotation, by 2 atan(h omega / 2) instead of h omega: only + - * / occur, so
 * host, device and the numpy model agree to the bit.  A collider with inv_inertia == 0 keeps the host's libm
 * (cos, sin)(h omega).  A list with bodies advances sub-step by sub-step, not by (sub + 1) h v from the step's start: equal
 * to the step without bodies by roundings only, bit for bit at S = 1.  The commit reads the list, the motions and the spins
 * back: egg_get_colliders, egg_get_collider_motion and egg_get_collider_spin return them; the loads cover the whole step.
 * A failed step advances nothing.  The coupling is explicit: a body much lighter than what it touches may oscillate
 * (DESIGN.md has the measured range).  Bodies meet each other only through collider contacts (below); no exact-order rule.  ONE handle only: a device group refuses
 * to step and egg_rx_begin returns EGG_ERR_UNSUPPORTED while a handle holds a body.
 * egg_set_collider_bodies: n must equal the current collider count, or 0 (no collider is a body).  Everything is checked
 * before anything changes: EGG_ERR_INVALID_ARGUMENT, with the collider's index in the message, for an n that does not match,
 * a component that is not finite, or a negative inv_mass, inv_inertia, drag or spin_drag.  egg_set_colliders resets the
 * bodies; egg_set_collider_motion, egg_set_collider_spin and egg_set_collider_surfaces leave them.  A -0.0 is stored as +0.0.
 * Refused while a step is in flight. */
typedef struct {
    double inv_mass, inv_inertia; /* 1 / mass, 1 / (mass px^2); 0 = not freed */
    double ax, ay;                /* px/s^2, with inv_mass > 0 only */
    double drag, spin_drag;       /* 1/s */
} egg_collider_body; /* 48 bytes */
int egg_set_collider_bodies(egg_handle *h, int32_t n, const egg_collider_body *b);
/* the bodies as stored, one per collider (zeros included): the count in *n, min(*n, cap) records copied */
int egg_get_collider_bodies(const egg_handle *h, int32_t cap, egg_collider_body *b, int32_t *n);

/* ---- collider contacts: bodies that meet the other colliders ("Collider contacts") ----
 * Every collider of the list may carry a CONTACT record {restitution, on, reserved}: restitution in [0, 1], on 0 or 1,
 * reserved 0.  Contacts ACT in a step exactly when bodies act (above) and some record is on.  While they do not, a step
 * launches exactly the kernels it launches today, with the same arguments -- a list with records on but no body, or with
 * loads off, included.  While they act, every sub-step ends, behind step 4 of collider bodies and on what that step has
 * written (the stored geometry and pivots of the sub-step's end, the new velocities and spins), with one more kernel.  FP64
 * in exactly this order, no contraction, + - * / sqrt only, h the sub-step; every comparison is false for a NaN:
 *   1. the generalised body: collider k has the weights mk = inv_mass, ik = inv_inertia (0 and 0 when it is no body) and at
 *      a point p the velocity  ux = vx - omega * (py - Py), uy = vy + omega * (px - Px),  P its stored spin pivot
 *   2. (a, b), a < b, is a PAIR when both are on, one is a disc, the other a half-plane, disc, container, segment or wall,
 *      and ((ma + ia) + mb) + ib > 0.  From the stored poses: the unit normal n from a to b, the gap g (negative: overlap),
 *      one contact point p.  Two discs meet along the centre line (coincident centres: DIRS[(b - a) & 7], the rule of
 *      coincident particles), g = d - (Ra + Rb), p on a's rim; a half-plane along its normal; a container holds the disc
 *      inside, g = (Rc - R) - d (coincident centres: DIRS likewise); a segment or wall at the closest point of the closed
 *      segment, end points included (a centre exactly on it: the segment's left normal ((-ey) / l, ex / l)).  Both sides
 *      evaluate one expression with a the smaller index.  Every other combination is no pair.
 *   3. one Jacobi iteration with constraint averaging, every pair from the velocities of the iteration's start:
 *        vn = nx * (ubx - uax) + ny * (uby - uay);  ca = (px - Pax) * ny - (py - Pay) * nx;  wa = ma + ia * (ca * ca);
 *        cb, wb likewise;  w = wa + wb.  A container with m = Rc - R > 0 first bends its gap to the wall -- a centre that
 *        slides h vt along a circle leaves it by (h vt)^2 / (2 d) although g + h vn says it stays --: with the velocities
 *        of the disc at its centre and of the container at its centre, o the unit vector from the one to the other,
 *        vt = ox * (udy - ucy) - oy * (udx - ucx);  s = h * vt;  q2 = m * m - s * s;  q2 < 0: q2 = 0;  g = sqrt(q2) - d
 *        (which is (Rc - R) - d when nothing slides).  The pair FIRES when w > 0 and g + h * vn < 0 (speculative: what would overlap
 *        at the next sub-step's pose), and then
 *        e = max(ea, eb);  t1 = (-g) / h;  t2 = -(e * vn);  target = t1 > t2 ? t1 : t2;  lam = (target - vn) / w
 *      b takes the impulse lam n at p, a takes -(lam n).  Collider k sums its impulses J over its partners in ascending
 *      index (sx, sy, and sz = sz + ((px - Pkx) * Jy - (py - Pky) * Jx)), and with count fired pairs, count > 0:
 *        mk > 0: vx = vx + (sx * mk) / count (y likewise);   ik > 0: omega = omega + (sz * ik) / count
 *   4. `iterations` of these, each from the one before; then a collider with ik > 0 recomputes its turn (c, s) from the
 *      new omega with the four lines of the integrator.
 * tests/contact_model.py is the definition; the device equals it bit for bit.  Contacts change velocities, spins and turns
 * only -- no particle, no load sum, no geometry --, so the commit, the read-back and a failed step are those of bodies.
 * The limits: no friction between bodies (a ball slides on a tilted plate); no pair without a disc; explicit and averaged,
 * so stacks are soft (DESIGN.md has the measured overlaps); a collider with both weights 0 is never moved and is a
 * kinematic partner; the pivot of a body rides with it only while its omega != 0 (step 2 of collider bodies), so a free
 * ball wants a spin, however small.  With e = 0 a body that would cross a partner within the sub-step is stopped where it
 * is and closes the rest in later sub-steps; it never arrives overlapped, and one that starts overlapped is pushed out in
 * one sub-step.  ONE handle only, as bodies: a device group refuses to step and egg_rx_begin returns EGG_ERR_UNSUPPORTED
 * while a handle holds a record that is on; exact order refuses such a list (EGG_ERR_UNSUPPORTED), and EGG_OPT_SOLVER_ORDER
 * refuses exact order while one is set.
 * egg_set_collider_contacts: n must equal the current collider count, or 0 (no collider meets another); iterations is
 * 1 .. 16, or 0 for the default of 4.  Everything is checked before anything changes: EGG_ERR_INVALID_ARGUMENT for an n that
 * does not match, a restitution that is not finite or outside [0, 1], an on that is not 0 or 1, a reserved that is not 0, or
 * iterations outside 0 .. 16.  egg_set_colliders with another list clears the records, as it clears the bodies.  Refused
 * while a step is in flight.
 * egg_get_collider_contact_solves: the fires, one per (pair, sub-step, iteration), over committed steps; a failed step adds
 * nothing. */
typedef struct {
    double restitution; /* 0 .. 1; a pair takes the larger of its two */
    int32_t on;         /* 0 or 1 */
    int32_t reserved;   /* 0 */
} egg_collider_contact; /* 16 bytes */
int egg_set_collider_contacts(egg_handle *h, int32_t n, const egg_collider_contact *c, int32_t iterations);
/* the records as stored, one per collider (off included): the count in *n, min(*n, cap) records copied, the iterations */
int egg_get_collider_contacts(const egg_handle *h, int32_t cap, egg_collider_contact *out, int32_t *n, int32_t *iterations);
int egg_get_collider_contact_solves(egg_handle *h, int64_t *solves);

/* ---- collider pose and collider styles: colliders in the picture ("Collider styles") ----
 * Not in the reference, which has no colliders and so draws none.
 * THE POSE.  Beside the list egg_get_colliders returns, a handle keeps the list as it stood at the START of the last
 * committed relaxed step -- what last_x / last_y are for the particles.  Every committed relaxed step copies the current
 * list into it just before the commit advances the list, whether or not anything moves; a failed or discarded step and the
 * motion, spin, surface and body setters leave it alone; egg_set_colliders sets BOTH lists to the new list, so a teleport
 * is not interpolated.  egg_get_collider_pose returns the list with every parameter
 *   p[i] = last.p[i] * (1.0 - t) + cur.p[i] * t        FP64, in exactly this order, on the host,
 * t = alpha clamped to [0, 1], or the handle's interpolation_alpha where alpha is NaN (as egg_render treats its own);
 * kind and type_mask are the current list's.  The count goes to *n, min(*n, cap) colliders are copied.  It is the pose the
 * renderer draws, for a host that draws the colliders itself between two steps.  Two consequences of mixing parameters:
 *   - a turning collider moves along the chord, not the arc: at 2 rad/s and 60 steps/s the step turns 1/30 rad and the
 *     chord's midpoint lies 1 - cos(1/60) = 1.4e-4 of the lever arm inside the arc;
 *   - a half-plane's mixed normal is not renormalised, as it is not after a turn: between two steps of a turning half-plane
 *     its length is below 1 by the same 1.4e-4.
 * STYLES.  Every collider of the list may carry a STYLE; the default is undrawn, and a list without a visible style makes
 * egg_render, egg_group_render and egg_draw_source_render launch exactly what they launch without and return the same bits.
 * A collider is VISIBLE when fill[3] > 0 and its kind has an inside (HALF_PLANE: the side n . pos < off, DISC: inside,
 * CONTAINER: outside the circle -- the solid side), or when line[3] > 0 && line_width > 0.  One kernel draws the visible
 * colliders of layer 0 onto the cleared screen, before the eggs, and one those of layer 1 after the eggs -- whether or not
 * the eggs are drawable: the boundary is visible before the first step.  Each launch counts in stats.kernel_launches.
 * Per screen pixel (i, j): wx = ((double)i + 0.5) + origin_x, wy likewise; the visible colliders of the layer in list order,
 * each at the pose of the frame's t, with the signed distance sd in FP64, in exactly this order, no contraction:
 *   HALF_PLANE  (nx * wx + ny * wy) - off
 *   DISC        dx = wx - cx, dy = wy - cy, sqrt(dx * dx + dy * dy) - R;    CONTAINER  R - sqrt(dx * dx + dy * dy)
 *   SEGMENT, WALL  e, l2, t, q as egg_set_colliders defines them for the position (wx, wy); ddx = wx - qx, ddy = wy - qy,
 *               sd = sqrt(ddx * ddx + ddy * ddy); no inside
 *   cf = (float)fmin(fmax(0.5 - sd, 0.0), 1.0), 0 for a kind without an inside;
 *   cl = (float)fmin(fmax((0.5 + 0.5 * (double)line_width) - fabs(sd), 0.0), 1.0) when line_width > 0, else 0;
 *   cf > 0 && fill[3] > 0: out = blend(out, (fill.rgb, fill[3] * cf)); then cl > 0 && line[3] > 0: the same with line, cl;
 *   blend is the "alpha" blend of the composite in float32: rgb = src.rgb * src.a + dst.rgb * (1 - src.a), a = src.a +
 *   dst.a * (1 - src.a).  A collider whose coverage at a pixel is 0 does not touch the pixel (a -0.0 stays -0.0).
 * egg_set_collider_styles: n must equal the current collider count, or 0 (nothing is drawn).  Everything is checked before
 * anything changes: EGG_ERR_INVALID_ARGUMENT, with the collider's index in the message, for an n that does not match, a
 * colour component that is not finite or outside [0, 1], a width that is not finite or outside [0, 64], a layer other than
 * 0 or 1.  Accepted in either solver order (it only ever draws a list that exists).  egg_set_colliders resets the styles to
 * undrawn; the motion, spin, surface, body and load setters leave them.  Refused while a step is in flight. */
typedef struct {
    float fill[4];      /* straight-alpha RGBA of the solid side; ignored by SEGMENT and WALL, which have no inside */
    float line[4];      /* RGBA of the outline / of the segment itself */
    float line_width;   /* px, 0 .. 64; 0: no line */
    int32_t layer;      /* 0: under the eggs (after the clear, before the white canvas); 1: over them */
} egg_collider_style; /* 40 bytes */
int egg_set_collider_styles(egg_handle *h, int32_t n, const egg_collider_style *s);
/* the styles as stored, one per collider (undrawn ones all zero): the count in *n, min(*n, cap) records copied */
int egg_get_collider_styles(const egg_handle *h, int32_t cap, egg_collider_style *s, int32_t *n);
int egg_get_collider_pose(egg_handle *h, double alpha, int32_t cap, egg_collider *c, int32_t *n);

/* ---- force fields (not in the reference, which has no forces as it has no boundary; DESIGN.md section 2.7, "Forces") ----
 * A handle holds an ordered list of at most EGG_MAX_FORCES fields.  The values are accelerations in px/s^2 and do not depend
 * on mass.  In every sub-step of a RELAXED step, for every particle of a type, the force step runs before the pre-solve,
 * which then runs unchanged (it damps, integrates and applies the follow constraint).  (x, y) is the position at the start
 * of the sub-step, (vx, vy) the velocity the pre-solve is about to damp, im the inverse mass:
 *   1. !(im > eps): the particle takes no force (the follow constraint's own test for an immovable particle).
 *   2. ax = +0.0, ay = +0.0; for every field with the type in `type_mask` (bit 0 white, bit 1 yolk), in list order:
 *      UNIFORM p = (gx, gy, -, -): ax = ax + gx, ay = ay + gy.
 *      RADIAL  p = (cx, cy, strength, R): dx = cx - x, dy = cy - y, d2 = dx dx + dy dy; d2 < R R && d2 > 0:
 *              d = sqrt(d2), w = 1 - d / R, s = strength w, ax = ax + (dx / d) s, ay = ay + (dy / d) s.  A positive strength
 *              attracts, a negative one repels; the falloff is linear, down to 0 at the edge; at d2 == 0 nothing.
 *      VORTEX  p = (cx, cy, strength, R): the same dx, dy, d2, d, w, s and condition;
 *              ax = ax + (-(dy / d)) s, ay = ay + (dx / d) s.
 *   3. vx = vx + sub_delta ax, vy = vy + sub_delta ay.
 * FP64 in exactly this order, no contraction; every comparison is false for a NaN.  The force is damped together with the
 * velocity, so a particle in free fall reaches a terminal speed.  Parameters a kind does not use are stored as 0.  An
 * acceleration that throws a particle beyond cell +-2^30 fails the step as any such position does, with nothing committed.
 * The fields do not move and are not drawn; a caller re-sets the list between steps to vary them.
 * Relaxed order only, as the colliders: a non-empty list on a handle in exact order is EGG_ERR_UNSUPPORTED, and
 * EGG_OPT_SOLVER_ORDER = 0 is EGG_ERR_UNSUPPORTED while the list is not empty; an empty list is always accepted.
 * egg_set_forces checks everything before it changes anything: EGG_ERR_INVALID_ARGUMENT, with the field's index in the
 * message, for n outside 0 .. EGG_MAX_FORCES, an unknown kind, a mask that is 0 or has bits beyond 3, a parameter that is
 * not finite, R <= 0 for RADIAL or VORTEX.  Refused while a step is in flight.  The list goes to the device when it is set,
 * never per step; with an empty list a step launches exactly what it launches without, and with one as many kernels. */
#define EGG_MAX_FORCES 16
enum { EGG_FORCE_UNIFORM = 0, EGG_FORCE_RADIAL = 1, EGG_FORCE_VORTEX = 2 };
typedef struct {
    int32_t kind;      /* EGG_FORCE_* */
    int32_t type_mask; /* bit 0 white, bit 1 yolk; never 0 */
    double p[4];
} egg_force; /* 40 bytes */
int egg_set_forces(egg_handle *h, int32_t n, const egg_force *f); /* n == 0 clears */
/* the list as stored: the count in *n, min(*n, cap) fields copied */
int egg_get_forces(const egg_handle *h, int32_t cap, egg_force *f, int32_t *n);

/* ---- viscosity (not in the reference, whose cohesion_strength moves nothing; DESIGN.md section 2.7, "Viscosity") ----
 * XSPH velocity smoothing with a coefficient c per particle type, 0 (the default) = off.  For a type with c in (0, 1], every
 * sub-step of a RELAXED step runs one more pass after its last collision pass (that pass's collider projection included)
 * and before the post-solve.  Positions are not touched: the pass rewrites the start-of-sub-step positions `prev` from
 * which the post-solve takes the velocity, so the committed velocity and the next sub-step's prediction are the smoothed
 * ones and every collision distance and collider constraint stays as the last pass left it.  With p_i the position of
 * particle i, u_i = (p_i.x - prev_i.x, p_i.y - prev_i.y) its displacement in this sub-step (every u taken before any prev
 * is rewritten) and H the type's spatial-hash cell size of the step:
 *   1. cells are built fresh from the positions, as in a collision pass;
 *   2. candidates and visit order are a collision pass's: 3x3 cells, x offset outer, y offset inner, ascending key inside
 *      a cell, j != i;
 *   3. for each candidate j: dx = p_j.x - p_i.x, dy = p_j.y - p_i.y, d2 = dx dx + dy dy; !(d2 < H H): skipped; otherwise
 *      d = sqrt(d2), w = 1 - d / H, sw = sw + w, sx = sx + w (u_j.x - u_i.x), sy = sy + w (u_j.y - u_i.y); the three sums
 *      start at +0.0 (a coincident pair has w = 1; the 3x3 cells cover the whole disc of radius H);
 *   4. !(inv_mass_i > eps) or !(sw > 0): prev_i keeps its bits;
 *   5. otherwise nux = u_i.x + c (sx / sw), nuy = u_i.y + c (sy / sw), prev_i = (p_i.x - nux, p_i.y - nuy): a convex blend of
 *      the particle's displacement and its neighbours' weighted mean, stable for every c in [0, 1].
 * FP64 in exactly this order, no contraction; every comparison is false for a NaN.  Pairs of any batch smooth each other;
 * white and yolk do not (their one interaction is egg_set_coupling).  pair_solves and max_pass_visits do not change; egg_get_viscosity_pairs counts, per type,
 * the distinct pairs with d2 < H H over the viscosity passes of committed steps (a failed or discarded step adds nothing).
 * Relaxed order only, as the colliders: a non-zero coefficient on a handle in exact order is EGG_ERR_UNSUPPORTED, and
 * EGG_OPT_SOLVER_ORDER = 0 is EGG_ERR_UNSUPPORTED while a coefficient is not zero; both zero is always accepted.  A
 * coefficient outside [0, 1] or NaN is EGG_ERR_INVALID_ARGUMENT and changes nothing.  Refused while a step is in flight.
 * With both coefficients zero a step launches exactly what it launches without; a type with c > 0 adds five launches per
 * sub-step. */
int egg_set_viscosity(egg_handle *h, const double c[2]); /* c[EGG_WHITE], c[EGG_YOLK] */
int egg_get_viscosity(const egg_handle *h, double c[2]);
int egg_get_viscosity_pairs(egg_handle *h, int64_t pairs[2]);

/* ---- white-yolk coupling (not in the reference, whose two types never see each other, L:1776-1786; DESIGN.md section
 * 2.7, "Coupling") ----
 * One cross-type collision pass per sub-step of a RELAXED step.  A handle holds two doubles that both types share: the
 * distance `factor` (finite, >= 0; 0, the default, = off) and the `strength` in [0, 1] (default 1).  The pass runs only
 * while factor > 0 and both types have particles, once per sub-step, BEFORE the sub-step's first collision pass:
 *   1. pre-solve + follow, both types;  2. the coupling pass, both types;  3. the C collision passes;  4. viscosity.
 * So colliders and walls keep the last word: a wall's sweep reads `prev`, which the coupling pass does not touch.  It is
 * a Jacobi pass with constraint averaging like the collision pass:
 *   cells       H = max(1.0, factor (white max_radius + yolk max_radius)) from the two configs; the cell of a particle is
 *               floor(x / H), floor(y / H); each type gets a table of its own over the positions the pre-solve + follow
 *               has just written.  A radius never exceeds its config's max_radius, so every pair within the coupling
 *               distance lies inside a 3x3 neighbourhood.
 *   candidates  of particle i of one type: every particle of the OTHER type in i's 3x3 cells, x offset -1..1 outer, y
 *               offset inner, ascending key inside a cell (the key: the particle's index within its type).
 *   pair        a is always the white particle, b the yolk one: both sides evaluate one expression, the collision
 *               correction's, with md = factor (ra + rb), compliance = (1 - strength) / sub_delta^2 (L:1337-1341) and the
 *               white config's eps.  wsum < eps: skipped, uncounted; d2 <= md md: fires; divisor < eps: zeros;
 *               current < eps: zero normal; clamp to +-|violation|; a coincident pair (d2 == 0) takes the normal
 *               DIRS[(b - a) & 7] of the two keys.  White takes (cax, cay), yolk (cbx, cby).
 *   update      x_i = x_i + (sx omega) / n_i when n_i pairs fired (omega: EGG_OPT_RELAXATION), else the position is
 *               copied; every pair of the pass reads the start-of-pass positions of both types.
 * egg_get_coupling_solves: the distinct cross pairs that fired, over committed steps (a failed or discarded step adds
 * nothing); pair_solves, max_pass_visits and every other counter are unchanged.  A NaN position or a cell beyond +-2^30 at
 * cell size H fails the step like any bad cell: nothing is committed.  A step whose H H is not finite (an absurd factor)
 * fails with EGG_ERR_INVALID_ARGUMENT before anything is launched.
 * ALL pairs of both types couple, whatever their batch: there is no batch tag and no adhesion band -- nothing pulls a yolk
 * back to its white.  ONE handle only: a device group refuses to step and egg_rx_begin returns EGG_ERR_UNSUPPORTED while
 * factor > 0 (the halo carries no ghosts of the other type).
 * Relaxed order only, as viscosity: factor > 0 on a handle in exact order is EGG_ERR_UNSUPPORTED, and
 * EGG_OPT_SOLVER_ORDER = 0 is EGG_ERR_UNSUPPORTED while factor > 0; factor == 0 is always accepted.  A NaN, negative or
 * infinite factor, or a strength outside [0, 1], is EGG_ERR_INVALID_ARGUMENT and changes nothing.  Refused while a step is
 * in flight.  With factor 0, or one type without particles, a step enqueues and launches exactly what it does without;
 * with coupling a sub-step adds five launches per type. */
int egg_set_coupling(egg_handle *h, double factor, double strength);
int egg_get_coupling(const egg_handle *h, double *factor, double *strength);
int egg_get_coupling_solves(egg_handle *h, int64_t *solves);

/* ---- white-yolk adhesion (not in the reference; DESIGN.md section 2.7, "Adhesion") ----
 * An option of its own beside coupling: a same-batch BAND in the coupling pass, which pulls a yolk back to its white the way
 * effective cohesion holds one type's batch together.  A handle holds two more doubles: `reach` (finite, >= 0; 0, the
 * default, = off) and `strength` in [0, 1] (default 1).  Adhesion ACTS in a relaxed step exactly when all three hold:
 *   1. coupling acts (its factor > 0 and both types have particles);  2. reach > factor;  3. the solver order is relaxed.
 * When it does not act -- reach == 0, reach <= factor (an empty band), coupling off, one type empty -- a step launches
 * the kernels it launched before, with the same arguments, in the same enqueue order.  When it acts, the coupling pass
 * above changes in three places and nowhere else:
 *   cells       H = max(1.0, max(factor, reach) (white max_radius + yolk max_radius)): both types' tables and the pass use
 *               it.  Candidates, visit order and the wsum < eps skip are unchanged; a step whose H H is not finite fails
 *               with EGG_ERR_INVALID_ARGUMENT before anything is launched.
 *   pair        (a white, b yolk), md = factor (ra + rb), rd = reach (ra + rb), d2 from the start-of-pass positions:
 *               d2 <= md md: the coupling correction, exactly as without adhesion.  Otherwise, when a and b belong to the
 *               same batch and d2 <= rd rd: the adhesion branch -- the same expressions in the same order with the TARGET
 *               distance md and the compliance (1 - strength) / sub_delta^2 of adhesion's own strength.  divisor < eps:
 *               zeros; current < eps: zero normal; clamp to +-|violation|.  Here violation > 0: the pair is pulled
 *               together, and its own correction never brings it closer than md.  A pair fires at most one branch; n_i
 *               counts fires of either kind; shares add in visit order; the update rule is unchanged.
 *   same batch  two particles are of the same batch iff the same egg_add (egg_import_batch) created them.
 * egg_get_adhesion_solves: the distinct cross pairs whose adhesion branch fired, over committed steps (a failed or
 * discarded step adds nothing); egg_get_coupling_solves keeps counting coupling-branch fires only, and every other counter
 * is unchanged.
 * The limits are coupling's.  Relaxed order only: reach > 0 on a handle in exact order is EGG_ERR_UNSUPPORTED, and
 * EGG_OPT_SOLVER_ORDER = 0 is EGG_ERR_UNSUPPORTED while reach > 0; reach == 0 is always accepted.  reach > 0 with
 * factor == 0 is accepted and does nothing until coupling is on.  A single handle only: a device group refuses to step and
 * egg_rx_begin returns EGG_ERR_UNSUPPORTED while reach > 0.  A NaN, negative or infinite reach, or a strength outside
 * [0, 1], is EGG_ERR_INVALID_ARGUMENT and changes nothing.  Refused while a step is in flight.  While it acts a sub-step
 * launches as many kernels as with coupling alone: the rank and the couple kernel run in their tagged instantiations. */
int egg_set_adhesion(egg_handle *h, double reach, double strength);
int egg_get_adhesion(const egg_handle *h, double *reach, double *strength);
int egg_get_adhesion_solves(egg_handle *h, int64_t *solves);

/* ---- yolk containment (not in the reference; DESIGN.md section 2.7, "Containment") ----
 * Adhesion is a soft band, not a container.  Containment is the container: a DISC around the centroid of a batch's white,
 * sized from the white's own spread, that no yolk particle of that batch may leave.  A handle holds two more doubles:
 * `factor` (finite, >= 0; 0, the default, = off) and `strength` in [0, 1] (default 1).  Containment ACTS in a relaxed step
 * on a handle when factor > 0 and that handle holds particles of both types; it does not depend on coupling or adhesion.
 * (Every batch has particles of both types, so a handle holds both or neither: a handle without batches launches nothing more.)
 * When it does not act a step launches exactly the kernels it launched before, with the same arguments, in the same
 * enqueue order.  When it acts, every sub-step runs: 1. pre-solve + follow of both types; 2. the coupling pass, if coupling
 * acts; 3. containment; 4. the collision passes; 5. viscosity, if on.  Colliders and walls keep the last word, and the
 * positions at the start of the sub-step (which the walls sweep from) are not touched.
 *   summary     of a batch's white, over the n white positions v[0 .. n) of the batch that enter the sub-step's first
 *               collision pass.  wsum(v): 64 accumulators a[0 .. 63] start at +0.0; for k = l, l + 64, ... < n ascending,
 *               a[l] = a[l] + v[k]; then for d = 32, 16, 8, 4, 2, 1: a[l] = a[l] + a[l ^ d] for all l at once; the result
 *               is a[0].  cx = wsum(x) / n, cy = wsum(y) / n, q[k] = (x[k] - cx) (x[k] - cx) + (y[k] - cy) (y[k] - cy),
 *               rho = sqrt(wsum(q) / n), L = factor rho; n == 0: L = +inf (defined so that an empty white
 *               contains nothing; egg_add and egg_import_batch refuse a batch without particles of a type, so it does
 *               not arise).  IEEE double, no contraction.  This summation order is part of the rule.
 *   projection  of a yolk particle of the same batch, at the position that would enter the yolk's first collision pass:
 *               dx = x - cx, dy = y - cy, d = sqrt(dx dx + dy dy); if d > L (false for a NaN):
 *               keep = L + (1 - strength) (d - L), s = keep / d, x = cx + dx s, y = cy + dy s.  One hit.  No mass test.
 *   one-way     the white is never moved: a disc, not the white's outline, and it does not hold the white together.
 * egg_get_containment_hits: the projections, one per (yolk particle, sub-step), over committed steps (a failed or discarded
 * step adds nothing).  Containment adds no failure path: a NaN in the white gives a NaN centre and every comparison is false.
 * Relaxed order only: factor > 0 on a handle in exact order is EGG_ERR_UNSUPPORTED, and EGG_OPT_SOLVER_ORDER = 0 is
 * EGG_ERR_UNSUPPORTED while factor > 0; factor == 0 is always accepted.  A NaN, negative or infinite factor, or a strength
 * outside [0, 1], is EGG_ERR_INVALID_ARGUMENT and changes nothing.  Refused while a step is in flight.  A batch lives wholly
 * on one handle, so containment also works on device groups and through egg_rx_* (sharded ranks), where coupling and adhesion
 * do not.  While it acts a sub-step launches one kernel more per type: the summary on the white, the projection on the yolk. */
int egg_set_containment(egg_handle *h, double factor, double strength);
int egg_get_containment(const egg_handle *h, double *factor, double *strength);
int egg_get_containment_hits(egg_handle *h, int64_t *hits);

/* ---- sensors: count and locate the particles inside caller-set regions (csrc/eggsim_sensors.hip) ----
 * Not in the reference.  A handle holds an ordered list of at most EGG_MAX_SENSORS regions; a READ reports, per region and
 * particle type, how many particles lie inside and the integer sums their centroid follows from.  Sensors only observe: a
 * step with a list set launches exactly the kernels it launches without one, with the same arguments, and a read changes
 * no particle and no step counter.  They read the COMMITTED positions -- the arrays egg_download_particles returns for
 * EGG_FIELD_X / EGG_FIELD_Y, not interpolated --, so they work in exact and in relaxed order alike.
 * A particle of type w at the committed (x, y) is INSIDE sensor k when type_mask has bit w (bit 0 white, bit 1 yolk) and the
 * test of the kind holds.  FP64 in exactly this order, no contraction; every comparison is false for a NaN, so a NaN
 * position is inside nothing.  Only the particle's centre counts: its radius is not read.
 *   HALF_PLANE  p = (nx, ny, off, -, -, -): s = (nx x + ny y) - off; inside iff s >= 0.0.  The side the normal points to: the
 *               side on which a collider with the same parameters keeps its particles.  The normal is normalised when the
 *               list is set, by the collider rule (len = sqrt(nx nx + ny ny), nx = nx / len, ny = ny / len); a normal shorter
 *               than the white config's eps is refused.
 *   DISC        p = (cx, cy, R, -, -, -): dx = x - cx, dy = y - cy, d2 = dx dx + dy dy; inside iff d2 <= R R.
 *   BOX         p = (cx, cy, hx, hy, ux, uy): (ux, uy) is the box's first axis, normalised when the list is set as a normal
 *               is.  dx = x - cx, dy = y - cy, u = dx ux + dy uy, v = dy ux - dx uy; inside iff fabs(u) <= hx && fabs(v) <= hy.
 *   CAPSULE     p = (x0, y0, x1, y1, R, -): e, l2, t and q exactly as the SEGMENT collider defines them, l2 == 0 included;
 *               dx = x - qx, dy = y - qy, d2 = dx dx + dy dy; inside iff d2 <= R R.  A band around a wall.
 * Parameters a kind does not use are stored as 0.
 * A particle that is inside sensor k contributes count[w] += 1, sx[w] += llrint(x * EGG_SENSOR_POSITION_SCALE),
 * sy[w] += llrint(y * EGG_SENSOR_POSITION_SCALE) to reading k (int64, round to nearest, ties to even).  If one of the two
 * scaled values is not finite or reaches 2^53 in magnitude, the particle is left out of all three and dropped[w] counts it,
 * once for every sensor it is inside: dropped is ONE pair of counters per read, not one per sensor.  The centroid of type w
 * in sensor k is ((double)sx[w] / EGG_SENSOR_POSITION_SCALE) / (double)count[w], in that order, and likewise for y; there is
 * none while count[w] == 0.  The resolution is 2^-16 px.  Integer addition is associative: a device group and sharded ranks
 * answer with one handle's numbers bit for bit.  The sums wrap only beyond 2^63.
 * egg_set_sensors checks everything before it changes anything and returns EGG_ERR_INVALID_ARGUMENT, with the sensor's index
 * in the message, for: n outside 0 .. EGG_MAX_SENSORS, an unknown kind, a type_mask that is 0 or has bits beyond 3, a
 * parameter that is not finite, R, hx or hy < 0, a normal or axis shorter than eps.  n == 0 clears the list.  Accepted in
 * either solver order; refused while a step is in flight.  egg_get_sensors returns the list as stored, normalised.
 * egg_read_sensors takes one reading of the state as committed now: min(*n, cap) readings, the two dropped counters.
 * egg_read_sensor_batches gives the counts only, for the listed batches in the caller's order:
 * counts[(i * n_sensors + k) * 2 + w] = particles of type w of batch ids[i] inside sensor k.  An unknown id returns
 * EGG_ERR_UNKNOWN_ID and nothing is written; a repeated id is answered twice.  A dropped particle is not counted here either.
 * Both reads are refused while a step is in flight, succeed with an empty list (*n = 0, nothing is written to counts) and
 * with a handle that holds no particles (zeros), and are not cached: every call measures.
 * Limits: centres only (no radius, no overlap test); no velocity or mass sums; no sensor that rides on a collider (a caller
 * re-sets the list from egg_get_colliders); at most 64. */
#define EGG_MAX_SENSORS 64
#define EGG_SENSOR_POSITION_SCALE 65536.0 /* 2^16 */
enum { EGG_SENSOR_HALF_PLANE = 0, EGG_SENSOR_DISC = 1, EGG_SENSOR_BOX = 2, EGG_SENSOR_CAPSULE = 3 };
typedef struct { int32_t kind; int32_t type_mask; double p[6]; } egg_sensor;   /* 56 bytes */
typedef struct { int64_t count[2], sx[2], sy[2]; } egg_sensor_reading;         /* 48 bytes; [0] white, [1] yolk */
int egg_set_sensors(egg_handle *h, int32_t n, const egg_sensor *sensors);
int egg_get_sensors(const egg_handle *h, int32_t cap, egg_sensor *out, int32_t *n);
int egg_read_sensors(egg_handle *h, int32_t cap, egg_sensor_reading *readings, int64_t dropped[2], int32_t *n);
int egg_read_sensor_batches(egg_handle *h, int64_t n_ids, const int64_t *ids, int32_t *counts /* [n_ids][n_sensors][2] */);

/* ---- probes: the nearest particle to a point and the first hit along a ray (csrc/eggsim_probes.hip) ----
 * Not in the reference.  Sensors answer "what is inside this region" with sums; a probe answers "what is here" with the
 * IDENTITY of one particle: the egg under the cursor, the first egg a line of sight meets, the particle nearest a utensil's
 * tip.  A call is STATELESS: the caller passes at most EGG_MAX_PROBES probes with the call and the handle stores neither the
 * list nor an answer.  Probes only observe: a step launches exactly the kernels it launches without them, and a call changes
 * no particle and no counter, those of egg_get_stats included.  They read the COMMITTED state -- the arrays
 * egg_download_particles returns for EGG_FIELD_X / EGG_FIELD_Y / EGG_FIELD_RADIUS, not interpolated --, so they work in
 * exact and in relaxed order alike.
 * A particle of type w at the committed (x, y) with radius r is a CANDIDATE of probe k when type_mask has bit w (bit 0 white,
 * bit 1 yolk) and the rule of the kind holds.  FP64 in exactly this order, no contraction, sqrt and / correctly rounded;
 * every comparison is false for a NaN, so a NaN position or radius is a candidate for nothing.
 *   POINT  p = (px, py, reach, -, -): dx = x - px, dy = y - py, d2 = dx dx + dy dy; candidate iff d2 <= reach reach && r == r;
 *          score = d2.  Only the centre is compared; the hit reports the radius, so a caller who asks "is the cursor ON a
 *          particle" tests score <= radius * radius itself.  reach is finite and >= 0, or +inf: the nearest, wherever it is.
 *   RAY    p = (x0, y0, x1, y1, pad): the first disc of radius R = r + pad that the segment from (x0, y0) to (x1, y1) enters.
 *          fx = x0 - x, fy = y0 - y, c = (fx fx + fy fy) - R R.  If c <= 0.0 the ray starts in or on the disc: candidate with
 *          t = 0.0.  Otherwise ex = x1 - x0, ey = y1 - y0, l2 = ex ex + ey ey, b = fx ex + fy ey; a miss unless b < 0.0;
 *          q = b b - l2 c; a miss unless q >= 0.0; t = (-b - sqrt(q)) / l2; a miss unless t <= 1.0.  score = t; the point of
 *          impact is (x0 + t ex, y0 + t ey).  pad is finite and >= 0; a ray whose l2 is below the white config's eps squared
 *          (or not finite) is refused.  t is never negative: sqrt(q) <= -b after rounding when c > 0.
 * Parameters a kind does not use are ignored.
 * The WINNER of probe k and type w is, among the candidates of type w, the one with the smallest score by < on doubles;
 * among equal scores the smallest batch key (egg_batch_info.key, the batch's position in the global creation order), then
 * the smallest index inside the batch's run of that type.  A handle lays its particles out in ascending key, so on one
 * handle that is the lowest array index; across the handles of a group and across ranks the same rule is well defined.
 * hits[2 k + w] reports found = 1, the batch's id, its key, the particle's 0-based index in the batch's run of that type (in
 * download order), the score and the particle's committed x, y, radius.  With no candidate -- also for a type the mask does
 * not cover -- found = 0 and every other field is 0.
 * egg_probe checks everything before it launches anything and returns EGG_ERR_INVALID_ARGUMENT, with the probe's index in
 * the message and hits untouched, for: n outside 0 .. EGG_MAX_PROBES, n > 0 without a list or without hits, an unknown kind,
 * a type_mask that is 0 or has bits beyond 3, a NaN in a parameter the kind uses, an infinity anywhere but a POINT's reach, a
 * negative reach or pad, a degenerate ray.  n == 0 succeeds and writes nothing.  A handle without particles answers
 * found = 0 everywhere and launches nothing; a type that no probe's mask covers contributes no work.  Refused while a step
 * is in flight (egg_step_begin or egg_rx_begin open).  Nothing is cached: every call measures.
 * Limits: centres for POINT, discs for RAY; one winner per type, no k-nearest; no probe that rides on a collider; colliders
 * themselves are not hit; at most 64 per call. */
#define EGG_MAX_PROBES 64
enum { EGG_PROBE_POINT = 0, EGG_PROBE_RAY = 1 };
typedef struct { int32_t kind; int32_t type_mask; double p[5]; } egg_probe_query;                                             /* 48 bytes */
typedef struct { int64_t id, key; int32_t index, found; double score, x, y, radius; } egg_probe_hit;                          /* 56 bytes */
int egg_probe(egg_handle *h, int32_t n, const egg_probe_query *probes, egg_probe_hit *hits /* [n][2]: [0] white, [1] yolk */);

/* ---- fields: the particles binned into a caller-set grid (csrc/eggsim_fields.hip) ----
 * Not in the reference.  Sensors answer "what is inside this region", a probe "what is here"; a field answers "where is the
 * egg" with a MAP: per cell of a regular grid and particle type the number of particles and, on request, the integer sums
 * their mean velocity follows from -- an occupancy map, a velocity map, an observation tensor.  A call is STATELESS: the
 * caller passes the grid with the call and the handle stores neither the grid nor an answer; nothing is cached.  Fields only
 * observe: a step launches exactly the kernels it launches without them, and a call changes no particle; of egg_get_stats
 * only kernel_launches moves, by one per call that launches.  They read the COMMITTED state -- the arrays
 * egg_download_particles returns for EGG_FIELD_X / EGG_FIELD_Y / EGG_FIELD_VX / EGG_FIELD_VY, not interpolated --, so they
 * work in exact and in relaxed order alike.
 * The grid has nx x ny square cells of side `cell` px, cell (0, 0) with its lower corner at (x0, y0).  Take a particle of
 * type w whose bit is in type_mask (bit 0 white, bit 1 yolk) at the committed (x, y) with the committed velocity (vx, vy).
 * FP64 in exactly this order, no contraction: inv = 1.0 / cell, computed ONCE on the host; fx = (x - x0) * inv;
 * fy = (y - y0) * inv.  The particle is INSIDE iff fx >= 0.0 && fx < (double)nx && fy >= 0.0 && fy < (double)ny; every
 * comparison is false for a NaN, so a NaN position is outside.  Its cell is ix = (int)fx, iy = (int)fy (truncation; -0.0 is
 * cell 0), index iy * nx + ix.  Only the particle's centre counts: its radius is not read.
 *   outside     outside[w] += 1 and nothing else.
 *   dropped     inside, svx / svy requested, and vx * EGG_FIELD_VELOCITY_SCALE or vy * EGG_FIELD_VELOCITY_SCALE is not
 *               finite or reaches 2^53 in magnitude: dropped[w] += 1 and nothing else (the sensors' rule).
 *   counted     otherwise: inside[w] += 1, count[w][cell] += 1, svx[w][cell] += llrint(vx * EGG_FIELD_VELOCITY_SCALE),
 *               svy[w][cell] += llrint(vy * EGG_FIELD_VELOCITY_SCALE) (int64, round to nearest, ties to even).
 * Every plane is [2][ny][nx], row-major, [0] white, [1] yolk.  count is required; svx and svy are given together or not at
 * all, and without them the velocities are not read and dropped is 0.  The planes of a type outside the mask, or without
 * particles, are all zero.  inside[w] + outside[w] + dropped[w] = the particles of type w, for every w in the mask.  The mean
 * velocity of a cell is ((double)svx / EGG_FIELD_VELOCITY_SCALE) / (double)count, in that order, and likewise for y; there is
 * none while the count is 0.  The resolution is 2^-16 px per unit of time.  Integer addition is associative: a device group
 * and sharded ranks answer with one handle's numbers bit for bit.  Every term is below 2^53 in magnitude, so a cell's sum
 * wraps only beyond 2^63: not with fewer than 1,024 particles in one cell, whatever their velocities.  count is 32 bits: a
 * type holds fewer than 2^31 particles.
 * units_tiled / units_direct tell how the device did the work (units of at most 1,024 particles whose cells were summed on
 * chip first, or added one by one); they depend on the scene's layout in memory, not only on its particles, and are no
 * part of the answer.  path = EGG_FIELD_PATH_DIRECT sends every unit down the second way: a test hook, the planes are equal.
 * egg_field checks everything before it launches or writes anything and returns EGG_ERR_INVALID_ARGUMENT, naming the field,
 * with planes and totals untouched, for: a NULL spec or NULL planes; nx or ny below 1 or nx * ny above EGG_FIELD_MAX_CELLS;
 * a cell that is not finite, not above 0 or whose inverse is not finite; x0 or y0 not finite; a type_mask outside 1 .. 3; an
 * unknown path; count NULL; only one of svx / svy.  totals may be NULL.  Refused while a step is in flight (egg_step_begin
 * or egg_rx_begin open).  A scene without covered particles zero-fills the planes and launches nothing.
 * egg_field writes planes in host memory.  egg_field_to writes planes that live on the handle's device (a torch tensor's
 * data_ptr()): it zeroes them itself, adds into them in place -- no copy -- and returns after the stream is idle, so the
 * tensor is ready on return.  It refuses, as above, a plane pointer that is not aligned to its word (4 bytes for count, 8
 * for svx / svy), that is not memory of the handle's device, or whose allocation ends before the plane does.
 * Limits: centres only (no splat by radius, no area or mass plane); no per-batch planes; no field that rides on a collider;
 * no egg_field_to for groups or sharded ranks; at most 2^20 cells per call. */
#define EGG_FIELD_MAX_CELLS (1 << 20)          /* nx * ny */
#define EGG_FIELD_VELOCITY_SCALE 65536.0       /* 2^16 */
enum { EGG_FIELD_PATH_AUTO = 0, EGG_FIELD_PATH_DIRECT = 1 };   /* DIRECT: test hook, see the kernel */
typedef struct { double x0, y0, cell; int32_t nx, ny, type_mask, path; } egg_field_spec;     /* 40 bytes */
typedef struct { int32_t *count; int64_t *svx, *svy; } egg_field_planes;                     /* each [2][ny][nx], row-major, [0] white [1] yolk */
typedef struct { int64_t inside[2], outside[2], dropped[2]; int32_t units_tiled, units_direct; } egg_field_totals; /* 56 bytes */
int egg_field(egg_handle *h, const egg_field_spec *spec, const egg_field_planes *host_out, egg_field_totals *totals);
int egg_field_to(egg_handle *h, const egg_field_spec *spec, const egg_field_planes *device_out, egg_field_totals *totals);

/* ---- pieces: the connected pieces of each batch (csrc/eggsim_pieces.hip) ----
 * Not in the reference.  Sensors, probes and fields say how much of the egg is where; pieces answer "is the egg still ONE
 * egg": has a wall cut it, has the yolk broken, how many particles have strayed, where is the body.  A call is STATELESS,
 * only observes (of egg_get_stats only kernel_launches moves, by at most 2 per call) and reads the COMMITTED state -- the
 * arrays egg_download_particles returns for EGG_FIELD_X / EGG_FIELD_Y / EGG_FIELD_RADIUS --, so it works in exact and in
 * relaxed order alike.  tests/pieces_model.py is the definition in numpy.
 * An ATOM is the particles of one type (white or yolk) of one live batch, numbered by their index in the batch, 0 .. n - 1
 * (the index of egg_probe_hit).  Two particles i and j of an atom are LINKED iff d2 <= L * L, FP64 in exactly this order,
 * no contraction:  dx = x[i] - x[j]; dy = y[i] - y[j]; d2 = dx * dx + dy * dy; L = reach[type] * (radius[i] + radius[j]).
 * The test is symmetric and false when anything in it is a NaN.  Particles of different batches or types are never linked.
 * A PIECE is a connected component of that graph; the LABEL of a particle is the lowest index in its piece; the BODY is the
 * largest piece, among pieces of equal size the one with the lower label.
 * Per requested batch and type one egg_piece_summary (out[i][0] white, out[i][1] yolk):
 *   n        particles of the atom; 0 for a type the mask leaves out or the batch lacks, and every other field is then 0
 *   pieces   number of pieces          largest  particles of the body          first  label of the body
 *   singles  pieces of exactly one particle
 *   dropped  body particles left out of the two sums by the sensors' rule: one of x, y times EGG_SENSOR_POSITION_SCALE is
 *            not finite or reaches 2^53 in magnitude
 *   sx, sy   int64 sums of llrint(x * EGG_SENSOR_POSITION_SCALE), llrint(y * EGG_SENSOR_POSITION_SCALE) over the body's
 *            particles that are not dropped; the body's centroid is ((double)sx / EGG_SENSOR_POSITION_SCALE) /
 *            (double)(largest - dropped), and likewise for y; there is none while largest == dropped.
 * n_ids = 0 with ids = NULL means every live batch in egg_list_ids order (out then holds that many pairs); an id may
 * repeat.  white_labels / yolk_labels are NULL or host memory for EVERY particle of the type (egg_download_particles order):
 * the label of every particle of a requested atom, -1 for a particle of an atom that was not asked for.
 * Every output is an integer and the fixed point of the labels is unique: the answer does not depend on the schedule, on
 * the device, or on how a scene is split over handles.
 * Everything is checked before anything is launched or written: EGG_ERR_INVALID_ARGUMENT for a NULL spec or out, n_ids < 0,
 * ids NULL with n_ids > 0, a reach that is not finite or not above 0, a type_mask outside 1 .. 3, a step in flight
 * (egg_step_begin or egg_rx_begin open); EGG_ERR_UNKNOWN_ID for an unknown id; EGG_ERR_UNSUPPORTED, naming the batch and
 * its count, for a requested atom of a covered type with more than EGG_PIECES_MAX_ATOM particles (the atom is solved in
 * the LDS of one compute unit).
 * Limits: no path for larger atoms; the solve tests all pairs of an atom per sweep (no neighbour grid); labels on one
 * handle only. */
#define EGG_PIECES_MAX_ATOM 4096
typedef struct { double reach[2]; int32_t type_mask; int32_t reserved; } egg_pieces_spec;                                     /* 24 bytes */
typedef struct { int32_t n, pieces, largest, first, singles, dropped; int64_t sx, sy; } egg_piece_summary;                  /* 40 bytes */
int egg_pieces(egg_handle *h, const egg_pieces_spec *spec, int64_t n_ids, const int64_t *ids,
               egg_piece_summary *out /* [n][2] */, int32_t *white_labels, int32_t *yolk_labels);

/* ---- several GPUs in one process (csrc/eggsim_group.cpp) -------------------------------------------------------
 * The multi-device form of the handle for a host that is ONE process (the LuaJIT wrapper): one egg_handle per device
 * behind one egg_group, x-slabs [cuts[k], cuts[k + 1]) of the plane per device (cuts: n_devices + 1 ascending values;
 * NULL with one device), global batch ids.  A batch is stepped by the device whose slab held its position when it was
 * added; batches whose claims for a step come within one spatial-hash cell of each other across devices are handed to
 * ONE device before that step runs (exact Gauss-Seidel order cannot cross a cut), so the results equal a
 * single handle's bit for bit.  A collision budget 0.05 N^2 (L:1752-1753) that could bind (few batches) needs every particle
 * of the type in one tile: the group then hands every batch to device 0 and steps there until batches are added or removed.  In relaxed order (egg_group_set_solver_order) nothing is handed over before a step: every
 * collision pass runs on every device over its own particles plus read-only ghost copies of its neighbours' particles
 * near it, and the results equal ONE relaxed handle holding every batch, bit for bit.  The same
 * device ordinal may appear more than once (several handles on one GPU: testing); different ordinals need peer access
 * for relaxed order.
 * egg_fluid_simulation_amd/sharding.py is the same protocol between processes over RCCL. */
typedef struct egg_group egg_group;
int egg_group_create(const egg_config *white, const egg_config *yolk, int32_t n_devices, const int32_t *devices,
                     const double *cuts, egg_group **out);
void egg_group_destroy(egg_group *g);
const char *egg_group_last_error(const egg_group *g);
int32_t egg_group_n_devices(const egg_group *g);
egg_handle *egg_group_handle(egg_group *g, int32_t k); /* the k-th device's handle, for downloads and statistics */
int egg_group_set_halo(egg_group *g, double halo_px);  /* how far outside its slab an island may idle before it is handed on (64) */
/* add / remove / set_target_position / get_position / update of SimulationHandler, ids global (L:27-135, L:140-155,
 * L:254-264, L:281-295, L:168-222) */
int egg_group_add(egg_group *g, double x, double y, double white_radius, double yolk_radius, int64_t white_n, int64_t yolk_n,
                  int64_t *out_id);
int egg_group_remove(egg_group *g, int64_t id);
int egg_group_set_target(egg_group *g, int64_t id, double x, double y);
int egg_group_get_position(egg_group *g, int64_t id, double *x, double *y);
int egg_group_update(egg_group *g, double delta, double step_delta, int32_t n_substeps, int32_t n_collision_steps,
                     int32_t *out_n_steps);
int egg_group_step(egg_group *g, double delta, int32_t n_substeps, int32_t n_collision_steps); /* _step directly */
/* which device index holds batch `id` now, and under which id of that device's handle */
int egg_group_owner(const egg_group *g, int64_t id, int32_t *device_index, int64_t *local_id);
int egg_group_get_counters(const egg_group *g, int64_t *migrations, int64_t *discarded_steps);
/* EGG_OPT_SOLVER_ORDER / EGG_OPT_RELAXATION for every handle of the group (same values and ranges; relaxation <= 0 keeps
 * the current value).  Relaxed order over handles on different devices needs peer access between them: EGG_ERR_UNSUPPORTED
 * otherwise.  Refused values change nothing. */
int egg_group_set_solver_order(egg_group *g, int32_t order, double relaxation);
/* EGG_OPT_COHESION for every handle of the group, with its rules (relaxed order only; back to exact order only with
 * cohesion off).  A refused value changes no handle.  Ghost records stay 40 bytes: a ghost's batch tag travels in the upper
 * 32 bits of its key word. */
int egg_group_set_cohesion(egg_group *g, int32_t mode);
/* egg_set_colliders for every handle of the group alike, with its rules (relaxed order only; back to exact order only
 * with an empty list); a refused list changes no handle.  Every device projects only the particles it owns, before their
 * positions travel as ghosts: the results equal one handle's.  The hits are summed over the handles. */
int egg_group_set_colliders(egg_group *g, int32_t n, const egg_collider *c);
int egg_group_get_colliders(const egg_group *g, int32_t cap, egg_collider *c, int32_t *n);
int egg_group_get_collider_hits(egg_group *g, int64_t hits[2]);
/* egg_set_collider_surfaces for every handle of the group alike, with its rules; a refused call changes no handle, and
 * egg_group_set_colliders resets the surfaces.  A step is refused while the handles differ.  The grips are summed. */
int egg_group_set_collider_surfaces(egg_group *g, int32_t n, const egg_collider_surface *s);
int egg_group_get_collider_surfaces(const egg_group *g, int32_t cap, egg_collider_surface *s, int32_t *n);
/* egg_set_collider_motion for every handle of the group alike, with its rules; a refused call changes no handle, and
 * egg_group_set_colliders resets the motions.  A step is refused while the handles differ; every handle advances its
 * stored geometry alike at the commit. */
int egg_group_set_collider_motion(egg_group *g, int32_t n, const egg_collider_motion *m);
int egg_group_get_collider_motion(const egg_group *g, int32_t cap, egg_collider_motion *m, int32_t *n);
/* egg_set_collider_spin for every handle of the group alike, with its rules; a refused call changes no handle, and
 * egg_group_set_colliders resets the spins.  A step is refused while the handles differ; every handle advances its stored
 * geometry and pivots alike at the commit. */
int egg_group_set_collider_spin(egg_group *g, int32_t n, const egg_collider_spin *s);
int egg_group_get_collider_spin(const egg_group *g, int32_t cap, egg_collider_spin *s, int32_t *n);
int egg_group_get_collider_grips(egg_group *g, int64_t grips[2]);
/* egg_set_collider_styles for every handle of the group alike, with its rules; a refused call changes no handle, and
 * egg_group_set_colliders resets the styles.  Not in the reference, which draws no colliders.  egg_group_render draws
 * handle 0's list and styles -- every handle holds and advances the same list -- at the group's interpolation alpha;
 * egg_group_get_collider_pose is egg_get_collider_pose of handle 0, a NaN alpha standing for the group's own. */
int egg_group_set_collider_styles(egg_group *g, int32_t n, const egg_collider_style *s);
int egg_group_get_collider_styles(const egg_group *g, int32_t cap, egg_collider_style *s, int32_t *n);
int egg_group_get_collider_pose(egg_group *g, double alpha, int32_t cap, egg_collider *c, int32_t *n);
/* egg_set_collider_loads for every handle of the group alike.  Every device projects only the particles it owns, so only
 * they contribute; the integer sums and the dropped counts are added over the handles, then converted once: the results
 * equal one handle's bit for bit.  A group whose handles differ in the switch refuses to step. */
int egg_group_set_collider_loads(egg_group *g, int on);
int egg_group_get_collider_load_sums(egg_group *g, int32_t cap, int64_t *sums /* [n][3] */, int64_t *dropped, double *sub_delta, int32_t *n);
int egg_group_get_collider_loads(egg_group *g, int32_t cap, egg_collider_load *out, int32_t *n);
/* egg_set_sensors for every handle of the group alike, with its rules; a refused list changes no handle.  A read adds the
 * handles' integers (readings and dropped); a batch is answered by the handle that owns it, ids being the group's.  The
 * results equal one handle's bit for bit. */
int egg_group_set_sensors(egg_group *g, int32_t n, const egg_sensor *sensors);
int egg_group_get_sensors(const egg_group *g, int32_t cap, egg_sensor *out, int32_t *n);
int egg_group_read_sensors(egg_group *g, int32_t cap, egg_sensor_reading *readings, int64_t dropped[2], int32_t *n);
int egg_group_read_sensor_batches(egg_group *g, int64_t n_ids, const int64_t *ids, int32_t *counts /* [n_ids][n_sensors][2] */);
/* egg_probe on every handle of the group with the same list; per (probe, type) the best of the handles' winners by (score,
 * key, index) is kept, and id is the group's id of the batch (the key the group gave egg_add_many_keyed).  The result equals
 * one handle that holds every batch, bit for bit, whichever device owns tied batches.  A failure on any handle writes
 * nothing. */
int egg_group_probe(egg_group *g, int32_t n, const egg_probe_query *probes, egg_probe_hit *hits /* [n][2] */);
/* egg_field on every handle of the group with the same grid; the handles' planes and totals are added on the host (two's
 * complement: the sum of the handles' sums is the sum over all their particles).  The result equals one handle that holds
 * every batch, bit for bit, units_tiled / units_direct aside.  A failure on any handle writes nothing.  There is no
 * egg_group_field_to: a group's particles live on several devices. */
int egg_group_field(egg_group *g, const egg_field_spec *spec, const egg_field_planes *host_out, egg_field_totals *totals);
/* egg_pieces without labels: every id is routed to the handle that owns the batch -- a batch lives wholly on one handle --
 * and the records are written in the caller's order; n_ids = 0 with ids = NULL means every live batch in
 * egg_group_list_ids order.  The records equal one handle's bit for bit.  A failure on any handle writes nothing. */
int egg_group_pieces(egg_group *g, const egg_pieces_spec *spec, int64_t n_ids, const int64_t *ids, egg_piece_summary *out /* [n][2] */);
/* egg_set_forces for every handle of the group alike, with its rules (relaxed order only; back to exact order only with
 * an empty list); a refused list changes no handle.  Every device accelerates only the particles it owns: the results
 * equal one handle's.  A group whose handles differ in their lists refuses to step. */
int egg_group_set_forces(egg_group *g, int32_t n, const egg_force *f);
int egg_group_get_forces(const egg_group *g, int32_t cap, egg_force *f, int32_t *n);
/* egg_set_viscosity for every handle of the group alike, with its rules (relaxed order only; back to exact order only with
 * both coefficients zero); refused values change no handle.  In a viscosity pass a ghost record carries the displacement u
 * in the two words that carry inverse mass and radius in a collision pass: a record stays 40 bytes.  The results equal one
 * handle's; the pairs are summed over the handles.  A group whose handles differ in their coefficients refuses to step. */
int egg_group_set_viscosity(egg_group *g, const double c[2]);
int egg_group_get_viscosity(const egg_group *g, double c[2]);
int egg_group_get_viscosity_pairs(egg_group *g, int64_t pairs[2]);
/* egg_set_containment for every handle of the group alike, with its rules (relaxed order only; back to exact order only
 * with the factor zero); refused values change no handle.  A batch lives wholly on one handle: nothing travels for it, and
 * the results equal one handle's; the hits are summed over the handles.  A group whose handles differ in (factor,
 * strength) refuses to step. */
int egg_group_set_containment(egg_group *g, double factor, double strength);
int egg_group_get_containment(const egg_group *g, double *factor, double *strength);
int egg_group_get_containment_hits(egg_group *g, int64_t *hits);
/* cumulative over relaxed group steps, both types: passes with a halo (the collision passes and, while a coefficient is not
 * zero, one viscosity pass per sub-step), ghost records the devices received, their bytes */
int egg_group_get_halo_counters(const egg_group *g, int64_t *passes, int64_t *records, int64_t *bytes);

/* ---- the rest of the SimulationHandler surface on a group.  One rule: whatever a group returns or draws equals, bit for
 * bit, what ONE handle holding the same batches (added in the same order) returns or draws -- in exact and in relaxed
 * order, wherever the cuts are and wherever hand-overs have put the batches.  Particle order is the group's global key:
 * the particle's index in one handle holding every live batch in ascending global id. */
/* set_white_config / set_yolk_config, get_*_config (L:226-248): the solver keys, for every handle of the group; the next
 * _step re-derives mass and radius exactly as one handle does (L:1731-1744) */
int egg_group_set_config(egg_group *g, int which, const egg_config *cfg);
int egg_group_get_config(const egg_group *g, int which, egg_config *cfg);
/* get_target_position (L:268-278) */
int egg_group_get_target(const egg_group *g, int64_t id, double *x, double *y);
/* list_ids (L:399-405): ascending global ids of the live batches; returns the count in *n, copies min(*n, cap) ids */
int egg_group_list_ids(const egg_group *g, int64_t cap, int64_t *ids, int64_t *n);
/* get_n_particles(id) / get_n_particles() with id < 0: totals over the group (L:409-419) */
int egg_group_get_n_particles(const egg_group *g, int64_t id, int64_t *n_white, int64_t *n_yolk);
/* elapsed / interpolation_alpha of egg_group_update (L:199-216) */
int egg_group_get_elapsed(const egg_group *g, double *elapsed, double *interpolation_alpha);
/* egg_download_particles over the group: one field of every particle of `which` in global-key order (doubles) */
int egg_group_download_particles(egg_group *g, int which, int field, double *dst, int64_t cap);
/* egg_get_environment over the group: the reductions run over all particles of the type in global-key order on the
 * device of handle 0, so all ten fields equal one handle's (the centroid sums are serial in particle order) */
int egg_group_get_environment(egg_group *g, int which, egg_environment *out);
/* Render attributes live in the GROUP (per global id / per type), not in its handles: a hand-over cannot lose them.
 * Semantics exactly as egg_set_render_config .. egg_set_color above, the reference's aliasing included: the render keys
 * of set_*_config give the config a NEW colour table (L:1307-1311); a batch created without a colour shares the
 * config's table (L:49-50), so egg_group_set_color on it retints the config; components clamp in egg_group_set_color
 * (L:300-319) and do not in egg_group_set_add_color (L:978-984); unknown id: EGG_WARN_UNKNOWN_ID from egg_group_set_color.
 * egg_group_add keeps its signature: call egg_group_set_add_color right after it for a colour argument of add (L:22-23). */
int egg_group_set_render_config(egg_group *g, int which, const egg_render_config *cfg);
int egg_group_get_render_config(const egg_group *g, int which, egg_render_config *cfg);
int egg_group_set_render_flags(egg_group *g, int32_t use_particle_color, int32_t use_lighting);
int egg_group_set_add_color(egg_group *g, int64_t id, int which, double r, double gr, double b, double a);
int egg_group_set_color(egg_group *g, int64_t id, int which, double r, double gr, double b, double a);
/* draw() of the group (L:158-161), as egg_render: every particle is gathered to the device of handle 0 in global-key
 * order (peer access between different ordinals: EGG_ERR_UNSUPPORTED without it), then the passes of egg_render run
 * there.  Nothing is drawn before the group's first _step or while the GROUP has no particles of one type; the canvases
 * grow only, over the group's draws (L:1957-1970); interpolation_alpha = NaN takes the group's (egg_group_update).
 * Refused while a handle of the group has a step in flight.  At most 2^31 - 1 particles of a type. */
int egg_group_render(egg_group *g, const egg_render_params *p, float *rgba);
/* the density canvas of `which` as the last egg_group_render left it (egg_render_canvas) */
int egg_group_render_canvas(egg_group *g, int which, float *rgba, int64_t cap_pixels, int32_t *w, int32_t *hgt, double *x0,
                            double *y0);
/* egg_get_instances over the group (the two meshes of L:513-523): the gather of egg_group_render, then the pack on the
 * device of handle 0, particles in global-key order; data and colour equal one handle's, bit for bit.  color_version is
 * the group's: it goes up with egg_group_add / _remove / _set_color / _set_add_color / _set_render_flags /
 * _set_render_config, not with hand-overs. */
int egg_group_get_instances(egg_group *g, int which, egg_instance *data, float *color, int64_t cap, int64_t *n,
                            uint64_t *color_version);

/* ---- relaxed order over several PROCESSES (csrc/eggsim_host_relaxed_wire.hip) -------------
 * One relaxed _step of ONE handle, driven pass by pass by a host that moves the ghost halo itself (one process per GPU:
 * egg_fluid_simulation_amd/sharding.py over torch.distributed / RCCL).  The handle knows nothing about the other
 * ranks: cell boxes go out and come in as egg_rx_box, ghost particles as messages.  When every rank drives its handle
 * through the sequence below and delivers every message, the ranks' particles end up with the bits ONE relaxed handle
 * holding all batches gives.  With S sub-steps and C collision passes, pass p = sub * C + c:
 *
 *   egg_rx_set_keys (per type, when the membership of ANY rank changed)
 *   egg_rx_begin
 *   for sub in 0 .. S-1:  egg_rx_substep(sub)
 *       for c in 0 .. C-1:  egg_rx_get_boxes(p)  ->  the ranks exchange boxes  ->  egg_rx_pack(p) + egg_rx_fetch
 *                           ->  the messages travel  ->  egg_rx_run_pass(p)
 *       with viscosity (a coefficient of egg_set_viscosity is not zero), v = EGG_RX_VISCOSITY_PASS + sub:
 *                           egg_rx_get_boxes(v)  ->  boxes  ->  egg_rx_pack(v) + egg_rx_fetch  ->  messages  ->  egg_rx_run_pass(v)
 *   egg_rx_check  ->  the ranks agree whether ANY of them flagged a bad position  ->  egg_rx_end(commit)
 *
 * The viscosity pass of sub-step `sub` comes after the sub-step's C collision passes and before the next egg_rx_substep /
 * egg_rx_check, which are refused until it has run.  It takes the types whose coefficient is not zero: the other type
 * reports an empty box, packs no record and runs nothing.  Its records have the same 5 words; words 2 and 3 carry the
 * sender's displacement (u.x, u.y) of the sub-step instead of inverse mass and radius.  EGG_RX_VISCOSITY_PASS + sub is
 * refused while both coefficients are zero.  Every rank sets the coefficients alike.
 *
 * A MESSAGE is one contiguous run of 64-bit words: word 0 the record count m, then m records of 5 words (40 bytes):
 * x, y, inverse mass, radius (doubles), global key (int64) -- 8 * (1 + 5 m) bytes.  The key is below 2^29; with
 * EGG_OPT_COHESION = 1 on the sender the upper 32 bits of the key word hold the particle's batch tag (the key base of
 * its batch), and they are zero otherwise.  Every rank sets EGG_OPT_COHESION alike.
 * All device work goes to the handle's own (non-blocking) streams.  A buffer the caller hands in is read from the
 * moment of the call: its contents must be complete (the caller has waited for its receive and synchronised the stream
 * that filled it), and a buffer in host memory must stay valid until the next egg_rx_get_boxes / egg_rx_check /
 * egg_rx_end of the handle returns.  A buffer a call fills is complete when the call returns.  Buffers may be host
 * memory or memory of the handle's device (hipMemcpyDefault), as for egg_export_batch.
 * Between egg_rx_begin and egg_rx_end the state-mutating entry points are refused.  The handle must be in relaxed order;
 * egg_step, egg_step_begin, egg_step_end and egg_get_claims_many behave as they do on any relaxed handle. */
#define EGG_RX_VISCOSITY_PASS 0x40000000
typedef struct {
    int32_t lo_x, lo_y, hi_x, hi_y; /* spatial-hash cells, inclusive */
    int32_t empty;                  /* 1: no particle of the type on this handle (the other fields are 0) */
} egg_rx_box;
/* Global keys of type `which`: keys[i] is the key (egg_add_many_keyed / egg_batch_info.key) of a batch, bases[i] the number
 * of particles of the type in all batches OF ALL RANKS with a smaller key, total the type's particle count over all
 * ranks (at most 2^29: EGG_ERR_UNSUPPORTED).  Every batch of this handle must be listed; others may be.  The device
 * copy is rebuilt at the next egg_rx_begin only when the values or the handle's batches changed. */
int egg_rx_set_keys(egg_handle *h, int which, int64_t n, const int64_t *keys, const int64_t *bases, int64_t total);
/* reserves room for the local particles + (total - local) ghosts per type, clears the status words; launches nothing
 * that writes the uncommitted state */
int egg_rx_begin(egg_handle *h, double delta, int32_t n_substeps, int32_t n_collision_steps);
/* pre-solve + follow of sub-step `sub` (after the post-solve of the one before); records the cell box of what it wrote */
int egg_rx_substep(egg_handle *h, int32_t sub);
/* the cell boxes of this handle's positions at the start of pass `pass`, per type (waits for the streams) */
int egg_rx_get_boxes(egg_handle *h, int32_t pass, egg_rx_box boxes[2]);
/* packs, for each of n_dest destinations, the local particles within one cell of its box: boxes[2 * k + type];
 * counts[2 * k + type] = records in the message for destination k (waits for the streams) */
int egg_rx_pack(egg_handle *h, int32_t pass, int32_t n_dest, const egg_rx_box *boxes, int64_t *counts);
/* copies the messages of the last egg_rx_pack out: out[2 * k + type] receives 8 * (1 + 5 * count) bytes, NULL skips it */
int egg_rx_fetch(egg_handle *h, int32_t n_dest, void *const *out);
/* the collision pass over the local particles + the ghosts of n_src received messages: msgs[2 * k + type] with
 * counts[2 * k + type] records (NULL or 0: none).  Writes local positions only and records the next pass's box. */
int egg_rx_run_pass(egg_handle *h, int32_t pass, int32_t n_src, const void *const *msgs, const int64_t *counts);
/* after the last pass, before anything is committed: *bad = 1 when a position of this handle is NaN or its cell lies
 * outside +-2^30; pairs[type] = pairs this handle counted; *ghost_records = ghost records it received in the step */
int egg_rx_check(egg_handle *h, int32_t *bad, int64_t pairs[2], int64_t *ghost_records);
/* commit = 1 (after egg_rx_check, refused when it reported bad): post-solve of the last sub-step, the step counts as one
 * relaxed _step.  commit = 0, at any point after egg_rx_begin: the state is as before egg_rx_begin. */
int egg_rx_end(egg_handle *h, int32_t commit);

/* ---- draw() of a scene sharded over several PROCESSES (csrc/eggsim_host_draw_source.hip) ----
 * One process per GPU (egg_fluid_simulation_amd/sharding.py): draw() depends on particle order twice -- the screen blend
 * and the serial centroid sums (L:1669-1718, L:2057-2058) --, so every rank sends the draw record of its particles to ONE
 * render rank, which puts them into the order of one handle holding every batch (the global key of egg_rx_set_keys) and
 * runs the passes of egg_render over them, unchanged.  The handle knows nothing about the other ranks:
 *
 *   every rank:    egg_draw_pack(type)  ->  the message travels (or stays, on the render rank)
 *   render rank:   egg_draw_source_layout(type)  ->  egg_draw_source_place(type) once per message and once for its own
 *                  particles  ->  egg_draw_source_render / _environment / _download / _render_canvas
 *
 * A MESSAGE holds the seven draw fields x, y, last_x, last_y, vx, vy, radius (L:513-517, L:744-813) of n particles, field
 * after field: double[7][n], 56 n bytes, particles in the sending handle's own order (ascending batch key).  Buffers may
 * be host memory or memory of the handle's device, as for egg_rx_fetch; a buffer a call fills is complete when the call
 * returns, a buffer a call reads must be complete (the caller has waited for its receive and synchronised the stream
 * that filled it) and may go when the call returns.  The shadow arrays (56 B per particle of the whole scene on the
 * render device), the canvases with their grow-only sizes (L:1957-1970) and the scratch of the passes belong to this
 * external source, not to the handle's own egg_render. */
/* the message of this handle's particles of `which` into `out` (room for cap_particles >= its particle count): one
 * kernel launch on the type's stream.  Refused while a step is in flight (egg_step_begin or egg_rx_begin open). */
int egg_draw_pack(egg_handle *h, int which, void *out, int64_t cap_particles);
/* (a) the layout of type `which` over all ranks: `total` particles (at most 2^31 - 1: EGG_ERR_UNSUPPORTED, as when the
 * render device has no room for them), atom_offset[k] the global key of the first particle of the k-th live batch in
 * ascending key, atom_color[4 k ..] the rgba its particles carry (L:978-990, L:1110-1129).  Forgets what was placed. */
int egg_draw_source_layout(egg_handle *h, int which, int64_t total, int64_t n_atoms, const int64_t *atom_offset, const float *atom_color);
/* (b) one message of n particles into its places: run r covers the particles run_src[r] .. run_src[r + 1] - 1 of the
 * message (run_src[0] = 0, ascending; the last run ends at n) and goes to run_dst[r] ..; a run is a stretch whose
 * destinations are consecutive (whole batches).  msg = NULL places this handle's own particles from its arrays without a
 * copy (n = its particle count; refused while a step is in flight).  Every run is checked against the message and the
 * layout before anything is launched; every particle of the layout must be placed exactly once before (c). */
int egg_draw_source_place(egg_handle *h, int which, const void *msg, int64_t n, int64_t n_runs, const int64_t *run_src, const int64_t *run_dst);
/* (c) draw() (L:158-161) as egg_render over the placed particles.  cfg[2], the two switches (L:448-449), `stepped` (a
 * _step has run: nothing is drawn before, L:1997-1999) and interpolation_alpha (taken where p->interpolation_alpha is
 * NaN) are the caller's: the sharded scene owns them, not this handle.  Nothing is drawn while a type has no particles. */
int egg_draw_source_render(egg_handle *h, const egg_render_params *p, const egg_render_config *cfg, int32_t use_particle_color,
                           int32_t use_lighting, int32_t stepped, double interpolation_alpha, float *rgba);
/* the density canvas of `which` as the last egg_draw_source_render left it (egg_render_canvas) */
int egg_draw_source_render_canvas(egg_handle *h, int which, float *rgba, int64_t cap_pixels, int32_t *w, int32_t *hgt, double *x0,
                                  double *y0);
/* egg_get_environment over the placed particles of `which` (L:1669-1718, L:1795-1815) */
int egg_draw_source_environment(egg_handle *h, int which, int32_t stepped, egg_environment *out);
/* egg_download_particles over the placed particles: `field` is one of the seven draw fields (EGG_FIELD_*) */
int egg_draw_source_download(egg_handle *h, int which, int field, double *dst, int64_t cap);
/* egg_get_instances over the placed particles (the two meshes of L:513-523), colours from the layout's atom_color; the
 * colour version is the caller's: the sharded scene owns the colours.  It reads the shadow arrays, not the handle's own:
 * like egg_draw_source_download it is not refused while a step of the handle is in flight. */
int egg_draw_source_instances(egg_handle *h, int which, egg_instance *data, float *color, int64_t cap, int64_t *n);

/* ---- impulses: push, blast, stir and brake the particles inside regions: include/eggsim_impulse.h ----
 * Two more entry points and their records, in a header of their own that this one brings along: a caller includes eggsim.h
 * and has the whole ABI. */
#include "eggsim_impulse.h"

/* ---- measures: per-batch mass, momentum, energy, extent and shape: include/eggsim_measure.h ----
 * Three more entry points, their spec and their record, in a header of their own as well. */
#include "eggsim_measure.h"

/* ---- cover: the particles' discs rastered into a grid -- area, depth, owner map: include/eggsim_cover.h ----
 * Three more entry points, their spec, planes and totals, in a header of their own as well. */
#include "eggsim_cover.h"

/* ---- touches: which eggs touch which, how much and where: include/eggsim_touch.h ----
 * Three more entry points, their spec, their query and their record, in a header of their own as well. */
#include "eggsim_touch.h"

#ifdef __cplusplus
}
#endif
#endif
