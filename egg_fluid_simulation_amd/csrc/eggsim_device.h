// eggsim_device.h -- structs shared by the host side (eggsim_host_*.hip) and the
// gfx950 kernels (eggsim_step.hip).  Not part of the public ABI.
#pragma once
#include <stdint.h>

#define EGG_MAX_PASSES 64     // per-pass counters kept for the first 64 collision passes of a step
#define EGG_WAVE 64

// Written by the step kernel, read back by the host after every step.
struct EggStatus {
    int32_t fail_claim;     // a particle left its atom's claimed cell box: tiles were not provably independent
    int32_t fail_overflow;  // a tile needed more visit-list entries than the launch provided
    int32_t fail_stall;     // the DAG executor did not drain (internal error guard)
    int32_t fail_range;     // a cell coordinate does not fit the packed tile-relative form
    int32_t min_slack;      // min over particles of the distance (cells) to their claim box edge at step end
    int32_t was_cut;        // single-tile mode: the collision budget cut some pass (L:1657-1658)
    int32_t fail_levels;    // packed pipeline: a group's pair-dependency DAG is deeper than the level table of the launch
    int32_t max_level;      // deepest level any group reached (what the level table must hold)
    int32_t fail_levlds;    // packed pipeline, out-of-order walk: a tile's pair stream is longer than the LDS level array of the launch
    int32_t reserved0;
    unsigned long long visits[EGG_MAX_PASSES]; // visited pairs per collision pass, summed over tiles
    unsigned long long max_list;               // largest visit-list length any tile had in one pass
    unsigned long long rounds;                 // DAG rounds, summed over tiles and passes
};

// One particle type (white or yolk) of one handler.  All pointers are device pointers.
struct EggStepArgs {
    // particle state, SoA, particle-index order (= the reference's array order, L:964-993)
    const double *x_in, *y_in, *vx_in, *vy_in;
    double *x_out, *y_out, *vx_out, *vy_out;
    const double *inv_mass, *radius;
    // atoms: the particles of one batch of this type, contiguous
    const int32_t *atom_offset;  // first particle
    const int32_t *atom_count;
    const int32_t *atom_batch;   // batch slot (equality = "same batch", L:1609)
    const double *atom_tx, *atom_ty;  // follow target (L:1763-1766)
    const double *atom_fd;            // 2 * sqrt(batch radius) (L:1454, L:1790)
    const int32_t *atom_claim;   // int4 {lo_x, lo_y, hi_x, hi_y}: cells the atom's particles may occupy this step
    int32_t *atom_aabb_out;      // int4: cells occupied at the end of the step
    int32_t *atom_fail;          // cleared when the atom's tile starts, set to 1 when a particle of the atom left its claim
    int32_t *atom_disp_out;      // int4: max particle travel in the LAST sub-step towards +x, -x, +y, -y (1/16 px)
    // tiles: independent groups of atoms, one workgroup each
    const int32_t *tile_atom_begin;  // [n_tiles + 1] into tile_atoms
    const int32_t *tile_atoms;       // atom ids, ascending inside a tile
    int32_t n_tiles;
    // scalars of the environment (L:1726-1774)
    double sub_delta, damping, follow_compliance, collision_compliance;
    double overlap_factor, cell_size, eps;
    double budget;             // max_n_collisions = fraction * N^2 (L:1752-1753)
    int32_t single_tile;       // 1: this launch is one tile holding every particle -> exact budget handling
    int32_t n_substeps, n_collision_steps;
    // LDS geometry of this launch
    int32_t nmax;      // particles per tile (capacity)
    int32_t amax;      // atoms per tile (capacity)
    int32_t ccap;      // cells: dense grid capacity (use_grid) or hash slots (power of two)
    int32_t use_grid;  // 1: cells are a dense grid over the tile's claim box, 0: open-addressing hash
    int32_t lcap;      // visit-list entries per pass (capacity)
    int32_t spin_sleep;  // 1: idle waves of the pair dataflow sleep between polls (many tiles per CU)
    int32_t threads;     // workgroup size this type's tiles want (a shared launch may bring more: the surplus waves exit)
    int32_t gens;        // hash generations kept alive (2; n_substeps when there is one collision pass per sub-step)
    int32_t pair_cache;  // 1: LDS holds lcap more 16-byte records (per-pair projection terms, see Tile::pinv)
    EggStatus *status;
    EggStatus *status_next;  // the other status block: re-initialised by this launch for the next one
    unsigned char *scratch;  // egg_step_kernel_gl / _gs: n_tiles slices of scratch_stride bytes
    unsigned long long scratch_stride;
};

#if defined(__HIPCC__)
__host__ __device__
#endif
static inline size_t egg_align16(size_t v) { return (v + 15) & ~(size_t)15; }

// bytes of one tile's slice of EggStepArgs::scratch (visit lists in global memory: own_pack 4 B, inc_tmp 8 B per entry)
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline size_t egg_step_scratch_bytes(int lcap, int single_tile, int gens = 2) {
    size_t l = (size_t)lcap, g = (size_t)(gens < 2 ? 2 : gens);
    return ((l * 4 + 15) & ~(size_t)15) + ((l * 8 + 15) & ~(size_t)15) + ((((single_tile ? g : 0) * l * 2) + 15) & ~(size_t)15);
}

// dynamic LDS bytes the step kernel carves for the geometry above (must match eggsim_step.hip)
static inline size_t egg_step_lds_bytes(int nmax, int amax, int ccap, int use_grid, int lcap, int single_tile,
                                        int global_lists, int threads, int pair_cache = 0, int gens = 2) {
    size_t n = (size_t)nmax, a = (size_t)amax, c = (size_t)ccap, l = (size_t)lcap, g = (size_t)(gens < 2 ? 2 : gens);
    size_t b = 0;
    b += 2 * egg_align16(n * 16);            // pos wr
    b += 2 * egg_align16((nmax > threads || threads >= 3 * nmax) ? n * 16 : 0);  // prev vel (registers otherwise; wide tiles: LDS)
    b += 3 * egg_align16(a * 8);             // atx aty afd
    b += egg_align16(g * n * 4);             // ckey[gens]
    b += egg_align16(g * c * 4);             // cell[gens]
    b += egg_align16(use_grid ? 0 : g * c * 4);  // hkeys[gens]
    b += egg_align16((single_tile ? g : 1) * (n + 1) * 4);  // own_off
    b += egg_align16((n + 1) * 4);           // inc_off
    b += 2 * egg_align16(n * 4);             // fill done
    if (!global_lists) b += 2 * egg_align16(l * 4);  // own_pack inc_tmp
    if (!global_lists && pair_cache) b += egg_align16(l * 16);  // pinv
    b += egg_align16(a * 4 * 4);             // aclaim
    b += egg_align16((a + 1) * 4);           // aoff
    b += 2 * egg_align16(a * 4);             // abatch aglob
    b += 2 * egg_align16(a * 4 * 4);         // aaabb adisp
    b += egg_align16(16 * 4);                // scalars
    b += egg_align16(g * n * 2);             // hitems[gens]
    b += 3 * egg_align16(n * 2);             // pslot aslot nlo
    if (!global_lists) b += egg_align16(single_tile ? g * l * 2 : 0);  // own_ent (exact-budget mode)
    return b;
}

// threads of the workgroup that runs a tile of at most nmax particles (one thread per particle)
static inline int egg_step_threads(int nmax, int spread) {
    int t = (nmax * spread + EGG_WAVE - 1) / EGG_WAVE * EGG_WAVE;
    return t < EGG_WAVE ? EGG_WAVE : (t > 1024 ? 1024 : t);
}

// ---------------------------------------------------------------------------------------------
// Packed pipeline (eggsim_packed.hip), the throughput path for many tiles per CU: one launch per phase
// instead of one fused launch per step.  The particles of the participating tiles are kept in PACKED order
// (tile after tile, atoms in tile order) in scratch arrays for the duration of a step; a collision pass is
//   egg_pk_lists   (one workgroup per tile)  cell grid + visit lists in the reference's order -> global memory
//   egg_pk_levels  (one workgroup per group) longest-path level of every pair (in-order or out-of-order walk)
//   egg_pk_sort    (one workgroup per group) the group's pairs sorted by level
//   egg_pk_exec    (one wave per group)      the group's positions in LDS; level by level, 64 pairs at a time
// A GROUP is a run of consecutive tiles whose particles one wave keeps in LDS.  Pairs of one level share no
// particle and all their predecessors lie in lower levels, so running the levels in order, each level's
// pairs in any order, is the reference's sequential result bit for bit.
struct EggPackedArgs {
    // particle-order state of the type, atoms, claims: as in EggStepArgs
    const double *x_in, *y_in, *vx_in, *vy_in;
    double *x_out, *y_out, *vx_out, *vy_out;
    const double *inv_mass, *radius;
    const int32_t *atom_offset, *atom_count, *atom_batch;
    const double *atom_tx, *atom_ty, *atom_fd;
    const int32_t *atom_claim;
    int32_t *atom_aabb_out, *atom_fail, *atom_disp_out;
    const int32_t *tile_atoms;  // atom ids of all tiles of the type (tile_geo gives a tile's range)
    int32_t n_tiles, n_groups;
    // Geometry of this class, computed by the host when tiles are formed, so that a kernel learns everything
    // about its tile or group from ONE load (every dependent global load costs a full memory round trip):
    const int32_t *tile_geo;    // [n_tiles][8]: first packed particle, particles, first entry in tile_atoms / tile_claims,
                                //               atoms, cell origin x, y (claims' minimum - 2), grid width, height
    const int32_t *tile_claims; // [4] per entry of tile_atoms: the atom's claim box {lo_x, lo_y, hi_x, hi_y}
    const int32_t *grp_geo;     // [n_groups][4]: first tile, end tile, first packed particle, particles
    int32_t p_begin, p_end;     // packed range of the class
    // packed per-particle arrays of the type (indexed by packed index)
    double *pk_pos, *pk_prev, *pk_wr;  // double2 each: position, position at the start of the sub-step, (inverse mass, radius)
    int32_t *pk_src;           // particle index in the particle-order arrays
    int32_t *pk_atom;          // atom id
    uint16_t *pk_aslot;        // atom slot inside the tile
    uint32_t *pk_ckey;         // [2][pk_stride] packed cell of the last pass of each sub-step parity
    int32_t pk_stride;
    // per tile (class-relative), `scap` words each: the tile's pair STREAM in the reference's order -- the visit
    // entries self | slow << 15 | other << 16 (tile-local indices) of every particle as `self`, ascending
    uint32_t *lists;
    uint16_t *lvl;             // level of each stream entry
    uint32_t *rank;            // per stream entry (out-of-order level walk): earlier entries involving the self | the partner << 16
    // per group, `sort_cap` words each: the group's pairs sorted by level (bit 31 set, indices group-local), and its
    // work list of `chunk_cap` words: chunk c = first word | (pairs - 1) << 26, at most 64 pairs of ONE level, levels ascending
    uint32_t *sorted;
    uint32_t *chunks;
    int32_t *grp_nchunks;      // [n_groups]
    uint32_t *lev_start;       // [n_groups][lev_cap + 2] first slot of every level in the group's sorted list
    int32_t *grp_nlev;         // [n_groups]
    int32_t *tile_total;       // [n_tiles] visit entries of the current pass (0: the tile failed a check)
    int32_t *tile_visits;      // [EGG_PK_MAX_PASSES][n_tiles] n_collided of each pass (L:1657)
    int32_t *tile_need;        // [EGG_PK_MAX_PASSES][n_tiles] visit entries each pass needed (list capacity check)
    int32_t *tile_slack;       // [n_tiles]
    int32_t *tile_fast;        // [n_tiles] 1: every pair of the tile may take the hand-expanded arithmetic (found by the step's first list pass)
    int32_t lcap, scap, lev_cap, sort_cap, chunk_cap;
    // LDS geometry of egg_pk_lists
    int32_t nmax, amax, ccap, use_grid, stage_cap;
    // environment
    double sub_delta, damping, follow_compliance, collision_compliance, overlap_factor, cell_size, eps;
    int32_t n_substeps, n_collision_steps;
    int32_t pass_seq, substep, stale;  // of the launch
    int32_t tune;              // developer switches (EGGSIM_TUNE), 0 in normal operation; unused by the kernels at present
    uint32_t *simd_claims;     // [4096] per compute unit: SIMDs taken by executor waves of egg_pk_levexec_kernel right now
    int32_t lev_lds_cap;       // out-of-order walk: entries of a tile's stream whose levels fit the LDS array of the launch
    EggStatus *status, *status_next;
};
#define EGG_PK_MAX_PASSES 64
#define EGG_PK_WINDOW 128  // stream words a sub-wave of egg_pk_levels holds in LDS at a time

// dynamic LDS of egg_pk_lists for the geometry above (must match eggsim_packed.hip)
// (gens: cell generations the launch holds -- 1 for a fresh pass, 2 for the stale pass)
static inline size_t egg_pk_lists_lds_bytes(int nmax, int amax, int ccap, int use_grid, int stage_cap, int gens) {
    size_t n = (size_t)nmax, a = (size_t)amax, c = (size_t)ccap, b = 0, G = (size_t)gens;
    b += egg_align16(G * n * 4);                  // ckey[gens]
    b += egg_align16(G * c * 4);                  // cell[gens]
    b += egg_align16(use_grid ? 0 : G * c * 4);   // hkeys[gens]
    b += egg_align16((n + 1) * 4);                // own_off
    b += egg_align16(n * 4);                      // fill
    b += egg_align16(a * 4 * 4);                  // aclaim
    b += egg_align16((a + 1) * 4);                // aoff
    b += egg_align16(16 * 4);                     // scalars
    b += egg_align16(G * n * 2);                  // hitems[gens]
    b += egg_align16(n * 2);                      // aslot
    {   // the partners kept by the counting pass; the grid builder's scratch (tmp, pslot) lives there before
        const size_t stage = egg_align16(((size_t)stage_cap + 1) * (n + 1) * 2), tmp = egg_align16(n * 4) + egg_align16(n * 2);  // ((n + 1) / 2 pairs of 2 stage_cap + 2 words)
        b += stage > tmp ? stage : tmp;
    }
    return b;
}
// egg_pk_levexec_kernel: the ring of ready-made pair records between its helper wave and its executor wave:
// EGG_PK_RING chunks x 64 lanes x (8 B addresses + 3 x 16 B constants)
#define EGG_PK_SPIN_LIMIT (1u << 24)  // polls a wave of the packed pipeline waits for another wave before it gives up (fail_stall = 4): seconds
#define EGG_PK_RING 8
#define EGG_PK_RING_BYTES (EGG_PK_RING * 64 * 56)
// dynamic LDS of egg_pk_levels_mr16 (the in-order walk): level histogram, last level and a stamp word per particle of the
// group, one stream window per sub-wave of 16 lanes
static inline size_t egg_pk_levels_mr_lds_bytes(int lev_cap, int group_particles, int threads) {
    return egg_align16((size_t)(lev_cap + 2) * 4) + egg_align16((size_t)group_particles * 2) +
           egg_align16((size_t)group_particles * 4) + egg_align16((size_t)(threads / 16) * EGG_PK_WINDOW * 4);
}
// dynamic LDS of egg_pk_levels_ooo (the out-of-order walk): level histogram, (completed pairs | last level) and the
// ranking pass's entry counter per particle of the group
// (+ a spare counter per lane), the levels of every stream entry of the group's tiles
static inline size_t egg_pk_levels_ooo_lds_bytes(int lev_cap, int group_particles, int tiles, int lev_lds_cap) {
    return egg_align16((size_t)(lev_cap + 2) * 4) + egg_align16((size_t)group_particles * 4) + 2 * egg_align16((size_t)(group_particles + 64) * 4) +
           egg_align16((size_t)tiles * (size_t)lev_lds_cap * 2);
}

// ---- headless renderer (eggsim_render.hip) ----
#define EGG_RENDER_TILE 16    // canvas tile edge in px: one workgroup of 256 threads per tile
#define EGG_RENDER_STAGE 128  // particles a tile stages in LDS at a time
struct EggRenderArgs {  // pass 1 of one type: particles -> canvas (_update_canvases, L:1995-2113)
    const double *x, *y, *last_x, *last_y, *vx, *vy, *radius;
    const int32_t *atom_offset;  // first particle of every atom (= batch), ascending
    const float4 *atom_color;    // the batch's particle colour (L:1110-1129)
    int32_t n, n_atoms;
    float t, tx, ty;             // interpolation alpha; translation world -> canvas px
    float texture_scale, motion_blur;
    int32_t premultiply;         // the non-instanced draw loop's setColor(r a, g a, b a, a) (L:2035-2041)
    int32_t cw, ch, tiles_x, tiles_y;
    uint32_t *tile_count, *tile_start, *tile_cursor;  // [tiles], [tiles + 1], [tiles]
    uint32_t *entries;           // the tiles' particle lists
    uint32_t *totals;            // [0] all list entries, [1] the longest list
    const float *texture;        // tsize x tsize density texture
    int32_t tsize;
    float4 *canvas;              // ch x cw
};
// dynamic LDS of egg_render_splat_kernel: bordered texture, staged instances + colours, the tile's list (padded to 2^k)
static inline size_t egg_render_splat_lds_bytes(int tsize, size_t padded_list) {
    return egg_align16((size_t)(tsize + 2) * (tsize + 2) * 4) + (size_t)EGG_RENDER_STAGE * (32 + 16) + padded_list * 4;
}
struct EggCompositeLayer {  // pass 2 of one type (_draw_canvases, L:2117-2175)
    const float4 *canvas;
    int32_t w, h;
    float x0, y0;  // the canvas's top-left corner on the screen
    float4 color, outline_color;
    float outline_thickness, highlight_strength, shadow_strength;
};
struct EggCompositeArgs {
    float4 *screen;
    int32_t screen_w, screen_h, n_layers;
    float threshold, smoothness;
    int32_t use_particle_color, use_lighting;
    EggCompositeLayer layer[2];
};
// colliders in the picture (egg_set_collider_styles; DESIGN.md section 2.7, "Collider styles"): the visible colliders of ONE
// layer at the pose of the frame, in list order -- the host leaves the others out, so a lane's index is a bit of the mask
#define EGG_DRAW_MAX_COLLIDERS 64  // one wave's width: lane k culls collider k
struct EggDrawCollider {  // 72 bytes
    double p[4];       // the pose's parameters
    int32_t kind;      // EGG_RX_COLLIDER_*
    float line_width;  // px; 0: no line
    float fill[4];     // fill[3] == 0: no fill (also where the kind has no inside)
    float line[4];     // line[3] == 0: no line
};
struct EggColliderDrawArgs {
    float4 *screen;
    const EggDrawCollider *list;
    int32_t count;     // 1 .. EGG_DRAW_MAX_COLLIDERS
    int32_t screen_w, screen_h;
    double origin_x, origin_y;
};

// the arguments of up to four launch classes sharing one launch (egg_step_kernel_multi*); unused slots have n_tiles = 0
struct EggStepArgs4 {
    EggStepArgs a[4];
};

// The relaxed-order path (eggsim_relaxed.hip): one particle type, one thread per particle.  A
// collision pass is a Jacobi pass over a spatial hash built fresh from the pass's start positions: open-addressed cell
// table (64-bit cell keys, linear probing), particles grouped by cell, ascending index inside a cell.
#define EGG_RX_EMPTY_KEY 0xFFFFFFFFFFFFFFFFull
struct EggRelaxedArgs {
    int32_t n;
    uint32_t table_mask;  // hash slots - 1 (a power of two, at least twice the particle count)
    int32_t pass;         // collision pass of the step (its pair counter is status[1 + pass])
    const double *x_in, *y_in, *vx_in, *vy_in;  // [cur]
    double *x_out, *y_out, *vx_out, *vy_out;    // [cur ^ 1]
    const double *inv_mass, *radius;
    const int32_t *p_atom;                        // atom of each particle
    const double *atom_tx, *atom_ty, *atom_fd;    // follow target and target distance of each atom
    double2 *pos, *pos_next, *prev;               // positions of this pass / after it, start of the sub-step
    double2 *spos, *swr;                          // (x, y) and (inverse mass, radius) grouped by cell
    int32_t *pslot, *tmp, *sidx;                  // hash slot of each particle, scatter scratch, particle of a grouped slot
    unsigned long long *hkey;                     // [table] cell key of a slot, EGG_RX_EMPTY_KEY when free
    uint32_t *hcount, *hstart;                    // [table + 1] particles per slot; their first grouped slot (exclusive scan)
    unsigned long long *status;                   // [0] a cell out of range or a NaN position, [1 + pass] pairs counted
    double damping, sub_delta, eps, follow_compliance;
    double collision_compliance, overlap, cell_size, omega;
};

// Device groups ("Several devices"): the group instantiations of the relaxed kernels
// (egg_rx_*_group_kernel) take these besides.  Entries are the n local particles, then the ghosts.
struct EggRxGroupFields {
    const int32_t *ekey;                 // [n + ghost capacity] global key of every entry
    int32_t *sloc;                       // [n + ghost capacity] entry of a grouped slot
    const unsigned long long *n_ghost;   // ghost entries of this pass (written by egg_rx_unpack_kernel)
    const double2 *gwr;                  // [ghost capacity] (inverse mass, radius) of the ghosts
    unsigned long long *box;             // 4 words: cell box of the positions the kernel writes (EGG_RX_BOX_*), or nullptr
};
struct EggRelaxedGroupArgs {
    EggRelaxedArgs a;
    EggRxGroupFields g;
};

// Effective cohesion (EGG_OPT_COHESION = 1, DESIGN.md section 2.7, "Cohesion"): the cohesive instantiations of the rank
// and gather kernels (egg_rx_*_coh_kernel) take these besides.  A batch TAG is equal for two particles exactly when they
// belong to one batch: the atom index on a single handle, the atom's key base (atom_tag) in a group or over the wire.
struct EggRxCohesionFields {
    double compliance;                   // _strength_to_compliance(cohesion_strength, sub_delta) (L:1772)
    double factor;                       // cohesion_interaction_distance_factor
    const int32_t *atom_tag;             // [atoms] tag of a local atom; nullptr: the atom index itself
    const int32_t *gtag;                 // [ghost capacity] tags of the ghosts (group instantiations)
    int32_t *stag;                       // [n + ghost capacity] tag of a grouped slot, next to spos / swr
    unsigned long long *solves;          // one word: pairs whose cohesion branch fired in this step
};

// Static colliders (egg_set_colliders, DESIGN.md section 2.7, "Colliders"): the collider instantiations of the gather
// kernel (egg_rx_gather*_col_kernel) take these besides.  The list is the handle's, in a small device buffer written when
// it is set; a record has the layout of the ABI's egg_collider (40 bytes), the half-plane's normal already normalised.
#define EGG_RX_MAX_COLLIDERS 64
#define EGG_RX_COLLIDER_HALF_PLANE 0  // = EGG_COLLIDER_* of include/eggsim.h
#define EGG_RX_COLLIDER_DISC 1
#define EGG_RX_COLLIDER_CONTAINER 2
#define EGG_RX_COLLIDER_SEGMENT 3
#define EGG_RX_COLLIDER_WALL 5  // (4 is not a kind) a segment that sweeps the sub-step's path (the *_col_wall instantiations only)
struct EggCollider {
    int32_t kind, type_mask;
    double p[4];
};
struct EggRxColliderFields {
    const EggCollider *list;             // [count], applied in this order; every lane reads the same record
    int32_t count;
    int32_t type_bit;                    // 1 white, 2 yolk: a collider applies when its type_mask has the bit
    unsigned long long *hits;            // one word: (collider, particle, pass) triples that moved a particle in this step
};

// Collider surfaces (egg_set_collider_surfaces, DESIGN.md section 2.7, "Collider surfaces"): the surface instantiations of
// the gather kernel (egg_rx_gather*_col_srf_kernel) take these besides the collider fields.  The records are parallel to
// the collider list, in a small device buffer written when they are set; a record has the layout of the ABI's
// egg_collider_surface (24 bytes).  The wall instantiations (egg_rx_gather*_col_wall_kernel, "Walls") take the same
// arguments: while the list holds a wall the records exist for every collider, defaults included.
struct EggSurface {
    double friction, vx, vy;
};
struct EggRxSurfaceFields {
    const EggSurface *list;              // [the collider count]; every lane reads the same record
    double sub_delta;                    // h of step 5c
    unsigned long long *grips;           // one word: friction applications (stick or slide) in this step
};

// Collider motion (egg_set_collider_motion, DESIGN.md section 2.7, "Collider motion"): the motion instantiations of the
// gather kernel (egg_rx_gather*_col_mov_kernel) take these besides the collider and surface fields.  The records are
// parallel to the collider list, in a small device buffer written when they are set, never per step; a record has the
// layout of the ABI's egg_collider_motion (16 bytes).  While a motion is not zero the surface records exist for every
// collider, defaults included, as they do with a wall in the list.
struct EggMotion {
    double vx, vy;
};
struct EggRxMotionFields {
    const EggMotion *list;               // [the collider count]; every lane reads the same record
    double t;                            // the end of the pass's sub-step, from the start of the step: (sub + 1) * sub_delta
};

// Collider spin (egg_set_collider_spin, DESIGN.md section 2.7, "Collider spin"): the spin instantiations of the gather
// kernel (egg_rx_gather*_col_spin_kernel) take these besides everything a motion instantiation takes.  The records are
// parallel to the collider list, in a small device buffer written when they are set; a record has the layout of the
// ABI's egg_collider_spin (24 bytes).  The sines and cosines are the host's (libm): a table the host writes once per step,
// one row of (cos, sin)(t omega) per sub-step and one of (cos, sin)(h omega), each with a pair per collider.  While a spin
// is not zero the motion and surface records exist for every collider, zeros and defaults included.
struct EggSpin {
    double px, py, omega;
};
struct EggRxSpinFields {
    const EggSpin *list;                 // [the collider count]; every lane reads the same record
    const double2 *cs;                   // [the collider count]: (cos, sin)(t omega), t the end of the pass's sub-step
    const double2 *hcs;                  // [the collider count]: (cos, sin)(h omega), one sub-step's turn
    double ts;                           // the start of the pass's sub-step, from the start of the step: sub * sub_delta
};

// Collider loads (egg_set_collider_loads, DESIGN.md section 2.7, "Collider loads"): the loads instantiations of the gather
// kernel (egg_rx_gather*_col_load_kernel) take these besides everything a spin instantiation takes.  One instantiation per
// (group, cohesion) serves every collider flavour: it is the most general one, and the three words below say which of its
// rules the flavour it stands in for would have run, so that it computes that flavour's bits (no "+ 0.0" of a motion that
// flavour never added).  The surface records exist for every collider (defaults when none are set); the motion records
// are read only while `moving` or `turning`, the spin records only while `turning` or `pivots`.
#define EGG_RX_LOAD_SCALE_IMPULSE 0x1p20  // = EGG_COLLIDER_LOAD_IMPULSE_SCALE of include/eggsim.h
#define EGG_RX_LOAD_SCALE_TORQUE 0x1p10   // = EGG_COLLIDER_LOAD_TORQUE_SCALE
#define EGG_RX_LOAD_LIMIT 0x1p53          // a scaled contribution that reaches it (or is not finite) is dropped whole
struct EggRxLoadFields {
    unsigned long long *sums;            // [the collider count][3]: int64 sums of (qx, qy, qz), two's complement; both types add
    unsigned long long *dropped;         // one word: contributions dropped in this step
    double eps;                          // a particle with !(inverse mass > eps) contributes nothing (the force step's test)
    int32_t moving;                      // a collider motion of the handle is not zero: the motion rule runs
    int32_t turning;                     // a collider spin of the handle is not zero: the spin rule runs for such a collider
    int32_t pivots;                      // the handle holds spin records: the torque is about them (else about the origin)
};

// Collider bodies (egg_set_collider_bodies, DESIGN.md section 2.7, "Collider bodies"): egg_rx_bodies_kernel runs once per
// sub-step of a step in which bodies act, one wave, lane k = collider k.  It rewrites the records the loads instantiations
// of the gather read -- the list, the motions, the spins and the row of turns -- from the loads the sub-step has added to the
// sums.  A record has the layout of the ABI's egg_collider_body (48 bytes).
struct EggBody {
    double inv_mass, inv_inertia, ax, ay, drag, spin_drag;
};
struct EggRxBodiesArgs {
    EggCollider *list;                   // [count]: becomes the geometry of the sub-step's end
    EggMotion *motions;                  // [count]
    EggSpin *spins;                      // [count]
    double2 *cs;                         // [count]: the turn (c, s) of one sub-step, read by the gathers as both of their rows
    const EggBody *bodies;               // [count]
    const unsigned long long *sums;      // [count][3]: the step's load sums so far (EggRxLoadFields::sums)
    unsigned long long *seen;            // [count][3]: the sums as the sub-step before left them
    double h;                            // the sub-step
    int32_t count;
};

// Collider contacts (egg_set_collider_contacts, DESIGN.md section 2.7, "Collider contacts"): egg_rx_contacts_kernel
// (eggsim_relaxed_contacts.hip) runs once per sub-step of a step in which contacts act, one wave, directly behind
// egg_rx_bodies_kernel on its stream, lane k = collider k.  It reads what the integrator has written and changes the
// velocities, the spins and the turns of bodies only.  A record has the layout of the ABI's egg_collider_contact (16 bytes).
#define EGG_RX_MAX_CONTACT_LANES 64  // = EGG_MAX_COLLIDERS: one wave holds the list
struct EggContact {
    double restitution;
    int32_t on, reserved;
};
struct EggRxContactsArgs {
    const EggCollider *list;             // [count]: the geometry of the sub-step's end
    EggMotion *motions;                  // [count]
    EggSpin *spins;                      // [count]: omega changes, the pivots stay
    double2 *cs;                         // [count]: the turn of a free-turning body follows its new spin
    const EggBody *bodies;               // [count]
    const EggContact *contacts;          // [count]
    unsigned long long *solves;          // [1]: the step's fires so far (zero at the step's start)
    double h;                            // the sub-step
    int32_t count;
    int32_t iterations;                  // 1 .. 16
};

// Force fields (egg_set_forces, DESIGN.md section 2.7, "Forces"): the force instantiations of the kernels that begin a
// sub-step (egg_rx_begin*_frc_kernel, egg_rx_mid*_frc_kernel) take these besides.  The list is the handle's, in a small
// device buffer written when it is set; a record has the layout of the ABI's egg_force (40 bytes).
#define EGG_RX_MAX_FORCES 16
#define EGG_RX_FORCE_UNIFORM 0  // = EGG_FORCE_* of include/eggsim.h
#define EGG_RX_FORCE_RADIAL 1
#define EGG_RX_FORCE_VORTEX 2
struct EggForce {
    int32_t kind, type_mask;
    double p[4];
};
struct EggRxForceFields {
    const EggForce *list;                // [count], summed in this order; every lane reads the same record
    int32_t count;
    int32_t type_bit;                    // 1 white, 2 yolk: a field acts when its type_mask has the bit
};

// Viscosity (egg_set_viscosity, DESIGN.md section 2.7, "Viscosity"): one more pass per sub-step, after its last collision
// pass.  insert / scan / scatter are the collision pass's; the viscous rank kernel (egg_rx_rank*_visc_kernel) writes every
// entry's displacement of the sub-step u = pos - prev into the grouped swr slot, and the viscosity gather
// (egg_rx_gather*_visc_kernel) blends u with the weighted mean of the neighbours' within one cell size and rewrites prev.
struct EggRxViscFields {
    double c;                            // the type's coefficient, in (0, 1]
    unsigned long long *pairs;           // one word: distinct pairs within the cell size, over the step's viscosity passes
};

// The ONE argument record of every flavoured kernel of a pass: the base arguments and every field group above.  A kernel
// reads the groups its row below names and nothing else; a group the step's switches leave off stays zero, and a field
// no kernel reads costs the device nothing.  (g.gwr in a viscosity pass: the ghosts' u.)
struct EggRxPassArgs {
    EggRelaxedArgs a;
    EggRxGroupFields g;
    EggRxCohesionFields c;
    EggRxColliderFields d;
    EggRxSurfaceFields s;
    EggRxMotionFields m;
    EggRxSpinFields r;
    EggRxLoadFields l;
    EggRxForceFields f;
    EggRxViscFields v;
};
static_assert(sizeof(EggRxPassArgs) <= 4096, "a kernel's arguments are limited to 4 KB");

// The flavour of a collision pass's gather, by what the handle's collider list asks for; a later one includes the rules of
// the ones before it, and the loads flavour stands in for all of them.
enum EggRxFlavour {
    EGG_RX_NONE, EGG_RX_COL, EGG_RX_SRF, EGG_RX_WALL, EGG_RX_MOV, EGG_RX_SPIN, EGG_RX_LOAD, EGG_RX_FLAVOURS
};

// The ONE list of the flavoured kernels; each takes EggRxPassArgs A.  Their definitions (eggsim_relaxed.hip), their
// declarations and the host's table of gathers (eggsim_host.h) are expansions of it.
//   GATHER(name, G, K, flavour, D, S, W, Mo, Sp, Ld): rx_gather<G, K, D, S, W> with the group fields (G), the cohesion
//     fields (K), the collider fields (D) and the surface fields (S) of A -- an empty constant where the column is 0 -- and
//     with &A.m (Mo), &A.r (Sp), &A.l (Ld) -- null where the column is 0.  The host launches table[G][K][flavour].
//   OTHER(name, call): the kernel's body is the call.
#define EGG_RX_PASS_KERNELS(GATHER, OTHER)                                                                            \
    GATHER(egg_rx_gather_kernel,                     0, 0, EGG_RX_NONE, 0, 0, 0, 0, 0, 0)                              \
    GATHER(egg_rx_gather_group_kernel,               1, 0, EGG_RX_NONE, 0, 0, 0, 0, 0, 0)                              \
    GATHER(egg_rx_gather_coh_kernel,                 0, 1, EGG_RX_NONE, 0, 0, 0, 0, 0, 0)                              \
    GATHER(egg_rx_gather_group_coh_kernel,           1, 1, EGG_RX_NONE, 0, 0, 0, 0, 0, 0)                              \
    GATHER(egg_rx_gather_col_kernel,                 0, 0, EGG_RX_COL,  1, 0, 0, 0, 0, 0)                              \
    GATHER(egg_rx_gather_group_col_kernel,           1, 0, EGG_RX_COL,  1, 0, 0, 0, 0, 0)                              \
    GATHER(egg_rx_gather_coh_col_kernel,             0, 1, EGG_RX_COL,  1, 0, 0, 0, 0, 0)                              \
    GATHER(egg_rx_gather_group_coh_col_kernel,       1, 1, EGG_RX_COL,  1, 0, 0, 0, 0, 0)                              \
    GATHER(egg_rx_gather_col_srf_kernel,             0, 0, EGG_RX_SRF,  1, 1, 0, 0, 0, 0)                              \
    GATHER(egg_rx_gather_group_col_srf_kernel,       1, 0, EGG_RX_SRF,  1, 1, 0, 0, 0, 0)                              \
    GATHER(egg_rx_gather_coh_col_srf_kernel,         0, 1, EGG_RX_SRF,  1, 1, 0, 0, 0, 0)                              \
    GATHER(egg_rx_gather_group_coh_col_srf_kernel,   1, 1, EGG_RX_SRF,  1, 1, 0, 0, 0, 0)                              \
    GATHER(egg_rx_gather_col_wall_kernel,            0, 0, EGG_RX_WALL, 1, 1, 1, 0, 0, 0)                              \
    GATHER(egg_rx_gather_group_col_wall_kernel,      1, 0, EGG_RX_WALL, 1, 1, 1, 0, 0, 0)                              \
    GATHER(egg_rx_gather_coh_col_wall_kernel,        0, 1, EGG_RX_WALL, 1, 1, 1, 0, 0, 0)                              \
    GATHER(egg_rx_gather_group_coh_col_wall_kernel,  1, 1, EGG_RX_WALL, 1, 1, 1, 0, 0, 0)                              \
    GATHER(egg_rx_gather_col_mov_kernel,             0, 0, EGG_RX_MOV,  1, 1, 1, 1, 0, 0)                              \
    GATHER(egg_rx_gather_group_col_mov_kernel,       1, 0, EGG_RX_MOV,  1, 1, 1, 1, 0, 0)                              \
    GATHER(egg_rx_gather_coh_col_mov_kernel,         0, 1, EGG_RX_MOV,  1, 1, 1, 1, 0, 0)                              \
    GATHER(egg_rx_gather_group_coh_col_mov_kernel,   1, 1, EGG_RX_MOV,  1, 1, 1, 1, 0, 0)                              \
    GATHER(egg_rx_gather_col_spin_kernel,            0, 0, EGG_RX_SPIN, 1, 1, 1, 1, 1, 0)                              \
    GATHER(egg_rx_gather_group_col_spin_kernel,      1, 0, EGG_RX_SPIN, 1, 1, 1, 1, 1, 0)                              \
    GATHER(egg_rx_gather_coh_col_spin_kernel,        0, 1, EGG_RX_SPIN, 1, 1, 1, 1, 1, 0)                              \
    GATHER(egg_rx_gather_group_coh_col_spin_kernel,  1, 1, EGG_RX_SPIN, 1, 1, 1, 1, 1, 0)                              \
    GATHER(egg_rx_gather_col_load_kernel,            0, 0, EGG_RX_LOAD, 1, 1, 1, 1, 1, 1)                              \
    GATHER(egg_rx_gather_group_col_load_kernel,      1, 0, EGG_RX_LOAD, 1, 1, 1, 1, 1, 1)                              \
    GATHER(egg_rx_gather_coh_col_load_kernel,        0, 1, EGG_RX_LOAD, 1, 1, 1, 1, 1, 1)                              \
    GATHER(egg_rx_gather_group_coh_col_load_kernel,  1, 1, EGG_RX_LOAD, 1, 1, 1, 1, 1, 1)                              \
    OTHER(egg_rx_rank_coh_kernel,         rx_rank<false, true>(A.a, EggRxGroupFields{}, A.c))                          \
    OTHER(egg_rx_rank_group_coh_kernel,   rx_rank<true, true>(A.a, A.g, A.c))                                          \
    OTHER(egg_rx_begin_frc_kernel,        rx_begin<false, true>(A.a, EggRxGroupFields{}, A.f))                         \
    OTHER(egg_rx_begin_group_frc_kernel,  rx_begin<true, true>(A.a, A.g, A.f))                                         \
    OTHER(egg_rx_mid_frc_kernel,          rx_mid<false, true>(A.a, EggRxGroupFields{}, A.f))                           \
    OTHER(egg_rx_mid_group_frc_kernel,    rx_mid<true, true>(A.a, A.g, A.f))                                           \
    OTHER(egg_rx_gather_visc_kernel,      rx_gather_visc<false>(A.a, EggRxGroupFields{}, A.v))                         \
    OTHER(egg_rx_gather_group_visc_kernel, rx_gather_visc<true>(A.a, A.g, A.v))

// White-yolk coupling (egg_set_coupling, DESIGN.md section 2.7, "Coupling"): one cross-type pass per sub-step, before its
// first collision pass.  Both types build their cell table at the shared cell size H (insert / scan / scatter / rank are
// the collision pass's, with A.cell_size = H), and egg_rx_couple_kernel walks the OTHER type's table from the own type's
// grouped slots.  A single handle only: the key of a particle is its index within its type.
struct EggRxCoupleFields {
    const unsigned long long *hkey;      // the other type's table, as its rank kernel has left it
    const uint32_t *hstart;
    const int32_t *sidx;
    const double2 *spos, *swr;
    uint32_t table_mask;
    int32_t white_is_self;               // 1: the own type is white = side a of every pair, and counts the pairs that fire
    double factor;                       // coupling distance = factor (ra + rb)
    double compliance;                   // _strength_to_compliance(strength, sub_delta) (L:1337-1341)
    double eps;                          // the white config's, on both sides: one pair, one expression
    unsigned long long *solves;          // one word (white side): cross pairs that fired in this step
};
struct EggRelaxedCoupleArgs {
    EggRelaxedArgs a;
    EggRxCoupleFields c;
};

// White-yolk adhesion (egg_set_adhesion, DESIGN.md section 2.7, "Adhesion"): a same-batch band in the coupling pass.  While
// it acts (coupling acts and reach > factor) both tables are built at H = max(1.0, reach (white max_radius + yolk
// max_radius)) through the cohesive rank kernel, which leaves a batch tag per grouped slot -- the atom index, which is one
// for both types of a handle: their atom lists come from the same live-batch order -- and egg_rx_couple_adh_kernel takes
// these besides.  A cross pair beyond the coupling distance, of one batch and within reach (ra + rb), is pulled back to
// the coupling distance through the coupling correction's own arithmetic with the adhesion compliance.
struct EggRxAdhesionFields {
    double reach;                        // band: md < d <= reach (ra + rb)
    double compliance;                   // _strength_to_compliance(adhesion strength, sub_delta)
    const int32_t *stag;                 // the own type's tags, in grouped order (next to A.spos / A.swr)
    const int32_t *other_stag;           // the other type's, next to the spos / swr of EggRxCoupleFields
    unsigned long long *solves;          // one word (white side): cross pairs whose adhesion branch fired in this step
};
struct EggRelaxedCoupleAdhArgs {
    EggRelaxedArgs a;
    EggRxCoupleFields c;
    EggRxAdhesionFields d;
};

// Yolk containment (egg_set_containment, DESIGN.md section 2.7, "Containment"): a disc around the centroid of a batch's
// white, of radius L = factor * (RMS distance of the white from its centroid), that no yolk particle of the batch may
// leave.  Per sub-step egg_rx_contain_sum_kernel summarises every white atom into (cx, cy, L) -- slice `sub` of
// summary[S][atoms][3] -- in the fixed FP64 order of the rule, and egg_rx_contain_kernel projects the yolk particles of
// the same atom index back onto the disc.  The atom index is one for both types of a handle (see adhesion above).
struct EggRxContainSumArgs {
    const double2 *pos;                  // the white positions that enter the sub-step's first collision pass
    const int32_t *atom_offset, *atom_count;
    int32_t n_atoms;
    double factor;
    double *summary;                     // [n_atoms][3] of this sub-step: cx, cy, L
};
struct EggRxContainArgs {
    double2 *pos;                        // the yolk positions that enter the sub-step's first collision pass, rewritten in place
    const int32_t *p_atom;
    int32_t n;
    double strength;
    const double *summary;               // [n_atoms][3] of this sub-step
    unsigned long long *hits;            // one word: projections of this step
    // group only: the cell box of the sub-step's first pass (4 words, filled by the begin / mid kernel), the cell size
    unsigned long long *box;
    double cell_size;
};

// A ghost record: a particle of a sender j that lies within one cell of a receiver k's cell box (40 bytes).  In a viscosity
// pass the two words inv_mass and radius carry u.x and u.y instead (the receiver's unpack copies them as they are).
struct EggGhost {
    double x, y, inv_mass, radius;
    int64_t key;  // global key (below 2^29); with effective cohesion the batch tag in the upper 32 bits, zero otherwise
};
// the key word of a record: atom_tag is null with cohesion off (the word is then the key alone, as ever)
#if defined(__HIPCC__)
static __device__ __forceinline__ int64_t rx_key_word(int32_t key, const int32_t *p_atom, const int32_t *atom_tag, int i) {
    return atom_tag ? (int64_t)(((unsigned long long)(uint32_t)atom_tag[p_atom[i]] << 32) | (uint32_t)key) : (int64_t)key;
}
#endif
#define EGG_RX_MAX_GROUP 16  // handles of one group that relaxed order supports
// Cell box words (zero = empty): [0] max of 2^32 - u(cx), [1] max of u(cx), [2] / [3] the same for cy, u(c) = c + 2^30 + 1.
#define EGG_RX_BOX_BIAS 0x40000001ll
struct EggRxPackArgs {  // sender side: one launch per pass packs for every receiver
    int32_t n, n_recv;                   // local particles; receivers
    double cell_size;
    const double2 *pos;
    const double *inv_mass, *radius;
    const int32_t *ekey;
    const int32_t *p_atom, *atom_tag;    // effective cohesion: the batch tag travels in the key word (null otherwise)
    const unsigned long long *box[EGG_RX_MAX_GROUP];  // each receiver's box for this pass (in the receiver's memory)
    EggGhost *send[EGG_RX_MAX_GROUP];                 // this sender's buffer for each receiver (capacity n)
    unsigned long long *count[EGG_RX_MAX_GROUP];      // records in it (in this sender's memory, zero at the step's start)
};
struct EggRxPackViscArgs {  // the viscosity pass's pack (egg_rx_pack_visc_kernel): the payload words carry pos - prev
    EggRxPackArgs p;
    const double2 *prev;
};
struct EggRxUnpackArgs {  // receiver side: pulls every sender's records for it into the ghost entries
    int32_t n, n_send;                   // local particles; senders
    double2 *pos;                        // positions of this pass; ghosts go to [n + g]
    double2 *gwr;
    int32_t *ekey;
    int32_t *gtag;                       // effective cohesion: the ghosts' batch tags, beside gwr (null otherwise)
    unsigned long long *n_ghost;
    const EggGhost *recs[EGG_RX_MAX_GROUP];           // in the senders' memory
    const unsigned long long *count[EGG_RX_MAX_GROUP];
};

#if defined(__HIPCC__)
// What the kernels of eggsim_relaxed.hip and eggsim_relaxed_wire.hip share.
// cell of a position; false, and cell (0, 0), for a NaN coordinate or a cell outside +-2^30
static __device__ __forceinline__ bool rx_cell(double2 p, double cell, int32_t &cx, int32_t &cy) {
    const double fx = floor(p.x / cell), fy = floor(p.y / cell);
    const bool ok = fx >= -0x1p30 && fx <= 0x1p30 && fy >= -0x1p30 && fy <= 0x1p30;
    cx = ok ? (int32_t)fx : 0;
    cy = ok ? (int32_t)fy : 0;
    return ok;
}

// The test the four senders of the ghost halo share (egg_rx_pack*_kernel, egg_rx_wire_pack*_kernel): a particle's cell
// against a receiver's grown cell box, lo x, hi x, lo y, hi y.
template <typename T>
static __device__ __forceinline__ bool rx_in_box(const T *bx, int32_t cx, int32_t cy) {
    return cx >= bx[0] && cx <= bx[1] && cy >= bx[2] && cy <= bx[3];
}

// Wave-aggregated append: the lanes with `take` get consecutive slots of *counter; returns this lane's slot.
static __device__ __forceinline__ int rx_append(unsigned long long *counter, bool take) {
    const unsigned long long mask = __ballot(take);
    if (!mask) return 0;
    const int lane = (int)(threadIdx.x & 63);
    const int leader = __ffsll((long long)mask) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(counter, (unsigned long long)__popcll(mask));
    base = __shfl(base, leader, 64);
    return (int)base + __popcll(mask & ((1ull << lane) - 1ull));
}
#endif

// Several processes ("Several processes"; eggsim_relaxed_wire.hip): the same halo when the
// other handles live in other processes.  Nothing of another handle is addressable: the destinations' boxes arrive
// as a small array in the sender's own memory, and the ghosts travel as MESSAGES -- word 0 the record count, then
// the 40-byte EggGhost records, contiguous -- which the host hands to the wire and the receiver reads from local memory.
#define EGG_RX_WIRE_BOX 5          // int32 per box: lo_x, lo_y, hi_x, hi_y (cells), empty flag -- egg_rx_box
#define EGG_RX_WIRE_RECORD_WORDS 5 // 64-bit words of a record
struct EggRxWirePackArgs {  // sender side: one launch packs for up to EGG_RX_MAX_GROUP destinations
    int32_t n, n_dest;                   // local particles; destinations of this launch
    double cell_size;
    const double2 *pos;
    const double *inv_mass, *radius;
    const int32_t *ekey;
    const int32_t *p_atom, *atom_tag;    // effective cohesion: the batch tag travels in the key word (null otherwise)
    const int32_t *boxes;                // [n_dest][EGG_RX_WIRE_BOX]: the destinations' boxes for this pass
    unsigned long long *msg;             // [n_dest] messages of `stride` words each (capacity n records, header zeroed)
    long long stride;
};
struct EggRxWirePackViscArgs {  // the viscosity pass's pack (egg_rx_wire_pack_visc_kernel): the payload words carry pos - prev
    EggRxWirePackArgs p;
    const double2 *prev;
};
struct EggRxWireUnpackArgs {  // receiver side: up to EGG_RX_MAX_GROUP received messages into the ghost entries
    int32_t n, n_src;                    // local particles; messages of this launch
    int32_t cap_ghost;                   // ghost entries the arrays hold
    double2 *pos;                        // positions of this pass; ghosts go to [n + g]
    double2 *gwr;
    int32_t *ekey;
    int32_t *gtag;                       // effective cohesion: the ghosts' batch tags, beside gwr (null otherwise)
    unsigned long long *n_ghost;
    const unsigned long long *msg[EGG_RX_MAX_GROUP];  // in this handle's memory
    int32_t cap[EGG_RX_MAX_GROUP];                    // records the host was told each message holds
};

// ---------------------------------------------------------------------------------------------
// Draw of a device group (eggsim_render_group.hip): the particles of ONE source handle and type are copied into the
// render device's shadow arrays, which hold every particle of the group in global-key order.  A RUN is a stretch of
// source particles whose destinations are consecutive too (whole batches; neighbouring batches whose keys are
// neighbours in the group merge into one run).
#define EGG_GATHER_FIELDS 7  // x, y, last_x, last_y, vx, vy, radius: the instanced-draw record (L:513-517)
#define EGG_GATHER_BLOCK 256
struct EggGatherArgs {
    const double *src[EGG_GATHER_FIELDS];  // the source handle's arrays (peer memory when it sits on another device)
    double *dst[EGG_GATHER_FIELDS];        // shadow arrays on the render device
    const int32_t *run_src;    // [n_runs + 1] first source particle of every run, ascending; run_src[n_runs] = n
    const int32_t *run_dst;    // [n_runs] where that particle goes
    const int32_t *block_run;  // [blocks] the run that holds the first particle of every workgroup
    int32_t n, n_runs, n_fields;
    int32_t total;             // particles the shadow arrays hold
};

// egg_draw_pack_kernel (eggsim_draw_pack.hip): the seven draw fields of one handle's particles of a type into ONE message,
// field after field (dst[f * n + i]), particles in the handle's own order.
struct EggDrawPackArgs {
    const double *src[EGG_GATHER_FIELDS];
    double *dst;  // [EGG_GATHER_FIELDS * n]
    int32_t n;
};

// egg_instances_kernel (eggsim_instances.hip): the reference's two per-particle meshes (L:513-523) of n particles -- the
// data mesh, seven floats per particle (egg_instance, 28 B), and the colour mesh, rgba per particle -- from seven source
// arrays: a handle's own, a group's shadow arrays or the external draw source's.
#define EGG_INSTANCE_BLOCK 256
struct EggInstanceArgs {
    const double *src[EGG_GATHER_FIELDS];  // x, y, last_x, last_y, vx, vy, radius
    float *data;                  // [7 n], 16-byte aligned; null: colour only
    float4 *color;                // [n]; null: data only
    const int32_t *atom_offset;   // [n_atoms] first particle of every atom, ascending from 0 (read when color != null)
    const float4 *atom_color;     // [n_atoms] the rgba an atom's particles carry
    int32_t n, n_atoms;
};

// ---------------------------------------------------------------------------------------------
// Sensors (eggsim_sensors.hip; include/eggsim.h, "sensors"): which committed positions lie inside
// the handle's regions.  A UNIT is at most EGG_SN_UNIT consecutive particles of ONE atom; one wave takes a unit at a time,
// a lane a particle of a chunk of 64, and lane k keeps sensor k's sums.  Nothing here is read or written by a step.
#define EGG_SN_MAX_SENSORS 64        // = EGG_MAX_SENSORS: one lane of a wave per sensor
#define EGG_SN_UNIT 1024
#define EGG_SN_SCALE 0x1p16          // = EGG_SENSOR_POSITION_SCALE
#define EGG_SN_LIMIT 0x1p53          // a scaled coordinate that reaches it (or is not finite) drops the particle
#define EGG_SN_HALF_PLANE 0
#define EGG_SN_DISC 1
#define EGG_SN_BOX 2
#define EGG_SN_CAPSULE 3
#define EGG_SN_ROWS 7                // words lane k of a wave leaves: count, sx, sy of white, of yolk; row 6: dropped[lane], lanes 0 and 1
#define EGG_SN_FINISH_THREADS 1024
struct EggSensor {  // egg_sensor
    int32_t kind, type_mask;
    double p[6];
};
struct EggSensorUnit {
    int32_t offset, count;  // particles [offset, offset + count) of the type's arrays, count in 1 .. EGG_SN_UNIT
    int32_t type;           // 0 white, 1 yolk
    int32_t reserved;
};
struct EggSensorArgs {
    const double *x[2], *y[2];        // the committed positions per type
    const EggSensor *sensors;
    const EggSensorUnit *units;
    int32_t n_sensors, n_units;
    long long *partials;              // totals: [waves][EGG_SN_ROWS][64]
    int32_t *unit_counts;             // per batch: [n_units][64], lane k the unit's count in sensor k
};
struct EggSensorFinishArgs {  // a workgroup per row adds the waves' partials: out[row * 64 + k], row 6 the dropped pair
    const long long *partials;
    int32_t n_waves, n_sensors;
    long long *out;                   // [EGG_SN_ROWS][64]
};
struct EggSensorBatchFinishArgs {  // counts[(i * n_sensors + k) * 2 + w] = sum of the units of row r = 2 i + w
    const int32_t *unit_counts;
    const int32_t *row_first, *row_units;  // [n_rows]: the units of (listed id, type), none for a type nothing covers
    int32_t n_rows, n_sensors;
    int32_t *counts;
};
#if defined(__HIPCC__)
// the test of one sensor record for one position (include/eggsim.h): FP64 in exactly this order, no contraction; every
// comparison is false for a NaN.  The ONE definition: the sensors read it through sn_inside, the impulses' regions through
// sn_test, which also hands out the d2 and R of a DISC or CAPSULE (a half-plane and a box leave them untouched).
static __device__ __forceinline__ bool sn_test(const EggSensor &s, double x, double y, double &d2_out, double &R_out) {
    if (s.kind == EGG_SN_HALF_PLANE) {
        const double sd = (s.p[0] * x + s.p[1] * y) - s.p[2];
        return sd >= 0.0;
    }
    if (s.kind == EGG_SN_BOX) {
        const double dx = x - s.p[0], dy = y - s.p[1];
        const double u = dx * s.p[4] + dy * s.p[5];
        const double v = dy * s.p[4] - dx * s.p[5];
        return fabs(u) <= s.p[2] && fabs(v) <= s.p[3];
    }
    double cx = s.p[0], cy = s.p[1], R = s.p[2];
    if (s.kind == EGG_SN_CAPSULE) {  // the nearest point of the segment, as the SEGMENT collider computes it
        const double ex = s.p[2] - s.p[0], ey = s.p[3] - s.p[1];
        const double l2 = ex * ex + ey * ey;
        double t = l2 == 0.0 ? 0.0 : ((x - s.p[0]) * ex + (y - s.p[1]) * ey) / l2;
        if (t < 0.0) t = 0.0;
        if (t > 1.0) t = 1.0;
        cx = s.p[0] + t * ex;
        cy = s.p[1] + t * ey;
        R = s.p[4];
    }
    const double dx = x - cx, dy = y - cy;
    const double d2 = dx * dx + dy * dy;
    d2_out = d2;
    R_out = R;
    return d2 <= R * R;
}
static __device__ __forceinline__ bool sn_inside(const EggSensor &s, double x, double y) {
    double d2, R;
    return sn_test(s, x, y, d2, R);
}
#endif

// ---------------------------------------------------------------------------------------------
// Probes (eggsim_probes.hip; include/eggsim.h, "probes"): the ONE committed particle per probe and
// type that is nearest a point or first along a ray.  The scan walks the units of the shared builder (push_units: at most
// EGG_SN_UNIT consecutive particles of one atom) with one wave per unit; lane k keeps probe k's best.  Nothing here is read
// or written by a step.
#define EGG_PB_MAX_PROBES 64         // = EGG_MAX_PROBES: one lane of a wave per probe
#define EGG_PB_POINT 0
#define EGG_PB_RAY 1
#define EGG_PB_FINISH_THREADS 1024
#define EGG_PB_FINISH_PROBES 8       // probes of one finishing workgroup: their 8 scores are one 64-byte line of a wave's row
typedef EggSensorUnit EggScanUnit;   // the unit of every scan: the shared host layer builds the tables (push_units, eggsim_host_scan.hip)
struct EggProbe {  // egg_probe_query
    int32_t kind, type_mask;
    double p[5];
};
struct EggProbeArgs {
    const double *x[2], *y[2], *radius[2];  // the committed positions and the radii per type
    const EggScanUnit *units;               // ascending array index within a type
    int32_t n_probes, n_units;
    double *part_score;                     // [2][64][waves]: probe k's best score of a wave per type, rows k < n_probes written
    int32_t *part_index;                    // [2][64][waves]: its array index in the type, -1 while there is none
    EggProbe probes[EGG_PB_MAX_PROBES];     // the call's list, in the launch arguments (3 KiB)
};
struct EggProbeOut {  // the winner of one (probe, type)
    double score, x, y, radius;
    int32_t index, reserved;                // array index in the type, -1: no candidate
};
struct EggProbeFinishArgs {  // workgroup (g, w): the best over the waves of probes 8 g .. 8 g + 7 of type w, out[2 k + w]
    const double *part_score;
    const int32_t *part_index;
    const double *x[2], *y[2], *radius[2];
    int32_t n_waves, n_probes;
    EggProbeOut *out;                       // [EGG_PB_MAX_PROBES][2]
};

// ---------------------------------------------------------------------------------------------
// Fields (eggsim_fields.hip; include/eggsim.h, "fields"): the committed particles binned into a
// caller-set grid, a count plane and two int64 velocity-sum planes per type.  The scan walks the units of the shared
// builder (push_units: at most EGG_SN_UNIT consecutive particles of one atom) with one wave per unit.  An atom is one egg's
// blob, so a unit's particles fall into a small rectangle of cells: where that rectangle holds at most EGG_FD_TILE_CELLS
// cells the wave sums it in LDS and adds every non-zero word to the planes once.  Nothing here is read or written by a step.
#define EGG_FD_TILE_CELLS 1024       // cells of a unit's rectangle the tile path holds: 4 KB of counts, 2 x 8 KB of sums
#define EGG_FD_SCALE 0x1p16          // = EGG_FIELD_VELOCITY_SCALE
#define EGG_FD_LIMIT 0x1p53          // a scaled velocity that reaches it (or is not finite) drops the particle
#define EGG_FD_TOTALS 8              // words of the totals: inside, outside, dropped per type, units tiled, units direct
struct EggFieldArgs {
    const double *x[2], *y[2];        // the committed positions per type
    const double *vx[2], *vy[2];      // the committed velocities per type (read by the <true> instantiation only)
    const EggScanUnit *units;
    int32_t n_units;
    int32_t nx, ny;
    int32_t tile_cells;               // 0 .. EGG_FD_TILE_CELLS: the largest rectangle of the tile path, 0 = every unit direct
    double x0, y0, inv;               // inv = 1.0 / cell, computed once on the host
    int32_t *count;                   // [2][ny][nx], zeroed before the launch
    unsigned long long *svx, *svy;    // [2][ny][nx] two's complement sums, zeroed before the launch (<true> only)
    unsigned long long *totals;       // [EGG_FD_TOTALS], zeroed before the launch
};

// ---------------------------------------------------------------------------------------------
// Pieces (eggsim_pieces.hip; include/eggsim.h, "pieces"): the connected pieces of every requested atom
// (the particles of one type of one batch) under the link rule d2 <= L * L, L = reach[type] * (radius[i] + radius[j]).  One
// workgroup per task; the atom's positions, radii, labels and piece sizes stay in dynamic LDS for the whole solve.  Nothing
// here is read or written by a step.
#define EGG_PC_MAX_ATOM 4096         // = EGG_PIECES_MAX_ATOM: 32 bytes of LDS per particle, 128 KB of a compute unit's 160
#define EGG_PC_WAVE_ATOM 512         // atoms up to this size go to the one-wave class, larger ones to the 256-thread class
#define EGG_PC_BLOCK 256             // threads of the second class
#define EGG_PC_OWN 4                 // particles a thread tests against one j read from LDS
#define EGG_PC_LDS_PER_PARTICLE 32   // x, y (16), radius (8), label (4), size (4)
#define EGG_PC_TAIL 64               // bytes of LDS behind the particles: flags and the waves' partial results
struct EggPiecesTask {               // one requested atom
    int32_t offset, count;           // its particles within the type's arrays
    int32_t type;                    // 0 white, 1 yolk
    int32_t slot;                    // its record in `out`
};
struct EggPieceSummary {             // = egg_piece_summary (40 bytes)
    int32_t n, pieces, largest, first, singles, dropped;
    long long sx, sy;
};
struct EggPiecesArgs {
    const double *x[2], *y[2], *radius[2];  // the committed positions and the radii per type
    const EggPiecesTask *tasks;             // the tasks of this launch's class
    int32_t n_tasks;
    double reach[2];
    EggPieceSummary *out;                   // one record per task, at task.slot; every task has a slot of its own
    int32_t *labels[2];                     // per type [n] filled with -1 before the launch, or null
    int32_t *sweeps;                        // sweeps per task at task.slot, or null (a developer figure: it depends on the schedule)
};

// ---------------------------------------------------------------------------------------------
// Impulses (eggsim_impulses.hip; include/eggsim_impulse.h): the committed velocities of the
// particles inside caller-set regions are edited in place, record after record, and integer totals come back.  The scan
// walks the units of the shared builder (push_units: at most EGG_SN_UNIT consecutive particles of one atom; `reserved`
// carries the id of the atom's batch here) with one wave per unit; lane k keeps record k's totals.  The ONLY arrays written
// are vx and vy of the committed state.  No step launches anything of this.
#define EGG_IM_MAX 64                // = EGG_MAX_IMPULSES: one lane of a wave per record
#define EGG_IM_SCALE 0x1p16          // = EGG_IMPULSE_SCALE
#define EGG_IM_LIMIT 0x1p53          // a scaled change of velocity that reaches it (or is not finite) is skipped
#define EGG_IM_KICK 0
#define EGG_IM_BLAST 1
#define EGG_IM_SWIRL 2
#define EGG_IM_BRAKE 3
#define EGG_IM_LINEAR 1
#define EGG_IM_BY_INV_MASS 2
#define EGG_IM_ALL_BATCHES (-1ll)
#define EGG_IM_ROWS 8                // words lane k of a wave leaves: count, sdvx, sdvy, skipped of white, then of yolk
#define EGG_IM_FINISH_THREADS 1024
typedef EggSensor EggRegion;         // a record's region is a sensor record, tested by sn_test
struct EggImpulse {                  // = egg_impulse_record (96 bytes)
    EggRegion region;
    int32_t action, flags;
    long long id;
    double a[3];
};
struct EggImpulseArgs {
    const double *x[2], *y[2], *inv_mass[2];  // the committed positions and the inverse masses per type (read)
    double *vx[2], *vy[2];                    // the committed velocities per type (read and written)
    const EggImpulse *recs;                   // the call's list, checked and normalised
    const EggScanUnit *units;
    int32_t n_recs, n_units;
    int32_t need_inv_mass;                    // some record has EGG_IM_BY_INV_MASS
    long long *partials;                      // [waves][EGG_IM_ROWS][64], or null: no totals are asked for
};
struct EggImpulseFinishArgs {  // a workgroup per row adds the waves' partials: out[row * 64 + k]
    const long long *partials;
    int32_t n_waves, n_recs;
    long long *out;                           // [EGG_IM_ROWS][64]
};

// ---------------------------------------------------------------------------------------------
// Measures (eggsim_measures.hip; include/eggsim_measure.h): per requested atom (the particles of
// one type of one batch) one record of EGG_MS_FIELDS int64 -- counts, quantised sums of position, mass, momentum and
// energy, the extremes, and central second moments about an origin the kernel derives from the first pass.  One workgroup
// per row; a row walks its atom twice.  Read-only on the particle arrays; no step launches anything of this.
#define EGG_MS_FIELDS 24             // = EGG_MEASURE_FIELDS: int64 words of a record
#define EGG_MS_SCALE 0x1p16          // = EGG_MEASURE_SCALE
#define EGG_MS_MASS_SCALE 0x1p32     // = EGG_MEASURE_MASS_SCALE
#define EGG_MS_LIMIT 0x1p53          // a scaled term that reaches it (or is not finite) drops the particle
#define EGG_MS_REGION 1              // = EGG_MEASURE_REGION
#define EGG_MS_BLOCK 256             // threads of a workgroup
#define EGG_MS_WAVE_ATOM 1024        // atoms up to this size are walked by the first wave alone, larger ones by all four
struct EggMeasureRow {               // one requested atom
    int32_t offset, count;           // its particles within the type's arrays, count >= 1
    int32_t type;                    // 0 white, 1 yolk
    int32_t slot;                    // its record in `out`: 2 * (index of the id in the call's list) + type
};
struct EggMeasureArgs {
    const double *x[2], *y[2], *vx[2], *vy[2], *radius[2], *inv_mass[2];  // the committed state per type
    const EggMeasureRow *rows;
    int32_t n_rows;
    int32_t use_region;              // spec.flags & EGG_MS_REGION
    EggRegion region;                // checked and normalised; tested by sn_test, its own type mask included
    long long *out;                  // [slots][EGG_MS_FIELDS]; a slot without a row is zeroed before the launch
};

// ---------------------------------------------------------------------------------------------
// Cover (eggsim_cover.hip; include/eggsim_cover.h): every committed particle's disc of radius
// scale * radius rastered into a caller-set grid -- per cell and type how many discs cover the cell's centre and, on request,
// the smallest batch id among them.  The scan walks the units of the shared builder (push_units: at most EGG_SN_UNIT
// consecutive particles of one atom) with one wave per unit.  A unit has ONE batch, so a tile holds counts only and the
// owner -- the unit's label in its spare word: its batch's id, or its key -- is written where the tile is flushed.  Read-only on the particle
// arrays; no step launches anything of this.
#define EGG_CV_TILE_CELLS 4096       // cells of a unit's union rectangle the tile paths hold: 16 KB of counts
#define EGG_CV_LANES_CELLS 784       // the largest footprint (cells of a disc's rectangle, 28 x 28) of the lane-per-particle path
#define EGG_CV_WAVE_CELLS 784        // the largest footprint of the wave-per-particle path: no wider than the lanes' bound, because
                                     // the sweep (profiles/r35_cover.md) found no footprint at which that path wins; beyond it: direct
#define EGG_CV_MAX_SPAN 64.0         // = EGG_COVER_MAX_SPAN: R * inv beyond it drops the particle
#define EGG_CV_TOTALS 16             // words of the totals: inside, outside, dropped, hits per type, units lanes, wave, direct,
                                     // then (the finishing kernel) covered per type, covered_both, covered_any, one spare
#define EGG_CV_FINISH_THREADS 256
struct EggCoverArgs {
    const double *x[2], *y[2], *radius[2];  // the committed positions and the radii per type
    const EggScanUnit *units;         // `reserved`: what a unit's discs write into the owner plane
    int32_t n_units;
    int32_t nx, ny;
    int32_t tile_cells;               // 0 .. EGG_CV_TILE_CELLS: the largest union rectangle of the tile paths, 0 = every unit direct
    int32_t lanes_cells;              // the largest footprint of the lanes path: 0 = never, INT32_MAX = wherever the tile fits
    int32_t wave_cells;               // the largest footprint of the wave path, taken above lanes_cells; a larger footprint: direct
    double x0, y0, cell, inv, scale;  // inv = 1.0 / cell, computed once on the host
    int32_t *cover;                   // [2][ny][nx], zeroed before the launch
    uint32_t *owner;                  // [2][ny][nx], preset to 0xFFFFFFFF before the launch, or null
    unsigned long long *totals;       // [EGG_CV_TOTALS], zeroed before the launch
};
struct EggCoverFinishArgs {           // covered[2], covered_both, covered_any from the finished cover planes
    const int32_t *cover;             // [2][cells]
    int64_t cells;                    // nx * ny
    unsigned long long *totals;       // words 11 .. 14
};

// ---------------------------------------------------------------------------------------------
// Touches (eggsim_touches.hip; include/eggsim_touch.h): which batches touch which, how much and
// where.  A QUERY is a set of discs of one type with a key; the queries of a call are taken in ROUNDS of at most
// EGG_TC_ROUND, one lane of a wave per query.  A gather kernel writes a round's table -- from the handle's own arrays or from
// discs the caller uploaded, so the scan has one input form --, the scan walks the units of the shared builder (push_units:
// at most EGG_SN_UNIT consecutive particles of one atom; `reserved` the id, or the key, of the unit's batch) with one wave
// per unit.  Read-only on the particle arrays; no step launches anything of this.
#define EGG_TC_ROUND 64              // queries of one round: one lane of a wave per query
#define EGG_TC_OWN (EGG_SN_UNIT / EGG_WAVE)  // particles of a unit a lane keeps in registers: 16, one bit each in the touched mask
#define EGG_TC_FIRST_RECORDS 256     // records the device buffer holds before a call has asked for more
struct EggTouchSource {  // one query as the host lists it
    int32_t offset, count;           // discs [offset, offset + count) of the source arrays of `type`, count >= 1
    int32_t type, slot;              // 0 white, 1 yolk; slot = 2 i + type for entry i of the caller's list
    long long key;                   // the batch the query leaves out: an id or a key as the units carry it, or -1 for none
    long long first;                 // the first disc of the query in the round's disc table
};
struct EggTouchQuery {   // one query of a round, as the gather kernel leaves it (72 bytes)
    long long first;                 // its discs in the disc table
    int32_t count, type, slot, empty;  // empty: no centre without a NaN in x, or none in y -- the query touches nothing
    long long key;
    double lo_x, lo_y, hi_x, hi_y;   // the box of its centres, every coordinate that is not a NaN
    double rmax;                     // the largest |r| that is not a NaN
};
struct EggTouchDisc {    // one disc of a round (48 bytes)
    double x, y, r;
    long long qx, qy;                // rint(x * EGG_SN_SCALE), rint(y * EGG_SN_SCALE); 0 where dropped
    long long dropped;               // 1: a scaled coordinate reaches EGG_SN_LIMIT or is not finite
};
struct EggTouchGatherArgs {
    const double *x[2], *y[2], *r[2];  // the source arrays per type: the handle's committed arrays, or the uploaded discs twice
    const EggTouchSource *sources;   // the round's queries
    int32_t n_queries;               // 1 .. EGG_TC_ROUND
    EggTouchQuery *queries;          // [EGG_TC_ROUND]
    EggTouchDisc *discs;
};
struct EggTouchRecord {  // egg_touch_record: a partial record of one (unit, query)
    int32_t slot, pairs, particles, dropped;
    long long other, sx, sy;
};
struct EggTouchArgs {
    const double *x[2], *y[2], *radius[2];  // the committed positions and the radii per type
    const EggScanUnit *units;        // `reserved`: the id, or the key, of the unit's batch
    int32_t n_units, n_queries;      // n_queries of this round, 1 .. EGG_TC_ROUND
    double reach[2];
    EggTouchRecord *out;             // [cap]
    int32_t cap;
    int32_t *cursor;                 // records asked for so far: it keeps counting past cap
    // (the round's queries and discs are kernel parameters of their own, const and __restrict__: eggsim_touches.hip)
    unsigned long long *candidates;  // developer counter (or null): the (unit, query) pairs the cull let through
};
