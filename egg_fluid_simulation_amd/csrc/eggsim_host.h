// eggsim_host.h -- what the host-side translation units of libeggsim.so share: the handle's state (particle arrays in
// HBM as SoA, batches, tiles, launch classes, the packed pipeline's plan), small helpers and the functions one unit
// calls in another.  Not part of the public ABI (include/eggsim.h).
//
//   eggsim_host_state.hip   particle creation, atoms, device buffers of a particle type
//   eggsim_host_tiling.hip  retile(): claims, islands, tiles, launch classes, the packed pipeline's groups
//   eggsim_host_step.hip    _step: environment scalars, kernel launches, validation / re-run / commit
//   eggsim_host_abi.hip     the extern "C" entry points of include/eggsim.h (except the renderer's)
//   eggsim_host_render.hip  egg_render* : the headless renderer's host side
//   eggsim_host_relaxed.hip _step in relaxed order (EGG_OPT_SOLVER_ORDER = 1): the driver of one (handle, type) -- every
//                           launch of eggsim_relaxed.hip's pass -- and the single handle's step built from it
//   eggsim_host_relaxed_group.hip  that driver over the handles of a device group: the events and peer pack / unpack between passes
//   eggsim_host_relaxed_wire.hip   that driver cut into the C ABI's egg_rx_* calls: one handle per process, the host carries the halo
//   eggsim_host_render_group.hip   draw / environment / download of a device group: gather to one device (eggsim_render_group.hip)
//   eggsim_host_draw_source.hip    the same for a scene sharded over processes: egg_draw_pack on every rank, egg_draw_source_* on one
//   eggsim_host_instances.hip      egg_get_instances / egg_instances_begin / _end: the instanced-draw record packed on the device
//   eggsim_host_sensors.hip        egg_set_sensors / egg_read_sensors / egg_read_sensor_batches: the list, the unit tables, the launches
//   eggsim_host_probes.hip         egg_probe: the checks, the unit table, the two launches, index -> (batch, key, index in the batch)
//   eggsim_host_fields.hip         egg_field / egg_field_to: the checks, the unit table, the zeroing, the one launch, the copies back
//   eggsim_host_pieces.hip         egg_pieces: the checks, the task table, at most two launches, the one copy of the records back
//   eggsim_host_impulses.hip       egg_impulse: the checks, the unit table, at most two launches, the one copy of the totals back
//   eggsim_host_measures.hip       egg_measure / egg_measure_to: the checks, the row table, the one launch, the one copy of the records back
//   eggsim_host_cover.hip          egg_cover / egg_cover_to: the checks, the unit table, the presets, the two launches, the copies back
//   eggsim_host_touches.hip        egg_touches / egg_touches_of: the checks, the queries, the rounds of two launches, the merge of the records
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/eggsim.h"
#include "eggsim_device.h"

extern "C" __global__ void egg_step_kernel(EggStepArgs A);
extern "C" __global__ void egg_step_kernel_gl(EggStepArgs A);
extern "C" __global__ void egg_step_kernel_occ(EggStepArgs A);
extern "C" __global__ void egg_step_kernel_wide(EggStepArgs A);
extern "C" __global__ void egg_env_bounds_kernel(const double *, const double *, const double *, const double *, const double *, int,
                                                   unsigned long long *);
extern "C" __global__ void egg_env_sums_kernel(const double *, const double *, const double *, const double *, int, double *);
extern "C" __global__ void egg_step_kernel_multi(EggStepArgs4 P);
extern "C" __global__ void egg_step_kernel_multi_occ(EggStepArgs4 P);
extern "C" __global__ void egg_step_kernel_multi_wide(EggStepArgs4 P);
extern "C" __global__ void egg_step_kernel_mg(EggStepArgs A);
extern "C" __global__ void egg_step_kernel_gl_mg(EggStepArgs A);
extern "C" __global__ void egg_step_kernel_gs_mg(EggStepArgs A);
extern "C" __global__ void egg_step_kernel_gs(EggStepArgs A);
extern "C" __global__ void egg_selftest_arith_kernel(unsigned long long, int, unsigned long long *);
extern "C" __global__ void egg_selftest_arith_operands_kernel(long long, const double *, const double *, const double *, double *);
extern "C" __global__ void egg_pk_plan_kernel(EggPackedArgs A);
extern "C" __global__ void egg_pk_begin_kernel(EggPackedArgs A);
extern "C" __global__ void egg_pk_mid_kernel(EggPackedArgs A);
extern "C" __global__ void egg_pk_lists_fresh_kernel(EggPackedArgs A);
extern "C" __global__ void egg_pk_lists_stale_kernel(EggPackedArgs A);
extern "C" __global__ void egg_pk_lists_first_kernel(EggPackedArgs A);
extern "C" __global__ void egg_pk_lists_stale_mid_kernel(EggPackedArgs A);
extern "C" __global__ void egg_pk_levels_mr16_kernel(EggPackedArgs A);
extern "C" __global__ void egg_pk_levels_ooo_kernel(EggPackedArgs A);
extern "C" __global__ void egg_pk_probe_lds_order_kernel(int trials, unsigned long long *bad);
extern "C" __global__ void egg_pk_exec_kernel(EggPackedArgs A);
extern "C" __global__ void egg_pk_exec_chain_kernel(EggPackedArgs A);
extern "C" __global__ void egg_pk_levexec_kernel(EggPackedArgs A);
extern "C" __global__ void egg_pk_sort_kernel(EggPackedArgs A);
extern "C" __global__ void egg_pk_sort_direct_kernel(EggPackedArgs A);
extern "C" __global__ void egg_pk_end_kernel(EggPackedArgs A);
extern "C" __global__ void egg_pk_reduce_kernel(EggPackedArgs A, int n_passes);
extern "C" __global__ void egg_rx_atoms_kernel(const int32_t *, const int32_t *, int, int32_t *);
extern "C" __global__ void egg_rx_begin_kernel(EggRelaxedArgs A);
extern "C" __global__ void egg_rx_mid_kernel(EggRelaxedArgs A);
extern "C" __global__ void egg_rx_end_kernel(EggRelaxedArgs A);
extern "C" __global__ void egg_rx_insert_kernel(EggRelaxedArgs A);
extern "C" __global__ void egg_rx_scatter_kernel(EggRelaxedArgs A);
extern "C" __global__ void egg_rx_rank_kernel(EggRelaxedArgs A);
extern "C" __global__ void egg_rx_begin_group_kernel(EggRelaxedGroupArgs A);
extern "C" __global__ void egg_rx_mid_group_kernel(EggRelaxedGroupArgs A);
extern "C" __global__ void egg_rx_insert_group_kernel(EggRelaxedGroupArgs A);
extern "C" __global__ void egg_rx_scatter_group_kernel(EggRelaxedGroupArgs A);
extern "C" __global__ void egg_rx_rank_group_kernel(EggRelaxedGroupArgs A);
// the flavoured kernels: the 28 gathers, the cohesive rank kernels, the force begin / mid kernels, the viscosity gathers
#define EGG_RX_DECLARE(name, ...) extern "C" __global__ void name(EggRxPassArgs A);
EGG_RX_PASS_KERNELS(EGG_RX_DECLARE, EGG_RX_DECLARE)
#undef EGG_RX_DECLARE
extern "C" __global__ void egg_rx_bodies_kernel(EggRxBodiesArgs A);
extern "C" __global__ void egg_rx_contacts_kernel(EggRxContactsArgs A);
extern "C" __global__ void egg_rx_rank_visc_kernel(EggRelaxedArgs A);
extern "C" __global__ void egg_rx_rank_group_visc_kernel(EggRelaxedGroupArgs A);
extern "C" __global__ void egg_rx_couple_kernel(EggRelaxedCoupleArgs K);
extern "C" __global__ void egg_rx_couple_adh_kernel(EggRelaxedCoupleAdhArgs K);
extern "C" __global__ void egg_rx_contain_sum_kernel(EggRxContainSumArgs K);
extern "C" __global__ void egg_rx_contain_kernel(EggRxContainArgs K);
extern "C" __global__ void egg_rx_contain_group_kernel(EggRxContainArgs K);
extern "C" __global__ void egg_rx_pack_visc_kernel(EggRxPackViscArgs P);
extern "C" __global__ void egg_rx_wire_pack_visc_kernel(EggRxWirePackViscArgs P);
extern "C" __global__ void egg_rx_gkey_kernel(const int32_t *, const int32_t *, const int32_t *, int, int32_t *);
extern "C" __global__ void egg_rx_pack_kernel(EggRxPackArgs P);
extern "C" __global__ void egg_rx_unpack_kernel(EggRxUnpackArgs U);
extern "C" __global__ void egg_rx_wire_pack_kernel(EggRxWirePackArgs P);
extern "C" __global__ void egg_rx_wire_unpack_kernel(EggRxWireUnpackArgs U);
extern "C" __global__ void egg_group_gather_kernel(EggGatherArgs A);
extern "C" __global__ void egg_draw_pack_kernel(EggDrawPackArgs A);
extern "C" __global__ void egg_instances_kernel(EggInstanceArgs A);
extern "C" __global__ void egg_sensor_sums_kernel(EggSensorArgs A);
extern "C" __global__ void egg_sensor_units_kernel(EggSensorArgs A);
extern "C" __global__ void egg_sensor_finish_kernel(EggSensorFinishArgs A);
extern "C" __global__ void egg_sensor_batch_finish_kernel(EggSensorBatchFinishArgs A);
extern "C" __global__ void egg_probe_scan_kernel(EggProbeArgs A);
extern "C" __global__ void egg_probe_finish_kernel(EggProbeFinishArgs A);
extern "C" __global__ void egg_field_count_kernel(EggFieldArgs A);
extern "C" __global__ void egg_field_velocity_kernel(EggFieldArgs A);
extern "C" __global__ void egg_pieces_wave_kernel(EggPiecesArgs A);
extern "C" __global__ void egg_pieces_block_kernel(EggPiecesArgs A);
extern "C" __global__ void egg_impulse_kernel(EggImpulseArgs A);
extern "C" __global__ void egg_impulse_quiet_kernel(EggImpulseArgs A);
extern "C" __global__ void egg_impulse_finish_kernel(EggImpulseFinishArgs A);
extern "C" __global__ void egg_measure_kernel(EggMeasureArgs A);
extern "C" __global__ void egg_cover_kernel(EggCoverArgs A);
extern "C" __global__ void egg_cover_finish_kernel(EggCoverFinishArgs A);
extern "C" __global__ void egg_touch_gather_kernel(EggTouchGatherArgs A);
extern "C" __global__ void egg_touch_kernel(EggTouchArgs A, const EggTouchQuery *__restrict__ Q, const EggTouchDisc *__restrict__ D);
extern "C" __global__ void egg_render_count_kernel(EggRenderArgs A);
extern "C" __global__ void egg_render_fill_kernel(EggRenderArgs A);
extern "C" __global__ void egg_render_scan_kernel(EggRenderArgs A);
extern "C" __global__ void egg_render_splat_kernel(EggRenderArgs A);
extern "C" __global__ void egg_render_composite_kernel(EggCompositeArgs A);
extern "C" __global__ void egg_render_clear_kernel(float4 *, size_t, float4);
extern "C" __global__ void egg_render_colliders_kernel(EggColliderDrawArgs A);
extern "C" __global__ void egg_atom_bounds_kernel(const double *, const double *, const int32_t *, const int32_t *,
                                                   int, double, int32_t *);
extern "C" __global__ void egg_rederive_kernel(const double *, double *, double *, int, int, double, double, int,
                                                double, double);
extern "C" __global__ void egg_centroid_kernel(const double *, const double *, const double *, const double *,
                                                const int32_t *, const int32_t *, const int32_t *, const int32_t *,
                                                int, double *, double *);

namespace egghost {


constexpr double kPi = 3.14159265358979323846;
constexpr size_t kLdsMax = 160 * 1024;  // per CU on gfx950; what a workgroup may use is probed at create
constexpr int kMaxTileParticles = 32000;  // 15-bit local indices in the kernel's pair sequences
constexpr int kMaxListEntries = 60000;    // lists in LDS: 16-bit list positions in the transposition's records
constexpr int kMaxGlobalListEntries = 8 << 20;  // lists in global memory (64-bit records): bounded by memory only

extern std::string g_create_error;  // why the last egg_create failed (egg_last_error(NULL))

template <typename T>
struct DevBuf {  // growable device array
    T *p = nullptr;
    size_t cap = 0;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    hipError_t reserve(size_t n, bool keep, hipStream_t s) {
        if (n <= cap) return hipSuccess;
        size_t ncap = std::max<size_t>(n, cap ? cap * 2 : 1024);
        T *q = nullptr;
        hipError_t e = hipMalloc((void **)&q, ncap * sizeof(T));
        if (e != hipSuccess) return e;
        if (keep && p && cap) {
            e = hipMemcpyAsync(q, p, cap * sizeof(T), hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) {
                (void)hipFree(q);
                return e;
            }
        }
        if (p) (void)hipFree(p);
        p = q;
        cap = ncap;
        return hipSuccess;
    }
};

template <typename T>
struct PinnedBuf {  // growable page-locked host array (async copies read/write it without staging)
    T *p = nullptr;
    size_t cap = 0;
    ~PinnedBuf() {
        if (p) (void)hipHostFree(p);
    }
    hipError_t reserve(size_t n) {
        if (n <= cap) return hipSuccess;
        size_t ncap = std::max<size_t>(n, cap ? cap * 2 : 1024);
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipHostMalloc((void **)&p, ncap * sizeof(T), hipHostMallocDefault);
        if (e == hipSuccess) cap = ncap;
        return e;
    }
};

struct Batch {
    int64_t id = 0;
    bool alive = false;
    double target_x = 0, target_y = 0;
    double white_radius = 0, yolk_radius = 0;
    int64_t n[2] = {0, 0};
    int64_t key = 0;  // position in the global creation order; particles are laid out in ascending key
    // render attributes (never read by the solver): the rgba its particles carry (L:978-990, L:1110-1129), and whether
    // the batch's colour table is its own (a colour argument of add) or the config's table (L:49-50)
    float pcolor[2][4] = {{1, 1, 1, 1}, {1, 1, 1, 1}};
    bool own_color[2] = {false, false};
};

struct Atom {
    int32_t batch = 0;  // index into Handle::batches
    int32_t offset = 0, count = 0;
};

struct Box {
    int32_t lo_x, lo_y, hi_x, hi_y;
};

struct LaunchClass {  // tiles of similar size share a launch (uniform LDS geometry)
    int first_tile = 0, n_tiles = 0;
    int nmax = 0, amax = 0, ccap = 0, use_grid = 0, lcap = 0;
    int global_lists = 0;  // visit lists in the scratch buffer instead of LDS
    int global_state = 0;  // everything in the scratch buffer (islands too large for LDS)
    int threads = 0;       // workgroup size
    int wide = 0;          // three lanes per particle for the list-building phases (egg_step_kernel_wide)
    int pair_cache = 0;    // per-pair projection terms cached in LDS (16 B per list entry)
    size_t scratch_stride = 0;
    size_t lds = 0, scratch_offset = 0;
    int packed = -1;       // index into System::pk when the class runs through the packed pipeline (eggsim_packed.hip)
};

// A launch class in the packed pipeline: its tiles' particles occupy [p_begin, p_end) of the type's packed arrays,
// consecutive tiles form GROUPS (one wave of egg_pk_levels / egg_pk_exec each).
struct PackedClass {
    int cls = 0;            // index into System::classes
    int n_tiles = 0, n_groups = 0;
    int p_begin = 0, p_end = 0;
    int tile_base = 0;      // first slot of the class in the per-tile arrays
    int group_base = 0;     // first slot in the per-group arrays
    size_t meta_tile_geo = 0, meta_grp_geo = 0;  // offsets (ints) into System::pk_meta
    int max_group_particles = 0;
    int fused_pass = 0;     // 1: levels, sort and executor of a group are ONE launch (egg_pk_levexec_kernel)
    size_t lds_pass = 0;    // its dynamic LDS: the larger of the two phases
    int lev_lds_cap = 0;    // out-of-order walk: stream entries per tile whose levels the LDS of a launch may hold (sized at re-tiling)
    int lev_lds_now = 0;    // ... and holds in this step's launches: no more than the last step's longest stream + 25 % asks for
    size_t lds_levels_now = 0, lds_pass_now = 0;
    int max_tiles_in_group = 0;
    int levels_ooo = 0;     // the level walk of the class: 0 in order (egg_pk_levels_mr16_kernel), 1 out of order (egg_pk_levels_ooo_kernel)
    int levels_threads = 64; // workgroup of the level walk (up to four waves per group)
    int lcap = 0, scap = 0;  // visit entries / stream words (entries + one header per particle) a tile may have
    int stage_cap = 0;       // partners per particle the list kernel's counting pass keeps in LDS
    int sort_cap = 0;        // words of a group's sorted list
    size_t sort_base = 0;
    int chunk_cap = 0;       // chunk descriptors per group
    size_t chunk_base = 0;
    size_t lds_sort = 0;     // 0: the sort kernel scatters straight into global memory
    size_t entry_base = 0;  // first stream word of the class in the per-entry arrays
    size_t lds_lists = 0, lds_lists_stale = 0, lds_levels = 0, lds_exec = 0;
    int threads_lists = 64, threads_lists_stale = 64;
};

// The relaxed-order path's buffers of one particle type (eggsim_host_relaxed.hip), allocated at its first step.
struct RelaxedBufs {
    DevBuf<double2> pos, pos_next, prev, spos, swr;
    DevBuf<int32_t> pslot, tmp, sidx, p_atom;
    DevBuf<unsigned long long> hkey, status;
    DevBuf<uint32_t> hcount, hstart;
    DevBuf<double> targets;               // [3][atoms]: follow x, follow y, target distance
    DevBuf<unsigned char> scan_tmp;       // hipcub scan scratch
    size_t scan_bytes = 0;
    uint32_t table = 0;                   // hash slots the buffers are sized for
    uint64_t atoms_gen = ~0ull;           // System::atoms_gen p_atom was built for
    PinnedBuf<unsigned long long> h_status;
    PinnedBuf<double> h_targets;
    // device groups (eggsim_host_relaxed_group.hip): entries n.. are ghosts of the other handles' particles
    DevBuf<int32_t> ekey, sloc, abase;    // [n + ghosts] global keys, [n + ghosts] entry of a grouped slot, [atoms] key base
    DevBuf<double2> gwr;                  // [ghosts] (inverse mass, radius)
    DevBuf<int32_t> stag, gtag;           // effective cohesion, allocated once it has been on: [n + ghosts] batch tag of a
                                          // grouped slot, [ghosts] the ghosts' tags
    DevBuf<EggGhost> send;                // [receivers][n] this handle's ghost records for the others
    std::vector<uint64_t> key_sig;        // every handle's atoms_gen when the keys were built
    // several processes (eggsim_host_relaxed_wire.hip): messages = word 0 the record count, then the records
    DevBuf<unsigned long long> wsend, wrecv;  // [destinations][1 + 5 n] packed here; staging copies of the received ones
    DevBuf<int32_t> wbox;                     // [destinations][EGG_RX_WIRE_BOX] the destinations' boxes of a pass
    PinnedBuf<int32_t> h_wbox;
    PinnedBuf<unsigned long long> h_wcount;   // [destinations] record counts of the last pack
    hipEvent_t ev_box[2] = {nullptr, nullptr}, ev_pack[2] = {nullptr, nullptr};  // by pass parity
    RelaxedBufs() = default;
    RelaxedBufs(const RelaxedBufs &) = delete;
    RelaxedBufs &operator=(const RelaxedBufs &) = delete;
    ~RelaxedBufs() {
        for (hipEvent_t e : {ev_box[0], ev_box[1], ev_pack[0], ev_pack[1]})
            if (e) (void)hipEventDestroy(e);
    }
};

struct System {  // one particle type
    egg_config cfg{};
    int64_t n = 0;
    int cur = 0;
    DevBuf<double> x[2], y[2], vx[2], vy[2], inv_mass, radius, mass_t;
    // atoms (host + device mirrors)
    std::vector<Atom> atoms;
    uint64_t atoms_gen = 0;  // counts the rebuilds of `atoms` (upload_atoms)
    DevBuf<int32_t> d_atom_offset, d_atom_count, d_atom_batch;
    // what a step launch reports, in ONE device buffer so that one copy brings it back: two status blocks
    // (the launch writes one and re-initialises the other for the next launch), the atoms' end-of-step cell
    // boxes, their last-sub-step travel
    DevBuf<int32_t> d_out;
    int parity = 0;  // status block of the most recent launch
    hipStream_t wait_stream = nullptr;  // stream the most recent launch of this type went to (the white one when fused)
    int timing_from = 0;                // type whose events time the most recent launch
    int gens = 2;    // hash generations the kernel keeps (n_substeps when n_collision_steps == 1, see PassCtx)
    std::vector<Box> aabb;  // host copy of the atoms' occupied cells
    bool aabb_valid = false;
    bool aabb_on_device = false;  // d_atom_aabb holds the cells of the CURRENT positions (written by the last step)
    bool atoms_dirty = true, targets_dirty = true, tiling_dirty = true;
    bool claims_stale = false;  // a target moved since the tiles were formed
    std::vector<int32_t> disp;                  // per atom: max particle travel of the last step (+x,-x,+y,-y; 1/16 px)
    bool disp_valid = false;                    // fetched together with the boxes of the current positions
    bool swept = false;                          // some claim was extended along predicted motion
    std::vector<int> extra_margin;               // per batch: extra claim cells after a failed check (decays)
    DevBuf<unsigned long long> d_env;            // egg_get_environment: 6 ordered keys + 4 sums
    DevBuf<int32_t> d_atom_fail;                 // per atom: a particle left the claim in the last launch
    // tiles
    std::vector<int32_t> tile_atom_begin, tile_atoms;
    // Per-step metadata (targets, claims, tiles) goes up in ONE async copy from a pinned staging
    // image; the atoms' end-of-step boxes and travel come back in one async copy behind the kernels.
    std::vector<double> h_tx, h_ty, h_fd;
    std::vector<Box> h_claim;
    bool meta_dirty = true;
    PinnedBuf<unsigned char> stage_up, stage_down;
    DevBuf<unsigned char> d_meta;
    size_t meta_off_ty = 0, meta_off_fd = 0, meta_off_claim = 0, meta_off_tbegin = 0, meta_off_tatoms = 0;
    bool out_copied = false;  // stage_down holds this launch's boxes / travel
    bool targets_moving = false;  // the caller moved targets before the most recent step
    bool eager_boxes = true;  // copy the atoms' boxes / travel back behind every step (the scene re-tiles every step: moving
                              // targets); a scene at rest fetches them only when a tiling needs them
    DevBuf<unsigned char> d_scratch;
    std::vector<LaunchClass> classes;
    int margin = 2;
    bool padded = false;   // the current claims carry motion padding or extra margins (see the commit in do_step)
    int since_tiling = 0;  // committed steps on the current tiling
    int single_tile = 0;  // exact-budget mode: everything in one tile
    int uncut_streak = 0;
    double list_factor = 6.0;  // visit-list capacity per particle, grows on overflow
    size_t list_min = 0;
    // environment of the previous step (L:1731-1744)
    bool has_env = false;
    double env_min_mass = 0, env_max_mass = 0, env_min_radius = 0, env_max_radius = 0;
    double tiled_cell_size = 0;
    // parameters of the step the tiles are being formed for (claims are swept along the follow motion)
    double step_follow_compliance = 57.6, step_damping = 0.9;
    int step_substeps = 2;
    bool pk_allowed = true;  // the (sub-steps, passes) shape of the step fits the packed pipeline's per-pass tables
    // packed pipeline (see PackedClass)
    std::vector<PackedClass> pk;
    std::vector<int32_t> pk_meta_host;       // tile_p0 / grp_tile0 of every packed class
    DevBuf<int32_t> pk_meta, pk_src, pk_atom, pk_tile, pk_nchunks;
    DevBuf<double> pk_pos, pk_prev, pk_wr;
    DevBuf<uint32_t> pk_ckey, pk_lists, pk_rank, pk_sorted, pk_levstart, pk_chunks;
    size_t pk_chunk_words = 0;
    DevBuf<uint16_t> pk_lvl, pk_aslot;
    size_t pk_meta_claims = 0;               // offset (ints) of the tile claims inside pk_meta
    int pk_n = 0, pk_tiles = 0, pk_groups = 0;
    size_t pk_entries = 0;                   // stream words over all packed tiles
    size_t pk_sort_words = 0;                // sorted-list words over all packed groups
    int pk_lev_cap = 255;                    // levels the tables hold; grows when a group's DAG is deeper
    int pk_seen_levels = 0;                  // longest dependency chain (levels) of a pass of the last committed step
    unsigned long long pk_seen_list = 0;     // longest pair stream any packed tile had in one pass of the last committed step
    size_t pk_lev_lds_min = 0;               // out-of-order walk: smallest LDS level array (entries per tile) after a fail_levlds
    bool pk_plan_dirty = true;
    // EGG_OPT_TIMING = 2: one event pair per launch group of the packed pipeline, read back when the step is committed
    struct PkStamp { hipEvent_t a, b; int kind, launches; };
    std::vector<PkStamp> pk_stamps;
    size_t pk_stamps_used = 0;
    EggStatus *h_status = nullptr;  // the most recent launch's status block inside stage_down (pinned)
    RelaxedBufs rx;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

constexpr size_t kStatInts = 160;  // one status block, padded to a multiple of 16 bytes
static_assert(sizeof(EggStatus) <= kStatInts * 4, "status block too small");
inline EggStatus *d_stat(System &s, int parity) { return (EggStatus *)(s.d_out.p + parity * kStatInts); }
inline int32_t *d_aabb(System &s) { return s.d_out.p + 2 * kStatInts; }
inline int32_t *d_disp(System &s) { return s.d_out.p + 2 * kStatInts + 4 * s.atoms.size(); }

}  // namespace egghost
namespace egghost {
struct WireStep;  // a relaxed step in flight between egg_rx_begin and egg_rx_end (eggsim_host_relaxed_wire.hip)
struct DrawSource;  // particles placed by egg_draw_source_place, their canvases and scratch (eggsim_host_draw_source.hip)
struct InstanceState;  // staging and pinned buffers of egg_get_instances / egg_instances_begin (eggsim_host_instances.hip)
struct SensorState;  // device copy of the sensor list, unit tables and partials of a read (eggsim_host_sensors.hip)
struct ProbeState;  // unit table, partials and winners of an egg_probe call (eggsim_host_probes.hip)
struct FieldState;  // unit table, planes and totals of an egg_field call (eggsim_host_fields.hip)
struct PiecesState;  // task table, records and labels of an egg_pieces call (eggsim_host_pieces.hip)
struct ImpulseState;  // records, unit table, partials and totals of an egg_impulse call (eggsim_host_impulses.hip)
struct MeasureState;  // row table and records of an egg_measure call (eggsim_host_measures.hip)
struct CoverState;  // unit table, planes and totals of an egg_cover call (eggsim_host_cover.hip)
struct TouchState;  // unit tables, the round's tables and the record buffer of an egg_touches call (eggsim_host_touches.hip)
// egg_handle::collider_dirty: the tables sync_collider_records has to copy (eggsim_host_colliders.hip)
enum : unsigned { kDirtyList = 1u, kDirtySurfaces = 2u, kDirtyMotions = 4u, kDirtySpins = 8u, kDirtyAllTables = 15u };
}
using namespace egghost;

struct egg_handle {
    int device = 0;
    System sys[2];
    std::vector<Batch> batches;  // index = id - 1 (ids are never reused, L:999-1000)
    std::vector<int32_t> order;  // indices of the live batches in ascending key = particle layout order
    int64_t next_key = 1;
    int64_t budget_particles[2] = {-1, -1};  // >= 0: particle count of the budget 0.05 N^2 (multi-GPU: global N)
    int64_t n_alive = 0;
    double elapsed = 0, interpolation_alpha = 0;
    egg_stats stats{};
    std::string error;
    int opt_margin = 2;
    int opt_no_fuse = 0;      // 1: never put both types into one launch
    int opt_tile_target = 60;  // islands smaller than a wave share one (a 15-particle yolk blob uses a quarter of its lanes)
    int opt_timing = 0;
    int opt_force_single = 0;
    int opt_spread = 0;  // threads per particle: 0 = automatic (3 for tiles that have a CU to themselves), else 1..4
    int opt_spin_sleep = -1;  // -1 auto
    bool packed_auto = false;  // the automatic choice, made when the white tiles are formed
    // EGGSIM_TUNE: developer switches, read at egg_create; 0 in normal operation
    //   bit 6 (64):  levels, sort and executor as separate launches instead of the fused pass
    //   bit 7 (128): egg_pk_begin_kernel / egg_pk_mid_kernel as launches of their own and the per-step memset of the
    //                atoms' claim flags, instead of the folded first list pass of every sub-step
    int opt_tune = 0;
    int opt_lists_threads[2] = {0, 0};  // EGGSIM_LISTS_THREADS="fresh,stale": threads of the list kernels' workgroups, 0 = retile()'s choice
    int opt_level_walk = 0;   // packed pipeline, EGG_OPT_LEVEL_WALK: 0 by regime, 1 always in order, 2 out of order wherever the probe allows
    // workgroups of a list kernel a compute unit really admits (registers included), as the runtime reports it for
    // (kernel, threads, dynamic LDS): asked when tiles are formed, once per combination
    struct PkResidency {
        const void *kernel;
        int threads;
        size_t lds;
        int blocks;
    };
    std::vector<PkResidency> pk_residency;  // (blocks 0: the runtime gave no answer)
    bool pk_residency_warned = false;
    DevBuf<uint32_t> simd_claims;   // egg_pk_levexec_kernel: which SIMDs of a compute unit run an executor wave (zero between launches)
    bool lds_lane_ordered = false;  // one ds_add_rtn serves same-address lanes in ascending lane order (probed at create)
    int opt_packed = -1;      // packed pipeline: -1 automatic (large scenes), 0 never, 1 every eligible class
    int opt_group_particles = 0;  // particles one wave of the packed executor keeps in LDS (16 B each): 0 = by scene size (retile), at most 1280
    int opt_solver_order = 0;       // EGG_OPT_SOLVER_ORDER: 0 exact (the reference's pair order), 1 relaxed
    double opt_relaxation = EGG_RELAXATION_DEFAULT;  // EGG_OPT_RELAXATION: omega of the relaxed pass
    int opt_cohesion = 0;           // EGG_OPT_COHESION: 0 dead as in the reference, 1 effective (relaxed order only)
    // static colliders (egg_set_colliders; relaxed order only): the list as egg_get_colliders returns it, and the hits of
    // committed steps per type.
    // THE RULE of the four tables on the device (eggsim_host_colliders.hip, sync_collider_records): while the list is not
    // empty, d_colliders, d_surfaces, d_motions and d_spins each hold one record per collider -- the host's where it has
    // one, the default or zero record where the host's vector is empty.  Whoever changes a host copy, or lets the device
    // run ahead of it, sets the table's bit in collider_dirty; prepare_step copies the marked tables before a step's first
    // launch, and nothing else writes them from the host.
    std::vector<egg_collider> colliders;
    DevBuf<EggCollider> d_colliders;
    unsigned collider_dirty = 0;  // kDirtyList | kDirtySurfaces | kDirtyMotions | kDirtySpins
    bool colliders_wall = false;  // the list holds an EGG_COLLIDER_WALL: a step launches the wall instantiations
    int64_t collider_hits[2] = {0, 0};
    // colliders in the picture (egg_get_collider_pose, egg_set_collider_styles): the list at the start of the last committed
    // relaxed step -- relaxed_commit copies `colliders` into it before it advances them, egg_set_colliders sets both -- and
    // the styles, empty = nothing is drawn, else one record per collider.  Host only: a draw uploads the pose it draws.
    std::vector<egg_collider> colliders_last;
    std::vector<egg_collider_style> styles;
    // collider surfaces (egg_set_collider_surfaces): empty = every surface is the default, else one record per collider;
    // whether any friction > 0 -- only then does a step launch the surface instantiations -- and the grips of committed
    // steps per type
    std::vector<egg_collider_surface> surfaces;
    DevBuf<EggSurface> d_surfaces;
    bool surfaces_grip = false;
    int64_t collider_grips[2] = {0, 0};
    // collider motion (egg_set_collider_motion): empty = every motion is zero, else one record per collider; whether any
    // component is not zero -- only then does a step launch the motion instantiations and a commit advance `colliders`
    std::vector<egg_collider_motion> motions;
    DevBuf<EggMotion> d_motions;
    bool motions_move = false;
    // collider spin (egg_set_collider_spin): empty = every spin is zero, else one record per collider; whether any omega is
    // not zero -- only then does a step launch the spin instantiations and a commit advance the pivots.  spin_table: the
    // step's sines and cosines as prepare_step computes them (libm), (cos, sin)(t omega) per sub-step and collider, then
    // (cos, sin)(h omega) per collider; the commit reads the last sub-step's row, the kernels its copy on the device
    std::vector<egg_collider_spin> spins;
    DevBuf<EggSpin> d_spins;
    bool spins_turn = false;
    std::vector<double2> spin_table;
    DevBuf<double2> d_spin_table;
    // collider loads (egg_set_collider_loads): the switch; the step's sums on the device, 3 words per collider and the
    // dropped word behind them, shared by both types' streams (cleared by prepare_step before either stream starts, read by
    // relaxed_commit once both have been waited for); the sums, the dropped count and the sub-step of the last committed
    // step that had the switch on and a list (zeros after egg_set_colliders)
    bool opt_loads = false;
    DevBuf<unsigned long long> d_loads;
    std::vector<int64_t> load_sums;
    int64_t load_dropped = 0;
    double load_sub_delta = 0.0;
    // collider bodies (egg_set_collider_bodies; relaxed order, one handle only): the records as egg_get_collider_bodies
    // returns them, empty = none; bodies_any = some record frees a translation or a rotation.  A step in which bodies act
    // (relaxed_step, bodies_act) puts the records, the row of turns and the sums the sub-step before has seen on the device, and
    // orders the two types' streams around the integrator with the two events (created by the first such step):
    // body_ready = the other type's last launch of the sub-step, body_done = the integrator of the sub-step
    std::vector<egg_collider_body> bodies;
    bool bodies_any = false;
    bool bodies_step = false;  // the step being committed had bodies acting: the commit reads the device's records back
    DevBuf<EggBody> d_bodies;
    DevBuf<double2> d_body_cs;
    DevBuf<unsigned long long> d_body_seen;
    hipEvent_t body_ready = nullptr, body_done = nullptr;
    // collider contacts (egg_set_collider_contacts; only where bodies act): the records as egg_get_collider_contacts returns
    // them, empty = none; contacts_any = some record is on.  A step in which contacts act puts the records on the device and
    // zeroes the word egg_rx_contacts_kernel counts the step's fires in; the commit adds that word to contact_solves.  The
    // word lives beside the bodies' records, not in a type's status block: a handle without particles has no such block,
    // and its bodies meet all the same.
    std::vector<egg_collider_contact> contacts;
    int32_t contact_iterations = 4;
    bool contacts_any = false;
    bool contacts_step = false;  // the step being committed had contacts acting: the commit reads the word back
    int64_t contact_solves = 0;
    DevBuf<EggContact> d_contacts;
    DevBuf<unsigned long long> d_contact_solves;
    // force fields (egg_set_forces; relaxed order only): the list as egg_get_forces returns it and its copy on the device
    // (written when the list is set, never per step)
    std::vector<egg_force> forces;
    DevBuf<EggForce> d_forces;
    // viscosity (egg_set_viscosity; relaxed order only): the coefficient per type, 0 = off, and the pairs the viscosity
    // passes of committed steps counted per type
    double viscosity[2] = {0.0, 0.0};
    int64_t viscosity_pairs[2] = {0, 0};
    // white-yolk coupling (egg_set_coupling; relaxed order, one handle only): the distance factor, 0 = off, the strength,
    // the cross pairs that fired in committed steps, and the four events of a coupled step (created by the first one):
    // built[w] = type w's table at the coupling cell size is complete, read[w] = type w's couple kernel has read the other
    // type's table
    double coupling_factor = 0.0, coupling_strength = 1.0;
    int64_t coupling_solves = 0;
    hipEvent_t couple_built[2] = {nullptr, nullptr}, couple_read[2] = {nullptr, nullptr};
    // white-yolk adhesion (egg_set_adhesion; a same-batch band in the coupling pass): the reach factor, 0 = off, the
    // strength, and the cross pairs whose adhesion branch fired in committed steps.  It acts in a step exactly when
    // coupling acts and reach > factor.
    double adhesion_reach = 0.0, adhesion_strength = 1.0;
    int64_t adhesion_solves = 0;
    // yolk containment (egg_set_containment; relaxed order, every path): the factor of the disc's radius over the RMS
    // radius of a batch's white, 0 = off, the strength, the projections of committed steps, the summaries of a step
    // ([S][atoms][3]: cx, cy, L) and one event per sub-step (grown on demand): the white stream has written that slice
    double containment_factor = 0.0, containment_strength = 1.0;
    int64_t containment_hits = 0;
    DevBuf<double> contain_summary;
    std::vector<hipEvent_t> contain_summed;
    int opt_force_cell_hash = 0;     // test hook: every launch class keys its cells by the LDS hash table, never the dense grid
    int opt_force_global_state = 0;  // test hook: run every tile through the global-memory-state kernel  // threads per particle in the step kernel's workgroups (pair dataflow spreading)
    hipDeviceProp_t prop{};
    size_t lds_limit = 64 * 1024;  // dynamic LDS a step-kernel workgroup may use
    bool in_flight = false;        // egg_step_begin without its egg_step_end
    // x / y [cur ^ 1] as egg_step_begin found them, per type: the positions at the start of the last committed step
    // (last_x / last_y of draw(), L:1795-1815) live in the buffer the launched step writes; a discard puts them back
    DevBuf<double> flight_last[2][2];
    hipEvent_t flight_saved = nullptr;
    double flight_delta = 0;
    int flight_s = 0, flight_c = 0;
    bool wire_active = false;      // egg_rx_begin without its egg_rx_end
    std::shared_ptr<egghost::WireStep> wire;  // global keys and the step in flight, allocated by the first egg_rx_* call
    std::shared_ptr<egghost::DrawSource> draw_source;  // allocated by the first egg_draw_source_* call
    DevBuf<double> draw_pack;      // egg_draw_pack into host memory: the message before its one copy out
    // counts the successful calls that can change a particle's colour or the particle count (egg_get_instances: a host
    // re-uploads its colour mesh only when this has moved)
    uint64_t color_version = 1;
    std::shared_ptr<egghost::InstanceState> instances;  // allocated by the first egg_get_instances / egg_instances_begin
    // sensors (egg_set_sensors; either solver order): the list as egg_get_sensors returns it, and what a read needs on the
    // device, allocated when a list is first set.  No step reads either.
    std::vector<egg_sensor> sensors;
    std::shared_ptr<egghost::SensorState> sensor_state;
    // probes (egg_probe; either solver order): what a call needs on the device, allocated by the first call that launches.
    // A call stores no list and no answer; no step reads this.
    std::shared_ptr<egghost::ProbeState> probe_state;
    // fields (egg_field / egg_field_to; either solver order): what a call needs on the device, allocated by the first call
    // that launches.  A call stores no grid and no answer; no step reads this.
    std::shared_ptr<egghost::FieldState> field_state;
    // pieces (egg_pieces; either solver order): what a call needs on the device, allocated by the first call that launches.
    // A call stores no answer; no step reads this.
    std::shared_ptr<egghost::PiecesState> pieces_state;
    // impulses (egg_impulse; either solver order): what a call needs on the device, allocated by the first call that
    // launches.  A call stores no list and no answer; no step reads this.
    std::shared_ptr<egghost::ImpulseState> impulse_state;
    // measures (egg_measure / egg_measure_to; either solver order): what a call needs on the device, allocated by the first
    // call that launches.  A call stores no answer; no step reads this.
    std::shared_ptr<egghost::MeasureState> measure_state;
    // cover (egg_cover / egg_cover_to; either solver order): what a call needs on the device, allocated by the first call
    // that launches.  A call stores no grid and no answer; no step reads this.
    std::shared_ptr<egghost::CoverState> cover_state;
    // touches (egg_touches / egg_touches_of; either solver order): what a call needs on the device, allocated by the first
    // call that launches; the record buffer keeps the size the largest answer asked for.  A call stores no answer; no step reads this.
    std::shared_ptr<egghost::TouchState> touch_state;
    // headless renderer (eggsim_render.hip)
    struct Render {
        egg_render_config cfg[2];
        int use_particle_color = 0, use_lighting = 1;  // L:448-449
        int canvas_w[2] = {0, 0}, canvas_h[2] = {0, 0};  // canvases only grow (L:1957-1970)
        double canvas_x0[2] = {0, 0}, canvas_y0[2] = {0, 0};  // world position of the canvases of the last egg_render
        bool canvas_valid = false;
        int last_w[2] = {0, 0}, last_h[2] = {0, 0};  // canvas sizes of the last egg_render
        DevBuf<float4> canvas[2], screen, atom_color;
        DevBuf<float> texture;
        std::vector<float> texture_host;
        int tsize = 0;
        double texture_radius = -1;
        DevBuf<uint32_t> tiles, entries, totals;
        DevBuf<EggDrawCollider> colliders;  // the visible colliders of the frame: layer 0's at 0, layer 1's at EGG_DRAW_MAX_COLLIDERS
    } render;
};
namespace egghost {

int fail(egg_handle *h, int code, const char *fmt, ...);

// state-mutating entry points are refused between egg_step_begin and egg_step_end: the launched step reads the
// arrays and tiles they would change, and egg_step_end validates / commits exactly what was launched
// (refuse_in_flight, eggsim_host_scan.hip, holds the two messages: EGG_OK, or the refusal under `name`)
int refuse_in_flight(egg_handle *h, const char *name);
#define REJECT_IN_FLIGHT(h, name)                                                                      \
    do {                                                                                               \
        const int _rc = egghost::refuse_in_flight(h, name);                                            \
        if (_rc != EGG_OK) return _rc;                                                                 \
    } while (0)

#define HIP_TRY(h, expr)                                                                               \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess)                                                                          \
            return fail(h, EGG_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),      \
                        __FILE__, __LINE__);                                                           \
    } while (0)


inline double clampd(double x, double lo, double hi) {  // math.lua:16-26
    if (x < lo) x = lo;
    if (x > hi) x = hi;
    return x;
}
inline double mixd(double lo, double hi, double t) { return lo * (1 - t) + hi * t; }  // math.lua:33-35

// What the renderer and the environment reductions read.  A handle fills it from its own System (render_source_of); a
// device group fills it from the shadow arrays on its render device and its own records (eggsim_host_render_group.hip).
struct RenderSource {
    egg_handle *h = nullptr;                 // device, LDS limit, error text, launch count: the handle / a group's render handle
    egg_handle::Render *R = nullptr;         // canvases with their grow-only sizes, screen, scratch of the passes
    const egg_render_config *cfg = nullptr;  // [2]
    int use_particle_color = 0, use_lighting = 1;
    bool stepped = false;                    // a _step has run: there are no canvases before (L:1997-1999)
    double alpha = 0;                        // interpolation_alpha of the last update (L:216)
    double max_radius = 0;                   // the larger config max_radius: sizes the density texture (L:626-629)
    hipStream_t stream = nullptr;            // the passes run here ...
    hipStream_t also_wait = nullptr;         // ... after everything on this stream has finished (may be null)
    struct Type {
        const double *x = nullptr, *y = nullptr, *last_x = nullptr, *last_y = nullptr, *vx = nullptr, *vy = nullptr, *radius = nullptr;
        const int32_t *atom_offset = nullptr;  // first particle of every atom, ascending
        int64_t n = 0;
        std::vector<float> atom_color;         // rgba per atom: the colour its particles carry (L:1110-1129)
        hipStream_t env_stream = nullptr;      // stream and scratch (16 words) of the environment reductions
        DevBuf<unsigned long long> *d_env = nullptr;
    } t[2];
    // colliders in the picture (collider_source_of): the two lists the frame's pose is mixed from and the styles; count 0
    // or no styles: nothing of this is drawn and nothing is launched for it
    const egg_collider *colliders = nullptr, *colliders_last = nullptr;
    const egg_collider_style *styles = nullptr;
    int32_t n_colliders = 0;
};
int render_source_of(egg_handle *h, RenderSource &S);  // eggsim_host_render.hip
// the colliders h holds as the frame's: a handle's own, handle 0's for a group, the render rank's for a sharded scene
void collider_source_of(const egg_handle *h, RenderSource &S);
// the pose of egg_get_collider_pose: p = last.p * (1.0 - t) + cur.p * t, kind and mask from cur
void collider_pose(const egg_collider *last, const egg_collider *cur, int32_t n, double t, egg_collider *out);
int render_from(RenderSource &S, const egg_render_params *p, float *rgba, const char *name);
int render_canvas_from(egg_handle *h, egg_handle::Render &R, const char *name, int which, float *rgba, int64_t cap_pixels, int32_t *w,
                       int32_t *hgt, double *x0, double *y0);
// the reductions of egg_get_environment over the arrays of T (eggsim_host_abi.hip)
int environment_of(egg_handle *h, bool stepped, const RenderSource::Type &T, egg_environment *out);
// eggsim_host_instances.hip: the two meshes of egg_get_instances from the arrays T describes -- a handle's own, a
// group's shadow arrays, the external draw source's -- into data / color (host or device memory, either may be null).
// One launch of egg_instances_kernel on `st` of h's device, which is idle when this returns; whatever else wrote the
// arrays must have finished or been put in front of `st`.  Errors go to h under `name`.
int instances_from(egg_handle *h, hipStream_t st, const RenderSource::Type &T, const char *name, egg_instance *data, float *color,
                   int64_t cap, int64_t *n);
// memory of h's device (a kernel may touch it) or anything else (reached through hipMemcpyDefault)
bool on_device_of(const egg_handle *h, const void *p);

Batch *find_batch(egg_handle *h, int64_t id);
const Batch *find_batch(const egg_handle *h, int64_t id);

// the per-particle template of a batch: offsets from the centre, mass factor, mass, radius
// (fibonacci_spiral L:907-918, get_mass L:921-938, add_particle L:941-997)
struct ParticleTemplate {
    std::vector<double> dx, dy, t, inv_mass, radius;
};
void make_template(const egg_config &cfg, double batch_radius, int64_t n_particles, ParticleTemplate &out);
int reserve_particles(egg_handle *h, System &s, int64_t need);
int append_particles(egg_handle *h, System &s, const ParticleTemplate &tp, int64_t n_batches, const double *cx, const double *cy);
int reserve_out(egg_handle *h, System &s, size_t na);
hipError_t wait_step(hipStream_t stream);
int upload_atoms(egg_handle *h, int which);

// eggsim_host_scan.hip: what the calls that scan the committed particles between steps share on the host
int upload_atoms(egg_handle *h);  // both types, white first
// the units of atom a of type w behind `units`: at most EGG_SN_UNIT consecutive particles each
void push_units(const Atom &a, int w, std::vector<EggScanUnit> &units);
// `mask` without the types that have no particles
int covered_types(const egg_handle *h, int mask);
// A feature's table of every unit of the types it covers, on the device.  refresh() rebuilds it when the coverage or the
// atoms of either type moved since it was built and is free otherwise; with_batch_ids puts the id of a unit's batch into
// its spare word -- or, in a table whose by_key is set (once, by the feature that embeds it), the batch's key.  Each feature
// embeds its own: features with different masks would rebuild a shared one in turn.
struct UnitTable {
    bool by_key = false;
    DevBuf<EggScanUnit> d_units;
    uint64_t gen[2] = {~0ull, ~0ull};
    int cover = -1;
    int32_t n_units = 0;
    int refresh(egg_handle *h, const char *name, int cover, bool with_batch_ids);
};
// workgroups of a grid sized to the device, not to the scene: n, at most per_cu per compute unit; env_name (or null)
// names a developer override of per_cu, 1 .. 32, read at every call
int grid_cap(const egg_handle *h, int64_t n, int per_cu_default, const char *env_name);
// `bytes` from p on lie inside one allocation of h's device
bool device_range_fits(const egg_handle *h, const void *p, size_t bytes);
// EGG_OK, or EGG_ERR_UNKNOWN_ID under `name` for the first listed id that names no live batch
int check_batch_ids(egg_handle *h, const char *name, int64_t n_ids, const int64_t *ids);
// the id of every live batch, in h->order
std::vector<int64_t> live_batch_ids(const egg_handle *h);
// the index into sys[w].atoms of every batch of h->batches, -1 where it has none; ONE map serves both types, which list
// the live batches in the same (creation) order (the handle's atoms must be current: upload_atoms)
std::vector<int32_t> atom_of_batch(const egg_handle *h);
// fn(atom, w, slot) for the atom of every listed (known) id and every type of `mask` that has particles, slot = 2 i + w
// for entry i of the list; an atom outside its type's arrays is EGG_ERR_INTERNAL under `name`, a non-zero code of fn ends
// the walk and is returned
template <typename Fn>
int for_each_requested_atom(egg_handle *h, const char *name, int mask, int64_t n_ids, const int64_t *ids, Fn fn) {
    const std::vector<int32_t> atom_of = atom_of_batch(h);
    for (int64_t i = 0; i < n_ids; ++i) {
        const int32_t a = atom_of[(size_t)(find_batch(h, ids[i]) - h->batches.data())];
        for (int w = 0; w < 2; ++w) {
            if (!(mask >> w & 1) || a < 0) continue;
            const Atom &at = h->sys[w].atoms[(size_t)a];
            if (at.count < 1) continue;
            if (at.offset < 0 || (int64_t)at.offset + at.count > h->sys[w].n)
                return fail(h, EGG_ERR_INTERNAL, "%s: atom %d of type %d holds %d particles from %d", name, (int)a, w, (int)at.count, (int)at.offset);
            const int rc = fn(at, w, (int32_t)(2 * i + w));
            if (rc != EGG_OK) return rc;
        }
    }
    return EGG_OK;
}
// the checks and the normalisation egg_set_sensors applies to one region record, for every caller that takes regions:
// EGG_OK, or the failure with `what` and the record's index k in the message (eggsim_host_sensors.hip)
typedef egg_sensor egg_region;
int check_region(egg_handle *h, const char *what, int32_t k, egg_region &o);
double cell_size_of(const egg_config &c);  // L:1756-1760
int fetch_end_aabb(egg_handle *h, System &s);

// eggsim_host_tiling.hip
extern double g_retile_ms[8];  // developer aid (EGGSIM_HOST_PROFILE=1): wall time of retile()'s sections
int retile(egg_handle *h, int which);

// eggsim_host_step.hip
struct Env {  // scalars of update_environment (L:1726-1774)
    double sub_delta, damping, follow_c, collision_c, budget, cell;
    double cohesion_c;  // L:1772 (read by effective cohesion only: the reference's cohesion never moves a particle)
};
Env make_env(const egg_config &c, double sub_delta, int64_t n);
// phase: kWhole = the complete step; kPrepare = tiles/claims only; kBegin = launch the first attempt and
// return (egg_step_begin); kEnd = finish a begun step: validate, re-run if needed, commit (egg_step_end)
enum { kWhole = 0, kPrepare = 1, kBegin = 2, kEnd = 3 };
int do_step(egg_handle *h, double delta, int S, int C, int phase = kWhole);  // L:1722-1989
// the step's config scalars of type w: mass / radius re-derived after a config change (L:1731-1744, L:1420-1430)
int follow_config(egg_handle *h, int w, bool launch);

// eggsim_host_relaxed.hip: a relaxed step of one (handle, type), written once; relaxed_step, relaxed_group_step and the
// egg_rx_* entry points are built from it and agree bit for bit.
constexpr int64_t kRelaxedMaxParticles = (int64_t)1 << 29;  // of one type, over everything that shares a step
#define EGG_RX_TOO_MANY_TEXT "relaxed order: more than 2^29 particles of one type"
constexpr char kRelaxedBadCellText[] = "relaxed order: a position is NaN or its spatial-hash cell lies outside +-2^30";
// Status words of one type: [0] bad cell, [1 + p] pairs of pass p (P = S C passes); with a halo besides, per pass, the
// cell box of its positions, the ghost entries received and -- device groups, nq handles holding the type -- the
// records sent to each of them.  With effective cohesion one more word: the pairs that cohered.  With colliders one
// more: their hits.  With viscosity the halo words cover V = S more passes, the viscosity pass of sub-step `sub` being
// halo pass P + sub, and one more word, the last, holds the pairs the viscosity passes counted.  V = 0 is the layout
// without.  With collider surfaces of which one has friction, or with a wall in the list, one more word behind all of
// these: the grips.  With coupling one more word behind all of these, on the white type only: the cross pairs that fired.
// While adhesion acts one more behind that one, on the white type only: the cross pairs that adhered.  While containment
// acts one more behind that one, the last, on the yolk type only: the projections.
struct RelaxedLayout {
    size_t P = 0, nq = 0;
    bool halo = false;  // ghosts of other handles' particles take part: the group instantiations of the kernels
    bool cohesion = false;  // (set by prepare_type from the handle's option)
    bool colliders = false;  // (set by prepare_type: the handle's collider list is not empty)
    bool forces = false;     // (set by prepare_type: the handle's force list is not empty; no status word of its own)
    size_t V = 0;            // (set by prepare_type: the sub-steps, when the type's viscosity coefficient is not zero)
    bool surfaces = false;   // (set by prepare_type: a collider surface of the handle has friction > 0, or walls, or motion)
    bool walls = false;      // (set by prepare_type: the handle's list holds a wall; implies surfaces)
    bool motion = false;     // (set by prepare_type: a collider motion of the handle is not zero; implies surfaces; no word of its own)
    bool spin = false;       // (set by prepare_type: a collider spin of the handle is not zero; implies surfaces; no word of its own)
    bool loads = false;      // (set by prepare_type: collider loads are on and the list is not empty; no word here: the sums have a buffer of their own)
    bool coupling = false;   // (set by prepare_type: the step runs coupling passes -- no halo, factor > 0, both types populated)
    bool coupled_word = false;  // (set by prepare_type: coupling, and the type is white: it holds the counter word)
    bool adhesion = false;      // (set by prepare_type: coupling, and the handle's adhesion reach exceeds the coupling factor)
    bool adhered_word = false;  // (set by prepare_type: adhesion, and the type is white)
    bool containment = false;    // (set by prepare_type: the handle's containment factor > 0 and both types populated)
    bool contained_word = false;  // (set by prepare_type: containment, and the type is yolk: it holds the counter word)
    size_t H() const { return P + V; }                                        // passes with a halo
    size_t box(size_t p) const { return 1 + P + 4 * p; }                      // 4 words
    size_t ghosts(size_t p) const { return 1 + P + 4 * H() + p; }
    size_t sent(size_t p, size_t m) const { return 1 + P + 5 * H() + p * nq + m; }  // to participant m
    size_t cohered() const { return halo ? 1 + P + 5 * H() + H() * nq : 1 + P; }
    size_t hits() const { return cohered() + (cohesion ? 1 : 0); }
    size_t visc() const { return hits() + (colliders ? 1 : 0); }
    size_t grips() const { return visc() + (V ? 1 : 0); }
    size_t coupled() const { return grips() + (surfaces ? 1 : 0); }
    size_t adhered() const { return coupled() + (coupled_word ? 1 : 0); }
    size_t contained() const { return adhered() + (adhered_word ? 1 : 0); }
    size_t words() const { return contained() + (contained_word ? 1 : 0); }
};
struct RelaxedStep {  // one type of one handle in a relaxed step
    egg_handle *h = nullptr;
    int w = 0, C = 0;
    Env env{};
    RelaxedLayout L;
    // The one argument record (prepare_type fills it; a group whose switch is off stays zero):
    //   A.a  the base arguments                     A.g  the halo's arrays (L.halo)
    //   A.c  effective cohesion (L.cohesion): compliance and factor of the type, the tag arrays
    //   A.d  static colliders (L.colliders): the handle's list, the type's bit, the hit counter
    //   A.s  collider surfaces (L.surfaces, or L.loads): the handle's records, the sub-step, the grip counter
    //   A.m  collider motion (L.motion or L.spin): the handle's records; launch_pass sets the pass's time
    //   A.r  collider spin (L.spin): the handle's records and table; launch_pass sets the pass's row
    //   A.l  collider loads (L.loads): the handle's sums, which rules the list's flavour runs
    //   A.f  force fields (L.forces): the handle's list, the type's bit
    //   A.v  viscosity (L.V): the type's coefficient, the pair counter
    EggRxPassArgs A{};
    EggRelaxedGroupArgs group_args() const { return EggRelaxedGroupArgs{A.a, A.g}; }  // what the unflavoured group kernels take
    EggRxFlavour flavour = EGG_RX_NONE;  // of the collision passes' gather (prepare_type, from L)
    double couple_cell = 0, couple_c = 0;  // coupling (L.coupling): the shared cell size H, the compliance of the strength
    double adhesion_c = 0;                 // adhesion (L.adhesion): the compliance of its own strength
    int64_t ghost_cap = 0;    // a pass runs over n + ghost_cap entries
    int launches = 0;         // kernel launches so far: into the statistics at the commit
    bool bodies = false;      // collider bodies act: launch_pass poses every sub-step as the first over the device's records
};
// key base of a local atom (batch key, particle count) into *base: EGG_OK, or the status it failed the handle with
using KeyBaseFn = std::function<int(int64_t, int64_t, int32_t *)>;
int prepare_step(egg_handle *h, double delta, int S, RelaxedStep st[2]);
// eggsim_host_colliders.hip: establishes the rule of the four collider tables (egg_handle::collider_dirty) for a handle
// whose list is not empty.  No step may be running.
int sync_collider_records(egg_handle *h);
int prepare_type(RelaxedStep &st, int C, size_t ghosts, const RelaxedLayout &L, const std::vector<uint64_t> &sig,
                 const KeyBaseFn &base_of);
int launch_substep(RelaxedStep &st, int sub);
int launch_pass(RelaxedStep &st, int p);
int launch_viscosity(RelaxedStep &st, int sub);
int launch_coupling_tables(RelaxedStep &st);
int launch_coupling(RelaxedStep &st, RelaxedStep &other);
int launch_contain_sum(RelaxedStep &st_white, int sub);
int launch_contain(RelaxedStep &st_yolk, RelaxedStep &st_white, int sub);
int read_status(RelaxedStep &st);
bool bad_cell(const RelaxedStep &st);
int launch_end(RelaxedStep &st);
void relaxed_commit(egg_handle *h, const RelaxedStep st[2], int S, int C, double ms);
int relaxed_step(egg_handle *h, double delta, int S, int C);
void leave_relaxed(egg_handle *h);  // back to exact order: the next exact step re-tiles from the current positions

// eggsim_host_relaxed_group.hip: the relaxed step of a device group (called by eggsim_group.cpp, which declares them
// itself: it sees only include/eggsim.h).  0 or an EGG_ERR_* code; on failure *error names the device and the reason.
int relaxed_group_peers(egg_handle *const *hs, int n, std::string *error);
int group_peers(egg_handle *const *hs, int n, const char *who, const char *what, std::string *error);
// the atoms of all handles of a group in ascending batch key = the group's particle layout order (global keys), per type;
// shared by the relaxed group step (ghost keys) and the group's draw (eggsim_host_render_group.hip).  The atoms of every
// handle must be current (upload_atoms).
struct GroupKeys {
    std::vector<std::pair<int64_t, int64_t>> sizes;  // (batch key, particles of the type), ascending
    std::vector<int64_t> base;                       // global key of the first particle of each
    int64_t total = 0;
    int64_t base_of(int64_t key, int64_t count) const;
};
void group_keys(egg_handle *const *hs, int n, int w, GroupKeys &K);
int relaxed_group_step(egg_handle *const *hs, int n, double delta, int S, int C, int64_t halo_records[1], std::string *error);

// eggsim_host_render_group.hip: what the draw of a device group and the draw of a scene sharded over processes
// (eggsim_host_draw_source.hip) share.  Shadow arrays hold x, y, last_x, last_y, vx, vy, radius (kDrawFields) of ALL
// particles of a type in global-key order on the render device.
struct DrawShadow {
    DevBuf<double> f[EGG_GATHER_FIELDS];
    DevBuf<int32_t> atom_offset;
    DevBuf<unsigned long long> d_env;
};
extern const int kDrawFields[EGG_GATHER_FIELDS];
const double *draw_field_of(System &s, int field);
void gather_table(const std::vector<int32_t> &run_src, const std::vector<int32_t> &run_dst, int64_t n, std::vector<int32_t> &tab);
int launch_gather(egg_handle *rh, hipStream_t st, const double *const *src, DrawShadow &sh, int n_fields, const int32_t *table,
                  int32_t n_runs, int64_t n, int64_t total);
void shadow_source(DrawShadow &sh, int64_t total, hipStream_t env_stream, RenderSource::Type &S);

}  // namespace egghost

