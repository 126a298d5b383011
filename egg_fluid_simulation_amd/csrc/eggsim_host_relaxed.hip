// eggsim_host_relaxed.hip -- SimulationHandler:_step (simulation_handler.lua:1722-1989) in relaxed order
// (EGG_OPT_SOLVER_ORDER = 1): the launches of eggsim_relaxed.hip.  No tiles, claims or re-runs:
// every collision pass is a Jacobi pass over a cell table built fresh from the pass's positions.  The double-buffer
// contract is the exact path's: the step reads x / y / vx / vy[cur], writes the end-of-step state into [cur ^ 1], and
// the commit flips cur.  See eggsim_host.h.
//
// The DRIVER of a relaxed step of one (handle, type) lives here, once: RelaxedStep (eggsim_host.h) with prepare_step,
// prepare_type, launch_substep, launch_pass, read_status, launch_end and relaxed_commit.  Three paths are built from it:
//   relaxed_step (below)                                one handle, everything enqueued in one go
//   relaxed_group_step (eggsim_host_relaxed_group.hip)  the handles of a device group; adds the peer halo between passes
//   egg_rx_* (eggsim_host_relaxed_wire.hip)             one handle per process; the host carries the halo between calls
// With a halo the entries of a pass are the local particles plus ghosts; nothing else differs, and the three paths agree
// bit for bit.
//
// The step's switches (RelaxedLayout L and RelaxedStep, eggsim_host.h; prepare_type sets them).  With a switch off a step
// enqueues and launches what it launched without it, with the same arguments; all three paths pick a switch up from here.
// "Flavour" is the gather of a collision pass, table[halo][cohesion][flavour] over the one kernel list of eggsim_device.h; the
// last column names the event or the status word the switch adds (words: RelaxedLayout).
//
// switch          on while                                      what it changes                                  adds
// --------------  --------------------------------------------  -----------------------------------------------  ----------------------
// L.halo          a group or wire step: ghosts of other         the group instantiations of every kernel; the     per pass a cell box, a
//                 handles' particles take part                  entries of a pass are local particles + ghosts    ghost count, sent counts
// L.cohesion      EGG_OPT_COHESION = 1 (effective)              the cohesive rank kernel and the cohesive row     word cohered()
//                                                               of gathers; A.c: compliance, factor, tag arrays
// L.colliders     egg_set_colliders: the list is not empty      flavour COL; A.d: the list, the type's bit        word hits()
// L.surfaces      egg_set_collider_surfaces: a friction > 0     flavour SRF; A.s: the records (one per collider,  word grips()
//                 (a surface velocity alone does nothing), or   defaults included, while walls, motion or spin)
//                 walls, motion or spin
// L.walls         the list holds an EGG_COLLIDER_WALL           flavour WALL, whether or not a friction is set    -
// L.motion        egg_set_collider_motion: one is not zero      flavour MOV; A.m: the records and the end time    -
//                                                               of the pass's sub-step; relaxed_commit advances
//                                                               the stored list and marks it dirty
// L.spin          egg_set_collider_spin: one is not zero        flavour SPIN; A.r: the records and the sub-step's -
//                                                               row of the table of sines and cosines prepare_step
//                                                               computes with libm and copies (no launch); the
//                                                               commit advances the list and the pivots
// L.loads         egg_set_collider_loads on, list not empty     flavour LOAD in place of whichever the list would -  (the sums have a
//                                                               launch; A.l says which of its rules to run; A.s   buffer of the handle:
//                                                               always filled (no grip word without surfaces)     cleared by prepare_step,
//                                                                                                                 read by relaxed_commit)
// st.bodies       egg_set_collider_bodies: a collider is a      the step is enqueued across both types; LOAD with events body_ready,
//                 body, loads on, list not empty                every rule on; launch_pass poses every sub-step   body_done
//                                                               as the first over the device's records; one
//                                                               egg_rx_bodies_kernel per sub-step rewrites them;
//                                                               the commit reads them back (take_bodies)
// h->contacts_step  egg_set_collider_contacts: bodies act and   one egg_rx_contacts_kernel directly behind every  a counter word of the
//                 a record is on                                integrator launch, same stream, same events       handle (take_contacts)
// L.forces        egg_set_forces: the list is not empty         the force instantiation of begin / mid; A.f       -
// L.V             egg_set_viscosity: the type's coefficient     launch_viscosity ends every sub-step: cell table, word visc(); with a halo
//                 is not zero                                   viscous rank kernel, viscosity gather (5          V more halo passes
//                                                               launches); A.v; the sub-step's last collision
//                                                               pass records the box that pass's halo needs
// L.coupling      egg_set_coupling: factor > 0, both types      the step is enqueued across both types; per       events built[w], read[w];
//                 populated, no halo                            sub-step launch_coupling_tables (4 launches, the  word coupled() (white)
//                                                               shared cell size H) and launch_coupling (1),
//                                                               which walks the OTHER type's table
// L.adhesion      egg_set_adhesion: coupling, reach > factor    the same launches in other instantiations: H      word adhered() (white)
//                                                               covers the band, the tables rank through the
//                                                               cohesive rank kernel, egg_rx_couple_adh_kernel
// L.containment   egg_set_containment: factor > 0, both types   two launches per sub-step in front of its first   one event per sub-step
//                 populated, with or without a halo             pass: launch_contain_sum (white stream, the       (contain_summed);
//                                                               sub-step's slice of summaries), launch_contain    word contained() (yolk)
//                                                               (yolk stream, waits for it and projects)
//
// Every path enqueues the white's launches of a sub-step before the yolk's, so every event has been recorded on the host
// before its wait is enqueued -- a wait on an event that has not been recorded yet waits for nothing -- and nothing is
// written while it may still be read.
#include <hipcub/hipcub.hpp>

#include "eggsim_host.h"

namespace egghost {

namespace {

// the gathers of EGG_RX_PASS_KERNELS (eggsim_device.h) by [halo][cohesion][flavour]: every row of the list fills its one slot
using RxPassKernel = void (*)(EggRxPassArgs);
struct RxGatherTable {
    RxPassKernel k[2][2][EGG_RX_FLAVOURS];
};
#define EGG_RX_SLOT(name, G, K, flavour, ...) t.k[G][K][flavour] = name;
#define EGG_RX_NO_SLOT(name, ...)
const RxGatherTable kRxGather = [] {
    RxGatherTable t{};
    EGG_RX_PASS_KERNELS(EGG_RX_SLOT, EGG_RX_NO_SLOT)
    return t;
}();
#undef EGG_RX_SLOT
#undef EGG_RX_NO_SLOT

// buffers of one type for n particles and `ghosts` ghost entries; the cell table has at least 2 (n + ghosts) slots (a
// probe always finds a free one); `words` status words
int reserve_relaxed(egg_handle *h, System &s, size_t ghosts, size_t words) {
    RelaxedBufs &r = s.rx;
    const size_t n = (size_t)s.n, ne = n + ghosts;
    uint32_t table = 1024;
    while ((size_t)table < 2 * ne) table <<= 1;
    HIP_TRY(h, r.pos.reserve(ne, false, s.stream));
    HIP_TRY(h, r.pos_next.reserve(ne, false, s.stream));
    HIP_TRY(h, r.prev.reserve(n, false, s.stream));
    HIP_TRY(h, r.spos.reserve(ne, false, s.stream));
    HIP_TRY(h, r.swr.reserve(ne, false, s.stream));
    HIP_TRY(h, r.pslot.reserve(ne, false, s.stream));
    HIP_TRY(h, r.tmp.reserve(ne, false, s.stream));
    HIP_TRY(h, r.sidx.reserve(ne, false, s.stream));
    if (r.p_atom.cap < n) r.atoms_gen = ~0ull;  // (a new array: rebuilt below)
    HIP_TRY(h, r.p_atom.reserve(n, false, s.stream));
    if (table != r.table) {
        HIP_TRY(h, r.hkey.reserve(table, false, s.stream));
        HIP_TRY(h, r.hcount.reserve((size_t)table + 1, false, s.stream));
        HIP_TRY(h, r.hstart.reserve((size_t)table + 1, false, s.stream));
        size_t bytes = 0;
        HIP_TRY(h, hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, r.hcount.p, r.hstart.p, (int)table + 1, s.stream));
        HIP_TRY(h, r.scan_tmp.reserve(bytes + 16, false, s.stream));
        r.scan_bytes = bytes;
        r.table = table;
    }
    HIP_TRY(h, r.status.reserve(words, false, s.stream));
    HIP_TRY(h, r.h_status.reserve(words));
    return EGG_OK;
}

// per-particle atoms after the atoms changed, follow targets after they moved (upload_atoms keeps the host copies)
int upload_relaxed_targets(egg_handle *h, System &s) {
    RelaxedBufs &r = s.rx;
    const size_t na = s.atoms.size();
    if (r.atoms_gen != s.atoms_gen) {
        if (na) {
            hipLaunchKernelGGL(egg_rx_atoms_kernel, dim3((unsigned)na), dim3(256), 0, s.stream, s.d_atom_offset.p,
                               s.d_atom_count.p, (int)na, r.p_atom.p);
            HIP_TRY(h, hipGetLastError());
            h->stats.kernel_launches++;
        }
        r.atoms_gen = s.atoms_gen;
        s.meta_dirty = true;
    }
    // meta_dirty: upload_atoms refreshed h_tx / h_ty / h_fd (leave_relaxed sets it again for the exact path's staging)
    if (s.meta_dirty) {
        HIP_TRY(h, r.targets.reserve(3 * na + 1, false, s.stream));
        HIP_TRY(h, r.h_targets.reserve(3 * na + 1));
        // the previous step's copy out of the staging image has completed: every step ends with a stream synchronise
        memcpy(r.h_targets.p, s.h_tx.data(), na * 8);
        memcpy(r.h_targets.p + na, s.h_ty.data(), na * 8);
        memcpy(r.h_targets.p + 2 * na, s.h_fd.data(), na * 8);
        if (na) HIP_TRY(h, hipMemcpyAsync(r.targets.p, r.h_targets.p, 3 * na * 8, hipMemcpyHostToDevice, s.stream));
        s.meta_dirty = false;
    }
    return EGG_OK;
}

// the kernels' arguments for one type's step
EggRelaxedArgs relaxed_args(egg_handle *h, int w, const Env &env) {
    System &s = h->sys[w];
    RelaxedBufs &r = s.rx;
    const int n = (int)s.n;
    const int in = s.cur, out = s.cur ^ 1;
    EggRelaxedArgs A{};
    A.n = n;
    A.table_mask = r.table - 1;
    A.x_in = s.x[in].p;
    A.y_in = s.y[in].p;
    A.vx_in = s.vx[in].p;
    A.vy_in = s.vy[in].p;
    A.x_out = s.x[out].p;
    A.y_out = s.y[out].p;
    A.vx_out = s.vx[out].p;
    A.vy_out = s.vy[out].p;
    A.inv_mass = s.inv_mass.p;
    A.radius = s.radius.p;
    A.p_atom = r.p_atom.p;
    const size_t na = s.atoms.size();
    A.atom_tx = r.targets.p;
    A.atom_ty = r.targets.p + na;
    A.atom_fd = r.targets.p + 2 * na;
    A.pos = r.pos.p;
    A.pos_next = r.pos_next.p;
    A.prev = r.prev.p;
    A.spos = r.spos.p;
    A.swr = r.swr.p;
    A.pslot = r.pslot.p;
    A.tmp = r.tmp.p;
    A.sidx = r.sidx.p;
    A.hkey = r.hkey.p;
    A.hcount = r.hcount.p;
    A.hstart = r.hstart.p;
    A.status = r.status.p;
    A.damping = env.damping;
    A.sub_delta = env.sub_delta;
    A.eps = s.cfg.eps;
    A.follow_compliance = env.follow_c;
    A.collision_compliance = env.collision_c;
    A.overlap = s.cfg.collision_overlap_factor;
    A.cell_size = env.cell;
    A.omega = h->opt_relaxation;
    return A;
}

}  // namespace

// Collider bodies act in a relaxed step of a handle whose list is not empty, holds a body, and records loads.
static bool bodies_act(const egg_handle *h) { return h->bodies_any && h->opt_loads && !h->colliders.empty(); }

// Collider contacts act where bodies act and some contact record is on.
static bool contacts_act(const egg_handle *h) { return bodies_act(h) && h->contacts_any; }

// Per step with bodies acting, over the collider tables prepare_step has synchronised: the body records, the turn (c, s) of
// the first sub-step per collider -- a free-turning body's by the four lines of the integrator, any other's by libm,
// (cos, sin)(h omega) -- and `seen`, which starts at zero with the sums.  The integrator is about to rewrite the list, the
// motions and the spins on the device: they are marked dirty here and take_bodies clears the marks, so a step that is not
// committed -- a failed one -- leaves them for the next step to put the host's untouched copies back.
static int prepare_bodies(egg_handle *h, double sub_delta) {
    const size_t n = h->colliders.size();
    h->collider_dirty |= kDirtyList | kDirtyMotions | kDirtySpins;
    std::vector<double2> cs(n);
    for (size_t k = 0; k < n; ++k) {
        const double omega = h->spins.empty() ? 0.0 : h->spins[k].omega;
        if (h->bodies[k].inv_inertia > 0.0) {
            const double u = 0.5 * (sub_delta * omega);
            const double den = 1.0 + u * u;
            cs[k] = double2{(1.0 - u * u) / den, (u + u) / den};
        } else {
            const double a = sub_delta * omega;
            cs[k] = double2{cos(a), sin(a)};
        }
    }
    const std::vector<unsigned long long> none(3 * n, 0ull);
    HIP_TRY(h, h->d_bodies.reserve(EGG_MAX_COLLIDERS, false, nullptr));
    HIP_TRY(h, h->d_body_cs.reserve(EGG_MAX_COLLIDERS, false, nullptr));
    HIP_TRY(h, h->d_body_seen.reserve(3 * (size_t)EGG_MAX_COLLIDERS, false, nullptr));
    HIP_TRY(h, hipMemcpy(h->d_bodies.p, h->bodies.data(), n * sizeof(egg_collider_body), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->d_body_cs.p, cs.data(), n * sizeof(double2), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->d_body_seen.p, none.data(), none.size() * 8, hipMemcpyHostToDevice));
    return EGG_OK;
}

// Per step with contacts acting, after prepare_bodies: the contact records, and the step's fires start at zero.
static int prepare_contacts(egg_handle *h) {
    const size_t n = h->colliders.size();
    const unsigned long long none = 0ull;
    HIP_TRY(h, h->d_contacts.reserve(EGG_MAX_COLLIDERS, false, nullptr));
    HIP_TRY(h, h->d_contact_solves.reserve(1, false, nullptr));
    HIP_TRY(h, hipMemcpy(h->d_contacts.p, h->contacts.data(), n * sizeof(egg_collider_contact), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->d_contact_solves.p, &none, 8, hipMemcpyHostToDevice));
    return EGG_OK;
}

// per step: the environment scalars of both types (a type without particles has them too: the commit reports its
// budget), config changes and the atoms
int prepare_step(egg_handle *h, double delta, int S, RelaxedStep st[2]) {
    const double sub_delta = std::max(delta / S, h->sys[0].cfg.eps);
    for (int w = 0; w < 2; ++w) {
        System &s = h->sys[w];
        st[w] = RelaxedStep{};
        st[w].h = h;
        st[w].w = w;
        st[w].env = make_env(s.cfg, sub_delta, h->budget_particles[w] >= 0 ? h->budget_particles[w] : s.n);
        int rc = follow_config(h, w, true);
        if (rc == EGG_OK) rc = upload_atoms(h, w);
        if (rc != EGG_OK) return rc;
    }
    if (!h->colliders.empty()) {  // the collider tables of the device, before either type's stream has work (no step is running)
        const int rc = sync_collider_records(h);
        if (rc != EGG_OK) return rc;
    }
    if (h->spins_turn && !h->colliders.empty()) {
        // the step's sines and cosines, by the host's libm (the model's): row sub holds (cos, sin)(t omega) with t the end
        // of sub-step sub, row S holds (cos, sin)(h omega); a pair per collider.  No step is running, so nothing reads the
        // copy on the device while it is written.
        const size_t n = h->colliders.size();
        h->spin_table.assign(((size_t)S + 1) * n, double2{1.0, 0.0});
        for (int sub = 0; sub <= S; ++sub) {
            const double t = sub < S ? (double)(sub + 1) * sub_delta : sub_delta;
            for (size_t k = 0; k < n; ++k) {
                const double a = t * h->spins[k].omega;
                h->spin_table[(size_t)sub * n + k] = double2{cos(a), sin(a)};
            }
        }
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, h->d_spin_table.reserve(h->spin_table.size(), false, nullptr));
        HIP_TRY(h, hipMemcpy(h->d_spin_table.p, h->spin_table.data(), h->spin_table.size() * sizeof(double2), hipMemcpyHostToDevice));
    }
    if (h->opt_loads && !h->colliders.empty()) {
        // the step's sums start at zero, before either type's stream has work (no step is running)
        const size_t n = h->colliders.size();
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, h->d_loads.reserve(3 * (size_t)EGG_MAX_COLLIDERS + 1, false, nullptr));
        const std::vector<unsigned long long> none(3 * n + 1, 0ull);
        HIP_TRY(h, hipMemcpy(h->d_loads.p, none.data(), none.size() * 8, hipMemcpyHostToDevice));
    }
    if (bodies_act(h)) {
        const int rc = prepare_bodies(h, sub_delta);
        return rc == EGG_OK && contacts_act(h) ? prepare_contacts(h) : rc;
    }
    return EGG_OK;
}

// per populated type: buffers for the local particles + `ghosts` ghost entries, targets, kernel arguments.  With a halo
// every entry has a global key: the keys of the local particles are rebuilt when `sig` (whatever the keys depend on)
// differs from the one they were built for, from the key base base_of gives for every local atom (EGG_OK, or the
// status it failed the handle with).
int prepare_type(RelaxedStep &st, int C, size_t ghosts, const RelaxedLayout &L, const std::vector<uint64_t> &sig,
                 const KeyBaseFn &base_of) {
    egg_handle *h = st.h;
    System &s = h->sys[st.w];
    RelaxedBufs &r = s.rx;
    const size_t n = (size_t)s.n;
    st.L = L;
    st.L.cohesion = h->opt_cohesion == EGG_COHESION_EFFECTIVE;
    st.L.colliders = !h->colliders.empty();
    st.L.walls = st.L.colliders && h->colliders_wall;
    st.L.motion = st.L.colliders && h->motions_move;
    st.L.spin = st.L.colliders && h->spins_turn;
    st.L.surfaces = st.L.colliders && (h->surfaces_grip || st.L.walls || st.L.motion || st.L.spin);
    st.L.loads = st.L.colliders && h->opt_loads;
    st.L.forces = !h->forces.empty();
    st.L.V = h->viscosity[st.w] > 0.0 ? L.P / (size_t)C : 0;
    st.L.coupling = !L.halo && h->coupling_factor > 0.0 && h->sys[0].n > 0 && h->sys[1].n > 0;
    st.L.coupled_word = st.L.coupling && st.w == 0;
    st.L.adhesion = st.L.coupling && h->adhesion_reach > h->coupling_factor;
    st.L.adhered_word = st.L.adhesion && st.w == 0;
    st.L.containment = h->containment_factor > 0.0 && h->sys[0].n > 0 && h->sys[1].n > 0;
    st.L.contained_word = st.L.containment && st.w == 1;
    st.C = C;
    st.ghost_cap = (int64_t)ghosts;
    int rc = reserve_relaxed(h, s, ghosts, st.L.words());
    if (rc == EGG_OK) rc = upload_relaxed_targets(h, s);
    if (rc != EGG_OK) return rc;
    st.A = EggRxPassArgs{};
    st.A.a = relaxed_args(h, st.w, st.env);
    // the gather's flavour: the loads instantiation stands in for every other; else the last switch on, which includes the ones before it
    st.flavour = st.L.loads      ? EGG_RX_LOAD
                 : st.L.spin     ? EGG_RX_SPIN
                 : st.L.motion   ? EGG_RX_MOV
                 : st.L.walls    ? EGG_RX_WALL
                 : st.L.surfaces ? EGG_RX_SRF
                 : st.L.colliders ? EGG_RX_COL
                                  : EGG_RX_NONE;
    if (st.L.cohesion) {  // the tag of a particle without a halo is its atom; with one, the atom's key base (below)
        HIP_TRY(h, r.stag.reserve(n + ghosts, false, s.stream));
        st.A.c.compliance = st.env.cohesion_c;
        st.A.c.factor = s.cfg.cohesion_interaction_distance_factor;
        st.A.c.stag = r.stag.p;
        st.A.c.solves = r.status.p + st.L.cohered();
    }
    if (st.L.colliders) {
        st.A.d.list = h->d_colliders.p;
        st.A.d.count = (int32_t)h->colliders.size();
        st.A.d.type_bit = 1 << st.w;
        st.A.d.hits = r.status.p + st.L.hits();
    }
    if (st.L.surfaces || st.L.loads) {  // (loads alone: the records as they are on the device: no friction, so no grip is ever counted)
        st.A.s.list = h->d_surfaces.p;
        st.A.s.sub_delta = st.env.sub_delta;
        st.A.s.grips = st.L.surfaces ? r.status.p + st.L.grips() : nullptr;
    }
    if (st.L.motion || st.L.spin) st.A.m.list = h->d_motions.p;
    if (st.L.spin) {
        st.A.r.list = h->d_spins.p;
        st.A.r.hcs = h->d_spin_table.p + (L.P / (size_t)C) * h->colliders.size();  // (the row behind the sub-steps')
    }
    if (st.L.loads) {
        st.A.l.sums = h->d_loads.p;
        st.A.l.dropped = h->d_loads.p + 3 * h->colliders.size();
        st.A.l.eps = h->sys[0].cfg.eps;
        st.A.l.moving = st.L.motion ? 1 : 0;
        st.A.l.turning = st.L.spin ? 1 : 0;
        st.A.l.pivots = h->spins.empty() ? 0 : 1;
        if (st.A.l.pivots && !st.L.spin) st.A.r.list = h->d_spins.p;
    }
    if (st.L.forces) {
        st.A.f.list = h->d_forces.p;
        st.A.f.count = (int32_t)h->forces.size();
        st.A.f.type_bit = 1 << st.w;
    }
    if (st.L.V) {
        st.A.v.c = h->viscosity[st.w];
        st.A.v.pairs = r.status.p + st.L.visc();
    }
    if (st.L.coupling) {  // both types share the cell size and the compliance
        const double widest = st.L.adhesion ? std::max(h->coupling_factor, h->adhesion_reach) : h->coupling_factor;
        st.couple_cell = std::max(1.0, widest * (h->sys[0].cfg.max_radius + h->sys[1].cfg.max_radius));
        // a coupling distance is at most H, and the pass squares it: with H H finite nothing in the pair arithmetic overflows
        if (!std::isfinite(st.couple_cell * st.couple_cell))
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "relaxed order: the coupling cell size %g (%s %g times the two max_radius) has no finite square",
                        st.couple_cell, st.L.adhesion ? "adhesion reach" : "factor", widest);
        const double alpha = 1 - clampd(h->coupling_strength, 0, 1);  // L:1337-1341
        st.couple_c = alpha / (st.env.sub_delta * st.env.sub_delta);
        for (int k = 0; k < 2; ++k) {
            if (!h->couple_built[k]) HIP_TRY(h, hipEventCreateWithFlags(&h->couple_built[k], hipEventDisableTiming));
            if (!h->couple_read[k]) HIP_TRY(h, hipEventCreateWithFlags(&h->couple_read[k], hipEventDisableTiming));
        }
    }
    if (st.L.adhesion) {  // the tags share the array of effective cohesion: the table of a coupling pass lives between collision passes
        HIP_TRY(h, r.stag.reserve(n + ghosts, false, s.stream));
        st.adhesion_c = (1 - clampd(h->adhesion_strength, 0, 1)) / (st.env.sub_delta * st.env.sub_delta);
    }
    if (st.L.containment)  // one slice of (cx, cy, L) per white atom and sub-step, on the handle (both streams use it)
        HIP_TRY(h, h->contain_summary.reserve(L.P / (size_t)C * h->sys[0].atoms.size() * 3, false, s.stream));
    if (!L.halo) return EGG_OK;
    const bool rebuild = r.key_sig != sig || r.ekey.cap < n + ghosts;  // (or a new array)
    HIP_TRY(h, r.ekey.reserve(n + ghosts, false, s.stream));
    HIP_TRY(h, r.sloc.reserve(n + ghosts, false, s.stream));
    HIP_TRY(h, r.gwr.reserve(std::max<size_t>(ghosts, 1), false, s.stream));
    if (rebuild) {
        // a batch's particles are consecutive in key order, as they are in the handle: key = base + place in the atom
        const size_t na = s.atoms.size();
        std::vector<int32_t> ab(na + 1, 0);
        for (size_t a = 0; a < na; ++a) {
            rc = base_of(h->batches[(size_t)s.atoms[a].batch].key, s.atoms[a].count, &ab[a]);
            if (rc != EGG_OK) return rc;
        }
        HIP_TRY(h, r.abase.reserve(na + 1, false, s.stream));
        HIP_TRY(h, hipMemcpyAsync(r.abase.p, ab.data(), (na + 1) * 4, hipMemcpyHostToDevice, s.stream));
        hipLaunchKernelGGL(egg_rx_gkey_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s.stream, r.p_atom.p,
                           s.d_atom_offset.p, r.abase.p, (int)n, r.ekey.p);
        ++st.launches;
        HIP_TRY(h, hipStreamSynchronize(s.stream));  // (ab is pageable host memory; membership changes only)
        r.key_sig = sig;
    }
    st.A.g.ekey = r.ekey.p;
    st.A.g.sloc = r.sloc.p;
    st.A.g.gwr = r.gwr.p;
    if (st.L.cohesion) {
        HIP_TRY(h, r.gtag.reserve(std::max<size_t>(ghosts, 1), false, s.stream));
        st.A.c.atom_tag = r.abase.p;
        st.A.c.gtag = r.gtag.p;
    }
    return EGG_OK;
}

// sub-step `sub` begins: pre-solve and follow into the positions of its first pass (and their cell box, with a halo).
// The step's status words start at zero.
int launch_substep(RelaxedStep &st, int sub) {
    System &s = st.h->sys[st.w];
    const dim3 grid((unsigned)((s.n + 255) / 256)), block(256);
    if (sub == 0) HIP_TRY(st.h, hipMemsetAsync(s.rx.status.p, 0, st.L.words() * 8, s.stream));
    if (st.L.halo) st.A.g.box = s.rx.status.p + st.L.box((size_t)sub * st.C);
    if (st.L.forces) {
        const RxPassKernel frc[2][2] = {{egg_rx_mid_frc_kernel, egg_rx_begin_frc_kernel}, {egg_rx_mid_group_frc_kernel, egg_rx_begin_group_frc_kernel}};
        hipLaunchKernelGGL(frc[st.L.halo][sub == 0], grid, block, 0, s.stream, st.A);
    } else if (st.L.halo) {
        hipLaunchKernelGGL(sub == 0 ? egg_rx_begin_group_kernel : egg_rx_mid_group_kernel, grid, block, 0, s.stream, st.group_args());
    } else {
        hipLaunchKernelGGL(sub == 0 ? egg_rx_begin_kernel : egg_rx_mid_kernel, grid, block, 0, s.stream, st.A.a);
    }
    ++st.launches;
    return EGG_OK;
}

// The cell table of a pass over n + ghost_cap entries (the ghost count is read on the device) from the positions in
// a.a.pos, at the cell size in a.a.cell_size: two memsets, insert, the scan of the counts, scatter.  With a halo the group
// instantiations.  Two launches; the caller counts them with its own.
static int launch_cell_table(RelaxedStep &st, const EggRxPassArgs &a, dim3 grid, dim3 block) {
    egg_handle *h = st.h;
    System &s = h->sys[st.w];
    RelaxedBufs &r = s.rx;
    const EggRelaxedGroupArgs ga{a.a, a.g};
    HIP_TRY(h, hipMemsetAsync(r.hkey.p, 0xFF, (size_t)r.table * 8, s.stream));
    HIP_TRY(h, hipMemsetAsync(r.hcount.p, 0, ((size_t)r.table + 1) * 4, s.stream));
    if (st.L.halo)
        hipLaunchKernelGGL(egg_rx_insert_group_kernel, grid, block, 0, s.stream, ga);
    else
        hipLaunchKernelGGL(egg_rx_insert_kernel, grid, block, 0, s.stream, a.a);
    size_t bytes = r.scan_bytes;
    HIP_TRY(h, hipcub::DeviceScan::ExclusiveSum(r.scan_tmp.p, bytes, r.hcount.p, r.hstart.p, (int)r.table + 1, s.stream));
    if (st.L.halo)
        hipLaunchKernelGGL(egg_rx_scatter_group_kernel, grid, block, 0, s.stream, ga);
    else
        hipLaunchKernelGGL(egg_rx_scatter_kernel, grid, block, 0, s.stream, a.a);
    return EGG_OK;
}

// collision pass p over the entries: cell table, grouping, the Jacobi gather.  With a halo the ghosts of the pass are in
// place behind the local positions (their count in the status words), and the gather records the cell box of the
// positions it writes for the next pass of the sub-step (the next sub-step's is recorded by its mid kernel) -- with
// viscosity also the sub-step's last, for the viscosity pass that follows it.
int launch_pass(RelaxedStep &st, int p) {
    egg_handle *h = st.h;
    System &s = h->sys[st.w];
    RelaxedBufs &r = s.rx;
    EggRxPassArgs &a = st.A;
    a.a.pass = p;
    if (st.L.halo) {
        a.g.n_ghost = r.status.p + st.L.ghosts((size_t)p);
        a.g.box = p % st.C + 1 < st.C ? r.status.p + st.L.box((size_t)p + 1)
                  : st.L.V            ? r.status.p + st.L.box(st.L.P + (size_t)(p / st.C))
                                      : nullptr;
    }
    if (st.L.motion || st.L.spin) a.m.t = (double)(p / st.C + 1) * st.env.sub_delta;  // the end of the pass's sub-step
    if (st.L.spin) {
        a.r.cs = h->d_spin_table.p + (size_t)(p / st.C) * h->colliders.size();  // the sub-step's row
        a.r.ts = (double)(p / st.C) * st.env.sub_delta;                          // ... and its start
    }
    if (st.bodies) {  // every sub-step is the first of a step over the records the integrator has left on the device
        a.m.t = st.env.sub_delta;
        a.r.cs = h->d_body_cs.p;
        a.r.ts = 0.0;
    }
    const dim3 grid((unsigned)((s.n + st.ghost_cap + 255) / 256)), block(256);  // (the ghost count is read on the device)
    const int rc = launch_cell_table(st, a, grid, block);
    if (rc != EGG_OK) return rc;
    if (st.L.cohesion)
        hipLaunchKernelGGL(st.L.halo ? egg_rx_rank_group_coh_kernel : egg_rx_rank_coh_kernel, grid, block, 0, s.stream, a);
    else if (st.L.halo)
        hipLaunchKernelGGL(egg_rx_rank_group_kernel, grid, block, 0, s.stream, st.group_args());
    else
        hipLaunchKernelGGL(egg_rx_rank_kernel, grid, block, 0, s.stream, a.a);
    hipLaunchKernelGGL(kRxGather.k[st.L.halo][st.L.cohesion][st.flavour], grid, block, 0, s.stream, a);
    st.launches += 5;
    std::swap(a.a.pos, a.a.pos_next);  // Jacobi: the next pass starts from this one's result
    return EGG_OK;
}

// the viscosity pass of sub-step `sub`, after its last collision pass (only with L.V): the cell structure of a collision
// pass over the same entries -- with a halo the ghosts of halo pass P + sub, whose records carry u -- then the viscous rank
// kernel and the viscosity gather, which rewrites prev.  Positions stay: nothing is swapped and no box is recorded.
int launch_viscosity(RelaxedStep &st, int sub) {
    System &s = st.h->sys[st.w];
    EggRxPassArgs &a = st.A;
    if (st.L.halo) {
        a.g.n_ghost = s.rx.status.p + st.L.ghosts(st.L.P + (size_t)sub);
        a.g.box = nullptr;
    }
    const dim3 grid((unsigned)((s.n + st.ghost_cap + 255) / 256)), block(256);  // (the ghost count is read on the device)
    const int rc = launch_cell_table(st, a, grid, block);
    if (rc != EGG_OK) return rc;
    if (st.L.halo)
        hipLaunchKernelGGL(egg_rx_rank_group_visc_kernel, grid, block, 0, s.stream, st.group_args());
    else
        hipLaunchKernelGGL(egg_rx_rank_visc_kernel, grid, block, 0, s.stream, a.a);
    hipLaunchKernelGGL(st.L.halo ? egg_rx_gather_group_visc_kernel : egg_rx_gather_visc_kernel, grid, block, 0, s.stream, a);
    st.launches += 5;
    return EGG_OK;
}

// The coupling pass of a sub-step, first half (only with L.coupling, so without a halo): the type's cell table over the
// positions its begin / mid kernel has just written, at the shared cell size H, into the table buffers of the collision
// passes (free until the sub-step's first one).  built[w] tells the other type's stream that the table is complete.
int launch_coupling_tables(RelaxedStep &st) {
    egg_handle *h = st.h;
    System &s = h->sys[st.w];
    EggRxPassArgs a = st.A;
    a.a.cell_size = st.couple_cell;
    const dim3 grid((unsigned)((s.n + 255) / 256)), block(256);
    const int rc = launch_cell_table(st, a, grid, block);
    if (rc != EGG_OK) return rc;
    if (st.L.adhesion) {  // the tag of a grouped slot is its atom index: one number per batch for both types
        a.c = EggRxCohesionFields{};
        a.c.stag = s.rx.stag.p;
        hipLaunchKernelGGL(egg_rx_rank_coh_kernel, grid, block, 0, s.stream, a);
    } else {
        hipLaunchKernelGGL(egg_rx_rank_kernel, grid, block, 0, s.stream, a.a);
    }
    st.launches += 4;
    HIP_TRY(h, hipEventRecord(h->couple_built[st.w], s.stream));
    return EGG_OK;
}

// Second half: once the other type's table is complete, the couple kernel gathers from it into pos_next; read[w] tells the
// other type's stream that its table may be cleared again.  Jacobi: both types read start-of-pass positions (the grouped
// copies), and the swap makes the result the start of the sub-step's first collision pass.  prev is not touched.
int launch_coupling(RelaxedStep &st, RelaxedStep &other) {
    egg_handle *h = st.h;
    System &s = h->sys[st.w];
    const RelaxedBufs &o = h->sys[other.w].rx;
    HIP_TRY(h, hipStreamWaitEvent(s.stream, h->couple_built[other.w], 0));
    EggRelaxedCoupleArgs k{st.A.a, EggRxCoupleFields{}};
    k.a.cell_size = st.couple_cell;
    k.c.hkey = o.hkey.p;
    k.c.hstart = o.hstart.p;
    k.c.sidx = o.sidx.p;
    k.c.spos = o.spos.p;
    k.c.swr = o.swr.p;
    k.c.table_mask = o.table - 1;
    k.c.white_is_self = st.w == 0;
    k.c.factor = h->coupling_factor;
    k.c.compliance = st.couple_c;
    k.c.eps = h->sys[0].cfg.eps;
    k.c.solves = st.L.coupled_word ? s.rx.status.p + st.L.coupled() : nullptr;
    const dim3 grid((unsigned)((s.n + 255) / 256)), block(256);
    if (st.L.adhesion) {
        EggRxAdhesionFields d{};
        d.reach = h->adhesion_reach;
        d.compliance = st.adhesion_c;
        d.stag = s.rx.stag.p;
        d.other_stag = o.stag.p;
        d.solves = st.L.adhered_word ? s.rx.status.p + st.L.adhered() : nullptr;
        hipLaunchKernelGGL(egg_rx_couple_adh_kernel, grid, block, 0, s.stream, EggRelaxedCoupleAdhArgs{k.a, k.c, d});
    } else {
        hipLaunchKernelGGL(egg_rx_couple_kernel, grid, block, 0, s.stream, k);
    }
    ++st.launches;
    HIP_TRY(h, hipEventRecord(h->couple_read[st.w], s.stream));
    std::swap(st.A.a.pos, st.A.a.pos_next);
    return EGG_OK;
}

// Containment of sub-step `sub`, first half (only with L.containment; st: the white type): the summary of every white
// atom over the positions that enter the sub-step's first collision pass, into slice `sub`, and the sub-step's event.
int launch_contain_sum(RelaxedStep &st, int sub) {
    egg_handle *h = st.h;
    System &s = h->sys[st.w];
    const size_t na = s.atoms.size();
    while (h->contain_summed.size() <= (size_t)sub) {
        hipEvent_t e = nullptr;
        HIP_TRY(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        h->contain_summed.push_back(e);
    }
    EggRxContainSumArgs k{};
    k.pos = st.A.a.pos;
    k.atom_offset = s.d_atom_offset.p;
    k.atom_count = s.d_atom_count.p;
    k.n_atoms = (int32_t)na;
    k.factor = h->containment_factor;
    k.summary = h->contain_summary.p + (size_t)sub * na * 3;
    hipLaunchKernelGGL(egg_rx_contain_sum_kernel, dim3((unsigned)((na + 3) / 4)), dim3(256), 0, s.stream, k);
    ++st.launches;
    HIP_TRY(h, hipEventRecord(h->contain_summed[(size_t)sub], s.stream));
    return EGG_OK;
}

// Second half (st: the yolk type): once the summaries of the sub-step are complete, every yolk particle beyond its batch's
// disc is projected back, in place.  prev is not touched.  With a halo the cells of the written positions go into the box
// of the sub-step's first pass, before the caller records ev_box or reads the box.
int launch_contain(RelaxedStep &st, RelaxedStep &white, int sub) {
    egg_handle *h = st.h;
    System &s = h->sys[st.w];
    HIP_TRY(h, hipStreamWaitEvent(s.stream, h->contain_summed[(size_t)sub], 0));
    EggRxContainArgs k{};
    k.pos = st.A.a.pos;
    k.p_atom = s.rx.p_atom.p;
    k.n = (int32_t)s.n;
    k.strength = h->containment_strength;
    k.summary = h->contain_summary.p + (size_t)sub * h->sys[white.w].atoms.size() * 3;
    k.hits = s.rx.status.p + st.L.contained();
    const dim3 grid((unsigned)((s.n + 255) / 256)), block(256);
    if (st.L.halo) {
        k.box = s.rx.status.p + st.L.box((size_t)sub * st.C);
        k.cell_size = st.env.cell;
        hipLaunchKernelGGL(egg_rx_contain_group_kernel, grid, block, 0, s.stream, k);
    } else {
        hipLaunchKernelGGL(egg_rx_contain_kernel, grid, block, 0, s.stream, k);
    }
    ++st.launches;
    return EGG_OK;
}

// the status words on their way to h_status; bad_cell() reads them once the stream has been waited for
int read_status(RelaxedStep &st) {
    System &s = st.h->sys[st.w];
    HIP_TRY(st.h, hipGetLastError());
    HIP_TRY(st.h, hipMemcpyAsync(s.rx.h_status.p, s.rx.status.p, st.L.words() * 8, hipMemcpyDeviceToHost, s.stream));
    return EGG_OK;
}

bool bad_cell(const RelaxedStep &st) { return st.h->sys[st.w].rx.h_status.p[0] != 0; }

// post-solve: the end-of-step state into [cur ^ 1]
int launch_end(RelaxedStep &st) {
    System &s = st.h->sys[st.w];
    hipLaunchKernelGGL(egg_rx_end_kernel, dim3((unsigned)((s.n + 255) / 256)), dim3(256), 0, s.stream, st.A.a);
    ++st.launches;
    HIP_TRY(st.h, hipGetLastError());
    return EGG_OK;
}

static int relaxed_finish(egg_handle *h, RelaxedStep st[2], int S, int C);

// The integrator of sub-step `sub` on the stream of st's type, behind that type's last launch of the sub-step.
static int launch_bodies(RelaxedStep &st) {
    egg_handle *h = st.h;
    EggRxBodiesArgs k{};
    k.list = h->d_colliders.p;
    k.motions = h->d_motions.p;
    k.spins = h->d_spins.p;
    k.cs = h->d_body_cs.p;
    k.bodies = h->d_bodies.p;
    k.sums = h->d_loads.p;
    k.seen = h->d_body_seen.p;
    k.h = st.env.sub_delta;
    k.count = (int32_t)h->colliders.size();
    hipLaunchKernelGGL(egg_rx_bodies_kernel, dim3(1), dim3(64), 0, h->sys[st.w].stream, k);
    ++st.launches;
    return EGG_OK;
}

// The contacts of sub-step `sub`, directly behind its integrator on the same stream: no event of their own.
static int launch_contacts(RelaxedStep &st) {
    egg_handle *h = st.h;
    EggRxContactsArgs k{};
    k.list = h->d_colliders.p;
    k.motions = h->d_motions.p;
    k.spins = h->d_spins.p;
    k.cs = h->d_body_cs.p;
    k.bodies = h->d_bodies.p;
    k.contacts = h->d_contacts.p;
    k.solves = h->d_contact_solves.p;
    k.h = st.env.sub_delta;
    k.count = (int32_t)h->colliders.size();
    k.iterations = h->contact_iterations;
    hipLaunchKernelGGL(egg_rx_contacts_kernel, dim3(1), dim3(64), 0, h->sys[st.w].stream, k);
    ++st.launches;
    return EGG_OK;
}

// Sub-step `sub` of the types in `on`, enqueued in the one order every step has: begin / mid; with coupling the tables, then
// the couple kernels; containment; then per type the waits, the collision passes and viscosity; with bodies the integrator
// and the contacts.  Called with both types it enqueues across them phase by phase, white first, so that every event a
// stream waits for -- built, read, summed, body_ready, body_done -- has been recorded on the host by then.
//   coupling: before a type's table is cleared again -- by the sub-step's first collision pass, or by launch_viscosity --
//     its stream waits until the other type's couple kernel has read it.
//   bodies: the gathers of both types read the records the integrator writes.  It runs on the stream of the first populated
//     type (`lead`), behind that type's launches of the sub-step; with both types populated it first waits for body_ready,
//     which the other stream records behind its own last launch of the sub-step, and the other stream waits for body_done
//     before its next gather.  Everything in front of a sub-step's first collision pass -- begin / mid, coupling,
//     containment -- reads no collider and runs ahead of that wait.  With one type empty there is one stream and no event.
// No host synchronisation inside the step.
static int enqueue_substep(egg_handle *h, RelaxedStep st[2], const bool on[2], int sub, int C, bool bodies) {
    int rc = EGG_OK;
    const bool both = on[0] && on[1];
    const bool coupled = both && st[0].L.coupling;
    const int lead = on[0] || !on[1] ? 0 : 1;  // (without a particle the integrators still run: a body falls by its own acceleration)
    for (int w = 0; w < 2 && rc == EGG_OK; ++w)
        if (on[w]) rc = launch_substep(st[w], sub);
    for (int w = 0; w < 2 && rc == EGG_OK && coupled; ++w) rc = launch_coupling_tables(st[w]);
    for (int w = 0; w < 2 && rc == EGG_OK; ++w) {
        if (!on[w]) continue;
        if (coupled) rc = launch_coupling(st[w], st[w ^ 1]);
        if (rc == EGG_OK && st[w].L.containment) rc = w == 0 ? launch_contain_sum(st[0], sub) : launch_contain(st[1], st[0], sub);
    }
    for (int w = 0; w < 2 && rc == EGG_OK; ++w) {
        if (!on[w]) continue;
        if (coupled) HIP_TRY(h, hipStreamWaitEvent(h->sys[w].stream, h->couple_read[w ^ 1], 0));
        if (bodies && both && w != lead && sub > 0) HIP_TRY(h, hipStreamWaitEvent(h->sys[w].stream, h->body_done, 0));
        for (int c = 0; c < C && rc == EGG_OK; ++c) rc = launch_pass(st[w], sub * C + c);
        if (rc == EGG_OK && st[w].L.V) rc = launch_viscosity(st[w], sub);
        if (rc == EGG_OK && bodies && both && w != lead) HIP_TRY(h, hipEventRecord(h->body_ready, h->sys[w].stream));
    }
    if (rc != EGG_OK || !bodies) return rc;
    if (both) HIP_TRY(h, hipStreamWaitEvent(h->sys[lead].stream, h->body_ready, 0));
    rc = launch_bodies(st[lead]);
    if (rc == EGG_OK && h->contacts_step) rc = launch_contacts(st[lead]);
    if (rc != EGG_OK) return rc;
    if (both) HIP_TRY(h, hipEventRecord(h->body_done, h->sys[lead].stream));
    return EGG_OK;
}

// The whole step of the types in `on` (st: after prepare_step): their arguments, every sub-step, the end kernels and the
// status words on their way to the host.
static int enqueue_types(egg_handle *h, RelaxedStep st[2], const bool on[2], int S, int C, bool bodies) {
    int rc = EGG_OK;
    for (int w = 0; w < 2; ++w) {
        if (!on[w]) continue;
        if (h->sys[w].n > kRelaxedMaxParticles) return fail(h, EGG_ERR_UNSUPPORTED, EGG_RX_TOO_MANY_TEXT);
        rc = prepare_type(st[w], C, 0, RelaxedLayout{(size_t)S * C, 0, false}, {}, nullptr);
        if (rc != EGG_OK) return rc;
        if (!bodies) continue;
        // the loads instantiation with every rule on, over a motion, a spin and a surface record per collider (A.s has them: loads are on)
        st[w].bodies = true;
        st[w].A.m.list = h->d_motions.p;
        st[w].A.r.list = h->d_spins.p;
        st[w].A.r.hcs = h->d_body_cs.p;
        st[w].A.l.moving = st[w].A.l.turning = st[w].A.l.pivots = 1;
    }
    if (bodies && on[0] && on[1]) {
        if (!h->body_ready) HIP_TRY(h, hipEventCreateWithFlags(&h->body_ready, hipEventDisableTiming));
        if (!h->body_done) HIP_TRY(h, hipEventCreateWithFlags(&h->body_done, hipEventDisableTiming));
    }
    if (bodies) {
        h->bodies_step = true;
        h->contacts_step = contacts_act(h);
    }
    if (h->opt_timing)
        for (int w = 0; w < 2; ++w)
            if (on[w]) HIP_TRY(h, hipEventRecord(h->sys[w].ev0, h->sys[w].stream));
    for (int sub = 0; sub < S; ++sub) {
        rc = enqueue_substep(h, st, on, sub, C, bodies);
        if (rc != EGG_OK) return rc;
    }
    for (int w = 0; w < 2; ++w) {
        if (!on[w]) continue;
        rc = launch_end(st[w]);
        if (rc == EGG_OK) rc = read_status(st[w]);
        if (rc != EGG_OK) return rc;
        if (h->opt_timing) HIP_TRY(h, hipEventRecord(h->sys[w].ev1, h->sys[w].stream));
    }
    return EGG_OK;
}

// One handle, everything enqueued in one go.  With coupling (factor > 0, both types populated) or with collider bodies the
// streams of the two types wait for each other's events, so the step is enqueued sub-step by sub-step across both types;
// otherwise type by type over all sub-steps, white first.
int relaxed_step(egg_handle *h, double delta, int S, int C) {  // L:1722-1989, collision passes relaxed
    h->bodies_step = h->contacts_step = false;
    if (h->bodies_any && !h->colliders.empty() && !h->opt_loads)  // (before anything is launched or copied)
        return fail(h, EGG_ERR_UNSUPPORTED, "relaxed order: collider bodies are integrated from their loads (egg_set_collider_loads with on = 1 first, "
                                            "or egg_set_collider_bodies with n = 0)");
    RelaxedStep st[2];
    int rc = prepare_step(h, delta, S, st);
    if (rc != EGG_OK) return rc;
    const bool on[2] = {h->sys[0].n > 0, h->sys[1].n > 0};
    const bool bodies = bodies_act(h);
    if (bodies || (h->coupling_factor > 0.0 && on[0] && on[1])) {
        rc = enqueue_types(h, st, on, S, C, bodies);
        const int lead = on[0] || !on[1] ? 0 : 1;
        if (rc == EGG_OK && bodies && !on[lead]) HIP_TRY(h, hipStreamSynchronize(h->sys[lead].stream));  // (relaxed_finish waits for populated types only)
    } else {
        const bool white[2] = {on[0], false}, yolk[2] = {false, on[1]};
        rc = enqueue_types(h, st, white, S, C, false);
        if (rc == EGG_OK) rc = enqueue_types(h, st, yolk, S, C, false);
    }
    return rc == EGG_OK ? relaxed_finish(h, st, S, C) : rc;
}

// a relaxed step whose launches are all enqueued: wait for both types, then fail on a bad cell or commit
static int relaxed_finish(egg_handle *h, RelaxedStep st[2], int S, int C) {
    double ms = 0;
    bool bad = false;
    for (int w = 0; w < 2; ++w) {
        System &s = h->sys[w];
        if (s.n == 0) continue;
        HIP_TRY(h, wait_step(s.stream));
        if (h->opt_timing) {
            float t = 0;
            HIP_TRY(h, hipEventElapsedTime(&t, s.ev0, s.ev1));
            h->stats.kernel_ms[w] = (double)t;
            ms = std::max(ms, (double)t);
        }
        bad |= bad_cell(st[w]);
    }
    if (bad) {  // nothing is committed: [cur] still holds the state before the step
        // ... and the records the integrator has rewritten stay marked dirty (prepare_bodies): the next step runs on the
        // host's untouched copies again.  The fires of the failed step are never read.
        h->bodies_step = h->contacts_step = false;
        h->stats.kernel_launches += st[0].launches + st[1].launches;
        return fail(h, EGG_ERR_UNSUPPORTED, "%s", kRelaxedBadCellText);
    }
    relaxed_commit(h, st, S, C, ms);
    return EGG_OK;
}

// Collider motion at the commit: the stored geometry of every collider becomes the geometry of the step's end, t = S h
// -- the expression the kernels of the last sub-step evaluated, so the same bits -- and the list is marked dirty: the copy
// on the device follows before the next step's first launch (sync_collider_records).
// Collider spin: a collider whose omega is not zero turns about its pivot, which rides on its motion, by the (c, s) of the
// last sub-step's row of the step's table, and its stored pivot becomes the pivot of the step's end; the spin records are
// marked dirty with the list.
static void advance_colliders(egg_handle *h, double t, int S) {
    if (h->bodies_step) return;  // (take_bodies has read the device's records, advanced sub-step by sub-step)
    const size_t n = h->colliders.size();
    for (size_t k = 0; k < n; ++k) {
        egg_collider &c = h->colliders[k];
        const egg_collider_motion m = h->motions.empty() ? egg_collider_motion{0.0, 0.0} : h->motions[k];
        const double ox = t * m.vx, oy = t * m.vy;
        if (h->spins_turn && h->spins[k].omega != 0.0) {
            egg_collider_spin &sp = h->spins[k];
            const double2 cs = h->spin_table[(size_t)(S - 1) * n + k];
            const double Px = sp.px + ox, Py = sp.py + oy;
            if (c.kind == EGG_COLLIDER_HALF_PLANE) {
                const double keep = c.p[2] - (c.p[0] * sp.px + c.p[1] * sp.py);
                const double nx = cs.x * c.p[0] - cs.y * c.p[1], ny = cs.y * c.p[0] + cs.x * c.p[1];
                c.p[0] = nx;
                c.p[1] = ny;
                c.p[2] = (nx * Px + ny * Py) + keep;
            } else {
                const double rx = c.p[0] - sp.px, ry = c.p[1] - sp.py;
                c.p[0] = Px + (cs.x * rx - cs.y * ry);
                c.p[1] = Py + (cs.y * rx + cs.x * ry);
                if (c.kind == EGG_COLLIDER_SEGMENT || c.kind == EGG_COLLIDER_WALL) {
                    const double qx = c.p[2] - sp.px, qy = c.p[3] - sp.py;
                    c.p[2] = Px + (cs.x * qx - cs.y * qy);
                    c.p[3] = Py + (cs.y * qx + cs.x * qy);
                }
            }
            sp.px = Px;
            sp.py = Py;
        } else if (c.kind == EGG_COLLIDER_HALF_PLANE) {
            c.p[2] = c.p[2] + (c.p[0] * ox + c.p[1] * oy);
        } else {
            c.p[0] = c.p[0] + ox;
            c.p[1] = c.p[1] + oy;
            if (c.kind == EGG_COLLIDER_SEGMENT || c.kind == EGG_COLLIDER_WALL) {
                c.p[2] = c.p[2] + ox;
                c.p[3] = c.p[3] + oy;
            }
        }
    }
    h->collider_dirty |= h->spins_turn ? kDirtyList | kDirtySpins : kDirtyList;
}

// Collider bodies at the commit: the list, the motions and the spins as the integrator of the last sub-step left them on
// the device become the handle's, in place of advance_colliders.  No step is running: every path waits for its streams
// before it commits, and the integrator ran on one of them.
static void take_bodies(egg_handle *h) {
    const size_t n = h->colliders.size();
    h->motions.resize(n);
    h->spins.resize(n);
    hipError_t e = hipSetDevice(h->device);
    if (e == hipSuccess) e = hipMemcpy(h->colliders.data(), h->d_colliders.p, n * sizeof(egg_collider), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(h->motions.data(), h->d_motions.p, n * sizeof(egg_collider_motion), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(h->spins.data(), h->d_spins.p, n * sizeof(egg_collider_spin), hipMemcpyDeviceToHost);
    if (e != hipSuccess) (void)fail(h, EGG_ERR_DEVICE, "relaxed order: the collider bodies did not reach the host: %s", hipGetErrorString(e));
    else h->collider_dirty &= ~(kDirtyList | kDirtyMotions | kDirtySpins);  // (host and device hold the same records again)
    h->motions_move = h->spins_turn = false;
    for (size_t k = 0; k < n; ++k) {
        h->motions_move |= h->motions[k].vx != 0.0 || h->motions[k].vy != 0.0;
        h->spins_turn |= h->spins[k].omega != 0.0;
    }
}

// Collider contacts at the commit: the fires the step's launches of egg_rx_contacts_kernel have counted join the handle's
// counter.  No step is running, as for take_bodies.
static void take_contacts(egg_handle *h) {
    unsigned long long fires = 0ull;
    hipError_t e = hipSetDevice(h->device);
    if (e == hipSuccess) e = hipMemcpy(&fires, h->d_contact_solves.p, 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) (void)fail(h, EGG_ERR_DEVICE, "relaxed order: the collider contacts' counter did not reach the host: %s", hipGetErrorString(e));
    else h->contact_solves += (int64_t)fires;
}

// Collider loads at the commit: the step's sums, which both types' streams have added into, become the handle's.  No step
// is running: every path waits for its streams before it commits, so one blocking copy sees every addition.
static void take_loads(egg_handle *h, double sub_delta) {
    const size_t n = h->colliders.size();
    std::vector<unsigned long long> words(3 * n + 1, 0ull);
    hipError_t e = hipSetDevice(h->device);
    if (e == hipSuccess) e = hipMemcpy(words.data(), h->d_loads.p, words.size() * 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        (void)fail(h, EGG_ERR_DEVICE, "relaxed order: the collider loads did not reach the host: %s", hipGetErrorString(e));
        return;
    }
    h->load_sums.resize(3 * n);
    for (size_t k = 0; k < 3 * n; ++k) h->load_sums[k] = (int64_t)words[k];
    h->load_dropped = (int64_t)words[3 * n];
    h->load_sub_delta = sub_delta;
}

// the commit of a relaxed step whose end kernels have run: flip cur, statistics from the status words read back
void relaxed_commit(egg_handle *h, const RelaxedStep st[2], int S, int C, double ms) {
    for (int w = 0; w < 2; ++w) {
        System &s = h->sys[w];
        h->stats.kernel_launches += st[w].launches;
        h->stats.budget[w] = st[w].env.budget;
        h->stats.max_pass_visits[w] = 0;
        if (!h->opt_timing || s.n == 0) h->stats.kernel_ms[w] = 0;
        if (s.n == 0) continue;
        s.cur ^= 1;
        int64_t most = 0;
        for (int p = 0; p < S * C; ++p) {
            const int64_t v = (int64_t)s.rx.h_status.p[1 + p];
            h->stats.pair_solves += v;
            most = std::max(most, v);
        }
        h->stats.max_pass_visits[w] = most;
        if (st[w].L.cohesion) h->stats.cohesion_solves += (int64_t)s.rx.h_status.p[st[w].L.cohered()];
        if (st[w].L.colliders) h->collider_hits[w] += (int64_t)s.rx.h_status.p[st[w].L.hits()];
        if (st[w].L.surfaces) h->collider_grips[w] += (int64_t)s.rx.h_status.p[st[w].L.grips()];
        if (st[w].L.V) h->viscosity_pairs[w] += (int64_t)s.rx.h_status.p[st[w].L.visc()];
        if (st[w].L.coupled_word) h->coupling_solves += (int64_t)s.rx.h_status.p[st[w].L.coupled()];
        if (st[w].L.adhered_word) h->adhesion_solves += (int64_t)s.rx.h_status.p[st[w].L.adhered()];
        if (st[w].L.contained_word) h->containment_hits += (int64_t)s.rx.h_status.p[st[w].L.contained()];
        h->stats.follow_solves += s.n * S;
        // the exact path's host copies of the atoms' cells describe older positions now
        s.aabb_valid = s.aabb_on_device = s.disp_valid = false;
        s.out_copied = false;
    }
    if (h->opt_loads && !h->colliders.empty()) take_loads(h, st[0].env.sub_delta);
    // the list at the start of this step, for the pose a frame draws (egg_get_collider_pose): taken before either of the two
    // ways a commit advances the list, whether or not anything moves -- what last_x / last_y are for the particles
    h->colliders_last = h->colliders;
    if (h->bodies_step) take_bodies(h);
    if (h->contacts_step) take_contacts(h);
    if ((h->motions_move || h->spins_turn) && !h->colliders.empty()) advance_colliders(h, (double)S * st[0].env.sub_delta, S);
    h->stats.last_step_kernel_ms = ms;
    if (h->opt_timing) {
        for (int w = 0; w < 2; ++w) h->stats.kernel_ms_sum[w] += h->stats.kernel_ms[w];
        h->stats.timed_steps++;
    }
    h->stats.steps++;
    h->stats.relaxed_steps++;
    h->bodies_step = h->contacts_step = false;
}

void leave_relaxed(egg_handle *h) {
    for (int w = 0; w < 2; ++w) {
        System &s = h->sys[w];
        s.tiling_dirty = true;
        s.aabb_valid = s.aabb_on_device = s.disp_valid = false;
        s.out_copied = false;
        s.meta_dirty = true;  // the relaxed steps took the target uploads over
    }
}

}  // namespace egghost
