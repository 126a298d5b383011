// eggsim_host_relaxed_group.hip -- one relaxed-order _step over the handles of a device group
// (eggsim_group.cpp), with a per-pass ghost halo instead of hand-overs.  The results equal one relaxed handle holding
// every batch, bit for bit.  The step of each (handle, type) is the driver of eggsim_host_relaxed.hip (RelaxedStep);
// what is written here is what a group adds: the global keys, the events and the peer pack / unpack between passes.
//
// Per particle type and collision pass p, on every handle k that holds particles of the type:
//   * the kernel that wrote the positions of pass p (egg_rx_begin / mid, or the gather of pass p - 1) recorded their
//     cell box into k's status words; k records ev_box;
//   * every sender j waits for the ev_box of the others, packs its particles within one cell of each receiver's box
//     into its own send buffers (egg_rx_pack_kernel), records ev_pack;
//   * k waits for the ev_pack of the others, pulls their records for it into its ghost entries (egg_rx_unpack_kernel)
//     and runs insert .. gather over local particles + ghosts.  The gather writes local positions only.
// With viscosity (egg_set_viscosity) a type whose coefficient is not zero runs one more such exchange per sub-step, after
// its last collision pass: the box is the one that pass's gather recorded, the pack is egg_rx_pack_visc_kernel (the records
// carry u = pos - prev where a collision pass's carry inverse mass and radius), the unpack is the same and the pass is
// launch_viscosity.  The events alternate over the exchanges in the order they run.
// With containment (egg_set_containment) a handle that holds both types runs the two launches of the driver behind the
// begin / mid kernel of every sub-step; nothing travels between handles for it.
// Every event is recorded on the host before any wait on it is enqueued: streams of different handles may share a
// hardware queue, and a wait must never sit in a queue ahead of the work it waits for.  Pass p + 1's pack waits for
// the receiver's box of p + 1, which the receiver records after it has read pass p's records: a send buffer is never
// overwritten while it is being read.
//
// The step commits on every handle or on none: the status words of all handles come back after the passes (one host
// synchronise), and the end kernels that write [cur ^ 1] run only if no handle flagged a bad cell.
#include "eggsim_host.h"

namespace egghost {

namespace {

int group_too_large(int n, std::string *error) {
    if (n <= EGG_RX_MAX_GROUP) return EGG_OK;
    *error = "relaxed order: a device group of more than 16 handles";
    return EGG_ERR_UNSUPPORTED;
}

int device_fail(egg_handle *const *hs, int k, std::string *error, int rc) {
    char buf[64];
    snprintf(buf, sizeof buf, "device %d: ", k);
    *error = buf + hs[k]->error;
    return rc;
}

#define GK_TRY(k, expr)                                                                                            \
    do {                                                                                                           \
        const int _rc = (expr);                                                                                    \
        if (_rc != EGG_OK) return device_fail(hs, (k), error, _rc);                                                \
    } while (0)

#define GK_HIP(k, expr) GK_TRY(k, [&]() -> int { HIP_TRY(hs[k], (expr)); return EGG_OK; }())

}  // namespace

// The global key of a particle: its index in ONE handle holding every live batch of the group in
// ascending batch key.  The atoms of all handles, sorted by key, with the running sum of their particle counts.
void group_keys(egg_handle *const *hs, int n, int w, GroupKeys &K) {
    K.sizes.clear();
    for (int k = 0; k < n; ++k)
        for (const Atom &a : hs[k]->sys[w].atoms) K.sizes.emplace_back(hs[k]->batches[(size_t)a.batch].key, (int64_t)a.count);
    std::sort(K.sizes.begin(), K.sizes.end());
    K.base.resize(K.sizes.size());
    int64_t acc = 0;
    for (size_t b = 0; b < K.sizes.size(); ++b) {
        K.base[b] = acc;
        acc += K.sizes[b].second;
    }
    K.total = acc;
}

int64_t GroupKeys::base_of(int64_t key, int64_t count) const {
    const std::pair<int64_t, int64_t> e(key, count);
    return base[(size_t)(std::lower_bound(sizes.begin(), sizes.end(), e) - sizes.begin())];
}

int relaxed_group_peers(egg_handle *const *hs, int n, std::string *error) {
    if (group_too_large(n, error) != EGG_OK) return EGG_ERR_UNSUPPORTED;
    return group_peers(hs, n, "relaxed order", "the ghost halo", error);
}

// peer access between every pair of different devices of the group, both ways; `who` / `what` word the refusal
int group_peers(egg_handle *const *hs, int n, const char *who, const char *what, std::string *error) {
    for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b) {
            const int da = hs[a]->device, db = hs[b]->device;
            if (da == db) continue;  // handles on one device need nothing
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, da, db) != hipSuccess || !can) {
                char buf[160];
                snprintf(buf, sizeof buf, "%s: device %d cannot access device %d (peer access is needed for %s)", who, da, db, what);
                *error = buf;
                return EGG_ERR_UNSUPPORTED;
            }
            (void)hipSetDevice(da);
            const hipError_t e = hipDeviceEnablePeerAccess(db, 0);
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) {
                (void)hipGetLastError();
                char buf[160];
                snprintf(buf, sizeof buf, "%s: enabling peer access from device %d to %d failed: %s", who, da, db, hipGetErrorString(e));
                *error = buf;
                return EGG_ERR_UNSUPPORTED;
            }
            (void)hipGetLastError();  // (hipErrorPeerAccessAlreadyEnabled is sticky as the last error)
        }
    return EGG_OK;
}

int relaxed_group_step(egg_handle *const *hs, int nh, double delta, int S, int C, int64_t halo_records[1], std::string *error) {
    if (group_too_large(nh, error) != EGG_OK) return EGG_ERR_UNSUPPORTED;
    RelaxedStep st[EGG_RX_MAX_GROUP][2];
    for (int k = 1; k < nh; ++k)
        if (hs[k]->opt_cohesion != hs[0]->opt_cohesion) {  // (a ghost's batch tag travels only when its sender coheres)
            *error = "relaxed order: the handles of the group differ in EGG_OPT_COHESION (egg_group_set_cohesion sets all)";
            return EGG_ERR_INVALID_ARGUMENT;
        }
    for (int k = 1; k < nh; ++k) {
        const std::vector<egg_collider> &a = hs[0]->colliders, &b = hs[k]->colliders;
        if (a.size() != b.size() || (!a.empty() && memcmp(a.data(), b.data(), a.size() * sizeof(egg_collider)) != 0)) {
            *error = "relaxed order: the handles of the group differ in their colliders (egg_group_set_colliders sets all)";
            return EGG_ERR_INVALID_ARGUMENT;
        }
        const std::vector<egg_collider_surface> &sa = hs[0]->surfaces, &sb = hs[k]->surfaces;
        if (sa.size() != sb.size() || (!sa.empty() && memcmp(sa.data(), sb.data(), sa.size() * sizeof(egg_collider_surface)) != 0)) {
            *error = "relaxed order: the handles of the group differ in their collider surfaces (egg_group_set_collider_surfaces sets all)";
            return EGG_ERR_INVALID_ARGUMENT;
        }
        // (all zeros and none compare alike: neither moves anything)
        const std::vector<egg_collider_motion> &ma = hs[0]->motions, &mb = hs[k]->motions;
        const bool same_motion = hs[0]->motions_move == hs[k]->motions_move &&
                                 (!hs[0]->motions_move || memcmp(ma.data(), mb.data(), ma.size() * sizeof(egg_collider_motion)) == 0);
        if (!same_motion) {
            *error = "relaxed order: the handles of the group differ in their collider motion (egg_group_set_collider_motion sets all)";
            return EGG_ERR_INVALID_ARGUMENT;
        }
    }
    for (int k = 1; k < nh; ++k) {  // (all zeros and none compare alike: neither turns anything)
        const std::vector<egg_collider_spin> &a = hs[0]->spins, &b = hs[k]->spins;
        const bool same_spin = hs[0]->spins_turn == hs[k]->spins_turn &&
                               (!hs[0]->spins_turn || (a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(egg_collider_spin)) == 0));
        if (!same_spin) {
            *error = "relaxed order: the handles of the group differ in their collider spin (egg_group_set_collider_spin sets all)";
            return EGG_ERR_INVALID_ARGUMENT;
        }
    }
    for (int k = 0; k < nh; ++k) {  // (the loads would have to be summed across the handles every sub-step)
        if (hs[k]->bodies_any) {
            *error = "relaxed order: collider bodies run on a single handle only (egg_set_collider_bodies with n = 0 first)";
            return EGG_ERR_UNSUPPORTED;
        }
    }
    for (int k = 0; k < nh; ++k) {  // (a contact changes a body, and bodies run on one handle)
        if (hs[k]->contacts_any) {
            *error = "relaxed order: collider contacts run on a single handle only (egg_set_collider_contacts with n = 0 first)";
            return EGG_ERR_UNSUPPORTED;
        }
    }
    for (int k = 1; k < nh; ++k) {  // (with loads on the pivots count although nothing turns: the torque is about them)
        const std::vector<egg_collider_spin> &a = hs[0]->spins, &b = hs[k]->spins;
        const bool same_pivots = !hs[0]->opt_loads || hs[0]->spins_turn ||
                                 (a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(egg_collider_spin)) == 0));
        if (hs[0]->opt_loads != hs[k]->opt_loads || !same_pivots) {
            *error = "relaxed order: the handles of the group differ in their collider loads (egg_group_set_collider_loads sets all)";
            return EGG_ERR_INVALID_ARGUMENT;
        }
    }
    for (int k = 1; k < nh; ++k) {
        const std::vector<egg_force> &a = hs[0]->forces, &b = hs[k]->forces;
        if (a.size() != b.size() || (!a.empty() && memcmp(a.data(), b.data(), a.size() * sizeof(egg_force)) != 0)) {
            *error = "relaxed order: the handles of the group differ in their force fields (egg_group_set_forces sets all)";
            return EGG_ERR_INVALID_ARGUMENT;
        }
    }
    for (int k = 1; k < nh; ++k)
        if (memcmp(hs[0]->viscosity, hs[k]->viscosity, sizeof hs[0]->viscosity) != 0) {  // (a ghost's u travels only when its sender smooths)
            *error = "relaxed order: the handles of the group differ in their viscosity (egg_group_set_viscosity sets all)";
            return EGG_ERR_INVALID_ARGUMENT;
        }
    for (int k = 1; k < nh; ++k)
        if (hs[k]->containment_factor != hs[0]->containment_factor || hs[k]->containment_strength != hs[0]->containment_strength) {
            *error = "relaxed order: the handles of the group differ in their containment (egg_group_set_containment sets all)";
            return EGG_ERR_INVALID_ARGUMENT;
        }
    for (int k = 0; k < nh; ++k)
        if (hs[k]->coupling_factor > 0.0) {  // (the halo carries no ghosts of the other type)
            *error = "relaxed order: white-yolk coupling runs on a single handle only (egg_set_coupling with factor 0 first)";
            return EGG_ERR_UNSUPPORTED;
        }
    for (int k = 0; k < nh; ++k)
        if (hs[k]->adhesion_reach > 0.0) {  // (a band in the coupling pass, which a group does not run)
            *error = "relaxed order: white-yolk adhesion runs on a single handle only (egg_set_adhesion with reach 0 first)";
            return EGG_ERR_UNSUPPORTED;
        }
    for (int k = 0; k < nh; ++k) {
        (void)hipSetDevice(hs[k]->device);
        GK_TRY(k, prepare_step(hs[k], delta, S, st[k]));
    }
    const size_t P = (size_t)S * C;
    std::vector<int> q[2];
    for (int w = 0; w < 2; ++w) {
        int64_t total = 0;
        for (int k = 0; k < nh; ++k)
            if (hs[k]->sys[w].n > 0) {
                q[w].push_back(k);
                total += hs[k]->sys[w].n;
            }
        if (total > kRelaxedMaxParticles) {
            *error = EGG_RX_TOO_MANY_TEXT " in the group";
            return EGG_ERR_UNSUPPORTED;
        }
        if (q[w].empty()) continue;
        RelaxedLayout L{P, q[w].size(), true};
        L.V = hs[0]->viscosity[w] > 0.0 ? (size_t)S : 0;
        // global keys: a batch's particles start at the sum of the type's counts over the live batches of smaller id
        // (every handle lays its batches out in ascending id: the key of particle i is base + its place in its atom)
        std::vector<uint64_t> sig((size_t)nh);
        for (int k = 0; k < nh; ++k) sig[(size_t)k] = hs[k]->sys[w].atoms_gen;
        GroupKeys keys;
        bool any_rebuild = false;
        for (int k : q[w])
            any_rebuild |= hs[k]->sys[w].rx.key_sig != sig || hs[k]->sys[w].rx.ekey.cap < (size_t)total;
        if (any_rebuild) group_keys(hs, nh, w, keys);
        const KeyBaseFn base_of = [&keys](int64_t key, int64_t count, int32_t *base) {
            *base = (int32_t)keys.base_of(key, count);
            return (int)EGG_OK;
        };
        for (int k : q[w]) {
            System &s = hs[k]->sys[w];
            RelaxedBufs &r = s.rx;
            (void)hipSetDevice(hs[k]->device);
            GK_TRY(k, prepare_type(st[k][w], C, (size_t)(total - s.n), L, sig, base_of));
            GK_HIP(k, r.send.reserve(q[w].size() * (size_t)s.n, false, s.stream));
            for (hipEvent_t *e : {&r.ev_box[0], &r.ev_box[1], &r.ev_pack[0], &r.ev_pack[1]})
                if (!*e) GK_HIP(k, hipEventCreateWithFlags(e, hipEventDisableTiming));
        }
    }
    // the passes, one type after the other (the types are independent: their streams overlap)
    for (int w = 0; w < 2; ++w) {
        const std::vector<int> &Q = q[w];
        const size_t nq = Q.size();
        RelaxedLayout L{P, nq, true};
        L.V = nq && hs[0]->viscosity[w] > 0.0 ? (size_t)S : 0;
        size_t seq = 0;  // exchanges so far: the events alternate
        // the halo of halo pass p (a collision pass, or P + sub: the viscosity pass of sub-step sub) and the pass itself
        const auto halo_pass = [&](size_t p, bool visc, int sub) -> int {
            const int par = (int)(seq++ & 1);
            for (size_t m = 0; m < nq; ++m) {
                const int k = Q[m];
                (void)hipSetDevice(hs[k]->device);
                GK_HIP(k, hipEventRecord(hs[k]->sys[w].rx.ev_box[par], hs[k]->sys[w].stream));
            }
            for (size_t mj = 0; mj < nq && nq > 1; ++mj) {  // senders
                const int j = Q[mj];
                System &s = hs[j]->sys[w];
                (void)hipSetDevice(hs[j]->device);
                EggRxPackArgs pk{};
                pk.n = (int)s.n;
                pk.cell_size = st[j][w].env.cell;
                pk.pos = st[j][w].A.a.pos;
                pk.inv_mass = s.inv_mass.p;
                pk.radius = s.radius.p;
                pk.ekey = s.rx.ekey.p;
                if (st[j][w].L.cohesion) {
                    pk.p_atom = s.rx.p_atom.p;
                    pk.atom_tag = st[j][w].A.c.atom_tag;
                }
                for (size_t mk = 0; mk < nq; ++mk) {
                    if (mk == mj) continue;
                    const int k = Q[mk];
                    GK_HIP(j, hipStreamWaitEvent(s.stream, hs[k]->sys[w].rx.ev_box[par], 0));
                    pk.box[pk.n_recv] = hs[k]->sys[w].rx.status.p + L.box(p);
                    pk.send[pk.n_recv] = s.rx.send.p + mk * (size_t)s.n;
                    pk.count[pk.n_recv] = s.rx.status.p + L.sent(p, mk);
                    ++pk.n_recv;
                }
                if (visc)
                    hipLaunchKernelGGL(egg_rx_pack_visc_kernel, dim3((unsigned)((s.n + 255) / 256)), dim3(256), 0, s.stream,
                                       EggRxPackViscArgs{pk, st[j][w].A.a.prev});
                else
                    hipLaunchKernelGGL(egg_rx_pack_kernel, dim3((unsigned)((s.n + 255) / 256)), dim3(256), 0, s.stream, pk);
                ++st[j][w].launches;
                GK_HIP(j, hipEventRecord(s.rx.ev_pack[par], s.stream));
            }
            for (size_t mk = 0; mk < nq; ++mk) {  // receivers
                const int k = Q[mk];
                egg_handle *h = hs[k];
                System &s = h->sys[w];
                RelaxedBufs &r = s.rx;
                (void)hipSetDevice(h->device);
                if (nq > 1) {
                    EggRxUnpackArgs up{};
                    up.n = (int)s.n;
                    up.pos = st[k][w].A.a.pos;
                    up.gwr = r.gwr.p;
                    up.ekey = r.ekey.p;
                    up.gtag = st[k][w].L.cohesion ? r.gtag.p : nullptr;
                    up.n_ghost = r.status.p + L.ghosts(p);
                    int64_t most = 0;
                    for (size_t mj = 0; mj < nq; ++mj) {
                        if (mj == mk) continue;
                        System &sj = hs[Q[mj]]->sys[w];
                        GK_HIP(k, hipStreamWaitEvent(s.stream, sj.rx.ev_pack[par], 0));
                        up.recs[up.n_send] = sj.rx.send.p + mk * (size_t)sj.n;
                        up.count[up.n_send] = sj.rx.status.p + L.sent(p, mk);
                        ++up.n_send;
                        most = std::max(most, sj.n);
                    }
                    hipLaunchKernelGGL(egg_rx_unpack_kernel, dim3((unsigned)((most + 255) / 256), (unsigned)up.n_send), dim3(256), 0,
                                       s.stream, up);
                    ++st[k][w].launches;
                }
                if (visc)
                    GK_TRY(k, launch_viscosity(st[k][w], sub));
                else
                    GK_TRY(k, launch_pass(st[k][w], (int)p));
            }
            return EGG_OK;
        };
        for (int sub = 0; sub < S; ++sub) {
            for (size_t m = 0; m < nq; ++m) {
                (void)hipSetDevice(hs[Q[m]]->device);
                GK_TRY(Q[m], launch_substep(st[Q[m]][w], sub));
                // containment is local to a handle: a batch lives wholly on one.  The white type (w = 0) of every sub-step
                // has been enqueued, and its event recorded, before the yolk's is; ev_box is recorded behind the projection.
                RelaxedStep *t = st[Q[m]];
                if (t[w].L.containment) GK_TRY(Q[m], w == 0 ? launch_contain_sum(t[0], sub) : launch_contain(t[1], t[0], sub));
            }
            for (int c = 0; c < C; ++c) {
                const int rc = halo_pass((size_t)sub * C + c, false, sub);
                if (rc != EGG_OK) return rc;
            }
            if (L.V) {
                const int rc = halo_pass(P + (size_t)sub, true, sub);
                if (rc != EGG_OK) return rc;
            }
        }
    }
    // all handles or none: the status words (bad cells, pair counts, ghost counts) of every handle, then the end kernels
    for (int w = 0; w < 2; ++w)
        for (int k : q[w]) {
            (void)hipSetDevice(hs[k]->device);
            GK_TRY(k, read_status(st[k][w]));
        }
    bool bad = false;
    for (int w = 0; w < 2; ++w)
        for (int k : q[w]) {
            (void)hipSetDevice(hs[k]->device);
            GK_HIP(k, wait_step(hs[k]->sys[w].stream));
            bad |= bad_cell(st[k][w]);
        }
    if (bad) {  // nothing is committed anywhere: every [cur] and [cur ^ 1] is as before the step
        *error = kRelaxedBadCellText;
        return EGG_ERR_UNSUPPORTED;
    }
    int64_t records = 0;
    for (int w = 0; w < 2; ++w)
        for (int k : q[w]) {
            (void)hipSetDevice(hs[k]->device);
            GK_TRY(k, launch_end(st[k][w]));
            for (size_t p = 0; p < st[k][w].L.H(); ++p) records += (int64_t)hs[k]->sys[w].rx.h_status.p[st[k][w].L.ghosts(p)];
        }
    for (int w = 0; w < 2; ++w)
        for (int k : q[w]) {
            (void)hipSetDevice(hs[k]->device);
            GK_HIP(k, wait_step(hs[k]->sys[w].stream));
        }
    for (int k = 0; k < nh; ++k) relaxed_commit(hs[k], st[k], S, C, 0.0);
    halo_records[0] += records;
    return EGG_OK;
}

}  // namespace egghost
