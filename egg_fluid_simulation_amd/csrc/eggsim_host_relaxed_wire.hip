// eggsim_host_relaxed_wire.hip -- one relaxed-order _step of ONE handle, driven pass by pass
// through the C ABI (egg_rx_*, include/eggsim.h) by a host that carries the ghost halo between processes
// (egg_fluid_simulation_amd/sharding.py).  The step of each type is the driver of eggsim_host_relaxed.hip (RelaxedStep),
// cut into calls at every place where relaxed_group_step (eggsim_host_relaxed_group.hip) reads another handle's memory or
// waits for another handle's event.  What differs between the two:
//
//   group step                                          here
//   ev_box of the others, their status words            egg_rx_get_boxes -> the host's all-gather -> boxes of egg_rx_pack
//   egg_rx_pack_kernel into per-receiver buffers        egg_rx_wire_pack_kernel into messages, egg_rx_fetch copies them out
//   ev_pack, egg_rx_unpack_kernel from peer memory      egg_rx_run_pass: staging copy of the received messages,
//                                                       egg_rx_wire_unpack_kernel
//   status words of all handles, then the end kernels   egg_rx_check -> the host's all-reduce -> egg_rx_end(commit)
//
// With viscosity (egg_set_viscosity) the sequence has one more pass per sub-step, addressed as EGG_RX_VISCOSITY_PASS + sub
// after the sub-step's collision passes: the same calls, for the types whose coefficient is not zero (the other type reports
// an empty box, packs nothing and runs nothing); egg_rx_pack uses egg_rx_wire_pack_visc_kernel, whose records carry u.
//
// The pass kernels are the group instantiations, unchanged: entries = local particles + ghosts with keys.  Everything is
// enqueued on the handle's own streams; every call that hands data to the host waits for them first.
#include "eggsim_host.h"

namespace egghost {

struct WireStep {
    // global keys (egg_rx_set_keys): (batch key, base) ascending, the type's total over all ranks
    std::vector<std::pair<int64_t, int64_t>> keys[2];
    int64_t total[2] = {-1, -1};
    uint64_t keys_gen[2] = {1, 1};
    // the step in flight
    double delta = 0;
    int S = 0, C = 0;
    int sub_done = 0, pass_done = 0;  // sub-steps begun, passes run
    int visc_done = 0;                // viscosity passes run (one per sub-step while a type's coefficient is not zero)
    bool checked = false, bad = false;
    RelaxedStep st[2];
    // the last egg_rx_pack
    int packed_pass = -1, n_dest = 0;
    std::vector<int64_t> counts;  // [n_dest][2]
    size_t stride[2] = {0, 0};    // words of one message slot in wsend
};

namespace {

WireStep &wire_of(egg_handle *h) {
    if (!h->wire) h->wire = std::make_shared<WireStep>();
    return *h->wire;
}

int need_active(egg_handle *h, const char *name) {
    if (!h->wire_active) return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: no relaxed step in flight (egg_rx_begin first)", name);
    return EGG_OK;
}

// The step has viscosity passes: decided from the handle's coefficients, not from the layout of the types it holds, so
// that a handle without particles of a type (or of any) walks the same sequence as the ranks that have them.  (The
// coefficients cannot change while the step is in flight.)
bool any_viscosity(const egg_handle *h) { return h->viscosity[0] > 0.0 || h->viscosity[1] > 0.0; }

// the pass that runs next: a collision pass, or the viscosity pass of a sub-step whose collision passes have all run
int next_pass(const egg_handle *h, const WireStep &W) {
    if (any_viscosity(h) && W.visc_done < W.sub_done && W.pass_done == (W.visc_done + 1) * W.C)
        return EGG_RX_VISCOSITY_PASS + W.visc_done;
    return W.pass_done;
}

// pass `pass` is the next to run and its sub-step has begun
int need_pass(egg_handle *h, const WireStep &W, int pass, const char *name) {
    const int rc = need_active(h, name);
    if (rc != EGG_OK) return rc;
    if (pass >= EGG_RX_VISCOSITY_PASS && !any_viscosity(h))
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: pass %d addresses a viscosity pass, and both coefficients are 0", name, pass);
    if (pass != next_pass(h, W) || (pass < EGG_RX_VISCOSITY_PASS && pass >= W.sub_done * W.C))
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: pass %d is out of sequence (%d passes run, %d sub-steps begun, %d viscosity passes run)",
                    name, pass, W.pass_done, W.sub_done, W.visc_done);
    return EGG_OK;
}

// a pass of the ABI as the layout counts it: the viscosity pass of sub-step sub is halo pass P + sub
size_t halo_pass(const RelaxedStep &st, int pass) {
    return pass >= EGG_RX_VISCOSITY_PASS ? st.L.P + (size_t)(pass - EGG_RX_VISCOSITY_PASS) : (size_t)pass;
}

// type w takes part in `pass`: it has particles and, in a viscosity pass, a coefficient
bool in_pass(egg_handle *h, const WireStep &W, int w, int pass) {
    return h->sys[w].n > 0 && (pass < EGG_RX_VISCOSITY_PASS || h->viscosity[w] > 0.0);
}

int wait_both(egg_handle *h) {
    for (int w = 0; w < 2; ++w) HIP_TRY(h, wait_step(h->sys[w].stream));
    return EGG_OK;
}

}  // namespace
}  // namespace egghost

extern "C" {

int egg_rx_set_keys(egg_handle *h, int which, int64_t n, const int64_t *keys, const int64_t *bases, int64_t total) {
    if (!h || (which != EGG_WHITE && which != EGG_YOLK) || n < 0 || (n > 0 && (!keys || !bases)) || total < 0)
        return h ? fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_rx_set_keys: invalid arguments") : EGG_ERR_INVALID_ARGUMENT;
    REJECT_IN_FLIGHT(h, "egg_rx_set_keys");
    if (total > kRelaxedMaxParticles) return fail(h, EGG_ERR_UNSUPPORTED, EGG_RX_TOO_MANY_TEXT " over all ranks");
    std::vector<std::pair<int64_t, int64_t>> v((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        if (bases[i] < 0 || bases[i] > total) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_rx_set_keys: a base lies outside [0, total]");
        v[(size_t)i] = {keys[i], bases[i]};
    }
    std::sort(v.begin(), v.end());
    WireStep &W = wire_of(h);
    if (v != W.keys[which] || total != W.total[which]) {
        W.keys[which].swap(v);
        W.total[which] = total;
        ++W.keys_gen[which];
    }
    return EGG_OK;
}

int egg_rx_begin(egg_handle *h, double delta, int32_t n_substeps, int32_t n_collision_steps) {
    if (!h) return EGG_ERR_INVALID_ARGUMENT;
    if (n_substeps < 1 || n_collision_steps < 1 || std::isnan(delta)) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_rx_begin: invalid arguments");
    if (h->opt_solver_order != EGG_SOLVER_RELAXED) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_rx_begin: the handle is not in relaxed order");
    REJECT_IN_FLIGHT(h, "egg_rx_begin");
    if (h->coupling_factor > 0.0)  // (the halo carries no ghosts of the other type)
        return fail(h, EGG_ERR_UNSUPPORTED, "egg_rx_begin: white-yolk coupling runs on a single handle only (egg_set_coupling with factor 0 first)");
    if (h->adhesion_reach > 0.0)  // (a band in the coupling pass)
        return fail(h, EGG_ERR_UNSUPPORTED, "egg_rx_begin: white-yolk adhesion runs on a single handle only (egg_set_adhesion with reach 0 first)");
    if (h->bodies_any)
        return fail(h, EGG_ERR_UNSUPPORTED, "egg_rx_begin: collider bodies run on a single handle only (egg_set_collider_bodies with n = 0 first)");
    if (h->contacts_any)
        return fail(h, EGG_ERR_UNSUPPORTED, "egg_rx_begin: collider contacts run on a single handle only (egg_set_collider_contacts with n = 0 first)");
    (void)hipSetDevice(h->device);
    WireStep &W = wire_of(h);
    const int S = n_substeps, C = n_collision_steps;
    int rc = prepare_step(h, delta, S, W.st);
    if (rc != EGG_OK) return rc;
    for (int w = 0; w < 2; ++w) {
        System &s = h->sys[w];
        if (s.n == 0) continue;
        const int64_t total = W.total[w];
        if (total < s.n) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_rx_begin: the global keys of type %d are not set (egg_rx_set_keys)", w);
        const KeyBaseFn base_of = [&](int64_t key, int64_t count, int32_t *base) {
            auto it = std::lower_bound(W.keys[w].begin(), W.keys[w].end(), std::make_pair(key, (int64_t)-1));
            if (it == W.keys[w].end() || it->first != key || it->second + count > total)
                return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_rx_begin: no (valid) global key base for the batch with key %lld, type %d",
                            (long long)key, w);
            *base = (int32_t)it->second;
            return (int)EGG_OK;
        };
        rc = prepare_type(W.st[w], C, (size_t)(total - s.n), RelaxedLayout{(size_t)S * C, 0, true},
                          {~0ull, s.atoms_gen, W.keys_gen[w]}, base_of);
        if (rc != EGG_OK) return rc;
    }
    HIP_TRY(h, hipGetLastError());
    W.delta = delta;
    W.S = S;
    W.C = C;
    W.sub_done = W.pass_done = W.visc_done = 0;
    W.checked = W.bad = false;
    W.packed_pass = -1;
    W.n_dest = 0;
    h->wire_active = true;
    return EGG_OK;
}

int egg_rx_substep(egg_handle *h, int32_t sub) {
    if (!h) return EGG_ERR_INVALID_ARGUMENT;
    int rc = need_active(h, "egg_rx_substep");
    if (rc != EGG_OK) return rc;
    WireStep &W = *h->wire;
    if (sub != W.sub_done || sub >= W.S || W.pass_done != sub * W.C || (any_viscosity(h) && W.visc_done != sub))
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_rx_substep: sub-step %d is out of sequence (%d begun, %d passes run, %d viscosity passes run)",
                    (int)sub, W.sub_done, W.pass_done, W.visc_done);
    (void)hipSetDevice(h->device);
    for (int w = 0; w < 2; ++w) {
        if (h->sys[w].n == 0) continue;
        rc = launch_substep(W.st[w], sub);
        // containment is local to the handle (a batch lives wholly on one rank): white first, so that the sub-step's event
        // is recorded before the yolk stream waits for it; egg_rx_get_boxes reads the box behind the projection
        if (rc == EGG_OK && W.st[w].L.containment) rc = w == 0 ? launch_contain_sum(W.st[0], sub) : launch_contain(W.st[1], W.st[0], sub);
        if (rc != EGG_OK) return rc;
    }
    HIP_TRY(h, hipGetLastError());
    ++W.sub_done;
    return EGG_OK;
}

int egg_rx_get_boxes(egg_handle *h, int32_t pass, egg_rx_box boxes[2]) {
    if (!h || !boxes) return EGG_ERR_INVALID_ARGUMENT;
    int rc = need_active(h, "egg_rx_get_boxes");
    if (rc == EGG_OK) rc = need_pass(h, *h->wire, pass, "egg_rx_get_boxes");
    if (rc != EGG_OK) return rc;
    WireStep &W = *h->wire;
    (void)hipSetDevice(h->device);
    for (int w = 0; w < 2; ++w) {
        System &s = h->sys[w];
        if (!in_pass(h, W, w, pass)) continue;
        const size_t at = W.st[w].L.box(halo_pass(W.st[w], pass));
        HIP_TRY(h, hipMemcpyAsync(s.rx.h_status.p + at, s.rx.status.p + at, 4 * 8, hipMemcpyDeviceToHost, s.stream));
    }
    rc = wait_both(h);
    if (rc != EGG_OK) return rc;
    for (int w = 0; w < 2; ++w) {
        System &s = h->sys[w];
        egg_rx_box &b = boxes[w];
        b = egg_rx_box{0, 0, 0, 0, 1};
        if (!in_pass(h, W, w, pass)) continue;
        const unsigned long long *q = s.rx.h_status.p + W.st[w].L.box(halo_pass(W.st[w], pass));
        if (q[1] == 0) continue;  // (cannot happen with particles; the words say "empty")
        b.lo_x = (int32_t)((long long)((1ull << 32) - q[0]) - EGG_RX_BOX_BIAS);
        b.hi_x = (int32_t)((long long)q[1] - EGG_RX_BOX_BIAS);
        b.lo_y = (int32_t)((long long)((1ull << 32) - q[2]) - EGG_RX_BOX_BIAS);
        b.hi_y = (int32_t)((long long)q[3] - EGG_RX_BOX_BIAS);
        b.empty = 0;
    }
    return EGG_OK;
}

int egg_rx_pack(egg_handle *h, int32_t pass, int32_t n_dest, const egg_rx_box *boxes, int64_t *counts) {
    if (!h || n_dest < 0 || (n_dest > 0 && (!boxes || !counts))) return EGG_ERR_INVALID_ARGUMENT;
    int rc = need_active(h, "egg_rx_pack");
    if (rc == EGG_OK) rc = need_pass(h, *h->wire, pass, "egg_rx_pack");
    if (rc != EGG_OK) return rc;
    WireStep &W = *h->wire;
    (void)hipSetDevice(h->device);
    W.packed_pass = pass;
    W.n_dest = n_dest;
    W.counts.assign((size_t)n_dest * 2, 0);
    if (n_dest == 0) return EGG_OK;
    const size_t nd = (size_t)n_dest;
    for (int w = 0; w < 2; ++w) {
        System &s = h->sys[w];
        RelaxedBufs &r = s.rx;
        if (!in_pass(h, W, w, pass)) continue;
        const size_t stride = 1 + (size_t)EGG_RX_WIRE_RECORD_WORDS * (size_t)s.n;
        W.stride[w] = stride;
        HIP_TRY(h, r.wsend.reserve(nd * stride, false, s.stream));
        HIP_TRY(h, r.wbox.reserve(nd * EGG_RX_WIRE_BOX, false, s.stream));
        HIP_TRY(h, r.h_wbox.reserve(nd * EGG_RX_WIRE_BOX));
        HIP_TRY(h, r.h_wcount.reserve(nd));
        // (the previous pack's copies have completed: egg_rx_pack ends with a wait)
        for (size_t k = 0; k < nd; ++k) {
            const egg_rx_box &b = boxes[2 * k + (size_t)w];
            int32_t *q = r.h_wbox.p + k * EGG_RX_WIRE_BOX;
            q[0] = b.lo_x;
            q[1] = b.lo_y;
            q[2] = b.hi_x;
            q[3] = b.hi_y;
            q[4] = b.empty ? 1 : 0;
            HIP_TRY(h, hipMemsetAsync(r.wsend.p + k * stride, 0, 8, s.stream));  // the message's record count
        }
        HIP_TRY(h, hipMemcpyAsync(r.wbox.p, r.h_wbox.p, nd * EGG_RX_WIRE_BOX * 4, hipMemcpyHostToDevice, s.stream));
        EggRxWirePackArgs pk{};
        pk.n = (int)s.n;
        pk.cell_size = W.st[w].env.cell;
        pk.pos = W.st[w].A.a.pos;
        pk.inv_mass = s.inv_mass.p;
        pk.radius = s.radius.p;
        pk.ekey = r.ekey.p;
        if (W.st[w].L.cohesion) {
            pk.p_atom = r.p_atom.p;
            pk.atom_tag = W.st[w].A.c.atom_tag;
        }
        pk.stride = (long long)stride;
        for (size_t k0 = 0; k0 < nd; k0 += EGG_RX_MAX_GROUP) {
            pk.n_dest = (int)std::min<size_t>(EGG_RX_MAX_GROUP, nd - k0);
            pk.boxes = r.wbox.p + k0 * EGG_RX_WIRE_BOX;
            pk.msg = r.wsend.p + k0 * stride;
            if (pass >= EGG_RX_VISCOSITY_PASS)
                hipLaunchKernelGGL(egg_rx_wire_pack_visc_kernel, dim3((unsigned)((s.n + 255) / 256)), dim3(256), 0, s.stream,
                                   EggRxWirePackViscArgs{pk, W.st[w].A.a.prev});
            else
                hipLaunchKernelGGL(egg_rx_wire_pack_kernel, dim3((unsigned)((s.n + 255) / 256)), dim3(256), 0, s.stream, pk);
            ++W.st[w].launches;
        }
        HIP_TRY(h, hipGetLastError());
        for (size_t k = 0; k < nd; ++k)
            HIP_TRY(h, hipMemcpyAsync(r.h_wcount.p + k, r.wsend.p + k * stride, 8, hipMemcpyDeviceToHost, s.stream));
    }
    rc = wait_both(h);
    if (rc != EGG_OK) return rc;
    for (int w = 0; w < 2; ++w) {
        System &s = h->sys[w];
        if (!in_pass(h, W, w, pass)) continue;
        for (size_t k = 0; k < nd; ++k) {
            const int64_t c = (int64_t)s.rx.h_wcount.p[k];
            if (c < 0 || c > s.n) return fail(h, EGG_ERR_INTERNAL, "egg_rx_pack: a message holds %lld records of %lld particles", (long long)c, (long long)s.n);
            W.counts[2 * k + (size_t)w] = c;
        }
    }
    for (size_t i = 0; i < 2 * nd; ++i) counts[i] = W.counts[i];
    return EGG_OK;
}

int egg_rx_fetch(egg_handle *h, int32_t n_dest, void *const *out) {
    if (!h || n_dest < 0 || (n_dest > 0 && !out)) return EGG_ERR_INVALID_ARGUMENT;
    int rc = need_active(h, "egg_rx_fetch");
    if (rc != EGG_OK) return rc;
    WireStep &W = *h->wire;
    if (W.packed_pass != next_pass(h, W) || n_dest != W.n_dest)
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_rx_fetch: no egg_rx_pack of this pass for %d destinations", (int)n_dest);
    (void)hipSetDevice(h->device);
    for (int w = 0; w < 2; ++w) {
        System &s = h->sys[w];
        for (size_t k = 0; k < (size_t)n_dest; ++k) {
            void *dst = out[2 * k + (size_t)w];
            if (!dst) continue;
            const size_t words = 1 + (size_t)EGG_RX_WIRE_RECORD_WORDS * (size_t)W.counts[2 * k + (size_t)w];
            if (!in_pass(h, W, w, W.packed_pass)) {  // an empty message
                const unsigned long long zero = 0;
                HIP_TRY(h, hipMemcpy(dst, &zero, 8, hipMemcpyDefault));  // (dst may be device memory)
                continue;
            }
            HIP_TRY(h, hipMemcpyAsync(dst, s.rx.wsend.p + k * W.stride[w], words * 8, hipMemcpyDefault, s.stream));
        }
    }
    return wait_both(h);
}

int egg_rx_run_pass(egg_handle *h, int32_t pass, int32_t n_src, const void *const *msgs, const int64_t *counts) {
    if (!h || n_src < 0 || (n_src > 0 && (!msgs || !counts))) return EGG_ERR_INVALID_ARGUMENT;
    int rc = need_active(h, "egg_rx_run_pass");
    if (rc == EGG_OK) rc = need_pass(h, *h->wire, pass, "egg_rx_run_pass");
    if (rc != EGG_OK) return rc;
    WireStep &W = *h->wire;
    (void)hipSetDevice(h->device);
    // every message is checked before anything is enqueued
    const bool visc = pass >= EGG_RX_VISCOSITY_PASS;
    for (int w = 0; w < 2; ++w) {
        int64_t sum = 0;
        for (size_t k = 0; k < (size_t)n_src; ++k) {
            const int64_t cnt = counts[2 * k + (size_t)w];
            if (cnt < 0 || (cnt > 0 && !msgs[2 * k + (size_t)w])) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_rx_run_pass: invalid message %d", (int)k);
            sum += cnt;
        }
        if (sum > W.st[w].ghost_cap)
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_rx_run_pass: %lld ghost records of type %d, the other ranks hold %lld particles",
                        (long long)sum, w, (long long)W.st[w].ghost_cap);
    }
    for (int w = 0; w < 2; ++w) {
        System &s = h->sys[w];
        RelaxedBufs &r = s.rx;
        if (!in_pass(h, W, w, pass)) continue;
        // staging copies of the messages in this handle's memory, then the unpack (16 messages per launch)
        size_t words = 0;
        for (size_t k = 0; k < (size_t)n_src; ++k)
            if (counts[2 * k + (size_t)w] > 0) words += 1 + (size_t)EGG_RX_WIRE_RECORD_WORDS * (size_t)counts[2 * k + (size_t)w];
        if (words) {
            HIP_TRY(h, r.wrecv.reserve(words, false, s.stream));
            EggRxWireUnpackArgs up{};
            up.n = (int)s.n;
            up.cap_ghost = (int)W.st[w].ghost_cap;
            up.pos = W.st[w].A.a.pos;
            up.gwr = r.gwr.p;
            up.ekey = r.ekey.p;
            up.gtag = W.st[w].L.cohesion ? r.gtag.p : nullptr;
            up.n_ghost = r.status.p + W.st[w].L.ghosts(halo_pass(W.st[w], pass));
            int64_t most = 0;
            size_t off = 0;
            auto flush = [&]() {
                if (!up.n_src) return;
                hipLaunchKernelGGL(egg_rx_wire_unpack_kernel, dim3((unsigned)((most + 255) / 256), (unsigned)up.n_src), dim3(256), 0, s.stream, up);
                ++W.st[w].launches;
                up.n_src = 0;
                most = 0;
            };
            for (size_t k = 0; k < (size_t)n_src; ++k) {
                const int64_t cnt = counts[2 * k + (size_t)w];
                if (cnt <= 0) continue;
                const size_t mw = 1 + (size_t)EGG_RX_WIRE_RECORD_WORDS * (size_t)cnt;
                HIP_TRY(h, hipMemcpyAsync(r.wrecv.p + off, msgs[2 * k + (size_t)w], mw * 8, hipMemcpyDefault, s.stream));
                up.msg[up.n_src] = r.wrecv.p + off;
                up.cap[up.n_src] = (int32_t)cnt;
                ++up.n_src;
                most = std::max(most, cnt);
                off += mw;
                if (up.n_src == EGG_RX_MAX_GROUP) flush();
            }
            flush();
        }
        rc = visc ? launch_viscosity(W.st[w], pass - EGG_RX_VISCOSITY_PASS) : launch_pass(W.st[w], pass);
        if (rc != EGG_OK) return rc;
        HIP_TRY(h, hipGetLastError());
    }
    ++(visc ? W.visc_done : W.pass_done);
    return EGG_OK;
}

int egg_rx_check(egg_handle *h, int32_t *bad, int64_t pairs[2], int64_t *ghost_records) {
    if (!h || !bad) return EGG_ERR_INVALID_ARGUMENT;
    int rc = need_active(h, "egg_rx_check");
    if (rc != EGG_OK) return rc;
    WireStep &W = *h->wire;
    if (W.pass_done != W.S * W.C) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_rx_check: %d of %d passes have run", W.pass_done, W.S * W.C);
    if (any_viscosity(h) && W.visc_done != W.S)
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_rx_check: %d of %d viscosity passes have run", W.visc_done, W.S);
    (void)hipSetDevice(h->device);
    for (int w = 0; w < 2; ++w) {
        if (h->sys[w].n == 0) continue;
        rc = read_status(W.st[w]);
        if (rc != EGG_OK) return rc;
    }
    rc = wait_both(h);
    if (rc != EGG_OK) return rc;
    W.bad = false;
    int64_t records = 0;
    for (int w = 0; w < 2; ++w) {
        System &s = h->sys[w];
        if (pairs) pairs[w] = 0;
        if (s.n == 0) continue;
        W.bad |= bad_cell(W.st[w]);
        for (size_t p = 0; p < W.st[w].L.P; ++p)
            if (pairs) pairs[w] += (int64_t)s.rx.h_status.p[1 + p];
        for (size_t p = 0; p < W.st[w].L.H(); ++p) records += (int64_t)s.rx.h_status.p[W.st[w].L.ghosts(p)];
    }
    W.checked = true;
    *bad = W.bad ? 1 : 0;
    if (ghost_records) *ghost_records = records;
    return EGG_OK;
}

int egg_rx_end(egg_handle *h, int32_t commit) {
    if (!h) return EGG_ERR_INVALID_ARGUMENT;
    int rc = need_active(h, "egg_rx_end");
    if (rc != EGG_OK) return rc;
    WireStep &W = *h->wire;
    (void)hipSetDevice(h->device);
    if (commit && !W.checked) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_rx_end: commit without egg_rx_check");
    h->wire_active = false;
    if (!commit || W.bad) {  // nothing wrote [cur ^ 1]: wait for what was enqueued and forget it
        rc = wait_both(h);
        if (rc != EGG_OK) return rc;
        return commit ? fail(h, EGG_ERR_UNSUPPORTED, "%s", kRelaxedBadCellText) : EGG_OK;
    }
    for (int w = 0; w < 2; ++w) {
        if (h->sys[w].n == 0) continue;
        rc = launch_end(W.st[w]);
        if (rc != EGG_OK) return rc;
    }
    rc = wait_both(h);
    if (rc != EGG_OK) return rc;
    relaxed_commit(h, W.st, W.S, W.C, 0.0);
    return EGG_OK;
}

}  // extern "C"
