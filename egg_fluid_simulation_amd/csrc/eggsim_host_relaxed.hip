// eggsim_host_relaxed.hip -- SimulationHandler:_step (simulation_handler.lua:1722-1989) in relaxed order
// (EGG_OPT_SOLVER_ORDER = 1): the launches of eggsim_relaxed.hip.  No tiles, claims or re-runs:
// every collision pass is a Jacobi pass over a cell table built fresh from the pass's positions.  The double-buffer
// contract is the exact path's: the step reads x / y / vx / vy[cur], writes the end-of-step state into [cur ^ 1], and
// the commit flips cur.  See eggsim_host.h.
#include <hipcub/hipcub.hpp>

#include "eggsim_host.h"

namespace egghost {

// buffers of one type for n particles and `ghosts` ghost entries (device groups); the cell table has at least
// 2 (n + ghosts) slots (a probe always finds a free one); `words` status words (0: the single handle's 1 + S C)
int reserve_relaxed(egg_handle *h, System &s, int S, int C, size_t ghosts, size_t words) {
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
    if (!words) words = 1 + (size_t)S * C;
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

// the kernels' arguments for one type's step (the group fields null: a single handle)
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

namespace {

// every launch of one type's step on its stream
int launch_relaxed(egg_handle *h, int w, const Env &env, int S, int C, int *launches) {
    System &s = h->sys[w];
    RelaxedBufs &r = s.rx;
    const int n = (int)s.n;
    EggRelaxedArgs A = relaxed_args(h, w, env);
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    int k = 0;
    HIP_TRY(h, hipMemsetAsync(r.status.p, 0, (1 + (size_t)S * C) * 8, s.stream));
    for (int sub = 0; sub < S; ++sub) {
        hipLaunchKernelGGL(sub == 0 ? egg_rx_begin_kernel : egg_rx_mid_kernel, grid, block, 0, s.stream, A);
        ++k;
        for (int c = 0; c < C; ++c) {
            A.pass = sub * C + c;
            HIP_TRY(h, hipMemsetAsync(r.hkey.p, 0xFF, (size_t)r.table * 8, s.stream));
            HIP_TRY(h, hipMemsetAsync(r.hcount.p, 0, ((size_t)r.table + 1) * 4, s.stream));
            hipLaunchKernelGGL(egg_rx_insert_kernel, grid, block, 0, s.stream, A);
            size_t bytes = r.scan_bytes;
            HIP_TRY(h, hipcub::DeviceScan::ExclusiveSum(r.scan_tmp.p, bytes, r.hcount.p, r.hstart.p, (int)r.table + 1, s.stream));
            hipLaunchKernelGGL(egg_rx_scatter_kernel, grid, block, 0, s.stream, A);
            hipLaunchKernelGGL(egg_rx_rank_kernel, grid, block, 0, s.stream, A);
            hipLaunchKernelGGL(egg_rx_gather_kernel, grid, block, 0, s.stream, A);
            k += 5;
            std::swap(A.pos, A.pos_next);  // Jacobi: the next pass starts from this one's result
        }
    }
    hipLaunchKernelGGL(egg_rx_end_kernel, grid, block, 0, s.stream, A);
    ++k;
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(r.h_status.p, r.status.p, (1 + (size_t)S * C) * 8, hipMemcpyDeviceToHost, s.stream));
    *launches += k;
    return EGG_OK;
}

}  // namespace

int relaxed_step(egg_handle *h, double delta, int S, int C) {  // L:1722-1989, collision passes relaxed
    const double sub_delta = std::max(delta / S, h->sys[0].cfg.eps);
    Env env[2];
    for (int w = 0; w < 2; ++w) {
        System &s = h->sys[w];
        env[w] = make_env(s.cfg, sub_delta, h->budget_particles[w] >= 0 ? h->budget_particles[w] : s.n);
        int rc = follow_config(h, w, true);
        if (rc != EGG_OK) return rc;
        rc = upload_atoms(h, w);
        if (rc != EGG_OK) return rc;
    }
    int launches = 0;
    for (int w = 0; w < 2; ++w) {
        System &s = h->sys[w];
        if (s.n == 0) continue;
        if (s.n > (int64_t)(1 << 29)) return fail(h, EGG_ERR_UNSUPPORTED, "relaxed order: more than 2^29 particles of one type");
        int rc = reserve_relaxed(h, s, S, C, 0, 0);
        if (rc == EGG_OK) rc = upload_relaxed_targets(h, s);
        if (rc != EGG_OK) return rc;
        if (h->opt_timing) HIP_TRY(h, hipEventRecord(s.ev0, s.stream));
        rc = launch_relaxed(h, w, env[w], S, C, &launches);
        if (rc != EGG_OK) return rc;
        if (h->opt_timing) HIP_TRY(h, hipEventRecord(s.ev1, s.stream));
    }
    h->stats.kernel_launches += launches;
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
        bad |= s.rx.h_status.p[0] != 0;
    }
    if (bad)  // nothing is committed: [cur] still holds the state before the step
        return fail(h, EGG_ERR_UNSUPPORTED, "relaxed order: a position is NaN or its spatial-hash cell lies outside +-2^30");
    relaxed_commit(h, env, S, C, ms);
    return EGG_OK;
}

// the commit of a relaxed step whose end kernels have run: flip cur, statistics from the status words read back
void relaxed_commit(egg_handle *h, const Env env[2], int S, int C, double ms) {
    for (int w = 0; w < 2; ++w) {
        System &s = h->sys[w];
        h->stats.budget[w] = env[w].budget;
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
        h->stats.follow_solves += s.n * S;
        // the exact path's host copies of the atoms' cells describe older positions now
        s.aabb_valid = s.aabb_on_device = s.disp_valid = false;
        s.out_copied = false;
    }
    h->stats.last_step_kernel_ms = ms;
    if (h->opt_timing) {
        for (int w = 0; w < 2; ++w) h->stats.kernel_ms_sum[w] += h->stats.kernel_ms[w];
        h->stats.timed_steps++;
    }
    h->stats.steps++;
    h->stats.relaxed_steps++;
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
