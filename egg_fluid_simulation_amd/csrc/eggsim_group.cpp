// eggsim_group.cpp -- several GPUs behind the C ABI: egg_group_* (include/eggsim.h).
//
// A LuaJIT / C host is ONE process, so its multi-GPU form is one process driving one egg_handle per device.  This
// file is a pure client of the single-device entry points (egg_create .. egg_step_begin / egg_step_end,
// egg_get_claims_many, egg_export_batch / egg_import_batch): the same protocol egg_fluid_simulation_amd/sharding.py runs
// between processes, without the messages.
//
//   * the plane is cut into x-slabs, one per device; a batch lives on the device whose slab holds its target when it
//     is added; ids are global, every handle lays its particles out in ascending global id (egg_add_many_keyed), so
//     results equal one handle holding everything, bit for bit;
//   * _step: every device launches its step (egg_step_begin fixes the claims of the step), the host then tests the
//     claims of batches on DIFFERENT devices against each other while the kernels run.  Claims of two batches closer
//     than one spatial-hash cell (simulation_handler.lua:1568-1578: what can interact) on different devices = the
//     sequential Gauss-Seidel order of the reference would cross devices: every device discards the launched step
//     (double-buffered state: free), the ISLANDS of such batches move to the lowest device involved
//     (egg_export_batch -> egg_import_batch), and the step is run again;
//   * an island that has left its slab's halo without meeting anything moves to the slab it is in after the step;
//   * the collision budget 0.05 N^2 (L:1752-1753) counts the particles of all devices (EGG_OPT_BUDGET_PARTICLES_*);
//     the visits of the step in flight are added up over the devices BEFORE it is committed; when the budget could
//     bind, the step is discarded and every batch goes to device 0, which steps them as one handle does (exact-budget
//     mode needs all particles of a type in one tile) until batches are added or removed.
//
// In relaxed order (egg_group_set_solver_order) there are no claims, budget or re-runs: the step
// is eggsim_host_relaxed_group.hip's (every pass over local particles plus ghosts of the neighbours', no hand-over),
// and afterwards a batch whose position lies more than `halo` px outside its slab moves to the slab that holds it.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/eggsim.h"
#include "eggsim_cover_merge.h"
#include "eggsim_group_draw.h"

namespace egghost {  // eggsim_host_relaxed_group.hip
int relaxed_group_peers(egg_handle *const *hs, int n, std::string *error);
int relaxed_group_step(egg_handle *const *hs, int n, double delta, int S, int C, int64_t halo_records[1], std::string *error);
}

namespace {
constexpr int64_t kGhostRecordBytes = 40;  // EggGhost (eggsim_device.h): x, y, inverse mass, radius, global key
}

struct egg_group {
    std::vector<egg_handle *> h;
    std::vector<double> cuts;  // n + 1 ascending x positions; slab k = [cuts[k], cuts[k + 1])
    double halo = 64.0;
    struct Rec {
        int owner = -1;
        int64_t local = 0;  // id inside the owning handle
        bool alive = false;
    };
    std::vector<Rec> batch;  // index = global id - 1
    bool budget_stale = true;
    bool consolidated = false;  // exact order: the budget may bind, device 0 holds and steps every batch (group_step_consolidated)
    double elapsed = 0, alpha = 0;
    int64_t migrations = 0, discarded_steps = 0;
    int64_t committed_visits[2] = {0, 0};
    int order = EGG_SOLVER_EXACT;
    int cohesion = EGG_COHESION_REFERENCE;  // egg_group_set_cohesion: every handle's EGG_OPT_COHESION
    std::vector<egg_collider> colliders;    // egg_group_set_colliders: every handle's list, as given
    std::vector<egg_collider_surface> surfaces;  // egg_group_set_collider_surfaces: every handle's records, as given
    std::vector<egg_collider_motion> motions;    // egg_group_set_collider_motion: every handle's records, as given
    std::vector<egg_collider_spin> spins;        // egg_group_set_collider_spin: every handle's records, as given
    std::vector<egg_collider_style> styles;      // egg_group_set_collider_styles: every handle's records, as given
    std::vector<egg_sensor> sensors;             // egg_group_set_sensors: every handle's list, as given
    std::vector<egg_force> forces;          // egg_group_set_forces: every handle's list, as given
    double viscosity[2] = {0.0, 0.0};       // egg_group_set_viscosity: every handle's coefficients
    double containment[2] = {0.0, 1.0};     // egg_group_set_containment: every handle's (factor, strength)
    int64_t halo_passes = 0, halo_records = 0;  // relaxed group steps: collision passes, ghost records received
    int64_t steps = 0;  // _step calls committed by the group
    // render attributes (never read by the solver): they live here, per global id / per type, so that a hand-over
    // between handles cannot lose them.  pcolor: [id - 1][type][rgba], the colour the batch's particles carry
    // (L:978-990, L:1110-1129); own_color: [id - 1][type], the batch's colour table is its own (a colour argument of
    // add) and not the config's (L:49-50)
    egg_render_config render_cfg[2];
    int use_particle_color = 0, use_lighting = 1;  // L:448-449
    std::vector<float> pcolor;
    std::vector<unsigned char> own_color;
    egghost::GroupDraw *draw = nullptr;  // device side of draws, created by the first one
    // counts the successful calls that can change a particle's colour or the group's particle count
    // (egg_group_get_instances); hand-overs change neither
    uint64_t color_version = 1;
    std::string error;
};

namespace {

int gfail(egg_group *g, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (g) g->error = buf;
    return code;
}

#define GTRY(g, k, expr)                                                                                          \
    do {                                                                                                          \
        const int _rc = (expr);                                                                                   \
        if (_rc < 0) return gfail(g, _rc, "device %d: %s", (int)(k), egg_last_error((g)->h[(size_t)(k)]));       \
    } while (0)

// A list every handle holds alike, set on all of them: set(h, n, records) on every handle, then `stored`, the group's
// copy, takes the new records.  A handle that refuses (handle 0 refuses bad records before any handle has changed; a later
// one is a handle somebody drives by hand) fails the group with its text: the handles before it go back to `stored`, and
// to whatever else `also` puts back on a handle, and `stored` stays as it was.
template <class R>
int set_on_every_handle(egg_group *g, int (*set)(egg_handle *, int32_t, const R *), int32_t n, const R *records, std::vector<R> &stored,
                        void (*also)(const egg_group *, egg_handle *) = nullptr) {
    for (size_t k = 0; k < g->h.size(); ++k) {
        const int rc = set(g->h[k], n, records);
        if (rc < 0) {
            for (size_t j = 0; j < k; ++j) {
                (void)set(g->h[j], (int32_t)stored.size(), stored.data());
                if (also) also(g, g->h[j]);
            }
            return gfail(g, rc, "device %d: %s", (int)k, egg_last_error(g->h[k]));
        }
    }
    stored.assign(records, records + (n > 0 ? n : 0));
    return EGG_OK;
}

int slab_of(const egg_group *g, double x) {
    int k = 0;
    const int n = (int)g->h.size();
    while (k + 1 < n && x >= g->cuts[(size_t)k + 1]) ++k;
    return k;
}

struct Claim {
    int64_t gid;
    int owner;
    double box[8];  // white lo_x lo_y hi_x hi_y, yolk ...
};

// the claims of every live batch for the step being prepared / in flight, per owner
int gather_claims(egg_group *g, std::vector<Claim> &out, double cell[2]) {
    out.clear();
    cell[0] = cell[1] = 0;
    const int n = (int)g->h.size();
    std::vector<std::vector<int64_t>> gids((size_t)n), lids((size_t)n);
    for (size_t i = 0; i < g->batch.size(); ++i)
        if (g->batch[i].alive) {
            gids[(size_t)g->batch[i].owner].push_back((int64_t)i + 1);
            lids[(size_t)g->batch[i].owner].push_back(g->batch[i].local);
        }
    for (int k = 0; k < n; ++k) {
        const size_t m = lids[(size_t)k].size();
        if (!m) continue;
        std::vector<double> boxes(8 * m);
        double cs[2] = {0, 0};
        GTRY(g, k, egg_get_claims_many(g->h[(size_t)k], (int64_t)m, lids[(size_t)k].data(), boxes.data(), cs));
        cell[0] = std::max(cell[0], cs[0]);
        cell[1] = std::max(cell[1], cs[1]);
        for (size_t j = 0; j < m; ++j) {
            Claim c;
            c.gid = gids[(size_t)k][j];
            c.owner = k;
            memcpy(c.box, &boxes[8 * j], sizeof c.box);
            out.push_back(c);
        }
    }
    return EGG_OK;
}

bool near(const Claim &a, const Claim &b, const double cell[2]) {
    for (int t = 0; t < 2; ++t) {
        const double *p = a.box + 4 * t, *q = b.box + 4 * t, c = cell[t];
        if (p[0] - q[2] < c && q[0] - p[2] < c && p[1] - q[3] < c && q[1] - p[3] < c) return true;
    }
    return false;
}

// Islands = batches chained by claims less than a cell apart, over ALL devices (sweep over the claims' low x).
// plan[gid] = the device an island must move to: the lowest device of an island that spans several, or -- for an island
// on one device that lies wholly outside that slab's halo -- the slab its middle is in.  conflicts: islands spanning devices.
int plan_moves(egg_group *g, const std::vector<Claim> &cl, const double cell[2], std::map<int64_t, int> &plan, int &conflicts) {
    plan.clear();
    conflicts = 0;
    const size_t n = cl.size();
    std::vector<size_t> order(n), parent(n);
    std::iota(order.begin(), order.end(), (size_t)0);
    std::iota(parent.begin(), parent.end(), (size_t)0);
    auto lo = [&](size_t i) { return std::min(cl[i].box[0], cl[i].box[4]); };
    auto hi = [&](size_t i) { return std::max(cl[i].box[2], cl[i].box[6]); };
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return lo(a) < lo(b); });
    auto find = [&](size_t v) {
        while (parent[v] != v) v = parent[v] = parent[parent[v]];
        return v;
    };
    const double reach = std::max(cell[0], cell[1]);
    for (size_t i = 0; i < n; ++i)
        for (size_t j = i + 1; j < n; ++j) {
            const size_t a = order[i], b = order[j];
            if (lo(b) - hi(a) >= reach) break;  // (sorted by low x: nothing further right can touch a -- boxes of similar width)
            if (near(cl[a], cl[b], cell)) {
                const size_t ra = find(a), rb = find(b);
                if (ra != rb) parent[std::max(ra, rb)] = std::min(ra, rb);
            }
        }
    // (the early exit above assumes no box hides a much wider one to its left: make up for it with the widest box)
    double widest = 0;
    for (size_t i = 0; i < n; ++i) widest = std::max(widest, hi(i) - lo(i));
    for (size_t i = 0; i < n; ++i)
        for (size_t j = i + 1; j < n; ++j) {
            const size_t a = order[i], b = order[j];
            if (lo(b) - lo(a) >= widest + reach) break;
            if (find(a) != find(b) && near(cl[a], cl[b], cell)) {
                const size_t ra = find(a), rb = find(b);
                parent[std::max(ra, rb)] = std::min(ra, rb);
            }
        }
    std::map<size_t, std::vector<size_t>> members;
    for (size_t i = 0; i < n; ++i) members[find(i)].push_back(i);
    const int nd = (int)g->h.size();
    for (auto &kv : members) {
        const std::vector<size_t> &m = kv.second;
        int lowest = nd, highest = -1;
        double x0 = std::numeric_limits<double>::infinity(), x1 = -x0;
        for (size_t i : m) {
            lowest = std::min(lowest, cl[i].owner);
            highest = std::max(highest, cl[i].owner);
            x0 = std::min(x0, lo(i));
            x1 = std::max(x1, hi(i));
        }
        int dest = -1;
        if (lowest != highest) {
            dest = lowest;
            ++conflicts;
        } else if ((lowest > 0 && x1 < g->cuts[(size_t)lowest] - g->halo) || (lowest + 1 < nd && x0 > g->cuts[(size_t)lowest + 1] + g->halo)) {
            dest = slab_of(g, 0.5 * (x0 + x1));
        }
        if (dest >= 0)
            for (size_t i : m)
                if (cl[i].owner != dest) plan[cl[i].gid] = dest;
    }
    return EGG_OK;
}

int move_batches(egg_group *g, const std::map<int64_t, int> &plan) {
    for (const auto &kv : plan) {
        egg_group::Rec &r = g->batch[(size_t)kv.first - 1];
        const int from = r.owner, to = kv.second;
        int64_t nw = 0, ny = 0;
        GTRY(g, from, egg_get_n_particles(g->h[(size_t)from], r.local, &nw, &ny));
        std::vector<double> ws(9 * (size_t)nw), ys(9 * (size_t)ny);
        egg_batch_info info;
        GTRY(g, from, egg_export_batch(g->h[(size_t)from], r.local, &info, ws.data(), ys.data()));
        int64_t lid = 0;
        GTRY(g, to, egg_import_batch(g->h[(size_t)to], &info, ws.data(), ys.data(), &lid));
        GTRY(g, from, egg_remove(g->h[(size_t)from], r.local));
        r.owner = to;
        r.local = lid;
        g->migrations++;
    }
    return EGG_OK;
}

int sync_budget(egg_group *g) {
    if (!g->budget_stale) return EGG_OK;
    int64_t tw = 0, ty = 0;
    for (size_t k = 0; k < g->h.size(); ++k) {
        int64_t nw = 0, ny = 0;
        GTRY(g, k, egg_get_n_particles(g->h[k], -1, &nw, &ny));
        tw += nw;
        ty += ny;
    }
    for (size_t k = 0; k < g->h.size(); ++k) {
        GTRY(g, k, egg_set_option(g->h[k], EGG_OPT_BUDGET_PARTICLES_WHITE, (double)tw));
        GTRY(g, k, egg_set_option(g->h[k], EGG_OPT_BUDGET_PARTICLES_YOLK, (double)ty));
    }
    g->budget_stale = false;
    return EGG_OK;
}

// hands islands over until no island spans devices (tiles and claims of the step re-formed every round)
int rebalance(egg_group *g, double delta, int S, int C) {
    for (int round = 0; round < 2 * (int)g->h.size() + 4; ++round) {
        for (size_t k = 0; k < g->h.size(); ++k) GTRY(g, k, egg_prepare_step(g->h[k], delta, S, C));
        std::vector<Claim> cl;
        double cell[2];
        int rc = gather_claims(g, cl, cell);
        if (rc != EGG_OK) return rc;
        std::map<int64_t, int> plan;
        int conflicts = 0;
        plan_moves(g, cl, cell, plan, conflicts);
        if (plan.empty()) return EGG_OK;
        rc = move_batches(g, plan);
        if (rc != EGG_OK) return rc;
    }
    return gfail(g, EGG_ERR_INTERNAL, "egg_group: batch hand-over did not settle");
}

// relaxed order: after a committed step, batches whose position lies more than `halo` px outside their slab move to the
// slab that holds it (where they sit does not change the results: the halo makes every device see what one would)
int rebalance_relaxed(egg_group *g) {
    const int n = (int)g->h.size();
    std::vector<std::vector<int64_t>> gids((size_t)n), lids((size_t)n);
    for (size_t i = 0; i < g->batch.size(); ++i)
        if (g->batch[i].alive) {
            gids[(size_t)g->batch[i].owner].push_back((int64_t)i + 1);
            lids[(size_t)g->batch[i].owner].push_back(g->batch[i].local);
        }
    std::map<int64_t, int> plan;
    for (int k = 0; k < n; ++k) {
        const size_t m = lids[(size_t)k].size();
        if (!m) continue;
        std::vector<double> xs(m), ys(m);
        GTRY(g, k, egg_get_positions_many(g->h[(size_t)k], (int64_t)m, lids[(size_t)k].data(), xs.data(), ys.data()));
        for (size_t j = 0; j < m; ++j) {
            const double x = xs[j];
            if (x < g->cuts[(size_t)k] - g->halo || x >= g->cuts[(size_t)k + 1] + g->halo) {
                const int dest = slab_of(g, x);
                if (dest != k) plan[gids[(size_t)k][j]] = dest;
            }
        }
    }
    return plan.empty() ? EGG_OK : move_batches(g, plan);
}

int group_step_relaxed(egg_group *g, double delta, int S, int C) {
    const size_t n = g->h.size();
    if (n == 1) {
        GTRY(g, 0, egg_step(g->h[0], delta, S, C));
        return EGG_OK;
    }
    std::string err;
    const int rc = egghost::relaxed_group_step(g->h.data(), (int)n, delta, S, C, &g->halo_records, &err);
    if (rc != EGG_OK) return gfail(g, rc, "%s", err.c_str());
    g->halo_passes += (int64_t)S * C + (g->viscosity[0] != 0.0 || g->viscosity[1] != 0.0 ? S : 0);  // (+ the viscosity passes)
    return rebalance_relaxed(g);
}

int group_step_any(egg_group *g, double delta, int S, int C);

int group_step(egg_group *g, double delta, int S, int C) {  // one _step (L:1722) on every device
    const int rc = group_step_any(g, delta, S, C);
    if (rc == EGG_OK) g->steps++;
    return rc;
}

// A collision budget 0.05 N^2 (L:1752-1753) that may bind (few batches: the yolk's does for nine or fewer) cuts passes
// short, and where it cuts depends on every visit before it: device 0 takes every batch and steps them as the single handle
// it then is; the other handles step empty.  Nothing strays back while the membership stays the same.
int group_step_consolidated(egg_group *g, double delta, int S, int C) {
    std::map<int64_t, int> plan;
    for (size_t i = 0; i < g->batch.size(); ++i)
        if (g->batch[i].alive && g->batch[i].owner != 0) plan[(int64_t)i + 1] = 0;
    int rc = plan.empty() ? EGG_OK : move_batches(g, plan);
    if (rc != EGG_OK) return rc;
    for (size_t k = 0; k < g->h.size(); ++k) GTRY(g, k, egg_step(g->h[k], delta, S, C));
    g->committed_visits[0] = g->committed_visits[1] = 0;
    return EGG_OK;
}

int group_step_any(egg_group *g, double delta, int S, int C) {
    if (g->order == EGG_SOLVER_RELAXED) return group_step_relaxed(g, delta, S, C);
    const size_t n = g->h.size();
    if (g->budget_stale) g->consolidated = false;  // batches came or went: the budget is another one
    int rc = sync_budget(g);
    if (rc != EGG_OK) return rc;
    if (g->consolidated && n > 1) return group_step_consolidated(g, delta, S, C);
    if (n == 1) {
        GTRY(g, 0, egg_step(g->h[0], delta, S, C));
        return EGG_OK;
    }
    for (size_t k = 0; k < n; ++k) GTRY(g, k, egg_step_begin(g->h[k], delta, S, C));
    auto discard = [&]() {
        for (size_t k = 0; k < n; ++k) (void)egg_step_end(g->h[k], 0);
    };
    std::vector<Claim> cl;
    double cell[2];
    rc = gather_claims(g, cl, cell);
    if (rc != EGG_OK) {
        discard();
        return rc;
    }
    std::map<int64_t, int> plan;
    int conflicts = 0;
    plan_moves(g, cl, cell, plan, conflicts);
    // the budget guard: what the step in flight visited, summed over the devices, against the global budget.
    // 1: the budget may bind (the step has been discarded); < 0: an error (discarded too)
    auto budget_trips = [&]() -> int {
        int64_t visits[2] = {g->committed_visits[0], g->committed_visits[1]};
        double budget[2] = {0, 0};
        int64_t sum[2] = {0, 0};
        for (size_t k = 0; k < n; ++k) {
            int64_t v[2] = {0, 0};
            double b[2] = {0, 0};
            const int prc = egg_step_peek_visits(g->h[k], v, b);
            if (prc < 0) {
                discard();
                return gfail(g, prc, "device %d: %s", (int)k, egg_last_error(g->h[k]));
            }
            for (int w = 0; w < 2; ++w) {
                sum[w] += v[w];
                budget[w] = std::max(budget[w], b[w]);
            }
        }
        for (int w = 0; w < 2; ++w)
            if ((double)std::max(visits[w], sum[w]) > std::max(1.0, std::ceil(budget[w]))) {
                // exact-budget mode needs all particles of the type in one tile, hence on one device
                discard();
                g->discarded_steps++;
                g->consolidated = true;
                return 1;
            }
        return 0;
    };
    int trips = budget_trips();
    if (trips < 0) return trips;
    if (trips) return group_step_consolidated(g, delta, S, C);
    auto note_committed = [&]() {
        g->committed_visits[0] = g->committed_visits[1] = 0;
        for (size_t k = 0; k < n; ++k) {
            egg_stats st;
            if (egg_get_stats(g->h[k], &st) == EGG_OK)
                for (int w = 0; w < 2; ++w) g->committed_visits[w] += st.max_pass_visits[w];
        }
    };
    if (conflicts == 0) {
        for (size_t k = 0; k < n; ++k) GTRY(g, k, egg_step_end(g->h[k], 1));
        note_committed();
        if (!plan.empty()) {  // strayed islands: handed to the slab they are in before the next step
            rc = rebalance(g, delta, S, C);
            if (rc != EGG_OK) return rc;
        }
        return EGG_OK;
    }
    discard();
    g->discarded_steps++;
    rc = rebalance(g, delta, S, C);
    if (rc != EGG_OK) return rc;
    for (size_t k = 0; k < n; ++k) GTRY(g, k, egg_step_begin(g->h[k], delta, S, C));
    trips = budget_trips();  // (islands that met on one device visit more pairs than they did apart)
    if (trips < 0) return trips;
    if (trips) return group_step_consolidated(g, delta, S, C);
    for (size_t k = 0; k < n; ++k) GTRY(g, k, egg_step_end(g->h[k], 1));
    note_committed();
    return EGG_OK;
}

bool group_alive(const egg_group *g, int64_t id) { return id >= 1 && id <= (int64_t)g->batch.size() && g->batch[(size_t)id - 1].alive; }

std::vector<int64_t> group_live_ids(const egg_group *g) {
    std::vector<int64_t> ids;
    for (size_t i = 0; i < g->batch.size(); ++i)
        if (g->batch[i].alive) ids.push_back((int64_t)i + 1);
    return ids;
}

// A batch is answered by the handle that owns it.  Per handle: the listed (live) ids it owns, one call(k, n, local ids, part)
// that fills recs_per_id records per id, and the records scattered into the caller's order.  A negative code of a call is the
// group's failure; `out` is written only after every handle has answered.
template <typename Rec, typename Call>
int route_to_owners(egg_group *g, int64_t n_ids, const int64_t *ids, size_t recs_per_id, Rec *out, Call call) {
    std::vector<Rec> all((size_t)n_ids * recs_per_id, Rec{});
    for (size_t k = 0; k < g->h.size(); ++k) {
        std::vector<int64_t> local, where;
        for (int64_t i = 0; i < n_ids; ++i) {
            const egg_group::Rec &r = g->batch[(size_t)ids[i] - 1];
            if (r.owner != (int)k) continue;
            local.push_back(r.local);
            where.push_back(i);
        }
        if (local.empty()) continue;
        std::vector<Rec> part(local.size() * recs_per_id, Rec{});
        const int rc = call(k, (int64_t)local.size(), local.data(), part.data());
        if (rc < 0) return gfail(g, rc, "device %d: %s", (int)k, egg_last_error(g->h[k]));
        for (size_t q = 0; q < local.size(); ++q)
            memcpy(&all[(size_t)where[q] * recs_per_id], &part[q * recs_per_id], recs_per_id * sizeof(Rec));
    }
    if (!all.empty()) memcpy(out, all.data(), all.size() * sizeof(Rec));
    return EGG_OK;
}

egghost::GroupView view_of(egg_group *g) {
    egghost::GroupView v;
    v.hs = g->h.data();
    v.n = (int)g->h.size();
    v.cfg = g->render_cfg;
    v.use_particle_color = g->use_particle_color;
    v.use_lighting = g->use_lighting;
    v.pcolor = g->pcolor.data();
    v.n_ids = (int64_t)g->batch.size();
    v.stepped = g->steps > 0;
    v.alpha = g->alpha;
    if (!g->draw) g->draw = egghost::group_draw_create();
    return v;
}

int gdone(egg_group *g, int rc, const std::string &err) {
    if (rc != EGG_OK) g->error = err;
    return rc;
}

float clamp01(double v) { return (float)std::min(std::max(v, 0.0), 1.0); }

}  // namespace

extern "C" {

int egg_group_create(const egg_config *white, const egg_config *yolk, int32_t n_devices, const int32_t *devices,
                     const double *cuts, egg_group **out) {
    if (!white || !out || n_devices < 1 || !devices || (n_devices > 1 && !cuts)) return EGG_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    egg_group *g = new egg_group();
    for (int k = 0; k <= n_devices; ++k) g->cuts.push_back(cuts ? cuts[k] : (k == 0 ? -std::numeric_limits<double>::infinity() : std::numeric_limits<double>::infinity()));
    for (int k = 0; k < n_devices; ++k)
        if (!(g->cuts[(size_t)k] < g->cuts[(size_t)k + 1])) {
            delete g;
            return EGG_ERR_INVALID_ARGUMENT;
        }
    for (int k = 0; k < n_devices; ++k) {
        egg_handle *h = nullptr;
        const int rc = egg_create(white, yolk, devices[k], &h);
        if (rc != EGG_OK) {
            for (egg_handle *q : g->h) egg_destroy(q);
            delete g;
            return rc;  // (egg_last_error(NULL) holds the reason)
        }
        g->h.push_back(h);
    }
    for (int w = 0; w < 2; ++w) (void)egg_default_render_config(w, &g->render_cfg[w]);
    *out = g;
    return EGG_OK;
}

void egg_group_destroy(egg_group *g) {
    if (!g) return;
    if (g->draw) egghost::group_draw_destroy(g->draw);  // (before the render handle goes)
    for (egg_handle *h : g->h) egg_destroy(h);
    delete g;
}

const char *egg_group_last_error(const egg_group *g) { return g ? g->error.c_str() : egg_last_error(nullptr); }

int32_t egg_group_n_devices(const egg_group *g) { return g ? (int32_t)g->h.size() : 0; }

egg_handle *egg_group_handle(egg_group *g, int32_t k) { return (g && k >= 0 && k < (int32_t)g->h.size()) ? g->h[(size_t)k] : nullptr; }

int egg_group_set_halo(egg_group *g, double halo_px) {
    if (!g || !(halo_px >= 0)) return EGG_ERR_INVALID_ARGUMENT;
    g->halo = halo_px;
    return EGG_OK;
}

int egg_group_add(egg_group *g, double x, double y, double white_radius, double yolk_radius, int64_t white_n, int64_t yolk_n,
                  int64_t *out_id) {
    if (!g) return EGG_ERR_INVALID_ARGUMENT;
    const int64_t gid = (int64_t)g->batch.size() + 1;
    const int k = slab_of(g, x);
    int64_t lid = 0;
    const int rc = egg_add_many_keyed(g->h[(size_t)k], 1, &x, &y, white_radius, yolk_radius, white_n, yolk_n, &gid, &lid);
    if (rc < 0) return gfail(g, rc, "device %d: %s", k, egg_last_error(g->h[(size_t)k]));
    egg_group::Rec r;
    r.owner = k;
    r.local = lid;
    r.alive = true;
    g->batch.push_back(r);
    for (int w = 0; w < 2; ++w) {  // L:978-990: the batch colour (here: the config's) or plain white
        const float white[4] = {1, 1, 1, 1};
        const float *c = g->use_particle_color ? g->render_cfg[w].color : white;
        g->pcolor.insert(g->pcolor.end(), c, c + 4);
        g->own_color.push_back(0);
    }
    g->budget_stale = true;
    g->color_version++;
    if (out_id) *out_id = gid;
    if (rc > 0) g->error = egg_last_error(g->h[(size_t)k]);  // the "few particles" warning (L:114-120): the batch exists
    return rc;
}

int egg_group_remove(egg_group *g, int64_t id) {
    if (!g) return EGG_ERR_INVALID_ARGUMENT;
    if (!group_alive(g, id)) {
        gfail(g, EGG_WARN_UNKNOWN_ID, "egg_group_remove: no batch with id `%lld`", (long long)id);
        return EGG_WARN_UNKNOWN_ID;  // the reference warns and carries on (L:145)
    }
    egg_group::Rec &r = g->batch[(size_t)id - 1];
    GTRY(g, r.owner, egg_remove(g->h[(size_t)r.owner], r.local));
    r.alive = false;
    g->budget_stale = true;
    g->color_version++;
    return EGG_OK;
}

int egg_group_set_target(egg_group *g, int64_t id, double x, double y) {
    if (!g) return EGG_ERR_INVALID_ARGUMENT;
    if (!group_alive(g, id)) {
        gfail(g, EGG_WARN_UNKNOWN_ID, "egg_group_set_target: no batch with id `%lld`", (long long)id);
        return EGG_WARN_UNKNOWN_ID;  // L:259
    }
    const egg_group::Rec &r = g->batch[(size_t)id - 1];
    GTRY(g, r.owner, egg_set_target(g->h[(size_t)r.owner], r.local, x, y));
    return EGG_OK;
}

int egg_group_get_position(egg_group *g, int64_t id, double *x, double *y) {
    if (!g || !x || !y) return EGG_ERR_INVALID_ARGUMENT;
    if (!group_alive(g, id))
        return gfail(g, EGG_ERR_UNKNOWN_ID, "egg_group_get_position: no batch with id `%lld`", (long long)id);  // L:286
    const egg_group::Rec &r = g->batch[(size_t)id - 1];
    GTRY(g, r.owner, egg_get_position(g->h[(size_t)r.owner], r.local, x, y));
    return EGG_OK;
}

int egg_group_owner(const egg_group *g, int64_t id, int32_t *device_index, int64_t *local_id) {
    if (!g || !group_alive(g, id)) return EGG_ERR_UNKNOWN_ID;
    if (device_index) *device_index = g->batch[(size_t)id - 1].owner;
    if (local_id) *local_id = g->batch[(size_t)id - 1].local;
    return EGG_OK;
}

int egg_group_step(egg_group *g, double delta, int32_t n_substeps, int32_t n_collision_steps) {
    if (!g || n_substeps < 1 || n_collision_steps < 1) return EGG_ERR_INVALID_ARGUMENT;
    return group_step(g, delta, n_substeps, n_collision_steps);
}

int egg_group_update(egg_group *g, double delta, double step_delta, int32_t n_substeps, int32_t n_collision_steps,
                     int32_t *out_n_steps) {  // the reference's accumulator (L:199-216) around the group's _step
    if (!g) return EGG_ERR_INVALID_ARGUMENT;
    if (!(step_delta > 0) || n_substeps < 1 || n_collision_steps < 1 || std::isnan(delta))
        return gfail(g, EGG_ERR_INVALID_ARGUMENT, "egg_group_update: invalid delta / step_delta / n_substeps / n_collision_steps");
    g->elapsed = g->elapsed + delta;
    int n_steps = 0;
    const double max_n_steps = std::max(4.0, 4 * std::ceil((1.0 / 60.0) / step_delta));
    while (g->elapsed >= step_delta) {
        const int rc = group_step(g, step_delta, n_substeps, n_collision_steps);
        if (rc != EGG_OK) return rc;
        g->elapsed = g->elapsed - step_delta;
        n_steps += 1;
        if (n_steps > max_n_steps) {  // death-spiral guard, L:208-213
            g->elapsed = 0;
            break;
        }
    }
    g->alpha = std::min(std::max(g->elapsed / step_delta, 0.0), 1.0);
    if (out_n_steps) *out_n_steps = n_steps;
    return EGG_OK;
}

int egg_group_get_counters(const egg_group *g, int64_t *migrations, int64_t *discarded_steps) {
    if (!g) return EGG_ERR_INVALID_ARGUMENT;
    if (migrations) *migrations = g->migrations;
    if (discarded_steps) *discarded_steps = g->discarded_steps;
    return EGG_OK;
}

int egg_group_set_solver_order(egg_group *g, int32_t order, double relaxation) {
    if (!g) return EGG_ERR_INVALID_ARGUMENT;
    if (order != EGG_SOLVER_EXACT && order != EGG_SOLVER_RELAXED)
        return gfail(g, EGG_ERR_INVALID_ARGUMENT, "egg_group_set_solver_order: solver order must be 0 (exact) or 1 (relaxed)");
    if (std::isnan(relaxation) || relaxation > 2)
        return gfail(g, EGG_ERR_INVALID_ARGUMENT, "egg_group_set_solver_order: relaxation must be in (0, 2] (<= 0 keeps the current value)");
    if (order == EGG_SOLVER_EXACT && g->cohesion != EGG_COHESION_REFERENCE)
        return gfail(g, EGG_ERR_UNSUPPORTED, "egg_group_set_solver_order: exact order has no effective cohesion: switch cohesion off first (egg_group_set_cohesion)");
    if (order == EGG_SOLVER_EXACT && !g->colliders.empty())
        return gfail(g, EGG_ERR_UNSUPPORTED, "egg_group_set_solver_order: exact order has no colliders: clear the list first (egg_group_set_colliders with n = 0)");
    if (order == EGG_SOLVER_EXACT && !g->forces.empty())
        return gfail(g, EGG_ERR_UNSUPPORTED, "egg_group_set_solver_order: exact order has no force fields: clear the list first (egg_group_set_forces with n = 0)");
    if (order == EGG_SOLVER_EXACT && (g->viscosity[0] != 0.0 || g->viscosity[1] != 0.0))
        return gfail(g, EGG_ERR_UNSUPPORTED, "egg_group_set_solver_order: exact order has no viscosity: set both coefficients to 0 first (egg_group_set_viscosity)");
    if (order == EGG_SOLVER_EXACT && g->containment[0] > 0.0)
        return gfail(g, EGG_ERR_UNSUPPORTED, "egg_group_set_solver_order: exact order has no yolk containment: set the factor to 0 first (egg_group_set_containment)");
    if (order == EGG_SOLVER_RELAXED && g->h.size() > 1) {  // the ghost halo reads the other devices' memory
        std::string err;
        const int rc = egghost::relaxed_group_peers(g->h.data(), (int)g->h.size(), &err);
        if (rc != EGG_OK) return gfail(g, rc, "egg_group_set_solver_order: %s", err.c_str());
    }
    if (relaxation > 0)
        for (size_t k = 0; k < g->h.size(); ++k) GTRY(g, k, egg_set_option(g->h[k], EGG_OPT_RELAXATION, relaxation));
    // (back to exact: every handle leaves relaxed order and re-tiles; the exact protocol hands islands over again)
    for (size_t k = 0; k < g->h.size(); ++k) GTRY(g, k, egg_set_option(g->h[k], EGG_OPT_SOLVER_ORDER, (double)order));
    if (order != g->order) g->budget_stale = true;
    g->order = order;
    return EGG_OK;
}

int egg_group_set_cohesion(egg_group *g, int32_t mode) {
    if (!g) return EGG_ERR_INVALID_ARGUMENT;
    if (mode != EGG_COHESION_REFERENCE && mode != EGG_COHESION_EFFECTIVE)
        return gfail(g, EGG_ERR_INVALID_ARGUMENT, "egg_group_set_cohesion: cohesion must be 0 (as the reference) or 1 (effective)");
    if (mode == EGG_COHESION_EFFECTIVE && g->order != EGG_SOLVER_RELAXED)
        return gfail(g, EGG_ERR_UNSUPPORTED, "egg_group_set_cohesion: effective cohesion needs relaxed order (egg_group_set_solver_order first)");
    for (size_t k = 0; k < g->h.size(); ++k) {
        const int rc = egg_set_option(g->h[k], EGG_OPT_COHESION, (double)mode);
        if (rc < 0) {  // (a handle somebody drives by hand: a step in flight, another order) -- the others go back
            for (size_t j = 0; j < k; ++j) (void)egg_set_option(g->h[j], EGG_OPT_COHESION, (double)g->cohesion);
            return gfail(g, rc, "device %d: %s", (int)k, egg_last_error(g->h[k]));
        }
    }
    g->cohesion = mode;
    return EGG_OK;
}

int egg_group_set_colliders(egg_group *g, int32_t n, const egg_collider *c) {
    if (!g) return EGG_ERR_INVALID_ARGUMENT;
    if ((!g->motions.empty() || !g->spins.empty()) && !g->h.empty()) {  // (committed steps have moved the lists: what a refused call goes back to is the list now)
        int32_t have = 0;
        (void)egg_get_colliders(g->h[0], 0, nullptr, &have);
        g->colliders.resize((size_t)have);
        (void)egg_get_colliders(g->h[0], have, g->colliders.data(), &have);
        if (!g->spins.empty()) (void)egg_get_collider_spin(g->h[0], have, g->spins.data(), &have);  // (and the pivots)
    }
    const int rc = set_on_every_handle(g, egg_set_colliders, n, c, g->colliders, [](const egg_group *g, egg_handle *h) {
        // (a handle that goes back to the list gets back the records a list that is set resets)
        (void)egg_set_collider_surfaces(h, (int32_t)g->surfaces.size(), g->surfaces.data());
        (void)egg_set_collider_motion(h, (int32_t)g->motions.size(), g->motions.data());
        (void)egg_set_collider_spin(h, (int32_t)g->spins.size(), g->spins.data());
        (void)egg_set_collider_styles(h, (int32_t)g->styles.size(), g->styles.data());
    });
    if (rc < 0) return rc;
    g->surfaces.clear();  // (every handle has reset its own)
    g->styles.clear();
    g->motions.clear();
    g->spins.clear();
    return EGG_OK;
}

int egg_group_set_collider_surfaces(egg_group *g, int32_t n, const egg_collider_surface *s) {
    if (!g) return EGG_ERR_INVALID_ARGUMENT;
    return set_on_every_handle(g, egg_set_collider_surfaces, n, s, g->surfaces);
}

int egg_group_get_collider_surfaces(const egg_group *g, int32_t cap, egg_collider_surface *s, int32_t *n) {
    if (!g || g->h.empty()) return EGG_ERR_INVALID_ARGUMENT;
    return egg_get_collider_surfaces(g->h[0], cap, s, n);  // (as stored: every handle holds the same records)
}

int egg_group_set_collider_motion(egg_group *g, int32_t n, const egg_collider_motion *m) {
    if (!g) return EGG_ERR_INVALID_ARGUMENT;
    return set_on_every_handle(g, egg_set_collider_motion, n, m, g->motions);
}

int egg_group_get_collider_motion(const egg_group *g, int32_t cap, egg_collider_motion *m, int32_t *n) {
    if (!g || g->h.empty()) return EGG_ERR_INVALID_ARGUMENT;
    return egg_get_collider_motion(g->h[0], cap, m, n);  // (as stored: every handle holds the same records)
}

int egg_group_set_collider_spin(egg_group *g, int32_t n, const egg_collider_spin *s) {
    if (!g) return EGG_ERR_INVALID_ARGUMENT;
    if (!g->spins.empty() && !g->h.empty()) {  // (committed steps have moved the pivots: what a refused call goes back to is the records now)
        int32_t have = 0;
        (void)egg_get_collider_spin(g->h[0], (int32_t)g->spins.size(), g->spins.data(), &have);
    }
    return set_on_every_handle(g, egg_set_collider_spin, n, s, g->spins);
}

int egg_group_get_collider_spin(const egg_group *g, int32_t cap, egg_collider_spin *s, int32_t *n) {
    if (!g || g->h.empty()) return EGG_ERR_INVALID_ARGUMENT;
    return egg_get_collider_spin(g->h[0], cap, s, n);  // (as stored: every handle holds the same records)
}

int egg_group_set_collider_styles(egg_group *g, int32_t n, const egg_collider_style *s) {
    if (!g) return EGG_ERR_INVALID_ARGUMENT;
    return set_on_every_handle(g, egg_set_collider_styles, n, s, g->styles);
}

int egg_group_get_collider_styles(const egg_group *g, int32_t cap, egg_collider_style *s, int32_t *n) {
    if (!g || g->h.empty()) return EGG_ERR_INVALID_ARGUMENT;
    return egg_get_collider_styles(g->h[0], cap, s, n);  // (as stored: every handle holds the same records)
}

int egg_group_get_collider_pose(egg_group *g, double alpha, int32_t cap, egg_collider *c, int32_t *n) {
    if (!g || g->h.empty()) return EGG_ERR_INVALID_ARGUMENT;
    // (every handle holds and advances the same two lists; the group's alpha, not handle 0's, is what its draw uses)
    return egg_get_collider_pose(g->h[0], alpha != alpha ? g->alpha : alpha, cap, c, n);
}

int egg_group_set_collider_loads(egg_group *g, int on) {
    if (!g) return EGG_ERR_INVALID_ARGUMENT;
    int was = 0;
    if (!g->h.empty()) (void)egg_get_collider_loads_enabled(g->h[0], &was);
    for (size_t k = 0; k < g->h.size(); ++k) {
        const int rc = egg_set_collider_loads(g->h[k], on);
        if (rc < 0) {  // (a handle with a step in flight: the others go back)
            for (size_t j = 0; j < k; ++j) (void)egg_set_collider_loads(g->h[j], was);
            return gfail(g, rc, "device %d: %s", (int)k, egg_last_error(g->h[k]));
        }
    }
    return EGG_OK;
}

// the integer sums and the dropped counts added over the handles (two's complement: the sum of the handles' sums is the
// sum over all their contributions); every handle of a committed step holds the same sub-step
int egg_group_get_collider_load_sums(egg_group *g, int32_t cap, int64_t *sums, int64_t *dropped, double *sub_delta, int32_t *n) {
    if (!g || g->h.empty()) return EGG_ERR_INVALID_ARGUMENT;
    int32_t have = 0;
    (void)egg_get_collider_load_sums(g->h[0], 0, nullptr, nullptr, nullptr, &have);
    if (n) *n = have;
    std::vector<uint64_t> total(3 * (size_t)have, 0);
    std::vector<int64_t> one(3 * (size_t)have, 0);
    int64_t lost = 0;
    double hs = 0.0;
    for (size_t k = 0; k < g->h.size(); ++k) {
        int64_t d = 0;
        double s = 0.0;
        int32_t m = 0;
        const int rc = egg_get_collider_load_sums(g->h[k], have, one.data(), &d, &s, &m);
        if (rc < 0) return gfail(g, rc, "device %d: %s", (int)k, egg_last_error(g->h[k]));
        for (size_t q = 0; q < 3 * (size_t)std::min(have, m); ++q) total[q] += (uint64_t)one[q];
        lost += d;
        if (k == 0) hs = s;
    }
    for (size_t q = 0; sums && q < 3 * (size_t)std::min(cap, have); ++q) sums[q] = (int64_t)total[q];
    if (dropped) *dropped = lost;
    if (sub_delta) *sub_delta = hs;
    return EGG_OK;
}

int egg_group_get_collider_loads(egg_group *g, int32_t cap, egg_collider_load *out, int32_t *n) {
    if (!g || g->h.empty()) return EGG_ERR_INVALID_ARGUMENT;
    int32_t have = 0;
    (void)egg_get_collider_load_sums(g->h[0], 0, nullptr, nullptr, nullptr, &have);
    std::vector<int64_t> sums(3 * (size_t)have, 0);
    double hs = 0.0;
    const int rc = egg_group_get_collider_load_sums(g, have, sums.data(), nullptr, &hs, nullptr);
    if (rc < 0) return rc;
    if (n) *n = have;
    for (int32_t k = 0; out && k < std::min(cap, have); ++k) {  // (converted once, with egg_get_collider_loads' two divisions)
        const bool any = hs > 0.0;
        out[k].jx = any ? ((double)sums[(size_t)(3 * k)] / EGG_COLLIDER_LOAD_IMPULSE_SCALE) / hs : 0.0;
        out[k].jy = any ? ((double)sums[(size_t)(3 * k + 1)] / EGG_COLLIDER_LOAD_IMPULSE_SCALE) / hs : 0.0;
        out[k].torque = any ? ((double)sums[(size_t)(3 * k + 2)] / EGG_COLLIDER_LOAD_TORQUE_SCALE) / hs : 0.0;
    }
    return EGG_OK;
}

// Sensors (include/eggsim.h, "sensors"): every handle holds the same list and measures the particles it owns.
int egg_group_set_sensors(egg_group *g, int32_t n, const egg_sensor *sensors) {
    if (!g) return EGG_ERR_INVALID_ARGUMENT;
    return set_on_every_handle(g, egg_set_sensors, n, sensors, g->sensors);
}

int egg_group_get_sensors(const egg_group *g, int32_t cap, egg_sensor *out, int32_t *n) {
    if (!g || g->h.empty()) return EGG_ERR_INVALID_ARGUMENT;
    return egg_get_sensors(g->h[0], cap, out, n);  // (as stored: every handle holds the same list)
}

// the readings and the dropped pair added over the handles (two's complement: the sum of the handles' sums is the sum over
// all their particles)
int egg_group_read_sensors(egg_group *g, int32_t cap, egg_sensor_reading *readings, int64_t dropped[2], int32_t *n) {
    if (!g || g->h.empty()) return EGG_ERR_INVALID_ARGUMENT;
    int32_t have = 0;
    (void)egg_get_sensors(g->h[0], 0, nullptr, &have);
    std::vector<uint64_t> total(6 * (size_t)have, 0);
    std::vector<egg_sensor_reading> one((size_t)have);
    int64_t lost[2] = {0, 0};
    for (size_t k = 0; k < g->h.size(); ++k) {
        int64_t d[2] = {0, 0};
        int32_t m = 0;
        const int rc = egg_read_sensors(g->h[k], have, one.data(), d, &m);
        if (rc < 0) return gfail(g, rc, "device %d: %s", (int)k, egg_last_error(g->h[k]));
        for (size_t q = 0; q < (size_t)std::min(have, m); ++q)
            for (int w = 0; w < 2; ++w) {
                total[6 * q + 0 + (size_t)w] += (uint64_t)one[q].count[w];
                total[6 * q + 2 + (size_t)w] += (uint64_t)one[q].sx[w];
                total[6 * q + 4 + (size_t)w] += (uint64_t)one[q].sy[w];
            }
        lost[0] += d[0];
        lost[1] += d[1];
    }
    if (n) *n = have;
    for (size_t q = 0; readings && q < (size_t)std::min(std::max(cap, 0), have); ++q)
        for (int w = 0; w < 2; ++w) {
            readings[q].count[w] = (int64_t)total[6 * q + 0 + (size_t)w];
            readings[q].sx[w] = (int64_t)total[6 * q + 2 + (size_t)w];
            readings[q].sy[w] = (int64_t)total[6 * q + 4 + (size_t)w];
        }
    if (dropped) {
        dropped[0] = lost[0];
        dropped[1] = lost[1];
    }
    return EGG_OK;
}

// a batch is answered by the handle that owns it: one call per handle over the ids it holds, scattered into the caller's order
int egg_group_read_sensor_batches(egg_group *g, int64_t n_ids, const int64_t *ids, int32_t *counts) {
    if (!g || g->h.empty() || n_ids < 0 || (n_ids > 0 && !ids)) return EGG_ERR_INVALID_ARGUMENT;
    for (int64_t i = 0; i < n_ids; ++i)  // (before anything is written)
        if (!group_alive(g, ids[i])) return gfail(g, EGG_ERR_UNKNOWN_ID, "egg_group_read_sensor_batches: no batch with id `%lld`", (long long)ids[i]);
    int32_t have = 0;
    (void)egg_get_sensors(g->h[0], 0, nullptr, &have);
    if (n_ids == 0 || have == 0) return EGG_OK;
    if (!counts) return gfail(g, EGG_ERR_INVALID_ARGUMENT, "egg_group_read_sensor_batches: counts is NULL");
    return route_to_owners<int32_t>(g, n_ids, ids, 2 * (size_t)have, counts, [&](size_t k, int64_t n, const int64_t *local, int32_t *part) {
        return egg_read_sensor_batches(g->h[k], n, local, part);
    });
}

// Probes (include/eggsim.h, "probes"): every handle answers for the particles it owns; per (probe, type) the best of those
// winners by (score, key, index) is the winner one handle with every batch would name.  The group's id of a batch is the key
// it gave egg_add_many_keyed.  Nothing is written before every handle has answered.
int egg_group_probe(egg_group *g, int32_t n, const egg_probe_query *probes, egg_probe_hit *hits) {
    if (!g || g->h.empty()) return EGG_ERR_INVALID_ARGUMENT;
    const size_t words = n > 0 && n <= EGG_MAX_PROBES ? 2 * (size_t)n : 0;
    std::vector<egg_probe_hit> best(words), one(std::max<size_t>(words, 1));
    for (size_t k = 0; k < g->h.size(); ++k) {
        const int rc = egg_probe(g->h[k], n, probes, hits ? one.data() : nullptr);  // (handle 0 refuses a bad list)
        if (rc < 0) return gfail(g, rc, "device %d: %s", (int)k, egg_last_error(g->h[k]));
        for (size_t q = 0; q < words; ++q) {
            const egg_probe_hit &a = one[q], &b = best[q];
            if (!a.found) continue;
            if (!b.found || a.score < b.score ||
                (a.score == b.score && (a.key < b.key || (a.key == b.key && a.index < b.index))))
                best[q] = a;
        }
    }
    for (egg_probe_hit &b : best)
        if (b.found) b.id = b.key;
    if (words) memcpy(hits, best.data(), words * sizeof(egg_probe_hit));
    return EGG_OK;
}

// Fields (include/eggsim.h, "fields"): every handle bins the particles it owns into the same grid; the planes and the totals
// are added on the host (two's complement: the sum of the handles' sums is the sum over all their particles).  Handle 0
// refuses a bad grid; nothing is written before every handle has answered.
int egg_group_field(egg_group *g, const egg_field_spec *spec, const egg_field_planes *host_out, egg_field_totals *totals) {
    if (!g || g->h.empty()) return EGG_ERR_INVALID_ARGUMENT;
    const bool shaped = spec && spec->nx >= 1 && spec->ny >= 1 && (int64_t)spec->nx * spec->ny <= EGG_FIELD_MAX_CELLS;
    const size_t words = shaped && host_out ? 2 * (size_t)spec->nx * (size_t)spec->ny : 0;
    const bool velocity = host_out && host_out->svx && host_out->svy;
    std::vector<int32_t> count(words, 0), one_count(std::max<size_t>(words, 1));
    std::vector<uint64_t> svx(velocity ? words : 0, 0), svy(velocity ? words : 0, 0);
    std::vector<int64_t> one_svx(std::max<size_t>(svx.size(), 1)), one_svy(std::max<size_t>(svy.size(), 1));
    uint64_t sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t k = 0; k < g->h.size(); ++k) {
        egg_field_planes one{};
        if (host_out) {  // (a missing plane stays missing: the handle refuses what it refuses alone)
            one.count = host_out->count ? one_count.data() : nullptr;
            one.svx = host_out->svx ? one_svx.data() : nullptr;
            one.svy = host_out->svy ? one_svy.data() : nullptr;
        }
        egg_field_totals t{};
        const int rc = egg_field(g->h[k], spec, host_out ? &one : nullptr, &t);
        if (rc < 0) return gfail(g, rc, "device %d: %s", (int)k, egg_last_error(g->h[k]));
        for (size_t q = 0; q < words; ++q) count[q] = (int32_t)((uint32_t)count[q] + (uint32_t)one_count[q]);
        for (size_t q = 0; q < svx.size(); ++q) {
            svx[q] += (uint64_t)one_svx[q];
            svy[q] += (uint64_t)one_svy[q];
        }
        for (int w = 0; w < 2; ++w) {
            sum[0 + w] += (uint64_t)t.inside[w];
            sum[2 + w] += (uint64_t)t.outside[w];
            sum[4 + w] += (uint64_t)t.dropped[w];
        }
        sum[6] += (uint64_t)t.units_tiled;
        sum[7] += (uint64_t)t.units_direct;
    }
    memcpy(host_out->count, count.data(), words * sizeof(int32_t));
    if (velocity) {
        memcpy(host_out->svx, svx.data(), words * sizeof(int64_t));
        memcpy(host_out->svy, svy.data(), words * sizeof(int64_t));
    }
    if (totals) {
        for (int w = 0; w < 2; ++w) {
            totals->inside[w] = (int64_t)sum[0 + w];
            totals->outside[w] = (int64_t)sum[2 + w];
            totals->dropped[w] = (int64_t)sum[4 + w];
        }
        totals->units_tiled = (int32_t)sum[6];
        totals->units_direct = (int32_t)sum[7];
    }
    return EGG_OK;
}

// Pieces (include/eggsim.h, "pieces"): a batch lives wholly on one handle, so every id is routed to its owner and the owner's
// records are copied to the caller's rows.  Nothing is written before every handle has answered.
int egg_group_pieces(egg_group *g, const egg_pieces_spec *spec, int64_t n_ids, const int64_t *ids, egg_piece_summary *out) {
    if (!g || g->h.empty()) return EGG_ERR_INVALID_ARGUMENT;
    if (!spec) return gfail(g, EGG_ERR_INVALID_ARGUMENT, "egg_group_pieces: spec is NULL");
    if (!out) return gfail(g, EGG_ERR_INVALID_ARGUMENT, "egg_group_pieces: out is NULL");
    for (int w = 0; w < 2; ++w)  // (checked here as well: a group without a requested batch asks no handle)
        if (!std::isfinite(spec->reach[w]) || !(spec->reach[w] > 0.0))
            return gfail(g, EGG_ERR_INVALID_ARGUMENT, "egg_group_pieces: reach[%d] = %g: it is finite and above 0", w, spec->reach[w]);
    if (spec->type_mask < 1 || spec->type_mask > 3)
        return gfail(g, EGG_ERR_INVALID_ARGUMENT, "egg_group_pieces: type_mask %d (bit 0 white, bit 1 yolk, never 0)", (int)spec->type_mask);
    if (n_ids < 0 || (n_ids > 0 && !ids) || (n_ids == 0 && ids))
        return gfail(g, EGG_ERR_INVALID_ARGUMENT, "egg_group_pieces: n_ids = %lld %s a list (0 and NULL mean every live batch)", (long long)n_ids,
                     ids ? "with" : "without");
    for (int64_t i = 0; i < n_ids; ++i)  // (before anything is written)
        if (!group_alive(g, ids[i])) return gfail(g, EGG_ERR_UNKNOWN_ID, "egg_group_pieces: no batch with id `%lld`", (long long)ids[i]);
    std::vector<int64_t> every;
    if (n_ids == 0) {
        every = group_live_ids(g);
        ids = every.data();
        n_ids = (int64_t)every.size();
    }
    return route_to_owners<egg_piece_summary>(g, n_ids, ids, 2, out, [&](size_t k, int64_t n, const int64_t *local, egg_piece_summary *part) {
        return egg_pieces(g->h[k], spec, n, local, part, nullptr, nullptr);
    });
}

// Impulses (include/eggsim_impulse.h): every handle edits the particles it owns.  A record's id is the group's: the owner
// gets its local id, every other handle EGG_IMPULSE_NO_BATCH, so the record is inert there and keeps its place in the order.
// First every handle checks the list with every record inert, which launches nothing; only then does any handle change a
// particle.  The totals are integers: the handles' totals added are one handle's.
int egg_group_impulse(egg_group *g, int32_t n, const egg_impulse_record *list, egg_impulse_result *results) {
    if (!g || g->h.empty()) return EGG_ERR_INVALID_ARGUMENT;
    if (n < 0 || n > EGG_MAX_IMPULSES)
        return gfail(g, EGG_ERR_INVALID_ARGUMENT, "egg_group_impulse: n = %d, a call takes 0 .. %d records", (int)n, EGG_MAX_IMPULSES);
    if (n > 0 && !list) return gfail(g, EGG_ERR_INVALID_ARGUMENT, "egg_group_impulse: n = %d without a list", (int)n);
    std::vector<egg_impulse_record> local(list, list + n);
    for (egg_impulse_record &o : local)
        if (o.id != EGG_IMPULSE_ALL_BATCHES) o.id = EGG_IMPULSE_NO_BATCH;
    for (size_t k = 0; k < g->h.size(); ++k) {  // (the checks of every handle, before anything changes)
        std::vector<egg_impulse_record> inert(local);
        for (egg_impulse_record &o : inert) o.id = EGG_IMPULSE_NO_BATCH;
        const int rc = egg_impulse(g->h[k], n, inert.data(), nullptr);
        if (rc < 0) return gfail(g, rc, "device %d: %s", (int)k, egg_last_error(g->h[k]));
    }
    for (int32_t i = 0; i < n; ++i) {
        const int64_t id = list[i].id;
        if (id == EGG_IMPULSE_ALL_BATCHES || id == EGG_IMPULSE_NO_BATCH) continue;
        if (!group_alive(g, id))
            return gfail(g, EGG_ERR_UNKNOWN_ID, "egg_group_impulse: record %d: no batch with id `%lld`", (int)i, (long long)id);
    }
    std::vector<egg_impulse_result> sum((size_t)n, egg_impulse_result{}), one((size_t)std::max<int32_t>(n, 1));
    for (size_t k = 0; k < g->h.size(); ++k) {
        for (int32_t i = 0; i < n; ++i) {
            const int64_t id = list[i].id;
            if (id == EGG_IMPULSE_ALL_BATCHES || id == EGG_IMPULSE_NO_BATCH) continue;
            const egg_group::Rec &r = g->batch[(size_t)id - 1];
            local[(size_t)i].id = r.owner == (int)k ? r.local : EGG_IMPULSE_NO_BATCH;
        }
        const int rc = egg_impulse(g->h[k], n, local.data(), results ? one.data() : nullptr);
        if (rc < 0) return gfail(g, rc, "device %d: %s", (int)k, egg_last_error(g->h[k]));
        if (!results) continue;
        for (int32_t i = 0; i < n; ++i)
            for (int w = 0; w < 2; ++w) {
                sum[(size_t)i].count[w] += one[(size_t)i].count[w];
                sum[(size_t)i].sdvx[w] = (int64_t)((uint64_t)sum[(size_t)i].sdvx[w] + (uint64_t)one[(size_t)i].sdvx[w]);
                sum[(size_t)i].sdvy[w] = (int64_t)((uint64_t)sum[(size_t)i].sdvy[w] + (uint64_t)one[(size_t)i].sdvy[w]);
                sum[(size_t)i].skipped[w] += one[(size_t)i].skipped[w];
            }
    }
    if (results && n > 0) memcpy(results, sum.data(), (size_t)n * sizeof(egg_impulse_result));
    return EGG_OK;
}

// Measures (include/eggsim_measure.h): a batch lives wholly on one handle, so every id is routed to its owner and the
// owner's records are copied to the caller's rows.  First every handle checks the spec with an empty list, which launches
// nothing; nothing is written before every handle has answered.
int egg_group_measure(egg_group *g, const egg_measure_spec *spec, int64_t n_ids, const int64_t *ids, egg_measure_record *out) {
    if (!g || g->h.empty()) return EGG_ERR_INVALID_ARGUMENT;
    if (!spec) return gfail(g, EGG_ERR_INVALID_ARGUMENT, "egg_group_measure: spec is NULL");
    if (!out) return gfail(g, EGG_ERR_INVALID_ARGUMENT, "egg_group_measure: out is NULL");
    if (n_ids < 0 || (n_ids > 0 && !ids))
        return gfail(g, EGG_ERR_INVALID_ARGUMENT, "egg_group_measure: n_ids = %lld without a list (0 and NULL mean every live batch)", (long long)n_ids);
    for (size_t k = 0; k < g->h.size(); ++k) {  // (the checks of every handle: flags, mask, region, a step in flight)
        const int64_t none = 0;
        egg_measure_record unused;
        const int rc = egg_measure(g->h[k], spec, 0, &none, &unused);
        if (rc < 0) return gfail(g, rc, "device %d: %s", (int)k, egg_last_error(g->h[k]));
    }
    for (int64_t i = 0; i < n_ids; ++i)  // (before anything is written)
        if (!group_alive(g, ids[i])) return gfail(g, EGG_ERR_UNKNOWN_ID, "egg_group_measure: no batch with id `%lld`", (long long)ids[i]);
    std::vector<int64_t> every;
    if (n_ids == 0 && !ids) {
        every = group_live_ids(g);
        ids = every.data();
        n_ids = (int64_t)every.size();
    }
    return route_to_owners<egg_measure_record>(g, n_ids, ids, 2, out, [&](size_t k, int64_t n, const int64_t *local, egg_measure_record *part) {
        return egg_measure(g->h[k], spec, n, local, part);
    });
}

// Cover (include/eggsim_cover.h): every handle rasters the particles it owns into the same grid; eggsim_cover_merge.h adds
// the cover planes, merges the owner planes -- taken as keys: a batch's key on its handle is the group's id -- by unsigned
// minimum and recounts
// covered, covered_both and covered_any from the merged planes; the other totals are added.  Handle 0 refuses a bad grid;
// nothing is written before every handle has answered.
int egg_group_cover(egg_group *g, const egg_cover_spec *spec, const egg_cover_planes *host_planes, egg_cover_totals *totals) {
    if (!g || g->h.empty()) return EGG_ERR_INVALID_ARGUMENT;
    const bool shaped = spec && spec->nx >= 1 && spec->ny >= 1 && (int64_t)spec->nx * spec->ny <= EGG_COVER_MAX_CELLS;
    const size_t words = shaped && host_planes && host_planes->cover ? 2 * (size_t)spec->nx * (size_t)spec->ny : 0;
    const bool with_owner = host_planes && host_planes->owner;
    std::vector<int32_t> cover(words, 0), one_cover(std::max<size_t>(words, 1)), one_owner(with_owner ? std::max<size_t>(words, 1) : 0);
    std::vector<uint32_t> owner(with_owner ? words : 0, 0xFFFFFFFFu);
    egg_cover_totals sum{};
    egg_cover_spec keyed = spec ? *spec : egg_cover_spec{};
    keyed.path |= EGG_COVER_OWNER_KEYS;  // (a batch's key on its handle is the group's id)
    for (size_t k = 0; k < g->h.size(); ++k) {
        egg_cover_planes one{};
        if (host_planes) {  // (a missing plane stays missing: the handle refuses what it refuses alone)
            one.cover = host_planes->cover ? one_cover.data() : nullptr;
            one.owner = with_owner ? one_owner.data() : nullptr;
        }
        egg_cover_totals t{};
        const int rc = egg_cover(g->h[k], spec ? &keyed : nullptr, host_planes ? &one : nullptr, &t);
        if (rc < 0) return gfail(g, rc, "device %d: %s", (int)k, egg_last_error(g->h[k]));
        eggcover::merge_planes(words, cover.data(), with_owner ? owner.data() : nullptr, one_cover.data(), with_owner ? one_owner.data() : nullptr);
        for (int w = 0; w < 2; ++w) {
            sum.inside[w] += t.inside[w];
            sum.outside[w] += t.outside[w];
            sum.dropped[w] += t.dropped[w];
            sum.hits[w] += t.hits[w];
        }
        sum.units_lanes += t.units_lanes;
        sum.units_wave += t.units_wave;
        sum.units_direct += t.units_direct;
    }
    eggcover::recount(words / 2, cover.data(), sum.covered, &sum.covered_both, &sum.covered_any);
    memcpy(host_planes->cover, cover.data(), words * sizeof(int32_t));
    if (with_owner) memcpy(host_planes->owner, owner.data(), words * sizeof(int32_t));
    if (totals) *totals = sum;
    return EGG_OK;
}

// Touches (include/eggsim_touch.h): a query's batch lives wholly on one handle, its partners on any.  Per handle: the listed
// batches it owns go through egg_touches, the others through egg_touches_of with their discs -- x, y and radius of
// egg_export_batch, what a hand-over reads -- and their key; everything by keys, a batch's key on its handle being the
// group's id.  The records of one (slot, other) are added and sorted.  First every handle checks the spec with an empty list
// of queries, which launches nothing; nothing is written before every handle has answered.
int egg_group_touches(egg_group *g, const egg_touch_spec *spec, int64_t n_ids, const int64_t *ids, int64_t cap, egg_touch_record *out,
                      int64_t *n_out) {
    if (!g || g->h.empty()) return EGG_ERR_INVALID_ARGUMENT;
    if (!n_out) return gfail(g, EGG_ERR_INVALID_ARGUMENT, "egg_group_touches: n_out is NULL");
    if (cap < 0 || (cap > 0 && !out))
        return gfail(g, EGG_ERR_INVALID_ARGUMENT, "egg_group_touches: cap = %lld %s a buffer", (long long)cap, out ? "with" : "without");
    if (n_ids < 0 || (n_ids > 0 && !ids) || (n_ids == 0 && ids))
        return gfail(g, EGG_ERR_INVALID_ARGUMENT, "egg_group_touches: n_ids = %lld %s a list (0 and NULL mean every live batch)", (long long)n_ids,
                     ids ? "with" : "without");
    egg_touch_spec keyed = spec ? *spec : egg_touch_spec{};
    keyed.flags |= EGG_TOUCH_BY_KEYS;
    for (size_t k = 0; k < g->h.size(); ++k) {  // (the checks of every handle: the spec, a step in flight)
        int64_t none = 0;
        const int rc = egg_touches_of(g->h[k], spec ? &keyed : nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, &none);
        if (rc < 0) return gfail(g, rc, "device %d: %s", (int)k, egg_last_error(g->h[k]));
    }
    for (int64_t i = 0; i < n_ids; ++i)  // (before anything is written)
        if (!group_alive(g, ids[i])) return gfail(g, EGG_ERR_UNKNOWN_ID, "egg_group_touches: no batch with id `%lld`", (long long)ids[i]);
    std::vector<int64_t> every;
    if (n_ids == 0) {
        every = group_live_ids(g);
        ids = every.data();
        n_ids = (int64_t)every.size();
    }
    // the discs of every listed batch, read once from its owner: [type] x, y, r
    struct Discs {
        std::vector<double> x[2], y[2], r[2];
    };
    std::map<int64_t, Discs> discs;
    if (g->h.size() > 1)
        for (int64_t i = 0; i < n_ids; ++i) {
            if (discs.count(ids[i])) continue;
            const egg_group::Rec &rec = g->batch[(size_t)ids[i] - 1];
            int64_t n[2] = {0, 0};
            GTRY(g, rec.owner, egg_get_n_particles(g->h[(size_t)rec.owner], rec.local, &n[0], &n[1]));
            std::vector<double> state[2] = {std::vector<double>(9 * (size_t)n[0] + 1), std::vector<double>(9 * (size_t)n[1] + 1)};
            egg_batch_info info{};
            GTRY(g, rec.owner, egg_export_batch(g->h[(size_t)rec.owner], rec.local, &info, state[0].data(), state[1].data()));
            Discs &d = discs[ids[i]];
            for (int w = 0; w < 2; ++w) {  // (field-major: x, y, vx, vy, last_x, last_y, inv_mass, radius, mass_t)
                const size_t m = (size_t)n[w];
                d.x[w].assign(state[w].begin(), state[w].begin() + m);
                d.y[w].assign(state[w].begin() + m, state[w].begin() + 2 * m);
                d.r[w].assign(state[w].begin() + 7 * m, state[w].begin() + 8 * m);
            }
        }
    std::map<std::pair<int32_t, int64_t>, egg_touch_record> sum;
    std::vector<egg_touch_record> part(1024);
    for (size_t k = 0; k < g->h.size(); ++k) {
        std::vector<int64_t> local, where;            // the listed batches handle k owns, and their entries
        std::vector<egg_touch_query> queries;          // the others, one query per type
        std::vector<int64_t> q_where;
        std::vector<double> x, y, r;
        for (int64_t i = 0; i < n_ids; ++i) {
            const egg_group::Rec &rec = g->batch[(size_t)ids[i] - 1];
            if (rec.owner == (int)k) {
                local.push_back(rec.local);
                where.push_back(i);
                continue;
            }
            const Discs &d = discs[ids[i]];
            for (int w = 0; w < 2; ++w) {
                queries.push_back(egg_touch_query{ids[i], w, (int32_t)d.x[w].size()});
                q_where.push_back(i);
                x.insert(x.end(), d.x[w].begin(), d.x[w].end());
                y.insert(y.end(), d.y[w].begin(), d.y[w].end());
                r.insert(r.end(), d.r[w].begin(), d.r[w].end());
            }
        }
        for (int form = 0; form < 2; ++form) {
            if (form == 0 ? local.empty() : queries.empty()) continue;
            int64_t n = 0;
            int rc = 0;
            for (int attempt = 0; attempt < 2; ++attempt) {  // (a short buffer: once more with the size the call named)
                rc = form == 0 ? egg_touches(g->h[k], &keyed, (int64_t)local.size(), local.data(), (int64_t)part.size(), part.data(), &n)
                               : egg_touches_of(g->h[k], &keyed, (int64_t)queries.size(), queries.data(), x.data(), y.data(), r.data(),
                                                (int64_t)part.size(), part.data(), &n);
                if (rc >= 0 || n <= (int64_t)part.size()) break;
                part.resize((size_t)n);
            }
            if (rc < 0) return gfail(g, rc, "device %d: %s", (int)k, egg_last_error(g->h[k]));
            for (int64_t q = 0; q < n; ++q) {
                egg_touch_record p = part[(size_t)q];
                // the handle's slot is 2 j + w over ITS list: entry j of `local`, or query j of `queries` (whose type is w)
                const int w = p.slot & 1;
                const int64_t entry = form == 0 ? where[(size_t)(p.slot >> 1)] : q_where[(size_t)(p.slot >> 1)];
                p.slot = (int32_t)(2 * entry + w);
                auto at = sum.find({p.slot, p.other});
                if (at == sum.end()) {
                    sum.emplace(std::make_pair(p.slot, p.other), p);
                    continue;
                }
                egg_touch_record &o = at->second;
                if ((int64_t)o.pairs + p.pairs > (int64_t)std::numeric_limits<int32_t>::max())
                    return gfail(g, EGG_ERR_UNSUPPORTED, "egg_group_touches: the pairs of slot %d with batch %lld do not fit 31 bits", (int)p.slot,
                                 (long long)p.other);
                o.pairs += p.pairs;
                o.particles += p.particles;
                o.dropped += p.dropped;
                o.sx = (int64_t)((uint64_t)o.sx + (uint64_t)p.sx);
                o.sy = (int64_t)((uint64_t)o.sy + (uint64_t)p.sy);
            }
        }
    }
    *n_out = (int64_t)sum.size();
    if ((int64_t)sum.size() > cap)
        return gfail(g, EGG_ERR_INVALID_ARGUMENT, "egg_group_touches: the answer holds %lld records, the buffer %lld", (long long)sum.size(), (long long)cap);
    int64_t at = 0;
    for (const auto &kv : sum) out[at++] = kv.second;  // (the map's order: slot, then other)
    return EGG_OK;
}

int egg_group_get_collider_grips(egg_group *g, int64_t grips[2]) {
    if (!g) return EGG_ERR_INVALID_ARGUMENT;
    if (!grips) return gfail(g, EGG_ERR_INVALID_ARGUMENT, "egg_group_get_collider_grips: grips is NULL");
    grips[0] = grips[1] = 0;
    for (size_t k = 0; k < g->h.size(); ++k) {
        int64_t one[2] = {0, 0};
        GTRY(g, k, egg_get_collider_grips(g->h[k], one));
        grips[0] += one[0];
        grips[1] += one[1];
    }
    return EGG_OK;
}

int egg_group_get_colliders(const egg_group *g, int32_t cap, egg_collider *c, int32_t *n) {
    if (!g || g->h.empty()) return EGG_ERR_INVALID_ARGUMENT;
    return egg_get_colliders(g->h[0], cap, c, n);  // (as stored: every handle holds the same list)
}

int egg_group_get_collider_hits(egg_group *g, int64_t hits[2]) {
    if (!g) return EGG_ERR_INVALID_ARGUMENT;
    if (!hits) return gfail(g, EGG_ERR_INVALID_ARGUMENT, "egg_group_get_collider_hits: hits is NULL");
    hits[0] = hits[1] = 0;
    for (size_t k = 0; k < g->h.size(); ++k) {
        int64_t one[2] = {0, 0};
        GTRY(g, k, egg_get_collider_hits(g->h[k], one));
        hits[0] += one[0];
        hits[1] += one[1];
    }
    return EGG_OK;
}

int egg_group_set_forces(egg_group *g, int32_t n, const egg_force *f) {
    if (!g) return EGG_ERR_INVALID_ARGUMENT;
    return set_on_every_handle(g, egg_set_forces, n, f, g->forces);
}

int egg_group_get_forces(const egg_group *g, int32_t cap, egg_force *f, int32_t *n) {
    if (!g || g->h.empty()) return EGG_ERR_INVALID_ARGUMENT;
    return egg_get_forces(g->h[0], cap, f, n);  // (as stored: every handle holds the same list)
}

int egg_group_set_viscosity(egg_group *g, const double c[2]) {
    if (!g || g->h.empty()) return EGG_ERR_INVALID_ARGUMENT;
    for (size_t k = 0; k < g->h.size(); ++k) {
        const int rc = egg_set_viscosity(g->h[k], c);
        if (rc < 0) {  // (handle 0 refuses bad values before any handle has changed; a later one: the others go back)
            for (size_t j = 0; j < k; ++j) (void)egg_set_viscosity(g->h[j], g->viscosity);
            return gfail(g, rc, "device %d: %s", (int)k, egg_last_error(g->h[k]));
        }
    }
    return egg_get_viscosity(g->h[0], g->viscosity);  // (as stored)
}

int egg_group_get_viscosity(const egg_group *g, double c[2]) {
    if (!g || g->h.empty()) return EGG_ERR_INVALID_ARGUMENT;
    return egg_get_viscosity(g->h[0], c);  // (every handle holds the same coefficients)
}

int egg_group_get_viscosity_pairs(egg_group *g, int64_t pairs[2]) {
    if (!g) return EGG_ERR_INVALID_ARGUMENT;
    if (!pairs) return gfail(g, EGG_ERR_INVALID_ARGUMENT, "egg_group_get_viscosity_pairs: pairs is NULL");
    pairs[0] = pairs[1] = 0;
    for (size_t k = 0; k < g->h.size(); ++k) {
        int64_t one[2] = {0, 0};
        GTRY(g, k, egg_get_viscosity_pairs(g->h[k], one));
        pairs[0] += one[0];
        pairs[1] += one[1];
    }
    return EGG_OK;
}

int egg_group_set_containment(egg_group *g, double factor, double strength) {
    if (!g || g->h.empty()) return EGG_ERR_INVALID_ARGUMENT;
    for (size_t k = 0; k < g->h.size(); ++k) {
        const int rc = egg_set_containment(g->h[k], factor, strength);
        if (rc < 0) {  // (handle 0 refuses bad values before any handle has changed; a later one: the others go back)
            for (size_t j = 0; j < k; ++j) (void)egg_set_containment(g->h[j], g->containment[0], g->containment[1]);
            return gfail(g, rc, "device %d: %s", (int)k, egg_last_error(g->h[k]));
        }
    }
    return egg_get_containment(g->h[0], &g->containment[0], &g->containment[1]);  // (as stored)
}

int egg_group_get_containment(const egg_group *g, double *factor, double *strength) {
    if (!g || g->h.empty()) return EGG_ERR_INVALID_ARGUMENT;
    return egg_get_containment(g->h[0], factor, strength);  // (every handle holds the same values)
}

int egg_group_get_containment_hits(egg_group *g, int64_t *hits) {
    if (!g) return EGG_ERR_INVALID_ARGUMENT;
    if (!hits) return gfail(g, EGG_ERR_INVALID_ARGUMENT, "egg_group_get_containment_hits: hits is NULL");
    *hits = 0;
    for (size_t k = 0; k < g->h.size(); ++k) {
        int64_t one = 0;
        GTRY(g, k, egg_get_containment_hits(g->h[k], &one));
        *hits += one;
    }
    return EGG_OK;
}

int egg_group_get_halo_counters(const egg_group *g, int64_t *passes, int64_t *records, int64_t *bytes) {
    if (!g) return EGG_ERR_INVALID_ARGUMENT;
    if (passes) *passes = g->halo_passes;
    if (records) *records = g->halo_records;
    if (bytes) *bytes = g->halo_records * kGhostRecordBytes;
    return EGG_OK;
}

int egg_group_set_config(egg_group *g, int which, const egg_config *cfg) {
    if (!g || !cfg || (which != EGG_WHITE && which != EGG_YOLK)) return EGG_ERR_INVALID_ARGUMENT;
    for (size_t k = 0; k < g->h.size(); ++k)  // (refused by one handle = refused by the first: the checks do not depend on the handle)
        GTRY(g, k, egg_set_config(g->h[k], which, cfg));
    g->budget_stale = true;
    return EGG_OK;
}

int egg_group_get_config(const egg_group *g, int which, egg_config *cfg) {
    if (!g || !cfg || (which != EGG_WHITE && which != EGG_YOLK)) return EGG_ERR_INVALID_ARGUMENT;
    return egg_get_config(g->h[0], which, cfg);
}

int egg_group_get_target(const egg_group *g, int64_t id, double *x, double *y) {  // L:268-278
    if (!g || !x || !y) return EGG_ERR_INVALID_ARGUMENT;
    if (!group_alive(g, id))
        return gfail(const_cast<egg_group *>(g), EGG_ERR_UNKNOWN_ID, "In SimulationHandler.get_target_position: no batch with id `%lld`", (long long)id);
    const egg_group::Rec &r = g->batch[(size_t)id - 1];
    return egg_get_target(g->h[(size_t)r.owner], r.local, x, y);
}

int egg_group_list_ids(const egg_group *g, int64_t cap, int64_t *ids, int64_t *n) {  // L:399-405
    if (!g || !n) return EGG_ERR_INVALID_ARGUMENT;
    int64_t k = 0;
    for (size_t i = 0; i < g->batch.size(); ++i) {
        if (!g->batch[i].alive) continue;
        if (ids && k < cap) ids[k] = (int64_t)i + 1;
        ++k;
    }
    *n = k;
    return EGG_OK;
}

int egg_group_get_n_particles(const egg_group *g, int64_t id, int64_t *n_white, int64_t *n_yolk) {  // L:409-419
    if (!g || !n_white || !n_yolk) return EGG_ERR_INVALID_ARGUMENT;
    if (id < 0) {
        *n_white = *n_yolk = 0;
        for (egg_handle *h : g->h) {
            int64_t nw = 0, ny = 0;
            (void)egg_get_n_particles(h, -1, &nw, &ny);
            *n_white += nw;
            *n_yolk += ny;
        }
        return EGG_OK;
    }
    if (!group_alive(g, id))
        return gfail(const_cast<egg_group *>(g), EGG_ERR_UNKNOWN_ID, "In SimulationHandler:get_n_particles: no batch with id `%lld`", (long long)id);
    const egg_group::Rec &r = g->batch[(size_t)id - 1];
    return egg_get_n_particles(g->h[(size_t)r.owner], r.local, n_white, n_yolk);
}

int egg_group_get_elapsed(const egg_group *g, double *elapsed, double *interpolation_alpha) {
    if (!g) return EGG_ERR_INVALID_ARGUMENT;
    if (elapsed) *elapsed = g->elapsed;
    if (interpolation_alpha) *interpolation_alpha = g->alpha;
    return EGG_OK;
}

int egg_group_download_particles(egg_group *g, int which, int field, double *dst, int64_t cap) {
    if (!g || !dst || (which != EGG_WHITE && which != EGG_YOLK) || field < 0 || field >= EGG_N_FIELDS) return EGG_ERR_INVALID_ARGUMENT;
    const egghost::GroupView v = view_of(g);
    std::string err;
    return gdone(g, egghost::group_draw_download(g->draw, v, which, field, dst, cap, &err), err);
}

int egg_group_get_environment(egg_group *g, int which, egg_environment *out) {
    if (!g || !out || (which != EGG_WHITE && which != EGG_YOLK)) return EGG_ERR_INVALID_ARGUMENT;
    const egghost::GroupView v = view_of(g);
    std::string err;
    return gdone(g, egghost::group_draw_environment(g->draw, v, which, out, &err), err);
}

int egg_group_set_render_config(egg_group *g, int which, const egg_render_config *cfg) {
    if (!g || !cfg || (which != EGG_WHITE && which != EGG_YOLK)) return EGG_ERR_INVALID_ARGUMENT;
    if (!(cfg->outline_thickness >= 0) || !(cfg->texture_scale > 0) || !std::isfinite(cfg->motion_blur) ||
        !std::isfinite(cfg->highlight_strength) || !std::isfinite(cfg->shadow_strength) || !(cfg->outline_thickness <= 256))
        return gfail(g, EGG_ERR_INVALID_ARGUMENT, "egg_group_set_render_config: value out of range");
    g->render_cfg[which] = *cfg;
    // config.color is a new table now (L:1307-1311): batches that shared the old one keep it for themselves
    for (size_t i = 0; i < g->batch.size(); ++i) g->own_color[2 * i + (size_t)which] = 1;
    g->color_version++;
    return EGG_OK;
}

int egg_group_get_render_config(const egg_group *g, int which, egg_render_config *cfg) {
    if (!g || !cfg || (which != EGG_WHITE && which != EGG_YOLK)) return EGG_ERR_INVALID_ARGUMENT;
    *cfg = g->render_cfg[which];
    return EGG_OK;
}

int egg_group_set_render_flags(egg_group *g, int32_t use_particle_color, int32_t use_lighting) {
    if (!g) return EGG_ERR_INVALID_ARGUMENT;
    g->use_particle_color = use_particle_color != 0;
    g->use_lighting = use_lighting != 0;
    g->color_version++;
    return EGG_OK;
}

int egg_group_set_add_color(egg_group *g, int64_t id, int which, double r, double gr, double b, double a) {
    if (!g || (which != EGG_WHITE && which != EGG_YOLK)) return EGG_ERR_INVALID_ARGUMENT;
    if (!group_alive(g, id)) return gfail(g, EGG_ERR_UNKNOWN_ID, "egg_group_set_add_color: no batch with id `%lld`", (long long)id);
    if (std::isnan(r) || std::isnan(gr) || std::isnan(b) || std::isnan(a))  // L:87-103
        return gfail(g, EGG_ERR_INVALID_ARGUMENT, "In SimulationHandler.add: %s color component is not a number", which == EGG_WHITE ? "white" : "yolk");
    g->own_color[2 * (size_t)(id - 1) + (size_t)which] = 1;
    if (g->use_particle_color) {  // add does not clamp (L:978-984)
        const float c[4] = {(float)r, (float)gr, (float)b, (float)a};
        memcpy(&g->pcolor[8 * (size_t)(id - 1) + 4 * (size_t)which], c, sizeof c);
    }
    g->color_version++;
    return EGG_OK;
}

int egg_group_set_color(egg_group *g, int64_t id, int which, double r, double gr, double b, double a) {
    if (!g || (which != EGG_WHITE && which != EGG_YOLK)) return EGG_ERR_INVALID_ARGUMENT;
    if (std::isnan(r) || std::isnan(gr) || std::isnan(b) || std::isnan(a))
        return gfail(g, EGG_ERR_INVALID_ARGUMENT, "egg_group_set_color: a colour component is not a number");
    if (!group_alive(g, id))
        return gfail(g, EGG_WARN_UNKNOWN_ID, "In SimulationHandler.%s: no batch with id `%lld`",
                     which == EGG_WHITE ? "set_white_color" : "set_egg_yolk_color", (long long)id);
    const float c[4] = {clamp01(r), clamp01(gr), clamp01(b), clamp01(a)};  // _assert_color (L:300-319)
    memcpy(&g->pcolor[8 * (size_t)(id - 1) + 4 * (size_t)which], c, sizeof c);
    if (!g->own_color[2 * (size_t)(id - 1) + (size_t)which]) memcpy(g->render_cfg[which].color, c, sizeof c);  // the shared table (L:49-50, L:349-350)
    g->color_version++;
    return EGG_OK;
}

int egg_group_render(egg_group *g, const egg_render_params *p, float *rgba) {
    if (!g || !p) return EGG_ERR_INVALID_ARGUMENT;
    const egghost::GroupView v = view_of(g);
    std::string err;
    return gdone(g, egghost::group_draw_render(g->draw, v, p, rgba, &err), err);
}

int egg_group_get_instances(egg_group *g, int which, egg_instance *data, float *color, int64_t cap, int64_t *n, uint64_t *color_version) {
    if (!g || (which != EGG_WHITE && which != EGG_YOLK) || cap < 0) return EGG_ERR_INVALID_ARGUMENT;
    const egghost::GroupView v = view_of(g);
    if (color_version) *color_version = g->color_version;
    std::string err;
    return gdone(g, egghost::group_draw_instances(g->draw, v, which, data, color, cap, n, &err), err);
}

int egg_group_render_canvas(egg_group *g, int which, float *rgba, int64_t cap_pixels, int32_t *w, int32_t *hgt, double *x0, double *y0) {
    if (!g || (which != EGG_WHITE && which != EGG_YOLK)) return EGG_ERR_INVALID_ARGUMENT;
    const egghost::GroupView v = view_of(g);
    std::string err;
    return gdone(g, egghost::group_draw_canvas(g->draw, v, which, rgba, cap_pixels, w, hgt, x0, y0, &err), err);
}

}  // extern "C"
