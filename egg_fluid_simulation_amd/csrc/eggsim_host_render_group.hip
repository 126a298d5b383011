// eggsim_host_render_group.hip -- draw(), the environment and the particle download of a device group (eggsim_group.cpp):
// a gather to ONE render device, then the single handle's renderer and reductions, unchanged (DESIGN.md section 2.6,
// "Several devices").
//
// The render device is the device of handle 0.  Per type it holds shadow arrays x, y, last_x, last_y, vx, vy, radius of
// ALL particles of the group in global-key order (the key of DESIGN.md section 2.7: the particle's index in one handle
// holding every live batch in ascending id), atom_offset and the atoms' colours in the same order.  Per source handle
// and type one launch of egg_group_gather_kernel (eggsim_render_group.hip) on the render handle's stream PULLS the
// handle's particles into their places: plain loads from the source's arrays (peer memory when the ordinals differ),
// plain stores to the render device's own memory.
//
// Ordering.  A draw is refused while a member handle has a step in flight, so nothing writes a source array during the
// gather; an event recorded on both streams of the source and waited for on the render stream orders the gather behind
// whatever those streams still hold (hand-over copies, a re-derivation).  Every entry point here ends with a synchronise
// of the render stream, so the gather has finished before the caller can start the next step.
#include "eggsim_group_draw.h"
#include "eggsim_host.h"

namespace egghost {

struct GroupDraw {
    egg_handle::Render R;  // canvases with their grow-only sizes, screen, scratch: the group's, not handle 0's
    struct Type {
        DrawShadow sh;  // the shadow arrays, atom_offset, reduction scratch
        GroupKeys keys;
        std::vector<uint64_t> sig;              // every handle's atoms_gen when the tables below were built
        std::vector<DevBuf<int32_t>> tables;    // per source handle: run_src [runs + 1], run_dst [runs], block_run [blocks]
        std::vector<int32_t> n_runs;
    } t[2];
    std::vector<hipEvent_t> ev;  // two per source handle, on its device
    bool peers = false;
    ~GroupDraw() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// ---- shared with the draw of a scene sharded over processes (eggsim_host_draw_source.hip)

const double *draw_field_of(System &s, int field) {
    switch (field) {
        case EGG_FIELD_X: return s.x[s.cur].p;
        case EGG_FIELD_Y: return s.y[s.cur].p;
        case EGG_FIELD_VX: return s.vx[s.cur].p;
        case EGG_FIELD_VY: return s.vy[s.cur].p;
        case EGG_FIELD_LAST_X: return s.x[s.cur ^ 1].p;  // positions at the start of the most recent _step (L:1795-1815)
        case EGG_FIELD_LAST_Y: return s.y[s.cur ^ 1].p;
        case EGG_FIELD_RADIUS: return s.radius.p;
        case EGG_FIELD_INV_MASS: return s.inv_mass.p;
        case EGG_FIELD_MASS_T: return s.mass_t.p;
        default: return nullptr;
    }
}

const int kDrawFields[EGG_GATHER_FIELDS] = {EGG_FIELD_X,  EGG_FIELD_Y,  EGG_FIELD_LAST_X, EGG_FIELD_LAST_Y,
                                            EGG_FIELD_VX, EGG_FIELD_VY, EGG_FIELD_RADIUS};

// run_src [runs + 1] (the last entry is n), run_dst [runs], block_run [blocks]: what egg_group_gather_kernel reads
void gather_table(const std::vector<int32_t> &run_src, const std::vector<int32_t> &run_dst, int64_t n, std::vector<int32_t> &tab) {
    const size_t nr = run_src.size(), nb = ((size_t)n + EGG_GATHER_BLOCK - 1) / EGG_GATHER_BLOCK;
    tab = run_src;
    tab.push_back((int32_t)n);
    tab.insert(tab.end(), run_dst.begin(), run_dst.end());
    size_t r = 0;
    for (size_t b = 0; b < nb; ++b) {
        const int32_t first = (int32_t)(b * EGG_GATHER_BLOCK);
        while (r + 1 < nr && first >= run_src[r + 1]) ++r;
        tab.push_back((int32_t)r);
    }
}

// one launch of egg_group_gather_kernel on `st`: n particles of src[0 .. n_fields) into their places in the shadow arrays
int launch_gather(egg_handle *rh, hipStream_t st, const double *const *src, DrawShadow &sh, int n_fields, const int32_t *table,
                  int32_t n_runs, int64_t n, int64_t total) {
    EggGatherArgs A;
    memset(&A, 0, sizeof A);
    for (int f = 0; f < n_fields; ++f) {
        A.src[f] = src[f];
        A.dst[f] = sh.f[f].p;
    }
    A.run_src = table;
    A.run_dst = A.run_src + n_runs + 1;
    A.block_run = A.run_dst + n_runs;
    A.n = (int32_t)n;
    A.n_runs = n_runs;
    A.n_fields = n_fields;
    A.total = (int32_t)total;
    hipLaunchKernelGGL(egg_group_gather_kernel, dim3((unsigned)(((size_t)n + EGG_GATHER_BLOCK - 1) / EGG_GATHER_BLOCK)),
                       dim3(EGG_GATHER_BLOCK), 0, st, A);
    HIP_TRY(rh, hipGetLastError());
    rh->stats.kernel_launches++;
    return EGG_OK;
}

// the shadow arrays as the renderer's source of one type (the colours are the caller's)
void shadow_source(DrawShadow &sh, int64_t total, hipStream_t env_stream, RenderSource::Type &S) {
    S.x = sh.f[0].p;
    S.y = sh.f[1].p;
    S.last_x = sh.f[2].p;
    S.last_y = sh.f[3].p;
    S.vx = sh.f[4].p;
    S.vy = sh.f[5].p;
    S.radius = sh.f[6].p;
    S.atom_offset = sh.atom_offset.p;
    S.n = total;
    S.env_stream = env_stream;
    S.d_env = &sh.d_env;
}

namespace {

int device_fail(const GroupView &V, int k, std::string *error, int rc) {
    char buf[64];
    snprintf(buf, sizeof buf, "device %d: ", k);
    *error = buf + V.hs[k]->error;
    return rc;
}

#define GD_TRY(k, expr)                                                                                            \
    do {                                                                                                           \
        const int _rc = (expr);                                                                                    \
        if (_rc != EGG_OK) return device_fail(V, (k), error, _rc);                                                 \
    } while (0)

#define GD_HIP(k, expr) GD_TRY(k, [&]() -> int { HIP_TRY(V.hs[k], (expr)); return EGG_OK; }())

int refuse_in_flight(const GroupView &V, const char *name, std::string *error) {
    for (int k = 0; k < V.n; ++k)
        if (V.hs[k]->in_flight) {
            char buf[160];
            snprintf(buf, sizeof buf, "%s: a step is in flight on device %d (egg_step_begin without egg_step_end)", name, k);
            *error = buf;
            return EGG_ERR_INVALID_ARGUMENT;
        }
    return EGG_OK;
}

// the atoms of every handle current, the group's keys of type w and -- when the membership changed -- the run tables
int update_tables(GroupDraw *D, const GroupView &V, int w, std::string *error) {
    GroupDraw::Type &T = D->t[w];
    std::vector<uint64_t> sig((size_t)V.n);
    for (int k = 0; k < V.n; ++k) {
        (void)hipSetDevice(V.hs[k]->device);
        GD_TRY(k, upload_atoms(V.hs[k], w));
        sig[(size_t)k] = V.hs[k]->sys[w].atoms_gen;
    }
    if (sig == T.sig && T.tables.size() == (size_t)V.n) return EGG_OK;
    group_keys(V.hs, V.n, w, T.keys);
    if (T.keys.total > (int64_t)std::numeric_limits<int32_t>::max()) {
        *error = "egg_group_render: more than 2^31 - 1 particles of one type in the group";
        return EGG_ERR_UNSUPPORTED;
    }
    egg_handle *rh = V.hs[0];
    hipStream_t st = rh->sys[0].stream;
    (void)hipSetDevice(rh->device);
    T.tables.resize((size_t)V.n);
    T.n_runs.assign((size_t)V.n, 0);
    const size_t na = T.keys.sizes.size();
    std::vector<int32_t> off(na + 1);
    for (size_t b = 0; b < na; ++b) off[b] = (int32_t)T.keys.base[b];
    off[na] = (int32_t)T.keys.total;
    GD_HIP(0, T.sh.atom_offset.reserve(na + 1, false, st));
    GD_HIP(0, hipMemcpyAsync(T.sh.atom_offset.p, off.data(), (na + 1) * 4, hipMemcpyHostToDevice, st));
    std::vector<std::vector<int32_t>> host((size_t)V.n);
    for (int k = 0; k < V.n; ++k) {
        egg_handle *h = V.hs[k];
        System &s = h->sys[w];
        if (s.n == 0) continue;
        std::vector<int32_t> run_src, run_dst;
        int64_t next_dst = -1;
        for (const Atom &a : s.atoms) {
            const int64_t base = T.keys.base_of(h->batches[(size_t)a.batch].key, a.count);
            if (base != next_dst) {  // (an atom that continues the previous one's destinations stays in its run)
                run_src.push_back(a.offset);
                run_dst.push_back((int32_t)base);
            }
            next_dst = base + a.count;
        }
        std::vector<int32_t> &tab = host[(size_t)k];
        gather_table(run_src, run_dst, s.n, tab);
        T.n_runs[(size_t)k] = (int32_t)run_src.size();
        GD_HIP(0, T.tables[(size_t)k].reserve(tab.size(), false, st));
        GD_HIP(0, hipMemcpyAsync(T.tables[(size_t)k].p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));
    }
    GD_HIP(0, hipStreamSynchronize(st));  // (the tables are pageable host memory; membership changes only)
    T.sig = sig;
    return EGG_OK;
}

// `n_fields` fields of every particle of type w into the shadow arrays f[0 .. n_fields), in global-key order
int gather(GroupDraw *D, const GroupView &V, int w, const int *fields, int n_fields, const char *name, std::string *error) {
    int rc = refuse_in_flight(V, name, error);
    if (rc != EGG_OK) return rc;
    if (!D->peers) {  // the gather reads the other devices' memory
        rc = group_peers(V.hs, V.n, name, "the gather to the render device", error);
        if (rc != EGG_OK) return rc;
        D->peers = true;
    }
    rc = update_tables(D, V, w, error);
    if (rc != EGG_OK) return rc;
    GroupDraw::Type &T = D->t[w];
    egg_handle *rh = V.hs[0];
    hipStream_t st = rh->sys[0].stream;
    const size_t total = (size_t)T.keys.total;
    if (total == 0) return EGG_OK;
    (void)hipSetDevice(rh->device);
    for (int f = 0; f < n_fields; ++f) GD_HIP(0, T.sh.f[f].reserve(total, false, st));
    if (D->ev.size() < 2 * (size_t)V.n) D->ev.resize(2 * (size_t)V.n, nullptr);
    for (int k = 0; k < V.n; ++k) {
        egg_handle *h = V.hs[k];
        System &s = h->sys[w];
        if (s.n == 0) continue;  // a handle that owns nothing of the type is normal
        (void)hipSetDevice(h->device);
        for (int q = 0; q < 2; ++q) {
            hipEvent_t &e = D->ev[2 * (size_t)k + q];
            if (!e) GD_HIP(k, hipEventCreateWithFlags(&e, hipEventDisableTiming));
            GD_HIP(k, hipEventRecord(e, h->sys[q].stream));
        }
        (void)hipSetDevice(rh->device);
        for (int q = 0; q < 2; ++q) GD_HIP(0, hipStreamWaitEvent(st, D->ev[2 * (size_t)k + q], 0));
        const double *src[EGG_GATHER_FIELDS] = {};
        for (int f = 0; f < n_fields; ++f) src[f] = draw_field_of(s, fields[f]);
        GD_TRY(0, launch_gather(rh, st, src, T.sh, n_fields, T.tables[(size_t)k].p, T.n_runs[(size_t)k], s.n, (int64_t)total));
    }
    return EGG_OK;
}

void fill_type(GroupDraw *D, const GroupView &V, int w, RenderSource::Type &S, bool colors) {
    GroupDraw::Type &T = D->t[w];
    shadow_source(T.sh, T.keys.total, V.hs[0]->sys[0].stream, S);
    if (!colors) return;
    const size_t na = T.keys.sizes.size();
    S.atom_color.assign(4 * na, 1.0f);
    for (size_t b = 0; b < na; ++b) {  // (in a group a batch's key is its global id)
        const int64_t gid = T.keys.sizes[b].first;
        if (gid >= 1 && gid <= V.n_ids) memcpy(&S.atom_color[4 * b], V.pcolor + 8 * (size_t)(gid - 1) + 4 * (size_t)w, 16);
    }
}

}  // namespace

GroupDraw *group_draw_create() { return new GroupDraw(); }

void group_draw_destroy(GroupDraw *d) { delete d; }

int group_draw_render(GroupDraw *D, const GroupView &V, const egg_render_params *p, float *rgba, std::string *error) {
    egg_handle *rh = V.hs[0];
    RenderSource S;
    S.h = rh;
    S.R = &D->R;
    S.cfg = V.cfg;
    S.use_particle_color = V.use_particle_color;
    S.use_lighting = V.use_lighting;
    S.stepped = V.stepped;
    S.alpha = V.alpha;
    S.max_radius = std::max(rh->sys[0].cfg.max_radius, rh->sys[1].cfg.max_radius);
    S.stream = rh->sys[0].stream;
    collider_source_of(rh, S);  // (every handle of the group holds and advances the same list)
    for (int w = 0; w < 2; ++w) {
        const int rc = gather(D, V, w, kDrawFields, EGG_GATHER_FIELDS, "egg_group_render", error);
        if (rc != EGG_OK) return rc;
        fill_type(D, V, w, S.t[w], true);
    }
    (void)hipSetDevice(rh->device);
    const int rc = render_from(S, p, rgba, "egg_group_render");
    if (rc != EGG_OK) *error = rh->error;
    return rc;
}

int group_draw_canvas(GroupDraw *D, const GroupView &V, int which, float *rgba, int64_t cap_pixels, int32_t *w, int32_t *hgt, double *x0,
                      double *y0, std::string *error) {
    const int rc = render_canvas_from(V.hs[0], D->R, "egg_group_render", which, rgba, cap_pixels, w, hgt, x0, y0);
    if (rc != EGG_OK) *error = V.hs[0]->error;
    return rc;
}

int group_draw_environment(GroupDraw *D, const GroupView &V, int which, egg_environment *out, std::string *error) {
    egg_handle *rh = V.hs[0];
    RenderSource::Type T;
    if (V.stepped) {  // (before the first _step the fields are the empty ones whatever the arrays hold)
        const int rc = gather(D, V, which, kDrawFields, EGG_GATHER_FIELDS, "egg_group_get_environment", error);
        if (rc != EGG_OK) return rc;
        fill_type(D, V, which, T, false);
    }
    (void)hipSetDevice(rh->device);
    const int rc = environment_of(rh, V.stepped, T, out);
    if (rc != EGG_OK) *error = rh->error;
    return rc;
}

// the two meshes of egg_get_instances over the group: the draw's gather, then the pack on the render device
int group_draw_instances(GroupDraw *D, const GroupView &V, int which, egg_instance *data, float *color, int64_t cap, int64_t *n,
                         std::string *error) {
    egg_handle *rh = V.hs[0];
    int rc = gather(D, V, which, kDrawFields, EGG_GATHER_FIELDS, "egg_group_get_instances", error);
    if (rc != EGG_OK) return rc;
    RenderSource::Type T;
    fill_type(D, V, which, T, color != nullptr);
    (void)hipSetDevice(rh->device);
    rc = instances_from(rh, rh->sys[0].stream, T, "egg_group_get_instances", data, color, cap, n);  // (the gather's stream)
    if (rc != EGG_OK) *error = rh->error;
    return rc;
}

int group_draw_download(GroupDraw *D, const GroupView &V, int which, int field, double *dst, int64_t cap, std::string *error) {
    egg_handle *rh = V.hs[0];
    GroupDraw::Type &T = D->t[which];
    int rc;
    if (field == EGG_FIELD_BATCH_ID) {
        rc = update_tables(D, V, which, error);
    } else {
        rc = gather(D, V, which, &field, 1, "egg_group_download_particles", error);
    }
    if (rc != EGG_OK) return rc;
    const int64_t total = T.keys.total;
    if (cap < total) {
        char buf[160];
        snprintf(buf, sizeof buf, "egg_group_download_particles: buffer holds %lld of %lld particles", (long long)cap, (long long)total);
        *error = buf;
        return EGG_ERR_INVALID_ARGUMENT;
    }
    if (total == 0) return EGG_OK;
    if (field == EGG_FIELD_BATCH_ID) {
        for (size_t b = 0; b < T.keys.sizes.size(); ++b)
            for (int64_t k = 0; k < T.keys.sizes[b].second; ++k) dst[T.keys.base[b] + k] = (double)T.keys.sizes[b].first;
        return EGG_OK;
    }
    (void)hipSetDevice(rh->device);
    hipStream_t st = rh->sys[0].stream;
    GD_HIP(0, hipMemcpyAsync(dst, T.sh.f[0].p, (size_t)total * 8, hipMemcpyDeviceToHost, st));
    GD_HIP(0, hipStreamSynchronize(st));
    return EGG_OK;
}

}  // namespace egghost
