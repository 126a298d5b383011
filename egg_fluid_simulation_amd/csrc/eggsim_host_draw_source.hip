// eggsim_host_draw_source.hip -- draw(), the environment and the particle download of a scene that is sharded over several
// PROCESSES (egg_fluid_simulation_amd/sharding.py; DESIGN.md section 2.6, "Several processes").  It is the device group's
// draw (eggsim_host_render_group.hip) cut where that reads another handle's memory:
//
//   group draw                                           here
//   gather kernel pulls from the source handle's arrays  egg_draw_pack on the source rank: ONE message of seven fields;
//                                                        the host carries it; egg_draw_source_place on the render rank
//                                                        runs the SAME gather kernel with the message as its source
//   group_keys over the handles' atoms                   egg_draw_source_layout: the caller's replicated key table
//   the group's render records (GroupView)               arguments of egg_draw_source_render
//
// Everything after the placement is the single handle's renderer and reductions, unchanged (render_from,
// environment_of, render_canvas_from).  The shadow arrays, the canvases with their grow-only sizes and the scratch of the
// passes belong to the DrawSource, not to the handle's own draw state (egg_render), as GroupDraw keeps them apart from
// handle 0's.  egg_draw_source_instances packs the placed particles into the reference's two meshes (eggsim_host_instances.hip).  All device work goes to the stream of the handle's white type; every entry point returns with it idle.
#include "eggsim_host.h"

namespace egghost {

struct DrawSource {
    egg_handle::Render R;
    struct Type {
        DrawShadow sh;
        int64_t total = -1;  // -1: no layout yet
        int64_t n_atoms = 0, placed = 0;
        std::vector<float> atom_color;
        DevBuf<int32_t> table;  // run tables of the message being placed
        DevBuf<double> stage;   // a message that arrived in host memory (or on another device)
    } t[2];
};

// memory of this handle's device (a kernel may touch it) or anything else (reached through hipMemcpyDefault)
bool on_device_of(const egg_handle *h, const void *p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // (plain host memory is "invalid value" to some runtimes)
        return false;
    }
    return a.type == hipMemoryTypeDevice && a.device == h->device;
}

namespace {

constexpr int64_t kMaxDrawParticles = std::numeric_limits<int32_t>::max();

DrawSource &source_of(egg_handle *h) {
    if (!h->draw_source) h->draw_source = std::make_shared<DrawSource>();
    return *h->draw_source;
}

int need_complete(egg_handle *h, const DrawSource::Type &T, int which, const char *name) {
    if (T.total < 0) return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: type %d has no layout (egg_draw_source_layout)", name, which);
    if (T.placed != T.total)
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: %lld of %lld particles of type %d are placed (egg_draw_source_place)", name,
                    (long long)T.placed, (long long)T.total, which);
    return EGG_OK;
}

int field_index(int field) {
    for (int f = 0; f < EGG_GATHER_FIELDS; ++f)
        if (kDrawFields[f] == field) return f;
    return -1;
}

}  // namespace
}  // namespace egghost

extern "C" {

int egg_draw_pack(egg_handle *h, int which, void *out, int64_t cap_particles) {
    if (!h || (which != EGG_WHITE && which != EGG_YOLK) || cap_particles < 0) return EGG_ERR_INVALID_ARGUMENT;
    REJECT_IN_FLIGHT(h, "egg_draw_pack");
    System &s = h->sys[which];
    if (cap_particles < s.n)
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_draw_pack: buffer holds %lld of %lld particles", (long long)cap_particles, (long long)s.n);
    if (s.n == 0) return EGG_OK;
    if (!out) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_draw_pack: no buffer");
    if (s.n > kMaxDrawParticles) return fail(h, EGG_ERR_UNSUPPORTED, "egg_draw_pack: more than 2^31 - 1 particles of one type");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->sys[which ^ 1].stream));  // (a fused launch or a hand-over may have used the other stream)
    const size_t n = (size_t)s.n;
    const bool direct = on_device_of(h, out);
    if (!direct) HIP_TRY(h, h->draw_pack.reserve(EGG_GATHER_FIELDS * n, false, s.stream));
    EggDrawPackArgs A;
    memset(&A, 0, sizeof A);
    for (int f = 0; f < EGG_GATHER_FIELDS; ++f) A.src[f] = draw_field_of(s, kDrawFields[f]);
    A.dst = direct ? (double *)out : h->draw_pack.p;
    A.n = (int32_t)n;
    hipLaunchKernelGGL(egg_draw_pack_kernel, dim3((unsigned)((n + EGG_GATHER_BLOCK - 1) / EGG_GATHER_BLOCK)), dim3(EGG_GATHER_BLOCK), 0,
                       s.stream, A);
    HIP_TRY(h, hipGetLastError());
    h->stats.kernel_launches++;
    if (!direct) HIP_TRY(h, hipMemcpyAsync(out, h->draw_pack.p, EGG_GATHER_FIELDS * n * 8, hipMemcpyDefault, s.stream));
    HIP_TRY(h, hipStreamSynchronize(s.stream));
    return EGG_OK;
}

int egg_draw_source_layout(egg_handle *h, int which, int64_t total, int64_t n_atoms, const int64_t *atom_offset, const float *atom_color) {
    if (!h || (which != EGG_WHITE && which != EGG_YOLK)) return EGG_ERR_INVALID_ARGUMENT;
    if (total < 0 || n_atoms < 0 || (n_atoms > 0 && (!atom_offset || !atom_color)) || (n_atoms == 0) != (total == 0))
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_draw_source_layout: invalid arguments");
    if (total > kMaxDrawParticles)
        return fail(h, EGG_ERR_UNSUPPORTED, "egg_draw_source_layout: more than 2^31 - 1 particles of one type over all ranks");
    for (int64_t a = 0; a < n_atoms; ++a)
        if ((a == 0 ? atom_offset[a] != 0 : atom_offset[a] <= atom_offset[a - 1]) || atom_offset[a] >= total)
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_draw_source_layout: atom offsets must start at 0, ascend and stay below the total");
    HIP_TRY(h, hipSetDevice(h->device));
    DrawSource::Type &T = source_of(h).t[which];
    hipStream_t st = h->sys[0].stream;
    T.total = -1;
    T.placed = 0;
    for (int f = 0; f < EGG_GATHER_FIELDS; ++f) {
        const hipError_t e = T.sh.f[f].reserve((size_t)total, false, st);
        if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            return fail(h, EGG_ERR_UNSUPPORTED, "egg_draw_source_layout: no room for %lld particles on the render device (56 B each)", (long long)total);
        }
        HIP_TRY(h, e);
    }
    std::vector<int32_t> off((size_t)n_atoms + 1);
    for (int64_t a = 0; a < n_atoms; ++a) off[(size_t)a] = (int32_t)atom_offset[a];
    off[(size_t)n_atoms] = (int32_t)total;
    HIP_TRY(h, T.sh.atom_offset.reserve((size_t)n_atoms + 1, false, st));
    HIP_TRY(h, hipMemcpyAsync(T.sh.atom_offset.p, off.data(), ((size_t)n_atoms + 1) * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipStreamSynchronize(st));  // (pageable host memory)
    T.atom_color.assign(atom_color, atom_color + 4 * (size_t)n_atoms);
    T.n_atoms = n_atoms;
    T.total = total;
    return EGG_OK;
}

int egg_draw_source_place(egg_handle *h, int which, const void *msg, int64_t n, int64_t n_runs, const int64_t *run_src, const int64_t *run_dst) {
    if (!h || (which != EGG_WHITE && which != EGG_YOLK) || n < 0 || n_runs < 0) return EGG_ERR_INVALID_ARGUMENT;
    if (!msg) REJECT_IN_FLIGHT(h, "egg_draw_source_place");  // (the handle's own arrays are the source)
    DrawSource::Type &T = source_of(h).t[which];
    if (T.total < 0) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_draw_source_place: type %d has no layout (egg_draw_source_layout)", which);
    System &s = h->sys[which];
    if (!msg && n != s.n)
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_draw_source_place: the handle holds %lld particles of type %d, not %lld", (long long)s.n, which, (long long)n);
    if (n == 0) return EGG_OK;
    if (n_runs < 1 || !run_src || !run_dst || T.placed + n > T.total)
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_draw_source_place: no runs, or more particles than the layout holds");
    // every run lies inside the message and inside the shadow arrays: nothing is enqueued before all of them are checked
    std::vector<int32_t> rs((size_t)n_runs), rd((size_t)n_runs);
    for (int64_t r = 0; r < n_runs; ++r) {
        const int64_t first = run_src[r], end = r + 1 < n_runs ? run_src[r + 1] : n;
        if ((r == 0 && first != 0) || end <= first || end > n || run_dst[r] < 0 || run_dst[r] + (end - first) > T.total)
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_draw_source_place: run %lld lies outside the message or the layout", (long long)r);
        rs[(size_t)r] = (int32_t)first;
        rd[(size_t)r] = (int32_t)run_dst[r];
    }
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = h->sys[0].stream;
    const double *src[EGG_GATHER_FIELDS];
    if (!msg) {
        HIP_TRY(h, hipStreamSynchronize(h->sys[1].stream));
        for (int f = 0; f < EGG_GATHER_FIELDS; ++f) src[f] = draw_field_of(s, kDrawFields[f]);
    } else {
        const double *base = (const double *)msg;
        if (!on_device_of(h, msg)) {  // staged once per message
            HIP_TRY(h, T.stage.reserve(EGG_GATHER_FIELDS * (size_t)n, false, st));
            HIP_TRY(h, hipMemcpyAsync(T.stage.p, msg, EGG_GATHER_FIELDS * (size_t)n * 8, hipMemcpyDefault, st));
            base = T.stage.p;
        }
        for (int f = 0; f < EGG_GATHER_FIELDS; ++f) src[f] = base + (size_t)f * (size_t)n;
    }
    std::vector<int32_t> tab;
    gather_table(rs, rd, n, tab);
    HIP_TRY(h, T.table.reserve(tab.size(), false, st));
    HIP_TRY(h, hipMemcpyAsync(T.table.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));
    const int rc = launch_gather(h, st, src, T.sh, EGG_GATHER_FIELDS, T.table.p, (int32_t)n_runs, n, T.total);
    HIP_TRY(h, hipStreamSynchronize(st));  // (the table is pageable; the message may go when the call returns)
    if (rc != EGG_OK) return rc;
    T.placed += n;
    return EGG_OK;
}

int egg_draw_source_render(egg_handle *h, const egg_render_params *p, const egg_render_config *cfg, int32_t use_particle_color,
                           int32_t use_lighting, int32_t stepped, double interpolation_alpha, float *rgba) {
    if (!h || !p || !cfg) return EGG_ERR_INVALID_ARGUMENT;
    for (int w = 0; w < 2; ++w)
        if (!(cfg[w].outline_thickness >= 0) || !(cfg[w].texture_scale > 0) || !std::isfinite(cfg[w].motion_blur) ||
            !std::isfinite(cfg[w].highlight_strength) || !std::isfinite(cfg[w].shadow_strength) || !(cfg[w].outline_thickness <= 256))
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_draw_source_render: render config value out of range");
    DrawSource &D = source_of(h);
    RenderSource S;
    S.h = h;
    S.R = &D.R;
    S.cfg = cfg;
    S.use_particle_color = use_particle_color != 0;
    S.use_lighting = use_lighting != 0;
    S.stepped = stepped != 0;
    S.alpha = interpolation_alpha;
    S.max_radius = std::max(h->sys[0].cfg.max_radius, h->sys[1].cfg.max_radius);
    S.stream = h->sys[0].stream;
    collider_source_of(h, S);  // (the render rank's own list: every rank holds and advances the same one)
    for (int w = 0; w < 2; ++w) {
        const int rc = need_complete(h, D.t[w], w, "egg_draw_source_render");
        if (rc != EGG_OK) return rc;
        shadow_source(D.t[w].sh, D.t[w].total, S.stream, S.t[w]);
        S.t[w].atom_color = D.t[w].atom_color;
    }
    return render_from(S, p, rgba, "egg_draw_source_render");
}

int egg_draw_source_render_canvas(egg_handle *h, int which, float *rgba, int64_t cap_pixels, int32_t *w, int32_t *hgt, double *x0, double *y0) {
    if (!h || (which != EGG_WHITE && which != EGG_YOLK)) return EGG_ERR_INVALID_ARGUMENT;
    return render_canvas_from(h, source_of(h).R, "egg_draw_source_render", which, rgba, cap_pixels, w, hgt, x0, y0);
}

int egg_draw_source_environment(egg_handle *h, int which, int32_t stepped, egg_environment *out) {
    if (!h || !out || (which != EGG_WHITE && which != EGG_YOLK)) return EGG_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    DrawSource::Type &T = source_of(h).t[which];
    RenderSource::Type S;
    if (stepped) {  // (before the first _step the fields are the empty ones whatever the arrays hold)
        const int rc = need_complete(h, T, which, "egg_draw_source_environment");
        if (rc != EGG_OK) return rc;
        shadow_source(T.sh, T.total, h->sys[0].stream, S);
    }
    return environment_of(h, stepped != 0, S, out);
}

int egg_draw_source_download(egg_handle *h, int which, int field, double *dst, int64_t cap) {
    if (!h || !dst || (which != EGG_WHITE && which != EGG_YOLK)) return EGG_ERR_INVALID_ARGUMENT;
    const int f = field_index(field);
    if (f < 0) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_draw_source_download: field %d is not one of the seven draw fields", field);
    DrawSource::Type &T = source_of(h).t[which];
    const int rc = need_complete(h, T, which, "egg_draw_source_download");
    if (rc != EGG_OK) return rc;
    if (cap < T.total)
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_draw_source_download: buffer holds %lld of %lld particles", (long long)cap, (long long)T.total);
    if (T.total == 0) return EGG_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = h->sys[0].stream;
    HIP_TRY(h, hipMemcpyAsync(dst, T.sh.f[f].p, (size_t)T.total * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    return EGG_OK;
}

int egg_draw_source_instances(egg_handle *h, int which, egg_instance *data, float *color, int64_t cap, int64_t *n) {
    if (!h || (which != EGG_WHITE && which != EGG_YOLK) || cap < 0) return EGG_ERR_INVALID_ARGUMENT;
    DrawSource::Type &T = source_of(h).t[which];
    const int rc = need_complete(h, T, which, "egg_draw_source_instances");
    if (rc != EGG_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    RenderSource::Type S;
    shadow_source(T.sh, T.total, h->sys[0].stream, S);  // (every placement ended with that stream idle)
    S.atom_color = T.atom_color;
    return instances_from(h, h->sys[0].stream, S, "egg_draw_source_instances", data, color, cap, n);
}

}  // extern "C"
