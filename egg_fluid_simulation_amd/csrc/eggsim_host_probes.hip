// eggsim_host_probes.hip -- probes (include/eggsim.h, "probes"): the checks of a call, the launches of
// eggsim_probes.hip over the unit table of the shared host layer (eggsim_host_scan.hip), and the way back from a winning
// array index to (batch, key, index in the batch).  A call is two launches on the white stream and one copy back; it stores
// no list and no answer, a step launches nothing of this and takes no argument from it.
#include "eggsim_host.h"

namespace egghost {

struct ProbeState {
    UnitTable units;  // every unit of every type some probe of the last call covered
    DevBuf<double> part_score;
    DevBuf<int32_t> part_index;
    DevBuf<EggProbeOut> out;
};

namespace {

// the grid is sized to the device, not to the scene: kWavesPerCu one-wave workgroups per compute unit at the most
// (EGGSIM_PROBE_WAVES_PER_CU: developer override, 1 .. 32; profiles/r28_probes.md has the sweep behind the default)
constexpr int kWavesPerCu = 16;

}  // namespace
}  // namespace egghost

extern "C" {

// Everything is checked before anything is launched or written.  Not cached: every call measures the arrays
// egg_download_particles would return now.
int egg_probe(egg_handle *h, int32_t n, const egg_probe_query *probes, egg_probe_hit *hits) {
    if (!h) return EGG_ERR_INVALID_ARGUMENT;
    REJECT_IN_FLIGHT(h, "egg_probe");
    static_assert(sizeof(egg_probe_query) == 48 && sizeof(EggProbe) == sizeof(egg_probe_query), "a probe record is 48 bytes");
    static_assert(sizeof(egg_probe_hit) == 56, "a hit is 56 bytes");
    static_assert(EGG_MAX_PROBES == EGG_PB_MAX_PROBES && EGG_PB_MAX_PROBES == EGG_WAVE, "one lane of a wave per probe");
    static_assert(EGG_PROBE_POINT == EGG_PB_POINT && EGG_PROBE_RAY == EGG_PB_RAY, "the kernel's probe kinds are the ABI's");
    static_assert(sizeof(EggProbeArgs) <= 4096, "the list travels in the launch arguments");
    if (n < 0 || n > EGG_MAX_PROBES)
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_probe: n = %d, a call takes 0 .. %d probes", (int)n, EGG_MAX_PROBES);
    if (n > 0 && !probes) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_probe: n = %d without a list", (int)n);
    if (n > 0 && !hits) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_probe: n = %d without hits", (int)n);
    int cover = 0;
    for (int32_t k = 0; k < n; ++k) {
        const egg_probe_query &o = probes[k];
        static const char *const names[2] = {"point", "ray"};
        if (o.kind != EGG_PROBE_POINT && o.kind != EGG_PROBE_RAY)
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_probe: probe %d: unknown kind %d", (int)k, (int)o.kind);
        if (o.type_mask < 1 || o.type_mask > 3)
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_probe: probe %d: type_mask %d (bit 0 white, bit 1 yolk, never 0)", (int)k,
                        (int)o.type_mask);
        const int used = o.kind == EGG_PROBE_POINT ? 3 : 5;  // (parameters a kind does not use are ignored)
        for (int q = 0; q < used; ++q) {
            if (std::isnan(o.p[q]))
                return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_probe: probe %d (%s): parameter %d is a NaN", (int)k, names[o.kind], q);
            if (std::isinf(o.p[q]) && !(o.kind == EGG_PROBE_POINT && q == 2 && o.p[q] > 0))
                return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_probe: probe %d (%s): parameter %d is not finite", (int)k, names[o.kind], q);
        }
        if (o.kind == EGG_PROBE_POINT && o.p[2] < 0)
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_probe: probe %d (point): reach %g is negative", (int)k, o.p[2]);
        if (o.kind == EGG_PROBE_RAY) {
            if (o.p[4] < 0) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_probe: probe %d (ray): pad %g is negative", (int)k, o.p[4]);
            const double ex = o.p[2] - o.p[0], ey = o.p[3] - o.p[1];
            const double l2 = ex * ex + ey * ey, eps = h->sys[0].cfg.eps;
            if (!(l2 >= eps * eps) || !std::isfinite(l2))
                return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_probe: probe %d (ray): degenerate, its squared length %g is below eps squared or not finite",
                            (int)k, l2);
        }
        cover |= o.type_mask;
    }
    if (n == 0) return EGG_OK;
    std::vector<egg_probe_hit> found((size_t)n * 2);  // (zeros: found = 0)
    cover = covered_types(h, cover);
    if (cover != 0) {  // (else nothing to launch: no particles of a type some probe covers)
        (void)hipSetDevice(h->device);
        int rc = upload_atoms(h);
        if (rc != EGG_OK) return rc;
        if (!h->probe_state) h->probe_state = std::make_shared<ProbeState>();
        ProbeState &S = *h->probe_state;
        System &W = h->sys[0], &Y = h->sys[1];
        rc = S.units.refresh(h, "egg_probe", cover, false);
        if (rc != EGG_OK) return rc;
        if (S.units.n_units > 0) {
            const int waves = grid_cap(h, S.units.n_units, kWavesPerCu, "EGGSIM_PROBE_WAVES_PER_CU");
            HIP_TRY(h, S.part_score.reserve((size_t)waves * 2 * EGG_WAVE, false, nullptr));
            HIP_TRY(h, S.part_index.reserve((size_t)waves * 2 * EGG_WAVE, false, nullptr));
            HIP_TRY(h, S.out.reserve((size_t)EGG_MAX_PROBES * 2, false, nullptr));
            HIP_TRY(h, hipStreamSynchronize(Y.stream));
            EggProbeArgs A{};
            EggProbeFinishArgs F{};
            for (int w = 0; w < 2; ++w) {
                System &s = h->sys[w];
                A.x[w] = F.x[w] = s.x[s.cur].p;
                A.y[w] = F.y[w] = s.y[s.cur].p;
                A.radius[w] = F.radius[w] = s.radius.p;
            }
            A.units = S.units.d_units.p;
            A.n_probes = F.n_probes = n;
            A.n_units = S.units.n_units;
            A.part_score = S.part_score.p;
            A.part_index = S.part_index.p;
            memcpy(A.probes, probes, (size_t)n * sizeof(egg_probe_query));
            hipLaunchKernelGGL(egg_probe_scan_kernel, dim3((unsigned)waves), dim3(EGG_WAVE), 0, W.stream, A);
            HIP_TRY(h, hipGetLastError());
            F.part_score = S.part_score.p;
            F.part_index = S.part_index.p;
            F.n_waves = (int32_t)waves;
            F.out = S.out.p;
            const unsigned groups = (unsigned)((n + EGG_PB_FINISH_PROBES - 1) / EGG_PB_FINISH_PROBES);
            hipLaunchKernelGGL(egg_probe_finish_kernel, dim3(groups, 2), dim3(EGG_PB_FINISH_THREADS), 0, W.stream, F);
            HIP_TRY(h, hipGetLastError());
            // (a probe call changes no counter: stats.kernel_launches counts what steps and draws launch)
            EggProbeOut host[EGG_MAX_PROBES * 2];
            HIP_TRY(h, hipMemcpyAsync(host, S.out.p, (size_t)n * 2 * sizeof(EggProbeOut), hipMemcpyDeviceToHost, W.stream));
            HIP_TRY(h, hipStreamSynchronize(W.stream));
            for (int32_t k = 0; k < n; ++k)
                for (int w = 0; w < 2; ++w) {
                    const EggProbeOut &o = host[2 * k + w];
                    if (o.index < 0) continue;
                    // the atom that holds the array index: the last one whose offset does not exceed it
                    const std::vector<Atom> &atoms = h->sys[w].atoms;
                    auto it = std::upper_bound(atoms.begin(), atoms.end(), o.index, [](int32_t at, const Atom &a) { return at < a.offset; });
                    if (it == atoms.begin() || o.index >= (it - 1)->offset + (it - 1)->count)
                        return fail(h, EGG_ERR_DEVICE, "egg_probe: probe %d: the winning index %d lies in no batch", (int)k, (int)o.index);
                    const Atom &a = *(it - 1);
                    const Batch &b = h->batches[(size_t)a.batch];
                    egg_probe_hit &hit = found[(size_t)(2 * k + w)];
                    hit.id = b.id;
                    hit.key = b.key;
                    hit.index = o.index - a.offset;
                    hit.found = 1;
                    hit.score = o.score;
                    hit.x = o.x;
                    hit.y = o.y;
                    hit.radius = o.radius;
                }
        }
    }
    memcpy(hits, found.data(), found.size() * sizeof(egg_probe_hit));
    return EGG_OK;
}

}  // extern "C"
