// eggsim_host_impulses.hip -- impulses (include/eggsim_impulse.h): the checks of a call and the
// launches of eggsim_impulses.hip over the unit table of the shared host layer (eggsim_host_scan.hip).  A call copies its records up (and the unit table, when the atoms
// moved since the last call), launches the edit and, when totals are asked for, the finishing kernel, and copies the
// totals back once.  It stores no list and no answer; a step launches nothing of this and takes no argument from it.
#include "eggsim_host.h"

namespace egghost {

struct ImpulseState {
    DevBuf<EggImpulse> d_recs;       // the call's records, checked and normalised
    UnitTable units;                 // every unit of both types, with the id of its batch
    DevBuf<long long> partials, out;
};

namespace {

// the grid is sized to the device, not to the scene: kWavesPerCu one-wave workgroups per compute unit at the most
constexpr int kWavesPerCu = 8;

}  // namespace
}  // namespace egghost

extern "C" {

// Everything is checked before anything is launched or changed.
int egg_impulse(egg_handle *h, int32_t n, const egg_impulse_record *list, egg_impulse_result *results) {
    if (!h) return EGG_ERR_INVALID_ARGUMENT;
    static_assert(sizeof(egg_impulse_record) == 96 && sizeof(EggImpulse) == sizeof(egg_impulse_record), "an impulse record is 96 bytes");
    static_assert(offsetof(egg_impulse_record, action) == 56 && offsetof(EggImpulse, action) == 56, "the action follows the region");
    static_assert(offsetof(egg_impulse_record, id) == 64 && offsetof(EggImpulse, id) == 64 && offsetof(egg_impulse_record, a) == 72 && offsetof(EggImpulse, a) == 72,
                  "the id and the parameters");
    static_assert(sizeof(egg_impulse_result) == 64 && EGG_IM_ROWS * sizeof(long long) == sizeof(egg_impulse_result), "a result is 64 bytes");
    static_assert(EGG_MAX_IMPULSES == EGG_IM_MAX && EGG_IM_MAX == EGG_WAVE, "one lane of a wave per record");
    static_assert(EGG_IMPULSE_SCALE == EGG_IM_SCALE, "the kernel's scale is the ABI's");
    static_assert(EGG_IMPULSE_KICK == EGG_IM_KICK && EGG_IMPULSE_BLAST == EGG_IM_BLAST && EGG_IMPULSE_SWIRL == EGG_IM_SWIRL &&
                      EGG_IMPULSE_BRAKE == EGG_IM_BRAKE && EGG_IMPULSE_LINEAR == EGG_IM_LINEAR && EGG_IMPULSE_BY_INV_MASS == EGG_IM_BY_INV_MASS &&
                      EGG_IMPULSE_ALL_BATCHES == EGG_IM_ALL_BATCHES,
                  "the kernel's actions, flags and sentinel are the ABI's");
    REJECT_IN_FLIGHT(h, "egg_impulse");
    if (n < 0 || n > EGG_MAX_IMPULSES)
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_impulse: n = %d, a call takes 0 .. %d records", (int)n, EGG_MAX_IMPULSES);
    if (n > 0 && !list) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_impulse: n = %d without a list", (int)n);
    std::vector<egg_impulse_record> recs((size_t)n);
    bool need_inv_mass = false;
    for (int32_t k = 0; k < n; ++k) {
        egg_impulse_record &o = recs[(size_t)k];
        o = list[k];
        static const char *const names[4] = {"kick", "blast", "swirl", "brake"};
        static const int used_of[4] = {2, 3, 3, 3};
        if (o.action < EGG_IMPULSE_KICK || o.action > EGG_IMPULSE_BRAKE)
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_impulse: record %d: unknown action %d", (int)k, (int)o.action);
        if (o.flags & ~(EGG_IMPULSE_LINEAR | EGG_IMPULSE_BY_INV_MASS))
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_impulse: record %d (%s): unknown flag bits %d", (int)k, names[o.action], (int)o.flags);
        {
            const int rc = check_region(h, "egg_impulse: record", k, o.region);
            if (rc != EGG_OK) return rc;
        }
        if (o.flags & EGG_IMPULSE_LINEAR) {  // (kinds 1 and 3 of a region: the disc and the capsule)
            const bool round_kind = o.region.kind == 1 || o.region.kind == 3;
            const double R = o.region.kind == 1 ? o.region.p[2] : o.region.p[4];
            if (!round_kind || !(R > 0.0))
                return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_impulse: record %d (%s): the linear weight is for a disc or a capsule with R > 0",
                            (int)k, names[o.action]);
        }
        if ((o.flags & EGG_IMPULSE_BY_INV_MASS) && (o.action == EGG_IMPULSE_SWIRL || o.action == EGG_IMPULSE_BRAKE))
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_impulse: record %d (%s): the weight by inverse mass is for a kick or a blast", (int)k,
                        names[o.action]);
        for (int q = 0; q < 3; ++q) {
            if (q >= used_of[o.action]) o.a[q] = 0.0;  // (not a parameter of the action)
            if (!std::isfinite(o.a[q]))
                return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_impulse: record %d (%s): parameter %d is not finite", (int)k, names[o.action], q);
        }
        if (o.action == EGG_IMPULSE_BRAKE && !(o.a[2] >= 0.0 && o.a[2] <= 1.0))
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_impulse: record %d (brake): k = %g is outside [0, 1]", (int)k, o.a[2]);
        if (o.id != EGG_IMPULSE_ALL_BATCHES && o.id != EGG_IMPULSE_NO_BATCH && !find_batch(h, o.id))
            return fail(h, EGG_ERR_UNKNOWN_ID, "egg_impulse: record %d: no batch with id `%lld`", (int)k, (long long)o.id);
        need_inv_mass |= (o.flags & EGG_IMPULSE_BY_INV_MASS) != 0;
    }
    if (results && n > 0) memset(results, 0, (size_t)n * sizeof(egg_impulse_result));
    System &W = h->sys[0], &Y = h->sys[1];
    if (n == 0 || W.n + Y.n == 0) return EGG_OK;
    (void)hipSetDevice(h->device);
    int rc = upload_atoms(h);
    if (rc != EGG_OK) return rc;
    if (!h->impulse_state) h->impulse_state = std::make_shared<ImpulseState>();
    ImpulseState &S = *h->impulse_state;
    rc = S.units.refresh(h, "egg_impulse", 3, true);
    if (rc != EGG_OK) return rc;
    // a list whose every record names no batch (a member of a group asked to check it) launches nothing
    bool reach = false;
    for (const egg_impulse_record &o : recs) reach |= o.id != EGG_IMPULSE_NO_BATCH;
    if (S.units.n_units == 0 || !reach) return EGG_OK;
    const int waves = grid_cap(h, S.units.n_units, kWavesPerCu, nullptr);
    HIP_TRY(h, S.d_recs.reserve(EGG_MAX_IMPULSES, false, nullptr));
    if (results) {
        HIP_TRY(h, S.partials.reserve((size_t)waves * EGG_IM_ROWS * EGG_WAVE, false, nullptr));
        HIP_TRY(h, S.out.reserve((size_t)EGG_IM_ROWS * EGG_WAVE, false, nullptr));
    }
    HIP_TRY(h, hipMemcpy(S.d_recs.p, recs.data(), (size_t)n * sizeof(egg_impulse_record), hipMemcpyHostToDevice));
    HIP_TRY(h, hipStreamSynchronize(Y.stream));  // (no step is running: every step ends with its streams waited for)
    EggImpulseArgs A{};
    for (int w = 0; w < 2; ++w) {
        System &s = h->sys[w];
        A.x[w] = s.x[s.cur].p;
        A.y[w] = s.y[s.cur].p;
        A.vx[w] = s.vx[s.cur].p;
        A.vy[w] = s.vy[s.cur].p;
        A.inv_mass[w] = s.inv_mass.p;
    }
    A.recs = S.d_recs.p;
    A.units = S.units.d_units.p;
    A.n_recs = n;
    A.n_units = S.units.n_units;
    A.need_inv_mass = need_inv_mass ? 1 : 0;
    A.partials = results ? S.partials.p : nullptr;
    if (results)
        hipLaunchKernelGGL(egg_impulse_kernel, dim3((unsigned)waves), dim3(EGG_WAVE), 0, W.stream, A);
    else
        hipLaunchKernelGGL(egg_impulse_quiet_kernel, dim3((unsigned)waves), dim3(EGG_WAVE), 0, W.stream, A);
    HIP_TRY(h, hipGetLastError());
    h->stats.kernel_launches += 1;
    if (!results) {
        HIP_TRY(h, hipStreamSynchronize(W.stream));
        return EGG_OK;
    }
    EggImpulseFinishArgs F{S.partials.p, (int32_t)waves, n, S.out.p};
    hipLaunchKernelGGL(egg_impulse_finish_kernel, dim3(EGG_IM_ROWS), dim3(EGG_IM_FINISH_THREADS), 0, W.stream, F);
    HIP_TRY(h, hipGetLastError());
    h->stats.kernel_launches += 1;
    long long host[EGG_IM_ROWS * EGG_WAVE];
    HIP_TRY(h, hipMemcpyAsync(host, S.out.p, sizeof host, hipMemcpyDeviceToHost, W.stream));
    HIP_TRY(h, hipStreamSynchronize(W.stream));
    // (the finishing kernel writes the entries of the records the list holds, nothing else)
    for (int32_t k = 0; k < n; ++k)
        for (int w = 0; w < 2; ++w) {
            results[k].count[w] = host[(4 * w + 0) * EGG_WAVE + k];
            results[k].sdvx[w] = host[(4 * w + 1) * EGG_WAVE + k];
            results[k].sdvy[w] = host[(4 * w + 2) * EGG_WAVE + k];
            results[k].skipped[w] = host[(4 * w + 3) * EGG_WAVE + k];
        }
    return EGG_OK;
}

}  // extern "C"
