// eggsim_host_measures.hip -- measures (include/eggsim_measure.h): the checks of a call, the row
// table and the one launch of eggsim_measures.hip, over the shared host layer of eggsim_host_scan.hip (the id list, the walk
// over its atoms, the test of the caller's device memory).  A call copies one row table up (none when the atoms, the mask and the
// id list are those of the last call) and, for egg_measure, the records back once; egg_measure_to leaves them in the
// caller's memory on the device.  It stores no answer; a step launches nothing of this and takes no argument from it.
#include "eggsim_host.h"

namespace egghost {

struct MeasureState {
    DevBuf<EggMeasureRow> d_rows;    // one row per requested (id, type) that has particles
    DevBuf<long long> d_out;         // egg_measure's records on the device: [2 n][EGG_MS_FIELDS]
    // what the table on the device was built from: it is kept while the atoms, the mask and the list stand
    uint64_t rows_gen[2] = {~0ull, ~0ull};
    int rows_mask = -1;
    bool rows_all = false;
    std::vector<int64_t> rows_ids;
    int32_t n_rows = 0;
};

namespace {

// Everything is checked before anything is launched or written.  Not cached: every call measures the arrays
// egg_download_particles would return now.
int measure_call(egg_handle *h, const char *name, const egg_measure_spec *spec, int64_t n_ids, const int64_t *ids, void *out,
                 int64_t capacity_bytes, bool to_device) {
    static_assert(sizeof(egg_measure_spec) == 64 && offsetof(egg_measure_spec, flags) == 56, "a measure spec is 64 bytes");
    static_assert(sizeof(egg_measure_record) == 192 && EGG_MS_FIELDS * sizeof(long long) == sizeof(egg_measure_record), "a record is 24 int64");
    static_assert(EGG_MEASURE_FIELDS == EGG_MS_FIELDS && EGG_MEASURE_REGION == EGG_MS_REGION, "the kernel's record and flag are the ABI's");
    static_assert(EGG_MEASURE_SCALE == EGG_MS_SCALE && EGG_MEASURE_MASS_SCALE == EGG_MS_MASS_SCALE, "the kernel's scales are the ABI's");
    static_assert(sizeof(EggRegion) == sizeof(egg_region), "a region is a region");
    REJECT_IN_FLIGHT(h, name);
    if (!spec) return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: spec is NULL", name);
    if (!out) return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: out is NULL", name);
    if (n_ids < 0 || (n_ids > 0 && !ids))
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: n_ids = %lld %s a list (0 and NULL mean every live batch)", name, (long long)n_ids,
                    ids ? "with" : "without");
    if (spec->flags & ~EGG_MEASURE_REGION) return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: unknown flag bits %d", name, (int)spec->flags);
    if (spec->type_mask < 1 || spec->type_mask > 3)
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: type_mask %d (bit 0 white, bit 1 yolk, never 0)", name, (int)spec->type_mask);
    const bool use_region = (spec->flags & EGG_MEASURE_REGION) != 0;
    egg_region region = spec->region;
    if (use_region) {
        const std::string what = std::string(name) + ": region";
        const int rc = check_region(h, what.c_str(), 0, region);
        if (rc != EGG_OK) return rc;
    }
    int rc = check_batch_ids(h, name, n_ids, ids);
    if (rc != EGG_OK) return rc;
    const bool all = n_ids == 0 && !ids;
    std::vector<int64_t> every;
    if (all) {
        every = live_batch_ids(h);
        ids = every.data();
        n_ids = (int64_t)every.size();
    }
    if (n_ids > (int64_t)(std::numeric_limits<int32_t>::max() / 4))
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: %lld ids in one call", name, (long long)n_ids);
    const size_t words = 2 * (size_t)n_ids * EGG_MS_FIELDS, bytes = words * sizeof(long long);
    (void)hipSetDevice(h->device);
    if (to_device) {
        if ((uintptr_t)out % 8 != 0) return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: device_out is not aligned to 8 bytes", name);
        if (capacity_bytes < 0 || (uint64_t)capacity_bytes < (uint64_t)bytes)
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: capacity_bytes = %lld, %lld batches take %zu", name, (long long)capacity_bytes,
                        (long long)n_ids, bytes);
        if (!device_range_fits(h, out, bytes))
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: device_out is not %zu bytes of memory of device %d", name, bytes, h->device);
    }
    if (n_ids == 0) return EGG_OK;  // (an empty list, or no live batch: nothing to launch and nothing to write)
    System &W = h->sys[0], &Y = h->sys[1];
    rc = upload_atoms(h);
    if (rc != EGG_OK) return rc;
    if (!h->measure_state) h->measure_state = std::make_shared<MeasureState>();
    MeasureState &S = *h->measure_state;
    const bool cached = S.rows_gen[0] == W.atoms_gen && S.rows_gen[1] == Y.atoms_gen && S.rows_mask == spec->type_mask && S.rows_all == all &&
                        (all || (S.rows_ids.size() == (size_t)n_ids && std::equal(S.rows_ids.begin(), S.rows_ids.end(), ids)));
    if (!cached) {
        S.rows_gen[0] = S.rows_gen[1] = ~0ull;  // (until the table below is complete)
        std::vector<EggMeasureRow> rows;
        rc = for_each_requested_atom(h, name, spec->type_mask, n_ids, ids, [&](const Atom &at, int w, int32_t slot) {
            rows.push_back(EggMeasureRow{at.offset, at.count, w, slot});
            return (int)EGG_OK;
        });
        if (rc != EGG_OK) return rc;
        HIP_TRY(h, S.d_rows.reserve(rows.size(), false, nullptr));
        if (!rows.empty()) HIP_TRY(h, hipMemcpy(S.d_rows.p, rows.data(), rows.size() * sizeof(EggMeasureRow), hipMemcpyHostToDevice));
        S.n_rows = (int32_t)rows.size();
        S.rows_mask = spec->type_mask;
        S.rows_all = all;
        if (all) S.rows_ids.clear(); else S.rows_ids.assign(ids, ids + n_ids);
        S.rows_gen[0] = W.atoms_gen;
        S.rows_gen[1] = Y.atoms_gen;
    }
    long long *table = (long long *)out;
    if (!to_device) {
        HIP_TRY(h, S.d_out.reserve(words, false, nullptr));
        table = S.d_out.p;
    }
    HIP_TRY(h, hipStreamSynchronize(Y.stream));  // (no step is running: every step ends with its streams waited for)
    // a record without a row -- a type the mask leaves out or the batch lacks -- is 0: the table is zeroed unless every record has a row
    if ((size_t)S.n_rows != 2 * (size_t)n_ids) HIP_TRY(h, hipMemsetAsync(table, 0, bytes, W.stream));
    if (S.n_rows > 0) {
        EggMeasureArgs A{};
        for (int w = 0; w < 2; ++w) {
            System &s = h->sys[w];
            A.x[w] = s.x[s.cur].p;
            A.y[w] = s.y[s.cur].p;
            A.vx[w] = s.vx[s.cur].p;
            A.vy[w] = s.vy[s.cur].p;
            A.radius[w] = s.radius.p;
            A.inv_mass[w] = s.inv_mass.p;
        }
        A.rows = S.d_rows.p;
        A.n_rows = S.n_rows;
        A.use_region = use_region ? 1 : 0;
        memcpy(&A.region, &region, sizeof region);
        A.out = table;
        hipLaunchKernelGGL(egg_measure_kernel, dim3((unsigned)S.n_rows), dim3(EGG_MS_BLOCK), 0, W.stream, A);
        HIP_TRY(h, hipGetLastError());
        h->stats.kernel_launches += 1;
    }
    if (!to_device) HIP_TRY(h, hipMemcpyAsync(out, table, bytes, hipMemcpyDeviceToHost, W.stream));
    HIP_TRY(h, hipStreamSynchronize(W.stream));
    return EGG_OK;
}

}  // namespace
}  // namespace egghost

extern "C" {

int egg_measure(egg_handle *h, const egg_measure_spec *spec, int64_t n_ids, const int64_t *ids, egg_measure_record *out) {
    if (!h) return EGG_ERR_INVALID_ARGUMENT;
    return measure_call(h, "egg_measure", spec, n_ids, ids, out, 0, false);
}

int egg_measure_to(egg_handle *h, const egg_measure_spec *spec, int64_t n_ids, const int64_t *ids, void *device_out, int64_t capacity_bytes) {
    if (!h) return EGG_ERR_INVALID_ARGUMENT;
    return measure_call(h, "egg_measure_to", spec, n_ids, ids, device_out, capacity_bytes, true);
}

}  // extern "C"
