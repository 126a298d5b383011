// eggsim_host_sensors.hip -- sensors (include/eggsim.h, "sensors"): the list, the check of a region
// record, the per-batch unit table and the launches of eggsim_sensors.hip, over the shared host layer of
// eggsim_host_scan.hip (the unit table of the totals, the grid cap, the id list).  A read is two launches on the white
// stream and one copy back; a step launches nothing of this and takes no argument from it.
#include "eggsim_host.h"

namespace egghost {

struct SensorState {
    DevBuf<EggSensor> d_sensors;        // written when the list is set, never per read
    UnitTable units;                    // the totals': every unit of every type some sensor covers
    DevBuf<long long> partials, out;
    // the per-batch read: built for the listed ids of every call
    DevBuf<EggSensorUnit> d_batch_units;
    DevBuf<int32_t> unit_counts, rows, counts;
};

// The checks and the normalisation of one region record (include/eggsim.h, "sensors"): the rule of egg_set_sensors, shared
// with every caller that takes regions.  `what` opens the message, k is the record's index.
int check_region(egg_handle *h, const char *what, int32_t k, egg_region &o) {
    static const char *const names[4] = {"half-plane", "disc", "box", "capsule"};
    static const int used_of[4] = {3, 3, 6, 5};
    if (o.kind < EGG_SENSOR_HALF_PLANE || o.kind > EGG_SENSOR_CAPSULE)
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s %d: unknown kind %d", what, (int)k, (int)o.kind);
    if (o.type_mask < 1 || o.type_mask > 3)
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s %d: type_mask %d (bit 0 white, bit 1 yolk, never 0)", what, (int)k,
                    (int)o.type_mask);
    for (int q = 0; q < 6; ++q) {
        if (q >= used_of[o.kind]) o.p[q] = 0.0;  // (not a parameter of the kind)
        if (!std::isfinite(o.p[q]))
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s %d (%s): parameter %d is not finite", what, (int)k, names[o.kind], q);
    }
    if (o.kind == EGG_SENSOR_DISC && o.p[2] < 0)
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s %d (disc): radius %g is negative", what, (int)k, o.p[2]);
    if (o.kind == EGG_SENSOR_CAPSULE && o.p[4] < 0)
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s %d (capsule): radius %g is negative", what, (int)k, o.p[4]);
    if (o.kind == EGG_SENSOR_BOX && (o.p[2] < 0 || o.p[3] < 0))
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s %d (box): half extent (%g, %g) is negative", what, (int)k, o.p[2], o.p[3]);
    if (o.kind == EGG_SENSOR_HALF_PLANE || o.kind == EGG_SENSOR_BOX) {  // normalised once, here, as a collider's normal is
        double *v = o.kind == EGG_SENSOR_BOX ? o.p + 4 : o.p;
        const double len = std::sqrt(v[0] * v[0] + v[1] * v[1]);
        if (!(len >= h->sys[0].cfg.eps) || !std::isfinite(len))
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s %d (%s): the %s's length %g is below eps or not finite", what, (int)k,
                        names[o.kind], o.kind == EGG_SENSOR_BOX ? "axis" : "normal", len);
        v[0] = v[0] / len;
        v[1] = v[1] / len;
    }
    return EGG_OK;
}

namespace {

// bit w: some sensor's mask covers type w and the type has particles
int sensor_cover(const egg_handle *h) {
    int cover = 0;
    for (const egg_sensor &s : h->sensors) cover |= s.type_mask;
    return covered_types(h, cover);
}

// the grid is sized to the device, not to the scene: kWavesPerCu one-wave workgroups per compute unit at the most
// (EGGSIM_SENSOR_WAVES_PER_CU: developer override, 1 .. 32; profiles/r27_sensors.md has the sweep behind the default)
constexpr int kWavesPerCu = 8;
int sensor_waves(const egg_handle *h, int64_t n_units) { return grid_cap(h, n_units, kWavesPerCu, "EGGSIM_SENSOR_WAVES_PER_CU"); }

void sensor_args(egg_handle *h, SensorState &S, EggSensorArgs &A) {
    A = EggSensorArgs{};
    for (int w = 0; w < 2; ++w) {
        System &s = h->sys[w];
        A.x[w] = s.x[s.cur].p;
        A.y[w] = s.y[s.cur].p;
    }
    A.sensors = S.d_sensors.p;
    A.n_sensors = (int32_t)h->sensors.size();
}

}  // namespace
}  // namespace egghost

extern "C" {

// Everything is checked before anything changes: a refused call leaves the list and its device copy as they were.
int egg_set_sensors(egg_handle *h, int32_t n, const egg_sensor *sensors) {
    if (!h) return EGG_ERR_INVALID_ARGUMENT;
    REJECT_IN_FLIGHT(h, "egg_set_sensors");
    static_assert(sizeof(egg_sensor) == 56 && sizeof(EggSensor) == sizeof(egg_sensor), "a sensor record is 56 bytes");
    static_assert(sizeof(egg_sensor_reading) == 48, "a reading is 48 bytes");
    static_assert(EGG_MAX_SENSORS == EGG_SN_MAX_SENSORS && EGG_SN_MAX_SENSORS == EGG_WAVE, "one lane of a wave per sensor");
    static_assert(EGG_SENSOR_POSITION_SCALE == EGG_SN_SCALE, "the kernel's scale is the ABI's");
    static_assert(EGG_SENSOR_HALF_PLANE == EGG_SN_HALF_PLANE && EGG_SENSOR_DISC == EGG_SN_DISC && EGG_SENSOR_BOX == EGG_SN_BOX &&
                      EGG_SENSOR_CAPSULE == EGG_SN_CAPSULE,
                  "the kernel's sensor kinds are the ABI's");
    if (n < 0 || n > EGG_MAX_SENSORS)
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_set_sensors: n = %d, a list holds 0 .. %d sensors", (int)n, EGG_MAX_SENSORS);
    if (n > 0 && !sensors) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_set_sensors: n = %d without a list", (int)n);
    std::vector<egg_sensor> list((size_t)n);
    for (int32_t k = 0; k < n; ++k) {
        egg_sensor &o = list[(size_t)k];
        o = sensors[k];
        const int rc = check_region(h, "egg_set_sensors: sensor", k, o);
        if (rc != EGG_OK) return rc;
    }
    if (n > 0) {  // (no step is running: every step ends with its streams waited for)
        HIP_TRY(h, hipSetDevice(h->device));
        if (!h->sensor_state) h->sensor_state = std::make_shared<SensorState>();
        HIP_TRY(h, h->sensor_state->d_sensors.reserve(EGG_MAX_SENSORS, false, nullptr));
        HIP_TRY(h, hipMemcpy(h->sensor_state->d_sensors.p, list.data(), (size_t)n * sizeof(egg_sensor), hipMemcpyHostToDevice));
    }
    h->sensors.swap(list);
    return EGG_OK;
}

int egg_get_sensors(const egg_handle *h, int32_t cap, egg_sensor *out, int32_t *n) {
    if (!h) return EGG_ERR_INVALID_ARGUMENT;
    const int32_t have = (int32_t)h->sensors.size();
    if (n) *n = have;
    if (out && cap > 0) memcpy(out, h->sensors.data(), (size_t)std::min(cap, have) * sizeof(egg_sensor));
    return EGG_OK;
}

// Not cached: every call measures the arrays egg_download_particles would return now.
int egg_read_sensors(egg_handle *h, int32_t cap, egg_sensor_reading *readings, int64_t dropped[2], int32_t *n) {
    if (!h) return EGG_ERR_INVALID_ARGUMENT;
    REJECT_IN_FLIGHT(h, "egg_read_sensors");
    const int32_t have = (int32_t)h->sensors.size();
    if (n) *n = have;
    if (dropped) dropped[0] = dropped[1] = 0;
    const int32_t give = readings ? std::min(std::max(cap, 0), have) : 0;
    if (give > 0) memset(readings, 0, (size_t)give * sizeof(egg_sensor_reading));
    if (have == 0) return EGG_OK;
    (void)hipSetDevice(h->device);
    {
        const int rc = upload_atoms(h);
        if (rc != EGG_OK) return rc;
    }
    const int cover = sensor_cover(h);
    if (cover == 0) return EGG_OK;  // (nothing to launch: no particles, or no sensor covers a type that has some)
    SensorState &S = *h->sensor_state;
    System &W = h->sys[0], &Y = h->sys[1];
    {
        const int rc = S.units.refresh(h, "egg_read_sensors", cover, false);
        if (rc != EGG_OK) return rc;
    }
    if (S.units.n_units == 0) return EGG_OK;
    const int waves = sensor_waves(h, S.units.n_units);
    HIP_TRY(h, S.partials.reserve((size_t)waves * EGG_SN_ROWS * EGG_WAVE, false, nullptr));
    HIP_TRY(h, S.out.reserve((size_t)EGG_SN_ROWS * EGG_WAVE, false, nullptr));
    HIP_TRY(h, hipStreamSynchronize(Y.stream));
    EggSensorArgs A;
    sensor_args(h, S, A);
    A.units = S.units.d_units.p;
    A.n_units = S.units.n_units;
    A.partials = S.partials.p;
    hipLaunchKernelGGL(egg_sensor_sums_kernel, dim3((unsigned)waves), dim3(EGG_WAVE), 0, W.stream, A);
    HIP_TRY(h, hipGetLastError());
    EggSensorFinishArgs F{S.partials.p, (int32_t)waves, have, S.out.p};
    hipLaunchKernelGGL(egg_sensor_finish_kernel, dim3(EGG_SN_ROWS), dim3(EGG_SN_FINISH_THREADS), 0, W.stream, F);
    HIP_TRY(h, hipGetLastError());
    h->stats.kernel_launches += 2;
    long long host[EGG_SN_ROWS * EGG_WAVE];
    HIP_TRY(h, hipMemcpyAsync(host, S.out.p, sizeof host, hipMemcpyDeviceToHost, W.stream));
    HIP_TRY(h, hipStreamSynchronize(W.stream));
    // (the finishing kernel writes the entries of the sensors the list holds and the dropped pair, nothing else)
    for (int32_t k = 0; k < give; ++k)
        for (int w = 0; w < 2; ++w) {
            readings[k].count[w] = host[(3 * w + 0) * EGG_WAVE + k];
            readings[k].sx[w] = host[(3 * w + 1) * EGG_WAVE + k];
            readings[k].sy[w] = host[(3 * w + 2) * EGG_WAVE + k];
        }
    if (dropped) {
        dropped[0] = host[6 * EGG_WAVE + 0];
        dropped[1] = host[6 * EGG_WAVE + 1];
    }
    return EGG_OK;
}

int egg_read_sensor_batches(egg_handle *h, int64_t n_ids, const int64_t *ids, int32_t *counts) {
    if (!h || n_ids < 0 || (n_ids > 0 && !ids)) return EGG_ERR_INVALID_ARGUMENT;
    REJECT_IN_FLIGHT(h, "egg_read_sensor_batches");
    {  // (before anything is written)
        const int rc = check_batch_ids(h, "egg_read_sensor_batches", n_ids, ids);
        if (rc != EGG_OK) return rc;
    }
    const int32_t have = (int32_t)h->sensors.size();
    if (n_ids == 0 || have == 0) return EGG_OK;
    if (!counts) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_read_sensor_batches: counts is NULL");
    if (n_ids > (int64_t)(std::numeric_limits<int32_t>::max() / (2 * EGG_WAVE)))
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_read_sensor_batches: %lld ids in one call", (long long)n_ids);
    const size_t words = (size_t)n_ids * (size_t)have * 2;
    memset(counts, 0, words * sizeof(int32_t));
    (void)hipSetDevice(h->device);
    {
        const int rc = upload_atoms(h);
        if (rc != EGG_OK) return rc;
    }
    const int cover = sensor_cover(h);
    if (cover == 0) return EGG_OK;
    SensorState &S = *h->sensor_state;
    System &W = h->sys[0], &Y = h->sys[1];
    // a batch listed twice has its units once and two rows that point at them
    const std::vector<int32_t> atom_of = atom_of_batch(h);
    std::vector<int32_t> first_of_atom[2];
    std::vector<EggSensorUnit> units;
    std::vector<int32_t> rows(4 * (size_t)n_ids, 0);  // [2 n_ids] first unit, then [2 n_ids] unit count
    for (int w = 0; w < 2; ++w) first_of_atom[w].assign(h->sys[w].atoms.size(), -1);
    for (int64_t i = 0; i < n_ids; ++i) {
        const int32_t a = atom_of[(size_t)ids[i] - 1];
        for (int w = 0; w < 2; ++w) {
            if (!(cover >> w & 1) || a < 0) continue;
            const Atom &at = h->sys[w].atoms[(size_t)a];
            if (first_of_atom[w][(size_t)a] < 0) {
                first_of_atom[w][(size_t)a] = (int32_t)units.size();
                push_units(at, w, units);
            }
            rows[(size_t)(2 * i + w)] = first_of_atom[w][(size_t)a];
            rows[(size_t)(2 * n_ids + 2 * i + w)] = (at.count + EGG_SN_UNIT - 1) / EGG_SN_UNIT;
        }
    }
    if (units.empty()) return EGG_OK;
    const int waves = sensor_waves(h, (int64_t)units.size());
    HIP_TRY(h, S.d_batch_units.reserve(units.size(), false, nullptr));
    HIP_TRY(h, S.unit_counts.reserve(units.size() * EGG_WAVE, false, nullptr));
    HIP_TRY(h, S.rows.reserve(rows.size(), false, nullptr));
    HIP_TRY(h, S.counts.reserve(words, false, nullptr));
    HIP_TRY(h, hipMemcpy(S.d_batch_units.p, units.data(), units.size() * sizeof(EggSensorUnit), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(S.rows.p, rows.data(), rows.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(h, hipStreamSynchronize(Y.stream));
    EggSensorArgs A;
    sensor_args(h, S, A);
    A.units = S.d_batch_units.p;
    A.n_units = (int32_t)units.size();
    A.unit_counts = S.unit_counts.p;
    hipLaunchKernelGGL(egg_sensor_units_kernel, dim3((unsigned)waves), dim3(EGG_WAVE), 0, W.stream, A);
    HIP_TRY(h, hipGetLastError());
    EggSensorBatchFinishArgs F{S.unit_counts.p, S.rows.p, S.rows.p + 2 * n_ids, (int32_t)(2 * n_ids), have, S.counts.p};
    const long long threads = 2 * (long long)n_ids * have;
    hipLaunchKernelGGL(egg_sensor_batch_finish_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, W.stream, F);
    HIP_TRY(h, hipGetLastError());
    h->stats.kernel_launches += 2;
    HIP_TRY(h, hipMemcpyAsync(counts, S.counts.p, words * sizeof(int32_t), hipMemcpyDeviceToHost, W.stream));
    HIP_TRY(h, hipStreamSynchronize(W.stream));
    return EGG_OK;
}

}  // extern "C"
