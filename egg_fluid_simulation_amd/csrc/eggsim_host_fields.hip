// eggsim_host_fields.hip -- fields (include/eggsim.h, "fields"): the checks of a call, the zeroing of
// the planes and the one launch of eggsim_fields.hip over the unit table of the shared host layer (eggsim_host_scan.hip).
// egg_field adds into planes the handle reserves and
// copies every requested plane back once; egg_field_to adds into the caller's planes on the device and copies nothing but
// the totals.  A call stores no grid and no answer; a step launches nothing of this and takes no argument from it.
#include "eggsim_host.h"

namespace egghost {

struct FieldState {
    UnitTable units;                      // every unit of every type the last call covered
    DevBuf<int32_t> count;                // egg_field's planes on the device: [2][ny][nx] each, grown on demand
    DevBuf<unsigned long long> svx, svy;
    DevBuf<unsigned long long> totals;    // [EGG_FD_TOTALS]
};

namespace {

// the grid is sized to the device, not to the scene: kWavesPerCu one-wave workgroups per compute unit at the most.  A wave
// of the velocity kernel holds 20 KB of LDS: 8 of them fill the 160 KB of a compute unit.
// (EGGSIM_FIELD_WAVES_PER_CU: developer override, 1 .. 32; EGGSIM_FIELD_TILE_CELLS: developer override of the tile path's
// largest rectangle, 0 .. EGG_FD_TILE_CELLS; profiles/r29_fields.md has the sweeps behind the defaults)
constexpr int kWavesPerCu = 8;
int field_tile_cells() {
    const char *e = getenv("EGGSIM_FIELD_TILE_CELLS");
    return e ? std::min(EGG_FD_TILE_CELLS, std::max(0, atoi(e))) : EGG_FD_TILE_CELLS;
}

// Everything is checked before anything is launched or written.  Not cached: every call measures the arrays
// egg_download_particles would return now.
int field_call(egg_handle *h, const char *name, const egg_field_spec *spec, const egg_field_planes *out, egg_field_totals *totals,
               bool to_device) {
    static_assert(sizeof(egg_field_spec) == 40, "a field spec is 40 bytes");
    static_assert(sizeof(egg_field_totals) == 56, "the totals are 56 bytes");
    static_assert(sizeof(egg_field_planes) == 24, "three plane pointers");
    static_assert(EGG_FIELD_VELOCITY_SCALE == EGG_FD_SCALE, "the kernel's scale is the ABI's");
    static_assert(EGG_FD_TILE_CELLS * (4 + 2 * 8) * kWavesPerCu <= (int)kLdsMax, "the wave cap per compute unit fits its LDS");
    REJECT_IN_FLIGHT(h, name);
    if (!spec) return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: spec is NULL", name);
    if (!out) return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: planes is NULL", name);
    if (spec->nx < 1 || spec->ny < 1 || (int64_t)spec->nx * spec->ny > EGG_FIELD_MAX_CELLS)
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: nx, ny = %d, %d: each is at least 1 and nx * ny at most %d", name, (int)spec->nx,
                    (int)spec->ny, (int)EGG_FIELD_MAX_CELLS);
    const double inv = 1.0 / spec->cell;
    if (!std::isfinite(spec->cell) || !(spec->cell > 0.0) || !std::isfinite(inv))
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: cell = %g: it is finite and above 0, and so is its inverse", name, spec->cell);
    if (!std::isfinite(spec->x0) || !std::isfinite(spec->y0))
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: x0, y0 = %g, %g is not finite", name, spec->x0, spec->y0);
    if (spec->type_mask < 1 || spec->type_mask > 3)
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: type_mask %d (bit 0 white, bit 1 yolk, never 0)", name, (int)spec->type_mask);
    if (spec->path != EGG_FIELD_PATH_AUTO && spec->path != EGG_FIELD_PATH_DIRECT)
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: unknown path %d", name, (int)spec->path);
    if (!out->count) return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: count is NULL", name);
    if ((out->svx == nullptr) != (out->svy == nullptr))
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: svx and svy are given together or not at all", name);
    const bool velocity = out->svx != nullptr;
    const size_t words = 2 * (size_t)spec->nx * (size_t)spec->ny;
    (void)hipSetDevice(h->device);
    if (to_device) {
        if ((uintptr_t)out->count % 4 != 0) return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: count is not aligned to 4 bytes", name);
        if (velocity && ((uintptr_t)out->svx % 8 != 0 || (uintptr_t)out->svy % 8 != 0))
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: %s is not aligned to 8 bytes", name, (uintptr_t)out->svx % 8 != 0 ? "svx" : "svy");
        if (!device_range_fits(h, out->count, words * sizeof(int32_t)))
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: count is not %zu bytes of memory of device %d", name, words * sizeof(int32_t), h->device);
        if (velocity && (!device_range_fits(h, out->svx, words * sizeof(int64_t)) || !device_range_fits(h, out->svy, words * sizeof(int64_t))))
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: %s is not %zu bytes of memory of device %d", name,
                        !device_range_fits(h, out->svx, words * sizeof(int64_t)) ? "svx" : "svy", words * sizeof(int64_t), h->device);
    }
    const int cover = covered_types(h, spec->type_mask);
    System &W = h->sys[0], &Y = h->sys[1];
    unsigned long long sums[EGG_FD_TOTALS] = {0, 0, 0, 0, 0, 0, 0, 0};
    int32_t n_units = 0;
    if (cover != 0) {
        int rc = upload_atoms(h);
        if (rc != EGG_OK) return rc;
        if (!h->field_state) h->field_state = std::make_shared<FieldState>();
        rc = h->field_state->units.refresh(h, name, cover, false);
        if (rc != EGG_OK) return rc;
        n_units = h->field_state->units.n_units;
    }
    if (n_units == 0) {  // (nothing to launch: no particles of a type the mask covers)
        if (to_device) {
            HIP_TRY(h, hipMemsetAsync(out->count, 0, words * sizeof(int32_t), W.stream));
            if (velocity) {
                HIP_TRY(h, hipMemsetAsync(out->svx, 0, words * sizeof(int64_t), W.stream));
                HIP_TRY(h, hipMemsetAsync(out->svy, 0, words * sizeof(int64_t), W.stream));
            }
            HIP_TRY(h, hipStreamSynchronize(W.stream));
        } else {
            memset(out->count, 0, words * sizeof(int32_t));
            if (velocity) {
                memset(out->svx, 0, words * sizeof(int64_t));
                memset(out->svy, 0, words * sizeof(int64_t));
            }
        }
    } else {
        FieldState &S = *h->field_state;
        EggFieldArgs A{};
        HIP_TRY(h, S.totals.reserve(EGG_FD_TOTALS, false, nullptr));
        if (to_device) {
            A.count = out->count;
            A.svx = (unsigned long long *)out->svx;
            A.svy = (unsigned long long *)out->svy;
        } else {
            HIP_TRY(h, S.count.reserve(words, false, nullptr));
            A.count = S.count.p;
            if (velocity) {
                HIP_TRY(h, S.svx.reserve(words, false, nullptr));
                HIP_TRY(h, S.svy.reserve(words, false, nullptr));
                A.svx = S.svx.p;
                A.svy = S.svy.p;
            }
        }
        for (int w = 0; w < 2; ++w) {
            System &s = h->sys[w];
            A.x[w] = s.x[s.cur].p;
            A.y[w] = s.y[s.cur].p;
            A.vx[w] = s.vx[s.cur].p;
            A.vy[w] = s.vy[s.cur].p;
        }
        A.units = S.units.d_units.p;
        A.n_units = n_units;
        A.nx = spec->nx;
        A.ny = spec->ny;
        A.tile_cells = spec->path == EGG_FIELD_PATH_DIRECT ? 0 : field_tile_cells();
        A.x0 = spec->x0;
        A.y0 = spec->y0;
        A.inv = inv;
        A.totals = S.totals.p;
        HIP_TRY(h, hipStreamSynchronize(Y.stream));
        // the planes in use and the totals, zeroed on the stream of the launch
        HIP_TRY(h, hipMemsetAsync(A.count, 0, words * sizeof(int32_t), W.stream));
        if (velocity) {
            HIP_TRY(h, hipMemsetAsync(A.svx, 0, words * sizeof(int64_t), W.stream));
            HIP_TRY(h, hipMemsetAsync(A.svy, 0, words * sizeof(int64_t), W.stream));
        }
        HIP_TRY(h, hipMemsetAsync(A.totals, 0, sizeof sums, W.stream));
        const int waves = grid_cap(h, n_units, kWavesPerCu, "EGGSIM_FIELD_WAVES_PER_CU");
        if (velocity)
            hipLaunchKernelGGL(egg_field_velocity_kernel, dim3((unsigned)waves), dim3(EGG_WAVE), 0, W.stream, A);
        else
            hipLaunchKernelGGL(egg_field_count_kernel, dim3((unsigned)waves), dim3(EGG_WAVE), 0, W.stream, A);
        HIP_TRY(h, hipGetLastError());
        h->stats.kernel_launches += 1;
        if (!to_device) {  // one copy per requested plane
            HIP_TRY(h, hipMemcpyAsync(out->count, A.count, words * sizeof(int32_t), hipMemcpyDeviceToHost, W.stream));
            if (velocity) {
                HIP_TRY(h, hipMemcpyAsync(out->svx, A.svx, words * sizeof(int64_t), hipMemcpyDeviceToHost, W.stream));
                HIP_TRY(h, hipMemcpyAsync(out->svy, A.svy, words * sizeof(int64_t), hipMemcpyDeviceToHost, W.stream));
            }
        }
        HIP_TRY(h, hipMemcpyAsync(sums, A.totals, sizeof sums, hipMemcpyDeviceToHost, W.stream));
        HIP_TRY(h, hipStreamSynchronize(W.stream));
    }
    if (totals) {
        for (int w = 0; w < 2; ++w) {
            totals->inside[w] = (int64_t)sums[0 + w];
            totals->outside[w] = (int64_t)sums[2 + w];
            totals->dropped[w] = (int64_t)sums[4 + w];
        }
        totals->units_tiled = (int32_t)sums[6];
        totals->units_direct = (int32_t)sums[7];
    }
    return EGG_OK;
}

}  // namespace
}  // namespace egghost

extern "C" {

int egg_field(egg_handle *h, const egg_field_spec *spec, const egg_field_planes *host_out, egg_field_totals *totals) {
    if (!h) return EGG_ERR_INVALID_ARGUMENT;
    return field_call(h, "egg_field", spec, host_out, totals, false);
}

int egg_field_to(egg_handle *h, const egg_field_spec *spec, const egg_field_planes *device_out, egg_field_totals *totals) {
    if (!h) return EGG_ERR_INVALID_ARGUMENT;
    return field_call(h, "egg_field_to", spec, device_out, totals, true);
}

}  // extern "C"
