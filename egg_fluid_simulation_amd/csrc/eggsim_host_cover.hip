// eggsim_host_cover.hip -- cover (include/eggsim_cover.h): the checks of a call, the zeroing and the
// preset of the planes and the two launches of eggsim_cover.hip over the unit table of the shared host layer
// (eggsim_host_scan.hip).  egg_cover fills planes the handle reserves and copies every requested plane back once;
// egg_cover_to fills the caller's planes on the device and copies nothing but the totals.  A call stores no grid and no
// answer; a step launches nothing of this and takes no argument from it.
#include "eggsim_host.h"

namespace egghost {

struct CoverState {
    UnitTable units, units_by_key;        // every unit of every type the last call covered, labelled with its batch's id / key
    CoverState() { units_by_key.by_key = true; }
    DevBuf<int32_t> cover;                // egg_cover's planes on the device: [2][ny][nx] each, grown on demand
    DevBuf<uint32_t> owner;
    DevBuf<unsigned long long> totals;    // [EGG_CV_TOTALS]
};

namespace {

// the grid is sized to the device, not to the scene: kWavesPerCu one-wave workgroups per compute unit at the most.  A wave
// holds 16 KB of LDS: 8 of them take 128 KB of the 160 KB of a compute unit.
// (EGGSIM_COVER_WAVES_PER_CU: developer override, 1 .. 32; EGGSIM_COVER_TILE_CELLS: developer override of the tile paths'
// largest union rectangle, 0 .. EGG_CV_TILE_CELLS; EGGSIM_COVER_LANES_CELLS, EGGSIM_COVER_WAVE_CELLS: developer overrides of the
// largest footprint of the lanes path and of the wave path; profiles/r35_cover.md has the sweeps behind the defaults)
constexpr int kWavesPerCu = 8;
int env_cells(const char *name, int most, int otherwise) {
    const char *e = getenv(name);
    return e ? std::min(most, std::max(0, atoi(e))) : otherwise;
}

// Everything is checked before anything is launched or written.  Not cached: every call rasters the arrays
// egg_download_particles would return now.
int cover_call(egg_handle *h, const char *name, const egg_cover_spec *spec, const egg_cover_planes *out, egg_cover_totals *totals,
               bool to_device) {
    static_assert(sizeof(egg_cover_spec) == 48, "a cover spec is 48 bytes");
    static_assert(sizeof(egg_cover_totals) == 112, "the totals are 112 bytes");
    static_assert(sizeof(egg_cover_planes) == 16, "two plane pointers");
    static_assert(EGG_COVER_MAX_SPAN == EGG_CV_MAX_SPAN, "the kernel's span is the ABI's");
    static_assert(EGG_CV_TILE_CELLS * 4 * kWavesPerCu <= (int)kLdsMax && EGG_CV_TILE_CELLS * 4 <= 64 * 1024, "the tiles fit the LDS");
    REJECT_IN_FLIGHT(h, name);
    if (!spec) return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: spec is NULL", name);
    if (!out) return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: planes is NULL", name);
    if (spec->nx < 1 || spec->ny < 1 || (int64_t)spec->nx * spec->ny > EGG_COVER_MAX_CELLS)
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: nx, ny = %d, %d: each is at least 1 and nx * ny at most %d", name, (int)spec->nx,
                    (int)spec->ny, (int)EGG_COVER_MAX_CELLS);
    const double inv = 1.0 / spec->cell;
    if (!std::isfinite(spec->cell) || !(spec->cell > 0.0) || !std::isfinite(inv))
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: cell = %g: it is finite and above 0, and so is its inverse", name, spec->cell);
    if (!std::isfinite(spec->x0) || !std::isfinite(spec->y0))
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: x0, y0 = %g, %g is not finite", name, spec->x0, spec->y0);
    if (!std::isfinite(spec->scale) || !(spec->scale > 0.0))
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: scale = %g: it is finite and above 0", name, spec->scale);
    if (spec->type_mask < 1 || spec->type_mask > 3)
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: type_mask %d (bit 0 white, bit 1 yolk, never 0)", name, (int)spec->type_mask);
    const bool by_key = spec->path >= 0 && (spec->path & EGG_COVER_OWNER_KEYS) != 0;  // (the flag rides on a path, never on a negative word)
    const int path = by_key ? spec->path & ~(int)EGG_COVER_OWNER_KEYS : spec->path;
    if (path < EGG_COVER_PATH_AUTO || path > EGG_COVER_PATH_WAVE)
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: unknown path %d", name, path);
    if (!out->cover) return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: cover is NULL", name);
    // the rectangle of a disc is conservative only while the grid resolves its own coordinates
    const double x1 = spec->x0 + (double)spec->nx * spec->cell, y1 = spec->y0 + (double)spec->ny * spec->cell;
    const double reach = std::max(std::max(std::fabs(spec->x0), std::fabs(spec->y0)), std::max(std::fabs(x1), std::fabs(y1)));
    if (!(reach <= spec->cell * 0x1p20))
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: the grid reaches %g, beyond 2^20 cells of %g: it does not resolve its coordinates", name,
                    reach, spec->cell);
    const bool owner = out->owner != nullptr;
    const size_t words = 2 * (size_t)spec->nx * (size_t)spec->ny, bytes = words * sizeof(int32_t);
    (void)hipSetDevice(h->device);
    if (to_device) {
        if ((uintptr_t)out->cover % 4 != 0 || (uintptr_t)out->owner % 4 != 0)
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: %s is not aligned to 4 bytes", name, (uintptr_t)out->cover % 4 != 0 ? "cover" : "owner");
        if (!device_range_fits(h, out->cover, bytes) || (owner && !device_range_fits(h, out->owner, bytes)))
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: %s is not %zu bytes of memory of device %d", name,
                        !device_range_fits(h, out->cover, bytes) ? "cover" : "owner", bytes, h->device);
    }
    if (owner)
        for (int32_t bi : h->order) {
            const int64_t label = by_key ? h->batches[(size_t)bi].key : h->batches[(size_t)bi].id;
            if (label < 0 || label > (int64_t)std::numeric_limits<int32_t>::max())
                return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: batch %s %lld does not fit the 31 bits of an owner word", name, by_key ? "key" : "id",
                            (long long)label);
        }
    const int types = covered_types(h, spec->type_mask);
    System &W = h->sys[0], &Y = h->sys[1];
    unsigned long long sums[EGG_CV_TOTALS] = {};
    int32_t n_units = 0;
    if (types != 0) {
        int rc = upload_atoms(h);
        if (rc != EGG_OK) return rc;
        if (!h->cover_state) h->cover_state = std::make_shared<CoverState>();
        UnitTable &T = by_key && owner ? h->cover_state->units_by_key : h->cover_state->units;  // (keys matter to the owner plane alone)
        rc = T.refresh(h, name, types, true);
        if (rc != EGG_OK) return rc;
        n_units = T.n_units;
    }
    if (n_units == 0) {  // (nothing to launch: no particles of a type the mask covers)
        if (to_device) {
            HIP_TRY(h, hipMemsetAsync(out->cover, 0, bytes, W.stream));
            if (owner) HIP_TRY(h, hipMemsetAsync(out->owner, 0xFF, bytes, W.stream));
            HIP_TRY(h, hipStreamSynchronize(W.stream));
        } else {
            memset(out->cover, 0, bytes);
            if (owner) memset(out->owner, 0xFF, bytes);
        }
    } else {
        CoverState &S = *h->cover_state;
        EggCoverArgs A{};
        HIP_TRY(h, S.totals.reserve(EGG_CV_TOTALS, false, nullptr));
        if (to_device) {
            A.cover = out->cover;
            A.owner = (uint32_t *)out->owner;
        } else {
            HIP_TRY(h, S.cover.reserve(words, false, nullptr));
            A.cover = S.cover.p;
            if (owner) {
                HIP_TRY(h, S.owner.reserve(words, false, nullptr));
                A.owner = S.owner.p;
            }
        }
        for (int w = 0; w < 2; ++w) {
            System &s = h->sys[w];
            A.x[w] = s.x[s.cur].p;
            A.y[w] = s.y[s.cur].p;
            A.radius[w] = s.radius.p;
        }
        A.units = (by_key && owner ? S.units_by_key : S.units).d_units.p;
        A.n_units = n_units;
        A.nx = spec->nx;
        A.ny = spec->ny;
        const int tile_cells = env_cells("EGGSIM_COVER_TILE_CELLS", EGG_CV_TILE_CELLS, EGG_CV_TILE_CELLS);
        const int most = std::numeric_limits<int32_t>::max();
        const int lanes_cells = env_cells("EGGSIM_COVER_LANES_CELLS", most, EGG_CV_LANES_CELLS);
        const int wave_cells = env_cells("EGGSIM_COVER_WAVE_CELLS", most, EGG_CV_WAVE_CELLS);
        A.tile_cells = path == EGG_COVER_PATH_DIRECT ? 0 : path == EGG_COVER_PATH_AUTO ? tile_cells : EGG_CV_TILE_CELLS;
        A.lanes_cells = path == EGG_COVER_PATH_LANES ? most : path == EGG_COVER_PATH_WAVE ? 0 : lanes_cells;
        A.wave_cells = path == EGG_COVER_PATH_LANES || path == EGG_COVER_PATH_WAVE ? most : wave_cells;
        A.x0 = spec->x0;
        A.y0 = spec->y0;
        A.cell = spec->cell;
        A.inv = inv;
        A.scale = spec->scale;
        A.totals = S.totals.p;
        HIP_TRY(h, hipStreamSynchronize(Y.stream));  // (no step is running: every step ends with its streams waited for)
        // the planes in use and the totals, zeroed or preset on the stream of the launches
        HIP_TRY(h, hipMemsetAsync(A.cover, 0, bytes, W.stream));
        if (owner) HIP_TRY(h, hipMemsetAsync(A.owner, 0xFF, bytes, W.stream));
        HIP_TRY(h, hipMemsetAsync(A.totals, 0, sizeof sums, W.stream));
        const int waves = grid_cap(h, n_units, kWavesPerCu, "EGGSIM_COVER_WAVES_PER_CU");
        hipLaunchKernelGGL(egg_cover_kernel, dim3((unsigned)waves), dim3(EGG_WAVE), 0, W.stream, A);
        HIP_TRY(h, hipGetLastError());
        EggCoverFinishArgs F{};
        F.cover = A.cover;
        F.cells = (int64_t)spec->nx * spec->ny;
        F.totals = A.totals;
        const int blocks = grid_cap(h, (F.cells + EGG_CV_FINISH_THREADS - 1) / EGG_CV_FINISH_THREADS, 4, nullptr);
        hipLaunchKernelGGL(egg_cover_finish_kernel, dim3((unsigned)blocks), dim3(EGG_CV_FINISH_THREADS), 0, W.stream, F);
        HIP_TRY(h, hipGetLastError());
        h->stats.kernel_launches += 2;
        if (!to_device) {  // one copy per requested plane
            HIP_TRY(h, hipMemcpyAsync(out->cover, A.cover, bytes, hipMemcpyDeviceToHost, W.stream));
            if (owner) HIP_TRY(h, hipMemcpyAsync(out->owner, A.owner, bytes, hipMemcpyDeviceToHost, W.stream));
        }
        HIP_TRY(h, hipMemcpyAsync(sums, A.totals, sizeof sums, hipMemcpyDeviceToHost, W.stream));
        HIP_TRY(h, hipStreamSynchronize(W.stream));
    }
    if (totals) {
        for (int w = 0; w < 2; ++w) {
            totals->inside[w] = (int64_t)sums[0 + w];
            totals->outside[w] = (int64_t)sums[2 + w];
            totals->dropped[w] = (int64_t)sums[4 + w];
            totals->hits[w] = (int64_t)sums[6 + w];
            totals->covered[w] = (int64_t)sums[11 + w];
        }
        totals->units_lanes = (int32_t)sums[8];
        totals->units_wave = (int32_t)sums[9];
        totals->units_direct = (int32_t)sums[10];
        totals->reserved = 0;
        totals->covered_both = (int64_t)sums[13];
        totals->covered_any = (int64_t)sums[14];
    }
    return EGG_OK;
}

}  // namespace
}  // namespace egghost

extern "C" {

int egg_cover(egg_handle *h, const egg_cover_spec *spec, const egg_cover_planes *host_planes, egg_cover_totals *totals) {
    if (!h) return EGG_ERR_INVALID_ARGUMENT;
    return cover_call(h, "egg_cover", spec, host_planes, totals, false);
}

int egg_cover_to(egg_handle *h, const egg_cover_spec *spec, const egg_cover_planes *device_planes, egg_cover_totals *totals) {
    if (!h) return EGG_ERR_INVALID_ARGUMENT;
    return cover_call(h, "egg_cover_to", spec, device_planes, totals, true);
}

}  // extern "C"
