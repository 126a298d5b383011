// eggsim_fields.hip -- fields (include/eggsim.h, "fields"): the committed particles binned into a
// caller-set grid.  Read-only on the particle arrays; no step launches anything of this file.
//
// A scatter, not a reduction: the destination of a particle is data.  Integer addition has no order, so any schedule of
// atomic adds gives the same bits -- that is why this kernel may use atomics where the step code may not.  The shape
// follows what is known of global atomics on this chip (measured for FLOAT adds; integer rates are measured for this
// kernel only, profiles/r29_fields.md): sum on chip whatever shares a destination, put consecutive lanes on consecutive
// words of a row, never one lane per row.
//
// A workgroup is ONE wave and takes a unit (at most EGG_SN_UNIT consecutive particles of one atom) at a time, so the unit
// and the grid are functions of blockIdx and kernel arguments only and live in scalar registers.  Per unit:
//   1. a first pass over its chunks of 64: every lane computes its particle's cell, keeps the min and max of ix, iy over
//      the chunks it was inside in, and the wave reduces them once; the outside count is the popcount of a ballot;
//   2. TILE path, if the rectangle [min, max] holds at most tile_cells cells: zero it in LDS, a second pass with LDS
//      integer atomics (count 32 bits, the sums 64), then the lanes walk the rectangle in row-major order, consecutive
//      lanes on consecutive cells, with one no-return device-scope atomicAdd per non-zero word;
//   3. DIRECT path otherwise: one global atomic per inside lane and plane.
// The totals are wave-uniform registers; lanes 0 .. 7 add them once per wave at the end.
#include <hip/hip_runtime.h>

#include "eggsim_device.h"

namespace {

__device__ __forceinline__ int fd_wave_min(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
    return v;
}

__device__ __forceinline__ int fd_wave_max(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}

// the cell of one position (include/eggsim.h): FP64 in exactly this order, no contraction; every comparison is false for a
// NaN.  ix, iy are converted only where the particle is inside: they then lie in [0, nx) x [0, ny).
__device__ __forceinline__ bool fd_cell(const EggFieldArgs &A, double x, double y, int &ix, int &iy) {
    const double fx = (x - A.x0) * A.inv, fy = (y - A.y0) * A.inv;
    const bool in = fx >= 0.0 && fx < (double)A.nx && fy >= 0.0 && fy < (double)A.ny;
    ix = in ? (int)fx : 0;
    iy = in ? (int)fy : 0;
    return in;
}

template <bool VELOCITY>
__device__ __forceinline__ void fd_body(const EggFieldArgs &A) {
    __shared__ int32_t t_count[EGG_FD_TILE_CELLS];
    __shared__ unsigned long long t_svx[VELOCITY ? EGG_FD_TILE_CELLS : 1], t_svy[VELOCITY ? EGG_FD_TILE_CELLS : 1];
    const int lane = (int)threadIdx.x;  // (a workgroup is one wave)
    const int wave = (int)blockIdx.x, n_waves = (int)gridDim.x;
    const size_t plane = (size_t)A.nx * (size_t)A.ny;
    // (wave-uniform)
    long long inside[2] = {0, 0}, outside[2] = {0, 0}, dropped[2] = {0, 0};
    long long tiled = 0, direct = 0;
    for (int u = wave; u < A.n_units; u += n_waves) {
        const EggScanUnit un = A.units[u];
        const int w = un.type != 0 ? 1 : 0;
        const double *X = A.x[w] + un.offset, *Y = A.y[w] + un.offset;
        const double *VX = VELOCITY ? A.vx[w] + un.offset : nullptr, *VY = VELOCITY ? A.vy[w] + un.offset : nullptr;
        int lo_x = A.nx, hi_x = -1, lo_y = A.ny, hi_y = -1;
        int n_out = 0;
        for (int base = 0; base < un.count; base += EGG_WAVE) {
            const bool live = base + lane < un.count;
            const double x = live ? X[base + lane] : 0.0, y = live ? Y[base + lane] : 0.0;
            int ix, iy;
            const bool in = fd_cell(A, x, y, ix, iy) && live;
            n_out += __popcll(__ballot(live && !in));
            if (in) {
                lo_x = min(lo_x, ix);
                hi_x = max(hi_x, ix);
                lo_y = min(lo_y, iy);
                hi_y = max(hi_y, iy);
            }
        }
        outside[w] += n_out;
        lo_x = fd_wave_min(lo_x);
        hi_x = fd_wave_max(hi_x);
        lo_y = fd_wave_min(lo_y);
        hi_y = fd_wave_max(hi_y);
        if (hi_x < lo_x) continue;  // (no particle of the unit is inside: wave-uniform)
        const int rw = hi_x - lo_x + 1, rh = hi_y - lo_y + 1;
        const long long rect = (long long)rw * rh;
        const bool tile = rect <= (long long)A.tile_cells;  // (wave-uniform; tile_cells <= EGG_FD_TILE_CELLS)
        int32_t *const g_count = A.count + (size_t)w * plane;
        unsigned long long *const g_svx = VELOCITY ? A.svx + (size_t)w * plane : nullptr;
        unsigned long long *const g_svy = VELOCITY ? A.svy + (size_t)w * plane : nullptr;
        if (tile) {
            for (int i = lane; i < (int)rect; i += EGG_WAVE) {
                t_count[i] = 0;
                if (VELOCITY) {
                    t_svx[i] = 0ull;
                    t_svy[i] = 0ull;
                }
            }
            __syncthreads();
        }
        int n_in = 0, n_drop = 0;
        for (int base = 0; base < un.count; base += EGG_WAVE) {
            const bool live = base + lane < un.count;
            const double x = live ? X[base + lane] : 0.0, y = live ? Y[base + lane] : 0.0;
            int ix, iy;
            const bool in = fd_cell(A, x, y, ix, iy) && live;
            bool ok = in;
            long long qx = 0, qy = 0;
            if (VELOCITY) {
                const double sx = (in ? VX[base + lane] : 0.0) * EGG_FD_SCALE, sy = (in ? VY[base + lane] : 0.0) * EGG_FD_SCALE;
                ok = in && fabs(sx) < EGG_FD_LIMIT && fabs(sy) < EGG_FD_LIMIT;  // (false for a NaN and for an infinity)
                qx = llrint(ok ? sx : 0.0);
                qy = llrint(ok ? sy : 0.0);
                n_drop += __popcll(__ballot(in && !ok));
            }
            n_in += __popcll(__ballot(ok));
            if (ok && tile) {
                const int i = (iy - lo_y) * rw + (ix - lo_x);  // in [0, rect): lo and hi were taken over these very cells
                atomicAdd(&t_count[i], 1);
                if (VELOCITY) {
                    atomicAdd(&t_svx[i], (unsigned long long)qx);
                    atomicAdd(&t_svy[i], (unsigned long long)qy);
                }
            } else if (ok) {
                const size_t c = (size_t)iy * (size_t)A.nx + (size_t)ix;  // below plane: the particle is inside
                atomicAdd(&g_count[c], 1);
                if (VELOCITY) {
                    atomicAdd(&g_svx[c], (unsigned long long)qx);
                    atomicAdd(&g_svy[c], (unsigned long long)qy);
                }
            }
        }
        inside[w] += n_in;
        dropped[w] += n_drop;
        if (tile) {
            ++tiled;
            __syncthreads();
            // row-major over the rectangle: consecutive lanes on consecutive cells of a row, a wave spans rows where the
            // rectangle is narrower than 64
            for (int i = lane; i < (int)rect; i += EGG_WAVE) {
                const int r = i / rw, q = i - r * rw;
                const size_t c = (size_t)(lo_y + r) * (size_t)A.nx + (size_t)(lo_x + q);  // inside [lo, hi], so below plane
                const int32_t n = t_count[i];
                if (n != 0) atomicAdd(&g_count[c], n);
                if (VELOCITY) {
                    const unsigned long long sx = t_svx[i], sy = t_svy[i];
                    if (sx != 0ull) atomicAdd(&g_svx[c], sx);
                    if (sy != 0ull) atomicAdd(&g_svy[c], sy);
                }
            }
            __syncthreads();  // (the next unit zeroes the tile)
        } else {
            ++direct;
        }
    }
    const long long mine = lane == 0 ? inside[0] : lane == 1 ? inside[1] : lane == 2 ? outside[0] : lane == 3 ? outside[1] :
                           lane == 4 ? dropped[0] : lane == 5 ? dropped[1] : lane == 6 ? tiled : lane == 7 ? direct : 0;
    if (lane < EGG_FD_TOTALS && mine != 0) atomicAdd(&A.totals[lane], (unsigned long long)mine);
}

}  // namespace

extern "C" __global__ void __launch_bounds__(64) egg_field_count_kernel(EggFieldArgs A) { fd_body<false>(A); }

extern "C" __global__ void __launch_bounds__(64) egg_field_velocity_kernel(EggFieldArgs A) { fd_body<true>(A); }
