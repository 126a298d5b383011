// eggsim_cover.hip -- cover (include/eggsim_cover.h): every committed particle's disc rastered into a
// caller-set grid.  Read-only on the particle arrays; no step launches anything of this file.
//
// A scatter with a data-dependent fan-out: a disc covers between 0 and 130 x 130 cell centres.  Integer addition and the
// unsigned minimum have no order, so any schedule of atomics gives the same bits.  The shape follows what is known of
// global atomics on this chip (profiles/r29_fields.md for integer adds): sum on chip whatever shares a destination, put
// consecutive lanes on consecutive words of a row, never one lane per row.
//
// A workgroup is ONE wave and takes a unit (at most EGG_SN_UNIT consecutive particles of one atom) at a time, so the unit
// and the grid are functions of blockIdx and kernel arguments only and live in scalar registers.  Per unit:
//   1. a first pass over its chunks of 64: every lane classifies its particle (dropped, outside, inside) and computes its
//      rectangle of cells; the wave reduces the union rectangle and the largest footprint; the totals are popcounts of ballots;
//   2. one of three wave-uniform paths:
//      TILE / LANES  the union fits tile_cells and no footprint exceeds lanes_cells: the tile is zeroed in LDS, one lane per
//                    particle walks its own rectangle with LDS integer atomics;
//      TILE / WAVE   the union fits, footprints lie above lanes_cells and within wave_cells (a band that is empty unless a
//                    caller forces the path: profiles/r35_cover.md): the wave takes the chunk's inside particles one after another,
//                    x, y, R and the rectangle broadcast to scalars, the lanes walk that rectangle row-major -- distinct
//                    lanes hold distinct cells, so plain LDS read-modify-writes;
//      DIRECT        the union does not fit, or a footprint exceeds both bounds: the same walk with one global atomicAdd (and atomicMin on the owner plane) per covered (disc, cell);
//   3. a tile is flushed row-major, consecutive lanes on consecutive cells, with one no-return global atomic per non-zero
//      cover word and, a unit having one batch, one atomicMin of its label per owner word under such a cell.
// The totals are wave-uniform registers; lanes 0 .. 10 add them once per wave at the end.  A second small kernel walks the
// finished planes once for covered[2], covered_both and covered_any.
#include <hip/hip_runtime.h>

#include "eggsim_device.h"

namespace {

__device__ __forceinline__ int cv_wave_min(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
    return v;
}

__device__ __forceinline__ int cv_wave_max(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}

__device__ __forceinline__ int cv_wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// the value lane `src` holds, src wave-uniform: a scalar
__device__ __forceinline__ int cv_from_lane(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ double cv_from_lane(double v, int src) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
}

enum { CV_INSIDE = 0, CV_OUTSIDE = 1, CV_DROPPED = 2 };

struct CvDisc {
    double x, y, R;
    int ix0, ix1, iy0, iy1;  // the rectangle of an INSIDE disc: 0 <= ix0 <= ix1 < nx, 0 <= iy0 <= iy1 < ny
};

// the fate and the rectangle of one particle (include/eggsim_cover.h): FP64 in exactly this order, no contraction; every
// comparison is false for a NaN.  The bounds are clamped in double and converted only for an inside disc.
__device__ __forceinline__ int cv_classify(const EggCoverArgs &A, double x, double y, double radius, CvDisc &d) {
    const double R = A.scale * radius;
    d.x = x;
    d.y = y;
    d.R = R;
    d.ix0 = d.iy0 = 0;
    d.ix1 = d.iy1 = -1;
    if (!(isfinite(x) && isfinite(y)) || !(R >= 0.0) || !(R * A.inv <= EGG_CV_MAX_SPAN)) return CV_DROPPED;
    const double fxl = ((x - R) - A.x0) * A.inv, fxh = ((x + R) - A.x0) * A.inv;
    const double fyl = ((y - R) - A.y0) * A.inv, fyh = ((y + R) - A.y0) * A.inv;
    if (fxh < 0.0 || fxl >= (double)A.nx || fyh < 0.0 || fyl >= (double)A.ny) return CV_OUTSIDE;
    d.ix0 = (int)floor(fmax(fxl, 0.0));
    d.ix1 = (int)floor(fmin(fxh, (double)(A.nx - 1)));
    d.iy0 = (int)floor(fmax(fyl, 0.0));
    d.iy1 = (int)floor(fmin(fyh, (double)(A.ny - 1)));
    return CV_INSIDE;
}

// is the centre of cell (ix, iy) covered by the disc (x, y, R)
__device__ __forceinline__ bool cv_covered(const EggCoverArgs &A, int ix, int iy, double x, double y, double R) {
    const double dx = (A.x0 + ((double)ix + 0.5) * A.cell) - x, dy = (A.y0 + ((double)iy + 0.5) * A.cell) - y;
    const double d2 = dx * dx + dy * dy;
    return d2 <= R * R;
}

}  // namespace

extern "C" __global__ void __launch_bounds__(64) egg_cover_kernel(EggCoverArgs A) {
    __shared__ int32_t t_cover[EGG_CV_TILE_CELLS];
    const int lane = (int)threadIdx.x;  // (a workgroup is one wave)
    const int wave = (int)blockIdx.x, n_waves = (int)gridDim.x;
    const size_t plane = (size_t)A.nx * (size_t)A.ny;
    // (wave-uniform)
    long long inside[2] = {0, 0}, outside[2] = {0, 0}, dropped[2] = {0, 0}, hits[2] = {0, 0};
    long long n_lanes = 0, n_wave = 0, n_direct = 0;
    for (int u = wave; u < A.n_units; u += n_waves) {
        const EggScanUnit un = A.units[u];
        const int w = un.type != 0 ? 1 : 0;
        const uint32_t id = (uint32_t)un.reserved;  // the label of the one batch of the unit: its id, or its key
        const double *X = A.x[w] + un.offset, *Y = A.y[w] + un.offset, *Rad = A.radius[w] + un.offset;
        int lo_x = A.nx, hi_x = -1, lo_y = A.ny, hi_y = -1, foot = 0;
        int n_in = 0, n_out = 0, n_drop = 0;
        for (int base = 0; base < un.count; base += EGG_WAVE) {
            const bool live = base + lane < un.count;
            CvDisc d;
            const int fate = cv_classify(A, live ? X[base + lane] : 0.0, live ? Y[base + lane] : 0.0, live ? Rad[base + lane] : 0.0, d);
            const bool in = live && fate == CV_INSIDE;
            n_in += __popcll(__ballot(in));
            n_out += __popcll(__ballot(live && fate == CV_OUTSIDE));
            n_drop += __popcll(__ballot(live && fate == CV_DROPPED));
            if (in) {
                lo_x = min(lo_x, d.ix0);
                hi_x = max(hi_x, d.ix1);
                lo_y = min(lo_y, d.iy0);
                hi_y = max(hi_y, d.iy1);
                foot = max(foot, (d.ix1 - d.ix0 + 1) * (d.iy1 - d.iy0 + 1));  // at most 130 x 130
            }
        }
        inside[w] += n_in;
        outside[w] += n_out;
        dropped[w] += n_drop;
        if (n_in == 0) continue;  // (no particle of the unit is inside: wave-uniform)
        lo_x = cv_wave_min(lo_x);
        hi_x = cv_wave_max(hi_x);
        lo_y = cv_wave_min(lo_y);
        hi_y = cv_wave_max(hi_y);
        foot = cv_wave_max(foot);
        const int rw = hi_x - lo_x + 1, rh = hi_y - lo_y + 1;
        const long long rect = (long long)rw * rh;
        const bool fits = rect <= (long long)A.tile_cells;  // (wave-uniform; tile_cells <= EGG_CV_TILE_CELLS)
        const bool by_lanes = fits && foot <= A.lanes_cells;
        const bool tile = by_lanes || (fits && foot <= A.wave_cells);
        int32_t *const g_cover = A.cover + (size_t)w * plane;
        uint32_t *const g_owner = A.owner ? A.owner + (size_t)w * plane : nullptr;
        if (tile) {
            for (int i = lane; i < (int)rect; i += EGG_WAVE) t_cover[i] = 0;
            __syncthreads();
        }
        int my_hits = 0;
        for (int base = 0; base < un.count; base += EGG_WAVE) {
            const bool live = base + lane < un.count;
            CvDisc d;
            const int fate = cv_classify(A, live ? X[base + lane] : 0.0, live ? Y[base + lane] : 0.0, live ? Rad[base + lane] : 0.0, d);
            const bool in = live && fate == CV_INSIDE;
            if (by_lanes) {
                if (in) {
                    for (int iy = d.iy0; iy <= d.iy1; ++iy)
                        for (int ix = d.ix0; ix <= d.ix1; ++ix)
                            if (cv_covered(A, ix, iy, d.x, d.y, d.R)) {
                                atomicAdd(&t_cover[(iy - lo_y) * rw + (ix - lo_x)], 1);  // in [0, rect): inside the union of these very rectangles
                                ++my_hits;
                            }
                }
                continue;
            }
            // the chunk's inside particles one after another, the whole wave on one rectangle
            for (unsigned long long todo = __ballot(in); todo != 0ull; todo &= todo - 1ull) {
                const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
                const double px = cv_from_lane(d.x, src), py = cv_from_lane(d.y, src), pR = cv_from_lane(d.R, src);
                const int bx0 = cv_from_lane(d.ix0, src), bx1 = cv_from_lane(d.ix1, src);
                const int by0 = cv_from_lane(d.iy0, src), by1 = cv_from_lane(d.iy1, src);
                const int bw = bx1 - bx0 + 1, cells = bw * (by1 - by0 + 1);
                for (int i = lane; i < cells; i += EGG_WAVE) {
                    const int r = i / bw, q = i - r * bw;
                    const int ix = bx0 + q, iy = by0 + r;  // inside [bx0, bx1] x [by0, by1], so inside the grid and the union
                    if (!cv_covered(A, ix, iy, px, py, pR)) continue;
                    ++my_hits;
                    if (tile) {
                        // distinct lanes hold distinct cells within one disc.  The NEXT disc may put another lane on this cell:
                        // that is safe because a workgroup is one wave, the loop over the discs is wave-uniform, and the LDS
                        // operations of one wave complete in program order -- with more than one wave this would need a barrier
                        t_cover[(iy - lo_y) * rw + (ix - lo_x)] += 1;
                    } else {
                        const size_t c = (size_t)iy * (size_t)A.nx + (size_t)ix;  // below plane
                        atomicAdd(&g_cover[c], 1);
                        if (g_owner) atomicMin(&g_owner[c], id);
                    }
                }
            }
        }
        hits[w] += cv_wave_sum(my_hits);
        if (tile) {
            if (by_lanes) ++n_lanes; else ++n_wave;
            __syncthreads();
            // row-major over the union rectangle: consecutive lanes on consecutive cells of a row
            for (int i = lane; i < (int)rect; i += EGG_WAVE) {
                const int32_t n = t_cover[i];
                if (n == 0) continue;
                const int r = i / rw, q = i - r * rw;
                const size_t c = (size_t)(lo_y + r) * (size_t)A.nx + (size_t)(lo_x + q);  // inside [lo, hi], so below plane
                atomicAdd(&g_cover[c], n);
                if (g_owner) atomicMin(&g_owner[c], id);
            }
            __syncthreads();  // (the next unit zeroes the tile)
        } else {
            ++n_direct;
        }
    }
    const long long mine = lane == 0 ? inside[0] : lane == 1 ? inside[1] : lane == 2 ? outside[0] : lane == 3 ? outside[1] :
                           lane == 4 ? dropped[0] : lane == 5 ? dropped[1] : lane == 6 ? hits[0] : lane == 7 ? hits[1] :
                           lane == 8 ? n_lanes : lane == 9 ? n_wave : lane == 10 ? n_direct : 0;
    if (lane < 11 && mine != 0) atomicAdd(&A.totals[lane], (unsigned long long)mine);
}

// covered[2], covered_both, covered_any: one walk over the finished planes, ballots, one atomic per wave and word
extern "C" __global__ void __launch_bounds__(EGG_CV_FINISH_THREADS) egg_cover_finish_kernel(EggCoverFinishArgs A) {
    const int lane = (int)threadIdx.x % EGG_WAVE;
    const int64_t first = ((int64_t)blockIdx.x * EGG_CV_FINISH_THREADS) + (int64_t)((int)threadIdx.x - lane);
    const int64_t stride = (int64_t)gridDim.x * EGG_CV_FINISH_THREADS;
    long long n_white = 0, n_yolk = 0, n_both = 0, n_any = 0;  // (wave-uniform)
    for (int64_t base = first; base < A.cells; base += stride) {
        const int64_t c = base + lane;
        const bool live = c < A.cells;
        const bool a = live && A.cover[c] > 0, b = live && A.cover[A.cells + c] > 0;
        n_white += __popcll(__ballot(a));
        n_yolk += __popcll(__ballot(b));
        n_both += __popcll(__ballot(a && b));
        n_any += __popcll(__ballot(a || b));
    }
    const long long mine = lane == 0 ? n_white : lane == 1 ? n_yolk : lane == 2 ? n_both : lane == 3 ? n_any : 0;
    if (lane < 4 && mine != 0) atomicAdd(&A.totals[11 + lane], (unsigned long long)mine);
}
