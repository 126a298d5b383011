// eggsim_measures.hip -- measures (include/eggsim_measure.h): per requested atom (the particles of
// one type of one batch) its counts, the quantised sums of position, mass, momentum and energy, the extremes, and the
// central second moments, the angular momentum and the reach about an origin taken from the first pass.  Read-only on the
// particle arrays; no step launches anything of this file.
//
// One workgroup of EGG_MS_BLOCK threads per row, one launch per call.  The row is a function of blockIdx alone, so it and
// the region sit in scalar registers.  An atom of at most EGG_MS_WAVE_ATOM particles is walked by the first wave alone:
// the other three waves leave at once, and that path holds no barrier.  A larger atom is walked by all four waves, whose
// partials meet in LDS.  Either way the atom is walked TWICE: pass 1 gives the counts, the sums and the extremes, from
// which every thread derives the origin by the one integer division; pass 2 reads the same lines again (they are in L2)
// and gives the central terms.  A lane keeps its accumulators in registers over all its chunks and a wave reduces them
// ONCE per pass.  Lanes 0 .. 23 of the first wave write the record, one word each.  No partials in memory, no finishing
// kernel, no atomics, no scratch.
//
// Sums are two's complement int64 and extremes are taken on the quantised integers: neither has an order, so the record
// does not depend on the schedule.  A lower extreme is kept negated, so that every extreme is a maximum.
#include <hip/hip_runtime.h>

#include "eggsim_device.h"

namespace {

// pass 1: ten sums, five maxima
enum { MS_N = 0, MS_DROPPED, MS_SX, MS_SY, MS_SM, MS_SMX, MS_SMY, MS_SPX, MS_SPY, MS_SE, MS_NLO_X, MS_NLO_Y, MS_HI_X, MS_HI_Y, MS_MAX_V2, MS_P1 };
constexpr int MS_P1_SUMS = MS_NLO_X;
// pass 2: five sums, one maximum
enum { MS_DC = 0, MS_SXX, MS_SXY, MS_SYY, MS_SL, MS_MAX_REACH, MS_P2 };
constexpr int MS_P2_SUMS = MS_MAX_REACH;
constexpr long long MS_LOWEST = (long long)0x8000000000000000ull;
constexpr int MS_WAVES = EGG_MS_BLOCK / EGG_WAVE;

__device__ __forceinline__ long long ms_wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = (long long)((unsigned long long)v + (unsigned long long)__shfl_xor(v, d, 64));
    return v;
}

__device__ __forceinline__ long long ms_wave_max(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const long long o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ long long ms_add(long long a, long long b) { return (long long)((unsigned long long)a + (unsigned long long)b); }

struct MsParticle {
    double x, y, vx, vy, r, m;
    bool measured;
};

// particle i of the row's atom (i < count is the caller's), and whether the call measures it
__device__ __forceinline__ MsParticle ms_load(const EggMeasureArgs &A, int w, int at, bool live) {
    MsParticle p;
    const int i = live ? at : 0;  // (a dead lane loads nothing and is measured by no call)
    p.x = live ? A.x[w][i] : 0.0;
    p.y = live ? A.y[w][i] : 0.0;
    p.vx = live ? A.vx[w][i] : 0.0;
    p.vy = live ? A.vy[w][i] : 0.0;
    p.r = live ? A.radius[w][i] : 0.0;
    p.m = 1.0 / (live ? A.inv_mass[w][i] : 1.0);
    bool in = live;
    if (A.use_region) {  // (uniform over the launch)
        double d2, R;
        in = in && (A.region.type_mask & (1 << w)) && sn_test(A.region, p.x, p.y, d2, R);
    }
    p.measured = in;
    return p;
}

// the thirteen terms of pass 1 in the header's order; true iff every one is below the limit in magnitude (false for a NaN)
__device__ __forceinline__ bool ms_terms1(const MsParticle &p, double f[13]) {
    f[0] = p.x * EGG_MS_SCALE;
    f[1] = p.y * EGG_MS_SCALE;
    f[2] = p.m * EGG_MS_MASS_SCALE;
    f[3] = (p.m * p.x) * EGG_MS_SCALE;
    f[4] = (p.m * p.y) * EGG_MS_SCALE;
    f[5] = (p.m * p.vx) * EGG_MS_SCALE;
    f[6] = (p.m * p.vy) * EGG_MS_SCALE;
    const double v2 = p.vx * p.vx + p.vy * p.vy;
    f[7] = (p.m * v2) * EGG_MS_SCALE;
    f[8] = v2 * EGG_MS_SCALE;
    f[9] = (p.x - p.r) * EGG_MS_SCALE;
    f[10] = (p.y - p.r) * EGG_MS_SCALE;
    f[11] = (p.x + p.r) * EGG_MS_SCALE;
    f[12] = (p.y + p.r) * EGG_MS_SCALE;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 13; ++k) ok = ok && fabs(f[k]) < EGG_MS_LIMIT;
    return ok;
}

// T threads walk the row: T = EGG_WAVE (the first wave alone, no barrier) or EGG_MS_BLOCK (all waves, partials in LDS)
template <int T>
__device__ __forceinline__ void ms_body(const EggMeasureArgs &A, const EggMeasureRow row, long long (*part1)[MS_P1], long long (*part2)[MS_P2]) {
    const int t = (int)threadIdx.x, lane = t & (EGG_WAVE - 1), wave = t / EGG_WAVE;
    const int n = row.count, w = row.type != 0 ? 1 : 0;
    // ---- pass 1
    long long a[MS_P1];
#pragma unroll
    for (int k = 0; k < MS_P1; ++k) a[k] = k < MS_P1_SUMS ? 0 : MS_LOWEST;
    for (int base = 0; base < n; base += T) {
        const int i = base + t;
        const MsParticle p = ms_load(A, w, row.offset + i, i < n);
        double f[13];
        const bool kept = ms_terms1(p, f) && p.measured;
        a[MS_N] += p.measured ? 1 : 0;
        a[MS_DROPPED] += p.measured && !kept ? 1 : 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) a[MS_SX + k] = ms_add(a[MS_SX + k], llrint(kept ? f[k] : 0.0));
        if (kept) {
            const long long v2 = llrint(f[8]), lx = -llrint(f[9]), ly = -llrint(f[10]), hx = llrint(f[11]), hy = llrint(f[12]);
            a[MS_MAX_V2] = v2 > a[MS_MAX_V2] ? v2 : a[MS_MAX_V2];
            a[MS_NLO_X] = lx > a[MS_NLO_X] ? lx : a[MS_NLO_X];
            a[MS_NLO_Y] = ly > a[MS_NLO_Y] ? ly : a[MS_NLO_Y];
            a[MS_HI_X] = hx > a[MS_HI_X] ? hx : a[MS_HI_X];
            a[MS_HI_Y] = hy > a[MS_HI_Y] ? hy : a[MS_HI_Y];
        }
    }
#pragma unroll
    for (int k = 0; k < MS_P1; ++k) a[k] = k < MS_P1_SUMS ? ms_wave_sum(a[k]) : ms_wave_max(a[k]);
    if (T != EGG_WAVE) {
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < MS_P1; ++k) part1[wave][k] = a[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < MS_P1; ++k) {
            long long v = part1[0][k];
#pragma unroll
            for (int q = 1; q < MS_WAVES; ++q) {
                const long long o = part1[q][k];
                v = k < MS_P1_SUMS ? ms_add(v, o) : (o > v ? o : v);
            }
            a[k] = v;
        }
    }
    // ---- the origin: the one integer division (C: truncation toward zero), by every thread alike
    const long long kept_n = a[MS_N] - a[MS_DROPPED];
    const long long ox_q = kept_n > 0 ? a[MS_SX] / kept_n : 0, oy_q = kept_n > 0 ? a[MS_SY] / kept_n : 0;
    const double ox = (double)ox_q / EGG_MS_SCALE, oy = (double)oy_q / EGG_MS_SCALE;
    // ---- pass 2 (workgroup-uniform: kept_n is the same in every thread)
    long long c[MS_P2];
#pragma unroll
    for (int k = 0; k < MS_P2; ++k) c[k] = k < MS_P2_SUMS ? 0 : MS_LOWEST;
    if (kept_n > 0) {
        for (int base = 0; base < n; base += T) {
            const int i = base + t;
            const MsParticle p = ms_load(A, w, row.offset + i, i < n);
            double f[13];
            const bool kept = ms_terms1(p, f) && p.measured;
            const double dx = p.x - ox, dy = p.y - oy;
            const double d2 = dx * dx + dy * dy;
            double g[5];
            g[0] = (dx * dx) * EGG_MS_SCALE;
            g[1] = (dx * dy) * EGG_MS_SCALE;
            g[2] = (dy * dy) * EGG_MS_SCALE;
            g[3] = (p.m * (dx * p.vy - dy * p.vx)) * EGG_MS_SCALE;
            g[4] = (sqrt(d2) + p.r) * EGG_MS_SCALE;
            bool ok = true;
#pragma unroll
            for (int k = 0; k < 5; ++k) ok = ok && fabs(g[k]) < EGG_MS_LIMIT;
            const bool central = kept && ok;
            c[MS_DC] += kept && !ok ? 1 : 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) c[MS_SXX + k] = ms_add(c[MS_SXX + k], llrint(central ? g[k] : 0.0));
            if (central) {
                const long long reach = llrint(g[4]);
                c[MS_MAX_REACH] = reach > c[MS_MAX_REACH] ? reach : c[MS_MAX_REACH];
            }
        }
#pragma unroll
        for (int k = 0; k < MS_P2; ++k) c[k] = k < MS_P2_SUMS ? ms_wave_sum(c[k]) : ms_wave_max(c[k]);
        if (T != EGG_WAVE) {
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < MS_P2; ++k) part2[wave][k] = c[k];
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < MS_P2; ++k) {
                long long v = part2[0][k];
#pragma unroll
                for (int q = 1; q < MS_WAVES; ++q) {
                    const long long o = part2[q][k];
                    v = k < MS_P2_SUMS ? ms_add(v, o) : (o > v ? o : v);
                }
                c[k] = v;
            }
        }
    }
    if (wave != 0) return;
    // ---- the record: every lane of the first wave holds every total; lane k writes word k
    const bool some = kept_n > 0, central = some && kept_n > c[MS_DC];
    long long rec[EGG_MS_FIELDS];
    rec[0] = n;
    rec[1] = a[MS_N];
    rec[2] = a[MS_DROPPED];
#pragma unroll
    for (int k = 0; k < 8; ++k) rec[3 + k] = some ? a[MS_SX + k] : 0;
    rec[11] = some ? -a[MS_NLO_X] : 0;
    rec[12] = some ? -a[MS_NLO_Y] : 0;
    rec[13] = some ? a[MS_HI_X] : 0;
    rec[14] = some ? a[MS_HI_Y] : 0;
    rec[15] = some ? a[MS_MAX_V2] : 0;
    rec[16] = ox_q;
    rec[17] = oy_q;
    rec[18] = some ? c[MS_DC] : 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) rec[19 + k] = central ? c[MS_SXX + k] : 0;
    rec[23] = central ? c[MS_MAX_REACH] : 0;
    long long mine = 0;
#pragma unroll
    for (int k = 0; k < EGG_MS_FIELDS; ++k) mine = lane == k ? rec[k] : mine;
    if (lane < EGG_MS_FIELDS) A.out[(size_t)row.slot * EGG_MS_FIELDS + lane] = mine;
}

}  // namespace

extern "C" __global__ void __launch_bounds__(EGG_MS_BLOCK) egg_measure_kernel(EggMeasureArgs A) {
    __shared__ long long part1[MS_WAVES][MS_P1], part2[MS_WAVES][MS_P2];
    if ((int)blockIdx.x >= A.n_rows) return;
    const EggMeasureRow row = A.rows[blockIdx.x];
    if (row.count <= EGG_MS_WAVE_ATOM) {  // (workgroup-uniform)
        if (threadIdx.x >= EGG_WAVE) return;  // (the path below holds no barrier)
        ms_body<EGG_WAVE>(A, row, part1, part2);
    } else {
        ms_body<EGG_MS_BLOCK>(A, row, part1, part2);
    }
}
