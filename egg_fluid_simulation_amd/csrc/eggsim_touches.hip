// eggsim_touches.hip -- touches (include/eggsim_touch.h): which batches touch which, how much and
// where.  Read-only on the particle arrays; no step launches anything of this file.
//
// The queries of a call are taken in rounds of at most EGG_TC_ROUND.  egg_touch_gather_kernel (one wave per query) copies a
// round's discs -- from the handle's own arrays or from the caller's uploaded discs -- into one table with their quantised
// coordinates and their dropped flag, and leaves per query the box of its centres and its largest radius.  The scan then has
// one input form.
//
// egg_touch_kernel: a workgroup is ONE wave and takes a unit (at most EGG_SN_UNIT consecutive particles of one atom, so of one
// batch and one type) at a time.  A lane keeps its up to EGG_TC_OWN particles in registers, particle j * 64 + lane in place
// j; a wave reduction gives the box of the unit's centres and its largest radius.  Lane k tests query k -- same type,
// another batch, boxes not apart -- and a ballot yields the candidate queries.  Per candidate a wave-uniform loop walks the
// query's discs: the disc is a uniform value (a scalar load, as eggsim_impulses.hip reads its records), every lane tests its
// own particles and keeps pairs, a 16-bit touched mask, dropped and the two sums.  A ballot of pairs != 0 decides whether
// the wave reductions run at all; lane 0 then takes a slot from the one global cursor and writes one partial record if the
// slot lies inside the buffer.  The cursor keeps counting past the end: the host runs the call once more with the buffer the
// first run asked for.  The host adds the partial records of one (slot, other) and sorts, so the order of the cursor is no
// part of any answer.  FP64 and integers only; no LDS, no scratch, no global atomic but the cursor (and, where a developer asks
// for it, one counter of the candidates).
#include <hip/hip_runtime.h>

#include "eggsim_device.h"

namespace {

__device__ __forceinline__ double tc_wave_min(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmin(v, __shfl_xor(v, d, 64));  // (fmin, fmax pass over a NaN)
    return v;
}

__device__ __forceinline__ double tc_wave_max(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_xor(v, d, 64));
    return v;
}

__device__ __forceinline__ int tc_wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ unsigned long long tc_wave_sum(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (unsigned long long)__shfl_xor((long long)v, d, 64);
    return v;
}

// THE CULL.  It may only skip what the rule rejects.  Two sets of discs A and B, the centres of A (every coordinate that is
// not a NaN) inside the box [a_lo, a_hi], those of B inside [b_lo, b_hi], every |r| of A at most ra and of B at most rb,
// are APART when in x or in y the gap g = fl(a_lo - b_hi) or g = fl(b_lo - a_hi) is above 0 and fl(g * g) > fl(Lmax * Lmax),
// Lmax = fl(reach * fl(ra + rb)).  No pair of sets that are apart touches:
//   - say g = fl(a_lo - b_hi) > 0 in x.  For a pair without a NaN, xa >= a_lo and xb <= b_hi, so xa - xb >= a_lo - b_hi and,
//     rounding being monotone, dx = fl(xa - xb) >= g > 0, hence fl(dx * dx) >= fl(g * g);
//   - fl(dy * dy) >= 0, so d2 = fl(fl(dx * dx) + fl(dy * dy)) >= fl(dx * dx): fl(dx * dx) <= fl(d2);
//   - |fl(ra' + rb')| <= fl(ra + rb) for the pair's own radii, reach > 0, so |L| <= Lmax and fl(L * L) <= fl(Lmax * Lmax);
//   - a touch needs fl(d2) <= fl(L * L), so fl(g * g) <= fl(Lmax * Lmax): the sets were not apart.
// A comparison with a NaN is false and falls to "not apart"; so does an overflow on both sides (inf > inf is false).  A pair
// with a NaN in it does not touch, so a NaN may stay outside the boxes and the radii; a set without a box touches nothing
// and is passed over before this test.  The tests hold the answers equal to the model, which has no cull.
__device__ __forceinline__ bool tc_apart_1d(double a_lo, double a_hi, double b_lo, double b_hi, double L2) {
    const double g0 = a_lo - b_hi, g1 = b_lo - a_hi;
    return (g0 > 0.0 && g0 * g0 > L2) || (g1 > 0.0 && g1 * g1 > L2);
}

__device__ __forceinline__ bool tc_apart(double a_lo_x, double a_lo_y, double a_hi_x, double a_hi_y, double ra, double b_lo_x, double b_lo_y,
                                         double b_hi_x, double b_hi_y, double rb, double reach) {
    const double Lmax = reach * (ra + rb);
    const double L2 = Lmax * Lmax;
    return tc_apart_1d(a_lo_x, a_hi_x, b_lo_x, b_hi_x, L2) || tc_apart_1d(a_lo_y, a_hi_y, b_lo_y, b_hi_y, L2);
}

}  // namespace

// one wave per query of the round: its discs into the table, its box and its largest radius into its header
extern "C" __global__ void __launch_bounds__(64) egg_touch_gather_kernel(EggTouchGatherArgs A) {
    const int lane = (int)threadIdx.x;
    const int q = (int)blockIdx.x;
    if (q >= A.n_queries) return;
    const EggTouchSource s = A.sources[q];
    const int w = s.type != 0 ? 1 : 0;
    const double *X = A.x[w] + s.offset, *Y = A.y[w] + s.offset, *R = A.r[w] + s.offset;
    EggTouchDisc *D = A.discs + s.first;
    const double inf = __builtin_huge_val();
    double lo_x = inf, lo_y = inf, hi_x = -inf, hi_y = -inf, rmax = 0.0;
    for (int i = lane; i < s.count; i += EGG_WAVE) {
        const double x = X[i], y = Y[i], r = R[i];
        const double fx = x * EGG_SN_SCALE, fy = y * EGG_SN_SCALE;
        const bool ok = fabs(fx) < EGG_SN_LIMIT && fabs(fy) < EGG_SN_LIMIT;  // (false for a NaN and for an infinity)
        EggTouchDisc d;
        d.x = x;
        d.y = y;
        d.r = r;
        d.qx = llrint(ok ? fx : 0.0);
        d.qy = llrint(ok ? fy : 0.0);
        d.dropped = ok ? 0 : 1;
        D[i] = d;
        lo_x = fmin(lo_x, x);
        hi_x = fmax(hi_x, x);
        lo_y = fmin(lo_y, y);
        hi_y = fmax(hi_y, y);
        rmax = fmax(rmax, fabs(r));
    }
    lo_x = tc_wave_min(lo_x);
    lo_y = tc_wave_min(lo_y);
    hi_x = tc_wave_max(hi_x);
    hi_y = tc_wave_max(hi_y);
    rmax = tc_wave_max(rmax);
    if (lane != 0) return;
    EggTouchQuery o;
    o.first = s.first;
    o.count = s.count;
    o.type = w;
    o.slot = s.slot;
    o.empty = (lo_x <= hi_x && lo_y <= hi_y) ? 0 : 1;
    o.key = s.key;
    o.lo_x = lo_x;
    o.lo_y = lo_y;
    o.hi_x = hi_x;
    o.hi_y = hi_y;
    o.rmax = rmax;
    A.queries[q] = o;
}

// Q and D, the round's two tables, are kernel parameters of their own: const and __restrict__ there tell the compiler that the
// kernel writes neither, which is what turns the uniform reads below into scalar loads
extern "C" __global__ void __launch_bounds__(64) egg_touch_kernel(EggTouchArgs A, const EggTouchQuery *__restrict__ Q,
                                                                  const EggTouchDisc *__restrict__ D) {
    const int lane = (int)threadIdx.x;  // (a workgroup is one wave)
    const int wave = (int)blockIdx.x, n_waves = (int)gridDim.x;
    const double inf = __builtin_huge_val();
    unsigned long long let_through = 0ull;  // (wave-uniform)
    for (int u = wave; u < A.n_units; u += n_waves) {
        const EggScanUnit un = A.units[u];
        const int w = un.type != 0 ? 1 : 0;
        const long long label = (long long)un.reserved;  // the one batch of the unit: its id, or its key
        const double reach = A.reach[w];
        const double *X = A.x[w] + un.offset, *Y = A.y[w] + un.offset, *Rad = A.radius[w] + un.offset;
        // the lane's particles: j * 64 + lane in place j, a NaN where the unit has none (a NaN touches nothing)
        double px[EGG_TC_OWN], py[EGG_TC_OWN], pr[EGG_TC_OWN];
        unsigned ok_mask = 0u;  // bit j: place j's scaled coordinates are finite and below EGG_SN_LIMIT
        double lo_x = inf, lo_y = inf, hi_x = -inf, hi_y = -inf, rmax = 0.0;
#pragma unroll
        for (int j = 0; j < EGG_TC_OWN; ++j) {
            const int i = j * EGG_WAVE + lane;
            const bool live = i < un.count;
            const double nan = __builtin_nan("");
            px[j] = live ? X[i] : nan;
            py[j] = live ? Y[i] : nan;
            pr[j] = live ? Rad[i] : nan;
            const double fx = px[j] * EGG_SN_SCALE, fy = py[j] * EGG_SN_SCALE;
            if (fabs(fx) < EGG_SN_LIMIT && fabs(fy) < EGG_SN_LIMIT) ok_mask |= 1u << j;  // (false for a NaN and for an infinity)
            lo_x = fmin(lo_x, px[j]);
            hi_x = fmax(hi_x, px[j]);
            lo_y = fmin(lo_y, py[j]);
            hi_y = fmax(hi_y, py[j]);
            rmax = fmax(rmax, fabs(pr[j]));
        }
        lo_x = tc_wave_min(lo_x);
        lo_y = tc_wave_min(lo_y);
        hi_x = tc_wave_max(hi_x);
        hi_y = tc_wave_max(hi_y);
        rmax = tc_wave_max(rmax);
        if (!(lo_x <= hi_x && lo_y <= hi_y)) continue;  // (wave-uniform: no centre without a NaN, the unit touches nothing)
        // lane k tests query k: same type, another batch, not empty, boxes not apart
        bool cand = false;
        if (lane < A.n_queries) {
            const EggTouchQuery q = Q[lane];
            cand = q.type == w && q.key != label && q.empty == 0 &&
                   !tc_apart(q.lo_x, q.lo_y, q.hi_x, q.hi_y, q.rmax, lo_x, lo_y, hi_x, hi_y, rmax, reach);
        }
        unsigned long long todo = __ballot(cand);
        let_through += (unsigned long long)__popcll(todo);
        for (; todo != 0ull; todo &= todo - 1ull) {
            const int k = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
            const long long first = Q[k].first;  // (uniform: scalar loads)
            const int count = Q[k].count;
            int pairs = 0, dropped = 0;
            unsigned touched = 0u;
            unsigned long long sx = 0ull, sy = 0ull;  // (two's complement: the sums wrap)
            for (int a = 0; a < count; ++a) {
                const EggTouchDisc d = D[first + a];  // (uniform)
                // the disc alone against the unit's box: the cull again, with the disc as a set of one
                if (tc_apart(d.x, d.y, d.x, d.y, fabs(d.r), lo_x, lo_y, hi_x, hi_y, rmax, reach)) continue;
#pragma unroll
                for (int j = 0; j < EGG_TC_OWN; ++j) {
                    // the rule (include/eggsim_touch.h): FP64 in exactly this order, no contraction; false for a NaN
                    const double dx = d.x - px[j], dy = d.y - py[j];
                    const double d2 = dx * dx + dy * dy;
                    const double L = reach * (d.r + pr[j]);
                    if (!(d2 <= L * L)) continue;
                    ++pairs;
                    touched |= 1u << j;
                    if (d.dropped != 0 || !(ok_mask >> j & 1u)) {
                        ++dropped;
                        continue;
                    }
                    sx += (unsigned long long)d.qx + (unsigned long long)llrint(px[j] * EGG_SN_SCALE);
                    sy += (unsigned long long)d.qy + (unsigned long long)llrint(py[j] * EGG_SN_SCALE);
                }
            }
            if (__ballot(pairs != 0) == 0ull) continue;  // (wave-uniform: only when there is one)
            const int n_pairs = tc_wave_sum(pairs), n_dropped = tc_wave_sum(dropped), n_particles = tc_wave_sum((int)__popc(touched));
            const unsigned long long tx = tc_wave_sum(sx), ty = tc_wave_sum(sy);
            if (lane == 0) {
                const int at = atomicAdd(A.cursor, 1);
                if (at >= 0 && at < A.cap) {
                    EggTouchRecord o;
                    o.slot = Q[k].slot;
                    o.pairs = n_pairs;
                    o.particles = n_particles;
                    o.dropped = n_dropped;
                    o.other = label;
                    o.sx = (long long)tx;
                    o.sy = (long long)ty;
                    A.out[at] = o;
                }
            }
        }
    }
    if (A.candidates && lane == 0 && let_through != 0ull) atomicAdd(A.candidates, let_through);
}
