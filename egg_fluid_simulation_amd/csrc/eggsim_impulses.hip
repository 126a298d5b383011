// eggsim_impulses.hip -- impulses (include/eggsim_impulse.h): edit the committed velocities of
// the particles inside the call's regions.  The only arrays written are vx and vy; no step launches anything of this file.
//
// A workgroup is ONE wave, so the unit a wave works on and the record it applies are functions of blockIdx and kernel
// arguments only: the compiler keeps them in scalar registers and reads them through the scalar cache.  Per chunk of 64
// particles every lane loads one particle (coalesced doubles: x, y, vx, vy, and inv_mass only when a record asks for it)
// and carries its velocity through the records in the list's order: record k finds what record k - 1 left.  A record whose
// mask or batch cannot match the unit is passed over wave-uniformly before any arithmetic; one whose region holds no
// particle of the chunk after the test and the ballot.  The counts are popcounts of ballots; only when some lane accepted
// an edit (a wave-uniform branch) are the two quantised changes reduced over the wave.  Lane k keeps record k's totals in
// its own registers: no LDS, no atomics.  A chunk stores vx, vy once, coalesced, and only when some record accepted an
// edit in it.  At the end lane k writes its partial (coalesced, nothing to zero) and a finishing kernel, one workgroup per
// row of the partials, adds them.  Particles are independent and integer addition has no order: the result equals any
// other schedule.
#include <hip/hip_runtime.h>

#include "eggsim_device.h"

namespace {

__device__ __forceinline__ long long im_wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

template <bool TOTALS>
__device__ __forceinline__ void im_body(const EggImpulseArgs &A) {
    const int lane = (int)threadIdx.x;  // (a workgroup is one wave)
    const int wave = (int)blockIdx.x, n_waves = (int)gridDim.x;
    long long cnt[2] = {0, 0}, sx[2] = {0, 0}, sy[2] = {0, 0}, skp[2] = {0, 0};
    for (int u = wave; u < A.n_units; u += n_waves) {
        const EggScanUnit un = A.units[u];
        const bool yolk = un.type != 0;
        const int t = yolk ? 1 : 0, bit = yolk ? 2 : 1;
        const long long batch = (long long)un.reserved;  // the id of the unit's batch
        const double *X = A.x[t] + un.offset, *Y = A.y[t] + un.offset, *IM = A.inv_mass[t] + un.offset;
        double *VX = A.vx[t] + un.offset, *VY = A.vy[t] + un.offset;
        for (int base = 0; base < un.count; base += EGG_WAVE) {
            const bool live = base + lane < un.count;
            const double x = live ? X[base + lane] : 0.0, y = live ? Y[base + lane] : 0.0;
            double vx = live ? VX[base + lane] : 0.0, vy = live ? VY[base + lane] : 0.0;
            const double im = A.need_inv_mass && live ? IM[base + lane] : 1.0;
            bool changed = false;
            for (int k = 0; k < A.n_recs; ++k) {
                const EggImpulse &r = A.recs[k];
                if (!(r.region.type_mask & bit)) continue;
                if (r.id != EGG_IM_ALL_BATCHES && r.id != batch) continue;
                double d2 = 0.0, R = 1.0;
                bool in = live && sn_test(r.region, x, y, d2, R);
                if (__ballot(in) == 0ull) continue;
                const int action = r.action, flags = r.flags;
                const double a0 = r.a[0], a1 = r.a[1], a2 = r.a[2];
                double w = 1.0;
                if (flags & EGG_IM_LINEAR) {  // (DISC and CAPSULE with R > 0 only: d2 and R are the test's own)
                    w = 1.0 - sqrt(d2) / R;
                    if (w < 0.0) w = 0.0;
                }
                if (flags & EGG_IM_BY_INV_MASS) w = w * im;
                double nvx, nvy;
                if (action == EGG_IM_KICK) {
                    nvx = vx + w * a0;
                    nvy = vy + w * a1;
                } else if (action == EGG_IM_BRAKE) {
                    const double g = w * a2;
                    nvx = vx + g * (a0 - vx);
                    nvy = vy + g * (a1 - vy);
                } else {
                    const double dx = x - a0, dy = y - a1;
                    if (action == EGG_IM_BLAST) {
                        const double b2 = dx * dx + dy * dy;
                        in = in && b2 > 0.0;  // (at the centre, or a NaN: the record passes the particle by)
                        const double g = (w * a2) / sqrt(b2);
                        nvx = vx + g * dx;
                        nvy = vy + g * dy;
                    } else {  // EGG_IM_SWIRL
                        const double g = w * a2;
                        nvx = vx - g * dy;
                        nvy = vy + g * dx;
                    }
                }
                const double dvx = nvx - vx, dvy = nvy - vy;
                const double fx = dvx * EGG_IM_SCALE, fy = dvy * EGG_IM_SCALE;
                const bool ok = fabs(fx) < EGG_IM_LIMIT && fabs(fy) < EGG_IM_LIMIT;  // (false for a NaN and for an infinity)
                const bool take = in && ok;
                const unsigned long long taken = __ballot(take);
                if (take) {
                    vx = nvx;
                    vy = nvy;
                    changed = true;
                }
                if (!TOTALS) continue;
                const int c = __popcll(taken), s = __popcll(__ballot(in && !ok));
                long long tx = 0, ty = 0;
                if (taken != 0ull) {
                    tx = im_wave_sum(llrint(take ? fx : 0.0));
                    ty = im_wave_sum(llrint(take ? fy : 0.0));
                }
                if (lane == k) {
                    if (yolk) {
                        cnt[1] += c;
                        sx[1] += tx;
                        sy[1] += ty;
                        skp[1] += s;
                    } else {
                        cnt[0] += c;
                        sx[0] += tx;
                        sy[0] += ty;
                        skp[0] += s;
                    }
                }
            }
            if (__ballot(changed) != 0ull && live) {
                VX[base + lane] = vx;
                VY[base + lane] = vy;
            }
        }
    }
    if (TOTALS) {
        long long *out = A.partials + (size_t)wave * EGG_IM_ROWS * EGG_WAVE + lane;
        out[0 * EGG_WAVE] = cnt[0];
        out[1 * EGG_WAVE] = sx[0];
        out[2 * EGG_WAVE] = sy[0];
        out[3 * EGG_WAVE] = skp[0];
        out[4 * EGG_WAVE] = cnt[1];
        out[5 * EGG_WAVE] = sx[1];
        out[6 * EGG_WAVE] = sy[1];
        out[7 * EGG_WAVE] = skp[1];
    }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(64) egg_impulse_kernel(EggImpulseArgs A) { im_body<true>(A); }

extern "C" __global__ void __launch_bounds__(64) egg_impulse_quiet_kernel(EggImpulseArgs A) { im_body<false>(A); }

// One workgroup per ROW of the partials.  A row has nk = n_recs lanes that carry something.  The threads form G = 1024 / nk
// groups of nk lanes; group g adds the waves g, g + G, .. of its row (consecutive lanes read consecutive words), LDS adds
// the groups.
extern "C" __global__ void __launch_bounds__(EGG_IM_FINISH_THREADS) egg_impulse_finish_kernel(EggImpulseFinishArgs A) {
    __shared__ long long red[EGG_IM_FINISH_THREADS];
    const int t = (int)threadIdx.x, row = (int)blockIdx.x;
    const int nk = A.n_recs;  // 1 .. 64
    const int G = EGG_IM_FINISH_THREADS / nk;
    const int g = t / nk, k = t - g * nk;
    long long sum = 0;
    if (g < G) {
        // eight loads in flight per thread: the walk over the waves is a chain of L2 round trips otherwise
        const long long *p = A.partials + (size_t)row * EGG_WAVE + k;
        const size_t stride = (size_t)EGG_IM_ROWS * EGG_WAVE;
        long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int w = g;
        for (; w + 7 * G < A.n_waves; w += 8 * G) {
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[q] += p[(size_t)(w + q * G) * stride];
        }
        for (; w < A.n_waves; w += G) acc[0] += p[(size_t)w * stride];
        sum = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    }
    red[t] = sum;
    __syncthreads();
    int half = 1;
    while (half < G) half <<= 1;
    for (half >>= 1; half >= 1; half >>= 1) {  // (t + half * nk = lane k of group g + half, below G * nk <= 1024)
        if (g + half < G && g < half) red[t] += red[t + half * nk];
        __syncthreads();
    }
    if (t < nk) A.out[row * EGG_WAVE + t] = red[t];
}
