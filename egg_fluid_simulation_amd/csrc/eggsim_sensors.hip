// eggsim_sensors.hip -- sensors (include/eggsim.h, "sensors"): count and locate the committed
// positions inside the handle's regions.  Read-only on the particle arrays; no step launches anything of this file.
//
// A workgroup is ONE wave, so the unit a wave works on and the sensor record it tests are functions of blockIdx and kernel
// arguments only: the compiler keeps them in scalar registers and reads them through the scalar cache.  Per chunk of 64
// particles every lane loads one particle (coalesced doubles) and quantises it once; per sensor whose mask covers the
// unit's type the wave evaluates the test and takes the ballot.  The count is the popcount of the mask; only when the mask
// is not empty (a wave-uniform branch) are the two quantised coordinates reduced over the wave.  Lane k keeps sensor k's
// sums in its own registers: no LDS, no atomics.  At the end lane k writes its partial (coalesced, nothing to zero) and a
// finishing kernel, one workgroup per row of the partials, adds them.  Integer addition has no order: the result equals
// any other schedule.
//
// The per-batch read is the same body in a second instantiation over the units of the listed batches: lane k writes the
// unit's count in sensor k, and a finishing kernel adds the units of every (listed id, type) in the caller's order.
#include <hip/hip_runtime.h>

#include "eggsim_device.h"

namespace {

// (the test of one sensor record for one position is sn_inside of eggsim_device.h: the impulses' regions share it)

__device__ __forceinline__ long long sn_wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// BATCH = false: the totals.  BATCH = true: counts per unit.
template <bool BATCH>
__device__ __forceinline__ void sn_body(const EggSensorArgs &A) {
    const int lane = (int)threadIdx.x;  // (a workgroup is one wave)
    const int wave = (int)blockIdx.x, n_waves = (int)gridDim.x;
    long long cnt[2] = {0, 0}, sx[2] = {0, 0}, sy[2] = {0, 0};
    long long dropped[2] = {0, 0};  // (wave-uniform)
    for (int u = wave; u < A.n_units; u += n_waves) {
        const EggSensorUnit un = A.units[u];
        const bool yolk = un.type != 0;
        const int bit = yolk ? 2 : 1;
        const double *X = A.x[yolk ? 1 : 0] + un.offset, *Y = A.y[yolk ? 1 : 0] + un.offset;
        int unit_count = 0;
        for (int base = 0; base < un.count; base += EGG_WAVE) {
            const bool live = base + lane < un.count;
            const double x = live ? X[base + lane] : 0.0, y = live ? Y[base + lane] : 0.0;
            const double fx = x * EGG_SN_SCALE, fy = y * EGG_SN_SCALE;
            const bool ok = fabs(fx) < EGG_SN_LIMIT && fabs(fy) < EGG_SN_LIMIT;  // (false for a NaN and for an infinity)
            const long long qx = llrint(ok ? fx : 0.0), qy = llrint(ok ? fy : 0.0);
            for (int k = 0; k < A.n_sensors; ++k) {
                const EggSensor s = A.sensors[k];
                if (!(s.type_mask & bit)) continue;
                const bool in = live && sn_inside(s, x, y);
                const unsigned long long inside = __ballot(in);
                if (inside == 0ull) continue;
                const int c = __popcll(__ballot(in && ok));
                const int lost = __popcll(inside) - c;
                if (BATCH) {
                    if (lane == k) unit_count += c;
                    continue;
                }
                if (yolk) dropped[1] += lost; else dropped[0] += lost;
                if (c == 0) continue;
                const long long tx = sn_wave_sum(in && ok ? qx : 0), ty = sn_wave_sum(in && ok ? qy : 0);
                if (lane == k) {
                    if (yolk) {
                        cnt[1] += c;
                        sx[1] += tx;
                        sy[1] += ty;
                    } else {
                        cnt[0] += c;
                        sx[0] += tx;
                        sy[0] += ty;
                    }
                }
            }
        }
        if (BATCH) A.unit_counts[(size_t)u * EGG_WAVE + lane] = unit_count;
    }
    if (!BATCH) {
        long long *out = A.partials + (size_t)wave * EGG_SN_ROWS * EGG_WAVE + lane;
        out[0 * EGG_WAVE] = cnt[0];
        out[1 * EGG_WAVE] = sx[0];
        out[2 * EGG_WAVE] = sy[0];
        out[3 * EGG_WAVE] = cnt[1];
        out[4 * EGG_WAVE] = sx[1];
        out[5 * EGG_WAVE] = sy[1];
        out[6 * EGG_WAVE] = lane == 0 ? dropped[0] : lane == 1 ? dropped[1] : 0;
    }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(64) egg_sensor_sums_kernel(EggSensorArgs A) { sn_body<false>(A); }

extern "C" __global__ void __launch_bounds__(64) egg_sensor_units_kernel(EggSensorArgs A) { sn_body<true>(A); }

// One workgroup per ROW of the partials: count, sx, sy of white, the same of yolk, and the dropped pair.  A row has nk
// lanes that carry something: the sensors of the list, 2 for the dropped pair.  The threads form G = 1024 / nk groups of nk
// lanes; group g adds the waves g, g + G, .. of its row (consecutive lanes read consecutive words), LDS adds the groups.
extern "C" __global__ void __launch_bounds__(EGG_SN_FINISH_THREADS) egg_sensor_finish_kernel(EggSensorFinishArgs A) {
    __shared__ long long red[EGG_SN_FINISH_THREADS];
    const int t = (int)threadIdx.x, row = (int)blockIdx.x;
    const int nk = row < 6 ? A.n_sensors : 2;  // 1 .. 64
    const int G = EGG_SN_FINISH_THREADS / nk;
    const int g = t / nk, k = t - g * nk;
    long long sum = 0;
    if (g < G) {
        // eight loads in flight per thread: the walk over the waves is a chain of L2 round trips otherwise
        const long long *p = A.partials + (size_t)row * EGG_WAVE + k;
        const size_t stride = (size_t)EGG_SN_ROWS * EGG_WAVE;
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

extern "C" __global__ void __launch_bounds__(256) egg_sensor_batch_finish_kernel(EggSensorBatchFinishArgs A) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)A.n_rows * A.n_sensors) return;
    const int r = (int)(i / A.n_sensors), k = (int)(i - (long long)r * A.n_sensors);
    const int first = A.row_first[r], units = A.row_units[r];
    int32_t c = 0;
    for (int u = 0; u < units; ++u) c += A.unit_counts[(size_t)(first + u) * EGG_WAVE + k];
    A.counts[((size_t)(r >> 1) * A.n_sensors + k) * 2 + (r & 1)] = c;
}
