// eggsim_probes.hip -- probes (include/eggsim.h, "probes"): per probe and particle type the ONE
// committed particle that is nearest a point or that a ray enters first.  Read-only on the particle arrays; no step launches
// anything of this file.
//
// The scan walks UNITS of at most 1,024 consecutive particles of one atom.  A workgroup is ONE wave, so the unit it works on
// and the probe record it evaluates are functions of blockIdx and kernel arguments only and stay in scalar registers; the
// call's list travels in the launch arguments.  Per chunk of 64 particles every lane loads one particle's x, y, radius; per probe whose mask covers
// the unit's type the wave evaluates the rule, drops what cannot beat the probe's running best and takes the ballot of what
// is left.  Only when that ballot is not empty (a wave-uniform branch; the common skip) is the score min-reduced over the
// wave.  Lane k keeps probe k's running best per type in its own registers: no LDS, no atomics.
//
// The tie rule -- equal scores go to the lowest array index of the type, which is the lowest batch key, then the lowest index
// in the batch -- is applied IN the reduction: within a chunk the lanes are in array order, so the winner is the first lane
// of the ballot of the lanes that hold the minimum; a wave meets its units in ascending array order, so a later chunk wins
// only with a strictly smaller score; the finishing kernel compares (score, array index) pairs.  A minimum by a total order
// has no schedule dependence: any grid gives the same answer.
#include <hip/hip_runtime.h>

#include "eggsim_device.h"

namespace {

// the rule of one probe for one particle (include/eggsim.h): FP64 in exactly this order, no contraction; every comparison is
// false for a NaN.  True: a candidate, with its score.
__device__ __forceinline__ bool pb_eval(const EggProbe &q, double x, double y, double r, double &score) {
    if (q.kind == EGG_PB_POINT) {
        const double dx = x - q.p[0], dy = y - q.p[1];
        const double d2 = dx * dx + dy * dy;
        score = d2;
        return d2 <= q.p[2] * q.p[2] && r == r;
    }
    const double R = r + q.p[4];
    const double fx = q.p[0] - x, fy = q.p[1] - y;
    const double c = (fx * fx + fy * fy) - R * R;
    score = 0.0;
    if (c <= 0.0) return true;  // the ray starts in or on the disc
    const double ex = q.p[2] - q.p[0], ey = q.p[3] - q.p[1];
    const double l2 = ex * ex + ey * ey;
    const double b = fx * ex + fy * ey;
    if (!(b < 0.0)) return false;
    const double disc = b * b - l2 * c;
    if (!(disc >= 0.0)) return false;
    const double t = (-b - sqrt(disc)) / l2;
    score = t;
    return t <= 1.0;
}

// lane k's value of v, k wave-uniform
__device__ __forceinline__ int pb_lane_int(int v, int k) { return __builtin_amdgcn_readlane(v, k); }
__device__ __forceinline__ double pb_lane_double(double v, int k) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), k), hi = __builtin_amdgcn_readlane(__double2hiint(v), k);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double pb_wave_min(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}

// (score, array index) a before b: none (index < 0) is last, equal scores go to the lower index
__device__ __forceinline__ bool pb_before(double sa, int ia, double sb, int ib) {
    return ia >= 0 && (ib < 0 || sa < sb || (sa == sb && ia < ib));
}

__device__ __forceinline__ void pb_scan(const EggProbeArgs &A) {
    const int lane = (int)threadIdx.x;  // (a workgroup is one wave)
    const int wave = (int)blockIdx.x, n_waves = (int)gridDim.x;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double best_w = inf, best_y = inf;  // lane k: probe k's best score of this wave per type
    int at_w = -1, at_y = -1;           // and its array index in the type, -1 while there is none
    for (int u = wave; u < A.n_units; u += n_waves) {  // (ascending array index within a type)
        const EggScanUnit un = A.units[u];
        const bool yolk = un.type != 0;
        const int bit = yolk ? 2 : 1;
        const double *X = A.x[yolk ? 1 : 0] + un.offset, *Y = A.y[yolk ? 1 : 0] + un.offset, *R = A.radius[yolk ? 1 : 0] + un.offset;
        for (int base = 0; base < un.count; base += EGG_WAVE) {
            const bool live = base + lane < un.count;
            const double x = live ? X[base + lane] : 0.0, y = live ? Y[base + lane] : 0.0, r = live ? R[base + lane] : 0.0;
            for (int k = 0; k < A.n_probes; ++k) {
                const EggProbe &q = A.probes[k];
                if (!(q.type_mask & bit)) continue;
                double s = 0.0;
                bool cand = live && pb_eval(q, x, y, r, s);
                // what the wave holds for probe k came from a lower array index: only a strictly smaller score replaces it
                const int have = pb_lane_int(yolk ? at_y : at_w, k);
                const double cur = pb_lane_double(yolk ? best_y : best_w, k);
                cand = cand && (have < 0 || s < cur);
                if (__ballot(cand) == 0ull) continue;
                const double m = pb_wave_min(cand ? s : inf);
                const int first = __ffsll((long long)__ballot(cand && s == m)) - 1;  // the lowest index among equal scores
                if (lane == k) {
                    if (yolk) {
                        best_y = m;
                        at_y = un.offset + base + first;
                    } else {
                        best_w = m;
                        at_w = un.offset + base + first;
                    }
                }
            }
        }
    }
    // the partials lie by (type, probe) first and wave last: the finishing kernel reads a probe's row densely
    if (lane < A.n_probes) {
        const size_t white = (size_t)lane * n_waves + wave, yolk = ((size_t)EGG_WAVE + lane) * n_waves + wave;
        A.part_score[white] = best_w;
        A.part_index[white] = at_w;
        A.part_score[yolk] = best_y;
        A.part_index[yolk] = at_y;
    }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(64) egg_probe_scan_kernel(EggProbeArgs A) { pb_scan(A); }

// Workgroup (g, w) finishes the P <= 8 probes 8 g .. 8 g + P - 1 of type w.  Each probe has G = 1024 / P consecutive
// threads: thread t belongs to probe 8 g + t / G and walks the waves t % G, t % G + G, .. of that probe's row of the
// partials (consecutive threads read consecutive words; a single probe is walked by all 1,024 threads), LDS takes the
// minimum over a probe's threads by the same (score, array index) order, and the probe's first thread gathers the
// winner's x, y, radius.
extern "C" __global__ void __launch_bounds__(EGG_PB_FINISH_THREADS) egg_probe_finish_kernel(EggProbeFinishArgs A) {
    __shared__ double red_score[EGG_PB_FINISH_THREADS];
    __shared__ int32_t red_index[EGG_PB_FINISH_THREADS];
    const int t = (int)threadIdx.x, w = (int)blockIdx.y;
    const int k0 = (int)blockIdx.x * EGG_PB_FINISH_PROBES;
    const int P = min(EGG_PB_FINISH_PROBES, A.n_probes - k0);  // 1 .. 8: the grid has no workgroup without a probe
    const int walks = EGG_PB_FINISH_THREADS / P;
    const int mine = t / walks, walk = t - mine * walks, k = k0 + mine;  // (mine >= P: one of the 1024 % P idle threads)
    double s = 0.0;
    int at = -1;
    if (mine < P) {
        const double *ps = A.part_score + ((size_t)w * EGG_WAVE + k) * A.n_waves;  // (the row of (type w, probe k))
        const int32_t *pi = A.part_index + ((size_t)w * EGG_WAVE + k) * A.n_waves;
#pragma unroll 4
        for (int wave = walk; wave < A.n_waves; wave += walks) {
            const double os = ps[wave];
            const int oi = pi[wave];
            if (pb_before(os, oi, s, at)) {
                s = os;
                at = oi;
            }
        }
    }
    red_score[t] = s;
    red_index[t] = at;
    __syncthreads();
    int half = 1;
    while (half < walks) half <<= 1;
    for (half >>= 1; half >= 1; half >>= 1) {  // (t + half = the same probe's thread of walk + half, below (mine + 1) * walks <= 1024)
        if (mine < P && walk < half && walk + half < walks) {
            const int o = t + half;
            if (pb_before(red_score[o], red_index[o], red_score[t], red_index[t])) {
                red_score[t] = red_score[o];
                red_index[t] = red_index[o];
            }
        }
        __syncthreads();
    }
    if (mine < P && walk == 0) {
        EggProbeOut o;
        o.index = red_index[t];
        o.reserved = 0;
        const bool found = o.index >= 0;  // (an index the scan wrote: inside the type's arrays)
        o.score = found ? red_score[t] : 0.0;
        o.x = found ? A.x[w][o.index] : 0.0;
        o.y = found ? A.y[w][o.index] : 0.0;
        o.radius = found ? A.radius[w][o.index] : 0.0;
        A.out[2 * k + w] = o;
    }
}
