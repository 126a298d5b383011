// eggsim_pieces.hip -- pieces (include/eggsim.h, "pieces"): the connected pieces of every requested
// atom (the particles of one type of one batch).  Read-only on the particle arrays; no step launches anything of this file.
//
// One workgroup per task (a grid stride where the grid is capped), in two classes: one wave for atoms of at most
// EGG_PC_WAVE_ATOM particles, EGG_PC_BLOCK threads for atoms up to EGG_PC_MAX_ATOM.  The atom lives in dynamic LDS for the
// whole solve: x, y as one 16-byte pair, the radius, the label and the size of the piece a particle leads, 32 bytes per
// particle, and EGG_PC_TAIL bytes of flags and totals behind them.
//
// The solve is a min-label propagation with pointer jumping.  Thread t owns the particles t, t + T, ..; it holds
// EGG_PC_OWN of them in registers and scans every j of the atom once for them: all lanes read the same LDS words (a
// broadcast, no bank conflict), test d2 <= L * L and keep the lowest label among the linked j.  A lower label is chased to
// where it points (label[m] < m) and stored.  The atom is done after a sweep that changed nothing.  Labels only fall, and
// only to indices of the same piece, so a lane that reads a label another lane is just lowering sees an older or a newer
// valid label: the fixed point is the same, only the number of sweeps depends on the schedule.  That number is no part of
// any answer.
//
// Where every radius of the atom has the same value L * L is one value: the test is hoisted on a workgroup-uniform flag,
// the product is the same expression reach * (r + r), squared.
//
// The finish: LDS integer adds give the size of every piece at its label, ballots count the pieces and the singles, a wave
// maximum over (size, -label) names the body, its quantised coordinates (EGG_SN_SCALE, EGG_SN_LIMIT) are summed over the
// wave by sn_wave_sum's rule, and thread 0 writes the one record.  The waves of the 256-thread class meet in the tail with
// LDS integer atomics (integer adds and maxima have no order).  No global atomics, no scratch.
#include <hip/hip_runtime.h>

#include "eggsim_device.h"

namespace {

struct PcTail {                      // behind the particles (EGG_PC_TAIL bytes)
    int32_t uniform;                 // every radius of the atom equals the first
    int32_t pieces, singles, dropped;
    unsigned long long best;         // (size << 32) | (INT32_MAX - label): the largest piece, the lower label among equals
    unsigned long long sx, sy;       // two's complement sums
};
static_assert(sizeof(PcTail) <= EGG_PC_TAIL, "the tail holds the flags and totals");

__device__ __forceinline__ long long pc_wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ unsigned long long pc_wave_max(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// one scan over every j for the EGG_PC_OWN particles base, base + T, .. of this thread; returns whether a label fell
template <int T, bool UNIFORM>
__device__ __forceinline__ bool pc_scan(int n, int base, double reach, const double2 *xy, const double *rad, int32_t *label) {
    double xi[EGG_PC_OWN], yi[EGG_PC_OWN], ri[EGG_PC_OWN];
    int32_t best[EGG_PC_OWN];
#pragma unroll
    for (int k = 0; k < EGG_PC_OWN; ++k) {
        const int i = base + k * T;
        const bool live = i < n;
        const double2 p = xy[live ? i : 0];
        xi[k] = live ? p.x : __builtin_nan("");  // (a NaN links to nothing)
        yi[k] = p.y;
        ri[k] = rad[live ? i : 0];
        best[k] = live ? label[i] : 0;
    }
    double l2u = 0.0;
    if (UNIFORM) {
        const double L = reach * (ri[0] + ri[0]);
        l2u = L * L;
    }
    for (int j = 0; j < n; ++j) {
        const double2 p = xy[j];
        const int32_t lj = label[j];
        const double rj = UNIFORM ? 0.0 : rad[j];
#pragma unroll
        for (int k = 0; k < EGG_PC_OWN; ++k) {
            const double dx = xi[k] - p.x, dy = yi[k] - p.y;
            const double d2 = dx * dx + dy * dy;
            double l2 = l2u;
            if (!UNIFORM) {
                const double L = reach * (ri[k] + rj);
                l2 = L * L;
            }
            const bool linked = d2 <= l2;  // (false when anything in it is a NaN)
            best[k] = linked && lj < best[k] ? lj : best[k];
        }
    }
    bool fell = false;
#pragma unroll
    for (int k = 0; k < EGG_PC_OWN; ++k) {
        const int i = base + k * T;
        if (i < n) {
            int32_t m = best[k];
            if (m < label[i]) {
                for (int32_t q = label[m]; q < m; q = label[m]) m = q;  // pointer jumping: strictly falling, so it ends; in [0, n)
                label[i] = m;
                fell = true;
            }
        }
    }
    return fell;
}

template <int T>
__device__ __forceinline__ void pc_body(const EggPiecesArgs &A) {
    extern __shared__ __align__(16) unsigned char pc_lds[];
    const int t = (int)threadIdx.x;
    for (int task_at = (int)blockIdx.x; task_at < A.n_tasks; task_at += (int)gridDim.x) {
        const EggPiecesTask task = A.tasks[task_at];
        const int n = task.count;  // 1 .. EGG_PC_MAX_ATOM (the host launches no empty atom and none over the cap)
        const int w = task.type != 0 ? 1 : 0;
        double2 *const xy = (double2 *)pc_lds;
        double *const rad = (double *)(pc_lds + (size_t)16 * n);
        int32_t *const label = (int32_t *)(pc_lds + (size_t)24 * n);
        int32_t *const size = (int32_t *)(pc_lds + (size_t)28 * n);
        PcTail *const tail = (PcTail *)(pc_lds + (size_t)EGG_PC_LDS_PER_PARTICLE * n);
        const double *X = A.x[w] + task.offset, *Y = A.y[w] + task.offset, *R = A.radius[w] + task.offset;
        if (t == 0) {
            tail->uniform = 1;
            tail->pieces = tail->singles = tail->dropped = 0;
            tail->best = tail->sx = tail->sy = 0ull;
        }
        __syncthreads();
        const double r0 = R[0];
        bool same = true;
        for (int i = t; i < n; i += T) {
            const double r = R[i];
            xy[i] = make_double2(X[i], Y[i]);
            rad[i] = r;
            label[i] = i;
            size[i] = 0;
            same = same && r == r0;  // (false for a NaN radius: the atom then takes the general path)
        }
        if (!same) tail->uniform = 0;
        __syncthreads();
        const bool uniform = tail->uniform != 0;  // (workgroup-uniform)
        const double reach = A.reach[w];
        int sweeps = 0;
        for (;;) {
            bool fell = false;
            for (int base = t; base < n; base += T * EGG_PC_OWN)
                fell |= uniform ? pc_scan<T, true>(n, base, reach, xy, rad, label) : pc_scan<T, false>(n, base, reach, xy, rad, label);
            ++sweeps;
            if (!__syncthreads_or(fell ? 1 : 0)) break;
        }
        // the sizes of the pieces at their labels
        for (int i = t; i < n; i += T) atomicAdd(&size[label[i]], 1);
        __syncthreads();
        int pieces = 0, singles = 0;  // (wave-uniform)
        unsigned long long best = 0ull;
        for (int base = 0; base < n; base += T) {  // (every wave runs the same trips: the ballots are taken by whole waves)
            const int i = base + t;
            const bool lead = i < n && label[i] == i;
            const int32_t s = lead ? size[i] : 0;
            pieces += __popcll(__ballot(lead));
            singles += __popcll(__ballot(lead && s == 1));
            const unsigned long long key = lead ? ((unsigned long long)(uint32_t)s << 32) | (uint32_t)(0x7fffffff - i) : 0ull;
            best = key > best ? key : best;
        }
        best = pc_wave_max(best);
        if ((t & (EGG_WAVE - 1)) == 0) {
            if (T == EGG_WAVE) {
                tail->pieces = pieces;
                tail->singles = singles;
                tail->best = best;
            } else {
                atomicAdd(&tail->pieces, pieces);
                atomicAdd(&tail->singles, singles);
                atomicMax(&tail->best, best);
            }
        }
        __syncthreads();
        const unsigned long long body = tail->best;
        const int32_t first = 0x7fffffff - (int32_t)(uint32_t)(body & 0xffffffffull), largest = (int32_t)(body >> 32);
        // the body's position sums: the quantisation and the drop rule of EGG_SN_SCALE / EGG_SN_LIMIT
        int dropped = 0;  // (wave-uniform)
        long long sx = 0, sy = 0;
        for (int base = 0; base < n; base += T) {
            const int i = base + t;
            const bool in = i < n && label[i] == first;
            const double2 p = xy[i < n ? i : 0];
            const double fx = p.x * EGG_SN_SCALE, fy = p.y * EGG_SN_SCALE;
            const bool ok = fabs(fx) < EGG_SN_LIMIT && fabs(fy) < EGG_SN_LIMIT;  // (false for a NaN and for an infinity)
            const long long qx = llrint(in && ok ? fx : 0.0), qy = llrint(in && ok ? fy : 0.0);
            const unsigned long long inside = __ballot(in);
            if (inside == 0ull) continue;  // (wave-uniform)
            dropped += __popcll(inside) - __popcll(__ballot(in && ok));
            sx += pc_wave_sum(qx);
            sy += pc_wave_sum(qy);
        }
        if (T != EGG_WAVE && (t & (EGG_WAVE - 1)) == 0) {
            atomicAdd(&tail->dropped, dropped);
            atomicAdd(&tail->sx, (unsigned long long)sx);
            atomicAdd(&tail->sy, (unsigned long long)sy);
        }
        if (T != EGG_WAVE) __syncthreads();
        if (t == 0) {
            EggPieceSummary rec;
            rec.n = n;
            rec.pieces = tail->pieces;
            rec.largest = largest;
            rec.first = first;
            rec.singles = tail->singles;
            rec.dropped = T == EGG_WAVE ? dropped : tail->dropped;
            rec.sx = T == EGG_WAVE ? sx : (long long)tail->sx;
            rec.sy = T == EGG_WAVE ? sy : (long long)tail->sy;
            A.out[task.slot] = rec;
            if (A.sweeps) A.sweeps[task.slot] = sweeps;
        }
        if (A.labels[w]) {
            int32_t *out = A.labels[w] + task.offset;
            for (int i = t; i < n; i += T) out[i] = label[i];
        }
        __syncthreads();  // (the next task of this workgroup rewrites the LDS)
    }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(EGG_WAVE) egg_pieces_wave_kernel(EggPiecesArgs A) { pc_body<EGG_WAVE>(A); }

extern "C" __global__ void __launch_bounds__(EGG_PC_BLOCK) egg_pieces_block_kernel(EggPiecesArgs A) { pc_body<EGG_PC_BLOCK>(A); }
