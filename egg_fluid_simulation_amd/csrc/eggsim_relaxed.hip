// eggsim_relaxed.hip -- gfx950 kernels of the relaxed-order collision solver (EGG_OPT_SOLVER_ORDER = 1; DESIGN.md
// section 2.7).  Everything but the collision pass is the reference's, as in the exact path: pre-solve + follow
// (egg_pre_follow, shared with the packed pipeline), post-solve.  The collision pass is a Jacobi pass with constraint
// averaging: every particle gathers the corrections of all its candidate pairs, computed from the positions at the
// start of the pass, and moves once by their mean scaled by omega.  One thread per particle, no atomics in the
// accumulation: the result does not depend on scheduling, and tests/relaxed_model.py reproduces it bit for bit.
//
// Per pass (host: eggsim_host_relaxed.hip):
//   egg_rx_insert_kernel   cell of every particle (floor(x / cell), L:1486-1511), its slot in the cell table, counts
//   (hipcub exclusive scan of the counts: each occupied slot's range of grouped positions)
//   egg_rx_scatter_kernel  particles into their slot's range (any order)
//   egg_rx_rank_kernel     ascending particle index inside each range (the reference's order inside a cell), grouped
//                          copies of (x, y) and (inverse mass, radius)
//   egg_rx_gather_kernel   the 3x3 cells of every particle in the reference's loop order (x offset outer, y inner,
//                          L:1568-1569), the pair corrections in that order, the averaged move
//
// All arithmetic is IEEE double in the order of the definition: compile with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include "eggsim_device.h"

#include "eggsim_tile.h"

namespace {

// normals of a coincident pair (d2 == 0), by (b - a) & 7: eight unit vectors, components 0, +-1, +-sqrt(1/2)
#define EGG_RX_S 0x1.6a09e667f3bcdp-1
__constant__ double kRxDirX[8] = {1.0, EGG_RX_S, 0.0, -EGG_RX_S, -1.0, -EGG_RX_S, 0.0, EGG_RX_S};
__constant__ double kRxDirY[8] = {0.0, EGG_RX_S, 1.0, EGG_RX_S, 0.0, -EGG_RX_S, -1.0, -EGG_RX_S};

// cell of a position; false for a NaN coordinate or a cell outside +-2^30
__device__ __forceinline__ bool rx_cell(double2 p, double cell, int32_t &cx, int32_t &cy) {
    const double fx = floor(p.x / cell), fy = floor(p.y / cell);
    const bool ok = fx >= -0x1p30 && fx <= 0x1p30 && fy >= -0x1p30 && fy <= 0x1p30;
    cx = ok ? (int32_t)fx : 0;
    cy = ok ? (int32_t)fy : 0;
    return ok;
}

__device__ __forceinline__ unsigned long long rx_key(int32_t cx, int32_t cy) {
    return ((unsigned long long)(uint32_t)(cx + 0x40000000) << 32) | (unsigned long long)(uint32_t)(cy + 0x40000000);
}

__device__ __forceinline__ uint32_t rx_hash(unsigned long long k) {  // the 64-bit finaliser of MurmurHash3
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (uint32_t)k;
}

}  // namespace

// per-particle atom index (run when the atoms change): one workgroup per atom
extern "C" __global__ void __launch_bounds__(256) egg_rx_atoms_kernel(const int32_t *atom_offset, const int32_t *atom_count,
                                                                      int n_atoms, int32_t *p_atom) {
    const int a = blockIdx.x;
    if (a >= n_atoms) return;
    const int g0 = atom_offset[a], cnt = atom_count[a];
    for (int q = threadIdx.x; q < cnt; q += 256) p_atom[g0 + q] = a;
}

// Start of a step: pre-solve + follow of the first sub-step from the committed state.
extern "C" __global__ void __launch_bounds__(256) egg_rx_begin_kernel(EggRelaxedArgs A) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= A.n) return;
    const int atom = A.p_atom[i];
    const double2 ps = make_double2(A.x_in[i], A.y_in[i]);
    double2 v = make_double2(A.vx_in[i], A.vy_in[i]);
    double2 out;
    egg_pre_follow(A.damping, A.sub_delta, A.eps, A.follow_compliance, ps, v, A.inv_mass[i], A.atom_tx[atom],
                   A.atom_ty[atom], A.atom_fd[atom], out);
    A.prev[i] = ps;
    A.pos[i] = out;
}

// Between two sub-steps: post-solve of the one (L:1690-1693), pre-solve + follow of the next.
extern "C" __global__ void __launch_bounds__(256) egg_rx_mid_kernel(EggRelaxedArgs A) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= A.n) return;
    const int atom = A.p_atom[i];
    const double2 ps = A.pos[i], pv = A.prev[i];
    double2 v = make_double2((ps.x - pv.x) / A.sub_delta, (ps.y - pv.y) / A.sub_delta);
    double2 out;
    egg_pre_follow(A.damping, A.sub_delta, A.eps, A.follow_compliance, ps, v, A.inv_mass[i], A.atom_tx[atom],
                   A.atom_ty[atom], A.atom_fd[atom], out);
    A.prev[i] = ps;
    A.pos[i] = out;
}

// End of the step: post-solve of the last sub-step into the [cur ^ 1] arrays -- unless a pass flagged a bad cell: the
// step then fails and [cur ^ 1] keeps the positions at the start of the last committed step (EGG_FIELD_LAST_X / Y).
extern "C" __global__ void __launch_bounds__(256) egg_rx_end_kernel(EggRelaxedArgs A) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= A.n || A.status[0] != 0) return;
    const double2 ps = A.pos[i], pv = A.prev[i];
    A.x_out[i] = ps.x;
    A.y_out[i] = ps.y;
    A.vx_out[i] = (ps.x - pv.x) / A.sub_delta;
    A.vy_out[i] = (ps.y - pv.y) / A.sub_delta;
}

// Cell of every particle, its slot in the cell table, the slot's particle count.  (The table is at least twice as
// large as the particle count: a probe always ends.)
extern "C" __global__ void __launch_bounds__(256) egg_rx_insert_kernel(EggRelaxedArgs A) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= A.n) return;
    int32_t cx, cy;
    if (!rx_cell(A.pos[i], A.cell_size, cx, cy)) A.status[0] = 1;  // (the step fails; cell (0, 0) keeps the pass in bounds)
    const unsigned long long key = rx_key(cx, cy);
    uint32_t h = rx_hash(key) & A.table_mask;
    for (;;) {
        const unsigned long long old = atomicCAS(&A.hkey[h], EGG_RX_EMPTY_KEY, key);
        if (old == EGG_RX_EMPTY_KEY || old == key) break;
        h = (h + 1) & A.table_mask;
    }
    atomicAdd(&A.hcount[h], 1u);
    A.pslot[i] = (int32_t)h;
}

// Every particle into its slot's range of grouped positions [hstart[h], hstart[h + 1]), in whatever order the
// atomics give (the counts are used up: nothing reads them afterwards).
extern "C" __global__ void __launch_bounds__(256) egg_rx_scatter_kernel(EggRelaxedArgs A) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= A.n) return;
    const int h = A.pslot[i];
    const uint32_t k = atomicSub(&A.hcount[h], 1u) - 1u;
    A.tmp[A.hstart[h] + k] = i;
}

// Inside a cell: ascending particle index (a particle's place = how many of its cell's particles have a smaller one),
// with the grouped copies of what the gather reads.
extern "C" __global__ void __launch_bounds__(256) egg_rx_rank_kernel(EggRelaxedArgs A) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= A.n) return;
    const int h = A.pslot[i];
    const int st = (int)A.hstart[h], en = (int)A.hstart[h + 1];
    int rank = 0;
    for (int e = st; e < en; ++e) rank += A.tmp[e] < i ? 1 : 0;
    const int t = st + rank;
    A.sidx[t] = i;
    A.spos[t] = A.pos[i];
    A.swr[t] = make_double2(A.inv_mass[i], A.radius[i]);
}

// The relaxed pass of DESIGN.md section 2.7, one thread per grouped slot (threads of a wave share cells).
extern "C" __global__ void __launch_bounds__(256) egg_rx_gather_kernel(EggRelaxedArgs A) {
    const int t = (int)(blockIdx.x * 256 + threadIdx.x);
    int pairs = 0;
    if (t < A.n) {
        const int i = A.sidx[t];
        const double2 p = A.spos[t], wr = A.swr[t];
        int32_t cx, cy;
        (void)rx_cell(p, A.cell_size, cx, cy);  // (a bad cell was flagged by the insert kernel)
        double sx = 0.0, sy = 0.0;
        int n_fired = 0;
        for (int ox = -1; ox <= 1; ++ox) {
            for (int oy = -1; oy <= 1; ++oy) {
                const unsigned long long key = rx_key(cx + ox, cy + oy);
                uint32_t h = rx_hash(key) & A.table_mask;
                unsigned long long k;
                while ((k = A.hkey[h]) != key && k != EGG_RX_EMPTY_KEY) h = (h + 1) & A.table_mask;
                if (k == EGG_RX_EMPTY_KEY) continue;
                const int st = (int)A.hstart[h], en = (int)A.hstart[h + 1];
                for (int e = st; e < en; ++e) {
                    const int j = A.sidx[e];
                    if (j == i) continue;
                    const double2 q = A.spos[e], wq = A.swr[e];
                    // pair (a, b), a < b: both sides evaluate the same expression
                    const bool first = i < j;
                    const double2 pa = first ? p : q, pb = first ? q : p;
                    const double wa = first ? wr.x : wq.x, wb = first ? wq.x : wr.x;
                    const double ra = first ? wr.y : wq.y, rb = first ? wq.y : wr.y;
                    const double wsum = wa + wb;
                    if (wsum < A.eps) continue;  // L:1601
                    pairs += j > i ? 1 : 0;
                    const double dx = pb.x - pa.x, dy = pb.y - pa.y;
                    const double d2 = dx * dx + dy * dy;
                    const double min_distance = A.overlap * (ra + rb);
                    if (!(d2 <= min_distance * min_distance)) continue;
                    ++n_fired;
                    const double divisor = wsum + A.collision_compliance;
                    if (divisor < A.eps) {  // _enforce_distance returns zeros (L:1527-1529)
                        sx = sx + 0.0;
                        sy = sy + 0.0;
                        continue;
                    }
                    const double current = sqrt(d2);
                    const double violation = current - min_distance;
                    double nx, ny;
                    if (d2 == 0.0) {  // coincident: the one departure from the reference's normalize(0, 0) = (0, 0)
                        const int k8 = (first ? j - i : i - j) & 7;
                        nx = kRxDirX[k8];
                        ny = kRxDirY[k8];
                    } else if (current < A.eps) {
                        nx = 0.0;
                        ny = 0.0;
                    } else {
                        nx = dx / current;
                        ny = dy / current;
                    }
                    double correction = -violation / divisor;
                    const double max_correction = fabs(violation);
                    if (correction < -max_correction) correction = -max_correction;
                    if (correction > max_correction) correction = max_correction;
                    if (first) {
                        sx = sx + -nx * correction * wa;
                        sy = sy + -ny * correction * wa;
                    } else {
                        sx = sx + nx * correction * wb;
                        sy = sy + ny * correction * wb;
                    }
                }
            }
        }
        double2 out = p;
        if (n_fired > 0) {
            out.x = p.x + (sx * A.omega) / (double)n_fired;
            out.y = p.y + (sy * A.omega) / (double)n_fired;
        }
        A.pos_next[i] = out;
    }
    // pairs counted (each once: by its smaller index), one atomic per wave
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) pairs += __shfl_xor(pairs, d, 64);
    if ((threadIdx.x & 63) == 0 && pairs) atomicAdd(&A.status[1 + A.pass], (unsigned long long)pairs);
}
