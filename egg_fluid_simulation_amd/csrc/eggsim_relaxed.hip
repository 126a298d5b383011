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
// In a device group (eggsim_host_relaxed_group.hip) every particle has a global key, its index in one handle holding
// every batch, and the pass runs over the local particles plus read-only ghosts of the neighbours': the kernels that
// write positions record their cell box, egg_rx_pack_kernel (sender) and egg_rx_unpack_kernel (receiver) move the
// ghosts, and the key replaces the index in the rank order, the pair orientation and the pair count.  On a single
// handle (the G = false instantiations) the key is the index and nothing else changes.
//
// With effective cohesion (EGG_OPT_COHESION = 1; DESIGN.md section 2.7, "Cohesion") the rank and gather kernels run in
// their cohesive instantiations (K = true, egg_rx_*_coh_kernel): the rank kernel writes a batch tag per grouped slot, and
// a same-batch pair beyond the collision distance but within cohesion_interaction_distance_factor (ra + rb) is pulled
// back to the collision distance through the collision correction's own arithmetic with the cohesion compliance.  The
// K = false instantiations are the kernels as they were.
//
// With static colliders (egg_set_colliders; DESIGN.md section 2.7, "Colliders") the gather kernel runs in its collider
// instantiations (D = true, egg_rx_gather*_col_kernel): the position a particle is about to get is projected out of /
// into every collider of the handle's list whose mask covers the type, in list order, before it is written.  The
// D = false instantiations are the kernels as they were.
//
// With collider surfaces (egg_set_collider_surfaces; DESIGN.md section 2.7, "Collider surfaces") of which at least one has
// friction > 0 the collider instantiations run as their surface twins (D = true and S = true,
// egg_rx_gather*_col_srf_kernel): right after a collider with friction has projected a particle, step 5c removes the
// tangential part of the particle's displacement over the sub-step, relative to the surface's velocity, up to friction
// times the depth the projection has just corrected.  The S = false instantiations are the kernels as they were.
//
// While the list holds a wall (EGG_COLLIDER_WALL; DESIGN.md section 2.7, "Walls") the surface twins run as their wall twins
// (D, S and W = true, egg_rx_gather*_col_wall_kernel): a wall is a segment that also sweeps the particle's path over the
// sub-step, prev[me] to the position now, and puts a particle that has crossed it back on the side it started from.  The
// W = false instantiations are the kernels as they were.
//
// While a collider's motion is not zero (egg_set_collider_motion; DESIGN.md section 2.7, "Collider motion") the wall twins
// run as their motion twins (egg_rx_gather*_col_mov_kernel, which take EggRxMotionFields besides): every collider is
// where it is at the end of the pass's sub-step, a wall sweeps in its own frame, and friction is taken relative to the
// moving surface.  Every other instantiation is the kernel as it was.
//
// While a collider's spin is not zero (egg_set_collider_spin; DESIGN.md section 2.7, "Collider spin") the motion twins run
// as their spin twins (egg_rx_gather*_col_spin_kernel, which take EggRxSpinFields besides): a collider with omega != 0 is
// turned about its pivot, which rides on its motion, by the angle of the sub-step's end -- sines and cosines are the
// host's --, a turning wall sweeps from the sub-step's start turned along with it by one sub-step, and friction takes the
// surface's velocity at the contact point.  A collider with omega == 0 takes the motion twin's expressions.
//
// With force fields (egg_set_forces; DESIGN.md section 2.7, "Forces") the kernels that begin a sub-step run in their force
// instantiations (F = true, egg_rx_begin*_frc_kernel, egg_rx_mid*_frc_kernel): the fields of the handle's list whose mask
// covers the type accelerate the velocity the pre-solve is about to damp.  The F = false instantiations are the kernels
// as they were.
//
// With viscosity (egg_set_viscosity; DESIGN.md section 2.7, "Viscosity") every sub-step of a type whose coefficient is not
// zero ends with one more pass over the same cell structure (insert, scan and scatter are the collision pass's):
// egg_rx_rank*_visc_kernel groups every entry's displacement of the sub-step u = pos - prev beside its position, and
// egg_rx_gather*_visc_kernel blends a particle's u with the weighted mean of its neighbours' within one cell size and
// rewrites prev.  Positions are not touched.  In a group the ghosts' u arrive in the record words that carry inverse mass
// and radius in a collision pass (egg_rx_pack_visc_kernel).  Nothing of it runs while both coefficients are zero.
//
// With white-yolk coupling (egg_set_coupling; DESIGN.md section 2.7, "Coupling"; one handle only) every sub-step runs one
// cross-type pass between its begin / mid kernel and its first collision pass: both types build their table at a shared
// cell size with the insert, scatter and rank kernels above, and egg_rx_couple_kernel moves every particle by the mean of
// its pairs with the OTHER type's particles, found in the other type's table.  Nothing of it runs while the factor is zero.
// With white-yolk adhesion besides (egg_set_adhesion; section 2.7, "Adhesion"; acts while reach > factor) the tables are
// built at the band's cell size through the cohesive rank kernel, which leaves the batch tags, and the pass runs as
// egg_rx_couple_adh_kernel: a same-batch cross pair in the band is pulled back to the coupling distance.
//
// With yolk containment (egg_set_containment; section 2.7, "Containment"; any path) every sub-step runs two more kernels in
// front of its first collision pass: egg_rx_contain_sum_kernel reduces every white atom to (cx, cy, L) in a fixed FP64
// order, and egg_rx_contain_kernel (egg_rx_contain_group_kernel with a halo) projects the yolk particles of the same atom
// index that lie beyond L back onto the disc.  Nothing of it runs while the factor is zero.
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

// (rx_cell and rx_append: eggsim_device.h, shared with eggsim_relaxed_wire.hip)
__device__ __forceinline__ unsigned long long rx_key(int32_t cx, int32_t cy) {
    return ((unsigned long long)(uint32_t)(cx + 0x40000000) << 32) | (unsigned long long)(uint32_t)(cy + 0x40000000);
}

// Cell box of the positions a wave writes (group only): every lane calls it, one atomic per word and wave.
__device__ __forceinline__ void rx_box(unsigned long long *box, bool have, double2 p, double cell) {
    int32_t cx = 0, cy = 0;
    if (have) (void)rx_cell(p, cell, cx, cy);  // (a bad cell was or will be flagged by the insert kernel)
    const unsigned long long ux = (unsigned long long)((long long)cx + EGG_RX_BOX_BIAS);
    const unsigned long long uy = (unsigned long long)((long long)cy + EGG_RX_BOX_BIAS);
    unsigned long long w0 = have ? (1ull << 32) - ux : 0ull, w1 = have ? ux : 0ull;
    unsigned long long w2 = have ? (1ull << 32) - uy : 0ull, w3 = have ? uy : 0ull;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        w0 = max(w0, __shfl_xor(w0, d, 64));
        w1 = max(w1, __shfl_xor(w1, d, 64));
        w2 = max(w2, __shfl_xor(w2, d, 64));
        w3 = max(w3, __shfl_xor(w3, d, 64));
    }
    if ((threadIdx.x & 63) == 0 && w1) {
        atomicMax(&box[0], w0);
        atomicMax(&box[1], w1);
        atomicMax(&box[2], w2);
        atomicMax(&box[3], w3);
    }
}

__device__ __forceinline__ uint32_t rx_hash(unsigned long long k) {  // the 64-bit finaliser of MurmurHash3
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (uint32_t)k;
}

// A value every lane of the wave holds alike, back in scalar registers: FP64 arithmetic runs on the vector unit, and what
// it computes from wave-uniform records would otherwise live in vector registers across the collider's whole rule.
__device__ __forceinline__ double rx_uniform(double v) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

// Step 5c of the relaxed pass: position-based Coulomb friction of the collider that has just projected the particle to
// `out`.  (nx, ny) and pen are the projection's normal and the depth it corrected, pv the particle's position at the
// start of the sub-step, h the sub-step.  The tangential part of the displacement relative to the surface is removed:
// all of it up to friction * pen (stick), that much of it beyond (slide).  Every comparison is false for a NaN.  Returns
// 1 for an application, 0 when the surface has no friction or there is no tangential displacement.
__device__ __forceinline__ int rx_grip(const EggSurface &sf, double h, double2 pv, double nx, double ny, double pen,
                                       double2 &out) {
    if (!(sf.friction > 0.0)) return 0;
    const double ex = (out.x - pv.x) - h * sf.vx;
    const double ey = (out.y - pv.y) - h * sf.vy;
    const double dn = ex * nx + ey * ny;
    const double tx = ex - dn * nx;
    const double ty = ey - dn * ny;
    const double tl2 = tx * tx + ty * ty;
    if (!(tl2 > 0.0)) return 0;
    const double tl = sqrt(tl2);
    const double lim = sf.friction * pen;
    if (tl <= lim) {  // stick
        out.x = out.x - tx;
        out.y = out.y - ty;
    } else {  // slide
        const double f = lim / tl;
        out.x = out.x - tx * f;
        out.y = out.y - ty * f;
    }
    return 1;
}

// Step 5c against a turning collider: the surface's velocity at the point `at` the projection has just produced, about the
// pivot (Px, Py) of the sub-step's end.  sf.vx / sf.vy already hold the surface's velocity plus the motion's.
__device__ __forceinline__ EggSurface rx_turning(const EggSurface &sf, double omega, double Px, double Py, const double2 &at) {
    EggSurface w = sf;
    w.vx = sf.vx - omega * (at.y - Py);
    w.vy = sf.vy + omega * (at.x - Px);
    return w;
}

// The start pv of the sub-step carried along with a turning wall by one sub-step: about the pivot where it was at the
// sub-step's start, to the pivot (Px, Py) of its end.  The records are read here once more: nothing of them stays in
// registers over the collider's whole rule.
__device__ __forceinline__ double2 rx_carried(const EggRxSpinFields *Sp, const EggRxMotionFields *Mo, int c, double Px, double Py,
                                              double2 pv) {
    const EggSpin sp = Sp->list[c];
    const EggMotion mo = Mo->list[c];
    const double2 hcs = Sp->hcs[c];  // one sub-step's turn
    const double psx = rx_uniform(sp.px + Sp->ts * mo.vx), psy = rx_uniform(sp.py + Sp->ts * mo.vy);
    const double ux = pv.x - psx, uy = pv.y - psy;
    return make_double2(Px + (hcs.x * ux - hcs.y * uy), Py + (hcs.y * ux + hcs.x * uy));
}

// Collider loads ("Collider loads"): what collider c has just done to the wave's particles, added to
// its three sums.  Every lane of the wave calls it (the loads instantiation runs the colliders where the wave is converged);
// `counts` is this lane's: a particle of this device that the collider has moved and whose inverse mass exceeds eps.  (bx, by)
// is the position that entered the collider's rule, `at` the one that left it, im the inverse mass, (Px, Py) the pivot.  A wave in
// which nothing counts returns at once; any other reduces the three integers across its lanes (integer addition: no order)
// and lane 0 adds them with one atomic each.
__device__ __forceinline__ void rx_tally(const EggRxLoadFields &Ld, int c, bool counts, double im, double bx, double by,
                                         const double2 &at, double Px, double Py) {
    if (__ballot(counts) == 0ull) return;
    const double m = 1.0 / im;
    const double ux = m * (bx - at.x);
    const double uy = m * (by - at.y);
    const double uz = (at.x - Px) * uy - (at.y - Py) * ux;
    const double fx = ux * EGG_RX_LOAD_SCALE_IMPULSE, fy = uy * EGG_RX_LOAD_SCALE_IMPULSE, fz = uz * EGG_RX_LOAD_SCALE_TORQUE;
    // (every comparison is false for a NaN: such a contribution is dropped)
    const bool ok = counts && fabs(fx) < EGG_RX_LOAD_LIMIT && fabs(fy) < EGG_RX_LOAD_LIMIT && fabs(fz) < EGG_RX_LOAD_LIMIT;
    long long qx = llrint(ok ? fx : 0.0), qy = llrint(ok ? fy : 0.0), qz = llrint(ok ? fz : 0.0);
    const bool some = __ballot(ok) != 0ull;
    const int dropped = __popcll(__ballot(counts && !ok));
    if (some) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            qx += __shfl_xor(qx, d, 64);
            qy += __shfl_xor(qy, d, 64);
            qz += __shfl_xor(qz, d, 64);
        }
    }
    if ((threadIdx.x & 63) == 0) {
        if (some) {
            atomicAdd(&Ld.sums[3 * c + 0], (unsigned long long)qx);
            atomicAdd(&Ld.sums[3 * c + 1], (unsigned long long)qy);
            atomicAdd(&Ld.sums[3 * c + 2], (unsigned long long)qz);
        }
        if (dropped) atomicAdd(Ld.dropped, (unsigned long long)dropped);
    }
}

// Step 5b of the relaxed pass: the colliders of the list whose mask covers the type, in list order, each on the result
// of the one before it.  i: the particle's key (picks the way out of a disc's centre); r: its radius.  Every lane of a
// wave reads the same record and takes the same branch on its kind.  Every comparison is false for a NaN: such a
// position stays.  Returns the colliders that moved the particle.
// S: step 5c, the surface of a collider that has just moved the particle (rx_grip); pv is the particle's position at the
// start of the sub-step, grips counts the applications.  The surface record is read like the collider record.
// W (with S only): the list may hold walls.  A wall is a segment whose first question is whether the straight path from pv
// to the position now meets it: then the particle goes back to its radius from the nearest point, on pv's side.  pv does
// not change inside a sub-step, so every pass sweeps from the same start.
// Mo (with W only; M below): every collider may move (egg_set_collider_motion; DESIGN.md section 2.7, "Collider motion").
// The switch is the pointer: every kernel passes either nullptr or the address of its own argument, so after inlining M is
// a constant and an instantiation without motion holds none of it.  (A sixth template parameter would put the gather's
// body one call deeper, and the four *_col_kernel instantiations then come out scheduled differently.)  The motion record
// is read like the collider record; the parameters of the sub-step's end are computed once per collider, in front of the
// branch on its kind, and go back to scalar registers (rx_uniform); a wall sweeps from pv carried along with it by one
// sub-step; step 5c takes the surface's velocity plus the motion's and reads the true pv.
// P (with Mo only; Sp): every collider may turn (egg_set_collider_spin; DESIGN.md section 2.7, "Collider spin").  Here the
// switch is a template parameter, picked by rx_gather from its own pointer: read from the pointer in this function, as M
// is, it left one addition of the wall and motion instantiations with its operands exchanged.  `turns` is the collider's
// own omega != 0, alike in every lane: such a collider takes the spin rule, whose primed parameters also go back to
// scalar registers; any other takes the motion rule as it stands.  Only the carried start of a turning wall and the
// surface's velocity at the contact point are per lane.
// L (with P only; Ld): the loads instantiation (egg_set_collider_loads; DESIGN.md section 2.7, "Collider loads"), which
// stands in for every flavour: whether the motion rule runs and whether a collider may turn are then words of Ld, alike in
// every lane, so that it evaluates the expressions of the flavour the handle would launch without loads.  Every lane of the
// wave is in here (one without a particle holds a NaN position, which no collider moves); `free` is the lane's: it holds a
// particle whose inverse mass im exceeds eps.  After each collider's rule, grip included, rx_tally adds what it did.
template <bool S, bool W, bool P, bool L = false>
__device__ __forceinline__ int rx_collide(const EggRxColliderFields &Co, const EggRxSurfaceFields &Su, const EggRxMotionFields *Mo,
                                          const EggRxSpinFields *Sp, int i, double r, double2 pv, double2 &out, int &grips,
                                          const EggRxLoadFields *Ld = nullptr, bool free = false, double im = 0.0) {
    const bool M = W && (L ? Ld->moving != 0 || Ld->turning != 0 : Mo != nullptr);
    static_assert(W || !P, "the spin instantiations are wall instantiations");
    static_assert(P || !L, "the loads instantiations are spin instantiations");
    int hits = 0;
    for (int c = 0; c < Co.count; ++c) {
        EggCollider col = Co.list[c];
        if (!(col.type_mask & Co.type_bit)) continue;
        EggSurface sf{};
        if (S) sf = Su.list[c];
        const int before = hits;                // (L: the hits in front of this collider)
        double LPx = 0.0, LPy = 0.0;            // (L: the pivot the torque is about)
        if (L && Ld->pivots) {                  // the spin record's pivot riding on the motion, as step 5b computes it
            const EggSpin sp = Sp->list[c];
            double ox = 0.0, oy = 0.0;
            if (M) {
                const EggMotion mo = Mo->list[c];
                ox = Mo->t * mo.vx;
                oy = Mo->t * mo.vy;
            }
            LPx = rx_uniform(sp.px + ox);
            LPy = rx_uniform(sp.py + oy);
        }
        bool turns = false;  // (P: this collider's omega is not zero; alike in every lane)
        double omega = 0.0, Px = 0.0, Py = 0.0;  // (P, read when it turns: the spin, the pivot at the sub-step's end)
        double hvx = 0.0, hvy = 0.0;  // (M: how far the collider carries the sub-step's start along, what a moving wall sweeps from)
        if (M) {  // the geometry at the end of the pass's sub-step, once per collider; step 5c adds the motion to the surface's velocity
            const EggMotion mo = Mo->list[c];
            const double ox = Mo->t * mo.vx, oy = Mo->t * mo.vy;
            if (P && (!L || Ld->turning)) {
                const EggSpin sp = Sp->list[c];
                turns = ((unsigned long long)__double_as_longlong(sp.omega) << 1) != 0ull;  // (omega != 0, on the scalar unit)
                if (turns) {  // about the pivot, which rides on the motion; (c, s) of the sub-step's end from the host's table
                    const double2 cs = Sp->cs[c];
                    omega = sp.omega;
                    Px = rx_uniform(sp.px + ox);
                    Py = rx_uniform(sp.py + oy);
                    if (col.kind == EGG_RX_COLLIDER_HALF_PLANE) {  // the pivot's signed distance to the plane is kept
                        const double keep = col.p[2] - (col.p[0] * sp.px + col.p[1] * sp.py);
                        const double nx = rx_uniform(cs.x * col.p[0] - cs.y * col.p[1]);
                        const double ny = rx_uniform(cs.y * col.p[0] + cs.x * col.p[1]);
                        col.p[0] = nx;
                        col.p[1] = ny;
                        col.p[2] = rx_uniform((nx * Px + ny * Py) + keep);
                    } else {
                        const double rx = col.p[0] - sp.px, ry = col.p[1] - sp.py;
                        col.p[0] = rx_uniform(Px + (cs.x * rx - cs.y * ry));
                        col.p[1] = rx_uniform(Py + (cs.y * rx + cs.x * ry));
                        if (col.kind == EGG_RX_COLLIDER_SEGMENT || col.kind == EGG_RX_COLLIDER_WALL) {
                            const double qx = col.p[2] - sp.px, qy = col.p[3] - sp.py;
                            col.p[2] = rx_uniform(Px + (cs.x * qx - cs.y * qy));
                            col.p[3] = rx_uniform(Py + (cs.y * qx + cs.x * qy));
                        }
                    }
                }
            }
            if (P && turns) {
                // (primed above)
            } else if (col.kind == EGG_RX_COLLIDER_HALF_PLANE) {
                col.p[2] = rx_uniform(col.p[2] + (col.p[0] * ox + col.p[1] * oy));
            } else {
                col.p[0] = rx_uniform(col.p[0] + ox);
                col.p[1] = rx_uniform(col.p[1] + oy);
                if (col.kind == EGG_RX_COLLIDER_SEGMENT || col.kind == EGG_RX_COLLIDER_WALL) {
                    col.p[2] = rx_uniform(col.p[2] + ox);
                    col.p[3] = rx_uniform(col.p[3] + oy);
                }
            }
            hvx = rx_uniform(Su.sub_delta * mo.vx);
            hvy = rx_uniform(Su.sub_delta * mo.vy);
            sf.vx = rx_uniform(sf.vx + mo.vx);
            sf.vy = rx_uniform(sf.vy + mo.vy);
        }
        const double2 pw = M ? (P && turns && col.kind == EGG_RX_COLLIDER_WALL ? rx_carried(Sp, Mo, c, Px, Py, pv)
                                                                               : make_double2(pv.x + hvx, pv.y + hvy))
                             : pv;
        const double x = out.x, y = out.y;
        if (col.kind == EGG_RX_COLLIDER_HALF_PLANE) {  // p = (nx, ny, off): keeps n . pos - off >= r
            const double s = (col.p[0] * x + col.p[1] * y) - (col.p[2] + r);
            if (s < 0.0) {
                out.x = x - s * col.p[0];
                out.y = y - s * col.p[1];
                ++hits;
                if (S) grips += rx_grip(P && turns ? rx_turning(sf, omega, Px, Py, out) : sf, Su.sub_delta, pv, col.p[0], col.p[1], -s, out);
            }
            if (L) rx_tally(*Ld, c, free && hits != before, im, x, y, out, LPx, LPy);
            continue;
        }
        double cx = col.p[0], cy = col.p[1], R = col.p[2];
        bool caught = false;         // (W only: the particle's path over the sub-step has crossed the wall)
        double a0 = 0.0, l2 = 0.0;   // (W only, read when caught: the side of pv, the wall's squared length)
        if (col.kind == EGG_RX_COLLIDER_SEGMENT || (W && col.kind == EGG_RX_COLLIDER_WALL)) {
            // p = (x0, y0, x1, y1): a disc of radius 0 at the nearest point
            const double ex = col.p[2] - col.p[0], ey = col.p[3] - col.p[1];
            l2 = ex * ex + ey * ey;
            double t = l2 == 0.0 ? 0.0 : ((x - col.p[0]) * ex + (y - col.p[1]) * ey) / l2;
            if (t < 0.0) t = 0.0;
            if (t > 1.0) t = 1.0;
            cx = col.p[0] + t * ex;
            cy = col.p[1] + t * ey;
            R = 0.0;
            if (W && col.kind == EGG_RX_COLLIDER_WALL) {  // the sweep: which side the sub-step started on, which side now
                a0 = ex * (pw.y - col.p[1]) - ey * (pw.x - col.p[0]);
                const double a1 = ex * (y - col.p[1]) - ey * (x - col.p[0]);
                if ((a0 > 0.0 && a1 <= 0.0) || (a0 < 0.0 && a1 >= 0.0)) {  // (a0 != 0, so l2 != 0)
                    const double u = a0 / (a0 - a1);
                    const double hx = pw.x + u * (x - pw.x), hy = pw.y + u * (y - pw.y);  // where the path meets the line
                    const double tc = ((hx - col.p[0]) * ex + (hy - col.p[1]) * ey) / l2;
                    caught = tc >= 0.0 && tc <= 1.0;  // ... and that is on the wall
                }
            }
        }
        const double dx = x - cx, dy = y - cy;
        const double d2 = dx * dx + dy * dy;
        if (col.kind == EGG_RX_COLLIDER_CONTAINER) {  // p = (cx, cy, R): stays inside
            double m = R - r;
            if (m < 0.0) m = 0.0;
            if (d2 > m * m) {
                const double d = sqrt(d2);
                out.x = cx + (dx / d) * m;
                out.y = cy + (dy / d) * m;
                ++hits;
                if (S) grips += rx_grip(P && turns ? rx_turning(sf, omega, Px, Py, out) : sf, Su.sub_delta, pv, dx / d, dy / d, d - m, out);
            }
        } else {  // disc, p = (cx, cy, R): stays outside
            const double m = R + r;
            if ((W && caught) || d2 < m * m) {
                const double d = sqrt(d2);
                double ux, uy, pen;
                if (W && caught) {  // back to its radius from the nearest point, along the unit normal towards pv's side
                    const double l = sqrt(l2);
                    const double ex = col.p[2] - col.p[0], ey = col.p[3] - col.p[1];
                    ux = a0 > 0.0 ? (-ey) / l : ey / l;
                    uy = a0 > 0.0 ? ex / l : (-ex) / l;
                    pen = m + d;
                } else {
                    if (d2 == 0.0) {
                        ux = kRxDirX[i & 7];
                        uy = kRxDirY[i & 7];
                    } else {
                        ux = dx / d;
                        uy = dy / d;
                    }
                    pen = m - d;
                }
                out.x = cx + ux * m;
                out.y = cy + uy * m;
                ++hits;
                if (S) grips += rx_grip(P && turns ? rx_turning(sf, omega, Px, Py, out) : sf, Su.sub_delta, pv, ux, uy, pen, out);
            }
        }
        if (L) rx_tally(*Ld, c, free && hits != before, im, x, y, out, LPx, LPy);
    }
    return hits;
}

// The force step in front of the pre-solve: the accelerations of the fields whose mask covers the type at the position ps
// the sub-step starts from, summed in list order, into the velocity v the pre-solve is about to damp.  A particle the
// follow constraint treats as immovable (!(im > eps)) takes none.  Every lane of a wave reads the same record and takes
// the same branch on its kind.  Every comparison is false for a NaN: such a position takes nothing from a bounded field.
__device__ __forceinline__ void rx_force(const EggRxForceFields &Fo, double sub_delta, double eps, double im, double2 ps,
                                         double2 &v) {
    if (!(im > eps)) return;
    double ax = 0.0, ay = 0.0;
    for (int c = 0; c < Fo.count; ++c) {
        const EggForce f = Fo.list[c];
        if (!(f.type_mask & Fo.type_bit)) continue;
        if (f.kind == EGG_RX_FORCE_UNIFORM) {  // p = (gx, gy)
            ax = ax + f.p[0];
            ay = ay + f.p[1];
            continue;
        }
        // radial and vortex, p = (cx, cy, strength, R): linear falloff down to 0 at R, nothing at the centre
        const double dx = f.p[0] - ps.x, dy = f.p[1] - ps.y;
        const double d2 = dx * dx + dy * dy;
        if (d2 < f.p[3] * f.p[3] && d2 > 0.0) {
            const double d = sqrt(d2);
            const double w = 1.0 - d / f.p[3];
            const double s = f.p[2] * w;
            if (f.kind == EGG_RX_FORCE_RADIAL) {  // towards the centre for a positive strength
                ax = ax + (dx / d) * s;
                ay = ay + (dy / d) * s;
            } else {  // vortex: along the radius turned by a quarter
                ax = ax + (-(dy / d)) * s;
                ay = ay + (dx / d) * s;
            }
        }
    }
    v.x = v.x + sub_delta * ax;
    v.y = v.y + sub_delta * ay;
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

// The kernels that take part in a device group come in two instantiations: G = false is the single handle's (the key
// is the index, no ghosts, no box; EggRelaxedArgs alone), G = true the group's (EggRelaxedGroupArgs; the flavoured
// kernels of either kind take EggRxPassArgs, see EGG_RX_PASS_KERNELS below).  The G = false
// instantiations compile to the same instructions as the kernels before groups existed.  (rx_insert and rx_gather
// take the arguments by value: by reference, the compiler schedules them differently.)
// F: the force fields act on the velocity before the pre-solve (rx_force); the F = false instantiations compile to the
// same instructions as the kernels before forces existed.
template <bool G, bool F>
__device__ __forceinline__ void rx_begin(const EggRelaxedArgs &A, const EggRxGroupFields &X, const EggRxForceFields &Fo) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    const bool live = i < A.n;
    if (!G && !live) return;
    double2 out = make_double2(0.0, 0.0);
    if (live) {
        const int atom = A.p_atom[i];
        const double2 ps = make_double2(A.x_in[i], A.y_in[i]);
        double2 v = make_double2(A.vx_in[i], A.vy_in[i]);
        if (F) rx_force(Fo, A.sub_delta, A.eps, A.inv_mass[i], ps, v);
        egg_pre_follow(A.damping, A.sub_delta, A.eps, A.follow_compliance, ps, v, A.inv_mass[i], A.atom_tx[atom],
                       A.atom_ty[atom], A.atom_fd[atom], out);
        A.prev[i] = ps;
        A.pos[i] = out;
    }
    if (G) rx_box(X.box, live, out, A.cell_size);
}

template <bool G, bool F>
__device__ __forceinline__ void rx_mid(const EggRelaxedArgs &A, const EggRxGroupFields &X, const EggRxForceFields &Fo) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    const bool live = i < A.n;
    if (!G && !live) return;
    double2 out = make_double2(0.0, 0.0);
    if (live) {
        const int atom = A.p_atom[i];
        const double2 ps = A.pos[i], pv = A.prev[i];
        double2 v = make_double2((ps.x - pv.x) / A.sub_delta, (ps.y - pv.y) / A.sub_delta);
        if (F) rx_force(Fo, A.sub_delta, A.eps, A.inv_mass[i], ps, v);
        egg_pre_follow(A.damping, A.sub_delta, A.eps, A.follow_compliance, ps, v, A.inv_mass[i], A.atom_tx[atom],
                       A.atom_ty[atom], A.atom_fd[atom], out);
        A.prev[i] = ps;
        A.pos[i] = out;
    }
    if (G) rx_box(X.box, live, out, A.cell_size);
}

// Start of a step: pre-solve + follow of the first sub-step from the committed state.
extern "C" __global__ void __launch_bounds__(256) egg_rx_begin_kernel(EggRelaxedArgs A) { rx_begin<false, false>(A, EggRxGroupFields{}, EggRxForceFields{}); }
extern "C" __global__ void __launch_bounds__(256) egg_rx_begin_group_kernel(EggRelaxedGroupArgs A) { rx_begin<true, false>(A.a, A.g, EggRxForceFields{}); }

// Between two sub-steps: post-solve of the one (L:1690-1693), pre-solve + follow of the next.
extern "C" __global__ void __launch_bounds__(256) egg_rx_mid_kernel(EggRelaxedArgs A) { rx_mid<false, false>(A, EggRxGroupFields{}, EggRxForceFields{}); }
extern "C" __global__ void __launch_bounds__(256) egg_rx_mid_group_kernel(EggRelaxedGroupArgs A) { rx_mid<true, false>(A.a, A.g, EggRxForceFields{}); }

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


// Entries of the pass: the local particles and, in a group, this pass's ghosts.
template <bool G>
__device__ __forceinline__ int rx_entries(const EggRelaxedArgs &A, const EggRxGroupFields &X) {
    return G ? A.n + (int)*X.n_ghost : A.n;
}

// Cell of every entry, its slot in the cell table, the slot's count.  (The table is at least twice as large as the
// entry count: a probe always ends.)
template <bool G>
__device__ __forceinline__ void rx_insert(EggRelaxedArgs A, const EggRxGroupFields &X) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= rx_entries<G>(A, X)) return;
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

// Every entry into its slot's range of grouped positions [hstart[h], hstart[h + 1]), in whatever order the atomics
// give, as its key (the counts are used up: nothing reads them afterwards).
template <bool G>
__device__ __forceinline__ void rx_scatter(const EggRelaxedArgs &A, const EggRxGroupFields &X) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= rx_entries<G>(A, X)) return;
    const int h = A.pslot[i];
    const uint32_t k = atomicSub(&A.hcount[h], 1u) - 1u;
    A.tmp[A.hstart[h] + k] = G ? X.ekey[i] : i;
}

// Inside a cell: ascending key (a particle's place = how many of its cell's particles have a smaller one), with the
// grouped copies of what the gather reads.  sidx holds the key; sloc (group only) the entry; stag (cohesive only) the
// batch tag.
template <bool G, bool K>
__device__ __forceinline__ void rx_rank(const EggRelaxedArgs &A, const EggRxGroupFields &X, const EggRxCohesionFields &Ch) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= rx_entries<G>(A, X)) return;
    const int key = G ? X.ekey[i] : i;
    const int h = A.pslot[i];
    const int st = (int)A.hstart[h], en = (int)A.hstart[h + 1];
    int rank = 0;
    for (int e = st; e < en; ++e) rank += A.tmp[e] < key ? 1 : 0;
    const int t = st + rank;
    A.sidx[t] = key;
    if (G) X.sloc[t] = i;
    A.spos[t] = A.pos[i];
    A.swr[t] = (!G || i < A.n) ? make_double2(A.inv_mass[i], A.radius[i]) : X.gwr[i - A.n];
    if (K) {
        if (!G || i < A.n) {
            const int atom = A.p_atom[i];
            Ch.stag[t] = Ch.atom_tag ? Ch.atom_tag[atom] : atom;
        } else {
            Ch.stag[t] = Ch.gtag[i - A.n];
        }
    }
}

// The relaxed pass of DESIGN.md section 2.7, one thread per grouped slot (threads of a wave share cells).  i is the
// key; in a group a ghost's slot gathers nothing (its own device moves it), and the gather records the box of what it
// writes when the pass is not the sub-step's last.  K: a pair that does not collide may cohere -- same tag, within reach
// -- and then runs the collision correction's arithmetic with the cohesion compliance (one path for both kinds).  D: the
// new position goes through the colliders before it is written (whether or not a pair fired).  S (with D only): a
// collider's surface acts right after its projection (step 5c); prev[me] is read once, for that.  W (with S only): the
// list may hold walls, which sweep from the same prev[me].  Mo (with W only): not null in the motion instantiations, whose
// colliders move (rx_collide).  Sp (with Mo only): not null in the spin instantiations, whose colliders turn besides.
// Ld (with Sp only; L below): not null in the loads instantiations (egg_rx_gather*_col_load_kernel), which also sum what
// every collider does to the particles.  The switch is the pointer, as Mo's is: after inlining L is a constant.  The sums
// are reduced across the wave, so there the colliders run behind the branch on the slot, where the wave is converged: a lane
// without a local particle brings a NaN position, which no collider moves, and writes nothing.
template <bool G, bool K, bool D, bool S, bool W>
__device__ __forceinline__ void rx_gather(EggRelaxedArgs A, const EggRxGroupFields &X, const EggRxCohesionFields &Ch,
                                          const EggRxColliderFields &Co, const EggRxSurfaceFields &Su,
                                          const EggRxMotionFields *Mo = nullptr, const EggRxSpinFields *Sp = nullptr,
                                          const EggRxLoadFields *Ld = nullptr) {
    static_assert(D || !S, "surfaces belong to colliders");
    static_assert(S || !W, "the wall instantiations are surface instantiations");
    const bool L = W && Ld != nullptr;
    bool have = false;     // (L only: the slot holds a local particle; li, lme, lwr, lout are its key, index, (w, r) and position)
    int li = 0, lme = 0;
    double2 lwr = make_double2(0.0, 0.0);
    double2 lout = make_double2(__longlong_as_double(0x7ff8000000000000ll), __longlong_as_double(0x7ff8000000000000ll));
    const int t = (int)(blockIdx.x * 256 + threadIdx.x);
    int pairs = 0;
    int cohered = 0;  // (K only)
    int hits = 0;     // (D only)
    int grips = 0;    // (S only)
    bool local = false;  // (group: the slot holds one of this device's particles; gout is its new position)
    double2 gout = make_double2(0.0, 0.0);
    if (G ? t < rx_entries<G>(A, X) && X.sloc[t] < A.n : t < A.n) {
        const int i = A.sidx[t];
        const int me = G ? X.sloc[t] : i;
        const double2 p = A.spos[t], wr = A.swr[t];
        const int32_t tag = K ? Ch.stag[t] : 0;
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
                    double compliance = A.collision_compliance;
                    if (!(d2 <= min_distance * min_distance)) {
                        if (!K) continue;
                        const double reach = Ch.factor * (ra + rb);
                        if (!(Ch.stag[e] == tag && d2 <= reach * reach)) continue;
                        compliance = Ch.compliance;  // cohesion: back to the collision distance, never closer
                        cohered += j > i ? 1 : 0;
                    }
                    ++n_fired;
                    const double divisor = wsum + compliance;
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
        if (D && !L) {
            const double2 pv = S ? A.prev[me] : make_double2(0.0, 0.0);
            hits = W && Sp != nullptr ? rx_collide<S, W, W>(Co, Su, Mo, Sp, i, wr.y, pv, out, grips)
                                      : rx_collide<S, W, false>(Co, Su, Mo, Sp, i, wr.y, pv, out, grips);
        }
        if (L) {
            have = true;
            li = i;
            lme = me;
            lwr = wr;
            lout = out;
        } else {
            A.pos_next[me] = out;
        }
        if (G) {
            local = true;
            gout = out;
        }
    }
    if (L) {  // every lane of the wave: the colliders and their loads
        const double2 pv = have ? A.prev[lme] : lout;
        hits = rx_collide<S, W, W, W>(Co, Su, Mo, Sp, li, lwr.y, pv, lout, grips, Ld, have && lwr.x > Ld->eps, lwr.x);
        if (have) A.pos_next[lme] = lout;
        if (G) gout = lout;
    }
    // pairs counted (each once: by its smaller key, on the device that holds it), one atomic per wave
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) pairs += __shfl_xor(pairs, d, 64);
    if ((threadIdx.x & 63) == 0 && pairs) atomicAdd(&A.status[1 + A.pass], (unsigned long long)pairs);
    if (K) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) cohered += __shfl_xor(cohered, d, 64);
        if ((threadIdx.x & 63) == 0 && cohered) atomicAdd(Ch.solves, (unsigned long long)cohered);
    }
    if (D) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) hits += __shfl_xor(hits, d, 64);
        if ((threadIdx.x & 63) == 0 && hits) atomicAdd(Co.hits, (unsigned long long)hits);
    }
    if (S) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) grips += __shfl_xor(grips, d, 64);
        if ((threadIdx.x & 63) == 0 && grips) atomicAdd(Su.grips, (unsigned long long)grips);
    }
    if (G && X.box) rx_box(X.box, local, gout, A.cell_size);
}

extern "C" __global__ void __launch_bounds__(256) egg_rx_insert_kernel(EggRelaxedArgs A) { rx_insert<false>(A, EggRxGroupFields{}); }
extern "C" __global__ void __launch_bounds__(256) egg_rx_insert_group_kernel(EggRelaxedGroupArgs A) { rx_insert<true>(A.a, A.g); }
extern "C" __global__ void __launch_bounds__(256) egg_rx_scatter_kernel(EggRelaxedArgs A) { rx_scatter<false>(A, EggRxGroupFields{}); }
extern "C" __global__ void __launch_bounds__(256) egg_rx_scatter_group_kernel(EggRelaxedGroupArgs A) { rx_scatter<true>(A.a, A.g); }
extern "C" __global__ void __launch_bounds__(256) egg_rx_rank_kernel(EggRelaxedArgs A) { rx_rank<false, false>(A, EggRxGroupFields{}, EggRxCohesionFields{}); }
extern "C" __global__ void __launch_bounds__(256) egg_rx_rank_group_kernel(EggRelaxedGroupArgs A) { rx_rank<true, false>(A.a, A.g, EggRxCohesionFields{}); }
// (the cohesive rank kernels and the 28 gathers: EGG_RX_PASS_KERNELS, expanded behind the viscosity pass)

// ---- collider bodies ----

// The integrator of collider bodies (egg_set_collider_bodies; DESIGN.md section 2.7, "Collider bodies"): one launch of one
// wave after the last pass of a sub-step of both types, lane k = collider k.  FP64 in exactly the order of the
// definition, no contraction: (1) the sub-step's impulse from the int64 sums, (2) the stored geometry and pivot become
// what the sub-step's gathers used at t = h -- the expressions of the host's advance_colliders, its omega != 0 branch
// included --, (3) the translation and (4) the rotation of a body, whose next turn is a Cayley rotation: only + - * /, so
// the host and the model agree with it to the bit.  Plain loads and stores; no atomics, no LDS.
extern "C" __global__ void __launch_bounds__(64) egg_rx_bodies_kernel(EggRxBodiesArgs A) {
    const int k = (int)threadIdx.x;
    if (k >= A.count) return;
    const double h = A.h;
    const EggBody b = A.bodies[k];
    EggCollider c = A.list[k];
    EggMotion m = A.motions[k];
    EggSpin sp = A.spins[k];
    double2 cs = A.cs[k];
    // 1. the impulse of the sub-step
    long long d[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const unsigned long long now = A.sums[3 * k + q];
        d[q] = (long long)(now - A.seen[3 * k + q]);
        A.seen[3 * k + q] = now;
    }
    const double Jx = ((double)d[0] / EGG_RX_LOAD_SCALE_IMPULSE) / h;
    const double Jy = ((double)d[1] / EGG_RX_LOAD_SCALE_IMPULSE) / h;
    const double Jz = ((double)d[2] / EGG_RX_LOAD_SCALE_TORQUE) / h;
    // 2. advance by what the sub-step used
    const double ox = h * m.vx, oy = h * m.vy;
    if (sp.omega != 0.0) {
        const double Px = sp.px + ox, Py = sp.py + oy;
        if (c.kind == EGG_RX_COLLIDER_HALF_PLANE) {
            const double keep = c.p[2] - (c.p[0] * sp.px + c.p[1] * sp.py);
            const double nx = cs.x * c.p[0] - cs.y * c.p[1], ny = cs.y * c.p[0] + cs.x * c.p[1];
            c.p[0] = nx;
            c.p[1] = ny;
            c.p[2] = (nx * Px + ny * Py) + keep;
        } else {
            const double rx = c.p[0] - sp.px, ry = c.p[1] - sp.py;
            c.p[0] = Px + (cs.x * rx - cs.y * ry);
            c.p[1] = Py + (cs.y * rx + cs.x * ry);
            if (c.kind == EGG_RX_COLLIDER_SEGMENT || c.kind == EGG_RX_COLLIDER_WALL) {
                const double qx = c.p[2] - sp.px, qy = c.p[3] - sp.py;
                c.p[2] = Px + (cs.x * qx - cs.y * qy);
                c.p[3] = Py + (cs.y * qx + cs.x * qy);
            }
        }
        sp.px = Px;
        sp.py = Py;
    } else if (c.kind == EGG_RX_COLLIDER_HALF_PLANE) {
        c.p[2] = c.p[2] + (c.p[0] * ox + c.p[1] * oy);
    } else {
        c.p[0] = c.p[0] + ox;
        c.p[1] = c.p[1] + oy;
        if (c.kind == EGG_RX_COLLIDER_SEGMENT || c.kind == EGG_RX_COLLIDER_WALL) {
            c.p[2] = c.p[2] + ox;
            c.p[3] = c.p[3] + oy;
        }
    }
    // 3. translation
    if (b.inv_mass > 0.0) {
        m.vx = m.vx + Jx * b.inv_mass;
        m.vy = m.vy + Jy * b.inv_mass;
        m.vx = m.vx + h * b.ax;
        m.vy = m.vy + h * b.ay;
        double f = 1.0 - h * b.drag;
        if (!(f > 0.0)) f = 0.0;
        m.vx = m.vx * f;
        m.vy = m.vy * f;
    }
    // 4. rotation
    if (b.inv_inertia > 0.0) {
        sp.omega = sp.omega + Jz * b.inv_inertia;
        double f = 1.0 - h * b.spin_drag;
        if (!(f > 0.0)) f = 0.0;
        sp.omega = sp.omega * f;
        const double u = 0.5 * (h * sp.omega);
        const double den = 1.0 + u * u;
        cs.x = (1.0 - u * u) / den;
        cs.y = (u + u) / den;
    }
    A.list[k] = c;
    A.motions[k] = m;
    A.spins[k] = sp;
    A.cs[k] = cs;
}

// ---- viscosity ----

// The viscous rank kernel: rx_rank's order inside a cell, with u = pos - prev of the entry in the grouped swr slot (a
// ghost's u arrived in its record).  A neighbour's inverse mass and radius are not needed in this pass.
template <bool G>
__device__ __forceinline__ void rx_rank_visc(const EggRelaxedArgs &A, const EggRxGroupFields &X) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= rx_entries<G>(A, X)) return;
    const int key = G ? X.ekey[i] : i;
    const int h = A.pslot[i];
    const int st = (int)A.hstart[h], en = (int)A.hstart[h + 1];
    int rank = 0;
    for (int e = st; e < en; ++e) rank += A.tmp[e] < key ? 1 : 0;
    const int t = st + rank;
    const double2 p = A.pos[i];
    A.sidx[t] = key;
    if (G) X.sloc[t] = i;
    A.spos[t] = p;
    if (!G || i < A.n) {
        const double2 pv = A.prev[i];
        A.swr[t] = make_double2(p.x - pv.x, p.y - pv.y);
    } else {
        A.swr[t] = X.gwr[i - A.n];
    }
}

// The viscosity pass (XSPH), one thread per grouped slot, candidates and visit order of rx_gather.  Every neighbour j
// within the cell size H adds w = 1 - d / H to sw and w (u_j - u_i) to (sx, sy); the particle's new displacement is
// u_i + c (s / sw), written as prev = p - that.  Neighbours are read from the grouped copies only and nothing reads another
// particle's prev: the write in place has no race.  A ghost's slot gathers nothing.  A pair is counted by the holder of
// its smaller key, one atomic per wave.
template <bool G>
__device__ __forceinline__ void rx_gather_visc(EggRelaxedArgs A, const EggRxGroupFields &X, const EggRxViscFields &V) {
    const int t = (int)(blockIdx.x * 256 + threadIdx.x);
    int pairs = 0;
    if (G ? t < rx_entries<G>(A, X) && X.sloc[t] < A.n : t < A.n) {
        const int i = A.sidx[t];
        const int me = G ? X.sloc[t] : i;
        const double2 p = A.spos[t], u = A.swr[t];
        const double H = A.cell_size, H2 = H * H;
        int32_t cx, cy;
        (void)rx_cell(p, A.cell_size, cx, cy);  // (a bad cell was flagged by the insert kernel)
        double sw = 0.0, sx = 0.0, sy = 0.0;
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
                    const double2 q = A.spos[e];
                    const double dx = q.x - p.x, dy = q.y - p.y;
                    const double d2 = dx * dx + dy * dy;
                    if (!(d2 < H2)) continue;
                    const double2 uq = A.swr[e];
                    pairs += j > i ? 1 : 0;
                    const double d = sqrt(d2);
                    const double w = 1.0 - d / H;
                    sw = sw + w;
                    sx = sx + w * (uq.x - u.x);
                    sy = sy + w * (uq.y - u.y);
                }
            }
        }
        if (A.inv_mass[me] > A.eps && sw > 0.0) {
            const double nux = u.x + V.c * (sx / sw), nuy = u.y + V.c * (sy / sw);
            A.prev[me] = make_double2(p.x - nux, p.y - nuy);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) pairs += __shfl_xor(pairs, d, 64);
    if ((threadIdx.x & 63) == 0 && pairs) atomicAdd(V.pairs, (unsigned long long)pairs);
}

extern "C" __global__ void __launch_bounds__(256) egg_rx_rank_visc_kernel(EggRelaxedArgs A) { rx_rank_visc<false>(A, EggRxGroupFields{}); }
extern "C" __global__ void __launch_bounds__(256) egg_rx_rank_group_visc_kernel(EggRelaxedGroupArgs A) { rx_rank_visc<true>(A.a, A.g); }

// ---- the flavoured kernels ----

// Every kernel of EGG_RX_PASS_KERNELS (eggsim_device.h), under its own name.  A column of a gather's row is a literal 0 or
// 1, so each wrapper hands rx_gather the constants the column stands for: an empty group, or no pointer at all.
#define EGG_RX_DEFINE_GATHER(name, G, K, flavour, D, S, W, Mo, Sp, Ld)                                                 \
    extern "C" __global__ void __launch_bounds__(256) name(EggRxPassArgs A) {                                          \
        rx_gather<G, K, D, S, W>(A.a, G ? A.g : EggRxGroupFields{}, K ? A.c : EggRxCohesionFields{},                    \
                                 D ? A.d : EggRxColliderFields{}, S ? A.s : EggRxSurfaceFields{}, Mo ? &A.m : nullptr, \
                                 Sp ? &A.r : nullptr, Ld ? &A.l : nullptr);                                            \
    }
#define EGG_RX_DEFINE_OTHER(name, ...) \
    extern "C" __global__ void __launch_bounds__(256) name(EggRxPassArgs A) { __VA_ARGS__; }
EGG_RX_PASS_KERNELS(EGG_RX_DEFINE_GATHER, EGG_RX_DEFINE_OTHER)
#undef EGG_RX_DEFINE_GATHER
#undef EGG_RX_DEFINE_OTHER

// ---- white-yolk coupling ----

// The coupling pass, one thread per grouped slot of the own type (threads of a wave share cells, so the walk over the
// other type's table is coherent).  Both tables were built at the shared cell size A.cell_size = H, so the 3x3 cells of
// the particle's own cell hold every particle of the other type within the coupling distance.  Candidates: the other
// type's particles in those cells, x offset outer, y offset inner, ascending key inside a cell.  Pair (a, b): a is the
// white particle, b the yolk one, whichever side evaluates it; the arithmetic is rx_gather's collision correction with
// min_distance = factor (ra + rb) and the coupling compliance.  The white side counts the pairs that fire, one atomic
// per wave.  Neighbours are read from grouped copies only; the move is written to pos_next.
// ADH (adhesion acts): a pair that does not couple may adhere -- same batch tag, within reach (ra + rb) -- and then runs
// the same arithmetic with the adhesion compliance: the target stays min_distance, so the pair is pulled together, never
// closer than the coupling distance.  A pair fires at most one of the two; the white side counts each kind in its own word.
template <bool ADH>
__device__ __forceinline__ void rx_couple(EggRelaxedArgs A, EggRxCoupleFields O, EggRxAdhesionFields Ad) {
    const int t = (int)(blockIdx.x * 256 + threadIdx.x);
    int solves = 0;
    int adhered = 0;  // (ADH only)
    if (t < A.n) {
        const int i = A.sidx[t];
        const double2 p = A.spos[t], wr = A.swr[t];
        const int32_t tag = ADH ? Ad.stag[t] : 0;
        const bool first = O.white_is_self != 0;
        int32_t cx, cy;
        (void)rx_cell(p, A.cell_size, cx, cy);  // (a bad cell was flagged by the insert kernel)
        double sx = 0.0, sy = 0.0;
        int n_fired = 0;
        for (int ox = -1; ox <= 1; ++ox) {
            for (int oy = -1; oy <= 1; ++oy) {
                const unsigned long long key = rx_key(cx + ox, cy + oy);
                uint32_t h = rx_hash(key) & O.table_mask;
                unsigned long long k;
                while ((k = O.hkey[h]) != key && k != EGG_RX_EMPTY_KEY) h = (h + 1) & O.table_mask;
                if (k == EGG_RX_EMPTY_KEY) continue;
                const int st = (int)O.hstart[h], en = (int)O.hstart[h + 1];
                for (int e = st; e < en; ++e) {
                    const int j = O.sidx[e];
                    const double2 q = O.spos[e], wq = O.swr[e];
                    const double2 pa = first ? p : q, pb = first ? q : p;
                    const double wa = first ? wr.x : wq.x, wb = first ? wq.x : wr.x;
                    const double ra = first ? wr.y : wq.y, rb = first ? wq.y : wr.y;
                    const double wsum = wa + wb;
                    if (wsum < O.eps) continue;
                    const double dx = pb.x - pa.x, dy = pb.y - pa.y;
                    const double d2 = dx * dx + dy * dy;
                    const double min_distance = O.factor * (ra + rb);
                    bool adheres = false;
                    if (!(d2 <= min_distance * min_distance)) {
                        if (!ADH) continue;
                        const double reach = Ad.reach * (ra + rb);
                        if (!(Ad.other_stag[e] == tag && d2 <= reach * reach)) continue;
                        adheres = true;  // adhesion: back to the coupling distance, never closer
                    }
                    ++n_fired;
                    if (ADH && adheres)
                        adhered += first ? 1 : 0;
                    else
                        solves += first ? 1 : 0;
                    const double divisor = wsum + (ADH && adheres ? Ad.compliance : O.compliance);
                    if (divisor < O.eps) {
                        sx = sx + 0.0;
                        sy = sy + 0.0;
                        continue;
                    }
                    const double current = sqrt(d2);
                    const double violation = current - min_distance;
                    double nx, ny;
                    if (d2 == 0.0) {  // coincident: by the two keys, b - a = yolk key - white key
                        const int k8 = (first ? j - i : i - j) & 7;
                        nx = kRxDirX[k8];
                        ny = kRxDirY[k8];
                    } else if (current < O.eps) {
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
    if (O.white_is_self) {  // (uniform over the launch)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) solves += __shfl_xor(solves, d, 64);
        if ((threadIdx.x & 63) == 0 && solves) atomicAdd(O.solves, (unsigned long long)solves);
        if (ADH) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) adhered += __shfl_xor(adhered, d, 64);
            if ((threadIdx.x & 63) == 0 && adhered) atomicAdd(Ad.solves, (unsigned long long)adhered);
        }
    }
}

extern "C" __global__ void __launch_bounds__(256) egg_rx_couple_kernel(EggRelaxedCoupleArgs K) { rx_couple<false>(K.a, K.c, EggRxAdhesionFields{}); }
extern "C" __global__ void __launch_bounds__(256) egg_rx_couple_adh_kernel(EggRelaxedCoupleAdhArgs K) { rx_couple<true>(K.a, K.c, K.d); }

// ---- yolk containment ----

// wsum of the rule: lane l has added v[o + l], v[o + l + 64], ... in ascending order into an accumulator that started at
// +0.0; the butterfly a[l] = a[l] + a[l ^ d], d = 32 .. 1, leaves the same bits in every lane (IEEE addition commutes).
__device__ __forceinline__ double rx_wsum(double a) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) a = a + __shfl_xor(a, d, 64);
    return a;
}

// The summary of every white atom for one sub-step: one wave per atom, four atoms per workgroup.  Two phases over the
// atom's positions, lane l reading entries l, l + 64, ... (neighbouring lanes read neighbouring double2): the sums of x
// and y, then the sum of the squared distances from the centroid.  cx = wsum(x) / n, cy = wsum(y) / n,
// L = factor * sqrt(wsum(q) / n); an empty atom contains nothing: L = +inf (the rule defines it; egg_add and
// egg_import_batch refuse a batch without particles of a type, so no scene reaches it).
extern "C" __global__ void __launch_bounds__(256) egg_rx_contain_sum_kernel(EggRxContainSumArgs K) {
    const int a = (int)(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (a >= K.n_atoms) return;  // (uniform over the wave)
    const int l = (int)(threadIdx.x & 63);
    const int o = K.atom_offset[a], n = K.atom_count[a];
    double ax = 0.0, ay = 0.0;
    for (int k = l; k < n; k += 64) {
        const double2 p = K.pos[o + k];
        ax = ax + p.x;
        ay = ay + p.y;
    }
    const double cx = rx_wsum(ax) / (double)n;
    const double cy = rx_wsum(ay) / (double)n;
    double aq = 0.0;
    for (int k = l; k < n; k += 64) {
        const double2 p = K.pos[o + k];
        aq = aq + ((p.x - cx) * (p.x - cx) + (p.y - cy) * (p.y - cy));
    }
    const double rho = sqrt(rx_wsum(aq) / (double)n);
    if (l == 0) {
        double *s = K.summary + 3 * (size_t)a;
        s[0] = cx;
        s[1] = cy;
        s[2] = n == 0 ? __builtin_inf() : K.factor * rho;
    }
}

// The projection: one thread per local yolk particle.  A particle farther than L from the centroid of its batch's white
// goes to keep = L + (1 - strength) (d - L) from it, along the same ray, in place; every comparison is false for a NaN.
// The projections are counted, one atomic per wave.  G (the halo paths): the cell of every position written is folded
// into the cell box of the sub-step's first pass, which the begin / mid kernel has just filled -- a superset of the true
// box, and extra ghosts are never visited.
template <bool G>
__device__ __forceinline__ void rx_contain(const EggRxContainArgs &K) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    int hits = 0;
    double2 out = make_double2(0.0, 0.0);
    if (i < K.n) {
        const double *s = K.summary + 3 * (size_t)K.p_atom[i];
        const double cx = s[0], cy = s[1], L = s[2];
        const double2 p = K.pos[i];
        const double dx = p.x - cx, dy = p.y - cy;
        const double d = sqrt(dx * dx + dy * dy);
        if (d > L) {  // (d > L >= 0, so d > 0)
            const double keep = L + (1.0 - K.strength) * (d - L);
            const double f = keep / d;
            out = make_double2(cx + dx * f, cy + dy * f);
            K.pos[i] = out;
            hits = 1;
        }
    }
    const bool wrote = hits != 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) hits += __shfl_xor(hits, d, 64);
    if ((threadIdx.x & 63) == 0 && hits) atomicAdd(K.hits, (unsigned long long)hits);
    if (G) rx_box(K.box, wrote, out, K.cell_size);
}

extern "C" __global__ void __launch_bounds__(256) egg_rx_contain_kernel(EggRxContainArgs K) { rx_contain<false>(K); }
extern "C" __global__ void __launch_bounds__(256) egg_rx_contain_group_kernel(EggRxContainArgs K) { rx_contain<true>(K); }

// ---- device groups ----

// global key of every local particle: abase[atom] = particles of the type in the group's batches with smaller ids
extern "C" __global__ void __launch_bounds__(256) egg_rx_gkey_kernel(const int32_t *p_atom, const int32_t *atom_offset,
                                                                     const int32_t *abase, int n, int32_t *ekey) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    const int a = p_atom[i];
    ekey[i] = abase[a] + (i - atom_offset[a]);
}

// Sender: every local particle whose cell lies in a receiver's cell box grown by one cell on each side goes into that
// receiver's send buffer, in any order (the receiver's rank kernel orders by key).  At most one record per particle
// and receiver: a buffer of capacity n cannot overflow.
extern "C" __global__ void __launch_bounds__(256) egg_rx_pack_kernel(EggRxPackArgs P) {
    __shared__ long long bx[EGG_RX_MAX_GROUP][4];  // lo x, hi x, lo y, hi y, grown
    if (threadIdx.x < (unsigned)P.n_recv) {
        const unsigned long long *b = P.box[threadIdx.x];
        const unsigned long long w0 = b[0], w1 = b[1], w2 = b[2], w3 = b[3];
        if (w1 == 0) {  // the receiver wrote no position: nothing is near it
            bx[threadIdx.x][0] = bx[threadIdx.x][2] = 1;
            bx[threadIdx.x][1] = bx[threadIdx.x][3] = 0;
        } else {
            bx[threadIdx.x][0] = (long long)((1ull << 32) - w0) - EGG_RX_BOX_BIAS - 1;
            bx[threadIdx.x][1] = (long long)w1 - EGG_RX_BOX_BIAS + 1;
            bx[threadIdx.x][2] = (long long)((1ull << 32) - w2) - EGG_RX_BOX_BIAS - 1;
            bx[threadIdx.x][3] = (long long)w3 - EGG_RX_BOX_BIAS + 1;
        }
    }
    __syncthreads();
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    const bool live = i < P.n;
    int32_t cx = 0, cy = 0;
    double2 p = make_double2(0.0, 0.0);
    if (live) {
        p = P.pos[i];
        (void)rx_cell(p, P.cell_size, cx, cy);
    }
    for (int k = 0; k < P.n_recv; ++k) {
        const bool take = live && rx_in_box(bx[k], cx, cy);
        const int slot = rx_append(P.count[k], take);
        if (take) {
            EggGhost g;
            g.x = p.x;
            g.y = p.y;
            g.inv_mass = P.inv_mass[i];
            g.radius = P.radius[i];
            g.key = rx_key_word(P.ekey[i], P.p_atom, P.atom_tag, i);
            P.send[k][slot] = g;
        }
    }
}

// The viscosity pass's sender: the same selection -- the take test is shared (rx_in_box); the box decode is written out
// again, because behind a shared helper or as a template egg_rx_pack_kernel no longer compiles to the instructions it had --
// and the two payload words of a record carry u = pos - prev instead of inverse mass and radius.
extern "C" __global__ void __launch_bounds__(256) egg_rx_pack_visc_kernel(EggRxPackViscArgs V) {
    const EggRxPackArgs &P = V.p;
    __shared__ long long bx[EGG_RX_MAX_GROUP][4];  // lo x, hi x, lo y, hi y, grown
    if (threadIdx.x < (unsigned)P.n_recv) {
        const unsigned long long *b = P.box[threadIdx.x];
        const unsigned long long w0 = b[0], w1 = b[1], w2 = b[2], w3 = b[3];
        if (w1 == 0) {  // the receiver wrote no position: nothing is near it
            bx[threadIdx.x][0] = bx[threadIdx.x][2] = 1;
            bx[threadIdx.x][1] = bx[threadIdx.x][3] = 0;
        } else {
            bx[threadIdx.x][0] = (long long)((1ull << 32) - w0) - EGG_RX_BOX_BIAS - 1;
            bx[threadIdx.x][1] = (long long)w1 - EGG_RX_BOX_BIAS + 1;
            bx[threadIdx.x][2] = (long long)((1ull << 32) - w2) - EGG_RX_BOX_BIAS - 1;
            bx[threadIdx.x][3] = (long long)w3 - EGG_RX_BOX_BIAS + 1;
        }
    }
    __syncthreads();
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    const bool live = i < P.n;
    int32_t cx = 0, cy = 0;
    double2 p = make_double2(0.0, 0.0);
    if (live) {
        p = P.pos[i];
        (void)rx_cell(p, P.cell_size, cx, cy);
    }
    for (int k = 0; k < P.n_recv; ++k) {
        const bool take = live && rx_in_box(bx[k], cx, cy);
        const int slot = rx_append(P.count[k], take);
        if (take) {
            EggGhost g;
            g.x = p.x;
            g.y = p.y;
            const double2 pv = V.prev[i];
            g.inv_mass = p.x - pv.x;
            g.radius = p.y - pv.y;
            g.key = rx_key_word(P.ekey[i], P.p_atom, P.atom_tag, i);
            P.send[k][slot] = g;
        }
    }
}

// Receiver: the records every sender packed for it, appended to the ghost entries [n, n + n_ghost).  Grid: x over the
// largest sender capacity, y over the senders.
extern "C" __global__ void __launch_bounds__(256) egg_rx_unpack_kernel(EggRxUnpackArgs U) {
    const int s = (int)blockIdx.y;
    const int q = (int)(blockIdx.x * 256 + threadIdx.x);
    const int cnt = (int)*U.count[s];
    if ((int)(blockIdx.x * 256) >= cnt) return;  // (uniform over the workgroup)
    const bool take = q < cnt;
    const int slot = rx_append(U.n_ghost, take);
    if (take) {
        const EggGhost r = U.recs[s][q];
        U.pos[U.n + slot] = make_double2(r.x, r.y);
        U.gwr[slot] = make_double2(r.inv_mass, r.radius);
        U.ekey[U.n + slot] = (int32_t)r.key;
        if (U.gtag) U.gtag[slot] = (int32_t)(r.key >> 32);
    }
}
