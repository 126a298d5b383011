// Collider contacts of the relaxed step (egg_set_collider_contacts; DESIGN.md section 2.7, "Collider contacts"): the one
// kernel that lets a collider body meet the other colliders.  A translation unit of its own, so that eggsim_relaxed.hip and
// every kernel in it stay what they were; compiled like them with -ffp-contract=off.
//
// egg_rx_contacts_kernel runs once per sub-step of a step in which contacts act, one wave, directly behind
// egg_rx_bodies_kernel on the same stream, lane k = collider k.  Its inputs are what the integrator has just written: the
// stored geometry and pivots of the sub-step's end, the new velocities and spins.  It changes velocities, spins and turns
// only.  FP64 in exactly the order of tests/contact_model.py, + - * / sqrt only: host-free, and equal to the model to the bit.
//
// Cross-lane traffic goes through a small LDS copy, not through shuffles.  A lane walks the partners j = 0 .. count - 1 in
// ascending order, so j is uniform over the wave and every lane reads the SAME LDS address: one broadcast per read, no
// bank conflict by construction.  The same record through ds_bpermute would cost two 32-bit permutes per double and
// thirteen doubles per partner, all through the same LDS crossbar, and the iteration's velocities would have to be kept
// apart from the ones being written; the LDS copy separates them with two barriers of one wave.  The static part (geometry,
// pivot, weights, restitution: 12 doubles and a word per collider, 6.5 KiB for 64) is written once per launch, the three
// doubles that an iteration changes once per iteration.
#include <hip/hip_runtime.h>

#include "eggsim_device.h"

namespace {

// normals of a coincident pair, by (b - a) & 7: the eight unit vectors of the relaxed pair rule
#define EGG_RXC_S 0x1.6a09e667f3bcdp-1
__constant__ double kRxcDirX[8] = {1.0, EGG_RXC_S, 0.0, -EGG_RXC_S, -1.0, -EGG_RXC_S, 0.0, EGG_RXC_S};
__constant__ double kRxcDirY[8] = {0.0, EGG_RXC_S, 1.0, EGG_RXC_S, 0.0, -EGG_RXC_S, -1.0, -EGG_RXC_S};

struct RxcShape {  // what rule 2 reads of a collider
    int32_t kind;
    double p0, p1, p2, p3;
};

__device__ __forceinline__ void rxc_unit(double dx, double dy, double d2, double d, int k8, double &ux, double &uy) {
    if (d2 == 0.0) {
        ux = kRxcDirX[k8];
        uy = kRxcDirY[k8];
    } else {
        ux = dx / d;
        uy = dy / d;
    }
}

struct RxcCurve {  // a container with m = Rc - R > 0: what rule 3 bends the gap to its wall with
    bool on;
    bool disc_is_b;
    double ox, oy, m, d;
};

// Rule 2 for the colliders A, B at the indices a < b: the unit normal from a to b, the gap and the contact point; false
// where the shapes make no pair.
__device__ __forceinline__ bool rxc_geometry(int a, int b, const RxcShape &A, const RxcShape &B, double &nx, double &ny, double &g, double &px,
                                             double &py, RxcCurve &curve) {
    const int k8 = (b - a) & 7;
    curve.on = false;
    if (A.kind == EGG_RX_COLLIDER_DISC && B.kind == EGG_RX_COLLIDER_DISC) {
        const double dx = B.p0 - A.p0;
        const double dy = B.p1 - A.p1;
        const double d2 = dx * dx + dy * dy;
        const double d = sqrt(d2);
        rxc_unit(dx, dy, d2, d, k8, nx, ny);
        g = d - (A.p2 + B.p2);
        px = A.p0 + nx * A.p2;
        py = A.p1 + ny * A.p2;
        return true;
    }
    const bool disc_is_b = A.kind != EGG_RX_COLLIDER_DISC;
    if (disc_is_b && B.kind != EGG_RX_COLLIDER_DISC) return false;
    const RxcShape &D = disc_is_b ? B : A;
    const RxcShape &O = disc_is_b ? A : B;
    const double cx = D.p0, cy = D.p1, R = D.p2;
    double ux, uy;
    if (O.kind == EGG_RX_COLLIDER_HALF_PLANE) {
        ux = O.p0;
        uy = O.p1;
        g = (ux * cx + uy * cy) - (O.p2 + R);
        px = cx - ux * R;
        py = cy - uy * R;
    } else if (O.kind == EGG_RX_COLLIDER_CONTAINER) {
        const double dx = cx - O.p0;
        const double dy = cy - O.p1;
        const double d2 = dx * dx + dy * dy;
        const double d = sqrt(d2);
        double ox, oy;
        rxc_unit(dx, dy, d2, d, k8, ox, oy);
        g = (O.p2 - R) - d;
        if (O.p2 - R > 0.0) curve = RxcCurve{true, disc_is_b, ox, oy, O.p2 - R, d};
        ux = -ox;
        uy = -oy;
        px = cx + ox * R;
        py = cy + oy * R;
    } else if (O.kind == EGG_RX_COLLIDER_SEGMENT || O.kind == EGG_RX_COLLIDER_WALL) {
        const double ex = O.p2 - O.p0;
        const double ey = O.p3 - O.p1;
        const double l2 = ex * ex + ey * ey;
        double t = l2 == 0.0 ? 0.0 : ((cx - O.p0) * ex + (cy - O.p1) * ey) / l2;
        if (t < 0.0) t = 0.0;
        if (t > 1.0) t = 1.0;
        px = O.p0 + t * ex;
        py = O.p1 + t * ey;
        const double dx = cx - px;
        const double dy = cy - py;
        const double d2 = dx * dx + dy * dy;
        const double d = sqrt(d2);
        if (d2 == 0.0 && l2 != 0.0) {  // the centre lies on the segment: its left normal
            const double ln = sqrt(l2);
            ux = (-ey) / ln;
            uy = ex / ln;
        } else {
            rxc_unit(dx, dy, d2, d, k8, ux, uy);
        }
        g = d - R;
    } else {
        return false;
    }
    nx = disc_is_b ? ux : -ux;
    ny = disc_is_b ? uy : -uy;
    return true;
}

}  // namespace

extern "C" __global__ void __launch_bounds__(64) egg_rx_contacts_kernel(EggRxContactsArgs A) {
    __shared__ RxcShape s_shape[EGG_RX_MAX_CONTACT_LANES];
    __shared__ double s_pivot[EGG_RX_MAX_CONTACT_LANES][2];
    __shared__ double s_weight[EGG_RX_MAX_CONTACT_LANES][2];
    __shared__ double s_e[EGG_RX_MAX_CONTACT_LANES];
    __shared__ int32_t s_on[EGG_RX_MAX_CONTACT_LANES];
    __shared__ double s_vel[EGG_RX_MAX_CONTACT_LANES][3];  // (vx, vy, omega) at the iteration's start
    __shared__ unsigned long long s_fires[EGG_RX_MAX_CONTACT_LANES];
    const int k = (int)threadIdx.x;
    const int count = A.count < EGG_RX_MAX_CONTACT_LANES ? A.count : EGG_RX_MAX_CONTACT_LANES;
    const bool live = k < count;  // (no early return: every lane of the wave meets the barriers)
    const double h = A.h;
    RxcShape me{EGG_RX_COLLIDER_HALF_PLANE, 0.0, 0.0, 0.0, 0.0};
    double Px = 0.0, Py = 0.0, vx = 0.0, vy = 0.0, omega = 0.0, mk = 0.0, ik = 0.0, ek = 0.0;
    int32_t on = 0;
    if (live) {
        const EggCollider c = A.list[k];
        const EggMotion m = A.motions[k];
        const EggSpin sp = A.spins[k];
        const EggBody b = A.bodies[k];
        const EggContact ct = A.contacts[k];
        me = RxcShape{c.kind, c.p[0], c.p[1], c.p[2], c.p[3]};
        Px = sp.px;
        Py = sp.py;
        vx = m.vx;
        vy = m.vy;
        omega = sp.omega;
        mk = b.inv_mass;
        ik = b.inv_inertia;
        ek = ct.restitution;
        on = ct.on;
    }
    s_shape[k] = me;
    s_pivot[k][0] = Px;
    s_pivot[k][1] = Py;
    s_weight[k][0] = mk;
    s_weight[k][1] = ik;
    s_e[k] = ek;
    s_on[k] = on;
    unsigned long long fires = 0ull;
    for (int it = 0; it < A.iterations; ++it) {
        s_vel[k][0] = vx;
        s_vel[k][1] = vy;
        s_vel[k][2] = omega;
        __syncthreads();
        double sx = 0.0, sy = 0.0, sz = 0.0;
        int n_fired = 0;
        for (int j = 0; j < count; ++j) {  // ascending partner index; j is uniform, so every read below is one broadcast
            if (!s_on[j]) continue;
            if (!on || j == k) continue;
            const bool first = k < j;  // this lane is a
            const RxcShape other = s_shape[j];
            const double mj = s_weight[j][0], ij = s_weight[j][1];
            const double ma = first ? mk : mj, ia = first ? ik : ij, mb = first ? mj : mk, ib = first ? ij : ik;
            if (!(((ma + ia) + mb) + ib > 0.0)) continue;
            double nx, ny, g, px, py;
            RxcCurve curve;
            if (!(first ? rxc_geometry(k, j, me, other, nx, ny, g, px, py, curve) : rxc_geometry(j, k, other, me, nx, ny, g, px, py, curve))) continue;
            const double Pjx = s_pivot[j][0], Pjy = s_pivot[j][1];
            const double vjx = s_vel[j][0], vjy = s_vel[j][1], oj = s_vel[j][2];
            const double Pax = first ? Px : Pjx, Pay = first ? Py : Pjy, Pbx = first ? Pjx : Px, Pby = first ? Pjy : Py;
            const double vax = first ? vx : vjx, vay = first ? vy : vjy, oa = first ? omega : oj;
            const double vbx = first ? vjx : vx, vby = first ? vjy : vy, ob = first ? oj : omega;
            const double uax = vax - oa * (py - Pay), uay = vay + oa * (px - Pax);
            const double ubx = vbx - ob * (py - Pby), uby = vby + ob * (px - Pbx);
            if (curve.on) {  // the gap the tangential travel of the sub-step leaves along the circle
                const bool disc_mine = curve.disc_is_b != first;  // (this lane is b when it is not a)
                const RxcShape &D = disc_mine ? me : other;
                const RxcShape &Q = disc_mine ? other : me;
                const double dvx = disc_mine ? vx : vjx, dvy = disc_mine ? vy : vjy, dom = disc_mine ? omega : oj;
                const double dPx = disc_mine ? Px : Pjx, dPy = disc_mine ? Py : Pjy;
                const double qvx = disc_mine ? vjx : vx, qvy = disc_mine ? vjy : vy, qom = disc_mine ? oj : omega;
                const double qPx = disc_mine ? Pjx : Px, qPy = disc_mine ? Pjy : Py;
                const double udx = dvx - dom * (D.p1 - dPy), udy = dvy + dom * (D.p0 - dPx);
                const double ucx = qvx - qom * (Q.p1 - qPy), ucy = qvy + qom * (Q.p0 - qPx);
                const double vt = curve.ox * (udy - ucy) - curve.oy * (udx - ucx);
                const double s = h * vt;
                double q2 = curve.m * curve.m - s * s;
                if (q2 < 0.0) q2 = 0.0;
                g = sqrt(q2) - curve.d;
            }
            const double vn = nx * (ubx - uax) + ny * (uby - uay);
            const double ca = (px - Pax) * ny - (py - Pay) * nx;
            const double cb = (px - Pbx) * ny - (py - Pby) * nx;
            const double wa = ma + ia * (ca * ca);
            const double wb = mb + ib * (cb * cb);
            const double w = wa + wb;
            if (!(w > 0.0 && g + h * vn < 0.0)) continue;
            const double ej = s_e[j];
            const double ea = first ? ek : ej, eb = first ? ej : ek;
            const double e = ea > eb ? ea : eb;
            const double t1 = (-g) / h;
            const double t2 = -(e * vn);
            const double target = t1 > t2 ? t1 : t2;
            const double lam = (target - vn) / w;
            double Jx = lam * nx, Jy = lam * ny;
            if (first) {
                Jx = -Jx;
                Jy = -Jy;
                ++fires;  // (a fire is counted by the smaller index)
            }
            sx = sx + Jx;
            sy = sy + Jy;
            sz = sz + ((px - Px) * Jy - (py - Py) * Jx);
            ++n_fired;
        }
        __syncthreads();  // every lane has read the iteration's velocities before any is replaced
        if (n_fired > 0) {
            const double cnt = (double)n_fired;
            if (mk > 0.0) {
                vx = vx + (sx * mk) / cnt;
                vy = vy + (sy * mk) / cnt;
            }
            if (ik > 0.0) omega = omega + (sz * ik) / cnt;
        }
    }
    s_fires[k] = fires;
    __syncthreads();
    if (live) {
        A.motions[k] = EggMotion{vx, vy};
        A.spins[k] = EggSpin{Px, Py, omega};
        if (ik > 0.0) {  // the integrator's four lines, from the spin the contacts have left
            const double u = 0.5 * (h * omega);
            const double den = 1.0 + u * u;
            A.cs[k] = double2{(1.0 - u * u) / den, (u + u) / den};
        }
    }
    if (k == 0) {  // the step's fires so far: one lane, a plain load and a plain store (no other launch touches the word)
        unsigned long long total = A.solves[0];
        for (int j = 0; j < count; ++j) total += s_fires[j];
        A.solves[0] = total;
    }
}
