// eggsim_host_colliders.hip -- the colliders of the relaxed pass ("Colliders" and the subsections
// behind it): the entry points that set and return the list and the records per collider, and the ONE owner of their
// copies on the device.
//
// The rule: while the list is not empty, d_colliders, d_surfaces, d_motions and d_spins each hold exactly one record per
// collider -- the host's record where the host has one, the default or zero record where the host's vector is empty.
// sync_collider_records establishes it, prepare_step calls it once per relaxed step, and a table is copied only when its
// bit in egg_handle::collider_dirty is set.  Three places set bits: the setters below (they change a host copy), the commit
// of a step in which colliders move or turn (advance_colliders has advanced the host's list and pivots), and the
// preparation of a step in which bodies act (the integrator is about to rewrite the device's list, motions and spins;
// take_bodies clears those bits once the host has read them back, so a step that is not committed leaves them set).  The
// setters never touch the device: a refused or failed call cannot leave host and device apart.
#include "eggsim_host.h"

namespace egghost {

namespace {

const egg_collider_style kNoStyle{{0, 0, 0, 0}, {0, 0, 0, 0}, 0, 0};
const egg_collider_surface kNoSurface{0.0, 0.0, 0.0};
const egg_collider_motion kNoMotion{0.0, 0.0};
const egg_collider_spin kNoSpin{0.0, 0.0, 0.0};
const egg_collider_body kNoBody{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
const egg_collider_contact kNoContact{0.0, 0, 0};

// what a table holds: the host's n records, or n times `none` (in `fill`) while the host has none
template <class R>
const R *records_or(const std::vector<R> &host, size_t n, const R &none, std::vector<R> &fill) {
    if (!host.empty()) return host.data();
    fill.assign(n, none);
    return fill.data();
}

// The checks every setter of records per collider opens with, under the entry point's name: EGG_OK, or the refusal.
int check_records(egg_handle *h, const char *name, int32_t n, const void *records) {
    if (!h) return EGG_ERR_INVALID_ARGUMENT;
    REJECT_IN_FLIGHT(h, name);
    if (n != 0 && n != (int32_t)h->colliders.size())
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: n = %d, the list holds %d colliders (n is that, or 0)", name, (int)n, (int)h->colliders.size());
    if (n > 0 && !records) return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: n = %d without records", name, (int)n);
    return EGG_OK;
}

// The getters' answer: a record per collider, as stored, or `none` while nothing is stored.
template <class R>
int get_records(const egg_handle *h, std::vector<R> egg_handle::*stored, const R &none, int32_t cap, R *out, int32_t *n) {
    if (!h) return EGG_ERR_INVALID_ARGUMENT;
    const std::vector<R> &have = h->*stored;
    const int32_t count = (int32_t)h->colliders.size();
    if (n) *n = count;
    for (int32_t k = 0; out && k < std::min(cap, count); ++k) out[k] = have.empty() ? none : have[(size_t)k];
    return EGG_OK;
}

}  // namespace

int sync_collider_records(egg_handle *h) {
    const size_t n = h->colliders.size();
    const unsigned dirty = h->collider_dirty;
    if (n == 0 || dirty == 0) return EGG_OK;
    std::vector<egg_collider_surface> srf;
    std::vector<egg_collider_motion> mov;
    std::vector<egg_collider_spin> spn;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, h->d_colliders.reserve(EGG_MAX_COLLIDERS, false, nullptr));
    HIP_TRY(h, h->d_surfaces.reserve(EGG_MAX_COLLIDERS, false, nullptr));
    HIP_TRY(h, h->d_motions.reserve(EGG_MAX_COLLIDERS, false, nullptr));
    HIP_TRY(h, h->d_spins.reserve(EGG_MAX_COLLIDERS, false, nullptr));
    if (dirty & kDirtyList) HIP_TRY(h, hipMemcpy(h->d_colliders.p, h->colliders.data(), n * sizeof(egg_collider), hipMemcpyHostToDevice));
    if (dirty & kDirtySurfaces)
        HIP_TRY(h, hipMemcpy(h->d_surfaces.p, records_or(h->surfaces, n, kNoSurface, srf), n * sizeof(egg_collider_surface), hipMemcpyHostToDevice));
    if (dirty & kDirtyMotions)
        HIP_TRY(h, hipMemcpy(h->d_motions.p, records_or(h->motions, n, kNoMotion, mov), n * sizeof(egg_collider_motion), hipMemcpyHostToDevice));
    if (dirty & kDirtySpins)
        HIP_TRY(h, hipMemcpy(h->d_spins.p, records_or(h->spins, n, kNoSpin, spn), n * sizeof(egg_collider_spin), hipMemcpyHostToDevice));
    h->collider_dirty = 0;  // (a copy that failed has left every bit set: the next step tries again)
    return EGG_OK;
}

}  // namespace egghost

extern "C" {

// The list ("Colliders").  Everything is checked before anything changes: a refused call leaves the
// list, the records per collider and the counters as they were.
int egg_set_colliders(egg_handle *h, int32_t n, const egg_collider *c) {
    if (!h) return EGG_ERR_INVALID_ARGUMENT;
    REJECT_IN_FLIGHT(h, "egg_set_colliders");
    if (n < 0 || n > EGG_MAX_COLLIDERS)
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_set_colliders: n = %d, a list holds 0 .. %d colliders", (int)n, EGG_MAX_COLLIDERS);
    if (n > 0 && !c) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_set_colliders: n = %d without a list", (int)n);
    static_assert(sizeof(egg_collider) == 40 && sizeof(EggCollider) == sizeof(egg_collider), "a collider record is 40 bytes");
    static_assert(EGG_MAX_COLLIDERS == EGG_RX_MAX_COLLIDERS && EGG_COLLIDER_HALF_PLANE == EGG_RX_COLLIDER_HALF_PLANE &&
                      EGG_COLLIDER_DISC == EGG_RX_COLLIDER_DISC && EGG_COLLIDER_CONTAINER == EGG_RX_COLLIDER_CONTAINER &&
                      EGG_COLLIDER_SEGMENT == EGG_RX_COLLIDER_SEGMENT && EGG_COLLIDER_WALL == EGG_RX_COLLIDER_WALL,
                  "the kernel's collider constants are the ABI's");
    std::vector<egg_collider> list((size_t)n);
    bool wall = false;
    for (int32_t k = 0; k < n; ++k) {
        egg_collider &o = list[(size_t)k];
        o = c[k];
        static const char *const names[6] = {"half-plane", "disc", "container", "segment", "", "wall"};  // (4 is not a kind)
        if ((o.kind < EGG_COLLIDER_HALF_PLANE || o.kind > EGG_COLLIDER_SEGMENT) && o.kind != EGG_COLLIDER_WALL)
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_set_colliders: collider %d: unknown kind %d", (int)k, (int)o.kind);
        if (o.type_mask < 1 || o.type_mask > 3)
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_set_colliders: collider %d: type_mask %d (bit 0 white, bit 1 yolk, never 0)", (int)k,
                        (int)o.type_mask);
        const int used = o.kind == EGG_COLLIDER_SEGMENT || o.kind == EGG_COLLIDER_WALL ? 4 : 3;
        wall |= o.kind == EGG_COLLIDER_WALL;
        for (int q = 0; q < 4; ++q) {
            if (q >= used) o.p[q] = 0.0;  // (not a parameter of the kind)
            if (!std::isfinite(o.p[q]))
                return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_set_colliders: collider %d (%s): parameter %d is not finite", (int)k,
                            names[o.kind], q);
        }
        if ((o.kind == EGG_COLLIDER_DISC || o.kind == EGG_COLLIDER_CONTAINER) && o.p[2] < 0)
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_set_colliders: collider %d (%s): radius %g is negative", (int)k, names[o.kind], o.p[2]);
        if (o.kind == EGG_COLLIDER_HALF_PLANE) {  // the normal is normalised once, here
            const double len = std::sqrt(o.p[0] * o.p[0] + o.p[1] * o.p[1]);
            if (!(len >= h->sys[0].cfg.eps) || !std::isfinite(len))
                return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_set_colliders: collider %d (half-plane): the normal's length %g is below eps or not finite",
                            (int)k, len);
            o.p[0] = o.p[0] / len;
            o.p[1] = o.p[1] / len;
        }
    }
    if (n > 0 && h->opt_solver_order != EGG_SOLVER_RELAXED)
        return fail(h, EGG_ERR_UNSUPPORTED, "egg_set_colliders: colliders need relaxed order (EGG_OPT_SOLVER_ORDER = 1 first)");
    h->colliders.swap(list);
    h->collider_dirty = kDirtyAllTables;  // (a new list: every table holds the old one's records)
    h->colliders_last = h->colliders;  // (a teleport is not interpolated: the pose is the new list at every alpha)
    h->styles.clear();                 // (and nothing is drawn)
    h->colliders_wall = wall;
    h->surfaces.clear();  // (the indices no longer mean anything: every surface is the default again)
    h->surfaces_grip = false;
    h->motions.clear();  // (and every motion zero)
    h->motions_move = false;
    h->spins.clear();  // (and every spin)
    h->spins_turn = false;
    h->load_sums.assign(3 * h->colliders.size(), 0);  // (the loads belonged to the old list; the switch stays)
    h->load_dropped = 0;
    h->load_sub_delta = 0.0;
    h->bodies.clear();  // (and no collider is a body)
    h->bodies_any = false;
    h->contacts.clear();  // (and none meets another; the iterations and the counter stay)
    h->contacts_any = false;
    return EGG_OK;
}

int egg_get_colliders(const egg_handle *h, int32_t cap, egg_collider *c, int32_t *n) {
    if (!h) return EGG_ERR_INVALID_ARGUMENT;
    const int32_t have = (int32_t)h->colliders.size();
    if (n) *n = have;
    if (c && cap > 0) memcpy(c, h->colliders.data(), (size_t)std::min(cap, have) * sizeof(egg_collider));
    return EGG_OK;
}

// Collider styles ("Collider styles"): one record per collider, or none (nothing is drawn).  Host
// state only: a draw uploads what it draws.  Everything is checked before anything changes.
int egg_set_collider_styles(egg_handle *h, int32_t n, const egg_collider_style *st) {
    static_assert(sizeof(egg_collider_style) == 40, "a style record is 40 bytes");
    static_assert(EGG_MAX_COLLIDERS == EGG_DRAW_MAX_COLLIDERS, "one lane of a wave per collider");
    const int rc = check_records(h, "egg_set_collider_styles", n, st);
    if (rc != EGG_OK) return rc;
    std::vector<egg_collider_style> list((size_t)n);
    for (int32_t k = 0; k < n; ++k) {
        egg_collider_style &o = list[(size_t)k];
        o = st[k];
        for (int q = 0; q < 4; ++q) {
            if (!(o.fill[q] >= 0.0f && o.fill[q] <= 1.0f))  // (false for a NaN)
                return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_set_collider_styles: collider %d: fill component %d is %g, not in [0, 1]", (int)k, q,
                            (double)o.fill[q]);
            if (!(o.line[q] >= 0.0f && o.line[q] <= 1.0f))
                return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_set_collider_styles: collider %d: line component %d is %g, not in [0, 1]", (int)k, q,
                            (double)o.line[q]);
            o.fill[q] = o.fill[q] + 0.0f;  // (-0.0 is stored as +0.0: handles set alike compare alike)
            o.line[q] = o.line[q] + 0.0f;
        }
        if (!(o.line_width >= 0.0f && o.line_width <= 64.0f))
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_set_collider_styles: collider %d: line width %g is not in [0, 64]", (int)k,
                        (double)o.line_width);
        o.line_width = o.line_width + 0.0f;
        if (o.layer != 0 && o.layer != 1)
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_set_collider_styles: collider %d: layer %d (0 under the eggs, 1 over them)", (int)k,
                        (int)o.layer);
    }
    h->styles.swap(list);
    return EGG_OK;
}

int egg_get_collider_styles(const egg_handle *h, int32_t cap, egg_collider_style *st, int32_t *n) {
    return get_records(h, &egg_handle::styles, kNoStyle, cap, st, n);
}

// The pose a frame draws: the list at the start of the last committed step mixed with the current one.
int egg_get_collider_pose(egg_handle *h, double alpha, int32_t cap, egg_collider *c, int32_t *n) {
    if (!h) return EGG_ERR_INVALID_ARGUMENT;
    const int32_t have = (int32_t)h->colliders.size();
    if (n) *n = have;
    if (!c || cap <= 0 || have == 0) return EGG_OK;
    const double t = std::isnan(alpha) ? h->interpolation_alpha : clampd(alpha, 0, 1);
    std::vector<egg_collider> pose((size_t)have);
    collider_pose(h->colliders_last.data(), h->colliders.data(), have, t, pose.data());
    memcpy(c, pose.data(), (size_t)std::min(cap, have) * sizeof(egg_collider));
    return EGG_OK;
}

// Collider surfaces ("Collider surfaces"): one record per collider, or none (all default).
// Everything is checked before anything changes.
int egg_set_collider_surfaces(egg_handle *h, int32_t n, const egg_collider_surface *sf) {
    static_assert(sizeof(egg_collider_surface) == 24 && sizeof(EggSurface) == sizeof(egg_collider_surface), "a surface record is 24 bytes");
    const int rc = check_records(h, "egg_set_collider_surfaces", n, sf);
    if (rc != EGG_OK) return rc;
    std::vector<egg_collider_surface> list((size_t)n);
    bool grip = false;
    for (int32_t k = 0; k < n; ++k) {
        egg_collider_surface &o = list[(size_t)k];
        o = sf[k];
        if (!std::isfinite(o.friction) || o.friction < 0)
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_set_collider_surfaces: collider %d: friction %g is negative or not finite", (int)k,
                        o.friction);
        if (!std::isfinite(o.vx) || !std::isfinite(o.vy))
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_set_collider_surfaces: collider %d: the velocity (%g, %g) is not finite", (int)k, o.vx,
                        o.vy);
        o.friction = o.friction + 0.0;  // (-0.0 is stored as +0.0, in every field: handles set alike compare alike)
        o.vx = o.vx + 0.0;
        o.vy = o.vy + 0.0;
        grip |= o.friction > 0.0;
    }
    h->surfaces.swap(list);
    h->surfaces_grip = grip;
    h->collider_dirty |= kDirtySurfaces;
    return EGG_OK;
}

int egg_get_collider_surfaces(const egg_handle *h, int32_t cap, egg_collider_surface *sf, int32_t *n) {
    return get_records(h, &egg_handle::surfaces, kNoSurface, cap, sf, n);
}

// Collider motion ("Collider motion"): one record per collider, or none (all zero).  Everything is
// checked before anything changes; geometry and surfaces stay as they are.
int egg_set_collider_motion(egg_handle *h, int32_t n, const egg_collider_motion *mo) {
    static_assert(sizeof(egg_collider_motion) == 16 && sizeof(EggMotion) == sizeof(egg_collider_motion), "a motion record is 16 bytes");
    const int rc = check_records(h, "egg_set_collider_motion", n, mo);
    if (rc != EGG_OK) return rc;
    std::vector<egg_collider_motion> list((size_t)n);
    bool move = false;
    for (int32_t k = 0; k < n; ++k) {
        egg_collider_motion &o = list[(size_t)k];
        o = mo[k];
        if (!std::isfinite(o.vx) || !std::isfinite(o.vy))
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_set_collider_motion: collider %d: the velocity (%g, %g) is not finite", (int)k, o.vx,
                        o.vy);
        o.vx = o.vx + 0.0;  // (-0.0 is stored as +0.0: handles set alike compare alike)
        o.vy = o.vy + 0.0;
        move |= o.vx != 0.0 || o.vy != 0.0;
    }
    h->motions.swap(list);
    h->motions_move = move;
    h->collider_dirty |= kDirtyMotions;
    return EGG_OK;
}

int egg_get_collider_motion(const egg_handle *h, int32_t cap, egg_collider_motion *mo, int32_t *n) {
    return get_records(h, &egg_handle::motions, kNoMotion, cap, mo, n);
}

// Collider spin ("Collider spin"): one record per collider, or none (all zero).  Everything is
// checked before anything changes; geometry, surfaces and motions stay as they are.
int egg_set_collider_spin(egg_handle *h, int32_t n, const egg_collider_spin *sp) {
    static_assert(sizeof(egg_collider_spin) == 24 && sizeof(EggSpin) == sizeof(egg_collider_spin), "a spin record is 24 bytes");
    const int rc = check_records(h, "egg_set_collider_spin", n, sp);
    if (rc != EGG_OK) return rc;
    std::vector<egg_collider_spin> list((size_t)n);
    bool turn = false;
    for (int32_t k = 0; k < n; ++k) {
        egg_collider_spin &o = list[(size_t)k];
        o = sp[k];
        if (!std::isfinite(o.px) || !std::isfinite(o.py))
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_set_collider_spin: collider %d: the pivot (%g, %g) is not finite", (int)k, o.px, o.py);
        if (!std::isfinite(o.omega))
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_set_collider_spin: collider %d: omega %g is not finite", (int)k, o.omega);
        o.px = o.px + 0.0;  // (-0.0 is stored as +0.0: handles set alike compare alike)
        o.py = o.py + 0.0;
        o.omega = o.omega + 0.0;
        turn |= o.omega != 0.0;
    }
    h->spins.swap(list);
    h->spins_turn = turn;
    h->collider_dirty |= kDirtySpins;
    return EGG_OK;
}

int egg_get_collider_spin(const egg_handle *h, int32_t cap, egg_collider_spin *sp, int32_t *n) {
    return get_records(h, &egg_handle::spins, kNoSpin, cap, sp, n);
}

// Collider loads ("Collider loads"): the switch only observes, so it is accepted in either order and
// with an empty list; the stored loads start again at zero.
int egg_set_collider_loads(egg_handle *h, int on) {
    if (!h) return EGG_ERR_INVALID_ARGUMENT;
    REJECT_IN_FLIGHT(h, "egg_set_collider_loads");
    static_assert(EGG_COLLIDER_LOAD_IMPULSE_SCALE == EGG_RX_LOAD_SCALE_IMPULSE && EGG_COLLIDER_LOAD_TORQUE_SCALE == EGG_RX_LOAD_SCALE_TORQUE,
                  "the kernel's load scales are the ABI's");
    h->opt_loads = on != 0;
    h->load_sums.assign(3 * h->colliders.size(), 0);
    h->load_dropped = 0;
    h->load_sub_delta = 0.0;
    return EGG_OK;
}

int egg_get_collider_loads_enabled(const egg_handle *h, int *on) {
    if (!h || !on) return EGG_ERR_INVALID_ARGUMENT;
    *on = h->opt_loads ? 1 : 0;
    return EGG_OK;
}

int egg_get_collider_load_sums(egg_handle *h, int32_t cap, int64_t *sums, int64_t *dropped, double *sub_delta, int32_t *n) {
    if (!h) return EGG_ERR_INVALID_ARGUMENT;
    const int32_t have = (int32_t)h->colliders.size();
    if (n) *n = have;
    for (int32_t k = 0; sums && k < 3 * std::min(cap, have); ++k) sums[k] = (size_t)k < h->load_sums.size() ? h->load_sums[(size_t)k] : 0;
    if (dropped) *dropped = h->load_dropped;
    if (sub_delta) *sub_delta = h->load_sub_delta;
    return EGG_OK;
}

int egg_get_collider_loads(egg_handle *h, int32_t cap, egg_collider_load *out, int32_t *n) {
    if (!h) return EGG_ERR_INVALID_ARGUMENT;
    const int32_t have = (int32_t)h->colliders.size();
    if (n) *n = have;
    const double hs = h->load_sub_delta;
    for (int32_t k = 0; out && k < std::min(cap, have); ++k) {
        const bool any = hs > 0.0 && (size_t)(3 * k + 2) < h->load_sums.size();
        out[k].jx = any ? ((double)h->load_sums[(size_t)(3 * k)] / EGG_COLLIDER_LOAD_IMPULSE_SCALE) / hs : 0.0;
        out[k].jy = any ? ((double)h->load_sums[(size_t)(3 * k + 1)] / EGG_COLLIDER_LOAD_IMPULSE_SCALE) / hs : 0.0;
        out[k].torque = any ? ((double)h->load_sums[(size_t)(3 * k + 2)] / EGG_COLLIDER_LOAD_TORQUE_SCALE) / hs : 0.0;
    }
    return EGG_OK;
}

// Collider bodies ("Collider bodies"): one record per collider, or none (no collider is a body).
// Everything is checked before anything changes; geometry, surfaces, motions and spins stay as they are.  Nothing goes to the
// device here: a step in which bodies act uploads the records it runs on.
int egg_set_collider_bodies(egg_handle *h, int32_t n, const egg_collider_body *b) {
    static_assert(sizeof(egg_collider_body) == 48 && sizeof(EggBody) == sizeof(egg_collider_body), "a body record is 48 bytes");
    const int rc = check_records(h, "egg_set_collider_bodies", n, b);
    if (rc != EGG_OK) return rc;
    std::vector<egg_collider_body> list((size_t)n);
    bool any = false;
    for (int32_t k = 0; k < n; ++k) {
        egg_collider_body &o = list[(size_t)k];
        o = b[k];
        if (!std::isfinite(o.inv_mass) || o.inv_mass < 0)
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_set_collider_bodies: collider %d: inv_mass %g is negative or not finite", (int)k, o.inv_mass);
        if (!std::isfinite(o.inv_inertia) || o.inv_inertia < 0)
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_set_collider_bodies: collider %d: inv_inertia %g is negative or not finite", (int)k,
                        o.inv_inertia);
        if (!std::isfinite(o.ax) || !std::isfinite(o.ay))
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_set_collider_bodies: collider %d: the acceleration (%g, %g) is not finite", (int)k, o.ax, o.ay);
        if (!std::isfinite(o.drag) || o.drag < 0)
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_set_collider_bodies: collider %d: drag %g is negative or not finite", (int)k, o.drag);
        if (!std::isfinite(o.spin_drag) || o.spin_drag < 0)
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_set_collider_bodies: collider %d: spin_drag %g is negative or not finite", (int)k, o.spin_drag);
        o.inv_mass = o.inv_mass + 0.0;  // (-0.0 is stored as +0.0: handles set alike compare alike)
        o.inv_inertia = o.inv_inertia + 0.0;
        o.ax = o.ax + 0.0;
        o.ay = o.ay + 0.0;
        o.drag = o.drag + 0.0;
        o.spin_drag = o.spin_drag + 0.0;
        any |= o.inv_mass > 0.0 || o.inv_inertia > 0.0;
    }
    h->bodies.swap(list);
    h->bodies_any = any;
    return EGG_OK;
}

int egg_get_collider_bodies(const egg_handle *h, int32_t cap, egg_collider_body *b, int32_t *n) {
    return get_records(h, &egg_handle::bodies, kNoBody, cap, b, n);
}

// Collider contacts ("Collider contacts"): one record per collider, or none (no collider meets
// another).  Everything is checked before anything changes; the bodies and everything else about the list stay as they are.
// Nothing goes to the device here: a step in which contacts act uploads the records it runs on.
int egg_set_collider_contacts(egg_handle *h, int32_t n, const egg_collider_contact *c, int32_t iterations) {
    static_assert(sizeof(egg_collider_contact) == 16 && sizeof(EggContact) == sizeof(egg_collider_contact), "a contact record is 16 bytes");
    const int rc = check_records(h, "egg_set_collider_contacts", n, c);
    if (rc != EGG_OK) return rc;
    if (iterations < 0 || iterations > 16)
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_set_collider_contacts: %d iterations (1 .. 16, or 0 for the default of 4)", (int)iterations);
    std::vector<egg_collider_contact> list((size_t)n);
    bool any = false;
    for (int32_t k = 0; k < n; ++k) {
        egg_collider_contact &o = list[(size_t)k];
        o = c[k];
        if (!std::isfinite(o.restitution) || o.restitution < 0.0 || o.restitution > 1.0)
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_set_collider_contacts: collider %d: the restitution %g lies outside [0, 1]", (int)k, o.restitution);
        if (o.on != 0 && o.on != 1) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_set_collider_contacts: collider %d: on = %d is not 0 or 1", (int)k, (int)o.on);
        if (o.reserved != 0) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_set_collider_contacts: collider %d: reserved = %d is not 0", (int)k, (int)o.reserved);
        o.restitution = o.restitution + 0.0;  // (-0.0 is stored as +0.0)
        any |= o.on != 0;
    }
    if (any && h->opt_solver_order != EGG_SOLVER_RELAXED)
        return fail(h, EGG_ERR_UNSUPPORTED, "egg_set_collider_contacts: collider contacts need relaxed order (EGG_OPT_SOLVER_ORDER = 1 first)");
    h->contacts.swap(list);
    h->contacts_any = any;
    h->contact_iterations = iterations == 0 ? 4 : iterations;
    return EGG_OK;
}

int egg_get_collider_contacts(const egg_handle *h, int32_t cap, egg_collider_contact *out, int32_t *n, int32_t *iterations) {
    if (h && iterations) *iterations = h->contact_iterations;
    return get_records(h, &egg_handle::contacts, kNoContact, cap, out, n);
}

int egg_get_collider_contact_solves(egg_handle *h, int64_t *solves) {
    if (!h) return EGG_ERR_INVALID_ARGUMENT;
    if (!solves) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_get_collider_contact_solves: solves is NULL");
    *solves = h->contact_solves;
    return EGG_OK;
}

int egg_get_collider_grips(egg_handle *h, int64_t grips[2]) {
    if (!h) return EGG_ERR_INVALID_ARGUMENT;
    if (!grips) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_get_collider_grips: grips is NULL");
    grips[0] = h->collider_grips[0];
    grips[1] = h->collider_grips[1];
    return EGG_OK;
}

int egg_get_collider_hits(egg_handle *h, int64_t hits[2]) {
    if (!h) return EGG_ERR_INVALID_ARGUMENT;
    if (!hits) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_get_collider_hits: hits is NULL");
    hits[0] = h->collider_hits[0];
    hits[1] = h->collider_hits[1];
    return EGG_OK;
}

}  // extern "C"
