// eggsim_host_instances.hip -- host side of the instanced-draw record (csrc/eggsim_instances.hip; DESIGN.md section 2.6,
// "The instanced-draw record"): egg_get_instances, egg_instances_begin / egg_instances_end, and instances_from, which
// egg_group_get_instances (eggsim_host_render_group.hip) and egg_draw_source_instances (eggsim_host_draw_source.hip)
// call with their shadow arrays.
//
// The reference uploads a data mesh (28 B per particle) and a colour mesh (16 B per particle) every frame (L:513-523,
// L:744-877).  Here ONE kernel launch per type narrows the seven double arrays to the data mesh's records and, when asked,
// spreads the per-atom colour table the splat reads over the particles; what crosses the host link is the 28 (+ 16) B per
// particle the host's mesh holds, not seven double arrays.
//
// Synchronous form: kernel and copy on the type's stream, which is idle when the call returns.
// Two halves: egg_instances_begin launches the kernel on the type's stream and the copy into pinned memory on a copy
// stream of its own and returns; egg_instances_end waits for the copy.  Two pinned data buffers per type alternate, so
// the pointers of one end stay valid while the next begin fills the other.  The colour mesh is packed and copied only
// when the handle's color_version has moved since the last pack of the type; its two buffers alternate on packs, not on
// begins, so an unchanged colour pointer stays valid for as long as it is handed out.  Ordering on the device: the pack
// waits (event) for whatever the OTHER type's stream holds, because a fused step launch writes both types from one
// stream; both type streams then wait for the pack, so a step started between begin and end -- which overwrites the
// buffer that holds last_x / last_y -- runs behind it, while the copy, which reads a staging buffer, overlaps with it.
// The pack reads nothing the host rewrites outside the streams: the atoms' offsets and colours it needs are copies kept
// here (an add or a remove rewrites the System's d_atom_offset with a blocking copy that the type streams do not order).
#include "eggsim_host.h"

namespace egghost {

struct InstanceState {
    // synchronous form and instances_from: packed here when the destination is host memory (or not 16-byte aligned)
    DevBuf<float4> d_data, d_color, d_atom_color;
    // two halves
    struct Type {
        DevBuf<float4> d_data[2], d_color[2], d_atom_color;
        PinnedBuf<float4> h_data[2], h_color[2], h_atom_color;
        // the atoms' first particles as the colour pack reads them: a copy of its own, so that an add or a remove after
        // begin (which rewrites the System's d_atom_offset from the host, outside the streams) cannot reach a pack in flight
        DevBuf<int32_t> d_atom_offset;
        PinnedBuf<int32_t> h_atom_offset;
        int slot = 0, cslot = 0;       // buffers the NEXT pack writes
        uint64_t packed_version = 0;   // color_version of the last colour pack (0: none yet)
        int64_t packed_n = -1;         // ... and the particles it covered
        const float *color = nullptr;  // the colour mesh to hand out
        const egg_instance *data = nullptr;
        int64_t n = 0;
        hipEvent_t before = nullptr, packed = nullptr;
    } t[2];
    hipStream_t copy = nullptr;
    hipEvent_t done = nullptr;
    int open_mask = 0;  // types of the open begin that egg_instances_end has not handed out yet
    uint64_t open_version = 0;
    ~InstanceState() {
        for (Type &T : t)
            for (hipEvent_t e : {T.before, T.packed})
                if (e) (void)hipEventDestroy(e);
        if (done) (void)hipEventDestroy(done);
        if (copy) {
            (void)hipStreamSynchronize(copy);
            (void)hipStreamDestroy(copy);
        }
    }
};

namespace {

constexpr int64_t kMaxInstanceParticles = std::numeric_limits<int32_t>::max();

InstanceState &state_of(egg_handle *h) {
    if (!h->instances) h->instances = std::make_shared<InstanceState>();
    return *h->instances;
}

size_t data_units(size_t n) { return (n * sizeof(egg_instance) + 15) / 16; }  // float4 units that hold n records

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// one launch: n particles of src into d_data (null: none) and d_color (null: none); colours from d_atom_color
int launch_pack(egg_handle *h, hipStream_t st, const RenderSource::Type &T, float4 *d_data, float4 *d_color, const float4 *d_atom_color,
                size_t n_atoms) {
    EggInstanceArgs A;
    memset(&A, 0, sizeof A);
    const double *src[EGG_GATHER_FIELDS] = {T.x, T.y, T.last_x, T.last_y, T.vx, T.vy, T.radius};
    for (int f = 0; f < EGG_GATHER_FIELDS; ++f) A.src[f] = src[f];
    A.data = (float *)d_data;
    A.color = d_color;
    A.atom_offset = T.atom_offset;
    A.atom_color = d_atom_color;
    A.n = (int32_t)T.n;
    A.n_atoms = (int32_t)n_atoms;
    hipLaunchKernelGGL(egg_instances_kernel, dim3((unsigned)(((size_t)T.n + EGG_INSTANCE_BLOCK - 1) / EGG_INSTANCE_BLOCK)),
                       dim3(EGG_INSTANCE_BLOCK), 0, st, A);
    HIP_TRY(h, hipGetLastError());
    h->stats.kernel_launches++;
    return EGG_OK;
}

// the handle's own arrays of one type (the colours as render_source_of builds them); the atoms must be current
void own_source(egg_handle *h, int w, bool colors, RenderSource::Type &T) {
    System &s = h->sys[w];
    T.x = s.x[s.cur].p;
    T.y = s.y[s.cur].p;
    T.last_x = s.x[s.cur ^ 1].p;  // positions at the start of the most recent _step (L:1795-1815)
    T.last_y = s.y[s.cur ^ 1].p;
    T.vx = s.vx[s.cur].p;
    T.vy = s.vy[s.cur].p;
    T.radius = s.radius.p;
    T.atom_offset = s.d_atom_offset.p;
    T.n = s.n;
    if (!colors) return;
    const size_t na = s.atoms.size();
    T.atom_color.resize(4 * na);
    for (size_t k = 0; k < na; ++k) memcpy(&T.atom_color[4 * k], h->batches[(size_t)s.atoms[k].batch].pcolor[w], 16);
}

}  // namespace

int instances_from(egg_handle *h, hipStream_t st, const RenderSource::Type &T, const char *name, egg_instance *data, float *color,
                   int64_t cap, int64_t *n) {
    if (n) *n = T.n;
    if (cap < T.n) return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: buffer holds %lld of %lld particles", name, (long long)cap, (long long)T.n);
    if (T.n == 0 || (!data && !color)) return EGG_OK;
    if (T.n > kMaxInstanceParticles) return fail(h, EGG_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 particles of one type", name);
    const size_t np = (size_t)T.n, na = T.atom_color.size() / 4;
    if (color && na == 0) return fail(h, EGG_ERR_INTERNAL, "%s: particles without a colour table", name);
    InstanceState &I = state_of(h);
    const int rc = [&]() -> int {
        // a destination on this device is written by the kernel itself (the data mesh: when its 16 B stores are aligned)
        const bool direct_data = data && on_device_of(h, data) && aligned16(data);
        const bool direct_color = color && on_device_of(h, color) && aligned16(color);
        float4 *d_data = nullptr, *d_color = nullptr;
        if (data) {
            if (!direct_data) HIP_TRY(h, I.d_data.reserve(data_units(np), false, st));
            d_data = direct_data ? (float4 *)data : I.d_data.p;
        }
        if (color) {
            if (!direct_color) HIP_TRY(h, I.d_color.reserve(np, false, st));
            d_color = direct_color ? (float4 *)color : I.d_color.p;
            HIP_TRY(h, I.d_atom_color.reserve(na, false, st));
            HIP_TRY(h, hipMemcpyAsync(I.d_atom_color.p, T.atom_color.data(), na * 16, hipMemcpyHostToDevice, st));
        }
        const int prc = launch_pack(h, st, T, d_data, d_color, I.d_atom_color.p, na);
        if (prc != EGG_OK) return prc;
        if (data && !direct_data) HIP_TRY(h, hipMemcpyAsync(data, d_data, np * sizeof(egg_instance), hipMemcpyDefault, st));
        if (color && !direct_color) HIP_TRY(h, hipMemcpyAsync(color, d_color, np * 16, hipMemcpyDefault, st));
        HIP_TRY(h, hipStreamSynchronize(st));  // (the colour table is pageable; the meshes are complete when the call returns)
        return EGG_OK;
    }();
    // a failure half-way leaves nothing in flight that reads the caller's colour table or writes the caller's memory
    if (rc != EGG_OK) (void)hipStreamSynchronize(st);
    return rc;
}

}  // namespace egghost

extern "C" {

int egg_get_instances(egg_handle *h, int which, egg_instance *data, float *color, int64_t cap, int64_t *n, uint64_t *color_version) {
    if (!h || (which != EGG_WHITE && which != EGG_YOLK) || cap < 0) return EGG_ERR_INVALID_ARGUMENT;
    REJECT_IN_FLIGHT(h, "egg_get_instances");
    if (h->instances && h->instances->open_mask)
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_get_instances: egg_instances_begin without its egg_instances_end");
    HIP_TRY(h, hipSetDevice(h->device));
    if (color_version) *color_version = h->color_version;
    System &s = h->sys[which];
    RenderSource::Type T;
    if (color && s.n > 0) {
        const int rc = upload_atoms(h, which);
        if (rc != EGG_OK) return rc;
    }
    own_source(h, which, color != nullptr && s.n > 0, T);
    HIP_TRY(h, hipStreamSynchronize(h->sys[which ^ 1].stream));  // (a fused launch or a hand-over may have used the other stream)
    return instances_from(h, s.stream, T, "egg_get_instances", data, color, cap, n);
}

int egg_instances_begin(egg_handle *h, int32_t type_mask) {
    if (!h || type_mask < 1 || type_mask > 3) return EGG_ERR_INVALID_ARGUMENT;
    REJECT_IN_FLIGHT(h, "egg_instances_begin");
    InstanceState &I = state_of(h);
    if (I.open_mask) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_instances_begin: the last begin has not been ended (egg_instances_end, once per type)");
    for (int w = 0; w < 2; ++w)
        if (((type_mask >> w) & 1) && h->sys[w].n > kMaxInstanceParticles)
            return fail(h, EGG_ERR_UNSUPPORTED, "egg_instances_begin: more than 2^31 - 1 particles of one type");
    HIP_TRY(h, hipSetDevice(h->device));
    if (!I.copy) HIP_TRY(h, hipStreamCreateWithFlags(&I.copy, hipStreamNonBlocking));
    if (!I.done) HIP_TRY(h, hipEventCreateWithFlags(&I.done, hipEventDisableTiming));
    for (int w = 0; w < 2; ++w) {
        if (!((type_mask >> w) & 1)) continue;
        InstanceState::Type &B = I.t[w];
        System &s = h->sys[w];
        hipStream_t st = s.stream, other = h->sys[w ^ 1].stream;
        const size_t np = (size_t)s.n;
        B.n = s.n;
        B.data = nullptr;
        const bool recolor = B.packed_version != h->color_version || B.packed_n != s.n;
        if (np == 0) {
            if (recolor) B.color = nullptr;
            B.packed_version = h->color_version;
            B.packed_n = 0;
            continue;
        }
        if (recolor) {
            const int rc = upload_atoms(h, w);
            if (rc != EGG_OK) return rc;
        }
        RenderSource::Type T;
        own_source(h, w, recolor, T);
        const size_t na = T.atom_color.size() / 4;
        const int slot = B.slot, cslot = B.cslot;
        HIP_TRY(h, B.d_data[slot].reserve(data_units(np), false, st));
        HIP_TRY(h, B.h_data[slot].reserve(data_units(np)));
        if (recolor) {
            HIP_TRY(h, B.d_color[cslot].reserve(np, false, st));
            HIP_TRY(h, B.h_color[cslot].reserve(np));
            HIP_TRY(h, B.d_atom_color.reserve(na, false, st));
            HIP_TRY(h, B.h_atom_color.reserve(na));
            HIP_TRY(h, B.d_atom_offset.reserve(na, false, st));
            HIP_TRY(h, B.h_atom_offset.reserve(na));
            memcpy(B.h_atom_color.p, T.atom_color.data(), na * 16);  // (pinned: the copies below do not wait for the host)
            for (size_t k = 0; k < na; ++k) B.h_atom_offset.p[k] = s.atoms[k].offset;
            T.atom_offset = B.d_atom_offset.p;
        }
        for (hipEvent_t *e : {&B.before, &B.packed})
            if (!*e) HIP_TRY(h, hipEventCreateWithFlags(e, hipEventDisableTiming));
        HIP_TRY(h, hipEventRecord(B.before, other));
        HIP_TRY(h, hipStreamWaitEvent(st, B.before, 0));
        if (recolor) {
            HIP_TRY(h, hipMemcpyAsync(B.d_atom_color.p, B.h_atom_color.p, na * 16, hipMemcpyHostToDevice, st));
            HIP_TRY(h, hipMemcpyAsync(B.d_atom_offset.p, B.h_atom_offset.p, na * 4, hipMemcpyHostToDevice, st));
        }
        const int rc = launch_pack(h, st, T, B.d_data[slot].p, recolor ? B.d_color[cslot].p : nullptr, B.d_atom_color.p, na);
        if (rc != EGG_OK) return rc;
        HIP_TRY(h, hipEventRecord(B.packed, st));
        HIP_TRY(h, hipStreamWaitEvent(other, B.packed, 0));
        HIP_TRY(h, hipStreamWaitEvent(I.copy, B.packed, 0));
        HIP_TRY(h, hipMemcpyAsync(B.h_data[slot].p, B.d_data[slot].p, np * sizeof(egg_instance), hipMemcpyDeviceToHost, I.copy));
        B.data = (const egg_instance *)B.h_data[slot].p;
        B.slot ^= 1;
        if (recolor) {
            HIP_TRY(h, hipMemcpyAsync(B.h_color[cslot].p, B.d_color[cslot].p, np * 16, hipMemcpyDeviceToHost, I.copy));
            B.color = (const float *)B.h_color[cslot].p;
            B.cslot ^= 1;
            B.packed_version = h->color_version;
            B.packed_n = s.n;
        }
    }
    HIP_TRY(h, hipEventRecord(I.done, I.copy));
    I.open_mask = type_mask;
    I.open_version = h->color_version;
    return EGG_OK;
}

int egg_instances_end(egg_handle *h, int which, const egg_instance **data, const float **color, int64_t *n, uint64_t *color_version) {
    if (!h || (which != EGG_WHITE && which != EGG_YOLK)) return EGG_ERR_INVALID_ARGUMENT;
    InstanceState &I = state_of(h);
    if (!((I.open_mask >> which) & 1))
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_instances_end: no egg_instances_begin is open for type %d", which);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipEventSynchronize(I.done));
    const InstanceState::Type &B = I.t[which];
    if (data) *data = B.data;
    if (color) *color = B.color;
    if (n) *n = B.n;
    if (color_version) *color_version = I.open_version;
    I.open_mask &= ~(1 << which);
    return EGG_OK;
}

}  // extern "C"
