// eggsim_host_scan.hip -- the host layer under the calls that scan the committed particles between steps (DESIGN.md
// sections 2.8 to 2.13): the refusal while a step is in flight, the atoms of both types, the unit builder and the unit
// table, the grid cap, the test of a caller's device memory, and the id lists with the walk over their atoms.  It names
// none of its callers, launches nothing and keeps no state of its own: a table belongs to the feature that embeds it.
#include "eggsim_host.h"

namespace egghost {

// the ONE definition of the two messages (REJECT_IN_FLIGHT, eggsim_host.h)
int refuse_in_flight(egg_handle *h, const char *name) {
    if (h->in_flight) return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: a step is in flight (egg_step_begin without egg_step_end)", name);
    if (h->wire_active) return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: a step is in flight (egg_rx_begin without egg_rx_end)", name);
    return EGG_OK;
}

int upload_atoms(egg_handle *h) {
    for (int w = 0; w < 2; ++w) {
        const int rc = upload_atoms(h, w);
        if (rc != EGG_OK) return rc;
    }
    return EGG_OK;
}

void push_units(const Atom &a, int w, std::vector<EggScanUnit> &units) {
    for (int32_t at = 0; at < a.count; at += EGG_SN_UNIT)
        units.push_back(EggScanUnit{a.offset + at, std::min<int32_t>(EGG_SN_UNIT, a.count - at), w, 0});
}

int covered_types(const egg_handle *h, int mask) {
    for (int w = 0; w < 2; ++w)
        if (h->sys[w].n == 0) mask &= ~(1 << w);
    return mask;
}

int UnitTable::refresh(egg_handle *h, const char *name, int want, bool with_batch_ids) {
    if (cover == want && gen[0] == h->sys[0].atoms_gen && gen[1] == h->sys[1].atoms_gen) return EGG_OK;
    gen[0] = gen[1] = ~0ull;  // (until the table below is complete)
    std::vector<EggScanUnit> units;
    for (int w = 0; w < 2; ++w) {
        if (!(want >> w & 1)) continue;
        for (const Atom &a : h->sys[w].atoms) {
            if (a.count < 1) continue;
            if (a.offset < 0 || (int64_t)a.offset + a.count > h->sys[w].n)
                return fail(h, EGG_ERR_INTERNAL, "%s: an atom of type %d holds %d particles from %d", name, w, (int)a.count, (int)a.offset);
            const size_t first = units.size();
            push_units(a, w, units);
            if (!with_batch_ids) continue;
            // (a unit's spare word carries the id of its batch: ids are 1 + the index into h->batches; or its key, from 0)
            const int64_t id = by_key ? h->batches[(size_t)a.batch].key : h->batches[(size_t)a.batch].id;
            if (id < (by_key ? 0 : 1) || id > (int64_t)std::numeric_limits<int32_t>::max())
                return fail(h, EGG_ERR_INTERNAL, "%s: batch %s %lld does not fit a unit's 32-bit word", name, by_key ? "key" : "id", (long long)id);
            for (size_t q = first; q < units.size(); ++q) units[q].reserved = (int32_t)id;
        }
    }
    HIP_TRY(h, d_units.reserve(units.size(), false, nullptr));
    if (!units.empty()) HIP_TRY(h, hipMemcpy(d_units.p, units.data(), units.size() * sizeof(EggScanUnit), hipMemcpyHostToDevice));
    n_units = (int32_t)units.size();
    cover = want;
    gen[0] = h->sys[0].atoms_gen;
    gen[1] = h->sys[1].atoms_gen;
    return EGG_OK;
}

int grid_cap(const egg_handle *h, int64_t n, int per_cu_default, const char *env_name) {
    const char *e = env_name ? getenv(env_name) : nullptr;
    const int per_cu = e ? std::min(32, std::max(1, atoi(e))) : per_cu_default;
    const int64_t most = per_cu * (int64_t)std::max(1, h->prop.multiProcessorCount);
    return (int)std::min<int64_t>(n, most);
}

bool device_range_fits(const egg_handle *h, const void *p, size_t bytes) {
    if (!on_device_of(h, p)) return false;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    const uintptr_t at = (uintptr_t)p, lo = (uintptr_t)base;
    return at >= lo && bytes <= size && at - lo <= size - bytes;
}

int check_batch_ids(egg_handle *h, const char *name, int64_t n_ids, const int64_t *ids) {
    for (int64_t i = 0; i < n_ids; ++i)
        if (!find_batch(h, ids[i])) return fail(h, EGG_ERR_UNKNOWN_ID, "%s: no batch with id `%lld`", name, (long long)ids[i]);
    return EGG_OK;
}

std::vector<int64_t> live_batch_ids(const egg_handle *h) {
    std::vector<int64_t> ids;
    for (int32_t bi : h->order) ids.push_back(h->batches[(size_t)bi].id);
    return ids;
}

std::vector<int32_t> atom_of_batch(const egg_handle *h) {
    std::vector<int32_t> atom_of_batch(h->batches.size(), -1);
    for (size_t a = 0; a < h->sys[0].atoms.size(); ++a) atom_of_batch[(size_t)h->sys[0].atoms[a].batch] = (int32_t)a;
    return atom_of_batch;
}

}  // namespace egghost
