// eggsim_host_touches.hip -- touches (include/eggsim_touch.h): the checks of a call, the list of its
// queries, the rounds of two launches of eggsim_touches.hip over the unit table of the shared host layer
// (eggsim_host_scan.hip), the one re-run when the record buffer was short, and the merge of the partial records.
// egg_touches takes its queries from the handle's own atoms, egg_touches_of from discs the caller hands in, which are
// uploaded once; both end in the same rounds.  A call stores no answer; a step launches nothing of this and takes no argument
// from it.
#include <map>

#include "eggsim_host.h"

namespace egghost {

struct TouchState {
    UnitTable units, units_by_key;        // every unit of every type the last call covered, labelled with its batch's id / key
    TouchState() { units_by_key.by_key = true; }
    DevBuf<EggTouchSource> d_sources;     // every query of the call
    DevBuf<EggTouchQuery> d_queries;      // [EGG_TC_ROUND]: the round's table
    DevBuf<EggTouchDisc> d_discs;         // the round's discs
    DevBuf<double> d_in;                  // egg_touches_of: the caller's x, y, r
    DevBuf<EggTouchRecord> d_out;         // the partial records
    size_t records = EGG_TC_FIRST_RECORDS;  // how many of them a run may write: the most any run has asked for
    DevBuf<int32_t> d_cursor;
    DevBuf<unsigned long long> d_candidates;  // EGGSIM_TOUCH_CANDIDATES only
};

namespace {

// the grid is sized to the device, not to the scene: kWavesPerCu one-wave workgroups per compute unit at the most.
// (EGGSIM_TOUCH_WAVES_PER_CU: developer override, 1 .. 32)
constexpr int kWavesPerCu = 8;

// what both entry points check alike, before anything is launched or written
int check_call(egg_handle *h, const char *name, const egg_touch_spec *spec, int64_t cap, const egg_touch_record *out, const int64_t *n_out) {
    static_assert(sizeof(egg_touch_spec) == 24, "a touch spec is 24 bytes");
    static_assert(sizeof(egg_touch_query) == 16, "a touch query is 16 bytes");
    static_assert(sizeof(egg_touch_record) == 40 && sizeof(EggTouchRecord) == sizeof(egg_touch_record), "a touch record is 40 bytes");
    static_assert(offsetof(egg_touch_record, other) == 16 && offsetof(EggTouchRecord, other) == 16, "the 64-bit words follow four int32");
    static_assert(sizeof(EggTouchQuery) == 72 && sizeof(EggTouchDisc) == 48, "the round's tables");
    static_assert(EGG_TC_ROUND == EGG_WAVE && EGG_TC_OWN * EGG_WAVE == EGG_SN_UNIT && EGG_TC_OWN <= 32, "a lane per query, a bit per place");
    REJECT_IN_FLIGHT(h, name);
    if (!spec) return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: spec is NULL", name);
    if (!n_out) return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: n_out is NULL", name);
    for (int w = 0; w < 2; ++w)
        if (!std::isfinite(spec->reach[w]) || !(spec->reach[w] > 0.0))
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: reach[%d] = %g: it is finite and above 0", name, w, spec->reach[w]);
    if (spec->type_mask < 1 || spec->type_mask > 3)
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: type_mask %d (bit 0 white, bit 1 yolk, never 0)", name, (int)spec->type_mask);
    if ((spec->flags & ~(int32_t)EGG_TOUCH_BY_KEYS) != 0) return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: unknown flags 0x%x", name, (unsigned)spec->flags);
    if (cap < 0 || (cap > 0 && !out))
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: cap = %lld %s a buffer", name, (long long)cap, out ? "with" : "without");
    return EGG_OK;
}

// The rounds.  `sources` lists the queries with at least one disc, of covered types, `first` not yet set; src the arrays per
// type their offsets index.  The partial records of one (slot, other) are added and the answer sorted.
int run_rounds(egg_handle *h, const char *name, const egg_touch_spec *spec, std::vector<EggTouchSource> &sources, const double *const src[3][2],
               int64_t cap, egg_touch_record *out, int64_t *n_out) {
    const bool by_key = (spec->flags & EGG_TOUCH_BY_KEYS) != 0;
    const int types = covered_types(h, spec->type_mask);
    std::vector<egg_touch_record> answer;
    if (types != 0 && !sources.empty()) {
        TouchState &S = *h->touch_state;
        UnitTable &T = by_key ? S.units_by_key : S.units;
        int rc = T.refresh(h, name, types, true);
        if (rc != EGG_OK) return rc;
        if (T.n_units > 0) {
            System &W = h->sys[0], &Y = h->sys[1];
            // a query's discs lie at `first` in its round's table
            const size_t n_rounds = (sources.size() + EGG_TC_ROUND - 1) / EGG_TC_ROUND;
            size_t most = 0;
            for (size_t r = 0; r < n_rounds; ++r) {
                long long at = 0;
                for (size_t q = r * EGG_TC_ROUND; q < std::min(sources.size(), (r + 1) * EGG_TC_ROUND); ++q) {
                    sources[q].first = at;
                    at += sources[q].count;
                }
                most = std::max(most, (size_t)at);
            }
            HIP_TRY(h, S.d_sources.reserve(sources.size(), false, nullptr));
            HIP_TRY(h, S.d_queries.reserve(EGG_TC_ROUND, false, nullptr));
            HIP_TRY(h, S.d_discs.reserve(most, false, nullptr));
            HIP_TRY(h, S.d_cursor.reserve(1, false, nullptr));
            HIP_TRY(h, hipMemcpy(S.d_sources.p, sources.data(), sources.size() * sizeof(EggTouchSource), hipMemcpyHostToDevice));
            const bool count_candidates = getenv("EGGSIM_TOUCH_CANDIDATES") != nullptr;
            if (count_candidates) HIP_TRY(h, S.d_candidates.reserve(1, false, nullptr));
            EggTouchGatherArgs G{};
            EggTouchArgs A{};
            for (int w = 0; w < 2; ++w) {
                System &s = h->sys[w];
                G.x[w] = src[0][w];
                G.y[w] = src[1][w];
                G.r[w] = src[2][w];
                A.x[w] = s.x[s.cur].p;
                A.y[w] = s.y[s.cur].p;
                A.radius[w] = s.radius.p;
                A.reach[w] = spec->reach[w];
            }
            G.queries = S.d_queries.p;
            G.discs = S.d_discs.p;
            A.units = T.d_units.p;
            A.n_units = T.n_units;
            A.cursor = S.d_cursor.p;
            A.candidates = count_candidates ? S.d_candidates.p : nullptr;
            const int waves = grid_cap(h, T.n_units, kWavesPerCu, "EGGSIM_TOUCH_WAVES_PER_CU");
            HIP_TRY(h, hipStreamSynchronize(Y.stream));  // (no step is running: every step ends with its streams waited for)
            int32_t asked = 0;
            // at most two runs: the cursor keeps counting past the end of the buffer, and a run that overflowed is run once
            // more with the buffer it asked for -- the call only reads, so the second run asks for the same
            for (int run = 0; run < 2; ++run) {
                HIP_TRY(h, S.d_out.reserve(S.records, false, nullptr));
                A.out = S.d_out.p;
                A.cap = (int32_t)std::min<size_t>(S.records, (size_t)std::numeric_limits<int32_t>::max());
                HIP_TRY(h, hipMemsetAsync(S.d_cursor.p, 0, sizeof(int32_t), W.stream));
                if (count_candidates) HIP_TRY(h, hipMemsetAsync(S.d_candidates.p, 0, sizeof(unsigned long long), W.stream));
                for (size_t r = 0; r < n_rounds; ++r) {
                    const int32_t n = (int32_t)(std::min(sources.size(), (r + 1) * EGG_TC_ROUND) - r * EGG_TC_ROUND);
                    G.sources = S.d_sources.p + r * EGG_TC_ROUND;
                    G.n_queries = A.n_queries = n;
                    hipLaunchKernelGGL(egg_touch_gather_kernel, dim3((unsigned)n), dim3(EGG_WAVE), 0, W.stream, G);
                    HIP_TRY(h, hipGetLastError());
                    hipLaunchKernelGGL(egg_touch_kernel, dim3((unsigned)waves), dim3(EGG_WAVE), 0, W.stream, A, (const EggTouchQuery *)S.d_queries.p,
                                       (const EggTouchDisc *)S.d_discs.p);
                    HIP_TRY(h, hipGetLastError());
                    h->stats.kernel_launches += 2;
                }
                HIP_TRY(h, hipMemcpyAsync(&asked, S.d_cursor.p, sizeof asked, hipMemcpyDeviceToHost, W.stream));
                HIP_TRY(h, hipStreamSynchronize(W.stream));
                if (asked < 0) return fail(h, EGG_ERR_UNSUPPORTED, "%s: more than 2^31 partial records", name);
                if ((size_t)asked <= S.records) break;
                if (run == 1) return fail(h, EGG_ERR_INTERNAL, "%s: the second run asked for %d records, the first for %zu", name, (int)asked, S.records);
                S.records = (size_t)asked;
            }
            if (count_candidates) {
                unsigned long long through = 0;
                HIP_TRY(h, hipMemcpy(&through, S.d_candidates.p, sizeof through, hipMemcpyDeviceToHost));
                fprintf(stderr, "egg_touches candidates: units %d queries %zu rounds %zu let through %llu partial records %d\n", (int)T.n_units,
                        sources.size(), n_rounds, through, (int)asked);
            }
            std::vector<egg_touch_record> part((size_t)asked);
            if (asked > 0) HIP_TRY(h, hipMemcpy(part.data(), S.d_out.p, part.size() * sizeof(egg_touch_record), hipMemcpyDeviceToHost));
            // several partial records of one (slot, other) arise when the other atom has several units
            std::map<std::pair<int32_t, int64_t>, egg_touch_record> sum;
            for (const egg_touch_record &p : part) {
                auto at = sum.find({p.slot, p.other});
                if (at == sum.end()) {
                    sum.emplace(std::make_pair(p.slot, p.other), p);
                    continue;
                }
                egg_touch_record &o = at->second;
                if ((int64_t)o.pairs + p.pairs > (int64_t)std::numeric_limits<int32_t>::max())
                    return fail(h, EGG_ERR_UNSUPPORTED, "%s: the pairs of slot %d with batch %lld do not fit 31 bits", name, (int)p.slot, (long long)p.other);
                o.pairs += p.pairs;
                o.particles += p.particles;
                o.dropped += p.dropped;
                o.sx = (int64_t)((uint64_t)o.sx + (uint64_t)p.sx);
                o.sy = (int64_t)((uint64_t)o.sy + (uint64_t)p.sy);
            }
            answer.reserve(sum.size());
            for (const auto &kv : sum) answer.push_back(kv.second);  // (the map's order: slot, then other)
        }
    }
    *n_out = (int64_t)answer.size();
    if ((int64_t)answer.size() > cap)
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "%s: the answer holds %lld records, the buffer %lld", name, (long long)answer.size(), (long long)cap);
    if (!answer.empty()) memcpy(out, answer.data(), answer.size() * sizeof(egg_touch_record));
    return EGG_OK;
}

}  // namespace
}  // namespace egghost

extern "C" {

// Everything is checked before anything is launched or written.  Not cached: every call scans the arrays
// egg_download_particles would return now.
int egg_touches(egg_handle *h, const egg_touch_spec *spec, int64_t n_ids, const int64_t *ids, int64_t cap, egg_touch_record *out,
                int64_t *n_out) {
    if (!h) return EGG_ERR_INVALID_ARGUMENT;
    int rc = check_call(h, "egg_touches", spec, cap, out, n_out);
    if (rc != EGG_OK) return rc;
    if (n_ids < 0 || (n_ids > 0 && !ids) || (n_ids == 0 && ids))
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_touches: n_ids = %lld %s a list (0 and NULL mean every live batch)", (long long)n_ids,
                    ids ? "with" : "without");
    rc = check_batch_ids(h, "egg_touches", n_ids, ids);
    if (rc != EGG_OK) return rc;
    std::vector<int64_t> every;
    if (n_ids == 0) {
        every = live_batch_ids(h);
        ids = every.data();
        n_ids = (int64_t)every.size();
    }
    if (n_ids > (int64_t)(std::numeric_limits<int32_t>::max() / 4))
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_touches: %lld ids in one call", (long long)n_ids);
    for (int64_t i = 0; i < n_ids; ++i) {
        const Batch *b = find_batch(h, ids[i]);
        for (int w = 0; w < 2; ++w)
            if ((spec->type_mask >> w & 1) && b->n[w] > EGG_TOUCH_MAX_QUERY)
                return fail(h, EGG_ERR_UNSUPPORTED, "egg_touches: batch `%lld` has %lld %s particles, a query holds at most %d", (long long)ids[i],
                            (long long)b->n[w], w ? "yolk" : "white", EGG_TOUCH_MAX_QUERY);
    }
    (void)hipSetDevice(h->device);
    rc = upload_atoms(h);
    if (rc != EGG_OK) return rc;
    if (!h->touch_state) h->touch_state = std::make_shared<TouchState>();
    const bool by_key = (spec->flags & EGG_TOUCH_BY_KEYS) != 0;
    std::vector<EggTouchSource> sources;
    rc = for_each_requested_atom(h, "egg_touches", covered_types(h, spec->type_mask), n_ids, ids, [&](const Atom &at, int w, int32_t slot) {
        const Batch &b = h->batches[(size_t)at.batch];
        sources.push_back(EggTouchSource{at.offset, at.count, w, slot, (long long)(by_key ? b.key : b.id), 0});
        return (int)EGG_OK;
    });
    if (rc != EGG_OK) return rc;
    const double *src[3][2];
    for (int w = 0; w < 2; ++w) {
        System &s = h->sys[w];
        src[0][w] = s.x[s.cur].p;
        src[1][w] = s.y[s.cur].p;
        src[2][w] = s.radius.p;
    }
    return run_rounds(h, "egg_touches", spec, sources, src, cap, out, n_out);
}

int egg_touches_of(egg_handle *h, const egg_touch_spec *spec, int64_t n_queries, const egg_touch_query *queries, const double *x,
                   const double *y, const double *r, int64_t cap, egg_touch_record *out, int64_t *n_out) {
    if (!h) return EGG_ERR_INVALID_ARGUMENT;
    int rc = check_call(h, "egg_touches_of", spec, cap, out, n_out);
    if (rc != EGG_OK) return rc;
    if (n_queries < 0 || (n_queries > 0 && !queries))
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_touches_of: n_queries = %lld %s a list", (long long)n_queries, queries ? "with" : "without");
    if (n_queries > (int64_t)(std::numeric_limits<int32_t>::max() / 4))
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_touches_of: %lld queries in one call", (long long)n_queries);
    int64_t total = 0;
    for (int64_t i = 0; i < n_queries; ++i) {
        const egg_touch_query &q = queries[i];
        if (q.type < 0 || q.type > 1) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_touches_of: query %lld: type %d (0 white, 1 yolk)", (long long)i, (int)q.type);
        if (q.count < 0) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_touches_of: query %lld: count %d is negative", (long long)i, (int)q.count);
        if (q.count > EGG_TOUCH_MAX_QUERY)
            return fail(h, EGG_ERR_UNSUPPORTED, "egg_touches_of: query %lld holds %d discs, a query holds at most %d", (long long)i, (int)q.count,
                        EGG_TOUCH_MAX_QUERY);
        total += q.count;
    }
    if (total > (int64_t)std::numeric_limits<int32_t>::max())
        return fail(h, EGG_ERR_UNSUPPORTED, "egg_touches_of: %lld discs in one call", (long long)total);
    if (total > 0 && (!x || !y || !r)) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_touches_of: %lld discs without x, y or r", (long long)total);
    for (int64_t i = 0; i < total; ++i)
        if (!std::isfinite(r[i])) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_touches_of: the radius of disc %lld is not finite", (long long)i);
    (void)hipSetDevice(h->device);
    rc = upload_atoms(h);
    if (rc != EGG_OK) return rc;
    if (!h->touch_state) h->touch_state = std::make_shared<TouchState>();
    TouchState &S = *h->touch_state;
    const int types = covered_types(h, spec->type_mask);
    std::vector<EggTouchSource> sources;
    int64_t at = 0;
    for (int64_t i = 0; i < n_queries; ++i) {
        const egg_touch_query &q = queries[i];
        if (q.count > 0 && (types >> q.type & 1)) sources.push_back(EggTouchSource{(int32_t)at, q.count, q.type, (int32_t)(2 * i + q.type), (long long)q.key, 0});
        at += q.count;
    }
    const double *src[3][2] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};
    if (!sources.empty()) {  // the caller's discs, uploaded once: x, y, r behind each other
        HIP_TRY(h, S.d_in.reserve(3 * (size_t)total, false, nullptr));
        const double *const from[3] = {x, y, r};
        for (int f = 0; f < 3; ++f) {
            HIP_TRY(h, hipMemcpy(S.d_in.p + (size_t)f * (size_t)total, from[f], (size_t)total * sizeof(double), hipMemcpyHostToDevice));
            src[f][0] = src[f][1] = S.d_in.p + (size_t)f * (size_t)total;
        }
    }
    return run_rounds(h, "egg_touches_of", spec, sources, src, cap, out, n_out);
}

}  // extern "C"
