// eggsim_host_pieces.hip -- pieces (include/eggsim.h, "pieces"): the checks of a call, the task table
// and the launches of eggsim_pieces.hip, one per class of atoms present, over the shared host layer of eggsim_host_scan.hip
// (the id list, the walk over its atoms, the grid cap).  A call copies one task table up (none when it
// asks for every live batch and neither the atoms nor the mask moved since the last such call) and the records back once.
// It stores no answer; a step launches nothing of this and takes no argument from it.
#include "eggsim_host.h"

namespace egghost {

struct PiecesState {
    DevBuf<EggPiecesTask> d_tasks;   // the wave class first, the block class behind it
    DevBuf<EggPieceSummary> d_out;   // one record per task
    DevBuf<int32_t> d_labels[2];     // per type [n], when labels are asked for
    DevBuf<int32_t> d_sweeps;        // EGGSIM_PIECES_SWEEPS only
    // the table of "every live batch", kept while the atoms and the mask stand
    uint64_t all_gen[2] = {~0ull, ~0ull};
    int all_mask = -1;
    bool table_is_all = false;
    int32_t n_class[2] = {0, 0}, max_class[2] = {0, 0};  // tasks and the largest atom per class
    size_t lds_granted[2] = {64 * 1024, 64 * 1024};      // dynamic LDS the runtime grants each kernel
};

namespace {

// the grid is sized to the device, not to the scene: kGroupsPerCu workgroups per compute unit at the most, the tasks
// beyond that are taken in a grid stride.  (EGGSIM_PIECES_GROUPS_PER_CU: developer override, 1 .. 32;
// profiles/r30_pieces.md has the sweep behind the default)
constexpr int kGroupsPerCu = 16;

size_t pieces_lds(int32_t largest) { return (size_t)EGG_PC_LDS_PER_PARTICLE * (size_t)largest + EGG_PC_TAIL; }

}  // namespace
}  // namespace egghost

extern "C" {

// Everything is checked before anything is launched or written.  Not cached: every call measures the arrays
// egg_download_particles would return now.
int egg_pieces(egg_handle *h, const egg_pieces_spec *spec, int64_t n_ids, const int64_t *ids, egg_piece_summary *out,
               int32_t *white_labels, int32_t *yolk_labels) {
    if (!h) return EGG_ERR_INVALID_ARGUMENT;
    static_assert(sizeof(egg_pieces_spec) == 24, "a pieces spec is 24 bytes");
    static_assert(sizeof(egg_piece_summary) == 40 && sizeof(EggPieceSummary) == sizeof(egg_piece_summary), "a piece summary is 40 bytes");
    static_assert(offsetof(egg_piece_summary, sx) == 24 && offsetof(EggPieceSummary, sx) == 24, "the sums follow six int32");
    static_assert(EGG_PIECES_MAX_ATOM == EGG_PC_MAX_ATOM, "the kernel's cap is the ABI's");
    static_assert((size_t)EGG_PC_LDS_PER_PARTICLE * EGG_PC_MAX_ATOM + EGG_PC_TAIL <= kLdsMax, "the largest atom fits a compute unit's LDS");
    static_assert(EGG_PC_WAVE_ATOM <= EGG_PC_MAX_ATOM, "the classes");
    REJECT_IN_FLIGHT(h, "egg_pieces");
    if (!spec) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_pieces: spec is NULL");
    if (!out) return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_pieces: out is NULL");
    if (n_ids < 0 || (n_ids > 0 && !ids) || (n_ids == 0 && ids))
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_pieces: n_ids = %lld %s a list (0 and NULL mean every live batch)", (long long)n_ids,
                    ids ? "with" : "without");
    int rc = check_batch_ids(h, "egg_pieces", n_ids, ids);
    if (rc != EGG_OK) return rc;
    for (int w = 0; w < 2; ++w)
        if (!std::isfinite(spec->reach[w]) || !(spec->reach[w] > 0.0))
            return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_pieces: reach[%d] = %g: it is finite and above 0", w, spec->reach[w]);
    if (spec->type_mask < 1 || spec->type_mask > 3)
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_pieces: type_mask %d (bit 0 white, bit 1 yolk, never 0)", (int)spec->type_mask);
    const bool all = n_ids == 0;
    std::vector<int64_t> every;
    if (all) {
        every = live_batch_ids(h);
        ids = every.data();
        n_ids = (int64_t)every.size();
    }
    if (n_ids > (int64_t)(std::numeric_limits<int32_t>::max() / 4))
        return fail(h, EGG_ERR_INVALID_ARGUMENT, "egg_pieces: %lld ids in one call", (long long)n_ids);
    for (int64_t i = 0; i < n_ids; ++i) {
        const Batch *b = find_batch(h, ids[i]);
        for (int w = 0; w < 2; ++w)
            if ((spec->type_mask >> w & 1) && b->n[w] > EGG_PIECES_MAX_ATOM)
                return fail(h, EGG_ERR_UNSUPPORTED, "egg_pieces: batch `%lld` has %lld %s particles, an atom holds at most %d", (long long)ids[i],
                            (long long)b->n[w], w ? "yolk" : "white", EGG_PIECES_MAX_ATOM);
    }
    int32_t *const host_labels[2] = {white_labels, yolk_labels};
    System &W = h->sys[0], &Y = h->sys[1];
    std::vector<egg_piece_summary> records(2 * (size_t)n_ids, egg_piece_summary{});
    (void)hipSetDevice(h->device);
    rc = upload_atoms(h);
    if (rc != EGG_OK) return rc;
    if (!h->pieces_state) h->pieces_state = std::make_shared<PiecesState>();
    PiecesState &S = *h->pieces_state;
    const bool cached = all && S.table_is_all && S.all_mask == spec->type_mask && S.all_gen[0] == W.atoms_gen && S.all_gen[1] == Y.atoms_gen;
    if (!cached) {
        S.table_is_all = false;  // (until the table below is complete)
        std::vector<EggPiecesTask> tasks[2];
        int32_t largest[2] = {0, 0};
        rc = for_each_requested_atom(h, "egg_pieces", spec->type_mask, n_ids, ids, [&](const Atom &at, int w, int32_t slot) {
            if (at.count > EGG_PC_MAX_ATOM)
                return fail(h, EGG_ERR_INTERNAL, "egg_pieces: atom %d of type %d holds %d particles from %d", (int)(&at - h->sys[w].atoms.data()), w,
                            (int)at.count, (int)at.offset);
            const int c = at.count <= EGG_PC_WAVE_ATOM ? 0 : 1;
            tasks[c].push_back(EggPiecesTask{at.offset, at.count, w, slot});
            largest[c] = std::max(largest[c], at.count);
            return (int)EGG_OK;
        });
        if (rc != EGG_OK) return rc;
        for (int c = 0; c < 2; ++c) {
            S.n_class[c] = (int32_t)tasks[c].size();
            S.max_class[c] = largest[c];
        }
        tasks[0].insert(tasks[0].end(), tasks[1].begin(), tasks[1].end());  // one table, one copy
        HIP_TRY(h, S.d_tasks.reserve(tasks[0].size(), false, nullptr));
        if (!tasks[0].empty())
            HIP_TRY(h, hipMemcpy(S.d_tasks.p, tasks[0].data(), tasks[0].size() * sizeof(EggPiecesTask), hipMemcpyHostToDevice));
        S.table_is_all = all;
        S.all_mask = spec->type_mask;
        S.all_gen[0] = W.atoms_gen;
        S.all_gen[1] = Y.atoms_gen;
    }
    const bool launch = S.n_class[0] + S.n_class[1] > 0;
    const bool count_sweeps = getenv("EGGSIM_PIECES_SWEEPS") != nullptr;
    if (launch) {
        EggPiecesArgs A{};
        for (int w = 0; w < 2; ++w) {
            System &s = h->sys[w];
            A.x[w] = s.x[s.cur].p;
            A.y[w] = s.y[s.cur].p;
            A.radius[w] = s.radius.p;
            A.reach[w] = spec->reach[w];
        }
        // the LDS of a class's largest atom, granted once per kernel and size
        const void *const kernels[2] = {(const void *)egg_pieces_wave_kernel, (const void *)egg_pieces_block_kernel};
        for (int c = 0; c < 2; ++c) {
            const size_t need = S.n_class[c] ? pieces_lds(S.max_class[c]) : 0;
            if (need <= S.lds_granted[c]) continue;
            if (hipFuncSetAttribute(kernels[c], hipFuncAttributeMaxDynamicSharedMemorySize, (int)pieces_lds(EGG_PC_MAX_ATOM)) != hipSuccess) {
                (void)hipGetLastError();
                return fail(h, EGG_ERR_UNSUPPORTED, "egg_pieces: the device grants no %zu bytes of LDS to a workgroup (an atom of %d particles)",
                            need, (int)S.max_class[c]);
            }
            S.lds_granted[c] = pieces_lds(EGG_PC_MAX_ATOM);
        }
        HIP_TRY(h, S.d_out.reserve(records.size(), false, nullptr));
        A.out = S.d_out.p;
        if (count_sweeps) {
            HIP_TRY(h, S.d_sweeps.reserve(records.size(), false, nullptr));
            A.sweeps = S.d_sweeps.p;
        }
        HIP_TRY(h, hipStreamSynchronize(Y.stream));
        for (int w = 0; w < 2; ++w) {
            if (!host_labels[w] || h->sys[w].n == 0 || !(spec->type_mask >> w & 1)) continue;
            HIP_TRY(h, S.d_labels[w].reserve((size_t)h->sys[w].n, false, nullptr));
            HIP_TRY(h, hipMemsetAsync(S.d_labels[w].p, 0xFF, (size_t)h->sys[w].n * sizeof(int32_t), W.stream));  // -1
            A.labels[w] = S.d_labels[w].p;
        }
        // (a record without a task stays as the host zeroed it: the copy back takes the tasks' records only)
        HIP_TRY(h, hipMemsetAsync(S.d_out.p, 0, records.size() * sizeof(EggPieceSummary), W.stream));
        if (count_sweeps) HIP_TRY(h, hipMemsetAsync(S.d_sweeps.p, 0, records.size() * sizeof(int32_t), W.stream));
        for (int c = 0; c < 2; ++c) {
            if (S.n_class[c] == 0) continue;
            A.tasks = S.d_tasks.p + (c ? S.n_class[0] : 0);
            A.n_tasks = S.n_class[c];
            const unsigned groups = (unsigned)grid_cap(h, S.n_class[c], kGroupsPerCu, "EGGSIM_PIECES_GROUPS_PER_CU");
            const size_t lds = pieces_lds(S.max_class[c]);
            if (c == 0)
                hipLaunchKernelGGL(egg_pieces_wave_kernel, dim3(groups), dim3(EGG_WAVE), lds, W.stream, A);
            else
                hipLaunchKernelGGL(egg_pieces_block_kernel, dim3(groups), dim3(EGG_PC_BLOCK), lds, W.stream, A);
            HIP_TRY(h, hipGetLastError());
            h->stats.kernel_launches += 1;
        }
        HIP_TRY(h, hipMemcpyAsync(records.data(), S.d_out.p, records.size() * sizeof(egg_piece_summary), hipMemcpyDeviceToHost, W.stream));
        HIP_TRY(h, hipStreamSynchronize(W.stream));
        if (count_sweeps) {
            std::vector<int32_t> sweeps(records.size());
            HIP_TRY(h, hipMemcpy(sweeps.data(), S.d_sweeps.p, sweeps.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
            long long sum = 0, tasks = 0;
            int32_t most = 0, least = std::numeric_limits<int32_t>::max();
            for (size_t q = 0; q < sweeps.size(); ++q)
                if (records[q].n > 0) {
                    sum += sweeps[q];
                    ++tasks;
                    most = std::max(most, sweeps[q]);
                    least = std::min(least, sweeps[q]);
                }
            fprintf(stderr, "egg_pieces sweeps: atoms %lld min %d max %d sum %lld\n", tasks, tasks ? (int)least : 0, (int)most, sum);
        }
    }
    for (int w = 0; w < 2; ++w) {
        if (!host_labels[w] || h->sys[w].n == 0) continue;
        if (launch && (spec->type_mask >> w & 1))
            HIP_TRY(h, hipMemcpy(host_labels[w], S.d_labels[w].p, (size_t)h->sys[w].n * sizeof(int32_t), hipMemcpyDeviceToHost));
        else
            memset(host_labels[w], 0xFF, (size_t)h->sys[w].n * sizeof(int32_t));
    }
    if (!records.empty()) memcpy(out, records.data(), records.size() * sizeof(egg_piece_summary));
    return EGG_OK;
}

}  // extern "C"
