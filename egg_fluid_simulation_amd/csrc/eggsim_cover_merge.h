// eggsim_cover_merge.h -- how the cover planes of several handles become one answer (include/eggsim_cover.h; DESIGN.md
// section 2.14): cover planes are added, owner planes -- taken as keys, which are the ids of the whole scene -- merged by
// unsigned minimum, and the counts that are not additive recounted from the merged planes.  Plain C++ without a device: the
// group (eggsim_group.cpp) is its one caller in the library, and it compiles alone under a sanitizer for its test.
#pragma once
#include <cstddef>
#include <cstdint>

namespace eggcover {

// one handle's planes into the merged ones.  `words` = 2 * ny * nx.  owner / one_owner may both be null.  The owner words are
// labels every handle agrees on (keys); -1 (none) is the largest unsigned value and loses against every label.
inline void merge_planes(size_t words, int32_t *cover, uint32_t *owner, const int32_t *one_cover, const int32_t *one_owner) {
    for (size_t q = 0; q < words; ++q) cover[q] = (int32_t)((uint32_t)cover[q] + (uint32_t)one_cover[q]);
    if (!owner || !one_owner) return;
    for (size_t q = 0; q < words; ++q)
        if ((uint32_t)one_owner[q] < owner[q]) owner[q] = (uint32_t)one_owner[q];
}

// covered[2], covered_both, covered_any of merged planes [2][cells]
inline void recount(size_t cells, const int32_t *cover, int64_t covered[2], int64_t *covered_both, int64_t *covered_any) {
    covered[0] = covered[1] = 0;
    *covered_both = *covered_any = 0;
    for (size_t c = 0; c < cells; ++c) {
        const bool a = cover[c] > 0, b = cover[cells + c] > 0;
        covered[0] += a;
        covered[1] += b;
        *covered_both += a && b;
        *covered_any += a || b;
    }
}

}  // namespace eggcover
