// eggsim_draw_pack.hip -- device side of egg_draw_pack ("Several processes"): the draw record of
// every particle of one type of one handle as ONE message for the render rank.
#include <hip/hip_runtime.h>

#include "eggsim_device.h"

// One thread per particle i.  The seven loads (one global_load_dwordx2 each, consecutive lanes read consecutive doubles)
// are all in flight before the first of the seven stores (global_store_dwordx2, consecutive again: field f starts at
// dst + f * n).  14 values' worth of registers, no LDS, no scratch, no atomics: every destination has one source.
extern "C" __global__ void __launch_bounds__(EGG_GATHER_BLOCK) egg_draw_pack_kernel(EggDrawPackArgs A) {
    const int i = (int)(blockIdx.x * EGG_GATHER_BLOCK + threadIdx.x);
    if (i >= A.n) return;
    double v[EGG_GATHER_FIELDS];
#pragma unroll
    for (int f = 0; f < EGG_GATHER_FIELDS; ++f) v[f] = A.src[f][i];
#pragma unroll
    for (int f = 0; f < EGG_GATHER_FIELDS; ++f) A.dst[(size_t)f * (size_t)A.n + (size_t)i] = v[f];
}
