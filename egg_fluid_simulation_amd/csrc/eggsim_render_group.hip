// eggsim_render_group.hip -- device side of a device group's draw ("Several devices"): the gather
// of one source handle's particles into the render device's shadow arrays.  Everything after the gather is
// eggsim_render.hip, unchanged.
#include <hip/hip_runtime.h>

#include "eggsim_device.h"

// One thread per SOURCE particle i: lanes of a wave read consecutive doubles of one field and -- runs being whole
// batches -- write consecutive doubles too, except where a run ends inside the wave.  The run of i is found by walking
// forward from the run of the workgroup's first particle (a table the host keeps per 256 particles): a batch has at
// least two particles, in practice 15 or more, so the walk is a handful of cached loads, not a bisection over every
// atom of the handle.  Plain loads, plain stores, no atomics: every destination has exactly one source.
extern "C" __global__ void __launch_bounds__(EGG_GATHER_BLOCK) egg_group_gather_kernel(EggGatherArgs A) {
    const int i = (int)(blockIdx.x * EGG_GATHER_BLOCK + threadIdx.x);
    if (i >= A.n) return;
    int r = A.block_run[blockIdx.x];
    while (r + 1 < A.n_runs && i >= A.run_src[r + 1]) ++r;
    const int d = A.run_dst[r] + (i - A.run_src[r]);
    if (d < 0 || d >= A.total) return;  // (cannot happen with the host's tables; never write outside the shadows)
    if (A.n_fields == EGG_GATHER_FIELDS) {  // a draw: all loads in flight before the first store
        double v[EGG_GATHER_FIELDS];
#pragma unroll
        for (int f = 0; f < EGG_GATHER_FIELDS; ++f) v[f] = A.src[f][i];
#pragma unroll
        for (int f = 0; f < EGG_GATHER_FIELDS; ++f) A.dst[f][d] = v[f];
        return;
    }
#pragma unroll
    for (int f = 0; f < EGG_GATHER_FIELDS; ++f)  // a download: one field
        if (f < A.n_fields) A.dst[f][d] = A.src[f][i];
}
