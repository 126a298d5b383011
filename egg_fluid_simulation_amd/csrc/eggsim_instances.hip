// eggsim_instances.hip -- device side of egg_get_instances / egg_instances_begin / egg_group_get_instances /
// egg_draw_source_instances ("The instanced-draw record"): the reference's data mesh and colour
// mesh (L:513-523, L:744-877) of every particle of one type, in the vertex format its shader reads.
#include <hip/hip_runtime.h>

#include "eggsim_device.h"

// One workgroup packs EGG_INSTANCE_BLOCK consecutive particles, one thread each.
//  * Loads: seven global_load_dwordx2, consecutive lanes on consecutive doubles of one field, all issued before the first
//    use; one v_cvt_f32_f64 each (round to nearest even, denormals kept: the narrowing numpy's astype(float32) does).
//  * Stores: a record is 28 B, so a thread storing its own record would issue seven dword stores 28 B apart.  The
//    workgroup's records are one contiguous stretch instead -- 256 x 28 B = 7,168 B = 448 x 16 B, and it starts at a
//    multiple of 7,168 B in a 16-byte aligned array --: the floats go through LDS (ds_write_b32 at a stride of 7 dwords:
//    odd, no bank conflict) and leave as global_store_dwordx4, consecutive lanes on consecutive 16 B (1 KiB per wave
//    instruction).  Only the last workgroup of a launch can end off a 16 B boundary; it finishes with dword stores.
//  * Colour: the particle's atom by bisection over the atoms' first particles, as the splat does it
//    (egg_render_splat_kernel), then one 16 B load and one 16 B store per thread, consecutive lanes on consecutive 16 B.
// No atomics; every destination has exactly one source, so the result does not depend on scheduling.
extern "C" __global__ void __launch_bounds__(EGG_INSTANCE_BLOCK) egg_instances_kernel(EggInstanceArgs A) {
    __shared__ __attribute__((aligned(16))) float rec[EGG_INSTANCE_BLOCK * EGG_GATHER_FIELDS];
    const int tid = (int)threadIdx.x;
    const long long first = (long long)blockIdx.x * EGG_INSTANCE_BLOCK;
    const long long left = (long long)A.n - first;
    const int m = left < EGG_INSTANCE_BLOCK ? (int)left : EGG_INSTANCE_BLOCK;  // particles of this workgroup
    if (tid < m) {
        const long long i = first + tid;
        if (A.data) {
            double v[EGG_GATHER_FIELDS];
#pragma unroll
            for (int f = 0; f < EGG_GATHER_FIELDS; ++f) v[f] = A.src[f][i];
#pragma unroll
            for (int f = 0; f < EGG_GATHER_FIELDS; ++f) rec[tid * EGG_GATHER_FIELDS + f] = (float)v[f];
        }
        if (A.color) {
            int lo = 0, hi = A.n_atoms - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (A.atom_offset[mid] <= i)
                    lo = mid;
                else
                    hi = mid - 1;
            }
            A.color[i] = A.atom_color[lo];
        }
    }
    if (!A.data) return;  // (uniform over the launch)
    __syncthreads();
    float *out = A.data + first * EGG_GATHER_FIELDS;
    const int words = m * EGG_GATHER_FIELDS;
    for (int q = tid; 4 * q < words; q += EGG_INSTANCE_BLOCK) {
        if (4 * q + 4 <= words) {
            reinterpret_cast<float4 *>(out)[q] = reinterpret_cast<const float4 *>(rec)[q];
        } else {
            for (int k = 4 * q; k < words; ++k) out[k] = rec[k];
        }
    }
}
