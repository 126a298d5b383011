// eggsim_relaxed_wire.hip -- gfx950 kernels of the relaxed-order ghost halo between PROCESSES (DESIGN.md section 2.7,
// "Several processes"; host: eggsim_host_relaxed_wire.hip).  The pass itself is eggsim_relaxed.hip's, in its group
// instantiations (local entries + ghosts with keys); only the two kernels that move the ghosts differ from the device
// group's: no pointer here leads into another handle's memory.
//
//   egg_rx_wire_pack_kernel    sender: the destinations' cell boxes come from a small array in the sender's own memory
//                              (the host filled it from the wire); per destination ONE contiguous message --
//                              word 0 the record count, then the EggGhost records -- that the host copies to the wire
//                              (egg_rx_wire_pack_visc_kernel: the viscosity pass's, whose records carry u = pos - prev
//                              in the words of inverse mass and radius)
//   egg_rx_wire_unpack_kernel  receiver: messages in local memory (a staging copy of the received tensors) into the
//                              ghost entries [n, n + ghosts)
//
// Plain vector loads and stores; the appends are wave-aggregated (one atomic per wave and destination; rx_append and
// rx_cell of eggsim_device.h, shared with eggsim_relaxed.hip).
#include <hip/hip_runtime.h>
#include "eggsim_device.h"

// Sender: every local particle whose cell lies in a destination's cell box grown by one cell on each side goes into
// that destination's message, in any order (the receiver's rank kernel orders by key).  A particle goes to a
// destination at most once: a message with room for n records cannot overflow.
extern "C" __global__ void __launch_bounds__(256) egg_rx_wire_pack_kernel(EggRxWirePackArgs P) {
    __shared__ int32_t bx[EGG_RX_MAX_GROUP][4];  // lo x, hi x, lo y, hi y, grown (|cell| <= 2^30: no overflow)
    if (threadIdx.x < (unsigned)P.n_dest) {
        const int32_t *b = P.boxes + (size_t)threadIdx.x * EGG_RX_WIRE_BOX;
        if (b[4]) {  // the destination wrote no position: nothing is near it
            bx[threadIdx.x][0] = bx[threadIdx.x][2] = 1;
            bx[threadIdx.x][1] = bx[threadIdx.x][3] = 0;
        } else {
            bx[threadIdx.x][0] = b[0] - 1;
            bx[threadIdx.x][1] = b[2] + 1;
            bx[threadIdx.x][2] = b[1] - 1;
            bx[threadIdx.x][3] = b[3] + 1;
        }
    }
    __syncthreads();
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    const bool live = i < P.n;
    int32_t cx = 0, cy = 0;
    EggGhost g{};
    if (live) {
        const double2 p = P.pos[i];
        (void)rx_cell(p, P.cell_size, cx, cy);  // ((0, 0) for a bad cell: the insert kernel of the pass flags it)
        g.x = p.x;
        g.y = p.y;
        g.inv_mass = P.inv_mass[i];
        g.radius = P.radius[i];
        g.key = rx_key_word(P.ekey[i], P.p_atom, P.atom_tag, i);
    }
    for (int k = 0; k < P.n_dest; ++k) {
        const bool take = live && rx_in_box(bx[k], cx, cy);
        unsigned long long *m = P.msg + (size_t)k * (size_t)P.stride;
        const int slot = rx_append(m, take);
        if (take) reinterpret_cast<EggGhost *>(m + 1)[slot] = g;
    }
}

// The viscosity pass's sender: the same selection -- the take test is shared (rx_in_box); the box decode is written out
// again, because behind a shared helper or as a template egg_rx_wire_pack_kernel no longer compiles to the instructions it
// had -- and the two payload words of a record carry u = pos - prev instead of inverse mass and radius.
extern "C" __global__ void __launch_bounds__(256) egg_rx_wire_pack_visc_kernel(EggRxWirePackViscArgs V) {
    const EggRxWirePackArgs &P = V.p;
    __shared__ int32_t bx[EGG_RX_MAX_GROUP][4];  // lo x, hi x, lo y, hi y, grown (|cell| <= 2^30: no overflow)
    if (threadIdx.x < (unsigned)P.n_dest) {
        const int32_t *b = P.boxes + (size_t)threadIdx.x * EGG_RX_WIRE_BOX;
        if (b[4]) {  // the destination wrote no position: nothing is near it
            bx[threadIdx.x][0] = bx[threadIdx.x][2] = 1;
            bx[threadIdx.x][1] = bx[threadIdx.x][3] = 0;
        } else {
            bx[threadIdx.x][0] = b[0] - 1;
            bx[threadIdx.x][1] = b[2] + 1;
            bx[threadIdx.x][2] = b[1] - 1;
            bx[threadIdx.x][3] = b[3] + 1;
        }
    }
    __syncthreads();
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    const bool live = i < P.n;
    int32_t cx = 0, cy = 0;
    EggGhost g{};
    if (live) {
        const double2 p = P.pos[i];
        (void)rx_cell(p, P.cell_size, cx, cy);  // ((0, 0) for a bad cell: the insert kernel of the pass flags it)
        g.x = p.x;
        g.y = p.y;
        const double2 pv = V.prev[i];
        g.inv_mass = p.x - pv.x;
        g.radius = p.y - pv.y;
        g.key = rx_key_word(P.ekey[i], P.p_atom, P.atom_tag, i);
    }
    for (int k = 0; k < P.n_dest; ++k) {
        const bool take = live && rx_in_box(bx[k], cx, cy);
        unsigned long long *m = P.msg + (size_t)k * (size_t)P.stride;
        const int slot = rx_append(m, take);
        if (take) reinterpret_cast<EggGhost *>(m + 1)[slot] = g;
    }
}

// Receiver: the records of every received message, appended to the ghost entries [n, n + n_ghost).  Grid: x over the
// largest message, y over the messages.  A message never yields more records than the host was told it holds.
extern "C" __global__ void __launch_bounds__(256) egg_rx_wire_unpack_kernel(EggRxWireUnpackArgs U) {
    const int s = (int)blockIdx.y;
    const int q = (int)(blockIdx.x * 256 + threadIdx.x);
    const unsigned long long *m = U.msg[s];
    const unsigned long long said = m[0];
    const int cnt = said < (unsigned long long)U.cap[s] ? (int)said : U.cap[s];
    if ((int)(blockIdx.x * 256) >= cnt) return;  // (uniform over the workgroup)
    const bool take = q < cnt;
    const int slot = rx_append(U.n_ghost, take);
    if (take && slot < U.cap_ghost) {
        const EggGhost r = reinterpret_cast<const EggGhost *>(m + 1)[q];
        U.pos[U.n + slot] = make_double2(r.x, r.y);
        U.gwr[slot] = make_double2(r.inv_mass, r.radius);
        U.ekey[U.n + slot] = (int32_t)r.key;
        if (U.gtag) U.gtag[slot] = (int32_t)(r.key >> 32);
    }
}
