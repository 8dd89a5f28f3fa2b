// lf_tile.h - how the workgroups of a tile share its work and hand their partial sums over in the one-launch form of the
// persistent kernels (lf_free.h, lf_pers.h).  Both kernels run this protocol; it lives here once.
#pragma once
#include "lf_kernels.h"

namespace lf {

// (PB, the threads of a persistent workgroup, and VF, the virtual workgroups of a tile: lf_layout.h)
constexpr int PTW = 8;       // walkers per tile
constexpr int QSTRIDE = 9;   // counters per tile: [0] grid queue, [1..8] catalogue queues of XCD 0..7
// The one-launch form's hand-over by POLLING (tiles whose walkers are all on the cells: the normal case).  The slots of partB /
// partC hold PART_EMPTY between launches (the host fills them, every finisher leaves them so); a workgroup writes its partial
// sums through and is done; the tile's FINISHER reads the slots past its caches until none is empty, adds them up and empties
// them again.  Against the counter (every workgroup: wait for the stores' acknowledgements, count, wait for the count; the last
// one: load, add) the launch's critical path loses two of its three trips to memory.
// WHO finishes: lf_free - the workgroup the deal expects to END LAST (the physical rank with the largest dealt cost, from the
// host: lf_hostprep.h deal_finishers, tile_finisher below), so that the others' sums are in memory when it gets there and the
// launch's last sums go from its own registers straight into the final addition: its own slots it neither stores nor polls
// nor empties (they stay PART_EMPTY), their values reach finalize_wave through LDS in the slots' positions - the order of
// every sum is the deal's, whoever adds.  (With the last rank - the lightest of the deal, done early - as finisher the slowest
// workgroup's store, half a poll round and the poll's way back lay between the launch's last sum and its end: DESIGN.md 3.4d.)
// lf_pers, and lf_free without a deal or with "poll" off: the workgroup of the last physical rank.
// A partial sum is never PART_EMPTY (a NaN is made canonical before it is stored);
// a finisher that has polled PART_POLLS times without success writes NaN (emcee raises on NaN) and sets the error word.
constexpr unsigned long long PART_EMPTY = 0x7ff8dead7ff8deadull;
constexpr int PART_POLLS = 1 << 19;

// The rank of this workgroup among the fgroup that serve the tile: workgroup g serves tiles (g / 8) % ntiles, + tile_stride, ...
__device__ __forceinline__ void tile_ranks(int tile, int ntiles, int tile_stride, int& fgroup, int& frank) {
    fgroup = 8;
    frank = (int)blockIdx.x & 7;
    if (ntiles <= tile_stride) {
        const int k = (int)blockIdx.x >> 3;   // (here tile = k mod ntiles, and the groups k, k + ntiles, ... share it)
        fgroup = 8 * ((tile_stride - tile + ntiles - 1) / ntiles);
        frank += 8 * ((k - tile) / ntiles);
    }
}

// lf_free's finisher of a tile served by fgroup workgroups: byte fgroup / 8 - 1 of the host's word (FreeArgs::fin_ranks), never
// past the last rank.  The rank depends on the context and on fgroup only: a group that loops over several tiles keeps one
// finisher, and nobody waits on a waiter.
constexpr int FIN_LAST = 0x1f170f07;      // the last rank of every group size
__device__ __forceinline__ int tile_finisher(int fin_ranks, int fgroup) {
    return min((fin_ranks >> (fgroup - 8)) & 0xff, fgroup - 1);
}

// A partial sum: in the fused form it is read by a workgroup on another XCD while the launch is still running, so it is
// written THROUGH this XCD's L2 (a relaxed store of agent scope: scope bits on the one store - no cache-wide write-back or
// invalidate, which is what a fence of that scope costs: measured 154 us per evaluation instead of 30)
template <bool FUSED>
__device__ __forceinline__ void pstore(double* p, double v) {
    if (FUSED) __hip_atomic_store(p, v == v ? v : __builtin_nan(""), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (never PART_EMPTY)
    else *p = v;
}

// STEP: thread t of the last wave, idle once its share of the tables is on its way, makes the accept step's two logarithms for
// walker w0 + t - (PB - 64) of the tile ahead, from the same Philox draws as the proposal's stretch factor and the accept step's
// uniform - bit for bit what accept_walker would make in the epilogue
template <bool STEP>
__device__ __forceinline__ void accept_terms_ahead(const StepArgs& sp, const AcceptArgs& ap, int w0, int nw, int t, double* spre) {
    if (STEP && t >= PB - 64 && t < PB - 64 + nw) {
        const int wl = t - (PB - 64);
        unsigned int rr[4];
        sampler_draw(sp.step, sp.half, w0 + wl, 0, sp.seed, rr);
        accept_terms(ap, w0 + wl, stretch_z(sp.a, u53(rr[0], rr[1])), spre[2 * wl], spre[2 * wl + 1]);
    }
}

// Lane ln of walker w's wave empties the walker's slots for the next launch (visible to it: a kernel boundary lies between):
// the first nC of partC, the first nB of partB.  own: the lane's slots were never written (lf_free's finisher keeps its own sums)
__device__ __forceinline__ void empty_slots(double* partB, double* partC, int w, int nslot, int nB, int nC, int ln, bool own = false) {
    if (ln < nC && !own) __hip_atomic_store(partC + (size_t)w * nslot + ln, __longlong_as_double((long long)PART_EMPTY), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ln < nB && !own) __hip_atomic_store(partB + (size_t)w * nslot + ln, __longlong_as_double((long long)PART_EMPTY), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The polling finisher (PART_EMPTY above), lane ln of walker w's wave: reads the first nC slots of partC and nB of partB past
// its caches until none is empty, leaves what it read in pre (pre[0] partC's slot ln, pre[1] partB's) and empties the slots
// again.  A lane whose slots have arrived does not load again: only the lanes still empty go round (the polls of 16 finishers x 8
// waves share the memory system with the workgroups still at work).  own: the lane's slots are this workgroup's own - pre holds
// them already, they are neither read nor emptied.  The sum itself is the kernel's: finalize_wave with the values in hand.
__device__ __forceinline__ void poll_finish(double* partB, double* partC, int w, int nslot, int nB, int nC, int ln, int* err, double (&pre)[2],
                                            bool own = false) {
    double* __restrict__ pb = partB + (size_t)w * nslot;
    double* __restrict__ pc = partC + (size_t)w * nslot;
    int tries = 0;
    bool wc = ln < nC && !own, wb = ln < nB && !own;      // still empty
    do {
        if (wc) pre[0] = __hip_atomic_load(pc + ln, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (wb) pre[1] = __hip_atomic_load(pb + ln, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        wc = wc && (unsigned long long)__double_as_longlong(pre[0]) == PART_EMPTY;
        wb = wb && (unsigned long long)__double_as_longlong(pre[1]) == PART_EMPTY;
    } while (__any(wc || wb) && ++tries < PART_POLLS);
    if (tries >= PART_POLLS) {        // (cannot happen while the device runs the launch's other workgroups)
        pre[0] = pre[1] = __builtin_nan("");
        if (ln == 0) atomicExch(err, 1);
    }
    empty_slots(partB, partC, w, nslot, nB, nC, ln, own);
}

// This thread's number, its wave and its lane, as a kernel makes them (lf_free: anew at every use, see fresh_tid there)
struct TileThread {
    int t, v, ln;
};

// The counting finisher, for tiles whose partial sums have no fixed writer to poll for.  This workgroup's partial sums are
// out - written through, and complete once its waves have waited for their stores' acknowledgements (the explicit
// s_waitcnt: the compiler does not emit one for a workgroup-scope fence, and the count must not overtake a partial sum on its
// way to memory); the count (one lane's returning atomic of agent scope on the tile's counter q[0], into sdone) comes after
// the barrier.  The last of the tile's fgroup workgroups to count runs fin(v, ln) on the waves of the tile's nw walkers -
// the kernel's sum, reading the partials from memory (finalize_wave<true>), and empty_slots when the next launch's tiles may
// poll - and zeroes the tile's counters for the next launch.  me() gives this thread's TileThread.
template <class Me, class Fin>
__device__ __forceinline__ void count_finish(int* q, int& sdone, int fgroup, int nw, Me&& me, Fin&& fin) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (every wave: its write-through stores have been acknowledged)
    __threadfence_block();
    __syncthreads();
    if (me().t == 0) sdone = atomicAdd(q, 1);
    __syncthreads();
    if (sdone == fgroup - 1) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const TileThread m = me();
        if (m.v < nw) fin(m.v, m.ln);
        if (m.t < QSTRIDE) q[m.t] = 0;
    }
}

}  // namespace lf
