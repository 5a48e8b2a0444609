// Distributed log-domain alpha / beta lattice sweep for MI355X (gfx950), diagonal-major layout (padded or compact):
// the reference's arithmetic -- one fp32 lse per cell, core_gather.cu:22-35,106-126,207-227 -- with ONE WORKGROUP PER
// 64-COLUMN BLOCK of a sweep.
//
// The step is lattice_ws.hip's, literally (lattice_step.h: same instructions on the chain, same bits): lanes are
// lattice columns, blocks of K = 8 diagonals, one s_barrier per block, a COMPUTE wave that touches only registers and
// LDS.  What changes is everything around it.
//
// 1. WHERE the column blocks run.  In lattice_ws.hip they share a workgroup, hence a CU, and all meet at every
//    barrier.  Here a column block is a workgroup of its own (three waves), wherever the dispatcher puts it, and the
//    boundary column travels through L2:
//      * ring: one 8-byte granule {fp32 value, 32-bit tag} per diagonal and (sweep, boundary); the producer's storer
//        wave publishes the 8 granules of a block with one agent-scope (sc1) store instruction the interval after the
//        compute wave produced them; tag = launch epoch ^ hash(ring) ^ hash(diagonal), never 0, and the rings are
//        zeroed in front of every launch (launch_ring_prepare, below): a granule validates only if THIS launch wrote it;
//      * the consumer's loader wave fetches the granules of a block DLOAD intervals ahead (LDS-DMA, like the pairs),
//        checks the tags when the block is due, and only if the producer is not there yet polls (after letting it get
//        LAG blocks further ahead, so that the following look-ahead fetches hit).  No flag, no fence, no back-pressure:
//        the ring is as long as the sweep;
//      * work items (column block, sweep) come from an atomic counter in column-block-major order: whoever holds item
//        i knows that its left neighbour, item i - 2N, is held by a workgroup that is running or done -- no assumption
//        about dispatch order or residency, any batch size;
//      * every wait is bounded; a timeout flags the sweep for the single-workgroup kernel launched behind (which
//        returns at once otherwise) instead of hanging.
// 2. The memory side has NO data-dependent control flow around memory instructions and no compiler-counted loads.
//    Measured (profiles/r04_wd_trace_*.txt, ISA): with "guarded" steps at the ends of a column block's life (memory
//    instructions under conditions) the waitcnt pass assumes the worst at every join and each such interval waits for
//    everything in flight -- ~1.5 us instead of 0.4 -- and because the heads of a sweep's column blocks run one
//    after the other that was ~20 us per boundary, in lattice_ws.hip too.  Here:
//      * LOADER wave: the (blank,label) pairs of a block arrive by LDS-DMA (four `buffer_load_dwordx4 ... lds`: two
//        diagonals of 64 pairs each), the neighbour's granules by a fifth; every interval issues all five (an
//        out-of-range offset where there is nothing to fetch: zeros land), waits with ONE hand-counted
//        `s_waitcnt vmcnt` and never holds a byte of it in a register; polls are inline assembly that drains the
//        queue itself;
//      * STORER wave: values LDS -> HBM one block behind (per-lane predicate, dropped by the buffer range check) and the
//        publication of the boundary column; stores only, it never waits for memory.
// 3. Instruction fetch.  A wave runs a 200-instruction block of straight-line code cold in ~2.4 us (the trace: first
//    block of each variant), and a column block's first blocks are on the critical path of the whole sweep.  So the
//    block exists ONCE per variant (compute_block_ip: in-place prefetch instead of two register buffers and a loop
//    unrolled twice) and the storer wave -- idle for the first intervals anyway -- runs the compute loop "dry" for
//    one block per variant before it takes up its own work: same instructions, same addresses, a warm instruction
//    cache when the compute wave gets there.
// Values handed over are the compute wave's own fp32 X registers, so the results are bit-identical to
// lattice_ws.hip's whatever the placement and timing (tests/test_gpu_wd.py).
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <random>
#include <type_traits>

#include "common.h"
#include "kernels.h"
#include "lattice_launch.h"
#include "lattice_step.h"

namespace rnnt {

#define RNNT_WD_NS wd8
#define RNNT_WD_KK 8
#include "lattice_wd_body.h"
#undef RNNT_WD_NS
#undef RNNT_WD_KK
#define RNNT_WD_NS wd16
#define RNNT_WD_KK 16
#include "lattice_wd_body.h"
#undef RNNT_WD_NS
#undef RNNT_WD_KK

// ---------------------------------------------------------------------------------------------------------------
// Ring preparation (until round 5 in lattice_pd.hip, whose probability-domain kernel introduced the protocol).
// The library's launch counter of this device: module-scope device memory (zero when the code object is loaded,
// never part of anybody's workspace), so it cannot be recycled, scribbled over or left uninitialised, and every
// REPLAY of a captured graph advances it too -- kernel arguments are frozen at capture time, and with a frozen
// epoch the granules of the previous replay would carry this replay's tags.
// ---------------------------------------------------------------------------------------------------------------
__device__ unsigned g_launch_counter;

// In front of every launch: clears the redo flags and the queue head (n words), hands the next value of the launch
// counter to the kernel (p[n]) and zeroes the hand-over rings (mail_vec 16-byte words; tag 0 never validates), so
// that nothing the workspace held before -- it is caller scratch with unspecified contents -- can be taken for a
// granule of this launch.  The clear is 1 % of the bytes the sweeps move.
__global__ void __launch_bounds__(256) k_prepare(int* p, int n, uint4* mail, size_t mail_vec) {
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i < n; i += 256) p[i] = 0;
        if (threadIdx.x == 0) p[n] = (int)(atomicAdd(&g_launch_counter, 1u) + 1u);
    }
    const uint4 z = make_uint4(0, 0, 0, 0);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < mail_vec; i += (size_t)gridDim.x * 256) mail[i] = z;
}

// host part of the launch epoch: random start, +1 per call
static unsigned next_launch_epoch() {
    // granules of earlier launches (same buffer) never validate.  Random start so that a recycled allocation of
    // another process does not either; the device-side counter (k_prepare) is added in the kernel.
    static std::atomic<unsigned> epoch{std::random_device{}()};
    return epoch.fetch_add(1, std::memory_order_relaxed) + 1;
}

// clears n_flags words at `flags` (redo flags + queue head), stores the next value of the launch counter at
// flags[n_flags] and zeroes ring_bytes (a multiple of 16) at `rings`
static hipError_t launch_ring_prepare(hipStream_t stream, int* flags, int n_flags, void* rings, size_t ring_bytes) {
    // the flags (2N ints) and the queue head are contiguous in the workspace (api.hip: carve).  One tiny kernel:
    // hipMemsetAsync of these few bytes becomes two fill kernels of ~5 us each.
    const size_t mail_vec = ring_bytes / 16;
    const unsigned prep_blocks = (unsigned)std::min<size_t>(512, std::max<size_t>(1, mail_vec / (256 * 8)));
    k_prepare<<<prep_blocks, 256, 0, stream>>>(flags, n_flags, reinterpret_cast<uint4*>(rings), mail_vec);
    return hipGetLastError();
}

// Device address of g_launch_counter on the stream's device, for the producers that carry the preparation out themselves
// (they live in another translation unit: the address travels as a kernel argument).  One query per device and process.
static unsigned* launch_counter_address(hipStream_t stream) {
    static std::atomic<unsigned*> cached[64];
    int dev = -1, cur = -2;
    if (hipStreamGetDevice(stream, &dev) != hipSuccess || hipGetDevice(&cur) != hipSuccess) return nullptr;
    if (dev < 0 || dev >= 64 || dev != cur) return nullptr;     // (hipGetSymbolAddress answers for the CURRENT device)
    unsigned* p = cached[dev].load(std::memory_order_acquire);
    if (!p) {
        void* q = nullptr;
        if (hipGetSymbolAddress(&q, HIP_SYMBOL(g_launch_counter)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        p = static_cast<unsigned*>(q);
        cached[dev].store(p, std::memory_order_release);
    }
    return p;
}

size_t wd_mail_bytes(int N, int T, int U) {
    const int nA = column_blocks(U);
    // (by SHAPE only -- the larger of the two block sizes' rings: a workspace's size must not depend on a setting)
    const size_t pitch = std::max(wd8::ring_pitch(T, U), wd16::ring_pitch(T, U));
    size_t bytes = nA < 2 ? 0 : (size_t)2 * N * (nA - 1) * pitch * sizeof(wd8::u64);
#ifdef RNNT_WD_STATS       // the stamp table of the diagnostics build, behind the rings
    bytes += (size_t)2 * N * nA * std::max(wd8::trace_slots(T, U), wd16::trace_slots(T, U)) * 8 * sizeof(wd8::u64);
#endif
    return bytes;
}

// bytes of rings a launch on `a` with blocks of block_diagonals uses
static size_t wd_ring_bytes(const LatticeArgs& a, int N, int block_diagonals) {
    const int nA = column_blocks(a.U);
    const size_t pitch = block_diagonals == 16 ? wd16::ring_pitch(a.T, a.U) : wd8::ring_pitch(a.T, a.U);
    return nA < 2 ? 0 : (size_t)2 * N * (nA - 1) * pitch * sizeof(wd8::u64);
}

bool wd_ring_prep(hipStream_t stream, const LatticeArgs& a, int N, int block_diagonals, RingPrep* prep) {
    if (N <= 0 || !a.redo || !a.queue || a.queue != a.redo + 2 * N) return false;
    if (column_blocks(a.U) > 1 && !a.mail) return false;
    unsigned* counter = launch_counter_address(stream);
    if (!counter) return false;
    const size_t ring_bytes = wd_ring_bytes(a, N, block_diagonals);
    *prep = RingPrep{a.redo, 2 * N + 1, counter, reinterpret_cast<uint4*>(a.mail), ring_bytes / 16};
    return true;
}

hipError_t launch_lattice_wd(hipStream_t stream, const LatticeArgs& a0, int N, int block_diagonals, bool lone) {
    if (N <= 0) return hipSuccess;
    const int nA = column_blocks(a0.U);
#ifdef RNNT_WD_STATS
    if (lone || !a0.mail) return hipErrorNotSupported;
#endif
    if (lone ? (nA != 1 || a0.redo) : (a0.offs32 || !a0.redo || !a0.queue || (nA > 1 && !a0.mail)))
        return hipErrorNotSupported;                                     // (32-bit offsets: the plain launch only)
    if ((long long)2 * N * nA >= (1ll << 31)) return hipErrorNotSupported;
    LatticeArgs a = a0;
    if (lone) {               // nothing to prepare, nothing to redo behind
        a.queue = nullptr;
        a.mail = nullptr;
    } else {
        a.epoch = next_launch_epoch();
        if (!a.prepared) {     // (prepared: the producer of this call's pair plane did it at the tail of its own launch)
            const hipError_t e = launch_ring_prepare(stream, a.redo, 2 * N + 1, a.mail, wd_ring_bytes(a, N, block_diagonals));
            if (e != hipSuccess) return e;
        }
    }
    const dim3 grid(2 * N * nA), block(3 * WAVE);
    if (block_diagonals == 16) {
        if (is_compact(a)) wd16::k_lattice_wd<true><<<grid, block, 0, stream>>>(a, nA);
        else wd16::k_lattice_wd<false><<<grid, block, 0, stream>>>(a, nA);
    } else {
        if (is_compact(a)) wd8::k_lattice_wd<true><<<grid, block, 0, stream>>>(a, nA);
        else wd8::k_lattice_wd<false><<<grid, block, 0, stream>>>(a, nA);
    }
    return hipGetLastError();
}

// The single-workgroup form: one workgroup of 3 * ceil(U / 64) waves per sweep, nothing but the planes in global memory.
// Two column blocks (U <= 128) fit the 64 KiB every kernel gets; five (U <= 320) take the large-LDS opt-in, 148 KiB of the
// CU's 160 (LDS-DMA lands above 64 KiB as well: M0 carries the full address on gfx950 -- tests/test_gpu_wd.py).
hipError_t launch_lattice_wl(hipStream_t stream, const LatticeArgs& a, int N, int max_blocks) {
    if (N <= 0) return hipSuccess;
    const int nA = column_blocks(a.U);
    const size_t lds = sizeof(wd8::Smem) * nA;
    if (nA > max_blocks || nA > WL_MAX_BLOCKS || lds > 160 * 1024) return hipErrorNotSupported;
    const dim3 grid(2 * N), block((nA == 2 ? 8 : 3 * nA) * WAVE);
    const bool compact = is_compact(a);
    const bool wide = nA > 2;                           // which instantiation (launch bounds: 512 / 960 threads)
    if (lds > 64 * 1024) {
        static std::atomic<bool> lds_allowed[4][64];
        const void* fn = wide ? (compact ? reinterpret_cast<const void*>(&wd8::k_lattice_wl<true, 5>)
                                         : reinterpret_cast<const void*>(&wd8::k_lattice_wl<false, 5>))
                              : (compact ? reinterpret_cast<const void*>(&wd8::k_lattice_wl<true, 2>)
                                         : reinterpret_cast<const void*>(&wd8::k_lattice_wl<false, 2>));
        const hipError_t e = allow_large_lds(fn, sizeof(wd8::Smem) * (wide ? 5 : 2),
                                             lds_allowed[(wide ? 2 : 0) + (compact ? 1 : 0)]);
        if (e != hipSuccess) return e;
    }
    if (wide) {
        if (compact) wd8::k_lattice_wl<true, 5><<<grid, block, lds, stream>>>(a);
        else wd8::k_lattice_wl<false, 5><<<grid, block, lds, stream>>>(a);
    } else {
        if (compact) wd8::k_lattice_wl<true, 2><<<grid, block, lds, stream>>>(a);
        else wd8::k_lattice_wl<false, 2><<<grid, block, lds, stream>>>(a);
    }
    return hipGetLastError();
}

}  // namespace rnnt
