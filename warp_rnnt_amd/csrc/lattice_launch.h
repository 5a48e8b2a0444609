// Internal to the lattice family (lattice.hip, lattice_ws.hip, lattice_wd.hip): the per-kernel launchers that
// launch_lattice dispatches to by the plan (lattice_plan.h), and the large-LDS opt-in two of them need.
// Each launcher keeps its own argument guards and answers hipErrorNotSupported for a call it cannot take.
#pragma once
#include <atomic>

#include "kernels.h"
#include "lattice_plan.h"

namespace rnnt {

// lattice_ws.hip: compute + I/O wave pairs, all column blocks of a sweep in one workgroup (diagonal-major loader only);
// hipErrorNotSupported when U > 512.  With a.redo set only the (utterance, direction) pairs flagged there are swept.
hipError_t launch_lattice_ws(hipStream_t stream, const LatticeArgs& a, int N);
// lattice_wd.hip: one three-wave workgroup per 64-column block, in blocks of block_diagonals (8 or 16) diagonals.
// lone: one column block per sweep and no flags -- a plain launch.  Else boundary columns through L2 rings (padded or 64-bit
// compact; any U): needs a.redo, a.queue = a.redo + 2N with the launch counter's value behind it and -- for U > 64 -- a.mail
// of wd_mail_bytes(N,T,U) bytes; zeroes flags, queue head and rings itself unless a.prepared.  Sweeps it flags in a.redo (a
// lost hand-over: never observed outside the short-spin build) are for the caller to redo with a single-workgroup kernel.
hipError_t launch_lattice_wd(hipStream_t stream, const LatticeArgs& a, int N, int block_diagonals, bool lone);
// ... and its single-workgroup form (lattice_wd.hip: k_lattice_wl): all column blocks of a sweep as waves of one
// workgroup, boundary columns through LDS; needs nothing but the planes (no flags, no rings), padded or compact with
// either offset width, honours a.redo and a.beta_only.  hipErrorNotSupported beyond max_blocks (<= 5) column blocks.
hipError_t launch_lattice_wl(hipStream_t stream, const LatticeArgs& a, int N, int max_blocks);
// the parcel for a launch of the ring kernel on `a` with that block size (flags, queue and rings as launch_lattice_wd would
// prepare them), or false when there is nothing to prepare / the launch counter's address cannot be had for the stream's device
bool wd_ring_prep(hipStream_t stream, const LatticeArgs& a, int N, int block_diagonals, RingPrep* prep);

// More than 64 KiB of dynamic LDS needs an opt-in per kernel and per device.  hipFuncSetAttribute is idempotent and
// thread-safe, so the only state kept is the caller's "already done" bit per device for this kernel; devices beyond the
// table simply repeat the call every launch.
inline hipError_t allow_large_lds(const void* kernel, size_t bytes, std::atomic<bool> (&done)[64]) {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) dev = -1;
    const bool tracked = dev >= 0 && dev < 64;
    if (tracked && done[dev].load(std::memory_order_acquire)) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess && tracked) done[dev].store(true, std::memory_order_release);
    return e;
}

}  // namespace rnnt
