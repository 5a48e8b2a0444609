// The dropout mask of the fused joint (joint.hip; include/warp_rnnt_amd_joint_dropout.h): ONE
// definition, compiled for the device (the three joint kernels) and for the host (rnnt_amd_joint_dropout_mask_host, which
// lets a CPU-only box check it against the Random123 known answers).  Plain C++ integer arithmetic only.
//
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): counter (c0,c1,c2,c3), key (k0,k1),
// ten rounds of
//   (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0))
// with the key stepped by (W0, W1) between rounds.
//
// Element k of h[n,t,u,:] is kept iff word (k & 3) of philox(counter = (n, t, u, k >> 2), key = (seed low, seed high)) is
// below dropout_threshold(p); kept elements are multiplied by dropout_scale(p).  The counter holds n, t, u themselves,
// not a cell index over the padded shape: an utterance's mask does not depend on the batch around it.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RNNT_PHILOX_HD __host__ __device__ __forceinline__
#else
#define RNNT_PHILOX_HD inline
#endif

namespace rnnt {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;   // round multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;   // key increments (Weyl sequence)

struct Philox4 {
    uint32_t w[4];
};

RNNT_PHILOX_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// keep iff word < threshold: min(2^32 - 1, floor((1 - p) 2^32)) with 1 - p in double from the fp32 argument
RNNT_PHILOX_HD uint32_t dropout_threshold(float p) {
    const double t = (1.0 - (double)p) * 4294967296.0;
    return t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t;   // (t > 0: the conversion truncates = floor)
}
RNNT_PHILOX_HD float dropout_scale(float p) { return (float)(1.0 / (1.0 - (double)p)); }

// the four keep words of elements 4 k4 ... 4 k4 + 3 of h[n,t,u,:]
RNNT_PHILOX_HD Philox4 dropout_words(uint64_t seed, int n, int t, int u, int k4) {
    return philox4x32_10((uint32_t)n, (uint32_t)t, (uint32_t)u, (uint32_t)k4, (uint32_t)seed, (uint32_t)(seed >> 32));
}

}  // namespace rnnt
