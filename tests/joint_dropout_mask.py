"""The dropout mask of the fused joint, restated in NumPy uint64 arithmetic -- TEST INFRASTRUCTURE ONLY (a helper, not a
test file).

The definition (include/warp_rnnt_amd_joint_dropout.h, warp_rnnt_amd/csrc/philox.h), independent of the C++ code:
  Philox4x32-10: multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85; ten rounds
  key     = (seed & 0xffffffff, seed >> 32), seed taken as a uint64
  counter = (n, t, u, k >> 2); output word (k & 3) decides element k of h[n,t,u,:]
  keep iff word < thr,  thr = min(2^32 - 1, floor((1 - (double)p) * 2^32)),  p the fp32 argument
  scale   = (float)(1 / (1 - (double)p))
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
LOW = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four arrays (broadcastable) of values below 2^32, key: two such; returns the four output words as uint64
    arrays holding 32-bit values."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & LOW for c in counter)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & LOW for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                      # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & LOW, (p0 >> S32) ^ c3 ^ k1, p0 & LOW
        k0, k1 = (k0 + W0) & LOW, (k1 + W1) & LOW
    return c0, c1, c2, c3


def threshold(p):
    """thr of the fp32 probability p, as a Python int."""
    q = 1.0 - float(np.float32(p))                      # (double)p, exactly
    return min(2 ** 32 - 1, int(np.floor(q * 4294967296.0)))


def scale(p):
    """(float)(1 / (1 - (double)p)) as a Python float."""
    return float(np.float32(1.0 / (1.0 - float(np.float32(p)))))


def seed_u64(seed):
    return int(seed) & (2 ** 64 - 1)


def keep_mask(seed, p, N, T, U, H):
    """The (N,T,U,H) keep mask, bool."""
    s = seed_u64(seed)
    n = np.arange(N, dtype=np.uint64)[:, None, None, None]
    t = np.arange(T, dtype=np.uint64)[None, :, None, None]
    u = np.arange(U, dtype=np.uint64)[None, None, :, None]
    k4 = np.arange((H + 3) // 4, dtype=np.uint64)[None, None, None, :]
    shape = (N, T, U, (H + 3) // 4)
    words = philox4x32_10((np.broadcast_to(n, shape), np.broadcast_to(t, shape), np.broadcast_to(u, shape),
                           np.broadcast_to(k4, shape)), (np.uint64(s & 0xFFFFFFFF), np.uint64(s >> 32)))
    w = np.stack(words, axis=-1).reshape(N, T, U, -1)[..., :H]          # element k = word (k & 3) of group k >> 2
    return w < np.uint64(threshold(p))
