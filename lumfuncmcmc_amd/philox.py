"""Philox4x32-10 and the 53-bit uniform of the device samplers (lf_kernels.h: philox4x32, u53, sampler_draw), in NumPy.

Counter (step, half, index, stream), key = seed: the host samplers and the tests draw exactly the numbers the kernels draw.
"""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32(c0, c1, c2, c3, k0, k1):
    """Vectorised Philox4x32-10 (uint64 arithmetic, words masked to 32 bits)."""
    c0, c1, c2, c3 = (np.asarray(x, dtype=np.uint64) & np.uint64(MASK) for x in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0 & MASK), np.uint64(k1 & MASK)
    m = np.uint64(MASK)
    for _ in range(10):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        n0 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & m
        n1 = p1 & m
        n2 = ((p0 >> np.uint64(32)) ^ c3 ^ k1) & m
        n3 = p0 & m
        c0, c1, c2, c3 = n0, n1, n2, n3
        k0 = (k0 + np.uint64(W0)) & m
        k1 = (k1 + np.uint64(W1)) & m
    return c0, c1, c2, c3


def draw(step, half, index, stream, seed):
    """sampler_draw: the four words for counter (step, half, index, stream) under key seed; index may be an array."""
    w = np.asarray(index, dtype=np.uint64)
    step, seed = int(step), int(seed)
    c0 = np.full_like(w, step & MASK)
    c1 = np.full_like(w, ((step >> 32) & MASK) ^ ((int(half) << 31) & MASK))
    return philox4x32(c0, c1, w, np.full_like(w, stream), seed & MASK, (seed >> 32) & MASK)


def u53(hi, lo):
    """53-bit uniform in [0, 1) from two words."""
    return (((hi << np.uint64(32)) | lo) >> np.uint64(11)).astype(np.float64) * 1.1102230246251565e-16
