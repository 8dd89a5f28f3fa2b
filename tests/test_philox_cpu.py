"""lumfuncmcmc_amd.philox against published vectors: philox4x32 is Philox4x32-10 of Random123 (Salmon et al. 2011; the
known-answer file of the library, kat_vectors), draw has the counter layout of lf_kernels.h's sampler_draw, u53 is a
53-bit uniform in [0, 1).  No GPU."""
import numpy as np
import pytest

from lumfuncmcmc_amd import philox

# counter x4, key x2 -> output x4 (Random123 kat_vectors: philox4x32 10)
KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff),
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_philox4x32_known_answers(ctr, key, out):
    got = philox.philox4x32(*ctr, *key)
    assert tuple(int(x) for x in got) == out


def test_philox4x32_is_vectorised_over_the_counter():
    """Arrays of counters give, element by element, what the scalars give - the three vectors at once, the key being common
    to a call, one call per key."""
    for ctr, key, out in KAT:
        cols = [np.array([c, 0, c]) for c in ctr]
        got = philox.philox4x32(*cols, *key)
        zero = philox.philox4x32(0, 0, 0, 0, *key)
        for word in range(4):
            assert got[word].dtype == np.uint64
            assert int(got[word][0]) == out[word] and int(got[word][2]) == out[word]
            assert int(got[word][1]) == int(zero[word])


def test_draw_counter_layout():
    """draw(step, half, index, stream, seed) = philox4x32(step's low word, step >> 32 with half in bit 31, index, stream;
    seed's low word, seed >> 32)."""
    seed = 0x299f31d0a4093822
    idx = np.array([0, 1, 0x13198a2e, 0xffffffff])
    for step, half, stream in [(0, 0, 0), (5, 1, 1), (0x243f6a88, 0, 2), ((3 << 32) | 7, 1, 0), ((0x7fffffff << 32) | 0xffffffff, 1, 3)]:
        got = philox.draw(step, half, idx, stream, seed)
        c1 = ((step >> 32) & 0x7fffffff) | (half << 31)
        ref = philox.philox4x32(np.full(4, step & 0xffffffff), np.full(4, c1), idx, np.full(4, stream), 0xa4093822, 0x299f31d0)
        for g, r in zip(got, ref):
            assert np.array_equal(g, r)
    # half moves bit 31 of word 1 and nothing else; step >> 32 sits in the low bits of the same word
    a = philox.draw(0, 1, idx, 0, seed)
    b = philox.philox4x32(np.zeros(4), np.full(4, 0x80000000), idx, np.zeros(4), 0xa4093822, 0x299f31d0)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    a = philox.draw(1 << 32, 0, idx, 0, seed)
    b = philox.philox4x32(np.zeros(4), np.ones(4), idx, np.zeros(4), 0xa4093822, 0x299f31d0)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # the third published vector through draw: step = its words 0 and 1 less bit 31 of word 1, which is set: half 1
    got = philox.draw((0x05a308d3 << 32) | 0x243f6a88, 1, np.array([0x13198a2e]), 0x03707344, seed)
    assert tuple(int(x[0]) for x in got) == KAT[2][2]


def test_u53():
    ones, zero = np.array([0xffffffff], dtype=np.uint64), np.array([0], dtype=np.uint64)
    assert philox.u53(ones, ones)[0] == 1.0 - 2.0 ** -53
    assert philox.u53(zero, zero)[0] == 0.0
    assert philox.u53(zero, np.array([0x7ff], dtype=np.uint64))[0] == 0.0           # the low 11 bits are dropped
    assert philox.u53(zero, np.array([0x800], dtype=np.uint64))[0] == 2.0 ** -53
    assert philox.u53(np.array([0x80000000], dtype=np.uint64), zero)[0] == 0.5
    r = philox.draw(11, 0, np.arange(20000), 0, 12345)
    u = philox.u53(r[0], r[1])
    assert u.dtype == np.float64 and u.min() >= 0.0 and u.max() < 1.0
    assert abs(u.mean() - 0.5) < 5.0 / np.sqrt(12.0 * len(u))                        # 5 sigma of a uniform's mean
