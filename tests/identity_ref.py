"""The reference's identity, independent of the product: alignment.cpp:82,90 compute
100.0 * matches / length, alignment.cpp:118-119 print it with "%f" (std::to_string) and
nanopore_read.py:497-498 parse the text back with float(). ref_pid6 is that round trip in plain
Python -- the expected value for everything under tests/ that compares identities. It imports
nothing from the package under test. TEST INFRASTRUCTURE ONLY."""
import numpy as np


def ref_pid6_scalar(m, l):
    """float('%f' % (100.0 * m / l)); NaN for l == 0 (the reference prints "-nan")."""
    return float('nan') if l == 0 else float('%f' % (100.0 * m / l))


def ref_pid6(m, l):
    """ref_pid6_scalar elementwise over (broadcast) integer arrays, as float64. The input is
    reduced to its unique (m, l) pairs, each formatted once."""
    m, l = np.broadcast_arrays(np.asarray(m, np.int64), np.asarray(l, np.int64))
    if m.size == 0:
        return np.zeros(m.shape, np.float64)
    key = ((m.ravel() + (1 << 31)).astype(np.uint64) << np.uint64(32)) | (l.ravel() + (1 << 31)).astype(np.uint64)
    uniq, inv = np.unique(key, return_inverse=True)
    um = ((uniq >> np.uint64(32)).astype(np.int64) - (1 << 31)).tolist()
    ul = ((uniq & np.uint64(0xFFFFFFFF)).astype(np.int64) - (1 << 31)).tolist()
    vals = np.array([ref_pid6_scalar(a, b) for a, b in zip(um, ul)], np.float64)
    return vals[inv.ravel()].reshape(m.shape)


# Lengths at which 100 * m / l * 1e6 lands on k + 0.5. 2^9 * 5^3 * 2^a (64000, 128000: every pair
# up to 2^17 that needs the exact product, tools/pid6_ties.c) and larger members of 2^9 * 5^b: the
# double product is a tie, the exact one is not. 512, 2560, 12800: exact ties, which round
# half-even.
TIE_LENGTHS_EVERY_M = (512, 2560, 12800, 64000, 128000)
TIE_LENGTHS_FIRST_M = (320000, 1600000, 8000000)
TIE_FIRST_M = 20001


def tie_grid():
    """(m, l) int32 arrays: every m of TIE_LENGTHS_EVERY_M, the first TIE_FIRST_M of the rest."""
    ms = [np.arange(l + 1) for l in TIE_LENGTHS_EVERY_M] + [np.arange(TIE_FIRST_M) for _ in TIE_LENGTHS_FIRST_M]
    ls = [np.full(len(a), l) for a, l in zip(ms, TIE_LENGTHS_EVERY_M + TIE_LENGTHS_FIRST_M)]
    return np.concatenate(ms).astype(np.int32), np.concatenate(ls).astype(np.int32)


def corrected_ties(l):
    """How many m in 0..l print a 6-decimal integer other than rint(d * 1e6) of the double
    product: the pairs a pid6 that never corrects a tie gets wrong. Reference side only."""
    n = 0
    for m in range(l + 1):
        d = 100.0 * m / l
        n += round(d * 1e6) != int(('%f' % d).replace('.', ''))
    return n
