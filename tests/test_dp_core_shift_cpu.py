"""The gap-extend-frame core of the run-tagged buckets (pcabi_dp.h pk::LayS / LaneShift /
align_lane_shift: the cross-mode kernels' inner columns), compiled for the HOST with g++ and run
against the oracle. Keys are kept relative to their anti-diagonal, so a gap extend is the identity;
tags fall with the column (H) and the row (V) instead of counting extends, and the stored keys are
rebased every P columns. What can go wrong is therefore: a shifted score leaving the 8-bit field
(shift_ok / shift_range), a tie decided differently from pk::LayT, the rebase, and the change back
to LayT keys before the last column -- so the cases are tie-heavy alphabets, every adapter length
in every bucket that holds it (extra padding rows), window lengths around the rebase period, long
gap runs, both ends of the allowed bias range, and the reference's golden rows."""
import ctypes
import os
import random
import subprocess
import tempfile

import pytest

from tests import golden_lib, oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEMES = [(3, -6, -5, -2), (1, -1, -3, -1), (3, -6, -2, -5), (5, -4, -8, -6), (2, -3, -5, -1), (2, -3, -2, -1)]
DEFAULT = SCHEMES[0]


@pytest.fixture(scope='module')
def model():
    out = os.path.join(tempfile.mkdtemp(prefix='pcabi_model_shift_'), 'dp_model_shift.so')
    subprocess.check_call(['g++', '-std=c++17', '-O2', '-shared', '-fPIC', '-o', out,
                           os.path.join(ROOT, 'tests', 'native', 'dp_model_shift.cpp')])
    L = ctypes.CDLL(out)
    L.pcabi_model_shift_ok.argtypes = [ctypes.c_int] * 6 + [ctypes.c_void_p] * 2
    L.pcabi_model_align_shift.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p] + [ctypes.c_int] * 7 + \
        [ctypes.c_void_p]
    L.pcabi_model_align_shift_bias.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p] + [ctypes.c_int] * 8 + \
        [ctypes.c_void_p]
    return L


def _ok(model, L, rpl, sc):
    P, B = ctypes.c_int(0), ctypes.c_int(0)
    if not model.pcabi_model_shift_ok(L, rpl, *sc, ctypes.byref(P), ctypes.byref(B)):
        return None
    return P.value, B.value


def _shift(model, r, a, rpl, sc, period=0):
    out = (ctypes.c_int * 8)()
    rc = model.pcabi_model_align_shift(r.encode(), len(r), a.encode(), len(a), rpl, period, *sc, out)
    return rc, list(out)


def _bias(model, r, a, rpl, sc, period, which):
    out = (ctypes.c_int * 8)()
    rc = model.pcabi_model_align_shift_bias(r.encode(), len(r), a.encode(), len(a), rpl, period, which, *sc, out)
    return rc, list(out)


def _buckets(L):
    return range((L + 3) & ~3, 33, 4)


def _embed(rng, a, al, n):
    """A window of about n columns holding the adapter with up to three long insertions / deletions."""
    b = list(a)
    for _ in range(rng.randint(0, 3)):
        p = rng.randint(0, len(b))
        if rng.random() < 0.5:
            b[p:p] = [rng.choice(al) for _ in range(rng.randint(1, 30))]
        else:
            del b[p:p + rng.randint(1, 8)]
    lead = max(0, n - len(b))
    k = rng.randint(0, lead)
    r = ''.join(rng.choice(al) for _ in range(k)) + ''.join(b) + ''.join(rng.choice(al) for _ in range(lead - k))
    return r or 'A'


def test_default_scheme_accepted_everywhere(model):
    """The default scheme runs the frame for 1-31 bp in every bucket that holds the adapter, with a
    period that keeps the rebase rare (32 columns up to 24 rows, 16 at 28, 8 at 32)."""
    for L in range(1, 32):
        for rpl in _buckets(L):
            pb = _ok(model, L, rpl, DEFAULT)
            assert pb is not None, (L, rpl)
            assert pb[0] == (32 if rpl <= 24 else 16 if rpl <= 28 else 8), (L, rpl, pb)


def test_declined_schemes(model):
    """shift_ok declines what cannot fit: linear gaps, gaps that cost nothing, a score range wider
    than the field at any period, and H runs longer than the tag budget."""
    assert _ok(model, 20, 20, (3, -6, -2, -2)) is None          # linear
    assert _ok(model, 20, 20, (3, -6, 0, -2)) is None           # free gap open
    assert _ok(model, 24, 24, (5, -4, -8, -6)) is None          # 24 x 5 + 6 x (24 + P) > 254
    assert _ok(model, 31, 32, (2, -3, -5, -1)) is None          # Hmax = 98 > KVB - 2
    assert _shift(model, 'ACGT', 'A' * 24, 24, (5, -4, -8, -6))[0] == -3


@pytest.mark.parametrize('k_sc', range(len(SCHEMES)))
def test_shift_core_every_length_every_bucket(model, k_sc):
    """Every L in 1-31 in every bucket that holds it, the four alphabets, window lengths 1, 2, P - 1,
    P, P + 1, 2 P, 150 and 400 (random windows and windows embedding the adapter with long
    insertions / deletions): all 8 fields against the oracle. Per scheme, the number of (L, bucket)
    pairs that ran and that were declined is fixed by shift_ok's bounds."""
    sc = SCHEMES[k_sc]
    rng = random.Random(100 + k_sc)
    ran = declined = cases = 0
    for L in range(1, 32):
        for rpl in _buckets(L):
            pb = _ok(model, L, rpl, sc)
            if pb is None:
                declined += 1
                assert _shift(model, 'A', 'A' * L, rpl, sc)[0] == -3
                continue
            ran += 1
            P = pb[0]
            for al in ('A', 'AT', 'ACGT', 'ACGTN'):
                a = ''.join(rng.choice(al) for _ in range(L))
                for n in (1, 2, P - 1, P, P + 1, 2 * P, 150, 400):
                    r = _embed(rng, a, al, n) if rng.random() < 0.5 else ''.join(rng.choice(al) for _ in range(n))
                    rc, res = _shift(model, r, a, rpl, sc)
                    assert rc == 0 and res == oracle_lib.align(r, a, sc), (sc, r, a, rpl, pb)
                    cases += 1
    # 143 (L, bucket) pairs in all. The split is the bounds' own (_fits, worked out in Python from
    # the documented ranges): the default scheme and (1, -1, -3, -1) fit everywhere; |ge| = 5 or 6
    # widens the frame by |ge| per row and column until 8 bits no longer hold it; ge = -1 makes the
    # H runs (Smax - Smin + 1 columns) outgrow the tags of the 24 to 32-row buckets.
    expect = {(3, -6, -5, -2): (143, 0), (1, -1, -3, -1): (143, 0), (3, -6, -2, -5): (132, 11),
              (5, -4, -8, -6): (99, 44), (2, -3, -5, -1): (133, 10), (2, -3, -2, -1): (136, 7)}[sc]
    assert (ran, declined) == expect, (sc, ran, declined)
    assert cases == ran * 32


def _fits(L, rpl, sc, P):
    """The documented range conditions, independently of the C++ predicate: LayT's own (span, 8-bit
    scores, H runs below the V-open tag), the frame's tag budget, and the shifted scores of every
    slot s at phases -1 .. P - 1 within 254 values (-127 .. 127, -128 is the sentinel)."""
    ma, mi, go, ge = sc
    if not (go < 0 and ge < 0 and go != ge):
        return False
    e, top, bs, msub = -ge, max(ma, mi), max(ma, mi, 0), min(ma, mi, 0)
    if L + (top * L // min(-go, e) if top > 0 else 0) >= 128:
        return False
    smin = go + (L - 1) * ge
    neg = go - ge - 1
    lo = min(smin + min(go + ge, mi, ma), neg + ge, neg, go)
    hi = max(L * top, 0, top)
    if lo < -128 or hi > 127 or (hi - smin) // e + 1 >= 127 - rpl:
        return False
    pmax = 32 if rpl <= 24 else 16 if rpl <= 28 else 8
    if not 2 <= P <= pmax or (L * bs - smin) // e + 1 + 2 > 128 - pmax - rpl:
        return False
    lo0, hi0 = go, go + e * P
    for s in range(1, rpl + 1):
        i = s - (rpl - L)
        slo, shi = (go + (i - 1) * ge, i * bs) if i >= 1 else (0, 0)
        ulo, uhi = (go + (i - 2) * ge, (i - 1) * bs) if i >= 2 else (0, 0)
        lo0 = min(lo0, min(slo + go, ulo + msub) + e * (s - 1))
        hi0 = max(hi0, max(shi + max(go + e, 0), uhi + bs) + e * (s + P - 1))
    return hi0 - lo0 <= 254


def test_shift_ok_matches_documented_bounds(model):
    """shift_ok accepts exactly the (L, bucket, scheme) triples whose documented bounds fit at some
    period, and returns the largest such power of two."""
    for sc in SCHEMES + [(3, -6, -2, -2), (2, 20, -5, -2), (0, 0, -1, -2), (4, -4, -12, -3)]:
        for L in range(1, 32):
            for rpl in _buckets(L):
                ps = [p for p in (32, 16, 8, 4, 2) if _fits(L, rpl, sc, p)]
                pb = _ok(model, L, rpl, sc)
                assert (pb[0] if pb else None) == (ps[0] if ps else None), (sc, L, rpl, pb, ps)


def test_shift_core_periods_and_bias_range(model):
    """Every period the predicate allows (not only the largest) and both ends of the bias range:
    at the lowest bias the largest shifted score sits at the top of the field, at the highest the
    smallest sits one above the sentinel."""
    rng = random.Random(7)
    n_checked = 0
    for k in range(1500):
        sc = SCHEMES[k % len(SCHEMES)]
        al = rng.choice(['A', 'AT', 'ACGT', 'ACGTN'])
        L = rng.randint(1, 31)
        rpl = rng.choice(list(_buckets(L)))
        a = ''.join(rng.choice(al) for _ in range(L))
        n = rng.choice([1, 2, 3, 7, 8, 9, 16, 17, 33, 64, 150, 260])
        r = _embed(rng, a, al, n) if k % 2 else ''.join(rng.choice(al) for _ in range(n))
        exp = None
        for period in (2, 4, 8, 16, 32):
            for which in (0, 1):
                rc, res = _bias(model, r, a, rpl, sc, period, which)
                if rc == -3:
                    continue
                exp = exp or oracle_lib.align(r, a, sc)
                assert rc == 0 and res == exp, (sc, r, a, rpl, period, which)
                n_checked += 1
    assert n_checked > 5000


def test_shift_core_longest_gap_runs(model):
    """All-mismatch poly-A / poly-C pairs: nothing matches, so the H and V runs extend as far as
    the scores allow (the tag budget's worst case), across many rebases."""
    n_checked = 0
    for sc in SCHEMES:
        for L in range(1, 32):
            for rpl in _buckets(L):
                pb = _ok(model, L, rpl, sc)
                if pb is None:
                    continue
                P = pb[0]
                for n in (1, 2, P - 1, P, P + 1, 2 * P, 150, 400):
                    for a, r in (('C' * L, 'A' * n), ('A' * L, 'C' * n)):
                        rc, res = _shift(model, r, a, rpl, sc)
                        assert rc == 0 and res == oracle_lib.align(r, a, sc), (sc, L, rpl, n)
                        n_checked += 1
    assert n_checked > 8000


def test_shift_core_golden_rows(model):
    """The reference's golden alignments with adapters up to 31 bp."""
    n_gold = 0
    for sc, r, a, exp in golden_lib.g1_rows():
        if not r or not a or len(a) > 31:
            continue
        rc, res = _shift(model, r, a, (len(a) + 3) & ~3, sc)
        if rc == -3:
            continue
        assert rc == 0
        rs, re_, as_, ae, score, m, l1, l2 = res
        p1 = '-nan' if l1 == 0 else '%f' % (100.0 * m / l1)
        p2 = '-nan' if l2 == 0 else '%f' % (100.0 * m / l2)
        assert '%d,%d,%d,%d,%d,%s,%s' % (rs, re_, as_, ae, score, p1, p2) == exp, (sc, r, a)
        n_gold += 1
    assert n_gold > 1000
