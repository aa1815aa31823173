"""The gap-extend-frame core of the packed 36-64-row buckets (pcabi_dp.h LanePShift /
align_lane_pshift / pshift_range / pshift_bucket: the cross-mode kernels' inner columns), compiled
for the HOST with g++ and run against the oracle. Keys are pk::Lay keys kept relative to their
anti-diagonal, so a gap extend is the identity; the 2-bit tie field is Lay's own, and the stored
keys are rebased every P columns. What can go wrong is therefore: a shifted score leaving the 10-bit
field (pshift_range), a tie decided differently from Lay, the rebase, and the change back to Lay
keys before the last column -- so the cases are tie-heavy alphabets, every adapter length from 33 to
63 in every bucket that holds it (extra padding rows), window lengths around every allowed rebase
period (forced, so short windows rebase too), long gap runs, both ends of the allowed bias range, and
the reference's golden rows."""
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
PERIODS = (512, 256, 128, 64, 32, 16, 8, 4, 2)
ALPHABETS = ('A', 'AT', 'ACGT', 'ACGTN')


@pytest.fixture(scope='module')
def model():
    out = os.path.join(tempfile.mkdtemp(prefix='pcabi_model_pshift_'), 'dp_model_pshift.so')
    subprocess.check_call(['g++', '-std=c++17', '-O2', '-shared', '-fPIC', '-o', out,
                           os.path.join(ROOT, 'tests', 'native', 'dp_model_pshift.cpp')])
    L = ctypes.CDLL(out)
    L.pcabi_model_pshift_range.argtypes = [ctypes.c_int] * 7 + [ctypes.c_void_p] * 2
    L.pcabi_model_pshift_bucket.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 6 + [ctypes.c_void_p] * 2
    L.pcabi_model_align_pshift.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p] + [ctypes.c_int] * 8 + \
        [ctypes.c_void_p]
    return L


def _range(model, L, rpl, sc, period):
    lo, hi = ctypes.c_int(0), ctypes.c_int(0)
    if not model.pcabi_model_pshift_range(L, rpl, period, *sc, ctypes.byref(lo), ctypes.byref(hi)):
        return None
    return lo.value, hi.value


def _ok(model, L, rpl, sc):
    lens = (ctypes.c_int32 * 1)(L)
    P, B = ctypes.c_int(0), ctypes.c_int(0)
    if not model.pcabi_model_pshift_bucket(lens, 1, rpl, *sc, ctypes.byref(P), ctypes.byref(B)):
        return None
    return P.value, B.value


def _pshift(model, r, a, rpl, sc, period=0, which=2):
    out = (ctypes.c_int * 8)()
    rc = model.pcabi_model_align_pshift(r.encode(), len(r), a.encode(), len(a), rpl, period, which, *sc, out)
    return rc, list(out)


def _buckets(L):
    return range(max(36, (L + 3) & ~3), 65, 4)


def _embed(rng, a, al, n):
    """A window of about n columns holding a mutated copy of the adapter with up to three long
    insertions / deletions."""
    b = [c if rng.random() > 0.1 else rng.choice(al) for c in a]
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
    """No hidden fallback: the default scheme runs the frame for 33-63 bp in every bucket that holds
    the adapter. The frame spans at most 63 x 3 + 2 x (64 + P) + a gap pair, about 330 + 2 P, of the
    field's 1023 values: P = 256 fits (842), 512 does not (1354)."""
    periods = {}
    for L in range(33, 64):
        for rpl in _buckets(L):
            pb = _ok(model, L, rpl, DEFAULT)
            assert pb is not None, (L, rpl)
            assert pb[0] == 256, (L, rpl, pb)
            periods[(L, rpl)] = pb[0]
    print('default scheme, accepted periods:', sorted(set(periods.values())), 'over', len(periods), '(L, bucket) pairs')


@pytest.mark.parametrize('k_sc', range(len(SCHEMES)))
def test_pshift_core_every_length_every_bucket(model, k_sc):
    """Every L in 33-63 in every bucket that holds it. At the period and bias the bucket would pick:
    the four alphabets x window lengths 1, 2, 150 and 223. At EVERY period pshift_range allows
    (forced, so the rebases fall inside short windows): window lengths P - 1, P, P + 1 and 2 P. Random
    windows and windows embedding a mutated adapter with long insertions / deletions; all 8 fields
    against the oracle. Every case counted as run was accepted by the range check (rc == 0)."""
    sc = SCHEMES[k_sc]
    rng = random.Random(300 + k_sc)
    ran = declined = cases = 0
    accepted = {}
    for L in range(33, 64):
        for rpl in _buckets(L):
            pb = _ok(model, L, rpl, sc)
            if pb is None:
                declined += 1
                assert _pshift(model, 'A', 'A' * L, rpl, sc)[0] == -3
                assert all(_range(model, L, rpl, sc, p) is None for p in PERIODS)
                continue
            ran += 1
            allowed = [p for p in PERIODS if _range(model, L, rpl, sc, p) is not None]
            assert allowed and allowed[0] == pb[0], (sc, L, rpl, pb, allowed)
            accepted[pb[0]] = accepted.get(pb[0], 0) + 1
            for al in ALPHABETS:
                a = ''.join(rng.choice(al) for _ in range(L))
                for n in (1, 2, 150, 223):
                    r = _embed(rng, a, al, n) if rng.random() < 0.5 else ''.join(rng.choice(al) for _ in range(n))
                    rc, res = _pshift(model, r, a, rpl, sc)
                    assert rc == 0 and res == oracle_lib.align(r, a, sc), (sc, r, a, rpl, pb)
                    cases += 1
            for p in allowed:
                al = rng.choice(ALPHABETS)
                a = ''.join(rng.choice(al) for _ in range(L))
                for n in (p - 1, p, p + 1, 2 * p):
                    r = _embed(rng, a, al, n) if rng.random() < 0.5 else ''.join(rng.choice(al) for _ in range(n))
                    rc, res = _pshift(model, r, a, rpl, sc, period=p)
                    assert rc == 0 and res == oracle_lib.align(r, a, sc), (sc, r, a, rpl, p)
                    cases += 1
    print('scheme', sc, 'ran', ran, 'declined', declined, 'cases', cases, 'accepted periods', sorted(accepted.items()))
    assert ran + declined == sum(len(_buckets(L)) for L in range(33, 64))
    if sc == DEFAULT:
        assert declined == 0
    assert ran > 0 and cases >= ran * 20


def _packed_fits(L, sc):
    """pk::Lay's documented range conditions (packed_ok, narrow layout)."""
    ma, mi, go, ge = sc
    if not (go < 0 and ge < 0) or L > 63:
        return False
    top = max(ma, mi)
    if L + (top * L // min(-go, -ge) if top > 0 else 0) > 255:
        return False
    smin = go + (L - 1) * ge if go != ge else L * ge
    neg = go - ge - 1
    lo = min(smin + min(go + ge, mi, ma), neg + ge, neg, go)
    hi = max(L * top, 0, top)
    return lo >= -512 and hi <= 511


def _fits(L, rpl, sc, P):
    """The documented range conditions, independently of the C++ predicate: Lay's own, affine gaps,
    and the shifted scores of every slot s at phases -1 .. P - 1 within 1023 values (-511 .. 511,
    -512 is the sentinel)."""
    ma, mi, go, ge = sc
    if go == ge or not _packed_fits(L, sc) or not 2 <= P <= 512:
        return False
    e, bs, msub = -ge, max(ma, mi, 0), min(ma, mi, 0)
    lo0, hi0 = go, go + e * P
    for s in range(1, rpl + 1):
        i = s - (rpl - L)
        slo, shi = (go + (i - 1) * ge, i * bs) if i >= 1 else (0, 0)
        ulo, uhi = (go + (i - 2) * ge, (i - 1) * bs) if i >= 2 else (0, 0)
        lo0 = min(lo0, min(slo + go, ulo + msub) + e * (s - 1))
        hi0 = max(hi0, max(shi + max(go + e, 0), uhi + bs) + e * (s + P - 1))
    return hi0 - lo0 <= 1022


def test_pshift_range_matches_documented_bounds(model):
    """pshift_range accepts exactly the (L, bucket, scheme, period) whose documented bounds fit, and
    the bucket's period is the largest such power of two."""
    for sc in SCHEMES + [(3, -6, -2, -2), (2, 20, -5, -2), (0, 0, -1, -2), (4, -4, -12, -3), (8, -8, -9, -8),
                         (3, -6, 0, -2)]:
        for L in range(33, 64):
            for rpl in _buckets(L):
                ps = [p for p in PERIODS if _fits(L, rpl, sc, p)]
                assert ps == [p for p in PERIODS if _range(model, L, rpl, sc, p) is not None], (sc, L, rpl)
                pb = _ok(model, L, rpl, sc)
                assert (pb[0] if pb else None) == (ps[0] if ps else None), (sc, L, rpl, pb, ps)
    assert _ok(model, 40, 40, (3, -6, -2, -2)) is None          # linear gaps keep Lay
    assert _ok(model, 40, 40, (3, -6, 0, -2)) is None           # free gap open: not packed at all
    assert _ok(model, 30, 32, DEFAULT) is None                  # the 4-32-row buckets are not this frame's


def test_pshift_bucket_intersects_ranges(model):
    """A bucket of several lengths takes one period and one bias inside every adapter's range."""
    for sc in SCHEMES:
        for rpl in range(36, 65, 4):
            lens = [L for L in range(rpl - 3, rpl + 1) if 33 <= L <= 63]
            arr = (ctypes.c_int32 * len(lens))(*lens)
            P, B = ctypes.c_int(0), ctypes.c_int(0)
            if not model.pcabi_model_pshift_bucket(arr, len(lens), rpl, *sc, ctypes.byref(P), ctypes.byref(B)):
                continue
            for L in lens:
                lo, hi = _range(model, L, rpl, sc, P.value)
                assert lo <= B.value <= hi, (sc, rpl, L, P.value, B.value)


def test_pshift_core_periods_and_bias_range(model):
    """Every period the predicate allows (not only the largest) and both ends of the bias range:
    at the lowest bias the largest shifted score sits at the top of the field, at the highest the
    smallest sits one above the sentinel."""
    rng = random.Random(11)
    n_checked = 0
    for k in range(900):
        sc = SCHEMES[k % len(SCHEMES)]
        al = rng.choice(ALPHABETS)
        L = rng.randint(33, 63)
        rpl = rng.choice(list(_buckets(L)))
        a = ''.join(rng.choice(al) for _ in range(L))
        n = rng.choice([1, 2, 3, 7, 8, 9, 16, 17, 33, 64, 65, 150, 223, 260, 600])
        r = _embed(rng, a, al, n) if k % 2 else ''.join(rng.choice(al) for _ in range(n))
        exp = None
        for period in PERIODS:
            for which in (0, 1):
                rc, res = _pshift(model, r, a, rpl, sc, period, which)
                if rc == -3:
                    continue
                exp = exp or oracle_lib.align(r, a, sc)
                assert rc == 0 and res == exp, (sc, r, a, rpl, period, which)
                n_checked += 1
    assert n_checked > 5000


def test_pshift_core_longest_gap_runs(model):
    """All-mismatch poly-A / poly-C pairs: nothing matches, so the H and V runs extend as far as the
    scores allow, across many rebases (period 8 where it is allowed, else the bucket's own)."""
    n_checked = 0
    for sc in SCHEMES:
        for L in range(33, 64):
            for rpl in _buckets(L):
                pb = _ok(model, L, rpl, sc)
                if pb is None:
                    continue
                for period in (0, 8):
                    for n in (1, 2, 9, 150, 223, 2 * pb[0]):
                        for a, r in (('C' * L, 'A' * n), ('A' * L, 'C' * n)):
                            rc, res = _pshift(model, r, a, rpl, sc, period)
                            assert rc == 0 and res == oracle_lib.align(r, a, sc), (sc, L, rpl, n, period)
                            n_checked += 1
    assert n_checked > 8000


def test_pshift_core_golden_rows(model):
    """The reference's golden alignments with adapters of 33 to 63 bp, at the bucket's own period and at a
    forced period of 8 (rebases inside every window)."""
    n_gold = 0
    for sc, r, a, exp in golden_lib.g1_rows():
        if not r or not a or not 33 <= len(a) <= 63:
            continue
        for period in (0, 8):
            rc, res = _pshift(model, r, a, max(36, (len(a) + 3) & ~3), sc, period)
            if rc == -3:
                continue
            assert rc == 0
            rs, re_, as_, ae, score, m, l1, l2 = res
            p1 = '-nan' if l1 == 0 else '%f' % (100.0 * m / l1)
            p2 = '-nan' if l2 == 0 else '%f' % (100.0 * m / l2)
            assert '%d,%d,%d,%d,%d,%s,%s' % (rs, re_, as_, ae, score, p1, p2) == exp, (sc, r, a, period)
            n_gold += 1
    print('golden rows checked:', n_gold)
    assert n_gold > 0
