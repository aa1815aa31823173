"""The gap-extend-frame cores' own last column (pcabi_dp.h LaneShift::last_column and
LanePShift::last_column, the end of align_lane_shift, align_lane_shift4 and align_lane_pshift),
compiled for the HOST with g++. The column runs the frame's cell and offers one candidate per row,
max(H, S with the tie field cleared), to the scout's key; no V candidate, no trailing-run
bookkeeping, no H candidate of its own at (L, n). Checked two ways on every input: all 8 fields
against the oracle, and all 8 plus diag_en against align_lane_packed on the same layout (LayT for 4
to 32 rows, Lay for 36 to 64), which keeps LanePacked's last column with the full bookkeeping.

Every bucket from 4 to 64 rows; two adapter lengths per bucket, the longest and the shortest of the
bucket's own four lengths that the range function accepts at some period (so one has padding rows
wherever two are accepted); window lengths 1-12, then P - 1, P, P + 1 around every period, and 150;
every power-of-two period -- what shift_ok and pshift_bucket choose from -- that shift_range /
pshift_range accept, at both ends of the bias range; align_lane_shift4 at the periods that are
multiples of 4; the six schemes of tests/test_dp_core_pshift_cpu.py.

The windows aim at the last column: a mutated adapter prefix a[:k] ending exactly at the window's
end; the same followed by 1-3 bases that differ from the adapter's next ones; the whole adapter
ending at column n; the whole adapter followed by a random tail (the scout's winner stands);
windows with no hit.

Winner categories, from the oracle's own fields. With re == n - 1 the end cell lies in the last
column, and its row bi follows from the two alignment lengths: the adapter's bases after the path
are counted in l2 and not in l1, so bi = L - (l2 - l1) + (as if rs == 0 else 0) (DESIGN.md section 3:
l2 - l1 = h - a0 + L - bi, h - a0 = as when the read starts the alignment). Below row L the last
path column is a diagonal when ae == bi - 1 and a read base over an adapter gap -- the H winner --
when ae == bi. The core's diag_en must say the same, which checks the derivation on every pair.
    below_d : re == n - 1, bi < L, ae == bi - 1
    below_h : re == n - 1, bi < L, ae == bi
    corner  : re == n - 1, bi == L                  (the end cell is (L, n))
    row_l   : re < n - 1, l1 > 0                    (row L before column n: ae == L - 1)
    none    : l1 == 0                               (no hit: the (L, 0) seed stands, score 0)
An H winner at (i, n) scores S(i, n - k) + go + (k - 1) ge and must beat the k diagonal steps from
the same cell, which end in the last column or in row L and score at least S(i, n - k) + k mi: when
a mismatch costs no more than either gap step (mi >= go and mi >= ge) there is none, so the minimum
for below_h is 0 under (1, -1, -3, -1) and (5, -4, -8, -6), and the test asserts that none occurs."""
import ctypes
import os
import random
import subprocess
import tempfile

import pytest

from tests import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEMES = [(3, -6, -5, -2), (1, -1, -3, -1), (3, -6, -2, -5), (5, -4, -8, -6), (2, -3, -5, -1), (2, -3, -2, -1)]
PERIODS_SMALL = (2, 4, 8, 16, 32)
PERIODS_LARGE = (2, 4, 8, 16, 32, 64, 128, 256, 512)
BUCKETS = list(range(4, 65, 4))
# buckets whose own lengths shift_range declines at every period (the H-run or score bounds of LayS)
NO_FRAME = {SCHEMES[0]: (), SCHEMES[1]: (), SCHEMES[2]: (28, 32), SCHEMES[3]: (24, 28, 32), SCHEMES[4]: (32,),
            SCHEMES[5]: (32,)}
# pairs per category and scheme that the generators must reach (the oracle alone decides)
MINIMUM = {'below_d': 150, 'below_h': 40, 'corner': 150, 'row_l': 150, 'none': 50}


def _win_lens(periods):
    ns = set(range(1, 13)) | {150}
    for p in periods:
        ns |= {p - 1, p, p + 1}
    return sorted(ns)


@pytest.fixture(scope='module')
def model():
    out = os.path.join(tempfile.mkdtemp(prefix='pcabi_model_lastcol_'), 'dp_model_lastcol.so')
    subprocess.check_call(['g++', '-std=c++17', '-O2', '-shared', '-fPIC', '-o', out,
                           os.path.join(ROOT, 'tests', 'native', 'dp_model_lastcol.cpp')])
    L = ctypes.CDLL(out)
    L.pcabi_model_lastcol.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p] + [ctypes.c_int] * 6 + \
        [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 3
    L.pcabi_model_lastcol_periods.argtypes = [ctypes.c_int] * 6 + [ctypes.c_void_p, ctypes.c_int]
    return L


def _periods(rpl):
    return PERIODS_SMALL if rpl <= 32 else PERIODS_LARGE


def _accepted(model, L, rpl, sc):
    ps = _periods(rpl)
    arr = (ctypes.c_int * len(ps))(*ps)
    return model.pcabi_model_lastcol_periods(L, rpl, *sc, arr, len(ps))


def _bucket_lengths(model, rpl, sc):
    """The longest and the shortest of the bucket's own lengths that some period accepts."""
    own = [L for L in range(max(1, rpl - 3), rpl + 1) if L <= (31 if rpl <= 32 else 63)]
    ok = [L for L in own if _accepted(model, L, rpl, sc)]
    return sorted({ok[-1], ok[0]}, reverse=True) if ok else []


def _mut(rng, s, al, rate):
    out = []
    for c in s:
        x = rng.random()
        if x < rate:
            out.append(rng.choice(al))
        elif x < rate * 1.3:
            continue
        elif x < rate * 1.6:
            out.append(c + rng.choice(al))
        else:
            out.append(c)
    return ''.join(out)


def _rand(rng, al, n):
    return ''.join(rng.choice(al) for _ in range(n))


def _foreign(rng, a, k, f):
    """f bases after a[:k], each different from the adapter's base at that place."""
    return ''.join(rng.choice([c for c in 'ACGT' if k + t >= len(a) or c != a[k + t]]) for t in range(f))


def windows(rng, a, n):
    """The five windows of n columns for adapter a (module docstring), lead filled from an alphabet
    that may lack the adapter's letters."""
    L = len(a)
    lead_al = rng.choice(['ACGT', 'ACGT', 'AT', 'ACGTN'])
    rate = rng.choice([0.0, 0.0, 0.06, 0.15])

    def fit(tail):
        tail = tail[-n:]
        return _rand(rng, lead_al, n - len(tail)) + tail

    k = rng.randint(max(1, min(L - 1, 3)), max(1, L - 1))
    f = rng.randint(1, 3)
    k2 = rng.randint(max(1, min(L - 1, 4)), max(1, L - 1))
    miss = [c for c in 'ACGT' if c not in a] or ['N']
    return [fit(_mut(rng, a[:k], 'ACGT', rate)),
            fit(_mut(rng, a[:k2], 'ACGT', rate / 2) + _foreign(rng, a, k2, f)),
            fit(_mut(rng, a, 'ACGT', rate)),
            fit(_mut(rng, a, 'ACGT', rate) + _rand(rng, miss, f + 2)),
            _rand(rng, miss, n) if rng.random() < 0.5 else _rand(rng, lead_al, n)]


def category(exp, n, L):
    rs, re_, as_, ae, score, m, l1, l2 = exp
    if l1 == 0:
        assert score == 0 and m == 0, exp      # the (L, 0) seed stands: no path
        return 'none'
    if re_ < n - 1:
        assert ae == L - 1, exp
        return 'row_l'
    bi = L - (l2 - l1) + (as_ if rs == 0 else 0)
    if bi == L:
        assert ae == L - 1, exp
        return 'corner'
    assert 1 <= bi < L and ae in (bi - 1, bi), (exp, bi)
    return 'below_h' if ae == bi else 'below_d'


@pytest.mark.parametrize('k_sc', range(len(SCHEMES)))
def test_last_column_every_bucket(model, k_sc):
    sc = SCHEMES[k_sc]
    ma, mi, go, ge = sc
    rng = random.Random(1000 + k_sc)
    cats = dict.fromkeys(MINIMUM, 0)
    ran = {}
    out, bad, mask = (ctypes.c_int * 9)(), (ctypes.c_int * 9)(), ctypes.c_int(0)
    for rpl in BUCKETS:
        ps = _periods(rpl)
        arr = (ctypes.c_int * len(ps))(*ps)
        lens = _bucket_lengths(model, rpl, sc)
        for L in lens:
            want = _accepted(model, L, rpl, sc)
            for n in _win_lens(ps):
                a = _rand(rng, rng.choice(['ACGT', 'ACGT', 'ACG', 'AT']), L)
                for r in windows(rng, a, n):
                    assert len(r) == n
                    rc = model.pcabi_model_lastcol(r.encode(), n, a.encode(), L, rpl, *sc, arr, len(ps), out, bad,
                                                   ctypes.byref(mask))
                    assert rc == 0, (sc, r, a, rpl, rc, list(out), list(bad))
                    assert mask.value == want != 0, (sc, L, rpl, mask.value, want)
                    exp = oracle_lib.align(r, a, sc)
                    assert list(out)[:8] == exp, (sc, r, a, rpl)
                    c = category(exp, n, L)
                    if c in ('below_d', 'below_h'):
                        assert out[8] == (1 if c == 'below_d' else 0), (sc, r, a, rpl, exp, out[8])
                    cats[c] += 1
                    ran[rpl] = ran.get(rpl, 0) + bin(mask.value).count('1')
    print('scheme', sc, 'categories', cats, 'period runs per bucket', sorted(ran.items()))
    # every (bucket, scheme) ran at least one period, but for the buckets in which shift_range declines
    # all four lengths at every period: they keep LayT under that scheme and never reach this column
    assert sorted(ran) == [rpl for rpl in BUCKETS if rpl not in NO_FRAME[sc]], (sc, sorted(ran))
    for c, least in MINIMUM.items():
        if c == 'below_h' and mi >= go and mi >= ge:
            assert cats[c] == 0, (sc, cats)
        else:
            assert cats[c] >= least, (sc, c, cats)
