"""The gap-extend-frame core's four-column pass (pcabi_dp.h align_lane_shift4: the cross-mode
kernels' path for waves whose windows all have one length), compiled for the HOST with g++ and
driven by a reader over the tile layout's dwords. Against align_lane_shift on the same input and
against the oracle, all 8 fields of every pair. What the pass changes: column 0 is stored at phase
-1, so the rebases fall at pass boundaries (before the columns P k + 1, not P k); the codes come out
of a held dword by constant shifts; the columns left over after the last whole pass and the last
column read the next dword; the reader may not go past the tile's ceil(n / 4) + 2 dwords. So: every
bucket, two adapter lengths in each (one with padding rows), every window length from 1 to 70 (all
residues mod 4 around every period) and 150, periods 8, 16 and 32 wherever shift_range accepts them,
both ends of the bias range, the four schemes of tests/test_gpu_shift.py."""
import ctypes
import os
import random
import subprocess
import tempfile

import pytest

from tests import oracle_lib
from tests.test_dp_core_shift_cpu import _embed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEMES = [(3, -6, -5, -2), (1, -1, -3, -1), (2, -3, -5, -1), (3, -6, -2, -5)]
WIN_LENS = list(range(1, 71)) + [150]
PERIODS = (8, 16, 32)


@pytest.fixture(scope='module')
def model():
    out = os.path.join(tempfile.mkdtemp(prefix='pcabi_model_shift4_'), 'dp_model_shift4.so')
    subprocess.check_call(['g++', '-std=c++17', '-O2', '-shared', '-fPIC', '-o', out,
                           os.path.join(ROOT, 'tests', 'native', 'dp_model_shift4.cpp')])
    L = ctypes.CDLL(out)
    L.pcabi_model_shift4.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p] + \
        [ctypes.c_int] * 8 + [ctypes.c_void_p]
    return L


def _run(model, which, r, a, rpl, period, bias, sc):
    out = (ctypes.c_int * 8)()
    rc = model.pcabi_model_shift4(which, r.encode(), len(r), a.encode(), len(a), rpl, period, bias, *sc, out)
    return rc, list(out)


@pytest.mark.parametrize('k_sc', range(len(SCHEMES)))
def test_shift4_every_bucket_every_length(model, k_sc):
    sc = SCHEMES[k_sc]
    rng = random.Random(400 + k_sc)
    ran = {}
    for rpl in range(4, 33, 4):
        for L in (min(rpl, 31), max(1, rpl - 3) if rpl < 32 else 29):
            for n in WIN_LENS:
                al = rng.choice(['A', 'AT', 'ACGT', 'ACGT', 'ACGTN'])
                a = ''.join(rng.choice(al) for _ in range(L))
                r = _embed(rng, a, al, n)[:n] if rng.random() < 0.5 else ''.join(rng.choice(al) for _ in range(n))
                exp = None
                for period in PERIODS:
                    for bias in (0, 1):
                        rc4, got4 = _run(model, 1, r, a, rpl, period, bias, sc)
                        rc1, got1 = _run(model, 0, r, a, rpl, period, bias, sc)
                        assert rc4 == rc1 and rc4 in (0, -3), (sc, r, a, rpl, period, bias, rc4, rc1)
                        if rc4 == -3:
                            continue
                        exp = exp or oracle_lib.align(r, a, sc)
                        assert got4 == got1 == exp, (sc, r, a, rpl, period, bias)
                        ran[(rpl, period)] = ran.get((rpl, period), 0) + 1
    # every bucket ran at its own largest period (pcabi::shift_pmax) for the schemes whose frame fits
    # everywhere; the other two schemes' declines are shift_range's (tests/test_dp_core_shift_cpu.py)
    if k_sc < 2:
        for rpl in range(4, 33, 4):
            for period in PERIODS:
                want = period <= (32 if rpl <= 24 else 16 if rpl <= 28 else 8)
                assert (ran.get((rpl, period), 0) == 2 * 2 * len(WIN_LENS)) == want, (sc, rpl, period, ran)
    assert sum(ran.values()) > 2000


def test_shift4_longest_gap_runs(model):
    """Nothing matches: the H and V runs extend as far as the scores allow, across the rebases."""
    n_checked = 0
    for sc in SCHEMES:
        for rpl in range(4, 33, 4):
            L = min(rpl, 31)
            for n in (4, 5, 8, 9, 16, 17, 32, 33, 34, 35, 36, 65, 150):
                for a, r in (('C' * L, 'A' * n), ('A' * L, 'C' * n)):
                    for period in PERIODS:
                        rc4, got4 = _run(model, 1, r, a, rpl, period, 2, sc)
                        rc1, got1 = _run(model, 0, r, a, rpl, period, 2, sc)
                        assert rc4 == rc1 and rc4 in (0, -3)
                        if rc4 == 0:
                            assert got4 == got1 == oracle_lib.align(r, a, sc), (sc, rpl, n, period)
                            n_checked += 1
    assert n_checked > 800
