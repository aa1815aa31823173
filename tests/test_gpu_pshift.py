"""The packed 36-64-row buckets' gap-extend frame on the GPU (pcabi_dp.h LanePShift, k_align<..,
PSHIFT> and class 1 of k_align_group): cross-mode launches whose adapters pass pcabi::pshift_bucket
keep their pk::Lay keys relative to the anti-diagonal and rebase them every P columns. Every field of
every (window, adapter) pair against the oracle, through pcabi_align_cross_dev (one launch per bucket;
PCABI_SPLIT=0 keeps the small launches off the row-split core, which stays on Lay) and through
pcabi_align_cross_multi_dev (grouped launches) over a start, an end and a ragged region of 300
windows each (two tiles, the second ragged). The first wave of every region holds 64 windows of 150
columns, the second a zero-length window; the other lengths run from 1 to 600 columns. The start and
end tables fill the buckets 36, 44, 52, 60 and 40, 48, 56, 64 (several adapters with padding rows);
the ragged table's eight buckets are merged to four by the engine, which adds up to seven padding
rows. The schemes: the default (P = 256: the 257-, 300- and 600-column windows rebase),
(1, -1, -3, -1) (P = 512: the 600-column windows), (5, -4, -8, -6) (|ge| = 6: P = 32 or 64) and
(8, -8, -4, -8), whose 62 and 63 bp adapters pshift_range declines while packed_ok accepts them -- so
the 64-row unit stays on Lay next to framed units in the same grouped launch. The host model
(tests/native/dp_model_pshift.cpp) gives each bucket's period, and the test asserts that windows
longer than it exist, so at least one rebase runs on the device."""
import ctypes
import os
import random
import subprocess
import tempfile

import numpy as np
import pytest

from tests import oracle_lib
from tests.test_gpu_parity import _mutate, _rand_seq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEMES = [(3, -6, -5, -2), (1, -1, -3, -1), (5, -4, -8, -6), (8, -8, -4, -8)]
DECLINING = (8, -8, -4, -8)
TABLE_LENS = [[36, 42, 44, 49, 52, 60], [37, 40, 46, 48, 53, 56, 62, 63], [33, 38, 41, 45, 50, 55, 59, 61]]
WIN_LENS = [1, 2, 7, 31, 32, 33, 63, 64, 65, 129, 150, 223, 257, 300, 600]
N_WIN = 300   # two tiles of 256, the second ragged
ZERO_AT = 100  # in the second wave


@pytest.fixture(scope='module')
def model():
    out = os.path.join(tempfile.mkdtemp(prefix='pcabi_model_pshift_'), 'dp_model_pshift.so')
    subprocess.check_call(['g++', '-std=c++17', '-O2', '-shared', '-fPIC', '-o', out,
                           os.path.join(ROOT, 'tests', 'native', 'dp_model_pshift.cpp')])
    L = ctypes.CDLL(out)
    L.pcabi_model_pshift_bucket.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 6 + [ctypes.c_void_p] * 2
    return L


def _bucket_period(model, lens, rpl, sc):
    arr = (ctypes.c_int32 * len(lens))(*lens)
    P, B = ctypes.c_int(0), ctypes.c_int(0)
    if not model.pcabi_model_pshift_bucket(arr, len(lens), rpl, *sc, ctypes.byref(P), ctypes.byref(B)):
        return None
    return P.value


def _cases(seed):
    rng = random.Random(seed)
    tables = [[_rand_seq(rng, L, rng.choice(['ACGT', 'ACGT', 'AT'])) for L in lens] for lens in TABLE_LENS]
    wins = []
    for adps in tables:   # start, end, ragged: three regions with windows of their own
        ws = []
        for k in range(N_WIN):
            n = 150 if k < 64 else (0 if k == ZERO_AT else rng.choice(WIN_LENS))
            r = _rand_seq(rng, n, rng.choice(['ACGT', 'ACGT', 'AT', 'ACGTN']))
            if n >= 63 and k % 2:
                a = _mutate(rng, rng.choice(adps), rng.choice([0.0, 0.08, 0.25]))
                p = rng.randint(0, max(0, n - len(a)))
                r = (r[:p] + a + r[p + len(a):])[:n]
            assert len(r) == n
            ws.append(r)
        wins.append(ws)
    return wins, tables


@pytest.mark.gpu
@pytest.mark.parametrize('scheme', SCHEMES)
def test_pshift_cross_and_grouped(gpu_lib, model, scheme, monkeypatch):
    from custom_porechop_abi_amd import _lib, engine
    L, vp = gpu_lib, ctypes.c_void_p
    monkeypatch.setenv('PCABI_SPLIT', '0')
    monkeypatch.delenv('PCABI_SHIFT', raising=False)
    wins, tables = _cases(70 + SCHEMES.index(scheme))
    n = N_WIN

    # the start and end tables hold four buckets each, so the engine merges none: the bucket of an
    # adapter is its length rounded up to 4 rows. From the host model: which run in the frame, and
    # that windows longer than the period exist (P < n: a rebase runs on the device).
    framed = 0
    for lens, ws in zip(TABLE_LENS[:2], wins[:2]):
        longest = max(len(w) for w in ws)
        for rpl in sorted({(x + 3) & ~3 for x in lens}):
            P = _bucket_period(model, [x for x in lens if (x + 3) & ~3 == rpl], rpl, scheme)
            if scheme == DECLINING and rpl == 64:
                assert P is None                     # the Lay unit of the grouped launch
                continue
            assert P is not None and P < longest, (scheme, rpl, P, longest)
            framed += 1
    assert framed == (7 if scheme == DECLINING else 8)

    bufs, tabs = [], []

    def h2d(a):
        a = np.ascontiguousarray(a)
        p = vp()
        _lib.check(L.pcabi_dev_malloc(ctypes.byref(p), max(a.nbytes, 16)), 'malloc')
        _lib.check(L.pcabi_dev_h2d(p, a.ctypes.data_as(vp), a.nbytes), 'h2d')
        bufs.append(p)
        return p

    def dalloc(nbytes):
        p = vp()
        _lib.check(L.pcabi_dev_malloc(ctypes.byref(p), max(nbytes, 16)), 'malloc')
        bufs.append(p)
        return p

    try:
        regions, singles, outs = [], [], []
        for w, adps in zip(wins, tables):
            pack = engine.SeqPack(w)
            lens = pack.lengths.astype(np.int32)
            assert list(lens[:64]) == [150] * 64 and lens[ZERO_AT] == 0
            offs = pack.offsets.astype(np.int64)
            toff = np.zeros((n + 255) // 256 + 1, np.int64)
            nd = L.pcabi_tile_layout(lens.ctypes.data_as(vp), n, toff.ctypes.data_as(vp))
            d_codes, d_off, d_len, d_toff = h2d(pack.codes), h2d(offs), h2d(lens), h2d(toff)
            d_tiles = dalloc(4 * int(nd))
            _lib.check(L.pcabi_tile_windows_dev(d_codes, d_off, d_len, n, d_toff, int(np.diff(toff).max() // 256),
                                                d_tiles, None), 'tile')
            c, o, l = engine.encode_adapters(adps)
            tab = vp()
            _lib.check(L.pcabi_adapters_create_scored(c.ctypes.data_as(vp), o.ctypes.data_as(vp), l.ctypes.data_as(vp),
                                                      len(adps), *scheme, ctypes.byref(tab)), 'adapters_create')
            tabs.append(tab)
            stride = n * len(adps)
            d_out, d_one = dalloc(4 * 8 * stride), dalloc(4 * 8 * stride)
            _lib.check(L.pcabi_dev_memset(d_out, 0x5A, 4 * 8 * stride), 'memset')
            _lib.check(L.pcabi_dev_memset(d_one, 0x5A, 4 * 8 * stride), 'memset')
            regions.append((d_tiles, d_toff, d_len, n, int(lens.max()), tab, d_out, stride))
            singles.append((d_tiles, d_toff, d_len, n, int(lens.max()), tab, d_one, stride))
            outs.append((d_out, d_one, stride, adps, w))
        st = vp()
        _lib.check(L.pcabi_stream_create(ctypes.byref(st)), 'stream')
        _lib.check(L.pcabi_align_cross_multi_dev(_lib.cross_regions(regions), len(regions), *scheme, st, None, None),
                   'multi')
        for r in singles:
            _lib.check(L.pcabi_align_cross_dev(*r[:6], *scheme, r[6], r[7], st), 'align')
        _lib.check(L.pcabi_stream_sync(st), 'sync')
        L.pcabi_stream_destroy(st)
        for d_out, d_one, stride, adps, w in outs:
            exp = oracle_lib.align_many(w, adps, (np.tile(np.arange(n), len(adps)), np.repeat(np.arange(len(adps)), n)),
                                        scheme)
            ok = exp[0] != -1
            assert int((~ok).sum()) == len(adps)                # the zero-length window, once per adapter:
            got = []                                            # the reference defines its field 0 only
            for d in (d_out, d_one):
                g = np.zeros((8, stride), np.int32)
                _lib.check(L.pcabi_dev_d2h(g.ctypes.data_as(vp), d, g.nbytes), 'd2h')
                assert np.array_equal(g[0], exp[0])
                bad = np.nonzero(np.any(g[:, ok] != exp[:, ok], axis=0))[0]
                assert bad.size == 0, (scheme, [(int(np.nonzero(ok)[0][k]) % n, int(np.nonzero(ok)[0][k]) // n)
                                                for k in bad[:8]])
                got.append(g)
            assert np.array_equal(got[0], got[1])
    finally:
        for t in tabs:
            L.pcabi_adapters_destroy(t)
        for p in bufs:
            L.pcabi_dev_free(p)
