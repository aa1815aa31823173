"""The run-tagged buckets' gap-extend frame on the GPU (pcabi_dp.h pk::LayS, k_align<.., SHIFT> and
class 0 of k_align_group): cross-mode launches whose adapters all pass pcabi::shift_ok keep their DP
keys relative to the anti-diagonal and rebase them every P columns (P = 32 up to 24 rows, 16 at 28,
8 at 32). Every field of every (window, adapter) pair against the oracle, through
pcabi_align_cross_dev (one launch per bucket; PCABI_SPLIT=0 keeps the small launches off the row-split
core, which stays on LayT) and through pcabi_align_cross_multi_dev (grouped launches) over a start, an
end and a ragged region. Window lengths sit around every period (P - 1, P, P + 1, 2 P) and at 1, 2, 150
and 400 columns; the adapters fill every bucket from 4 to 32 rows, several with padding rows. The
schemes: the default and (1, -1, -3, -1), which run the frame in every bucket; (2, -3, -5, -1), whose
22-31 bp adapters shift_ok declines (H runs of up to 3 L + 5 columns outgrow the tags) while layt_ok
accepts them -- so their buckets fall back to LayT next to shifted ones in the same grouped launch;
and (3, -6, -2, -5), which runs with shorter periods where |ge| = 5 widens the frame, and whose
buckets holding adapters of 25 bp and more leave the run-tagged layout altogether (packed keys)."""
import ctypes
import random

import numpy as np
import pytest

from tests import oracle_lib
from tests.test_gpu_parity import _mutate, _rand_seq

SCHEMES = [(3, -6, -5, -2), (1, -1, -3, -1), (2, -3, -5, -1), (3, -6, -2, -5)]
ADP_LENS = [1, 3, 4, 7, 8, 12, 13, 16, 19, 20, 21, 22, 24, 24, 26, 28, 30, 31]
WIN_LENS = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 64, 150, 150, 400]
N_WIN = 300   # two tiles of 256, the second ragged


def _cases(seed):
    rng = random.Random(seed)
    adps = [_rand_seq(rng, L, rng.choice(['ACGT', 'ACGT', 'AT'])) for L in ADP_LENS]
    wins = []
    for _ in range(3):   # start, end, ragged: three regions with windows of their own
        ws = []
        for k in range(N_WIN):
            n = rng.choice(WIN_LENS)
            r = _rand_seq(rng, n, rng.choice(['ACGT', 'ACGT', 'AT', 'ACGTN']))
            if n >= 31 and k % 2:
                a = _mutate(rng, rng.choice(adps), rng.choice([0.0, 0.08, 0.25]))
                p = rng.randint(0, max(0, n - len(a)))
                r = (r[:p] + a + r[p + len(a):])[:n]
            ws.append(r)
        wins.append(ws)
    # region tables: all buckets; the 21-24 bp bucket alone with the 32-row one; the small buckets
    tables = [adps, [a for a in adps if len(a) >= 21], [a for a in adps if len(a) <= 20]]
    return wins, tables


@pytest.mark.gpu
@pytest.mark.parametrize('scheme', SCHEMES)
def test_shift_cross_and_grouped(gpu_lib, scheme, monkeypatch):
    from custom_porechop_abi_amd import _lib, engine
    L, vp = gpu_lib, ctypes.c_void_p
    monkeypatch.setenv('PCABI_SPLIT', '0')
    wins, tables = _cases(SCHEMES.index(scheme))
    n = N_WIN
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
            for d in (d_out, d_one):
                got = np.zeros((8, stride), np.int32)
                _lib.check(L.pcabi_dev_d2h(got.ctypes.data_as(vp), d, got.nbytes), 'd2h')
                assert np.array_equal(got, exp)
    finally:
        for t in tabs:
            L.pcabi_adapters_destroy(t)
        for p in bufs:
            L.pcabi_dev_free(p)
