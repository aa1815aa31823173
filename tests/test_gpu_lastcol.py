"""The gap-extend-frame cores' own last column on the GPU (pcabi_dp.h LaneShift::last_column and
LanePShift::last_column: k_align<.., SHIFT / PSHIFT> and both classes of k_align_group). The column
offers max(H, S) per row to the scout's key and reads Best off the surviving key, so the windows
here are the ones that end in it (tests/test_dp_core_lastcol_cpu.py's generators: an adapter prefix
ending at the window's end, the same followed by 1-3 foreign bases, the whole adapter ending at
column n, the whole adapter before a foreign tail, no hit), each built for an adapter of its own
region's table. Eight waves of 64 windows per region: uniform waves of 1, 2, 4, 5, 6, 33 and 150
columns (the four-column passes with 0, 1, 0, 0, 1, 8 and 37 whole passes and every count of
columns left over before the last one) and one ragged wave (the column-by-column loop). Four
regions whose tables hold four buckets each, so the engine merges none and every bucket from 4 to
64 rows runs as itself, each with a full-length adapter and one with padding rows. The default scheme
and (3, -6, -2, -5), where H wins ties at other places and the 28- and 32-row buckets leave the
frame. As tests/test_gpu_cross_uniform.py: PCABI_SPLIT=0, through pcabi_align_cross_dev and
pcabi_align_cross_multi_dev, result buffers pre-filled with 0x5A; every field of every pair
against the oracle, and the two calls against each other."""
import ctypes
import random

import numpy as np
import pytest

from tests import oracle_lib
from tests.test_dp_core_lastcol_cpu import category, windows
from tests.test_gpu_parity import _rand_seq

SCHEMES = [(3, -6, -5, -2), (3, -6, -2, -5)]
UNIFORM = [1, 2, 4, 5, 6, 33, 150]
RAGGED = [1, 2, 3, 5, 7, 9, 16, 17, 31, 33, 64, 65, 100, 149, 150, 150]
# per region: adapter lengths filling four buckets, a full one and one with padding rows in each
TABLE_LENS = [[4, 2, 12, 10, 20, 17, 28, 26], [8, 5, 16, 13, 24, 22, 31, 29],
              [36, 33, 44, 42, 52, 49, 60, 58], [40, 37, 48, 46, 56, 53, 63, 61]]


def _wave_lengths(rng):
    lens = []
    for n in UNIFORM:
        lens += [n] * 64
    return lens + [rng.choice(RAGGED) for _ in range(64)]


def _cases(seed):
    rng = random.Random(seed)
    tables = [[_rand_seq(rng, L, rng.choice(['ACGT', 'ACGT', 'ACG', 'AT'])) for L in lens] for lens in TABLE_LENS]
    wins = []
    for adps in tables:
        ws = []
        for k, n in enumerate(_wave_lengths(rng)):
            ws.append(windows(rng, adps[k % len(adps)], n)[(k // len(adps)) % 5])
            assert len(ws[-1]) == n
        wins.append(ws)
    return wins, tables


@pytest.mark.gpu
@pytest.mark.parametrize('scheme', SCHEMES)
def test_last_column_cross_and_grouped(gpu_lib, scheme, monkeypatch):
    from custom_porechop_abi_amd import _lib, engine
    L, vp = gpu_lib, ctypes.c_void_p
    monkeypatch.setenv('PCABI_SPLIT', '0')
    monkeypatch.delenv('PCABI_SHIFT', raising=False)
    wins, tables = _cases(90 + SCHEMES.index(scheme))
    n = len(wins[0])
    assert n == 64 * (len(UNIFORM) + 1)
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
            assert all(list(lens[64 * k:64 * k + 64]) == [u] * 64 for k, u in enumerate(UNIFORM))
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
        cats = {}
        for d_out, d_one, stride, adps, w in outs:
            pa = np.repeat(np.arange(len(adps)), n)
            pw = np.tile(np.arange(n), len(adps))
            exp = oracle_lib.align_many(w, adps, (pw, pa), scheme)
            got = []
            for d in (d_out, d_one):
                g = np.zeros((8, stride), np.int32)
                _lib.check(L.pcabi_dev_d2h(g.ctypes.data_as(vp), d, g.nbytes), 'd2h')
                bad = np.nonzero(np.any(g != exp, axis=0))[0]
                assert bad.size == 0, (scheme, [(int(k) % n, int(k) // n) for k in bad[:8]])
                got.append(g)
            assert np.array_equal(got[0], got[1])
            for k in range(stride):
                c = category([int(x) for x in exp[:, k]], len(w[pw[k]]), len(adps[pa[k]]))
                cats[c] = cats.get(c, 0) + 1
        print('scheme', scheme, 'winner categories', sorted(cats.items()))
        # the windows reach every kind of winner the column tells apart (the oracle's own fields)
        assert all(cats.get(c, 0) >= 100 for c in ('below_d', 'below_h', 'corner', 'row_l', 'none')), cats
    finally:
        for t in tabs:
            L.pcabi_adapters_destroy(t)
        for p in bufs:
            L.pcabi_dev_free(p)
