"""The gap-extend frame's four-column passes on the GPU (pcabi_dp.h align_lane_shift4, taken by
run_lane in cross mode when all live windows of a wave have one length: the headline's case). With
random per-window lengths tests/test_gpu_shift.py and tests/test_gpu_group.py only reach the
column-by-column loop, so here whole 64-window waves share a length: one wave for each length at
the pass boundaries (n - 1 a multiple of 4 and its neighbours) and around every rebase period
(8, 16, 32), and three waves that must take the old loop -- 63 equal lengths and one different,
64 equal lengths with a zero-length window among them, and the region's last wave cut short by
n_win (its live lanes agree, so that one runs the passes with idle lanes beside them). As
test_gpu_shift.py: PCABI_SPLIT=0, its 18 adapter lengths (every bucket from 4 to 32 rows) and its
four schemes, through pcabi_align_cross_dev and pcabi_align_cross_multi_dev, result buffers
pre-filled with 0x5A. Every field of every pair against the oracle (for the zero-length window the
reference defines field 0 only, as in tests/test_gpu_parity.py), and the two calls against each
other in every field."""
import ctypes
import random

import numpy as np
import pytest

from tests import oracle_lib
from tests.test_gpu_parity import _mutate, _rand_seq
from tests.test_gpu_shift import ADP_LENS, SCHEMES

UNIFORM = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 15, 16, 17, 19, 20, 21, 31, 32, 33, 35, 36, 37, 64, 65, 150]
LAST_LIVE = 40   # windows of the region's last wave


def _wave_lengths():
    lens = []
    for n in UNIFORM:
        lens += [n] * 64
    lens += [20] * 17 + [23] + [20] * 46       # one lane disagrees
    lens += [33] * 40 + [0] + [33] * 23        # a zero-length window among equals
    lens += [24] * LAST_LIVE                   # cut short by n_win
    return lens


def _cases(seed):
    rng = random.Random(seed)
    adps = [_rand_seq(rng, L, rng.choice(['ACGT', 'ACGT', 'AT'])) for L in ADP_LENS]
    wins = []
    for k, n in enumerate(_wave_lengths()):
        r = _rand_seq(rng, n, rng.choice(['ACGT', 'ACGT', 'AT', 'ACGTN']))
        if n >= 12 and k % 2:
            a = _mutate(rng, rng.choice(adps), rng.choice([0.0, 0.08, 0.25]))
            p = rng.randint(0, max(0, n - len(a)))
            r = (r[:p] + a + r[p + len(a):])[:n]
        assert len(r) == n
        wins.append(r)
    return wins, adps


@pytest.mark.gpu
@pytest.mark.parametrize('scheme', SCHEMES)
def test_uniform_waves_cross_and_grouped(gpu_lib, scheme, monkeypatch):
    from custom_porechop_abi_amd import _lib, engine
    L, vp = gpu_lib, ctypes.c_void_p
    monkeypatch.setenv('PCABI_SPLIT', '0')
    wins, adps = _cases(50 + SCHEMES.index(scheme))
    n = len(wins)
    assert n == (len(UNIFORM) + 2) * 64 + LAST_LIVE
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
        pack = engine.SeqPack(wins)
        lens = pack.lengths.astype(np.int32)
        assert list(lens) == _wave_lengths()
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
        region = (d_tiles, d_toff, d_len, n, int(lens.max()), tab, d_out, stride)
        st = vp()
        _lib.check(L.pcabi_stream_create(ctypes.byref(st)), 'stream')
        _lib.check(L.pcabi_align_cross_multi_dev(_lib.cross_regions([region]), 1, *scheme, st, None, None), 'multi')
        _lib.check(L.pcabi_align_cross_dev(*region[:6], *scheme, d_one, stride, st), 'align')
        _lib.check(L.pcabi_stream_sync(st), 'sync')
        L.pcabi_stream_destroy(st)
        exp = oracle_lib.align_many(wins, adps, (np.tile(np.arange(n), len(adps)), np.repeat(np.arange(len(adps)), n)),
                                    scheme)
        ok = exp[0] != -1
        assert int((~ok).sum()) == len(adps)                    # the zero-length window, once per adapter
        got = []
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
