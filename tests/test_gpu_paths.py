"""Alignment paths and adapter profiles on the GPU (csrc/pcabi_paths.hip) against the oracle's own
gapped rows (tests/path_oracle.c): run lists equal pair by pair, the eight fields equal
engine.align's, the pileup equal to a numpy accumulation over the helper's rows."""
import ctypes
import random

import numpy as np
import pytest

from tests import path_oracle_lib
from tests.identity_ref import ref_pid6
from tests.test_gpu_parity import SCHEMES, _mutate, _rand_seq
from tests.test_paths_cpu import DEFAULT, KNOWN

pytestmark = pytest.mark.gpu

LANE_EDGE_ROWS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128)


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _expected_runs(reads, adps, pairs, scheme):
    return [path_oracle_lib.runs(reads[w], adps[a], scheme) for w, a in zip(*pairs)]


def _check(reads, adps, pairs, scheme):
    """engine.align_paths over whole reads as windows: runs equal the helper's pair by pair, the
    fields equal engine.align's."""
    from custom_porechop_abi_amd import engine
    pack = engine.SeqPack(reads)
    win = pack.views(np.zeros(len(reads), np.int64), pack.lengths)
    pairs = (np.asarray(pairs[0], np.int32), np.asarray(pairs[1], np.int32))
    res, run_off, runs = engine.align_paths(win, adps, scheme, pairs)
    assert np.array_equal(res, engine.align(win, adps, scheme, pairs=pairs))
    assert run_off[0] == 0 and run_off[-1] == len(runs) and (np.diff(run_off) >= 0).all()
    for t, exp in enumerate(_expected_runs(reads, adps, pairs, scheme)):
        got = runs[run_off[t]:run_off[t + 1]]
        assert np.array_equal(got, exp), (t, reads[pairs[0][t]][:80], adps[pairs[1][t]], got[:12], exp[:12])
    return res, run_off, runs


def _cross(n_win, n_adp):
    return np.tile(np.arange(n_win), n_adp), np.repeat(np.arange(n_adp), n_win)


def _edge_case_set(seed):
    """60 windows x 10 adapters: adapters at the lane boundaries (two rows per lane), windows of 0,
    1, 149, 150, 151 and 600 bases over five alphabets (the small ones tie-heavy), and 150-base
    windows with an adapter planted at 8 % mutations. Adapters longer than their window included."""
    rng = random.Random(seed)
    adps = []
    for rows in LANE_EDGE_ROWS:
        adps.append(_rand_seq(rng, rows, {32: 'AT', 63: 'A'}.get(rows, 'ACGT')))
    reads = [_rand_seq(rng, n, alph) for alph in ('A', 'AT', 'ACGT', 'ACGTN', 'ACGT-')
             for n in (0, 1, 149, 150, 151, 600)]
    for k in range(30):
        a = _mutate(rng, adps[2 + k % 8], 0.08)
        body = _rand_seq(rng, 150, 'ACGT')
        p = rng.randint(0, 150 - min(len(a), 150))
        reads.append((body[:p] + a + body[p + len(a):])[:150])
    return reads, adps


def test_known_answers(gpu_lib):
    from custom_porechop_abi_amd import engine
    reads = [k[0] for k in KNOWN]
    adps = [k[1] for k in KNOWN]
    idx = np.arange(len(KNOWN))
    res, run_off, runs = _check(reads, adps, (idx, idx), DEFAULT)
    for t, (read, adapter, rr, ar) in enumerate(KNOWN):
        r = runs[run_off[t]:run_off[t + 1]]
        assert engine.path_rows(r, read, adapter) == (rr, ar)
        assert engine.path_fields(r) == [int(x) for k, x in enumerate(res[:, t]) if k != 4]


@pytest.mark.parametrize('scheme', SCHEMES[:6])
def test_runs_exact_at_lane_boundaries(gpu_lib, scheme):
    reads, adps = _edge_case_set(11 + SCHEMES.index(scheme))
    _check(reads, adps, _cross(len(reads), len(adps)), scheme)


def test_long_reads(gpu_lib):
    """8 kb and 40 kb reads (traces in device scratch, column offsets past 32 k): an adapter planted
    past position 33,000 and one near the end."""
    rng = random.Random(5)
    adps = [_rand_seq(rng, 24, 'ACGT'), _rand_seq(rng, 68, 'ACGT')]
    r8 = _rand_seq(rng, 8000, 'ACGT')
    r8 = r8[:7950] + _mutate(rng, adps[0], 0.08) + r8[7950:7960]
    r40 = _rand_seq(rng, 40000, 'ACGT')
    r40 = r40[:33500] + _mutate(rng, adps[1], 0.08) + r40[33500:39960] + _mutate(rng, adps[0], 0.05) + r40[39960:39970]
    res, _, _ = _check([r8, r40], adps, _cross(2, 2), DEFAULT)
    assert res[0, 0] > 7000 and res[0, 1] > 33000 and res[0, 3] > 33000     # pairs: adapter-major


@pytest.mark.parametrize('scheme', [(2, -1, 0, 0), (0, 0, 0, 0), (1, -1, 1, 1)])
def test_free_gap_schemes_and_scratch_traces(gpu_lib, scheme):
    """Free-gap schemes (paths that wander over the whole matrix) on a 2,400-base window against a
    128-row adapter -- a trace that does not fit LDS -- and on 150 bases against 24 rows."""
    rng = random.Random(sum(scheme) + 40)
    adps = [_rand_seq(rng, 128, 'ACGT'), _rand_seq(rng, 24, 'ACGT')]
    reads = []
    for k in range(4):
        r = _rand_seq(rng, 2400, 'ACGT' if k % 2 else 'AT')
        reads.append(r[:1000] + _mutate(rng, adps[0], 0.08) + r[1000:2400 - 128])
    for k in range(8):
        r = _rand_seq(rng, 150, 'ACGTN' if k % 2 else 'ACGT')
        reads.append(r[:60] + _mutate(rng, adps[1], 0.1) + r[60:120])
    before = gpu_lib.pcabi_paths_scratch_pairs()
    pw = np.concatenate([np.arange(4), np.arange(4, 12), np.arange(4, 12)])
    pa = np.concatenate([np.zeros(4, int), np.ones(8, int), np.zeros(8, int)])
    _check(reads, adps, (pw, pa), scheme)
    print('pairs with the trace in device scratch:', gpu_lib.pcabi_paths_scratch_pairs() - before)


def test_rounds_within_a_small_scratch_budget(gpu_lib, monkeypatch):
    """A 1 MB budget: 2,400-base traces (0.3 MB each against 128 rows) run in several rounds, with
    LDS pairs in between, and give the same lists; a pair whose trace alone exceeds the budget is
    refused by name."""
    from custom_porechop_abi_amd import _lib, engine
    monkeypatch.setenv('PCABI_PATHS_SCRATCH_MB', '1')
    rng = random.Random(9)
    adps = [_rand_seq(rng, 128, 'ACGT'), _rand_seq(rng, 30, 'ACGT')]
    reads = [_rand_seq(rng, 2400, 'ACGT') for _ in range(5)] + [_rand_seq(rng, 150, 'ACGT') for _ in range(5)]
    _check(reads, adps, _cross(len(reads), 2), DEFAULT)
    reads.append(_rand_seq(rng, 9000, 'ACGT'))
    pack = engine.SeqPack(reads)
    win = pack.views(np.zeros(len(reads), np.int64), pack.lengths)
    with pytest.raises(_lib.PcabiError, match=r'\(-1\).*pair 1 .*9000 bases.*scratch budget'):
        engine.align_paths(win, adps, DEFAULT, ([0, 10], [0, 0]))


def _raw_host(L, win, adps, pairs, scheme, cap):
    from custom_porechop_abi_amd import engine
    codes, offs, lens = win
    ac, ao, al = engine.encode_adapters(adps)
    tw, ta = (np.ascontiguousarray(p, np.int32) for p in pairs)
    n = len(tw)
    res = np.full((8, n), 77, np.int32)
    run_off = np.full(n + 1, -5, np.int64)
    runs = np.zeros(max(cap, 1), np.uint32)
    total = L.pcabi_align_paths_host(0, _vp(codes), codes.size, _vp(offs), _vp(lens), len(lens), _vp(ac), _vp(ao),
                                     _vp(al), len(al), _vp(tw), _vp(ta), n, *scheme, _vp(res), _vp(run_off), _vp(runs),
                                     cap)
    return total, res, run_off, runs


def test_capacity_protocol(gpu_lib):
    from custom_porechop_abi_amd import engine
    reads, adps = _edge_case_set(3)
    reads, adps = reads[20:50], adps[3:7]
    pack = engine.SeqPack(reads)
    win = pack.views(np.zeros(len(reads), np.int64), pack.lengths)
    pairs = _cross(len(reads), len(adps))
    total, res, run_off, _ = _raw_host(gpu_lib, win, adps, pairs, DEFAULT, 1)
    assert total > 1 and run_off[0] == 0 and run_off[-1] == total and (np.diff(run_off) >= 0).all()
    total2, res2, run_off2, runs2 = _raw_host(gpu_lib, win, adps, pairs, DEFAULT, int(total))
    total3, res3, run_off3, runs3 = _raw_host(gpu_lib, win, adps, pairs, DEFAULT, int(total) + 5000)
    assert total2 == total3 == total
    assert np.array_equal(res, res3) and np.array_equal(run_off, run_off3)
    assert np.array_equal(res2, res3) and np.array_equal(run_off2, run_off3)
    assert np.array_equal(runs2[:total], runs3[:total])
    exp = np.concatenate(_expected_runs(reads, adps, pairs, DEFAULT))
    assert np.array_equal(runs3[:total], exp)


def test_limits_refused_from_the_arguments(gpu_lib):
    from custom_porechop_abi_amd import _lib, engine
    assert gpu_lib.pcabi_max_path_adapter_len() == 128
    pack = engine.SeqPack(['ACGTACGTAC' * 20])
    win = pack.views([0], pack.lengths)
    with pytest.raises(_lib.PcabiError, match=r'\(-1\).*129 bases'):
        engine.align_paths(win, ['A' * 129], DEFAULT, ([0], [0]))
    assert b'129' in gpu_lib.pcabi_last_error()


def test_device_abi_back_to_back(gpu_lib):
    """Two different batches one after the other on one caller stream (the scratch is reused): each
    equals the host ABI's answer, and the caller's codes are byte-identical afterwards."""
    from custom_porechop_abi_amd import _lib, engine
    L = gpu_lib
    check = _lib.check
    bufs = []

    def dev(a):
        a = np.ascontiguousarray(a)
        p = ctypes.c_void_p()
        check(L.pcabi_dev_malloc(ctypes.byref(p), max(a.nbytes, 16)), 'malloc')
        bufs.append(p)
        if a.nbytes:
            check(L.pcabi_dev_h2d(p, _vp(a), a.nbytes), 'h2d')
        return p

    def back(p, like):
        out = np.empty_like(like)
        if out.nbytes:
            check(L.pcabi_dev_d2h(_vp(out), p, out.nbytes), 'd2h')
        return out

    stream = ctypes.c_void_p()
    check(L.pcabi_stream_create(ctypes.byref(stream)), 'stream')
    try:
        rng = random.Random(21)
        batches = []
        for k, scheme in enumerate((DEFAULT, (2, -1, -1, -1))):
            reads, adps = _edge_case_set(70 + k)
            reads = reads[12 * k:12 * k + 36] + [_rand_seq(rng, 2400 + 100 * k, 'ACGT')]
            adps = adps[1 + k:9:2]
            pairs = _cross(len(reads), len(adps))
            batches.append((reads, adps, pairs, scheme))
        for reads, adps, pairs, scheme in batches:
            pack = engine.SeqPack(reads)
            win = pack.views(np.zeros(len(reads), np.int64), pack.lengths)
            want, wres, woff, wruns = _raw_host(L, win, adps, pairs, scheme, 1 << 16)
            assert 0 < want <= 1 << 16
            ac, ao, al = engine.encode_adapters(adps)
            tw, ta = (np.ascontiguousarray(p, np.int32) for p in pairs)
            n = len(tw)
            d_codes, d_off, d_len = dev(win[0]), dev(win[1]), dev(win[2])
            d_ac, d_ao, d_al, d_tw, d_ta = dev(ac), dev(ao), dev(al), dev(tw), dev(ta)
            d_res, d_roff, d_runs = dev(np.zeros((8, n), np.int32)), dev(np.zeros(n + 1, np.int64)), \
                dev(np.zeros(int(want), np.uint32))
            total = L.pcabi_align_paths_dev(d_codes, d_off, d_len, len(win[2]), d_ac, d_ao, d_al, len(al), d_tw, d_ta, n,
                                            *scheme, d_res, d_roff, d_runs, int(want), stream)
            assert total == want, (total, L.pcabi_last_error())
            assert np.array_equal(back(d_res, wres), wres)
            assert np.array_equal(back(d_roff, woff), woff)
            assert np.array_equal(back(d_runs, wruns[:want]), wruns[:want])
            assert np.array_equal(back(d_codes, win[0]), win[0])
    finally:
        check(L.pcabi_stream_destroy(stream), 'stream destroy')
        for p in bufs:
            L.pcabi_dev_free(p)


def _profile_reference(reads, adps, pairs, select, scheme):
    """The pileup by a plain walk over the helper's rows."""
    col = {'A': 0, 'C': 1, 'G': 2, 'T': 3, 'N': 4}
    counts = np.zeros((len(adps), max(len(a) for a in adps), 7), np.int64)
    for t, (w, a) in enumerate(zip(*pairs)):
        if not select[t]:
            continue
        rr, ar = path_oracle_lib.rows(reads[w], adps[a], scheme)
        has_r = [c != '-' for c in rr]
        has_a = [c != '-' for c in ar]
        if not rr:
            continue
        st = max(has_r.index(True), has_a.index(True))
        en = len(rr) - 1 - max(has_r[::-1].index(True), has_a[::-1].index(True))
        ai = 0
        for c in range(len(rr)):
            if st <= c <= en:
                if not has_a[c]:
                    counts[a, max(ai - 1, 0), 6] += 1
                elif not has_r[c]:
                    counts[a, ai, 5] += 1
                else:
                    counts[a, ai, col[rr[c]]] += 1
            ai += has_a[c]
    return counts


def test_adapter_profile(gpu_lib):
    from custom_porechop_abi_amd import engine
    rng = random.Random(33)
    adps = [_rand_seq(rng, n, 'ACGT') for n in (24, 33, 68)]
    reads = []
    for k in range(500):
        body = _rand_seq(rng, 150, 'ACGTN' if k % 7 == 0 else 'ACGT')
        if k % 5 != 4:
            a = _mutate(rng, adps[k % 3], 0.12)
            p = rng.randint(-10, 150 - len(a) + 10)         # some hang over either end
            body = (body[:max(p, 0)] + a[max(-p, 0):] + body[max(p, 0) + len(a):])[:150]
        reads.append(body)
    pairs = _cross(len(reads), len(adps))
    pack = engine.SeqPack(reads)
    win = pack.views(np.zeros(len(reads), np.int64), pack.lengths)
    res = engine.align(win, adps, DEFAULT, pairs=pairs)
    select = ref_pid6(res[5], res[7]) >= 75
    assert 200 < select.sum() < len(select)
    exp = _profile_reference(reads, adps, pairs, select, DEFAULT)
    assert exp[:, :, 5].sum() > 0 and exp[:, :, 6].sum() > 0 and exp[:, :, :4].sum() > 5000
    got = engine.adapter_profile(win, adps, DEFAULT, pairs, select=select)
    assert got.shape == (3, 68, 7) and got.dtype == np.int64
    assert np.array_equal(got, exp)
    again = engine.adapter_profile(win, adps, DEFAULT, pairs, select=select, counts=got)
    assert np.array_equal(again, 2 * exp)
    everything = engine.adapter_profile(win, adps, DEFAULT, pairs)
    assert np.array_equal(everything, _profile_reference(reads, adps, pairs, np.ones(len(pairs[0]), bool), DEFAULT))
