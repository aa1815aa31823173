"""Argument checks of the host-buffer entry points (include/pcabi.h: the *_host / *_seqs entries and
the legacy drop-in). Every entry validates its arguments before its first HIP call, so a refused
call gives its code and message on a machine with no GPU; so do the few answers that need no device.
One bad argument at a time (two where the order of the checks is the point); no call here is a valid
compute call. check_compatibility is not covered: it asks HIP for the current device first."""
import ctypes

import numpy as np
import pytest

from custom_porechop_abi_amd import _lib

E_ARG = -1
P = ctypes.c_void_p
SC = (3, -6, -5, -2)


@pytest.fixture(scope='module')
def L():
    lib = _lib.lib()
    lib.pcabi_compat_host.argtypes = [ctypes.c_int, P, ctypes.c_int64, P, P, ctypes.c_int64, P, P, ctypes.c_int64, P]
    lib.pcabi_compat_host.restype = ctypes.c_int
    lib.pcabi_compat_all_vs_all_host.argtypes = [ctypes.c_int, P, ctypes.c_int64, P, P, ctypes.c_int64, P]
    lib.pcabi_compat_all_vs_all_host.restype = ctypes.c_int
    return lib


def p(a):
    return None if a is None else a.ctypes.data_as(P)


def i32(*v):
    return np.array(v, dtype=np.int32)


def i64(*v):
    return np.array(v, dtype=np.int64)


def refused(L, rc, msg):
    assert rc == E_ARG
    assert L.pcabi_last_error().decode() == msg


# two windows of 8 bases in a buffer of 8 + 8 + 16 bytes, two adapters of 4 bases
CODES = np.zeros(32, np.uint8)
WOFF, WLEN = i64(0, 8), i32(8, 8)
ACODES = np.zeros(8, np.uint8)
AOFF, ALEN = i32(0, 4), i32(4, 4)
OUT = np.zeros(8 * 4, np.int32)


def windows(**kw):
    """The (codes, codes_len, win_off, win_len, n_win, adp_codes, adp_off, adp_len, n_adp) run the
    windowed entries share, with replacements."""
    a = dict(codes=CODES, codes_len=CODES.size, woff=WOFF, wlen=WLEN, n_win=2, acodes=ACODES, aoff=AOFF, alen=ALEN,
             n_adp=2)
    a.update(kw)
    return (p(a['codes']), a['codes_len'], p(a['woff']), p(a['wlen']), a['n_win'], p(a['acodes']), p(a['aoff']),
            p(a['alen']), a['n_adp'])


def max_adp(L):
    return L.pcabi_max_adapter_len()


def max_win(L):
    return L.pcabi_max_window_len()


# (replacements of windows(), message); {A} / {W}: pcabi_max_adapter_len() / pcabi_max_window_len()
WINDOW_CASES = [
    (dict(n_win=-1), 'negative count'),
    (dict(n_adp=-1), 'negative count'),
    (dict(alen=i32(4, 0)), 'adapter length 0 outside 1..{A}'),
    (dict(alen='A+1'), 'adapter length {A1} outside 1..{A}'),
    (dict(wlen=i32(8, -1)), 'window length out of range'),
    (dict(wlen='W+1'), 'window length out of range'),
    (dict(woff=i64(0, 9)), 'window outside the buffer or buffer not padded by 16 bytes'),
    (dict(woff=i64(-1, 8)), 'window outside the buffer or buffer not padded by 16 bytes'),
    # two at once: the adapter lengths are checked before the windows, the counts before both
    (dict(alen=i32(0, 4), wlen=i32(-1, 8)), 'adapter length 0 outside 1..{A}'),
    (dict(n_win=-1, alen=i32(0, 4)), 'negative count'),
]


def window_case(L, kw, msg):
    kw = dict(kw)
    if isinstance(kw.get('alen'), str):
        kw['alen'] = i32(4, max_adp(L) + 1)
    if isinstance(kw.get('wlen'), str):
        kw['wlen'] = i32(8, max_win(L) + 1)
    return kw, msg.format(A=max_adp(L), A1=max_adp(L) + 1)


@pytest.mark.parametrize('device', [-1, 16])
def test_bad_device_index(L, device):
    msg = 'bad device index'
    refused(L, L.pcabi_align_host(device, *windows(), None, None, 0, *SC, p(OUT)), msg)
    best = np.zeros(2)
    refused(L, L.pcabi_best_full_identity_host(device, *windows(), *SC, p(best), 0), msg)
    refused(L, L.pcabi_first_hits_host(device, *windows(), *SC, 70.0, p(OUT)), msg)
    refused(L, L.pcabi_middle_scan_host(device, *windows(), *SC, 70.0, p(OUT), 4), msg)
    s = ctypes.c_char_p(b'ACGTACGT')
    addr = np.array([ctypes.cast(s, P).value], dtype=np.uint64)
    refused(L, L.pcabi_stage_seqs_host(device, p(addr), p(i32(8)), 1, p(CODES), CODES.size), msg)
    refused(L, L.pcabi_middle_scan_seqs(device, p(addr), p(i32(8)), 1, p(ACODES), p(AOFF), p(ALEN), 2, *SC, 70.0,
                                        p(OUT), 4), msg)
    refused(L, L.pcabi_middle_cuts_host(device, p(OUT), 0, 0, 1, p(CODES), p(CODES), 1, 0, 0, p(i64(0, 0)), None), msg)
    refused(L, L.pcabi_barcode_call_host(device, p(OUT), 1, p(i32(0)), p(i32(0)), 1, p(OUT), 1, p(i32(0)), p(i32(0)),
                                         1, 1, 70.0, 5.0, 0, p(i32(0)), None), msg)
    # the compatibility entries reach the check with their task lists built
    flag = i32(7)
    refused(L, L.pcabi_compat_host(device, p(CODES), CODES.size, p(WOFF), p(WLEN), 2, p(i32(0)), p(i32(1)), 1,
                                   p(flag)), msg)
    mat = np.zeros(4, np.int32)
    refused(L, L.pcabi_compat_all_vs_all_host(device, p(CODES), CODES.size, p(WOFF), p(WLEN), 2, p(mat)), msg)
    assert mat.tolist() == [-1, 0, 0, -1]          # the diagonal is written first
    refused(L, end_host(L, device=device), msg)
    refused(L, end_seqs(L, device=device), msg)


@pytest.mark.parametrize('kw,msg', WINDOW_CASES)
def test_windowed_entries_refuse(L, kw, msg):
    kw, msg = window_case(L, kw, msg)
    w = windows(**kw)
    refused(L, L.pcabi_align_host(0, *w, None, None, 0, *SC, p(OUT)), msg)
    refused(L, L.pcabi_first_hits_host(0, *w, *SC, 70.0, p(OUT)), msg)
    refused(L, L.pcabi_best_full_identity_host(0, *w, *SC, p(np.zeros(2)), 0), msg)
    refused(L, L.pcabi_middle_scan_host(0, *w, *SC, 70.0, p(OUT), 4), msg)


def test_align_host_tasks(L):
    for tw, ta in ((i32(0, 2), i32(0, 1)), (i32(0, -1), i32(0, 1)), (i32(0, 1), i32(0, 2)), (i32(0, 1), i32(-1, 1))):
        refused(L, L.pcabi_align_host(0, *windows(), p(tw), p(ta), 2, *SC, p(OUT)), 'task index out of range')
    refused(L, L.pcabi_align_host(0, *windows(), p(i32(0)), p(i32(0)), -1, *SC, p(OUT)), 'negative count')
    # the windows are checked before the tasks
    refused(L, L.pcabi_align_host(0, *windows(wlen=i32(8, -1)), p(i32(0, 2)), p(i32(0, 1)), 2, *SC, p(OUT)),
            'window length out of range')
    # nothing to align: no device needed
    assert L.pcabi_align_host(0, *windows(), p(i32(0)), p(i32(0)), 0, *SC, p(OUT)) == 0
    assert L.pcabi_align_host(0, *windows(n_win=0), None, None, 0, *SC, p(OUT)) == 0


def test_best_full_identity_host(L):
    refused(L, L.pcabi_best_full_identity_host(0, *windows(), *SC, None, 0), 'best is NULL')
    # no window or no adapter: every maximum stays as given, whatever the device index
    best = np.array([1.5, 2.5])
    assert L.pcabi_best_full_identity_host(-1, *windows(n_win=0), *SC, p(best), 0) == 0
    assert L.pcabi_best_full_identity_host(0, *windows(n_adp=0), *SC, None, 0) == 0
    assert best.tolist() == [1.5, 2.5]


def test_first_hits_host_without_a_device(L):
    hits = np.full(5 * 2, 9, np.int32)
    assert L.pcabi_first_hits_host(0, *windows(n_adp=0), *SC, 70.0, p(hits)) == 0
    assert hits.tolist() == [-1, -1, -1, -1, 0, 0, 0, 0, 0, 0]
    assert L.pcabi_first_hits_host(0, *windows(n_win=0), *SC, 70.0, p(hits)) == 0


def test_middle_scan_host(L):
    refused(L, L.pcabi_middle_scan_host(0, *windows(), *SC, 70.0, p(OUT), -1), 'negative count')
    assert L.pcabi_middle_scan_host(0, *windows(n_win=0), *SC, 70.0, p(OUT), 4) == 0
    assert L.pcabi_middle_scan_host(0, *windows(n_adp=0), *SC, 70.0, p(OUT), 4) == 0


def strings(*seqs):
    keep = [ctypes.c_char_p(s) if s is not None else None for s in seqs]
    addr = np.array([ctypes.cast(k, P).value or 0 if k is not None else 0 for k in keep], dtype=np.uint64)
    return keep, addr


def test_stage_seqs_host(L):
    keep, addr = strings(b'ACGTA', b'ACG')
    out = np.zeros(8 + 4 + 16, np.uint8)
    refused(L, L.pcabi_stage_seqs_host(0, p(addr), p(i32(5, 3)), -1, p(out), out.size), 'negative count')
    refused(L, L.pcabi_stage_seqs_host(0, p(addr), p(i32(5, -1)), 2, p(out), out.size), 'window length out of range')
    refused(L, L.pcabi_stage_seqs_host(0, p(addr), p(i32(5, max_win(L) + 1)), 2, p(out), out.size),
            'window length out of range')
    _, null = strings(b'ACGTA', None)
    refused(L, L.pcabi_stage_seqs_host(0, p(null), p(i32(5, 3)), 2, p(out), out.size), 'NULL sequence')
    refused(L, L.pcabi_stage_seqs_host(0, p(addr), p(i32(5, 3)), 2, p(out), out.size - 1),
            'output buffer smaller than the layout')
    # the sequences are checked before the size of the output
    refused(L, L.pcabi_stage_seqs_host(0, p(null), p(i32(5, 3)), 2, p(out), 0), 'NULL sequence')


def test_middle_scan_seqs(L):
    keep, addr = strings(b'ACGTA', b'ACG')
    tail = (p(ACODES), p(AOFF), p(ALEN), 2, *SC, 70.0, p(OUT), 4)
    refused(L, L.pcabi_middle_scan_seqs(0, p(addr), p(i32(5, 3)), -1, *tail), 'negative count')
    refused(L, L.pcabi_middle_scan_seqs(0, p(addr), p(i32(5, 3)), 2, p(ACODES), p(AOFF), p(ALEN), 2, *SC, 70.0, p(OUT),
                                        -1), 'negative count')
    refused(L, L.pcabi_middle_scan_seqs(0, p(addr), p(i32(5, 3)), 2, p(ACODES), p(AOFF), p(i32(4, 0)), 2, *SC, 70.0,
                                        p(OUT), 4), 'adapter length 0 outside 1..%d' % max_adp(L))
    refused(L, L.pcabi_middle_scan_seqs(0, p(addr), p(i32(5, -1)), 2, *tail), 'window length out of range')
    refused(L, L.pcabi_middle_scan_seqs(0, p(addr), p(i32(5, max_win(L) + 1)), 2, *tail), 'window length out of range')
    _, null = strings(None, b'ACG')
    refused(L, L.pcabi_middle_scan_seqs(0, p(null), p(i32(5, 3)), 2, *tail), 'NULL sequence')
    assert L.pcabi_middle_scan_seqs(0, p(addr), p(i32(5, 3)), 0, *tail) == 0
    assert L.pcabi_middle_scan_seqs(0, p(addr), p(i32(5, 3)), 2, p(ACODES), p(AOFF), p(ALEN), 0, *SC, 70.0, p(OUT),
                                    4) == 0


def test_middle_cuts_host(L):
    hits = np.array([[0, 1], [0, 1], [3, 4], [9, 9]], np.int32)      # rows read, adapter, start, end
    flags = np.zeros(2, np.uint8)
    off, cuts = np.zeros(3, np.int64), np.zeros(4, np.int64)

    def call(h=hits, stride=2, n_hits=2, n_reads=2, n_adp=2):
        return L.pcabi_middle_cuts_host(0, p(h), stride, n_hits, n_reads, p(flags), p(flags), n_adp, 0, 1, p(off),
                                        p(cuts))
    refused(L, call(n_hits=-1), 'bad counts')
    refused(L, call(n_reads=-1), 'bad counts')
    refused(L, call(n_adp=-1), 'bad counts')
    refused(L, call(stride=1), 'bad counts')                         # hit_stride < n_hits
    for r, c, v in ((0, 1, 2), (0, 0, -1), (1, 1, 2), (1, 0, -1)):
        h = hits.copy()
        h[r, c] = v
        refused(L, call(h=h), 'hit read / adapter index out of range')
    refused(L, call(stride=1, n_reads=1), 'bad counts')              # the counts come before the indices


def test_barcode_call_host(L):
    res = np.zeros(8 * 2, np.int32)
    call, slot = np.zeros(1, np.int32), i32(0, 1)

    def run(n_read=1, n_sa=2, n_ea=2, s_adp=slot, ns=2, e_adp=slot, ne=2):
        return L.pcabi_barcode_call_host(0, p(res), n_sa, p(s_adp), p(slot), ns, p(res), n_ea, p(e_adp), p(slot), ne,
                                         n_read, 70.0, 5.0, 0, p(call), None)
    for kw in (dict(n_read=-1), dict(n_sa=-1), dict(n_ea=-1), dict(ns=-1), dict(ne=-1)):
        refused(L, run(**kw), 'negative count')
    refused(L, run(s_adp=i32(0, 2)), 'start slot adapter out of range')
    refused(L, run(s_adp=i32(-1, 1)), 'start slot adapter out of range')
    refused(L, run(e_adp=i32(0, 2)), 'end slot adapter out of range')
    refused(L, run(s_adp=i32(0, 2), e_adp=i32(2, 0)), 'start slot adapter out of range')
    assert run(n_read=0) == 0


def test_compat_host(L):
    flags = np.full(2, 7, np.int32)

    def run(n_seq=2, pi=i32(0), pj=i32(1), n_pairs=1, lens=WLEN, device=0):
        return L.pcabi_compat_host(device, p(CODES), CODES.size, p(WOFF), p(lens), n_seq, p(pi), p(pj), n_pairs,
                                   p(flags))
    refused(L, run(n_seq=-1), 'negative count')
    refused(L, run(n_pairs=-1), 'negative count')
    refused(L, run(n_seq=2 ** 31), 'too many sequences')
    for pi, pj in ((i32(2), i32(1)), (i32(-1), i32(1)), (i32(0), i32(2)), (i32(0), i32(-1))):
        refused(L, run(pi=pi, pj=pj), 'pair index out of range')
    refused(L, run(lens=i32(max_adp(L) + 2, max_adp(L) + 1)),
            'check_compatibility: the shorter sequence exceeds %d bases' % max_adp(L))
    # pairs with an empty sequence are answered without a device, whatever its index
    assert run(lens=i32(8, 0), pi=i32(0, 1), pj=i32(1, 0), n_pairs=2, device=-1) == 0
    assert flags.tolist() == [0, 0]
    assert run(n_pairs=0) == 0


def test_compat_all_vs_all_host(L):
    refused(L, L.pcabi_compat_all_vs_all_host(0, p(CODES), CODES.size, p(WOFF), p(WLEN), -1, None), 'negative count')
    refused(L, L.pcabi_compat_all_vs_all_host(0, p(CODES), CODES.size, p(WOFF), p(WLEN), 46341, None),
            'too many sequences for one matrix')
    mat = np.zeros(1, np.int32)
    assert L.pcabi_compat_all_vs_all_host(0, p(CODES), CODES.size, p(WOFF), p(WLEN), 1, p(mat)) == 0
    assert mat.tolist() == [-1]
    assert L.pcabi_compat_all_vs_all_host(0, p(CODES), CODES.size, p(WOFF), p(WLEN), 0, p(mat)) == 0


# ---- end decisions: one read, start window [0, 8), end window [8, 16) -----------------------------
def end_args(kw):
    a = dict(device=0, codes_len=CODES.size, s_off=i64(0), s_len=i32(8), e_off=i64(8), e_len=i32(8), n_read=1,
             sa_len=ALEN, n_sa=2, ea_len=ALEN, n_ea=2, cap=4, bc_s=i32(0), n_bc_s=1, bc_e=i32(1), n_bc_e=1)
    a.update(kw)
    return a


def end_host(L, **kw):
    a = end_args(kw)
    trim, hits, cnt, full = np.zeros(1, np.int32), np.zeros(7 * 4, np.int32), np.full(2, 9, np.int64), np.zeros(2)
    rc = L.pcabi_end_decisions_host(a['device'], p(CODES), a['codes_len'], p(a['s_off']), p(a['s_len']), p(a['e_off']),
                                    p(a['e_len']), a['n_read'], p(ACODES), p(AOFF), p(a['sa_len']), a['n_sa'],
                                    p(ACODES), p(AOFF), p(a['ea_len']), a['n_ea'], *SC, 8, 2, 75.0, 4, p(trim), p(trim),
                                    p(hits), p(hits), a['cap'], p(cnt), p(a['bc_s']), a['n_bc_s'], p(a['bc_e']),
                                    a['n_bc_e'], p(full))
    end_host.cnt = cnt.tolist()
    return rc


def end_seqs(L, win=(b'ACGTACGT', b'TTTTACGT'), win_len=None, **kw):
    a = end_args(kw)
    keep, addr = strings(*win)
    win_len = i32(8, 8) if win_len is None else win_len
    trim, hits, cnt, full = np.zeros(1, np.int32), np.zeros(7 * 4, np.int32), np.full(2, 9, np.int64), np.zeros(2)
    return L.pcabi_end_decisions_seqs(a['device'], p(addr), p(win_len), a['n_read'], p(ACODES), p(AOFF),
                                      p(a['sa_len']), a['n_sa'], p(ACODES), p(AOFF), p(a['ea_len']), a['n_ea'], *SC, 8,
                                      2, 75.0, 4, p(trim), p(trim), p(hits), p(hits), a['cap'], p(cnt), p(a['bc_s']),
                                      a['n_bc_s'], p(a['bc_e']), a['n_bc_e'], p(full))


@pytest.mark.parametrize('entry', ['host', 'seqs'])
def test_end_decisions_refuse(L, entry):
    run = end_host if entry == 'host' else end_seqs
    A = max_adp(L)
    for kw in (dict(n_read=-1), dict(n_sa=-1), dict(n_ea=-1), dict(cap=-1), dict(n_bc_s=-1), dict(n_bc_e=-1)):
        refused(L, run(L, **kw), 'negative count')
    refused(L, run(L, sa_len=i32(4, 0)), 'adapter length 0 outside 1..%d' % A)
    refused(L, run(L, ea_len=i32(A + 1, 4)), 'adapter length %d outside 1..%d' % (A + 1, A))
    refused(L, run(L, bc_s=i32(2)), 'start barcode adapter out of range')
    refused(L, run(L, bc_s=i32(-1)), 'start barcode adapter out of range')
    refused(L, run(L, bc_e=i32(2)), 'end barcode adapter out of range')
    # two at once: start side before end side, adapters before barcode indices
    refused(L, run(L, sa_len=i32(0, 4), ea_len=i32(A + 1, 4)), 'adapter length 0 outside 1..%d' % A)
    refused(L, run(L, ea_len=i32(4, 0), bc_s=i32(2)), 'adapter length 0 outside 1..%d' % A)


def test_end_decisions_host_windows(L):
    W = max_win(L)
    refused(L, end_host(L, s_len=i32(-1)), 'window length out of range')
    refused(L, end_host(L, e_len=i32(W + 1)), 'window length out of range')
    refused(L, end_host(L, e_off=i64(9)), 'window outside the buffer or buffer not padded by 16 bytes')
    refused(L, end_host(L, s_off=i64(-1)), 'window outside the buffer or buffer not padded by 16 bytes')
    refused(L, end_host(L, codes_len=CODES.size - 9), 'window outside the buffer or buffer not padded by 16 bytes')
    # the start windows are checked before the end windows, the adapters before either
    refused(L, end_host(L, s_off=i64(25), e_len=i32(-1)), 'window outside the buffer or buffer not padded by 16 bytes')
    refused(L, end_host(L, sa_len=i32(4, 0), s_len=i32(-1)), 'adapter length 0 outside 1..%d' % max_adp(L))
    assert end_host(L, n_read=0) == 0
    assert end_host.cnt == [0, 0]


def test_end_decisions_seqs_windows(L):
    W = max_win(L)
    refused(L, end_seqs(L, win_len=i32(8, -1)), 'window length out of range')
    refused(L, end_seqs(L, win_len=i32(W + 1, 8)), 'window length out of range')
    refused(L, end_seqs(L, win=(b'ACGTACGT', None)), 'NULL sequence')
    # the strings are laid out before the device index is looked at
    refused(L, end_seqs(L, win=(None, b'ACGTACGT'), device=-1), 'NULL sequence')
    assert end_seqs(L, n_read=0) == 0


def test_adapter_alignment_of_an_empty_string(L):
    for read, adp in ((b'', b'ACGT'), (b'ACGT', b'')):
        s = L.adapterAlignment(read, adp, *SC)
        assert ctypes.string_at(s) == b'-1,0,-1,0,-2147483648,0.000000,0.000000'
        L.freeCString(s)
