"""Batched host interface to the MI355X adapter-alignment engine (libpcabi.so).

Sequences travel as Dna5 codes (A=0 C=1 G=2 T/U=3 other=4; the table of
S/basic/alphabet_residue_tabs.h:113-140 in the reference's vendored SeqAn) packed in one
byte buffer. A *window* is an (offset, length) view into that buffer (any offset); the buffer
carries 16 bytes of padding past its last sequence, as libpcabi requires (include/pcabi.h).

The reference encodes each Python str with UTF-8 before handing it to SeqAn
(porechop_abi/cpp_function_wrappers.py:52), so a non-ASCII character becomes several N codes;
``encode_seq`` reproduces that byte-for-byte.
"""
import ctypes
import itertools

import numpy as np

from ._lib import NFIELDS, check, lib

DNA5 = np.full(256, 4, dtype=np.uint8)
for _c, _v in (('A', 0), ('C', 1), ('G', 2), ('T', 3), ('U', 3)):
    DNA5[ord(_c)] = _v
    DNA5[ord(_c.lower())] = _v

PAD = 16


_AS_UTF8 = None


try:
    from . import _pystr   # the drivers' host helpers (csrc/pystr.c, built by __graft_entry__.build)
except ImportError:        # not built: the same results through Python-level passes
    _pystr = None


def str_buffers(seqs):
    """(character addresses uint64[n], lengths int64[n]) of a list of ASCII strs in one native
    pass (_pystr.ascii_buffers), or None when an item is not an ASCII str. The addresses are
    valid while the strs live."""
    n = len(seqs)
    if n == 0:
        return None
    if _pystr is None:
        try:
            if not all(map(str.isascii, seqs)):
                return None
        except TypeError:
            return None
        return (np.fromiter(map(_as_utf8(), seqs), np.uint64, n), np.fromiter(map(len, seqs), np.int64, n))
    addr = np.empty(n, np.uint64)
    lens = np.empty(n, np.int64)
    return (addr, lens) if _pystr.ascii_buffers(seqs, addr, lens) else None


def _as_utf8():
    global _AS_UTF8
    if _AS_UTF8 is None:
        f = ctypes.pythonapi.PyUnicode_AsUTF8
        f.restype, f.argtypes = ctypes.c_void_p, [ctypes.py_object]
        _AS_UTF8 = f
    return _AS_UTF8


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def encode_seq(seq):
    """str -> Dna5 codes (uint8 array), byte-exact with the reference's UTF-8 marshalling."""
    return DNA5[np.frombuffer(seq.encode('utf-8'), dtype=np.uint8)]


class SeqPack(object):
    """Sequences packed back to back (4-aligned starts, 16 bytes tail padding)."""

    def __init__(self, seqs):
        raw = self._pack_ascii(seqs)
        if raw is None:
            parts = []
            offs = np.zeros(len(seqs), dtype=np.int64)
            lens = np.zeros(len(seqs), dtype=np.int32)
            pos = 0
            for k, s in enumerate(seqs):
                b = s.encode('utf-8') if isinstance(s, str) else bytes(s)
                n = len(b)
                offs[k] = pos
                lens[k] = n
                pad = (-n) & 3
                parts.append(b)
                if pad:
                    parts.append(b'N' * pad)
                pos += n + pad
            parts.append(b'N' * PAD)
            raw = b''.join(parts)
        else:
            raw, offs, lens = raw
        self.codes = np.empty(len(raw), dtype=np.uint8)
        # the S/basic/alphabet_residue_tabs.h table, in C (threads for large batches)
        lib().pcabi_encode_dna5(raw, self.codes.ctypes.data_as(ctypes.c_void_p), len(raw))
        self.offsets = offs
        self.lengths = lens

    @staticmethod
    def _pack_ascii(seqs):
        """The same layout for a list of ASCII str (reads always are): one join and one encode
        instead of one encode per sequence (8 kb reads: ~4x faster). None for anything else."""
        if not seqs or not all(type(x) is str for x in seqs):
            return None
        if sum(map(len, seqs)) > 2000 * len(seqs):         # long reads: the copies dominate, no gain
            return None
        lens = np.fromiter(map(len, seqs), dtype=np.int64, count=len(seqs))
        pads = (-lens) & 3
        fill = ('', 'N', 'NN', 'NNN')
        joined = ''.join(itertools.chain(itertools.chain.from_iterable(zip(seqs, map(fill.__getitem__, pads.tolist()))),
                                         ('N' * PAD,)))
        if not joined.isascii():                       # multi-byte UTF-8: byte lengths differ
            return None
        offs = np.zeros(len(seqs), dtype=np.int64)
        np.cumsum((lens + pads)[:-1], out=offs[1:])
        return joined.encode('ascii'), offs, lens.astype(np.int32)

    @classmethod
    def windows(cls, seqs, starts, lengths, index=None, bufs=None, lazy=False):
        """The pack of [seqs[k][a:a + l] for k, a, l in zip(index, starts, lengths)] (index
        defaults to every sequence once; same layout as SeqPack of those slices) without making
        them: for ASCII str the codes are gathered from the strs' own buffers by
        pcabi_encode_dna5_gather (one byte per base, so character positions are byte positions).
        `starts` / `lengths` must lie inside each sequence. bufs: str_buffers(seqs) when the caller
        has it already. lazy: for ASCII str, a StrWindows (the same layout, not yet gathered) instead."""
        starts = np.asarray(starts, np.int64)
        lengths = np.asarray(lengths, np.int64)
        idx = np.arange(len(seqs)) if index is None else np.asarray(index, np.int64)
        n = len(idx)
        # CPython keeps an ASCII str's bytes inside the object: PyUnicode_AsUTF8 is their address
        # (no copy), valid while `seqs` holds the strs -- i.e. for this call
        if bufs is None and n > 0:
            bufs = str_buffers(seqs)
        if n == 0 or bufs is None:                     # bytes / arrays / non-ASCII: the slicing path
            return cls([seqs[k][a:a + l] for k, a, l in zip(idx.tolist(), starts.tolist(), lengths.tolist())])
        have = bufs[1][idx]
        if len(starts) != n or len(lengths) != n or (starts < 0).any() or (lengths < 0).any() or \
                (starts + lengths > have).any():
            raise ValueError('SeqPack.windows: a window lies outside its sequence')
        addr = bufs[0][idx] + starts.astype(np.uint64)
        offs = np.zeros(n, np.int64)
        np.cumsum((lengths + ((-lengths) & 3))[:-1], out=offs[1:])
        total = int(offs[-1] + lengths[-1] + ((-lengths[-1]) & 3)) + PAD
        if lazy:
            return StrWindows(seqs, addr, lengths, offs, total)
        self = cls.__new__(cls)
        self.codes = np.empty(total, np.uint8)
        lib().pcabi_encode_dna5_gather(_ptr(addr), _ptr(lengths), _ptr(offs), n, _ptr(self.codes), total)
        self.offsets = offs
        self.lengths = lengths.astype(np.int32)
        return self

    def __len__(self):
        return len(self.lengths)

    def views(self, starts, lengths, index=None):
        """Window views [start, start+len) of packed sequences (start relative to each sequence):
        (codes, offsets, lengths). No copy -- the kernels accept any offset."""
        idx = np.arange(len(self.lengths)) if index is None else np.asarray(index)
        starts = np.asarray(starts, dtype=np.int64)
        lengths = np.asarray(lengths, dtype=np.int32)
        return self.codes, self.offsets[idx] + starts, lengths


class StrWindows(object):
    """A window pack not made yet: the windows as addresses into ASCII strs (str_buffers) and
    lengths, at SeqPack.windows' offsets. engine.end_decisions hands the addresses to the library,
    which gathers and encodes them into pinned staging buffers itself (pcabi_end_decisions_seqs);
    np.asarray(w) makes the Dna5 pack for anything that needs the bytes. `codes` is the object
    itself, so it stands where a SeqPack's codes buffer goes; it keeps `seqs` (the strs) alive."""

    def __init__(self, seqs, addr, lengths, offsets, total):
        self.seqs = seqs
        self.addr = np.ascontiguousarray(addr, np.uint64)
        self._lens64 = np.ascontiguousarray(lengths, np.int64)
        self.lengths = self._lens64.astype(np.int32)
        self.offsets = np.ascontiguousarray(offsets, np.int64)
        self.size = int(total)
        self.codes = self

    def __len__(self):
        return self.size

    def __array__(self, dtype=None, copy=None):
        codes = np.empty(self.size, np.uint8)
        lib().pcabi_encode_dna5_gather(_ptr(self.addr), _ptr(self._lens64), _ptr(self.offsets), len(self.lengths),
                                       _ptr(codes), self.size)
        return codes if dtype is None else codes.astype(dtype, copy=False)


def start_end_windows(pack, end_size):
    """(start windows, end windows) exactly as seq[:end_size] and seq[-end_size:]
    (porechop_abi/nanopore_read.py:164,169,181,203), as packed views."""
    n = pack.lengths.astype(np.int64)
    e = int(end_size)
    s_len = np.minimum(n, e) if e >= 0 else np.maximum(n + e, 0)
    if e > 0:
        e_start = np.maximum(n - e, 0)
    elif e == 0:
        e_start = np.zeros_like(n)          # seq[-0:] is the whole sequence
    else:
        e_start = np.minimum(-e, n)
    e_len = n - e_start
    sw = pack.views(np.zeros_like(n), s_len.astype(np.int32))
    ew = pack.views(e_start, e_len.astype(np.int32))
    return sw, ew


def encode_adapters(adapter_seqs):
    b = [encode_seq(s) for s in adapter_seqs]
    lens = np.array([len(x) for x in b], dtype=np.int32)
    offs = np.zeros(len(b), dtype=np.int32)
    if len(b) > 1:
        offs[1:] = np.cumsum(lens)[:-1]
    codes = np.concatenate(b + [np.zeros(PAD, np.uint8)]).astype(np.uint8)
    return codes, offs, lens


def align(windows, adapter_seqs, scoring_scheme_vals, pairs=None, device=0):
    """Align windows against adapters on the GPU.

    windows: (codes uint8, offsets int64, lengths int32) as from SeqPack.views.
    pairs=None -> cross product, result column a*n_win + w; else (win_idx, adp_idx) arrays.
    Returns int32 array (8, n_results): rs, re, as, ae, score, m, l1, l2 (pcabi.h field order).
    """
    codes, offs, lens = windows
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    acodes, aoffs, alens = encode_adapters(adapter_seqs)
    n_win = len(lens)
    n_adp = len(alens)
    if pairs is None:
        tw = ta = None
        n_task = 0
        n_res = n_win * n_adp
    else:
        tw = np.ascontiguousarray(pairs[0], dtype=np.int32)
        ta = np.ascontiguousarray(pairs[1], dtype=np.int32)
        n_task = len(tw)
        n_res = n_task
    out = np.zeros((NFIELDS, n_res), dtype=np.int32)
    if n_res == 0:
        return out
    m, mm, go, ge = (int(x) for x in scoring_scheme_vals[:4])
    rc = lib().pcabi_align_host(device, _ptr(codes), codes.size, _ptr(offs), _ptr(lens), n_win,
                                _ptr(acodes), _ptr(aoffs), _ptr(alens), n_adp,
                                _ptr(tw), _ptr(ta), n_task, m, mm, go, ge, _ptr(out))
    check(rc, 'pcabi_align_host')
    return out


def first_hits(windows, adapter_seqs, scoring_scheme_vals, threshold, device=0):
    """Middle-scan round 1 on the GPU (pcabi_first_hits_host): for every window, the first adapter
    in list order whose full-adapter identity is not below `threshold`.
    Returns int32 (5, n_win): adapter index (-1 = none), rs, re (inclusive), m, l2."""
    codes, offs, lens = windows
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    acodes, aoffs, alens = encode_adapters(adapter_seqs)
    n_win = len(lens)
    out = np.zeros((5, n_win), dtype=np.int32)
    if n_win == 0:
        return out
    m, mm, go, ge = (int(x) for x in scoring_scheme_vals[:4])
    rc = lib().pcabi_first_hits_host(device, _ptr(codes), codes.size, _ptr(offs), _ptr(lens), n_win,
                                     _ptr(acodes), _ptr(aoffs), _ptr(alens), len(alens), m, mm, go, ge,
                                     float(threshold), _ptr(out))
    check(rc, 'pcabi_first_hits_host')
    return out


def middle_scan(windows, adapter_seqs, scoring_scheme_vals, threshold, device=0):
    """The reference's masked re-alignment loop (nanopore_read.py:219-252) for a batch of reads,
    in rounds on the GPU (pcabi_middle_scan_host). Returns int32 (6, n_hits): read, adapter,
    read_start, read_end (exclusive), m, l2, in discovery order (per read: the reference's order)."""
    codes, offs, lens = windows
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    acodes, aoffs, alens = encode_adapters(adapter_seqs)
    n_win = len(lens)
    if n_win == 0 or not len(alens):
        return np.zeros((6, 0), np.int32)
    m, mm, go, ge = (int(x) for x in scoring_scheme_vals[:4])
    cap = max(1024, n_win // 4)
    while True:
        out = np.zeros((6, cap), dtype=np.int32)
        n = lib().pcabi_middle_scan_host(device, _ptr(codes), codes.size, _ptr(offs), _ptr(lens), n_win,
                                         _ptr(acodes), _ptr(aoffs), _ptr(alens), len(alens), m, mm, go, ge,
                                         float(threshold), _ptr(out), cap)
        if n < 0:
            check(int(n), 'pcabi_middle_scan_host')
        if n <= cap:
            return out[:, :n]
        cap = int(n)


def middle_scan_seqs(addr, lens, adapter_seqs, scoring_scheme_vals, threshold, device=0):
    """middle_scan over windows given as host string addresses (pcabi_middle_scan_seqs): addr
    uint64[n] the address of each window's first character (an ASCII str's own bytes, see
    str_buffers), lens its length; the library encodes them into pinned staging buffers while the
    earlier chunks copy to the device -- no Dna5 pack in pageable memory. Same result as
    middle_scan over the packed windows."""
    addr = np.ascontiguousarray(addr, dtype=np.uint64)
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    acodes, aoffs, alens = encode_adapters(adapter_seqs)
    n_win = len(lens)
    if n_win == 0 or not len(alens):
        return np.zeros((6, 0), np.int32)
    m, mm, go, ge = (int(x) for x in scoring_scheme_vals[:4])
    cap = max(1024, n_win // 4)
    while True:
        out = np.zeros((6, cap), dtype=np.int32)
        n = lib().pcabi_middle_scan_seqs(device, _ptr(addr), _ptr(lens), n_win, _ptr(acodes), _ptr(aoffs),
                                         _ptr(alens), len(alens), m, mm, go, ge, float(threshold), _ptr(out), cap)
        if n < 0:
            check(int(n), 'pcabi_middle_scan_seqs')
        if n <= cap:
            return out[:, :n]
        cap = int(n)


def best_full_identity(windows, adapter_seqs, scoring_scheme_vals, best=None, device=0, best_device_ptr=None):
    """Adapter-set search reduction on the GPU (pcabi_best_full_identity_host,
    porechop_abi/nanopore_read.py:158-173): best[a] = max(best[a], max over windows of the full
    identity of (window, adapter a)), the (adapter, window) results never leaving the device.
    best: float64[n_adp] start values (zeros if None), returned updated. best_device_ptr: an int
    device address of float64[n_adp] on `device` to update in place instead (e.g. the tensor an
    RCCL all-reduce reduces next); then None is returned."""
    codes, offs, lens = windows
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    acodes, aoffs, alens = encode_adapters(adapter_seqs)
    m, mm, go, ge = (int(x) for x in scoring_scheme_vals[:4])
    if best_device_ptr is not None:
        rc = lib().pcabi_best_full_identity_host(device, _ptr(codes), codes.size, _ptr(offs), _ptr(lens), len(lens),
                                                 _ptr(acodes), _ptr(aoffs), _ptr(alens), len(alens), m, mm, go, ge,
                                                 ctypes.c_void_p(int(best_device_ptr)), 1)
        check(rc, 'pcabi_best_full_identity_host')
        return None
    out = np.zeros(len(alens), np.float64) if best is None else np.array(best, dtype=np.float64)
    rc = lib().pcabi_best_full_identity_host(device, _ptr(codes), codes.size, _ptr(offs), _ptr(lens), len(lens),
                                             _ptr(acodes), _ptr(aoffs), _ptr(alens), len(alens), m, mm, go, ge,
                                             _ptr(out), 0)
    check(rc, 'pcabi_best_full_identity_host')
    return out


_END_LIST_RATIO = [4.0]


def end_decisions(codes, start_windows, end_windows, start_seqs, end_seqs, scoring_scheme_vals, end_size, extra_trim,
                  end_threshold, min_trim_size, bc_start=None, bc_end=None, device=0):
    """find_start_trim / find_end_trim for a batch of reads on the GPU (pcabi_end_decisions_host,
    porechop_abi/nanopore_read.py:175-217): only the decisions come back, never the result matrix.

    codes: one Dna5 buffer holding both window sets, or the StrWindows they are views of (start
    windows, then end windows: pcabi_end_decisions_seqs); start_windows / end_windows: (offsets
    int64, lengths int32). Returns (start_trim int32[n], end_trim int32[n], start_list, end_list,
    bc_full): each list is int32 (7, k) -- read, adapter, rs, re (inclusive), m, l1, l2 -- of the
    alignments the reference records, read-major in adapter order; bc_full is float64
    (len(bc_start) + len(bc_end), n) full identities of the listed adapters (None without them)."""
    s_off = np.ascontiguousarray(start_windows[0], dtype=np.int64)
    s_len = np.ascontiguousarray(start_windows[1], dtype=np.int32)
    e_off = np.ascontiguousarray(end_windows[0], dtype=np.int64)
    e_len = np.ascontiguousarray(end_windows[1], dtype=np.int32)
    n = len(s_len)
    # window strings (StrWindows: start windows then end windows, the views its own) go to the
    # library as addresses; anything else as a Dna5 buffer
    strs = isinstance(codes, StrWindows) and len(codes.lengths) == 2 * n and \
        np.array_equal(codes.offsets, np.concatenate([s_off, e_off])) and \
        np.array_equal(codes.lengths, np.concatenate([s_len, e_len]))
    if not strs:
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
    sa, so, sl = encode_adapters(start_seqs)
    ea, eo, el = encode_adapters(end_seqs)
    bs = np.ascontiguousarray(bc_start if bc_start is not None else [], dtype=np.int32)
    be = np.ascontiguousarray(bc_end if bc_end is not None else [], dtype=np.int32)
    st = np.zeros(n, np.int32)
    et = np.zeros(n, np.int32)
    nb = len(bs) + len(be)
    bc_full = np.zeros((nb, n), np.float64) if nb else None
    # list capacity from the most alignments per read seen so far (a call whose lists overflow runs
    # again -- the whole decision, ~half the driver's library time, r05); the lists are np.empty:
    # only the columns written are ever touched, so headroom costs address space, not time
    cap = int(n * _END_LIST_RATIO[0] * 1.25) + 1024
    m, mm, go, ge = (int(x) for x in scoring_scheme_vals[:4])
    while True:
        sh = np.empty((7, cap), np.int32)
        eh = np.empty((7, cap), np.int32)
        cnt = np.zeros(2, np.int64)
        if strs:
            rc = lib().pcabi_end_decisions_seqs(device, _ptr(codes.addr), _ptr(codes.lengths), n, _ptr(sa), _ptr(so),
                                                _ptr(sl), len(sl), _ptr(ea), _ptr(eo), _ptr(el), len(el), m, mm, go, ge,
                                                int(end_size), int(extra_trim), float(end_threshold),
                                                int(min_trim_size), _ptr(st), _ptr(et), _ptr(sh), _ptr(eh), cap,
                                                _ptr(cnt), _ptr(bs), len(bs), _ptr(be), len(be), _ptr(bc_full))
            check(rc, 'pcabi_end_decisions_seqs')
        else:
            rc = lib().pcabi_end_decisions_host(device, _ptr(codes), codes.size, _ptr(s_off), _ptr(s_len),
                                                _ptr(e_off), _ptr(e_len), n, _ptr(sa), _ptr(so), _ptr(sl), len(sl),
                                                _ptr(ea), _ptr(eo), _ptr(el), len(el), m, mm, go, ge, int(end_size),
                                                int(extra_trim), float(end_threshold), int(min_trim_size), _ptr(st),
                                                _ptr(et), _ptr(sh), _ptr(eh), cap, _ptr(cnt), _ptr(bs), len(bs),
                                                _ptr(be), len(be), _ptr(bc_full))
            check(rc, 'pcabi_end_decisions_host')
        if n:
            _END_LIST_RATIO[0] = max(_END_LIST_RATIO[0], float(cnt.max()) / n)
        if cnt.max() <= cap:
            return st, et, sh[:, :cnt[0]], eh[:, :cnt[1]], bc_full
        cap = int(cnt.max())


def middle_cuts(hits, n_reads, bad_start, bad_end, good_side, bad_side, device=0):
    """Middle trim ranges of a scan's hits on the GPU (pcabi_middle_cuts_host,
    porechop_abi/nanopore_read.py:233-250): hits int32 (>= 4, n_hits) rows read, adapter,
    read_start, read_end (exclusive); bad_start / bad_end: per adapter, its name is a start / end
    sequence name. Returns (cut_off int64[n_reads + 1], cuts int64[2 * n_hits]) grouped per read
    in discovery order -- pcabi_reads_write's cut layout."""
    hits = np.ascontiguousarray(hits, dtype=np.int32)
    n_hits = hits.shape[1] if hits.ndim == 2 else 0
    bs = np.ascontiguousarray(bad_start, dtype=np.uint8)
    be = np.ascontiguousarray(bad_end, dtype=np.uint8)
    cut_off = np.zeros(n_reads + 1, np.int64)
    cuts = np.zeros(2 * n_hits, np.int64)
    rc = lib().pcabi_middle_cuts_host(device, _ptr(hits), n_hits, n_hits, n_reads, _ptr(bs), _ptr(be), len(bs),
                                      int(good_side), int(bad_side), _ptr(cut_off), _ptr(cuts))
    check(rc, 'pcabi_middle_cuts_host')
    return cut_off, cuts


_PID6_TAB = []


def pid6(m, l):
    """float('%f' % (100*m/l)) elementwise (NaN where l == 0), the reference's identity text
    round trip (porechop_abi/src/alignment.cpp:118-119, porechop_abi/nanopore_read.py:497-498).
    Pairs with 0 <= m, l < 256 (every end-window alignment) come from a table the library filled
    once (pcabi_pid6_host over all 65,536 pairs): the drivers convert ~10^6 pairs per batch."""
    m = np.ascontiguousarray(m, dtype=np.int32)
    l = np.ascontiguousarray(l, dtype=np.int32)
    if m.size > 4096 and m.shape == l.shape:
        small = ((m | l) & ~255) == 0
        if small.all():
            if not _PID6_TAB:
                mm, ll = np.divmod(np.arange(65536, dtype=np.int32), 256)
                tab = np.empty(65536, dtype=np.float64)
                lib().pcabi_pid6_host(_ptr(np.ascontiguousarray(mm)), _ptr(np.ascontiguousarray(ll)), 65536, _ptr(tab))
                _PID6_TAB.append(tab)
            return _PID6_TAB[0][(m << 8) | l]
    out = np.empty(m.shape, dtype=np.float64)
    lib().pcabi_pid6_host(_ptr(m), _ptr(l), m.size, _ptr(out))
    return out


def identities(res):
    """(full_adapter_identity, aligned_region_identity, read_start, read_end_exclusive) arrays,
    the tuple align_adapter returns (porechop_abi/nanopore_read.py:485-500)."""
    rs = res[0]
    failed = rs == -1
    full = pid6(res[5], res[7])
    part = pid6(res[5], res[6])
    full[failed] = 0.0
    part[failed] = 0.0
    read_end = np.where(failed, 0, res[1] + 1).astype(np.int64)
    return full, part, rs.astype(np.int64), read_end


def barcode_call(start_res, end_res, start_slots, end_slots, n_read, barcode_threshold, barcode_diff,
                 require_two, device=0, with_scores=False):
    """determine_barcode for a batch of reads on the GPU (pcabi_barcode_call_host,
    porechop_abi/nanopore_read.py:408-482).

    start_res / end_res: int32 (8, n_adp * n_read) cross-product results (column a*n_read + r).
    *_slots: (slot_adp, slot_name) int32 arrays, the side's barcode dict in insertion order
    (porechop_abi.barcode_slots). Returns call int32[n_read] (barcode id, -1 = 'none') and, with
    with_scores, float64 (n_read, 4)."""
    def side(res, slots):
        res = np.ascontiguousarray(res, dtype=np.int32).reshape(NFIELDS, -1)
        adp = np.ascontiguousarray(slots[0], dtype=np.int32)
        name = np.ascontiguousarray(slots[1], dtype=np.int32)
        n_adp = res.shape[1] // n_read if n_read else 0
        return res, adp, name, n_adp

    sr, sa, sn, n_sa = side(start_res, start_slots)
    er, ea, en, n_ea = side(end_res, end_slots)
    call = np.full(n_read, -1, dtype=np.int32)
    scores = np.zeros((n_read, 4), dtype=np.float64) if with_scores else None
    if n_read:
        rc = lib().pcabi_barcode_call_host(device, _ptr(sr), n_sa, _ptr(sa), _ptr(sn), len(sa), _ptr(er), n_ea,
                                           _ptr(ea), _ptr(en), len(ea), n_read, float(barcode_threshold),
                                           float(barcode_diff), int(bool(require_two)), _ptr(call),
                                           _ptr(scores) if with_scores else None)
        check(rc, 'pcabi_barcode_call_host')
    return (call, scores) if with_scores else call


# ---- alignment paths and adapter profiles (include/pcabi.h, csrc/pcabi_paths.hip) ------------------
OP_MATCH, OP_MISMATCH, OP_READ_ONLY, OP_ADAPTER_ONLY = range(4)
PROFILE_COLS = ('A', 'C', 'G', 'T', 'N', 'DEL', 'INS')
_DNA5_LETTERS = 'ACGTN'
_PATH_RUNS_RATIO = [8.0]


def _path_inputs(windows, adapter_seqs, pairs):
    codes, offs, lens = windows
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    tw = np.ascontiguousarray(pairs[0], dtype=np.int32)
    ta = np.ascontiguousarray(pairs[1], dtype=np.int32)
    if len(tw) != len(ta):
        raise ValueError('pairs: the two index arrays differ in length')
    return codes, offs, lens, encode_adapters(adapter_seqs), tw, ta


def align_paths(windows, adapter_seqs, scoring_scheme_vals, pairs, device=0):
    """The alignments themselves for explicit (window, adapter) pairs (pcabi_align_paths_host).

    windows / pairs as for align. Returns (res, run_off, runs): res int32 (8, n) the fields align
    returns for the pairs; runs uint32, the columns of the gapped rows left to right, run-length
    encoded as (run_length << 2) | op (OP_MATCH, OP_MISMATCH, OP_READ_ONLY, OP_ADAPTER_ONLY); the
    runs of pair t are runs[run_off[t]:run_off[t + 1]] (none for an empty window). The run buffer
    grows and the call runs again when it was too small, as middle_scan does for its hits."""
    codes, offs, lens, (acodes, aoffs, alens), tw, ta = _path_inputs(windows, adapter_seqs, pairs)
    n = len(tw)
    res = np.zeros((NFIELDS, n), dtype=np.int32)
    run_off = np.zeros(n + 1, dtype=np.int64)
    if n == 0:
        return res, run_off, np.zeros(0, np.uint32)
    m, mm, go, ge = (int(x) for x in scoring_scheme_vals[:4])
    cap = int(n * _PATH_RUNS_RATIO[0] * 1.25) + 1024
    while True:
        runs = np.empty(cap, dtype=np.uint32)
        total = lib().pcabi_align_paths_host(device, _ptr(codes), codes.size, _ptr(offs), _ptr(lens), len(lens),
                                             _ptr(acodes), _ptr(aoffs), _ptr(alens), len(alens), _ptr(tw), _ptr(ta), n,
                                             m, mm, go, ge, _ptr(res), _ptr(run_off), _ptr(runs), cap)
        if total < 0:
            check(int(total), 'pcabi_align_paths_host')
        _PATH_RUNS_RATIO[0] = max(_PATH_RUNS_RATIO[0], float(total) / n)
        if total <= cap:
            return res, run_off, runs[:total]
        cap = int(total)


def path_ops(runs):
    """One op per column (uint8) from a pair's run list."""
    runs = np.asarray(runs, dtype=np.uint32)
    return np.repeat((runs & 3).astype(np.uint8), (runs >> 2).astype(np.int64))


def path_rows(runs, read, adapter):
    """(read_row, adapter_row): the gapped rows of a pair's run list as text, '-' for gaps and ACGTN
    letters (the way SeqAn prints Dna5: anything that is not A, C, G, T or U shows as N). No runs
    (no alignment: an empty sequence) give two empty rows."""
    ops = path_ops(runs)
    if len(ops) == 0:
        return '', ''
    rc, ac = encode_seq(read), encode_seq(adapter)
    has_r, has_a = ops != OP_ADAPTER_ONLY, ops != OP_READ_ONLY
    if int(has_r.sum()) != len(rc) or int(has_a.sum()) != len(ac):
        raise ValueError('path_rows: the run list does not belong to these sequences')
    letters = np.frombuffer((_DNA5_LETTERS + '-').encode(), np.uint8)
    rr = np.full(len(ops), 5, np.uint8)
    ar = np.full(len(ops), 5, np.uint8)
    rr[has_r] = rc
    ar[has_a] = ac
    return letters[rr].tobytes().decode(), letters[ar].tobytes().decode()


def path_fields(runs):
    """ScoredAlignment's rules (porechop_abi/src/alignment.cpp:6-110) over a pair's run list, on the
    CPU: [rs, re, as, ae, m, l1, l2] -- align's fields without the score; rs = -1 for no runs."""
    ops = path_ops(runs)
    if len(ops) == 0:
        return [-1, -1, -1, -1, 0, 0, 0]
    has_r, has_a = ops != OP_ADAPTER_ONLY, ops != OP_READ_ONLY
    rb = np.concatenate([[0], np.cumsum(has_r)])        # bases before each column
    ab = np.concatenate([[0], np.cumsum(has_a)])
    # the first column with a base seen in both rows, and the same from the right
    st = int(max(np.argmax(has_r), np.argmax(has_a)))
    n = len(ops)
    en = int(n - 1 - max(np.argmax(has_r[::-1]), np.argmax(has_a[::-1])))
    a_pos = np.flatnonzero(has_a)
    a0, a1 = int(a_pos[0]), int(a_pos[-1])
    m = int((ops[st:en + 1] == OP_MATCH).sum())
    return [int(rb[st]), int(rb[en]), int(ab[st]), int(ab[en]), m, en - st + 1, a1 - a0 + 1]


def format_alignment(runs, read, adapter):
    """Three lines of text: the read row, '|' under the matching columns, the adapter row."""
    rr, ar = path_rows(runs, read, adapter)
    mid = ''.join('|' if op == OP_MATCH else ' ' for op in path_ops(runs).tolist())
    return '%s\n%s\n%s' % (rr, mid, ar)


def adapter_profile(windows, adapter_seqs, scoring_scheme_vals, pairs, select=None, counts=None, device=0):
    """Per-position pileup of the windows over their adapters on the GPU (pcabi_align_paths_host,
    then pcabi_adapter_profile_host): int64 (n_adp, longest adapter, 7) counts of A, C, G, T, N,
    DEL, INS (PROFILE_COLS) per adapter position, over the aligned region of every pair (select: a
    boolean per pair, None = all). counts: an earlier result to add to (returned updated)."""
    codes, offs, lens, (acodes, aoffs, alens), tw, ta = _path_inputs(windows, adapter_seqs, pairs)
    n_adp = len(alens)
    max_len = int(alens.max()) if n_adp else 0
    if counts is None:
        counts = np.zeros((n_adp, max_len, len(PROFILE_COLS)), np.int64)
    else:
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        if counts.shape != (n_adp, max_len, len(PROFILE_COLS)):
            raise ValueError('adapter_profile: counts has shape %r, not %r'
                             % (counts.shape, (n_adp, max_len, len(PROFILE_COLS))))
    if len(tw) == 0 or counts.size == 0:
        return counts
    sel = None if select is None else np.ascontiguousarray(select, dtype=np.uint8)
    if sel is not None and len(sel) != len(tw):
        raise ValueError('adapter_profile: select has %d entries for %d pairs' % (len(sel), len(tw)))
    res, run_off, runs = align_paths((codes, offs, lens), adapter_seqs, scoring_scheme_vals, (tw, ta), device)
    rs = np.ascontiguousarray(res[0])
    rc = lib().pcabi_adapter_profile_host(device, _ptr(rs), _ptr(run_off), _ptr(runs), _ptr(codes), codes.size,
                                          _ptr(offs), _ptr(lens), len(lens), _ptr(tw), _ptr(ta), _ptr(sel), len(tw),
                                          n_adp, max_len, _ptr(counts))
    check(rc, 'pcabi_adapter_profile_host')
    return counts


# ---- gzip on the device (csrc/pcabi_deflate.hip) -------------------------------------------------
GZIP_LONG_LINE = 1024     # include/pcabi.h PCABI_GZIP_LONG_LINE
GZIP_BLOCK_CAP = 65535    # include/pcabi.h PCABI_GZIP_BLOCK_CAP


def _gzip_input(data, blocks):
    buf = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else \
        np.ascontiguousarray(data, np.uint8).reshape(-1)
    off = None if blocks is None else np.ascontiguousarray(blocks, np.int64)
    if off is not None and (off.ndim != 1 or off.size < 1):
        raise ValueError('blocks is the CSR list block_off[n_blocks + 1]')
    return buf, off


def gzip_block_len():
    """The fixed block length used when no block list is given (pcabi_gzip_block_len)."""
    return int(lib().pcabi_gzip_block_len())


def gzip_bound(n, n_blocks=0):
    """Capacity that always holds the stream of n bytes in n_blocks blocks (0: fixed blocks)."""
    return int(lib().pcabi_gzip_bound(int(n), int(n_blocks)))


def gzip_line_blocks(data, long_line=GZIP_LONG_LINE, cap=GZIP_BLOCK_CAP):
    """The writer's line-aligned block list for text (pcabi_gzip_plan_lines): int64 block_off."""
    buf, _ = _gzip_input(data, None)
    L = lib()
    nb = L.pcabi_gzip_plan_lines(_ptr(buf), buf.size, int(long_line), int(cap), None, 0)
    if nb < 0:
        check(int(nb), 'pcabi_gzip_plan_lines')
    off = np.zeros(nb + 1, np.int64)
    L.pcabi_gzip_plan_lines(_ptr(buf), buf.size, int(long_line), int(cap), _ptr(off), off.size)
    return off


def gzip_compress(data, blocks=None, device=0, cap=None):
    """data (bytes or a uint8 array) as a gzip stream compressed on GPU `device` (pcabi_gzip_host):
    Huffman-only deflate, one block per entry of blocks (block_off[n_blocks + 1], every block 1..65535
    bytes; None: fixed blocks of gzip_block_len()), possibly several gzip members. Returns bytes.
    cap (tests): the output capacity offered; a too small one raises ValueError naming the size
    needed."""
    buf, off = _gzip_input(data, blocks)
    L = lib()
    nb = 0 if off is None else off.size - 1
    size = gzip_bound(buf.size, nb) if cap is None else int(cap)
    out = np.empty(max(size, 1), np.uint8)
    n = L.pcabi_gzip_host(int(device), _ptr(buf), buf.size, None if off is None else _ptr(off), nb, _ptr(out), size)
    if n < 0:
        check(int(n), 'pcabi_gzip_host')
    if n > size:
        raise ValueError('gzip_compress: capacity %d, needed %d' % (size, n))
    return out[:n].tobytes()


# ---- gunzip on the device (csrc/pcabi_inflate.hip) -----------------------------------------------
BGZF_BLOCK_CAP = 65280    # include/pcabi.h PCABI_BGZF_BLOCK_CAP
BGZF_MEMBER_MAX = 65536   # include/pcabi.h PCABI_BGZF_MEMBER_MAX
BGZF_EOF = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')


def bgzf_compress(data, blocks=None, device=0, eof=True, cap=None):
    """data as a BGZF stream compressed on GPU `device` (pcabi_bgzf_host): one indexed gzip member per
    block (blocks: block_off[n_blocks + 1], every block 1..65280 bytes; None: fixed blocks of
    min(gzip_block_len(), 65280)), the 28-byte end-of-file member after them when eof. Returns bytes."""
    buf, off = _gzip_input(data, blocks)
    L = lib()
    nb = 0 if off is None else off.size - 1
    size = int(L.pcabi_bgzf_bound(buf.size, nb, int(bool(eof)))) if cap is None else int(cap)
    out = np.empty(max(size, 1), np.uint8)
    n = L.pcabi_bgzf_host(int(device), _ptr(buf), buf.size, None if off is None else _ptr(off), nb, int(bool(eof)),
                          _ptr(out), size)
    if n < 0:
        check(int(n), 'pcabi_bgzf_host')
    if n > size:
        raise ValueError('bgzf_compress: capacity %d, needed %d' % (size, n))
    return out[:n].tobytes()


def bgzf_index(data):
    """The members of a block-gzipped (BGZF) stream, listed from their headers without decoding
    (pcabi_gunzip_index): (in_off, out_off), int64 arrays of members + 1 entries (member starts and
    the prefix sums of the decoded sizes), or None when the stream is gzip but not indexable.
    A broken or truncated chain raises PcabiError."""
    buf, _ = _gzip_input(data, None)
    L = lib()
    m = L.pcabi_gunzip_index(_ptr(buf), buf.size, None, None, 0)
    if m < 0:
        check(int(m), 'pcabi_gunzip_index')
    if m == 0:
        return None
    in_off, out_off = np.zeros(m + 1, np.int64), np.zeros(m + 1, np.int64)
    L.pcabi_gunzip_index(_ptr(buf), buf.size, _ptr(in_off), _ptr(out_off), m + 1)
    return in_off, out_off


def gunzip(data, device=0, cap=None):
    """A block-gzipped stream inflated on GPU `device` (pcabi_gunzip_host). Returns bytes. A stream
    that is not indexable, or a member that does not inflate, raises PcabiError. cap (tests): the
    output capacity offered; a too small one raises ValueError naming the size needed."""
    buf, _ = _gzip_input(data, None)
    L = lib()
    if cap is None:
        idx = bgzf_index(buf)
        size = 0 if idx is None else int(idx[1][-1])
    else:
        size = int(cap)
    out = np.empty(max(size, 1), np.uint8)
    n = L.pcabi_gunzip_host(int(device), _ptr(buf), buf.size, _ptr(out), size)
    if n < 0:
        check(int(n), 'pcabi_gunzip_host')
    if n > size:
        raise ValueError('gunzip: capacity %d, needed %d' % (size, n))
    return out[:n].tobytes()


# ---- gunzip on the device, streams without an index (csrc/pcabi_gzstream.hip) ----------------------
GUNZIP_STREAM_STATS = ('spans', 'cuts', 'confirmed', 'rejected', 'members', 'dev_bytes', 'host_bytes')


def gunzip_stream(data, device=0, cap=None):
    """Any gzip stream (ordinary gzip, multi-member gzip, BGZF) inflated on GPU `device`
    (pcabi_gunzip_stream_host): chunks of the deflate stream decoded in parallel from speculative block
    starts, spans the device cannot take through zlib. Returns bytes, zlib's exactly; a bad stream
    raises PcabiError naming the member, its offset and the status. cap (tests): the output capacity
    offered; a too small one raises ValueError naming the size needed."""
    buf, _ = _gzip_input(data, None)
    L = lib()
    size = max(4 * buf.size, 1 << 16) if cap is None else int(cap)
    while True:
        out = np.empty(max(size, 1), np.uint8)
        n = L.pcabi_gunzip_stream_host(int(device), _ptr(buf), buf.size, _ptr(out), size)
        if n < 0:
            check(int(n), 'pcabi_gunzip_stream_host')
        if n <= size:
            return out[:n].tobytes()
        if cap is not None:
            raise ValueError('gunzip_stream: capacity %d, needed %d' % (size, n))
        size = int(n)


def gunzip_stream_stats():
    """What the last gunzip_stream call, or the reader last read from (misc.read_batches gunzip_plain),
    did on this thread (pcabi_gunzip_stream_last_stats): a dict of spans, chunk cuts, chunks confirmed on
    the chain, rejected candidates, members, bytes decoded on the device, bytes decoded by the host
    fallback."""
    s = np.zeros(len(GUNZIP_STREAM_STATS), np.int64)
    lib().pcabi_gunzip_stream_last_stats(_ptr(s))
    return dict(zip(GUNZIP_STREAM_STATS, (int(x) for x in s)))


# ---- unaligned BAM input (csrc/pcabi_bam.h, csrc/pcabi_bam.hip) ----------------------------------
# include/pcabi.h pcabi_bam_rec
BAM_REC = np.dtype([('rec', np.int64), ('seq_out', np.int64), ('qual_out', np.int64), ('code_out', np.int64),
                    ('tile0', np.int64), ('seq_at', np.int32), ('l_seq', np.int32), ('flag', np.int32),
                    ('name_len', np.int32)])


def bam_index(data):
    """The records of a whole inflated BAM file (pcabi_bam_index): (recs, totals). recs: a BAM_REC
    array of the kept records (secondary and supplementary ones skipped) with their output offsets
    in the batch layout; totals: int64 [5] = sequence bytes, quality bytes, code bytes (16 bytes of
    tail padding included), name bytes, tiles. A bad header, an invalid record or a truncated chain
    raises PcabiError."""
    buf, _ = _gzip_input(data, None)
    L = lib()
    totals = np.zeros(5, np.int64)
    n = L.pcabi_bam_index(_ptr(buf), buf.size, None, 0, _ptr(totals))
    if n < 0:
        check(int(n), 'pcabi_bam_index')
    recs = np.zeros(int(n), BAM_REC)
    if n > 0:
        L.pcabi_bam_index(_ptr(buf), buf.size, _ptr(recs), int(n), _ptr(totals))
    return recs, totals


def bam_unpack(data, recs, totals=None, device=0, out=None):
    """The records of a bam_index table unpacked from the inflated bytes `data` into (seq, qual,
    codes) uint8 arrays in the batch layout (pcabi_bam_unpack_host): on GPU `device`, or with the
    host build of the same code when device < 0. out: three preallocated C-contiguous uint8 arrays
    to fill instead (bytes no record owns keep their values); totals: bam_index's, for the sizes and
    the place of the 16 bytes of tail padding."""
    buf, _ = _gzip_input(data, None)
    recs = np.ascontiguousarray(recs, BAM_REC)
    if totals is None:
        ln = recs['l_seq'].astype(np.int64)
        totals = np.array([ln.sum(), ln.sum(), ((ln + 3) & ~3).sum() + 16, 0, 0], np.int64)
    if out is None:
        out = (np.zeros(int(totals[0]), np.uint8), np.zeros(int(totals[1]), np.uint8), np.zeros(int(totals[2]), np.uint8))
    seq, qual, codes = out
    for a in out:
        if a.dtype != np.uint8 or not a.flags['C_CONTIGUOUS']:
            raise ValueError('bam_unpack: outputs are C-contiguous uint8 arrays')
    rc = lib().pcabi_bam_unpack_host(int(device), _ptr(buf), buf.size, _ptr(recs), recs.size, _ptr(seq), seq.size,
                                     _ptr(qual), qual.size, _ptr(codes), codes.size, int(totals[2]) - 16)
    check(int(rc), 'pcabi_bam_unpack_host')
    return seq, qual, codes


# ---- unaligned BAM output (csrc/pcabi_bam.h, csrc/pcabi_bam.hip) ---------------------------------
# include/pcabi.h pcabi_bam_part
BAM_PART = np.dtype([('seq_src', np.int64), ('qual_src', np.int64), ('side_off', np.int64), ('out', np.int64),
                     ('tile0', np.int64), ('l_seq', np.int32), ('name_len', np.int32), ('aux_len', np.int32),
                     ('reserved', np.int32)])


def bam_pack_plan(parts, out0=0):
    """Output offsets and tiles of a part table (pcabi_bam_pack_plan): fills parts['out'] and
    parts['tile0'] in place for a record chain that starts at out0; returns (the chain's end, tiles).
    parts: a C-contiguous BAM_PART array with the sources, the side offsets and the lengths set."""
    if parts.dtype != BAM_PART or not parts.flags['C_CONTIGUOUS']:
        raise ValueError('bam_pack_plan: parts is a C-contiguous BAM_PART array')
    tiles = np.zeros(1, np.int64)
    end = lib().pcabi_bam_pack_plan(_ptr(parts), parts.size, int(out0), _ptr(tiles))
    if end < 0:
        check(int(end), 'pcabi_bam_pack_plan')
    return int(end), int(tiles[0])


def bam_pack(seq, qual, side, parts, out, device=0):
    """The parts of a planned table laid out as BAM records in `out` (pcabi_bam_pack_host): on GPU
    `device`, or with the host build of the same code when device < 0. seq / qual: the letters and the
    quality characters the parts' sources index; side: the names and aux bytes; out: a C-contiguous
    uint8 array, filled in place (bytes no part owns keep their values) and returned."""
    arrs = [np.ascontiguousarray(np.frombuffer(a, np.uint8) if isinstance(a, (bytes, bytearray)) else a, np.uint8)
            for a in (seq, qual, side)]
    parts = np.ascontiguousarray(parts, BAM_PART)
    if out.dtype != np.uint8 or not out.flags['C_CONTIGUOUS']:
        raise ValueError('bam_pack: out is a C-contiguous uint8 array')
    rc = lib().pcabi_bam_pack_host(int(device), _ptr(arrs[0]), arrs[0].size, _ptr(arrs[1]), arrs[1].size, _ptr(arrs[2]),
                                   arrs[2].size, _ptr(parts), parts.size, _ptr(out), out.size)
    check(int(rc), 'pcabi_bam_pack_host')
    return out


# ---- modification tags remapped onto parts (csrc/pcabi_mods.h, csrc/pcabi_mods.hip) ---------------
# include/pcabi.h pcabi_mods_read, pcabi_mods_part
MODS_READ = np.dtype([('seq_off', np.int64), ('mm_off', np.int64), ('ml_off', np.int64), ('part0', np.int64),
                      ('l_seq', np.int32), ('mm_len', np.int32), ('ml_len', np.int32), ('mn', np.int32),
                      ('n_parts', np.int32), ('flags', np.int32)])
MODS_PART = np.dtype([('out', np.int64), ('read', np.int32), ('s0', np.int32), ('ns', np.int32), ('len', np.int32)])
MODS_OLD_MM, MODS_BAD, MODS_OLD_ML = 1, 2, 4


def _mods_args(seq, tags, reads, name):
    arrs = [np.ascontiguousarray(np.frombuffer(a, np.uint8) if isinstance(a, (bytes, bytearray)) else a, np.uint8)
            for a in (seq, tags)]
    if reads.dtype != MODS_READ or not reads.flags['C_CONTIGUOUS']:
        raise ValueError('%s: reads is a C-contiguous MODS_READ array' % name)
    return arrs


def mods_plan(seq, tags, reads, parts, device=0):
    """The lengths of every part's remapped MM / ML / MN tag bytes and which reads' tags are usable
    (pcabi_mods_plan): on GPU `device`, or with the host build of the same code when device < 0.
    seq: the reads' letters in the reader's orientation; tags: the MM texts and ML values the MODS_READ
    array `reads` indexes; parts: a C-contiguous MODS_PART array with read / s0 / ns set, whose 'len' is
    filled in place. Returns (parts, usable uint8 [n_reads])."""
    seq, tags = _mods_args(seq, tags, reads, 'mods_plan')
    if parts.dtype != MODS_PART or not parts.flags['C_CONTIGUOUS']:
        raise ValueError('mods_plan: parts is a C-contiguous MODS_PART array')
    usable = np.zeros(reads.size, np.uint8)
    rc = lib().pcabi_mods_plan(int(device), _ptr(seq), seq.size, _ptr(tags), tags.size, _ptr(reads), reads.size, _ptr(parts),
                               parts.size, _ptr(usable))
    check(int(rc), 'pcabi_mods_plan')
    return parts, usable


def mods_remap(seq, tags, reads, parts, out, device=0):
    """Every part's tag bytes written to out[part.out, part.out + part.len) (pcabi_mods_remap): parts
    as mods_plan left them, with 'out' set; out: a C-contiguous uint8 array, filled in place (bytes no
    part owns keep their values) and returned."""
    seq, tags = _mods_args(seq, tags, reads, 'mods_remap')
    parts = np.ascontiguousarray(parts, MODS_PART)
    if out.dtype != np.uint8 or not out.flags['C_CONTIGUOUS']:
        raise ValueError('mods_remap: out is a C-contiguous uint8 array')
    rc = lib().pcabi_mods_remap(int(device), _ptr(seq), seq.size, _ptr(tags), tags.size, _ptr(reads), reads.size, _ptr(parts),
                                parts.size, _ptr(out), out.size)
    check(int(rc), 'pcabi_mods_remap')
    return out


def mods_counts(reset=False):
    """(reads whose modification tags were remapped, reads whose tags were dropped as not usable) since
    the last reset (pcabi_mods_counts)."""
    v = np.zeros(2, np.int64)
    lib().pcabi_mods_counts(int(bool(reset)), _ptr(v[0:1]), _ptr(v[1:2]))
    return int(v[0]), int(v[1])


# ---- move tables remapped onto parts (csrc/pcabi_moves.h, csrc/pcabi_moves.hip) ---------------------
# include/pcabi.h pcabi_moves_read (40 bytes: 4 of padding at its end), pcabi_moves_part
MOVES_READ = np.dtype([('mv_off', np.int64), ('part0', np.int64), ('l_seq', np.int32), ('n_vals', np.int32), ('ts', np.int32),
                       ('n_parts', np.int32), ('flags', np.int32)], align=True)
MOVES_PART = np.dtype([('out', np.int64), ('read', np.int32), ('s0', np.int32), ('ns', np.int32), ('len', np.int32)])
MOVES_BAD = 1
assert MOVES_READ.itemsize == 40 and MOVES_PART.itemsize == 24


def _moves_args(tags, reads, name):
    tags = np.ascontiguousarray(np.frombuffer(tags, np.uint8) if isinstance(tags, (bytes, bytearray)) else tags, np.uint8)
    if reads.dtype != MOVES_READ or not reads.flags['C_CONTIGUOUS']:
        raise ValueError('%s: reads is a C-contiguous MOVES_READ array' % name)
    return tags


def moves_plan(tags, reads, parts, device=0):
    """The lengths of every part's remapped mv / ts tag bytes and which reads' move tables are usable
    (pcabi_moves_plan): on GPU `device`, or with the host build of the same code when device < 0. tags:
    the bytes the MOVES_READ array `reads` indexes (mv_off: a table's first value, its stride); parts: a
    C-contiguous MOVES_PART array with read / s0 / ns set, whose 'len' is filled in place. Returns
    (parts, usable uint8 [n_reads])."""
    tags = _moves_args(tags, reads, 'moves_plan')
    if parts.dtype != MOVES_PART or not parts.flags['C_CONTIGUOUS']:
        raise ValueError('moves_plan: parts is a C-contiguous MOVES_PART array')
    usable = np.zeros(reads.size, np.uint8)
    rc = lib().pcabi_moves_plan(int(device), _ptr(tags), tags.size, _ptr(reads), reads.size, _ptr(parts), parts.size, _ptr(usable))
    check(int(rc), 'pcabi_moves_plan')
    return parts, usable


def moves_remap(tags, reads, parts, out, device=0):
    """Every part's tag bytes (mv, then ts) written to out[part.out, part.out + part.len)
    (pcabi_moves_remap): parts as moves_plan left them, with 'out' set; out: a C-contiguous uint8 array,
    filled in place (bytes no part owns keep their values) and returned."""
    tags = _moves_args(tags, reads, 'moves_remap')
    parts = np.ascontiguousarray(parts, MOVES_PART)
    if out.dtype != np.uint8 or not out.flags['C_CONTIGUOUS']:
        raise ValueError('moves_remap: out is a C-contiguous uint8 array')
    rc = lib().pcabi_moves_remap(int(device), _ptr(tags), tags.size, _ptr(reads), reads.size, _ptr(parts), parts.size, _ptr(out),
                                 out.size)
    check(int(rc), 'pcabi_moves_remap')
    return out


def moves_counts(reset=False):
    """(reads whose move table was remapped, reads whose mv was dropped as not usable) since the last
    reset (pcabi_moves_counts)."""
    v = np.zeros(2, np.int64)
    lib().pcabi_moves_counts(int(bool(reset)), _ptr(v[0:1]), _ptr(v[1:2]))
    return int(v[0]), int(v[1])


# ---- SAM tags in FASTQ / FASTA headers (csrc/pcabi_auxtext.h, csrc/pcabi_auxtext.hip) ---------------
# include/pcabi.h pcabi_auxtext_part, pcabi_fastx_part
AUXTEXT_PART = np.dtype([('aux_off', np.int64), ('out', np.int64), ('len', np.int64), ('aux_len', np.int32),
                         ('reserved', np.int32)])
FASTX_PART = np.dtype([('seq_src', np.int64), ('qual_src', np.int64), ('name_off', np.int64), ('aux_off', np.int64),
                       ('text_len', np.int64), ('out', np.int64), ('tile0', np.int64), ('l_seq', np.int32),
                       ('l_qual', np.int32), ('name_len', np.int32), ('aux_len', np.int32), ('flags', np.int32),
                       ('reserved', np.int32)])
FASTX_RNA = 1
assert AUXTEXT_PART.itemsize == 32 and FASTX_PART.itemsize == 80


def _bytes_arg(a):
    return np.ascontiguousarray(np.frombuffer(a, np.uint8) if isinstance(a, (bytes, bytearray)) else a, np.uint8)


def auxtext_plan(aux, parts, device=0):
    """The length of every chain's SAM text (pcabi_auxtext_plan): on GPU `device`, or with the host
    build of the same code when device < 0. aux: the bytes the C-contiguous AUXTEXT_PART array `parts`
    indexes (aux_off / aux_len set); 'len' is filled in place, -1 for a chain that does not walk.
    Adds the tags to auxtext_counts(). Returns parts."""
    aux = _bytes_arg(aux)
    if parts.dtype != AUXTEXT_PART or not parts.flags['C_CONTIGUOUS']:
        raise ValueError('auxtext_plan: parts is a C-contiguous AUXTEXT_PART array')
    rc = lib().pcabi_auxtext_plan(int(device), _ptr(aux), aux.size, _ptr(parts), parts.size)
    check(int(rc), 'pcabi_auxtext_plan')
    return parts


def auxtext_write(aux, parts, out, device=0):
    """Every chain's text written to out[part.out, part.out + part.len) (pcabi_auxtext_write): parts as
    auxtext_plan left them, with 'out' set; out: a C-contiguous uint8 array, filled in place (bytes no
    part owns keep their values) and returned."""
    aux = _bytes_arg(aux)
    parts = np.ascontiguousarray(parts, AUXTEXT_PART)
    if out.dtype != np.uint8 or not out.flags['C_CONTIGUOUS']:
        raise ValueError('auxtext_write: out is a C-contiguous uint8 array')
    rc = lib().pcabi_auxtext_write(int(device), _ptr(aux), aux.size, _ptr(parts), parts.size, _ptr(out), out.size)
    check(int(rc), 'pcabi_auxtext_write')
    return out


def auxtext_counts(reset=False):
    """(tags written as text, tags left out) since the last reset (pcabi_auxtext_counts)."""
    v = np.zeros(2, np.int64)
    lib().pcabi_auxtext_counts(int(bool(reset)), _ptr(v[0:1]), _ptr(v[1:2]))
    return int(v[0]), int(v[1])


def aux_text(aux_chains, device=None):
    """The SAM text of each aux chain (a list of bytes): tab-separated TG:T:value fields, b'' for a
    chain without tags, None for a chain that does not walk. device None or < 0: the host build."""
    dev = -1 if device is None else int(device)
    chains = [bytes(c) for c in aux_chains]
    parts = np.zeros(len(chains), AUXTEXT_PART)
    parts['aux_len'] = [len(c) for c in chains]
    parts['aux_off'][1:] = np.cumsum(parts['aux_len'][:-1], dtype=np.int64)
    blob = b''.join(chains)
    auxtext_plan(blob, parts, dev)
    lens = np.maximum(parts['len'], 0)
    parts['out'][1:] = np.cumsum(lens[:-1], dtype=np.int64)
    out = np.zeros(int(lens.sum()), np.uint8)
    auxtext_write(blob, parts, out, dev)
    buf = out.tobytes()
    return [None if p['len'] < 0 else buf[int(p['out']):int(p['out']) + int(p['len'])] for p in parts]


def fastx_pack_plan(parts, fasta=False, out0=0):
    """Output offsets and tiles of a FASTX_PART table (pcabi_fastx_pack_plan): fills parts['out'] and
    parts['tile0'] in place for records that start at out0; returns (the end, tiles)."""
    if parts.dtype != FASTX_PART or not parts.flags['C_CONTIGUOUS']:
        raise ValueError('fastx_pack_plan: parts is a C-contiguous FASTX_PART array')
    tiles = np.zeros(1, np.int64)
    end = lib().pcabi_fastx_pack_plan(_ptr(parts), parts.size, int(bool(fasta)), int(out0), _ptr(tiles))
    if end < 0:
        check(int(end), 'pcabi_fastx_pack_plan')
    return int(end), int(tiles[0])


def fastx_pack(seq, qual, side, parts, out, fasta=False, device=0):
    """The parts of a planned table laid out as FASTQ / FASTA records in `out`, their aux chains' SAM
    text in the headers (pcabi_fastx_pack_host): on GPU `device`, or with the host build of the same
    code when device < 0. side: the names and the aux chains; out: a C-contiguous uint8 array, filled
    in place (bytes no part owns keep their values) and returned."""
    arrs = [_bytes_arg(a) for a in (seq, qual, side)]
    parts = np.ascontiguousarray(parts, FASTX_PART)
    if out.dtype != np.uint8 or not out.flags['C_CONTIGUOUS']:
        raise ValueError('fastx_pack: out is a C-contiguous uint8 array')
    rc = lib().pcabi_fastx_pack_host(int(device), _ptr(arrs[0]), arrs[0].size, _ptr(arrs[1]), arrs[1].size, _ptr(arrs[2]),
                                     arrs[2].size, _ptr(parts), parts.size, int(bool(fasta)), _ptr(out), out.size)
    check(int(rc), 'pcabi_fastx_pack_host')
    return out


# ---- SAM tags read from FASTQ / FASTA headers (csrc/pcabi_auxparse.h, csrc/pcabi_auxparse.hip) ---------
# include/pcabi.h pcabi_auxparse_part
AUXPARSE_PART = np.dtype([('text_off', np.int64), ('out', np.int64), ('len', np.int64), ('text_len', np.int64),
                          ('n_float', np.int32), ('tags', np.int32), ('left_out', np.int32), ('reserved', np.int32)])
assert AUXPARSE_PART.itemsize == 48


def auxparse_plan(text, parts, device=0):
    """The length of every header's chain of aux bytes (pcabi_auxparse_plan): on GPU `device`, or with
    the host build of the same rule when device < 0. text: the bytes the C-contiguous AUXPARSE_PART
    array `parts` indexes (text_off / text_len set); 'len', 'n_float', 'tags' and 'left_out' are filled
    in place. Adds the tags and the left-out fields to auxparse_counts(). Returns parts."""
    text = _bytes_arg(text)
    if parts.dtype != AUXPARSE_PART or not parts.flags['C_CONTIGUOUS']:
        raise ValueError('auxparse_plan: parts is a C-contiguous AUXPARSE_PART array')
    rc = lib().pcabi_auxparse_plan(int(device), _ptr(text), text.size, _ptr(parts), parts.size)
    check(int(rc), 'pcabi_auxparse_plan')
    return parts


def auxparse_write(text, parts, out, device=0):
    """Every header's chain written to out[part.out, part.out + part.len) (pcabi_auxparse_write): parts
    as auxparse_plan left them, with 'out' set; out: a C-contiguous uint8 array, filled in place (bytes
    no part owns keep their values) and returned."""
    text = _bytes_arg(text)
    parts = np.ascontiguousarray(parts, AUXPARSE_PART)
    if out.dtype != np.uint8 or not out.flags['C_CONTIGUOUS']:
        raise ValueError('auxparse_write: out is a C-contiguous uint8 array')
    rc = lib().pcabi_auxparse_write(int(device), _ptr(text), text.size, _ptr(parts), parts.size, _ptr(out), out.size)
    check(int(rc), 'pcabi_auxparse_write')
    return out


def auxparse_counts(reset=False):
    """(tags read, fields left out) since the last reset (pcabi_auxparse_counts)."""
    v = np.zeros(2, np.int64)
    lib().pcabi_auxparse_counts(int(bool(reset)), _ptr(v[0:1]), _ptr(v[1:2]))
    return int(v[0]), int(v[1])


def aux_parse(headers, device=None):
    """The chain of BAM aux bytes of each header (bytes: the text after '@' / '>', or a single header
    instead of a list): the tab-separated TG:T:value fields behind the first tab, b'' for a header
    without tags. device None or < 0: the host build."""
    if isinstance(headers, (bytes, bytearray)):
        return aux_parse([headers], device)[0]
    dev = -1 if device is None else int(device)
    heads = [bytes(h) for h in headers]
    parts = np.zeros(len(heads), AUXPARSE_PART)
    parts['text_len'] = [len(h) for h in heads]
    parts['text_off'][1:] = np.cumsum(parts['text_len'][:-1], dtype=np.int64)
    blob = b''.join(heads)
    auxparse_plan(blob, parts, dev)
    parts['out'][1:] = np.cumsum(parts['len'][:-1], dtype=np.int64)
    out = np.zeros(int(parts['len'].sum()), np.uint8)
    auxparse_write(blob, parts, out, dev)
    buf = out.tobytes()
    return [buf[int(p['out']):int(p['out']) + int(p['len'])] for p in parts]


# ---- quality stage: end crop and read filter (csrc/pcabi_qual.h, csrc/pcabi_qual.hip) ---------------
# include/pcabi.h pcabi_qual_read, pcabi_qual_opts
QUAL_READ = np.dtype([('front', np.int32), ('tail', np.int32), ('kept', np.int32), ('flags', np.int32), ('q_sum', np.int64),
                      ('err_sum', np.uint64)])
QUAL_OPTS = np.dtype([('window', np.int32), ('reserved', np.int32), ('min_window_sum', np.int64), ('min_length', np.int64),
                      ('max_length', np.int64), ('max_mean_err', np.uint64)])
QUAL_TOO_SHORT, QUAL_TOO_LONG, QUAL_LOW_QUALITY, QUAL_NO_QUALITIES = 1, 2, 4, 8
QUAL_FAIL = QUAL_TOO_SHORT | QUAL_TOO_LONG | QUAL_LOW_QUALITY
assert QUAL_READ.itemsize == 32 and QUAL_OPTS.itemsize == 40


def qual_error_table():
    """E[q] = round(2^32 * 10^(-q / 10)) for q = 0..93 as the library holds it (pcabi_qual_error_table)."""
    t = np.zeros(94, np.uint64)
    lib().pcabi_qual_error_table(_ptr(t))
    return t


def qual_opts(window=0, min_window_q=0.0, min_length=0, max_length=0, min_mean_q=0.0):
    """The thresholds as the integers the library takes (a QUAL_OPTS record): min_window_sum =
    ceil(min_window_q * window); max_mean_err = floor(2^32 * 10^(-min_mean_q / 10)), the mean error
    probability that mean quality stands for (min_mean_q <= 0: 2^32, no test). The only place where the
    thresholds are converted."""
    import math
    o = np.zeros(1, QUAL_OPTS)
    o['window'] = int(window)
    o['min_window_sum'] = int(math.ceil(float(min_window_q) * int(window)))
    o['min_length'], o['max_length'] = int(min_length), int(max_length)
    o['max_mean_err'] = 1 << 32 if min_mean_q <= 0 else int(math.floor(2.0 ** 32 * 10.0 ** (-float(min_mean_q) / 10.0)))
    return o


def quality_filter(qual, span_off, span_len, window=0, min_window_q=0.0, min_length=0, max_length=0, min_mean_q=0.0, device=0,
                   opts=None):
    """Every read's span cropped at both ends to its outermost windows of `window` qualities whose mean
    Phred is min_window_q or more, then its length and mean-quality tests (pcabi_qual_filter_host; the
    rule: include/pcabi.h). qual: the quality bytes; span_off / span_len: every read's span in them,
    span_off < 0 for a read without qualities. On GPU `device`, or with the host build of the same code
    when device is None or < 0. opts: a QUAL_OPTS record that replaces the thresholds (the integers as
    they are). Returns a QUAL_READ array: front, tail, kept, flags (QUAL_*), q_sum, err_sum."""
    qual = _bytes_arg(qual)
    span_off = np.ascontiguousarray(span_off, np.int64)
    span_len = np.ascontiguousarray(span_len, np.int32)
    if span_off.shape != span_len.shape or span_off.ndim != 1:
        raise ValueError('quality_filter: span_off and span_len are one-dimensional and equally long')
    if opts is None:
        opts = qual_opts(window, min_window_q, min_length, max_length, min_mean_q)
    opts = np.ascontiguousarray(opts, QUAL_OPTS)
    out = np.zeros(span_off.size, QUAL_READ)
    rc = lib().pcabi_qual_filter_host(-1 if device is None else int(device), _ptr(qual), qual.size, _ptr(span_off), _ptr(span_len),
                                      span_off.size, _ptr(opts), _ptr(out))
    check(int(rc), 'pcabi_qual_filter_host')
    return out


# include/pcabi.h pcabi_qual_piece
QUAL_PIECE = np.dtype([('read', np.int64), ('begin', np.int64), ('end', np.int64), ('q', QUAL_READ)])
assert QUAL_PIECE.itemsize == 56


def quality_pieces_bound(span_len, cut_off):
    """The host-side bounds of the piece stage (pcabi_qual_pieces_bound): (pieces, segments)."""
    span_len = np.ascontiguousarray(span_len, np.int32)
    cut_off = np.ascontiguousarray(cut_off, np.int64)
    if cut_off.ndim != 1 or cut_off.size != span_len.size + 1:
        raise ValueError('quality_pieces_bound: cut_off holds one entry more than there are reads')
    out = np.zeros(2, np.int64)
    check(int(lib().pcabi_qual_pieces_bound(_ptr(span_len), _ptr(cut_off), span_len.size, out[0:].ctypes.data, out[1:].ctypes.data)),
          'pcabi_qual_pieces_bound')
    return int(out[0]), int(out[1])


def quality_filter_pieces(qual, span_off, span_len, cut_off, cuts, window=0, min_window_q=0.0, min_length=0, max_length=0,
                          min_mean_q=0.0, device=0, opts=None):
    """The split reads of a batch judged piece by piece (pcabi_qual_pieces_host; the rule: include/pcabi.h).
    qual / span_off / span_len as quality_filter takes them (span_len: the trimmed lengths); cut_off / cuts:
    the reads' ranges in the writers' layout (int64 [n + 1], int64 [2 * cut_off[n]]). Every piece the
    writers would cut a split read into is cropped and tested like a read of its own. On GPU `device`, or
    with the host build when device is None or < 0. Returns (cut_off', cuts', pieces, piece_off): the cut
    layout that makes every writer emit exactly the cropped, passing pieces; a QUAL_PIECE array (read,
    begin, end, q: a QUAL_READ record); piece_off int64 [n + 1], read r's pieces being
    pieces[piece_off[r]:piece_off[r + 1]]."""
    qual = _bytes_arg(qual)
    span_off = np.ascontiguousarray(span_off, np.int64)
    span_len = np.ascontiguousarray(span_len, np.int32)
    cut_off = np.ascontiguousarray(cut_off, np.int64)
    cuts = np.ascontiguousarray(cuts, np.int64).reshape(-1)
    n = span_off.size
    if span_off.shape != span_len.shape or span_off.ndim != 1:
        raise ValueError('quality_filter_pieces: span_off and span_len are one-dimensional and equally long')
    if cut_off.ndim != 1 or cut_off.size != n + 1 or int(cut_off[-1]) * 2 != cuts.size:
        raise ValueError('quality_filter_pieces: cut_off holds n + 1 entries and cuts two values a range')
    if opts is None:
        opts = qual_opts(window, min_window_q, min_length, max_length, min_mean_q)
    opts = np.ascontiguousarray(opts, QUAL_OPTS)
    cap, _ = quality_pieces_bound(span_len, cut_off)
    n_ranges = cuts.size // 2
    piece_off, cut_off2 = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    pieces, cuts2 = np.zeros(cap, QUAL_PIECE), np.zeros(2 * (n_ranges + 2 * cap), np.int64)
    rc = lib().pcabi_qual_pieces_host(-1 if device is None else int(device), _ptr(qual), qual.size, _ptr(span_off), _ptr(span_len), n,
                                      _ptr(cut_off), _ptr(cuts), _ptr(opts), _ptr(piece_off), _ptr(pieces), cap, _ptr(cut_off2),
                                      _ptr(cuts2), n_ranges + 2 * cap)
    check(int(rc), 'pcabi_qual_pieces_host')
    n_pieces = int(piece_off[n])
    return cut_off2, cuts2[:2 * int(cut_off2[n])].copy(), pieces[:n_pieces].copy(), piece_off
