"""ctypes access to a host build of csrc/pcabi_gzstream.h (tests/gzstream_cpu.cpp), and the stream
corpora the CPU and GPU tests of the parallel gzip decoder share. Every expected byte comes from
Python's zlib / gzip. TEST INFRASTRUCTURE ONLY."""
import ctypes
import glob
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, '_gzstream_cpu.so')
CSRC = os.path.join(os.path.dirname(HERE), 'custom_porechop_abi_amd', 'csrc')
DEPS = [os.path.join(CSRC, n) for n in ('pcabi_gzstream.h', 'pcabi_inflate.h', 'pcabi_deflate.h', 'pcabi_crc.h')] + \
    [os.path.join(os.path.dirname(HERE), 'include', 'pcabi.h')]
GOLDEN_GZ = sorted(glob.glob(os.path.join(HERE, 'golden', 'data', '*.gz')))
E_PARSE = -4
GUARD = 64
STATS = ('spans', 'cuts', 'confirmed', 'rejected', 'members', 'dev_bytes', 'host_bytes')
CAND_DYN, CAND_MEMBER = 1, 2

_lib = None


def build():
    src = os.path.join(HERE, 'gzstream_cpu.cpp')
    if not os.path.isfile(SO) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in [src] + DEPS):
        tmp = '%s.%d.tmp' % (SO, os.getpid())
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-Wall', '-o', tmp, src, '-lz'])
        os.replace(tmp, SO)
    return SO


def load():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build())
        P, i64 = ctypes.c_void_p, ctypes.c_int64
        L.gzs_stream.argtypes = [P, i64, i64, i64, i64, P, i64, P, P]
        L.gzs_stream.restype = i64
        L.gzs_quick_dynamic.argtypes = [P, i64, i64]
        L.gzs_find.argtypes = [P, i64, i64, i64, P]
        L.gzs_blocks.argtypes = [P, i64, i64, i64, ctypes.c_uint32, P, ctypes.c_uint32, P, P, P]
        L.gzs_resolve.argtypes = [P, i64, P, P, P]
        L.gzs_resolve.restype = None
        _lib = L
    return _lib


def _arr(data):
    return np.frombuffer(data, np.uint8) if len(data) else np.zeros(1, np.uint8)


def stream(data, chunk_bytes, span_bytes=1 << 20, min_chunks=0, cap=None):
    """The stream through the host build: (bytes, stats dict), or (error message, stats dict, bytes
    decoded before the error) when it is refused. Guard bytes around the output are checked."""
    L = load()
    z = _arr(data)
    cap = 16 * len(data) + (4 << 20) if cap is None else cap
    out = np.full(cap + 2 * GUARD, 0xA5, np.uint8)
    stats = np.zeros(8, np.int64)
    msg = ctypes.create_string_buffer(256)
    n = L.gzs_stream(z.ctypes.data, len(data), chunk_bytes, span_bytes, min_chunks, out.ctypes.data + GUARD, cap,
                     stats.ctypes.data, msg)
    assert (out[:GUARD] == 0xA5).all() and (out[GUARD + cap:] == 0xA5).all(), 'wrote outside the output range'
    st = dict(zip(STATS, (int(x) for x in stats[:7])))
    if n < 0:
        assert n == E_PARSE
        return msg.value.decode(), st, out[GUARD:GUARD + int(stats[7])].tobytes()
    if n > cap:   # the needed length; nothing written
        assert (out == 0xA5).all()
        return int(n), st
    return out[GUARD:GUARD + n].tobytes(), st


def find(data, lo, hi):
    """(kind, decoder start bit) of the first candidate in the bit range [lo, hi)."""
    z = _arr(data)
    pos = ctypes.c_int64(-1)
    kind = load().gzs_find(z.ctypes.data, len(data), lo, hi, ctypes.addressof(pos))
    return kind, pos.value


def blocks(data, start_bit, stop_bit, hist, cap, marker=True):
    """Blocks from start_bit to the first boundary at or past stop_bit: (status, symbols or None,
    produced, end bit, final)."""
    z = _arr(data)
    sym = np.zeros(cap + 1, np.uint16)
    produced, end_bit, fin = ctypes.c_uint32(0), ctypes.c_int64(0), ctypes.c_int(0)
    st = load().gzs_blocks(z.ctypes.data, len(data), start_bit, stop_bit, hist, sym.ctypes.data if marker else None, cap,
                           ctypes.addressof(produced), ctypes.addressof(end_bit), ctypes.addressof(fin))
    return st, (sym[:produced.value] if marker else None), produced.value, end_bit.value, fin.value


def resolve(sym, win):
    """(bytes, the window after them) of symbols through a 32768-byte window."""
    sym = np.ascontiguousarray(sym, np.uint16)
    win = np.frombuffer(win, np.uint8)
    assert win.size == 32768
    out, nxt = np.zeros(max(sym.size, 1), np.uint8), np.zeros(32768, np.uint8)
    load().gzs_resolve(sym.ctypes.data, sym.size, win.ctypes.data, out.ctypes.data, nxt.ctypes.data)
    return out[:sym.size].tobytes(), nxt.tobytes()


# ---- corpora -----------------------------------------------------------------------------------------
_text = None


def text():
    """About 650 KB of FASTQ-like text: 300 records of 200 to 2000 bases over ACGT, qualities uniform
    in 35..69, seeded."""
    global _text
    if _text is None:
        rng = np.random.RandomState(11)
        out = []
        for k in range(300):
            ln = int(rng.randint(200, 2001))
            out.append(b'@read_%d runid=0123abcd ch=%d\n' % (k, k % 512) + bytes(rng.choice(list(b'ACGT'), ln).astype(np.uint8)) +
                       b'\n+\n' + bytes(rng.randint(35, 70, ln).astype(np.uint8)) + b'\n')
        _text = b''.join(out)
    return _text


def gz(data, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=31):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, mem, strategy)
    return c.compress(data) + c.flush()


def chunk_for(mem):
    return 4096 if mem == 1 else 32768


TEXT_SETTINGS = [(6, 8), (6, 1), (1, 1), (9, 3)]


def history_streams():
    """[(name, stream, data, chunk_bytes)]: matches that run across chunk boundaries."""
    rng = np.random.RandomState(5)
    block = bytes(rng.randint(0, 256, 32768).astype(np.uint8))
    out = []
    for mem in (1, 8):
        out.append(('rand32k-x8-mem%d' % mem, gz(block * 8, 9, mem), block * 8, chunk_for(mem)))
    out.append(('A-200000', gz(b'A' * 200000, 6, 1), b'A' * 200000, 4096))
    out.append(('AB-100000', gz(b'AB' * 100000, 6, 1), b'AB' * 100000, 4096))
    out.append(('zeros-3MiB', gz(bytes(3 << 20), 9, 8), bytes(3 << 20), 32768))
    return out


def raw_piece(data, level, mem, strategy, flush):
    """A raw deflate piece from a compressor of its own, ended by `flush`: after Z_SYNC_FLUSH / Z_FULL_FLUSH
    it is byte-aligned and not final, so pieces concatenate into one deflate stream."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    return c.compress(data) + c.flush(flush)


def wrap(raw, data):
    """The gzip member of a raw deflate stream that decodes to data."""
    return bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3]) + raw + struct.pack('<II', zlib.crc32(data), len(data) & 0xffffffff)


def mixed_flush_stream():
    """One stream that changes level and strategy between Z_FULL_FLUSH and Z_SYNC_FLUSH calls: empty
    stored blocks after headers that end inside a byte."""
    t = text()
    steps = [(6, zlib.Z_DEFAULT_STRATEGY, zlib.Z_FULL_FLUSH), (1, zlib.Z_HUFFMAN_ONLY, zlib.Z_SYNC_FLUSH),
             (9, zlib.Z_RLE, zlib.Z_FULL_FLUSH), (0, zlib.Z_DEFAULT_STRATEGY, zlib.Z_SYNC_FLUSH),
             (6, zlib.Z_FIXED, zlib.Z_SYNC_FLUSH), (6, zlib.Z_DEFAULT_STRATEGY, zlib.Z_FULL_FLUSH)]
    piece, n = 20011, 12
    raw = b''
    for k in range(n):
        level, strat, fl = steps[k % len(steps)]
        raw += raw_piece(t[k * piece:(k + 1) * piece], level, 1, strat, fl if k + 1 < n else zlib.Z_FINISH)
    return wrap(raw, t[:n * piece]), t[:n * piece]


def block_type_streams():
    """[(name, stream, data, chunk_bytes)]: stored, fixed, Huffman-only and RLE blocks, and the mixed one."""
    t = text()[:300000]
    out = [('stored', gz(t, 0, 1), t, 4096), ('fixed', gz(t, 6, 1, zlib.Z_FIXED), t, 4096),
           ('huffman-only', gz(t, 6, 1, zlib.Z_HUFFMAN_ONLY), t, 4096), ('rle', gz(t, 6, 1, zlib.Z_RLE), t, 4096)]
    s, d = mixed_flush_stream()
    out.append(('mixed-flush', s, d, 4096))
    return out


def hand_member(data, fname=None, extra=None, fhcrc=False, flg_or=0):
    """A gzip member built by hand: FNAME / FEXTRA / FHCRC as asked."""
    flg = (8 if fname is not None else 0) | (4 if extra is not None else 0) | (2 if fhcrc else 0) | flg_or
    h = bytes([0x1f, 0x8b, 8, flg, 0, 0, 0, 0, 0, 3])
    if extra is not None:
        h += struct.pack('<H', len(extra)) + extra
    if fname is not None:
        h += fname + b'\0'
    if fhcrc:
        h += struct.pack('<H', zlib.crc32(h) & 0xffff)
    return h + gz(data, 6, 1, wbits=-15) + struct.pack('<II', zlib.crc32(data), len(data) & 0xffffffff)


def member_streams():
    """[(name, stream, data, members)]: concatenated members of every size and header shape."""
    t = text()
    parts = [b'', t[:700], t[700:150000], b'x', t[150000:150900], t[150900:400000]]
    s = b''.join(gzip.compress(p) if k % 2 else gz(p, 6, 1) for k, p in enumerate(parts))
    out = [('sizes', s, b''.join(parts), len(parts))]
    s = hand_member(t[:90000], fname=b'reads.fastq') + hand_member(t[90000:200000], extra=b'XY\x03\x00abc', fhcrc=True) + \
        gzip.compress(b'')
    out.append(('headers', s, t[:200000], 3))
    return out


def false_candidate_stream(chunk_bytes=4096, copies=4):
    """Copies of a raw deflate stream A (20 KB of the text at (6, 1): several non-final dynamic blocks,
    and its first bytes are a valid dynamic block header) inside a payload that is compressed at
    level 0 between two level-6 sections of the text, Z_FULL_FLUSH between the sections. The padding
    before every copy is chosen so that the copy lies byte-aligned in a stored block and starts within
    64 bytes after a multiple of chunk_bytes of the compressed position. Returns (stream, data,
    compressed offsets of the copies)."""
    t = text()
    a = gz(t[:20000], 6, 1, wbits=-15)
    head = bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3]) + raw_piece(t[:120000], 6, 1, zlib.Z_DEFAULT_STRATEGY, zlib.Z_FULL_FLUSH)
    pads = [3 * chunk_bytes] * copies

    def build():
        payload = b''.join(b'N' * p + a for p in pads)
        return payload, raw_piece(payload, 0, 8, zlib.Z_DEFAULT_STRATEGY, zlib.Z_FULL_FLUSH)

    def places(mid):
        out, at = [], 0
        for _ in range(copies):
            at = mid.find(a, at)
            out.append(len(head) + at if at >= 0 else -1)
            if at < 0:
                break
            at += len(a)
        return out

    for j in range(copies):
        for _ in range(12):
            payload, mid = build()
            pos = places(mid)
            if len(pos) > j and pos[j] >= 0 and 0 < pos[j] % chunk_bytes <= 64:
                break
            if len(pos) <= j or pos[j] < 0:
                pads[j] += 997          # the copy straddles a stored block's header: move it
            else:
                pads[j] += (8 - pos[j]) % chunk_bytes
        else:
            raise AssertionError('no placement for copy %d' % j)
    payload, mid = build()
    data = t[:120000] + payload + t[120000:240000]
    tail = raw_piece(t[120000:240000], 6, 1, zlib.Z_DEFAULT_STRATEGY, zlib.Z_FINISH)
    return head + mid + tail + struct.pack('<II', zlib.crc32(data), len(data)), data, places(mid)


def error_streams():
    """[(name, stream)] from the text at (6, 1): every one makes zlib raise."""
    s = gz(text(), 6, 1)
    out = [('cut-%d' % k, s[:-k]) for k in (1, 5, 9, 4000)]
    for name, at in (('first', 2000), ('middle', len(s) // 2), ('last', len(s) - 1500)):
        b = bytearray(s)
        b[at] ^= 0x10
        out.append(('flip-' + name, bytes(b)))
    out.append(('crc', s[:-8] + struct.pack('<I', struct.unpack('<I', s[-8:-4])[0] ^ 1) + s[-4:]))
    out.append(('isize', s[:-4] + struct.pack('<I', len(text()) + 1)))
    out.append(('reserved-flag', s + hand_member(b'second member', flg_or=0x20)))
    return out


def zlib_prefix(data):
    """The bytes zlib hands out before it raises on a damaged single-member stream."""
    d = zlib.decompressobj(31)
    out = []
    try:
        for at in range(0, len(data), 512):
            out.append(d.decompress(data[at:at + 512]))
    except zlib.error:
        pass
    return b''.join(out)


def zlib_all(data):
    """What zlib makes of a whole gzip stream, member after member, as gzread does: the bytes, or
    raises zlib.error (also for a stream that ends early). Bytes after the last member that do not
    start with the magic are ignored."""
    out = []
    first = True
    while data:
        if not first and data[:2] != b'\x1f\x8b':
            break
        d = zlib.decompressobj(31)
        out.append(d.decompress(data))
        if not d.eof:
            raise zlib.error('stream ends early')
        data = d.unused_data
        first = False
    return b''.join(out)


def zlib_members(data):
    """How many members zlib finds in a gzip stream."""
    m = 0
    while data[:2] == b'\x1f\x8b':
        d = zlib.decompressobj(31)
        d.decompress(data)
        assert d.eof
        data = d.unused_data
        m += 1
    return m
