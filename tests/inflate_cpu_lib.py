"""ctypes access to a host build of csrc/pcabi_inflate.h (tests/inflate_cpu.cpp), and the member
corpora the CPU and GPU inflate tests share. TEST INFRASTRUCTURE ONLY."""
import ctypes
import os
import struct
import subprocess
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, '_inflate_cpu.so')
CSRC = os.path.join(os.path.dirname(HERE), 'custom_porechop_abi_amd', 'csrc')
DEPS = [os.path.join(CSRC, n) for n in ('pcabi_inflate.h', 'pcabi_deflate.h', 'pcabi_crc.h')] + \
    [os.path.join(os.path.dirname(HERE), 'include', 'pcabi.h')]

E_HEADER, E_CODE, E_DIST, E_INPUT, E_OUTPUT, E_LENGTH, E_CRC = range(1, 8)
E_PARSE = -4
EOF_MARKER = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')
GUARD = 64

_lib = None


def build():
    src = os.path.join(HERE, 'inflate_cpu.cpp')
    if not os.path.isfile(SO) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in [src] + DEPS):
        tmp = '%s.%d.tmp' % (SO, os.getpid())
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-Wall', '-o', tmp, src])
        os.replace(tmp, SO)
    return SO


def load():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build())
        P = ctypes.c_void_p
        L.infl_member.argtypes = [P, ctypes.c_int64, P, ctypes.c_uint32, P]
        L.infl_member.restype = ctypes.c_int
        L.infl_index.argtypes = [P, ctypes.c_int64, P, P, ctypes.c_int64]
        L.infl_index.restype = ctypes.c_int64
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def inflate_member(member, cap=None):
    """One gzip member through the host decoder, input and output between guard bytes that are
    checked. Returns (status, bytes or None)."""
    L = load()
    isize = struct.unpack('<I', member[-4:])[0] if len(member) >= 4 else 0
    cap = min(isize, 65536) if cap is None else cap
    zin = np.full(len(member) + 2 * GUARD, 0x5A, np.uint8)
    zin[GUARD:GUARD + len(member)] = np.frombuffer(member, np.uint8)
    keep = zin.copy()
    out = np.full(cap + 2 * GUARD, 0xA5, np.uint8)
    n = ctypes.c_uint32(0)
    st = L.infl_member(zin.ctypes.data + GUARD, len(member), out.ctypes.data + GUARD, cap, ctypes.addressof(n))
    assert np.array_equal(zin, keep), 'input changed'
    assert (out[:GUARD] == 0xA5).all() and (out[GUARD + cap:] == 0xA5).all(), 'wrote outside the output range'
    return st, (out[GUARD:GUARD + n.value].tobytes() if st == 0 else None)


def index(stream):
    """pcabi_inflate::gunzip_index: (in_off, out_off), 0 or a negative code."""
    L = load()
    z = np.frombuffer(stream, np.uint8) if len(stream) else np.zeros(1, np.uint8)
    m = L.infl_index(_p(z), len(stream), None, None, 0)
    if m <= 0:
        return int(m)
    a, b = np.full(m + 2, -7, np.int64), np.full(m + 2, -7, np.int64)
    assert L.infl_index(_p(z), len(stream), _p(a), _p(b), m) == m and a[0] == -7 and b[0] == -7   # cap too small
    assert L.infl_index(_p(z), len(stream), _p(a), _p(b), m + 1) == m
    assert a[m + 1] == -7 and b[m + 1] == -7
    return a[:m + 1], b[:m + 1]


# ---- members ---------------------------------------------------------------------------------------
def bgzf_header(payload_len, extra_before=b'', extra_after=b'', fname=None, fhcrc=False):
    """A BGZF member header for payload_len deflate bytes: BC carries the member's size - 1 (clamped
    for the few decoder-only members here whose incompressible 64 KiB do not fit a BGZF member)."""
    xlen = len(extra_before) + 6 + len(extra_after)
    tail = fname + b'\0' if fname is not None else b''
    total = 12 + xlen + len(tail) + (2 if fhcrc else 0) + payload_len + 8
    flg = 4 | (8 if fname is not None else 0) | (2 if fhcrc else 0)
    h = bytes([0x1f, 0x8b, 8, flg, 0, 0, 0, 0, 0, 0xff]) + struct.pack('<H', xlen) + extra_before + \
        b'BC' + struct.pack('<HH', 2, min(total - 1, 65535)) + extra_after + tail
    return h + (struct.pack('<H', zlib.crc32(h) & 0xffff) if fhcrc else b'')


def member(payload, data, isize=None, crc=None, **kw):
    """The BGZF member of a raw deflate payload that decodes to data."""
    return bgzf_header(len(payload), **kw) + payload + struct.pack(
        '<II', zlib.crc32(data) if crc is None else crc, len(data) if isize is None else isize)


def deflate_raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=()):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, last = b'', 0
    for cut in flush_at:
        out += c.compress(data[last:cut]) + c.flush(zlib.Z_FULL_FLUSH)
        last = cut
    return out + c.compress(data[last:]) + c.flush()


def zlib_raw(payload):
    """What zlib makes of a raw deflate stream: the bytes, or None when it raises or the stream
    does not end."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(payload)
    except zlib.error:
        return None
    return out if d.eof and not d.unused_data else None


def bgzf_zlib(data, block=65280, level=6):
    """data re-blocked to BGZF by zlib, with the end-of-file marker."""
    out = b''
    for lo in range(0, len(data), block):
        out += member(deflate_raw(data[lo:lo + block], level), data[lo:lo + block])
    return out + EOF_MARKER


class BitWriter(object):
    """LSB-first bit stream (RFC 1951 3.1.1)."""

    def __init__(self):
        self.bits = []

    def put(self, v, n):
        """n bits of v, least significant first (header fields, extra bits)."""
        for i in range(n):
            self.bits.append((v >> i) & 1)
        return self

    def code(self, c, n):
        """A Huffman code of n bits, most significant first."""
        for i in reversed(range(n)):
            self.bits.append((c >> i) & 1)
        return self

    def align(self):
        while len(self.bits) % 8:
            self.bits.append(0)
        return self

    def raw(self, data):
        assert len(self.bits) % 8 == 0
        for b in data:
            self.put(b, 8)
        return self

    def tobytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + k] << k for k in range(8)) for i in range(0, len(b), 8))


def canonical(lengths):
    """RFC 1951 3.2.2: {symbol: (code, length)}."""
    mx = max(lengths) if len(lengths) else 0
    cnt = [0] * (mx + 2)
    for ln in lengths:
        if ln:
            cnt[ln] += 1
    code, nxt = 0, [0] * (mx + 2)
    for b in range(1, mx + 1):
        code = (code + cnt[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, ln in enumerate(lengths):
        if ln:
            out[s] = (nxt[ln], ln)
            nxt[ln] += 1
    return out


CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]


def dynamic_header(w, lit_len, dist_len, cl_items, cl_len, final=1, hclen=None):
    """BFINAL, BTYPE 10 and a dynamic header whose code lengths are sent as cl_items: a list of
    (code-length symbol, extra value). lit_len / dist_len are only counted (HLIT, HDIST)."""
    w.put(final, 1).put(2, 2).put(len(lit_len) - 257, 5).put(len(dist_len) - 1, 5)
    n = max(i for i in range(19) if cl_len[CL_ORDER[i]]) + 1 if hclen is None else hclen
    n = max(n, 4)
    w.put(n - 4, 4)
    for i in range(n):
        w.put(cl_len[CL_ORDER[i]], 3)
    cc = canonical(cl_len)
    for s, x in cl_items:
        w.code(*cc[s])
        if s == 16:
            w.put(x, 2)
        elif s == 17:
            w.put(x, 3)
        elif s == 18:
            w.put(x, 7)
    return w


def plain_items(lengths):
    return [(ln, 0) for ln in lengths]


def cl_lengths_for(items, maxbits=7):
    """A complete code-length code (lengths for the 19 symbols) covering the symbols used."""
    used = sorted(set(s for s, _ in items))
    if len(used) == 1:
        used.append((used[0] + 1) % 19)
    ln = [0] * 19
    k = 1
    while (1 << k) < len(used):
        k += 1
    short = (1 << k) - len(used)     # symbols that get k - 1 bits
    for i, s in enumerate(used):
        ln[s] = k - 1 if i < short else k
    assert k <= maxbits and sum(2.0 ** -x for x in ln if x) == 1.0
    return ln


def emit(w, lit_codes, dist_codes, tokens):
    """tokens: ints (literals / 256) or ('m', length, distance) or ('sym', litlen symbol) or
    ('dsym', length, distance symbol, extra value)."""
    for t in tokens:
        if isinstance(t, int):
            w.code(*lit_codes[t])
            continue
        if t[0] == 'sym':
            w.code(*lit_codes[t[1]])
            continue
        ln = t[1]
        li = max(i for i in range(29) if LEN_BASE[i] <= ln)
        w.code(*lit_codes[257 + li]).put(ln - LEN_BASE[li], LEN_EXTRA[li])
        if t[0] == 'dsym':
            w.code(*dist_codes[t[2]]).put(t[3], 13 if t[2] >= 30 else DIST_EXTRA[t[2]])
        else:
            di = max(i for i in range(30) if DIST_BASE[i] <= t[2])
            w.code(*dist_codes[di]).put(t[2] - DIST_BASE[di], DIST_EXTRA[di])
    return w


def dynamic_block(w, lit_len, dist_len, tokens, items=None, cl_len=None, final=1, hclen=None):
    items = plain_items(list(lit_len) + list(dist_len)) if items is None else items
    cl_len = cl_lengths_for(items) if cl_len is None else cl_len
    dynamic_header(w, lit_len, dist_len, items, cl_len, final, hclen)
    return emit(w, canonical(lit_len), canonical(dist_len), tokens)


FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def fixed_block(w, tokens, final=1):
    w.put(final, 1).put(1, 2)
    return emit(w, canonical(FIXED_LIT), canonical(FIXED_DIST), tokens)


def fastq_text(n, seed=0):
    rng = np.random.RandomState(seed)
    out = []
    size = 0
    k = 0
    while size < n:
        ln = int(rng.randint(50, 400))
        rec = b'@read_%d runid=abc ch=%d\n' % (k, k % 512) + bytes(rng.choice(list(b'ACGT'), ln).astype(np.uint8)) + \
            b'\n+\n' + bytes((rng.randint(0, 40, ln) + 33).astype(np.uint8)) + b'\n'
        out.append(rec)
        size += len(rec)
        k += 1
    return b''.join(out)[:n]


SIZES = [0, 1, 2, 3, 257, 258, 259, 32767, 32768, 32769, 65535, 65536]


def sound_members():
    """[(name, member bytes, decoded bytes)]: zlib-made and hand-built members that decode."""
    rng = np.random.RandomState(1)
    out = []
    kinds = {
        'fastq': lambda n: fastq_text(n, 3),
        'one': lambda n: b'A' * n,
        'two': lambda n: bytes(rng.choice([65, 10], n).astype(np.uint8)),
        'random': lambda n: bytes(rng.randint(0, 256, n).astype(np.uint8)),
    }
    strategies = [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE]
    k = 0
    for kind, make in kinds.items():
        for n in SIZES:
            data = make(n)
            # every size with two (level, strategy) pairs, rotating so that all 16 pairs occur
            for j in range(2):
                level, strat = [0, 1, 6, 9][k % 4], strategies[(k // 4) % 4]
                k += 1
                flush = (n // 3, n // 3, 2 * n // 3) if j else ()
                out.append(('%s-%d-l%d-s%d-f%d' % (kind, n, level, strat, j), member(deflate_raw(data, level, strat, flush), data),
                            data))
    data = bytes(rng.randint(0, 256, 32768).astype(np.uint8))
    data += data[:258]
    out.append(('len258-dist32768', member(deflate_raw(data, 9), data), data))
    w = fixed_block(BitWriter(), list(data[:32768]) + [('m', 258, 32768), 256])
    out.append(('len258-dist32768-hand', member(w.tobytes(), data), data))
    data = b'Q' * 65535
    out.append(('dist1-65535', member(deflate_raw(data, 6), data), data))
    w = fixed_block(BitWriter(), [81] + [('m', 258, 1)] * 253 + [('m', 257, 1), ('m', 3, 1), 256])
    out.append(('dist1-65535-hand', member(w.tobytes(), data), data))
    out += hand_built()
    return out


def hand_built():
    out = []

    def add(name, w, data, **kw):
        out.append((name, member(w.tobytes(), data, **kw), data))

    # a 15-bit literal code: lengths 1, 2, ..., 14, 15, 15 over 16 symbols (Kraft sum 1)
    lit = [0] * 257
    syms = [256, 65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 76, 77, 78, 79]
    for i, s in enumerate(syms):
        lit[s] = min(i + 1, 15)
    data = bytes(syms[1:]) * 3
    add('lit15', dynamic_block(BitWriter(), lit, [1], list(data) + [256]), data)

    # HLIT = 29, HDIST = 29, HCLEN = 15, the maxima: 226 codes of 8 bits + 60 of 9 (226 / 256 +
    # 60 / 512 = 1), 28 distance codes of 5 bits + 2 of 4; matches in use
    lit = [8] * 226 + [9] * 60
    dist = [5] * 28 + [4] * 2
    body = bytes(range(256)) * 2
    data = bytearray(body)
    toks = list(body)
    for ln, d in ((258, 512), (3, 1), (100, 300), (258, 1)):
        toks.append(('m', ln, d))
        for _ in range(ln):
            data.append(data[-d])
    add('maxima', dynamic_block(BitWriter(), lit, dist, toks + [256], hclen=19), bytes(data))

    # a 16-run that crosses from the literal/length lengths into the distance lengths: HLIT = 1,
    # four literals of 5 bits, twelve of 4, symbols 256 and 257 of 4 (4 / 32 + 14 / 16 = 1), sixteen
    # distance codes of 4 bits. After symbol 256's length, 17 more 4s follow: runs of 6, 6 and 5,
    # the first of which covers symbol 257 and distance codes 0..4.
    lit = [5, 5, 5, 5] + [4] * 12 + [0] * 240 + [4, 4]
    dist = [4] * 16
    items = plain_items(lit[:257]) + [(16, 3), (16, 3), (16, 2)]
    body = bytes([0, 1, 2, 3, 4, 5, 15, 14, 13])
    toks = list(body) + [('m', 3, 9), ('m', 3, 1), 256]
    add('run16-crosses-hlit', dynamic_block(BitWriter(), lit, dist, toks, items), body + body[:3] + bytes([body[2]]) * 3)

    # an 18-run that crosses: HLIT = 10 (267 lengths), A = 1 bit, B and end-of-block 2 bits; the
    # zeros of symbols 257..266 and of distance codes 0..3 are one run of 14; distance code 4 has
    # the single length 1 (and is not used)
    lit = [0] * 267
    lit[65], lit[66], lit[256] = 1, 2, 2
    dist = [0, 0, 0, 0, 1]
    items = [(18, 65 - 11), (1, 0), (2, 0), (18, 138 - 11), (18, 189 - 138 - 11), (2, 0), (18, 14 - 11), (1, 0)]
    add('run18-crosses-hlit', dynamic_block(BitWriter(), lit, dist, [65, 66, 65, 66, 65, 256], items), b'ABABA')

    # one distance code of length 1, used / unused (this project's encoder's header); HDIST = 0
    # with length 0 (literals only)
    lit = [0] * 258
    lit[65], lit[66], lit[256], lit[257] = 2, 2, 2, 2
    add('dist-one-used', dynamic_block(BitWriter(), lit, [1], [65, 66, ('m', 3, 1), 256]), b'ABBBB')
    lit = [0] * 257
    lit[65], lit[66], lit[256] = 1, 2, 2
    add('dist-one-unused', dynamic_block(BitWriter(), lit, [1], [65, 66, 65, 256]), b'ABA')
    add('dist-none', dynamic_block(BitWriter(), lit, [0], [65, 66, 65, 256]), b'ABA')

    # a stored block after a dynamic block at each of the 8 bit phases: A has a 1-bit code, so
    # every further A moves the dynamic block's end by one bit
    seen = set()
    for extra in range(16):
        w = dynamic_block(BitWriter(), lit, [0], [65] * extra + [256], final=0)
        phase = len(w.bits) % 8
        if phase in seen:
            continue
        seen.add(phase)
        w.put(1, 1).put(0, 2).align().put(5, 16).put(5 ^ 0xffff, 16).raw(b'hello')
        add('stored-after-dyn-phase%d' % phase, w, b'A' * extra + b'hello')
    assert len(seen) == 8

    # several blocks, mixed: fixed, empty stored, fixed with a match that reaches back across the
    # block boundary, a final empty stored block
    w = fixed_block(BitWriter(), list(b'abcdef') + [256], final=0)
    w.put(0, 1).put(0, 2).align().put(0, 16).put(0xffff, 16)
    fixed_block(w, [('m', 6, 6), 256], final=0)
    w.put(1, 1).put(0, 2).align().put(0, 16).put(0xffff, 16)
    add('mixed-blocks', w, b'abcdefabcdef')
    return out


def damaged_members():
    """[(name, member bytes, expected status)]: every payload makes zlib raise (or never end)."""
    out = []
    good = b'hello hello hello hello'

    def add(name, payload, status, data=good, **kw):
        out.append((name, member(payload, data, **kw), status))

    add('nlen-wrong', BitWriter().put(1, 1).put(0, 2).align().put(5, 16).put(4 ^ 0xffff, 16).raw(b'hello').tobytes(),
        E_HEADER)
    add('btype3', BitWriter().put(1, 1).put(3, 2).put(0, 13).tobytes(), E_HEADER)
    lit = [0] * 257
    lit[65], lit[66], lit[67], lit[256] = 1, 1, 2, 2
    add('oversubscribed', dynamic_block(BitWriter(), lit, [1], []).put(0, 16).tobytes(), E_CODE)
    lit = [0] * 257
    lit[65], lit[66], lit[256] = 2, 2, 2
    add('incomplete-lit', dynamic_block(BitWriter(), lit, [1], []).put(0, 16).tobytes(), E_CODE)
    lit = [0] * 257
    lit[65], lit[256] = 1, 1
    items = [(16, 0)] + plain_items(lit[3:] + [1])
    add('run16-first', dynamic_block(BitWriter(), lit, [1], [], items, cl_lengths_for(items)).put(0, 16).tobytes(), E_CODE)
    add('sym286', fixed_block(BitWriter(), [65, ('sym', 286), 256]).tobytes(), E_CODE)
    add('dist30', fixed_block(BitWriter(), [65, 66, 67, ('dsym', 3, 30, 0), 256]).tobytes(), E_CODE)
    add('dist-before-start', fixed_block(BitWriter(), [65, 66, ('m', 3, 3), 256]).tobytes(), E_DIST)
    data = fastq_text(600, 5)
    small = deflate_raw(data, 6)
    for k in range(len(small)):
        out.append(('cut-%d' % k, member(small[:k], data), E_INPUT))
    out.append(('isize-small', member(small, data, isize=len(data) - 1), E_OUTPUT))
    out.append(('isize-large', member(small, data, isize=len(data) + 1), E_LENGTH))
    # one flipped bit in a stored block's bytes still decodes
    st = deflate_raw(data, 0)
    flipped = bytearray(st)
    flipped[40] ^= 4
    out.append(('bitflip-crc', member(bytes(flipped), data), E_CRC))
    return out


def damaged_payload_of(m):
    """The raw deflate payload of a member built by member() with a plain BGZF header."""
    return m[18:-8]
