"""gzip compressed on the GPU (csrc/pcabi_deflate.hip; include/pcabi.h pcabi_gzip_*). Every
stream must decompress to its input with Python's gzip (which checks the CRC-32 and ISIZE of every
member) and member by member with zlib.decompressobj(31), consuming the stream exactly."""
import ctypes
import glob
import gzip
import os
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p


def _vp(a):
    return a.ctypes.data_as(P) if a is not None else None


def members(stream):
    """Decoded members of a gzip stream, one zlib.decompressobj(31) each; the stream is consumed exactly."""
    out, rest = [], stream
    while rest:
        d = zlib.decompressobj(31)
        out.append(d.decompress(rest))
        assert d.eof, 'truncated member'
        rest = d.unused_data
    return out


def check(data, blocks=None, min_members=1):
    from custom_porechop_abi_amd import engine
    data = bytes(data)
    z = engine.gzip_compress(data, blocks)
    assert gzip.decompress(z) == data
    ms = members(z)
    assert len(ms) >= min_members and b''.join(ms) == data
    nb = 0 if blocks is None else len(blocks) - 1
    assert len(z) <= engine.gzip_bound(len(data), nb)
    return z


@pytest.fixture(scope='module')
def B(gpu_lib):
    b = gpu_lib.pcabi_gzip_block_len()
    assert 1 <= b <= 65535
    return b


@pytest.fixture
def tuned(gpu_lib):
    """Small members and staged passes for one test; the defaults come back after it."""
    def tune(block_len=0, member_blocks=0, chunk_bytes=0):
        assert gpu_lib.pcabi_gzip_tune(block_len, member_blocks, chunk_bytes) == 0
    yield tune
    assert gpu_lib.pcabi_gzip_tune(0, 0, 0) == 0


def test_empty_and_one_byte(gpu_lib):
    z = check(b'')
    assert len(z) == 20 and len(members(z)) == 1      # one empty member
    check(b'\x00')
    check(b'A')
    check(b'\xff')


def test_one_symbol(gpu_lib, B):
    for n in (1, 2, B - 1, B, B + 1, 3 * B + 17):
        check(b'G' * n)
    check(b'\x00' * (B + 1))


def test_two_symbols(gpu_lib, B):
    rng = np.random.default_rng(2)
    check(b'AB')
    check(np.where(rng.random(3 * B + 5) < 0.01, 65, 255).astype(np.uint8))
    check(np.where(rng.random(777) < 0.5, 0, 10).astype(np.uint8))


def test_incompressible_is_stored(gpu_lib):
    from custom_porechop_abi_amd import engine
    rng = np.random.default_rng(3)
    for n in (65535, 65536):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        z = check(data)
        blocks = -(-n // engine.gzip_block_len())
        assert len(z) == n + 5 * blocks + 20          # every block stored: 5 bytes each, one member
        off = np.array([0, 65535, n] if n > 65535 else [0, n], np.int64)
        assert len(check(data, off)) == n + 5 * (len(off) - 1) + 20


def test_all_values_equal_counts(gpu_lib):
    rng = np.random.default_rng(4)
    data = np.repeat(np.arange(256, dtype=np.uint8), 100)
    rng.shuffle(data)
    check(data, np.array([0, data.size], np.int64))
    check(np.arange(256, dtype=np.uint8))


def _fib(n):
    a, b, out = 1, 1, []
    for _ in range(n):
        out.append(a)
        a, b = b, a + b
    return out


def test_length_limit(gpu_lib):
    """One block whose unlimited Huffman code is deeper than 15 bits: 22 values with Fibonacci counts
    (46,367 bytes; depth 21 when ties go the deep way) and 20 values with counts falling by 0.6
    (a chain of depth 20 whichever way ties go). A dynamic block must come out, and decode."""
    rng = np.random.default_rng(5)
    for counts in (_fib(22), np.floor(25000 * 0.6 ** np.arange(20)).astype(np.int64).tolist()):
        vals = rng.permutation(256)[:len(counts)].astype(np.uint8)
        data = np.repeat(vals, counts)
        rng.shuffle(data)
        assert data.size <= 65535
        z = check(data, np.array([0, data.size], np.int64))
        assert len(z) < data.size // 2


def test_block_lists(gpu_lib):
    rng = np.random.default_rng(6)
    text = (b'ACGTTGCA' * 40 + b'\n' + bytes(rng.integers(38, 73, 300, dtype=np.uint8)) + b'\n') * 700
    n = len(text)
    check(text[:300], np.arange(301, dtype=np.int64))                       # blocks of 1 byte
    pattern, sizes = [1, 65535, 2, 3, 65534, 1, 17, 4096, 4097, 255], []     # tiny and maximal blocks mixed
    while sum(sizes) + pattern[len(sizes) % 10] <= n:
        sizes.append(pattern[len(sizes) % 10])
    if sum(sizes) < n:
        sizes.append(n - sum(sizes))
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    assert off[-1] == n and np.all(np.diff(off) >= 1) and np.all(np.diff(off) <= 65535)
    check(text, off)
    ragged = np.concatenate([np.arange(0, n, 10007), [n]]).astype(np.int64)  # the last block is ragged
    assert (n - ragged[-2]) not in (0, 10007)
    check(text, ragged)


def test_bad_block_list_refused(gpu_lib):
    from custom_porechop_abi_amd import _lib, engine
    data = b'A' * 70000
    for off in ([0, 10, 10, 70000 - 65535, 70000], [0, 65536, 70000], [0, 4464], [1, 70000], [0, 70001]):
        with pytest.raises(_lib.PcabiError) as e:
            engine.gzip_compress(data, np.array(off, np.int64))
        assert '(-1)' in str(e.value)                                       # PCABI_E_ARG


def test_members_and_staged_passes(gpu_lib, tuned):
    """Several members per pass and several staged passes: 2 KiB blocks, 3 blocks per member, 64 KiB
    per pass over ~600 KB."""
    from custom_porechop_abi_amd import engine
    rng = np.random.default_rng(7)
    data = bytes(rng.choice(np.frombuffer(b'ACGT', np.uint8), 600001))
    tuned(2048, 3, 65536)
    assert engine.gzip_block_len() == 2048
    z = check(data, min_members=600001 // (3 * 2048))
    assert all(len(m) <= 3 * 2048 for m in members(z))
    off = engine.gzip_line_blocks(data, 1024, 5000)
    z2 = check(data, off, min_members=len(off) // 3)
    tuned(0, 0, 0)
    assert gzip.decompress(engine.gzip_compress(data)) == data


def test_small_buffer_is_left_alone(gpu_lib):
    from custom_porechop_abi_amd import engine
    rng = np.random.default_rng(8)
    data = np.frombuffer(bytes(rng.choice(np.frombuffer(b'ACGTN\n', np.uint8), 200000)), np.uint8)
    z = engine.gzip_compress(data)
    need = len(z)
    for cap in (need - 1, need // 2, 19, 0):
        buf = np.full(need + 64, 0xA5, np.uint8)
        got = gpu_lib.pcabi_gzip_host(0, _vp(data), data.size, None, 0, _vp(buf), cap)
        assert got == need
        assert np.all(buf[cap:] == 0xA5)
    buf = np.full(need + 64, 0xA5, np.uint8)
    assert gpu_lib.pcabi_gzip_host(0, _vp(data), data.size, None, 0, _vp(buf), need) == need
    assert buf[:need].tobytes() == z and np.all(buf[need:] == 0xA5)


def _dev_gzip(L, data, off, cap=None):
    """pcabi_gzip_dev on a stream of the caller's, every buffer on the device."""
    from custom_porechop_abi_amd._lib import check as chk
    data = np.frombuffer(bytes(data), np.uint8)
    nb = 0 if off is None else len(off) - 1
    bound = L.pcabi_gzip_bound(data.size, nb)
    cap = bound if cap is None else cap
    sb = L.pcabi_gzip_scratch_bytes(data.size, nb)
    chk(L.pcabi_dev_set(0), 'pcabi_dev_set')
    st = P()
    chk(L.pcabi_stream_create(ctypes.byref(st)), 'stream')
    ptrs = []

    def dmalloc(nbytes):
        p = P()
        chk(L.pcabi_dev_malloc(ctypes.byref(p), max(int(nbytes), 16)), 'malloc')
        ptrs.append(p)
        return p
    try:
        d_in, d_out, d_len, d_scr = dmalloc(data.size), dmalloc(bound + 64), dmalloc(8), dmalloc(sb)
        d_off = None
        if data.size:
            chk(L.pcabi_dev_h2d(d_in, _vp(data), data.size), 'h2d')
        if off is not None:
            off = np.ascontiguousarray(off, np.int64)
            d_off = dmalloc(off.nbytes)
            chk(L.pcabi_dev_h2d(d_off, _vp(off), off.nbytes), 'h2d')
        chk(L.pcabi_dev_memset(d_out, 0xA5, bound + 64), 'memset')
        chk(L.pcabi_gzip_dev(st, d_in, data.size, d_off, nb, d_out, cap, d_len, d_scr, sb), 'pcabi_gzip_dev')
        chk(L.pcabi_stream_sync(st), 'sync')
        n = np.zeros(1, np.int64)
        out = np.zeros(bound + 64, np.uint8)
        chk(L.pcabi_dev_d2h(_vp(n), d_len, 8), 'd2h')
        chk(L.pcabi_dev_d2h(_vp(out), d_out, out.size), 'd2h')
        return int(n[0]), out
    finally:
        for p in ptrs:
            L.pcabi_dev_free(p)
        L.pcabi_stream_destroy(st)


def test_dev_entry_matches_host_entry(gpu_lib):
    from custom_porechop_abi_amd import engine
    rng = np.random.default_rng(9)
    text = (b'@r\n' + bytes(rng.choice(np.frombuffer(b'ACGT', np.uint8), 9000)) + b'\n+\n' +
            bytes(rng.integers(38, 73, 9000, dtype=np.uint8)) + b'\n') * 9
    mixed = np.concatenate([[0, 1, 2], np.arange(5000, len(text), 40000), [len(text)]]).astype(np.int64)
    for off in (None, engine.gzip_line_blocks(text), mixed):
        n, out = _dev_gzip(gpu_lib, text, off)
        z = engine.gzip_compress(text, off)
        assert n == len(z) and out[:n].tobytes() == z
        assert np.all(out[n:] == 0xA5)
        n2, out2 = _dev_gzip(gpu_lib, text, off, cap=n - 1)                  # too small: the size, nothing written
        assert n2 == n and np.all(out2 == 0xA5)
    n, out = _dev_gzip(gpu_lib, b'', None)
    assert n == 20 and gzip.decompress(out[:n].tobytes()) == b''
    bad = np.array([0, 70000, len(text)], np.int64)                          # a block past 65535 bytes: -1, untouched
    n, out = _dev_gzip(gpu_lib, text, bad)
    assert n == -1 and np.all(out == 0xA5)


def test_golden_texts(gpu_lib):
    from custom_porechop_abi_amd import engine
    paths = sorted(glob.glob(os.path.join(ROOT, 'tests', 'golden', 'data', '*.gz')))
    assert len(paths) >= 4
    for path in paths:
        text = gzip.open(path, 'rb').read()
        check(text)
        off = engine.gzip_line_blocks(text)
        lines_end = np.cumsum([len(l) + 1 for l in text.split(b'\n')[:-1]])
        long_ends = lines_end[np.diff(np.concatenate([[0], lines_end])) >= engine.GZIP_LONG_LINE]
        assert np.isin(long_ends, off).all()
        check(text, off)
