"""Block-gzipped input inflated on the GPU (csrc/pcabi_inflate.hip; include/pcabi.h pcabi_gunzip_*).
The corpora are those of tests/test_inflate_cpu.py, where the same decoder source runs on the host;
the expected bytes come from zlib."""
import ctypes
import glob
import gzip
import os

import numpy as np
import pytest

from tests import inflate_cpu_lib as I

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p


def _vp(a):
    return a.ctypes.data_as(P) if a is not None else None


@pytest.fixture(scope='module')
def sound():
    return I.sound_members()


@pytest.fixture(scope='module')
def damaged():
    return I.damaged_members()


@pytest.fixture
def tuned(gpu_lib):
    def tune(chunk_bytes=0):
        assert gpu_lib.pcabi_gunzip_tune(chunk_bytes) == 0
    yield tune
    assert gpu_lib.pcabi_gunzip_tune(0) == 0


def dev_gunzip(L, members, sizes, pad=64, cap_delta=0):
    """pcabi_gunzip_dev over a list of members laid end to end, every buffer on the device, the
    output (pad bytes on either side of the members' ranges) pre-filled with 0xA5.
    Returns (rc, status[m], out)."""
    from custom_porechop_abi_amd._lib import check as chk
    z = np.frombuffer(b''.join(members), np.uint8)
    in_off = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int64)
    out_off = (np.concatenate([[0], np.cumsum(sizes)]) + pad).astype(np.int64)
    nm = len(members)
    total = int(out_off[-1]) + pad
    out_cap = int(out_off[-1]) + cap_delta
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
        d_z, d_out, d_in_off, d_out_off, d_st = dmalloc(z.size), dmalloc(total), dmalloc(in_off.nbytes), \
            dmalloc(out_off.nbytes), dmalloc(4 * nm)
        if z.size:
            chk(L.pcabi_dev_h2d(d_z, _vp(z), z.size), 'h2d')
        chk(L.pcabi_dev_h2d(d_in_off, _vp(in_off), in_off.nbytes), 'h2d')
        chk(L.pcabi_dev_h2d(d_out_off, _vp(out_off), out_off.nbytes), 'h2d')
        chk(L.pcabi_dev_memset(d_out, 0xA5, total), 'memset')
        chk(L.pcabi_dev_memset(d_st, 0x7f, 4 * nm), 'memset')
        sb = L.pcabi_gunzip_scratch_bytes(nm)
        assert sb >= 0
        d_scr = dmalloc(sb) if sb else None
        rc = L.pcabi_gunzip_dev(st, d_z, z.size, d_in_off, d_out_off, nm, d_out, out_cap, d_st, d_scr, sb)
        chk(L.pcabi_stream_sync(st), 'sync')
        status, out = np.zeros(nm, np.int32), np.zeros(total, np.uint8)
        chk(L.pcabi_dev_d2h(_vp(status), d_st, 4 * nm), 'd2h')
        chk(L.pcabi_dev_d2h(_vp(out), d_out, total), 'd2h')
        return rc, status, out, out_off
    finally:
        for p in ptrs:
            L.pcabi_dev_free(p)
        L.pcabi_stream_destroy(st)


def test_sound_members(gpu_lib, sound):
    """All sound members in one launch, end to end in one output buffer (so every member's range
    starts at an odd address): each decodes to zlib's bytes and nothing outside the ranges changes."""
    members, datas = [m for _, m, _ in sound], [d for _, _, d in sound]
    rc, status, out, out_off = dev_gunzip(gpu_lib, members, [len(d) for d in datas], pad=61)
    assert rc == 0
    bad = [(sound[k][0], int(s)) for k, s in enumerate(status) if s != 0]
    assert not bad, bad
    for k, d in enumerate(datas):
        assert out[out_off[k]:out_off[k + 1]].tobytes() == d, sound[k][0]
    assert np.all(out[:61] == 0xA5) and np.all(out[out_off[-1]:] == 0xA5)


def test_damaged_members_give_their_status(gpu_lib, damaged):
    """Error paths: the status the host build of the same source gives, nothing else."""
    members = [m for _, m, _ in damaged]
    sizes = [min(int.from_bytes(m[-4:], 'little'), 65536) for m in members]
    rc, status, out, out_off = dev_gunzip(gpu_lib, members, sizes)
    assert rc == 0
    wrong = [(damaged[k][0], int(s), damaged[k][2]) for k, s in enumerate(status) if s != damaged[k][2]]
    assert not wrong, wrong
    assert np.all(out[:64] == 0xA5) and np.all(out[out_off[-1]:] == 0xA5)


def test_damaged_member_among_sound_neighbours(gpu_lib, sound, damaged):
    pick = [s for s in sound if s[0] in ('maxima', 'lit15', 'mixed-blocks') or s[0].startswith('fastq-32769')] + sound[:6]
    bad = [d for d in damaged if d[0] in ('bitflip-crc', 'dist-before-start', 'cut-100', 'oversubscribed')]
    assert len(bad) == 4
    for b in bad:
        members = [s[1] for s in pick[:4]] + [b[1]] + [s[1] for s in pick[4:]]
        datas = [s[2] for s in pick[:4]] + [None] + [s[2] for s in pick[4:]]
        sizes = [len(d) if d is not None else min(int.from_bytes(b[1][-4:], 'little'), 65536) for d in datas]
        rc, status, out, out_off = dev_gunzip(gpu_lib, members, sizes)
        assert rc == 0
        assert [int(s) for s in status] == [0] * 4 + [b[2]] + [0] * (len(pick) - 4)
        for k, d in enumerate(datas):
            if d is not None:
                assert out[out_off[k]:out_off[k + 1]].tobytes() == d
        assert np.all(out[:64] == 0xA5) and np.all(out[out_off[-1]:] == 0xA5)


def test_out_cap_too_small_is_refused(gpu_lib, sound):
    pick = [s for s in sound if 0 < len(s[2]) < 5000][:5]
    members, datas = [s[1] for s in pick], [s[2] for s in pick]
    rc, status, out, out_off = dev_gunzip(gpu_lib, members, [len(d) for d in datas], cap_delta=-1)
    assert rc != 0 or status[-1] == I.E_OUTPUT
    assert np.all(out[out_off[-2]:] == 0xA5)        # the refused member wrote nothing
    if rc == 0:
        assert not status[:-1].any()
        for k, d in enumerate(datas[:-1]):
            assert out[out_off[k]:out_off[k + 1]].tobytes() == d
    assert gpu_lib.pcabi_gunzip_dev(None, None, -1, None, None, 0, None, 0, None, None, 0) < 0


def _stream(n_members, seed):
    text = I.fastq_text(n_members * 3000, seed)
    cuts = np.linspace(0, len(text), n_members + 1).astype(int)
    parts = [text[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    z = b''.join(I.member(I.deflate_raw(p, 6 if k % 2 else 1), p) for k, p in enumerate(parts))
    return text, z


def test_host_entry_and_staged_passes(gpu_lib, tuned):
    """~300 members through pcabi_gunzip_host with staged passes forced small (many passes, both
    slots in turn) and with the default."""
    from custom_porechop_abi_amd import engine
    text, z = _stream(300, 11)
    z += I.EOF_MARKER
    assert gzip.decompress(z) == text
    in_off, out_off = engine.bgzf_index(z)
    assert len(in_off) == 302 and out_off[-1] == len(text) and in_off[-1] == len(z)
    assert engine.gunzip(z) == text
    for chunk in (1, 20000, 100000):
        tuned(chunk)
        assert engine.gunzip(z) == text
    tuned(0)
    t = (ctypes.c_double * 3)()
    gpu_lib.pcabi_gunzip_last_times(ctypes.byref(t, 0), ctypes.byref(t, 8), ctypes.byref(t, 16))
    assert all(x >= 0 for x in t)


def test_host_entry_small_buffer_is_left_alone(gpu_lib):
    text, z = _stream(20, 12)
    zb = np.frombuffer(z, np.uint8)
    for cap in (len(text) - 1, 10, 0):
        buf = np.full(len(text) + 64, 0xA5, np.uint8)
        assert gpu_lib.pcabi_gunzip_host(0, _vp(zb), zb.size, _vp(buf), cap) == len(text)
        assert np.all(buf == 0xA5)
    buf = np.full(len(text) + 64, 0xA5, np.uint8)
    assert gpu_lib.pcabi_gunzip_host(0, _vp(zb), zb.size, _vp(buf), len(text)) == len(text)
    assert buf[:len(text)].tobytes() == text and np.all(buf[len(text):] == 0xA5)


def test_host_entry_errors(gpu_lib, tuned):
    from custom_porechop_abi_amd import _lib, engine
    text, z = _stream(12, 13)
    with pytest.raises(_lib.PcabiError) as e:
        engine.gunzip(gzip.compress(text))
    assert '(-1)' in str(e.value)                                            # PCABI_E_ARG: not indexable
    assert engine.bgzf_index(gzip.compress(text)) is None
    with pytest.raises(_lib.PcabiError) as e:
        engine.gunzip(z[:-5])
    assert '(-4)' in str(e.value)                                            # PCABI_E_PARSE: truncated chain
    in_off, _ = engine.bgzf_index(z)
    bad = bytearray(z)
    bad[in_off[7] + 200] ^= 0x10                                             # inside member 7's payload
    for chunk in (0, 9000):
        tuned(chunk)
        with pytest.raises(_lib.PcabiError) as e:
            engine.gunzip(bytes(bad))
        assert '(-4)' in str(e.value) and 'member 7 ' in str(e.value) and 'offset %d ' % in_off[7] in str(e.value)


def test_golden_texts_reblocked(gpu_lib):
    from custom_porechop_abi_amd import engine
    paths = sorted(glob.glob(os.path.join(ROOT, 'tests', 'golden', 'data', '*.gz')))
    assert len(paths) >= 4
    for path in paths:
        text = gzip.open(path, 'rb').read()
        for block, level in ((65280, 6), (4000, 9), (65280, 1)):
            assert engine.gunzip(I.bgzf_zlib(text, block, level)) == text


# ---- BGZF output from the device encoder (pcabi_bgzf_*), read back on the device ----------------
def _fib(n):
    a, b, out = 1, 1, []
    for _ in range(n):
        out.append(a)
        a, b = b, a + b
    return out


def bgzf_check(data, blocks=None, eof=True):
    """engine.bgzf_compress(data): decodes with Python's gzip and with engine.gunzip, every member
    is at most 65536 bytes, the BSIZE chain ends exactly at the stream's end, the marker closes it."""
    from custom_porechop_abi_amd import engine
    data = bytes(data)
    z = engine.bgzf_compress(data, blocks, eof=eof)
    assert (gzip.decompress(z) if z else b'') == data
    pos, sizes = 0, []
    while pos < len(z):
        assert z[pos:pos + 4] == b'\x1f\x8b\x08\x04' and z[pos + 10:pos + 16] == b'\x06\x00BC\x02\x00'
        size = int.from_bytes(z[pos + 16:pos + 18], 'little') + 1
        assert 28 <= size <= 65536
        sizes.append(int.from_bytes(z[pos + size - 4:pos + size], 'little'))
        pos += size
    assert pos == len(z)
    assert (z[-28:] == engine.BGZF_EOF) if eof else (not z.endswith(engine.BGZF_EOF) or not data)
    nb = 0 if blocks is None else len(blocks) - 1
    assert len(z) <= gpu_bound(len(data), nb, eof)
    if z:
        idx = engine.bgzf_index(z)
        assert idx is not None and list(np.diff(idx[1])) == sizes and idx[0][-1] == len(z)
        assert engine.gunzip(z) == data
    return z


def gpu_bound(n, nb, eof):
    from custom_porechop_abi_amd import _lib
    return int(_lib.lib().pcabi_bgzf_bound(n, nb, int(eof)))


def test_bgzf_round_trips(gpu_lib):
    """The inputs of test_gpu_deflate.py through engine.gunzip(engine.bgzf_compress(x))."""
    from custom_porechop_abi_amd import engine
    rng = np.random.default_rng(3)
    assert bgzf_check(b'') == engine.BGZF_EOF and bgzf_check(b'', eof=False) == b''
    for x in (b'\x00', b'A', b'G' * 65280, b'G' * 65281, b'AB' * 50000):
        bgzf_check(x)
        bgzf_check(x, eof=False)
    raw = rng.integers(0, 256, 65280, dtype=np.uint8).tobytes()      # incompressible: a stored block
    z = bgzf_check(raw, np.array([0, 65280], np.int64))
    assert len(z) == 65280 + 5 + 28 + 28 and len(z) - 28 <= 65536
    for counts in (_fib(22), np.floor(25000 * 0.6 ** np.arange(20)).astype(np.int64).tolist()):   # length-limited code
        vals = rng.permutation(256)[:len(counts)].astype(np.uint8)
        data = np.repeat(vals, counts)
        rng.shuffle(data)
        assert data.size <= 65280
        assert len(bgzf_check(data, np.array([0, data.size], np.int64))) < data.size // 2
    text = (b'ACGTTGCA' * 40 + b'\n' + bytes(rng.integers(38, 73, 300, dtype=np.uint8)) + b'\n') * 300
    sizes = [1, 65280, 2, 3, 65279, 1, 17, 4096]
    off = np.concatenate([[0], np.minimum(np.cumsum(sizes), len(text))]).astype(np.int64)
    off = np.unique(np.concatenate([off, [len(text)]]))
    bgzf_check(text, off)
    bgzf_check(text, engine.gzip_line_blocks(text, cap=engine.BGZF_BLOCK_CAP))


def test_bgzf_long_block_refused(gpu_lib):
    from custom_porechop_abi_amd import _lib, engine
    data = b'A' * 70000
    for off in ([0, 65281, 70000], [0, 10, 10, 70000 - 65280, 70000], [0, 4464], [1, 70000]):
        with pytest.raises(_lib.PcabiError) as e:
            engine.bgzf_compress(data, np.array(off, np.int64))
        assert '(-1)' in str(e.value)
    z = engine.bgzf_compress(data)
    with pytest.raises(ValueError):
        engine.bgzf_compress(data, cap=len(z) - 1)


def test_bgzf_golden_texts(gpu_lib, tuned):
    from custom_porechop_abi_amd import engine
    paths = sorted(glob.glob(os.path.join(ROOT, 'tests', 'golden', 'data', '*.gz')))
    assert len(paths) >= 4
    for path in paths:
        text = gzip.open(path, 'rb').read()
        bgzf_check(text)
        z = bgzf_check(text, engine.gzip_line_blocks(text, cap=engine.BGZF_BLOCK_CAP), eof=False)
        tuned(50000)
        assert engine.gunzip(z) == text
        tuned(0)


# SHA-256 of engine.gzip_compress's bytes for the inputs of test_gpu_deflate.py's
# test_dev_entry_matches_host_entry, recorded on an MI355X from the commit before pcabi_deflate.hip
# learnt the BGZF member layout: the plain gzip stream must not change.
GZIP_SHA256 = {
    'fixed': '11d51993f508677668f66cf8b79bfb2ea5429de36febfef5a94c18d4a36ac550',
    'lines': '25ca348dc757f249696eaf8d9aa6b8dd62c90ecff118b436391523eb86275032',
    'mixed': '33eae1b240bd8f705964309c134eacd6439709e9cd7c1e3153abf92f36f3a6a3',
    'empty': 'ac73670af3abed54ac6fb4695131f4099be9fbe39d6076c5d0264a6bbdae9d83',
}


def test_gzip_compress_bytes_unchanged(gpu_lib):
    import hashlib
    from custom_porechop_abi_amd import engine
    rng = np.random.default_rng(9)
    text = (b'@r\n' + bytes(rng.choice(np.frombuffer(b'ACGT', np.uint8), 9000)) + b'\n+\n' +
            bytes(rng.integers(38, 73, 9000, dtype=np.uint8)) + b'\n') * 9
    mixed = np.concatenate([[0, 1, 2], np.arange(5000, len(text), 40000), [len(text)]]).astype(np.int64)
    got = {name: hashlib.sha256(engine.gzip_compress(text, off)).hexdigest()
           for name, off in (('fixed', None), ('lines', engine.gzip_line_blocks(text)), ('mixed', mixed))}
    got['empty'] = hashlib.sha256(engine.gzip_compress(b'')).hexdigest()
    assert got == GZIP_SHA256
