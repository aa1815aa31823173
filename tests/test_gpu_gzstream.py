"""Ordinary (non-BGZF) gzip input inflated on the GPU (csrc/pcabi_gzstream.hip; include/pcabi.h
pcabi_gunzip_stream_*; engine.gunzip_stream; misc / FileTrimmer gunzip_plain). The corpora are those
of tests/test_gzstream_cpu.py, where the same source runs on the host; every expected byte comes
from zlib / gzip. The streams are small; the tune switch makes them many chunks."""
import ctypes
import gzip
import os
import zlib

import numpy as np
import pytest

from tests import golden_lib
from tests import gzstream_cpu_lib as G

pytestmark = pytest.mark.gpu

DATA = os.path.join(golden_lib.GOLDEN, 'data')
P = ctypes.c_void_p
FIELDS = ('name_off', 'seq_off', 'qual_off', 'spacer_off', 'names', 'seq', 'qual', 'spacer', 'rna', 'codes',
          'code_off', 'lengths')
ALL_HOST = 1 << 40   # a min_chunks no span reaches


@pytest.fixture
def tuned(gpu_lib):
    def tune(chunk_bytes=0, span_bytes=0, min_chunks=0):
        assert gpu_lib.pcabi_gunzip_stream_tune(chunk_bytes, span_bytes, min_chunks) == 0
    yield tune
    assert gpu_lib.pcabi_gunzip_stream_tune(0, 0, 0) == 0


def gunzip(L, data, cap=None):
    """pcabi_gunzip_stream_host between 64 guard bytes of 0xA5 on either side, which must survive.
    Returns (bytes, stats); raises PcabiError as engine.gunzip_stream does."""
    from custom_porechop_abi_amd import engine
    from custom_porechop_abi_amd._lib import check
    z = np.frombuffer(data, np.uint8) if len(data) else np.zeros(1, np.uint8)
    cap = len(zlib_len(data)) if cap is None else cap
    out = np.full(cap + 2 * G.GUARD, 0xA5, np.uint8)
    n = L.pcabi_gunzip_stream_host(0, z.ctypes.data_as(P), len(data), P(out.ctypes.data + G.GUARD), cap)
    assert (out[:G.GUARD] == 0xA5).all() and (out[G.GUARD + cap:] == 0xA5).all(), 'wrote outside the output range'
    if n < 0:
        check(int(n), 'pcabi_gunzip_stream_host')
    st = engine.gunzip_stream_stats()
    if n > cap:
        assert (out == 0xA5).all(), 'a too small buffer was written to'
        return int(n), st
    return out[G.GUARD:G.GUARD + n].tobytes(), st


def zlib_len(data):
    try:
        return G.zlib_all(data)
    except zlib.error:
        return bytes(4 * len(data) + 65536)


# ---- 1. text -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('level,mem', G.TEXT_SETTINGS)
def test_text(gpu_lib, tuned, level, mem):
    t = G.text()
    tuned(G.chunk_for(mem))
    got, st = gunzip(gpu_lib, G.gz(t, level, mem))
    assert got == t
    assert st['host_bytes'] == 0 and st['confirmed'] >= 4 and st['dev_bytes'] == len(t), st


def test_golden_files(gpu_lib, tuned):
    from custom_porechop_abi_amd import engine
    assert len(G.GOLDEN_GZ) == 4
    tuned(4096)
    for path in G.GOLDEN_GZ:
        with open(path, 'rb') as f:
            s = f.read()
        got, st = gunzip(gpu_lib, s)
        assert got == gzip.open(path).read(), path
        assert st['host_bytes'] == 0 and st['members'] == 1, (path, st)
        assert engine.gunzip_stream(s) == got
        # the existing entries keep refusing such a stream
        assert engine.bgzf_index(s) is None
        with pytest.raises(Exception):
            engine.gunzip(s)


# ---- 2. history across chunk boundaries ----------------------------------------------------------------
@pytest.mark.parametrize('k', range(5))
def test_history_across_chunks(gpu_lib, tuned, k):
    name, s, data, chunk = G.history_streams()[k]
    tuned(chunk)
    got, st = gunzip(gpu_lib, s)
    assert got == data, name
    assert st['host_bytes'] == 0 and st['dev_bytes'] == len(data), (name, st)


# ---- 3. block types ------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', range(5))
def test_block_types(gpu_lib, tuned, k):
    name, s, data, chunk = G.block_type_streams()[k]
    assert G.zlib_all(s) == data
    tuned(chunk)
    got, st = gunzip(gpu_lib, s)
    assert got == data, name
    assert st['dev_bytes'] + st['host_bytes'] == len(data), (name, st)
    tuned(chunk, 0, ALL_HOST)
    got, st = gunzip(gpu_lib, s)
    assert got == data, name
    assert st['host_bytes'] == len(data) and st['dev_bytes'] == 0, (name, st)


# ---- 4. members ----------------------------------------------------------------------------------------
def test_members(gpu_lib, tuned):
    from custom_porechop_abi_amd import engine
    tuned(4096)
    for name, s, data, members in G.member_streams():
        assert gzip.decompress(s) == data, name
        got, st = gunzip(gpu_lib, s)
        assert got == data and st['members'] == members, (name, st)
    t = G.text()[:300000]
    s = engine.gzip_compress(t)          # the project's own multi-member stream
    got, st = gunzip(gpu_lib, s)
    assert got == t == gzip.decompress(s) and st['members'] == G.zlib_members(s) >= 1, st
    s = engine.bgzf_compress(t)          # BGZF with its end-of-file member
    got, st = gunzip(gpu_lib, s)
    assert got == t and st['members'] == len(engine.bgzf_index(s)[0]) - 1 == G.zlib_members(s) >= 3, st


# ---- 5. a false candidate ------------------------------------------------------------------------------
def test_false_candidate(gpu_lib, tuned):
    s, data, places = G.false_candidate_stream(4096)
    assert G.zlib_all(s) == data
    assert all(0 < p % 4096 <= 64 for p in places)
    tuned(4096)
    got, st = gunzip(gpu_lib, s)
    assert got == data
    assert st['rejected'] >= 1, st


# ---- 6. spans ------------------------------------------------------------------------------------------
def test_spans(gpu_lib, tuned):
    t = G.text()
    s = G.gz(t, 6, 1)
    tuned(4096, 65536)
    got, st = gunzip(gpu_lib, s)
    assert got == t
    assert st['spans'] >= len(s) // 65536 >= 3 and st['host_bytes'] == 0, st


# ---- 7. errors -----------------------------------------------------------------------------------------
def test_errors(gpu_lib, tuned):
    from custom_porechop_abi_amd._lib import PcabiError
    tuned(4096)
    for name, s in G.error_streams():
        with pytest.raises(zlib.error):
            G.zlib_all(s)
        with pytest.raises(PcabiError) as e:
            gunzip(gpu_lib, s)
        msg = str(e.value)
        assert '(-4)' in msg and 'member %d at offset ' % (1 if name == 'reserved-flag' else 0) in msg, (name, msg)


def test_small_capacity_and_empty_input(gpu_lib, tuned):
    from custom_porechop_abi_amd import engine
    t = G.text()[:100000]
    s = G.gz(t, 6, 1)
    tuned(4096)
    assert gunzip(gpu_lib, s, cap=len(t) - 1)[0] == len(t)
    with pytest.raises(ValueError):
        engine.gunzip_stream(s, cap=1000)
    assert gunzip(gpu_lib, b'')[0] == b''
    assert engine.gunzip_stream(b'') == b''


# ---- 8. the reader -------------------------------------------------------------------------------------
def _same(a, b):
    assert (a.n, a.type) == (b.n, b.type)
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


@pytest.fixture(scope='module')
def text_file(tmp_path_factory):
    p = str(tmp_path_factory.mktemp('gzs') / 'reads.fastq.gz')
    with open(p, 'wb') as f:
        f.write(G.gz(G.text(), 6, 1))
    return p


def test_reader_loads_the_same(gpu_lib, tuned, text_file):
    from custom_porechop_abi_amd import engine, misc
    tuned(4096)
    for path in G.GOLDEN_GZ + [text_file]:
        for raw in (False, True):
            _same(misc.load_batch(path, raw=raw, gunzip_device=0, gunzip_plain=True), misc.load_batch(path, raw=raw))
        assert engine.gunzip_stream_stats()['dev_bytes'] > 0, path
    with pytest.raises(ValueError):
        misc.load_batch(text_file, gunzip_plain=True)
    with pytest.raises(ValueError):
        next(misc.read_batches(text_file, gunzip_plain=True))
    with pytest.raises(ValueError):
        next(misc.text_chunks(text_file, 1000, gunzip_plain=True))


def test_reader_batches_and_text_chunks(gpu_lib, tuned, text_file):
    from custom_porechop_abi_amd import misc
    tuned(4096, 65536)
    a = list(misc.read_batches(text_file, max_reads=17, gunzip_device=0, gunzip_plain=True))
    b = list(misc.read_batches(text_file, max_reads=17))
    assert len(a) == len(b) > 10
    for x, y in zip(a, b):
        _same(x, y)
    got = b''.join(bytes(mv) for mv in misc.text_chunks(text_file, 50000, gunzip_device=0, gunzip_plain=True))
    assert got == G.text()


def test_file_trimmer_reads_plain_gzip_on_device(gpu_lib, tuned, tmp_path):
    from custom_porechop_abi_amd.pipeline import FileTrimmer
    from tests.test_pipeline import _matching
    case = [c for c in golden_lib.g2()['cases'] if c['case'] == 'one_adapter_set'][0]
    o = case['opts']
    in_path = os.path.join(DATA, 'test_one_adapter_set.fastq.gz')
    tuned(4096)
    outs = {}
    for dev in (False, True):
        ft = FileTrimmer(_matching(case), o['scoring'], o['end_size'], o['end_threshold'], o['extra_end_trim'],
                         o['min_trim_size'], o['middle_threshold'], 10, 100, 1000, gunzip_on_device=dev, gunzip_plain=dev)
        try:
            out = str(tmp_path / ('out%d.fastq' % dev))
            counts = ft.trim_file(in_path, out, 'fastq', max_reads=7)
            stats = getattr(ft, 'gunzip_stream_stats', None)
        finally:
            ft.close()
        outs[dev] = (counts, open(out, 'rb').read())
    assert outs[True] == outs[False] and len(outs[True][1]) > 0
    assert stats is not None and stats['dev_bytes'] > 0, stats
    with pytest.raises(ValueError):
        FileTrimmer(_matching(case), o['scoring'], gunzip_plain=True)


def test_reader_damage_in_the_last_chunk(gpu_lib, tuned, tmp_path):
    """The records before the damage come out first, then the read error, as with the zlib reader."""
    from custom_porechop_abi_amd import _lib, misc
    s = bytearray(G.gz(G.text(), 6, 1))
    s[len(s) - 1500] ^= 0x10
    p = str(tmp_path / 'bad.fastq.gz')
    with open(p, 'wb') as f:
        f.write(bytes(s))
    tuned(4096, 65536)
    n, it = 0, misc.read_batches(p, max_reads=20, gunzip_device=0, gunzip_plain=True)
    with pytest.raises(ValueError):
        for b in it:
            n += b.n
    assert 'read error' in _lib.lib().pcabi_last_error().decode()
    # the damage lies in the last 1 % of the stream: the records wholly before it came out first
    assert 280 <= n <= 300, n
    with pytest.raises(ValueError):
        misc.load_batch(p, gunzip_device=0, gunzip_plain=True)
    with pytest.raises(ValueError):
        misc.load_batch(p)   # zlib refuses the file too
