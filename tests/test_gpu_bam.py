"""Unaligned BAM input on the device: k_bam_unpack against the host build of the same code and the
Python expectation (engine.bam_unpack), the reader on the device path (misc.load_batch / read_batches
gunzip_device=0) against the host path, and FileTrimmer end to end."""
import gzip
import os

import numpy as np
import pytest

from tests import bam_lib as B
from tests import golden_lib
from tests import inflate_cpu_lib as I

pytestmark = pytest.mark.gpu

DATA = os.path.join(golden_lib.GOLDEN, 'data')
GUARD = 64


@pytest.fixture(scope='module')
def corpus():
    recs = B.corpus_a()
    return recs, B.expected(recs)


@pytest.fixture
def tuned(gpu_lib):
    def tune(chunk_bytes=0):
        assert gpu_lib.pcabi_gunzip_tune(chunk_bytes) == 0
    yield tune
    assert gpu_lib.pcabi_gunzip_tune(0) == 0


def _write(tmp_path, name, data):
    p = str(tmp_path / name)
    with open(p, 'wb') as f:
        f.write(data)
    return p


def _last_error(L):
    return L.pcabi_last_error().decode()


# ---- 1. the kernel against the host template -----------------------------------------------------------
@pytest.mark.parametrize('shift', [0, 1, 7])
def test_kernel_matches_host_and_expected(gpu_lib, corpus, shift):
    """Corpus A through engine.bam_unpack on the device and with the host build. shift moves the
    outputs' starts off their 16-byte alignment, on the device too: pcabi_bam_unpack_host gives its
    device outputs the caller's misalignment. The device-side guard bytes are the library's (64 on
    either side of each device output, checked after the kernel, PCABI_E_DEVICE when touched); the numpy
    guards here see the host build's writes and the copy back."""
    from custom_porechop_abi_amd import engine
    recs, exp = corpus
    raw = B.raw_bam(recs, b'@HD\tVN:1.6\n', [(b'chr1', 1000)])
    keep = bytes(raw)
    table, totals = engine.bam_index(raw)
    got = {}
    for device in (0, -1):
        outs = [np.full(int(totals[k]) + 2 * GUARD + shift, 0xA5, np.uint8) for k in range(3)]
        views = tuple(o[GUARD + shift:o.size - GUARD] for o in outs)
        got[device] = engine.bam_unpack(raw, table, totals, device=device, out=views)
        for o in outs:
            assert (o[:GUARD + shift] == 0xA5).all() and (o[-GUARD:] == 0xA5).all(), 'wrote outside an output'
    assert raw == keep, 'input changed'
    for a, b in zip(got[0], got[-1]):
        assert np.array_equal(a, b)
    seq, qual, codes = got[0]
    assert seq.tobytes() == b''.join(exp['seq']) and qual.tobytes() == b''.join(exp['qual'])
    assert np.array_equal(codes, exp['codes'])


def test_kernel_leaves_unowned_bytes_alone(gpu_lib):
    """Outputs spread out with gaps between the records: the gaps keep their bytes."""
    from custom_porechop_abi_amd import engine
    recs = B.small_records(9, seed=8, lo=1, hi=9000)
    raw = B.raw_bam(recs)
    table, totals = engine.bam_index(raw)
    table = table.copy()
    table['seq_out'] += 13 * (1 + np.arange(table.size))
    table['qual_out'] += 29 * (1 + np.arange(table.size))
    table['code_out'] += 4 * (1 + np.arange(table.size))
    totals = totals.copy()
    totals[2] += 4 * (table.size + 1)                      # the tail padding after the last record's codes
    size = int(totals[2]) + 29 * (table.size + 1)
    got = {}
    for device in (0, -1):
        outs = tuple(np.full(size, 0xA5, np.uint8) for _ in range(3))
        got[device] = engine.bam_unpack(raw, table, totals, device=device, out=outs)
    e = B.expected(recs)
    for k, (field, off) in enumerate((('seq', 'seq_out'), ('qual', 'qual_out'))):
        assert np.array_equal(got[0][k], got[-1][k])
        owned = np.zeros(size, bool)
        for r, want in zip(table, e[field]):
            lo = int(r[off])
            assert got[0][k][lo:lo + len(want)].tobytes() == want
            owned[lo:lo + len(want)] = True
        assert (got[0][k][~owned] == 0xA5).all()
    assert np.array_equal(got[0][2], got[-1][2])
    owned = np.zeros(size, bool)
    owned[int(totals[2]) - 16:int(totals[2])] = True      # the tail padding
    for r in table:
        owned[int(r['code_out']):int(r['code_out']) + ((int(r['l_seq']) + 3) & ~3)] = True
    assert (got[0][2][~owned] == 0xA5).all() and (got[0][2][int(totals[2]) - 16:int(totals[2])] == 4).all()


# ---- 2. the reader on the device -----------------------------------------------------------------------
@pytest.mark.parametrize('chunk', [4096, 65536, 0])
@pytest.mark.parametrize('block_bytes,level', [(37, 0), (37, 6), (4096, 0), (4096, 6), (65280, 0), (65280, 6)])
def test_reader_on_device_matches_host_path(gpu_lib, tmp_path, tuned, corpus, block_bytes, level, chunk):
    from custom_porechop_abi_amd import misc
    recs, exp = corpus
    path = _write(tmp_path, 'a.bam', B.make_bam(recs, b'@HD\tVN:1.6\n', (), block_bytes, level))
    tuned(chunk)
    if chunk == 4096:   # the 70,001-base record spans many groups
        assert max(len(B.record_bytes(r)) for r in recs) > 3 * 4096
    dev = misc.load_batch(path, gunzip_device=0)
    tuned(0)
    B.assert_batch(dev, exp, 'device')
    B.assert_same(B.batch_views(dev), B.batch_views(misc.load_batch(path)), 'device against host')


def test_header_and_markers_on_device(gpu_lib, tmp_path, tuned, corpus):
    from custom_porechop_abi_amd import misc
    recs, exp = corpus
    text = b'@HD\tVN:1.6\n' + b''.join(b'@CO\tline %06d of a long header\n' % k for k in range(2200))
    refs = [(b'chr1', 248956422), (b'a_reference_with_a_longer_name', 5)]
    tuned(4096)
    for name, data in (('h.bam', B.make_bam(recs, text, refs, 4096)), ('m.bam', B.make_bam(recs, b'', (), 4096, 6, True, 3)),
                       ('n.bam', B.make_bam(recs, b'', (), 4096, 6, False))):
        B.assert_batch(misc.load_batch(_write(tmp_path, name, data), gunzip_device=0), exp, name)


# ---- 3. streaming --------------------------------------------------------------------------------------
@pytest.mark.parametrize('limits', [{'max_reads': 7}, {'max_bases': 1000}])
def test_batches_on_device(gpu_lib, tmp_path, tuned, limits):
    from custom_porechop_abi_amd import misc
    recs = B.small_records(50)
    path = _write(tmp_path, 'b.bam', B.make_bam(recs, b'', (), 3000))
    tuned(4096)
    dev = list(misc.read_batches(path, gunzip_device=0, **limits))
    host = list(misc.read_batches(path, **limits))
    assert [b.n for b in dev] == [b.n for b in host] and len(dev) > 3
    B.assert_same(B.concat_batches(dev), B.expected(recs))


# ---- 4. errors -----------------------------------------------------------------------------------------
def _faulty(path, gpu_lib, before, name):
    from custom_porechop_abi_amd import misc
    got = []
    with pytest.raises(ValueError):
        for b in misc.read_batches(path, max_reads=5, gunzip_device=0):
            got.append(b)
    assert _last_error(gpu_lib).startswith('read error:'), _last_error(gpu_lib)
    if before:
        B.assert_same(B.concat_batches(got), B.expected(before), name)
    else:
        assert got == []
    with pytest.raises(ValueError):
        misc.load_batch(path, gunzip_device=0)


@pytest.mark.parametrize('case', B.fault_cases(), ids=[c[0] for c in B.fault_cases()])
def test_faults_on_device(gpu_lib, tmp_path, tuned, case):
    name, raw, before = case
    tuned(4096)
    _faulty(_write(tmp_path, 'f.bam', B.bgzf(raw, 700)), gpu_lib, before, name)


def test_damaged_member_on_device(gpu_lib, tmp_path, tuned):
    """A BGZF member that does not inflate after the tenth record: ten records, then the read error."""
    recs = B.small_records(30, seed=9, lo=300, hi=400)
    head = B.raw_bam(recs[:10])
    rest = b''.join(B.record_bytes(r) for r in recs[10:])
    bad = bytearray(I.member(I.deflate_raw(rest[:600], 6), rest[:600]))
    bad[-6] ^= 0x40                                    # the CRC-32
    data = B.bgzf(head, 700, eof=False) + bytes(bad) + B.bgzf(rest[600:], 700)
    tuned(4096)
    _faulty(_write(tmp_path, 'd.bam', data), gpu_lib, recs[:10], 'damaged member')
    assert 'does not inflate' in _last_error(gpu_lib)


# ---- 5. end to end -------------------------------------------------------------------------------------
def test_file_trimmer_reads_bam(gpu_lib, tmp_path):
    """FileTrimmer on a BAM made from the golden reads: the output is the FASTQ run's, byte for byte, with
    the records unpacked on the device and on the host."""
    from custom_porechop_abi_amd import misc
    from custom_porechop_abi_amd.pipeline import FileTrimmer
    from tests.test_pipeline import _matching
    case = [c for c in golden_lib.g2()['cases'] if c['case'] == 'one_adapter_set'][0]
    o = case['opts']
    fq_path = os.path.join(DATA, 'test_one_adapter_set.fastq.gz')
    text = gzip.decompress(open(fq_path, 'rb').read())
    fq = misc.load_batch(fq_path)
    recs = [{'name': fq.name(i).encode(), 'seq': fq.sequence(i), 'qual': [ord(c) - 33 for c in fq.quals(i)], 'flag': 4}
            for i in range(fq.n)]
    assert fq.n > 7 and not fq.rna.any()
    paths = {'fastq': _write(tmp_path, 'in.fastq.gz', I.bgzf_zlib(text, 5000, 6)),
             'bam': _write(tmp_path, 'in.bam', B.make_bam(recs, b'@HD\tVN:1.6\tSO:unknown\n', (), 5000))}
    outs = {}
    for kind, dev in (('fastq', False), ('bam', True), ('bam', False)):
        ft = FileTrimmer(_matching(case), o['scoring'], o['end_size'], o['end_threshold'], o['extra_end_trim'],
                         o['min_trim_size'], o['middle_threshold'], 10, 100, 1000, gunzip_on_device=dev)
        try:
            out = str(tmp_path / ('out_%s_%d.fastq' % (kind, dev)))
            counts = ft.trim_file(paths[kind], out, 'fastq', max_reads=7)
        finally:
            ft.close()
        outs[kind, dev] = (counts, open(out, 'rb').read())
    assert outs['bam', True] == outs['fastq', False] == outs['bam', False] and len(outs['bam', True][1]) > 0
