"""The trimmed-read writer with gzip compressed on the GPU (pcabi_reads_write_dev, gz = 2;
misc.write_reads(gzip_device=...), FileTrimmer(gzip_on_device=True)): the file decompresses to the
bytes the plain writer writes for the same arguments, the project's reader reads it back, and the
streams are small enough (the size bars of the device encoder against zlib)."""
import gzip
import os
import zlib

import numpy as np
import pytest

from tests import golden_lib
from tests.test_gpu_deflate import members

pytestmark = pytest.mark.gpu

DATA = os.path.join(golden_lib.GOLDEN, 'data')


@pytest.fixture(scope='module')
def batches(gpu_lib):
    from custom_porechop_abi_amd import misc
    return {name: misc.load_batch(os.path.join(DATA, name)) for name in
            ('test_one_adapter_set.fastq.gz', 'test_barcodes.fastq.gz', 'test_choose_barcodes_1.fasta.gz')}


@pytest.fixture(scope='module')
def rna_batch(gpu_lib, tmp_path_factory):
    from custom_porechop_abi_amd import misc
    rng = np.random.default_rng(11)
    path = str(tmp_path_factory.mktemp('rna') / 'rna.fastq')
    with open(path, 'wb') as f:
        for k, n in enumerate([30, 1500, 2600, 4000, 1]):
            seq = bytes(rng.choice(np.frombuffer(b'ACGU', np.uint8), n))
            f.write(b'@rna%d some text\n' % k + seq + b'\n+\n' + bytes(rng.integers(38, 73, n, dtype=np.uint8)) + b'\n')
    b = misc.load_batch(path)
    assert b.n == 5
    return b


def _both(tmp_path, b, fmt, **kw):
    """write_reads plain and on the device with the same arguments: (plain bytes, gzip bytes)."""
    from custom_porechop_abi_amd import misc
    plain, gz = str(tmp_path / ('p.' + fmt)), str(tmp_path / ('d.' + fmt + '.gz'))
    for p in (plain, gz):
        if os.path.exists(p):
            os.remove(p)
    e0 = misc.write_reads(b, plain, fmt, **kw)
    e1 = misc.write_reads(b, gz, fmt + '.gz', gzip_device=0, **kw)
    assert e0 == e1                                   # reads emitted
    text, z = open(plain, 'rb').read(), open(gz, 'rb').read()
    assert gzip.decompress(z) == text
    assert b''.join(members(z)) == text
    return text, z, gz


def _trims(b, seed):
    rng = np.random.default_rng(seed)
    lens = np.array([len(b.sequence(i)) for i in range(b.n)])
    st = rng.integers(0, 60, b.n).astype(np.int32)
    et = rng.integers(0, 60, b.n).astype(np.int32)
    st[::5] = 0
    et[::7] = 0
    st[1::11] = lens[1::11] + 5                       # trimmed away entirely: no record
    return st, et, lens


def _cuts(lens, st, et, seed):
    """Middle cut ranges on about half the reads, some splitting into parts under min_split."""
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(lens):
        tl = max(0, int(n) - int(st[i]) - int(et[i]))
        if i % 2 == 0 or tl < 50:
            out.append([])
            continue
        k = int(rng.integers(1, 4))
        pts = np.sort(rng.integers(0, tl, 2 * k))
        out.append([(int(pts[2 * j]), int(pts[2 * j + 1])) for j in range(k)])
    return out


@pytest.mark.parametrize('name', ['test_one_adapter_set.fastq.gz', 'test_barcodes.fastq.gz'])
def test_write_reads_cases(batches, name, tmp_path):
    from custom_porechop_abi_amd import misc
    b = batches[name]
    st, et, lens = _trims(b, 1)
    cuts = _cuts(lens, st, et, 2)
    text, _, _ = _both(tmp_path, b, 'fastq')                                        # no trims
    assert text.count(b'\n') == 4 * b.n
    _both(tmp_path, b, 'fastq', start_trim=st, end_trim=et)                         # start and end trims
    split, _, _ = _both(tmp_path, b, 'fastq', start_trim=st, end_trim=et, middle_cuts=cuts, min_split_read_size=100)
    assert b'_2' in split                                                           # reads were split
    _both(tmp_path, b, 'fastq', start_trim=st, end_trim=et, middle_cuts=cuts, discard_middle=True)
    sel = (np.arange(b.n) % 3 != 0).astype(np.uint8)
    _both(tmp_path, b, 'fastq', start_trim=st, end_trim=et, middle_cuts=cuts, select=sel)
    _both(tmp_path, b, 'fastq', start_trim=st, end_trim=et, middle_cuts=cuts, untrimmed=True)
    fa, _, _ = _both(tmp_path, b, 'fasta', start_trim=st, end_trim=et)              # FASTA, 70 columns
    assert fa.startswith(b'>')
    # an empty selection: a valid gzip file of nothing, no reads emitted
    text, z, _ = _both(tmp_path, b, 'fastq', select=np.zeros(b.n, np.uint8))
    assert text == b'' and len(z) > 0
    # the project's reader reads the device-compressed file back to the same records
    text, z, gz_path = _both(tmp_path, b, 'fastq', start_trim=st, end_trim=et)
    plain_path = str(tmp_path / 'p.fastq')
    rec = lambda bb: [(bb.name(i), bb.sequence(i), bb.quals(i)) for i in range(bb.n)]
    got = [r for bb in misc.read_batches(gz_path, max_reads=5) for r in rec(bb)]
    exp = [r for bb in misc.read_batches(plain_path, max_reads=5) for r in rec(bb)]
    assert got == exp and len(got) > 0


def test_write_reads_fasta_input_and_rna(batches, rna_batch, tmp_path):
    b = batches['test_choose_barcodes_1.fasta.gz']
    _both(tmp_path, b, 'fasta')
    _both(tmp_path, b, 'fastq')
    text, _, _ = _both(tmp_path, rna_batch, 'fastq')
    assert b'U' in text and b'T' not in text.split(b'\n')[1]                         # RNA reads keep their U
    _both(tmp_path, rna_batch, 'fastq', start_trim=np.array([3, 10, 0, 7, 0], np.int32),
          end_trim=np.array([3, 10, 9, 0, 0], np.int32), middle_cuts=[[], [(500, 600)], [(1000, 1100)], [], []],
          min_split_read_size=300)
    _both(tmp_path, rna_batch, 'fasta')


def test_append_adds_members(batches, tmp_path):
    from custom_porechop_abi_amd import misc
    b = batches['test_one_adapter_set.fastq.gz']
    st, et, _ = _trims(b, 3)
    plain, gz = str(tmp_path / 'a.fastq'), str(tmp_path / 'a.fastq.gz')
    first = (np.arange(b.n) % 2 == 0).astype(np.uint8)
    for k, sel in enumerate((first, 1 - first)):
        e0 = misc.write_reads(b, plain, 'fastq', st, et, select=sel, append=k > 0)
        e1 = misc.write_reads(b, gz, 'fastq.gz', st, et, select=sel, append=k > 0, gzip_device=0)
        assert e0 == e1 > 0
    text, z = open(plain, 'rb').read(), open(gz, 'rb').read()
    assert gzip.decompress(z) == text and len(members(z)) >= 2
    # and not appending truncates
    misc.write_reads(b, gz, 'fastq.gz', st, et, select=first, gzip_device=0)
    misc.write_reads(b, plain, 'fastq', st, et, select=first)
    assert gzip.decompress(open(gz, 'rb').read()) == open(plain, 'rb').read()


def test_default_gz_path_unchanged(batches, tmp_path):
    """gzip_device=None keeps the zlib path: one member, the same text."""
    from custom_porechop_abi_amd import misc
    b = batches['test_one_adapter_set.fastq.gz']
    p = str(tmp_path / 'z.fastq.gz')
    misc.write_reads(b, p, 'fastq.gz')
    z = open(p, 'rb').read()
    misc.write_reads(b, str(tmp_path / 'z.fastq'), 'fastq')
    assert len(members(z)) == 1 and gzip.decompress(z) == open(str(tmp_path / 'z.fastq'), 'rb').read()


def _g2_case(name):
    return [c for c in golden_lib.g2()['cases'] if c['case'] == name][0]


def test_file_trimmer_on_device(gpu_lib, tmp_path):
    from custom_porechop_abi_amd.pipeline import FileTrimmer
    from tests.test_pipeline import _matching
    case = _g2_case('one_adapter_set')
    o = case['opts']
    in_path = os.path.join(DATA, 'test_one_adapter_set.fastq.gz')
    outs = {}
    for dev in (False, True):
        fmt = 'fastq.gz' if dev else 'fastq'
        ft = FileTrimmer(_matching(case), o['scoring'], o['end_size'], o['end_threshold'], o['extra_end_trim'],
                         o['min_trim_size'], o['middle_threshold'], 10, 100, 1000, gzip_on_device=dev)
        try:
            counts = ft.trim_file(in_path, str(tmp_path / ('out.' + fmt)), fmt, max_reads=7)   # several batches
        finally:
            ft.close()
        outs[dev] = (counts, open(str(tmp_path / ('out.' + fmt)), 'rb').read())
    assert outs[True][0] == outs[False][0]
    assert len(outs[False][1]) > 0 and gzip.decompress(outs[True][1]) == outs[False][1]
    assert len(members(outs[True][1])) > 1            # a batch appends members


def test_file_trimmer_barcode_bins_on_device(gpu_lib, tmp_path):
    from custom_porechop_abi_amd.pipeline import FileTrimmer
    from tests.test_pipeline import _matching
    case = _g2_case('barcodes')
    o = case['opts']
    in_path = os.path.join(DATA, 'test_barcodes.fastq.gz')
    bins = {}
    for dev in (False, True):
        fmt = 'fastq.gz' if dev else 'fastq'
        bdir = str(tmp_path / ('bins%d' % dev))
        ft = FileTrimmer(_matching(case), o['scoring'], o['end_size'], o['end_threshold'], o['extra_end_trim'],
                         o['min_trim_size'], o['middle_threshold'], 10, 100, 1000, barcode_dir=bdir,
                         forward_or_reverse_barcodes=case['forward_or_reverse'],
                         require_two_barcodes=bool(o.get('require_two')), gzip_on_device=dev)
        try:
            counts = ft.trim_file(in_path, str(tmp_path / 'unused'), fmt, max_reads=3)
        finally:
            ft.close()
        bins[dev] = ({k: v[1] for k, v in counts['bins'].items()}, {f[:-len(fmt) - 1]: open(os.path.join(bdir, f), 'rb').read()
                                      for f in sorted(os.listdir(bdir))})
    assert bins[True][0] == bins[False][0] and sorted(bins[True][1]) == sorted(bins[False][1]) and bins[False][1]
    for name, text in bins[False][1].items():
        assert gzip.decompress(bins[True][1][name]) == text, name


def _bench_fastq(n_reads, mean_len, seed):
    """FASTQ text made the way the benchmark's e2e workload writes its input (bench.py write_fastq):
    synthetic reads, ONT-like headers, qualities uniform in 5..39."""
    from custom_porechop_abi_amd import synth
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b'ACGTN', np.uint8)
    parts = []
    for k, r in enumerate(synth.make_reads(n_reads, mean_len, seed=12345)):
        q = (rng.integers(5, 40, len(r)) + 33).astype(np.uint8).tobytes()
        parts.append(b'@read%d runid=synthetic ch=%d\n' % (k, k % 512) + letters[r].tobytes() + b'\n+\n' + q + b'\n')
    return b''.join(parts)


def test_stream_sizes_against_zlib(gpu_lib):
    """Line-aligned blocks: no larger than zlib level 6. Fixed blocks: at most 1.05 x zlib's
    Z_HUFFMAN_ONLY. (CPU estimates with optimal lengths: 0.92 x and 1.015 x.)"""
    from custom_porechop_abi_amd import engine
    text = _bench_fastq(300, 8000, 99)
    assert len(text) >= 2 * 1000 * 1000
    lined = engine.gzip_compress(text, engine.gzip_line_blocks(text))
    fixed = engine.gzip_compress(text)
    assert gzip.decompress(lined) == text and gzip.decompress(fixed) == text
    z6 = len(zlib.compress(text, 6))
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
    zh = len(c.compress(text) + c.flush())
    print('gzip sizes: text %d, zlib-6 %d, huffman-only %d, device line-aligned %d (%.4f x zlib-6), '
          'device fixed %d (%.4f x huffman-only)' % (len(text), z6, zh, len(lined), len(lined) / z6, len(fixed),
                                                     len(fixed) / zh))
    assert len(lined) <= z6
    assert len(fixed) <= 1.05 * zh
