"""Block-gzipped (BGZF) FASTA / FASTQ input read through the GPU (pcabi_fastx_open_dev;
misc.load_batch / read_batches / text_chunks gunzip_device=..., FileTrimmer(gunzip_on_device=True)):
the same batches, field by field, as the zlib path gives on the same file."""
import glob
import gzip
import json
import os

import numpy as np
import pytest

from tests import golden_lib
from tests import inflate_cpu_lib as I

pytestmark = pytest.mark.gpu

DATA = os.path.join(golden_lib.GOLDEN, 'data')
G3 = json.load(gzip.open(os.path.join(golden_lib.GOLDEN, 'g3_io.json.gz'), 'rt'))
FIELDS = ('name_off', 'seq_off', 'qual_off', 'spacer_off', 'names', 'seq', 'qual', 'spacer', 'rna', 'codes',
          'code_off', 'lengths')


def _text(path):
    raw = open(path, 'rb').read()
    return gzip.decompress(raw) if raw[:2] == b'\x1f\x8b' else raw


def _same(a, b):
    assert (a.n, a.type) == (b.n, b.type)
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


@pytest.fixture
def tuned(gpu_lib):
    def tune(chunk_bytes=0):
        assert gpu_lib.pcabi_gunzip_tune(chunk_bytes) == 0
    yield tune
    assert gpu_lib.pcabi_gunzip_tune(0) == 0


def _texts():
    paths = set(glob.glob(os.path.join(DATA, '*.gz'))) | set(os.path.join(golden_lib.GOLDEN, c['file']) for c in G3['cases'])
    return [p for p in sorted(paths) if os.path.isfile(p)]


def test_golden_texts_load_the_same(gpu_lib, tmp_path, tuned):
    """Every golden FASTA / FASTQ text (the universal-newline and no-final-terminator fixtures of
    test_io.py among them) re-blocked to BGZF by zlib, in whole blocks and in blocks so small that
    records straddle members, refill groups of one member included."""
    from custom_porechop_abi_amd import misc
    paths = _texts()
    assert len(paths) >= 8
    seen = 0
    for k, path in enumerate(paths):
        text = _text(path)
        if not text or text[:1] not in (b'>', b'@'):
            continue
        seen += 1
        for block, chunk in ((65280, 0), (257, 0), (97, 1) if len(text) < 5000 else (1021, 3000)):
            p = str(tmp_path / ('t%d_%d.gz' % (k, block)))
            z = I.bgzf_zlib(text, block, 6)
            open(p, 'wb').write(z)
            assert I.index(z) != 0
            tuned(chunk)
            for raw in (False, True):
                _same(misc.load_batch(p, raw=raw, gunzip_device=0), misc.load_batch(p, raw=raw))
            tuned(0)
        # and by this project's own encoder: fixed blocks, and the writer's line-aligned ones
        from custom_porechop_abi_amd import engine
        for j, blocks in enumerate((None, engine.gzip_line_blocks(text, cap=engine.BGZF_BLOCK_CAP))):
            p = str(tmp_path / ('e%d_%d.gz' % (k, j)))
            open(p, 'wb').write(engine.bgzf_compress(text, blocks))
            for raw in (False, True):
                _same(misc.load_batch(p, raw=raw, gunzip_device=0), misc.load_batch(p, raw=raw))
    assert seen >= 8


def test_streaming_batches_and_text_chunks(gpu_lib, tmp_path, tuned):
    from custom_porechop_abi_amd import misc
    text = I.fastq_text(400000, 21)
    text = text[:text.rindex(b'\n@') + 1]
    p = str(tmp_path / 'reads.fastq.gz')
    open(p, 'wb').write(I.bgzf_zlib(text, 30000, 1))
    tuned(70000)     # a few members per refill group, several groups
    a = [b for b in misc.read_batches(p, max_reads=50, gunzip_device=0)]
    b = [b for b in misc.read_batches(p, max_reads=50)]
    assert len(a) == len(b) > 5
    for x, y in zip(a, b):
        _same(x, y)
    got = b''.join(bytes(mv) for mv in misc.text_chunks(p, 50000, gunzip_device=0))
    assert got == text
    tuned(0)
    _same(misc.load_batch(p, gunzip_device=0), misc.load_batch(p))


def test_not_indexable_falls_back(gpu_lib, tmp_path):
    from custom_porechop_abi_amd import misc
    text = I.fastq_text(50000, 22)
    text = text[:text.rindex(b'\n@') + 1]
    plain, gz = str(tmp_path / 'a.fastq'), str(tmp_path / 'a.fastq.gz')
    open(plain, 'wb').write(text)
    open(gz, 'wb').write(gzip.compress(text))
    ref = misc.load_batch(plain)
    _same(misc.load_batch(gz, gunzip_device=0), ref)
    _same(misc.load_batch(plain, gunzip_device=0), ref)


def test_damaged_member_is_the_readers_error(gpu_lib, tmp_path, tuned):
    """The records before the damaged member come out first, then the reader's read error."""
    from custom_porechop_abi_amd import _lib, misc
    lines = I.fastq_text(200000, 23).split(b'\n')
    recs = [b'\n'.join(lines[k:k + 4]) + b'\n' for k in range(0, len(lines) - 4, 4)]
    # members of 40 whole records: the damaged one starts at a record start, so the parser meets the
    # read error between records (inside a record it reports a truncated record, as with zlib)
    parts = [b''.join(recs[k:k + 40]) for k in range(0, len(recs), 40)]
    assert len(parts) > 8
    z = bytearray(b''.join(I.member(I.deflate_raw(q), q) for q in parts) + I.EOF_MARKER)
    in_off, _ = I.index(bytes(z))
    z[in_off[6] + 300] ^= 0x40
    p = str(tmp_path / 'bad.fastq.gz')
    open(p, 'wb').write(bytes(z))
    for chunk in (0, 45000):
        tuned(chunk)
        with pytest.raises(ValueError):
            misc.load_batch(p, gunzip_device=0)
        msg = _lib.lib().pcabi_last_error().decode()
        assert 'read error' in msg and 'member 6 ' in msg
        n, it = 0, misc.read_batches(p, max_reads=20, gunzip_device=0)
        with pytest.raises(ValueError):
            for b in it:
                n += b.n
        assert n == 240      # the six sound members' records came out first
    with pytest.raises(ValueError):
        misc.load_batch(p)   # zlib refuses the file too


def test_file_trimmer_reads_bgzf_on_device(gpu_lib, tmp_path):
    from custom_porechop_abi_amd.pipeline import FileTrimmer
    from tests.test_pipeline import _matching
    case = [c for c in golden_lib.g2()['cases'] if c['case'] == 'one_adapter_set'][0]
    o = case['opts']
    text = _text(os.path.join(DATA, 'test_one_adapter_set.fastq.gz'))
    in_path = str(tmp_path / 'in.fastq.gz')
    open(in_path, 'wb').write(I.bgzf_zlib(text, 5000, 6))
    outs = {}
    for dev in (False, True):
        ft = FileTrimmer(_matching(case), o['scoring'], o['end_size'], o['end_threshold'], o['extra_end_trim'],
                         o['min_trim_size'], o['middle_threshold'], 10, 100, 1000, gunzip_on_device=dev)
        try:
            out = str(tmp_path / ('out%d.fastq' % dev))
            counts = ft.trim_file(in_path, out, 'fastq', max_reads=7)
        finally:
            ft.close()
        outs[dev] = (counts, open(out, 'rb').read())
    assert outs[True] == outs[False] and len(outs[True][1]) > 0


def test_file_trimmer_bgzf_out_and_back_in(gpu_lib, tmp_path):
    """FileTrimmer(gzip_on_device, bgzf, gunzip_on_device) on the G2 input re-blocked to BGZF: the
    output decompresses to the plain run's bytes, is indexable, ends with the marker, and read back
    in gives the same records."""
    from custom_porechop_abi_amd import engine, misc
    from custom_porechop_abi_amd.pipeline import FileTrimmer
    from tests.test_pipeline import _matching
    case = [c for c in golden_lib.g2()['cases'] if c['case'] == 'one_adapter_set'][0]
    o = case['opts']
    text = _text(os.path.join(DATA, 'test_one_adapter_set.fastq.gz'))
    in_path = str(tmp_path / 'in.fastq.gz')
    open(in_path, 'wb').write(engine.bgzf_compress(text))
    outs = {}
    for dev in (False, True):
        fmt = 'fastq.gz' if dev else 'fastq'
        ft = FileTrimmer(_matching(case), o['scoring'], o['end_size'], o['end_threshold'], o['extra_end_trim'],
                         o['min_trim_size'], o['middle_threshold'], 10, 100, 1000, gzip_on_device=dev, bgzf=dev,
                         gunzip_on_device=dev)
        try:
            out = str(tmp_path / ('out.' + fmt))
            counts = ft.trim_file(in_path, out, fmt, max_reads=7)      # several batches appended
        finally:
            ft.close()
        outs[dev] = (counts, open(out, 'rb').read(), out)
    z = outs[True][1]
    assert outs[True][0] == outs[False][0] and len(outs[False][1]) > 0
    assert gzip.decompress(z) == outs[False][1]
    idx = engine.bgzf_index(z)
    assert idx is not None and len(idx[0]) - 1 >= 3       # a member or more per appended batch, and the marker
    assert z[-28:] == engine.BGZF_EOF and z.count(engine.BGZF_EOF) == 1
    assert engine.gunzip(z) == outs[False][1]
    _same(misc.load_batch(outs[True][2], gunzip_device=0), misc.load_batch(outs[False][2]))
    with pytest.raises(ValueError):
        FileTrimmer(_matching(case), o['scoring'], bgzf=True)
    with pytest.raises(ValueError):
        misc.write_reads(misc.load_batch(outs[False][2]), str(tmp_path / 'x.fastq.gz'), 'fastq.gz', bgzf=True)


def test_write_reads_bgzf_appends_and_finishes(gpu_lib, tmp_path):
    from custom_porechop_abi_amd import engine, misc
    b = misc.load_batch(os.path.join(DATA, 'test_two_adapter_sets.fastq.gz'))
    plain, z = str(tmp_path / 'a.fastq'), str(tmp_path / 'a.fastq.gz')
    for k in range(2):
        misc.write_reads(b, plain, 'fastq', append=k > 0)
        misc.write_reads(b, z, 'fastq.gz', append=k > 0, gzip_device=0, bgzf=True)
    raw = open(z, 'rb').read()
    assert engine.BGZF_EOF not in raw and engine.bgzf_index(raw) is not None
    misc.bgzf_finish(z)
    raw = open(z, 'rb').read()
    assert raw[-28:] == engine.BGZF_EOF and gzip.decompress(raw) == open(plain, 'rb').read()
    assert engine.gunzip(raw) == open(plain, 'rb').read()
    _same(misc.load_batch(z, gunzip_device=0), misc.load_batch(plain))
