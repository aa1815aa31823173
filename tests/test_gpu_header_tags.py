"""SAM tags in FASTQ / FASTA headers on the GPU: k_auxtext_size / k_auxtext_write / k_fastx_pack
(engine.auxtext_plan / auxtext_write / fastx_pack with device=0) against tests/header_tags_ref.py's
restatement, the text writer's device path (the text laid out and compressed on the device) against its
host path and against what out_format 'bam' writes, and FileTrimmer from a BAM to FASTQ with header_tags."""
import gzip
import signal

import pytest

from tests import golden_lib
from tests import header_tags_ref as H
from tests import test_header_tags_cpu as C

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _time_limit():
    """Every test of this file under its own time limit: a step that does not come back ends the test."""
    def expired(signum, frame):
        raise TimeoutError('a GPU step of this test took more than 120 s')
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(120)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


# ---- table level -------------------------------------------------------------------------------------------
def test_corpus_against_restatement(gpu_lib):
    C.check_table(C.chain_corpus(), 0)


def test_alignments(gpu_lib):
    C.check_alignments(0)


def test_refusals(gpu_lib):
    C.check_refusals(0)


def test_device_and_host_agree_on_every_byte(gpu_lib):
    chains = C.chain_corpus()
    assert C.run_table(chains, 0) == C.run_table(chains, -1)


@pytest.mark.parametrize('fasta', [False, True])
def test_fastx_pack(gpu_lib, fasta):
    C.check_fastx(fasta, 0)
    C.check_fastx(fasta, 0, skew=9)


# ---- file level: BAM in with tags, compressed text out ---------------------------------------------------------
@pytest.mark.parametrize('bgzf', [False, True])
@pytest.mark.parametrize('fmt', ['fastq.gz', 'fasta.gz'])
def test_bam_in_text_out(gpu_lib, tmp_path, fmt, bgzf):
    from custom_porechop_abi_amd import misc
    batch, base = C.file_case(tmp_path)
    plain = fmt[:-3]
    for vname, extra in C.variants(batch.n):
        for tags in (C.TAG_OPTIONS if vname == 'cuts' else C.TAG_OPTIONS[3:]):
            kw = dict(base, **extra)
            host = str(tmp_path / ('host.' + plain))
            misc.write_reads(batch, host, plain, keep_aux=True, header_tags=True, **kw, **tags)
            with open(host, 'rb') as f:
                host_text = f.read()
            C.check_file(tmp_path, batch, fmt, kw, tags, gzip_device=0, bgzf=bgzf, host_text=host_text)
    # two appended batches; with bgzf the finished file reads back through the device reader
    text = C.check_file(tmp_path, batch, fmt, base, C.TAG_OPTIONS[3], gzip_device=0, bgzf=bgzf, twice=True)
    if bgzf:
        back = misc.load_batch(str(tmp_path / ('tags.' + fmt)), gunzip_device=0)
        recs = H.split_records(text, fmt.startswith('fasta'))
        assert back.n == len(recs)
        for k, (head, seq, _) in enumerate(recs):
            assert back.seq[back.seq_off[k]:back.seq_off[k + 1]].tobytes() == seq
            assert back.names[back.name_off[k]:back.name_off[k + 1]].tobytes() == head.strip()


def test_option_off_writes_todays_bytes(gpu_lib, tmp_path):
    from custom_porechop_abi_amd import misc
    batch, base = C.file_case(tmp_path, 30)
    for bgzf in (False, True):
        a, b = str(tmp_path / 'a.fastq.gz'), str(tmp_path / 'b.fastq.gz')
        misc.write_reads(batch, a, 'fastq.gz', gzip_device=0, bgzf=bgzf, **base)
        misc.write_reads(batch, b, 'fastq.gz', gzip_device=0, bgzf=bgzf, header_tags=False, **base)
        with open(a, 'rb') as f, open(b, 'rb') as g:
            assert f.read() == g.read()


def test_long_header_spans_blocks(gpu_lib, tmp_path):
    """A header far longer than a deflate block (a 300 k-move table: a 600 kB line) and a read of several
    tiles, on the device against the host."""
    import numpy as np
    from custom_porechop_abi_amd import misc
    from tests import bam_lib as B
    from tests import test_moves_cpu as V
    rng = np.random.RandomState(3)
    n = 150000
    seq = ''.join(rng.choice(list('ACGT'), n))
    moves = [1, 0] * n
    aux = b'RGZgrp\0' + C.scalar(b'de', 'f', 0.03125) + V.mv_aux(6, moves) + V.ts_aux(100)
    src = str(tmp_path / 'long.bam')
    with open(src, 'wb') as f:
        f.write(B.make_bam([{'name': b'long', 'seq': seq, 'qual': [20] * n, 'flag': 4, 'aux': aux},
                            {'name': b'short', 'seq': 'ACGTACGT', 'qual': [20] * 8, 'flag': 4, 'aux': b'qsC\x07'}], b'@HD\tVN:1.6\n', (), 5000))
    batch = misc.load_batch(src, keep_aux=True)
    kw = dict(start_trim=[1000, 0], end_trim=[500, 0], keep_aux=True, keep_moves=True, header_tags=True)
    for fmt in ('fastq', 'fasta'):
        host, dev = str(tmp_path / ('h.' + fmt)), str(tmp_path / ('d.%s.gz' % fmt))
        misc.write_reads(batch, host, fmt, **kw)
        misc.write_reads(batch, dev, fmt + '.gz', gzip_device=0, **kw)
        with open(host, 'rb') as f, open(dev, 'rb') as g:
            text = f.read()
            assert gzip.decompress(g.read()) == text
        head = text.split(b'\n', 1)[0]
        assert head.startswith(b'@long\tRG:Z:grp\tde:f:0.03125\tmv:B:c,6,1,0' if fmt == 'fastq' else b'>long\tRG:Z:grp\tde:f:0.03125\tmv:B:c,6,1,0')
        assert head.endswith(b'\tts:i:%d' % (100 + 6 * 2000)) and len(head) > 590000


def test_bam_and_text_writers_keep_their_device_state_apart(gpu_lib, tmp_path, tmp_path_factory):
    """The BAM writer and the tagged text writer each keep a remap stage on the device between calls. One
    process, one small batch (a dozen reads of at most 200 bases with MM / ML and mv / ts, both trims and a
    split): BAM, then tagged fastq.gz, then BAM again, all on the device. Each file inflates to what the host
    path writes for the same options, and the second BAM is the first byte for byte."""
    from custom_porechop_abi_amd import misc
    from tests import test_writer_errors_cpu as W
    batch, base = W.case(tmp_path_factory)
    kw = dict(base, keep_aux=True, keep_mods=True, keep_moves=True)

    def written(name, fmt, gzip_device, **more):
        path = str(tmp_path / name)
        assert misc.write_reads(batch, path, fmt, gzip_device=gzip_device, **kw, **more) == batch.n
        with open(path, 'rb') as f:
            return f.read()

    bam1 = written('dev1.bam', 'bam', 0)
    text = written('dev.fastq.gz', 'fastq.gz', 0, header_tags=True)
    bam2 = written('dev2.bam', 'bam', 0)
    host_bam = gzip.decompress(written('host.bam', 'bam', None))
    host_text = gzip.decompress(written('host.fastq.gz', 'fastq.gz', None, header_tags=True))
    assert b'\tMM:Z:' in host_text and b'\tmv:B:c,' in host_text and b'read5_2' in host_text
    assert gzip.decompress(bam1) == host_bam
    assert gzip.decompress(text) == host_text
    assert bam2 == bam1


# ---- the pipeline -----------------------------------------------------------------------------------------------
def test_file_trimmer_header_tags(gpu_lib, tmp_path):
    """FileTrimmer(keep_tags, header_tags) from a .bam to .fastq: record by record the header parses to the
    tags of the record its own BAM output holds."""
    from custom_porechop_abi_amd import misc
    from tests.test_gpu_bam_pack import _trimmer
    from tests.test_gpu_moves import _golden_moves_bam
    case = [c for c in golden_lib.g2()['cases'] if c['case'] == 'one_adapter_set'][0]
    src, reads = _golden_moves_bam(tmp_path, 'test_one_adapter_set.fastq.gz')
    outs = {}
    for name, fmt, kw in (('bam', 'bam', {}), ('fq', 'fastq', {'header_tags': True}), ('gz', 'fastq.gz', {'header_tags': True}),
                          ('today', 'fastq', {})):
        ft = _trimmer(case, filter_reads=False, gzip_on_device=True, gunzip_on_device=True, keep_tags=True, keep_moves=True, **kw)
        try:
            ft.trim_file(src, str(tmp_path / (name + '.' + fmt)), fmt, max_reads=7)
        finally:
            ft.close()
        outs[name] = str(tmp_path / (name + '.' + fmt))
    back = misc.load_batch(outs['bam'], gunzip_device=0, keep_aux=True)
    text = C.read_text(outs['fq'], 'fastq')
    assert C.read_text(outs['gz'], 'fastq.gz') == text
    recs, old = H.split_records(text, False), H.split_records(C.read_text(outs['today'], 'fastq'), False)
    assert len(recs) == len(old) == back.n and back.n > 7
    moved = 0
    for k, (head, seq, qual) in enumerate(recs):
        name, fields = H.parse_header(head)
        assert (name, seq, qual) == old[k]
        assert fields == H.expected_fields(back.aux(k))
        moved += any(t == b'mv' for t, _, _ in fields)
    assert moved > 7
