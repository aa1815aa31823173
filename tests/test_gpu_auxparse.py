"""SAM tags read from FASTQ / FASTA headers on the GPU: k_auxparse_size / k_auxparse_write (engine.auxparse_plan /
auxparse_write / aux_parse with device=0) against tests/auxparse_ref.py's restatement and against the host
build, the reader's device path (plain FASTQ, ordinary gzip inflated on the device, BGZF) against the same
reads read from BAM, one header longer than any pass structure, and FileTrimmer from a FASTQ with tags in its
headers against the equivalent BAM."""
import signal

import numpy as np
import pytest

from tests import golden_lib
from tests import test_auxparse_cpu as C
from tests import test_header_tags_cpu as HT

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
def test_literal_vectors(gpu_lib):
    from custom_porechop_abi_amd import engine
    got = engine.aux_parse([b'read 1 comment\t' + f for f, _ in C.LITERALS], 0)
    for (f, want), g in zip(C.LITERALS, got):
        assert g == (want or b''), (f, g, want)


def test_corpus_against_restatement(gpu_lib):
    C.check_table(C.header_corpus(), 0)


def test_alignments(gpu_lib):
    C.check_alignments(0)


def test_refusals(gpu_lib):
    C.check_refusals(0)


def test_round_trip_through_the_formatter(gpu_lib):
    C.check_round_trip(0)


def test_device_and_host_agree_on_every_byte(gpu_lib):
    headers = C.header_corpus()
    dev, host = C.run_table(headers, 0), C.run_table(headers, -1)
    assert dev[1:] == host[1:]                        # the table, both counters, the gaps
    # (a NaN's bytes are the host's strtod's on both sides: the device leaves floats to it)
    assert dev[0] == host[0]


def test_long_header(gpu_lib):
    """One header longer than any pass structure: a 300,000-move table, a 600 kB line. Device against host."""
    from custom_porechop_abi_amd import engine
    moves = np.random.RandomState(3).randint(0, 2, 300000)
    head = b'long runid=abc\tRG:Z:grp\tde:f:0.03125\tmv:B:c,6' + b''.join(b',%d' % m for m in moves.tolist()) + b'\tts:i:100'
    assert len(head) > 600000
    dev, host = engine.aux_parse([head, b'short\tqs:i:7'], 0), engine.aux_parse([head, b'short\tqs:i:7'], -1)
    assert dev == host
    assert dev[0][:22] == b'RGZgrp\0def\x00\x00\x00\x3dmvBc\xe1\x93\x04\x00' and dev[0][22] == 6
    assert dev[0][23:23 + 300000] == bytes(moves.tolist()) and dev[0][-4:] == b'tsCd' and dev[1] == b'qsC\x07'


# ---- file level: the reader's device path -----------------------------------------------------------------------
def test_text_in_matches_bam_in(gpu_lib, tmp_path):
    """The input as plain FASTQ, as .gz with gunzip_plain, and as BGZF through gunzip_device=0: the batch read
    with tags_from_headers on the device holds what the host build reads, and writes what the batch read
    from BAM writes."""
    from custom_porechop_abi_amd import engine, misc
    from_bam, base = C.file_case(tmp_path)
    src = str(tmp_path / 'src.fastq')
    host = misc.load_batch(src, keep_aux=True, tags_from_headers=True)
    gz, bg = str(tmp_path / 'plain.fastq.gz'), str(tmp_path / 'bgzf.fastq.gz')
    misc.write_reads(from_bam, gz, 'fastq.gz', keep_aux=True, header_tags=True)
    misc.write_reads(from_bam, bg, 'fastq.gz', keep_aux=True, header_tags=True, gzip_device=0, bgzf=True)
    misc.bgzf_finish(bg)
    cuts = [v for v in HT.variants(from_bam.n) if v[0] in ('cuts', 'select')]
    for path, kw in ((src, {}), (gz, {'gunzip_plain': True}), (bg, {})):
        engine.auxparse_counts(reset=True)
        dev = misc.load_batch(path, keep_aux=True, tags_from_headers=True, gunzip_device=0, **kw)
        tags, left = engine.auxparse_counts(reset=True)
        assert tags > 4 * dev.n and left == 0
        assert [dev.aux(i) for i in range(dev.n)] == [host.aux(i) for i in range(host.n)]
        C.check_files(tmp_path, from_bam, dev, base, ('fastq', 'bam'), variants=HT.variants(from_bam.n) if path == src else cuts)
    # batches of a streamed read, and the device writer behind the device reader
    got = [b.aux(i) for b in misc.read_batches(bg, max_reads=7, keep_aux=True, tags_from_headers=True, gunzip_device=0) for i in range(b.n)]
    assert got == [host.aux(i) for i in range(host.n)]
    C.check_files(tmp_path, from_bam, dev, base, ('fastq.gz',), variants=cuts, gzip_device=0, bgzf=True)


# ---- the pipeline -----------------------------------------------------------------------------------------------
def _forward_moves_bam(tmp_path, fq_name):
    """The golden reads as a BAM whose records carry RG, ts, a move table made for each read, ns, qs and de,
    every record forward-strand: what a FASTQ with these tags in its headers is equivalent to."""
    import os
    import struct
    from custom_porechop_abi_amd import misc
    from tests import bam_lib as B
    from tests import test_moves_cpu as V
    from tests.test_gpu_moves import DATA
    fq = misc.load_batch(os.path.join(DATA, fq_name))
    rng = np.random.RandomState(9)
    recs = []
    for i in range(fq.n):
        seq = fq.sequence(i)
        moves = V.make_moves(rng, len(seq), 2.0, lead=int(rng.randint(0, 30)))
        aux = (b'RGZgrp\0' + V.ts_aux(10 + i, 'i') + V.mv_aux(5 + i % 2, moves) + b'nsi' + struct.pack('<i', 99999) + b'qsC' + bytes([i % 200]) +
               b'def' + struct.pack('<f', 0.03125 * i))
        recs.append({'name': fq.name(i).split()[0].encode(), 'seq': seq, 'qual': [ord(c) - 33 for c in fq.quals(i)], 'flag': 4, 'aux': aux})
    path = str(tmp_path / 'in.bam')
    with open(path, 'wb') as f:
        f.write(B.make_bam(recs, b'@HD\tVN:1.6\tSO:unknown\n@RG\tID:grp\n', (), 5000))
    return path


def test_file_trimmer_tags_from_headers(gpu_lib, tmp_path):
    """FileTrimmer(keep_tags, tags_from_headers, header_tags, gzip_on_device, gunzip_on_device) run on a FASTQ
    with tags in its headers and on the equivalent BAM: the decompressed outputs are identical."""
    from custom_porechop_abi_amd import misc
    from tests.test_gpu_bam_pack import _trimmer
    case = [c for c in golden_lib.g2()['cases'] if c['case'] == 'one_adapter_set'][0]
    bam = _forward_moves_bam(tmp_path, 'test_one_adapter_set.fastq.gz')
    batch = misc.load_batch(bam, keep_aux=True)
    assert bool(batch.as_stored.all())
    fq = str(tmp_path / 'tagged.fastq.gz')
    misc.write_reads(batch, fq, 'fastq.gz', keep_aux=True, header_tags=True, gzip_device=0, bgzf=True)
    misc.bgzf_finish(fq)
    outs = {}
    for name, src, kw in (('bam', bam, {}), ('fq', fq, {'tags_from_headers': True})):
        ft = _trimmer(case, filter_reads=False, gzip_on_device=True, gunzip_on_device=True, keep_tags=True, keep_moves=True, header_tags=True, **kw)
        try:
            ft.trim_file(src, str(tmp_path / (name + '.fastq.gz')), 'fastq.gz', max_reads=7)
        finally:
            ft.close()
        outs[name] = HT.read_text(str(tmp_path / (name + '.fastq.gz')), 'fastq.gz')
    assert outs['fq'] == outs['bam'] and outs['bam'].count(b'\tmv:B:c,') > 7
