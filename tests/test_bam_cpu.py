"""Unaligned BAM input on the host path (no GPU): the record layer (csrc/pcabi_bam.h) through
misc.load_batch / read_batches, engine.bam_index and engine.bam_unpack(device=-1), against the
expected batches tests/bam_lib.py computes in Python from the record lists."""
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

from tests import bam_lib as B

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def corpus():
    recs = B.corpus_a()
    return recs, B.expected(recs)


def _write(tmp_path, name, data):
    p = str(tmp_path / name)
    with open(p, 'wb') as f:
        f.write(data)
    return p


def _last_error():
    from custom_porechop_abi_amd._lib import lib
    return lib().pcabi_last_error().decode()


# ---- 1. corpus A -------------------------------------------------------------------------------------
def test_corpus_covers_what_it_claims(corpus):
    recs, exp = corpus
    assert set(B.L_SEQ) <= set(len(r['seq']) for r in recs)
    starts = set((36 + len(r['name']) + 1 + 4 * r.get('n_cigar', 0)) % 16 for r in recs)
    assert starts == set(range(16))
    assert set(''.join(r['seq'] for r in recs)) == set(B.LETTERS)
    assert set(q for r in recs if r.get('qual') for q in r['qual']) == set(range(94))
    assert any(r.get('qual') is None for r in recs) and sum('aux' in r for r in recs) >= len(recs) // 2 - 1
    rev = [len(r['seq']) % 2 for r in B.kept(recs) if r['flag'] & 0x10]
    assert 0 in rev and 1 in rev
    assert len(B.kept(recs)) == len(recs) - 2 and b'secondary' not in exp['names'] and b'supplementary' not in exp['names']


def test_corpus_through_load_batch(tmp_path, corpus):
    from custom_porechop_abi_amd import misc
    recs, exp = corpus
    path = _write(tmp_path, 'a.bam', B.make_bam(recs, b'@HD\tVN:1.6\tSO:unknown\n'))
    B.assert_batch(misc.load_batch(path), exp)
    B.assert_batch(misc.load_batch(path, raw=True), exp, 'raw')
    got = B.concat_batches(list(misc.read_batches(path)))
    B.assert_same(got, exp, 'read_batches')


def test_corpus_through_the_direct_abi(corpus):
    from custom_porechop_abi_amd import engine
    recs, exp = corpus
    raw = B.raw_bam(recs, b'@HD\tVN:1.6\n', [(b'chr1', 1000)])
    table, totals = engine.bam_index(raw)
    assert table.size == len(exp['names'])
    assert np.array_equal(table['l_seq'], exp['len']) and np.array_equal(table['code_out'], exp['code_off'])
    assert totals[0] == totals[1] == int(exp['len'].sum()) and totals[2] == exp['codes'].size
    assert totals[3] == sum(len(n) for n in exp['names'])
    names = [raw[int(r['rec']) + 36:int(r['rec']) + 36 + int(r['name_len'])] for r in table]
    assert names == exp['names']
    keep = bytes(raw)
    guard = 64
    outs = [np.full(int(totals[k]) + 2 * guard, 0xA5, np.uint8) for k in range(3)]
    seq, qual, codes = engine.bam_unpack(raw, table, totals, device=-1, out=tuple(o[guard:o.size - guard] for o in outs))
    for o in outs:
        assert (o[:guard] == 0xA5).all() and (o[-guard:] == 0xA5).all(), 'wrote outside an output'
    assert raw == keep
    assert seq.tobytes() == b''.join(exp['seq']) and qual.tobytes() == b''.join(exp['qual'])
    assert np.array_equal(codes, exp['codes'])


def test_letters_and_codes_follow_the_fastq_reader(tmp_path, corpus):
    """2. the records a FASTQ can hold, written as FASTQ and read by the FASTQ reader: every view equal."""
    from custom_porechop_abi_amd import misc
    recs, _ = corpus
    text, keep = B.fastq_text(recs)
    assert len(keep) >= 35
    fq = misc.load_batch(_write(tmp_path, 'a.fastq', text))
    bam = misc.load_batch(_write(tmp_path, 'a.bam', B.make_bam(keep)))
    B.assert_batch(bam, B.expected(keep))
    B.assert_same(B.batch_views(bam), B.batch_views(fq), 'bam against fastq')
    assert np.array_equal(bam.rna, fq.rna) and np.array_equal(bam.seq_off, fq.seq_off)
    assert np.array_equal(bam.qual_off, fq.qual_off) and np.array_equal(bam.name_off, fq.name_off)
    recs_raw, kind = misc.load_fasta_or_fastq(_write(tmp_path, 'b.bam', B.make_bam(keep[:5])))
    e = B.expected(keep[:5])
    assert kind == 'FASTQ'
    assert recs_raw == [(n.decode().split()[0], s.decode(), '', q.decode(), n.decode())
                        for n, s, q in zip(e['names'], e['seq'], e['qual'])]


# ---- 3. blocking -------------------------------------------------------------------------------------
@pytest.mark.parametrize('block_bytes', [37, 4096, 65280])
@pytest.mark.parametrize('level', [0, 6])
def test_blocking(tmp_path, corpus, block_bytes, level):
    from custom_porechop_abi_amd import misc
    recs, exp = corpus
    path = _write(tmp_path, 'a.bam', B.make_bam(recs, b'@HD\tVN:1.6\n', (), block_bytes, level))
    B.assert_batch(misc.load_batch(path), exp)


def test_header_spanning_members_and_eof_markers(tmp_path, corpus):
    from custom_porechop_abi_amd import misc
    recs, exp = corpus
    text = b'@HD\tVN:1.6\n' + b''.join(b'@CO\tline %06d of a long header\n' % k for k in range(2200))
    assert len(text) > 70000
    refs = [(b'chr1', 248956422), (b'a_reference_with_a_longer_name', 5)]
    B.assert_batch(misc.load_batch(_write(tmp_path, 'h.bam', B.make_bam(recs, text, refs, 4096))), exp, 'long header')
    B.assert_batch(misc.load_batch(_write(tmp_path, 'm.bam', B.make_bam(recs, b'', (), 4096, 6, True, 3))), exp, 'marker inside')
    B.assert_batch(misc.load_batch(_write(tmp_path, 'n.bam', B.make_bam(recs, b'', (), 4096, 6, False))), exp, 'no marker')


# ---- 4. batching -------------------------------------------------------------------------------------
@pytest.mark.parametrize('limits', [{'max_reads': 7}, {'max_bases': 1000}])
def test_batches_concatenate_to_the_whole_file(tmp_path, limits):
    from custom_porechop_abi_amd import misc
    recs = B.small_records(50)
    path = _write(tmp_path, 'b.bam', B.make_bam(recs, b'', (), 3000))
    batches = list(misc.read_batches(path, **limits))
    assert len(batches) > 3
    if 'max_reads' in limits:
        assert [b.n for b in batches] == [7] * 7 + [1]
    else:   # a batch ends with the record that reaches max_bases
        for b in batches[:-1]:
            assert int(b.lengths.sum()) >= 1000 > int(b.lengths[:-1].sum())
    B.assert_same(B.concat_batches(batches), B.expected(recs))
    B.assert_batch(misc.load_batch(path), B.expected(recs))


# ---- 5. errors ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', B.fault_cases(), ids=[c[0] for c in B.fault_cases()])
def test_faults_come_after_the_records_before_them(tmp_path, case):
    from custom_porechop_abi_amd import misc
    name, raw, before = case
    path = _write(tmp_path, 'f.bam', B.bgzf(raw, 700))
    it = misc.read_batches(path, max_reads=5)
    got = []
    with pytest.raises(ValueError):
        for b in it:
            got.append(b)
    assert _last_error().startswith('read error:'), _last_error()
    if before:
        B.assert_same(B.concat_batches(got), B.expected(before), name)
    else:
        assert got == []
    with pytest.raises(ValueError):     # the whole-file loaders do not return a partial batch
        misc.load_batch(path)
    assert _last_error().startswith('read error:')


def test_index_refuses_damaged_chains():
    from custom_porechop_abi_amd import engine
    from custom_porechop_abi_amd._lib import PcabiError
    for name, raw, _ in B.fault_cases():
        with pytest.raises(PcabiError):
            engine.bam_index(raw)


def test_unpack_refuses_a_table_outside_the_buffers():
    from custom_porechop_abi_amd import engine
    from custom_porechop_abi_amd._lib import PcabiError
    raw = B.raw_bam(B.small_records(3))
    table, totals = engine.bam_index(raw)
    for field, value in (('rec', len(raw)), ('l_seq', 1 << 20), ('seq_out', int(totals[0])), ('code_out', -4)):
        bad = table.copy()
        bad[field][1] = value
        with pytest.raises(PcabiError):
            engine.bam_unpack(raw, bad, totals, device=-1)


# ---- 6. refusals -------------------------------------------------------------------------------------
def test_text_chunks_and_sharded_runs_refuse_bam(tmp_path):
    from custom_porechop_abi_amd import misc, shards
    path = _write(tmp_path, 'r.bam', B.make_bam(B.small_records(4)))
    with pytest.raises(ValueError, match='BAM'):
        next(misc.text_chunks(path, 1 << 20))
    with pytest.raises(ValueError, match='BAM'):
        shards.trim_file_sharded(path, str(tmp_path / 'out.fastq'))
    assert misc.is_bam(path) and not misc.is_bam(_write(tmp_path, 'x.fastq', b'@a\nAC\n+\n!!\n'))
    assert misc.input_files(path) == [(path, None)]
    from custom_porechop_abi_amd._lib import lib
    import ctypes
    L = misc._declare(lib())
    h = ctypes.c_void_p()
    assert L.pcabi_fastx_open(os.fsencode(path), 0, ctypes.byref(h)) == 0
    try:
        assert L.pcabi_fastx_type(h) == misc.FASTQ and L.pcabi_fastx_remaining(h) == -1
        assert L.pcabi_fastx_set_range(h, 0, 10) == -1 and L.pcabi_fastx_record_start(h, 0) == -1
    finally:
        L.pcabi_fastx_close(h)


def test_cli_reads_bam(tmp_path):
    """load_reads, the CLI's loader: a BAM is a FASTQ read type, so the 'auto' output format is fastq."""
    from custom_porechop_abi_amd import misc
    recs = B.small_records(6)
    path = _write(tmp_path, 'c.bam', B.make_bam(recs))
    reads, check_reads, read_type = misc.load_reads(path, 0, None, 3)
    e = B.expected(recs)
    assert read_type == 'FASTQ' and len(check_reads) == 3
    assert [(r.name, r.seq, r.quals) for r in reads] == [(n.decode(), s.decode(), q.decode())
                                                         for n, s, q in zip(e['names'], e['seq'], e['qual'])]


# ---- 7. sanitizer-built mutation run -----------------------------------------------------------------
def test_mutations_under_sanitizers(tmp_path):
    """tests/bam_fuzz_main.cpp (csrc/pcabi_bam.h alone), built with -fsanitize=address,undefined as a
    program of its own and run as a child process over seeded mutations of a small record buffer."""
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path / 'bam_fuzz')
    base = ['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
            os.path.join(HERE, 'bam_fuzz_main.cpp')]
    for extra in (['-static-libasan', '-static-libubsan'], []):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        if r.returncode == 0:
            break
    if r.returncode != 0 and ('asan' in r.stderr or 'ubsan' in r.stderr or 'sanitize' in r.stderr):
        pytest.skip('the sanitizer runtime cannot be linked')
    assert r.returncode == 0, r.stderr
    recs = [r for r in B.corpus_a() if len(r['seq']) <= 300][:24] + B.small_records(4, lo=500, hi=700)
    seed = _write(tmp_path, 'seed.bin', B.raw_bam(recs, b'@HD\tVN:1.6\n', [(b'chr1', 1000)]))
    r = subprocess.run([exe, seed, '1', '4000'], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'mutations 4000' in r.stdout
