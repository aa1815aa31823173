"""Unaligned BAM output on the host path (no GPU): the pack half of the record layer (csrc/pcabi_bam.h)
through engine.bam_pack(device=-1), the writer (misc.write_reads(..., 'bam', gzip_device=None)) and the
aux tags a BAM reader keeps, byte for byte against tests/bam_lib.py's record_bytes / header_bytes and
Python's zlib."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import bam_lib as B
from tests import bam_pack_lib as P

HERE = os.path.dirname(os.path.abspath(__file__))


def _write(tmp_path, name, data):
    p = str(tmp_path / name)
    with open(p, 'wb') as f:
        f.write(data)
    return p


# ---- 1. engine.bam_pack against record_bytes ---------------------------------------------------------
def test_corpus_covers_what_it_claims():
    seq, qual, side, parts, records = P.pack_corpus()
    assert set(parts['l_seq']) == set(P.L_SEQ)
    assert set(parts['name_len']) == set(P.NAME_LEN) and set(parts['aux_len']) == set(P.AUX_LEN)
    planned, _ = P.planned_with_gaps(parts)
    assert set(int(o) % 16 for o in planned['out']) == set(range(16))
    assert set(int(o) % 16 for o in planned['seq_src']) == set(range(16))
    letters = set(seq.tobytes().decode('latin-1'))
    assert set(B.LETTERS + 'Uacgtn.') <= letters
    assert set(''.join(r['seq'] for r in records)) == set(B.LETTERS)
    assert (parts['qual_src'] < 0).any() and set(range(33, 127)) | {32, 0x80, 0xFF} <= set(qual.tolist())


def test_pack_host_matches_record_bytes():
    from custom_porechop_abi_amd import engine
    seq, qual, side, parts, records = P.pack_corpus()
    planned, end = P.planned_with_gaps(parts)
    out = np.full(end + 7, 0xA5, np.uint8)
    engine.bam_pack(seq, qual, side, planned, out, device=-1)
    exp = P.expected_image(planned, records, out.size)
    bad = np.flatnonzero(out != exp)
    assert bad.size == 0, (bad[:8], out[bad[:8]], exp[bad[:8]])


def test_pack_chain_is_a_bam_the_reader_walks():
    """The planned chain behind a header is what engine.bam_index walks and bam_unpack gives back."""
    from custom_porechop_abi_amd import engine
    seq, qual, side, parts, records = P.pack_corpus()
    head = B.header_bytes(b'@HD\tVN:1.6\n')
    planned = parts.copy()
    end, _ = engine.bam_pack_plan(planned, len(head))
    out = np.zeros(end, np.uint8)
    out[:len(head)] = np.frombuffer(head, np.uint8)
    engine.bam_pack(seq, qual, side, planned, out, device=-1)
    assert out.tobytes() == head + b''.join(B.record_bytes(r) for r in records)
    recs, totals = engine.bam_index(out)
    assert recs.size == len(records)
    s, q, _ = engine.bam_unpack(out, recs, totals, device=-1)
    names, es, eq = P.reads_of(records)
    assert s.tobytes() == b''.join(es) and q.tobytes() == b''.join(eq)


def test_pack_refuses_bad_tables():
    from custom_porechop_abi_amd import engine
    from custom_porechop_abi_amd._lib import PcabiError
    seq, qual, side, parts, _ = P.pack_corpus()
    planned = parts[:4].copy()
    end, _ = engine.bam_pack_plan(planned)
    out = np.zeros(end, np.uint8)
    for field, value in (('seq_src', seq.size), ('qual_src', qual.size), ('side_off', side.size), ('out', 1), ('tile0', 5),
                         ('l_seq', -1), ('name_len', 255), ('aux_len', -1)):
        bad = planned.copy()
        bad[field][3] = value
        with pytest.raises(PcabiError):
            engine.bam_pack(seq, qual, side, bad, out, device=-1)
    with pytest.raises(PcabiError):
        engine.bam_pack(seq, qual, side, planned, out[:-1].copy(), device=-1)
    long_name = planned.copy()
    long_name['name_len'][0] = 255
    with pytest.raises(PcabiError):
        engine.bam_pack_plan(long_name)


# ---- 2. the writer -----------------------------------------------------------------------------------
def check_bam_file(path, header, text, absent_quals, n_bam, n_fq, load_kw=None):
    """Everything a written file must be, from the FASTQ text the existing writer gave for the same
    arguments. Returns the decoded stream."""
    from custom_porechop_abi_amd import misc
    with open(path, 'rb') as f:
        data = f.read()
    assert data[-28:] == B.EOF_MARKER
    mem = P.members(data[:-28])
    assert all(1 <= len(d) <= P.BLOCK for _, d in mem) and all(len(m) <= 65536 for m, _ in mem)
    stream = b''.join(d for _, d in mem)
    records = P.records_of_fastq(text, absent_quals)
    chunks = [B.record_bytes(r) for r in records]
    assert stream == B.header_bytes(P.DEFAULT_HEADER if header is None else header) + b''.join(chunks)
    assert n_bam == n_fq
    back = misc.load_batch(path, **(load_kw or {}))
    assert P.batch_reads(back) == P.reads_of(records)
    return mem, stream


@pytest.mark.parametrize('variant', P.VARIANTS)
@pytest.mark.parametrize('kind', ['fastq', 'fasta', 'bam'])
def test_writer_host_path(tmp_path, kind, variant):
    path, header, text, n_bam, n_fq = P.write_two_batches(tmp_path, kind, variant, None, 'h')
    mem, stream = check_bam_file(path, header, text, kind == 'fasta', n_bam, n_fq)
    assert len(mem) >= 3 and len(stream) >= 200000
    # the first batch's members are full but its last; a record lies across a member edge
    assert len(mem[0][1]) == P.BLOCK and len(mem[1][1]) == P.BLOCK
    edges = set(np.cumsum([len(d) for _, d in mem]).tolist())
    at, spans = len(B.header_bytes(P.DEFAULT_HEADER if header is None else header)), 0
    while at < len(stream):
        size = 4 + int.from_bytes(stream[at:at + 4], 'little')
        spans += any(at < e < at + size for e in edges)
        at += size
    assert at == len(stream) and spans >= 1
    if variant == 'split':
        assert any(h.split(b' ')[0].split(b'\t')[0].endswith(b'_2') for h, _, _ in P.parse_fastq(text))


def test_writer_names_and_empty_batches(tmp_path):
    """Names: cut at the first space or tab, to 254 bytes, '*' when empty. A batch that writes no record
    still writes the header on a first write, and nothing on an appended one."""
    from custom_porechop_abi_amd import misc
    long = b'n' * 300
    src = _write(tmp_path, 'n.fastq', b'@' + long + b' c\nACGT\n+\nIIII\n@ lead\nAC\n+\nII\n@t\tx y\nACG\n+\nIII\n')
    b = misc.load_batch(src)
    out = str(tmp_path / 'n.bam')
    assert misc.write_reads(b, out, 'bam') == 3
    assert misc.write_reads(b, out, 'bam', append=True, select=np.zeros(3, np.uint8)) == 0
    misc.bgzf_finish(out)
    with open(out, 'rb') as f:
        data = f.read()
    mem = P.members(data[:-28])
    assert len(mem) == 1
    q = [40] * 4
    exp = [{'name': long[:254], 'seq': 'ACGT', 'qual': q}, {'name': b'*', 'seq': 'AC', 'qual': q[:2]},
           {'name': b't', 'seq': 'ACG', 'qual': q[:3]}]
    assert mem[0][1] == B.header_bytes(P.DEFAULT_HEADER) + b''.join(B.record_bytes(r) for r in exp)
    only = str(tmp_path / 'e.bam')
    assert misc.write_reads(b, only, 'bam', select=np.zeros(3, np.uint8), bam_header=b'@CO\tx\n') == 0
    with open(only, 'rb') as f:
        mem = P.members(f.read())
    assert [d for _, d in mem] == [B.header_bytes(b'@CO\tx\n')]


def test_header_only_file(tmp_path):
    """misc.write_bam_header (what FileTrimmer writes for an input without reads): a BAM the reader takes,
    with the header and no record."""
    from custom_porechop_abi_amd import misc
    for k, text in enumerate((None, b'@HD\tVN:1.6\n@RG\tID:x\n')):
        path = str(tmp_path / ('empty%d.bam' % k))
        misc.write_bam_header(path, text)
        misc.bgzf_finish(path)
        with open(path, 'rb') as f:
            data = f.read()
        assert data[-28:] == B.EOF_MARKER
        assert [d for _, d in P.members(data[:-28])] == [B.header_bytes(P.DEFAULT_HEADER if text is None else text)]
        b = misc.load_batch(path)
        assert b.n == 0 and b.bam_header == (P.DEFAULT_HEADER if text is None else text)


# ---- 3. aux tags -------------------------------------------------------------------------------------
RG, MM = b'RGZgroup\0', b'MMZC+m,1,2;\0'     # bam_lib.corpus_a's first and last tag (qs lies between)


def _aux_case(tmp_path):
    from custom_porechop_abi_amd import misc
    recs = B.corpus_a()
    src = _write(tmp_path, 'a.bam', B.make_bam(recs, b'@HD\tVN:1.6\n@RG\tID:group\n'))
    kept = B.kept(recs)
    st = np.array([(0, 0, 3, 1)[i % 4] for i in range(len(kept))], np.int32)
    return misc, recs, src, kept, st


def test_aux_tags_kept_and_filtered(tmp_path):
    misc, recs, src, kept, st = _aux_case(tmp_path)
    b = misc.load_batch(src, keep_aux=True)
    assert b.n == len(kept) and b.bam_header == b'@HD\tVN:1.6\n@RG\tID:group\n'
    for i, r in enumerate(kept):
        assert b.aux(i) == r.get('aux', b'') and b.as_stored[i] == (0 if r['flag'] & 0x10 else 1)
    got = [x for bb in misc.read_batches(src, max_reads=7, keep_aux=True) for x in (bb.aux(i) for i in range(bb.n))]
    assert got == [r.get('aux', b'') for r in kept]
    out = str(tmp_path / 'o.bam')
    misc.write_reads(b, out, 'bam', start_trim=st, bam_header=b.bam_header, keep_aux=True)
    misc.bgzf_finish(out)
    exp_reads = B.expected(recs)
    exp, seen = [], set()
    for i, r in enumerate(kept):
        seq = exp_reads['seq'][i][int(st[i]):]
        if not seq:
            continue
        aux = b''
        if 'aux' in r:
            whole = st[i] == 0 and not r['flag'] & 0x10
            assert r['aux'].startswith(RG + b'qsC') and r['aux'].endswith(MM) and len(r['aux']) == len(RG) + 4 + len(MM)
            aux = r['aux'] if whole else r['aux'][:-len(MM)]
            seen.add(('whole' if whole else 'trimmed' if not r['flag'] & 0x10 else 'reverse'))
        exp.append({'name': r['name'], 'seq': seq.decode(), 'qual': P.phred(exp_reads['qual'][i][int(st[i]):]), 'aux': aux})
    assert seen == {'whole', 'trimmed', 'reverse'}
    with open(out, 'rb') as f:
        data = f.read()
    stream = b''.join(d for _, d in P.members(data[:-28]))
    # (absent qualities read as '+' and are written back as Phred 10)
    assert stream == B.header_bytes(b.bam_header) + b''.join(B.record_bytes(r) for r in exp)
    back = misc.load_batch(out, keep_aux=True)
    assert [back.aux(i) for i in range(back.n)] == [r['aux'] for r in exp]


def test_no_tags_without_keep_aux(tmp_path):
    misc, recs, src, kept, st = _aux_case(tmp_path)
    b = misc.load_batch(src)
    assert b.aux(0) is None and b.aux_off is None and b.as_stored is None
    out = str(tmp_path / 'o.bam')
    misc.write_reads(b, out, 'bam', keep_aux=True)      # nothing kept: nothing to write
    kept_b = misc.load_batch(src, keep_aux=True)
    out2 = str(tmp_path / 'o2.bam')
    misc.write_reads(kept_b, out2, 'bam', keep_aux=False)
    for path in (out, out2):
        misc.bgzf_finish(path)
        back = misc.load_batch(path, keep_aux=True)
        assert back.n == sum(1 for r in kept if r['seq']) and all(back.aux(i) == b'' for i in range(back.n))
    fq = _write(tmp_path, 'x.fastq', b'@a\nACGT\n+\nIIII\n')
    assert misc.load_batch(fq, keep_aux=True).aux(0) is None     # not BAM: the switch does nothing
    assert [x.aux_off for x in misc.read_batches(fq, keep_aux=True)] == [None]


def test_broken_aux_chain_raises_after_the_records_before_it(tmp_path):
    from custom_porechop_abi_amd import misc
    good = B.small_records(12, seed=5)
    for r in good[::2]:
        r['aux'] = b'RGZg\0' + b'XBBs' + b'\x02\x00\x00\x00' + b'\x01\x00\x02\x00'
    for k, aux in enumerate((b'RGZgroup', b'qsC', b'XXQ\0', b'XBBz\0\0\0\0', b'XBBi\x05\0\0\0' + b'\0' * 19)):
        bad = {'name': b'bad', 'seq': 'ACGTACGTAC', 'qual': [20] * 10, 'aux': aux}
        src = _write(tmp_path, 'f%d.bam' % k, B.make_bam(good + [bad] + B.small_records(3, seed=9)))
        assert misc.load_batch(src).n == 16                       # not kept: not walked
        with pytest.raises(ValueError, match='aux'):
            misc.load_batch(src, keep_aux=True)
        it = misc.read_batches(src, max_reads=5, keep_aux=True)
        seen = 0
        with pytest.raises(ValueError, match='aux'):
            for b in it:
                seen += b.n
        assert seen == 12


def test_sharded_runs_refuse_bam_output(tmp_path):
    from custom_porechop_abi_amd import shards
    with pytest.raises(ValueError, match='BAM output'):
        shards.trim_file_sharded(os.path.join(HERE, 'nothing.fastq'), str(tmp_path / 'o.bam'), 'bam')


# ---- 4. the record layer alone, under sanitizers -----------------------------------------------------
def test_pack_layer_under_sanitizers(tmp_path):
    """tests/bam_pack_fuzz_main.cpp (csrc/pcabi_bam.h alone), built with -fsanitize=address,undefined as
    a program of its own and run as a child process: random part tables against a byte-wise
    restatement, the kernel's piece walk at every misalignment, pack then unpack, and the aux walk."""
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path / 'bam_pack_fuzz')
    base = ['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
            os.path.join(HERE, 'bam_pack_fuzz_main.cpp')]
    for extra in (['-static-libasan', '-static-libubsan'], []):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        if r.returncode == 0:
            break
    if r.returncode != 0 and ('asan' in r.stderr or 'ubsan' in r.stderr or 'sanitize' in r.stderr):
        pytest.skip('the sanitizer runtime cannot be linked')
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, '1', '1500'], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'rounds 1500' in r.stdout
