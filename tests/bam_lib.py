"""A pure-Python BAM writer and the expected batch of a record list, for the BAM input tests
(test_bam_cpu.py, test_gpu_bam.py). TEST INFRASTRUCTURE ONLY: nothing here is computed by the code
under test.

A record is a dict: name (bytes, without the NUL), seq (str over '=ACMGRSVTWYHKDBN'), qual (a list of
Phred values, or None for absent qualities: 0xFF bytes), flag (int), n_cigar (int), aux (bytes after
the qualities)."""
import itertools
import struct
import zlib

import numpy as np

from . import inflate_cpu_lib as icl

LETTERS = '=ACMGRSVTWYHKDBN'
COMPLEMENT = dict(zip('=ACMGRSVTWYHKDBN', '=TGKCYSBAWRDMHVN'))
EOF_MARKER = icl.EOF_MARKER


def record_bytes(r, block_size=None):
    """One BAM record with its block_size prefix (block_size: a value to write instead of the true one)."""
    seq, name = r['seq'], r['name']
    n_cigar = r.get('n_cigar', 0)
    code = [LETTERS.index(c) for c in seq] + ([0] if len(seq) % 2 else [])
    packed = bytes(code[i] << 4 | code[i + 1] for i in range(0, len(code), 2))
    qual = bytes([0xFF] * len(seq)) if r.get('qual') is None else bytes(r['qual'])
    assert len(qual) == len(seq)
    cigar = b''.join(struct.pack('<I', (7 + k) << 4 | 4) for k in range(n_cigar))
    body = struct.pack('<iiBBHHHiiii', -1, -1, r.get('l_read_name', len(name) + 1), 0, 4680, n_cigar, r.get('flag', 4),
                       r.get('l_seq', len(seq)), -1, -1, 0) + name + b'\0' + cigar + packed + qual + r.get('aux', b'')
    return struct.pack('<i', len(body) if block_size is None else block_size) + body


def header_bytes(header_text=b'', refs=(), version=1):
    out = b'BAM' + bytes([version]) + struct.pack('<i', len(header_text)) + header_text + struct.pack('<i', len(refs))
    for name, length in refs:
        out += struct.pack('<i', len(name) + 1) + name + b'\0' + struct.pack('<i', length)
    return out


def raw_bam(records, header_text=b'', refs=(), version=1):
    """The inflated bytes of a BAM file."""
    return header_bytes(header_text, refs, version) + b''.join(record_bytes(r) for r in records)


def bgzf(data, block_bytes=65280, level=6, eof=True, eof_after=None):
    """data as BGZF members of block_bytes decoded bytes each (framing: inflate_cpu_lib.bgzf_header);
    eof: the end-of-file marker at the end; eof_after: a member index after which one more marker goes."""
    out, k = [], 0
    for lo in range(0, len(data), block_bytes):
        piece = data[lo:lo + block_bytes]
        out.append(icl.member(icl.deflate_raw(piece, level), piece))
        k += 1
        if eof_after is not None and k == eof_after:
            out.append(EOF_MARKER)
    return b''.join(out) + (EOF_MARKER if eof else b'')


def make_bam(records, header_text=b'', refs=(), block_bytes=65280, level=6, eof=True, eof_after=None):
    return bgzf(raw_bam(records, header_text, refs), block_bytes, level, eof, eof_after)


def kept(records):
    return [r for r in records if not r.get('flag', 4) & 0x900]


def expected(records):
    """The batch a record list must give, by the rules of the record layer: names, seq, qual (lists of
    bytes), codes (uint8, 4-aligned starts, padding and 16 tail bytes of 4), code_off, len."""
    names, seqs, quals, code_off, lens = [], [], [], [], []
    codes = []
    at = 0
    for r in kept(records):
        seq, qual = r['seq'], r.get('qual')
        if r.get('flag', 4) & 0x10:
            seq = ''.join(COMPLEMENT[c] for c in reversed(seq))
            qual = None if qual is None else list(reversed(qual))
        names.append(r['name'])
        seqs.append(seq.encode())
        quals.append(b'+' * len(seq) if qual is None or (len(qual) and qual[0] == 0xFF) else bytes(q + 33 for q in qual))
        c = np.full((len(seq) + 3) & ~3, 4, np.uint8)
        c[:len(seq)] = [{'A': 0, 'C': 1, 'G': 2, 'T': 3}.get(ch, 4) for ch in seq]
        codes.append(c)
        code_off.append(at)
        lens.append(len(seq))
        at += c.size
    codes.append(np.full(16, 4, np.uint8))
    return {'names': names, 'seq': seqs, 'qual': quals, 'codes': np.concatenate(codes),
            'code_off': np.array(code_off, np.int64), 'len': np.array(lens, np.int32)}


def batch_views(b):
    """A ReadBatch in the shape of expected()."""
    n = b.n
    cut = lambda buf, off: [buf[off[i]:off[i + 1]].tobytes() for i in range(n)]   # noqa: E731
    return {'names': cut(b.names, b.name_off), 'seq': cut(b.seq, b.seq_off), 'qual': cut(b.qual, b.qual_off),
            'codes': np.array(b.codes), 'code_off': np.array(b.code_off), 'len': np.array(b.lengths)}


def assert_same(got, exp, what=''):
    for key in ('names', 'seq', 'qual'):
        assert len(got[key]) == len(exp[key]), (what, key, len(got[key]), len(exp[key]))
        for i, (a, b) in enumerate(zip(got[key], exp[key])):
            assert a == b, (what, key, i, a[:40], b[:40])
    for key in ('len', 'code_off', 'codes'):
        assert np.array_equal(got[key], exp[key]), (what, key)


def assert_batch(b, exp, what=''):
    from custom_porechop_abi_amd import misc
    assert b.type == misc.FASTQ
    assert_same(batch_views(b), exp, what)
    assert not b.rna.any() and b.spacer.size == 0 and not b.spacer_off.any()
    assert np.array_equal(b.seq_off, b.qual_off)


def concat_batches(batches):
    """Several batches' views as one (code offsets re-based, each batch's 16 tail bytes dropped)."""
    out = {'names': [], 'seq': [], 'qual': []}
    codes, code_off, lens, at = [], [], [], 0
    for b in batches:
        v = batch_views(b)
        for key in out:
            out[key] += v[key]
        assert v['codes'].size >= 16 and (v['codes'][-16:] == 4).all()
        codes.append(v['codes'][:-16])
        code_off.append(v['code_off'] + at)
        lens.append(v['len'])
        at += v['codes'].size - 16
    out['codes'] = np.concatenate(codes + [np.full(16, 4, np.uint8)])
    out['code_off'] = np.concatenate(code_off) if code_off else np.zeros(0, np.int64)
    out['len'] = np.concatenate(lens) if lens else np.zeros(0, np.int32)
    return out


L_SEQ = [0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097, 8193,
         70001]
_corpus = None


def corpus_a():
    """The shared record corpus: every l_seq of L_SEQ; qname lengths 1..9 and 254 crossed with 0..3
    CIGAR operations (the sequence start hits every residue mod 16); all 16 codes; qualities 0..93; one
    record without qualities; aux tags in half the records; reverse-strand records of odd and even
    length; one secondary and one supplementary record, which must be absent from the batch."""
    global _corpus
    if _corpus is not None:
        return _corpus
    rng = np.random.RandomState(11)
    recs = []
    for i, (qlen, n_cigar) in enumerate(itertools.product(list(range(1, 10)) + [254], range(4))):
        ln = L_SEQ[i % len(L_SEQ)]
        seq = ''.join(LETTERS[c] for c in rng.randint(0, 16, ln))
        if ln >= 16:
            seq = LETTERS + seq[16:]
        qual = [int(q) for q in rng.randint(0, 94, ln)]
        if ln >= 94:
            qual[:94] = range(94)
        name = bytes(rng.randint(48, 123, qlen).astype(np.uint8)).replace(b'@', b'a')
        flag = 4 | (0x10 if ln in (3, 16, 33, 257, 4096, 8193, 70001) else 0)
        rec = {'name': name, 'seq': seq, 'qual': qual, 'flag': flag, 'n_cigar': n_cigar}
        if i % 2:
            rec['aux'] = b'RGZgroup\0' + b'qsC' + bytes([i]) + b'MMZC+m,1,2;\0'
        recs.append(rec)
    recs[9]['qual'] = None          # l_seq 16, reverse strand, qualities absent
    recs[20]['qual'] = None         # l_seq 255, forward
    recs.insert(5, {'name': b'secondary', 'seq': 'ACGTACGT', 'qual': [30] * 8, 'flag': 0x100})
    recs.insert(30, {'name': b'supplementary', 'seq': 'ACGTACGTA', 'qual': [30] * 9, 'flag': 0x800 | 0x10})
    _corpus = recs
    return recs


def fastq_text(records):
    """The records a FASTQ can hold (a base or more, qualities present) as FASTQ text, by the rules of
    the record layer; and those records."""
    keep = [r for r in kept(records) if len(r['seq']) >= 1 and r.get('qual') is not None]
    e = expected(keep)
    return b''.join(b'@' + n + b'\n' + s + b'\n+\n' + q + b'\n' for n, s, q in zip(e['names'], e['seq'], e['qual'])), keep


def small_records(n, seed=3, lo=20, hi=400):
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        ln = int(rng.randint(lo, hi))
        out.append({'name': b'read_%d' % i, 'seq': ''.join('ACGT'[c] for c in rng.randint(0, 4, ln)),
                    'qual': [int(q) for q in rng.randint(0, 60, ln)], 'flag': 4 | (0x10 if i % 5 == 0 else 0)})
    return out


def fault_cases():
    """[(name, inflated BAM bytes, records delivered before the fault)]: damaged record chains."""
    good = small_records(12, seed=5)
    head = raw_bam(good)
    extra = {'name': b'x', 'seq': 'ACGTACGTAC', 'qual': [20] * 10}
    cases = [('cut-in-record', head + record_bytes(extra)[:-7], good),
             ('block-31', head + record_bytes(extra, block_size=31), good),
             ('block-small', head + record_bytes(extra, block_size=32 + 2 + 5 + 9) + record_bytes(extra), good),
             ('l_read_name-0', head + record_bytes(dict(extra, l_read_name=0)), good),
             ('l_seq-neg', head + record_bytes(dict(extra, l_seq=-1)), good),
             ('l_text-past-end', b'BAM\1' + struct.pack('<i', 1 << 20) + b'@HD\tVN:1.6\n', []),
             ('version-2', raw_bam(good, version=2), [])]
    return cases
