"""Shared inputs of the BAM output tests (test_bam_pack_cpu.py, test_gpu_bam_pack.py): the part corpus
of engine.bam_pack, the two-batch writer cases and the helpers that take a written file apart. TEST
INFRASTRUCTURE ONLY: what a file must hold is restated with tests/bam_lib.py (header_bytes,
record_bytes) and Python's zlib, never with the code under test."""
import struct
import zlib

import numpy as np

from tests import bam_lib as B

L_SEQ = [0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 255, 256, 257, 16383, 16384, 16385, 32769]
NAME_LEN = list(range(1, 18)) + [254]
AUX_LEN = [0, 1, 15, 16, 17, 40000]
BLOCK = 65280
DEFAULT_HEADER = b'@HD\tVN:1.6\tSO:unknown\n'


def letter_map(text):
    """Letters as a BAM record holds them: the 16 codes' letters as they are, U as T, anything else N."""
    return ''.join(c if c in B.LETTERS else ('T' if c == 'U' else 'N') for c in text)


def phred(qual_bytes):
    return [min(93, max(0, c - 33)) for c in qual_bytes]


_corpus = None


def pack_corpus():
    """(seq, qual, side, parts, records): source buffers (uint8), an unplanned engine.BAM_PART table and
    the records it must give. Three passes over L_SEQ: name lengths 1..17 and 254 (record starts hit
    every residue mod 16), gaps of 0..16 bytes in front of every source (misaligned sources), aux lengths
    0, 1, 15, 16, 17 and 40000, the 16 letters plus U, lower case and '.', qualities '!'..'~' with an
    interior space and a byte >= 0x80, and parts without qualities."""
    global _corpus
    if _corpus is not None:
        return _corpus
    from custom_porechop_abi_amd import engine
    rng = np.random.RandomState(23)
    alphabet = np.frombuffer((B.LETTERS + 'Uacgtn.').encode(), np.uint8)
    seq, qual, side, parts, records = [], [], [], [], []
    seq_at = qual_at = side_at = 0
    for i, ln in enumerate(L_SEQ * 3):
        nlen, gap, alen = NAME_LEN[(i * 7 + i // 17) % len(NAME_LEN)], (i * 5) % 17, AUX_LEN[(i + i // 17) % len(AUX_LEN)]
        letters = alphabet[rng.randint(0, alphabet.size, ln)]
        if ln >= alphabet.size:
            letters[:alphabet.size] = alphabet
        q = rng.randint(33, 127, ln).astype(np.uint8)
        if ln >= 94:
            q[:94] = np.arange(33, 127)
        if ln >= 255:
            q[100], q[101], q[102] = 32, 0x80, 0xFF    # an interior space, bytes >= 0x80
        absent = i % 5 == 3
        name = rng.randint(33, 127, nlen).astype(np.uint8)
        aux = rng.randint(0, 256, alen).astype(np.uint8)
        seq += [rng.randint(65, 91, gap).astype(np.uint8), letters]
        seq_at += gap
        if not absent:
            qual += [rng.randint(33, 127, gap).astype(np.uint8), q]
            qual_at += gap
        side += [name, aux]
        parts.append((seq_at, -1 if absent else qual_at, side_at, 0, 0, ln, nlen, alen, 0))
        records.append({'name': name.tobytes(), 'seq': letter_map(letters.tobytes().decode('latin-1')),
                        'qual': None if absent else phred(q.tobytes()), 'aux': aux.tobytes()})
        seq_at += ln
        qual_at += 0 if absent else ln
        side_at += nlen + alen
    cat = lambda parts_: np.concatenate(parts_) if parts_ else np.zeros(0, np.uint8)   # noqa: E731
    _corpus = (cat(seq), cat(qual), cat(side), np.array(parts, engine.BAM_PART), records)
    return _corpus


def planned_with_gaps(parts, out0=5):
    """The table planned from out0, then every record moved back by a few more bytes, so that bytes no
    part owns lie in front of, between and behind the records. Returns (parts, end)."""
    from custom_porechop_abi_amd import engine
    parts = parts.copy()
    end, tiles = engine.bam_pack_plan(parts, out0)
    exp_tiles = sum(max(1, -(-int(ln) // 16384)) for ln in parts['l_seq'])
    assert tiles == exp_tiles
    shift = np.cumsum(np.arange(parts.size) % 3)
    parts['out'] += shift
    return parts, int(end + shift[-1])


def expected_image(parts, records, size):
    img = np.full(size, 0xA5, np.uint8)
    for p, r in zip(parts, records):
        rb = B.record_bytes(r)
        img[int(p['out']):int(p['out']) + len(rb)] = np.frombuffer(rb, np.uint8)
    return img


# ---- files -------------------------------------------------------------------------------------------
def members(data):
    """A BGZF file's members as (whole member bytes, decoded bytes); every member's framing is checked:
    the 18-byte header with BSIZE, raw deflate that zlib inflates, CRC-32 and ISIZE."""
    out, at = [], 0
    while at < len(data):
        h = data[at:at + 18]
        assert h[:4] == b'\x1f\x8b\x08\x04' and h[10:16] == b'\x06\x00BC\x02\x00', (at, h)
        size = struct.unpack('<H', h[16:18])[0] + 1
        m = data[at:at + size]
        assert len(m) == size, 'BSIZE runs past the file'
        d = zlib.decompressobj(-15)
        dec = d.decompress(m[18:-8]) + d.flush()
        assert d.eof and not d.unused_data
        crc, isize = struct.unpack('<II', m[-8:])
        assert crc == zlib.crc32(dec) and isize == len(dec)
        out.append((m, dec))
        at += size
    return out


def parse_fastq(text):
    """[(header, seq, qual)] of four-line FASTQ text (bytes)."""
    lines = text.split(b'\n')
    assert lines[-1] == b'' and (len(lines) - 1) % 4 == 0
    return [(lines[k][1:], lines[k + 1], lines[k + 3]) for k in range(0, len(lines) - 1, 4)]


def records_of_fastq(text, absent_quals=False):
    """The BAM records the FASTQ text of the same write must become."""
    recs = []
    for header, seq, qual in parse_fastq(text):
        name = header.split(b' ')[0].split(b'\t')[0][:254] or b'*'
        recs.append({'name': name, 'seq': letter_map(seq.decode()), 'qual': None if absent_quals else phred(qual)})
    return recs


def reads_of(records):
    """(names, seq, qual) as the project's reader gives the records back."""
    return ([r['name'] for r in records], [r['seq'].encode() for r in records],
            [b'+' * len(r['seq']) if r['qual'] is None else bytes(q + 33 for q in r['qual']) for r in records])


def batch_reads(b):
    cut = lambda buf, off: [buf[off[i]:off[i + 1]].tobytes() for i in range(b.n)]   # noqa: E731
    return cut(b.names, b.name_off), cut(b.seq, b.seq_off), cut(b.qual, b.qual_off)


# ---- the two-batch writer case -----------------------------------------------------------------------
def writer_reads(kind, seed=7):
    """Two batches' worth of reads for input kind 'fastq' | 'fasta' | 'bam': [(header, seq, qual)] x 2.
    The first batch holds ~290k bases (a stream of four members or more in every variant, so records span
    members), the second
    a few reads. Headers carry comments after a space or a tab; some reads are RNA (U) in the text
    kinds; one read is shorter than its trims."""
    rng = np.random.RandomState(seed)
    out = []
    for n_reads, lo, hi in ((64, 2500, 6500), (9, 200, 2500)):
        reads = []
        for i in range(n_reads):
            ln = int(rng.randint(lo, hi)) if i != 5 else 30
            letters = 'ACGU' if (kind != 'bam' and i % 7 == 3) else 'ACGT'
            seq = ''.join(letters[c] for c in rng.randint(0, 4, ln))
            if i % 9 == 1 and kind != 'bam':
                seq = seq[:10] + 'NRYK' + seq[14:]
            qual = bytes(rng.randint(33, 127, ln).astype(np.uint8))
            header = b'r%d_%d' % (len(out), i)
            if kind != 'bam':
                header += [b'', b' comment x=1', b'\ttabbed'][i % 3]
            reads.append((header, seq.encode(), qual))
        out.append(reads)
    return out


def writer_file(kind, reads):
    if kind == 'fastq':
        return b''.join(b'@' + h + b'\n' + s + b'\n+\n' + q + b'\n' for h, s, q in reads)
    if kind == 'fasta':
        return b''.join(b'>' + h + b'\n' + s + b'\n' for h, s, q in reads)
    recs = [{'name': h, 'seq': s.decode(), 'qual': [c - 33 for c in q], 'flag': 4 | (0x10 if i % 4 == 1 else 0),
             'aux': b'RGZgrp\0' if i % 2 else b''} for i, (h, s, q) in enumerate(reads)]
    return B.make_bam(recs, b'@HD\tVN:1.6\tSO:unknown\n@RG\tID:grp\n')


VARIANTS = ['split', 'discard_middle', 'untrimmed', 'select']


def writer_args(variant, n, lengths, seed=1):
    """write_reads keyword arguments for a batch of n reads: start and end trims, middle cuts on every
    third read (one cut leaves a piece under min_split_read_size), and the variant's switch."""
    rng = np.random.RandomState(seed)
    st = rng.randint(0, 40, n).astype(np.int32)
    et = rng.randint(0, 40, n).astype(np.int32)
    st[::4] = 0
    et[::6] = 0
    cuts = []
    for i in range(n):
        tl = max(0, int(lengths[i]) - int(st[i]) - int(et[i]))
        if i % 3 == 2 and tl > 900:
            cuts.append([(tl // 3, tl // 3 + 50), (tl // 3 + 120, tl // 3 + 160), (2 * tl // 3, 2 * tl // 3 + 10)])
        else:
            cuts.append(None)
    kw = dict(start_trim=st, end_trim=et, middle_cuts=cuts, min_split_read_size=100)
    if variant == 'discard_middle':
        kw['discard_middle'] = True
    elif variant == 'untrimmed':
        kw['untrimmed'] = True
    elif variant == 'select':
        kw['select'] = (np.arange(n) % 3 != 1).astype(np.uint8)
    return kw


def write_two_batches(tmp_path, kind, variant, gzip_device, tag):
    """Writes the case's two batches as BAM (append, then bgzf_finish) and as FASTQ text through the
    existing writer with the same arguments. Returns (bam path, header text, FASTQ text, n emitted
    (bam), n emitted (fastq))."""
    import os
    from custom_porechop_abi_amd import misc
    ext = {'fastq': 'fastq', 'fasta': 'fasta', 'bam': 'bam'}[kind]
    bam_path, fq_path = str(tmp_path / ('out_%s.bam' % tag)), str(tmp_path / ('out_%s.fastq' % tag))
    header = None
    n_bam = n_fq = 0
    for k, reads in enumerate(writer_reads(kind)):
        src = str(tmp_path / ('in_%s_%d.%s' % (tag, k, ext)))
        with open(src, 'wb') as f:
            f.write(writer_file(kind, reads))
        b = misc.load_batch(src)
        assert b.n == len(reads)
        if k == 0:
            header = b.bam_header
            assert (header is not None) == (kind == 'bam')
        kw = writer_args(variant, b.n, b.lengths, seed=k + 1)
        n_bam += misc.write_reads(b, bam_path, 'bam', append=k > 0, gzip_device=gzip_device, bam_header=header, **kw)
        n_fq += misc.write_reads(b, fq_path, 'fastq', append=k > 0, **kw)
    misc.bgzf_finish(bam_path)
    with open(fq_path, 'rb') as f:
        text = f.read() if os.path.getsize(fq_path) else b''
    return bam_path, header, text, n_bam, n_fq
