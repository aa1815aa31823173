"""SAM tags in FASTQ / FASTA headers (include/pcabi.h "SAM tags in FASTQ / FASTA headers"), host build
(device = -1): the aux chains' text and the text records against tests/header_tags_ref.py, then BAM in
with tags -> text out against what out_format 'bam' writes for the same options. tests/test_gpu_header_tags.py
runs the same checkers on the device."""
import gzip
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import header_tags_ref as H
from tests import test_moves_cpu as V

HERE = os.path.dirname(os.path.abspath(__file__))

ARRAY_LENGTHS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 4097]
EDGES = {'C': [0, 9, 10, 99, 100, 255], 'c': [-128, -100, -99, -10, -9, -1, 127, 0],
         's': [-32768, 32767, -10000, -9999, 9999, 10000, -1], 'S': [32768, 65535, 0, 999, 1000],
         'i': [-2 ** 31, 2 ** 31 - 1, -999999999, -1000000000, 99999, 100000, 0],
         'I': [2 ** 31, 4294967295, 999999999, 1000000000, 0],
         'f': [0.0, -0.5, 1e-7, 12345678.0, float('inf'), -float('inf'), 3.4028234e38, 1.17549435e-38, 100000.0, 1e6]}
SEQ_LENGTHS = [1, 69, 70, 71, 140, 16383, 16384, 16385, 40000]


def scalar(name, typ, v):
    return name + typ.encode() + struct.pack(H.FMT[typ], v)


def array(name, sub, vals):
    return name + b'B' + sub.encode() + struct.pack('<I', len(vals)) + b''.join(struct.pack(H.FMT[sub], v) for v in vals)


def array_values(sub, n, seed=0):
    """n values of subtype sub that run through every digit width, the edges first."""
    e = EDGES[sub]
    rng = np.random.RandomState(seed + n)
    lo, hi = {'c': (-128, 127), 'C': (0, 255), 's': (-32768, 32767), 'S': (0, 65535), 'i': (-2 ** 31, 2 ** 31 - 1),
              'I': (0, 2 ** 32 - 1), 'f': (0, 0)}[sub]
    out = []
    for k in range(n):
        if k < len(e):
            out.append(e[k])
        elif sub == 'f':
            out.append(float(np.float32(rng.standard_normal() * 10.0 ** rng.randint(-8, 9))))
        else:
            w = 10 ** rng.randint(1, 11)   # a magnitude first, so that short values are as common as long ones
            out.append(int(max(lo, min(hi, rng.randint(-w, w) if lo < 0 else rng.randint(0, w)))))
    return out


def chain_corpus():
    """Aux chains that meet every type, subtype, digit width, array length, string kind and guard."""
    chains = [b'']
    for typ, vals in EDGES.items():
        chains += [scalar(b'X' + typ.encode(), typ, v) for v in vals]
        chains.append(b''.join(scalar(b'Y%d' % (k % 10), typ, v) for k, v in enumerate(vals)))
        chains.append(array(b'ar', typ, vals))
        for n in ARRAY_LENGTHS:
            chains.append(array(b'a' + typ.encode(), typ, array_values(typ, n)))
    for n in ARRAY_LENGTHS:   # move tables: one digit an element
        chains.append(b'mvBc' + struct.pack('<I', n + 1) + b'\x05' + bytes(np.random.RandomState(n).randint(0, 2, n).tolist()))
    strings = [b'XZZ\0', b'XYZa b:c : d\0', b'hxH1AE301\0', b'XAA!', b'XAA~', b'XAA ', b'MMZC+m,1,2;\0',
               b'lgZ' + bytes(range(0x20, 0x7F)) * 3 + b'\0', b'l2Z' + b'x' * 63 + b'\0', b'l3Z' + b'x' * 64 + b'\0',
               b'l4Z' + b'x' * 65 + b'\0']
    chains += strings
    chains.append(b''.join(strings))
    left_out = [b'1XZabc\0', b'X_Zabc\0', b'XAA\x7f', b'XAA\x1f', b'XZZa\tb\0', b'XZZa\nb\0', b'XZZ\xc3\xa9\0', b'XHH\x01\0',
                b'l5Z' + b'x' * 64 + b'\x01' + b'y' * 70 + b'\0', b'_1i' + struct.pack('<i', 5), b'9aBc' + struct.pack('<I', 2) + b'\1\2']
    chains += left_out
    chains.append(b''.join(left_out))                                   # a chain of only left-out tags
    chains.append(strings[1] + left_out[0] + scalar(b'ns', 'i', -77) + left_out[4] + array(b'ML', 'C', [0, 255, 7]))
    # chains that do not walk
    chains += [b'XZZabc', b'XY', b'XQ\0\0\0', b'XBBq' + struct.pack('<I', 0), b'XBBc' + struct.pack('<I', 5) + b'\1\2',
               b'XBBc\1\0', b'XIi\0\0', scalar(b'ok', 'C', 7) + b'XZZabc', b'XBBi' + struct.pack('<I', 0xFFFFFFFF) + b'\0' * 16,
               b'XAA', b'okZfine\0XHH12']
    return chains


def run_table(chains, device, aux_align=lambda j: (5 * j) % 16, out_align=lambda j: (3 * j + 1) % 16):
    """The chains laid into a blob (chain j at alignment aux_align(j)), planned, written with gaps between
    the outputs (part j at alignment out_align(j)). -> (texts, lens, counters, the gaps kept their bytes)."""
    from custom_porechop_abi_amd import engine
    parts = np.zeros(len(chains), engine.AUXTEXT_PART)
    blob = bytearray()
    for j, c in enumerate(chains):
        while len(blob) % 16 != aux_align(j):
            blob.append(0xCC)
        parts[j]['aux_off'], parts[j]['aux_len'] = len(blob), len(c)
        blob += c
    blob += b'\xCC' * 3
    engine.auxtext_counts(reset=True)
    engine.auxtext_plan(bytes(blob), parts, device)
    counters = engine.auxtext_counts(reset=True)
    cursor = 7
    for j in range(len(chains)):
        if parts[j]['len'] > 0:
            while cursor % 16 != out_align(j):
                cursor += 1
            parts[j]['out'] = cursor
            cursor += int(parts[j]['len']) + 1
    out = np.full(cursor + 9, 0xEE, np.uint8)
    engine.auxtext_write(bytes(blob), parts, out, device)
    assert engine.auxtext_counts(reset=True) == (0, 0)     # the plan counts, not the write
    owned = np.zeros(out.size, bool)
    texts = []
    for p in parts:
        a, n = int(p['out']), int(p['len'])
        if n > 0:
            owned[a:a + n] = True
        texts.append(None if n < 0 else out[a:a + n].tobytes() if n > 0 else b'')
    return texts, parts['len'].tolist(), counters, bool((out[~owned] == 0xEE).all())


def check_table(chains, device, **kw):
    texts, lens, counters, gaps_kept = run_table(chains, device, **kw)
    want_w = want_l = 0
    for j, c in enumerate(chains):
        want = H.sam_text(c)
        assert texts[j] == want, (j, c[:60], texts[j] if texts[j] is None else texts[j][:120], want if want is None else want[:120])
        assert lens[j] == (-1 if want is None else len(want))
        w, l = H.counts(c)
        want_w, want_l = want_w + w, want_l + l
    assert counters == (want_w, want_l)
    assert gaps_kept
    return counters


def check_alignments(device):
    """One array tag, and one string, at each of the 16 alignments of the blob crossed with each of the 16
    alignments of the text's destination."""
    for chain in (array(b'mv', 'c', [5] + [k % 2 for k in range(130)]), array(b'ML', 'C', array_values('C', 67)),
                  array(b'xs', 's', array_values('s', 40)), b'MMZ' + b'C+m,10,2,3;' * 9 + b'\0'):
        check_table([chain] * 256, device, aux_align=lambda j: j % 16, out_align=lambda j: j // 16)


def check_refusals(device):
    from custom_porechop_abi_amd import engine
    from custom_porechop_abi_amd._lib import PcabiError
    blob = scalar(b'ns', 'i', 12345) + b'XZZab\0'
    parts = np.zeros(2, engine.AUXTEXT_PART)
    parts['aux_off'], parts['aux_len'] = [0, 7], [7, 6]
    engine.auxtext_plan(blob, parts, device)
    assert parts['len'].tolist() == [len(b'\tns:i:12345'), len(b'\tXZ:Z:ab')]
    parts['out'] = [0, 20]
    out = np.zeros(40, np.uint8)
    engine.auxtext_write(blob, parts, out, device)
    for change in ({'len': [5, 8]}, {'out': [0, 5]}, {'out': [0, 33]}, {'out': [-1, 20]}, {'aux_off': [0, 8]}, {'aux_len': [7, 7]}):
        bad = parts.copy()
        for k, v in change.items():
            bad[k] = v
        with pytest.raises(PcabiError):
            engine.auxtext_write(blob, bad, out.copy(), device)
    bad = parts.copy()
    bad['aux_len'] = [7, 7]
    with pytest.raises(PcabiError):
        engine.auxtext_plan(blob, bad, device)


def fastx_cases():
    rng = np.random.RandomState(12)
    chains = [c for c in chain_corpus() if len(c) < 400]
    cases = []
    for k, n in enumerate(SEQ_LENGTHS + [5, 141, 70 * 234, 16384 * 2]):
        seq = bytes(rng.choice(list(b'ACGTN'), n).tolist())
        qual = bytes(rng.randint(33, 127, n).tolist())
        name = [b'r%d' % k, b'read_%d runid=abc ch=%d' % (k, k), b'x' * 300, b'a\tb'][k % 4]
        aux = [chains[(7 * k + 3) % len(chains)], b'', array(b'mv', 'c', [5] + [j % 2 for j in range(2 * n)]) + scalar(b'ts', 'i', 10 + k),
               b'XZZabc'][k % 4]
        cases.append({'name': name, 'aux': aux, 'seq': seq, 'qual': qual, 'rna': k % 5 == 2})
    cases.append({'name': b'f', 'aux': array(b'fl', 'f', EDGES['f']) + scalar(b'fx', 'f', -0.5), 'seq': b'ACGT', 'qual': b'!!!!', 'rna': True})
    return cases


def check_fastx(fasta, device, skew=0):
    """The cases laid out with gaps between the records, against the restatement's records."""
    from custom_porechop_abi_amd import engine
    cases = fastx_cases()
    parts = np.zeros(len(cases), engine.FASTX_PART)
    ap = np.zeros(len(cases), engine.AUXTEXT_PART)
    seq, qual, side = bytearray(b'..'), bytearray(b'.'), bytearray(b'...')
    for k, c in enumerate(cases):
        p = parts[k]
        p['seq_src'], p['l_seq'] = len(seq), len(c['seq'])
        seq += c['seq'] + b'.' * (k % 3)
        p['qual_src'], p['l_qual'] = len(qual), 0 if fasta else len(c['qual'])
        qual += c['qual'] + b'.' * (k % 5)
        p['aux_off'], p['aux_len'] = len(side), len(c['aux'])
        side += c['aux'] + b'.' * (k % 4)
        p['name_off'], p['name_len'] = len(side), len(c['name'])
        side += c['name']
        p['flags'] = engine.FASTX_RNA if c['rna'] else 0
        ap[k]['aux_off'], ap[k]['aux_len'] = p['aux_off'], p['aux_len']
    engine.auxtext_plan(bytes(side), ap, device)
    parts['text_len'] = ap['len']
    end, tiles = engine.fastx_pack_plan(parts, fasta, 0)
    want = [H.record(fasta, c['name'], c['aux'], c['seq'], c['qual'], c['rna']) for c in cases]
    assert end == sum(len(w) for w in want)
    assert tiles == sum(max(1, -(-len(c['seq']) // 16384)) for c in cases)
    parts['out'] += 5 + 3 * np.arange(len(cases))         # gaps between the records
    buf = np.full(skew + end + 5 + 3 * len(cases) + 11, 0xEE, np.uint8)
    out = buf[skew:]
    engine.fastx_pack(bytes(seq), bytes(qual), bytes(side), parts, out, fasta, device)
    owned = np.zeros(out.size, bool)
    for k, w in enumerate(want):
        a = int(parts[k]['out'])
        got = out[a:a + len(w)].tobytes()
        assert got == w, (k, fasta, cases[k]['name'][:20], len(w), next(i for i in range(len(w)) if got[i] != w[i]))
        owned[a:a + len(w)] = True
    assert (out[~owned] == 0xEE).all() and (buf[:skew] == 0xEE).all()
    # refusals: a text length that is not the plan's, an unplanned table, a record outside the output
    from custom_porechop_abi_amd._lib import PcabiError
    for field, k, v in (('text_len', 2, int(parts[2]['text_len']) + 1), ('tile0', 3, 0), ('out', len(cases) - 1, out.size - 3),
                        ('seq_src', 0, len(seq)), ('out', 1, int(parts[0]['out']) + 1)):
        bad = parts.copy()
        bad[k][field] = v
        with pytest.raises(PcabiError):
            engine.fastx_pack(bytes(seq), bytes(qual), bytes(side), bad, out.copy(), fasta, device)


# ---- 1. table level ------------------------------------------------------------------------------------
def test_worked_example():
    from custom_porechop_abi_amd import engine
    aux = (b'RGZgrp\0' + scalar(b'ns', 'i', 99999) + scalar(b'qs', 'C', 12) + scalar(b'de', 'f', 0.0125) +
           b'mvBc' + struct.pack('<I', 4) + b'\x05\x01\x00\x01' + array(b'ML', 'C', []) + b'stA+')
    want = b'\tRG:Z:grp\tns:i:99999\tqs:i:12\tde:f:0.0125\tmv:B:c,5,1,0,1\tML:B:C\tst:A:+'
    assert H.sam_text(aux) == want
    assert engine.aux_text([aux, b'', b'XZZabc']) == [want, b'', None]
    assert H.parse_header(b'read 1 ch=5' + want)[0] == b'read 1 ch=5'
    assert H.parse_header(b'read' + want)[1] == H.expected_fields(aux)


def test_corpus_against_restatement():
    counters = check_table(chain_corpus(), -1)
    # (equal to the restatement's counts, checked above; here: that the corpus is not empty of either kind --
    # seven types with 13 array lengths each are written, the eleven left-out tags twice)
    assert counters[0] > 7 * 13 and counters[1] >= 22


def test_alignments():
    check_alignments(-1)


def test_refusals():
    check_refusals(-1)


@pytest.mark.parametrize('fasta', [False, True])
def test_fastx_pack(fasta):
    check_fastx(fasta, -1)
    check_fastx(fasta, -1, skew=9)


# ---- 2. file level: BAM in with tags, text out -----------------------------------------------------------
def file_case(tmp_path, n=60):
    """A BAM with MM ML MN mv ts and other tags (tests/test_moves_cpu.py's writer corpus, reverse-strand
    records and unusable tags included), loaded with keep_aux, and trims and cuts derived from its parts."""
    from custom_porechop_abi_amd import misc
    reads = V.writer_reads(n, with_mods=True)
    V.write_case(tmp_path, reads, None, False, 'unused.bam')     # leaves in.bam
    batch = misc.load_batch(str(tmp_path / 'in.bam'), keep_aux=True)
    st = [r['parts'][0][0] for r in reads]
    et = [r['l_seq'] - (r['parts'][-1][0] + r['parts'][-1][1]) for r in reads]
    cuts = [[(p[0] + p[1] - r['parts'][0][0], q[0] - r['parts'][0][0]) for p, q in zip(r['parts'], r['parts'][1:])] for r in reads]
    return batch, {'start_trim': st, 'end_trim': et, 'middle_cuts': cuts, 'min_split_read_size': 1}


def variants(n):
    sel = (np.arange(n) % 3 != 1).astype(np.uint8)
    return [('cuts', {}), ('discard', {'discard_middle': True}), ('select', {'select': sel}), ('untrimmed', {'untrimmed': True}),
            ('minsplit', {'min_split_read_size': 12})]


TAG_OPTIONS = [{}, {'keep_mods': True}, {'keep_moves': True}, {'keep_mods': True, 'keep_moves': True}]


def read_text(path, fmt):
    with open(path, 'rb') as f:
        data = f.read()
    return gzip.decompress(data) if fmt.endswith('.gz') else data


def counters_reset():
    from custom_porechop_abi_amd import engine
    return engine.mods_counts(reset=True), engine.moves_counts(reset=True)


def check_file(tmp_path, batch, fmt, kw, tags, gzip_device=None, bgzf=False, twice=False, host_text=None):
    """Assertions 2, 3 and 5 of one written file (4 when host_text is given). -> its text."""
    from custom_porechop_abi_amd import misc
    fasta = fmt.startswith('fasta')
    paths = {k: str(tmp_path / (k + '.' + (fmt if k != 'bam' else 'bam'))) for k in ('tags', 'today', 'bam')}
    dev = {'gzip_device': gzip_device, 'bgzf': bgzf} if gzip_device is not None else {}
    counts = {}
    for k in ('tags', 'today', 'bam'):
        for f in (paths[k],):
            if os.path.exists(f):
                os.remove(f)
        counters_reset()
        for rep in range(2 if twice else 1):
            if k == 'tags':
                n = misc.write_reads(batch, paths[k], fmt, append=rep > 0, keep_aux=True, header_tags=True, **kw, **tags, **dev)
            elif k == 'today':
                n = misc.write_reads(batch, paths[k], fmt, append=rep > 0, **kw, **dev)
            else:
                n = misc.write_reads(batch, paths[k], 'bam', append=rep > 0, keep_aux=True, **kw, **tags)
            counts.setdefault(k, []).append(n)
        counts[k].append(counters_reset())
        if k == 'bam' or bgzf:
            misc.bgzf_finish(paths[k])
    assert counts['tags'] == counts['bam'], (counts['tags'], counts['bam'])          # 5: return values and counters
    assert counts['tags'][:-1] == counts['today'][:-1]
    text, today = read_text(paths['tags'], fmt), read_text(paths['today'], fmt)
    got, old = H.split_records(text, fasta), H.split_records(today, fasta)
    back = misc.load_batch(paths['bam'], keep_aux=True)
    assert len(got) == len(old) == back.n and back.n > 0
    with_tags = 0
    for k, ((head, seq, qual), (head0, seq0, qual0)) in enumerate(zip(got, old)):
        name, fields = H.parse_header(head)
        assert (name, seq, qual) == (head0, seq0, qual0)                              # 2: cut at the first tab
        assert head.split(b'\t')[0] == head0
        assert fields == H.expected_fields(back.aux(k)), (k, head[:200], back.aux(k)[:100])   # 3: the BAM record's tags
        assert head == head0 + (H.sam_text(back.aux(k)) or b'')
        with_tags += bool(fields)
    assert with_tags > len(got) // 2
    if host_text is not None:
        assert text == host_text                                                     # 4
    return text


@pytest.mark.parametrize('fmt', ['fastq', 'fasta', 'fastq.gz'])
def test_bam_in_text_out(tmp_path, fmt):
    batch, base = file_case(tmp_path)
    seen = set()
    for vname, extra in variants(batch.n):
        for tags in TAG_OPTIONS:
            text = check_file(tmp_path, batch, fmt, dict(base, **extra), tags)
            seen.add((vname, tuple(sorted(tags)), b'\tmv:B:c,' in text, b'\tMM:Z:' in text))
    # the remapped tags are there when asked for; a changed read carries none of them otherwise
    assert ('cuts', ('keep_mods', 'keep_moves'), True, True) in seen
    check_file(tmp_path, batch, fmt, base, TAG_OPTIONS[3], twice=True)                # two appended batches


def test_option_off_and_fastq_batches_write_todays_bytes(tmp_path):
    """Assertion 1: with header_tags off, or on a batch without aux bytes, the file is today's."""
    from custom_porechop_abi_amd import misc
    batch, base = file_case(tmp_path, 30)
    for fmt in ('fastq', 'fasta', 'fastq.gz'):
        a, b, c, d = (str(tmp_path / ('%s.%s' % (k, fmt))) for k in 'abcd')
        misc.write_reads(batch, a, fmt, **base)
        misc.write_reads(batch, b, fmt, header_tags=False, **base)
        with open(a, 'rb') as f, open(b, 'rb') as g:
            assert f.read() == g.read()
        if fmt == 'fastq':
            plain = misc.load_batch(a)                 # read from FASTQ: no aux bytes
            assert plain.n > 0
            misc.write_reads(plain, c, fmt, start_trim=[1] * plain.n)
            misc.write_reads(plain, d, fmt, start_trim=[1] * plain.n, keep_aux=True, header_tags=True, keep_mods=True, keep_moves=True)
            with open(c, 'rb') as f, open(d, 'rb') as g:
                assert f.read() == g.read()
    # a batch read from BAM without keep_aux holds no aux bytes either
    bare = misc.load_batch(str(tmp_path / 'in.bam'))
    misc.write_reads(bare, str(tmp_path / 'e.fastq'), 'fastq', **base)
    misc.write_reads(bare, str(tmp_path / 'f.fastq'), 'fastq', keep_aux=True, header_tags=True, **base)
    with open(str(tmp_path / 'e.fastq'), 'rb') as f, open(str(tmp_path / 'f.fastq'), 'rb') as g:
        assert f.read() == g.read()


def test_header_comments_stay_in_front_of_the_tags(tmp_path):
    """The name part is the whole header as the text writers write it (comments included, `_k` in front of
    the first blank for a split piece); the tags follow it."""
    from custom_porechop_abi_amd import misc
    from tests import bam_lib as B
    seq = 'ACGT' * 30
    aux = b'RGZgrp\0' + scalar(b'de', 'f', 0.25) + V.mv_aux(5, [1] * 120) + V.ts_aux(10)
    src = str(tmp_path / 'c.bam')
    with open(src, 'wb') as f:
        f.write(B.make_bam([{'name': b'read1', 'seq': seq, 'qual': [30] * 120, 'flag': 4, 'aux': aux}], b'@HD\tVN:1.6\n', (), 5000))
    batch = misc.load_batch(src, keep_aux=True)
    out = str(tmp_path / 'c.fastq')
    misc.write_reads(batch, out, 'fastq', start_trim=[4], middle_cuts=[[(40, 50)]], min_split_read_size=1, keep_aux=True,
                     keep_moves=True, header_tags=True)
    recs = H.split_records(read_text(out, 'fastq'), False)
    assert [r[0] for r in recs] == [b'read1_1\tRG:Z:grp\tde:f:0.25\tmv:B:c,5' + b',1' * 40 + b'\tts:i:30',
                                    b'read1_2\tRG:Z:grp\tde:f:0.25\tmv:B:c,5' + b',1' * 66 + b'\tts:i:280']


# ---- 3. the Python surface ---------------------------------------------------------------------------------
def test_value_errors(tmp_path):
    from custom_porechop_abi_amd import misc
    from custom_porechop_abi_amd.pipeline import FileTrimmer
    batch, base = file_case(tmp_path, 5)
    x = str(tmp_path / 'x')
    with pytest.raises(ValueError):
        misc.write_reads(batch, x + '.bam', 'bam', keep_aux=True, header_tags=True)
    with pytest.raises(ValueError):
        misc.write_reads(batch, x + '.fastq', 'fastq', header_tags=True)
    # the two old ones: the tag options on a text format without header_tags
    with pytest.raises(ValueError):
        misc.write_reads(batch, x + '.fastq', 'fastq', keep_aux=True, keep_mods=True)
    with pytest.raises(ValueError):
        misc.write_reads(batch, x + '.fastq', 'fastq', keep_aux=True, keep_moves=True)
    with pytest.raises(ValueError):
        misc.write_reads(batch, x + '.fastq', 'fastq', keep_mods=True, header_tags=True)
    with pytest.raises(ValueError):
        FileTrimmer([], header_tags=True)


# ---- 4. the shared header alone, under sanitizers -------------------------------------------------------------
def test_auxtext_layer_under_sanitizers(tmp_path):
    """tests/auxtext_fuzz_main.cpp (csrc/pcabi_auxtext.h alone), built with -fsanitize=address,undefined as
    a program of its own and run as a child process: random and truncated chains in blocks of exactly
    their size, the 64 lanes of the string scan and the array passes played in turn against the byte-wise
    walk and a formatter of its own, and the text records' tiles against whole records."""
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path / 'auxtext_fuzz')
    base = ['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
            os.path.join(HERE, 'auxtext_fuzz_main.cpp')]
    for extra in (['-static-libasan', '-static-libubsan'], []):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        if r.returncode == 0:
            break
    if r.returncode != 0 and ('asan' in r.stderr or 'ubsan' in r.stderr or 'sanitize' in r.stderr):
        pytest.skip('the sanitizer runtime cannot be linked')
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, '1', '3000'], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'rounds 3000' in r.stdout
