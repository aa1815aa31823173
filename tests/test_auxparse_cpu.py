"""SAM tags read from FASTQ / FASTA headers (include/pcabi.h "SAM tags read from FASTQ / FASTA headers"), host
build (device = -1): literal vectors written by hand from SAMv1 section 4.2.4, a corpus against
tests/auxparse_ref.py, the round trip through the existing formatter (engine.aux_text), the refusals, and
files: the same reads as BAM with aux and as FASTQ / FASTA with that aux in the headers must write the same
outputs. tests/test_gpu_auxparse.py runs the same checkers on the device."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import auxparse_ref as R
from tests import bam_lib as B
from tests import header_tags_ref as H
from tests import mods_ref
from tests import test_header_tags_cpu as HT
from tests import test_moves_cpu as V

HERE = os.path.dirname(os.path.abspath(__file__))

# ---- 1. literal vectors ------------------------------------------------------------------------------------
# (header field, the aux bytes it gives, or None when it is left out)
LITERALS = [
    (b'NM:i:5', b'NMC\x05'),
    (b'XN:i:-1', b'XNc\xff'),
    (b'XS:i:300', b'XSS\x2c\x01'),
    (b'XI:i:4294967295', b'XII\xff\xff\xff\xff'),
    (b'Xi:i:-2147483648', b'Xii\x00\x00\x00\x80'),
    (b'XI:i:4294967296', None),
    (b'Xi:i:-2147483649', None),
    (b'XI:i:99999999999', None),
    (b'RG:Z:a b', b'RGZa b\0'),
    (b'XZ:Z:', b'XZZ\0'),
    (b'XH:H:1ae3', b'XHH1ae3\0'),
    (b'XH:H:1AE', None),
    (b'ML:B:C,0,255,7', b'MLBC\x03\0\0\0\x00\xff\x07'),
    (b'ML:B:C,0,256', None),
    (b'mv:B:c,6,1,0', b'mvBc\x03\0\0\0\x06\x01\x00'),
    (b'XB:B:s', b'XBBs\0\0\0\0'),
    (b'de:f:0.25', b'def\x00\x00\x80\x3e'),
    (b'XF:B:f,1,-0.5', b'XFBf\x02\0\0\0\x00\x00\x80\x3f\x00\x00\x00\xbf'),
    # more of the integer typing
    (b'XC:i:255', b'XCC\xff'), (b'XS:i:256', b'XSS\x00\x01'), (b'XS:i:65535', b'XSS\xff\xff'), (b'XI:i:65536', b'XII\x00\x00\x01\x00'),
    (b'Xc:i:-128', b'Xcc\x80'), (b'Xs:i:-129', b'Xss\x7f\xff'), (b'Xs:i:-32768', b'Xss\x00\x80'), (b'Xi:i:-32769', b'Xii\xff\x7f\xff\xff'),
    (b'X0:i:-0', b'X0c\x00'), (b'XP:i:+7', b'XPC\x07'), (b'XL:i:0000000300', b'XLS\x2c\x01'), (b'XL:i:00000000300', None),
    (b'XE:i:', None), (b'XE:i:-', None), (b'XE:i:1 ', None), (b'XE:i:0x10', None),
    (b'st:A:+', b'stA+'), (b'st:A: ', b'stA '), (b'st:A:', None), (b'st:A:ab', None), (b'st:A:\x7f', None),
    (b'XH:H:', b'XHH\0'), (b'XH:H:1g', None),
    (b'ef:f:1e-3', b'eff' + struct.pack('<f', 1e-3)), (b'ef:f:-.5E+1', b'eff' + struct.pack('<f', -5.0)), (b'ef:f:inf', b'eff\x00\x00\x80\x7f'),
    (b'ef:f:-inf', b'eff\x00\x00\x80\xff'), (b'ef:f:1e39', b'eff\x00\x00\x80\x7f'), (b'ef:f:5.', None), (b'ef:f:1e', None),
    (b'ef:f:0x1p3', None), (b'ef:f:Inf', None), (b'ef:f:' + b'1' * 32, None), (b'ef:f:' + b'1' * 31, b'eff' + struct.pack('<f', float('1' * 31))),
    (b'ab:B:c,-128,127', b'abBc\x02\0\0\0\x80\x7f'), (b'ab:B:c,-129', None), (b'ab:B:S,65535', b'abBS\x01\0\0\0\xff\xff'),
    (b'ab:B:S,-0', b'abBS\x01\0\0\0\x00\x00'), (b'ab:B:S,-1', None), (b'ab:B:I,4294967295', b'abBI\x01\0\0\0\xff\xff\xff\xff'),
    (b'ab:B:i,2147483648', None), (b'ab:B:c,', None), (b'ab:B:c,1,', None), (b'ab:B:c,,1', None), (b'ab:B:c1', None), (b'ab:B:', None),
    (b'ab:B:q,1', None), (b'ab:B:f,1,x', None),
    # the left-out kinds
    (b'X:Z:a', None), (b'1X:Z:a', None), (b'X_:Z:a', None), (b'XQ:Q:a', None), (b'XZ:z:a', None), (b'XZZa', None), (b'XZ;Z:a', None),
    (b'XZ:Z:a\x7fb', None), (b'XZ:Z:\xc3\xa9', None), (b'', None), (b'XZ:Z', None), (b'XZ:Z:a\x00', None),
]


def test_literal_vectors():
    from custom_porechop_abi_amd import engine
    engine.auxparse_counts(reset=True)
    got = engine.aux_parse([b'read 1 comment\t' + f for f, _ in LITERALS])
    kept = sum(w is not None for _, w in LITERALS)
    assert engine.auxparse_counts(reset=True) == (kept, len(LITERALS) - kept)
    for (f, want), g in zip(LITERALS, got):
        assert g == (want or b''), (f, g, want)
    # all of them in one header: the kept ones in header order; a trailing tab is one more field left out
    every = b'name\t' + b'\t'.join(f for f, _ in LITERALS) + b'\t'
    assert engine.aux_parse(every) == b''.join(w for _, w in LITERALS if w is not None)
    assert engine.auxparse_counts(reset=True) == (kept, len(LITERALS) - kept + 1)
    # the restatement agrees with the hand-written bytes
    for f, want in LITERALS:
        assert R.field(f) == want, f


# ---- 2. the corpus against the restatement -----------------------------------------------------------------
ARRAY_LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 4097]
Z_LENGTHS = [0, 63, 64, 65, 200]
USUAL = [b'qs:f:17.3421', b'du:f:1.2345', b'ns:i:12345', b'ts:i:10', b'mx:i:1', b'ch:i:1201', b'st:Z:2024-05-01T12:34:56.789+00:00',
         b'rn:i:40312', b'fn:Z:PAK12345_pass_0a1b2c3d_00000017.pod5', b'sm:f:85.1234', b'sd:f:12.8791', b'sv:Z:quantile', b'dx:i:0',
         b'RG:Z:0a1b2c3d4e5f_dna_r10.4.1_e8.2_400bps_sup@v4.3.0', b'pi:Z:8a1b2c3d-0000-4000-8000-1234567890ab', b'sp:i:0',
         b'mv:B:c,6,1,0,1,1,0,0,1,0,1', b'MM:Z:C+m?,3,0,12;C+h?,3,0,12;', b'ML:B:C,0,255,7,12,200,3', b'MN:i:180']


def elem_text(sub, v):
    return (b'%g' % float(np.float32(v))) if sub == 'f' else b'%d' % v


def header_corpus():
    """Headers that meet every type and subtype, every array length around the pass, element widths that put
    the pass boundary at every position of an element, the string lengths around the pass, bad elements
    in late passes, and the literal vectors."""
    rng = np.random.RandomState(5)
    hs = [b'', b'no_tab_at_all comment', b'\tXZ:Z:starts with a tab', b'n\t', b'n\t\t', b'\t', b'n\t\tNM:i:5\t\tXN:i:-1\t']
    hs += [b'read 1 comment\t' + f for f, _ in LITERALS]
    for sub in 'cCsSiIf':                                   # every array length, for every subtype
        for n in ARRAY_LENGTHS:
            hs.append(b'r\ta%c:B:%c' % (ord(sub), ord(sub)) + b''.join(b',' + elem_text(sub, v) for v in HT.array_values(sub, n)))
    for pad in range(70):                                   # one-digit elements: the boundary at every position
        n = 60 + pad
        hs.append(b'n' * pad + b'\tmv:B:c,5' + b''.join(b',%d' % b for b in rng.randint(0, 2, n).tolist()) + b'\tts:i:%d' % pad)
    edge = [b'-2147483648', b'2147483647', b'-1000000000', b'7']
    for pad in range(26):                                   # B:i at the 11-character edges
        hs.append(b'n' * pad + b'\tXi:B:i' + b''.join(b',' + edge[(k * (1 + pad % 3)) % 4] for k in range(40)) + b'\tXI:B:I,4294967295,0')
    for k in range(40):                                     # mixed widths
        sub = 'cCsSiIf'[k % 7]
        vals = HT.array_values(sub, 40 + 5 * k, seed=k)
        hs.append(b'mix%d\t' % k + b'x%d:B:%c' % (k % 10, ord(sub)) + b''.join(b',' + elem_text(sub, v) for v in vals) + b'\tok:A:!')
    for n in Z_LENGTHS:                                     # strings around the pass; the tab on byte 63, 64, 65
        for typ, fill in ((b'Z', b'a b:c,d;'), (b'H', b'0aF9')):
            hs.append(b'r\tXZ:%s:' % typ + (fill * 60)[:n] + b'\tNM:i:%d' % n)
            hs.append(b'r\tXZ:%s:' % typ + (fill * 60)[:n])
    for pad in range(60, 70):
        hs.append(b'n' * pad + b'\tNM:i:5\tXF:f:0.5')        # the first tab around the pass boundary
        hs.append(b'r\tNM:i:' + b'1' * pad + b'\tok:i:5')    # a scalar that runs over the pass
    # a bad element in a pass other than the first, good fields behind it; a bad byte late in a string
    for at in (3, 40, 70, 130, 199):
        for sub, bad in (('c', b'128'), ('C', b'-1'), ('s', b'x'), ('i', b'2147483648'), ('f', b'1e'), ('S', b''), ('I', b'12345678901')):
            el = [b'1'] * 200
            el[at] = bad
            hs.append(b'r\tgd:i:1\tbd:B:%c,' % ord(sub) + b','.join(el) + b'\tg2:Z:after\tg3:B:c,1,2,3')
        hs.append(b'r\tbz:Z:' + b'z' * at + b'\x7f' + b'z' * 10 + b'\tg2:Z:after')
    hs.append(b'r\tlg:B:c,' + b'1' * 70 + b'\tg2:i:1')        # an element longer than a pass
    hs.append(b'r\tlg:B:f,' + b'1' * 40 + b',1\tg2:i:1')
    hs.append(b'read1 runid=abc ch=5\t' + b'\t'.join(USUAL))   # twenty fields: a basecaller's usual set
    hs.append(b'dup\tXX:i:1\tXX:i:2\tXX:Z:three')              # duplicate names are kept
    hs.append(b'nan\tna:f:nan\tnb:B:f,-nan,nan,1')
    return hs


def run_table(headers, device, text_align=lambda j: (5 * j) % 16, out_align=lambda j: (3 * j + 1) % 16):
    """The headers laid into a blob (header j at alignment text_align(j), between bytes that would change the
    result if they were read), planned, written with gaps between the outputs (part j at alignment
    out_align(j)). -> (chains, the table, counters, whether the gaps kept their bytes)."""
    from custom_porechop_abi_amd import engine
    parts = np.zeros(len(headers), engine.AUXPARSE_PART)
    blob = bytearray()
    for j, h in enumerate(headers):
        blob += b',7\t'
        while len(blob) % 16 != text_align(j):
            blob += b','
        parts[j]['text_off'], parts[j]['text_len'] = len(blob), len(h)
        blob += h
    blob += b',9\tXX:i:1'
    engine.auxparse_counts(reset=True)
    engine.auxparse_plan(bytes(blob), parts, device)
    counters = engine.auxparse_counts(reset=True)
    cursor = 7
    for j in range(len(headers)):
        if parts[j]['len'] > 0:
            while cursor % 16 != out_align(j):
                cursor += 1
            parts[j]['out'] = cursor
            cursor += int(parts[j]['len']) + 1
    out = np.full(cursor + 9, 0xEE, np.uint8)
    engine.auxparse_write(bytes(blob), parts, out, device)
    assert engine.auxparse_counts(reset=True) == (0, 0)      # the plan counts, not the write
    owned = np.zeros(out.size, bool)
    chains = []
    for p in parts:
        a, n = int(p['out']), int(p['len'])
        owned[a:a + n] = True
        chains.append(out[a:a + n].tobytes())
    table = [(int(p['len']), int(p['n_float']), int(p['tags']), int(p['left_out'])) for p in parts]
    return chains, table, counters, bool((out[~owned] == 0xEE).all())


def check_table(headers, device, **kw):
    chains, table, counters, gaps_kept = run_table(headers, device, **kw)
    tags = left = 0
    for j, h in enumerate(headers):
        want, t, l = R.parse(h)
        assert R.same_chain(chains[j], want), (j, h[:80], chains[j][:60], want[:60])
        nf = sum(1 if typ == 'f' else len(v) // 4 if sub == 'f' else 0 for _, typ, sub, v in R.walk(want))
        assert table[j] == (len(want), nf, t, l), (j, h[:80], table[j], (len(want), nf, t, l))
        tags, left = tags + t, left + l
    assert counters == (tags, left)
    assert gaps_kept
    return counters


def check_alignments(device):
    """A move table, a float array and a string at each of the 16 alignments of the blob crossed with each of
    the 16 alignments of the chain's destination."""
    for h in (b'r\tmv:B:c,5' + b',1,0' * 65, b'r\tfl:B:f' + b',0.5,-1e3' * 20 + b'\tde:f:2', b'r\tMM:Z:' + b'C+m,10,2,3;' * 9 + b'\tXS:i:300'):
        check_table([h] * 256, device, text_align=lambda j: j % 16, out_align=lambda j: j // 16)


def check_refusals(device):
    from custom_porechop_abi_amd import engine
    from custom_porechop_abi_amd._lib import PcabiError
    blob = b'a\tns:i:12345' + b'b\tXZ:Z:ab\tde:f:1'
    parts = np.zeros(2, engine.AUXPARSE_PART)
    parts['text_off'], parts['text_len'] = [0, 12], [12, 16]
    engine.auxparse_plan(blob, parts, device)
    assert parts['len'].tolist() == [5, 13] and parts['n_float'].tolist() == [0, 1]
    parts['out'] = [0, 20]
    out = np.zeros(40, np.uint8)
    engine.auxparse_write(blob, parts, out, device)
    assert out[:5].tobytes() == b'nsS\x39\x30' and out[20:33].tobytes() == b'XZZab\0def\x00\x00\x80\x3f'
    # a wrong len, overlapping outputs, an output outside the buffer, a part outside the text
    for change in ({'len': [4, 13]}, {'len': [5, 14]}, {'out': [0, 4]}, {'out': [0, 28]}, {'out': [-1, 20]}, {'text_len': [12, 17]},
                   {'text_off': [0, 13]}, {'text_off': [-1, 12]}, {'n_float': [1, 1]}):
        bad = parts.copy()
        for k, v in change.items():
            bad[k] = v
        with pytest.raises(PcabiError):
            engine.auxparse_write(blob, bad, out.copy(), device)
    bad = parts.copy()
    bad['text_len'] = [12, 17]
    with pytest.raises(PcabiError):
        engine.auxparse_plan(blob, bad, device)


def test_corpus_against_restatement():
    counters = check_table(header_corpus(), -1)
    assert counters[0] > 300 and counters[1] > 80      # both kinds are there


def test_alignments():
    check_alignments(-1)


def test_refusals():
    check_refusals(-1)


# ---- 3. the round trip through the existing formatter ------------------------------------------------------
def retyped(chain):
    """The chain without the tags its text leaves out, every integer scalar as the smallest type of its text
    (a '-' selects the signed ones), every float as the float32 of its '%g' text: six digits are what the
    text holds."""
    out = b''
    flags = [left for _, _, _, left in H.fields(chain)]
    for (tag, typ, raw), left in zip(mods_ref.walk_aux(chain), flags):
        if left:
            continue
        val = raw[3:]
        if typ in 'cCsSiI':
            t, v = R.int_tag(b'%d' % struct.unpack(H.FMT[typ], val)[0])
            out += tag + t.encode() + struct.pack(R.FMT[t], v)
        elif typ == 'f':
            out += tag + b'f' + R.float_bytes(H.number('f', val).encode())
        elif typ == 'B' and chr(val[0]) == 'f':
            n = struct.unpack_from('<I', val, 1)[0]
            out += tag + b'B' + val[:5] + b''.join(R.float_bytes(H.number('f', val[5 + 4 * k:9 + 4 * k]).encode()) for k in range(n))
        else:
            out += raw
    return out


def check_round_trip(device):
    from custom_porechop_abi_amd import engine
    chains = [c for c in HT.chain_corpus() if H.walks(c)]
    texts = engine.aux_text(chains, device)
    assert None not in texts and len(chains) > 150
    back = engine.aux_parse([b'n' + t for t in texts], device)
    assert engine.aux_text(back, device) == texts
    floats = 0
    for c, b in zip(chains, back):
        assert R.same_chain(b, retyped(c)), (c[:60], b[:60])
        floats += sum(1 if typ == 'f' else len(v) // 4 if sub == 'f' else 0 for _, typ, sub, v in R.walk(b))
    assert floats > 4000


def test_round_trip_through_the_formatter():
    check_round_trip(-1)


# ---- 4. files: the same reads as BAM and as text with the tags in the headers ----------------------------------
def file_case(tmp_path, n=60):
    """tests/test_moves_cpu.py's writer corpus (MM ML MN mv ts and other tags, the unusable kinds included), every
    record forward-strand, as in.bam; that batch written with today's header_tags path and no trims as
    src.fastq / src.fasta (and whatever `more` asks for); and trims and cuts derived from the reads' parts."""
    from custom_porechop_abi_amd import misc
    reads = V.writer_reads(n, with_mods=True)
    # (a tag that cannot stand in a header is not in the text file, and the two inputs would differ by it: the
    # corpus's one such tag, an mv string of control bytes, becomes a printable one)
    recs = [{'name': b'r%d' % i, 'seq': r['seq'], 'qual': [(7 * i + k) % 60 for k in range(len(r['seq']))], 'flag': 4,
             'aux': r['aux'].replace(b'mvZ\x05\x01\0', b'mvZ51\0') + b'qsC' + bytes([i % 200]) + b'def' + struct.pack('<f', 0.015625 * i)}
            for i, r in enumerate(reads)]
    assert all(H.counts(r['aux']) == (len(H.fields(r['aux'])), 0) for r in recs)
    src = str(tmp_path / 'in.bam')
    with open(src, 'wb') as f:
        f.write(B.make_bam(recs, b'@HD\tVN:1.6\tSO:unknown\n', (), 5000))
    batch = misc.load_batch(src, keep_aux=True)
    assert batch.n == len(reads) and bool(batch.as_stored.all())
    for fmt in ('fastq', 'fasta'):
        misc.write_reads(batch, str(tmp_path / ('src.' + fmt)), fmt, keep_aux=True, header_tags=True)
    st = [r['parts'][0][0] for r in reads]
    et = [r['l_seq'] - (r['parts'][-1][0] + r['parts'][-1][1]) for r in reads]
    cuts = [[(p[0] + p[1] - r['parts'][0][0], q[0] - r['parts'][0][0]) for p, q in zip(r['parts'], r['parts'][1:])] for r in reads]
    return batch, {'start_trim': st, 'end_trim': et, 'middle_cuts': cuts, 'min_split_read_size': 1}


def bam_records(path, quals=True):
    from custom_porechop_abi_amd import misc
    b = misc.load_batch(path, keep_aux=True)
    return [(b.name(i), b.sequence(i), b.quals(i) if quals else None, H.sam_text(b.aux(i))) for i in range(b.n)]


def check_files(tmp_path, from_bam, from_text, base, out_formats, quals=True, variants=None, **write_kw):
    """For every variant x tag option: write_reads of the batch read from text with tags_from_headers gives,
    byte for byte, the text the batch read from BAM gives; as 'bam', records with equal names, bases,
    qualities and SAM text of the aux; and the mods / moves counters agree between the two routes."""
    from custom_porechop_abi_amd import misc
    assert from_text.n == from_bam.n and from_text.aux_off is not None and bool(from_text.as_stored.all())
    seen = set()
    for vname, extra in (variants or HT.variants(from_bam.n)):
        for tags in HT.TAG_OPTIONS:
            kw = dict(base, **extra)
            for fmt in out_formats:
                paths, counts = {}, {}
                for route, batch in (('bam', from_bam), ('text', from_text)):
                    paths[route] = str(tmp_path / ('%s_out.%s' % (route, fmt)))
                    HT.counters_reset()
                    if fmt == 'bam':
                        n = misc.write_reads(batch, paths[route], 'bam', keep_aux=True, **kw, **tags)
                        misc.bgzf_finish(paths[route])
                    else:
                        n = misc.write_reads(batch, paths[route], fmt, keep_aux=True, header_tags=True, **kw, **tags, **write_kw)
                        if write_kw.get('bgzf'):
                            misc.bgzf_finish(paths[route])
                    counts[route] = (n, HT.counters_reset())
                assert counts['bam'] == counts['text'], (vname, tags, fmt, counts)
                if fmt == 'bam':
                    a, b = bam_records(paths['bam'], quals), bam_records(paths['text'], quals)
                    assert a == b and len(a) > 0, (vname, tags)
                else:
                    a, b = HT.read_text(paths['bam'], fmt), HT.read_text(paths['text'], fmt)
                    assert a == b and len(a) > 0, (vname, tags, fmt)
                    seen.add((vname, tuple(sorted(tags)), b'\tmv:B:c,' in a, b'\tMM:Z:' in a))
    return seen


def test_text_in_matches_bam_in(tmp_path):
    from custom_porechop_abi_amd import engine, misc
    from_bam, base = file_case(tmp_path)
    engine.auxparse_counts(reset=True)
    fq = misc.load_batch(str(tmp_path / 'src.fastq'), keep_aux=True, tags_from_headers=True)
    tags, left = engine.auxparse_counts(reset=True)
    assert tags > 4 * fq.n and left == 0
    seen = check_files(tmp_path, from_bam, fq, base, ('fastq', 'fasta', 'bam'))
    # the remapped tags are there when asked for
    assert ('cuts', ('keep_mods', 'keep_moves'), True, True) in seen
    fa = misc.load_batch(str(tmp_path / 'src.fasta'), keep_aux=True, tags_from_headers=True)
    assert [fa.aux(i) for i in range(fa.n)] == [fq.aux(i) for i in range(fq.n)]
    check_files(tmp_path, from_bam, fa, base, ('fasta', 'bam'), quals=False)
    # batches of a streamed read carry their own chains
    got = [b.aux(i) for b in misc.read_batches(str(tmp_path / 'src.fastq'), max_reads=7, keep_aux=True, tags_from_headers=True)
           for i in range(b.n)]
    assert got == [fq.aux(i) for i in range(fq.n)]


def test_names_with_comments_and_split_pieces(tmp_path):
    """The name part of such a batch is the header up to its first tab: the comment stays, the `_k` of a split
    piece goes where it goes today (in front of the first tab), and the parsed tags are not written a second time."""
    from custom_porechop_abi_amd import misc
    src = str(tmp_path / 'c.fastq')
    seq = 'ACGT' * 30
    with open(src, 'wb') as f:
        f.write(b'@read1 ch=5 x\tRG:Z:grp\tde:f:0.25\tmv:B:c,5' + b',1' * 120 + b'\tts:i:10\tbogus field\n' + seq.encode() + b'\n+\n' + b'I' * 120 + b'\n')
    batch = misc.load_batch(src, keep_aux=True, tags_from_headers=True)
    assert batch.aux(0) == b'RGZgrp\0def\x00\x00\x80\x3e' + V.mv_aux(5, [1] * 120) + b'tsC\x0a'
    out = str(tmp_path / 'o.fastq')
    misc.write_reads(batch, out, 'fastq', start_trim=[4], middle_cuts=[[(40, 50)]], min_split_read_size=1, keep_aux=True,
                     keep_moves=True, header_tags=True)
    recs = H.split_records(HT.read_text(out, 'fastq'), False)
    assert [r[0] for r in recs] == [b'read1 ch=5 x_1\tRG:Z:grp\tde:f:0.25\tmv:B:c,5' + b',1' * 40 + b'\tts:i:30',
                                    b'read1 ch=5 x_2\tRG:Z:grp\tde:f:0.25\tmv:B:c,5' + b',1' * 66 + b'\tts:i:280']
    # as BAM the name ends at the first blank
    misc.write_reads(batch, str(tmp_path / 'o.bam'), 'bam', keep_aux=True)
    misc.bgzf_finish(str(tmp_path / 'o.bam'))
    back = misc.load_batch(str(tmp_path / 'o.bam'), keep_aux=True)
    assert back.name(0) == 'read1' and back.aux(0) == batch.aux(0)


def test_option_off_is_todays_behaviour(tmp_path):
    """keep_aux alone on a FASTQ input still holds no aux, and what is written from it is today's bytes: the
    whole header verbatim. With the option on but header_tags off the text writers still copy the header."""
    from custom_porechop_abi_amd import misc
    _, base = file_case(tmp_path, 30)
    src = str(tmp_path / 'src.fastq')
    plain, kept, tagged = misc.load_batch(src), misc.load_batch(src, keep_aux=True), misc.load_batch(src, keep_aux=True, tags_from_headers=True)
    assert kept.aux_off is None and kept.aux(0) is None and tagged.aux_off is not None
    for fmt in ('fastq', 'fasta', 'fastq.gz'):
        a, b, c, d = (str(tmp_path / ('%s.%s' % (k, fmt))) for k in 'abcd')
        misc.write_reads(plain, a, fmt, **base)
        misc.write_reads(kept, b, fmt, keep_aux=True, header_tags=True, keep_mods=True, keep_moves=True, **base)
        misc.write_reads(tagged, c, fmt, **base)
        misc.write_reads(tagged, d, fmt, header_tags=False, **base)
        want = HT.read_text(a, fmt)
        assert HT.read_text(b, fmt) == want and HT.read_text(c, fmt) == want and HT.read_text(d, fmt) == want
    heads = [h for h, _, _ in H.split_records(HT.read_text(str(tmp_path / 'a.fastq'), 'fastq'), False)]
    assert sum(b'\tmv:B:c,' in h for h in heads) > 10       # today: the stale tags, copied with the header


# ---- 5. refusals of the Python surface and of the reader -------------------------------------------------------
def test_value_errors_and_raw_reader(tmp_path):
    import ctypes
    from custom_porechop_abi_amd import misc
    from custom_porechop_abi_amd._lib import lib
    from custom_porechop_abi_amd.pipeline import FileTrimmer
    src = str(tmp_path / 'x.fastq')
    with open(src, 'wb') as f:
        f.write(b'@r\tNM:i:5\nACGT\n+\nIIII\n')
    with pytest.raises(ValueError):
        misc.load_batch(src, tags_from_headers=True)
    with pytest.raises(ValueError):
        next(misc.read_batches(src, tags_from_headers=True))
    with pytest.raises(ValueError):
        misc.load_batch(src, raw=True, keep_aux=True, tags_from_headers=True)
    with pytest.raises(ValueError):
        FileTrimmer([], tags_from_headers=True)
    L = misc._declare(lib())
    for raw, want_ok in ((1, False), (0, True)):
        h = ctypes.c_void_p()
        assert L.pcabi_fastx_open(os.fsencode(src), raw, ctypes.byref(h)) == 0
        try:
            rc = L.pcabi_fastx_header_tags(h, 1, -1)
            assert (rc == 0) == want_ok
            if not want_ok:
                assert rc == -1 and b'raw' in L.pcabi_last_error()      # PCABI_E_ARG
        finally:
            L.pcabi_fastx_close(h)
    # a BAM reader: no effect
    bam = str(tmp_path / 'x.bam')
    with open(bam, 'wb') as f:
        f.write(B.make_bam([{'name': b'r', 'seq': 'ACGT', 'qual': [30] * 4, 'flag': 4, 'aux': b'NMC\x05'}], b'@HD\tVN:1.6\n', (), 5000))
    b = misc.load_batch(bam, keep_aux=True, tags_from_headers=True)
    assert b.aux(0) == b'NMC\x05'


# ---- 6. the shared header alone, under sanitizers ----------------------------------------------------------------
def test_auxparse_layer_under_sanitizers(tmp_path):
    """tests/auxparse_fuzz_main.cpp (csrc/pcabi_auxparse.h alone), built with -fsanitize=address,undefined as a
    program of its own and run as a child process: random and truncated headers in blocks of exactly their
    size, the 64 lanes of each pass played in turn against the byte-wise parse()."""
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path / 'auxparse_fuzz')
    base = ['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
            os.path.join(HERE, 'auxparse_fuzz_main.cpp')]
    for extra in (['-static-libasan', '-static-libubsan'], []):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        if r.returncode == 0:
            break
    if r.returncode != 0 and ('asan' in r.stderr or 'ubsan' in r.stderr or 'sanitize' in r.stderr):
        pytest.skip('the sanitizer runtime cannot be linked')
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, '1', '3000'], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'rounds 3000 fails 0' in r.stdout
