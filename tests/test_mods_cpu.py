"""Base-modification tags (MM / ML / MN) remapped onto parts of reads, without a GPU: the table-level
API with device=-1 (engine.mods_plan / mods_remap: the host build of csrc/pcabi_mods.h) and the BAM writer
with keep_mods, against tests/mods_ref.py's restatement and literals."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import bam_lib as B
from tests import mods_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- tables from reads ---------------------------------------------------------------------------------
def tables(reads):
    """reads: [{'seq': str (the reader's orientation), 'aux': bytes, 'parts': [(s0, ns)]}] ->
    (seq uint8, tags uint8, MODS_READ array, MODS_PART array)."""
    from custom_porechop_abi_amd import engine
    seq, tags = b'', b'\xee'   # (offset 0 is never a tag's)
    rd = np.zeros(len(reads), engine.MODS_READ)
    pt = np.zeros(sum(len(r['parts']) for r in reads), engine.MODS_PART)
    k = 0
    for i, r in enumerate(reads):
        mm, ml, mn, mm_tag, ml_tag, bad = R.mods_of_aux(r['aux'])
        rd[i] = (len(seq), len(tags), len(tags) + len(mm or b''), k, len(r['seq']), -1 if mm is None else len(mm),
                 -1 if ml is None else len(ml), -1 if mn is None or bad else mn, len(r['parts']),
                 (engine.MODS_OLD_MM if mm_tag == b'Mm' else 0) | (engine.MODS_OLD_ML if ml_tag == b'Ml' else 0) |
                 (engine.MODS_BAD if bad else 0))
        seq += r['seq'].encode()
        tags += (mm or b'') + (ml or b'')
        for s0, ns in r['parts']:
            pt[k] = (0, i, s0, ns, 0)
            k += 1
    return np.frombuffer(seq, np.uint8), np.frombuffer(tags, np.uint8), rd, pt


def run_tables(reads, device, gap=3):
    """-> ([tag bytes of every part], usable); the parts' outputs lie `gap` bytes apart in a buffer of
    0xA5, which must come back untouched around them."""
    from custom_porechop_abi_amd import engine
    seq, tags, rd, pt = tables(reads)
    pt, usable = engine.mods_plan(seq, tags, rd, pt, device=device)
    at = gap
    for k in range(pt.size):
        pt['out'][k] = at
        at += int(pt['len'][k]) + gap
    out = np.full(at, 0xA5, np.uint8)
    engine.mods_remap(seq, tags, rd, pt, out, device=device)
    got, owned = [], np.zeros(at, bool)
    for k in range(pt.size):
        a, n = int(pt['out'][k]), int(pt['len'][k])
        got.append(out[a:a + n].tobytes())
        owned[a:a + n] = True
    assert (out[~owned] == 0xA5).all()
    return got, usable


def expected_tags(r, s0, ns):
    """What the restatement says the table-level API writes for one part: the remapped tags alone."""
    if not R.read_usable(r['seq'], r['aux']):
        return b''
    return R.part_aux(r['seq'], b''.join(raw for tag, _, raw in R.walk_aux(r['aux']) if tag in R.POSITIONAL[:5]), s0, ns, False)


def check_against_ref(reads, got, usable):
    k = 0
    for i, r in enumerate(reads):
        ok = R.read_usable(r['seq'], r['aux'])
        assert bool(usable[i]) == ok, (i, r['aux'][:80])
        full = R.decode_aux(r['seq'], r['aux']) if ok else None
        for s0, ns in r['parts']:
            assert got[k] == expected_tags(r, s0, ns), (i, s0, ns, got[k][:80], r['aux'][:80])
            if ok:   # the semantic check: the output decoded against the part's own letters
                assert R.decode_aux(r['seq'][s0:s0 + ns], got[k]) == R.slice_records(full, s0, ns), (i, s0, ns)
            k += 1
    assert k == len(got)


# ---- the corpus ----------------------------------------------------------------------------------------
HEADERS = [('C', '+', 'm', ''), ('C', '+', 'h', '?'), ('C', '+', 'mh', '.'), ('A', '+', 'a', '?'), ('N', '+', 'n', ''),
           ('U', '+', 'e', '.'), ('G', '-', 'm', '?'), ('T', '+', '76792', ''), ('A', '-', '21839', '.'), ('G', '+', 'o', '')]


def make_tags(rng, seq, headers, density, with_ml=True, with_mn=None, old=False, pad_digits=False, empty=()):
    """The aux bytes of usable MM / ML / MN tags for seq: every group marks a random `density` share of its
    base's occurrences (none for the group indices in `empty`)."""
    mm, ml = b'', b''
    for g, (base, strand, codes, flag) in enumerate(headers):
        occ = R.occurrences(seq, base)
        pick = [] if g in empty else [o for o in range(len(occ)) if rng.rand() < density]
        mm += (base + strand + codes + flag).encode()
        last = -1
        for o in pick:
            d = o - last - 1
            mm += b',' + (b'%03d' % d if pad_digits and rng.rand() < 0.2 else b'%d' % d)
            last = o
            ml += bytes(rng.randint(0, 256, 1 if codes.isdigit() else len(codes)).astype(np.uint8))
        mm += b';'
    out = (b'Mm' if old else b'MM') + b'Z' + mm + b'\0'
    if with_ml:
        out += (b'Ml' if old else b'ML') + b'BC' + struct.pack('<I', len(ml)) + ml
    if with_mn is not None:
        out += b'MN' + {'i': b'i' + struct.pack('<i', len(seq)), 'S': b'S' + struct.pack('<H', len(seq) & 0xffff),
                        'I': b'I' + struct.pack('<I', len(seq))}[with_mn]
    return out


def random_parts(rng, n, k):
    """k disjoint ascending parts of [0, n) with gaps between and around them."""
    cuts = sorted(rng.choice(np.arange(1, max(n, 2 * k + 2)), 2 * k, replace=False).tolist()) if n > 2 * k + 2 else [0, n]
    return [(min(a, n), min(b, n) - min(a, n)) for a, b in zip(cuts[0::2], cuts[1::2])]


UNUSABLE = [   # (what, MM and friends as aux bytes) for the read CACCGCTCAGGT (C at 0 2 3 5 7)
    ('no ; at the end', b'MMZC+m,1\0'), ('bad base', b'MMZX+m,1;\0'), ('no strand', b'MMZCm,1;\0'), ('no code', b'MMZC+,1;\0'),
    ('upper code', b'MMZC+M,1;\0'), ('mixed code', b'MMZC+m5,1;\0'), ('two flags', b'MMZC+m.?,1;\0'),
    ('empty count', b'MMZC+m,,1;\0'), ('comma at the end', b'MMZC+m,1,;\0'), ('negative', b'MMZC+m,-1;\0'),
    ('space', b'MMZC+m, 1;\0'), ('text behind', b'MMZC+m,1;x\0'), ('count over int32', b'MMZC+m,2147483648;\0'),
    ('huge count', b'MMZC+m,99999999999999999999999;\0'), ('ordinal past the last C', b'MMZC+m,1,0,2;\0'),
    ('ordinal past the read (N)', b'MMZN+n,12;\0'), ('ML too short', b'MMZC+m,1,0;\0MLBC' + struct.pack('<I', 1) + b'\x07'),
    ('ML too long', b'MMZC+mh,1;\0MLBC' + struct.pack('<I', 3) + b'\x07\x08\x09'), ('MN wrong', b'MMZC+m,1;\0MNi' + struct.pack('<i', 11)),
    ('ML without MM', b'MLBC' + struct.pack('<I', 1) + b'\x07'), ('MN alone', b'MNi' + struct.pack('<i', 12)),
    ('MM and Mm', b'MMZC+m,1;\0MmZC+m,1;\0'), ('MM twice', b'MMZC+m,1;\0MMZC+h,1;\0'), ('MM not Z', b'MMAx'),
    ('ML of shorts', b'MMZC+m,1;\0MLBS' + struct.pack('<IH', 1, 7)), ('MN a float', b'MMZC+m,1;\0MNf' + struct.pack('<f', 12.0)),
    ('33 groups', b'MMZ' + b'C+m;' * 33 + b'\0'),
]
SHORT = 'CACCGCTCAGGT'


def corpus(seed=11, n=160):
    """Reads with every feature the issue lists; usable by construction but for the UNUSABLE ones mixed in."""
    rng = np.random.RandomState(seed)
    reads = []
    for i in range(n):
        ln = int(rng.choice([60, 130, 257, 400, 900]))
        letters = 'ACGT' if i % 4 else 'ACGTACGTACGTRYKMSWN'   # every fourth read with IUPAC letters
        seq = ''.join(rng.choice(list(letters), ln))
        kind = i % 16
        hs = [HEADERS[j] for j in rng.choice(len(HEADERS), int(rng.randint(1, 5)), replace=False)]
        if kind == 0:
            hs = [HEADERS[0], HEADERS[1], HEADERS[2]]          # C+m, C+h and C+mh side by side
        if kind == 1:
            hs = [HEADERS[4], HEADERS[5], HEADERS[7]]          # N, U, a ChEBI code
        kw = {'with_ml': kind != 2, 'with_mn': [None, 'i', 'S', 'I'][i % 4], 'old': kind == 3, 'pad_digits': kind == 4,
              'empty': (0,) if kind == 5 else ()}
        if kind == 6:
            aux = b'MMZ\0' + (b'MLBC' + struct.pack('<I', 0) if i % 32 == 6 else b'')   # an empty MM string
        elif kind == 7 and i % 32 == 7:
            aux = UNUSABLE[(i // 32) % len(UNUSABLE)][1]
            seq = SHORT + seq
        else:
            aux = make_tags(rng, seq, hs, 0.3, **kw)
        reads.append({'seq': seq, 'aux': aux, 'parts': random_parts(rng, len(seq), int(rng.randint(1, 6))),
                      'reverse': i % 3 == 1})
    return reads


_corpus = None


def shared_corpus():
    global _corpus
    if _corpus is None:
        _corpus = corpus()
    return _corpus


def corpus_conditions(reads):
    """(share of unusable reads, share of parts that both keep and lose an entry), from the restatement."""
    bad = both = parts = 0
    for r in reads:
        full = R.decode_aux(r['seq'], r['aux']) if R.read_usable(r['seq'], r['aux']) else None
        bad += full is None
        for s0, ns in r['parts']:
            parts += 1
            if full:
                kept = len(R.slice_records(full, s0, ns))
                both += 0 < kept < len(full)
    return bad / len(reads), both / parts


# ---- 1. the worked example ---------------------------------------------------------------------------
def test_worked_example():
    aux = b'MMZC+m?,1,0,1;\0MLBC' + struct.pack('<I', 3) + bytes([10, 20, 30])
    reads = [{'seq': 'CACCGCTC', 'aux': aux, 'parts': [(3, 5), (0, 3), (4, 3), (0, 8)]}]
    got, usable = run_tables(reads, -1)
    assert list(usable) == [1]
    ml = lambda *v: b'MLBC' + struct.pack('<I', len(v)) + bytes(v)   # noqa: E731
    assert got == [b'MMZC+m?,0,1;\0' + ml(20, 30), b'MMZC+m?,1;\0' + ml(10), b'MMZC+m?;\0' + ml(), aux]
    assert R.decode('CACCGCTC', b'C+m?,1,0,1;', bytes([10, 20, 30]), None) == [(2, 'C', '+', 'm', 10), (3, 'C', '+', 'm', 20),
                                                                              (7, 'C', '+', 'm', 30)]
    assert R.decode_aux('CGCTC', got[0]) == [(0, 'C', '+', 'm', 20), (4, 'C', '+', 'm', 30)]


def test_codes_and_mn():
    """ML order for a combined code (m@5, h@5, m@12, h@12), U counting T, N counting every base, MN."""
    seq = 'ATCGNTTCCAC'
    aux = (b'MMZC+mh,1,1;U-e.,0,1;N+n?,4,5;\0MLBC' + struct.pack('<I', 8) + bytes([1, 2, 3, 4, 5, 6, 7, 8]) + b'MNC' + bytes([11]))
    got, usable = run_tables([{'seq': seq, 'aux': aux, 'parts': [(4, 5), (0, 11), (9, 2)]}], -1)
    assert list(usable) == [1]
    # C at 2 7 8 10 -> C+mh marks 7 and 10; T at 1 5 6 -> U-e marks 1 and 6; N marks 4 and 10
    assert got[0] == b'MMZC+mh,0;U-e.,1;N+n?,0;\0MLBC' + struct.pack('<I', 4) + bytes([1, 2, 6, 7]) + b'MNi' + struct.pack('<i', 5)
    assert got[1] == aux[:-4] + b'MNi' + struct.pack('<i', 11)
    assert got[2] == b'MMZC+mh,0;U-e.;N+n?,1;\0MLBC' + struct.pack('<I', 3) + bytes([3, 4, 8]) + b'MNi' + struct.pack('<i', 2)


# ---- 2. the corpus -------------------------------------------------------------------------------------
def test_corpus_conditions():
    bad, both = corpus_conditions(shared_corpus())
    assert 0 < bad <= 0.10, bad
    assert both >= 0.5, both


def test_corpus_against_restatement():
    reads = shared_corpus()
    got, usable = run_tables(reads, -1)
    check_against_ref(reads, got, usable)


def test_counters():
    from custom_porechop_abi_amd import engine
    reads = shared_corpus()
    seq, tags, rd, pt = tables(reads)
    engine.mods_counts(reset=True)
    _, usable = engine.mods_plan(seq, tags, rd, pt, device=-1)
    good = sum(R.read_usable(r['seq'], r['aux']) for r in reads)
    assert engine.mods_counts(reset=True) == (good, len(reads) - good) and int(usable.sum()) == good
    assert engine.mods_counts() == (0, 0)


# ---- 3. what is not usable -----------------------------------------------------------------------------
@pytest.mark.parametrize('what,aux', UNUSABLE, ids=[w for w, _ in UNUSABLE])
def test_unusable_tags_are_dropped(what, aux):
    good = {'seq': SHORT, 'aux': b'MMZC+m,1;\0', 'parts': [(1, 9)]}
    reads = [good, {'seq': SHORT, 'aux': aux, 'parts': [(0, 12), (2, 5)]}, good]
    assert not R.read_usable(SHORT, aux)
    got, usable = run_tables(reads, -1)
    assert list(usable) == [1, 0, 1]
    assert got == [b'MMZC+m,0;\0', b'', b'', b'MMZC+m,0;\0']


def test_group_limit_is_32():
    aux = b'MMZ' + b'C+m,0;' + b'A-a?;' * 31 + b'\0'
    got, usable = run_tables([{'seq': SHORT, 'aux': aux, 'parts': [(1, 11)]}], -1)
    assert list(usable) == [1] and got == [b'MMZ' + b'C+m;' + b'A-a?;' * 31 + b'\0']


def test_tables_outside_their_buffers_are_refused():
    from custom_porechop_abi_amd import engine
    reads = [{'seq': SHORT, 'aux': b'MMZC+m,1;\0MLBC' + struct.pack('<I', 1) + b'\x07', 'parts': [(1, 9), (0, 3)]}]
    seq, tags, rd, pt = tables(reads)
    for field, value in (('seq_off', 1), ('l_seq', 13), ('mm_off', tags.size), ('mm_len', tags.size), ('ml_off', tags.size),
                         ('part0', 1), ('n_parts', 3), ('seq_off', -1)):
        bad = rd.copy()
        bad[field][0] = value
        with pytest.raises(Exception, match='does not fit|does not lie|belongs to no read'):
            engine.mods_plan(seq, tags, bad, pt.copy(), device=-1)
    for field, value in (('s0', -1), ('ns', 13), ('read', 1), ('read', -1)):
        bad = pt.copy()
        bad[field][1] = value
        with pytest.raises(Exception, match='does not fit|does not lie|belongs to no read'):
            engine.mods_plan(seq, tags, rd, bad, device=-1)
    pt, _ = engine.mods_plan(seq, tags, rd, pt, device=-1)
    pt['out'] = [0, int(pt['len'][0])]
    out = np.zeros(int(pt['len'].sum()), np.uint8)
    engine.mods_remap(seq, tags, rd, pt, out, device=-1)
    for field, value in (('len', int(pt['len'][1]) + 1), ('out', out.size), ('out', 1), ('out', -1)):
        bad = pt.copy()
        bad[field][1] = value
        with pytest.raises(Exception, match="not the plan's|does not fit the output|overlap"):
            engine.mods_remap(seq, tags, rd, bad, out, device=-1)


# ---- 4. the writer -------------------------------------------------------------------------------------
def writer_case(tmp_path, reads, name='in.bam'):
    """The corpus as a BAM (RG before and qs behind the modification tags; `reverse` reads stored
    reverse-complemented), loaded with keep_aux, and trims / cuts derived from the reads' parts."""
    from custom_porechop_abi_amd import misc
    recs = []
    for i, r in enumerate(reads):
        seq, qual, flag = r['seq'], [(7 * i + k) % 60 for k in range(len(r['seq']))], 4
        if r.get('reverse'):
            seq, qual, flag = ''.join(B.COMPLEMENT[c] for c in reversed(seq)), qual[::-1], 4 | 0x10
        recs.append({'name': b'r%d' % i, 'seq': seq, 'qual': qual, 'flag': flag,
                     'aux': b'RGZgrp\0' + r['aux'] + b'mvBc' + struct.pack('<I', 2) + b'\x05\x01' + b'qsC' + bytes([i % 200])})
    path = str(tmp_path / name)
    with open(path, 'wb') as f:
        f.write(B.make_bam(recs, b'@HD\tVN:1.6\tSO:unknown\n', (), 5000))
    # parts -> start trim, end trim and the cuts between the parts (relative to the trimmed read)
    st, et, cuts = [], [], []
    for r in reads:
        ps = [p for p in r['parts'] if p[1] > 0]
        if not ps or r.get('whole'):
            ps = [(0, len(r['seq']))]
            r = dict(r, parts=ps)
        a, e = ps[0][0], ps[-1][0] + ps[-1][1]
        st.append(a)
        et.append(len(r['seq']) - e)
        cuts.append([(p[0] + p[1] - a, q[0] - a) for p, q in zip(ps, ps[1:])])
    return path, recs, st, et, cuts


def written_parts(reads):
    for i, r in enumerate(reads):
        ps = [p for p in r['parts'] if p[1] > 0]
        if not ps or r.get('whole'):
            ps = [(0, len(r['seq']))]
        merged = []   # parts that touch are one piece to the writer
        for p in ps:
            if merged and merged[-1][0] + merged[-1][1] == p[0]:
                merged[-1] = (merged[-1][0], merged[-1][1] + p[1])
            else:
                merged.append(p)
        for s0, ns in merged:
            yield i, r, s0, ns, (s0 == 0 and ns == len(r['seq']) and len(merged) == 1)


def check_written(back, reads, recs, keep_mods):
    exp = list(written_parts(reads))
    assert back.n == len(exp)
    kept_some = 0
    for k, (i, r, s0, ns, whole) in enumerate(exp):
        assert back.seq[back.seq_off[k]:back.seq_off[k + 1]].tobytes().decode() == r['seq'][s0:s0 + ns]
        want = R.part_aux(r['seq'], recs[i]['aux'], s0, ns, whole and not r.get('reverse'), keep_mods)
        assert back.aux(k) == want, (k, i, s0, ns, back.aux(k)[:90], want[:90])
        if keep_mods and R.read_usable(r['seq'], r['aux']):
            full = R.decode_aux(r['seq'], r['aux'])
            assert R.decode_aux(r['seq'][s0:s0 + ns], back.aux(k)) == R.slice_records(full, s0, ns)
            kept_some += bool(R.slice_records(full, s0, ns)) and not (whole and not r.get('reverse'))
    return kept_some


def write_case(tmp_path, reads, gzip_device, keep_mods, name):
    from custom_porechop_abi_amd import engine, misc
    path, recs, st, et, cuts = writer_case(tmp_path, reads)
    batch = misc.load_batch(path, keep_aux=True)
    out = str(tmp_path / name)
    engine.mods_counts(reset=True)
    n = misc.write_reads(batch, out, 'bam', start_trim=st, end_trim=et, middle_cuts=cuts, min_split_read_size=1,
                         gzip_device=gzip_device, keep_aux=True, keep_mods=keep_mods)
    misc.bgzf_finish(out)
    assert n == len(reads)
    return out, recs, engine.mods_counts(reset=True)


def writer_reads():
    reads = [dict(r) for r in shared_corpus()[:96]]
    for i in (0, 1, 9, 20):
        reads[i]['whole'] = True   # written whole: forward ones verbatim, reverse ones remapped with s0 = 0
    return reads


def test_writer_keep_mods(tmp_path):
    from custom_porechop_abi_amd import misc
    reads = writer_reads()
    out, recs, counts = write_case(tmp_path, reads, None, True, 'out.bam')
    back = misc.load_batch(out, keep_aux=True)
    assert check_written(back, reads, recs, True) > len(reads) // 2
    changed = [r for i, r, s0, ns, whole in written_parts(reads) if not (whole and not r.get('reverse'))]
    uniq = {id(r): r for r in changed}.values()
    good = sum(R.read_usable(r['seq'], r['aux']) for r in uniq)
    assert counts == (good, len(uniq) - good) and len(uniq) - good > 0
    # and with the option off: today's rule
    out, recs, counts = write_case(tmp_path, reads, None, False, 'off.bam')
    check_written(misc.load_batch(out, keep_aux=True), reads, recs, False)
    assert counts == (0, 0)


def unusable_reads(cases=None):
    """Every UNUSABLE entry twice -- trimmed, and stored reverse-strand and written whole -- each between
    usable reads: what the writer's own walk of the aux chain has to find (exactly one MM, no tag twice,
    the types) as well as what the text and the lengths show."""
    good = {'seq': SHORT, 'aux': b'MMZC+m,1;\0MNC' + bytes([12]), 'parts': [(1, 9)]}
    reads = [dict(good)]
    for _, aux in (UNUSABLE if cases is None else cases):
        reads += [{'seq': SHORT, 'aux': aux, 'parts': [(2, 5)]}, dict(good),
                  {'seq': SHORT, 'aux': aux, 'parts': [(0, 12)], 'reverse': True}, dict(good, reverse=True)]
    return reads


@pytest.mark.parametrize('what,aux', UNUSABLE, ids=[w for w, _ in UNUSABLE])
def test_writer_drops_unusable_tags_and_keeps_the_others(tmp_path, what, aux):
    """The writer finds the read unusable itself (pcabi_reads_write_bam walks the chain): its parts carry RG
    and qs and none of MM ML MN mv, it is counted as dropped, and its neighbours are remapped."""
    from custom_porechop_abi_amd import misc
    reads = unusable_reads([(what, aux)])
    out, recs, counts = write_case(tmp_path, reads, None, True, 'out.bam')
    back = misc.load_batch(out, keep_aux=True)
    check_written(back, reads, recs, True)
    assert counts == (3, 2)
    for k in (1, 3):
        assert back.aux(k) == b'RGZgrp\0qsC' + bytes([k])
    for k in (0, 2):
        assert back.aux(k) == b'RGZgrp\0qsC' + bytes([k]) + b'MMZC+m,0;\0MNi' + struct.pack('<i', 9)


def test_keep_mods_needs_the_tags(tmp_path):
    from custom_porechop_abi_amd import misc
    from custom_porechop_abi_amd.pipeline import FileTrimmer
    path, *_ = writer_case(tmp_path, shared_corpus()[:3])
    batch = misc.load_batch(path, keep_aux=True)
    with pytest.raises(ValueError):
        misc.write_reads(batch, str(tmp_path / 'x.bam'), 'bam', keep_mods=True)
    with pytest.raises(ValueError):
        misc.write_reads(batch, str(tmp_path / 'x.fastq'), 'fastq', keep_aux=True, keep_mods=True)
    with pytest.raises(ValueError):
        FileTrimmer([], keep_mods=True)


# ---- 5. the shared header alone, under sanitizers -------------------------------------------------------
def test_mods_layer_under_sanitizers(tmp_path):
    """tests/mods_fuzz_main.cpp (csrc/pcabi_mods.h alone), built with -fsanitize=address,undefined as a
    program of its own and run as a child process: random tag bytes, random part tables, valid tags with
    single bytes flipped, the outputs in buffers of exactly their planned size, and the kernel's strided
    byte copies against the host's."""
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path / 'mods_fuzz')
    base = ['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
            os.path.join(HERE, 'mods_fuzz_main.cpp')]
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
