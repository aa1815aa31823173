"""Move tables (mv) and ts remapped onto parts of reads, without a GPU: the table-level API with device=-1
(engine.moves_plan / moves_remap: the host build of csrc/pcabi_moves.h) and the BAM writer with keep_moves,
against tests/moves_ref.py's restatement and literals."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import bam_lib as B
from tests import moves_ref as M
from tests import test_mods_cpu as C

HERE = os.path.dirname(os.path.abspath(__file__))
INT32_MAX = 2 ** 31 - 1


# ---- move tables and their tags ------------------------------------------------------------------------
def make_moves(rng, l_seq, mean=2.0, lead=0):
    """l_seq ones with geometric dwells of the given mean, behind `lead` zeros."""
    if l_seq == 0:
        return [0] * lead
    dwell = rng.geometric(1.0 / mean, l_seq)
    mv = np.zeros(lead + int(dwell.sum()), np.uint8)
    mv[lead + np.concatenate([[0], np.cumsum(dwell)[:-1]]).astype(np.int64)] = 1
    return mv.tolist() if l_seq else [0] * lead


def mv_aux(stride, moves, sub=b'c'):
    return b'mvB' + sub + struct.pack('<I', 1 + len(moves)) + bytes([stride & 0xFF]) + bytes(moves)


def ts_aux(v, typ='i'):
    return b'ts' + typ.encode() + struct.pack(M.INT_FMT[typ], v)


def tables(reads, pads=None, tail=0):
    """reads: [{'l_seq': int, 'aux': bytes, 'parts': [(s0, ns)]}] -> (tags uint8, MOVES_READ array, MOVES_PART
    array). The blob is the reads' aux chains, each behind pads[i] bytes (1 when not given: offset 0 is never
    a tag's) and `tail` bytes behind the last; a read without mv has no entry."""
    from custom_porechop_abi_amd import engine
    with_mv = [r for r in reads if M.moves_of_aux(r['aux']) is not None]
    tags = b''
    rd = np.zeros(len(with_mv), engine.MOVES_READ)
    pt = np.zeros(sum(len(r['parts']) for r in with_mv), engine.MOVES_PART)
    k = 0
    for i, r in enumerate(with_mv):
        tags += b'\xee' * (1 if pads is None else pads[i])
        vals, ts, bad = M.moves_of_aux(r['aux'])
        at = 0
        for tag, typ, raw in M.walk_aux(r['aux']):
            if tag == b'mv' and not bad:
                rd[i]['mv_off'] = len(tags) + at + 8
            at += len(raw)
        rd[i]['part0'], rd[i]['l_seq'], rd[i]['n_vals'] = k, r['l_seq'], len(vals)
        rd[i]['ts'] = -1 if ts is None or bad else ts
        rd[i]['n_parts'], rd[i]['flags'] = len(r['parts']), engine.MOVES_BAD if bad else 0
        tags += r['aux']
        for s0, ns in r['parts']:
            pt[k] = (0, i, s0, ns, 0)
            k += 1
    tags += b'\xee' * tail
    return np.frombuffer(tags, np.uint8), rd, pt


def run_tables(reads, device, gap=3, pads=None, tail=0):
    """-> ([tag bytes of every part of the reads with mv], usable); the parts' outputs lie `gap` bytes apart
    in a buffer of 0xA5, which must come back untouched around them."""
    from custom_porechop_abi_amd import engine
    tags, rd, pt = tables(reads, pads, tail)
    pt, usable = engine.moves_plan(tags, rd, pt, device=device)
    at = gap
    for k in range(pt.size):
        pt['out'][k] = at
        at += int(pt['len'][k]) + gap
    out = np.full(at, 0xA5, np.uint8)
    engine.moves_remap(tags, rd, pt, out, device=device)
    got, owned = [], np.zeros(at, bool)
    for k in range(pt.size):
        a, n = int(pt['out'][k]), int(pt['len'][k])
        got.append(out[a:a + n].tobytes())
        owned[a:a + n] = True
    assert (out[~owned] == 0xA5).all()
    return got, usable


def check_against_ref(reads, got, usable):
    k = i = 0
    for r in reads:
        if M.moves_of_aux(r['aux']) is None:
            continue
        want, ok = M.read_tags(r['aux'], r['l_seq'], r['parts'])
        assert bool(usable[i]) == ok, (i, r['aux'][:60])
        for j, (s0, ns) in enumerate(r['parts']):
            assert got[k] == want[j], (i, s0, ns, got[k][:40], want[j][:40])
            k += 1
        i += 1
    assert k == len(got) and i == len(usable)


def tiling(rng, n, k):
    """k ascending parts that tile [0, n), only the first of which starts the read."""
    if n == 0:
        return [(0, 0)]
    cuts = [0] + sorted(rng.randint(1, n + 1, k - 1).tolist()) + [n]
    return [(a, b - a) for a, b in zip(cuts, cuts[1:])]


def corpus(seed=23, n=300):
    rng = np.random.RandomState(seed)
    reads = []
    for i in range(n):
        l_seq = int(rng.choice([0, 1, 5, 60, 130, 257, 900, 2500]))
        stride = int(rng.choice([1, 5, 6, 10, 127]))
        moves = make_moves(rng, l_seq, 1.0 + 2.0 * rng.rand(), lead=int(rng.randint(0, 40)) if i % 3 == 0 else 0)
        aux = b'RGZgrp\0'
        if i % 4:
            typ = 'cCsSiI'[i % 6]
            aux += ts_aux(int(rng.randint(0, [100, 200, 30000, 60000, 10 ** 6, 10 ** 6][i % 6])), typ)
        aux += mv_aux(stride, moves, b'C' if i % 5 == 0 else b'c') + b'nsi' + struct.pack('<i', 12345 + i)
        if i % 37 == 36 and l_seq >= 5:
            aux = UNUSABLE[(i // 37) % len(UNUSABLE)][1](l_seq, stride, moves)
        parts = tiling(rng, l_seq, int(rng.randint(1, 6))) if i % 2 else C.random_parts(rng, l_seq, int(rng.randint(1, 5)))
        reads.append({'l_seq': l_seq, 'aux': aux, 'parts': parts, 'tiles': bool(i % 2), 'reverse': i % 3 == 1})
    return reads


UNUSABLE = [   # (what, aux bytes of (l_seq, stride, moves) usable but for that)
    ('mv of shorts', lambda n, s, m: b'mvBs' + struct.pack('<I', 1 + len(m)) + struct.pack('<%dh' % (1 + len(m)), s, *m)),
    ('mv a string', lambda n, s, m: b'mvZ\x05\x01\0'),
    ('mv twice', lambda n, s, m: mv_aux(s, m) + mv_aux(s, m)),
    ('no values', lambda n, s, m: b'mvBc' + struct.pack('<I', 0)),
    ('stride 0', lambda n, s, m: mv_aux(0, m)),
    ('stride negative', lambda n, s, m: mv_aux(-3, m)),
    ('stride 128 (B:C)', lambda n, s, m: mv_aux(128, m, b'C')),
    ('a move of 2', lambda n, s, m: mv_aux(s, m[:len(m) // 2] + [2] + m[len(m) // 2 + 1:])),
    ('a move of 0xFF', lambda n, s, m: mv_aux(s, m[:-1] + [0xFF])),
    ('ones above l_seq', lambda n, s, m: mv_aux(s, m + [1])),
    ('ones below l_seq', lambda n, s, m: mv_aux(s, m[:m.index(1)] + [0] + m[m.index(1) + 1:])),
    ('ts negative', lambda n, s, m: ts_aux(-1, 'i') + mv_aux(s, m)),
    ('ts a string', lambda n, s, m: b'tsZ12\0' + mv_aux(s, m)),
    ('ts a float', lambda n, s, m: b'tsf' + struct.pack('<f', 12.0) + mv_aux(s, m)),
    ('ts twice', lambda n, s, m: ts_aux(3, 'C') + mv_aux(s, m) + ts_aux(3, 'C')),
    ('ts overflow', lambda n, s, m: ts_aux(INT32_MAX - 3, 'i') + mv_aux(s, m)),
    ('ts above int32', lambda n, s, m: ts_aux(INT32_MAX + 1, 'I') + mv_aux(s, m)),
]
SHORT_MOVES = [0, 1, 0, 1, 1, 0, 0, 1, 1, 0, 1, 0]   # 6 bases; p = 1 3 4 7 8 10, n = 12


_corpus = None


def shared_corpus():
    global _corpus
    if _corpus is None:
        _corpus = corpus()
    return _corpus


# ---- 1. the worked example ---------------------------------------------------------------------------
def test_worked_example():
    aux = ts_aux(100, 'S') + mv_aux(5, SHORT_MOVES)
    reads = [{'l_seq': 6, 'aux': aux, 'parts': [(0, 6), (0, 2), (2, 3), (5, 1), (6, 0), (0, 0), (1, 0)]}]
    got, usable = run_tables(reads, -1)
    assert list(usable) == [1]
    tag = lambda moves, ts: b'mvBc' + struct.pack('<I', 1 + len(moves)) + b'\x05' + bytes(moves) + b'tsi' + struct.pack('<i', ts)   # noqa: E731
    assert got == [tag(SHORT_MOVES, 100), tag([0, 1, 0, 1], 100), tag([1, 0, 0, 1, 1, 0], 120), tag([1, 0], 150), tag([], 160),
                   tag([0], 100), tag([], 115)]
    assert got == M.read_tags(aux, 6, reads[0]['parts'])[0]
    # without ts no ts is written; B:C comes out as B:c
    got, _ = run_tables([{'l_seq': 6, 'aux': mv_aux(5, SHORT_MOVES, b'C'), 'parts': [(2, 3)]}], -1)
    assert got == [b'mvBc' + struct.pack('<I', 7) + b'\x05' + bytes([1, 0, 0, 1, 1, 0])]


# ---- 2. the corpus -------------------------------------------------------------------------------------
def test_corpus_against_restatement():
    reads = shared_corpus()
    assert len(reads) == 300
    got, usable = run_tables(reads, -1)
    check_against_ref(reads, got, usable)
    assert 0 < (usable == 0).sum() <= 30


def test_tiling_parts_concatenate_and_hold_their_ones():
    reads = shared_corpus()
    got, usable = run_tables(reads, -1)
    k = tiled = 0
    for i, r in enumerate(reads):
        vals, ts, bad = M.moves_of_aux(r['aux'])
        slices = []
        for s0, ns in r['parts']:
            if usable[i]:
                n = struct.unpack_from('<I', got[k], 4)[0]
                body = got[k][9:8 + n]
                assert got[k][:4] == b'mvBc' and got[k][8] == vals[0] and len(body) == n - 1
                assert sum(body) == ns and set(body) <= {0, 1}
                slices.append(body)
                if ts is not None:
                    q0 = sum(len(s) for s in slices[:-1]) if r['tiles'] else M.slice_of(vals[1:], s0, ns)[0]
                    assert got[k][8 + n:] == b'tsi' + struct.pack('<i', ts + vals[0] * q0)
            k += 1
        if usable[i] and r['tiles']:
            assert b''.join(slices) == bytes(vals[1:])
            tiled += 1
    assert tiled > 100


def test_counters():
    from custom_porechop_abi_amd import engine
    reads = shared_corpus()
    tags, rd, pt = tables(reads)
    engine.moves_counts(reset=True)
    _, usable = engine.moves_plan(tags, rd, pt, device=-1)
    good = sum(M.read_tags(r['aux'], r['l_seq'], r['parts'])[1] for r in reads)
    assert engine.moves_counts(reset=True) == (good, len(reads) - good) and int(usable.sum()) == good
    assert engine.moves_counts() == (0, 0)


# ---- 3. what is not usable -----------------------------------------------------------------------------
@pytest.mark.parametrize('what,make', UNUSABLE, ids=[w for w, _ in UNUSABLE])
def test_unusable_tables_are_dropped(what, make):
    from custom_porechop_abi_amd import engine
    good = {'l_seq': 6, 'aux': ts_aux(7, 'C') + mv_aux(5, SHORT_MOVES), 'parts': [(1, 4)]}
    reads = [good, {'l_seq': 6, 'aux': make(6, 5, SHORT_MOVES), 'parts': [(0, 6), (2, 3)]}, good]
    assert M.read_tags(reads[1]['aux'], 6, reads[1]['parts'])[1] is False
    engine.moves_counts(reset=True)
    got, usable = run_tables(reads, -1)
    assert engine.moves_counts(reset=True) == (2, 1)
    assert list(usable) == [1, 0, 1]
    want = b'mvBc' + struct.pack('<I', 8) + b'\x05' + bytes([1, 1, 0, 0, 1, 1, 0]) + b'tsi' + struct.pack('<i', 7 + 5 * 3)
    assert got == [want, b'', b'', want]


def test_ts_overflow_depends_on_the_parts():
    aux = ts_aux(INT32_MAX - 3, 'i') + mv_aux(5, SHORT_MOVES)
    got, usable = run_tables([{'l_seq': 6, 'aux': aux, 'parts': [(0, 4)]}, {'l_seq': 6, 'aux': aux, 'parts': [(0, 4), (1, 2)]}], -1)
    assert list(usable) == [1, 0] and got[1:] == [b'', b''] and got[0].endswith(b'tsi' + struct.pack('<i', INT32_MAX - 3))


def test_tables_outside_their_buffers_are_refused():
    from custom_porechop_abi_amd import engine
    reads = [{'l_seq': 6, 'aux': ts_aux(7, 'C') + mv_aux(5, SHORT_MOVES), 'parts': [(1, 4), (0, 3)]}]
    tags, rd, pt = tables(reads)
    for field, value in (('mv_off', tags.size), ('mv_off', -1), ('n_vals', tags.size), ('n_vals', -1), ('l_seq', -1), ('part0', 1),
                         ('n_parts', 3), ('n_parts', -1)):
        bad = rd.copy()
        bad[field][0] = value
        with pytest.raises(Exception, match='does not fit|does not lie|belongs to no read'):
            engine.moves_plan(tags, bad, pt.copy(), device=-1)
    for field, value in (('s0', -1), ('ns', 7), ('s0', 4), ('read', 1), ('read', -1)):
        bad = pt.copy()
        bad[field][1] = value
        with pytest.raises(Exception, match='does not fit|does not lie|belongs to no read'):
            engine.moves_plan(tags, rd, bad, device=-1)
    pt, _ = engine.moves_plan(tags, rd, pt, device=-1)
    pt['out'] = [0, int(pt['len'][0])]
    out = np.zeros(int(pt['len'].sum()), np.uint8)
    engine.moves_remap(tags, rd, pt, out, device=-1)
    for field, value in (('len', int(pt['len'][1]) + 1), ('out', out.size), ('out', 1), ('out', -1)):
        bad = pt.copy()
        bad[field][1] = value
        with pytest.raises(Exception, match="not the plan's|does not fit the output|overlap"):
            engine.moves_remap(tags, rd, bad, out, device=-1)


# ---- 4. the writer -------------------------------------------------------------------------------------
def writer_reads(n=90, with_mods=False):
    """Corpus reads with letters (and, with_mods, usable MM / ML / MN in front of the other tags); parts
    that do not touch (the writer joins touching ones); a few written whole; the unusable kinds between."""
    rng = np.random.RandomState(4)
    reads = []
    for i, r in enumerate(shared_corpus()[:n]):
        r = dict(r, seq=''.join(rng.choice(list('ACGT'), r['l_seq'])))
        if r['l_seq'] == 0:
            continue
        if with_mods and i % 3:
            r['mods'] = C.make_tags(rng, r['seq'], [C.HEADERS[0], C.HEADERS[3]], 0.3, with_mn='i')
            r['aux'] = r['mods'] + r['aux']
        r['parts'] = [p for p in C.random_parts(rng, r['l_seq'], int(rng.randint(1, 4))) if p[1] > 0] or [(0, r['l_seq'])]
        if i % 11 == 0:
            r['parts'] = [(0, r['l_seq'])]    # written whole: forward ones verbatim, reverse ones remapped
        reads.append(r)
    for k, (_, make) in enumerate(UNUSABLE):
        moves = make_moves(rng, 40, 2.0)
        reads.insert(3 * k + 1, {'l_seq': 40, 'seq': ''.join(rng.choice(list('ACGT'), 40)), 'parts': [(3, 20), (30, 5)],
                                 'aux': b'RGZgrp\0' + make(40, 5, moves) + b'nsi' + struct.pack('<i', 77), 'reverse': k % 2 == 1})
    return reads


def write_case(tmp_path, reads, gzip_device, keep_moves, name, keep_mods=False):
    """The reads as a BAM (`reverse` ones stored reverse-complemented: mv is not reversed), loaded with
    keep_aux and written with trims and cuts derived from the parts. -> (path, moves counters)."""
    from custom_porechop_abi_amd import engine, misc
    recs = []
    for i, r in enumerate(reads):
        seq, qual, flag = r['seq'], [(7 * i + k) % 60 for k in range(len(r['seq']))], 4
        if r.get('reverse'):
            seq, qual, flag = ''.join(B.COMPLEMENT[c] for c in reversed(seq)), qual[::-1], 4 | 0x10
        recs.append({'name': b'r%d' % i, 'seq': seq, 'qual': qual, 'flag': flag, 'aux': r['aux'] + b'qsC' + bytes([i % 200])})
    src = str(tmp_path / 'in.bam')
    with open(src, 'wb') as f:
        f.write(B.make_bam(recs, b'@HD\tVN:1.6\tSO:unknown\n', (), 5000))
    st = [r['parts'][0][0] for r in reads]
    et = [r['l_seq'] - (r['parts'][-1][0] + r['parts'][-1][1]) for r in reads]
    cuts = [[(p[0] + p[1] - r['parts'][0][0], q[0] - r['parts'][0][0]) for p, q in zip(r['parts'], r['parts'][1:])] for r in reads]
    batch = misc.load_batch(src, keep_aux=True)
    out = str(tmp_path / name)
    engine.moves_counts(reset=True)
    n = misc.write_reads(batch, out, 'bam', start_trim=st, end_trim=et, middle_cuts=cuts, min_split_read_size=1,
                         gzip_device=gzip_device, keep_aux=True, keep_mods=keep_mods, keep_moves=keep_moves)
    misc.bgzf_finish(out)
    assert n == len(reads)
    return out, engine.moves_counts(reset=True)


def check_written(back, reads, keep_moves, keep_mods=False):
    """Every written record against the restatement; -> how many changed parts carry an mv."""
    k = with_mv = 0
    for i, r in enumerate(reads):
        for j, (s0, ns) in enumerate(r['parts']):
            assert back.seq[back.seq_off[k]:back.seq_off[k + 1]].tobytes().decode() == r['seq'][s0:s0 + ns]
            verbatim = (s0, ns) == (0, r['l_seq']) and not r.get('reverse')
            mods = C.expected_tags({'seq': r['seq'], 'aux': r['mods']}, s0, ns) if keep_mods and 'mods' in r else b''
            want = M.part_aux(r['aux'] + b'qsC' + bytes([i % 200]), r['l_seq'], r['parts'], j, verbatim, keep_moves, mods)
            assert back.aux(k) == want, (k, i, s0, ns, back.aux(k)[:90], want[:90])
            with_mv += not verbatim and b'mvBc' in want
            k += 1
    assert back.n == k
    return with_mv


def changed_counts(reads):
    """(usable, not usable) among the reads with an mv that are written changed."""
    good = bad = 0
    for r in reads:
        if r['parts'] == [(0, r['l_seq'])] and not r.get('reverse'):
            continue
        if M.moves_of_aux(r['aux']) is not None:
            ok = M.read_tags(r['aux'], r['l_seq'], r['parts'])[1]
            good, bad = good + ok, bad + (not ok)
    return good, bad


def test_writer_keep_moves(tmp_path):
    from custom_porechop_abi_amd import misc
    reads = writer_reads()
    out, counts = write_case(tmp_path, reads, None, True, 'out.bam')
    back = misc.load_batch(out, keep_aux=True)
    assert check_written(back, reads, True) > len(reads) // 2
    assert counts == changed_counts(reads) and counts[1] >= len(UNUSABLE)
    # tag order on one changed usable read with a ts in front of mv: the others in file order, then mv, then ts
    k = 0
    for i, r in enumerate(reads):
        got = M.moves_of_aux(r['aux'])
        if (r['parts'][0] != (0, r['l_seq']) and got[1] is not None and M.usable(*got, r['l_seq'], r['parts'])):
            tags = [t for t, _, _ in M.walk_aux(back.aux(k))]
            assert tags == [b'RG', b'ns', b'qs', b'mv', b'ts'], tags
            old = dict((t, raw) for t, _, raw in M.walk_aux(r['aux']))
            new = dict((t, raw) for t, _, raw in M.walk_aux(back.aux(k)))
            assert new[b'ns'] == old[b'ns'] and new[b'ts'][2:3] == b'i'
            break
        k += len(r['parts'])
    else:
        raise AssertionError('no such read')
    # and with the option off: mv dropped, ts verbatim
    out, counts = write_case(tmp_path, reads, None, False, 'off.bam')
    assert check_written(misc.load_batch(out, keep_aux=True), reads, False) == 0 and counts == (0, 0)


def test_unusable_reads_keep_ts_verbatim(tmp_path):
    from custom_porechop_abi_amd import misc
    moves = SHORT_MOVES
    good = {'l_seq': 6, 'seq': 'ACGTAC', 'aux': ts_aux(9, 'C') + mv_aux(5, moves), 'parts': [(1, 4)]}
    bad = {'l_seq': 6, 'seq': 'ACGTAC', 'aux': ts_aux(9, 'C') + mv_aux(5, moves + [1]), 'parts': [(1, 4)]}
    whole = dict(good, parts=[(0, 6)])
    reads = [good, bad, whole, dict(whole, reverse=True), good]
    out, counts = write_case(tmp_path, reads, None, True, 'out.bam')
    back = misc.load_batch(out, keep_aux=True)
    check_written(back, reads, True)
    assert counts == (3, 1)
    new = b'mvBc' + struct.pack('<I', 8) + b'\x05' + bytes([1, 1, 0, 0, 1, 1, 0]) + b'tsi' + struct.pack('<i', 9 + 15)
    assert back.aux(0) == b'qsC\x00' + new
    assert back.aux(1) == ts_aux(9, 'C') + b'qsC\x01'
    assert back.aux(2) == whole['aux'] + b'qsC\x02'                     # byte-identical to the input
    assert back.aux(3) == b'qsC\x03' + mv_aux(5, moves) + ts_aux(9, 'i')  # reverse-strand: remapped, nothing reversed


def _write_direct(batch, path, reads, keep_aux, tag_flags, new_entry):
    from custom_porechop_abi_amd import misc
    L = misc._declare(misc.lib())
    st = np.ascontiguousarray([r['parts'][0][0] for r in reads], np.int32)
    et = np.ascontiguousarray([r['l_seq'] - (r['parts'][-1][0] + r['parts'][-1][1]) for r in reads], np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    head = (batch._h, os.fsencode(path), 0, p(st), p(et), None, None, 1, 0, 0, None, None, 0, keep_aux)
    rc = L.pcabi_reads_write_bam_tags(*head, tag_flags, -1) if new_entry else L.pcabi_reads_write_bam(*head, -1)
    assert rc == len(reads)


@pytest.mark.parametrize('keep_aux', [0, 1, 2])
def test_tag_flags_0_writes_the_old_file(tmp_path, keep_aux):
    from custom_porechop_abi_amd import misc
    reads = [dict(r, parts=[(r['parts'][0][0], r['parts'][-1][0] + r['parts'][-1][1] - r['parts'][0][0])])
             for r in writer_reads(40, with_mods=True)]
    write_case(tmp_path, reads, None, False, 'unused.bam')   # leaves in.bam
    batch = misc.load_batch(str(tmp_path / 'in.bam'), keep_aux=True)
    _write_direct(batch, str(tmp_path / 'old.bam'), reads, keep_aux, 0, False)
    _write_direct(batch, str(tmp_path / 'new.bam'), reads, keep_aux, 0, True)
    with open(str(tmp_path / 'old.bam'), 'rb') as f, open(str(tmp_path / 'new.bam'), 'rb') as g:
        old = f.read()
        assert old == g.read() and len(old) > 1000
    if keep_aux:
        _write_direct(batch, str(tmp_path / 'moves.bam'), reads, keep_aux, 1, True)
        with open(str(tmp_path / 'moves.bam'), 'rb') as f:
            assert f.read() != old
    L = misc._declare(misc.lib())
    assert L.pcabi_reads_write_bam_tags(batch._h, os.fsencode(str(tmp_path / 'x.bam')), 0, None, None, None, None, 1, 0, 0, None, None,
                                        0, 1, 2, -1) < 0   # an unknown flag


def test_keep_mods_and_keep_moves_together(tmp_path):
    from custom_porechop_abi_amd import engine, misc
    reads = writer_reads(60, with_mods=True)
    engine.mods_counts(reset=True)
    out, counts = write_case(tmp_path, reads, None, True, 'both.bam', keep_mods=True)
    mods_counts = engine.mods_counts(reset=True)
    back = misc.load_batch(out, keep_aux=True)
    assert check_written(back, reads, True, True) > len(reads) // 2
    assert counts == changed_counts(reads) and mods_counts[0] > 10 and mods_counts[1] == 0
    both = 0
    for k in range(back.n):
        tags = [t for t, _, _ in M.walk_aux(back.aux(k))]
        if b'MM' in tags and b'mv' in tags and tags[0] != b'MM':   # (MM first: a read written verbatim)
            both += 1
            rest = tags[tags.index(b'MM'):]
            assert rest in ([b'MM', b'ML', b'MN', b'mv', b'ts'], [b'MM', b'ML', b'MN', b'mv']), tags
    assert both > 10
    # keep_mods alone still drops mv, keep_moves alone still drops MM
    out, _ = write_case(tmp_path, reads, None, False, 'mods.bam', keep_mods=True)
    assert check_written(misc.load_batch(out, keep_aux=True), reads, False, True) == 0


def test_keep_moves_needs_the_tags(tmp_path):
    from custom_porechop_abi_amd import misc
    from custom_porechop_abi_amd.pipeline import FileTrimmer
    reads = writer_reads(5)
    write_case(tmp_path, reads, None, False, 'unused.bam')
    batch = misc.load_batch(str(tmp_path / 'in.bam'), keep_aux=True)
    with pytest.raises(ValueError):
        misc.write_reads(batch, str(tmp_path / 'x.bam'), 'bam', keep_moves=True)
    with pytest.raises(ValueError):
        misc.write_reads(batch, str(tmp_path / 'x.fastq'), 'fastq', keep_aux=True, keep_moves=True)
    with pytest.raises(ValueError):
        FileTrimmer([], keep_moves=True)


# ---- 5. the shared header alone, under sanitizers -------------------------------------------------------
def test_moves_layer_under_sanitizers(tmp_path):
    """tests/moves_fuzz_main.cpp (csrc/pcabi_moves.h alone), built with -fsanitize=address,undefined as a
    program of its own and run as a child process: tables at every alignment in blocks of exactly their
    size, the 64 lanes of count, select and copy played against the byte-by-byte walk."""
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path / 'moves_fuzz')
    base = ['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
            os.path.join(HERE, 'moves_fuzz_main.cpp')]
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
