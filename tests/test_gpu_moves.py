"""Move tables remapped on the GPU: k_moves_count / the scan / k_moves_select / k_moves_size / k_moves_write
(engine.moves_plan / moves_remap with device=0) against the host build of the same code and
tests/moves_ref.py's restatement, the BAM writer's device path with keep_moves against its host path, and
FileTrimmer BAM to BAM with keep_moves."""
import os
import signal
import struct

import numpy as np
import pytest

from tests import bam_lib as B
from tests import golden_lib
from tests import moves_ref as M
from tests import test_moves_cpu as C

pytestmark = pytest.mark.gpu

DATA = os.path.join(golden_lib.GOLDEN, 'data')
COUNTS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8193, 65537)
SEG = 4096


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


# ---- the shapes at which the kernels can go wrong --------------------------------------------------------
def read_of(moves, parts, stride=5, ts=1000, sub=b'c', tail=b'nsi\x07\0\0\0'):
    aux = b'RGZgrp\0' + (C.ts_aux(ts, 'i') if ts is not None else b'') + C.mv_aux(stride, moves, sub) + tail
    return {'l_seq': int(sum(m == 1 for m in moves)), 'aux': aux, 'parts': parts}


def edge_parts(l_seq):
    """(0, 0), (l_seq, 0), (0, l_seq), single-base parts at both ends, a part in the middle."""
    ps = [(0, 0), (l_seq, 0), (0, l_seq)]
    if l_seq >= 1:
        ps += [(0, 1), (l_seq - 1, 1), (l_seq // 2, l_seq - l_seq // 2), (l_seq // 3, l_seq // 3)]
    return ps


def shape_reads():
    rng = np.random.RandomState(5)
    reads = []
    for n in COUNTS:   # n moves, about every second one a base
        moves = (rng.rand(n) < 0.5).astype(np.uint8).tolist()
        reads.append(read_of(moves, edge_parts(sum(moves)), sub=b'C' if n % 2 else b'c', ts=None if n % 3 == 0 else 1000 + n))
    # every move a base (p(k) = k): boundaries on the first and the last byte of a lane's 16 bytes (all 16
    # residues, whatever the tag's alignment), of a 64-byte pass and of a segment
    ks = list(range(4088, 4105)) + [63, 64, 127, 128, 4095, 4096, 8191, 8192, 8299]
    reads.append(read_of([1] * 8300, [(k, 1) for k in ks] + [(0, 8300)]))
    # the same edges with dwells between the bases: ones at 4095 and 4096, at 8191 and 8192 and nowhere near
    moves = [0] * 9000
    for at in (5, 4095, 4096, 8191, 8192, 8999):
        moves[at] = 1
    reads.append(read_of(moves, [(k, 1) for k in range(6)] + [(1, 4), (0, 6)]))
    # one dwell of more than 8192 blocks (12500: at least two whole segments without a base, which select
    # steps over)
    moves = C.make_moves(rng, 50, 2.0) + [0] * 12500 + C.make_moves(rng, 70, 2.0)
    reads.append(read_of(moves, [(49, 1), (50, 1), (49, 2), (0, 50), (50, 70), (0, 120), (51, 0)]))
    # leading zeros, short and longer than a segment
    for lead in (100, 5000):
        reads.append(read_of(C.make_moves(rng, 300, 2.0, lead=lead), [(0, 0), (0, 1), (1, 299), (0, 300), (1, 0)]))
    # no bases at all: moves of zeros only
    reads.append(read_of([0] * 77, [(0, 0)]))
    # seven parts on one read
    cuts = [0, 700, 701, 1800, 2900, 2901, 4100, 5000]
    reads.append(read_of(C.make_moves(rng, 5000, 2.2), [(a, b - a) for a, b in zip(cuts, cuts[1:])]))
    # unusable between usable: an invalid byte only in the last segment, one base short, and the chain's kinds
    moves = C.make_moves(rng, 5000, 2.0)
    assert len(moves) > 2 * SEG + 10
    bad_last = read_of(moves[:-1] + [2], [(10, 100), (4000, 900)])
    bad_last['l_seq'] = 5000
    short = read_of(moves, [(10, 100)])
    short['l_seq'] = 5001
    reads[3:3] = [bad_last]
    reads[9:9] = [short]
    for k, (_, make) in enumerate(C.UNUSABLE):
        m = C.make_moves(rng, 40, 2.0)
        reads.insert(2 * k + 1, {'l_seq': 40, 'aux': b'RGZgrp\0' + make(40, 5, m) + b'nsi\x07\0\0\0', 'parts': [(3, 20), (30, 5)]})
    # more than half of the batch without an mv tag
    plain = [{'l_seq': int(rng.randint(1, 300)), 'aux': b'RGZgrp\0', 'parts': [(0, 1)]} for _ in range(len(reads) + 5)]
    out = [x for k, r in enumerate(reads) for x in (r, plain[k])] + plain[len(reads):]
    out.append(read_of(C.make_moves(rng, 200, 2.0), [(3, 100)], tail=b''))   # its tag flush against the blob's end
    return out


def shape_pads(reads):
    """Padding before each read's chain such that the tables' first values take all 16 alignments in turn."""
    pads, at, k = [], 0, 0
    for r in reads:
        if M.moves_of_aux(r['aux']) is None:
            continue
        mv_at = [sum(len(raw) for _, _, raw in M.walk_aux(r['aux'])[:j]) for j, (t, _, _) in enumerate(M.walk_aux(r['aux'])) if t == b'mv'][0]
        pad = (k % 16 - (at + mv_at + 8)) % 16
        pads.append(pad)
        at += pad + len(r['aux'])
        k += 1
    return pads


_shapes = None


def shapes():
    global _shapes
    if _shapes is None:
        reads = shape_reads()
        _shapes = (reads, shape_pads(reads))
    return _shapes


# ---- 1. the table-level API ----------------------------------------------------------------------------
def test_kernels_match_host_and_restatement(gpu_lib):
    from custom_porechop_abi_amd import engine
    reads, pads = shapes()
    engine.moves_counts(reset=True)
    dev, usable_d = C.run_tables(reads, 0, pads=pads)
    counts = engine.moves_counts(reset=True)
    host, usable_h = C.run_tables(reads, -1, pads=pads)
    assert np.array_equal(usable_d, usable_h)
    good = int(usable_h.sum())
    assert counts == (good, usable_h.size - good) and 0 < good < usable_h.size
    bad = [k for k, (a, b) in enumerate(zip(dev, host)) if a != b]
    assert not bad, (bad[:8], dev[bad[0]][:60], host[bad[0]][:60])
    C.check_against_ref(reads, dev, usable_d)


def test_corpus_on_device(gpu_lib):
    reads = C.shared_corpus()
    dev, usable = C.run_tables(reads, 0)
    C.check_against_ref(reads, dev, usable)


def test_refused_tables_launch_nothing(gpu_lib):
    """Out-of-range tables are refused on the host (PCABI_E_ARG) before anything is launched."""
    from custom_porechop_abi_amd import engine
    reads = [{'l_seq': 6, 'aux': C.ts_aux(7, 'C') + C.mv_aux(5, C.SHORT_MOVES), 'parts': [(1, 4), (0, 3)]}]
    tags, rd, pt = C.tables(reads)
    for field, value in (('mv_off', tags.size), ('n_vals', tags.size), ('n_parts', 3)):
        bad = rd.copy()
        bad[field][0] = value
        with pytest.raises(Exception, match='does not fit|does not lie|belongs to no read'):
            engine.moves_plan(tags, bad, pt.copy(), device=0)
    bad = pt.copy()
    bad['ns'][1] = 7
    with pytest.raises(Exception, match='does not lie'):
        engine.moves_plan(tags, rd, bad, device=0)
    pt, _ = engine.moves_plan(tags, rd, pt, device=0)
    pt['out'] = [0, 1]
    with pytest.raises(Exception, match='overlap'):
        engine.moves_remap(tags, rd, pt, np.zeros(64, np.uint8), device=0)


def test_shapes_cover_the_edges():
    """(no GPU work: what shape_reads() promises, from the restatement)"""
    reads, pads = shapes()
    tags, rd, pt = C.tables(reads, pads)
    with_mv = [r for r in reads if M.moves_of_aux(r['aux']) is not None]
    assert len(with_mv) * 2 < len(reads)
    assert {int(v) - 1 for v in rd['n_vals']} >= set(COUNTS)
    assert {int(o) % 16 for o, f in zip(rd['mv_off'], rd['flags']) if not f} == set(range(16))
    assert int(rd['mv_off'][-1]) + int(rd['n_vals'][-1]) == tags.size           # flush against the end
    in16, in64, inseg, empty_segs, lead, seven, bad_kinds = set(), set(), set(), 0, 0, 0, set()
    part_kinds = set()
    for i, r in enumerate(with_mv):
        vals, ts, bad = M.moves_of_aux(r['aux'])
        ok = M.usable(vals, ts, bad, r['l_seq'], r['parts'])
        if not ok:
            if not bad and vals and sum(v == 1 for v in vals[1:]) == r['l_seq'] - 1:
                bad_kinds.add('short')
            if not bad and len(vals) > 2 * SEG and all(v in (0, 1) for v in vals[1:-SEG]) and vals[-1] == 2:
                bad_kinds.add('last segment')
            bad_kinds.add('chain' if bad else 'values')
            continue
        moves = vals[1:]
        seven += len(r['parts']) == 7
        lead += bool(moves) and moves[0] == 0 and r['l_seq'] > 0
        segs = [sum(moves[a:a + SEG]) for a in range(0, len(moves), SEG)]
        for s0, ns in r['parts']:
            part_kinds |= {'0,0'} if (s0, ns) == (0, 0) else set()
            part_kinds |= {'l,0'} if (s0, ns) == (r['l_seq'], 0) else set()
            part_kinds |= {'0,l'} if (s0, ns) == (0, r['l_seq']) else set()
            part_kinds |= {'first'} if (s0, ns) == (0, 1) else set()
            part_kinds |= {'last'} if ns == 1 and s0 == r['l_seq'] - 1 else set()
            part_kinds |= {'no bases'} if r['l_seq'] == 0 else set()
            for q in M.slice_of(moves, s0, ns):
                if q < len(moves) and moves[q] == 1:
                    in16.add((int(rd['mv_off'][i]) + 1 + q) % 16)
                    in64.add(q % SEG % 64)
                    inseg.add(q % SEG)
                    empty_segs += any(c == 0 for c in segs[:q // SEG]) and segs[q // SEG] > 0
    assert {0, 15} <= in16 and {0, 63} <= in64 and {0, SEG - 1} <= inseg
    assert empty_segs >= 2 and lead >= 2 and seven >= 2
    assert part_kinds == {'0,0', 'l,0', '0,l', 'first', 'last', 'no bases'}
    assert bad_kinds == {'short', 'last segment', 'chain', 'values'}


# ---- 2. the writer ---------------------------------------------------------------------------------------
def writer_reads():
    """The CPU tests' writer reads (reverse-strand records, split pieces, every unusable kind) and a few of
    the long shapes, cut in two pieces each."""
    rng = np.random.RandomState(8)
    reads = C.writer_reads(70)
    big = [dict(r) for r in shapes()[0] if M.moves_of_aux(r['aux']) is not None and r['l_seq'] > 2000][:6]
    for k, r in enumerate(big):
        n = r['l_seq']
        r.update(seq=''.join(rng.choice(list('ACGT'), n)), reverse=k % 2 == 1, parts=[(n // 7, n // 3), (n // 2 + 1, n // 4)])
    plain = [{'l_seq': 50, 'seq': ''.join(rng.choice(list('ACGT'), 50)), 'aux': b'RGZgrp\0', 'parts': [(5, 40)]} for _ in range(10)]
    return reads + big + plain


def test_writer_on_device_matches_host_path(gpu_lib, tmp_path):
    from custom_porechop_abi_amd import misc
    from tests.test_gpu_bam_pack import _finished_stream
    reads = writer_reads()
    dev, counts_d = C.write_case(tmp_path, reads, 0, True, 'dev.bam')
    host, counts_h = C.write_case(tmp_path, reads, None, True, 'host.bam')
    assert counts_d == counts_h == C.changed_counts(reads) and counts_d[0] > 0 and counts_d[1] >= len(C.UNUSABLE)
    assert _finished_stream(dev) == _finished_stream(host)
    back = misc.load_batch(dev, gunzip_device=0, keep_aux=True)
    assert C.check_written(back, reads, True) > len(reads) // 2
    assert any(r.get('reverse') and len(r['parts']) > 1 for r in reads)
    # with the option off the device path writes what the host path writes, without mv
    dev, counts = C.write_case(tmp_path, reads, 0, False, 'dev_off.bam')
    host, _ = C.write_case(tmp_path, reads, None, False, 'host_off.bam')
    assert counts == (0, 0) and _finished_stream(dev) == _finished_stream(host)
    assert C.check_written(misc.load_batch(dev, gunzip_device=0, keep_aux=True), reads, False) == 0


def test_writer_with_mods_and_moves_on_device(gpu_lib, tmp_path):
    """Both tag sets sized in one round trip: the device path's stream is the host path's."""
    from custom_porechop_abi_amd import misc
    from tests.test_gpu_bam_pack import _finished_stream
    reads = C.writer_reads(60, with_mods=True)
    dev, counts_d = C.write_case(tmp_path, reads, 0, True, 'dev.bam', keep_mods=True)
    host, counts_h = C.write_case(tmp_path, reads, None, True, 'host.bam', keep_mods=True)
    assert counts_d == counts_h and _finished_stream(dev) == _finished_stream(host)
    assert C.check_written(misc.load_batch(dev, gunzip_device=0, keep_aux=True), reads, True, True) > len(reads) // 2


# ---- 3. FileTrimmer --------------------------------------------------------------------------------------
def _golden_moves_bam(tmp_path, fq_name):
    """The golden reads as a BAM whose records carry RG, ts, a move table made for each read, ns and qs;
    every fourth record is stored reverse-complemented."""
    from custom_porechop_abi_amd import misc
    fq = misc.load_batch(os.path.join(DATA, fq_name))
    rng = np.random.RandomState(9)
    recs, reads = [], {}
    for i in range(fq.n):
        orig = fq.sequence(i)
        seq, qual, flag = orig, [ord(c) - 33 for c in fq.quals(i)], 4
        if i % 4 == 1:
            seq, qual, flag = ''.join(B.COMPLEMENT[c] for c in reversed(seq)), qual[::-1], 4 | 0x10
        moves = C.make_moves(rng, len(orig), 2.0, lead=int(rng.randint(0, 30)))
        name = fq.name(i).split()[0].encode()
        aux = b'RGZgrp\0' + C.ts_aux(10 + i, 'i') + C.mv_aux(5 + i % 2, moves) + b'nsi' + struct.pack('<i', 99999) + b'qsC' + bytes([i % 200])
        recs.append({'name': name, 'seq': seq, 'qual': qual, 'flag': flag, 'aux': aux})
        reads[name] = (orig, aux, bool(flag & 0x10), moves, 5 + i % 2, 10 + i)
    path = str(tmp_path / 'in.bam')
    with open(path, 'wb') as f:
        f.write(B.make_bam(recs, b'@HD\tVN:1.6\tSO:unknown\n@RG\tID:grp\n', (), 5000))
    return path, reads


def test_file_trimmer_keep_moves(gpu_lib, tmp_path):
    from custom_porechop_abi_amd import engine, misc
    from tests.test_gpu_bam_pack import _trimmer
    case = [c for c in golden_lib.g2()['cases'] if c['case'] == 'one_adapter_set'][0]
    src, reads = _golden_moves_bam(tmp_path, 'test_one_adapter_set.fastq.gz')
    ft = _trimmer(case, filter_reads=False, gzip_on_device=True, gunzip_on_device=True, keep_tags=True, keep_moves=True)
    engine.moves_counts(reset=True)
    try:
        ft.trim_file(src, str(tmp_path / 'out.bam'), 'bam', max_reads=7)
    finally:
        ft.close()
    counts = engine.moves_counts(reset=True)
    assert counts[0] > 0 and counts[1] == 0
    back = misc.load_batch(str(tmp_path / 'out.bam'), gunzip_device=0, keep_aux=True)
    assert back.n > 7
    moved = 0
    for k in range(back.n):
        nm = back.names[back.name_off[k]:back.name_off[k + 1]].tobytes()
        orig, aux, rev, moves, stride, ts = reads.get(nm) or reads[nm.rsplit(b'_', 1)[0]]
        part = back.seq[back.seq_off[k]:back.seq_off[k + 1]].tobytes().decode()
        s0 = orig.find(part)
        assert s0 >= 0 and orig.find(part, s0 + 1) < 0
        whole = nm in reads and len(part) == len(orig)
        assert back.aux(k) == M.part_aux(aux, len(orig), [(s0, len(part))], 0, whole and not rev), nm
        new = dict((t, raw) for t, _, raw in M.walk_aux(back.aux(k)))
        assert sum(new[b'mv'][9:]) == len(part) and new[b'mv'][8] == stride
        got_ts = struct.unpack_from(M.INT_FMT[chr(new[b'ts'][2])], new[b'ts'], 3)[0]
        q0 = M.slice_of(moves, s0, len(part))[0]
        assert got_ts - ts == stride * q0
        moved += s0 > 0 and q0 > 0
    assert moved > 0
