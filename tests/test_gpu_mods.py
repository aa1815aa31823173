"""Base-modification tags remapped on the GPU: k_mods_plan / k_mods_write (engine.mods_plan / mods_remap
with device=0) against the host build of the same code and tests/mods_ref.py's restatement, the BAM
writer's device path with keep_mods against its host path, and FileTrimmer BAM to BAM with keep_mods."""
import os
import struct

import numpy as np
import pytest

from tests import bam_lib as B
from tests import golden_lib
from tests import mods_ref as R
from tests import test_mods_cpu as C

pytestmark = pytest.mark.gpu

DATA = os.path.join(golden_lib.GOLDEN, 'data')


# ---- the shapes at which the kernels can go wrong --------------------------------------------------------
def tags_of(seq, groups, ml=True, mn=True):
    """groups: [(header str, base, n_codes, [ordinals], [count widths or None])] -> aux bytes."""
    mm, vals = b'', b''
    for g, (header, base, n_codes, ords, widths) in enumerate(groups):
        mm += header.encode()
        last = -1
        for k, o in enumerate(ords):
            mm += b',' + (b'%0*d' % (widths[k], o - last - 1) if widths else b'%d' % (o - last - 1))
            last = o
            vals += bytes([(17 * g + 3 * k + c) % 256 for c in range(n_codes)])
        mm += b';'
    out = b'MMZ' + mm + b'\0'
    if ml:
        out += b'MLBC' + struct.pack('<I', len(vals)) + vals
    if mn:
        out += b'MNi' + struct.pack('<i', len(seq))
    return out


def straddling_counts(rng, header, n_entries):
    """Ordinals and count widths (1..7 digits, zero-padded) for a group that starts the MM text, chosen so
    that a number lies across every multiple of 64 (hence of 256) of the text; and the multiples covered."""
    at, ords, widths, covered, o = len(header), [], [], [], -1
    for _ in range(n_entries):
        at += 1                               # the ','
        edge = (at // 64 + 1) * 64            # the next multiple of 64 behind the number's first digit
        gap = edge - at
        w = int(rng.randint(gap + 1, 8)) if 1 <= gap <= 6 else 1 + len(widths) % 3
        if at < edge < at + w:
            covered.append(edge)
        o += 1 + int(rng.randint(0, 10 if w == 1 else 60))
        ords.append(o)
        widths.append(w)
        at += w
    return ords, widths, covered


def shape_reads():
    rng = np.random.RandomState(5)
    reads = []
    for ln in (0, 1, 63, 64, 65, 16383, 16384, 16385, 32769):
        seq = ''.join(rng.choice(list('ACGT'), ln))
        occ_c, occ_n = R.occurrences(seq, 'C'), list(range(ln))
        every = occ_c and list(range(0, len(occ_c), max(1, len(occ_c) // 40)))
        groups = [('C+mh?', 'C', 2, list(every) if every else [], None),
                  ('N-n', 'N', 1, [ln - 1] if ln else [], None),          # the read's last base
                  ('A+a.', 'A', 1, [0] if 'A' in seq else [], None)]       # its first A
        # boundaries on a modified base, one before it and one behind it; a part that keeps nothing
        mods = sorted({occ_c[o] for o in groups[0][3]} | ({ln - 1} if ln else set()))
        parts = [(0, ln)]
        for p in mods[:3] + mods[-2:]:
            parts += [(p, min(5, ln - p)), (max(p - 1, 0), 1 + (p > 0)), (min(p + 1, ln), 0), (0, p), (0, p + 1)]
        reads.append({'seq': seq, 'aux': tags_of(seq, groups), 'parts': parts})
    # groups of 0, 1, 63, 64, 65 and 1000 entries, each also behind a group of another size
    seq = ''.join(rng.choice(list('ACGT'), 5000))
    occ_g = R.occurrences(seq, 'G')
    for n in (0, 1, 63, 64, 65, 1000):
        step = max(1, len(occ_g) // max(n, 1))
        ords = list(range(0, n * step, step))[:n]
        assert len(ords) == n and (not ords or ords[-1] < len(occ_g))
        groups = [('G+m', 'G', 1, ords, None), ('T-76792.', 'T', 1, [2, 3, 700], None), ('G+o?', 'G', 1, ords[::2], None)]
        cuts = [0, 700, 701, 1800, 2900, 2901, 4100, 5000]             # seven parts, some of one base
        reads.append({'seq': seq, 'aux': tags_of(seq, groups, ml=n != 64), 'parts': [(a, b - a) for a, b in zip(cuts, cuts[1:])]})
    # numbers of 1..7 digits across every multiple of 64 and 256 bytes of the text
    seq = ''.join(rng.choice(list('ACGT'), 16385))
    ords, widths, covered = straddling_counts(rng, 'N+n', 420)
    assert ords[-1] < len(seq) and covered == list(range(64, 64 * (len(covered) + 1), 64)) and covered[-1] >= 1024
    assert set(widths) == {1, 2, 3, 4, 5, 6, 7}
    reads.append({'seq': seq, 'aux': tags_of(seq, [('N+n', 'N', 1, ords, widths), ('C+m', 'C', 1, [0, 5, 6, 4000], None)]),
                  'parts': [(0, 16385), (ords[10], ords[300] - ords[10]), (ords[10] + 1, 7), (ords[419], 1), (ords[419] + 1, 3), (0, ords[0])]})
    # one unusable read between usable ones; most reads of the batch without any tag
    reads.insert(4, {'seq': C.SHORT, 'aux': b'MMZC+m,1,0,2;\0', 'parts': [(0, 12), (3, 4)]})
    plain = [{'seq': ''.join(rng.choice(list('ACGT'), int(rng.randint(1, 300)))), 'aux': b'', 'parts': [(0, 1)]} for _ in range(60)]
    return [x for k, r in enumerate(reads) for x in ([r] + plain[3 * k:3 * k + 3])] + plain[3 * len(reads):]


_shapes = None


def shapes():
    global _shapes
    if _shapes is None:
        _shapes = shape_reads()
    return _shapes


# ---- 1. the table-level API ----------------------------------------------------------------------------
def test_kernels_match_host_and_restatement(gpu_lib):
    from custom_porechop_abi_amd import engine
    reads = shapes() + C.shared_corpus()[:80]
    assert len(reads) <= 300 and sum(r['aux'] == b'' for r in shapes()) > len(shapes()) // 2
    engine.mods_counts(reset=True)
    dev, usable_d = C.run_tables(reads, 0)
    counts = engine.mods_counts(reset=True)
    host, usable_h = C.run_tables(reads, -1)
    assert np.array_equal(usable_d, usable_h)
    good = int(usable_h.sum())
    assert counts == (good, len(reads) - good) and 0 < good < len(reads)
    bad = [k for k, (a, b) in enumerate(zip(dev, host)) if a != b]
    assert not bad, (bad[:8], dev[bad[0]][:60], host[bad[0]][:60])
    C.check_against_ref(reads, dev, usable_d)
    # the shapes do what they are there for
    kept = [len(t) > 0 for t in dev]
    assert any(kept) and not all(kept)


def test_shapes_cover_the_edges():
    """(no GPU work: what shape_reads() promises, from the restatement)"""
    reads = [r for r in shapes() if r['aux']]
    assert sorted({len(r['seq']) for r in reads} & {0, 1, 63, 64, 65, 16383, 16384, 16385, 32769}) == [0, 1, 63, 64, 65, 16383, 16384,
                                                                                                          16385, 32769]
    sizes, five, nothing = set(), 0, 0
    for r in reads:
        mm = R.mods_of_aux(r['aux'])[0]
        sizes |= {len(g[4]) for g in R.parse_mm(mm)}
        five += len(r['parts']) >= 5
        full = R.decode_aux(r['seq'], r['aux'])
        nothing += bool(full) and any(not R.slice_records(full, s0, ns) for s0, ns in r['parts'])
    assert {0, 1, 63, 64, 65, 1000} <= sizes and five >= 5 and nothing >= 5


# ---- 2. the writer ---------------------------------------------------------------------------------------
def test_writer_on_device_matches_host_path(gpu_lib, tmp_path):
    from custom_porechop_abi_amd import misc
    from tests.test_gpu_bam_pack import _finished_stream
    reads = C.writer_reads()
    big = [dict(r, reverse=k % 2 == 1) for k, r in enumerate(shapes()) if r['aux'] and 60 < len(r['seq'])][:8]
    for r in big:   # the writer takes ascending parts that do not touch
        r['parts'] = [(len(r['seq']) // 7, len(r['seq']) // 3), (len(r['seq']) // 2 + 1, len(r['seq']) // 4)]
    reads = reads[:60] + big + C.unusable_reads()   # every usability failure, inside RG .. qs, between usable reads
    dev, recs, counts_d = C.write_case(tmp_path, reads, 0, True, 'dev.bam')
    host, _, counts_h = C.write_case(tmp_path, reads, None, True, 'host.bam')
    assert counts_d == counts_h and counts_d[0] > 0 and counts_d[1] >= 2 * len(C.UNUSABLE)
    assert _finished_stream(dev) == _finished_stream(host)
    back = misc.load_batch(dev, gunzip_device=0, keep_aux=True)
    assert C.check_written(back, reads, recs, True) > len(reads) // 2
    # with the option off the device path writes what the host path writes, without the tags
    dev, recs, counts = C.write_case(tmp_path, reads, 0, False, 'dev_off.bam')
    host, _, _ = C.write_case(tmp_path, reads, None, False, 'host_off.bam')
    assert counts == (0, 0) and _finished_stream(dev) == _finished_stream(host)
    C.check_written(misc.load_batch(dev, gunzip_device=0, keep_aux=True), reads, recs, False)


# ---- 3. FileTrimmer --------------------------------------------------------------------------------------
def _golden_mods_bam(tmp_path, fq_name):
    """The golden reads as a BAM whose records carry RG, MM / ML / MN made for each read (three groups, a
    twentieth of their bases' occurrences marked) and qs; every fourth record is stored reverse-complemented."""
    from custom_porechop_abi_amd import misc
    fq = misc.load_batch(os.path.join(DATA, fq_name))
    rng = np.random.RandomState(9)
    recs, reads = [], {}
    for i in range(fq.n):
        orig = fq.sequence(i)
        seq, qual, flag = orig, [ord(c) - 33 for c in fq.quals(i)], 4
        assert set(orig) <= set(B.LETTERS)
        if i % 4 == 1:
            seq, qual, flag = ''.join(B.COMPLEMENT[c] for c in reversed(seq)), qual[::-1], 4 | 0x10
        hs = [C.HEADERS[j] for j in rng.choice(len(C.HEADERS), 3, replace=False)]
        mods = C.make_tags(rng, orig, hs, 0.05, with_ml=i % 5 != 0, with_mn=[None, 'i'][i % 2], old=i % 7 == 3)
        name = fq.name(i).split()[0].encode()
        recs.append({'name': name, 'seq': seq, 'qual': qual, 'flag': flag,
                     'aux': b'RGZgrp\0' + mods + b'qsC' + bytes([i % 200])})
        reads[name] = (orig, recs[-1]['aux'], bool(flag & 0x10))
    header = b'@HD\tVN:1.6\tSO:unknown\n@RG\tID:grp\n'
    path = str(tmp_path / 'in.bam')
    with open(path, 'wb') as f:
        f.write(B.make_bam(recs, header, (), 5000))
    return path, reads


def test_file_trimmer_keep_mods(gpu_lib, tmp_path):
    from custom_porechop_abi_amd import engine, misc
    from tests.test_gpu_bam_pack import _finished_stream, _trimmer
    case = [c for c in golden_lib.g2()['cases'] if c['case'] == 'one_adapter_set'][0]
    src, reads = _golden_mods_bam(tmp_path, 'test_one_adapter_set.fastq.gz')
    outs = {}
    for name, kw in (('mods', {'keep_mods': True}), ('off', {'keep_mods': False}), ('today', {})):
        ft = _trimmer(case, filter_reads=False, gzip_on_device=True, gunzip_on_device=True, keep_tags=True, **kw)
        engine.mods_counts(reset=True)
        try:
            ft.trim_file(src, str(tmp_path / (name + '.bam')), 'bam', max_reads=7)
        finally:
            ft.close()
        outs[name] = (str(tmp_path / (name + '.bam')), engine.mods_counts(reset=True))
    # keep_mods=False is the default of this build, no more: that the default still writes the bytes it wrote
    # before the option existed rests on the writer tests that were there before (test_gpu_bam_pack.py,
    # test_bam_pack_cpu.py), which assert the drop byte for byte
    assert _finished_stream(outs['off'][0]) == _finished_stream(outs['today'][0]) and outs['off'][1] == (0, 0)
    assert outs['mods'][1][0] > 0 and outs['mods'][1][1] == 0
    changed_with_mods = 0
    for name, keep_mods in (('mods', True), ('off', False)):
        back = misc.load_batch(outs[name][0], gunzip_device=0, keep_aux=True)
        assert back.n > 7
        for k in range(back.n):
            nm = back.names[back.name_off[k]:back.name_off[k + 1]].tobytes()
            orig, aux, rev = reads.get(nm) or reads[nm.rsplit(b'_', 1)[0]]
            part = back.seq[back.seq_off[k]:back.seq_off[k + 1]].tobytes().decode()
            s0 = orig.find(part)
            assert s0 >= 0 and orig.find(part, s0 + 1) < 0
            whole = nm in reads and len(part) == len(orig)
            assert back.aux(k) == R.part_aux(orig, aux, s0, len(part), whole and not rev, keep_mods), (name, nm)
            if keep_mods:   # the semantic check, against the input record's decoded modifications
                want = R.slice_records(R.decode_aux(orig, aux), s0, len(part))
                assert R.decode_aux(part, back.aux(k)) == want, nm
                changed_with_mods += bool(want) and not (whole and not rev)
    assert changed_with_mods > 0
