"""The piece stage on the GPU: k_piece_keys / the sort / k_piece_count / k_piece_spans / k_piece_cuts around the
quality kernels (engine.quality_filter_pieces with device=0), byte for byte against the host build and so
against tests/qual_pieces_ref.py's restatement; and FileTrimmer(quality_per_piece=True) end to end against
output built from the decisions of a run with the option off plus the restatement. (The pipeline has no
CPU path -- FileTrimmer opens the device -- so the end-to-end tests live here.)"""
import gzip
import os
import signal

import numpy as np
import pytest

from tests import golden_lib
from tests import qual_pieces_ref as P
from tests import qual_ref as R
from tests import test_qual_pieces_cpu as C

pytestmark = pytest.mark.gpu


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


# ---- the table-level API -------------------------------------------------------------------------------
def _same(a, b):
    return all(x.tobytes() == y.tobytes() and x.dtype == y.dtype for x, y in zip(a, b))


def _device_is_host(o, *arrays):
    dev, host = C.run(o, *arrays, 0), C.run(o, *arrays, -1)
    assert _same(dev, host)
    return dev


@pytest.mark.parametrize('k', range(len(P.option_sets())))
def test_fuzz_on_device(gpu_lib, k):
    """(the host build equals the restatement on the same inputs: tests/test_qual_pieces_cpu.py)"""
    pieces = _device_is_host(P.option_sets()[k], *P.fuzz_batch())[2]
    assert pieces.size > 3000


def test_crafted_reads_on_device(gpu_lib):
    for case in P.crafted_cases():
        C.check_case(*case, 0)
        _device_is_host(*case[1:])
    for case in P.equality_cases():
        pieces = C.check_case(*case[:-1], 0)[0]
        assert [(p[3][3] & R.FAIL) == 0 for p in pieces] == case[-1], case[0]
    # an empty batch
    none = np.zeros(0, np.int64)
    cut_off2, cuts2, pieces, piece_off = C.run(R.to_ints(5, 15.0), np.zeros(0, np.uint8), none, np.zeros(0, np.int32), np.zeros(1, np.int64), none, 0)
    assert cut_off2.tolist() == [0] and piece_off.tolist() == [0] and cuts2.size == 0 and pieces.size == 0


def test_piece_spans_at_every_alignment(gpu_lib):
    """Piece spans that begin at blob offsets with every residue mod 16, every read split."""
    rng = np.random.RandomState(41)
    b = R.Blob()
    cut_off, cuts = [0], []
    for al in range(16):
        for n, cut in ((200 + al, (70, 87)), (4200, (3 + al, 40)), (40, (10, 10 + al % 3 + 1))):
            q = rng.randint(33 + 5, 33 + 40, n)
            q[cut[0] - 8:cut[0]] = 33 + 2
            b.add(q.tolist(), align=al)
            cuts += [cut[0], cut[1]]
            cut_off.append(len(cuts) // 2)
    qual, off, ln = b.arrays()
    cut_off, cuts = np.array(cut_off, np.int64), np.array(cuts, np.int64)
    o = R.to_ints(6, 14.0, 20, 4150, 11.0)
    pieces = C.check_case('alignments', o, qual, off, ln, cut_off, cuts, 0)[0]
    _device_is_host(o, qual, off, ln, cut_off, cuts)
    assert {(int(off[p[0]]) + p[1]) % 16 for p in pieces} == set(range(16))
    assert {(int(off[p[0]]) + p[1] + p[3][0]) % 16 for p in pieces} == set(range(16))
    assert len({p[0] for p in pieces}) == len(ln), 'every read is split'
    assert len({p[3][3] & R.FAIL for p in pieces}) >= 3


def test_bad_arguments_launch_nothing(gpu_lib):
    from custom_porechop_abi_amd._lib import PcabiError
    qual = np.full(100, 70, np.uint8)
    good = R.to_ints(4, 10.0)
    off, ln = np.array([0, 50], np.int64), np.array([50, 50], np.int32)
    co, cu = np.array([0, 1, 2], np.int64), np.array([10, 20, 10, 20], np.int64)
    for o, a in ((dict(good, window=65), off), (dict(good, max_mean_err=2 ** 32 + 1), off), (good, np.array([0, 60], np.int64))):
        with pytest.raises(PcabiError, match=r'\(-1\)'):
            C.run(o, qual, a, ln, co, cu, 0)


# ---- FileTrimmer ---------------------------------------------------------------------------------------
DATA = os.path.join(golden_lib.GOLDEN, 'data')
OPTS = dict(quality_window=10, quality_window_q=12.0, min_length=500, max_length=50000, min_mean_q=9.0)


def _case():
    return [c for c in golden_lib.g2()['cases'] if c['case'] == 'one_adapter_set'][0]


def _trimmer(min_split, **kw):
    from custom_porechop_abi_amd.pipeline import FileTrimmer
    from tests.test_pipeline import _matching
    o = _case()['opts']
    return FileTrimmer(_matching(_case()), o['scoring'], o['end_size'], o['end_threshold'], o['extra_end_trim'], o['min_trim_size'],
                       o['middle_threshold'], 10, 100, min_split, **kw)


def _adapters():
    from tests.test_pipeline import _matching
    sets = _matching(_case())
    return [a.start_sequence[1] for a in sets if a.start_sequence][0], [a.end_sequence[1] for a in sets if a.end_sequence][0]


def _write_fastq(path, recs):
    with open(path, 'w') as f:
        for name, seq, q in recs:
            f.write('@%s\n%s\n+\n%s\n' % (name, seq, ''.join(chr(33 + int(x)) for x in q)))
    return path


def _chimeras(tmp_path, n_reads=200):
    """About 200 reads: most with one or two planted middle adapters and low qualities beside them, pieces of
    all sizes around min_length, some reads without a middle adapter, some of poor quality throughout."""
    start, end = _adapters()
    rng = np.random.RandomState(51)

    def body(n):
        return ''.join(rng.choice(list('ACGT'), n))

    recs = []
    for i in range(n_reads):
        parts = [body(int(rng.randint(150, 2500))) for _ in range(int(rng.randint(1, 4)))]
        seq = start + (start if i % 2 else end).join(parts) + (end if i % 5 else '')
        q = np.full(len(seq), 30)
        at = len(start)
        for p in parts[:-1]:                               # Phred 3 on both sides of each junction
            at += len(p)
            lo, hi = int(rng.randint(0, 160)), int(rng.randint(0, 160))
            q[max(at - lo, 0):at + len(start) + hi] = 3
            at += len(start if i % 2 else end)
        if i % 9 == 0:
            q[:] = np.where(np.arange(len(seq)) % 2, 30, 3)  # every window reaches 12, the mean error is about Q6
        recs.append(('c%d extra words' % i if i % 4 == 0 else 'c%d' % i, seq, q))
    return _write_fastq(str(tmp_path / 'chimeras.fastq'), recs)


def _expected(batch, off_decisions, fork, min_split, opts):
    """From the decisions of the option-off run: the restatement's pieces, cuts and keep mask, the text of
    the FASTQ output and the tallies."""
    st, et, co, cu, _, keep = off_decisions
    o = R.to_ints(opts['quality_window'], opts['quality_window_q'], opts['min_length'], opts['max_length'], opts['min_mean_q'])
    ns = batch.lengths.astype(np.int64)
    spans = [R.py_span(int(n), int(a), int(e)) for n, a, e in zip(ns, st, et)]
    has_q = np.diff(batch.qual_off) == ns
    span_off = np.array([int(batch.qual_off[i]) + a if has_q[i] else -1 for i, (a, _) in enumerate(spans)], np.int64)
    span_len = np.array([b - a for a, b in spans], np.int32)
    pieces, piece_off, cut_off2, cuts2 = P.stage(batch.qual, span_off, span_len, co, cu, o)
    keep2 = np.ones(batch.n, np.uint8) if keep is None else keep.copy()
    text, n_split = [], 0
    for r in range(batch.n):
        ranges = P.read_ranges(co, cu, r)
        if any(e > b for b, e in ranges):
            n_split += 1
            keep2[r] = 1 if fork is None else fork[r]      # the pieces are judged, not the read
        judged = [(b, e, rec) for _, b, e, rec in pieces[piece_off[r]:piece_off[r + 1]]]
        for name, s, q in P.written(batch.name(r), batch.sequence(r), batch.quals(r), int(st[r]), int(et[r]), ranges, judged, min_split,
                                    bool(keep2[r])):
            text.append('@%s\n%s\n+\n%s\n' % (name, s, q))
    recs = [p[3] for p in pieces]
    tally = {'pieces': len(recs), 'piece_cropped': sum(r[0] + r[1] > 0 for r in recs), 'piece_cropped_bases': sum(r[0] + r[1] for r in recs),
             'piece_too_short': sum((r[3] & R.TOO_SHORT) != 0 for r in recs), 'piece_too_long': sum((r[3] & R.TOO_LONG) != 0 for r in recs),
             'piece_low_quality': sum((r[3] & R.LOW_QUALITY) != 0 for r in recs)}
    return pieces, (np.array(cut_off2, np.int64), np.array(cuts2, np.int64)), keep2, ''.join(text).encode(), tally, n_split


def _bam_content(path):
    from custom_porechop_abi_amd import misc
    b = misc.load_batch(path)
    return [(b.name(i), b.sequence(i), b.quals(i)) for i in range(b.n)]


@pytest.mark.parametrize('fmt,filter_reads', [('fastq', True), ('fastq', False), ('bam', False), ('fastq.gz', False)])
def test_file_trimmer_matches_restatement(gpu_lib, tmp_path, fmt, filter_reads):
    """fastq: the file against text built in Python; bam: against the unchanged writer given the restatement's
    cuts; fastq.gz: compressed on the device, the same text."""
    from custom_porechop_abi_amd import misc
    src = _chimeras(tmp_path)
    got, want = str(tmp_path / ('got.' + fmt)), str(tmp_path / ('want.' + fmt))
    kw = dict(filter_reads=filter_reads, gzip_on_device=fmt == 'fastq.gz')
    if fmt == 'bam':
        kw.update(keep_tags=True, keep_mods=True, keep_moves=True)
    on, off, plain = _trimmer(200, quality_per_piece=True, **dict(kw, **OPTS)), _trimmer(200, **dict(kw, **OPTS)), _trimmer(200, **kw)
    try:
        counts = on.trim_file(src, got, fmt)
        batch = misc.load_batch(src)
        d_off, d_plain = off.trim(batch), plain.trim(batch)
        fork = ((d_plain[0] > 0) & (d_plain[1] > 0)).astype(np.uint8) if filter_reads else None
        pieces, cuts2, keep2, text, tally, n_split = _expected(batch, d_off, fork, 200, OPTS)
        d = on.trim(batch)
        assert np.array_equal(d[0], d_off[0]) and np.array_equal(d[1], d_off[1]) and np.array_equal(d[4], d_off[4])
        assert np.array_equal(d[2], cuts2[0]) and np.array_equal(d[3], cuts2[1]) and np.array_equal(d[5], keep2)
        assert P.as_tuples(on.last_quality_pieces) == pieces and on.last_quality.tobytes() == off.last_quality.tobytes()
        assert [int(on.last_piece_off[r + 1] - on.last_piece_off[r]) for r in range(batch.n)] == \
            [sum(p[0] == r for p in pieces) for r in range(batch.n)]
        if fmt == 'bam':
            misc.write_reads(batch, want, fmt, d_off[0], d_off[1], None, 200, False, select=keep2, cut_arrays=cuts2)
            misc.bgzf_finish(want)
    finally:
        on.close()
        off.close()
        plain.close()
    if fmt == 'bam':
        assert _bam_content(got) == _bam_content(want) and len(_bam_content(got)) > 100
        names = [n for n, _, _ in _bam_content(got)]
        assert [('@' + n).encode() for n in names] == [ln.split(b' ')[0] for ln in text.split(b'\n')[::4] if ln]
    else:
        with (gzip.open if fmt == 'fastq.gz' else open)(got, 'rb') as f:
            assert f.read() == text
    assert {k: counts['quality'][k] for k in tally} == tally and counts['reads_in'] == batch.n
    # the input does what it was made for
    assert n_split > 100 and tally['pieces'] > 250 and tally['piece_cropped'] > 100
    assert tally['piece_too_short'] > 20 and tally['piece_low_quality'] > 5
    assert text.count(b'_2') > 30 and b'extra words' in text


def test_pieces_are_what_is_filtered(gpu_lib, tmp_path):
    """A read of two 300-base pieces with min_length=500 writes nothing; a 60 kb chimera of two 30 kb reads
    with max_length=50000 writes both halves (min_split_read_size=0)."""
    start, end = _adapters()
    rng = np.random.RandomState(61)

    def body(n):
        return ''.join(rng.choice(list('ACGT'), n))

    recs = [('two300', start + body(300) + start + body(300) + end), ('chimera', start + body(30000) + start + body(30000) + end),
            ('whole', start + body(900) + end)]
    src = _write_fastq(str(tmp_path / 'in.fastq'), [(n, s, np.full(len(s), 30)) for n, s in recs])
    out = str(tmp_path / 'out.fastq')
    ft = _trimmer(0, filter_reads=False, min_length=500, max_length=50000, quality_per_piece=True)
    try:
        counts = ft.trim_file(src, out, 'fastq')
    finally:
        ft.close()
    got = C._parse_fastq(out)
    assert [n for n, _, _ in got] == ['chimera_1', 'chimera_2', 'whole']
    assert all(29800 <= len(s) <= 30000 and s in recs[1][1] for _, s, _ in got[:2]) and 850 < len(got[2][1]) <= 900
    assert counts['quality']['pieces'] == 4 and counts['quality']['piece_too_short'] == 2 and counts['quality']['piece_too_long'] == 0
    assert counts['quality']['too_long'] == 1      # the chimera as a whole: no longer what decides


def test_option_needs_the_stage(gpu_lib):
    with pytest.raises(ValueError, match='quality_per_piece'):
        _trimmer(1000, quality_per_piece=True)


def test_option_changes_nothing_without_middle_hits(gpu_lib, tmp_path):
    from custom_porechop_abi_amd import misc
    start, end = _adapters()
    rng = np.random.RandomState(71)
    recs = []
    for i in range(60):
        n = int(rng.randint(200, 3000))
        seq = (start if i % 3 else '') + ''.join(rng.choice(list('ACGT'), n)) + (end if i % 4 else '')
        q = np.full(len(seq), 30)
        q[:int(rng.randint(0, 150))] = 3
        recs.append(('p%d' % i, seq, q))
    src = _write_fastq(str(tmp_path / 'plain.fastq'), recs)
    on, off = _trimmer(1000, quality_per_piece=True, **OPTS), _trimmer(1000, **OPTS)
    try:
        batch = misc.load_batch(src)
        a, b = on.trim(batch), off.trim(batch)
        assert int(b[2][-1]) == 0 and on.last_quality_pieces.size == 0
        for x, y in zip(a, b):
            assert (x is None and y is None) or (np.array_equal(x, y) and x.dtype == y.dtype)
        c_on, c_off = on.trim_file(src, str(tmp_path / 'a.fastq'), 'fastq'), off.trim_file(src, str(tmp_path / 'b.fastq'), 'fastq')
    finally:
        on.close()
        off.close()
    assert c_on['quality']['pieces'] == 0 and {k: v for k, v in c_on['quality'].items() if not k.startswith('piece')} == c_off['quality']
    with open(str(tmp_path / 'a.fastq'), 'rb') as f, open(str(tmp_path / 'b.fastq'), 'rb') as g:
        assert f.read() == g.read() != b''


def test_bins_get_the_new_cuts(gpu_lib, tmp_path):
    """With barcode_dir set the bins' writer takes the same cuts: these adapters are no barcodes, so every read
    goes to the bin 'none', which must hold what the main output of a run without bins holds."""
    src = _chimeras(tmp_path)
    bdir, main = str(tmp_path / 'bins'), str(tmp_path / 'main.fastq')
    binned, plain = _trimmer(200, quality_per_piece=True, barcode_dir=bdir, **OPTS), _trimmer(200, quality_per_piece=True, **OPTS)
    try:
        c_bins = binned.trim_file(src, str(tmp_path / 'unused'), 'fastq')
        c_main = plain.trim_file(src, main, 'fastq')
    finally:
        binned.close()
        plain.close()
    assert sorted(os.listdir(bdir)) == ['none.fastq'] and c_bins['quality'] == c_main['quality'] and c_main['quality']['pieces'] > 250
    with open(os.path.join(bdir, 'none.fastq'), 'rb') as f, open(main, 'rb') as g:
        text = f.read()
        assert text == g.read() and text.count(b'_2') > 30


def test_tags_follow_the_pieces(gpu_lib, tmp_path):
    """BAM to BAM with keep_tags / keep_mods / keep_moves: every written piece's whole aux chain -- MM ML MN mv
    ts remapped, the other tags kept -- is what tests/mods_ref.py and tests/moves_ref.py give for the cropped
    piece's span of its read; names, bases and qualities are the restatement's."""
    from custom_porechop_abi_amd import misc
    from tests import bam_lib as B
    from tests import moves_ref as M
    from tests import test_mods_cpu as MC
    from tests import test_moves_cpu as VC
    start, end = _adapters()
    rng = np.random.RandomState(81)
    recs, reads = [], {}
    for i in range(24):
        parts = [''.join(rng.choice(list('ACGT'), int(rng.randint(250, 1800)))) for _ in range(1 + i % 3)]
        seq = start + start.join(parts) + end
        qual = np.full(len(seq), 30)
        at = len(start)
        for p in parts[:-1]:                               # Phred 2 on both sides of each junction
            at += len(p)
            qual[max(at - int(rng.randint(0, 260)), 0):at + len(start) + int(rng.randint(0, 260))] = 2
            at += len(start)
        mods = MC.make_tags(rng, seq, [MC.HEADERS[0], MC.HEADERS[3]], 0.3, with_mn='i') if i % 4 else b''
        aux = mods + b'RGZgrp\0' + VC.ts_aux(10 + i, 'i') + VC.mv_aux(5, VC.make_moves(rng, len(seq), 2.0, lead=int(rng.randint(0, 9))))
        name = b'r%d' % i
        recs.append({'name': name, 'seq': seq, 'qual': qual.tolist(), 'flag': 4, 'aux': aux})
        reads[name.decode()] = (seq, aux, mods)
    src, out = str(tmp_path / 'in.bam'), str(tmp_path / 'out.bam')
    with open(src, 'wb') as f:
        f.write(B.make_bam(recs, b'@HD\tVN:1.6\tSO:unknown\n@RG\tID:grp\n', (), 5000))
    opts = dict(quality_window=8, quality_window_q=20.0, min_length=300, max_length=0, min_mean_q=0.0)
    kw = dict(filter_reads=False, keep_tags=True, keep_mods=True, keep_moves=True)
    on, off = _trimmer(100, quality_per_piece=True, **dict(kw, **opts)), _trimmer(100, **dict(kw, **opts))
    try:
        on.trim_file(src, out, 'bam')
        batch = misc.load_batch(src, keep_aux=True)
        d_off = off.trim(batch)
    finally:
        on.close()
        off.close()
    pieces, _, keep2, _, tally, n_split = _expected(batch, d_off, None, 100, opts)
    piece_off = np.concatenate([[0], np.cumsum(np.bincount([p[0] for p in pieces], minlength=batch.n))])
    want = []
    for r in range(batch.n):
        judged = [(b, e, rec) for _, b, e, rec in pieces[piece_off[r]:piece_off[r + 1]]]
        want += [(r,) + w for w in P.written_spans(batch.name(r), int(batch.lengths[r]), int(d_off[0][r]), int(d_off[1][r]),
                                                   P.read_ranges(d_off[2], d_off[3], r), judged, 100, bool(keep2[r]))]
    back = misc.load_batch(out, keep_aux=True)
    assert [back.name(k) for k in range(back.n)] == [w[1] for w in want]
    remapped = inner = 0
    for k, (r, name, s0, n) in enumerate(want):
        seq, aux, mods = reads[batch.name(r)]
        assert back.sequence(k) == seq[s0:s0 + n] and back.quals(k) == batch.quals(r)[s0:s0 + n], name
        verbatim = (s0, n) == (0, len(seq))
        want_mods = MC.expected_tags({'seq': seq, 'aux': mods}, s0, n) if mods else b''
        assert back.aux(k) == M.part_aux(aux, len(seq), [(s0, n)], 0, verbatim, True, want_mods), name
        tags = dict((t, raw) for t, _, raw in M.walk_aux(back.aux(k)))
        assert b'mv' in tags and b'ts' in tags and b'RG' in tags and (not mods or b'MM' in tags), name
        remapped += bool(mods) and not verbatim
        inner += name.endswith('_2') or name.endswith('_3')
    # the input does what it was made for: split reads, cropped pieces, pieces dropped for their length
    assert n_split >= 12 and tally['piece_cropped'] >= 12 and tally['piece_too_short'] > 0 and remapped > 10 and inner > 6
