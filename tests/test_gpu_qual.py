"""The quality stage on the GPU: k_qual_crop / the scan / k_qual_sum / k_qual_finish (engine.quality_filter with
device=0) against tests/qual_ref.py's restatement and, field for field, the host build; FileTrimmer with the
stage on against a run with the stage off whose trims and keep mask were replaced by the restatement's; the
tags of a BAM input following the crop; and the options off."""
import os
import signal

import numpy as np
import pytest

from tests import bam_lib as B
from tests import golden_lib
from tests import moves_ref as M
from tests import qual_ref as R
from tests import test_mods_cpu as MC
from tests import test_moves_cpu as VC
from tests import test_qual_cpu as C

pytestmark = pytest.mark.gpu

DATA = os.path.join(golden_lib.GOLDEN, 'data')
OPTS = dict(quality_window=10, quality_window_q=12.0, min_length=1000, max_length=11500, min_mean_q=9.0)


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


# ---- 1. the table-level API ----------------------------------------------------------------------------
def _device_and_host(name, o, qual, off, ln):
    exp = C.check_case(name, o, qual, off, ln, 0)
    dev, host = C.run(o, qual, off, ln, 0), C.run(o, qual, off, ln, -1)
    assert dev.tobytes() == host.tobytes(), name
    return exp


@pytest.mark.parametrize('k', range(len(R.crop_cases())))
def test_cases_on_device(gpu_lib, k):
    _device_and_host(*R.crop_cases()[k])


def test_threshold_equality_on_device(gpu_lib):
    for name, o, qual, off, ln, ok in R.equality_cases():
        exp = _device_and_host(name, o, qual, off, ln)
        assert [(r[3] & R.FAIL) == 0 for r in exp] == ok, name


def test_bad_arguments_launch_nothing(gpu_lib):
    from custom_porechop_abi_amd._lib import PcabiError
    qual = np.full(100, 70, np.uint8)
    good = R.to_ints(4, 10.0)
    for o, off, ln in ((dict(good, window=65), [0], [10]), (dict(good, max_mean_err=2 ** 32 + 1), [0], [10]), (good, [95], [10])):
        with pytest.raises(PcabiError, match=r'\(-1\)'):
            C.run(o, qual, np.array(off, np.int64), np.array(ln, np.int32), 0)


def test_random_batch(gpu_lib):
    o, qual, off, ln = R.random_batch()
    exp = _device_and_host('random', o, qual, off, ln)
    assert len(exp) == 2000 and int(ln.max()) <= 9000 and qual.size < 12 << 20
    cropped = sum(r[0] + r[1] > 0 for r in exp)
    failed = sum((r[3] & R.FAIL) != 0 for r in exp)
    for flag in (R.TOO_SHORT, R.TOO_LONG, R.LOW_QUALITY, R.NO_QUALITIES):
        assert 0 < sum((r[3] & flag) != 0 for r in exp) < len(exp)
    assert len(exp) // 5 < cropped < len(exp) // 2 and len(exp) // 5 < failed < len(exp) // 2


# ---- 2. FileTrimmer ------------------------------------------------------------------------------------
def _case():
    return [c for c in golden_lib.g2()['cases'] if c['case'] == 'one_adapter_set'][0]


def _trimmer(**kw):
    from tests.test_gpu_bam_pack import _trimmer as make
    return make(_case(), **kw)


def _fastq(tmp_path):
    """The golden reads (they carry qualities) and hand-made ones: low-quality ends around adapters, a middle
    adapter, reads the filters drop, and a read shorter than end_size that ends in the end adapter (the end
    trim counts from end_size, so it is longer than the read)."""
    from custom_porechop_abi_amd import misc
    from tests.test_pipeline import _matching
    sets = _matching(_case())
    start = [a.start_sequence[1] for a in sets if a.start_sequence][0]
    end = [a.end_sequence[1] for a in sets if a.end_sequence][0]
    rng = np.random.RandomState(21)

    def body(n):
        return ''.join(rng.choice(list('ACGT'), n))

    def quals(n, head, tail, q=30):
        v = np.full(n, q)
        v[:head] = 3
        v[n - tail:] = 2
        return ''.join(chr(33 + int(x)) for x in v)

    g = misc.load_batch(os.path.join(DATA, 'test_one_adapter_set.fastq.gz'))
    recs = [(g.name(i), g.sequence(i), g.quals(i)) for i in range(g.n)]
    assert all(len(s) == len(q) for _, s, q in recs)
    made = [('low_ends', start + body(3000) + end, 140, 95), ('middle', start + body(1500) + start + body(1600) + end, 70, 0),
            ('short_end', body(40) + end, 0, 0), ('no_adapters', body(2500), 33, 44), ('short', start + body(400) + end, 0, 0)]
    for name, seq, head, tail in made:
        recs.append((name, seq, quals(len(seq), min(head, len(seq)), tail)))
    # every window of 10 reaches a mean of 12, but half of the bases are Phred 3: a mean error of about Q6
    seq = start + body(2000) + end
    recs.append(('poor_mean', seq, ''.join(chr(33 + (30 if k % 2 else 3)) for k in range(len(seq)))))
    path = str(tmp_path / 'in.fastq')
    with open(path, 'w') as f:
        for name, seq, q in recs:
            f.write('@%s\n%s\n+\n%s\n' % (name, seq, q))
    return path


def _expected(ft_off, batch, opts):
    """The stage-off trimmer's decisions with the restatement's crops and flags put in their place."""
    st, et, _, _, _, keep = ft_off.trim(batch)
    o = R.to_ints(opts['quality_window'], opts['quality_window_q'], opts['min_length'], opts['max_length'], opts['min_mean_q'])
    ns = batch.lengths.astype(np.int64)
    spans = [R.py_span(int(n), int(a), int(e)) for n, a, e in zip(ns, st, et)]
    has_q = np.diff(batch.qual_off) == ns
    off = np.array([int(batch.qual_off[i]) + a if has_q[i] else -1 for i, (a, _) in enumerate(spans)], np.int64)
    recs = R.records(batch.qual, off, [b - a for a, b in spans], o)
    new = [R.new_trims(int(n), int(a), int(e), r[0], r[1]) for n, a, e, r in zip(ns, st, et, recs)]
    st2, et2 = (np.array([t[k] for t in new], np.int32) for k in (0, 1))
    co, cu, _ = ft_off.middle_scan(batch, st2, et2)
    passed = np.array([(r[3] & R.FAIL) == 0 for r in recs], np.uint8)
    keep2 = passed if keep is None else keep & passed
    tally = {'cropped_reads': sum(r[0] + r[1] > 0 for r in recs), 'cropped_bases': sum(r[0] + r[1] for r in recs),
             'too_short': sum((r[3] & R.TOO_SHORT) != 0 for r in recs), 'too_long': sum((r[3] & R.TOO_LONG) != 0 for r in recs),
             'low_quality': sum((r[3] & R.LOW_QUALITY) != 0 for r in recs), 'no_qualities': sum((r[3] & R.NO_QUALITIES) != 0 for r in recs)}
    return (st, et), (st2, et2), (co, cu), keep2, recs, tally


def _content(path, fmt):
    from custom_porechop_abi_amd import misc
    if fmt != 'bam':
        with open(path, 'rb') as f:
            return f.read()
    b = misc.load_batch(path)
    return [(b.name(i), b.sequence(i), b.quals(i)) for i in range(b.n)]


@pytest.mark.parametrize('fmt,filter_reads', [('fastq', True), ('bam', False)])
def test_file_trimmer_matches_restatement(gpu_lib, tmp_path, fmt, filter_reads):
    from custom_porechop_abi_amd import misc
    src = _fastq(tmp_path)
    got, want = str(tmp_path / ('got.' + fmt)), str(tmp_path / ('want.' + fmt))
    on, off = _trimmer(filter_reads=filter_reads, **OPTS), _trimmer(filter_reads=filter_reads)
    try:
        counts = on.trim_file(src, got, fmt)
        batch = misc.load_batch(src)
        (st, et), (st2, et2), cuts, keep2, recs, tally = _expected(off, batch, OPTS)
        misc.write_reads(batch, want, fmt, st2, et2, None, off.min_split, off.discard_middle, select=keep2, cut_arrays=cuts)
        if fmt == 'bam':
            misc.bgzf_finish(want)
        # the stage on, on the same batch: the decisions themselves
        d = on.trim(batch)
        assert np.array_equal(d[0], st2) and np.array_equal(d[1], et2) and np.array_equal(d[5], keep2)
        assert np.array_equal(d[2], cuts[0]) and np.array_equal(d[3], cuts[1])
        assert R.as_tuples(on.last_quality) == recs
    finally:
        on.close()
        off.close()
    assert _content(got, fmt) == _content(want, fmt) and len(_content(got, fmt)) > 0
    assert counts['quality'] == tally and counts['reads_in'] == batch.n and counts['reads_kept'] == int(keep2.sum())
    # the input does what it was made for
    assert all(tally[k] > 0 for k in ('cropped_reads', 'too_short', 'too_long', 'low_quality')) and tally['no_qualities'] == 0
    assert 0 < int(keep2.sum()) < batch.n
    assert any(int(e) > int(n) for e, n in zip(et, batch.lengths)), 'no end trim longer than its read'
    assert cuts[0][-1] > 0, 'no middle adapter was cut'
    changed = [(a, b, c, e) for a, b, c, e in zip(st, et, st2, et2) if (a, b) != (c, e)]
    assert changed and any(a > 0 and b > 0 for a, b, _, _ in changed)


def test_options_off_change_nothing(gpu_lib, tmp_path):
    from custom_porechop_abi_amd import misc
    src = _fastq(tmp_path)
    plain = _trimmer()
    off = _trimmer(quality_window=0, quality_window_q=0.0, min_length=0, max_length=0, min_mean_q=0.0)
    # a window quality without a window switches nothing on
    q_only = _trimmer(quality_window_q=30.0)
    try:
        batch = misc.load_batch(src)
        a, b, c = plain.trim(batch), off.trim(batch), q_only.trim(batch)
        assert len(a) == len(b) == 6
        for x, y, z in zip(a, b, c):
            assert (x is None and y is None and z is None) or (np.array_equal(x, y) and np.array_equal(x, z) and x.dtype == y.dtype)
        assert off.last_quality is None
        counts = [t.trim_file(src, str(tmp_path / name), 'fastq') for t, name in ((plain, 'a.fastq'), (off, 'b.fastq'))]
    finally:
        plain.close()
        off.close()
        q_only.close()
    assert counts[0] == counts[1] and 'quality' not in counts[0]
    assert _content(str(tmp_path / 'a.fastq'), 'fastq') == _content(str(tmp_path / 'b.fastq'), 'fastq') != b''


def test_tags_follow_the_crop(gpu_lib, tmp_path):
    """BAM to BAM with keep_tags / keep_mods / keep_moves: MM ML MN mv ts of a cropped read are those of
    the cropped span by tests/mods_ref.py and tests/moves_ref.py."""
    from custom_porechop_abi_amd import misc
    rng = np.random.RandomState(31)
    recs, reads = [], {}
    for i in range(14):
        n = int(rng.randint(300, 6000))
        seq = ''.join(rng.choice(list('ACGT'), n))
        head, tail = (0, 0) if i % 5 == 0 else (int(rng.randint(0, 120)), int(rng.randint(0, 120)))
        qual = [2] * head + [30] * (n - head - tail) + [3] * tail
        mods = MC.make_tags(rng, seq, [MC.HEADERS[0], MC.HEADERS[3]], 0.3, with_mn='i') if i % 3 else b''
        aux = mods + b'RGZgrp\0' + VC.ts_aux(10 + i, 'i') + VC.mv_aux(5, VC.make_moves(rng, n, 2.0, lead=int(rng.randint(0, 9))))
        name = b'r%d' % i
        recs.append({'name': name, 'seq': seq, 'qual': qual, 'flag': 4, 'aux': aux})
        reads[name.decode()] = (seq, aux, mods)
    src, out = str(tmp_path / 'in.bam'), str(tmp_path / 'out.bam')
    with open(src, 'wb') as f:
        f.write(B.make_bam(recs, b'@HD\tVN:1.6\tSO:unknown\n@RG\tID:grp\n', (), 5000))
    opts = dict(quality_window=8, quality_window_q=20.0, min_length=0, max_length=0, min_mean_q=0.0)
    kw = dict(filter_reads=False, keep_tags=True, keep_mods=True, keep_moves=True)
    on, off = _trimmer(**dict(kw, **opts)), _trimmer(**kw)
    try:
        on.trim_file(src, out, 'bam')
        batch = misc.load_batch(src, keep_aux=True)
        _, (st2, et2), cuts, keep2, qrecs, tally = _expected(off, batch, opts)
    finally:
        on.close()
        off.close()
    assert cuts[0][-1] == 0 and keep2.all() and 0 < tally['cropped_reads'] < batch.n
    back = misc.load_batch(out, keep_aux=True)
    assert back.n == batch.n
    remapped = 0
    for k in range(back.n):
        seq, aux, mods = reads[back.name(k)]
        a, b = R.py_span(len(seq), int(st2[k]), int(et2[k]))
        assert back.sequence(k) == seq[a:b]
        verbatim = (a, b) == (0, len(seq))
        want_mods = MC.expected_tags({'seq': seq, 'aux': mods}, a, b - a) if mods else b''
        assert back.aux(k) == M.part_aux(aux, len(seq), [(a, b - a)], 0, verbatim, True, want_mods), back.name(k)
        remapped += (not verbatim) and a > 0
    assert remapped > 3
