"""The piece stage's host build (engine.quality_filter_pieces(..., device=-1): csrc/pcabi_pieces.h and
csrc/pcabi_qual.h on the host) against tests/qual_pieces_ref.py's restatement: every field of every piece and
every entry of the new cut layout; the enumerator against what today's writer writes; and the two headers as
a program of their own under the sanitizers. No GPU needed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import qual_pieces_ref as P
from tests import qual_ref as R

DEVICE = -1
HERE = os.path.dirname(os.path.abspath(__file__))


def run(o, qual, off, ln, cut_off, cuts, device):
    from custom_porechop_abi_amd import engine
    opts = np.zeros(1, engine.QUAL_OPTS)
    for k, v in o.items():
        opts[k] = v
    return engine.quality_filter_pieces(qual, off, ln, cut_off, cuts, opts=opts, device=device)


def check_case(name, o, qual, off, ln, cut_off, cuts, device):
    cut_off2, cuts2, pieces, piece_off = run(o, qual, off, ln, cut_off, cuts, device)
    exp = P.stage(qual, off, ln, cut_off, cuts, o)
    got = P.as_tuples(pieces)
    bad = [i for i, (g, e) in enumerate(zip(got, exp[0])) if g != e]
    assert len(got) == len(exp[0]) and not bad, (name, len(got), len(exp[0]), bad[:5], got[bad[0]], exp[0][bad[0]])
    assert piece_off.tolist() == exp[1], name
    assert cut_off2.tolist() == exp[2], name
    assert cuts2.tolist() == exp[3], name
    return exp


@pytest.mark.parametrize('k', range(len(P.option_sets())))
def test_fuzz_matches_restatement(k):
    check_case('fuzz %d' % k, P.option_sets()[k], *P.fuzz_batch(), DEVICE)


def test_fuzz_covers_what_it_promises():
    qual, off, ln, cut_off, cuts = P.fuzz_batch()
    assert 2500 <= len(ln) <= 3500 and int(ln.max()) <= 20000 and int(np.diff(cut_off).max()) == 12
    seen = {k: 0 for k in ('empty', 'below0', 'beyond', 'outside', 'whole', 'duplicate', 'adjacent', 'nested', 'overlap', 'unsorted',
                           'no_qual_split', 'outside_only')}
    for r in range(len(ln)):
        tl, rg = int(ln[r]), P.read_ranges(cut_off, cuts, r)
        live = [x for x in rg if x[1] > x[0]]
        seen['empty'] += len(live) < len(rg)
        seen['below0'] += any(b < 0 < e for b, e in live)
        seen['beyond'] += any(b < tl < e for b, e in live)
        outside = [x for x in live if x[0] >= tl or x[1] <= 0]
        seen['outside'] += bool(outside)
        seen['outside_only'] += bool(live) and len(outside) == len(live) and tl > 0
        seen['whole'] += any(b <= 0 and e >= tl for b, e in live) and tl > 0
        seen['duplicate'] += len(set(live)) < len(live)
        seen['adjacent'] += any(x[1] == y[0] for x in live for y in live)
        seen['nested'] += any(x[0] < y[0] and y[1] < x[1] for x in live for y in live)
        seen['overlap'] += any(x[0] < y[0] < x[1] < y[1] for x in live for y in live)
        seen['unsorted'] += [x[0] for x in rg] != sorted(x[0] for x in rg)
        seen['no_qual_split'] += off[r] < 0 and bool(live)
    assert all(v >= 5 for v in seen.values()), seen
    # a read whose only non-empty ranges lie outside [0, tl) is split into the one piece [0, tl)
    assert P.pieces_of(10, [(12, 15)]) == [(0, 10)] and P.pieces_of(10, [(-5, -2), (3, 3)]) == [(0, 10)]
    assert P.pieces_of(10, [(3, 3)]) == [] and P.pieces_of(10, [(-1, 11)]) == [] and P.pieces_of(0, [(0, 5)]) == []
    assert P.pieces_of(10, [(4, 6), (0, 2), (5, 8)]) == [(2, 4), (8, 10)]


def test_reads_without_qualities():
    """Their pieces are enumerated, never cropped, pass the quality test, and the length tests apply."""
    qual, off, ln, cut_off, cuts = P.fuzz_batch()
    o = P.option_sets()[6]
    assert o['window'] == 5 and o['min_length'] == 300 and o['max_mean_err'] < 2 ** 32
    pieces = run(o, qual, off, ln, cut_off, cuts, DEVICE)[2]
    bare = pieces[off[pieces['read']] < 0]
    q = bare['q']
    assert bare.size > 50 and not (q['front'] | q['tail']).any() and (q['kept'] == bare['end'] - bare['begin']).all()
    assert ((q['flags'] & R.NO_QUALITIES) != 0).all() and not (q['flags'] & R.LOW_QUALITY).any()
    assert (((q['flags'] & R.TOO_SHORT) != 0) == (q['kept'] < 300)).all() and (q['flags'] & R.TOO_SHORT).any()


@pytest.mark.parametrize('k', range(len(P.crafted_cases())))
def test_crafted_reads(k):
    case = P.crafted_cases()[k]
    pieces = check_case(*case, DEVICE)[0]
    name, o = case[0], case[1]
    if name == '300 ranges':
        assert len(pieces) == 301 and int(case[5][-1]) == 300
        assert sum(p[3][0] > 0 for p in pieces) >= 70
    if name.startswith('piece sizes'):
        W = o['window']
        assert [p[2] - p[1] for p in pieces] == [W - 1, W, 4095, 4096, 4097, 8192, W - 1, W]
        ok = [(p[3][3] & R.FAIL) == 0 for p in pieces]
        assert [p[3][2] for p in pieces][::6] == [0, 0] and not ok[0] and not ok[6] and ok[1:5] == [True] * 4
    if name == 'after the whole-read crop':
        W = o['window']
        assert len(pieces) == 2 and pieces[0][1] == 0 and pieces[1][2] == int(case[4][0])
        assert all(p[2] - p[1] >= W for p in pieces)
        assert pieces[0][3][0] == 0 and pieces[1][3][1] == 0 and pieces[0][3][1] > 0 and pieces[1][3][0] > 0


@pytest.mark.parametrize('k', range(len(P.equality_cases())))
def test_threshold_equality(k):
    case = P.equality_cases()[k]
    pieces = check_case(*case[:-1], DEVICE)[0]
    assert [(p[3][3] & R.FAIL) == 0 for p in pieces] == case[-1], case[0]


def test_degenerate_batches():
    o = R.to_ints(5, 15.0, 10, 0, 10.0)
    none = np.zeros(0, np.int64)
    cut_off2, cuts2, pieces, piece_off = run(o, np.zeros(0, np.uint8), none, np.zeros(0, np.int32), np.zeros(1, np.int64), none, DEVICE)
    assert cut_off2.tolist() == [0] and piece_off.tolist() == [0] and cuts2.size == 0 and pieces.size == 0
    # no ranges, and ranges that are all empty: the output equals the input, with 0 pieces
    _, qual, off, ln = R.random_batch()
    n = len(ln)
    for cut_off, cuts in ((np.zeros(n + 1, np.int64), none), (np.arange(n + 1, dtype=np.int64), np.repeat(np.arange(n, dtype=np.int64), 2))):
        cut_off2, cuts2, pieces, piece_off = run(o, qual, off, ln, cut_off, cuts, DEVICE)
        assert np.array_equal(cut_off2, cut_off) and np.array_equal(cuts2, cuts) and pieces.size == 0 and not piece_off.any()


def test_bad_arguments_are_refused():
    from custom_porechop_abi_amd import engine
    from custom_porechop_abi_amd._lib import PcabiError, lib
    qual = np.full(100, 70, np.uint8)
    good = R.to_ints(4, 10.0)
    off, ln = np.array([0, 50], np.int64), np.array([50, 50], np.int32)
    co, cu = np.array([0, 1, 2], np.int64), np.array([10, 20, 10, 20], np.int64)
    assert len(run(good, qual, off, ln, co, cu, DEVICE)[2]) == 4
    for o, a, n in ((dict(good, window=65), off, ln), (dict(good, max_mean_err=2 ** 32 + 1), off, ln),
                    (good, np.array([0, 60], np.int64), ln), (good, off, np.array([50, -1], np.int32))):
        with pytest.raises(PcabiError, match=r'\(-1\)'):
            run(o, qual, a, n, co, cu, DEVICE)
    # (engine's own shape check reads cut_off[-1]: the rest goes straight to the library)
    L = lib()
    assert _host(L, engine, good, qual, off, ln, co, cu, 4, 10) == 0
    # cut_off that descends or does not begin at 0
    assert _host(L, engine, good, qual, off, ln, np.array([0, 2, 1], np.int64), cu, 4, 10) == -1
    assert _host(L, engine, good, qual, off, ln, np.array([1, 1, 2], np.int64), cu, 4, 10) == -1
    # outputs that are too small: pieces below the bound of 4, cuts below 2 + 2 * 4 ranges
    assert _host(L, engine, good, qual, off, ln, co, cu, 3, 10) == -1 and _host(L, engine, good, qual, off, ln, co, cu, 4, 9) == -1


def _host(L, engine, o, qual, off, ln, co, cu, piece_cap, cuts_cap):
    opts = np.zeros(1, engine.QUAL_OPTS)
    for k, v in o.items():
        opts[k] = v
    n = len(ln)
    piece_off, cut_off2 = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    pieces, cuts2 = np.zeros(max(piece_cap, 1), engine.QUAL_PIECE), np.zeros(2 * max(cuts_cap, 1), np.int64)
    ptr = engine._ptr
    return int(L.pcabi_qual_pieces_host(-1, ptr(qual), qual.size, ptr(off), ptr(ln), n, ptr(co), ptr(cu), ptr(opts), ptr(piece_off),
                                        ptr(pieces), piece_cap, ptr(cut_off2), ptr(cuts2), cuts_cap))


def test_bounds():
    from custom_porechop_abi_amd import engine
    ln = np.array([100, 5000, 0, 9000], np.int32)
    co = np.array([0, 0, 3, 4, 4], np.int64)
    # pieces <= ranges + reads with ranges; segments <= n_segs of those reads' spans + that
    assert engine.quality_pieces_bound(ln, co) == (4 + 2, 2 + 0 + 6)
    assert engine.quality_pieces_bound(ln[:0], co[:1]) == (0, 0)


# ---- 2. the enumerator against today's writer ---------------------------------------------------------------
def _parse_fastq(path):
    with open(path) as f:
        lines = f.read().split('\n')
    assert lines[-1] == '' and (len(lines) - 1) % 4 == 0
    return [(lines[k][1:], lines[k + 1], lines[k + 3]) for k in range(0, len(lines) - 1, 4)]


def test_enumerator_matches_the_writer(tmp_path):
    """What the unchanged writer writes for random cuts with min_split_read_size = 0: the names _1 .. _n and
    the lengths of the restatement's pieces (csrc/pcabi_pieces.h and read_parts cannot drift apart)."""
    from custom_porechop_abi_amd import misc
    rng = np.random.RandomState(23)
    src, out = str(tmp_path / 'in.fastq'), str(tmp_path / 'out.fastq')
    reads = []
    with open(src, 'w') as f:
        for i in range(400):
            n = int(rng.randint(1, 900))
            seq = ''.join(rng.choice(list('ACGT'), n))
            qual = ''.join(chr(c) for c in rng.randint(35, 80, n))
            name = 'r%d' % i + (' with a comment' if i % 3 == 0 else '\tXY:i:1' if i % 3 == 1 else '')
            reads.append((name, seq, qual))
            f.write('@%s\n%s\n+\n%s\n' % (name, seq, qual))
    batch = misc.load_batch(src)
    cut_off, cuts = [0], []
    for name, seq, _ in reads:
        for s, e in P._random_ranges(rng, len(seq), int(rng.randint(0, 9))):
            cuts += [s, e]
        cut_off.append(len(cuts) // 2)
    cut_off, cuts = np.array(cut_off, np.int64), np.array(cuts, np.int64)
    misc.write_reads(batch, out, 'fastq', None, None, None, 0, False, cut_arrays=(cut_off, cuts))
    want, n_split = [], 0
    for r, (name, seq, qual) in enumerate(reads):
        ranges = P.read_ranges(cut_off, cuts, r)
        if not any(e > b for b, e in ranges):
            want.append((name, seq, qual))
            continue
        n_split += 1
        for k, (b, e) in enumerate(P.pieces_of(len(seq), ranges)):
            want.append((P.numbered(name, k + 1), seq[b:e], qual[b:e]))
    assert _parse_fastq(out) == want and n_split > 200 and len(want) > 600


# ---- 4. the two headers under the sanitizers ----------------------------------------------------------------
def test_pieces_layer_under_sanitizers(tmp_path):
    """tests/qual_pieces_fuzz_main.cpp (csrc/pcabi_pieces.h and csrc/pcabi_qual.h alone), built with
    -fsanitize=address,undefined as a program of its own and run as a child process."""
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path / 'qual_pieces_fuzz')
    base = ['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
            os.path.join(HERE, 'qual_pieces_fuzz_main.cpp')]
    for extra in (['-static-libasan', '-static-libubsan'], []):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        if r.returncode == 0:
            break
    if r.returncode != 0 and ('asan' in r.stderr or 'ubsan' in r.stderr or 'sanitize' in r.stderr):
        pytest.skip('the sanitizer runtime cannot be linked')
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, '1', '4000'], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'rounds 4000' in r.stdout
