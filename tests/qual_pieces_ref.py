"""The piece stage's rule (include/pcabi.h pcabi_qual_pieces_*) restated in plain Python: the pieces of a
split read by marking every position a non-empty range covers, tests/qual_ref.py applied to each piece, the
new cut layout and the records a writer emits from it; and the inputs at which the rule can go wrong
(tests/test_qual_pieces_cpu.py runs them on the host build, tests/test_gpu_qual_pieces.py on the device).
Nothing here comes from the code under test."""
import functools

import numpy as np

from tests import qual_ref as R


def pieces_of(tl, ranges):
    """The pieces [(begin, end)] of a read of tl positions with `ranges` [(begin, end)]; [] when no range is
    non-empty (the read is not split)."""
    live = [(int(b), int(e)) for b, e in ranges if e > b]
    if not live:
        return []
    tl = max(int(tl), 0)
    cut = np.zeros(tl + 2, bool)            # positions 1 .. tl stand for 0 .. tl - 1; the ends stay cut
    cut[0] = cut[tl + 1] = True
    for b, e in live:
        b, e = min(max(b, 0), tl), min(max(e, 0), tl)
        if e > b:
            cut[1 + b:1 + e] = True
    edge = np.diff(cut.astype(np.int8))
    return list(zip((np.nonzero(edge == -1)[0]).tolist(), (np.nonzero(edge == 1)[0]).tolist()))


def read_ranges(cut_off, cuts, r):
    return [(int(cuts[2 * k]), int(cuts[2 * k + 1])) for k in range(int(cut_off[r]), int(cut_off[r + 1]))]


def stage(qual, span_off, span_len, cut_off, cuts, o):
    """-> (pieces [(read, begin, end, (front, tail, kept, flags, q_sum, err_sum))], piece_off, cut_off', cuts')"""
    pieces, piece_off, cut_off2, cuts2 = [], [0], [0], []
    for r in range(len(span_len)):
        ranges = read_ranges(cut_off, cuts, r)
        for b, e in ranges:
            cuts2 += [b, e]
        off = int(span_off[r])
        for b, e in pieces_of(int(span_len[r]), ranges):
            rec = R.read_record(qual, off + b if off >= 0 else off, e - b, o)
            pieces.append((r, b, e, rec))
            if rec[3] & R.FAIL:
                cuts2 += [b, e, e, e]
            else:
                cuts2 += [b, b + rec[0], e - rec[1], e]
        piece_off.append(len(pieces))
        cut_off2.append(len(cuts2) // 2)
    return pieces, piece_off, cut_off2, cuts2


def as_tuples(pieces):
    """engine.QUAL_PIECE records as stage()'s tuples."""
    return [(int(p['read']), int(p['begin']), int(p['end']), R.as_tuples([p['q']])[0]) for p in pieces]


def numbered(name, k):
    """add_number_to_read_name: _k goes behind the name's first word."""
    for sep in ('\t', ' '):
        if sep in name:
            p = name.index(sep)
            return name[:p] + '_%d' % k + name[p:]
    return name + '_%d' % k


def written_spans(name, n_seq, st, et, ranges, judged, min_split, keep=True):
    """The (name, first base, length) records the writers emit for one read of n_seq bases of a
    quality_per_piece run: st / et its trims, ranges its middle cuts, judged [(begin, end, record)] its pieces
    by stage(). A read that is not split is written whole when keep is set."""
    a, b = R.py_span(n_seq, st, et)
    if not any(e > s for s, e in ranges):
        return [(name, a, b - a)] if keep and b > a else []
    out = []
    if not keep:
        return out
    for s, e, rec in judged:
        if rec[3] & R.FAIL:
            continue
        s, e = s + rec[0], e - rec[1]
        if e - s <= 0 or e - s < min_split:
            continue
        out.append((numbered(name, len(out) + 1), a + s, e - s))
    return out


def written(name, seq, qual, st, et, ranges, judged, min_split, keep=True):
    """written_spans as (name, sequence, qualities)."""
    return [(nm, seq[s:s + n], qual[s:s + n]) for nm, s, n in written_spans(name, len(seq), st, et, ranges, judged, min_split, keep)]


# ---- the inputs --------------------------------------------------------------------------------------------
def option_sets():
    """W in {0, 1, 5, 64}, with and without each limit (integers, as the library takes them)."""
    sets = []
    for W, mn, mx, mq in ((0, 0, 0, 0.0), (0, 300, 6000, 12.0), (1, 0, 0, 0.0), (1, 0, 6000, 0.0), (5, 300, 0, 0.0), (5, 0, 0, 12.0),
                          (5, 300, 6000, 12.0), (64, 0, 0, 0.0), (64, 300, 6000, 12.0)):
        sets.append(R.to_ints(W, 15.0, mn, mx, mq))
    return sets


def _random_ranges(rng, tl, m):
    """m ranges around a read of tl positions in the kinds the rule names."""
    out = []
    for _ in range(m):
        kind = int(rng.randint(0, 12))
        a = int(rng.randint(0, tl + 1))
        ln = int(rng.randint(1, max(2, tl // 6 + 2)))
        if kind == 0:
            rg = (a, a)                                         # empty
        elif kind == 1:
            rg = (a + ln, a)                                    # end below begin: empty
        elif kind == 2:
            rg = (-int(rng.randint(1, 300)), int(rng.randint(0, min(tl, 200) + 1)))          # begins below 0
        elif kind == 3:
            rg = (max(tl - int(rng.randint(0, 200)), 0), tl + int(rng.randint(1, 300)))      # ends beyond tl
        elif kind == 4:
            rg = (tl + int(rng.randint(0, 50)), tl + int(rng.randint(51, 90))) if rng.randint(0, 2) else \
                (-int(rng.randint(51, 90)), -int(rng.randint(0, 50)))                       # wholly outside
        elif kind == 5 and out:
            rg = out[int(rng.randint(0, len(out)))]             # duplicate
        elif kind == 6 and out:
            b, e = out[int(rng.randint(0, len(out)))]
            rg = (e, e + ln)                                    # adjacent
        elif kind == 7 and out:
            b, e = out[int(rng.randint(0, len(out)))]
            rg = (b + (e - b) // 3, e - (e - b) // 3)           # nested
        elif kind == 8 and out:
            b, e = out[int(rng.randint(0, len(out)))]
            rg = ((b + e) // 2, e + ln)                         # overlapping
        elif kind == 9 and rng.randint(0, 6) == 0:
            rg = (-int(rng.randint(0, 3)), tl + int(rng.randint(0, 3)))                      # the whole read
        else:
            rg = (a, a + ln)
        out.append(rg)
    return out


@functools.lru_cache(maxsize=None)
def fuzz_batch(n_reads=3000, seed=5):
    """About 3,000 reads of 0..20,000 qualities with 0..12 ranges each, in any order: low qualities beside
    about half of the ranges' ends, some reads without qualities. -> (blob, span_off, span_len, cut_off, cuts)"""
    rng = np.random.RandomState(seed)
    b = R.Blob()
    cut_off, cuts = [0], []
    for i in range(n_reads):
        n = int(rng.randint(0, 20001)) if i % 7 else int(rng.randint(0, 200))
        ranges = _random_ranges(rng, n, int(rng.randint(0, 13))) if i % 3 else []
        if i % 11 == 10:
            b.add_none(n)
        else:
            q = rng.randint(33 + 8, 33 + 40, n).astype(np.uint8)
            for s, e in ranges:
                if rng.randint(0, 2):
                    lo, hi = max(min(s, n) - int(rng.randint(0, 90)), 0), max(min(e, n), 0) + int(rng.randint(0, 90))
                    q[lo:hi] = rng.randint(33, 33 + 6, max(min(hi, n) - lo, 0))
            b.add(q.tobytes(), gap=int(rng.randint(0, 4)))
        for s, e in ranges:
            cuts += [s, e]
        cut_off.append(len(cuts) // 2)
    qual, off, ln = b.arrays()
    return qual, off, ln, np.array(cut_off, np.int64), np.array(cuts, np.int64)


def _batch(reads):
    """reads: [(quality bytes or an int for a read without qualities, ranges)]"""
    b = R.Blob()
    cut_off, cuts = [0], []
    for q, ranges in reads:
        if isinstance(q, int):
            b.add_none(q)
        else:
            b.add(bytes(bytearray(q)))
        for s, e in ranges:
            cuts += [s, e]
        cut_off.append(len(cuts) // 2)
    qual, off, ln = b.arrays()
    return qual, off, ln, np.array(cut_off, np.int64), np.array(cuts, np.int64)


@functools.lru_cache(maxsize=None)
def crafted_cases():
    """-> [(name, opts as integers, blob, span_off, span_len, cut_off, cuts)]"""
    G, B = R.GOOD, R.BAD
    cases = []
    rng = np.random.RandomState(17)
    # one read with 300 ranges, shuffled, some overlapping, low qualities beside some
    n = 60000
    q = rng.randint(33 + 20, 33 + 40, n).astype(np.uint8)
    ranges = []
    for k in range(300):
        s = 150 + 199 * k
        ranges.append((s, s + int(rng.randint(1, 120))))
        if k % 4 == 0:
            q[ranges[-1][1]:ranges[-1][1] + 30] = B
    rng.shuffle(ranges)
    cases.append(('300 ranges', R.to_ints(5, 15.0, 90, 0, 10.0)) + _batch([(q.tolist(), ranges)]))
    # pieces of exactly W - 1, W, 4095, 4096, 4097 and 8192 bytes between 10-base cuts
    for W in (5, 64):
        sizes = [W - 1, W, 4095, 4096, 4097, 8192, W - 1, W]
        q, ranges = [], []
        for k, sz in enumerate(sizes):
            q += ([G] * sz if k % 2 == 0 else [B] * 3 + [G] * (sz - 6) + [B] * 3 if sz > 64 else [B] + [G] * (sz - 2) + [B]) + [B] * 10
            ranges.append((len(q) - 10, len(q)))
        cases.append(('piece sizes W%d' % W, R.to_ints(W, 15.0, W, 8191, 3.0)) + _batch([(q, ranges[::-1])]))
    # a first piece starting at 0 and a last one ending at tl, after a whole-read crop with the same options
    W = 5
    o = R.to_ints(W, 15.0, 0, 0, 0.0)
    raw = [B] * 37 + [G] * 400 + [B] * 20 + [G] * 300 + [B] * 41
    front, tail, kept = R.read_record(np.array(raw, np.uint8), 0, len(raw), o)[:3]
    assert 0 < front <= 37 and 0 < tail <= 41
    island = 37 - front + 400                                            # the 20 bad bases inside the cropped read
    cases.append(('after the whole-read crop', o) + _batch([(raw[front:front + kept], [(island + 5, island + 15)])]))
    return cases


@functools.lru_cache(maxsize=None)
def equality_cases():
    """An equality case for each threshold, on the piece: -> [(name, opts, blob, span_off, span_len, cut_off,
    cuts, expected pass per piece)]. The read is 120 + 10 + 120 bytes of Phred 10 with its middle 10 cut."""
    out = []
    arrays = _batch([([33 + 10] * 250, [(120, 130)])])
    for mn, mx, ok in ((120, 0, True), (121, 0, False), (0, 120, True), (0, 119, False)):
        out.append(('len %d %d' % (mn, mx), dict(R.to_ints(), min_length=mn, max_length=mx)) + arrays + ([ok, ok],))
    for d, ok in ((0, True), (-1, False)):
        out.append(('err %+d' % d, dict(R.to_ints(), max_mean_err=R.ERR[10] + d)) + arrays + ([ok, ok],))
    # the window sum: a piece whose only window reaches min_window_sum exactly, and one that is one short
    W = 4
    q = [33 + 20] * W + [33] * 10 + [33 + 20] * (W - 1) + [33 + 19]
    out.append(('window sum', R.to_ints(W, 20.0, 1, 0, 0.0)) + _batch([(q, [(W, W + 10)])]) + ([True, False],))
    return out
