"""The quality stage's rule (include/pcabi.h pcabi_qual_*) restated in plain Python: slicing, clamping,
windows by brute force, sums with Python integers; and the small shapes at which the rule can go wrong
(tests/test_qual_cpu.py runs them on the host build, tests/test_gpu_qual.py on the device)."""
import functools
import math

import numpy as np

TOO_SHORT, TOO_LONG, LOW_QUALITY, NO_QUALITIES = 1, 2, 4, 8
FAIL = TOO_SHORT | TOO_LONG | LOW_QUALITY
ERR = [round(2 ** 32 * 10 ** (-q / 10)) for q in range(94)]
SEG = 4096


def to_ints(window=0, min_window_q=0.0, min_length=0, max_length=0, min_mean_q=0.0):
    """The thresholds as integers, as the issue defines them."""
    return {'window': int(window), 'min_window_sum': int(math.ceil(min_window_q * window)), 'min_length': int(min_length),
            'max_length': int(max_length),
            'max_mean_err': 2 ** 32 if min_mean_q <= 0 else int(math.floor(2 ** 32 * 10 ** (-min_mean_q / 10)))}


def py_span(ns, st, et):
    """What the writers' slice seq[st:ns - et] keeps, as [a, b); st == et == 0: the whole read."""
    if st == 0 and et == 0:
        return 0, ns
    a, b, _ = slice(st, ns - et).indices(ns)
    return a, max(a, b)


def read_record(qual, off, n, o):
    """(front, tail, kept, flags, q_sum, err_sum) of one span; off < 0: a read without qualities."""
    W, has_q = o['window'], off >= 0
    front = tail = 0
    q = np.clip(np.asarray(qual[off:off + n], np.int64) - 33, 0, 93) if has_q else None
    if W > 0 and has_q:
        # every window's sum, each from its own W values
        sums = np.lib.stride_tricks.sliding_window_view(q, W).sum(axis=1) if n >= W else np.zeros(0, np.int64)
        good = np.nonzero(sums >= o['min_window_sum'])[0]
        if good.size:
            front, tail = int(good[0]), n - (int(good[-1]) + W)
        else:
            front, tail = n, 0
    kept = n - front - tail
    q_sum = err_sum = 0
    if has_q:
        count = np.bincount(q[front:front + kept], minlength=94)
        q_sum = sum(int(c) * k for k, c in enumerate(count))
        err_sum = sum(int(c) * ERR[k] for k, c in enumerate(count))
    flags = 0 if has_q else NO_QUALITIES
    if kept < o['min_length']:
        flags |= TOO_SHORT
    if o['max_length'] > 0 and kept > o['max_length']:
        flags |= TOO_LONG
    if has_q and err_sum > kept * o['max_mean_err']:
        flags |= LOW_QUALITY
    return front, tail, kept, flags, q_sum, err_sum


def records(qual, span_off, span_len, o):
    return [read_record(qual, int(a), int(n), o) for a, n in zip(span_off, span_len)]


def new_trims(ns, st, et, front, tail):
    """The trims handed on for a read of ns bases with adapter trims st / et."""
    if front + tail == 0:
        return st, et
    a, b = py_span(ns, st, et)
    return a + front, ns - (b - tail)


def as_tuples(recs):
    return [tuple(int(r[k]) for k in ('front', 'tail', 'kept', 'flags', 'q_sum', 'err_sum')) for r in recs]


# ---- the cases ---------------------------------------------------------------------------------------------
GOOD, BAD = 33 + 30, 33 + 2


class Blob(object):
    """Spans laid into one blob between filler bytes that alternate 0xFF and 0x00 (a read outside a span
    changes a sum); a span's first byte at a chosen alignment."""

    def __init__(self):
        self.bytes, self.off, self.len, self.k = bytearray(), [], [], 0

    def _fill(self, n):
        for _ in range(n):
            self.bytes.append(0xFF if self.k % 2 == 0 else 0x00)
            self.k += 1

    def add(self, q, align=None, gap=3):
        self._fill(gap)
        if align is not None:
            self._fill((align - len(self.bytes)) % 16)
        self.off.append(len(self.bytes))
        self.len.append(len(q))
        self.bytes += bytes(q)

    def add_none(self, n):
        self.off.append(-1)
        self.len.append(n)

    def arrays(self, tail_fill=5):
        if tail_fill:
            self._fill(tail_fill)
        return np.frombuffer(bytes(self.bytes), np.uint8), np.array(self.off, np.int64), np.array(self.len, np.int32)


def with_good(n, W, at, good=GOOD, bad=BAD):
    """n bad bytes with W good ones from each position of `at` on."""
    q = [bad] * n
    for p in at:
        q[p:p + W] = [good] * W
    return q[:n]


@functools.lru_cache(maxsize=None)
def crop_cases():
    """-> [(name, opts as integers, blob, span_off, span_len)]"""
    cases = []
    for W in (1, 4, 63, 64):
        o = dict(to_ints(W, 20.0), min_length=0)
        b = Blob()
        for n in sorted({0, 1, W - 1, W, W + 1}):                      # span length against the window
            b.add([GOOD] * n)
            b.add([BAD] * n)
        L = 400
        for p in (0, 63, 64, 65, 127, 128):                              # the first / the last good window
            b.add(with_good(L, W, [p, L - W]))                           #   front at p
            b.add(with_good(L, W, [0, L - W - p]))                       #   tail mirrored
            b.add(with_good(L, W, [p]))                                  #   exactly one: f == g
            b.add(with_good(L, W, [L - W - p]))
        b.add([BAD] * L)                                                 # no good window
        b.add(with_good(100, W, [10, 10 + max(1, W // 2)]))              # front and tail windows overlap
        # a window one short of the sum, beside one that reaches it exactly
        exact = [33] * 50 + [33 + 20] * W + [33] * 50
        b.add(exact)
        if W > 1:
            b.add([33] * 50 + [33 + 20] * (W - 1) + [33 + 19] + [33] * 50)
        else:
            b.add([33] * 50 + [33 + 19] + [33] * 50)
        cases.append(('W%d' % W, o, ) + b.arrays())
    # window = 0 with only the filters on
    b = Blob()
    for n in (0, 1, 99, 100, 101, 199, 200, 201):
        b.add([33 + 15] * n)
    b.add([33 + 9] * 150)
    b.add([33 + 10] * 150)
    cases.append(('filters only', to_ints(0, 0.0, 100, 200, 10.0)) + b.arrays())
    # every byte alignment of the blob; the last span ends at the blob's last byte
    rng = np.random.RandomState(11)
    b = Blob()
    for al in range(16):
        for n in (1, 15, 16, 17, 100 + al):
            b.add(rng.randint(33, 80, n).tolist(), align=al)
    b.add(rng.randint(33, 80, 333).tolist(), align=7)
    cases.append(('alignments', to_ints(8, 12.0, 10, 0, 7.0)) + b.arrays(tail_fill=0))
    # kept lengths across segment boundaries, one long read with a low-quality island, runs of kept = 0
    b = Blob()
    dead = [BAD] * 70
    for _ in range(3):
        b.add(dead)
    for k, kept in enumerate((4095, 4096, 4097, 8193)):
        b.add([BAD] * (5 + k) + rng.randint(33 + 30, 33 + 32, kept).tolist() + [BAD] * (9 - k), align=(5 * k + 1) % 16)
        if k == 1:
            for _ in range(3):
                b.add(dead)
    island = rng.randint(33 + 30, 33 + 32, 70000)
    island[30000:30300] = BAD
    b.add([BAD] * 200 + island.tolist() + [BAD] * 130, align=9)
    for _ in range(3):
        b.add(dead)
    # (only a window of 16 good values reaches 480: 15 of them and a bad one give 467 at most)
    cases.append(('segments', to_ints(16, 30.0, 1, 0, 12.0)) + b.arrays())
    # the bytes at the clamp's edges, and reads without qualities between reads with them
    b = Blob()
    edge = [0, 32, 33, 126, 127, 255]
    b.add(edge * 20)
    b.add_none(50)
    b.add([126, 127, 255] * 30 + [0, 32, 33] * 30)
    b.add_none(0)
    b.add_none(5000)
    b.add([0, 32, 33] * 30 + [255] * 10 + [0] * 7)
    b.add_none(3)
    cases.append(('bytes', to_ints(4, 40.0, 4, 4999, 3.0)) + b.arrays())
    return cases


@functools.lru_cache(maxsize=None)
def equality_cases():
    """-> [(name, opts as integers, blob, span_off, span_len, expected pass)]"""
    out = []
    for Q in (0, 7, 20, 93):
        b = Blob()
        b.add([33 + Q] * 777)
        arrays = b.arrays()
        for d, ok in ((0, True), (-1, False)):
            if ERR[Q] + d < 0:
                continue
            o = dict(to_ints(), max_mean_err=ERR[Q] + d)
            out.append(('Q%d%+d' % (Q, d), o) + arrays + ([ok],))
    b = Blob()
    b.add([33 + 10] * 120)
    arrays = b.arrays()
    for mn, mx, ok in ((120, 0, True), (121, 0, False), (119, 0, True), (0, 120, True), (0, 119, False), (0, 121, True)):
        out.append(('len %d %d' % (mn, mx), dict(to_ints(), min_length=mn, max_length=mx)) + arrays + ([ok],))
    return out


@functools.lru_cache(maxsize=None)
def random_batch(n_reads=2000, seed=3):
    """Reads of 0..9000 bases: about a third with ends of Phred 0..4 (they crop: no window of such values
    reaches 50), about a third of Phred 6..13 throughout (no crop, as every window reaches 60, and a mean
    error of about Q9: they fail), some without qualities. -> (opts, blob, span_off, span_len)"""
    rng = np.random.RandomState(seed)
    b = Blob()
    for i in range(n_reads):
        n = int(rng.randint(0, 9001))
        kind = rng.randint(0, 10)
        if kind == 9:
            b.add_none(n)
            continue
        q = rng.randint(33 + 18, 33 + 40, n)
        if kind < 3:
            h, t = int(rng.randint(0, 200)), int(rng.randint(0, 200))
            q[:h] = rng.randint(33, 33 + 5, min(h, n))
            q[max(n - t, 0):] = rng.randint(33, 33 + 5, n - max(n - t, 0))
        elif kind < 6:
            q = rng.randint(33 + 6, 33 + 14, n)
        b.add(q.tolist(), gap=int(rng.randint(0, 4)))
    return (to_ints(10, 5.0, 500, 8500, 10.0),) + b.arrays()
