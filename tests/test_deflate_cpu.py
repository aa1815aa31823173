"""The gzip encoder's device-free parts (csrc/pcabi_deflate.h, built for the host by
tests/deflate_cpu_lib.py): the length-limited code construction the kernel's lane runs, the dynamic
block header plan and the writer's block planner. A Python bit-writer assembles a block from the
lengths alone; zlib must decode it and its size must be the predicted one. No GPU."""
import zlib

import numpy as np
import pytest

from tests import deflate_cpu_lib as D


class BitWriter(object):
    """LSB-first bit stream, as RFC 1951 packs it."""

    def __init__(self):
        self.acc, self.k, self.nbits, self.out = 0, 0, 0, bytearray()

    def put(self, v, n):
        v, n = int(v), int(n)
        assert 0 <= v < (1 << n) or (n == 0 and v == 0)
        self.acc |= v << self.k
        self.k += n
        self.nbits += n
        while self.k >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.k -= 8

    def align(self):
        if self.k:
            self.put(0, 8 - self.k)

    def bytes(self):
        assert self.k == 0
        return bytes(self.out)


def fib(n):
    a, b, out = 1, 1, []
    for _ in range(n):
        out.append(a)
        a, b = b, a + b
    return out


def data_of(counts, rng):
    vals = np.repeat(np.arange(256, dtype=np.uint8), counts)
    rng.shuffle(vals)
    return vals.tobytes()


def histograms():
    rng = np.random.default_rng(5)
    out = {}
    c = np.zeros(256, np.int64)
    c[65] = 1
    out['one_symbol_once'] = c.copy()
    c[65] = 40000
    out['one_symbol_many'] = c.copy()
    c = np.zeros(256, np.int64)
    c[[0, 255]] = [3, 60000]
    out['two_symbols'] = c
    out['all_equal'] = np.full(256, 255, np.int64)
    out['all_once'] = np.ones(256, np.int64)
    c = np.zeros(256, np.int64)
    c[rng.permutation(256)[:22]] = fib(22)            # 46,367 bytes, unlimited depth 21
    assert c.sum() == 46367
    out['fibonacci22'] = c
    c = np.zeros(256, np.int64)
    c[rng.permutation(256)[:23]] = fib(23)[::-1]      # 75,024 would pass the cap: 23 values scaled down
    c = np.maximum(1, c * 65535 // (c.sum() + 23)) * (c > 0)
    out['fibonacci23_scaled'] = c
    c = np.zeros(256, np.int64)
    c[rng.permutation(256)[:20]] = np.floor(25000 * 0.6 ** np.arange(20)).astype(np.int64)
    out['geometric06'] = c                            # ratio below the golden one: a chain, depth 20
    for k in range(6):
        out['random%d' % k] = rng.integers(0, 200, 256) * (rng.random(256) < rng.random())
    for k in range(4):
        g = np.floor(30000 * 0.5 ** (np.arange(256) / (k + 1.0))).astype(np.int64)
        out['skewed%d' % k] = g[rng.permutation(256)]
    c = np.zeros(256, np.int64)
    c[[65, 67, 71, 84]] = [2000, 2100, 1900, 2050]
    c[10] = 1
    c[[64, 48, 49, 50, 45]] = [1, 3, 2, 2, 4]
    out['sequence_line'] = c
    c = np.zeros(256, np.int64)
    c[38:73] = rng.multinomial(8000, np.full(35, 1 / 35.0))
    c[10] = 1
    out['quality_line'] = c
    return {k: v for k, v in out.items() if 0 < v.sum() <= 65535}


HISTS = histograms()


def test_histograms_cover_the_cases():
    assert {'one_symbol_once', 'two_symbols', 'fibonacci22', 'fibonacci23_scaled', 'geometric06', 'all_equal', 'random0',
            'skewed0'} <= set(HISTS)


@pytest.mark.parametrize('name', sorted(HISTS))
def test_code_lengths_and_block(name):
    cnt = HISTS[name]
    p = D.plan_block(cnt)
    lit, cl = p['lit_len'].astype(int), p['cl_len'].astype(int)
    used = np.concatenate([cnt > 0, [True]])
    assert np.all((lit[used] >= 1) & (lit[used] <= 15)) and np.all(lit[~used] == 0)
    assert sum(2 ** (15 - l) for l in lit[used]) == 2 ** 15          # complete: Kraft sum exactly 1
    # the code-length code: the lengths sent are the 257 above and the distance code's single 1
    sent = np.concatenate([lit, [1]])
    cl_used = np.bincount(sent, minlength=19) > 0
    assert np.all((cl[cl_used] >= 1) & (cl[cl_used] <= 7)) and np.all(cl[~cl_used] == 0)
    assert sum(2 ** (7 - l) for l in cl[cl_used]) == 2 ** 7
    assert 4 <= p['hclen4'] <= 19
    order = D.cl_order()
    assert all(cl[order[i]] == 0 for i in range(p['hclen4'], 19))
    # a block assembled from the lengths alone
    data = data_of(cnt, np.random.default_rng(1))
    lit_code = D.codes(lit, 15).astype(int)
    assert np.array_equal(D.codes(cl, 7), p['cl_code'])
    cl_code = p['cl_code'].astype(int)
    w = BitWriter()
    w.put(0, 1)
    w.put(2, 2)
    w.put(0, 5)
    w.put(0, 5)
    w.put(p['hclen4'] - 4, 4)
    for i in range(p['hclen4']):
        w.put(cl[order[i]], 3)
    for l in sent:
        w.put(cl_code[l], cl[l])
    assert w.nbits == p['hdr_bits']
    for c in data:
        w.put(lit_code[c], lit[c])
    w.put(lit_code[256], lit[256])
    assert w.nbits == p['block_bits']
    w.put(0, 3)
    w.align()
    for c in (0, 0, 0xff, 0xff):
        w.put(c, 8)
    blob = w.bytes()
    assert len(blob) == D.load().dfl_dyn_bytes(p['block_bits'])
    d = zlib.decompressobj(-15)
    assert d.decompress(blob + b'\x03\x00') == data
    assert d.eof and d.unused_data == b''
    # the unlimited code is deeper than 15 bits here: the limiter had work to do
    if name == 'geometric06':
        assert unlimited_depth(np.concatenate([cnt, [1]])) > 15 and lit[used].max() == 15


def unlimited_depth(cnt):
    import heapq
    h = [(int(v), 0) for v in cnt if v]
    heapq.heapify(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1))
    return h[0][1]


def test_stored_size():
    assert D.load().dfl_stored_bytes(65535) == 65540 and D.load().dfl_stored_bytes(1) == 6


def fastq_text(rng, lens, name_len=40):
    parts = []
    for k, n in enumerate(lens):
        name = ('read%d ' % k).ljust(name_len, 'x')
        seq = ''.join('ACGT'[i] for i in rng.integers(0, 4, n))
        qual = ''.join(chr(33 + i) for i in rng.integers(5, 40, n))
        parts.append('@%s\n%s\n+\n%s\n' % (name, seq, qual))
    return ''.join(parts).encode()


def planner_texts():
    rng = np.random.default_rng(9)
    out = {
        'empty': b'',
        'one_byte': b'A',
        'no_newline': b'ACGT' * 5000,
        'long_reads': fastq_text(rng, [8000, 12000, 300, 1023, 1024, 1022, 70000, 140000, 5, 9000]),
        'short_reads': fastq_text(rng, [200] * 900),
        'fasta70': b''.join(b'>r%d\n' % k + b'\n'.join([b'ACGTACGTAC' * 7] * 30) + b'\n' for k in range(60)),
        'newlines': b'\n' * 70000,
        'long_then_eof': b'@r\n' + b'A' * 66000,
    }
    return out


TEXTS = planner_texts()


@pytest.mark.parametrize('name', sorted(TEXTS))
@pytest.mark.parametrize('long_line,cap', [(1024, 65535), (64, 100), (1, 1)])
def test_planner(name, long_line, cap):
    text = TEXTS[name]
    off = D.plan_lines(text, long_line, cap)
    assert off[0] == 0 and off[-1] == len(text)
    sizes = np.diff(off)
    assert np.all(sizes >= 1) and np.all(sizes <= cap)             # ascending, 1..cap bytes each
    assert (len(off) == 1) == (len(text) == 0)
    # the end of every line of long_line bytes or more (its '\n' included) is a block boundary
    ends = set(off.tolist())
    pos = 0
    for line in text.split(b'\n')[:-1]:
        end = pos + len(line) + 1
        if end - pos >= long_line:
            assert end in ends, (pos, end)
        pos = end
    if name == 'long_reads' and cap == 65535:
        # short lines ride with the long line after them: "@name\nSEQ\n" and "+\nQUAL\n" are one block each
        assert off[1] == 1 + 40 + 1 + 8000 + 1 and off[2] == off[1] + 2 + 8000 + 1
    if name == 'short_reads' and cap == 65535:
        assert np.all(sizes[:-1] > 65535 - 256)                    # short lines fill blocks up to the cap
