"""Crafted inputs for the k-mer kernels (TEST INFRASTRUCTURE ONLY), shared by tests/test_kmer_core_cpu.py
(csrc/pcabi_kmer.h through the host model) and tests/test_gpu_kmer.py (the entry points on the device).
A case is a packed sequence set in the entry points' layout (Dna5 codes, 4-aligned starts) plus
arguments; what to expect always comes from tests/kmer_oracle.py, never from the library.
test_kmer_core_cpu.py::test_cases_cover_what_they_promise asserts, from the restatement, that the
cases hold what this file says they hold."""
import numpy as np

from tests import kmer_oracle as O

N = 4
APPROX_K = (4, 5, 8, 16, 31, 32)
# (sequences, k-mers): around the 32 sequences a block walks (97: four blocks add into one count) and
# the 64 k-mers of a lane group
APPROX_SHAPES = ((1, 1), (31, 63), (32, 64), (33, 65), (97, 130))
EXACT_K = (2, 3, 4, 15, 16, 31, 32)
IDX_N, IDX_PAD = 5, 6          # the sequences of an approximate case with an N in the copy / bases as padding
MAX_LEN = 72                   # approximate cases: every length below this


class Pack(object):
    """Sequences in the engine layout, as approx_counter.Samples holds them."""

    def __init__(self, codes, offs, lens):
        self.codes, self.offs, self.lens = codes, offs, lens

    def __len__(self):
        return len(self.lens)

    def seq(self, i):
        return self.codes[int(self.offs[i]):int(self.offs[i]) + int(self.lens[i])]


def pack(seqs, rng=None, pads=None):
    """4-aligned starts. The bytes up to the next start are N, or random base codes when rng is given,
    or begin with pads[i]; 16 bytes of N close the buffer."""
    ln = np.array([len(s) for s in seqs], np.int64)
    offs = np.zeros(len(seqs), np.int64)
    if len(seqs):
        offs[1:] = np.cumsum((ln + 3) & ~3)[:-1]
    total = int(offs[-1] + ((ln[-1] + 3) & ~3)) if len(seqs) else 0
    codes = np.full(total + 16, N, np.uint8)
    if rng is not None:
        codes[:total] = rng.integers(0, 4, total)
    for i, s in enumerate(seqs):
        a = int(offs[i])
        codes[a:a + len(s)] = s
        p = (pads or {}).get(i)
        if p is not None:
            assert len(s) + len(p) <= (len(s) + 3) & ~3
            codes[a + len(s):a + len(s) + len(p)] = p
    return Pack(codes, offs, ln.astype(np.int32))


def same(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.argwhere(got != exp)
    assert not len(bad), (what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])


def kmer_codes(v, k):
    return np.array([(int(v) >> (2 * (k - 1 - i))) & 3 for i in range(k)], np.uint8)


def kmer_value(codes):
    v = 0
    for x in codes.tolist():
        v = (v << 2) | int(x)
    return v


def _edit(rng, codes, n_edits):
    """n_edits random substitutions, insertions and deletions (they may cancel: the distance is the DP's)."""
    s = codes.tolist()
    for _ in range(n_edits):
        kind = int(rng.integers(0, 3))
        p = int(rng.integers(0, len(s)))
        if kind == 0:
            s[p] = (s[p] + int(rng.integers(1, 4))) & 3
        elif kind == 1:
            s.insert(p, int(rng.integers(0, 4)))
        elif len(s) > 1:
            del s[p]
    return np.array(s, np.uint8)


def pad_prefix_len(k):
    """The longest proper prefix of a k-mer that does not fill its last dword."""
    return k - 1 if (k - 1) % 4 else k - 2


def approx_case(k, n_seq, n_kmers, seed=0):
    """Sequence i carries a copy of a listed k-mer with i % 5 edits (4: no copy), at its start, ending
    on its last base, or starting two bases into a dword, by (i // 5) % 3. Lengths: 0, 1, k - 1, k, k + 1,
    then every length from 2 to MAX_LEN - 1, then random ones. Sequence IDX_N is k-mer 0 with its middle base an N
    (d = 1); sequence IDX_PAD is the longest prefix of k-mer 0 that leaves its dword open, the k-mer's
    next bases being the padding (d = k - its length; a walk that runs to the dword's end finds less).
    All other padding is random base codes too. The list holds TTT...T, AAA...A and one k-mer twice."""
    rng = np.random.default_rng(1000 * k + 10 * n_seq + seed)
    kmers = [kmer_value(rng.integers(0, 4, k)) for _ in range(n_kmers)]
    if n_kmers >= 4:
        kmers[1], kmers[2] = 4 ** k - 1, 0
    if n_kmers >= 2:
        kmers[-1] = kmers[0]
    lens = [0, 1, k - 1, k, k + 1, k, k] + list(range(2, MAX_LEN))
    if n_seq == 1:
        lens = [k + 2 + seed % 4]
    lens = (lens + [int(x) for x in rng.integers(k, MAX_LEN, max(0, n_seq - len(lens)))])[:n_seq]
    seqs, plants = [], []
    for i, n in enumerate(lens):
        s = rng.integers(0, 4, n).astype(np.uint8)
        if n and rng.random() < 0.3:
            s[int(rng.integers(0, n))] = N
        edits, place = i % 5, (i // 5) % 3
        if edits < 4:
            q = int(rng.integers(0, n_kmers))
            c = _edit(rng, kmer_codes(kmers[q], k), edits)
            if len(c) <= n:
                p = (0, n - len(c), min(2 + 4 * int(rng.integers(0, 4)), n - len(c)))[place]
                s[p:p + len(c)] = c
                plants.append((i, q, edits, place, p, len(c)))
        seqs.append(s)
    pads = {}
    if n_seq > IDX_PAD:
        first = kmer_codes(kmers[0], k)
        seqs[IDX_N] = first.copy()
        seqs[IDX_N][k // 2] = N
        m = pad_prefix_len(k)
        seqs[IDX_PAD] = first[:m].copy()
        pads[IDX_PAD] = first[m:(m + 3) & ~3]
    return dict(name='approx-k%d-%dx%d' % (k, n_seq, n_kmers), k=k, pack=pack(seqs, rng, pads),
                kmers=np.array(kmers, np.uint64), plants=plants)


def approx_cases():
    return [approx_case(k, s, q) for k in APPROX_K for s, q in APPROX_SHAPES]


def random_approx_case(k, seed):
    """Seeded random k-mers and texts with planted copies, at one k (the CPU test's Myers check)."""
    return approx_case(k, 97, 40, seed=seed + 1)


def _rand(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def exact_sets(k):
    """'main': lengths 0, k - 1, k, k + 1, 129, 257 (a block's 128 lanes stride twice and three times);
    one N at position k of 2 k + 3 bases (the last base of window 1, the first of window k); a run of
    five N; a sequence of N alone; AAA...A of 257 and 129 bases (one k-mer 300 times or more);
    TTT...T of 257; one random sequence three times and a second one twice (equal counts).
    'clean': no N and nothing shorter than k, TTT...T the largest key -- with threshold inf no position
    is skipped.  'short': every sequence shorter than k.  'none': no sequence."""
    rng = np.random.default_rng(77 + k)
    one_n = _rand(rng, 2 * k + 3)
    one_n[k] = N
    run_n = _rand(rng, 3 * k + 5)
    run_n[k + 1:k + 6] = N
    rep, rep2 = _rand(rng, 129), _rand(rng, 70)
    main = [_rand(rng, 0), _rand(rng, k - 1), _rand(rng, k), _rand(rng, k + 1), _rand(rng, 129), _rand(rng, 257),
            one_n, run_n, np.full(k + 2, N, np.uint8), np.zeros(257, np.uint8), np.zeros(129, np.uint8),
            np.full(257, 3, np.uint8), rep, rep2, rep.copy(), rep2.copy(), rep.copy()]
    clean = [np.full(60, 3, np.uint8), _rand(rng, 129), np.concatenate([np.full(k, 3, np.uint8), _rand(rng, 40)]),
             _rand(rng, k)]
    short = [_rand(rng, n) for n in range(k)]
    return dict(main=pack(main), clean=pack(clean), short=pack(short), none=pack([]))


def exact_cases(k):
    """Thresholds inf, 0 (every position of a k-mer with a score is skipped), one equal to a score that
    occurs, and 16 at k >= 31 (above TTT...T's score). Forbidden sets: none, the most frequent k-mer,
    the smallest and the largest k-mer present, and up to 1000 entries of which 40 are present."""
    sets = exact_sets(k)
    p = sets['main']
    v, dna = O.window_values(p, k)
    present, cnt = np.unique(v[dna], return_counts=True)
    score = O.dimer_score(present, k)
    finite = np.unique(score[np.isfinite(score)])   # the middle one of the distinct scores
    eq = float(finite[len(finite) // 2]) if len(finite) else 1.0
    rng = np.random.default_rng(99 + k)
    some = present[rng.permutation(len(present))[:40]]
    many = np.unique(np.concatenate([some, np.array([kmer_value(_rand(rng, k)) for _ in range(960)], np.uint64)]))
    none = np.zeros(0, np.uint64)
    inf = float('inf')
    out = [('inf', p, inf, none), ('zero', p, 0.0, none), ('eq', p, eq, none),
           ('forbid-one', p, inf, present[np.argmax(cnt)][None]),
           ('eq-forbid-minmax', p, eq, np.array([present[0], present[-1]], np.uint64)),
           ('forbid-many', p, inf, many), ('eq-forbid-many', p, eq, many),
           ('clean', sets['clean'], inf, none), ('short', sets['short'], inf, none), ('none', sets['none'], inf, none)]
    if k >= 31:
        out += [('sixteen', p, 16.0, none), ('sixteen-forbid-minmax', p, 16.0, np.array([present[0], present[-1]], np.uint64))]
    return [dict(name='exact-k%d-%s' % (k, name), k=k, pack=pk, thr=thr, forb=np.asarray(forb, np.uint64))
            for name, pk, thr, forb in out]


def top_case():
    """The main set at k = 5, threshold inf: 1,024 possible k-mers over 1,700 positions, so many counts
    are equal and some are 1. Returns the case, a `top` whose top-th count is shared beyond the rank, and the counts."""
    case = exact_cases(5)[0]
    km, cn = O.count_kmers_top(case['pack'], 5, case['thr'])
    tie = [t for t in range(2, len(cn)) if cn[t - 1] == cn[t] and cn[t - 2] == cn[t - 1]][0]
    return case, tie, cn
