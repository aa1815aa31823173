"""The k-mer kernels' arithmetic (csrc/pcabi_kmer.h: the dimer score, the window key, the pattern masks,
Myers' column step and the dword walk of best_distance) on the host, through tests/native/kmer_model.cpp,
against tests/kmer_oracle.py: a plain edit-distance DP (free text start, minimum over text ends) and the
restated reference arithmetic of count_kmers. Everything is integer or float32-exact; no GPU needed.
tests/test_gpu_kmer.py runs the same cases (tests/kmer_cases.py) through the entry points on the device."""
import ctypes
import itertools
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import kmer_cases as C
from tests import kmer_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_model(src=os.path.join(ROOT, 'tests', 'native', 'kmer_model.cpp')):
    out = os.path.join(tempfile.mkdtemp(prefix='pcabi_kmer_model_'), 'kmer_model.so')
    subprocess.check_call(['g++', '-std=c++17', '-O2', '-shared', '-fPIC', '-Wall', '-o', out, src])
    L = ctypes.CDLL(out)
    P, i64 = ctypes.c_void_p, ctypes.c_int64
    L.kmer_model_keys.argtypes = [P, P, P, i64, ctypes.c_int, ctypes.c_float, P, i64, P, P, P]
    L.kmer_model_low_complexity.argtypes = [P, i64, ctypes.c_int, ctypes.c_float, P]
    L.kmer_model_best.argtypes = [P, P, P, i64, ctypes.c_int, P, i64, P]
    for f in (L.kmer_model_keys, L.kmer_model_low_complexity, L.kmer_model_best):
        f.restype = None
    return L


@pytest.fixture(scope='module')
def model():
    return build_model()


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def model_best(L, pk, kmers, k):
    kmers = np.ascontiguousarray(kmers, np.uint64)
    assert not (pk.offs & 3).any() and pk.codes.size % 4 == 0
    out = np.full((len(kmers), len(pk)), -1, np.int32)
    L.kmer_model_best(_p(pk.codes), _p(pk.offs), _p(pk.lens), len(pk), k, _p(kmers), len(kmers), _p(out))
    return out.astype(np.int64)


def model_counts(L, pk, k, thr, forb):
    """k_kmer_keys on the host, then what the sort and the run-length encode make of its keys."""
    key_off = np.zeros(len(pk) + 1, np.int64)
    key_off[1:] = np.cumsum(np.maximum(pk.lens.astype(np.int64) - k + 1, 0))
    keys = np.zeros(int(key_off[-1]), np.uint64)
    has = np.full(int(key_off[-1]), 7, np.uint8)
    forb = np.ascontiguousarray(forb, np.uint64)
    L.kmer_model_keys(_p(pk.codes), _p(pk.offs), _p(pk.lens), len(pk), k, thr, _p(forb) if len(forb) else None, len(forb),
                      _p(key_off), _p(keys), _p(has))
    assert set(has.tolist()) <= {0, 1} and (keys[has == 0] == np.uint64(2 ** 64 - 1)).all()
    km, cn = np.unique(keys[has == 1], return_counts=True)
    return km, cn.astype(np.int64)


def model_low(L, kmers, k, thr):
    kmers = np.ascontiguousarray(kmers, np.uint64)
    out = np.full(len(kmers), 7, np.uint8)
    L.kmer_model_low_complexity(_p(kmers), len(kmers), k, thr, _p(out))
    return out.astype(bool)


def test_fast_restatement_is_the_plain_dp():
    """kmer_oracle.best_distances (a running minimum down each column) against the cell-by-cell DP."""
    for k in (4, 8, 32):
        case = C.approx_case(k, 33, 9)
        C.same(O.best_distances(case['pack'], case['kmers'], k), O.best_distances_plain(case['pack'], case['kmers'], k), k)


def test_myers_exhaustive_k4(model):
    """Every 4-mer against every text of 0..6 letters over the five codes."""
    kmers = np.arange(256, dtype=np.uint64)
    n_texts = 0
    for n in range(7):
        texts = [np.array(t, np.uint8) for t in itertools.product(range(5), repeat=n)]
        pk = C.pack(texts, np.random.default_rng(n))
        C.same(model_best(model, pk, kmers, 4), O.best_distances_plain(pk, kmers, 4), n)
        n_texts += len(texts)
    assert n_texts == sum(5 ** n for n in range(7))


@pytest.mark.parametrize('k', (5, 8, 16, 31, 32))
def test_myers_random(model, k):
    for seed in range(3):
        case = C.random_approx_case(k, seed)
        C.same(model_best(model, case['pack'], case['kmers'], k), O.best_distances(case['pack'], case['kmers'], k), (k, seed))


@pytest.mark.parametrize('idx', range(len(C.APPROX_K) * len(C.APPROX_SHAPES)))
def test_approx_cases_match_restatement(model, idx):
    case = C.approx_cases()[idx]
    C.same(model_best(model, case['pack'], case['kmers'], case['k']), O.best_distances(case['pack'], case['kmers'], case['k']),
         case['name'])


def _thresholds(scores):
    """Every score that occurs (equality decides), inf, 0."""
    s = np.unique(scores[np.isfinite(scores)]).tolist()
    return s + [float('inf'), 0.0]


@pytest.mark.parametrize('k', (2, 3, 4, 5, 16, 31, 32))
def test_low_complexity_is_the_reference_arithmetic(model, k):
    if k in (4, 5):
        kmers = np.arange(4 ** k, dtype=np.uint64)
    else:
        rng = np.random.default_rng(k)
        kmers = [C.kmer_value(rng.integers(0, 4, k)) for _ in range(300)]
        # low-complexity ones too: few letters, short periods
        kmers += [C.kmer_value(np.resize(rng.integers(0, 4, p), k)) for p in (1, 1, 2, 2, 3, 3, 4, 5) for _ in range(8)]
        kmers = np.unique(np.array(kmers + [0, 4 ** k - 1], np.uint64))
    scores = O.dimer_score(kmers, k)
    assert np.isnan(scores).all() if k == 2 else np.isfinite(scores).all()
    thrs = _thresholds(scores)
    assert len(thrs) > 2 or k == 2
    for thr in thrs:
        with np.errstate(invalid='ignore'):
            exp = scores >= np.float32(thr)   # NaN at k = 2: never low-complexity
        C.same(model_low(model, kmers, k, thr), exp, (k, thr))
        if k == 2:
            assert not exp.any()


@pytest.mark.parametrize('k', C.EXACT_K)
def test_exact_cases_match_restatement(model, k):
    for case in C.exact_cases(k):
        km, cn = model_counts(model, case['pack'], k, case['thr'], case['forb'])
        ekm, ecn = O.count_kmers(case['pack'], k, case['thr'], case['forb'])
        C.same(km, ekm, case['name'])
        C.same(cn, ecn, case['name'])


@pytest.mark.parametrize('k', (4, 5))
def test_window_key_at_every_occurring_threshold(model, k):
    """The main set's windows at every score that occurs, with and without a forbidden set."""
    cases = C.exact_cases(k)
    pk, many = cases[0]['pack'], cases[5]['forb']
    v, dna = O.window_values(pk, k)
    for thr in _thresholds(O.dimer_score(v[dna], k)):
        for forb in (np.zeros(0, np.uint64), many):
            km, cn = model_counts(model, pk, k, thr, forb)
            ekm, ecn = O.count_kmers(pk, k, thr, forb)
            C.same(km, ekm, (k, thr))
            C.same(cn, ecn, (k, thr))


def test_cases_cover_what_they_promise():
    """(what tests/kmer_cases.py promises, from the restatement)"""
    poly_t = {k: np.uint64(4 ** k - 1) for k in C.EXACT_K}
    for k in C.APPROX_K:
        dist, tails, places = set(), set(), set()
        for case in [c for c in C.approx_cases() if c['k'] == k]:
            pk, kmers = case['pack'], case['kmers']
            best = O.best_distances(pk, kmers, k)
            dist |= set(np.minimum(best, 4).reshape(-1).tolist())
            # the best column lies in the ragged tail: without the tail's bases the distance is larger,
            # and the count would change
            cut = C.Pack(pk.codes, pk.offs, pk.lens & ~3)
            lost = (best <= 2) & (O.best_distances(cut, kmers, k) > best)
            tails |= set((pk.lens[np.argwhere(lost)[:, 1]] & 3).tolist())
            places |= {(e, place) for (_, _, e, place, _, _) in case['plants']}
            if len(pk) > C.IDX_PAD:
                assert len(pk) in (31, 32, 33, 97) and len(kmers) in (63, 64, 65, 130)
                assert (kmers[0] == kmers[-1]) and kmers[1] == np.uint64(4 ** k - 1) and kmers[2] == 0
                assert (pk.seq(C.IDX_N) == C.N).sum() == 1 and best[0, C.IDX_N] == 1
                m = C.pad_prefix_len(k)
                a = int(pk.offs[C.IDX_PAD])
                assert int(pk.lens[C.IDX_PAD]) == m and m % 4 and best[0, C.IDX_PAD] == k - m
                assert k - m == 1 or k == 5
                through = min((m + 3) & ~3, k)      # a walk to the dword's end sees more of the k-mer
                assert (pk.codes[a:a + through] == C.kmer_codes(kmers[0], k)[:through]).all()
                ends = pk.offs + pk.lens
                gaps = [pk.codes[int(e):(int(e) + 3) & ~3] for e in ends]
                assert sum(len(g) for g in gaps) > 20 and all((g < 4).all() for g in gaps)
            if len(pk) == 97:
                assert {0, 1, k - 1, k, k + 1} | set(range(2, C.MAX_LEN)) <= set(pk.lens.tolist())
                # copies across a dword boundary, and at the start
                assert any(p % 4 == 2 for (_, _, _, place, p, _) in case['plants'] if place == 2)
                assert any(p == 0 for (_, _, _, place, p, _) in case['plants'] if place == 0)
        assert dist == {0, 1, 2, 3, 4}, (k, dist)
        assert tails == {1, 2, 3}, (k, tails)
        assert places == {(e, p) for e in range(4) for p in range(3)}, k
    for k in C.EXACT_K:
        cases = {c['name'].split('-', 2)[2]: c for c in C.exact_cases(k)}
        pk = cases['inf']['pack']
        v, dna = O.window_values(pk, k)
        assert {0, k - 1, k, k + 1, 129, 257} <= set(pk.lens.tolist())
        km, cn = O.count_kmers(pk, k, float('inf'))
        assert cn.max() >= 300 and not dna.all() and dna.any()
        assert km[-1] == poly_t[k] and km[0] == 0
        assert (km >> np.uint64(2 * k - 1)).any()                       # first base G or T
        zero = O.count_kmers(pk, k, 0.0)[0]
        assert len(zero) == (0 if k > 2 else len(km))                   # k = 2: no score, nothing skipped
        eq = cases['eq']['thr']
        if k > 2:
            s = O.dimer_score(v[dna], k)
            assert (s == np.float32(eq)).any() and (s < np.float32(eq)).any() and ((s > np.float32(eq)).any() or k == 3)
        one, minmax, many = cases['forbid-one']['forb'], cases['eq-forbid-minmax']['forb'], cases['forbid-many']['forb']
        assert len(one) == 1 and one[0] in km and minmax.tolist() == [km[0], km[-1]]
        assert np.isin(many, km).sum() >= min(40, len(km)) and (k < 15 or len(many) > 990)
        assert (np.diff(many.astype(object)) > 0).all()
        assert len(cases['forbid-one']['forb']) and len(cases['inf']['forb']) == 0
        cl = cases['clean']['pack']
        cv, cdna = O.window_values(cl, k)
        ckm, ccn = O.count_kmers(cl, k, float('inf'))
        assert cdna.all() and ccn.sum() == len(cv) and ckm[-1] == poly_t[k] and (cl.lens >= k).all()
        assert (cases['short']['pack'].lens < k).all() and len(cases['short']['pack']) == k
        assert len(cases['none']['pack']) == 0
        assert len(O.count_kmers(cases['short']['pack'], k, float('inf'))[0]) == 0
        if k >= 31:
            # TTT...T scores below 16 and is counted next to skipped positions
            km16, cn16 = O.count_kmers(pk, k, 16.0)
            assert O.dimer_score([poly_t[k]], k)[0] < 16 and km16[-1] == poly_t[k] and cn16[-1] == 257 - k + 1
            assert len(km16) < len(v)
    case, tie, cn = C.top_case()
    desc = np.sort(cn)[::-1]
    assert desc[tie - 1] == desc[tie] and len(np.unique(cn)) < len(cn) // 2 and desc[0] > 2 > desc[-1]
