"""The k-mer counter's three entry points on the GPU (csrc/pcabi_kmer.hip: k_kmer_keys + hipcub sort /
run-length encode, the top cut, k_kmer_approx), kernel by kernel on the crafted cases of
tests/kmer_cases.py: every k-mer and every count against tests/kmer_oracle.py, exactly. The cases reach
what the G5 driver runs (tests/test_kmer.py) never do: k 2 .. 32 (the full mask, bit 31, 64 key bits and the
32-mer TTT...T, whose value is the skipped positions' sentinel), sequences of every length modulo 4,
shorter than k and empty, bases instead of N between the sequences, block and lane-group edges, every
approximate count and not only the top ones, and the cut rule with ties, min_count and the cap protocol.
tests/test_kmer_core_cpu.py checks the same cases on the host and that they hold what they promise."""
import ctypes

import numpy as np
import pytest

from tests import kmer_cases as C
from tests import kmer_oracle as O


def _names(cases):
    return [c['name'] for c in cases]


APPROX = C.approx_cases()


@pytest.mark.gpu
@pytest.mark.parametrize('idx', range(len(APPROX)), ids=_names(APPROX))
def test_approx_counts(gpu_lib, idx):
    from custom_porechop_abi_amd import approx_counter as AC
    case = APPROX[idx]
    got = AC.error_count(case['pack'], case['kmers'], case['k'])
    C.same(got, O.error_count(case['pack'], case['kmers'], case['k']), case['name'])
    if len(case['kmers']) > 1:
        assert got[0] == got[-1]        # the k-mer listed twice


@pytest.mark.gpu
@pytest.mark.parametrize('k', C.EXACT_K)
def test_exact_counts(gpu_lib, k):
    from custom_porechop_abi_amd import approx_counter as AC
    for case in C.exact_cases(k):
        km, cn = AC.count_kmers(case['pack'], k, case['thr'], case['forb'].tolist())
        ekm, ecn = O.count_kmers(case['pack'], k, case['thr'], case['forb'])
        assert [AC.kmer_to_str(v, k) for v in km.tolist()] == [AC.kmer_to_str(v, k) for v in ekm.tolist()], case['name']
        C.same(cn, ecn, case['name'])
        # the same through the sort by count, no cut
        tkm, tcn = AC.count_kmers_top(case['pack'], k, case['thr'], case['forb'].tolist())
        ekm, ecn = O.count_kmers_top(case['pack'], k, case['thr'], case['forb'])
        C.same(tkm, ekm, case['name'] + ' top')
        C.same(tcn, ecn, case['name'] + ' top')


@pytest.mark.gpu
def test_top_cut(gpu_lib):
    from custom_porechop_abi_amd import approx_counter as AC
    case, tie, cn = C.top_case()
    pk, k, thr = case['pack'], case['k'], case['thr']
    n_unique = len(cn)
    for top in (0, 1, tie, n_unique, n_unique + 5):
        for min_count in (0, 2, int(cn.max()) + 1):
            km, c = AC.count_kmers_top(pk, k, thr, (), top=top, min_count=min_count)
            ekm, ec = O.count_kmers_top(pk, k, thr, (), top=top, min_count=min_count)
            C.same(km, ekm, (top, min_count))
            C.same(c, ec, (top, min_count))
    km, c = AC.count_kmers_top(pk, k, thr, (), top=tie)
    assert len(km) > tie and c[tie - 1] == c[-1] and (np.diff(km[c == c[-1]].astype(object)) > 0).all()


@pytest.mark.gpu
def test_top_cap_protocol(gpu_lib):
    """cap below the answer: its size comes back and nothing is written; cap equal to it: filled."""
    from custom_porechop_abi_amd import approx_counter as AC
    case, tie, cn = C.top_case()
    pk, k = case['pack'], case['k']
    L = AC._declare(gpu_lib)
    ekm, ec = O.count_kmers_top(pk, k, case['thr'], (), top=tie)
    ekm_all, ec_all = O.count_kmers(pk, k, case['thr'])
    for top, ekm, ec in ((tie, ekm, ec), (-1, ekm_all, ec_all)):     # the cut, and pcabi_kmer_count_host's mode
        n_out = len(ekm)
        for cap in (n_out - 1, 0, n_out):
            km = np.full(n_out + 2, 0xABABABABABABABAB, np.uint64)
            c = np.full(n_out + 2, 0xCDCDCDCD, np.uint32)
            n = L.pcabi_kmer_top_host(0, AC._p(pk.codes), pk.codes.size, AC._p(pk.offs), AC._p(pk.lens), len(pk), k,
                                      ctypes.c_float(case['thr']), None, 0, top, 0, AC._p(km), AC._p(c), cap)
            assert n == n_out, (top, cap, n)
            if cap < n_out:
                assert (km == np.uint64(0xABABABABABABABAB)).all() and (c == 0xCDCDCDCD).all(), (top, cap)
            else:
                C.same(km[:n_out], ekm, (top, cap))
                C.same(c[:n_out].astype(np.int64), ec, (top, cap))
                assert (km[n_out:] == np.uint64(0xABABABABABABABAB)).all() and (c[n_out:] == 0xCDCDCDCD).all()


@pytest.mark.gpu
def test_poly_t_32mer_is_counted(gpu_lib):
    """The 32-mer TTT...T has the value the skipped positions are stored as (~0): it must come back
    with its own count, with skipped positions next to it, without any, and forbidden."""
    from custom_porechop_abi_amd import approx_counter as AC
    cases = {c['name'].split('-', 2)[2]: c for c in C.exact_cases(32)}
    poly_t = 'T' * 32
    for name, there in (('sixteen', True), ('inf', True), ('clean', True), ('sixteen-forbid-minmax', False), ('zero', False)):
        case = cases[name]
        km, cn = AC.count_kmers(case['pack'], 32, case['thr'], case['forb'].tolist())
        ekm, ecn = O.count_kmers(case['pack'], 32, case['thr'], case['forb'])
        got = dict(zip([AC.kmer_to_str(v, 32) for v in km.tolist()], cn.tolist()))
        exp = dict(zip([AC.kmer_to_str(v, 32) for v in ekm.tolist()], ecn.tolist()))
        assert (poly_t in exp) == there, name
        assert got.get(poly_t) == exp.get(poly_t), (name, got.get(poly_t), exp.get(poly_t))
        tkm, tcn = AC.count_kmers_top(case['pack'], 32, case['thr'], case['forb'].tolist(), top=3)
        ekm, ecn = O.count_kmers_top(case['pack'], 32, case['thr'], case['forb'], top=3)
        C.same(tkm, ekm, name)
        C.same(tcn, ecn, name)
