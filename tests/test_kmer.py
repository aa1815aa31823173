"""Ab-initio k-mer counter (custom_porechop_abi_amd/approx_counter.py, csrc/pcabi_kmer.hip) vs
the reference program's own output files (tests/golden/g5_kmer.json.gz, tools/make_golden_g5.py:
oracle/_ref/approx_counter built from porechop_abi/ab_initio_src/approx_counter.cpp, every read
sampled so the reference is deterministic):
  * not gpu: the driver (config / options, sampling, CompareCount ordering, DUST complexity,
    threshold scaling, forbidden and solid k-mers, multi-run names, the skip-end quirk, export)
    with the CPU restatement of the two counting steps (tests/kmer_oracle.py);
  * gpu    : the same with the HIP kernels (k_kmer_keys + hipcub sort / RLE, k_kmer_approx).
G5-edge (tests/golden/g5_kmer_edge.json.gz, the cases 'edge0' ..) pins the ends of the k range on a small
third input: k 4, 5, 8, 11, 21, 24, 31 and 32, the last with a low-complexity threshold that lets the
32-mer TTT...T through -- its value is the one skipped positions are stored as. Below k = 4 the reference
program crashes in errorCount, so no case pins the approximate counts there. The kernels themselves are
tested case by case in tests/test_gpu_kmer.py and tests/test_kmer_core_cpu.py."""
import gzip
import json
import os
import shutil

import pytest

from tests import golden_lib

G5 = json.load(gzip.open(os.path.join(golden_lib.GOLDEN, 'g5_kmer.json.gz'), 'rt'))['cases']
EDGE = json.load(gzip.open(os.path.join(golden_lib.GOLDEN, 'g5_kmer_edge.json.gz'), 'rt'))['cases']
CASES = dict([(i, c) for i, c in enumerate(G5)] + [('edge%d' % i, c) for i, c in enumerate(EDGE)])
EDGE_CPU = [i for i in CASES if str(i).startswith('edge')]   # small enough for the CPU restatement, all of them


def _run_case(case, tmp_path):
    from custom_porechop_abi_amd import approx_counter as AC
    src = os.path.join(golden_lib.GOLDEN, case['input'])
    plain = str(tmp_path / 'reads.fasta')
    with gzip.open(src, 'rb') as f, open(plain, 'wb') as g:
        shutil.copyfileobj(f, g)
    args = [os.path.join(golden_lib.GOLDEN, a) if a.startswith('kmer/') else a for a in case['args']]
    AC.main([plain, '-o', str(tmp_path / 'out'), '-e', str(tmp_path / 'exact'), '-sn', '1000000', '-nt', '4',
             '-v', '0'] + args)
    return {fn: open(tmp_path / fn).read() for fn in case['files']}


def _compare(case, got):
    solid = '-sk' in case['args']
    for fn, exp in case['files'].items():
        if solid and fn.startswith('exact'):
            # get_solid_kmers uses an unstable std::sort on counts: ties have no defined order
            assert sorted(got[fn].splitlines()) == sorted(exp.splitlines()), fn
            counts = [int(x.split('\t')[1]) for x in got[fn].splitlines()]
            assert counts == sorted(counts, reverse=True)
        else:
            assert got[fn] == exp, fn


@pytest.mark.parametrize('idx', list(range(len(G5))) + EDGE_CPU)
def test_counter_driver_with_cpu_restatement(idx, tmp_path, monkeypatch):
    from custom_porechop_abi_amd import approx_counter as AC
    from tests import kmer_oracle
    monkeypatch.setattr(AC, 'count_kmers', kmer_oracle.count_kmers)
    monkeypatch.setattr(AC, 'count_kmers_top', kmer_oracle.count_kmers_top)
    monkeypatch.setattr(AC, 'error_count', kmer_oracle.error_count)
    case = CASES[idx]
    if idx in (1, 2, 3, 6):
        pytest.skip('CPU restatement: a subset of the cases keeps the CPU suite short')
    _compare(case, _run_case(case, tmp_path))


@pytest.mark.gpu
@pytest.mark.parametrize('idx', list(CASES))
def test_counter_on_gpu_matches_reference(gpu_lib, idx, tmp_path):
    case = CASES[idx]
    _compare(case, _run_case(case, tmp_path))


def test_threshold_and_complexity_match_reference_arithmetic():
    import numpy as np
    from custom_porechop_abi_amd import approx_counter as AC
    assert AC.adjust_threshold(1.0, 16, 16) == 1.0
    assert AC.adjust_threshold(1.5, 16, 12) == float(np.float32(1.5) * np.float32(121 / 225.0))
    km = AC.str_to_kmer('ACACACACACACACAC')
    assert AC.kmer_to_str(km, 16) == 'ACACACACACACACAC'
    # ACAC...: dimers alternate AC / CA, 8 + 7 of them: (8*7 + 7*6) / 28
    assert AC.complexity([km], 16)[0] == np.float32(98) / np.float32(28)
