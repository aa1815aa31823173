"""The quality stage's host build (engine.quality_filter(..., device=-1): csrc/pcabi_qual.h on the io
threads) against tests/qual_ref.py's restatement, every field of every read, at the small shapes where the
rule can go wrong. No GPU needed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import qual_ref as R

DEVICE = -1


def run(o, qual, off, ln, device):
    from custom_porechop_abi_amd import engine
    opts = np.zeros(1, engine.QUAL_OPTS)
    for k, v in o.items():
        opts[k] = v
    return engine.quality_filter(qual, off, ln, opts=opts, device=device)


def check_case(name, o, qual, off, ln, device):
    got = R.as_tuples(run(o, qual, off, ln, device))
    exp = R.records(qual, off, ln, o)
    bad = [i for i, (g, e) in enumerate(zip(got, exp)) if g != e]
    assert not bad and len(got) == len(exp), (name, bad[:5], got[bad[0]], exp[bad[0]], int(off[bad[0]]), int(ln[bad[0]]))
    return exp


def test_error_table_is_the_formula():
    from custom_porechop_abi_amd import engine
    t = engine.qual_error_table()
    assert t.dtype == np.uint64 and [int(x) for x in t] == R.ERR and len(R.ERR) == 94
    # no entry is near a rounding tie, so the float formula is exact
    assert min(abs((2 ** 32 * 10 ** (-q / 10)) % 1 - 0.5) for q in range(94)) > 0.002


def test_thresholds_become_integers_in_engine():
    from custom_porechop_abi_amd import engine
    for kw in ({}, {'window': 10, 'min_window_q': 12.5}, {'window': 64, 'min_window_q': 7.01, 'min_mean_q': 10.0},
               {'min_length': 5, 'max_length': 9, 'min_mean_q': 0.5}):
        o = engine.qual_opts(**kw)
        assert {k: int(o[k][0]) for k in R.to_ints()} == R.to_ints(**kw)
    assert int(engine.qual_opts()['max_mean_err'][0]) == 2 ** 32


@pytest.mark.parametrize('k', range(len(R.crop_cases())))
def test_cases_match_restatement(k):
    name, o, qual, off, ln = R.crop_cases()[k]
    check_case(name, o, qual, off, ln, DEVICE)


def test_cases_cover_what_they_promise():
    """(what crop_cases() promises, from the restatement)"""
    fronts, tails, one, none_good, kepts, aligns, zero_runs = set(), set(), 0, 0, set(), set(), []
    for name, o, qual, off, ln in R.crop_cases():
        recs = R.records(qual, off, ln, o)
        W = o['window']
        for (front, tail, kept, flags, _, _), a, n in zip(recs, off, ln):
            if a < 0:
                continue
            aligns.add(int(a + front) % 16)
            kepts.add(kept)
            if W and n >= W:
                fronts.add(front)
                tails.add(tail)
                one += kept == W
                none_good += kept == 0
        if name == 'alignments':
            assert int(off[-1]) + int(ln[-1]) == qual.size
            assert {int(a) % 16 for a in off} == set(range(16))
        if name == 'segments':
            z = [r[2] == 0 for r in recs]
            zero_runs = [i for i in range(len(z) - 2) if all(z[i:i + 3])]
            assert zero_runs[0] == 0 and zero_runs[-1] == len(z) - 3 and any(0 < i < len(z) - 3 for i in zero_runs)
            assert {4095, 4096, 4097, 8193} <= {r[2] for r in recs} and max(r[2] for r in recs) == 70000
        if name == 'bytes':
            assert {0, 32, 33, 126, 127, 255} <= set(qual.tolist()) and sum(a < 0 for a in off) >= 3
        assert set(qual.tolist()) >= {0, 255}
    assert {0, 63, 64, 65, 127, 128} <= fronts and {0, 63, 64, 65, 127, 128} <= tails
    assert one > 8 and none_good > 8 and aligns == set(range(16))


def test_window_sum_equality():
    """A window whose sum is exactly min_window_sum is good, one that is one short is not."""
    for W in (1, 4, 63, 64):
        name, o, qual, off, ln = [c for c in R.crop_cases() if c[0] == 'W%d' % W][0]
        assert o['min_window_sum'] == 20 * W
        recs = R.as_tuples(run(o, qual, off[-2:], ln[-2:], DEVICE))
        assert recs[0][:3] == (50, 50, W) and recs[1][:3] == (int(ln[-1]), 0, 0)


@pytest.mark.parametrize('k', range(len(R.equality_cases())))
def test_threshold_equality(k):
    name, o, qual, off, ln, ok = R.equality_cases()[k]
    exp = check_case(name, o, qual, off, ln, DEVICE)
    assert [(r[3] & R.FAIL) == 0 for r in exp] == ok, name


def test_bad_arguments_are_refused():
    from custom_porechop_abi_amd._lib import PcabiError
    qual = np.full(100, 70, np.uint8)
    good = R.to_ints(4, 10.0)
    for o, off, ln in ((dict(good, window=65), [0], [10]), (dict(good, max_mean_err=2 ** 32 + 1), [0], [10]),
                       (good, [95], [10]), (good, [101], [0]), (good, [0], [-1])):
        with pytest.raises(PcabiError, match=r'\(-1\)'):
            run(o, qual, np.array(off, np.int64), np.array(ln, np.int32), DEVICE)
    assert R.as_tuples(run(good, qual, np.array([90], np.int64), np.array([10], np.int32), DEVICE))[0][2] == 10


def test_qual_layer_under_sanitizers(tmp_path):
    """tests/qual_fuzz_main.cpp (csrc/pcabi_qual.h alone), built with -fsanitize=address,undefined as a
    program of its own and run as a child process: spans in blocks of exactly their size, the scans and
    sum_lane's lanes played against byte-by-byte sums."""
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path / 'qual_fuzz')
    base = ['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
            os.path.join(os.path.dirname(os.path.abspath(__file__)), 'qual_fuzz_main.cpp')]
    for extra in (['-static-libasan', '-static-libubsan'], []):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        if r.returncode == 0:
            break
    if r.returncode != 0 and ('asan' in r.stderr or 'ubsan' in r.stderr or 'sanitize' in r.stderr):
        pytest.skip('the sanitizer runtime cannot be linked')
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, '1', '5000'], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'rounds 5000' in r.stdout
