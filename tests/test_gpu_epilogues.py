"""The decision epilogues on crafted result tables: k_end_trim, k_flag_count / k_flag_write,
k_first_hit, k_best_full_id, k_trim_views and the identity they all compare, the DEVICE build of
pcabi::pid6 (csrc/pcabi_dp.h), through the C ABI (include/pcabi.h).

Tables are built in numpy and uploaded through torch tensors. Expected values are plain Python
loops that restate the reference's lines (porechop_abi/nanopore_read.py) over the same tables,
with tests/identity_ref.py's '%f' round trip as the identity: none of the product's Python and
nothing of tests/oracle_lib.py is used. Table rows are legal results -- rs == -1 for a failed
alignment, otherwise 0 <= rs <= re, 0 <= m <= min(l1, l2), l1, l2 >= 1 -- except the rows that
are there to be NaN (a zero length), which are counted apart.

Result layout (pcabi_align_cross_dev): field f of (adapter a, window w) at res[f * stride +
a * n_win + w]; fields rs, re (inclusive), as, ae, score, m, l1, l2."""
import ctypes
import random

import numpy as np
import pytest

from tests import identity_ref
from tests.identity_ref import ref_pid6, ref_pid6_scalar

pytestmark = pytest.mark.gpu

RS, RE, M, L1, L2 = 0, 1, 5, 6, 7
JUNK = -12345          # beyond the block a call may read or write: never a legal field


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _table(n_adp, n_win, pad):
    """An (8, stride) table of JUNK; stride = n_adp * n_win + pad."""
    return np.full((8, n_adp * n_win + pad), JUNK, np.int32)


def _set(res, i, rs, re, m, l1, l2):
    res[:, i] = (rs, re, 0, max(l2 - 1, 0), 3 * m, m, l1, l2)


# ---- the device build of pid6, bit for bit ----------------------------------------------------

def _device_pid6(L, m, l):
    """pid6(m[a], l[a]) from the device: k_best_full_id over one window per adapter with best
    zeroed leaves best[a] = max(0.0, pid6(m, l2)). At most 65,536 adapters per launch."""
    out = np.empty(len(m), np.float64)
    for lo in range(0, len(m), 65536):
        mm, ll = m[lo:lo + 65536], l[lo:lo + 65536]
        n = len(mm)
        res = np.zeros((8, n), np.int32)
        res[M], res[L1], res[L2] = mm, ll, ll
        res[RE] = 0
        d_res, d_best = _dev(res), _dev(np.zeros(n, np.float64))
        assert L.pcabi_best_full_identity_dev(_p(d_res), n, 1, n, _p(d_best), _stream()) == 0
        out[lo:lo + n] = _host(d_best)
    return out


def _assert_same_bits(got, exp, m, l):
    bad = np.nonzero(got.view(np.uint64) != exp.view(np.uint64))[0]
    low, high = int((got[bad] < exp[bad]).sum()), int((got[bad] > exp[bad]).sum())
    print('device pid6: %d pairs, %d differ (%d low, %d high)' % (len(m), len(bad), low, high))
    assert len(bad) == 0, [(int(m[i]), int(l[i]), repr(got[i]), repr(exp[i])) for i in bad[:6]]


def test_device_pid6_grid(gpu_lib):
    """Every pair 0 <= m <= l <= 700 (test_abi.py's and test_dp_core_cpu.py's grids, on the device)."""
    l = np.repeat(np.arange(1, 701), np.arange(2, 702)).astype(np.int32)
    m = np.concatenate([np.arange(0, k + 1) for k in range(1, 701)]).astype(np.int32)
    _assert_same_bits(_device_pid6(gpu_lib, m, l), ref_pid6(m, l), m, l)


@pytest.mark.parametrize('length', identity_ref.TIE_LENGTHS_EVERY_M + identity_ref.TIE_LENGTHS_FIRST_M)
def test_device_pid6_ties(gpu_lib, length):
    """The lengths whose products d * 1e6 land on k + 0.5 (identity_ref.py). At 64000 and 128000
    the exact product decides 12,403 pairs each: a device build whose tie test is fused into an
    fma of the exact product (-ffp-contract=fast on `d * 1e6 - k`) is off by 1e-6 on all of them."""
    every = length in identity_ref.TIE_LENGTHS_EVERY_M
    m = np.arange(length + 1 if every else identity_ref.TIE_FIRST_M, dtype=np.int32)
    l = np.full(len(m), length, np.int32)
    if length in (64000, 128000):
        assert identity_ref.corrected_ties(length) >= 10000
    _assert_same_bits(_device_pid6(gpu_lib, m, l), ref_pid6(m, l), m, l)


def _decided_ties(length=64000, each=2):
    """(m, value, threshold): odd m whose tie the exact product decides, `each` of them rounding
    up and `each` down, with the threshold midway between the value and the neighbour 1e-6 away
    that rint(d * 1e6) alone gives -- a wrong tie lands on the other side of it."""
    out, ups, downs = [], 0, 0
    for m in range(1, length, 2):
        d = 100.0 * m / length
        k, naive = int(('%f' % d).replace('.', '')), round(d * 1e6)
        if k == naive or (ups if k > naive else downs) >= each:
            continue
        ups, downs = ups + (k > naive), downs + (k < naive)
        value, wrong = ref_pid6_scalar(m, length), float('%d.%06d' % divmod(naive, 1000000))
        thr = (value + wrong) / 2
        assert abs(value - wrong) < 1.5e-6 and min(value, wrong) < thr < max(value, wrong)
        out.append((m, value, thr))
        if ups == each and downs == each:
            break
    assert ups == each and downs == each
    return out


def test_tie_decides_end_trim(gpu_lib):
    """k_end_trim's `partial_score > end_threshold` (nanopore_read.py:187, :209) with the partial
    identity pid6(m, 64000) a decided tie and the threshold beside it."""
    length = 64000
    for m, value, thr in _decided_ties(length):
        res = _table(1, 1, 0)
        _set(res, 0, 5, 14, m, length, length)
        d_res, d_st, d_et = _dev(res), _dev(np.full(1, JUNK, np.int32)), _dev(np.full(1, JUNK, np.int32))
        assert gpu_lib.pcabi_end_trim_dev(_p(d_res), 1, 1, _p(d_res), 1, 1, 1, 150, 2, thr, 4, _p(d_st), _p(d_et),
                                          None, None, _stream()) == 0
        trims = value > thr
        assert (int(_host(d_st)[0]), int(_host(d_et)[0])) == ((15 + 2, 150 - 5 + 2) if trims else (0, 0)), (m, thr)


def test_tie_decides_first_hit(gpu_lib):
    """k_first_hit's threshold compare with the full identity pid6(m, 64000) a decided tie: the
    first adapter hits or the (certain) second one does."""
    length = 64000
    for m, value, thr in _decided_ties(length):
        res = _table(2, 1, 0)
        _set(res, 0, 5, 14, m, length, length)
        _set(res, 1, 7, 30, 24, 24, 24)
        d_res, d_hits = _dev(res), _dev(np.full((5, 1), JUNK, np.int32))
        assert gpu_lib.pcabi_first_hit_dev(_p(d_res), 2, 1, 2, thr, _p(d_hits), 1, _stream()) == 0
        exp = [0, 5, 14, m, length] if not value < thr else [1, 7, 30, 24, 24]
        assert _host(d_hits)[:, 0].tolist() == exp, (m, thr)


def test_tie_decides_barcode_call(gpu_lib):
    """k_barcode_call's best score is pid6(m, 64000) bit for bit, and `best >= threshold`
    (nanopore_read.py:476) goes the reference's way with the threshold beside a decided tie."""
    length = 64000
    for m, value, thr in _decided_ties(length):
        res = _table(1, 1, 0)
        _set(res, 0, 5, 14, m, length, length)
        d_res, slot = _dev(res), _dev(np.zeros(1, np.int32))
        d_call, d_scores = _dev(np.full(1, JUNK, np.int32)), _dev(np.full(4, -1.0))
        assert gpu_lib.pcabi_barcode_call_dev(_p(d_res), 1, _p(slot), _p(slot), 1, None, 0, None, None, 0, 1, thr, 0.0,
                                              0, _p(d_call), _p(d_scores), _stream()) == 0
        scores = _host(d_scores)
        assert scores.view(np.uint64)[0] == np.float64(value).view(np.uint64), (m, repr(scores[0]), repr(value))
        assert scores[1:].tolist() == [0.0, 0.0, 0.0]
        assert int(_host(d_call)[0]) == (0 if value >= thr else -1), (m, thr)


# ---- k_end_trim and the alignment lists ---------------------------------------------------------

N_READS = (0, 1, 63, 64, 65, 257)
N_ADPS = (0, 1, 3, 4, 5, 15, 16, 17, 33)
END_SIZES = (1, 150)
EXTRAS = (0, 2, 1000)
MIN_TRIMS = (0, 4, 151)
THRESHOLDS = (0.0, 75.0, 90.0, 100.0)
# partial identities exactly on a threshold, and one match more / fewer
ON_THRESHOLD = ((3, 4), (9, 10), (1, 1))
BESIDE = ((2, 4), (4, 4), (8, 10), (10, 10), (0, 1))


def _end_side(rng, n_adp, n_read, pad, side, end_size, min_trim):
    """One side's table. Every read is all-failed with probability 1/8; otherwise each row draws a
    kind: failed, NaN (l1 == 0), on / beside a threshold, the side's edge (re + 1 == end_size at
    the start, rs == 0 at the end), an aligned stretch of min_trim - 1 or min_trim bases, or free."""
    res = _table(n_adp, n_read, pad)
    for r in range(n_read):
        dead = rng.random() < 0.125
        for a in range(n_adp):
            i = a * n_read + r
            kind = 'failed' if dead else rng.choice(('failed', 'nan', 'on', 'beside', 'edge', 'short', 'long',
                                                     'free', 'free', 'free', 'good', 'good'))
            rs = rng.randint(0 if side else 1, 40)
            re = rs + rng.randint(0, 60)
            m, l1 = rng.choice(ON_THRESHOLD + BESIDE)
            if kind == 'failed':
                _set(res, i, -1, 20, 10, 10, 10)          # only rs says so: the rest would trim
                continue
            if kind == 'nan':
                m, l1 = 0, 0
            elif kind == 'on':
                m, l1 = rng.choice(ON_THRESHOLD)
            elif kind == 'beside':
                m, l1 = rng.choice(BESIDE)
            elif kind == 'edge':
                m, l1 = 19, 20
                if side == 0:
                    re = end_size - 1
                    rs = rng.randint(0, re)
                else:
                    rs = 0
            elif kind in ('short', 'long'):
                m, l1 = 19, 20
                span = max(min_trim - (kind == 'short'), 1)
                re = rs + span - 1
            elif kind == 'good':
                l1 = rng.randint(20, 40)
                m = l1 - rng.randint(0, 1)
            else:
                l1 = rng.randint(1, 40)
                m = rng.randint(0, l1)
            _set(res, i, rs, re, m, l1, l1 + rng.randint(0, 5))
    return res


def _expected_end_side(res, n_adp, n_read, side, end_size, extra, thr, min_trim, seen):
    """find_start_trim (nanopore_read.py:181-192) / find_end_trim (:203-214) over the table's rows,
    align_adapter's parse (:488-498) included. Returns the amounts, the flags and the recorded
    alignments (read-major, adapter order: the order the reference appends them in)."""
    trim, flags, rows = [0] * n_read, np.zeros(n_adp * n_read, np.uint8), []
    for r in range(n_read):
        amount, winner, n_failed = 0, None, 0
        for a in range(n_adp):
            i = a * n_read + r
            rs, re, m, l1, l2 = (int(res[f, i]) for f in (RS, RE, M, L1, L2))
            if rs == -1:
                read_end, partial = 0, 0.0
                n_failed += 1
                seen['failed'] += 1
            else:
                read_end, partial = re + 1, ref_pid6_scalar(m, l1)
            edge_ok = read_end != end_size if side == 0 else rs != 0
            long_enough = read_end - rs >= min_trim
            if rs != -1:
                seen['nan'] += l1 == 0
                seen['on_threshold'] += partial == thr and (m, l1) in ON_THRESHOLD
                seen['one_more'] += (m - 1, l1) in ON_THRESHOLD and ref_pid6_scalar(m - 1, l1) == thr
                seen['one_fewer'] += (m + 1, l1) in ON_THRESHOLD and ref_pid6_scalar(m + 1, l1) == thr
                seen['edge_start' if side == 0 else 'edge_end'] += partial > thr and long_enough and not edge_ok
                seen['span_min_minus_1'] += partial > thr and edge_ok and read_end - rs == min_trim - 1
                seen['span_min'] += partial > thr and edge_ok and read_end - rs == min_trim
            if partial > thr and edge_ok and long_enough:
                trim_amount = (read_end + extra) if side == 0 else (end_size - rs) + extra
                if trim_amount > amount:
                    winner = a
                amount = max(amount, trim_amount)
                flags[i] = 1
                rows.append((r, a, rs, re, m, l1, l2))
        trim[r] = amount
        seen['all_failed_reads'] += n_adp > 0 and n_failed == n_adp
        if winner is not None:
            seen['winner_wave_%d' % (winner % 4)] += 1
            seen['winner_second_pass'] += winner >= 16
    return trim, flags, rows


def _check_flag_list(L, d_flags, flags, n_adp, n_read, d_res, stride, rows):
    """pcabi_flag_list_dev: the recorded alignments in the reference's order and their count; with
    a cap below the count the count alone comes back (pcabi.h: "a side whose count exceeds cap is
    not written")."""
    n = len(rows)
    assert n == int(flags.sum())
    for cap in sorted({n, n + 3, max(n - 1, 0)}):
        d_out, d_n = _dev(np.full((7, cap), JUNK, np.int32)), _dev(np.full(1, 2**63 - 1, np.uint64).view(np.int64))
        assert L.pcabi_flag_list_dev(_p(d_flags), n_adp, n_read, _p(d_res), stride, _p(d_out), cap, _p(d_n),
                                     _stream()) == 0
        assert int(_host(d_n)[0]) == n
        out = _host(d_out)
        if cap < n:
            assert (out == JUNK).all()
        else:
            assert out[:, :n].T.tolist() == [list(x) for x in rows]
            assert (out[:, n:] == JUNK).all()


def test_end_trim_and_alignment_lists(gpu_lib):
    """pcabi_end_trim_dev (k_end_trim: four waves stride the adapters by 4, four adapters in flight
    per wave, so 16 adapters per pass; the waves' maxima meet in LDS) and pcabi_flag_list_dev over
    its flags, against nanopore_read.py:175-217. The reference-side counters at the end show that
    the cases held every edge named there."""
    from collections import Counter
    rng = random.Random(20)
    seen, used = Counter(), Counter()
    n_cases = 36
    for c in range(n_cases):
        n_read = N_READS[c % 6]
        n_sa, n_ea = N_ADPS[c % 9], N_ADPS[(2 * c + 4) % 9]
        end_size, extra = END_SIZES[(c // 2) % 2], EXTRAS[(c // 3) % 3]
        min_trim, thr = MIN_TRIMS[(c // 4) % 3], THRESHOLDS[(c // 5) % 4]
        pad, with_flags = (0, 7)[(c // 6) % 2], c % 4 != 3
        for key, v in (('n_read', n_read), ('n_sa', n_sa), ('n_ea', n_ea), ('end_size', end_size), ('extra', extra),
                       ('min_trim', min_trim), ('thr', thr), ('pad', pad), ('flags', with_flags)):
            used[key, v] += 1
        tabs = [_end_side(rng, n, n_read, pad, side, end_size, min_trim) for side, n in enumerate((n_sa, n_ea))]
        exp = [_expected_end_side(t, n, n_read, side, end_size, extra, thr, min_trim, seen)
               for side, (t, n) in enumerate(zip(tabs, (n_sa, n_ea)))]
        d_tabs = [_dev(t) for t in tabs]
        d_trim = [_dev(np.full(n_read + 8, JUNK, np.int32)) for _ in range(2)]
        d_flag = [_dev(np.full(n * n_read + 8, 0xEE, np.uint8)) if with_flags else None for n in (n_sa, n_ea)]
        rc = gpu_lib.pcabi_end_trim_dev(_p(d_tabs[0]), n_sa * n_read + pad, n_sa, _p(d_tabs[1]), n_ea * n_read + pad,
                                        n_ea, n_read, end_size, extra, thr, min_trim, _p(d_trim[0]), _p(d_trim[1]),
                                        _p(d_flag[0]), _p(d_flag[1]), _stream())
        assert rc == 0
        case = (c, n_read, n_sa, n_ea, end_size, extra, min_trim, thr, pad)
        for side, n_adp in enumerate((n_sa, n_ea)):
            trim, flags, rows = exp[side]
            got = _host(d_trim[side])
            assert got[:n_read].tolist() == trim, (case, side)
            assert (got[n_read:] == JUNK).all()
            if with_flags:
                got = _host(d_flag[side])
                assert np.array_equal(got[:n_adp * n_read], flags), (case, side)
                assert (got[n_adp * n_read:] == 0xEE).all()
                if n_adp:
                    _check_flag_list(gpu_lib, d_flag[side], flags, n_adp, n_read, d_tabs[side], n_adp * n_read + pad, rows)
    for key, values in (('n_read', N_READS), ('n_sa', N_ADPS), ('n_ea', N_ADPS), ('end_size', END_SIZES),
                        ('extra', EXTRAS), ('min_trim', MIN_TRIMS), ('thr', THRESHOLDS), ('pad', (0, 7)),
                        ('flags', (False, True))):
        assert all(used[key, v] for v in values), key
    for key in ('failed', 'nan', 'on_threshold', 'one_more', 'one_fewer', 'edge_start', 'edge_end', 'span_min_minus_1',
                'span_min', 'all_failed_reads', 'winner_wave_0', 'winner_wave_1', 'winner_wave_2', 'winner_wave_3',
                'winner_second_pass'):
        assert seen[key] >= 5, (key, dict(seen))


# ---- k_first_hit ------------------------------------------------------------------------------------

@pytest.mark.parametrize('n_adp', [1, 2, 98])
def test_first_hit(gpu_lib, n_adp):
    """pcabi_first_hit_dev against the first pass of find_middle_adapters' loop over the unmasked
    read (nanopore_read.py:226-252): the first adapter in list order whose full identity reaches
    the threshold, else (-1, -1, 0, 0, 0). Rows sit exactly on the threshold (3/4 at 75.0), fail,
    or lie below it; in some windows the first two adapters are both over it.

    The NaN rows (l2 == 0 with rs != -1) pin the kernel's own statement of the test, not the
    reference's. The reference line is :233, `if full_score >= middle_threshold:` ... `else:
    break`, under which a NaN identity would NOT hit; the kernel (and the oracle's loop,
    oracle_lib.middle_scan_windows) state it as `if full < threshold: break`, under which it
    does. The two agree on every row the DP can produce: a result with rs != -1 has l2 >= 1
    (alignment.cpp:55-56, :89-90) and a failed one scores 0.0 (nanopore_read.py:491-494), so no
    NaN reaches this compare. The expected values below follow the kernel's comment."""
    from collections import Counter
    rng = random.Random(7 + n_adp)
    thr = 75.0
    seen = Counter()
    for n_win in (0, 1, 255, 256, 257):
        pad = 3
        res = _table(n_adp, n_win, pad)
        for w in range(n_win):
            quiet = rng.random() < 0.3                 # no adapter reaches the threshold
            for a in range(n_adp):
                kind = rng.choice(('failed', 'below', 'below', 'below') + (() if quiet else ('on', 'over', 'nan')))
                if not quiet and a < 2 and rng.random() < 0.3:
                    kind = 'over'
                rs = rng.randint(0, 500)
                re = rs + rng.randint(0, 40)
                if kind == 'failed':
                    _set(res, a * n_win + w, -1, 20, 24, 24, 24)
                    continue
                m, l2 = {'below': (rng.randint(0, 17), 24), 'on': (3, 4), 'over': (rng.randint(19, 24), 24),
                         'nan': (0, 0)}[kind]
                _set(res, a * n_win + w, rs, re, m, max(l2, 1), l2)
        exp = np.zeros((5, n_win), np.int32)
        for w in range(n_win):
            hit, over = (-1, -1, 0, 0, 0), []
            for a in range(n_adp):
                rs, re, m, l2 = (int(res[f, a * n_win + w]) for f in (RS, RE, M, L2))
                full = 0.0 if rs == -1 else ref_pid6_scalar(m, l2)
                if not full < thr:
                    over.append(a)
                    if hit[0] == -1:
                        hit = (a, rs, re, m, l2)
                        seen['met_exactly'] += full == thr
                        seen['nan'] += full != full
            seen['none'] += hit[0] == -1
            seen['first_two_over'] += over[:2] == [0, 1]
            exp[:, w] = hit
        hit_stride = n_win + 5
        d_res, d_hits = _dev(res), _dev(np.full((5, hit_stride), JUNK, np.int32))
        assert gpu_lib.pcabi_first_hit_dev(_p(d_res), n_adp * n_win + pad, n_win, n_adp, thr, _p(d_hits), hit_stride,
                                           _stream()) == 0
        got = _host(d_hits)
        assert np.array_equal(got[:, :n_win], exp), n_win
        assert (got[:, n_win:] == JUNK).all()
    assert min(seen['met_exactly'], seen['none'], seen['nan']) >= 5, dict(seen)
    assert n_adp < 2 or seen['first_two_over'] >= 5


# ---- k_best_full_id ---------------------------------------------------------------------------------

@pytest.mark.parametrize('n_win', [0, 1, 255, 256, 257, 1000])
def test_best_full_identity(gpu_lib, n_win):
    """pcabi_best_full_identity_dev against `best = max(best, full_score)` over the windows
    (nanopore_read.py:166-168, :171-173; full_score 0.0 for a failed alignment, :491-494), with
    `best` pre-filled above and below the block's maximum, an adapter whose rows all failed (its
    `best` stays), and a stride larger than the block. No NaN rows: Python's max of a NaN depends
    on the order and the reference gives no rule."""
    rng = random.Random(n_win)
    n_adp, pad = 6, 5
    res = _table(n_adp, n_win, pad)
    for a in range(n_adp):
        for w in range(n_win):
            if a == 2 or rng.random() < 0.2:
                _set(res, a * n_win + w, -1, 20, 24, 24, 24)
            else:
                l2 = rng.randint(20, 30)
                _set(res, a * n_win + w, rng.randint(0, 100), 120, rng.randint(0, l2 - 1), l2, l2)
    best = np.array([0.0, 150.0, 12.5, 1e-6, 99.999999, 0.0])
    exp = best.tolist()
    for a in range(n_adp):
        for w in range(n_win):
            rs, m, l2 = (int(res[f, a * n_win + w]) for f in (RS, M, L2))
            exp[a] = max(exp[a], 0.0 if rs == -1 else ref_pid6_scalar(m, l2))
    if n_win >= 255:
        assert exp[0] > best[0] and exp[1] == best[1] and exp[2] == best[2] and exp[3] > best[3] and exp[4] == best[4]
    d_res, d_best = _dev(res), _dev(best)
    assert gpu_lib.pcabi_best_full_identity_dev(_p(d_res), n_adp * n_win + pad, n_win, n_adp, _p(d_best), _stream()) == 0
    assert _host(d_best).view(np.uint64).tolist() == np.array(exp).view(np.uint64).tolist()


# ---- k_trim_views -----------------------------------------------------------------------------------

@pytest.mark.parametrize('n_read', [0, 1, 257])
def test_trim_views(gpu_lib, n_read):
    """pcabi_trim_views_dev against get_seq_with_start_end_adapters_trimmed (nanopore_read.py:66-72):
    the slice seq[start_trim : len(seq) - end_trim], taken here from a range of the read's length
    with Python's own slicing. The trims add up to less than, exactly and more than the read, an
    end trim alone exceeds it (the stop goes negative and counts from the end), and the offsets
    lie above 2^32 (arithmetic only: nothing is read through them)."""
    from collections import Counter
    rng = random.Random(3 * n_read + 1)
    seen = Counter()
    off = np.array([rng.choice((0, 1 << 32, (1 << 40) + 12345, (1 << 33) - 7)) + rng.randint(0, 1000)
                    for _ in range(n_read)], np.int64)
    ln = np.array([rng.choice((0, 1, 100, 149, 151, 5000)) for _ in range(n_read)], np.int32)
    st, et = np.zeros(n_read, np.int32), np.zeros(n_read, np.int32)
    exp_off, exp_len = [], []
    for k in range(n_read):
        n = int(ln[k]) if n_read > 1 else 100
        ln[k] = n
        kind = ('below', 'equal', 'above', 'wrap', 'none', 'start_past')[k % 6] if n_read > 1 else 'wrap'
        s = rng.randint(0, n // 4 if kind == 'wrap' else n)
        e = {'below': rng.randint(0, max(n - s - 1, 0)), 'equal': n - s, 'above': n - s + rng.randint(1, 3),
             'wrap': n + rng.randint(1, max(n // 2, 1)), 'none': 0, 'start_past': rng.randint(0, 152)}[kind]
        if kind == 'none':
            s = 0
        if kind == 'start_past':
            s = n + rng.randint(1, 152)
        st[k], et[k] = s, e
        seq = range(n)
        view = seq if not s and not e else seq[s:n - e]
        seen['below'] += s + e < n
        seen['equal'] += s + e == n
        seen['above'] += s + e > n
        seen['wrapped_nonempty'] += e > n and len(view) > 0
        assert len(view) == 0 or view[0] == s
        exp_off.append(int(off[k]) + s)
        exp_len.append(len(view))
    d = [_dev(x) for x in (off, ln, st, et)]
    d_voff, d_vlen = _dev(np.full(n_read + 4, JUNK, np.int64)), _dev(np.full(n_read + 4, JUNK, np.int32))
    assert gpu_lib.pcabi_trim_views_dev(_p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), n_read, _p(d_voff), _p(d_vlen),
                                        _stream()) == 0
    voff, vlen = _host(d_voff), _host(d_vlen)
    assert vlen[:n_read].tolist() == exp_len
    assert voff[:n_read].tolist() == exp_off
    assert (voff[n_read:] == JUNK).all() and (vlen[n_read:] == JUNK).all()
    assert n_read == 0 or (min(exp_len) >= 0 and seen['wrapped_nonempty'] >= 1)
    assert n_read < 257 or (min(seen['below'], seen['equal'], seen['above']) >= 20 and max(off) > 1 << 32)
