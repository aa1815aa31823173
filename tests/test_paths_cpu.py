"""Alignment paths, the CPU side: the row helper (tests/path_oracle.c, the oracle's own row builder),
engine.path_fields / path_rows / format_alignment over run lists, and the new ABI symbols. No GPU."""
import numpy as np
import pytest

from tests import oracle_lib, path_oracle_lib
from tests.test_gpu_freegap import FREE_SCHEMES
from tests.test_gpu_parity import SCHEMES, _case_set

DEFAULT = (3, -6, -5, -2)
# (read, adapter, read row, adapter row) under the default scheme, read off the oracle's row builder
KNOWN = [('ACGTACGTAC', 'GTAC', 'ACGTACGTAC', '--GTAC----'),
         ('GGGGGGGG', 'TTTT', '----GGGGGGGG', 'TTTT--------'),
         ('AC--GT', 'ACGT', 'ACNNGT', 'AC--GT'),
         ('A', 'C', '-A', 'C-'),
         ('TTACGGTACTT', 'ACGTAC', 'TTACGGTACTT', '--AC-GTAC--')]
PATH_SCHEMES = SCHEMES[:6] + FREE_SCHEMES[:4]


def _pairs():
    """About 2,000 (read, adapter, scheme) cases over the parity tests' case sets."""
    out = []
    for k, sc in enumerate(PATH_SCHEMES):
        reads, adps = _case_set(500 + k, 40, 5, 220, 128)
        out += [(r, a, sc) for r in reads for a in adps]
    return out


@pytest.fixture(scope='module')
def cases():
    return [(r, a, sc, path_oracle_lib.runs(r, a, sc)) for r, a, sc in _pairs()]


def test_known_rows():
    from custom_porechop_abi_amd import engine
    for read, adapter, rr, ar in KNOWN:
        assert path_oracle_lib.rows(read, adapter, DEFAULT) == (rr, ar)
        runs = path_oracle_lib.runs(read, adapter, DEFAULT)
        assert engine.path_rows(runs, read, adapter) == (rr, ar)
        assert engine.path_fields(runs) == [x for k, x in enumerate(oracle_lib.align(read, adapter, DEFAULT)) if k != 4]
    runs = path_oracle_lib.runs('TTACGGTACTT', 'ACGTAC', DEFAULT)
    assert runs.tolist() == [(2 << 2) | 2, (2 << 2) | 0, (1 << 2) | 2, (4 << 2) | 0, (2 << 2) | 2]
    assert engine.format_alignment(runs, 'TTACGGTACTT', 'ACGTAC') == 'TTACGGTACTT\n  || ||||  \n--AC-GTAC--'


def test_path_fields_equal_oracle_fields(cases):
    """ScoredAlignment's rules over the helper's runs give the oracle's seven non-score fields."""
    from custom_porechop_abi_amd import engine
    assert len(cases) >= 1900
    seen_empty = seen_degenerate = 0
    for read, adapter, sc, runs in cases:
        exp = oracle_lib.align(read, adapter, sc)
        assert engine.path_fields(runs) == exp[:4] + exp[5:], (read, adapter, sc)
        seen_empty += exp[0] == -1
        seen_degenerate += exp[0] != -1 and exp[6] == 0
    assert seen_empty and seen_degenerate


def test_runs_are_well_formed(cases):
    for read, adapter, sc, runs in cases:
        if not read:
            assert len(runs) == 0
            continue
        ops, lens = (runs & 3).astype(np.int64), (runs >> 2).astype(np.int64)
        assert (lens > 0).all() and (np.diff(ops) != 0).all()
        assert lens[ops != 3].sum() == len(read.encode()) and lens[ops != 2].sum() == len(adapter)
        assert len(runs) <= 2 * len(adapter) + 4       # the kernels' staging bound


def test_path_rows_round_trip(cases):
    from custom_porechop_abi_amd import engine
    for read, adapter, sc, runs in cases:
        assert engine.path_rows(runs, read, adapter) == path_oracle_lib.rows(read, adapter, sc)
    with pytest.raises(ValueError):
        engine.path_rows(path_oracle_lib.runs('ACGT', 'AC', DEFAULT), 'ACG', 'AC')


def test_abi_exports_path_entry_points():
    from custom_porechop_abi_amd import _lib
    names = _lib.exported_symbols()
    for name in ('pcabi_align_paths_host', 'pcabi_align_paths_dev', 'pcabi_adapter_profile_host',
                 'pcabi_adapter_profile_dev', 'pcabi_max_path_adapter_len'):
        assert name in names
    L = _lib.lib()
    assert L.pcabi_max_path_adapter_len() == 128
    assert L.pcabi_version() == 1


def test_path_arguments_refused_without_a_launch():
    """Bad arguments come back as PCABI_E_ARG from the arguments alone (no device is touched)."""
    from custom_porechop_abi_amd import _lib, engine
    pack = engine.SeqPack(['ACGTACGTAC'])
    win = pack.views([0], pack.lengths)
    with pytest.raises(_lib.PcabiError, match=r'\(-1\).*129 bases'):
        engine.align_paths(win, ['GTAC', 'A' * 129], DEFAULT, ([0], [0]))
    with pytest.raises(_lib.PcabiError, match=r'\(-1\).*task index'):
        engine.align_paths(win, ['GTAC'], DEFAULT, ([1], [0]))
    res, run_off, runs = engine.align_paths(win, ['GTAC'], DEFAULT, ([], []))
    assert res.shape == (8, 0) and run_off.tolist() == [0] and len(runs) == 0
