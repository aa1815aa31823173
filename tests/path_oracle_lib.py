"""ctypes access to the oracle's gapped rows (tests/path_oracle.c). TEST INFRASTRUCTURE ONLY."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, '_path_oracle.so')

_lib = None


def build():
    src = os.path.join(HERE, 'path_oracle.c')
    dep = os.path.join(os.path.dirname(HERE), 'oracle', 'pcabi_oracle.c')
    if not os.path.isfile(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(dep)):
        tmp = '%s.%d.tmp' % (SO, os.getpid())
        subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-pthread', '-o', tmp, src])
        os.replace(tmp, SO)
    return SO


def load():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build())
        L.pcabi_path_oracle_rows.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int] + \
            [ctypes.c_int] * 4 + [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int]
        _lib = L
    return _lib


def rows(read, adapter, scheme):
    """(read row, adapter row) of one pair as the oracle's row builder leaves them: '-' for gaps,
    ACGTN letters (the way SeqAn prints Dna5). ('', '') for an empty input."""
    L = load()
    rb, ab = read.encode('utf-8'), adapter.encode('utf-8')
    cap = len(rb) + len(ab) + 2
    rr, ar = ctypes.create_string_buffer(cap), ctypes.create_string_buffer(cap)
    n = L.pcabi_path_oracle_rows(rb, len(rb), ab, len(ab), *[int(x) for x in scheme[:4]], rr, ar, cap)
    assert 0 <= n <= cap
    return rr.raw[:n].decode(), ar.raw[:n].decode()


def ops_of_rows(read_row, adapter_row):
    """One op per column (include/pcabi.h PCABI_OP_*), uint8."""
    r = np.frombuffer(read_row.encode(), np.uint8)
    a = np.frombuffer(adapter_row.encode(), np.uint8)
    gap = ord('-')
    return np.where(r == gap, 3, np.where(a == gap, 2, np.where(r == a, 0, 1))).astype(np.uint8)


def rle(ops):
    """ops -> uint32 runs (run_length << 2) | op, neighbouring runs of different ops."""
    ops = np.asarray(ops, np.uint8)
    if len(ops) == 0:
        return np.zeros(0, np.uint32)
    cut = np.flatnonzero(np.diff(ops)) + 1
    start = np.concatenate([[0], cut])
    length = np.diff(np.concatenate([start, [len(ops)]]))
    return ((length.astype(np.uint32) << 2) | ops[start]).astype(np.uint32)


def runs(read, adapter, scheme):
    """The run list of one pair, as pcabi_align_paths_* return it."""
    return rle(ops_of_rows(*rows(read, adapter, scheme)))
