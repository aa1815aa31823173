"""ctypes access to a host build of csrc/pcabi_deflate.h (tests/deflate_cpu.cpp). TEST INFRASTRUCTURE ONLY."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, '_deflate_cpu.so')
HDR = os.path.join(os.path.dirname(HERE), 'custom_porechop_abi_amd', 'csrc', 'pcabi_deflate.h')

_lib = None


def build():
    src = os.path.join(HERE, 'deflate_cpu.cpp')
    if not os.path.isfile(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(HDR)):
        tmp = '%s.%d.tmp' % (SO, os.getpid())
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-Wall', '-o', tmp, src])
        os.replace(tmp, SO)
    return SO


def load():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build())
        P = ctypes.c_void_p
        L.dfl_plan_block.argtypes = [P] * 7
        L.dfl_plan_block.restype = None
        L.dfl_codes.argtypes = [P, ctypes.c_int, ctypes.c_int, P]
        L.dfl_codes.restype = None
        L.dfl_cl_order.restype = ctypes.c_int
        L.dfl_dyn_bytes.argtypes = [ctypes.c_uint32]
        L.dfl_dyn_bytes.restype = ctypes.c_uint32
        L.dfl_stored_bytes.argtypes = [ctypes.c_uint32]
        L.dfl_stored_bytes.restype = ctypes.c_uint32
        L.dfl_plan_lines.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, P, ctypes.c_int64]
        L.dfl_plan_lines.restype = ctypes.c_int64
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def plan_block(cnt256):
    """Literal counts (256) -> dict(lit_len[257], cl_len[19], cl_code[19], hclen4, hdr_bits, block_bits)."""
    L = load()
    cnt = np.ascontiguousarray(cnt256, np.uint32)
    assert cnt.size == 256
    lit_len, cl_len, cl_code = np.zeros(257, np.uint8), np.zeros(19, np.uint8), np.zeros(19, np.uint16)
    h, hb, bb = ctypes.c_int(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
    L.dfl_plan_block(_p(cnt), _p(lit_len), _p(cl_len), _p(cl_code), ctypes.addressof(h), ctypes.addressof(hb),
                     ctypes.addressof(bb))
    return dict(lit_len=lit_len, cl_len=cl_len, cl_code=cl_code, hclen4=h.value, hdr_bits=hb.value,
                block_bits=bb.value)


def codes(lengths, maxbits):
    """Canonical codes, bit-reversed for the LSB-first stream, of a length table."""
    L = load()
    ln = np.ascontiguousarray(lengths, np.uint8)
    out = np.zeros(ln.size, np.uint16)
    L.dfl_codes(_p(ln), ln.size, int(maxbits), _p(out))
    return out


def cl_order():
    L = load()
    return [L.dfl_cl_order(i) for i in range(19)]


def plan_lines(text, long_line, cap):
    """The writer's block list for text: int64 block_off."""
    L = load()
    nb = L.dfl_plan_lines(text, len(text), long_line, cap, None, 0)
    off = np.zeros(nb + 1, np.int64)
    L.dfl_plan_lines(text, len(text), long_line, cap, _p(off), off.size)
    return off
