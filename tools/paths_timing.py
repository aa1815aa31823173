"""Timing of the alignment-path call (GPU box): python tools/paths_timing.py [--reads 100000]

Start windows (150 bp) of synthetic reads, each paired with its best start adapter (largest full
identity over the start adapters of the first 50 adapter sets, from one cross product). Times, as
wall clock around each call (median of --steps after --warmup):
  paths_dev   pcabi_align_paths_dev, inputs and outputs resident on the device
  paths_host  pcabi_align_paths_host, host buffers (copies included)
  align_host  pcabi_align_host on the same pairs: the eight fields alone, host buffers
and the share of pairs whose trace went to device scratch instead of LDS. Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  (one HIP runtime)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from custom_porechop_abi_amd import _lib, adapters as A, engine, synth  # noqa: E402

SCORING = (3, -6, -5, -2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=100000)
    ap.add_argument('--end-size', type=int, default=150)
    ap.add_argument('--steps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    L = _lib.lib()
    vp = ctypes.c_void_p
    n = args.reads
    sets = [a for a in A.fresh_adapters() if '(full sequence)' not in a.name][:50]
    adps = sorted(set(a.start_sequence[1] for a in sets if a.start_sequence))
    reads = synth.make_reads(n, 8000, seed=12345, keep=args.end_size)
    codes, s_off, s_len, _, _ = synth.pack_end_windows(reads, args.end_size)
    win = (codes, np.ascontiguousarray(s_off, np.int64), np.ascontiguousarray(s_len, np.int32))
    res = engine.align(win, adps, SCORING)
    full = np.where(res[0] == -1, 0.0, engine.pid6(res[5], res[7])).reshape(len(adps), n)
    tw = np.arange(n, dtype=np.int32)
    ta = full.argmax(axis=0).astype(np.int32)
    ac, ao, al = engine.encode_adapters(adps)

    def ptr(a):
        return a.ctypes.data_as(vp)

    def median_ms(fn):
        for _ in range(args.warmup):
            fn()
        t = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(t))

    out = np.zeros((8, n), np.int32)
    run_off = np.zeros(n + 1, np.int64)
    cap = 64 * n
    runs = np.zeros(cap, np.uint32)

    def align_host():
        _lib.check(L.pcabi_align_host(0, ptr(codes), codes.size, ptr(win[1]), ptr(win[2]), n, ptr(ac), ptr(ao), ptr(al),
                                      len(al), ptr(tw), ptr(ta), n, *SCORING, ptr(out)), 'pcabi_align_host')

    def paths_host():
        total = L.pcabi_align_paths_host(0, ptr(codes), codes.size, ptr(win[1]), ptr(win[2]), n, ptr(ac), ptr(ao), ptr(al),
                                         len(al), ptr(tw), ptr(ta), n, *SCORING, ptr(out), ptr(run_off), ptr(runs), cap)
        if total < 0 or total > cap:
            _lib.check(int(min(total, -1)), 'pcabi_align_paths_host')
        return total

    bufs = []

    def dev(a):
        p = vp()
        _lib.check(L.pcabi_dev_malloc(ctypes.byref(p), max(a.nbytes, 16)), 'malloc')
        _lib.check(L.pcabi_dev_h2d(p, ptr(a), a.nbytes), 'h2d')
        bufs.append(p)
        return p

    d = [dev(x) for x in (codes, win[1], win[2], ac, ao, al, tw, ta, out, run_off, runs)]
    stream = vp()
    _lib.check(L.pcabi_stream_create(ctypes.byref(stream)), 'stream')

    def paths_dev():
        total = L.pcabi_align_paths_dev(d[0], d[1], d[2], n, d[3], d[4], d[5], len(al), d[6], d[7], n, *SCORING, d[8],
                                        d[9], d[10], cap, stream)
        if total < 0 or total > cap:
            _lib.check(int(min(total, -1)), 'pcabi_align_paths_dev')
        return total

    t_align = median_ms(align_host)
    fields = out.copy()
    t_host = median_ms(paths_host)
    same = bool(np.array_equal(fields, out))
    before = L.pcabi_paths_scratch_pairs()
    total = paths_dev()
    in_scratch = L.pcabi_paths_scratch_pairs() - before
    t_dev = median_ms(paths_dev)
    _lib.check(L.pcabi_stream_destroy(stream), 'stream destroy')
    for p in bufs:
        L.pcabi_dev_free(p)
    print(json.dumps({'pairs': n, 'adapters': len(adps), 'runs': int(total), 'runs_per_pair': round(total / n, 2),
                      'paths_dev_ms': round(t_dev, 3), 'paths_host_ms': round(t_host, 3),
                      'align_host_ms': round(t_align, 3), 'paths_dev_over_align_host': round(t_dev / t_align, 3),
                      'paths_host_over_align_host': round(t_host / t_align, 3),
                      'scratch_trace_share': round(in_scratch / n, 6), 'fields_equal_align_host': same}))


if __name__ == '__main__':
    main()
