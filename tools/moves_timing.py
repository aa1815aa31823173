"""Timing of the move-table remap in BAM output (GPU box): python tools/moves_timing.py
[--reads 100000] [--mean-len 8000] [--repeats 3] [--device 0] [--out profiles/bam/moves_timing_100k.json]

One synthetic batch (uniform ACGT, mean --mean-len, every read trimmed by 40 bases at both ends, so every
read is a changed read) as an unaligned BAM whose records carry ts, mv (stride 5, geometric dwells of mean 2:
about 2 moves per base), ns and qs, read with keep_aux and written to BAM three ways, after one warm-up of
each, --repeats times in turn:
  (a) moves_device  misc.write_reads(..., 'bam', gzip_device=D, keep_aux=True, keep_moves=True)
  (b) drop_device   the same with keep_moves=False: the existing drop path, the baseline
  (c) moves_host    the write with gzip_device=None, keep_moves=True (only the remap's share, the host build on
                    the io threads, is reported beside the whole write)
Wall clock around each call (they end synchronised), the median over the repeats; the device-event times of
k_moves_count, the scan, k_moves_select with k_moves_size, and k_moves_write (medians too) from --repeats more
(a) calls with profiling on; the share of 8 TB/s they reach, taking 1 byte per move read by k_moves_count and
2 bytes per move kept by k_moves_write; the host build's wall time from (c) and the wall time of (a)'s sizing
step (pcabi_moves_last_times). (a) is checked against (c): both must inflate to the same bytes. --device -1
skips (a) and (b). Prints one JSON line (and writes it to --out)."""
import argparse
import ctypes
import json
import os
import struct
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from custom_porechop_abi_amd import _lib, engine, misc  # noqa: E402
from tools.mods_timing import bgzf_stored, inflate_all  # noqa: E402

HBM_PEAK_GBPS = 8000.0
STRIDE = 5
TRIM = 40


def make_bam(path, n_reads, mean_len, seed=7):
    """-> (bases, moves, moves kept by a trim of TRIM bases at both ends)."""
    rng = np.random.default_rng(seed)
    code = np.array([1, 2, 4, 8], np.uint8)   # A C G T
    bases = moves = kept = 0
    with open(path, 'wb') as f:
        text = b'@HD\tVN:1.6\tSO:unknown\n'
        pending = [b'BAM\1' + struct.pack('<i', len(text)) + text + struct.pack('<i', 0)]
        size = len(pending[0])
        for k0 in range(0, n_reads, 512):   # the dwells of 512 reads drawn at once
            lens = np.maximum(200, rng.normal(mean_len, mean_len / 4, min(512, n_reads - k0))).astype(np.int64)
            first = np.concatenate(([0], np.cumsum(lens)))
            dwell = rng.geometric(0.5, int(first[-1]))
            start = np.concatenate(([0], np.cumsum(dwell)))   # a base's first move; [-1]: all the moves
            mv_all = np.zeros(int(start[-1]), np.uint8)
            mv_all[start[:-1]] = 1
            for j, ln in enumerate(lens):
                ln, k = int(ln), k0 + j
                s = rng.integers(0, 4, ln).astype(np.uint8)
                c = code[s]
                if ln & 1:
                    c = np.append(c, np.uint8(0))
                packed = (c[0::2] << 4 | c[1::2]).tobytes()
                qual = rng.integers(5, 40, ln).astype(np.uint8).tobytes()
                a, e = int(start[first[j]]), int(start[first[j + 1]])
                aux = (b'RGZgrp\0tsi' + struct.pack('<i', 10 + k % 1000) + b'mvBc' + struct.pack('<I', 1 + e - a) + bytes([STRIDE]) +
                       mv_all[a:e].tobytes() + b'nsi' + struct.pack('<i', STRIDE * (e - a) + 10 + k % 1000) + b'qsC' + bytes([k % 200]))
                name = b'read%d\0' % k
                body = struct.pack('<iiBBHHHiiii', -1, -1, len(name), 0, 4680, 0, 4, ln, -1, -1, 0) + name + packed + qual + aux
                pending.append(struct.pack('<i', len(body)) + body)
                size += len(body) + 4
                bases += ln
                moves += e - a
                kept += int(start[first[j + 1] - TRIM]) - int(start[first[j] + TRIM])
                if size > (64 << 20):
                    bgzf_stored(pending, f)
                    pending, size = [], 0
        bgzf_stored(pending, f)
    misc.bgzf_finish(path)
    return bases, moves, kept


def moves_times(L, reset):
    ms, nbytes = (ctypes.c_double * 6)(), ctypes.c_int64()
    L.pcabi_moves_last_times(int(reset), ms, ctypes.byref(nbytes))
    return [float(x) for x in ms], int(nbytes.value)


def measure(L, args, tmp):
    src = os.path.join(tmp, 'in.bam')
    bases, moves, kept = make_bam(src, args.reads, args.mean_len)
    b = misc.load_batch(src, keep_aux=True)
    os.remove(src)
    trim = np.full(b.n, TRIM, np.int32)
    dev = None if args.device < 0 else args.device
    paths = {k: os.path.join(tmp, 'out_' + k) for k in 'abc'}

    def write(k, device, keep_moves):
        return misc.write_reads(b, paths[k], 'bam', start_trim=trim, end_trim=trim, gzip_device=device, keep_aux=True,
                                keep_moves=keep_moves)

    calls = {'c': lambda: write('c', None, True)}
    if dev is not None:
        calls.update({'a': lambda: write('a', dev, True), 'b': lambda: write('b', dev, False)})
    times = {k: [] for k in calls}
    host_ms, plan_ms = [], []
    for k in sorted(calls):
        assert calls[k]() == b.n   # warm-up
    for _ in range(args.repeats):
        for k in sorted(calls):
            moves_times(L, True)
            t0 = time.perf_counter()
            calls[k]()
            times[k].append(time.perf_counter() - t0)
            if k == 'c':
                host_ms.append(moves_times(L, True)[0][4])
            if k == 'a':
                plan_ms.append(moves_times(L, True)[0][5])
    res = {'reads': int(b.n), 'bases': int(bases), 'moves': int(moves), 'moves_kept': int(kept), 'repeats': args.repeats,
           'moves_host_write_ms': round(1e3 * float(np.median(times['c'])), 2),
           'host_remap_ms': round(float(np.median(host_ms)), 2), 'host_remap_runs_ms': [round(x, 2) for x in host_ms]}
    if dev is not None:
        engine.moves_counts(reset=True)
        L.pcabi_bam_last_times(1, 1, None, None)
        prof = []
        for _ in range(args.repeats):   # profiled calls of their own: the events are not in the wall figures
            moves_times(L, True)
            calls['a']()
            prof.append(moves_times(L, True))
        L.pcabi_bam_last_times(0, 1, None, None)
        ms = [float(np.median([p[0][k] for p in prof])) for k in range(4)]
        a, bb = 1e3 * float(np.median(times['a'])), 1e3 * float(np.median(times['b']))
        count_gbps, write_gbps = moves / max(ms[0], 1e-9) / 1e6, 2 * kept / max(ms[3], 1e-9) / 1e6
        res.update({'moves_device_write_ms': round(a, 2), 'drop_device_write_ms': round(bb, 2), 'device_remap_extra_ms': round(a - bb, 2),
                    'a_runs_ms': [round(1e3 * x, 2) for x in times['a']], 'b_runs_ms': [round(1e3 * x, 2) for x in times['b']],
                    'device_sizing_step_ms': round(float(np.median(plan_ms)), 2), 'k_moves_count_ms': round(ms[0], 3),
                    'scan_ms': round(ms[1], 3), 'k_moves_select_ms': round(ms[2], 3), 'k_moves_write_ms': round(ms[3], 3),
                    'kernel_runs_ms': [[round(x, 3) for x in p[0][:4]] for p in prof], 'kernel_bytes': prof[-1][1],
                    'k_moves_count_GBps': round(count_gbps, 1), 'k_moves_count_share_of_hbm_peak': round(count_gbps / HBM_PEAK_GBPS, 4),
                    'k_moves_write_GBps': round(write_gbps, 1), 'k_moves_write_share_of_hbm_peak': round(write_gbps / HBM_PEAK_GBPS, 4),
                    'reads_remapped_dropped': list(engine.moves_counts(reset=True)),
                    'a_and_c_inflate_equal': inflate_all(paths['a']) == inflate_all(paths['c']) if args.check else None})
    for p in paths.values():
        if os.path.exists(p):
            os.remove(p)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=100000)
    ap.add_argument('--mean-len', type=int, default=8000)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--check', type=int, default=1, help='compare the inflated bytes of (a) and (c)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    L = _lib.lib()
    tmp = tempfile.mkdtemp(prefix='pcabi_moves_')
    line = json.dumps(measure(L, args, tmp))
    print(line, flush=True)
    os.rmdir(tmp)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
