"""Timing of the text writer with tags in its headers (GPU box): python tools/header_tags_timing.py
[--reads 100000] [--mean-len 1000] [--repeats 5] [--device 0] [--out profiles/bam/header_tags_timing_100k.json]

One synthetic batch (uniform ACGT, mean --mean-len, every read trimmed by 40 bases at both ends, so every
read is a changed read) as an unaligned BAM whose records carry CpG 5mC calls (MM C+m?, ML, MN), a move
table (mv, stride 5, geometric dwells of mean 2: about 2 moves per base), ts, ns and qs, read with keep_aux
and written four ways with keep_mods and keep_moves, after one warm-up of each, --repeats times in turn:
  (a) tags_device   misc.write_reads(..., 'fastq.gz', gzip_device=D, bgzf=True, header_tags=True): the remap,
                    k_auxtext_size, k_fastx_pack and the BGZF encoder on the device
  (b) tags_host     misc.write_reads(..., 'fastq', header_tags=True): the host build of the same text, not
                    compressed (zlib on one thread would drown every other figure)
  (c) bam_device    misc.write_reads(..., 'bam', gzip_device=D) of the same batch with the same options: the
                    nearest thing the writer could do before, the only meaningful baseline
  (d) today_device  misc.write_reads(..., 'fastq.gz', gzip_device=D, bgzf=True) without tags: today's text path
Wall clock around each call (they end synchronised), the median over the repeats; the device-event times of
k_auxtext_size and k_fastx_pack (medians) from --repeats more (a) calls with timing on, the bytes they moved
and the share of 8 TB/s that is. (a) is checked against (b): it must inflate to the same bytes. No figure is a
pass mark. Prints one JSON line (and writes it to --out)."""
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
    """-> (bases, moves, MM bytes, ML values)."""
    rng = np.random.default_rng(seed)
    code = np.array([1, 2, 4, 8], np.uint8)   # A C G T
    bases = moves = mm_bytes = ml_vals = 0
    with open(path, 'wb') as f:
        text = b'@HD\tVN:1.6\tSO:unknown\n'
        pending = [b'BAM\1' + struct.pack('<i', len(text)) + text + struct.pack('<i', 0)]
        size = len(pending[0])
        for k0 in range(0, n_reads, 512):   # the dwells of 512 reads drawn at once
            lens = np.maximum(200, rng.normal(mean_len, mean_len / 4, min(512, n_reads - k0))).astype(np.int64)
            first = np.concatenate(([0], np.cumsum(lens)))
            dwell = rng.geometric(0.5, int(first[-1]))
            start = np.concatenate(([0], np.cumsum(dwell)))
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
                is_c = s == 1
                cpg = np.flatnonzero(is_c[:-1] & (s[1:] == 2))
                ords = np.cumsum(is_c)[cpg] - 1
                gaps = np.diff(np.concatenate(([-1], ords))) - 1
                mm = b'C+m?' + b''.join(b',%d' % g for g in gaps) + b';'
                ml = rng.integers(0, 256, gaps.size).astype(np.uint8).tobytes()
                a, e = int(start[first[j]]), int(start[first[j + 1]])
                aux = (b'RGZgrp\0MMZ' + mm + b'\0MLBC' + struct.pack('<I', gaps.size) + ml + b'MNi' + struct.pack('<i', ln) +
                       b'tsi' + struct.pack('<i', 10 + k % 1000) + b'mvBc' + struct.pack('<I', 1 + e - a) + bytes([STRIDE]) +
                       mv_all[a:e].tobytes() + b'nsi' + struct.pack('<i', STRIDE * (e - a) + 10 + k % 1000) + b'qsC' + bytes([k % 200]))
                name = b'read%d\0' % k
                body = struct.pack('<iiBBHHHiiii', -1, -1, len(name), 0, 4680, 0, 4, ln, -1, -1, 0) + name + packed + qual + aux
                pending.append(struct.pack('<i', len(body)) + body)
                size += len(body) + 4
                bases += ln
                moves += e - a
                mm_bytes += len(mm)
                ml_vals += gaps.size
                if size > (64 << 20):
                    bgzf_stored(pending, f)
                    pending, size = [], 0
        bgzf_stored(pending, f)
    misc.bgzf_finish(path)
    return bases, moves, mm_bytes, ml_vals


def kernel_times(L, on, reset):
    ms, nbytes = (ctypes.c_double * 2)(), (ctypes.c_int64 * 2)()
    L.pcabi_auxtext_last_times(int(on), int(reset), ms, nbytes)
    return [float(x) for x in ms], [int(x) for x in nbytes]


def measure(L, args, tmp):
    src = os.path.join(tmp, 'in.bam')
    bases, moves, mm_bytes, ml_vals = make_bam(src, args.reads, args.mean_len)
    b = misc.load_batch(src, keep_aux=True)
    os.remove(src)
    trim = np.full(b.n, TRIM, np.int32)
    dev = args.device
    paths = {k: os.path.join(tmp, 'out_' + k) for k in 'abcd'}
    tags = {'start_trim': trim, 'end_trim': trim, 'keep_aux': True, 'keep_mods': True, 'keep_moves': True}
    calls = {'a': lambda: misc.write_reads(b, paths['a'], 'fastq.gz', gzip_device=dev, bgzf=True, header_tags=True, **tags),
             'b': lambda: misc.write_reads(b, paths['b'], 'fastq', header_tags=True, **tags),
             'c': lambda: misc.write_reads(b, paths['c'], 'bam', gzip_device=dev, **tags),
             'd': lambda: misc.write_reads(b, paths['d'], 'fastq.gz', gzip_device=dev, bgzf=True, start_trim=trim, end_trim=trim)}
    for k in sorted(calls):
        assert calls[k]() == b.n   # warm-up
    equal = None
    if args.check:
        with open(paths['b'], 'rb') as f:
            equal = inflate_all(paths['a']) == f.read()
    text_bytes = os.path.getsize(paths['b'])
    sizes = {k: os.path.getsize(paths[k]) for k in 'acd'}
    times = {k: [] for k in calls}
    for _ in range(args.repeats):
        for k in sorted(calls):
            t0 = time.perf_counter()
            calls[k]()
            times[k].append(time.perf_counter() - t0)
    engine.auxtext_counts(reset=True)
    kernel_times(L, 1, 1)
    prof = []
    for _ in range(args.repeats):   # timed calls of their own: the events are not in the wall figures
        calls['a']()
        prof.append(kernel_times(L, 1, 1))
    kernel_times(L, 0, 1)
    counts = engine.auxtext_counts(reset=True)
    ms = [float(np.median([p[0][k] for p in prof])) for k in range(2)]
    nbytes = prof[-1][1]
    gbps = [nbytes[k] / max(ms[k], 1e-9) / 1e6 for k in range(2)]
    med = {k: round(1e3 * float(np.median(v)), 2) for k, v in times.items()}
    res = {'reads': int(b.n), 'bases': int(bases), 'moves': int(moves), 'mm_bytes': int(mm_bytes), 'ml_values': int(ml_vals),
           'repeats': args.repeats, 'text_bytes': int(text_bytes), 'tags_device_file_bytes': sizes['a'], 'bam_device_file_bytes': sizes['c'],
           'today_device_file_bytes': sizes['d'],
           'tags_device_write_ms': med['a'], 'tags_host_plain_write_ms': med['b'], 'bam_device_write_ms': med['c'],
           'today_device_write_ms': med['d'], 'runs_ms': {k: [round(1e3 * x, 2) for x in v] for k, v in times.items()},
           'k_auxtext_size_ms': round(ms[0], 3), 'k_fastx_pack_ms': round(ms[1], 3),
           'kernel_runs_ms': [[round(x, 3) for x in p[0]] for p in prof], 'k_auxtext_size_bytes': nbytes[0], 'k_fastx_pack_bytes': nbytes[1],
           'k_auxtext_size_GBps': round(gbps[0], 1), 'k_auxtext_size_share_of_hbm_peak': round(gbps[0] / HBM_PEAK_GBPS, 4),
           'k_fastx_pack_GBps': round(gbps[1], 1), 'k_fastx_pack_share_of_hbm_peak': round(gbps[1] / HBM_PEAK_GBPS, 4),
           'tags_written_left_out_per_call': [counts[0] // args.repeats, counts[1] // args.repeats],
           'device_and_host_inflate_equal': equal}
    for p in paths.values():
        if os.path.exists(p):
            os.remove(p)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=100000)
    ap.add_argument('--mean-len', type=int, default=1000)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--check', type=int, default=1, help='compare the inflated bytes of (a) with (b)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    L = _lib.lib()
    tmp = tempfile.mkdtemp(prefix='pcabi_header_tags_')
    line = json.dumps(measure(L, args, tmp))
    print(line, flush=True)
    os.rmdir(tmp)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
