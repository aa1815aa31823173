"""Timing of the reader that parses SAM tags from FASTQ headers (GPU box): python tools/header_tags_read_timing.py
[--reads 100000] [--mean-len 1000] [--repeats 5] [--device 0] [--out profiles/bam/header_tags_read_timing_100k.json]

The workload of tools/header_tags_timing.py (uniform ACGT, mean --mean-len, CpG 5mC calls as MM C+m? / ML / MN,
a move table of stride 5 with about 2 moves per base, ts, ns, qs, RG) written as a plain FASTQ whose headers
carry those tags (misc.write_reads header_tags=True, no trims), then read three ways, after one warm-up of
each, --repeats times in turn:
  (a) tags_device   misc.load_batch(fastq, keep_aux=True, tags_from_headers=True, gunzip_device=D): the header
                    blob up, k_auxparse_size, k_auxparse_write, the chains and the floats' fix-ups back
  (b) tags_host     misc.load_batch(fastq, keep_aux=True, tags_from_headers=True): the host build on the io threads
  (c) no_tags       misc.load_batch(fastq): the reader with the option off, the code the reader ran before the
                    option existed; (a) - (c) and (b) - (c) are what the option adds
Wall clock around each call, the median over the repeats; the device-event times of the two kernels (medians)
from --repeats more (a) calls with timing on, the bytes they moved and the share of 8 TB/s that is. (a) is
checked against (b) and against the aux bytes of the BAM the FASTQ was made from (as their SAM text). No figure
is a pass mark. Prints one JSON line (and writes it to --out)."""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from custom_porechop_abi_amd import _lib, engine, misc  # noqa: E402
from tools.header_tags_timing import make_bam  # noqa: E402

HBM_PEAK_GBPS = 8000.0


def kernel_times(L, on, reset):
    ms, nbytes = (ctypes.c_double * 2)(), (ctypes.c_int64 * 2)()
    L.pcabi_auxparse_last_times(int(on), int(reset), ms, nbytes)
    return [float(x) for x in ms], [int(x) for x in nbytes]


def measure(L, args, tmp):
    bam, fq = os.path.join(tmp, 'in.bam'), os.path.join(tmp, 'in.fastq')
    bases, moves, mm_bytes, ml_vals = make_bam(bam, args.reads, args.mean_len)
    b = misc.load_batch(bam, keep_aux=True)
    os.remove(bam)
    assert misc.write_reads(b, fq, 'fastq', keep_aux=True, header_tags=True) == b.n
    dev = args.device
    calls = {'a': lambda: misc.load_batch(fq, keep_aux=True, tags_from_headers=True, gunzip_device=dev),
             'b': lambda: misc.load_batch(fq, keep_aux=True, tags_from_headers=True),
             'c': lambda: misc.load_batch(fq)}
    engine.auxparse_counts(reset=True)
    got = {k: calls[k]() for k in sorted(calls)}   # warm-up
    counts = engine.auxparse_counts(reset=True)
    header_bytes, chain_bytes = int(got['a'].name_off[-1]), int(got['a'].aux_off[-1])
    equal = None
    if args.check:
        equal = bool(np.array_equal(got['a'].aux_bytes, got['b'].aux_bytes) and np.array_equal(got['a'].aux_off, got['b'].aux_off))
        step = max(1, b.n // 2000)
        idx = list(range(0, b.n, step))
        equal = equal and engine.aux_text([got['a'].aux(i) for i in idx]) == engine.aux_text([b.aux(i) for i in idx])
    del got, b
    times = {k: [] for k in calls}
    for _ in range(args.repeats):
        for k in sorted(calls):
            t0 = time.perf_counter()
            x = calls[k]()
            times[k].append(time.perf_counter() - t0)
            del x
    kernel_times(L, 1, 1)
    prof = []
    for _ in range(args.repeats):   # timed calls of their own: the events are not in the wall figures
        x = calls['a']()
        del x
        prof.append(kernel_times(L, 1, 1))
    kernel_times(L, 0, 1)
    ms = [float(np.median([p[0][k] for p in prof])) for k in range(2)]
    nbytes = prof[-1][1]
    gbps = [nbytes[k] / max(ms[k], 1e-9) / 1e6 for k in range(2)]
    med = {k: round(1e3 * float(np.median(v)), 2) for k, v in times.items()}
    res = {'reads': int(args.reads), 'bases': int(bases), 'moves': int(moves), 'mm_bytes': int(mm_bytes), 'ml_values': int(ml_vals),
           'repeats': args.repeats, 'fastq_bytes': os.path.getsize(fq), 'header_bytes': header_bytes, 'chain_bytes': chain_bytes,
           'tags_device_load_ms': med['a'], 'tags_host_load_ms': med['b'], 'no_tags_load_ms': med['c'],
           'device_adds_ms': round(med['a'] - med['c'], 2), 'host_adds_ms': round(med['b'] - med['c'], 2),
           'runs_ms': {k: [round(1e3 * x, 2) for x in v] for k, v in times.items()},
           'k_auxparse_size_ms': round(ms[0], 3), 'k_auxparse_write_ms': round(ms[1], 3),
           'kernel_runs_ms': [[round(x, 3) for x in p[0]] for p in prof], 'k_auxparse_size_bytes': nbytes[0], 'k_auxparse_write_bytes': nbytes[1],
           'k_auxparse_size_GBps': round(gbps[0], 1), 'k_auxparse_size_share_of_hbm_peak': round(gbps[0] / HBM_PEAK_GBPS, 4),
           'k_auxparse_write_GBps': round(gbps[1], 1), 'k_auxparse_write_share_of_hbm_peak': round(gbps[1] / HBM_PEAK_GBPS, 4),
           'tags_read_left_out_per_call': [counts[0] // 2, counts[1] // 2], 'device_host_and_bam_agree': equal}
    os.remove(fq)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=100000)
    ap.add_argument('--mean-len', type=int, default=1000)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--check', type=int, default=1, help='compare (a) with (b) and with the BAM the FASTQ was made from')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    L = _lib.lib()
    tmp = tempfile.mkdtemp(prefix='pcabi_header_tags_read_')
    line = json.dumps(measure(L, args, tmp))
    print(line, flush=True)
    os.rmdir(tmp)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
