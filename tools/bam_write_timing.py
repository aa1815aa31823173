"""Timing of unaligned BAM output (GPU box): python tools/bam_write_timing.py [--reads 100000]
[--pairs 3] [--out profiles/bam/bam_write_timing_100k.json]

One batch of the e2e workload's reads (synthetic, mean 8 kb, random qualities) parsed from a plain FASTQ
file, then written whole (no trims) three ways, in alternating pairs after one warm-up of each:
  (a) bam_device    misc.write_reads(..., 'bam', gzip_device=0): k_bam_pack, then the BGZF encoder, on the device
  (b) fastq_bgzf    misc.write_reads(..., 'fastq.gz', gzip_device=0, bgzf=True): the existing gz = 3 writer
  (c) bam_host      misc.write_reads(..., 'bam'): the host build of the pack, zlib per member on the io threads
Wall clock around each call (they end synchronised), the median over the pairs; layout / compress /
write seconds of the last call from pcabi_reads_write_last_times; k_bam_pack's device-event time and
the bytes it read and wrote from one more profiled (a); the file sizes. (a) is checked against (c):
both must inflate to the same bytes. Prints one JSON line (and writes it to --out)."""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from custom_porechop_abi_amd import _lib, misc, synth  # noqa: E402


def inflate_all(path):
    with open(path, 'rb') as f:
        data = f.read()
    out, at = [], 0
    while at < len(data):
        size = (data[at + 16] | data[at + 17] << 8) + 1
        out.append(zlib.decompress(data[at + 18:at + size - 8], -15))
        at += size
    return b''.join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=100000)
    ap.add_argument('--mean-len', type=int, default=8000)
    ap.add_argument('--pairs', type=int, default=3)
    ap.add_argument('--check', type=int, default=1, help='compare the inflated bytes of (a) and (c)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    L = _lib.lib()
    rng = np.random.default_rng(99)
    letters = np.frombuffer(b'ACGTN', np.uint8)
    tmp = tempfile.mkdtemp(prefix='pcabi_bamw_')
    src = os.path.join(tmp, 'in.fastq')
    bases = 0
    with open(src, 'wb') as f:
        for k, r in enumerate(synth.make_reads(args.reads, args.mean_len, seed=12345)):
            q = (rng.integers(5, 40, len(r)) + 33).astype(np.uint8).tobytes()
            f.write(b'@read%d runid=synthetic ch=%d\n' % (k, k % 512) + letters[r].tobytes() + b'\n+\n' + q + b'\n')
            bases += len(r)
    b = misc.load_batch(src)
    os.remove(src)
    paths = {k: os.path.join(tmp, 'out_' + k) for k in 'abc'}
    calls = {'a': lambda: misc.write_reads(b, paths['a'], 'bam', gzip_device=0),
             'b': lambda: misc.write_reads(b, paths['b'], 'fastq.gz', gzip_device=0, bgzf=True),
             'c': lambda: misc.write_reads(b, paths['c'], 'bam')}
    times = {k: [] for k in calls}
    phases = {}

    def run(k, keep=True):
        t0 = time.perf_counter()
        n = calls[k]()
        dt = time.perf_counter() - t0
        assert n == b.n
        if keep:
            times[k].append(dt)
        t = (ctypes.c_double * 3)()
        L.pcabi_reads_write_last_times(ctypes.byref(t, 0), ctypes.byref(t, 8), ctypes.byref(t, 16))
        phases[k] = [round(float(x), 4) for x in t]

    for k in calls:
        run(k, keep=False)
    for _ in range(args.pairs):   # alternating pairs: (a, b), then (a, c)
        run('a')
        run('b')
        run('a')
        run('c')
    ms, nbytes = ctypes.c_double(), ctypes.c_int64()
    L.pcabi_bam_last_times(1, 1, None, None)
    L.pcabi_bam_pack_last_times(1, None, None)
    run('a', keep=False)
    L.pcabi_bam_pack_last_times(1, ctypes.byref(ms), ctypes.byref(nbytes))
    L.pcabi_bam_last_times(0, 1, None, None)
    same = None
    if args.check:
        same = inflate_all(paths['a']) == inflate_all(paths['c'])
    med = {k: float(np.median(v)) for k, v in times.items()}
    res = {
        'reads': int(b.n), 'bases': int(bases), 'pairs': args.pairs,
        'a_bam_device_s': round(med['a'], 4), 'b_fastq_bgzf_device_s': round(med['b'], 4), 'c_bam_host_s': round(med['c'], 4),
        'a_over_b': round(med['a'] / med['b'], 3), 'c_over_a': round(med['c'] / med['a'], 2),
        'a_runs_s': [round(x, 4) for x in times['a']], 'b_runs_s': [round(x, 4) for x in times['b']],
        'c_runs_s': [round(x, 4) for x in times['c']],
        'a_layout_compress_write_s': phases['a'], 'b_layout_compress_write_s': phases['b'],
        'c_layout_compress_write_s': phases['c'],
        'k_bam_pack_ms': round(ms.value, 3), 'k_bam_pack_bytes': int(nbytes.value),
        'k_bam_pack_GBps': round(nbytes.value / max(ms.value, 1e-9) / 1e6, 1),
        'k_bam_pack_share_of_compress': round(ms.value * 1e-3 / max(phases['a'][1], 1e-9), 4),
        'bam_device_file_bytes': os.path.getsize(paths['a']), 'fastq_bgzf_file_bytes': os.path.getsize(paths['b']),
        'bam_host_file_bytes': os.path.getsize(paths['c']), 'a_and_c_inflate_equal': same,
    }
    for p in paths.values():
        os.remove(p)
    os.rmdir(tmp)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
