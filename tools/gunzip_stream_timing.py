"""Timing of ordinary (non-BGZF) gzip input (GPU box): python tools/gunzip_stream_timing.py
[--reads 100000] [--out profiles/gzstream/gunzip_stream_timing_100k.json]

One batch of the e2e workload's FASTQ (synthetic reads of mean 8 kb, bench.py's write_fastq text),
parsed once, then written as
  level6  one ordinary gzip member at zlib level 6, no index. To make 1.6 GB of it in seconds the text
          is compressed in 4 MiB pieces on a thread pool, every piece ended by a sync flush (what pigz
          writes): one deflate stream, whose matches do not reach across a piece's start
  gz2     this project's own '.gz' output of the batch (misc.write_reads(..., gzip_device=0):
          multi-member gzip, literal-only blocks)
For each file, as wall clock around misc.load_batch (median of --steps after --warmup, the calls end
synchronised):
  zlib    the host path (pcabi_fastx_load, gzread on one thread)
  device  gunzip_device=0, gunzip_plain=True (pcabi_fastx_open_dev2: spans inflated on the GPU)
and around engine.gunzip_stream (pcabi_gunzip_stream_host), then one more such call with device events
around every kernel (pcabi_gunzip_stream_last_times: each kernel waited for, so that call is not a
wall-clock figure): finder, counting pass, decode, window hand-down, resolve, summed over the spans,
and the stats line. Prints one JSON line (and writes it to --out)."""
import argparse
import ctypes
import json
import os
import struct
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch  # noqa: F401  (one HIP runtime per process)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from custom_porechop_abi_amd import _lib, engine, misc, synth  # noqa: E402


def write_fastq(path, reads, seed):
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b'ACGTN', np.uint8)
    with open(path, 'wb') as f:
        for k, r in enumerate(reads):
            q = (rng.integers(5, 40, len(r)) + 33).astype(np.uint8).tobytes()
            f.write(b'@read%d runid=synthetic ch=%d\n' % (k, k % 512) + letters[r].tobytes() + b'\n+\n' + q + b'\n')


def gzip_level6(text, piece=4 << 20, threads=16):
    """text as one gzip member at level 6, compressed piece by piece in parallel."""
    cuts = list(range(0, len(text), piece)) or [0]

    def one(lo):
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        return c.compress(text[lo:lo + piece]) + c.flush(zlib.Z_FINISH if lo == cuts[-1] else zlib.Z_SYNC_FLUSH)
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(one, cuts))
    return bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3]) + b''.join(parts) + struct.pack('<II', zlib.crc32(text), len(text) & 0xffffffff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=100000)
    ap.add_argument('--mean-len', type=int, default=8000)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--chunk-bytes', type=int, default=0)
    ap.add_argument('--span-bytes', type=int, default=0)
    ap.add_argument('--min-chunks', type=int, default=0)
    ap.add_argument('--sweep', default='', help='chunk:span[,chunk:span...]: engine.gunzip_stream of the level6 file under each')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    L = _lib.lib()
    _lib.check(L.pcabi_gunzip_stream_tune(args.chunk_bytes, args.span_bytes, args.min_chunks), 'pcabi_gunzip_stream_tune')
    tmp = tempfile.mkdtemp(prefix='pcabi_gzstream_')
    plain = os.path.join(tmp, 'in.fastq')
    write_fastq(plain, synth.make_reads(args.reads, args.mean_len, seed=12345), 99)
    batch = misc.load_batch(plain)
    text = open(plain, 'rb').read()
    os.remove(plain)

    def median(fn):
        for _ in range(args.warmup):
            fn()
        t = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        return float(np.median(t))

    def note(msg):
        print(msg, file=sys.stderr, flush=True)

    note('batch of %d reads, %d bytes of text' % (batch.n, len(text)))
    res = {'reads': batch.n, 'text_bytes': len(text), 'chunk_bytes': args.chunk_bytes, 'span_bytes': args.span_bytes,
           'min_chunks': args.min_chunks}
    for tag in ('level6', 'gz2'):
        path = os.path.join(tmp, tag + '.fastq.gz')
        if tag == 'level6':
            with open(path, 'wb') as f:
                f.write(gzip_level6(text))
        else:
            misc.write_reads(batch, path, 'fastq.gz', gzip_device=0)
        z = open(path, 'rb').read()
        assert engine.bgzf_index(z) is None
        assert misc.load_batch(path, gunzip_device=0, gunzip_plain=True).n == batch.n
        note('%s: %d bytes' % (tag, len(z)))
        t_zlib = median(lambda: misc.load_batch(path))
        note('%s: zlib load %.3f s' % (tag, t_zlib))
        t_dev = median(lambda: misc.load_batch(path, gunzip_device=0, gunzip_plain=True))
        reader_stats = engine.gunzip_stream_stats()
        note('%s: device load %.3f s' % (tag, t_dev))
        ok = engine.gunzip_stream(z) == text
        t_host = median(lambda: engine.gunzip_stream(z))
        ms = (ctypes.c_double * 5)()
        L.pcabi_gunzip_stream_last_times(1, 1, None)
        engine.gunzip_stream(z)
        L.pcabi_gunzip_stream_last_times(0, 0, ms)
        stats = engine.gunzip_stream_stats()
        if tag == 'level6' and args.sweep:
            sweep = {}
            for item in args.sweep.split(','):
                c, s = (int(x) for x in item.split(':'))
                _lib.check(L.pcabi_gunzip_stream_tune(c, s, args.min_chunks), 'pcabi_gunzip_stream_tune')
                sweep[item] = round(median(lambda: engine.gunzip_stream(z)), 4)
                note('%s: sweep %s %.3f s' % (tag, item, sweep[item]))
            _lib.check(L.pcabi_gunzip_stream_tune(args.chunk_bytes, args.span_bytes, args.min_chunks), 'pcabi_gunzip_stream_tune')
            res['level6_sweep_gunzip_stream_s'] = sweep
        res.update({
            tag + '_file_bytes': len(z), tag + '_ok': bool(ok), tag + '_zlib_load_s': round(t_zlib, 4),
            tag + '_device_load_s': round(t_dev, 4), tag + '_zlib_over_device': round(t_zlib / t_dev, 2),
            tag + '_gunzip_stream_s': round(t_host, 4),
            tag + '_kernel_ms': dict(zip(('finder', 'count', 'decode', 'handdown', 'resolve'), (round(float(x), 2) for x in ms))),
            tag + '_stats': stats, tag + '_reader_stats': reader_stats,
        })
        os.remove(path)
    os.rmdir(tmp)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
