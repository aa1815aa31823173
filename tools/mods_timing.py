"""Timing of the modification-tag remap in BAM output (GPU box): python tools/mods_timing.py
[--reads 100000] [--mean-len 8000] [--repeats 5] [--device 0] [--out profiles/bam/mods_timing.json]

One synthetic batch (uniform ACGT, mean --mean-len, every read trimmed by 40 bases at both ends, so every
read is a changed read) as an unaligned BAM whose records carry MM / ML / MN, under two tag loads:
  cpg   C+m? listing every C of a CG (about 1 % of the bases)
  6ma   A+a. listing every A
read with keep_aux and written to BAM three ways, after one warm-up of each, --repeats times in turn:
  (a) mods_device   misc.write_reads(..., 'bam', gzip_device=D, keep_aux=True, keep_mods=True)
  (b) drop_device   the same with keep_mods=False: the existing drop path, the baseline
  (c) mods_host     the table-level plan and remap of (a)'s reads with the host build on the io threads
                    (the write with gzip_device=None, keep_mods=True; only the remap's share is reported)
Wall clock around each call (they end synchronised), the median over the repeats; k_mods_plan's and
k_mods_write's device-event times (medians too), the bytes they read and wrote and that as a share of 8 TB/s,
from --repeats more (a) calls with profiling on; the host build's wall time from (c) and the wall time of (a)'s sizing step -- the aux blob and the
tables up, k_mods_plan, the lengths back, behind the letters' upload on the same stream -- (pcabi_mods_last_times). (a) is checked against (c): both must
inflate to the same bytes. reads_remapped_dropped counts over the profiled calls. --device -1 skips (a) and (b). Prints one JSON line per load (and writes them to
--out)."""
import argparse
import ctypes
import json
import os
import struct
import sys
import tempfile
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from custom_porechop_abi_amd import _lib, engine, misc  # noqa: E402

HBM_PEAK_GBPS = 8000.0


def bgzf_stored(chunks, f):
    """chunks of bytes as BGZF members of stored (level 0) deflate, 65280 decoded bytes each."""
    buf = b''.join(chunks)
    for lo in range(0, len(buf), 65280):
        piece = buf[lo:lo + 65280]
        c = zlib.compressobj(0, zlib.DEFLATED, -15)
        body = c.compress(piece) + c.flush()
        f.write(b'\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0' + struct.pack('<H', len(body) + 25) + body +
                struct.pack('<II', zlib.crc32(piece), len(piece)))


def make_bam(path, n_reads, mean_len, load, seed=7):
    """-> (bases, MM bytes, ML bytes)."""
    rng = np.random.default_rng(seed)
    code = np.array([1, 2, 4, 8], np.uint8)   # A C G T
    bases = mm_bytes = ml_bytes = 0
    with open(path, 'wb') as f:
        text = b'@HD\tVN:1.6\tSO:unknown\n'
        pending = [b'BAM\1' + struct.pack('<i', len(text)) + text + struct.pack('<i', 0)]
        size = len(pending[0])
        for k in range(n_reads):
            ln = int(max(200, rng.normal(mean_len, mean_len / 4)))
            s = rng.integers(0, 4, ln).astype(np.uint8)
            c = code[s]
            if ln & 1:
                c = np.append(c, np.uint8(0))
            packed = (c[0::2] << 4 | c[1::2]).tobytes()
            qual = rng.integers(5, 40, ln).astype(np.uint8).tobytes()
            if load == '6ma':
                n_ent = int((s == 0).sum())
                mm = b'A+a.' + b',0' * n_ent + b';'
            else:
                is_c = s == 1
                cpg = np.flatnonzero(is_c[:-1] & (s[1:] == 2))
                ords = np.cumsum(is_c)[cpg] - 1                      # the CpG C's ordinals among the C's
                gaps = np.diff(np.concatenate(([-1], ords))) - 1
                n_ent = gaps.size
                mm = b'C+m?' + b''.join(b',%d' % g for g in gaps) + b';'
            ml = rng.integers(0, 256, n_ent).astype(np.uint8).tobytes()
            aux = (b'RGZgrp\0MMZ' + mm + b'\0MLBC' + struct.pack('<I', n_ent) + ml + b'MNi' + struct.pack('<i', ln) +
                   b'qsC' + bytes([k % 200]))
            name = b'read%d\0' % k
            body = struct.pack('<iiBBHHHiiii', -1, -1, len(name), 0, 4680, 0, 4, ln, -1, -1, 0) + name + packed + qual + aux
            pending.append(struct.pack('<i', len(body)) + body)
            size += len(body) + 4
            bases += ln
            mm_bytes += len(mm)
            ml_bytes += n_ent
            if size > (64 << 20):
                bgzf_stored(pending, f)
                pending, size = [], 0
        bgzf_stored(pending, f)
    misc.bgzf_finish(path)
    return bases, mm_bytes, ml_bytes


def inflate_all(path):
    with open(path, 'rb') as f:
        data = f.read()
    out, at = [], 0
    while at < len(data):
        size = (data[at + 16] | data[at + 17] << 8) + 1
        out.append(zlib.decompress(data[at + 18:at + size - 8], -15))
        at += size
    return b''.join(out)


def mods_times(L, reset):
    ms, nbytes = (ctypes.c_double * 4)(), ctypes.c_int64()
    L.pcabi_mods_last_times(int(reset), ms, ctypes.byref(nbytes))
    return [float(x) for x in ms], int(nbytes.value)


def measure(L, load, args, tmp):
    src = os.path.join(tmp, 'in_%s.bam' % load)
    bases, mm_bytes, ml_bytes = make_bam(src, args.reads, args.mean_len, load)
    b = misc.load_batch(src, keep_aux=True)
    os.remove(src)
    trim = np.full(b.n, 40, np.int32)
    dev = None if args.device < 0 else args.device
    paths = {k: os.path.join(tmp, 'out_%s_%s' % (load, k)) for k in 'abc'}

    def write(k, device, keep_mods):
        return misc.write_reads(b, paths[k], 'bam', start_trim=trim, end_trim=trim, gzip_device=device, keep_aux=True,
                                keep_mods=keep_mods)

    calls = {'c': lambda: write('c', None, True)}
    if dev is not None:
        calls.update({'a': lambda: write('a', dev, True), 'b': lambda: write('b', dev, False)})
    times = {k: [] for k in calls}
    host_ms, plan_ms = [], []
    for k in sorted(calls):
        assert calls[k]() == b.n   # warm-up
    for _ in range(args.repeats):
        for k in sorted(calls):
            mods_times(L, True)
            t0 = time.perf_counter()
            calls[k]()
            times[k].append(time.perf_counter() - t0)
            if k == 'c':
                host_ms.append(mods_times(L, True)[0][2])
            if k == 'a':
                plan_ms.append(mods_times(L, True)[0][3])
    res = {'load': load, 'reads': int(b.n), 'bases': int(bases), 'mm_bytes': int(mm_bytes), 'ml_bytes': int(ml_bytes),
           'repeats': args.repeats, 'mods_host_write_ms': round(1e3 * float(np.median(times['c'])), 2),
           'host_remap_ms': round(float(np.median(host_ms)), 2), 'host_remap_runs_ms': [round(x, 2) for x in host_ms]}
    if dev is not None:
        engine.mods_counts(reset=True)
        L.pcabi_bam_last_times(1, 1, None, None)
        prof = []
        for _ in range(args.repeats):   # profiled calls of their own: the events are not in the wall figures
            mods_times(L, True)
            calls['a']()
            prof.append(mods_times(L, True))
        L.pcabi_bam_last_times(0, 1, None, None)
        ms = [float(np.median([p[0][k] for p in prof])) for k in range(2)]
        nbytes = prof[-1][1]
        kernel_ms = ms[0] + ms[1]
        a, bb = 1e3 * float(np.median(times['a'])), 1e3 * float(np.median(times['b']))
        res.update({'mods_device_write_ms': round(a, 2), 'drop_device_write_ms': round(bb, 2), 'device_remap_extra_ms': round(a - bb, 2),
                    'a_runs_ms': [round(1e3 * x, 2) for x in times['a']], 'b_runs_ms': [round(1e3 * x, 2) for x in times['b']],
                    'device_sizing_step_ms': round(float(np.median(plan_ms)), 2), 'k_mods_plan_ms': round(ms[0], 3), 'k_mods_write_ms': round(ms[1], 3),
                    'k_mods_plan_runs_ms': [round(p[0][0], 3) for p in prof], 'kernel_bytes': nbytes,
                    'kernel_GBps': round(nbytes / max(kernel_ms, 1e-9) / 1e6, 1),
                    'share_of_hbm_peak': round(nbytes / max(kernel_ms, 1e-9) / 1e6 / HBM_PEAK_GBPS, 4),
                    'reads_remapped_dropped': list(engine.mods_counts(reset=True)),
                    'a_and_c_inflate_equal': inflate_all(paths['a']) == inflate_all(paths['c']) if args.check else None})
    for p in paths.values():
        if os.path.exists(p):
            os.remove(p)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=100000)
    ap.add_argument('--mean-len', type=int, default=8000)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--loads', default='cpg,6ma')
    ap.add_argument('--check', type=int, default=1, help='compare the inflated bytes of (a) and (c)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    L = _lib.lib()
    tmp = tempfile.mkdtemp(prefix='pcabi_mods_')
    lines = []
    for load in args.loads.split(','):
        lines.append(json.dumps(measure(L, load, args, tmp)))
        print(lines[-1], flush=True)
    os.rmdir(tmp)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
