"""Timing of the quality stage (GPU box): python tools/qual_timing.py [--reads 100000] [--mean-len 8000]
[--repeats 3] [--device 0] [--file-reads 100000] [--out profiles/qual/qual_timing_100k.json]

The table level. One synthetic batch: --reads reads of mean --mean-len with qualities of Phred 15..39 and,
on every read, a head and a tail of 10..59 bases of Phred 0..4; window 10 at a mean of 10, min_length 1000,
min_mean_q 10. engine.quality_filter on the device and with the host build (device=-1, on the io threads),
after one warm-up of each, --repeats times in turn. Reported: the device-event times of k_qual_crop and
k_qual_sum (medians, from pcabi_qual_last_times) and the rate of k_qual_sum over the kept bytes against the
6.3 TB/s of HBM bandwidth that is achievable on an MI355X; the wall time of the device stage behind the
uploads (kernels, scan, records back) and of the whole call (blob up included) against the host build's.
The device's records must equal the host build's.

The whole file. --file-reads reads of bench.py's e2e workload (synth.make_reads, its FASTQ text) through
FileTrimmer.trim_file, FASTQ to FASTQ, with the stage on (window 10 at 10, min_length 1000, min_mean_q 7)
and off, as three alternating on / off pairs after one warm-up of each; the range seen is reported.
--file-reads 0 skips it. --device -1 runs the host build alone. Prints one JSON line (and writes it to --out).

--pieces [--share 0.05,1.0]: the piece stage on the same batch (engine.quality_filter_pieces). In the stated
share of the reads a middle adapter is planted: one cut range of 120 bases around the read's middle with 30
bases of Phred 0..4 on either side of it, so each such read gives two pieces that crop. Reported per share
(medians, from pcabi_qual_pieces_last_times): the plan kernels (keys, sort, count, scan, spans), k_qual_crop
and k_qual_sum over the piece spans, k_piece_cuts, the wall time of the device stage behind the uploads and
of the host build; beside them k_qual_crop / k_qual_sum over the whole reads from the same run. The device's
results must equal the host build's."""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401  (one HIP runtime: _lib.py)
from custom_porechop_abi_amd import _lib, adapters, engine, synth  # noqa: E402
from tools.gz_timing import write_fastq  # noqa: E402

HBM_ACHIEVABLE_GBPS = 6300.0
OPTS = dict(window=10, min_window_q=10.0, min_length=1000, min_mean_q=10.0)


def make_batch(n_reads, mean_len, seed=7):
    rng = np.random.default_rng(seed)
    lens = np.maximum(200, rng.normal(mean_len, mean_len / 4, n_reads)).astype(np.int64)
    off = np.concatenate(([0], np.cumsum(lens)))
    qual = (rng.integers(15, 40, int(off[-1]), dtype=np.uint8) + 33).astype(np.uint8)
    for side in (0, 1):
        n = rng.integers(10, 60, n_reads)
        for k in range(int(n.max())):   # the k-th base from each read's end, for the reads whose run is that long
            at = (off[:-1] + k if side == 0 else off[1:] - 1 - k)[n > k]
            qual[at] = rng.integers(33, 38, at.size, dtype=np.uint8)
    return qual, off[:-1].copy(), lens.astype(np.int32)


def qual_times(L, on, reset):
    ms, nbytes = (ctypes.c_double * 4)(), (ctypes.c_int64 * 2)()
    L.pcabi_qual_last_times(int(on), int(reset), ms, nbytes)
    return [float(x) for x in ms]


def table_level(L, args):
    qual, off, ln = make_batch(args.reads, args.mean_len)
    res = {'reads': int(ln.size), 'quality_bytes': int(qual.size), 'repeats': args.repeats, 'opts': OPTS}
    host = engine.quality_filter(qual, off, ln, device=-1, **OPTS)   # warm-up, and the reference
    res['kept_bytes'] = int(host['kept'].sum())
    res['cropped_reads'] = int((host['front'] + host['tail'] > 0).sum())
    res['failed_reads'] = int(((host['flags'] & engine.QUAL_FAIL) != 0).sum())
    host_ms, dev_ms, call_ms, kern = [], [], [], []
    if args.device >= 0:
        res['device_equals_host'] = bool(engine.quality_filter(qual, off, ln, device=args.device, **OPTS).tobytes() == host.tobytes())
    for _ in range(args.repeats):
        qual_times(L, 0, 1)
        engine.quality_filter(qual, off, ln, device=-1, **OPTS)
        host_ms.append(qual_times(L, 0, 1)[2])
        if args.device >= 0:
            t0 = time.perf_counter()
            engine.quality_filter(qual, off, ln, device=args.device, **OPTS)
            call_ms.append(1e3 * (time.perf_counter() - t0))
            dev_ms.append(qual_times(L, 1, 1)[3])
            engine.quality_filter(qual, off, ln, device=args.device, **OPTS)   # a call of its own with the events on
            kern.append(qual_times(L, 0, 1)[:2])
    res.update({'host_build_ms': round(float(np.median(host_ms)), 2), 'host_build_runs_ms': [round(x, 2) for x in host_ms]})
    if args.device >= 0:
        crop, summ = (float(np.median([k[j] for k in kern])) for j in (0, 1))
        gbps = res['kept_bytes'] / max(summ, 1e-9) / 1e6
        res.update({'k_qual_crop_ms': round(crop, 3), 'k_qual_sum_ms': round(summ, 3), 'kernel_runs_ms': [[round(x, 3) for x in k] for k in kern],
                    'k_qual_sum_GBps': round(gbps, 1), 'k_qual_sum_share_of_achievable_hbm': round(gbps / HBM_ACHIEVABLE_GBPS, 4),
                    'device_stage_ms': round(float(np.median(dev_ms)), 2), 'device_stage_runs_ms': [round(x, 2) for x in dev_ms],
                    'device_call_with_upload_ms': round(float(np.median(call_ms)), 2),
                    'host_over_device_stage': round(float(np.median(host_ms)) / max(float(np.median(dev_ms)), 1e-9), 1)})
    return res


def piece_times(L, on, reset):
    ms, nbytes = (ctypes.c_double * 6)(), (ctypes.c_int64 * 4)()
    L.pcabi_qual_pieces_last_times(int(on), int(reset), ms, nbytes)
    return [float(x) for x in ms]


def plant_cuts(qual, off, ln, share, seed=9):
    """A middle adapter's cut in `share` of the reads: -> (qual with low qualities beside the cuts, cut_off, cuts)."""
    rng = np.random.default_rng(seed)
    qual = qual.copy()
    hit = rng.random(ln.size) < share if share < 1.0 else np.ones(ln.size, bool)
    hit &= ln >= 400
    mid = ln.astype(np.int64) // 2
    for k in range(30):
        for at in (off[hit] + mid[hit] - 61 - k, off[hit] + mid[hit] + 60 + k):
            qual[at] = rng.integers(33, 38, at.size, dtype=np.uint8)
    cut_off = np.concatenate(([0], np.cumsum(hit))).astype(np.int64)
    cuts = np.stack([mid[hit] - 60, mid[hit] + 60], axis=1).reshape(-1).astype(np.int64)
    return qual, cut_off, cuts


def pieces_level(L, args):
    qual0, off, ln = make_batch(args.reads, args.mean_len)
    out = {}
    for share in [float(x) for x in args.share.split(',')]:
        qual, cut_off, cuts = plant_cuts(qual0, off, ln, share)
        run = lambda dev: engine.quality_filter_pieces(qual, off, ln, cut_off, cuts, device=dev, **OPTS)  # noqa: E731
        host = run(-1)
        res = {'split_reads': int(cut_off[-1]), 'pieces': int(host[2].size), 'piece_bytes': int((host[2]['end'] - host[2]['begin']).sum()),
               'pieces_cropped': int((host[2]['q']['front'] + host[2]['q']['tail'] > 0).sum()),
               'pieces_failed': int(((host[2]['q']['flags'] & engine.QUAL_FAIL) != 0).sum())}
        host_ms, dev_ms, kern, whole = [], [], [], []
        if args.device >= 0:
            dev = run(args.device)
            res['device_equals_host'] = all(a.tobytes() == b.tobytes() for a, b in zip(dev, host))
        for _ in range(args.repeats):
            piece_times(L, 0, 1)
            run(-1)
            host_ms.append(piece_times(L, 0, 1)[4])
            if args.device >= 0:
                run(args.device)
                dev_ms.append(piece_times(L, 1, 1)[5])
                run(args.device)                                       # a call of its own with the events on
                kern.append(piece_times(L, 0, 1)[:4])
                qual_times(L, 1, 1)
                engine.quality_filter(qual, off, ln, device=args.device, **OPTS)
                whole.append(qual_times(L, 0, 1)[:2])
        res['host_build_ms'] = round(float(np.median(host_ms)), 2)
        if args.device >= 0:
            med = [float(np.median([k[j] for k in kern])) for j in range(4)]
            res.update({'plan_kernels_ms': round(med[0], 3), 'piece_crop_ms': round(med[1], 3), 'piece_sum_ms': round(med[2], 3),
                        'k_piece_cuts_ms': round(med[3], 3), 'kernel_runs_ms': [[round(x, 3) for x in k] for k in kern],
                        'device_stage_ms': round(float(np.median(dev_ms)), 2), 'device_stage_runs_ms': [round(x, 2) for x in dev_ms],
                        'whole_read_crop_ms': round(float(np.median([w[0] for w in whole])), 3),
                        'whole_read_sum_ms': round(float(np.median([w[1] for w in whole])), 3)})
        out['share_%g' % share] = res
    return {'reads': int(ln.size), 'quality_bytes': int(qual0.size), 'repeats': args.repeats, 'opts': OPTS, 'pieces': out}


def whole_file(args, tmp):
    from custom_porechop_abi_amd.pipeline import FileTrimmer
    src = os.path.join(tmp, 'in.fastq')
    write_fastq(src, synth.make_reads(args.file_reads, args.mean_len, seed=12345), 99)
    sets = [a for a in adapters.fresh_adapters() if '(full sequence)' not in a.name][:50]
    base = (sets, (3, -6, -5, -2), 150, 75.0, 2, 4, 90.0, 10, 100, 1000)
    trimmers = {'off': FileTrimmer(*base, device=args.device),
                'on': FileTrimmer(*base, device=args.device, quality_window=10, quality_window_q=10.0, min_length=1000, min_mean_q=7.0)}
    times, counts = {'on': [], 'off': []}, {}
    try:
        for rep in range(4):   # the first pair warms up
            for k in ('on', 'off'):
                out = os.path.join(tmp, 'out_%s_%d.fastq' % (k, rep))
                t0 = time.perf_counter()
                counts[k] = trimmers[k].trim_file(src, out, 'fastq')
                if rep:
                    times[k].append(time.perf_counter() - t0)
                os.remove(out)
    finally:
        for t in trimmers.values():
            t.close()
    os.remove(src)
    ratio = [a / b for a, b in zip(times['on'], times['off'])]
    return {'file_reads': args.file_reads, 'file_on_s': [round(x, 3) for x in times['on']], 'file_off_s': [round(x, 3) for x in times['off']],
            'file_on_over_off': [round(x, 3) for x in ratio], 'file_counts_on': counts['on'], 'file_counts_off': counts['off']}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=100000)
    ap.add_argument('--mean-len', type=int, default=8000)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--file-reads', type=int, default=100000)
    ap.add_argument('--out', default=None)
    ap.add_argument('--pieces', action='store_true')
    ap.add_argument('--share', default='0.05,1.0')
    args = ap.parse_args()
    L = _lib.lib()
    res = pieces_level(L, args) if args.pieces else table_level(L, args)
    if args.file_reads > 0 and args.device >= 0 and not args.pieces:
        tmp = tempfile.mkdtemp(prefix='pcabi_qual_')
        res.update(whole_file(args, tmp))
        os.rmdir(tmp)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
