"""Timing of unaligned BAM input (GPU box): python tools/bam_timing.py [--reads 100000] [--div 20]
[--out profiles/bam/bam_timing_100k.json]

The e2e workload's reads (synthetic, mean 8 kb) with random qualities, as a BAM file and as a BGZF FASTQ
file, both in 65,280-byte blocks at zlib level 6. zlib in Python is too slow to compress the whole
input, so the members are made from a SAMPLE of reads / --div reads and TILED --div times behind the
BAM header (each copy of the sample's members starts at a record boundary, so the chain stays valid;
read names repeat). Wall clock around misc.load_batch, median of --steps after --warmup, the calls end
synchronised:
  (a) fastq_device  the BGZF FASTQ with gunzip_device=0 (what the reader could do before BAM input)
  (b) bam_host      the BAM on the host path (gzread, records unpacked by the host build)
  (c) bam_device    the BAM with gunzip_device=0 (k_inflate, then k_bam_unpack next to the bytes)
For (c), summed over the groups from device events (pcabi_bam_last_times): k_inflate, k_bam_unpack,
the copies to the device (compressed bytes, tables, the window's device-to-device moves) and from it
(inflated bytes, status, the three outputs); inflate of one group overlaps the unpack of the one
before, so the sums are device time, not wall clock. Then k_bam_unpack alone on one stream
(pcabi_bam_unpack_dev over a few copies of the sample, device events): bytes read and written over its
time, against the HBM peak, and the host build of the same unpack over the same records (one thread;
scaled to the whole input by reads). Prints one JSON line (and writes it to --out)."""
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
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from custom_porechop_abi_amd import _lib, engine, misc, synth  # noqa: E402

HBM_PEAK_GBPS = 8000.0   # MI355X: 8 TB/s


def members(data, level=6):
    out = []
    for lo in range(0, len(data), engine.BGZF_BLOCK_CAP):
        part = data[lo:lo + engine.BGZF_BLOCK_CAP]
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 9)
        p = c.compress(part) + c.flush()
        out.append(bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0]) + b'BC' + struct.pack('<HH', 2, len(p) + 25) +
                   p + struct.pack('<II', zlib.crc32(part), len(part)))
    return b''.join(out)


def bam_record(name, codes, qual):
    """One unaligned record: codes = Dna5 (0..4), qual = Phred bytes."""
    nib = np.array([1, 2, 4, 8, 15], np.uint8)[codes]
    if nib.size % 2:
        nib = np.append(nib, np.uint8(0))
    packed = (nib[0::2] << 4 | nib[1::2]).astype(np.uint8).tobytes()
    body = struct.pack('<iiBBHHHiiii', -1, -1, len(name) + 1, 0, 4680, 0, 4, len(codes), -1, -1, 0) + name + b'\0' + \
        packed + qual.tobytes()
    return struct.pack('<i', len(body)) + body


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=100000)
    ap.add_argument('--div', type=int, default=20)
    ap.add_argument('--mean-len', type=int, default=8000)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    L = _lib.lib()
    n_sample = max(1, args.reads // args.div)
    reads = synth.make_reads(n_sample, args.mean_len, seed=12345)
    rng = np.random.default_rng(99)
    letters = np.frombuffer(b'ACGTN', np.uint8)
    fq, recs = [], []
    for k, r in enumerate(reads):
        q = rng.integers(5, 40, len(r)).astype(np.uint8)
        name = b'read%d' % k
        fq.append(b'@' + name + b'\n' + letters[r].tobytes() + b'\n+\n' + (q + 33).astype(np.uint8).tobytes() + b'\n')
        recs.append(bam_record(name, np.asarray(r), q))
    fq_text, rec_bytes = b''.join(fq), b''.join(recs)
    header = b'BAM\1' + struct.pack('<i', 11) + b'@HD\tVN:1.6\n' + struct.pack('<i', 0)
    tmp = tempfile.mkdtemp(prefix='pcabi_bam_')
    fq_path, bam_path = os.path.join(tmp, 'in.fastq.gz'), os.path.join(tmp, 'in.bam')
    with open(fq_path, 'wb') as f:
        f.write(members(fq_text) * args.div + engine.BGZF_EOF)
    with open(bam_path, 'wb') as f:
        f.write(members(header) + members(rec_bytes) * args.div + engine.BGZF_EOF)
    n_reads = n_sample * args.div
    bases = int(sum(len(r) for r in reads)) * args.div

    def median(fn):
        for _ in range(args.warmup):
            fn()
        t = []
        for _ in range(args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        return float(np.median(t))

    a = misc.load_batch(fq_path, gunzip_device=0)
    c = misc.load_batch(bam_path, gunzip_device=0)
    same = a.n == c.n == n_reads and np.array_equal(a.seq, c.seq) and np.array_equal(a.qual, c.qual) and \
        np.array_equal(a.codes, c.codes) and np.array_equal(a.code_off, c.code_off)
    b = misc.load_batch(bam_path)
    same = bool(same and np.array_equal(b.seq, c.seq) and np.array_equal(b.qual, c.qual) and np.array_equal(b.codes, c.codes))
    del a, b, c
    t_a = median(lambda: misc.load_batch(fq_path, gunzip_device=0))
    t_b = median(lambda: misc.load_batch(bam_path))
    t_c = median(lambda: misc.load_batch(bam_path, gunzip_device=0))
    # (c) once more with device events around every kernel and copy
    ms, nbytes = (ctypes.c_double * 4)(), ctypes.c_int64()
    L.pcabi_bam_last_times(1, 1, None, None)
    t0 = time.perf_counter()
    misc.load_batch(bam_path, gunzip_device=0)
    t_prof = time.perf_counter() - t0
    L.pcabi_bam_last_times(0, 1, ms, ctypes.byref(nbytes))
    dev_ms = [float(x) for x in ms]
    total = sum(dev_ms) or 1.0

    # k_bam_unpack alone: a few copies of the sample's records on the device
    copies = max(1, min(args.div, (256 << 20) // max(1, len(rec_bytes))))
    raw = header + rec_bytes * copies
    table, totals = engine.bam_index(raw)
    d_raw = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to('cuda:0')
    d_tab = torch.from_numpy(table.view(np.uint8).copy()).to('cuda:0')
    d_out = [torch.empty(int(totals[k]) + 64, dtype=torch.uint8, device='cuda:0') for k in range(3)]
    st = torch.cuda.current_stream()
    kms = []
    for _ in range(args.warmup + args.steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        _lib.check(L.pcabi_bam_unpack_dev(ctypes.c_void_p(st.cuda_stream), d_raw.data_ptr(), len(raw), d_tab.data_ptr(),
                                          table.size, int(totals[4]), d_out[0].data_ptr(), int(totals[0]),
                                          d_out[1].data_ptr(), int(totals[1]), d_out[2].data_ptr(), int(totals[2]),
                                          int(totals[2]) - 16), 'pcabi_bam_unpack_dev')
        ev[1].record()
        torch.cuda.synchronize()
        kms.append(ev[0].elapsed_time(ev[1]))
    k_s = float(np.median(kms[args.warmup:])) * 1e-3
    ln = table['l_seq'].astype(np.int64)
    moved = int(((ln + 1) // 2 + ln).sum() + 2 * ln.sum() + int(totals[2]) + table.nbytes)
    h_seq, h_qual, h_codes = engine.bam_unpack(raw, table, totals, device=-1)
    # the host build of the same unpack over the same records, one thread, into touched buffers
    t_host_unpack = median(lambda: engine.bam_unpack(raw, table, totals, device=-1, out=(h_seq, h_qual, h_codes)))
    ok = bool(np.array_equal(d_out[0][:int(totals[0])].cpu().numpy(), h_seq) and
              np.array_equal(d_out[1][:int(totals[1])].cpu().numpy(), h_qual) and
              np.array_equal(d_out[2][:int(totals[2])].cpu().numpy(), h_codes))
    res = {
        'reads': n_reads, 'bases': bases, 'sample_reads': n_sample, 'tiled': args.div, 'block_bytes': engine.BGZF_BLOCK_CAP,
        'level': 6, 'fastq_file_bytes': os.path.getsize(fq_path), 'bam_file_bytes': os.path.getsize(bam_path),
        'fastq_text_bytes': len(fq_text) * args.div, 'bam_inflated_bytes': len(header) + len(rec_bytes) * args.div,
        'batches_equal': same,
        'a_fastq_device_load_s': round(t_a, 4), 'b_bam_host_load_s': round(t_b, 4), 'c_bam_device_load_s': round(t_c, 4),
        'b_over_c': round(t_b / t_c, 2), 'a_over_c': round(t_a / t_c, 2),
        'c_profiled_load_s': round(t_prof, 4),
        'c_k_inflate_ms': round(dev_ms[0], 2), 'c_k_bam_unpack_ms': round(dev_ms[1], 2),
        'c_copies_to_device_ms': round(dev_ms[2], 2), 'c_copies_from_device_ms': round(dev_ms[3], 2),
        'c_share_k_inflate': round(dev_ms[0] / total, 3), 'c_share_k_bam_unpack': round(dev_ms[1] / total, 3),
        'c_share_copies': round((dev_ms[2] + dev_ms[3]) / total, 3),
        'c_k_bam_unpack_bytes': int(nbytes.value),
        'c_k_bam_unpack_GBps': round(nbytes.value / max(dev_ms[1], 1e-9) / 1e6, 1),
        'alone_records': int(table.size), 'alone_bases': int(ln.sum()), 'alone_bytes_moved': moved,
        'alone_k_bam_unpack_s': round(k_s, 6), 'alone_k_bam_unpack_GBps': round(moved / k_s / 1e9, 1),
        'alone_share_of_hbm_peak': round(moved / k_s / 1e9 / HBM_PEAK_GBPS, 3), 'hbm_peak_GBps': HBM_PEAK_GBPS,
        'alone_host_unpack_s': round(t_host_unpack, 4),
        'host_unpack_whole_input_s_scaled': round(t_host_unpack * args.div / copies, 3),
        'alone_ok': ok,
    }
    os.remove(fq_path)
    os.remove(bam_path)
    os.rmdir(tmp)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
