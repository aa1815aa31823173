"""Timing of gzip output (GPU box): python tools/gz_timing.py [--reads 100000] [--out profiles/gz/gz_timing.json]

One batch of the e2e workload's FASTQ (synthetic reads of mean 8 kb, bench.py's write_fastq text),
parsed once, then written three ways, untrimmed, as wall clock around misc.write_reads (median of
--steps after --warmup):
  plain      the plain writer (gz = 0)
  zlib       the host path (gz = 1): on the first reads / --zlib-div reads of the batch, scaled
             linearly to the batch (zlib_scaled_s; zlib_sample_s is what was measured)
  device     gz = 2 on GPU 0, with the writer's own split of the call: layout (sizing, fill, block
             planning), compress, file write; and pcabi_gzip_host's split of compress: copy into
             pinned memory, waiting for the device, copy out of pinned memory (the three overlap
             with the device's work, so they add up to less than the parts run alone)
  parts      one 64 MiB chunk of the text alone through pinned memory on a stream: copy up, the four
             kernels (pcabi_gzip_dev), copy back; scaled to the batch as *_batch_s
and the three file sizes. Prints one JSON line (and writes it to --out)."""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from custom_porechop_abi_amd import _lib, engine, misc, synth  # noqa: E402


def write_fastq(path, reads, seed):
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b'ACGTN', np.uint8)
    with open(path, 'wb') as f:
        for k, r in enumerate(reads):
            q = (rng.integers(5, 40, len(r)) + 33).astype(np.uint8).tobytes()
            f.write(b'@read%d runid=synthetic ch=%d\n' % (k, k % 512) + letters[r].tobytes() + b'\n+\n' + q + b'\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reads', type=int, default=100000)
    ap.add_argument('--mean-len', type=int, default=8000)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--zlib-div', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    L = _lib.lib()
    tmp = tempfile.mkdtemp(prefix='pcabi_gz_')
    in_path = os.path.join(tmp, 'in.fastq')
    write_fastq(in_path, synth.make_reads(args.reads, args.mean_len, seed=12345), 99)
    b = misc.load_batch(in_path)
    os.remove(in_path)
    outs = {k: os.path.join(tmp, 'out.' + k) for k in ('fastq', 'z.fastq.gz', 'd.fastq.gz')}

    def last_times():
        a, c, w = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        L.pcabi_reads_write_last_times(ctypes.byref(a), ctypes.byref(c), ctypes.byref(w))
        i, s, o = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        L.pcabi_gzip_last_times(ctypes.byref(i), ctypes.byref(s), ctypes.byref(o))
        return np.array([a.value, c.value, w.value, i.value, s.value, o.value])

    def median(fn, steps=args.steps, warmup=args.warmup):
        for _ in range(warmup):
            fn()
        t, parts = [], []
        for _ in range(steps):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
            parts.append(last_times())
        return float(np.median(t)), np.median(np.array(parts), axis=0)

    t_plain, p_plain = median(lambda: misc.write_reads(b, outs['fastq'], 'fastq'))
    n_sample = max(1, b.n // args.zlib_div)
    sel = (np.arange(b.n) < n_sample).astype(np.uint8)
    t_zlib, _ = median(lambda: misc.write_reads(b, outs['z.fastq.gz'], 'fastq.gz', select=sel), steps=1, warmup=0)
    zlib_size_sample = os.path.getsize(outs['z.fastq.gz'])
    misc.write_reads(b, outs['fastq'], 'fastq', select=sel)
    sample_text = os.path.getsize(outs['fastq'])
    misc.write_reads(b, outs['fastq'], 'fastq')
    text_size = os.path.getsize(outs['fastq'])
    scale = text_size / sample_text
    t_dev, p_dev = median(lambda: misc.write_reads(b, outs['d.fastq.gz'], 'fastq.gz', gzip_device=0))
    dev_size = os.path.getsize(outs['d.fastq.gz'])

    # the parts alone, on one chunk
    chunk = min(text_size, 64 << 20)
    with open(outs['fastq'], 'rb') as f:
        text = np.frombuffer(f.read(chunk), np.uint8)
    off = engine.gzip_line_blocks(text)
    nb = off.size - 1
    bound, sb = L.pcabi_gzip_bound(chunk, nb), L.pcabi_gzip_scratch_bytes(chunk, nb)
    h_in = torch.from_numpy(text.copy()).pin_memory()
    h_off = torch.from_numpy(off).pin_memory()
    h_out = torch.empty(bound, dtype=torch.uint8).pin_memory()
    d_in = torch.empty(chunk, dtype=torch.uint8, device='cuda:0')
    d_off = torch.empty(off.size, dtype=torch.int64, device='cuda:0')
    d_out = torch.empty(bound, dtype=torch.uint8, device='cuda:0')
    d_len = torch.zeros(1, dtype=torch.int64, device='cuda:0')
    d_scr = torch.empty(sb, dtype=torch.uint8, device='cuda:0')
    st = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ms = []
    for _ in range(args.warmup + args.steps):
        ev[0].record()
        d_in.copy_(h_in, non_blocking=True)
        d_off.copy_(h_off, non_blocking=True)
        ev[1].record()
        _lib.check(L.pcabi_gzip_dev(ctypes.c_void_p(st.cuda_stream), d_in.data_ptr(), chunk, d_off.data_ptr(), nb,
                                    d_out.data_ptr(), bound, d_len.data_ptr(), d_scr.data_ptr(), sb), 'pcabi_gzip_dev')
        torch.cuda.synchronize()
        zn = int(d_len.item())
        ev[2].record()
        h_out[:zn].copy_(d_out[:zn], non_blocking=True)
        ev[3].record()
        torch.cuda.synchronize()
        ms.append((ev[0].elapsed_time(ev[1]), None, ev[2].elapsed_time(ev[3])))
        # the kernels alone, timed on their own
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(L.pcabi_gzip_dev(ctypes.c_void_p(st.cuda_stream), d_in.data_ptr(), chunk, d_off.data_ptr(), nb,
                                    d_out.data_ptr(), bound, d_len.data_ptr(), d_scr.data_ptr(), sb), 'pcabi_gzip_dev')
        e1.record()
        torch.cuda.synchronize()
        ms[-1] = (ms[-1][0], e0.elapsed_time(e1), ms[-1][2])
    up, kern, back = (float(x) * 1e-3 for x in np.median(np.array(ms[args.warmup:], float), axis=0))
    k = text_size / chunk
    import gzip
    ok = gzip.decompress(h_out[:zn].numpy().tobytes()) == text.tobytes()
    res = {
        'reads': b.n, 'text_bytes': text_size, 'plain_s': round(t_plain, 4),
        'plain_layout_s': round(float(p_plain[0]), 4), 'plain_file_write_s': round(float(p_plain[2]), 4),
        'zlib_sample_reads': n_sample, 'zlib_sample_s': round(t_zlib, 3), 'zlib_scaled_s': round(t_zlib * scale, 2),
        'zlib_scale': round(scale, 3), 'zlib_bytes_scaled': int(zlib_size_sample * scale),
        'device_s': round(t_dev, 4), 'device_bytes': dev_size,
        'device_layout_s': round(float(p_dev[0]), 4), 'device_compress_s': round(float(p_dev[1]), 4),
        'device_file_write_s': round(float(p_dev[2]), 4), 'compress_copy_in_s': round(float(p_dev[3]), 4),
        'compress_wait_s': round(float(p_dev[4]), 4), 'compress_copy_out_s': round(float(p_dev[5]), 4),
        'chunk_bytes': chunk, 'chunk_copy_up_s': round(up, 5), 'chunk_kernels_s': round(kern, 5),
        'chunk_copy_back_s': round(back, 5), 'copy_up_batch_s': round(up * k, 4), 'kernels_batch_s': round(kern * k, 4),
        'copy_back_batch_s': round(back * k, 4), 'kernels_GBps': round(chunk / kern / 1e9, 1),
        'chunk_roundtrip_ok': bool(ok),
        'zlib_over_device': round(t_zlib * scale / t_dev, 1), 'device_over_plain': round(t_dev / t_plain, 2),
        'ratio_plain_over_device_bytes': round(text_size / dev_size, 4),
        'ratio_plain_over_zlib_bytes': round(sample_text / zlib_size_sample, 4),
    }
    for p in outs.values():
        if os.path.exists(p):
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
