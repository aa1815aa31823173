"""Timing of block-gzipped input (GPU box): python tools/gunzip_timing.py [--reads 100000] [--div 20]
[--out profiles/gunzip/gunzip_timing_100k.json]

One batch of the e2e workload's FASTQ (synthetic reads of mean 8 kb, bench.py's write_fastq text),
parsed once, then
  literal  the whole batch written once as BGZF by this project's writer (misc.write_reads(...,
           gzip_device=0, bgzf=True) + misc.bgzf_finish: literal-only members, one distance code,
           no runs in the headers)
  level6   the first reads / --div reads of the batch re-blocked in 65280-byte blocks through zlib
           level 6 in Python (members with matches; zlib is too slow to make the whole batch so)
For each file, as wall clock around misc.load_batch (median of --steps after --warmup, the calls end
synchronised):
  zlib     the host path (pcabi_fastx_load, gzread on one thread)
  device   gunzip_device=0 (pcabi_fastx_open_dev: groups of members inflated on the GPU)
and around engine.gunzip (pcabi_gunzip_host) with its split: copy into pinned memory, waiting for the
device, copy out of pinned memory. Then one staged chunk alone on a stream, from device events: copy
up, k_inflate (pcabi_gunzip_dev), copy back, and the kernel's decoded GB/s. The chunk holds a multiple
of 512 members (two resident workgroups on each of 256 CUs), 4096 at the most, so that no partial
round of workgroups trails the others.
Prints one JSON line (and writes it to --out)."""
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


def write_fastq(path, reads, seed):
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b'ACGTN', np.uint8)
    with open(path, 'wb') as f:
        for k, r in enumerate(reads):
            q = (rng.integers(5, 40, len(r)) + 33).astype(np.uint8).tobytes()
            f.write(b'@read%d runid=synthetic ch=%d\n' % (k, k % 512) + letters[r].tobytes() + b'\n+\n' + q + b'\n')


def bgzf(text, level, strategy):
    out = []
    for lo in range(0, len(text), engine.BGZF_BLOCK_CAP):
        part = text[lo:lo + engine.BGZF_BLOCK_CAP]
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        p = c.compress(part) + c.flush()
        out.append(bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0]) + b'BC' + struct.pack('<HH', 2, len(p) + 25) +
                   p + struct.pack('<II', zlib.crc32(part), len(part)))
    return b''.join(out) + engine.BGZF_EOF


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
    tmp = tempfile.mkdtemp(prefix='pcabi_gunzip_')
    plain = os.path.join(tmp, 'in.fastq')
    write_fastq(plain, synth.make_reads(args.reads, args.mean_len, seed=12345), 99)
    batch = misc.load_batch(plain)
    n_sample = max(1, batch.n // args.div)
    sel = (np.arange(batch.n) < n_sample).astype(np.uint8)
    misc.write_reads(batch, plain, 'fastq', select=sel)
    sample_text = open(plain, 'rb').read()
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

    res = {'reads': batch.n, 'level6_reads': n_sample}
    for tag in ('literal', 'level6'):
        path = os.path.join(tmp, tag + '.fastq.gz')
        if tag == 'literal':
            misc.write_reads(batch, path, 'fastq.gz', gzip_device=0, bgzf=True)
            misc.bgzf_finish(path)
            n_reads = batch.n
        else:
            with open(path, 'wb') as f:
                f.write(bgzf(sample_text, 6, zlib.Z_DEFAULT_STRATEGY))
            n_reads = n_sample
        z = open(path, 'rb').read()
        assert misc.load_batch(path, gunzip_device=0).n == n_reads
        t_zlib = median(lambda: misc.load_batch(path))
        t_dev = median(lambda: misc.load_batch(path, gunzip_device=0))
        text = engine.gunzip(z)
        if tag == 'level6':
            assert text == sample_text
        t_host = median(lambda: engine.gunzip(z))
        a, w, o = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        L.pcabi_gunzip_last_times(ctypes.byref(a), ctypes.byref(w), ctypes.byref(o))
        in_off, out_off = engine.bgzf_index(z)
        members = int(in_off.size - 1)
        m = min(4096, members // 512 * 512) or members
        zb, ob = int(in_off[m]), int(out_off[m])
        # one staged chunk alone
        h_in = torch.from_numpy(np.frombuffer(z[:zb], np.uint8).copy()).pin_memory()
        h_out = torch.empty(ob, dtype=torch.uint8).pin_memory()
        d_in = torch.empty(zb, dtype=torch.uint8, device='cuda:0')
        d_out = torch.empty(ob, dtype=torch.uint8, device='cuda:0')
        d_io = torch.from_numpy(in_off[:m + 1].copy()).to('cuda:0')
        d_oo = torch.from_numpy(out_off[:m + 1].copy()).to('cuda:0')
        d_st = torch.zeros(m, dtype=torch.int32, device='cuda:0')
        st = torch.cuda.current_stream()
        ms = []
        for _ in range(args.warmup + args.steps):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            d_in.copy_(h_in, non_blocking=True)
            ev[1].record()
            _lib.check(L.pcabi_gunzip_dev(ctypes.c_void_p(st.cuda_stream), d_in.data_ptr(), zb, d_io.data_ptr(),
                                          d_oo.data_ptr(), m, d_out.data_ptr(), ob, d_st.data_ptr(), None, 0),
                       'pcabi_gunzip_dev')
            ev[2].record()
            h_out.copy_(d_out, non_blocking=True)
            ev[3].record()
            torch.cuda.synchronize()
            ms.append([ev[k].elapsed_time(ev[k + 1]) for k in range(3)])
        up, kern, back = (float(x) * 1e-3 for x in np.median(np.array(ms[args.warmup:], float), axis=0))
        ok = int(d_st.abs().sum().item()) == 0 and h_out.numpy().tobytes() == text[:ob]
        res.update({
            tag + '_text_bytes': len(text), tag + '_file_bytes': len(z), tag + '_members': members,
            tag + '_zlib_load_s': round(t_zlib, 4), tag + '_device_load_s': round(t_dev, 4),
            tag + '_zlib_over_device': round(t_zlib / t_dev, 2),
            tag + '_gunzip_host_s': round(t_host, 4), tag + '_copy_in_s': round(a.value, 4),
            tag + '_wait_s': round(w.value, 4), tag + '_copy_out_s': round(o.value, 4),
            tag + '_chunk_members': m, tag + '_chunk_decoded_bytes': ob, tag + '_chunk_copy_up_s': round(up, 5),
            tag + '_chunk_kernel_s': round(kern, 5), tag + '_chunk_copy_back_s': round(back, 5),
            tag + '_kernel_decoded_GBps': round(ob / kern / 1e9, 2), tag + '_chunk_ok': bool(ok),
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
