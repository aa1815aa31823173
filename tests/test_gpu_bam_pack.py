"""Unaligned BAM output on the GPU: k_bam_pack (engine.bam_pack(device=0)) against the host build of the
same code, the writer's device path (misc.write_reads(..., 'bam', gzip_device=0)) against its host path,
and FileTrimmer BAM to BAM."""
import os

import numpy as np
import pytest

from tests import bam_lib as B
from tests import bam_pack_lib as P
from tests import golden_lib

pytestmark = pytest.mark.gpu

DATA = os.path.join(golden_lib.GOLDEN, 'data')


def _write(tmp_path, name, data):
    p = str(tmp_path / name)
    with open(p, 'wb') as f:
        f.write(data)
    return p


# ---- 1. the kernel against the host build --------------------------------------------------------------
@pytest.mark.parametrize('shift', [0, 1, 9])
def test_kernel_matches_host_and_record_bytes(gpu_lib, shift):
    """The part corpus (tile edges, 16-byte pieces, odd lengths, l_seq == 0) through engine.bam_pack on
    the device and with the host build. shift moves the output off a 16-byte boundary (the device output
    starts as far off one as the caller's pointer); the entry point checks its 64 guard bytes, and the
    bytes no part owns keep their 0xA5."""
    from custom_porechop_abi_amd import engine
    seq, qual, side, parts, records = P.pack_corpus()
    planned, end = P.planned_with_gaps(parts)
    size = end + 7

    def run(device):
        raw = np.full(size + 32, 0xA5, np.uint8)
        at = (-raw.ctypes.data) % 16 + shift
        out = raw[at:at + size]
        assert out.ctypes.data % 16 == shift
        engine.bam_pack(seq, qual, side, planned, out, device=device)
        assert (raw[:at] == 0xA5).all() and (raw[at + size:] == 0xA5).all()
        return out.copy()

    host, dev = run(-1), run(0)
    bad = np.flatnonzero(host != dev)
    assert bad.size == 0, (bad[:8], host[bad[:8]], dev[bad[:8]])
    assert np.array_equal(dev, P.expected_image(planned, records, size))


def test_kernel_skips_parts_outside_the_buffers(gpu_lib):
    """pcabi_bam_pack_dev with a table whose parts point outside a buffer: those parts write nothing, the
    others are written (the host entry refuses such a table before any launch)."""
    import ctypes
    from custom_porechop_abi_amd import engine
    from custom_porechop_abi_amd._lib import check
    seq, qual, side, parts, records = P.pack_corpus()
    planned = parts[:12].copy()
    end, tiles = engine.bam_pack_plan(planned)
    bad = planned.copy()
    bad['seq_src'][2] = seq.size
    bad['qual_src'][4] = qual.size - 1
    bad['side_off'][6] = side.size
    bad['out'][8] = end
    bad['name_len'][10] = 255
    skipped = {2, 4, 6, 8, 10}
    assert all(planned['l_seq'][k] > 0 or k in (6, 8, 10) for k in skipped)
    L = gpu_lib
    VP = ctypes.c_void_p
    bufs = []

    def up(a):
        p = VP()
        check(L.pcabi_dev_malloc(ctypes.byref(p), max(a.nbytes, 1) + 64), 'pcabi_dev_malloc')
        bufs.append(p)
        check(L.pcabi_dev_h2d(p, a.ctypes.data_as(VP), a.nbytes), 'pcabi_dev_h2d')
        return p

    try:
        check(L.pcabi_dev_set(0), 'pcabi_dev_set')
        out = np.full(end, 0xA5, np.uint8)
        d = [up(a) for a in (seq, qual, side, bad, out)]
        check(L.pcabi_bam_pack_dev(None, d[0], seq.size, d[1], qual.size, d[2], side.size, d[3], bad.size, tiles, d[4], end),
              'pcabi_bam_pack_dev')
        check(L.pcabi_dev_sync(), 'pcabi_dev_sync')
        check(L.pcabi_dev_d2h(out.ctypes.data_as(VP), d[4], out.nbytes), 'pcabi_dev_d2h')
    finally:
        for p in bufs:
            L.pcabi_dev_free(p)
    keep = [k for k in range(planned.size) if k not in skipped]
    assert np.array_equal(out, P.expected_image(planned[keep], [records[k] for k in keep], end))


# ---- 2. the writer --------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,variant', [('fastq', 'split'), ('bam', 'split'), ('fasta', 'select'), ('fastq', 'untrimmed'),
                                          ('bam', 'discard_middle')])
def test_writer_on_device_matches_host_path(gpu_lib, tmp_path, kind, variant):
    """The two-batch case written with gzip_device=0 and with gzip_device=None: the same decoded bytes
    (which are header_bytes + record_bytes of the FASTQ writer's parts), well-formed members, and the same
    reads back through the device reader."""
    from custom_porechop_abi_amd import misc
    from tests.test_bam_pack_cpu import check_bam_file
    host_path, header, text, n_h, n_fq = P.write_two_batches(tmp_path, kind, variant, None, 'h')
    dev_path, header_d, text_d, n_d, _ = P.write_two_batches(tmp_path, kind, variant, 0, 'd')
    assert (header_d, text_d, n_d) == (header, text, n_h)
    mem_d, stream_d = check_bam_file(dev_path, header, text, kind == 'fasta', n_d, n_fq, {'gunzip_device': 0})
    with open(host_path, 'rb') as f:
        stream_h = b''.join(d for _, d in P.members(f.read()[:-28]))
    assert stream_d == stream_h
    assert len(mem_d) >= 3 and [len(d) for _, d in mem_d[:2]] == [P.BLOCK, P.BLOCK]
    back = misc.load_batch(dev_path, gunzip_device=0)
    assert P.batch_reads(back) == P.batch_reads(misc.load_batch(host_path))


# ---- 3. FileTrimmer -------------------------------------------------------------------------------------
def _golden_bam(tmp_path, fq_name):
    """The golden reads (adapters at their ends and in their middles) as a BAM whose records carry RG, qs
    and MM tags; every fourth record is stored reverse-complemented."""
    from custom_porechop_abi_amd import misc
    fq = misc.load_batch(os.path.join(DATA, fq_name))
    recs = []
    for i in range(fq.n):
        seq, qual = fq.sequence(i), [ord(c) - 33 for c in fq.quals(i)]
        flag = 4
        if i % 4 == 1 and set(seq) <= set(B.LETTERS):
            seq, qual, flag = ''.join(B.COMPLEMENT[c] for c in reversed(seq)), qual[::-1], 4 | 0x10
        recs.append({'name': fq.name(i).split()[0].encode(), 'seq': seq, 'qual': qual, 'flag': flag,
                     'aux': b'RGZgrp\0' + b'qsC' + bytes([i % 200]) + b'MMZC+m,1,2;\0'})
    header = b'@HD\tVN:1.6\tSO:unknown\n@RG\tID:grp\n'
    return _write(tmp_path, 'in.bam', B.make_bam(recs, header, (), 5000)), recs, header


def _trimmer(case, **kw):
    from custom_porechop_abi_amd.pipeline import FileTrimmer
    from tests.test_pipeline import _matching
    o = case['opts']
    return FileTrimmer(_matching(case), o['scoring'], o['end_size'], o['end_threshold'], o['extra_end_trim'],
                       o['min_trim_size'], o['middle_threshold'], 10, 100, 1000, **kw)


def _finished_stream(path):
    with open(path, 'rb') as f:
        data = f.read()
    assert data[-28:] == B.EOF_MARKER and data[-56:-28] != B.EOF_MARKER
    return b''.join(d for _, d in P.members(data[:-28]))


def test_file_trimmer_bam_to_bam(gpu_lib, tmp_path):
    from custom_porechop_abi_amd import misc
    case = [c for c in golden_lib.g2()['cases'] if c['case'] == 'one_adapter_set'][0]
    src, recs, header = _golden_bam(tmp_path, 'test_one_adapter_set.fastq.gz')
    out_bam, out_fq = str(tmp_path / 'out.bam'), str(tmp_path / 'out.fastq')
    # (the read filter off: every read is written, trimmed, split or whole)
    ft = _trimmer(case, filter_reads=False, gzip_on_device=True, gunzip_on_device=True, keep_tags=True)
    try:
        c_bam = ft.trim_file(src, out_bam, 'bam', max_reads=7)        # several batches
        c_fq = ft.trim_file(src, out_fq, 'fastq', max_reads=7)
    finally:
        ft.close()
    assert c_bam == c_fq
    with open(out_fq, 'rb') as f:
        text = f.read()
    exp = P.records_of_fastq(text)
    assert len(exp) > 7
    stream = _finished_stream(out_bam)
    assert stream.startswith(B.header_bytes(header))
    back = misc.load_batch(out_bam, gunzip_device=0, keep_aux=True)
    assert back.bam_header == header and P.batch_reads(back) == P.reads_of(exp)
    # tags: RG and qs on every record; MM only on reads written whole from forward records
    by_name = {r['name']: r for r in recs}
    whole = changed = 0
    for i in range(back.n):
        name = back.names[back.name_off[i]:back.name_off[i + 1]].tobytes()
        r = by_name.get(name) or by_name[name.rsplit(b'_', 1)[0]]
        same = name in by_name and not r['flag'] & 0x10 and back.seq[back.seq_off[i]:back.seq_off[i + 1]].tobytes() == r['seq'].encode()
        assert back.aux(i) == (r['aux'] if same else r['aux'][:-len(b'MMZC+m,1,2;\0')]), name
        whole += same
        changed += not same
    assert changed > 0
    # and the whole file is the restatement's bytes
    aux = [back.aux(i) for i in range(back.n)]
    assert stream == B.header_bytes(header) + b''.join(B.record_bytes(dict(r, aux=a)) for r, a in zip(exp, aux))


def test_file_trimmer_bam_bins(gpu_lib, tmp_path):
    from custom_porechop_abi_amd import misc
    case = [c for c in golden_lib.g2()['cases'] if c['case'] == 'barcodes'][0]
    o = case['opts']
    in_path = os.path.join(DATA, 'test_barcodes.fastq.gz')
    bins = {}
    for fmt in ('fastq', 'bam'):
        bdir = str(tmp_path / ('bins_' + fmt))
        ft = _trimmer(case, barcode_dir=bdir, forward_or_reverse_barcodes=case['forward_or_reverse'],
                      require_two_barcodes=bool(o.get('require_two')), gzip_on_device=True)
        try:
            counts = ft.trim_file(in_path, str(tmp_path / 'unused'), fmt, max_reads=3)
        finally:
            ft.close()
        bins[fmt] = ({k: v[1] for k, v in counts['bins'].items()},
                     {f[:-len(fmt) - 1]: os.path.join(bdir, f) for f in sorted(os.listdir(bdir))})
    assert bins['bam'][0] == bins['fastq'][0] and sorted(bins['bam'][1]) == sorted(bins['fastq'][1]) and bins['fastq'][1]
    for name, fq_path in bins['fastq'][1].items():
        with open(fq_path, 'rb') as f:
            exp = P.records_of_fastq(f.read())
        stream = _finished_stream(bins['bam'][1][name])          # every bin: header first, marker last, once
        assert stream == B.header_bytes(P.DEFAULT_HEADER) + b''.join(B.record_bytes(r) for r in exp), name
        assert P.batch_reads(misc.load_batch(bins['bam'][1][name], gunzip_device=0)) == P.reads_of(exp)

