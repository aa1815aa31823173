"""The kept buffers of the file path's device stages (csrc/pcabi_hostdev.h Owned; the encoder's and the
decoder's stage, a GunzipReader's slots, BamDev, PackDev) inside one process: a small call, a larger
one that makes the buffers grow, the small one again, and readers opened and closed one after the
other. Every result is checked against zlib or the host path."""
import gzip

import numpy as np
import pytest

from tests import bam_pack_lib as P
from tests import inflate_cpu_lib as I

pytestmark = pytest.mark.gpu


def _whole_records(text):
    return text[:text.rindex(b'\n@') + 1]


def test_encoder_stage_regrows_and_is_reused(gpu_lib):
    """pcabi_gzip_host on 40 KB, on 300 KB in 1000-byte blocks (passes of 64 KiB, so five of them, each
    of more blocks than the stage's floor of 16: a larger reserve), on the 40 KB again, then
    pcabi_bgzf_host on the 300 KB."""
    from custom_porechop_abi_amd import engine
    small, large = I.fastq_text(40000, 31), I.fastq_text(300000, 32)
    blocks = np.arange(0, len(large) + 1, 1000, dtype=np.int64)
    assert blocks[-1] == len(large)
    assert gpu_lib.pcabi_gzip_tune(0, 0, 65536) == 0
    try:
        z1 = engine.gzip_compress(small)
        z2 = engine.gzip_compress(large, blocks)
        z3 = engine.gzip_compress(small)
        z4 = engine.bgzf_compress(large, blocks)
    finally:
        assert gpu_lib.pcabi_gzip_tune(0, 0, 0) == 0
    assert gzip.decompress(z1) == small and gzip.decompress(z2) == large and gzip.decompress(z4) == large
    assert z3 == z1
    assert b''.join(d for _, d in P.members(z4[:-28])) == large and z4[-28:] == I.EOF_MARKER


def test_decoder_stage_and_reader_lifetimes(gpu_lib, tmp_path):
    """pcabi_gunzip_host on 21 members of 2,000 bytes (one group), on 300 (groups of 64 KiB: 32 members
    each, so both slots, ten passes, and a larger reserve than the first call's), on the 21 again; then
    two device readers on the small file, one after the other, each read to its end."""
    from custom_porechop_abi_amd import engine, misc
    small, large = _whole_records(I.fastq_text(39900, 33)), I.fastq_text(598000, 34)
    zs, zl = I.bgzf_zlib(small, 2000, 1), I.bgzf_zlib(large, 2000, 1)
    assert len(engine.bgzf_index(zs)[0]) - 1 == 21 and len(engine.bgzf_index(zl)[0]) - 1 == 300   # the end marker counts
    path = str(tmp_path / 'small.fastq.gz')
    with open(path, 'wb') as f:
        f.write(zs)
    assert gpu_lib.pcabi_gunzip_tune(65536) == 0
    try:
        assert engine.gunzip(zs) == gzip.decompress(zs) == small
        assert engine.gunzip(zl) == gzip.decompress(zl) == large
        assert engine.gunzip(zs) == small
        host = [P.batch_reads(b) for b in misc.read_batches(path, max_reads=25)]
        assert len(host) >= 3
        for _ in range(2):
            assert [P.batch_reads(b) for b in misc.read_batches(path, max_reads=25, gunzip_device=0)] == host
    finally:
        assert gpu_lib.pcabi_gunzip_tune(0) == 0


def _fastq(n, lo, hi, seed):
    rng = np.random.RandomState(seed)
    reads = []
    for k in range(n):
        ln = int(rng.randint(lo, hi + 1))
        reads.append((b'r%d_%d' % (seed, k), bytes(rng.choice(list(b'ACGT'), ln).astype(np.uint8)),
                      bytes((rng.randint(0, 41, ln) + 33).astype(np.uint8))))
    return reads


def test_bam_writer_and_reader_buffers(gpu_lib, tmp_path):
    """pcabi_reads_write_bam on the device with 50 reads, with 3,000 reads of 200..2,000 bases (3.3 Mb:
    the sequence, quality, stream and compressed buffers outgrow their first 1 MiB), with the 50 again;
    each file against the host path's. Then the large file back through the device BAM reader in
    batches of 500 reads, inflated in groups of 256 KiB, so the window moves between its two buffers
    with a carried record and grows."""
    from custom_porechop_abi_amd import misc
    sets = {'small': _fastq(50, 200, 2000, 41), 'large': _fastq(3000, 200, 2000, 42)}
    batch = {}
    for name, reads in sets.items():
        src = str(tmp_path / (name + '.fastq'))
        with open(src, 'wb') as f:
            f.write(P.writer_file('fastq', reads))
        batch[name] = misc.load_batch(src)
        assert batch[name].n == len(reads)
    files = {}
    for k, name in enumerate(('small', 'large', 'small')):
        for dev in (0, None):
            out = str(tmp_path / ('%d_%s.bam' % (k, 'd' if dev == 0 else 'h')))
            assert misc.write_reads(batch[name], out, 'bam', gzip_device=dev) == batch[name].n
            misc.bgzf_finish(out)
            with open(out, 'rb') as f:
                files[k, dev] = f.read()
        assert gzip.decompress(files[k, 0]) == gzip.decompress(files[k, None])
    assert files[0, 0] == files[2, 0]
    assert len(gzip.decompress(files[1, 0])) > 4 << 20
    assert gpu_lib.pcabi_gunzip_tune(1 << 18) == 0
    try:
        got = [P.batch_reads(b) for b in misc.read_batches(str(tmp_path / '1_d.bam'), max_reads=500, gunzip_device=0)]
    finally:
        assert gpu_lib.pcabi_gunzip_tune(0) == 0
    assert len(got) >= 6 and max(len(g[0]) for g in got) == 500
    exp = sets['large']
    assert [x for g in got for x in g[0]] == [r[0] for r in exp]
    assert [x for g in got for x in g[1]] == [r[1] for r in exp]
    assert [x for g in got for x in g[2]] == [r[2] for r in exp]
