"""The writers' error paths and bookkeeping, without a GPU (the host paths of misc.write_reads: the plain text
writer, its zlib path, the host BAM writer and the host text writer with tags in the headers): a path that
cannot be opened says `could not write`, a file that refuses the bytes says `write failed`, no call leaves a
descriptor open, and the three times of pcabi_reads_write_last_times are sub-intervals of the call."""
import ctypes
import math
import os
import time

import numpy as np
import pytest

from tests import bam_lib as B
from tests import test_mods_cpu as C
from tests import test_moves_cpu as V

TAGS = {'keep_aux': True, 'keep_mods': True, 'keep_moves': True}
# (what, out_format, options): every host writer, the tagged ones with the remap stage
WRITERS = [('plain', 'fastq', {}), ('zlib', 'fastq.gz', {}), ('bam', 'bam', dict(TAGS, gzip_device=None)),
           ('tagged', 'fastq', dict(TAGS, header_tags=True)), ('tagged zlib', 'fastq.gz', dict(TAGS, header_tags=True))]
_case = None


def case(tmp_path_factory):
    """A dozen reads of 60..200 bases with MM / ML / MN and mv / ts, from a BAM loaded with keep_aux; trims on
    most, and a middle cut in read 5, so that numbered names occur. Made once."""
    global _case
    if _case is None:
        from custom_porechop_abi_amd import misc
        rng = np.random.RandomState(12)
        recs = []
        for i in range(12):
            n = [60, 200, 97, 128, 64, 180, 71, 150, 199, 65, 113, 160][i]
            seq = ''.join(rng.choice(list('ACGT'), n))
            aux = (C.make_tags(rng, seq, [C.HEADERS[0], C.HEADERS[3]], 0.3, with_mn='i') + b'RGZgrp\0' +
                   V.mv_aux(5, V.make_moves(rng, n, 2.0)) + V.ts_aux(10 + i))
            recs.append({'name': b'read%d' % i, 'seq': seq, 'qual': [(3 * i + k) % 50 for k in range(n)], 'flag': 4, 'aux': aux})
        src = str(tmp_path_factory.mktemp('writer_errors') / 'in.bam')
        with open(src, 'wb') as f:
            f.write(B.make_bam(recs, b'@HD\tVN:1.6\tSO:unknown\n', (), 5000))
        batch = misc.load_batch(src, keep_aux=True)
        assert batch.n == 12
        cuts = [[] for _ in range(12)]
        cuts[5] = [(70, 90)]
        _case = batch, {'start_trim': [i % 4 * 3 for i in range(12)], 'end_trim': [i % 3 * 5 for i in range(12)],
                        'middle_cuts': cuts, 'min_split_read_size': 1}
    return _case


def open_fds():
    return len(os.listdir('/proc/self/fd'))


def last_times():
    from custom_porechop_abi_amd import _lib
    t = (ctypes.c_double * 3)(-1, -1, -1)
    _lib.lib().pcabi_reads_write_last_times(ctypes.byref(t, 0), ctypes.byref(t, 8), ctypes.byref(t, 16))
    return list(t)


def refused(batch, path, fmt, kw, words):
    """The call raises check()'s error with `words` in its message and leaves no descriptor open."""
    from custom_porechop_abi_amd import misc
    from custom_porechop_abi_amd._lib import PcabiError
    before = open_fds()
    with pytest.raises(PcabiError) as e:
        misc.write_reads(batch, path, fmt, **kw)
    assert words in str(e.value), str(e.value)
    assert open_fds() == before


@pytest.mark.parametrize('what,fmt,opts', WRITERS, ids=[w[0] for w in WRITERS])
def test_missing_directory(tmp_path, tmp_path_factory, what, fmt, opts):
    batch, base = case(tmp_path_factory)
    path = str(tmp_path / 'no_such_directory' / ('out.' + fmt))
    refused(batch, path, fmt, dict(base, **opts), 'could not write')
    assert not os.path.exists(os.path.dirname(path))


# the zlib path of pcabi_reads_write does not look at gzclose's result: not pinned here
@pytest.mark.parametrize('what,fmt,opts', [w for w in WRITERS if w[0] != 'zlib'], ids=[w[0] for w in WRITERS if w[0] != 'zlib'])
def test_failed_write(tmp_path_factory, what, fmt, opts):
    if not os.path.exists('/dev/full'):
        pytest.skip('no /dev/full')
    batch, base = case(tmp_path_factory)
    refused(batch, '/dev/full', fmt, dict(base, **opts), 'write failed')


@pytest.mark.parametrize('what,fmt,opts', WRITERS, ids=[w[0] for w in WRITERS])
def test_success_leaves_no_descriptor_and_sound_times(tmp_path, tmp_path_factory, what, fmt, opts):
    from custom_porechop_abi_amd import misc
    batch, base = case(tmp_path_factory)
    path = str(tmp_path / ('out.' + fmt))
    before = open_fds()
    t0 = time.perf_counter()
    n = misc.write_reads(batch, path, fmt, **dict(base, **opts))
    wall = time.perf_counter() - t0
    times = last_times()
    assert open_fds() == before
    assert n == 12 and os.path.getsize(path) > 0
    print(what, times, wall)
    assert all(math.isfinite(t) and t >= 0 for t in times), times
    assert sum(times) <= wall, (times, wall)      # each is a sub-interval of the call, and they do not overlap
