"""The gzip decoder's device-free core (csrc/pcabi_inflate.h) built for the host: sound members,
damaged members, the BGZF member index and a sanitizer-built mutation run. The expected bytes
always come from zlib; every hand-built stream is first shown to zlib."""
import gzip
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests import deflate_cpu_lib as D
from tests import inflate_cpu_lib as I

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def sound():
    return I.sound_members()


@pytest.fixture(scope='module')
def damaged():
    return I.damaged_members()


def test_corpus_is_what_zlib_says(sound, damaged):
    """The yardstick first: zlib decodes every sound member to the intended bytes and refuses
    every damaged one."""
    for name, m, data in sound:
        assert I.zlib_raw(I.damaged_payload_of(m)) == data, name
        assert gzip.decompress(m) == data, name
    for name, m, _ in damaged:
        with pytest.raises((zlib.error, EOFError, OSError)):
            gzip.decompress(m)


def test_corpus_covers_the_issue_list(sound):
    names = [n for n, _, _ in sound]
    for size in I.SIZES:
        assert any('-%d-' % size in n for n in names)
    for lvl in (0, 1, 6, 9):
        for strat in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE):
            assert any('-l%d-s%d-' % (lvl, strat) in n for n in names)
    assert sum(n.startswith('stored-after-dyn-phase') for n in names) == 8


def test_sound_members_decode(sound):
    for name, m, data in sound:
        st, got = I.inflate_member(m)
        assert st == 0, (name, st)
        assert got == data, name


def test_members_of_the_projects_encoder_decode():
    """Headers from the encoder's planner (one distance code of length 1, no runs) turned into
    members by the bit writer here."""
    rng = np.random.RandomState(7)
    for data in (I.fastq_text(5000, 9), b'A', b'AB' * 700, bytes(rng.randint(0, 256, 3000).astype(np.uint8)),
                 bytes(np.repeat(np.arange(200, dtype=np.uint8), np.arange(200) ** 2 % 97 + 1))):
        cnt = np.bincount(np.frombuffer(data, np.uint8), minlength=256)
        plan = D.plan_block(cnt)
        lit = [int(x) for x in plan['lit_len']]
        cl = [int(x) for x in plan['cl_len']]
        w = I.BitWriter().put(0, 1).put(2, 2).put(0, 5).put(0, 5).put(plan['hclen4'] - 4, 4)
        for i in range(plan['hclen4']):
            w.put(cl[I.CL_ORDER[i]], 3)
        cc = I.canonical(cl)
        for ln in lit + [1]:
            w.code(*cc[ln])
        assert len(w.bits) == plan['hdr_bits']
        I.emit(w, I.canonical(lit), {}, list(data) + [256])
        assert len(w.bits) == plan['block_bits']
        # the sync marker and the closing empty fixed block, as the encoder writes them
        w.put(0, 3).align().put(0, 16).put(0xffff, 16).put(1, 1).put(1, 2).put(0, 7).align()
        payload = w.tobytes()
        assert I.zlib_raw(payload) == data
        st, got = I.inflate_member(I.member(payload, data))
        assert (st, got) == (0, data)


def test_damaged_members_give_their_status(damaged):
    for name, m, status in damaged:
        st, _ = I.inflate_member(m)
        assert st == status, (name, st, status)


def test_header_fields_are_skipped():
    data = b'ACGT' * 100
    p = I.deflate_raw(data)
    for kw in (dict(extra_before=b'XY\x03\x00abc'), dict(extra_after=b'ZZ\x00\x00'), dict(fname=b'reads.fastq'),
               dict(fname=b'x', fhcrc=True), dict(extra_before=b'AB\x01\x00q', extra_after=b'CD\x02\x00rs', fhcrc=True)):
        m = I.member(p, data, **kw)
        assert gzip.decompress(m) == data
        assert I.inflate_member(m) == (0, data)
    assert I.inflate_member(b'\x1f\x8b\x07' + I.member(p, data)[3:])[0] == I.E_HEADER
    assert I.inflate_member(I.member(p, data)[:17])[0] == I.E_HEADER
    assert I.inflate_member(I.member(p + b'\x00', data))[0] == I.E_HEADER   # a byte between stream and trailer


def test_smaller_capacity_is_refused():
    data = I.fastq_text(1000, 2)
    assert I.inflate_member(I.member(I.deflate_raw(data), data), cap=999)[0] == I.E_OUTPUT


# ---- the member index --------------------------------------------------------------------------------
def _stream(parts, **kw):
    return b''.join(I.member(I.deflate_raw(d), d, **kw) for d in parts)


def test_index_bgzf():
    parts = [I.fastq_text(70000, 1)[:65280], b'x' * 100, b'', b'tail\n']
    s = _stream(parts)
    in_off, out_off = I.index(s)
    assert len(in_off) == 5 and in_off[0] == 0 and in_off[-1] == len(s)
    assert list(np.diff(out_off)) == [len(p) for p in parts]
    for k, p in enumerate(parts):
        assert gzip.decompress(s[in_off[k]:in_off[k + 1]]) == p


def test_index_extra_subfields_fname_fhcrc():
    parts = [b'one\n' * 50, b'two\n' * 70]
    for kw in (dict(extra_before=b'XY\x03\x00abc', extra_after=b'ZZ\x00\x00'), dict(fname=b'a.fq', fhcrc=True)):
        s = _stream(parts, **kw)
        in_off, out_off = I.index(s)
        assert list(out_off) == [0, 200, 480] and in_off[-1] == len(s)
        assert gzip.decompress(s) == b''.join(parts)


def test_index_not_indexable():
    assert I.index(gzip.compress(b'hello')) == 0
    assert I.index(_stream([b'abc']) + gzip.compress(b'hello')) == 0
    big = I.member(I.deflate_raw(b'\0' * 65537), b'\0' * 65537)
    assert I.index(big) == 0
    assert I.index(b'') == 0


def test_index_truncated_or_not_gzip():
    s = _stream([I.fastq_text(3000, 4), b'abc'])
    first = I.index(s)[0][1]
    for cut in (first - 1, first + 5, len(s) - 1, 10):
        assert I.index(s[:cut]) == I.E_PARSE
    assert I.index(b'@read\nACGT\n+\n!!!!\n' * 3) == I.E_PARSE


def test_index_eof_markers_anywhere():
    a, b = _stream([b'abc\n' * 10]), _stream([b'defg\n' * 10])
    s = I.EOF_MARKER + a + I.EOF_MARKER + b + I.EOF_MARKER
    in_off, out_off = I.index(s)
    assert list(np.diff(out_off)) == [0, 40, 0, 50, 0]
    assert list(np.diff(in_off)) == [28, len(a), 28, len(b), 28]
    st, got = I.inflate_member(I.EOF_MARKER)
    assert (st, got) == (0, b'')


# ---- sanitizer-built mutation run ------------------------------------------------------------------
def test_mutations_under_sanitizers(tmp_path, sound, damaged):
    """tests/inflate_fuzz_main.cpp, built with -fsanitize=address,undefined as a program of its own
    and run as a child process over seeded mutations of the corpora."""
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path / 'inflate_fuzz')
    base = ['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
            os.path.join(HERE, 'inflate_fuzz_main.cpp'), '-lz']
    # the runtimes linked into the program itself where the toolchain has them, so that nothing
    # about the process's library order matters
    for extra in (['-static-libasan', '-static-libubsan'], []):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        if r.returncode == 0:
            break
    if r.returncode != 0 and ('asan' in r.stderr or 'ubsan' in r.stderr or 'sanitize' in r.stderr):
        pytest.skip('the sanitizer runtime cannot be linked')
    assert r.returncode == 0, r.stderr
    corpus = str(tmp_path / 'corpus.bin')
    # every sound member (the 64 KiB ones and the 258 / 32768 match included) is decoded as it is;
    # mutations draw from them all
    corpus_members = [m for _, m, _ in sound]
    with open(corpus, 'wb') as f:
        for m in corpus_members:
            f.write(struct.pack('<I', len(m)) + m)
    r = subprocess.run([exe, corpus, '1', str(len(corpus_members) + 4000)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    # the damaged members as seeds of their own: nothing here has to decode
    with open(corpus, 'wb') as f:
        for _, m, _ in damaged:
            f.write(struct.pack('<I', len(m)) + m)
    r = subprocess.run([exe, corpus, '2', '3000', 'mutate-only'], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
