"""The parallel gzip stream decoder's device-free core (csrc/pcabi_gzstream.h, the block loop and the
marker / counting sinks of csrc/pcabi_inflate.h) built for the host: the finder's header check, the
stop rule, the chain walk, the window hand-down, the resolve step and the zlib fallback, on the
corpora the GPU tests use, with small chunks. The expected bytes always come from zlib / gzip."""
import gzip
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests import gzstream_cpu_lib as G

HERE = os.path.dirname(os.path.abspath(__file__))
HUGE = 1 << 40


def _ok(res, data, name=''):
    assert len(res) == 2, (name, res[0])
    got, st = res
    assert got == data, name
    return st


# ---- the pieces ----------------------------------------------------------------------------------------
def _block_starts(raw):
    """Bit offsets of the block boundaries of a raw deflate stream, from the counting sink one block at a
    time, each checked against zlib: the bytes up to it decode to the same length."""
    pos, out, total = 0, [], 0
    while True:
        st, _, produced, end, fin = G.blocks(raw, pos, pos + 1, 0 if pos == 0 else 32768, 1 << 30, marker=False)
        assert st == 0
        out.append((pos, total))
        total += produced
        if fin:
            assert total == len(zlib.decompress(raw, -15))
            return out, end
        pos = end


def test_finder_header_check_and_first_candidate():
    t = G.text()[:60000]
    raw = G.gz(t, 6, 1, wbits=-15)
    starts, end = _block_starts(raw)
    assert len(starts) > 20
    assert (end + 7) // 8 == len(raw)
    L = G.load()
    z = np.frombuffer(raw, np.uint8)
    true = set(p for p, _ in starts)
    # every non-final dynamic block start passes the cheap check (zlib writes dynamic blocks here)
    passing = [p for p, _ in starts[:-1] if L.gzs_quick_dynamic(z.ctypes.data, len(raw), p)]
    assert len(passing) >= len(starts) - 2
    # the first candidate at or after any bit is a true block start: this text has no false one
    for lo in (1, 8 * 1000 + 3, 8 * 4096, 8 * 9000 + 5):
        kind, pos = G.find(raw, lo, 8 * len(raw))
        assert kind == G.CAND_DYN and pos in true and pos >= lo
        assert pos == min(p for p in passing if p >= lo)
    # stored and fixed blocks are never candidates
    for strat_level in ((zlib.Z_FIXED, 6), (zlib.Z_DEFAULT_STRATEGY, 0)):
        r = G.gz(t[:20000], strat_level[1], 1, strat_level[0], wbits=-15)
        assert G.find(r, 0, 8 * len(r))[0] == 0
    # a member start: the candidate is its first deflate bit
    m = G.hand_member(t[:500], fname=b'a.fq')
    s = b'\0' * 7 + m
    assert G.find(s, 8, 8 * len(s)) == (G.CAND_MEMBER, 8 * (7 + 10 + 5))
    assert G.find(b'\0' * 7 + G.hand_member(t[:500], flg_or=0x40), 8, 8 * len(s))[0] != G.CAND_MEMBER


def test_marker_sink_and_window_hand_down():
    """A decoder started at a later block with an unknown window: its symbols, resolved through the true
    window, are zlib's bytes, and the handed-down window is the last 32768 bytes."""
    t = G.text()[:120000]
    raw = G.gz(t, 9, 1, wbits=-15)
    starts, _ = _block_starts(raw)
    for idx in (5, len(starts) // 2, len(starts) - 2):
        pos, before = starts[idx]
        st, sym, produced, end, fin = G.blocks(raw, pos, HUGE, 32768, len(t))
        assert st == 0 and fin == 1 and before + produced == len(t)
        assert (sym >= 0x8000).any(), 'no marker: the test text has no match across the block start'
        win = (b'\0' * 32768 + t[:before])[-32768:]
        got, nxt = G.resolve(sym, win)
        assert got == t[before:]
        assert nxt == t[-32768:]
        # a short chunk keeps the older part of its own window
        st, sym, produced, end, fin = G.blocks(raw, pos, pos + 1, 32768, len(t))
        assert st == 0 and produced < 32768
        got, nxt = G.resolve(sym, win)
        assert got == t[before:before + produced] and nxt == (b'\0' * 32768 + t[:before + produced])[-32768:]
    # with no history a match before position 0 is refused, as inflate_raw refuses it
    assert G.blocks(raw, starts[5][0], HUGE, 0, len(t))[0] == 3
    # overlapping copies (dist < len) across the start
    data = b'A' * 5000 + b'AB' * 3000
    raw = G.gz(data, 6, 1, wbits=-15)
    starts, _ = _block_starts(raw)
    pos, before = starts[len(starts) // 2]
    st, sym, produced, _, _ = G.blocks(raw, pos, HUGE, 32768, len(data))
    assert st == 0 and G.resolve(sym, (b'\0' * 32768 + data[:before])[-32768:])[0] == data[before:]


def test_counting_sink_agrees_and_limits():
    t = G.text()[:50000]
    raw = G.gz(t, 6, 1, wbits=-15)
    a = G.blocks(raw, 0, HUGE, 0, len(t), marker=False)
    b = G.blocks(raw, 0, HUGE, 0, len(t), marker=True)
    assert a[0] == b[0] == 0 and a[2:] == b[2:] and a[2] == len(t)
    assert G.blocks(raw, 0, HUGE, 0, len(t) - 1, marker=False)[0] == 5
    assert G.blocks(raw, 0, HUGE, 0, len(t) - 1, marker=True)[0] == 5


# ---- whole streams -------------------------------------------------------------------------------------
@pytest.mark.parametrize('level,mem', G.TEXT_SETTINGS)
def test_text(level, mem):
    t = G.text()
    assert 600000 < len(t) < 700000
    st = _ok(G.stream(G.gz(t, level, mem), G.chunk_for(mem)), t)
    assert st['host_bytes'] == 0 and st['confirmed'] >= 4 and st['dev_bytes'] == len(t) and st['members'] == 1, st


def test_golden_files():
    assert len(G.GOLDEN_GZ) == 4
    for path in G.GOLDEN_GZ:
        with open(path, 'rb') as f:
            s = f.read()
        assert s[3] & 8, 'ordinary gzip with FNAME'
        st = _ok(G.stream(s, 4096), gzip.open(path).read(), path)
        # these files hold one block, or one and a final one: a single chunk on the chain
        assert st['host_bytes'] == 0 and st['confirmed'] >= 1 and st['members'] == 1, (path, st)


def test_history_across_chunks():
    for name, s, data, chunk in G.history_streams():
        st = _ok(G.stream(s, chunk), data, name)
        assert st['host_bytes'] == 0, (name, st)


def test_block_types_device_and_fallback():
    for name, s, data, chunk in G.block_type_streams():
        assert G.zlib_all(s) == data, name
        st = _ok(G.stream(s, chunk), data, name)
        assert st['dev_bytes'] + st['host_bytes'] == len(data), (name, st)
        st = _ok(G.stream(s, chunk, min_chunks=1 << 30), data, name)
        assert st['host_bytes'] == len(data) and st['dev_bytes'] == 0, (name, st)


def test_members():
    for name, s, data, members in G.member_streams():
        assert gzip.decompress(s) == data, name
        for chunk in (4096, 512):
            st = _ok(G.stream(s, chunk), data, name)
            assert st['members'] == members, (name, st)
    # trailing bytes that are no member start are ignored, as gzread does
    s = G.gz(b'hello', 6, 1)
    assert _ok(G.stream(s + b'\0' * 100, 4096), b'hello')['members'] == 1
    assert _ok(G.stream(b'', 4096), b'')['members'] == 0
    assert len(G.stream(b'@read\nACGT\n', 4096)) == 3


def test_false_candidate():
    s, data, places = G.false_candidate_stream(4096)
    assert G.zlib_all(s) == data
    assert len(places) == 4 and all(0 < p % 4096 <= 64 for p in places)
    # the finder takes a copy for a block start
    k = places[0] // 4096
    kind, pos = G.find(s, 8 * 4096 * k, 8 * 4096 * (k + 1))
    assert (kind, pos) == (G.CAND_DYN, 8 * places[0])
    st = _ok(G.stream(s, 4096), data)
    assert st['rejected'] >= 1, st


def test_spans():
    t = G.text()
    s = G.gz(t, 6, 1)
    st = _ok(G.stream(s, 4096, span_bytes=65536), t)
    assert st['spans'] >= len(s) // 65536 and st['host_bytes'] == 0, st
    # spans that take turns: a min_chunks no short last span reaches
    st = _ok(G.stream(s, 4096, span_bytes=65536, min_chunks=16), t)
    assert st['host_bytes'] > 0 and st['dev_bytes'] > 0, st


def test_errors():
    for name, s in G.error_streams():
        with pytest.raises(zlib.error):
            G.zlib_all(s)
        for min_chunks in (0, 1 << 30):
            res = G.stream(s, 4096, min_chunks=min_chunks)
            assert len(res) == 3, name
            assert 'gzip member %d at offset ' % (1 if name == 'reserved-flag' else 0) in res[0], (name, res[0])
    # what was decoded before the damage is zlib's too
    bad = dict(G.error_streams())['flip-last']
    res = G.stream(bad, 4096, span_bytes=65536)
    theirs = G.zlib_prefix(bad)
    m = min(len(res[2]), len(theirs))
    assert m > 300000 and res[2][:m] == theirs[:m]


def test_small_capacity_reports_the_length():
    t = G.text()[:100000]
    got, st = G.stream(G.gz(t, 6, 1), 4096, cap=1000)
    assert got == len(t)


# ---- sanitizer-built mutation run ------------------------------------------------------------------
def test_mutations_under_sanitizers(tmp_path):
    """tests/gzstream_fuzz_main.cpp, built with -fsanitize=address,undefined as a program of its own
    and run as a child process over seeded mutations of the corpora."""
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path / 'gzstream_fuzz')
    base = ['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
            os.path.join(HERE, 'gzstream_fuzz_main.cpp'), '-lz']
    for extra in (['-static-libasan', '-static-libubsan'], []):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        if r.returncode == 0:
            break
    if r.returncode != 0 and ('asan' in r.stderr or 'ubsan' in r.stderr or 'sanitize' in r.stderr):
        pytest.skip('the sanitizer runtime cannot be linked')
    assert r.returncode == 0, r.stderr
    t = G.text()
    seeds = [G.gz(t[:150000], 6, 1), G.gz(t[:60000], 1, 1), G.gz(t[:40000], 0, 1), G.gz(t[:60000], 6, 1, zlib.Z_FIXED),
             G.mixed_flush_stream()[0][:], G.member_streams()[1][1], G.gz(b'AB' * 30000, 6, 1),
             G.gz(t[:700], 6, 1) + G.gz(b'', 6, 1) + G.gz(t[700:30000], 9, 1)]
    corpus = str(tmp_path / 'corpus.bin')
    with open(corpus, 'wb') as f:
        for s in seeds:
            f.write(struct.pack('<I', len(s)) + s)
    r = subprocess.run([exe, corpus, '1', '1500'], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
