"""Sequence-file I/O on both sides of the alignment engine (mirror of porechop_abi/misc.py:60-168
and the read loading / output of porechop_abi/porechop_abi.py:133-187, 535-668).

The parsing and writing run in libpcabi's native host units (csrc/pcabi_io.cpp, csrc/pcabi_write.cpp: zlib, the
reference's parse rules, NanoporeRead's normalisation); this module is the Python surface:
  * load_fasta_or_fastq(filename) -> (records, 'FASTA' | 'FASTQ'), the reference's tuples
    (FASTA: (short_name, seq, full_name); FASTQ: (short_name, seq, spacer, quals, full_name));
    the sequence text is the file's own (the reference normalises it later, in NanoporeRead);
  * load_reads(path, verbosity, print_dest, check_read_count) -> (reads, check_reads, read_type)
    with NanoporeRead objects, for a file or an Albacore-style directory of FASTQs;
  * ReadBatch / read_batches(path): the batched path -- names, normalised sequences, qualities
    and the Dna5 codes already in the engine's packed layout (engine.SeqPack's), no per-read
    Python objects;
  * write_reads(batch, path, ...): the reference's trimmed FASTA / FASTQ output for a batch.
"""
import ctypes
import os
import sys

import numpy as np

from ._lib import check, lib

FASTA, FASTQ = 0, 1


class _View(ctypes.Structure):
    _fields_ = [('n', ctypes.c_int64), ('type', ctypes.c_int32), ('names', ctypes.c_void_p),
                ('name_off', ctypes.c_void_p), ('seq', ctypes.c_void_p), ('seq_off', ctypes.c_void_p),
                ('qual', ctypes.c_void_p), ('qual_off', ctypes.c_void_p), ('rna', ctypes.c_void_p),
                ('spacer', ctypes.c_void_p), ('spacer_off', ctypes.c_void_p), ('codes', ctypes.c_void_p), ('codes_len', ctypes.c_int64), ('code_off', ctypes.c_void_p),
                ('len', ctypes.c_void_p)]


def _declare(L):
    if getattr(L, '_io_declared', False):
        return L
    P, i64, c_int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    sig = {
        'pcabi_fastx_open': ([ctypes.c_char_p, c_int, ctypes.POINTER(P)], c_int),
        'pcabi_fastx_open_dev': ([ctypes.c_char_p, c_int, c_int, ctypes.POINTER(P)], c_int),
        'pcabi_fastx_open_dev2': ([ctypes.c_char_p, c_int, c_int, c_int, ctypes.POINTER(P)], c_int),
        'pcabi_fastx_type': ([P], c_int),
        'pcabi_fastx_next': ([P, i64, i64, ctypes.POINTER(P)], i64),
        'pcabi_fastx_close': ([P], None),
        'pcabi_fastx_load': ([ctypes.c_char_p, c_int, ctypes.POINTER(P)], c_int),
        'pcabi_reads_count': ([P], i64),
        'pcabi_reads_type': ([P], c_int),
        'pcabi_reads_views': ([P, ctypes.POINTER(_View)], c_int),
        'pcabi_reads_free': ([P], None),
        'pcabi_reads_write': ([P, ctypes.c_char_p, c_int, c_int, c_int, P, P, P, P, c_int, c_int, c_int, P], c_int),
        'pcabi_reads_write_dev': ([P, ctypes.c_char_p, c_int, c_int, c_int, P, P, P, P, c_int, c_int, c_int, P, c_int],
                                  c_int),
        'pcabi_bgzf_write_eof': ([ctypes.c_char_p], c_int),
        'pcabi_reads_write_bam': ([P, ctypes.c_char_p, c_int, P, P, P, P, c_int, c_int, c_int, P, ctypes.c_char_p, i64,
                                   c_int, c_int], c_int),
        'pcabi_reads_write_bam_tags': ([P, ctypes.c_char_p, c_int, P, P, P, P, c_int, c_int, c_int, P, ctypes.c_char_p,
                                        i64, c_int, c_int, c_int], c_int),
        'pcabi_fastx_keep_aux': ([P, c_int], c_int),
        'pcabi_fastx_header_tags': ([P, c_int, c_int], c_int),
        'pcabi_reads_aux': ([P, ctypes.POINTER(P), ctypes.POINTER(P), ctypes.POINTER(P)], c_int),
        'pcabi_fastx_bam_header': ([P, ctypes.POINTER(P), ctypes.POINTER(i64)], c_int),
        'pcabi_fastx_record_start': ([P, i64], i64),
        'pcabi_fastx_set_range': ([P, i64, i64], c_int),
        'pcabi_fastx_remaining': ([P], i64),
        'pcabi_fastx_next_text': ([P, i64, ctypes.POINTER(P), ctypes.POINTER(i64)], c_int),
    }
    for name, (a, r) in sig.items():
        f = getattr(L, name)
        f.argtypes, f.restype = a, r
    L._io_declared = True
    return L


class _Owner(object):
    """Owns a native batch; numpy views into its buffers keep it alive (zero-copy)."""

    def __init__(self, handle):
        self.h = handle

    def __del__(self):
        h, self.h = self.h, None
        if h:
            try:
                _declare(lib()).pcabi_reads_free(h)
            except Exception:
                pass


def _view(owner, ptr, dtype, n):
    """numpy view of n items at ptr inside owner's batch (no copy)."""
    dtype = np.dtype(dtype)
    if n == 0 or not ptr:
        return np.zeros(0, dtype)
    raw = (ctypes.c_uint8 * (n * dtype.itemsize)).from_address(ptr)
    raw._owner = owner                         # the ctypes buffer keeps the batch alive
    return np.frombuffer(raw, dtype=dtype, count=n)


class ReadBatch(object):
    """One batch of parsed reads, as zero-copy numpy views of the native buffers.

    names / seq / qual: uint8 buffers with int64 offsets [n + 1]; rna: uint8 [n];
    codes: Dna5 uint8 buffer, code_off int64 [n] (4-aligned), lengths int32 [n] -- the layout
    engine.SeqPack builds, so (codes, code_off + start, length) are engine windows directly.
    The native batch lives as long as this object or any of its arrays (write_reads uses it).
    bam_header: the header text (bytes) of the BAM file the batch came from, else None. With
    keep_aux (read_batches / load_batch) a BAM batch also holds its records' aux tags: aux_bytes /
    aux_off int64 [n + 1] and as_stored uint8 [n] (0: a reverse-strand record, whose bases the reader
    reverse-complemented); all None otherwise. A FASTA / FASTQ batch read with tags_from_headers holds the
    tags parsed from its headers in the same three arrays (as_stored is 1 for every read)."""

    def __init__(self, handle, bam_header=None):
        L = _declare(lib())
        v = _View()
        self._owner = _Owner(handle)
        check(L.pcabi_reads_views(handle, ctypes.byref(v)), 'pcabi_reads_views')
        n = int(v.n)
        o = self._owner
        self.type = int(v.type)
        self.n = n
        self.name_off = _view(o, v.name_off, np.int64, n + 1)
        self.seq_off = _view(o, v.seq_off, np.int64, n + 1)
        self.qual_off = _view(o, v.qual_off, np.int64, n + 1)
        self.spacer_off = _view(o, v.spacer_off, np.int64, n + 1)
        self.names = _view(o, v.names, np.uint8, int(self.name_off[-1]) if n else 0)
        self.seq = _view(o, v.seq, np.uint8, int(self.seq_off[-1]) if n else 0)
        self.qual = _view(o, v.qual, np.uint8, int(self.qual_off[-1]) if n else 0)
        self.spacer = _view(o, v.spacer, np.uint8, int(self.spacer_off[-1]) if n else 0)
        self.rna = _view(o, v.rna, np.uint8, n)
        self.codes = _view(o, v.codes, np.uint8, int(v.codes_len))
        self.code_off = _view(o, v.code_off, np.int64, n)
        self.lengths = _view(o, v.len, np.int32, n)
        self.bam_header = bam_header
        ax, ao, st = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        check(L.pcabi_reads_aux(handle, ctypes.byref(ax), ctypes.byref(ao), ctypes.byref(st)), 'pcabi_reads_aux')
        self.aux_bytes = self.aux_off = self.as_stored = None
        if ao.value:
            self.aux_off = _view(o, ao.value, np.int64, n + 1)
            self.aux_bytes = _view(o, ax.value, np.uint8, int(self.aux_off[-1]))
            self.as_stored = _view(o, st.value, np.uint8, n)

    @property
    def _h(self):
        return self._owner.h

    def __len__(self):
        return self.n

    def _text(self, buf, off, i):
        return buf[off[i]:off[i + 1]].tobytes().decode()

    def name(self, i):
        return self._text(self.names, self.name_off, i)

    def sequence(self, i):
        return self._text(self.seq, self.seq_off, i)

    def quals(self, i):
        return self._text(self.qual, self.qual_off, i)

    def aux(self, i):
        """Record i's aux tags as the file holds them (bytes); None when the batch keeps none."""
        if self.aux_off is None:
            return None
        return self.aux_bytes[self.aux_off[i]:self.aux_off[i + 1]].tobytes()

    def spacer_line(self, i):
        return self._text(self.spacer, self.spacer_off, i)

    def views(self, starts=None, lengths=None):
        """Engine windows (codes, offsets, lengths) of [start, start + length) of every read."""
        st = np.zeros(self.n, np.int64) if starts is None else np.asarray(starts, np.int64)
        ln = self.lengths if lengths is None else np.asarray(lengths, np.int32)
        return self.codes, self.code_off + st, ln

    def nanopore_reads(self):
        """The reference's NanoporeRead objects (name = full header; seq / quals already
        normalised, so the constructor leaves them unchanged except for the rna flag)."""
        from .nanopore_read import NanoporeRead
        out = []
        for i in range(self.n):
            r = NanoporeRead(self.name(i), self.sequence(i), self.quals(i))
            r.rna = bool(self.rna[i])
            out.append(r)
        return out


def _open_error(path):
    msg = lib().pcabi_last_error()
    return msg.decode() if msg else path


def input_files(path):
    """The sequence files of an input, as load_reads sees it (porechop_abi.py:133-187): a file (FASTA,
    FASTQ or BAM, plain or gzip) is itself (albacore barcode None); a directory is an Albacore output
    directory -- every *.fastq / *.fastq.gz under it, sorted by path, each with the barcode its path names
    (get_albacore_barcode_from_path). Exits like the reference when nothing is found."""
    if os.path.isfile(path):
        return [(path, None)]
    if os.path.isdir(path):
        fastqs = sorted([os.path.join(d, f) for d, _, fs in os.walk(path) for f in fs
                         if f.lower().endswith('.fastq') or f.lower().endswith('.fastq.gz')])
        if not fastqs:
            sys.exit('Error: could not find fastq files in ' + path)
        return [(f, get_albacore_barcode_from_path(f)) for f in fastqs]
    sys.exit('Error: could not find ' + path)


def load_check_reads(path, check_read_count):
    """The check reads of load_reads (porechop_abi.py:133-187) as NanoporeRead objects: a file's
    first check_read_count records; for an Albacore directory the first
    round(check_read_count / files) records of every file, in file order."""
    files = input_files(path)
    per_file = check_read_count if os.path.isfile(path) else int(round(check_read_count / len(files)))
    out = []
    for f, _ in files:
        if per_file <= 0:
            break
        for b in read_batches(f, max_reads=per_file, max_bases=1 << 62):
            out += b.nanopore_reads()
            break
    return out


def record_boundaries(path, parts):
    """Byte offsets [parts + 1] splitting a plain FASTA / FASTQ file into `parts` contiguous record
    ranges of about equal size (so about equal bases): each cut is moved forward to the next record
    start (pcabi_fastx_record_start). None for a gzip file (it cannot be entered mid-stream) and for
    a directory (its files are streamed in order)."""
    if os.path.isdir(path):
        return None
    L = _declare(lib())
    h = ctypes.c_void_p()
    rc = L.pcabi_fastx_open(os.fsencode(path), 0, ctypes.byref(h))
    if rc != 0:
        raise ValueError(_open_error(path))
    try:
        if get_compression_type(path) != 'plain':
            return None
        size = os.path.getsize(path)
        cuts = [0]
        for k in range(1, parts):
            b = L.pcabi_fastx_record_start(h, size * k // parts)
            if b < 0:
                return None
            cuts.append(max(int(b), cuts[-1]))
        cuts.append(size)
        return cuts
    finally:
        L.pcabi_fastx_close(h)


def _starts_bgzf(path):
    """Whether the file's first gzip member carries the BGZF 'BC' subfield. Anything else (a plain
    file, ordinary gzip) keeps the loader it always had, whatever gunzip_device says."""
    try:
        with open(path, 'rb') as f:
            h = f.read(12)
            if len(h) < 12 or h[:3] != b'\x1f\x8b\x08' or not h[3] & 4:
                return False
            extra = f.read(h[10] | h[11] << 8)
    except OSError:
        return False
    q = 0
    while q + 4 <= len(extra):
        slen = extra[q + 2] | extra[q + 3] << 8
        if extra[q:q + 2] == b'BC' and slen == 2:
            return True
        q += 4 + slen
    return False


def is_bam(path):
    """Whether the file is a BAM file: gzip (BGZF) whose decoded bytes start with 'BAM'."""
    import zlib
    try:
        with open(path, 'rb') as f:
            head = f.read(1 << 16)
        if head[:3] != b'\x1f\x8b\x08':
            return False
        return zlib.decompressobj(31).decompress(head, 4)[:3] == b'BAM'
    except (OSError, zlib.error):
        return False


OPEN_GUNZIP_PLAIN = 1   # include/pcabi.h PCABI_OPEN_GUNZIP_PLAIN


def _check_gunzip_plain(gunzip_device, gunzip_plain):
    if gunzip_plain and gunzip_device is None:
        raise ValueError('gunzip_plain needs gunzip_device')


def _check_tags_from_headers(tags_from_headers, keep_aux, raw):
    if tags_from_headers and not keep_aux:
        raise ValueError('tags_from_headers needs keep_aux')
    if tags_from_headers and raw:
        raise ValueError('tags_from_headers does not go with raw: a raw batch keeps the file\'s text')


def _fastx_open(L, path, raw, gunzip_device, keep_aux=False, gunzip_plain=False, tags_from_headers=False, tags_device=None):
    """pcabi_fastx_open, or pcabi_fastx_open_dev when gunzip_device names a GPU (a block-gzipped file
    is then inflated there; any other file reads as before, unless gunzip_plain sends ordinary gzip
    there too: pcabi_fastx_open_dev2). keep_aux: pcabi_fastx_keep_aux. tags_from_headers:
    pcabi_fastx_header_tags on tags_device (None: the host build). Returns (rc, handle)."""
    h = ctypes.c_void_p()
    if gunzip_device is None:
        rc = L.pcabi_fastx_open(os.fsencode(path), int(raw), ctypes.byref(h))
    elif gunzip_plain:
        rc = L.pcabi_fastx_open_dev2(os.fsencode(path), int(raw), int(gunzip_device), OPEN_GUNZIP_PLAIN, ctypes.byref(h))
    else:
        rc = L.pcabi_fastx_open_dev(os.fsencode(path), int(raw), int(gunzip_device), ctypes.byref(h))
    if rc == 0 and keep_aux:
        L.pcabi_fastx_keep_aux(h, 1)
    if rc == 0 and tags_from_headers:
        rc = L.pcabi_fastx_header_tags(h, 1, -1 if tags_device is None else int(tags_device))
        if rc != 0:
            L.pcabi_fastx_close(h)
    return rc, h


def _bam_header(L, h):
    """A BAM reader's header text (bytes) once it has read a batch; None for any other input."""
    p, n = ctypes.c_void_p(), ctypes.c_int64()
    L.pcabi_fastx_bam_header(h, ctypes.byref(p), ctypes.byref(n))
    return ctypes.string_at(p.value, n.value) if n.value > 0 else None


def ramp_sizes(max_reads, remaining_reads=None, done=0):
    """The next batch's read count for a pipeline's ramp (misc.read_batches ramp=True): batches
    grow from max_reads / 8 by doubling (the later stages start after a small first parse) and,
    once fewer than 1.5 x max_reads reads remain (remaining_reads, estimated from the bytes left),
    take half of what remains, down to max_reads / 8 (the last write is a small one, overlapped by
    the trims before it). done: batches already read."""
    lo = max(1, max_reads // 8)
    want = min(max_reads, lo << done)
    if remaining_reads is not None and remaining_reads < 1.5 * max_reads:
        want = min(want, remaining_reads if remaining_reads <= 2 * lo else (remaining_reads + 1) // 2)
    return max(1, int(want))


def read_batches(path, max_reads=100000, max_bases=1 << 30, raw=False, byte_range=None, first_reads=None,
                 ramp=False, gunzip_device=None, keep_aux=False, gunzip_plain=False, tags_from_headers=False):
    """Stream a FASTA / FASTQ(.gz) or unaligned BAM file as ReadBatch objects (pcabi_fastx_next; a BAM
    file's records arrive as FASTQ batches, see include/pcabi.h "unaligned BAM input"); byte_range =
    (begin, end) record starts of a plain file (record_boundaries) reads only that range;
    first_reads: the first batch's size, if other than max_reads (a pipeline starts its later
    stages sooner on a small first batch); ramp: batch sizes from ramp_sizes (a plain file's last
    batches shrink too, from the bytes left and the bytes per read so far). Batching never changes
    what is read or written, only when. gunzip_device: a GPU that inflates a block-gzipped (BGZF)
    input (pcabi_fastx_open_dev) and, for a BAM file, unpacks its records; None reads every gzip
    input with zlib; gunzip_plain (with gunzip_device): ordinary gzip, which has no index, is inflated
    there too, in parallel from speculative block starts (include/pcabi.h pcabi_gunzip_stream_*).
    keep_aux: a BAM input's batches keep their records' aux tags (ReadBatch.aux),
    for write_reads(..., 'bam', keep_aux=True); any other input: no effect, unless tags_from_headers
    (with keep_aux) asks for the tags a FASTA / FASTQ input carries in its headers, as `samtools fastq -T`,
    `dorado --emit-fastq` and write_reads(header_tags=True) write them: the tab-separated TG:T:value
    fields of every header are parsed into aux bytes (include/pcabi.h "SAM tags read from FASTQ / FASTA
    headers"), on gunzip_device when given, else with the host build, and the batch is written like one
    read from BAM (engine.auxparse_counts() tells how many tags were read
    and how many fields left out). A BAM input's batches carry its header text (ReadBatch.bam_header)."""
    _check_gunzip_plain(gunzip_device, gunzip_plain)
    _check_tags_from_headers(tags_from_headers, keep_aux, raw)
    L = _declare(lib())
    rc, h = _fastx_open(L, path, raw, gunzip_device, keep_aux, gunzip_plain, tags_from_headers, gunzip_device)
    if rc != 0:
        raise ValueError(_open_error(path))
    if byte_range is not None and L.pcabi_fastx_set_range(h, int(byte_range[0]), int(byte_range[1])) != 0:
        L.pcabi_fastx_close(h)
        raise ValueError(_open_error(path))
    try:
        want = int(first_reads) if first_reads else (ramp_sizes(int(max_reads)) if ramp else int(max_reads))
        left0 = L.pcabi_fastx_remaining(h)
        n_done, b_done, k = 0, 0, 0
        while True:
            b = ctypes.c_void_p()
            n = L.pcabi_fastx_next(h, want, int(max_bases), ctypes.byref(b))
            if n < 0:
                raise ValueError(_open_error(path))
            if n == 0:
                L.pcabi_reads_free(b)
                return
            k += 1
            want = int(max_reads)
            if ramp:
                left = L.pcabi_fastx_remaining(h)
                n_done += n
                est = None
                if left >= 0 and left0 > 0:
                    b_done = left0 - left
                    est = int(left * n_done / max(1, b_done))
                want = ramp_sizes(int(max_reads), est, k)
            yield ReadBatch(b, _bam_header(L, h))
    finally:
        L.pcabi_fastx_close(h)


def text_chunks(path, chunk_bytes, gunzip_device=None, gunzip_plain=False):
    """Stream a FASTA / FASTQ(.gz) file (not BAM: its records are binary, the reader refuses) as
    spans of its decoded text holding whole records, cut
    where a fresh reader parses the same records (pcabi_fastx_next_text): yields memoryviews of at
    least chunk_bytes (the last may be shorter), each valid until the next one is requested.
    gunzip_device, gunzip_plain: as in read_batches."""
    _check_gunzip_plain(gunzip_device, gunzip_plain)
    L = _declare(lib())
    rc, h = _fastx_open(L, path, 0, gunzip_device, False, gunzip_plain)
    if rc != 0:
        raise ValueError(_open_error(path))
    try:
        while True:
            p, n = ctypes.c_void_p(), ctypes.c_int64()
            rc = L.pcabi_fastx_next_text(h, int(chunk_bytes), ctypes.byref(p), ctypes.byref(n))
            if rc < 0:
                raise ValueError(_open_error(path))
            if rc == 0:
                return
            yield memoryview((ctypes.c_char * int(n.value)).from_address(p.value)).cast('B')
    finally:
        L.pcabi_fastx_close(h)


def load_batch(path, raw=False, gunzip_device=None, keep_aux=False, gunzip_plain=False, tags_from_headers=False):
    """The whole FASTA, FASTQ or BAM file as one ReadBatch (pcabi_fastx_load); raw keeps the file's
    own text. gunzip_device: a GPU that inflates a block-gzipped (BGZF) input, a BAM file included,
    whose records are then unpacked there too (pcabi_fastx_open_dev). keep_aux, gunzip_plain,
    tags_from_headers: as in read_batches."""
    _check_gunzip_plain(gunzip_device, gunzip_plain)
    _check_tags_from_headers(tags_from_headers, keep_aux, raw)
    L = _declare(lib())
    b = ctypes.c_void_p()
    bam = is_bam(path)
    plain = bool(gunzip_plain) and not bam and get_compression_type(path) == 'gz' and not _starts_bgzf(path)
    if bam or plain or tags_from_headers or (gunzip_device is not None and _starts_bgzf(path)):
        rc, h = _fastx_open(L, path, raw, gunzip_device if (plain or _starts_bgzf(path)) else None, keep_aux, plain,
                            tags_from_headers, gunzip_device)
        if rc != 0:
            raise ValueError(_open_error(path))
        try:
            if L.pcabi_fastx_next(h, (1 << 63) - 1, (1 << 63) - 1, ctypes.byref(b)) < 0:
                raise ValueError(_open_error(path))
            # one more call, whatever the type: a BAM reader delivers the records before a fault first
            # and raises on the next call; a FASTA / FASTQ reader returns no records here
            more = ctypes.c_void_p()
            rc = L.pcabi_fastx_next(h, 1, 1, ctypes.byref(more))
            if rc >= 0:
                L.pcabi_reads_free(more)
            else:
                L.pcabi_reads_free(b)
                raise ValueError(_open_error(path))
            header = _bam_header(L, h)
        finally:
            L.pcabi_fastx_close(h)
        return ReadBatch(b, header)
    rc = L.pcabi_fastx_load(os.fsencode(path), int(raw), ctypes.byref(b))
    if rc != 0:
        raise ValueError(_open_error(path))
    return ReadBatch(b)


# ---- the reference's Python surface (porechop_abi/misc.py) -----------------------------------
def get_compression_type(filename):
    """misc.py:60-81: 'gz' / 'plain' by magic bytes; bzip2 / zip exit with the reference's text."""
    with open(filename, 'rb') as f:
        start = f.read(4)
    if start.startswith(b'\x1f\x8b\x08'):
        return 'gz'
    if start.startswith(b'\x42\x5a\x68'):
        sys.exit('Error: cannot use bzip2 format - use gzip instead')
    if start.startswith(b'\x50\x4b\x03\x04'):
        sys.exit('Error: cannot use zip format - use gzip instead')
    return 'plain'


def load_fasta_or_fastq(filename):
    """misc.py:108-120 through the native reader in raw mode (the file's own text; the reference
    normalises it later, in NanoporeRead). FASTA, FASTQ or BAM: a BAM file gives the 'FASTQ' tuples
    (empty spacer line)."""
    if not os.path.isfile(filename):
        sys.exit('Error: could not find ' + filename)
    get_compression_type(filename)
    try:
        b = load_batch(filename, raw=True)
    except ValueError:
        sys.exit('\nError: ' + filename + ' could not be parsed - is it formatted correctly?')
    if b.type == FASTA:
        recs = []
        for i in range(b.n):
            full = b.name(i)
            recs.append((full.split()[0], b.sequence(i), full))
        return recs, 'FASTA'
    recs = []
    for i in range(b.n):
        full = b.name(i)
        recs.append((full.split()[0], b.sequence(i), b.spacer_line(i), b.quals(i), full))
    return recs, 'FASTQ'


# Terminal formatting of the verbose output (misc.py:270-316): the same escape codes.
END_FORMATTING = '\033[0m'
BOLD = '\033[1m'
UNDERLINE = '\033[4m'
RED = '\033[31m'
YELLOW = '\033[93m'


def red(text):
    return RED + text + END_FORMATTING


def yellow(text):
    return YELLOW + text + END_FORMATTING


def add_line_breaks_to_sequence(sequence, line_length):
    """misc.py:327-338."""
    if not sequence:
        return '\n'
    return ''.join(sequence[p:p + line_length] + '\n' for p in range(0, len(sequence), line_length))


def load_reads(input_file_or_directory, verbosity, print_dest, check_read_count):
    """porechop_abi.py:133-187: NanoporeRead objects from a FASTA, FASTQ or BAM file, or from every
    *.fastq(.gz)
    under an Albacore-style directory (check reads spread over the files, barcode from the path)."""
    if os.path.isfile(input_file_or_directory):
        if verbosity > 0:
            print('\nLoading reads', flush=True, file=print_dest)
            print(input_file_or_directory, flush=True, file=print_dest)
        get_compression_type(input_file_or_directory)
        try:
            b = load_batch(input_file_or_directory)
        except ValueError:
            sys.exit('\nError: ' + input_file_or_directory + ' could not be parsed - is it formatted correctly?')
        reads = b.nanopore_reads()
        read_type = 'FASTA' if b.type == FASTA else 'FASTQ'
        check_reads = reads[:check_read_count]
    elif os.path.isdir(input_file_or_directory):
        fastqs = sorted([os.path.join(d, f) for d, _, fs in os.walk(input_file_or_directory) for f in fs
                         if f.lower().endswith('.fastq') or f.lower().endswith('.fastq.gz')])
        if not fastqs:
            sys.exit('Error: could not find fastq files in ' + input_file_or_directory)
        reads, check_reads, read_type = [], [], 'FASTQ'
        per_file = int(round(check_read_count / len(fastqs)))
        for fq in fastqs:
            if verbosity > 0:
                print(fq, flush=True, file=print_dest)
            file_reads = load_batch(fq).nanopore_reads()
            bc = get_albacore_barcode_from_path(fq)
            for r in file_reads:
                r.albacore_barcode_call = bc
            reads += file_reads
            check_reads += file_reads[:per_file]
    else:
        sys.exit('Error: could not find ' + input_file_or_directory)
    if verbosity > 0:
        print('{:,}'.format(len(reads)) + ' reads loaded\n\n', flush=True, file=print_dest)
    return reads, check_reads, read_type


def get_albacore_barcode_from_path(albacore_path):
    """porechop_abi.py:190-197: the last /barcodeNN/ directory of the path."""
    import re
    if '/unclassified/' in albacore_path:
        return 'none'
    matches = re.findall('/barcode(\\d\\d)/', albacore_path)
    return 'BC' + matches[-1] if matches else None


def write_reads(batch, path, out_format='fastq', start_trim=None, end_trim=None, middle_cuts=None,
                min_split_read_size=1000, discard_middle=False, untrimmed=False, select=None, append=False,
                cut_arrays=None, gzip_device=None, bgzf=False, bam_header=None, keep_aux=False, keep_mods=False,
                keep_moves=False, header_tags=False):
    """NanoporeRead.get_fasta / get_fastq for every read of a ReadBatch, natively
    (pcabi_reads_write). Returns how many reads produced output (a non-empty read string). out_format: 'fasta' | 'fastq' | 'fasta.gz' | 'fastq.gz'.
    gzip_device: None compresses a '.gz' format with zlib on the host; a device index compresses it on
    that GPU (pcabi_reads_write_dev, gz = 2: a multi-member gzip file of the same text). bgzf (with
    gzip_device): gz = 3, one indexed BGZF member per block of at most 65280 bytes, which bgzip,
    htslib and this project's device reader take member by member; the end-of-file marker is not
    written, so batches can be appended: bgzf_finish(path) closes the file.
    out_format 'bam' (pcabi_reads_write_bam): unaligned BAM records in BGZF members of 65280 bytes,
    packed and compressed on GPU gzip_device, or on the host (zlib) when it is None; both give the same
    decoded bytes. A first write (append=False) starts with the BAM header, whose text is bam_header
    (bytes; None: '@HD\tVN:1.6\tSO:unknown\n'); bgzf_finish(path) closes the file. A record's name is
    the header up to its first space or tab (header comments are dropped), RNA reads are written with
    T, a FASTA batch has absent qualities, a quality-less FASTQ record's '+' padding is Phred 10.
    keep_aux: write the aux tags a batch read with keep_aux holds -- verbatim for a read written whole
    and as stored, without the position-dependent tags MM ML MN Mm Ml mv (dropped, not recomputed) for
    a trimmed read, a split piece or a read from a reverse-strand record. keep_mods (with keep_aux):
    MM ML MN Mm Ml are recomputed for such a read instead (include/pcabi.h "base-modification tags"),
    on gzip_device when it is given; a read whose tags are not usable loses them as before.
    engine.mods_counts() tells how many reads went which way. keep_moves (with keep_aux, independent of
    keep_mods; pcabi_reads_write_bam_tags): such a read's move table mv is cut to each part and its ts
    moved along (include/pcabi.h "move tables"), behind the other tags and MM ML MN; a read whose table
    is not usable loses mv as before and keeps its ts; engine.moves_counts() tells how many went which
    way. Direct-RNA move tables (which run against the sequence) and the sp / pi tags are not handled.
    header_tags (the four text formats, with keep_aux; pcabi_reads_write_tags): every record's header is
    its name followed by the SAM text (tab-separated TG:T:value fields, what `samtools fastq -T` writes
    and `minimap2 -y` reads) of the aux bytes out_format 'bam' would give the same part with the same
    keep_aux / keep_mods / keep_moves, which are accepted for a text format only together with it. A
    '.gz' format with gzip_device lays the text out and compresses it on that GPU; every other case
    builds it on the host; both give the same decompressed bytes. A batch without aux bytes writes what
    it writes without header_tags. A batch whose tags were read from its own headers (read_batches
    tags_from_headers) is written with the header up to its first tab as the name, so the tag text it
    came with is not repeated in front of the new. engine.auxtext_counts() tells how many tags were written and how
    many were left out (a name outside [A-Za-z][A-Za-z0-9], an A / Z / H value with a byte outside
    0x20..0x7E).
    middle_cuts: per read a list of (begin, end) ranges of the trimmed sequence (the reference's
    middle_trim_positions as ranges), or None; cut_arrays: the same as (cut_off int64 [n + 1],
    cuts int64 [2 * n_cuts]) arrays."""
    L = _declare(lib())
    gz = out_format.endswith('.gz')
    fasta = out_format.startswith('fasta')
    n = batch.n
    st = None if start_trim is None else np.ascontiguousarray(start_trim, np.int32)
    et = None if end_trim is None else np.ascontiguousarray(end_trim, np.int32)
    co = cu = None
    if cut_arrays is not None:
        co = np.ascontiguousarray(cut_arrays[0], np.int64)
        cu = np.ascontiguousarray(cut_arrays[1], np.int64)
        if cu.size == 0:
            cu = np.zeros(2, np.int64)
    elif middle_cuts is not None:
        co = np.zeros(n + 1, np.int64)
        flat = []
        for i, rg in enumerate(middle_cuts):
            rg = [(int(a), int(b)) for a, b in (rg or []) if b > a]
            co[i + 1] = co[i] + len(rg)
            for a, b in rg:
                flat += [a, b]
        cu = np.array(flat if flat else [0, 0], np.int64)
    sel = None if select is None else np.ascontiguousarray(select, np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
    if bgzf and not (gz and gzip_device is not None):
        raise ValueError("bgzf applies to a '.gz' format compressed on a device (gzip_device)")
    if header_tags and out_format == 'bam':
        raise ValueError("header_tags applies to the text formats: out_format 'bam' carries its tags itself")
    if header_tags and not keep_aux:
        raise ValueError('header_tags needs keep_aux')
    if keep_mods and not (keep_aux and (out_format == 'bam' or header_tags)):
        raise ValueError("keep_mods applies to out_format 'bam' with keep_aux")
    if keep_moves and not (keep_aux and (out_format == 'bam' or header_tags)):
        raise ValueError("keep_moves applies to out_format 'bam' with keep_aux")
    if out_format == 'bam':
        hdr = None if bam_header is None else bytes(bam_header)
        if keep_moves:
            rc = L.pcabi_reads_write_bam_tags(batch._h, os.fsencode(path), int(append), p(st), p(et), p(co), p(cu),
                                              int(min_split_read_size), int(discard_middle), int(untrimmed), p(sel), hdr,
                                              0 if hdr is None else len(hdr), 2 if keep_mods else 1, 1,
                                              -1 if gzip_device is None else int(gzip_device))
            if rc < 0:
                check(rc, 'pcabi_reads_write_bam_tags')
            return int(rc)
        rc = L.pcabi_reads_write_bam(batch._h, os.fsencode(path), int(append), p(st), p(et), p(co), p(cu),
                                     int(min_split_read_size), int(discard_middle), int(untrimmed), p(sel), hdr,
                                     0 if hdr is None else len(hdr), 2 if keep_mods else int(bool(keep_aux)),
                                     -1 if gzip_device is None else int(gzip_device))
        if rc < 0:
            check(rc, 'pcabi_reads_write_bam')
        return int(rc)
    if header_tags:
        mode = (3 if bgzf else 2) if (gz and gzip_device is not None) else int(gz)
        rc = L.pcabi_reads_write_tags(batch._h, os.fsencode(path), int(append), mode, int(fasta), p(st), p(et), p(co), p(cu),
                                      int(min_split_read_size), int(discard_middle), int(untrimmed), p(sel),
                                      -1 if gzip_device is None else int(gzip_device), 2 if keep_mods else 1,
                                      1 if keep_moves else 0, 1)
        if rc < 0:
            check(rc, 'pcabi_reads_write_tags')
        return int(rc)
    if gz and gzip_device is not None:
        rc = L.pcabi_reads_write_dev(batch._h, os.fsencode(path), int(append), 3 if bgzf else 2, int(fasta), p(st), p(et), p(co),
                                     p(cu), int(min_split_read_size), int(discard_middle), int(untrimmed), p(sel),
                                     int(gzip_device))
    else:
        rc = L.pcabi_reads_write(batch._h, os.fsencode(path), int(append), int(gz), int(fasta), p(st), p(et), p(co),
                                 p(cu), int(min_split_read_size), int(discard_middle), int(untrimmed), p(sel))
    if rc < 0:
        check(rc, 'pcabi_reads_write')
    return int(rc)


def write_bam_header(path, bam_header=None):
    """A BAM file that holds its header and no record (what write_reads(..., 'bam') starts a file
    with), for an input without reads: one BGZF member, made here with zlib. bgzf_finish closes it."""
    import struct
    import zlib
    text = b'@HD\tVN:1.6\tSO:unknown\n' if bam_header is None else bytes(bam_header)
    data = b'BAM\1' + struct.pack('<i', len(text)) + text + struct.pack('<i', 0)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = c.compress(data) + c.flush()
    with open(path, 'wb') as f:
        f.write(b'\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0' + struct.pack('<H', len(body) + 25) + body +
                struct.pack('<II', zlib.crc32(data), len(data)))


def bgzf_finish(path):
    """Append the 28-byte BGZF end-of-file marker to a file written with write_reads(bgzf=True) or
    write_reads(out_format='bam') (pcabi_bgzf_write_eof)."""
    L = _declare(lib())
    check(L.pcabi_bgzf_write_eof(os.fsencode(path)), 'pcabi_bgzf_write_eof')


def positions_to_ranges(positions):
    """A set of positions (NanoporeRead.middle_trim_positions) -> sorted disjoint [a, b) ranges."""
    out = []
    for x in sorted(positions):
        if out and out[-1][1] == x:
            out[-1][1] = x + 1
        else:
            out.append([x, x + 1])
    return [tuple(r) for r in out]
