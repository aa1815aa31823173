"""File-to-file trimming on one GPU: the CLI's hot path without per-read Python objects
(porechop_abi/porechop_abi.py:41-131 after adapter-set discovery).

    ReadBatch (native parse, misc.read_batches)
      -> H2D of the packed Dna5 codes, start / end window views        (engine layout, no repack)
      -> k_tile_windows / k_align cross products / k_end_trim           (find_adapters_at_read_ends)
      -> trims D2H (8 B / read)
      -> opt-in: the quality stage crops the trimmed spans and tests the reads (pcabi_qual_filter_dev)
      -> pcabi_middle_scan_dev over the trimmed reads                   (find_adapters_in_read_middles)
      -> middle cut ranges (NanoporeRead._apply_middle_hit: pcabi_middle_cuts on the device)
      -> the fork's start-and-end filter (porechop_abi.py:36-39)
      -> native trimmed FASTA / FASTQ writer                             (output_reads, get_fastq)

Decisions are the reference's (same kernels and epilogues the parity tests cover); barcode
demultiplexing and verbose output stay with the per-read drivers (porechop_abi.py here).
"""
import ctypes
import os
import queue
import threading
import time

import numpy as np

from . import misc
from ._lib import check, cross_regions, lib
from .engine import QUAL_FAIL, QUAL_LOW_QUALITY, QUAL_NO_QUALITIES, QUAL_PIECE, QUAL_READ, QUAL_TOO_LONG, QUAL_TOO_SHORT, \
    encode_adapters, middle_cuts, qual_opts
from .porechop_abi import middle_adapter_list

VP = ctypes.c_void_p


def _bgzf_mode(trimmer, out_format):
    """Whether this trimmer writes out_format as BGZF: the option, a '.gz' format, the device encoder
    (trim_file also serves trimmers that are not FileTrimmers and know none of these)."""
    return bool(getattr(trimmer, 'bgzf', False)) and out_format.endswith('.gz') and \
        getattr(trimmer, 'gzip_device', None) is not None


def _finish_mode(trimmer, out_format):
    """Whether the files of this run end with the BGZF end-of-file marker: BGZF text, or BAM."""
    return out_format == 'bam' or _bgzf_mode(trimmer, out_format)


def _trimmed_span(lens, st, et):
    """get_seq_with_start_end_adapters_trimmed (nanopore_read.py:66-71): the Python slice seq[st:len - et]
    of the reference as (first base, length) per read; a read with st == et == 0 is taken whole."""
    trimmed = (st > 0) | (et > 0)
    end = lens - et
    end = np.where(end < 0, np.maximum(lens + end, 0), end)
    a = np.minimum(st, lens)
    return np.where(trimmed, a, 0), np.where(trimmed, np.maximum(end - a, 0), lens)


def _bam_kw(trimmer, out_format, b):
    """misc.write_reads' BAM arguments for batch b: the input's header text when it was BAM, and the
    trimmer's keep_tags, keep_mods and keep_moves; for a text format with header_tags, the same tag
    options and header_tags (misc.write_reads)."""
    keep = bool(getattr(trimmer, 'keep_tags', False))
    if out_format != 'bam':
        if not (keep and getattr(trimmer, 'header_tags', False)):
            return {}
        return {'keep_aux': True, 'header_tags': True, 'keep_mods': bool(getattr(trimmer, 'keep_mods', False)),
                'keep_moves': bool(getattr(trimmer, 'keep_moves', False))}
    return {'bam_header': getattr(b, 'bam_header', None), 'keep_aux': keep,
            'keep_mods': keep and bool(getattr(trimmer, 'keep_mods', False)),
            'keep_moves': keep and bool(getattr(trimmer, 'keep_moves', False))}


class FileTrimmer(object):
    """Device state for trimming batches against one list of matching adapter sets.

    Options follow the reference's arguments (arg_parser.py defaults): end_size 150,
    end_threshold 75, extra_end_trim 2, min_trim_size 4, middle_threshold 90, extra middle trim
    10 (good side) / 100 (bad side), min_split_read_size 1000, no_split False, discard_middle
    False, adapter filter on (the fork's).

    The quality stage (off by default; on when quality_window, min_length, max_length or min_mean_q is
    set) does on the device what NanoFilt, chopper or fastplong's --cut_front --cut_tail --mean_qual
    --length_required do to the trimmed file (engine.quality_filter; the rule: include/pcabi.h). It runs
    after the end trim and before the middle scan on the span the adapter trims left: quality_window /
    quality_window_q crop the span at both ends to its outermost windows of quality_window bases with a
    mean Phred of quality_window_q or more, and the crops are added to start_trim / end_trim, so every
    writer, BAM with remapped MM ML MN mv ts included, writes the cropped read as it writes a trimmed
    one; min_length / max_length / min_mean_q (the Phred of the mean error probability) then test the
    kept span and clear the read's keep bit. A read without qualities is not cropped and passes the
    quality test. The fork's start-and-end filter still goes by the adapter trims; with
    filter_reads=False keep is the pass mask. The filter sees the kept span with its middle adapters:
    split pieces are not filtered one by one unless quality_per_piece is set (below). The barcode bins go through the same trims and keep mask;
    with untrimmed=True their writer ignores the trims, as it does today, so the crop is not visible
    there while the filter still applies. last_quality holds the last batch's QUAL_READ records.

    quality_per_piece=True (it needs the stage on) judges split reads piece by piece, as a filter run on
    the written file would: after the middle scan the pieces the writers would cut a split read into are
    cropped and tested on the device like reads of their own (engine.quality_filter_pieces, the rule:
    include/pcabi.h), and trim() returns in place of the scan's cuts a cut layout with which every writer,
    the bins' included, emits exactly the cropped, passing pieces, numbered _1, _2, ... over the pieces
    written, min_split_read_size applying to the cropped piece. A split read's keep bit no longer takes the
    whole-read verdict (a read all of whose pieces fail writes nothing); the fork's start-and-end filter
    and discard_middle are unchanged. last_quality_pieces holds the last batch's QUAL_PIECE records,
    last_piece_off their offsets per read."""

    barcode_dir = None                    # -b off (set by __init__)
    gzip_device = None                    # '.gz' formats through zlib on the host (set by __init__)
    bgzf = False                          # device-compressed '.gz' output as plain multi-member gzip
    gunzip_device = None                  # gzip inputs through zlib on the host (set by __init__)
    gunzip_plain = False                  # with gunzip_device: ordinary gzip inputs on the device too
    keep_tags = False                     # BAM to BAM: aux tags are dropped (set by __init__)
    keep_mods = False                     # with keep_tags: MM ML MN of changed reads are dropped, not remapped
    keep_moves = False                    # with keep_tags: mv of changed reads is dropped, ts copied
    header_tags = False                   # with keep_tags: text outputs carry no tags in their headers
    tags_from_headers = False             # with keep_tags: a text input's headers are not parsed for tags
    quality_window = 0                    # no quality crop
    quality_window_q = 0.0                # with quality_window: every window qualifies
    min_length = 0                        # no read is too short
    max_length = 0                        # no read is too long
    min_mean_q = 0.0                      # no read is of too low a quality
    last_quality = None                   # the quality stage's records of the last batch (stage on)
    quality_per_piece = False             # split reads are judged whole, middle adapters included
    last_quality_pieces = None            # the piece stage's records of the last batch (quality_per_piece)
    last_piece_off = None                 # read r's pieces: last_quality_pieces[last_piece_off[r]:last_piece_off[r + 1]]

    def __init__(self, matching_sets, scoring_scheme_vals=(3, -6, -5, -2), end_size=150, end_threshold=75.0,
                 extra_end_trim=2, min_trim_size=4, middle_threshold=90.0, extra_middle_trim_good_side=10,
                 extra_middle_trim_bad_side=100, min_split_read_size=1000, no_split=False, discard_middle=False,
                 filter_reads=True, device=0, barcode_dir=None, forward_or_reverse_barcodes='forward',
                 barcode_threshold=75.0, barcode_diff=5.0, require_two_barcodes=False, untrimmed=False,
                 discard_unassigned=False, gzip_on_device=False, gunzip_on_device=False, bgzf=False, keep_tags=False,
                 keep_mods=False, keep_moves=False, gunzip_plain=False, header_tags=False, tags_from_headers=False, quality_window=0,
                 quality_window_q=0.0, min_length=0, max_length=0, min_mean_q=0.0, quality_per_piece=False):
        self.L = L = lib()
        if not 0 <= int(quality_window) <= 64:
            raise ValueError('quality_window is 0 (off) or 1..64')
        self.quality_window, self.quality_window_q = int(quality_window), float(quality_window_q)
        self.min_length, self.max_length, self.min_mean_q = int(min_length), int(max_length), float(min_mean_q)
        if quality_per_piece and not self._quality_on():
            raise ValueError('quality_per_piece needs the quality stage on (quality_window, min_length, max_length or min_mean_q)')
        self.quality_per_piece = bool(quality_per_piece)
        # tags_from_headers: a FASTA / FASTQ input's tags are read from its headers (misc.read_batches
        # tags_from_headers; on the device with gunzip_on_device, else the host build), so every writer,
        # the bins' included, carries them as it carries a BAM input's
        if tags_from_headers and not keep_tags:
            raise ValueError('tags_from_headers needs keep_tags')
        self.tags_from_headers = bool(tags_from_headers)
        # header_tags: a text output format carries each part's tags in its header as SAM text
        # (misc.write_reads header_tags), the bins' writers included; gzip_on_device lays the text out on
        # the device
        if header_tags and not keep_tags:
            raise ValueError('header_tags needs keep_tags')
        self.header_tags = bool(header_tags)
        # out_format 'bam' from a BAM input: the records' aux tags are read and written (misc.write_reads
        # keep_aux: verbatim on reads written whole and as stored, without the position-dependent tags
        # MM ML MN Mm Ml mv, which are dropped and not recomputed, on changed reads)
        self.keep_tags = bool(keep_tags)
        # keep_mods: MM ML MN Mm Ml of a changed read are recomputed for each part it is written as
        # (misc.write_reads keep_mods), the bins' writers included
        if keep_mods and not keep_tags:
            raise ValueError('keep_mods needs keep_tags')
        self.keep_mods = bool(keep_mods)
        # keep_moves: mv of a changed read is cut to each part it is written as and ts moved along
        # (misc.write_reads keep_moves), the bins' writers included
        if keep_moves and not keep_tags:
            raise ValueError('keep_moves needs keep_tags')
        self.keep_moves = bool(keep_moves)
        self.device = int(device)
        # '.gz' output formats: zlib on the host (default) or the device encoder (misc.write_reads)
        self.gzip_device = self.device if gzip_on_device else None
        # with gzip_on_device: '.gz' output as indexed BGZF members (misc.write_reads bgzf), every
        # file the run wrote (bins included) finished with the end-of-file marker
        if bgzf and not gzip_on_device:
            raise ValueError('bgzf needs gzip_on_device=True')
        self.bgzf = bool(bgzf)
        # block-gzipped (BGZF) inputs: zlib on the host (default) or inflated on the device by the reader
        # thread (misc.read_batches gunzip_device); any other input reads as before
        self.gunzip_device = self.device if gunzip_on_device else None
        # with gunzip_on_device: ordinary gzip inputs (no index) are inflated on the device as well
        # (misc.read_batches gunzip_plain)
        if gunzip_plain and not gunzip_on_device:
            raise ValueError('gunzip_plain needs gunzip_on_device=True')
        self.gunzip_plain = bool(gunzip_plain)
        check(L.pcabi_dev_set(device), 'pcabi_dev_set')
        self.sc = tuple(int(x) for x in scoring_scheme_vals[:4])
        self.E, self.thr, self.extra, self.min_trim = int(end_size), float(end_threshold), int(extra_end_trim), \
            int(min_trim_size)
        self.mthr, self.good, self.bad = float(middle_threshold), int(extra_middle_trim_good_side), \
            int(extra_middle_trim_bad_side)
        self.min_split, self.no_split, self.discard_middle = int(min_split_read_size), bool(no_split), \
            bool(discard_middle)
        # the reference filters only when some adapter set matched (porechop_abi.py:93-122); with
        # none, every read is written unchanged
        self.filter_reads = bool(filter_reads) and bool(matching_sets)
        self.start_adps = [a.start_sequence[1] for a in matching_sets if a.start_sequence]
        self.end_adps = [a.end_sequence[1] for a in matching_sets if a.end_sequence]
        mids, start_names, end_names = middle_adapter_list(matching_sets)
        self.mid_adps = [x[1] for x in mids]
        self.bad_start = np.array([x[0] in start_names for x in mids], bool)
        self.bad_end = np.array([x[0] in end_names for x in mids], bool)
        self.tabs = [self._table(x) for x in (self.start_adps, self.end_adps, self.mid_adps)]
        self.scan = VP()
        if self.mid_adps:
            check(L.pcabi_scan_create(self.tabs[2], ctypes.byref(self.scan)), 'pcabi_scan_create')
        self.stream = VP()
        check(L.pcabi_stream_create(ctypes.byref(self.stream)), 'pcabi_stream_create')
        self.dev = {}
        self.times = {}
        # -b: barcode bins (porechop_abi.py:80-104, 581-638). The dicts find_start_trim /
        # find_end_trim fill become slot tables (porechop_abi.barcode_slots), the call runs on the
        # device after the end trim (pcabi_barcode_call_dev), and the writer sends every read to
        # <barcode_dir>/<call>.<format>; --untrimmed and --discard_unassigned as the reference
        # (the former only applies to bins there too).
        self.barcode_dir = barcode_dir
        if barcode_dir is not None:
            from .porechop_abi import barcode_slots
            ids = {}
            start_sets = [a for a in matching_sets if a.start_sequence]
            end_sets = [a for a in matching_sets if a.end_sequence]
            self.bc_slots = (barcode_slots(start_sets, forward_or_reverse_barcodes, ids),
                             barcode_slots(end_sets, forward_or_reverse_barcodes, ids))
            self.bc_names = {v: k for k, v in ids.items()}
            self.bc_thr, self.bc_diff, self.bc_two = float(barcode_threshold), float(barcode_diff), \
                bool(require_two_barcodes)
            self.untrimmed, self.discard_unassigned = bool(untrimmed), bool(discard_unassigned)

    def _table(self, seqs):
        if not seqs:
            return None
        c, o, l = encode_adapters(seqs)
        t = VP()
        check(self.L.pcabi_adapters_create_scored(c.ctypes.data_as(VP), o.ctypes.data_as(VP), l.ctypes.data_as(VP),
                                                  len(seqs), *self.sc, ctypes.byref(t)), 'pcabi_adapters_create')
        return t

    def _buf(self, key, nbytes):
        nbytes = max(int(nbytes), 16)
        if key not in self.dev or self.dev[key][1] < nbytes:
            if key in self.dev:
                # grown with headroom: batches of varying size do not reallocate (a free waits for
                # the device) every time one is a little larger than the last
                nbytes = max(nbytes, self.dev[key][1] + self.dev[key][1] // 4)
                self.L.pcabi_dev_free(self.dev[key][0])
            p = VP()
            check(self.L.pcabi_dev_malloc(ctypes.byref(p), nbytes), 'pcabi_dev_malloc')
            self.dev[key] = (p, nbytes)
        return self.dev[key][0]

    def _h2d(self, key, arr):
        arr = np.ascontiguousarray(arr)
        p = self._buf(key, arr.nbytes)
        if arr.nbytes:
            check(self.L.pcabi_dev_copy_async(p, arr.ctypes.data_as(VP), arr.nbytes, 0, self.stream), 'h2d')
        return p

    def _quality_on(self):
        return self.quality_window > 0 or self.min_length > 0 or self.max_length > 0 or self.min_mean_q > 0

    def _quality_stage(self, batch, lens, trims, d_qual):
        """The quality stage on the spans the adapter trims left (the qualities are on their way to the
        device): -> (start_trim, end_trim) with the crops added, and the reads' QUAL_READ records."""
        L, nb = self.L, batch.n
        st, et = trims[0].astype(np.int64), trims[1].astype(np.int64)
        a, n = _trimmed_span(lens, st, et)
        has_q = np.diff(batch.qual_off) == lens
        span_off = np.where(has_q, batch.qual_off[:-1] + a, -1).astype(np.int64)
        span_len = n.astype(np.int32)
        opts = qual_opts(self.quality_window, self.quality_window_q, self.min_length, self.max_length, self.min_mean_q)
        n_segs = int(L.pcabi_qual_seg_bound(span_len.ctypes.data_as(VP), nb))
        need = int(L.pcabi_qual_scratch_bytes(nb, n_segs))
        if need < 0:
            check(need, 'pcabi_qual_scratch_bytes')
        recs = np.zeros(nb, QUAL_READ)
        d_off, d_len = self._h2d('qoff', span_off), self._h2d('qlen', span_len)
        d_out, d_scr = self._buf('qout', recs.nbytes), self._buf('qscratch', need)
        check(L.pcabi_qual_filter_dev(d_qual, batch.qual.size, d_off, d_len, nb, n_segs, opts.ctypes.data_as(VP), d_out, d_scr, need,
                                      self.stream), 'pcabi_qual_filter_dev')
        check(L.pcabi_dev_copy_async(recs.ctypes.data_as(VP), d_out, recs.nbytes, 1, self.stream), 'd2h')
        check(L.pcabi_stream_sync(self.stream), 'sync')
        front, tail = recs['front'].astype(np.int64), recs['tail'].astype(np.int64)
        cropped = front + tail > 0
        new_st = np.where(cropped, a + front, st).astype(np.int32)
        new_et = np.where(cropped, lens - (a + n - tail), et).astype(np.int32)
        return new_st, new_et, recs

    def _piece_stage(self, batch, lens, trims, d_qual, cut_off, cuts):
        """The piece stage on the cuts the middle scan found (the qualities are still on the device; the
        spans are those the whole-read stage's trims leave): -> (cut_off', cuts', pieces, piece_off)."""
        L, nb = self.L, batch.n
        a, n = _trimmed_span(lens, trims[0].astype(np.int64), trims[1].astype(np.int64))
        has_q = np.diff(batch.qual_off) == lens
        span_off = np.where(has_q, batch.qual_off[:-1] + a, -1).astype(np.int64)
        span_len = n.astype(np.int32)
        cut_off = np.ascontiguousarray(cut_off, np.int64)
        cuts = np.ascontiguousarray(cuts, np.int64).reshape(-1)
        n_ranges = int(cut_off[-1])
        opts = qual_opts(self.quality_window, self.quality_window_q, self.min_length, self.max_length, self.min_mean_q)
        bound = np.zeros(2, np.int64)
        check(L.pcabi_qual_pieces_bound(span_len.ctypes.data_as(VP), cut_off.ctypes.data_as(VP), nb, bound[0:].ctypes.data_as(VP),
                                        bound[1:].ctypes.data_as(VP)), 'pcabi_qual_pieces_bound')
        cap, n_segs = int(bound[0]), int(bound[1])
        cuts_cap = n_ranges + 2 * cap
        need = int(L.pcabi_qual_pieces_scratch_bytes(nb, n_ranges, cap, n_segs))
        if need < 0:
            check(need, 'pcabi_qual_pieces_scratch_bytes')
        d_off, d_len = self._h2d('qoff', span_off), self._h2d('qlen', span_len)
        d_co, d_cu = self._h2d('pcut_off', cut_off), self._h2d('pcuts', cuts)
        d_po, d_pieces = self._buf('ppiece_off', 8 * (nb + 1)), self._buf('ppieces', QUAL_PIECE.itemsize * cap)
        d_co2, d_cu2 = self._buf('pcut_off2', 8 * (nb + 1)), self._buf('pcuts2', 16 * cuts_cap)
        d_scr = self._buf('pscratch', need)
        check(L.pcabi_qual_pieces_dev(d_qual, batch.qual.size, d_off, d_len, nb, d_co, d_cu, n_ranges, cap, n_segs, opts.ctypes.data_as(VP),
                                      d_po, d_pieces, d_co2, d_cu2, cuts_cap, d_scr, need, self.stream), 'pcabi_qual_pieces_dev')
        piece_off, cut_off2 = np.zeros(nb + 1, np.int64), np.zeros(nb + 1, np.int64)
        pieces, cuts2 = np.zeros(cap, QUAL_PIECE), np.zeros(2 * cuts_cap, np.int64)
        # the bounds are small next to the batch: everything comes up in one go, the counts trim it
        for dst, src in ((piece_off, d_po), (cut_off2, d_co2), (pieces, d_pieces), (cuts2, d_cu2)):
            if dst.nbytes:
                check(L.pcabi_dev_copy_async(dst.ctypes.data_as(VP), src, dst.nbytes, 1, self.stream), 'd2h')
        check(L.pcabi_stream_sync(self.stream), 'sync')
        n_pieces = int(piece_off[nb])
        if not 0 <= n_pieces <= cap or int(cut_off2[nb]) != n_ranges + 2 * n_pieces:
            raise RuntimeError('the piece stage returned %d pieces for a bound of %d' % (n_pieces, cap))
        return cut_off2, cuts2[:2 * int(cut_off2[nb])].copy(), pieces[:n_pieces].copy(), piece_off

    def _tick(self, key, t):
        now = time.perf_counter()
        self.times[key] = self.times.get(key, 0.0) + now - t
        return now

    def trim(self, batch, albacore=None):
        """Decisions for one ReadBatch: (start_trim, end_trim, cut_off, cuts, hits, keep).
        albacore: the barcode of the Albacore directory the batch came from (misc.input_files), or
        None; with -b a device call that disagrees with it becomes 'none' (nanopore_read.py:479-482)."""
        L, sc, nb = self.L, self.sc, batch.n
        t = time.perf_counter()
        lens = batch.lengths.astype(np.int64)
        E = self.E
        s_len = (np.minimum(lens, E) if E >= 0 else np.maximum(lens + E, 0)).astype(np.int32)
        if E > 0:
            e_start = np.maximum(lens - E, 0)
        elif E == 0:
            e_start = np.zeros_like(lens)
        else:
            e_start = np.minimum(-E, lens)
        e_len = (lens - e_start).astype(np.int32)
        d_codes = self._h2d('codes', batch.codes)
        quality = self._quality_on()
        # the qualities cross PCIe beside the alignment
        d_qual = self._h2d('qual', batch.qual) if quality and nb else None
        self.last_quality = np.zeros(0, QUAL_READ) if quality else None
        per_piece = quality and self.quality_per_piece
        self.last_quality_pieces = np.zeros(0, QUAL_PIECE) if per_piece else None
        self.last_piece_off = np.zeros(nb + 1, np.int64) if per_piece else None
        trims = np.zeros((2, nb), np.int32)
        res = [None, None]
        regions = []
        n_ad = (len(self.start_adps), len(self.end_adps))
        for side, (w_off, w_len) in enumerate(((batch.code_off, s_len), (batch.code_off + e_start, e_len))):
            res[side] = self._buf('res%d' % side, 4 * 8 * max(1, n_ad[side]) * nb)
            if not n_ad[side] or nb == 0:
                continue
            toff = np.zeros((nb + 255) // 256 + 1, np.int64)
            nd = L.pcabi_tile_layout(w_len.ctypes.data_as(VP), nb, toff.ctypes.data_as(VP))
            d_off, d_len = self._h2d('off%d' % side, w_off), self._h2d('len%d' % side, w_len)
            d_toff = self._h2d('toff%d' % side, toff)
            d_tiles = self._buf('tiles%d' % side, 4 * nd)
            check(L.pcabi_tile_windows_dev(d_codes, d_off, d_len, nb, d_toff, int(np.diff(toff).max() // 256), d_tiles,
                                           self.stream), 'tile')
            regions.append((d_tiles, d_toff, d_len, nb, int(w_len.max()), self.tabs[side], res[side], n_ad[side] * nb))
        if regions:
            # both read ends in one call: their register buckets in grouped launches (r06)
            arr = cross_regions(regions)
            check(L.pcabi_align_cross_multi_dev(arr, len(regions), *sc, self.stream, None, None), 'align')
        if nb:
            d_st, d_et = self._buf('st', 4 * nb), self._buf('et', 4 * nb)
            check(L.pcabi_end_trim_dev(res[0], n_ad[0] * nb, n_ad[0], res[1], n_ad[1] * nb, n_ad[1], nb, E, self.extra,
                                       self.thr, self.min_trim, d_st, d_et, None, None, self.stream), 'end_trim')
            check(L.pcabi_dev_copy_async(trims[0].ctypes.data_as(VP), d_st, 4 * nb, 1, self.stream), 'd2h')
            check(L.pcabi_dev_copy_async(trims[1].ctypes.data_as(VP), d_et, 4 * nb, 1, self.stream), 'd2h')
            if self.barcode_dir is not None:
                calls = np.full(nb, -1, np.int32)
                (sa, sn), (ea, en) = self.bc_slots
                d_call = self._buf('bcall', 4 * nb)
                slots = [self._h2d('bc%d' % i, x) for i, x in enumerate((sa, sn, ea, en))]
                check(L.pcabi_barcode_call_dev(res[0], n_ad[0] * nb, slots[0], slots[1], len(sa), res[1],
                                               n_ad[1] * nb, slots[2], slots[3], len(ea), nb, self.bc_thr,
                                               self.bc_diff, int(self.bc_two), d_call, None, self.stream),
                      'barcode_call')
                check(L.pcabi_dev_copy_async(calls.ctypes.data_as(VP), d_call, 4 * nb, 1, self.stream), 'd2h')
                self.last_calls = calls
            check(L.pcabi_stream_sync(self.stream), 'sync')
            if self.barcode_dir is not None and albacore is not None:
                self.last_calls = self.albacore_filter(self.last_calls, albacore)
        elif self.barcode_dir is not None:
            self.last_calls = np.full(nb, -1, np.int32)
        t = self._tick('end_trim', t)
        adapter_trims = trims
        if quality and nb:
            # before the middle scan forms its windows: middle cuts are positions of the trimmed sequence
            st, et, self.last_quality = self._quality_stage(batch, lens, trims, d_qual)
            trims = (st, et)
            t = self._tick('quality', t)
        cut_off, cuts, hits = self.middle_scan(batch, trims[0], trims[1], d_codes)
        t = self._tick('middle', t)
        split = None
        if per_piece and nb and int(cut_off[-1]) > 0:
            # the writers' rule: a read with a non-empty range is split; its pieces are judged, not the read
            nonempty = np.concatenate([[0], np.cumsum(cuts[1::2] > cuts[0::2])])
            split = nonempty[cut_off[1:]] > nonempty[cut_off[:-1]]
            cut_off, cuts, self.last_quality_pieces, self.last_piece_off = self._piece_stage(batch, lens, trims, d_qual, cut_off, cuts)
            t = self._tick('quality_pieces', t)
        keep = None
        if self.filter_reads:
            # the fork's filter: start AND end alignments (a recorded alignment always trims >= 1)
            keep = ((adapter_trims[0] > 0) & (adapter_trims[1] > 0)).astype(np.uint8)
        if quality:
            passed = ((self.last_quality['flags'] & QUAL_FAIL) == 0).astype(np.uint8)
            if split is not None:
                passed[split] = 1
            keep = passed if keep is None else keep & passed
        return trims[0], trims[1], cut_off, cuts, hits, keep

    def middle_scan(self, batch, start_trim, end_trim, d_codes=None):
        """The middle adapters of the reads as start_trim / end_trim leave them: (cut_off, cuts, hits).
        d_codes: the batch's codes on the device (trim() passes its copy), else they are uploaded."""
        L, sc, nb = self.L, self.sc, batch.n
        lens = batch.lengths.astype(np.int64)
        cut_off = np.zeros(nb + 1, np.int64)
        cuts = np.zeros(0, np.int64)
        hits = np.zeros((6, 0), np.int32)
        if self.mid_adps and not self.no_split and nb:
            if d_codes is None:
                d_codes = self._h2d('codes', batch.codes)
            # get_seq_with_start_end_adapters_trimmed (nanopore_read.py:66-71): the Python slice
            # seq[st:len - et] of the reference, as a window of the packed read
            a, t_len = _trimmed_span(lens, np.asarray(start_trim, np.int64), np.asarray(end_trim, np.int64))
            t_len = t_len.astype(np.int32)
            t_off = batch.code_off + a
            d_toff, d_tlen = self._h2d('toffm', t_off), self._h2d('tlenm', t_len)
            cap = max(4096, nb)
            while True:
                hits = np.zeros((6, cap), np.int32)
                nh = L.pcabi_middle_scan_dev(self.scan, d_codes, d_toff, d_tlen, t_len.ctypes.data_as(VP), nb, *sc,
                                             self.mthr, hits.ctypes.data_as(VP), cap, self.stream)
                if nh < 0:
                    check(int(nh), 'pcabi_middle_scan_dev')
                if nh <= cap:
                    break
                cap = int(nh)                 # the scan leaves the codes intact: rerun, larger

            hits = hits[:, :int(nh)]
            # NanoporeRead._apply_middle_hit's trim ranges (nanopore_read.py:242-250) on the device,
            # grouped per read in the writer's cut layout
            cut_off, cuts = middle_cuts(hits, nb, self.bad_start, self.bad_end, self.good, self.bad, self.device)
        return cut_off, cuts, hits

    def albacore_filter(self, calls, albacore):
        """determine_barcode's Albacore cross-check (nanopore_read.py:479-482): a read binned by
        Albacore keeps Porechop's call only when both agree, else it is 'none' (-1); reads of the
        'unclassified' directory (albacore 'none') all become 'none'."""
        ids = {v: k for k, v in self.bc_names.items()}
        want = ids.get(albacore, -2)
        return np.where(calls == want, calls, -1).astype(np.int32)

    def trim_file(self, in_path, out_path, out_format='fastq', max_reads=200000, byte_range=None, batch_filter=None,
                  segments=None, source=None):
        """Trim a FASTA / FASTQ(.gz) file -- or an Albacore output directory, its *.fastq(.gz) files
        in sorted order as load_reads reads them (porechop_abi.py:133-187), each batch carrying
        its file's barcode for the -b cross-check -- batch by batch into out_path. Returns read
        counts.

        Shards (shards.trim_file_sharded): byte_range = (begin, end) record starts of a plain file
        reads only that range; batch_filter(k) False skips batch k (parsed, not trimmed or
        written); segments, a list, receives (k, begin, end) byte spans of out_path per written batch;
        source, an iterable of (key, ReadBatch, albacore barcode), replaces reading in_path (the
        spooled chunks of shards.spool_batches; key is what segments record).

        Three stages overlap across batches: a reader thread parses the next batch, this thread
        runs the device work, a writer thread writes the previous batch (in file order). The
        library's parse, alignment and write calls release the GIL. times: 'parse' / 'write_wait'
        are this thread's waits, 'read' / 'write' the reader's / writer's own busy time (overlapped).

        With the quality stage on, counts['quality'] tallies its records: cropped_reads, cropped_bases,
        too_short, too_long, low_quality, no_qualities; with quality_per_piece also pieces, piece_cropped,
        piece_cropped_bases, piece_too_short, piece_too_long, piece_low_quality over the split reads' pieces."""
        counts = {'reads_in': 0, 'reads_kept': 0}
        quality = None
        if getattr(self, '_quality_on', lambda: False)():
            quality = counts['quality'] = {k: 0 for k in ('cropped_reads', 'cropped_bases', 'too_short', 'too_long', 'low_quality',
                                                         'no_qualities')}
            if getattr(self, 'quality_per_piece', False):
                quality.update({k: 0 for k in ('pieces', 'piece_cropped', 'piece_cropped_bases', 'piece_too_short', 'piece_too_long',
                                               'piece_low_quality')})
        # PCABI_PIPE_TRACE=1: (stage, batch, begin, end) per stage and batch in self.trace (the
        # pipeline's timeline: which stage holds the others up)
        trace = self.trace = [] if os.environ.get('PCABI_PIPE_TRACE') == '1' else None
        bins = {}                             # barcode name -> (path, reads selected for it)
        if self.barcode_dir is not None:
            os.makedirs(self.barcode_dir, exist_ok=True)
            counts['bins'] = bins
        # batches parsed ahead / trimmed and waiting for the writer (PCABI_PIPE_DEPTH, default 2)
        depth = max(1, int(os.environ.get('PCABI_PIPE_DEPTH', '2')))
        pq = queue.Queue(maxsize=depth)
        wq = queue.Queue(maxsize=depth)
        errors = []
        stop = threading.Event()          # set when this thread leaves: the reader stops putting

        def put_parsed(item):
            while not stop.is_set():
                try:
                    pq.put(item, timeout=0.05)
                    return True
                except queue.Full:
                    pass
            return False

        def batches():
            files = misc.input_files(in_path)
            if len(files) > 1 or files[0][1] is not None:
                if byte_range is not None:
                    raise ValueError('byte ranges apply to a single plain file, not to a directory')
            for f, alb in files:
                # batch sizes ramp up at the start and down at the end (misc.ramp_sizes): the first
                # parse and the last write are small, so they overlap the other stages
                keep = bool(getattr(self, 'keep_tags', False)) and (out_format == 'bam' or bool(getattr(self, 'header_tags', False)))
                for b in misc.read_batches(f, max_reads=max_reads, byte_range=byte_range, ramp=True,
                                           gunzip_device=getattr(self, 'gunzip_device', None), keep_aux=keep,
                                           gunzip_plain=bool(getattr(self, 'gunzip_plain', False)),
                                           tags_from_headers=keep and bool(getattr(self, 'tags_from_headers', False))):
                    yield b, alb
                if getattr(self, 'gunzip_plain', False):
                    # the reader thread's own figures (engine.gunzip_stream_stats is per thread)
                    from . import engine
                    self.gunzip_stream_stats = engine.gunzip_stream_stats()

        def produce():
            try:
                if getattr(self, 'gunzip_device', None) is not None:
                    check(self.L.pcabi_dev_set(self.device), 'pcabi_dev_set')   # this thread's own device
                items = iter(source if source is not None else
                             ((k, b, alb) for k, (b, alb) in enumerate(batches())))
                while True:
                    t0 = time.perf_counter()
                    item = next(items, None)
                    # the reader's own busy time (parse; overlapped like 'write')
                    t1 = time.perf_counter()
                    self.times['read'] = self.times.get('read', 0.0) + t1 - t0
                    if trace is not None:
                        trace.append(('read', item[0] if item is not None else -1, t0, t1))
                    if item is None:
                        break
                    k, b, alb = item
                    if batch_filter is not None and not batch_filter(k):
                        continue
                    if not put_parsed((k, b, alb)):
                        return
                put_parsed(None)
            except BaseException as ex:   # handed to the consumer
                put_parsed(ex)

        def consume_writes():
            first = True
            while True:
                item = wq.get()
                if item is None:
                    break
                if errors:
                    continue                 # drain after a failure
                k, b, st, et, co, cu, keep, calls = item
                t0 = time.perf_counter()
                try:
                    if calls is not None:
                        self._write_bins(b, out_format, st, et, co, cu, keep, calls, bins, k, segments)
                    else:
                        at = os.path.getsize(out_path) if (segments is not None and not first) else 0
                        misc.write_reads(b, out_path, out_format, st, et, None, self.min_split, self.discard_middle,
                                         select=keep, append=not first, cut_arrays=(co, cu),
                                         gzip_device=getattr(self, 'gzip_device', None),
                                         bgzf=_bgzf_mode(self, out_format), **_bam_kw(self, out_format, b))
                        if segments is not None:
                            segments.append((k, at, os.path.getsize(out_path)))
                except BaseException as ex:
                    errors.append(ex)
                first = False
                counts['reads_in'] += b.n
                counts['reads_kept'] += int(keep.sum()) if keep is not None else b.n
                t1 = time.perf_counter()
                self.times['write'] = self.times.get('write', 0.0) + t1 - t0
                if trace is not None:
                    trace.append(('write', k, t0, t1))
            if first and not errors and self.barcode_dir is None:   # empty input: still create the output
                if out_format == 'bam':
                    misc.write_bam_header(out_path)
                else:
                    open(out_path, 'wb').close()

        reader = threading.Thread(target=produce, daemon=True)
        writer = threading.Thread(target=consume_writes, daemon=True)
        reader.start()
        writer.start()
        t = time.perf_counter()
        try:
            while not errors:                # a failed write stops the run at the next batch
                b = pq.get()
                t = self._tick('parse', t)   # waiting for a parsed batch
                if b is None:
                    break
                if isinstance(b, BaseException):
                    raise b
                k, b, alb = b
                t0 = t
                st, et, co, cu, _, keep = self.trim(b) if alb is None else self.trim(b, albacore=alb)
                calls = self.last_calls if self.barcode_dir is not None else None
                if quality is not None:
                    q = self.last_quality
                    crop = q['front'].astype(np.int64) + q['tail']
                    quality['cropped_reads'] += int((crop > 0).sum())
                    quality['cropped_bases'] += int(crop.sum())
                    for key, bit in (('too_short', QUAL_TOO_SHORT), ('too_long', QUAL_TOO_LONG), ('low_quality', QUAL_LOW_QUALITY),
                                     ('no_qualities', QUAL_NO_QUALITIES)):
                        quality[key] += int(((q['flags'] & bit) != 0).sum())
                    if self.last_quality_pieces is not None:
                        q = self.last_quality_pieces['q']
                        crop = q['front'].astype(np.int64) + q['tail']
                        quality['pieces'] += int(q.size)
                        quality['piece_cropped'] += int((crop > 0).sum())
                        quality['piece_cropped_bases'] += int(crop.sum())
                        for key, bit in (('piece_too_short', QUAL_TOO_SHORT), ('piece_too_long', QUAL_TOO_LONG),
                                         ('piece_low_quality', QUAL_LOW_QUALITY)):
                            quality[key] += int(((q['flags'] & bit) != 0).sum())
                t1 = time.perf_counter()
                wq.put((k, b, st, et, co, cu, keep, calls))   # the writer drains even after a failure
                del b
                t = time.perf_counter()
                self.times['put_wait'] = self.times.get('put_wait', 0.0) + t - t1
                if trace is not None:
                    trace.append(('trim', k, t0, t1))
                    trace.append(('put', k, t1, t))
        finally:
            # on every exit (errors included) the reader's pending put times out on `stop`, so
            # joining it cannot block on a full queue
            stop.set()
            wq.put(None)
            writer.join()
            reader.join()
        self._tick('write_wait', t)
        if errors:
            raise errors[0]
        if _finish_mode(self, out_format):
            for path in [out_path] + [p for p, _ in bins.values()]:
                if os.path.isfile(path):
                    misc.bgzf_finish(path)
        return counts

    def _write_bins(self, b, out_format, st, et, co, cu, keep, calls, bins, k=0, segments=None):
        """One batch into the barcode bins (porechop_abi.py:581-610): the reads of each call, in
        read order, appended to <barcode_dir>/<name>.<format> (created, not appended, the first
        time the run writes it, as the reference opens each bin with 'wt'). segments (sharded
        runs) receives (k, name, begin, end) byte spans per bin write. As in the reference
        (porechop_abi.py:598-604) a bin exists only once some read of it produced output, and it
        counts only those reads: a write that emitted nothing leaves no file and no span."""
        sel = np.ones(b.n, bool) if keep is None else keep.astype(bool)
        if self.discard_unassigned:
            sel &= calls >= 0
        for cid in np.unique(calls[sel]).tolist():
            name = self.bc_names.get(cid, 'none') if cid >= 0 else 'none'
            mask = (sel & (calls == cid)).astype(np.uint8)
            path = os.path.join(self.barcode_dir, name + '.' + out_format)
            fresh = name not in bins
            at = 0 if fresh else os.path.getsize(path)
            emitted = misc.write_reads(b, path, out_format, st, et, None, self.min_split, self.discard_middle,
                                       untrimmed=self.untrimmed, select=mask, append=not fresh, cut_arrays=(co, cu),
                                       gzip_device=getattr(self, 'gzip_device', None),
                                       bgzf=_bgzf_mode(self, out_format), **_bam_kw(self, out_format, b))
            if emitted == 0:
                if fresh and os.path.exists(path):
                    os.remove(path)             # the reference never opens an empty bin
                continue
            bins[name] = (path, (0 if fresh else bins[name][1]) + emitted)
            if segments is not None:
                segments.append((k, name, at, os.path.getsize(path)))

    def close(self):
        L = self.L
        for p, _ in self.dev.values():
            L.pcabi_dev_free(p)
        self.dev = {}
        if self.scan:
            L.pcabi_scan_destroy(self.scan)
            self.scan = VP()
        for t in self.tabs:
            if t:
                L.pcabi_adapters_destroy(t)
        self.tabs = []
        if self.stream:
            L.pcabi_stream_destroy(self.stream)
            self.stream = VP()
