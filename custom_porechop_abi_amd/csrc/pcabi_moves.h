// pcabi_moves.h -- the basecaller's move table (mv) and its sample offset (ts) remapped onto parts of a
// read: the usability checks, the slice rule and the byte emitters (pcabi_moves.hip, pcabi_write.cpp;
// include/pcabi.h pcabi_moves_*; DESIGN.md "BAM output"). Nothing here is device-only: the kernels, the
// host build (device < 0) and the CPU tests (tests/moves_fuzz_main.cpp builds it alone) run the same code.
//
// mv is a B:c (or B:C) array: the stride S, then n moves of 0 or 1, one per S samples; a 1 starts a base.
// With p(k) the index of the k-th 1 (from 0) and p(ones) = n, a part [s0, s0 + ns) of the read takes the
// moves [q0, q1): q0 = 0 when s0 == 0, else p(s0); q1 = p(s0 + ns). It is written as `mv B c`, the count
// 1 + q1 - q0, S, the slice byte for byte, and then, when the read had a ts tag, `ts i` with ts + S * q0.
//
// The moves of all reads are cut into segments of kSeg moves, laid out flat (seg_off[read] is a read's
// first). Counting: a lane takes 16 bytes at a time at 16-aligned offsets of the tag blob; bytes of the
// load outside the segment read as 0 (load16), a dword is valid when (w & 0xFEFEFEFE) == 0 and then holds
// popcount(w) ones. An exclusive scan of `count + (invalid ? kBadUnit : 0)` over the flat array gives, per
// read, ones and the number of invalid segments at once (read_sums). Selecting the k-th one: select_seg
// finds the segment whose prefix range holds k (segments without a one fall out of the search), then the
// segment goes by 64 bytes a pass, one a lane: the ballot of `byte == 1` and is_kth() name the lane.
#pragma once
#include <cstdint>
#include <cstring>

#include "../../include/pcabi.h"

#ifndef PCABI_HD
#if defined(__HIPCC__)
#define PCABI_HD __host__ __device__
#else
#define PCABI_HD
#endif
#endif

namespace pcabi_moves {

constexpr int64_t kSeg = 4096;                  // moves a segment
constexpr int64_t kChunk = 4096;                // output bytes a workgroup of k_moves_write copies
constexpr int64_t kHead = 9;                    // 'm' 'v' 'B' 'c', the count, the stride
constexpr int64_t kTsLen = 7;                   // 't' 's' 'i', the value
constexpr int64_t kBadUnit = (int64_t)1 << 40;  // an invalid segment in the scanned sums (above every count)
constexpr int64_t kMaxVals = INT32_MAX - 64;    // values a table may hold: its parts' lengths stay int32

PCABI_HD inline int64_t n_moves(const pcabi_moves_read &r) { return r.n_vals > 0 ? (int64_t)r.n_vals - 1 : 0; }
PCABI_HD inline int64_t n_segs(const pcabi_moves_read &r) { return (n_moves(r) + kSeg - 1) / kSeg; }
// the first move in the tag blob (the stride lies one byte before it)
PCABI_HD inline int64_t moves_at(const pcabi_moves_read &r) { return r.mv_off + 1; }

PCABI_HD inline bool read_fits(const pcabi_moves_read &r, int64_t tags_n, int64_t n_parts) {
    if (r.l_seq < 0 || r.n_vals < 0 || r.n_vals > kMaxVals || r.n_parts < 0 || r.part0 < 0 || r.mv_off < 0) return false;
    if (r.mv_off > tags_n || r.n_vals > tags_n - r.mv_off) return false;
    return r.part0 <= n_parts && r.n_parts <= n_parts - r.part0;
}

PCABI_HD inline bool dword_ok(uint32_t w) { return (w & 0xFEFEFEFEu) == 0; }
PCABI_HD inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// The 16 bytes tags[pos, pos + 16) as four dwords, with every byte outside [a, e) read as 0 and never
// touched: a load that lies inside [a, e) is one 16-byte load, any other goes byte by byte.
PCABI_HD inline void load16(const uint8_t *tags, int64_t pos, int64_t a, int64_t e, uint32_t w[4]) {
    if (pos >= a && pos + 16 <= e) {
        if (aligned16(tags + pos)) memcpy(w, __builtin_assume_aligned(tags + pos, 16), 16);
        else memcpy(w, tags + pos, 16);
        return;
    }
    w[0] = w[1] = w[2] = w[3] = 0;
    const int64_t lo = pos > a ? pos : a, hi = pos + 16 < e ? pos + 16 : e;
    for (int64_t k = lo; k < hi; ++k) w[(k - pos) >> 2] |= (uint32_t)tags[k] << (8 * ((k - pos) & 3));
}

PCABI_HD inline int popc32(uint32_t w) { return __builtin_popcount(w); }
PCABI_HD inline int popc64(uint64_t w) { return __builtin_popcountll(w); }

// One lane's share of the moves tags[a, e): the loads at the 16-aligned offsets a & ~15, + 16, ... are
// dealt to the lanes in turn. Adds the ones of its valid dwords to *ones; returns false when a dword of
// its share is not valid.
PCABI_HD inline bool count_lane(const uint8_t *tags, int64_t a, int64_t e, int lane, int n_lanes, int64_t *ones) {
    bool ok = true;
    for (int64_t pos = (a & ~(int64_t)15) + 16 * (int64_t)lane; pos < e; pos += 16 * (int64_t)n_lanes) {
        uint32_t w[4];
        load16(tags, pos, a, e, w);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ok = ok && dword_ok(w[k]);
            *ones += popc32(w[k]);
        }
    }
    return ok;
}
// what a segment adds to the scanned array
PCABI_HD inline int64_t seg_value(int64_t ones, bool ok) { return ok ? ones : ones + kBadUnit; }

// ones and invalid segments of a read from the scan's values at its first segment and behind its last
PCABI_HD inline void read_sums(int64_t pre0, int64_t pre1, int64_t *ones, int64_t *n_bad) {
    const int64_t d = pre1 - pre0;
    *ones = d & (kBadUnit - 1);
    *n_bad = d >> 40;
}

// The segment of a read that holds its k-th one: the first s in [0, n_seg) with ones(segments 0..s) > k,
// from pre[0, n_seg] (the scan's values from the read's first segment on); n_seg when the read has no
// more than k ones. *before = the ones ahead of that segment.
PCABI_HD inline int64_t select_seg(const int64_t *pre, int64_t n_seg, int64_t k, int64_t *before) {
    const int64_t base = pre[0];
    int64_t lo = 0, hi = n_seg;   // the answer lies in [lo, hi]
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (((pre[mid + 1] - base) & (kBadUnit - 1)) > k) hi = mid;
        else lo = mid + 1;
    }
    *before = lo < n_seg ? (pre[lo] - base) & (kBadUnit - 1) : 0;
    return lo;
}

// in a ballot of `byte == 1`: is `lane` the bit that is the r-th set one (from 0)?
PCABI_HD inline bool is_kth(uint64_t mask, int lane, int64_t r) {
    return ((mask >> lane) & 1) != 0 && popc64(mask & (((uint64_t)1 << lane) - 1)) == r;
}

// The byte-by-byte walk of one segment tags[a, e): the offset from a of its r-th 1, or -1.
PCABI_HD inline int64_t select_walk(const uint8_t *tags, int64_t a, int64_t e, int64_t r) {
    for (int64_t k = a; k < e; ++k)
        if (tags[k] == 1 && r-- == 0) return k - a;
    return -1;
}

// a part's boundaries in bases, and which k of p(k) each asks for (-1: the part starts the read, q0 = 0)
PCABI_HD inline int64_t edge_k(const pcabi_moves_part &p, int side) {
    if (side == 0) return p.s0 == 0 ? -1 : (int64_t)p.s0;
    return (int64_t)p.s0 + p.ns;
}

PCABI_HD inline int stride_of(const uint8_t *tags, const pcabi_moves_read &r) { return r.n_vals >= 1 ? (int)tags[r.mv_off] : 0; }

// usable, but for what the parts' q0 decide (ts_fits)
PCABI_HD inline bool table_usable(const pcabi_moves_read &r, int stride, int64_t ones, int64_t n_bad) {
    return !(r.flags & PCABI_MOVES_BAD) && r.n_vals >= 1 && stride >= 1 && stride <= 127 && n_bad == 0 && ones == r.l_seq;
}
PCABI_HD inline int64_t ts_of(const pcabi_moves_read &r, int stride, int64_t q0) { return (int64_t)r.ts + (int64_t)stride * q0; }
PCABI_HD inline bool ts_fits(const pcabi_moves_read &r, int stride, int64_t q0) { return r.ts < 0 || ts_of(r, stride, q0) <= INT32_MAX; }
PCABI_HD inline int64_t tag_len(const pcabi_moves_read &r, int64_t q0, int64_t q1) {
    return kHead + (q1 - q0) + (r.ts >= 0 ? kTsLen : 0);
}

// Byte j of a part's tag bytes outside its slice: j < kHead (the head and the stride) or j >= kHead + m
// (the ts tag), m = q1 - q0.
PCABI_HD inline uint8_t fixed_byte(int64_t j, int64_t m, int stride, int64_t ts_new) {
    if (j < 4) return (uint8_t)("mvBc"[j]);
    if (j < 8) return (uint8_t)((uint64_t)(1 + m) >> (8 * (j - 4)));
    if (j == 8) return (uint8_t)stride;
    const int64_t t = j - kHead - m;
    if (t < 3) return (uint8_t)("tsi"[t]);
    return (uint8_t)((uint64_t)ts_new >> (8 * (t - 3)));
}

// One lane's share of the bytes [j0, j1) of a part's tag bytes, written to dst (the part's first byte):
// the fixed bytes one by one; the slice src[0, m) -> dst[kHead, kHead + m) byte-wise up to the first
// 16-aligned destination, then in 16-byte pieces dealt to the lanes in turn (source and destination are
// mutually unaligned: an unaligned load, an aligned store), then byte-wise again.
PCABI_HD inline void copy_lane(uint8_t *dst, const uint8_t *src, int64_t m, int stride, int64_t ts_new, int64_t len, int64_t j0,
                               int64_t j1, int lane, int n_lanes) {
    if (j1 > len) j1 = len;
    const int64_t c0 = j0 > kHead ? j0 : kHead, c1 = j1 < kHead + m ? j1 : kHead + m;   // the slice's share of [j0, j1)
    for (int64_t j = j0 + lane; j < j1; j += n_lanes)
        if (j < kHead || j >= kHead + m) dst[j] = fixed_byte(j, m, stride, ts_new);
    if (c0 >= c1) return;
    int64_t head = (int64_t)((16 - ((uintptr_t)(dst + c0) & 15u)) & 15u);
    if (head > c1 - c0) head = c1 - c0;
    const int64_t body = (c1 - c0 - head) / 16;
    for (int64_t j = c0 + lane; j < c0 + head; j += n_lanes) dst[j] = src[j - kHead];
    for (int64_t k = lane; k < body; k += n_lanes) {
        uint8_t v[16];
        const int64_t j = c0 + head + 16 * k;
        memcpy(v, src + (j - kHead), 16);
        memcpy(__builtin_assume_aligned(dst + j, 16), v, 16);
    }
    for (int64_t j = c0 + head + 16 * body + lane; j < c1; j += n_lanes) dst[j] = src[j - kHead];
}

}  // namespace pcabi_moves
