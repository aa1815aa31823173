// pcabi_qual.h -- the quality stage's rule: a read's span cropped at both ends to its outermost windows of
// acceptable quality, then its length and mean-quality tests (pcabi_qual.hip; include/pcabi.h pcabi_qual_*;
// DESIGN.md "Quality stage"). Nothing here is device-only: the kernels and the host build (device < 0) run
// the same code.
//
// A quality byte c is Phred q = clamp(c - 33, 0, 93). The span of a read is n bytes of the quality blob
// from `off` on; off < 0 names a read without qualities, which is never cropped and passes the quality
// test. With S(p) the sum of q over [p, p + W) and f / g the least / greatest p in [0, n - W] with
// S(p) >= min_window_sum, the kept span is [f, g + W): front = f, tail = n - (g + W); without such a
// window (or n < W) front = n, tail = 0, kept = 0. W == 0 keeps the span. Over the kept span q_sum is the
// sum of q and err_sum the sum of E[q] = round(2^32 * 10^(-q / 10)), the error probability in units of
// 2^-32. Equality passes: a window sum equal to min_window_sum qualifies, err_sum equal to kept *
// max_mean_err is not LOW_QUALITY.
//
// The kept spans are cut into segments of kSeg bytes, laid out flat (seg_off[read], an exclusive scan of
// n_segs(kept) on the device). A lane takes 16 bytes at a time at 16-aligned offsets of the blob
// (sum_lane); a load that sticks out of the segment goes byte by byte over the part inside, so no byte
// outside [off + f, off + g + W) is read.
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

namespace pcabi_qual {

constexpr int64_t kSeg = 4096;                      // quality bytes a segment
constexpr int kMaxWindow = 64;                      // one window start a lane
constexpr int kMaxQ = 93;
constexpr int64_t kMaxBlob = (int64_t)1 << 31;      // bytes a batch may hold
constexpr uint64_t kErrOne = (uint64_t)1 << 32;     // error probability 1: max_mean_err's "off"
constexpr int32_t kFail = PCABI_QUAL_TOO_SHORT | PCABI_QUAL_TOO_LONG | PCABI_QUAL_LOW_QUALITY;   // a read, or a piece, fails

// E[q] = round(2^32 * 10^(-q / 10)), q = 0..93 (tests/qual_ref.py recomputes it)
#define PCABI_QUAL_ERR_TABLE                                                                                        \
    4294967296ull, 3411613790ull, 2709941160ull, 2152582778ull, 1709857278ull, 1358187913ull, 1078847007ull,        \
        856958639ull, 680706443ull, 540704347ull, 429496730ull, 341161379ull, 270994116ull, 215258278ull,           \
        170985728ull, 135818791ull, 107884701ull, 85695864ull, 68070644ull, 54070435ull, 42949673ull, 34116138ull,  \
        27099412ull, 21525828ull, 17098573ull, 13581879ull, 10788470ull, 8569586ull, 6807064ull, 5407043ull,        \
        4294967ull, 3411614ull, 2709941ull, 2152583ull, 1709857ull, 1358188ull, 1078847ull, 856959ull, 680706ull,   \
        540704ull, 429497ull, 341161ull, 270994ull, 215258ull, 170986ull, 135819ull, 107885ull, 85696ull, 68071ull, \
        54070ull, 42950ull, 34116ull, 27099ull, 21526ull, 17099ull, 13582ull, 10788ull, 8570ull, 6807ull, 5407ull,  \
        4295ull, 3412ull, 2710ull, 2153ull, 1710ull, 1358ull, 1079ull, 857ull, 681ull, 541ull, 429ull, 341ull,      \
        271ull, 215ull, 171ull, 136ull, 108ull, 86ull, 68ull, 54ull, 43ull, 34ull, 27ull, 22ull, 17ull, 14ull,      \
        11ull, 9ull, 7ull, 5ull, 4ull, 3ull, 3ull, 2ull

PCABI_HD inline uint64_t err_of(int q) {
    static constexpr uint64_t kErr[kMaxQ + 1] = {PCABI_QUAL_ERR_TABLE};
    return kErr[q];
}

PCABI_HD inline int phred(uint8_t c) { return c < 33 ? 0 : c > 126 ? kMaxQ : (int)c - 33; }

PCABI_HD inline bool opts_ok(const pcabi_qual_opts &o) {
    return o.window >= 0 && o.window <= kMaxWindow && o.max_mean_err <= kErrOne;
}
// a span against the blob: off < 0 is a read without qualities and touches nothing
PCABI_HD inline bool span_fits(int64_t off, int64_t n, int64_t qual_n) { return n >= 0 && (off < 0 || (off <= qual_n && n <= qual_n - off)); }
PCABI_HD inline bool crop_on(const pcabi_qual_opts &o, int64_t off) { return o.window > 0 && off >= 0; }

// The crop's scans run over "steps": step j from the front is byte j of the span, from the tail byte
// n - 1 - j, so that one rule serves both ends. The window that starts at step v covers the steps
// [v, v + W) and exists when v <= n - W.
PCABI_HD inline int64_t step_pos(int64_t n, bool from_tail, int64_t j) { return from_tail ? n - 1 - j : j; }

// The first step v in [0, n - W] whose window sums to min_sum or more, or -1: the host build's sliding
// window (the kernel takes 64 steps a pass, pcabi_qual.hip scan_wave).
inline int64_t scan_host(const uint8_t *q, int64_t n, int W, int64_t min_sum, bool from_tail) {
    if (n < W) return -1;
    int64_t s = 0;
    for (int64_t j = 0; j < W; ++j) s += phred(q[step_pos(n, from_tail, j)]);
    for (int64_t v = 0;; ++v) {
        if (s >= min_sum) return v;
        if (v + W >= n) return -1;
        s += phred(q[step_pos(n, from_tail, v + W)]) - phred(q[step_pos(n, from_tail, v)]);
    }
}

// front, tail and kept from the two scans' first steps (vf < 0: no window qualifies)
PCABI_HD inline void crop_of(int64_t n, int64_t vf, int64_t vt, pcabi_qual_read *r) {
    r->front = (int32_t)(vf < 0 ? n : vf);
    r->tail = (int32_t)(vf < 0 ? 0 : vt);
    r->kept = (int32_t)(n - r->front - r->tail);
}

PCABI_HD inline int64_t n_segs(int64_t kept) { return (kept + kSeg - 1) / kSeg; }

// One lane's share of the bytes q[a, e): the loads at the 16-aligned offsets a & ~15, + 16, ... are dealt
// to the lanes in turn; err: E[] (the kernel's copy in LDS, the host's table).
template <class Err>
PCABI_HD inline void sum_lane(const uint8_t *q, int64_t a, int64_t e, int lane, int n_lanes, const Err &err, int64_t *q_sum, uint64_t *err_sum) {
    for (int64_t pos = (a & ~(int64_t)15) + 16 * (int64_t)lane; pos < e; pos += 16 * (int64_t)n_lanes) {
        if (pos >= a && pos + 16 <= e) {
            uint8_t v[16];
            if (((uintptr_t)(q + pos) & 15u) == 0) memcpy(v, __builtin_assume_aligned(q + pos, 16), 16);
            else memcpy(v, q + pos, 16);
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int p = phred(v[k]);
                *q_sum += p;
                *err_sum += err(p);
            }
            continue;
        }
        const int64_t lo = pos > a ? pos : a, hi = pos + 16 < e ? pos + 16 : e;
        for (int64_t k = lo; k < hi; ++k) {
            const int p = phred(q[k]);
            *q_sum += p;
            *err_sum += err(p);
        }
    }
}

// the flags of a read from its kept length and sums
PCABI_HD inline int32_t flags_of(const pcabi_qual_opts &o, bool has_qual, int64_t kept, uint64_t err_sum) {
    int32_t f = has_qual ? 0 : PCABI_QUAL_NO_QUALITIES;
    if (kept < o.min_length) f |= PCABI_QUAL_TOO_SHORT;
    if (o.max_length > 0 && kept > o.max_length) f |= PCABI_QUAL_TOO_LONG;
    if (has_qual && err_sum > (uint64_t)kept * o.max_mean_err) f |= PCABI_QUAL_LOW_QUALITY;
    return f;
}

}  // namespace pcabi_qual
