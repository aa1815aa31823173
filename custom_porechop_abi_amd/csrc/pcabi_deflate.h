// pcabi_deflate.h -- the parts of the gzip encoder (pcabi_deflate.hip) that hold no device code:
// the length-limited Huffman code construction, the code-length-code (dynamic block header) plan
// and the writer's block planner. Everything here compiles as plain C++ too (tests/deflate_cpu.cpp
// builds a helper from it), so the code the kernel runs is checkable without a GPU.
//
// Format (RFC 1951): every input block becomes one deflate block of literals + end-of-block, no
// matches. A dynamic block's literal/length code has 257 lengths (HLIT = 0) limited to 15 bits and
// complete; HDIST = 0 (one distance code) with the single length 1 that RFC 1951 3.2.7 prescribes
// for "only one distance code"; the code-length code is limited to 7 bits and complete; the 258
// lengths are sent one by one (no 16 / 17 / 18 runs).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define PCABI_HD __host__ __device__
#else
#define PCABI_HD
#endif

namespace pcabi_deflate {

constexpr int kLitSyms = 257;        // 256 literals + end-of-block
constexpr int kMaxLitBits = 15;
constexpr int kClSyms = 19;
constexpr int kMaxClBits = 7;
constexpr int kBlockCap = 65535;     // one stored block holds any input block
constexpr int kDefaultBlock = 32768; // fixed block length when the caller gives no list
constexpr int kLongLine = 1024;      // the writer never lets a block span the end of a line this long
constexpr int kHdrWords = 60;        // 17 + 19 * 3 + 258 * 7 = 1880 bits at the most
constexpr int kStoredOverhead = 5;   // 00, LEN, NLEN
constexpr int kSyncBytes = 4;        // 00 00 FF FF after the 3 header bits + padding of the empty stored block
constexpr int kMemberOverhead = 20;  // 10 header + 2 final empty fixed block + 8 trailer

// scratch of one construction: internal-node weights, parents (leaves 0..n-1, internal n..2n-2), depths
struct HcWork {
    uint32_t w[kLitSyms];
    uint16_t parent[2 * kLitSyms];
    uint16_t depth[kLitSyms];
};

// The used symbols (cnt > 0) ascending by (count, symbol). Returns how many.
PCABI_HD inline int hc_sort(const uint32_t *cnt, int nsym, uint16_t *order) {
    int n = 0;
    for (int s = 0; s < nsym; ++s) {
        if (!cnt[s]) continue;
        int k = n++;
        while (k > 0 && cnt[order[k - 1]] > cnt[s]) {
            order[k] = order[k - 1];
            --k;
        }
        order[k] = (uint16_t)s;
    }
    return n;
}

// Code lengths of the n used symbols order[0..n) (ascending by count): Huffman's algorithm with two
// queues, depths clamped to maxbits, the Kraft sum repaired the way zlib's gen_bitlen does it (a leaf
// of the deepest level below maxbits that has one moves down and takes an overflowing leaf as sibling),
// lengths handed out longest-first to the rarest symbols. bl_count[l] = codes of length l. len[] is
// written for the used symbols only. The result is complete (Kraft sum 1) for n >= 2; n == 1 gives
// the single length 1.
PCABI_HD inline void hc_lengths_sorted(const uint16_t *order, int n, const uint32_t *cnt, int maxbits,
                                       uint8_t *len, uint16_t *bl_count, HcWork &wk) {
    for (int b = 0; b <= kMaxLitBits; ++b) bl_count[b] = 0;
    if (n <= 0) return;
    if (n == 1) {
        len[order[0]] = 1;
        bl_count[1] = 1;
        return;
    }
    int li = 0, ii = 0, ni = 0;
    for (int k = 0; k < n - 1; ++k) {
        uint32_t sum = 0;
        for (int pick = 0; pick < 2; ++pick) {
            int node;
            if (li < n && (ii >= ni || cnt[order[li]] <= wk.w[ii])) {
                sum += cnt[order[li]];
                node = li++;
            } else {
                sum += wk.w[ii];
                node = n + ii++;
            }
            wk.parent[node] = (uint16_t)(n + ni);
        }
        wk.w[ni++] = sum;
    }
    // depths clamped on the way down, every clamped node (internal ones too) counted: gen_bitlen's
    // bookkeeping, which its repair loop below relies on
    int overflow = 0;
    wk.depth[n - 2] = 0;
    for (int i = n - 3; i >= 0; --i) {
        int d = wk.depth[wk.parent[n + i] - n] + 1;
        if (d > maxbits) {
            d = maxbits;
            ++overflow;
        }
        wk.depth[i] = (uint16_t)d;
    }
    for (int l = 0; l < n; ++l) {
        int d = wk.depth[wk.parent[l] - n] + 1;
        if (d > maxbits) {
            d = maxbits;
            ++overflow;
        }
        ++bl_count[d];
    }
    while (overflow > 0) {
        int bits = maxbits - 1;
        while (bl_count[bits] == 0) --bits;
        --bl_count[bits];
        bl_count[bits + 1] = (uint16_t)(bl_count[bits + 1] + 2);
        --bl_count[maxbits];
        overflow -= 2;
    }
    int k = 0;
    for (int bits = maxbits; bits >= 1; --bits)
        for (int c = 0; c < bl_count[bits]; ++c) len[order[k++]] = (uint8_t)bits;
}

PCABI_HD inline uint32_t hc_rev(uint32_t code, int len) {
    uint32_t r = 0;
    for (int i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
    return r;
}

// first canonical code of every length (RFC 1951 3.2.2)
PCABI_HD inline void hc_next_code(const uint16_t *bl_count, int maxbits, uint16_t *next_code) {
    uint32_t code = 0;
    next_code[0] = 0;
    for (int b = 1; b <= maxbits; ++b) {
        code = (code + (b > 1 ? bl_count[b - 1] : 0)) << 1;
        next_code[b] = (uint16_t)code;
    }
}

// canonical codes of every symbol, bit-reversed for the LSB-first stream (serial form)
PCABI_HD inline void hc_codes(const uint8_t *len, int nsym, const uint16_t *bl_count, int maxbits, uint16_t *code) {
    uint16_t next[kMaxLitBits + 1];
    hc_next_code(bl_count, maxbits, next);
    for (int s = 0; s < nsym; ++s) code[s] = len[s] ? (uint16_t)hc_rev(next[len[s]]++, len[s]) : 0;
}

// order in which the code-length-code lengths are sent
PCABI_HD inline int hc_cl_order(int i) {
    const uint8_t o[kClSyms] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return o[i];
}

// The code-length code from the histogram of the 258 lengths sent (257 literal/length + the one
// distance length 1): cl_len / cl_code (reversed) per symbol 0..18, *hclen4 = how many of the 19
// lengths are sent (4..19). Returns the bits before the 258 coded lengths: 3 + 5 + 5 + 4 + 3 * *hclen4.
PCABI_HD inline int hc_cl_plan(const uint32_t *clcnt, uint8_t *cl_len, uint16_t *cl_code, int *hclen4, HcWork &wk) {
    uint16_t order[kClSyms], blc[kMaxLitBits + 1];
    for (int s = 0; s < kClSyms; ++s) cl_len[s] = 0;
    const int n = hc_sort(clcnt, kClSyms, order);
    hc_lengths_sorted(order, n, clcnt, kMaxClBits, cl_len, blc, wk);
    hc_codes(cl_len, kClSyms, blc, kMaxClBits, cl_code);
    int h = kClSyms;
    while (h > 4 && cl_len[hc_cl_order(h - 1)] == 0) --h;
    *hclen4 = h;
    return 17 + 3 * h;
}

// Everything about one block from its literal histogram (cnt[256] is set to 1 here), serially: the
// literal/length lengths, the code-length code, the header's bit count and the whole dynamic
// block's (header + data + end-of-block). The kernel computes the same figures with the sort, the
// sums and the code assignment spread over a workgroup.
PCABI_HD inline void hc_plan_block(uint32_t *cnt, uint8_t *lit_len, uint8_t *cl_len, uint16_t *cl_code, int *hclen4,
                                   uint32_t *hdr_bits, uint32_t *block_bits, HcWork &wk) {
    uint16_t order[kLitSyms], blc[kMaxLitBits + 1];
    cnt[256] = 1;
    for (int s = 0; s < kLitSyms; ++s) lit_len[s] = 0;
    const int n = hc_sort(cnt, kLitSyms, order);
    hc_lengths_sorted(order, n, cnt, kMaxLitBits, lit_len, blc, wk);
    uint32_t clcnt[kClSyms] = {0};
    for (int s = 0; s < kLitSyms; ++s) ++clcnt[lit_len[s]];
    ++clcnt[1];   // the distance code's single length
    uint32_t bits = (uint32_t)hc_cl_plan(clcnt, cl_len, cl_code, hclen4, wk);
    for (int s = 0; s < kLitSyms; ++s) bits += cl_len[lit_len[s]];
    bits += cl_len[1];
    *hdr_bits = bits;
    for (int s = 0; s < kLitSyms; ++s) bits += cnt[s] * lit_len[s];
    *block_bits = bits;
}

// bytes of a block in its two forms, given the dynamic form's bits (header + data + end-of-block):
// the dynamic block is followed by the 3 header bits of an empty stored block, padding and 00 00 FF FF
PCABI_HD inline uint32_t dyn_bytes(uint32_t block_bits) { return (block_bits + 3 + 7) / 8 + kSyncBytes; }
PCABI_HD inline uint32_t stored_bytes(uint32_t n) { return n + kStoredOverhead; }

// ---- the writer's block planner (host) -------------------------------------------------------
// Cuts text[lo, hi) (lo at a line start) into blocks of 1..cap bytes; emit(end) receives every
// block's end, ascending, the last one hi. A line counts with its '\n'. A line of long_line bytes or
// more ends a block: it forms one with the short lines pending before it (headers, "+"), cut evenly
// into ceil(bytes / cap) pieces when that is more than cap bytes. Short lines accumulate up to cap.
// So no block spans the end of a long line, and short lines never pay for a block of their own
// next to a long one. long_line <= cap.
template <class Emit>
inline void plan_blocks(const char *text, int64_t lo, int64_t hi, int64_t long_line, int64_t cap, Emit emit) {
    int64_t bs = lo, p = lo;
    while (p < hi) {
        const void *nl = memchr(text + p, '\n', (size_t)(hi - p));
        const int64_t e = nl ? (int64_t)((const char *)nl - text) + 1 : hi;
        if (e - p >= long_line) {
            const int64_t span = e - bs, k = (span + cap - 1) / cap;
            for (int64_t j = 1; j <= k; ++j) emit(bs + span * j / k);
            bs = e;
        } else if (e - bs > cap) {
            emit(p);
            bs = p;
        }
        p = e;
    }
    if (bs < hi) emit(hi);
}

}  // namespace pcabi_deflate
