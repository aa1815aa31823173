// pcabi_kmer.h -- the arithmetic of the ab-initio k-mer counts (pcabi_kmer.hip; include/pcabi.h
// pcabi_kmer_*; DESIGN.md "k-mer counts"). Nothing here is device-only: the kernels and the tests' host
// model (tests/native/kmer_model.cpp) run the same code.
//
// A k-mer (2 <= k <= 32) is its 2-bit value, first base in the top bits (dna2int,
// approx_counter.cpp:55-62). A window of k Dna5 codes (0..3, 4 = N) has a key unless it holds an N, is
// low-complexity or is forbidden: window_key says which. A position without a key is stored as kSkip. Below
// k = 32 kSkip has bits above the 2k a key uses; at k = 32 it is also the value of the 32-mer TTT...T, so
// whoever stores kSkip there has to count how often (pcabi_kmer.hip subtracts that count from the last
// run).
//
// The approximate count needs, for a k-mer and a sequence, the least edit distance between the k-mer and
// any substring: Myers' bit-vector algorithm (1999) with D[0][j] = 0 (free text start). The state is the
// vertical deltas of one column (pv / mv, pattern base i at bit i) and the score D[k][j]; best_distance is
// the minimum of the score over the columns, k for an empty sequence. Sequences lie at 4-aligned offsets
// and are read a dword (four codes, first in the low byte) at a time; of the last dword only the
// n - j0 codes that belong to the sequence count, whatever the bytes behind them hold.
#pragma once
#include <cstdint>

#ifndef PCABI_HD
#if defined(__HIPCC__)
#define PCABI_HD __host__ __device__
#else
#define PCABI_HD
#endif
#endif

namespace pcabi_kmer {

constexpr uint64_t kSkip = ~0ull;
constexpr int kSeqPerBlock = 32;   // sequences a block of k_kmer_approx walks

// haveLowComplexity (approx_counter.cpp:214-234): counts[16] of the k-1 dimers, sum of
// v (v - 1) over them == twice the number of equal dimer pairs; s = sum / float(2 (k - 2)).
// At k = 2 s is 0 / 0: the compare is false, as in the reference, and no 2-mer is low-complexity.
PCABI_HD inline bool low_complexity(uint64_t kmer, int k, float thr) {
    uint32_t pairs = 0;
    for (int i = 0; i < k - 1; ++i) {
        const uint32_t a = (uint32_t)(kmer >> (2 * i)) & 15u;
        for (int j = i + 1; j < k - 1; ++j) pairs += ((uint32_t)(kmer >> (2 * j)) & 15u) == a;
    }
    const float s = (float)(2u * pairs) / (float)(2 * (k - 2));
    return s >= thr;
}

// isForbiddenKmer (:330-332): a lookup in the sorted set
PCABI_HD inline bool forbidden(uint64_t v, const uint64_t *forb, int64_t n_forb) {
    int64_t lo = 0, hi = n_forb;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (forb[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo < n_forb && forb[lo] == v;
}

// The window c[0 .. k): true and its key, or false (an N, low-complexity, forbidden).
PCABI_HD inline bool window_key(const uint8_t *c, int k, float thr, const uint64_t *forb, int64_t n_forb, uint64_t *key) {
    uint64_t v = 0;
    bool dna = true;
    for (int i = 0; i < k; ++i) {
        const uint32_t x = c[i];
        dna = dna && x < 4;
        v = (v << 2) | (x & 3u);
    }
    if (!dna || low_complexity(v, k, thr) || forbidden(v, forb, n_forb)) return false;
    *key = v;
    return true;
}

// Bit i of p[b] is set when pattern base i (bits 2 (k - 1 - i) of the k-mer) is b; `all` has the k
// pattern bits, `high` the last one.
struct Masks {
    uint32_t p0, p1, p2, p3, all, high;
};

PCABI_HD inline Masks pattern_masks(uint64_t km, int k) {
    Masks m = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < k; ++i) {
        const uint32_t b = (uint32_t)(km >> (2 * (k - 1 - i))) & 3u;
        const uint32_t bit = 1u << i;
        m.p0 |= b == 0 ? bit : 0u;
        m.p1 |= b == 1 ? bit : 0u;
        m.p2 |= b == 2 ? bit : 0u;
        m.p3 |= b == 3 ? bit : 0u;
    }
    m.all = k == 32 ? 0xFFFFFFFFu : ((1u << k) - 1u);
    m.high = 1u << (k - 1);
    return m;
}

// the pattern positions that match the code x (an N matches none)
PCABI_HD inline uint32_t match_mask(const Masks &m, uint32_t x) {
    return x == 0 ? m.p0 : (x == 1 ? m.p1 : (x == 2 ? m.p2 : (x == 3 ? m.p3 : 0u)));
}

struct Column {
    uint32_t pv, mv;
    int score;
};

PCABI_HD inline Column first_column(const Masks &m, int k) { return Column{m.all, 0u, k}; }

// one text code: the next column's deltas and score. (eq and pv lie within `all` and ph, mh, pv, mv
// are masked where they are made, so the & all on the carry sum changes no result: bits of xh above the
// pattern reach nothing. It stays for the reader.)
PCABI_HD inline void myers_step(Column &c, const Masks &m, uint32_t eq) {
    const uint32_t xv = eq | c.mv;
    const uint32_t xh = ((((eq & c.pv) + c.pv) & m.all) ^ c.pv) | eq;
    uint32_t ph = c.mv | (~(xh | c.pv) & m.all);
    uint32_t mh = c.pv & xh;
    c.score += (ph & m.high) ? 1 : ((mh & m.high) ? -1 : 0);
    ph = (ph << 1) & m.all;
    mh = (mh << 1) & m.all;
    c.pv = mh | (~(xv | ph) & m.all);
    c.mv = ph & xv;
}

// The least edit distance of the pattern to a substring of the n codes at `words` (4-aligned).
PCABI_HD inline int best_distance(const Masks &m, int k, const uint32_t *words, int n) {
    Column c = first_column(m, k);
    int best = k;
    for (int j0 = 0; j0 < n; j0 += 4) {
        const uint32_t w = words[j0 >> 2];
        const int nb = n - j0 < 4 ? n - j0 : 4;
        for (int b = 0; b < nb; ++b) {
            myers_step(c, m, match_mask(m, (w >> (8 * b)) & 0xFFu));
            best = c.score < best ? c.score : best;
        }
    }
    return best;
}

}  // namespace pcabi_kmer
