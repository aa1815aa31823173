// moves_fuzz_main.cpp -- csrc/pcabi_moves.h alone, as a program of its own, for a sanitizer build
// (tests/test_moves_cpu.py builds it with -fsanitize=address,undefined and runs it as a child process).
// TEST INFRASTRUCTURE ONLY.
//
// usage: moves_fuzz <seed> <rounds>
// Every round draws a move table (random or edge length around the 16-byte, 64-byte and segment sizes,
// random dwell, now and then a long run of zeros or an invalid byte) at a random offset of a heap block of
// exactly its size, and checks against the byte-by-byte walk
//   1. count: every segment counted as the kernel does it, the 64 lanes played in turn (count_lane), and as
//      the host does it (one lane): the same ones and the same verdict as the walk's;
//   2. select: for random k and the edge ones (first and last of the table, of a segment), select_seg over
//      the prefixes, then the segment by 64 bytes a pass with the lanes' ballot and is_kth: the walk's p(k);
//   3. copy: a part's tag bytes written into a block of exactly their length at a random alignment, by
//      chunks of kChunk with 64 lanes (copy_lane) and by one lane: the bytes the rule states.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../custom_porechop_abi_amd/csrc/pcabi_moves.h"

using namespace pcabi_moves;

static uint64_t g_state;
static uint32_t rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33);
}

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "line %d: %s\n", __LINE__, #c);             \
            abort();                                                    \
        }                                                               \
    } while (0)

// a block of exactly n bytes (n == 0 too), so that a byte past either end is the sanitizer's
struct Exact {
    uint8_t *p;
    explicit Exact(size_t n) : p((uint8_t *)malloc(n ? n : 1)) {}
    ~Exact() { free(p); }
};

static const int64_t kEdge[] = {0, 1, 2, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8193, 12289};

// p(k) of the selection as the kernel does it
static int64_t select_wave(const uint8_t *tags, const pcabi_moves_read &r, const std::vector<int64_t> &pre, int64_t k) {
    const int64_t n = n_moves(r), ns = n_segs(r);
    int64_t before = 0;
    const int64_t sg = select_seg(pre.data(), ns, k, &before);
    if (sg >= ns) return n;
    const int64_t a = moves_at(r) + sg * kSeg, e = moves_at(r) + (n < (sg + 1) * kSeg ? n : (sg + 1) * kSeg);
    int64_t left = k - before;
    for (int64_t pos = a; pos < e; pos += 64) {
        uint64_t m = 0;
        for (int l = 0; l < 64; ++l)
            if (pos + l < e && tags[pos + l] == 1) m |= (uint64_t)1 << l;
        const int c = popc64(m);
        if (left < c) {
            int hits = 0, lane = -1;
            for (int l = 0; l < 64; ++l)
                if (is_kth(m, l, left)) ++hits, lane = l;
            CHECK(hits == 1);
            return pos - moves_at(r) + lane;
        }
        left -= c;
    }
    return n;
}

int main(int argc, char **argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const long rounds = argc > 2 ? atol(argv[2]) : 1000;
    g_state = seed * 0x9E3779B97F4A7C15ull + 1;
    long n_bad = 0, n_parts = 0;
    for (long round = 0; round < rounds; ++round) {
        const int64_t n = rnd() % 4 ? kEdge[rnd() % (sizeof kEdge / sizeof *kEdge)] + (rnd() % 8 == 0 ? rnd() % 3 : 0) : rnd() % 20000;
        const int64_t pad = rnd() % 40, tail = rnd() % 3 ? 0 : rnd() % 20;
        const int64_t tags_n = pad + 1 + n + tail;
        Exact blob((size_t)tags_n);
        for (int64_t i = 0; i < tags_n; ++i) blob.p[i] = (uint8_t)rnd();   // what lies around the table is anything
        pcabi_moves_read r;
        memset(&r, 0, sizeof r);
        r.mv_off = pad, r.n_vals = (int32_t)(n + 1), r.ts = rnd() % 3 ? (int32_t)(rnd() % 100000) : -1, r.n_parts = 0;
        const int stride = 1 + rnd() % 127;
        blob.p[pad] = (uint8_t)stride;
        uint8_t *mv = blob.p + pad + 1;
        const uint32_t dwell = 1 + rnd() % 6;
        for (int64_t i = 0; i < n; ++i) mv[i] = rnd() % dwell == 0;
        if (n > 0 && rnd() % 4 == 0) {   // a long run without a one: whole segments of it, or a leading one
            const int64_t a = rnd() % 2 ? 0 : rnd() % n, len = rnd() % (n - a + 1);
            memset(mv + a, 0, (size_t)len);
        }
        const bool spoil = n > 0 && rnd() % 5 == 0;
        if (spoil) mv[rnd() % 3 == 0 ? n - 1 : rnd() % n] = rnd() % 2 ? 2 : 0xFF;
        CHECK(read_fits(r, tags_n, 0) && stride_of(blob.p, r) == stride);

        // 1. count
        const int64_t ns = n_segs(r);
        std::vector<int64_t> pre((size_t)ns + 1, 0);
        int64_t walk_ones = 0, walk_bad_segs = 0;
        for (int64_t s = 0; s < ns; ++s) {
            const int64_t a = moves_at(r) + s * kSeg, e = moves_at(r) + (n < (s + 1) * kSeg ? n : (s + 1) * kSeg);
            int64_t ones = 0, lanes_ones = 0, host_ones = 0;
            bool ok = true, lanes_ok = true;
            for (int64_t i = a; i < e; ++i) ok = ok && blob.p[i] <= 1;
            for (int64_t i = a; i < e; ++i) ones += blob.p[i] == 1;
            for (int l = 0; l < 64; ++l) lanes_ok = count_lane(blob.p, a, e, l, 64, &lanes_ones) && lanes_ok;
            const bool host_ok = count_lane(blob.p, a, e, 0, 1, &host_ones);
            CHECK(lanes_ok == ok && host_ok == ok);
            if (ok) CHECK(lanes_ones == ones && host_ones == ones);
            CHECK(lanes_ones == host_ones);
            pre[(size_t)s + 1] = pre[(size_t)s] + seg_value(lanes_ones, lanes_ok);
            walk_ones += ones, walk_bad_segs += !ok;
        }
        int64_t ones = 0, bad_segs = 0;
        read_sums(pre[0], pre[(size_t)ns], &ones, &bad_segs);
        CHECK(bad_segs == walk_bad_segs && (bad_segs == 0) == !spoil);
        r.l_seq = (int32_t)walk_ones;
        CHECK(table_usable(r, stride, ones, bad_segs) == !spoil);
        if (spoil) {
            ++n_bad;
            continue;
        }
        CHECK(ones == walk_ones);

        // 2. select
        std::vector<int64_t> p_of;
        for (int64_t i = 0; i < n; ++i)
            if (mv[i] == 1) p_of.push_back(i);
        p_of.push_back(n);
        std::vector<int64_t> ks = {0, ones, ones > 0 ? ones - 1 : 0};
        for (int64_t s = 1; s <= ns; ++s) {   // the first and the last one of a segment
            const int64_t b = pre[(size_t)s] & (kBadUnit - 1);
            ks.push_back(b < ones ? b : ones);
            ks.push_back(b > 0 ? b - 1 : 0);
        }
        for (int t = 0; t < 8; ++t) ks.push_back(rnd() % (ones + 1));
        for (int64_t k : ks) {
            const int64_t got = select_wave(blob.p, r, pre, k);
            CHECK(got == p_of[(size_t)k]);
            // the host build's way
            int64_t before = 0, at = n;
            const int64_t sg = select_seg(pre.data(), ns, k, &before);
            if (sg < ns) {
                const int64_t a = moves_at(r) + sg * kSeg;
                const int64_t w = select_walk(blob.p, a, moves_at(r) + (n < (sg + 1) * kSeg ? n : (sg + 1) * kSeg), k - before);
                CHECK(w >= 0);
                at = sg * kSeg + w;
            }
            CHECK(at == got);
        }

        // 3. copy
        for (int t = 0; t < 3; ++t) {
            pcabi_moves_part part;
            memset(&part, 0, sizeof part);
            part.s0 = (int32_t)(rnd() % 3 == 0 ? 0 : rnd() % (ones + 1));
            part.ns = (int32_t)(rnd() % 4 == 0 ? ones - part.s0 : rnd() % (ones - part.s0 + 1));
            const int64_t k0 = edge_k(part, 0), q0 = k0 < 0 ? 0 : p_of[(size_t)k0], q1 = p_of[(size_t)edge_k(part, 1)];
            CHECK(q0 <= q1);
            const int64_t len = tag_len(r, q0, q1), m = q1 - q0, ts_new = ts_of(r, stride, q0), off = rnd() % 16;
            std::vector<uint8_t> want;
            for (char c : {'m', 'v', 'B', 'c'}) want.push_back((uint8_t)c);
            for (int b = 0; b < 4; ++b) want.push_back((uint8_t)((uint64_t)(1 + m) >> (8 * b)));
            want.push_back((uint8_t)stride);
            want.insert(want.end(), mv + q0, mv + q1);
            if (r.ts >= 0) {
                for (char c : {'t', 's', 'i'}) want.push_back((uint8_t)c);
                for (int b = 0; b < 4; ++b) want.push_back((uint8_t)((uint64_t)ts_new >> (8 * b)));
            }
            CHECK((int64_t)want.size() == len);
            int64_t kept = 0;
            for (int64_t i = q0; i < q1; ++i) kept += mv[i];
            CHECK(kept == part.ns);
            // (the 16-byte stores want a 16-aligned block to be aligned against: a block of len + off bytes
            // from aligned_alloc would be padded, so the block is exact and the offset moves the part)
            Exact a((size_t)(len + off)), b((size_t)(len + off));
            memset(a.p, 0xA5, (size_t)(len + off));
            memset(b.p, 0xA5, (size_t)(len + off));
            for (int64_t j0 = 0; j0 < len; j0 += kChunk)
                for (int l = 0; l < 64; ++l) copy_lane(a.p + off, mv + q0, m, stride, ts_new, len, j0, j0 + kChunk, l, 64);
            copy_lane(b.p + off, mv + q0, m, stride, ts_new, len, 0, len, 0, 1);
            CHECK(memcmp(a.p + off, want.data(), (size_t)len) == 0 && memcmp(b.p + off, want.data(), (size_t)len) == 0);
            for (int64_t i = 0; i < off; ++i) CHECK(a.p[i] == 0xA5 && b.p[i] == 0xA5);
            ++n_parts;
        }
    }
    printf("rounds %ld unusable %ld parts %ld\n", rounds, n_bad, n_parts);
    return 0;
}
