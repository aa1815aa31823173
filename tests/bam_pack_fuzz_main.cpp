// bam_pack_fuzz_main.cpp -- the pack half of csrc/pcabi_bam.h alone, as a program of its own, for a
// sanitizer build (tests/test_bam_pack_cpu.py builds it with -fsanitize=address,undefined and runs it as
// a child process). TEST INFRASTRUCTURE ONLY.
//
// usage: bam_pack_fuzz <seed> <rounds>
// Every round draws a random part table (lengths around the 16-byte and tile edges, random names, aux
// bytes and source offsets) over heap blocks of exactly the sizes the table needs, and checks
//   1. the planned chain packed whole (pack_part) against a byte-wise restatement written here;
//   2. the same chain packed the way the kernel does it -- heads strided over 256 lanes, tiles of 16384
//      bases cut into pieces of the destination's 16-byte grid -- at every output misalignment: same bytes,
//      and the bytes around the chain untouched;
//   3. pack followed by unpack_range gives the letters (after the letter map) and qualities back;
//   4. random bytes, and chains of valid tags cut short, through the aux walk.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../custom_porechop_abi_amd/csrc/pcabi_bam.h"

using namespace pcabi_bam;

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

// ---- the restatement: plain tables, one byte at a time ------------------------------------------
static int ref_code(uint8_t c) {
    static const char *kLetters = "=ACMGRSVTWYHKDBN";
    if (c == 'U') return 8;
    for (int k = 0; k < 16; ++k)
        if (c != 0 && (uint8_t)kLetters[k] == c) return k;
    return 15;
}
static void put32(std::vector<uint8_t> &o, int64_t v) {
    for (int k = 0; k < 4; ++k) o.push_back((uint8_t)((uint32_t)v >> (8 * k)));
}
static void put16(std::vector<uint8_t> &o, int v) {
    o.push_back((uint8_t)v);
    o.push_back((uint8_t)(v >> 8));
}
static std::vector<uint8_t> ref_record(const pcabi_bam_part &p, const uint8_t *seq, const uint8_t *qual, const uint8_t *side) {
    std::vector<uint8_t> o;
    const int64_t l = p.l_seq;
    put32(o, 32 + p.name_len + 1 + (l + 1) / 2 + l + p.aux_len);
    put32(o, -1);
    put32(o, -1);
    o.push_back((uint8_t)(p.name_len + 1));
    o.push_back(0);
    put16(o, 4680);
    put16(o, 0);
    put16(o, 4);
    put32(o, l);
    put32(o, -1);
    put32(o, -1);
    put32(o, 0);
    for (int k = 0; k < p.name_len; ++k) o.push_back(side[p.side_off + k]);
    o.push_back(0);
    for (int64_t i = 0; i < l; i += 2) {
        const int hi = ref_code(seq[p.seq_src + i]), lo = i + 1 < l ? ref_code(seq[p.seq_src + i + 1]) : 0;
        o.push_back((uint8_t)(hi * 16 + lo));
    }
    for (int64_t i = 0; i < l; ++i) {
        if (p.qual_src < 0) {
            o.push_back(0xff);
        } else {
            const int c = qual[p.qual_src + i];
            o.push_back((uint8_t)(c < 33 ? 0 : c > 126 ? 93 : c - 33));
        }
    }
    for (int k = 0; k < p.aux_len; ++k) o.push_back(side[p.side_off + p.name_len + k]);
    return o;
}

// the kernel's walk over one part, on the host: lanes and pieces in turn
static void pack_like_kernel(const pcabi_bam_part &p, const uint8_t *seq, const uint8_t *qual, const uint8_t *side, uint8_t *out) {
    uint8_t *rec = out + p.out;
    for (int lane = 0; lane < 256; ++lane) pack_head(p, side, rec, lane, 256);
    const uint8_t *src = seq + p.seq_src, *qsrc = p.qual_src >= 0 ? qual + p.qual_src : nullptr;
    uint8_t *sq = rec + part_seq_at(p), *ql = sq + ((int64_t)p.l_seq + 1) / 2;
    for (int64_t t0 = 0; t0 < p.l_seq; t0 += kTileBases) {
        const int64_t t1 = t0 + kTileBases < p.l_seq ? t0 + kTileBases : (int64_t)p.l_seq;
        {
            const int64_t d = (int64_t)(uintptr_t)sq, y0 = t0 / 2, y1 = (t1 + 1) / 2;
            const int64_t a = (d + y0) & ~(int64_t)15, pieces = (d + y1 - a + 15) >> 4;
            for (int64_t k = 0; k < pieces; ++k) {
                const int64_t q0 = a + 16 * k - d, c0 = q0 > y0 ? q0 : y0, c1 = q0 + 16 < y1 ? q0 + 16 : y1;
                pack_range(src, qsrc, p.l_seq, 2 * c0, 2 * c1 < t1 ? 2 * c1 : t1, sq, nullptr);
            }
        }
        {
            const int64_t d = (int64_t)(uintptr_t)ql;
            const int64_t a = (d + t0) & ~(int64_t)15, pieces = (d + t1 - a + 15) >> 4;
            for (int64_t k = 0; k < pieces; ++k) {
                const int64_t q0 = a + 16 * k - d, b0 = q0 > t0 ? q0 : t0, b1 = q0 + 16 < t1 ? q0 + 16 : t1;
                pack_range(src, qsrc, p.l_seq, b0, b1, nullptr, ql);
            }
        }
    }
}

static void round_tables() {
    static const int kLens[] = {0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 63, 64, 65, 255, 256, 257, 16383, 16384, 16385, 32769};
    static const char kAlphabet[] = "=ACMGRSVTWYHKDBNUacgtn.*- \x01\x7f";
    const int n_parts = 1 + (int)(rnd() % 6);
    std::vector<pcabi_bam_part> parts((size_t)n_parts);
    int64_t seq_n = rnd() % 17, qual_n = rnd() % 17, side_n = rnd() % 5;
    for (pcabi_bam_part &p : parts) {
        memset(&p, 0, sizeof p);
        const uint32_t pick = rnd() % 24;
        p.l_seq = pick < 21 ? kLens[pick] : (int32_t)(rnd() % 600);
        if (p.l_seq > 300 && rnd() % 4) p.l_seq = (int32_t)(rnd() % 300);   // long ones now and then
        p.name_len = rnd() % 8 == 0 ? 254 : (int32_t)(rnd() % 18);
        p.aux_len = rnd() % 3 == 0 ? 0 : (int32_t)(rnd() % 40);
        p.seq_src = seq_n;
        seq_n += p.l_seq + rnd() % 3;
        p.qual_src = rnd() % 5 == 0 ? -1 : qual_n;
        if (p.qual_src >= 0) qual_n += p.l_seq + rnd() % 3;
        p.side_off = side_n;
        side_n += p.name_len + p.aux_len;
    }
    // exact-size heap blocks: the last part's sources end where the blocks end
    seq_n = parts.back().seq_src + parts.back().l_seq;
    int64_t q_end = 0;
    for (const pcabi_bam_part &p : parts)
        if (p.qual_src >= 0 && p.qual_src + p.l_seq > q_end) q_end = p.qual_src + p.l_seq;
    qual_n = q_end;
    uint8_t *seq = new uint8_t[seq_n ? (size_t)seq_n : 1], *qual = new uint8_t[qual_n ? (size_t)qual_n : 1],
            *side = new uint8_t[side_n ? (size_t)side_n : 1];
    for (int64_t i = 0; i < seq_n; ++i) seq[i] = rnd() % 8 ? (uint8_t)kAlphabet[rnd() % (sizeof kAlphabet - 1)] : (uint8_t)rnd();
    for (int64_t i = 0; i < qual_n; ++i) qual[i] = rnd() % 8 ? (uint8_t)(33 + rnd() % 94) : (uint8_t)rnd();
    for (int64_t i = 0; i < side_n; ++i) side[i] = (uint8_t)(1 + rnd() % 255);
    PackLayout lay;
    for (pcabi_bam_part &p : parts) lay.place(&p);
    const int64_t total = lay.out;
    std::vector<uint8_t> ref;
    int64_t tiles = 0;
    for (const pcabi_bam_part &p : parts) {
        CHECK(part_fits(p, seq_n, qual_n, side_n, total));
        CHECK(p.out == (int64_t)ref.size() && p.tile0 == tiles);
        tiles += p.l_seq == 0 ? 1 : (p.l_seq + 16383) / 16384;
        const std::vector<uint8_t> r = ref_record(p, seq, qual, side);
        CHECK((int64_t)r.size() == part_size(p));
        ref.insert(ref.end(), r.begin(), r.end());
    }
    CHECK(tiles == lay.tiles && (int64_t)ref.size() == total);
    // 1. whole, into a block of exactly the chain's size
    uint8_t *whole = new uint8_t[total ? (size_t)total : 1];
    memset(whole, 0xA5, (size_t)total);
    for (const pcabi_bam_part &p : parts) pack_part(p, seq, qual, side, whole);
    CHECK(memcmp(whole, ref.data(), (size_t)total) == 0);
    // 2. the kernel's way at one misalignment a round (all sixteen over the rounds), bytes around untouched
    const int shift = (int)(rnd() % 16);
    const size_t room = (((size_t)total + (size_t)shift + 15) / 16 + 1) * 16;
    uint8_t *raw = (uint8_t *)aligned_alloc(16, room);
    memset(raw, 0xA5, room);
    for (const pcabi_bam_part &p : parts) pack_like_kernel(p, seq, qual, side, raw + shift);
    CHECK(memcmp(raw + shift, ref.data(), (size_t)total) == 0);
    for (size_t i = 0; i < room; ++i)
        if (i < (size_t)shift || i >= (size_t)shift + (size_t)total) CHECK(raw[i] == 0xA5);
    // 3. back through the unpack: the letters after the letter map, the qualities after the clamp
    for (const pcabi_bam_part &p : parts) {
        const int64_t l = p.l_seq;
        uint8_t *s2 = new uint8_t[l ? (size_t)l : 1], *q2 = new uint8_t[l ? (size_t)l : 1];
        const uint8_t *sq = whole + p.out + part_seq_at(p);
        unpack_range(sq, p.l_seq, 4, 0, l, s2, q2, nullptr);
        for (int64_t i = 0; i < l; ++i) {
            CHECK(s2[i] == (uint8_t)"=ACMGRSVTWYHKDBN"[ref_code(seq[p.seq_src + i])]);
            if (p.qual_src < 0) {
                CHECK(q2[i] == '+');
            } else {
                const int c = qual[p.qual_src + i];
                // (a first quality of 0xFF reads as "absent": the clamp never writes it)
                CHECK(q2[i] == (uint8_t)((c < 33 ? 0 : c > 126 ? 93 : c - 33) + 33));
            }
        }
        delete[] s2;
        delete[] q2;
    }
    free(raw);
    delete[] whole;
    delete[] seq;
    delete[] qual;
    delete[] side;
}

static void append_tag(std::vector<uint8_t> &a) {
    static const char kTypes[] = "AcCsSiIfZHB";
    const char t = kTypes[rnd() % 11];
    a.push_back((uint8_t)('A' + rnd() % 26));
    a.push_back((uint8_t)('a' + rnd() % 26));
    a.push_back((uint8_t)t);
    auto bytes = [&](int n) {
        for (int k = 0; k < n; ++k) a.push_back((uint8_t)rnd());
    };
    if (t == 'A' || t == 'c' || t == 'C') bytes(1);
    else if (t == 's' || t == 'S') bytes(2);
    else if (t == 'i' || t == 'I' || t == 'f') bytes(4);
    else if (t == 'Z' || t == 'H') {
        for (int k = (int)(rnd() % 9); k > 0; --k) a.push_back((uint8_t)(1 + rnd() % 255));
        a.push_back(0);
    } else {
        static const char kSub[] = "cCsSiIf";
        static const int kWidth[] = {1, 1, 2, 2, 4, 4, 4};
        const int sub = (int)(rnd() % 7), count = (int)(rnd() % 6);
        a.push_back((uint8_t)kSub[sub]);
        put32(a, count);
        bytes(count * kWidth[sub]);
    }
}

static void round_aux() {
    // a chain of valid tags walks tag by tag to its end; cut anywhere inside a tag it does not
    std::vector<uint8_t> a;
    std::vector<size_t> ends{0};
    for (int k = (int)(rnd() % 6); k > 0; --k) {
        append_tag(a);
        ends.push_back(a.size());
    }
    {
        uint8_t *h = new uint8_t[a.size() ? a.size() : 1];
        if (!a.empty()) memcpy(h, a.data(), a.size());
        int64_t at = 0;
        for (size_t k = 1; k < ends.size(); ++k) {
            at = aux_next(h, (int64_t)a.size(), at);
            CHECK(at == (int64_t)ends[k]);
        }
        CHECK(aux_walks(h, (int64_t)a.size()));
        delete[] h;
    }
    if (!a.empty()) {
        const size_t cut = rnd() % a.size();
        bool on_edge = false;
        for (size_t e : ends) on_edge = on_edge || e == cut;
        uint8_t *h = new uint8_t[cut ? cut : 1];
        if (cut) memcpy(h, a.data(), cut);
        CHECK(aux_walks(h, (int64_t)cut) == on_edge);
        delete[] h;
    }
    // random bytes in a block of exactly their size: the walk ends inside it, whatever it says
    const size_t n = rnd() % 64;
    uint8_t *r = new uint8_t[n ? n : 1];
    for (size_t i = 0; i < n; ++i) r[i] = rnd() % 3 ? (uint8_t)"AcCsSiIfZHBX\0"[rnd() % 13] : (uint8_t)rnd();
    int64_t at = 0;
    while (at >= 0 && at < (int64_t)n) {
        const int64_t nx = aux_next(r, (int64_t)n, at);
        CHECK(nx < 0 || (nx > at && nx <= (int64_t)n));
        at = nx;
    }
    delete[] r;
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: bam_pack_fuzz <seed> <rounds>\n");
        return 2;
    }
    g_state = strtoull(argv[1], nullptr, 10) * 2654435761ull + 1;
    const long rounds = atol(argv[2]);
    for (long k = 0; k < rounds; ++k) {
        round_tables();
        round_aux();
    }
    printf("rounds %ld\n", rounds);
    return 0;
}
