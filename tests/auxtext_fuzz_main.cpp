// auxtext_fuzz_main.cpp -- csrc/pcabi_auxtext.h alone, as a program of its own, for a sanitizer build
// (tests/test_header_tags_cpu.py builds it with -fsanitize=address,undefined and runs it as a child
// process). TEST INFRASTRUCTURE ONLY.
//
// usage: auxtext_fuzz <seed> <rounds>
// Every round draws an aux chain (random tags of every type and subtype, names and bytes that the guards
// leave out now and then, arrays around the 64-element pass, strings around the 64-byte pass), truncates
// it now and then, puts it into a heap block of exactly its size, and checks
//   1. the byte-wise walk (walk) against a formatter of this file's own (snprintf): the same text, the same
//      counts, -1 for the same chains; written into a block of exactly the text's length;
//   2. the wave's walk, its 64 lanes played in turn: zh_lane with the two ballots for strings, elem_len, a
//      prefix sum and elem_put for arrays, the floats read from the host's table of slots (float_fill):
//      the same text again;
//   3. a text record of the chain: pack_fixed and pack_tile over tiles and 256 lanes against pack_part, and
//      both against the record put together here, in a block of exactly the record's length.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../custom_porechop_abi_amd/csrc/pcabi_auxtext.h"

using namespace pcabi_auxtext;

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
    explicit Exact(size_t n) : p((uint8_t *)malloc(n ? n : 1)) {
        if (!n) {
            free(p);
            p = (uint8_t *)malloc(0);
        }
    }
    ~Exact() { free(p); }
};

static void put32(std::vector<uint8_t> &v, uint32_t x) {
    for (int k = 0; k < 4; ++k) v.push_back((uint8_t)(x >> (8 * k)));
}

static int64_t edge_value(int w, bool sign) {
    static const int64_t e[] = {0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999999, 1000000000, 2147483647, 4294967295ll};
    int64_t v = e[rnd() % 15];
    if (rnd() % 3 == 0) v = rnd();
    if (sign && rnd() % 2) v = -v - (rnd() % 2);
    const int64_t lo = sign ? -((int64_t)1 << (8 * w - 1)) : 0, hi = sign ? ((int64_t)1 << (8 * w - 1)) - 1 : ((int64_t)1 << (8 * w)) - 1;
    return v < lo ? lo : v > hi ? hi : v;
}

static void put_number(std::vector<uint8_t> &v, char t) {
    if (t == 'f') {
        static const float e[] = {0.f, -0.5f, 1e-7f, 12345678.f, 3.4028234e38f, 1.17549435e-38f, 100000.f, 1e6f, 0.0125f};
        float f = e[rnd() % 9];
        if (rnd() % 3 == 0) {
            const uint32_t bits = rnd() ^ (rnd() << 16);
            memcpy(&f, &bits, 4);
        }
        if (rnd() % 16 == 0) f = rnd() % 2 ? __builtin_inff() : -__builtin_inff();
        uint32_t bits;
        memcpy(&bits, &f, 4);
        put32(v, bits);
        return;
    }
    const int w = width_of((uint8_t)t);
    const int64_t x = edge_value(w, t == 'c' || t == 's' || t == 'i');
    for (int k = 0; k < w; ++k) v.push_back((uint8_t)((uint64_t)x >> (8 * k)));
}

static std::vector<uint8_t> draw_chain() {
    std::vector<uint8_t> v;
    const int n_tags = (int)(rnd() % 6);
    static const char types[] = "AcCsSiIfZHBBB";
    static const char subs[] = "cCsSiIf";
    static const uint32_t lens[] = {0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200};
    for (int k = 0; k < n_tags; ++k) {
        v.push_back(rnd() % 12 ? (uint8_t)('A' + rnd() % 26 + (rnd() % 2) * 32) : (uint8_t)rnd());
        v.push_back(rnd() % 12 ? (uint8_t)(rnd() % 2 ? '0' + rnd() % 10 : 'a' + rnd() % 26) : (uint8_t)rnd());
        const char t = rnd() % 40 ? types[rnd() % 13] : (char)rnd();
        v.push_back((uint8_t)t);
        if (t == 'A') {
            v.push_back(rnd() % 8 ? (uint8_t)(0x20 + rnd() % 0x5F) : (uint8_t)rnd());
        } else if (t == 'Z' || t == 'H') {
            const uint32_t n = lens[rnd() % 13];
            const uint32_t ugly = rnd() % 6 ? n : rnd() % (n + 1);
            for (uint32_t j = 0; j < n; ++j) v.push_back(j == ugly ? (uint8_t)(1 + rnd() % 31) : (uint8_t)(0x20 + rnd() % 0x5F));
            if (rnd() % 20) v.push_back(0);
        } else if (t == 'B') {
            const char s = rnd() % 30 ? subs[rnd() % 7] : (char)rnd();
            v.push_back((uint8_t)s);
            const uint32_t n = lens[rnd() % 13];
            put32(v, rnd() % 40 ? n : n + 1 + rnd() % 5);   // now and then a count that runs past the end
            if (width_of((uint8_t)s))
                for (uint32_t j = 0; j < n; ++j) put_number(v, s == 'c' && rnd() % 2 ? 'C' : s);
        } else if (width_of((uint8_t)t)) {
            put_number(v, t);
        }
    }
    if (!v.empty() && rnd() % 8 == 0) v.resize(rnd() % v.size());
    return v;
}

// this file's own formatter: false when the chain does not walk
static bool format(const uint8_t *a, int64_t n, std::string *text, int64_t *written, int64_t *left) {
    int64_t at = 0;
    text->clear();
    *written = *left = 0;
    auto number = [&](char t, const uint8_t *p, std::string *o) {
        char buf[64];
        if (t == 'f') {
            float f;
            memcpy(&f, p, 4);
            snprintf(buf, sizeof buf, "%g", (double)f);
        } else {
            int64_t x = 0;
            const int w = width_of((uint8_t)t);
            uint64_t u = 0;
            for (int k = 0; k < w; ++k) u |= (uint64_t)p[k] << (8 * k);
            x = (int64_t)u;
            if ((t == 'c' || t == 's' || t == 'i') && (u >> (8 * w - 1))) x = (int64_t)u - ((int64_t)1 << (8 * w));
            snprintf(buf, sizeof buf, "%lld", (long long)x);
        }
        *o += buf;
    };
    while (at < n) {
        if (n - at < 3) return false;
        const uint8_t *tg = a + at;
        const char t = (char)tg[2];
        bool good = ((tg[0] >= 'A' && tg[0] <= 'Z') || (tg[0] >= 'a' && tg[0] <= 'z')) &&
                    ((tg[1] >= 'A' && tg[1] <= 'Z') || (tg[1] >= 'a' && tg[1] <= 'z') || (tg[1] >= '0' && tg[1] <= '9'));
        std::string val;
        int64_t q = at + 3;
        if (t == 'A') {
            if (n - q < 1) return false;
            good = good && a[q] >= 0x20 && a[q] <= 0x7E;
            val.push_back((char)a[q]);
            q += 1;
        } else if (t == 'Z' || t == 'H') {
            for (;; ++q) {
                if (q >= n) return false;
                if (a[q] == 0) break;
                if (a[q] < 0x20 || a[q] > 0x7E) good = false;
                val.push_back((char)a[q]);
            }
            q += 1;
        } else if (t == 'B') {
            if (n - q < 5) return false;
            const char s = (char)a[q];
            const int w = strchr("cC", s) ? 1 : strchr("sS", s) ? 2 : strchr("iIf", s) ? 4 : 0;
            if (!s || !w) return false;
            const int64_t count = (int64_t)((uint32_t)a[q + 1] | (uint32_t)a[q + 2] << 8 | (uint32_t)a[q + 3] << 16 | (uint32_t)a[q + 4] << 24);
            q += 5;
            if (count * w > n - q) return false;
            val.push_back(s);
            for (int64_t k = 0; k < count; ++k) {
                val.push_back(',');
                number(s, a + q + k * w, &val);
            }
            q += count * w;
        } else {
            const int w = t && strchr("cC", t) ? 1 : t && strchr("sS", t) ? 2 : t && strchr("iIf", t) ? 4 : 0;
            if (!w || n - q < w) return false;
            number(t, a + q, &val);
            q += w;
        }
        if (good) {
            *text += '\t';
            *text += (char)tg[0];
            *text += (char)tg[1];
            *text += ':';
            *text += t == 'f' || t == 'A' || t == 'Z' || t == 'H' || t == 'B' ? t : 'i';
            *text += ':';
            *text += val;
            ++*written;
        } else {
            ++*left;
        }
        at = q;
    }
    return true;
}

// the wave's walk (pcabi_auxtext.hip wave_walk), the 64 lanes in turn
static int64_t lanes_walk(const uint8_t *a, int64_t n, Floats fl, uint8_t *dst, int64_t room) {
    int64_t at = 0, len = 0;
    while (at < n) {
        Tag t = tag_at(a, n, at);
        if (!t.ok) return -1;
        bool good = name_ok(a + at);
        int64_t vlen = 0;
        if (t.type == 'Z' || t.type == 'H') {
            int64_t end = -1;
            bool bad = false;
            for (int64_t q = t.val; q < n && end < 0; q += kWaveLanes) {
                uint64_t nul = 0, ugly = 0;
                for (int l = 0; l < kWaveLanes; ++l) {
                    const int c = zh_lane(a, n, q + l);
                    nul |= (uint64_t)(c == 1) << l, ugly |= (uint64_t)(c == 2) << l;
                }
                if (nul) {
                    const int f = __builtin_ctzll(nul);
                    if (ugly & (((uint64_t)1 << f) - 1)) bad = true;
                    end = q + f;
                } else if (ugly) {
                    bad = true;
                }
            }
            if (end < 0) return -1;
            good = good && !bad;
            vlen = end - t.val;
            t.next = end + 1;
        } else if (t.type == 'A') {
            good = good && printable(a[t.val]);
            vlen = 1;
        } else if (t.type == 'f') {
            uint8_t s[kFloatSlot];
            vlen = float_get(fl, 0, a + t.val, s);
        } else if (t.type != 'B') {
            vlen = dec_len(int_at(a + t.val, t.type));
        }
        uint8_t *d = dst ? dst + len + kHead : nullptr;
        const int64_t rm = dst ? room - len : 0, r = rm - kHead;
        if (good) {
            for (int l = 0; l < kHead; ++l)
                if (l < rm) dst[len + l] = head_byte(a + at, l);
            if (t.type == 'Z' || t.type == 'H' || t.type == 'A') {
                for (int l = 0; l < kWaveLanes; ++l)
                    for (int64_t k = l; k < vlen && k < r; k += kWaveLanes) d[k] = a[t.val + k];
            } else if (t.type == 'f') {
                uint8_t s[kFloatSlot];
                const int m = float_get(fl, 0, a + t.val, s);
                for (int k = 0; k < m && k < r; ++k) d[k] = s[k];
            } else if (t.type != 'B') {
                dec_put(d, r, int_at(a + t.val, t.type), (int)vlen);
            }
        }
        if (t.type == 'B') {
            if (good && r > 0) d[0] = t.sub;
            int64_t w = 1;
            if (good)
                for (int64_t k0 = 0; k0 < t.count; k0 += kWaveLanes) {
                    int el[kWaveLanes], total = 0;
                    for (int l = 0; l < kWaveLanes; ++l) el[l] = k0 + l < t.count ? elem_len(a, t, k0 + l, fl) : 0;
                    for (int l = 0; l < kWaveLanes; ++l) {
                        if (dst && k0 + l < t.count) elem_put(d + w + total, r - w - total, a, t, k0 + l, fl, el[l]);
                        total += el[l];
                    }
                    w += total;
                }
            vlen = w;
        }
        if (t.type == 'f') fl.cur += 1;
        if (t.type == 'B' && t.sub == 'f') fl.cur += t.count;
        if (good) len += kHead + vlen;
        at = t.next;
    }
    return len;
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s <seed> <rounds>\n", argv[0]);
        return 2;
    }
    g_state = strtoull(argv[1], nullptr, 10) * 0x9E3779B97F4A7C15ull + 1;
    const long rounds = strtol(argv[2], nullptr, 10);
    long n_bad = 0, n_left = 0, n_floats = 0;
    for (long round = 0; round < rounds; ++round) {
        const std::vector<uint8_t> chain = draw_chain();
        const int64_t n = (int64_t)chain.size();
        Exact blk((size_t)n);
        if (n) memcpy(blk.p, chain.data(), (size_t)n);
        std::string want;
        int64_t ww = 0, wl = 0;
        const bool ok = format(blk.p, n, &want, &ww, &wl);
        // 1. the byte-wise walk
        int64_t gw = 0, gl = 0;
        const int64_t len = walk(blk.p, n, Floats{nullptr, 0, 0}, nullptr, 0, &gw, &gl);
        CHECK(ok ? len == (int64_t)want.size() : len == -1);
        if (!ok) {
            CHECK(gw == 0 && gl == 0);
            CHECK(lanes_walk(blk.p, n, Floats{nullptr, 0, 0}, nullptr, 0) == -1);
            CHECK(float_count(blk.p, n) == -1);
            ++n_bad;
            continue;
        }
        CHECK(gw == ww && gl == wl);
        n_left += wl;
        Exact t1((size_t)len), t2((size_t)len), t3((size_t)(len > 3 ? len - 3 : 0));
        CHECK(walk(blk.p, n, Floats{nullptr, 0, 0}, t1.p, len, nullptr, nullptr) == len);
        CHECK(memcmp(t1.p, want.data(), (size_t)len) == 0);
        // 2. the lanes in turn, the floats from the host's table
        std::vector<uint8_t> slots;
        const int64_t nf = float_count(blk.p, n);
        CHECK(nf >= 0);
        float_fill(blk.p, n, &slots);
        CHECK((int64_t)slots.size() == nf * kFloatSlot);
        n_floats += nf;
        Exact tab(slots.size());
        if (!slots.empty()) memcpy(tab.p, slots.data(), slots.size());
        const Floats fl{slots.empty() ? (const uint8_t *)"" : tab.p, nf, 0};
        CHECK(lanes_walk(blk.p, n, fl, t2.p, len) == len);
        CHECK(memcmp(t2.p, want.data(), (size_t)len) == 0);
        CHECK(walk(blk.p, n, fl, nullptr, 0, nullptr, nullptr) == len);
        // a room smaller than the text: nothing behind it is written
        if (len > 3) {
            CHECK(lanes_walk(blk.p, n, fl, t3.p, len - 3) == len);
            CHECK(memcmp(t3.p, want.data(), (size_t)(len - 3)) == 0);
        }
        // 3. a text record
        for (int fasta = 0; fasta < 2; ++fasta) {
            static const int64_t ls[] = {1, 69, 70, 71, 140, 141, 333, 16383, 16384, 16385, 33000};
            const int64_t l_seq = ls[rnd() % (round % 16 ? 7 : 11)], name_len = rnd() % 40, off = rnd() % 16;
            std::vector<uint8_t> seq((size_t)l_seq), qual((size_t)l_seq), side;
            for (auto &c : seq) c = (uint8_t)"ACGTN"[rnd() % 5];
            for (auto &c : qual) c = (uint8_t)(33 + rnd() % 94);
            side.insert(side.end(), chain.begin(), chain.end());
            for (int64_t k = 0; k < name_len; ++k) side.push_back((uint8_t)('a' + rnd() % 26));
            pcabi_fastx_part p;
            memset(&p, 0, sizeof p);
            p.l_seq = (int32_t)l_seq, p.l_qual = fasta ? 0 : (int32_t)l_seq, p.name_off = n, p.name_len = (int32_t)name_len;
            p.aux_len = (int32_t)n, p.text_len = len, p.flags = rnd() % 3 == 0 ? PCABI_FASTX_RNA : 0, p.out = off;
            std::string rec(1, fasta ? '>' : '@');
            rec.append((const char *)side.data() + n, (size_t)name_len);
            rec += want;
            rec += '\n';
            std::string bases((const char *)seq.data(), (size_t)l_seq);
            if (p.flags)
                for (char &c : bases)
                    if (c == 'T') c = 'U';
            if (fasta) {
                for (int64_t k = 0; k < l_seq; k += 70) rec += bases.substr((size_t)k, 70) + "\n";
            } else {
                rec += bases + "\n+\n" + std::string((const char *)qual.data(), (size_t)l_seq) + "\n";
            }
            const int64_t rl = record_len(p, fasta != 0);
            CHECK(rl == (int64_t)rec.size());
            CHECK(fastx_fits(p, fasta != 0, l_seq, l_seq, (int64_t)side.size(), off + rl));
            Exact sq((size_t)l_seq), ql((size_t)l_seq), sd(side.size()), a((size_t)(off + rl)), b((size_t)(off + rl));
            memcpy(sq.p, seq.data(), (size_t)l_seq);
            memcpy(ql.p, qual.data(), (size_t)l_seq);
            if (!side.empty()) memcpy(sd.p, side.data(), side.size());
            memset(a.p, 0xA5, (size_t)(off + rl));
            memset(b.p, 0xA5, (size_t)(off + rl));
            pack_part(p, fasta != 0, sq.p, ql.p, sd.p, a.p);
            CHECK(memcmp(a.p + off, rec.data(), (size_t)rl) == 0);
            for (int64_t t = 0; t < part_tiles(p); ++t) {
                const int64_t t0 = t * kTileBases, t1e = t0 + kTileBases < l_seq ? t0 + kTileBases : l_seq;
                for (int l = 0; l < 256; ++l) {
                    if (t == 0) pack_fixed(p, fasta != 0, sd.p, b.p + off, l, 256);
                    pack_tile(p, fasta != 0, sq.p, ql.p, b.p + off, t0, t1e, l, 256);
                }
            }
            if (len > 0) CHECK(lanes_walk(sd.p, n, fl, b.p + off + 1 + name_len, len) == len);
            CHECK(memcmp(b.p + off, rec.data(), (size_t)rl) == 0);
            for (int64_t i = 0; i < off; ++i) CHECK(a.p[i] == 0xA5 && b.p[i] == 0xA5);
        }
    }
    printf("rounds %ld unwalkable %ld left_out %ld floats %ld\n", rounds, n_bad, n_left, n_floats);
    return 0;
}
