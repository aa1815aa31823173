// mods_fuzz_main.cpp -- csrc/pcabi_mods.h alone, as a program of its own, for a sanitizer build
// (tests/test_mods_cpu.py builds it with -fsanitize=address,undefined and runs it as a child process).
// TEST INFRASTRUCTURE ONLY.
//
// usage: mods_fuzz <seed> <rounds>
// Every round draws a read, an MM text (random bytes, bytes over the grammar's alphabet, or a valid text,
// whole or with single bytes flipped), ML values and a part table, all in heap blocks of exactly their
// sizes, and checks
//   1. the walk byte by byte (parse) against the walk 64 bytes a pass with the lanes played one after
//      another (lane_load / lane_judge / lane_store / pass_advance, the kernel's order of steps): the same
//      verdict, and for a text that passes the same tables;
//   2. a valid text left whole is usable and gives back its own entries;
//   3. for a usable read, every part's tags written into a block of exactly the planned length, once by
//      the host's loop and once as the kernel strides them (64 lanes, emit_fixed / emit_group): the same
//      bytes, which walk as an aux chain (pcabi_bam.h aux_walks).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../custom_porechop_abi_amd/csrc/pcabi_mods.h"

using namespace pcabi_mods;

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
template <class T>
struct Exact {
    T *p;
    explicit Exact(size_t n) : p((T *)malloc(n * sizeof(T) ? n * sizeof(T) : 1)) {}
    ~Exact() { free(p); }
};

// the walk as the kernel does it, the lanes played in turn
static bool parse_wave(const uint8_t *t, int64_t n, Ent *ents, int64_t cap, Group *groups, int *n_groups, int64_t *n_ent) {
    PassState st;
    for (int64_t pos = 0; pos < n; pos += 64) {
        LaneA a[64];
        LaneB b[64];
        uint64_t semi = 0, comma = 0, endm = 0, badm = 0;
        for (int l = 0; l < 64; ++l) {
            a[l] = lane_load(t, n, pos + l);
            semi |= (uint64_t)a[l].semi << l;
            comma |= (uint64_t)a[l].comma << l;
        }
        int64_t incl[64], run = 0;
        for (int l = 0; l < 64; ++l) {
            b[l] = lane_judge(t, n, pos, l, a[l], semi, comma, st);
            endm |= (uint64_t)b[l].end << l;
            run += b[l].end ? b[l].v + 1 : 0;
            incl[l] = run;
        }
        for (int l = 0; l < 64; ++l)
            badm |= (uint64_t)lane_store(t, pos, l, a[l], b[l], incl[l], incl[b[l].ls < 0 ? 0 : b[l].ls], semi, endm, st, ents, cap,
                                         groups)
                    << l;
        pass_advance(&st, pos, semi, comma, endm, incl[63], incl[semi ? high_bit(semi) : 0], badm != 0);
    }
    *n_groups = (int)(st.n_grp < kMaxGroups ? st.n_grp : kMaxGroups);
    *n_ent = st.ent_n;
    return pass_end(st, n);
}

static std::string valid_text(const std::string &seq, std::vector<int32_t> *ords) {
    static const char *heads[] = {"C+m", "C+h?", "C+mh.", "A+a", "N+n?", "U-e.", "G-76792", "T+21839?"};
    std::string t;
    const int ng = (int)(rnd() % 5);
    for (int g = 0; g < ng; ++g) {
        const char *h = heads[rnd() % 8];
        t += h;
        const int base = group_base((uint8_t)h[0]);
        int64_t have = 0;
        for (char c : seq) have += base == 4 || letter_class((uint8_t)c) == base;
        int64_t o = -1;
        const int want = (int)(rnd() % 4 == 0 ? 0 : rnd() % 90);
        for (int k = 0; k < want; ++k) {
            const int64_t d = rnd() % 3 == 0 ? rnd() % 40 : rnd() % 3;
            if (o + 1 + d >= have) break;
            o += 1 + d;
            char num[32];
            snprintf(num, sizeof num, rnd() % 9 == 0 ? ",%04lld" : ",%lld", (long long)d);
            t += num;
            ords->push_back((int32_t)o);
        }
        t += ';';
    }
    return t;
}

int main(int argc, char **argv) {
    g_state = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const long rounds = argc > 2 ? atol(argv[2]) : 1000;
    long usable_rounds = 0, parts_written = 0;
    for (long round = 0; round < rounds; ++round) {
        const int64_t l_seq = rnd() % 5 == 0 ? rnd() % 4 : rnd() % 700;
        std::string seq;
        for (int64_t i = 0; i < l_seq; ++i) seq += "ACGTACGTACGTNRYU"[rnd() % 16];
        std::vector<int32_t> ords;
        std::string text;
        const int mode = (int)(rnd() % 5);
        bool whole = false;
        if (mode == 0) {
            for (int k = (int)(rnd() % 300); k > 0; --k) text += (char)rnd();
        } else if (mode == 1) {
            for (int k = (int)(rnd() % 300); k > 0; --k) text += "ACGTUN+-mh.?,;0123456789"[rnd() % 24];
        } else {
            text = valid_text(seq, &ords);
            whole = mode != 2 || text.empty();
            if (!whole) text[rnd() % text.size()] = rnd() % 2 ? (char)rnd() : "ACN+-mh.?,;019"[rnd() % 14];
        }
        const int64_t n = (int64_t)text.size(), cap = ent_cap(n);
        Exact<uint8_t> t((size_t)n), s((size_t)l_seq);
        memcpy(t.p, text.data(), (size_t)n);
        memcpy(s.p, seq.data(), (size_t)l_seq);
        Exact<Ent> e1((size_t)cap), e2((size_t)cap);
        Group g1[kMaxGroups], g2[kMaxGroups];
        memset(g1, 0, sizeof g1);
        memset(g2, 0, sizeof g2);
        int ng1 = 0, ng2 = 0;
        int64_t ne2 = 0;
        const bool ok1 = parse(t.p, n, e1.p, cap, g1, &ng1);
        const bool ok2 = parse_wave(t.p, n, e2.p, cap, g2, &ng2, &ne2);
        CHECK(ok1 == ok2);
        if (ok1) {
            CHECK(ng1 == ng2 && memcmp(g1, g2, sizeof(Group) * (size_t)ng1) == 0);
            int64_t ne1 = ng1 ? g1[ng1 - 1].ent0 + g1[ng1 - 1].n_ent : 0;
            CHECK(ne1 == ne2 && memcmp(e1.p, e2.p, sizeof(Ent) * (size_t)ne1) == 0);
        }
        // ML values and the read's entry
        int64_t ml_vals = 0;
        if (ok1)
            for (int g = 0; g < ng1; ++g) ml_vals += (int64_t)g1[g].n_ent * g1[g].n_codes;
        const bool has_ml = rnd() % 3 != 0;
        const int64_t ml_len = has_ml ? (rnd() % 8 == 0 ? (int64_t)(rnd() % 50) : ml_vals) : 0;
        Exact<uint8_t> tags((size_t)(n + ml_len));
        memcpy(tags.p, t.p, (size_t)n);
        for (int64_t k = 0; k < ml_len; ++k) tags.p[n + k] = (uint8_t)rnd();
        pcabi_mods_read r;
        memset(&r, 0, sizeof r);
        r.l_seq = (int32_t)l_seq, r.mm_len = (int32_t)n, r.ml_off = n, r.ml_len = has_ml ? (int32_t)ml_len : -1;
        r.mn = rnd() % 2 ? -1 : (rnd() % 8 == 0 ? (int32_t)(rnd() % 700) : (int32_t)l_seq);
        r.flags = (int32_t)(rnd() % 16 == 0 ? PCABI_MODS_BAD : 0) | (rnd() % 2 ? PCABI_MODS_OLD_MM : 0) | (rnd() % 2 ? PCABI_MODS_OLD_ML : 0);
        ReadTables tb;
        const bool usable = read_tables(r, s.p, tags.p, e1.p, &tb);
        if (whole && !(r.flags & PCABI_MODS_BAD) && (!has_ml || ml_len == ml_vals) && (r.mn < 0 || r.mn == l_seq)) {
            CHECK(ok1 && usable);
            size_t k = 0;
            for (int g = 0; g < tb.n_groups; ++g)
                for (int j = 0; j < tb.groups[g].n_ent; ++j) CHECK(k < ords.size() && e1.p[tb.groups[g].ent0 + j].ord == ords[k++]);
            CHECK(k == ords.size());
        }
        if (!usable) continue;
        ++usable_rounds;
        // parts: random, and the edges
        for (int k = 0; k < 6; ++k) {
            int64_t s0 = l_seq ? rnd() % (l_seq + 1) : 0, ns = rnd() % (l_seq - s0 + 1);
            if (k == 0) s0 = 0, ns = l_seq;
            if (k == 1) ns = 0;
            int32_t c0[4], c1[4];
            count_to(s.p, s0, c0);
            count_to(s.p, s0 + ns, c1);
            const int64_t len = part_tags(r, tb, e1.p, tags.p, s0, ns, c0, c1, nullptr);
            Exact<uint8_t> a((size_t)len), b((size_t)len);
            memset(a.p, 0xA5, (size_t)len);
            memset(b.p, 0x5A, (size_t)len);
            CHECK(part_tags(r, tb, e1.p, tags.p, s0, ns, c0, c1, a.p) == len);
            // the kernel's order: spans and offsets first, then every lane's strided copies
            int64_t mm = 0, ml = 0, mm_at[kMaxGroups], ml_at[kMaxGroups];
            Span sp[kMaxGroups];
            for (int g = 0; g < tb.n_groups; ++g) {
                const Group &gr = tb.groups[g];
                sp[g] = group_span(gr, e1.p, r.mm_len, base_count(c0, gr.base, s0), base_count(c1, gr.base, s0 + ns));
                mm_at[g] = mm, ml_at[g] = ml;
                mm += sp[g].mm_bytes;
                ml += (int64_t)(sp[g].e1 - sp[g].e0) * gr.n_codes;
            }
            const int has = has_of(r);
            CHECK(tags_len(mm, ml, has) == len);
            for (int lane = 63; lane >= 0; --lane) {
                emit_fixed(b.p, mm, ml, has, (int32_t)ns, lane, 64);
                for (int g = 0; g < tb.n_groups; ++g)
                    emit_group(tb.groups[g], sp[g], tags.p, has_ml ? tags.p + n : nullptr, b.p + 3 + mm_at[g],
                               has_ml ? b.p + 3 + mm + 1 + 8 + ml_at[g] : nullptr, lane, 64);
            }
            CHECK(memcmp(a.p, b.p, (size_t)len) == 0);
            CHECK(pcabi_bam::aux_walks(a.p, len));
            ++parts_written;
        }
    }
    printf("rounds %ld usable %ld parts %ld\n", rounds, usable_rounds, parts_written);
    return 0;
}
