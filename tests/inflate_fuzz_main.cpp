// Stand-alone mutation run over the gzip decoder's host build (csrc/pcabi_inflate.h), meant to be
// compiled with -fsanitize=address,undefined and linked with zlib (tests/test_inflate_cpu.py does
// both). Usage: inflate_fuzz CORPUS SEED ITERATIONS [mutate-only]. CORPUS holds members as (uint32 length, bytes).
// Every mutation (bit flips, truncations, splices) is decoded from and into heap buffers of the
// exact size, and by zlib; a mutation that decodes must decode to what zlib gives, and a mutation
// that zlib decodes may be refused only as a bad code (PCABI_INFLATE_E_CODE: the decoder refuses a
// literal/length code of one single code, which zlib lets pass), never for any other reason.
// Exit 0 = all held. TEST INFRASTRUCTURE ONLY.
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../custom_porechop_abi_amd/csrc/pcabi_inflate.h"

using namespace pcabi_inflate;

static uint64_t g_state;
static uint32_t rnd() {   // xorshift64*
    g_state ^= g_state >> 12;
    g_state ^= g_state << 25;
    g_state ^= g_state >> 27;
    return (uint32_t)((g_state * 0x2545F4914F6CDD1DULL) >> 32);
}

// zlib on one gzip member: true and the bytes when it decodes, ends and uses all the input
static bool by_zlib(const std::vector<uint8_t> &z, std::vector<uint8_t> &out) {
    z_stream s{};
    if (inflateInit2(&s, 15 + 16) != Z_OK) return false;
    out.resize(kMemberMax + 1);
    s.next_in = const_cast<Bytef *>(z.data());
    s.avail_in = (uInt)z.size();
    s.next_out = out.data();
    s.avail_out = (uInt)out.size();
    const int rc = inflate(&s, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && s.avail_in == 0;
    out.resize(s.total_out);
    inflateEnd(&s);
    return ok;
}

int main(int argc, char **argv) {
    if (argc != 4 && argc != 5) return 2;
    const bool mutate_only = argc == 5;   // the corpus need not decode (damaged seeds)
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<std::vector<uint8_t>> corpus;
    uint32_t len;
    while (fread(&len, 4, 1, f) == 1) {
        std::vector<uint8_t> m(len);
        if (len && fread(m.data(), 1, len, f) != len) return 2;
        corpus.push_back(m);
    }
    fclose(f);
    if (corpus.empty()) return 2;
    g_state = 0x9E3779B97F4A7C15ULL ^ (uint64_t)atoll(argv[2]);
    const long iters = atol(argv[3]);
    long decoded = 0, refused = 0, stricter = 0;
    Tables *t = new Tables;
    for (long it = 0; it < iters; ++it) {
        std::vector<uint8_t> m = corpus[rnd() % corpus.size()];
        const uint32_t kind = !mutate_only && it < (long)corpus.size() ? 3 : rnd() % 3;   // the corpus itself first
        if (kind == 0 && !m.empty()) {
            const int flips = 1 + rnd() % 3;
            for (int k = 0; k < flips; ++k) m[rnd() % m.size()] ^= (uint8_t)(1u << (rnd() % 8));
        } else if (kind == 1) {
            m.resize(rnd() % (m.size() + 1));
        } else if (kind == 2) {
            const std::vector<uint8_t> &o = corpus[rnd() % corpus.size()];
            const size_t a = rnd() % (m.size() + 1), b = rnd() % (o.size() + 1);
            m.resize(a);
            m.insert(m.end(), o.begin() + b, o.end());
        } else {
            m = corpus[it];
        }
        // exact-size heap copies, so the sanitizer sees any access outside them
        uint8_t *z = (uint8_t *)malloc(m.size() ? m.size() : 1);
        for (size_t i = 0; i < m.size(); ++i) z[i] = m[i];
        const uint32_t isize = m.size() >= 4 ? le32(m.data() + m.size() - 4) : 0;
        const uint32_t cap = isize > (uint32_t)kMemberMax ? (uint32_t)kMemberMax : isize;
        uint8_t *out = (uint8_t *)malloc(cap ? cap : 1);
        SerialPar par;
        SerialSink sink{out};
        uint32_t n = 0;
        const int st = inflate_member(par, sink, *t, z, (int64_t)m.size(), cap, &n);
        if (st < 0 || st > PCABI_INFLATE_E_CRC) {
            fprintf(stderr, "iteration %ld: status %d\n", it, st);
            return 1;
        }
        if (st == 0) {
            std::vector<uint8_t> ref;
            const bool ok = by_zlib(m, ref);
            bool same = ok && ref.size() == n;
            for (uint32_t i = 0; same && i < n; ++i) same = ref[i] == out[i];
            if (!same) {
                fprintf(stderr, "iteration %ld (kind %u): decoded %u bytes, zlib %s %zu\n", it, kind, n,
                        ok ? "gives" : "refuses after", ref.size());
                return 1;
            }
            ++decoded;
        } else {
            if (kind == 3) {
                fprintf(stderr, "corpus member %ld refused with status %d\n", it, st);
                return 1;
            }
            std::vector<uint8_t> ref;
            if (by_zlib(m, ref) && ref.size() <= (size_t)kMemberMax) {
                if (st != PCABI_INFLATE_E_CODE) {
                    fprintf(stderr, "iteration %ld (kind %u): refused with status %d what zlib decodes (%zu bytes)\n", it,
                            kind, st, ref.size());
                    return 1;
                }
                ++stricter;
            }
            ++refused;
        }
        free(z);
        free(out);
    }
    delete t;
    printf("%ld decoded, %ld refused (%ld of them bad-code refusals of streams zlib decodes)\n", decoded, refused,
           stricter);
    return 0;
}
