// Stand-alone mutation run over the parallel gzip stream decoder's host build (csrc/pcabi_gzstream.h
// over the serial backend), meant to be compiled with -fsanitize=address,undefined and linked with
// zlib (tests/test_gzstream_cpu.py does both). Usage: gzstream_fuzz CORPUS SEED ITERATIONS. CORPUS
// holds gzip streams as (uint32 length, bytes). Every seed is decoded as it is; then seeded mutations
// (bit flips in headers and payloads, truncation at every one of the last 64 bytes, swapped trailers,
// spliced and appended members) are decoded from heap buffers of the exact size, with small chunks
// and spans, on the chain and through the fallback, and by zlib member after member as gzread reads
// them. The two must agree on accept or reject, and on the bytes where both accept.
// Exit 0 = all held. TEST INFRASTRUCTURE ONLY.
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../custom_porechop_abi_amd/csrc/pcabi_gzstream.h"

using namespace pcabi_gzstream;

static uint64_t g_state;
static uint32_t rnd() {   // xorshift64*
    g_state ^= g_state >> 12;
    g_state ^= g_state << 25;
    g_state ^= g_state >> 27;
    return (uint32_t)((g_state * 0x2545F4914F6CDD1DULL) >> 32);
}

// zlib on a whole stream, member after member: bytes after a member that do not start with the
// magic are ignored; anything else that is no sound member is refused
static bool by_zlib(const std::vector<uint8_t> &z, std::vector<uint8_t> &out) {
    out.clear();
    size_t pos = 0;
    bool first = true;
    std::vector<uint8_t> buf(1 << 16);
    while (pos < z.size()) {
        if (!(z.size() - pos >= 2 && z[pos] == 0x1f && z[pos + 1] == 0x8b)) return !first;
        z_stream s{};
        if (inflateInit2(&s, 15 + 16) != Z_OK) return false;
        s.next_in = const_cast<Bytef *>(z.data() + pos);
        s.avail_in = (uInt)(z.size() - pos);
        int rc = Z_OK;
        while (rc == Z_OK) {
            s.next_out = buf.data();
            s.avail_out = (uInt)buf.size();
            rc = inflate(&s, Z_NO_FLUSH);
            out.insert(out.end(), buf.data(), buf.data() + (buf.size() - s.avail_out));
            if (rc == Z_OK && s.avail_in == 0 && s.avail_out != 0) rc = Z_BUF_ERROR;   // the input ends early
        }
        pos = z.size() - s.avail_in;
        inflateEnd(&s);
        if (rc != Z_STREAM_END) return false;
        first = false;
    }
    return true;
}

static bool by_ours(const std::vector<uint8_t> &z, const Tune &tune, std::vector<uint8_t> &out) {
    // the stream in a heap block of its exact size, so that a read past either end is caught
    uint8_t *copy = (uint8_t *)malloc(z.size() ? z.size() : 1);
    if (!z.empty()) memcpy(copy, z.data(), z.size());
    SerialBackend be;
    GzStream<SerialBackend> s(copy, (int64_t)z.size(), tune, be);
    out.clear();
    int rc;
    while ((rc = s.next(out)) > 0) {
    }
    free(copy);
    return rc == 0;
}

int main(int argc, char **argv) {
    if (argc != 4) return 2;
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
    long accepted = 0, refused = 0;
    static const int64_t chunks[] = {512, 1024, 4096}, spans[] = {8192, 65536, 1 << 20};
    std::vector<uint8_t> a, b;
    for (long it = 0; it < iters; ++it) {
        std::vector<uint8_t> z = corpus[it < (long)corpus.size() ? (size_t)it : rnd() % corpus.size()];
        const char *what = "seed";
        if (it >= (long)corpus.size() && !z.empty()) {
            const size_t n = z.size();
            switch (rnd() % 8) {
            case 0:   // bit flips in the header
                what = "header flip";
                z[rnd() % (n < 24 ? n : 24)] ^= (uint8_t)(1u << (rnd() % 8));
                break;
            case 1:   // bit flips in the payload
            case 2:
                what = "payload flip";
                for (int k = 1 + (int)(rnd() % 3); k > 0; --k) z[rnd() % n] ^= (uint8_t)(1u << (rnd() % 8));
                break;
            case 3:   // truncation at every one of the last 64 bytes, in turn
                what = "truncation";
                z.resize(n - 1 - (size_t)(it % 64) % n);
                break;
            case 4: {   // the trailer of another seed
                what = "swapped trailer";
                const std::vector<uint8_t> &o = corpus[rnd() % corpus.size()];
                if (n >= 8 && o.size() >= 8) memcpy(z.data() + n - 8, o.data() + o.size() - 8, 8);
                break;
            }
            case 5: {   // another seed appended: one more member, or more
                what = "appended";
                const std::vector<uint8_t> &o = corpus[rnd() % corpus.size()];
                z.insert(z.end(), o.begin(), o.end());
                if (rnd() % 2) z[n + rnd() % 12] ^= (uint8_t)(1u << (rnd() % 8));
                break;
            }
            case 6:   // bytes after the last member
                what = "trailing bytes";
                for (int k = 1 + (int)(rnd() % 40); k > 0; --k) z.push_back((uint8_t)(rnd() % 4 ? 0 : rnd()));
                break;
            default: {   // a run of bytes overwritten
                what = "overwritten run";
                const size_t at = rnd() % n, k = 1 + rnd() % 16;
                for (size_t i = at; i < n && i < at + k; ++i) z[i] = (uint8_t)rnd();
                break;
            }
            }
        }
        const Tune tune{chunks[rnd() % 3], spans[rnd() % 3], (rnd() % 4) ? 1 : (int64_t)1 << 40};
        const bool ok_z = by_zlib(z, a), ok_o = by_ours(z, tune, b);
        if (ok_z != ok_o || (ok_z && a != b)) {
            fprintf(stderr, "iteration %ld (%s, %zu bytes, chunk %lld span %lld min %lld): zlib %s, decoder %s%s\n", it, what,
                    z.size(), (long long)tune.chunk_bytes, (long long)tune.span_bytes, (long long)tune.min_chunks,
                    ok_z ? "accepts" : "refuses", ok_o ? "accepts" : "refuses", ok_z && ok_o ? ", other bytes" : "");
            return 1;
        }
        if (it < (long)corpus.size() && !ok_z) {
            fprintf(stderr, "seed %ld does not decode\n", it);
            return 1;
        }
        ++(ok_z ? accepted : refused);
    }
    printf("%ld accepted, %ld refused\n", accepted, refused);
    return 0;
}
