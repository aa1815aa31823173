// bam_fuzz_main.cpp -- csrc/pcabi_bam.h alone, as a program of its own, for a sanitizer build
// (tests/test_bam_cpu.py builds it with -fsanitize=address,undefined and runs it as a child process).
// TEST INFRASTRUCTURE ONLY.
//
// usage: bam_fuzz <inflated BAM file> <seed> <mutations>
// Every mutation of the file's bytes lives in a heap block of exactly its size; the header skip and
// the record walk run over it, then every record the walk accepted is unpacked -- whole, and again in
// the kernel's 16-byte destination pieces at every output misalignment -- into buffers sized exactly
// from the table. The two unpacks must agree. The unmutated file goes first and must be accepted whole.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../custom_porechop_abi_amd/csrc/pcabi_bam.h"

using namespace pcabi_bam;

static uint64_t g_state;
static uint32_t rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33);
}

// returns the number of records unpacked, -1 when the header or the chain is refused
static long run(const uint8_t *src, size_t n, int shift) {
    uint8_t *b = new uint8_t[n ? n : 1];
    memcpy(b, src, n);
    long done = -1;
    const int64_t h = header_len(b, (int64_t)n);
    if (h > 0) {
        Layout count;
        int64_t stop = 0;
        const int64_t kept = walk(b, (int64_t)n, h, nullptr, 0, &count, &stop);
        // an invalid record stops the walk; what came before it was accepted and is unpacked
        Layout lay;
        const int64_t upto = stop;
        std::vector<pcabi_bam_rec> recs((size_t)(kept < 0 ? 0 : kept));
        int64_t n_recs = kept;
        if (kept < 0) {   // walk again over the accepted prefix
            Layout tmp;
            int64_t s2 = 0;
            n_recs = walk(b, upto, h, nullptr, 0, &tmp, &s2);
            if (n_recs < 0) abort();
            recs.resize((size_t)n_recs);
        }
        int64_t s3 = 0;
        if (walk(b, upto, h, recs.data(), n_recs, &lay, &s3) != n_recs) abort();
        // exact-size outputs; the piecewise copies start `shift` bytes into a 16-aligned block
        uint8_t *seq = new uint8_t[(size_t)lay.seq ? (size_t)lay.seq : 1], *qual = new uint8_t[(size_t)lay.seq ? (size_t)lay.seq : 1],
                *codes = new uint8_t[(size_t)lay.code ? (size_t)lay.code : 1];
        uint8_t *raw2[3];
        uint8_t *out2[3];
        const size_t sizes[3] = {(size_t)lay.seq, (size_t)lay.seq, (size_t)lay.code};
        for (int o = 0; o < 3; ++o) {
            raw2[o] = (uint8_t *)aligned_alloc(16, ((sizes[o] + (size_t)shift + 15) / 16 + 1) * 16);
            out2[o] = raw2[o] + shift;
        }
        for (const pcabi_bam_rec &r : recs) {
            if (!rec_fits(r, (int64_t)n, lay.seq, lay.seq, lay.code)) abort();
            const uint8_t *sq = b + r.rec + r.seq_at;
            unpack_range(sq, r.l_seq, r.flag, 0, r.l_seq, seq + r.seq_out, qual + r.qual_out, codes + r.code_out);
            uint8_t *dst[3] = {out2[0] + r.seq_out, out2[1] + r.qual_out, out2[2] + r.code_out};
            for (int o = 0; o < 3; ++o) {
                const int64_t d = (int64_t)(uintptr_t)dst[o], a = d & ~(int64_t)15;
                for (int64_t p0 = a - d; p0 < r.l_seq; p0 += 16)
                    unpack_range(sq, r.l_seq, r.flag, p0 > 0 ? p0 : 0, p0 + 16 < r.l_seq ? p0 + 16 : r.l_seq, o == 0 ? dst[0] : nullptr,
                                 o == 1 ? dst[1] : nullptr, o == 2 ? dst[2] : nullptr);
            }
        }
        if (memcmp(seq, out2[0], sizes[0]) || memcmp(qual, out2[1], sizes[1]) || memcmp(codes, out2[2], sizes[2])) {
            fprintf(stderr, "piecewise unpack differs from the whole-record unpack\n");
            abort();
        }
        for (int o = 0; o < 3; ++o) free(raw2[o]);
        delete[] seq;
        delete[] qual;
        delete[] codes;
        done = kept < 0 ? -1 : (stop == (int64_t)n ? (long)n_recs : -1);
    }
    delete[] b;
    return done;
}

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> file;
    uint8_t buf[4096];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) file.insert(file.end(), buf, buf + k);
    fclose(f);
    g_state = strtoull(argv[2], nullptr, 10) * 2654435761ull + 1;
    const long count = atol(argv[3]);
    long whole = 0;
    for (int shift = 0; shift < 16; ++shift) {
        const long got = run(file.data(), file.size(), shift);
        if (got <= 0) {
            fprintf(stderr, "the unmutated file was refused\n");
            return 1;
        }
        whole = got;
    }
    static const int32_t kValues[] = {0, 1, 2, 31, 32, 33, -1, -2, 255, 256, 65535, 65536, 0x7fffffff, (int32_t)0x80000000};
    long accepted = 0;
    for (long m = 0; m < count; ++m) {
        std::vector<uint8_t> x = file;
        if (rnd() % 8 == 0) x.resize(rnd() % (x.size() + 1));   // cut
        const int edits = 1 + (int)(rnd() % 3);
        for (int e = 0; e < edits && !x.empty(); ++e) {
            const size_t at = rnd() % x.size();
            switch (rnd() % 4) {
            case 0: x[at] = (uint8_t)rnd(); break;
            case 1: x[at] = (uint8_t)(x[at] + (rnd() & 1 ? 1 : -1)); break;
            case 2: x[at] ^= (uint8_t)(1u << (rnd() % 8)); break;
            default: {
                const int32_t v = kValues[rnd() % (sizeof kValues / sizeof kValues[0])];
                for (size_t k = 0; k < 4 && at + k < x.size(); ++k) x[at + k] = (uint8_t)((uint32_t)v >> (8 * k));
            }
            }
        }
        if (run(x.data(), x.size(), (int)(rnd() % 16)) >= 0) ++accepted;
    }
    printf("records %ld, mutations %ld, accepted whole %ld\n", whole, count, accepted);
    return 0;
}
