// qual_fuzz_main.cpp -- csrc/pcabi_qual.h alone, as a program of its own for a sanitizer build
// (tests/test_qual_cpu.py): random spans in blocks of exactly their size, the two scans against every
// window summed on its own, and sum_lane dealt to 1..64 lanes against the byte-by-byte sums.
// usage: qual_fuzz <seed> <rounds>
#include <cstdio>
#include <cstdlib>

#include "../custom_porechop_abi_amd/csrc/pcabi_qual.h"

using namespace pcabi_qual;

int main(int argc, char **argv) {
    srand(argc > 1 ? (unsigned)atoi(argv[1]) : 1u);
    const long rounds = argc > 2 ? atol(argv[2]) : 1000;
    for (long it = 0; it < rounds; ++it) {
        const int n = rand() % 300, W = 1 + rand() % kMaxWindow;
        uint8_t *q = (uint8_t *)malloc(n ? (size_t)n : 1);   // a read past either end of the span is a finding
        for (int k = 0; k < n; ++k) q[k] = (uint8_t)(rand() % 3 ? 33 + rand() % 40 : rand());
        const int64_t min_sum = rand() % (W * 30 + 1);
        const int64_t vf = scan_host(q, n, W, min_sum, false), vt = vf < 0 ? 0 : scan_host(q, n, W, min_sum, true);
        pcabi_qual_read r{};
        crop_of(n, vf, vt, &r);
        int64_t f = -1, g = -1;
        for (int p = 0; p + W <= n; ++p) {
            int64_t s = 0;
            for (int k = 0; k < W; ++k) s += phred(q[p + k]);
            if (s >= min_sum) g = p, f = f < 0 ? p : f;
        }
        if (r.front != (f < 0 ? n : f) || r.tail != (f < 0 ? 0 : n - (g + W)) || r.kept != n - r.front - r.tail) {
            printf("round %ld: the crop of n = %d, W = %d differs\n", it, n, W);
            return 1;
        }
        const int n_lanes = 1 + rand() % 64;
        int64_t q_sum = 0, q_want = 0;
        uint64_t err_sum = 0, err_want = 0;
        for (int lane = 0; lane < n_lanes; ++lane) sum_lane(q, r.front, (int64_t)r.front + r.kept, lane, n_lanes, err_of, &q_sum, &err_sum);
        for (int k = r.front; k < r.front + r.kept; ++k) q_want += phred(q[k]), err_want += err_of(phred(q[k]));
        if (q_sum != q_want || err_sum != err_want) {
            printf("round %ld: the sums of n = %d over %d lanes differ\n", it, n, n_lanes);
            return 1;
        }
        free(q);
    }
    printf("rounds %ld\n", rounds);
    return 0;
}
