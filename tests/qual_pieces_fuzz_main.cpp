// qual_pieces_fuzz_main.cpp -- csrc/pcabi_pieces.h and csrc/pcabi_qual.h alone, as a program of their own for
// a sanitizer build (tests/test_qual_pieces_cpu.py): random ranges around a read in a block of exactly its
// size, the walk over the sorted ranges against a position-by-position marking, every piece cropped and
// summed inside its own bounds, and the new ranges played back as the writers read them.
// usage: qual_pieces_fuzz <seed> <rounds>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../custom_porechop_abi_amd/csrc/pcabi_pieces.h"
#include "../custom_porechop_abi_amd/csrc/pcabi_qual.h"

using namespace pcabi_qual;

struct Piece {
    int64_t b, e;
};

int main(int argc, char **argv) {
    srand(argc > 1 ? (unsigned)atoi(argv[1]) : 1u);
    const long rounds = argc > 2 ? atol(argv[2]) : 1000;
    for (long it = 0; it < rounds; ++it) {
        const int tl = rand() % 5 ? rand() % 400 : rand() % 4, m = rand() % 4 ? rand() % 13 : 300;
        const int W = rand() % (kMaxWindow + 1);
        uint8_t *q = (uint8_t *)malloc(tl ? (size_t)tl : 1);   // a read past either end of the read is a finding
        for (int k = 0; k < tl; ++k) q[k] = (uint8_t)(rand() % 3 ? 33 + rand() % 40 : rand());
        int64_t *cuts = (int64_t *)malloc(m ? sizeof(int64_t) * 2 * (size_t)m : 1);
        for (int k = 0; k < m; ++k) {
            const int64_t a = rand() % (tl + 60) - 30, n = rand() % 4 ? rand() % (m > 20 ? 3 : tl / 4 + 2) : -(rand() % 3);
            cuts[2 * k] = a, cuts[2 * k + 1] = a + n;
        }
        // the walk, over the ranges in (key, index) order
        std::vector<std::pair<int64_t, int64_t>> order;
        for (int k = 0; k < m; ++k) order.emplace_back(pcabi_pieces::sort_key(cuts[2 * k], tl), k);
        std::sort(order.begin(), order.end());
        std::vector<Piece> got;
        const int64_t n_got = pcabi_pieces::walk(
            tl, m,
            [&](int64_t j, int64_t *b, int64_t *e) {
                const int64_t k = order[(size_t)j].second;
                *b = cuts[2 * k], *e = cuts[2 * k + 1];
            },
            [&](int64_t j, int64_t b, int64_t e) {
                if (j != (int64_t)got.size()) printf("round %ld: piece %ld out of turn\n", it, (long)j), exit(1);
                got.push_back({b, e});
            });
        // the marking
        std::vector<char> cut((size_t)tl, 0);
        bool split = false;   // the writers' rule: one non-empty range
        for (int k = 0; k < m; ++k) split = split || cuts[2 * k + 1] > cuts[2 * k];
        for (int k = 0; k < m; ++k)
            for (int64_t p = std::max<int64_t>(cuts[2 * k], 0); p < std::min<int64_t>(cuts[2 * k + 1], tl); ++p) cut[(size_t)p] = 1;
        std::vector<Piece> want;
        for (int p = 0; split && p < tl; ++p)
            if (!cut[(size_t)p]) {
                if (p == 0 || cut[(size_t)p - 1]) want.push_back({p, p});
                want.back().e = p + 1;
            }
        bool same = n_got == (int64_t)want.size() && got.size() == want.size();
        for (size_t k = 0; same && k < want.size(); ++k) same = got[k].b == want[k].b && got[k].e == want[k].e;
        if (!same) {
            printf("round %ld: the pieces of tl = %d with %d ranges differ\n", it, tl, m);
            return 1;
        }
        // every piece as a span of its own; its two ranges lie inside it and leave the kept span
        const int64_t min_sum = rand() % (W * 30 + 1);
        for (const Piece &pc : got) {
            const int64_t n = pc.e - pc.b;
            pcabi_qual_read r{};
            r.kept = (int32_t)n;
            if (W > 0) {
                const int64_t vf = scan_host(q + pc.b, n, W, min_sum, false);
                crop_of(n, vf, vf < 0 ? 0 : scan_host(q + pc.b, n, W, min_sum, true), &r);
            }
            sum_lane(q, pc.b + r.front, pc.b + r.front + r.kept, 0, 1, err_of, &r.q_sum, &r.err_sum);
            int64_t want_q = 0;
            for (int64_t p = pc.b + r.front; p < pc.b + r.front + r.kept; ++p) want_q += phred(q[p]);
            const bool failed = rand() % 4 == 0;
            int64_t rg[4];
            pcabi_pieces::piece_ranges(pc.b, pc.e, r.front, r.tail, failed, rg);
            const int64_t left = (pc.e - pc.b) - std::max<int64_t>(rg[1] - rg[0], 0) - std::max<int64_t>(rg[3] - rg[2], 0);
            if (want_q != r.q_sum || rg[0] != pc.b || rg[3] != pc.e || rg[1] < rg[0] || rg[2] > rg[3] || rg[1] > rg[2] ||
                left != (failed ? 0 : r.kept)) {
                printf("round %ld: piece [%ld, %ld) of tl = %d, W = %d differs\n", it, (long)pc.b, (long)pc.e, tl, W);
                return 1;
            }
        }
        free(q);
        free(cuts);
    }
    printf("rounds %ld\n", rounds);
    return 0;
}
