/* pid6_ties: which (matches, length) pairs reach pid6's tie correction (csrc/pcabi_dp.h)?
 *
 * pid6 rounds d * 1e6 (d = 100.0 * m / l) to an integer, half-even on the EXACT product. The
 * double product p = d * 1e6 can land exactly on k + 0.5 while the exact product lies beside it
 * (e = fma(d, 1e6, -p) != 0); then rint(p) picks the even neighbour and the correction moves it
 * to the side e points to. This program enumerates 0 <= m <= l <= LIMIT and prints those pairs,
 * with the count per length and the total (DESIGN.md section 2 records them).
 *
 *   cc -O2 -ffp-contract=off -fopenmp -o pid6_ties tools/pid6_ties.c -lm
 *   ./pid6_ties [LIMIT]            (default 131072 = 2^17; about 8.6e9 pairs)
 *
 * -ffp-contract=off matters: a compiler that fuses p into a later subtraction never sees the tie.
 * Not part of the test suite. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

/* 0 = no correction; +1 / -1 = rint(p) moved up / down by one */
static int tie_correction(int m, int l, double *out) {
    const double d = (100.0 * (double)m) / (double)l;
    const double p = d * 1e6;
    const double e = fma(d, 1e6, -p);
    double k = rint(p);
    const double f = p - k;
    int c = 0;
    if (f == 0.5 && e > 0.0) c = 1;
    else if (f == -0.5 && e < 0.0) c = -1;
    *out = (k + c) / 1e6;
    return c;
}

int main(int argc, char **argv) {
    const long limit = argc > 1 ? atol(argv[1]) : 131072;
    if (limit < 1 || limit > 2147483647L) {
        fprintf(stderr, "usage: pid6_ties [LIMIT >= 1]\n");
        return 2;
    }
    long *cnt = calloc((size_t)limit + 1, sizeof(long));
    if (!cnt) return 1;
#pragma omp parallel for schedule(dynamic, 64)
    for (long l = 1; l <= limit; ++l) {
        long c = 0;
        double v;
        for (long m = 0; m <= l; ++m) c += tie_correction((int)m, (int)l, &v) != 0;
        cnt[l] = c;
    }
    long total = 0, up = 0, families = 0;
    for (long l = 1; l <= limit; ++l) {
        if (!cnt[l]) continue;
        ++families;
        for (long m = 0; m <= l; ++m) {
            double v;
            const int c = tie_correction((int)m, (int)l, &v);
            if (!c) continue;
            printf("%ld %ld %+d %.6f\n", m, l, c, v);
            up += c > 0;
        }
        total += cnt[l];
    }
    for (long l = 1; l <= limit; ++l)
        if (cnt[l]) printf("# l = %ld: %ld pairs\n", l, cnt[l]);
    printf("# limit %ld: %ld pairs (%ld up, %ld down) in %ld lengths\n", limit, total, up, total - up, families);
    free(cnt);
    return 0;
}
