/*
 * path_oracle.c -- TEST INFRASTRUCTURE ONLY: the gapped rows the CPU oracle's row builder makes
 * (oracle/pcabi_oracle.c build_rows, whose summary fields tests/test_oracle_golden.py pins to the
 * reference's own output), copied out for the alignment-path tests. Built on demand by
 * tests/path_oracle_lib.py.
 */
#include "../oracle/pcabi_oracle.c"

/* Returns the row length (0 for an empty input); rr / ar receive min(length, cap) characters. */
int pcabi_path_oracle_rows(const char *read, int n, const char *adapter, int l, int ma, int mi, int go, int ge,
                           char *rr_out, char *ar_out, int cap) {
    char *rr, *ar;
    int score;
    const int len = build_rows(read, n, adapter, l, ma, mi, go, ge, 0, &rr, &ar, &score);
    if (len > 0) {
        memcpy(rr_out, rr, (size_t)(len < cap ? len : cap));
        memcpy(ar_out, ar, (size_t)(len < cap ? len : cap));
    }
    free(rr);
    free(ar);
    return len;
}
