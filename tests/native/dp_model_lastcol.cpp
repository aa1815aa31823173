// Host build of the gap-extend-frame cores (custom_porechop_abi_amd/csrc/pcabi_dp.h:
// align_lane_shift, align_lane_shift4, align_lane_pshift) next to align_lane_packed on the same
// layout (LayT for the buckets of 4..32 rows, Lay for 36..64), which keeps LanePacked's last column
// with the full best-cell bookkeeping: the frame cores' own last column (LaneShift::last_column,
// LanePShift::last_column) must report the same end cell, type and attributes. TEST-ONLY, as
// dp_model_shift4.cpp.
#include <vector>

#include "../../custom_porechop_abi_amd/csrc/pcabi_dp.h"

static int dna5(unsigned char c) {
    switch (c) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2;
                 case 'T': case 't': case 'U': case 'u': return 3; default: return 4; }
}

struct Row {
    const int32_t *p;
    int32_t operator()(int s) const { return p[s - 1]; }
    void quad(int q, int32_t *dst) const { for (int k = 0; k < 4; ++k) dst[k] = p[4 * q + k]; }
};

static void put(const pcabi::Result &r, int *out) {
    out[0] = r.rs; out[1] = r.re; out[2] = r.as; out[3] = r.ae;
    out[4] = r.score; out[5] = r.m; out[6] = r.l1; out[7] = r.l2; out[8] = r.diag_en;
}

static bool same(const pcabi::Result &a, const pcabi::Result &b) {
    return a.rs == b.rs && a.re == b.re && a.as == b.as && a.ae == b.ae && a.score == b.score && a.m == b.m &&
           a.l1 == b.l1 && a.l2 == b.l2 && a.diag_en == b.diag_en;
}

// One window against one adapter in bucket RPL: the packed core with LanePacked's last column into
// out[0..8] (the 8 fields and diag_en), then every period of `periods` the range function accepts at
// both ends of its bias range -- align_lane_shift and, where the period is a multiple of 4,
// align_lane_shift4 (RPL <= 32), or align_lane_pshift (RPL >= 36) -- each compared with it in all 9.
// *ran: bit k set when periods[k] ran. 0: all agree; 1 + 8 k + 2 core + bias: the first run that
// differs (its result in bad[0..8]); -4: the tile reader left the tile.
template <int RPL>
static int run(const char *read, int n, const char *adp, int L, pcabi::Scoring sc, const int *periods, int n_periods,
               int *out, int *bad, int *ran) {
    constexpr bool SMALL = RPL <= 32;
    const int off = RPL - L;
    auto ad = [&](int s) { return s <= off ? pcabi::PAD_CODE : dna5((unsigned char)adp[s - off - 1]); };
    auto rd = [&](int j) { return j <= n ? dna5((unsigned char)read[j - 1]) : 4; };
    using YOld = typename std::conditional<SMALL, pcabi::pk::LayT<RPL>, pcabi::pk::Lay<RPL>>::type;
    int32_t tab_old[pcabi::pk::TAB_W * RPL], tab[pcabi::pk::TAB_W * RPL];
    for (int c = 0; c < pcabi::pk::TAB_W; ++c)
        for (int s = 1; s <= RPL; ++s) {
            tab_old[c * RPL + s - 1] = pcabi::pk::sub_key<RPL, decltype(ad), YOld>(s, c, ad, off, sc);
            if constexpr (SMALL) tab[c * RPL + s - 1] = pcabi::pk::sub_key_shift<RPL>(s, c, ad, off, sc);
            else tab[c * RPL + s - 1] = pcabi::pk::sub_key_pshift<RPL>(s, c, ad, off, sc);
        }
    auto tabfn_old = [&](int rc) { return Row{tab_old + rc * RPL}; };
    auto tabfn = [&](int rc) { return Row{tab + rc * RPL}; };
    const pcabi::Result old = pcabi::align_lane_packed<RPL, true, false, YOld>(rd, n, tabfn_old, L, sc);
    put(old, out);
    const int nq = (n + 3) / 4 + 2;
    std::vector<uint32_t> tile(nq, 0u);
    for (int k = 0; k < n; ++k) tile[k / 4] |= (uint32_t)dna5((unsigned char)read[k]) << (8 * (k & 3));
    *ran = 0;
    for (int k = 0; k < n_periods; ++k) {
        const int P = periods[k];
        int blo, bhi;
        if constexpr (SMALL) { if (!pcabi::shift_range(L, RPL, sc, P, blo, bhi)) continue; }
        else { if (!pcabi::pshift_range(L, RPL, sc, P, blo, bhi)) continue; }
        *ran |= 1 << k;
        for (int wb = 0; wb < 2; ++wb) {
            const int B = wb ? bhi : blo;
            if constexpr (SMALL) {
                const pcabi::Result r1 = pcabi::align_lane_shift<RPL>(rd, n, tabfn, L, sc, P, B);
                if (!same(r1, old)) { put(r1, bad); return 1 + 8 * k + wb; }
                if ((P & 3) == 0) {
                    bool oob = false;
                    auto tr = [&](int q) {
                        if (q < 0 || q >= nq) { oob = true; return 0u; }
                        return tile[q];
                    };
                    const pcabi::Result r4 = pcabi::align_lane_shift4<RPL>(tr, n, tabfn, L, sc, P, B);
                    if (oob) return -4;
                    if (!same(r4, old)) { put(r4, bad); return 1 + 8 * k + 2 + wb; }
                }
            } else {
                const pcabi::Result r2 = pcabi::align_lane_pshift<RPL>(rd, n, tabfn, L, sc, P, B);
                if (!same(r2, old)) { put(r2, bad); return 1 + 8 * k + 4 + wb; }
            }
        }
    }
    return 0;
}

// -1: bad arguments, -2: no such bucket, -3: the layout's own range check (layt_ok / packed_ok)
// declines the adapter, so no core of this bucket runs it.
extern "C" int pcabi_model_lastcol(const char *read, int n, const char *adp, int L, int rpl, int ma, int mi, int go,
                                   int ge, const int *periods, int n_periods, int *out, int *bad, int *ran) {
    pcabi::Scoring sc{ma, mi, go, ge};
    if (L <= 0 || n <= 0 || L > rpl || n_periods > 30) return -1;
    *ran = 0;
    if (rpl <= 32 ? !pcabi::layt_ok(L, rpl, sc) : (go == ge || !pcabi::packed_ok(L, rpl, sc))) return -3;
    switch (rpl) {
#define C(R) case R: return run<R>(read, n, adp, L, sc, periods, n_periods, out, bad, ran);
    C(4) C(8) C(12) C(16) C(20) C(24) C(28) C(32) C(36) C(40) C(44) C(48) C(52) C(56) C(60) C(64)
#undef C
    default: return -2;
    }
}

// Which of `periods` the bucket's range function accepts for an adapter of L bases (bit k).
extern "C" int pcabi_model_lastcol_periods(int L, int rpl, int ma, int mi, int go, int ge, const int *periods,
                                           int n_periods) {
    pcabi::Scoring sc{ma, mi, go, ge};
    int m = 0, blo, bhi;
    for (int k = 0; k < n_periods; ++k)
        if (rpl <= 32 ? pcabi::shift_range(L, rpl, sc, periods[k], blo, bhi)
                      : pcabi::pshift_range(L, rpl, sc, periods[k], blo, bhi)) m |= 1 << k;
    return m;
}
