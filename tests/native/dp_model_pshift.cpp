// Host build of the packed buckets' gap-extend-frame core (custom_porechop_abi_amd/csrc/pcabi_dp.h:
// LanePShift, align_lane_pshift, pshift_range, pshift_bucket) for CPU-side checks against oracle/.
// TEST-ONLY, as dp_model.cpp: the exact per-lane algorithm the cross-mode kernels run, without a GPU.
#include "../../custom_porechop_abi_amd/csrc/pcabi_dp.h"

static int dna5(unsigned char c) {
    switch (c) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2;
                 case 'T': case 't': case 'U': case 'u': return 3; default: return 4; }
}

template <int RPL>
static void run_pshift(const char *read, int n, const char *adp, int L, pcabi::Scoring sc, int P, int B, int *out) {
    const int off = RPL - L;
    auto rd = [&](int j) { return j <= n ? dna5((unsigned char)read[j - 1]) : 4; };
    auto ad = [&](int s) { return s <= off ? pcabi::PAD_CODE : dna5((unsigned char)adp[s - off - 1]); };
    // c-major table, the layout the kernels keep in LDS: tab[c * RPL + s - 1]
    int32_t tab[pcabi::pk::TAB_W * RPL];
    for (int c = 0; c < pcabi::pk::TAB_W; ++c)
        for (int s = 1; s <= RPL; ++s) tab[c * RPL + s - 1] = pcabi::pk::sub_key_pshift<RPL>(s, c, ad, off, sc);
    struct Row {
        const int32_t *p;
        int32_t operator()(int s) const { return p[s - 1]; }
        void quad(int q, int32_t *dst) const { for (int k = 0; k < 4; ++k) dst[k] = p[4 * q + k]; }
    };
    auto tabfn = [&](int rc) { return Row{tab + rc * RPL}; };
    const pcabi::Result r = pcabi::align_lane_pshift<RPL>(rd, n, tabfn, L, sc, P, B);
    out[0] = r.rs; out[1] = r.re; out[2] = r.as; out[3] = r.ae;
    out[4] = r.score; out[5] = r.m; out[6] = r.l1; out[7] = r.l2;
}

static int run(const char *read, int n, const char *adp, int L, int rpl, pcabi::Scoring sc, int P, int B, int *out) {
    switch (rpl) {
#define C(R) case R: run_pshift<R>(read, n, adp, L, sc, P, B, out); break;
    C(36) C(40) C(44) C(48) C(52) C(56) C(60) C(64)
#undef C
    default: return -2;
    }
    return 0;
}

// pshift_range at one period: 1 and the bias range, or 0
extern "C" int pcabi_model_pshift_range(int L, int rpl, int period, int ma, int mi, int go, int ge, int *blo,
                                        int *bhi) {
    return pcabi::pshift_range(L, rpl, pcabi::Scoring{ma, mi, go, ge}, period, *blo, *bhi) ? 1 : 0;
}

// pshift_bucket: the period and bias the engine picks for a bucket holding these adapter lengths
// (or for one adapter alone); 0 when the bucket keeps Lay
extern "C" int pcabi_model_pshift_bucket(const int32_t *lens, int n_adp, int rpl, int ma, int mi, int go, int ge,
                                         int *P, int *B) {
    return pcabi::pshift_bucket(lens, n_adp, rpl, pcabi::Scoring{ma, mi, go, ge}, *P, *B) ? 1 : 0;
}

// The core at an explicit register bucket; period <= 0: pshift_bucket's period for this adapter, else that
// (forced, smaller) period. which: 0 the lowest bias of the range, 1 the highest, else the middle.
// -3: declined.
extern "C" int pcabi_model_align_pshift(const char *read, int n, const char *adp, int L, int rpl, int period,
                                        int which, int ma, int mi, int go, int ge, int *out) {
    pcabi::Scoring sc{ma, mi, go, ge};
    if (L <= 0 || n <= 0) return -1;
    int P = period, B = 0;
    const int32_t len = L;
    if (period <= 0 && !pcabi::pshift_bucket(&len, 1, rpl, sc, P, B)) return -3;
    int blo, bhi;
    if (!pcabi::pshift_range(L, rpl, sc, P, blo, bhi)) return -3;
    B = which == 0 ? blo : (which == 1 ? bhi : blo + (bhi - blo) / 2);
    return run(read, n, adp, L, rpl, sc, P, B, out);
}
