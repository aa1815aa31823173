// Host build of the gap-extend-frame core (custom_porechop_abi_amd/csrc/pcabi_dp.h: pk::LayS,
// LaneShift, align_lane_shift, shift_ok) for CPU-side checks against oracle/. TEST-ONLY, as
// dp_model.cpp: the exact per-lane algorithm the cross-mode kernels run, without a GPU.
#include "../../custom_porechop_abi_amd/csrc/pcabi_dp.h"

static int dna5(unsigned char c) {
    switch (c) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2;
                 case 'T': case 't': case 'U': case 'u': return 3; default: return 4; }
}

template <int RPL>
static void run_shift(const char *read, int n, const char *adp, int L, pcabi::Scoring sc, int P, int B, int *out) {
    const int off = RPL - L;
    auto rd = [&](int j) { return j <= n ? dna5((unsigned char)read[j - 1]) : 4; };
    auto ad = [&](int s) { return s <= off ? pcabi::PAD_CODE : dna5((unsigned char)adp[s - off - 1]); };
    // c-major table, the layout the kernels keep in LDS: tab[c * RPL + s - 1]
    int32_t tab[pcabi::pk::TAB_W * RPL];
    for (int c = 0; c < pcabi::pk::TAB_W; ++c)
        for (int s = 1; s <= RPL; ++s) tab[c * RPL + s - 1] = pcabi::pk::sub_key_shift<RPL>(s, c, ad, off, sc);
    struct Row {
        const int32_t *p;
        int32_t operator()(int s) const { return p[s - 1]; }
        void quad(int q, int32_t *dst) const { for (int k = 0; k < 4; ++k) dst[k] = p[4 * q + k]; }
    };
    auto tabfn = [&](int rc) { return Row{tab + rc * RPL}; };
    const pcabi::Result r = pcabi::align_lane_shift<RPL>(rd, n, tabfn, L, sc, P, B);
    out[0] = r.rs; out[1] = r.re; out[2] = r.as; out[3] = r.ae;
    out[4] = r.score; out[5] = r.m; out[6] = r.l1; out[7] = r.l2;
}

// shift_ok: 1 and (*P, *B), or 0 when the bucket keeps LayT for this adapter
extern "C" int pcabi_model_shift_ok(int L, int rpl, int ma, int mi, int go, int ge, int *P, int *B) {
    return pcabi::shift_ok(L, rpl, pcabi::Scoring{ma, mi, go, ge}, *P, *B) ? 1 : 0;
}

// The core at an explicit register bucket; period <= 0: shift_ok's period and bias, else that
// period with the bias centred in its range (shift_range). -3: declined.
extern "C" int pcabi_model_align_shift(const char *read, int n, const char *adp, int L, int rpl, int period,
                                       int ma, int mi, int go, int ge, int *out) {
    pcabi::Scoring sc{ma, mi, go, ge};
    if (L <= 0 || n <= 0) return -1;
    int P = period, B = 0;
    if (period <= 0) {
        if (!pcabi::shift_ok(L, rpl, sc, P, B)) return -3;
    } else {
        int blo, bhi;
        if (!pcabi::shift_range(L, rpl, sc, P, blo, bhi)) return -3;
        B = (blo + bhi) / 2;
    }
    switch (rpl) {
#define C(R) case R: run_shift<R>(read, n, adp, L, sc, P, B, out); break;
    C(4) C(8) C(12) C(16) C(20) C(24) C(28) C(32)
#undef C
    default: return -2;
    }
    return 0;
}

// The extremes of the bias range (which = 0: lowest, 1: highest): every bias shift_range allows
// must give the same results.
extern "C" int pcabi_model_align_shift_bias(const char *read, int n, const char *adp, int L, int rpl, int period,
                                            int which, int ma, int mi, int go, int ge, int *out) {
    pcabi::Scoring sc{ma, mi, go, ge};
    if (L <= 0 || n <= 0) return -1;
    int blo, bhi;
    if (!pcabi::shift_range(L, rpl, sc, period, blo, bhi)) return -3;
    const int B = which ? bhi : blo;
    switch (rpl) {
#define C(R) case R: run_shift<R>(read, n, adp, L, sc, period, B, out); break;
    C(4) C(8) C(12) C(16) C(20) C(24) C(28) C(32)
#undef C
    default: return -2;
    }
    return 0;
}
