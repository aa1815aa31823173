// Host build of the gap-extend-frame core's four-column pass (custom_porechop_abi_amd/csrc/
// pcabi_dp.h: align_lane_shift4, the cross-mode kernels' path for waves whose windows all have one
// length), driven by a host reader over the tile layout's dwords (codes 4 q .. 4 q + 3 in dword q,
// zero past the window's end), next to align_lane_shift on the same input. TEST-ONLY, as
// dp_model_shift.cpp.
#include <vector>

#include "../../custom_porechop_abi_amd/csrc/pcabi_dp.h"

static int dna5(unsigned char c) {
    switch (c) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2;
                 case 'T': case 't': case 'U': case 'u': return 3; default: return 4; }
}

// which = 0: align_lane_shift (a byte reader), 1: align_lane_shift4 (a tile-dword reader that fails
// the run, rc -4, on a dword the tile layout does not hold: index > ceil(n / 4) + 1)
template <int RPL>
static int run(int which, const char *read, int n, const char *adp, int L, pcabi::Scoring sc, int P, int B, int *out) {
    const int off = RPL - L;
    auto ad = [&](int s) { return s <= off ? pcabi::PAD_CODE : dna5((unsigned char)adp[s - off - 1]); };
    int32_t tab[pcabi::pk::TAB_W * RPL];
    for (int c = 0; c < pcabi::pk::TAB_W; ++c)
        for (int s = 1; s <= RPL; ++s) tab[c * RPL + s - 1] = pcabi::pk::sub_key_shift<RPL>(s, c, ad, off, sc);
    struct Row {
        const int32_t *p;
        int32_t operator()(int s) const { return p[s - 1]; }
        void quad(int q, int32_t *dst) const { for (int k = 0; k < 4; ++k) dst[k] = p[4 * q + k]; }
    };
    auto tabfn = [&](int rc) { return Row{tab + rc * RPL}; };
    pcabi::Result r;
    if (which == 0) {
        auto rd = [&](int j) { return j <= n ? dna5((unsigned char)read[j - 1]) : 4; };
        r = pcabi::align_lane_shift<RPL>(rd, n, tabfn, L, sc, P, B);
    } else {
        const int nq = (n + 3) / 4 + 2;
        std::vector<uint32_t> tile(nq, 0u);
        for (int k = 0; k < n; ++k) tile[k / 4] |= (uint32_t)dna5((unsigned char)read[k]) << (8 * (k & 3));
        bool oob = false;
        auto tr = [&](int q) {
            if (q < 0 || q >= nq) { oob = true; return 0u; }
            return tile[q];
        };
        r = pcabi::align_lane_shift4<RPL>(tr, n, tabfn, L, sc, P, B);
        if (oob) return -4;
    }
    out[0] = r.rs; out[1] = r.re; out[2] = r.as; out[3] = r.ae;
    out[4] = r.score; out[5] = r.m; out[6] = r.l1; out[7] = r.l2;
    return 0;
}

// Period `period` (the pass needs a multiple of 4) with the bias at the low end of shift_range's
// interval (which_bias = 0), the high end (1) or its centre (2: shift_ok's choice for that period).
// -3: shift_range declines the period for this adapter.
extern "C" int pcabi_model_shift4(int which, const char *read, int n, const char *adp, int L, int rpl, int period,
                                  int which_bias, int ma, int mi, int go, int ge, int *out) {
    pcabi::Scoring sc{ma, mi, go, ge};
    if (L <= 0 || n <= 0 || (period & 3) != 0) return -1;
    int blo, bhi;
    if (!pcabi::shift_range(L, rpl, sc, period, blo, bhi)) return -3;
    const int B = which_bias == 0 ? blo : (which_bias == 1 ? bhi : (blo + bhi) / 2);
    switch (rpl) {
#define C(R) case R: return run<R>(which, read, n, adp, L, sc, period, B, out);
    C(4) C(8) C(12) C(16) C(20) C(24) C(28) C(32)
#undef C
    default: return -2;
    }
}
