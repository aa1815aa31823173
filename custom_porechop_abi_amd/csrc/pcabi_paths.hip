// pcabi_paths.hip -- alignment paths and per-position adapter profiles (include/pcabi.h,
// pcabi_align_paths_* / pcabi_adapter_profile_*; DESIGN.md §4 "Alignment paths").
//
// The attribute cores (pcabi_dp.h) never keep a trace; this unit is the one place that does. For one
// (window, adapter) pair it produces the columns of the gapped rows SeqAn's globalAlignment(...,
// AlignConfig<1,1,1,1>) leaves in Align -- head free-gap columns, the GapsLeft traceback path, tail
// free-gap columns (S/align/dp_traceback_impl.h:197-370, 379-455, 497-548) -- as run-length encoded
// ops, and the ScoredAlignment fields (porechop_abi/src/alignment.cpp:6-110) computed from those very
// columns.
//
//   k_paths<AFFINE>   one wavefront per pair. Lane l owns adapter rows 2l + 1 and 2l + 2 (up to 128
//                     rows); the lanes run as a systolic pipeline over the read columns: at step t
//                     lane l computes column t - l + 1 from what lane l - 1 computed at step t - 1,
//                     received by one DPP wavefront shift (wave_shr:1; lane 0 takes row 0 instead).
//                     The read base travels down the lanes the same way. Every cell's trace byte
//                     (the TraceBitMap_ roles D, H, H-open, V, V-open, max-from-V, max-from-H, plus
//                     "the two codes are equal") is stored skewed by step -- one 2-byte store per
//                     lane, a contiguous line per wavefront step -- in LDS when the pair's trace fits
//                     the block's share, else in device scratch. The scout (last row j = 0..n-1,
//                     then last column rows 0..L, strict '>') rides along; lane 0 then walks the
//                     trace, emits the runs right to left into an LDS staging list and derives the
//                     eight fields from it.
//   k_path_scan       run counts of a round -> CSR offsets, carried on from the previous round.
//   k_path_compact    staged runs -> the caller's CSR run list.
//   k_adapter_profile one thread per selected pair walks its runs inside the aligned region and
//                     adds to the (adapter, position, A C G T N DEL INS) counters.
//
// Pairs are processed in rounds whose scratch (global traces + run staging) stays within a constant
// budget (PCABI_PATHS_SCRATCH_MB, default 256); a pair that alone exceeds it is refused.
#include <hipcub/hipcub.hpp>

#include <atomic>
#include <climits>
#include <cstring>
#include <mutex>
#include <vector>

#include "pcabi_kern.h"

namespace pcabi_eng {
namespace {

constexpr int kPathRows = 128;                    // two rows per lane
constexpr int kStage = 2 * kPathRows + 4;         // most runs a path has: 2L + 1 inside, head, two tails
constexpr int kLdsTrace = 16 * 1024;              // per-wavefront LDS share of the trace
constexpr int64_t kRoundPairs = 1 << 18;
constexpr int NEGV = INT_MIN / 2;                 // DPCellDefaultInfinity, S/align/dp_cell.h:144-145

enum { T_D = 1, T_H = 2, T_HO = 4, T_V = 8, T_VO = 16, T_MAXV = 32, T_MAXH = 64, T_EQ = 128 };

struct PathParams {
    const uint8_t *codes;
    const int64_t *win_off;
    const int32_t *win_len;
    const uint8_t *adp_codes;
    const int32_t *adp_off;
    const int32_t *adp_len;
    const int32_t *task_win, *task_adp;
    int64_t t0;              // first task of the round
    const int64_t *goff;     // per pair of the round: byte offset of its trace in gtrace, -1 = LDS
    const int64_t *soff;     // per pair of the round: word offset of its staged runs
    uint8_t *gtrace;
    uint32_t *stage;
    int32_t *cnt;            // per pair of the round: number of runs
    int32_t *out;
    int64_t out_stride;
    int ma, mi, go, ge;
};

// lane i reads lane i - 1 across the whole wavefront; lane 0 keeps `first`
__device__ __forceinline__ int from_lane_above(int first, int v) {
    return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xF, 0xF, false);
}

// One DP cell, S/align/dp_formula_affine.h:66-125 / dp_formula_linear.h:65-105 with _maxScore's
// "left unless left < right" ties (S/align/dp_formula.h:153-163).
template <bool AFFINE>
__device__ __forceinline__ void cell(int diag_s, int left_s, int left_h, int up_s, int up_v, bool eq, int ma,
                                     int mi, int go, int ge, int &s, int &h, int &v, int &tv) {
    const int diag = diag_s + (eq ? ma : mi);
    if (AFFINE) {
        const int hx = left_h + ge, ho = left_s + go;
        const bool hopen = hx < ho;
        h = hopen ? ho : hx;
        const int vx = up_v + ge, vo = up_s + go;
        const bool vopen = vx < vo;
        v = vopen ? vo : vx;
        const bool fromh = v < h;
        const int g = fromh ? h : v;
        const bool notd = diag < g;
        s = notd ? g : diag;
        tv = (notd ? (fromh ? T_MAXH : T_MAXV) : T_D) | (hopen ? T_HO : T_H) | (vopen ? T_VO : T_V);
    } else {
        const int vv = up_s + ge, hh = left_s + ge;
        const bool fromh = vv < hh;
        const int g = fromh ? hh : vv;
        const bool notd = diag < g;
        s = notd ? g : diag;
        tv = notd ? (fromh ? (T_H | T_MAXH) : (T_V | T_MAXV)) : T_D;
        h = NEGV;
        v = NEGV;
    }
    tv |= eq ? T_EQ : 0;
}

template <bool AFFINE>
__device__ __forceinline__ void run_pair(uint8_t *T, const uint8_t *rd, int n, const uint8_t *ad, int L,
                                         const PathParams &p, int k, uint32_t *stg, int *s_cnt) {
    const int lane = threadIdx.x;
    const int nl = (L + 1) >> 1, Lp = 2 * nl;
    const bool lane_on = lane < nl;
    const int i0 = 2 * lane + 1;
    const int a0 = i0 - 1 < L ? ad[i0 - 1] : 255;       // 255: the phantom row under an odd adapter
    const int a1 = i0 < L ? ad[i0] : 255;
    const bool last_lane = lane == nl - 1;
    const bool last_is_1 = (L & 1) == 0;                // row L is the lane's second row

    int sl0 = 0, sl1 = 0, hl0 = NEGV, hl1 = NEGV, vl0 = NEGV, vl1 = NEGV;   // own rows, previous column
    int sup_prev = 0;                                    // row i0 - 1, previous column
    int os = 0, ov = NEGV;                               // own second row, last column computed
    int rcur = 4, q = 4;
    int best_row = 0, bj_row = 0, bv_row = NEGV, bh_row = NEGV;   // S[L][0] = 0 > -inf
    const int steps = n + nl - 1;
    for (int t = 0; t < steps; ++t) {
        if ((t & 63) == 0) {
            const int idx = t + lane;
            q = idx < n ? rd[idx] : 4;
        }
        const int r_in = __builtin_amdgcn_readlane(q, t & 63);
        rcur = from_lane_above(r_in, rcur);
        const int up_s = from_lane_above(0, os), up_v = from_lane_above(NEGV, ov);
        const int j = t - lane + 1;
        if (lane_on && j >= 1 && j <= n) {
            int s0, h0, v0, t0, s1, h1, v1, t1;
            cell<AFFINE>(sup_prev, sl0, hl0, up_s, up_v, rcur == a0, p.ma, p.mi, p.go, p.ge, s0, h0, v0, t0);
            cell<AFFINE>(sl0, sl1, hl1, s0, v0, rcur == a1, p.ma, p.mi, p.go, p.ge, s1, h1, v1, t1);
            *(uint16_t *)(T + (size_t)t * Lp + 2 * lane) = (uint16_t)(t0 | (t1 << 8));
            if (last_lane && j < n) {
                const int sL = last_is_1 ? s1 : s0;
                if (sL > best_row) {
                    best_row = sL;
                    bj_row = j;
                    bv_row = last_is_1 ? v1 : v0;
                    bh_row = last_is_1 ? h1 : h0;
                }
            }
            sup_prev = up_s;
            sl0 = s0; hl0 = h0; vl0 = v0;
            sl1 = s1; hl1 = h1; vl1 = v1;
            os = s1; ov = v1;
        }
    }

    // last column, rows 1..L in order with strict '>': the largest score, the smallest row on ties
    long long key = LLONG_MIN;
    if (lane_on) {
        key = ((long long)sl0 << 32) | (unsigned)(0x7fffffff - i0);
        if (i0 + 1 <= L) {
            const long long k1 = ((long long)sl1 << 32) | (unsigned)(0x7fffffff - (i0 + 1));
            key = k1 > key ? k1 : key;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const long long other = __shfl_xor(key, o);
        key = other > key ? other : key;
    }
    const int cval = (int)(key >> 32), ci = 0x7fffffff - (int)(unsigned)(key & 0xffffffffll);
    const int owner = (ci - 1) >> 1;
    const bool sel1 = ((ci - 1) & 1) != 0;
    const int cv = __shfl(sel1 ? vl1 : vl0, owner), ch = __shfl(sel1 ? hl1 : hl0, owner);
    best_row = __shfl(best_row, nl - 1);
    bj_row = __shfl(bj_row, nl - 1);
    bv_row = __shfl(bv_row, nl - 1);
    bh_row = __shfl(bh_row, nl - 1);
    __syncthreads();            // the trace bytes of every lane are visible to lane 0

    if (lane == 0) {
        int best = best_row, bi = L, bj = bj_row, cell_v = bv_row, cell_h = bh_row;
        if (cval > best) { best = cval; bi = ci; bj = n; cell_v = cv; cell_h = ch; }
        auto trace = [&](int i, int j) -> int {
            return (i > 0 && j > 0) ? T[(size_t)(j - 1 + ((i - 1) >> 1)) * Lp + (i - 1)] : 0;
        };
        // runs are emitted right to left, equal neighbours merged
        int pos = kStage, cur_op = -1, cur_len = 0;
        auto emit = [&](int op, int len) {
            if (len <= 0) return;
            if (op == cur_op) { cur_len += len; return; }
            if (cur_op >= 0 && pos > 0) stg[--pos] = ((uint32_t)cur_len << 2) | (uint32_t)cur_op;
            cur_op = op;
            cur_len = len;
        };
        emit(PCABI_OP_READ_ONLY, n - bj);
        emit(PCABI_OP_ADAPTER_ONLY, L - bi);
        int i = bi, j = bj;
        if (i > 0 && j > 0) {
            int tv = trace(i, j);
            if (AFFINE) {       // S/align/dp_algorithm_impl.h:1170-1186
                if (cell_v == best) tv = (tv & ~T_D) | T_MAXV;
                else if (cell_h == best) tv = (tv & ~T_D) | T_MAXH;
            }
            while (i > 0 && j > 0 && (tv & 0x7f) != 0) {
                if (tv & T_D) {
                    emit((tv & T_EQ) ? PCABI_OP_MATCH : PCABI_OP_MISMATCH, 1);
                    --i; --j;
                    tv = trace(i, j);
                } else if ((tv & T_MAXV) && (tv & T_V)) {
                    if (AFFINE) {
                        while ((!(tv & T_VO) || (tv & T_V)) && i != 1) {
                            emit(PCABI_OP_ADAPTER_ONLY, 1);
                            --i;
                            tv = trace(i, j);
                        }
                    }
                    emit(PCABI_OP_ADAPTER_ONLY, 1);
                    --i;
                    tv = trace(i, j);
                } else if ((tv & T_MAXV) && (tv & T_VO)) {
                    emit(PCABI_OP_ADAPTER_ONLY, 1);
                    --i;
                    tv = trace(i, j);
                } else if ((tv & T_MAXH) && (tv & T_H)) {
                    if (AFFINE) {
                        while ((!(tv & T_HO) || (tv & T_H)) && j != 1) {
                            emit(PCABI_OP_READ_ONLY, 1);
                            --j;
                            tv = trace(i, j);
                        }
                    }
                    emit(PCABI_OP_READ_ONLY, 1);
                    --j;
                    tv = trace(i, j);
                } else if ((tv & T_MAXH) && (tv & T_HO)) {
                    emit(PCABI_OP_READ_ONLY, 1);
                    --j;
                    tv = trace(i, j);
                } else {
                    break;
                }
            }
        }
        if (i != 0) emit(PCABI_OP_ADAPTER_ONLY, i);
        else if (j != 0) emit(PCABI_OP_READ_ONLY, j);
        emit(-2, 1);            // flushes the last run
        const int cnt = kStage - pos;
        *s_cnt = cnt;

        // ScoredAlignment over the columns (alignment.cpp:27-109); st and en are run boundaries
        int st = -1, rs = 0, as = 0, a_first = -1, a_last = -1, m = 0;
        {
            bool rseen = false, aseen = false;
            int c = 0, rb = 0, ab = 0;
            for (int u = pos; u < kStage; ++u) {
                const int op = (int)(stg[u] & 3u), len = (int)(stg[u] >> 2);
                const bool hr = op != PCABI_OP_ADAPTER_ONLY, ha = op != PCABI_OP_READ_ONLY;
                rseen |= hr;
                aseen |= ha;
                if (st < 0 && rseen && aseen) { st = c; rs = rb; as = ab; }
                if (ha) {
                    if (a_first < 0) a_first = c;
                    a_last = c + len - 1;
                }
                if (op == PCABI_OP_MATCH) m += len;
                c += len;
                rb += hr ? len : 0;
                ab += ha ? len : 0;
            }
        }
        int en = -1, re = 0, ae = 0;
        {
            bool rseen = false, aseen = false;
            int c = 0;
            for (int u = pos; u < kStage; ++u) c += (int)(stg[u] >> 2);
            int rb = n, ab = L;     // bases in the columns before c
            for (int u = kStage - 1; u >= pos; --u) {
                const int op = (int)(stg[u] & 3u), len = (int)(stg[u] >> 2);
                const bool hr = op != PCABI_OP_ADAPTER_ONLY, ha = op != PCABI_OP_READ_ONLY;
                rseen |= hr;
                aseen |= ha;
                if (rseen && aseen) {
                    en = c - 1;
                    re = rb - (hr ? 1 : 0);
                    ae = ab - (ha ? 1 : 0);
                    break;
                }
                c -= len;
                rb -= hr ? len : 0;
                ab -= ha ? len : 0;
            }
        }
        const int l1 = en - st + 1;
        const int64_t o = p.t0 + k;
        p.out[0 * p.out_stride + o] = rs;
        p.out[1 * p.out_stride + o] = re;
        p.out[2 * p.out_stride + o] = as;
        p.out[3 * p.out_stride + o] = ae;
        p.out[4 * p.out_stride + o] = best;
        p.out[5 * p.out_stride + o] = l1 > 0 ? m : 0;
        p.out[6 * p.out_stride + o] = l1;
        p.out[7 * p.out_stride + o] = a_last - a_first + 1;
        p.cnt[k] = cnt;
    }
    __syncthreads();
    const int cnt = min(*s_cnt, 2 * L + 4);      // the pair's staging slot (a path never has more runs)
    uint32_t *dst = p.stage + p.soff[k];
    for (int u = lane; u < cnt; u += 64) dst[u] = stg[kStage - *s_cnt + u];
}

template <bool AFFINE>
__global__ __launch_bounds__(64) void k_paths(PathParams p) {
    extern __shared__ __align__(16) uint8_t lds_trace[];
    __shared__ uint32_t stg[kStage];
    __shared__ int s_cnt;
    const int k = blockIdx.x;
    const int64_t t = p.t0 + k;
    const int w = p.task_win[t], a = p.task_adp[t];
    const int n = p.win_len[w], L = p.adp_len[a];
    if (n <= 0 || L <= 0) {           // _isValidDPSettings: an empty sequence has no alignment
        if (threadIdx.x == 0) {
            for (int f = 0; f < 4; ++f) p.out[f * p.out_stride + t] = (f & 1) ? 0 : -1;   // as empty_result()
            p.out[4 * p.out_stride + t] = INT_MIN;
            for (int f = 5; f < 8; ++f) p.out[f * p.out_stride + t] = 0;
            p.cnt[k] = 0;
        }
        return;
    }
    const uint8_t *rd = p.codes + p.win_off[w], *ad = p.adp_codes + p.adp_off[a];
    const int64_t g = p.goff[k];
    if (g < 0) run_pair<AFFINE>(lds_trace, rd, n, ad, L, p, k, stg, &s_cnt);
    else run_pair<AFFINE>(p.gtrace + g, rd, n, ad, L, p, k, stg, &s_cnt);
}

// run_off[1 .. n] of the round (run_off points at the round's first task) from its counts, carried
// on from *total, which it moves to the round's end
__global__ __launch_bounds__(1024) void k_path_scan(const int32_t *cnt, int n, int64_t *run_off, long long *total) {
    using Scan = hipcub::BlockScan<long long, 1024>;
    __shared__ typename Scan::TempStorage tmp;
    __shared__ long long carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = *total;
    __syncthreads();
    for (int base = 0; base < n; base += 1024) {
        const long long v = base + tid < n ? cnt[base + tid] : 0;
        long long inc, agg;
        Scan(tmp).InclusiveSum(v, inc, agg);
        const long long c = carry;
        if (base + tid < n) run_off[base + tid + 1] = c + inc;
        __syncthreads();
        if (tid == 0) carry = c + agg;
        __syncthreads();
    }
    if (tid == 0) *total = carry;
}

__global__ __launch_bounds__(64) void k_path_compact(const int32_t *cnt, const int64_t *soff, const uint32_t *stage,
                                                     const int64_t *run_off, uint32_t *runs, int64_t cap) {
    const int k = blockIdx.x;
    const int c = cnt[k];
    const int64_t dst = run_off[k];
    const uint32_t *src = stage + soff[k];
    for (int u = threadIdx.x; u < c; u += 64)
        if (dst + u < cap) runs[dst + u] = src[u];
}

__global__ __launch_bounds__(256) void k_adapter_profile(const int32_t *res, const int64_t *run_off,
                                                         const uint32_t *runs, const uint8_t *codes,
                                                         const int64_t *win_off, const int32_t *win_len,
                                                         const int32_t *task_win, const int32_t *task_adp,
                                                         const uint8_t *select, int64_t n_task, int32_t n_adp,
                                                         int32_t max_adp_len, unsigned long long *counts) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_task) return;
    if (select && !select[t]) return;
    if (res && res[t] == -1) return;
    const int a = task_adp[t], w = task_win[t];
    if (a < 0 || a >= n_adp) return;
    const int64_t lo = run_off[t], hi = run_off[t + 1];
    // the aligned region [st, en] (alignment.cpp:28-52) in whole runs [u0, u1]
    int64_t u0 = -1, u1 = -1;
    {
        bool rseen = false, aseen = false;
        for (int64_t u = lo; u < hi; ++u) {
            const int op = (int)(runs[u] & 3u);
            rseen |= op != PCABI_OP_ADAPTER_ONLY;
            aseen |= op != PCABI_OP_READ_ONLY;
            if (rseen && aseen) { u0 = u; break; }
        }
        rseen = aseen = false;
        for (int64_t u = hi - 1; u >= lo; --u) {
            const int op = (int)(runs[u] & 3u);
            rseen |= op != PCABI_OP_ADAPTER_ONLY;
            aseen |= op != PCABI_OP_READ_ONLY;
            if (rseen && aseen) { u1 = u; break; }
        }
    }
    if (u0 < 0 || u1 < u0) return;
    const uint8_t *rd = codes + win_off[w];
    const int n = win_len[w];
    unsigned long long *row = counts + (size_t)a * max_adp_len * PCABI_PROFILE_NCOL;
    int ai = 0, rj = 0;           // adapter / read bases left of the current column
    for (int64_t u = lo; u <= u1; ++u) {
        const int op = (int)(runs[u] & 3u), len = (int)(runs[u] >> 2);
        if (u >= u0) {
            for (int c = 0; c < len; ++c) {
                int pos, col;
                if (op == PCABI_OP_READ_ONLY) {
                    pos = ai > 0 ? ai - 1 : 0;      // the last adapter base to its left
                    col = PCABI_PROFILE_INS;
                } else if (op == PCABI_OP_ADAPTER_ONLY) {
                    pos = ai + c;
                    col = PCABI_PROFILE_DEL;
                } else {
                    pos = ai + c;
                    const int code = rj + c < n ? rd[rj + c] : 4;
                    col = code < 4 ? code : PCABI_PROFILE_N;
                }
                if (pos < max_adp_len) atomicAdd(&row[(size_t)pos * PCABI_PROFILE_NCOL + col], 1ull);
            }
        }
        ai += op != PCABI_OP_READ_ONLY ? len : 0;
        rj += op != PCABI_OP_ADAPTER_ONLY ? len : 0;
    }
}

// ---- host logic -----------------------------------------------------------------------------------

struct DevMem {            // plain device allocation, freed on scope exit
    void *p = nullptr;
    ~DevMem() { if (p) (void)hipFree(p); }
    int get(size_t bytes) {
        const hipError_t e = hipMalloc(&p, std::max<size_t>(bytes, 256));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            return fail(PCABI_E_NOMEM, "hipMalloc failed (" + std::to_string(bytes) + " bytes): " + hipGetErrorString(e));
        }
        return 0;
    }
};

// Per-device scratch of the path kernels, kept between calls (a call holds the mutex until its
// stream has drained, so two callers never share it).
struct PathsState {
    std::mutex mu;
    void *scratch = nullptr;
    size_t cap = 0;
    void *meta = nullptr;      // goff, soff (int64 x kRoundPairs each), cnt (int32 x kRoundPairs), total
    hipStream_t stream = nullptr;
    int ensure(size_t bytes) {
        if (!meta) {
            const hipError_t e = hipMalloc(&meta, (size_t)kRoundPairs * 20 + 64);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                meta = nullptr;
                return fail(PCABI_E_NOMEM, std::string("hipMalloc of the path round tables: ") + hipGetErrorString(e));
            }
        }
        if (bytes <= cap) return 0;
        if (scratch) (void)hipFree(scratch);
        scratch = nullptr;
        cap = 0;
        const hipError_t e = hipMalloc(&scratch, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            scratch = nullptr;
            return fail(PCABI_E_NOMEM, "hipMalloc failed (" + std::to_string(bytes) + " bytes): " + hipGetErrorString(e));
        }
        cap = bytes;
        pcabi_poison(scratch, bytes);
        return 0;
    }
};
PathsState g_paths[16];
std::atomic<long long> g_scratch_pairs{0};

int64_t scratch_budget() {
    const char *e = std::getenv("PCABI_PATHS_SCRATCH_MB");
    const long mb = e ? std::atol(e) : 0;
    return (int64_t)(mb > 0 ? mb : 256) << 20;
}

struct Round {
    int64_t t0 = 0;
    std::vector<int64_t> goff, soff;
    int64_t trace_bytes = 0, stage_words = 0;
    int lds = 0;
};

int check_path_args(const int32_t *win_len, int64_t n_win, const int32_t *adp_len, int32_t n_adp,
                    const int32_t *task_win, const int32_t *task_adp, int64_t n_task) {
    if (n_win < 0 || n_adp < 0 || n_task < 0) return fail(PCABI_E_ARG, "negative count");
    if (n_task > 0 && (!task_win || !task_adp)) return fail(PCABI_E_ARG, "paths take explicit (window, adapter) pairs");
    for (int a = 0; a < n_adp; ++a)
        if (adp_len[a] < 1 || adp_len[a] > kPathRows)
            return fail(PCABI_E_ARG, "adapter " + std::to_string(a) + " has " + std::to_string(adp_len[a]) +
                                         " bases: alignment paths take adapters of 1.." + std::to_string(kPathRows));
    for (int64_t w = 0; w < n_win; ++w)
        if (win_len[w] < 0 || win_len[w] > pcabi::MAX_WINDOW_LEN) return fail(PCABI_E_ARG, "window length out of range");
    for (int64_t t = 0; t < n_task; ++t)
        if (task_win[t] < 0 || task_win[t] >= n_win || task_adp[t] < 0 || task_adp[t] >= n_adp)
            return fail(PCABI_E_ARG, "task index out of range");
    return 0;
}

// The rounds of a call: consecutive tasks whose global traces and run staging fit the budget.
int plan_rounds(const int32_t *win_len, const int32_t *adp_len, const int32_t *task_win, const int32_t *task_adp,
                int64_t n_task, std::vector<Round> &rounds, int64_t *n_global) {
    const int64_t budget = scratch_budget();
    Round cur;
    int64_t used = 0;
    for (int64_t t = 0; t < n_task; ++t) {
        const int64_t n = win_len[task_win[t]], L = adp_len[task_adp[t]];
        const int64_t nl = (L + 1) / 2;
        int64_t trace = 0, words = 0;
        bool lds = true;
        if (n > 0) {
            trace = ((n + nl - 1) * 2 * nl + 15) & ~(int64_t)15;
            words = 2 * L + 4;
            lds = trace <= kLdsTrace;
        }
        const int64_t cost = 4 * words + (lds ? 0 : trace);
        if (cost > budget)
            return fail(PCABI_E_ARG, "pair " + std::to_string(t) + " (window of " + std::to_string(n) + " bases, adapter of " +
                                         std::to_string(L) + "): its trace of " + std::to_string(trace) +
                                         " bytes exceeds the scratch budget of " + std::to_string(budget) + " bytes");
        if (!cur.goff.empty() && (used + cost > budget || (int64_t)cur.goff.size() >= kRoundPairs)) {
            rounds.push_back(std::move(cur));
            cur = Round();
            cur.t0 = t;
            used = 0;
        }
        if (cur.goff.empty()) cur.t0 = t;
        cur.goff.push_back(lds ? -1 : cur.trace_bytes);
        cur.soff.push_back(cur.stage_words);
        if (lds) cur.lds = std::max(cur.lds, (int)trace);
        else { cur.trace_bytes += trace; ++*n_global; }
        cur.stage_words += words;
        used += cost;
    }
    if (!cur.goff.empty()) rounds.push_back(std::move(cur));
    return 0;
}

// Every pointer but the h_* ones is a device pointer; queues the rounds on st and waits for them.
int64_t paths_run(PathsState &S, const uint8_t *codes, const int64_t *win_off, const int32_t *win_len,
                  const uint8_t *adp_codes, const int32_t *adp_off, const int32_t *adp_len, const int32_t *task_win,
                  const int32_t *task_adp, int64_t n_task, const int32_t *h_win_len, const int32_t *h_adp_len,
                  const int32_t *h_task_win, const int32_t *h_task_adp, int ma, int mi, int go, int ge, int32_t *out,
                  int64_t *run_off, uint32_t *runs, int64_t runs_cap, hipStream_t st) {
    std::vector<Round> rounds;
    int64_t n_global = 0;
    if (int rc = plan_rounds(h_win_len, h_adp_len, h_task_win, h_task_adp, n_task, rounds, &n_global)) return rc;
    size_t need = 256;
    for (const Round &r : rounds)
        need = std::max(need, (size_t)((r.trace_bytes + 255) & ~(int64_t)255) + 4 * (size_t)r.stage_words + 256);
    if (int rc = S.ensure(need)) return rc;
    int64_t *d_goff = (int64_t *)S.meta, *d_soff = d_goff + kRoundPairs;
    int32_t *d_cnt = (int32_t *)(d_soff + kRoundPairs);
    long long *d_total = (long long *)((char *)S.meta + (size_t)kRoundPairs * 20);
    HIP_TRY(hipMemsetAsync(d_total, 0, sizeof(long long), st));
    HIP_TRY(hipMemsetAsync(run_off, 0, sizeof(int64_t), st));
    for (const Round &r : rounds) {
        const int nr = (int)r.goff.size();
        HIP_TRY(hipMemcpyAsync(d_goff, r.goff.data(), sizeof(int64_t) * nr, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_soff, r.soff.data(), sizeof(int64_t) * nr, hipMemcpyHostToDevice, st));
        PathParams p{};
        p.codes = codes; p.win_off = win_off; p.win_len = win_len;
        p.adp_codes = adp_codes; p.adp_off = adp_off; p.adp_len = adp_len;
        p.task_win = task_win; p.task_adp = task_adp;
        p.t0 = r.t0;
        p.goff = d_goff; p.soff = d_soff;
        p.gtrace = (uint8_t *)S.scratch;
        p.stage = (uint32_t *)((char *)S.scratch + ((r.trace_bytes + 255) & ~(int64_t)255));
        p.cnt = d_cnt;
        p.out = out; p.out_stride = n_task;
        p.ma = ma; p.mi = mi; p.go = go; p.ge = ge;
        if (go != ge) hipLaunchKernelGGL(k_paths<true>, dim3((unsigned)nr), dim3(64), (size_t)r.lds, st, p);
        else hipLaunchKernelGGL(k_paths<false>, dim3((unsigned)nr), dim3(64), (size_t)r.lds, st, p);
        hipLaunchKernelGGL(k_path_scan, dim3(1), dim3(1024), 0, st, (const int32_t *)d_cnt, nr, run_off + r.t0, d_total);
        hipLaunchKernelGGL(k_path_compact, dim3((unsigned)nr), dim3(64), 0, st, (const int32_t *)d_cnt,
                           (const int64_t *)d_soff, (const uint32_t *)p.stage, (const int64_t *)(run_off + r.t0), runs,
                           runs_cap);
        HIP_TRY(hipGetLastError());
    }
    long long total = 0;
    HIP_TRY(hipMemcpyAsync(&total, d_total, sizeof(long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));      // also: the rounds' host tables outlive their copies
    g_scratch_pairs.fetch_add(n_global);
    return (int64_t)total;
}

int paths_state(int device, PathsState **out) {
    if (device < 0 || device >= 16) return fail(PCABI_E_ARG, "bad device index");
    *out = &g_paths[device];
    return 0;
}

int host_device_ready(PathsState &S, int device) {
    HIP_TRY(hipSetDevice(device));
    if (S.stream) return 0;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(PCABI_E_DEVICE, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950");
    HIP_TRY(hipStreamCreateWithFlags(&S.stream, hipStreamNonBlocking));
    return 0;
}

}  // namespace
}  // namespace pcabi_eng

using namespace pcabi_eng;

extern "C" {

int pcabi_max_path_adapter_len(void) { return kPathRows; }

int64_t pcabi_paths_scratch_pairs(void) { return g_scratch_pairs.load(); }

int64_t pcabi_align_paths_dev(const uint8_t *codes, const int64_t *win_off, const int32_t *win_len, int64_t n_win,
                              const uint8_t *adp_codes, const int32_t *adp_off, const int32_t *adp_len, int32_t n_adp,
                              const int32_t *task_win, const int32_t *task_adp, int64_t n_task, int match,
                              int mismatch, int gap_open, int gap_extend, int32_t *out, int64_t *run_off,
                              uint32_t *runs, int64_t runs_cap, void *stream) {
    if (n_win < 0 || n_adp < 0 || n_task < 0 || runs_cap < 0) return fail(PCABI_E_ARG, "negative count");
    if (!run_off) return fail(PCABI_E_ARG, "run_off is NULL");
    const hipStream_t st = (hipStream_t)stream;
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    PathsState *S;
    if (int rc = paths_state(device, &S)) return rc;
    // the plan needs the lengths and the pairs on the host
    std::vector<int32_t> h_wl((size_t)n_win), h_al((size_t)n_adp), h_tw((size_t)n_task), h_ta((size_t)n_task);
    if (n_win) HIP_TRY(hipMemcpyAsync(h_wl.data(), win_len, sizeof(int32_t) * (size_t)n_win, hipMemcpyDeviceToHost, st));
    if (n_adp) HIP_TRY(hipMemcpyAsync(h_al.data(), adp_len, sizeof(int32_t) * (size_t)n_adp, hipMemcpyDeviceToHost, st));
    if (n_task && task_win && task_adp) {
        HIP_TRY(hipMemcpyAsync(h_tw.data(), task_win, sizeof(int32_t) * (size_t)n_task, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h_ta.data(), task_adp, sizeof(int32_t) * (size_t)n_task, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (int rc = check_path_args(h_wl.data(), n_win, h_al.data(), n_adp, task_win ? h_tw.data() : nullptr,
                                 task_adp ? h_ta.data() : nullptr, n_task))
        return rc;
    std::lock_guard<std::mutex> lock(S->mu);
    return paths_run(*S, codes, win_off, win_len, adp_codes, adp_off, adp_len, task_win, task_adp, n_task, h_wl.data(),
                     h_al.data(), h_tw.data(), h_ta.data(), match, mismatch, gap_open, gap_extend, out, run_off, runs,
                     runs_cap, st);
}

int64_t pcabi_align_paths_host(int device, const uint8_t *codes, int64_t codes_len, const int64_t *win_off,
                               const int32_t *win_len, int64_t n_win, const uint8_t *adp_codes,
                               const int32_t *adp_off, const int32_t *adp_len, int32_t n_adp, const int32_t *task_win,
                               const int32_t *task_adp, int64_t n_task, int match, int mismatch, int gap_open,
                               int gap_extend, int32_t *out, int64_t *run_off, uint32_t *runs, int64_t runs_cap) {
    if (runs_cap < 0 || codes_len < 0) return fail(PCABI_E_ARG, "negative count");
    if (!run_off) return fail(PCABI_E_ARG, "run_off is NULL");
    if (int rc = check_path_args(win_len, n_win, adp_len, n_adp, task_win, task_adp, n_task)) return rc;
    int64_t adp_bytes = 0;
    for (int a = 0; a < n_adp; ++a) {
        if (adp_off[a] < 0) return fail(PCABI_E_ARG, "negative adapter offset");
        adp_bytes = std::max<int64_t>(adp_bytes, (int64_t)adp_off[a] + adp_len[a]);
    }
    for (int64_t w = 0; w < n_win; ++w)
        if (win_len[w] > 0 && (win_off[w] < 0 || win_off[w] + win_len[w] + 16 > codes_len))
            return fail(PCABI_E_ARG, "window outside the buffer or buffer not padded by 16 bytes");
    run_off[0] = 0;
    if (n_task == 0) return 0;
    PathsState *S;
    if (int rc = paths_state(device, &S)) return rc;
    std::lock_guard<std::mutex> lock(S->mu);
    if (int rc = host_device_ready(*S, device)) return rc;
    const hipStream_t st = S->stream;
    const size_t nw = (size_t)n_win, nt = (size_t)n_task, na = (size_t)n_adp;
    DevMem d_codes, d_woff, d_wlen, d_ac, d_aoff, d_alen, d_tw, d_ta, d_out, d_roff, d_runs;
    if (int rc = d_codes.get((size_t)codes_len)) return rc;
    if (int rc = d_woff.get(8 * nw)) return rc;
    if (int rc = d_wlen.get(4 * nw)) return rc;
    if (int rc = d_ac.get((size_t)adp_bytes)) return rc;
    if (int rc = d_aoff.get(4 * na)) return rc;
    if (int rc = d_alen.get(4 * na)) return rc;
    if (int rc = d_tw.get(4 * nt)) return rc;
    if (int rc = d_ta.get(4 * nt)) return rc;
    if (int rc = d_out.get(4 * PCABI_NFIELDS * nt)) return rc;
    if (int rc = d_roff.get(8 * (nt + 1))) return rc;
    if (int rc = d_runs.get(4 * (size_t)runs_cap)) return rc;
    HIP_TRY(hipMemcpyAsync(d_codes.p, codes, (size_t)codes_len, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_woff.p, win_off, 8 * nw, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_wlen.p, win_len, 4 * nw, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_ac.p, adp_codes, (size_t)adp_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_aoff.p, adp_off, 4 * na, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_alen.p, adp_len, 4 * na, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_tw.p, task_win, 4 * nt, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_ta.p, task_adp, 4 * nt, hipMemcpyHostToDevice, st));
    const int64_t total = paths_run(*S, (const uint8_t *)d_codes.p, (const int64_t *)d_woff.p, (const int32_t *)d_wlen.p,
                                    (const uint8_t *)d_ac.p, (const int32_t *)d_aoff.p, (const int32_t *)d_alen.p,
                                    (const int32_t *)d_tw.p, (const int32_t *)d_ta.p, n_task, win_len, adp_len, task_win,
                                    task_adp, match, mismatch, gap_open, gap_extend, (int32_t *)d_out.p,
                                    (int64_t *)d_roff.p, (uint32_t *)d_runs.p, runs_cap, st);
    if (total < 0) return total;
    HIP_TRY(hipMemcpyAsync(out, d_out.p, 4 * PCABI_NFIELDS * nt, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(run_off, d_roff.p, 8 * (nt + 1), hipMemcpyDeviceToHost, st));
    if (total <= runs_cap && total > 0)
        HIP_TRY(hipMemcpyAsync(runs, d_runs.p, 4 * (size_t)total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return total;
}

int pcabi_adapter_profile_dev(const int32_t *res, const int64_t *run_off, const uint32_t *runs, const uint8_t *codes,
                              const int64_t *win_off, const int32_t *win_len, const int32_t *task_win,
                              const int32_t *task_adp, const uint8_t *select, int64_t n_task, int32_t n_adp,
                              int32_t max_adp_len, int64_t *counts, void *stream) {
    if (n_task < 0 || n_adp < 0 || max_adp_len < 0) return fail(PCABI_E_ARG, "negative count");
    if (n_task == 0 || n_adp == 0 || max_adp_len == 0) return 0;
    if (!run_off || !runs || !counts) return fail(PCABI_E_ARG, "NULL run list or counters");
    hipLaunchKernelGGL(k_adapter_profile, dim3((unsigned)((n_task + 255) / 256)), dim3(256), 0, (hipStream_t)stream, res,
                       run_off, runs, codes, win_off, win_len, task_win, task_adp, select, n_task, n_adp, max_adp_len,
                       (unsigned long long *)counts);
    HIP_TRY(hipGetLastError());
    return 0;
}

int pcabi_adapter_profile_host(int device, const int32_t *res, const int64_t *run_off, const uint32_t *runs,
                               const uint8_t *codes, int64_t codes_len, const int64_t *win_off, const int32_t *win_len,
                               int64_t n_win, const int32_t *task_win, const int32_t *task_adp, const uint8_t *select,
                               int64_t n_task, int32_t n_adp, int32_t max_adp_len, int64_t *counts) {
    if (n_task < 0 || n_adp < 0 || max_adp_len < 0 || n_win < 0 || codes_len < 0) return fail(PCABI_E_ARG, "negative count");
    if (n_task == 0 || n_adp == 0 || max_adp_len == 0) return 0;
    if (!run_off || !counts || !task_win || !task_adp) return fail(PCABI_E_ARG, "NULL run list, pairs or counters");
    for (int64_t w = 0; w < n_win; ++w)
        if (win_len[w] < 0 || (win_len[w] > 0 && (win_off[w] < 0 || win_off[w] + win_len[w] + 16 > codes_len)))
            return fail(PCABI_E_ARG, "window outside the buffer or buffer not padded by 16 bytes");
    for (int64_t t = 0; t < n_task; ++t) {
        if (task_win[t] < 0 || task_win[t] >= n_win || task_adp[t] < 0 || task_adp[t] >= n_adp)
            return fail(PCABI_E_ARG, "task index out of range");
        if (run_off[t] < 0 || run_off[t + 1] < run_off[t]) return fail(PCABI_E_ARG, "run offsets not ascending");
    }
    const int64_t total = run_off[n_task];
    if (total > 0 && !runs) return fail(PCABI_E_ARG, "NULL run list");
    PathsState *S;
    if (int rc = paths_state(device, &S)) return rc;
    std::lock_guard<std::mutex> lock(S->mu);
    if (int rc = host_device_ready(*S, device)) return rc;
    const hipStream_t st = S->stream;
    const size_t nw = (size_t)n_win, nt = (size_t)n_task;
    const size_t nc = (size_t)n_adp * (size_t)max_adp_len * PCABI_PROFILE_NCOL;
    DevMem d_res, d_roff, d_runs, d_codes, d_woff, d_wlen, d_tw, d_ta, d_sel, d_cnt;
    if (int rc = d_roff.get(8 * (nt + 1))) return rc;
    if (int rc = d_runs.get(4 * (size_t)total)) return rc;
    if (int rc = d_codes.get((size_t)codes_len)) return rc;
    if (int rc = d_woff.get(8 * nw)) return rc;
    if (int rc = d_wlen.get(4 * nw)) return rc;
    if (int rc = d_tw.get(4 * nt)) return rc;
    if (int rc = d_ta.get(4 * nt)) return rc;
    if (int rc = d_cnt.get(8 * nc)) return rc;
    if (res) {
        if (int rc = d_res.get(4 * nt)) return rc;
        HIP_TRY(hipMemcpyAsync(d_res.p, res, 4 * nt, hipMemcpyHostToDevice, st));
    }
    if (select) {
        if (int rc = d_sel.get(nt)) return rc;
        HIP_TRY(hipMemcpyAsync(d_sel.p, select, nt, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(d_roff.p, run_off, 8 * (nt + 1), hipMemcpyHostToDevice, st));
    if (total > 0) HIP_TRY(hipMemcpyAsync(d_runs.p, runs, 4 * (size_t)total, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_codes.p, codes, (size_t)codes_len, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_woff.p, win_off, 8 * nw, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_wlen.p, win_len, 4 * nw, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_tw.p, task_win, 4 * nt, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_ta.p, task_adp, 4 * nt, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_cnt.p, counts, 8 * nc, hipMemcpyHostToDevice, st));
    if (int rc = pcabi_adapter_profile_dev((const int32_t *)d_res.p, (const int64_t *)d_roff.p, (const uint32_t *)d_runs.p,
                                           (const uint8_t *)d_codes.p, (const int64_t *)d_woff.p,
                                           (const int32_t *)d_wlen.p, (const int32_t *)d_tw.p, (const int32_t *)d_ta.p,
                                           (const uint8_t *)d_sel.p, n_task, n_adp, max_adp_len, (int64_t *)d_cnt.p, st))
        return rc;
    HIP_TRY(hipMemcpyAsync(counts, d_cnt.p, 8 * nc, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"
