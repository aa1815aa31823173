// pcabi_engine.hip -- gfx950 kernels + C ABI of the adapter-alignment engine (include/pcabi.h).
//
// Kernel map:
//   k_align<RPL, AFFINE, KIND>  one lane = one (window, adapter) DP with the adapter's RPL rows
//                               in VGPRs, one column (read base) per step (pcabi_dp.h). The
//                               wave's adapter is uniform. KIND picks the DP core: PACKED
//                               (score|tie-break|attributes in one int32 key, substitution keys
//                               from an LDS table), FAST (separate score/attribute registers,
//                               adapters <= 64) or GENERIC (any scoring, adapters <= 128).
//                               Two work shapes: cross (every window x every adapter of a
//                               bucket; XCD-aware tile order) and pairs (explicit tasks grouped
//                               into per-adapter waves on the host).
//   k_end_trim                  per-read decision epilogue (nanopore_read.py:175-217).
//   k_best_full_id              per-adapter max of the full-adapter identity
//                               (nanopore_read.py:158-173), deterministic (max is exact).
//   k_first_hit                 middle-scan round 1: first adapter over the threshold per read
//                               (nanopore_read.py:219-252).
//   k_tile_windows              window list -> tile layout (coalesced cross-mode reads).
// The device-resident middle scan (its kernels, its scratch, the host-driven loop and the queued
// rounds) is pcabi_middle.hip; this unit keeps the scan's host-buffer entries, which use Engine.
// What the two share is declared in pcabi_host.h.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <immintrin.h>

#include <algorithm>
#include <chrono>
#include <atomic>
#include <cstdio>
#include <memory>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "../../include/pcabi.h"
#include "pcabi_dp.h"
#include "pcabi_kern.h"
#include "pcabi_host.h"

namespace {
thread_local std::string g_err;
}  // namespace

namespace pcabi_eng {
int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
}  // namespace pcabi_eng

using namespace pcabi_eng;

namespace {


int bucket_of(int L, const pcabi::Scoring &sc, bool allow_wide = true) {
    if (L > kMaxRPL) return kStripedBucket;
    if (L <= 64) {
        const int rpl = (L + 3) & ~3;
        if (pcabi::fast_ok(L, rpl, sc)) return rpl / 4 - 1;
    } else if (allow_wide && L <= pcabi::pk::MAX_L) {
        const int rpl = (L + 3) & ~3;
        if (pcabi::packed_ok(L, rpl, sc)) return 16 + (rpl - 68) / 4;
    } else if (allow_wide && L <= pcabi::pk::MAX_L_LONG) {
        const int b = L <= 96 ? 22 : (L <= 112 ? 23 : 24);
        if (pcabi::long_ok(L, kBuckets[b].rpl, sc)) return b;
    }
    // The generic core keeps every row's state in registers: past 64 rows under affine gaps it
    // spills (k_align<96 / 128, true, 1>: hundreds of VGPRs to scratch) and runs slower than the
    // striped core, which holds 32 rows at a time.
    if (L > 64 && sc.go != sc.ge) return kStripedBucket;
    for (int b = 0; b < kNumBuckets; ++b)
        if (kBuckets[b].kind == GENERIC && L <= kBuckets[b].rpl) return b;
    return -1;
}

// ---- decision epilogues --------------------------------------------------------------------

// One block per 64 reads: wave w takes adapters w, w + 4, ... of both sides (lane = read: the
// loads of one adapter's field are 256-B coalesced), the four partial maxima meet in LDS. (r03: one
// thread per read looped over every adapter -- 391 blocks for 100k reads, latency-bound.) r06: the
// four fields a decision reads (rs, re, m, l1: 16 of the result's 32 bytes) are loaded
// unconditionally, four adapters at a time, so a wave keeps 16 independent loads in flight instead
// of a dependent pair per adapter (the kernel reads 149 MB per headline step: HBM-bound, 42 us in r05).
struct EndFields {
    int rs, re, m, l1;
};
__device__ __forceinline__ EndFields end_fields(const int32_t *res, int64_t stride, int64_t i) {
    return EndFields{res[0 * stride + i], res[1 * stride + i], res[5 * stride + i], res[6 * stride + i]};
}

__global__ __launch_bounds__(256) void k_end_trim(const int32_t *sres, int64_t sstride, int32_t n_sa,
                                                  const int32_t *eres, int64_t estride, int32_t n_ea,
                                                  int64_t n_read, int end_size, int extra,
                                                  double thr, int min_trim,
                                                  int32_t *start_trim, int32_t *end_trim,
                                                  uint8_t *shit, uint8_t *ehit) {
    __shared__ int s_st[4][64], s_et[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * 64 + lane;
    const bool live = r < n_read;
    constexpr int U = 4;                              // adapters in flight per wave
    // find_start_trim (nanopore_read.py:175-195)
    int st = 0;
    for (int a0 = w; live && a0 < n_sa; a0 += 4 * U) {
        EndFields f[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int a = a0 + 4 * u;
            f[u] = a < n_sa ? end_fields(sres, sstride, (int64_t)a * n_read + r) : EndFields{-1, 0, 0, 0};
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int a = a0 + 4 * u;
            if (a >= n_sa) break;
            const int rs = f[u].rs;
            int re1 = 0, hit = 0;
            double partial = 0.0;
            if (rs != -1) {
                re1 = f[u].re + 1;
                partial = pcabi::pid6(f[u].m, f[u].l1);
            }
            if (partial > thr && re1 != end_size && re1 - rs >= min_trim) {
                st = max(st, re1 + extra);
                hit = 1;
            }
            if (shit) shit[(int64_t)a * n_read + r] = (uint8_t)hit;
        }
    }
    // find_end_trim (nanopore_read.py:197-217)
    int et = 0;
    for (int a0 = w; live && a0 < n_ea; a0 += 4 * U) {
        EndFields f[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int a = a0 + 4 * u;
            f[u] = a < n_ea ? end_fields(eres, estride, (int64_t)a * n_read + r) : EndFields{-1, 0, 0, 0};
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int a = a0 + 4 * u;
            if (a >= n_ea) break;
            const int rs = f[u].rs;
            int re1 = 0, hit = 0;
            double partial = 0.0;
            if (rs != -1) {
                re1 = f[u].re + 1;
                partial = pcabi::pid6(f[u].m, f[u].l1);
            }
            if (partial > thr && rs != 0 && re1 - rs >= min_trim) {
                et = max(et, (end_size - rs) + extra);
                hit = 1;
            }
            if (ehit) ehit[(int64_t)a * n_read + r] = (uint8_t)hit;
        }
    }
    s_st[w][lane] = st;
    s_et[w][lane] = et;
    __syncthreads();
    if (w == 0 && live) {
        start_trim[r] = max(max(s_st[0][lane], s_st[1][lane]), max(s_st[2][lane], s_st[3][lane]));
        end_trim[r] = max(max(s_et[0][lane], s_et[1][lane]), max(s_et[2][lane], s_et[3][lane]));
    }
}

// best[a] = max(best[a], max_w pid2): one block per adapter, uint64 ordering of non-negative
// doubles == numeric ordering, so the max is exact and order independent.
__global__ __launch_bounds__(256) void k_best_full_id(const int32_t *res, int64_t stride, int64_t n_win,
                                                      double *best) {
    const int a = blockIdx.x;
    __shared__ unsigned long long red[256];
    unsigned long long mx = 0;
    for (int64_t w = threadIdx.x; w < n_win; w += 256) {
        const int64_t i = (int64_t)a * n_win + w;
        const int rs = res[0 * stride + i];
        const double full = (rs == -1) ? 0.0 : pcabi::pid6(res[5 * stride + i], res[7 * stride + i]);
        const unsigned long long b = (unsigned long long)__double_as_longlong(full);
        mx = b > mx ? b : mx;
    }
    red[threadIdx.x] = mx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] > red[threadIdx.x + s] ? red[threadIdx.x] : red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const unsigned long long cur = (unsigned long long)__double_as_longlong(best[a]);
        best[a] = __longlong_as_double((long long)(red[0] > cur ? red[0] : cur));
    }
}

// Barcode call (porechop_abi/nanopore_read.py:408-482) over the barcode dicts that
// find_start_trim / find_end_trim fill (:193-195, :215-217). A side's dict is given as slots in
// insertion order: slot k holds barcode id name[k] with the full-adapter identity of adapter
// adp[k] (the LAST adapter of that name in set order -- a dict keeps a key's first position and
// its last value). The reference's stable sorts reduce to strict '>' scans in slot order:
//   per side  : best / second = first two of the descending stable sort
//   merged    : entries ordered by (-score, start before end, slot); best = the first, second =
//               the first entry whose name differs (the dedup keeps each name's first entry)
// Missing entries are ('none', 0.0), the reference's defaults (nanopore_read.py:58-61).
struct BcSide {
    const int32_t *res;
    int64_t stride;
    const int32_t *adp, *name;
    int32_t n;
};

__device__ __forceinline__ double bc_score(const BcSide &s, int k, int64_t n_read, int64_t r) {
    const int64_t i = (int64_t)s.adp[k] * n_read + r;
    return s.res[0 * s.stride + i] == -1 ? 0.0 : pcabi::pid6(s.res[5 * s.stride + i], s.res[7 * s.stride + i]);
}

__global__ __launch_bounds__(256) void k_barcode_call(BcSide st, BcSide en, int64_t n_read, double thr, double diff,
                                                      int require_two, int32_t *call, double *scores) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_read) return;
    int c = -1;
    if (require_two) {
        double b[2][2] = {{0.0, 0.0}, {0.0, 0.0}};   // [side][best, second]
        int bn[2] = {-1, -1};
        int cnt[2] = {0, 0};
        for (int side = 0; side < 2; ++side) {
            const BcSide &s = side ? en : st;
            for (int k = 0; k < s.n; ++k) {
                const double x = bc_score(s, k, n_read, r);
                if (cnt[side] == 0 || x > b[side][0]) {
                    if (cnt[side] > 0) b[side][1] = b[side][0];
                    b[side][0] = x;
                    bn[side] = s.name[k];
                } else if (cnt[side] == 1 || x > b[side][1]) {
                    b[side][1] = x;
                }
                ++cnt[side];
            }
        }
        if (b[0][0] >= thr && b[1][0] >= thr && b[0][0] >= b[0][1] + diff && b[1][0] >= b[1][1] + diff &&
            bn[0] == bn[1])
            c = bn[0];
        if (scores) {
            scores[4 * r + 0] = b[0][0]; scores[4 * r + 1] = b[0][1];
            scores[4 * r + 2] = b[1][0]; scores[4 * r + 3] = b[1][1];
        }
    } else {
        double b1 = 0.0, b2 = 0.0;
        int n1 = -1;
        bool has1 = false, has2 = false;
        for (int side = 0; side < 2; ++side) {
            const BcSide &s = side ? en : st;
            for (int k = 0; k < s.n; ++k) {
                const double x = bc_score(s, k, n_read, r);
                const int nm = s.name[k];
                if (!has1 || x > b1) {
                    // the previous best heads the entries of every other name
                    if (has1 && n1 != nm) { b2 = b1; has2 = true; }
                    b1 = x; n1 = nm; has1 = true;
                } else if (nm != n1 && (!has2 || x > b2)) {
                    b2 = x; has2 = true;
                }
            }
        }
        if (b1 >= thr && b1 >= b2 + diff) c = has1 ? n1 : -1;
        if (scores) {
            scores[4 * r + 0] = b1; scores[4 * r + 1] = b2;
            scores[4 * r + 2] = 0.0; scores[4 * r + 3] = 0.0;
        }
    }
    call[r] = c;
}

// Middle-scan round 1 (porechop_abi/nanopore_read.py:219-252): per read, the FIRST adapter in
// list order whose full-adapter identity is not below the threshold on the unmasked read. The
// reference's loop hits exactly that adapter first (the ones before it fail on this same
// sequence and are never revisited), so only this hit leaves the device: hits[f * hit_stride +
// w] for f = adapter (-1 = none), rs, re (inclusive), m, l2.
__global__ __launch_bounds__(256) void k_first_hit(const int32_t *res, int64_t stride, int64_t n_win,
                                                   int32_t n_adp, double thr, const int32_t *start_adp,
                                                   int32_t *hits, int64_t hit_stride) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= n_win) return;
    int32_t fa = -1, frs = -1, fre = 0, fm = 0, fl = 0;
    for (int a = start_adp ? start_adp[w] : 0; a < n_adp; ++a) {
        const int64_t i = (int64_t)a * n_win + w;
        const int rs = res[0 * stride + i];
        const int m = res[5 * stride + i], l2 = res[7 * stride + i];
        const double full = (rs == -1) ? 0.0 : pcabi::pid6(m, l2);
        if (!(full < thr)) {   // Python: `if full < middle_threshold: break` (NaN does not break)
            fa = a; frs = rs; fre = res[1 * stride + i]; fm = m; fl = l2;
            break;
        }
    }
    hits[0 * hit_stride + w] = fa;
    hits[1 * hit_stride + w] = frs;
    hits[2 * hit_stride + w] = fre;
    hits[3 * hit_stride + w] = fm;
    hits[4 * hit_stride + w] = fl;
}


// The reads with their end adapters trimmed (nanopore_read.py:44-49,
// get_seq_with_start_end_adapters_trimmed): the slice seq[start_trim : len - end_trim] with Python's
// rules, as trimmed_bounds (porechop_abi.py) gives it on the host -- a negative stop (an end trim
// longer than the read: a read shorter than end_size) counts from the end, both ends are clipped,
// and the view is empty when they meet.
__global__ __launch_bounds__(256) void k_trim_views(const int64_t *read_off, const int32_t *read_len,
                                                    const int32_t *start_trim, const int32_t *end_trim, int64_t n,
                                                    int64_t *view_off, int32_t *view_len) {
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256) {
        const int64_t len = read_len[k], st = start_trim[k];
        int64_t stop = len - end_trim[k];
        if (stop < 0) stop += len;
        stop = min(max(stop, (int64_t)0), len);
        view_off[k] = read_off[k] + st;
        view_len[k] = (int32_t)max(stop - min(st, len), (int64_t)0);
    }
}

// ---- launch plumbing -------------------------------------------------------------------------

// Tile layout of a window list (cross mode): windows [256t, 256t + 256) form tile t; dword
// (t, q, lane) = codes 4q..4q+3 of window 256t + lane, at tiles[tile_off[t] + 256q + lane].
// Zero past each window's end. Thread = window: it loads its window's 64-byte slab (17 dwords,
// independent loads, any offset: a byte funnel shift) and writes its 16 dwords down the tile's
// rows, so every row store of a wave is 256 contiguous bytes. (r01-r05: 16 threads per window and
// an LDS transpose, each thread 16 dependent load chains in turn: 25 us per 100k 150-bp windows.)
// grid (n_tiles, <= 1024): blockIdx.y strides over 16-chunk slabs.
__global__ __launch_bounds__(256) void k_tile_windows(const uint8_t *codes, const int64_t *win_off,
                                                      const int32_t *win_len, int64_t n_win,
                                                      const int64_t *tile_off, uint32_t *tiles) {
    const int64_t t = blockIdx.x;
    const int64_t base = tile_off[t];
    const int64_t nq = (tile_off[t + 1] - base) / 256;
    const int64_t w = t * 256 + threadIdx.x;
    int64_t n = 0;
    const uint8_t *wb = codes;
    if (w < n_win) {
        n = max(win_len[w], 0);
        wb = codes + win_off[w];
    }
    for (int64_t q0 = (int64_t)blockIdx.y * 16; q0 < nq; q0 += (int64_t)gridDim.y * 16) {
        const int64_t c0 = 4 * q0;
        const int64_t avail = n - c0;                 // window bytes from column c0 on
        const uint8_t *b = wb + c0;
        const int sh = (int)((uintptr_t)b & 3);
        const uint32_t *q = reinterpret_cast<const uint32_t *>(b - sh);
        uint32_t d[17];
#pragma unroll
        for (int k = 0; k < 17; ++k) d[k] = (avail > 0 && 4 * k < avail + sh) ? q[k] : 0u;   // dwords holding window bytes
        const int nqq = (int)std::min<int64_t>(16, nq - q0);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (k >= nqq) break;
            uint32_t v = sh ? __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh) : d[k];
            const int64_t rem = avail - 4 * k;
            v = rem >= 4 ? v : (rem > 0 ? v & ((1u << (8 * rem)) - 1u) : 0u);
            tiles[base + (q0 + k) * 256 + threadIdx.x] = v;
        }
    }
}

}  // namespace

namespace pcabi_eng {   // (pcabi_host.h: the middle scan uses these too)

int64_t tile_layout(const int32_t *win_len, int64_t n_win, int64_t *tile_off, int64_t *max_nq) {
    const int64_t n_tiles = (n_win + 255) / 256;
    int64_t off = 0, mq = 0;
    for (int64_t t = 0; t < n_tiles; ++t) {
        int32_t mx = 0;
        for (int64_t w = t * 256; w < std::min<int64_t>(n_win, t * 256 + 256); ++w) mx = std::max(mx, win_len[w]);
        const int64_t nq = (mx + 3) / 4 + 2;   // + the reader's one-chunk-ahead fetch
        tile_off[t] = off;
        off += nq * 256;
        mq = std::max(mq, nq);
    }
    tile_off[n_tiles] = off;
    if (max_nq) *max_nq = mq;
    return off;
}

void launch_tiles(const uint8_t *codes, const int64_t *win_off, const int32_t *win_len, int64_t n_win,
                  const int64_t *tile_off, int64_t max_nq, uint32_t *tiles, hipStream_t st) {
    const int64_t n_tiles = (n_win + 255) / 256;
    if (n_tiles == 0) return;
    const dim3 grid((unsigned)n_tiles, (unsigned)std::min<int64_t>(std::max<int64_t>((max_nq + 15) / 16, 1), 1024));
    hipLaunchKernelGGL(k_tile_windows, grid, dim3(256), 0, st, codes, win_off, win_len, n_win, tile_off, tiles);
}

// Buckets the chunked candidate DP serves: the packed core's (FAST buckets laid out packed, WIDE)
// and the generic and striped cores' (long adapters).
bool chunkable(int b, bool packed) {
    return kBuckets[b].kind == WIDE || kBuckets[b].kind == LONG || kBuckets[b].kind == GENERIC ||
           kBuckets[b].kind == STRIPED || (kBuckets[b].kind == FAST && packed);
}

// Lanes per window of the row-split core (k_align_split) for a cross-mode launch of `waves`
// waves: 4 (2 under 16 rows) for launches under 1024 waves, else 1 (the one-lane core).
// PCABI_SPLIT=0 turns the split off, 2 / 4 force it (tests: the split core on any launch). The split costs ~1.3-1.7x the VALU work per
// cell (the per-step exchange and bookkeeping over R / K rows), so it pays only where a launch is
// latency-bound on its own: r04 A/B (profiles/r04/split_ab/), a threshold of 4096 waves split the
// headline's one-adapter buckets (1,564 waves), which run beside the other side's buckets anyway:
// 7.78 -> 7.98 ms per step; the set search of 10k reads (156 waves per adapter) gained 2.79 ->
// 2.53 ms.
int split_lanes(int rpl, int64_t waves) {
    const char *e = std::getenv("PCABI_SPLIT");
    const int forced = (e && e[0]) ? std::atoi(e) : -1;
    int K = 1;
    if (forced >= 0) K = forced;
    else if (waves < 1024) K = rpl < 16 ? 2 : 4;
    return (K == 2 || K == 4) && pcabi::split_ok(rpl, K) ? K : 1;
}

// packed: bucket_pack_mode (0 untagged cores off, 1 packed key layout, 2 run-tagged layout)
int dispatch(int b, const KParams &p, bool affine, hipStream_t st, int packed) {
    if (kBuckets[b].kind == STRIPED) return launch_striped(p, affine, st);
    const int64_t tiles8 = (p.n_win + 8 * 256 - 1) / (8 * 256) * 8;   // window tiles, padded to 8
    dim3 grid = p.task_win ? dim3((unsigned)((p.n_waves + 3) / 4))
                           : dim3((unsigned)(tiles8 * p.n_adp));
    const BucketDef d = kBuckets[b];
    if (!p.task_win && !p.compat && packed && d.kind == FAST && d.rpl <= 64) {
        // a launch too small to fill the chip: K lanes per window (pcabi_dp.h LaneSplit)
        const int K = split_lanes(d.rpl, (p.n_win + 255) / 256 * 4 * (int64_t)p.n_adp);
        if (K > 1 && dispatch_split(d.rpl, K, p, affine, packed == 2, st)) return 0;
    }
    if (d.kind == LONG || d.kind == WIDE || (d.kind == FAST && packed && d.rpl > 32))
        dispatch_packed_large(d.rpl, d.kind == LONG, p, affine, grid, st);
    else if (d.kind == FAST && packed)
        dispatch_packed_small(d.rpl, p, affine, grid, st, packed == 2);
    else
        dispatch_fast(d.rpl, d.kind == GENERIC, p, affine, grid, st);
    return 0;
}

// Packed-key kernels serve a fast bucket when every adapter in it satisfies the range
// conditions of pcabi_dp.h packed_ok (any window length).
bool bucket_packed_ok(int b, const std::vector<int32_t> &lens, const pcabi::Scoring &sc) {
    if (kBuckets[b].kind == WIDE || kBuckets[b].kind == LONG) return true;   // assigned only when packed_ok / long_ok holds
    if (kBuckets[b].kind != FAST || kBuckets[b].rpl > pcabi::pk::MAX_RPL) return false;
    for (int32_t L : lens)
        if (!pcabi::packed_ok(L, kBuckets[b].rpl, sc)) return false;
    return true;
}

// How k_align serves a bucket: 0 = not packed (fast / generic cores), 1 = packed key layout,
// 2 = the run-tagged layout (pcabi_dp.h pk::LayT: affine buckets of <= 32 rows whose adapters all
// pass layt_ok; one VALU op per cell less).
int bucket_pack_mode(int b, const std::vector<int32_t> &lens, const pcabi::Scoring &sc) {
    if (!bucket_packed_ok(b, lens, sc)) return 0;
    if (kBuckets[b].kind != FAST || kBuckets[b].rpl > 32) return 1;
    for (int32_t L : lens)
        if (!pcabi::layt_ok(L, kBuckets[b].rpl, sc)) return 1;
    return 2;
}

}  // namespace pcabi_eng

namespace {

// Whether a cross-mode launch of a run-tagged bucket (bucket_pack_mode 2) runs its inner columns in
// the gap-extend frame (pcabi_dp.h pk::LayS): every adapter passes shift_ok, at one period (the
// largest every adapter allows) and one bias (the middle of the ranges' intersection). Sets
// p.shift_p / p.shift_b (0: the bucket keeps LayT). The chunk, split and pairs launches keep LayT.
void bucket_shift(int b, const std::vector<int32_t> &lens, const pcabi::Scoring &sc, int pack_mode, KParams &p) {
    p.shift_p = p.shift_b = 0;
    if (pack_mode != 2 || lens.empty() || sc.go == sc.ge) return;
    const char *e = std::getenv("PCABI_SHIFT");   // PCABI_SHIFT=0: every bucket keeps LayT (A/B measurements)
    if (e && e[0] == '0') return;
    const int rpl = kBuckets[b].rpl;
    for (int P = pcabi::shift_pmax(rpl); P >= 2; P >>= 1) {
        int lo = INT32_MIN, hi = INT32_MAX;
        bool ok = true;
        for (int32_t L : lens) {
            int blo, bhi;
            if (!pcabi::shift_range(L, rpl, sc, P, blo, bhi)) { ok = false; break; }
            lo = std::max(lo, blo);
            hi = std::min(hi, bhi);
        }
        if (ok && lo <= hi) {
            p.shift_p = P;
            p.shift_b = lo + (hi - lo) / 2;
            return;
        }
    }
}

// Host-side layout of a bucket's adapter table.
struct BucketHost {
    std::vector<uint8_t> pad;   // n * RPL bytes (striped: n * rt)
    std::vector<int32_t> len, id;
    int rt = 0;                 // striped: table rows per adapter
};

// At most this many FAST buckets per adapter table: a cross product launches its buckets side by
// side (the caller's stream + SideStreams::N), and a bucket of one or two adapters is too small
// a grid to fill the GPU on its own.
constexpr int kMaxFastBuckets = 4;

// Bucket of every adapter: its own register bucket, then the cheapest merges of a FAST bucket
// into the next larger non-empty one (cost = adapters x added padding rows) until at most
// kMaxFastBuckets remain. Only merges the packed core can serve with the scoring `sc` (it
// passes scores through any number of padding rows; the fast core allows at most 3).
// all_striped: every adapter on the striped core (needs_striped: long windows under a scoring
// with no path-span bound).
std::vector<int> assign_buckets(const int32_t *adp_len, int32_t n_adp, const pcabi::Scoring &sc, bool merge,
                                bool allow_wide, bool all_striped = false) {
    std::vector<int> b_of(n_adp);
    int count[kNumBuckets] = {};
    for (int a = 0; a < n_adp; ++a) {
        b_of[a] = all_striped ? kStripedBucket : bucket_of(adp_len[a], sc, allow_wide);
        ++count[b_of[a]];
    }
    if (all_striped) return b_of;
    auto packed_all = [&](int b, int extra_from) {
        for (int a = 0; a < n_adp; ++a)
            if ((b_of[a] == b || b_of[a] == extra_from) && !pcabi::packed_ok(adp_len[a], kBuckets[b].rpl, sc))
                return false;
        return true;
    };
    const int max_fast = kMaxFastBuckets;
    while (merge) {
        std::vector<int> fast;
        for (int b = 0; b < kNumBuckets; ++b)
            if (count[b] && kBuckets[b].kind == FAST) fast.push_back(b);
        if ((int)fast.size() <= max_fast) break;
        int best = -1;
        int64_t best_cost = 0;
        for (size_t k = 0; k + 1 < fast.size(); ++k) {
            const int i = fast[k], j = fast[k + 1];
            // more than 3 padding rows: only the packed core passes scores through them
            if (!packed_all(j, i)) continue;
            const int64_t cost = (int64_t)count[i] * (kBuckets[j].rpl - kBuckets[i].rpl);
            if (best < 0 || cost < best_cost) { best = (int)k; best_cost = cost; }
        }
        if (best < 0) break;
        const int i = fast[best], j = fast[best + 1];
        for (int a = 0; a < n_adp; ++a)
            if (b_of[a] == i) b_of[a] = j;
        count[j] += count[i];
        count[i] = 0;
    }
    return b_of;
}

void build_buckets(const uint8_t *adp_codes, const int32_t *adp_off, const int32_t *adp_len,
                   int32_t n_adp, const pcabi::Scoring &sc, BucketHost (&bk)[kNumBuckets], bool merge = true,
                   bool allow_wide = true, bool all_striped = false) {
    const std::vector<int> b_of = assign_buckets(adp_len, n_adp, sc, merge, allow_wide, all_striped);
    for (int a = 0; a < n_adp; ++a)
        if (b_of[a] == kStripedBucket)
            bk[kStripedBucket].rt = std::max(bk[kStripedBucket].rt, (adp_len[a] + kStripeTab - 1) / kStripeTab * kStripeTab);
    for (int a = 0; a < n_adp; ++a) {
        const int L = adp_len[a];
        const int b = b_of[a];
        const int R = b == kStripedBucket ? bk[b].rt : kBuckets[b].rpl;
        BucketHost &h = bk[b];
        const size_t base = h.pad.size();
        h.pad.resize(base + R, (uint8_t)pcabi::PAD_CODE);
        const int off = R - L;
        for (int k = 0; k < L; ++k) h.pad[base + off + k] = adp_codes[adp_off[a] + k];
        h.len.push_back(L);
        h.id.push_back(a);
    }
}

}  // namespace

// error channel shared with the host I/O unit (csrc/pcabi_io.cpp)
namespace pcabi_internal {
int fail(int code, const std::string &msg) { return pcabi_eng::fail(code, msg); }
}  // namespace pcabi_internal

// ---- prepared adapter tables (device) ---------------------------------------------------------
std::atomic<uint64_t> g_table_serial{0};   // struct pcabi_adapters: pcabi_host.h

// the scratch generation (pcabi_scratch.h)
std::atomic<uint64_t> g_buf_gen{0};

// Debug switch PCABI_POISON: every fresh scratch allocation and every growth (Scratch, the shadow
// arena, the stream-ordered scratch of the epilogues and the striped core)
// is filled with one byte before use, so a kernel or host path that reads scratch nothing wrote
// sees garbage instead of the zeros fresh hipMalloc memory usually holds (the
// r05 `need2` read went unnoticed for that reason). "1" fills 0xFF (every int -1); a hex byte such
// as "0x3f" fills that byte (0x3f: every int32 / int64 a huge positive count whose growth arithmetic
// -- need + need / 4 -- does not overflow; 0x7f wrapped there and hid the r05 need2 read).
int pcabi_poison_byte() {
    static const int b = [] {
        const char *e = std::getenv("PCABI_POISON");
        if (!e || !e[0] || (e[0] == '0' && !e[1])) return -1;
        if (e[0] == '1' && !e[1]) return 0xFF;
        return (int)(std::strtol(e, nullptr, 0) & 0xFF);
    }();
    return b;
}
void pcabi_poison(void *p, size_t bytes) {
    if (pcabi_poison_byte() < 0 || !p || !bytes) return;
    (void)hipMemset(p, pcabi_poison_byte(), bytes);
    (void)hipDeviceSynchronize();
}
void pcabi_poison_async(void *p, size_t bytes, hipStream_t st) {
    if (pcabi_poison_byte() >= 0 && p && bytes) (void)hipMemsetAsync(p, pcabi_poison_byte(), bytes, st);
}

namespace {
using DeviceBuf = Scratch<uint8_t>;   // Engine's buffers: bytes, cast at their uses
}  // namespace

namespace pcabi_eng {

// Side streams of a device for the fork / join of pcabi_align_cross_dev's bucket launches. A fork
// region takes its side streams from a rotating start, so two regions queued back to back (the
// headline's two sides, each a cross product on its own caller stream) use different side streams
// and their launches overlap (r04 trace: with 3 shared side streams the end side's small buckets
// queued behind the start side's).
struct SideStreams {
    static constexpr int N = 6;
    std::mutex mu;               // one fork / join region at a time per device
    bool init = false;
    int next = 0;                // the next region's first side stream
    hipStream_t s[N] = {};
    hipEvent_t fork = nullptr, join[N] = {};
};
SideStreams g_side[16];
std::mutex g_side_mu;

int side_streams(int dev, SideStreams **out) {
    if (dev < 0 || dev >= 16) return fail(PCABI_E_ARG, "bad device index");
    std::lock_guard<std::mutex> g(g_side_mu);
    SideStreams &ss = g_side[dev];
    if (!ss.init) {
        // plain streams on the process's GPU_MAX_HW_QUEUES (side streams with a CU mask, a hardware
        // queue each, measured slower in r04n)
        for (int i = 0; i < SideStreams::N; ++i) {
            HIP_TRY(hipStreamCreateWithFlags(&ss.s[i], hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&ss.join[i], hipEventDisableTiming));
        }
        HIP_TRY(hipEventCreateWithFlags(&ss.fork, hipEventDisableTiming));
        ss.init = true;
    }
    *out = &ss;
    return 0;
}

// pcabi_set_side_streams: whether fork / join regions use the side streams (initially on)
constexpr int kSideStreamsDefault = 1;
std::atomic<int> g_side_on{kSideStreamsDefault};
bool side_streams_on() { return g_side_on.load(std::memory_order_relaxed) != 0; }

// Per-stream setting (pcabi_stream_side_streams, r05): a caller that runs cross products on several
// streams at once turns the side streams off for ITS streams only; streams without an entry follow
// the process-wide default (pcabi_set_side_streams).
std::mutex g_stream_side_mu;
std::vector<std::pair<hipStream_t, int>> g_stream_side;   // few entries: a linear scan
bool side_streams_on(hipStream_t st) {
    {
        std::lock_guard<std::mutex> g(g_stream_side_mu);
        for (const auto &e : g_stream_side)
            if (e.first == st) return e.second != 0;
    }
    return side_streams_on();
}

// ForkJoin (pcabi_host.h)
int ForkJoin::begin(hipStream_t m, size_t n_launch) {
    main = m;
    if (n_launch <= 1 || !side_streams_on(m)) return 0;  // off: every launch on the caller's stream
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (int rc = side_streams(dev, &ss)) return rc;
    lock = std::unique_lock<std::mutex>(ss->mu);
    first = ss->next;
    HIP_TRY(hipEventRecord(ss->fork, main));
    return 0;
}
hipStream_t ForkJoin::at(size_t k) {
    if (k == 0 || !ss) return main;
    const int i = (int)((first + k - 1) % SideStreams::N);
    if (!(used & (1u << i))) (void)hipStreamWaitEvent(ss->s[i], ss->fork, 0);
    used |= 1u << i;
    n_side = std::max(n_side, (int)k);
    return ss->s[i];
}
int ForkJoin::end() {
    for (int i = 0; i < SideStreams::N; ++i) {
        if (!(used & (1u << i))) continue;
        HIP_TRY(hipEventRecord(ss->join[i], ss->s[i]));
        HIP_TRY(hipStreamWaitEvent(main, ss->join[i], 0));
    }
    if (ss && n_side) ss->next = (first + n_side) % SideStreams::N;
    used = 0;
    n_side = 0;
    if (lock.owns_lock()) lock.unlock();
    return 0;
}

}  // namespace pcabi_eng

namespace {

// Per-device state for the host-buffer API (serialised by a mutex: the legacy ABI is called
// concurrently from the reference's ThreadPool workers, porechop_abi.py:228,418,504).
struct Engine {
    std::mutex mu;
    bool init = false;
    hipStream_t stream = nullptr;
    DeviceBuf codes, woff, wlen, out, tasks_win, tasks_out, wave_adp, tiles, toff, hits, bc;
    pcabi_scan *scan = nullptr;   // scratch of the middle scan (pcabi_middle_scan_host)
    DeviceBuf pad[kNumBuckets], len[kNumBuckets], id[kNumBuckets];
    // pcabi_end_decisions_host: both sides' windows, results, trims, flags and lists; the two
    // sides' prepared adapter tables, kept while the adapters and the scoring stay the same
    DeviceBuf dec[17];
    // pcabi_middle_scan_seqs: pinned staging slots the host strings are encoded into while the
    // previous slots' copies run (allocated on first use, kept)
    uint8_t *stage[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t stage_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    DeviceBuf stage_dev;          // the slots' device copies (2-bit codes + N masks), unpacked into place
    struct DTab {
        std::vector<uint8_t> codes;
        std::vector<int32_t> lens;
        pcabi::Scoring sc{0, 0, 0, 0};
        pcabi_adapters *t = nullptr;
    } dtab[2];
};

// Never destroyed: the buffers free themselves, and a destructor run at process exit would call
// hipFree after the HIP runtime is gone.
Engine *const g_engines = new Engine[16];

int engine_init(Engine &e, int device) {
    if (e.init) return 0;
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(PCABI_E_DEVICE, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950");
    HIP_TRY(hipStreamCreateWithFlags(&e.stream, hipStreamNonBlocking));
    e.init = true;
    return 0;
}

int check_common(const int32_t *adp_len, int32_t n_adp) {
    for (int a = 0; a < n_adp; ++a)
        if (adp_len[a] < 1 || adp_len[a] > pcabi::MAX_STRIPED_LEN)
            return fail(PCABI_E_ARG, "adapter length " + std::to_string(adp_len[a]) + " outside 1.." +
                                         std::to_string(pcabi::MAX_STRIPED_LEN));
    return 0;
}

// The register cores keep the path's start column mod 2^16 (pcabi_dp.h attribute word), which
// is exact only when every window is short or the path span is bounded (gap costs < 0). Any
// other scoring the reference accepts (arg_parser.py:229-236: any four integers, e.g. gap costs
// >= 0) on windows of 32 k and more runs on the striped core instead, whose two-word attributes
// never wrap (align_lane_striped): true when that routing is needed.
bool needs_striped(const pcabi::Scoring &sc, int max_L, int64_t max_win) {
    if (max_win < 32768 - 256) return false;
    const int b = pcabi::span_bound(max_L, sc.ma, sc.mi, sc.go, sc.ge);
    return b < 0 || b + max_L >= 32768;
}

}  // namespace

extern "C" {

const char *pcabi_last_error(void) { return g_err.c_str(); }
int pcabi_version(void) { return 1; }
int pcabi_max_adapter_len(void) { return pcabi::MAX_STRIPED_LEN; }
int pcabi_max_window_len(void) { return pcabi::MAX_WINDOW_LEN; }

int pcabi_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void pcabi_encode_dna5(const char *ascii, uint8_t *codes, int64_t n) {
    static const struct Tab {
        uint8_t t[256];
        Tab() {
            for (int c = 0; c < 256; ++c) t[c] = 4;
            t['A'] = t['a'] = 0;
            t['C'] = t['c'] = 1;
            t['G'] = t['g'] = 2;
            t['T'] = t['t'] = t['U'] = t['u'] = 3;
        }
    } tab;
    auto run = [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) codes[i] = tab.t[(unsigned char)ascii[i]];
    };
    // whole batches of reads (hundreds of MB from the Python drivers) on up to 16 host threads
    const int64_t per = 8 << 20;
    const int nt = (int)std::min<int64_t>(16, std::max<int64_t>(1, n / per));
    if (nt <= 1) {
        run(0, n);
        return;
    }
    std::vector<std::thread> th;
    for (int k = 0; k < nt; ++k) th.emplace_back(run, n * k / nt, n * (k + 1) / nt);
    for (auto &t : th) t.join();
}

void pcabi_pid6_host(const int32_t *m, const int32_t *l, int64_t n, double *out) {
    for (int64_t k = 0; k < n; ++k) out[k] = pcabi::pid6(m[k], l[k]);
}

}  // extern "C"

namespace {

// Shared body of pcabi_align_host / pcabi_first_hits_host. first_thr != nullptr (cross mode
// only): out receives the k_first_hit fields (5 x n_win) instead of the raw results.
// All-vs-all link matrix from the cross product f[a * n + w] (window w as row 0, sequence a as
// rows): per pair the reference's orientation (row 0 = the longer, ties -> the first argument of
// consensus.py:90-97, i < j), mirrored; -1 on the diagonal. 32 x 32 tiles through LDS so both
// the direct and the transposed reads are coalesced.
__global__ __launch_bounds__(256) void k_orient(const int32_t *f, const int32_t *len, int64_t n, int32_t *mat) {
    __shared__ int32_t direct[32][33], trans[32][33];
    const int64_t r0 = (int64_t)blockIdx.y * 32, c0 = (int64_t)blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8 threads
    for (int y = ty; y < 32; y += 8) {
        const int64_t r = r0 + y, c = c0 + tx;
        direct[y][tx] = (r < n && c < n) ? f[r * n + c] : 0;
        const int64_t rt = c0 + y, ct = r0 + tx;                 // f[c][r] for the tile, row-wise
        trans[tx][y] = (rt < n && ct < n) ? f[rt * n + ct] : 0;
    }
    __syncthreads();
    for (int y = ty; y < 32; y += 8) {
        const int64_t r = r0 + y, c = c0 + tx;
        if (r >= n || c >= n) continue;
        int32_t v = -1;
        if (r != c) {
            const int64_t i = r < c ? r : c, j = r < c ? c : r;
            // want f[j * n + i] when len[i] >= len[j], else f[i * n + j]
            const bool from_j = len[i] >= len[j];
            const bool j_is_r = (j == r);
            v = (from_j == j_is_r) ? direct[y][tx] : trans[y][tx];
        }
        mat[r * n + c] = v;
    }
}

int align_host_impl(int device, const uint8_t *codes, int64_t codes_len, const int64_t *win_off,
                    const int32_t *win_len, int64_t n_win, const uint8_t *adp_codes,
                    const int32_t *adp_off, const int32_t *adp_len, int32_t n_adp,
                    const int32_t *task_win, const int32_t *task_adp, int64_t n_task, int match,
                    int mismatch, int gap_open, int gap_extend, const double *first_thr, int32_t *out,
                    bool compat = false, bool orient = false, double *best = nullptr, bool best_dev = false) {
    if (device < 0 || device >= 16) return fail(PCABI_E_ARG, "bad device index");
    if (n_win < 0 || n_adp < 0 || n_task < 0) return fail(PCABI_E_ARG, "negative count");
    if (int rc = check_common(adp_len, n_adp)) return rc;
    for (int64_t w = 0; w < n_win; ++w) {
        if (win_len[w] < 0 || win_len[w] > pcabi::MAX_WINDOW_LEN)
            return fail(PCABI_E_ARG, "window length out of range");
        if (win_len[w] > 0 && (win_off[w] < 0 || win_off[w] + win_len[w] + 16 > codes_len))
            return fail(PCABI_E_ARG, "window outside the buffer or buffer not padded by 16 bytes");
    }
    const int64_t n_res = task_win ? n_task : (int64_t)n_adp * n_win;
    if (task_win)
        for (int64_t t = 0; t < n_task; ++t)
            if (task_win[t] < 0 || task_win[t] >= n_win || task_adp[t] < 0 || task_adp[t] >= n_adp)
                return fail(PCABI_E_ARG, "task index out of range");
    if (n_res == 0) return 0;

    Engine &e = g_engines[device];
    std::lock_guard<std::mutex> lock(e.mu);
    if (int rc = engine_init(e, device)) return rc;
    HIP_TRY(hipSetDevice(device));

    const pcabi::Scoring sc{match, mismatch, gap_open, gap_extend};
    int64_t max_win = 0;
    bool striped_only = false;
    {
        int max_L = 0;
        for (int a = 0; a < n_adp; ++a)
            if (adp_len[a] <= kMaxRPL) max_L = std::max(max_L, (int)adp_len[a]);   // striped: c never wraps
        for (int64_t w = 0; w < n_win; ++w) max_win = std::max<int64_t>(max_win, win_len[w]);
        striped_only = needs_striped(sc, max_L, max_win);
    }
    BucketHost bk[kNumBuckets];
    build_buckets(adp_codes, adp_off, adp_len, n_adp, sc, bk, true, true, striped_only);

    if (int rc = e.codes.ensure((size_t)codes_len)) return rc;
    if (int rc = e.woff.ensure(sizeof(int64_t) * (size_t)std::max<int64_t>(n_win, 1))) return rc;
    if (int rc = e.wlen.ensure(sizeof(int32_t) * (size_t)std::max<int64_t>(n_win, 1))) return rc;
    if (int rc = e.out.ensure(sizeof(int32_t) * PCABI_NFIELDS * (size_t)n_res)) return rc;
    HIP_TRY(hipMemcpyAsync(e.codes.p, codes, (size_t)codes_len, hipMemcpyHostToDevice, e.stream));
    HIP_TRY(hipMemcpyAsync(e.woff.p, win_off, sizeof(int64_t) * (size_t)n_win, hipMemcpyHostToDevice, e.stream));
    HIP_TRY(hipMemcpyAsync(e.wlen.p, win_len, sizeof(int32_t) * (size_t)n_win, hipMemcpyHostToDevice, e.stream));

    KParams p{};
    p.codes = (const uint8_t *)e.codes.p;
    p.win_off = (const int64_t *)e.woff.p;
    p.win_len = (const int32_t *)e.wlen.p;
    p.n_win = n_win;
    p.out = (int32_t *)e.out.p;
    p.out_stride = n_res;
    p.sc = sc;
    p.compat = compat ? (int32_t *)e.out.p : nullptr;   // pairs mode only (checked by the caller)
    const bool affine = gap_open != gap_extend;

    // host-side pair grouping (pairs mode): per bucket, per adapter, runs padded to 64 lanes
    std::vector<std::vector<int32_t>> per_adp;
    if (task_win) {
        per_adp.resize(n_adp);
        for (int64_t t = 0; t < n_task; ++t) per_adp[task_adp[t]].push_back((int32_t)t);
        // longest windows first: lanes of a wave then run near-equal column counts
        for (auto &v : per_adp)
            std::stable_sort(v.begin(), v.end(), [&](int32_t x, int32_t y) {
                return win_len[task_win[x]] > win_len[task_win[y]];
            });
    }
    std::vector<int32_t> tw, to, wa;
    struct CrossLaunch {
        int b;
        KParams p;
        int packed;   // bucket_pack_mode
    };
    std::vector<CrossLaunch> cross;
    for (int b = 0; b < kNumBuckets; ++b) {
        BucketHost &h = bk[b];
        if (h.len.empty()) continue;
        const int nb = (int)h.len.size();
        if (int rc = e.pad[b].ensure(h.pad.size())) return rc;
        if (int rc = e.len[b].ensure(sizeof(int32_t) * nb)) return rc;
        if (int rc = e.id[b].ensure(sizeof(int32_t) * nb)) return rc;
        HIP_TRY(hipMemcpyAsync(e.pad[b].p, h.pad.data(), h.pad.size(), hipMemcpyHostToDevice, e.stream));
        HIP_TRY(hipMemcpyAsync(e.len[b].p, h.len.data(), sizeof(int32_t) * nb, hipMemcpyHostToDevice, e.stream));
        HIP_TRY(hipMemcpyAsync(e.id[b].p, h.id.data(), sizeof(int32_t) * nb, hipMemcpyHostToDevice, e.stream));
        p.adp_pad = (const uint32_t *)e.pad[b].p;
        p.adp_len = (const int32_t *)e.len[b].p;
        p.adp_id = (const int32_t *)e.id[b].p;
        p.n_adp = nb;
        p.rt = h.rt;
        p.max_cols = (int32_t)std::min<int64_t>(max_win, INT32_MAX);
        if (!task_win) {
            p.task_win = nullptr;
            if (n_win > 0 && !p.tiles) {
                std::vector<int64_t> toff((size_t)((n_win + 255) / 256 + 1));
                int64_t max_nq = 0;
                const int64_t nd = tile_layout(win_len, n_win, toff.data(), &max_nq);
                if (int rc = e.toff.ensure(sizeof(int64_t) * toff.size())) return rc;
                if (int rc = e.tiles.ensure(sizeof(uint32_t) * (size_t)nd)) return rc;
                HIP_TRY(hipMemcpyAsync(e.toff.p, toff.data(), sizeof(int64_t) * toff.size(), hipMemcpyHostToDevice, e.stream));
                launch_tiles(p.codes, p.win_off, p.win_len, n_win, (const int64_t *)e.toff.p, max_nq,
                             (uint32_t *)e.tiles.p, e.stream);
                // toff (host) must outlive the async copy
                HIP_TRY(hipStreamSynchronize(e.stream));
                p.tiles = (const uint32_t *)e.tiles.p;
                p.tile_off = (const int64_t *)e.toff.p;
            }
            // launched below, side by side once every bucket's table is on its way
            if (n_win > 0) {
                const int pack = bucket_pack_mode(b, h.len, sc);
                bucket_shift(b, h.len, sc, pack, p);
                cross.push_back({b, p, pack});
            }
        } else {
            tw.clear(); to.clear(); wa.clear();
            for (int k = 0; k < nb; ++k) {
                const std::vector<int32_t> &ts = per_adp[h.id[k]];
                for (size_t s = 0; s < ts.size(); s += 64) {
                    wa.push_back(k);
                    for (size_t q = 0; q < 64; ++q) {
                        if (s + q < ts.size()) { tw.push_back(task_win[ts[s + q]]); to.push_back(ts[s + q]); }
                        else { tw.push_back(-1); to.push_back(0); }
                    }
                }
            }
            if (wa.empty()) continue;
            // the per-bucket task arrays must stay alive until the kernel has read them
            if (int rc = e.tasks_win.ensure(sizeof(int32_t) * tw.size())) return rc;
            if (int rc = e.tasks_out.ensure(sizeof(int32_t) * to.size())) return rc;
            if (int rc = e.wave_adp.ensure(sizeof(int32_t) * wa.size())) return rc;
            HIP_TRY(hipMemcpyAsync(e.tasks_win.p, tw.data(), sizeof(int32_t) * tw.size(), hipMemcpyHostToDevice, e.stream));
            HIP_TRY(hipMemcpyAsync(e.tasks_out.p, to.data(), sizeof(int32_t) * to.size(), hipMemcpyHostToDevice, e.stream));
            HIP_TRY(hipMemcpyAsync(e.wave_adp.p, wa.data(), sizeof(int32_t) * wa.size(), hipMemcpyHostToDevice, e.stream));
            p.task_win = (const int32_t *)e.tasks_win.p;
            p.task_out = (const int32_t *)e.tasks_out.p;
            p.wave_adp = (const int32_t *)e.wave_adp.p;
            p.n_waves = (int64_t)wa.size();
            if (int rc = dispatch(b, p, affine, e.stream, bucket_pack_mode(b, h.len, sc))) return rc;
            // host vectors are reused by the next bucket: drain before overwriting
            HIP_TRY(hipStreamSynchronize(e.stream));
        }
        HIP_TRY(hipGetLastError());
        // bucket buffers are reused across calls only; keep them distinct per bucket
    }
    if (!cross.empty()) {
        // the host bucket tables (bk) outlive these launches: they are read by the copies queued
        // on e.stream before the fork
        std::stable_sort(cross.begin(), cross.end(), [&](const CrossLaunch &x, const CrossLaunch &y) {
            return (int64_t)x.p.n_adp * kBuckets[x.b].rpl > (int64_t)y.p.n_adp * kBuckets[y.b].rpl;
        });
        ForkJoin fj;
        if (int rc = fj.begin(e.stream, cross.size())) return rc;
        for (size_t k = 0; k < cross.size(); ++k)
            if (int rc = dispatch(cross[k].b, cross[k].p, affine, fj.at(k), cross[k].packed)) {
                (void)fj.end();
                return rc;
            }
        if (int rc = fj.end()) return rc;
        HIP_TRY(hipGetLastError());
    }
    if (first_thr) {
        if (int rc = e.hits.ensure(sizeof(int32_t) * 5 * (size_t)n_win)) return rc;
        hipLaunchKernelGGL(k_first_hit, dim3((unsigned)((n_win + 255) / 256)), dim3(256), 0, e.stream,
                           (const int32_t *)e.out.p, n_res, n_win, n_adp, *first_thr, nullptr,
                           (int32_t *)e.hits.p, n_win);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out, e.hits.p, sizeof(int32_t) * 5 * (size_t)n_win, hipMemcpyDeviceToHost,
                               e.stream));
    } else if (best) {     // adapter-set search: per-adapter max of the full identity, on the device
        double *d_best = best;
        if (!best_dev) {
            if (int rc = e.hits.ensure(sizeof(double) * (size_t)n_adp)) return rc;
            d_best = (double *)e.hits.p;
            HIP_TRY(hipMemcpyAsync(d_best, best, sizeof(double) * (size_t)n_adp, hipMemcpyHostToDevice, e.stream));
        }
        hipLaunchKernelGGL(k_best_full_id, dim3((unsigned)n_adp), dim3(256), 0, e.stream, (const int32_t *)e.out.p,
                           n_res, n_win, d_best);
        HIP_TRY(hipGetLastError());
        if (!best_dev)
            HIP_TRY(hipMemcpyAsync(best, d_best, sizeof(double) * (size_t)n_adp, hipMemcpyDeviceToHost, e.stream));
    } else if (orient) {   // compat all-vs-all: n_win == n_adp == n, the matrix comes back
        if (int rc = e.hits.ensure(sizeof(int32_t) * (size_t)n_res)) return rc;
        const unsigned tb = (unsigned)((n_win + 31) / 32);
        hipLaunchKernelGGL(k_orient, dim3(tb, tb), dim3(256), 0, e.stream, (const int32_t *)e.out.p,
                           (const int32_t *)e.wlen.p, n_win, (int32_t *)e.hits.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out, e.hits.p, sizeof(int32_t) * (size_t)n_res, hipMemcpyDeviceToHost, e.stream));
    } else {
        HIP_TRY(hipMemcpyAsync(out, e.out.p, sizeof(int32_t) * (compat ? 1 : PCABI_NFIELDS) * (size_t)n_res,
                               hipMemcpyDeviceToHost, e.stream));
    }
    HIP_TRY(hipStreamSynchronize(e.stream));
    return 0;
}

}  // namespace

namespace {
int64_t middle_scan_resident(Engine &e, const int64_t *win_off, const int32_t *win_len, int64_t n_win,
                             const uint8_t *adp_codes, const int32_t *adp_off, const int32_t *adp_len, int32_t n_adp,
                             int match, int mismatch, int gap_open, int gap_extend, double threshold, int32_t *hits,
                             int64_t cap);
int stage_seqs(Engine &e, uint8_t *dst, const char *const *seqs, const int32_t *len, const int64_t *off, int64_t n,
               int64_t total);
}  // namespace

extern "C" {

int pcabi_align_host(int device, const uint8_t *codes, int64_t codes_len, const int64_t *win_off,
                     const int32_t *win_len, int64_t n_win, const uint8_t *adp_codes,
                     const int32_t *adp_off, const int32_t *adp_len, int32_t n_adp,
                     const int32_t *task_win, const int32_t *task_adp, int64_t n_task, int match,
                     int mismatch, int gap_open, int gap_extend, int32_t *out) {
    return align_host_impl(device, codes, codes_len, win_off, win_len, n_win, adp_codes, adp_off, adp_len,
                           n_adp, task_win, task_adp, n_task, match, mismatch, gap_open, gap_extend, nullptr,
                           out);
}

int pcabi_best_full_identity_host(int device, const uint8_t *codes, int64_t codes_len, const int64_t *win_off,
                                  const int32_t *win_len, int64_t n_win, const uint8_t *adp_codes,
                                  const int32_t *adp_off, const int32_t *adp_len, int32_t n_adp, int match,
                                  int mismatch, int gap_open, int gap_extend, double *best, int best_on_device) {
    if (!best && n_adp > 0) return fail(PCABI_E_ARG, "best is NULL");
    if (n_win == 0 || n_adp == 0) return 0;     // no window: every maximum stays as given
    return align_host_impl(device, codes, codes_len, win_off, win_len, n_win, adp_codes, adp_off, adp_len, n_adp,
                           nullptr, nullptr, 0, match, mismatch, gap_open, gap_extend, nullptr, nullptr, false, false,
                           best, best_on_device != 0);
}

int pcabi_first_hits_host(int device, const uint8_t *codes, int64_t codes_len, const int64_t *win_off,
                          const int32_t *win_len, int64_t n_win, const uint8_t *adp_codes,
                          const int32_t *adp_off, const int32_t *adp_len, int32_t n_adp, int match,
                          int mismatch, int gap_open, int gap_extend, double threshold, int32_t *hits) {
    if (n_win > 0 && n_adp == 0) {
        for (int64_t w = 0; w < n_win; ++w) {
            hits[w] = -1; hits[n_win + w] = -1; hits[2 * n_win + w] = 0; hits[3 * n_win + w] = 0;
            hits[4 * n_win + w] = 0;
        }
        return 0;
    }
    return align_host_impl(device, codes, codes_len, win_off, win_len, n_win, adp_codes, adp_off, adp_len,
                           n_adp, nullptr, nullptr, 0, match, mismatch, gap_open, gap_extend, &threshold, hits);
}

int64_t pcabi_middle_scan_host(int device, const uint8_t *codes, int64_t codes_len, const int64_t *win_off,
                               const int32_t *win_len, int64_t n_win, const uint8_t *adp_codes,
                               const int32_t *adp_off, const int32_t *adp_len, int32_t n_adp, int match,
                               int mismatch, int gap_open, int gap_extend, double threshold, int32_t *hits,
                               int64_t cap) {
    if (device < 0 || device >= 16) return fail(PCABI_E_ARG, "bad device index");
    if (n_win < 0 || n_adp < 0 || cap < 0) return fail(PCABI_E_ARG, "negative count");
    if (int rc = check_common(adp_len, n_adp)) return rc;
    for (int64_t w = 0; w < n_win; ++w) {
        if (win_len[w] < 0 || win_len[w] > pcabi::MAX_WINDOW_LEN)
            return fail(PCABI_E_ARG, "window length out of range");
        if (win_len[w] > 0 && (win_off[w] < 0 || win_off[w] + win_len[w] + 16 > codes_len))
            return fail(PCABI_E_ARG, "window outside the buffer or buffer not padded by 16 bytes");
    }
    if (n_win == 0 || n_adp == 0) return 0;
    Engine &e = g_engines[device];
    std::lock_guard<std::mutex> lock(e.mu);
    if (int rc = engine_init(e, device)) return rc;
    HIP_TRY(hipSetDevice(device));
    if (int rc = e.codes.ensure((size_t)codes_len)) return rc;
    HIP_TRY(hipMemcpyAsync(e.codes.p, codes, (size_t)codes_len, hipMemcpyHostToDevice, e.stream));
    return middle_scan_resident(e, win_off, win_len, n_win, adp_codes, adp_off, adp_len, n_adp, match, mismatch,
                                gap_open, gap_extend, threshold, hits, cap);
}

int pcabi_stage_seqs_host(int device, const char *const *seqs, const int32_t *seq_len, int64_t n, uint8_t *out,
                          int64_t out_len) {
    if (device < 0 || device >= 16) return fail(PCABI_E_ARG, "bad device index");
    if (n < 0) return fail(PCABI_E_ARG, "negative count");
    int64_t total = 0;
    std::vector<int64_t> off((size_t)n);
    for (int64_t w = 0; w < n; ++w) {
        if (seq_len[w] < 0 || seq_len[w] > pcabi::MAX_WINDOW_LEN) return fail(PCABI_E_ARG, "window length out of range");
        if (seq_len[w] > 0 && !seqs[w]) return fail(PCABI_E_ARG, "NULL sequence");
        off[(size_t)w] = total;
        total += ((int64_t)seq_len[w] + 3) & ~(int64_t)3;
    }
    total += 16;
    if (out_len < total) return fail(PCABI_E_ARG, "output buffer smaller than the layout");
    Engine &e = g_engines[device];
    std::lock_guard<std::mutex> lock(e.mu);
    if (int rc = engine_init(e, device)) return rc;
    HIP_TRY(hipSetDevice(device));
    if (int rc = e.codes.ensure((size_t)total)) return rc;
    if (int rc = stage_seqs(e, (uint8_t *)e.codes.p, seqs, seq_len, off.data(), n, total)) return rc;
    HIP_TRY(hipMemcpyAsync(out, e.codes.p, (size_t)total, hipMemcpyDeviceToHost, e.stream));
    HIP_TRY(hipStreamSynchronize(e.stream));
    return 0;
}

int64_t pcabi_middle_scan_seqs(int device, const char *const *seqs, const int32_t *seq_len, int64_t n,
                               const uint8_t *adp_codes, const int32_t *adp_off, const int32_t *adp_len,
                               int32_t n_adp, int match, int mismatch, int gap_open, int gap_extend,
                               double threshold, int32_t *hits, int64_t cap) {
    if (device < 0 || device >= 16) return fail(PCABI_E_ARG, "bad device index");
    if (n < 0 || n_adp < 0 || cap < 0) return fail(PCABI_E_ARG, "negative count");
    if (int rc = check_common(adp_len, n_adp)) return rc;
    // the layout of pcabi_middle_scan_host's buffer (and of the Python SeqPack): windows back to
    // back from 4-aligned offsets, N between them and 16 N bytes after the last
    std::vector<int64_t> off((size_t)n);
    int64_t total = 0;
    for (int64_t w = 0; w < n; ++w) {
        if (seq_len[w] < 0 || seq_len[w] > pcabi::MAX_WINDOW_LEN) return fail(PCABI_E_ARG, "window length out of range");
        if (seq_len[w] > 0 && !seqs[w]) return fail(PCABI_E_ARG, "NULL sequence");
        off[(size_t)w] = total;
        total += ((int64_t)seq_len[w] + 3) & ~(int64_t)3;
    }
    total += 16;
    if (n == 0 || n_adp == 0) return 0;
    Engine &e = g_engines[device];
    std::lock_guard<std::mutex> lock(e.mu);
    if (int rc = engine_init(e, device)) return rc;
    HIP_TRY(hipSetDevice(device));
    if (int rc = e.codes.ensure((size_t)total)) return rc;
    if (int rc = stage_seqs(e, (uint8_t *)e.codes.p, seqs, seq_len, off.data(), n, total)) return rc;
    return middle_scan_resident(e, off.data(), seq_len, n, adp_codes, adp_off, adp_len, n_adp, match, mismatch,
                                gap_open, gap_extend, threshold, hits, cap);
}

}  // extern "C"

namespace {

// The middle scan over windows whose codes are in e.codes (being copied there on e.stream).
int64_t middle_scan_resident(Engine &e, const int64_t *win_off, const int32_t *win_len, int64_t n_win,
                             const uint8_t *adp_codes, const int32_t *adp_off, const int32_t *adp_len, int32_t n_adp,
                             int match, int mismatch, int gap_open, int gap_extend, double threshold, int32_t *hits,
                             int64_t cap) {
    if (int rc = e.woff.ensure(sizeof(int64_t) * (size_t)n_win)) return rc;
    if (int rc = e.wlen.ensure(sizeof(int32_t) * (size_t)n_win)) return rc;
    HIP_TRY(hipMemcpyAsync(e.woff.p, win_off, sizeof(int64_t) * (size_t)n_win, hipMemcpyHostToDevice, e.stream));
    HIP_TRY(hipMemcpyAsync(e.wlen.p, win_len, sizeof(int32_t) * (size_t)n_win, hipMemcpyHostToDevice, e.stream));
    pcabi_adapters *tab = nullptr;
    if (int rc = pcabi_adapters_create_scored(adp_codes, adp_off, adp_len, n_adp, match, mismatch, gap_open,
                                              gap_extend, &tab))
        return rc;
    if (!e.scan) {
        if (int rc = pcabi_scan_create(tab, &e.scan)) return rc;
    }
    scan_set_table(e.scan, tab);   // (the kept scan serves each call's own table)
    const int64_t r = pcabi_middle_scan_dev(e.scan, (uint8_t *)e.codes.p, (const int64_t *)e.woff.p,
                                            (const int32_t *)e.wlen.p, win_len, n_win, match, mismatch, gap_open,
                                            gap_extend, threshold, hits, cap, e.stream);
    (void)hipStreamSynchronize(e.stream);
    scan_set_table(e.scan, nullptr);
    pcabi_adapters_destroy(tab);
    return r;
}

// Host strings -> Dna5 codes at dst (device): the layout's bytes [0, total) in chunks of kStageBytes.
// r05: what crosses PCIe is 3 bits a base, not 8 -- each chunk travels as 2-bit codes (base j of
// a 32-base block at bits 2j of its 8 bytes) plus a 1-bit "not A/C/G/T/U" mask (bit j of the
// block's 32-bit word), k_unpack_codes writes the Dna5 bytes (S/basic/alphabet_residue_tabs.h's
// table, as pcabi_encode_dna5: A/a 0, C/c 1, G/g 2, T/t/U/u 3, anything else N = 4) into dst.
// The worker threads gather their share of a chunk's characters (the windows' own bytes, N
// between them) into a thread-local block and encode it with AVX2 (a scalar loop without it) into
// one of four pinned slots; this thread queues each chunk's two copies and its unpack on e.stream
// and waits for a slot only when a worker needs it again. Nothing is written to pageable memory.
constexpr int64_t kStageBytes = 32 << 20;
constexpr int64_t kStageCodes = kStageBytes / 4, kStageMask = kStageBytes / 8, kStageSlot = kStageCodes + kStageMask;

__global__ __launch_bounds__(256) void k_unpack_codes(const uint32_t *__restrict__ codes, const uint32_t *__restrict__ mask,
                                                      uint8_t *__restrict__ dst, int64_t n) {
    // 16 bases a thread: one dword of codes, half a mask word, one 16-byte store
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t b = 16 * q;
    if (b >= n) return;
    const uint32_t c = codes[q];
    const uint32_t m = (mask[q >> 1] >> (16 * (q & 1))) & 0xFFFFu;
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t x = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = 4 * k + j;
            const uint32_t v = (m >> i) & 1u ? 4u : (c >> (2 * i)) & 3u;
            x |= v << (8 * j);
        }
        w[k] = x;
    }
    if (b + 16 <= n) {
        *reinterpret_cast<uint4 *>(dst + b) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (int64_t i = b; i < n; ++i) dst[i] = (uint8_t)(w[(i - b) >> 2] >> (8 * ((i - b) & 3)));
    }
}

// 32 characters -> 8 bytes of 2-bit codes + the 32-bit N mask (the scalar and AVX2 forms agree)
inline void pack32_scalar(const uint8_t *s, uint8_t *codes, uint32_t *mask) {
    uint64_t c = 0;
    uint32_t m = 0;
    for (int j = 0; j < 32; ++j) {
        const uint8_t u = s[j] & 0xDF;
        uint32_t v = 4;
        if (u == 'A') v = 0;
        else if (u == 'C') v = 1;
        else if (u == 'G') v = 2;
        else if (u == 'T' || u == 'U') v = 3;
        if (v == 4) m |= 1u << j;
        else c |= (uint64_t)v << (2 * j);
    }
    std::memcpy(codes, &c, 8);
    *mask = m;
}
__attribute__((target("avx2"))) void pack_avx2(const uint8_t *s, int64_t nblk, uint8_t *codes, uint32_t *mask) {
    const __m256i df = _mm256_set1_epi8((char)0xDF);
    const __m256i kA = _mm256_set1_epi8('A'), kC = _mm256_set1_epi8('C'), kG = _mm256_set1_epi8('G');
    const __m256i kT = _mm256_set1_epi8('T'), kU = _mm256_set1_epi8('U');
    const __m256i one = _mm256_set1_epi8(1), two = _mm256_set1_epi8(2), three = _mm256_set1_epi8(3);
    const __m256i m14 = _mm256_set1_epi16(0x0401);             // bytes (1, 4): c0 + 4 c1
    const __m256i m116 = _mm256_set1_epi32(0x00100001);        // words (1, 16)
    const __m256i sh = _mm256_setr_epi8(0, 4, 8, 12, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
                                        0, 4, 8, 12, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1);
    const __m256i perm = _mm256_setr_epi32(0, 4, 1, 1, 1, 1, 1, 1);
    for (int64_t b = 0; b < nblk; ++b) {
        const __m256i u = _mm256_and_si256(_mm256_loadu_si256(reinterpret_cast<const __m256i *>(s + 32 * b)), df);
        const __m256i eA = _mm256_cmpeq_epi8(u, kA), eC = _mm256_cmpeq_epi8(u, kC), eG = _mm256_cmpeq_epi8(u, kG);
        const __m256i eT = _mm256_or_si256(_mm256_cmpeq_epi8(u, kT), _mm256_cmpeq_epi8(u, kU));
        const __m256i code = _mm256_or_si256(_mm256_or_si256(_mm256_and_si256(eC, one), _mm256_and_si256(eG, two)),
                                             _mm256_and_si256(eT, three));
        const __m256i ok = _mm256_or_si256(_mm256_or_si256(eA, eC), _mm256_or_si256(eG, eT));
        mask[b] = ~(uint32_t)_mm256_movemask_epi8(ok);
        const __m256i p2 = _mm256_maddubs_epi16(code, m14);      // per 16 bits: c0 | c1 << 2
        const __m256i p4 = _mm256_madd_epi16(p2, m116);          // per 32 bits: c0 .. c3 in the low byte
        const __m256i g = _mm256_permutevar8x32_epi32(_mm256_shuffle_epi8(p4, sh), perm);
        _mm_storel_epi64(reinterpret_cast<__m128i *>(codes + 8 * b), _mm256_castsi256_si128(g));
    }
}

int stage_seqs(Engine &e, uint8_t *dst, const char *const *seqs, const int32_t *len, const int64_t *off, int64_t n,
               int64_t total) {
    constexpr int kSlots = 4;
    for (int k = 0; k < kSlots; ++k) {
        if (!e.stage[k]) {
            HIP_TRY(hipHostMalloc((void **)&e.stage[k], (size_t)kStageSlot, hipHostMallocDefault));
            HIP_TRY(hipEventCreateWithFlags(&e.stage_ev[k], hipEventDisableTiming));
        }
        // a call that failed after staging may have left copies out of a slot in flight
        HIP_TRY(hipEventSynchronize(e.stage_ev[k]));
    }
    if (int rc = e.stage_dev.ensure((size_t)(kSlots * kStageSlot))) return rc;
    // PCABI_STAGE_SCALAR=1: the scalar encoder (the form used without AVX2), for its test
    const char *sc_env = std::getenv("PCABI_STAGE_SCALAR");
    const bool avx2 = __builtin_cpu_supports("avx2") && !(sc_env && sc_env[0] == '1');
    // characters [b0, b1) of the layout into raw (windows' bytes, 'N' between them)
    auto gather = [&](int64_t b0, int64_t b1, uint8_t *raw) {
        int64_t w = std::upper_bound(off, off + n, b0) - off - 1;
        int64_t b = b0;
        while (b < b1) {
            if (w >= n) {
                std::memset(raw + (b - b0), 'N', (size_t)(b1 - b));
                break;
            }
            const int64_t s = off[w], t = s + len[w], nx = w + 1 < n ? off[w + 1] : total;
            if (b < t) {
                const int64_t hi = std::min(t, b1);
                std::memcpy(raw + (b - b0), seqs[w] + (b - s), (size_t)(hi - b));
                b = hi;
            }
            const int64_t hi = std::min(nx, b1);
            if (b < hi) {
                std::memset(raw + (b - b0), 'N', (size_t)(hi - b));
                b = hi;
            }
            ++w;
        }
    };
    const int64_t n_chunk = (total + kStageBytes - 1) / kStageBytes;
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>({16, (int64_t)std::thread::hardware_concurrency(),
                                                                 total / (1 << 20)}));
    std::unique_ptr<std::atomic<int>[]> left(new std::atomic<int>[(size_t)n_chunk]);
    for (int64_t c = 0; c < n_chunk; ++c) left[c].store(nt);
    std::atomic<int64_t> free_upto{std::min<int64_t>(kSlots, n_chunk)};   // chunks below it may be encoded
    std::atomic<bool> stop{false};
    auto work = [&](int t) {
        constexpr int64_t kBlk = 256 << 10;                    // characters gathered at a time (L2-resident)
        std::unique_ptr<uint8_t[]> raw(new uint8_t[kBlk + 32]);
        for (int64_t c = 0; c < n_chunk; ++c) {
            while (free_upto.load(std::memory_order_acquire) <= c && !stop.load(std::memory_order_relaxed))
                std::this_thread::yield();
            if (stop.load(std::memory_order_relaxed)) return;
            const int64_t c0 = c * kStageBytes, c1 = std::min(total, c0 + kStageBytes);
            // the thread's share: 32-base blocks of the chunk (the last one may run past c1: 'N')
            const int64_t nb = (c1 - c0 + 31) / 32;
            const int64_t k0 = nb * t / nt, k1 = nb * (t + 1) / nt;
            uint8_t *slot = e.stage[c % kSlots];
            for (int64_t k = k0; k < k1; k += kBlk / 32) {
                const int64_t ke = std::min(k1, k + kBlk / 32);
                const int64_t b0 = c0 + 32 * k, b1 = std::min(c1, c0 + 32 * ke);
                gather(b0, b1, raw.get());
                if (b1 - b0 < 32 * (ke - k)) std::memset(raw.get() + (b1 - b0), 'N', (size_t)(32 * (ke - k) - (b1 - b0)));
                uint8_t *codes = slot + 8 * k;
                uint32_t *mask = reinterpret_cast<uint32_t *>(slot + kStageCodes) + k;
                if (avx2) pack_avx2(raw.get(), ke - k, codes, mask);
                else
                    for (int64_t q = 0; q < ke - k; ++q) pack32_scalar(raw.get() + 32 * q, codes + 8 * q, mask + q);
            }
            left[c].fetch_sub(1, std::memory_order_release);
        }
    };
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t) th.emplace_back(work, t);
    int rc = 0;
    std::string err;
    int64_t freed = std::min<int64_t>(kSlots, n_chunk);   // chunks [0, freed) have a slot
    for (int64_t c = 0; c < n_chunk && !rc; ++c) {
        while (left[c].load(std::memory_order_acquire) > 0) std::this_thread::yield();
        const int64_t c0 = c * kStageBytes, c1 = std::min(total, c0 + kStageBytes);
        const int64_t nb = (c1 - c0 + 31) / 32;
        const int s = (int)(c % kSlots);
        uint8_t *dslot = (uint8_t *)e.stage_dev.p + s * kStageSlot;
        hipError_t he = hipMemcpyAsync(dslot, e.stage[s], (size_t)(8 * nb), hipMemcpyHostToDevice, e.stream);
        if (he == hipSuccess)
            he = hipMemcpyAsync(dslot + kStageCodes, e.stage[s] + kStageCodes, (size_t)(4 * nb), hipMemcpyHostToDevice,
                                e.stream);
        if (he == hipSuccess) he = hipEventRecord(e.stage_ev[s], e.stream);
        if (he == hipSuccess) {
            const int64_t nq = (c1 - c0 + 15) / 16;
            hipLaunchKernelGGL(k_unpack_codes, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, e.stream,
                               (const uint32_t *)dslot, (const uint32_t *)(dslot + kStageCodes), dst + c0, c1 - c0);
            he = hipGetLastError();
        }
        // hand the workers the slot of the oldest copy still queued once it has landed, keeping
        // kSlots - 1 chunks queued or being encoded behind it (the device slot is reused in stream
        // order: its next copy follows this chunk's unpack)
        const int64_t oldest = c - (kSlots - 2);
        if (he == hipSuccess && oldest >= 0 && freed < n_chunk) {
            he = hipEventSynchronize(e.stage_ev[oldest % kSlots]);
            if (he == hipSuccess) {
                freed = std::min<int64_t>(n_chunk, oldest + kSlots);
                free_upto.store(freed, std::memory_order_release);
            }
        }
        if (he != hipSuccess) {
            rc = PCABI_E_DEVICE;
            err = std::string("staging copy: ") + hipGetErrorString(he);
            break;
        }
    }
    stop.store(true);
    for (auto &t : th) t.join();
    if (rc) return fail(rc, err);
    return 0;
}

}  // namespace

// k_first_hit from each window's start adapter on (start_adp == nullptr: from the first): the
// middle scan's host-driven rounds (pcabi_middle.hip) and pcabi_first_hit_dev
int pcabi_eng::first_hit_from(const int32_t *res, int64_t stride, int64_t n_win, int32_t n_adp, double threshold,
                              const int32_t *start_adp, int32_t *hits, int64_t hit_stride, hipStream_t st) {
    if (n_win <= 0) return 0;
    hipLaunchKernelGGL(k_first_hit, dim3((unsigned)((n_win + 255) / 256)), dim3(256), 0, st, res, stride, n_win,
                       n_adp, threshold, start_adp, hits, hit_stride);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" {

int pcabi_first_hit_dev(const int32_t *res, int64_t stride, int64_t n_win, int32_t n_adp, double threshold,
                        int32_t *hits, int64_t hit_stride, void *stream) {
    return first_hit_from(res, stride, n_win, n_adp, threshold, nullptr, hits, hit_stride, (hipStream_t)stream);
}

// ---- legacy drop-in --------------------------------------------------------------------------

static int fmt_pid(char *buf, size_t cap, int m, int l) {
    if (l == 0) return std::snprintf(buf, cap, "-nan");
    return std::snprintf(buf, cap, "%f", 100.0 * m / l);
}

char *adapterAlignment(char *readSeq, char *adapterSeq, int matchScore, int mismatchScore,
                       int gapOpenScore, int gapExtensionScore) {
    const int64_t n = (int64_t)std::strlen(readSeq);
    const int32_t L = (int32_t)std::strlen(adapterSeq);
    char *s = (char *)std::malloc(256);
    if (!s) return nullptr;
    if (n == 0 || L == 0) {
        std::snprintf(s, 256, "-1,0,-1,0,%d,0.000000,0.000000", (int)0x80000000);
        return s;
    }
    std::vector<uint8_t> codes((size_t)((n + 3) & ~3LL) + 16, 4);
    pcabi_encode_dna5(readSeq, codes.data(), n);
    std::vector<uint8_t> ac((size_t)L);
    pcabi_encode_dna5(adapterSeq, ac.data(), L);
    const int64_t woff = 0;
    const int32_t wlen = (int32_t)n;
    const int32_t aoff = 0;
    int32_t out[PCABI_NFIELDS];
    int device = 0;
    (void)hipGetDevice(&device);
    int rc = pcabi_align_host(device, codes.data(), (int64_t)codes.size(), &woff, &wlen, 1, ac.data(), &aoff,
                              &L, 1, nullptr, nullptr, 0, matchScore, mismatchScore, gapOpenScore,
                              gapExtensionScore, out);
    if (rc != 0) {
        // The reference has no error channel and answers every non-empty input: a "-1" sentinel
        // here would read as "no alignment" and silently change trimming decisions, so stop.
        std::fprintf(stderr, "libpcabi: adapterAlignment failed: %s\n", pcabi_last_error());
        std::free(s);
        std::abort();
    }
    char p1[64], p2[64];
    fmt_pid(p1, sizeof p1, out[PCABI_F_M], out[PCABI_F_L1]);
    fmt_pid(p2, sizeof p2, out[PCABI_F_M], out[PCABI_F_L2]);
    std::snprintf(s, 256, "%d,%d,%d,%d,%d,%s,%s", out[0], out[1], out[2], out[3], out[4], p1, p2);
    return s;
}

void freeCString(char *p) { std::free(p); }

// ---- device-resident interface ----------------------------------------------------------------

int pcabi_dev_set(int device) { HIP_TRY(hipSetDevice(device)); return 0; }
int pcabi_dev_malloc(void **ptr, int64_t bytes) { HIP_TRY(hipMalloc(ptr, (size_t)bytes)); return 0; }
int pcabi_dev_free(void *ptr) { HIP_TRY(hipFree(ptr)); return 0; }
int pcabi_dev_h2d(void *dst, const void *src, int64_t bytes) {
    HIP_TRY(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyHostToDevice)); return 0;
}
int pcabi_dev_d2h(void *dst, const void *src, int64_t bytes) {
    HIP_TRY(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDeviceToHost)); return 0;
}
int pcabi_dev_memset(void *dst, int value, int64_t bytes) { HIP_TRY(hipMemset(dst, value, (size_t)bytes)); return 0; }
int pcabi_dev_sync(void) { HIP_TRY(hipDeviceSynchronize()); return 0; }
int pcabi_dev_copy_async(void *dst, const void *src, int64_t bytes, int kind, void *stream) {
    const hipMemcpyKind k = kind == 0 ? hipMemcpyHostToDevice : (kind == 1 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice);
    if (kind < 0 || kind > 2) return fail(PCABI_E_ARG, "copy kind must be 0 (h2d), 1 (d2h) or 2 (d2d)");
    HIP_TRY(hipMemcpyAsync(dst, src, (size_t)bytes, k, (hipStream_t)stream));
    return 0;
}
int pcabi_stream_create(void **stream) {
    hipStream_t s;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = (void *)s;
    return 0;
}
int pcabi_stream_destroy(void *stream) { HIP_TRY(hipStreamDestroy((hipStream_t)stream)); return 0; }
int pcabi_stream_sync(void *stream) { HIP_TRY(hipStreamSynchronize((hipStream_t)stream)); return 0; }
int pcabi_event_create(void **ev) {
    hipEvent_t e;
    HIP_TRY(hipEventCreate(&e));
    *ev = (void *)e;
    return 0;
}
int pcabi_event_destroy(void *ev) { HIP_TRY(hipEventDestroy((hipEvent_t)ev)); return 0; }
int pcabi_event_record(void *ev, void *stream) { HIP_TRY(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream)); return 0; }
int pcabi_stream_wait_event(void *stream, void *ev) {
    HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)ev, 0));
    return 0;
}
int pcabi_event_elapsed_ms(float *ms, void *start, void *stop) {
    HIP_TRY(hipEventSynchronize((hipEvent_t)stop));
    HIP_TRY(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return 0;
}

}  // extern "C"

namespace {
// Device adapter table. sc == nullptr: laid out for the fast buckets (any scoring with negative
// gap costs; pcabi_align_cross_dev rejects scorings the layout cannot serve); otherwise small
// buckets are merged for that scoring (assign_buckets).
int adapters_create_impl(const uint8_t *adp_codes, const int32_t *adp_off, const int32_t *adp_len,
                         int32_t n_adp, const pcabi::Scoring *sc, pcabi_adapters **out, bool all_striped = false) {
    if (int rc = check_common(adp_len, n_adp)) return rc;
    BucketHost bk[kNumBuckets];
    build_buckets(adp_codes, adp_off, adp_len, n_adp, sc ? *sc : pcabi::Scoring{1, -1, -1, -1}, bk, sc != nullptr,
                  sc != nullptr, all_striped);
    pcabi_adapters *a = new pcabi_adapters();
    a->n_adp = n_adp;
    a->hoff.resize((size_t)n_adp);
    a->hlen.assign(adp_len, adp_len + n_adp);
    for (int k = 0; k < n_adp; ++k) {
        a->hoff[k] = (int32_t)a->hcodes.size();
        for (int i = 0; i < adp_len[k]; ++i) {
            if (adp_codes[adp_off[k] + i] > 3) a->has_n = true;
            a->hcodes.push_back(adp_codes[adp_off[k] + i]);
        }
    }
    for (int b = 0; b < kNumBuckets; ++b) {
        const int nb = (int)bk[b].len.size();
        a->count[b] = nb;
        if (!nb) continue;
        a->lens[b] = bk[b].len;
        a->ids[b] = bk[b].id;
        a->rt[b] = bk[b].rt;
        for (int k = 0; k < nb; ++k) {
            if (bk[b].len[k] != kBuckets[b].rpl) a->padded[b] = true;
            a->max_off[b] = std::max(a->max_off[b], kBuckets[b].rpl - bk[b].len[k]);
        }
        if (hipMalloc((void **)&a->pad[b], bk[b].pad.size()) != hipSuccess ||
            hipMalloc((void **)&a->len[b], sizeof(int32_t) * nb) != hipSuccess ||
            hipMalloc((void **)&a->id[b], sizeof(int32_t) * nb) != hipSuccess) {
            pcabi_adapters_destroy(a);
            return fail(PCABI_E_NOMEM, "hipMalloc failed for adapter table");
        }
        (void)hipMemcpy(a->pad[b], bk[b].pad.data(), bk[b].pad.size(), hipMemcpyHostToDevice);
        (void)hipMemcpy(a->len[b], bk[b].len.data(), sizeof(int32_t) * nb, hipMemcpyHostToDevice);
        (void)hipMemcpy(a->id[b], bk[b].id.data(), sizeof(int32_t) * nb, hipMemcpyHostToDevice);
    }
    *out = a;
    return 0;
}
}  // namespace

// Whether a table's register layout serves a scoring on windows up to max_win long: padded FAST
// buckets need gap costs < 0 (the fast core's pass-through padding rows), merged buckets (more
// than 3 padding rows) and the wide / long buckets the packed core's range conditions, and long
// windows a bounded path span (needs_striped).
bool layout_serves(const pcabi_adapters *adps, const pcabi::Scoring &sc, int64_t max_win) {
    int max_L = 0;
    bool regs = false;
    for (int b = 0; b < kNumBuckets; ++b) {
        if (!adps->count[b] || kBuckets[b].kind == STRIPED) continue;
        regs = true;
        for (int32_t L : adps->lens[b]) max_L = std::max<int>(max_L, L);
        if (kBuckets[b].kind == FAST && adps->padded[b] && !pcabi::fast_ok(kBuckets[b].rpl - 1, kBuckets[b].rpl, sc))
            return false;
        if (kBuckets[b].kind == FAST && adps->max_off[b] > 3 && !bucket_packed_ok(b, adps->lens[b], sc)) return false;
        if (kBuckets[b].kind == WIDE || kBuckets[b].kind == LONG)
            for (int32_t L : adps->lens[b])
                if (kBuckets[b].kind == WIDE ? !pcabi::packed_ok(L, kBuckets[b].rpl, sc)
                                             : !pcabi::long_ok(L, kBuckets[b].rpl, sc))
                    return false;
    }
    return !regs || !needs_striped(sc, max_L, max_win);
}

// The layout of `adps` to run a scoring on windows up to max_win long: the table itself when it
// serves them, else a layout of the same adapters built for them on first use and cached in the
// table -- every adapter on the striped core when the windows need it, else register buckets for
// this scoring. The reference accepts any scoring for any read (arg_parser.py:229-236,
// adapter_align.cpp:11-31), so the device ABI does too.
int adapters_for(const pcabi_adapters *adps, const pcabi::Scoring &sc, int64_t max_win, const pcabi_adapters **use) {
    if (layout_serves(adps, sc, max_win)) {
        *use = adps;
        return 0;
    }
    pcabi_adapters *a = const_cast<pcabi_adapters *>(adps);   // the cache is the only mutable part
    std::lock_guard<std::mutex> g(a->alt_mu);
    std::vector<int32_t> off((size_t)a->n_adp);
    for (int32_t k = 0; k < a->n_adp; ++k) off[k] = a->hoff[k];
    // register buckets laid out (and merged) for this scoring, if they serve these windows
    pcabi_adapters *t = nullptr;
    for (auto &e : a->alt_scored)
        if (e.first.ma == sc.ma && e.first.mi == sc.mi && e.first.go == sc.go && e.first.ge == sc.ge) t = e.second;
    if (!t) {
        if (int rc = adapters_create_impl(a->hcodes.data(), off.data(), a->hlen.data(), a->n_adp, &sc, &t)) return rc;
        a->alt_scored.emplace_back(sc, t);
    }
    if (layout_serves(t, sc, max_win)) {
        *use = t;
        return 0;
    }
    if (!a->alt_striped) {
        t = nullptr;
        if (int rc = adapters_create_impl(a->hcodes.data(), off.data(), a->hlen.data(), a->n_adp, &sc, &t, true))
            return rc;
        a->alt_striped = t;
    }
    *use = a->alt_striped;
    return 0;
}

extern "C" {

int pcabi_adapters_create(const uint8_t *adp_codes, const int32_t *adp_off, const int32_t *adp_len,
                          int32_t n_adp, pcabi_adapters **out) {
    return adapters_create_impl(adp_codes, adp_off, adp_len, n_adp, nullptr, out);
}

int pcabi_adapters_create_scored(const uint8_t *adp_codes, const int32_t *adp_off, const int32_t *adp_len,
                                 int32_t n_adp, int match, int mismatch, int gap_open, int gap_extend,
                                 pcabi_adapters **out) {
    const pcabi::Scoring sc{match, mismatch, gap_open, gap_extend};
    return adapters_create_impl(adp_codes, adp_off, adp_len, n_adp, &sc, out);
}

void pcabi_adapters_destroy(pcabi_adapters *a) {
    if (!a) return;
    for (auto &e : a->alt_scored) pcabi_adapters_destroy(e.second);
    pcabi_adapters_destroy(a->alt_striped);
    for (int b = 0; b < kNumBuckets; ++b) {
        if (a->pad[b]) (void)hipFree(a->pad[b]);
        if (a->len[b]) (void)hipFree(a->len[b]);
        if (a->id[b]) (void)hipFree(a->id[b]);
    }
    delete a;
}

int64_t pcabi_tile_layout(const int32_t *win_len, int64_t n_win, int64_t *tile_off) {
    if (n_win < 0 || !win_len || !tile_off) return fail(PCABI_E_ARG, "bad arguments");
    return tile_layout(win_len, n_win, tile_off, nullptr);
}

int pcabi_tile_windows_dev(const uint8_t *codes, const int64_t *win_off, const int32_t *win_len,
                           int64_t n_win, const int64_t *tile_off, int64_t max_chunks, uint32_t *tiles,
                           void *stream) {
    if (n_win < 0) return fail(PCABI_E_ARG, "bad arguments");
    launch_tiles(codes, win_off, win_len, n_win, tile_off, max_chunks, tiles, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int pcabi_align_cross_dev(const uint32_t *tiles, const int64_t *tile_off, const int32_t *win_len,
                          int64_t n_win, int32_t max_win_len, const pcabi_adapters *adps, int match,
                          int mismatch, int gap_open, int gap_extend, int32_t *out, int64_t out_stride,
                          void *stream) {
    return pcabi_align_cross_dev_marked(tiles, tile_off, win_len, n_win, max_win_len, adps, match, mismatch,
                                        gap_open, gap_extend, out, out_stride, stream, nullptr, nullptr);
}

int pcabi_align_cross_dev_marked(const uint32_t *tiles, const int64_t *tile_off, const int32_t *win_len,
                                 int64_t n_win, int32_t max_win_len, const pcabi_adapters *adps, int match,
                                 int mismatch, int gap_open, int gap_extend, int32_t *out, int64_t out_stride,
                                 void *stream, void *ev_begin, void *ev_end) {
    if (!adps || n_win < 0 || (n_win > 0 && (!tiles || !tile_off))) return fail(PCABI_E_ARG, "bad arguments");
    if (n_win == 0) return 0;
    // a layout of the table that serves this scoring on these windows (the table's own when it can)
    if (int rc = adapters_for(adps, pcabi::Scoring{match, mismatch, gap_open, gap_extend}, max_win_len, &adps))
        return rc;
    KParams p{};
    p.tiles = tiles;
    p.tile_off = tile_off;
    p.win_len = win_len;
    p.n_win = n_win;
    p.out = out;
    p.out_stride = out_stride;
    p.sc = pcabi::Scoring{match, mismatch, gap_open, gap_extend};
    p.max_cols = max_win_len;
    const bool affine = gap_open != gap_extend;
    std::vector<int> order;
    for (int b = 0; b < kNumBuckets; ++b)
        if (adps->count[b]) order.push_back(b);
    // Largest bucket (adapters x rows) on the caller's stream, the others spread over the
    // device's side streams (fork / join with events): a bucket holding one or two adapters is
    // too small a grid to fill 256 CUs on its own, side by side they do.
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
        return (int64_t)adps->count[x] * kBuckets[x].rpl > (int64_t)adps->count[y] * kBuckets[y].rpl;
    });
    ForkJoin fj;
    if (int rc = fj.begin((hipStream_t)stream, order.size())) return rc;
    for (size_t k = 0; k < order.size(); ++k) {
        const int b = order[k];
        p.adp_pad = adps->pad[b];
        p.adp_len = adps->len[b];
        p.adp_id = adps->id[b];
        p.n_adp = adps->count[b];
        p.rt = adps->rt[b];
        const hipStream_t st = fj.at(k);
        // the largest bucket runs on the caller's stream (k == 0): the optional events bracket it
        if (k == 0 && ev_begin) HIP_TRY(hipEventRecord((hipEvent_t)ev_begin, st));
        const int pack = bucket_pack_mode(b, adps->lens[b], p.sc);
        bucket_shift(b, adps->lens[b], p.sc, pack, p);
        if (int rc = dispatch(b, p, affine, st, pack)) {
            (void)fj.end();
            return rc;
        }
        if (k == 0 && ev_end) HIP_TRY(hipEventRecord((hipEvent_t)ev_end, st));
    }
    if (int rc = fj.end()) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}

int pcabi_align_cross_multi_dev(const pcabi_cross_region *regions, int32_t n_regions, int match, int mismatch,
                                int gap_open, int gap_extend, void *stream, void *ev_begin, void *ev_end) {
    if (n_regions < 0 || (n_regions > 0 && !regions)) return fail(PCABI_E_ARG, "bad arguments");
    const pcabi::Scoring sc{match, mismatch, gap_open, gap_extend};
    const bool affine = gap_open != gap_extend;
    // the units: (region, bucket) with its launch class (-1: a launch of its own)
    struct Unit {
        int cls, b, pack;
        KParams p;
        int64_t blocks, cost;
    };
    std::vector<Unit> units;
    for (int32_t r = 0; r < n_regions; ++r) {
        const pcabi_cross_region &g = regions[r];
        if (!g.adps || g.n_win < 0 || (g.n_win > 0 && (!g.tiles || !g.tile_off || !g.win_len || !g.out)))
            return fail(PCABI_E_ARG, "bad region " + std::to_string(r));
        if (g.n_win == 0) continue;
        const pcabi_adapters *adps = nullptr;
        if (int rc = adapters_for(g.adps, sc, g.max_win_len, &adps)) return rc;
        for (int b = 0; b < kNumBuckets; ++b) {
            if (!adps->count[b]) continue;
            Unit u{};
            u.b = b;
            u.pack = bucket_pack_mode(b, adps->lens[b], sc);
            u.cls = kBuckets[b].kind == FAST ? group_class(kBuckets[b].rpl, u.pack, affine) : -1;
            KParams &p = u.p;
            p.tiles = g.tiles;
            p.tile_off = g.tile_off;
            p.win_len = g.win_len;
            p.n_win = g.n_win;
            p.out = g.out;
            p.out_stride = g.out_stride;
            p.sc = sc;
            p.max_cols = g.max_win_len;
            p.adp_pad = adps->pad[b];
            p.adp_len = adps->len[b];
            p.adp_id = adps->id[b];
            p.n_adp = adps->count[b];
            p.rt = adps->rt[b];
            bucket_shift(b, adps->lens[b], sc, u.pack, p);
            u.blocks = (g.n_win + 8 * 256 - 1) / (8 * 256) * 8 * (int64_t)p.n_adp;
            u.cost = (g.n_win + 255) / 256 * (int64_t)p.n_adp * kBuckets[b].rpl;
            units.push_back(u);
        }
    }
    if (units.empty()) return 0;
    // the launches: per class, its units longest rows first in segments of at most kMaxGroupSegs;
    // a class of one unit launches it on its own (k_align, the row split where that applies)
    struct Launch {
        int cls;                 // -1: units[unit] alone
        size_t unit;
        GroupParams gp;
        int64_t blocks, cost;
    };
    std::vector<Launch> launches;
    for (int c = 0; c < kGroupClasses; ++c) {
        std::vector<size_t> mine;
        for (size_t k = 0; k < units.size(); ++k)
            if (units[k].cls == c) mine.push_back(k);
        if (mine.size() == 1) units[mine[0]].cls = -1;
        if (mine.size() <= 1) continue;
        std::stable_sort(mine.begin(), mine.end(),
                         [&](size_t x, size_t y) { return kBuckets[units[x].b].rpl > kBuckets[units[y].b].rpl; });
        for (size_t k0 = 0; k0 < mine.size(); k0 += kMaxGroupSegs) {
            Launch l{};
            l.cls = c;
            l.gp.sc = sc;
            for (size_t k = k0; k < std::min(mine.size(), k0 + kMaxGroupSegs); ++k) {
                const Unit &u = units[mine[k]];
                GroupSeg &s = l.gp.seg[l.gp.n_seg++];
                s.tiles = u.p.tiles;
                s.tile_off = u.p.tile_off;
                s.win_len = u.p.win_len;
                s.n_win = u.p.n_win;
                s.adp_pad = u.p.adp_pad;
                s.adp_len = u.p.adp_len;
                s.adp_id = u.p.adp_id;
                s.n_adp = u.p.n_adp;
                s.out = u.p.out;
                s.out_stride = u.p.out_stride;
                s.rpl = kBuckets[u.b].rpl;
                s.shift_p = u.p.shift_p;
                s.shift_b = u.p.shift_b;
                s.block0 = l.blocks;
                l.blocks += u.blocks;
                l.cost += u.cost;
            }
            launches.push_back(l);
        }
    }
    for (size_t k = 0; k < units.size(); ++k)
        if (units[k].cls < 0) {
            Launch l{};
            l.cls = -1;
            l.unit = k;
            l.cost = units[k].cost;
            launches.push_back(l);
        }
    std::stable_sort(launches.begin(), launches.end(), [](const Launch &x, const Launch &y) { return x.cost > y.cost; });
    ForkJoin fj;
    if (int rc = fj.begin((hipStream_t)stream, launches.size())) return rc;
    for (size_t k = 0; k < launches.size(); ++k) {
        const Launch &l = launches[k];
        const hipStream_t st = fj.at(k);
        if (k == 0 && ev_begin) HIP_TRY(hipEventRecord((hipEvent_t)ev_begin, st));
        if (l.cls >= 0) {
            dispatch_group(l.cls, l.gp, l.blocks, st);
        } else {
            const Unit &u = units[l.unit];
            if (int rc = dispatch(u.b, u.p, affine, st, u.pack)) {
                (void)fj.end();
                return rc;
            }
        }
        if (k == 0 && ev_end) HIP_TRY(hipEventRecord((hipEvent_t)ev_end, st));
    }
    if (int rc = fj.end()) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"




extern "C" {

int pcabi_set_side_streams(int on) {
    const int prev = side_streams_on() ? 1 : 0;
    if (on >= 0) g_side_on.store(on ? 1 : 0);
    return prev;
}

int pcabi_stream_side_streams(void *stream, int on) {
    const hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> g(g_stream_side_mu);
    for (size_t k = 0; k < g_stream_side.size(); ++k)
        if (g_stream_side[k].first == st) {
            const int prev = g_stream_side[k].second;
            if (on < 0) g_stream_side.erase(g_stream_side.begin() + (long)k);
            else g_stream_side[k].second = on ? 1 : 0;
            return prev;
        }
    if (on >= 0) g_stream_side.emplace_back(st, on ? 1 : 0);
    return -1;
}


int pcabi_middle_cuts_host(int device, const int32_t *hits, int64_t hit_stride, int64_t n_hits, int64_t n_reads,
                           const uint8_t *bad_start, const uint8_t *bad_end, int32_t n_adp, int good_side,
                           int bad_side, int64_t *cut_off, int64_t *cuts) {
    if (device < 0 || device >= 16) return fail(PCABI_E_ARG, "bad device index");
    if (n_hits < 0 || n_reads < 0 || n_adp < 0 || hit_stride < n_hits) return fail(PCABI_E_ARG, "bad counts");
    for (int64_t k = 0; k < n_hits; ++k)
        if (hits[k] < 0 || hits[k] >= n_reads || hits[hit_stride + k] < 0 || hits[hit_stride + k] >= n_adp)
            return fail(PCABI_E_ARG, "hit read / adapter index out of range");
    Engine &e = g_engines[device];
    std::lock_guard<std::mutex> lock(e.mu);
    if (int rc = engine_init(e, device)) return rc;
    HIP_TRY(hipSetDevice(device));
    const size_t hb = sizeof(int32_t) * 4 * (size_t)std::max<int64_t>(n_hits, 1);
    const size_t fb = 2 * (size_t)std::max<int32_t>(n_adp, 1);
    const size_t ob = sizeof(int64_t) * ((size_t)n_reads + 1), cb = sizeof(int64_t) * 2 * (size_t)std::max<int64_t>(n_hits, 1);
    if (int rc = e.bc.ensure(hb + fb + ob + cb + 64)) return rc;
    char *p = (char *)e.bc.p;
    int32_t *d_hits = (int32_t *)p;
    uint8_t *d_flags = (uint8_t *)(p + hb);
    int64_t *d_off = (int64_t *)(((uintptr_t)(p + hb + fb) + 7) & ~(uintptr_t)7);
    int64_t *d_cuts = d_off + n_reads + 1;
    // the four used rows (read, adapter, read_start, read_end), packed with stride n_hits
    for (int f = 0; f < 4 && n_hits; ++f)
        HIP_TRY(hipMemcpyAsync(d_hits + f * n_hits, hits + f * hit_stride, sizeof(int32_t) * (size_t)n_hits,
                               hipMemcpyHostToDevice, e.stream));
    if (n_adp) {
        HIP_TRY(hipMemcpyAsync(d_flags, bad_start, (size_t)n_adp, hipMemcpyHostToDevice, e.stream));
        HIP_TRY(hipMemcpyAsync(d_flags + n_adp, bad_end, (size_t)n_adp, hipMemcpyHostToDevice, e.stream));
    }
    if (int rc = pcabi_middle_cuts_dev(d_hits, n_hits, n_hits, n_reads, d_flags, d_flags + n_adp, good_side, bad_side,
                                       d_off, d_cuts, e.stream))
        return rc;
    HIP_TRY(hipMemcpyAsync(cut_off, d_off, sizeof(int64_t) * ((size_t)n_reads + 1), hipMemcpyDeviceToHost, e.stream));
    if (n_hits)
        HIP_TRY(hipMemcpyAsync(cuts, d_cuts, sizeof(int64_t) * 2 * (size_t)n_hits, hipMemcpyDeviceToHost, e.stream));
    HIP_TRY(hipStreamSynchronize(e.stream));
    return 0;
}

int pcabi_end_trim_dev(const int32_t *start_res, int64_t start_stride, int32_t n_sa,
                       const int32_t *end_res, int64_t end_stride, int32_t n_ea, int64_t n_read,
                       int end_size, int extra_trim, double end_threshold, int min_trim_size,
                       int32_t *start_trim, int32_t *end_trim, uint8_t *start_hit, uint8_t *end_hit,
                       void *stream) {
    if (n_read <= 0) return 0;
    const unsigned blocks = (unsigned)((n_read + 63) / 64);
    hipLaunchKernelGGL(k_end_trim, dim3(blocks), dim3(256), 0, (hipStream_t)stream, start_res, start_stride,
                       n_sa, end_res, end_stride, n_ea, n_read, end_size, extra_trim, end_threshold,
                       min_trim_size, start_trim, end_trim, start_hit, end_hit);
    HIP_TRY(hipGetLastError());
    return 0;
}

int pcabi_trim_views_dev(const int64_t *read_off, const int32_t *read_len, const int32_t *start_trim,
                         const int32_t *end_trim, int64_t n_read, int64_t *view_off, int32_t *view_len, void *stream) {
    if (n_read < 0) return fail(PCABI_E_ARG, "bad read count");
    if (n_read == 0) return 0;
    hipLaunchKernelGGL(k_trim_views, dim3((unsigned)std::min<int64_t>((n_read + 255) / 256, 4096)), dim3(256), 0,
                       (hipStream_t)stream, read_off, read_len, start_trim, end_trim, n_read, view_off, view_len);
    HIP_TRY(hipGetLastError());
    return 0;
}

int pcabi_best_full_identity_dev(const int32_t *res, int64_t stride, int64_t n_win, int32_t n_adp,
                                 double *best, void *stream) {
    if (n_adp <= 0 || n_win <= 0) return 0;
    hipLaunchKernelGGL(k_best_full_id, dim3((unsigned)n_adp), dim3(256), 0, (hipStream_t)stream, res, stride,
                       n_win, best);
    HIP_TRY(hipGetLastError());
    return 0;
}

int pcabi_barcode_call_dev(const int32_t *start_res, int64_t start_stride, const int32_t *start_slot_adp,
                           const int32_t *start_slot_name, int32_t n_start_slots, const int32_t *end_res,
                           int64_t end_stride, const int32_t *end_slot_adp, const int32_t *end_slot_name,
                           int32_t n_end_slots, int64_t n_read, double barcode_threshold, double barcode_diff,
                           int require_two, int32_t *call, double *scores, void *stream) {
    if (n_read < 0 || n_start_slots < 0 || n_end_slots < 0) return fail(PCABI_E_ARG, "negative count");
    if (n_read == 0) return 0;
    const BcSide st{start_res, start_stride, start_slot_adp, start_slot_name, n_start_slots};
    const BcSide en{end_res, end_stride, end_slot_adp, end_slot_name, n_end_slots};
    hipLaunchKernelGGL(k_barcode_call, dim3((unsigned)((n_read + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       st, en, n_read, barcode_threshold, barcode_diff, require_two, call, scores);
    HIP_TRY(hipGetLastError());
    return 0;
}

int pcabi_compat_host(int device, const uint8_t *codes, int64_t codes_len, const int64_t *seq_off,
                      const int32_t *seq_len, int64_t n_seq, const int32_t *pair_i, const int32_t *pair_j,
                      int64_t n_pairs, int32_t *flags) {
    if (n_seq < 0 || n_pairs < 0) return fail(PCABI_E_ARG, "negative count");
    if (n_seq > INT32_MAX) return fail(PCABI_E_ARG, "too many sequences");
    // row 0 = the longer sequence (make_stringSet, compatibility.cpp:17-28: ties keep seq1 first)
    std::vector<int32_t> tw, ta;
    std::vector<int64_t> at;           // result slot of each task
    tw.reserve((size_t)n_pairs);
    ta.reserve((size_t)n_pairs);
    for (int64_t t = 0; t < n_pairs; ++t) {
        const int32_t i = pair_i[t], j = pair_j[t];
        if (i < 0 || i >= n_seq || j < 0 || j >= n_seq) return fail(PCABI_E_ARG, "pair index out of range");
        const bool swap = seq_len[i] < seq_len[j];
        const int32_t lo = swap ? j : i, sh = swap ? i : j;
        flags[t] = 0;                  // empty sequences: no alignment (the reference is undefined)
        if (seq_len[lo] == 0 || seq_len[sh] == 0) continue;
        if (seq_len[sh] > pcabi::MAX_STRIPED_LEN)
            return fail(PCABI_E_ARG, "check_compatibility: the shorter sequence exceeds " +
                                         std::to_string(pcabi::MAX_STRIPED_LEN) + " bases");
        tw.push_back(lo);
        ta.push_back(sh);
        at.push_back(t);
    }
    if (tw.empty()) return 0;
    std::vector<uint8_t> acodes;
    std::vector<int32_t> aoff((size_t)n_seq), alen((size_t)n_seq);
    for (int64_t k = 0; k < n_seq; ++k) {
        aoff[k] = (int32_t)acodes.size();
        alen[k] = std::max<int32_t>(1, std::min<int32_t>(seq_len[k], pcabi::MAX_STRIPED_LEN));
        for (int32_t q = 0; q < alen[k]; ++q) acodes.push_back(seq_len[k] > 0 ? codes[seq_off[k] + q] : 0);
    }
    std::vector<int32_t> got(tw.size());
    // compatibility.h:5-8: Score<int, Simple>(match 2, mismatch -1, gap -1) -> linear gaps
    if (int rc = align_host_impl(device, codes, codes_len, seq_off, seq_len, n_seq, acodes.data(), aoff.data(),
                                 alen.data(), (int32_t)n_seq, tw.data(), ta.data(), (int64_t)tw.size(), 2, -1, -1, -1,
                                 nullptr, got.data(), true))
        return rc;
    for (size_t k = 0; k < tw.size(); ++k) flags[at[k]] = got[k];
    return 0;
}

int pcabi_compat_all_vs_all_host(int device, const uint8_t *codes, int64_t codes_len, const int64_t *seq_off,
                                 const int32_t *seq_len, int64_t n_seq, int32_t *mat) {
    if (n_seq < 0) return fail(PCABI_E_ARG, "negative count");
    if (n_seq > 46340) return fail(PCABI_E_ARG, "too many sequences for one matrix");
    const int64_t n = n_seq;
    for (int64_t k = 0; k < n; ++k) mat[k * n + k] = -1;   // every other entry is written below
    if (n < 2) return 0;
    bool cross_ok = true;
    for (int64_t k = 0; k < n; ++k) cross_ok = cross_ok && seq_len[k] >= 1 && seq_len[k] <= pcabi::MAX_STRIPED_LEN;
    if (!cross_ok) {
        // some sequence cannot be a DP row set: explicit pairs (the longer is never a row set)
        std::vector<int32_t> pi, pj;
        for (int64_t i = 0; i < n; ++i)
            for (int64_t j = i + 1; j < n; ++j) { pi.push_back((int32_t)i); pj.push_back((int32_t)j); }
        std::vector<int32_t> f(pi.size());
        if (int rc = pcabi_compat_host(device, codes, codes_len, seq_off, seq_len, n, pi.data(), pj.data(),
                                       (int64_t)pi.size(), f.data()))
            return rc;
        for (size_t t = 0; t < pi.size(); ++t) mat[(int64_t)pi[t] * n + pj[t]] = mat[(int64_t)pj[t] * n + pi[t]] = f[t];
        return 0;
    }
    // every sequence against every sequence in the tiled cross mode (both orientations, no host
    // task lists), then per pair the orientation the reference uses: row 0 = the longer, ties ->
    // the first argument (consensus.py:90-97 passes seq_i, seq_j with i < j)
    std::vector<uint8_t> acodes;
    std::vector<int32_t> aoff((size_t)n);
    for (int64_t k = 0; k < n; ++k) {
        aoff[k] = (int32_t)acodes.size();
        acodes.insert(acodes.end(), codes + seq_off[k], codes + seq_off[k] + seq_len[k]);
    }
    // the cross product f[a * n + w] stays on the device; k_orient writes the matrix
    return align_host_impl(device, codes, codes_len, seq_off, seq_len, n, acodes.data(), aoff.data(), seq_len,
                           (int32_t)n, nullptr, nullptr, 0, 2, -1, -1, -1, nullptr, mat, true, true);
}

int check_compatibility(char *raw_seq1, char *raw_seq2) {
    // SeqAn String<Dna> (compatibility.h:23): A C G T/U, anything else -> A
    const size_t n1 = raw_seq1 ? std::strlen(raw_seq1) : 0, n2 = raw_seq2 ? std::strlen(raw_seq2) : 0;
    std::vector<uint8_t> codes(((n1 + 3) & ~(size_t)3) + n2 + 16, 0);
    auto enc = [](char c) -> uint8_t {
        switch (c) {
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': case 'U': case 'u': return 3;
        default: return 0;
        }
    };
    for (size_t k = 0; k < n1; ++k) codes[k] = enc(raw_seq1[k]);
    const int64_t o2 = (int64_t)((n1 + 3) & ~(size_t)3);
    for (size_t k = 0; k < n2; ++k) codes[o2 + k] = enc(raw_seq2[k]);
    const int64_t off[2] = {0, o2};
    const int32_t len[2] = {(int32_t)n1, (int32_t)n2};
    const int32_t pi = 0, pj = 1;
    int32_t flag = 0;
    int device = 0;
    (void)hipGetDevice(&device);
    if (pcabi_compat_host(device, codes.data(), (int64_t)codes.size(), off, len, 2, &pi, &pj, 1, &flag) != 0) {
        // the reference has no error channel and never fails here: stop rather than answer wrongly
        std::fprintf(stderr, "libpcabi: check_compatibility failed: %s\n", pcabi_last_error());
        std::abort();
    }
    return flag;
}

int pcabi_barcode_call_host(int device, const int32_t *start_res, int32_t n_sa, const int32_t *start_slot_adp,
                            const int32_t *start_slot_name, int32_t n_start_slots, const int32_t *end_res,
                            int32_t n_ea, const int32_t *end_slot_adp, const int32_t *end_slot_name,
                            int32_t n_end_slots, int64_t n_read, double barcode_threshold, double barcode_diff,
                            int require_two, int32_t *call, double *scores) {
    if (device < 0 || device >= 16) return fail(PCABI_E_ARG, "bad device index");
    if (n_read < 0 || n_sa < 0 || n_ea < 0 || n_start_slots < 0 || n_end_slots < 0)
        return fail(PCABI_E_ARG, "negative count");
    for (int k = 0; k < n_start_slots; ++k)
        if (start_slot_adp[k] < 0 || start_slot_adp[k] >= n_sa) return fail(PCABI_E_ARG, "start slot adapter out of range");
    for (int k = 0; k < n_end_slots; ++k)
        if (end_slot_adp[k] < 0 || end_slot_adp[k] >= n_ea) return fail(PCABI_E_ARG, "end slot adapter out of range");
    if (n_read == 0) return 0;
    Engine &e = g_engines[device];
    std::lock_guard<std::mutex> lock(e.mu);
    if (int rc = engine_init(e, device)) return rc;
    HIP_TRY(hipSetDevice(device));
    const size_t sres = sizeof(int32_t) * PCABI_NFIELDS * (size_t)n_sa * (size_t)n_read;
    const size_t eres = sizeof(int32_t) * PCABI_NFIELDS * (size_t)n_ea * (size_t)n_read;
    const size_t slots = sizeof(int32_t) * 2 * (size_t)(n_start_slots + n_end_slots);
    if (int rc = e.bc.ensure(sres + eres + slots + sizeof(int32_t) * (size_t)n_read + 32 * (size_t)n_read + 64))
        return rc;
    char *p = (char *)e.bc.p;
    int32_t *d_sres = (int32_t *)p; p += sres;
    int32_t *d_eres = (int32_t *)p; p += eres;
    int32_t *d_slots = (int32_t *)p; p += slots;
    int32_t *d_call = (int32_t *)p; p += sizeof(int32_t) * (size_t)n_read;
    p = (char *)(((uintptr_t)p + 7) & ~(uintptr_t)7);
    double *d_scores = (double *)p;
    std::vector<int32_t> h_slots;
    h_slots.insert(h_slots.end(), start_slot_adp, start_slot_adp + n_start_slots);
    h_slots.insert(h_slots.end(), start_slot_name, start_slot_name + n_start_slots);
    h_slots.insert(h_slots.end(), end_slot_adp, end_slot_adp + n_end_slots);
    h_slots.insert(h_slots.end(), end_slot_name, end_slot_name + n_end_slots);
    if (sres) HIP_TRY(hipMemcpyAsync(d_sres, start_res, sres, hipMemcpyHostToDevice, e.stream));
    if (eres) HIP_TRY(hipMemcpyAsync(d_eres, end_res, eres, hipMemcpyHostToDevice, e.stream));
    if (slots) HIP_TRY(hipMemcpyAsync(d_slots, h_slots.data(), slots, hipMemcpyHostToDevice, e.stream));
    const int32_t *ss = d_slots, *en_ = d_slots + 2 * n_start_slots;
    if (int rc = pcabi_barcode_call_dev(d_sres, (int64_t)n_sa * n_read, ss, ss + n_start_slots, n_start_slots, d_eres,
                                        (int64_t)n_ea * n_read, en_, en_ + n_end_slots, n_end_slots, n_read,
                                        barcode_threshold, barcode_diff, require_two, d_call,
                                        scores ? d_scores : nullptr, e.stream))
        return rc;
    HIP_TRY(hipMemcpyAsync(call, d_call, sizeof(int32_t) * (size_t)n_read, hipMemcpyDeviceToHost, e.stream));
    if (scores)
        HIP_TRY(hipMemcpyAsync(scores, d_scores, 32 * (size_t)n_read, hipMemcpyDeviceToHost, e.stream));
    HIP_TRY(hipStreamSynchronize(e.stream));
    return 0;
}

}  // extern "C"

// ---- end-trim decisions of the reference-API driver (find_adapters_at_read_ends) -----------------
extern "C" int pcabi_flag_list_dev(const uint8_t *flag, int32_t n_adp, int64_t n_read, const int32_t *res,
                                   int64_t stride, int32_t *out, int64_t cap, unsigned long long *n_out,
                                   void *stream);

namespace {

// out[j * n_read + r] = the full-adapter identity (pid6(m, l2), 0.0 for no alignment) of adapter
// sel[j] on read r: the barcode dicts of find_start_trim / find_end_trim (nanopore_read.py:193-195).
__global__ __launch_bounds__(256) void k_full_ids(const int32_t *res, int64_t stride, int64_t n_read,
                                                  const int32_t *sel, int32_t n_sel, double *out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)n_sel * n_read) return;
    const int32_t j = (int32_t)(i / n_read);
    const int64_t q = (int64_t)sel[j] * n_read + (i - (int64_t)j * n_read);
    out[i] = res[q] == -1 ? 0.0 : pcabi::pid6(res[5 * stride + q], res[7 * stride + q]);
}

// The compact form of a side's alignment list for the D2H (pcabi_end_decisions_host): per
// alignment six int16 (adapter, rs, re, m, l1, l2), per read its alignment count (uint16, two per
// dword); the read row is rebuilt on the host from the counts (the list is read-major). 12 B per
// alignment + 2 B per read instead of 28 B per alignment.
__global__ __launch_bounds__(256) void k_list_pack(const int32_t *list, int64_t dcap, int64_t cnt, int16_t *out,
                                                   uint32_t *counts) {
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < cnt; k += (int64_t)gridDim.x * 256) {
        const int32_t r = list[k];
#pragma unroll
        for (int f = 0; f < 6; ++f) out[f * cnt + k] = (int16_t)list[(f + 1) * dcap + k];
        atomicAdd(&counts[r >> 1], 1u << (16 * (r & 1)));
    }
}

int side_table(Engine::DTab &c, const uint8_t *codes, const int32_t *off, const int32_t *len, int32_t n,
               const pcabi::Scoring &sc, pcabi_adapters **out) {
    std::vector<uint8_t> key;
    for (int32_t a = 0; a < n; ++a) key.insert(key.end(), codes + off[a], codes + off[a] + len[a]);
    if (c.t && c.sc.ma == sc.ma && c.sc.mi == sc.mi && c.sc.go == sc.go && c.sc.ge == sc.ge && c.codes == key &&
        c.lens == std::vector<int32_t>(len, len + n)) {
        *out = c.t;
        return 0;
    }
    if (c.t) pcabi_adapters_destroy(c.t);   // the previous call synchronised its stream
    c.t = nullptr;
    if (int rc = adapters_create_impl(codes, off, len, n, &sc, &c.t)) return rc;
    c.codes.swap(key);
    c.lens.assign(len, len + n);
    c.sc = sc;
    *out = c.t;
    return 0;
}

}  // namespace

namespace {
// pcabi_end_decisions_host / _seqs: the windows' codes come from `codes` (a host Dna5 buffer) or,
// when `win` is set, from the 2 n_read window strings (start windows, then end windows), encoded
// straight into pinned staging buffers while earlier chunks copy (stage_seqs)
int end_decisions_impl(
    int device, const uint8_t *codes, const char *const *win, const int32_t *win_len, int64_t codes_len,
    const int64_t *s_off, const int32_t *s_len, const int64_t *e_off, const int32_t *e_len, int64_t n_read,
    const uint8_t *sa_codes, const int32_t *sa_off, const int32_t *sa_len, int32_t n_sa, const uint8_t *ea_codes,
    const int32_t *ea_off, const int32_t *ea_len, int32_t n_ea, int match, int mismatch, int gap_open, int gap_extend,
    int end_size, int extra_trim, double end_threshold, int min_trim_size, int32_t *start_trim, int32_t *end_trim,
    int32_t *start_hits, int32_t *end_hits, int64_t cap, int64_t *n_hits, const int32_t *bc_s, int32_t n_bc_s,
    const int32_t *bc_e, int32_t n_bc_e, double *bc_full) {
    if (device < 0 || device >= 16) return fail(PCABI_E_ARG, "bad device index");
    if (n_read < 0 || n_sa < 0 || n_ea < 0 || cap < 0 || n_bc_s < 0 || n_bc_e < 0) return fail(PCABI_E_ARG, "negative count");
    if (int rc = check_common(sa_len, n_sa)) return rc;
    if (int rc = check_common(ea_len, n_ea)) return rc;
    for (int side = 0; side < 2; ++side) {
        const int64_t *off = side ? e_off : s_off;
        const int32_t *len = side ? e_len : s_len;
        for (int64_t w = 0; w < n_read; ++w) {
            if (len[w] < 0 || len[w] > pcabi::MAX_WINDOW_LEN) return fail(PCABI_E_ARG, "window length out of range");
            if (len[w] > 0 && (off[w] < 0 || off[w] + len[w] + 16 > codes_len))
                return fail(PCABI_E_ARG, "window outside the buffer or buffer not padded by 16 bytes");
        }
    }
    for (int32_t j = 0; j < n_bc_s; ++j)
        if (bc_s[j] < 0 || bc_s[j] >= n_sa) return fail(PCABI_E_ARG, "start barcode adapter out of range");
    for (int32_t j = 0; j < n_bc_e; ++j)
        if (bc_e[j] < 0 || bc_e[j] >= n_ea) return fail(PCABI_E_ARG, "end barcode adapter out of range");
    n_hits[0] = n_hits[1] = 0;
    if (n_read == 0) return 0;
    // PCABI_END_PROF=1: the call's host / device phases on stderr
    static const bool prof = [] { const char *v = std::getenv("PCABI_END_PROF"); return v && v[0] == '1'; }();
    const auto t0 = std::chrono::steady_clock::now();
    auto mark = [&](const char *what) {
        if (prof)
            std::fprintf(stderr, "pcabi_end_decisions: %-10s %.3f ms\n", what,
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    };
    Engine &e = g_engines[device];
    std::lock_guard<std::mutex> lock(e.mu);
    if (int rc = engine_init(e, device)) return rc;
    HIP_TRY(hipSetDevice(device));
    const pcabi::Scoring sc{match, mismatch, gap_open, gap_extend};
    const hipStream_t st = e.stream;
    const size_t n = (size_t)n_read;
    const int32_t n_adp[2] = {n_sa, n_ea};
    // buffers: 0 codes; per side (base 1 + 6 side): offsets, lengths, tile offsets, tiles, results, flags;
    // 13 trims (2 x n); 14 lists (2 sides x 7 x n_read x n_adp bound); 15 counts + barcode identities
    if (int rc = e.dec[0].ensure((size_t)codes_len)) return rc;
    if (win) {
        std::vector<int64_t> off(2 * n);
        std::copy(s_off, s_off + n, off.begin());
        std::copy(e_off, e_off + n, off.begin() + (int64_t)n);
        if (int rc = stage_seqs(e, (uint8_t *)e.dec[0].p, win, win_len, off.data(), 2 * n_read, codes_len)) return rc;
    } else {
        HIP_TRY(hipMemcpyAsync(e.dec[0].p, codes, (size_t)codes_len, hipMemcpyHostToDevice, st));
    }
    mark("staged");
    if (int rc = e.dec[13].ensure(8 * n)) return rc;
    int32_t *d_st = (int32_t *)e.dec[13].p, *d_et = d_st + n;
    std::vector<int64_t> toff[2];
    const int32_t *res[2] = {nullptr, nullptr};
    uint8_t *flag[2] = {nullptr, nullptr};
    pcabi_cross_region reg[2];
    int32_t n_reg = 0;
    for (int side = 0; side < 2; ++side) {
        const int64_t *off = side ? e_off : s_off;
        const int32_t *len = side ? e_len : s_len;
        DeviceBuf *b = e.dec + 1 + 6 * side;
        if (int rc = b[0].ensure(8 * n)) return rc;
        if (int rc = b[1].ensure(4 * n)) return rc;
        toff[side].assign((n + 255) / 256 + 1, 0);
        int64_t max_nq = 0;
        const int64_t nd = tile_layout(len, n_read, toff[side].data(), &max_nq);
        if (int rc = b[2].ensure(8 * toff[side].size())) return rc;
        if (int rc = b[3].ensure(4 * (size_t)std::max<int64_t>(nd, 1))) return rc;
        if (int rc = b[4].ensure(4 * PCABI_NFIELDS * n * (size_t)std::max(n_adp[side], 1))) return rc;
        if (int rc = b[5].ensure(n * (size_t)std::max(n_adp[side], 1))) return rc;
        HIP_TRY(hipMemcpyAsync(b[0].p, off, 8 * n, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(b[1].p, len, 4 * n, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(b[2].p, toff[side].data(), 8 * toff[side].size(), hipMemcpyHostToDevice, st));
        res[side] = (const int32_t *)b[4].p;
        flag[side] = (uint8_t *)b[5].p;
        if (!n_adp[side]) continue;
        int32_t max_len = 0;
        for (size_t w = 0; w < n; ++w) max_len = std::max(max_len, len[w]);
        pcabi_adapters *tab = nullptr;
        if (int rc = side_table(e.dtab[side], side ? ea_codes : sa_codes, side ? ea_off : sa_off, side ? ea_len : sa_len,
                                n_adp[side], sc, &tab))
            return rc;
        launch_tiles((const uint8_t *)e.dec[0].p, (const int64_t *)b[0].p, (const int32_t *)b[1].p, n_read,
                     (const int64_t *)b[2].p, max_nq, (uint32_t *)b[3].p, st);
        reg[n_reg++] = pcabi_cross_region{(const uint32_t *)b[3].p, (const int64_t *)b[2].p, (const int32_t *)b[1].p,
                                          n_read, max_len, tab, (int32_t *)b[4].p, (int64_t)n_adp[side] * n_read};
    }
    // both read ends in one call: the register buckets of both sides in grouped launches (r06)
    if (int rc = pcabi_align_cross_multi_dev(reg, n_reg, match, mismatch, gap_open, gap_extend, st, nullptr, nullptr))
        return rc;
    if (int rc = pcabi_end_trim_dev(res[0], (int64_t)n_sa * n_read, n_sa, res[1], (int64_t)n_ea * n_read, n_ea, n_read,
                                    end_size, extra_trim, end_threshold, min_trim_size, d_st, d_et, flag[0], flag[1], st))
        return rc;
    // the alignment lists (device capacity: every pair of the side -- they never overflow there)
    const size_t dcap[2] = {n * (size_t)n_sa, n * (size_t)n_ea};
    if (int rc = e.dec[14].ensure(4 * 7 * (dcap[0] + dcap[1]) + 16)) return rc;
    int32_t *d_list[2] = {(int32_t *)e.dec[14].p, (int32_t *)e.dec[14].p + 7 * dcap[0]};
    const size_t nbc = (size_t)n_bc_s + (size_t)n_bc_e;
    if (int rc = e.dec[15].ensure(64 + ((4 * nbc + 7) & ~(size_t)7) + 8 * nbc * n)) return rc;   // d_full below
    unsigned long long *d_cnt = (unsigned long long *)e.dec[15].p;
    int32_t *d_sel = (int32_t *)((char *)e.dec[15].p + 16);
    double *d_full = (double *)((char *)e.dec[15].p + 64 + ((4 * nbc + 7) & ~(size_t)7));
    for (int side = 0; side < 2; ++side) {
        if (!n_adp[side]) {
            HIP_TRY(hipMemsetAsync(d_cnt + side, 0, 8, st));
            continue;
        }
        if (int rc = pcabi_flag_list_dev(flag[side], n_adp[side], n_read, res[side], (int64_t)n_adp[side] * n_read,
                                         d_list[side], (int64_t)dcap[side], d_cnt + side, st))
            return rc;
    }
    if (nbc && bc_full) {
        std::vector<int32_t> sel(bc_s, bc_s + n_bc_s);
        sel.insert(sel.end(), bc_e, bc_e + n_bc_e);
        HIP_TRY(hipMemcpyAsync(d_sel, sel.data(), 4 * nbc, hipMemcpyHostToDevice, st));
        for (int side = 0; side < 2; ++side) {
            const int32_t ns = side ? n_bc_e : n_bc_s;
            if (!ns) continue;
            const int64_t tot = (int64_t)ns * n_read;
            hipLaunchKernelGGL(k_full_ids, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, res[side],
                               (int64_t)n_adp[side] * n_read, n_read, d_sel + (side ? n_bc_s : 0), ns,
                               d_full + (side ? (size_t)n_bc_s * n : 0));
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(bc_full, d_full, 8 * nbc * n, hipMemcpyDeviceToHost, st));
    }
    unsigned long long cnt[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(start_trim, d_st, 4 * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(end_trim, d_et, 4 * n, hipMemcpyDeviceToHost, st));
    mark("queued");
    HIP_TRY(hipMemcpyAsync(cnt, d_cnt, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    mark("device");
    n_hits[0] = (int64_t)cnt[0];
    n_hits[1] = (int64_t)cnt[1];
    // the lists: compact (int16 fields, per-read counts) when every field fits 16 bits -- the
    // alignment lengths l1 / l2 reach the window plus the adapter
    int32_t max_win = 0, max_adp = 0;
    for (size_t w = 0; w < n; ++w) max_win = std::max(max_win, std::max(s_len[w], e_len[w]));
    for (int32_t a = 0; a < n_sa; ++a) max_adp = std::max(max_adp, sa_len[a]);
    for (int32_t a = 0; a < n_ea; ++a) max_adp = std::max(max_adp, ea_len[a]);
    const bool compact = (int64_t)max_win + max_adp < 32768 && n_sa < 32768 && n_ea < 32768;
    const size_t half = (n + 1) / 2;                // count dwords per side
    if (compact) {
        size_t words = 0;
        for (int side = 0; side < 2; ++side)
            if ((int64_t)cnt[side] <= cap) words += 3 * (size_t)cnt[side] + half;   // 6 int16 = 3 dwords
        if (int rc = e.dec[16].ensure(4 * words + 64)) return rc;
        std::vector<uint32_t> h((size_t)words);
        size_t at = 0, at_side[2] = {0, 0};
        for (int side = 0; side < 2; ++side) {
            const int64_t k = (int64_t)cnt[side];
            if (k > cap) continue;
            at_side[side] = at;
            uint32_t *dc = (uint32_t *)e.dec[16].p + at + 3 * (size_t)k;
            HIP_TRY(hipMemsetAsync(dc, 0, 4 * half, st));
            if (k)
                hipLaunchKernelGGL(k_list_pack, dim3((unsigned)std::min<int64_t>((k + 255) / 256, 4096)), dim3(256), 0, st,
                                   d_list[side], (int64_t)dcap[side], k, (int16_t *)((uint32_t *)e.dec[16].p + at), dc);
            at += 3 * (size_t)k + half;
        }
        HIP_TRY(hipGetLastError());
        if (words) HIP_TRY(hipMemcpyAsync(h.data(), e.dec[16].p, 4 * words, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        mark("lists d2h");
        for (int side = 0; side < 2; ++side) {
            int32_t *dst = side ? end_hits : start_hits;
            const int64_t k = (int64_t)cnt[side];
            if (k > cap || !k) continue;            // too many: the caller grows cap and calls again
            const int16_t *f16 = (const int16_t *)(h.data() + at_side[side]);
            const uint16_t *c16 = (const uint16_t *)(h.data() + at_side[side] + 3 * (size_t)k);
            int64_t j = 0;
            for (size_t r = 0; r < n && j < k; ++r)
                for (uint16_t c = c16[r]; c > 0; --c) dst[j++] = (int32_t)r;
            for (int f = 0; f < 6; ++f)
                for (int64_t q = 0; q < k; ++q) dst[(f + 1) * cap + q] = f16[f * k + q];
        }
        mark("unpacked");
        return 0;
    }
    for (int side = 0; side < 2; ++side) {
        int32_t *dst = side ? end_hits : start_hits;
        const int64_t k = (int64_t)cnt[side];
        if (k > cap || !k) continue;                // too many: the caller grows cap and calls again
        for (int f = 0; f < 7; ++f)                 // rows of the device list (stride dcap) -> stride cap
            HIP_TRY(hipMemcpyAsync(dst + f * cap, d_list[side] + f * dcap[side], 4 * (size_t)k, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}
}  // namespace

extern "C" int pcabi_end_decisions_host(
    int device, const uint8_t *codes, int64_t codes_len, const int64_t *s_off, const int32_t *s_len,
    const int64_t *e_off, const int32_t *e_len, int64_t n_read, const uint8_t *sa_codes, const int32_t *sa_off,
    const int32_t *sa_len, int32_t n_sa, const uint8_t *ea_codes, const int32_t *ea_off, const int32_t *ea_len,
    int32_t n_ea, int match, int mismatch, int gap_open, int gap_extend, int end_size, int extra_trim,
    double end_threshold, int min_trim_size, int32_t *start_trim, int32_t *end_trim, int32_t *start_hits,
    int32_t *end_hits, int64_t cap, int64_t *n_hits, const int32_t *bc_s, int32_t n_bc_s, const int32_t *bc_e,
    int32_t n_bc_e, double *bc_full) {
    return end_decisions_impl(device, codes, nullptr, nullptr, codes_len, s_off, s_len, e_off, e_len, n_read, sa_codes,
                              sa_off, sa_len, n_sa, ea_codes, ea_off, ea_len, n_ea, match, mismatch, gap_open,
                              gap_extend, end_size, extra_trim, end_threshold, min_trim_size, start_trim, end_trim,
                              start_hits, end_hits, cap, n_hits, bc_s, n_bc_s, bc_e, n_bc_e, bc_full);
}

// pcabi_end_decisions_host over window strings: win / win_len hold the n_read start windows, then
// the n_read end windows (addresses of their first characters -- ASCII, one byte per base -- and
// lengths); the library lays them out as the host entry's buffer and encodes them itself.
extern "C" int pcabi_end_decisions_seqs(
    int device, const char *const *win, const int32_t *win_len, int64_t n_read, const uint8_t *sa_codes,
    const int32_t *sa_off, const int32_t *sa_len, int32_t n_sa, const uint8_t *ea_codes, const int32_t *ea_off,
    const int32_t *ea_len, int32_t n_ea, int match, int mismatch, int gap_open, int gap_extend, int end_size,
    int extra_trim, double end_threshold, int min_trim_size, int32_t *start_trim, int32_t *end_trim,
    int32_t *start_hits, int32_t *end_hits, int64_t cap, int64_t *n_hits, const int32_t *bc_s, int32_t n_bc_s,
    const int32_t *bc_e, int32_t n_bc_e, double *bc_full) {
    if (n_read < 0) return fail(PCABI_E_ARG, "negative count");
    const int64_t nw = 2 * n_read;
    std::vector<int64_t> off((size_t)nw);
    int64_t total = 0;
    for (int64_t w = 0; w < nw; ++w) {
        if (win_len[w] < 0 || win_len[w] > pcabi::MAX_WINDOW_LEN) return fail(PCABI_E_ARG, "window length out of range");
        if (win_len[w] > 0 && !win[w]) return fail(PCABI_E_ARG, "NULL sequence");
        off[(size_t)w] = total;
        total += ((int64_t)win_len[w] + 3) & ~(int64_t)3;
    }
    total += 16;
    return end_decisions_impl(device, nullptr, win, win_len, total, off.data(), win_len, off.data() + n_read,
                              win_len + n_read, n_read, sa_codes, sa_off, sa_len, n_sa, ea_codes, ea_off, ea_len, n_ea,
                              match, mismatch, gap_open, gap_extend, end_size, extra_trim, end_threshold, min_trim_size,
                              start_trim, end_trim, start_hits, end_hits, cap, n_hits, bc_s, n_bc_s, bc_e, n_bc_e,
                              bc_full);
}
