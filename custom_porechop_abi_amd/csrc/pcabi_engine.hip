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
// This unit is the device layer: bucket assignment and dispatch, the decision-epilogue kernels and
// their _dev launchers, prepared adapter tables, the cross products over device pointers, the side
// streams, and the error channel, scratch generation and poison switch every unit shares. The
// device-resident middle scan is pcabi_middle.hip; the entries that take host buffers (and the
// per-device state they keep) are pcabi_hostapi.hip, built on this unit's public ABI. What the
// units share beyond include/pcabi.h is declared in pcabi_host.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
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


// Whether a cross-mode launch of a run-tagged bucket (bucket_pack_mode 2), or of a packed bucket of
// 36..64 rows (bucket_pack_mode 1), runs its inner columns in the gap-extend frame (pcabi_dp.h
// pk::LayS / LanePShift): every adapter passes shift_ok / pshift_range, at one period (the largest
// every adapter allows) and one bias (the middle of the ranges' intersection). Sets p.shift_p /
// p.shift_b (0: the bucket keeps LayT / Lay). The chunk, split and pairs launches keep LayT / Lay.
void bucket_shift(int b, const std::vector<int32_t> &lens, const pcabi::Scoring &sc, int pack_mode, KParams &p) {
    p.shift_p = p.shift_b = 0;
    if (lens.empty() || sc.go == sc.ge) return;
    const char *e = std::getenv("PCABI_SHIFT");   // PCABI_SHIFT=0: every bucket keeps LayT / Lay (A/B measurements)
    if (e && e[0] == '0') return;
    const int rpl = kBuckets[b].rpl;
    if (pack_mode == 1 && kBuckets[b].kind == FAST && rpl >= 36 && rpl <= 64) {
        int P, B;
        if (pcabi::pshift_bucket(lens.data(), (int)lens.size(), rpl, sc, P, B)) {
            p.shift_p = P;
            p.shift_b = B;
        }
        return;
    }
    if (pack_mode != 2) return;
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

}  // namespace pcabi_eng

namespace {

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

}  // namespace

// the host-side layout of every bucket's adapter table (BucketHost: pcabi_host.h)
void pcabi_eng::build_buckets(const uint8_t *adp_codes, const int32_t *adp_off, const int32_t *adp_len,
                              int32_t n_adp, const pcabi::Scoring &sc, BucketHost (&bk)[kNumBuckets], bool merge,
                              bool allow_wide, bool all_striped) {
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


// (pcabi_host.h: the host-buffer unit checks its arguments with these too)
int check_adapter_lens(const int32_t *adp_len, int32_t n_adp) {
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

}  // namespace pcabi_eng

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
    if (int rc = check_adapter_lens(adp_len, n_adp)) return rc;
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
        const int64_t nw = (int64_t)bk[b].pad.size() / 4;   // rows are a multiple of four bytes
        if (a->pad[b].reserve(nw, nw) || a->len[b].reserve(nb, nb) || a->id[b].reserve(nb, nb)) {
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

// Bucket b of a prepared table as launch parameters: its device arrays and, for the cross shape, how
// k_align serves it under the scoring (the return value: bucket_pack_mode; p.shift_p / p.shift_b:
// bucket_shift).
static int record_event(void *ev, hipStream_t st) {
    HIP_TRY(hipEventRecord((hipEvent_t)ev, st));
    return 0;
}

static int bucket_params(const pcabi_adapters *t, int b, const pcabi::Scoring &sc, KParams &p) {
    p.adp_pad = t->pad[b];
    p.adp_len = t->len[b];
    p.adp_id = t->id[b];
    p.n_adp = t->count[b];
    p.rt = t->rt[b];
    const int pack = bucket_pack_mode(b, t->lens[b], sc);
    bucket_shift(b, t->lens[b], sc, pack, p);
    return pack;
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
    delete a;   // the buckets' device arrays free themselves
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
        const int pack = bucket_params(adps, b, p.sc, p);
        const hipStream_t st = fj.at(k);
        // the largest bucket runs on the caller's stream (k == 0): the optional events bracket it
        int rc = k == 0 && ev_begin ? record_event(ev_begin, st) : 0;
        if (!rc) rc = dispatch(b, p, affine, st, pack);
        if (!rc && k == 0 && ev_end) rc = record_event(ev_end, st);
        if (rc) {
            (void)fj.end();
            return rc;
        }
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
            KParams &p = u.p;
            p.tiles = g.tiles;
            p.tile_off = g.tile_off;
            p.win_len = g.win_len;
            p.n_win = g.n_win;
            p.out = g.out;
            p.out_stride = g.out_stride;
            p.sc = sc;
            p.max_cols = g.max_win_len;
            u.pack = bucket_params(adps, b, sc, p);
            u.cls = kBuckets[b].kind == FAST ? group_class(kBuckets[b].rpl, u.pack, affine) : -1;
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
        int rc = k == 0 && ev_begin ? record_event(ev_begin, st) : 0;
        if (!rc && l.cls >= 0) dispatch_group(l.cls, l.gp, l.blocks, st);
        else if (!rc) rc = dispatch(units[l.unit].b, units[l.unit].p, affine, st, units[l.unit].pack);
        if (!rc && k == 0 && ev_end) rc = record_event(ev_end, st);
        if (rc) {
            (void)fj.end();
            return rc;
        }
    }
    if (int rc = fj.end()) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}

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

}  // extern "C"
