// pcabi_middle.hip -- the device-resident middle-adapter scan (pcabi_middle_scan_dev; the reference's
// find_middle_adapters, nanopore_read.py:219-252): the kernels only the scan launches, its scratch
// (pcabi_scan), the shadow arena of the input-preserving masking, the host-driven round loop
// (filtered_first_hits, device_plan_hits) and the queued device rounds (middle_device_rounds).
// The DP cores, the bucket dispatch, the fork / join and the adapter table are the engine's
// (pcabi_host.h, pcabi_kern.h); the seeds are pcabi_seed.hip. k_first_hit stays in the engine, which
// launches it too: the scan reaches it through pcabi_first_hit_dev.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/pcabi.h"
#include "pcabi_dp.h"
#include "pcabi_kern.h"
#include "pcabi_host.h"

using namespace pcabi_eng;

namespace {

// ---- middle-scan score filter (pcabi_dp.h filter_lane) -------------------------------------------
// PCABI_MIDDLE_FILTER=0 in the environment turns it off (A/B timing; results are identical).
bool middle_filter_on() {
    const char *e = std::getenv("PCABI_MIDDLE_FILTER");
    return !(e && e[0] == '0');
}

// Owned end columns per chunk of the middle scan's candidate DP (pcabi_dp.h sf::chunk_plan):
// short enough that the longest read's chunks finish with the rest, long enough that the D-column
// lead-in of each chunk stays a few percent. A round with few candidates (later rounds: the
// reads that just hit) takes shorter chunks, down to kChunkColsMin, while the task list stays
// within kChunkTasks: a launch of a few waves runs as long as its longest chunk, one lane per
// column, so the chunk length is its latency.
constexpr int kChunkCols = 512;
constexpr int kChunkColsMin = 64;
constexpr int64_t kChunkTasks = 65536;

// PCABI_HOSTPROF=1: the middle scan prints its host-side time marks per call to stderr (where the
// host spends the time between the end trim's kernels and the scan's first launch).
struct HostMarks {
    bool on = false;
    std::vector<std::pair<const char *, std::chrono::steady_clock::time_point>> m;
    HostMarks() {
        const char *e = std::getenv("PCABI_HOSTPROF");
        on = e && e[0] == '1';
    }
    void mark(const char *what) {
        if (on) m.emplace_back(what, std::chrono::steady_clock::now());
    }
    ~HostMarks() {
        if (!on || m.empty()) return;
        std::string s;
        for (size_t k = 1; k < m.size(); ++k)
            s += std::string(" ") + m[k].first + "=" +
                 std::to_string(std::chrono::duration<double, std::micro>(m[k].second - m[k - 1].second).count());
        std::fprintf(stderr, "[pcabi hostprof] us:%s\n", s.c_str());
    }
};

thread_local HostMarks *g_hm = nullptr;
inline void hmark(const char *what) {
    if (g_hm) g_hm->mark(what);
}

// PCABI_DEBUG=1: the middle scan prints its candidate counts per round to stderr.
const bool g_debug = [] {
    const char *e = std::getenv("PCABI_DEBUG");
    return e && e[0] == '1';
}();

// Round 1 of the middle scan from exact seeds (pcabi_seed.hip) instead of the score filter:
// PCABI_MIDDLE_SEEDS=0 off, 1 (default) when the cost model prefers them, 2 whenever they apply.
int middle_seed_mode() {
    const char *e = std::getenv("PCABI_MIDDLE_SEEDS");
    if (!e || !e[0]) return 1;
    return e[0] == '0' ? 0 : (e[0] == '2' ? 2 : 1);
}

// Seeded rounds plan their candidate DP on the device (PCABI_MIDDLE_DEVPLAN=0: on the host).
bool middle_devplan_on() {
    const char *e = std::getenv("PCABI_MIDDLE_DEVPLAN");
    return !(e && e[0] == '0');
}

// Queued rounds run the candidate DP over the verified seeds' windows, with the whole read only for
// the candidates whose window winner is a hit the certificate cannot vouch for (k_certify). The
// windows pay on long reads only: the second plan's launches cost more than they save at 8 kb
// (2.90 -> 2.86 ms), break even at 12 kb and win 10-12 % from 16 kb (20 kb: 4.21 -> 3.70 ms,
// profiles/r03/final/windows_sweep/). So they run when the batch's mean read length reaches
// kWindowsMeanLen -- from the host lengths when the caller passes them, else from the previous
// call's round-1 segment total (pcabi_scan::last_mean). PCABI_MIDDLE_WINDOWS=1 / 0 forces them.
constexpr double kWindowsMeanLen = 10000.0;   // r05ac in-process A/B (graphs off): off 1.99 / on 2.03 ms at
                                              // 8 kb, off 2.50 / on 2.29 at 14 kb, off 3.21 / on 2.74 at 20 kb
bool middle_windows_on(double mean_len) {
    const char *e = std::getenv("PCABI_MIDDLE_WINDOWS");
    if (e && e[0] == '1') return true;
    if (e && e[0] == '0') return false;
    return mean_len >= kWindowsMeanLen;
}

// Queued rounds from this index on (0 = round 1) launch their band classes and candidate-DP
// buckets one after the other on the scan's stream: after round 1 only the reads that hit are
// left, their launches last a few microseconds, and each fork / join over side streams costs
// ~15-20 us of event latency (profiles/r03/final/kernel_trace_middle_8kb.csv). r05at (in-process
// A/B, profiles/r05/at/): from round 2 on (1) 1.93 ms at 8 kb / 2.53 at 20 kb, against 1.96-1.99 /
// 2.65-2.69 from round 3 on (2, the r03-r05 default, round 2 replayed from a graph) and 2.02 /
// 2.51 with round 1 serial too (0). Captured round graphs (run_round) hold only serial rounds: a
// capture never records another caller's work on the shared side streams.
constexpr int kMiddleSerialFrom = 1;

// Device planning aims at this many waves per candidate-DP round (4 per SIMD): the chunk length
// is the longest of 512, 256, 128, 64 owned columns that still reaches it.
int64_t middle_plan_waves() {
    const char *e = std::getenv("PCABI_MIDDLE_PLAN_WAVES");
    return (e && e[0]) ? std::max<int64_t>(1, std::atoll(e)) : 4096;
}


// Views of a subset of windows: sub[k] = window idx[k].
__global__ __launch_bounds__(256) void k_gather_views(const int64_t *win_off, const int32_t *win_len,
                                                      const int32_t *idx, int64_t n, int64_t *sub_off,
                                                      int32_t *sub_len) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    sub_off[k] = win_off[idx[k]];
    sub_len[k] = win_len[idx[k]];
}

// ---- input-preserving masking (r05) ------------------------------------------------------------
// The reference masks a COPY of the read (nanopore_read.py:225 masked_seq = the trimmed read, :234
// rebuilt with '-'), so the caller's sequence is never touched. The scan does the same on the
// device: the caller's codes are read-only, and a read's first hit copies the whole window into a
// shadow arena owned by the scan (16-byte aligned, zero tail padding for the window readers'
// look-ahead), with the hit's span masked as it is copied; from then on the read's effective offset
// eoff[w] (an offset from `codes`, like win_off) points at the copy, which later hits mask in place.
// Only reads that hit are ever copied (round 1: ~4.5 % of a batch); every round after round 1 runs
// on reads that hit in round 1 only.
__device__ __forceinline__ int64_t shadow_bytes(int32_t len) { return ((int64_t)max(len, 0) + 16 + 15) & ~(int64_t)15; }

// Masking of a round's hits (nanopore_read.py:245, the span becomes '-', Dna5 N): the blocks stride
// over the list (8 int32 per hit, k_round_hits' layout), a block's threads over the read. o[7] > 0:
// the read's first hit, shadow at arena byte (o[7] - 1) * 16 (k_round_hits' allocation): the window
// is copied from the caller's codes with the span masked, and eoff redirected; o[7] == 0: the read
// already has its copy (eoff), the span is masked there. *bump > cap (the round's allocations did
// not fit): nothing is copied or masked, the round is flagged (rflag bit 8) and holds no next round,
// so the host grows the arena and queues it again.
__global__ __launch_bounds__(256) void k_mask_list(const uint8_t *codes, const int64_t *win_off, int64_t *eoff,
                                                   const int32_t *win_len, const int32_t *list, int32_t *n_dev,
                                                   uint8_t *arena, int64_t arena_rel, int64_t cap,
                                                   const unsigned long long *bump, int32_t *rflag) {
    if ((int64_t)*bump > cap) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            if (rflag) *rflag |= 8;
            *n_dev = 0;
        }
        return;
    }
    const int64_t nh = *n_dev;
    for (int64_t j = blockIdx.x; j < nh; j += gridDim.x) {
        const int32_t *o = list + 8 * j;
        const int32_t w = o[0], rs = o[2], rend = rs == -1 ? 0 : o[3] + 1;
        if (o[7] > 0) {
            // 16 bytes per thread and pass: the source's aligned dwords (those holding a byte of the
            // window: the caller's padding is not assumed), shifted into place, the span masked,
            // bytes past the window zero, one 16-byte store
            const int64_t at = (int64_t)(o[7] - 1) * 16;
            const int32_t len = win_len[w];
            const int64_t nb = shadow_bytes(len);
            const uintptr_t sa = (uintptr_t)(codes + win_off[w]);
            const uint32_t *s4 = reinterpret_cast<const uint32_t *>(sa & ~(uintptr_t)3);
            const int a0 = (int)(sa & 3), sh = 8 * a0;
            const int64_t lim = (int64_t)len + a0;      // source dword k holds window bytes iff 4k < lim
            uint4 *dst = reinterpret_cast<uint4 *>(arena + at);
            for (int64_t c = threadIdx.x; c * 16 < nb; c += 256) {
                uint32_t d[5];
#pragma unroll
                for (int k = 0; k < 5; ++k) d[k] = (4 * (4 * c + k) < lim) ? s4[4 * c + k] : 0u;
                uint32_t v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    uint32_t x = sh ? __builtin_amdgcn_alignbit(d[i + 1], d[i], sh) : d[i];
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int64_t pos = 16 * c + 4 * i + b;
                        const uint32_t m = 0xFFu << (8 * b);
                        if (pos >= len) x &= ~m;
                        else if (pos >= rs && pos < rend) x = (x & ~m) | (4u << (8 * b));
                    }
                    v[i] = x;
                }
                dst[c] = make_uint4(v[0], v[1], v[2], v[3]);
            }
            if (threadIdx.x == 0) eoff[w] = arena_rel + at;
        } else {
            // the copy already exists: eoff[w] lies in the arena
            uint8_t *dst = arena + (eoff[w] - arena_rel);
            for (int64_t i = rs + threadIdx.x; i < rend; i += 256) dst[i] = 4;
        }
    }
}

// The arena moved (grown): every redirected offset follows it.
__global__ __launch_bounds__(256) void k_shadow_rebase(const int64_t *win_off, int64_t *eoff, int64_t n, int64_t delta) {
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256)
        if (eoff[k] != win_off[k]) eoff[k] += delta;
}

// ---- device-planned candidate DP (middle scan, seeded rounds) --------------------------------
// The seeds leave the candidate pairs on the device as unordered keys (adapter << 32 | window).
// k_plan_count counts each adapter's tasks for the four chunk lengths, the host lays the waves
// out (one adapter per wave, adapters in bucket order: n_adp numbers, not tasks), k_plan_place
// writes the task slots, the DP runs per bucket, and k_merge_* pick per candidate the first chunk
// (read order) with the largest score, then per window the first adapter (list order) whose
// full identity is not below the threshold -- the host path's rules (filtered_first_hits).
constexpr int kPlanC = 5;     // chunk lengths kPlanMin << c, c = 0..4
constexpr int kPlanMin = 32;  // (r05: 32-column chunks for the few whole reads a round certifies)

__device__ __forceinline__ int plan_tasks(int len, int span, int c) {
    if (span < 0) return 1;                          // whole windows
    const int C = kPlanMin << c;
    return (len + C - 1) / C;                        // sf::chunk_plan's chunk count
}

__device__ __forceinline__ bool plan_valid(int64_t key, const int32_t *v_len, const int32_t *start) {
    const int32_t a = (int32_t)(key >> 32), k = (int32_t)(key & 0xFFFFFFFF);
    return v_len[k] > 0 && (!start || a >= start[k]);
}

// Wave helpers (every lane of the wave takes part): sum, inclusive scan.
__device__ __forceinline__ int wave_sum(int x) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
    return x;
}
__device__ __forceinline__ int wave_incl_scan(int x) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    return x;
}

// Candidates of one adapter are typically many (the reads' own adapter), so the per-adapter
// counters are updated once per (wave, adapter): the lanes of one adapter are reduced first.
// nc_dev != nullptr: the candidate count is on the device (at most nc); the blocks stride.
__global__ __launch_bounds__(256) void k_plan_count(const int64_t *cand, int64_t nc, const unsigned long long *nc_dev,
                                                    const int32_t *v_len, const int32_t *start, const int32_t *span,
                                                    int32_t *adp_tasks, const int32_t *cmask) {
    const int64_t ncl = nc_dev ? min((int64_t)*nc_dev, nc) : nc;
    const int lane = threadIdx.x & 63;
    for (int64_t b0 = (int64_t)blockIdx.x * 256; b0 < ncl; b0 += (int64_t)gridDim.x * 256) {   // uniform
        const int64_t i = b0 + threadIdx.x;
        const int64_t key = i < ncl ? cand[i] : 0;
        const bool active = i < ncl && plan_valid(key, v_len, start) && (!cmask || cmask[i]);
        const int32_t a = active ? (int32_t)(key >> 32) : -1;
        int nt[kPlanC] = {};
        if (active) {
            const int32_t k = (int32_t)(key & 0xFFFFFFFF);
#pragma unroll
            for (int c = 0; c < kPlanC; ++c) nt[c] = plan_tasks(v_len[k], span[a], c);
        }
        uint64_t pending = __ballot(active);
        while (pending) {                            // wave-uniform
            const int leader = __ffsll((unsigned long long)pending) - 1;
            const int32_t a0 = __shfl(a, leader);
            const bool mine = active && a == a0;
#pragma unroll
            for (int c = 0; c < kPlanC; ++c) {
                const int sum = wave_sum(mine ? nt[c] : 0);
                if (lane == leader) atomicAdd(&adp_tasks[a0 * kPlanC + c], sum);
            }
            pending &= ~__ballot(mine);
        }
    }
}

// Task slots: adapter a's tasks fill slots [wave_off[a] * 64, ...) in any order (a slot's result
// depends only on its own task); idle slots keep task_win = -1. cidx[a]: the chunk length of a's
// bucket (kPlanMin << cidx). nc_dev / slots_dev (device counts, nullptr: host values): the candidate
// count, and the slots the layout holds (a task past them is not written: the layout overflowed).
__global__ __launch_bounds__(256) void k_plan_place(const int64_t *cand, int64_t nc, const unsigned long long *nc_dev,
                                                    const int32_t *v_len, const int32_t *start, const int32_t *span,
                                                    const int32_t *cidx, const int64_t *wave_off, int32_t *fill,
                                                    int32_t *tw, int32_t *to, int4 *tck, int32_t *tcand,
                                                    const int64_t *slots_dev, int32_t *cbase_out, const int32_t *cmask) {
    const int64_t ncl = nc_dev ? min((int64_t)*nc_dev, nc) : nc;
    const int64_t slots = slots_dev ? *slots_dev : INT64_MAX;
    const int lane = threadIdx.x & 63;
    for (int64_t b0 = (int64_t)blockIdx.x * 256; b0 < ncl; b0 += (int64_t)gridDim.x * 256) {   // uniform
        const int64_t i = b0 + threadIdx.x;
        const int64_t key = i < ncl ? cand[i] : 0;
        const bool active = i < ncl && plan_valid(key, v_len, start) && (!cmask || cmask[i]);
        const int32_t a = active ? (int32_t)(key >> 32) : -1, k = (int32_t)(key & 0xFFFFFFFF);
        int n = 0, D = -1, c = 0, nt = 0;
        if (active) {
            n = v_len[k];
            D = span[a];
            c = cidx[a];
            nt = plan_tasks(n, D, c);
        }
        int64_t base = 0;
        uint64_t pending = __ballot(active);
        while (pending) {                            // wave-uniform: one atomic per (wave, adapter)
            const int leader = __ffsll((unsigned long long)pending) - 1;
            const int32_t a0 = __shfl(a, leader);
            const bool mine = active && a == a0;
            const int x = mine ? nt : 0;
            const int incl = wave_incl_scan(x);
            const int total = __shfl(incl, 63);
            int b1 = 0;
            if (lane == leader) b1 = atomicAdd(&fill[a0], total);
            b1 = __shfl(b1, leader);
            if (mine) base = wave_off[a0] * 64 + b1 + (incl - x);
            pending &= ~__ballot(mine);
        }
        if (cbase_out) {                             // the tasks are written by k_plan_fill
            if (i < ncl) cbase_out[i] = active ? (int32_t)base : -1;
            continue;
        }
        if (!active) continue;
        const int C = kPlanMin << c;
        for (int t = 0; t < nt; ++t) {
            const int64_t q = base + t;
            if (q >= slots) break;
            int4 ck = make_int4(0, 0, 0, 0);
            if (D >= 0) {                            // sf::chunk_plan, chunk t
                const int lo = 1 + t * C, hi = lo + C;
                const int st = max(0, lo - 1 - D);
                ck = hi > n ? make_int4(st, n - st, lo - st, -1) : make_int4(st, hi - 1 - st, lo - st, hi - st);
            }
            tw[q] = k;
            to[q] = (int32_t)q;
            tck[q] = ck;
            tcand[q] = (int32_t)i;
        }
    }
}

// The task slots of k_plan_place's candidates, one wave per candidate (its lanes over the chunks):
// a read of 8 kb has 63 chunks of 128 columns, which one lane wrote one after another.
__global__ __launch_bounds__(256) void k_plan_fill(const int64_t *cand, int64_t nc, const unsigned long long *nc_dev,
                                                   const int32_t *v_len, const int32_t *span, const int32_t *cidx,
                                                   const int32_t *cbase, int32_t *tw, int32_t *to, int4 *tck,
                                                   int32_t *tcand, const int64_t *slots_dev) {
    const int64_t ncl = nc_dev ? min((int64_t)*nc_dev, nc) : nc;
    const int64_t slots = *slots_dev;
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * 4;
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < ncl; i += waves) {
        const int32_t base = cbase[i];
        if (base < 0) continue;                      // wave-uniform
        const int64_t key = cand[i];
        const int32_t a = (int32_t)(key >> 32), k = (int32_t)(key & 0xFFFFFFFF);
        const int n = v_len[k], D = span[a], c = cidx[a];
        const int nt = plan_tasks(n, D, c), C = kPlanMin << c;
        for (int t = lane; t < nt; t += 64) {
            const int64_t q = (int64_t)base + t;
            if (q >= slots) break;
            int4 ck = make_int4(0, 0, 0, 0);
            if (D >= 0) {                            // sf::chunk_plan, chunk t
                const int lo = 1 + t * C, hi = lo + C;
                const int st = max(0, lo - 1 - D);
                ck = hi > n ? make_int4(st, n - st, lo - st, -1) : make_int4(st, hi - 1 - st, lo - st, hi - st);
            }
            tw[q] = k;
            to[q] = (int32_t)q;
            tck[q] = ck;
            tcand[q] = (int32_t)i;
        }
    }
}

// ---- candidate windows (device rounds, PCABI_MIDDLE_WINDOWS): one chunk per verified seed ------
// A verified seed (pcabi_seed.hip put_verified: read, adapter | E << 24, the diagonal's codes offset)
// is a band task of a candidate pair whose bound reached T. Every alignment of the pair scoring >= T
// holds an exact piece, whose task is verified, and stays within E diagonals of it: it ends in row L
// at a column of d0 + L - E .. d0 + L + E, or in the read's last column when the band reaches it. One
// chunk per verified seed that owns those columns (started D + 1 columns earlier: sf::chunk_plan's
// rule, so an owned cell >= T gets the whole read's score and attributes) replaces the pair's
// whole-read chunks -- 8 kb x L cells become ~(D + 2E) x L. The merge's rules are unchanged and
// still give the whole-read answer whenever it reaches T: the largest score, then the smallest first
// owned column (overlapping windows of one pair report the same first maximum of a shared cell).
__device__ __forceinline__ bool wseed_valid(const int4 &v, const int32_t *v_len, const int32_t *start) {
    const int32_t a = v.y & 0xFFFFFF, k = v.x;
    return v_len[k] > 0 && (!start || a >= start[k]);
}

__device__ __forceinline__ int4 wseed_chunk(const int4 &v, const int64_t *v_off, const int32_t *v_len,
                                            const int32_t *alen, const int32_t *span) {
    const int32_t a = v.y & 0xFFFFFF, E = (int32_t)((uint32_t)v.y >> 24), k = v.x;
    const int64_t dabs = (int64_t)(((uint64_t)(uint32_t)v.w << 32) | (uint32_t)v.z);
    const int d0 = (int)(dabs - v_off[k]);
    const int n = v_len[k], L = alen[a], D = span[a];
    int lo = max(1, d0 + L - E);
    const int hi = d0 + L + E + 1;
    if (hi > n) {                                    // the band reaches the read end: the last chunk
        lo = min(lo, n);
        const int st = max(0, lo - 1 - D);
        return make_int4(st, n - st, lo - st, -1);
    }
    const int st = max(0, lo - 1 - D);
    return make_int4(st, hi - 1 - st, lo - st, hi - st);
}

// Per adapter its windows (the same count under every chunk length, so k_plan_layout's choice does
// not matter): one atomic per (wave, adapter).
__global__ __launch_bounds__(256) void k_wplan_count(const int4 *vl, const int32_t *vcount, int64_t vcap,
                                                     const int32_t *v_len, const int32_t *start, int32_t *adp_tasks) {
    const int64_t nv = min((int64_t)*vcount, vcap);
    const int lane = threadIdx.x & 63;
    for (int64_t b0 = (int64_t)blockIdx.x * 256; b0 < nv; b0 += (int64_t)gridDim.x * 256) {   // uniform
        const int64_t i = b0 + threadIdx.x;
        const int4 v = i < nv ? vl[i] : make_int4(0, 0, 0, 0);
        const bool active = i < nv && wseed_valid(v, v_len, start);
        const int32_t a = active ? (v.y & 0xFFFFFF) : -1;
        uint64_t pending = __ballot(active);
        while (pending) {                            // wave-uniform
            const int leader = __ffsll((unsigned long long)pending) - 1;
            const int32_t a0 = __shfl(a, leader);
            const bool mine = active && a == a0;
            const int sum = wave_sum(mine ? 1 : 0);
            if (lane == leader)
                for (int c = 0; c < kPlanC; ++c) atomicAdd(&adp_tasks[a0 * kPlanC + c], sum);
            pending &= ~__ballot(mine);
        }
    }
}

// The window task slots (k_plan_place's layout: adapter a's tasks from wave_off[a] * 64), the
// candidate of each from the pair map k_cands wrote (pmap, row stride n).
__global__ __launch_bounds__(256) void k_wplan_place(const int4 *vl, const int32_t *vcount, int64_t vcap,
                                                     const int64_t *v_off, const int32_t *v_len, const int32_t *start,
                                                     const int32_t *alen, const int32_t *span, const int32_t *pmap,
                                                     int64_t n, const int64_t *wave_off, int32_t *fill, int32_t *tw,
                                                     int32_t *to, int4 *tck, int32_t *tcand, const int64_t *slots_dev) {
    const int64_t nv = min((int64_t)*vcount, vcap);
    const int64_t slots = *slots_dev;
    const int lane = threadIdx.x & 63;
    for (int64_t b0 = (int64_t)blockIdx.x * 256; b0 < nv; b0 += (int64_t)gridDim.x * 256) {   // uniform
        const int64_t i = b0 + threadIdx.x;
        const int4 v = i < nv ? vl[i] : make_int4(0, 0, 0, 0);
        const bool active = i < nv && wseed_valid(v, v_len, start);
        const int32_t a = active ? (v.y & 0xFFFFFF) : -1;
        int64_t q = 0;
        uint64_t pending = __ballot(active);
        while (pending) {                            // wave-uniform: one atomic per (wave, adapter)
            const int leader = __ffsll((unsigned long long)pending) - 1;
            const int32_t a0 = __shfl(a, leader);
            const bool mine = active && a == a0;
            const int x = mine ? 1 : 0;
            const int incl = wave_incl_scan(x);
            const int total = __shfl(incl, 63);
            int b1 = 0;
            if (lane == leader) b1 = atomicAdd(&fill[a0], total);
            b1 = __shfl(b1, leader);
            if (mine) q = wave_off[a0] * 64 + b1 + (incl - x);
            pending &= ~__ballot(mine);
        }
        if (!active || q >= slots) continue;
        tw[q] = v.x;
        to[q] = (int32_t)q;
        tck[q] = wseed_chunk(v, v_off, v_len, alen, span);
        tcand[q] = pmap[(int64_t)a * n + v.x];
    }
}

// Merge key of a task: larger score first, then the earlier chunk. Chunks are told apart by their
// first owned column (start + own_lo, unique per chunk), not by their start: near the read
// start several chunks begin at offset 0.
__device__ __forceinline__ uint64_t merge_key(int32_t score, int4 ck) {
    return ((uint64_t)((uint32_t)score ^ 0x80000000u) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)(ck.x + ck.z));
}

// A candidate's chunk tasks sit in consecutive slots, so a wave's lanes mostly share a few
// candidates: a segmented max over each run of equal candidates (shuffles) leaves one atomic per
// run instead of one per task (64 same-address atomics per wave serialised: ~48 us of round 1).
__global__ __launch_bounds__(256) void k_merge_best(const int32_t *tw, const int4 *tck, const int32_t *tcand,
                                                    const int32_t *res, int64_t slots, const int64_t *slots_dev,
                                                    unsigned long long *best) {
    const int64_t ns = slots_dev ? *slots_dev : slots;
    const int lane = threadIdx.x & 63;
    for (int64_t b0 = (int64_t)blockIdx.x * 256; b0 < ns; b0 += (int64_t)gridDim.x * 256) {   // block-uniform
        const int64_t q = b0 + threadIdx.x;
        const bool live = q < ns && tw[q] >= 0;
        const int32_t cand = live ? tcand[q] : -1 - lane;           // idle lanes: runs of their own
        unsigned long long key = live ? (unsigned long long)merge_key(res[4 * slots + q], tck[q]) : 0ull;
        const int32_t prev = __shfl_up(cand, 1);
        const uint64_t heads = __ballot(lane == 0 || prev != cand);
        const int start = 63 - __clzll(heads & ((2ull << lane) - 1ull));   // this lane's run head
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long o = __shfl_up(key, d);
            if (lane - d >= start) key = key > o ? key : o;
        }
        const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
        if (live && tail) atomicMax(&best[cand], key);
    }
}

// The candidate windows' certificate, per window slot that holds its candidate's best (k_merge_best):
// only a winner that is a hit (full identity not below the threshold) needs one. If the whole
// read's best alignment A* were a hit, it would have an exact piece and stay in its band, so it
// would be in a window and be the windows' winner; so a winner that is no hit proves the pair has
// no hit. A winner that is a hit is the whole read's best when its score is above U[a] (pcabi_seed
// cert_bounds: every alignment without an exact piece, or with more gap columns than the band
// allows, scores at most U[a]; U[a] >= T - 1). Otherwise the candidate is flagged (cmask 1, its
// window best dropped) and its whole read runs in chunks. Block 0 also clears the plan counters for
// that second plan.
__global__ __launch_bounds__(256) void k_certify(const int64_t *cand, const int32_t *tw, const int4 *tck,
                                                 const int32_t *tcand, const int32_t *res, int64_t slots,
                                                 const int64_t *slots_dev, double thr, const int32_t *U,
                                                 unsigned long long *best, int32_t *cmask, int32_t *adp_tasks,
                                                 int32_t *fill, int32_t n_adp) {
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i < n_adp * kPlanC; i += 256) adp_tasks[i] = 0;
        for (int i = threadIdx.x; i < n_adp; i += 256) fill[i] = 0;
    }
    const int64_t ns = *slots_dev;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < ns; q += (int64_t)gridDim.x * 256) {
        if (tw[q] < 0) continue;
        const int32_t ci = tcand[q];
        const int32_t score = res[4 * slots + q];
        if ((unsigned long long)merge_key(score, tck[q]) != best[ci]) continue;
        const int rs = res[0 * slots + q];
        const double full = rs == -1 ? 0.0 : pcabi::pid6(res[5 * slots + q], res[7 * slots + q]);
        if (full < thr) continue;                    // no hit: the pair has none (NaN is a hit, as k_merge_hit)
        if (score > U[(int32_t)(cand[ci] >> 32)]) continue;
        cmask[ci] = 1;
        best[ci] = 0ull;
    }
}

// pass 0: per window the smallest adapter whose winning chunk reaches the threshold (atomicMin);
// pass 1: that candidate writes the window's hit (rs / re back to whole-window offsets).
// slots: the result rows' stride; slots_dev: the live slots (nullptr: all).
__global__ __launch_bounds__(256) void k_merge_hit(const int64_t *cand, const int32_t *tw, const int4 *tck,
                                                   const int32_t *tcand, const int32_t *res, int64_t slots,
                                                   const int64_t *slots_dev, const unsigned long long *best, double thr,
                                                   int pass, int32_t *hit_a, int32_t *hb, int64_t n,
                                                   const int32_t *cmask, int want) {
    const int64_t ns = slots_dev ? *slots_dev : slots;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < ns; q += (int64_t)gridDim.x * 256) {
        if (tw[q] < 0) continue;
        const int32_t ci = tcand[q];
        if (cmask && cmask[ci] != want) continue;    // (candidate windows: this plan does not decide it)
        const int4 ck = tck[q];
        const int32_t st = ck.x;
        if ((unsigned long long)merge_key(res[4 * slots + q], ck) != best[ci]) continue;
        const int rs = res[0 * slots + q];
        const int m = res[5 * slots + q], l2 = res[7 * slots + q];
        const double full = rs == -1 ? 0.0 : pcabi::pid6(m, l2);
        if (full < thr) continue;                    // NaN goes on, as the reference's loop
        const int32_t k = tw[q], a = (int32_t)(cand[ci] >> 32);
        if (pass == 0) {
            atomicMin(&hit_a[k], a);
        } else if (hit_a[k] == a) {
            hb[0 * n + k] = a;
            hb[1 * n + k] = rs + st;
            hb[2 * n + k] = res[1 * slots + q] + st;
            hb[3 * n + k] = m;
            hb[4 * n + k] = l2;
        }
    }
}

// The windows that hit, compacted (window, adapter, rs, re, m, l2), in any order.
__global__ __launch_bounds__(256) void k_hits_compact(const int32_t *hb, int64_t n, int32_t *out,
                                                      unsigned int *cnt) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n || hb[k] < 0) return;
    const unsigned int j = atomicAdd(cnt, 1u);
    int32_t *o = out + 6 * (int64_t)j;
    o[0] = (int32_t)k;
#pragma unroll
    for (int f = 0; f < 5; ++f) o[1 + f] = hb[f * n + k];
}


// ---- queued middle-scan rounds (middle_device_rounds): the kernels between the seeded plan's ------
// steps, every count read on the device

// Start of a round: views of its windows (sub[k] = window cur[k], k < n_dev; cur == nullptr: none,
// round 1 reads the windows themselves) and the round's counters zeroed -- the next round's read
// count, the plan flag, the plan's per-adapter task counts (n_adp x kPlanC) and fill counters.
// n_first != nullptr (round 1): its read count, n_first_val, is written too.
__global__ __launch_bounds__(256) void k_round_views(const int64_t *win_off, const int32_t *win_len, const int32_t *cur,
                                                     const int32_t *n_dev, int64_t *sub_off, int32_t *sub_len,
                                                     int32_t *n_next, int32_t *plan_flag, int32_t *ptasks,
                                                     int32_t *pfill, int32_t n_adp, int32_t *n_first,
                                                     int32_t n_first_val) {
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) {
            *n_next = 0;
            *plan_flag = 0;
            if (n_first) *n_first = n_first_val;
        }
        for (int i = threadIdx.x; i < n_adp * kPlanC; i += 256) ptasks[i] = 0;
        for (int i = threadIdx.x; i < n_adp; i += 256) pfill[i] = 0;
    }
    if (!cur) return;
    const int64_t n = *n_dev;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256) {
        sub_off[k] = win_off[cur[k]];
        sub_len[k] = win_len[cur[k]];
    }
}

// Before the merges: the candidates' best keys zeroed (k < *n_cand), the round's per-window hit
// adapter (INT32_MAX) and hit table row 0 (-1) reset (k < *n_dev).
__global__ __launch_bounds__(256) void k_merge_reset(unsigned long long *best, const unsigned long long *n_cand, int64_t cap,
                                                     int32_t *hit_a, int32_t *hb, const int32_t *n_dev,
                                                     int32_t *cmask) {
    const int64_t nc = min((int64_t)*n_cand, cap), nr = *n_dev;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nc; i += (int64_t)gridDim.x * 256) {
        best[i] = 0ull;
        if (cmask) cmask[i] = 0;
    }
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < nr; k += (int64_t)gridDim.x * 256) {
        hit_a[k] = INT32_MAX;
        hb[k] = -1;
    }
}

// Profile counters (pcabi_scan_profile): a round's reads and bases, and a plan's tasks and DP cells
// (columns x adapter rows; a whole-window task, chunk (0, 0, 0, 0), computes its window).
__global__ __launch_bounds__(256) void k_prof_round(const int32_t *v_len, const int32_t *n_dev, unsigned long long *out) {
    const int64_t n = *n_dev;
    unsigned long long b = 0;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256) b += (uint32_t)v_len[k];
    for (int d = 32; d > 0; d >>= 1) b += __shfl_xor(b, d);
    if ((threadIdx.x & 63) == 0) atomicAdd(&out[1], b);
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&out[0], (unsigned long long)n);
}

__global__ __launch_bounds__(256) void k_prof_cells(const int32_t *tw, const int4 *tck, const int32_t *tcand,
                                                    const int64_t *cand, const int32_t *v_len, const int32_t *alen,
                                                    const int64_t *slots_dev, unsigned long long *out) {
    const int64_t ns = *slots_dev;
    unsigned long long t = 0, c = 0;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < ns; q += (int64_t)gridDim.x * 256) {
        const int32_t k = tw[q];
        if (k < 0) continue;
        const int4 ck = tck[q];
        const int32_t a = (int32_t)(cand[tcand[q]] >> 32);
        const int cols = (ck.x | ck.y | ck.z | ck.w) ? ck.y : v_len[k];
        t += 1;
        c += (unsigned long long)cols * (uint32_t)alen[a];
    }
    for (int d = 32; d > 0; d >>= 1) {
        t += __shfl_xor(t, d);
        c += __shfl_xor(c, d);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&out[2], t);
        atomicAdd(&out[3], c);
    }
}

// The device plan's layout (device_plan_hits' host part, on the device, one block): per bucket
// the longest chunk length whose waves reach `target` (else the shortest), every adapter's wave
// offset (buckets in order, a bucket's adapters in order, one adapter per wave), the wave ->
// bucket-local adapter table, the idle lanes of every adapter's last wave (task -1), and per
// bucket (first wave, waves). More slots than slots_cap: flag, need = the slots, no waves.
//   bk_first[n_bk + 1]: the buckets' ranges of bk_adp (global adapter ids) / bk_local (their
//   index in the bucket's table); tasks[a * kPlanC + c]: k_plan_count's counts.
__global__ __launch_bounds__(256) void k_plan_layout(const int32_t *tasks, int32_t n_bk, const int32_t *bk_first,
                                                     const int32_t *bk_adp, const int32_t *bk_local, int64_t target,
                                                     int64_t slots_cap, int32_t *cidx, int64_t *woff, int32_t *wa,
                                                     int32_t *tw, int32_t *bk_waves, int64_t *slots_total,
                                                     int32_t *flag, int64_t *need) {
    typedef hipcub::BlockScan<long long, 256> Scan;
    __shared__ typename Scan::TempStorage scan_tmp;
    __shared__ unsigned long long s_w[kNumBuckets][kPlanC];
    __shared__ int s_bc[kNumBuckets];
    __shared__ long long s_carry;
    const int32_t n_all = bk_first[n_bk];
    for (int i = threadIdx.x; i < kNumBuckets * kPlanC; i += 256) s_w[i / kPlanC][i % kPlanC] = 0;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    auto bucket_of = [&](int32_t j) {
        int32_t b = 0;
        while (b + 1 < n_bk && bk_first[b + 1] <= j) ++b;
        return b;
    };
    // per bucket the waves of each chunk length; the longest length whose waves reach the target
    for (int32_t j = threadIdx.x; j < n_all; j += 256) {
        const int32_t a = bk_adp[j], b = bucket_of(j);
#pragma unroll
        for (int c = 1; c < kPlanC; ++c) atomicAdd(&s_w[b][c], (unsigned long long)((tasks[a * kPlanC + c] + 63) / 64));
    }
    __syncthreads();
    for (int32_t b = threadIdx.x; b < n_bk; b += 256) {
        int bc = 0;
        for (int c = kPlanC - 1; c > 0; --c)
            if ((int64_t)s_w[b][c] >= target) {
                bc = c;
                break;
            }
        s_bc[b] = bc;
    }
    __syncthreads();
    // wave offsets: an exclusive scan over the adapters (buckets in order, a bucket's in order)
    for (int32_t j0 = 0; j0 < n_all; j0 += 256) {      // block-uniform
        const int32_t j = j0 + threadIdx.x;
        long long w = 0;
        int32_t a = -1, b = 0;
        if (j < n_all) {
            a = bk_adp[j];
            b = bucket_of(j);
            cidx[a] = s_bc[b];
            w = (tasks[a * kPlanC + s_bc[b]] + 63) / 64;
        }
        long long ex, tot;
        Scan(scan_tmp).ExclusiveSum(w, ex, tot);
        ex += s_carry;
        if (a >= 0) woff[a] = ex;
        __syncthreads();
        if (threadIdx.x == 0) s_carry += tot;
        __syncthreads();
    }
    const int64_t slots = s_carry * 64;
    for (int32_t b = threadIdx.x; b < n_bk; b += 256) {
        const int64_t lo = bk_first[b] < n_all ? woff[bk_adp[bk_first[b]]] : s_carry;
        const int64_t hi = bk_first[b + 1] < n_all ? woff[bk_adp[bk_first[b + 1]]] : s_carry;
        bk_waves[2 * b] = (int32_t)lo;
        bk_waves[2 * b + 1] = slots > slots_cap ? 0 : (int32_t)(hi - lo);
    }
    if (slots > slots_cap) {                         // too small: no waves, the round reruns larger
        if (threadIdx.x == 0) {
            *flag = 1;
            *need = slots;
            *slots_total = 0;
        }
        return;
    }
    if (threadIdx.x == 0) *slots_total = slots;
    // the wave -> bucket-local adapter table and the idle lanes of every adapter's last wave: one
    // wave per adapter
    const int lane = threadIdx.x & 63;
    for (int32_t j = threadIdx.x >> 6; j < n_all; j += 4) {
        const int32_t a = bk_adp[j];
        const int32_t nt = tasks[a * kPlanC + cidx[a]];
        const int64_t nw = (nt + 63) / 64, w0 = woff[a];
        for (int64_t w = lane; w < nw; w += 64) wa[w0 + w] = bk_local[j];
        const int64_t t = nt + lane;
        if (t < nw * 64) tw[w0 * 64 + t] = -1;
    }
}

// A round's hits (k_merge_hit's per-window table hb, row stride n) -> the round's list (8 int32
// each: read, adapter, rs, re, m, l2, position, 0), the next round's reads (those that hit, from
// the adapter that hit) and their count. A round whose seed / plan buffers overflowed keeps nothing
// (no hits, no next round, no masking): the host sees rflag and reruns it with larger buffers.
// (r04) The list is an ORDERED compaction -- a round's hits in the order of its reads, which round
// 1 takes in read order -- so every round's list is sorted by read and the host concatenates the
// rounds without sorting (an indirect std::sort of ~5 k hits cost ~0.1-0.4 ms of host time per
// call). k_round_count counts each 256-entry chunk's hits; a chunk's base is the sum of the counts
// before it (summed by the block: a few hundred chunks), its hits' places a block scan.
__global__ __launch_bounds__(256) void k_round_count(const int32_t *hb, const int32_t *n_dev, const int32_t *seed_flags,
                                                     const int32_t *plan_flag, int32_t *counts) {
    if (seed_flags[0] || seed_flags[1] || *plan_flag) return;
    const int64_t nr = *n_dev, nch = (nr + 255) / 256;
    for (int64_t c = blockIdx.x; c < nch; c += gridDim.x) {   // block-uniform
        const int64_t k = c * 256 + threadIdx.x;
        const int cnt = __syncthreads_count(k < nr && hb[k] >= 0);
        if (threadIdx.x == 0) counts[c] = cnt;
    }
}

// (r05) A read's first masked hit also takes its shadow-arena space here (k_mask_list copies it):
// one atomic per block over the block's scanned sizes; o[7] = 1 + the 16-byte unit it starts at.
__global__ __launch_bounds__(256) void k_round_hits(const int32_t *hb, int64_t n, const int32_t *n_dev, const int32_t *cur,
                                                    const int32_t *counts, int32_t *list, int32_t *n_next,
                                                    int32_t *cur_next, int32_t *start_next, const int32_t *seed_flags,
                                                    const int32_t *plan_flag, int32_t *rflag, const int64_t *win_off,
                                                    const int64_t *eoff, const int32_t *win_len,
                                                    unsigned long long *bump) {
    typedef hipcub::BlockScan<int, 256> Scan;
    typedef hipcub::BlockScan<long long, 256> Scan64;
    __shared__ typename Scan::TempStorage scan_tmp;
    __shared__ typename Scan64::TempStorage scan64_tmp;
    __shared__ unsigned long long s_at;
    __shared__ int s_part[4];
    const int32_t f = (seed_flags[0] ? 1 : 0) | (seed_flags[1] ? 2 : 0) | (*plan_flag ? 4 : 0);
    if (blockIdx.x == 0 && threadIdx.x == 0) *rflag = f;
    if (f) return;
    const int64_t nr = *n_dev, nch = (nr + 255) / 256;
    for (int64_t c = blockIdx.x; c < nch; c += gridDim.x) {   // block-uniform
        int part = 0;                                          // hits of the chunks before c
        for (int64_t i = threadIdx.x; i < c; i += 256) part += counts[i];
        for (int d = 32; d > 0; d >>= 1) part += __shfl_xor(part, d);
        if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = part;
        __syncthreads();
        const int base = s_part[0] + s_part[1] + s_part[2] + s_part[3];
        const int64_t k = c * 256 + threadIdx.x;
        const int32_t a = k < nr ? hb[k] : -1;
        int pos = 0, tot = 0;
        Scan(scan_tmp).ExclusiveSum(a >= 0 ? 1 : 0, pos, tot);
        const int32_t r = a >= 0 ? (cur ? cur[k] : (int32_t)k) : 0;
        const int32_t rs = a >= 0 ? hb[1 * n + k] : -1, re = a >= 0 ? hb[2 * n + k] : 0;
        // shadow space (16-byte units) of a first masked hit
        long long units = 0;
        if (a >= 0 && rs != -1 && re + 1 > rs && eoff[r] == win_off[r]) units = shadow_bytes(win_len[r]) / 16;
        long long uex = 0, utot = 0;
        Scan64(scan64_tmp).ExclusiveSum(units, uex, utot);
        if (threadIdx.x == 0) s_at = utot ? atomicAdd(bump, (unsigned long long)utot * 16ull) : 0ull;
        __syncthreads();
        if (a >= 0) {
            const int32_t j = base + pos;
            int32_t *o = list + 8 * (int64_t)j;
            o[0] = r;
            o[1] = a;
            o[2] = rs;
            o[3] = re;
            o[4] = hb[3 * n + k];
            o[5] = hb[4 * n + k];
            o[6] = (int32_t)k;
            const long long at = (long long)(s_at / 16ull) + uex;   // a unit index; < 2^31 (checked by the host's cap)
            o[7] = units ? (int32_t)min(at + 1, (long long)INT32_MAX) : 0;
            cur_next[j] = r;
            start_next[j] = a;
        }
        if (c == nch - 1 && threadIdx.x == 0) *n_next = base + tot;
        __syncthreads();                                       // s_part, scan_tmp reused
    }
}

}  // namespace

// Per-phase profile of the device-resident middle scan (pcabi_scan_profile): events around the
// phases of every queued round, which is then synchronised on its own (a diagnostic pass, never
// the timed one), and the algorithmic units the rounds processed (profile kernels, counters).
enum MidPhase { kPhScan, kPhExpand, kPhBands, kPhCands, kPhPlan, kPhDp, kPhOther, kPhases };
struct MidProf {
    bool on = false;
    std::vector<hipEvent_t> pool;
    size_t used = 0;
    std::vector<std::tuple<int, hipEvent_t, hipEvent_t>> spans;   // this round's (phase, from, to)
    double ms[kPhases] = {};
    int64_t rounds = 0, reads = 0, bases = 0, raw = 0, band_in = 0, band_edge = 0, dp_tasks = 0, dp_cells = 0;
    double round1_ms = 0.0;                                        // round 1's runs (whole rounds)
    // the pinned band classes' work: per class lane-rows issued, active lane-rows, tasks, passes
    unsigned long long band[8] = {};
    hipEvent_t get() {
        if (used == pool.size()) {
            hipEvent_t e = nullptr;
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
            pool.push_back(e);
        }
        return pool[used++];
    }
    ~MidProf() {
        for (hipEvent_t e : pool) (void)hipEventDestroy(e);
    }
    // A round's marks (all no-ops while off): begin_round() before its first launch, mark() after a
    // phase, seeds_done() after the seeding, end_round() after its last launch -- which synchronises
    // the stream, so a profiled round runs on its own.
    Scratch<unsigned long long> counters;           // the profile kernels' device counters (4 x u64)
    hipEvent_t r_begin = nullptr, r_seed[4] = {};
    struct SeedMarksOff {                           // the seed state never keeps a finished round's events
        pcabi_seed::State *s;
        ~SeedMarksOff() {
            pcabi_seed::profile_events(s, nullptr);
            (void)pcabi_seed::profile_band_stats(s, false);
        }
    };
    int begin_round(pcabi_seed::State *seed, hipStream_t st) {
        if (!on) return 0;
        used = 0;
        spans.clear();
        if (int rc = counters.ensure(8)) return rc;
        HIP_TRY(hipMemsetAsync(counters.p, 0, 32, st));
        r_begin = get();
        for (auto &e : r_seed) e = get();
        if (!r_begin || !r_seed[3]) return fail(PCABI_E_DEVICE, "profile events");
        HIP_TRY(hipEventRecord(r_begin, st));
        pcabi_seed::profile_events(seed, r_seed);
        return pcabi_seed::profile_band_stats(seed, true);
    }
    hipEvent_t mark(int phase, hipEvent_t from, hipStream_t st) {   // a span from `from` to now
        if (!on) return nullptr;
        hipEvent_t e = get();
        if (!e || hipEventRecord(e, st) != hipSuccess) return nullptr;
        if (phase >= 0 && from) spans.emplace_back(phase, from, e);
        return e;
    }
    void seeds_done(hipStream_t st) {
        if (!on) return;
        spans.emplace_back(kPhScan, r_seed[0], r_seed[1]);
        spans.emplace_back(kPhExpand, r_seed[1], r_seed[2]);
        spans.emplace_back(kPhBands, r_seed[2], r_seed[3]);
        (void)mark(kPhCands, r_seed[3], st);
    }
    int end_round(pcabi_seed::State *seed, bool first, hipStream_t st) {
        if (!on) return 0;
        const hipEvent_t r_end = mark(-1, nullptr, st);
        int64_t cnt[3] = {};
        if (int rc = pcabi_seed::profile_counts(seed, cnt, st)) return rc;   // (synchronises st)
        unsigned long long bst[8];
        if (int rc = pcabi_seed::band_stats(seed, bst)) return rc;
        for (int i = 0; i < 8; ++i) band[i] += bst[i];
        unsigned long long u[4] = {};
        HIP_TRY(hipMemcpy(u, counters.p, sizeof(u), hipMemcpyDeviceToHost));
        float tot = 0.f;
        HIP_TRY(hipEventElapsedTime(&tot, r_begin, r_end));
        double named = 0.0;
        for (const auto &sp : spans) {
            float span_ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&span_ms, std::get<1>(sp), std::get<2>(sp)));
            ms[std::get<0>(sp)] += span_ms;
            named += span_ms;
        }
        ms[kPhOther] += std::max(0.0, (double)tot - named);
        if (first) round1_ms += tot;
        rounds += 1;
        reads += (int64_t)u[0];
        bases += (int64_t)u[1];
        dp_tasks += (int64_t)u[2];
        dp_cells += (int64_t)u[3];
        raw += cnt[0];
        band_in += cnt[1];
        band_edge += cnt[2];
        return 0;
    }
};

// The queued rounds' control block, on the device and (copied once per batch of rounds) in pinned
// host memory. Kernels take pointers to its members.
constexpr int kSlots = 16;                          // round slots held on the device (wrapped past)
struct RoundCtl {
    int32_t n[kSlots + 2];                          // n[r]: round slot r's reads; n[r + 1]: its hits
    int32_t flag[kSlots + 2];                       // per round slot: what overflowed (0: the round is final)
    int64_t slots, need;                            // the first plan's task slots: taken, needed
    int32_t plan_flag, plan_flag_hi;                // the plans' overflow flag (an int32 in an 8-byte cell)
    int64_t need2;                                  // the second plan's task slots needed
    unsigned long long bump;                        // shadow-arena bytes taken
};
static_assert(offsetof(RoundCtl, flag) == 4 * (kSlots + 2) && offsetof(RoundCtl, slots) == 8 * (kSlots + 2) &&
                  offsetof(RoundCtl, need) == offsetof(RoundCtl, slots) + 8 &&
                  offsetof(RoundCtl, plan_flag) == offsetof(RoundCtl, slots) + 16 &&
                  offsetof(RoundCtl, need2) == offsetof(RoundCtl, slots) + 24 &&
                  offsetof(RoundCtl, bump) == offsetof(RoundCtl, slots) + 32 && sizeof(RoundCtl) == 184,
              "the control block's layout");
struct RoundCtlHost {
    RoundCtl c;
    int64_t seg_total;                              // round 1's segment total (the next call's mean length)
};

// Task slots of one candidate-DP plan: per slot the window, the output row, the chunk and the
// candidate, per wave its adapter, and the DP's results.
struct PlanSlots {
    Scratch<int32_t> tw, to, cand, wa, res;
    Scratch<int4> tck;
    // (queued rounds) device words the plan's layout writes: per bucket its first wave and waves, the
    // slots it took and the slots it needs
    int32_t *bk_waves = nullptr;
    int64_t *slots = nullptr, *need = nullptr;
    int reserve(int64_t slots_cap) {
        if (int rc = tw.ensure(slots_cap)) return rc;
        if (int rc = to.ensure(slots_cap)) return rc;
        if (int rc = tck.ensure(slots_cap)) return rc;
        if (int rc = cand.ensure(slots_cap)) return rc;
        if (int rc = wa.ensure(slots_cap / 64 + 1)) return rc;
        return res.ensure((int64_t)PCABI_NFIELDS * slots_cap);
    }
};

// What a queued round's launches take by value or address: a captured round graph is replayed only
// for an equal key (all int64, compared as bytes).
struct RoundKey {
    int64_t round_base, codes, win_off, win_len, n, windows, threshold_e6, ma, mi, go, ge, table, slots_cap, shadow_cap,
        shadow, target, buf_gen;
    bool operator==(const RoundKey &o) const { return std::memcmp(this, &o, sizeof(*this)) == 0; }
    bool operator!=(const RoundKey &o) const { return !(*this == o); }
};

struct pcabi_scan {
    const pcabi_adapters *adps = nullptr;
    // host-driven rounds: tiles, cross-product results and first hits, the round's reads and views
    Scratch<uint32_t> tiles;
    Scratch<int64_t> toff, soff;
    Scratch<int32_t> res, hits, idx, start, slen, mwin;
    Scratch<int16_t> s16;                           // score filter / seed bounds
    PlanSlots plan, plan2;                          // candidate DP; the candidate windows' whole-read plan
    // device planning: per adapter span, task counts, fill, wave offset, chunk index, length; per
    // candidate the best key and first task; per read the winning adapter and hit; the hit list
    Scratch<int32_t> pspan, ptasks, pfill, pcidx, plen, pcbase, phit, phb, plist;
    Scratch<int64_t> pwoff;
    Scratch<unsigned long long> pbest;
    Scratch<unsigned int> pcnt;
    Scratch<int32_t> pcert, pucert;                 // candidate windows: flagged candidates, certificate bounds
    pcabi_seed::State *seed = nullptr; // seeded round-1 bounds (pcabi_seed.hip)
    // queued rounds (middle_device_rounds): per round slot the reads, their start adapters and the
    // hit list; the control block; the plans' bucket tables (q_bk2: the second plan's waves); the
    // second plan's slot count
    Scratch<int32_t> q_cur, q_start, q_list, q_bk, q_bk2;
    Scratch<RoundCtl> q_ctl;
    Scratch<int64_t> q_slots2;
    pcabi_internal::PinBuf<int32_t> h_stage;        // pinned host staging of the queued rounds' hit lists
    pcabi_internal::PinBuf<RoundCtlHost> h_ctl;     // pinned: the control block of a batch
    int64_t spec_hits = 4096;                       // hits per round copied with the counts (grows to fit)
    double last_mean = 0.0;                         // the previous call's mean read length (round 1)
    int64_t q_slots_cap = 0;
    std::vector<int32_t> h_ucert;                   // the certificate bounds last uploaded to pucert
    std::vector<int32_t> h_up;                      // bucket tables | spans | lengths last uploaded
    const void *up_at[3] = {nullptr, nullptr, nullptr};   // ... into these buffers
    Scratch<int32_t> pcount;                        // k_round_count's per-chunk hit counts
    // (r05) input-preserving masking: the reads' effective offsets and the shadow arena of the
    // masked copies (shadow_cap: its usable bytes), a zeroed bump for the host-driven loop
    Scratch<int64_t> eoff;
    Scratch<uint8_t> shadow;
    Scratch<unsigned long long> shadow_zero;
    int64_t shadow_cap = 0;
    MidProf prof;                                   // pcabi_scan_profile
    // (r05) later rounds replayed from captured graphs, one per round slot: the key is everything
    // a round's launches take by value or address (a zeroed key equals no round's: tables count from 1)
    struct RoundGraph {
        RoundKey key{}, seen{};             // the captured graph's key; the last key queued directly
        hipGraphExec_t exec = nullptr;
    };
    RoundGraph graphs[32];
    int rounds_hint = 3;                            // rounds the last call needed (the first batch's size)
    uint64_t last_table = 0;                        // the adapter table (serial) of the last call
    ~pcabi_scan() {
        for (auto &g : graphs)
            if (g.exec) (void)hipGraphExecDestroy(g.exec);
        if (seed) pcabi_seed::destroy(seed);
    }
};

void pcabi_eng::scan_set_table(pcabi_scan *s, const pcabi_adapters *adps) { s->adps = adps; }

extern "C" {

int pcabi_scan_create(const pcabi_adapters *adps, pcabi_scan **out) {
    if (!adps || !out) return fail(PCABI_E_ARG, "bad arguments");
    pcabi_scan *s = new pcabi_scan();
    s->adps = adps;
    *out = s;
    return 0;
}

void pcabi_scan_destroy(pcabi_scan *s) {
    delete s;   // its buffers, graphs and seed state go with it
}

}  // extern "C"

namespace {

// Per bucket: whether its candidate DP runs chunked -- the core serves chunks (chunkable) and every
// adapter has a chunk lead-in D (sf::chunk_span at the adapter's filter threshold) -- and, if so,
// each entry's D. An empty bucket is not chunked.
struct BucketSpans {
    bool chunk = false;
    std::vector<int> span;
};
std::vector<BucketSpans> chunk_spans(const pcabi_adapters *adps, const pcabi::Scoring &scr, double threshold) {
    std::vector<BucketSpans> out(kNumBuckets);
    for (int b = 0; b < kNumBuckets; ++b) {
        const int nb = adps->count[b];
        if (!nb) continue;
        bool chunk = chunkable(b, bucket_packed_ok(b, adps->lens[b], scr));
        std::vector<int> sp((size_t)nb, -1);
        for (int kk = 0; chunk && kk < nb; ++kk) {
            const int L = adps->lens[b][kk];
            sp[kk] = pcabi::sf::chunk_span(L, pcabi::sf::filter_threshold(L, threshold, scr), scr);
            if (sp[kk] < 0) chunk = false;
        }
        out[b].chunk = chunk;
        if (chunk) out[b].span.swap(sp);
    }
    return out;
}

// The candidate DP of a host-laid-out plan, one launch per used bucket side by side: bucket
// used[k] runs waves [wave0[k], wave0[k + 1]) of the task slots, in chunks (chunked[k]) or on whole
// windows, over at most max_cols[k] columns. p: the launch's windows, output and scoring.
int launch_buckets(const pcabi_adapters *adps, KParams p, const PlanSlots &ps, const std::vector<int> &used,
                   const std::vector<char> &chunked, const std::vector<int32_t> &max_cols,
                   const std::vector<int64_t> &wave0, hipStream_t st) {
    const pcabi::Scoring &scr = p.sc;
    ForkJoin fj;
    if (int rc = fj.begin(st, used.size())) return rc;
    for (size_t k = 0; k < used.size(); ++k) {
        const int b = used[k];
        p.adp_pad = adps->pad[b];
        p.adp_len = adps->len[b];
        p.adp_id = adps->id[b];
        p.n_adp = adps->count[b];
        p.task_win = ps.tw.p + wave0[k] * 64;
        p.task_out = ps.to.p + wave0[k] * 64;
        p.wave_adp = ps.wa.p + wave0[k];
        p.task_chunk = ps.tck.p + wave0[k] * 64;
        p.n_waves = wave0[k + 1] - wave0[k];
        p.rt = adps->rt[b];
        p.max_cols = max_cols[k];
        int rc;
        if (chunked[k]) {
            rc = dispatch_chunk(b, p, scr.go != scr.ge, fj.at(k), bucket_pack_mode(b, adps->lens[b], scr) == 2);
        } else {
            p.task_chunk = nullptr;   // whole windows
            rc = dispatch(b, p, scr.go != scr.ge, fj.at(k), bucket_pack_mode(b, adps->lens[b], scr));
        }
        if (rc) {
            (void)fj.end();
            return rc;
        }
    }
    return fj.end();
}

// Round 1 of the middle scan through the score filter: best scores of every (read, adapter) in
// packed 16-bit lanes (k_score_filter), then the attribute DP only for the pairs that can reach
// the threshold (pairs mode), and per read the first of those (adapter order) that does.
// Fills hb (5 x n, the k_first_hit layout). Returns 1 if it ran, 0 if the filter does not apply
// to this scoring (caller falls back to the full cross product), < 0 on error.
// Later rounds (h_start != nullptr) reuse round 1's scores as bounds: masking turns read bases
// into N, which never matches an adapter base, so no alignment of the masked read scores above
// the same alignment of the unmasked one -- a pair below the threshold in round 1 stays below.
// h16 / pos1: round 1's scores (adapter-major, round-1 positions) and each read's position.
// Seeds (pcabi_seed.hip) replace the filter when they apply; they are cheap enough to run again
// in every later round on the masked reads (seeded: in, round 1 used them; out, this call did),
// where the hits just masked no longer seed their adapter. make_tiles() lays out this round's
// tiles, which only the filter reads.
// Seeded round with the candidates on the device (dcand: nc unordered keys a << 32 | window):
// plans, runs and merges the candidate DP on the device (kernels above) and fills hb (5 x n, the
// k_first_hit layout) from the windows that hit, the only data that comes back. d_start: this
// round's first adapter per window (device), nullptr in round 1. max_len: longest window.
int device_plan_hits(pcabi_scan *sc, const uint8_t *codes, const int64_t *v_off, const int32_t *v_len, int64_t n,
                     int32_t max_len, const int32_t *d_start, const int64_t *dcand, int64_t nc,
                     const pcabi::Scoring &scr, double threshold, std::vector<int32_t> &hb, hipStream_t st) {
    const pcabi_adapters *adps = sc->adps;
    const int32_t n_adp = adps->n_adp;
    hb.assign((size_t)(5 * n), 0);
    for (int64_t k = 0; k < n; ++k) hb[k] = -1;
    if (nc == 0) return 1;
    // per adapter: the chunk lead-in D of its bucket's plan (-1: whole windows), as the host plan
    std::vector<int32_t> span((size_t)n_adp, -1);
    std::vector<int32_t> bspan(kNumBuckets, 0);       // largest D of a chunked bucket
    const std::vector<BucketSpans> bsp = chunk_spans(adps, scr, threshold);
    for (int b = 0; b < kNumBuckets; ++b)
        for (size_t kk = 0; kk < bsp[b].span.size(); ++kk) {
            span[adps->ids[b][kk]] = bsp[b].span[kk];
            bspan[b] = std::max(bspan[b], bsp[b].span[kk]);
        }
    if (int rc = sc->pspan.ensure(n_adp)) return rc;
    if (int rc = sc->ptasks.ensure((int64_t)n_adp * kPlanC)) return rc;
    if (int rc = sc->pfill.ensure(n_adp)) return rc;
    if (int rc = sc->pwoff.ensure(n_adp)) return rc;
    if (int rc = sc->pcidx.ensure(n_adp)) return rc;
    HIP_TRY(hipMemcpyAsync(sc->pspan.p, span.data(), sizeof(int32_t) * n_adp, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(sc->ptasks.p, 0, sizeof(int32_t) * n_adp * kPlanC, st));
    const unsigned gc = (unsigned)((nc + 255) / 256);
    hipLaunchKernelGGL(k_plan_count, dim3(gc), dim3(256), 0, st, dcand, nc, nullptr, v_len, d_start,
                       sc->pspan.p, sc->ptasks.p, nullptr);
    HIP_TRY(hipGetLastError());
    std::vector<int32_t> tasks((size_t)n_adp * kPlanC);
    HIP_TRY(hipMemcpyAsync(tasks.data(), sc->ptasks.p, sizeof(int32_t) * tasks.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // chunk length per bucket (the buckets run side by side): the longest whose waves reach the
    // target -- a launch of few waves runs as long as its longest chunk -- else the shortest
    const int64_t target = middle_plan_waves();
    std::vector<int32_t> cidx((size_t)n_adp, 0);
    std::vector<int> bc(kNumBuckets, 0);
    for (int b = 0; b < kNumBuckets; ++b) {
        if (!bsp[b].chunk) continue;
        for (int cc = kPlanC - 1; cc > 0; --cc) {
            int64_t w = 0;
            for (int32_t a : adps->ids[b]) w += (tasks[(size_t)a * kPlanC + cc] + 63) / 64;
            if (w >= target) {
                bc[b] = cc;
                break;
            }
        }
        for (int32_t a : adps->ids[b]) cidx[a] = bc[b];
    }
    // wave layout: buckets in order, a bucket's adapters in order, one adapter per wave
    std::vector<int64_t> woff((size_t)n_adp, 0);
    std::vector<int32_t> wa;
    std::vector<int> nb_used;
    std::vector<char> nb_chunked;
    std::vector<int32_t> nb_maxcols;
    std::vector<int64_t> wave0;
    for (int b = 0; b < kNumBuckets; ++b) {
        const int nb = adps->count[b];
        if (!nb) continue;
        const size_t w_before = wa.size();
        for (int kk = 0; kk < nb; ++kk) {
            const int32_t a = adps->ids[b][kk];
            woff[a] = (int64_t)wa.size();
            const int64_t nw = (tasks[(size_t)a * kPlanC + bc[b]] + 63) / 64;
            for (int64_t w = 0; w < nw; ++w) wa.push_back(kk);
        }
        if (wa.size() == w_before) continue;
        nb_used.push_back(b);
        nb_chunked.push_back(bsp[b].chunk ? 1 : 0);
        nb_maxcols.push_back(bsp[b].chunk ? std::min<int32_t>(max_len, (kPlanMin << bc[b]) + bspan[b] + 1) : max_len);
        wave0.push_back((int64_t)w_before);
    }
    wave0.push_back((int64_t)wa.size());
    const int64_t slots = (int64_t)wa.size() * 64;
    if (g_debug) {
        std::string d;
        for (size_t k = 0; k < nb_used.size(); ++k)
            d += " rpl" + std::to_string(kBuckets[nb_used[k]].rpl) + ":" + std::to_string(wave0[k + 1] - wave0[k]) +
                 "w/c" + std::to_string(kPlanMin << bc[nb_used[k]]);
        std::fprintf(stderr, "[pcabi] middle device plan: %lld candidates, waves per bucket:%s\n", (long long)nc,
                     d.c_str());
    }
    if (slots == 0) return 1;
    PlanSlots &ps = sc->plan;
    if (int rc = ps.reserve(slots)) return rc;
    if (int rc = sc->pbest.ensure(nc)) return rc;
    if (int rc = sc->phit.ensure(n)) return rc;
    if (int rc = sc->phb.ensure(5 * n)) return rc;
    if (int rc = sc->plist.ensure(6 * n)) return rc;
    if (int rc = sc->pcnt.ensure(1)) return rc;
    HIP_TRY(hipMemcpyAsync(sc->pwoff.p, woff.data(), sizeof(int64_t) * n_adp, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(sc->pcidx.p, cidx.data(), sizeof(int32_t) * n_adp, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ps.wa.p, wa.data(), sizeof(int32_t) * wa.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)ps.tw.p, -1, (size_t)slots, st));
    HIP_TRY(hipMemsetAsync(sc->pfill.p, 0, sizeof(int32_t) * n_adp, st));
    hipLaunchKernelGGL(k_plan_place, dim3(gc), dim3(256), 0, st, dcand, nc, nullptr, v_len, d_start,
                       sc->pspan.p, sc->pcidx.p, sc->pwoff.p,
                       sc->pfill.p,
                       ps.tw.p, ps.to.p, ps.tck.p, ps.cand.p, nullptr,
                       nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    KParams p{};
    p.codes = codes;
    p.win_off = v_off;
    p.win_len = v_len;
    p.n_win = n;
    p.out = ps.res.p;
    p.out_stride = slots;
    p.sc = scr;
    if (int rc = launch_buckets(adps, p, sc->plan, nb_used, nb_chunked, nb_maxcols, wave0, st)) return rc;
    HIP_TRY(hipGetLastError());
    const unsigned gs = (unsigned)((slots + 255) / 256), gn = (unsigned)((n + 255) / 256);
    HIP_TRY(hipMemsetAsync(sc->pbest.p, 0, sizeof(unsigned long long) * nc, st));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)sc->phit.p, INT32_MAX, (size_t)n, st));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)sc->phb.p, -1, (size_t)n, st));
    HIP_TRY(hipMemsetAsync(sc->pcnt.p, 0, sizeof(unsigned int), st));
    const int32_t *tw = ps.tw.p, *tcand = ps.cand.p;
    const int4 *tck = ps.tck.p;
    const int32_t *res = ps.res.p;
    hipLaunchKernelGGL(k_merge_best, dim3(gs), dim3(256), 0, st, tw, tck, tcand, res, slots, nullptr,
                       sc->pbest.p);
    for (int pass = 0; pass < 2; ++pass)
        hipLaunchKernelGGL(k_merge_hit, dim3(gs), dim3(256), 0, st, dcand, tw, tck, tcand, res, slots, nullptr,
                           sc->pbest.p, threshold, pass, sc->phit.p,
                           sc->phb.p, n, nullptr, 0);
    hipLaunchKernelGGL(k_hits_compact, dim3(gn), dim3(256), 0, st, sc->phb.p, n,
                       sc->plist.p, sc->pcnt.p);
    HIP_TRY(hipGetLastError());
    unsigned int nh = 0;
    HIP_TRY(hipMemcpyAsync(&nh, sc->pcnt.p, sizeof(nh), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if ((int64_t)nh > n) return fail(PCABI_E_DEVICE, "middle scan: hit count overflow");
    std::vector<int32_t> list((size_t)6 * nh);
    if (nh) {
        HIP_TRY(hipMemcpyAsync(list.data(), sc->plist.p, sizeof(int32_t) * list.size(), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    for (unsigned int j = 0; j < nh; ++j) {
        const int32_t *o = list.data() + 6 * (size_t)j;
        const int64_t k = o[0];
        for (int f = 0; f < 5; ++f) hb[(size_t)f * n + k] = o[1 + f];
    }
    return 1;
}

template <typename MakeTiles>
int filtered_first_hits(pcabi_scan *sc, const uint8_t *codes, const int64_t *v_off, const int32_t *v_len,
                        const int32_t *h_len, int64_t n, const int32_t *h_start, const int32_t *d_start,
                        int32_t max_len, const int32_t *reads,
                        std::vector<int16_t> &h16, int64_t n1, const std::vector<int32_t> &pos1,
                        const pcabi::Scoring &scr, double threshold, std::vector<int32_t> &hb, bool &seeded,
                        const MakeTiles &make_tiles, hipStream_t st) {
    const pcabi_adapters *adps = sc->adps;
    const int32_t n_adp = adps->n_adp;
    std::vector<int> fb;   // buckets the score filter serves, largest first
    for (int b = 0; b < kNumBuckets; ++b)
        if (adps->count[b] && (kBuckets[b].kind == FAST || kBuckets[b].kind == WIDE) &&
            pcabi::sf::filter_ok(kBuckets[b].rpl, scr))
            fb.push_back(b);
    const int seed_mode = middle_seed_mode();
    if (fb.empty() && !seed_mode) return 0;
    std::stable_sort(fb.begin(), fb.end(), [&](int x, int y) {
        return (int64_t)adps->count[x] * kBuckets[x].rpl > (int64_t)adps->count[y] * kBuckets[y].rpl;
    });
    std::vector<char> filtered((size_t)n_adp, 0);
    std::vector<int32_t> lenof((size_t)n_adp, 0);
    for (int b = 0; b < kNumBuckets; ++b)
        for (size_t k = 0; k < adps->ids[b].size(); ++k) lenof[adps->ids[b][k]] = adps->lens[b][k];
    for (int b : fb)
        for (int32_t id : adps->ids[b]) filtered[id] = 1;
    // 1. bounds of every (adapter, read): seeds (any round, when round 1 used them) or the score
    //    filter (round 1 only), buckets side by side
    bool local = !h_start;   // h16 holds this round's bounds (a * n + k), not round 1's
    std::vector<int64_t> seed_cands;   // seeded: the filtered candidates, sorted (a << 32 | k)
    if (!h_start || seeded) {
        if (int rc = sc->s16.ensure((size_t)n * n_adp)) return rc;
        int got = 0;
        const int mode = seed_mode;
        if (mode && (!h_start || seeded)) {
            if (!sc->seed) sc->seed = pcabi_seed::create();
            // seeds cover every adapter the plan accepts, long (generic-core) ones included
            // (striped adapters stay outside: every read is their candidate)
            std::vector<int> rows((size_t)n_adp, 0);
            for (int b = 0; b < kNumBuckets; ++b)
                if (kBuckets[b].kind != STRIPED)
                    for (int32_t id : adps->ids[b]) rows[id] = kBuckets[b].rpl;
            // every adapter seeded (no striped one): the candidates stay on the device
            const bool devplan = middle_devplan_on() && adps->count[kStripedBucket] == 0;
            const int64_t *dcand = nullptr;
            int64_t ndc = 0;
            got = pcabi_seed::bounds(sc->seed, adps, adps->hcodes.data(), adps->hoff.data(), adps->hlen.data(),
                                     n_adp, rows, codes, v_off, v_len, n, scr, threshold, h_start ? 2 : mode,
                                     sc->s16.p, devplan ? nullptr : &seed_cands,
                                     devplan ? &dcand : nullptr, &ndc, st);
            if (got < 0) return got;
            if (got > 0 && devplan) {
                seeded = true;
                return device_plan_hits(sc, codes, v_off, v_len, n, max_len, h_start ? d_start : nullptr, dcand, ndc,
                                        scr, threshold, hb, st);
            }
        }
        if (h_start && !got) return fail(PCABI_E_DEVICE, "middle scan: seeds stopped applying after round 1");
        seeded = got > 0;
        if (seeded) {
            for (int b = 0; b < kNumBuckets; ++b)
                if (kBuckets[b].kind != STRIPED)
                    for (int32_t id : adps->ids[b]) filtered[id] = 1;
        } else if (fb.empty()) {
            return 0;
        } else {
            if (int rc = make_tiles()) return rc;
            ForkJoin fj;
            if (int rc = fj.begin(st, fb.size())) return rc;
            for (size_t k = 0; k < fb.size(); ++k) {
                const int b = fb[k];
                FParams f{};
                f.tiles = sc->tiles.p;
                f.tile_off = sc->toff.p;
                f.win_len = v_len;
                f.n_win = n;
                f.adp_pad = adps->pad[b];
                f.adp_len = adps->len[b];
                f.adp_id = adps->id[b];
                f.n_adp = adps->count[b];
                f.s16 = sc->s16.p;
                f.sc = scr;
                dispatch_filter(kBuckets[b].rpl, f, scr.go != scr.ge, fj.at(k));
            }
            if (int rc = fj.end()) return rc;
            HIP_TRY(hipGetLastError());
            h16.resize((size_t)n * n_adp);
            HIP_TRY(hipMemcpyAsync(h16.data(), sc->s16.p, sizeof(int16_t) * h16.size(), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        local = true;
    }
    // 2. candidates (adapter-major): pairs that can reach the threshold, from each read's start
    //    adapter on
    std::vector<int32_t> cand_w, cand_a;
    size_t sc_i = 0;
    for (int32_t a = 0; a < n_adp; ++a) {
        if (seeded && filtered[a]) {                   // from the device's list
            for (; sc_i < seed_cands.size() && (int32_t)(seed_cands[sc_i] >> 32) == a; ++sc_i) {
                const int32_t k = (int32_t)(seed_cands[sc_i] & 0xFFFFFFFF);
                if (h_len[k] <= 0 || (h_start && a < h_start[k])) continue;
                cand_w.push_back(k);
                cand_a.push_back(a);
            }
            continue;
        }
        const int T = pcabi::sf::filter_threshold(lenof[a], threshold, scr);
        const int16_t *row = filtered[a] ? h16.data() + (size_t)a * (local ? n : n1) : nullptr;
        for (int64_t k = 0; k < n; ++k) {
            if (h_len[k] <= 0 || (h_start && a < h_start[k])) continue;
            if (!row || row[local ? k : pos1[reads[k]]] >= T) { cand_w.push_back((int32_t)k); cand_a.push_back(a); }
        }
    }
    const int64_t n_task = (int64_t)cand_w.size();
    hb.assign((size_t)(5 * n), 0);
    for (int64_t k = 0; k < n; ++k) { hb[k] = -1; hb[n + k] = -1; }
    if (g_debug) {
        std::vector<int64_t> per((size_t)n_adp, 0);
        for (int32_t a : cand_a) ++per[a];
        std::string s;
        for (int32_t a = 0; a < n_adp; ++a) s += std::to_string(per[a]) + (a + 1 < n_adp ? "," : "");
        std::fprintf(stderr, "[pcabi] middle round %s: %lld reads, %lld candidate pairs; per adapter: %s\n",
                     h_start ? "2+" : "1", (long long)n, (long long)n_task, s.c_str());
    }
    if (n_task == 0) return 1;
    // attribute DP of the candidates: one task list per bucket (waves of 64 lanes, one adapter
    // per wave), all buckets in one upload, launched side by side. Packed-core buckets split
    // long reads into chunks (sf::chunk_plan), so no lane walks a whole long read alone: a task
    // is one chunk, and a candidate's chunks are merged below.
    std::vector<int64_t> first((size_t)n_adp + 1, 0);
    for (int64_t t = 0; t < n_task; ++t) ++first[cand_a[t] + 1];
    for (int32_t a = 0; a < n_adp; ++a) first[a + 1] += first[a];
    std::vector<int32_t> tw, to, wa;
    std::vector<int4> tck;
    std::vector<int64_t> task_cand;                 // task -> candidate
    std::vector<int32_t> task_start;                // task -> read offset of its chunk
    std::vector<int> nb_used;
    std::vector<char> nb_chunked;
    std::vector<int32_t> nb_maxcols;                // longest window / chunk per bucket (striped scratch)
    std::vector<int64_t> wave0;
    // chunk length: the shortest (power of two >= kChunkColsMin) whose task count stays within
    // kChunkTasks (the count over all candidates, chunked or not -- a bound)
    int chunk_cols = kChunkCols;
    for (int c = kChunkColsMin; c < kChunkCols; c *= 2) {
        int64_t tasks = 0;
        for (int64_t t = 0; t < n_task && tasks <= kChunkTasks; ++t) tasks += (h_len[cand_w[t]] + c - 1) / c;
        if (tasks <= kChunkTasks) {
            chunk_cols = c;
            break;
        }
    }
    const std::vector<BucketSpans> bsp = chunk_spans(adps, scr, threshold);
    for (int b = 0; b < kNumBuckets; ++b) {
        const int nb = adps->count[b];
        if (!nb) continue;
        const size_t w_before = wa.size();
        const bool chunk = bsp[b].chunk;
        const std::vector<int> &span = bsp[b].span;
        int32_t maxcols = 0;
        for (int kk = 0; kk < nb; ++kk) {
            const int32_t a = adps->ids[b][kk];
            int lane = 64;
            auto add = [&](int64_t t, int32_t w, int4 ck) {
                maxcols = std::max(maxcols, chunk ? ck.y : h_len[w]);
                if (lane == 64) {
                    wa.push_back(kk);
                    lane = 0;
                }
                tw.push_back(w);
                to.push_back((int32_t)task_cand.size());
                tck.push_back(ck);
                task_cand.push_back(t);
                task_start.push_back(ck.x);
                ++lane;
            };
            for (int64_t t = first[a]; t < first[a + 1]; ++t) {
                const int32_t k = cand_w[t];
                if (chunk)
                    pcabi::sf::chunk_plan(h_len[k], span[kk], chunk_cols, [&](const pcabi::sf::Chunk &c) {
                        add(t, k, make_int4(c.start, c.len, c.own_lo, c.own_hi));
                    });
                else
                    add(t, k, make_int4(0, 0, 0, 0));
            }
            for (; lane < 64; ++lane) {                // idle lanes of the adapter's last wave
                tw.push_back(-1);
                to.push_back(0);
                tck.push_back(make_int4(0, 0, 0, 0));
            }
        }
        if (wa.size() == w_before) continue;
        nb_used.push_back(b);
        nb_chunked.push_back(chunk ? 1 : 0);
        nb_maxcols.push_back(maxcols);
        wave0.push_back((int64_t)w_before);
    }
    wave0.push_back((int64_t)wa.size());
    const int64_t n_run = (int64_t)task_cand.size();
    if (g_debug) {
        std::string s;
        for (size_t k = 0; k < nb_used.size(); ++k)
            s += " rpl" + std::to_string(kBuckets[nb_used[k]].rpl) + ":" + std::to_string(wave0[k + 1] - wave0[k]) +
                 "w/" + std::to_string(nb_maxcols[k]) + "c";
        std::fprintf(stderr, "[pcabi] middle tasks %lld (chunks of %d), waves per bucket:%s\n", (long long)n_run,
                     chunk_cols, s.c_str());
    }
    PlanSlots &ps = sc->plan;   // (host-laid-out: every list at its own size)
    if (int rc = ps.res.ensure((int64_t)PCABI_NFIELDS * n_run)) return rc;
    if (int rc = ps.tw.ensure((int64_t)tw.size())) return rc;
    if (int rc = ps.to.ensure((int64_t)to.size())) return rc;
    if (int rc = ps.wa.ensure((int64_t)wa.size())) return rc;
    if (int rc = ps.tck.ensure((int64_t)tck.size())) return rc;
    HIP_TRY(hipMemcpyAsync(ps.tw.p, tw.data(), sizeof(int32_t) * tw.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ps.to.p, to.data(), sizeof(int32_t) * to.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ps.wa.p, wa.data(), sizeof(int32_t) * wa.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ps.tck.p, tck.data(), sizeof(int4) * tck.size(), hipMemcpyHostToDevice, st));
    KParams p{};
    p.codes = codes;
    p.win_off = v_off;
    p.win_len = v_len;
    p.n_win = n;
    p.out = ps.res.p;
    p.out_stride = n_run;
    p.sc = scr;
    if (int rc = launch_buckets(adps, p, sc->plan, nb_used, nb_chunked, nb_maxcols, wave0, st)) return rc;
    HIP_TRY(hipGetLastError());
    std::vector<int32_t> res((size_t)PCABI_NFIELDS * n_run);
    HIP_TRY(hipMemcpyAsync(res.data(), ps.res.p, sizeof(int32_t) * res.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // merge each candidate's chunks: the first (read order) with the largest score; read offsets
    // back to the whole read
    std::vector<int64_t> best((size_t)n_task, -1);
    for (int64_t u = 0; u < n_run; ++u) {
        const int64_t t = task_cand[u];
        if (best[t] < 0 || res[4 * n_run + u] > res[4 * n_run + best[t]]) best[t] = u;
    }
    // 3. per read, the first candidate (adapter order) over the threshold
    for (int64_t t = 0; t < n_task; ++t) {
        const int64_t k = cand_w[t];
        const int32_t a = cand_a[t];
        if (hb[k] >= 0 && hb[k] <= a) continue;
        const int64_t u = best[t];
        const int rs = res[0 * n_run + u];
        const int m = res[5 * n_run + u], l2 = res[7 * n_run + u];
        const double full = rs == -1 ? 0.0 : pcabi::pid6(m, l2);
        if (full < threshold) continue;
        hb[k] = a;
        hb[n + k] = rs + task_start[u];
        hb[2 * n + k] = res[1 * n_run + u] + task_start[u];
        hb[3 * n + k] = m;
        hb[4 * n + k] = l2;
    }
    return 1;
}


// PCABI_MIDDLE_DEVROUNDS=0: the seeded scan keeps the host-driven round loop (A/B runs).
bool middle_devrounds_on() {
    const char *e = std::getenv("PCABI_MIDDLE_DEVROUNDS");
    return !(e && e[0] == '0');
}

// ---- the shadow arena of the input-preserving masking (k_round_hits, k_mask_list) ----------------
// eoff values are offsets from the caller's `codes`, so a copy in the arena is addressed as
// codes + eoff like any window (a flat device address space).
int64_t shadow_rel(const pcabi_scan *sc, const uint8_t *codes) {
    return (int64_t)((intptr_t)sc->shadow.p - (intptr_t)codes);
}
constexpr int64_t kShadowMax = (int64_t)INT32_MAX * 16;   // k_round_hits' 16-byte unit index is an int32
constexpr int64_t kShadowLead = 256;                      // arena bytes before the first copy

// The arena's first size: 1/8 of the batch's bases (about 3x the ~4.5 % of reads a round 1 hits at
// the default threshold), at least 16 MB; tests set it with the 4th PCABI_MIDDLE_INIT_CAPS value.
int shadow_reserve(pcabi_scan *sc, const int32_t *h_win_len, int64_t n) {
    if (sc->shadow_cap > 0) return 0;
    int64_t want = 16ll << 20;
    if (h_win_len) {
        int64_t bases = 0;
        for (int64_t k = 0; k < n; ++k) bases += std::max(h_win_len[k], 0);
        want = std::max(want, bases / 8);
    }
    const int64_t arena = pcabi_internal::middle_init_caps().arena;
    if (arena > 0) want = arena;
    want = std::min(std::max(want, kShadowLead), kShadowMax);
    if (int rc = sc->shadow.ensure(want)) return rc;
    sc->shadow_cap = want;
    return 0;
}

// A larger arena (the round that ran out flagged itself and is queued again): the copies move with
// it (eoff rebased), and the bump goes on from the old end. taken: the bytes the rounds asked for.
int shadow_grow(pcabi_scan *sc, const uint8_t *codes, const int64_t *win_off, int64_t *eoff, int64_t n, int64_t taken,
                unsigned long long *d_bump, hipStream_t st) {
    (void)codes;
    const int64_t old_cap = sc->shadow_cap;
    const int64_t want = std::min<int64_t>(std::max<int64_t>(2 * std::max(old_cap, taken), 1ll << 20), kShadowMax);
    if (want <= old_cap || want < taken - old_cap) return fail(PCABI_E_NOMEM, "middle scan: shadow arena past its limit");
    void *np = nullptr;
    if (hipMalloc(&np, (size_t)want) != hipSuccess) return fail(PCABI_E_NOMEM, "hipMalloc failed (shadow arena)");
    pcabi_poison(np, (size_t)want);
    if (sc->shadow.p && old_cap > 0) HIP_TRY(hipMemcpyAsync(np, sc->shadow.p, (size_t)old_cap, hipMemcpyDeviceToDevice, st));
    const int64_t delta = (int64_t)((intptr_t)np - (intptr_t)sc->shadow.p);
    if (sc->shadow.p && n > 0)
        hipLaunchKernelGGL(k_shadow_rebase, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 2048)), dim3(256), 0, st,
                           win_off, eoff, n, delta);
    HIP_TRY(hipGetLastError());
    const unsigned long long at = (unsigned long long)old_cap;
    if (d_bump) HIP_TRY(hipMemcpyAsync(d_bump, &at, sizeof(at), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    // (not through ensure(): the new arena exists before the old one goes, because the copies move)
    if (sc->shadow.p) HIP_TRY(hipFree(sc->shadow.p));
    sc->shadow.p = (uint8_t *)np;
    sc->shadow.cap = want;
    sc->shadow_cap = want;
    return 0;
}

// Overflow recovery of the queued rounds, counted for the tests (pcabi_middle_requeues).
std::atomic<int64_t> g_requeues{0};
std::atomic<int32_t> g_requeue_flags{0};

// Tests: PCABI_MIDDLE_FAULT="round:bits[,round:bits...]" makes the first run of that round (0 =
// round 1 of a call) overflow for real -- its raw-hit slabs (1), inside-task regions (2) and / or
// candidate-DP task slots (4) shrunk to nothing -- so its kernels flag it, nothing of it is kept and
// it is queued again (without growing: the real capacities were enough).
std::vector<std::pair<int64_t, int>> middle_faults() {
    std::vector<std::pair<int64_t, int>> f;
    const char *e = std::getenv("PCABI_MIDDLE_FAULT");
    while (e && *e) {
        long long r = 0;
        int bits = 0, used = 0;
        if (std::sscanf(e, "%lld:%d%n", &r, &bits, &used) < 2 || used <= 0) break;
        f.emplace_back((int64_t)r, bits & 15);
        e += used;
        if (*e == ',') ++e;
    }
    return f;
}

// ---- the queued device rounds (middle_device_rounds, below) ---------------------------------------
constexpr int kBatch = 3;                       // rounds queued per host check (later batches)
constexpr unsigned kGrid = 2048;                // blocks of the device-counted launches

// What the rounds of one call share.
struct RoundsCall {
    pcabi_scan *sc;
    const pcabi_adapters *adps;
    const uint8_t *codes;
    const int64_t *win_off;
    const int32_t *win_len;
    int64_t n;
    pcabi::Scoring scr;
    double threshold;
    hipStream_t st;
    // the table's plan: the buckets in use, each adapter's chunk span, the bucket tables (host, device)
    std::vector<int> used, pack_mode;           // (pack_mode: bucket_pack_mode of used[k])
    std::vector<int32_t> span, bk_first, bk_adp, bk_local;
    int n_bk = 0;
    int32_t *d_bk_first = nullptr, *d_bk_adp = nullptr, *d_bk_local = nullptr;
    RoundCtl *ctl = nullptr;                    // the device control block
    int64_t *eoff = nullptr;                    // the reads' effective offsets
    bool windows = false;                       // candidate windows (middle_windows_on)
    int dp_serial_from = 0;                     // rounds from here on launch their DP buckets serially
    int64_t target = 0;                         // waves a plan aims at (middle_plan_waves)
    unsigned gn = 0;                            // blocks of the per-read launches
    bool graphs_on = false;
    // tests: the injected overflows, which of them fired, and per slot what its last queueing injected
    std::vector<std::pair<int64_t, int>> faults;
    std::vector<char> fired;
    int injected[kSlots + 1] = {};
    int64_t round_base = 0;                     // global round number of slot 0
    int64_t spec = 0;                           // hits per round staged with the counts
    std::vector<int32_t> out;                   // (8 ints per hit) of the finished rounds
    std::vector<int64_t> out_round;             // ... and each hit's round
    int64_t most_hits = 0;
    int32_t *cur_of(int slot) const { return sc->q_cur.p + (int64_t)slot * n; }
    int32_t *start_of(int slot) const { return sc->q_start.p + (int64_t)slot * n; }
    int32_t *list_of(int slot) const { return sc->q_list.p + (int64_t)slot * 8 * n; }
    bool first_round(int r) const { return r == 0 && round_base == 0; }   // round 1: the windows themselves
};

// Pointers and flags of one round being queued.
struct RoundCtx {
    int r = 0;                                  // its slot
    int fault = 0;                              // injected overflows (tests)
    bool first = false;
    int64_t slots_cap = 0;                      // task slots per plan
    const int32_t *nr = nullptr, *start = nullptr, *cur = nullptr;   // its read count, start adapters, reads
    const int64_t *v_off = nullptr;             // its views
    const int32_t *v_len = nullptr;
    // the seeds' results (pcabi_seed::bounds_dev)
    const int64_t *dcand = nullptr;
    const unsigned long long *dcount = nullptr;
    const int32_t *sflags = nullptr;
    const int4 *vlist = nullptr;
    const int32_t *vcount = nullptr, *pmap = nullptr;
    int64_t vcap = 0;
    int64_t ncap = 0;                           // candidates at most: reads x adapters
};

// Whether the queued rounds serve this table and scoring: every bucket chunked (the device plan's
// launches are k_align_chunk) and a seed plan that applies. 1, 0 (declined) or an error.
int rounds_plan(RoundsCall &c) {
    const pcabi_adapters *adps = c.adps;
    const int32_t n_adp = adps->n_adp;
    if (!middle_devrounds_on() || !middle_devplan_on() || adps->count[kStripedBucket] || c.n >= (1ll << 31) ||
        (int64_t)c.n * n_adp >= (1ll << 40))
        return 0;
    const std::vector<BucketSpans> bsp = chunk_spans(adps, c.scr, c.threshold);
    c.span.assign((size_t)n_adp, -1);
    c.bk_first.assign(1, 0);
    for (int b = 0; b < kNumBuckets; ++b) {
        const int nb = adps->count[b];
        if (!nb) continue;
        if (!bsp[b].chunk) return 0;
        for (int kk = 0; kk < nb; ++kk) {
            c.span[adps->ids[b][kk]] = bsp[b].span[kk];
            c.bk_adp.push_back(adps->ids[b][kk]);
            c.bk_local.push_back(kk);
        }
        c.used.push_back(b);
        c.pack_mode.push_back(bucket_pack_mode(b, adps->lens[b], c.scr));
        c.bk_first.push_back((int32_t)c.bk_adp.size());
    }
    c.n_bk = (int)c.used.size();
    std::vector<int> rows((size_t)n_adp, 0);
    for (int b = 0; b < kNumBuckets; ++b)
        for (int32_t id : adps->ids[b]) rows[id] = kBuckets[b].rpl;
    if (!c.sc->seed) c.sc->seed = pcabi_seed::create();
    hmark("setup");
    const int rc = pcabi_seed::plan_ready(c.sc->seed, adps->hcodes.data(), adps->hoff.data(), adps->hlen.data(), n_adp,
                                          rows, c.scr, c.threshold, middle_seed_mode(), c.st);
    hmark("plan");
    return rc < 0 ? rc : (rc ? 1 : 0);
}

// The call's device buffers, the bucket tables' upload and the choice of candidate windows.
int rounds_buffers(RoundsCall &c, const int32_t *h_win_len) {
    pcabi_scan *sc = c.sc;
    const pcabi_adapters *adps = c.adps;
    const int64_t n = c.n, n_adp = adps->n_adp;
    const hipStream_t st = c.st;
    if (int rc = sc->q_cur.ensure(n * (kSlots + 1))) return rc;
    if (int rc = sc->q_start.ensure(n * (kSlots + 1))) return rc;
    if (int rc = sc->q_list.ensure(8 * n * kSlots)) return rc;
    if (int rc = sc->q_ctl.ensure(1)) return rc;
    if (int rc = sc->eoff.ensure(n)) return rc;
    if (int rc = shadow_reserve(sc, h_win_len, n)) return rc;
    if (int rc = sc->soff.ensure(n)) return rc;
    if (int rc = sc->slen.ensure(n)) return rc;
    if (int rc = sc->pspan.ensure(n_adp)) return rc;
    if (int rc = sc->plen.ensure(n_adp)) return rc;
    if (int rc = sc->ptasks.ensure(n_adp * kPlanC)) return rc;
    if (int rc = sc->pfill.ensure(n_adp)) return rc;
    if (int rc = sc->pwoff.ensure(n_adp)) return rc;
    if (int rc = sc->pcidx.ensure(n_adp)) return rc;
    if (int rc = sc->phit.ensure(n)) return rc;
    if (int rc = sc->phb.ensure(5 * n)) return rc;
    if (int rc = sc->pbest.ensure(n * n_adp)) return rc;
    if (int rc = sc->pcbase.ensure(n * n_adp)) return rc;
    if (int rc = sc->pcount.ensure(n / 256 + 2)) return rc;
    const int64_t n_first = (int64_t)c.bk_first.size(), n_in = (int64_t)c.bk_adp.size();
    if (int rc = sc->q_bk.ensure(n_first + 2 * n_in + 2 * c.n_bk + 16)) return rc;
    if (int rc = sc->q_slots2.ensure(8)) return rc;
    if (int rc = sc->q_bk2.ensure(2 * c.n_bk + 16)) return rc;
    if (int rc = sc->pcert.ensure(n * n_adp)) return rc;
    if (sc->pucert.cap < n_adp) sc->h_ucert.clear();   // (re)allocated below
    if (int rc = sc->pucert.ensure(n_adp)) return rc;
    c.ctl = sc->q_ctl.p;
    c.eoff = sc->eoff.p;
    c.d_bk_first = sc->q_bk.p;
    c.d_bk_adp = c.d_bk_first + n_first;
    c.d_bk_local = c.d_bk_adp + n_in;
    sc->plan.bk_waves = c.d_bk_local + n_in;
    sc->plan.slots = &c.ctl->slots;
    sc->plan.need = &c.ctl->need;
    sc->plan2.bk_waves = sc->q_bk2.p;
    sc->plan2.slots = sc->q_slots2.p;
    sc->plan2.need = &c.ctl->need2;
    std::vector<int32_t> bk_host(c.bk_first);
    bk_host.insert(bk_host.end(), c.bk_adp.begin(), c.bk_adp.end());
    bk_host.insert(bk_host.end(), c.bk_local.begin(), c.bk_local.end());
    {   // the bucket tables, spans and lengths depend on the table and scoring only: up once per
        // change (three pageable copies cost ~20 us of every call otherwise)
        std::vector<int32_t> key(bk_host);
        key.insert(key.end(), c.span.begin(), c.span.end());
        key.insert(key.end(), adps->hlen.begin(), adps->hlen.end());
        const void *where[3] = {sc->q_bk.p, sc->pspan.p, sc->plen.p};
        if (key != sc->h_up || std::memcmp(where, sc->up_at, sizeof(where)) != 0) {
            HIP_TRY(hipMemcpyAsync(sc->q_bk.p, bk_host.data(), 4 * bk_host.size(), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(sc->pspan.p, c.span.data(), 4 * (size_t)n_adp, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(sc->plen.p, adps->hlen.data(), 4 * (size_t)n_adp, hipMemcpyHostToDevice, st));
            sc->h_up.swap(key);
            std::memcpy(sc->up_at, where, sizeof(where));
        }
    }
    double mean_len = sc->last_mean;
    if (h_win_len) {
        double tot = 0.0;
        for (int64_t k = 0; k < n; ++k) tot += h_win_len[k];
        mean_len = n ? tot / (double)n : 0.0;
    }
    hmark("bufs");
    c.windows = middle_windows_on(mean_len);
    if (c.windows) {
        std::vector<int32_t> U;
        pcabi_seed::cert_bounds(sc->seed, U);
        if (U != sc->h_ucert) {                       // a new plan: its bounds up once (pageable: staged)
            HIP_TRY(hipMemcpyAsync(sc->pucert.p, U.data(), 4 * (size_t)n_adp, hipMemcpyHostToDevice, st));
            sc->h_ucert = U;
        }
    }
    return 0;
}

// The state every call starts from: the plans' counts zeroed, the reads at the caller's offsets, an
// empty arena; the first slot capacity, the tests' faults, the serial thresholds, the graph switch
// and the pinned buffers.
int rounds_start(RoundsCall &c) {
    pcabi_scan *sc = c.sc;
    const hipStream_t st = c.st;
    // the plans' slot counts and needs start at 0 (the block is uninitialised device memory: a round
    // that overflowed read a need its plan never wrote -- r05aa, a 10^18-byte growth request)
    HIP_TRY(hipMemsetAsync(&c.ctl->slots, 0, offsetof(RoundCtl, bump) - offsetof(RoundCtl, slots), st));
    // the reads' effective offsets start as the caller's; no shadow taken yet
    HIP_TRY(hipMemcpyAsync(c.eoff, c.win_off, sizeof(int64_t) * c.n, hipMemcpyDeviceToDevice, st));
    // the bump starts past the arena's lead-in (kShadowLead bytes no copy uses: band loads that
    // reach a little before a read's start stay inside the allocation)
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)&c.ctl->bump, (int)kShadowLead, 1, st));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)((int32_t *)&c.ctl->bump + 1), 0, 1, st));
    if (sc->q_slots_cap == 0) {
        sc->q_slots_cap = std::max<int64_t>(1 << 20, 4 * c.n);
        const int64_t slots = pcabi_internal::middle_init_caps().slots;   // tests
        if (slots > 0) sc->q_slots_cap = slots;
    }
    c.faults = middle_faults();
    c.fired.assign(c.faults.size(), 0);
    // the candidate-DP buckets' own threshold: in the window rounds (long reads) round 1's buckets
    // run serial too (r05aw in-process A/B, 20 kb: 2.512 -> 2.491 ms; 8 kb whole-read rounds keep
    // them side by side: 1.933 against 1.999 serial)
    c.dp_serial_from = c.windows ? 0 : kMiddleSerialFrom;
    c.target = middle_plan_waves();
    c.gn = (unsigned)std::min<int64_t>((c.n + 255) / 256, kGrid);
    // A round other than a call's first one is ~40 small launches and fork / join events whose
    // arguments depend only on the slot, the call's inputs and the scratch addresses: it is captured
    // once into a graph and replayed (r05: one host call instead of ~40 launches and ~10 event
    // operations, and the graph's ~1.6 us per kernel instead of ~2.7 back to back, tools/
    // launch_bench.hip; r05au: serial rounds too, the fork setting in the key). Not for rounds that
    // inject faults (tests), profile, debug or the legacy stream, and only rounds that run serial
    // (a capture would record another caller's launches on the shared side streams).
    c.graphs_on = st != nullptr && c.faults.empty() && !g_debug && !sc->prof.on && sc->last_table == c.adps->serial;
    // (a table new to this scan -- e.g. the host API's per-call tables -- runs its rounds directly:
    // a capture pays only for a table the next call uses again)
    sc->last_table = c.adps->serial;
    if (int rc = sc->h_ctl.reserve(1, 1)) return rc;
    sc->h_ctl.p->seg_total = -1;
    // every queued round's first spec entries come back with the counts (one synchronisation per
    // batch of rounds instead of two); a round with more hits fetches the rest after
    c.spec = std::min<int64_t>(sc->spec_hits, c.n);
    const int64_t want = 8 * c.spec * kBatch;
    return sc->h_stage.reserve(want, want);
}

// The round's injected overflows (tests), each fired once until a requeue re-arms it.
int take_faults(RoundsCall &c, int r) {
    int fault = 0;
    for (size_t k = 0; k < c.faults.size(); ++k)
        if (!c.fired[k] && c.faults[k].first == c.round_base + r) {
            fault |= c.faults[k].second;
            c.fired[k] = 1;
        }
    c.injected[r] = fault;
    return fault;
}

// The round's views (round 1: the windows themselves) and its seeds.
int round_seeds(RoundsCall &c, RoundCtx &x) {
    pcabi_scan *sc = c.sc;
    const int32_t n_adp = c.adps->n_adp;
    hipLaunchKernelGGL(k_round_views, dim3(x.first ? 1 : c.gn), dim3(256), 0, c.st, c.eoff, c.win_len, x.cur, x.nr,
                       sc->soff.p, sc->slen.p, c.ctl->n + x.r + 1, &c.ctl->plan_flag, sc->ptasks.p, sc->pfill.p, n_adp,
                       x.first ? c.ctl->n : nullptr, (int32_t)c.n);
    x.v_off = x.first ? c.eoff : sc->soff.p;
    x.v_len = x.first ? c.win_len : sc->slen.p;
    if (int rc = pcabi_seed::bounds_dev(sc->seed, c.codes, x.v_off, x.v_len, c.n, x.nr, n_adp, c.scr, &x.dcand, &x.dcount,
                                        &x.sflags, c.windows ? &x.vlist : nullptr, &x.vcount, &x.pmap, &x.vcap, c.st))
        return rc;
    if (sc->prof.on) {
        sc->prof.seeds_done(c.st);
        hipLaunchKernelGGL(k_prof_round, dim3(64), dim3(256), 0, c.st, x.v_len, x.nr, sc->prof.counters.p);
    }
    return 0;
}

// A plan's counts, layout and task slots on the device. win: the verified seeds' windows, else the
// candidates' whole-read chunks (cmask != nullptr: only the candidates it flags).
int plan_slots(RoundsCall &c, const RoundCtx &x, const PlanSlots &pl, bool win, const int32_t *cmask) {
    pcabi_scan *sc = c.sc;
    const hipStream_t st = c.st;
    if (win)
        hipLaunchKernelGGL(k_wplan_count, dim3(kGrid), dim3(256), 0, st, x.vlist, x.vcount, x.vcap, x.v_len, x.start,
                           sc->ptasks.p);
    else
        hipLaunchKernelGGL(k_plan_count, dim3(kGrid), dim3(256), 0, st, x.dcand, x.ncap, x.dcount, x.v_len, x.start,
                           sc->pspan.p, sc->ptasks.p, cmask);
    // the flagged candidates' whole reads (cmask): half the wave target, so their chunks are
    // 64 columns rather than 32 at a few hundred reads -- the lead-in (the adapter's span) is
    // recomputed per chunk (r05q: 20 kb 3.21-3.27 -> 3.13-3.22 ms; 8 kb keeps 4096)
    hipLaunchKernelGGL(k_plan_layout, dim3(1), dim3(256), 0, st, sc->ptasks.p, c.n_bk, c.d_bk_first, c.d_bk_adp,
                       c.d_bk_local, cmask ? std::max<int64_t>(1, c.target / 2) : c.target, x.slots_cap, sc->pcidx.p,
                       sc->pwoff.p, pl.wa.p, pl.tw.p, pl.bk_waves, pl.slots, &c.ctl->plan_flag, pl.need);
    if (win) {
        hipLaunchKernelGGL(k_wplan_place, dim3(kGrid), dim3(256), 0, st, x.vlist, x.vcount, x.vcap, x.v_off, x.v_len,
                           x.start, sc->plen.p, sc->pspan.p, x.pmap, c.n, sc->pwoff.p, sc->pfill.p, pl.tw.p, pl.to.p,
                           pl.tck.p, pl.cand.p, pl.slots);
    } else {
        hipLaunchKernelGGL(k_plan_place, dim3(kGrid), dim3(256), 0, st, x.dcand, x.ncap, x.dcount, x.v_len, x.start,
                           sc->pspan.p, sc->pcidx.p, sc->pwoff.p, sc->pfill.p, pl.tw.p, pl.to.p, pl.tck.p, pl.cand.p,
                           pl.slots, sc->pcbase.p, cmask);
        hipLaunchKernelGGL(k_plan_fill, dim3(kGrid), dim3(256), 0, st, x.dcand, x.ncap, x.dcount, x.v_len, sc->pspan.p,
                           sc->pcidx.p, sc->pcbase.p, pl.tw.p, pl.to.p, pl.tck.p, pl.cand.p, pl.slots);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// A plan's candidate DP: the launches stride over the device's wave counts. The run-tagged buckets
// (<= 28 rows) go as one grouped launch (k_align_chunk_group), longest rows first; the other buckets
// (and a lone run-tagged one) launch on their own. (Not launch_buckets: these launches read their
// waves from the device, share one region with the grouped launch, pick their lane split per bucket
// and fork only before the serial threshold.)
int plan_dp(RoundsCall &c, const RoundCtx &x, const PlanSlots &pl) {
    const pcabi_adapters *adps = c.adps;
    const pcabi::Scoring &scr = c.scr;
    KParams p{};
    p.codes = c.codes;
    p.win_off = x.v_off;
    p.win_len = x.v_len;
    p.n_win = c.n;
    p.out = pl.res.p;
    p.out_stride = x.slots_cap;
    p.sc = scr;
    p.task_win = pl.tw.p;
    p.task_out = pl.to.p;
    p.wave_adp = pl.wa.p;
    p.task_chunk = pl.tck.p;
    p.n_waves = kGrid;
    // two lanes per chunk task in the candidate-window rounds (long reads: the windows and the
    // certified-out candidates' whole reads), one lane in the whole-read rounds of shorter reads
    // (r05y / r05z in-process A/B: two lanes everywhere made the 20 kb scan 0.13 ms faster --
    // most of it the whole reads' 32-column chunks -- and the 8 kb one 0.08-0.09 ms slower)
    p.chunk_split = c.windows ? 2 : 0;
    const bool affine_dp = scr.go != scr.ge;
    ChunkGroupParams cg{};
    std::vector<int> singles;
    for (int k = c.n_bk - 1; k >= 0; --k) {
        const int b = c.used[k];
        if (p.chunk_split == 0 && affine_dp && c.pack_mode[k] == 2 && kBuckets[b].kind == FAST &&
            kBuckets[b].rpl <= kChunkGroupRpl && cg.n_seg < kMaxChunkSegs) {
            ChunkSeg &sg = cg.seg[cg.n_seg++];
            sg.adp_pad = adps->pad[b];
            sg.adp_len = adps->len[b];
            sg.adp_id = adps->id[b];
            sg.dev_waves = pl.bk_waves + 2 * k;
            sg.n_adp = adps->count[b];
            sg.rpl = kBuckets[b].rpl;
        } else {
            singles.push_back(k);
        }
    }
    if (cg.n_seg == 1) {                         // a lone bucket: its own launch, as before
        for (int k = 0; k < c.n_bk; ++k)
            if (pl.bk_waves + 2 * k == cg.seg[0].dev_waves) singles.push_back(k);
        cg.n_seg = 0;
    }
    std::sort(singles.begin(), singles.end());
    const size_t n_launch = singles.size() + (cg.n_seg ? 1 : 0);
    ForkJoin fj;
    if (int rc = fj.begin(c.st, c.round_base + x.r >= c.dp_serial_from ? 1 : n_launch)) return rc;
    size_t li = 0;
    if (cg.n_seg) {
        cg.p = p;
        dispatch_chunk_group(cg, 4 * (unsigned)p.n_waves, fj.at(li++));
    }
    for (int k : singles) {
        const int b = c.used[k];
        p.adp_pad = adps->pad[b];
        p.adp_len = adps->len[b];
        p.adp_id = adps->id[b];
        p.n_adp = adps->count[b];
        p.rt = adps->rt[b];
        p.dev_waves = pl.bk_waves + 2 * k;
        // the packed buckets (36+ rows) of the whole-read rounds on the row-split core, two
        // lanes per chunk task (r06: 8 kb middle scan 1.74-1.86 -> 1.71-1.75 ms; their
        // one-lane waves hold 109-132 VGPRs, 3-4 waves per SIMD)
        const int split_keep = p.chunk_split;
        if (p.chunk_split == 0 && c.pack_mode[k] != 2 && kBuckets[b].kind == FAST && kBuckets[b].rpl >= 36)
            p.chunk_split = 2;
        const int rc_d = dispatch_chunk(b, p, affine_dp, fj.at(li++), c.pack_mode[k] == 2);
        p.chunk_split = split_keep;
        if (rc_d) {
            (void)fj.end();
            return rc_d;
        }
    }
    if (int rc = fj.end()) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}

// One candidate-DP plan into a set of task slots, planned and run (with the profile's marks).
int run_plan(RoundsCall &c, const RoundCtx &x, PlanSlots &pl, bool win, const int32_t *cmask) {
    MidProf &prof = c.sc->prof;
    if (int rc = pl.reserve(x.slots_cap)) return rc;
    const hipEvent_t pr_plan = prof.mark(-1, nullptr, c.st);
    if (int rc = plan_slots(c, x, pl, win, cmask)) return rc;
    const hipEvent_t pr_dp = prof.mark(kPhPlan, pr_plan, c.st);
    if (int rc = plan_dp(c, x, pl)) return rc;
    if (prof.on) {
        (void)prof.mark(kPhDp, pr_dp, c.st);
        hipLaunchKernelGGL(k_prof_cells, dim3(256), dim3(256), 0, c.st, pl.tw.p, pl.tck.p, pl.cand.p, x.dcand, x.v_len,
                           c.sc->plen.p, pl.slots, prof.counters.p);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

void merge_reset(RoundsCall &c, const RoundCtx &x, int32_t *cert) {
    pcabi_scan *sc = c.sc;
    hipLaunchKernelGGL(k_merge_reset, dim3(kGrid), dim3(256), 0, c.st, sc->pbest.p, x.dcount, x.ncap, sc->phit.p,
                       sc->phb.p, x.nr, cert);
}
void merge_best(RoundsCall &c, const RoundCtx &x, const PlanSlots &pl) {
    hipLaunchKernelGGL(k_merge_best, dim3(kGrid), dim3(256), 0, c.st, pl.tw.p, pl.tck.p, pl.cand.p, pl.res.p,
                       x.slots_cap, pl.slots, c.sc->pbest.p);
}
void merge_hit(RoundsCall &c, const RoundCtx &x, const PlanSlots &pl, int pass, const int32_t *cmask) {
    pcabi_scan *sc = c.sc;
    hipLaunchKernelGGL(k_merge_hit, dim3(kGrid), dim3(256), 0, c.st, x.dcand, pl.tw.p, pl.tck.p, pl.cand.p, pl.res.p,
                       x.slots_cap, pl.slots, sc->pbest.p, c.threshold, pass, sc->phit.p, sc->phb.p, c.n, cmask, 0);
}

// A whole-read round: every candidate's read in chunks, merged per candidate, then per read.
int whole_read_round(RoundsCall &c, const RoundCtx &x) {
    PlanSlots &pw = c.sc->plan;
    if (int rc = run_plan(c, x, pw, false, nullptr)) return rc;
    merge_reset(c, x, nullptr);
    merge_best(c, x, pw);
    for (int pass = 0; pass < 2; ++pass) merge_hit(c, x, pw, pass, nullptr);
    return 0;
}

// A candidate-window round: the windows; then per candidate the certificate (k_certify): its best
// window score is the whole read's when it lies above every score an alignment without an exact
// piece, or with more gap columns than the band, can reach; the other candidates (flagged) run
// their whole reads in chunks, into the same merge.
int window_round(RoundsCall &c, const RoundCtx &x) {
    pcabi_scan *sc = c.sc;
    PlanSlots &pw = sc->plan, &pf = sc->plan2;
    if (int rc = run_plan(c, x, pw, true, nullptr)) return rc;
    merge_reset(c, x, sc->pcert.p);
    merge_best(c, x, pw);
    hipLaunchKernelGGL(k_certify, dim3(kGrid), dim3(256), 0, c.st, x.dcand, pw.tw.p, pw.tck.p, pw.cand.p, pw.res.p,
                       x.slots_cap, pw.slots, c.threshold, sc->pucert.p, sc->pbest.p, sc->pcert.p, sc->ptasks.p,
                       sc->pfill.p, c.adps->n_adp);
    const int32_t *flagged = sc->pcert.p;
    if (int rc = run_plan(c, x, pf, false, flagged)) return rc;
    merge_best(c, x, pf);
    for (int pass = 0; pass < 2; ++pass) {
        merge_hit(c, x, pw, pass, flagged);       // certified candidates: their windows
        merge_hit(c, x, pf, pass, nullptr);       // flagged candidates: their whole reads
    }
    return 0;
}

// The round's hit count and list, the next round's reads, and the hits masked in the shadow copies.
int round_hits(RoundsCall &c, const RoundCtx &x) {
    pcabi_scan *sc = c.sc;
    RoundCtl *ctl = c.ctl;
    const int r = x.r;
    hipLaunchKernelGGL(k_round_count, dim3(c.gn), dim3(256), 0, c.st, sc->phb.p, x.nr, x.sflags, &ctl->plan_flag,
                       sc->pcount.p);
    hipLaunchKernelGGL(k_round_hits, dim3(c.gn), dim3(256), 0, c.st, sc->phb.p, c.n, x.nr, x.cur, sc->pcount.p,
                       c.list_of(r), ctl->n + r + 1, c.cur_of(r + 1), c.start_of(r + 1), x.sflags, &ctl->plan_flag,
                       ctl->flag + r, c.win_off, c.eoff, c.win_len, &ctl->bump);
    hipLaunchKernelGGL(k_mask_list, dim3(4096), dim3(256), 0, c.st, c.codes, c.win_off, c.eoff, c.win_len, c.list_of(r),
                       ctl->n + r + 1, sc->shadow.p, shadow_rel(sc, c.codes),
                       (x.fault & 8) ? (int64_t)-1 : sc->shadow_cap, &ctl->bump, ctl->flag + r);
    HIP_TRY(hipGetLastError());
    return 0;
}

// PCABI_DEBUG: the round's counts (debugging only: a synchronisation per round).
int debug_round(RoundsCall &c, const RoundCtx &x) {
    pcabi_scan *sc = c.sc;
    int64_t cnt[5];
    if (int rc = pcabi_seed::debug_counts(sc->seed, cnt, c.st)) return rc;
    int32_t rn[2];
    int64_t sl = 0;
    HIP_TRY(hipMemcpy(rn, c.ctl->n + x.r, 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&sl, &c.ctl->slots, 8, hipMemcpyDeviceToHost));
    std::fprintf(stderr, "[pcabi] middle round %lld: %d reads, band tasks %lld + %lld edge, %lld + %lld edge, "
                 "%lld candidates, %lld task slots, %d hits\n", (long long)(c.round_base + x.r), rn[0],
                 (long long)cnt[0], (long long)cnt[1], (long long)cnt[2], (long long)cnt[3], (long long)cnt[4],
                 (long long)sl, rn[1]);
    if (!c.windows) return 0;
    // the certificate's flagged candidates, their plan
    std::vector<int32_t> fl((size_t)std::max<int64_t>(1, std::min<int64_t>(cnt[4], x.ncap)));
    HIP_TRY(hipMemcpy(fl.data(), sc->pcert.p, 4 * fl.size(), hipMemcpyDeviceToHost));
    int64_t nf = 0, sl2 = 0;
    for (int32_t f : fl) nf += f != 0;
    HIP_TRY(hipMemcpy(&sl2, sc->plan2.slots, 8, hipMemcpyDeviceToHost));
    std::vector<int32_t> bw(2 * (size_t)c.n_bk), bw2(2 * (size_t)c.n_bk);
    HIP_TRY(hipMemcpy(bw.data(), sc->plan.bk_waves, 4 * bw.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(bw2.data(), sc->plan2.bk_waves, 4 * bw2.size(), hipMemcpyDeviceToHost));
    std::string w1, w2;
    for (int b = 0; b < c.n_bk; ++b) {
        w1 += " " + std::to_string(bw[2 * b + 1]);
        w2 += " " + std::to_string(bw2[2 * b + 1]);
    }
    std::fprintf(stderr, "[pcabi]   windows plan waves per bucket:%s; %lld flagged, whole-read plan %lld slots, "
                 "waves per bucket:%s\n", w1.c_str(), (long long)nf, (long long)sl2, w2.c_str());
    return 0;
}

// One round queued on the stream: views, seeds, the plan(s) and their merges, then count, hits and mask.
int queue_round(RoundsCall &c, int r) {
    pcabi_scan *sc = c.sc;
    RoundCtx x;
    x.r = r;
    x.fault = take_faults(c, r);
    if (x.fault & 3) pcabi_seed::shrink_next(sc->seed, x.fault & 3);
    if (c.round_base + r >= kMiddleSerialFrom) pcabi_seed::serial_next(sc->seed);
    x.slots_cap = (x.fault & 4) ? 64 : sc->q_slots_cap;
    if (int rc = sc->plan.reserve(x.slots_cap)) return rc;
    x.first = c.first_round(r);
    x.nr = c.ctl->n + r;
    x.start = x.first ? nullptr : c.start_of(r);
    x.cur = x.first ? nullptr : c.cur_of(r);
    x.ncap = c.n * (int64_t)c.adps->n_adp;
    if (int rc = sc->prof.begin_round(sc->seed, c.st)) return rc;
    MidProf::SeedMarksOff seed_marks_off{sc->seed};
    if (int rc = round_seeds(c, x)) return rc;
    if (int rc = c.windows ? window_round(c, x) : whole_read_round(c, x)) return rc;
    if (int rc = round_hits(c, x)) return rc;
    if (g_debug)
        if (int rc = debug_round(c, x)) return rc;
    return sc->prof.end_round(sc->seed, x.first, c.st);
}

// A round other than the call's first, when it runs serial: replayed from its slot's captured graph
// while the key holds, captured on the second sight of a key, else queued directly.
int run_round(RoundsCall &c, int r) {
    pcabi_scan *sc = c.sc;
    const bool serial = c.round_base + r >= kMiddleSerialFrom && c.round_base + r >= c.dp_serial_from;
    if (!c.graphs_on || c.first_round(r) || !serial) return queue_round(c, r);
    const hipStream_t st = c.st;
    RoundKey key{c.round_base, (int64_t)(intptr_t)c.codes, (int64_t)(intptr_t)c.win_off, (int64_t)(intptr_t)c.win_len,
                 c.n, c.windows ? 1 : 0, (int64_t)(c.threshold * 1e6), c.scr.ma, c.scr.mi, c.scr.go, c.scr.ge,
                 (int64_t)c.adps->serial, sc->q_slots_cap, sc->shadow_cap, (int64_t)(intptr_t)sc->shadow.p, c.target,
                 (int64_t)g_buf_gen.load()};
    auto &g = sc->graphs[r & 31];
    if (g.exec && g.key == key) {
        HIP_TRY(hipGraphLaunch(g.exec, st));
        return 0;
    }
    if (g.exec) {
        (void)hipGraphExecDestroy(g.exec);
        g.exec = nullptr;
    }
    // captured on the second sight of a key: a caller alternating inputs (or switches) keeps
    // queueing directly instead of paying a capture per call
    if (g.seen != key) {
        g.seen = key;
        return queue_round(c, r);
    }
    // the round's buffers exist after round 1 of this call; a reallocation while capturing would
    // change the generation: the graph is then dropped and the round queued directly
    if (hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed) != hipSuccess) {
        (void)hipGetLastError();
        return queue_round(c, r);
    }
    const uint64_t gen0 = g_buf_gen.load();
    const int rc = queue_round(c, r);
    hipGraph_t graph = nullptr;
    const hipError_t ec = hipStreamEndCapture(st, &graph);
    if (rc) {
        if (graph) (void)hipGraphDestroy(graph);
        return rc;
    }
    hipGraphExec_t exec = nullptr;
    const bool ok = ec == hipSuccess && graph && g_buf_gen.load() == gen0 &&
                    hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess;
    if (graph) (void)hipGraphDestroy(graph);
    if (!ok) {                                   // nothing of the round ran: queue it directly
        (void)hipGetLastError();
        if (exec) (void)hipGraphExecDestroy(exec);
        return queue_round(c, r);
    }
    g.exec = exec;
    key.buf_gen = (int64_t)g_buf_gen.load();
    g.key = key;
    HIP_TRY(hipGraphLaunch(g.exec, st));
    return 0;
}

// Rounds [slot, upto) queued, then the control block and every round's first staged hits in one
// synchronisation.
int queue_batch(RoundsCall &c, int slot, int upto) {
    pcabi_scan *sc = c.sc;
    const hipStream_t st = c.st;
    for (int r = slot; r < upto; ++r) {
        if (int rc = run_round(c, r)) return rc;
        hmark("round");
        if (c.first_round(r))                     // round 1's segment total (the next call's mean length)
            HIP_TRY(hipMemcpyAsync(&sc->h_ctl.p->seg_total, pcabi_seed::seg_cum_dev(sc->seed) + c.n, sizeof(int64_t),
                                   hipMemcpyDeviceToHost, st));
    }
    hmark("queue");
    HIP_TRY(hipMemcpyAsync(&sc->h_ctl.p->c, c.ctl, sizeof(RoundCtl), hipMemcpyDeviceToHost, st));   // counts, flags, needs
    for (int r = slot; r < upto; ++r)
        HIP_TRY(hipMemcpyAsync(sc->h_stage.p + 8 * (size_t)c.spec * (r - slot), c.list_of(r), 32 * (size_t)c.spec,
                               hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    hmark("sync");
    return 0;
}

// The lists of the finished rounds [slot, done_to): the staged part, then (rarely) the rest.
int collect_lists(RoundsCall &c, int slot, int done_to) {
    const RoundCtl &h = c.sc->h_ctl.p->c;
    for (int r = slot; r < done_to; ++r) {
        const int64_t nh = h.n[r + 1];
        if (!nh) continue;
        c.most_hits = std::max(c.most_hits, nh);
        const int32_t *st_r = c.sc->h_stage.p + 8 * (size_t)c.spec * (r - slot);
        c.out.insert(c.out.end(), st_r, st_r + 8 * (size_t)std::min(nh, c.spec));
        if (nh > c.spec) {
            const size_t old = c.out.size();
            c.out.resize(old + 8 * (size_t)(nh - c.spec));
            HIP_TRY(hipMemcpy(c.out.data() + old, c.list_of(r) + 8 * c.spec, 32 * (size_t)(nh - c.spec),
                              hipMemcpyDeviceToHost));
        }
        c.out_round.insert(c.out_round.end(), (size_t)nh, c.round_base + r);
    }
    return 0;
}

void debug_batch(const RoundsCall &c, int slot, int upto) {
    const RoundCtl &h = c.sc->h_ctl.p->c;
    for (int r = slot; r < upto; ++r)
        std::fprintf(stderr, "[pcabi] middle queued round %lld: %d reads, %d hits, flag %d\n",
                     (long long)(c.round_base + r), h.n[r], h.n[r + 1], h.flag[r]);
}

// Round `bad` flagged an overflow (nothing of it or after it was kept): grow what overflowed, so
// that it can be queued again.
int recover_overflow(RoundsCall &c, int bad) {
    pcabi_scan *sc = c.sc;
    const RoundCtl &h = sc->h_ctl.p->c;
    const int flag = h.flag[bad];
    g_requeues.fetch_add(1);
    g_requeue_flags.fetch_or(flag & 15);
    // the rounds queued behind it ran on no reads: their injected faults fire again
    for (size_t k = 0; k < c.faults.size(); ++k)
        if (c.faults[k].first > c.round_base + bad) c.fired[k] = 0;
    if (c.injected[bad]) {
        // an injected overflow (tests): the real buffers were large enough, queue it again
    } else if ((flag & 3) && !pcabi_seed::grow_after_overflow(sc->seed, flag & 1, (flag >> 1) & 1)) {
        return fail(PCABI_E_DEVICE, "middle scan: seed buffers past their limits");
    }
    if ((flag & 4) && !c.injected[bad]) {
        // need2: the whole-read plan's slots, written only by the window rounds' second plan
        const int64_t most = std::max(h.need, c.windows ? h.need2 : (int64_t)0);
        sc->q_slots_cap = std::max<int64_t>(2 * sc->q_slots_cap, most + most / 4);
    }
    // the shadow arena was too small for the round's first hits: a larger one (the copies
    // made so far move with it), allocations go on past the old end
    if ((flag & 8) && (int64_t)h.bump > sc->shadow_cap)
        if (int rc = shadow_grow(sc, c.codes, c.win_off, c.eoff, c.n, (int64_t)h.bump, &c.ctl->bump, c.st)) return rc;
    HIP_TRY(hipStreamSynchronize(c.st));
    return 0;
}

// Past the last slot: the next round's reads move to slot 0, the round numbers go on.
int wrap_slots(RoundsCall &c) {
    const int32_t n_next = c.sc->h_ctl.p->c.n[kSlots];
    const hipStream_t st = c.st;
    HIP_TRY(hipMemcpyAsync(c.cur_of(0), c.cur_of(kSlots), 4 * (size_t)n_next, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(c.start_of(0), c.start_of(kSlots), 4 * (size_t)n_next, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(c.ctl->n, c.ctl->n + kSlots, 4, hipMemcpyDeviceToDevice, st));
    c.round_base += kSlots;
    return 0;
}

// The hits in (round, read) order: per read the reference's discovery order. The rounds come in
// order and each round's list in read order (k_round_hits' ordered compaction): only checked here.
int64_t write_hits(const RoundsCall &c, int32_t *hits, int64_t cap) {
    const int64_t total = (int64_t)c.out_round.size();
    for (int64_t j = 1; j < total; ++j)
        if (c.out_round[j] == c.out_round[j - 1] && c.out[8 * j] <= c.out[8 * (j - 1)])
            return fail(PCABI_E_DEVICE, "middle scan: a round's hit list is out of read order");
    for (int64_t q = 0; q < total && q < cap; ++q) {
        const int32_t *o = c.out.data() + 8 * q;
        hits[0 * cap + q] = o[0];
        hits[1 * cap + q] = o[1];
        hits[2 * cap + q] = o[2];
        hits[3 * cap + q] = o[2] == -1 ? 0 : o[3] + 1;
        hits[4 * cap + q] = o[4];
        hits[5 * cap + q] = o[5];
    }
    return total;
}

// The whole seeded middle scan as QUEUED rounds: no host synchronisation between the end trim and
// the scan's result. Every round runs the seeded plan's steps with its counts on the device -- the
// reads of the round (round 1: all windows, longest first by a device radix sort; later: those
// that just hit, from the adapter that hit), the seeds (pcabi_seed::bounds_dev), the plan's counts,
// layout and task slots (k_plan_count, k_plan_layout, k_plan_place), the chunked candidate DP (the
// launches stride over the device's wave counts), the merges, the round's hit list and the
// masking. The host queues kBatch rounds, reads the round counts once, and queues more while
// reads still hit. A buffer that overflowed in a round flags it before anything of it is kept or
// masked; the host grows the buffers and queues that round again. The hits come back once, sorted
// by (round, read): per read the reference's discovery order.
// Returns the hit count (> 0, <= 0 on error as pcabi_middle_scan_dev); applied = false when the
// seeded plan does not cover this table and scoring (the caller runs the host-driven loop).
int64_t middle_device_rounds(pcabi_scan *sc, const uint8_t *codes, const int64_t *win_off, const int32_t *win_len,
                             const int32_t *h_win_len, int64_t n_win, const pcabi::Scoring &scr, double threshold,
                             int32_t *hits, int64_t cap, hipStream_t st, bool &applied) {
    applied = false;
    RoundsCall c{sc, sc->adps, codes, win_off, win_len, n_win, scr, threshold, st};
    const int ready = rounds_plan(c);
    if (ready <= 0) return ready;
    applied = true;
    if (int rc = rounds_buffers(c, h_win_len)) return rc;
    if (int rc = rounds_start(c)) return rc;
    const RoundCtlHost &h = *sc->h_ctl.p;
    // the first batch's rounds: as many as the previous call needed (its rounds up to the first one
    // that found nothing), 2 to 3. Data where round 2 finds nothing then skips a third round of ~35
    // empty launches, data with a third round pays no extra host round trip for it (r05y, in-process
    // A/B: the 20 kb scan 2.86 ms with 3 against 2.72 with 2, the 8 kb one 2.01 with 3 against 2.19
    // with 2).
    const int batch1 = std::min(kBatch, std::max(2, sc->rounds_hint));
    int slot = 0;                                   // next round to queue (slot index)
    hmark("pre");
    for (int guard = 0;; ++guard) {
        if (guard > 10000) return fail(PCABI_E_DEVICE, "middle scan: rounds did not settle");
        const int upto = std::min(slot + (c.first_round(slot) ? batch1 : kBatch), kSlots);
        if (int rc = queue_batch(c, slot, upto)) return rc;
        // the first flagged round: it and the rounds after it are queued again
        int bad = -1;
        for (int r = slot; r < upto && bad < 0; ++r)
            if (h.c.flag[r]) bad = r;
        if (int rc = collect_lists(c, slot, bad >= 0 ? bad : upto)) return rc;
        if (g_debug) debug_batch(c, slot, upto);
        if (bad >= 0) {
            if (int rc = recover_overflow(c, bad)) return rc;
            slot = bad;
            continue;
        }
        if (h.c.n[upto] == 0) {                     // the last queued round found no hit
            // the rounds this call needed: up to the first that found nothing (the next call's first batch)
            int need_r = upto;
            for (int r = slot; r < upto; ++r)
                if (h.c.n[r + 1] == 0) {
                    need_r = r + 1;
                    break;
                }
            sc->rounds_hint = (int)std::min<int64_t>(c.round_base + need_r, 64);
            break;
        }
        slot = upto;
        if (slot == kSlots) {
            if (int rc = wrap_slots(c)) return rc;
            slot = 0;
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
    // the next call stages as many hits per round as this one's busiest round had (+ 25 %), and
    // takes its mean read length from this call's round-1 segments
    hmark("end");
    sc->spec_hits = std::max<int64_t>(4096, c.most_hits + c.most_hits / 4);
    if (h.seg_total >= 0 && c.n > 0) sc->last_mean = (double)h.seg_total * pcabi_seed::seg_positions() / (double)c.n;
    return write_hits(c, hits, cap);
}

}  // namespace

extern "C" {

int32_t pcabi_scan_profile(pcabi_scan *s, int32_t mode, double *out, int32_t n_out) {
    if (!s || mode < 0 || mode > 2 || n_out < 0 || (n_out && !out)) return fail(PCABI_E_ARG, "bad arguments");
    MidProf &p = s->prof;
    if (mode == 1) {
        std::fill(p.ms, p.ms + kPhases, 0.0);
        p.rounds = p.reads = p.bases = p.raw = p.band_in = p.band_edge = p.dp_tasks = p.dp_cells = 0;
        p.round1_ms = 0.0;
        std::fill(p.band, p.band + 8, 0ull);
    }
    if (mode != 2) p.on = mode == 1;
    const int32_t nv = kPhases + 9 + 8 + 2;
    const double v[nv] = {p.ms[0], p.ms[1], p.ms[2], p.ms[3], p.ms[4], p.ms[5], p.ms[6],
                          (double)p.rounds, (double)p.reads, (double)p.bases, (double)p.raw,
                          (double)p.band_in, (double)p.band_edge, (double)p.dp_tasks, (double)p.dp_cells,
                          p.round1_ms,
                          (double)p.band[0], (double)p.band[1], (double)p.band[2], (double)p.band[3],
                          (double)p.band[4], (double)p.band[5], (double)p.band[6], (double)p.band[7],
                          (double)(s->seed ? pcabi_seed::band_e(s->seed, 0) : 0),
                          (double)(s->seed ? pcabi_seed::band_e(s->seed, 1) : 0)};
    const int32_t k = std::min<int32_t>(n_out, nv);
    for (int32_t i = 0; i < k; ++i) out[i] = v[i];
    return nv;
}

int64_t pcabi_middle_requeues(int32_t *flags_seen) {
    if (flags_seen) *flags_seen = g_requeue_flags.load();
    return g_requeues.load();
}

int64_t pcabi_middle_scan_dev(pcabi_scan *sc, const uint8_t *codes, const int64_t *win_off, const int32_t *win_len,
                              const int32_t *h_win_len, int64_t n_win, int match, int mismatch, int gap_open,
                              int gap_extend, double threshold, int32_t *hits, int64_t cap, void *stream) {
    if (!sc || n_win < 0 || cap < 0) return fail(PCABI_E_ARG, "bad arguments");
    if (!(threshold > 0.0))
        return fail(PCABI_E_ARG, "middle threshold must be > 0 (the reference's loop never ends otherwise)");
    const hipStream_t st = (hipStream_t)stream;
    const int32_t n_adp = sc->adps->n_adp;
    if (n_win == 0 || n_adp == 0) return 0;
    HostMarks hm;
    struct MarksOff {
        ~MarksOff() { g_hm = nullptr; }
    } marks_off;
    g_hm = hm.on ? &hm : nullptr;
    hmark("entry");
    // the layout of the scan's table that serves this scoring on these reads (adapters_for: any
    // scoring the reference accepts, any read length), for the duration of the call
    struct TableSwap {
        pcabi_scan *s;
        const pcabi_adapters *own;
        ~TableSwap() { s->adps = own; }
    } swap_back{sc, sc->adps};
    std::vector<int32_t> h_len_copy;
    auto host_lengths = [&]() -> int {              // lengths only on the device: one small copy
        if (h_win_len) return 0;
        h_len_copy.resize((size_t)n_win);
        HIP_TRY(hipMemcpyAsync(h_len_copy.data(), win_len, 4 * (size_t)n_win, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        h_win_len = h_len_copy.data();
        return 0;
    };
    const pcabi::Scoring scoring{match, mismatch, gap_open, gap_extend};
    {
        // the longest window decides the layout only when the table may not serve every length
        // (a scoring without a span bound): otherwise no length needs to come to the host
        int32_t longest = INT32_MAX / 2;
        if (!layout_serves(sc->adps, scoring, longest)) {
            if (int rc = host_lengths()) return rc;
            longest = 0;
            for (int64_t k = 0; k < n_win; ++k) longest = std::max(longest, h_win_len[k]);
        }
        const pcabi_adapters *use = nullptr;
        if (int rc = adapters_for(sc->adps, scoring, longest, &use)) return rc;
        sc->adps = use;
    }
    {
        bool applied = false;
        const int64_t r = middle_device_rounds(sc, codes, win_off, win_len, h_win_len, n_win, scoring, threshold, hits,
                                               cap, st, applied);
        if (applied || r < 0) return r;
    }
    if (int rc = host_lengths()) return rc;
    // input-preserving masking (k_mask_list): effective offsets, shadows allocated on the host here
    if (int rc = sc->eoff.ensure(n_win)) return rc;
    if (int rc = sc->shadow_zero.ensure(1)) return rc;
    if (int rc = shadow_reserve(sc, h_win_len, n_win)) return rc;
    int64_t *eoff = sc->eoff.p;
    HIP_TRY(hipMemcpyAsync(eoff, win_off, sizeof(int64_t) * n_win, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemsetAsync(sc->shadow_zero.p, 0, sizeof(unsigned long long), st));
    std::vector<char> shadowed((size_t)n_win, 0);
    int64_t sh_bump = kShadowLead;                  // arena bytes taken (the lead-in first)
    int64_t n_hits = 0;
    std::vector<int32_t> cur, nxt, nxt_start, hm_list, lens;
    std::vector<int32_t> hb;
    std::vector<int64_t> toff;
    std::vector<int16_t> h16;                       // round-1 filter scores (bounds for later rounds)
    std::vector<int32_t> pos1((size_t)n_win, 0);    // read -> round-1 position
    bool filt_round1 = false;
    bool seeded = false;                            // round 1 took its bounds from seeds
    // Round 1 visits the reads longest first: lanes of a wave (and tiles) then run near-equal
    // column counts (read lengths are log-normal; unsorted, a wave would idle ~2/3 of its lanes).
    cur.resize((size_t)n_win);
    for (int64_t k = 0; k < n_win; ++k) cur[k] = (int32_t)k;
    {
        // longest first, ties in read order: a stable LSD radix sort on (longest - length), 11-bit
        // digits over the bits the longest length needs (two passes up to 4 M bases)
        int32_t longest = 0;
        for (int64_t k = 0; k < n_win; ++k) longest = std::max(longest, h_win_len[k]);
        int bits = 1;
        while (bits < 31 && (1u << bits) <= (uint32_t)longest) ++bits;
        std::vector<int32_t> tmp((size_t)n_win);
        std::vector<uint32_t> key((size_t)n_win), ktmp((size_t)n_win);
        for (int64_t k = 0; k < n_win; ++k) key[k] = (uint32_t)(longest - std::max(h_win_len[k], 0));
        constexpr int kDig = 11;
        std::vector<int64_t> cnt((size_t)1 << kDig);
        for (int sh = 0; sh < bits; sh += kDig) {
            std::fill(cnt.begin(), cnt.end(), 0);
            for (int64_t k = 0; k < n_win; ++k) ++cnt[(key[k] >> sh) & ((1u << kDig) - 1)];
            int64_t run = 0;
            for (int64_t &c : cnt) { const int64_t x = c; c = run; run += x; }
            for (int64_t k = 0; k < n_win; ++k) {
                const int64_t d = cnt[(key[k] >> sh) & ((1u << kDig) - 1)]++;
                tmp[d] = cur[k];
                ktmp[d] = key[k];
            }
            cur.swap(tmp);
            key.swap(ktmp);
        }
    }
    for (int round = 0;; ++round) {
        const int64_t n = (int64_t)cur.size();
        const int64_t *v_off = eoff;
        const int32_t *v_len = win_len;
        lens.resize((size_t)n);
        {
            for (int64_t k = 0; k < n; ++k) lens[k] = h_win_len[cur[k]];
            if (int rc = sc->idx.ensure(n)) return rc;
            if (int rc = sc->start.ensure(n)) return rc;
            if (int rc = sc->soff.ensure(n)) return rc;
            if (int rc = sc->slen.ensure(n)) return rc;
            HIP_TRY(hipMemcpyAsync(sc->idx.p, cur.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, st));
            if (round > 0)
                HIP_TRY(hipMemcpyAsync(sc->start.p, nxt_start.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_gather_views, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, eoff, win_len,
                               sc->idx.p, n, sc->soff.p, sc->slen.p);
            v_off = sc->soff.p;
            v_len = sc->slen.p;
        }
        // tiles of this round's windows (the score filter and the full cross product read them)
        int32_t max_len = 0;
        for (int32_t l : lens) max_len = std::max(max_len, l);
        if (int rc = sc->hits.ensure(5 * (size_t)n)) return rc;
        bool tiled = false;
        auto make_tiles = [&]() -> int {
            if (tiled) return 0;
            toff.assign((size_t)((n + 255) / 256 + 1), 0);
            int64_t max_nq = 0;
            const int64_t nd = tile_layout(lens.data(), n, toff.data(), &max_nq);
            if (int rc = sc->toff.ensure(toff.size())) return rc;
            if (int rc = sc->tiles.ensure((size_t)nd)) return rc;
            HIP_TRY(hipMemcpyAsync(sc->toff.p, toff.data(), sizeof(int64_t) * toff.size(), hipMemcpyHostToDevice, st));
            launch_tiles(codes, v_off, v_len, n, sc->toff.p, max_nq, sc->tiles.p, st);
            tiled = true;
            return 0;
        };
        int filt = 0;
        if (middle_filter_on() && (round == 0 || filt_round1)) {
            filt = filtered_first_hits(sc, codes, v_off, v_len, lens.data(), n, round == 0 ? nullptr : nxt_start.data(),
                                       round == 0 ? nullptr : sc->start.p, max_len,
                                       cur.data(), h16, n_win, pos1,
                                       pcabi::Scoring{match, mismatch, gap_open, gap_extend}, threshold, hb, seeded,
                                       make_tiles, st);
            if (round == 0) {
                // the bound needs masked bases (N) to never match an adapter base
                filt_round1 = filt > 0 && !sc->adps->has_n;
                for (int64_t k = 0; k < n; ++k) pos1[cur[k]] = (int32_t)k;
            }
            if (filt < 0) return filt;
        }
        if (!filt) {
            const auto t0 = std::chrono::steady_clock::now();
            if (int rc = make_tiles()) return rc;
            if (g_debug) HIP_TRY(hipStreamSynchronize(st));
            const auto t1 = std::chrono::steady_clock::now();
            if (int rc = sc->res.ensure(PCABI_NFIELDS * (size_t)n * n_adp)) return rc;
            if (int rc = pcabi_align_cross_dev(sc->tiles.p, sc->toff.p, v_len, n,
                                               max_len, sc->adps, match, mismatch, gap_open, gap_extend,
                                               sc->res.p, n * n_adp, stream))
                return rc;
            if (g_debug) {
                HIP_TRY(hipStreamSynchronize(st));
                const auto t2 = std::chrono::steady_clock::now();
                std::fprintf(stderr, "[pcabi] middle host round %d: tiles %.3f ms, cross product %.3f ms (%lld x %d, longest %d)\n",
                             round, std::chrono::duration<double, std::milli>(t1 - t0).count(),
                             std::chrono::duration<double, std::milli>(t2 - t1).count(), (long long)n, n_adp, max_len);
            }
            if (int rc = first_hit_from(sc->res.p, n * n_adp, n, n_adp, threshold,
                                        round == 0 ? nullptr : sc->start.p, sc->hits.p, n, st))
                return rc;
            hb.resize((size_t)(5 * n));
            HIP_TRY(hipMemcpyAsync(hb.data(), sc->hits.p, sizeof(int32_t) * 5 * n, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        nxt.clear(); nxt_start.clear(); hm_list.clear();
        for (int64_t k = 0; k < n; ++k) {
            const int32_t a = hb[k];
            if (a < 0) continue;
            const int32_t r = cur[k];
            const int32_t rs = hb[n + k], re = hb[2 * n + k];
            const int32_t rend = rs == -1 ? 0 : re + 1;
            if (n_hits < cap) {
                hits[0 * cap + n_hits] = r;
                hits[1 * cap + n_hits] = a;
                hits[2 * cap + n_hits] = rs;
                hits[3 * cap + n_hits] = rend;
                hits[4 * cap + n_hits] = hb[3 * n + k];
                hits[5 * cap + n_hits] = hb[4 * n + k];
            }
            ++n_hits;
            nxt.push_back(r);
            nxt_start.push_back(a);
            if (rend > rs) {                       // k_mask_list's entry; a read's first: its shadow
                int32_t unit = 0;
                if (!shadowed[r]) {
                    shadowed[r] = 1;
                    unit = (int32_t)(sh_bump / 16) + 1;
                    sh_bump += (std::max(h_win_len[r], 0) + 16 + 15) & ~(int64_t)15;
                }
                const int32_t e[8] = {r, a, rs, re, 0, 0, 0, unit};
                hm_list.insert(hm_list.end(), e, e + 8);
            }
        }
        if (g_debug)
            std::fprintf(stderr, "[pcabi] middle host round %d: %lld reads, %zu hits (%s)\n", round, (long long)n,
                         nxt.size(), filt ? "filtered" : "cross product");
        if (nxt.empty()) break;
        if (!hm_list.empty()) {
            if (sh_bump > sc->shadow_cap) {           // grow first: this round's copies go past the end
                if (sh_bump > kShadowMax) return fail(PCABI_E_NOMEM, "middle scan: shadow arena past its limit");
                if (int rc = shadow_grow(sc, codes, win_off, eoff, n_win, sh_bump, nullptr, st)) return rc;
            }
            const int32_t m = (int32_t)(hm_list.size() / 8);
            if (int rc = sc->mwin.ensure((hm_list.size() + 1))) return rc;
            HIP_TRY(hipMemcpyAsync(sc->mwin.p, hm_list.data(), sizeof(int32_t) * hm_list.size(), hipMemcpyHostToDevice, st));
            int32_t *d_m = sc->mwin.p + hm_list.size();
            HIP_TRY(hipMemcpyAsync(d_m, &m, sizeof(int32_t), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_mask_list, dim3((unsigned)std::min<int32_t>(m, 1024)), dim3(256), 0, st, codes, win_off,
                               eoff, win_len, sc->mwin.p, d_m, sc->shadow.p,
                               shadow_rel(sc, codes), sc->shadow_cap, sc->shadow_zero.p,
                               (int32_t *)nullptr);
            HIP_TRY(hipGetLastError());
        }
        // host vectors uploaded above must stay intact until the copies ran
        HIP_TRY(hipStreamSynchronize(st));
        // next round: the reads that just hit, longest first, each from the adapter that hit
        std::vector<int32_t> perm(nxt.size());
        for (size_t k = 0; k < perm.size(); ++k) perm[k] = (int32_t)k;
        std::stable_sort(perm.begin(), perm.end(),
                         [&](int32_t x, int32_t y) { return h_win_len[nxt[x]] > h_win_len[nxt[y]]; });
        cur.resize(perm.size());
        std::vector<int32_t> st_sorted(perm.size());
        for (size_t k = 0; k < perm.size(); ++k) { cur[k] = nxt[perm[k]]; st_sorted[k] = nxt_start[perm[k]]; }
        nxt_start.swap(st_sorted);
    }
    return n_hits;
}

}  // extern "C"
