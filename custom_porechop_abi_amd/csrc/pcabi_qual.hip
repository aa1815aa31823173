// pcabi_qual.hip -- the quality stage on the GPU (gfx950): reads cropped at both ends to their outermost
// windows of acceptable quality, then their length and mean-quality tests (include/pcabi.h pcabi_qual_*;
// DESIGN.md "Quality stage"); the rule and every per-lane function are csrc/pcabi_qual.h's, the same the
// host build runs.
//
// k_qual_crop: one wave per read. scan_wave takes 64 window starts a pass: a lane loads the quality byte of
//   its step and, the first W - 1 lanes, the one 64 further on; two wave prefix sums give every lane its
//   window's sum, a ballot names the first lane that qualifies, and the scan stops at the first pass that
//   holds one. The same runs from the tail over mirrored steps. front / tail / kept go into the read's
//   record and n_segs(kept) into the array the scan takes.
// the scan: hipcub's exclusive device scan over the reads' segment counts, one value more than there are
//   reads, so seg_off[read] is a read's first segment and seg_off[n_reads] their number.
// k_qual_sum: the work is spread by bytes, not by reads: one wave per segment of kSeg kept bytes. The grid
//   is the host's upper bound from the uncropped spans; a wave beyond the device's count exits. A binary
//   search of seg_off names the segment's read (owner_of: the last read that starts at or before it, so
//   runs of reads without segments fall out); E[] lies in LDS; sum_lane takes the segment's 16-byte loads,
//   a wave sum gives its two sums.
// k_qual_finish: one thread per read adds its segments' sums and sets the flags.
// Every loop runs to a length the host passed and checked, or that the kernel checked against the blob's
// length (a span outside the blob is a read without qualities: nothing of it is read). No atomics, no
// inline assembly.
// The piece stage (pcabi_qual_pieces_*, further down) lists the pieces of the split reads on the device and
// runs the same four kernels over them: a span is a span, of a read or of a piece.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <string>
#include <thread>
#include <vector>

#include "../../include/pcabi.h"
#include "pcabi_hostdev.h"
#include "pcabi_pieces.h"
#include "pcabi_qual.h"

using namespace pcabi_internal;
using namespace pcabi_qual;

static_assert(sizeof(pcabi_qual_read) == 32, "pcabi_qual_read is 32 bytes");

namespace {

constexpr int kWave = 64;

__device__ inline int64_t wave_sum(int64_t x) {
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) x += __shfl_xor((long long)x, d);
    return x;
}

__device__ inline int wave_prefix(int x, int lane) {   // inclusive
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    return x;
}

// the last i in [0, n) with off[i] <= v (off ascending, off[0] <= v)
__device__ inline int64_t owner_of(const int64_t *off, int64_t n, int64_t v) {
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// scan_host for a wave: the first step v in [0, n - W] whose window sums to min_sum or more, or -1
__device__ inline int64_t scan_wave(const uint8_t *q, int64_t n, int W, int64_t min_sum, bool from_tail, int lane) {
    for (int64_t base = 0; base + W <= n; base += kWave) {   // uniform
        const int64_t j0 = base + lane, j1 = j0 + kWave;
        const int x0 = j0 < n ? phred(q[step_pos(n, from_tail, j0)]) : 0;
        const int x1 = lane < W - 1 && j1 < n ? phred(q[step_pos(n, from_tail, j1)]) : 0;
        const int p0 = wave_prefix(x0, lane), p1 = wave_prefix(x1, lane);
        // the sum of the steps [base, base + j): 0 for j = 0, p0[j - 1] up to 64, then p0[63] + p1[j - 65]
        const int hi = lane + W;   // 1 .. 127
        const int in0 = __shfl(p0, (hi - 1) & 63), in1 = __shfl(p1, (hi - 65) & 63), all0 = __shfl(p0, 63);
        const int s = (hi <= kWave ? in0 : all0 + in1) - (p0 - x0);
        const uint64_t m = __ballot(j0 + W <= n && s >= min_sum);
        if (m) return base + (__ffsll((long long)m) - 1);
    }
    return -1;
}

__global__ __launch_bounds__(kWave) void k_qual_crop(const uint8_t *__restrict__ qual, int64_t qual_n, const int64_t *__restrict__ span_off,
                                                     const int32_t *__restrict__ span_len, int64_t n_reads, pcabi_qual_opts o,
                                                     pcabi_qual_read *__restrict__ out, int64_t *__restrict__ nseg) {
    const int64_t ri = blockIdx.x;
    if (ri >= n_reads) return;
    const int lane = threadIdx.x;
    int64_t off = span_off[ri], n = span_len[ri];
    if (!span_fits(off, n, qual_n)) off = -1, n = n < 0 ? 0 : n;
    pcabi_qual_read r;
    r.front = r.tail = 0, r.kept = (int32_t)n, r.q_sum = 0, r.err_sum = 0;
    r.flags = off >= 0 ? 0 : PCABI_QUAL_NO_QUALITIES;
    if (crop_on(o, off)) {   // uniform
        const int64_t vf = scan_wave(qual + off, n, o.window, o.min_window_sum, false, lane);
        const int64_t vt = vf < 0 ? 0 : scan_wave(qual + off, n, o.window, o.min_window_sum, true, lane);
        crop_of(n, vf, vt, &r);
    }
    if (lane == 0) {
        out[ri] = r;
        nseg[ri] = off >= 0 ? n_segs(r.kept) : 0;
        if (ri == 0) nseg[n_reads] = 0;
    }
}

__global__ __launch_bounds__(kWave) void k_qual_sum(const uint8_t *__restrict__ qual, const int64_t *__restrict__ span_off, int64_t n_reads,
                                                    const pcabi_qual_read *__restrict__ recs, const int64_t *__restrict__ seg_off,
                                                    int64_t n_segs_cap, int64_t *__restrict__ seg_q, uint64_t *__restrict__ seg_err) {
    __shared__ uint64_t s_err[kMaxQ + 1];
    const int lane = threadIdx.x;
    for (int k = lane; k <= kMaxQ; k += kWave) s_err[k] = err_of(k);
    __syncthreads();
    const int64_t sg = blockIdx.x;
    if (sg >= n_segs_cap || sg >= seg_off[n_reads]) return;   // surplus
    const int64_t ri = owner_of(seg_off, n_reads + 1, sg);
    if (ri >= n_reads) return;
    const pcabi_qual_read r = recs[ri];
    const int64_t k = sg - seg_off[ri];
    int64_t qs = 0;
    uint64_t es = 0;
    if (!(r.flags & PCABI_QUAL_NO_QUALITIES) && k * kSeg < r.kept) {   // uniform
        const int64_t a0 = span_off[ri] + r.front;
        sum_lane(qual, a0 + k * kSeg, a0 + std::min<int64_t>(r.kept, (k + 1) * kSeg), lane, kWave, [&](int p) { return s_err[p]; }, &qs, &es);
    }
    qs = wave_sum(qs);
    es = (uint64_t)wave_sum((int64_t)es);
    if (lane == 0) seg_q[sg] = qs, seg_err[sg] = es;
}

__global__ void k_qual_finish(int64_t n_reads, pcabi_qual_opts o, const int64_t *__restrict__ seg_off, int64_t n_segs_cap,
                              const int64_t *__restrict__ seg_q, const uint64_t *__restrict__ seg_err, pcabi_qual_read *__restrict__ out) {
    const int64_t ri = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ri >= n_reads) return;
    pcabi_qual_read r = out[ri];
    const int64_t s1 = std::min(seg_off[ri + 1], n_segs_cap);
    for (int64_t s = seg_off[ri]; s < s1; ++s) r.q_sum += seg_q[s], r.err_sum += seg_err[s];
    r.flags = flags_of(o, !(r.flags & PCABI_QUAL_NO_QUALITIES), r.kept, r.err_sum);
    out[ri] = r;
}

KernelTimes g_times;   // 0 k_qual_crop, 1 k_qual_sum (tools/qual_timing.py)
std::atomic<int64_t> g_host_ns{0};   // wall time of the host build
std::atomic<int64_t> g_dev_ns{0};    // wall time of the device stage behind the uploads

constexpr int64_t kAlign = 256;
int64_t aligned(int64_t n) { return (n + kAlign - 1) / kAlign * kAlign; }

int check_opts(const pcabi_qual_opts *o) {
    if (!o) return fail(PCABI_E_ARG, "bad arguments");
    if (o->window < 0 || o->window > kMaxWindow) return fail(PCABI_E_ARG, "window is 0 (off) or 1..64");
    if (o->max_mean_err > kErrOne) return fail(PCABI_E_ARG, "max_mean_err is at most 2^32");
    return 0;
}

int scan_tmp_bytes(int64_t n_reads, size_t *tmp) {
    *tmp = 0;
    PCABI_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, *tmp, (int64_t *)nullptr, (int64_t *)nullptr, (int)(n_reads + 1), (hipStream_t) nullptr));
    return 0;
}

// The stage queued on `st`; spans (two, or null): events around the two kernels, switched by `times`. The
// spans are reads to the whole-read stage and pieces to the piece stage: the kernels do not care.
int qual_run(const uint8_t *qual, int64_t qual_n, const int64_t *span_off, const int32_t *span_len, int64_t n_reads, int64_t n_segs_cap,
             const pcabi_qual_opts &o, pcabi_qual_read *out, void *scratch, int64_t scratch_len, hipStream_t st, EventSpan *spans,
             KernelTimes &times = g_times) {
    if (n_reads <= 0) return 0;
    size_t tmp = 0;
    if (int rc = scan_tmp_bytes(n_reads, &tmp)) return rc;
    const int64_t need = pcabi_qual_scratch_bytes(n_reads, n_segs_cap);
    if (need < 0) return (int)need;
    if (!scratch || scratch_len < need || ((uintptr_t)scratch & 15u)) return fail(PCABI_E_ARG, "the scratch buffer is too small or not 16-aligned");
    uint8_t *p = (uint8_t *)scratch;
    int64_t *nseg = (int64_t *)p;
    p += aligned((n_reads + 1) * 8);
    int64_t *seg_off = (int64_t *)p;
    p += aligned((n_reads + 1) * 8);
    int64_t *seg_q = (int64_t *)p;
    p += aligned(n_segs_cap * 8);
    uint64_t *seg_err = (uint64_t *)p;
    p += aligned(n_segs_cap * 8);
    if (spans) spans[0].begin(times, st);
    hipLaunchKernelGGL(k_qual_crop, dim3((unsigned)n_reads), dim3(kWave), 0, st, qual, qual_n, span_off, span_len, n_reads, o, out, nseg);
    PCABI_TRY(hipGetLastError());
    if (spans) spans[0].end(st);
    PCABI_TRY(hipcub::DeviceScan::ExclusiveSum(p, tmp, nseg, seg_off, (int)(n_reads + 1), st));
    if (n_segs_cap > 0) {
        if (spans) spans[1].begin(times, st);
        hipLaunchKernelGGL(k_qual_sum, dim3((unsigned)n_segs_cap), dim3(kWave), 0, st, qual, span_off, n_reads, out, seg_off, n_segs_cap, seg_q,
                           seg_err);
        PCABI_TRY(hipGetLastError());
        if (spans) spans[1].end(st);
    }
    hipLaunchKernelGGL(k_qual_finish, dim3((unsigned)((n_reads + 255) / 256)), dim3(256), 0, st, n_reads, o, seg_off, n_segs_cap, seg_q, seg_err,
                       out);
    PCABI_TRY(hipGetLastError());
    return 0;
}

// The host build: reads by threads; a read's kept span is summed in one piece (sum_lane as one lane).
void filter_host(const uint8_t *qual, const int64_t *span_off, const int32_t *span_len, int64_t n_reads, const pcabi_qual_opts &o,
                 pcabi_qual_read *out, bool timed = true) {
    const int nt = (int)std::min<int64_t>(io_thread_count(), std::max<int64_t>(1, n_reads / 64));
    const double t_begin = now_s();
    auto work = [&](int t) {
        for (int64_t i = n_reads * t / nt; i < n_reads * (t + 1) / nt; ++i) {
            const int64_t off = span_off[i], n = span_len[i];
            pcabi_qual_read r;
            r.front = r.tail = 0, r.kept = (int32_t)n, r.flags = 0, r.q_sum = 0, r.err_sum = 0;
            if (crop_on(o, off)) {
                const int64_t vf = scan_host(qual + off, n, o.window, o.min_window_sum, false);
                crop_of(n, vf, vf < 0 ? 0 : scan_host(qual + off, n, o.window, o.min_window_sum, true), &r);
            }
            if (off >= 0) sum_lane(qual, off + r.front, off + r.front + r.kept, 0, 1, err_of, &r.q_sum, &r.err_sum);
            r.flags = flags_of(o, off >= 0, r.kept, r.err_sum);
            out[i] = r;
        }
    };
    if (nt <= 1) {
        work(0);
    } else {
        std::vector<std::thread> th;
        for (int t = 0; t < nt; ++t) th.emplace_back(work, t);
        for (auto &x : th) x.join();
    }
    if (timed) g_host_ns += (int64_t)((now_s() - t_begin) * 1e9);
}

// ---- the piece stage: split reads judged piece by piece (pcabi_pieces.h; include/pcabi.h pcabi_qual_pieces_*) ----
// k_piece_keys: one thread per range: its read (a binary search of cut_off) and its begin, clamped to
//   [0, tl], as one 64-bit key; hipcub's radix sort of (key, range index) puts every read's ranges in
//   ascending begin, however many it has.
// k_piece_count: one thread per read walks its sorted ranges (pcabi_pieces::walk) and counts its pieces; an
//   exclusive device scan of the counts is piece_off.
// k_piece_spans: the same walk writes the pieces (read, begin, end) and their spans of the quality blob; the
//   slots between the device's count and the host's bound become spans without qualities of length 0, so
//   the crop, sum and finish kernels run over the bound with nothing read back.
// k_piece_cuts: one thread per read writes cut_off' and cuts' (the read's ranges as they came, then two
//   ranges a piece, pcabi_pieces::piece_ranges) and the pieces' records.
// Every write is guarded by the capacity the host passed.
static_assert(sizeof(pcabi_qual_piece) == 56, "pcabi_qual_piece is 56 bytes");

__global__ __launch_bounds__(256) void k_piece_keys(const int64_t *__restrict__ cut_off, const int64_t *__restrict__ cuts,
                                                    const int32_t *__restrict__ span_len, int64_t n_reads, int64_t n_ranges,
                                                    uint64_t *__restrict__ key, uint32_t *__restrict__ idx) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_ranges) return;
    int64_t r = owner_of(cut_off, n_reads + 1, k);
    if (r >= n_reads) r = n_reads - 1;
    const int64_t tl = std::max<int64_t>(span_len[r], 0);
    key[k] = ((uint64_t)r << 32) | (uint64_t)pcabi_pieces::sort_key(cuts[2 * k], tl);
    idx[k] = (uint32_t)k;
}

// read r's walk over its sorted ranges
template <class Piece>
__device__ inline int64_t walk_read(int64_t r, const int64_t *cut_off, const int64_t *cuts, int64_t n_ranges, const uint32_t *order,
                                    const int32_t *span_len, Piece &&piece) {
    const int64_t k0 = cut_off[r], k1 = std::min(cut_off[r + 1], n_ranges);
    return pcabi_pieces::walk(
        span_len[r], k1 - k0,
        [&](int64_t j, int64_t *b, int64_t *e) {
            const int64_t k = order[k0 + j];
            *b = cuts[2 * k], *e = cuts[2 * k + 1];
        },
        piece);
}

__global__ __launch_bounds__(256) void k_piece_count(const int64_t *__restrict__ cut_off, const int64_t *__restrict__ cuts, int64_t n_ranges,
                                                     const uint32_t *__restrict__ order, const int32_t *__restrict__ span_len,
                                                     int64_t n_reads, int64_t *__restrict__ cnt) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_reads) return;
    cnt[r] = walk_read(r, cut_off, cuts, n_ranges, order, span_len, [](int64_t, int64_t, int64_t) {});
    if (r == 0) cnt[n_reads] = 0;
}

__global__ __launch_bounds__(256) void k_piece_spans(const int64_t *__restrict__ cut_off, const int64_t *__restrict__ cuts, int64_t n_ranges,
                                                     const uint32_t *__restrict__ order, const int64_t *__restrict__ span_off,
                                                     const int32_t *__restrict__ span_len, int64_t n_reads,
                                                     const int64_t *__restrict__ piece_off, int64_t piece_cap,
                                                     pcabi_qual_piece *__restrict__ pieces, int64_t *__restrict__ pspan_off,
                                                     int32_t *__restrict__ pspan_len) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_reads) {
        const int64_t p0 = piece_off[i], off = span_off[i];
        walk_read(i, cut_off, cuts, n_ranges, order, span_len, [&](int64_t j, int64_t b, int64_t e) {
            const int64_t p = p0 + j;
            if (p >= piece_cap) return;
            pieces[p].read = i, pieces[p].begin = b, pieces[p].end = e;
            pspan_off[p] = off < 0 ? off : off + b;
            pspan_len[p] = (int32_t)(e - b);
        });
    }
    if (i < piece_cap && i >= piece_off[n_reads]) {   // surplus
        pieces[i].read = -1, pieces[i].begin = 0, pieces[i].end = 0;
        pspan_off[i] = -1, pspan_len[i] = 0;
    }
}

__global__ __launch_bounds__(256) void k_piece_cuts(const int64_t *__restrict__ cut_off, const int64_t *__restrict__ cuts, int64_t n_ranges,
                                                    int64_t n_reads, const int64_t *__restrict__ piece_off, int64_t piece_cap,
                                                    const pcabi_qual_read *__restrict__ precs, pcabi_qual_piece *__restrict__ pieces,
                                                    int64_t *__restrict__ cut_off_out, int64_t *__restrict__ cuts_out, int64_t cuts_cap) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_reads) return;
    if (r == 0) cut_off_out[n_reads] = cut_off[n_reads] + 2 * piece_off[n_reads];
    int64_t at = cut_off[r] + 2 * piece_off[r];
    cut_off_out[r] = at;
    for (int64_t k = cut_off[r]; k < std::min(cut_off[r + 1], n_ranges); ++k, ++at)
        if (at < cuts_cap) cuts_out[2 * at] = cuts[2 * k], cuts_out[2 * at + 1] = cuts[2 * k + 1];
    for (int64_t p = piece_off[r]; p < std::min(piece_off[r + 1], piece_cap); ++p, at += 2) {
        const pcabi_qual_read q = precs[p];
        pieces[p].q = q;
        int64_t rg[4];
        pcabi_pieces::piece_ranges(pieces[p].begin, pieces[p].end, q.front, q.tail, (q.flags & kFail) != 0, rg);
        if (at + 1 < cuts_cap) cuts_out[2 * at] = rg[0], cuts_out[2 * at + 1] = rg[1], cuts_out[2 * at + 2] = rg[2], cuts_out[2 * at + 3] = rg[3];
    }
}

KernelTimes g_ptimes_plan;   // 0 the plan kernels (keys, sort, count, scan, spans), 1 k_piece_cuts
KernelTimes g_ptimes_qual;   // 0 k_qual_crop, 1 k_qual_sum over the piece spans
std::atomic<int64_t> g_phost_ns{0};   // wall time of the piece stage's host build
std::atomic<int64_t> g_pdev_ns{0};    // wall time of the device piece stage behind the uploads

int piece_tmp_bytes(int64_t n_reads, int64_t n_ranges, size_t *tmp) {
    size_t a = 0, b = 0;
    PCABI_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, a, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                                 (int)std::max<int64_t>(n_ranges, 1), 0, 64, (hipStream_t) nullptr));
    PCABI_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, b, (int64_t *)nullptr, (int64_t *)nullptr, (int)(n_reads + 1), (hipStream_t) nullptr));
    *tmp = std::max(a, b);
    return 0;
}

bool piece_sizes_ok(int64_t n_reads, int64_t n_ranges, int64_t piece_cap, int64_t seg_cap) {
    return n_reads >= 0 && n_ranges >= 0 && piece_cap >= 0 && seg_cap >= 0 && n_reads < INT32_MAX - 1 && n_ranges < INT32_MAX / 4 &&
           piece_cap < INT32_MAX / 4 && seg_cap < INT32_MAX;
}

// The piece stage queued on `st`; spans (four, or null): events around the plan, the piece crop, the piece
// sum and k_piece_cuts.
int pieces_run(const uint8_t *qual, int64_t qual_n, const int64_t *span_off, const int32_t *span_len, int64_t n_reads, const int64_t *cut_off,
               const int64_t *cuts, int64_t n_ranges, int64_t piece_cap, int64_t seg_cap, const pcabi_qual_opts &o, int64_t *piece_off,
               pcabi_qual_piece *pieces, int64_t *cut_off_out, int64_t *cuts_out, int64_t cuts_cap, void *scratch, int64_t scratch_len,
               hipStream_t st, EventSpan *spans) {
    if (n_reads <= 0) {
        PCABI_TRY(hipMemsetAsync(piece_off, 0, 8, st));
        PCABI_TRY(hipMemsetAsync(cut_off_out, 0, 8, st));
        return 0;
    }
    const int64_t need = pcabi_qual_pieces_scratch_bytes(n_reads, n_ranges, piece_cap, seg_cap);
    if (need < 0) return (int)need;
    if (!scratch || scratch_len < need || ((uintptr_t)scratch & 15u)) return fail(PCABI_E_ARG, "the scratch buffer is too small or not 16-aligned");
    size_t tmp = 0;
    if (int rc = piece_tmp_bytes(n_reads, n_ranges, &tmp)) return rc;
    const int64_t inner = pcabi_qual_scratch_bytes(piece_cap, seg_cap);
    if (inner < 0) return (int)inner;
    uint8_t *p = (uint8_t *)scratch;
    auto take = [&](int64_t bytes) {
        uint8_t *q = p;
        p += aligned(bytes);
        return q;
    };
    uint64_t *key = (uint64_t *)take(n_ranges * 8), *key2 = (uint64_t *)take(n_ranges * 8);
    uint32_t *idx = (uint32_t *)take(n_ranges * 4), *order = (uint32_t *)take(n_ranges * 4);
    int64_t *cnt = (int64_t *)take((n_reads + 1) * 8);
    int64_t *pspan_off = (int64_t *)take(piece_cap * 8);
    int32_t *pspan_len = (int32_t *)take(piece_cap * 4);
    pcabi_qual_read *precs = (pcabi_qual_read *)take(piece_cap * (int64_t)sizeof(pcabi_qual_read));
    void *t = take((int64_t)tmp + 1);
    void *inner_scratch = take(inner);
    const unsigned g_reads = (unsigned)((n_reads + 255) / 256);
    if (spans) spans[0].begin(g_ptimes_plan, st);
    if (n_ranges > 0) {
        hipLaunchKernelGGL(k_piece_keys, dim3((unsigned)((n_ranges + 255) / 256)), dim3(256), 0, st, cut_off, cuts, span_len, n_reads, n_ranges,
                           key, idx);
        PCABI_TRY(hipGetLastError());
        int end_bit = 33;   // the begin's 31 bits, then the read's
        while (end_bit < 64 && ((int64_t)1 << (end_bit - 32)) <= n_reads) ++end_bit;
        size_t ts = tmp;
        PCABI_TRY(hipcub::DeviceRadixSort::SortPairs(t, ts, key, key2, idx, order, (int)n_ranges, 0, end_bit, st));
    }
    hipLaunchKernelGGL(k_piece_count, dim3(g_reads), dim3(256), 0, st, cut_off, cuts, n_ranges, order, span_len, n_reads, cnt);
    PCABI_TRY(hipGetLastError());
    size_t ts = tmp;
    PCABI_TRY(hipcub::DeviceScan::ExclusiveSum(t, ts, cnt, piece_off, (int)(n_reads + 1), st));
    hipLaunchKernelGGL(k_piece_spans, dim3((unsigned)((std::max(n_reads, piece_cap) + 255) / 256)), dim3(256), 0, st, cut_off, cuts, n_ranges,
                       order, span_off, span_len, n_reads, piece_off, piece_cap, pieces, pspan_off, pspan_len);
    PCABI_TRY(hipGetLastError());
    if (spans) spans[0].end(st);
    if (int rc = qual_run(qual, qual_n, pspan_off, pspan_len, piece_cap, seg_cap, o, precs, inner_scratch, inner, st, spans ? spans + 1 : nullptr,
                          g_ptimes_qual))
        return rc;
    if (spans) spans[3].begin(g_ptimes_plan, st);
    hipLaunchKernelGGL(k_piece_cuts, dim3(g_reads), dim3(256), 0, st, cut_off, cuts, n_ranges, n_reads, piece_off, piece_cap, precs, pieces,
                       cut_off_out, cuts_out, cuts_cap);
    PCABI_TRY(hipGetLastError());
    if (spans) spans[3].end(st);
    return 0;
}

// The host build: a read's ranges sorted by (key, index), the same walk and the cut layout on the calling
// thread; only filter_host over the piece spans fans out to the io threads.
void pieces_host(const uint8_t *qual, const int64_t *span_off, const int32_t *span_len, int64_t n_reads, const int64_t *cut_off,
                 const int64_t *cuts, const pcabi_qual_opts &o, int64_t *piece_off, pcabi_qual_piece *pieces, int64_t *cut_off_out,
                 int64_t *cuts_out) {
    const double t_begin = now_s();
    std::vector<std::pair<int64_t, int64_t>> order;
    std::vector<int64_t> pspan_off;
    std::vector<int32_t> pspan_len;
    int64_t np = 0;
    for (int64_t r = 0; r < n_reads; ++r) {
        piece_off[r] = np;
        const int64_t k0 = cut_off[r], m = cut_off[r + 1] - k0, tl = std::max<int64_t>(span_len[r], 0);
        order.clear();
        for (int64_t k = k0; k < k0 + m; ++k) order.emplace_back(pcabi_pieces::sort_key(cuts[2 * k], tl), k);
        std::sort(order.begin(), order.end());
        np += pcabi_pieces::walk(
            tl, m,
            [&](int64_t j, int64_t *b, int64_t *e) {
                const int64_t k = order[(size_t)j].second;
                *b = cuts[2 * k], *e = cuts[2 * k + 1];
            },
            [&](int64_t j, int64_t b, int64_t e) {
                pcabi_qual_piece &pc = pieces[piece_off[r] + j];
                pc.read = r, pc.begin = b, pc.end = e;
                pspan_off.push_back(span_off[r] < 0 ? span_off[r] : span_off[r] + b);
                pspan_len.push_back((int32_t)(e - b));
            });
    }
    piece_off[n_reads] = np;
    std::vector<pcabi_qual_read> precs((size_t)np);
    if (np) filter_host(qual, pspan_off.data(), pspan_len.data(), np, o, precs.data(), false);
    for (int64_t r = 0; r < n_reads; ++r) {
        int64_t at = cut_off[r] + 2 * piece_off[r];
        cut_off_out[r] = at;
        for (int64_t k = cut_off[r]; k < cut_off[r + 1]; ++k, ++at) cuts_out[2 * at] = cuts[2 * k], cuts_out[2 * at + 1] = cuts[2 * k + 1];
        for (int64_t p = piece_off[r]; p < piece_off[r + 1]; ++p, at += 2) {
            const pcabi_qual_read &q = pieces[p].q = precs[(size_t)p];
            pcabi_pieces::piece_ranges(pieces[p].begin, pieces[p].end, q.front, q.tail, (q.flags & kFail) != 0, cuts_out + 2 * at);
        }
    }
    cut_off_out[n_reads] = cut_off[n_reads] + 2 * np;
    g_phost_ns += (int64_t)((now_s() - t_begin) * 1e9);
}

}  // namespace

extern "C" {

int64_t pcabi_qual_seg_bound(const int32_t *span_len, int64_t n_reads) {
    int64_t s = 0;
    for (int64_t i = 0; i < n_reads; ++i) s += n_segs(std::max<int64_t>(span_len[i], 0));
    return s;
}

int64_t pcabi_qual_scratch_bytes(int64_t n_reads, int64_t n_segs_cap) {
    if (n_reads < 0 || n_segs_cap < 0 || n_reads >= INT32_MAX - 1 || n_segs_cap >= INT32_MAX)
        return fail(PCABI_E_ARG, "too many reads or segments for one launch");
    size_t tmp = 0;
    if (int rc = scan_tmp_bytes(n_reads, &tmp)) return rc;
    return 2 * aligned((n_reads + 1) * 8) + 2 * aligned(n_segs_cap * 8) + aligned((int64_t)tmp + 1);
}

int pcabi_qual_filter_dev(const uint8_t *qual, int64_t qual_n, const int64_t *span_off, const int32_t *span_len, int64_t n_reads,
                          int64_t n_segs_cap, const pcabi_qual_opts *opts, pcabi_qual_read *out, void *scratch, int64_t scratch_len,
                          void *stream) {
    if (int rc = check_opts(opts)) return rc;
    if (qual_n < 0 || n_reads < 0 || n_segs_cap < 0 || (n_reads > 0 && (!span_off || !span_len || !out)) || (qual_n > 0 && !qual))
        return fail(PCABI_E_ARG, "bad arguments");
    if (qual_n > kMaxBlob) return fail(PCABI_E_ARG, "a batch holds at most 2^31 quality bytes");
    return qual_run(qual, qual_n, span_off, span_len, n_reads, n_segs_cap, *opts, out, scratch, scratch_len, (hipStream_t)stream, nullptr);
}

int pcabi_qual_filter_host(int device, const uint8_t *qual, int64_t qual_n, const int64_t *span_off, const int32_t *span_len, int64_t n_reads,
                           const pcabi_qual_opts *opts, pcabi_qual_read *out) {
    if (int rc = check_opts(opts)) return rc;
    if (qual_n < 0 || n_reads < 0 || (n_reads > 0 && (!span_off || !span_len || !out)) || (qual_n > 0 && !qual))
        return fail(PCABI_E_ARG, "bad arguments");
    if (qual_n > kMaxBlob) return fail(PCABI_E_ARG, "a batch holds at most 2^31 quality bytes");
    if (n_reads >= INT32_MAX - 1) return fail(PCABI_E_ARG, "too many reads for one launch");
    for (int64_t i = 0; i < n_reads; ++i)
        if (!span_fits(span_off[i], span_len[i], qual_n))
            return fail(PCABI_E_ARG, "the span of read " + std::to_string(i) + " lies outside the quality blob");
    if (n_reads == 0) return 0;
    if (device < 0) {
        filter_host(qual, span_off, span_len, n_reads, *opts, out);
        return 0;
    }
    PCABI_TRY(hipSetDevice(device));
    const int64_t cap = pcabi_qual_seg_bound(span_len, n_reads);
    const int64_t scratch_len = pcabi_qual_scratch_bytes(n_reads, cap);
    if (scratch_len < 0) return (int)scratch_len;
    DevBuf<> d_qual, d_scratch;
    DevBuf<int64_t> d_off;
    DevBuf<int32_t> d_len;
    DevBuf<pcabi_qual_read> d_out;
    if (int rc = d_qual.reserve(qual_n + 16, qual_n + 16)) return rc;
    if (int rc = d_scratch.reserve(scratch_len, scratch_len)) return rc;
    if (int rc = d_off.reserve(n_reads, n_reads)) return rc;
    if (int rc = d_len.reserve(n_reads, n_reads)) return rc;
    if (int rc = d_out.reserve(n_reads, n_reads)) return rc;
    if (qual_n > 0) PCABI_TRY(hipMemcpy(d_qual, qual, (size_t)qual_n, hipMemcpyHostToDevice));
    PCABI_TRY(hipMemcpy(d_off, span_off, (size_t)n_reads * 8, hipMemcpyHostToDevice));
    PCABI_TRY(hipMemcpy(d_len, span_len, (size_t)n_reads * 4, hipMemcpyHostToDevice));
    PCABI_TRY(hipDeviceSynchronize());
    const double t_begin = now_s();
    EventSpan spans[2];
    const int rc = qual_run(d_qual, qual_n, d_off, d_len, n_reads, cap, *opts, d_out, d_scratch, scratch_len, nullptr, spans);
    const hipError_t e = hipStreamSynchronize(nullptr);
    int64_t span_bytes = 0;
    for (int64_t i = 0; i < n_reads; ++i) span_bytes += span_off[i] >= 0 ? span_len[i] : 0;
    spans[0].harvest(g_times, 0, span_bytes);
    spans[1].harvest(g_times, 1, span_bytes);
    if (rc) return rc;
    PCABI_TRY(e);
    PCABI_TRY(hipMemcpy(out, d_out, (size_t)n_reads * sizeof(pcabi_qual_read), hipMemcpyDeviceToHost));
    g_dev_ns += (int64_t)((now_s() - t_begin) * 1e9);
    return 0;
}

int pcabi_qual_pieces_bound(const int32_t *span_len, const int64_t *cut_off, int64_t n_reads, int64_t *n_pieces, int64_t *n_segs_out) {
    if (n_reads < 0 || (n_reads > 0 && (!span_len || !cut_off))) return fail(PCABI_E_ARG, "bad arguments");
    int64_t pieces = 0, segs = 0;
    for (int64_t r = 0; r < n_reads; ++r) {
        const int64_t m = cut_off[r + 1] - cut_off[r];
        if (m < 0) return fail(PCABI_E_ARG, "cut_off descends at read " + std::to_string(r));
        if (m == 0) continue;
        pieces += m + 1;
        segs += n_segs(std::max<int64_t>(span_len[r], 0));
    }
    if (n_pieces) *n_pieces = pieces;
    if (n_segs_out) *n_segs_out = segs + pieces;
    return 0;
}

int64_t pcabi_qual_pieces_scratch_bytes(int64_t n_reads, int64_t n_ranges, int64_t piece_cap, int64_t seg_cap) {
    if (!piece_sizes_ok(n_reads, n_ranges, piece_cap, seg_cap)) return fail(PCABI_E_ARG, "too many reads, ranges, pieces or segments for one launch");
    size_t tmp = 0;
    if (int rc = piece_tmp_bytes(n_reads, n_ranges, &tmp)) return rc;
    const int64_t inner = pcabi_qual_scratch_bytes(piece_cap, seg_cap);
    if (inner < 0) return inner;
    return 2 * aligned(n_ranges * 8) + 2 * aligned(n_ranges * 4) + aligned((n_reads + 1) * 8) + aligned(piece_cap * 8) + aligned(piece_cap * 4) +
           aligned(piece_cap * (int64_t)sizeof(pcabi_qual_read)) + aligned((int64_t)tmp + 1) + aligned(inner);
}

static int pieces_check(const pcabi_qual_opts *opts, const uint8_t *qual, int64_t qual_n, const int64_t *span_off, const int32_t *span_len,
                        int64_t n_reads, const int64_t *cut_off, const int64_t *cuts, int64_t n_ranges, int64_t piece_cap, int64_t seg_cap,
                        const int64_t *piece_off, const pcabi_qual_piece *pieces, const int64_t *cut_off_out, const int64_t *cuts_out,
                        int64_t cuts_cap) {
    if (int rc = check_opts(opts)) return rc;
    if (qual_n < 0 || n_reads < 0 || n_ranges < 0 || piece_cap < 0 || seg_cap < 0 || cuts_cap < 0 || !cut_off || !piece_off || !cut_off_out ||
        (n_reads > 0 && (!span_off || !span_len)) || (qual_n > 0 && !qual) || (n_ranges > 0 && !cuts) || (piece_cap > 0 && !pieces) ||
        (cuts_cap > 0 && !cuts_out))
        return fail(PCABI_E_ARG, "bad arguments");
    if (qual_n > kMaxBlob) return fail(PCABI_E_ARG, "a batch holds at most 2^31 quality bytes");
    if (!piece_sizes_ok(n_reads, n_ranges, piece_cap, seg_cap)) return fail(PCABI_E_ARG, "too many reads, ranges, pieces or segments for one launch");
    // every read with ranges may give one piece more than it has ranges
    if (piece_cap < n_ranges + (n_ranges > 0)) return fail(PCABI_E_ARG, "piece_cap is below the bound of pcabi_qual_pieces_bound");
    if (cuts_cap < n_ranges + 2 * piece_cap) return fail(PCABI_E_ARG, "cuts_out holds fewer than n_ranges + 2 * piece_cap ranges");
    return 0;
}

int pcabi_qual_pieces_dev(const uint8_t *qual, int64_t qual_n, const int64_t *span_off, const int32_t *span_len, int64_t n_reads,
                          const int64_t *cut_off, const int64_t *cuts, int64_t n_ranges, int64_t piece_cap, int64_t seg_cap,
                          const pcabi_qual_opts *opts, int64_t *piece_off, pcabi_qual_piece *pieces, int64_t *cut_off_out, int64_t *cuts_out,
                          int64_t cuts_cap, void *scratch, int64_t scratch_len, void *stream) {
    if (int rc = pieces_check(opts, qual, qual_n, span_off, span_len, n_reads, cut_off, cuts, n_ranges, piece_cap, seg_cap, piece_off, pieces,
                              cut_off_out, cuts_out, cuts_cap))
        return rc;
    return pieces_run(qual, qual_n, span_off, span_len, n_reads, cut_off, cuts, n_ranges, piece_cap, seg_cap, *opts, piece_off, pieces,
                      cut_off_out, cuts_out, cuts_cap, scratch, scratch_len, (hipStream_t)stream, nullptr);
}

int pcabi_qual_pieces_host(int device, const uint8_t *qual, int64_t qual_n, const int64_t *span_off, const int32_t *span_len, int64_t n_reads,
                           const int64_t *cut_off, const int64_t *cuts, const pcabi_qual_opts *opts, int64_t *piece_off,
                           pcabi_qual_piece *pieces, int64_t piece_cap, int64_t *cut_off_out, int64_t *cuts_out, int64_t cuts_cap) {
    if (int rc = check_opts(opts)) return rc;
    if (n_reads < 0 || !cut_off || (n_reads > 0 && (!span_off || !span_len))) return fail(PCABI_E_ARG, "bad arguments");
    if (cut_off[0] != 0) return fail(PCABI_E_ARG, "cut_off begins at 0");
    int64_t bound = 0, seg_cap = 0;
    if (int rc = pcabi_qual_pieces_bound(span_len, cut_off, n_reads, &bound, &seg_cap)) return rc;
    const int64_t n_ranges = cut_off[n_reads];
    if (piece_cap < bound) return fail(PCABI_E_ARG, "piece_cap is below the bound of pcabi_qual_pieces_bound");
    if (int rc = pieces_check(opts, qual, qual_n, span_off, span_len, n_reads, cut_off, cuts, n_ranges, piece_cap, seg_cap, piece_off, pieces,
                              cut_off_out, cuts_out, cuts_cap))
        return rc;
    for (int64_t i = 0; i < n_reads; ++i)
        if (!span_fits(span_off[i], span_len[i], qual_n))
            return fail(PCABI_E_ARG, "the span of read " + std::to_string(i) + " lies outside the quality blob");
    if (device < 0) {
        pieces_host(qual, span_off, span_len, n_reads, cut_off, cuts, *opts, piece_off, pieces, cut_off_out, cuts_out);
        return 0;
    }
    PCABI_TRY(hipSetDevice(device));
    const int64_t scratch_len = pcabi_qual_pieces_scratch_bytes(n_reads, n_ranges, piece_cap, seg_cap);
    if (scratch_len < 0) return (int)scratch_len;
    DevBuf<> d_qual, d_scratch;
    DevBuf<int64_t> d_off, d_cut_off, d_cuts, d_piece_off, d_cut_off_out, d_cuts_out;
    DevBuf<int32_t> d_len;
    DevBuf<pcabi_qual_piece> d_pieces;
    if (int rc = d_qual.reserve(qual_n + 16, qual_n + 16)) return rc;
    if (int rc = d_scratch.reserve(scratch_len + 16, scratch_len + 16)) return rc;
    if (int rc = d_off.reserve(n_reads + 1, n_reads + 1)) return rc;
    if (int rc = d_len.reserve(n_reads + 1, n_reads + 1)) return rc;
    if (int rc = d_cut_off.reserve(n_reads + 1, n_reads + 1)) return rc;
    if (int rc = d_cuts.reserve(2 * n_ranges + 2, 2 * n_ranges + 2)) return rc;
    if (int rc = d_piece_off.reserve(n_reads + 1, n_reads + 1)) return rc;
    if (int rc = d_cut_off_out.reserve(n_reads + 1, n_reads + 1)) return rc;
    if (int rc = d_cuts_out.reserve(2 * cuts_cap + 2, 2 * cuts_cap + 2)) return rc;
    if (int rc = d_pieces.reserve(piece_cap + 1, piece_cap + 1)) return rc;
    if (qual_n > 0) PCABI_TRY(hipMemcpy(d_qual, qual, (size_t)qual_n, hipMemcpyHostToDevice));
    if (n_reads > 0) {
        PCABI_TRY(hipMemcpy(d_off, span_off, (size_t)n_reads * 8, hipMemcpyHostToDevice));
        PCABI_TRY(hipMemcpy(d_len, span_len, (size_t)n_reads * 4, hipMemcpyHostToDevice));
    }
    PCABI_TRY(hipMemcpy(d_cut_off, cut_off, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice));
    if (n_ranges > 0) PCABI_TRY(hipMemcpy(d_cuts, cuts, (size_t)n_ranges * 16, hipMemcpyHostToDevice));
    PCABI_TRY(hipDeviceSynchronize());
    const double t_begin = now_s();
    EventSpan spans[4];
    const int rc = pieces_run(d_qual, qual_n, d_off, d_len, n_reads, d_cut_off, d_cuts, n_ranges, piece_cap, seg_cap, *opts, d_piece_off, d_pieces,
                              d_cut_off_out, d_cuts_out, cuts_cap, d_scratch, scratch_len, nullptr, spans);
    const hipError_t e = hipStreamSynchronize(nullptr);
    int64_t span_bytes = 0;   // an upper bound of the pieces' bytes: the split reads' spans
    for (int64_t i = 0; i < n_reads; ++i) span_bytes += span_off[i] >= 0 && cut_off[i + 1] > cut_off[i] ? span_len[i] : 0;
    spans[0].harvest(g_ptimes_plan, 0, n_ranges * 16);
    spans[1].harvest(g_ptimes_qual, 0, span_bytes);
    spans[2].harvest(g_ptimes_qual, 1, span_bytes);
    spans[3].harvest(g_ptimes_plan, 1, (n_ranges + 2 * piece_cap) * 16);
    if (rc) return rc;
    PCABI_TRY(e);
    PCABI_TRY(hipMemcpy(piece_off, d_piece_off, (size_t)(n_reads + 1) * 8, hipMemcpyDeviceToHost));
    PCABI_TRY(hipMemcpy(cut_off_out, d_cut_off_out, (size_t)(n_reads + 1) * 8, hipMemcpyDeviceToHost));
    const int64_t np = piece_off[n_reads];
    if (np < 0 || np > piece_cap || cut_off_out[n_reads] != n_ranges + 2 * np) return fail(PCABI_E_DEVICE, "the piece stage's counts do not add up");
    if (np > 0) PCABI_TRY(hipMemcpy(pieces, d_pieces, (size_t)np * sizeof(pcabi_qual_piece), hipMemcpyDeviceToHost));
    if (n_ranges + 2 * np > 0) PCABI_TRY(hipMemcpy(cuts_out, d_cuts_out, (size_t)(n_ranges + 2 * np) * 16, hipMemcpyDeviceToHost));
    g_pdev_ns += (int64_t)((now_s() - t_begin) * 1e9);
    return 0;
}

void pcabi_qual_pieces_last_times(int on, int reset, double *ms, int64_t *bytes) {
    double a[2] = {0, 0}, b[2] = {0, 0};
    int64_t ab[2] = {0, 0}, bb[2] = {0, 0};
    g_ptimes_plan.last(on, reset, a, ab);
    g_ptimes_qual.last(on, reset, b, bb);
    if (ms) ms[0] = a[0], ms[1] = b[0], ms[2] = b[1], ms[3] = a[1], ms[4] = 1e-6 * (double)g_phost_ns.load(), ms[5] = 1e-6 * (double)g_pdev_ns.load();
    if (bytes) bytes[0] = ab[0], bytes[1] = bb[0], bytes[2] = bb[1], bytes[3] = ab[1];
    if (reset) g_phost_ns = 0, g_pdev_ns = 0;
}

void pcabi_qual_error_table(uint64_t *table) {
    for (int q = 0; q <= kMaxQ; ++q) table[q] = err_of(q);
}

void pcabi_qual_last_times(int on, int reset, double *ms, int64_t *bytes) {
    g_times.last(on, reset, ms, bytes);
    if (ms) ms[2] = 1e-6 * (double)g_host_ns.load(), ms[3] = 1e-6 * (double)g_dev_ns.load();
    if (reset) g_host_ns = 0, g_dev_ns = 0;
}

}  // extern "C"
