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

// The stage queued on `st`; spans (two, or null): events around the two kernels.
int qual_run(const uint8_t *qual, int64_t qual_n, const int64_t *span_off, const int32_t *span_len, int64_t n_reads, int64_t n_segs_cap,
             const pcabi_qual_opts &o, pcabi_qual_read *out, void *scratch, int64_t scratch_len, hipStream_t st, EventSpan *spans) {
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
    if (spans) spans[0].begin(g_times, st);
    hipLaunchKernelGGL(k_qual_crop, dim3((unsigned)n_reads), dim3(kWave), 0, st, qual, qual_n, span_off, span_len, n_reads, o, out, nseg);
    PCABI_TRY(hipGetLastError());
    if (spans) spans[0].end(st);
    PCABI_TRY(hipcub::DeviceScan::ExclusiveSum(p, tmp, nseg, seg_off, (int)(n_reads + 1), st));
    if (n_segs_cap > 0) {
        if (spans) spans[1].begin(g_times, st);
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
                 pcabi_qual_read *out) {
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
    g_host_ns += (int64_t)((now_s() - t_begin) * 1e9);
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

void pcabi_qual_error_table(uint64_t *table) {
    for (int q = 0; q <= kMaxQ; ++q) table[q] = err_of(q);
}

void pcabi_qual_last_times(int on, int reset, double *ms, int64_t *bytes) {
    g_times.last(on, reset, ms, bytes);
    if (ms) ms[2] = 1e-6 * (double)g_host_ns.load(), ms[3] = 1e-6 * (double)g_dev_ns.load();
    if (reset) g_host_ns = 0, g_dev_ns = 0;
}

}  // extern "C"
