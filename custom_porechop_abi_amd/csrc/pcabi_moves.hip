// pcabi_moves.hip -- move tables (mv) and their sample offset (ts) remapped onto parts of reads on the GPU
// (gfx950): include/pcabi.h pcabi_moves_*; DESIGN.md "BAM output"; the rule and every per-lane function are
// csrc/pcabi_moves.h's, the same the host build runs.
//
// The work is spread by bytes, not by reads: the moves of all reads are cut into segments of 4096, laid
// out flat (seg_off[read], from the host).
// k_moves_count: one wave per segment. A binary search of seg_off names the segment's read; the lanes
//   take the segment's 16-aligned 16-byte loads in turn (count_lane: the first and the last load of a
//   segment are masked to it, so any alignment of the tag in the blob is fine and nothing outside the
//   segment is read); a wave sum gives the segment's ones, a ballot whether all its dwords were valid.
// the scan: hipcub's exclusive device scan over the segments' values (+ 1 << 40 for an invalid one), with
//   one value more than there are segments, so that a read's ones and invalid segments are the difference
//   of two entries.
// k_moves_select: one wave per part boundary (two a part). select_seg searches the read's prefixes for
//   the segment that holds the wanted one (segments without a one fall out of the search); that segment
//   goes by 64 bytes a pass, one a lane: a ballot of `byte == 1`, its popcount against what is still to
//   skip, and is_kth() on the pass that holds it. q[2 * part + side] is the move's index.
// k_moves_size: one thread per read: usable or not (table_usable, ts_fits over its parts), then its
//   parts' lengths. lens (4 bytes a part) and the flags (1 a read) are all that goes back.
// k_moves_write: one wave per 4096 output bytes of a part (chunk0[part], from the host once the lengths
//   are known): copy_lane writes head, stride, slice (16-byte pieces, byte-wise head and tail) and ts.
// Every loop runs to a length the host passed and checked (check_tables). No atomics, no inline assembly.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/pcabi.h"
#include "pcabi_hostdev.h"
#include "pcabi_moves.h"

using namespace pcabi_internal;
using namespace pcabi_moves;

namespace {

constexpr int kWave = 64;

__device__ inline int64_t wave_sum(int64_t x) {
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) x += __shfl_xor((long long)x, d);
    return x;
}

// the last i in [0, n) with off[i] <= v (off ascending, off[0] <= v)
PCABI_HD inline int64_t owner_of(const int64_t *off, int64_t n, int64_t v) {
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(kWave) void k_moves_count(const uint8_t *__restrict__ tags, int64_t tags_n,
                                                       const pcabi_moves_read *__restrict__ reads, int64_t n_reads,
                                                       const int64_t *__restrict__ seg_off, int64_t n_segs_all,
                                                       int64_t *__restrict__ val) {
    const int64_t sg = blockIdx.x;
    if (sg >= n_segs_all) return;
    const int lane = threadIdx.x;
    const int64_t ri = owner_of(seg_off, n_reads + 1, sg);
    int64_t ones = 0;
    bool ok = false;
    if (ri < n_reads) {   // uniform
        const pcabi_moves_read r = reads[ri];
        const int64_t n = n_moves(r), k = sg - seg_off[ri];
        if (r.mv_off >= 0 && r.n_vals <= tags_n - r.mv_off && k * kSeg < n) {
            const int64_t a = moves_at(r) + k * kSeg, e = moves_at(r) + std::min(n, (k + 1) * kSeg);
            ok = count_lane(tags, a, e, lane, kWave, &ones);
        }
    }
    ones = wave_sum(ones);
    const bool all_ok = __ballot(!ok) == 0;
    if (lane == 0) val[sg] = seg_value(ones, all_ok);
}

__global__ __launch_bounds__(kWave) void k_moves_select(const uint8_t *__restrict__ tags, int64_t tags_n,
                                                        const pcabi_moves_read *__restrict__ reads, int64_t n_reads,
                                                        const pcabi_moves_part *__restrict__ parts, int64_t n_parts,
                                                        const int64_t *__restrict__ seg_off, const int64_t *__restrict__ pre,
                                                        int32_t *__restrict__ q) {
    const int64_t bi = blockIdx.x;
    if (bi >= 2 * n_parts) return;
    const int lane = threadIdx.x;
    const pcabi_moves_part p = parts[bi >> 1];
    if (p.read < 0 || p.read >= n_reads) return;   // uniform
    const pcabi_moves_read r = reads[p.read];
    const int64_t n = n_moves(r), k = edge_k(p, (int)(bi & 1));
    int64_t at = n;   // p(k) of a read with no more than k ones
    if (k < 0) {
        at = 0;
    } else if (r.mv_off >= 0 && r.n_vals <= tags_n - r.mv_off) {
        const int64_t s0 = seg_off[p.read], ns = seg_off[p.read + 1] - s0;
        int64_t before = 0;
        const int64_t sg = ns == n_segs(r) ? select_seg(pre + s0, ns, k, &before) : ns;
        if (sg < ns) {
            const int64_t a = moves_at(r) + sg * kSeg, e = moves_at(r) + std::min(n, (sg + 1) * kSeg);
            int64_t left = k - before;
            for (int64_t pos = a; pos < e; pos += kWave) {
                const uint64_t m = __ballot(pos + lane < e && tags[pos + lane] == 1);
                const int c = __popcll(m);
                if (left < c) {
                    const uint64_t hit = __ballot(is_kth(m, lane, left));
                    at = pos - moves_at(r) + (hit ? __ffsll((long long)hit) - 1 : 0);
                    break;
                }
                left -= c;
            }
        }
    }
    if (lane == 0) q[bi] = (int32_t)at;
}

__global__ void k_moves_size(const uint8_t *__restrict__ tags, int64_t tags_n, const pcabi_moves_read *__restrict__ reads,
                             int64_t n_reads, const pcabi_moves_part *__restrict__ parts, int64_t n_parts,
                             const int64_t *__restrict__ seg_off, const int64_t *__restrict__ pre, const int32_t *__restrict__ q,
                             int32_t *__restrict__ lens, uint8_t *__restrict__ usable) {
    const int64_t ri = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ri >= n_reads) return;
    const pcabi_moves_read r = reads[ri];
    bool ok = read_fits(r, tags_n, n_parts);
    int stride = 0;
    if (ok) {
        int64_t ones = 0, n_bad = 0;
        read_sums(pre[seg_off[ri]], pre[seg_off[ri + 1]], &ones, &n_bad);
        stride = stride_of(tags, r);
        ok = table_usable(r, stride, ones, n_bad);
        for (int64_t j = r.part0; ok && j < r.part0 + r.n_parts; ++j) ok = ts_fits(r, stride, q[2 * j]);
    }
    usable[ri] = ok ? 1 : 0;
    if (!ok) return;   // lens was cleared
    for (int64_t j = r.part0; j < r.part0 + r.n_parts; ++j) lens[j] = (int32_t)tag_len(r, q[2 * j], q[2 * j + 1]);
}

__global__ __launch_bounds__(kWave) void k_moves_write(const uint8_t *__restrict__ tags, int64_t tags_n,
                                                       const pcabi_moves_read *__restrict__ reads, int64_t n_reads,
                                                       const pcabi_moves_part *__restrict__ parts, int64_t n_parts,
                                                       const int64_t *__restrict__ chunk0, int64_t n_chunks,
                                                       const int32_t *__restrict__ q, const uint8_t *__restrict__ usable,
                                                       uint8_t *__restrict__ out, int64_t out_cap) {
    const int64_t ci = blockIdx.x;
    if (ci >= n_chunks) return;
    const int lane = threadIdx.x;
    const int64_t pi = owner_of(chunk0, n_parts + 1, ci);
    if (pi >= n_parts) return;   // uniform
    const pcabi_moves_part p = parts[pi];
    if (p.read < 0 || p.read >= n_reads || p.len <= 0 || p.out < 0 || p.len > out_cap - p.out || !usable[p.read]) return;
    const pcabi_moves_read r = reads[p.read];
    const int64_t q0 = q[2 * pi], q1 = q[2 * pi + 1], n = n_moves(r);
    // the plan's checks, again: this kernel takes them from memory
    if (r.mv_off < 0 || r.n_vals < 1 || r.n_vals > tags_n - r.mv_off || q0 < 0 || q0 > q1 || q1 > n || tag_len(r, q0, q1) != p.len) return;
    const int stride = stride_of(tags, r);
    const int64_t j0 = (ci - chunk0[pi]) * kChunk;
    copy_lane(out + p.out, tags + moves_at(r) + q0, q1 - q0, stride, ts_of(r, stride, q0), p.len, j0, j0 + kChunk, lane, kWave);
}

std::atomic<int64_t> g_remapped{0}, g_dropped{0};
std::atomic<int64_t> g_host_ns{0};   // wall time of the host build, for the timing tool
std::atomic<int64_t> g_dev_ns{0};    // wall time of the device sizing step

// The tables against the blob and each other (PCABI_E_ARG).
int check_tables(int64_t tags_n, const pcabi_moves_read *reads, int64_t n_reads, const pcabi_moves_part *parts, int64_t n_parts) {
    for (int64_t i = 0; i < n_reads; ++i) {
        const pcabi_moves_read &r = reads[i];
        if (!read_fits(r, tags_n, n_parts))
            return fail(PCABI_E_ARG, "read " + std::to_string(i) + " of the move table does not fit the buffers");
        for (int64_t j = r.part0; j < r.part0 + r.n_parts; ++j) {
            const pcabi_moves_part &p = parts[j];
            if (p.read != i || p.s0 < 0 || p.ns < 0 || (int64_t)p.s0 + p.ns > r.l_seq)
                return fail(PCABI_E_ARG, "part " + std::to_string(j) + " does not lie inside read " + std::to_string(i));
        }
    }
    for (int64_t j = 0; j < n_parts; ++j) {
        const pcabi_moves_part &p = parts[j];
        if (p.read < 0 || p.read >= n_reads || j < reads[p.read].part0 || j >= reads[p.read].part0 + reads[p.read].n_parts)
            return fail(PCABI_E_ARG, "part " + std::to_string(j) + " belongs to no read of the table");
    }
    return 0;
}

std::vector<int64_t> seg_offsets(const pcabi_moves_read *reads, int64_t n_reads) {
    std::vector<int64_t> off((size_t)n_reads + 1, 0);
    for (int64_t i = 0; i < n_reads; ++i) off[(size_t)i + 1] = off[(size_t)i] + n_segs(reads[i]);
    return off;
}

// a part's first chunk of kChunk output bytes
std::vector<int64_t> chunk_offsets(const pcabi_moves_part *parts, int64_t n_parts) {
    std::vector<int64_t> off((size_t)n_parts + 1, 0);
    for (int64_t j = 0; j < n_parts; ++j)
        off[(size_t)j + 1] = off[(size_t)j] + (std::max<int64_t>(parts[j].len, 0) + kChunk - 1) / kChunk;
    return off;
}

void count_reads(const uint8_t *usable, int64_t n_reads) {
    int64_t good = 0;
    for (int64_t i = 0; i < n_reads; ++i) good += usable[i] ? 1 : 0;
    g_remapped += good;
    g_dropped += n_reads - good;
}

}  // namespace

// What the host build's sizing pass leaves for its writing pass: every part boundary's move.
struct pcabi_internal::MovesHost {
    std::vector<int32_t> q;         // 2 a part
    std::vector<uint8_t> usable;    // 1 a read
};

namespace {

// The host build: reads by threads; per read the segments' counts (count_lane as one lane), their
// prefixes, select_seg and the byte-by-byte walk of the chosen segment. out == nullptr sizes (parts[].len,
// usable, *keep filled); else the parts' bytes are written from what *keep holds.
void plan_host(const uint8_t *tags, const pcabi_moves_read *reads, int64_t n_reads, pcabi_moves_part *parts, int64_t n_parts,
               uint8_t *usable, uint8_t *out, MovesHost *keep) {
    const int nt = (int)std::min<int64_t>(io_thread_count(), std::max<int64_t>(1, n_reads / 64));
    const double t_begin = now_s();
    if (!out) {
        keep->q.assign((size_t)n_parts * 2, 0);
        keep->usable.assign((size_t)n_reads, 0);
    }
    auto work = [&](int t) {
        std::vector<int64_t> pre;
        for (int64_t i = n_reads * t / nt; i < n_reads * (t + 1) / nt; ++i) {
            const pcabi_moves_read &r = reads[i];
            const int64_t n = n_moves(r), ns = n_segs(r);
            if (out) {
                if (!keep->usable[(size_t)i]) continue;
                const int stride = stride_of(tags, r);
                for (int64_t j = r.part0; j < r.part0 + r.n_parts; ++j) {
                    const int64_t q0 = keep->q[(size_t)(2 * j)], q1 = keep->q[(size_t)(2 * j + 1)];
                    if (parts[j].len > 0)
                        copy_lane(out + parts[j].out, tags + moves_at(r) + q0, q1 - q0, stride, ts_of(r, stride, q0), parts[j].len, 0,
                                  parts[j].len, 0, 1);
                }
                continue;
            }
            pre.assign((size_t)ns + 1, 0);
            for (int64_t k = 0; k < ns; ++k) {
                int64_t ones = 0;
                const bool ok = count_lane(tags, moves_at(r) + k * kSeg, moves_at(r) + std::min(n, (k + 1) * kSeg), 0, 1, &ones);
                pre[(size_t)k + 1] = pre[(size_t)k] + seg_value(ones, ok);
            }
            int64_t ones = 0, n_bad = 0;
            read_sums(pre[0], pre[(size_t)ns], &ones, &n_bad);
            const int stride = stride_of(tags, r);
            bool ok = table_usable(r, stride, ones, n_bad);
            for (int64_t j = r.part0; j < r.part0 + r.n_parts; ++j)
                for (int side = 0; side < 2; ++side) {
                    const int64_t k = edge_k(parts[j], side);
                    int64_t at = n, before = 0;
                    if (k < 0) {
                        at = 0;
                    } else {
                        const int64_t sg = select_seg(pre.data(), ns, k, &before);
                        if (sg < ns) {
                            const int64_t a = moves_at(r) + sg * kSeg;
                            const int64_t w = select_walk(tags, a, moves_at(r) + std::min(n, (sg + 1) * kSeg), k - before);
                            if (w >= 0) at = sg * kSeg + w;
                        }
                    }
                    keep->q[(size_t)(2 * j + side)] = (int32_t)at;
                    if (side == 0) ok = ok && ts_fits(r, stride, at);
                }
            keep->usable[(size_t)i] = ok ? 1 : 0;
            if (usable) usable[i] = ok ? 1 : 0;
            if (ok)
                for (int64_t j = r.part0; j < r.part0 + r.n_parts; ++j)
                    parts[j].len = (int32_t)tag_len(r, keep->q[(size_t)(2 * j)], keep->q[(size_t)(2 * j + 1)]);
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

namespace pcabi_internal {

struct MovesDev {
    DevBuf<> tags;
    DevBuf<pcabi_moves_read> reads;
    DevBuf<pcabi_moves_part> parts;
    DevBuf<int64_t> seg_off, val, pre, chunk0;
    DevBuf<int32_t> q, lens;
    DevBuf<> usable, scan_tmp;
    std::vector<int32_t> h_lens;    // what comes back of the sizing step
    std::vector<uint8_t> h_usable;
    std::vector<int64_t> h_seg_off, h_chunk0;   // the sources of asynchronous copies: they live as long as the stream may read them
    int64_t n_reads = 0, n_parts = 0, tags_n = 0;   // what the plan before left there
    double t_begin = 0;
};

int64_t moves_host_ns(int reset, int64_t *dev_plan_ns) {
    const int64_t v = g_host_ns.load();
    *dev_plan_ns = g_dev_ns.load();
    if (reset) g_host_ns = 0, g_dev_ns = 0;
    return v;
}

MovesDev *moves_dev_new() { return new MovesDev; }
void moves_dev_free(MovesDev *d) { delete d; }
MovesHost *moves_host_new() { return new MovesHost; }
void moves_host_free(MovesHost *h) { delete h; }

int moves_check(const MovesTables &t) { return check_tables(t.tags_n, t.reads, t.n_reads, t.parts, t.n_parts); }

int moves_plan_host(MovesHost *keep, const MovesTables &t) {
    if (int rc = moves_check(t)) return rc;
    for (int64_t j = 0; j < t.n_parts; ++j) t.parts[j].len = 0;
    plan_host(t.tags, t.reads, t.n_reads, t.parts, t.n_parts, t.usable, nullptr, keep);
    count_reads(t.usable, t.n_reads);
    return 0;
}

void moves_write_host(MovesHost *keep, const MovesTables &t, uint8_t *out) {
    plan_host(t.tags, t.reads, t.n_reads, t.parts, t.n_parts, nullptr, out, keep);
}

// The device half, first step: the tag blob and the tables go up, the three sizing stages are queued on
// `stream` and the parts' lengths and the reads' flags are on their way back. The tables were checked
// (moves_check). Does not synchronise: moves_dev_plan_end does, so that whoever sizes other tags on the
// same stream in between shares the round trip.
int moves_dev_plan_begin(MovesDev *d, void *stream, const MovesTables &t) {
    hipStream_t st = (hipStream_t)stream;
    d->t_begin = now_s();
    d->n_reads = d->n_parts = d->tags_n = 0;
    const int64_t n_reads = t.n_reads, n_parts = t.n_parts, tags_n = t.tags_n;
    for (int64_t j = 0; j < n_parts; ++j) t.parts[j].len = 0;
    if (n_reads <= 0) return 0;
    if (n_reads >= INT32_MAX / 2 || n_parts >= INT32_MAX / 2) return fail(PCABI_E_ARG, "too many reads for one launch");
    d->h_seg_off = seg_offsets(t.reads, n_reads);
    const std::vector<int64_t> &off = d->h_seg_off;
    const int64_t n_seg = off.back();
    if (n_seg >= INT32_MAX) return fail(PCABI_E_ARG, "too many moves for one launch");
    auto grow = [](int64_t n) { return n + n / 4 + 64; };
    size_t tmp = 0;
    PCABI_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, (int64_t *)nullptr, (int64_t *)nullptr, (int)(n_seg + 1), st));
    if (int rc = d->tags.reserve(tags_n + 64, grow(tags_n))) return rc;
    if (int rc = d->reads.reserve(n_reads, grow(n_reads))) return rc;
    if (int rc = d->parts.reserve(n_parts + 1, grow(n_parts))) return rc;
    if (int rc = d->seg_off.reserve(n_reads + 1, grow(n_reads))) return rc;
    if (int rc = d->val.reserve(n_seg + 1, grow(n_seg))) return rc;
    if (int rc = d->pre.reserve(n_seg + 1, grow(n_seg))) return rc;
    if (int rc = d->q.reserve(2 * n_parts + 2, 2 * grow(n_parts))) return rc;
    if (int rc = d->lens.reserve(n_parts + 1, grow(n_parts))) return rc;
    if (int rc = d->usable.reserve(n_reads, grow(n_reads))) return rc;
    if (int rc = d->scan_tmp.reserve((int64_t)tmp + 1, grow((int64_t)tmp))) return rc;
    PCABI_TRY(hipMemsetAsync(d->lens, 0, (size_t)(n_parts + 1) * 4, st));
    PCABI_TRY(hipMemsetAsync(d->q, 0, (size_t)(2 * n_parts + 2) * 4, st));
    PCABI_TRY(hipMemsetAsync(d->val, 0, (size_t)(n_seg + 1) * 8, st));
    if (tags_n > 0) PCABI_TRY(hipMemcpyAsync(d->tags, t.tags, (size_t)tags_n, hipMemcpyHostToDevice, st));
    PCABI_TRY(hipMemcpyAsync(d->reads, t.reads, (size_t)n_reads * sizeof(pcabi_moves_read), hipMemcpyHostToDevice, st));
    if (n_parts > 0) PCABI_TRY(hipMemcpyAsync(d->parts, t.parts, (size_t)n_parts * sizeof(pcabi_moves_part), hipMemcpyHostToDevice, st));
    PCABI_TRY(hipMemcpyAsync(d->seg_off, off.data(), (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, st));
    const bool prof = prof_on();
    void *sp = prof ? prof_begin(st, 7) : nullptr;
    if (n_seg > 0) {
        hipLaunchKernelGGL(k_moves_count, dim3((unsigned)n_seg), dim3(kWave), 0, st, d->tags.p, tags_n, d->reads.p, n_reads, d->seg_off.p,
                           n_seg, d->val.p);
        PCABI_TRY(hipGetLastError());
    }
    if (prof) prof_end(st, sp), sp = prof_begin(st, 8);
    PCABI_TRY(hipcub::DeviceScan::ExclusiveSum(d->scan_tmp.p, tmp, d->val.p, d->pre.p, (int)(n_seg + 1), st));
    if (prof) prof_end(st, sp), sp = prof_begin(st, 9);
    if (n_parts > 0) {
        hipLaunchKernelGGL(k_moves_select, dim3((unsigned)(2 * n_parts)), dim3(kWave), 0, st, d->tags.p, tags_n, d->reads.p, n_reads,
                           d->parts.p, n_parts, d->seg_off.p, d->pre.p, d->q.p);
        PCABI_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_moves_size, dim3((unsigned)((n_reads + 255) / 256)), dim3(256), 0, st, d->tags.p, tags_n, d->reads.p, n_reads,
                       d->parts.p, n_parts, d->seg_off.p, d->pre.p, d->q.p, d->lens.p, d->usable.p);
    PCABI_TRY(hipGetLastError());
    if (prof) {
        prof_end(st, sp);
        int64_t bytes = n_seg * 24 + n_parts * (int64_t)(sizeof(pcabi_moves_part) + 12) + n_reads * (int64_t)(sizeof(pcabi_moves_read) + 9);
        for (int64_t i = 0; i < n_reads; ++i) bytes += n_moves(t.reads[i]);
        bytes += 2 * n_parts * (kSeg / 2);   // a boundary reads half a segment on average
        prof_add_bytes(7, bytes);
    }
    d->h_lens.assign((size_t)n_parts, 0);
    d->h_usable.assign((size_t)n_reads, 0);
    if (n_parts > 0) PCABI_TRY(hipMemcpyAsync(d->h_lens.data(), d->lens, (size_t)n_parts * 4, hipMemcpyDeviceToHost, st));
    PCABI_TRY(hipMemcpyAsync(d->h_usable.data(), d->usable, (size_t)n_reads, hipMemcpyDeviceToHost, st));
    d->n_reads = n_reads, d->n_parts = n_parts, d->tags_n = tags_n;
    return 0;
}

// Second step: waits for the stream, fills parts[].len and usable[], counts the reads.
int moves_dev_plan_end(MovesDev *d, void *stream, const MovesTables &t) {
    if (t.n_reads <= 0) return 0;
    PCABI_TRY(hipStreamSynchronize((hipStream_t)stream));
    for (int64_t i = 0; i < t.n_reads; ++i) t.usable[i] = d->h_usable[(size_t)i];
    for (int64_t j = 0; j < t.n_parts; ++j) t.parts[j].len = d->h_lens[(size_t)j];
    count_reads(t.usable, t.n_reads);
    g_dev_ns += (int64_t)((now_s() - d->t_begin) * 1e9);
    return 0;
}

// The parts (with out set) of the plan before it written into d_out[0, out_cap), asynchronous on `stream`.
int moves_dev_write(MovesDev *d, void *stream, const pcabi_moves_part *parts, int64_t n_parts, uint8_t *d_out, int64_t out_cap) {
    hipStream_t st = (hipStream_t)stream;
    if (n_parts != d->n_parts) return fail(PCABI_E_ARG, "not the parts that were planned");
    if (n_parts <= 0 || d->n_reads <= 0) return 0;
    d->h_chunk0 = chunk_offsets(parts, n_parts);
    const std::vector<int64_t> &off = d->h_chunk0;
    const int64_t n_chunks = off.back();
    if (n_chunks <= 0) return 0;
    if (n_chunks >= INT32_MAX) return fail(PCABI_E_ARG, "too many bytes for one launch");
    if (int rc = d->chunk0.reserve(n_parts + 1, n_parts + n_parts / 4 + 64)) return rc;
    PCABI_TRY(hipMemcpyAsync(d->parts, parts, (size_t)n_parts * sizeof(pcabi_moves_part), hipMemcpyHostToDevice, st));
    PCABI_TRY(hipMemcpyAsync(d->chunk0, off.data(), (size_t)(n_parts + 1) * 8, hipMemcpyHostToDevice, st));
    const bool prof = prof_on();
    void *sp = prof ? prof_begin(st, 10) : nullptr;
    hipLaunchKernelGGL(k_moves_write, dim3((unsigned)n_chunks), dim3(kWave), 0, st, d->tags.p, d->tags_n, d->reads.p, d->n_reads,
                       d->parts.p, n_parts, d->chunk0.p, n_chunks, d->q.p, d->usable.p, d_out, out_cap);
    PCABI_TRY(hipGetLastError());
    if (prof) {
        prof_end(st, sp);
        int64_t bytes = 0;
        for (int64_t j = 0; j < n_parts; ++j) bytes += 2 * (int64_t)parts[j].len + (int64_t)sizeof(pcabi_moves_part) + 8;
        prof_add_bytes(10, bytes);
    }
    return 0;
}

}  // namespace pcabi_internal

extern "C" {

int pcabi_moves_plan(int device, const uint8_t *tags, int64_t tags_n, const pcabi_moves_read *reads, int64_t n_reads,
                     pcabi_moves_part *parts, int64_t n_parts, uint8_t *usable) {
    if (tags_n < 0 || n_reads < 0 || n_parts < 0 || (tags_n > 0 && !tags) || (n_reads > 0 && (!reads || !usable)) || (n_parts > 0 && !parts))
        return fail(PCABI_E_ARG, "bad arguments");
    const MovesTables t{tags, tags_n, reads, n_reads, parts, n_parts, usable};
    if (device < 0) {
        MovesHost keep;
        return moves_plan_host(&keep, t);
    }
    if (int rc = moves_check(t)) return rc;   // before any launch
    PCABI_TRY(hipSetDevice(device));
    MovesDev dev;
    if (int rc = moves_dev_plan_begin(&dev, nullptr, t)) return rc;
    return moves_dev_plan_end(&dev, nullptr, t);
}

int pcabi_moves_remap(int device, const uint8_t *tags, int64_t tags_n, const pcabi_moves_read *reads, int64_t n_reads,
                      const pcabi_moves_part *parts, int64_t n_parts, uint8_t *out, int64_t out_cap) {
    if (tags_n < 0 || n_reads < 0 || n_parts < 0 || out_cap < 0 || (tags_n > 0 && !tags) || (n_reads > 0 && !reads) ||
        (n_parts > 0 && !parts) || (out_cap > 0 && !out))
        return fail(PCABI_E_ARG, "bad arguments");
    if (int rc = check_tables(tags_n, reads, n_reads, parts, n_parts)) return rc;
    // the plan again, on the host: the caller's lengths must be its lengths, and no two ranges may meet
    std::vector<pcabi_moves_part> mine(parts, parts + n_parts);
    std::vector<uint8_t> usable((size_t)n_reads);
    for (pcabi_moves_part &p : mine) p.len = 0;
    MovesHost keep;
    plan_host(tags, reads, n_reads, mine.data(), n_parts, usable.data(), nullptr, &keep);
    std::vector<std::pair<int64_t, int64_t>> spans;
    for (int64_t j = 0; j < n_parts; ++j) {
        if (mine[(size_t)j].len != parts[j].len) return fail(PCABI_E_ARG, "part " + std::to_string(j) + ": len is not the plan's");
        if (parts[j].len > 0 && (parts[j].out < 0 || parts[j].len > out_cap - parts[j].out))
            return fail(PCABI_E_ARG, "part " + std::to_string(j) + " does not fit the output");
        if (parts[j].len > 0) spans.emplace_back(parts[j].out, parts[j].out + parts[j].len);
    }
    std::sort(spans.begin(), spans.end());
    for (size_t k = 1; k < spans.size(); ++k)
        if (spans[k].first < spans[k - 1].second) return fail(PCABI_E_ARG, "two parts' outputs overlap");
    if (device < 0) {
        plan_host(tags, reads, n_reads, const_cast<pcabi_moves_part *>(parts), n_parts, nullptr, out, &keep);
        return 0;
    }
    PCABI_TRY(hipSetDevice(device));
    constexpr int64_t kGuard = 64;
    std::vector<uint8_t> stage((size_t)(out_cap + 2 * kGuard), 0xA5);
    if (out_cap > 0) std::memcpy(stage.data() + kGuard, out, (size_t)out_cap);
    DevBuf<> d_out;
    MovesDev dev;
    if (int rc = d_out.reserve((int64_t)stage.size(), (int64_t)stage.size())) return rc;
    PCABI_TRY(hipMemcpy(d_out, stage.data(), stage.size(), hipMemcpyHostToDevice));
    const MovesTables t{tags, tags_n, reads, n_reads, mine.data(), n_parts, usable.data()};
    if (int rc = moves_dev_plan_begin(&dev, nullptr, t)) return rc;
    PCABI_TRY(hipStreamSynchronize(nullptr));
    for (int64_t j = 0; j < n_parts; ++j)
        if (dev.h_lens[(size_t)j] != parts[j].len)
            return fail(PCABI_E_DEVICE, "the move kernels and the host build disagree on part " + std::to_string(j));
    if (int rc = moves_dev_write(&dev, nullptr, parts, n_parts, d_out + kGuard, out_cap)) return rc;
    PCABI_TRY(hipStreamSynchronize(nullptr));
    PCABI_TRY(hipMemcpy(stage.data(), d_out, stage.size(), hipMemcpyDeviceToHost));
    for (int64_t g = 0; g < kGuard; ++g)
        if (stage[(size_t)(kGuard - 1 - g)] != 0xA5 || stage[(size_t)(kGuard + out_cap + g)] != 0xA5)
            return fail(PCABI_E_DEVICE, "k_moves_write wrote outside its output");
    if (out_cap > 0) std::memcpy(out, stage.data() + kGuard, (size_t)out_cap);
    return 0;
}

void pcabi_moves_counts(int reset, int64_t *remapped, int64_t *dropped) {
    if (remapped) *remapped = g_remapped.load();
    if (dropped) *dropped = g_dropped.load();
    if (reset) g_remapped = 0, g_dropped = 0;
}

}  // extern "C"
