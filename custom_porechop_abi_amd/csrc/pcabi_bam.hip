// pcabi_bam.hip -- unaligned BAM records unpacked on the GPU (gfx950): include/pcabi.h pcabi_bam_*;
// DESIGN.md "BAM input".
//
// k_bam_unpack: the packed 4-bit sequence and the raw qualities of every record in a table the host
// built (pcabi_bam.h walk) become sequence letters, qualities + 33 and Dna5 codes in the reader's
// batch layout. Work is split by tiles of 16384 bases, one workgroup of 256 lanes per tile, so a 2 Mb
// read is 123 workgroups and a 200-base read is one. The workgroup finds its record by a binary
// search over the table's tile0 column (uniform, scalar loads). For each of the three outputs the
// tile is cut where the *destination* is 16-byte aligned: a lane takes such pieces in turn, loads a
// piece's eight (or nine) packed bytes or sixteen quality bytes with one unaligned wide load, and stores
// sixteen aligned bytes; the lanes holding the ragged first and last piece store single bytes
// (pcabi_bam.h unpack_range, the function the host reader runs too). A reverse-strand record's piece
// reads its bases from the record's end. No atomics, no inline assembly; a record writes its own
// output ranges only (the codes' padding up to the next multiple of four belongs to it).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/pcabi.h"
#include "pcabi_bam.h"

namespace pcabi_internal {
int fail(int code, const std::string &msg);
}
using pcabi_internal::fail;
using namespace pcabi_bam;

#define BAM_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) return fail(PCABI_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

namespace {

constexpr int kLanes = 256;

__global__ __launch_bounds__(kLanes) void k_bam_unpack(const uint8_t *__restrict__ bam, int64_t n,
                                                       const pcabi_bam_rec *__restrict__ recs, int64_t n_recs,
                                                       int64_t n_tiles, uint8_t *__restrict__ seq, int64_t seq_cap,
                                                       uint8_t *__restrict__ qual, int64_t qual_cap,
                                                       uint8_t *__restrict__ codes, int64_t codes_cap,
                                                       int64_t tail_off) {
    const int64_t tile = blockIdx.x;
    if (tile >= n_tiles) {   // the extra workgroup: the batch's 16 bytes of tail padding
        if (tail_off >= 0 && tail_off + 16 <= codes_cap && threadIdx.x < 16) codes[tail_off + threadIdx.x] = 4;
        return;
    }
    // the last record whose tile0 <= tile (records without bases share the next record's tile0)
    int64_t lo = 0, hi = n_recs - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (recs[mid].tile0 <= tile) lo = mid;
        else hi = mid - 1;
    }
    const pcabi_bam_rec r = recs[lo];
    const int64_t t0 = (tile - r.tile0) * kTileBases;
    if (!rec_fits(r, n, seq_cap, qual_cap, codes_cap) || t0 < 0 || t0 >= r.l_seq) return;   // uniform
    const int64_t t1 = t0 + kTileBases < r.l_seq ? t0 + kTileBases : (int64_t)r.l_seq;
    const uint8_t *sq = bam + r.rec + r.seq_at;
    uint8_t *out[3] = {seq + r.seq_out, qual + r.qual_out, codes + r.code_out};
#pragma unroll
    for (int o = 0; o < 3; ++o) {
        // pieces [a + 16k, a + 16k + 16) of the destination's address space, clipped to the tile
        const int64_t d = (int64_t)(uintptr_t)out[o];
        const int64_t a = (d + t0) & ~(int64_t)15;
        const int64_t pieces = (d + t1 - a + 15) >> 4;
        for (int64_t k = threadIdx.x; k < pieces; k += kLanes) {
            const int64_t p0 = a + 16 * k - d, b0 = p0 > t0 ? p0 : t0, b1 = p0 + 16 < t1 ? p0 + 16 : t1;
            unpack_range(sq, r.l_seq, r.flag, b0, b1, o == 0 ? out[0] : nullptr, o == 1 ? out[1] : nullptr,
                         o == 2 ? out[2] : nullptr);
        }
    }
}

int launch(hipStream_t st, const uint8_t *bam, int64_t n, const pcabi_bam_rec *recs, int64_t n_recs, int64_t n_tiles,
           uint8_t *seq, int64_t seq_cap, uint8_t *qual, int64_t qual_cap, uint8_t *codes, int64_t codes_cap,
           int64_t tail_off) {
    if (n_tiles < 0 || n_tiles >= INT32_MAX) return fail(PCABI_E_ARG, "too many tiles for one launch");
    if (n_recs <= 0 && tail_off < 0) return 0;
    const int64_t tiles = n_recs > 0 ? n_tiles : 0;
    hipLaunchKernelGGL(k_bam_unpack, dim3((unsigned)(tiles + 1)), dim3(kLanes), 0, st, bam, n, recs, n_recs, tiles, seq,
                       seq_cap, qual, qual_cap, codes, codes_cap, tail_off);
    BAM_TRY(hipGetLastError());
    return 0;
}

// ---- device-event spans (the timing tool) --------------------------------------------------------
struct Span {
    hipEvent_t a = nullptr, b = nullptr;
    int kind = 0;
};
std::mutex g_prof_mu;
bool g_prof = false;
std::vector<Span *> g_spans;
double g_ms[4] = {0, 0, 0, 0};
int64_t g_unpack_bytes = 0;

void harvest() {   // g_prof_mu held; the spans' streams are idle
    for (Span *s : g_spans) {
        float ms = 0;
        if (s->a && s->b && hipEventSynchronize(s->b) == hipSuccess && hipEventElapsedTime(&ms, s->a, s->b) == hipSuccess)
            g_ms[s->kind] += ms;
        if (s->a) (void)hipEventDestroy(s->a);
        if (s->b) (void)hipEventDestroy(s->b);
        delete s;
    }
    g_spans.clear();
}

}  // namespace

namespace pcabi_internal {

bool prof_on() {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    return g_prof;
}

// kind: 0 k_inflate, 1 k_bam_unpack, 2 copies to the device, 3 copies from the device
void *prof_begin(void *stream, int kind) {
    Span *s = new Span();
    s->kind = kind;
    if (hipEventCreate(&s->a) != hipSuccess || hipEventCreate(&s->b) != hipSuccess ||
        hipEventRecord(s->a, (hipStream_t)stream) != hipSuccess) {
        if (s->a) (void)hipEventDestroy(s->a);
        if (s->b) (void)hipEventDestroy(s->b);
        delete s;
        return nullptr;
    }
    return s;
}

void prof_end(void *stream, void *span) {
    if (!span) return;
    Span *s = (Span *)span;
    (void)hipEventRecord(s->b, (hipStream_t)stream);
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_spans.push_back(s);
}

// ---- the device half of the BAM reader (csrc/pcabi_io.cpp) ---------------------------------------
// A mirror on the device of the reader's window of inflated bytes (the carried incomplete record, then
// the newest group), the record table and the three outputs, which come back through pinned memory.
struct BamDev {
    int device = 0;
    uint8_t *win[2] = {nullptr, nullptr};   // the window, ping-pong: the carry moves between them
    int64_t cap[2] = {0, 0};
    int cur = 0;
    int64_t len = 0;
    hipStream_t st = nullptr;               // the stream of the newest group
    hipEvent_t moved = nullptr;             // recorded on st behind the window's copies
    bool moved_set = false;
    pcabi_bam_rec *d_recs = nullptr, *p_recs = nullptr;
    int64_t recs_cap = 0;
    uint8_t *d_out = nullptr, *p_out = nullptr;
    int64_t out_cap = 0;
};

int bam_dev_open(int device, BamDev **out) {
    BamDev *b = new BamDev();
    b->device = device;
    *out = b;
    return 0;
}

void bam_dev_close(BamDev *b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->moved_set) (void)hipEventSynchronize(b->moved);
    if (b->st) (void)hipStreamSynchronize(b->st);
    if (b->moved) (void)hipEventDestroy(b->moved);
    for (int k = 0; k < 2; ++k)
        if (b->win[k]) (void)hipFree(b->win[k]);
    if (b->d_recs) (void)hipFree(b->d_recs);
    if (b->p_recs) (void)hipHostFree(b->p_recs);
    if (b->d_out) (void)hipFree(b->d_out);
    if (b->p_out) (void)hipHostFree(b->p_out);
    delete b;
}

// window = window[keep_from, len) + src[0, n) (src on the device), ordered on `stream`. The groups'
// streams alternate, and the stream of the group before already holds the next group's inflate: the new
// copies wait for the event behind the last window copies alone, never for that stream, so the inflate
// runs on beside them and beside the unpack.
int bam_dev_append(BamDev *b, int64_t keep_from, const uint8_t *src, int64_t n, void *stream) {
    BAM_TRY(hipSetDevice(b->device));
    hipStream_t st = (hipStream_t)stream;
    if (!b->moved) BAM_TRY(hipEventCreateWithFlags(&b->moved, hipEventDisableTiming));
    if (b->moved_set && b->st != st) BAM_TRY(hipStreamWaitEvent(st, b->moved, 0));
    b->st = st;
    if (keep_from < 0 || keep_from > b->len || n < 0) return fail(PCABI_E_ARG, "bad window");
    const int64_t carry = b->len - keep_from, need = carry + n + 64;
    const int nxt = b->cur ^ 1;
    if (b->cap[nxt] < need) {
        if (b->win[nxt]) BAM_TRY(hipFree(b->win[nxt]));
        b->win[nxt] = nullptr;
        b->cap[nxt] = 0;
        const int64_t want = std::max<int64_t>(need + need / 2, 1 << 20);
        BAM_TRY(hipMalloc((void **)&b->win[nxt], (size_t)want));
        b->cap[nxt] = want;
    }
    const bool prof = prof_on();
    void *sp = prof ? prof_begin(st, 2) : nullptr;
    if (carry > 0)
        BAM_TRY(hipMemcpyAsync(b->win[nxt], b->win[b->cur] + keep_from, (size_t)carry, hipMemcpyDeviceToDevice, st));
    if (n > 0) BAM_TRY(hipMemcpyAsync(b->win[nxt] + carry, src, (size_t)n, hipMemcpyDeviceToDevice, st));
    if (prof) prof_end(st, sp);
    BAM_TRY(hipEventRecord(b->moved, st));
    b->moved_set = true;
    b->cur = nxt;
    b->len = carry + n;
    return 0;
}

// The table's records (offsets relative to the window and to the outputs' starts) unpacked on the
// window's stream; *seq / *qual / *codes = the outputs in pinned memory, valid until the next call.
// Synchronises.
int bam_dev_unpack(BamDev *b, const pcabi_bam_rec *recs, int64_t n_recs, const Layout &lay, const uint8_t **seq,
                   const uint8_t **qual, const uint8_t **codes) {
    BAM_TRY(hipSetDevice(b->device));
    hipStream_t st = b->st;
    if (n_recs > b->recs_cap) {
        if (b->d_recs) BAM_TRY(hipFree(b->d_recs));
        if (b->p_recs) BAM_TRY(hipHostFree(b->p_recs));
        b->d_recs = b->p_recs = nullptr;
        b->recs_cap = 0;
        const int64_t want = std::max<int64_t>(n_recs + n_recs / 2, 1024);
        BAM_TRY(hipMalloc((void **)&b->d_recs, (size_t)want * sizeof(pcabi_bam_rec)));
        BAM_TRY(hipHostMalloc((void **)&b->p_recs, (size_t)want * sizeof(pcabi_bam_rec), hipHostMallocDefault));
        b->recs_cap = want;
    }
    // seq | qual | codes, each region's start 256-aligned
    const int64_t seq_sz = (lay.seq + 255) & ~(int64_t)255, code_sz = (lay.code + 255) & ~(int64_t)255;
    const int64_t total = 2 * seq_sz + code_sz + 256;
    if (total > b->out_cap) {
        if (b->d_out) BAM_TRY(hipFree(b->d_out));
        if (b->p_out) BAM_TRY(hipHostFree(b->p_out));
        b->d_out = b->p_out = nullptr;
        b->out_cap = 0;
        const int64_t want = std::max<int64_t>(total + total / 4, 1 << 20);
        BAM_TRY(hipMalloc((void **)&b->d_out, (size_t)want));
        BAM_TRY(hipHostMalloc((void **)&b->p_out, (size_t)want, hipHostMallocDefault));
        b->out_cap = want;
    }
    std::memcpy(b->p_recs, recs, (size_t)n_recs * sizeof(pcabi_bam_rec));
    const bool prof = prof_on();
    void *sp = prof ? prof_begin(st, 2) : nullptr;
    BAM_TRY(hipMemcpyAsync(b->d_recs, b->p_recs, (size_t)n_recs * sizeof(pcabi_bam_rec), hipMemcpyHostToDevice, st));
    if (prof) prof_end(st, sp), sp = prof_begin(st, 1);
    if (int rc = launch(st, b->win[b->cur], b->len, b->d_recs, n_recs, lay.tiles, b->d_out, lay.seq, b->d_out + seq_sz,
                        lay.seq, b->d_out + 2 * seq_sz, lay.code, -1))
        return rc;
    if (prof) prof_end(st, sp), sp = prof_begin(st, 3);
    // the three regions' used bytes come back in one copy when they are small, else one each
    if (lay.seq > 0) {
        BAM_TRY(hipMemcpyAsync(b->p_out, b->d_out, (size_t)lay.seq, hipMemcpyDeviceToHost, st));
        BAM_TRY(hipMemcpyAsync(b->p_out + seq_sz, b->d_out + seq_sz, (size_t)lay.seq, hipMemcpyDeviceToHost, st));
        BAM_TRY(hipMemcpyAsync(b->p_out + 2 * seq_sz, b->d_out + 2 * seq_sz, (size_t)lay.code, hipMemcpyDeviceToHost, st));
    }
    if (prof) {
        prof_end(st, sp);
        std::lock_guard<std::mutex> lk(g_prof_mu);
        g_unpack_bytes += (lay.seq + 1) / 2 + lay.seq + 2 * lay.seq + lay.code + n_recs * (int64_t)sizeof(pcabi_bam_rec);
    }
    BAM_TRY(hipStreamSynchronize(st));
    *seq = b->p_out;
    *qual = b->p_out + seq_sz;
    *codes = b->p_out + 2 * seq_sz;
    return 0;
}

}  // namespace pcabi_internal

extern "C" {

int64_t pcabi_bam_index(const uint8_t *bam, int64_t n, pcabi_bam_rec *recs, int64_t cap, int64_t *totals) {
    if (n < 0 || (n > 0 && !bam) || cap < 0 || (cap > 0 && !recs)) return fail(PCABI_E_ARG, "bad arguments");
    const int64_t h = header_len(bam, n);
    if (h < 0) return fail(PCABI_E_PARSE, "not a BAM header");
    if (h == 0) return fail(PCABI_E_PARSE, "truncated BAM header");
    Layout lay;
    int64_t stop = 0;
    const int64_t kept = walk(bam, n, h, recs, cap, &lay, &stop);
    if (kept < 0) return fail(PCABI_E_PARSE, "invalid BAM record at offset " + std::to_string(stop));
    if (stop != n) return fail(PCABI_E_PARSE, "truncated BAM record at offset " + std::to_string(stop));
    if (totals) {
        totals[0] = totals[1] = lay.seq;
        totals[2] = lay.code + 16;
        totals[3] = lay.names;
        totals[4] = lay.tiles;
    }
    return kept;
}

int pcabi_bam_unpack_dev(void *stream, const uint8_t *bam, int64_t n, const pcabi_bam_rec *recs, int64_t n_recs,
                         int64_t n_tiles, uint8_t *seq, int64_t seq_cap, uint8_t *qual, int64_t qual_cap,
                         uint8_t *codes, int64_t codes_cap, int64_t tail_off) {
    if (n < 0 || n_recs < 0 || n_tiles < 0 || seq_cap < 0 || qual_cap < 0 || codes_cap < 0 ||
        (n_recs > 0 && (!bam || !recs)) || (seq_cap > 0 && !seq) || (qual_cap > 0 && !qual) || (codes_cap > 0 && !codes) ||
        (tail_off >= 0 && tail_off + 16 > codes_cap))
        return fail(PCABI_E_ARG, "bad arguments");
    return launch((hipStream_t)stream, bam, n, recs, n_recs, n_tiles, seq, seq_cap, qual, qual_cap, codes, codes_cap,
                  tail_off);
}

int pcabi_bam_unpack_host(int device, const uint8_t *bam, int64_t n, const pcabi_bam_rec *recs, int64_t n_recs,
                          uint8_t *seq, int64_t seq_cap, uint8_t *qual, int64_t qual_cap, uint8_t *codes,
                          int64_t codes_cap, int64_t tail_off) {
    if (n < 0 || n_recs < 0 || seq_cap < 0 || qual_cap < 0 || codes_cap < 0 || (n_recs > 0 && (!bam || !recs)) ||
        (seq_cap > 0 && !seq) || (qual_cap > 0 && !qual) || (codes_cap > 0 && !codes) ||
        (tail_off >= 0 && tail_off + 16 > codes_cap))
        return fail(PCABI_E_ARG, "bad arguments");
    int64_t tiles = 0;
    for (int64_t i = 0; i < n_recs; ++i) {
        if (!rec_fits(recs[i], n, seq_cap, qual_cap, codes_cap) || recs[i].tile0 != tiles)
            return fail(PCABI_E_ARG, "record " + std::to_string(i) + " of the table does not fit the buffers");
        tiles += ((int64_t)recs[i].l_seq + kTileBases - 1) / kTileBases;
    }
    if (device < 0) {
        for (int64_t i = 0; i < n_recs; ++i) {
            const pcabi_bam_rec &r = recs[i];
            unpack_range(bam + r.rec + r.seq_at, r.l_seq, r.flag, 0, r.l_seq, seq + r.seq_out, qual + r.qual_out,
                         codes + r.code_out);
        }
        if (tail_off >= 0) std::memset(codes + tail_off, 4, 16);
        return 0;
    }
    BAM_TRY(hipSetDevice(device));
    // every output sits between 64 guard bytes on the device, checked after the kernel; bytes no record
    // owns go up and come back as they were
    constexpr int64_t kGuard = 64;
    uint8_t *host_out[3] = {seq, qual, codes};
    const int64_t caps[3] = {seq_cap, qual_cap, codes_cap};
    std::vector<uint8_t> stage[3];
    uint8_t *d_bam = nullptr, *d_out[3] = {nullptr, nullptr, nullptr};
    pcabi_bam_rec *d_recs = nullptr;
    int rc = 0;
    auto step = [&](hipError_t e, const char *what) {
        if (!rc && e != hipSuccess) rc = fail(PCABI_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
    };
    step(hipMalloc((void **)&d_bam, (size_t)n + 64), "hipMalloc");
    step(hipMalloc((void **)&d_recs, (size_t)(n_recs + 1) * sizeof(pcabi_bam_rec)), "hipMalloc");
    if (!rc && n > 0) step(hipMemcpy(d_bam, bam, (size_t)n, hipMemcpyHostToDevice), "hipMemcpy");
    if (!rc && n_recs > 0)
        step(hipMemcpy(d_recs, recs, (size_t)n_recs * sizeof(pcabi_bam_rec), hipMemcpyHostToDevice), "hipMemcpy");
    int64_t base[3];   // the device output starts as far off a 16-byte boundary as the caller's pointer
    for (int o = 0; o < 3; ++o) {
        base[o] = kGuard + (int64_t)((uintptr_t)host_out[o] & 15u);
        stage[o].assign((size_t)(base[o] + caps[o] + kGuard), 0xA5);
        if (caps[o] > 0) std::memcpy(stage[o].data() + base[o], host_out[o], (size_t)caps[o]);
        step(hipMalloc((void **)&d_out[o], stage[o].size()), "hipMalloc");
        if (!rc) step(hipMemcpy(d_out[o], stage[o].data(), stage[o].size(), hipMemcpyHostToDevice), "hipMemcpy");
    }
    if (!rc)
        rc = launch(nullptr, d_bam, n, d_recs, n_recs, tiles, d_out[0] + base[0], seq_cap, d_out[1] + base[1], qual_cap,
                    d_out[2] + base[2], codes_cap, tail_off);
    if (!rc) step(hipStreamSynchronize(nullptr), "hipStreamSynchronize");
    for (int o = 0; o < 3 && !rc; ++o) {
        step(hipMemcpy(stage[o].data(), d_out[o], stage[o].size(), hipMemcpyDeviceToHost), "hipMemcpy");
        if (rc) break;
        for (int64_t g = 0; g < kGuard; ++g)
            if (stage[o][(size_t)(base[o] - 1 - g)] != 0xA5 || stage[o][(size_t)(base[o] + caps[o] + g)] != 0xA5) {
                rc = fail(PCABI_E_DEVICE, "k_bam_unpack wrote outside output " + std::to_string(o));
                break;
            }
    }
    if (!rc)
        for (int o = 0; o < 3; ++o)
            if (caps[o] > 0) std::memcpy(host_out[o], stage[o].data() + base[o], (size_t)caps[o]);
    (void)hipFree(d_bam);
    (void)hipFree(d_recs);
    for (int o = 0; o < 3; ++o) (void)hipFree(d_out[o]);
    return rc;
}

void pcabi_bam_last_times(int on, int reset, double *ms, int64_t *bytes) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    harvest();
    if (ms)
        for (int k = 0; k < 4; ++k) ms[k] = g_ms[k];
    if (bytes) *bytes = g_unpack_bytes;
    if (reset) {
        for (double &v : g_ms) v = 0;
        g_unpack_bytes = 0;
    }
    if (on >= 0) g_prof = on != 0;
}

}  // extern "C"
