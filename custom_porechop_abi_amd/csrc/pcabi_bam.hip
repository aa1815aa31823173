// pcabi_bam.hip -- unaligned BAM records unpacked (k_bam_unpack) and packed (k_bam_pack, further down)
// on the GPU (gfx950): include/pcabi.h pcabi_bam_*; DESIGN.md "BAM input", "BAM output".
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
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/pcabi.h"
#include "pcabi_bam.h"
#include "pcabi_hostdev.h"

using namespace pcabi_internal;
using namespace pcabi_bam;

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
    PCABI_TRY(hipGetLastError());
    return 0;
}

// k_bam_pack: the inverse (DESIGN.md "BAM output"). A table of parts (pcabi_bam.h PackLayout) becomes a
// chain of unmapped BAM records: one workgroup per tile of 16384 bases, the part found by the same
// uniform binary search over tile0. Every part owns at least one tile, a part without bases too: the
// workgroup of a part's first tile also writes block_size, the fixed fields, the name with its NUL and
// the aux bytes, as byte copies striding over the lanes. The packed sequence (two letters a byte) and
// the qualities (character - 33) are cut where the destination is 16-byte aligned, as in the unpack:
// a lane loads a piece's 32 letters or 16 quality characters and stores sixteen aligned bytes; the
// ragged first and last pieces are single bytes. Tile edges are even base counts, so no packed byte
// has two writers. A part writes its own record's bytes only.
__global__ __launch_bounds__(kLanes) void k_bam_pack(const uint8_t *__restrict__ seq, int64_t seq_n,
                                                     const uint8_t *__restrict__ qual, int64_t qual_n,
                                                     const uint8_t *__restrict__ side, int64_t side_n,
                                                     const pcabi_bam_part *__restrict__ parts, int64_t n_parts,
                                                     int64_t n_tiles, uint8_t *__restrict__ out, int64_t out_cap) {
    const int64_t tile = blockIdx.x;
    if (tile >= n_tiles || n_parts <= 0) return;
    int64_t lo = 0, hi = n_parts - 1;   // the last part whose tile0 <= tile
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (parts[mid].tile0 <= tile) lo = mid;
        else hi = mid - 1;
    }
    const pcabi_bam_part p = parts[lo];
    if (!part_fits(p, seq_n, qual_n, side_n, out_cap)) return;   // uniform
    const int64_t t0 = (tile - p.tile0) * kTileBases;
    if (t0 < 0 || t0 >= part_tiles(p) * kTileBases) return;
    uint8_t *rec = out + p.out;
    if (t0 == 0) pack_head(p, side, rec, threadIdx.x, kLanes);
    if (t0 >= p.l_seq) return;
    const int64_t t1 = t0 + kTileBases < p.l_seq ? t0 + kTileBases : (int64_t)p.l_seq;
    const uint8_t *src = seq + p.seq_src, *qsrc = p.qual_src >= 0 ? qual + p.qual_src : nullptr;
    uint8_t *sq = rec + part_seq_at(p), *ql = sq + ((int64_t)p.l_seq + 1) / 2;
    {   // packed sequence: bytes [t0 / 2, (t1 + 1) / 2) in pieces of the destination's 16-byte grid
        const int64_t d = (int64_t)(uintptr_t)sq, y0 = t0 / 2, y1 = (t1 + 1) / 2;
        const int64_t a = (d + y0) & ~(int64_t)15, pieces = (d + y1 - a + 15) >> 4;
        for (int64_t k = threadIdx.x; k < pieces; k += kLanes) {
            const int64_t q0 = a + 16 * k - d, c0 = q0 > y0 ? q0 : y0, c1 = q0 + 16 < y1 ? q0 + 16 : y1;
            pack_range(src, qsrc, p.l_seq, 2 * c0, 2 * c1 < t1 ? 2 * c1 : t1, sq, nullptr);
        }
    }
    {   // qualities: bytes [t0, t1)
        const int64_t d = (int64_t)(uintptr_t)ql;
        const int64_t a = (d + t0) & ~(int64_t)15, pieces = (d + t1 - a + 15) >> 4;
        for (int64_t k = threadIdx.x; k < pieces; k += kLanes) {
            const int64_t q0 = a + 16 * k - d, b0 = q0 > t0 ? q0 : t0, b1 = q0 + 16 < t1 ? q0 + 16 : t1;
            pack_range(src, qsrc, p.l_seq, b0, b1, nullptr, ql);
        }
    }
}

int launch_pack(hipStream_t st, const uint8_t *seq, int64_t seq_n, const uint8_t *qual, int64_t qual_n, const uint8_t *side,
                int64_t side_n, const pcabi_bam_part *parts, int64_t n_parts, int64_t n_tiles, uint8_t *out, int64_t out_cap) {
    if (n_tiles < 0 || n_tiles >= INT32_MAX) return fail(PCABI_E_ARG, "too many tiles for one launch");
    if (n_parts <= 0 || n_tiles == 0) return 0;
    hipLaunchKernelGGL(k_bam_pack, dim3((unsigned)n_tiles), dim3(kLanes), 0, st, seq, seq_n, qual, qual_n, side, side_n, parts,
                       n_parts, n_tiles, out, out_cap);
    PCABI_TRY(hipGetLastError());
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
// [4]: k_bam_pack, [5]: k_mods_plan, [6]: k_mods_write, [7..10]: k_moves_count, its scan, k_moves_select, k_moves_write
double g_ms[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
int64_t g_unpack_bytes = 0, g_pack_bytes = 0, g_mods_bytes = 0, g_moves_bytes = 0;

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

// kind: 0 k_inflate, 1 k_bam_unpack, 2 copies to the device, 3 copies from the device, 4 k_bam_pack,
// 5 k_mods_plan, 6 k_mods_write, 7 k_moves_count, 8 the move tables' scan, 9 k_moves_select and k_moves_size, 10 k_moves_write
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
    DevBuf<> win[2];                        // the window, ping-pong: the carry moves between them
    int cur = 0;
    int64_t len = 0;
    hipStream_t st = nullptr;               // the stream of the newest group (the GunzipReader's)
    hipEvent_t moved = nullptr;             // recorded on st behind the window's copies
    bool moved_set = false;
    DevBuf<pcabi_bam_rec> d_recs;
    PinBuf<pcabi_bam_rec> p_recs;
    DevBuf<> d_out;
    PinBuf<> p_out;
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
    delete b;
}

// window = window[keep_from, len) + src[0, n) (src on the device), ordered on `stream`. The groups'
// streams alternate, and the stream of the group before already holds the next group's inflate: the new
// copies wait for the event behind the last window copies alone, never for that stream, so the inflate
// runs on beside them and beside the unpack.
int bam_dev_append(BamDev *b, int64_t keep_from, const uint8_t *src, int64_t n, void *stream) {
    PCABI_TRY(hipSetDevice(b->device));
    hipStream_t st = (hipStream_t)stream;
    if (!b->moved) PCABI_TRY(hipEventCreateWithFlags(&b->moved, hipEventDisableTiming));
    if (b->moved_set && b->st != st) PCABI_TRY(hipStreamWaitEvent(st, b->moved, 0));
    b->st = st;
    if (keep_from < 0 || keep_from > b->len || n < 0) return fail(PCABI_E_ARG, "bad window");
    const int64_t carry = b->len - keep_from, need = carry + n + 64;
    const int nxt = b->cur ^ 1;
    if (int rc = b->win[nxt].reserve(need, std::max<int64_t>(need + need / 2, 1 << 20))) return rc;
    const bool prof = prof_on();
    void *sp = prof ? prof_begin(st, 2) : nullptr;
    if (carry > 0)
        PCABI_TRY(hipMemcpyAsync(b->win[nxt], b->win[b->cur] + keep_from, (size_t)carry, hipMemcpyDeviceToDevice, st));
    if (n > 0) PCABI_TRY(hipMemcpyAsync(b->win[nxt] + carry, src, (size_t)n, hipMemcpyDeviceToDevice, st));
    if (prof) prof_end(st, sp);
    PCABI_TRY(hipEventRecord(b->moved, st));
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
    PCABI_TRY(hipSetDevice(b->device));
    hipStream_t st = b->st;
    const int64_t recs_want = std::max<int64_t>(n_recs + n_recs / 2, 1024);
    if (int rc = b->d_recs.reserve(n_recs, recs_want)) return rc;
    if (int rc = b->p_recs.reserve(n_recs, recs_want)) return rc;
    // seq | qual | codes, each region's start 256-aligned
    const int64_t seq_sz = (lay.seq + 255) & ~(int64_t)255, code_sz = (lay.code + 255) & ~(int64_t)255;
    const int64_t total = 2 * seq_sz + code_sz + 256, out_want = std::max<int64_t>(total + total / 4, 1 << 20);
    if (int rc = b->d_out.reserve(total, out_want)) return rc;
    if (int rc = b->p_out.reserve(total, out_want)) return rc;
    std::memcpy(b->p_recs, recs, (size_t)n_recs * sizeof(pcabi_bam_rec));
    const bool prof = prof_on();
    void *sp = prof ? prof_begin(st, 2) : nullptr;
    PCABI_TRY(hipMemcpyAsync(b->d_recs, b->p_recs, (size_t)n_recs * sizeof(pcabi_bam_rec), hipMemcpyHostToDevice, st));
    if (prof) prof_end(st, sp), sp = prof_begin(st, 1);
    if (int rc = launch(st, b->win[b->cur], b->len, b->d_recs, n_recs, lay.tiles, b->d_out, lay.seq, b->d_out + seq_sz,
                        lay.seq, b->d_out + 2 * seq_sz, lay.code, -1))
        return rc;
    if (prof) prof_end(st, sp), sp = prof_begin(st, 3);
    // the three regions' used bytes come back in one copy when they are small, else one each
    if (lay.seq > 0) {
        PCABI_TRY(hipMemcpyAsync(b->p_out, b->d_out, (size_t)lay.seq, hipMemcpyDeviceToHost, st));
        PCABI_TRY(hipMemcpyAsync(b->p_out + seq_sz, b->d_out + seq_sz, (size_t)lay.seq, hipMemcpyDeviceToHost, st));
        PCABI_TRY(hipMemcpyAsync(b->p_out + 2 * seq_sz, b->d_out + 2 * seq_sz, (size_t)lay.code, hipMemcpyDeviceToHost, st));
    }
    if (prof) {
        prof_end(st, sp);
        std::lock_guard<std::mutex> lk(g_prof_mu);
        g_unpack_bytes += (lay.seq + 1) / 2 + lay.seq + 2 * lay.seq + lay.code + n_recs * (int64_t)sizeof(pcabi_bam_rec);
    }
    PCABI_TRY(hipStreamSynchronize(st));
    *seq = b->p_out;
    *qual = b->p_out + seq_sz;
    *codes = b->p_out + 2 * seq_sz;
    return 0;
}

// ---- the device half of the BAM writer (csrc/pcabi_write.cpp) ------------------------------------
// head[0, head_n) (the file header, or nothing) and the record chain of `parts` (planned from head_n)
// form one stream of stream_n bytes in device memory: the text, the table and the side blob go up,
// k_bam_pack writes the chain, the BGZF encoder (pcabi_bgzf_dev) reads it there in members of 65280
// bytes, and only the compressed bytes come back, into pinned memory that `sink` reads before the call
// returns. The buffers are kept between calls (one device at a time, one call at a time). Returns the
// compressed length or a negative code.
namespace {
struct PackDev {
    int device = -1;
    DevBuf<> buf[6];   // seq, qual, side, parts, stream, z
    DevBuf<> scratch;
    DevBuf<int64_t> d_len;
    PinBuf<> p_z;      // the compressed bytes, pinned
    Stream st;
    RemapDev remap;    // the remap stage's device side (pcabi_hostdev.h)
};
// kept for the process and never destroyed (a deliberate leak): a destructor at exit would call into a
// HIP runtime that may already have shut down
PackDev &g_pack = *new PackDev;
std::mutex g_pack_mu;
}  // namespace

namespace {
int64_t write_dev(int device, const uint8_t *seq, int64_t seq_n, const uint8_t *qual, int64_t qual_n, BamWriteJob job,
                  const ModsTables *mods, const MovesTables *moves, const std::function<void(BamWriteJob *)> *layout,
                  const std::function<void(const uint8_t *, int64_t)> &sink) {
    std::lock_guard<std::mutex> lk(g_pack_mu);
    if (device < 0) PCABI_TRY(hipGetDevice(&device));
    if (g_pack.device >= 0 && g_pack.device != device) {
        (void)hipSetDevice(g_pack.device);
        g_pack.st.release();
        g_pack.remap.release();
        g_pack = PackDev();
    }
    PCABI_TRY(hipSetDevice(device));
    g_pack.device = device;
    if (!g_pack.st)
        if (int rc = g_pack.st.create()) return rc;
    if (int rc = g_pack.d_len.reserve(8, 8)) return rc;
    hipStream_t st = g_pack.st;
    // the letters first: the remap counts them where the pack reads them
    if (int rc = g_pack.buf[0].reserve(seq_n + 64, std::max<int64_t>(seq_n + 64 + seq_n / 4, 1 << 20))) return rc;
    if (seq_n > 0) PCABI_TRY(hipMemcpyAsync(g_pack.buf[0], seq, (size_t)seq_n, hipMemcpyHostToDevice, st));
    // the tags to remap are sized in one round trip
    if (int rc = g_pack.remap.plan(device, st, seq, g_pack.buf[0], seq_n, mods, moves)) return rc;
    if (mods || moves) (*layout)(&job);
    const uint8_t *head = job.head, *side = job.side;
    const pcabi_bam_part *parts = job.parts;
    const int64_t head_n = job.head_n, side_n = job.side_n, n_parts = job.n_parts, n_tiles = job.n_tiles, stream_n = job.stream_n;
    if (stream_n <= 0) return 0;
    const int64_t block = PCABI_BGZF_BLOCK_CAP;
    const int64_t z_cap = pcabi_bgzf_bound(stream_n, std::max<int64_t>((stream_n + block - 1) / block, 1), 0);
    const int64_t sc = pcabi_bgzf_scratch_bytes(stream_n, block);
    if (z_cap < 0 || sc < 0) return z_cap < 0 ? z_cap : sc;
    const int64_t need[6] = {seq_n + 64, qual_n + 64, side_n + 64, n_parts * (int64_t)sizeof(pcabi_bam_part) + 64,
                             stream_n + 64, z_cap + 64};
    for (int k = 1; k < 6; ++k)
        if (int rc = g_pack.buf[k].reserve(need[k], std::max<int64_t>(need[k] + need[k] / 4, 1 << 20))) return rc;
    if (int rc = g_pack.scratch.reserve(sc, sc + sc / 4)) return rc;
    uint8_t *d_seq = g_pack.buf[0], *d_qual = g_pack.buf[1], *d_side = g_pack.buf[2], *d_stream = g_pack.buf[4],
            *d_z = g_pack.buf[5];
    pcabi_bam_part *d_parts = (pcabi_bam_part *)g_pack.buf[3].p;
    if (qual_n > 0) PCABI_TRY(hipMemcpyAsync(d_qual, qual, (size_t)qual_n, hipMemcpyHostToDevice, st));
    if (side_n > 0) PCABI_TRY(hipMemcpyAsync(d_side, side, (size_t)side_n, hipMemcpyHostToDevice, st));
    if (n_parts > 0)
        PCABI_TRY(hipMemcpyAsync(d_parts, parts, (size_t)n_parts * sizeof(pcabi_bam_part), hipMemcpyHostToDevice, st));
    if (head_n > 0) PCABI_TRY(hipMemcpyAsync(d_stream, head, (size_t)head_n, hipMemcpyHostToDevice, st));
    if (int rc = g_pack.remap.write(st, mods, moves, d_side, side_n)) return rc;
    const bool prof = prof_on();
    void *sp = prof ? prof_begin(st, 4) : nullptr;
    if (int rc = launch_pack(st, d_seq, seq_n, d_qual, qual_n, d_side, side_n, d_parts, n_parts, n_tiles, d_stream, stream_n))
        return rc;
    if (prof) {
        prof_end(st, sp);
        std::lock_guard<std::mutex> pk(g_prof_mu);
        for (int64_t i = 0; i < n_parts; ++i) g_pack_bytes += 2 * (int64_t)parts[i].l_seq + part_size(parts[i]);
        g_pack_bytes += n_parts * (int64_t)sizeof(pcabi_bam_part);
    }
    if (int rc = pcabi_bgzf_dev(st, d_stream, stream_n, block, d_z, z_cap, g_pack.d_len, g_pack.scratch, g_pack.scratch.cap))
        return rc;
    int64_t zn = 0;
    PCABI_TRY(hipMemcpyAsync(&zn, g_pack.d_len, 8, hipMemcpyDeviceToHost, st));
    PCABI_TRY(hipStreamSynchronize(st));
    if (zn < 0 || zn > z_cap) return fail(PCABI_E_DEVICE, "the BGZF encoder refused the stream");
    if (int rc = g_pack.p_z.reserve(zn, std::max<int64_t>(zn + zn / 4, 1 << 20))) return rc;
    if (zn > 0) PCABI_TRY(hipMemcpyAsync(g_pack.p_z, d_z, (size_t)zn, hipMemcpyDeviceToHost, st));
    PCABI_TRY(hipStreamSynchronize(st));
    sink(g_pack.p_z, zn);
    return zn;
}
}  // namespace

int64_t bam_write_dev(int device, const uint8_t *head, int64_t head_n, const uint8_t *seq, int64_t seq_n, const uint8_t *qual,
                      int64_t qual_n, const uint8_t *side, int64_t side_n, const pcabi_bam_part *parts, int64_t n_parts,
                      int64_t n_tiles, int64_t stream_n, const std::function<void(const uint8_t *, int64_t)> &sink) {
    BamWriteJob job;
    job.head = head, job.head_n = head_n, job.side = side, job.side_n = side_n;
    job.parts = parts, job.n_parts = n_parts, job.n_tiles = n_tiles, job.stream_n = stream_n;
    return write_dev(device, seq, seq_n, qual, qual_n, job, nullptr, nullptr, nullptr, sink);
}

int64_t bam_write_tags_dev(int device, const uint8_t *seq, int64_t seq_n, const uint8_t *qual, int64_t qual_n, const ModsTables *mods,
                           const MovesTables *moves, const std::function<void(BamWriteJob *)> &layout,
                           const std::function<void(const uint8_t *, int64_t)> &sink) {
    return write_dev(device, seq, seq_n, qual, qual_n, BamWriteJob(), mods, moves, &layout, sink);
}

void prof_add_bytes(int kind, int64_t bytes) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (kind == 5 || kind == 6) g_mods_bytes += bytes;
    if (kind >= 7 && kind <= 10) g_moves_bytes += bytes;
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
    PCABI_TRY(hipSetDevice(device));
    // every output sits between 64 guard bytes on the device, checked after the kernel; bytes no record
    // owns go up and come back as they were
    constexpr int64_t kGuard = 64;
    uint8_t *host_out[3] = {seq, qual, codes};
    const int64_t caps[3] = {seq_cap, qual_cap, codes_cap};
    std::vector<uint8_t> stage[3];
    DevBuf<> d_bam, d_out[3];
    DevBuf<pcabi_bam_rec> d_recs;
    int rc = d_bam.reserve(n + 64, n + 64);
    if (!rc) rc = d_recs.reserve(n_recs + 1, n_recs + 1);
    auto step = [&](hipError_t e, const char *what) {
        if (!rc && e != hipSuccess) rc = fail(PCABI_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
    };
    if (!rc && n > 0) step(hipMemcpy(d_bam, bam, (size_t)n, hipMemcpyHostToDevice), "hipMemcpy");
    if (!rc && n_recs > 0)
        step(hipMemcpy(d_recs, recs, (size_t)n_recs * sizeof(pcabi_bam_rec), hipMemcpyHostToDevice), "hipMemcpy");
    int64_t base[3];   // the device output starts as far off a 16-byte boundary as the caller's pointer
    for (int o = 0; o < 3; ++o) {
        base[o] = kGuard + (int64_t)((uintptr_t)host_out[o] & 15u);
        stage[o].assign((size_t)(base[o] + caps[o] + kGuard), 0xA5);
        if (caps[o] > 0) std::memcpy(stage[o].data() + base[o], host_out[o], (size_t)caps[o]);
        if (!rc) rc = d_out[o].reserve((int64_t)stage[o].size(), (int64_t)stage[o].size());
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
    return rc;
}

void pcabi_bam_last_times(int on, int reset, double *ms, int64_t *bytes) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    harvest();
    if (ms)
        for (int k = 0; k < 4; ++k) ms[k] = g_ms[k];
    if (bytes) *bytes = g_unpack_bytes;
    if (reset) {
        for (int k = 0; k < 4; ++k) g_ms[k] = 0;
        g_unpack_bytes = 0;
    }
    if (on >= 0) g_prof = on != 0;
}

int64_t pcabi_bam_pack_plan(pcabi_bam_part *parts, int64_t n_parts, int64_t out0, int64_t *tiles) {
    if (n_parts < 0 || (n_parts > 0 && !parts) || out0 < 0) return fail(PCABI_E_ARG, "bad arguments");
    PackLayout lay;
    lay.out = out0;
    for (int64_t i = 0; i < n_parts; ++i) {
        if (parts[i].l_seq < 0 || parts[i].name_len < 0 || parts[i].name_len > kMaxName || parts[i].aux_len < 0)
            return fail(PCABI_E_ARG, "part " + std::to_string(i) + ": lengths >= 0, a name of at most 254 bytes");
        lay.place(&parts[i]);
    }
    if (tiles) *tiles = lay.tiles;
    return lay.out;
}

int pcabi_bam_pack_dev(void *stream, const uint8_t *seq, int64_t seq_n, const uint8_t *qual, int64_t qual_n,
                       const uint8_t *side, int64_t side_n, const pcabi_bam_part *parts, int64_t n_parts,
                       int64_t n_tiles, uint8_t *out, int64_t out_cap) {
    if (seq_n < 0 || qual_n < 0 || side_n < 0 || n_parts < 0 || n_tiles < 0 || out_cap < 0 || (n_parts > 0 && !parts) ||
        (seq_n > 0 && !seq) || (qual_n > 0 && !qual) || (side_n > 0 && !side) || (out_cap > 0 && !out))
        return fail(PCABI_E_ARG, "bad arguments");
    return launch_pack((hipStream_t)stream, seq, seq_n, qual, qual_n, side, side_n, parts, n_parts, n_tiles, out, out_cap);
}

int pcabi_bam_pack_host(int device, const uint8_t *seq, int64_t seq_n, const uint8_t *qual, int64_t qual_n,
                        const uint8_t *side, int64_t side_n, const pcabi_bam_part *parts, int64_t n_parts,
                        uint8_t *out, int64_t out_cap) {
    if (seq_n < 0 || qual_n < 0 || side_n < 0 || n_parts < 0 || out_cap < 0 || (n_parts > 0 && !parts) ||
        (seq_n > 0 && !seq) || (qual_n > 0 && !qual) || (side_n > 0 && !side) || (out_cap > 0 && !out))
        return fail(PCABI_E_ARG, "bad arguments");
    int64_t tiles = 0, end = 0;
    for (int64_t i = 0; i < n_parts; ++i) {
        const pcabi_bam_part &p = parts[i];
        if (!part_fits(p, seq_n, qual_n, side_n, out_cap) || p.tile0 != tiles || p.out < end)
            return fail(PCABI_E_ARG, "part " + std::to_string(i) + " of the table does not fit the buffers");
        tiles += part_tiles(p);
        end = p.out + part_size(p);
    }
    if (device < 0) {
        for (int64_t i = 0; i < n_parts; ++i) pack_part(parts[i], seq, qual, side, out);
        return 0;
    }
    PCABI_TRY(hipSetDevice(device));
    // the output sits between 64 guard bytes on the device, checked after the kernel; bytes no part
    // owns go up and come back as they were
    constexpr int64_t kGuard = 64;
    const int64_t base = kGuard + (int64_t)((uintptr_t)out & 15u);   // as far off a 16-byte boundary as the caller's pointer
    std::vector<uint8_t> stage((size_t)(base + out_cap + kGuard), 0xA5);
    if (out_cap > 0) std::memcpy(stage.data() + base, out, (size_t)out_cap);
    DevBuf<> d_seq, d_qual, d_side, d_parts, d_out;
    int rc = 0;
    auto step = [&](hipError_t e, const char *what) {
        if (!rc && e != hipSuccess) rc = fail(PCABI_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
    };
    auto up = [&](DevBuf<> &d, const void *h, int64_t n) {
        if (!rc) rc = d.reserve(n + 64, n + 64);
        if (!rc && n > 0) step(hipMemcpy(d, h, (size_t)n, hipMemcpyHostToDevice), "hipMemcpy");
    };
    up(d_seq, seq, seq_n);
    up(d_qual, qual, qual_n);
    up(d_side, side, side_n);
    up(d_parts, parts, n_parts * (int64_t)sizeof(pcabi_bam_part));
    up(d_out, stage.data(), (int64_t)stage.size());
    if (!rc)
        rc = launch_pack(nullptr, d_seq, seq_n, d_qual, qual_n, d_side, side_n, (const pcabi_bam_part *)d_parts.p, n_parts, tiles,
                         d_out + base, out_cap);
    if (!rc) step(hipStreamSynchronize(nullptr), "hipStreamSynchronize");
    if (!rc) step(hipMemcpy(stage.data(), d_out, stage.size(), hipMemcpyDeviceToHost), "hipMemcpy");
    for (int64_t g = 0; g < kGuard && !rc; ++g)
        if (stage[(size_t)(base - 1 - g)] != 0xA5 || stage[(size_t)(base + out_cap + g)] != 0xA5)
            rc = fail(PCABI_E_DEVICE, "k_bam_pack wrote outside its output");
    if (!rc && out_cap > 0) std::memcpy(out, stage.data() + base, (size_t)out_cap);
    return rc;
}

void pcabi_bam_pack_last_times(int reset, double *ms, int64_t *bytes) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    harvest();
    if (ms) *ms = g_ms[4];
    if (bytes) *bytes = g_pack_bytes;
    if (reset) {
        g_ms[4] = 0;
        g_pack_bytes = 0;
    }
}

void pcabi_mods_last_times(int reset, double *ms, int64_t *bytes) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    harvest();
    int64_t dev_ns = 0;
    const int64_t host_ns = mods_host_ns(reset, &dev_ns);
    if (ms) ms[0] = g_ms[5], ms[1] = g_ms[6], ms[2] = 1e-6 * (double)host_ns, ms[3] = 1e-6 * (double)dev_ns;
    if (bytes) *bytes = g_mods_bytes;
    if (reset) {
        g_ms[5] = g_ms[6] = 0;
        g_mods_bytes = 0;
    }
}

void pcabi_moves_last_times(int reset, double *ms, int64_t *bytes) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    harvest();
    int64_t dev_ns = 0;
    const int64_t host_ns = moves_host_ns(reset, &dev_ns);
    if (ms) ms[0] = g_ms[7], ms[1] = g_ms[8], ms[2] = g_ms[9], ms[3] = g_ms[10], ms[4] = 1e-6 * (double)host_ns, ms[5] = 1e-6 * (double)dev_ns;
    if (bytes) *bytes = g_moves_bytes;
    if (reset) {
        g_ms[7] = g_ms[8] = g_ms[9] = g_ms[10] = 0;
        g_moves_bytes = 0;
    }
}

}  // extern "C"
