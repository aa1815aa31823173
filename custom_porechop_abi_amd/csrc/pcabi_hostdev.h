// pcabi_hostdev.h -- the host plumbing the file path's device stages share (pcabi_deflate.hip,
// pcabi_inflate.hip, pcabi_bam.hip, pcabi_mods.hip, pcabi_moves.hip, pcabi_auxtext.hip, pcabi_auxparse.hip, pcabi_qual.hip,
// pcabi_io.cpp, pcabi_write.cpp): the error macro, the pinned-memory copy, the clock, the owner of a device
// or pinned buffer, the owner of a stream, the owners of a writer's remap stage, and the declarations of
// every pcabi_internal function that crosses a unit. What names a HIP type sits under __HIPCC__; the rest
// compiles with a plain C++ compiler (pcabi_io.cpp, pcabi_write.cpp, tests/hostdev_main.cpp).
#pragma once

#include <time.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/pcabi.h"

namespace pcabi_bam {
struct Layout;
}

namespace pcabi_internal {

int fail(int code, const std::string &msg);   // pcabi_engine.hip: pcabi_last_error()

inline void par_memcpy(void *dst, const void *src, size_t n) {
    constexpr size_t kPiece = 8u << 20;
    const int nt = (int)std::min<size_t>(4, n / kPiece);
    if (nt <= 1) {
        std::memcpy(dst, src, n);
        return;
    }
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t) {
        const size_t a = n * t / nt, e = n * (t + 1) / nt;
        th.emplace_back([=] { std::memcpy((char *)dst + a, (const char *)src + a, e - a); });
    }
    for (auto &x : th) x.join();
}

inline double now_s() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

// A buffer of T that frees itself: Mem::alloc(void **, bytes) returns 0 or a fail() code, Mem::free(void *)
// releases. cap (in elements) is non-zero only while p is live, so "does it hold n" is a question to the
// allocation itself. The device that must be current when memory goes is the holder's business.
template <class Mem, class T = uint8_t>
struct Owned {
    T *p = nullptr;
    int64_t cap = 0;
    Owned() = default;
    Owned(Owned &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    Owned &operator=(Owned &&o) noexcept {
        if (this != &o) {
            release();
            p = o.p, cap = o.cap;
            o.p = nullptr, o.cap = 0;
        }
        return *this;
    }
    ~Owned() { release(); }
    void release() {
        if (p) Mem::free(p);
        p = nullptr, cap = 0;
    }
    // room for `need` elements: nothing when they fit, else the old block goes first and `want` (the
    // caller's growth rule, >= need) are allocated; a failure leaves {nullptr, 0}
    int reserve(int64_t need, int64_t want) {
        if (need <= cap) return 0;
        release();
        void *q = nullptr;
        if (int rc = Mem::alloc(&q, (size_t)want * sizeof(T))) return rc;
        p = (T *)q, cap = want;
        return 0;
    }
    operator T *() const { return p; }
};

// no two of the spans [first, second) may meet (the outputs of a table's parts); sorts them
inline bool spans_disjoint(std::vector<std::pair<int64_t, int64_t>> &spans) {
    std::sort(spans.begin(), spans.end());
    for (size_t k = 1; k < spans.size(); ++k)
        if (spans[k].first < spans[k - 1].second) return false;
    return true;
}

// may kept buffers serve a call that needs these sizes? holds(owner, need, owner, need, ...)
inline bool holds() { return true; }
template <class O, class... Rest>
bool holds(const O &o, int64_t need, const Rest &...rest) {
    return need <= o.cap && holds(rest...);
}

#ifdef __HIPCC__
#define PCABI_TRY(expr)                                                                     \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return pcabi_internal::fail(PCABI_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

struct DevAlloc {
    static int alloc(void **p, size_t n) {
        PCABI_TRY(hipMalloc(p, n));
        return 0;
    }
    static void free(void *p) { (void)hipFree(p); }
};
struct PinAlloc {
    static int alloc(void **p, size_t n) {
        PCABI_TRY(hipHostMalloc(p, n, hipHostMallocDefault));
        return 0;
    }
    static void free(void *p) { (void)hipHostFree(p); }
};
template <class T = uint8_t>
using DevBuf = Owned<DevAlloc, T>;
template <class T = uint8_t>
using PinBuf = Owned<PinAlloc, T>;

// a non-blocking stream, synchronised and destroyed when it goes
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream &&o) noexcept : s(o.s) { o.s = nullptr; }
    Stream &operator=(Stream &&o) noexcept {
        if (this != &o) {
            release();
            s = o.s;
            o.s = nullptr;
        }
        return *this;
    }
    ~Stream() { release(); }
    int create() {
        release();
        PCABI_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        return 0;
    }
    void release() {
        if (s) {
            (void)hipStreamSynchronize(s);
            (void)hipStreamDestroy(s);
        }
        s = nullptr;
    }
    operator hipStream_t() const { return s; }
};

// Device-event timing of a unit's two kernels (its timing tool's *_last_times entry): off by default.
struct KernelTimes {
    std::mutex mu;
    bool on = false;
    double ms[2] = {0, 0};
    int64_t bytes[2] = {0, 0};
    // the entry point: sets the switch, reports the sums (null pointers: not wanted), clears them
    void last(int on_, int reset, double *ms_out, int64_t *bytes_out) {
        std::lock_guard<std::mutex> lk(mu);
        on = on_ != 0;
        for (int k = 0; k < 2; ++k) {
            if (ms_out) ms_out[k] = ms[k];
            if (bytes_out) bytes_out[k] = bytes[k];
            if (reset) ms[k] = 0, bytes[k] = 0;
        }
    }
};
// events around one kernel on a stream; harvest (the stream idle) adds the time to sum `kind`
struct EventSpan {
    hipEvent_t a = nullptr, b = nullptr;
    bool on = false;
    void begin(KernelTimes &t, hipStream_t st) {
        {
            std::lock_guard<std::mutex> lk(t.mu);
            on = t.on;
        }
        if (!on) return;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess || hipEventRecord(a, st) != hipSuccess) on = false;
    }
    void end(hipStream_t st) {
        if (on && hipEventRecord(b, st) != hipSuccess) on = false;
    }
    void harvest(KernelTimes &t, int kind, int64_t n) {
        float ms = 0;
        if (on && hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&ms, a, b) == hipSuccess) {
            std::lock_guard<std::mutex> lk(t.mu);
            t.ms[kind] += ms;
            t.bytes[kind] += n;
        }
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
        a = b = nullptr, on = false;
    }
};
#endif

// ---- pcabi_inflate.hip ---------------------------------------------------------------------------
std::vector<int64_t> gunzip_passes(const int64_t *out_off, int64_t m0, int64_t m1, int64_t chunk);
int64_t gunzip_chunk_bytes();
int gunzip_group_async(void *stream, const uint8_t *z, const int64_t *in_off, const int64_t *out_off, int64_t m0,
                       int64_t m1, uint8_t *pin_in, int64_t *pin_off, uint8_t *dev_in, int64_t *dev_off,
                       uint8_t *dev_out, int32_t *dev_status, uint8_t *pin_out, int32_t *pin_status);
int gunzip_group_check(const int32_t *pin_status, const int64_t *in_off, int64_t m0, int64_t m1);
// the device source of a block-gzipped input
struct GunzipReader;
int gunzip_reader_open(const uint8_t *z, int64_t n, int device, GunzipReader **out);
int64_t gunzip_reader_read(GunzipReader *g, char *dst, int64_t room);
int64_t gunzip_reader_take(GunzipReader *g, const uint8_t **host, const uint8_t **dev, void **stream);
void gunzip_reader_unread(GunzipReader *g);
int gunzip_reader_device(const GunzipReader *g);
int64_t gunzip_reader_total(const GunzipReader *g);
void gunzip_reader_close(GunzipReader *g);

// ---- pcabi_gzstream.hip --------------------------------------------------------------------------
// the device source of a gzip input without an index (z stays mapped until close)
struct GzStreamReader;
int gzstream_reader_open(const uint8_t *z, int64_t n, int device, GzStreamReader **out);
int64_t gzstream_reader_read(GzStreamReader *g, char *dst, int64_t room);
void gzstream_reader_close(GzStreamReader *g);

// ---- pcabi_bam.hip -------------------------------------------------------------------------------
// device-event spans of the BAM timing tool: no-ops unless profiling is on
bool prof_on();
void *prof_begin(void *stream, int kind);
void prof_end(void *stream, void *span);
// the device half of a BAM reader
struct BamDev;
int bam_dev_open(int device, BamDev **out);
void bam_dev_close(BamDev *b);
int bam_dev_append(BamDev *b, int64_t keep_from, const uint8_t *src, int64_t n, void *stream);
int bam_dev_unpack(BamDev *b, const pcabi_bam_rec *recs, int64_t n_recs, const pcabi_bam::Layout &lay,
                   const uint8_t **seq, const uint8_t **qual, const uint8_t **codes);
// the device half of the BAM writer: the stream packed and compressed on the device; sink receives its
// members (pinned memory, valid inside the call)
int64_t bam_write_dev(int device, const uint8_t *head, int64_t head_n, const uint8_t *seq, int64_t seq_n, const uint8_t *qual,
                      int64_t qual_n, const uint8_t *side, int64_t side_n, const pcabi_bam_part *parts, int64_t n_parts,
                      int64_t n_tiles, int64_t stream_n, const std::function<void(const uint8_t *, int64_t)> &sink);
// The same with modification tags to remap (pcabi_mods.hip): the letters go up once, the device sizes
// the parts' tags (mods->parts[].len, mods->usable), `layout` then builds the side blob with a gap
// behind each part's kept tags, sets mods->parts[].out to the gaps and fills the job; the gaps are
// filled in the device copy of the blob before k_bam_pack runs.
struct BamWriteJob {
    const uint8_t *head = nullptr, *side = nullptr;
    const pcabi_bam_part *parts = nullptr;
    int64_t head_n = 0, side_n = 0, n_parts = 0, n_tiles = 0, stream_n = 0;
};
// the tags to remap, of either kind: the tag blob, the tables, the reads' flags (ModsTables: pcabi_mods.hip,
// MovesTables: pcabi_moves.hip)
template <class Read, class Part>
struct TagTables {
    const uint8_t *tags = nullptr;
    int64_t tags_n = 0;
    const Read *reads = nullptr;
    int64_t n_reads = 0;
    Part *parts = nullptr;
    int64_t n_parts = 0;
    uint8_t *usable = nullptr;
};
using ModsTables = TagTables<pcabi_mods_read, pcabi_mods_part>;
using MovesTables = TagTables<pcabi_moves_read, pcabi_moves_part>;
// mods and moves: either may be null, not both; the two are sized in one round trip before `layout` runs
int64_t bam_write_tags_dev(int device, const uint8_t *seq, int64_t seq_n, const uint8_t *qual, int64_t qual_n, const ModsTables *mods,
                           const MovesTables *moves, const std::function<void(BamWriteJob *)> &layout,
                           const std::function<void(const uint8_t *, int64_t)> &sink);
// 5 k_mods_plan, 6 k_mods_write; 7 the move tables' sizing stages, 10 k_moves_write
void prof_add_bytes(int kind, int64_t bytes);

// ---- pcabi_io.cpp --------------------------------------------------------------------------------
int io_thread_count();   // the threads a host stage fans out to (PCABI_IO_THREADS)

// ---- pcabi_mods.hip ------------------------------------------------------------------------------
// the device half of the remap: the tag blob, the tables and the scratch tables of the plan before
struct ModsDev;
// the host build's tables, kept from its sizing pass (device < 0) for its writing pass
struct ModsHost;
// device < 0: the host build; else dev / stream / d_seq name the device side. Checks the tables
// (PCABI_E_ARG), fills parts[].len and usable[], counts the reads.
int mods_plan_any(int device, ModsDev *dev, ModsHost *keep, void *stream, const uint8_t *seq, const uint8_t *d_seq, int64_t seq_n,
                  const ModsTables &t);
int mods_dev_plan(ModsDev *d, void *stream, const uint8_t *d_seq, int64_t seq_n, const ModsTables &t);
int mods_dev_write(ModsDev *d, void *stream, const pcabi_mods_part *parts, int64_t n_parts, uint8_t *d_out, int64_t out_cap);
void mods_write_host(ModsHost *keep, const uint8_t *seq, const ModsTables &t, uint8_t *out);
ModsHost *mods_host_new();
void mods_host_free(ModsHost *h);
ModsDev *mods_dev_new();
// wall time the host build took, and the device plan step (copies up, kernel, lengths back): pcabi_mods_last_times
int64_t mods_host_ns(int reset, int64_t *dev_plan_ns);
void mods_dev_free(ModsDev *d);   // its device current


// ---- pcabi_moves.hip -----------------------------------------------------------------------------
// the device half of the move-table remap: the tag blob, the tables, the segment prefixes and every
// part boundary's move of the plan before
struct MovesDev;
// the host build's part boundaries, kept from its sizing pass for its writing pass
struct MovesHost;
int moves_check(const MovesTables &t);   // the tables against the blob and each other (PCABI_E_ARG)
// the host build: checks the tables, fills parts[].len and usable[], counts the reads; then the bytes
int moves_plan_host(MovesHost *keep, const MovesTables &t);
void moves_write_host(MovesHost *keep, const MovesTables &t, uint8_t *out);
// the device: begin queues the sizing on `stream` (tables checked before), end waits and fills
// parts[].len and usable[] and counts; write fills the parts' bytes into d_out, asynchronous
int moves_dev_plan_begin(MovesDev *d, void *stream, const MovesTables &t);
int moves_dev_plan_end(MovesDev *d, void *stream, const MovesTables &t);
int moves_dev_write(MovesDev *d, void *stream, const pcabi_moves_part *parts, int64_t n_parts, uint8_t *d_out, int64_t out_cap);
MovesHost *moves_host_new();
void moves_host_free(MovesHost *h);
MovesDev *moves_dev_new();
void moves_dev_free(MovesDev *d);   // its device current
int64_t moves_host_ns(int reset, int64_t *dev_plan_ns);   // pcabi_moves_last_times

// ---- the remap stage of a writer: both kinds of tags sized, then written into the side blob's gaps ----
// (mods / moves: the tables of the kind, null when the batch has none to remap)
struct RemapFree {
    void operator()(ModsHost *h) const { mods_host_free(h); }
    void operator()(MovesHost *h) const { moves_host_free(h); }
    void operator()(ModsDev *d) const { mods_dev_free(d); }
    void operator()(MovesDev *d) const { moves_dev_free(d); }
};
// The host build: plan() sizes the parts' tags (parts[].len, usable[]) and returns the first non-zero
// code; write() fills the gaps the caller then laid out (parts[].out) in side and lets the plan go.
struct RemapHost {
    std::unique_ptr<ModsHost, RemapFree> mh;
    std::unique_ptr<MovesHost, RemapFree> vh;
    const uint8_t *seq = nullptr;
    const ModsTables *mods = nullptr;
    const MovesTables *moves = nullptr;
    int plan(const uint8_t *seq_, int64_t seq_n, const ModsTables *mods_, const MovesTables *moves_) {
        seq = seq_, mods = mods_, moves = moves_;
        if (mods) {
            mh.reset(mods_host_new());
            if (int rc = mods_plan_any(-1, nullptr, mh.get(), nullptr, seq, nullptr, seq_n, *mods)) return rc;
        }
        if (moves) {
            vh.reset(moves_host_new());
            if (int rc = moves_plan_host(vh.get(), *moves)) return rc;
        }
        return 0;
    }
    void write(uint8_t *side) {
        if (mods) mods_write_host(mh.get(), seq, *mods, side);
        if (moves) moves_write_host(vh.get(), *moves, side);
        mh.reset(), vh.reset();
    }
};
// The device: kept by a writer's device side between calls, made at its first use. plan() sizes both kinds
// in one round trip on `stream` (the letters lie at d_seq already): the move tables' stages are queued, the
// modification tags' plan runs behind them and waits for the stream, then the lengths are read. write()
// queues the kernels that fill the gaps of the blob's device copy. release(): its device current.
struct RemapDev {
    std::unique_ptr<ModsDev, RemapFree> md;
    std::unique_ptr<MovesDev, RemapFree> vd;
    int plan(int device, void *stream, const uint8_t *seq, const uint8_t *d_seq, int64_t seq_n, const ModsTables *mods,
             const MovesTables *moves) {
        if (moves) {
            if (!vd) vd.reset(moves_dev_new());
            if (int rc = moves_check(*moves)) return rc;
            if (int rc = moves_dev_plan_begin(vd.get(), stream, *moves)) return rc;
        }
        if (mods) {
            if (!md) md.reset(mods_dev_new());
            if (int rc = mods_plan_any(device, md.get(), nullptr, stream, seq, d_seq, seq_n, *mods)) return rc;
        }
        return moves ? moves_dev_plan_end(vd.get(), stream, *moves) : 0;
    }
    int write(void *stream, const ModsTables *mods, const MovesTables *moves, uint8_t *d_side, int64_t side_n) {
        if (mods)
            if (int rc = mods_dev_write(md.get(), stream, mods->parts, mods->n_parts, d_side, side_n)) return rc;
        return moves ? moves_dev_write(vd.get(), stream, moves->parts, moves->n_parts, d_side, side_n) : 0;
    }
    void release() { md.reset(), vd.reset(); }
};

// ---- pcabi_deflate.hip ---------------------------------------------------------------------------
// pcabi_bgzf_dev with a block list (device pointer, n_blocks + 1 entries, every block 1..65280 bytes):
// one BGZF member per block; scratch of pcabi_gzip_scratch_bytes(n, n_blocks)
int bgzf_dev_blocks(void *stream, const uint8_t *in, int64_t n, const int64_t *block_off, int64_t n_blocks, uint8_t *out,
                    int64_t cap, int64_t *out_len, void *scratch, int64_t scratch_len);

// ---- pcabi_auxtext.hip ---------------------------------------------------------------------------
// The device half of the text writer with tags in the headers (pcabi_reads_write_tags, gz = 2 / 3): the
// letters go up, the remapped tags are sized as for BAM output, `layout` then builds the side blob with
// its gaps, sets the tables' out to the gaps and fills the job (the parts without text_len / out /
// tile0; kept[i] = the bytes of part i's chain that lie before its gaps); the gaps are filled in the
// device copy of the blob, the chains' texts sized there, the records and the deflate blocks planned
// on the host, the text laid out and compressed on the device; sink receives the compressed bytes
// (pinned memory, valid inside the call). Returns their length or a negative code.
struct FastxWriteJob {
    const uint8_t *side = nullptr;
    int64_t side_n = 0;
    pcabi_fastx_part *parts = nullptr;
    const int32_t *kept = nullptr;
    int64_t n_parts = 0;
};
int64_t fastx_write_tags_dev(int device, const uint8_t *seq, int64_t seq_n, const uint8_t *qual, int64_t qual_n, const ModsTables *mods,
                             const MovesTables *moves, bool fasta, bool bgzf, const std::function<void(FastxWriteJob *)> &layout,
                             const std::function<void(const uint8_t *, int64_t)> &sink);

// ---- pcabi_auxparse.hip --------------------------------------------------------------------------
// The device side of a reader that parses its headers' tags (pcabi_fastx_header_tags): a stream and the
// buffers kept between batches.
struct AuxParseDev;
AuxParseDev *auxparse_dev_new();
void auxparse_dev_free(AuxParseDev *d);
// The chains of the n headers text[off[i], off[i + 1]), back to back in *aux with their offsets in
// *aux_off (n + 1 entries); counts the tags. device >= 0: the blob goes up once, both kernels run on d's
// stream, the chains and the floats' fix-ups come back; device < 0: the host build on the io threads
// (d may be null).
int auxparse_headers(int device, AuxParseDev *d, const uint8_t *text, const int64_t *off, int64_t n, std::vector<uint8_t> *aux,
                     std::vector<int64_t> *aux_off);

}  // namespace pcabi_internal
