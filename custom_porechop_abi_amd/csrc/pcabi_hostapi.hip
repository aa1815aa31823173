// pcabi_hostapi.hip -- the host-buffer entry points of include/pcabi.h: the calls that take host
// arrays, stage them on a device, run the device ABI and bring the answers back. The Python drivers,
// the reference job and the legacy drop-in (adapterAlignment, check_compatibility) go through here.
//
// Per device there is one Engine: a mutex (the legacy ABI is called concurrently from the
// reference's ThreadPool workers, porechop_abi.py:228,418,504), a stream and the buffers kept from
// call to call. An entry validates its arguments (before any HIP call), opens a Session, and runs a
// sequence of named steps over the Engine.
//
// What this unit needs from the engine (pcabi_engine.hip): the public device ABI -- prepared tables
// (pcabi_adapters_create_scored), pcabi_align_cross_multi_dev, the decision epilogues
// (pcabi_end_trim_dev, pcabi_best_full_identity_dev, pcabi_flag_list_dev, pcabi_middle_cuts_dev,
// pcabi_barcode_call_dev) and the middle scan (pcabi_middle_scan_dev) -- and, for the pairs / cross
// launches of pcabi_align_host over its own bucket tables, what pcabi_host.h declares: the bucket
// layout (BucketHost, build_buckets, needs_striped, check_adapter_lens), the per-bucket launch
// choices (bucket_pack_mode, bucket_shift), dispatch, ForkJoin, the tile layout and first_hit_from.
// Kernels here are the ones only this layer uses: k_orient, k_unpack_codes, k_full_ids, k_list_pack.
#include <hip/hip_runtime.h>

#include <immintrin.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/pcabi.h"
#include "pcabi_dp.h"
#include "pcabi_kern.h"
#include "pcabi_host.h"

using namespace pcabi_eng;
using pcabi_internal::PinBuf;

namespace {

// ---- per-device state ------------------------------------------------------------------------------

struct Event {
    hipEvent_t e = nullptr;
    ~Event() {
        if (e) (void)hipEventDestroy(e);
    }
};

// The regions of one byte buffer, in order: take<T>(n) is the next n elements of T, from the next
// multiple of `align` bytes (the buffers start 256-byte aligned).
struct Carve {
    char *p;
    template <class T>
    T *take(size_t n, size_t align = 1) {
        p = (char *)(((uintptr_t)p + align - 1) & ~(uintptr_t)(align - 1));
        T *r = (T *)p;
        p += sizeof(T) * n;
        return r;
    }
};

constexpr int kStageSlots = 4;

struct Engine {
    std::mutex mu;
    bool init = false;
    hipStream_t stream = nullptr;
    // pcabi_align_host and its kin, the middle-scan entries: windows, results, pair tasks, tiles, epilogues
    Scratch<uint8_t> codes;
    Scratch<int64_t> woff, toff;
    Scratch<int32_t> wlen, out, tasks_win, tasks_out, wave_adp, hits;
    Scratch<uint32_t> tiles;
    Scratch<double> best;
    Scratch<uint32_t> pad[kNumBuckets];   // the call's own bucket tables
    Scratch<int32_t> len[kNumBuckets], id[kNumBuckets];
    Scratch<uint8_t> bc;          // pcabi_middle_cuts_host / pcabi_barcode_call_host: one block, carved
    pcabi_scan *scan = nullptr;   // scratch of the middle scan (pcabi_middle_scan_host)
    // pcabi_end_decisions_host: both sides' windows, results, flags, trims and lists
    struct EndSide {
        Scratch<int64_t> off, toff;
        Scratch<int32_t> len, res;
        Scratch<uint32_t> tiles;
        Scratch<uint8_t> flag;
    };
    struct EndDec {
        Scratch<uint8_t> codes;
        EndSide side[2];
        Scratch<int32_t> trims;     // start trims, end trims
        Scratch<int32_t> lists;     // per side 7 rows x (reads x adapters): they never overflow there
        Scratch<uint8_t> counts;    // one block, carved: list counts, barcode selection, its identities
        Scratch<uint32_t> packed;   // the compact lists on their way to the host
    } dec;
    // stage_seqs: pinned slots the host strings are encoded into while the previous slots' copies run
    // (allocated on first use, kept), and their device copies (2-bit codes + N masks)
    struct StageSlot {
        PinBuf<uint8_t> buf;
        Event ev;
    } stage[kStageSlots];
    Scratch<uint8_t> stage_dev;
    // the two sides' prepared adapter tables, kept while the adapters and the scoring stay the same
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

int check_device(int device) { return device < 0 || device >= 16 ? fail(PCABI_E_ARG, "bad device index") : 0; }

// A device's engine opened for one call: locked, initialised on first use, its device current.
struct Session {
    Engine *eng = nullptr;
    std::unique_lock<std::mutex> lock;
    int open(int device) {
        if (int rc = check_device(device)) return rc;
        eng = &g_engines[device];
        lock = std::unique_lock<std::mutex>(eng->mu);
        if (int rc = engine_init(*eng, device)) return rc;
        HIP_TRY(hipSetDevice(device));
        return 0;
    }
};

template <class T>
int h2d(T *dst, const T *src, size_t n, hipStream_t st) {
    HIP_TRY(hipMemcpyAsync(dst, src, sizeof(T) * n, hipMemcpyHostToDevice, st));
    return 0;
}
template <class T>
int d2h(T *dst, const T *src, size_t n, hipStream_t st) {
    HIP_TRY(hipMemcpyAsync(dst, src, sizeof(T) * n, hipMemcpyDeviceToHost, st));
    return 0;
}

// ---- argument checks ---------------------------------------------------------------------------------

// windows [off, off + len) of a buffer of codes_len bytes that ends in 16 bytes of padding
int check_windows(const int64_t *off, const int32_t *len, int64_t n, int64_t codes_len) {
    for (int64_t w = 0; w < n; ++w) {
        if (len[w] < 0 || len[w] > pcabi::MAX_WINDOW_LEN) return fail(PCABI_E_ARG, "window length out of range");
        if (len[w] > 0 && (off[w] < 0 || off[w] + len[w] + 16 > codes_len))
            return fail(PCABI_E_ARG, "window outside the buffer or buffer not padded by 16 bytes");
    }
    return 0;
}

// The layout of n strings as a window buffer (and of the Python SeqPack): windows back to back from
// 4-aligned offsets off[0..n), N between them and 16 N bytes after the last; *total = its bytes.
int seq_layout(const char *const *seqs, const int32_t *len, int64_t n, int64_t *off, int64_t *total) {
    int64_t at = 0;
    for (int64_t w = 0; w < n; ++w) {
        if (len[w] < 0 || len[w] > pcabi::MAX_WINDOW_LEN) return fail(PCABI_E_ARG, "window length out of range");
        if (len[w] > 0 && !seqs[w]) return fail(PCABI_E_ARG, "NULL sequence");
        off[w] = at;
        at += ((int64_t)len[w] + 3) & ~(int64_t)3;
    }
    *total = at + 16;
    return 0;
}

// ---- host strings -> Dna5 codes on the device ------------------------------------------------------------
// The layout's bytes [0, total) in chunks of kStageBytes. What crosses PCIe is 3 bits a base, not 8:
// each chunk travels as 2-bit codes (base j of a 32-base block at bits 2j of its 8 bytes) plus a
// 1-bit "not A/C/G/T/U" mask (bit j of the block's 32-bit word), k_unpack_codes writes the Dna5 bytes
// (S/basic/alphabet_residue_tabs.h's table, as pcabi_encode_dna5: A/a 0, C/c 1, G/g 2, T/t/U/u 3,
// anything else N = 4) into dst. The worker threads gather their share of a chunk's characters (the
// windows' own bytes, N between them) into a thread-local block and encode it with AVX2 (a scalar
// loop without it) into one of four pinned slots; the calling thread queues each chunk's two copies
// and its unpack on the engine's stream and waits for a slot only when a worker needs it again.
// Nothing is written to pageable memory.
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

// One stage_seqs call as its worker threads see it.
struct StageJob {
    const char *const *seqs;
    const int32_t *len;
    const int64_t *off;
    int64_t n, total, n_chunk;
    int nt;                                   // worker threads
    bool avx2;
    uint8_t *slot[kStageSlots];
    std::unique_ptr<std::atomic<int>[]> left; // per chunk: workers still encoding it
    std::atomic<int64_t> free_upto{0};        // chunks below it may be encoded
    std::atomic<bool> stop{false};

    // characters [b0, b1) of the layout into raw (windows' bytes, 'N' between them)
    void gather(int64_t b0, int64_t b1, uint8_t *raw) const {
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
    }

    // worker t: its share of every chunk, as soon as the chunk's slot is free
    void work(int t) {
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
            uint8_t *s = slot[c % kStageSlots];
            for (int64_t k = k0; k < k1; k += kBlk / 32) {
                const int64_t ke = std::min(k1, k + kBlk / 32);
                const int64_t b0 = c0 + 32 * k, b1 = std::min(c1, c0 + 32 * ke);
                gather(b0, b1, raw.get());
                if (b1 - b0 < 32 * (ke - k)) std::memset(raw.get() + (b1 - b0), 'N', (size_t)(32 * (ke - k) - (b1 - b0)));
                uint8_t *codes = s + 8 * k;
                uint32_t *mask = reinterpret_cast<uint32_t *>(s + kStageCodes) + k;
                if (avx2) pack_avx2(raw.get(), ke - k, codes, mask);
                else
                    for (int64_t q = 0; q < ke - k; ++q) pack32_scalar(raw.get() + 32 * q, codes + 8 * q, mask + q);
            }
            left[c].fetch_sub(1, std::memory_order_release);
        }
    }
};

// the pinned slots and their device copies, with no copy of an earlier call left in flight
int stage_slots(Engine &e) {
    for (Engine::StageSlot &s : e.stage) {
        if (!s.buf.p) {
            if (int rc = s.buf.reserve(kStageSlot, kStageSlot)) return rc;
            HIP_TRY(hipEventCreateWithFlags(&s.ev.e, hipEventDisableTiming));
        }
        // a call that failed after staging may have left copies out of a slot in flight
        HIP_TRY(hipEventSynchronize(s.ev.e));
    }
    return e.stage_dev.ensure(kStageSlots * kStageSlot);
}

// chunk c (encoded in its slot): its two copies, the slot's event, its unpack into dst
hipError_t stage_queue_chunk(Engine &e, uint8_t *dst, int64_t c, int64_t total) {
    const int64_t c0 = c * kStageBytes, c1 = std::min(total, c0 + kStageBytes);
    const int64_t nb = (c1 - c0 + 31) / 32;
    const int s = (int)(c % kStageSlots);
    const uint8_t *src = e.stage[s].buf.p;
    uint8_t *dslot = e.stage_dev.p + s * kStageSlot;
    hipError_t he = hipMemcpyAsync(dslot, src, (size_t)(8 * nb), hipMemcpyHostToDevice, e.stream);
    if (he == hipSuccess)
        he = hipMemcpyAsync(dslot + kStageCodes, src + kStageCodes, (size_t)(4 * nb), hipMemcpyHostToDevice, e.stream);
    if (he == hipSuccess) he = hipEventRecord(e.stage[s].ev.e, e.stream);
    if (he != hipSuccess) return he;
    const int64_t nq = (c1 - c0 + 15) / 16;
    hipLaunchKernelGGL(k_unpack_codes, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, e.stream,
                       (const uint32_t *)dslot, (const uint32_t *)(dslot + kStageCodes), dst + c0, c1 - c0);
    return hipGetLastError();
}

int stage_seqs(Engine &e, uint8_t *dst, const char *const *seqs, const int32_t *len, const int64_t *off, int64_t n,
               int64_t total) {
    if (int rc = stage_slots(e)) return rc;
    StageJob job{seqs, len, off, n, total};
    // PCABI_STAGE_SCALAR=1: the scalar encoder (the form used without AVX2), for its test
    const char *sc_env = std::getenv("PCABI_STAGE_SCALAR");
    job.avx2 = __builtin_cpu_supports("avx2") && !(sc_env && sc_env[0] == '1');
    const int64_t n_chunk = job.n_chunk = (total + kStageBytes - 1) / kStageBytes;
    job.nt = (int)std::max<int64_t>(1, std::min<int64_t>({16, (int64_t)std::thread::hardware_concurrency(),
                                                          total / (1 << 20)}));
    for (int k = 0; k < kStageSlots; ++k) job.slot[k] = e.stage[k].buf.p;
    job.left.reset(new std::atomic<int>[(size_t)n_chunk]);
    for (int64_t c = 0; c < n_chunk; ++c) job.left[c].store(job.nt);
    int64_t freed = std::min<int64_t>(kStageSlots, n_chunk);   // chunks [0, freed) have a slot
    job.free_upto.store(freed);
    std::vector<std::thread> th;
    for (int t = 0; t < job.nt; ++t) th.emplace_back([&job, t] { job.work(t); });
    hipError_t he = hipSuccess;
    for (int64_t c = 0; c < n_chunk && he == hipSuccess; ++c) {
        while (job.left[c].load(std::memory_order_acquire) > 0) std::this_thread::yield();
        he = stage_queue_chunk(e, dst, c, total);
        // hand the workers the slot of the oldest copy still queued once it has landed, keeping
        // kStageSlots - 1 chunks queued or being encoded behind it (the device slot is reused in
        // stream order: its next copy follows this chunk's unpack)
        const int64_t oldest = c - (kStageSlots - 2);
        if (he == hipSuccess && oldest >= 0 && freed < n_chunk) {
            he = hipEventSynchronize(e.stage[oldest % kStageSlots].ev.e);
            if (he == hipSuccess) {
                freed = std::min<int64_t>(n_chunk, oldest + kStageSlots);
                job.free_upto.store(freed, std::memory_order_release);
            }
        }
    }
    job.stop.store(true);
    for (auto &t : th) t.join();
    if (he != hipSuccess) return fail(PCABI_E_DEVICE, std::string("staging copy: ") + hipGetErrorString(he));
    return 0;
}

// ---- pcabi_align_host and the entries built on it ----------------------------------------------------

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

// What leaves the device after the alignments.
enum class Epilogue {
    Results,       // out: the PCABI_NFIELDS result rows
    CompatFlags,   // out: one check_compatibility flag per task
    FirstHits,     // out: the k_first_hit fields (5 x n_win) at first_thr
    BestHost,      // best[n_adp] (host): max with the full identity, in and out
    BestDev,       // best[n_adp] on the device
    Orient,        // out: the all-vs-all link matrix (n_win == n_adp, flags oriented by k_orient)
};

// Windows x adapters, every pair (cross: task_win == nullptr) or the listed tasks (pairs).
struct AlignArgs {
    int device;
    const uint8_t *codes;
    int64_t codes_len;
    const int64_t *win_off;
    const int32_t *win_len;
    int64_t n_win;
    const uint8_t *adp_codes;
    const int32_t *adp_off, *adp_len;
    int32_t n_adp;
    const int32_t *task_win, *task_adp;
    int64_t n_task;
    pcabi::Scoring sc;
    Epilogue epi;
    int32_t *out;
    double first_thr;
    double *best;
    int64_t n_res() const { return task_win ? n_task : (int64_t)n_adp * n_win; }
    bool flags() const { return epi == Epilogue::CompatFlags || epi == Epilogue::Orient; }
};

int align_validate(const AlignArgs &a) {
    if (int rc = check_device(a.device)) return rc;
    if (a.n_win < 0 || a.n_adp < 0 || a.n_task < 0) return fail(PCABI_E_ARG, "negative count");
    if (int rc = check_adapter_lens(a.adp_len, a.n_adp)) return rc;
    if (int rc = check_windows(a.win_off, a.win_len, a.n_win, a.codes_len)) return rc;
    if (a.task_win)
        for (int64_t t = 0; t < a.n_task; ++t)
            if (a.task_win[t] < 0 || a.task_win[t] >= a.n_win || a.task_adp[t] < 0 || a.task_adp[t] >= a.n_adp)
                return fail(PCABI_E_ARG, "task index out of range");
    return 0;
}

// the windows and the result buffer; p: what every launch of the call shares
int align_stage(Engine &e, const AlignArgs &a, int64_t max_win, KParams &p) {
    if (int rc = e.codes.ensure(a.codes_len)) return rc;
    if (int rc = e.woff.ensure(std::max<int64_t>(a.n_win, 1))) return rc;
    if (int rc = e.wlen.ensure(std::max<int64_t>(a.n_win, 1))) return rc;
    if (int rc = e.out.ensure(PCABI_NFIELDS * a.n_res())) return rc;
    if (int rc = h2d(e.codes.p, a.codes, (size_t)a.codes_len, e.stream)) return rc;
    if (int rc = h2d(e.woff.p, a.win_off, (size_t)a.n_win, e.stream)) return rc;
    if (int rc = h2d(e.wlen.p, a.win_len, (size_t)a.n_win, e.stream)) return rc;
    p.codes = e.codes;
    p.win_off = e.woff;
    p.win_len = e.wlen;
    p.n_win = a.n_win;
    p.out = e.out;
    p.out_stride = a.n_res();
    p.sc = a.sc;
    p.compat = a.flags() ? e.out.p : nullptr;
    p.max_cols = (int32_t)std::min<int64_t>(max_win, INT32_MAX);
    return 0;
}

// bucket b's table into the engine's buffers (kept distinct per bucket: the launches of a call run
// side by side) and into p
int upload_bucket(Engine &e, int b, const BucketHost &h, KParams &p) {
    const size_t nb = h.len.size();
    if (int rc = e.pad[b].ensure((int64_t)(h.pad.size() / 4))) return rc;
    if (int rc = e.len[b].ensure((int64_t)nb)) return rc;
    if (int rc = e.id[b].ensure((int64_t)nb)) return rc;
    HIP_TRY(hipMemcpyAsync(e.pad[b].p, h.pad.data(), h.pad.size(), hipMemcpyHostToDevice, e.stream));
    if (int rc = h2d(e.len[b].p, h.len.data(), nb, e.stream)) return rc;
    if (int rc = h2d(e.id[b].p, h.id.data(), nb, e.stream)) return rc;
    p.adp_pad = e.pad[b];
    p.adp_len = e.len[b];
    p.adp_id = e.id[b];
    p.n_adp = (int32_t)nb;
    p.rt = h.rt;
    return 0;
}

// the windows in tile layout, for the cross launches
int tile_windows(Engine &e, const AlignArgs &a, KParams &p) {
    std::vector<int64_t> toff((size_t)((a.n_win + 255) / 256 + 1));
    int64_t max_nq = 0;
    const int64_t nd = tile_layout(a.win_len, a.n_win, toff.data(), &max_nq);
    if (int rc = e.toff.ensure((int64_t)toff.size())) return rc;
    if (int rc = e.tiles.ensure(nd)) return rc;
    if (int rc = h2d(e.toff.p, toff.data(), toff.size(), e.stream)) return rc;
    launch_tiles(p.codes, p.win_off, p.win_len, a.n_win, e.toff, max_nq, e.tiles, e.stream);
    HIP_TRY(hipStreamSynchronize(e.stream));   // toff (host) must outlive the async copy
    p.tiles = e.tiles;
    p.tile_off = e.toff;
    return 0;
}

// Cross shape: every bucket's launch side by side, once every bucket's table is on its way. The host
// bucket tables (bk) outlive the launches: they are read by the copies queued before the fork.
int align_cross(Engine &e, const AlignArgs &a, const BucketHost (&bk)[kNumBuckets], KParams p) {
    struct CrossLaunch {
        int b;
        KParams p;
        int packed;   // bucket_pack_mode
    };
    std::vector<CrossLaunch> cross;
    for (int b = 0; b < kNumBuckets; ++b) {
        const BucketHost &h = bk[b];
        if (h.len.empty()) continue;
        if (int rc = upload_bucket(e, b, h, p)) return rc;
        if (!p.tiles)
            if (int rc = tile_windows(e, a, p)) return rc;
        const int pack = bucket_pack_mode(b, h.len, a.sc);
        bucket_shift(b, h.len, a.sc, pack, p);
        cross.push_back({b, p, pack});
        HIP_TRY(hipGetLastError());
    }
    std::stable_sort(cross.begin(), cross.end(), [&](const CrossLaunch &x, const CrossLaunch &y) {
        return (int64_t)x.p.n_adp * kBuckets[x.b].rpl > (int64_t)y.p.n_adp * kBuckets[y.b].rpl;
    });
    ForkJoin fj;
    if (int rc = fj.begin(e.stream, cross.size())) return rc;
    for (size_t k = 0; k < cross.size(); ++k)
        if (int rc = dispatch(cross[k].b, cross[k].p, a.sc.go != a.sc.ge, fj.at(k), cross[k].packed)) {
            (void)fj.end();
            return rc;
        }
    if (int rc = fj.end()) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}

// Pairs shape: per bucket, its adapters' tasks in waves of one adapter each, runs padded to 64 lanes
// (lane: window, result slot; -1 = idle), one launch per bucket.
int align_pairs(Engine &e, const AlignArgs &a, const BucketHost (&bk)[kNumBuckets], KParams p) {
    std::vector<std::vector<int32_t>> per_adp((size_t)a.n_adp);
    for (int64_t t = 0; t < a.n_task; ++t) per_adp[a.task_adp[t]].push_back((int32_t)t);
    // longest windows first: lanes of a wave then run near-equal column counts
    for (auto &v : per_adp)
        std::stable_sort(v.begin(), v.end(), [&](int32_t x, int32_t y) {
            return a.win_len[a.task_win[x]] > a.win_len[a.task_win[y]];
        });
    std::vector<int32_t> tw, to, wa;
    for (int b = 0; b < kNumBuckets; ++b) {
        const BucketHost &h = bk[b];
        if (h.len.empty()) continue;
        if (int rc = upload_bucket(e, b, h, p)) return rc;
        tw.clear(); to.clear(); wa.clear();
        for (int k = 0; k < p.n_adp; ++k) {
            const std::vector<int32_t> &ts = per_adp[h.id[k]];
            for (size_t s = 0; s < ts.size(); s += 64) {
                wa.push_back(k);
                for (size_t q = 0; q < 64; ++q) {
                    if (s + q < ts.size()) { tw.push_back(a.task_win[ts[s + q]]); to.push_back(ts[s + q]); }
                    else { tw.push_back(-1); to.push_back(0); }
                }
            }
        }
        if (wa.empty()) continue;
        if (int rc = e.tasks_win.ensure((int64_t)tw.size())) return rc;
        if (int rc = e.tasks_out.ensure((int64_t)to.size())) return rc;
        if (int rc = e.wave_adp.ensure((int64_t)wa.size())) return rc;
        if (int rc = h2d(e.tasks_win.p, tw.data(), tw.size(), e.stream)) return rc;
        if (int rc = h2d(e.tasks_out.p, to.data(), to.size(), e.stream)) return rc;
        if (int rc = h2d(e.wave_adp.p, wa.data(), wa.size(), e.stream)) return rc;
        p.task_win = e.tasks_win;
        p.task_out = e.tasks_out;
        p.wave_adp = e.wave_adp;
        p.n_waves = (int64_t)wa.size();
        if (int rc = dispatch(b, p, a.sc.go != a.sc.ge, e.stream, bucket_pack_mode(b, h.len, a.sc))) return rc;
        // the task arrays (host and device) are reused by the next bucket: drain before overwriting
        HIP_TRY(hipStreamSynchronize(e.stream));
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

int align_epilogue(Engine &e, const AlignArgs &a) {
    const int64_t n_res = a.n_res();
    const hipStream_t st = e.stream;
    switch (a.epi) {
    case Epilogue::FirstHits:
        if (int rc = e.hits.ensure(5 * a.n_win)) return rc;
        if (int rc = first_hit_from(e.out, n_res, a.n_win, a.n_adp, a.first_thr, nullptr, e.hits, a.n_win, st)) return rc;
        if (int rc = d2h(a.out, e.hits.p, 5 * (size_t)a.n_win, st)) return rc;
        break;
    case Epilogue::BestHost:   // adapter-set search: per-adapter max of the full identity, on the device
        if (int rc = e.best.ensure(a.n_adp)) return rc;
        if (int rc = h2d(e.best.p, a.best, (size_t)a.n_adp, st)) return rc;
        if (int rc = pcabi_best_full_identity_dev(e.out, n_res, a.n_win, a.n_adp, e.best, st)) return rc;
        if (int rc = d2h(a.best, e.best.p, (size_t)a.n_adp, st)) return rc;
        break;
    case Epilogue::BestDev:
        if (int rc = pcabi_best_full_identity_dev(e.out, n_res, a.n_win, a.n_adp, a.best, st)) return rc;
        break;
    case Epilogue::Orient: {   // n_win == n_adp: the cross product stays on the device, the matrix comes back
        if (int rc = e.hits.ensure(n_res)) return rc;
        const unsigned tb = (unsigned)((a.n_win + 31) / 32);
        hipLaunchKernelGGL(k_orient, dim3(tb, tb), dim3(256), 0, st, (const int32_t *)e.out.p,
                           (const int32_t *)e.wlen.p, a.n_win, e.hits.p);
        HIP_TRY(hipGetLastError());
        if (int rc = d2h(a.out, e.hits.p, (size_t)n_res, st)) return rc;
        break;
    }
    case Epilogue::CompatFlags:
        if (int rc = d2h(a.out, e.out.p, (size_t)n_res, st)) return rc;
        break;
    case Epilogue::Results:
        if (int rc = d2h(a.out, e.out.p, PCABI_NFIELDS * (size_t)n_res, st)) return rc;
        break;
    }
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int align_host_impl(const AlignArgs &a) {
    if (int rc = align_validate(a)) return rc;
    if (a.n_res() == 0) return 0;
    Session s;
    if (int rc = s.open(a.device)) return rc;
    Engine &e = *s.eng;
    // The register cores keep the path's start column mod 2^16: long windows under a scoring with
    // no bound on the path span run every adapter on the striped core (needs_striped)
    int max_L = 0;
    int64_t max_win = 0;
    for (int k = 0; k < a.n_adp; ++k)
        if (a.adp_len[k] <= kMaxRPL) max_L = std::max(max_L, (int)a.adp_len[k]);   // striped: c never wraps
    for (int64_t w = 0; w < a.n_win; ++w) max_win = std::max<int64_t>(max_win, a.win_len[w]);
    BucketHost bk[kNumBuckets];
    build_buckets(a.adp_codes, a.adp_off, a.adp_len, a.n_adp, a.sc, bk, true, true, needs_striped(a.sc, max_L, max_win));
    KParams p{};
    if (int rc = align_stage(e, a, max_win, p)) return rc;
    if (int rc = a.task_win ? align_pairs(e, a, bk, p) : align_cross(e, a, bk, p)) return rc;
    return align_epilogue(e, a);
}

AlignArgs cross_args(int device, const uint8_t *codes, int64_t codes_len, const int64_t *win_off, const int32_t *win_len,
                     int64_t n_win, const uint8_t *adp_codes, const int32_t *adp_off, const int32_t *adp_len,
                     int32_t n_adp, const pcabi::Scoring &sc, Epilogue epi, int32_t *out) {
    return AlignArgs{device, codes, codes_len, win_off, win_len, n_win, adp_codes, adp_off, adp_len, n_adp,
                     nullptr, nullptr, 0, sc, epi, out, 0.0, nullptr};
}

// ---- the middle scan over host buffers -----------------------------------------------------------------

// The middle scan over windows whose codes are in e.codes (being copied there on e.stream).
int64_t middle_scan_resident(Engine &e, const int64_t *win_off, const int32_t *win_len, int64_t n_win,
                             const uint8_t *adp_codes, const int32_t *adp_off, const int32_t *adp_len, int32_t n_adp,
                             int match, int mismatch, int gap_open, int gap_extend, double threshold, int32_t *hits,
                             int64_t cap) {
    if (int rc = e.woff.ensure(n_win)) return rc;
    if (int rc = e.wlen.ensure(n_win)) return rc;
    if (int rc = h2d(e.woff.p, win_off, (size_t)n_win, e.stream)) return rc;
    if (int rc = h2d(e.wlen.p, win_len, (size_t)n_win, e.stream)) return rc;
    pcabi_adapters *tab = nullptr;
    if (int rc = pcabi_adapters_create_scored(adp_codes, adp_off, adp_len, n_adp, match, mismatch, gap_open,
                                              gap_extend, &tab))
        return rc;
    if (!e.scan) {
        if (int rc = pcabi_scan_create(tab, &e.scan)) return rc;
    }
    scan_set_table(e.scan, tab);   // (the kept scan serves each call's own table)
    const int64_t r = pcabi_middle_scan_dev(e.scan, e.codes, e.woff, e.wlen, win_len, n_win, match, mismatch, gap_open,
                                            gap_extend, threshold, hits, cap, e.stream);
    (void)hipStreamSynchronize(e.stream);
    scan_set_table(e.scan, nullptr);
    pcabi_adapters_destroy(tab);
    return r;
}

}  // namespace

extern "C" {

int pcabi_align_host(int device, const uint8_t *codes, int64_t codes_len, const int64_t *win_off,
                     const int32_t *win_len, int64_t n_win, const uint8_t *adp_codes,
                     const int32_t *adp_off, const int32_t *adp_len, int32_t n_adp,
                     const int32_t *task_win, const int32_t *task_adp, int64_t n_task, int match,
                     int mismatch, int gap_open, int gap_extend, int32_t *out) {
    return align_host_impl(AlignArgs{device, codes, codes_len, win_off, win_len, n_win, adp_codes, adp_off, adp_len,
                                     n_adp, task_win, task_adp, n_task, {match, mismatch, gap_open, gap_extend},
                                     Epilogue::Results, out, 0.0, nullptr});
}

int pcabi_best_full_identity_host(int device, const uint8_t *codes, int64_t codes_len, const int64_t *win_off,
                                  const int32_t *win_len, int64_t n_win, const uint8_t *adp_codes,
                                  const int32_t *adp_off, const int32_t *adp_len, int32_t n_adp, int match,
                                  int mismatch, int gap_open, int gap_extend, double *best, int best_on_device) {
    if (!best && n_adp > 0) return fail(PCABI_E_ARG, "best is NULL");
    if (n_win == 0 || n_adp == 0) return 0;     // no window: every maximum stays as given
    AlignArgs a = cross_args(device, codes, codes_len, win_off, win_len, n_win, adp_codes, adp_off, adp_len, n_adp,
                             {match, mismatch, gap_open, gap_extend},
                             best_on_device ? Epilogue::BestDev : Epilogue::BestHost, nullptr);
    a.best = best;
    return align_host_impl(a);
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
    AlignArgs a = cross_args(device, codes, codes_len, win_off, win_len, n_win, adp_codes, adp_off, adp_len, n_adp,
                             {match, mismatch, gap_open, gap_extend}, Epilogue::FirstHits, hits);
    a.first_thr = threshold;
    return align_host_impl(a);
}

int64_t pcabi_middle_scan_host(int device, const uint8_t *codes, int64_t codes_len, const int64_t *win_off,
                               const int32_t *win_len, int64_t n_win, const uint8_t *adp_codes,
                               const int32_t *adp_off, const int32_t *adp_len, int32_t n_adp, int match,
                               int mismatch, int gap_open, int gap_extend, double threshold, int32_t *hits,
                               int64_t cap) {
    if (int rc = check_device(device)) return rc;
    if (n_win < 0 || n_adp < 0 || cap < 0) return fail(PCABI_E_ARG, "negative count");
    if (int rc = check_adapter_lens(adp_len, n_adp)) return rc;
    if (int rc = check_windows(win_off, win_len, n_win, codes_len)) return rc;
    if (n_win == 0 || n_adp == 0) return 0;
    Session s;
    if (int rc = s.open(device)) return rc;
    Engine &e = *s.eng;
    if (int rc = e.codes.ensure(codes_len)) return rc;
    if (int rc = h2d(e.codes.p, codes, (size_t)codes_len, e.stream)) return rc;
    return middle_scan_resident(e, win_off, win_len, n_win, adp_codes, adp_off, adp_len, n_adp, match, mismatch,
                                gap_open, gap_extend, threshold, hits, cap);
}

int pcabi_stage_seqs_host(int device, const char *const *seqs, const int32_t *seq_len, int64_t n, uint8_t *out,
                          int64_t out_len) {
    if (int rc = check_device(device)) return rc;
    if (n < 0) return fail(PCABI_E_ARG, "negative count");
    int64_t total = 0;
    std::vector<int64_t> off((size_t)n);
    if (int rc = seq_layout(seqs, seq_len, n, off.data(), &total)) return rc;
    if (out_len < total) return fail(PCABI_E_ARG, "output buffer smaller than the layout");
    Session s;
    if (int rc = s.open(device)) return rc;
    Engine &e = *s.eng;
    if (int rc = e.codes.ensure(total)) return rc;
    if (int rc = stage_seqs(e, e.codes, seqs, seq_len, off.data(), n, total)) return rc;
    if (int rc = d2h(out, e.codes.p, (size_t)total, e.stream)) return rc;
    HIP_TRY(hipStreamSynchronize(e.stream));
    return 0;
}

int64_t pcabi_middle_scan_seqs(int device, const char *const *seqs, const int32_t *seq_len, int64_t n,
                               const uint8_t *adp_codes, const int32_t *adp_off, const int32_t *adp_len,
                               int32_t n_adp, int match, int mismatch, int gap_open, int gap_extend,
                               double threshold, int32_t *hits, int64_t cap) {
    if (int rc = check_device(device)) return rc;
    if (n < 0 || n_adp < 0 || cap < 0) return fail(PCABI_E_ARG, "negative count");
    if (int rc = check_adapter_lens(adp_len, n_adp)) return rc;
    std::vector<int64_t> off((size_t)n);
    int64_t total = 0;
    if (int rc = seq_layout(seqs, seq_len, n, off.data(), &total)) return rc;
    if (n == 0 || n_adp == 0) return 0;
    Session s;
    if (int rc = s.open(device)) return rc;
    Engine &e = *s.eng;
    if (int rc = e.codes.ensure(total)) return rc;
    if (int rc = stage_seqs(e, e.codes, seqs, seq_len, off.data(), n, total)) return rc;
    return middle_scan_resident(e, off.data(), seq_len, n, adp_codes, adp_off, adp_len, n_adp, match, mismatch,
                                gap_open, gap_extend, threshold, hits, cap);
}

// ---- legacy drop-in ------------------------------------------------------------------------------------

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
    if (int rc = align_host_impl(AlignArgs{device, codes, codes_len, seq_off, seq_len, n_seq, acodes.data(),
                                           aoff.data(), alen.data(), (int32_t)n_seq, tw.data(), ta.data(),
                                           (int64_t)tw.size(), {2, -1, -1, -1}, Epilogue::CompatFlags, got.data(),
                                           0.0, nullptr}))
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
    return align_host_impl(cross_args(device, codes, codes_len, seq_off, seq_len, n, acodes.data(), aoff.data(), seq_len,
                                      (int32_t)n, {2, -1, -1, -1}, Epilogue::Orient, mat));
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

// ---- device epilogues over host buffers ----------------------------------------------------------------

int pcabi_middle_cuts_host(int device, const int32_t *hits, int64_t hit_stride, int64_t n_hits, int64_t n_reads,
                           const uint8_t *bad_start, const uint8_t *bad_end, int32_t n_adp, int good_side,
                           int bad_side, int64_t *cut_off, int64_t *cuts) {
    if (int rc = check_device(device)) return rc;
    if (n_hits < 0 || n_reads < 0 || n_adp < 0 || hit_stride < n_hits) return fail(PCABI_E_ARG, "bad counts");
    for (int64_t k = 0; k < n_hits; ++k)
        if (hits[k] < 0 || hits[k] >= n_reads || hits[hit_stride + k] < 0 || hits[hit_stride + k] >= n_adp)
            return fail(PCABI_E_ARG, "hit read / adapter index out of range");
    Session s;
    if (int rc = s.open(device)) return rc;
    Engine &e = *s.eng;
    const size_t nh = (size_t)std::max<int64_t>(n_hits, 1), na = (size_t)std::max<int32_t>(n_adp, 1);
    const size_t nr = (size_t)n_reads + 1;
    if (int rc = e.bc.ensure((int64_t)(sizeof(int32_t) * 4 * nh + 2 * na + sizeof(int64_t) * (nr + 2 * nh) + 64))) return rc;
    Carve c{(char *)e.bc.p};
    int32_t *d_hits = c.take<int32_t>(4 * nh);
    uint8_t *d_flags = c.take<uint8_t>(2 * na);
    int64_t *d_off = c.take<int64_t>(nr, 8);
    int64_t *d_cuts = c.take<int64_t>(2 * nh);
    // the four used rows (read, adapter, read_start, read_end), packed with stride n_hits
    for (int f = 0; f < 4 && n_hits; ++f)
        if (int rc = h2d(d_hits + f * n_hits, hits + f * hit_stride, (size_t)n_hits, e.stream)) return rc;
    if (n_adp) {
        if (int rc = h2d(d_flags, bad_start, (size_t)n_adp, e.stream)) return rc;
        if (int rc = h2d(d_flags + n_adp, bad_end, (size_t)n_adp, e.stream)) return rc;
    }
    if (int rc = pcabi_middle_cuts_dev(d_hits, n_hits, n_hits, n_reads, d_flags, d_flags + n_adp, good_side, bad_side,
                                       d_off, d_cuts, e.stream))
        return rc;
    if (int rc = d2h(cut_off, d_off, nr, e.stream)) return rc;
    if (n_hits)
        if (int rc = d2h(cuts, d_cuts, 2 * (size_t)n_hits, e.stream)) return rc;
    HIP_TRY(hipStreamSynchronize(e.stream));
    return 0;
}

int pcabi_barcode_call_host(int device, const int32_t *start_res, int32_t n_sa, const int32_t *start_slot_adp,
                            const int32_t *start_slot_name, int32_t n_start_slots, const int32_t *end_res,
                            int32_t n_ea, const int32_t *end_slot_adp, const int32_t *end_slot_name,
                            int32_t n_end_slots, int64_t n_read, double barcode_threshold, double barcode_diff,
                            int require_two, int32_t *call, double *scores) {
    if (int rc = check_device(device)) return rc;
    if (n_read < 0 || n_sa < 0 || n_ea < 0 || n_start_slots < 0 || n_end_slots < 0)
        return fail(PCABI_E_ARG, "negative count");
    for (int k = 0; k < n_start_slots; ++k)
        if (start_slot_adp[k] < 0 || start_slot_adp[k] >= n_sa) return fail(PCABI_E_ARG, "start slot adapter out of range");
    for (int k = 0; k < n_end_slots; ++k)
        if (end_slot_adp[k] < 0 || end_slot_adp[k] >= n_ea) return fail(PCABI_E_ARG, "end slot adapter out of range");
    if (n_read == 0) return 0;
    Session s;
    if (int rc = s.open(device)) return rc;
    Engine &e = *s.eng;
    const size_t n = (size_t)n_read;
    const size_t sres = PCABI_NFIELDS * (size_t)n_sa * n, eres = PCABI_NFIELDS * (size_t)n_ea * n;   // int32 each
    const size_t slots = 2 * (size_t)(n_start_slots + n_end_slots);
    if (int rc = e.bc.ensure((int64_t)(sizeof(int32_t) * (sres + eres + slots + n) + 32 * n + 64))) return rc;
    Carve c{(char *)e.bc.p};
    int32_t *d_sres = c.take<int32_t>(sres);
    int32_t *d_eres = c.take<int32_t>(eres);
    int32_t *d_slots = c.take<int32_t>(slots);
    int32_t *d_call = c.take<int32_t>(n);
    double *d_scores = c.take<double>(4 * n, 8);
    std::vector<int32_t> h_slots;
    h_slots.insert(h_slots.end(), start_slot_adp, start_slot_adp + n_start_slots);
    h_slots.insert(h_slots.end(), start_slot_name, start_slot_name + n_start_slots);
    h_slots.insert(h_slots.end(), end_slot_adp, end_slot_adp + n_end_slots);
    h_slots.insert(h_slots.end(), end_slot_name, end_slot_name + n_end_slots);
    if (sres)
        if (int rc = h2d(d_sres, start_res, sres, e.stream)) return rc;
    if (eres)
        if (int rc = h2d(d_eres, end_res, eres, e.stream)) return rc;
    if (slots)
        if (int rc = h2d(d_slots, h_slots.data(), slots, e.stream)) return rc;
    const int32_t *ss = d_slots, *en_ = d_slots + 2 * n_start_slots;
    if (int rc = pcabi_barcode_call_dev(d_sres, (int64_t)n_sa * n_read, ss, ss + n_start_slots, n_start_slots, d_eres,
                                        (int64_t)n_ea * n_read, en_, en_ + n_end_slots, n_end_slots, n_read,
                                        barcode_threshold, barcode_diff, require_two, d_call,
                                        scores ? d_scores : nullptr, e.stream))
        return rc;
    if (int rc = d2h(call, d_call, n, e.stream)) return rc;
    if (scores)
        if (int rc = d2h(scores, d_scores, 4 * n, e.stream)) return rc;
    HIP_TRY(hipStreamSynchronize(e.stream));
    return 0;
}

}  // extern "C"

// ---- end-trim decisions of the reference-API driver (find_adapters_at_read_ends) ------------------------

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

// One read end of a pcabi_end_decisions call: its windows, adapters, listed barcode adapters, list out.
struct EndSideArgs {
    const int64_t *off;
    const int32_t *len;
    const uint8_t *adp_codes;
    const int32_t *adp_off, *adp_len;
    int32_t n_adp;
    const int32_t *bc;
    int32_t n_bc;
    int32_t *hits;
};

// pcabi_end_decisions_host / _seqs: the windows' codes come from `codes` (a host Dna5 buffer) or,
// when `win` is set, from the 2 n_read window strings (start windows, then end windows), encoded
// straight into pinned staging buffers while earlier chunks copy (stage_seqs)
struct EndArgs {
    int device;
    const uint8_t *codes;
    const char *const *win;
    const int32_t *win_len;
    int64_t codes_len;
    int64_t n_read;
    EndSideArgs side[2];   // start, end
    pcabi::Scoring sc;
    int end_size, extra_trim;
    double end_threshold;
    int min_trim_size;
    int32_t *start_trim, *end_trim;
    int64_t cap;
    int64_t *n_hits;
    double *bc_full;
    size_t dcap(int s) const { return (size_t)n_read * (size_t)side[s].n_adp; }   // a side's list rows on the device
};

// PCABI_END_PROF=1: the call's host / device phases on stderr
struct EndProf {
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void mark(const char *what) const {
        static const bool on = [] { const char *v = std::getenv("PCABI_END_PROF"); return v && v[0] == '1'; }();
        if (on)
            std::fprintf(stderr, "pcabi_end_decisions: %-10s %.3f ms\n", what,
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
};

int end_validate(const EndArgs &a) {
    if (int rc = check_device(a.device)) return rc;
    if (a.n_read < 0 || a.side[0].n_adp < 0 || a.side[1].n_adp < 0 || a.cap < 0 || a.side[0].n_bc < 0 || a.side[1].n_bc < 0)
        return fail(PCABI_E_ARG, "negative count");
    for (const EndSideArgs &s : a.side)
        if (int rc = check_adapter_lens(s.adp_len, s.n_adp)) return rc;
    for (const EndSideArgs &s : a.side)
        if (int rc = check_windows(s.off, s.len, a.n_read, a.codes_len)) return rc;
    for (int side = 0; side < 2; ++side)
        for (int32_t j = 0; j < a.side[side].n_bc; ++j)
            if (a.side[side].bc[j] < 0 || a.side[side].bc[j] >= a.side[side].n_adp)
                return fail(PCABI_E_ARG, side ? "end barcode adapter out of range" : "start barcode adapter out of range");
    return 0;
}

int end_stage(Engine &e, const EndArgs &a) {
    if (int rc = e.dec.codes.ensure(a.codes_len)) return rc;
    if (!a.win) return h2d(e.dec.codes.p, a.codes, (size_t)a.codes_len, e.stream);
    const size_t n = (size_t)a.n_read;
    std::vector<int64_t> off(2 * n);
    std::copy(a.side[0].off, a.side[0].off + n, off.begin());
    std::copy(a.side[1].off, a.side[1].off + n, off.begin() + (int64_t)n);
    return stage_seqs(e, e.dec.codes, a.win, a.win_len, off.data(), 2 * a.n_read, a.codes_len);
}

// The side's prepared table, kept from the last call while the adapters and the scoring are the same.
int side_table(Engine::DTab &c, const EndSideArgs &s, const pcabi::Scoring &sc, pcabi_adapters **out) {
    std::vector<uint8_t> key;
    for (int32_t a = 0; a < s.n_adp; ++a)
        key.insert(key.end(), s.adp_codes + s.adp_off[a], s.adp_codes + s.adp_off[a] + s.adp_len[a]);
    if (c.t && c.sc.ma == sc.ma && c.sc.mi == sc.mi && c.sc.go == sc.go && c.sc.ge == sc.ge && c.codes == key &&
        c.lens == std::vector<int32_t>(s.adp_len, s.adp_len + s.n_adp)) {
        *out = c.t;
        return 0;
    }
    if (c.t) pcabi_adapters_destroy(c.t);   // the previous call synchronised its stream
    c.t = nullptr;
    if (int rc = pcabi_adapters_create_scored(s.adp_codes, s.adp_off, s.adp_len, s.n_adp, sc.ma, sc.mi, sc.go, sc.ge,
                                              &c.t))
        return rc;
    c.codes.swap(key);
    c.lens.assign(s.adp_len, s.adp_len + s.n_adp);
    c.sc = sc;
    *out = c.t;
    return 0;
}

// a side's windows and tile offsets (toff: read by the copy queued here) on the device, its tiles
// queued; *reg: its cross product
int end_side_windows(Engine &e, const EndArgs &a, int side, std::vector<int64_t> &toff, pcabi_cross_region *reg,
                     int32_t *n_reg) {
    const EndSideArgs &s = a.side[side];
    Engine::EndSide &b = e.dec.side[side];
    const int64_t n = a.n_read, na = std::max(s.n_adp, 1);
    const hipStream_t st = e.stream;
    if (int rc = b.off.ensure(n)) return rc;
    if (int rc = b.len.ensure(n)) return rc;
    toff.assign((size_t)((n + 255) / 256 + 1), 0);
    int64_t max_nq = 0;
    const int64_t nd = tile_layout(s.len, n, toff.data(), &max_nq);
    if (int rc = b.toff.ensure((int64_t)toff.size())) return rc;
    if (int rc = b.tiles.ensure(std::max<int64_t>(nd, 1))) return rc;
    if (int rc = b.res.ensure(PCABI_NFIELDS * n * na)) return rc;
    if (int rc = b.flag.ensure(n * na)) return rc;
    if (int rc = h2d(b.off.p, s.off, (size_t)n, st)) return rc;
    if (int rc = h2d(b.len.p, s.len, (size_t)n, st)) return rc;
    if (int rc = h2d(b.toff.p, toff.data(), toff.size(), st)) return rc;
    if (!s.n_adp) return 0;
    pcabi_adapters *tab = nullptr;
    if (int rc = side_table(e.dtab[side], s, a.sc, &tab)) return rc;
    launch_tiles(e.dec.codes, b.off, b.len, n, b.toff, max_nq, b.tiles, st);
    const int32_t max_len = n ? *std::max_element(s.len, s.len + n) : 0;
    reg[(*n_reg)++] = pcabi_cross_region{b.tiles, b.toff, b.len, n, std::max(max_len, 0), tab, b.res, s.n_adp * n};
    return 0;
}

// both read ends in one multi call (the register buckets of both sides in grouped launches), then
// the trims and the per-pair hit flags. toff: the sides' tile offsets, which the caller keeps until the
// stream is drained.
int end_align_trim(Engine &e, const EndArgs &a, std::vector<int64_t> (&toff)[2]) {
    const int64_t n = a.n_read;
    if (int rc = e.dec.trims.ensure(2 * n)) return rc;
    pcabi_cross_region reg[2];
    int32_t n_reg = 0;
    for (int side = 0; side < 2; ++side)
        if (int rc = end_side_windows(e, a, side, toff[side], reg, &n_reg)) return rc;
    if (int rc = pcabi_align_cross_multi_dev(reg, n_reg, a.sc.ma, a.sc.mi, a.sc.go, a.sc.ge, e.stream, nullptr, nullptr))
        return rc;
    const Engine::EndSide &s = e.dec.side[0], &t = e.dec.side[1];
    const int32_t n_sa = a.side[0].n_adp, n_ea = a.side[1].n_adp;
    return pcabi_end_trim_dev(s.res, n_sa * n, n_sa, t.res, n_ea * n, n_ea, n, a.end_size, a.extra_trim, a.end_threshold,
                              a.min_trim_size, e.dec.trims, e.dec.trims + n, s.flag, t.flag, e.stream);
}

// The alignment lists on the device (list(s): side s's seven rows), the listed adapters' identities
// and the trims on their way back; cnt: the lists' lengths, read back (the stream is drained).
int32_t *end_list(Engine &e, const EndArgs &a, int side) { return e.dec.lists.p + (side ? 7 * a.dcap(0) : 0); }

int end_lists(Engine &e, const EndArgs &a, const EndProf &prof, unsigned long long (&cnt)[2]) {
    const hipStream_t st = e.stream;
    const size_t n = (size_t)a.n_read, nbc = (size_t)a.side[0].n_bc + (size_t)a.side[1].n_bc;
    if (int rc = e.dec.lists.ensure((int64_t)(7 * (a.dcap(0) + a.dcap(1)) + 4))) return rc;
    if (int rc = e.dec.counts.ensure((int64_t)(64 + ((4 * nbc + 7) & ~(size_t)7) + 8 * nbc * n))) return rc;
    Carve c{(char *)e.dec.counts.p};
    unsigned long long *d_cnt = c.take<unsigned long long>(2);
    int32_t *d_sel = c.take<int32_t>(nbc);
    double *d_full = c.take<double>(nbc * n, 8);
    for (int side = 0; side < 2; ++side) {
        const int32_t na = a.side[side].n_adp;
        if (!na) {
            HIP_TRY(hipMemsetAsync(d_cnt + side, 0, 8, st));
            continue;
        }
        if (int rc = pcabi_flag_list_dev(e.dec.side[side].flag, na, a.n_read, e.dec.side[side].res, na * a.n_read,
                                         end_list(e, a, side), (int64_t)a.dcap(side), d_cnt + side, st))
            return rc;
    }
    if (nbc && a.bc_full) {
        std::vector<int32_t> sel(a.side[0].bc, a.side[0].bc + a.side[0].n_bc);
        sel.insert(sel.end(), a.side[1].bc, a.side[1].bc + a.side[1].n_bc);
        if (int rc = h2d(d_sel, sel.data(), nbc, st)) return rc;
        for (int side = 0; side < 2; ++side) {
            const int32_t ns = a.side[side].n_bc, before = side ? a.side[0].n_bc : 0;
            if (!ns) continue;
            const int64_t tot = (int64_t)ns * a.n_read;
            hipLaunchKernelGGL(k_full_ids, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st,
                               (const int32_t *)e.dec.side[side].res.p, (int64_t)a.side[side].n_adp * a.n_read, a.n_read,
                               (const int32_t *)(d_sel + before), ns, d_full + (size_t)before * n);
        }
        HIP_TRY(hipGetLastError());
        if (int rc = d2h(a.bc_full, d_full, nbc * n, st)) return rc;
    }
    if (int rc = d2h(a.start_trim, e.dec.trims.p, n, st)) return rc;
    if (int rc = d2h(a.end_trim, e.dec.trims.p + n, n, st)) return rc;
    prof.mark("queued");
    if (int rc = d2h(cnt, d_cnt, 2, st)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    prof.mark("device");
    return 0;
}

// The lists to the host in the compact form (k_list_pack), unpacked into the callers' rows of stride
// cap. A side with more alignments than cap is left out: the caller grows cap and calls again.
int end_read_compact(Engine &e, const EndArgs &a, const EndProf &prof, const unsigned long long (&cnt)[2]) {
    const hipStream_t st = e.stream;
    const size_t n = (size_t)a.n_read, half = (n + 1) / 2;                // count dwords per side
    size_t words = 0, at_side[2] = {0, 0};
    for (int side = 0; side < 2; ++side) {
        at_side[side] = words;
        if ((int64_t)cnt[side] <= a.cap) words += 3 * (size_t)cnt[side] + half;   // 6 int16 = 3 dwords
    }
    if (int rc = e.dec.packed.ensure((int64_t)(words + 16))) return rc;
    std::vector<uint32_t> h(words);
    for (int side = 0; side < 2; ++side) {
        const int64_t k = (int64_t)cnt[side];
        if (k > a.cap) continue;
        uint32_t *rows = e.dec.packed.p + at_side[side], *dc = rows + 3 * (size_t)k;
        HIP_TRY(hipMemsetAsync(dc, 0, 4 * half, st));
        if (k)
            hipLaunchKernelGGL(k_list_pack, dim3((unsigned)std::min<int64_t>((k + 255) / 256, 4096)), dim3(256), 0, st,
                               (const int32_t *)end_list(e, a, side), (int64_t)a.dcap(side), k, (int16_t *)rows, dc);
    }
    HIP_TRY(hipGetLastError());
    if (words)
        if (int rc = d2h(h.data(), (const uint32_t *)e.dec.packed.p, words, st)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    prof.mark("lists d2h");
    for (int side = 0; side < 2; ++side) {
        int32_t *dst = a.side[side].hits;
        const int64_t k = (int64_t)cnt[side];
        if (k > a.cap || !k) continue;
        const int16_t *f16 = (const int16_t *)(h.data() + at_side[side]);
        const uint16_t *c16 = (const uint16_t *)(h.data() + at_side[side] + 3 * (size_t)k);
        int64_t j = 0;
        for (size_t r = 0; r < n && j < k; ++r)
            for (uint16_t c = c16[r]; c > 0; --c) dst[j++] = (int32_t)r;
        for (int f = 0; f < 6; ++f)
            for (int64_t q = 0; q < k; ++q) dst[(f + 1) * a.cap + q] = f16[f * k + q];
    }
    prof.mark("unpacked");
    return 0;
}

// the lists as they are: rows of the device list (stride dcap) -> stride cap
int end_read_plain(Engine &e, const EndArgs &a, const unsigned long long (&cnt)[2]) {
    for (int side = 0; side < 2; ++side) {
        const int64_t k = (int64_t)cnt[side];
        if (k > a.cap || !k) continue;                // too many: the caller grows cap and calls again
        for (int f = 0; f < 7; ++f)
            if (int rc = d2h(a.side[side].hits + f * a.cap, (const int32_t *)end_list(e, a, side) + f * a.dcap(side),
                             (size_t)k, e.stream))
                return rc;
    }
    HIP_TRY(hipStreamSynchronize(e.stream));
    return 0;
}

int end_decisions_impl(const EndArgs &a) {
    if (int rc = end_validate(a)) return rc;
    a.n_hits[0] = a.n_hits[1] = 0;
    if (a.n_read == 0) return 0;
    EndProf prof;
    Session s;
    if (int rc = s.open(a.device)) return rc;
    Engine &e = *s.eng;
    if (int rc = end_stage(e, a)) return rc;
    prof.mark("staged");
    std::vector<int64_t> toff[2];
    if (int rc = end_align_trim(e, a, toff)) return rc;
    unsigned long long cnt[2] = {0, 0};
    if (int rc = end_lists(e, a, prof, cnt)) return rc;
    a.n_hits[0] = (int64_t)cnt[0];
    a.n_hits[1] = (int64_t)cnt[1];
    // compact (int16 fields, per-read counts) when every field fits 16 bits -- the alignment lengths
    // l1 / l2 reach the window plus the adapter
    int32_t max_win = 0, max_adp = 0;
    for (const EndSideArgs &sd : a.side) {
        for (int64_t w = 0; w < a.n_read; ++w) max_win = std::max(max_win, sd.len[w]);
        for (int32_t k = 0; k < sd.n_adp; ++k) max_adp = std::max(max_adp, sd.adp_len[k]);
    }
    const bool compact = (int64_t)max_win + max_adp < 32768 && a.side[0].n_adp < 32768 && a.side[1].n_adp < 32768;
    return compact ? end_read_compact(e, a, prof, cnt) : end_read_plain(e, a, cnt);
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
    return end_decisions_impl(EndArgs{device, codes, nullptr, nullptr, codes_len, n_read,
                                      {{s_off, s_len, sa_codes, sa_off, sa_len, n_sa, bc_s, n_bc_s, start_hits},
                                       {e_off, e_len, ea_codes, ea_off, ea_len, n_ea, bc_e, n_bc_e, end_hits}},
                                      {match, mismatch, gap_open, gap_extend}, end_size, extra_trim, end_threshold,
                                      min_trim_size, start_trim, end_trim, cap, n_hits, bc_full});
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
    std::vector<int64_t> off((size_t)(2 * n_read));
    int64_t total = 0;
    if (int rc = seq_layout(win, win_len, 2 * n_read, off.data(), &total)) return rc;
    const int64_t *e_off = off.data() + n_read;
    const int32_t *e_len = win_len + n_read;
    return end_decisions_impl(EndArgs{device, nullptr, win, win_len, total, n_read,
                                      {{off.data(), win_len, sa_codes, sa_off, sa_len, n_sa, bc_s, n_bc_s, start_hits},
                                       {e_off, e_len, ea_codes, ea_off, ea_len, n_ea, bc_e, n_bc_e, end_hits}},
                                      {match, mismatch, gap_open, gap_extend}, end_size, extra_trim, end_threshold,
                                      min_trim_size, start_trim, end_trim, cap, n_hits, bc_full});
}
