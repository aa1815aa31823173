// pcabi_gzstream.hip -- ordinary (non-BGZF) gzip input inflated on the GPU (gfx950): include/pcabi.h
// pcabi_gunzip_stream_*; DESIGN.md "gunzip on the device". The method and everything that holds no
// device-only construct is in pcabi_gzstream.h; here are the kernels and the device backend of its
// stream driver.
//
//   k_gz_find    one wavefront per cut: the first candidate at or after it (a lane per bit offset for
//                the cheap header test, the survivors verified wave-wide by read_dynamic / build_table)
//   k_gz_count   one wavefront per candidate: the decoder over the counting sink (size, end bit, final)
//   k_gz_decode  one wavefront per chunk on the chain: the decoder over the marker sink, whose LDS
//                ring holds the last 32768 symbols (64 KiB) next to the Tables: 80 KiB, two per CU
//   k_gz_window  one workgroup: the windows handed down the chain, chunk after chunk, in LDS
//   k_gz_resolve one workgroup per 16 KiB of output: symbols to bytes through the chunk's window,
//                CRC-32 of the piece, aligned 16-byte stores with bytes at the ragged ends
// All stores are plain C++ stores.
#include <hip/hip_runtime.h>

#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>

#include "../../include/pcabi.h"
#include "pcabi_crc.h"
#include "pcabi_gzstream.h"
#include "pcabi_hostdev.h"

using namespace pcabi_internal;
using namespace pcabi_inflate;
using namespace pcabi_gzstream;
using namespace pcabi_crc;

namespace {

constexpr int kWave = 64;

__device__ const CrcTables d_tab = make_tables();

struct WaveParX {
    __device__ int lane() const { return (int)threadIdx.x; }
    __device__ int lanes() const { return kWave; }
    __device__ void sync() const { __syncthreads(); }
    __device__ int lowest(bool pred) const {
        const unsigned long long m = __ballot(pred);
        return m ? __ffsll((long long)m) - 1 : -1;
    }
    __device__ int bcast(int v, int l) const { return __shfl(v, l); }
};

// SerialMarkerSink wave-wide: one lane stores literals, copies are spread over the lanes. A copy's
// sources lie before pos (i % dist), so no lane reads what another one writes; in the ring a source
// slot may be a later destination's (dist near 32768), which the same or a later pass writes.
struct WaveMarkerSink {
    uint16_t *ring;
    uint16_t *out;
    uint32_t hist;
    __device__ uint32_t history() const { return hist; }
    __device__ void put(uint32_t pos, uint8_t c) {
        if (threadIdx.x == 0) {
            ring[pos & (kWindow - 1)] = c;
            out[pos] = c;
        }
    }
    __device__ void copy(uint32_t pos, uint32_t dist, uint32_t len) {
        __syncthreads();
        const uint32_t from = pos - dist;
        for (uint32_t i = threadIdx.x; i < len; i += kWave) {
            const uint16_t s = ring[(from + (dist >= len ? i : i % dist)) & (kWindow - 1)];
            ring[(pos + i) & (kWindow - 1)] = s;
            out[pos + i] = s;
        }
        __syncthreads();
    }
    __device__ void store(uint32_t pos, const uint8_t *src, uint32_t len) {
        for (uint32_t i = threadIdx.x; i < len; i += kWave) {
            ring[(pos + i) & (kWindow - 1)] = src[i];
            out[pos + i] = src[i];
        }
    }
};

__global__ __launch_bounds__(kWave) void k_gz_find(const uint8_t *__restrict__ z, uint32_t n, int64_t chunk_bytes, int64_t ncuts,
                                                   int64_t *__restrict__ cand, int32_t *__restrict__ kind) {
    __shared__ Tables t;
    const int64_t k = (int64_t)blockIdx.x + 1;
    if (k >= ncuts) return;
    WaveParX par;
    int64_t pos = -1;
    int32_t kd = CAND_NONE;
    const int64_t lo = 8 * k * chunk_bytes, end = 8 * (int64_t)n, hi = lo + 8 * chunk_bytes < end ? lo + 8 * chunk_bytes : end;
    find_candidate(par, t, z, n, lo, hi, &pos, &kd);
    if (threadIdx.x == 0) {
        cand[k] = pos;
        kind[k] = kd;
    }
}

__global__ __launch_bounds__(kWave) void k_gz_count(const uint8_t *__restrict__ z, uint32_t n, const int64_t *__restrict__ cand,
                                                    const int32_t *__restrict__ kind, int64_t ncuts, int64_t chunk_bits,
                                                    int64_t limit_bits, ChunkRes *__restrict__ res) {
    __shared__ Tables t;
    const int64_t k = blockIdx.x;
    ChunkRes r{0, 0, -1, 0, 0};
    const int kd = kind[k];
    const int64_t start = cand[k];
    if (kd != CAND_NONE && start >= 0 && start <= 8 * (int64_t)n) {   // uniform
        WaveParX par;
        CountSink sink{cand_history(kd)};
        const CandStop stop{cand, ncuts, chunk_bits, limit_bits};
        Bits b = bits_at(z, n, start);
        r.status = inflate_blocks(par, sink, t, b, kChunkOutMax, stop, &r.produced, &r.end_bit, &r.final_block);
    }
    if (threadIdx.x == 0) res[k] = r;
}

__global__ __launch_bounds__(kWave) void k_gz_decode(const uint8_t *__restrict__ z, uint32_t n, const int64_t *__restrict__ cand,
                                                     const int32_t *__restrict__ kind, int64_t ncuts, int64_t chunk_bits,
                                                     int64_t limit_bits, const int32_t *__restrict__ conf,
                                                     const int64_t *__restrict__ off, uint16_t *__restrict__ sym, int64_t sym_cap,
                                                     int32_t *__restrict__ status) {
    __shared__ uint16_t ring[kWindow];
    __shared__ Tables t;
    const int64_t i = blockIdx.x, k = conf[i];
    const int64_t lo = off[i], hi = off[i + 1];
    int st = PCABI_INFLATE_E_OUTPUT;
    if (k >= 0 && k < ncuts && lo >= 0 && hi >= lo && hi <= sym_cap && hi - lo <= (int64_t)kChunkOutMax && cand[k] >= 0 &&
        cand[k] <= 8 * (int64_t)n) {   // uniform
        WaveParX par;
        WaveMarkerSink sink{ring, sym + lo, cand_history(kind[k])};
        if (sink.hist) marker_ring_init(par, ring);
        const CandStop stop{cand, ncuts, chunk_bits, limit_bits};
        Bits b = bits_at(z, n, cand[k]);
        uint32_t produced = 0;
        int64_t end_bit = 0;
        int fin = 0;
        st = inflate_blocks(par, sink, t, b, (uint32_t)(hi - lo), stop, &produced, &end_bit, &fin);
        if (!st && (int64_t)produced != hi - lo) st = PCABI_INFLATE_E_LENGTH;
    }
    if (threadIdx.x == 0) status[i] = st;
}

constexpr int kWinThreads = 1024;
// win[0, 32768) is the first chunk's window; win[(i + 1) * 32768 ...) becomes the window after chunk i
__global__ __launch_bounds__(kWinThreads) void k_gz_window(const uint16_t *__restrict__ sym, const int64_t *__restrict__ off,
                                                           int64_t nc, uint8_t *win) {
    __shared__ __attribute__((aligned(16))) uint8_t w[2][kWindow];
    for (uint32_t j = threadIdx.x * 4u; j < kWindow; j += kWinThreads * 4u) *(uint32_t *)&w[0][j] = *(const uint32_t *)&win[j];
    __syncthreads();
    int cur = 0;
    for (int64_t i = 0; i < nc; ++i) {
        const int64_t lo = off[i], len = off[i + 1] - lo;
        const uint8_t *c = w[cur];
        uint8_t *x = w[cur ^ 1];
        for (uint32_t j0 = threadIdx.x * 4u; j0 < kWindow; j0 += kWinThreads * 4u) {
            uint32_t word = 0;
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                const int64_t j = j0 + q, src = len - (int64_t)kWindow + j;
                const uint32_t b = src >= 0 ? resolve_sym(sym[lo + src], c) : c[j + len];
                word |= b << (8 * q);
            }
            *(uint32_t *)&x[j0] = word;
            *(uint32_t *)&win[(i + 1) * (int64_t)kWindow + j0] = word;
        }
        __syncthreads();
        cur ^= 1;
    }
}

constexpr int kResThreads = 256;
__global__ __launch_bounds__(kResThreads) void k_gz_resolve(const uint16_t *__restrict__ sym, const int64_t *__restrict__ off,
                                                            const int32_t *__restrict__ tile_chunk,
                                                            const int64_t *__restrict__ tile_at, const uint8_t *__restrict__ win,
                                                            const uint32_t *__restrict__ min_marker, uint8_t *__restrict__ out,
                                                            int64_t out_cap, uint32_t *__restrict__ tile_crc,
                                                            int32_t *__restrict__ tile_status) {
    __shared__ __attribute__((aligned(16))) uint8_t bytes[kTile];
    __shared__ uint32_t tab[768];
    __shared__ uint32_t red[kResThreads / kWave];
    const int64_t t = blockIdx.x;
    const int32_t c = tile_chunk[t];
    const int64_t lo = off[c] + tile_at[t];
    const int64_t left = off[c + 1] - lo;
    if (lo < 0 || left <= 0 || lo + (left < kTile ? left : kTile) > out_cap) {   // uniform
        if (threadIdx.x == 0) {
            tile_crc[t] = 0;
            tile_status[t] = PCABI_INFLATE_E_OUTPUT;
        }
        return;
    }
    const uint32_t len = (uint32_t)(left < kTile ? left : kTile);
    const uint8_t *w = win + (int64_t)c * kWindow;
    const uint32_t mm = min_marker[c];
    for (int i = threadIdx.x; i < 256; i += kResThreads) {
        tab[i] = d_tab.byte[i];
        tab[256 + i] = d_tab.xp[0][i];
        tab[512 + i] = d_tab.xp[1][i];
    }
    int bad = 0;
    for (uint32_t i = threadIdx.x; i < len; i += kResThreads) {
        const uint16_t s = sym[lo + i];
        if ((s & kMarker) && (uint32_t)(s & (kWindow - 1)) < mm) bad = 1;
        bytes[i] = resolve_sym(s, w);
    }
    bad = __syncthreads_or(bad);
    // the piece's CRC-32: 16-byte lane chunks, each moved past the bytes after it, xor-reduced
    uint32_t acc = 0;
    for (uint32_t first = threadIdx.x * 16u; first < len; first += kResThreads * 16u) {
        const uint32_t m = min(16u, len - first);
        uint32_t crc = 0xffffffffu;
        for (uint32_t j = 0; j < m; ++j) crc = tab[(crc ^ bytes[first + j]) & 0xff] ^ (crc >> 8);
        crc ^= 0xffffffffu;
        const uint32_t after = len - (first + m);   // < 16384
        uint32_t xp = tab[256 + (after & 255)];
        if (after >> 8) xp = mulmod(xp, tab[512 + (after >> 8)]);
        acc ^= mulmod(crc, xp);
    }
    for (int d = 32; d >= 1; d >>= 1) acc ^= __shfl_xor(acc, d);
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t all = 0;
        for (int i = 0; i < kResThreads / kWave; ++i) all ^= red[i];
        tile_crc[t] = all;
        tile_status[t] = bad ? PCABI_INFLATE_E_DIST : 0;
    }
    // LDS -> global: bytes up to the first 16-byte boundary of the destination, aligned 16-byte
    // stores, bytes after the last boundary
    uint8_t *o = out + lo;
    const uint32_t head = min(len, (uint32_t)((16u - ((uintptr_t)o & 15u)) & 15u));
    const uint32_t nvec = (len - head) / 16u, tail0 = head + nvec * 16u;
    if (threadIdx.x < head) o[threadIdx.x] = bytes[threadIdx.x];
    for (uint32_t v = threadIdx.x; v < nvec; v += kResThreads) {
        const uint8_t *s = bytes + head + v * 16u;
        uint32_t x[4];
        if ((head & 3u) == 0) {   // uniform: the LDS side is word-aligned too
#pragma unroll
            for (int q = 0; q < 4; ++q) x[q] = ((const uint32_t *)s)[q];
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                x[q] = (uint32_t)s[4 * q] | (uint32_t)s[4 * q + 1] << 8 | (uint32_t)s[4 * q + 2] << 16 | (uint32_t)s[4 * q + 3] << 24;
        }
        *(uint4 *)(o + head + v * 16u) = make_uint4(x[0], x[1], x[2], x[3]);
    }
    if (tail0 + threadIdx.x < len) o[tail0 + threadIdx.x] = bytes[tail0 + threadIdx.x];
}

// ---- host side ---------------------------------------------------------------------------------
std::mutex g_mu;   // the tune values, the kernel times, the host entry's backend
Tune g_tune = kDefaultTune;
bool g_time_on = false;
double g_ms[5] = {0, 0, 0, 0, 0};   // finder, counting pass, decode, hand-down, resolve
thread_local int64_t t_stats[ST_N] = {0, 0, 0, 0, 0, 0, 0};

// The device backend of pcabi_gzstream.h's Stream: the current device's buffers, kept between spans.
struct DevBackend {
    Stream st;
    PinBuf<> pin_in, pin_out;
    DevBuf<> d_in, d_out, d_win;
    DevBuf<uint16_t> d_sym;
    DevBuf<int64_t> d_cand, d_off, d_tile_at;
    DevBuf<int32_t> d_kind, d_conf, d_status, d_tile_chunk, d_tile_status;
    DevBuf<uint32_t> d_minm, d_tile_crc;
    DevBuf<ChunkRes> d_res;
    std::vector<int32_t> tile_chunk, tile_status;
    std::vector<int64_t> tile_at;
    std::vector<uint32_t> tile_crc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool timing = false;

    ~DevBackend() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    int begin() {
        if (!st.s) {
            if (int rc = st.create()) return rc;
        }
        {
            std::lock_guard<std::mutex> lk(g_mu);
            timing = g_time_on;
        }
        if (timing && !e0) {
            PCABI_TRY(hipEventCreate(&e0));
            PCABI_TRY(hipEventCreate(&e1));
        }
        return 0;
    }
    int tick() {
        if (timing) PCABI_TRY(hipEventRecord(e0, st));
        return 0;
    }
    int tock(int kind) {
        PCABI_TRY(hipGetLastError());
        if (!timing) return 0;
        PCABI_TRY(hipEventRecord(e1, st));
        PCABI_TRY(hipEventSynchronize(e1));
        float ms = 0;
        PCABI_TRY(hipEventElapsedTime(&ms, e0, e1));
        std::lock_guard<std::mutex> lk(g_mu);
        g_ms[kind] += ms;
        return 0;
    }
    template <class B>
    static int room(B &b, int64_t need) {
        return b.reserve(need, need + need / 4 + 64);
    }
    int load(const uint8_t *src, int64_t nbytes) {
        if (int rc = begin()) return rc;
        if (int rc = room(pin_in, nbytes + 16)) return rc;
        if (int rc = room(d_in, nbytes + 16)) return rc;
        par_memcpy(pin_in, src, (size_t)nbytes);
        PCABI_TRY(hipMemcpyAsync(d_in, pin_in, (size_t)nbytes, hipMemcpyHostToDevice, st));
        return 0;
    }
    int find(Plan &p) {
        const size_t nc = (size_t)p.ncuts;
        if (int rc = room(d_cand, p.ncuts)) return rc;
        if (int rc = room(d_kind, p.ncuts)) return rc;
        PCABI_TRY(hipMemcpyAsync(d_cand, p.cand.data(), 8 * nc, hipMemcpyHostToDevice, st));
        PCABI_TRY(hipMemcpyAsync(d_kind, p.kind.data(), 4 * nc, hipMemcpyHostToDevice, st));
        if (p.ncuts > 1) {
            if (int rc = tick()) return rc;
            hipLaunchKernelGGL(k_gz_find, dim3((unsigned)(p.ncuts - 1)), dim3(kWave), 0, st, d_in.p, (uint32_t)p.nbytes, p.chunk_bytes,
                               p.ncuts, d_cand.p, d_kind.p);
            if (int rc = tock(0)) return rc;
        }
        return 0;   // count() brings the candidates back with the results
    }
    int count(Plan &p) {
        const size_t nc = (size_t)p.ncuts;
        if (int rc = room(d_res, p.ncuts)) return rc;
        if (int rc = tick()) return rc;
        hipLaunchKernelGGL(k_gz_count, dim3((unsigned)p.ncuts), dim3(kWave), 0, st, d_in.p, (uint32_t)p.nbytes, d_cand.p, d_kind.p,
                           p.ncuts, 8 * p.chunk_bytes, p.limit_bits, d_res.p);
        if (int rc = tock(1)) return rc;
        PCABI_TRY(hipMemcpyAsync(p.cand.data(), d_cand, 8 * nc, hipMemcpyDeviceToHost, st));
        PCABI_TRY(hipMemcpyAsync(p.kind.data(), d_kind, 4 * nc, hipMemcpyDeviceToHost, st));
        PCABI_TRY(hipMemcpyAsync(p.res.data(), d_res, sizeof(ChunkRes) * nc, hipMemcpyDeviceToHost, st));
        PCABI_TRY(hipStreamSynchronize(st));
        return 0;
    }
    int run(Plan &p, uint8_t *out, uint32_t *crc, int32_t *status, uint8_t *win_last) {
        const int64_t nc = (int64_t)p.conf.size(), total = p.off[(size_t)nc];
        tile_chunk.clear();
        tile_at.clear();
        for (int64_t i = 0; i < nc; ++i)
            for (int64_t at = 0; at < p.off[i + 1] - p.off[i]; at += kTile) {
                tile_chunk.push_back((int32_t)i);
                tile_at.push_back(at);
            }
        const int64_t nt = (int64_t)tile_chunk.size();
        tile_crc.assign((size_t)nt, 0);
        tile_status.assign((size_t)nt, 0);
        if (int rc = room(d_conf, nc)) return rc;
        if (int rc = room(d_off, nc + 1)) return rc;
        if (int rc = room(d_minm, nc)) return rc;
        if (int rc = room(d_status, nc)) return rc;
        if (int rc = room(d_win, (nc + 1) * (int64_t)kWindow)) return rc;
        if (int rc = room(d_sym, total + 16)) return rc;
        if (int rc = room(d_out, total + 16)) return rc;
        if (int rc = room(pin_out, total + 16)) return rc;
        if (int rc = room(d_tile_chunk, nt + 1)) return rc;
        if (int rc = room(d_tile_at, nt + 1)) return rc;
        if (int rc = room(d_tile_crc, nt + 1)) return rc;
        if (int rc = room(d_tile_status, nt + 1)) return rc;
        PCABI_TRY(hipMemcpyAsync(d_conf, p.conf.data(), 4 * (size_t)nc, hipMemcpyHostToDevice, st));
        PCABI_TRY(hipMemcpyAsync(d_off, p.off.data(), 8 * (size_t)(nc + 1), hipMemcpyHostToDevice, st));
        PCABI_TRY(hipMemcpyAsync(d_minm, p.min_marker.data(), 4 * (size_t)nc, hipMemcpyHostToDevice, st));
        PCABI_TRY(hipMemcpyAsync(d_win, p.win0, kWindow, hipMemcpyHostToDevice, st));
        if (nt > 0) {
            PCABI_TRY(hipMemcpyAsync(d_tile_chunk, tile_chunk.data(), 4 * (size_t)nt, hipMemcpyHostToDevice, st));
            PCABI_TRY(hipMemcpyAsync(d_tile_at, tile_at.data(), 8 * (size_t)nt, hipMemcpyHostToDevice, st));
        }
        if (int rc = tick()) return rc;
        hipLaunchKernelGGL(k_gz_decode, dim3((unsigned)nc), dim3(kWave), 0, st, d_in.p, (uint32_t)p.nbytes, d_cand.p, d_kind.p, p.ncuts,
                           8 * p.chunk_bytes, p.limit_bits, d_conf.p, d_off.p, d_sym.p, total, d_status.p);
        if (int rc = tock(2)) return rc;
        if (int rc = tick()) return rc;
        hipLaunchKernelGGL(k_gz_window, dim3(1), dim3(kWinThreads), 0, st, d_sym.p, d_off.p, nc, d_win.p);
        if (int rc = tock(3)) return rc;
        if (nt > 0) {
            if (int rc = tick()) return rc;
            hipLaunchKernelGGL(k_gz_resolve, dim3((unsigned)nt), dim3(kResThreads), 0, st, d_sym.p, d_off.p, d_tile_chunk.p, d_tile_at.p,
                               d_win.p, d_minm.p, d_out.p, total, d_tile_crc.p, d_tile_status.p);
            if (int rc = tock(4)) return rc;
            PCABI_TRY(hipMemcpyAsync(tile_crc.data(), d_tile_crc, 4 * (size_t)nt, hipMemcpyDeviceToHost, st));
            PCABI_TRY(hipMemcpyAsync(tile_status.data(), d_tile_status, 4 * (size_t)nt, hipMemcpyDeviceToHost, st));
            PCABI_TRY(hipMemcpyAsync(pin_out, d_out, (size_t)total, hipMemcpyDeviceToHost, st));
        }
        PCABI_TRY(hipMemcpyAsync(status, d_status, 4 * (size_t)nc, hipMemcpyDeviceToHost, st));
        PCABI_TRY(hipMemcpyAsync(win_last, d_win.p + nc * (int64_t)kWindow, kWindow, hipMemcpyDeviceToHost, st));
        PCABI_TRY(hipStreamSynchronize(st));
        if (total > 0) par_memcpy(out, pin_out, (size_t)total);
        for (int64_t i = 0; i < nc; ++i) crc[i] = 0;
        for (int64_t t = 0; t < nt; ++t) {
            const int64_t i = tile_chunk[(size_t)t];
            const int64_t len = std::min<int64_t>(kTile, p.off[i + 1] - p.off[i] - tile_at[(size_t)t]);
            crc[i] = crc_combine(crc[i], tile_crc[(size_t)t], (uint64_t)len);
            if (tile_status[(size_t)t] && !status[i]) status[i] = tile_status[(size_t)t];
        }
        return 0;
    }
};

Tune tune_now() {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_tune;
}

// kept for the process and never destroyed (a deliberate leak, as pcabi_inflate.hip's stage)
DevBackend *g_be = nullptr;
int g_be_device = -1;
std::mutex g_call_mu;

}  // namespace

namespace pcabi_internal {

// ---- the streaming source behind pcabi_fastx_open_dev2 (csrc/pcabi_io.cpp) ---------------------
// A thread of the reader's own runs the stream span by span on its own HIP stream and keeps up to
// two decoded spans ahead of the parser.
struct GzStreamReader {
    const uint8_t *z = nullptr;
    int64_t n = 0;
    int device = 0;
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    struct Item {
        std::vector<uint8_t> bytes;
        int rc = 1;   // 1: bytes; 0: the end; < 0: an error, msg
        std::string msg;
        int64_t stats[ST_N];
    };
    std::deque<Item> q;
    bool stop = false;
    Item cur;
    size_t at = 0;
    bool ended = false;
};

static void reader_main(GzStreamReader *g) {
    DevBackend *be = nullptr;
    int rc = 1;
    std::string msg;
    if (hipSetDevice(g->device) != hipSuccess) {
        rc = PCABI_E_DEVICE;
        msg = "hipSetDevice failed";
    } else {
        be = new DevBackend();
    }
    GzStream<DevBackend> *s = be ? new GzStream<DevBackend>(g->z, g->n, tune_now(), *be) : nullptr;
    while (rc > 0) {
        GzStreamReader::Item it;
        rc = s->next(it.bytes);
        it.rc = rc;
        if (rc < 0) it.msg = s->err ? s->err_msg : std::string(pcabi_last_error());
        std::copy(s->stats, s->stats + ST_N, it.stats);
        std::unique_lock<std::mutex> lk(g->mu);
        g->cv.wait(lk, [&] { return g->stop || g->q.size() < 2; });
        if (g->stop) break;
        g->q.push_back(std::move(it));
        g->cv.notify_all();
    }
    if (!s && rc < 0) {
        GzStreamReader::Item it;
        it.rc = rc;
        it.msg = msg;
        std::fill(it.stats, it.stats + ST_N, 0);
        std::lock_guard<std::mutex> lk(g->mu);
        g->q.push_back(std::move(it));
        g->cv.notify_all();
    }
    delete s;
    delete be;   // its device is current on this thread
}

int gzstream_reader_open(const uint8_t *z, int64_t n, int device, GzStreamReader **out) {
    *out = nullptr;
    GzStreamReader *g = new GzStreamReader();
    g->z = z;
    g->n = n;
    g->device = device;
    g->th = std::thread(reader_main, g);
    *out = g;
    return 0;
}

// up to room decoded bytes into dst: > 0, 0 at the end of the stream, or a negative code (message
// set) once everything before the bad place has been handed out
int64_t gzstream_reader_read(GzStreamReader *g, char *dst, int64_t room) {
    for (;;) {
        if (g->at < g->cur.bytes.size()) {
            const int64_t k = std::min<int64_t>(room, (int64_t)(g->cur.bytes.size() - g->at));
            std::memcpy(dst, g->cur.bytes.data() + g->at, (size_t)k);
            g->at += (size_t)k;
            return k;
        }
        if (g->ended) return g->cur.rc < 0 ? fail(g->cur.rc, g->cur.msg) : 0;
        std::unique_lock<std::mutex> lk(g->mu);
        g->cv.wait(lk, [&] { return !g->q.empty(); });
        g->cur = std::move(g->q.front());
        g->q.pop_front();
        g->at = 0;
        g->cv.notify_all();
        lk.unlock();
        std::copy(g->cur.stats, g->cur.stats + ST_N, t_stats);
        if (g->cur.rc <= 0) {
            g->ended = true;
            g->cur.bytes.clear();
        }
    }
}

void gzstream_reader_close(GzStreamReader *g) {
    if (!g) return;
    {
        std::lock_guard<std::mutex> lk(g->mu);
        g->stop = true;
        g->cv.notify_all();
    }
    if (g->th.joinable()) g->th.join();
    delete g;
}

}  // namespace pcabi_internal

extern "C" {

int pcabi_gunzip_stream_tune(int64_t chunk_bytes, int64_t span_bytes, int64_t min_chunks) {
    if (chunk_bytes < 0 || span_bytes < 0 || min_chunks < 0 || (chunk_bytes && chunk_bytes < 512) || span_bytes > kSpanInMax ||
        chunk_bytes > kSpanInMax)
        return fail(PCABI_E_ARG, "chunk_bytes 512.., span_bytes up to 96 MiB, min_chunks >= 0 (0 = the default)");
    std::lock_guard<std::mutex> lk(g_mu);
    g_tune.chunk_bytes = chunk_bytes ? chunk_bytes : kDefaultTune.chunk_bytes;
    g_tune.span_bytes = span_bytes ? span_bytes : kDefaultTune.span_bytes;
    g_tune.min_chunks = min_chunks ? min_chunks : kDefaultTune.min_chunks;
    if (g_tune.span_bytes < g_tune.chunk_bytes) g_tune.span_bytes = g_tune.chunk_bytes;
    return 0;
}

void pcabi_gunzip_stream_last_stats(int64_t *s) {
    if (s) std::copy(t_stats, t_stats + ST_N, s);
}

void pcabi_gunzip_stream_last_times(int on, int reset, double *ms) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (on >= 0) g_time_on = on != 0;
    if (ms) std::copy(g_ms, g_ms + 5, ms);
    if (reset) std::fill(g_ms, g_ms + 5, 0.0);
}

int64_t pcabi_gunzip_stream_host(int device, const uint8_t *z, int64_t n, uint8_t *out, int64_t cap) {
    if (n < 0 || cap < 0 || (n > 0 && !z) || (cap > 0 && !out)) return fail(PCABI_E_ARG, "bad arguments");
    std::lock_guard<std::mutex> lk(g_call_mu);
    if (device < 0) PCABI_TRY(hipGetDevice(&device));
    PCABI_TRY(hipSetDevice(device));
    if (g_be && g_be_device != device) {
        (void)hipSetDevice(g_be_device);
        delete g_be;
        g_be = nullptr;
        PCABI_TRY(hipSetDevice(device));
    }
    if (!g_be) g_be = new DevBackend();
    g_be_device = device;
    GzStream<DevBackend> s(z, n, tune_now(), *g_be);
    std::vector<uint8_t> acc;
    int rc;
    while ((rc = s.next(acc)) > 0) {
    }
    std::copy(s.stats, s.stats + ST_N, t_stats);
    if (rc < 0) return s.err ? fail(s.err, s.err_msg) : rc;
    const int64_t total = (int64_t)acc.size();
    if (total > cap) return total;
    if (total > 0) par_memcpy(out, acc.data(), (size_t)total);
    return total;
}

}  // extern "C"
