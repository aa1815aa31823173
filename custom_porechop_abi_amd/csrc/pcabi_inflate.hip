// pcabi_inflate.hip -- block-gzipped (BGZF) input inflated on the GPU (gfx950): include/pcabi.h
// pcabi_gunzip_*; DESIGN.md "gunzip on the device".
//
// k_inflate: one workgroup of one wavefront per gzip member. The member's whole output (at most
// 64 KiB) lives in LDS and is the LZ77 window; next to it the decode tables (pcabi_inflate.h
// Tables, 15 KiB), so two workgroups share a CU's 160 KiB. The decoder is pcabi_inflate.h's, with
// the wave-wide policies below: every lane runs the serial symbol loop on the same values (table
// lookups are LDS broadcasts, input bytes come from one address), one lane stores literals, match
// and stored-block copies and the table construction are spread over the 64 lanes. After the last
// block the wave computes the CRC-32 (16-byte lane chunks, each multiplied by x^(8 * bytes after it)
// mod P and xor-reduced, the encoder's scheme) and, when it matches, writes the member from LDS to
// global memory as aligned 16-byte stores with bytes at the ragged ends.
// All stores are plain C++ stores.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/pcabi.h"
#include "pcabi_crc.h"
#include "pcabi_hostdev.h"
#include "pcabi_inflate.h"

using namespace pcabi_internal;
using namespace pcabi_inflate;
using namespace pcabi_crc;

namespace {

constexpr int kWave = 64;

__device__ const CrcTables d_tab = make_tables();

struct WavePar {
    __device__ int lane() const { return (int)threadIdx.x; }
    __device__ int lanes() const { return kWave; }
    __device__ void sync() const { __syncthreads(); }
};

// the member's output in LDS; crc() borrows the (finished) decode tables' space for its tables
struct WaveSink {
    uint8_t *win;
    uint32_t *tab;   // 768 words
    __device__ void put(uint32_t pos, uint8_t c) {
        if (threadIdx.x == 0) win[pos] = c;
    }
    // out[pos + i] = out[pos - dist + i % dist]: every source byte lies before pos
    __device__ void copy(uint32_t pos, uint32_t dist, uint32_t len) {
        __syncthreads();
        const uint32_t from = pos - dist;
        for (uint32_t i = threadIdx.x; i < len; i += kWave) win[pos + i] = win[from + (dist >= len ? i : i % dist)];
        __syncthreads();
    }
    __device__ void store(uint32_t pos, const uint8_t *src, uint32_t len) {
        for (uint32_t i = threadIdx.x; i < len; i += kWave) win[pos + i] = src[i];
    }
    __device__ uint32_t crc(uint32_t len) {
        __syncthreads();
        for (int i = threadIdx.x; i < 256; i += kWave) {
            tab[i] = d_tab.byte[i];
            tab[256 + i] = d_tab.xp[0][i];
            tab[512 + i] = d_tab.xp[1][i];
        }
        __syncthreads();
        uint32_t acc = 0;
        for (uint32_t first = threadIdx.x * 16u; first < len; first += kWave * 16u) {
            const uint32_t m = min(16u, len - first);
            uint32_t c = 0xffffffffu;
            for (uint32_t j = 0; j < m; ++j) c = tab[(c ^ win[first + j]) & 0xff] ^ (c >> 8);
            c ^= 0xffffffffu;
            const uint32_t after = len - (first + m);   // < 65536
            uint32_t xp = tab[256 + (after & 255)];
            if (after >> 8) xp = mulmod(xp, tab[512 + (after >> 8)]);
            acc ^= mulmod(c, xp);
        }
        for (int d = 32; d >= 1; d >>= 1) acc ^= __shfl_xor(acc, d);
        return acc;
    }
};

__global__ __launch_bounds__(kWave) void k_inflate(const uint8_t *__restrict__ z, int64_t n,
                                                   const int64_t *__restrict__ in_off,
                                                   const int64_t *__restrict__ out_off, uint8_t *__restrict__ out,
                                                   int64_t out_cap, int32_t *__restrict__ status) {
    __shared__ __attribute__((aligned(16))) uint8_t win[kMemberMax];
    __shared__ Tables t;
    const int64_t m = blockIdx.x;
    const int64_t lo = in_off[m], hi = in_off[m + 1], olo = out_off[m], ohi = out_off[m + 1];
    int st;
    uint32_t len = 0;
    if (lo < 0 || hi < lo || hi > n) {   // uniform
        st = PCABI_INFLATE_E_HEADER;
    } else if (olo < 0 || ohi < olo || ohi > out_cap || ohi - olo > kMemberMax) {
        st = PCABI_INFLATE_E_OUTPUT;
    } else {
        WavePar par;
        WaveSink sink{win, t.lit};
        st = inflate_member(par, sink, t, z + lo, hi - lo, (uint32_t)(ohi - olo), &len);
    }
    if (threadIdx.x == 0) status[m] = st;
    if (st != 0) return;
    // LDS -> global: bytes up to the first 16-byte boundary of the destination, aligned 16-byte
    // stores, bytes after the last boundary
    uint8_t *o = out + olo;
    const uint32_t head = min(len, (uint32_t)((16u - ((uintptr_t)o & 15u)) & 15u));
    const uint32_t nvec = (len - head) / 16u, tail0 = head + nvec * 16u;
    if (threadIdx.x < head) o[threadIdx.x] = win[threadIdx.x];
    for (uint32_t v = threadIdx.x; v < nvec; v += kWave) {
        const uint8_t *s = win + head + v * 16u;
        uint32_t w[4];
        if ((head & 3u) == 0) {   // uniform: the LDS side is word-aligned too
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = ((const uint32_t *)s)[k];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                w[k] = (uint32_t)s[4 * k] | (uint32_t)s[4 * k + 1] << 8 | (uint32_t)s[4 * k + 2] << 16 |
                       (uint32_t)s[4 * k + 3] << 24;
        }
        *(uint4 *)(o + head + v * 16u) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    if (tail0 + threadIdx.x < len) o[tail0 + threadIdx.x] = win[tail0 + threadIdx.x];
}

// ---- host side ---------------------------------------------------------------------------------

constexpr int64_t kDefaultChunk = 32ll << 20;
int64_t g_chunk_bytes = kDefaultChunk;

int launch(hipStream_t st, const uint8_t *z, int64_t n, const int64_t *in_off, const int64_t *out_off, int64_t nm,
           uint8_t *out, int64_t out_cap, int32_t *status) {
    if (nm > 0) hipLaunchKernelGGL(k_inflate, dim3((unsigned)nm), dim3(kWave), 0, st, z, n, in_off, out_off, out, out_cap, status);
    PCABI_TRY(hipGetLastError());
    return 0;
}

// The host entry's staging slots: pinned and device buffers kept between calls (one device at a
// time; a call on another device, or a larger pass, reallocates). One call runs at a time.
struct Slot {
    PinBuf<> pin_in, pin_out;
    PinBuf<int64_t> pin_off;   // in_off[members + 1], then out_off[members + 1]
    PinBuf<int32_t> pin_status;
    DevBuf<> dev_in, dev_out;
    DevBuf<int64_t> dev_off;
    DevBuf<int32_t> dev_status;
    int64_t m0 = 0, m1 = 0;
    Stream st;   // the last member: the first to go
    // f(buffer, elements) for every buffer of groups of up to in_bytes / out_bytes / members, until one
    // returns false
    template <class F>
    bool each(int64_t in_bytes, int64_t out_bytes, int64_t members, F f) {
        return f(pin_in, in_bytes + 16) && f(pin_out, out_bytes + 16) && f(pin_off, 2 * (members + 1)) &&
               f(pin_status, members + 4) && f(dev_in, in_bytes + 16) && f(dev_out, out_bytes + 16) &&
               f(dev_off, 2 * (members + 1)) && f(dev_status, members + 4);
    }
};
constexpr int kSlots = 2;
struct Stage {
    int device = -1;
    Slot s[kSlots];
    double t_copy_in = 0, t_sync = 0, t_copy_out = 0;
};
// kept for the process and never destroyed (a deliberate leak): a destructor at exit would call into a
// HIP runtime that may already have shut down
Stage &g_stage = *new Stage;
std::mutex g_stage_mu;

// a slot's stream and buffers for groups of up to in_bytes / out_bytes / members (current device)
int slot_alloc(Slot &s, int64_t in_bytes, int64_t out_bytes, int64_t members) {
    int rc = s.st.create();
    if (!rc) s.each(in_bytes, out_bytes, members, [&](auto &b, int64_t n) { return (rc = b.reserve(n, n)) == 0; });
    return rc;
}

// Whether the kept buffers serve is read from the buffers themselves, so a reserve that failed half-way
// is done again by the next call.
int stage_reserve(int device, int64_t in_bytes, int64_t out_bytes, int64_t members) {
    bool kept = g_stage.device == device;
    for (Slot &s : g_stage.s)
        kept = kept && s.each(in_bytes, out_bytes, members, [](auto &b, int64_t n) { return holds(b, n); });
    if (kept) return 0;
    if (g_stage.device >= 0) {
        (void)hipSetDevice(g_stage.device);
        for (Slot &s : g_stage.s) {
            s.st.release();
            s = Slot();
        }
    }
    PCABI_TRY(hipSetDevice(device));
    g_stage.device = device;
    for (Slot &s : g_stage.s)
        if (int rc = slot_alloc(s, in_bytes, out_bytes, members)) return rc;
    return 0;
}

}  // namespace

namespace pcabi_internal {

// Members [m0, m1) of an indexed stream cut into passes of at most `chunk` decoded bytes (a pass
// holds at least one member): pass p = members [pass[p], pass[p + 1]).
std::vector<int64_t> gunzip_passes(const int64_t *out_off, int64_t m0, int64_t m1, int64_t chunk) {
    std::vector<int64_t> pass{m0};
    int64_t first = m0;
    for (int64_t m = m0; m < m1; ++m)
        if (m > first && out_off[m + 1] - out_off[first] > chunk) {
            pass.push_back(m);
            first = m;
        }
    if (m1 > m0) pass.push_back(m1);
    return pass;
}

int64_t gunzip_chunk_bytes() { return g_chunk_bytes; }

// One group of members through a caller's own buffers, asynchronously on st: pinned pin_in / pin_off /
// pin_status and device buffers sized for the group. The decoded bytes land in pin_out.
int gunzip_group_async(void *stream, const uint8_t *z, const int64_t *in_off, const int64_t *out_off, int64_t m0,
                       int64_t m1, uint8_t *pin_in, int64_t *pin_off, uint8_t *dev_in, int64_t *dev_off,
                       uint8_t *dev_out, int32_t *dev_status, uint8_t *pin_out, int32_t *pin_status) {
    hipStream_t st = (hipStream_t)stream;
    const int64_t nm = m1 - m0, lo = in_off[m0], bytes = in_off[m1] - lo, olo = out_off[m0], obytes = out_off[m1] - olo;
    if (bytes > 0) par_memcpy(pin_in, z + lo, (size_t)bytes);
    for (int64_t m = m0; m <= m1; ++m) {
        pin_off[m - m0] = in_off[m] - lo;
        pin_off[nm + 1 + m - m0] = out_off[m] - olo;
    }
    const bool prof = prof_on();
    void *sp = prof ? prof_begin(st, 2) : nullptr;
    if (bytes > 0) PCABI_TRY(hipMemcpyAsync(dev_in, pin_in, (size_t)bytes, hipMemcpyHostToDevice, st));
    PCABI_TRY(hipMemcpyAsync(dev_off, pin_off, 16 * (size_t)(nm + 1), hipMemcpyHostToDevice, st));
    if (prof) prof_end(st, sp), sp = prof_begin(st, 0);
    if (int rc = launch(st, dev_in, bytes, dev_off, dev_off + nm + 1, nm, dev_out, obytes, dev_status)) return rc;
    if (prof) prof_end(st, sp), sp = prof_begin(st, 3);
    if (nm > 0) PCABI_TRY(hipMemcpyAsync(pin_status, dev_status, 4 * (size_t)nm, hipMemcpyDeviceToHost, st));
    if (obytes > 0) PCABI_TRY(hipMemcpyAsync(pin_out, dev_out, (size_t)obytes, hipMemcpyDeviceToHost, st));
    if (prof) prof_end(st, sp);
    return 0;
}

// the first failing member of a finished group as the decoder's error, or 0
int gunzip_group_check(const int32_t *pin_status, const int64_t *in_off, int64_t m0, int64_t m1) {
    for (int64_t m = m0; m < m1; ++m)
        if (pin_status[m - m0] != 0)
            return fail(PCABI_E_PARSE, "gzip member " + std::to_string(m) + " at offset " + std::to_string(in_off[m]) +
                                           " does not inflate (status " + std::to_string(pin_status[m - m0]) + ")");
    return 0;
}

// ---- the streaming source behind pcabi_fastx_open_dev (csrc/pcabi_io.cpp) ----------------------
// An indexed stream read group by group: while the caller consumes group p from pinned memory,
// group p + 1 inflates on the reader's own stream.
struct GunzipReader {
    const uint8_t *z = nullptr;
    int device = 0;
    std::vector<int64_t> in_off, out_off, pass;
    Slot s[kSlots];
    int64_t np = 0, consume = 0;       // passes; the next pass to hand out
    int64_t cur_len = 0, cur_at = 0;   // usable bytes of the pass being handed out, and the cursor
    uint8_t *cur = nullptr;
    int pending = 0;                   // a member failed: raised once the bytes before it are out
    std::string pending_msg;
};

static void reader_free(GunzipReader *g) {
    (void)hipSetDevice(g->device);
    delete g;
}

static int reader_launch(GunzipReader *g, int64_t p) {
    Slot &s = g->s[p % kSlots];
    s.m0 = g->pass[p];
    s.m1 = g->pass[p + 1];
    return gunzip_group_async(s.st, g->z, g->in_off.data(), g->out_off.data(), s.m0, s.m1, s.pin_in, s.pin_off, s.dev_in,
                              s.dev_off, s.dev_out, s.dev_status, s.pin_out, s.pin_status);
}

static int reader_alloc(GunzipReader *g, int64_t max_in, int64_t max_out, int64_t max_m) {
    PCABI_TRY(hipSetDevice(g->device));
    for (Slot &s : g->s)
        if (int rc = slot_alloc(s, max_in, max_out, max_m)) return rc;
    return 0;
}

// z[0, n) stays mapped by the caller until gunzip_reader_close. *out = nullptr (and 0 returned) when
// the stream is not indexable: the caller reads it with zlib. A negative code for a device error.
int gunzip_reader_open(const uint8_t *z, int64_t n, int device, GunzipReader **out) {
    *out = nullptr;
    const int64_t nm = gunzip_index(z, n, nullptr, nullptr, 0);
    if (nm <= 0) return 0;   // zlib reports a broken chain its own way
    GunzipReader *g = new GunzipReader();
    g->z = z;
    g->device = device;
    g->in_off.resize((size_t)nm + 1);
    g->out_off.resize((size_t)nm + 1);
    gunzip_index(z, n, g->in_off.data(), g->out_off.data(), nm + 1);
    int64_t chunk;
    {
        std::lock_guard<std::mutex> lk(g_stage_mu);
        chunk = g_chunk_bytes;
    }
    g->pass = gunzip_passes(g->out_off.data(), 0, nm, chunk);
    g->np = (int64_t)g->pass.size() - 1;
    int64_t max_in = 1, max_out = 1, max_m = 1;
    for (int64_t p = 0; p < g->np; ++p) {
        max_in = std::max(max_in, g->in_off[g->pass[p + 1]] - g->in_off[g->pass[p]]);
        max_out = std::max(max_out, g->out_off[g->pass[p + 1]] - g->out_off[g->pass[p]]);
        max_m = std::max(max_m, g->pass[p + 1] - g->pass[p]);
    }
    int rc = reader_alloc(g, max_in, max_out, max_m);
    if (!rc && g->np > 0) rc = reader_launch(g, 0);
    if (rc) {
        reader_free(g);
        return rc;
    }
    *out = g;
    return 0;
}

// up to room decoded bytes into dst: > 0, 0 at the end of the stream, or PCABI_E_PARSE (message
// set) once everything before the first failing member has been handed out
int64_t gunzip_reader_read(GunzipReader *g, char *dst, int64_t room) {
    for (;;) {
        if (g->cur_at < g->cur_len) {
            const int64_t k = std::min(room, g->cur_len - g->cur_at);
            std::memcpy(dst, g->cur + g->cur_at, (size_t)k);
            g->cur_at += k;
            return k;
        }
        if (g->pending) return fail(g->pending, g->pending_msg);
        if (g->consume >= g->np) return 0;
        PCABI_TRY(hipSetDevice(g->device));
        const int64_t p = g->consume++;
        Slot &s = g->s[p % kSlots];
        PCABI_TRY(hipStreamSynchronize(s.st));
        int64_t good = s.m1;
        for (int64_t m = s.m0; m < s.m1; ++m)
            if (s.pin_status[m - s.m0] != 0) {
                good = m;
                g->pending = PCABI_E_PARSE;
                g->pending_msg = "gzip member " + std::to_string(m) + " at offset " + std::to_string(g->in_off[m]) +
                                 " does not inflate (status " + std::to_string(s.pin_status[m - s.m0]) + ")";
                break;
            }
        g->cur = s.pin_out;
        g->cur_at = 0;
        g->cur_len = g->out_off[good] - g->out_off[s.m0];
        if (!g->pending && p + 1 < g->np)
            if (int rc = reader_launch(g, p + 1)) return rc;
    }
}

// The rest of the current group, or the next group, in place: its bytes in pinned memory (*host) and
// on the device (*dev), both valid until the call after the next one; *stream = the stream that
// inflated it (the group two further on is launched on it). Returns the length (> 0), 0 at the end of
// the stream, or a negative code as gunzip_reader_read does.
int64_t gunzip_reader_take(GunzipReader *g, const uint8_t **host, const uint8_t **dev, void **stream) {
    for (;;) {
        if (g->cur_at < g->cur_len) {
            Slot &s = g->s[(g->consume - 1) % kSlots];
            const int64_t k = g->cur_len - g->cur_at;
            *host = g->cur + g->cur_at;
            *dev = s.dev_out + g->cur_at;
            *stream = s.st;
            g->cur_at = g->cur_len;
            return k;
        }
        char none;
        const int64_t rc = gunzip_reader_read(g, &none, 0);   // room 0: moves to the next group, copies nothing
        if (rc < 0) return rc;
        if (g->cur_at >= g->cur_len) {
            if (g->pending) return fail(g->pending, g->pending_msg);
            if (g->consume >= g->np) return 0;
        }
    }
}

// hand the current group out again from its first byte (the type sniff of pcabi_fastx_open_dev read
// from it)
void gunzip_reader_unread(GunzipReader *g) { g->cur_at = 0; }

int gunzip_reader_device(const GunzipReader *g) { return g->device; }

// the stream's decoded length, from the index
int64_t gunzip_reader_total(const GunzipReader *g) { return g->out_off.empty() ? 0 : g->out_off.back(); }

void gunzip_reader_close(GunzipReader *g) {
    if (g) reader_free(g);
}

}  // namespace pcabi_internal

extern "C" {

int64_t pcabi_gunzip_index(const uint8_t *z, int64_t n, int64_t *in_off, int64_t *out_off, int64_t cap) {
    if (n < 0 || (n > 0 && !z) || cap < 0) return fail(PCABI_E_ARG, "bad arguments");
    const int64_t m = gunzip_index(z, n, in_off, out_off, cap);
    if (m < 0) return fail(PCABI_E_PARSE, "not a chain of gzip members (truncated file?)");
    return m;
}

int64_t pcabi_gunzip_scratch_bytes(int64_t n_members) {
    if (n_members < 0) return fail(PCABI_E_ARG, "negative size");
    return 0;
}

int pcabi_gunzip_tune(int64_t chunk_bytes) {
    if (chunk_bytes < 0 || chunk_bytes > (1ll << 31)) return fail(PCABI_E_ARG, "chunk_bytes 1..2 GiB (0 = default)");
    std::lock_guard<std::mutex> lk(g_stage_mu);
    g_chunk_bytes = chunk_bytes ? chunk_bytes : kDefaultChunk;
    return 0;
}

int pcabi_gunzip_dev(void *stream, const uint8_t *z, int64_t n, const int64_t *in_off, const int64_t *out_off,
                     int64_t n_members, uint8_t *out, int64_t out_cap, int32_t *status, void *scratch,
                     int64_t scratch_len) {
    (void)scratch;
    if (n < 0 || n_members < 0 || out_cap < 0 || scratch_len < 0 || n_members > INT32_MAX || (n > 0 && !z) ||
        (out_cap > 0 && !out) || (n_members > 0 && (!in_off || !out_off || !status)))
        return fail(PCABI_E_ARG, "bad arguments");
    return launch((hipStream_t)stream, z, n, in_off, out_off, n_members, out, out_cap, status);
}

int64_t pcabi_gunzip_host(int device, const uint8_t *z, int64_t n, uint8_t *out, int64_t cap) {
    if (n < 0 || cap < 0 || (n > 0 && !z) || (cap > 0 && !out)) return fail(PCABI_E_ARG, "bad arguments");
    const int64_t nm = gunzip_index(z, n, nullptr, nullptr, 0);
    if (nm < 0) return fail(PCABI_E_PARSE, "not a chain of gzip members (truncated file?)");
    if (nm == 0) return fail(PCABI_E_ARG, "not block-gzipped: a member without a BC subfield");
    std::vector<int64_t> in_off((size_t)nm + 1), out_off((size_t)nm + 1);
    gunzip_index(z, n, in_off.data(), out_off.data(), nm + 1);
    const int64_t total = out_off[nm];
    if (total > cap) return total;
    std::lock_guard<std::mutex> lk(g_stage_mu);
    const std::vector<int64_t> pass = pcabi_internal::gunzip_passes(out_off.data(), 0, nm, g_chunk_bytes);
    const int64_t np = (int64_t)pass.size() - 1;
    int64_t max_in = 0, max_out = 0, max_m = 0;
    for (int64_t p = 0; p < np; ++p) {
        max_in = std::max(max_in, in_off[pass[p + 1]] - in_off[pass[p]]);
        max_out = std::max(max_out, out_off[pass[p + 1]] - out_off[pass[p]]);
        max_m = std::max(max_m, pass[p + 1] - pass[p]);
    }
    if (device < 0) PCABI_TRY(hipGetDevice(&device));
    PCABI_TRY(hipSetDevice(device));
    if (int rc = stage_reserve(device, std::max<int64_t>(max_in, 1 << 16), std::max<int64_t>(max_out, 1 << 16),
                               std::max<int64_t>(max_m, 16)))
        return rc;
    g_stage.t_copy_in = g_stage.t_sync = g_stage.t_copy_out = 0;
    int rc_all = 0;
    for (int64_t i = 0; i < np + 1; ++i) {
        if (i < np && !rc_all) {   // stage A: copy up, kernel, status and bytes back to pinned memory
            Slot &s = g_stage.s[i % kSlots];
            s.m0 = pass[i];
            s.m1 = pass[i + 1];
            const double t0 = now_s();
            const int rc = pcabi_internal::gunzip_group_async(s.st, z, in_off.data(), out_off.data(), s.m0, s.m1, s.pin_in,
                                                              s.pin_off, s.dev_in, s.dev_off, s.dev_out, s.dev_status,
                                                              s.pin_out, s.pin_status);
            g_stage.t_copy_in += now_s() - t0;
            if (rc) rc_all = rc;
        }
        if (i >= 1) {   // stage B: into the caller's buffer
            Slot &s = g_stage.s[(i - 1) % kSlots];
            double t0 = now_s();
            PCABI_TRY(hipStreamSynchronize(s.st));
            g_stage.t_sync += now_s() - t0;
            if (!rc_all) rc_all = pcabi_internal::gunzip_group_check(s.pin_status, in_off.data(), s.m0, s.m1);
            t0 = now_s();
            if (!rc_all) par_memcpy(out + out_off[s.m0], s.pin_out, (size_t)(out_off[s.m1] - out_off[s.m0]));
            g_stage.t_copy_out += now_s() - t0;
        }
    }
    return rc_all ? rc_all : total;
}

void pcabi_gunzip_last_times(double *copy_in, double *wait, double *copy_out) {
    std::lock_guard<std::mutex> lk(g_stage_mu);
    if (copy_in) *copy_in = g_stage.t_copy_in;
    if (wait) *wait = g_stage.t_sync;
    if (copy_out) *copy_out = g_stage.t_copy_out;
}

}  // extern "C"
