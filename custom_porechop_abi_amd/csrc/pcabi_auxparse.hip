// pcabi_auxparse.hip -- SAM tags read from FASTQ / FASTA headers, on the GPU (gfx950): include/pcabi.h
// pcabi_auxparse_*, pcabi_fastx_header_tags; DESIGN.md "Tags read from text headers"; the rule and the
// wave's walk are csrc/pcabi_auxparse.h's (wave_parse), which the CPU fuzz program plays lane by lane.
//
// k_auxparse_size: one wave per header; per part the chain's length, its float count, the tags read and
//   the fields left out (24 bytes a part go back).
// k_auxparse_write: one wave per header; the chain into out[part.out, part.out + part.len) and a Fix
//   record per float into the part's own slots [fix0, fix0 + n_float) of the fix-up table (fix0: the
//   host's prefix sum over the float counts). A part whose plan left no field out is stored in the pass
//   that checks it; any other part has each array checked before it is stored.
// The host fills the fix-ups with strtod once the chains are back (fill_floats): it reads the texts the
// records name, never the headers.
// Every load stays inside the part's text and every store inside the part's own length (put, fix_put);
// every loop runs to a length the host passed. No atomics, no inline assembly.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/pcabi.h"
#include "pcabi_auxparse.h"
#include "pcabi_hostdev.h"

using namespace pcabi_internal;
using namespace pcabi_auxparse;

namespace {

constexpr int kWave = 64;
constexpr int64_t kGuard = 64;

// what k_auxparse_size leaves per part
struct ParseSize {
    int64_t len;
    int32_t n_float, tags, left_out, reserved;
};

// the hardware's wave for wave_parse
struct DevWave {
    int lane;
    template <class F>
    __device__ uint64_t ballot(F f) {
        return __ballot(f(lane));
    }
    template <class F>
    __device__ void each(F f) {
        f(lane);
    }
};

__global__ __launch_bounds__(kWave) void k_auxparse_size(const uint8_t *__restrict__ text, int64_t text_n,
                                                         const pcabi_auxparse_part *__restrict__ parts, int64_t n_parts,
                                                         ParseSize *__restrict__ sizes) {
    const int64_t pi = blockIdx.x;
    if (pi >= n_parts) return;
    const pcabi_auxparse_part p = parts[pi];
    DevWave w{(int)threadIdx.x};
    Counts c{0, 0, 0};
    int64_t len = 0;
    if (part_fits(p, text_n))   // uniform
        len = wave_parse(w, text + p.text_off, p.text_len, nullptr, 0, nullptr, 0, 0, 0, 0, false, &c);
    if (threadIdx.x == 0) sizes[pi] = ParseSize{len, (int32_t)c.n_float, (int32_t)c.tags, (int32_t)c.left_out, 0};
}

__global__ __launch_bounds__(kWave) void k_auxparse_write(const uint8_t *__restrict__ text, int64_t text_n,
                                                          const pcabi_auxparse_part *__restrict__ parts, int64_t n_parts,
                                                          const int64_t *__restrict__ fix0, Fix *__restrict__ fix, int64_t n_fix,
                                                          uint8_t *__restrict__ out, int64_t out_cap) {
    const int64_t pi = blockIdx.x;
    if (pi >= n_parts) return;
    const pcabi_auxparse_part p = parts[pi];
    if (!part_fits(p, text_n) || p.len <= 0 || p.out < 0 || p.len > out_cap - p.out || p.n_float < 0) return;   // uniform
    // the part's own fix-up slots, inside the table
    int64_t lo = fix ? fix0[pi] : 0, hi = lo + p.n_float;
    if (!fix || lo < 0 || hi > n_fix) lo = hi = 0;
    DevWave w{(int)threadIdx.x};
    wave_parse(w, text + p.text_off, p.text_len, out + p.out, p.len, fix, lo, hi, p.text_off, p.out, p.left_out == 0, nullptr);
}

std::atomic<int64_t> g_tags{0}, g_left_out{0};

// ---- device-event timing (tools/header_tags_read_timing.py) ----
KernelTimes g_times;
struct Span : EventSpan {
    void begin(hipStream_t st) { EventSpan::begin(g_times, st); }
    void harvest(int kind, int64_t bytes) { EventSpan::harvest(g_times, kind, bytes); }
};

int check_parts(const pcabi_auxparse_part *parts, int64_t n_parts, int64_t text_n) {
    for (int64_t i = 0; i < n_parts; ++i)
        if (!part_fits(parts[i], text_n) || parts[i].text_len > INT32_MAX)
            return fail(PCABI_E_ARG, "part " + std::to_string(i) + " does not lie inside the text");
    return 0;
}

// fn(t) for t in [0, nt) on threads of its own
template <class F>
void fan(int nt, F &&fn) {
    if (nt <= 1) {
        fn(0);
        return;
    }
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t) th.emplace_back(fn, t);
    for (auto &x : th) x.join();
}
int threads_for(int64_t n_parts) { return (int)std::min<int64_t>(io_thread_count(), std::max<int64_t>(1, n_parts / 256)); }

// the host build of the plan, the parts dealt to the io threads in ranges
void plan_host(const uint8_t *text, pcabi_auxparse_part *parts, int64_t n_parts) {
    const int nt = threads_for(n_parts);
    fan(nt, [&](int t) {
        for (int64_t i = n_parts * t / nt; i < n_parts * (t + 1) / nt; ++i) {
            Counts c;
            parts[i].len = parse(text + parts[i].text_off, parts[i].text_len, nullptr, 0, false, &c);
            parts[i].n_float = (int32_t)c.n_float, parts[i].tags = (int32_t)c.tags, parts[i].left_out = (int32_t)c.left_out;
        }
    });
}
void write_host(const uint8_t *text, const pcabi_auxparse_part *parts, int64_t n_parts, uint8_t *out) {
    const int nt = threads_for(n_parts);
    fan(nt, [&](int t) {
        for (int64_t i = n_parts * t / nt; i < n_parts * (t + 1) / nt; ++i)
            if (parts[i].len > 0)
                parse(text + parts[i].text_off, parts[i].text_len, out + parts[i].out, parts[i].len, parts[i].left_out == 0, nullptr);
    });
}
void count(const pcabi_auxparse_part *parts, int64_t n_parts) {
    int64_t a = 0, b = 0;
    for (int64_t i = 0; i < n_parts; ++i) a += parts[i].tags, b += parts[i].left_out;
    g_tags += a, g_left_out += b;
}

// The floats of the chains in out[0, out_cap): every record names a text the device found well-formed;
// one that does not lie inside the buffers, or is not a float after all, is a device fault.
int fill_floats(const uint8_t *text, int64_t text_n, const Fix *fix, int64_t n_fix, uint8_t *out, int64_t out_cap) {
    for (int64_t k = 0; k < n_fix; ++k) {
        const Fix &f = fix[k];
        if (f.len < 1 || f.len > kMaxFloat || f.text_off < 0 || f.text_off > text_n - f.len || f.out_off < 0 || f.out_off > out_cap - 4 ||
            !float_scan(text + f.text_off, f.len))
            return fail(PCABI_E_DEVICE, "k_auxparse_write left a fix-up record that names no float");
        const float x = float_value(text + f.text_off, f.len);
        std::memcpy(out + f.out_off, &x, 4);
    }
    return 0;
}

}  // namespace

// The device side of one reader (or one call): the buffers kept between batches and the stream.
struct pcabi_internal::AuxParseDev {
    int device = -1;
    Stream st;
    DevBuf<> text, out;
    DevBuf<pcabi_auxparse_part> parts;
    DevBuf<ParseSize> sizes;
    DevBuf<int64_t> fix0;
    DevBuf<Fix> fix;
    std::vector<ParseSize> h_sizes;
    std::vector<int64_t> h_fix0;
    std::vector<Fix> h_fix;
};

namespace {

int64_t grow(int64_t n) { return n + n / 4 + 64; }

// the text up (once), k_auxparse_size over the table, parts[] filled from what comes back. Synchronises.
int size_dev(AuxParseDev *d, hipStream_t st, const uint8_t *text, int64_t text_n, pcabi_auxparse_part *parts, int64_t n_parts) {
    if (n_parts >= INT32_MAX) return fail(PCABI_E_ARG, "too many parts for one launch");
    if (n_parts <= 0) return 0;
    if (int rc = d->text.reserve(text_n + 64, grow(text_n + 64))) return rc;
    if (int rc = d->parts.reserve(n_parts, grow(n_parts))) return rc;
    if (int rc = d->sizes.reserve(n_parts, grow(n_parts))) return rc;
    d->h_sizes.assign((size_t)n_parts, ParseSize{0, 0, 0, 0, 0});
    if (text_n > 0) PCABI_TRY(hipMemcpyAsync(d->text, text, (size_t)text_n, hipMemcpyHostToDevice, st));
    PCABI_TRY(hipMemcpyAsync(d->parts, parts, (size_t)n_parts * sizeof(pcabi_auxparse_part), hipMemcpyHostToDevice, st));
    Span sp;
    sp.begin(st);
    hipLaunchKernelGGL(k_auxparse_size, dim3((unsigned)n_parts), dim3(kWave), 0, st, d->text.p, text_n, d->parts.p, n_parts, d->sizes.p);
    PCABI_TRY(hipGetLastError());
    sp.end(st);
    PCABI_TRY(hipMemcpyAsync(d->h_sizes.data(), d->sizes, (size_t)n_parts * sizeof(ParseSize), hipMemcpyDeviceToHost, st));
    PCABI_TRY(hipStreamSynchronize(st));
    int64_t bytes = 0;
    for (int64_t i = 0; i < n_parts; ++i) {
        const ParseSize &z = d->h_sizes[(size_t)i];
        parts[i].len = z.len, parts[i].n_float = z.n_float, parts[i].tags = z.tags, parts[i].left_out = z.left_out;
        bytes += parts[i].text_len;
    }
    sp.harvest(0, bytes + n_parts * (int64_t)(sizeof(pcabi_auxparse_part) + sizeof(ParseSize)));
    return 0;
}

// k_auxparse_write over a planned table whose text lies in d->text already: the chains into the device
// output d_out[0, out_cap) (pre is what precedes it in d->out: guard bytes), then out[0, out_cap) and the
// fix-ups back, the floats filled. stage: where the device output is copied to (out_cap + 2 * pre bytes)
// when the caller checks guards, else nullptr and only out is filled. Synchronises.
int write_dev(AuxParseDev *d, hipStream_t st, const uint8_t *text, int64_t text_n, const pcabi_auxparse_part *parts, int64_t n_parts,
              uint8_t *out, int64_t out_cap, int64_t pre, uint8_t *stage) {
    if (n_parts <= 0) return 0;
    d->h_fix0.assign((size_t)n_parts + 1, 0);
    int64_t chain_bytes = 0, text_bytes = 0;
    for (int64_t i = 0; i < n_parts; ++i) {
        d->h_fix0[(size_t)i + 1] = d->h_fix0[(size_t)i] + (parts[i].len > 0 ? std::max(parts[i].n_float, 0) : 0);
        chain_bytes += std::max<int64_t>(parts[i].len, 0), text_bytes += parts[i].text_len;
    }
    const int64_t n_fix = d->h_fix0[(size_t)n_parts];
    if (int rc = d->parts.reserve(n_parts, grow(n_parts))) return rc;
    if (int rc = d->fix0.reserve(n_parts + 1, grow(n_parts + 1))) return rc;
    if (int rc = d->fix.reserve(std::max<int64_t>(n_fix, 1), grow(n_fix))) return rc;
    d->h_fix.assign((size_t)n_fix, Fix{-1, -1, 0, 0});
    PCABI_TRY(hipMemcpyAsync(d->parts, parts, (size_t)n_parts * sizeof(pcabi_auxparse_part), hipMemcpyHostToDevice, st));
    PCABI_TRY(hipMemcpyAsync(d->fix0, d->h_fix0.data(), (size_t)(n_parts + 1) * 8, hipMemcpyHostToDevice, st));
    if (n_fix > 0) PCABI_TRY(hipMemsetAsync(d->fix, 0xFF, (size_t)n_fix * sizeof(Fix), st));   // a slot nobody fills names no float
    Span sp;
    sp.begin(st);
    hipLaunchKernelGGL(k_auxparse_write, dim3((unsigned)n_parts), dim3(kWave), 0, st, d->text.p, text_n, d->parts.p, n_parts, d->fix0.p,
                       n_fix > 0 ? d->fix.p : nullptr, n_fix, d->out.p + pre, out_cap);
    PCABI_TRY(hipGetLastError());
    sp.end(st);
    if (stage) PCABI_TRY(hipMemcpyAsync(stage, d->out, (size_t)(out_cap + 2 * pre), hipMemcpyDeviceToHost, st));
    else if (out_cap > 0) PCABI_TRY(hipMemcpyAsync(out, d->out + pre, (size_t)out_cap, hipMemcpyDeviceToHost, st));
    if (n_fix > 0) PCABI_TRY(hipMemcpyAsync(d->h_fix.data(), d->fix, (size_t)n_fix * sizeof(Fix), hipMemcpyDeviceToHost, st));
    PCABI_TRY(hipStreamSynchronize(st));
    sp.harvest(1, text_bytes + chain_bytes + n_fix * (int64_t)sizeof(Fix) + n_parts * (int64_t)(sizeof(pcabi_auxparse_part) + 8));
    return fill_floats(text, text_n, d->h_fix.data(), n_fix, stage ? stage + pre : out, out_cap);
}

}  // namespace

AuxParseDev *pcabi_internal::auxparse_dev_new() { return new AuxParseDev; }
void pcabi_internal::auxparse_dev_free(AuxParseDev *d) {
    if (!d) return;
    if (d->device >= 0) (void)hipSetDevice(d->device);
    delete d;
}

int pcabi_internal::auxparse_headers(int device, AuxParseDev *d, const uint8_t *text, const int64_t *off, int64_t n,
                                     std::vector<uint8_t> *aux, std::vector<int64_t> *aux_off) {
    static const uint8_t kNone = 0;
    if (!text) text = &kNone;
    const int64_t text_n = n > 0 ? off[n] : 0;
    std::vector<pcabi_auxparse_part> parts((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        std::memset(&parts[(size_t)i], 0, sizeof(pcabi_auxparse_part));
        parts[(size_t)i].text_off = off[i], parts[(size_t)i].text_len = off[i + 1] - off[i];
    }
    if (int rc = check_parts(parts.data(), n, text_n)) return rc;
    hipStream_t st = nullptr;
    if (device >= 0) {
        if (!d) return fail(PCABI_E_ARG, "bad arguments");
        PCABI_TRY(hipSetDevice(device));
        if (d->device != device) {
            if (d->device >= 0) return fail(PCABI_E_ARG, "a reader parses its headers on one device");
            d->device = device;
            if (int rc = d->st.create()) return rc;
        }
        st = d->st;
        if (int rc = size_dev(d, st, text, text_n, parts.data(), n)) return rc;
    } else {
        plan_host(text, parts.data(), n);
    }
    count(parts.data(), n);
    aux_off->assign((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i) {
        parts[(size_t)i].out = (*aux_off)[(size_t)i];
        (*aux_off)[(size_t)i + 1] = (*aux_off)[(size_t)i] + parts[(size_t)i].len;
    }
    const int64_t out_n = (*aux_off)[(size_t)n];
    aux->assign((size_t)out_n, 0);
    if (out_n == 0) return 0;
    if (device < 0) {
        write_host(text, parts.data(), n, aux->data());
        return 0;
    }
    if (int rc = d->out.reserve(out_n + 64, grow(out_n + 64))) return rc;
    return write_dev(d, st, text, text_n, parts.data(), n, aux->data(), out_n, 0, nullptr);
}

extern "C" {

int pcabi_auxparse_plan(int device, const uint8_t *text, int64_t text_n, pcabi_auxparse_part *parts, int64_t n_parts) {
    if (text_n < 0 || n_parts < 0 || (text_n > 0 && !text) || (n_parts > 0 && !parts)) return fail(PCABI_E_ARG, "bad arguments");
    if (int rc = check_parts(parts, n_parts, text_n)) return rc;
    static const uint8_t kNone = 0;
    if (!text) text = &kNone;
    if (device < 0) {
        plan_host(text, parts, n_parts);
    } else {
        PCABI_TRY(hipSetDevice(device));
        AuxParseDev d;
        if (int rc = size_dev(&d, nullptr, text, text_n, parts, n_parts)) return rc;
    }
    count(parts, n_parts);
    return 0;
}

int pcabi_auxparse_write(int device, const uint8_t *text, int64_t text_n, const pcabi_auxparse_part *parts, int64_t n_parts,
                         uint8_t *out, int64_t out_cap) {
    if (text_n < 0 || n_parts < 0 || out_cap < 0 || (text_n > 0 && !text) || (n_parts > 0 && !parts) || (out_cap > 0 && !out))
        return fail(PCABI_E_ARG, "bad arguments");
    if (int rc = check_parts(parts, n_parts, text_n)) return rc;
    static const uint8_t kNone = 0;
    if (!text) text = &kNone;
    // the plan again, on the host: the caller's table must be its table, and no two ranges may meet
    std::vector<pcabi_auxparse_part> mine(parts, parts + n_parts);
    plan_host(text, mine.data(), n_parts);
    std::vector<std::pair<int64_t, int64_t>> spans;
    for (int64_t i = 0; i < n_parts; ++i) {
        const pcabi_auxparse_part &p = parts[i], &m = mine[(size_t)i];
        if (p.len != m.len) return fail(PCABI_E_ARG, "part " + std::to_string(i) + ": len is not the plan's");
        if (p.n_float != m.n_float || p.tags != m.tags || p.left_out != m.left_out)
            return fail(PCABI_E_ARG, "part " + std::to_string(i) + ": the counts are not the plan's");
        if (p.len > 0 && (p.out < 0 || p.len > out_cap - p.out)) return fail(PCABI_E_ARG, "part " + std::to_string(i) + " does not fit the output");
        if (p.len > 0) spans.emplace_back(p.out, p.out + p.len);
    }
    if (!spans_disjoint(spans)) return fail(PCABI_E_ARG, "two parts' outputs overlap");
    if (device < 0) {
        write_host(text, parts, n_parts, out);
        return 0;
    }
    if (n_parts >= INT32_MAX) return fail(PCABI_E_ARG, "too many parts for one launch");
    if (n_parts == 0) return 0;
    PCABI_TRY(hipSetDevice(device));
    AuxParseDev d;
    std::vector<uint8_t> stage((size_t)(out_cap + 2 * kGuard), 0xA5);
    if (out_cap > 0) std::memcpy(stage.data() + kGuard, out, (size_t)out_cap);
    if (int rc = d.text.reserve(text_n + 64, text_n + 64)) return rc;
    if (int rc = d.out.reserve((int64_t)stage.size(), (int64_t)stage.size())) return rc;
    if (text_n > 0) PCABI_TRY(hipMemcpy(d.text, text, (size_t)text_n, hipMemcpyHostToDevice));
    PCABI_TRY(hipMemcpy(d.out, stage.data(), stage.size(), hipMemcpyHostToDevice));
    const int rc = write_dev(&d, nullptr, text, text_n, parts, n_parts, nullptr, out_cap, kGuard, stage.data());
    for (int64_t g = 0; g < kGuard; ++g)
        if (stage[(size_t)(kGuard - 1 - g)] != 0xA5 || stage[(size_t)(kGuard + out_cap + g)] != 0xA5)
            return fail(PCABI_E_DEVICE, "k_auxparse_write wrote outside its output");
    if (rc) return rc;
    if (out_cap > 0) std::memcpy(out, stage.data() + kGuard, (size_t)out_cap);
    return 0;
}

void pcabi_auxparse_counts(int reset, int64_t *tags_read, int64_t *fields_left_out) {
    if (tags_read) *tags_read = g_tags.load();
    if (fields_left_out) *fields_left_out = g_left_out.load();
    if (reset) g_tags = 0, g_left_out = 0;
}

void pcabi_auxparse_last_times(int on, int reset, double *ms, int64_t *bytes) {
    g_times.last(on, reset, ms, bytes);
}

}  // extern "C"
