// pcabi_auxtext.hip -- the SAM text of aux chains and the text records that carry it, on the GPU
// (gfx950): include/pcabi.h pcabi_auxtext_*, pcabi_fastx_pack_*; DESIGN.md "Tags in text headers"; the
// rule and every per-lane function are csrc/pcabi_auxtext.h's, the same the host build runs.
//
// wave_walk: one wave walks one chain tag by tag, uniformly (every lane reads the same tag header).
//   A Z / H value goes 64 bytes a pass: zh_lane names what a lane saw, two ballots find the NUL and a
//   byte that is not printable; the copy is a byte a lane. An array goes 64 elements a pass: elem_len
//   gives a lane its element's characters (comparisons), a shuffle scan places them, elem_put stores the
//   lane's own digits as byte stores. Scalars are lane 0's. Floats come from the host's table of texts.
// k_auxtext_size: one wave per part, lengths and counts only (16 bytes a part go back).
// k_auxtext_write: one wave per part, the text into out[part.out, part.out + part.len).
// k_fastx_pack: one workgroup of 256 per tile of 16384 bases; a binary search of tile0 names the part.
//   The workgroup of a part's first tile writes '@' / '>', the name, the line feeds and '+' (pack_fixed)
//   and its first wave the tag text (wave_walk); every tile copies its bases and qualities in pieces of
//   the destination's 16-byte grid (pack_tile: an unaligned load, an aligned store; FASTA's line feeds
//   fall at p + p / 70).
// Every loop runs to a length the host passed; every offset from a table is checked against its buffer
// (part_fits, fastx_fits) and every store against the part's own length. No atomics, no inline assembly.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pcabi.h"
#include "pcabi_auxtext.h"
#include "pcabi_hostdev.h"

using namespace pcabi_internal;
using namespace pcabi_auxtext;

namespace {

constexpr int kWave = 64;
constexpr int kPackLanes = 256;
constexpr int64_t kGuard = 64;

// what k_auxtext_size leaves per part
struct AuxSize {
    int64_t len;
    int32_t written, left_out;
};

// the exclusive prefix of x over the wave; *total = the wave's sum
__device__ inline int wave_scan(int x, int lane, int *total) {
    int v = x;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int y = __shfl_up(v, d);
        if (lane >= d) v += y;
    }
    *total = __shfl(v, kWave - 1);
    return v - x;
}

// One wave over the chain a[0, n): the text's length or -1. kWrite: the text goes to dst[0, room) as well.
template <bool kWrite>
__device__ int64_t wave_walk(const uint8_t *a, int64_t n, Floats fl, uint8_t *dst, int64_t room, int lane, int *written, int *left_out) {
    int64_t at = 0, len = 0;
    int nw = 0, nl = 0;
    while (at < n) {   // uniform
        Tag t = tag_at(a, n, at);
        if (!t.ok) return -1;
        bool good = name_ok(a + at);
        int64_t vlen = 0;
        if (t.type == 'Z' || t.type == 'H') {
            int64_t end = -1;
            bool bad = false;
            for (int64_t q = t.val; q < n; q += kWave) {
                const int c = zh_lane(a, n, q + lane);
                const uint64_t nul = __ballot(c == 1), ugly = __ballot(c == 2);
                if (nul) {
                    const int f = __ffsll((long long)nul) - 1;
                    if (ugly & (((uint64_t)1 << f) - 1)) bad = true;
                    end = q + f;
                    break;
                }
                if (ugly) bad = true;
            }
            if (end < 0) return -1;
            good = good && !bad;
            vlen = end - t.val;
            t.next = end + 1;
        } else if (t.type == 'A') {
            good = good && printable(a[t.val]);
            vlen = 1;
        } else if (t.type == 'f') {
            uint8_t s[kFloatSlot];
            vlen = float_get(fl, 0, a + t.val, s);
        } else if (t.type != 'B') {
            vlen = dec_len(int_at(a + t.val, t.type));
        }
        uint8_t *d = kWrite ? dst + len + kHead : nullptr;
        const int64_t rm = kWrite ? room - len : 0, r = rm - kHead;
        if (kWrite && good) {
            if (lane < kHead && lane < rm) dst[len + lane] = head_byte(a + at, lane);
            if (t.type == 'Z' || t.type == 'H' || t.type == 'A') {
                for (int64_t k = lane; k < vlen && k < r; k += kWave) d[k] = a[t.val + k];
            } else if (t.type == 'f') {
                if (lane == 0) {
                    uint8_t s[kFloatSlot];
                    const int m = float_get(fl, 0, a + t.val, s);
                    for (int k = 0; k < m && k < r; ++k) d[k] = s[k];
                }
            } else if (t.type != 'B') {
                if (lane == 0) dec_put(d, r, int_at(a + t.val, t.type), (int)vlen);
            }
        }
        if (t.type == 'B') {
            if (kWrite && good && lane == 0 && r > 0) d[0] = t.sub;
            int64_t w = 1;
            if (good) {   // a tag that is left out needs no length
                for (int64_t k0 = 0; k0 < t.count; k0 += kWave) {
                    const int64_t k = k0 + lane;
                    const int el = k < t.count ? elem_len(a, t, k, fl) : 0;
                    int total = 0;
                    const int ex = wave_scan(el, lane, &total);
                    if (kWrite && k < t.count) elem_put(d + w + ex, r - w - ex, a, t, k, fl, el);
                    w += total;
                }
            }
            vlen = w;
        }
        if (t.type == 'f') fl.cur += 1;
        if (t.type == 'B' && t.sub == 'f') fl.cur += t.count;
        if (good) len += kHead + vlen, ++nw;
        else ++nl;
        at = t.next;
    }
    *written = nw, *left_out = nl;
    return len;
}

__device__ inline Floats floats_of(const uint8_t *ftext, const int64_t *fslot0, int64_t n_slots, int64_t pi) {
    // without a table every float reads as empty (float_slot): the host makes one whenever a chain holds a float
    return Floats{ftext, ftext ? n_slots : 0, ftext && fslot0 ? fslot0[pi] : 0};
}

__global__ __launch_bounds__(kWave) void k_auxtext_size(const uint8_t *__restrict__ aux, int64_t aux_n,
                                                        const pcabi_auxtext_part *__restrict__ parts, int64_t n_parts,
                                                        const uint8_t *__restrict__ ftext, const int64_t *__restrict__ fslot0,
                                                        int64_t n_slots, AuxSize *__restrict__ sizes) {
    const int64_t pi = blockIdx.x;
    if (pi >= n_parts) return;
    const int lane = threadIdx.x;
    const pcabi_auxtext_part p = parts[pi];
    int nw = 0, nl = 0;
    int64_t len = -1;
    if (part_fits(p, aux_n))   // uniform
        len = wave_walk<false>(aux + p.aux_off, p.aux_len, floats_of(ftext, fslot0, n_slots, pi), nullptr, 0, lane, &nw, &nl);
    if (len < 0) nw = nl = 0;
    if (lane == 0) sizes[pi] = AuxSize{len, nw, nl};
}

__global__ __launch_bounds__(kWave) void k_auxtext_write(const uint8_t *__restrict__ aux, int64_t aux_n,
                                                         const pcabi_auxtext_part *__restrict__ parts, int64_t n_parts,
                                                         const uint8_t *__restrict__ ftext, const int64_t *__restrict__ fslot0,
                                                         int64_t n_slots, uint8_t *__restrict__ out, int64_t out_cap) {
    const int64_t pi = blockIdx.x;
    if (pi >= n_parts) return;
    const int lane = threadIdx.x;
    const pcabi_auxtext_part p = parts[pi];
    if (!part_fits(p, aux_n) || p.len <= 0 || p.out < 0 || p.len > out_cap - p.out) return;   // uniform
    int nw = 0, nl = 0;
    wave_walk<true>(aux + p.aux_off, p.aux_len, floats_of(ftext, fslot0, n_slots, pi), out + p.out, p.len, lane, &nw, &nl);
}

__global__ __launch_bounds__(kPackLanes) void k_fastx_pack(const uint8_t *__restrict__ seq, int64_t seq_n,
                                                           const uint8_t *__restrict__ qual, int64_t qual_n,
                                                           const uint8_t *__restrict__ side, int64_t side_n,
                                                           const pcabi_fastx_part *__restrict__ parts, int64_t n_parts,
                                                           int64_t n_tiles, int fasta, const uint8_t *__restrict__ ftext,
                                                           const int64_t *__restrict__ fslot0, int64_t n_slots,
                                                           uint8_t *__restrict__ out, int64_t out_cap) {
    const int64_t tile = blockIdx.x;
    if (tile >= n_tiles || n_parts <= 0) return;
    int64_t lo = 0, hi = n_parts - 1;   // the last part whose tile0 <= tile
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (parts[mid].tile0 <= tile) lo = mid;
        else hi = mid - 1;
    }
    const pcabi_fastx_part p = parts[lo];
    if (!fastx_fits(p, fasta != 0, seq_n, qual_n, side_n, out_cap)) return;   // uniform
    const int64_t t0 = (tile - p.tile0) * kTileBases;
    if (t0 < 0 || t0 >= part_tiles(p) * kTileBases) return;
    uint8_t *rec = out + p.out;
    if (t0 == 0) {
        pack_fixed(p, fasta != 0, side, rec, threadIdx.x, kPackLanes);
        if (threadIdx.x < kWave && p.text_len > 0) {   // the first wave, whole
            int nw = 0, nl = 0;
            wave_walk<true>(side + p.aux_off, p.aux_len, floats_of(ftext, fslot0, n_slots, lo), rec + 1 + p.name_len, p.text_len,
                            (int)threadIdx.x, &nw, &nl);
        }
    }
    const int64_t t1 = t0 + kTileBases < p.l_seq ? t0 + kTileBases : (int64_t)p.l_seq;
    pack_tile(p, fasta != 0, seq, qual, rec, t0, t1, threadIdx.x, kPackLanes);
}

std::atomic<int64_t> g_written{0}, g_left_out{0};

// ---- device-event timing (tools/header_tags_timing.py) ----
KernelTimes g_times;
struct Span : EventSpan {
    void begin(hipStream_t st) { EventSpan::begin(g_times, st); }
    void harvest(int kind, int64_t bytes) { EventSpan::harvest(g_times, kind, bytes); }
};

// The floats' texts of the chains aux[off[i], off[i] + len[i]) (the host prints them): slot0[i] = part i's
// first slot. Chains that do not walk get none.
template <class Off, class Len>
void float_table(const uint8_t *aux, int64_t n_parts, Off off, Len len, std::vector<uint8_t> *ftext, std::vector<int64_t> *slot0) {
    slot0->assign((size_t)n_parts + 1, 0);
    for (int64_t i = 0; i < n_parts; ++i) {
        (*slot0)[(size_t)i] = (int64_t)ftext->size() / kFloatSlot;
        const int64_t n = len(i);
        // (the walk reads the tags' heads and the strings, and steps over the arrays: a move table costs nothing)
        if (n > 0 && float_count(aux + off(i), n) > 0) float_fill(aux + off(i), n, ftext);
    }
    (*slot0)[(size_t)n_parts] = (int64_t)ftext->size() / kFloatSlot;
}

int check_parts(const pcabi_auxtext_part *parts, int64_t n_parts, int64_t aux_n) {
    for (int64_t i = 0; i < n_parts; ++i)
        if (!part_fits(parts[i], aux_n)) return fail(PCABI_E_ARG, "part " + std::to_string(i) + " does not lie inside the aux bytes");
    return 0;
}

// the host build of the plan: lengths and counts, the parts dealt to the io threads in ranges
void plan_host(const uint8_t *aux, pcabi_auxtext_part *parts, int64_t n_parts) {
    const int nt = (int)std::min<int64_t>(io_thread_count(), std::max<int64_t>(1, n_parts / 256));
    std::vector<int64_t> nw((size_t)nt, 0), nl((size_t)nt, 0);
    auto work = [&](int t) {
        for (int64_t i = n_parts * t / nt; i < n_parts * (t + 1) / nt; ++i)
            parts[i].len = walk(aux + parts[i].aux_off, parts[i].aux_len, Floats{nullptr, 0, 0}, nullptr, 0, &nw[(size_t)t], &nl[(size_t)t]);
    };
    if (nt <= 1) {
        work(0);
    } else {
        std::vector<std::thread> th;
        for (int t = 0; t < nt; ++t) th.emplace_back(work, t);
        for (auto &x : th) x.join();
    }
    for (int t = 0; t < nt; ++t) g_written += nw[(size_t)t], g_left_out += nl[(size_t)t];
}

// The device side of a sizing pass: what is uploaded stays for the writing pass.
struct AuxDev {
    DevBuf<> aux, ftext;
    DevBuf<pcabi_auxtext_part> parts;
    DevBuf<int64_t> slot0;
    DevBuf<AuxSize> sizes;
    std::vector<uint8_t> h_ftext;
    std::vector<int64_t> h_slot0;
    std::vector<AuxSize> h_sizes;
    int64_t n_slots = 0;
};

// the float table up (null pointers when no chain holds a float)
int floats_up(AuxDev *d, hipStream_t st, int64_t n_parts) {
    d->n_slots = (int64_t)d->h_ftext.size() / kFloatSlot;
    if (d->n_slots == 0) return 0;
    if (int rc = d->ftext.reserve((int64_t)d->h_ftext.size(), (int64_t)d->h_ftext.size() + 4096)) return rc;
    if (int rc = d->slot0.reserve(n_parts + 1, n_parts + n_parts / 4 + 64)) return rc;
    PCABI_TRY(hipMemcpyAsync(d->ftext, d->h_ftext.data(), d->h_ftext.size(), hipMemcpyHostToDevice, st));
    PCABI_TRY(hipMemcpyAsync(d->slot0, d->h_slot0.data(), (size_t)(n_parts + 1) * 8, hipMemcpyHostToDevice, st));
    return 0;
}

// k_auxtext_size over a table whose chains lie in d_aux (device); the sizes come back to d->h_sizes. Synchronises.
int size_dev(AuxDev *d, hipStream_t st, const uint8_t *d_aux, int64_t aux_n, const pcabi_auxtext_part *parts, int64_t n_parts, Span *sp) {
    if (n_parts >= INT32_MAX) return fail(PCABI_E_ARG, "too many parts for one launch");
    d->h_sizes.assign((size_t)n_parts, AuxSize{-1, 0, 0});
    if (n_parts <= 0) return 0;
    if (int rc = d->parts.reserve(n_parts, n_parts + n_parts / 4 + 64)) return rc;
    if (int rc = d->sizes.reserve(n_parts, n_parts + n_parts / 4 + 64)) return rc;
    if (int rc = floats_up(d, st, n_parts)) return rc;
    PCABI_TRY(hipMemcpyAsync(d->parts, parts, (size_t)n_parts * sizeof(pcabi_auxtext_part), hipMemcpyHostToDevice, st));
    if (sp) sp->begin(st);
    hipLaunchKernelGGL(k_auxtext_size, dim3((unsigned)n_parts), dim3(kWave), 0, st, d_aux, aux_n, d->parts.p, n_parts,
                       d->n_slots ? d->ftext.p : nullptr, d->n_slots ? d->slot0.p : nullptr, d->n_slots, d->sizes.p);
    PCABI_TRY(hipGetLastError());
    if (sp) sp->end(st);
    PCABI_TRY(hipMemcpyAsync(d->h_sizes.data(), d->sizes, (size_t)n_parts * sizeof(AuxSize), hipMemcpyDeviceToHost, st));
    PCABI_TRY(hipStreamSynchronize(st));
    return 0;
}

int launch_pack(hipStream_t st, const uint8_t *seq, int64_t seq_n, const uint8_t *qual, int64_t qual_n, const uint8_t *side,
                int64_t side_n, const pcabi_fastx_part *parts, int64_t n_parts, int64_t n_tiles, int fasta, const uint8_t *ftext,
                const int64_t *fslot0, int64_t n_slots, uint8_t *out, int64_t out_cap) {
    if (n_tiles < 0 || n_tiles >= INT32_MAX) return fail(PCABI_E_ARG, "too many tiles for one launch");
    if (n_parts <= 0 || n_tiles == 0) return 0;
    hipLaunchKernelGGL(k_fastx_pack, dim3((unsigned)n_tiles), dim3(kPackLanes), 0, st, seq, seq_n, qual, qual_n, side, side_n, parts,
                       n_parts, n_tiles, fasta, ftext, fslot0, n_slots, out, out_cap);
    PCABI_TRY(hipGetLastError());
    return 0;
}

// The writer's block list from line lengths alone: pcabi_deflate::plan_blocks' rules (a line counts with
// its '\n'; a line of long_line bytes or more ends a block, with the short lines pending before it, cut
// evenly when that is more than cap; short lines accumulate up to cap).
struct LinePlanner {
    int64_t long_line, cap, bs = 0, p = 0;
    std::vector<int64_t> *off;
    void line(int64_t len) {
        const int64_t e = p + len;
        if (len >= long_line) {
            const int64_t span = e - bs, k = (span + cap - 1) / cap;
            for (int64_t j = 1; j <= k; ++j) off->push_back(bs + span * j / k);
            bs = e;
        } else if (e - bs > cap) {
            off->push_back(p);
            bs = p;
        }
        p = e;
    }
    void end() {
        if (bs < p) off->push_back(p);
    }
};

// the device side of the text writer, kept between calls (one device at a time, one call at a time);
// never destroyed: a destructor at exit would call into a HIP runtime that may already have shut down
struct WriteDev {
    int device = -1;
    DevBuf<> seq, qual, side, text, z, scratch;
    DevBuf<pcabi_fastx_part> parts;
    DevBuf<int64_t> block_off, d_len;
    PinBuf<> p_z;
    Stream st;
    AuxDev aux;
    RemapDev remap;
};
WriteDev &g_wd = *new WriteDev;
std::mutex g_wd_mu;

}  // namespace

int64_t pcabi_internal::fastx_write_tags_dev(int device, const uint8_t *seq, int64_t seq_n, const uint8_t *qual, int64_t qual_n,
                                             const ModsTables *mods, const MovesTables *moves, bool fasta, bool bgzf,
                                             const std::function<void(FastxWriteJob *)> &layout,
                                             const std::function<void(const uint8_t *, int64_t)> &sink) {
    std::lock_guard<std::mutex> lk(g_wd_mu);
    if (device < 0) PCABI_TRY(hipGetDevice(&device));
    if (g_wd.device >= 0 && g_wd.device != device) {
        (void)hipSetDevice(g_wd.device);
        g_wd.st.release();
        g_wd.remap.release();
        g_wd = WriteDev();
    }
    PCABI_TRY(hipSetDevice(device));
    g_wd.device = device;
    if (!g_wd.st)
        if (int rc = g_wd.st.create()) return rc;
    hipStream_t st = g_wd.st;
    auto grow = [](int64_t n) { return std::max<int64_t>(n + n / 4, 1 << 20); };
    if (int rc = g_wd.d_len.reserve(8, 8)) return rc;
    // steps 1, 2: the letters up, the remapped tags sized in one round trip (as the BAM writer does)
    if (int rc = g_wd.seq.reserve(seq_n + 64, grow(seq_n + 64))) return rc;
    if (seq_n > 0) PCABI_TRY(hipMemcpyAsync(g_wd.seq, seq, (size_t)seq_n, hipMemcpyHostToDevice, st));
    if (int rc = g_wd.remap.plan(device, st, seq, g_wd.seq, seq_n, mods, moves)) return rc;
    // step 3: the side blob with its gaps, the parts
    FastxWriteJob job;
    layout(&job);
    const int64_t n_parts = job.n_parts, side_n = job.side_n;
    if (n_parts <= 0) return 0;
    for (int64_t i = 0; i < n_parts; ++i) {
        const pcabi_fastx_part &p = job.parts[i];
        if (p.aux_off < 0 || p.aux_len < 0 || p.aux_off > side_n || p.aux_len > side_n - p.aux_off || job.kept[i] < 0 ||
            job.kept[i] > p.aux_len)
            return fail(PCABI_E_ARG, "a part's tags do not lie inside the side blob");
    }
    // the floats of the kept tags (the gaps hold MM ML MN mv ts: no float)
    AuxDev &ad = g_wd.aux;
    ad.h_ftext.clear();
    float_table(job.side, n_parts, [&](int64_t i) { return job.parts[i].aux_off; }, [&](int64_t i) { return (int64_t)job.kept[i]; },
                &ad.h_ftext, &ad.h_slot0);
    // step 4: the blob up, the remap kernels fill its gaps
    if (int rc = g_wd.side.reserve(side_n + 64, grow(side_n + 64))) return rc;
    if (int rc = g_wd.qual.reserve(qual_n + 64, grow(qual_n + 64))) return rc;
    if (side_n > 0) PCABI_TRY(hipMemcpyAsync(g_wd.side, job.side, (size_t)side_n, hipMemcpyHostToDevice, st));
    if (qual_n > 0 && !fasta) PCABI_TRY(hipMemcpyAsync(g_wd.qual, qual, (size_t)qual_n, hipMemcpyHostToDevice, st));
    if (int rc = g_wd.remap.write(st, mods, moves, g_wd.side, side_n)) return rc;
    // step 5: every part's text length
    std::vector<pcabi_auxtext_part> ap((size_t)n_parts);
    for (int64_t i = 0; i < n_parts; ++i) ap[(size_t)i] = pcabi_auxtext_part{job.parts[i].aux_off, 0, 0, job.parts[i].aux_len, 0};
    Span sp_size, sp_pack;
    if (int rc = size_dev(&ad, st, g_wd.side, side_n, ap.data(), n_parts, &sp_size)) return rc;
    // step 6: the records' offsets and the deflate blocks, from the line lengths
    FastxLayout lay;
    lay.fasta = fasta;
    std::vector<int64_t> block_off{0};
    LinePlanner lp{PCABI_GZIP_LONG_LINE, bgzf ? (int64_t)PCABI_BGZF_BLOCK_CAP : (int64_t)PCABI_GZIP_BLOCK_CAP, 0, 0, &block_off};
    int64_t nw = 0, nl = 0, aux_bytes = 0, text_bytes = 0;
    for (int64_t i = 0; i < n_parts; ++i) {
        pcabi_fastx_part &p = job.parts[i];
        const AuxSize &z = ad.h_sizes[(size_t)i];
        p.text_len = z.len > 0 ? z.len : 0;
        nw += z.written, nl += z.left_out;
        aux_bytes += p.aux_len, text_bytes += p.text_len;
        lay.place(&p);
        lp.line(head_len(p));
        if (fasta) {
            for (int64_t k = 0; k < p.l_seq; k += kFastaLine) lp.line(std::min<int64_t>(kFastaLine, p.l_seq - k) + 1);
        } else {
            lp.line((int64_t)p.l_seq + 1);
            lp.line(2);
            lp.line((int64_t)p.l_qual + 1);
        }
    }
    lp.end();
    g_written += nw, g_left_out += nl;
    const int64_t text_n = lay.out, nb = (int64_t)block_off.size() - 1;
    // steps 7, 8: the text laid out, then compressed where it lies
    const int64_t z_cap = bgzf ? pcabi_bgzf_bound(text_n, std::max<int64_t>(nb, 1), 0) : pcabi_gzip_bound(text_n, std::max<int64_t>(nb, 1));
    const int64_t sc = pcabi_gzip_scratch_bytes(text_n, std::max<int64_t>(nb, 1));
    if (z_cap < 0 || sc < 0) return z_cap < 0 ? z_cap : sc;
    if (int rc = g_wd.parts.reserve(n_parts, n_parts + n_parts / 4 + 64)) return rc;
    if (int rc = g_wd.text.reserve(text_n + 64, grow(text_n + 64))) return rc;
    if (int rc = g_wd.z.reserve(z_cap + 64, grow(z_cap + 64))) return rc;
    if (int rc = g_wd.scratch.reserve(sc, sc + sc / 4)) return rc;
    if (int rc = g_wd.block_off.reserve(nb + 1, nb + nb / 4 + 64)) return rc;
    PCABI_TRY(hipMemcpyAsync(g_wd.parts, job.parts, (size_t)n_parts * sizeof(pcabi_fastx_part), hipMemcpyHostToDevice, st));
    PCABI_TRY(hipMemcpyAsync(g_wd.block_off, block_off.data(), (size_t)(nb + 1) * 8, hipMemcpyHostToDevice, st));
    sp_pack.begin(st);
    if (int rc = launch_pack(st, g_wd.seq, seq_n, g_wd.qual, fasta ? 0 : qual_n, g_wd.side, side_n, g_wd.parts, n_parts, lay.tiles, fasta,
                             ad.n_slots ? ad.ftext.p : nullptr, ad.n_slots ? ad.slot0.p : nullptr, ad.n_slots, g_wd.text, text_n))
        return rc;
    sp_pack.end(st);
    if (bgzf) {
        if (int rc = bgzf_dev_blocks(st, g_wd.text, text_n, g_wd.block_off, nb, g_wd.z, z_cap, g_wd.d_len, g_wd.scratch, g_wd.scratch.cap))
            return rc;
    } else {
        if (int rc = pcabi_gzip_dev(st, g_wd.text, text_n, g_wd.block_off, nb, g_wd.z, z_cap, g_wd.d_len, g_wd.scratch, g_wd.scratch.cap))
            return rc;
    }
    int64_t zn = 0;
    PCABI_TRY(hipMemcpyAsync(&zn, g_wd.d_len, 8, hipMemcpyDeviceToHost, st));
    PCABI_TRY(hipStreamSynchronize(st));
    int64_t seq_bytes = 0;
    for (int64_t i = 0; i < n_parts; ++i) seq_bytes += (int64_t)job.parts[i].l_seq + (fasta ? 0 : job.parts[i].l_qual);
    sp_size.harvest(0, aux_bytes + n_parts * (int64_t)(sizeof(pcabi_auxtext_part) + sizeof(AuxSize)));
    sp_pack.harvest(1, aux_bytes + seq_bytes + text_n + n_parts * (int64_t)sizeof(pcabi_fastx_part));
    if (zn < 0 || zn > z_cap) return fail(PCABI_E_DEVICE, "the encoder refused the text");
    if (int rc = g_wd.p_z.reserve(zn, grow(zn))) return rc;
    if (zn > 0) PCABI_TRY(hipMemcpyAsync(g_wd.p_z, g_wd.z, (size_t)zn, hipMemcpyDeviceToHost, st));
    PCABI_TRY(hipStreamSynchronize(st));
    sink(g_wd.p_z, zn);
    return zn;
}

extern "C" {

int pcabi_auxtext_plan(int device, const uint8_t *aux, int64_t aux_n, pcabi_auxtext_part *parts, int64_t n_parts) {
    if (aux_n < 0 || n_parts < 0 || (aux_n > 0 && !aux) || (n_parts > 0 && !parts)) return fail(PCABI_E_ARG, "bad arguments");
    if (int rc = check_parts(parts, n_parts, aux_n)) return rc;
    static const uint8_t kNone = 0;
    if (!aux) aux = &kNone;
    if (device < 0) {
        plan_host(aux, parts, n_parts);
        return 0;
    }
    PCABI_TRY(hipSetDevice(device));
    AuxDev d;
    float_table(aux, n_parts, [&](int64_t i) { return parts[i].aux_off; }, [&](int64_t i) { return (int64_t)parts[i].aux_len; },
                &d.h_ftext, &d.h_slot0);
    if (int rc = d.aux.reserve(aux_n + 64, aux_n + 64)) return rc;
    if (aux_n > 0) PCABI_TRY(hipMemcpy(d.aux, aux, (size_t)aux_n, hipMemcpyHostToDevice));
    if (int rc = size_dev(&d, nullptr, d.aux, aux_n, parts, n_parts, nullptr)) return rc;
    int64_t nw = 0, nl = 0;
    for (int64_t i = 0; i < n_parts; ++i) {
        parts[i].len = d.h_sizes[(size_t)i].len;
        nw += d.h_sizes[(size_t)i].written, nl += d.h_sizes[(size_t)i].left_out;
    }
    g_written += nw, g_left_out += nl;
    return 0;
}

int pcabi_auxtext_write(int device, const uint8_t *aux, int64_t aux_n, const pcabi_auxtext_part *parts, int64_t n_parts,
                        uint8_t *out, int64_t out_cap) {
    if (aux_n < 0 || n_parts < 0 || out_cap < 0 || (aux_n > 0 && !aux) || (n_parts > 0 && !parts) || (out_cap > 0 && !out))
        return fail(PCABI_E_ARG, "bad arguments");
    if (int rc = check_parts(parts, n_parts, aux_n)) return rc;
    static const uint8_t kNone = 0;
    if (!aux) aux = &kNone;
    // the plan again, on the host: the caller's lengths must be its lengths, and no two ranges may meet
    std::vector<std::pair<int64_t, int64_t>> spans;
    for (int64_t i = 0; i < n_parts; ++i) {
        const pcabi_auxtext_part &p = parts[i];
        if (walk(aux + p.aux_off, p.aux_len, Floats{nullptr, 0, 0}, nullptr, 0, nullptr, nullptr) != p.len)
            return fail(PCABI_E_ARG, "part " + std::to_string(i) + ": len is not the plan's");
        if (p.len > 0 && (p.out < 0 || p.len > out_cap - p.out)) return fail(PCABI_E_ARG, "part " + std::to_string(i) + " does not fit the output");
        if (p.len > 0) spans.emplace_back(p.out, p.out + p.len);
    }
    if (!spans_disjoint(spans)) return fail(PCABI_E_ARG, "two parts' outputs overlap");
    if (device < 0) {
        for (int64_t i = 0; i < n_parts; ++i)
            if (parts[i].len > 0)
                walk(aux + parts[i].aux_off, parts[i].aux_len, Floats{nullptr, 0, 0}, out + parts[i].out, parts[i].len, nullptr, nullptr);
        return 0;
    }
    if (n_parts >= INT32_MAX) return fail(PCABI_E_ARG, "too many parts for one launch");
    PCABI_TRY(hipSetDevice(device));
    AuxDev d;
    float_table(aux, n_parts, [&](int64_t i) { return parts[i].aux_off; }, [&](int64_t i) { return (int64_t)parts[i].aux_len; },
                &d.h_ftext, &d.h_slot0);
    std::vector<uint8_t> stage((size_t)(out_cap + 2 * kGuard), 0xA5);
    if (out_cap > 0) std::memcpy(stage.data() + kGuard, out, (size_t)out_cap);
    DevBuf<> d_out;
    if (int rc = d_out.reserve((int64_t)stage.size(), (int64_t)stage.size())) return rc;
    if (int rc = d.aux.reserve(aux_n + 64, aux_n + 64)) return rc;
    if (int rc = d.parts.reserve(n_parts + 1, n_parts + 1)) return rc;
    PCABI_TRY(hipMemcpy(d_out, stage.data(), stage.size(), hipMemcpyHostToDevice));
    if (aux_n > 0) PCABI_TRY(hipMemcpy(d.aux, aux, (size_t)aux_n, hipMemcpyHostToDevice));
    if (n_parts > 0) PCABI_TRY(hipMemcpy(d.parts, parts, (size_t)n_parts * sizeof(pcabi_auxtext_part), hipMemcpyHostToDevice));
    if (int rc = floats_up(&d, nullptr, n_parts)) return rc;
    if (n_parts > 0) {
        hipLaunchKernelGGL(k_auxtext_write, dim3((unsigned)n_parts), dim3(kWave), 0, nullptr, d.aux.p, aux_n, d.parts.p, n_parts,
                           d.n_slots ? d.ftext.p : nullptr, d.n_slots ? d.slot0.p : nullptr, d.n_slots, d_out + kGuard, out_cap);
        PCABI_TRY(hipGetLastError());
    }
    PCABI_TRY(hipStreamSynchronize(nullptr));
    PCABI_TRY(hipMemcpy(stage.data(), d_out, stage.size(), hipMemcpyDeviceToHost));
    for (int64_t g = 0; g < kGuard; ++g)
        if (stage[(size_t)(kGuard - 1 - g)] != 0xA5 || stage[(size_t)(kGuard + out_cap + g)] != 0xA5)
            return fail(PCABI_E_DEVICE, "k_auxtext_write wrote outside its output");
    if (out_cap > 0) std::memcpy(out, stage.data() + kGuard, (size_t)out_cap);
    return 0;
}

void pcabi_auxtext_counts(int reset, int64_t *tags_written, int64_t *tags_left_out) {
    if (tags_written) *tags_written = g_written.load();
    if (tags_left_out) *tags_left_out = g_left_out.load();
    if (reset) g_written = 0, g_left_out = 0;
}

void pcabi_auxtext_last_times(int on, int reset, double *ms, int64_t *bytes) {
    g_times.last(on, reset, ms, bytes);
}

int64_t pcabi_fastx_pack_plan(pcabi_fastx_part *parts, int64_t n_parts, int fasta, int64_t out0, int64_t *tiles) {
    if (n_parts < 0 || out0 < 0 || (n_parts > 0 && !parts)) return fail(PCABI_E_ARG, "bad arguments");
    FastxLayout lay;
    lay.out = out0, lay.fasta = fasta != 0;
    for (int64_t i = 0; i < n_parts; ++i) {
        if (parts[i].l_seq < 0 || parts[i].l_qual < 0 || parts[i].name_len < 0 || parts[i].text_len < -1)
            return fail(PCABI_E_ARG, "part " + std::to_string(i) + ": negative length");
        lay.place(&parts[i]);
    }
    if (tiles) *tiles = lay.tiles;
    return lay.out;
}

int pcabi_fastx_pack_dev(void *stream, const uint8_t *seq, int64_t seq_n, const uint8_t *qual, int64_t qual_n, const uint8_t *side,
                         int64_t side_n, const pcabi_fastx_part *parts, int64_t n_parts, int64_t n_tiles, int fasta, const uint8_t *ftext,
                         const int64_t *fslot0, int64_t n_slots, uint8_t *out, int64_t out_cap) {
    if (seq_n < 0 || qual_n < 0 || side_n < 0 || n_parts < 0 || out_cap < 0 || n_slots < 0 || (n_parts > 0 && !parts) ||
        (out_cap > 0 && !out) || (n_slots > 0 && (!ftext || !fslot0)))
        return fail(PCABI_E_ARG, "bad arguments");
    return launch_pack((hipStream_t)stream, seq, seq_n, qual, qual_n, side, side_n, parts, n_parts, n_tiles, fasta, n_slots ? ftext : nullptr,
                       n_slots ? fslot0 : nullptr, n_slots, out, out_cap);
}

int pcabi_fastx_pack_host(int device, const uint8_t *seq, int64_t seq_n, const uint8_t *qual, int64_t qual_n, const uint8_t *side,
                          int64_t side_n, const pcabi_fastx_part *parts, int64_t n_parts, int fasta, uint8_t *out, int64_t out_cap) {
    if (seq_n < 0 || qual_n < 0 || side_n < 0 || n_parts < 0 || out_cap < 0 || (seq_n > 0 && !seq) || (qual_n > 0 && !qual) ||
        (side_n > 0 && !side) || (n_parts > 0 && !parts) || (out_cap > 0 && !out))
        return fail(PCABI_E_ARG, "bad arguments");
    static const uint8_t kNone = 0;
    if (!side) side = &kNone;
    const bool fa = fasta != 0;
    // the table against the buffers, the plan and the text lengths
    int64_t tiles = 0;
    std::vector<std::pair<int64_t, int64_t>> spans;
    for (int64_t i = 0; i < n_parts; ++i) {
        const pcabi_fastx_part &p = parts[i];
        if (!fastx_fits(p, fa, seq_n, qual_n, side_n, out_cap))
            return fail(PCABI_E_ARG, "part " + std::to_string(i) + " does not lie inside the buffers");
        if (p.tile0 != tiles) return fail(PCABI_E_ARG, "part " + std::to_string(i) + " was not planned");
        const int64_t len = walk(side + p.aux_off, p.aux_len, Floats{nullptr, 0, 0}, nullptr, 0, nullptr, nullptr);
        if (text_len_of(p) != (len > 0 ? len : 0)) return fail(PCABI_E_ARG, "part " + std::to_string(i) + ": text_len is not the plan's");
        tiles += part_tiles(p);
        spans.emplace_back(p.out, p.out + record_len(p, fa));
    }
    if (!spans_disjoint(spans)) return fail(PCABI_E_ARG, "two parts' records overlap");
    if (device < 0) {
        for (int64_t i = 0; i < n_parts; ++i) pack_part(parts[i], fa, seq, qual, side, out);
        return 0;
    }
    PCABI_TRY(hipSetDevice(device));
    AuxDev d;
    float_table(side, n_parts, [&](int64_t i) { return parts[i].aux_off; }, [&](int64_t i) { return (int64_t)parts[i].aux_len; },
                &d.h_ftext, &d.h_slot0);
    // the output as far off a 16-byte boundary as the caller's pointer, between guard bytes
    const int64_t skew = (int64_t)((uintptr_t)out & 15u);
    std::vector<uint8_t> stage((size_t)(out_cap + 2 * kGuard + 16), 0xA5);
    if (out_cap > 0) std::memcpy(stage.data() + kGuard + skew, out, (size_t)out_cap);
    DevBuf<> d_seq, d_qual, d_side, d_out;
    DevBuf<pcabi_fastx_part> d_parts;
    if (int rc = d_seq.reserve(seq_n + 64, seq_n + 64)) return rc;
    if (int rc = d_qual.reserve(qual_n + 64, qual_n + 64)) return rc;
    if (int rc = d_side.reserve(side_n + 64, side_n + 64)) return rc;
    if (int rc = d_parts.reserve(n_parts + 1, n_parts + 1)) return rc;
    if (int rc = d_out.reserve((int64_t)stage.size(), (int64_t)stage.size())) return rc;
    if (seq_n > 0) PCABI_TRY(hipMemcpy(d_seq, seq, (size_t)seq_n, hipMemcpyHostToDevice));
    if (qual_n > 0) PCABI_TRY(hipMemcpy(d_qual, qual, (size_t)qual_n, hipMemcpyHostToDevice));
    if (side_n > 0) PCABI_TRY(hipMemcpy(d_side, side, (size_t)side_n, hipMemcpyHostToDevice));
    if (n_parts > 0) PCABI_TRY(hipMemcpy(d_parts, parts, (size_t)n_parts * sizeof(pcabi_fastx_part), hipMemcpyHostToDevice));
    PCABI_TRY(hipMemcpy(d_out, stage.data(), stage.size(), hipMemcpyHostToDevice));
    if (int rc = floats_up(&d, nullptr, n_parts)) return rc;
    if (int rc = launch_pack(nullptr, d_seq, seq_n, d_qual, qual_n, d_side, side_n, d_parts, n_parts, tiles, fasta,
                             d.n_slots ? d.ftext.p : nullptr, d.n_slots ? d.slot0.p : nullptr, d.n_slots, d_out + kGuard + skew, out_cap))
        return rc;
    PCABI_TRY(hipStreamSynchronize(nullptr));
    PCABI_TRY(hipMemcpy(stage.data(), d_out, stage.size(), hipMemcpyDeviceToHost));
    for (int64_t g = 0; g < kGuard; ++g)
        if (stage[(size_t)(kGuard + skew - 1 - g)] != 0xA5 || stage[(size_t)(kGuard + skew + out_cap + g)] != 0xA5)
            return fail(PCABI_E_DEVICE, "k_fastx_pack wrote outside its output");
    if (out_cap > 0) std::memcpy(out, stage.data() + kGuard + skew, (size_t)out_cap);
    return 0;
}

}  // extern "C"
