// pcabi_mods.hip -- base-modification tags (MM / ML / MN) remapped onto parts of reads on the GPU
// (gfx950): include/pcabi.h pcabi_mods_*; DESIGN.md "BAM output"; the rule and every per-byte, per-group
// function are csrc/pcabi_mods.h's, the same the host build runs.
//
// k_mods_plan: one wave (a workgroup of 64 lanes) per read.
//   1. Counting. The read's letters go by 64 a pass, one a lane; four ballots give the masks of A, C, G
//      and T, their popcounts the running counts. A lane keeps one part boundary in a register (a read
//      of more than 32 parts: the lanes stride over them in memory); a boundary inside the pass takes
//      running count + popcount(mask below it). Counts at a boundary go
//      to cnt[part][side][4]; the running counts end as the read's totals.
//   2. Parsing. The MM text goes by 64 bytes a pass. Ballots of ';' and ',' give every byte the start
//      of its group and whether a ',' came since (the last set bit below the lane, or the state
//      carried from the pass before), which is all byte_ok() needs. The lane on a number's last digit
//      reads the number backwards from memory (count_at: a number may straddle passes), a wave-wide
//      inclusive scan of count + 1 minus its value at the group's ';' gives the ordinal, and a
//      popcount of the number-end mask the entry's index. Entries (ordinal, text offset) go to the
//      read's slice of a scratch table, group records to the read's 32 slots.
//   3. Lane 0 runs the usability checks (finish_groups); then, for each part, lane g takes group g:
//      two binary searches over the group's ordinals give the kept run, and the lanes' byte counts add
//      up to the part's length (lens[part]: 4 bytes a part is all that goes back to the host).
// k_mods_write: one wave per part. Lane g repeats the two searches of group g; a wave-wide scan places
// the groups; then the lanes stride over the bytes of each group in turn (emit_group) and over the
// fixed bytes (emit_fixed). It writes out[part.out, part.out + part.len) only, and only when the length
// it computes is the part's len.
// Every loop runs to a length the host passed (l_seq, mm_len, n_parts, 32 groups); count_at walks back
// over digits no further than the text's start. No atomics, no inline assembly.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/pcabi.h"
#include "pcabi_hostdev.h"
#include "pcabi_mods.h"

using namespace pcabi_internal;
using namespace pcabi_mods;

namespace {

constexpr int kWave = 64;

__device__ inline int64_t wave_scan(int64_t x, int lane) {   // inclusive
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const long long y = __shfl_up((long long)x, d);
        if (lane >= d) x += y;
    }
    return x;
}
__device__ inline int64_t wave_sum(int64_t x) {
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) x += __shfl_xor((long long)x, d);
    return x;
}

// a part's boundaries inside its read
PCABI_HD inline void part_bounds(const pcabi_mods_part &p, int64_t l_seq, int64_t *b0, int64_t *b1) {
    int64_t a = p.s0, e = (int64_t)p.s0 + p.ns;
    a = a < 0 ? 0 : a > l_seq ? l_seq : a;
    e = e < a ? a : e > l_seq ? l_seq : e;
    *b0 = a, *b1 = e;
}

__global__ __launch_bounds__(kWave) void k_mods_plan(const uint8_t *__restrict__ seq, int64_t seq_n,
                                                     const uint8_t *__restrict__ tags, int64_t tags_n,
                                                     const pcabi_mods_read *__restrict__ reads, int64_t n_reads,
                                                     const pcabi_mods_part *__restrict__ parts, int64_t n_parts,
                                                     const int64_t *__restrict__ ent_off, Ent *__restrict__ ents, int64_t n_ents,
                                                     Group *__restrict__ groups, int32_t *__restrict__ cnt,
                                                     int32_t *__restrict__ info, int32_t *__restrict__ lens) {
    __shared__ int s_usable;
    const int64_t ri = blockIdx.x;
    if (ri >= n_reads) return;
    const int lane = threadIdx.x;
    const pcabi_mods_read r = reads[ri];
    const int64_t e_at = ent_off[ri], e_cap = ent_off[ri + 1] - e_at;
    if (!read_fits(r, seq_n, tags_n, n_parts) || e_at < 0 || e_cap < 0 || e_cap > n_ents - e_at) {   // uniform
        if (lane == 0) info[ri] = -1;
        return;
    }
    Group *grp = groups + ri * kMaxGroups;
    Ent *ent = ents + e_at;

    // 1. counts of A C G T before every part boundary, and in the whole read
    int32_t run[4] = {0, 0, 0, 0};
    {
        const uint8_t *s = seq + r.seq_off;
        const int64_t nb = 2 * (int64_t)r.n_parts;
        auto edge = [&](int64_t j) {   // boundary j of the read: part j / 2, its start or its end
            int64_t b0, b1;
            part_bounds(parts[r.part0 + (j >> 1)], r.l_seq, &b0, &b1);
            return (j & 1) ? b1 : b0;
        };
        // up to 32 parts: a lane keeps its one boundary in a register; more: the lanes stride over them
        const bool few = nb <= kWave;
        const int64_t mine = few && lane < nb ? edge(lane) : -1;
        for (int64_t pos = 0; pos <= r.l_seq; pos += kWave) {
            const int cls = pos + lane < r.l_seq ? letter_class(s[pos + lane]) : 5;
            uint64_t m[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) m[k] = __ballot(cls == k);
            for (int64_t j0 = 0; j0 < nb; j0 += kWave) {
                const int64_t j = j0 + lane;
                const int64_t b = few ? mine : j < nb ? edge(j) : -1;
                if (b >= pos && b < pos + kWave) {
                    const uint64_t lt = ((uint64_t)1 << (b - pos)) - 1;
#pragma unroll
                    for (int k = 0; k < 4; ++k) cnt[(r.part0 + (j >> 1)) * 8 + (j & 1) * 4 + k] = run[k] + __popcll(m[k] & lt);
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) run[k] += __popcll(m[k]);
        }
    }

    // 2. the MM text into entries and groups
    PassState st;
    st.ok = r.mm_len >= 0;
    {
        const uint8_t *t = tags + (r.mm_len >= 0 ? r.mm_off : 0);
        const int64_t n = r.mm_len >= 0 ? r.mm_len : 0;
        for (int64_t pos = 0; pos < n; pos += kWave) {
            const LaneA a = lane_load(t, n, pos + lane);
            const uint64_t semi = __ballot(a.semi), comma = __ballot(a.comma);
            const LaneB b = lane_judge(t, n, pos, lane, a, semi, comma, st);
            const int64_t incl = wave_scan(b.end ? b.v + 1 : 0, lane);
            const int64_t at_semi = __shfl((long long)incl, b.ls < 0 ? 0 : b.ls);
            const uint64_t endm = __ballot(b.end);
            const bool bad = lane_store(t, pos, lane, a, b, incl, at_semi, semi, endm, st, ent, e_cap, grp);
            const int64_t total = __shfl((long long)incl, kWave - 1);
            const int64_t at_last = __shfl((long long)incl, semi ? high_bit(semi) : 0);
            pass_advance(&st, pos, semi, comma, endm, total, at_last, __ballot(bad) != 0);
        }
    }
    const bool ok = pass_end(st, r.mm_len >= 0 ? r.mm_len : 0);
    const int64_t n_grp = st.n_grp, ent_n = st.ent_n;
    const int ng = (int)(n_grp < kMaxGroups ? n_grp : kMaxGroups);
    __syncthreads();

    // 3. usable or not; the parts' lengths
    if (lane == 0) {
        int64_t ml_vals = 0;
        const bool usable = finish_groups(grp, ng, ent, ent_n < e_cap ? ent_n : e_cap, r, run, ok, &ml_vals);
        s_usable = usable ? 1 : 0;
        info[ri] = usable ? ng : -1;
    }
    __syncthreads();
    if (!s_usable) return;
    const int has = has_of(r);
    for (int64_t j = 0; j < r.n_parts; ++j) {
        const pcabi_mods_part p = parts[r.part0 + j];
        int64_t b0, b1, mm = 0, ml = 0;
        part_bounds(p, r.l_seq, &b0, &b1);
        if (lane < ng) {
            const Group g = grp[lane];
            const int32_t *c = cnt + (r.part0 + j) * 8;
            const Span s = group_span(g, ent, r.mm_len, base_count(c, g.base, b0), base_count(c + 4, g.base, b1));
            mm = s.mm_bytes;
            ml = (int64_t)(s.e1 - s.e0) * g.n_codes;
        }
        mm = wave_sum(mm);
        ml = wave_sum(ml);
        if (lane == 0) lens[r.part0 + j] = (int32_t)tags_len(mm, ml, has);
    }
}

__global__ __launch_bounds__(kWave) void k_mods_write(const uint8_t *__restrict__ tags, int64_t tags_n,
                                                      const pcabi_mods_read *__restrict__ reads, int64_t n_reads,
                                                      const pcabi_mods_part *__restrict__ parts, int64_t n_parts,
                                                      const int64_t *__restrict__ ent_off, const Ent *__restrict__ ents,
                                                      int64_t n_ents, const Group *__restrict__ groups,
                                                      const int32_t *__restrict__ cnt, const int32_t *__restrict__ info,
                                                      uint8_t *__restrict__ out, int64_t out_cap) {
    __shared__ Span s_span[kMaxGroups];
    __shared__ int64_t s_mm_at[kMaxGroups], s_ml_at[kMaxGroups];
    const int64_t pi = blockIdx.x;
    if (pi >= n_parts) return;
    const int lane = threadIdx.x;
    const pcabi_mods_part p = parts[pi];
    if (p.read < 0 || p.read >= n_reads || p.len <= 0 || p.out < 0 || p.len > out_cap - p.out) return;   // uniform
    const pcabi_mods_read r = reads[p.read];
    const int ng = info[p.read];
    const int64_t e_at = ent_off[p.read], e_cap = ent_off[p.read + 1] - e_at;
    if (ng < 0 || ng > kMaxGroups || r.mm_len < 0 || r.mm_off < 0 || r.mm_len > tags_n - r.mm_off ||
        (r.ml_len >= 0 && (r.ml_off < 0 || r.ml_len > tags_n - r.ml_off)) || e_at < 0 || e_cap < 0 || e_cap > n_ents - e_at)
        return;
    const Group *grp = groups + (int64_t)p.read * kMaxGroups;
    const Ent *ent = ents + e_at;
    int64_t b0, b1, mm = 0, ml = 0;
    part_bounds(p, r.l_seq, &b0, &b1);
    Span s;
    bool fits = true;
    if (lane < ng) {
        const Group g = grp[lane];
        // the plan's checks of the tables, again: this kernel takes them from memory
        fits = g.ent0 >= 0 && g.n_ent >= 0 && (int64_t)g.ent0 + g.n_ent <= e_cap && g.hdr_at >= 0 && g.hdr_len >= 0 &&
               (int64_t)g.hdr_at + g.hdr_len <= r.mm_len && g.n_codes >= 1 && g.ml0 >= 0 &&
               (r.ml_len < 0 || (int64_t)g.ml0 + (int64_t)g.n_ent * g.n_codes <= r.ml_len);
        if (fits) {
            const int32_t *c = cnt + pi * 8;
            s = group_span(g, ent, r.mm_len, base_count(c, g.base, b0), base_count(c + 4, g.base, b1));
            mm = s.mm_bytes;
            ml = (int64_t)(s.e1 - s.e0) * g.n_codes;
        }
    }
    if (__ballot(!fits)) return;
    const int64_t mm_incl = wave_scan(mm, lane), ml_incl = wave_scan(ml, lane);
    const int64_t mm_all = __shfl((long long)mm_incl, kWave - 1), ml_all = __shfl((long long)ml_incl, kWave - 1);
    const int has = has_of(r);
    if (tags_len(mm_all, ml_all, has) != p.len) return;   // uniform
    if (lane < ng) {
        s_span[lane] = s;
        s_mm_at[lane] = mm_incl - mm;
        s_ml_at[lane] = ml_incl - ml;
    }
    __syncthreads();
    uint8_t *dst = out + p.out;
    const uint8_t *text = tags + r.mm_off, *mlv = r.ml_len >= 0 ? tags + r.ml_off : nullptr;
    emit_fixed(dst, mm_all, ml_all, has, (int32_t)(b1 - b0), lane, kWave);
    for (int g = 0; g < ng; ++g)
        emit_group(grp[g], s_span[g], text, mlv, dst + 3 + s_mm_at[g], mlv ? dst + 3 + mm_all + 1 + 8 + s_ml_at[g] : nullptr, lane,
                   kWave);
}

std::atomic<int64_t> g_remapped{0}, g_dropped{0};
std::atomic<int64_t> g_host_ns{0};   // wall time of the host build (plan_host), for the timing tool
std::atomic<int64_t> g_dev_ns{0};    // wall time of the device plan step (copies up, kernel, lengths back)

// The tables against their buffers and each other (PCABI_E_ARG).
int check_tables(int64_t seq_n, int64_t tags_n, const pcabi_mods_read *reads, int64_t n_reads, const pcabi_mods_part *parts,
                 int64_t n_parts) {
    for (int64_t i = 0; i < n_reads; ++i) {
        const pcabi_mods_read &r = reads[i];
        if (!read_fits(r, seq_n, tags_n, n_parts))
            return fail(PCABI_E_ARG, "read " + std::to_string(i) + " of the table does not fit the buffers");
        for (int64_t j = r.part0; j < r.part0 + r.n_parts; ++j) {
            const pcabi_mods_part &p = parts[j];
            if (p.read != i || p.s0 < 0 || p.ns < 0 || (int64_t)p.s0 + p.ns > r.l_seq)
                return fail(PCABI_E_ARG, "part " + std::to_string(j) + " does not lie inside read " + std::to_string(i));
        }
    }
    for (int64_t j = 0; j < n_parts; ++j) {
        const pcabi_mods_part &p = parts[j];
        if (p.read < 0 || p.read >= n_reads || j < reads[p.read].part0 || j >= reads[p.read].part0 + reads[p.read].n_parts)
            return fail(PCABI_E_ARG, "part " + std::to_string(j) + " belongs to no read of the table");
    }
    return 0;
}

std::vector<int64_t> ent_offsets(const pcabi_mods_read *reads, int64_t n_reads) {
    std::vector<int64_t> off((size_t)n_reads + 1, 0);
    for (int64_t i = 0; i < n_reads; ++i) off[(size_t)i + 1] = off[(size_t)i] + ent_cap(reads[i].mm_len);
    return off;
}

}  // namespace

// What the host build's sizing pass leaves for its writing pass, as the device keeps its tables between
// the two kernels: per thread (the two passes cut the reads alike) the entries of its reads, allocated and
// first touched by the thread itself, and their groups back to back; per read where its own lie and how
// many groups it has (-1: not usable); per part the base counts at its edges.
struct pcabi_internal::ModsHost {
    struct Slice {
        std::unique_ptr<Ent[]> ents;
        std::vector<Group> groups;
    };
    std::vector<Slice> slices;
    std::vector<int64_t> ent_at, grp_at;
    std::vector<int32_t> n_groups;
    std::vector<int32_t> cnt;   // 8 a part
};

namespace {

// the host build: reads by threads. out == nullptr sizes (parts[].len, usable, *keep filled); else the
// parts' bytes are written from what *keep holds.
void plan_host(const uint8_t *seq, const uint8_t *tags, const pcabi_mods_read *reads, int64_t n_reads, pcabi_mods_part *parts,
               int64_t n_parts, uint8_t *usable, uint8_t *out, ModsHost *keep) {
    const int nt = (int)std::min<int64_t>(io_thread_count(), std::max<int64_t>(1, n_reads / 64));
    const double t_begin = now_s();
    if (!out) {
        keep->slices = std::vector<ModsHost::Slice>((size_t)nt);
        keep->ent_at.assign((size_t)n_reads, 0);
        keep->grp_at.assign((size_t)n_reads, 0);
        keep->n_groups.assign((size_t)n_reads, -1);
        keep->cnt.assign((size_t)n_parts * 8, 0);
    }
    auto work = [&](int t) {
        const int64_t lo = n_reads * t / nt, hi = n_reads * (t + 1) / nt;
        ModsHost::Slice &mine = keep->slices[(size_t)t];
        if (!out) {
            int64_t cap = 0;
            for (int64_t i = lo; i < hi; ++i) keep->ent_at[(size_t)i] = cap, cap += ent_cap(reads[i].mm_len);
            mine.ents.reset(new Ent[(size_t)cap + 1]);
        }
        ReadTables tb;
        for (int64_t i = lo; i < hi; ++i) {
            const pcabi_mods_read &r = reads[i];
            Ent *ents = mine.ents.get() + keep->ent_at[(size_t)i];
            if (!out) {
                const bool ok = read_tables(r, seq, tags, ents, &tb);
                if (usable) usable[i] = ok ? 1 : 0;
                if (ok) {
                    keep->grp_at[(size_t)i] = (int64_t)mine.groups.size();
                    keep->n_groups[(size_t)i] = tb.n_groups;
                    mine.groups.insert(mine.groups.end(), tb.groups, tb.groups + tb.n_groups);
                }
            }
            const int ng = keep->n_groups[(size_t)i];
            if (ng < 0) continue;
            const Group *groups = mine.groups.data() + keep->grp_at[(size_t)i];
            Counter counter(seq + r.seq_off);
            for (int64_t j = r.part0; j < r.part0 + r.n_parts; ++j) {
                pcabi_mods_part &p = parts[j];
                int32_t *c = keep->cnt.data() + 8 * j;
                if (!out) {
                    std::memcpy(c, counter.to(p.s0), 4 * sizeof(int32_t));
                    std::memcpy(c + 4, counter.to((int64_t)p.s0 + p.ns), 4 * sizeof(int32_t));
                    p.len = (int32_t)part_tags(r, groups, ng, ents, tags, p.s0, p.ns, c, c + 4, nullptr);
                } else if (p.len > 0) {
                    part_tags(r, groups, ng, ents, tags, p.s0, p.ns, c, c + 4, out + p.out);
                }
            }
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

void count_reads(const uint8_t *usable, int64_t n_reads) {
    int64_t good = 0;
    for (int64_t i = 0; i < n_reads; ++i) good += usable[i] ? 1 : 0;
    g_remapped += good;
    g_dropped += n_reads - good;
}

}  // namespace

namespace pcabi_internal {

struct ModsDev {
    DevBuf<> tags;
    DevBuf<pcabi_mods_read> reads;
    DevBuf<pcabi_mods_part> parts;
    DevBuf<Ent> ents;          // every read's entries, ent_off[read] on
    DevBuf<int64_t> ent_off;
    DevBuf<Group> groups;      // kMaxGroups a read
    DevBuf<int32_t> cnt;       // A C G T before a part's start and end: 8 a part
    DevBuf<int32_t> info;      // a read's group count, -1 when its tags are not usable
    DevBuf<int32_t> lens;      // a part's tag bytes: all that comes back of the parts
    int64_t n_reads = 0, n_parts = 0, n_ents = 0, tags_n = 0;   // what the plan before left there
};

int64_t mods_host_ns(int reset, int64_t *dev_plan_ns) {
    const int64_t v = g_host_ns.load();
    *dev_plan_ns = g_dev_ns.load();
    if (reset) g_host_ns = 0, g_dev_ns = 0;
    return v;
}

ModsDev *mods_dev_new() { return new ModsDev; }
void mods_dev_free(ModsDev *d) { delete d; }

int mods_plan_any(int device, ModsDev *dev, ModsHost *keep, void *stream, const uint8_t *seq, const uint8_t *d_seq, int64_t seq_n,
                  const ModsTables &t) {
    if (int rc = check_tables(seq_n, t.tags_n, t.reads, t.n_reads, t.parts, t.n_parts)) return rc;
    for (int64_t j = 0; j < t.n_parts; ++j) t.parts[j].len = 0;
    if (device < 0) plan_host(seq, t.tags, t.reads, t.n_reads, t.parts, t.n_parts, t.usable, nullptr, keep);
    else if (int rc = mods_dev_plan(dev, stream, d_seq, seq_n, t)) return rc;
    count_reads(t.usable, t.n_reads);
    return 0;
}

void mods_write_host(ModsHost *keep, const uint8_t *seq, const ModsTables &t, uint8_t *out) {
    plan_host(seq, t.tags, t.reads, t.n_reads, t.parts, t.n_parts, nullptr, out, keep);
}

ModsHost *mods_host_new() { return new ModsHost; }
void mods_host_free(ModsHost *h) { delete h; }

// The device half: the tag blob and the tables go up (the letters are the caller's, already there), the
// plan kernel runs on `stream`, the parts' lengths and the reads' flags come back. Synchronises.
int mods_dev_plan(ModsDev *d, void *stream, const uint8_t *d_seq, int64_t seq_n, const ModsTables &t) {
    const auto [tags, tags_n, reads, n_reads, parts, n_parts, usable] = t;
    hipStream_t st = (hipStream_t)stream;
    const double t_begin = now_s();
    d->n_reads = d->n_parts = d->n_ents = d->tags_n = 0;
    if (n_reads <= 0) return 0;
    if (n_reads >= INT32_MAX || n_parts >= INT32_MAX) return fail(PCABI_E_ARG, "too many reads for one launch");
    const std::vector<int64_t> off = ent_offsets(reads, n_reads);
    const int64_t n_ents = off.back();
    auto grow = [](int64_t n) { return n + n / 4 + 64; };
    if (int rc = d->tags.reserve(tags_n + 64, grow(tags_n))) return rc;
    if (int rc = d->reads.reserve(n_reads, grow(n_reads))) return rc;
    if (int rc = d->parts.reserve(n_parts + 1, grow(n_parts))) return rc;
    if (int rc = d->ents.reserve(n_ents + 1, grow(n_ents))) return rc;
    if (int rc = d->ent_off.reserve(n_reads + 1, grow(n_reads))) return rc;
    if (int rc = d->groups.reserve(n_reads * kMaxGroups, grow(n_reads) * kMaxGroups)) return rc;
    if (int rc = d->cnt.reserve(n_parts * 8 + 8, grow(n_parts) * 8)) return rc;
    if (int rc = d->info.reserve(n_reads, grow(n_reads))) return rc;
    if (int rc = d->lens.reserve(n_parts + 1, grow(n_parts))) return rc;
    if (n_parts > 0) PCABI_TRY(hipMemsetAsync(d->lens, 0, (size_t)n_parts * 4, st));
    if (tags_n > 0) PCABI_TRY(hipMemcpyAsync(d->tags, tags, (size_t)tags_n, hipMemcpyHostToDevice, st));
    PCABI_TRY(hipMemcpyAsync(d->reads, reads, (size_t)n_reads * sizeof(pcabi_mods_read), hipMemcpyHostToDevice, st));
    if (n_parts > 0) PCABI_TRY(hipMemcpyAsync(d->parts, parts, (size_t)n_parts * sizeof(pcabi_mods_part), hipMemcpyHostToDevice, st));
    PCABI_TRY(hipMemcpyAsync(d->ent_off, off.data(), (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, st));
    const bool prof = prof_on();
    void *sp = prof ? prof_begin(st, 5) : nullptr;
    hipLaunchKernelGGL(k_mods_plan, dim3((unsigned)n_reads), dim3(kWave), 0, st, d_seq, seq_n, d->tags.p, tags_n, d->reads.p, n_reads,
                       d->parts.p, n_parts, d->ent_off.p, d->ents.p, n_ents, d->groups.p, d->cnt.p, d->info.p, d->lens.p);
    PCABI_TRY(hipGetLastError());
    if (prof) {
        prof_end(st, sp);
        int64_t bytes = tags_n + n_ents * (int64_t)sizeof(Ent) + n_parts * (int64_t)(sizeof(pcabi_mods_part) + 32);
        for (int64_t i = 0; i < n_reads; ++i) bytes += reads[i].l_seq + (int64_t)sizeof(pcabi_mods_read);
        prof_add_bytes(5, bytes);
    }
    std::vector<int32_t> info((size_t)n_reads), lens((size_t)n_parts);
    if (n_parts > 0) PCABI_TRY(hipMemcpyAsync(lens.data(), d->lens, (size_t)n_parts * 4, hipMemcpyDeviceToHost, st));
    PCABI_TRY(hipMemcpyAsync(info.data(), d->info, (size_t)n_reads * 4, hipMemcpyDeviceToHost, st));
    PCABI_TRY(hipStreamSynchronize(st));
    for (int64_t i = 0; i < n_reads; ++i) usable[i] = info[(size_t)i] >= 0 ? 1 : 0;
    for (int64_t j = 0; j < n_parts; ++j) parts[j].len = lens[(size_t)j];
    d->n_reads = n_reads, d->n_parts = n_parts, d->n_ents = n_ents, d->tags_n = tags_n;
    g_dev_ns += (int64_t)((now_s() - t_begin) * 1e9);
    return 0;
}

// The parts (with out set) of the plan before it written into d_out[0, out_cap), asynchronous on `stream`.
int mods_dev_write(ModsDev *d, void *stream, const pcabi_mods_part *parts, int64_t n_parts, uint8_t *d_out, int64_t out_cap) {
    hipStream_t st = (hipStream_t)stream;
    if (n_parts != d->n_parts) return fail(PCABI_E_ARG, "not the parts that were planned");
    if (n_parts <= 0 || d->n_reads <= 0) return 0;
    PCABI_TRY(hipMemcpyAsync(d->parts, parts, (size_t)n_parts * sizeof(pcabi_mods_part), hipMemcpyHostToDevice, st));
    const bool prof = prof_on();
    void *sp = prof ? prof_begin(st, 6) : nullptr;
    hipLaunchKernelGGL(k_mods_write, dim3((unsigned)n_parts), dim3(kWave), 0, st, d->tags.p, d->tags_n, d->reads.p, d->n_reads,
                       d->parts.p, n_parts, d->ent_off.p, d->ents.p, d->n_ents, d->groups.p, d->cnt.p, d->info.p, d_out, out_cap);
    PCABI_TRY(hipGetLastError());
    if (prof) {
        prof_end(st, sp);
        int64_t bytes = 0;
        for (int64_t j = 0; j < n_parts; ++j) bytes += 2 * (int64_t)parts[j].len + (int64_t)sizeof(pcabi_mods_part);
        prof_add_bytes(6, bytes);
    }
    return 0;
}

}  // namespace pcabi_internal

extern "C" {

int pcabi_mods_plan(int device, const uint8_t *seq, int64_t seq_n, const uint8_t *tags, int64_t tags_n,
                    const pcabi_mods_read *reads, int64_t n_reads, pcabi_mods_part *parts, int64_t n_parts, uint8_t *usable) {
    if (seq_n < 0 || tags_n < 0 || n_reads < 0 || n_parts < 0 || (seq_n > 0 && !seq) || (tags_n > 0 && !tags) ||
        (n_reads > 0 && (!reads || !usable)) || (n_parts > 0 && !parts))
        return fail(PCABI_E_ARG, "bad arguments");
    const ModsTables t{tags, tags_n, reads, n_reads, parts, n_parts, usable};
    if (device < 0) {
        ModsHost keep;
        return mods_plan_any(-1, nullptr, &keep, nullptr, seq, nullptr, seq_n, t);
    }
    PCABI_TRY(hipSetDevice(device));
    DevBuf<> d_seq;
    ModsDev dev;
    if (int rc = d_seq.reserve(seq_n + 64, seq_n + 64)) return rc;
    if (seq_n > 0) PCABI_TRY(hipMemcpy(d_seq, seq, (size_t)seq_n, hipMemcpyHostToDevice));
    return mods_plan_any(device, &dev, nullptr, nullptr, seq, d_seq, seq_n, t);
}

int pcabi_mods_remap(int device, const uint8_t *seq, int64_t seq_n, const uint8_t *tags, int64_t tags_n,
                     const pcabi_mods_read *reads, int64_t n_reads, const pcabi_mods_part *parts, int64_t n_parts, uint8_t *out,
                     int64_t out_cap) {
    if (seq_n < 0 || tags_n < 0 || n_reads < 0 || n_parts < 0 || out_cap < 0 || (seq_n > 0 && !seq) || (tags_n > 0 && !tags) ||
        (n_reads > 0 && !reads) || (n_parts > 0 && !parts) || (out_cap > 0 && !out))
        return fail(PCABI_E_ARG, "bad arguments");
    if (int rc = check_tables(seq_n, tags_n, reads, n_reads, parts, n_parts)) return rc;
    // the plan again, on the host: the caller's lengths must be its lengths, and no two ranges may meet
    std::vector<pcabi_mods_part> mine(parts, parts + n_parts);
    std::vector<uint8_t> usable((size_t)n_reads);
    ModsHost keep;
    plan_host(seq, tags, reads, n_reads, mine.data(), n_parts, usable.data(), nullptr, &keep);
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
        plan_host(seq, tags, reads, n_reads, const_cast<pcabi_mods_part *>(parts), n_parts, nullptr, out, &keep);
        return 0;
    }
    PCABI_TRY(hipSetDevice(device));
    constexpr int64_t kGuard = 64;
    std::vector<uint8_t> stage((size_t)(out_cap + 2 * kGuard), 0xA5);
    if (out_cap > 0) std::memcpy(stage.data() + kGuard, out, (size_t)out_cap);
    DevBuf<> d_seq, d_out;
    ModsDev dev;
    if (int rc = d_seq.reserve(seq_n + 64, seq_n + 64)) return rc;
    if (int rc = d_out.reserve((int64_t)stage.size(), (int64_t)stage.size())) return rc;
    if (seq_n > 0) PCABI_TRY(hipMemcpy(d_seq, seq, (size_t)seq_n, hipMemcpyHostToDevice));
    PCABI_TRY(hipMemcpy(d_out, stage.data(), stage.size(), hipMemcpyHostToDevice));
    if (int rc = mods_dev_plan(&dev, nullptr, d_seq, seq_n, ModsTables{tags, tags_n, reads, n_reads, mine.data(), n_parts, usable.data()})) return rc;
    for (int64_t j = 0; j < n_parts; ++j)
        if (mine[(size_t)j].len != parts[j].len) return fail(PCABI_E_DEVICE, "k_mods_plan and the host build disagree on part " + std::to_string(j));
    if (int rc = mods_dev_write(&dev, nullptr, parts, n_parts, d_out + kGuard, out_cap)) return rc;
    PCABI_TRY(hipStreamSynchronize(nullptr));
    PCABI_TRY(hipMemcpy(stage.data(), d_out, stage.size(), hipMemcpyDeviceToHost));
    for (int64_t g = 0; g < kGuard; ++g)
        if (stage[(size_t)(kGuard - 1 - g)] != 0xA5 || stage[(size_t)(kGuard + out_cap + g)] != 0xA5)
            return fail(PCABI_E_DEVICE, "k_mods_write wrote outside its output");
    if (out_cap > 0) std::memcpy(out, stage.data() + kGuard, (size_t)out_cap);
    return 0;
}

void pcabi_mods_counts(int reset, int64_t *remapped, int64_t *dropped) {
    if (remapped) *remapped = g_remapped.load();
    if (dropped) *dropped = g_dropped.load();
    if (reset) g_remapped = 0, g_dropped = 0;
}

}  // extern "C"
