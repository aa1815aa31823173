// pcabi_mods.h -- base-modification tags (MM / ML / MN, SAMtags "Base modifications") remapped onto
// parts of a read: the MM grammar, the usability checks and the per-part rule (pcabi_mods.hip,
// pcabi_write.cpp; include/pcabi.h pcabi_mods_*; DESIGN.md "BAM output"). Nothing here is device-only: the
// kernels, the host build (device < 0) and the CPU tests (tests/mods_fuzz_main.cpp builds it alone) run
// the same code. What differs is the walk over the tag text: parse() goes byte by byte, the kernel takes
// 64 bytes a pass and gets every byte's group start and counts state from ballots; both judge a byte with
// byte_ok(), read a number with count_at() and fill the same two tables.
//
// MM text: groups `base strand codes [flag] (,count)* ;` with base one of ACGTUN, strand + or -, codes
// lower-case letters or one decimal number, flag . or ?. A count says how many occurrences of the
// group's base (U counts T, N counts every base) to skip before the next modified one, along the read
// as the reader returns it. So a group's entries have ordinals o0 = d0, ok = o(k-1) + 1 + dk among the
// occurrences of its base, and a part [s0, s0 + ns) with c0 / c1 occurrences before its start / end
// keeps the entries with c0 <= ordinal < c1: a contiguous run [e0, e1). The group is written as its
// header, then ",ordinal(e0) - c0", then the text of the counts e0 + 1 .. e1 - 1 as it stood, then ";".
// ML holds one byte per entry per code in MM order, MN the read's length.
//
// Tables of one read: Ent per count (its ordinal; `tend`, the text offset behind its last digit),
// Group per group. Every offset taken from a table is checked against its buffer before it is used.
#pragma once
#include "pcabi_bam.h"

namespace pcabi_mods {

constexpr int kMaxGroups = 32;                 // groups per read; a read with more is not usable
constexpr int64_t kSat = (int64_t)1 << 32;     // counts and ordinals saturate here (above every int32)

struct Ent {
    int32_t ord, tend;
};
struct Group {
    int32_t hdr_at, hdr_len;   // base, strand, codes and flag in the MM text
    int32_t ent0, n_ent;       // its entries in the read's Ent table
    int32_t n_codes, base;     // ML values per entry; 0..3 = A C G T (U), 4 = N
    int32_t ml0, reserved;     // ML values of the groups before it
};

PCABI_HD inline bool is_digit(uint32_t c) { return c - '0' < 10u; }
PCABI_HD inline bool is_lower(uint32_t c) { return c - 'a' < 26u; }
PCABI_HD inline bool is_flag(uint32_t c) { return c == '.' || c == '?'; }
// a group's base letter: 0..3 for A C G T, U as T, 4 for N, -1 for anything else
PCABI_HD inline int group_base(uint32_t c) {
    return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' || c == 'U' ? 3 : c == 'N' ? 4 : -1;
}
// a read letter as the pack writes it (pcabi_bam.h code_of): 0..3 for A C G T, 4 for any other code
PCABI_HD inline int letter_class(uint32_t c) {
    const uint32_t k = pcabi_bam::code_of(c);
    return k == 1 ? 0 : k == 2 ? 1 : k == 4 ? 2 : k == 8 ? 3 : 4;
}

// Whether byte c may stand where it stands: p = the byte before it (';' before the first), rel = its
// offset from its group's start, in_counts = a ',' came since the group's start. A text all of whose
// bytes pass and whose last byte is ';' (or that is empty) is well formed.
PCABI_HD inline bool byte_ok(uint32_t c, uint32_t p, int64_t rel, bool in_counts) {
    if (rel == 0) return group_base(c) >= 0;
    if (rel == 1) return c == '+' || c == '-';
    const bool pd = is_digit(p), pl = is_lower(p), pf = is_flag(p);
    if (c == ',') return pd || (!in_counts && (pl || pf));
    if (in_counts) return is_digit(c) || (c == ';' && pd);
    if (is_lower(c)) return rel == 2 || pl;
    if (is_digit(c)) return rel == 2 || pd;
    if (is_flag(c)) return pl || pd;
    if (c == ';') return pl || pd || pf;
    return false;
}

// The decimal number whose last digit is t[i] (i < n), saturated at kSat. Leading zeros are fine.
PCABI_HD inline int64_t count_at(const uint8_t *t, int64_t n, int64_t i) {
    if (i < 0 || i >= n) return kSat;
    int64_t k = i;
    while (k > 0 && is_digit(t[k - 1])) --k;
    int64_t v = 0;
    for (; k <= i; ++k) {
        v = v * 10 + (int64_t)(t[k] - '0');
        if (v > kSat) v = kSat;
    }
    return v;
}

// What the byte that ends a group's header (its first ',', or its ';' when it has no counts) knows
// about the group: t[at, i) is the header.
PCABI_HD inline void group_head(const uint8_t *t, int64_t at, int64_t i, Group *g) {
    g->hdr_at = (int32_t)at;
    g->hdr_len = (int32_t)(i - at);
    g->base = i > at ? group_base(t[at]) : -1;
    int64_t codes = i - at - 2;
    if (codes > 0 && is_flag(t[i - 1])) --codes;
    g->n_codes = (codes > 0 && is_digit(t[at + 2])) ? 1 : (int32_t)(codes > 0 ? codes : 0);
}

// The walk, byte by byte: t[0, n) into ents[0, cap) and groups[0, kMaxGroups). false when the text is
// not well formed, a count does not fit int32, or there are more groups or entries than the tables hold.
inline bool parse(const uint8_t *t, int64_t n, Ent *ents, int64_t cap, Group *groups, int *n_groups) {
    int64_t at = 0, n_ent = 0, ent0 = 0, sum = 0;
    int ng = 0;
    bool in_counts = false, ok = true;
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t c = t[i], p = i > 0 ? t[i - 1] : (uint32_t)';';
        ok = ok && byte_ok(c, p, i - at, in_counts);
        if (in_counts && is_digit(c) && !(i + 1 < n && is_digit(t[i + 1]))) {
            const int64_t v = count_at(t, n, i);
            ok = ok && v <= INT32_MAX && n_ent < cap;
            sum += v + 1;
            if (sum > kSat * 256) sum = kSat * 256;
            if (n_ent < cap) ents[n_ent] = Ent{(int32_t)(sum - 1 > INT32_MAX ? INT32_MAX : sum - 1), (int32_t)(i + 1)};
            ++n_ent;
        }
        if ((c == ',' && !in_counts) || (c == ';' && !in_counts)) {
            if (ng < kMaxGroups) group_head(t, at, i, &groups[ng]);
        }
        if (c == ',') in_counts = true;
        if (c == ';') {
            if (ng < kMaxGroups) {
                groups[ng].ent0 = (int32_t)ent0;
                groups[ng].n_ent = (int32_t)(n_ent - ent0);
                groups[ng].ml0 = groups[ng].reserved = 0;
            }
            ++ng;
            at = i + 1;
            ent0 = n_ent;
            sum = 0;
            in_counts = false;
        }
    }
    ok = ok && at == n && ng <= kMaxGroups;
    *n_groups = ng < kMaxGroups ? ng : kMaxGroups;
    return ok;
}

// ---- the walk, 64 bytes a pass (the kernel; tests/mods_fuzz_main.cpp plays the lanes) -----------------
// A pass takes t[pos, pos + 64), a byte a lane. Between the lane functions stand the wave's collectives:
// ballots of a.semi and a.comma before lane_judge; an inclusive scan `incl` of (b.end ? b.v + 1 : 0), its
// value at lane b.ls, and a ballot of b.end before lane_store; a ballot of what lane_store returns, the
// scan's total and its value at the pass's last ';' before pass_advance.
struct PassState {   // what a pass hands to the next (uniform)
    int64_t g_start = 0, last_comma = -1;   // where the open group starts; the last ',' so far
    int64_t ordsum = 0, ent_grp = 0;        // the open group's sum of count + 1, and its entries
    int64_t n_grp = 0, ent_n = 0;           // closed groups; entries
    bool ok = true;
};
struct LaneA {
    uint32_t c, p;
    bool act, semi, comma;
};
struct LaneB {
    int64_t at, v;   // its group's start; the count that ends here
    int ls;          // the lane of the last ';' before this one in the pass, or -1
    bool in_counts, bad, end;
};
PCABI_HD inline int high_bit(uint64_t m) { return 63 - __builtin_clzll(m); }
PCABI_HD inline LaneA lane_load(const uint8_t *t, int64_t n, int64_t i) {
    LaneA a;
    a.act = i < n;
    a.c = a.act ? t[i] : 0u;
    a.p = (a.act && i > 0) ? t[i - 1] : (uint32_t)';';
    a.semi = a.act && a.c == ';';
    a.comma = a.act && a.c == ',';
    return a;
}
PCABI_HD inline LaneB lane_judge(const uint8_t *t, int64_t n, int64_t pos, int lane, const LaneA &a, uint64_t semi, uint64_t comma,
                                 const PassState &st) {
    const uint64_t below = ((uint64_t)1 << lane) - 1, sb = semi & below, cb = comma & below;
    const int64_t i = pos + lane;
    LaneB b;
    b.ls = sb ? high_bit(sb) : -1;
    b.at = sb ? pos + b.ls + 1 : st.g_start;
    const int64_t lc = cb ? pos + high_bit(cb) : st.last_comma;
    b.in_counts = lc >= b.at;
    b.bad = a.act && !byte_ok(a.c, a.p, i - b.at, b.in_counts);
    b.end = a.act && b.in_counts && is_digit(a.c) && !(i + 1 < n && is_digit(t[i + 1]));
    b.v = b.end ? count_at(t, n, i) : 0;
    return b;
}
// writes the lane's entry and its share of its group's record; returns whether the lane saw the text fail
PCABI_HD inline bool lane_store(const uint8_t *t, int64_t pos, int lane, const LaneA &a, const LaneB &b, int64_t incl, int64_t at_semi,
                                uint64_t semi, uint64_t endm, const PassState &st, Ent *ent, int64_t e_cap, Group *grp) {
    const uint64_t below = ((uint64_t)1 << lane) - 1, sb = semi & below;
    const int64_t i = pos + lane;
    int64_t ord = (sb ? incl - at_semi : st.ordsum + incl) - 1;
    if (ord > INT32_MAX) ord = INT32_MAX;
    const uint64_t mine = sb ? endm & below & ~(((uint64_t)2 << b.ls) - 1) : endm & below;   // ends before it in its group
    const int64_t k_all = st.ent_n + __builtin_popcountll(endm & below);
    const int64_t k_grp = (sb ? 0 : st.ent_grp) + __builtin_popcountll(mine);
    const int64_t gi = st.n_grp + __builtin_popcountll(sb);
    bool bad = b.bad;
    if (b.end) {
        if (b.v > INT32_MAX || k_all >= e_cap) bad = true;
        else ent[k_all] = Ent{(int32_t)ord, (int32_t)(i + 1)};
    }
    if (a.act && !b.in_counts && (a.c == ',' || a.c == ';') && gi < kMaxGroups) group_head(t, b.at, i, &grp[gi]);
    if (a.semi && gi < kMaxGroups) {
        grp[gi].ent0 = (int32_t)(k_all - k_grp);
        grp[gi].n_ent = (int32_t)k_grp;
        grp[gi].ml0 = grp[gi].reserved = 0;
    }
    return bad;
}
// total = the scan's value at lane 63, at_last = its value at the lane of the pass's last ';'
PCABI_HD inline void pass_advance(PassState *st, int64_t pos, uint64_t semi, uint64_t comma, uint64_t endm, int64_t total,
                                  int64_t at_last, bool any_bad) {
    if (semi) {
        const int last = high_bit(semi);
        st->g_start = pos + last + 1;
        st->ordsum = total - at_last;
        st->ent_grp = __builtin_popcountll(endm & ~(((uint64_t)2 << last) - 1));
    } else {
        st->ordsum += total;
        st->ent_grp += __builtin_popcountll(endm);
    }
    if (st->ordsum > kSat * 256) st->ordsum = kSat * 256;
    if (comma) st->last_comma = pos + high_bit(comma);
    st->n_grp += __builtin_popcountll(semi);
    st->ent_n += __builtin_popcountll(endm);
    if (any_bad) st->ok = false;
}
PCABI_HD inline bool pass_end(const PassState &st, int64_t n) { return st.ok && st.g_start == n && st.n_grp <= kMaxGroups; }

// The number of occurrences of a group's base before position b, from the counts of A C G T before it.
PCABI_HD inline int64_t base_count(const int32_t *acgt, int base, int64_t b) { return base >= 0 && base < 4 ? acgt[base] : b; }

// Group g against its tables and the read: the entries inside ents[0, n_ent_all), a header inside the
// text, and the last ordinal below the read's count of the base.
PCABI_HD inline bool group_ok(const Group &g, const Ent *ents, int64_t n_ent_all, int64_t mm_len, const int32_t *acgt_all,
                              int64_t l_seq) {
    if (g.ent0 < 0 || g.n_ent < 0 || (int64_t)g.ent0 + g.n_ent > n_ent_all) return false;
    if (g.hdr_at < 0 || g.hdr_len < 3 || (int64_t)g.hdr_at + g.hdr_len > mm_len || g.n_codes < 1 || g.base < 0) return false;
    if (g.n_ent == 0) return true;
    return (int64_t)ents[g.ent0 + g.n_ent - 1].ord < base_count(acgt_all, g.base, l_seq);
}

// The first entry of e[0, n) whose ordinal is >= c (ordinals ascend).
PCABI_HD inline int32_t first_at_least(const Ent *e, int32_t n, int64_t c) {
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if ((int64_t)e[mid].ord < c) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

PCABI_HD inline int digits_of(uint32_t v) {
    int k = 1;
    while (v >= 10) v /= 10, ++k;
    return k;
}

// A group's share of a part: the kept entries [e0, e1), the first kept count, the bytes of MM text it
// takes and where the verbatim counts lie.
struct Span {
    int32_t e0, e1;
    uint32_t first;        // ordinal(e0) - c0
    int32_t from, to;      // the MM text [from, to): ",count" of the entries e0 + 1 .. e1 - 1
    int32_t mm_bytes;      // header, counts and ';'
};
PCABI_HD inline Span group_span(const Group &g, const Ent *ents, int64_t mm_len, int64_t c0, int64_t c1) {
    Span s;
    const Ent *e = ents + g.ent0;
    s.e0 = first_at_least(e, g.n_ent, c0);
    s.e1 = first_at_least(e, g.n_ent, c1);
    if (s.e1 < s.e0) s.e1 = s.e0;
    s.first = 0;
    s.from = s.to = 0;
    s.mm_bytes = g.hdr_len + 1;
    if (s.e1 > s.e0) {
        s.first = (uint32_t)((int64_t)e[s.e0].ord - c0);
        s.from = e[s.e0].tend;
        s.to = e[s.e1 - 1].tend;
        if (s.from < 0 || s.to < s.from || s.to > mm_len) s.from = s.to = 0;   // tables the parse did not write
        s.mm_bytes += 1 + digits_of(s.first) + (s.to - s.from);
    }
    return s;
}

// A part's tag bytes: MM (Z), then ML (B:C) when the read had one, then MN (i) when it had one.
constexpr int kHasMl = 1, kHasMn = 2, kOldMm = 4, kOldMl = 8;
PCABI_HD inline int64_t tags_len(int64_t mm_bytes, int64_t ml_vals, int has) {
    return 3 + mm_bytes + 1 + ((has & kHasMl) ? 8 + ml_vals : 0) + ((has & kHasMn) ? 7 : 0);
}

// The fixed bytes of a part's tags: byte copies k = first, first + step, ... of the MM tag's name and
// type, its NUL, the ML tag's head and the whole MN tag. mm_bytes / ml_vals: the sums over the groups.
PCABI_HD inline void emit_fixed(uint8_t *dst, int64_t mm_bytes, int64_t ml_vals, int has, int32_t ns, int64_t first, int64_t step) {
    uint8_t f[19];
    f[0] = 'M', f[1] = (has & kOldMm) ? 'm' : 'M', f[2] = 'Z', f[3] = 0;
    f[4] = 'M', f[5] = (has & kOldMl) ? 'l' : 'L', f[6] = 'B', f[7] = 'C';
    for (int k = 0; k < 4; ++k) f[8 + k] = (uint8_t)((uint32_t)ml_vals >> (8 * k));
    f[12] = 'M', f[13] = 'N', f[14] = 'i';
    for (int k = 0; k < 4; ++k) f[15 + k] = (uint8_t)((uint32_t)ns >> (8 * k));
    const int64_t nul = 3 + mm_bytes, ml_at = nul + 1, mn_at = ml_at + ((has & kHasMl) ? 8 + ml_vals : 0);
    for (int64_t k = first; k < 3; k += step) dst[k] = f[k];
    if (first == 0) dst[nul] = 0;
    if (has & kHasMl)
        for (int64_t k = first; k < 8; k += step) dst[ml_at + k] = f[4 + k];
    if (has & kHasMn)
        for (int64_t k = first; k < 7; k += step) dst[mn_at + k] = f[12 + k];
}

// One group's bytes of a part: mm = where its MM bytes go, ml = where its ML values go (nullptr: none);
// text / mlv = the read's MM text and ML values. Byte copies first, first + step, ...
PCABI_HD inline void emit_group(const Group &g, const Span &s, const uint8_t *text, const uint8_t *mlv, uint8_t *mm, uint8_t *ml,
                                int64_t first, int64_t step) {
    for (int64_t k = first; k < g.hdr_len; k += step) mm[k] = text[g.hdr_at + k];
    uint8_t *q = mm + g.hdr_len;
    if (s.e1 > s.e0) {
        const int nd = digits_of(s.first);
        if (first == 0) {
            q[0] = ',';
            uint32_t v = s.first;
            for (int k = nd; k >= 1; --k) q[k] = (uint8_t)('0' + v % 10), v /= 10;
        }
        q += 1 + nd;
        const int64_t run = s.to - s.from;
        for (int64_t k = first; k < run; k += step) q[k] = text[s.from + k];
        q += run;
        if (ml) {
            const int64_t nv = (int64_t)(s.e1 - s.e0) * g.n_codes;
            const uint8_t *src = mlv + g.ml0 + (int64_t)s.e0 * g.n_codes;
            for (int64_t k = first; k < nv; k += step) ml[k] = src[k];
        }
    }
    if (first == 0) q[0] = ';';
}

// ---- one read, on the host -----------------------------------------------------------------------
// A read's tags against its letters: the tables filled and whether the tags are usable.
struct ReadTables {
    Group groups[kMaxGroups];
    int n_groups = 0;
    int64_t ml_vals = 0;
};

// A table entry against the buffers it names.
PCABI_HD inline bool read_fits(const pcabi_mods_read &r, int64_t seq_n, int64_t tags_n, int64_t n_parts) {
    if (r.l_seq < 0 || r.seq_off < 0 || r.l_seq > seq_n - r.seq_off) return false;
    if (r.n_parts < 0 || r.part0 < 0 || r.n_parts > n_parts - r.part0) return false;
    if (r.mm_len >= 0 && (r.mm_off < 0 || r.mm_len > tags_n - r.mm_off)) return false;
    if (r.ml_len >= 0 && (r.ml_off < 0 || r.ml_len > tags_n - r.ml_off)) return false;
    return true;
}
PCABI_HD inline int has_of(const pcabi_mods_read &r) {
    return (r.ml_len >= 0 ? kHasMl : 0) | (r.mn >= 0 ? kHasMn : 0) | ((r.flags & PCABI_MODS_OLD_MM) ? kOldMm : 0) |
           ((r.flags & PCABI_MODS_OLD_ML) ? kOldMl : 0);
}
// the entries a read's MM text can hold at most (",d" each; a text that ends in a digit one more)
PCABI_HD inline int64_t ent_cap(int64_t mm_len) { return mm_len > 0 ? mm_len / 2 + 1 : 0; }

// Counts of A C G T in seq[0, b), kept so that ascending boundaries of one read cost one pass over it.
struct Counter {
    const uint8_t *seq;
    int64_t pos = 0;
    int32_t acgt[4] = {0, 0, 0, 0};
    explicit Counter(const uint8_t *s) : seq(s) {}
    const int32_t *to(int64_t b) {
        static const struct Table {
            uint8_t k[256];
            Table() {
                for (int c = 0; c < 256; ++c) k[c] = (uint8_t)letter_class((uint32_t)c);
            }
        } table;
        if (b < pos) pos = 0, acgt[0] = acgt[1] = acgt[2] = acgt[3] = 0;
        int32_t n[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (; pos < b; ++pos) ++n[table.k[seq[pos]]];
        for (int k = 0; k < 4; ++k) acgt[k] += n[k];
        return acgt;
    }
};
inline void count_to(const uint8_t *seq, int64_t b, int32_t *acgt) {
    Counter c(seq);
    memcpy(acgt, c.to(b), 4 * sizeof(int32_t));
}

// The checks behind the parse, shared with the kernel: the groups against the read, ML's length, MN,
// the host's own verdict. Fills every group's ml0. ok = what the parse returned.
PCABI_HD inline bool finish_groups(Group *groups, int n_groups, const Ent *ents, int64_t n_ent_all, const pcabi_mods_read &r,
                                   const int32_t *acgt_all, bool ok, int64_t *ml_vals) {
    int64_t ml = 0;
    for (int g = 0; g < n_groups; ++g) {
        ok = ok && group_ok(groups[g], ents, n_ent_all, r.mm_len, acgt_all, r.l_seq);
        groups[g].ml0 = (int32_t)ml;
        if (ok) ml += (int64_t)groups[g].n_ent * groups[g].n_codes;
    }
    *ml_vals = ml;
    if (r.flags & PCABI_MODS_BAD) ok = false;
    if (r.mm_len < 0) ok = false;
    if (r.ml_len >= 0 && ml != r.ml_len) ok = false;
    if (r.mn >= 0 && r.mn != r.l_seq) ok = false;
    return ok;
}

inline bool read_tables(const pcabi_mods_read &r, const uint8_t *seq, const uint8_t *tags, Ent *ents, ReadTables *t) {
    bool ok = r.mm_len >= 0;
    t->n_groups = 0;
    if (ok) ok = parse(tags + r.mm_off, r.mm_len, ents, ent_cap(r.mm_len), t->groups, &t->n_groups);
    int32_t all[4];
    count_to(seq + r.seq_off, r.l_seq, all);
    return finish_groups(t->groups, t->n_groups, ents, ent_cap(r.mm_len), r, all, ok, &t->ml_vals);
}

// A part of a usable read: its tags' length, and with dst their bytes too. c0 / c1: counts of A C G T
// before the part's start and end.
inline int64_t part_tags(const pcabi_mods_read &r, const Group *groups, int n_groups, const Ent *ents, const uint8_t *tags, int64_t s0,
                         int64_t ns, const int32_t *c0, const int32_t *c1, uint8_t *dst) {
    int64_t mm = 0, ml = 0;
    const int has = has_of(r);
    for (int pass = 0; pass < (dst ? 2 : 1); ++pass) {
        int64_t mm_at = 0, ml_at = 0;
        for (int g = 0; g < n_groups; ++g) {
            const Group &gr = groups[g];
            const Span s = group_span(gr, ents, r.mm_len, base_count(c0, gr.base, s0), base_count(c1, gr.base, s0 + ns));
            if (pass == 1)
                emit_group(gr, s, tags + r.mm_off, r.ml_len >= 0 ? tags + r.ml_off : nullptr, dst + 3 + mm_at,
                           r.ml_len >= 0 ? dst + 3 + mm + 1 + 8 + ml_at : nullptr, 0, 1);
            mm_at += s.mm_bytes;
            ml_at += (int64_t)(s.e1 - s.e0) * gr.n_codes;
        }
        mm = mm_at, ml = ml_at;
    }
    if (dst) emit_fixed(dst, mm, ml, has, (int32_t)ns, 0, 1);
    return tags_len(mm, ml, has);
}
inline int64_t part_tags(const pcabi_mods_read &r, const ReadTables &t, const Ent *ents, const uint8_t *tags, int64_t s0, int64_t ns,
                         const int32_t *c0, const int32_t *c1, uint8_t *dst) {
    return part_tags(r, t.groups, t.n_groups, ents, tags, s0, ns, c0, c1, dst);
}

}  // namespace pcabi_mods
