// pcabi_auxtext.h -- the SAM text of BAM aux chains, and text records (FASTQ / FASTA) that carry it in
// their headers: the tag walk, the guards, the digit rule and the byte emitters (pcabi_auxtext.hip,
// pcabi_write.cpp; include/pcabi.h pcabi_auxtext_*, pcabi_fastx_pack_*; DESIGN.md "Tags in text headers").
// Nothing here is device-only: the kernels, the host build (device < 0) and the CPU tests
// (tests/auxtext_fuzz_main.cpp builds it alone) run the same code.
//
// Text of a chain: per tag a tab, the two name bytes, ':', the type letter (c C s S i I all give 'i'),
// ':' and the value; an array is its subtype letter and ",value" per element. A tag whose name is not
// [A-Za-z][A-Za-z0-9], or whose A / Z / H value holds a byte outside 0x20..0x7E, is left out. A chain
// that does not walk (unknown type or subtype, Z / H without its NUL, a value past the end) has no text:
// length -1.
//
// The walk is uniform over a wave: every lane reads the same tag header. Inside a tag the lanes share
// the bytes: a Z / H value goes 64 bytes a pass (zh_lane names what a lane saw, two ballots find the
// NUL and a byte that is not printable), an array 64 elements a pass (elem_len gives a lane its
// element's characters from comparisons, a wave scan places it, elem_put stores its own digits).
// Floats: the host prints them (float_text, C's %g of the value widened to double); a device build
// reads them from a table of 16-byte slots the host made for the chain, in the order the walk meets
// them (float_slot).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/pcabi.h"

#ifndef PCABI_HD
#if defined(__HIPCC__)
#define PCABI_HD __host__ __device__
#else
#define PCABI_HD
#endif
#endif

namespace pcabi_auxtext {

constexpr int kWaveLanes = 64;
constexpr int kHead = 6;          // tab, two name bytes, ':', the type letter, ':'
constexpr int kFloatSlot = 16;    // a float's text in the host's table: its length, then at most 15 characters
constexpr int kTileBases = 16384; // bases a workgroup of k_fastx_pack copies
constexpr int kFastaLine = 70;

PCABI_HD inline int width_of(uint8_t t) {
    return t == 'c' || t == 'C' ? 1 : t == 's' || t == 'S' ? 2 : t == 'i' || t == 'I' || t == 'f' ? 4 : 0;
}
PCABI_HD inline bool is_int(uint8_t t) { return t == 'c' || t == 'C' || t == 's' || t == 'S' || t == 'i' || t == 'I'; }
PCABI_HD inline bool alpha(uint8_t c) { return (uint8_t)((c | 0x20) - 'a') < 26; }
PCABI_HD inline bool name_ok(const uint8_t *tg) { return alpha(tg[0]) && (alpha(tg[1]) || (uint8_t)(tg[1] - '0') < 10); }
PCABI_HD inline bool printable(uint8_t c) { return c >= 0x20 && c <= 0x7E; }
PCABI_HD inline uint32_t le32u(const uint8_t *p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// the value of an integer of type t (c C s S i I) at p
PCABI_HD inline int64_t int_at(const uint8_t *p, uint8_t t) {
    switch (t) {
        case 'c': return (int8_t)p[0];
        case 'C': return p[0];
        case 's': return (int16_t)((uint32_t)p[0] | (uint32_t)p[1] << 8);
        case 'S': return (int64_t)((uint32_t)p[0] | (uint32_t)p[1] << 8);
        case 'i': return (int32_t)le32u(p);
        default: return (int64_t)le32u(p);
    }
}

// characters of v in decimal, the sign included (|v| <= 2^32): comparisons, no division
PCABI_HD inline int dec_len(int64_t v) {
    const uint64_t m = v < 0 ? (uint64_t)(-v) : (uint64_t)v;
    int d = 1;
    d += m >= 10u;
    d += m >= 100u;
    d += m >= 1000u;
    d += m >= 10000u;
    d += m >= 100000u;
    d += m >= 1000000u;
    d += m >= 10000000u;
    d += m >= 100000000u;
    d += m >= 1000000000u;
    return d + (v < 0);
}
// v in decimal at dst[0, n), n = dec_len(v); bytes at or behind dst + room are not written
PCABI_HD inline void dec_put(uint8_t *dst, int64_t room, int64_t v, int n) {
    uint64_t m = v < 0 ? (uint64_t)(-v) : (uint64_t)v;
    for (int k = n - 1; k >= (v < 0 ? 1 : 0); --k) {
        if (k < room) dst[k] = (uint8_t)('0' + m % 10u);
        m /= 10u;
    }
    if (v < 0 && room > 0) dst[0] = '-';
}

// A float's text, C's printf("%g") of the float32 at p widened to double: t[0, return value).
// Host only: a device build reads what the host printed (float_slot).
inline int float_text(const uint8_t *p, char t[kFloatSlot]) {
    float f;
    memcpy(&f, p, 4);
    const int n = snprintf(t, kFloatSlot, "%g", (double)f);
    return n < 0 ? 0 : n < kFloatSlot ? n : kFloatSlot - 1;
}
// slot k of the host's table: the text's length (0 when k lies outside the table), *t = its characters
PCABI_HD inline int float_slot(const uint8_t *ftext, int64_t n_slots, int64_t k, const uint8_t **t) {
    if (!ftext || k < 0 || k >= n_slots) return 0;
    const uint8_t *s = ftext + k * kFloatSlot;
    *t = s + 1;
    return s[0] < kFloatSlot ? s[0] : kFloatSlot - 1;
}

// Where a chain's floats come from: a host build prints them (ftext == nullptr), a device build and a
// host build that is given the table read slot `cur` on.
struct Floats {
    const uint8_t *ftext;
    int64_t n_slots;
    int64_t cur;
};
PCABI_HD inline int float_get(const Floats &fl, int64_t k, const uint8_t *p, uint8_t t[kFloatSlot]) {
#if !defined(__HIP_DEVICE_COMPILE__)
    if (!fl.ftext) return float_text(p, (char *)t);
#endif
    const uint8_t *s = nullptr;
    const int n = float_slot(fl.ftext, fl.n_slots, fl.cur + k, &s);
    for (int j = 0; j < n; ++j) t[j] = s[j];
    return n;
}

// One tag's header, read the same by every lane. ok = false: the chain does not walk here (Z / H are
// not yet searched for their NUL: next = -1 until zh_end is known).
struct Tag {
    bool ok;
    uint8_t type, sub;
    int w;           // bytes of a value or an element
    int64_t val;     // the value's (the first element's) offset in the chain
    int64_t count;   // elements of an array
    int64_t next;
};
PCABI_HD inline Tag tag_at(const uint8_t *a, int64_t n, int64_t at) {
    Tag t;
    t.ok = false, t.type = t.sub = 0, t.w = 0, t.val = t.count = 0, t.next = -1;
    if (at < 0 || n - at < 3) return t;
    t.type = a[at + 2];
    t.val = at + 3;
    if (t.type == 'A') {
        t.w = 1;
    } else if (width_of(t.type)) {
        t.w = width_of(t.type);
    } else if (t.type == 'Z' || t.type == 'H') {
        t.ok = true;
        return t;
    } else if (t.type == 'B') {
        if (n - t.val < 5 || !width_of(a[t.val])) return t;
        t.sub = a[t.val];
        t.w = width_of(t.sub);
        t.count = (int64_t)le32u(a + t.val + 1);
        t.val += 5;
        if (t.count * t.w > n - t.val) return t;
        t.ok = true;
        t.next = t.val + t.count * t.w;
        return t;
    } else {
        return t;
    }
    if (n - t.val < t.w) return t;
    t.ok = true;
    t.next = t.val + t.w;
    return t;
}

// what a lane sees of a Z / H value at a[pos]: 0 a printable byte, 1 the NUL, 2 any other byte, 3 past the end
PCABI_HD inline int zh_lane(const uint8_t *a, int64_t n, int64_t pos) {
    if (pos >= n) return 3;
    const uint8_t c = a[pos];
    return c == 0 ? 1 : printable(c) ? 0 : 2;
}

// characters of element k of an array, its comma included
PCABI_HD inline int elem_len(const uint8_t *a, const Tag &t, int64_t k, const Floats &fl) {
    if (t.sub == 'f') {
        uint8_t s[kFloatSlot];
        return 1 + float_get(fl, k, a + t.val + 4 * k, s);
    }
    return 1 + dec_len(int_at(a + t.val + k * t.w, t.sub));
}
// element k written at dst[0, len): the comma, then its characters; nothing at or behind dst + room
PCABI_HD inline void elem_put(uint8_t *dst, int64_t room, const uint8_t *a, const Tag &t, int64_t k, const Floats &fl, int len) {
    if (room > 0) dst[0] = ',';
    if (t.sub == 'f') {
        uint8_t s[kFloatSlot];
        const int n = float_get(fl, k, a + t.val + 4 * k, s);
        for (int j = 0; j < n && 1 + j < room; ++j) dst[1 + j] = s[j];
        return;
    }
    dec_put(dst + 1, room - 1, int_at(a + t.val + k * t.w, t.sub), len - 1);
}

// byte k of a tag's head
PCABI_HD inline uint8_t head_byte(const uint8_t *tg, int k) {
    const uint8_t t = tg[2];
    return k == 0 ? (uint8_t)'\t' : k == 1 ? tg[0] : k == 2 ? tg[1] : k == 4 ? (is_int(t) ? (uint8_t)'i' : t) : (uint8_t)':';
}

// The byte-wise walk of one chain a[0, n) (the host build): the text's length, or -1 for a chain that
// does not walk. dst != nullptr: the text is written to dst[0, room) as well (nothing behind room).
// *written / *left_out count the tags (untouched at -1).
inline int64_t walk(const uint8_t *a, int64_t n, Floats fl, uint8_t *dst, int64_t room, int64_t *written, int64_t *left_out) {
    int64_t at = 0, len = 0, nw = 0, nl = 0;
    while (at < n) {
        Tag t = tag_at(a, n, at);
        if (!t.ok) return -1;
        bool good = name_ok(a + at);
        int64_t vlen = 0;
        if (t.type == 'Z' || t.type == 'H') {
            int64_t q = t.val;
            for (;; ++q) {
                const int c = zh_lane(a, n, q);
                if (c == 3) return -1;
                if (c == 1) break;
                if (c == 2) good = false;
            }
            vlen = q - t.val;
            t.next = q + 1;
        } else if (t.type == 'A') {
            good = good && printable(a[t.val]);
            vlen = 1;
        } else if (t.type == 'f') {
            uint8_t s[kFloatSlot];
            vlen = float_get(fl, 0, a + t.val, s);
        } else if (t.type == 'B') {
            vlen = 1;
            for (int64_t k = 0; k < t.count; ++k) vlen += elem_len(a, t, k, fl);
        } else {
            vlen = dec_len(int_at(a + t.val, t.type));
        }
        if (good && dst) {
            uint8_t *d = dst + len;
            const int64_t rm = room - len;
            for (int k = 0; k < kHead; ++k)
                if (k < rm) d[k] = head_byte(a + at, k);
            d += kHead;
            const int64_t r = rm - kHead;
            if (t.type == 'Z' || t.type == 'H' || t.type == 'A') {
                for (int64_t k = 0; k < vlen && k < r; ++k) d[k] = a[t.val + k];
            } else if (t.type == 'f') {
                uint8_t s[kFloatSlot];
                const int m = float_get(fl, 0, a + t.val, s);
                for (int k = 0; k < m && k < r; ++k) d[k] = s[k];
            } else if (t.type == 'B') {
                if (r > 0) d[0] = t.sub;
                int64_t w = 1;
                for (int64_t k = 0; k < t.count; ++k) {
                    const int el = elem_len(a, t, k, fl);
                    elem_put(d + w, r - w, a, t, k, fl, el);
                    w += el;
                }
            } else {
                dec_put(d, r, int_at(a + t.val, t.type), (int)vlen);
            }
        }
        if (t.type == 'f') fl.cur += 1;
        if (t.type == 'B' && t.sub == 'f') fl.cur += t.count;
        if (good) len += kHead + vlen, ++nw;
        else ++nl;
        at = t.next;
    }
    if (written) *written += nw;
    if (left_out) *left_out += nl;
    return len;
}

// how many float slots a chain needs (f tags and B:f elements, in walk order); -1 when it does not walk
inline int64_t float_count(const uint8_t *a, int64_t n) {
    int64_t at = 0, c = 0;
    while (at < n) {
        Tag t = tag_at(a, n, at);
        if (!t.ok) return -1;
        if (t.type == 'Z' || t.type == 'H') {
            const void *z = memchr(a + t.val, 0, (size_t)(n - t.val));
            if (!z) return -1;
            t.next = (int64_t)((const uint8_t *)z - a) + 1;
        }
        if (t.type == 'f') c += 1;
        if (t.type == 'B' && t.sub == 'f') c += t.count;
        at = t.next;
    }
    return c;
}
// the slots themselves, appended to *tab (the host, for a device build)
template <class Vec>
inline void float_fill(const uint8_t *a, int64_t n, Vec *tab) {
    int64_t at = 0;
    auto add = [&](const uint8_t *p) {
        char s[kFloatSlot];
        const int m = float_text(p, s);
        const size_t base = tab->size();
        tab->resize(base + kFloatSlot, 0);
        (*tab)[base] = (uint8_t)m;
        for (int j = 0; j < m; ++j) (*tab)[base + 1 + (size_t)j] = (uint8_t)s[j];
    };
    while (at < n) {
        Tag t = tag_at(a, n, at);
        if (!t.ok) return;
        if (t.type == 'Z' || t.type == 'H') {
            const void *z = memchr(a + t.val, 0, (size_t)(n - t.val));
            if (!z) return;
            t.next = (int64_t)((const uint8_t *)z - a) + 1;
        }
        if (t.type == 'f') add(a + t.val);
        if (t.type == 'B' && t.sub == 'f')
            for (int64_t k = 0; k < t.count; ++k) add(a + t.val + 4 * k);
        at = t.next;
    }
}

// a table entry against the blob
PCABI_HD inline bool part_fits(const pcabi_auxtext_part &p, int64_t aux_n) {
    return p.aux_len >= 0 && p.aux_off >= 0 && p.aux_off <= aux_n && p.aux_len <= aux_n - p.aux_off;
}

// ---- text records ----------------------------------------------------------------------------------
// FASTQ: '@' name tag-text '\n' bases '\n' '+' '\n' qualities '\n'. FASTA: '>' name tag-text '\n', then
// the bases in lines of 70, each followed by '\n'.

PCABI_HD inline int64_t text_len_of(const pcabi_fastx_part &p) { return p.text_len > 0 ? p.text_len : 0; }
PCABI_HD inline int64_t head_len(const pcabi_fastx_part &p) { return 1 + (int64_t)p.name_len + text_len_of(p) + 1; }
PCABI_HD inline int64_t fasta_seq_len(int64_t l_seq) { return l_seq + (l_seq + kFastaLine - 1) / kFastaLine; }
PCABI_HD inline int64_t record_len(const pcabi_fastx_part &p, bool fasta) {
    return head_len(p) + (fasta ? fasta_seq_len(p.l_seq) : (int64_t)p.l_seq + 3 + (int64_t)p.l_qual + 1);
}
PCABI_HD inline int64_t part_tiles(const pcabi_fastx_part &p) {
    const int64_t t = ((int64_t)p.l_seq + kTileBases - 1) / kTileBases;
    return t > 0 ? t : 1;
}
PCABI_HD inline bool fastx_fits(const pcabi_fastx_part &p, bool fasta, int64_t seq_n, int64_t qual_n, int64_t side_n, int64_t out_cap) {
    if (p.l_seq < 0 || p.l_qual < 0 || p.name_len < 0 || p.aux_len < 0 || p.seq_src < 0 || p.name_off < 0 || p.aux_off < 0 ||
        p.out < 0 || p.tile0 < 0 || p.text_len < -1)
        return false;
    if (p.l_seq > seq_n - p.seq_src) return false;
    if (!fasta && p.l_qual > 0 && (p.qual_src < 0 || p.l_qual > qual_n - p.qual_src)) return false;
    if (p.name_len > side_n - p.name_off || p.aux_len > side_n - p.aux_off) return false;
    return record_len(p, fasta) <= out_cap - p.out;
}

PCABI_HD inline uint8_t base_out(uint8_t c, bool rna) { return rna && c == 'T' ? (uint8_t)'U' : c; }
// byte j of a FASTA record's sequence lines
PCABI_HD inline uint8_t fasta_byte(const uint8_t *src, int64_t l_seq, int64_t j, bool rna) {
    const int64_t line = j / (kFastaLine + 1), col = j % (kFastaLine + 1), b = line * kFastaLine + col;
    return col == kFastaLine || b >= l_seq ? (uint8_t)'\n' : base_out(src[b], rna);
}
PCABI_HD inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// The bytes dst[j0, j1) of a run that copies src (rna: T as U) or holds FASTA lines of src[0, l_seq):
// single bytes up to the first 16-aligned destination that still has 16 bytes to go, then sixteen at a
// time (an unaligned load, an aligned store), then single bytes.
PCABI_HD inline void copy_range(uint8_t *dst, const uint8_t *src, int64_t l_seq, int64_t j0, int64_t j1, bool rna, bool lines) {
    int64_t j = j0;
    auto one = [&](int64_t k) { return lines ? fasta_byte(src, l_seq, k, rna) : base_out(src[k], rna); };
    for (; j < j1 && !(aligned16(dst + j) && j + 16 <= j1); ++j) dst[j] = one(j);
    for (; j + 16 <= j1; j += 16) {
        uint8_t v[16];
        if (lines) {
            for (int k = 0; k < 16; ++k) v[k] = fasta_byte(src, l_seq, j + k, rna);
        } else {
            memcpy(v, src + j, 16);
            if (rna)
                for (int k = 0; k < 16; ++k) v[k] = base_out(v[k], true);
        }
        memcpy(__builtin_assume_aligned(dst + j, 16), v, 16);
    }
    for (; j < j1; ++j) dst[j] = one(j);
}

// A tile's share [b0, b1) of a part's bases (and, FASTQ, of its qualities), dealt to the lanes in
// pieces of the destination's 16-byte grid. rec = the record's first byte.
PCABI_HD inline void pack_tile(const pcabi_fastx_part &p, bool fasta, const uint8_t *seq, const uint8_t *qual, uint8_t *rec, int64_t b0,
                               int64_t b1, int lane, int n_lanes) {
    const bool rna = (p.flags & PCABI_FASTX_RNA) != 0;
    const uint8_t *src = seq + p.seq_src;
    uint8_t *sq = rec + head_len(p);
    // destination bytes [y0, y1) of the sequence
    const int64_t y0 = fasta ? b0 + b0 / kFastaLine : b0;
    const int64_t y1 = fasta ? (b1 >= p.l_seq ? fasta_seq_len(p.l_seq) : b1 + b1 / kFastaLine) : b1;
    {
        const int64_t d = (int64_t)(uintptr_t)sq, a = (d + y0) & ~(int64_t)15, pieces = (d + y1 - a + 15) >> 4;
        for (int64_t k = lane; k < pieces; k += n_lanes) {
            const int64_t q0 = a + 16 * k - d, c0 = q0 > y0 ? q0 : y0, c1 = q0 + 16 < y1 ? q0 + 16 : y1;
            copy_range(sq, src, p.l_seq, c0, c1, rna, fasta);
        }
    }
    if (fasta) return;
    // qualities [b0, b1) of [0, l_qual), scaled to the tile: the tiles cut l_qual where they cut l_seq
    const int64_t g0 = b0 < p.l_qual ? b0 : p.l_qual, g1 = b1 >= p.l_seq ? p.l_qual : (b1 < p.l_qual ? b1 : p.l_qual);
    if (g0 >= g1) return;
    uint8_t *ql = sq + p.l_seq + 3;
    const uint8_t *qs = qual + p.qual_src;
    const int64_t d = (int64_t)(uintptr_t)ql, a = (d + g0) & ~(int64_t)15, pieces = (d + g1 - a + 15) >> 4;
    for (int64_t k = lane; k < pieces; k += n_lanes) {
        const int64_t q0 = a + 16 * k - d, c0 = q0 > g0 ? q0 : g0, c1 = q0 + 16 < g1 ? q0 + 16 : g1;
        copy_range(ql, qs, p.l_qual, c0, c1, false, false);
    }
}

// What a record holds besides its tag text, bases and qualities: '@' / '>', the name, the line feeds
// and '+', as byte copies k = first, first + step, ...
PCABI_HD inline void pack_fixed(const pcabi_fastx_part &p, bool fasta, const uint8_t *side, uint8_t *rec, int64_t first, int64_t step) {
    const uint8_t *nm = side + p.name_off;
    for (int64_t k = first; k < p.name_len; k += step) rec[1 + k] = nm[k];
    if (first != 0) return;
    rec[0] = fasta ? '>' : '@';
    const int64_t h = head_len(p);
    rec[h - 1] = '\n';
    if (fasta) return;
    uint8_t *e = rec + h + p.l_seq;
    e[0] = '\n', e[1] = '+', e[2] = '\n';
    e[3 + p.l_qual] = '\n';
}

// One whole part (the host build): its tag text by the byte-wise walk.
inline void pack_part(const pcabi_fastx_part &p, bool fasta, const uint8_t *seq, const uint8_t *qual, const uint8_t *side, uint8_t *out) {
    uint8_t *rec = out + p.out;
    pack_fixed(p, fasta, side, rec, 0, 1);
    if (p.text_len > 0) walk(side + p.aux_off, p.aux_len, Floats{nullptr, 0, 0}, rec + 1 + p.name_len, p.text_len, nullptr, nullptr);
    pack_tile(p, fasta, seq, qual, rec, 0, p.l_seq, 0, 1);
}

// Output offsets and tiles of the next part.
struct FastxLayout {
    int64_t out = 0, tiles = 0;
    bool fasta = false;
    void place(pcabi_fastx_part *p) {
        p->out = out;
        p->tile0 = tiles;
        out += record_len(*p, fasta);
        tiles += part_tiles(*p);
    }
};

}  // namespace pcabi_auxtext
