// pcabi_bam.h -- the record layer of unaligned BAM input and output (pcabi_bam.hip, pcabi_io.cpp, pcabi_write.cpp; the
// pack half for output is at the end of the file). Input: the header
// skip, the record walk and the unpack of one record's bases into the reader's batch layout (sequence
// letters, qualities, Dna5 codes). Nothing here is device-only: the kernel (k_bam_unpack), the host
// reader and the CPU tests (tests/bam_fuzz_main.cpp builds it alone) run the same code.
//
// Format (SAM/BAM specification 4.2): after the BGZF layer a BAM file is "BAM\1", l_text, the text,
// n_ref and per reference l_name, name, l_ref; then records chained by a length prefix:
//   block_size i32 | refID i32 | pos i32 | l_read_name u8 | mapq u8 | bin u16 | n_cigar_op u16 |
//   flag u16 | l_seq i32 | next_refID i32 | next_pos i32 | tlen i32 | read_name (NUL-terminated) |
//   cigar u32[n_cigar_op] | seq u8[(l_seq + 1) / 2] | qual u8[l_seq] | aux tags
// A sequence byte holds two bases as 4-bit codes over "=ACMGRSVTWYHKDBN", the earlier base in the
// high nibble. All integers are little-endian.
//
// Rules (what samtools fastq writes, in the project's batch layout):
//   * secondary (0x100) and supplementary (0x800) records are skipped;
//   * a reverse-strand record (0x10) is reverse-complemented (A/T, C/G, M/K, R/Y, V/B, H/D; =, S, W, N
//     map to themselves: the complement of a code is its four bits reversed) and its qualities are
//     reversed;
//   * name = read_name without its NUL (l_read_name - 1 bytes); qualities q + 33 (mod 256); a first
//     quality byte of 0xFF (qualities absent) gives '+' for every base; Dna5 code 0..3 for A, C, G, T,
//     4 for anything else; codes are padded with 4 to the next multiple of four bases.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/pcabi.h"

#ifndef PCABI_HD
#if defined(__HIPCC__)
#define PCABI_HD __host__ __device__
#else
#define PCABI_HD
#endif
#endif

#if defined(__clang__)
#define PCABI_BAM_UNROLL _Pragma("unroll")
#else
#define PCABI_BAM_UNROLL
#endif

namespace pcabi_bam {

constexpr int kFixed = 32;          // bytes of a record's fixed fields (after block_size)
constexpr int kTileBases = 16384;   // bases per workgroup of k_bam_unpack
constexpr int kSkipFlags = 0x100 | 0x800;
constexpr int kReverse = 0x10;

PCABI_HD inline uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
PCABI_HD inline int32_t le32(const uint8_t *p) {
    return (int32_t)((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
}

// The header's length when b[0, n) holds it whole; 0 when more bytes are needed; -1 when it is not a
// BAM header (the magic, or a negative length).
PCABI_HD inline int64_t header_len(const uint8_t *b, int64_t n) {
    if (n < 4) return 0;
    if (b[0] != 'B' || b[1] != 'A' || b[2] != 'M' || b[3] != 1) return -1;
    if (n < 8) return 0;
    const int64_t l_text = le32(b + 4);
    if (l_text < 0) return -1;
    int64_t at = 8 + l_text;
    if (n < at + 4) return 0;
    const int64_t n_ref = le32(b + at);
    if (n_ref < 0) return -1;
    at += 4;
    for (int64_t r = 0; r < n_ref; ++r) {
        if (n < at + 4) return 0;
        const int64_t l_name = le32(b + at);
        if (l_name < 0) return -1;
        at += 4 + l_name + 4;
        if (n < at) return 0;
    }
    return at;
}

// The record at b[at, n): 1 and *r filled (offsets and tile0 left 0) when it is valid and whole, 0 when
// more bytes are needed, -1 when it is invalid. *size = 4 + block_size when 1 is returned.
PCABI_HD inline int record_at(const uint8_t *b, int64_t n, int64_t at, pcabi_bam_rec *r, int64_t *size) {
    if (n - at < 4) return 0;
    const int64_t block = le32(b + at);
    if (block < kFixed) return -1;
    if (n - at < 4 + kFixed) return 0;
    const uint8_t *f = b + at + 4;
    const int64_t l_name = f[8], n_cigar = le16(f + 12), l_seq = le32(f + 16);
    if (l_name < 1 || l_seq < 0) return -1;
    const int64_t seq_at = 4 + kFixed + l_name + 4 * n_cigar;
    if (seq_at - 4 + (l_seq + 1) / 2 + l_seq > block) return -1;
    if (n - at < 4 + block) return 0;
    r->rec = at;
    r->seq_out = r->qual_out = r->code_out = r->tile0 = 0;
    r->seq_at = (int32_t)seq_at;
    r->l_seq = (int32_t)l_seq;
    r->flag = (int32_t)le16(f + 14);
    r->name_len = (int32_t)l_name - 1;
    *size = 4 + block;
    return 1;
}

// Output offsets of the next record in the batch layout: sequence and qualities back to back, codes at
// 4-aligned starts; tile0 counts k_bam_unpack's tiles.
struct Layout {
    int64_t seq = 0, code = 0, tiles = 0, names = 0;
    PCABI_HD void place(pcabi_bam_rec *r) {
        r->seq_out = r->qual_out = seq;
        r->code_out = code;
        r->tile0 = tiles;
        seq += r->l_seq;
        code += ((int64_t)r->l_seq + 3) & ~(int64_t)3;
        tiles += ((int64_t)r->l_seq + kTileBases - 1) / kTileBases;
        names += r->name_len;
    }
};

// Records of b[at, n) from record to record: those that are kept (not secondary / supplementary) go to
// recs[0, cap) with their offsets placed by *lay; all are counted. Returns the count of kept records,
// -1 at an invalid record. *stop = the first byte not consumed (an incomplete record's start, the
// invalid record's start, or n).
inline int64_t walk(const uint8_t *b, int64_t n, int64_t at, pcabi_bam_rec *recs, int64_t cap, Layout *lay,
                    int64_t *stop) {
    int64_t kept = 0;
    for (;;) {
        pcabi_bam_rec r;
        int64_t size = 0;
        const int rc = record_at(b, n, at, &r, &size);
        if (rc <= 0) {
            *stop = at;
            return rc < 0 ? -1 : kept;
        }
        at += size;
        if (r.flag & kSkipFlags) continue;
        lay->place(&r);
        if (kept < cap) recs[kept] = r;
        ++kept;
    }
}

// ---- unpack ------------------------------------------------------------------------------------

// 16-entry tables held in registers: letters (8 bytes each), complements and Dna5 codes (a nibble each)
constexpr uint64_t kLettersLo = 0x565352474D43413Dull;   // = A C M G R S V
constexpr uint64_t kLettersHi = 0x4E42444B48595754ull;   // T W Y H K D B N
constexpr uint64_t kComp = 0xF7B3D591E6A2C480ull;
constexpr uint64_t kDna5 = 0x4444444344424104ull;

PCABI_HD inline uint32_t letter_of(uint32_t c) { return (uint32_t)((c & 8 ? kLettersHi : kLettersLo) >> ((c & 7) * 8)) & 0xffu; }
PCABI_HD inline uint32_t comp_of(uint32_t c) { return (uint32_t)(kComp >> (c * 4)) & 15u; }
PCABI_HD inline uint32_t dna5_of(uint32_t c) { return (uint32_t)(kDna5 >> (c * 4)) & 15u; }
PCABI_HD inline uint32_t nibble_at(const uint8_t *sq, int64_t i) { return (i & 1) ? (sq[i >> 1] & 15u) : (uint32_t)(sq[i >> 1] >> 4); }
// the code of output base p
PCABI_HD inline uint32_t base_at(const uint8_t *sq, int64_t l_seq, bool rev, int64_t p) {
    return rev ? comp_of(nibble_at(sq, l_seq - 1 - p)) : nibble_at(sq, p);
}

PCABI_HD inline uint64_t bswap64(uint64_t x) { return __builtin_bswap64(x); }
PCABI_HD inline void store16(uint8_t *dst, const uint8_t *v) { memcpy(__builtin_assume_aligned(dst, 16), v, 16); }
PCABI_HD inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// The 16 codes of output bases [p, p + 16) (all inside the read) as nibbles of one word: output base
// p + k at bits 60 - 4k (forward) or 4k (reverse, not yet complemented). One unaligned 8-byte load, and
// the ninth byte when the run starts on a low nibble.
PCABI_HD inline uint64_t codes16(const uint8_t *sq, int64_t l_seq, bool rev, int64_t p) {
    const int64_t lo = rev ? l_seq - 16 - p : p;
    const uint8_t *s = sq + (lo >> 1);
    uint64_t w;
    memcpy(&w, s, 8);
    w = bswap64(w);
    return (lo & 1) ? (w << 4 | (uint64_t)(s[8] >> 4)) : w;
}

// Output bases [b0, b1) of one record: sq = its sequence bytes (the qualities follow them), seq / qual /
// codes = where the record's base 0 goes in each output, or nullptr to leave that output alone. Stores
// are 16 bytes wide where the destination is 16-aligned and the range covers them, single bytes at the
// ragged ends; nothing outside [b0, b1) is written, except the codes' padding up to the next multiple
// of four when b1 == l_seq.
PCABI_HD inline void unpack_range(const uint8_t *sq, int32_t l_seq32, int32_t flags, int64_t b0, int64_t b1,
                                  uint8_t *seq, uint8_t *qual, uint8_t *codes) {
    const int64_t l_seq = l_seq32;
    const bool rev = (flags & kReverse) != 0;
    const uint8_t *ql = sq + (l_seq + 1) / 2;
    if (b1 > l_seq) b1 = l_seq;
    if (b0 < 0) b0 = 0;
    if (seq) {
        int64_t p = b0;
        for (; p < b1 && !(aligned16(seq + p) && p + 16 <= b1); ++p) seq[p] = (uint8_t)letter_of(base_at(sq, l_seq, rev, p));
        for (; p + 16 <= b1; p += 16) {
            const uint64_t w = codes16(sq, l_seq, rev, p);
            uint8_t v[16];
            if (rev) {
PCABI_BAM_UNROLL
                for (int k = 0; k < 16; ++k) v[k] = (uint8_t)letter_of(comp_of((uint32_t)(w >> (4 * k)) & 15u));
            } else {
PCABI_BAM_UNROLL
                for (int k = 0; k < 16; ++k) v[k] = (uint8_t)letter_of((uint32_t)(w >> (60 - 4 * k)) & 15u);
            }
            store16(seq + p, v);
        }
        for (; p < b1; ++p) seq[p] = (uint8_t)letter_of(base_at(sq, l_seq, rev, p));
    }
    if (codes) {
        int64_t p = b0;
        for (; p < b1 && !(aligned16(codes + p) && p + 16 <= b1); ++p) codes[p] = (uint8_t)dna5_of(base_at(sq, l_seq, rev, p));
        for (; p + 16 <= b1; p += 16) {
            const uint64_t w = codes16(sq, l_seq, rev, p);
            uint8_t v[16];
            if (rev) {
PCABI_BAM_UNROLL
                for (int k = 0; k < 16; ++k) v[k] = (uint8_t)dna5_of(comp_of((uint32_t)(w >> (4 * k)) & 15u));
            } else {
PCABI_BAM_UNROLL
                for (int k = 0; k < 16; ++k) v[k] = (uint8_t)dna5_of((uint32_t)(w >> (60 - 4 * k)) & 15u);
            }
            store16(codes + p, v);
        }
        for (; p < b1; ++p) codes[p] = (uint8_t)dna5_of(base_at(sq, l_seq, rev, p));
        if (b1 == l_seq && b0 <= b1)
            for (int64_t q = l_seq; q < ((l_seq + 3) & ~(int64_t)3); ++q) codes[q] = 4;
    }
    if (qual && b0 < b1) {
        const bool absent = ql[0] == 0xff;
        int64_t p = b0;
        for (; p < b1 && !(aligned16(qual + p) && p + 16 <= b1); ++p)
            qual[p] = absent ? (uint8_t)'+' : (uint8_t)(ql[rev ? l_seq - 1 - p : p] + 33u);
        for (; p + 16 <= b1; p += 16) {
            uint8_t q[16], v[16];
            if (absent) {
PCABI_BAM_UNROLL
                for (int k = 0; k < 16; ++k) v[k] = (uint8_t)'+';
            } else if (rev) {
                memcpy(q, ql + (l_seq - 16 - p), 16);
PCABI_BAM_UNROLL
                for (int k = 0; k < 16; ++k) v[k] = (uint8_t)(q[15 - k] + 33u);
            } else {
                memcpy(q, ql + p, 16);
PCABI_BAM_UNROLL
                for (int k = 0; k < 16; ++k) v[k] = (uint8_t)(q[k] + 33u);
            }
            store16(qual + p, v);
        }
        for (; p < b1; ++p) qual[p] = absent ? (uint8_t)'+' : (uint8_t)(ql[rev ? l_seq - 1 - p : p] + 33u);
    }
}

// A table entry against the buffers it names: the record's sequence and qualities inside bam[0, n), its
// outputs inside their capacities.
PCABI_HD inline bool rec_fits(const pcabi_bam_rec &r, int64_t n, int64_t seq_cap, int64_t qual_cap, int64_t codes_cap) {
    const int64_t l = r.l_seq;
    if (l < 0 || r.rec < 0 || r.seq_at < 0 || r.seq_out < 0 || r.qual_out < 0 || r.code_out < 0) return false;
    if (r.rec > n || r.seq_at > n - r.rec || (l + 1) / 2 + l > n - r.rec - r.seq_at) return false;
    return l <= seq_cap - r.seq_out && l <= qual_cap - r.qual_out && ((l + 3) & ~(int64_t)3) <= codes_cap - r.code_out;
}

// ---- pack (BAM output) ---------------------------------------------------------------------------
// The inverse of the unpack: parts of a batch (include/pcabi.h pcabi_bam_part) laid out as a chain of
// unmapped records. The kernel (k_bam_pack), the host writer and the CPU tests
// (tests/bam_pack_fuzz_main.cpp builds it alone) run the same code.

constexpr int kMaxName = 254;   // l_read_name is a byte and counts the NUL

PCABI_HD inline int64_t part_size(const pcabi_bam_part &p) {
    return 4 + kFixed + ((int64_t)p.name_len + 1) + ((int64_t)p.l_seq + 1) / 2 + (int64_t)p.l_seq + (int64_t)p.aux_len;
}
PCABI_HD inline int64_t part_tiles(const pcabi_bam_part &p) {
    const int64_t t = ((int64_t)p.l_seq + kTileBases - 1) / kTileBases;
    return t > 0 ? t : 1;   // a record without bases still has a header to write
}
// where a part's packed sequence starts, from the record's start
PCABI_HD inline int64_t part_seq_at(const pcabi_bam_part &p) { return 4 + kFixed + (int64_t)p.name_len + 1; }

// Output offsets and tiles of the next part of the chain.
struct PackLayout {
    int64_t out = 0, tiles = 0;
    PCABI_HD void place(pcabi_bam_part *p) {
        p->out = out;
        p->tile0 = tiles;
        out += part_size(*p);
        tiles += part_tiles(*p);
    }
};

// Letter -> code over "=ACMGRSVTWYHKDBN" (U -> T, anything else -> N): a nibble per letter of 'A'..'P'
// and 'Q'..'`' in two registers.
constexpr uint64_t kCodeAP = 0xFFF3FCFFB4FFD2E1ull;
constexpr uint64_t kCodeQ = 0xFFFFFFFAF978865Full;
PCABI_HD inline uint32_t code_of(uint32_t c) {
    const uint32_t u = c - 65u;
    if (u < 16u) return (uint32_t)(kCodeAP >> (4 * u)) & 15u;
    if (u < 32u) return (uint32_t)(kCodeQ >> (4 * (u - 16u))) & 15u;
    return c == '=' ? 0u : 15u;
}
PCABI_HD inline uint8_t phred_of(uint32_t c) { return (uint8_t)(c < 33u ? 0u : c > 126u ? 93u : c - 33u); }

// Output bases [b0, b1) of one part: src / qsrc = its letters and quality characters (qsrc nullptr:
// absent, 0xFF), l_seq its length, sq / ql = where the record's packed sequence and its qualities
// start, or nullptr to leave that output alone. With sq, b0 is even (tile and piece edges fall on even
// base counts, so no packed byte has two writers; an odd b0 writes no sequence byte). Stores are 16 bytes wide where the destination is
// 16-aligned and the range covers them, single bytes at the ragged ends; nothing outside the range's
// own packed-sequence bytes [b0 / 2, (b1 + 1) / 2) and quality bytes [b0, b1) is written.
PCABI_HD inline void pack_range(const uint8_t *src, const uint8_t *qsrc, int32_t l_seq32, int64_t b0, int64_t b1,
                                uint8_t *sq, uint8_t *ql) {
    const int64_t l_seq = l_seq32;
    if (b1 > l_seq) b1 = l_seq;
    if (b0 < 0) b0 = 0;
    if (b0 >= b1) return;
    if (sq && !(b0 & 1)) {
        const int64_t e = (b1 + 1) / 2;   // bytes [p, e)
        auto byte_at = [&](int64_t p) {
            const uint32_t hi = code_of(src[2 * p]), lo = 2 * p + 1 < l_seq ? code_of(src[2 * p + 1]) : 0u;
            return (uint8_t)(hi << 4 | lo);
        };
        int64_t p = b0 / 2;
        for (; p < e && !(aligned16(sq + p) && 2 * (p + 16) <= b1); ++p) sq[p] = byte_at(p);
        for (; 2 * (p + 16) <= b1; p += 16) {
            uint8_t c[32], v[16];
            memcpy(c, src + 2 * p, 32);
PCABI_BAM_UNROLL
            for (int k = 0; k < 16; ++k) v[k] = (uint8_t)(code_of(c[2 * k]) << 4 | code_of(c[2 * k + 1]));
            store16(sq + p, v);
        }
        for (; p < e; ++p) sq[p] = byte_at(p);
    }
    if (ql) {
        int64_t p = b0;
        for (; p < b1 && !(aligned16(ql + p) && p + 16 <= b1); ++p) ql[p] = qsrc ? phred_of(qsrc[p]) : (uint8_t)0xff;
        for (; p + 16 <= b1; p += 16) {
            uint8_t q[16], v[16];
            if (qsrc) {
                memcpy(q, qsrc + p, 16);
PCABI_BAM_UNROLL
                for (int k = 0; k < 16; ++k) v[k] = phred_of(q[k]);
            } else {
PCABI_BAM_UNROLL
                for (int k = 0; k < 16; ++k) v[k] = 0xff;
            }
            store16(ql + p, v);
        }
        for (; p < b1; ++p) ql[p] = qsrc ? phred_of(qsrc[p]) : (uint8_t)0xff;
    }
}

// Byte k of a record's block_size and fixed fields (k in [0, 36)).
PCABI_HD inline uint8_t head_byte(const pcabi_bam_part &p, int k) {
    const uint32_t block = (uint32_t)(part_size(p) - 4), l = (uint32_t)p.l_seq;
    if (k < 4) return (uint8_t)(block >> (8 * k));
    if (k < 12) return 0xff;                                   // refID, pos = -1
    if (k == 12) return (uint8_t)(p.name_len + 1);             // l_read_name
    if (k == 13) return 0;                                     // mapq
    if (k < 16) return (uint8_t)(4680u >> (8 * (k - 14)));     // bin
    if (k < 18) return 0;                                      // n_cigar_op
    if (k < 20) return (uint8_t)(4u >> (8 * (k - 18)));        // flag: unmapped
    if (k < 24) return (uint8_t)(l >> (8 * (k - 20)));         // l_seq
    if (k < 32) return 0xff;                                   // next_refID, next_pos = -1
    return 0;                                                  // tlen
}

// Everything of a record but its bases: block_size, fixed fields, name, NUL and the aux bytes, as byte
// copies k = first, first + step, ... (the kernel strides them over the lanes; the host passes 0, 1).
PCABI_HD inline void pack_head(const pcabi_bam_part &p, const uint8_t *side, uint8_t *rec, int64_t first, int64_t step) {
    const int64_t head = 4 + kFixed, nm = p.name_len, aux_at = part_seq_at(p) + ((int64_t)p.l_seq + 1) / 2 + p.l_seq;
    const uint8_t *s = side + p.side_off;
    for (int64_t k = first; k < head; k += step) rec[k] = head_byte(p, (int)k);
    for (int64_t k = first; k <= nm; k += step) rec[head + k] = k < nm ? s[k] : (uint8_t)0;
    for (int64_t k = first; k < p.aux_len; k += step) rec[aux_at + k] = s[nm + k];
}

// One whole part (the host build): seq / qual / side / out are the buffers' starts.
inline void pack_part(const pcabi_bam_part &p, const uint8_t *seq, const uint8_t *qual, const uint8_t *side, uint8_t *out) {
    uint8_t *rec = out + p.out, *sq = rec + part_seq_at(p);
    pack_head(p, side, rec, 0, 1);
    pack_range(seq + p.seq_src, p.qual_src >= 0 ? qual + p.qual_src : nullptr, p.l_seq, 0, p.l_seq, sq,
               sq + ((int64_t)p.l_seq + 1) / 2);
}

// A part against the buffers it names.
PCABI_HD inline bool part_fits(const pcabi_bam_part &p, int64_t seq_n, int64_t qual_n, int64_t side_n, int64_t out_cap) {
    const int64_t l = p.l_seq;
    if (l < 0 || p.name_len < 0 || p.name_len > kMaxName || p.aux_len < 0 || p.seq_src < 0 || p.side_off < 0 || p.out < 0 ||
        p.tile0 < 0)
        return false;
    if (l > seq_n - p.seq_src || (p.qual_src >= 0 && l > qual_n - p.qual_src)) return false;
    if ((int64_t)p.name_len + p.aux_len > side_n - p.side_off) return false;
    return part_size(p) <= out_cap - p.out;
}

// The tag at a[at, n) of an aux chain: the offset behind it, or -1 when its type is not one of
// A c C s S i I f Z H B or it runs past n.
PCABI_HD inline int64_t aux_next(const uint8_t *a, int64_t n, int64_t at) {
    if (at < 0 || n - at < 3) return -1;
    auto width = [](uint8_t t) { return t == 'c' || t == 'C' ? 1 : t == 's' || t == 'S' ? 2 : t == 'i' || t == 'I' || t == 'f' ? 4 : 0; };
    const uint8_t t = a[at + 2];
    int64_t q = at + 3;
    if (t == 'A') return n - q >= 1 ? q + 1 : -1;
    if (width(t)) return n - q >= width(t) ? q + width(t) : -1;
    if (t == 'Z' || t == 'H') {
        for (; q < n; ++q)
            if (a[q] == 0) return q + 1;
        return -1;
    }
    if (t == 'B') {
        if (n - q < 5 || !width(a[q])) return -1;
        const int64_t count = (uint32_t)le32(a + q + 1), bytes = count * width(a[q]);
        return bytes <= n - q - 5 ? q + 5 + bytes : -1;
    }
    return -1;
}
// Whether a[0, n) is a chain of whole tags.
PCABI_HD inline bool aux_walks(const uint8_t *a, int64_t n) {
    int64_t at = 0;
    while (at < n) {
        at = aux_next(a, n, at);
        if (at < 0) return false;
    }
    return true;
}
// Tags whose values count bases of the stored sequence: dropped from a read that was changed.
PCABI_HD inline bool aux_positional(const uint8_t *tag) {
    return (tag[0] == 'M' && (tag[1] == 'M' || tag[1] == 'L' || tag[1] == 'N' || tag[1] == 'm' || tag[1] == 'l')) ||
           (tag[0] == 'm' && tag[1] == 'v');
}

}  // namespace pcabi_bam
