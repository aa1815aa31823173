// pcabi_bam.h -- the record layer of unaligned BAM input (pcabi_bam.hip, pcabi_io.cpp): the header
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

}  // namespace pcabi_bam
