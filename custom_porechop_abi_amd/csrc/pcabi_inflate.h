// pcabi_inflate.h -- the parts of the gzip decoder (pcabi_inflate.hip) that hold no device-only
// construct: a bit reader bounded to one member's bytes, block header parsing, code-length decoding,
// decode-table construction, the symbol loop, the gzip member frame and the BGZF member index.
// Everything compiles as plain C++ too (tests/inflate_cpu.cpp builds a helper from it), so the code
// the kernel runs is checkable without a GPU.
//
// Format: RFC 1951 in full (stored, fixed and dynamic blocks, any number per member, matches of
// 3..258 bytes at distances 1..32768) inside one RFC 1952 member whose decoded bytes are at most
// `cap` (65536 for a BGZF member). Two policies make the same code serial on the host and wave-wide
// on the device:
//   Par   lane() / lanes() / sync(): table construction strides its loops by lanes(); one lane does
//         the serial bookkeeping; sync() separates the phases (a no-op on the host);
//   Sink  put(pos, byte) / copy(pos, dist, len) / store(pos, src, len) / crc(len): where decoded
//         bytes go. Every lane runs the symbol loop on the same (uniform) values. A sink may say
//         with history() how much lies before its position 0 (0 or 32768; none when it has no such
//         member): the sinks of a decoder that starts inside a stream (pcabi_gzstream.h).
// The block loop (inflate_blocks) starts at any bit, stops at a block boundary a stop rule picks and
// reports where it stopped; inflate_raw is that loop from bit 0 to the final block.
// Decode tables: a primary lookup (10 bits literal/length, 9 bits distance, 7 bits code lengths)
// whose entries for longer codes point at second-level tables of 2^(longest code below - root)
// entries. The sizes below always suffice: a second-level table of 2^k entries is full (incomplete
// codes are refused) and so holds at least k + 1 symbols, that is at most 2^k / (k + 1) entries per
// symbol, which grows with k. Literal/length (k <= 5): at most 286 * 32 / 6 = 1525 <= 1536 entries.
// Distance (k <= 6): were 29 or 30 of the 30 symbols in second-level tables, the one short code left
// would cover at most half of the 512 primary prefixes and each of the other 256 would need a table
// of its own with two symbols or more; so at most 28 are, and 28 * 64 / 7 = 256 entries.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/pcabi.h"
#include "pcabi_deflate.h"   // PCABI_HD

#if defined(__HIPCC__)
#define PCABI_INL __attribute__((always_inline))   // the symbol loop and the header parsing: one body
#define PCABI_NOINL __attribute__((noinline))      // the table builder: a call, so that its registers are
#else                                              // not live across the symbol loop (no spills, no scratch)
#define PCABI_INL
#define PCABI_NOINL inline
#endif

namespace pcabi_inflate {

constexpr int kLitRoot = 10, kDistRoot = 9, kClRoot = 7;
constexpr int kLitTable = 1024 + 1536, kDistTable = 512 + 256, kClTable = 128;
constexpr int kMaxLit = 288, kMaxDist = 32, kMaxBits = 15;
constexpr int kMemberMax = 65536;    // decoded bytes of one member on the device
constexpr int kMinMember = 18;       // 10 header + 8 trailer

// table entry: bits 0..3 code bits to drop (0 = no such code), 4..6 type, 8..11 extra bits (second
// level: its index bits), 16..31 value (literal, base length, base distance, second-level offset)
enum { T_LIT = 1, T_LEN = 2, T_EOB = 3, T_SUB = 4, T_BAD = 5, T_DIST = 6, T_CL = 7 };
enum { K_LIT = 0, K_DIST = 1, K_CL = 2 };

PCABI_HD PCABI_INL inline uint32_t entry(uint32_t nbits, uint32_t type, uint32_t extra, uint32_t val) {
    return nbits | type << 4 | extra << 8 | val << 16;
}
PCABI_HD PCABI_INL inline uint32_t e_bits(uint32_t e) { return e & 15u; }
PCABI_HD PCABI_INL inline uint32_t e_type(uint32_t e) { return (e >> 4) & 7u; }
PCABI_HD PCABI_INL inline uint32_t e_extra(uint32_t e) { return (e >> 8) & 15u; }
PCABI_HD PCABI_INL inline uint32_t e_val(uint32_t e) { return e >> 16; }

struct Tables {
    uint32_t lit[kLitTable];
    uint32_t dist[kDistTable];
    uint32_t cl[kClTable];
    uint16_t code[kMaxLit + kMaxDist];   // canonical code of every symbol of the table being built
    uint8_t len[kMaxLit + kMaxDist];     // literal/length lengths, then the distance lengths
    uint16_t count[kMaxBits + 1];
    uint16_t first[kMaxBits + 1];
    int32_t err;
    int32_t fixed_built;                 // lit / dist hold the fixed code's tables
};

// what symbol s of a code decodes to, as a table entry that drops nbits
PCABI_HD PCABI_INL inline uint32_t sym_entry(int kind, int s, uint32_t nbits) {
    if (kind == K_CL) return entry(nbits, T_CL, 0, (uint32_t)s);
    if (kind == K_DIST) {
        if (s >= 30) return entry(nbits, T_BAD, 0, 0);
        if (s < 4) return entry(nbits, T_DIST, 0, 1u + (uint32_t)s);
        const uint32_t x = (uint32_t)(s - 2) >> 1;
        return entry(nbits, T_DIST, x, 1u + ((2u + ((uint32_t)s & 1u)) << x));
    }
    if (s < 256) return entry(nbits, T_LIT, 0, (uint32_t)s);
    if (s == 256) return entry(nbits, T_EOB, 0, 0);
    if (s >= 286) return entry(nbits, T_BAD, 0, 0);
    if (s == 285) return entry(nbits, T_LEN, 0, 258);
    const uint32_t i = (uint32_t)(s - 257);
    if (i < 8) return entry(nbits, T_LEN, 0, 3u + i);
    const uint32_t x = (i - 4) >> 2;
    return entry(nbits, T_LEN, x, 3u + ((4u + (i & 3u)) << x));
}

PCABI_HD PCABI_INL inline uint32_t rev_bits(uint32_t v, int n) {
    uint32_t r = 0;
    for (int i = 0; i < n; ++i) r |= ((v >> i) & 1u) << (n - 1 - i);
    return r;
}

// The decode table of the code with lengths len[0, nsym) (0 = unused, <= 15): table[0, 1 << root)
// primary, second-level tables after it, cap entries in all. Refuses (PCABI_INFLATE_E_CODE) an
// over-subscribed code and an incomplete one, except that a distance code may have no code at all
// or one single code of length 1. Returns the same status on every lane.
template <class Par>
PCABI_HD PCABI_NOINL int build_table(Par &par, Tables &t, const uint8_t *len, int nsym, int root, uint32_t *table, int cap,
                                int kind) {
    const int lane = par.lane(), nl = par.lanes();
    for (int i = lane; i < (1 << root); i += nl) table[i] = 0;
    par.sync();
    if (lane == 0) {
        int err = 0;
        for (int l = 0; l <= kMaxBits; ++l) t.count[l] = 0;
        for (int s = 0; s < nsym; ++s) ++t.count[len[s]];
        const int used = nsym - t.count[0];
        int left = 1;
        for (int l = 1; l <= kMaxBits && left >= 0; ++l) left = 2 * left - t.count[l];
        if (left < 0) err = PCABI_INFLATE_E_CODE;
        else if (left > 0 && !(kind == K_DIST && (used == 0 || (used == 1 && t.count[1] == 1))))
            err = PCABI_INFLATE_E_CODE;
        if (!err) {
            uint32_t code = 0;
            t.first[0] = 0;
            for (int l = 1; l <= kMaxBits; ++l) {
                code = (code + (l > 1 ? t.count[l - 1] : 0u)) << 1;
                t.first[l] = (uint16_t)code;   // < 2^l
            }
            // second-level tables: every primary prefix that longer codes share gets one, as wide
            // as the longest of them (lengths ascend with the canonical code, so the last one wins)
            int p0 = -1;
            for (int l = root + 1; l <= kMaxBits; ++l) {
                if (!t.count[l]) continue;
                const int lo = t.first[l] >> (l - root), hi = (t.first[l] + t.count[l] - 1) >> (l - root);
                if (p0 < 0) p0 = lo;
                for (int p = lo; p <= hi; ++p) table[rev_bits((uint32_t)p, root)] = (uint32_t)(l - root);
            }
            int alloc = 1 << root;
            for (int p = p0; p >= 0 && p < (1 << root) && !err; ++p) {
                const uint32_t r = rev_bits((uint32_t)p, root), k = table[r];
                if (!k) continue;
                if (alloc + (1 << k) > cap) {
                    err = PCABI_INFLATE_E_CODE;
                    table[r] = 0;
                } else {
                    table[r] = entry((uint32_t)root, T_SUB, k, (uint32_t)alloc);
                    alloc += 1 << k;
                }
            }
            for (int s = 0; s < nsym; ++s)
                if (len[s]) t.code[s] = t.first[len[s]]++;
        }
        t.err = err;
    }
    par.sync();
    const int err = t.err;
    if (!err) {
        for (int s = lane; s < nsym; s += nl) {
            const int l = len[s];
            if (!l) continue;
            const uint32_t c = t.code[s];
            if (l <= root) {
                const uint32_t e = sym_entry(kind, s, (uint32_t)l);
                for (uint32_t j = rev_bits(c, l); j < (1u << root); j += 1u << l) table[j] = e;
            } else {
                const int low = l - root;
                const uint32_t sub = table[rev_bits(c >> low, root)], k = e_extra(sub), off = e_val(sub);
                const uint32_t e = sym_entry(kind, s, (uint32_t)low);
                for (uint32_t j = rev_bits(c & ((1u << low) - 1u), low); j < (1u << k); j += 1u << low) table[off + j] = e;
            }
        }
    }
    par.sync();
    return err;
}

// ---- bit reader, bounded to [p, p + n) ---------------------------------------------------------
struct Bits {
    const uint8_t *p;
    uint32_t n, pos;    // pos: next byte to fetch (a member is far below 4 GiB)
    uint64_t buf;       // the low cnt bits are the stream's next bits; bits above them are zero or
    int cnt;            // bits the stream really holds there (a wide fetch brings a partial byte)
};

PCABI_HD PCABI_INL inline void refill(Bits &b) {
    if (b.pos + 8 <= b.n) {   // wide fetch, stays inside the member
        uint64_t w;
        memcpy(&w, b.p + b.pos, 8);
        b.buf |= w << b.cnt;
        const int adv = (63 - b.cnt) >> 3;
        b.pos += (uint32_t)adv;
        b.cnt += adv * 8;
    } else {
        while (b.cnt <= 56 && b.pos < b.n) {
            b.buf |= (uint64_t)b.p[b.pos++] << b.cnt;
            b.cnt += 8;
        }
    }
}
PCABI_HD PCABI_INL inline void drop(Bits &b, int k) {
    b.buf >>= k;
    b.cnt -= k;
}
// k <= 16 bits into *v; false when the member holds fewer
PCABI_HD PCABI_INL inline bool take(Bits &b, int k, uint32_t *v) {
    if (b.cnt < k) {
        refill(b);
        if (b.cnt < k) return false;
    }
    *v = (uint32_t)(b.buf & ((1ull << k) - 1ull));
    drop(b, k);
    return true;
}

// One symbol of a two-level table. The lookup may index with bits past the member's end (zeros);
// the entry found is used only when the member holds all the bits it drops.
// Returns 0 and the entry, or a status.
PCABI_HD PCABI_INL inline int decode_sym(Bits &b, const uint32_t *table, int root, uint32_t *out) {
    uint32_t e = table[b.buf & ((1u << root) - 1u)];
    if (e_type(e) == T_SUB) {
        if (b.cnt < root) return PCABI_INFLATE_E_INPUT;
        drop(b, root);
        e = table[e_val(e) + (uint32_t)(b.buf & ((1u << e_extra(e)) - 1u))];
    }
    const int nb = (int)e_bits(e);
    if (nb == 0) return b.cnt < 1 ? PCABI_INFLATE_E_INPUT : PCABI_INFLATE_E_CODE;
    if (b.cnt < nb) return PCABI_INFLATE_E_INPUT;
    drop(b, nb);
    *out = e;
    return 0;
}

// order in which the code-length-code lengths are sent (16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1
// 15), five bits each in two words so that the lookup needs no table in memory
PCABI_HD PCABI_INL inline int cl_order(int i) {
    return (int)((i < 12 ? 0x22caa324e804a30ull >> (5 * i) : 0x3c2e1346cull >> (5 * (i - 12))) & 31u);
}

// the dynamic block's header after BTYPE: the literal/length lengths t.len[0, *n_lit) and the
// distance lengths after them
template <class Par>
PCABI_HD PCABI_INL inline int read_dynamic(Par &par, Tables &t, Bits &b, int *n_lit, int *n_dist) {
    uint32_t hlit, hdist, hclen;
    if (!take(b, 5, &hlit) || !take(b, 5, &hdist) || !take(b, 4, &hclen)) return PCABI_INFLATE_E_INPUT;
    const int nlit = (int)hlit + 257, ndist = (int)hdist + 1, ncl = (int)hclen + 4;
    if (nlit > 286 || ndist > 30) return PCABI_INFLATE_E_HEADER;
    // the 3-bit lengths: every lane reads them, one writes
    par.sync();   // nobody still reads t.len of the block before
    for (int i = 0; i < 19; ++i) {
        uint32_t v = 0;
        if (i < ncl && !take(b, 3, &v)) return PCABI_INFLATE_E_INPUT;
        if (par.lane() == 0) t.len[cl_order(i)] = (uint8_t)v;
    }
    par.sync();
    if (int rc = build_table(par, t, t.len, 19, kClRoot, t.cl, kClTable, K_CL)) return rc;
    // HLIT + HDIST lengths, one sequence
    const int total = nlit + ndist;
    int i = 0;
    uint32_t prev = 0;
    while (i < total) {
        if (b.cnt < 16) refill(b);
        uint32_t e;
        if (int rc = decode_sym(b, t.cl, kClRoot, &e)) return rc;
        const uint32_t s = e_val(e);
        uint32_t rep = 1, v = s, x = 0;
        if (s == 16) {
            if (i == 0) return PCABI_INFLATE_E_CODE;
            if (!take(b, 2, &x)) return PCABI_INFLATE_E_INPUT;
            rep = 3 + x;
            v = prev;
        } else if (s == 17) {
            if (!take(b, 3, &x)) return PCABI_INFLATE_E_INPUT;
            rep = 3 + x;
            v = 0;
        } else if (s == 18) {
            if (!take(b, 7, &x)) return PCABI_INFLATE_E_INPUT;
            rep = 11 + x;
            v = 0;
        }
        if (i + (int)rep > total) return PCABI_INFLATE_E_CODE;
        if (par.lane() == 0)
            for (uint32_t k = 0; k < rep; ++k) t.len[i + (int)k] = (uint8_t)v;
        i += (int)rep;
        prev = v;
    }
    par.sync();
    if (t.len[256] == 0) return PCABI_INFLATE_E_CODE;   // no end-of-block code
    *n_lit = nlit;
    *n_dist = ndist;
    return 0;
}

// the fixed code's lengths, in the same layout
template <class Par>
PCABI_HD PCABI_INL inline void fixed_lengths(Par &par, Tables &t) {
    par.sync();
    for (int s = par.lane(); s < kMaxLit + kMaxDist; s += par.lanes())
        t.len[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
    par.sync();
}

// How much history lies before a sink's position 0: what its history() says (0, or 32768 for a sink
// that stands for an unknown window), 0 for a sink without one.
template <class Sink>
PCABI_HD PCABI_INL inline auto sink_history(const Sink &s, int) -> decltype((uint32_t)s.history()) {
    return (uint32_t)s.history();
}
template <class Sink>
PCABI_HD PCABI_INL inline uint32_t sink_history(const Sink &, long) {
    return 0;
}

// the stop rule of a decoder that runs to the final block
struct NeverStop {
    PCABI_HD bool operator()(int64_t) const { return false; }
};

// a bit reader over [z, z + n) that stands on bit `bit` (0 <= bit <= 8 n)
PCABI_HD PCABI_INL inline Bits bits_at(const uint8_t *z, uint32_t n, int64_t bit) {
    Bits b{z, n, (uint32_t)(bit >> 3), 0, 0};
    const int k = (int)(bit & 7);
    if (k && b.pos < n) {
        b.buf = (uint64_t)(z[b.pos++] >> k);
        b.cnt = 8 - k;
    }
    return b;
}
// the bit the reader stands on
PCABI_HD PCABI_INL inline int64_t bit_pos(const Bits &b) { return 8 * (int64_t)b.pos - b.cnt; }

// Deflate blocks from the bit b stands on into the sink, at most limit bytes, until a final block
// has been decoded or stop(bit position) holds at a block boundary (asked after every block that is
// not final). *produced = bytes decoded, *end_bit = the bit after the last block decoded,
// *was_final = that block was a final one. A match may reach sink_history() bytes before the
// sink's position 0. Every loop below drops at least one input bit per turn or returns.
template <class Par, class Sink, class Stop>
PCABI_HD PCABI_INL inline int inflate_blocks(Par &par, Sink &sink, Tables &t, Bits &b, uint32_t limit, const Stop &stop,
                                   uint32_t *produced, int64_t *end_bit, int *was_final) {
    const uint8_t *z = b.p;
    const uint32_t hist = sink_history(sink, 0);
    uint32_t opos = 0;
    *produced = 0;
    *end_bit = 0;
    *was_final = 0;
    if (par.lane() == 0) t.fixed_built = 0;
    par.sync();
    for (;;) {
        uint32_t hdr;
        if (!take(b, 3, &hdr)) return PCABI_INFLATE_E_INPUT;
        const uint32_t final_block = hdr & 1u, btype = hdr >> 1;
        if (btype == 3) return PCABI_INFLATE_E_HEADER;
        if (btype == 0) {
            drop(b, b.cnt & 7);
            uint32_t len, nlen;
            if (!take(b, 16, &len) || !take(b, 16, &nlen)) return PCABI_INFLATE_E_INPUT;
            if ((len ^ 0xffffu) != nlen) return PCABI_INFLATE_E_HEADER;
            const uint32_t src = b.pos - (uint32_t)(b.cnt >> 3);   // the byte the bit cursor stands on
            if (len > b.n - src) return PCABI_INFLATE_E_INPUT;
            if (len > limit - opos) return PCABI_INFLATE_E_OUTPUT;
            sink.store(opos, z + src, len);
            opos += len;
            b.pos = src + len;
            b.buf = 0;
            b.cnt = 0;
        } else {
            int nlit = kMaxLit, ndist = kMaxDist;
            const bool have = btype == 1 && t.fixed_built;   // a run of fixed blocks builds once
            if (btype == 1) {
                if (!have) fixed_lengths(par, t);
            } else if (int rc = read_dynamic(par, t, b, &nlit, &ndist)) {
                return rc;
            }
            if (!have) {
#if defined(__HIPCC__)
#pragma unroll 1
#endif
                for (int k = 0; k < 2; ++k)
                    if (int rc = build_table(par, t, k ? t.len + nlit : t.len, k ? ndist : nlit, k ? kDistRoot : kLitRoot,
                                             k ? t.dist : t.lit, k ? kDistTable : kLitTable, k ? K_DIST : K_LIT))
                        return rc;
                par.sync();
                if (par.lane() == 0) t.fixed_built = btype == 1;
                par.sync();
            }
            for (;;) {
                if (b.cnt < 48) refill(b);   // 15 + 5 + 15 + 13 bits at the most per turn
                uint32_t e;
                if (int rc = decode_sym(b, t.lit, kLitRoot, &e)) return rc;
                const uint32_t type = e_type(e);
                if (type == T_LIT) {
                    if (opos >= limit) return PCABI_INFLATE_E_OUTPUT;
                    sink.put(opos++, (uint8_t)e_val(e));
                    continue;
                }
                if (type == T_EOB) break;
                if (type != T_LEN) return PCABI_INFLATE_E_CODE;
                uint32_t x = 0;
                if (!take(b, (int)e_extra(e), &x)) return PCABI_INFLATE_E_INPUT;
                const uint32_t len = e_val(e) + x;
                uint32_t d;
                if (int rc = decode_sym(b, t.dist, kDistRoot, &d)) return rc;
                if (e_type(d) != T_DIST) return PCABI_INFLATE_E_CODE;
                if (!take(b, (int)e_extra(d), &x)) return PCABI_INFLATE_E_INPUT;
                const uint32_t dist = e_val(d) + x;
                if (dist > opos && dist - opos > hist) return PCABI_INFLATE_E_DIST;
                if (len > limit - opos) return PCABI_INFLATE_E_OUTPUT;
                sink.copy(opos, dist, len);
                opos += len;
            }
        }
        if (final_block) {
            *was_final = 1;
            break;
        }
        if (stop(bit_pos(b))) break;
    }
    *produced = opos;
    *end_bit = bit_pos(b);
    return 0;
}

// The deflate stream in [z, z + n) into the sink, at most limit bytes. *produced = bytes decoded,
// *used = input bytes consumed (whole bytes: the final block's padding counts).
template <class Par, class Sink>
PCABI_HD PCABI_INL inline int inflate_raw(Par &par, Sink &sink, Tables &t, const uint8_t *z, int64_t n, uint32_t limit,
                                uint32_t *produced, int64_t *used) {
    Bits b{z, (uint32_t)n, 0, 0, 0};
    int64_t end_bit = 0;
    int was_final = 0;
    *used = 0;
    if (int rc = inflate_blocks(par, sink, t, b, limit, NeverStop(), produced, &end_bit, &was_final)) {
        *produced = 0;
        return rc;
    }
    *used = (int64_t)(b.pos - (uint32_t)(b.cnt >> 3));
    return 0;
}

PCABI_HD PCABI_INL inline uint32_t le32(const uint8_t *p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// One gzip member z[0, n) (RFC 1952: FEXTRA, FNAME, FCOMMENT, FHCRC skipped) into the sink, whose
// room is cap bytes. Checks the trailer's ISIZE and CRC-32. *out_len = ISIZE on success.
template <class Par, class Sink>
PCABI_HD PCABI_INL inline int inflate_member(Par &par, Sink &sink, Tables &t, const uint8_t *z, int64_t n, uint32_t cap,
                                   uint32_t *out_len) {
    *out_len = 0;
    if (n < kMinMember || n > 0x7fffffff || z[0] != 0x1f || z[1] != 0x8b || z[2] != 8 || (z[3] & 0xe0)) return PCABI_INFLATE_E_HEADER;
    const int flg = z[3];
    const int64_t end = n - 8;   // the trailer
    int64_t h = 10;
    if (flg & 4) {
        if (h + 2 > end) return PCABI_INFLATE_E_HEADER;
        h += 2 + ((int64_t)z[h] | (int64_t)z[h + 1] << 8);
        if (h > end) return PCABI_INFLATE_E_HEADER;
    }
    for (int f = 8; f <= 16; f <<= 1) {   // FNAME, FCOMMENT: zero-terminated
        if (!(flg & f)) continue;
        while (h < end && z[h]) ++h;
        if (h >= end) return PCABI_INFLATE_E_HEADER;
        ++h;
    }
    if (flg & 2) {   // FHCRC: the low 16 bits of the header's CRC-32
        if (h + 2 > end) return PCABI_INFLATE_E_HEADER;
        uint32_t c = 0xffffffffu;
        for (int64_t i = 0; i < h; ++i) {
            c ^= z[i];
            for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
        }
        if (((c ^ 0xffffffffu) & 0xffffu) != ((uint32_t)z[h] | (uint32_t)z[h + 1] << 8)) return PCABI_INFLATE_E_HEADER;
        h += 2;
    }
    const uint32_t crc = le32(z + end), isize = le32(z + end + 4);
    if (isize > cap) return PCABI_INFLATE_E_OUTPUT;
    uint32_t produced = 0;
    int64_t used = 0;
    if (int rc = inflate_raw(par, sink, t, z + h, end - h, isize, &produced, &used)) return rc;
    if (produced < isize) return PCABI_INFLATE_E_LENGTH;
    if (used != end - h) return PCABI_INFLATE_E_HEADER;   // bytes between the stream and the trailer
    if (sink.crc(isize) != crc) return PCABI_INFLATE_E_CRC;
    *out_len = isize;
    return 0;
}

// ---- the member index (host) -------------------------------------------------------------------
// Walks the members of z[0, n) by their headers' BC subfields (BGZF). m members: in_off[0..m]
// (in_off[m] = n) and out_off[0..m] (prefix sums of ISIZE) are written when m + 1 <= cap. Returns m,
// 0 when some member is not indexable (no BC subfield, CM != 8, ISIZE > 65536), PCABI_E_PARSE when
// the chain is broken or runs past n.
inline int64_t gunzip_index(const uint8_t *z, int64_t n, int64_t *in_off, int64_t *out_off, int64_t cap) {
    for (int pass = 0; pass < 2; ++pass) {
        int64_t pos = 0, m = 0, total = 0;
        while (pos < n) {
            if (n - pos < kMinMember || z[pos] != 0x1f || z[pos + 1] != 0x8b) return PCABI_E_PARSE;
            if (z[pos + 2] != 8 || !(z[pos + 3] & 4)) return 0;
            const int64_t xlen = (int64_t)z[pos + 10] | (int64_t)z[pos + 11] << 8, x0 = pos + 12, x1 = x0 + xlen;
            if (x1 + 8 > n) return PCABI_E_PARSE;
            int64_t bsize = -1;
            for (int64_t q = x0; q < x1;) {
                if (q + 4 > x1) return PCABI_E_PARSE;
                const int64_t slen = (int64_t)z[q + 2] | (int64_t)z[q + 3] << 8;
                if (q + 4 + slen > x1) return PCABI_E_PARSE;
                if (z[q] == 'B' && z[q + 1] == 'C' && slen == 2 && bsize < 0) bsize = (int64_t)z[q + 4] | (int64_t)z[q + 5] << 8;
                q += 4 + slen;
            }
            if (bsize < 0) return 0;
            const int64_t next = pos + bsize + 1;
            if (next > n || next < x1 + 8) return PCABI_E_PARSE;
            const uint32_t isize = le32(z + next - 4);
            if (isize > (uint32_t)kMemberMax) return 0;
            if (pass == 1) {
                in_off[m] = pos;
                out_off[m] = total;
            }
            total += isize;
            pos = next;
            ++m;
        }
        if (pass == 1) {
            in_off[m] = n;
            out_off[m] = total;
        }
        if (pass == 0 && (m == 0 || m + 1 > cap || !in_off || !out_off)) return m;
        if (pass == 1) return m;
    }
    return 0;
}

// ---- the serial policies (host build, and the reference the kernel's are read against) ---------
struct SerialPar {
    PCABI_HD int lane() const { return 0; }
    PCABI_HD int lanes() const { return 1; }
    PCABI_HD void sync() const {}
};

// ---- sinks of a decoder that starts inside a stream (pcabi_gzstream.h) --------------------------
// Symbols instead of bytes: a value below 256 is a byte; kMarker | j stands for byte j of the 32768
// bytes that precede the sink's position 0 (the window of whatever was decoded before, unknown
// while this decoder runs). ring holds the last 32768 symbols and is the LZ77 window, out (when not
// null) receives every symbol; matches copy symbols, so markers travel with them.
constexpr uint32_t kWindow = 32768;
constexpr uint16_t kMarker = 0x8000;

// ring[j] = the symbol at position j - 32768: the unknown window, as markers
template <class Par>
PCABI_HD PCABI_INL inline void marker_ring_init(Par &par, uint16_t *ring) {
    for (uint32_t j = (uint32_t)par.lane(); j < kWindow; j += (uint32_t)par.lanes()) ring[j] = (uint16_t)(kMarker | j);
    par.sync();
}

struct SerialMarkerSink {
    uint16_t *ring;   // kWindow symbols
    uint16_t *out;
    uint32_t hist;    // 0: nothing precedes position 0 (a member's start); kWindow: markers do
    PCABI_HD uint32_t history() const { return hist; }
    PCABI_HD void put(uint32_t pos, uint8_t c) {
        ring[pos & (kWindow - 1)] = c;
        out[pos] = c;
    }
    // a source may be written by this very copy (dist < len): ascending order reads it after
    PCABI_HD void copy(uint32_t pos, uint32_t dist, uint32_t len) {
        for (uint32_t i = 0; i < len; ++i) {
            const uint16_t s = ring[(pos + i - dist) & (kWindow - 1)];
            ring[(pos + i) & (kWindow - 1)] = s;
            out[pos + i] = s;
        }
    }
    PCABI_HD void store(uint32_t pos, const uint8_t *src, uint32_t len) {
        for (uint32_t i = 0; i < len; ++i) {
            ring[(pos + i) & (kWindow - 1)] = src[i];
            out[pos + i] = src[i];
        }
    }
};

// sizes only: a decoder over this sink writes nothing
struct CountSink {
    uint32_t hist;
    PCABI_HD uint32_t history() const { return hist; }
    PCABI_HD void put(uint32_t, uint8_t) const {}
    PCABI_HD void copy(uint32_t, uint32_t, uint32_t) const {}
    PCABI_HD void store(uint32_t, const uint8_t *, uint32_t) const {}
};

#if !defined(__HIPCC__)
}  // namespace pcabi_inflate
#include "pcabi_crc.h"
namespace pcabi_inflate {
struct SerialSink {
    uint8_t *out;
    void put(uint32_t pos, uint8_t c) { out[pos] = c; }
    void copy(uint32_t pos, uint32_t dist, uint32_t len) {
        for (uint32_t i = 0; i < len; ++i) out[pos + i] = out[pos + i - dist];
    }
    void store(uint32_t pos, const uint8_t *src, uint32_t len) {
        if (len) memcpy(out + pos, src, len);
    }
    uint32_t crc(uint32_t len) const {
        static const pcabi_crc::CrcTables tab = pcabi_crc::make_tables();
        uint32_t c = 0xffffffffu;
        for (uint32_t i = 0; i < len; ++i) c = tab.byte[(c ^ out[i]) & 0xff] ^ (c >> 8);
        return c ^ 0xffffffffu;
    }
};
#endif

}  // namespace pcabi_inflate
