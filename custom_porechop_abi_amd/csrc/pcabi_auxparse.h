// pcabi_auxparse.h -- SAM tags read from FASTQ / FASTA headers: the tab-separated TG:T:value fields of
// a header parsed into a chain of BAM aux bytes (include/pcabi.h "SAM tags read from FASTQ / FASTA
// headers", which states the rule; pcabi_auxparse.hip, pcabi_io.cpp; DESIGN.md "Tags read from text
// headers"). pcabi_auxtext.h run backwards. Nothing here is device-only: the kernels, the host build
// (device < 0) and the CPU tests (tests/auxparse_fuzz_main.cpp builds it alone) run the same code.
//
// Two readings of the rule stand side by side. parse() walks a header byte by byte (the host build).
// wave_parse() walks it the way a wave does, written against a Wave type that gives it ballot() over
// the 64 lanes: the kernels pass the hardware's ballot, the fuzz program one that plays the lanes in
// turn. The walk from field to field is uniform (every lane reads the same head); find_tab looks for
// the next tab 64 bytes a pass; a Z / H / A value goes 64 bytes a pass (value_end: one ballot for the
// tab, one for the bytes that are not allowed); an array goes 64 text bytes a pass (array_pass: a lane
// holds one byte, a ballot names the commas, a lane that holds a comma parses the element behind it,
// whose length it reads off the ballot; its index is the elements before the pass plus the commas
// below it, its store val + index * width; a pass that ends inside an element starts the next pass at
// that element's comma).
// Floats: the device checks the syntax (the field's length depends on it) and leaves a Fix -- where the
// text lies, how long it is, where the 4 bytes go; the host fills them with strtod (float_value).
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../../include/pcabi.h"

#ifndef PCABI_HD
#if defined(__HIPCC__)
#define PCABI_HD __host__ __device__
#else
#define PCABI_HD
#endif
#endif

namespace pcabi_auxparse {

constexpr int kWaveLanes = 64;
constexpr int kHead = 5;        // two name bytes, ':', the type letter, ':'
constexpr int kMaxInt = 11;     // a sign and ten digits
constexpr int kMaxFloat = 31;

// a float left to the host: text[text_off, text_off + len) of the blob -> out[out_off, out_off + 4)
struct Fix {
    int64_t text_off, out_off;
    int32_t len, reserved;
};
struct Counts {
    int64_t n_float, tags, left_out;
};

PCABI_HD inline bool alpha(uint8_t c) { return (uint8_t)((c | 0x20) - 'a') < 26; }
PCABI_HD inline bool digit(uint8_t c) { return (uint8_t)(c - '0') < 10; }
PCABI_HD inline bool hexdigit(uint8_t c) { return digit(c) || (uint8_t)((c | 0x20) - 'a') < 6; }
PCABI_HD inline bool printable(uint8_t c) { return c >= 0x20 && c <= 0x7E; }
PCABI_HD inline int width_of(uint8_t t) {
    return t == 'c' || t == 'C' ? 1 : t == 's' || t == 'S' ? 2 : t == 'i' || t == 'I' || t == 'f' ? 4 : 0;
}
// the five bytes TG:T: at f
PCABI_HD inline bool head_ok(const uint8_t *f) {
    const uint8_t t = f[3];
    return alpha(f[0]) && (alpha(f[1]) || digit(f[1])) && f[2] == ':' && f[4] == ':' &&
           (t == 'A' || t == 'i' || t == 'f' || t == 'Z' || t == 'H' || t == 'B');
}
// may byte c stand in a value of type A / Z / H
PCABI_HD inline bool byte_ok(uint8_t type, uint8_t c) { return type == 'H' ? hexdigit(c) : printable(c); }

// [-+]?[0-9]{1,10} at s[0, n): its value, and whether a '-' leads it
PCABI_HD inline bool int_scan(const uint8_t *s, int64_t n, int64_t *v, bool *minus) {
    if (n < 1 || n > kMaxInt) return false;
    *minus = s[0] == '-';
    const int k0 = s[0] == '-' || s[0] == '+' ? 1 : 0;
    if (n - k0 < 1 || n - k0 > 10) return false;
    int64_t m = 0;
    for (int k = k0; k < (int)n; ++k) {
        if (!digit(s[k])) return false;
        m = m * 10 + (s[k] - '0');
    }
    *v = *minus ? -m : m;
    return true;
}
// htslib's smallest type of a scalar; 0 outside -2^31 .. 2^32 - 1
PCABI_HD inline uint8_t int_type(int64_t v, bool minus) {
    if (minus) return v < -2147483648LL ? 0 : v >= -128 ? 'c' : v >= -32768 ? 's' : 'i';
    return v > 4294967295LL ? 0 : v <= 255 ? 'C' : v <= 65535 ? 'S' : 'I';
}
PCABI_HD inline bool in_range(uint8_t sub, int64_t v) {
    switch (sub) {
        case 'c': return v >= -128 && v <= 127;
        case 'C': return v >= 0 && v <= 255;
        case 's': return v >= -32768 && v <= 32767;
        case 'S': return v >= 0 && v <= 65535;
        case 'i': return v >= -2147483648LL && v <= 2147483647LL;
        case 'I': return v >= 0 && v <= 4294967295LL;
        default: return false;
    }
}
// SAM's float syntax at s[0, n), or [-+]?inf, [-+]?nan
PCABI_HD inline bool float_scan(const uint8_t *s, int64_t n) {
    if (n < 1 || n > kMaxFloat) return false;
    int k = s[0] == '-' || s[0] == '+' ? 1 : 0;
    const int m = (int)n;
    if (m - k == 3 && ((s[k] == 'i' && s[k + 1] == 'n' && s[k + 2] == 'f') || (s[k] == 'n' && s[k + 1] == 'a' && s[k + 2] == 'n')))
        return true;
    int d0 = 0, d1 = 0;
    bool dot = false;
    for (; k < m && digit(s[k]); ++k) ++d0;
    if (k < m && s[k] == '.') {
        dot = true;
        for (++k; k < m && digit(s[k]); ++k) ++d1;
    }
    if (dot ? d1 < 1 : d0 < 1) return false;
    if (k < m && (s[k] == 'e' || s[k] == 'E')) {
        ++k;
        if (k < m && (s[k] == '-' || s[k] == '+')) ++k;
        int de = 0;
        for (; k < m && digit(s[k]); ++k) ++de;
        if (de < 1) return false;
    }
    return k == m;
}
// C's (float)strtod of a text float_scan accepted. Host only.
inline float float_value(const uint8_t *s, int n) {
    char t[kMaxFloat + 1];
    memcpy(t, s, (size_t)n);
    t[n] = 0;
    return (float)strtod(t, nullptr);
}
// an array element of subtype sub at s[0, n): well-formed and inside the subtype's range; *v an integer's value
PCABI_HD inline bool elem_scan(uint8_t sub, const uint8_t *s, int64_t n, int64_t *v) {
    if (sub == 'f') return float_scan(s, n);
    bool minus = false;
    return int_scan(s, n, v, &minus) && in_range(sub, *v);
}

// dst[at] = c where that lies inside dst[0, room)
PCABI_HD inline void put(uint8_t *dst, int64_t room, int64_t at, uint8_t c) {
    if (at >= 0 && at < room) dst[at] = c;
}
// the low w bytes of v, little-endian, at dst[at, at + w)
PCABI_HD inline void int_put(uint8_t *dst, int64_t room, int64_t at, int64_t v, int w) {
    for (int k = 0; k < w; ++k) put(dst, room, at + k, (uint8_t)((uint64_t)v >> (8 * k)));
}
// slot k of the fix-up table, where k lies inside the part's own slots [lo, hi)
PCABI_HD inline void fix_put(Fix *fix, int64_t lo, int64_t hi, int64_t k, int64_t text_off, int64_t out_off, int64_t len) {
    if (fix && k >= lo && k < hi) fix[k] = Fix{text_off, out_off, (int32_t)len, 0};
}

// a table entry against the blob
PCABI_HD inline bool part_fits(const pcabi_auxparse_part &p, int64_t text_n) {
    return p.text_len >= 0 && p.text_off >= 0 && p.text_off <= text_n && p.text_len <= text_n - p.text_off;
}

// ---- the byte-wise walk (the host build) -------------------------------------------------------------
// One candidate field t[0, n) (no tab in it): the bytes it adds to the chain, or -1 when it is left
// out. dst != nullptr: they are written to dst[at, ...) as well (nothing outside dst[0, room)), floats by
// float_value; trusted: the plan left no field of this header out, so an array is stored in the sweep
// that checks it, otherwise it is checked first. *nf = its floats.
inline int64_t field(const uint8_t *t, int64_t n, uint8_t *dst, int64_t room, int64_t at, bool trusted, int64_t *nf) {
    *nf = 0;
    if (n < kHead || !head_ok(t)) return -1;
    const uint8_t type = t[3];
    const uint8_t *v = t + kHead;
    const int64_t vn = n - kHead;
    auto head = [&](uint8_t ty) {
        put(dst, room, at, t[0]), put(dst, room, at + 1, t[1]), put(dst, room, at + 2, ty);
    };
    auto fput = [&](int64_t to, const uint8_t *s, int64_t len) {
        const float x = float_value(s, (int)len);
        uint8_t b[4];
        memcpy(b, &x, 4);
        for (int k = 0; k < 4; ++k) put(dst, room, to + k, b[k]);
    };
    if (type == 'A' || type == 'Z' || type == 'H') {
        for (int64_t k = 0; k < vn; ++k)
            if (!byte_ok(type, v[k])) return -1;
        if (type == 'A' ? vn != 1 : type == 'H' && (vn & 1)) return -1;
        if (dst) {
            head(type);
            for (int64_t k = 0; k < vn; ++k) put(dst, room, at + 3 + k, v[k]);
            if (type != 'A') put(dst, room, at + 3 + vn, 0);
        }
        return type == 'A' ? 4 : 3 + vn + 1;
    }
    if (type == 'i') {
        int64_t x = 0;
        bool minus = false;
        const uint8_t ty = int_scan(v, vn, &x, &minus) ? int_type(x, minus) : 0;
        if (!ty) return -1;
        if (dst) head(ty), int_put(dst, room, at + 3, x, width_of(ty));
        return 3 + width_of(ty);
    }
    if (type == 'f') {
        if (!float_scan(v, vn)) return -1;
        *nf = 1;
        if (dst) head('f'), fput(at + 3, v, vn);
        return 7;
    }
    // B: the subtype letter, then ",element" zero or more times
    const int w = vn >= 1 ? width_of(v[0]) : 0;
    if (!w) return -1;
    const uint8_t sub = v[0];
    int64_t count = 0;
    for (int pass = dst && trusted ? 1 : 0; pass < (dst ? 2 : 1); ++pass) {   // check and count, then store
        count = 0;
        for (int64_t k = 1; k < vn;) {
            if (v[k] != ',') return -1;
            int64_t e = k + 1;
            while (e < vn && v[e] != ',') ++e;
            int64_t x = 0;
            if (!elem_scan(sub, v + k + 1, e - k - 1, &x)) return -1;
            if (pass == 1) {
                if (sub == 'f') fput(at + 8 + count * 4, v + k + 1, e - k - 1);
                else int_put(dst, room, at + 8 + count * w, x, w);
            }
            ++count;
            k = e;
        }
    }
    if (dst) head('B'), put(dst, room, at + 3, sub), int_put(dst, room, at + 4, count, 4);
    if (sub == 'f') *nf = count;
    return 8 + count * w;
}

// One header t[0, n): the chain's length. dst != nullptr: the chain is written to dst[0, room) as well
// (trusted: see field). *c is set: the floats the chain holds, the tags read, the fields left out.
inline int64_t parse(const uint8_t *t, int64_t n, uint8_t *dst, int64_t room, bool trusted, Counts *c) {
    Counts k{0, 0, 0};
    int64_t len = 0;
    const uint8_t *tab = n > 0 ? (const uint8_t *)memchr(t, '\t', (size_t)n) : nullptr;
    for (int64_t at = tab ? tab - t : n; at < n;) {
        int64_t e = at + 1;
        while (e < n && t[e] != '\t') ++e;
        int64_t nf = 0;
        const int64_t w = field(t + at + 1, e - at - 1, dst, room, len, trusted, &nf);
        if (w < 0) ++k.left_out;
        else len += w, ++k.tags, k.n_float += nf;
        at = e;
    }
    if (c) *c = k;
    return len;
}

// ---- the wave's walk ---------------------------------------------------------------------------------
// Wave: uint64_t ballot(f) -- bit l is f(l), for the 64 lanes l; each(f) -- f(l) for every lane.
PCABI_HD inline uint64_t below(int l) { return l >= 64 ? ~(uint64_t)0 : ((uint64_t)1 << l) - 1; }

// the first tab of t[from, n), or n
template <class Wave>
PCABI_HD inline int64_t find_tab(Wave &w, const uint8_t *t, int64_t n, int64_t from) {
    for (int64_t q = from; q < n; q += kWaveLanes) {
        const uint64_t tabs = w.ballot([&](int l) { return q + l < n && t[q + l] == '\t'; });
        if (tabs) return q + __builtin_ctzll(tabs);
    }
    return n;
}

// the end of the A / Z / H value that starts at v (the first tab, or n); *bad: a byte of it is not allowed
template <class Wave>
PCABI_HD inline int64_t value_end(Wave &w, const uint8_t *t, int64_t n, int64_t v, uint8_t type, bool *bad) {
    *bad = false;
    for (int64_t q = v; q < n; q += kWaveLanes) {
        const uint64_t tabs = w.ballot([&](int l) { return q + l < n && t[q + l] == '\t'; });
        const uint64_t ugly = w.ballot([&](int l) { return q + l < n && !byte_ok(type, t[q + l]); });
        if (tabs) {
            const int f = __builtin_ctzll(tabs);
            if (ugly & below(f)) *bad = true;
            return q + f;
        }
        if (ugly) *bad = true;
    }
    return n;
}

// The elements of an array of subtype sub whose text starts at q0 (behind the subtype letter). true: a
// well-formed array, *count its elements, *end the field's end. false: the field is left out, *end a
// place inside it. kStore: element k's integer goes to dst[val + k * width), a float's Fix to slot
// fix0 + k.
template <bool kStore, class Wave>
PCABI_HD inline bool array_pass(Wave &w, const uint8_t *t, int64_t n, int64_t q0, uint8_t sub, uint8_t *dst, int64_t room, int64_t val,
                                Fix *fix, int64_t fix_lo, int64_t fix_hi, int64_t fix0, int64_t text_base, int64_t out_base,
                                int64_t *count, int64_t *end) {
    const int wd = width_of(sub);
    int64_t q = q0, cnt = 0;
    for (;;) {   // q grows by at least one a pass and stops at n
        // cut: the first lane whose byte is a tab or lies past the end
        const uint64_t stops = w.ballot([&](int l) { return q + l >= n || t[q + l] == '\t'; });
        const int cut = stops ? __builtin_ctzll(stops) : kWaveLanes;
        const uint64_t commas = w.ballot([&](int l) { return q + l < n && t[q + l] == ','; }) & below(cut);
        *end = q;
        if (cut == 0) {   // (the first pass only: a later one starts at a comma) no elements
            *count = cnt;
            return true;
        }
        if (!(commas & 1)) return false;   // the text behind the subtype letter does not start with a comma
        const bool last = cut < kWaveLanes;
        const int top = 63 - __builtin_clzll(commas);
        if (!last && top == 0) return false;   // an element of 63 bytes or more
        // the elements that end inside this pass: all of them in the last pass, else all but the top one
        const uint64_t mine = last ? commas : commas & ~((uint64_t)1 << top);
        const uint64_t bad = w.ballot([&](int l) {
            if (!(mine >> l & 1)) return false;
            const uint64_t above = l >= 63 ? 0 : commas >> (l + 1);
            const int64_t elen = above ? __builtin_ctzll(above) : cut - l - 1;
            int64_t x = 0;
            const bool ok = elem_scan(sub, t + q + l + 1, elen, &x);
            if (kStore && ok) {
                const int64_t k = cnt + __builtin_popcountll(mine & below(l));
                if (sub == 'f') fix_put(fix, fix_lo, fix_hi, fix0 + k, text_base + q + l + 1, out_base + val + k * 4, elen);
                else int_put(dst, room, val + k * wd, x, wd);
            }
            return !ok;
        });
        if (bad) return false;
        cnt += __builtin_popcountll(mine);
        if (last) {
            *count = cnt;
            *end = q + cut;
            return true;
        }
        q += top;
    }
}

// One header t[0, n), walked by a wave: the chain's length, *c as parse() sets it. dst != nullptr: the
// chain goes to dst[0, room) as well, and the floats' Fix records to the slots [fix_lo, fix_hi) of fix
// (text_base / out_base: where t and dst lie in the blob and in the output). trusted: the plan found no
// field to leave out, so an array is stored in the pass that checks it; otherwise it is checked first.
template <class Wave>
PCABI_HD inline int64_t wave_parse(Wave &w, const uint8_t *t, int64_t n, uint8_t *dst, int64_t room, Fix *fix, int64_t fix_lo,
                                   int64_t fix_hi, int64_t text_base, int64_t out_base, bool trusted, Counts *c) {
    Counts k{0, 0, 0};
    int64_t len = 0;
    for (int64_t at = find_tab(w, t, n, 0); at < n;) {   // uniform: t[at] is a tab
        const int64_t f = at + 1, v = f + kHead;
        int64_t e = f, add = -1, nf = 0;
        // (a tab among the five head bytes fails head_ok)
        if (n - f < kHead || !head_ok(t + f)) {
            e = find_tab(w, t, n, f);
        } else if (t[f + 3] == 'A' || t[f + 3] == 'Z' || t[f + 3] == 'H') {
            const uint8_t type = t[f + 3];
            bool bad = false;
            e = value_end(w, t, n, v, type, &bad);
            const int64_t vn = e - v;
            if (!bad && (type == 'A' ? vn == 1 : type != 'H' || !(vn & 1))) {
                add = type == 'A' ? 4 : 3 + vn + 1;
                if (dst)
                    w.each([&](int l) {   // a byte a lane
                        if (l < 3) put(dst, room, len + l, l == 2 ? type : t[f + l]);
                        for (int64_t j = l; j < vn; j += kWaveLanes) put(dst, room, len + 3 + j, t[v + j]);
                        if (l == 0 && type != 'A') put(dst, room, len + 3 + vn, 0);
                    });
            }
        } else if (t[f + 3] == 'i') {
            e = find_tab(w, t, n, v);
            int64_t x = 0;
            bool minus = false;
            const uint8_t ty = int_scan(t + v, e - v, &x, &minus) ? int_type(x, minus) : 0;
            if (ty) {
                add = 3 + width_of(ty);
                if (dst)
                    w.each([&](int l) {
                        if (l == 0) put(dst, room, len, t[f]), put(dst, room, len + 1, t[f + 1]), put(dst, room, len + 2, ty),
                                    int_put(dst, room, len + 3, x, width_of(ty));
                    });
            }
        } else if (t[f + 3] == 'f') {
            e = find_tab(w, t, n, v);
            if (float_scan(t + v, e - v)) {
                add = 7, nf = 1;
                if (dst)
                    w.each([&](int l) {
                        if (l == 0) {
                            put(dst, room, len, t[f]), put(dst, room, len + 1, t[f + 1]), put(dst, room, len + 2, 'f');
                            fix_put(fix, fix_lo, fix_hi, fix_lo + k.n_float, text_base + v, out_base + len + 3, e - v);
                        }
                    });
            }
        } else {   // B
            const uint8_t sub = v < n ? t[v] : 0;
            const int wd = width_of(sub);   // (0 for a tab)
            int64_t count = 0;
            bool ok = wd != 0;
            e = v;
            if (ok && !(dst && trusted))
                ok = array_pass<false>(w, t, n, v + 1, sub, nullptr, 0, 0, nullptr, 0, 0, 0, 0, 0, &count, &e);
            if (ok && dst)
                ok = array_pass<true>(w, t, n, v + 1, sub, dst, room, len + 8, fix, fix_lo, fix_hi, fix_lo + k.n_float, text_base,
                                      out_base, &count, &e);
            if (!ok) {
                e = find_tab(w, t, n, e);
            } else {
                add = 8 + count * wd, nf = sub == 'f' ? count : 0;
                if (dst)
                    w.each([&](int l) {
                        if (l == 0) {
                            put(dst, room, len, t[f]), put(dst, room, len + 1, t[f + 1]), put(dst, room, len + 2, 'B');
                            put(dst, room, len + 3, sub), int_put(dst, room, len + 4, count, 4);
                        }
                    });
            }
        }
        if (add < 0) ++k.left_out;
        else len += add, ++k.tags, k.n_float += nf;
        at = e;
    }
    if (c) *c = k;
    return len;
}

}  // namespace pcabi_auxparse
