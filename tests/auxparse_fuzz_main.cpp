// auxparse_fuzz_main.cpp -- csrc/pcabi_auxparse.h alone, as a program of its own for
// -fsanitize=address,undefined (tests/test_auxparse_cpu.py builds and runs it): random and truncated headers
// in heap blocks of exactly their size, the chains in blocks of exactly the planned length, so that a
// load or a store one byte outside is a report. The wave's walk (wave_parse) runs against a Wave that plays
// the 64 lanes of every ballot in turn, and must give what the byte-wise parse() gives: the length, the
// three counts and, with its fix-ups filled, every byte -- checked first (any part), stored in the pass that
// checks (a part without left-out fields), and with too little room (nothing behind the room is written).
// usage: auxparse_fuzz <seed> <rounds>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../custom_porechop_abi_amd/csrc/pcabi_auxparse.h"

using namespace pcabi_auxparse;

namespace {

struct PlayedWave {
    template <class F>
    uint64_t ballot(F f) {
        uint64_t m = 0;
        for (int l = 0; l < kWaveLanes; ++l)
            if (f(l)) m |= (uint64_t)1 << l;
        return m;
    }
    template <class F>
    void each(F f) {
        for (int l = 0; l < kWaveLanes; ++l) f(l);
    }
};

std::mt19937_64 rng;
int64_t pick(int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); }

std::string number(char sub) {
    switch (pick(0, 9)) {
        case 0: return std::to_string(pick(-140, 300));
        case 1: return std::to_string(pick(-40000, 70000));
        case 2: return std::to_string(pick(-2147483650LL, 4294967298LL));
        case 3: return "+" + std::to_string(pick(0, 99999));
        case 4: return std::string((size_t)pick(1, 12), (char)('0' + pick(0, 9)));
        case 5: return "-0";
        default: break;
    }
    if (sub == 'c') return std::to_string(pick(-128, 127));
    if (sub == 's') return std::to_string(pick(-32768, 32767));
    if (sub == 'S') return std::to_string(pick(0, 65535));
    if (sub == 'i') return std::to_string(pick(-2147483648LL, 2147483647LL));
    if (sub == 'I') return std::to_string(pick(0, 4294967295LL));
    return std::to_string(pick(0, 255));
}
std::string real() {
    static const char *odd[] = {"inf", "-inf", "+inf", "nan", "-nan", ".5", "5.", "1e", "1e+", "-.5e-3", "1.5.2", "", "+", "e5", "0x10",
                                "1e400", "-1e-400", "3.4028236e38", "0.1000000000000000055511151231257", "12345678901234567890123456789012"};
    if (pick(0, 3) == 0) return odd[pick(0, (int64_t)(sizeof odd / sizeof *odd) - 1)];
    char b[64];
    snprintf(b, sizeof b, pick(0, 1) ? "%g" : "%.9e", (double)pick(-1000000, 1000000) / (double)pick(1, 100000));
    return b;
}
std::string array(char sub, int64_t n) {
    std::string s(1, sub);
    for (int64_t k = 0; k < n; ++k) s += "," + (sub == 'f' ? real() : pick(0, 40) ? number(sub).substr(0, 11) : number('x'));
    return s;
}
std::string field() {
    static const char subs[] = "cCsSiIf";
    static const char *names[] = {"mv", "ML", "MM", "ts", "X1", "a9", "qs", "ns", "1X", "x"};
    std::string f = names[pick(0, 9)];
    const int kind = (int)pick(0, 11);
    auto text = [](int64_t n, bool hex) {
        std::string s;
        for (int64_t k = 0; k < n; ++k) s += hex ? "0123456789abcdefABCDEF"[pick(0, 21)] : (char)pick(0x20, 0x7E);
        return s;
    };
    switch (kind) {
        case 0: return f + ":A:" + text(pick(0, 2), false);
        case 1: return f + ":i:" + number('x');
        case 2: return f + ":f:" + real();
        case 3: return f + ":Z:" + text(pick(0, 3) ? pick(0, 70) : pick(60, 200), false);
        case 4: return f + ":H:" + text(pick(0, 3) ? 2 * pick(0, 40) : pick(0, 130), true);
        case 5: return f + ":Z:" + text(pick(0, 70), false) + (char)pick(0x7F, 0xFF) + text(pick(0, 70), false);
        case 6: return f + ":Q:" + text(pick(0, 5), false);
        case 7: return text(pick(0, 8), false);
        default: break;
    }
    const char sub = pick(0, 20) ? subs[pick(0, 6)] : 'q';
    // move tables of one-digit elements, so that the pass boundary falls on every position
    if (kind == 8) {
        std::string s = f + ":B:c";
        for (int64_t k = pick(0, 400); k > 0; --k) s += pick(0, 1) ? ",0" : ",1";
        return s;
    }
    static const int64_t lens[] = {0, 1, 2, 5, 6, 31, 32, 63, 64, 65, 127, 128, 129, 300};
    std::string s = f + ":B:" + array(sub, lens[pick(0, 13)]);
    if (pick(0, 15) == 0) s += ",";
    if (pick(0, 15) == 0) s.insert((size_t)pick(0, (int64_t)s.size()), ",");
    return s;
}
std::string header() {
    std::string h;
    const int64_t nm = pick(0, 70);
    for (int64_t k = 0; k < nm && pick(0, 9); ++k) h += (char)pick(0x20, 0x7E);
    for (int64_t k = pick(0, 6); k > 0; --k) h += "\t" + field();
    if (pick(0, 9) == 0) h += "\t";
    if (pick(0, 9) == 0 && !h.empty()) h.resize((size_t)pick(0, (int64_t)h.size()));   // truncated anywhere
    if (pick(0, 19) == 0 && !h.empty()) h[(size_t)pick(0, (int64_t)h.size() - 1)] = (char)pick(0, 255);
    return h;
}

int fails = 0;
int64_t seen_tags = 0, seen_left_out = 0, seen_floats = 0, seen_bytes = 0;
void fail(const char *what, const std::string &h) {
    if (++fails < 10) {
        fprintf(stderr, "FAIL %s: header of %zu bytes:", what, h.size());
        for (size_t k = 0; k < h.size() && k < 300; ++k) fprintf(stderr, h[k] >= 0x20 && h[k] < 0x7F ? "%c" : "\\x%02x", (unsigned char)h[k]);
        fprintf(stderr, "\n");
    }
}

// the wave's chain of text[0, n) in a block of exactly `room` bytes, its fix-ups filled
bool wave_chain(const uint8_t *text, int64_t n, int64_t room, int64_t n_float, bool trusted, std::vector<uint8_t> *chain, Counts *c) {
    uint8_t *dst = (uint8_t *)malloc((size_t)room + 1);   // (+ 1: a block of no bytes is a block all the same)
    memset(dst, 0xEE, (size_t)room);
    Fix *fix = (Fix *)malloc(sizeof(Fix) * (size_t)(n_float + 1));
    for (int64_t k = 0; k < n_float; ++k) fix[k] = Fix{-1, -1, 0, 0};
    PlayedWave w;
    wave_parse(w, text, n, dst, room, fix, 0, n_float, 0, 0, trusted, c);
    bool ok = true;
    for (int64_t k = 0; k < n_float; ++k) {
        const Fix &f = fix[k];
        if (f.out_off + 4 > room) continue;   // its place lies behind the room: the record may or may not stand
        if (f.len < 1 || f.len > kMaxFloat || f.text_off < 0 || f.text_off + f.len > n || f.out_off < 0 || !float_scan(text + f.text_off, f.len)) {
            ok = false;
            continue;
        }
        const float x = float_value(text + f.text_off, f.len);
        memcpy(dst + f.out_off, &x, 4);
    }
    chain->assign(dst, dst + room);
    free(dst);
    free(fix);
    return ok;
}

void round_of(const std::string &h) {
    const int64_t n = (int64_t)h.size();
    uint8_t *text = (uint8_t *)malloc((size_t)n + 1);
    memcpy(text, h.data(), (size_t)n);
    uint8_t *exact = (uint8_t *)realloc(text, (size_t)(n > 0 ? n : 1));   // exactly its size
    text = exact ? exact : text;
    Counts a{0, 0, 0}, b{0, 0, 0};
    const int64_t len = parse(text, n, nullptr, 0, false, &a);
    PlayedWave w;
    const int64_t wl = wave_parse(w, text, n, nullptr, 0, nullptr, 0, 0, 0, 0, false, &b);
    seen_tags += a.tags, seen_left_out += a.left_out, seen_floats += a.n_float, seen_bytes += len;
    if (len != wl || a.n_float != b.n_float || a.tags != b.tags || a.left_out != b.left_out) fail("plan", h);
    std::vector<uint8_t> want((size_t)len, 0xEE), got;
    Counts c{0, 0, 0};
    if (parse(text, n, want.data(), len, false, &c) != len) fail("parse twice", h);
    if (a.left_out == 0) {   // stored in the sweep that checks
        std::vector<uint8_t> one((size_t)len, 0xEE);
        if (parse(text, n, one.data(), len, true, &c) != len || one != want) fail("parse trusted", h);
    }
    if (!wave_chain(text, n, len, a.n_float, false, &got, &c) || got != want) fail("checked first", h);
    if (a.left_out == 0 && (!wave_chain(text, n, len, a.n_float, true, &got, &c) || got != want)) fail("trusted", h);
    if (len > 0) {   // too little room: a prefix, and nothing behind it
        const int64_t room = pick(0, len - 1);
        wave_chain(text, n, room, a.n_float, a.left_out == 0, &got, &c);
        std::vector<uint8_t> host((size_t)room, 0xEE);
        parse(text, n, host.data(), room, a.left_out == 0, nullptr);
        // (the floats behind the room are not filled on either side)
        if (a.n_float == 0 && (got != host || !std::equal(host.begin(), host.end(), want.begin()))) fail("short room", h);
    }
    free(text);
}

}  // namespace

int main(int argc, char **argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int64_t rounds = argc > 2 ? atoll(argv[2]) : 1000;
    rng.seed(seed);
    // the shapes a wave can go wrong at, then random headers
    for (int64_t pad = 0; pad < 140; ++pad) {
        const std::string name((size_t)pad, 'n');
        round_of(name + "\tXZ:Z:" + std::string((size_t)(130 - (pad % 131)), 'z') + "\tNM:i:5");
        round_of(name + "\tmv:B:c,6" + array('c', 70).substr(1) + "\tts:i:-77");
        round_of(name + "\tXB:B:i,-2147483648,2147483647,-2147483648,2147483647,-2147483648,2147483647,-2147483648\tde:f:0.25");
        round_of(name + "\tXF:B:f,1,-0.5,inf,1e-3,12345.678e3,nan\tXA:A:x\tXB:B:s");
    }
    for (int64_t r = 0; r < rounds; ++r) round_of(header());
    printf("rounds %lld fails %d tags %lld left_out %lld floats %lld bytes %lld\n", (long long)rounds, fails, (long long)seen_tags,
           (long long)seen_left_out, (long long)seen_floats, (long long)seen_bytes);
    return fails ? 1 : 0;
}
